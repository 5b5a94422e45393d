// mrt_inst.h — which pt_megakernel instantiation serves a scene: the one host-side statement of the rule.  Plain C++ with no HIP
// dependency, so that the launchers (mrt_kernels.hip, mrt_denoise.hip), mrt_api.cpp and the x86 builds of tests/emu all call the
// same function.
#pragma once
#include "mrt_trace.h"

namespace mrt {

// The FEAT template argument of the pt_megakernel instantiation that serves a scene with feature set `features` in a
// launch shape: the 64- and 256-thread shapes with the scene in LDS exist for every plain feature set; the large
// shapes (512 / 1024 threads, scene through L2) with and without the triangle / mesh code; the instance-BVH kernels in
// four feature sets per shape -- plain primitives without / with lights (sphere and plane crowds), everything but
// triangles and meshes, everything -- of which the smallest covering one runs (a Minecraft-shaped scene without the
// triangle / mesh code: 113 VGPRs and no scratch instead of 128 + 72 B, +15 %).  Scenes with per-corner attributes (F_VATTR)
// always take the full set, and so do scenes with an environment texture or a filtered texture (F_ENV, which comes with
// F_VATTR).  Reported in mrt_stats.kernel_features.
inline u32 pt_instantiation(u32 block_threads, bool scene_in_lds, u32 features)
{
    constexpr u32 FN = F_ALL & ~F_TRI;
    const u32 need = features & F_ALL;
    const u32 big = (need & F_TRI) ? (u32)F_ALL : FN;
    u32 cold = (scene_in_lds && (features & F_COLD)) ? (u32)F_COLD : 0u;             // the cold kernels exist in the big feature sets only
    if (cold && (features & F_DEEP) && (need & F_TRI)) cold |= F_DEEP;               // ... and the deep ones with the mesh code only
    const u32 nostash = (scene_in_lds && block_threads == 1024u && (features & F_NOSTASH) && !cold) ? (u32)F_NOSTASH : 0u;
    // per-corner attributes (the scene has a triangle or a mesh): the full feature set in every shape and staging level
    if (features & F_VATTR) return F_ALL | F_VATTR | (features & (F_BVH | F_ENV)) | (scene_in_lds ? cold | nostash : 0u);
    if (features & F_BVH) {
        if (!scene_in_lds) return big | F_BVH;
        const u32 pick = (need & (F_BOX | F_TRI | F_MAPS)) == 0 ? (need & F_LIGHTS) : big;
        // sphere / plane crowds whose instances are all untransformed (the reference's Instance.json): F_IDENT builds
        const u32 ident = ((features & F_IDENT) && pick != big && !nostash && !cold && block_threads != 64u) ? (u32)F_IDENT : 0u;
        return pick | F_BVH | nostash | cold | ident;
    }
    if (!scene_in_lds) return big;
    if (cold) return big | cold;
    // scenes whose instances are all untransformed: the F_IDENT builds of the plain 256-thread kernels without triangle / map code
    if (block_threads == 256u && (features & F_IDENT) && (need & (F_TRI | F_MAPS)) == 0u) return need | F_IDENT;
    if (block_threads == 64u || block_threads == 256u) return need;
    return big | nostash;
}

}  // namespace mrt
