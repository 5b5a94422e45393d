// mrt_inst.h — which pt_megakernel instantiation serves a scene, and the LDS a workgroup of it needs: the one host-side statement
// of both rules.  Plain C++ with no HIP dependency, so that the launchers (mrt_kernels.hip, mrt_denoise.hip), the kernels
// (mrt_pt_kernel.h), the launch policy (mrt_plan.cpp), the host units (mrt_hooks.cpp, mrt_radiance.cpp) and the x86 builds of tests/emu all call the same functions.
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

// The per-path LDS stash (mrt_trace.h) is used by every launch shape that has room for it next to the scene: the
// 64- and 256-thread workgroups with the scene in LDS.  It moves 7-25 VGPRs of rarely touched state out of the loop.
constexpr bool lds_stash_for(bool scene_in_lds, int block_threads, u32 feat)
{
#ifdef MRT_NO_STASH
    return false;
#else
    (void)scene_in_lds;      // scenes read through L2 keep the stash too: the LDS is otherwise empty
    return block_threads != 512 && !(feat & F_NOSTASH);
#endif
}

// The kernels that understand tapered items (Params.band_items): the 256-thread
// kernels with the scene and the lane stash in LDS whose paths end before their scatter (the Cornell box's family), with either
// tile source.  Every other instantiation is launched with band_items == 0 and carries none of the code.
constexpr bool band_kernel(bool scene_in_lds, int block_threads, u32 feat)
{
    return scene_in_lds && block_threads == 256 && end_before_scatter(feat) && lds_stash_for(scene_in_lds, block_threads, feat);
}

// LDS bytes per workgroup of a launch: staged scene + lane stash + the mesh kernels' walk areas
inline size_t pt_lds_bytes(const Params &P, u32 block_threads, bool scene_in_lds, u32 features)
{
    const u32 inst = pt_instantiation(block_threads, scene_in_lds, features);      // what the kernel itself sees as FEAT
    size_t lds = scene_in_lds ? (size_t)staged_words_for(P, inst) * 4u : 0u;
    lds = (lds + 15u) & ~(size_t)15u;
    if (lds_stash_for(scene_in_lds, (int)block_threads, inst)) lds += (size_t)stash_slots_for(inst, block_threads) * block_threads * sizeof(float);
    if (has_walk_area(inst)) lds += (size_t)P.walk_cap * block_threads * sizeof(u32);
    return lds;
}

}  // namespace mrt
