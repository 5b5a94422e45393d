// mrt_megakernel.h — launch bounds of the path-tracing kernel (pt_megakernel of mrt_pt_kernel.h: the ordinary instantiations
// in mrt_kernels.hip, the tile-list ones in mrt_adapt.hip) and the list of its instantiations.
#pragma once
#include <hip/hip_runtime.h>

#include "mrt_inst.h"      // lds_stash_for
#include "mrt_trace.h"

namespace mrt {

// Workgroup = tiles_x x tiles_y wavefronts, each wavefront an 8x8 pixel tile (64 lanes): neighbouring
// pixels share most of their path prefix, which keeps the per-lane predicates of the uniform traversal
// loop coherent.  Rows are the shard-local rows of this context (block-cyclic over shards).
// Register budget per instantiation (second __launch_bounds__ argument = minimum waves per SIMD).  The kernel is
// VALU-issue bound, so the light variants (planes / spheres / boxes, no maps, no lights, no triangles) are squeezed to
// 6 waves per SIMD (80 VGPRs, a few spills: measured +14 % on the Cornell box); the heavier variants lose more to
// spills than they gain from occupancy and keep the compiler's choice.  MRT_WAVES_PER_EU overrides (experiments).
#ifndef MRT_BVH_WAVES
#define MRT_BVH_WAVES 6
#endif
constexpr int waves_for(u32 feat_, int block_threads)
{
#ifdef MRT_WAVES_PER_EU
    return MRT_WAVES_PER_EU;
#else
    const u32 feat = plain_feat(feat_);      // (F_IDENT changes nothing here)
    // Planes and spheres only (the Cornell box), 256-thread workgroups: 8 waves per SIMD (64 VGPRs).  With single-wave
    // workgroups every wavefront brings its own 5.5 KB of LDS (scene copy + stash) and the CU tops out at 29 of them, so a
    // bound of 8 only bought spills there (-3 %); four waves around one copy need 13 KB and all 32 fit: 7.42 -> 7.93
    // Gsamples/s on the headline frame (7.71 with the 7-wave build of the same shape).  With boxes (CornellBox2) 8 loses to 7.
    if (feat == 0u && block_threads == 256) return 8;
    // The instance-BVH kernels without mesh code, warm staging (F_COLD: texels in global memory, so the LDS no longer caps the
    // resident wavefronts at one 1024-thread workgroup): bound to 6 waves per SIMD (80 VGPRs, a few spills).  These walks
    // wait on dependent LDS reads, not on issue slots: the Minecraft-shaped scene gains 12 % with 5 waves, 16 % with 6, 17 %
    // with 7-8 over the 4 its 114 VGPRs allow.  The mesh kernels stay at 4: their LDS footprint caps them at 16 waves per CU.
    if ((feat & F_COLD) && (feat & F_BVH) && !(feat & F_TRI)) return MRT_BVH_WAVES;
    // Scenes with lights but without meshes, triangles or an instance BVH (example/Default.json, dof.json: 106-122 VGPRs as the
    // compiler would have it, 4 waves): bound to 5 waves per SIMD (96 VGPRs).  1080p renders: default scene 110 -> 118
    // Gsamples/s, dof scene 17.7 -> 20.3 (6 waves: 111 / 19.2).  The mesh kernels lose with every register taken from them
    // (kitchen-sink scene: 3284 / 3095 / 2765 Msamples/s at 4 / 5 / 6 waves).
    if ((feat & F_LIGHTS) && !(feat & (F_TRI | F_BVH | F_COLD | F_NOSTASH)) && block_threads <= 256) return 5;      // (larger workgroups: LDS-capped at 16 waves per CU anyway)
    return (feat & ~F_BOX) == 0 ? 7 : ((feat & (F_LIGHTS | F_TRI | F_BVH)) == 0 ? 6 : 4);      // the BVH walks need their registers more than two extra waves
#endif
}

// Instantiations of the kernel (with either tile source), per workgroup size (MRT_CASE(T, F) is defined at each use): one per feature set for the two
// common launch shapes with the scene in LDS: 256 threads (2x2 wave tiles) and 64 threads (one 8x8 tile per workgroup, used
// when the frame has too few tiles to balance 256 CUs with 4-wave workgroups).  The 512-thread shape (one LDS copy per CU,
// scenes of 78-160 KB) and the scene-in-L2 fallback and the 1024-thread shape (one LDS copy + stash per CU, 16 waves) carry
// every feature.
#define MRT_PLAIN16(T) MRT_CASE(T, 0) MRT_CASE(T, 1) MRT_CASE(T, 2) MRT_CASE(T, 3) MRT_CASE(T, 4) MRT_CASE(T, 5) MRT_CASE(T, 6) MRT_CASE(T, 7) \
    MRT_CASE(T, 8) MRT_CASE(T, 9) MRT_CASE(T, 10) MRT_CASE(T, 11) MRT_CASE(T, 12) MRT_CASE(T, 13) MRT_CASE(T, 14) MRT_CASE(T, 15)
#define MRT_BVH4(T, X) MRT_CASE(T, F_BVH | (X)) MRT_CASE(T, F_LIGHTS | F_BVH | (X)) MRT_CASE(T, (F_ALL & ~F_TRI) | F_BVH | (X)) MRT_CASE(T, F_ALL | F_BVH | (X))
#define MRT_BIG2(T, X) MRT_CASE(T, (F_ALL & ~F_TRI) | (X)) MRT_CASE(T, F_ALL | (X))
#define MRT_IDENT4(T) MRT_CASE(T, F_IDENT) MRT_CASE(T, F_IDENT | F_BOX) MRT_CASE(T, F_IDENT | F_LIGHTS) MRT_CASE(T, F_IDENT | F_BOX | F_LIGHTS)
#define MRT_IDENT_BVH2(T) MRT_CASE(T, F_IDENT | F_BVH) MRT_CASE(T, F_IDENT | F_LIGHTS | F_BVH)
#define MRT_DEEP2(T) MRT_CASE(T, F_ALL | F_COLD | F_DEEP) MRT_CASE(T, F_ALL | F_BVH | F_COLD | F_DEEP)
// Scenes with per-corner attributes (F_VATTR) always take the full feature set: per shape and staging level one
// kernel without and one with the instance BVH.
#define MRT_VATTR2(T, X) MRT_CASE(T, F_ALL | F_VATTR | (X)) MRT_CASE(T, F_ALL | F_BVH | F_VATTR | (X))
#define MRT_VATTR6(T) MRT_VATTR2(T, 0u) MRT_VATTR2(T, F_COLD) MRT_VATTR2(T, F_COLD | F_DEEP)
// Scenes with an environment texture (F_ENV) likewise, on top of F_VATTR: the same family once more.
#define MRT_ENV2(T, X) MRT_VATTR2(T, F_ENV | (X))
#define MRT_ENV6(T) MRT_ENV2(T, 0u) MRT_ENV2(T, F_COLD) MRT_ENV2(T, F_COLD | F_DEEP)
#define MRT_SHAPES_64 MRT_PLAIN16(64) MRT_BVH4(64, 0u) MRT_VATTR2(64, 0u) MRT_ENV2(64, 0u)
#define MRT_SHAPES_256 MRT_PLAIN16(256) MRT_IDENT4(256) MRT_BVH4(256, 0u) MRT_IDENT_BVH2(256) MRT_BIG2(256, F_COLD) MRT_BVH4(256, F_COLD) MRT_DEEP2(256) \
    MRT_VATTR6(256) MRT_ENV6(256)
#define MRT_SHAPES_512 MRT_BIG2(512, 0u) MRT_BVH4(512, 0u) MRT_IDENT_BVH2(512) MRT_BIG2(512, F_COLD) MRT_BVH4(512, F_COLD) MRT_DEEP2(512) MRT_VATTR6(512) MRT_ENV6(512)
#define MRT_SHAPES_1024 MRT_BIG2(1024, 0u) MRT_BVH4(1024, 0u) MRT_IDENT_BVH2(1024) MRT_BIG2(1024, F_NOSTASH) MRT_BVH4(1024, F_NOSTASH) \
    MRT_BIG2(1024, F_COLD) MRT_BVH4(1024, F_COLD) MRT_DEEP2(1024) MRT_VATTR6(1024) MRT_VATTR2(1024, F_NOSTASH) MRT_ENV6(1024) MRT_ENV2(1024, F_NOSTASH)
#define MRT_SHAPES_L2 MRT_CASE_L2(F_ALL & ~F_TRI) MRT_CASE_L2(F_ALL) MRT_CASE_L2((F_ALL & ~F_TRI) | F_BVH) MRT_CASE_L2(F_ALL | F_BVH) \
    MRT_CASE_L2(F_ALL | F_VATTR) MRT_CASE_L2(F_ALL | F_BVH | F_VATTR) \
    MRT_CASE_L2(F_ALL | F_VATTR | F_ENV) MRT_CASE_L2(F_ALL | F_BVH | F_VATTR | F_ENV)

}  // namespace mrt
