// mrt_rays_adapt.hip — gfx950 kernels of mrt_radiance_adaptive.  A translation unit of its own, so that the other
// kernels are compiled exactly as without it.
//
//   pt_rays_tiles   wavefront W = 4 * workgroup + wave of a launch of 256-thread workgroups serves entry W / k_split of a list of
//                   8x8 tiles with chunk phase W % k_split; lane l is pixel (8 tx + l % 8, 8 ty + l / 8) of that tile, traced on
//                   its caller-supplied ray (rays_tile_body, mrt_rays_adapt.h) behind the staging prologue of pt_rays
//
// Build: as mrt_kernels.hip.
#include <hip/hip_runtime.h>

#include "mrt_kernels.h"
#include "mrt_megakernel.h"
#include "mrt_rays_adapt.h"

namespace mrt {

template <bool SCENE_IN_LDS, u32 FEAT>
__global__ void __launch_bounds__(256, waves_for(FEAT, 256)) pt_rays_tiles(const Params P, const u32 *__restrict__ blob_g, const u32 *__restrict__ list, u32 n_listed,
                                                                           const float *__restrict__ orig, const float *__restrict__ dir)
{
    // the staging prologue of pt_rays (mrt_rays.hip), written out: a shared helper is not free
    extern __shared__ uint4 lds_blob[];
    const float *F;
    if (SCENE_IN_LDS) {
        const uint4 *g = reinterpret_cast<const uint4 *>(P.blob);
        const u32 n4 = staged_words_for(P, FEAT) >> 2;
        for (u32 i = threadIdx.x; i < n4; i += blockDim.x) lds_blob[i] = g[i];
        __syncthreads();
        F = reinterpret_cast<const float *>(lds_blob);
    } else {
        F = reinterpret_cast<const float *>(P.blob);
    }
    Scn S;
    S.F = F;
    S.U = F;
    S.G = reinterpret_cast<const float *>(blob_g);
    S.P = &P;
    S.wk = nullptr; S.wk_stride = 256;                 // (no feature set of MRT_RAYS_LIST has a walk area)
    static_assert(!has_walk_area(FEAT), "pt_rays_tiles has no walk areas");
    const u32 wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    u32 seg = 0;
    // (after the staging barrier) the wavefronts past the list and the lanes outside the frame stay out of the body, as pt_rays'
    // lanes behind n: not part of any wave vote
    if (wave < n_listed * P.k_split) {
        const u32 entry = wave / P.k_split, phase = wave - entry * P.k_split;
        u32 p;
        if (rays_tile_pixel(list[entry], threadIdx.x & 63u, P.nw, P.nh, p)) {
            const V3 o = v3(orig[(size_t)p * 3], orig[(size_t)p * 3 + 1], orig[(size_t)p * 3 + 2]);
            const V3 d = v3(dir[(size_t)p * 3], dir[(size_t)p * 3 + 1], dir[(size_t)p * 3 + 2]);
            rays_tile_body<FEAT>(S, p, phase, o, d, seg);
        }
    }
    if (P.count_segments) {
        // wave-level sum (every lane of the wavefront is here again), one atomic per wavefront
        u32 v = seg;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63u) == 0u && v) atomicAdd(P.segments, (unsigned long long)v);
    }
}

// ---- launcher (declared in mrt_rays_adapt.h) ----
hipError_t launch_rays_tiles(const Params &P, bool scene_in_lds, u32 inst, const TileList &tl, const float *orig, const float *dir, hipStream_t stream)
{
    if (!tl.n) return hipSuccess;
    const dim3 grid((unsigned)(((unsigned long long)tl.n * P.k_split + 3ull) / 4ull));
    const size_t lds = rays_lds_bytes(P, scene_in_lds, inst);
#define MRT_RAYS(F) \
    if (inst == (u32)(F)) { \
        if (scene_in_lds) { \
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&pt_rays_tiles<true, (F)>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) return e; \
            hipLaunchKernelGGL((pt_rays_tiles<true, (F)>), grid, dim3(256), lds, stream, P, P.blob, tl.tiles, tl.n, orig, dir); \
        } else { \
            hipLaunchKernelGGL((pt_rays_tiles<false, (F)>), grid, dim3(256), 0, stream, P, P.blob, tl.tiles, tl.n, orig, dir); \
        } \
        return hipGetLastError(); \
    }
    MRT_RAYS_LIST
#undef MRT_RAYS
    return hipErrorInvalidConfiguration;
}

}  // namespace mrt
