// mrt_rays.hip — gfx950 kernels of mrt_radiance and mrt_camera_rays.  A translation unit of its own, so that the
// other kernels are compiled exactly as without it.
//
//   pt_rays       ray i = thread i of a launch of 256-thread workgroups (lane i % 64 of wavefront i / 64): every sample of the call
//                 on a caller-supplied primary ray (rays_body, mrt_rays.h), behind the staging prologue of pt_megakernel
//                 (mrt_pt_kernel.h) -- the whole scene in LDS, or read through L2 -- with the per-path state in registers
//   camera_rays   the lens-centre camera ray of every supersampled pixel
//
// Build: as mrt_kernels.hip.
#include <hip/hip_runtime.h>

#include "mrt_kernels.h"
#include "mrt_megakernel.h"
#include "mrt_rays.h"

namespace mrt {

template <bool SCENE_IN_LDS, u32 FEAT>
__global__ void __launch_bounds__(256, waves_for(FEAT, 256)) pt_rays(const Params P, const u32 *__restrict__ blob_g, u32 n, const float *__restrict__ orig,
                                                                     const float *__restrict__ dir, const u32 *__restrict__ key)
{
    // the staging prologue of pt_megakernel (mrt_pt_kernel.h has the original), written out: a shared helper is not free
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
    static_assert(!has_walk_area(FEAT), "pt_rays has no walk areas");
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    u32 seg = 0;
    // (after the staging barrier) the lanes behind n stay out of the body, as do_tile's !active lanes: not part of any wave vote
    if (i < n) {
        const V3 o = v3(orig[(size_t)i * 3], orig[(size_t)i * 3 + 1], orig[(size_t)i * 3 + 2]);
        const V3 d = v3(dir[(size_t)i * 3], dir[(size_t)i * 3 + 1], dir[(size_t)i * 3 + 2]);
        rays_body<FEAT>(S, i, o, d, key ? key[i] : i, seg);
    }
    if (P.count_segments) {
        // wave-level sum (every lane of the wavefront is here again), one atomic per wavefront
        u32 v = seg;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63u) == 0u && v) atomicAdd(P.segments, (unsigned long long)v);
    }
}

// pixel p = thread p of 256-thread workgroups; either output may be null
__global__ void __launch_bounds__(256) camera_rays(const Params P, float *__restrict__ orig, float *__restrict__ dir)
{
    const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= (size_t)P.nw * P.nh) return;
    V3 o, d;
    camera_ray_of(P, reinterpret_cast<const float *>(P.blob), (u32)(p % P.nw), (u32)(p / P.nw), o, d);
    if (orig) { orig[p * 3] = o.x; orig[p * 3 + 1] = o.y; orig[p * 3 + 2] = o.z; }
    if (dir) { dir[p * 3] = d.x; dir[p * 3 + 1] = d.y; dir[p * 3 + 2] = d.z; }
}

// ---- launchers (declared in mrt_kernels.h) ----
size_t rays_lds_bytes(const Params &P, bool scene_in_lds, u32 inst)
{
    return scene_in_lds ? (((size_t)staged_words_for(P, inst) * 4u + 15u) & ~(size_t)15u) : 0u;
}

hipError_t launch_rays(const Params &P, bool scene_in_lds, u32 inst, u32 n, const float *orig, const float *dir, const u32 *key, hipStream_t stream)
{
    const dim3 grid((n + 255u) / 256u);
    const size_t lds = rays_lds_bytes(P, scene_in_lds, inst);
#define MRT_RAYS(F) \
    if (inst == (u32)(F)) { \
        if (scene_in_lds) { \
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&pt_rays<true, (F)>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) return e; \
            hipLaunchKernelGGL((pt_rays<true, (F)>), grid, dim3(256), lds, stream, P, P.blob, n, orig, dir, key); \
        } else { \
            hipLaunchKernelGGL((pt_rays<false, (F)>), grid, dim3(256), 0, stream, P, P.blob, n, orig, dir, key); \
        } \
        return hipGetLastError(); \
    }
    MRT_RAYS_LIST
#undef MRT_RAYS
    return hipErrorInvalidConfiguration;
}

hipError_t launch_camera_rays(const Params &P, float *orig, float *dir, hipStream_t stream)
{
    const size_t np = (size_t)P.nw * P.nh;
    hipLaunchKernelGGL(camera_rays, dim3((unsigned)((np + 255u) / 256u)), dim3(256), 0, stream, P, orig, dir);
    return hipGetLastError();
}

}  // namespace mrt
