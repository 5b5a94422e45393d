// mrt_gather.hip — gfx950 kernels of mrt_gather and mrt_gather_rays.  A translation unit of its own, so that the
// other kernels are compiled exactly as without it; no path-tracing kernel is instantiated here (the rays go through launch_rays).
//
//   gather_gen      ray r = thread r of a launch of 256-thread workgroups: ray (first + r / n_dirs, r % n_dirs) of the call
//                   (gather_ray, mrt_gather.h) into the workspace
//   gather_reduce   one wavefront per point, four points per 256-thread workgroup: lane l sums its directions l, l + 64, ...
//                   (gather_lane_partial), the 64 partials are combined with __shfl_down at distances 32, 16, 8, 4, 2, 1 and lane 0
//                   writes the scaled result
//
// Build: as mrt_kernels.hip.
#include <hip/hip_runtime.h>

#include "mrt_gather.h"

namespace mrt {

__global__ void __launch_bounds__(256) gather_gen(const GatherSet g, const float *__restrict__ pos, const float *__restrict__ normal, u32 first,
                                                  u32 n_rays, float *__restrict__ orig, float *__restrict__ dir, u32 *__restrict__ key)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rays) return;
    const u32 il = r / g.n_dirs, j = r - il * g.n_dirs;
    const size_t i = (size_t)first + il;
    G3 o, d;
    u32 k;
    gather_ray(g, (u32)i, j, pos + i * 3u, normal ? normal + i * 3u : nullptr, o, d, k);
    if (orig) { orig[(size_t)r * 3u] = o.x; orig[(size_t)r * 3u + 1u] = o.y; orig[(size_t)r * 3u + 2u] = o.z; }
    if (dir) { dir[(size_t)r * 3u] = d.x; dir[(size_t)r * 3u + 1u] = d.y; dir[(size_t)r * 3u + 2u] = d.z; }
    if (key) key[r] = k;
}

template <u32 OUT>
__global__ void __launch_bounds__(256) gather_reduce(const float *__restrict__ sums, const float *__restrict__ dirs, u32 n_points, u32 n_dirs,
                                                     u32 n_samples, float *__restrict__ res)
{
    constexpr u32 W = gather_words(OUT);
    const u32 pt = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (pt >= n_points) return;                            // whole wavefronts leave: every lane of a wavefront that stays takes part below
    const size_t base = (size_t)pt * n_dirs * 3u;
    float p[W];
    gather_lane_partial<OUT>(sums + base, dirs + base, n_dirs, lane, n_samples, p);
    // p[l] += p[l + 32], then 16, 8, 4, 2, 1: lane 0 only ever reads lanes that hold the sum of their own subtree
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (u32 w = 0; w < W; ++w) p[w] = p[w] + __shfl_down(p[w], off, 64);
    }
    const float scale = gather_scale<OUT>(n_dirs);
    if (lane == 0u) {
#pragma unroll
        for (u32 w = 0; w < W; ++w) res[(size_t)pt * W + w] = p[w] * scale;
    }
}

// ---- launchers (declared in mrt_gather.h) ----
hipError_t launch_gather_gen(const GatherSet &g, const float *pos, const float *normal, u32 first, u32 count, float *orig, float *dir, u32 *key,
                             hipStream_t stream)
{
    const u32 n_rays = count * g.n_dirs;                   // < 2^30 (the host cuts its batches so)
    hipLaunchKernelGGL(gather_gen, dim3((n_rays + 255u) / 256u), dim3(256), 0, stream, g, pos, normal, first, n_rays, orig, dir, key);
    return hipGetLastError();
}

hipError_t launch_gather_reduce(u32 out, const float *sums, const float *dirs, u32 count, u32 n_dirs, u32 n_samples, float *res, hipStream_t stream)
{
    const dim3 grid((count + 3u) / 4u);
    if (out == MRT_GATHER_SH9)
        hipLaunchKernelGGL((gather_reduce<MRT_GATHER_SH9>), grid, dim3(256), 0, stream, sums, dirs, count, n_dirs, n_samples, res);
    else if (out == MRT_GATHER_MEAN)
        hipLaunchKernelGGL((gather_reduce<MRT_GATHER_MEAN>), grid, dim3(256), 0, stream, sums, dirs, count, n_dirs, n_samples, res);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace mrt
