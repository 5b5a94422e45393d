// mrt_denoise.hip — gfx950 kernels of the first-hit AOVs and the a-trous denoiser (mrt_aov, mrt_denoise, mrt_img_denoised;
// DESIGN.md §13).  A translation unit of its own, so that the path-tracing kernels are compiled exactly as without it.
//
//   aov_first_hit   one lens-centre camera ray per supersampled pixel, scene read through L2 (the feature sets of the L2
//                   path-tracing shape): guide (normal, depth, world point, hit flag), albedo, renderer and flat instance index
//   dn_mean         passes = 0: the mean c = A * rc, unchanged
//   dn_pass         one a-trous pass at step s = 2^i over one residue class (x mod s, y mod s) of the frame -- a dense 5x5
//                   stencil on that sub-image -- a 16x16 block per 256-thread workgroup with its 2-entry halo in LDS;
//                   pass 0 demodulates the accumulator on load, the last pass remodulates into the output
//
// Build: as mrt_kernels.hip.
#include <hip/hip_runtime.h>

#include "mrt_denoise.h"
#include "mrt_kernels.h"

namespace mrt {

template <u32 FEAT>
__global__ void __launch_bounds__(256) aov_first_hit(const Params P, float4 *__restrict__ guide, float *__restrict__ albedo, i32 *__restrict__ ids)
{
    const u32 x = blockIdx.x * 16u + (threadIdx.x & 15u), y = blockIdx.y * 16u + (threadIdx.x >> 4);
    if (x >= P.nw || y >= P.nh) return;
    Scn S;
    S.F = reinterpret_cast<const float *>(P.blob);
    S.U = S.F; S.G = S.F; S.P = &P;
    S.wk = nullptr; S.wk_stride = 256u;          // the L2 shape has no walk area (has_walk_area: F_COLD kernels only)
    const AovPixel a = aov_pixel<FEAT>(S, x, y);
    const size_t p = (size_t)y * P.nw + x, np = (size_t)P.nw * P.nh;
    guide[p] = make_float4(a.g.nx, a.g.ny, a.g.nz, a.g.t);
    guide[np + p] = make_float4(a.g.px, a.g.py, a.g.pz, a.g.hit);
    albedo[3 * p] = a.albedo.x; albedo[3 * p + 1] = a.albedo.y; albedo[3 * p + 2] = a.albedo.z;
    ids[2 * p] = a.rend; ids[2 * p + 1] = a.inst;
}

__global__ void __launch_bounds__(256) dn_mean(const float *__restrict__ accum, float rc, const u32 *__restrict__ tile_count, u32 nw, u32 nh,
                                               float *__restrict__ out)
{
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nw * nh) return;
    const u32 y = i / nw, x = i - y * nw;
    const float r = mean_rc({accum, rc, tile_count, nw}, x, y);
    for (u32 k = 0; k < 3u; ++k) out[(size_t)i * 3 + k] = accum[(size_t)i * 3 + k] * r;
}

struct DnPassArgs {
    u32 nw, nh, step, cx, cy;          // frame, step s = 2^i, residue classes per axis (min(s, nw), min(s, nh))
    u32 first, last;
    float sc, sn, sp;
    const float4 *e_in;                // not first: e of the previous pass, one float4 per pixel
    const float *accum;                // first: the accumulator [nh][nw][3] ...
    float rc;                          // ... with this 1/count, or
    const u32 *tile_count;             // ... per 8x8 tile counts (adaptive; null: rc): with nw, the fields of a MeanSrc (mrt_adapt.h)
    const float *albedo;               // [nh][nw][3]
    const float4 *guide;               // [2][nh][nw]: (n, t), (x, hit)
    float4 *e_out;                     // not last
    float *out;                        // last: c' [nh][nw][3]
};

constexpr u32 kDnB = 16, kDnT = kDnB + 4;   // output block, LDS tile with the 2-entry halo

#define MRT_DN_ENV 0
#include "mrt_dn_pass_kernel.h"
#undef MRT_DN_ENV
#define MRT_DN_ENV 1
#include "mrt_dn_pass_kernel.h"
#undef MRT_DN_ENV

// ---- launchers (declared in mrt_kernels.h) ----
hipError_t launch_aov(const Params &P, u32 features, float *guide, float *albedo, i32 *ids, hipStream_t stream)
{
    constexpr u32 FN = F_ALL & ~F_TRI;
    const u32 inst = pt_instantiation(256u, false, features);       // the L2 shape
    const dim3 grid((P.nw + 15u) / 16u, (P.nh + 15u) / 16u);
    float4 *g = reinterpret_cast<float4 *>(guide);
    switch (inst) {
    case FN: hipLaunchKernelGGL((aov_first_hit<FN>), grid, dim3(256), 0, stream, P, g, albedo, ids); break;
    case F_ALL: hipLaunchKernelGGL((aov_first_hit<F_ALL>), grid, dim3(256), 0, stream, P, g, albedo, ids); break;
    case FN | F_BVH: hipLaunchKernelGGL((aov_first_hit<FN | F_BVH>), grid, dim3(256), 0, stream, P, g, albedo, ids); break;
    case F_ALL | F_BVH: hipLaunchKernelGGL((aov_first_hit<F_ALL | F_BVH>), grid, dim3(256), 0, stream, P, g, albedo, ids); break;
    case F_ALL | F_VATTR: hipLaunchKernelGGL((aov_first_hit<F_ALL | F_VATTR>), grid, dim3(256), 0, stream, P, g, albedo, ids); break;
    case F_ALL | F_BVH | F_VATTR: hipLaunchKernelGGL((aov_first_hit<F_ALL | F_BVH | F_VATTR>), grid, dim3(256), 0, stream, P, g, albedo, ids); break;
    case F_ALL | F_VATTR | F_ENV: hipLaunchKernelGGL((aov_first_hit<F_ALL | F_VATTR | F_ENV>), grid, dim3(256), 0, stream, P, g, albedo, ids); break;
    case F_ALL | F_BVH | F_VATTR | F_ENV: hipLaunchKernelGGL((aov_first_hit<F_ALL | F_BVH | F_VATTR | F_ENV>), grid, dim3(256), 0, stream, P, g, albedo, ids); break;
    default: return hipErrorInvalidConfiguration;
    }
    return hipGetLastError();
}

hipError_t launch_denoise(const MeanSrc &S, const float *guide, const float *albedo, u32 nh, u32 passes,
                          float sc, float sn, float sp, float *e0, float *e1, float *out, hipStream_t stream, bool env)
{
    const u32 nw = S.nw;
    if (passes == 0u) {
        hipLaunchKernelGGL(dn_mean, dim3((unsigned)(((size_t)nw * nh + 255u) / 256u)), dim3(256), 0, stream, S.sums, S.rc, S.tile_count, nw, nh, out);
        return hipGetLastError();
    }
    float4 *buf[2] = {reinterpret_cast<float4 *>(e0), reinterpret_cast<float4 *>(e1)};
    for (u32 i = 0; i < passes; ++i) {
        DnPassArgs A;
        A.nw = nw; A.nh = nh; A.step = 1u << i;
        A.cx = A.step < nw ? A.step : nw;
        A.cy = A.step < nh ? A.step : nh;
        A.first = i == 0u; A.last = i + 1u == passes;
        A.sc = dn_pass_sc(sc, i); A.sn = sn; A.sp = sp;
        A.e_in = buf[(i + 1u) & 1u]; A.e_out = buf[i & 1u];
        A.accum = S.sums; A.rc = S.rc; A.tile_count = S.tile_count;
        A.albedo = albedo; A.guide = reinterpret_cast<const float4 *>(guide);
        A.out = out;
        // sub-images of a class are at most ceil(n / s) wide / high
        const u32 sw = (nw + A.step - 1u) / A.step, sh = (nh + A.step - 1u) / A.step;
        const dim3 grid(A.cx * ((sw + kDnB - 1u) / kDnB), A.cy * ((sh + kDnB - 1u) / kDnB));
        if (env) hipLaunchKernelGGL(dn_pass_env, grid, dim3(256), 0, stream, A);
        else hipLaunchKernelGGL(dn_pass, grid, dim3(256), 0, stream, A);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace mrt
