// mrt_denoise.hip — gfx950 kernels of the first-hit AOVs and the a-trous denoiser (mrt_aov, mrt_denoise, mrt_img_denoised;
// DESIGN.md §13).  A translation unit of its own, so that the path-tracing kernels are compiled exactly as without it.
//
//   aov_first_hit   one lens-centre camera ray per supersampled pixel, scene read through L2 (the feature sets of the L2
//                   path-tracing shape): guide (normal, depth, world point, hit flag), albedo, renderer and flat instance index
//   aov_rays        the same pass on one caller-supplied ray per pixel (mrt_aov_rays)
//   dn_mean         passes = 0: the mean c = A * rc, unchanged
//   dn_pass         one a-trous pass at step s = 2^i over one residue class (x mod s, y mod s) of the frame -- a dense 5x5
//                   stencil on that sub-image -- a 16x16 block per 256-thread workgroup with its 2-entry halo in LDS;
//                   pass 0 demodulates the accumulator on load, the last pass remodulates into the output; WRAP: the frame is
//                   periodic in x, a halo entry left or right of the frame is loaded from its frame x modulo nw
//
// Build: as mrt_kernels.hip.
#include <hip/hip_runtime.h>

#include "mrt_denoise.h"
#include "mrt_kernels.h"
#include "mrt_megakernel.h"      // MRT_SHAPES_L2

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

// aov_first_hit on the ray that orig / dir [nh][nw][3] hold for the pixel, traced as given: the same scene, the same planes
template <u32 FEAT>
__global__ void __launch_bounds__(256) aov_rays(const Params P, const float *__restrict__ orig, const float *__restrict__ dir,
                                                float4 *__restrict__ guide, float *__restrict__ albedo, i32 *__restrict__ ids)
{
    const u32 x = blockIdx.x * 16u + (threadIdx.x & 15u), y = blockIdx.y * 16u + (threadIdx.x >> 4);
    if (x >= P.nw || y >= P.nh) return;
    Scn S;
    S.F = reinterpret_cast<const float *>(P.blob);
    S.U = S.F; S.G = S.F; S.P = &P;
    S.wk = nullptr; S.wk_stride = 256u;          // no walk area, as above
    const size_t p = (size_t)y * P.nw + x, np = (size_t)P.nw * P.nh;
    const AovPixel a = aov_ray<FEAT>(S, v3(orig[3 * p], orig[3 * p + 1], orig[3 * p + 2]), v3(dir[3 * p], dir[3 * p + 1], dir[3 * p + 2]));
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

// ENV: the kernel of contexts with an environment texture, whose miss pixels are demodulated by their backdrop
// E(d) too (mrt_denoise.h dn_demod)
// WRAP: the kernel of frames periodic in x (MRT_AOV_WRAP_X).  Only the tile load differs: it is the frame x of the
// tap, rx + s * si, that is reduced modulo nw -- a wrapped tap generally lands in another residue class (nw % s != 0)
template <bool ENV, bool WRAP>
__global__ void __launch_bounds__(256) dn_pass(const DnPassArgs A)
{
    __shared__ float4 s_e[kDnT * kDnT];
    __shared__ float4 s_g0[kDnT * kDnT];
    __shared__ float4 s_g1[kDnT * kDnT];
    // block -> residue class (rx, ry) and block (bx, by) of that class's sub-image; sub-image pixel (i, j) is frame pixel
    // (rx + s * i, ry + s * j)
    const u32 rx = blockIdx.x % A.cx, bx = blockIdx.x / A.cx;
    const u32 ry = blockIdx.y % A.cy, by = blockIdx.y / A.cy;
    const u32 s = A.step;
    const size_t np = (size_t)A.nw * A.nh;
    for (u32 t = threadIdx.x; t < kDnT * kDnT; t += 256u) {
        const u32 lj = t / kDnT, li = t - lj * kDnT;
        const long long si = (long long)(bx * kDnB + li) - 2, sj = (long long)(by * kDnB + lj) - 2;
        long long fx = (long long)rx + (long long)s * si;
        const long long fy = (long long)ry + (long long)s * sj;
        bool in_x = si >= 0 && fx < (long long)A.nw;
        if constexpr (WRAP) {
            if (!in_x) fx = dn_wrap(fx, A.nw);
            in_x = true;
        }
        float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g0 = e, g1 = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        if (in_x && sj >= 0 && fy < (long long)A.nh) {
            const size_t p = (size_t)fy * A.nw + (size_t)fx;
            g0 = A.guide[p];
            g1 = A.guide[np + p];
            if (A.first) {
                const float r = mean_rc({A.accum, A.rc, A.tile_count, A.nw}, (u32)fx, (u32)fy);
                e.x = (A.accum[3 * p] * r) / dn_demod(A.albedo[3 * p], g1.w, ENV);
                e.y = (A.accum[3 * p + 1] * r) / dn_demod(A.albedo[3 * p + 1], g1.w, ENV);
                e.z = (A.accum[3 * p + 2] * r) / dn_demod(A.albedo[3 * p + 2], g1.w, ENV);
            } else {
                e = A.e_in[p];
            }
        }
        s_e[t] = e; s_g0[t] = g0; s_g1[t] = g1;
    }
    __syncthreads();
    const u32 li = threadIdx.x & 15u, lj = threadIdx.x >> 4;
    const u32 fx = rx + s * (bx * kDnB + li), fy = ry + s * (by * kDnB + lj);
    if ((unsigned long long)rx + (unsigned long long)s * (bx * kDnB + li) >= A.nw ||
        (unsigned long long)ry + (unsigned long long)s * (by * kDnB + lj) >= A.nh) return;
    const u32 c = (lj + 2u) * kDnT + li + 2u;
    auto guide_of = [&](u32 k) { const float4 a = s_g0[k], b = s_g1[k]; DnGuide g; g.nx = a.x; g.ny = a.y; g.nz = a.z; g.t = a.w; g.px = b.x; g.py = b.y; g.pz = b.z; g.hit = b.w; return g; };
    const DnGuide gp = guide_of(c);
    const float4 ep4 = s_e[c];
    const float ep[3] = {ep4.x, ep4.y, ep4.z};
    DnAcc acc;
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const u32 k = (u32)((int)(lj + 2u) + dy) * kDnT + (u32)((int)(li + 2u) + dx);
            const float4 eq4 = s_e[k];
            const float eq[3] = {eq4.x, eq4.y, eq4.z};
            acc.add(dn_tap_weight(dn_k5(dx) * dn_k5(dy), ep, eq, gp, guide_of(k), A.sc, A.sn, A.sp), eq);
        }
    float r[3];
    acc.result(ep, r);
    const size_t p = (size_t)fy * A.nw + fx;
    if (A.last) {
        for (u32 ch = 0; ch < 3u; ++ch) A.out[3 * p + ch] = r[ch] * dn_demod(A.albedo[3 * p + ch], gp.hit, ENV);
    } else {
        A.e_out[p] = make_float4(r[0], r[1], r[2], 0.0f);
    }
}

// ---- launchers (declared in mrt_kernels.h) ----
hipError_t launch_aov(const Params &P, u32 features, float *guide, float *albedo, i32 *ids, hipStream_t stream)
{
    const u32 inst = pt_instantiation(256u, false, features);       // the L2 shape
    const dim3 grid((P.nw + 15u) / 16u, (P.nh + 15u) / 16u);
    float4 *g = reinterpret_cast<float4 *>(guide);
#define MRT_CASE_L2(F) case (F): hipLaunchKernelGGL((aov_first_hit<(F)>), grid, dim3(256), 0, stream, P, g, albedo, ids); break;
    switch (inst) { MRT_SHAPES_L2 default: return hipErrorInvalidConfiguration; }
#undef MRT_CASE_L2
    return hipGetLastError();
}

hipError_t launch_aov_rays(const Params &P, u32 features, const float *orig, const float *dir, float *guide, float *albedo, i32 *ids, hipStream_t stream)
{
    const u32 inst = pt_instantiation(256u, false, features);       // the L2 shape
    const dim3 grid((P.nw + 15u) / 16u, (P.nh + 15u) / 16u);
    float4 *g = reinterpret_cast<float4 *>(guide);
#define MRT_CASE_L2(F) case (F): hipLaunchKernelGGL((aov_rays<(F)>), grid, dim3(256), 0, stream, P, orig, dir, g, albedo, ids); break;
    switch (inst) { MRT_SHAPES_L2 default: return hipErrorInvalidConfiguration; }
#undef MRT_CASE_L2
    return hipGetLastError();
}

hipError_t launch_denoise(const MeanSrc &S, const float *guide, const float *albedo, u32 nh, u32 passes,
                          float sc, float sn, float sp, float *e0, float *e1, float *out, hipStream_t stream, bool env, bool wrap_x)
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
        if (wrap_x) {
            if (env) hipLaunchKernelGGL((dn_pass<true, true>), grid, dim3(256), 0, stream, A);
            else hipLaunchKernelGGL((dn_pass<false, true>), grid, dim3(256), 0, stream, A);
        } else {
            if (env) hipLaunchKernelGGL((dn_pass<true, false>), grid, dim3(256), 0, stream, A);
            else hipLaunchKernelGGL((dn_pass<false, false>), grid, dim3(256), 0, stream, A);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace mrt
