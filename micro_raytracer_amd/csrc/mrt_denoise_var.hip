// mrt_denoise_var.hip — gfx950 kernels of the variance-guided denoiser mode (MRT_DN_VARIANCE).  A translation
// unit of its own: the kernels of mrt_denoise.hip and the path tracer are compiled exactly as without it.
//
//   dnv_prep   16x16 pixels per 256-thread workgroup, halo 1 in LDS: e = demodulated mean, h2 = squared half difference of the two
//              half-buffer estimates, the firefly clamp against the 8 neighbours' unclamped luminance; writes (e, h2)
//   dnv_init   halo 3: the 7x7 guide-weighted mean of h2, the initial variance v; h2 and the two guide planes in LDS; writes (e, v)
//   dnv_pass   one a-trous pass at step s = 2^i in dn_pass's residue-class tiling (20x20 LDS tile, three float4 planes); the variance
//              travels in the e plane's .w; its 3x3 prefilter uses the +-s taps of the tile; the last pass remodulates into the output
// One lane per pixel, no cross-lane reductions: bit-deterministic and equal to the x86 build of mrt_denoise_var.h.
// Environment contexts (miss pixels demodulated by their backdrop) are a run-time flag here.
//
// Build: as mrt_kernels.hip.
#include <hip/hip_runtime.h>

#include "mrt_denoise_var.h"
#include "mrt_kernels.h"

namespace mrt {

struct DnvArgs {
    u32 nw, nh, env;
    float f, sn, sp;                   // firefly factor (+inf: off), guide terms
    const float *accum, *half;         // A, H [nh][nw][3]
    const u32 *tile_count;             // per 8x8 tile counts
    const float *albedo;               // [nh][nw][3]
    const float4 *guide;               // [2][nh][nw]: (n, t), (x, hit)
    const float4 *in;                  // dnv_init: (e, h2) of dnv_prep
    float4 *out;
};

constexpr u32 kDnvB = 16, kDnvT1 = kDnvB + 2, kDnvT3 = kDnvB + 6, kDnvT = kDnvB + 4;

__device__ inline DnGuide dnv_guide_of(float4 a, float4 b)
{
    DnGuide g;
    g.nx = a.x; g.ny = a.y; g.nz = a.z; g.t = a.w; g.px = b.x; g.py = b.y; g.pz = b.z; g.hit = b.w;
    return g;
}

__global__ void __launch_bounds__(256) dnv_prep(const DnvArgs A)
{
    __shared__ float4 s_e[kDnvT1 * kDnvT1];          // (e, hit); hit -1: outside the frame, matches no pixel
    const size_t np = (size_t)A.nw * A.nh;
    const bool env = A.env != 0u;
    for (u32 t = threadIdx.x; t < kDnvT1 * kDnvT1; t += 256u) {
        const u32 lj = t / kDnvT1, li = t - lj * kDnvT1;
        const long long fx = (long long)(blockIdx.x * kDnvB + li) - 1, fy = (long long)(blockIdx.y * kDnvB + lj) - 1;
        float4 e = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        if (fx >= 0 && fy >= 0 && fx < (long long)A.nw && fy < (long long)A.nh) {
            const size_t p = (size_t)fy * A.nw + (size_t)fx;
            const float hit = A.guide[np + p].w;
            const float a[3] = {A.accum[3 * p], A.accum[3 * p + 1], A.accum[3 * p + 2]};
            const float alb[3] = {A.albedo[3 * p], A.albedo[3 * p + 1], A.albedo[3 * p + 2]};
            float m[3];
            dnv_mean(a, alb, hit, A.tile_count[tile_index(A.nw, (u32)fx, (u32)fy)], env, m);
            e = make_float4(m[0], m[1], m[2], hit);
        }
        s_e[t] = e;
    }
    __syncthreads();
    const u32 li = threadIdx.x & 15u, lj = threadIdx.x >> 4;
    const u32 x = blockIdx.x * kDnvB + li, y = blockIdx.y * kDnvB + lj;
    if (x >= A.nw || y >= A.nh) return;
    const size_t p = (size_t)y * A.nw + x;
    const u32 c = (lj + 1u) * kDnvT1 + li + 1u;
    const float4 ep4 = s_e[c];
    float e[3] = {ep4.x, ep4.y, ep4.z};
    if (dnv_finite(A.f)) {
        float m = -__builtin_inff();
        bool have = false;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (dx == 0 && dy == 0) continue;
                const float4 q = s_e[(u32)((int)(lj + 1u) + dy) * kDnvT1 + (u32)((int)(li + 1u) + dx)];
                if (q.w != ep4.w) continue;
                const float eq[3] = {q.x, q.y, q.z};
                have = true;
                m = dnv_firefly_max(m, dnv_lum(eq));
            }
        dnv_firefly(e, have, m, A.f);
    }
    const float a[3] = {A.accum[3 * p], A.accum[3 * p + 1], A.accum[3 * p + 2]};
    const float h[3] = {A.half[3 * p], A.half[3 * p + 1], A.half[3 * p + 2]};
    const float alb[3] = {A.albedo[3 * p], A.albedo[3 * p + 1], A.albedo[3 * p + 2]};
    const float h2 = dnv_h2(a, h, alb, ep4.w, A.tile_count[tile_index(A.nw, x, y)], env);
    A.out[p] = make_float4(e[0], e[1], e[2], h2);
}

__global__ void __launch_bounds__(256) dnv_init(const DnvArgs A)
{
    __shared__ float s_h[kDnvT3 * kDnvT3];
    __shared__ float4 s_g0[kDnvT3 * kDnvT3];
    __shared__ float4 s_g1[kDnvT3 * kDnvT3];
    const size_t np = (size_t)A.nw * A.nh;
    for (u32 t = threadIdx.x; t < kDnvT3 * kDnvT3; t += 256u) {
        const u32 lj = t / kDnvT3, li = t - lj * kDnvT3;
        const long long fx = (long long)(blockIdx.x * kDnvB + li) - 3, fy = (long long)(blockIdx.y * kDnvB + lj) - 3;
        float h = 0.0f;
        float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g1 = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        if (fx >= 0 && fy >= 0 && fx < (long long)A.nw && fy < (long long)A.nh) {
            const size_t p = (size_t)fy * A.nw + (size_t)fx;
            h = A.in[p].w;
            g0 = A.guide[p];
            g1 = A.guide[np + p];
        }
        s_h[t] = h; s_g0[t] = g0; s_g1[t] = g1;
    }
    __syncthreads();
    const u32 li = threadIdx.x & 15u, lj = threadIdx.x >> 4;
    const u32 x = blockIdx.x * kDnvB + li, y = blockIdx.y * kDnvB + lj;
    if (x >= A.nw || y >= A.nh) return;
    const u32 c = (lj + 3u) * kDnvT3 + li + 3u;
    const DnGuide gp = dnv_guide_of(s_g0[c], s_g1[c]);
    DnvInit acc;
    for (int dy = -3; dy <= 3; ++dy)
        for (int dx = -3; dx <= 3; ++dx) {
            const u32 k = (u32)((int)(lj + 3u) + dy) * kDnvT3 + (u32)((int)(li + 3u) + dx);
            const float4 b = s_g1[k];
            if (b.w < 0.0f) continue;                      // outside the frame
            acc.add(gp, dnv_guide_of(s_g0[k], b), A.sn, A.sp, s_h[k]);
        }
    const size_t p = (size_t)y * A.nw + x;
    const float4 e = A.in[p];
    A.out[p] = make_float4(e.x, e.y, e.z, acc.result(s_h[c]));
}

struct DnvPassArgs {
    u32 nw, nh, step, cx, cy;          // frame, step s = 2^i, residue classes per axis (min(s, nw), min(s, nh))
    u32 last, env;
    float sv, sn, sp;
    const float4 *e_in;                // (e, v) of the previous pass or of dnv_init
    const float *albedo;               // [nh][nw][3]
    const float4 *guide;               // [2][nh][nw]
    float4 *e_out;                     // not last
    float *out;                        // last: c' [nh][nw][3]
};

__global__ void __launch_bounds__(256) dnv_pass(const DnvPassArgs A)
{
    __shared__ float4 s_e[kDnvT * kDnvT];
    __shared__ float4 s_g0[kDnvT * kDnvT];
    __shared__ float4 s_g1[kDnvT * kDnvT];
    // block -> residue class (rx, ry) and block (bx, by) of that class's sub-image, as dn_pass
    const u32 rx = blockIdx.x % A.cx, bx = blockIdx.x / A.cx;
    const u32 ry = blockIdx.y % A.cy, by = blockIdx.y / A.cy;
    const u32 s = A.step;
    const size_t np = (size_t)A.nw * A.nh;
    for (u32 t = threadIdx.x; t < kDnvT * kDnvT; t += 256u) {
        const u32 lj = t / kDnvT, li = t - lj * kDnvT;
        const long long si = (long long)(bx * kDnvB + li) - 2, sj = (long long)(by * kDnvB + lj) - 2;
        const long long fx = (long long)rx + (long long)s * si, fy = (long long)ry + (long long)s * sj;
        float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g0 = e, g1 = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        if (si >= 0 && sj >= 0 && fx < (long long)A.nw && fy < (long long)A.nh) {
            const size_t p = (size_t)fy * A.nw + (size_t)fx;
            g0 = A.guide[p];
            g1 = A.guide[np + p];
            e = A.e_in[p];
        }
        s_e[t] = e; s_g0[t] = g0; s_g1[t] = g1;
    }
    __syncthreads();
    const u32 li = threadIdx.x & 15u, lj = threadIdx.x >> 4;
    if ((unsigned long long)rx + (unsigned long long)s * (bx * kDnvB + li) >= A.nw ||
        (unsigned long long)ry + (unsigned long long)s * (by * kDnvB + lj) >= A.nh) return;
    const u32 fx = rx + s * (bx * kDnvB + li), fy = ry + s * (by * kDnvB + lj);
    const u32 c = (lj + 2u) * kDnvT + li + 2u;
    const DnGuide gp = dnv_guide_of(s_g0[c], s_g1[c]);
    const float4 ep4 = s_e[c];
    const float ep[3] = {ep4.x, ep4.y, ep4.z};
    DnvBlur vb;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const u32 k = (u32)((int)(lj + 2u) + dy) * kDnvT + (u32)((int)(li + 2u) + dx);
            if (s_g1[k].w < 0.0f) continue;                // outside the frame
            vb.add(dx, dy, s_e[k].w);
        }
    const float b = vb.result(), lp = dnv_lum(ep);
    DnvAcc acc;
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const u32 k = (u32)((int)(lj + 2u) + dy) * kDnvT + (u32)((int)(li + 2u) + dx);
            const float4 eq4 = s_e[k];
            const float eq[3] = {eq4.x, eq4.y, eq4.z};
            acc.add(dnv_tap_weight(dn_k5(dx) * dn_k5(dy), lp, dnv_lum(eq), b, gp, dnv_guide_of(s_g0[k], s_g1[k]), A.sv, A.sn, A.sp), eq, eq4.w);
        }
    float r[3], v;
    acc.result(ep, ep4.w, r, v);
    const size_t p = (size_t)fy * A.nw + fx;
    if (A.last) {
        for (u32 ch = 0; ch < 3u; ++ch) A.out[3 * p + ch] = r[ch] * dn_demod(A.albedo[3 * p + ch], gp.hit, A.env != 0u);
    } else {
        A.e_out[p] = make_float4(r[0], r[1], r[2], v);
    }
}

// ---- launcher (declared in mrt_kernels.h) ----
hipError_t launch_denoise_var(const MeanSrc &S, const float *half, const float *guide, const float *albedo, u32 nh, u32 passes,
                              float sv, float sn, float sp, float firefly, float *e0, float *e1, float *out, hipStream_t stream, bool env)
{
    if (passes == 0u || !half || !S.tile_count) return hipErrorInvalidValue;
    const u32 nw = S.nw;
    float4 *buf[2] = {reinterpret_cast<float4 *>(e0), reinterpret_cast<float4 *>(e1)};
    const dim3 frame((nw + kDnvB - 1u) / kDnvB, (nh + kDnvB - 1u) / kDnvB);
    DnvArgs V;
    V.nw = nw; V.nh = nh; V.env = env ? 1u : 0u;
    V.f = firefly; V.sn = sn; V.sp = sp;
    V.accum = S.sums; V.half = half; V.tile_count = S.tile_count; V.albedo = albedo;
    V.guide = reinterpret_cast<const float4 *>(guide);
    V.in = nullptr; V.out = buf[0];
    hipLaunchKernelGGL(dnv_prep, frame, dim3(256), 0, stream, V);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    V.in = buf[0]; V.out = buf[1];
    hipLaunchKernelGGL(dnv_init, frame, dim3(256), 0, stream, V);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    for (u32 i = 0; i < passes; ++i) {
        DnvPassArgs A;
        A.nw = nw; A.nh = nh; A.step = 1u << i;
        A.cx = A.step < nw ? A.step : nw;
        A.cy = A.step < nh ? A.step : nh;
        A.last = i + 1u == passes; A.env = V.env;
        A.sv = sv; A.sn = sn; A.sp = sp;
        A.e_in = buf[(i + 1u) & 1u]; A.e_out = buf[i & 1u];
        A.albedo = albedo; A.guide = V.guide;
        A.out = out;
        const u32 sw = (nw + A.step - 1u) / A.step, sh = (nh + A.step - 1u) / A.step;
        const dim3 grid(A.cx * ((sw + kDnvB - 1u) / kDnvB), A.cy * ((sh + kDnvB - 1u) / kDnvB));
        hipLaunchKernelGGL(dnv_pass, grid, dim3(256), 0, stream, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace mrt
