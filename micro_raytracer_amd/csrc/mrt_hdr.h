// mrt_hdr.h — per-element bodies of the linear float image (mrt_img_hdr): the mean radiance, or the denoiser's
// filtered means, resampled in f32 to the output resolution with no tone map and no quantisation.  Shared by the kernels of
// mrt_hdr.hip and, for the CPU-side unit tests, an x86 build (tests/emu/hdr_probe.cpp).
//
//   m[y][x][c]   = A[y][x][c] * rc[y][x]       rc = 1/count as the tone map forms it: the context's, or that of tile (x/8, y/8)
//                                              (filtered means: rc = 1.0f, m is c' itself)
//   t[oy][x][c]  = sum_i m[vl[oy]+i][x][c] * vw[oy][i]
//   u[oy][ox][c] = sum_i t[oy][hl[ox]+i][c] * hw[ox][i]
//   out          = u > 0 ? u : 0               negative filter lobes and NaN give 0, +inf stays
// f32, unfused (-ffp-contract=off), every sum from +0.0f with its taps added in index order; vertical first, as lanczos3_v/_h.
// Without a resize out = m > 0 ? m : 0.
#pragma once
#include "mrt_adapt.h"

namespace mrt {

// What the vertical pass reads is the MeanSrc of mrt_adapt.h (the sums and their 1/count); the x86 probe of the tests
// (tests/emu/hdr_probe.cpp) names it as the float image's own
using HdrSrc = MeanSrc;

// m of element e = x * 3 + c of source row y
MRT_HD float hdr_mean(const MeanSrc &S, u32 y, u32 e)
{
    const float rc = mean_rc(S, e / 3u, y);
    return S.sums[(size_t)y * S.nw * 3u + e] * rc;
}

MRT_HD float hdr_clamp(float u) { return u > 0.0f ? u : 0.0f; }

// t[oy0 .. oy0 + R)[e] of the vertical pass, rows past dh left out: one walk over the source rows the R outputs span, each mean
// formed once and added to every output whose taps hold that row -- per output still its own taps in index order from +0.0f.
template <u32 R>
MRT_HD void hdr_vertical(const MeanSrc &S, u32 e, u32 oy0, u32 dh, const u32 *left, const u32 *count, const float *weight, u32 cap, float *t)
{
    u32 l[R], n[R];
    u32 lo = 0xffffffffu, hi = 0u;
#pragma unroll
    for (u32 r = 0; r < R; ++r) {
        const bool in = oy0 + r < dh;
        l[r] = in ? left[oy0 + r] : 0u;
        n[r] = in ? count[oy0 + r] : 0u;
        t[r] = 0.0f;
        if (in && l[r] < lo) lo = l[r];
        if (in && l[r] + n[r] > hi) hi = l[r] + n[r];
    }
    for (u32 s = lo; s < hi; ++s) {
        const float m = hdr_mean(S, s, e);
#pragma unroll
        for (u32 r = 0; r < R; ++r) {
            const u32 i = s - l[r];                            // wraps below the first tap: then i >= n[r]
            if (i < n[r]) t[r] += m * weight[(size_t)(oy0 + r) * cap + i];
        }
    }
}

// out[0..3) of output column ox from row t[sw][3] of the vertical pass
MRT_HD void hdr_horizontal(const float *trow, u32 l, u32 n, const float *w, float *out)
{
    float u0 = 0.0f, u1 = 0.0f, u2 = 0.0f;
    for (u32 i = 0; i < n; ++i) {
        const float *p = trow + (size_t)(l + i) * 3u;
        u0 += p[0] * w[i]; u1 += p[1] * w[i]; u2 += p[2] * w[i];
    }
    out[0] = hdr_clamp(u0); out[1] = hdr_clamp(u1); out[2] = hdr_clamp(u2);
}

}  // namespace mrt
