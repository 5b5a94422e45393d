// mrt_adapt.h — per-pixel and per-tile bodies of the adaptive-sampling stop rule (mrt_execute_adaptive), and what
// its per-tile counts make of a frame's means: MeanSrc, the one statement of a pixel's 1/count.
// Shared by the kernels, the host units and, for the CPU-side unit tests, an x86 build.
//
// A tile that has traced n samples per pixel holds A (the sum of all n) and H (the sum of its even-numbered rounds: n/2
// samples).  Its error compares the two means, relative to the square root of the pixel's brightness:
//   rc = 1/n, rh = 1/(n/2);  I = A * rc, J = H * rh
//   e_pixel = ((|I_r - J_r| + |I_g - J_g|) + |I_b - J_b|) / (1e-4 + sqrt((I_r + I_g) + I_b))
//   e_tile  = max over the tile's in-frame pixels; a NaN e_pixel makes the tile unconverged
// f32, in exactly this order (-ffp-contract=off; IEEE division and square root), so that numpy can restate it bit for bit.
#pragma once
#include "mrt_math.h"

namespace mrt {

// 1/n as the tone map forms it for a count n (mrt_accum.cpp img_tonemap: 1.0f / (float)count)
MRT_HD float adapt_recip(u32 n) { return 1.0f / (float)n; }

// the 8x8 tile of pixel (x, y) in the per-tile tables of an nw pixels wide frame (fewer tiles than pixels: 32 bits hold it)
MRT_HD u32 tile_index(u32 nw, u32 x, u32 y) { return (y >> 3) * ((nw + 7u) >> 3) + (x >> 3); }

// A frame's mean radiance as every consumer of it reads it (tone map, denoisers, linear float image): sums [nh][nw][3] with one
// 1/count, or -- tile_count not null, after an adaptive render -- with the counts of the 8x8 tiles.  Finished means: rc = 1.0f.
struct MeanSrc {
    const float *sums;
    float rc;
    const u32 *tile_count;
    u32 nw;
};

// 1/count of pixel (x, y)
MRT_HD float mean_rc(const MeanSrc &S, u32 x, u32 y) { return S.tile_count ? adapt_recip(S.tile_count[tile_index(S.nw, x, y)]) : S.rc; }

// e_pixel of one pixel: a, h = its three A and H words; rc = adapt_recip(n), rh = adapt_recip(n / 2)
MRT_HD float adapt_pixel_error(const float *a, const float *h, float rc, float rh)
{
    const float ir = a[0] * rc, ig = a[1] * rc, ib = a[2] * rc;
    const float jr = h[0] * rh, jg = h[1] * rh, jb = h[2] * rh;
    const float num = (fabs_(ir - jr) + fabs_(ig - jg)) + fabs_(ib - jb);
    return num / (1e-4f + sqrt_((ir + ig) + ib));
}

// the stop test of one tile: e_max = max of its pixels' errors without NaNs, any_nan = some pixel's error is NaN
MRT_HD bool adapt_converged(float e_max, bool any_nan, float threshold) { return !any_nan && e_max <= threshold; }

// e_tile of wave tile (tx, ty) of an nw x nh frame of [nh][nw][3] sums at count n, pixel by pixel (the evaluation kernel
// forms the same maximum with a wave reduction; max is exact, so the order does not matter).  *any_nan: a pixel's error is NaN
MRT_HD float adapt_tile_error(const float *A, const float *H, u32 nw, u32 nh, u32 tx, u32 ty, u32 n, bool *any_nan)
{
    const float rc = adapt_recip(n), rh = adapt_recip(n / 2u);
    float e_max = 0.0f;
    bool nan = false;
    for (u32 j = 0; j < 64u; ++j) {
        const u32 x = tx * 8u + (j & 7u), y = ty * 8u + (j >> 3);
        if (x >= nw || y >= nh) continue;
        const size_t w = ((size_t)y * nw + x) * 3u;
        const float e = adapt_pixel_error(A + w, H + w, rc, rh);
        if (e != e) nan = true;
        else if (e > e_max) e_max = e;
    }
    *any_nan = nan;
    return e_max;
}

}  // namespace mrt
