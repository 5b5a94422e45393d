// mrt_kernels.hip — gfx950 kernels of libmrt_hip.so.
//
//   pt_megakernel    Sampler::execute (reference src/sampler.rs:28-78) and everything of src/rt.rs
//                    it reaches: one lane per supersampled pixel, all samples of the launch in
//                    registers, scene staged in LDS, one accumulator read-modify-write per launch.
//   (pt_megakernel<.., TileList>, the same over a list of 8x8 tiles, and the other kernels of adaptive sampling: mrt_adapt.hip)
//   tonemap_u8       Sampler::img's per-pixel map (src/sampler.rs:84-96); tonemap_tiles_u8: with each 8x8 tile's own sample count
//   lanczos3_v/_h    image::imageops::resize(.., Lanczos3) (src/sampler.rs:98): vertical pass to f32,
//                    horizontal pass to u8, taps precomputed on the host.
//   math_selftest    elementwise device math contract, for the parity tests.
//
// Build: hipcc --offload-arch=gfx950 -ffp-contract=off (no fast-math; IEEE divide / sqrt).
#include <hip/hip_runtime.h>

#include "mrt_kernels.h"
#include "mrt_megakernel.h"
#include "mrt_post.h"
#include "mrt_pt_kernel.h"
#include "mrt_trace.h"

namespace mrt {

// acc[p] += chunk sums in chunk order (the canonical order of mrt_trace.h), one thread per accumulator word
__global__ void __launch_bounds__(256) reduce_chunks(float *__restrict__ accum, const float *__restrict__ partial, size_t n_words,
                                                     size_t stride, u32 n_chunks)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_words) return;
    float a = accum[i];
    for (u32 j = 0; j < n_chunks; ++j) a += partial[(size_t)j * stride + i];
    accum[i] = a;
}

// rows of the gathered shard accumulators -> their place in the frame (multi-device contexts)
__global__ void __launch_bounds__(256) scatter_rows(float *__restrict__ frame, const float *__restrict__ gathered, const u32 *__restrict__ rowmap,
                                                    u32 n_rows, u32 row_words)
{
    const u32 r = blockIdx.y;
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows || i >= row_words) return;
    const u32 y = rowmap[r];
    if (y == 0xffffffffu) return;
    frame[(size_t)y * row_words + i] = gathered[(size_t)r * row_words + i];
}

__global__ void __launch_bounds__(256) tonemap_u8(const float *__restrict__ accum, unsigned char *__restrict__ out,
                                                  u32 n_px, float rc, float gamma, float wexp)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_px) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(size_t)i * 3 + k] = tonemap_channel(accum[(size_t)i * 3 + k], rc, gamma, wexp);
}

// tonemap_u8 with each pixel's own count: rc = 1/count of its 8x8 wave tile (adaptive renders)
__global__ void __launch_bounds__(256) tonemap_tiles_u8(const float *__restrict__ accum, unsigned char *__restrict__ out, const u32 *__restrict__ tile_count,
                                                        u32 nw, u32 nh, float gamma, float wexp)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nw * nh) return;
    const u32 y = i / nw, x = i - y * nw;
    const float rc = adapt_recip(tile_count[tile_index(nw, x, y)]);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(size_t)i * 3 + k] = tonemap_channel(accum[(size_t)i * 3 + k], rc, gamma, wexp);
}

// vertical_sample of image 0.24: out[oy][x][c] = sum_i src[left+i][x][c] * w[i], f32, taps in order
__global__ void __launch_bounds__(256) lanczos3_v(const unsigned char *__restrict__ src, float *__restrict__ dst, u32 sw, u32 dh,
                                                  const u32 *__restrict__ left, const u32 *__restrict__ count,
                                                  const float *__restrict__ weight, u32 cap)
{
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;      // element = x * 3 + c
    const u32 oy = blockIdx.y;
    if (e >= sw * 3u || oy >= dh) return;
    const u32 l = left[oy], n = count[oy];
    const float *w = weight + (size_t)oy * cap;
    float t = 0.0f;
    for (u32 i = 0; i < n; ++i) t += (float)src[(size_t)(l + i) * sw * 3u + e] * w[i];
    dst[(size_t)oy * sw * 3u + e] = t;
}

// horizontal_sample: clamp to [0,255], round half away from zero, u8
__global__ void __launch_bounds__(256) lanczos3_h(const float *__restrict__ src, unsigned char *__restrict__ dst, u32 sw, u32 dw, u32 dh,
                                                  const u32 *__restrict__ left, const u32 *__restrict__ count,
                                                  const float *__restrict__ weight, u32 cap)
{
    const u32 ox = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 y = blockIdx.y;
    if (ox >= dw || y >= dh) return;
    const u32 l = left[ox], n = count[ox];
    const float *w = weight + (size_t)ox * cap;
    float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
    for (u32 i = 0; i < n; ++i) {
        const float *p = src + ((size_t)y * sw + (l + i)) * 3u;
        t0 += p[0] * w[i]; t1 += p[1] * w[i]; t2 += p[2] * w[i];
    }
    unsigned char *q = dst + ((size_t)y * dw + ox) * 3u;
    q[0] = resample_to_u8(t0); q[1] = resample_to_u8(t1); q[2] = resample_to_u8(t2);
}

__global__ void math_selftest(int op, const float *a, const float *b, float *out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = a[i], y = b ? b[i] : 0.0f;
    float s, c, r = 0.0f;
    switch (op) {
    case 0: sincos_(x, s, c); r = s; break;
    case 1: sincos_(x, s, c); r = c; break;
    case 2: r = acos_(x); break;
    case 3: r = atan2_(x, y); break;
    case 4: r = pow_(x, y); break;
    case 5: r = recip_(x); break;
    case 6: r = sqrt_(x); break;
    case 7: r = div_(x, y); break;
    case 8: r = fmax_(x, y); break;
    case 9: r = fmin_(x, y); break;
    case 10: r = u2f((u32)total_key(x)); break;
    case 11: r = u32_to_unit(draw_u32(f2u(x), f2u(y))); break;
    case 12: r = norm(v3(x, y, 0.25f)).x; break;
    default: break;
    }
    out[i] = r;
}

// Exhaustive / randomised comparison of the wave-uniform fast cores of mrt_math.h (sqrt_, recip_, div_, recip_sqrt_)
// with the compiler's full IEEE expansions, on the device.  Inputs are generated from the element index:
//   op 0 sqrt, op 1 recip: x = the bit pattern `first + i` (a sweep of 2^32 indices covers every f32)
//   op 2 divide, op 3 norm scale (1 / sqrt(x*x + y*y + z*z) as norm() computes it): operands hashed from (seed, first + i);
//        three wavefronts in four draw exponents inside the fast window (so the cores run), the fourth draws raw
//        bit patterns (zeros, denormals, infinities, NaNs: the fallback runs).
// A NaN result matches any NaN (payloads are not part of the contract).  Counts mismatches; keeps one example.
__device__ inline float sweep_operand(u32 h, bool windowed)
{
    if (!windowed) return u2f(h);
    const u32 e = 127u - 40u + (h >> 9) % 80u;                   // exponent field inside [2^-40, 2^40)
    return u2f((h & 0x80000000u) | (e << 23) | (mix32(h) & 0x7fffffu));
}
__global__ void __launch_bounds__(256) math_sweep(int op, unsigned long long first, unsigned long long n, u32 seed,
                                                  unsigned long long *mismatches, float *example)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long idx = first + i;
    const bool windowed = ((idx >> 6) & 3ull) != 3ull;           // per wavefront, so that the wave-uniform fast path is taken
    const u32 k = mix32((u32)idx ^ seed) + (u32)(idx >> 32) * kGold;
    float a = 0.0f, b = 0.0f, c = 0.0f, fast = 0.0f, ref = 0.0f;
    switch (op) {
    case 0: a = u2f((u32)idx); fast = sqrt_(a); ref = __builtin_sqrtf(a); break;
    case 1: a = u2f((u32)idx); fast = recip_(a); ref = 1.0f / a; break;
    case 2: a = sweep_operand(mix32(k + 1u), windowed); b = sweep_operand(mix32(k + 2u), windowed); fast = div_(a, b); ref = a / b; break;
    case 3: {
        a = sweep_operand(mix32(k + 1u), windowed); b = sweep_operand(mix32(k + 2u), windowed); c = sweep_operand(mix32(k + 3u), windowed);
        const float m = a * a + b * b + c * c;
        fast = recip_sqrt_(m); ref = 1.0f / __builtin_sqrtf(m);
        break;
    }
    default: break;
    }
    const bool same = f2u(fast) == f2u(ref) || (fast != fast && ref != ref);
    if (!same) {
        if (atomicAdd(mismatches, 1ull) == 0ull) { example[0] = a; example[1] = b; example[2] = fast; example[3] = ref; }
    }
}

// ---- launchers (declared in mrt_kernels.h); the instantiations: mrt_megakernel.h, which of them serves a scene and its LDS: mrt_inst.h ----
hipError_t launch_pt(const Params &P, u32 block_threads, bool scene_in_lds, u32 features, hipStream_t stream, const TileList *TL)
{
    if (block_threads != P.tiles_x * P.tiles_y * 64u) return hipErrorInvalidConfiguration;
    const u32 tile_w = P.tiles_x * 8u, tile_h = P.tiles_y * 8u;
    const u32 items = P.band_items ? P.band_items : P.k_split;      // items per tile: bands (persistent band-kernel launches) or chunk phases
    if (P.band_items && !(block_threads > 64u && P.persist_grid)) return hipErrorInvalidConfiguration;
    dim3 grid((P.nw + tile_w - 1) / tile_w, (P.local_rows + tile_h - 1) / tile_h, items);
    if (TL) {                                // tile-list launch: one wavefront per listed tile, list entries packed along x
        if (!TL->n) return hipSuccess;
        const u32 per_wg = P.tiles_x * P.tiles_y;
        grid = dim3((TL->n + per_wg - 1) / per_wg, 1, items);
    }
    if (block_threads > 64u && P.persist_grid) {
        const unsigned long long n_wg = (unsigned long long)grid.x * grid.y * grid.z;
        grid = dim3((unsigned)(n_wg < P.persist_grid ? n_wg : P.persist_grid), 1, 1);
    }
    const size_t lds = pt_lds_bytes(P, block_threads, scene_in_lds, features);
    const u32 inst = pt_instantiation(block_threads, scene_in_lds, features);
    if (TL) return launch_pt_list(P, *TL, grid, lds, block_threads, scene_in_lds, inst, stream);
    return launch_pt_inst(P, grid, lds, block_threads, scene_in_lds, inst, stream);
}

hipError_t configure_pt(size_t max_lds_bytes)
{
    const hipError_t e = configure_pt_inst<>(max_lds_bytes);
    return e != hipSuccess ? e : configure_pt_list(max_lds_bytes);
}

hipError_t launch_reduce_chunks(float *accum, const float *partial, size_t n_words, size_t stride, u32 n_chunks, hipStream_t stream)
{
    hipLaunchKernelGGL(reduce_chunks, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, stream, accum, partial, n_words, stride, n_chunks);
    return hipGetLastError();
}

hipError_t launch_scatter_rows(float *frame, const float *gathered, const u32 *rowmap, u32 n_rows, u32 row_words, hipStream_t stream)
{
    hipLaunchKernelGGL(scatter_rows, dim3((row_words + 255) / 256, n_rows), dim3(256), 0, stream, frame, gathered, rowmap, n_rows, row_words);
    return hipGetLastError();
}

hipError_t launch_tonemap(const MeanSrc &S, unsigned char *out, u32 nh, float gamma, float wexp, hipStream_t stream)
{
    const u32 n_px = S.nw * nh;
    if (S.tile_count) hipLaunchKernelGGL(tonemap_tiles_u8, dim3((n_px + 255) / 256), dim3(256), 0, stream, S.sums, out, S.tile_count, S.nw, nh, gamma, wexp);
    else hipLaunchKernelGGL(tonemap_u8, dim3((n_px + 255) / 256), dim3(256), 0, stream, S.sums, out, n_px, S.rc, gamma, wexp);
    return hipGetLastError();
}

hipError_t launch_lanczos_v(const unsigned char *src, float *dst, u32 sw, u32 dh, const DevTaps &v, hipStream_t stream)
{
    hipLaunchKernelGGL(lanczos3_v, dim3((sw * 3u + 255) / 256, dh), dim3(256), 0, stream, src, dst, sw, dh, v.left, v.count, v.weight, v.cap);
    return hipGetLastError();
}

hipError_t launch_lanczos_h(const float *src, unsigned char *dst, u32 sw, u32 dw, u32 dh, const DevTaps &h, hipStream_t stream)
{
    hipLaunchKernelGGL(lanczos3_h, dim3((dw + 255) / 256, dh), dim3(256), 0, stream, src, dst, sw, dw, dh, h.left, h.count, h.weight, h.cap);
    return hipGetLastError();
}

hipError_t launch_math_selftest(int op, const float *a, const float *b, float *out, size_t n, hipStream_t stream)
{
    hipLaunchKernelGGL(math_selftest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, op, a, b, out, n);
    return hipGetLastError();
}

hipError_t launch_math_sweep(int op, unsigned long long first, unsigned long long n, u32 seed, unsigned long long *mismatches, float *example, hipStream_t stream)
{
    hipLaunchKernelGGL(math_sweep, dim3((unsigned)((n + 255ull) / 256ull)), dim3(256), 0, stream, op, first, n, seed, mismatches, example);
    return hipGetLastError();
}

}  // namespace mrt
