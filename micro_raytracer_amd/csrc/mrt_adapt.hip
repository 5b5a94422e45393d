// mrt_adapt.hip — gfx950 kernels of adaptive sampling (mrt_execute_adaptive).
//
//   pt_megakernel<.., TileList>   pt_megakernel (mrt_pt_kernel.h) over a list of 8x8 wave tiles (the tiles still running); its
//                         144 instantiations are compiled here, next to the 144 ordinary ones of mrt_kernels.hip
//   reduce_chunks_listed  reduce_chunks over the listed tiles, into the accumulator and (even rounds) the half buffer
//   adapt_eval            the stop rule (mrt_adapt.h) per listed tile, one wavefront per tile
//   adapt_compact         the next tile list, in list order
// (tonemap_tiles_u8, the tone map with each tile's own count, stands next to tonemap_u8 in mrt_kernels.hip)
//
// Build: as mrt_kernels.hip.
#include <hip/hip_runtime.h>

#include "mrt_adapt.h"
#include "mrt_kernels.h"
#include "mrt_pt_kernel.h"

namespace mrt {

// One wavefront per listed 8x8 tile, lane = pixel: wave tile list[blockIdx.x] -> this lane's accumulator word; false for lanes
// outside the frame
__device__ inline bool listed_pixel(const u32 *list, u32 nw, u32 nh, u32 &word)
{
    const u32 n_tx = (nw + 7u) >> 3, tile = list[blockIdx.x], lane = threadIdx.x;
    const u32 ty = tile / n_tx, tx = tile - ty * n_tx;
    const u32 x = tx * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);
    word = (y * nw + x) * 3u;
    return x < nw && y < nh;
}

// reduce_chunks over the listed tiles only (the chunk planes of unlisted tiles hold stale data): acc += chunk sums in chunk
// order; half (the even rounds' sum H, may be null) receives the same chunk sums in the same order
__global__ void __launch_bounds__(64) reduce_chunks_listed(float *__restrict__ accum, float *__restrict__ half, const float *__restrict__ partial,
                                                           const u32 *__restrict__ list, u32 nw, u32 nh, size_t stride, u32 n_chunks)
{
    u32 w;
    if (!listed_pixel(list, nw, nh, w)) return;
    for (u32 c = 0; c < 3u; ++c) {
        float a = accum[w + c];
        for (u32 j = 0; j < n_chunks; ++j) a += partial[(size_t)j * stride + w + c];
        accum[w + c] = a;
        if (half) {
            float h = half[w + c];
            for (u32 j = 0; j < n_chunks; ++j) h += partial[(size_t)j * stride + w + c];
            half[w + c] = h;
        }
    }
}

// The stop rule at count n for every listed tile (mrt_adapt.h): tile_count[tile] = n, tile_conv[tile] = e_tile <= threshold,
// keep[i] = the tile runs on (not converged, and not `last`).  Wave max of the lanes' errors; a NaN error never converges.
__global__ void __launch_bounds__(64) adapt_eval(const float *__restrict__ accum, const float *__restrict__ half, const u32 *__restrict__ list,
                                                 u32 nw, u32 nh, u32 n, float threshold, u32 last, u32 *__restrict__ keep,
                                                 u32 *__restrict__ tile_count, u32 *__restrict__ tile_conv)
{
    u32 w;
    float e = 0.0f;
    if (listed_pixel(list, nw, nh, w)) e = adapt_pixel_error(accum + w, half + w, adapt_recip(n), adapt_recip(n / 2u));
    const bool any_nan = __builtin_amdgcn_ballot_w64(e != e) != 0ull;
    float m = e != e ? 0.0f : e;
    for (int off = 32; off > 0; off >>= 1) { const float o = __shfl_xor(m, off, 64); m = o > m ? o : m; }
    if (threadIdx.x == 0) {
        const bool conv = adapt_converged(m, any_nan, threshold);
        const u32 tile = list[blockIdx.x];
        tile_count[tile] = n;
        tile_conv[tile] = conv ? 1u : 0u;
        keep[blockIdx.x] = (!conv && !last) ? 1u : 0u;
    }
}

// out = the entries list[i] with keep[i] != 0, in list order (ascending stays ascending); *n_out = their number.  One
// workgroup of 1024 threads walks the list in blocks: ballot per wavefront, wave offsets through LDS.
__global__ void __launch_bounds__(1024) adapt_compact(const u32 *__restrict__ list, const u32 *__restrict__ keep, u32 n, u32 *__restrict__ out,
                                                      u32 *__restrict__ n_out)
{
    __shared__ u32 wave_n[16];
    __shared__ u32 base_s;
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) base_s = 0u;
    __syncthreads();
    for (u32 b = 0; b < n; b += 1024u) {
        const u32 i = b + threadIdx.x;
        const bool k = i < n && keep[i] != 0u;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(k);
        if (lane == 0) wave_n[wave] = (u32)__builtin_popcountll(m);
        __syncthreads();
        u32 off = base_s;
        for (u32 v = 0; v < wave; ++v) off += wave_n[v];
        if (k) out[off + (u32)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = list[i];
        __syncthreads();
        if (threadIdx.x == 0) { u32 t = 0; for (u32 v = 0; v < 16u; ++v) t += wave_n[v]; base_s += t; }
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_out = base_s;
}

// ---- launchers (declared in mrt_kernels.h) ----
hipError_t launch_pt_list(const Params &P, const TileList &TL, dim3 grid, size_t lds, u32 block_threads, bool scene_in_lds, u32 inst, hipStream_t stream)
{
    return launch_pt_inst(P, grid, lds, block_threads, scene_in_lds, inst, stream, TL);
}

hipError_t configure_pt_list(size_t max_lds_bytes) { return configure_pt_inst<TileList>(max_lds_bytes); }

hipError_t launch_reduce_chunks_listed(float *accum, float *half, const float *partial, const u32 *list, u32 n_listed, u32 nw, u32 nh,
                                       size_t stride, u32 n_chunks, hipStream_t stream)
{
    if (!n_listed) return hipSuccess;
    hipLaunchKernelGGL(reduce_chunks_listed, dim3(n_listed), dim3(64), 0, stream, accum, half, partial, list, nw, nh, stride, n_chunks);
    return hipGetLastError();
}

hipError_t launch_adapt_eval(const float *accum, const float *half, const u32 *list, u32 n_listed, u32 nw, u32 nh, u32 n, float threshold, bool last,
                             u32 *keep, u32 *tile_count, u32 *tile_conv, u32 *list_out, u32 *n_out, hipStream_t stream)
{
    if (n_listed) hipLaunchKernelGGL(adapt_eval, dim3(n_listed), dim3(64), 0, stream, accum, half, list, nw, nh, n, threshold, last ? 1u : 0u, keep, tile_count, tile_conv);
    hipLaunchKernelGGL(adapt_compact, dim3(1), dim3(1024), 0, stream, list, keep, n_listed, list_out, n_out);
    return hipGetLastError();
}

}  // namespace mrt
