// mrt_pt_kernel.h — the path-tracing kernel and the host side of its instantiations.  ONE template for both tile sources: the
// ordinary launches (mrt_kernels.hip: pt_megakernel<b, T, F>, every tile of the shard) and the tile-list launches of adaptive
// sampling (mrt_adapt.hip: pt_megakernel<b, T, F, TileList>, with the list as a third kernel argument).  The tile source is a
// trailing parameter pack, empty or one TileList, so the ordinary kernel keeps its name and its argument block, and the body is
// the kernel's own: a body or a staging prologue moved into a shared device function changes the register allocation of the
// headline kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "mrt_megakernel.h"      // waves_for, lds_stash_for, the instantiation lists
#include "mrt_trace.h"

namespace mrt {

// The tile source of a launch: tile i of `all` (no list: the tiles of the shard in row-major order), or entry i of a TileList
__device__ inline u32 tile_count(u32 all) { return all; }
__device__ inline u32 tile_count(u32, const TileList &TL) { return TL.n; }
__device__ inline u32 tile_at(u32 i) { return i; }
__device__ inline u32 tile_at(u32 i, const TileList &TL) { return TL.tiles[i]; }

template <bool SCENE_IN_LDS, int BLOCK_THREADS, u32 FEAT, class... Tiles>
__global__ void __launch_bounds__(BLOCK_THREADS, waves_for(FEAT, BLOCK_THREADS)) pt_megakernel(const Params P, const u32 *__restrict__ blob_g, const Tiles... TL)
{
    extern __shared__ uint4 lds_blob[];
    const float *F;
    // words of the scene this workgroup stages: all of it, or (F_COLD) the hot prefix -- records, transforms, materials, node
    // arrays; triangles, membership tables and texels are then read from global memory
    const u32 staged_words = !SCENE_IN_LDS ? 0u : staged_words_for(P, FEAT);
    if (SCENE_IN_LDS) {
        const uint4 *g = reinterpret_cast<const uint4 *>(P.blob);
        const u32 n4 = staged_words >> 2;
        for (u32 i = threadIdx.x; i < n4; i += blockDim.x) lds_blob[i] = g[i];
        __syncthreads();
        F = reinterpret_cast<const float *>(lds_blob);
    } else {
        F = reinterpret_cast<const float *>(P.blob);
    }

    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    Scn S;
    S.F = F;
    S.U = F;
    S.G = reinterpret_cast<const float *>(blob_g);
    S.P = &P;
    // behind the staged scene (16-byte aligned): [lane stash: ST_SLOTS x blockDim floats] [walk areas: P.walk_cap x blockDim words]
    const u32 stash_base4 = (staged_words + 3u) >> 2;
    constexpr bool kStash = lds_stash_for(SCENE_IN_LDS, BLOCK_THREADS, FEAT);
    S.wk = nullptr; S.wk_stride = BLOCK_THREADS;
    if constexpr (has_walk_area(FEAT))
        S.wk = (void *)(reinterpret_cast<float *>(lds_blob + stash_base4) + (kStash ? stash_slots_for(FEAT, BLOCK_THREADS) * BLOCK_THREADS : 0u) + threadIdx.x);
    u32 segments = 0;
#ifdef MRT_PHASE_TIMING
    unsigned long long wave_ticks[4] = {0ull, 0ull, 0ull, 0ull};
#endif
    // The band kernels (mrt_inst.h): an item of a launch with Params.band_items is (band, tile) -- chunks [first, first + len) of
    // the tile, from the band table or, behind the listed bands, one chunk -- and a lane traces its pixel's chunks of the band
    constexpr bool kBands = band_kernel(SCENE_IN_LDS, BLOCK_THREADS, FEAT);
    // one 8x8 tile of shard-local rows for this wavefront, lane k of the sample split (band kernels: item k of the tile)
    auto do_tile = [&](u32 tx, u32 ty, u32 k) {
        const u32 x = tx * 8u + (lane & 7u);
        const u32 ry = ty * 8u + (lane >> 3);
        // shard-local row -> frame row: row block b of this shard is frame row block b * shard_count + shard_index
        const u32 blk = ry / P.shard_rows;
        const u32 y = (blk * P.shard_count + P.shard_index) * P.shard_rows + (ry - blk * P.shard_rows);
        const bool active = x < P.nw && ry < P.local_rows && y < P.nh;
        u32 seg = 0;
        LaneJob job;
        if constexpr (kBands) {
            BandJobs jobs;
            jobs.stride = P.k_split;
            jobs.end = (P.sample_base + P.n_samples - 1u) / kChunk - P.sample_base / kChunk + 1u;      // the launch's chunks
            if (P.band_items) {
                const bool listed = k < P.n_bands;
                const u32 len = listed ? P.band_len[k] : 1u;
                k = listed ? P.band_first[k] : P.band_tail + (k - P.n_bands);
                jobs.stride = 1u;
                jobs.end = k + len;
            }
            if (!active) return;
            job.k = k;
            job.word = (ry * P.nw + x) * 3u;        // < 2^32: mrt_create limits a shard to 2^30 pixels
            LdsStash<BLOCK_THREADS> st;
            st.base = (lds_vfloat *)(reinterpret_cast<float *>(lds_blob + stash_base4) + threadIdx.x);
#ifdef MRT_PHASE_TIMING
            unsigned long long tk[4] = {0ull, 0ull, 0ull, 0ull};
#else
            unsigned long long *tk = nullptr;
#endif
            render_pixel<FEAT, LdsStash<BLOCK_THREADS>, CameraRays, BandJobs>(S, st, x, y, job, seg, tk, CameraRays(), jobs);
#ifdef MRT_PHASE_TIMING
            for (int i = 0; i < 4; ++i) wave_ticks[i] += tk[i];
#endif
            segments += seg;
            return;
        }
        if (!active) return;
        job.k = k;
        job.word = (ry * P.nw + x) * 3u;        // < 2^32: mrt_create limits a shard to 2^30 pixels
        if constexpr (lds_stash_for(SCENE_IN_LDS, BLOCK_THREADS, FEAT)) {
            // per-lane column behind the scene blob (16-byte aligned): ST_SLOTS x blockDim floats
#ifdef MRT_PHASE_TIMING
            unsigned long long tk[4] = {0ull, 0ull, 0ull, 0ull};
#else
            unsigned long long *tk = nullptr;
#endif
            LdsStash<BLOCK_THREADS> st;
            st.base = (lds_vfloat *)(reinterpret_cast<float *>(lds_blob + stash_base4) + threadIdx.x);
            render_pixel<FEAT>(S, st, x, y, job, seg, tk);
#ifdef MRT_PHASE_TIMING
            for (int k = 0; k < 4; ++k) wave_ticks[k] += tk[k];
#endif
        } else {
            RegStash st;
            render_pixel<FEAT>(S, st, x, y, job, seg);
        }
        segments += seg;
    };
    // Persistent workgroup (more than one wavefront, P.persist_grid set): its wavefronts draw tiles from a counter until the
    // launch is out of tiles, so a CU never waits for the slowest wavefront of a workgroup (whose LDS copy of the scene
    // would otherwise keep the next workgroup out).  Otherwise blockIdx addresses the one tile of each wavefront.
    // A tile-list launch maps its tile index i -- counter-drawn or blockIdx-addressed -- to TL.tiles[i].
    const bool persist = BLOCK_THREADS > 64 && P.persist_grid != 0u;
    const u32 n_tx = (P.nw + 7u) >> 3, n_ty = (P.local_rows + 7u) >> 3;
    const u32 per_k = tile_count(n_tx * n_ty, TL...), total = per_k * ((kBands && P.band_items) ? P.band_items : P.k_split);
    for (;;) {
        u32 tx = blockIdx.x * P.tiles_x + wave % P.tiles_x, ty = blockIdx.y * P.tiles_y + wave / P.tiles_x, k = blockIdx.z;
        if (persist) {
            u32 t = 0;
            if (lane == 0) t = atomicAdd(P.tile_counter, 1u);
            t = __builtin_amdgcn_readfirstlane(t);
            if (t >= total) break;
            k = t / per_k;
            const u32 r = tile_at(t - k * per_k, TL...);
            ty = r / n_tx;
            tx = r - ty * n_tx;
        } else if constexpr (sizeof...(Tiles) != 0) {
            // plain grid of a list launch: grid.x = ceil(n_listed / waves per workgroup), wavefront -> list entry
            const u32 i = blockIdx.x * (P.tiles_x * P.tiles_y) + wave;
            if (i >= per_k) break;
            const u32 r = tile_at(i, TL...);
            ty = r / n_tx;
            tx = r - ty * n_tx;
        }
        do_tile(tx, ty, k);
        if (!persist) break;
    }
#ifdef MRT_PHASE_TIMING
    // one lane per wavefront (the longest-running one speaks for the wave: every lane carries the wave's clock differences)
    for (int k = 0; k < 4; ++k) {
        unsigned long long v = wave_ticks[k];
        for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
        if (lane == 0 && v) atomicAdd(P.segments + 2 + k, v);
    }
#endif
    if (P.count_segments) {
        // wave-level sum (every lane of the wavefront is here), one atomic per wavefront
        u32 v = segments;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0 && v) atomicAdd(P.segments, (unsigned long long)v);
    }
}

// ---- host side of one tile source (the exported launchers are in mrt_kernels.hip / mrt_adapt.hip, each with its own 144 kernels)
// Launch instantiation `inst` (pt_instantiation) of a launch shape, grid and LDS bytes as launch_pt computed them; TL: the tile
// list of a tile-list launch, or nothing.  A shape without that instantiation is an invalid configuration.
template <class... Tiles>
inline hipError_t launch_pt_inst(const Params &P, dim3 grid, size_t lds, u32 block_threads, bool scene_in_lds, u32 inst, hipStream_t stream, const Tiles &...TL)
{
#define MRT_CASE(T, F) case (F): hipLaunchKernelGGL((pt_megakernel<true, T, (F), Tiles...>), grid, dim3(T), lds, stream, P, P.blob, TL...); return hipGetLastError();
#define MRT_CASE_L2(F) case (F): hipLaunchKernelGGL((pt_megakernel<false, 256, (F), Tiles...>), grid, dim3(256), lds, stream, P, P.blob, TL...); return hipGetLastError();
    if (!scene_in_lds) {
        if (block_threads != 256u) return hipErrorInvalidConfiguration;
        switch (inst) { MRT_SHAPES_L2 default: break; }
    } else if (block_threads == 64u) {
        switch (inst) { MRT_SHAPES_64 default: break; }
    } else if (block_threads == 256u) {
        switch (inst) { MRT_SHAPES_256 default: break; }
    } else if (block_threads == 512u) {
        switch (inst) { MRT_SHAPES_512 default: break; }
    } else if (block_threads == 1024u) {
        switch (inst) { MRT_SHAPES_1024 default: break; }
    }
#undef MRT_CASE
#undef MRT_CASE_L2
    return hipErrorInvalidConfiguration;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) for every scene-in-LDS instantiation of one tile source
template <class... Tiles>
inline hipError_t configure_pt_inst(size_t max_lds_bytes)
{
    const int b = (int)max_lds_bytes;
    hipError_t e;
#define MRT_CASE(T, F) \
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void *>(&pt_megakernel<true, T, (F), Tiles...>), hipFuncAttributeMaxDynamicSharedMemorySize, b)) != hipSuccess) return e;
    MRT_SHAPES_64 MRT_SHAPES_256 MRT_SHAPES_512 MRT_SHAPES_1024
#undef MRT_CASE
    return hipSuccess;
}

}  // namespace mrt
