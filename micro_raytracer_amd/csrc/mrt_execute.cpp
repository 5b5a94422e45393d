// mrt_execute.cpp — mrt_execute and mrt_get_stats on one device: the launch loop every batch shares (uniform, adaptive,
// look-ahead), the sample split, the look-ahead of the eager per-call path, deferred execution, the lazy statistics.
// The functions defined here as mrt::api::name are the ones other units call: mrt_ctx.h declares them and says what they do.
#include <stdio.h>

#include <chrono>
#include <utility>

#include "mrt_ctx.h"
#include "mrt_rays_adapt.h"

using namespace mrt;
using namespace mrt::api;

namespace {

// Sample-split until the launch has ~25 rounds of 32 waves per CU: shorter wavefronts balance the tail of a launch (tiles
// differ in path length).  Measured on the 1080p x 1024 spp Cornell box (tests/gpu_shard_probe.py): whole frame 328 -> 315 ms
// with 4 lanes per pixel, one shard of 8 GPUs 47.1 -> 42.4 ms with 16; round 3, persistent 256-thread workgroups: 1 / 2 / 4 / 8
// lanes per pixel 292.9 / 274.7 / 267.7 / 265.7 ms, hence a split of 8 at 1080p (the target was 120 000 wavefronts: 4).
// The split says whether a launch goes through the chunk planes and is what mrt_stats reports.  The items of such a launch are
// the split's interleaved chunk phases -- 8 chunks each at 1080p x 1024 samples -- only under MRT_K_SPLIT and in the kernels
// that are no band kernels (mrt_inst.h); a band kernel's launch is cut into tapered bands of contiguous chunks instead
// (plan_bands, mrt_plan.cpp: 31, 16, 8, 4, 2, 1, 1, 1 chunks there), which keeps the long items' fuller wavefronts and
// drains the launch at single chunks: 190.8 -> 187.0 ms.
constexpr unsigned long long kSplitTargetWaves = 200000ull;
// A sample-split launch writes one f32x3 chunk sum per pixel per 16 samples; the buffer is bounded by cutting one
// mrt_execute into several launches of at most this many sample chunks (1024 samples) and this many bytes.  Launch
// boundaries are chunk boundaries, so the canonical accumulation order -- and every bit -- is unchanged.
constexpr u32 kMaxChunksPerLaunch = 64u;
constexpr size_t kPartialBudgetBytes = (size_t)4u << 30;

}  // namespace

// ---- the statistics of one execute: the lazy half --------------------------------------------------------------------------------
int mrt::api::resolve_stats(mrt_ctx *c)
{
    if (!c->stats_pending) return MRT_OK;
    c->stats_pending = false;
    int rc = set_device(c);
    if (rc) return rc;
    double k = 0, r = 0;
    for (u32 i = 0; i + 2u < c->ev_used; i += 3u) {
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, c->evs[i].get(), c->evs[i + 1].get()));
        HIP_TRY(hipEventElapsedTime(&b, c->evs[i + 1].get(), c->evs[i + 2].get()));
        k += a; r += b;
    }
    c->stats.kernel_ms = k;
    c->stats.reduce_ms = c->stats.k_split > 1u ? r : 0.0;
    if (c->count_segments) {
        unsigned long long seg = 0;
        HIP_TRY(hipMemcpy(&seg, c->segments.p, sizeof seg, hipMemcpyDeviceToHost));
        c->stats.segments = seg;
    }
    if (c->knobs.debug_fallbacks) {
        unsigned long long t[3] = {0, 0, 0};
        HIP_TRY(hipMemcpy(t, c->segments.p + 5, sizeof t, hipMemcpyDeviceToHost));
        fprintf(stderr, "[mrt fallbacks] since mrt_create: NaN directions (shortcut) %llu, walk area full %llu, rays the triangle BVH may not cull %llu\n", t[0], t[1], t[2]);
    }
#ifdef MRT_PHASE_TIMING
    {   // debug build: shader-clock ticks per phase, summed over wavefronts since the context was created
        unsigned long long t[4] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpy(t, c->segments.p + 2, sizeof t, hipMemcpyDeviceToHost));
        const double tot = (double)(t[0] + t[1] + t[2] + t[3]);
        fprintf(stderr, "[mrt phase ticks] closest-hit query %.3f  shading %.3f  shadow query %.3f  ray set-up / regeneration %.3f  (total %.4g wave-ticks)\n",
                t[0] / tot, t[1] / tot, t[2] / tot, t[3] / tot, tot);
    }
#endif
    return MRT_OK;
}

// Lanes per pixel (k_split) and sample chunks per launch (cap) of a batch of n_chunks chunks over wave_tiles 8x8 tiles;
// (re)allocates the chunk planes the split needs.  planes: the batch must go through the chunk planes (k_split >= 2 even for
// a single chunk: the adaptive even rounds, whose chunk sums are added to the half buffer too) -- MRT_ERR_LIMIT without them.
static int split_policy(mrt_ctx *c, unsigned long long wave_tiles, u32 n_chunks, bool planes, u32 &k_split, u32 &cap)
{
    k_split = 1;
    // (a frame of 100 000 wave tiles or more -- 4K -- has its 25 rounds without splitting: CornellBox2 at 3840x2160 loses 1.6 %
    // to a second lane per pixel, 985 -> 1001 ms)
    const unsigned long long split_target = wave_tiles >= 100000ull ? 0ull : kSplitTargetWaves;
    while (k_split * 2u <= n_chunks && k_split < 16u && wave_tiles * k_split < split_target) k_split *= 2u;
    if (c->knobs.k_split) { k_split = c->knobs.k_split; while (k_split > n_chunks) k_split /= 2u; }
    if (planes && k_split < 2u) k_split = 2u;
    const size_t plane = plane_floats(c);
    cap = kMaxChunksPerLaunch;                           // chunks per launch
    if (c->knobs.max_chunks) cap = c->knobs.max_chunks;
    size_t budget = kPartialBudgetBytes;
    if (c->knobs.partial_budget) budget = c->knobs.partial_budget;
    if (k_split > 1u) {
        if (cap < k_split) cap = k_split;
        while (cap > k_split && plane * cap * sizeof(float) > budget) cap /= 2u;
        const size_t need = plane * (n_chunks < cap ? n_chunks : cap);
        if (need * sizeof(float) > budget) k_split = 1u;                       // not even k_split planes fit: one lane per pixel
        else if (need > c->partial.n && !hip_tolerated(c->partial.alloc(need, c->knobs.partial_fail_alloc ? (size_t)1 << 60 : 0))) k_split = 1u;
    }
    if (planes && k_split < 2u) return fail(MRT_ERR_LIMIT, "mrt_execute_adaptive: no memory for the chunk planes of a round");
    return MRT_OK;
}

// One trace launch of P on `stream`: the tile counter P draws from is reset first when the launch is persistent (before ev0, so
// the kernel time leaves the reset out), then ev0, launch_pt, ev1 (null events are not recorded).  tl: a tile-list launch.
// rk: the trace launch is pt_rays_tiles on rk's rays over tl (mrt_radiance_adaptive) instead of the context's own kernel.
static int launch_trace(mrt_ctx *c, const Params &P, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const TileList *tl, const RaysKernel *rk = nullptr)
{
    if (c->plan.block_threads > 64u && P.persist_grid) HIP_TRY(hipMemsetAsync(P.tile_counter, 0, sizeof(u32), stream));
    if (ev0) HIP_TRY(hipEventRecord(ev0, stream));
    if (rk) HIP_TRY(launch_rays_tiles(P, rk->in_lds, rk->inst, *tl, rk->orig, rk->dir, stream));
    else HIP_TRY(launch_pt(P, c->plan.block_threads, c->plan.in_lds, c->pk.features, stream, tl));
    if (ev1) HIP_TRY(hipEventRecord(ev1, stream));
    return MRT_OK;
}

int mrt::api::launch_batch(mrt_ctx *c, u32 base, u32 n, const TileList *tl, float *half, bool planes, u32 &k_split, u32 &ks_max, RaysKernel *rk)
{
    Params &P = rk ? rk->P : c->P;                   // the launch's arguments: the context's own, or those of the supplied-ray kernel
    const u32 n_chunks = (base + n - 1u) / kChunk - base / kChunk + 1u;
    // sample split: spread a small frame over more wavefronts, one lane per (pixel, every k-th sample chunk)
    const unsigned long long wave_tiles = tl ? tl->n : (unsigned long long)((c->pk.nw + 7) / 8) * ((c->local_rows + 7) / 8);
    u32 cap = kMaxChunksPerLaunch;
    int rc = split_policy(c, wave_tiles, n_chunks, planes, k_split, cap);
    if (rc) return rc;
    const size_t plane = plane_floats(c);
    P.partial = c->partial.p;
    P.partial_stride = plane;
    const u32 s_end = base + n;
    while (base < s_end) {
        // this launch: samples [base, stop), stop on a chunk boundary (or the end); k_split == 1 needs no buffer: one launch
        u32 stop = s_end;
        if (k_split > 1u) {
            const unsigned long long lim = ((unsigned long long)(base / kChunk) + cap) * kChunk;
            if (lim < stop) stop = (u32)lim;
        }
        const u32 nc = (stop - 1u) / kChunk - base / kChunk + 1u;
        u32 ks = k_split;
        while (ks > nc) ks /= 2u;
        if (planes && ks < 2u) ks = 2u;                  // (a lane of chunk phase >= nc has nothing to do)
        P.n_samples = stop - base;
        P.sample_base = base;
        P.k_split = ks;
        if (ks > ks_max) ks_max = ks;
        while (c->event_timing && c->evs.size() < (size_t)c->ev_used + 3u) { Event e; HIP_TRY(create(e)); c->evs.push_back(std::move(e)); }
        const Event *ev = c->event_timing ? &c->evs[c->ev_used] : nullptr;
        P.persist_grid = (rk || (c->plan.small_plain_grid && stop - base < kChunk)) ? 0u : c->persist_grid;     // (pt_rays_tiles: a plain grid)
        // Tapered items: a persistent launch through the chunk planes of a band kernel cuts its nc
        // chunks into contiguous bands, longest first, instead of ks interleaved phases.  An explicit MRT_K_SPLIT keeps the phases.
        P.band_items = 0u;
        if (ks > 1u && !c->knobs.k_split && P.persist_grid && c->plan.block_threads > 64u
            && band_kernel(c->plan.in_lds, (int)c->plan.block_threads, c->plan.inst)) {
            const Bands b = plan_bands(nc, wave_tiles, (unsigned long long)c->persist_grid * (c->plan.block_threads / 64u), c->knobs);
            P.band_items = b.items; P.n_bands = b.n; P.band_tail = b.tail;
            for (u32 i = 0; i < kMaxBands; ++i) { P.band_first[i] = b.first[i]; P.band_len[i] = b.len[i]; }
        }
        if ((rc = launch_trace(c, P, c->stream.get(), ev ? ev[0].get() : nullptr, ev ? ev[1].get() : nullptr, tl, rk))) return rc;
        if (ks > 1u) {
            if (tl) HIP_TRY(launch_reduce_chunks_listed(c->d_accum, half, c->partial.p, tl->tiles, tl->n, c->pk.nw, c->pk.nh, plane, nc, c->stream.get()));
            else HIP_TRY(launch_reduce_chunks(c->d_accum, c->partial.p, (size_t)c->local_rows * c->pk.nw * 3, plane, nc, c->stream.get()));
        }
        if (ev) { HIP_TRY(hipEventRecord(ev[2].get(), c->stream.get())); c->ev_used += 3u; }
        c->stats.launches += 1u;
        base = stop;
    }
    return MRT_OK;
}

void mrt::api::reset_exec_stats(mrt_ctx *c)
{
    c->stats.kernel_ms = 0; c->stats.reduce_ms = 0; c->stats.gather_ms = 0; c->stats.launches = 0; c->stats.samples = 0; c->stats.segments = 0;
    c->stats_pending = false; c->ev_used = 0;
}

int mrt::api::exec_launch(mrt_ctx *c, uint32_t n_samples)
{
    int rc = set_device(c);
    if (rc) return rc;
    reset_exec_stats(c);
    if (!(n_samples && c->local_rows)) return MRT_OK;
    if (c->count_segments) HIP_TRY(hipMemsetAsync(c->segments.p, 0, sizeof(unsigned long long), c->stream.get()));
    u32 ks_max = 0;                                  // (the uniform path reports the policy's k_split)
    if ((rc = launch_batch(c, c->count, n_samples, nullptr, nullptr, false, c->stats.k_split, ks_max))) return rc;
    return MRT_OK;
}

int mrt::api::exec_finish(mrt_ctx *c, uint32_t n_samples)
{
    int rc = set_device(c);
    if (rc) return rc;
    if (n_samples && c->local_rows) {
        HIP_TRY(hipStreamSynchronize(c->stream.get()));
        c->stats.samples = (uint64_t)c->local_rows * c->pk.nw * n_samples;
        c->stats_pending = true;
    }
    c->count += n_samples;                                        // src/sampler.rs:76
    return MRT_OK;
}

// ---- look-ahead of the eager per-call path -----------------------------------------------------------------------------------
// The reference's callers run ONE Sampler::execute per sample and wait for it (src/cli.rs:162-170, src/http.rs:141-144).  A
// one-sample launch cannot regenerate paths inside a lane (a wavefront lasts as long as its longest path: lane utilisation
// 0.65 against 0.70, 0.36 ms per 1080p pass against 0.25 inside a batched launch), and the image is a pure function of (scene,
// seed, sample index) -- so a context that sees one-sample calls arrive back to back traces AHEAD: samples [k, k + n) in one
// launch on a second stream, every sample into a plane of its own (Params.to_planes), and each call
// only folds its sample's plane into the accumulator (reduce_chunks, 0.02 ms) and waits for that.  The accumulator holds
// exactly the samples the caller has asked for at every return, added one by one in index order -- bit for bit what the plain
// per-call loop leaves there -- so observing it (mrt_accum, mrt_img, a bound or handed-out pointer) needs no special case.  Two
// plane sets: while one is folded call by call, the next launch already runs.  It starts at the third consecutive
// one-sample call with two samples per launch and doubles up to la_max (32), so a caller that stops early wastes at most about
// the work it has used; any other call (n != 1, reset, set_accum) drops what was traced ahead.
void mrt::api::la_drop(mrt_ctx *c)
{
    if (c->la && (c->la->n[0] || c->la->n[1])) (void)hipStreamSynchronize(c->la->stream.get());
    if (c->la) c->la->n[0] = c->la->n[1] = 0;
    c->la_streak = 0;
}

// launch the trace of samples [base, base + n) into plane set i (asynchronous, on the look-ahead stream, created by the first call)
static int la_launch(mrt_ctx *c, int i, u32 base, u32 n)
{
    const size_t plane = plane_floats(c);
    if (!c->la) {
        std::unique_ptr<Lookahead> la(new Lookahead());
        HIP_TRY(create(la->stream));
        for (int k = 0; k < 2; ++k) { HIP_TRY(create(la->ev0[k])); HIP_TRY(create(la->ev1[k])); }
        HIP_TRY(la->counter.alloc(1));
        c->la = std::move(la);
    }
    Lookahead &la = *c->la;
    if (plane * n > la.planes[i].n && !hip_tolerated(la.planes[i].alloc(plane * n))) return MRT_ERR_LIMIT;     // the caller falls back
    Params P = c->P;
    P.n_samples = n; P.sample_base = base; P.k_split = 1u; P.to_planes = 1u; P.band_items = 0u;
    P.partial = la.planes[i].p; P.partial_stride = plane;
    P.count_segments = 0u;
    // small scenes: the plain grid (their persistent grid fills every wave slot of the chip and would keep the folds out until
    // the launch has ended); larger ones leave slots free and keep their persistent workgroups, with a tile counter of their own
    P.persist_grid = c->plan.small_plain_grid ? 0u : c->persist_grid;
    P.tile_counter = la.counter.p;
    const int rc = launch_trace(c, P, la.stream.get(), la.ev0[i].get(), la.ev1[i].get(), nullptr);
    if (rc) return rc;
    la.base[i] = base; la.n[i] = n;
    return MRT_OK;
}

// one eager one-sample call served from the look-ahead planes; returns MRT_ERR_LIMIT when the planes cannot be had (the caller
// then runs the plain launch from here on) and kLaPlain when the two sets would reach past sample index 0xffffffff (the caller
// runs the plain launch for this call only)
constexpr int kLaPlain = 1;
static int run_lookahead(mrt_ctx *c)
{
    int rc = set_device(c);
    if (rc) return rc;
    const u32 k = c->count;
    int s = -1;
    if (c->la) for (int i = 0; i < 2; ++i) if (c->la->n[i] && k >= c->la->base[i] && k < c->la->base[i] + c->la->n[i]) s = i;
    if (s < 0) {
        // nothing traced ahead for this sample (first use, or what was ahead has been dropped): start both sets
        la_drop(c);
        c->la_streak = 2;
        const u32 n0 = 2u < c->la_max ? 2u : c->la_max;
        const u32 n1 = 2u * n0 < c->la_max ? 2u * n0 : c->la_max;
        if ((unsigned long long)k + n0 + n1 > 0xffffffffull) return kLaPlain;      // (a set's base + n must not wrap)
        if ((rc = la_launch(c, 0, k, n0))) return rc;
        if ((rc = la_launch(c, 1, k + n0, n1))) { (void)hipStreamSynchronize(c->la->stream.get()); c->la->n[0] = c->la->n[1] = 0; return rc; }
        s = 0;
    }
    Lookahead &la = *c->la;
    const size_t plane = plane_floats(c);
    const size_t words = (size_t)c->local_rows * c->pk.nw * 3;
    HIP_TRY(hipStreamWaitEvent(c->stream.get(), la.ev1[s].get(), 0));
    HIP_TRY(launch_reduce_chunks(c->d_accum, la.planes[s].p + (size_t)(k - la.base[s]) * plane, words, plane, 1u, c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));                // the fold has run, so the set's launch has ended too
    c->count += 1u;
    reset_exec_stats(c);
    c->stats.launches = 1u; c->stats.k_split = 1u;
    c->stats.samples = (uint64_t)c->local_rows * c->pk.nw;
    if (c->event_timing) {
        float ms = 0;
        if (hip_tolerated(hipEventElapsedTime(&ms, la.ev0[s].get(), la.ev1[s].get()))) c->stats.kernel_ms = (double)ms / (double)la.n[s];   // this sample's share of its launch
    }
    if (k + 1u == la.base[s] + la.n[s]) {
        // the set is spent (its last plane has been folded): the next launch goes into it, behind the other set's, twice as long
        const int o = 1 - s;
        const unsigned long long nb = (unsigned long long)la.base[o] + la.n[o];
        const u32 nn = 2u * la.n[o] < c->la_max ? 2u * la.n[o] : c->la_max;
        la.n[s] = 0;
        if (la.n[o] && nb + nn <= 0xffffffffull) (void)la_launch(c, s, (u32)nb, nn);      // (a failure here only means a later call starts over)
    }
    return MRT_OK;
}

static int run_samples(mrt_ctx *c, uint32_t n_samples)
{
    int rc;
    if (c->group) return exec_group(c, n_samples);
    if (c->la_enabled && n_samples == 1u && c->local_rows) {
        if (c->la_streak >= 2u) {
            rc = run_lookahead(c);
            if (rc == MRT_ERR_LIMIT) c->la_enabled = false;      // no memory for the planes: the plain per-call launch from here on
            else if (rc != kLaPlain) return rc;                  // (kLaPlain: this call only, at the top of the sample range)
        } else {
            ++c->la_streak;
        }
    } else {
        la_drop(c);
    }
    if ((rc = exec_launch(c, n_samples))) return rc;
    return exec_finish(c, n_samples);
}

int mrt::api::settle(mrt_ctx *c)
{
    if (!c->pending) return MRT_OK;
    const u32 n = c->pending;
    c->pending = 0;
    return run_samples(c, n);
}
constexpr u32 kDeferLimit = 1024u;        // booked samples that trigger a launch by themselves (one full-size batch)

int mrt::api::enter(mrt_ctx *c)
{
    const int rc = set_device(c);
    return rc ? rc : settle(c);
}

extern "C" {

int mrt_execute(mrt_ctx *c, uint32_t n_samples, double *seconds)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_execute: null context");
    if (c->adaptive) return fail(MRT_ERR_STATE, "mrt_execute: the context holds an adaptive render (per-tile sample counts): mrt_reset first");
    if ((unsigned long long)c->count + c->pending + n_samples > 0xffffffffull) return fail(MRT_ERR_LIMIT, "mrt_execute: sample count overflows u32");
    const auto t0 = std::chrono::steady_clock::now();
    int rc = MRT_OK;
    const bool deferred = c->defer && !c->exposed();
    if (deferred) {
        c->pending += n_samples;
        if (c->pending >= kDeferLimit) rc = settle(c);
    } else {
        rc = run_samples(c, n_samples);
    }
    if (rc) return rc;
    c->stats.deferred = deferred ? 1u : 0u;       // whether THIS call was booked (MRT_FLAG_DEFER honoured) or ran at once
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ok();
    return MRT_OK;
}

int mrt_get_stats(mrt_ctx *c, mrt_stats *out)
{
    if (!c || !out) return fail(MRT_ERR_ARG, "mrt_get_stats: null argument");
    if (c->pending) { const int rc = enter(c); if (rc) return rc; }      // an observation: booked samples are traced first
    if (c->stats_pending) { const int rc = resolve_stats(c); if (rc) return rc; }
    *out = c->stats;
    ok();
    return MRT_OK;
}

}  // extern "C"
