// mrt_adaptive.cpp — tile-adaptive sampling: mrt_execute_adaptive, mrt_radiance_adaptive, mrt_sample_counts,
// mrt_adapt_half.
#include <chrono>
#include <utility>
#include <vector>

#include "mrt_ctx.h"

using namespace mrt;
using namespace mrt::api;

// ---- adaptive sampling ---------------------------------------------------------------------------------------------------------
// rk: the rounds trace rk's caller-supplied rays (mrt_radiance_adaptive) in place of the camera's; everything else is shared
static int adapt_run(mrt_ctx *c, const mrt_adapt *a, mrt_adapt_info *info, RaysKernel *rk = nullptr)
{
    const u32 nw = c->pk.nw, nh = c->pk.nh, n_tx = (nw + 7u) / 8u, n_ty = (nh + 7u) / 8u, n_tiles = n_tx * n_ty;
    const size_t acc_floats = plane_floats(c);
    if (!c->ad) {
        std::unique_ptr<Adaptive> ad(new Adaptive());
        HIP_TRY(ad->half.alloc(acc_floats));
        HIP_TRY(ad->tiles.alloc(5u * (size_t)n_tiles + 1u));
        ad->n_tiles = n_tiles;
        c->ad = std::move(ad);
    }
    Adaptive &ad = *c->ad;
    u32 *lists[2] = {ad.tiles.p, ad.tiles.p + n_tiles};
    u32 *keep = ad.tiles.p + 2u * (size_t)n_tiles, *tcount = ad.counts(), *tconv = ad.tiles.p + 4u * (size_t)n_tiles;
    u32 *d_n = ad.tiles.p + 5u * (size_t)n_tiles;
    std::vector<u32> all(n_tiles);
    for (u32 t = 0; t < n_tiles; ++t) all[t] = t;
    HIP_TRY(hipMemcpy(lists[0], all.data(), n_tiles * sizeof(u32), hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(c->d_accum, 0, acc_floats * sizeof(float), c->stream.get()));
    HIP_TRY(hipMemsetAsync(ad.half.p, 0, acc_floats * sizeof(float), c->stream.get()));
    HIP_TRY(hipMemsetAsync(tcount, 0, 2u * (size_t)n_tiles * sizeof(u32), c->stream.get()));
    if (c->count_segments) HIP_TRY(hipMemsetAsync(c->segments.p, 0, sizeof(unsigned long long), c->stream.get()));
    u32 n_active = n_tiles, n = 0, rounds = 0, cur = 0;
    while (n_active) {
        for (int r = 0; r < 2; ++r, ++rounds, n += a->step) {
            // one round over the tiles still running; even rounds go through the chunk planes, whose sums are added, in chunk
            // order, to the accumulator and to the half buffer alike.  The adaptive path reports the largest split as k_split.
            const bool even = (rounds & 1u) == 0u;
            const TileList tl{lists[cur], n_active};
            u32 k_split = 1;
            const int rc = launch_batch(c, n, a->step, &tl, even ? ad.half.p : nullptr, even, k_split, c->stats.k_split, rk);
            if (rc) return rc;
        }
        if (n < a->min_samples) continue;
        // the stop rule at count n for every tile still running; the next list, and its length (the one read-back of a step)
        HIP_TRY(launch_adapt_eval(c->d_accum, ad.half.p, lists[cur], n_active, nw, nh, n, a->threshold, n >= a->max_samples, keep, tcount, tconv,
                                  lists[cur ^ 1u], d_n, c->stream.get()));
        HIP_TRY(hipMemcpyAsync(&n_active, d_n, sizeof(u32), hipMemcpyDeviceToHost, c->stream.get()));
        HIP_TRY(hipStreamSynchronize(c->stream.get()));
        cur ^= 1u;
    }
    std::vector<u32> conv(n_tiles);
    ad.tile_count.assign(n_tiles, 0u);
    HIP_TRY(hipMemcpy(ad.tile_count.data(), tcount, n_tiles * sizeof(u32), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(conv.data(), tconv, n_tiles * sizeof(u32), hipMemcpyDeviceToHost));
    uint64_t samples = 0;
    u32 lo = 0xffffffffu, hi = 0, n_conv = 0;
    for (u32 t = 0; t < n_tiles; ++t) {
        const u32 ty = t / n_tx, tx = t - ty * n_tx;
        const u32 px = ((nw - tx * 8u) < 8u ? nw - tx * 8u : 8u) * ((nh - ty * 8u) < 8u ? nh - ty * 8u : 8u);
        const u32 k = ad.tile_count[t];
        samples += (uint64_t)k * px;
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
        n_conv += conv[t] ? 1u : 0u;
    }
    c->count = lo;
    c->adaptive = true;
    c->adaptive_rays = rk != nullptr;
    c->stats.samples = samples;
    c->stats_pending = true;
    if (info) {
        int rc = resolve_stats(c);
        if (rc) return rc;
        info->samples = samples;
        info->rounds = rounds;
        info->launches = c->stats.launches;
        info->tiles = n_tiles;
        info->tiles_converged = n_conv;
        info->min_count = lo;
        info->max_count = hi;
        info->kernel_ms = c->stats.kernel_ms;
    }
    return MRT_OK;
}

// The rules of mrt_adapt, shared by both adaptive calls (fn: the caller's name in the message)
static int adapt_rule(const mrt_adapt *a, const char *fn)
{
    const unsigned long long two = 2ull * a->step;
    if (a->step == 0u || a->step % kChunk) return fail(MRT_ERR_ARG, "%s: step %u is not a positive multiple of %u", fn, a->step, kChunk);
    if (a->min_samples == 0u || a->min_samples % two || a->max_samples == 0u || a->max_samples % two)
        return fail(MRT_ERR_ARG, "%s: min_samples %u and max_samples %u must be positive multiples of 2 * step = %llu", fn, a->min_samples, a->max_samples, two);
    if (a->min_samples > a->max_samples) return fail(MRT_ERR_ARG, "%s: min_samples %u > max_samples %u", fn, a->min_samples, a->max_samples);
    if (!(a->threshold >= 0.0f)) return fail(MRT_ERR_ARG, "%s: threshold %g is not >= 0", fn, (double)a->threshold);
    return MRT_OK;
}

// ... and their precondition: one device, no samples held or booked
static int adapt_state(const mrt_ctx *c, const char *fn)
{
    if (c->group || c->shard_count > 1u) return fail(MRT_ERR_STATE, "%s: sharded and multi-device contexts are not supported", fn);
    if (c->adaptive || c->count || c->pending || c->full.p)
        return fail(MRT_ERR_STATE, "%s: the context holds samples (an adaptive render starts from none): mrt_reset first", fn);
    return MRT_OK;
}

static void adapt_begin(mrt_ctx *c)
{
    la_drop(c);
    reset_exec_stats(c);
    c->stats.k_split = 1; c->stats.deferred = 0;
}

// A failed adaptive run leaves nothing half done behind: the context is an empty uniform one again
static int adapt_rollback(mrt_ctx *c, int rc)
{
    return keep_first_error(rc, [&] {
        (void)hipStreamSynchronize(c->stream.get());
        (void)hipMemsetAsync(c->d_accum, 0, plane_floats(c) * sizeof(float), c->stream.get());      // on the stream the next launch runs on
        (void)hipStreamSynchronize(c->stream.get());
        (void)hipGetLastError();
        c->adaptive = false; c->adaptive_rays = false; c->count = 0; c->stats_pending = false; c->ev_used = 0;
    });
}

extern "C" {

int mrt_execute_adaptive(mrt_ctx *c, const mrt_adapt *a, mrt_adapt_info *info, double *seconds)
{
    if (!c || !a) return fail(MRT_ERR_ARG, "mrt_execute_adaptive: null argument");
    int rc;
    if ((rc = adapt_rule(a, "mrt_execute_adaptive")) || (rc = adapt_state(c, "mrt_execute_adaptive"))) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = set_device(c))) return rc;
    adapt_begin(c);
    if ((rc = adapt_run(c, a, info))) return adapt_rollback(c, rc);
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ok();
    return MRT_OK;
}

// mrt_execute_adaptive on one caller-supplied ray per supersampled pixel: the same rounds, rule and state, the
// trace launches on the supplied rays (pt_rays_tiles)
int mrt_radiance_adaptive(mrt_ctx *c, const mrt_rays_adapt *r, mrt_adapt_info *info, double *seconds)
{
    if (!c || !r || !r->orig || !r->dir) return fail(MRT_ERR_ARG, "mrt_radiance_adaptive: null argument");
    int rc;
    if ((rc = adapt_rule(&r->rule, "mrt_radiance_adaptive"))) return rc;
    if ((rc = rays_words(r->flags, r->reserved, "mrt_radiance_adaptive"))) return rc;
    if ((rc = adapt_state(c, "mrt_radiance_adaptive"))) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = set_device(c))) return rc;
    RaysKernel k;
    if ((rc = rays_kernel(c, k))) return rc;
    // the rays on the device: the caller's own, or one upload for the whole call
    DeviceRays rays;
    HIP_TRY(rays.take(r->orig, r->dir, (size_t)c->pk.nw * c->pk.nh, (r->flags & MRT_RAYS_DEVICE) != 0u));
    k.orig = rays.orig; k.dir = rays.dir;
    // the kernel writes what the frame kernel of an adaptive render writes: the context's accumulator, chunk planes and counters
    k.P.to_planes = 0u;
    k.P.accum = c->d_accum;
    k.P.count_segments = c->count_segments ? 1u : 0u; k.P.segments = c->segments.p;
    k.P.tile_counter = nullptr; k.P.persist_grid = 0u; k.P.band_items = 0u;
    adapt_begin(c);
    if ((rc = adapt_run(c, &r->rule, info, &k))) return adapt_rollback(c, rc);
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ok();
    return MRT_OK;
}

int mrt_sample_counts(mrt_ctx *c, uint32_t *counts)
{
    if (!c || !counts) return fail(MRT_ERR_ARG, "mrt_sample_counts: null argument");
    if (const int rc = enter(c)) return rc;
    const u32 nw = c->pk.nw, nh = c->pk.nh;
    const u32 uniform = frame_of(c).count;
    for (u32 y = 0; y < nh; ++y)
        for (u32 x = 0; x < nw; ++x) counts[(size_t)y * nw + x] = c->adaptive ? c->ad->tile_count[tile_index(nw, x, y)] : uniform;
    ok();
    return MRT_OK;
}

int mrt_adapt_half(mrt_ctx *c, float *rgb)
{
    if (!c || !rgb) return fail(MRT_ERR_ARG, "mrt_adapt_half: null argument");
    if (!c->adaptive) return fail(MRT_ERR_STATE, "mrt_adapt_half: no adaptive render on this context since its last reset");
    if (const int rc = set_device(c)) return rc;
    HIP_TRY(hipMemcpy(rgb, c->ad->half.p, (size_t)c->pk.nw * c->pk.nh * 3 * sizeof(float), hipMemcpyDeviceToHost));
    ok();
    return MRT_OK;
}

}  // extern "C"
