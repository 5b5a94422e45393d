// mrt_gather.cpp — point gathers: mrt_gather, mrt_gather_rays.  Rays are formed on the device (gather_gen), traced by
// mrt_radiance's own kernel (launch_rays) and reduced per point (gather_reduce); only positions, normals and answers cross the
// host boundary.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "mrt_ctx.h"
#include "mrt_gather.h"

using namespace mrt;
using namespace mrt::api;

namespace {

constexpr u32 kBatchRays = 1u << 22;             // rays of a default batch: 40 B of workspace each
constexpr u32 kMaxRays = (1u << 30) - 1u;        // of any batch: launch_rays addresses its sums in u32 words
constexpr u32 kSegBlocks = 256u;                 // counter blocks of a call; batch b takes block b % kSegBlocks

// Everything of *g that both entry points refuse, in the order of mrt.h's list (out and first / count are the callers' own)
int gather_words_ok(const mrt_ctx *c, const mrt_gather_desc *g, const char *fn)
{
    if (!c || !g || !g->pos) return fail(MRT_ERR_ARG, "%s: null argument", fn);
    if (g->n == 0 || g->n >= ((size_t)1 << 30)) return fail(MRT_ERR_ARG, "%s: n = %zu is outside 1 .. 2^30 - 1", fn, g->n);
    if (g->n_dirs == 0 || g->n_dirs > 65536u) return fail(MRT_ERR_ARG, "%s: n_dirs = %u is outside 1 .. 65536", fn, g->n_dirs);
    if (g->n_samples == 0) return fail(MRT_ERR_ARG, "%s: n_samples = 0", fn);
    if ((unsigned long long)g->sample_base + g->n_samples > 0xffffffffull)
        return fail(MRT_ERR_ARG, "%s: samples [%u, + %u) reach past 2^32 - 1", fn, g->sample_base, g->n_samples);
    if (g->dist != MRT_GATHER_SPHERE && g->dist != MRT_GATHER_HEMI_COS) return fail(MRT_ERR_ARG, "%s: unknown dist %u", fn, g->dist);
    if (g->out != MRT_GATHER_MEAN && g->out != MRT_GATHER_SH9) return fail(MRT_ERR_ARG, "%s: unknown out %u", fn, g->out);
    if (g->out == MRT_GATHER_SH9 && g->dist != MRT_GATHER_SPHERE) return fail(MRT_ERR_ARG, "%s: MRT_GATHER_SH9 needs MRT_GATHER_SPHERE", fn);
    if (g->dist == MRT_GATHER_HEMI_COS && !g->normal) return fail(MRT_ERR_ARG, "%s: MRT_GATHER_HEMI_COS needs normal", fn);
    if (g->dist == MRT_GATHER_SPHERE && g->normal) return fail(MRT_ERR_ARG, "%s: MRT_GATHER_SPHERE takes no normal", fn);
    if (!(g->offset >= 0.0f) || !std::isfinite(g->offset)) return fail(MRT_ERR_ARG, "%s: offset %g is not finite and >= 0", fn, (double)g->offset);
    int rc;
    if ((rc = rays_words(g->flags, g->reserved, fn))) return rc;
    if (c->group) return fail(MRT_ERR_STATE, "%s: multi-device context", fn);
    return MRT_OK;
}

GatherSet gather_set(const mrt_ctx *c, const mrt_gather_desc *g)
{
    return {c->P.seed_lo, c->P.seed_hi, g->key_base, g->n_dirs, g->dist, g->offset};
}

// points per batch: whole points, the caller's number or the default, and never more rays than a launch addresses
u32 batch_points(const mrt_gather_desc *g, size_t points)
{
    const u32 want = g->batch_points ? g->batch_points : std::max(1u, kBatchRays / g->n_dirs);
    return (u32)std::min<size_t>(std::min(want, kMaxRays / g->n_dirs), points);
}

// pos and normal of the call on the device: the caller's pointers, or one upload each
struct DevicePoints {
    DeviceMem<float> up_p, up_n;
    const float *pos = nullptr, *normal = nullptr;
    hipError_t take(const mrt_gather_desc *g, bool on_device)
    {
        pos = g->pos; normal = g->normal;
        if (on_device) return hipSuccess;
        const size_t words = g->n * 3u;
        hipError_t e;
        if ((e = up_p.alloc(words)) || (e = hipMemcpy(up_p.p, g->pos, words * sizeof(float), hipMemcpyHostToDevice))) return e;
        pos = up_p.p;
        if (g->normal) {
            if ((e = up_n.alloc(words)) || (e = hipMemcpy(up_n.p, g->normal, words * sizeof(float), hipMemcpyHostToDevice))) return e;
            normal = up_n.p;
        }
        return hipSuccess;
    }
};

}  // namespace

extern "C" {

int mrt_gather(mrt_ctx *c, const mrt_gather_desc *g, float *out, mrt_gather_info *info)
{
    int rc;
    if ((rc = gather_words_ok(c, g, "mrt_gather"))) return rc;
    if (!out) return fail(MRT_ERR_ARG, "mrt_gather: null argument");
    if ((rc = set_device(c))) return rc;
    RaysKernel k;
    if ((rc = rays_kernel(c, k))) return rc;
    const bool dev = (g->flags & MRT_RAYS_DEVICE) != 0u;
    const size_t n = g->n;
    const u32 nd = g->n_dirs, W = gather_words(g->out);
    const u32 bp = batch_points(g, n);
    const size_t batches = (n + bp - 1u) / bp;
    const GatherSet gs = gather_set(c, g);
    DevicePoints pts;
    HIP_TRY(pts.take(g, dev));
    DeviceMem<float> d_out;
    float *res = out;
    if (!dev) {
        HIP_TRY(d_out.alloc(n * W));
        res = d_out.p;
    }
    // the workspace of one batch, allocated once: rays, keys and per-ray sums never leave the device
    const size_t ws_rays = (size_t)bp * nd;
    DeviceMem<float> w_o, w_d, w_s;
    DeviceMem<u32> w_k;
    HIP_TRY(w_o.alloc(ws_rays * 3u));
    HIP_TRY(w_d.alloc(ws_rays * 3u));
    HIP_TRY(w_s.alloc(ws_rays * 3u));
    HIP_TRY(w_k.alloc(ws_rays));
    // every batch brings its own counter block (alloc_counters' layout), as mrt_radiance brings one
    const u32 seg_blocks = (u32)std::min<size_t>(batches, kSegBlocks);
    DeviceMem<unsigned long long> d_seg;
    HIP_TRY(d_seg.alloc((size_t)seg_blocks * 8u));
    HIP_TRY(hipMemset(d_seg.p, 0, (size_t)seg_blocks * 8u * sizeof(unsigned long long)));
    Event ev[4];
    if (info)
        for (Event &e : ev) HIP_TRY(create(e));
    double gen_ms = 0.0, kernel_ms = 0.0, reduce_ms = 0.0;
    hipStream_t st = c->stream.get();
    k.P.n_samples = g->n_samples; k.P.sample_base = g->sample_base;
    k.P.k_split = 1u; k.P.to_planes = 0u;
    k.P.accum = w_s.p; k.P.partial = nullptr; k.P.partial_stride = 0ull;
    k.P.count_segments = 1u;
    k.P.tile_counter = nullptr; k.P.persist_grid = 0u;
    size_t b = 0;
    for (size_t first = 0; first < n; first += bp, ++b) {
        const u32 count = (u32)std::min<size_t>(bp, n - first);
        const u32 rays = count * nd;
        k.P.segments = d_seg.p + (b % seg_blocks) * 8u;
        if (info) HIP_TRY(hipEventRecord(ev[0].get(), st));
        HIP_TRY(launch_gather_gen(gs, pts.pos, pts.normal, (u32)first, count, w_o.p, w_d.p, w_k.p, st));
        HIP_TRY(hipMemsetAsync(w_s.p, 0, (size_t)rays * 3u * sizeof(float), st));
        if (info) HIP_TRY(hipEventRecord(ev[1].get(), st));
        HIP_TRY(launch_rays(k.P, k.in_lds, k.inst, rays, w_o.p, w_d.p, w_k.p, st));
        if (info) HIP_TRY(hipEventRecord(ev[2].get(), st));
        HIP_TRY(launch_gather_reduce(g->out, w_s.p, w_d.p, count, nd, g->n_samples, res + first * W, st));
        if (info) {
            // the events are reused by the next batch: read them now
            HIP_TRY(hipEventRecord(ev[3].get(), st));
            HIP_TRY(hipEventSynchronize(ev[3].get()));
            float t[3] = {0.0f, 0.0f, 0.0f};
            for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&t[i], ev[i].get(), ev[i + 1].get()));
            gen_ms += t[0]; kernel_ms += t[1]; reduce_ms += t[2];
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (!dev) HIP_TRY(hipMemcpy(out, d_out.p, n * W * sizeof(float), hipMemcpyDeviceToHost));
    if (info) {
        memset(info, 0, sizeof *info);
        std::vector<unsigned long long> seg((size_t)seg_blocks * 8u);
        HIP_TRY(hipMemcpy(seg.data(), d_seg.p, seg.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (u32 i = 0; i < seg_blocks; ++i) info->segments += seg[(size_t)i * 8u];
        info->gen_ms = gen_ms; info->kernel_ms = kernel_ms; info->reduce_ms = reduce_ms;
        info->rays = (uint64_t)n * nd;
        info->samples = info->rays * g->n_samples;
        info->batches = (uint32_t)batches;
        info->kernel_features = k.inst;
        info->scene_in_lds = k.in_lds ? 1u : 0u;
        info->lds_bytes = (uint32_t)k.lds;
    }
    ok();
    return MRT_OK;
}

int mrt_gather_rays(mrt_ctx *c, const mrt_gather_desc *g, size_t first, size_t count, float *orig, float *dir, uint32_t *key)
{
    int rc;
    if ((rc = gather_words_ok(c, g, "mrt_gather_rays"))) return rc;
    if (first > g->n || count > g->n - first)
        return fail(MRT_ERR_ARG, "mrt_gather_rays: points [%zu, + %zu) reach past n = %zu", first, count, g->n);
    if ((rc = set_device(c))) return rc;
    if (count == 0 || (!orig && !dir && !key)) { ok(); return MRT_OK; }
    const bool dev = (g->flags & MRT_RAYS_DEVICE) != 0u;
    const u32 nd = g->n_dirs;
    const u32 bp = batch_points(g, count);
    const GatherSet gs = gather_set(c, g);
    DevicePoints pts;
    HIP_TRY(pts.take(g, dev));
    // host outputs: one batch of each on the device, copied out batch by batch
    const size_t ws_rays = (size_t)bp * nd;
    DeviceMem<float> w_o, w_d;
    DeviceMem<u32> w_k;
    if (!dev) {
        if (orig) HIP_TRY(w_o.alloc(ws_rays * 3u));
        if (dir) HIP_TRY(w_d.alloc(ws_rays * 3u));
        if (key) HIP_TRY(w_k.alloc(ws_rays));
    }
    hipStream_t st = c->stream.get();
    for (size_t done = 0; done < count; done += bp) {
        const u32 cnt = (u32)std::min<size_t>(bp, count - done);
        const size_t at = done * nd, rays = (size_t)cnt * nd;
        float *po = !orig ? nullptr : dev ? orig + at * 3u : w_o.p;
        float *pd = !dir ? nullptr : dev ? dir + at * 3u : w_d.p;
        u32 *pk = !key ? nullptr : dev ? key + at : w_k.p;
        HIP_TRY(launch_gather_gen(gs, pts.pos, pts.normal, (u32)(first + done), cnt, po, pd, pk, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (!dev) {
            if (orig) HIP_TRY(hipMemcpy(orig + at * 3u, w_o.p, rays * 3u * sizeof(float), hipMemcpyDeviceToHost));
            if (dir) HIP_TRY(hipMemcpy(dir + at * 3u, w_d.p, rays * 3u * sizeof(float), hipMemcpyDeviceToHost));
            if (key) HIP_TRY(hipMemcpy(key + at, w_k.p, rays * sizeof(u32), hipMemcpyDeviceToHost));
        }
    }
    ok();
    return MRT_OK;
}

}  // extern "C"
