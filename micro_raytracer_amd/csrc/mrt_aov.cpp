// mrt_aov.cpp — first-hit AOVs and the denoisers on them: mrt_aov, mrt_aov_rays, mrt_denoise,
// mrt_img_denoised.
#include <string.h>

#include <utility>
#include <vector>

#include "mrt_ctx.h"
#include "mrt_denoise.h"

using namespace mrt;
using namespace mrt::api;

// The context's Aov state, allocated on first use
static int aov_state(mrt_ctx *c)
{
    if (!c->aov) {
        const size_t np = (size_t)c->pk.nw * c->pk.nh;
        std::unique_ptr<Aov> a(new Aov());
        HIP_TRY(a->guide.alloc(np * 8u));
        HIP_TRY(a->albedo.alloc(np * 3u));
        HIP_TRY(a->ids.alloc(np * 2u));
        HIP_TRY(alloc_counters(a->seg));
        for (Event &e : a->ev) HIP_TRY(create(e));
        c->aov = std::move(a);
    }
    return MRT_OK;
}

// What aov_compute and mrt_aov_rays share around their launch: the flat scene, the context's Aov state, and the Params of that
// scene with its blob and the AOV counter block ...
struct AovPass { const Packed *pk; Params P; };
static int aov_pass(mrt_ctx *c, AovPass &ap)
{
    const FlatScene fs = flat_scene(c);
    if (!fs.blob) return g_status;
    if (const int rc = aov_state(c)) return rc;
    ap.pk = &fs.pk;
    ap.P = fs.pk.P;
    ap.P.blob = fs.blob;
    ap.P.segments = c->aov->seg.p;
    return MRT_OK;
}
// ... and the bookkeeping after a successful pass
static void aov_done(mrt_ctx *c, const AovPass &ap)
{
    c->aov->inst_first = inst_first(*ap.pk);
    c->aov_ready = true;
}

// The AOV buffers of this context, computed on first use: *ms = HIP-event time of the pass (0 when they were there already)
static int aov_compute(mrt_ctx *c, bool &cached, double &ms)
{
    cached = c->aov_ready;
    ms = 0.0;
    if (c->aov_ready) return MRT_OK;
    AovPass ap;
    if (const int rc = aov_pass(c, ap)) return rc;
    Aov &a = *c->aov;
    HIP_TRY(hipEventRecord(a.ev[0].get(), c->stream.get()));
    HIP_TRY(launch_aov(ap.P, ap.pk->features, a.guide.p, a.albedo.p, a.ids.p, c->stream.get()));
    HIP_TRY(hipEventRecord(a.ev[1].get(), c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    { float t = 0.0f; HIP_TRY(hipEventElapsedTime(&t, a.ev[0].get(), a.ev[1].get())); ms = t; }
    aov_done(c, ap);
    return MRT_OK;
}

namespace {
// Filter options -> passes, the 1/sigma^2 formed in f32 (sigma = +inf: 0, the term is off), the mode and its firefly factor
struct DnOpts { u32 passes, mode; float sc, sn, sp, sv, firefly; };
}  // namespace

static int denoise_opts(const mrt_denoise_opts *o, const char *fn, DnOpts &r)
{
    mrt_denoise_opts d;
    memset(&d, 0, sizeof d);
    d.passes = MRT_DENOISE_PASSES;
    d.sigma_color = MRT_DENOISE_SIGMA_COLOR; d.sigma_normal = MRT_DENOISE_SIGMA_NORMAL; d.sigma_plane = MRT_DENOISE_SIGMA_PLANE;
    if (!o) o = &d;
    if (o->passes > kDnMaxPasses) return fail(MRT_ERR_ARG, "%s: passes %u > %u", fn, o->passes, kDnMaxPasses);
    const float sg[3] = {o->sigma_color, o->sigma_normal, o->sigma_plane};
    for (float s : sg) if (!(s > 0.0f)) return fail(MRT_ERR_ARG, "%s: sigma %g is not > 0", fn, (double)s);
    if (o->mode != MRT_DN_ATROUS && o->mode != MRT_DN_VARIANCE) return fail(MRT_ERR_ARG, "%s: unknown mode %u", fn, o->mode);
    if (!(o->sigma_var >= 0.0f)) return fail(MRT_ERR_ARG, "%s: sigma_var %g is not >= 0", fn, (double)o->sigma_var);
    if (!(o->firefly >= 0.0f)) return fail(MRT_ERR_ARG, "%s: firefly %g is not >= 0", fn, (double)o->firefly);
    if (o->mode == MRT_DN_ATROUS && (o->sigma_var != 0.0f || o->firefly != 0.0f))
        return fail(MRT_ERR_ARG, "%s: sigma_var and firefly belong to MRT_DN_VARIANCE and must be 0 in MRT_DN_ATROUS", fn);
    r.passes = o->passes; r.mode = o->mode;
    r.sc = 1.0f / (sg[0] * sg[0]);
    r.sn = 1.0f / (sg[1] * sg[1]);
    r.sp = 1.0f / (sg[2] * sg[2]);
    const float sv = o->sigma_var != 0.0f ? o->sigma_var : MRT_DN_SIGMA_VAR;
    r.sv = 1.0f / (sv * sv);
    r.firefly = o->firefly != 0.0f ? o->firefly : MRT_DN_FIREFLY;
    return MRT_OK;
}

// The filtered means of the accumulator into the context's output plane (*out, on the device); an observation like mrt_img.
// mrt_img_hdr (mrt_hdr.cpp) calls it too: mrt_ctx.h declares it.
int mrt::api::denoise_run(mrt_ctx *c, const mrt_denoise_opts *o, mrt_denoise_info *info, const char *fn, const float **out)
{
    DnOpts d;
    MeanSrc S;
    bool cached;
    double aov_ms;
    int rc;
    if ((rc = denoise_opts(o, fn, d)) || (rc = enter(c))) return rc;
    if (d.mode == MRT_DN_VARIANCE && !c->adaptive)
        return fail(MRT_ERR_STATE, "%s: MRT_DN_VARIANCE needs the half buffer of an adaptive render on this context since its last reset or "
                    "mrt_set_accum; for a uniform budget of n samples call mrt_execute_adaptive with threshold 0 and min_samples = max_samples = n", fn);
    const bool rays_aov = c->aov_ready && c->aov->from_rays;
    // the half buffer and the guides must belong to the same grid: the camera's frame, or the rays of mrt_radiance_adaptive
    if (d.mode == MRT_DN_VARIANCE && c->adaptive_rays && !rays_aov)
        return fail(MRT_ERR_STATE, "%s: MRT_DN_VARIANCE reads the adaptive half buffer, which belongs to the rays of mrt_radiance_adaptive, but the "
                    "AOVs are the camera's own; install those of the same rays with mrt_aov_rays first", fn);
    if (d.mode == MRT_DN_VARIANCE && !c->adaptive_rays && rays_aov)
        return fail(MRT_ERR_STATE, "%s: MRT_DN_VARIANCE reads the adaptive half buffer, which belongs to the camera's frame, but the AOVs "
                    "installed are those of caller-supplied rays; mrt_aov_rays(ctx, NULL, NULL, 0) returns to the camera's", fn);
    if ((rc = whole_frame(c, fn, "", S)) || (rc = aov_compute(c, cached, aov_ms))) return rc;
    Aov &a = *c->aov;
    const u32 nw = c->pk.nw, nh = c->pk.nh;
    const size_t np = (size_t)nw * nh;
    if (!a.dn.p) HIP_TRY(a.dn.alloc(np * 11u));
    float *e0 = a.dn.p, *e1 = e0 + 4u * np, *dst = e1 + 4u * np;
    const bool env = c->pk.P.off_env != 0u;
    HIP_TRY(hipEventRecord(a.ev[0].get(), c->stream.get()));
    if (d.mode == MRT_DN_VARIANCE && d.passes != 0u)
        HIP_TRY(launch_denoise_var(S, c->ad->half.p, a.guide.p, a.albedo.p, nh, d.passes, d.sv, d.sn, d.sp, d.firefly, e0, e1, dst, c->stream.get(), env));
    else
        HIP_TRY(launch_denoise(S, a.guide.p, a.albedo.p, nh, d.passes, d.sc, d.sn, d.sp, e0, e1, dst, c->stream.get(), env, a.wrap_x));
    HIP_TRY(hipEventRecord(a.ev[1].get(), c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, a.ev[0].get(), a.ev[1].get()));
    if (info) {
        memset(info, 0, sizeof *info);
        info->aov_ms = aov_ms; info->filter_ms = ms; info->passes = d.passes; info->aov_cached = cached ? 1u : 0u;
        info->reserved[0] = d.mode;
    }
    *out = dst;
    return MRT_OK;
}

extern "C" {

int mrt_aov(mrt_ctx *c, float *depth, float *normal, float *albedo, int32_t *renderer, int32_t *instance)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_aov: null context");
    bool cached;
    double ms;
    int rc;
    if ((rc = set_device(c)) || (rc = aov_compute(c, cached, ms))) return rc;
    const Aov &a = *c->aov;
    const size_t np = (size_t)c->pk.nw * c->pk.nh;
    if (depth || normal) {
        std::vector<float> g(np * 4u);
        HIP_TRY(hipMemcpy(g.data(), a.guide.p, np * 4u * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t p = 0; p < np; ++p) {
            if (depth) depth[p] = g[4 * p + 3];
            if (normal) for (int k = 0; k < 3; ++k) normal[3 * p + k] = g[4 * p + k];
        }
    }
    if (albedo) HIP_TRY(hipMemcpy(albedo, a.albedo.p, np * 3u * sizeof(float), hipMemcpyDeviceToHost));
    if (renderer || instance) {
        std::vector<i32> ids(np * 2u);
        HIP_TRY(hipMemcpy(ids.data(), a.ids.p, np * 2u * sizeof(i32), hipMemcpyDeviceToHost));
        for (size_t p = 0; p < np; ++p) {
            const i32 r = ids[2 * p];
            if (renderer) renderer[p] = r;
            if (instance) instance[p] = r < 0 ? -1 : ids[2 * p + 1] - (i32)a.inst_first[(u32)r];
        }
    }
    ok();
    return MRT_OK;
}

// The AOV pass on one caller-supplied ray per pixel; its planes stand where the camera's stood until (NULL, NULL, 0) drops them.
// Not an observation: no enter(), nothing of the accumulator, of what was booked or traced ahead, or of the statistics is touched.
int mrt_aov_rays(mrt_ctx *c, const float *orig, const float *dir, uint32_t flags)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_aov_rays: null context");
    if (!orig != !dir) return fail(MRT_ERR_ARG, "mrt_aov_rays: orig and dir are both given, or both NULL");
    if (flags & ~(uint32_t)(MRT_AOV_RAYS_DEVICE | MRT_AOV_WRAP_X)) return fail(MRT_ERR_ARG, "mrt_aov_rays: unknown flags 0x%x", flags);
    if (!orig && flags) return fail(MRT_ERR_ARG, "mrt_aov_rays: flags 0x%x without rays", flags);
    if (c->group) return fail(MRT_ERR_STATE, "mrt_aov_rays: multi-device context");
    int rc;
    if ((rc = set_device(c))) return rc;
    if (!orig) {                                  // back to the camera's own: the next use computes them
        c->aov_ready = false;
        if (c->aov) { c->aov->from_rays = false; c->aov->wrap_x = false; }
        ok();
        return MRT_OK;
    }
    AovPass ap;
    if ((rc = aov_pass(c, ap))) return rc;
    Aov &a = *c->aov;
    DeviceRays rays;
    HIP_TRY(rays.take(orig, dir, (size_t)c->pk.nw * c->pk.nh, (flags & MRT_AOV_RAYS_DEVICE) != 0u));
    // whatever fails from here on leaves no half-written planes behind as anybody's AOVs
    c->aov_ready = false;
    a.from_rays = false; a.wrap_x = false;
    HIP_TRY(launch_aov_rays(ap.P, ap.pk->features, rays.orig, rays.dir, a.guide.p, a.albedo.p, a.ids.p, c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    a.from_rays = true;
    a.wrap_x = (flags & MRT_AOV_WRAP_X) != 0u;
    aov_done(c, ap);
    ok();
    return MRT_OK;
}

int mrt_denoise(mrt_ctx *c, const mrt_denoise_opts *o, float *rgb, mrt_denoise_info *info)
{
    if (!c || !rgb) return fail(MRT_ERR_ARG, "mrt_denoise: null argument");
    const float *dst = nullptr;
    int rc = denoise_run(c, o, info, "mrt_denoise", &dst);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(rgb, dst, (size_t)c->pk.nw * c->pk.nh * 3u * sizeof(float), hipMemcpyDeviceToHost));
    ok();
    return MRT_OK;
}

// mrt_img on the filtered means: tonemap_channel(c', 1.0f, gamma, wexp), then the Lanczos3 path of mrt_img
int mrt_img_denoised(mrt_ctx *c, const mrt_denoise_opts *o, uint8_t *rgb8, mrt_denoise_info *info)
{
    if (!c || !rgb8) return fail(MRT_ERR_ARG, "mrt_img_denoised: null argument");
    const float *dst = nullptr;
    int rc;
    if ((rc = denoise_run(c, o, info, "mrt_img_denoised", &dst)) || (rc = img_prepare(c))) return rc;
    HIP_TRY(hipEventRecord(c->ev0.get(), c->stream.get()));
    HIP_TRY(launch_tonemap(mean_src(c, dst), c->img->ss.p, c->pk.nh, c->pk.gamma, tonemap_wexp(c), c->stream.get()));
    return img_finish(c, rgb8, true);
}

}  // extern "C"
