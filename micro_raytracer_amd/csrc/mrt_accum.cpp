// mrt_accum.cpp — the entry points that observe or replace the accumulator (mrt_accum*, mrt_bind_accum, mrt_set_accum*,
// mrt_reset, mrt_dims) and the image path on it: tone map, Lanczos3, mrt_img / mrt_img_ss.
// The functions defined here as mrt::api::name are the ones other units call: mrt_ctx.h declares them and says what they do.
#include <string.h>

#include <utility>
#include <vector>

#include "mrt_ctx.h"

using namespace mrt;
using namespace mrt::api;

// A copy or a fill of device memory that later launches of this context read: on the context's stream, and waited for.
// hipMemcpy between two device buffers and hipMemset return before the device has done the work, and they run on the null
// stream, which the context's non-blocking stream is not ordered against: the next launch (the fold of a look-ahead plane is the
// quickest) would read the accumulator while the copy still writes it, and the copy would then overwrite that sample.
static int copy_on_stream(mrt_ctx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    return MRT_OK;
}
static int zero_on_stream(mrt_ctx *c, void *dst, size_t bytes)
{
    HIP_TRY(hipMemsetAsync(dst, 0, bytes, c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    return MRT_OK;
}

// mrt_set_accum / mrt_set_accum_device on a single-device context: the whole frame into the accumulator, or, on a sharded
// context, next to its own rows (only mrt_img and mrt_accum read it there)
static int set_frame(mrt_ctx *c, const void *rgb, hipMemcpyKind kind, uint32_t count)
{
    const size_t floats = (size_t)c->pk.nw * c->pk.nh * 3;
    int rc;
    if (c->shard_count == 1) {
        if ((rc = copy_on_stream(c, c->d_accum, rgb, floats * sizeof(float), kind))) return rc;
        c->count = count;
    } else {
        if (!c->full.p) HIP_TRY(c->full.alloc(floats));
        if ((rc = copy_on_stream(c, c->full.p, rgb, floats * sizeof(float), kind))) return rc;
        c->full_count = count;
    }
    ok();
    return MRT_OK;
}


// ---- the image path --------------------------------------------------------------------------------------------------------------
int mrt::api::img_prepare(mrt_ctx *c)
{
    if (c->img) return MRT_OK;
    const u32 nw = c->pk.nw, nh = c->pk.nh, rw = c->pk.res_w, rh = c->pk.res_h;
    const bool resize = rw != nw || rh != nh;
    if (resize && (rw == 0 || rh == 0)) return fail(MRT_ERR_SCENE, "mrt_img: zero output resolution");
    std::unique_ptr<Image> im(new Image());
    const int rc = [&]() -> int {
        HIP_TRY(im->ss.alloc((size_t)nw * nh * 3));
        if (!resize) return MRT_OK;
        ResampleTaps v, h;
        lanczos3_taps(nh, rh, v);
        lanczos3_taps(nw, rw, h);
        HIP_TRY(im->lanczos3.v.upload(v, rh));
        HIP_TRY(im->lanczos3.h.upload(h, rw));
        HIP_TRY(im->tmp.alloc((size_t)nw * rh * 3));
        HIP_TRY(im->out.alloc((size_t)rw * rh * 3));
        return MRT_OK;
    }();
    if (rc) { im.reset(); (void)hipGetLastError(); return rc; }     // (what failed is not left pending for the next launch)
    c->img = std::move(im);
    return MRT_OK;
}

static int img_tonemap(mrt_ctx *c, const char *fn)
{
    MeanSrc S;
    if (const int rc = whole_frame(c, fn, " (the reference would panic on an empty map, src/sampler.rs:85)", S)) return rc;
    HIP_TRY(hipEventRecord(c->ev0.get(), c->stream.get()));
    HIP_TRY(launch_tonemap(S, c->img->ss.p, c->pk.nh, c->pk.gamma, tonemap_wexp(c), c->stream.get()));
    return MRT_OK;
}

int mrt::api::img_finish(mrt_ctx *c, uint8_t *rgb8, bool resize)
{
    const u32 nw = c->pk.nw, nh = c->pk.nh, rw = c->pk.res_w, rh = c->pk.res_h;
    const Image &im = *c->img;
    const unsigned char *src = im.ss.p;
    size_t bytes = (size_t)nw * nh * 3;
    if (resize && (rw != nw || rh != nh)) {
        HIP_TRY(launch_lanczos_v(im.ss.p, im.tmp.p, nw, rh, im.lanczos3.v.dev(), c->stream.get()));
        HIP_TRY(launch_lanczos_h(im.tmp.p, im.out.p, nw, rw, rh, im.lanczos3.h.dev(), c->stream.get()));
        src = im.out.p;
        bytes = (size_t)rw * rh * 3;
    }
    HIP_TRY(hipEventRecord(c->ev1.get(), c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    { float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, c->ev0.get(), c->ev1.get())); c->stats.img_ms = ms; }
    HIP_TRY(hipMemcpy(rgb8, src, bytes, hipMemcpyDeviceToHost));
    ok();
    return MRT_OK;
}

extern "C" {

int mrt_dims(const mrt_ctx *c, uint32_t *nw, uint32_t *nh, uint32_t *local_rows)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_dims: null context");
    if (nw) *nw = c->pk.nw;
    if (nh) *nh = c->pk.nh;
    if (local_rows) *local_rows = c->local_rows;
    ok();
    return MRT_OK;
}

int mrt_accum_local(mrt_ctx *c, float *rgb, uint32_t *rows)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_accum_local: null context");
    if (const int rc = enter(c)) return rc;
    if (rows) memcpy(rows, c->row_of.data(), sizeof(u32) * c->local_rows);
    const float *src = c->group ? c->full.p : c->d_accum;         // a multi-device context owns every row
    if (rgb && c->local_rows) HIP_TRY(hipMemcpy(rgb, src, (size_t)c->local_rows * c->pk.nw * 3 * sizeof(float), hipMemcpyDeviceToHost));
    ok();
    return MRT_OK;
}

int mrt_accum(mrt_ctx *c, float *rgb, uint32_t *count)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_accum: null context");
    if (const int rc = enter(c)) return rc;
    const Frame f = frame_of(c);
    const size_t row_bytes = (size_t)c->pk.nw * 3 * sizeof(float);
    if (rgb && f.rgb) HIP_TRY(hipMemcpy(rgb, f.rgb, row_bytes * c->pk.nh, hipMemcpyDeviceToHost));
    else if (rgb) {                           // a shard's own rows, in their places
        std::vector<float> tmp((size_t)c->local_rows * c->pk.nw * 3);
        if (c->local_rows) HIP_TRY(hipMemcpy(tmp.data(), c->d_accum, row_bytes * c->local_rows, hipMemcpyDeviceToHost));
        for (u32 r = 0; r < c->local_rows; ++r) memcpy((char *)rgb + row_bytes * c->row_of[r], (char *)tmp.data() + row_bytes * r, row_bytes);
    }
    if (count) *count = f.count;
    ok();
    return MRT_OK;
}

int mrt_accum_device_ptr(mrt_ctx *c, void **dev_ptr, size_t *bytes)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_accum_device_ptr: null context");
    if (const int rc = enter(c)) return rc;
    c->handed_out = true;                     // from now on the caller may read the accumulator behind the library's back (sticky)
    if (dev_ptr) *dev_ptr = c->group ? c->full.p : c->d_accum;
    if (bytes) *bytes = plane_floats(c) * sizeof(float);
    ok();
    return MRT_OK;
}

int mrt_padded_rows(const mrt_ctx *c, uint32_t *rows)
{
    if (!c || !rows) return fail(MRT_ERR_ARG, "mrt_padded_rows: null argument");
    *rows = c->padded_rows;
    ok();
    return MRT_OK;
}

int mrt_bind_accum(mrt_ctx *c, void *dev_ptr, size_t bytes)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_bind_accum: null context");
    if (c->group) return fail(MRT_ERR_STATE, "mrt_bind_accum: not available on a multi-device context");
    if (const int rc = enter(c)) return rc;
    const size_t need = plane_floats(c) * sizeof(float);
    float *dst = dev_ptr ? (float *)dev_ptr : c->accum_own.p;
    if (dev_ptr && bytes < need) return fail(MRT_ERR_ARG, "mrt_bind_accum: buffer of %zu bytes, need %zu", bytes, need);     // nothing changed
    if (dst != c->d_accum) {
        if (const int rc = copy_on_stream(c, dst, c->d_accum, need, hipMemcpyDeviceToDevice)) return rc;
        c->d_accum = dst;
        c->P.accum = dst;
    }
    c->bound = dev_ptr != nullptr;            // only a bind that succeeded: the caller reads this memory whenever it likes, so every execute runs at once
    ok();
    return MRT_OK;
}

int mrt_set_accum_device(mrt_ctx *c, const void *dev_rgb, uint32_t count)
{
    if (!c || !dev_rgb) return fail(MRT_ERR_ARG, "mrt_set_accum_device: null argument");
    if (const int rc = enter(c)) return rc;
    la_drop(c); c->adaptive = false;              // the sample count changes under what was traced ahead
    if (c->group) return fail(MRT_ERR_STATE, "mrt_set_accum_device: use mrt_set_accum on a multi-device context");
    return set_frame(c, dev_rgb, hipMemcpyDeviceToDevice, count);
}

int mrt_set_accum(mrt_ctx *c, const float *rgb, uint32_t count)
{
    if (!c || !rgb) return fail(MRT_ERR_ARG, "mrt_set_accum: null argument");
    if (const int rc = enter(c)) return rc;
    la_drop(c); c->adaptive = false;
    if (!c->group) return set_frame(c, rgb, hipMemcpyHostToDevice, count);
    const size_t row_bytes = (size_t)c->pk.nw * 3 * sizeof(float);
    HIP_TRY(hipMemcpy(c->full.p, rgb, row_bytes * c->pk.nh, hipMemcpyHostToDevice));
    for (auto &s : c->group->subs) {
        HIP_TRY(hipSetDevice(s->device));
        for (u32 i = 0; i < s->local_rows; ++i)
            HIP_TRY(hipMemcpy((char *)s->d_accum + row_bytes * i, (const char *)rgb + row_bytes * s->row_of[i], row_bytes, hipMemcpyHostToDevice));
        s->count = count;
    }
    c->count = count; c->full_count = count;
    ok();
    return MRT_OK;
}

int mrt_reset(mrt_ctx *c)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_reset: null context");
    c->pending = 0;                           // booked samples of a deferred context are dropped with everything else
    int rc = set_device(c);
    if (rc) return rc;
    la_drop(c); c->adaptive = false;
    if (c->group) {
        for (auto &s : c->group->subs) if ((rc = mrt_reset(s.get()))) return rc;
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipMemset(c->full.p, 0, (size_t)c->pk.nh * c->pk.nw * 3 * sizeof(float)));
    } else {
        if ((rc = zero_on_stream(c, c->d_accum, plane_floats(c) * sizeof(float)))) return rc;
        c->full.reset();
    }
    c->count = 0; c->full_count = 0;
    ok();
    return MRT_OK;
}

int mrt_img_ss(mrt_ctx *c, uint8_t *rgb8)
{
    if (!c || !rgb8) return fail(MRT_ERR_ARG, "mrt_img_ss: null argument");
    int rc;
    if ((rc = enter(c)) || (rc = img_prepare(c)) || (rc = img_tonemap(c, "mrt_img_ss"))) return rc;
    return img_finish(c, rgb8, false);
}

int mrt_img(mrt_ctx *c, uint8_t *rgb8)
{
    if (!c || !rgb8) return fail(MRT_ERR_ARG, "mrt_img: null argument");
    int rc;
    if ((rc = enter(c)) || (rc = img_prepare(c)) || (rc = img_tonemap(c, "mrt_img"))) return rc;
    return img_finish(c, rgb8, true);
}

}  // extern "C"
