// mrt_hdr.cpp — the linear float image and its writers: mrt_img_hdr resamples the mean radiance, or the denoiser's
// filtered means, in f32 to the output resolution on the device -- no tone map, no quantisation --; mrt_save_image_f32 writes
// such an image as a Radiance .hdr or a .pfm (host only).
#include <errno.h>
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "mrt_ctx.h"

using namespace mrt;
using namespace mrt::api;

// The Hdr state of this context, created whole by the first call: a failure half-way leaves the context as it was
static int hdr_prepare(mrt_ctx *c)
{
    if (c->hdr) return MRT_OK;
    const u32 nw = c->pk.nw, nh = c->pk.nh, rw = c->pk.res_w, rh = c->pk.res_h;
    std::unique_ptr<Hdr> hd(new Hdr());
    const int rc = [&]() -> int {
        for (Event &e : hd->ev) HIP_TRY(create(e));
        HIP_TRY(hd->out.alloc((size_t)rw * rh * 3));
        if (rw == nw && rh == nh) return MRT_OK;
        ResampleTaps v, h;
        box_taps(nh, rh, v);
        box_taps(nw, rw, h);
        HIP_TRY(hd->box.v.upload(v, rh));
        HIP_TRY(hd->box.h.upload(h, rw));
        HIP_TRY(hd->tmp.alloc((size_t)nw * rh * 3));
        return MRT_OK;
    }();
    if (rc) { hd.reset(); (void)hipGetLastError(); return rc; }
    c->hdr = std::move(hd);
    return MRT_OK;
}

namespace {

// ---- the writers ---------------------------------------------------------------------------------------------------------------
int failf(int code, const std::string &msg) { return fail(code, "%s", msg.c_str()); }

// One RGBE pixel, rounding to nearest (read_hdr decodes b * 2^(e - 136), so the round trip errs by at most 2^(E-9) <= v / 256 per
// component below the saturation at exponent byte 255)
void rgbe(const float *rgb, uint8_t *out)
{
    double c[3], v = 0.0;
    for (int k = 0; k < 3; ++k) {
        const float x = rgb[k];
        c[k] = !(x >= 0.0f) ? 0.0 : (x > FLT_MAX ? (double)FLT_MAX : (double)x);     // NaN and negatives: 0; +inf: FLT_MAX
        if (c[k] > v) v = c[k];
    }
    out[0] = out[1] = out[2] = out[3] = 0;
    if (v < ldexp(1.0, -127)) return;
    int E;
    (void)frexp(v, &E);                                        // v = f * 2^E, f in [0.5, 1)
    double b[3];
    auto mantissas = [&]() { double top = 0.0; for (int k = 0; k < 3; ++k) { b[k] = floor(ldexp(c[k], 8 - E) + 0.5); if (b[k] > top) top = b[k]; } return top; };
    if (mantissas() >= 256.0) { E += 1; (void)mantissas(); }
    if (E + 128 > 255) {                                       // saturated: the largest exponent byte, mantissas capped
        E = 127;
        (void)mantissas();
        for (int k = 0; k < 3; ++k) if (b[k] > 255.0) b[k] = 255.0;
    }
    for (int k = 0; k < 3; ++k) out[k] = (uint8_t)b[k];
    out[3] = (uint8_t)(E + 128);
}

// one channel of a new-style run-length scanline: runs of 4..127 equal bytes as (128 + n, byte), the rest as literals of 1..128
void rle_channel(const uint8_t *p, uint32_t w, std::vector<uint8_t> &out)
{
    auto run_at = [&](uint32_t x, uint32_t most) { uint32_t r = 1; while (x + r < w && r < most && p[x + r] == p[x]) ++r; return r; };
    for (uint32_t x = 0; x < w;) {
        const uint32_t r = run_at(x, 127u);
        if (r >= 4u) { out.push_back((uint8_t)(128u + r)); out.push_back(p[x]); x += r; continue; }
        const uint32_t start = x;
        while (x < w && x - start < 128u && run_at(x, 4u) < 4u) ++x;
        out.push_back((uint8_t)(x - start));
        out.insert(out.end(), p + start, p + x);
    }
}

}  // namespace

extern "C" {

int mrt_img_hdr(mrt_ctx *c, const mrt_hdr_opts *o, float *rgb, mrt_hdr_info *info)
{
    if (!c || !rgb) return fail(MRT_ERR_ARG, "mrt_img_hdr: null argument");
    mrt_hdr_opts d;
    memset(&d, 0, sizeof d);
    if (!o) o = &d;
    if (o->filter != MRT_RESIZE_LANCZOS3 && o->filter != MRT_RESIZE_BOX) return fail(MRT_ERR_ARG, "mrt_img_hdr: unknown filter %u", o->filter);
    if (o->reserved0) return fail(MRT_ERR_ARG, "mrt_img_hdr: reserved0 must be 0");
    for (int k = 0; k < 4; ++k) if (o->reserved[k]) return fail(MRT_ERR_ARG, "mrt_img_hdr: reserved[%d] must be 0", k);
    mrt_hdr_info hi;
    memset(&hi, 0, sizeof hi);
    // the source: the filtered means as they are, or the frame's sums and their 1/count
    MeanSrc S;
    int rc;
    if (o->denoise) {
        const float *dn = nullptr;
        if ((rc = denoise_run(c, o->denoise, &hi.dn, "mrt_img_hdr", &dn))) return rc;
        S = mean_src(c, dn);
    } else {
        if ((rc = enter(c)) || (rc = whole_frame(c, "mrt_img_hdr", "", S))) return rc;
    }
    if ((rc = img_prepare(c)) || (rc = hdr_prepare(c))) return rc;
    const u32 nw = c->pk.nw, nh = c->pk.nh, rw = c->pk.res_w, rh = c->pk.res_h;
    Hdr &hd = *c->hdr;
    hipStream_t st = c->stream.get();
    if (c->event_timing) HIP_TRY(hipEventRecord(hd.ev[0].get(), st));
    if (rw == nw && rh == nh) {
        HIP_TRY(launch_hdr_copy(S, hd.out.p, nh, st));
    } else {                                      // Lanczos3: the taps of mrt_img
        const Resampler &r = o->filter == MRT_RESIZE_BOX ? hd.box : c->img->lanczos3;
        HIP_TRY(launch_hdr_v(S, hd.tmp.p, rh, r.v.dev(), st));
        HIP_TRY(launch_hdr_h(hd.tmp.p, hd.out.p, nw, rw, rh, r.h.dev(), st));
    }
    if (c->event_timing) HIP_TRY(hipEventRecord(hd.ev[1].get(), st));
    HIP_TRY(hipStreamSynchronize(st));
    if (c->event_timing) { float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, hd.ev[0].get(), hd.ev[1].get())); hi.resize_ms = ms; }
    HIP_TRY(hipMemcpy(rgb, hd.out.p, (size_t)rw * rh * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (info) *info = hi;
    ok();
    return MRT_OK;
}

int mrt_save_image_f32(const char *path, const float *rgb, uint32_t w, uint32_t h)
{
    if (!path || !rgb || !w || !h) return failf(MRT_ERR_ARG, "mrt_save_image_f32: null path / pixels or empty image");
    const char *dot = strrchr(path, '.');
    const std::string ext = dot ? dot + 1 : "";
    std::vector<uint8_t> out;
    char hdr[96];
    if (ext == "pfm" || ext == "PFM") {
        const int n = snprintf(hdr, sizeof hdr, "PF\n%u %u\n-1.0\n", w, h);
        out.insert(out.end(), hdr, hdr + n);
        const size_t row = (size_t)w * 3 * sizeof(float);
        for (uint32_t y = h; y-- > 0;) {                       // rows bottom to top; the host is little-endian, as the scale says
            const uint8_t *p = (const uint8_t *)rgb + row * y;
            out.insert(out.end(), p, p + row);
        }
    } else if (ext == "hdr" || ext == "HDR") {
        const int n = snprintf(hdr, sizeof hdr, "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %u +X %u\n", h, w);
        out.insert(out.end(), hdr, hdr + n);
        const bool rle = w >= 8u && w <= 32767u;
        std::vector<uint8_t> px((size_t)w * 4), ch(w);
        for (uint32_t y = 0; y < h; ++y) {
            for (uint32_t x = 0; x < w; ++x) rgbe(rgb + ((size_t)y * w + x) * 3, px.data() + (size_t)x * 4);
            if (!rle) { out.insert(out.end(), px.begin(), px.end()); continue; }
            out.push_back(2); out.push_back(2); out.push_back((uint8_t)(w >> 8)); out.push_back((uint8_t)(w & 255u));
            for (int k = 0; k < 4; ++k) {
                for (uint32_t x = 0; x < w; ++x) ch[x] = px[(size_t)x * 4 + k];
                rle_channel(ch.data(), w, out);
            }
        }
    } else {
        return failf(MRT_ERR_ARG, std::string("mrt_save_image_f32: unsupported extension in '") + path + "' (.hdr and .pfm are written)");
    }
    FILE *f = fopen(path, "wb");
    if (!f) return failf(MRT_ERR_STATE, std::string("mrt_save_image_f32: cannot open '") + path + "': " + strerror(errno));
    const size_t wr = fwrite(out.data(), 1, out.size(), f);
    const int werr = errno;
    if (fclose(f) != 0 || wr != out.size()) return failf(MRT_ERR_STATE, std::string("mrt_save_image_f32: short write to '") + path + "': " + strerror(werr ? werr : errno));
    ok();
    return MRT_OK;
}

}  // extern "C"
