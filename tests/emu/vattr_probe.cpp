// TEST INFRASTRUCTURE: x86 build of the per-corner attribute code of csrc/mrt_trace.h -- the interpolation
// functions alone, the first-hit AOV pass and the path tracer's render_pixel on scenes packed with a mrt_desc_ext -- for
// tests/test_vattr_host.py and tests/test_gpu_vattr.py.
// Built by the tests themselves through tests/emu/build.py: the flags of tests/emu/Makefile, with mrt_pack.cpp.
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "lane_host.h"

using namespace mrt;

static std::string g_err;

extern "C" {

const char *va_error(void) { return g_err.c_str(); }

// tri_bary / vattr_normal / vattr_uv on n independent inputs: p, v0, e1, e2 [n][3], vn [n][9], uv [n][6] ->
// bary [n][3] (b1, b2, ok), normal [n][3] (object space, not normalised), tex [n][2]
void va_interp(uint32_t n, const float *p, const float *v0, const float *e1, const float *e2, const float *vn, const float *uv,
               float *bary, float *normal, float *tex)
{
    for (uint32_t i = 0; i < n; ++i) {
        const V3 P_ = v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]), A = v3(v0[3 * i], v0[3 * i + 1], v0[3 * i + 2]);
        const V3 E1 = v3(e1[3 * i], e1[3 * i + 1], e1[3 * i + 2]), E2 = v3(e2[3 * i], e2[3 * i + 1], e2[3 * i + 2]);
        const Bary b = tri_bary(P_, A, E1, E2);
        bary[3 * i] = b.b1; bary[3 * i + 1] = b.b2; bary[3 * i + 2] = b.ok ? 1.0f : 0.0f;
        const V3 nn = vattr_normal(P_, A, E1, E2, vn + 9 * i);
        normal[3 * i] = nn.x; normal[3 * i + 1] = nn.y; normal[3 * i + 2] = nn.z;
        const UV t = vattr_uv(P_, A, E1, E2, uv + 6 * i);
        tex[2 * i] = t.x; tex[2 * i + 1] = t.y;
    }
}

// bary_mix alone: out[i] = a0 + (b1 (a1 - a0) + b2 (a2 - a0))
void va_mix(uint32_t n, const float *b1, const float *b2, const float *a0, const float *a1, const float *a2, float *out)
{
    for (uint32_t i = 0; i < n; ++i) { Bary b; b.b1 = b1[i]; b.b2 = b2[i]; b.ok = true; out[i] = bary_mix(b, a0[i], a1[i], a2[i]); }
}

// the packed blob and what the layout tests need: info = features, off_vattr, n_vattr_rows, blob_words, lds_words, lds_words_warm,
// lds_words_hot, off_rend.  blob may be NULL; at most cap words are copied
int va_pack(const mrt_render_desc *d, const mrt_desc_ext *ext, uint32_t *blob, uint32_t cap, uint32_t *info /*[8]*/)
{
    Packed pk;
    const int rc = pack_scene(d, pk, g_err, PackOpts(), ext);
    if (rc) return rc;
    const uint32_t v[8] = {pk.features, pk.off_vattr, pk.n_vattr_rows, pk.P.blob_words, pk.P.lds_words, pk.P.lds_words_warm, pk.P.lds_words_hot, pk.P.off_rend};
    memcpy(info, v, sizeof v);
    if (blob) memcpy(blob, pk.blob.data(), sizeof(uint32_t) * (cap < pk.P.blob_words ? cap : pk.P.blob_words));
    return 0;
}

// mrt_aov of a scene with attributes: guide[nh][nw][8] (normal, depth, world point, hit flag), albedo[nh][nw][3], renderer[nh][nw]
// deep_nodes: 0 = binary triangle BVHs (F_ALL), 0xffffffff = the warm lane code on them (F_COLD), n = 4-wide tables of which the
// first n nodes count as staged (F_COLD | F_DEEP), as tests/emu/emu.cpp emu_render_deep
int va_aov(const mrt_render_desc *d, const mrt_desc_ext *ext, uint32_t deep_nodes, float *guide, float *albedo, int32_t *renderer)
{
    lane::Packing k;
    const lane::Level lv = lane::level_of(deep_nodes);
    const int rc = lane::pack(d, ext, PackOpts(), lv, k, g_err);
    if (rc) return rc;
    return lane::aov_frame(k, lane::lane_inst(k.pk, lv.flags, false), guide, albedo, renderer, nullptr, g_err);
}

// the path tracer's per-lane body over the whole frame (tests/emu/emu.cpp emu_render_deep with attributes): accum[nh][nw][3]
int va_render(const mrt_render_desc *d, const mrt_desc_ext *ext, uint64_t seed, uint32_t sample_base, uint32_t n_samples, uint32_t threads,
              uint32_t deep_nodes, float *accum)
{
    lane::Packing k;
    const lane::Level lv = lane::level_of(deep_nodes);
    const int rc = lane::pack(d, ext, PackOpts(), lv, k, g_err);
    if (rc) return rc;
    return lane::render_frame(k, lane::lane_inst(k.pk, lv.flags, false), seed, sample_base, n_samples, 0, k.pk.nh, threads, accum, nullptr, g_err);
}

}
