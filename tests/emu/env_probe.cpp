// TEST INFRASTRUCTURE: x86 build of the environment-texture code of csrc/mrt_trace.h -- env_uv alone, the packer
// with a mrt_env, the first-hit AOV pass, the a-trous filter and the path tracer's render_pixel -- for tests/test_env_host.py and
// tests/test_gpu_env.py.
// Built by the tests themselves through tests/emu/build.py: the flags of tests/emu/Makefile, with mrt_pack.cpp.
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "lane_host.h"

using namespace mrt;

static std::string g_err;

extern "C" {

const char *ev_error(void) { return g_err.c_str(); }

// env_uv and env_index on n directions d[n][3]: uv[n][2], idx[n] for a w x h texture
void ev_uv(uint32_t n, uint32_t mapping, float rot, uint32_t w, uint32_t h, const float *d, float *uv, uint32_t *idx)
{
    for (uint32_t i = 0; i < n; ++i) {
        const UV r = env_uv(mapping, rot, v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]));
        uv[2 * i] = r.x; uv[2 * i + 1] = r.y;
        idx[i] = env_index(r, w, h);
    }
}

// the math contract's functions the restatement takes from this build: op 0 atan2_(a, b), 1 acos_(a), 2 div_(a, b)
void ev_math(uint32_t op, uint32_t n, const float *a, const float *b, float *out)
{
    for (uint32_t i = 0; i < n; ++i) out[i] = op == 0u ? atan2_(a[i], b[i]) : (op == 1u ? acos_(a[i]) : div_(a[i], b[i]));
}

// hit_uv of a unit sphere at the origin for the hit points p[n][3], and norm(p)
void ev_sphere_uv(uint32_t n, const float *p, float *uv, float *normed)
{
    Params P;
    memset(&P, 0, sizeof P);
    Scn S;
    memset(&S, 0, sizeof S);
    S.P = &P;
    Obj o;
    memset(&o, 0, sizeof o);
    o.kind = KIND_SPHERE; o.pos = v3(0.0f, 0.0f, 0.0f); o.ident = true;
    for (uint32_t i = 0; i < n; ++i) {
        const V3 v = v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
        const UV r = hit_uv<F_ALL>(S, o, v, 0);
        uv[2 * i] = r.x; uv[2 * i + 1] = r.y;
        const V3 m = norm(v);
        normed[3 * i] = m.x; normed[3 * i + 1] = m.y; normed[3 * i + 2] = m.z;
    }
}

// the packed scene: info = features, blob_words, lds_words, lds_words_warm, lds_words_hot, off_env, sizeof(Params), walk_cap;
// params (sizeof(Params) bytes) and blob (at most cap words) may be NULL
int ev_pack(const mrt_render_desc *d, const mrt_desc_ext *ext, uint32_t *info /*[8]*/, void *params, uint32_t *blob, uint64_t cap)
{
    Packed pk;
    const int rc = pack_scene(d, pk, g_err, PackOpts(), ext);
    if (rc) return rc;
    const uint32_t v[8] = {pk.features, pk.P.blob_words, pk.P.lds_words, pk.P.lds_words_warm, pk.P.lds_words_hot, pk.P.off_env, (uint32_t)sizeof(Params), pk.P.walk_cap};
    memcpy(info, v, sizeof v);
    if (params) memcpy(params, &pk.P, sizeof(Params));
    if (blob) memcpy(blob, pk.blob.data(), sizeof(uint32_t) * (size_t)(cap < pk.P.blob_words ? cap : pk.P.blob_words));
    return 0;
}

// Params.sky_init of the packed scene
int ev_sky_init(const mrt_render_desc *d, const mrt_desc_ext *ext, float *out /*[3]*/)
{
    Packed pk;
    const int rc = pack_scene(d, pk, g_err, PackOpts(), ext);
    if (rc) return rc;
    memcpy(out, pk.P.sky_init, sizeof pk.P.sky_init);
    return 0;
}

// mrt_aov: guide[nh][nw][8] (normal, depth, world point, hit flag), albedo[nh][nw][3], renderer[nh][nw] and, where instance is not
// NULL, instance[nh][nw]: the index within the renderer's inst list (the flat index less the renderer's first, as mrt_aov maps it)
int ev_aov_inst(const mrt_render_desc *d, const mrt_desc_ext *ext, float *guide, float *albedo, int32_t *renderer, int32_t *instance)
{
    lane::Packing k;
    const int rc = lane::pack(d, ext, PackOpts(), lane::Level(), k, g_err);
    if (rc) return rc;
    return lane::aov_frame(k, lane::lane_inst(k.pk, 0u, false), guide, albedo, renderer, instance, g_err);
}

int ev_aov(const mrt_render_desc *d, const mrt_desc_ext *ext, float *guide, float *albedo, int32_t *renderer)
{
    return ev_aov_inst(d, ext, guide, albedo, renderer, nullptr);
}

// mrt_denoise: the filtered means out[nh][nw][3] of the sums A[nh][nw][3] at per-pixel counts[nh][nw]; env: the context has an
// environment texture (miss pixels demodulated by their albedo too)
void ev_filter(const float *A, const uint32_t *counts, const float *guide, const float *albedo, uint32_t nw, uint32_t nh, uint32_t passes,
               float sc, float sn, float sp, uint32_t env, float *out)
{
    lane::atrous_host(A, counts, guide, albedo, nw, nh, passes, sc, sn, sp, env != 0u, out);
}

// the path tracer's per-lane body over the whole frame: accum[nh][nw][3]; warm != 0: the F_COLD lane code
int ev_render(const mrt_render_desc *d, const mrt_desc_ext *ext, uint64_t seed, uint32_t sample_base, uint32_t n_samples, uint32_t threads,
              uint32_t warm, float *accum)
{
    lane::Packing k;
    lane::Level lv;
    if (warm) lv.flags = F_COLD;
    const int rc = lane::pack(d, ext, PackOpts(), lv, k, g_err);
    if (rc) return rc;
    return lane::render_frame(k, lane::lane_inst(k.pk, lv.flags, false), seed, sample_base, n_samples, 0, k.pk.nh, threads, accum, nullptr, g_err);
}

}
