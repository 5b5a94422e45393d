// TEST INFRASTRUCTURE: x86 build of the environment-texture code of csrc/mrt_trace.h -- env_uv alone, the packer
// with a mrt_env, the first-hit AOV pass, the a-trous filter and the path tracer's render_pixel -- for tests/test_env_host.py and
// tests/test_gpu_env.py.
// Built by the tests themselves: g++ -O2 [-mfma] -std=c++17 -ffp-contract=off -shared -fPIC (no fast-math) with mrt_pack.cpp.
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../micro_raytracer_amd/csrc/mrt_denoise.h"
#include "../../micro_raytracer_amd/csrc/mrt_pack.h"

using namespace mrt;

static std::string g_err;

namespace {

struct Packing {
    Packed pk;
    Params P;
    Scn S;
};

int pack(const mrt_render_desc *d, const mrt_desc_ext *ext, Packing &k)
{
    const int rc = pack_scene(d, k.pk, g_err, PackOpts(), ext);
    if (rc) return rc;
    k.P = k.pk.P;
    k.P.local_rows = k.pk.nh; k.P.shard_index = 0; k.P.shard_count = 1; k.P.shard_rows = 8; k.P.k_split = 1;
    k.S.F = reinterpret_cast<const float *>(k.pk.blob.data());
    k.S.U = k.S.F; k.S.G = k.S.F; k.S.P = &k.P; k.S.wk = nullptr; k.S.wk_stride = 1;
    return 0;
}

// the instantiation pt_instantiation picks: the full feature set with F_VATTR | F_ENV for a scene with an environment
template <u32 X>
void render_one(const Packing &k, RegStash &st, u32 x, u32 y, const LaneJob &job, u32 &sg)
{
    const u32 f = k.pk.features;
    constexpr u32 E = F_ALL | F_VATTR | F_ENV | X, V = F_ALL | F_VATTR | X, A = F_ALL | X;
    if (f & F_ENV) { if (f & F_BVH) render_pixel<E | F_BVH>(k.S, st, x, y, job, sg); else render_pixel<E>(k.S, st, x, y, job, sg); }
    else if (f & F_VATTR) { if (f & F_BVH) render_pixel<V | F_BVH>(k.S, st, x, y, job, sg); else render_pixel<V>(k.S, st, x, y, job, sg); }
    else { if (f & F_BVH) render_pixel<A | F_BVH>(k.S, st, x, y, job, sg); else render_pixel<A>(k.S, st, x, y, job, sg); }
}

AovPixel aov_one(const Packing &k, u32 x, u32 y)
{
    const u32 f = k.pk.features;
    constexpr u32 E = F_ALL | F_VATTR | F_ENV, V = F_ALL | F_VATTR, A = F_ALL;
    if (f & F_ENV) return (f & F_BVH) ? aov_pixel<E | F_BVH>(k.S, x, y) : aov_pixel<E>(k.S, x, y);
    if (f & F_VATTR) return (f & F_BVH) ? aov_pixel<V | F_BVH>(k.S, x, y) : aov_pixel<V>(k.S, x, y);
    return (f & F_BVH) ? aov_pixel<A | F_BVH>(k.S, x, y) : aov_pixel<A>(k.S, x, y);
}

}  // namespace

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
    Packing k;
    const int rc = pack(d, ext, k);
    if (rc) return rc;
    unsigned long long seg[8] = {0};
    k.P.segments = seg;
    std::vector<u32> first(k.P.n_rend, 0u);
    for (u32 i = k.P.n_inst; i-- > 0;) first[k.pk.blob[k.P.off_instx + i * INSTX_WORDS + INSTX_REND]] = i;
    for (u32 y = 0; y < k.pk.nh; ++y)
        for (u32 x = 0; x < k.pk.nw; ++x) {
            const AovPixel a = aov_one(k, x, y);
            const size_t p = (size_t)y * k.pk.nw + x;
            memcpy(guide + 8 * p, &a.g, sizeof(DnGuide));
            albedo[3 * p] = a.albedo.x; albedo[3 * p + 1] = a.albedo.y; albedo[3 * p + 2] = a.albedo.z;
            renderer[p] = a.rend;
            if (instance) instance[p] = a.rend < 0 ? -1 : a.inst - (i32)first[(u32)a.rend];
        }
    return 0;
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
    const size_t np = (size_t)nw * nh;
    const DnGuide *g = reinterpret_cast<const DnGuide *>(guide);
    std::vector<float> e(np * 3), t(np * 3);
    for (size_t p = 0; p < np; ++p) {
        const float rc = 1.0f / (float)counts[p];
        for (int k = 0; k < 3; ++k) {
            const float c = A[3 * p + k] * rc;
            if (passes == 0u) out[3 * p + k] = c;
            else e[3 * p + k] = c / dn_demod(albedo[3 * p + k], g[p].hit, env != 0u);
        }
    }
    if (passes == 0u) return;
    for (u32 i = 0; i < passes; ++i) {
        dn_pass_host(e.data(), g, nw, nh, 1u << i, dn_pass_sc(sc, i), sn, sp, t.data());
        e.swap(t);
    }
    for (size_t p = 0; p < np; ++p)
        for (int k = 0; k < 3; ++k) out[3 * p + k] = e[3 * p + k] * dn_demod(albedo[3 * p + k], g[p].hit, env != 0u);
}

// the path tracer's per-lane body over the whole frame: accum[nh][nw][3]; warm != 0: the F_COLD lane code
int ev_render(const mrt_render_desc *d, const mrt_desc_ext *ext, uint64_t seed, uint32_t sample_base, uint32_t n_samples, uint32_t threads,
              uint32_t warm, float *accum)
{
    Packing k;
    const int rc = pack(d, ext, k);
    if (rc) return rc;
    k.P.seed_lo = (u32)seed; k.P.seed_hi = (u32)(seed >> 32);
    k.P.n_samples = n_samples; k.P.sample_base = sample_base; k.P.accum = accum;
    std::atomic<uint32_t> next(0);
    if (threads == 0) threads = 1;
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < threads; ++t) pool.emplace_back([&]() {
        for (;;) {
            const uint32_t y = next.fetch_add(1);
            if (y >= k.pk.nh) break;
            for (uint32_t x = 0; x < k.pk.nw; ++x) {
                u32 sg = 0;
                RegStash st; LaneJob job; job.k = 0; job.word = (y * k.pk.nw + x) * 3u;
                if (warm) render_one<F_COLD>(k, st, x, y, job, sg); else render_one<0u>(k, st, x, y, job, sg);
            }
        }
    });
    for (auto &th : pool) th.join();
    return 0;
}

}
