// TEST INFRASTRUCTURE: x86 build of the per-corner attribute code of csrc/mrt_trace.h -- the interpolation
// functions alone, the first-hit AOV pass and the path tracer's render_pixel on scenes packed with a mrt_desc_ext -- for
// tests/test_vattr_host.py and tests/test_gpu_vattr.py.
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

// deep: 0 = binary triangle BVHs (F_ALL), 0xffffffff = the warm lane code on them (F_COLD), n = 4-wide tables of which the
// first n nodes count as staged (F_COLD | F_DEEP), as tests/emu/emu.cpp emu_render_deep
struct Packing {
    Packed pk;
    Params P;
    Scn S;
    bool warm = false, deep = false;
};

int pack(const mrt_render_desc *d, const mrt_desc_ext *ext, uint32_t deep_nodes, Packing &k)
{
    k.warm = deep_nodes == 0xffffffffu;
    k.deep = deep_nodes != 0u && !k.warm;
    PackOpts po;
    po.tbvh_wide = k.deep;
    const int rc = pack_scene(d, k.pk, g_err, po, ext);
    if (rc) return rc;
    if (k.deep && !k.pk.tbvh_wide) { g_err = "no triangle BVH to widen"; return -100; }
    k.P = k.pk.P;
    if (k.deep) { k.P.n_tbvh_hot = deep_nodes; k.P.walk_cap = kWalkCapDefault; }
    k.P.local_rows = k.pk.nh; k.P.shard_index = 0; k.P.shard_count = 1; k.P.shard_rows = 8; k.P.k_split = 1;
    k.S.F = reinterpret_cast<const float *>(k.pk.blob.data());
    k.S.U = k.S.F; k.S.G = k.S.F; k.S.P = &k.P; k.S.wk = nullptr; k.S.wk_stride = 1;
    return 0;
}

// the instantiation pt_instantiation picks for a scene with attributes (always the full feature set) / without
template <u32 X>
void render_one(const Packing &k, RegStash &st, u32 x, u32 y, const LaneJob &job, u32 &sg)
{
    const u32 f = k.pk.features;
    if (f & F_VATTR) {
        if (f & F_BVH) render_pixel<F_ALL | F_BVH | F_VATTR | X>(k.S, st, x, y, job, sg); else render_pixel<F_ALL | F_VATTR | X>(k.S, st, x, y, job, sg);
    } else {
        if (f & F_BVH) render_pixel<F_ALL | F_BVH | X>(k.S, st, x, y, job, sg); else render_pixel<F_ALL | X>(k.S, st, x, y, job, sg);
    }
}

template <u32 X>
AovPixel aov_one(const Packing &k, u32 x, u32 y)
{
    const u32 f = k.pk.features;
    if (f & F_VATTR) return (f & F_BVH) ? aov_pixel<F_ALL | F_BVH | F_VATTR | X>(k.S, x, y) : aov_pixel<F_ALL | F_VATTR | X>(k.S, x, y);
    return (f & F_BVH) ? aov_pixel<F_ALL | F_BVH | X>(k.S, x, y) : aov_pixel<F_ALL | X>(k.S, x, y);
}

}  // namespace

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
int va_aov(const mrt_render_desc *d, const mrt_desc_ext *ext, uint32_t deep_nodes, float *guide, float *albedo, int32_t *renderer)
{
    Packing k;
    const int rc = pack(d, ext, deep_nodes, k);
    if (rc) return rc;
    unsigned long long seg[8] = {0};
    k.P.segments = seg;
    for (u32 y = 0; y < k.pk.nh; ++y)
        for (u32 x = 0; x < k.pk.nw; ++x) {
            const AovPixel a = k.deep ? aov_one<F_COLD | F_DEEP>(k, x, y) : (k.warm ? aov_one<F_COLD>(k, x, y) : aov_one<0u>(k, x, y));
            const size_t p = (size_t)y * k.pk.nw + x;
            memcpy(guide + 8 * p, &a.g, sizeof(DnGuide));
            albedo[3 * p] = a.albedo.x; albedo[3 * p + 1] = a.albedo.y; albedo[3 * p + 2] = a.albedo.z;
            renderer[p] = a.rend;
        }
    return 0;
}

// the path tracer's per-lane body over the whole frame (tests/emu/emu.cpp emu_render_deep with attributes): accum[nh][nw][3]
int va_render(const mrt_render_desc *d, const mrt_desc_ext *ext, uint64_t seed, uint32_t sample_base, uint32_t n_samples, uint32_t threads,
              uint32_t deep_nodes, float *accum)
{
    Packing k;
    const int rc = pack(d, ext, deep_nodes, k);
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
                if (k.deep) render_one<F_COLD | F_DEEP>(k, st, x, y, job, sg);
                else if (k.warm) render_one<F_COLD>(k, st, x, y, job, sg);
                else render_one<0u>(k, st, x, y, job, sg);
            }
        }
    });
    for (auto &th : pool) th.join();
    return 0;
}

}
