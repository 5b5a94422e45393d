// lane_host.h -- TEST INFRASTRUCTURE: the x86 lane harness the probes of this directory share.  Packs a scene the way mrt_create
// does and wires up the Scn the lane code reads (pack), names the kernel instantiation a probe runs (lane_inst: the full feature
// set at a staging level, or the F_IDENT build pt_instantiation of csrc/mrt_inst.h picks), dispatches a run-time FEAT to its
// compiled instantiation (with_feat over LANE_FEAT_LIST) and runs whole frames: the path tracer's render_pixel over a pool of
// row-stealing threads (render_frame), the first-hit AOV pass (aov_frame; aov_store for a probe's own loop over supplied rays), the
// a-trous filter (atrous_host, wrap_x for a grid periodic in x) and the camera-ray loop over a frame (camera_rays); ray_at reads ray
// i of a packed [n][3] array.
// Header-only, and included AFTER a probe's MRT_COUNT / MRT_PROBE* hooks: it is what pulls in mrt_trace.h.
#pragma once
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../micro_raytracer_amd/csrc/mrt_denoise.h"
#include "../../micro_raytracer_amd/csrc/mrt_inst.h"
#include "../../micro_raytracer_amd/csrc/mrt_pack.h"

namespace lane {

using namespace mrt;

// Staging level of the lane code: flags 0 = the whole scene staged (binary triangle BVHs), F_COLD = the warm lane code on them,
// F_COLD | F_DEEP = 4-wide tables of which the first `hot` nodes count as staged (on the CPU both halves are the same memory), with
// walk areas of `walk_cap` entries (0: the packer's)
struct Level {
    u32 flags = 0, hot = 0, walk_cap = 0;
};
// the probes' deep_nodes argument: 0, 0xffffffff = warm, n = deep with n staged nodes
inline Level level_of(u32 deep_nodes, u32 walk_cap = kWalkCapDefault)
{
    Level lv;
    if (deep_nodes == 0xffffffffu) lv.flags = F_COLD;
    else if (deep_nodes) { lv.flags = F_COLD | F_DEEP; lv.hot = deep_nodes; lv.walk_cap = walk_cap; }
    return lv;
}

struct Packing {
    Packed pk;
    Params P;
    Scn S;
    std::vector<float> frame;     // pack_scratch: the accumulator of a probe that watches the lanes and keeps no radiance
};

// pack_scene and everything a lane needs beside it: one shard that owns the whole frame, one lane per pixel, the three views of
// the blob on the one copy there is.  Returns pack_scene's code, or -100 for a deep level on a scene without triangle BVH.
inline int pack(const mrt_render_desc *d, const mrt_desc_ext *ext, PackOpts po, const Level &lv, Packing &k, std::string &err)
{
    if (lv.flags & F_DEEP) po.tbvh_wide = true;
    const int rc = pack_scene(d, k.pk, err, po, ext);
    if (rc) return rc;
    if (po.tbvh_wide && !k.pk.tbvh_wide) { err = "no triangle BVH to widen"; return -100; }
    k.P = k.pk.P;
    if (lv.flags & F_DEEP) { k.P.n_tbvh_hot = lv.hot; if (lv.walk_cap) k.P.walk_cap = lv.walk_cap; }
    k.P.local_rows = k.pk.nh; k.P.shard_index = 0; k.P.shard_count = 1; k.P.shard_rows = 8; k.P.k_split = 1;
    k.S.F = reinterpret_cast<const float *>(k.pk.blob.data());
    k.S.U = k.S.F; k.S.G = k.S.F; k.S.P = &k.P; k.S.wk = nullptr; k.S.wk_stride = 1;
    return 0;
}

inline void set_sampling(Packing &k, uint64_t seed, u32 sample_base, u32 n_samples, float *accum)
{
    k.P.seed_lo = (u32)seed; k.P.seed_hi = (u32)(seed >> 32);
    k.P.n_samples = n_samples; k.P.sample_base = sample_base; k.P.accum = accum;
}

// pack for a probe that only watches the lanes run: scenes without mrt_desc_ext, sampling into a frame of the Packing's own
inline int pack_scratch(const mrt_render_desc *d, const Level &lv, uint64_t seed, u32 sample_base, u32 n_samples, Packing &k, std::string &err)
{
    const int rc = pack(d, nullptr, PackOpts(), lv, k, err);
    if (rc) return rc;
    k.frame.assign((size_t)k.pk.nw * k.pk.nh * 3, 0.0f);
    set_sampling(k, seed, sample_base, n_samples, k.frame.data());
    return 0;
}

// The instantiations the x86 build compiles: the full feature set without / with the instance BVH, per-corner attributes and the
// environment at the three staging levels (no deep build with an environment), and the F_IDENT builds of the 256-thread kernels.
// A probe whose entry points run a few of them only may define its own LANE_FEAT_LIST before it includes this header, to spare
// the compile time (each entry costs seconds); whatever is not in the list is an error at run time (with_feat), never another kernel.
#define LANE_LEVELS(F) LANE_F(F) LANE_F((F) | F_COLD) LANE_F((F) | F_COLD | F_DEEP)
#ifndef LANE_FEAT_LIST
#define LANE_FEAT_LIST \
    LANE_LEVELS(F_ALL) LANE_LEVELS(F_ALL | F_BVH) LANE_LEVELS(F_ALL | F_VATTR) LANE_LEVELS(F_ALL | F_BVH | F_VATTR) \
    LANE_F(F_ALL | F_VATTR | F_ENV) LANE_F(F_ALL | F_VATTR | F_ENV | F_COLD) LANE_F(F_ALL | F_BVH | F_VATTR | F_ENV) LANE_F(F_ALL | F_BVH | F_VATTR | F_ENV | F_COLD) \
    LANE_F(F_IDENT) LANE_F(F_IDENT | F_BOX) LANE_F(F_IDENT | F_LIGHTS) LANE_F(F_IDENT | F_BOX | F_LIGHTS) LANE_F(F_IDENT | F_BVH) LANE_F(F_IDENT | F_LIGHTS | F_BVH)
#endif

// fn(std::integral_constant<u32, FEAT>()) for the instantiation `inst`; false: not one of the list (nothing was called)
template <class Fn>
inline bool with_feat(u32 inst, Fn &&fn)
{
    switch (inst) {
#define LANE_F(F) case (u32)(F): fn(std::integral_constant<u32, (u32)(F)>()); return true;
        LANE_FEAT_LIST
#undef LANE_F
    default: return false;
    }
}
inline int no_inst(u32 inst, std::string &err)
{
    err = "FEAT " + std::to_string(inst) + " is not an instantiation of the x86 harness";
    return -110;
}

// What a probe runs for a packed scene at staging level `level` (Level.flags): the full feature set -- or, with allow_ident at
// level 0, the F_IDENT build wherever the 256-thread kernels with the scene in LDS have one for it (as mrt_create does it: a
// scene whose instances are all untransformed asks pt_instantiation with F_IDENT set)
inline u32 lane_inst(const Packed &pk, u32 level, bool allow_ident)
{
    const u32 scene = pk.features & (F_ALL | F_BVH | F_VATTR | F_ENV);
    if (allow_ident && level == 0u && pk.all_ident) {
        const u32 real = pt_instantiation(256u, true, scene | F_IDENT);
        if (real & F_IDENT) return real;
    }
    return F_ALL | (scene & (F_BVH | F_VATTR | F_ENV)) | level;
}

// The megakernel's per-lane body on pixel (x, y): every sample of the launch, accumulated into P.accum (set_sampling); segments +=
// the path segments traced.  False: `inst` is not in the list
inline bool render_lane(const Packing &k, u32 inst, u32 x, u32 y, uint64_t &segments)
{
    return with_feat(inst, [&](auto feat) {
        u32 sg = 0;
        RegStash st; LaneJob job; job.k = 0; job.word = (y * k.pk.nw + x) * 3u;
        render_pixel<decltype(feat)::value>(k.S, st, x, y, job, sg);
        segments += sg;
    });
}

// render_lane over every pixel of rows [row0, row1) of the frame, accumulating into accum[nh][nw][3]: `threads` threads that take
// the next row each; *segments (may be NULL): the path segments traced
inline int render_frame(Packing &k, u32 inst, uint64_t seed, u32 sample_base, u32 n_samples, u32 row0, u32 row1, u32 threads, float *accum,
                        uint64_t *segments, std::string &err)
{
    if (!with_feat(inst, [](auto) {})) return no_inst(inst, err);
    set_sampling(k, seed, sample_base, n_samples, accum);
    if (row1 > k.pk.nh) row1 = k.pk.nh;
    std::atomic<uint32_t> next(row0);
    std::atomic<uint64_t> segs(0);
    if (threads == 0) threads = 1;
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < threads; ++t) pool.emplace_back([&]() {
        uint64_t local = 0;
        for (;;) {
            const uint32_t y = next.fetch_add(1);
            if (y >= row1) break;
            for (uint32_t x = 0; x < k.pk.nw; ++x) render_lane(k, inst, x, y, local);
        }
        segs += local;
    });
    for (auto &th : pool) th.join();
    if (segments) *segments = segs.load();
    return 0;
}

// ray i of a packed [n][3] array, and back
inline V3 ray_at(const float *a, size_t i) { return v3(a[3 * i], a[3 * i + 1], a[3 * i + 2]); }
inline void put3(float *a, size_t i, V3 v) { a[3 * i] = v.x; a[3 * i + 1] = v.y; a[3 * i + 2] = v.z; }

// ray(x, y, o, d) -- how the caller's kernel forms the lens-centre ray of a pixel -- over the frame: orig, dir [nh][nw][3]
template <class Ray>
inline void camera_rays(const Packing &k, float *orig, float *dir, Ray &&ray)
{
    for (u32 y = 0; y < k.pk.nh; ++y)
        for (u32 x = 0; x < k.pk.nw; ++x) {
            V3 o, d;
            ray(x, y, o, d);
            put3(orig, (size_t)y * k.pk.nw + x, o);
            put3(dir, (size_t)y * k.pk.nw + x, d);
        }
}

// One AovPixel into plane entry p: guide[p][8], albedo[p][3], renderer[p] and, where instance is not NULL, instance[p]: the index
// within the renderer's inst list (the flat index less the renderer's first of `first` = inst_first(pk), as mrt_aov maps it)
inline void aov_store(const AovPixel &a, const std::vector<u32> &first, size_t p, float *guide, float *albedo, int32_t *renderer, int32_t *instance)
{
    memcpy(guide + 8 * p, &a.g, sizeof(DnGuide));
    put3(albedo, p, a.albedo);
    renderer[p] = a.rend;
    if (instance) instance[p] = a.rend < 0 ? -1 : a.inst - (i32)first[(u32)a.rend];
}

// mrt_aov: guide[nh][nw][8] (normal, depth, world point, hit flag), albedo[nh][nw][3], renderer[nh][nw] and, where instance is not
// NULL, instance[nh][nw]
inline int aov_frame(Packing &k, u32 inst, float *guide, float *albedo, int32_t *renderer, int32_t *instance, std::string &err)
{
    unsigned long long seg[8] = {0};
    k.P.segments = seg;
    const std::vector<u32> first = inst_first(k.pk);
    const bool known = with_feat(inst, [&](auto feat) {
        for (u32 y = 0; y < k.pk.nh; ++y)
            for (u32 x = 0; x < k.pk.nw; ++x)
                aov_store(aov_pixel<decltype(feat)::value>(k.S, x, y), first, (size_t)y * k.pk.nw + x, guide, albedo, renderer, instance);
    });
    k.P.segments = nullptr;
    return known ? 0 : no_inst(inst, err);
}

// mrt_denoise: the filtered means out[nh][nw][3] of the sums A[nh][nw][3] at per-pixel counts[nh][nw], guided by guide / albedo;
// env: the context has an environment texture (miss pixels demodulated by their albedo too); wrap_x: the frame is periodic in x
inline void atrous_host(const float *A, const uint32_t *counts, const float *guide, const float *albedo, uint32_t nw, uint32_t nh, uint32_t passes,
                        float sc, float sn, float sp, bool env, float *out, bool wrap_x = false)
{
    const size_t np = (size_t)nw * nh;
    const DnGuide *g = reinterpret_cast<const DnGuide *>(guide);
    std::vector<float> e(np * 3), t(np * 3);
    for (size_t p = 0; p < np; ++p) {
        const float rc = 1.0f / (float)counts[p];
        for (int c3 = 0; c3 < 3; ++c3) {
            const float c = A[3 * p + c3] * rc;
            if (passes == 0u) out[3 * p + c3] = c;
            else e[3 * p + c3] = c / dn_demod(albedo[3 * p + c3], g[p].hit, env);
        }
    }
    if (passes == 0u) return;
    for (u32 i = 0; i < passes; ++i) {
        dn_pass_host(e.data(), g, nw, nh, 1u << i, dn_pass_sc(sc, i), sn, sp, t.data(), wrap_x);
        e.swap(t);
    }
    for (size_t p = 0; p < np; ++p)
        for (int c3 = 0; c3 < 3; ++c3) out[3 * p + c3] = e[3 * p + c3] * dn_demod(albedo[3 * p + c3], g[p].hit, env);
}

}  // namespace lane
