// TEST INFRASTRUCTURE: x86 build of the per-ray bodies of csrc/mrt_rays.h -- the text of mrt_radiance's and mrt_camera_rays' kernels
// -- on a scene packed by pack_scene, for tests/test_rays_host.py and tests/test_gpu_rays.py.
// Built by the tests themselves through tests/emu/build.py: the flags of tests/emu/Makefile, with mrt_pack.cpp.
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../micro_raytracer_amd/csrc/mrt_rays.h"

// what this probe runs: the feature sets of pt_rays (MRT_RAYS_LIST itself) and the F_IDENT builds a scene's own frame kernel may be
#define MRT_RAYS(F) LANE_F(F)
#define LANE_FEAT_LIST MRT_RAYS_LIST \
    LANE_F(F_IDENT) LANE_F(F_IDENT | F_BOX) LANE_F(F_IDENT | F_LIGHTS) LANE_F(F_IDENT | F_BOX | F_LIGHTS) LANE_F(F_IDENT | F_BVH) LANE_F(F_IDENT | F_LIGHTS | F_BVH)
#include "lane_host.h"

using namespace mrt;

static std::string g_err;

extern "C" {

const char *ry_error(void) { return g_err.c_str(); }

// (nw, nh) of the supersampled frame, Packed.features, the scene's own instantiation (lane_inst at level 0, F_IDENT where the
// 256-thread kernels have it) and the one pt_rays runs (pt_instantiation(256, false, features))
int ry_info(const mrt_render_desc *d, const mrt_desc_ext *ext, uint32_t *info /*[8]*/)
{
    lane::Packing k;
    const int rc = lane::pack(d, ext, PackOpts(), lane::Level(), k, g_err);
    if (rc) return rc;
    const uint32_t v[8] = {k.pk.nw, k.pk.nh, k.pk.features, lane::lane_inst(k.pk, 0u, true), pt_instantiation(256u, false, k.pk.features),
                           k.pk.axis_scan ? 1u : 0u, k.P.lds_words, 0u};
    memcpy(info, v, sizeof v);
    return 0;
}

// mrt_camera_rays: orig, dir [nh][nw][3]
int ry_camera_rays(const mrt_render_desc *d, const mrt_desc_ext *ext, float *orig, float *dir)
{
    lane::Packing k;
    const int rc = lane::pack(d, ext, PackOpts(), lane::Level(), k, g_err);
    if (rc) return rc;
    lane::camera_rays(k, orig, dir, [&](u32 x, u32 y, V3 &o, V3 &dr) { camera_ray_of(k.P, k.S.F, x, y, o, dr); });
    return 0;
}

// mrt_radiance: rays_body<feat> on n rays, rgb [n][3] (zeroed here); key may be NULL; *segments may be NULL
int ry_radiance(const mrt_render_desc *d, const mrt_desc_ext *ext, uint32_t feat, uint64_t seed, uint32_t sample_base, uint32_t n_samples,
                uint32_t n, const float *orig, const float *dir, const uint32_t *key, uint32_t threads, float *rgb, uint64_t *segments)
{
    lane::Packing k;
    const int rc = lane::pack(d, ext, PackOpts(), lane::Level(), k, g_err);
    if (rc) return rc;
    if (!lane::with_feat(feat, [](auto) {})) return lane::no_inst(feat, g_err);
    if ((k.pk.features & F_ALL & ~feat) != 0u) { g_err = "FEAT does not cover the scene"; return -104; }
    if ((feat & F_IDENT) && !k.pk.all_ident) { g_err = "F_IDENT on a scene with a transformed instance"; return -103; }
    memset(rgb, 0, (size_t)n * 3 * sizeof(float));
    lane::set_sampling(k, seed, sample_base, n_samples, rgb);
    std::atomic<uint32_t> next(0);
    std::atomic<uint64_t> segs(0);
    if (threads == 0) threads = 1;
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < threads; ++t) pool.emplace_back([&]() {
        uint64_t local = 0;
        for (;;) {
            const uint32_t i0 = next.fetch_add(64);
            if (i0 >= n) break;
            for (uint32_t i = i0; i < n && i < i0 + 64u; ++i)
                lane::with_feat(feat, [&](auto f) {
                    u32 sg = 0;
                    rays_body<decltype(f)::value>(k.S, i, lane::ray_at(orig, i), lane::ray_at(dir, i), key ? key[i] : i, sg);
                    local += sg;
                });
        }
        segs += local;
    });
    for (auto &th : pool) th.join();
    if (segments) *segments = segs.load();
    return 0;
}

}
