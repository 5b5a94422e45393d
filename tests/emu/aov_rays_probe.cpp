// TEST INFRASTRUCTURE: x86 build of the supplied-ray AOV body and of the a-trous pass on a frame periodic in x (csrc/mrt_denoise.h:
// aov_ray, dn_pass_host with wrap_x), for tests/test_aov_rays_host.py and tests/test_gpu_aov_rays.py.
// Built by the tests themselves through tests/emu/build.py: the flags of tests/emu/Makefile, with mrt_pack.cpp.
#include <stddef.h>
#include <string.h>

#include <string>
#include <vector>

// the whole scene staged, without / with instance BVH, per-corner attributes and environment: what lane_inst names at level 0
#define LANE_FEAT_LIST LANE_F(F_ALL) LANE_F(F_ALL | F_BVH) LANE_F(F_ALL | F_VATTR) LANE_F(F_ALL | F_BVH | F_VATTR) \
    LANE_F(F_ALL | F_VATTR | F_ENV) LANE_F(F_ALL | F_BVH | F_VATTR | F_ENV)
#include "lane_host.h"

using namespace mrt;

static std::string g_err;

extern "C" {

const char *ar_error(void) { return g_err.c_str(); }

// the supersampled frame of a description: dims[2] = nw, nh
int ar_dims(const mrt_render_desc *d, const mrt_desc_ext *ext, uint32_t *dims)
{
    lane::Packing k;
    const int rc = lane::pack(d, ext, PackOpts(), lane::Level(), k, g_err);
    if (rc) return rc;
    dims[0] = k.pk.nw; dims[1] = k.pk.nh;
    return 0;
}

// the lens-centre ray of every pixel as aov_pixel forms it: orig, dir [nh][nw][3]
int ar_camera_rays(const mrt_render_desc *d, const mrt_desc_ext *ext, float *orig, float *dir)
{
    lane::Packing k;
    const int rc = lane::pack(d, ext, PackOpts(), lane::Level(), k, g_err);
    if (rc) return rc;
    lane::camera_rays(k, orig, dir, [&](u32 x, u32 y, V3 &o, V3 &dd) {
        camera_ray_centre(k.P, k.S.F + k.P.off_cam, pixel_focus(k.P, (float)x, (float)y), o, dd);
    });
    return 0;
}

// aov_pixel over the frame (mrt_aov): guide[nh][nw][8], albedo[nh][nw][3], renderer / instance[nh][nw]
int ar_aov_pixel(const mrt_render_desc *d, const mrt_desc_ext *ext, float *guide, float *albedo, int32_t *renderer, int32_t *instance)
{
    lane::Packing k;
    const int rc = lane::pack(d, ext, PackOpts(), lane::Level(), k, g_err);
    if (rc) return rc;
    return lane::aov_frame(k, lane::lane_inst(k.pk, 0u, false), guide, albedo, renderer, instance, g_err);
}

// aov_ray on n rays traced as given (mrt_aov_rays; n = nw * nh for a grid): guide[n][8], albedo[n][3], renderer / instance[n], the
// instance within its renderer
int ar_aov_rays(const mrt_render_desc *d, const mrt_desc_ext *ext, uint64_t n, const float *orig, const float *dir, float *guide, float *albedo,
                int32_t *renderer, int32_t *instance)
{
    lane::Packing k;
    const int rc = lane::pack(d, ext, PackOpts(), lane::Level(), k, g_err);
    if (rc) return rc;
    unsigned long long seg[8] = {0};
    k.P.segments = seg;
    const std::vector<u32> first = inst_first(k.pk);
    const u32 inst = lane::lane_inst(k.pk, 0u, false);
    const bool known = lane::with_feat(inst, [&](auto feat) {
        for (size_t p = 0; p < n; ++p)
            lane::aov_store(aov_ray<decltype(feat)::value>(k.S, lane::ray_at(orig, p), lane::ray_at(dir, p)), first, p, guide, albedo, renderer, instance);
    });
    k.P.segments = nullptr;
    return known ? 0 : lane::no_inst(inst, g_err);
}

// one pass of the filter over e[nh][nw][3] at this step: out[nh][nw][3]
void ar_pass(const float *e, const float *guide, uint32_t nw, uint32_t nh, uint32_t step, float sc, float sn, float sp, uint32_t wrap_x, float *out)
{
    dn_pass_host(e, reinterpret_cast<const DnGuide *>(guide), nw, nh, step, sc, sn, sp, out, wrap_x != 0u);
}

// mrt_denoise on installed planes: lane::atrous_host with the wrap flag -- the filtered means out[nh][nw][3] of the sums
// A[nh][nw][3] at per-pixel counts[nh][nw]; env: the context has an environment texture
void ar_filter(const float *A, const uint32_t *counts, const float *guide, const float *albedo, uint32_t nw, uint32_t nh, uint32_t passes,
               float sc, float sn, float sp, uint32_t env, uint32_t wrap_x, float *out)
{
    lane::atrous_host(A, counts, guide, albedo, nw, nh, passes, sc, sn, sp, env != 0u, out, wrap_x != 0u);
}

}
