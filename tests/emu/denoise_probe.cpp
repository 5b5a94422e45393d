// TEST INFRASTRUCTURE: x86 build of csrc/mrt_denoise.h (first-hit AOVs, a-trous filter) and the host packer, for
// tests/test_denoise_host.py and tests/test_gpu_denoise.py.
// Built by the tests themselves through tests/emu/build.py: the flags of tests/emu/Makefile, with mrt_pack.cpp.
#include <stddef.h>
#include <string.h>

#include <string>

#define LANE_FEAT_LIST LANE_F(F_ALL) LANE_F(F_ALL | F_BVH)      // scenes without mrt_desc_ext, whole scene staged
#include "lane_host.h"

using namespace mrt;

static std::string g_err;

extern "C" {

const char *dn_error(void) { return g_err.c_str(); }

// mrt_aov of a scene: guide[nh][nw][8] (normal, depth, world point, hit flag), albedo[nh][nw][3], renderer / instance[nh][nw]
// (instance within its renderer, as mrt_aov reports it)
int dn_aov(const mrt_render_desc *d, float *guide, float *albedo, int32_t *renderer, int32_t *instance)
{
    lane::Packing k;
    const int rc = lane::pack(d, nullptr, PackOpts(), lane::Level(), k, g_err);
    if (rc) return rc;
    return lane::aov_frame(k, lane::lane_inst(k.pk, 0u, false), guide, albedo, renderer, instance, g_err);
}

// mrt_denoise: the filtered means out[nh][nw][3] of the sums A[nh][nw][3] at per-pixel counts[nh][nw], guided by guide / albedo
void dn_filter(const float *A, const uint32_t *counts, const float *guide, const float *albedo, uint32_t nw, uint32_t nh, uint32_t passes,
               float sc, float sn, float sp, float *out)
{
    lane::atrous_host(A, counts, guide, albedo, nw, nh, passes, sc, sn, sp, false, out);
}

}
