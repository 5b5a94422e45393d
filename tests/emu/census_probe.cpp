// TEST INFRASTRUCTURE: x86 build of the REDUCED feature sets of the path-tracing kernel (csrc/mrt_trace.h) for
// tests/test_instantiation_census.py -- the sixteen plain sets of MRT_PLAIN16, the four picks of MRT_BVH4 and the F_IDENT builds
// (csrc/mrt_megakernel.h), each rendering a whole frame through render_pixel.  The full set is among them (15, and 15 | F_BVH):
// a reduced build must be the full build with dead code removed, bit for bit.
// Built by the test itself through tests/emu/build.py: the flags of tests/emu/Makefile, with mrt_pack.cpp.
#include "../../micro_raytracer_amd/csrc/mrt_scene.h"

#define LANE_PLAIN16 LANE_F(0) LANE_F(1) LANE_F(2) LANE_F(3) LANE_F(4) LANE_F(5) LANE_F(6) LANE_F(7) LANE_F(8) LANE_F(9) LANE_F(10) LANE_F(11) \
    LANE_F(12) LANE_F(13) LANE_F(14) LANE_F(15)
#define LANE_FEAT_LIST LANE_PLAIN16 \
    LANE_F(F_BVH) LANE_F(F_LIGHTS | F_BVH) LANE_F((F_ALL & ~F_TRI) | F_BVH) LANE_F(F_ALL | F_BVH) \
    LANE_F(F_IDENT) LANE_F(F_IDENT | F_BOX) LANE_F(F_IDENT | F_LIGHTS) LANE_F(F_IDENT | F_BOX | F_LIGHTS) LANE_F(F_IDENT | F_BVH) LANE_F(F_IDENT | F_LIGHTS | F_BVH)

#include <string>

#include "lane_host.h"

using namespace mrt;

static std::string g_err;

extern "C" {

const char *cs_error(void) { return g_err.c_str(); }

// the instantiations of this build: feat[cap], returns the count
uint32_t cs_list(uint32_t *feat, uint32_t cap)
{
    uint32_t n = 0;
#define LANE_F(F) { if (n < cap) feat[n] = (uint32_t)(F); ++n; }
    LANE_FEAT_LIST
#undef LANE_F
    return n;
}

// the packed scene's feature bits and all_ident: info[2]
int cs_features(const mrt_render_desc *d, const mrt_desc_ext *ext, uint32_t *info)
{
    Packed pk;
    const int rc = pack_scene(d, pk, g_err, PackOpts(), ext);
    if (rc) return rc;
    info[0] = pk.features; info[1] = pk.all_ident ? 1u : 0u;
    return 0;
}

// the per-lane body of instantiation `inst` (exactly that one: anything outside the list is an error) over the whole frame, the
// whole scene staged: accum[nh][nw][3]
int cs_render(const mrt_render_desc *d, const mrt_desc_ext *ext, uint32_t inst, uint64_t seed, uint32_t n_samples, uint32_t threads, float *accum)
{
    lane::Packing k;
    const int rc = lane::pack(d, ext, PackOpts(), lane::Level(), k, g_err);
    if (rc) return rc;
    return lane::render_frame(k, inst, seed, 0, n_samples, 0, k.pk.nh, threads, accum, nullptr, g_err);
}

}
