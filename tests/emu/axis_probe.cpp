// TEST INFRASTRUCTURE: x86 build of the closest-hit scan of csrc/mrt_trace.h with its axis body (F_IDENT) -- the
// packer's classification and AXIS table, single closest-hit queries through either scan body, and the path tracer's
// render_pixel -- for tests/test_axis_scan.py.  wave_all is the lane's own predicate here, so every ray chooses its body itself.
// Built by the test itself through tests/emu/build.py: the flags of tests/emu/Makefile, with mrt_pack.cpp.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>

// queries answered by the axis body (CT_AXIS_SCAN of mrt_trace.h), per thread: ax_trace reads it around every query
static thread_local unsigned long long g_axis_queries = 0;
#define MRT_COUNT(counter) do { if ((counter) == CT_AXIS_SCAN) ++g_axis_queries; } while (0)

#define LANE_FEAT_LIST LANE_F(F_IDENT)      // the one kernel this probe is about
#include "lane_host.h"                      // (after the hook above)

using namespace mrt;

static std::string g_err;

namespace {

using lane::Packing;

// axis: 0 clears Params.axis_scan, 1 leaves the packer's verdict, -1 follows MRT_AXIS_SCAN as mrt_create does
int pack(const mrt_render_desc *d, int axis, Packing &k)
{
    const int rc = lane::pack(d, nullptr, PackOpts(), lane::Level(), k, g_err);
    if (rc) return rc;
    if (axis < 0) { const char *e = getenv("MRT_AXIS_SCAN"); axis = (e && !atoi(e)) ? 0 : 1; }
    if (!axis) k.P.axis_scan = 0u;
    return 0;
}

// the kernel mrt_create picks is the plain F_IDENT one: every instance untransformed, planes and spheres, no lights, no BVH
bool plain_ident(const Packed &pk) { return pk.all_ident && pk.features == 0u; }

}  // namespace

extern "C" {

const char *ax_error(void) { return g_err.c_str(); }

// info: features, all_ident, Packed.axis_scan, Params.axis_scan, Params.off_axis, n_inst, Params.off_inst, blob_words;
// blob (at most cap words) may be NULL
int ax_pack(const mrt_render_desc *d, uint32_t *info /*[8]*/, uint32_t *blob, uint64_t cap)
{
    Packed pk;
    const int rc = pack_scene(d, pk, g_err);
    if (rc) return rc;
    const uint32_t v[8] = {pk.features, pk.all_ident ? 1u : 0u, pk.axis_scan ? 1u : 0u, pk.P.axis_scan, pk.P.off_axis, pk.P.n_inst, pk.P.off_inst, pk.P.blob_words};
    memcpy(info, v, sizeof v);
    if (blob) memcpy(blob, pk.blob.data(), sizeof(uint32_t) * (size_t)(cap < pk.P.blob_words ? cap : pk.P.blob_words));
    return 0;
}

// n closest-hit queries trace<false, F_IDENT>: out[i] = hit, flat instance, t0 bits, t1 bits, renderer, 1 if the axis body answered
int ax_trace(const mrt_render_desc *d, int axis, uint32_t n, const float *orig, const float *dir, uint32_t *out)
{
    Packing k;
    const int rc = pack(d, axis, k);
    if (rc) return rc;
    if (!plain_ident(k.pk)) { g_err = "not a scene of the plain F_IDENT kernel"; return -100; }
    for (uint32_t i = 0; i < n; ++i) {
        const V3 o = v3(orig[3 * i], orig[3 * i + 1], orig[3 * i + 2]), dr = v3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
        const RayPre ray = ray_pre<F_IDENT>(o, dr);
        Hit h;
        const unsigned long long before = g_axis_queries;
        const bool hit = trace<false, F_IDENT>(k.S, ray, h);
        uint32_t *q = out + (size_t)i * 6;
        q[0] = hit ? 1u : 0u; q[1] = hit ? h.inst : 0u; q[2] = hit ? f2u(h.t0) : 0u; q[3] = hit ? f2u(h.t1) : 0u; q[4] = hit ? (uint32_t)h.rend : 0u;
        q[5] = (uint32_t)(g_axis_queries - before);
    }
    return 0;
}

// the path tracer's per-lane body over the whole frame: accum[nh][nw][3], the path segments traced
int ax_render(const mrt_render_desc *d, int axis, uint64_t seed, uint32_t n_samples, uint32_t threads, float *accum, uint64_t *segments)
{
    Packing k;
    const int rc = pack(d, axis, k);
    if (rc) return rc;
    if (!plain_ident(k.pk)) { g_err = "not a scene of the plain F_IDENT kernel"; return -100; }
    return lane::render_frame(k, F_IDENT, seed, 0, n_samples, 0, k.pk.nh, threads, accum, segments, g_err);
}

}
