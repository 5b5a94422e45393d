// TEST INFRASTRUCTURE: x86 build of the closest-hit scan of csrc/mrt_trace.h (F_IDENT) that counts, per query and
// per frame, how often the axis body is entered (CT_AXIS_SCAN) and how often it hands its query to the generic body after the
// loop (CT_AXIS_REDO: a plane numerator below the division core's window) -- for tests/test_axis_scan_scalar.py.  wave_all is the
// lane's own predicate here, so the counts are per ray; a wavefront of the GPU redoes a query when any of its 64 lanes would.
// Built by the test itself through tests/emu/build.py: the flags of tests/emu/Makefile, with mrt_pack.cpp.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <string>

static thread_local unsigned long long g_cnt[3] = {0, 0, 0};      // closest-hit queries, axis body entered, axis body redone
#define MRT_COUNT(counter) \
    do { if ((counter) == CT_TRACE) ++g_cnt[0]; else if ((counter) == CT_AXIS_SCAN) ++g_cnt[1]; else if ((counter) == CT_AXIS_REDO) ++g_cnt[2]; } while (0)

#define LANE_FEAT_LIST LANE_F(F_IDENT)      // the one kernel this probe is about
#include "lane_host.h"                      // (after the hook above)

using namespace mrt;

static std::string g_err;

extern "C" {

const char *ar_error(void) { return g_err.c_str(); }

// n closest-hit queries trace<false, F_IDENT>: out[i] = hit, flat instance, t0 bits, t1 bits, renderer, axis body entered, redone;
// axis 0 clears Params.axis_scan
int ar_trace(const mrt_render_desc *d, int axis, uint32_t n, const float *orig, const float *dir, uint32_t *out)
{
    lane::Packing k;
    const int rc = lane::pack(d, nullptr, PackOpts(), lane::Level(), k, g_err);
    if (rc) return rc;
    if (!(k.pk.all_ident && k.pk.features == 0u)) { g_err = "not a scene of the plain F_IDENT kernel"; return -100; }
    if (!axis) k.P.axis_scan = 0u;
    for (uint32_t i = 0; i < n; ++i) {
        const V3 o = v3(orig[3 * i], orig[3 * i + 1], orig[3 * i + 2]), dr = v3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
        const RayPre ray = ray_pre<F_IDENT>(o, dr);
        Hit h;
        const unsigned long long scan0 = g_cnt[1], redo0 = g_cnt[2];
        const bool hit = trace<false, F_IDENT>(k.S, ray, h);
        uint32_t *q = out + (size_t)i * 7;
        q[0] = hit ? 1u : 0u; q[1] = hit ? h.inst : 0u; q[2] = hit ? f2u(h.t0) : 0u; q[3] = hit ? f2u(h.t1) : 0u; q[4] = hit ? (uint32_t)h.rend : 0u;
        q[5] = (uint32_t)(g_cnt[1] - scan0); q[6] = (uint32_t)(g_cnt[2] - redo0);
    }
    return 0;
}

// the path tracer's per-lane body over the whole frame on one thread: counts[3] = closest-hit queries, axis body entered, redone;
// info[3] = words of the blob, P.off_axis, P.n_inst
int ar_census(const mrt_render_desc *d, uint64_t seed, uint32_t n_samples, float *accum, uint64_t *counts, uint32_t *info)
{
    lane::Packing k;
    const int rc = lane::pack(d, nullptr, PackOpts(), lane::Level(), k, g_err);
    if (rc) return rc;
    if (!(k.pk.all_ident && k.pk.features == 0u)) { g_err = "not a scene of the plain F_IDENT kernel"; return -100; }
    info[0] = k.pk.P.blob_words; info[1] = k.pk.P.off_axis; info[2] = k.pk.P.n_inst;
    lane::set_sampling(k, seed, 0, n_samples, accum);
    const unsigned long long c0[3] = {g_cnt[0], g_cnt[1], g_cnt[2]};
    uint64_t segs = 0;
    for (uint32_t y = 0; y < k.pk.nh; ++y)
        for (uint32_t x = 0; x < k.pk.nw; ++x)
            if (!lane::render_lane(k, F_IDENT, x, y, segs)) return lane::no_inst(F_IDENT, g_err);
    for (int c = 0; c < 3; ++c) counts[c] = g_cnt[c] - c0[c];
    return 0;
}

}
