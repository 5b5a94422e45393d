// TEST INFRASTRUCTURE: x86 build of the ray-query body of csrc/mrt_rayq.h -- the per-ray text of the device hook
// mrt_selftest_trace -- on a scene packed by pack_scene (with or without mrt_desc_ext), for tests/test_ray_query_host.py and
// tests/test_gpu_ray_query.py.  wave_all is the lane's own predicate here, so every ray chooses its bodies itself.
// Built by the tests themselves through tests/emu/build.py: the flags of tests/emu/Makefile, with mrt_pack.cpp.
#include <stdint.h>
#include <string.h>

#include <string>

// closest-hit queries answered by the axis body (CT_AXIS_SCAN of mrt_trace.h): rq_trace reads it around every ray
static thread_local unsigned long long g_axis_queries = 0;
#define MRT_COUNT(counter) do { if ((counter) == CT_AXIS_SCAN) ++g_axis_queries; } while (0)

#include "../../micro_raytracer_amd/csrc/mrt_rayq.h"
#include "lane_host.h"      // (after the hook above)

using namespace mrt;

static std::string g_err;

extern "C" {

const char *rq_error(void) { return g_err.c_str(); }

enum { RQ_FEAT = 0, RQ_AXIS, RQ_WIDE, RQ_HOT, RQ_WALK_CAP, RQ_REF_WALK, RQ_CFG_WORDS = 8 };

// info: Packed.features, all_ident, Packed.axis_scan, n_inst, n_rend, n_bvh_nodes, n_tbvh_nodes, tbvh_wide
int rq_pack(const mrt_render_desc *d, const mrt_desc_ext *ext, uint32_t wide, uint32_t *info /*[8]*/)
{
    Packed pk;
    PackOpts po; po.tbvh_wide = wide != 0u;
    const int rc = pack_scene(d, pk, g_err, po, ext);
    if (rc) return rc;
    const uint32_t v[8] = {pk.features, pk.all_ident ? 1u : 0u, pk.axis_scan ? 1u : 0u, pk.P.n_inst, pk.P.n_rend, pk.n_bvh_nodes, pk.n_tbvh_nodes, pk.tbvh_wide ? 1u : 0u};
    memcpy(info, v, sizeof v);
    return 0;
}

// n rays through rayq_body<FEAT>.  cfg: [RQ_FEAT] the FEAT to run, one of the hook's instantiations  [RQ_AXIS] 0 clears
// Params.axis_scan, 1 leaves the packer's verdict, 2 sets it whatever the packer said (negative controls only)  [RQ_WIDE] 4-wide
// triangle BVHs (F_DEEP)  [RQ_HOT] Params.n_tbvh_hot  [RQ_WALK_CAP] Params.walk_cap (0: kLeafQueue)  [RQ_REF_WALK] meshes through
// the reference's octree walk.  out[i][10]: the MRT_TRACE_WORDS words of the body -- the instance flat, as the kernel leaves it
// -- and the number of closest-hit queries of this ray the axis body answered; inst_first[n_rend] (may be NULL): flat index of
// each renderer's first instance.
int rq_trace(const mrt_render_desc *d, const mrt_desc_ext *ext, const uint32_t *cfg, uint32_t n, const float *orig, const float *dir, uint32_t *out,
             uint32_t *inst_first)
{
    lane::Packing k;
    PackOpts po; po.tbvh_wide = cfg[RQ_WIDE] != 0u;
    const int rc = lane::pack(d, ext, po, lane::Level(), k, g_err);
    if (rc) return rc;
    const Packed &pk = k.pk;
    Params &P = k.P;
    const Scn &S = k.S;
    const u32 feat = cfg[RQ_FEAT];
    if (((feat & F_DEEP) != 0u) != pk.tbvh_wide) { g_err = "F_DEEP goes with the 4-wide table and with nothing else"; return -101; }
    if (((feat & F_BVH) != 0u) != ((pk.features & F_BVH) != 0u)) { g_err = "F_BVH does not match the packed scene"; return -102; }
    if ((feat & F_IDENT) && !pk.all_ident) { g_err = "F_IDENT on a scene with a transformed instance"; return -103; }
    if ((pk.features & F_ALL & ~feat) != 0u) { g_err = "FEAT does not cover the scene"; return -104; }
    if (((pk.features & F_VATTR) != 0u) != ((feat & F_VATTR) != 0u)) { g_err = "F_VATTR does not match the packed scene"; return -105; }
    if (cfg[RQ_AXIS] == 0u) P.axis_scan = 0u;
    if (cfg[RQ_AXIS] == 2u) P.axis_scan = 1u;
    P.n_tbvh_hot = cfg[RQ_HOT];
    P.walk_cap = cfg[RQ_WALK_CAP] ? cfg[RQ_WALK_CAP] : kLeafQueue;
    if (P.walk_cap > kWalkCapMax || P.walk_cap < 4u) { g_err = "walk_cap"; return -106; }
    const bool ref_walk = cfg[RQ_REF_WALK] != 0u;
    if (inst_first) {
        for (u32 r = 0; r < P.n_rend; ++r) inst_first[r] = 0u;
        for (u32 i = P.n_inst; i-- > 0;) inst_first[pk.blob[P.off_instx + i * INSTX_WORDS + INSTX_REND]] = i;
    }
    bool known = false;
    for (uint32_t i = 0; i < n; ++i) {
        const V3 o = v3(orig[3 * i], orig[3 * i + 1], orig[3 * i + 2]), dr = v3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
        uint32_t *q = out + (size_t)i * 10;
        const unsigned long long before = g_axis_queries;
        bool done = false;
#define MRT_RQ(L, F) if (!done && feat == (u32)(F)) { rayq_body<(F)>(S, o, dr, q, ref_walk); done = true; }
        MRT_RAYQ_LIST
#undef MRT_RQ
        known = done;
        if (!done) break;
        q[9] = (uint32_t)(g_axis_queries - before);
    }
    if (n && !known) { g_err = "FEAT " + std::to_string(feat) + " is not an instantiation of the hook"; return -107; }
    return 0;
}

}
