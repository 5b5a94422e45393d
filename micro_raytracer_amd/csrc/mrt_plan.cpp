// mrt_plan.cpp — the launch policy of mrt_create (mrt_plan.h): staging level, launch shape, walk areas; and the one reader of the
// library's environment switches.
#include "mrt_plan.h"

#include <stdlib.h>
#include <string.h>

#include <string>

namespace mrt {

Knobs Knobs::from_env()
{
    // on when it holds a non-zero number ("MRT_DEFER=0" and an empty value are off)
    auto env_on = [](const char *name) { const char *v = getenv(name); return v && *v && strtol(v, nullptr, 10) != 0; };
    Knobs k;
    k.scene_in_l2 = getenv("MRT_SCENE_IN_L2") != nullptr;
    k.no_persist = getenv("MRT_NO_PERSIST") != nullptr;
    k.partial_fail_alloc = getenv("MRT_PARTIAL_FAIL_ALLOC") != nullptr;
    k.force_rccl = getenv("MRT_FORCE_RCCL") != nullptr;
    k.defer = env_on("MRT_DEFER");
    k.debug_fallbacks = env_on("MRT_DEBUG_FALLBACKS");
    if (const char *f = getenv("MRT_COLD")) k.cold = atoi(f) ? 1 : 0;
    if (const char *f = getenv("MRT_DEEP_NODES")) { k.deep_set = true; k.deep_nodes = (size_t)strtoul(f, nullptr, 10); }
    if (const char *f = getenv("MRT_BLOCK_THREADS")) k.block_threads = (u32)atoi(f);
    if (const char *f = getenv("MRT_WALK_CAP")) { const int v = atoi(f); if (v >= 4 && v <= (int)kWalkCapMax) k.walk_cap = (u32)v; }
    if (const char *f = getenv("MRT_AXIS_SCAN")) { if (!atoi(f)) k.axis_scan = false; }
    if (const char *f = getenv("MRT_K_SPLIT")) { const int v = atoi(f); k.k_split = v < 1 ? 1u : (u32)v; }
    if (const char *f = getenv("MRT_MAX_CHUNKS")) { const int v = atoi(f); if (v > 0) k.max_chunks = (u32)v; }
    if (const char *f = getenv("MRT_PARTIAL_LIMIT_BYTES")) k.partial_budget = (size_t)strtoull(f, nullptr, 10);
    if (const char *f = getenv("MRT_LOOKAHEAD")) { const int v = atoi(f); if (v <= 1) k.lookahead_off = true; else k.lookahead_max = v > 64 ? 64u : (u32)v; }
    if (const char *f = getenv("MRT_GPUS")) k.gpus = (u32)atoi(f);
    if (const char *f = getenv("MRT_BANDS")) {
        // lengths >= 1, non-increasing, at most kMaxBands of them above 1
        u32 n = 0, above = 0, prev = 0xffffffffu;
        bool ok = *f != 0;
        while (ok && *f) {
            char *end = nullptr;
            const unsigned long v = strtoul(f, &end, 10);
            ok = end != f && v >= 1ul && v <= prev && n < 64u && (*end == ',' || *end == 0);
            if (!ok) break;
            k.bands[n++] = prev = (u32)v;
            if (v > 1ul) ++above;
            f = *end ? end + 1 : end;
        }
        k.n_bands = (ok && above <= kMaxBands) ? n : 0u;
    }
    return k;
}

// The rule.  Items are drawn longest band first by wavefronts that never stop.  When the last item of a band is drawn it runs for
// a whole item, and every other wavefront slot has to find work behind the band for as long: about one item of the band per slot
// if every tile cost the same, more where tiles differ (a tile's paths are up to twice the mean's length on the headline frame),
// and what lies behind drains in the same way.  So a band of L chunks must leave kBandSlack of its items per slot behind it:
// tiles * (rem - L) >= kBandSlack * slots * L, that is L = rem * tiles / (tiles + kBandSlack * slots), rounded down.  Below two
// chunks the rest are single chunks -- the shortest item there is, so the launch drains at the length of one chunk.
// kBandSlack is measured (1080p x 1024 samples, 32400 tiles on 8192 slots, ms per step against 190.8 with interleaved items):
// 2: 191.8, 3: 186.5, 4: 187.0, 6: 188.1, 8: 188.8 -- the far side of the knee, 4, stands (bands of 31, 16, 8, 4, 2 and 3 x 1).
constexpr unsigned long long kBandSlack = 4ull;
Bands plan_bands(u32 n_chunks, unsigned long long tiles, unsigned long long slots, const Knobs &knobs)
{
    Bands b;
    u32 at = 0;
    if (!tiles) tiles = 1ull;
    for (u32 i = 0; at < n_chunks && b.n < kMaxBands; ++i) {
        const u32 rem = n_chunks - at;
        unsigned long long L = (unsigned long long)rem * tiles / (tiles + kBandSlack * slots);
        if (knobs.n_bands) L = i < knobs.n_bands ? knobs.bands[i] : 1ull;
        if (L > rem) L = rem;
        if (L < 2ull) break;
        b.first[b.n] = at; b.len[b.n] = (u32)L; ++b.n;
        at += (u32)L;
    }
    b.tail = at;
    b.items = b.n + (n_chunks - at);
    return b;
}

namespace {

// What is staged in LDS, and the launch shape.
// LDS per workgroup = staged scene + lane stash (+ the mesh kernels' walk areas): pt_lds_bytes knows.  Staging levels:
//   all     the whole packed scene (minus the octree leaf lists);
//   warm    F_COLD: texels stay in global memory (touched at most once per shaded hit); mesh kernels get a per-lane walk area;
//   deep    F_COLD | F_DEEP: meshes beyond the LDS.  The triangle-BVH table is in level order, so as many of its first
//           nodes -- the top levels of every tree -- as fit next to the small tables are staged; deeper nodes and the
//           triangles are read from global memory too;
//   none    everything through L2 (the small tables themselves do not fit).
// Launch shape, chosen for resident wavefronts per CU (the kernel is VALU-issue bound and wants >= 16): the smallest
// workgroup that reaches 16 waves per CU wins (smaller workgroups balance better), else the shape with the most:
//   256 threads (2x2 wave tiles of 8x8 pixels) + 10 KB lane stash per copy of the scene (64-thread workgroups -- one
//   wavefront, its own 5.5 KB of LDS -- remain as a forced shape for the tests);
//   512 threads (4x2 tiles), no stash; 1024 threads (4x4 tiles) + 40 KB stash: one LDS copy serves 16 waves.
// Mesh kernels of the warm and deep levels own a per-lane walk area (Params.walk_cap entries, mrt_trace.h): the leaf queue
// of the binary walk (8 to 16 entries, warm: what the LDS has left), or node stack + leaf queue of the 4-wide walk (16
// entries, deep: the scene is packed again with 4-wide triangle BVHs).
// The knobs that force a level, a shape or a walk area: mrt_plan.h.
constexpr u32 kWarm = F_COLD, kDeep = F_COLD | F_DEEP;

// LDS of a workgroup of `shape` threads at the staging level `marker`, and the resident wavefronts per CU it allows
size_t lds_of(const Packed &pk, u32 shape, u32 marker) { return pt_lds_bytes(pk.P, shape, true, (pk.features & (F_ALL | F_BVH)) | marker); }
bool fits(const Packed &pk, u32 shape, u32 marker) { return lds_of(pk, shape, marker) <= kLdsLimit; }
bool fits_any(const Packed &pk, u32 marker) { return fits(pk, 256u, marker) || fits(pk, 512u, marker) || fits(pk, 1024u, marker); }
size_t waves(const Packed &pk, u32 shape, u32 marker)
{
    const size_t l = lds_of(pk, shape, marker);
    return l > kLdsLimit ? (size_t)0 : (shape / 64u) * (kLdsLimit / (l ? l : 1));
}

// Step 1, the staging level: 0, kWarm or kDeep, or in_lds = false for none.  The deep level packs the scene again.
u32 staging_level(const mrt_render_desc *desc, const mrt_desc_ext *ext, const Knobs &knobs, bool mesh_walk, Packed &pk, bool &in_lds)
{
    const bool has_warm = pk.P.lds_words_warm < pk.P.lds_words || mesh_walk;     // (mesh kernels: the warm marker also buys the walk area)
    u32 cold = 0u;
    in_lds = !knobs.scene_in_l2;
    if (!in_lds) return cold;
    const bool warm_ok = has_warm && fits_any(pk, kWarm) && knobs.cold != 0;
    const bool all_ok = fits_any(pk, 0u) && !(knobs.cold == 1 && warm_ok);
    // a mesh scene takes the warm level when a 16-wave workgroup fits with stash and leaf queues (closest-hit walks in one
    // round: VALU -8.5 %, time -2 % on the 967-triangle bench scene); everything else takes the whole scene when it fits;
    // an instance-BVH scene whose texels alone force a single 1024-thread workgroup per CU takes the warm level too: its
    // kernel is built for 6 waves per SIMD, which 256-thread workgroups around an LDS copy without the texels can supply
    const bool bvh_no_mesh = (pk.features & F_BVH) != 0u && (pk.features & F_TRI) == 0u;
    if (knobs.deep_set && mesh_walk) cold = kDeep;
    else if (mesh_walk && warm_ok && fits(pk, 1024u, kWarm)) cold = kWarm;
    else if (bvh_no_mesh && warm_ok && knobs.cold < 0 && waves(pk, 256u, 0u) < 16u && waves(pk, 256u, kWarm) >= 24u) cold = kWarm;
    else if (all_ok) cold = 0u;
    else if (warm_ok) cold = kWarm;
    else if (mesh_walk) cold = kDeep;
    else in_lds = false;
    if (cold == kDeep) {
        // packed again with 4-wide triangle BVHs in level order; everything hot in front of the node table + lane stash +
        // walk areas of one 1024-thread workgroup; the rest of the LDS holds the first nodes of the table
        PackOpts po; po.tbvh_wide = true;
        Packed again; std::string err2;
        bool ok2 = pack_scene(desc, again, err2, po, ext) == MRT_OK && again.tbvh_wide;
        const size_t fixed = (size_t)ST_SLOTS * 1024u * sizeof(float) + (size_t)knobs.walk_cap * 1024u * sizeof(u32) + 1024u;
        const size_t front = ok2 ? (size_t)again.P.off_tbvh * 4 : 0;
        ok2 = ok2 && front + fixed < kLdsLimit;
        if (ok2) {
            const size_t room = (kLdsLimit - fixed - front) / (B4_WORDS * 4);
            size_t n = knobs.deep_set ? knobs.deep_nodes : room;
            if (n > room) n = room;
            if (n > again.n_tbvh_nodes) n = again.n_tbvh_nodes;
            const u32 n_mesh = (again.P.off_node - again.P.off_mesh) / MESH_WORDS;
            ok2 = n >= n_mesh && n_mesh > 0u;            // every root is staged
            if (ok2) {
                const u32 keep = pk.features;
                pk = again;
                pk.features = keep;
                pk.P.walk_cap = knobs.walk_cap;
                pk.P.n_tbvh_hot = (u32)n;
                pk.P.lds_words_hot = (pk.P.off_tbvh + (u32)n * B4_WORDS + 3u) & ~3u;
            }
        }
        if (!ok2) { cold = 0u; in_lds = false; }
    }
    return cold;
}

// Step 2, the launch shape at the staging level `cold`: pl.block_threads and pl.small_plain_grid; returns the shape markers
// (cold, or F_NOSTASH)
u32 launch_shape(const Knobs &knobs, const Packed &pk, u32 cold, bool in_lds, size_t blob_bytes, Plan &pl)
{
    u32 want = 256u, marker = cold;
    pl.small_plain_grid = false;
    if (in_lds) {
        const size_t w256 = waves(pk, 256u, cold), w512 = waves(pk, 512u, cold), w1024 = waves(pk, 1024u, cold);
        // small scenes (<= 6 KB: ~29 single-wave workgroups per CU would fit): 256-thread workgroups all the same -- four waves
        // around one LDS copy, so that 32 waves per CU fit: +4 % on the headline frame, +7 % with the 8-wave build of the plane /
        // sphere kernel, +4 % on CornellBox2 -- persistent for batched launches, on the plain grid for launches of less than
        // one sample chunk (a one-sample pass over the 1080p frame: persistent 0.56 ms, single-wave workgroups 0.39, this 0.37)
        if (w256 >= 16u) { want = 256u; pl.small_plain_grid = blob_bytes <= kSmallScene && !cold; }
        else if (w512 >= 16u) want = 512u;
        else if (w1024 >= 16u) want = 1024u;
        else if (w256 >= w512 && w256 >= 8u) want = 256u;
        else if (!cold && fits(pk, 1024u, F_NOSTASH)) { want = 1024u; marker |= F_NOSTASH; }      // one LDS copy for 16 waves, lane state in registers
        else want = w1024 ? 1024u : (w512 ? 512u : 256u);
        const u32 f = knobs.block_threads;
        if ((f == 64u && !cold) || f == 256u || f == 512u || f == 1024u) { if (fits(pk, f, cold)) { want = f; marker = cold; pl.small_plain_grid = false; } }
    }
    pl.block_threads = want;
    pl.tiles_x = want == 64u ? 1u : (want == 256u ? 2u : 4u);
    pl.tiles_y = want == 64u ? 1u : (want == 1024u ? 4u : 2u);
    return marker;
}

// Step 3: the leaf queue of the warm mesh kernels takes what the LDS has left while the workgroups per CU stay the same
// (967-triangle bench scene: 13 entries, +2 % over 8: fewer walks need a second round)
void grow_leaf_queue(Packed &pk, u32 shape, u32 marker)
{
    const size_t w0 = waves(pk, shape, marker);
    while (pk.P.walk_cap < kWalkCapMax) {
        ++pk.P.walk_cap;
        if (waves(pk, shape, marker) != w0) { --pk.P.walk_cap; break; }
    }
}

}  // namespace

void plan_launch(const mrt_render_desc *desc, const mrt_desc_ext *ext, const Knobs &knobs, Packed &pk, Plan &pl)
{
    const bool mesh_walk = pk.n_tbvh_nodes != 0u && (pk.features & (F_TRI | F_BOX)) == (F_TRI | F_BOX);
    pk.P.walk_cap = mesh_walk ? kLeafQueue : 0u;         // (only kernels with a walk area count it: pt_lds_bytes)
    bool in_lds = true;
    const u32 cold = staging_level(desc, ext, knobs, mesh_walk, pk, in_lds);
    const size_t full_bytes = (size_t)pk.P.lds_words * 4;
    const size_t blob_bytes = in_lds ? (size_t)staged_words_for(pk.P, cold) * 4 : full_bytes;
    const u32 marker = launch_shape(knobs, pk, cold, in_lds, blob_bytes, pl);
    pk.features = (pk.features & (F_ALL | F_BVH | F_VATTR | F_ENV)) | marker | (pk.all_ident ? (u32)F_IDENT : 0u);      // (pt_instantiation: which shapes have F_IDENT builds)
    // MRT_AXIS_SCAN=0 (tests, A/B runs): the closest-hit scan of the plain F_IDENT kernel keeps its generic body for every query
    if (!knobs.axis_scan) pk.P.axis_scan = 0u;
    if (in_lds && marker == kWarm && mesh_walk && has_walk_area(pk.features)) grow_leaf_queue(pk, pl.block_threads, marker);
    pl.in_lds = in_lds;
    pl.staged_bytes = blob_bytes;
    pl.lds_bytes = pt_lds_bytes(pk.P, pl.block_threads, in_lds, pk.features);
    pl.inst = pt_instantiation(pl.block_threads, in_lds, pk.features);
    pl.staging = !in_lds ? 3u : ((pk.features & F_DEEP) ? 2u : ((pk.features & F_COLD) ? 1u : 0u));
}

void fill_stats(const Plan &pl, mrt_stats &st)
{
    st.lds_bytes = (u32)pl.lds_bytes; st.block_threads = pl.block_threads; st.scene_bytes = (u32)pl.staged_bytes;
    st.kernel_features = pl.inst; st.scene_in_lds = pl.in_lds ? 1u : 0u;
}

void fill_plan(const Plan &pl, const Packed &pk, u32 tbvh_nodes, mrt_plan &out)
{
    memset(&out, 0, sizeof out);
    out.staging = pl.staging;
    out.block_threads = pl.block_threads;
    out.lds_bytes = (uint32_t)pl.lds_bytes;
    out.staged_bytes = pl.in_lds ? (uint32_t)pl.staged_bytes : 0u;
    out.scene_bytes = pk.P.lds_words * 4u;
    out.kernel_features = pl.inst;
    out.tbvh_nodes = tbvh_nodes;
    out.tbvh_hot_nodes = pl.staging == 3u ? 0u : (pl.staging == 2u ? pk.P.n_tbvh_hot : tbvh_nodes);
    out.small_plain_grid = pl.small_plain_grid ? 1u : 0u;
    out.walk_cap = pk.P.walk_cap;
}

}  // namespace mrt
