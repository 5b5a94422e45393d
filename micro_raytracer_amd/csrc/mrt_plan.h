// mrt_plan.h — the launch plan of a context and the environment switches of the library.  Plain C++ with no HIP dependency: the
// policy is checked, and can be built stand-alone under a sanitizer, where no device exists (mrt_plan_launch).
#pragma once
#include "../../include/mrt.h"
#include "mrt_inst.h"
#include "mrt_pack.h"

namespace mrt {

constexpr size_t kLdsLimit = 160u * 1024u;          // LDS per CU on gfx950
constexpr size_t kSmallScene = 6u * 1024u;          // <= this: launches of less than one sample chunk take the plain grid (no tile counter)

// Every environment switch of the library (experiments, tests), read by from_env() alone: once per mrt_create / mrt_plan_launch
// (the tests change the environment between contexts), never on the path of mrt_execute.  A group's sub-contexts get the group's.
//   MRT_SCENE_IN_L2, MRT_NO_PERSIST,               on when set, whatever the value ("0" and empty included)
//   MRT_PARTIAL_FAIL_ALLOC, MRT_FORCE_RCCL
//   MRT_DEFER, MRT_DEBUG_FALLBACKS                 a non-zero number ("MRT_DEFER=0" and an empty value are off)
//   MRT_COLD                                       unset / atoi == 0 (forbid the warm level) / atoi != 0 (force it): three states
//   MRT_DEEP_NODES                                 set-ness forces the deep level; value by strtoul, clamped to the room
//   MRT_BLOCK_THREADS                              atoi; only 64 (not on a cold level), 256, 512, 1024 count, and only if they fit
//   MRT_WALK_CAP                                   atoi within [4, kWalkCapMax], else the default: entries of the deep level's walk area
//   MRT_AXIS_SCAN                                  set and atoi == 0 switches the axis scan of mrt_trace.h off
//   MRT_K_SPLIT                                    atoi, values below 1 become 1: forced lanes per pixel
//   MRT_MAX_CHUNKS                                 atoi > 0: chunks per launch
//   MRT_BANDS                                      "48,8,4,2,1,1": forced band lengths of a tapered launch (plan_bands), non-increasing,
//                                                  at most kMaxBands above 1; an invalid list is ignored
//   MRT_PARTIAL_LIMIT_BYTES                        strtoull: budget of the chunk planes
//   MRT_LOOKAHEAD                                  atoi <= 1 disables the look-ahead, else min(v, 64) samples per launch at most
//   MRT_GPUS                                       atoi, used only when mrt_opts.n_devices == 0 (the Rust shim's knob)
struct Knobs {
    bool scene_in_l2 = false, no_persist = false, partial_fail_alloc = false, force_rccl = false, defer = false, debug_fallbacks = false;
    int cold = -1;                                // MRT_COLD: -1 unset, 0 forbids the warm level, 1 forces it
    bool deep_set = false;                        // MRT_DEEP_NODES ...
    size_t deep_nodes = 0;                        // ... and its value
    u32 block_threads = 0, k_split = 0, max_chunks = 0, gpus = 0;      // 0: unset
    size_t partial_budget = 0;                    // 0: unset
    u32 walk_cap = kWalkCapDefault;
    bool axis_scan = true, lookahead_off = false;
    u32 lookahead_max = 0;                        // 0: the default
    u32 n_bands = 0;                              // MRT_BANDS: entries of bands[] (0: unset) ...
    u32 bands[64] = {};                           // ... and the lengths
    static Knobs from_env();
};

// The bands of one tapered launch of n_chunks sample chunks: the listed bands (longest first, each longer than one chunk), then
// every remaining chunk as a band of its own.  items = n + (n_chunks - tail) bands in all, which cover chunks 0 .. n_chunks - 1
// exactly once, in order, with non-increasing lengths.
struct Bands {
    u32 n = 0, first[kMaxBands] = {}, len[kMaxBands] = {};
    u32 tail = 0;                                 // first chunk of the single-chunk bands
    u32 items = 0;
};
// tiles: 8x8 wave tiles of the launch; slots: wavefronts resident on the device at once; the knobs' MRT_BANDS list overrides the rule
Bands plan_bands(u32 n_chunks, unsigned long long tiles, unsigned long long slots, const Knobs &knobs);

// What a context stages in LDS and the shape of its launches: the one record of plan_launch's outcome.
struct Plan {
    bool in_lds = true;
    u32 block_threads = 256;                      // workgroup size of the batched launches = tiles_x x tiles_y wavefronts
    u32 tiles_x = 2, tiles_y = 2;
    bool small_plain_grid = false;                // launches of less than one sample chunk (the per-sample calls of the reference's callers) take
                                                  // the plain grid, one workgroup per 2x2 wave tiles: no tile counter to reset and draw from
    size_t staged_bytes = 0, lds_bytes = 0;       // packed scene bytes a workgroup stages (read through L2: the whole scene); pt_lds_bytes
    u32 inst = 0;                                 // pt_instantiation: the kernel's FEAT template argument
    u32 staging = 0;                              // mrt_plan.staging: 0 all | 1 warm | 2 deep | 3 none
};

// A pure function of the packed scene and the knobs: no device, no environment.  May re-pack the scene (deep staging: 4-wide
// triangle BVHs); sets pk.features (shape markers, F_IDENT), pk.P.walk_cap, n_tbvh_hot, lds_words_hot and axis_scan.
void plan_launch(const mrt_render_desc *desc, const mrt_desc_ext *ext, const Knobs &knobs, Packed &pk, Plan &pl);
void fill_stats(const Plan &pl, mrt_stats &st);      // the plan-derived fields of mrt_stats
// mrt_plan of a planned scene; tbvh_nodes: the scene's triangle-BVH nodes as first packed (binary)
void fill_plan(const Plan &pl, const Packed &pk, u32 tbvh_nodes, mrt_plan &out);

}  // namespace mrt
