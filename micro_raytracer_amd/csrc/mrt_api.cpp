// mrt_api.cpp — the C ABI of include/mrt.h: context management, uploads, launches, read-back.
// Replaces the reference's Sampler (src/sampler.rs:11-100); there is no CPU rendering path here:
// without a HIP device every entry point that needs one fails with MRT_ERR_DEVICE.
#include <hip/hip_runtime_api.h>
#include <dlfcn.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <chrono>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mrt.h"
#include "mrt_denoise.h"
#include "mrt_kernels.h"
#include "mrt_pack.h"
#include "mrt_plan.h"
#include "mrt_trace.h"

using namespace mrt;

namespace {

thread_local std::string g_err;
thread_local int g_status = MRT_OK;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    g_status = code;
    return code;
}
void ok() { g_status = MRT_OK; }

// an error path that still waits for work already launched: the caller gets the first error, rc, whatever `cleanup` runs into
template <class F> int keep_first_error(int rc, F &&cleanup)
{
    const std::string keep = g_err;
    cleanup();
    g_err = keep; g_status = rc;
    return rc;
}

// A HIP call whose failure is tolerated: HIP 7 keeps the last *real* error pending (hipGetLastError no longer reports the
// last call's status), so the pending error is cleared here or the next launch's hipGetLastError() would report it.
bool hip_tolerated(hipError_t e)
{
    if (e == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

#define HIP_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) return fail(MRT_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_));    \
    } while (0)

// ---- owners of device resources: every allocation, event and stream of a context is released by its owner's destructor ----
// `n` elements of T in device memory.  alloc frees what is held, then asks for `count` elements (`bytes` instead when it is
// not 0: MRT_PARTIAL_FAIL_ALLOC asks for an impossible size), and leaves the owner empty when that fails.
template <class T> struct DeviceMem {
    T *p = nullptr;
    size_t n = 0;
    DeviceMem() = default;
    DeviceMem(DeviceMem &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    ~DeviceMem() { reset(); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    hipError_t alloc(size_t count, size_t bytes = 0)
    {
        reset();
        const hipError_t e = hipMalloc((void **)&p, bytes ? bytes : count * sizeof(T));
        if (e == hipSuccess) n = count; else p = nullptr;
        return e;
    }
};
struct EventDestroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct StreamDestroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
using Event = std::unique_ptr<ihipEvent_t, EventDestroy>;
using Stream = std::unique_ptr<ihipStream_t, StreamDestroy>;
hipError_t create(Event &ev) { hipEvent_t e; const hipError_t r = hipEventCreate(&e); if (r == hipSuccess) ev.reset(e); return r; }
hipError_t create(Stream &st) { hipStream_t s; const hipError_t r = hipStreamCreateWithFlags(&s, hipStreamNonBlocking); if (r == hipSuccess) st.reset(s); return r; }

// ---- RCCL, loaded on demand (only in-process multi-device contexts need it; signatures from rccl/rccl.h) ----
typedef struct ncclComm *ncclComm_t;
struct Rccl {
    void *lib = nullptr;
    int (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;                                        // rccl.h:236
    int (*CommDestroy)(ncclComm_t) = nullptr;                                                              // rccl.h:260
    int (*Gather)(const void *, void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;             // rccl.h:745
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;                                                          // rccl.h:339
    std::mutex mu;
    bool load(std::string &err)
    {
        std::lock_guard<std::mutex> lock(mu);
        if (lib) return true;
        for (const char *name : {"/opt/rocm/lib/librccl.so", "librccl.so", "librccl.so.1"}) { lib = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (lib) break; }
        if (!lib) { err = std::string("cannot load librccl.so: ") + dlerror(); return false; }
        CommInitAll = (decltype(CommInitAll))dlsym(lib, "ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        Gather = (decltype(Gather))dlsym(lib, "ncclGather");
        GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd");
        GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        if (!CommInitAll || !CommDestroy || !Gather || !GroupStart || !GroupEnd || !GetErrorString) { err = "librccl.so lacks a required symbol"; return false; }
        return true;
    }
};
Rccl g_rccl;
constexpr int kNcclFloat = 7;                        // ncclFloat32, rccl.h:466

// Sample-split until the launch has ~25 rounds of 32 waves per CU: shorter wavefronts balance the tail of a launch (tiles
// differ in path length).  Measured on the 1080p x 1024 spp Cornell box (tests/gpu_shard_probe.py): whole frame 328 -> 315 ms
// with 4 lanes per pixel, one shard of 8 GPUs 47.1 -> 42.4 ms with 16; round 3, persistent 256-thread workgroups: 1 / 2 / 4 / 8
// lanes per pixel 292.9 / 274.7 / 267.7 / 265.7 ms, hence 8 at 1080p (the target was 120 000 wavefronts: 4).
constexpr unsigned long long kSplitTargetWaves = 200000ull;
// A sample-split launch writes one f32x3 chunk sum per pixel per 16 samples; the buffer is bounded by cutting one
// mrt_execute into several launches of at most this many sample chunks (1024 samples) and this many bytes.  Launch
// boundaries are chunk boundaries, so the canonical accumulation order -- and every bit -- is unchanged.
constexpr u32 kMaxChunksPerLaunch = 64u;
constexpr size_t kPartialBudgetBytes = (size_t)4u << 30;

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) for every instantiation: once per device, not per mrt_create.  A device counts
// as configured only after a SUCCESSFUL pass, so a transient failure is retried by the next mrt_create instead of being
// returned for the rest of the process; the table grows with the device index.
std::mutex g_cfg_mu;
std::vector<char> g_cfg_done;
hipError_t configure_pt_once(int device)      // the caller has made `device` current
{
    if (device < 0) return configure_pt(kLdsLimit);
    std::lock_guard<std::mutex> lock(g_cfg_mu);
    if ((size_t)device < g_cfg_done.size() && g_cfg_done[device]) return hipSuccess;
    const hipError_t e = configure_pt(kLdsLimit);
    if (e != hipSuccess) return e;
    if ((size_t)device >= g_cfg_done.size()) g_cfg_done.resize((size_t)device + 1, 0);
    g_cfg_done[device] = 1;
    return hipSuccess;
}

// ---- per-feature state: built whole on first use (a group's by mrt_create), held by the context through a unique_ptr ----

// look-ahead of the eager per-call path: two sets of per-sample planes [n][padded_rows][nw][3], set i: samples [base[i], + n[i])
struct Lookahead {
    Stream stream;                                // the look-ahead launches; the folds run on the context's stream
    Event ev0[2], ev1[2];                         // around set i's trace launch, on `stream`
    DeviceMem<u32> counter;                       // tile counter of persistent look-ahead launches (the eager launches keep their own)
    DeviceMem<float> planes[2];
    u32 base[2] = {0, 0}, n[2] = {0, 0};
};
// adaptive sampling (mrt_execute_adaptive)
struct Adaptive {
    DeviceMem<float> half;                        // H: [padded_rows][nw][3], per pixel the sum of its even-numbered rounds
    DeviceMem<u32> tiles;                         // [n_tiles] x 5 + 1: two tile lists, keep flags, per-tile count, per-tile converged flag, list length
    u32 n_tiles = 0;
    std::vector<u32> tile_count;                  // per-tile counts of the last adaptive call (host copy)
    u32 *counts() const { return tiles.p + 3u * (size_t)n_tiles; }      // ... on the device, where the tone map and the denoiser read them
};
// the image path (mrt_img, mrt_img_ss, mrt_img_denoised); Lanczos3 to the output resolution when it differs: the taps of both
// passes (vl ... hcap), the vertical pass's output (tmp), the image (out)
struct Image {
    DeviceMem<unsigned char> ss;                  // the tone-mapped supersampled frame [nh][nw][3]
    DeviceMem<u32> vl, vc, hl, hc;
    DeviceMem<float> vw, hw, tmp;
    DeviceMem<unsigned char> out;
    u32 vcap = 0, hcap = 0;
};
// first-hit AOVs and the denoiser (mrt_aov, mrt_denoise: DESIGN.md §13), on the context's device; the AOVs depend on scene and
// camera only and survive mrt_reset
struct Aov {
    DeviceMem<float> guide;                       // [2][nh][nw] float4: (normal, depth), (world point, hit flag)
    DeviceMem<float> albedo;                      // [nh][nw][3]
    DeviceMem<i32> ids;                           // [nh][nw][2]: renderer, flat instance index
    DeviceMem<unsigned long long> seg;            // the AOV kernel's diagnostic counters (mrt_trace.h count_fallback)
    DeviceMem<u32> blob;                          // the scene the AOV kernel reads when the context's is not it (deep staging, multi-device contexts)
    Event ev[2];                                  // around the AOV pass, then around the filter
    std::vector<u32> inst_first;                  // flat index of each renderer's first instance (ids -> mrt_scene order)
    DeviceMem<float> dn;                          // two e planes ([nh][nw] float4) and the filtered means [nh][nw][3]: the first mrt_denoise
};
// in-process multi-device context (mrt_opts.n_devices > 1): one sharded sub-context per device, gathered on device 0
struct Group {
    std::vector<std::unique_ptr<mrt_ctx>> subs;
    std::vector<ncclComm_t> comms;
    DeviceMem<float> gather;                      // [n_devices][padded_rows][nw][3] on device 0
    DeviceMem<u32> rowmap;                        // [n_devices][padded_rows] frame row of each gathered row (0xffffffff: padding)
    void release();                               // the sub-contexts, then the comms
    ~Group();
};

}  // namespace

struct mrt_ctx {
    int device = 0;
    Stream stream;                                // declared first: destroyed last
    Event ev0, ev1;                               // img timing; on a group context: around scatter_rows
    Event ev_g0, ev_g1;                           // sub-context of a group: around this rank's part of the ncclGather, on its stream
    std::vector<Event> evs;                       // 3 per launch of the last execute: start, after pt_megakernel, after reduce_chunks
    u32 ev_used = 0;
    bool stats_pending = false;                   // event times / segment counter of the last execute not read back yet
    bool count_segments = false;                  // MRT_FLAG_COUNT_SEGMENTS
    bool event_timing = true;                     // !MRT_FLAG_NO_EVENT_TIMING
    bool defer = false;                           // MRT_FLAG_DEFER / MRT_DEFER=1
    bool handed_out = false;                      // mrt_accum_device_ptr gave the raw device pointer away: sticky, the caller may read it at any time
    bool bound = false;                           // the accumulator lives in caller memory (a successful mrt_bind_accum)
    bool exposed() const { return handed_out || bound; }   // either way the memory is visible behind the library's back: no deferral
    Knobs knobs;                                  // the environment as mrt_create found it (a thread-per-connection server calls
                                                  // mrt_execute per sample: that path reads no environment)
    u32 pending = 0;                              // samples requested by deferred mrt_execute calls and not traced yet
    // look-ahead of the eager per-call path (the reference's callers run one Sampler::execute per sample): see run_lookahead
    bool la_enabled = false;                      // eager single-device context without MRT_FLAG_NO_LOOKAHEAD / MRT_LOOKAHEAD=0
    u32 la_max = 32;                              // samples per look-ahead launch at most (MRT_LOOKAHEAD=n)
    u32 la_streak = 0;                            // consecutive one-sample calls so far
    std::unique_ptr<Lookahead> la;
    Packed pk;
    std::unique_ptr<Packed> aov_pk;               // deep-staged contexts: the scene as packed without them (binary triangle BVHs) for the AOV kernel
    Params P;
    DeviceMem<u32> blob;                          // the packed scene (none on a group context: it lives on the sub-contexts)
    float *d_accum = nullptr;                     // [padded_rows][nw][3], rows past local_rows stay zero: accum_own or caller memory
    DeviceMem<float> accum_own;
    DeviceMem<float> partial;                     // chunk sums of a sample-split launch
    u32 padded_rows = 0;
    DeviceMem<unsigned long long> segments;       // segment counter + tile counter + 4 phase clocks (debug builds)
    u32 count = 0;                                // Sampler.last_count
    uint64_t seed = 0;
    u32 shard_index = 0, shard_count = 1, shard_rows = 8, local_rows = 0;
    std::vector<u32> row_of;                      // local row -> frame row
    DeviceMem<float> full;                        // [nh][nw][3]: a group's frame, or the full frame a sharded context received
    u32 full_count = 0;
    Plan plan;                                    // staging level, launch shape, kernel instantiation (mrt_plan.h): fixed by mrt_create
    u32 persist_grid = 0;                         // persistent grid of the batched shape
    mrt_stats stats;
    std::unique_ptr<Group> group;
    bool adaptive = false;                        // the accumulator holds an adaptive render: per-tile counts, count = the smallest
    std::unique_ptr<Adaptive> ad;
    std::unique_ptr<Image> img;
    bool aov_ready = false;                       // the AOVs have been computed
    std::unique_ptr<Aov> aov;
    // The sub-contexts and the RCCL comms go first; then this context's own resources on its device -- the look-ahead planes
    // only after the launches that write them have ended -- and its stream last (members are destroyed in reverse order).
    ~mrt_ctx()
    {
        if (group) group->release();
        if (!stream) return;                      // nothing was created on the device
        (void)hipSetDevice(device);
        if (la) (void)hipStreamSynchronize(la->stream.get());
    }
};

namespace {

void Group::release()
{
    subs.clear();
    for (ncclComm_t cm : comms) if (cm) g_rccl.CommDestroy(cm);
    comms.clear();
}
Group::~Group() { release(); }

// floats of one [padded_rows][nw][3] plane: the accumulator, H, a chunk plane, a look-ahead plane
size_t plane_floats(const mrt_ctx *c) { return (size_t)c->padded_rows * c->pk.nw * 3; }

int set_device(const mrt_ctx *c)
{
    HIP_TRY(hipSetDevice(c->device));
    return MRT_OK;
}

// The frame an observation reads and its sample count: the full frame of a group, or of a sharded context that received one,
// else the accumulator -- rgb is null when that holds only the context's own rows.
struct Frame { const float *rgb; u32 count; };
Frame frame_of(const mrt_ctx *c)
{
    if (c->full.p) return {c->full.p, c->full_count};
    return {c->shard_count == 1 ? c->d_accum : nullptr, c->count};
}
// ... for an observation of the whole frame's means (the image, the denoiser), refused without the whole frame or a sample
int whole_frame(const mrt_ctx *c, const char *fn, const char *empty_note, Frame &f)
{
    f = frame_of(c);
    if (!f.rgb) return fail(MRT_ERR_STATE, "%s: this context holds only its own rows; gather and mrt_set_accum first", fn);
    if (f.count == 0) return fail(MRT_ERR_STATE, "%s: no samples accumulated%s", fn, empty_note);
    return MRT_OK;
}

}  // namespace

// error text / status setter for the other translation units of the library (mrt_image_io.cpp)
int mrt_internal_fail(int code, const char *msg) { return fail(code, "%s", msg); }
void mrt_internal_ok() { ok(); }

extern "C" {

uint32_t mrt_abi_version(void) { return MRT_ABI_VERSION; }
const char *mrt_last_error(void) { return g_err.c_str(); }
int mrt_last_status(void) { return g_status; }

int mrt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static mrt_ctx *create_single(const mrt_render_desc *desc, const mrt_opts *opts, const mrt_desc_ext *ext, const Knobs &knobs)
{
    const u32 shard_count = opts->shard_count ? opts->shard_count : 1;
    if (opts->shard_index >= shard_count) { fail(MRT_ERR_ARG, "mrt_create: shard_index %u >= shard_count %u", opts->shard_index, shard_count); return nullptr; }

    std::unique_ptr<mrt_ctx> c(new mrt_ctx());              // every failure below: the context is destroyed with what it holds
    std::string err;
    const int rc = pack_scene(desc, c->pk, err, PackOpts(), ext);
    if (rc != MRT_OK) { fail(rc, "mrt_create: %s", err.c_str()); return nullptr; }
    c->knobs = knobs;
    Plan &plan = c->plan;
    plan_launch(desc, ext, knobs, c->pk, plan);   // may re-pack the scene (deep staging: 4-wide triangle BVHs), before anything is uploaded
    if (c->pk.tbvh_wide) {                   // the AOV kernel (scene through L2, no F_DEEP build) walks the binary triangle BVHs
        c->aov_pk.reset(new Packed());
        if (pack_scene(desc, *c->aov_pk, err, PackOpts(), ext) != MRT_OK) { fail(MRT_ERR_SCENE, "mrt_create: %s", err.c_str()); return nullptr; }
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { fail(MRT_ERR_DEVICE, "mrt_create: no HIP device (this backend has no CPU path)"); return nullptr; }
    int dev = opts->device;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    if (dev >= ndev) { fail(MRT_ERR_ARG, "mrt_create: device %d of %d", dev, ndev); return nullptr; }
    c->device = dev;
    c->seed = opts->seed;
    c->shard_index = opts->shard_index; c->shard_count = shard_count;
    c->shard_rows = opts->shard_rows ? opts->shard_rows : 8;

    // rows of this shard: row block b (shard_rows rows) belongs to shard b % shard_count
    const u32 nh = c->pk.nh;
    for (u32 y = 0; y < nh; ++y) if ((y / c->shard_rows) % shard_count == c->shard_index) c->row_of.push_back(y);
    c->local_rows = (u32)c->row_of.size();

    auto bail = [&](int code, const char *what, hipError_t e) { fail(code, "mrt_create: %s: %s", what, hipGetErrorString(e)); return (mrt_ctx *)nullptr; };
    hipError_t e;
    if ((e = hipSetDevice(dev)) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipSetDevice", e);
    if ((e = create(c->stream)) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipStreamCreate", e);
    if ((e = create(c->ev0)) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipEventCreate", e);
    if ((e = create(c->ev1)) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipEventCreate", e);
    const size_t all_words = c->pk.blob.size();
    if ((e = c->blob.alloc(all_words ? all_words : 4)) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipMalloc(scene)", e);
    if ((e = hipMemcpy(c->blob.p, c->pk.blob.data(), all_words * 4, hipMemcpyHostToDevice)) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipMemcpy(scene)", e);
    {
        const u32 n_blocks = (nh + c->shard_rows - 1) / c->shard_rows;
        c->padded_rows = ((n_blocks + shard_count - 1) / shard_count) * c->shard_rows;
        if (shard_count == 1) c->padded_rows = nh;
    }
    if ((e = c->accum_own.alloc(plane_floats(c.get()))) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipMalloc(accumulator)", e);
    c->d_accum = c->accum_own.p;
    if ((e = hipMemset(c->d_accum, 0, plane_floats(c.get()) * sizeof(float))) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipMemset", e);
    if ((e = c->segments.alloc(8)) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipMalloc", e);
    if ((e = hipMemset(c->segments.p, 0, 8 * sizeof(unsigned long long))) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipMemset", e);

    c->pk.P.tiles_x = plan.tiles_x;
    c->pk.P.tiles_y = plan.tiles_y;
    if (plan.in_lds && (e = configure_pt_once(dev)) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipFuncSetAttribute", e);

    c->P = c->pk.P;
    c->P.local_rows = c->local_rows; c->P.shard_index = c->shard_index; c->P.shard_count = c->shard_count; c->P.shard_rows = c->shard_rows;
    c->P.seed_lo = (u32)c->seed; c->P.seed_hi = (u32)(c->seed >> 32);
    c->P.blob = c->blob.p; c->P.accum = c->d_accum; c->P.segments = c->segments.p;
    c->P.tile_counter = reinterpret_cast<u32 *>(c->segments.p + 1);
    {
        // persistent launches (workgroups of more than one wavefront): as many workgroups as fit the device at once; each
        // wavefront then draws 8x8 tiles from a counter, so no CU waits for the slowest wavefront of a workgroup
        int n_cu = 0;
        if (!hip_tolerated(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device)) || n_cu <= 0) n_cu = 256;
        const size_t lds = plan.lds_bytes;
        size_t per_cu = 32u / (plan.block_threads / 64u);
        if (lds && kLdsLimit / lds < per_cu) per_cu = kLdsLimit / lds;
        if (per_cu < 1u) per_cu = 1u;
        c->persist_grid = plan.block_threads > 64u && !knobs.no_persist ? (u32)(n_cu * per_cu) : 0u;
        c->P.persist_grid = c->persist_grid;
    }
    c->count_segments = (opts->flags & MRT_FLAG_COUNT_SEGMENTS) != 0;
    c->event_timing = (opts->flags & MRT_FLAG_NO_EVENT_TIMING) == 0;
    c->P.count_segments = c->count_segments ? 1u : 0u;
    memset(&c->stats, 0, sizeof c->stats);
    fill_stats(plan, c->stats);
    c->defer = (opts->flags & MRT_FLAG_DEFER) != 0 || (knobs.defer && opts->shard_count <= 1);
    // (MRT_FLAG_COUNT_SEGMENTS: every call runs its own launch, so that mrt_stats.segments counts that call's paths)
    c->la_enabled = !c->defer && !c->count_segments && (opts->flags & MRT_FLAG_NO_LOOKAHEAD) == 0;
    if (knobs.lookahead_off) c->la_enabled = false;
    if (knobs.lookahead_max) c->la_max = knobs.lookahead_max;
    {   // both plane sets together stay below 4 GiB (32 samples of a 1080p frame: 2 x 0.8 GB; a 4K frame gets 20 per launch)
        const size_t plane_bytes = plane_floats(c.get()) * sizeof(float);
        const size_t fit = plane_bytes ? ((size_t)2u << 30) / plane_bytes : 0;
        if (fit < 2) c->la_enabled = false; else if (fit < c->la_max) c->la_max = (u32)fit;
    }
    ok();
    return c.release();
}

// In-process multi-device context: n sharded sub-contexts (device r renders row blocks b = r mod n), one RCCL
// ncclGather of the padded shard accumulators to device 0 per mrt_execute, rows placed into the frame by scatter_rows.
static mrt_ctx *create_group(const mrt_render_desc *desc, const mrt_opts *opts, const mrt_desc_ext *ext, u32 n, const Knobs &knobs)
{
    std::string err;
    if (!g_rccl.load(err)) { fail(MRT_ERR_DEVICE, "mrt_create: %s", err.c_str()); return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || (u32)ndev < n) { fail(MRT_ERR_DEVICE, "mrt_create: n_devices = %u but %d HIP device(s) are visible", n, ndev); return nullptr; }
    std::unique_ptr<mrt_ctx> g(new mrt_ctx());              // every failure below: the context is destroyed with what it holds
    const int rc = pack_scene(desc, g->pk, err, PackOpts(), ext);
    if (rc != MRT_OK) { fail(rc, "mrt_create: %s", err.c_str()); return nullptr; }
    g->device = 0; g->seed = opts->seed;
    g->knobs = knobs;
    g->defer = (opts->flags & MRT_FLAG_DEFER) != 0 || knobs.defer;
    g->shard_count = 1; g->shard_index = 0; g->shard_rows = opts->shard_rows ? opts->shard_rows : 8;
    g->local_rows = g->pk.nh; g->padded_rows = g->pk.nh;
    for (u32 y = 0; y < g->pk.nh; ++y) g->row_of.push_back(y);
    g->group.reset(new Group());
    Group &gr = *g->group;
    for (u32 r = 0; r < n; ++r) {
        mrt_opts o = *opts;
        o.n_devices = 0; o.device = (int)r; o.shard_index = r; o.shard_count = n; o.shard_rows = g->shard_rows;
        o.flags &= ~MRT_FLAG_DEFER;                   // the group defers, not its shards
        gr.subs.emplace_back(create_single(desc, &o, ext, knobs));
        if (!gr.subs.back()) return nullptr;
    }
    auto bail = [&](const char *what, const char *why) { fail(MRT_ERR_DEVICE, "mrt_create: %s: %s", what, why); return (mrt_ctx *)nullptr; };
    hipError_t e;
    if ((e = hipSetDevice(0)) != hipSuccess) return bail("hipSetDevice", hipGetErrorString(e));
    if ((e = create(g->stream)) != hipSuccess) return bail("hipStreamCreate", hipGetErrorString(e));
    if ((e = create(g->ev0)) != hipSuccess || (e = create(g->ev1)) != hipSuccess) return bail("hipEventCreate", hipGetErrorString(e));
    const u32 pr = gr.subs[0]->padded_rows, nw = g->pk.nw, nh = g->pk.nh;
    const size_t plane = plane_floats(gr.subs[0].get());
    if ((e = g->full.alloc((size_t)nh * nw * 3)) != hipSuccess) return bail("hipMalloc(frame)", hipGetErrorString(e));
    if ((e = hipMemset(g->full.p, 0, (size_t)nh * nw * 3 * sizeof(float))) != hipSuccess) return bail("hipMemset", hipGetErrorString(e));
    if ((e = gr.gather.alloc(plane * n)) != hipSuccess) return bail("hipMalloc(gather)", hipGetErrorString(e));
    std::vector<u32> rowmap((size_t)n * pr, 0xffffffffu);
    for (u32 r = 0; r < n; ++r) for (u32 i = 0; i < gr.subs[r]->local_rows; ++i) rowmap[(size_t)r * pr + i] = gr.subs[r]->row_of[i];
    if ((e = gr.rowmap.alloc(rowmap.size())) != hipSuccess) return bail("hipMalloc(rowmap)", hipGetErrorString(e));
    if ((e = hipMemcpy(gr.rowmap.p, rowmap.data(), rowmap.size() * sizeof(u32), hipMemcpyHostToDevice)) != hipSuccess) return bail("hipMemcpy(rowmap)", hipGetErrorString(e));
    std::vector<int> devs(n);
    for (u32 r = 0; r < n; ++r) devs[r] = (int)r;
    gr.comms.assign(n, nullptr);
    const int nrc = g_rccl.CommInitAll(gr.comms.data(), (int)n, devs.data());
    if (nrc != 0) return bail("ncclCommInitAll", g_rccl.GetErrorString(nrc));
    g->P = g->pk.P;
    memset(&g->stats, 0, sizeof g->stats);
    fill_stats(gr.subs[0]->plan, g->stats);
    ok();
    return g.release();
}

mrt_ctx *mrt_create(const mrt_render_desc *desc, const mrt_opts *opts) { return mrt_create_ext(desc, opts, nullptr); }

mrt_ctx *mrt_create_ext(const mrt_render_desc *desc, const mrt_opts *opts, const mrt_desc_ext *ext)
{
    g_err.clear();
    if (!desc || !opts) { fail(MRT_ERR_ARG, "mrt_create: null argument"); return nullptr; }
    if (opts->abi_version != MRT_ABI_VERSION) { fail(MRT_ERR_ARG, "mrt_create: ABI version %u, library has %u", opts->abi_version, MRT_ABI_VERSION); return nullptr; }
    const Knobs knobs = Knobs::from_env();
    const u32 n = opts->n_devices ? opts->n_devices : knobs.gpus;               // MRT_GPUS: the Rust shim's knob
    if (n > 1 || (n == 1 && knobs.force_rccl)) {                                 // MRT_FORCE_RCCL (tests): the group path on one device
        if (opts->shard_count > 1) { fail(MRT_ERR_ARG, "mrt_create: n_devices and shard_count are mutually exclusive"); return nullptr; }
        return create_group(desc, opts, ext, n, knobs);
    }
    return create_single(desc, opts, ext, knobs);
}

void mrt_destroy(mrt_ctx *ctx) { delete ctx; }

// Lazy half of the per-execute statistics: HIP-event times and (MRT_FLAG_COUNT_SEGMENTS) the segment counter are read
// back when somebody asks (mrt_get_stats), not on every mrt_execute -- the reference's callers run one pass per call
// (src/cli.rs:162-170), so the per-call cost is what the drop-in binary pays 1024 times per frame.
static int resolve_stats(mrt_ctx *c)
{
    if (!c->stats_pending) return MRT_OK;
    c->stats_pending = false;
    int rc = set_device(c);
    if (rc) return rc;
    double k = 0, r = 0;
    for (u32 i = 0; i + 2u < c->ev_used; i += 3u) {
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, c->evs[i].get(), c->evs[i + 1].get()));
        HIP_TRY(hipEventElapsedTime(&b, c->evs[i + 1].get(), c->evs[i + 2].get()));
        k += a; r += b;
    }
    c->stats.kernel_ms = k;
    c->stats.reduce_ms = c->stats.k_split > 1u ? r : 0.0;
    if (c->count_segments) {
        unsigned long long seg = 0;
        HIP_TRY(hipMemcpy(&seg, c->segments.p, sizeof seg, hipMemcpyDeviceToHost));
        c->stats.segments = seg;
    }
    if (c->knobs.debug_fallbacks) {
        unsigned long long t[3] = {0, 0, 0};
        HIP_TRY(hipMemcpy(t, c->segments.p + 5, sizeof t, hipMemcpyDeviceToHost));
        fprintf(stderr, "[mrt fallbacks] since mrt_create: NaN directions (shortcut) %llu, walk area full %llu, rays the triangle BVH may not cull %llu\n", t[0], t[1], t[2]);
    }
#ifdef MRT_PHASE_TIMING
    {   // debug build: shader-clock ticks per phase, summed over wavefronts since the context was created
        unsigned long long t[4] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpy(t, c->segments.p + 2, sizeof t, hipMemcpyDeviceToHost));
        const double tot = (double)(t[0] + t[1] + t[2] + t[3]);
        fprintf(stderr, "[mrt phase ticks] closest-hit query %.3f  shading %.3f  shadow query %.3f  ray set-up / regeneration %.3f  (total %.4g wave-ticks)\n",
                t[0] / tot, t[1] / tot, t[2] / tot, t[3] / tot, tot);
    }
#endif
    return MRT_OK;
}

// Lanes per pixel (k_split) and sample chunks per launch (cap) of a batch of n_chunks chunks over wave_tiles 8x8 tiles;
// (re)allocates the chunk planes the split needs.  planes: the batch must go through the chunk planes (k_split >= 2 even for
// a single chunk: the adaptive even rounds, whose chunk sums are added to the half buffer too) -- MRT_ERR_LIMIT without them.
static int split_policy(mrt_ctx *c, unsigned long long wave_tiles, u32 n_chunks, bool planes, u32 &k_split, u32 &cap)
{
    k_split = 1;
    // (a frame of 100 000 wave tiles or more -- 4K -- has its 25 rounds without splitting: CornellBox2 at 3840x2160 loses 1.6 %
    // to a second lane per pixel, 985 -> 1001 ms)
    const unsigned long long split_target = wave_tiles >= 100000ull ? 0ull : kSplitTargetWaves;
    while (k_split * 2u <= n_chunks && k_split < 16u && wave_tiles * k_split < split_target) k_split *= 2u;
    if (c->knobs.k_split) { k_split = c->knobs.k_split; while (k_split > n_chunks) k_split /= 2u; }
    if (planes && k_split < 2u) k_split = 2u;
    const size_t plane = plane_floats(c);
    cap = kMaxChunksPerLaunch;                           // chunks per launch
    if (c->knobs.max_chunks) cap = c->knobs.max_chunks;
    size_t budget = kPartialBudgetBytes;
    if (c->knobs.partial_budget) budget = c->knobs.partial_budget;
    if (k_split > 1u) {
        if (cap < k_split) cap = k_split;
        while (cap > k_split && plane * cap * sizeof(float) > budget) cap /= 2u;
        const size_t need = plane * (n_chunks < cap ? n_chunks : cap);
        if (need * sizeof(float) > budget) k_split = 1u;                       // not even k_split planes fit: one lane per pixel
        else if (need > c->partial.n && !hip_tolerated(c->partial.alloc(need, c->knobs.partial_fail_alloc ? (size_t)1 << 60 : 0))) k_split = 1u;
    }
    if (planes && k_split < 2u) return fail(MRT_ERR_LIMIT, "mrt_execute_adaptive: no memory for the chunk planes of a round");
    return MRT_OK;
}

// One trace launch of P on `stream`: the tile counter P draws from is reset first when the launch is persistent (before ev0, so
// the kernel time leaves the reset out), then ev0, launch_pt, ev1 (null events are not recorded).  tl: a tile-list launch.
static int launch_trace(mrt_ctx *c, const Params &P, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const TileList *tl)
{
    if (c->plan.block_threads > 64u && P.persist_grid) HIP_TRY(hipMemsetAsync(P.tile_counter, 0, sizeof(u32), stream));
    if (ev0) HIP_TRY(hipEventRecord(ev0, stream));
    HIP_TRY(launch_pt(P, c->plan.block_threads, c->plan.in_lds, c->pk.features, stream, tl));
    if (ev1) HIP_TRY(hipEventRecord(ev1, stream));
    return MRT_OK;
}

// Samples [base, base + n) of the whole frame (tl null) or of the listed tiles, asynchronous on c->stream: the sample split
// (split_policy, sized from the tiles traced), cut into chunk-aligned launches, each followed by the fold of its chunk sums into
// the accumulator -- and into `half` too when it is not null (listed tiles only).  planes: every launch goes through the chunk
// planes.  k_split receives split_policy's lanes per pixel; ks_max is raised to the largest split of any launch.
static int launch_batch(mrt_ctx *c, u32 base, u32 n, const TileList *tl, float *half, bool planes, u32 &k_split, u32 &ks_max)
{
    const u32 n_chunks = (base + n - 1u) / kChunk - base / kChunk + 1u;
    // sample split: spread a small frame over more wavefronts, one lane per (pixel, every k-th sample chunk)
    const unsigned long long wave_tiles = tl ? tl->n : (unsigned long long)((c->pk.nw + 7) / 8) * ((c->local_rows + 7) / 8);
    u32 cap = kMaxChunksPerLaunch;
    int rc = split_policy(c, wave_tiles, n_chunks, planes, k_split, cap);
    if (rc) return rc;
    const size_t plane = plane_floats(c);
    c->P.partial = c->partial.p;
    c->P.partial_stride = plane;
    const u32 s_end = base + n;
    while (base < s_end) {
        // this launch: samples [base, stop), stop on a chunk boundary (or the end); k_split == 1 needs no buffer: one launch
        u32 stop = s_end;
        if (k_split > 1u) {
            const unsigned long long lim = ((unsigned long long)(base / kChunk) + cap) * kChunk;
            if (lim < stop) stop = (u32)lim;
        }
        const u32 nc = (stop - 1u) / kChunk - base / kChunk + 1u;
        u32 ks = k_split;
        while (ks > nc) ks /= 2u;
        if (planes && ks < 2u) ks = 2u;                  // (a lane of chunk phase >= nc has nothing to do)
        c->P.n_samples = stop - base;
        c->P.sample_base = base;
        c->P.k_split = ks;
        if (ks > ks_max) ks_max = ks;
        while (c->event_timing && c->evs.size() < (size_t)c->ev_used + 3u) { Event e; HIP_TRY(create(e)); c->evs.push_back(std::move(e)); }
        const Event *ev = c->event_timing ? &c->evs[c->ev_used] : nullptr;
        c->P.persist_grid = (c->plan.small_plain_grid && stop - base < kChunk) ? 0u : c->persist_grid;
        if ((rc = launch_trace(c, c->P, c->stream.get(), ev ? ev[0].get() : nullptr, ev ? ev[1].get() : nullptr, tl))) return rc;
        if (ks > 1u) {
            if (tl) HIP_TRY(launch_reduce_chunks_listed(c->d_accum, half, c->partial.p, tl->tiles, tl->n, c->pk.nw, c->pk.nh, plane, nc, c->stream.get()));
            else HIP_TRY(launch_reduce_chunks(c->d_accum, c->partial.p, (size_t)c->local_rows * c->pk.nw * 3, plane, nc, c->stream.get()));
        }
        if (ev) { HIP_TRY(hipEventRecord(ev[2].get(), c->stream.get())); c->ev_used += 3u; }
        c->stats.launches += 1u;
        base = stop;
    }
    return MRT_OK;
}

// the statistics of one execute start over (an adaptive call's, and a look-ahead call's, as well)
static void reset_exec_stats(mrt_ctx *c)
{
    c->stats.kernel_ms = 0; c->stats.reduce_ms = 0; c->stats.gather_ms = 0; c->stats.launches = 0; c->stats.samples = 0; c->stats.segments = 0;
    c->stats_pending = false; c->ev_used = 0;
}

// asynchronous half of mrt_execute on one device: everything up to the closing event
static int exec_launch(mrt_ctx *c, uint32_t n_samples)
{
    int rc = set_device(c);
    if (rc) return rc;
    reset_exec_stats(c);
    if (!(n_samples && c->local_rows)) return MRT_OK;
    if (c->count_segments) HIP_TRY(hipMemsetAsync(c->segments.p, 0, sizeof(unsigned long long), c->stream.get()));
    u32 ks_max = 0;                                  // (the uniform path reports the policy's k_split)
    if ((rc = launch_batch(c, c->count, n_samples, nullptr, nullptr, false, c->stats.k_split, ks_max))) return rc;
    return MRT_OK;
}

static int exec_finish(mrt_ctx *c, uint32_t n_samples)
{
    int rc = set_device(c);
    if (rc) return rc;
    if (n_samples && c->local_rows) {
        HIP_TRY(hipStreamSynchronize(c->stream.get()));
        c->stats.samples = (uint64_t)c->local_rows * c->pk.nw * n_samples;
        c->stats_pending = true;
    }
    c->count += n_samples;                                        // src/sampler.rs:76
    return MRT_OK;
}

static int exec_group(mrt_ctx *g, uint32_t n_samples)
{
    Group &gr = *g->group;
    const u32 n = (u32)gr.subs.size();
    int rc = MRT_OK;
    u32 launched = 0;
    for (; launched < n; ++launched) if ((rc = exec_launch(gr.subs[launched].get(), n_samples))) break;
    // an error from here on still waits for everything that was launched, so no kernel is left running on a buffer
    // the caller may free; the first error is the one reported
    auto drain = [&](u32 upto) { for (u32 r = 0; r < upto; ++r) { if (hipSetDevice(gr.subs[r]->device) == hipSuccess) (void)hipStreamSynchronize(gr.subs[r]->stream.get()); } (void)hipGetLastError(); };
    if (rc) return keep_first_error(rc, [&] { drain(launched + (launched < n ? 1u : 0u)); });
    // one gather per batch: rank r sends its padded shard accumulator, device 0 receives rank i at offset i * plane.
    // gather_ms is device time, not host time around asynchronous launches: every sub-stream records an event after its
    // kernels (before its part of the gather) and one after it; the slowest stream's interval plus scatter_rows is the
    // exchange.  A rank whose kernels finish early waits inside the collective for the slowest one, so the figure is an
    // upper bound of the transfer itself; kernel_ms (the slowest rank's kernels) is reported next to it.
    const size_t plane = plane_floats(gr.subs[0].get());
    hipError_t he = hipSuccess;
    for (u32 r = 0; r < n && he == hipSuccess; ++r) {
        mrt_ctx *s = gr.subs[r].get();
        if ((he = hipSetDevice(s->device)) != hipSuccess) break;
        if (!s->ev_g0 && (he = create(s->ev_g0)) != hipSuccess) break;
        if (!s->ev_g1 && (he = create(s->ev_g1)) != hipSuccess) break;
        he = hipEventRecord(s->ev_g0.get(), s->stream.get());
    }
    int nrc = he == hipSuccess ? g_rccl.GroupStart() : 0;
    if (he == hipSuccess && nrc == 0) {
        for (u32 r = 0; r < n && nrc == 0 && he == hipSuccess; ++r) {
            if ((he = hipSetDevice(gr.subs[r]->device)) != hipSuccess) break;
            nrc = g_rccl.Gather(gr.subs[r]->d_accum, r == 0 ? gr.gather.p : nullptr, plane, kNcclFloat, 0, gr.comms[r], gr.subs[r]->stream.get());
        }
        const int nrc2 = g_rccl.GroupEnd();                         // always closed, whatever happened inside the group
        if (nrc == 0) nrc = nrc2;
    }
    for (u32 r = 0; r < n && he == hipSuccess && nrc == 0; ++r) {
        if ((he = hipSetDevice(gr.subs[r]->device)) != hipSuccess) break;
        he = hipEventRecord(gr.subs[r]->ev_g1.get(), gr.subs[r]->stream.get());
    }
    if (he != hipSuccess || nrc != 0) {
        drain(n);
        if (he != hipSuccess) return fail(MRT_ERR_DEVICE, "HIP call failed around the gather group: %s", hipGetErrorString(he));
        return fail(MRT_ERR_DEVICE, "ncclGather: %s", g_rccl.GetErrorString(nrc));
    }
    for (auto &s : gr.subs) if ((rc = exec_finish(s.get(), n_samples))) return keep_first_error(rc, [&] { drain(n); });    // syncs every stream (kernel + gather)
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(hipEventRecord(g->ev0.get(), g->stream.get()));
    HIP_TRY(launch_scatter_rows(g->full.p, gr.gather.p, gr.rowmap.p, n * gr.subs[0]->padded_rows, g->pk.nw * 3u, g->stream.get()));
    HIP_TRY(hipEventRecord(g->ev1.get(), g->stream.get()));
    HIP_TRY(hipStreamSynchronize(g->stream.get()));
    g->count += n_samples;
    g->full_count = g->count;
    memset(&g->stats, 0, offsetof(mrt_stats, lds_bytes));
    g->stats.reduce_ms = 0;
    double gather_ms = 0;
    for (const auto &s : gr.subs) {
        if ((rc = resolve_stats(s.get()))) return rc;
        if (s->stats.kernel_ms > g->stats.kernel_ms) g->stats.kernel_ms = s->stats.kernel_ms;
        if (s->stats.reduce_ms > g->stats.reduce_ms) g->stats.reduce_ms = s->stats.reduce_ms;
        g->stats.samples += s->stats.samples; g->stats.segments += s->stats.segments; g->stats.launches += s->stats.launches;
        float ms = 0;
        HIP_TRY(hipSetDevice(s->device));
        // a sub-context without rows of its own (a frame of fewer row blocks than devices) or a call with n_samples == 0
        // still joined the gather, but exec_finish did not synchronise its stream: wait for its closing event here, or
        // hipEventElapsedTime answers hipErrorNotReady after the counts have been advanced
        HIP_TRY(hipEventSynchronize(s->ev_g1.get()));
        HIP_TRY(hipEventElapsedTime(&ms, s->ev_g0.get(), s->ev_g1.get()));
        if (ms > gather_ms) gather_ms = ms;
    }
    HIP_TRY(hipSetDevice(g->device));
    { float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, g->ev0.get(), g->ev1.get())); gather_ms += ms; }      // + placing the rows into the frame
    g->stats.k_split = gr.subs[0]->stats.k_split;
    g->stats.gather_ms = gather_ms;
    return MRT_OK;
}

// ---- look-ahead of the eager per-call path -----------------------------------------------------------------------------------
// The reference's callers run ONE Sampler::execute per sample and wait for it (src/cli.rs:162-170, src/http.rs:141-144).  A
// one-sample launch cannot regenerate paths inside a lane (a wavefront lasts as long as its longest path: lane utilisation
// 0.65 against 0.70, 0.36 ms per 1080p pass against 0.25 inside a batched launch), and the image is a pure function of (scene,
// seed, sample index) -- so a context that sees one-sample calls arrive back to back traces AHEAD: samples [k, k + n) in one
// launch on a second stream, every sample into a plane of its own (Params.to_planes), and each call
// only folds its sample's plane into the accumulator (reduce_chunks, 0.02 ms) and waits for that.  The accumulator holds
// exactly the samples the caller has asked for at every return, added one by one in index order -- bit for bit what the plain
// per-call loop leaves there -- so observing it (mrt_accum, mrt_img, a bound or handed-out pointer) needs no special case.  Two
// plane sets: while one is folded call by call, the next launch already runs.  It starts at the third consecutive
// one-sample call with two samples per launch and doubles up to la_max (32), so a caller that stops early wastes at most about
// the work it has used; any other call (n != 1, reset, set_accum) drops what was traced ahead.
static void la_drop(mrt_ctx *c)
{
    if (c->la && (c->la->n[0] || c->la->n[1])) (void)hipStreamSynchronize(c->la->stream.get());
    if (c->la) c->la->n[0] = c->la->n[1] = 0;
    c->la_streak = 0;
}

// launch the trace of samples [base, base + n) into plane set i (asynchronous, on the look-ahead stream, created by the first call)
static int la_launch(mrt_ctx *c, int i, u32 base, u32 n)
{
    const size_t plane = plane_floats(c);
    if (!c->la) {
        std::unique_ptr<Lookahead> la(new Lookahead());
        HIP_TRY(create(la->stream));
        for (int k = 0; k < 2; ++k) { HIP_TRY(create(la->ev0[k])); HIP_TRY(create(la->ev1[k])); }
        HIP_TRY(la->counter.alloc(1));
        c->la = std::move(la);
    }
    Lookahead &la = *c->la;
    if (plane * n > la.planes[i].n && !hip_tolerated(la.planes[i].alloc(plane * n))) return MRT_ERR_LIMIT;     // the caller falls back
    Params P = c->P;
    P.n_samples = n; P.sample_base = base; P.k_split = 1u; P.to_planes = 1u;
    P.partial = la.planes[i].p; P.partial_stride = plane;
    P.count_segments = 0u;
    // small scenes: the plain grid (their persistent grid fills every wave slot of the chip and would keep the folds out until
    // the launch has ended); larger ones leave slots free and keep their persistent workgroups, with a tile counter of their own
    P.persist_grid = c->plan.small_plain_grid ? 0u : c->persist_grid;
    P.tile_counter = la.counter.p;
    const int rc = launch_trace(c, P, la.stream.get(), la.ev0[i].get(), la.ev1[i].get(), nullptr);
    if (rc) return rc;
    la.base[i] = base; la.n[i] = n;
    return MRT_OK;
}

// one eager one-sample call served from the look-ahead planes; returns MRT_ERR_LIMIT when the planes cannot be had (the caller
// then runs the plain launch from here on) and kLaPlain when the two sets would reach past sample index 0xffffffff (the caller
// runs the plain launch for this call only)
constexpr int kLaPlain = 1;
static int run_lookahead(mrt_ctx *c)
{
    int rc = set_device(c);
    if (rc) return rc;
    const u32 k = c->count;
    int s = -1;
    if (c->la) for (int i = 0; i < 2; ++i) if (c->la->n[i] && k >= c->la->base[i] && k < c->la->base[i] + c->la->n[i]) s = i;
    if (s < 0) {
        // nothing traced ahead for this sample (first use, or what was ahead has been dropped): start both sets
        la_drop(c);
        c->la_streak = 2;
        const u32 n0 = 2u < c->la_max ? 2u : c->la_max;
        const u32 n1 = 2u * n0 < c->la_max ? 2u * n0 : c->la_max;
        if ((unsigned long long)k + n0 + n1 > 0xffffffffull) return kLaPlain;      // (a set's base + n must not wrap)
        if ((rc = la_launch(c, 0, k, n0))) return rc;
        if ((rc = la_launch(c, 1, k + n0, n1))) { (void)hipStreamSynchronize(c->la->stream.get()); c->la->n[0] = c->la->n[1] = 0; return rc; }
        s = 0;
    }
    Lookahead &la = *c->la;
    const size_t plane = plane_floats(c);
    const size_t words = (size_t)c->local_rows * c->pk.nw * 3;
    HIP_TRY(hipStreamWaitEvent(c->stream.get(), la.ev1[s].get(), 0));
    HIP_TRY(launch_reduce_chunks(c->d_accum, la.planes[s].p + (size_t)(k - la.base[s]) * plane, words, plane, 1u, c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));                // the fold has run, so the set's launch has ended too
    c->count += 1u;
    reset_exec_stats(c);
    c->stats.launches = 1u; c->stats.k_split = 1u;
    c->stats.samples = (uint64_t)c->local_rows * c->pk.nw;
    if (c->event_timing) {
        float ms = 0;
        if (hip_tolerated(hipEventElapsedTime(&ms, la.ev0[s].get(), la.ev1[s].get()))) c->stats.kernel_ms = (double)ms / (double)la.n[s];   // this sample's share of its launch
    }
    if (k + 1u == la.base[s] + la.n[s]) {
        // the set is spent (its last plane has been folded): the next launch goes into it, behind the other set's, twice as long
        const int o = 1 - s;
        const unsigned long long nb = (unsigned long long)la.base[o] + la.n[o];
        const u32 nn = 2u * la.n[o] < c->la_max ? 2u * la.n[o] : c->la_max;
        la.n[s] = 0;
        if (la.n[o] && nb + nn <= 0xffffffffull) (void)la_launch(c, s, (u32)nb, nn);      // (a failure here only means a later call starts over)
    }
    return MRT_OK;
}

static int run_samples(mrt_ctx *c, uint32_t n_samples)
{
    int rc;
    if (c->group) return exec_group(c, n_samples);
    if (c->la_enabled && n_samples == 1u && c->local_rows) {
        if (c->la_streak >= 2u) {
            rc = run_lookahead(c);
            if (rc == MRT_ERR_LIMIT) c->la_enabled = false;      // no memory for the planes: the plain per-call launch from here on
            else if (rc != kLaPlain) return rc;                  // (kLaPlain: this call only, at the top of the sample range)
        } else {
            ++c->la_streak;
        }
    } else {
        la_drop(c);
    }
    if ((rc = exec_launch(c, n_samples))) return rc;
    return exec_finish(c, n_samples);
}

// Deferred execution (MRT_FLAG_DEFER): trace what earlier mrt_execute calls only booked.  Called by every entry point that
// observes or replaces the accumulator; the result is the same set of samples as if each call had run at once.
static int settle(mrt_ctx *c)
{
    if (!c->pending) return MRT_OK;
    const u32 n = c->pending;
    c->pending = 0;
    return run_samples(c, n);
}
constexpr u32 kDeferLimit = 1024u;        // booked samples that trigger a launch by themselves (one full-size batch)

// the prologue of the entry points that observe or replace the accumulator: the context's device, then what was booked
static int enter(mrt_ctx *c)
{
    const int rc = set_device(c);
    return rc ? rc : settle(c);
}

int mrt_execute(mrt_ctx *c, uint32_t n_samples, double *seconds)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_execute: null context");
    if (c->adaptive) return fail(MRT_ERR_STATE, "mrt_execute: the context holds an adaptive render (per-tile sample counts): mrt_reset first");
    if ((unsigned long long)c->count + c->pending + n_samples > 0xffffffffull) return fail(MRT_ERR_LIMIT, "mrt_execute: sample count overflows u32");
    const auto t0 = std::chrono::steady_clock::now();
    int rc = MRT_OK;
    const bool deferred = c->defer && !c->exposed();
    if (deferred) {
        c->pending += n_samples;
        if (c->pending >= kDeferLimit) rc = settle(c);
    } else {
        rc = run_samples(c, n_samples);
    }
    if (rc) return rc;
    c->stats.deferred = deferred ? 1u : 0u;       // whether THIS call was booked (MRT_FLAG_DEFER honoured) or ran at once
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ok();
    return MRT_OK;
}

// ---- adaptive sampling ---------------------------------------------------------------------------------------------------------
static int adapt_run(mrt_ctx *c, const mrt_adapt *a, mrt_adapt_info *info)
{
    const u32 nw = c->pk.nw, nh = c->pk.nh, n_tx = (nw + 7u) / 8u, n_ty = (nh + 7u) / 8u, n_tiles = n_tx * n_ty;
    const size_t acc_floats = plane_floats(c);
    if (!c->ad) {
        std::unique_ptr<Adaptive> ad(new Adaptive());
        HIP_TRY(ad->half.alloc(acc_floats));
        HIP_TRY(ad->tiles.alloc(5u * (size_t)n_tiles + 1u));
        ad->n_tiles = n_tiles;
        c->ad = std::move(ad);
    }
    Adaptive &ad = *c->ad;
    u32 *lists[2] = {ad.tiles.p, ad.tiles.p + n_tiles};
    u32 *keep = ad.tiles.p + 2u * (size_t)n_tiles, *tcount = ad.counts(), *tconv = ad.tiles.p + 4u * (size_t)n_tiles;
    u32 *d_n = ad.tiles.p + 5u * (size_t)n_tiles;
    std::vector<u32> all(n_tiles);
    for (u32 t = 0; t < n_tiles; ++t) all[t] = t;
    HIP_TRY(hipMemcpy(lists[0], all.data(), n_tiles * sizeof(u32), hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(c->d_accum, 0, acc_floats * sizeof(float), c->stream.get()));
    HIP_TRY(hipMemsetAsync(ad.half.p, 0, acc_floats * sizeof(float), c->stream.get()));
    HIP_TRY(hipMemsetAsync(tcount, 0, 2u * (size_t)n_tiles * sizeof(u32), c->stream.get()));
    if (c->count_segments) HIP_TRY(hipMemsetAsync(c->segments.p, 0, sizeof(unsigned long long), c->stream.get()));
    u32 n_active = n_tiles, n = 0, rounds = 0, cur = 0;
    while (n_active) {
        for (int r = 0; r < 2; ++r, ++rounds, n += a->step) {
            // one round over the tiles still running; even rounds go through the chunk planes, whose sums are added, in chunk
            // order, to the accumulator and to the half buffer alike.  The adaptive path reports the largest split as k_split.
            const bool even = (rounds & 1u) == 0u;
            const TileList tl{lists[cur], n_active};
            u32 k_split = 1;
            const int rc = launch_batch(c, n, a->step, &tl, even ? ad.half.p : nullptr, even, k_split, c->stats.k_split);
            if (rc) return rc;
        }
        if (n < a->min_samples) continue;
        // the stop rule at count n for every tile still running; the next list, and its length (the one read-back of a step)
        HIP_TRY(launch_adapt_eval(c->d_accum, ad.half.p, lists[cur], n_active, nw, nh, n, a->threshold, n >= a->max_samples, keep, tcount, tconv,
                                  lists[cur ^ 1u], d_n, c->stream.get()));
        HIP_TRY(hipMemcpyAsync(&n_active, d_n, sizeof(u32), hipMemcpyDeviceToHost, c->stream.get()));
        HIP_TRY(hipStreamSynchronize(c->stream.get()));
        cur ^= 1u;
    }
    std::vector<u32> conv(n_tiles);
    ad.tile_count.assign(n_tiles, 0u);
    HIP_TRY(hipMemcpy(ad.tile_count.data(), tcount, n_tiles * sizeof(u32), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(conv.data(), tconv, n_tiles * sizeof(u32), hipMemcpyDeviceToHost));
    uint64_t samples = 0;
    u32 lo = 0xffffffffu, hi = 0, n_conv = 0;
    for (u32 t = 0; t < n_tiles; ++t) {
        const u32 ty = t / n_tx, tx = t - ty * n_tx;
        const u32 px = ((nw - tx * 8u) < 8u ? nw - tx * 8u : 8u) * ((nh - ty * 8u) < 8u ? nh - ty * 8u : 8u);
        const u32 k = ad.tile_count[t];
        samples += (uint64_t)k * px;
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
        n_conv += conv[t] ? 1u : 0u;
    }
    c->count = lo;
    c->adaptive = true;
    c->stats.samples = samples;
    c->stats_pending = true;
    if (info) {
        int rc = resolve_stats(c);
        if (rc) return rc;
        info->samples = samples;
        info->rounds = rounds;
        info->launches = c->stats.launches;
        info->tiles = n_tiles;
        info->tiles_converged = n_conv;
        info->min_count = lo;
        info->max_count = hi;
        info->kernel_ms = c->stats.kernel_ms;
    }
    return MRT_OK;
}

int mrt_execute_adaptive(mrt_ctx *c, const mrt_adapt *a, mrt_adapt_info *info, double *seconds)
{
    if (!c || !a) return fail(MRT_ERR_ARG, "mrt_execute_adaptive: null argument");
    const unsigned long long two = 2ull * a->step;
    if (a->step == 0u || a->step % kChunk) return fail(MRT_ERR_ARG, "mrt_execute_adaptive: step %u is not a positive multiple of %u", a->step, kChunk);
    if (a->min_samples == 0u || a->min_samples % two || a->max_samples == 0u || a->max_samples % two)
        return fail(MRT_ERR_ARG, "mrt_execute_adaptive: min_samples %u and max_samples %u must be positive multiples of 2 * step = %llu", a->min_samples, a->max_samples, two);
    if (a->min_samples > a->max_samples) return fail(MRT_ERR_ARG, "mrt_execute_adaptive: min_samples %u > max_samples %u", a->min_samples, a->max_samples);
    if (!(a->threshold >= 0.0f)) return fail(MRT_ERR_ARG, "mrt_execute_adaptive: threshold %g is not >= 0", (double)a->threshold);
    if (c->group || c->shard_count > 1u) return fail(MRT_ERR_STATE, "mrt_execute_adaptive: sharded and multi-device contexts are not supported");
    if (c->adaptive || c->count || c->pending || c->full.p)
        return fail(MRT_ERR_STATE, "mrt_execute_adaptive: the context holds samples (an adaptive render starts from none): mrt_reset first");
    const auto t0 = std::chrono::steady_clock::now();
    int rc = set_device(c);
    if (rc) return rc;
    la_drop(c);
    reset_exec_stats(c);
    c->stats.k_split = 1; c->stats.deferred = 0;
    if ((rc = adapt_run(c, a, info)))
        return keep_first_error(rc, [&] {            // nothing half done stays behind: the context is an empty uniform one again
            (void)hipStreamSynchronize(c->stream.get());
            (void)hipMemset(c->d_accum, 0, plane_floats(c) * sizeof(float));
            (void)hipGetLastError();
            c->adaptive = false; c->count = 0; c->stats_pending = false; c->ev_used = 0;
        });
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ok();
    return MRT_OK;
}

int mrt_sample_counts(mrt_ctx *c, uint32_t *counts)
{
    if (!c || !counts) return fail(MRT_ERR_ARG, "mrt_sample_counts: null argument");
    if (const int rc = enter(c)) return rc;
    const u32 nw = c->pk.nw, nh = c->pk.nh, n_tx = (nw + 7u) / 8u;
    const u32 uniform = frame_of(c).count;
    for (u32 y = 0; y < nh; ++y)
        for (u32 x = 0; x < nw; ++x) counts[(size_t)y * nw + x] = c->adaptive ? c->ad->tile_count[(y / 8u) * n_tx + x / 8u] : uniform;
    ok();
    return MRT_OK;
}

int mrt_adapt_half(mrt_ctx *c, float *rgb)
{
    if (!c || !rgb) return fail(MRT_ERR_ARG, "mrt_adapt_half: null argument");
    if (!c->adaptive) return fail(MRT_ERR_STATE, "mrt_adapt_half: no adaptive render on this context since its last reset");
    if (const int rc = set_device(c)) return rc;
    HIP_TRY(hipMemcpy(rgb, c->ad->half.p, (size_t)c->pk.nw * c->pk.nh * 3 * sizeof(float), hipMemcpyDeviceToHost));
    ok();
    return MRT_OK;
}

int mrt_dims(const mrt_ctx *c, uint32_t *nw, uint32_t *nh, uint32_t *local_rows)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_dims: null context");
    if (nw) *nw = c->pk.nw;
    if (nh) *nh = c->pk.nh;
    if (local_rows) *local_rows = c->local_rows;
    ok();
    return MRT_OK;
}

int mrt_accum_local(mrt_ctx *c, float *rgb, uint32_t *rows)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_accum_local: null context");
    if (const int rc = enter(c)) return rc;
    if (rows) memcpy(rows, c->row_of.data(), sizeof(u32) * c->local_rows);
    const float *src = c->group ? c->full.p : c->d_accum;         // a multi-device context owns every row
    if (rgb && c->local_rows) HIP_TRY(hipMemcpy(rgb, src, (size_t)c->local_rows * c->pk.nw * 3 * sizeof(float), hipMemcpyDeviceToHost));
    ok();
    return MRT_OK;
}

int mrt_accum(mrt_ctx *c, float *rgb, uint32_t *count)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_accum: null context");
    if (const int rc = enter(c)) return rc;
    const Frame f = frame_of(c);
    const size_t row_bytes = (size_t)c->pk.nw * 3 * sizeof(float);
    if (rgb && f.rgb) HIP_TRY(hipMemcpy(rgb, f.rgb, row_bytes * c->pk.nh, hipMemcpyDeviceToHost));
    else if (rgb) {                           // a shard's own rows, in their places
        std::vector<float> tmp((size_t)c->local_rows * c->pk.nw * 3);
        if (c->local_rows) HIP_TRY(hipMemcpy(tmp.data(), c->d_accum, row_bytes * c->local_rows, hipMemcpyDeviceToHost));
        for (u32 r = 0; r < c->local_rows; ++r) memcpy((char *)rgb + row_bytes * c->row_of[r], (char *)tmp.data() + row_bytes * r, row_bytes);
    }
    if (count) *count = f.count;
    ok();
    return MRT_OK;
}

int mrt_accum_device_ptr(mrt_ctx *c, void **dev_ptr, size_t *bytes)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_accum_device_ptr: null context");
    if (const int rc = enter(c)) return rc;
    c->handed_out = true;                     // from now on the caller may read the accumulator behind the library's back (sticky)
    if (dev_ptr) *dev_ptr = c->group ? c->full.p : c->d_accum;
    if (bytes) *bytes = plane_floats(c) * sizeof(float);
    ok();
    return MRT_OK;
}

int mrt_padded_rows(const mrt_ctx *c, uint32_t *rows)
{
    if (!c || !rows) return fail(MRT_ERR_ARG, "mrt_padded_rows: null argument");
    *rows = c->padded_rows;
    ok();
    return MRT_OK;
}

int mrt_bind_accum(mrt_ctx *c, void *dev_ptr, size_t bytes)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_bind_accum: null context");
    if (c->group) return fail(MRT_ERR_STATE, "mrt_bind_accum: not available on a multi-device context");
    if (const int rc = enter(c)) return rc;
    const size_t need = plane_floats(c) * sizeof(float);
    float *dst = dev_ptr ? (float *)dev_ptr : c->accum_own.p;
    if (dev_ptr && bytes < need) return fail(MRT_ERR_ARG, "mrt_bind_accum: buffer of %zu bytes, need %zu", bytes, need);     // nothing changed
    if (dst != c->d_accum) {
        HIP_TRY(hipMemcpy(dst, c->d_accum, need, hipMemcpyDeviceToDevice));
        c->d_accum = dst;
        c->P.accum = dst;
    }
    c->bound = dev_ptr != nullptr;            // only a bind that succeeded: the caller reads this memory whenever it likes, so every execute runs at once
    ok();
    return MRT_OK;
}

// mrt_set_accum / mrt_set_accum_device on a single-device context: the whole frame into the accumulator, or, on a sharded
// context, next to its own rows (only mrt_img and mrt_accum read it there)
static int set_frame(mrt_ctx *c, const void *rgb, hipMemcpyKind kind, uint32_t count)
{
    const size_t floats = (size_t)c->pk.nw * c->pk.nh * 3;
    if (c->shard_count == 1) {
        HIP_TRY(hipMemcpy(c->d_accum, rgb, floats * sizeof(float), kind));
        c->count = count;
    } else {
        if (!c->full.p) HIP_TRY(c->full.alloc(floats));
        HIP_TRY(hipMemcpy(c->full.p, rgb, floats * sizeof(float), kind));
        c->full_count = count;
    }
    ok();
    return MRT_OK;
}

int mrt_set_accum_device(mrt_ctx *c, const void *dev_rgb, uint32_t count)
{
    if (!c || !dev_rgb) return fail(MRT_ERR_ARG, "mrt_set_accum_device: null argument");
    if (const int rc = enter(c)) return rc;
    la_drop(c); c->adaptive = false;              // the sample count changes under what was traced ahead
    if (c->group) return fail(MRT_ERR_STATE, "mrt_set_accum_device: use mrt_set_accum on a multi-device context");
    return set_frame(c, dev_rgb, hipMemcpyDeviceToDevice, count);
}

int mrt_set_accum(mrt_ctx *c, const float *rgb, uint32_t count)
{
    if (!c || !rgb) return fail(MRT_ERR_ARG, "mrt_set_accum: null argument");
    if (const int rc = enter(c)) return rc;
    la_drop(c); c->adaptive = false;
    if (!c->group) return set_frame(c, rgb, hipMemcpyHostToDevice, count);
    const size_t row_bytes = (size_t)c->pk.nw * 3 * sizeof(float);
    HIP_TRY(hipMemcpy(c->full.p, rgb, row_bytes * c->pk.nh, hipMemcpyHostToDevice));
    for (auto &s : c->group->subs) {
        HIP_TRY(hipSetDevice(s->device));
        for (u32 i = 0; i < s->local_rows; ++i)
            HIP_TRY(hipMemcpy((char *)s->d_accum + row_bytes * i, (const char *)rgb + row_bytes * s->row_of[i], row_bytes, hipMemcpyHostToDevice));
        s->count = count;
    }
    c->count = count; c->full_count = count;
    ok();
    return MRT_OK;
}

int mrt_reset(mrt_ctx *c)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_reset: null context");
    c->pending = 0;                           // booked samples of a deferred context are dropped with everything else
    int rc = set_device(c);
    if (rc) return rc;
    la_drop(c); c->adaptive = false;
    if (c->group) {
        for (auto &s : c->group->subs) if ((rc = mrt_reset(s.get()))) return rc;
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipMemset(c->full.p, 0, (size_t)c->pk.nh * c->pk.nw * 3 * sizeof(float)));
    } else {
        HIP_TRY(hipMemset(c->d_accum, 0, plane_floats(c) * sizeof(float)));
        c->full.reset();
    }
    c->count = 0; c->full_count = 0;
    ok();
    return MRT_OK;
}

// The image buffers, created whole by the first call: a failure half-way leaves the context as it was, and the next call
// starts over
static int img_prepare(mrt_ctx *c)
{
    if (c->img) return MRT_OK;
    const u32 nw = c->pk.nw, nh = c->pk.nh, rw = c->pk.res_w, rh = c->pk.res_h;
    const bool resize = rw != nw || rh != nh;
    if (resize && (rw == 0 || rh == 0)) return fail(MRT_ERR_SCENE, "mrt_img: zero output resolution");
    std::unique_ptr<Image> im(new Image());
    const int rc = [&]() -> int {
        HIP_TRY(im->ss.alloc((size_t)nw * nh * 3));
        if (!resize) return MRT_OK;
        ResampleTaps v, h;
        lanczos3_taps(nh, rh, v);
        lanczos3_taps(nw, rw, h);
        HIP_TRY(im->vl.alloc(rh));
        HIP_TRY(im->vc.alloc(rh));
        HIP_TRY(im->vw.alloc((size_t)rh * v.cap));
        HIP_TRY(im->hl.alloc(rw));
        HIP_TRY(im->hc.alloc(rw));
        HIP_TRY(im->hw.alloc((size_t)rw * h.cap));
        HIP_TRY(hipMemcpy(im->vl.p, v.left.data(), sizeof(u32) * rh, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(im->vc.p, v.count.data(), sizeof(u32) * rh, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(im->vw.p, v.weight.data(), sizeof(float) * (size_t)rh * v.cap, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(im->hl.p, h.left.data(), sizeof(u32) * rw, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(im->hc.p, h.count.data(), sizeof(u32) * rw, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(im->hw.p, h.weight.data(), sizeof(float) * (size_t)rw * h.cap, hipMemcpyHostToDevice));
        HIP_TRY(im->tmp.alloc((size_t)nw * rh * 3));
        HIP_TRY(im->out.alloc((size_t)rw * rh * 3));
        im->vcap = v.cap; im->hcap = h.cap;
        return MRT_OK;
    }();
    if (rc) { im.reset(); (void)hipGetLastError(); return rc; }     // (what failed is not left pending for the next launch)
    c->img = std::move(im);
    return MRT_OK;
}

static int img_tonemap(mrt_ctx *c, const char *fn)
{
    Frame f;
    if (const int rc = whole_frame(c, fn, " (the reference would panic on an empty map, src/sampler.rs:85)", f)) return rc;
    const float wexp = (1.0f - c->pk.exp) * (1.0f - c->pk.exp);
    HIP_TRY(hipEventRecord(c->ev0.get(), c->stream.get()));
    if (c->adaptive)                          // each pixel with its tile's 1/count (tile counts of the last adaptive call)
        HIP_TRY(launch_tonemap_tiles(f.rgb, c->img->ss.p, c->ad->counts(), c->pk.nw, c->pk.nh, c->pk.gamma, wexp, c->stream.get()));
    else
        HIP_TRY(launch_tonemap(f.rgb, c->img->ss.p, c->pk.nw * c->pk.nh, 1.0f / (float)f.count, c->pk.gamma, wexp, c->stream.get()));
    return MRT_OK;
}

// The end of the image entry points: the tone-mapped frame, through Lanczos3 when `resize` asks for the output resolution and it
// differs (image 0.24 resize copies when the dimensions match); then close the timing of the image kernels, wait for them and
// copy the image out
static int img_finish(mrt_ctx *c, uint8_t *rgb8, bool resize)
{
    const u32 nw = c->pk.nw, nh = c->pk.nh, rw = c->pk.res_w, rh = c->pk.res_h;
    const Image &im = *c->img;
    const unsigned char *src = im.ss.p;
    size_t bytes = (size_t)nw * nh * 3;
    if (resize && (rw != nw || rh != nh)) {
        HIP_TRY(launch_lanczos_v(im.ss.p, im.tmp.p, nw, rh, im.vl.p, im.vc.p, im.vw.p, im.vcap, c->stream.get()));
        HIP_TRY(launch_lanczos_h(im.tmp.p, im.out.p, nw, rw, rh, im.hl.p, im.hc.p, im.hw.p, im.hcap, c->stream.get()));
        src = im.out.p;
        bytes = (size_t)rw * rh * 3;
    }
    HIP_TRY(hipEventRecord(c->ev1.get(), c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    { float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, c->ev0.get(), c->ev1.get())); c->stats.img_ms = ms; }
    HIP_TRY(hipMemcpy(rgb8, src, bytes, hipMemcpyDeviceToHost));
    ok();
    return MRT_OK;
}

int mrt_img_ss(mrt_ctx *c, uint8_t *rgb8)
{
    if (!c || !rgb8) return fail(MRT_ERR_ARG, "mrt_img_ss: null argument");
    int rc;
    if ((rc = enter(c)) || (rc = img_prepare(c)) || (rc = img_tonemap(c, "mrt_img_ss"))) return rc;
    return img_finish(c, rgb8, false);
}

int mrt_img(mrt_ctx *c, uint8_t *rgb8)
{
    if (!c || !rgb8) return fail(MRT_ERR_ARG, "mrt_img: null argument");
    int rc;
    if ((rc = enter(c)) || (rc = img_prepare(c)) || (rc = img_tonemap(c, "mrt_img"))) return rc;
    return img_finish(c, rgb8, true);
}

// ---- first-hit AOVs and the a-trous denoiser -------------------------------------------------------------------
// The AOV buffers of this context, computed on first use: *ms = HIP-event time of the pass (0 when they were there already)
// The context's Aov state, allocated on first use: the buffers, and the upload of the scene as the kernels without F_DEEP read
// it where the context's own blob is not that (shared by the AOV pass and mrt_radiance)
static int aov_state(mrt_ctx *c)
{
    const Packed &ap = c->aov_pk ? *c->aov_pk : c->pk;
    const bool own_blob = c->aov_pk || !c->blob.p;      // deep staging, or a multi-device context (its scene lives on the sub-contexts)
    if (!c->aov) {
        const size_t np = (size_t)ap.nw * ap.nh;
        std::unique_ptr<Aov> a(new Aov());
        HIP_TRY(a->guide.alloc(np * 8u));
        HIP_TRY(a->albedo.alloc(np * 3u));
        HIP_TRY(a->ids.alloc(np * 2u));
        HIP_TRY(a->seg.alloc(8u));
        HIP_TRY(hipMemset(a->seg.p, 0, 8u * sizeof(unsigned long long)));
        if (own_blob) {
            const size_t words = ap.blob.size();
            HIP_TRY(a->blob.alloc(words ? words : 4u));
            HIP_TRY(hipMemcpy(a->blob.p, ap.blob.data(), words * 4u, hipMemcpyHostToDevice));
        }
        for (Event &e : a->ev) HIP_TRY(create(e));
        c->aov = std::move(a);
    }
    return MRT_OK;
}

static int aov_compute(mrt_ctx *c, bool &cached, double &ms)
{
    cached = c->aov_ready;
    ms = 0.0;
    if (c->aov_ready) return MRT_OK;
    const Packed &ap = c->aov_pk ? *c->aov_pk : c->pk;
    const bool own_blob = c->aov_pk || !c->blob.p;
    int rc;
    if ((rc = aov_state(c))) return rc;
    Aov &a = *c->aov;
    Params P = ap.P;
    P.blob = own_blob ? a.blob.p : c->blob.p;
    P.segments = a.seg.p;
    HIP_TRY(hipEventRecord(a.ev[0].get(), c->stream.get()));
    HIP_TRY(launch_aov(P, ap.features, a.guide.p, a.albedo.p, a.ids.p, c->stream.get()));
    HIP_TRY(hipEventRecord(a.ev[1].get(), c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    { float t = 0.0f; HIP_TRY(hipEventElapsedTime(&t, a.ev[0].get(), a.ev[1].get())); ms = t; }
    a.inst_first = inst_first(ap);
    c->aov_ready = true;
    return MRT_OK;
}

int mrt_aov(mrt_ctx *c, float *depth, float *normal, float *albedo, int32_t *renderer, int32_t *instance)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_aov: null context");
    bool cached;
    double ms;
    int rc;
    if ((rc = set_device(c)) || (rc = aov_compute(c, cached, ms))) return rc;
    const Aov &a = *c->aov;
    const size_t np = (size_t)c->pk.nw * c->pk.nh;
    if (depth || normal) {
        std::vector<float> g(np * 4u);
        HIP_TRY(hipMemcpy(g.data(), a.guide.p, np * 4u * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t p = 0; p < np; ++p) {
            if (depth) depth[p] = g[4 * p + 3];
            if (normal) for (int k = 0; k < 3; ++k) normal[3 * p + k] = g[4 * p + k];
        }
    }
    if (albedo) HIP_TRY(hipMemcpy(albedo, a.albedo.p, np * 3u * sizeof(float), hipMemcpyDeviceToHost));
    if (renderer || instance) {
        std::vector<i32> ids(np * 2u);
        HIP_TRY(hipMemcpy(ids.data(), a.ids.p, np * 2u * sizeof(i32), hipMemcpyDeviceToHost));
        for (size_t p = 0; p < np; ++p) {
            const i32 r = ids[2 * p];
            if (renderer) renderer[p] = r;
            if (instance) instance[p] = r < 0 ? -1 : ids[2 * p + 1] - (i32)a.inst_first[(u32)r];
        }
    }
    ok();
    return MRT_OK;
}

// Filter options -> passes, the 1/sigma^2 formed in f32 (sigma = +inf: 0, the term is off), the mode and its firefly factor
struct DnOpts { u32 passes, mode; float sc, sn, sp, sv, firefly; };

static int denoise_opts(const mrt_denoise_opts *o, const char *fn, DnOpts &r)
{
    mrt_denoise_opts d;
    memset(&d, 0, sizeof d);
    d.passes = MRT_DENOISE_PASSES;
    d.sigma_color = MRT_DENOISE_SIGMA_COLOR; d.sigma_normal = MRT_DENOISE_SIGMA_NORMAL; d.sigma_plane = MRT_DENOISE_SIGMA_PLANE;
    if (!o) o = &d;
    if (o->passes > kDnMaxPasses) return fail(MRT_ERR_ARG, "%s: passes %u > %u", fn, o->passes, kDnMaxPasses);
    const float sg[3] = {o->sigma_color, o->sigma_normal, o->sigma_plane};
    for (float s : sg) if (!(s > 0.0f)) return fail(MRT_ERR_ARG, "%s: sigma %g is not > 0", fn, (double)s);
    if (o->mode != MRT_DN_ATROUS && o->mode != MRT_DN_VARIANCE) return fail(MRT_ERR_ARG, "%s: unknown mode %u", fn, o->mode);
    if (!(o->sigma_var >= 0.0f)) return fail(MRT_ERR_ARG, "%s: sigma_var %g is not >= 0", fn, (double)o->sigma_var);
    if (!(o->firefly >= 0.0f)) return fail(MRT_ERR_ARG, "%s: firefly %g is not >= 0", fn, (double)o->firefly);
    if (o->mode == MRT_DN_ATROUS && (o->sigma_var != 0.0f || o->firefly != 0.0f))
        return fail(MRT_ERR_ARG, "%s: sigma_var and firefly belong to MRT_DN_VARIANCE and must be 0 in MRT_DN_ATROUS", fn);
    r.passes = o->passes; r.mode = o->mode;
    r.sc = 1.0f / (sg[0] * sg[0]);
    r.sn = 1.0f / (sg[1] * sg[1]);
    r.sp = 1.0f / (sg[2] * sg[2]);
    const float sv = o->sigma_var != 0.0f ? o->sigma_var : MRT_DN_SIGMA_VAR;
    r.sv = 1.0f / (sv * sv);
    r.firefly = o->firefly != 0.0f ? o->firefly : MRT_DN_FIREFLY;
    return MRT_OK;
}

// The filtered means of the accumulator into the context's output plane (*out, on the device); an observation like mrt_img
static int denoise_run(mrt_ctx *c, const mrt_denoise_opts *o, mrt_denoise_info *info, const char *fn, const float **out)
{
    DnOpts d;
    Frame f;
    bool cached;
    double aov_ms;
    int rc;
    if ((rc = denoise_opts(o, fn, d)) || (rc = enter(c))) return rc;
    if (d.mode == MRT_DN_VARIANCE && !c->adaptive)
        return fail(MRT_ERR_STATE, "%s: MRT_DN_VARIANCE needs the half buffer of an adaptive render on this context since its last reset or "
                    "mrt_set_accum; for a uniform budget of n samples call mrt_execute_adaptive with threshold 0 and min_samples = max_samples = n", fn);
    if ((rc = whole_frame(c, fn, "", f)) || (rc = aov_compute(c, cached, aov_ms))) return rc;
    Aov &a = *c->aov;
    const u32 nw = c->pk.nw, nh = c->pk.nh;
    const size_t np = (size_t)nw * nh;
    if (!a.dn.p) HIP_TRY(a.dn.alloc(np * 11u));
    float *e0 = a.dn.p, *e1 = e0 + 4u * np, *dst = e1 + 4u * np;
    const u32 *tc = c->adaptive ? c->ad->counts() : nullptr;     // per-tile counts of the last adaptive call
    const bool env = c->pk.P.off_env != 0u;
    HIP_TRY(hipEventRecord(a.ev[0].get(), c->stream.get()));
    if (d.mode == MRT_DN_VARIANCE && d.passes != 0u)
        HIP_TRY(launch_denoise_var(f.rgb, c->ad->half.p, tc, a.guide.p, a.albedo.p, nw, nh, d.passes, d.sv, d.sn, d.sp, d.firefly, e0, e1, dst, c->stream.get(), env));
    else
        HIP_TRY(launch_denoise(f.rgb, 1.0f / (float)f.count, tc, a.guide.p, a.albedo.p, nw, nh, d.passes, d.sc, d.sn, d.sp, e0, e1, dst, c->stream.get(), env));
    HIP_TRY(hipEventRecord(a.ev[1].get(), c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, a.ev[0].get(), a.ev[1].get()));
    if (info) {
        memset(info, 0, sizeof *info);
        info->aov_ms = aov_ms; info->filter_ms = ms; info->passes = d.passes; info->aov_cached = cached ? 1u : 0u;
        info->reserved[0] = d.mode;
    }
    *out = dst;
    return MRT_OK;
}

int mrt_denoise(mrt_ctx *c, const mrt_denoise_opts *o, float *rgb, mrt_denoise_info *info)
{
    if (!c || !rgb) return fail(MRT_ERR_ARG, "mrt_denoise: null argument");
    const float *dst = nullptr;
    int rc = denoise_run(c, o, info, "mrt_denoise", &dst);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(rgb, dst, (size_t)c->pk.nw * c->pk.nh * 3u * sizeof(float), hipMemcpyDeviceToHost));
    ok();
    return MRT_OK;
}

// mrt_img on the filtered means: tonemap_channel(c', 1.0f, gamma, wexp), then the Lanczos3 path of mrt_img
int mrt_img_denoised(mrt_ctx *c, const mrt_denoise_opts *o, uint8_t *rgb8, mrt_denoise_info *info)
{
    if (!c || !rgb8) return fail(MRT_ERR_ARG, "mrt_img_denoised: null argument");
    const float *dst = nullptr;
    int rc;
    if ((rc = denoise_run(c, o, info, "mrt_img_denoised", &dst)) || (rc = img_prepare(c))) return rc;
    const float wexp = (1.0f - c->pk.exp) * (1.0f - c->pk.exp);
    HIP_TRY(hipEventRecord(c->ev0.get(), c->stream.get()));
    HIP_TRY(launch_tonemap(dst, c->img->ss.p, c->pk.nw * c->pk.nh, 1.0f, c->pk.gamma, wexp, c->stream.get()));
    return img_finish(c, rgb8, true);
}

int mrt_get_stats(mrt_ctx *c, mrt_stats *out)
{
    if (!c || !out) return fail(MRT_ERR_ARG, "mrt_get_stats: null argument");
    if (c->pending) { const int rc = enter(c); if (rc) return rc; }      // an observation: booked samples are traced first
    if (c->stats_pending) { const int rc = resolve_stats(c); if (rc) return rc; }
    *out = c->stats;
    ok();
    return MRT_OK;
}

int mrt_plan_launch(const mrt_render_desc *desc, mrt_plan *out) { return mrt_plan_launch_ext(desc, nullptr, out); }

int mrt_plan_launch_ext(const mrt_render_desc *desc, const mrt_desc_ext *ext, mrt_plan *out)
{
    if (!desc || !out) return fail(MRT_ERR_ARG, "mrt_plan_launch: null argument");
    Packed pk;
    std::string err;
    const int rc = pack_scene(desc, pk, err, PackOpts(), ext);
    if (rc != MRT_OK) return fail(rc, "mrt_plan_launch: %s", err.c_str());
    const u32 n_nodes = pk.n_tbvh_nodes;
    Plan pl;
    plan_launch(desc, ext, Knobs::from_env(), pk, pl);
    fill_plan(pl, pk, n_nodes, *out);
    ok();
    return MRT_OK;
}

int mrt_selftest_math(int device, int op, const float *a, const float *b, float *out, size_t n)
{
    if (!a || !out) return fail(MRT_ERR_ARG, "mrt_selftest_math: null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MRT_ERR_DEVICE, "mrt_selftest_math: no HIP device");
    if (device < 0) device = 0;
    HIP_TRY(hipSetDevice(device));
    if (n == 0) { ok(); return MRT_OK; }
    const size_t bytes = n * sizeof(float);
    DeviceMem<float> da, dout, db;
    HIP_TRY(da.alloc(n));
    HIP_TRY(dout.alloc(n));
    HIP_TRY(hipMemcpy(da.p, a, bytes, hipMemcpyHostToDevice));
    if (b) { HIP_TRY(db.alloc(n)); HIP_TRY(hipMemcpy(db.p, b, bytes, hipMemcpyHostToDevice)); }
    if (op >= 16) {
        if (op > 19) return fail(MRT_ERR_ARG, "mrt_selftest_math: op %d", op);
        HIP_TRY(launch_math_selftest_ext(op, da.p, db.p, dout.p, n, nullptr));
    } else {
        HIP_TRY(launch_math_selftest(op, da.p, db.p, dout.p, n, nullptr));
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
    ok();
    return MRT_OK;
}

int mrt_selftest_trace(mrt_ctx *c, size_t n, const float *orig, const float *dir, uint32_t *out)
{
    if (!c || !orig || !dir || !out) return fail(MRT_ERR_ARG, "mrt_selftest_trace: null argument");
    if (n == 0 || n >= ((size_t)1 << 31)) return fail(MRT_ERR_ARG, "mrt_selftest_trace: n = %zu", n);
    if (c->group) return fail(MRT_ERR_STATE, "mrt_selftest_trace: multi-device context");
    if (c->shard_count > 1) return fail(MRT_ERR_STATE, "mrt_selftest_trace: sharded context");
    const bool in_lds = c->plan.in_lds;
    const u32 inst = pt_instantiation(256u, in_lds, c->pk.features);
    if (!rayq_has(in_lds, inst))
        return fail(MRT_ERR_STATE, "mrt_selftest_trace: no ray-query kernel for FEAT %u with the scene in %s", inst, in_lds ? "LDS" : "L2");
    const size_t lds = pt_lds_bytes(c->P, 256u, in_lds, c->pk.features);
    if (lds > kLdsLimit) return fail(MRT_ERR_STATE, "mrt_selftest_trace: FEAT %u needs %zu bytes of LDS at 256 threads", inst, lds);
    int rc;
    if ((rc = set_device(c))) return rc;
    DeviceMem<float> d_o, d_d;
    DeviceMem<u32> d_out;
    HIP_TRY(d_o.alloc(n * 3u));
    HIP_TRY(d_d.alloc(n * 3u));
    HIP_TRY(d_out.alloc(n * MRT_TRACE_WORDS));
    HIP_TRY(hipMemcpy(d_o.p, orig, n * 3u * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_d.p, dir, n * 3u * sizeof(float), hipMemcpyHostToDevice));
    // the context's own parameter block and blob: staging level, walk areas and the axis scan act as in its renders; the diagnostic
    // counters of the mesh walks (mrt_trace.h count_fallback) go to a buffer of the call's own: nothing of the context is written
    DeviceMem<unsigned long long> d_seg;
    HIP_TRY(d_seg.alloc(8u));
    HIP_TRY(hipMemset(d_seg.p, 0, 8u * sizeof(unsigned long long)));
    Params P = c->P;
    P.count_segments = 0u;
    P.segments = d_seg.p;
    P.tile_counter = nullptr; P.accum = nullptr; P.partial = nullptr;
    HIP_TRY(launch_rayq(P, in_lds, inst, lds, (u32)n, d_o.p, d_d.p, d_out.p, c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    HIP_TRY(hipMemcpy(out, d_out.p, n * MRT_TRACE_WORDS * sizeof(u32), hipMemcpyDeviceToHost));
    // flat instance index -> index within its renderer's inst list
    const std::vector<u32> first = inst_first(c->pk);
    for (size_t i = 0; i < n; ++i) {
        uint32_t *q = out + i * MRT_TRACE_WORDS;
        if (q[0] && q[2] < first.size()) q[3] -= first[q[2]];
    }
    ok();
    return MRT_OK;
}

// ---- radiance along caller-supplied rays ------------------------------------------------------------------------
int mrt_radiance(mrt_ctx *c, const mrt_rays *r, float *rgb, mrt_rays_info *info)
{
    if (!c || !r || !rgb || !r->orig || !r->dir) return fail(MRT_ERR_ARG, "mrt_radiance: null argument");
    if (r->n == 0 || r->n >= ((size_t)1 << 30)) return fail(MRT_ERR_ARG, "mrt_radiance: n = %zu is outside 1 .. 2^30 - 1", r->n);
    if (r->n_samples == 0) return fail(MRT_ERR_ARG, "mrt_radiance: n_samples = 0");
    if ((unsigned long long)r->sample_base + r->n_samples > 0xffffffffull)
        return fail(MRT_ERR_ARG, "mrt_radiance: samples [%u, + %u) reach past 2^32 - 1", r->sample_base, r->n_samples);
    if (r->flags & ~(uint32_t)MRT_RAYS_DEVICE) return fail(MRT_ERR_ARG, "mrt_radiance: unknown flags 0x%x", r->flags);
    if (r->reserved[0] || r->reserved[1] || r->reserved[2]) return fail(MRT_ERR_ARG, "mrt_radiance: reserved words must be 0");
    if (c->group) return fail(MRT_ERR_STATE, "mrt_radiance: multi-device context");
    int rc;
    if ((rc = set_device(c))) return rc;
    // The scene as a kernel without F_DEEP reads it: the context's own blob, or (deep staging) the binary-BVH packing of the AOV pass
    const Packed &rp = c->aov_pk ? *c->aov_pk : c->pk;
    Params P = c->P;
    if (c->aov_pk) {
        if ((rc = aov_state(c))) return rc;
        P = rp.P;
        P.seed_lo = c->P.seed_lo; P.seed_hi = c->P.seed_hi;
        P.blob = c->aov->blob.p;
    }
    const u32 inst = pt_instantiation(256u, false, rp.features);
    // Staged in LDS when the context stages the whole scene and four 256-thread workgroups of it -- the 4 waves per SIMD these
    // feature sets are bound to -- still fit a CU; through L2 otherwise (warm, deep and L2 contexts, MRT_SCENE_IN_L2)
    const bool in_lds = c->plan.in_lds && c->plan.staging == 0u && rays_lds_bytes(P, true, inst) <= kLdsLimit / 4u;
    const size_t lds = rays_lds_bytes(P, in_lds, inst);
    const size_t n = r->n;
    const bool dev = (r->flags & MRT_RAYS_DEVICE) != 0u;
    DeviceMem<float> d_o, d_d, d_rgb;
    DeviceMem<u32> d_key;
    const float *po = r->orig, *pd = r->dir;
    const u32 *pkey = r->key;
    float *pout = rgb;
    if (!dev) {
        HIP_TRY(d_o.alloc(n * 3u));
        HIP_TRY(d_d.alloc(n * 3u));
        HIP_TRY(d_rgb.alloc(n * 3u));
        HIP_TRY(hipMemcpy(d_o.p, r->orig, n * 3u * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_d.p, r->dir, n * 3u * sizeof(float), hipMemcpyHostToDevice));
        if (r->key) {
            HIP_TRY(d_key.alloc(n));
            HIP_TRY(hipMemcpy(d_key.p, r->key, n * sizeof(u32), hipMemcpyHostToDevice));
            pkey = d_key.p;
        }
        po = d_o.p; pd = d_d.p; pout = d_rgb.p;
    }
    // everything the kernel writes belongs to the call: the sums, and a segment counter of its own
    DeviceMem<unsigned long long> d_seg;
    HIP_TRY(d_seg.alloc(8u));
    Event e0, e1;
    HIP_TRY(create(e0));
    HIP_TRY(create(e1));
    hipStream_t st = c->stream.get();
    HIP_TRY(hipMemsetAsync(d_seg.p, 0, 8u * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(pout, 0, n * 3u * sizeof(float), st));
    P.n_samples = r->n_samples; P.sample_base = r->sample_base;
    P.k_split = 1u; P.to_planes = 0u;
    P.accum = pout; P.partial = nullptr; P.partial_stride = 0ull;
    P.count_segments = 1u; P.segments = d_seg.p;
    P.tile_counter = nullptr; P.persist_grid = 0u;
    HIP_TRY(hipEventRecord(e0.get(), st));
    HIP_TRY(launch_rays(P, in_lds, inst, (u32)n, po, pd, pkey, st));
    HIP_TRY(hipEventRecord(e1.get(), st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!dev) HIP_TRY(hipMemcpy(rgb, d_rgb.p, n * 3u * sizeof(float), hipMemcpyDeviceToHost));
    if (info) {
        memset(info, 0, sizeof *info);
        float t = 0.0f;
        HIP_TRY(hipEventElapsedTime(&t, e0.get(), e1.get()));
        unsigned long long seg = 0;
        HIP_TRY(hipMemcpy(&seg, d_seg.p, sizeof seg, hipMemcpyDeviceToHost));
        info->kernel_ms = t;
        info->samples = (uint64_t)n * r->n_samples;
        info->segments = seg;
        info->kernel_features = inst;
        info->scene_in_lds = in_lds ? 1u : 0u;
        info->lds_bytes = (uint32_t)lds;
    }
    ok();
    return MRT_OK;
}

int mrt_camera_rays(mrt_ctx *c, float *orig, float *dir)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_camera_rays: null context");
    if (c->group) return fail(MRT_ERR_STATE, "mrt_camera_rays: multi-device context");
    int rc;
    if ((rc = set_device(c))) return rc;
    const size_t words = (size_t)c->pk.nw * c->pk.nh * 3u;
    DeviceMem<float> d_o, d_d;
    if (orig) HIP_TRY(d_o.alloc(words));
    if (dir) HIP_TRY(d_d.alloc(words));
    if (orig || dir) {
        HIP_TRY(launch_camera_rays(c->P, d_o.p, d_d.p, c->stream.get()));
        HIP_TRY(hipStreamSynchronize(c->stream.get()));
    }
    if (orig) HIP_TRY(hipMemcpy(orig, d_o.p, words * sizeof(float), hipMemcpyDeviceToHost));
    if (dir) HIP_TRY(hipMemcpy(dir, d_d.p, words * sizeof(float), hipMemcpyDeviceToHost));
    ok();
    return MRT_OK;
}

int mrt_selftest_sweep(int device, int op, uint64_t first, uint64_t count, uint32_t seed, uint64_t *mismatches, float *example)
{
    if (!mismatches) return fail(MRT_ERR_ARG, "mrt_selftest_sweep: null argument");
    if (op < 0 || op > 3) return fail(MRT_ERR_ARG, "mrt_selftest_sweep: op %d", op);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MRT_ERR_DEVICE, "mrt_selftest_sweep: no HIP device");
    if (device < 0) device = 0;
    HIP_TRY(hipSetDevice(device));
    DeviceMem<unsigned long long> d_mis;
    DeviceMem<float> d_ex;
    unsigned long long mis = 0;
    float ex[4] = {0, 0, 0, 0};
    HIP_TRY(d_mis.alloc(1));
    HIP_TRY(d_ex.alloc(4));
    HIP_TRY(hipMemset(d_mis.p, 0, sizeof(unsigned long long)));
    HIP_TRY(hipMemset(d_ex.p, 0, 4 * sizeof(float)));
    const uint64_t slice = 1ull << 28;                 // one launch per 2^28 elements
    for (uint64_t done = 0; done < count; done += slice) {
        const uint64_t n = count - done < slice ? count - done : slice;
        HIP_TRY(launch_math_sweep(op, first + done, n, seed, d_mis.p, d_ex.p, nullptr));
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&mis, d_mis.p, sizeof mis, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ex, d_ex.p, sizeof ex, hipMemcpyDeviceToHost));
    *mismatches = mis;
    if (example) memcpy(example, ex, sizeof ex);
    ok();
    return MRT_OK;
}

}  // extern "C"
