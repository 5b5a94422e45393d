// mrt_ctx.h — what the host units behind the C ABI of include/mrt.h share: the error state, the owners of device resources, the
// per-feature state structs, the context, and the few functions that cross from one unit to another (DESIGN.md §1 has the map
// of the units).  Internal to the library; no kernel source includes it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/mrt.h"
#include "mrt_err.h"
#include "mrt_kernels.h"
#include "mrt_pack.h"
#include "mrt_plan.h"
#include "mrt_trace.h"

namespace mrt {
namespace api {

// A HIP call whose failure is tolerated: HIP 7 keeps the last *real* error pending (hipGetLastError no longer reports the
// last call's status), so the pending error is cleared here or the next launch's hipGetLastError() would report it.
inline bool hip_tolerated(hipError_t e)
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
// The counter block Params.segments points at, zeroed: segment counter + tile counter + 4 phase clocks (debug builds) and the
// diagnostic counters of the mesh walks (mrt_trace.h count_fallback).  The context has one; a call that must leave the
// context untouched (the AOV pass, mrt_selftest_trace, mrt_radiance) brings its own.
inline hipError_t alloc_counters(DeviceMem<unsigned long long> &m)
{
    const hipError_t e = m.alloc(8);
    return e != hipSuccess ? e : hipMemset(m.p, 0, 8 * sizeof(unsigned long long));
}
// Caller-supplied rays on the device for the length of one call (mrt_radiance, mrt_radiance_adaptive, mrt_aov_rays): orig and dir
// are what a launch reads -- the caller's own device pointers (on_device), or one upload of its n_rays x 3 host floats each
struct DeviceRays {
    DeviceMem<float> up_o, up_d;
    const float *orig = nullptr, *dir = nullptr;
    hipError_t take(const float *o, const float *d, size_t n_rays, bool on_device)
    {
        orig = o; dir = d;
        if (on_device) return hipSuccess;
        const size_t words = n_rays * 3u;
        hipError_t e;
        if ((e = up_o.alloc(words)) || (e = up_d.alloc(words)) || (e = hipMemcpy(up_o.p, o, words * sizeof(float), hipMemcpyHostToDevice)) ||
            (e = hipMemcpy(up_d.p, d, words * sizeof(float), hipMemcpyHostToDevice))) return e;
        orig = up_o.p; dir = up_d.p;
        return hipSuccess;
    }
};
struct EventDestroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct StreamDestroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
using Event = std::unique_ptr<ihipEvent_t, EventDestroy>;
using Stream = std::unique_ptr<ihipStream_t, StreamDestroy>;
inline hipError_t create(Event &ev) { hipEvent_t e; const hipError_t r = hipEventCreate(&e); if (r == hipSuccess) ev.reset(e); return r; }
inline hipError_t create(Stream &st) { hipStream_t s; const hipError_t r = hipStreamCreateWithFlags(&s, hipStreamNonBlocking); if (r == hipSuccess) st.reset(s); return r; }

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
// One axis of a resample on the device: the tables of a ResampleTaps over n output indices, as the kernels read them (DevTaps)
struct Taps {
    DeviceMem<u32> left, count;
    DeviceMem<float> weight;
    u32 cap = 0;
    hipError_t upload(const ResampleTaps &t, u32 n)
    {
        hipError_t e;
        if ((e = left.alloc(n)) || (e = count.alloc(n)) || (e = weight.alloc((size_t)n * t.cap))) return e;
        if ((e = hipMemcpy(left.p, t.left.data(), sizeof(u32) * n, hipMemcpyHostToDevice)) ||
            (e = hipMemcpy(count.p, t.count.data(), sizeof(u32) * n, hipMemcpyHostToDevice)) ||
            (e = hipMemcpy(weight.p, t.weight.data(), sizeof(float) * (size_t)n * t.cap, hipMemcpyHostToDevice))) return e;
        cap = t.cap;
        return hipSuccess;
    }
    DevTaps dev() const { return {left.p, count.p, weight.p, cap}; }
};
// ... and both passes of one: vertical first
struct Resampler { Taps v, h; };
// the image path (mrt_img, mrt_img_ss, mrt_img_denoised); Lanczos3 to the output resolution when it differs: its taps, the
// vertical pass's output (tmp), the image (out)
struct Image {
    DeviceMem<unsigned char> ss;                  // the tone-mapped supersampled frame [nh][nw][3]
    Resampler lanczos3;
    DeviceMem<float> tmp;
    DeviceMem<unsigned char> out;
};
// the linear float image (mrt_img_hdr), created whole by the first call: the box taps (the Lanczos3 taps are the
// Image's own), the vertical pass's output, the image, the events around the call's kernels
struct Hdr {
    Resampler box;
    DeviceMem<float> tmp, out;                    // tmp [res_h][nw][3], out [res_h][res_w][3]
    Event ev[2];
};
// first-hit AOVs and the denoiser (mrt_aov, mrt_denoise: DESIGN.md §13), on the context's device; the AOVs depend on scene and
// camera only (or on the rays mrt_aov_rays was given) and survive mrt_reset
struct Aov {
    DeviceMem<float> guide;                       // [2][nh][nw] float4: (normal, depth), (world point, hit flag)
    DeviceMem<float> albedo;                      // [nh][nw][3]
    DeviceMem<i32> ids;                           // [nh][nw][2]: renderer, flat instance index
    DeviceMem<unsigned long long> seg;            // the AOV kernel's diagnostic counters (mrt_trace.h count_fallback)
    Event ev[2];                                  // around the AOV pass, then around the filter
    std::vector<u32> inst_first;                  // flat index of each renderer's first instance (ids -> mrt_scene order)
    bool from_rays = false;                       // the planes are those of caller-supplied rays (mrt_aov_rays), not the camera's
    bool wrap_x = false;                          // ... of a grid periodic in x (MRT_AOV_WRAP_X): the a-trous passes wrap their horizontal taps
    DeviceMem<float> dn;                          // two e planes ([nh][nw] float4) and the filtered means [nh][nw][3]: the first mrt_denoise
};
// in-process multi-device context (mrt_opts.n_devices > 1): one sharded sub-context per device, gathered on device 0
typedef struct ncclComm *ncclComm_t;
struct Group {
    std::vector<std::unique_ptr<mrt_ctx>> subs;
    std::vector<ncclComm_t> comms;
    DeviceMem<float> gather;                      // [n_devices][padded_rows][nw][3] on device 0
    DeviceMem<u32> rowmap;                        // [n_devices][padded_rows] frame row of each gathered row (0xffffffff: padding)
    void release();                               // the sub-contexts, then the comms
    ~Group();
};

}  // namespace api
}  // namespace mrt

struct mrt_ctx {
    int device = 0;
    mrt::api::Stream stream;                      // declared first: destroyed last
    mrt::api::Event ev0, ev1;                     // img timing; on a group context: around scatter_rows
    mrt::api::Event ev_g0, ev_g1;                 // sub-context of a group: around this rank's part of the ncclGather, on its stream
    std::vector<mrt::api::Event> evs;             // 3 per launch of the last execute: start, after pt_megakernel, after reduce_chunks
    mrt::u32 ev_used = 0;
    bool stats_pending = false;                   // event times / segment counter of the last execute not read back yet
    bool count_segments = false;                  // MRT_FLAG_COUNT_SEGMENTS
    bool event_timing = true;                     // !MRT_FLAG_NO_EVENT_TIMING
    bool defer = false;                           // MRT_FLAG_DEFER / MRT_DEFER=1
    bool handed_out = false;                      // mrt_accum_device_ptr gave the raw device pointer away: sticky, the caller may read it at any time
    bool bound = false;                           // the accumulator lives in caller memory (a successful mrt_bind_accum)
    bool exposed() const { return handed_out || bound; }   // either way the memory is visible behind the library's back: no deferral
    mrt::Knobs knobs;                             // the environment as mrt_create found it (a thread-per-connection server calls
                                                  // mrt_execute per sample: that path reads no environment)
    mrt::u32 pending = 0;                         // samples requested by deferred mrt_execute calls and not traced yet
    // look-ahead of the eager per-call path (the reference's callers run one Sampler::execute per sample): see run_lookahead
    bool la_enabled = false;                      // eager single-device context without MRT_FLAG_NO_LOOKAHEAD / MRT_LOOKAHEAD=0
    mrt::u32 la_max = 32;                         // samples per look-ahead launch at most (MRT_LOOKAHEAD=n)
    mrt::u32 la_streak = 0;                       // consecutive one-sample calls so far
    std::unique_ptr<mrt::api::Lookahead> la;
    mrt::Packed pk;
    std::unique_ptr<mrt::Packed> aov_pk;          // deep-staged contexts: the scene as packed without them (binary triangle BVHs) for the kernels without F_DEEP
    mrt::Params P;
    mrt::api::DeviceMem<mrt::u32> blob;           // the packed scene (none on a group context: it lives on the sub-contexts)
    mrt::api::DeviceMem<mrt::u32> flat_blob;      // the flat scene where `blob` is not it (deep staging, group contexts): uploaded by the first flat_scene()
    float *d_accum = nullptr;                     // [padded_rows][nw][3], rows past local_rows stay zero: accum_own or caller memory
    mrt::api::DeviceMem<float> accum_own;
    mrt::api::DeviceMem<float> partial;           // chunk sums of a sample-split launch
    mrt::u32 padded_rows = 0;
    mrt::api::DeviceMem<unsigned long long> segments;   // the context's counter block (alloc_counters)
    mrt::u32 count = 0;                           // Sampler.last_count
    uint64_t seed = 0;
    mrt::u32 shard_index = 0, shard_count = 1, shard_rows = 8, local_rows = 0;
    std::vector<mrt::u32> row_of;                 // local row -> frame row
    mrt::api::DeviceMem<float> full;              // [nh][nw][3]: a group's frame, or the full frame a sharded context received
    mrt::u32 full_count = 0;
    mrt::Plan plan;                               // staging level, launch shape, kernel instantiation (mrt_plan.h): fixed by mrt_create
    mrt::u32 persist_grid = 0;                    // persistent grid of the batched shape
    mrt_stats stats;
    std::unique_ptr<mrt::api::Group> group;
    bool adaptive = false;                        // the accumulator holds an adaptive render: per-tile counts, count = the smallest
    bool adaptive_rays = false;                   // ... of caller-supplied rays (mrt_radiance_adaptive): the half buffer belongs to their grid, not the camera's frame
    std::unique_ptr<mrt::api::Adaptive> ad;
    std::unique_ptr<mrt::api::Image> img;
    std::unique_ptr<mrt::api::Hdr> hdr;
    bool aov_ready = false;                       // the AOVs have been computed
    std::unique_ptr<mrt::api::Aov> aov;
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

namespace mrt {
namespace api {

// floats of one [padded_rows][nw][3] plane: the accumulator, H, a chunk plane, a look-ahead plane
inline size_t plane_floats(const mrt_ctx *c) { return (size_t)c->padded_rows * c->pk.nw * 3; }

// (1 - exp)^2 of the extended Reinhard curve, as both tone-map launches take it (the frame's and the filtered means')
inline float tonemap_wexp(const mrt_ctx *c) { return (1.0f - c->pk.exp) * (1.0f - c->pk.exp); }

inline int set_device(const mrt_ctx *c)
{
    HIP_TRY(hipSetDevice(c->device));
    return MRT_OK;
}

// The frame an observation reads and its sample count: the full frame of a group, or of a sharded context that received one,
// else the accumulator -- rgb is null when that holds only the context's own rows.
struct Frame { const float *rgb; u32 count; };
inline Frame frame_of(const mrt_ctx *c)
{
    if (c->full.p) return {c->full.p, c->full_count};
    return {c->shard_count == 1 ? c->d_accum : nullptr, c->count};
}
// The means an observation reads (mrt_adapt.h MeanSrc): a plane of finished means as it is (the denoiser's output), or -- means
// null -- that frame's sums with its 1/count, per 8x8 tile after an adaptive render (the tile counts of the last adaptive call)
inline MeanSrc mean_src(const mrt_ctx *c, const float *means = nullptr)
{
    if (means) return {means, 1.0f, nullptr, c->pk.nw};
    const Frame f = frame_of(c);
    return {f.rgb, adapt_recip(f.count), c->adaptive ? c->ad->counts() : nullptr, c->pk.nw};
}
// ... of the whole frame (the image, the denoiser, the float image), refused without the whole frame or a sample
inline int whole_frame(const mrt_ctx *c, const char *fn, const char *empty_note, MeanSrc &S)
{
    const Frame f = frame_of(c);
    if (!f.rgb) return fail(MRT_ERR_STATE, "%s: this context holds only its own rows; gather and mrt_set_accum first", fn);
    if (f.count == 0) return fail(MRT_ERR_STATE, "%s: no samples accumulated%s", fn, empty_note);
    S = mean_src(c);
    return MRT_OK;
}

// ---- the functions that cross unit boundaries ---------------------------------------------------------------------------------

// mrt_create.cpp
// The scene as a kernel without F_DEEP reads it (the AOV pass, mrt_radiance): the context's own packing and blob, or -- deep
// staging, whose own blob holds 4-wide triangle BVHs, and multi-device contexts, whose scene lives on the sub-contexts -- the
// flat packing and an upload of it made by the first call.  blob is null when that upload failed (the error is set).
struct FlatScene { const Packed &pk; const u32 *blob; };
FlatScene flat_scene(mrt_ctx *c);
// A multi-device context's mrt_execute: every sub-context's launches, one ncclGather to device 0, the rows into the frame
int exec_group(mrt_ctx *g, uint32_t n_samples);

// mrt_radiance.cpp
// What mrt_radiance and mrt_radiance_adaptive launch for this context: the arguments of a kernel without F_DEEP on the flat scene
// (the context's seed; accumulator, planes, counters and sampling range are the caller's to set), its instantiation
// pt_instantiation(256, false, features), whether it stages the scene in LDS, and its LDS bytes.  orig, dir: the rays of a
// tile-list launch, on the device (launch_batch).  Sets the error and returns its code when the flat scene cannot be had.
struct RaysKernel {
    Params P;
    u32 inst = 0;
    bool in_lds = false;
    size_t lds = 0;
    const float *orig = nullptr, *dir = nullptr;
};
int rays_kernel(mrt_ctx *c, RaysKernel &k);
// The flags and reserved words of mrt_rays and mrt_rays_adapt (fn: the caller's name in the message)
inline int rays_words(uint32_t flags, const uint32_t (&reserved)[3], const char *fn)
{
    if (flags & ~(uint32_t)MRT_RAYS_DEVICE) return fail(MRT_ERR_ARG, "%s: unknown flags 0x%x", fn, flags);
    if (reserved[0] || reserved[1] || reserved[2]) return fail(MRT_ERR_ARG, "%s: reserved words must be 0", fn);
    return MRT_OK;
}

// mrt_execute.cpp
// asynchronous half of mrt_execute on one device: everything up to the closing event
int exec_launch(mrt_ctx *c, uint32_t n_samples);
// ... and the other half: wait for it, advance the count
int exec_finish(mrt_ctx *c, uint32_t n_samples);
// the statistics of one execute start over (an adaptive call's, and a look-ahead call's, as well)
void reset_exec_stats(mrt_ctx *c);
// Lazy half of the per-execute statistics: HIP-event times and (MRT_FLAG_COUNT_SEGMENTS) the segment counter are read
// back when somebody asks (mrt_get_stats), not on every mrt_execute -- the reference's callers run one pass per call
// (src/cli.rs:162-170), so the per-call cost is what the drop-in binary pays 1024 times per frame.
int resolve_stats(mrt_ctx *c);
// Samples [base, base + n) of the whole frame (tl null) or of the listed tiles, asynchronous on c->stream: the sample split
// (split_policy, sized from the tiles traced), cut into chunk-aligned launches, each followed by the fold of its chunk sums into
// the accumulator -- and into `half` too when it is not null (listed tiles only).  planes: every launch goes through the chunk
// planes.  k_split receives split_policy's lanes per pixel; ks_max is raised to the largest split of any launch.
// rk (listed tiles only): the trace launches are pt_rays_tiles on rk's rays with rk->P -- whose sampling range, split and planes
// this sets -- in place of the context's own kernel and c->P; split, cut and folds are the same.
int launch_batch(mrt_ctx *c, u32 base, u32 n, const TileList *tl, float *half, bool planes, u32 &k_split, u32 &ks_max, RaysKernel *rk = nullptr);
// The look-ahead of the eager per-call path: any call other than a one-sample execute (n != 1, reset, set_accum) drops what was
// traced ahead
void la_drop(mrt_ctx *c);
// Deferred execution (MRT_FLAG_DEFER): trace what earlier mrt_execute calls only booked.  Called by every entry point that
// observes or replaces the accumulator; the result is the same set of samples as if each call had run at once.
int settle(mrt_ctx *c);
// the prologue of the entry points that observe or replace the accumulator: the context's device, then what was booked
int enter(mrt_ctx *c);

// mrt_accum.cpp
// The image buffers, created whole by the first call: a failure half-way leaves the context as it was, and the next call
// starts over
int img_prepare(mrt_ctx *c);
// The end of the image entry points: the tone-mapped frame, through Lanczos3 when `resize` asks for the output resolution and it
// differs (image 0.24 resize copies when the dimensions match); then close the timing of the image kernels, wait for them and
// copy the image out
int img_finish(mrt_ctx *c, uint8_t *rgb8, bool resize);

// mrt_aov.cpp
// The filtered means of the accumulator into the context's output plane (*out [nh][nw][3], on the device); an observation like
// mrt_img, with its own enter()
int denoise_run(mrt_ctx *c, const mrt_denoise_opts *o, mrt_denoise_info *info, const char *fn, const float **out);

}  // namespace api
}  // namespace mrt
