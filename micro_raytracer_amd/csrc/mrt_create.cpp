// mrt_create.cpp — mrt_create / mrt_destroy: the single-device context, and the in-process multi-device one with everything
// that is its alone (the RCCL loader, the group's gather in exec_group); the flat scene of contexts whose own blob is not it.
// The functions defined here as mrt::api::name are the ones other units call: mrt_ctx.h declares them and says what they do.
#include <dlfcn.h>
#include <stddef.h>
#include <string.h>

#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "mrt_ctx.h"
#include "mrt_shard.h"

using namespace mrt;
using namespace mrt::api;

namespace {

// ---- RCCL, loaded on demand (only in-process multi-device contexts need it; signatures from rccl/rccl.h) ----
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

}  // namespace

void mrt::api::Group::release()
{
    subs.clear();
    for (ncclComm_t cm : comms) if (cm) g_rccl.CommDestroy(cm);
    comms.clear();
}
mrt::api::Group::~Group() { release(); }

// (mrt_ctx.h)  The upload is the context's: whichever reader calls first makes it, every later call finds it.
FlatScene mrt::api::flat_scene(mrt_ctx *c)
{
    if (!c->aov_pk && c->blob.p) return {c->pk, c->blob.p};
    const Packed &fp = c->aov_pk ? *c->aov_pk : c->pk;
    if (!c->flat_blob.p) {
        const size_t words = fp.blob.size();
        const int rc = [&]() -> int {
            HIP_TRY(c->flat_blob.alloc(words ? words : 4u));
            HIP_TRY(hipMemcpy(c->flat_blob.p, fp.blob.data(), words * 4u, hipMemcpyHostToDevice));
            return MRT_OK;
        }();
        if (rc) { c->flat_blob.reset(); return {fp, nullptr}; }
    }
    return {fp, c->flat_blob.p};
}

// ---- mrt_execute on a multi-device context ---------------------------------------------------------------------------------------
int mrt::api::exec_group(mrt_ctx *g, uint32_t n_samples)
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

extern "C" {

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
    if (c->pk.tbvh_wide) {                   // the kernels without an F_DEEP build (flat_scene) walk the binary triangle BVHs
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

    // rows of this shard and the rows its planes are allocated for (mrt_shard.h): checked before the first allocation, since a
    // plane of fewer rows than the kernels write is an out-of-bounds device write -- a guard, no input should reach it
    {
        ShardLayout L = shard_layout(c->pk.nh, opts->shard_index, shard_count, opts->shard_rows);
        if (L.local_rows > L.padded_rows || L.padded_rows > 0xffffffffull) {
            fail(MRT_ERR_ARG, "mrt_create: shard layout of %u rows (shard %u of %u, blocks of %u): %u local rows in %llu padded rows", c->pk.nh,
                 opts->shard_index, shard_count, opts->shard_rows, L.local_rows, (unsigned long long)L.padded_rows);
            return nullptr;
        }
        c->shard_rows = L.shard_rows;              // the effective value, min(shard_rows, nh): what the kernels divide by
        c->local_rows = L.local_rows;
        c->padded_rows = (u32)L.padded_rows;
        c->row_of = std::move(L.row_of);
    }

    auto bail = [&](int code, const char *what, hipError_t e) { fail(code, "mrt_create: %s: %s", what, hipGetErrorString(e)); return (mrt_ctx *)nullptr; };
    hipError_t e;
    if ((e = hipSetDevice(dev)) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipSetDevice", e);
    if ((e = create(c->stream)) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipStreamCreate", e);
    if ((e = create(c->ev0)) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipEventCreate", e);
    if ((e = create(c->ev1)) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipEventCreate", e);
    const size_t all_words = c->pk.blob.size();
    if ((e = c->blob.alloc(all_words ? all_words : 4)) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipMalloc(scene)", e);
    if ((e = hipMemcpy(c->blob.p, c->pk.blob.data(), all_words * 4, hipMemcpyHostToDevice)) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipMemcpy(scene)", e);
    if ((e = c->accum_own.alloc(plane_floats(c.get()))) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipMalloc(accumulator)", e);
    c->d_accum = c->accum_own.p;
    if ((e = hipMemset(c->d_accum, 0, plane_floats(c.get()) * sizeof(float))) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipMemset", e);
    if ((e = alloc_counters(c->segments)) != hipSuccess) return bail(MRT_ERR_DEVICE, "hipMalloc(counters)", e);

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
    g->shard_count = 1; g->shard_index = 0;
    {   // the group itself owns every row; its sub-contexts deal them by the caller's shard_rows
        ShardLayout L = shard_layout(g->pk.nh, 0, 1, opts->shard_rows);
        g->shard_rows = L.shard_rows; g->local_rows = L.local_rows; g->padded_rows = (u32)L.padded_rows;
        g->row_of = std::move(L.row_of);
    }
    g->group.reset(new Group());
    Group &gr = *g->group;
    for (u32 r = 0; r < n; ++r) {
        mrt_opts o = *opts;
        o.n_devices = 0; o.device = (int)r; o.shard_index = r; o.shard_count = n; o.shard_rows = opts->shard_rows;
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

}  // extern "C"
