// mrt_hooks.cpp — the entry points the tests drive the library's parts through: the launch plan as data (mrt_plan_launch*, host
// only) and the device self-tests (mrt_selftest_math, mrt_selftest_sweep, mrt_selftest_trace).
#include <string.h>

#include <string>
#include <vector>

#include "mrt_ctx.h"

using namespace mrt;
using namespace mrt::api;

extern "C" {

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
    HIP_TRY(alloc_counters(d_seg));
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
