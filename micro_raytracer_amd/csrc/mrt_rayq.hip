// mrt_rayq.hip — gfx950 kernel of the ray-query test hook (mrt_selftest_trace).  A translation unit of its own, so
// that the other kernels are compiled exactly as without it.
//
//   rayq   ray i = thread i of a launch of 256-thread workgroups (lane i % 64 of wavefront i / 64): the closest-hit and the
//          shadow query of trace on a caller-supplied ray, behind the prologue of pt_megakernel (mrt_pt_kernel.h) -- the
//          scene staged in LDS as the context's path-tracing kernel stages it, the walk areas behind the stash region
//   math_selftest_ext   ops 16.. of mrt_selftest_math: the composed expressions of the math contract as their call sites write
//          them (hit_uv / env_uv's longitude and latitude, the sphere's two roots over one reciprocal), elementwise
//
// Build: as mrt_kernels.hip.
#include <hip/hip_runtime.h>

#include "mrt_kernels.h"
#include "mrt_megakernel.h"
#include "mrt_rayq.h"

namespace mrt {

template <bool SCENE_IN_LDS, u32 FEAT>
__global__ void __launch_bounds__(256) rayq(const Params P, const u32 *__restrict__ blob_g, u32 n, const float *__restrict__ orig,
                                            const float *__restrict__ dir, u32 *__restrict__ out)
{
    constexpr int BLOCK_THREADS = 256;
    // the staging prologue of pt_megakernel (mrt_pt_kernel.h has the original), written out: a shared helper is not free
    extern __shared__ uint4 lds_blob[];
    const float *F;
    const u32 staged_words = !SCENE_IN_LDS ? 0u : staged_words_for(P, FEAT);
    if (SCENE_IN_LDS) {
        const uint4 *g = reinterpret_cast<const uint4 *>(P.blob);
        const u32 n4 = staged_words >> 2;
        for (u32 i = threadIdx.x; i < n4; i += blockDim.x) lds_blob[i] = g[i];
        __syncthreads();
        F = reinterpret_cast<const float *>(lds_blob);
    } else {
        F = reinterpret_cast<const float *>(P.blob);
    }
    Scn S;
    S.F = F;
    S.U = F;
    S.G = reinterpret_cast<const float *>(blob_g);
    S.P = &P;
    // behind the staged scene (16-byte aligned): [lane stash region, unused here] [walk areas: P.walk_cap x blockDim words]
    const u32 stash_base4 = (staged_words + 3u) >> 2;
    constexpr bool kStash = lds_stash_for(SCENE_IN_LDS, BLOCK_THREADS, FEAT);
    S.wk = nullptr; S.wk_stride = BLOCK_THREADS;
    if constexpr (has_walk_area(FEAT))
        S.wk = (void *)(reinterpret_cast<float *>(lds_blob + stash_base4) + (kStash ? stash_slots_for(FEAT, BLOCK_THREADS) * BLOCK_THREADS : 0u) + threadIdx.x);
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;                              // (after the staging barrier) as do_tile's !active lanes: not part of any wave vote
    const V3 o = v3(orig[(size_t)i * 3], orig[(size_t)i * 3 + 1], orig[(size_t)i * 3 + 2]);
    const V3 d = v3(dir[(size_t)i * 3], dir[(size_t)i * 3 + 1], dir[(size_t)i * 3 + 2]);
    u32 r[MRT_TRACE_WORDS];
    rayq_body<FEAT>(S, o, d, r);
    for (u32 k = 0; k < MRT_TRACE_WORDS; ++k) out[(size_t)i * MRT_TRACE_WORDS + k] = r[k];
}

// element i = thread i of 256-thread workgroups, as in math_selftest (mrt_kernels.hip): lane i % 64 of wavefront i / 64, and the
// lanes behind n leave before any wave vote
__global__ void __launch_bounds__(256) math_selftest_ext(int op, const float *__restrict__ a, const float *__restrict__ b,
                                                         float *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = a[i], y = b ? b[i] : 0.0f;
    float q0, q1, r = 0.0f;
    switch (op) {
    case 16: r = 0.5f + div_(0.5f * atan2_(x, -y), kPi); break;                   // hit_uv's sphere branch, env_uv: u
    case 17: r = div_(acos_(fmin_(fmax_(x, -1.0f), 1.0f)), kPi); break;           // env_uv, latlong: v
    case 18: div2_(x, y, x + y, q0, q1); r = q0; break;
    case 19: div2_(x, y, x + y, q0, q1); r = q1; break;
    default: break;
    }
    out[i] = r;
}

// ---- launchers (declared in mrt_kernels.h) ----
hipError_t launch_math_selftest_ext(int op, const float *a, const float *b, float *out, size_t n, hipStream_t stream)
{
    hipLaunchKernelGGL(math_selftest_ext, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, op, a, b, out, n);
    return hipGetLastError();
}

hipError_t launch_rayq(const Params &P, bool scene_in_lds, u32 inst, size_t lds, u32 n, const float *orig, const float *dir, u32 *out, hipStream_t stream)
{
    const dim3 grid((n + 255u) / 256u);
#define MRT_RQ(L, F) \
    if (scene_in_lds == (L) && inst == (u32)(F)) { \
        if (L) { \
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&rayq<L, (F)>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) return e; \
        } \
        hipLaunchKernelGGL((rayq<L, (F)>), grid, dim3(256), lds, stream, P, P.blob, n, orig, dir, out); \
        return hipGetLastError(); \
    }
    MRT_RAYQ_LIST
#undef MRT_RQ
    return hipErrorInvalidConfiguration;
}

bool rayq_has(bool scene_in_lds, u32 inst)
{
#define MRT_RQ(L, F) if (scene_in_lds == (L) && inst == (u32)(F)) return true;
    MRT_RAYQ_LIST
#undef MRT_RQ
    return false;
}

}  // namespace mrt

// ---- mrt_selftest_instantiations (include/mrt.h): host only, no device ----
// The rows are the expansion of the MRT_SHAPES_* lists of mrt_megakernel.h, the text launch_pt_inst (mrt_pt_kernel.h) dispatches
// over: one row per (block_threads, scene_in_lds, FEAT) that exists as pt_megakernel<.., F> and pt_megakernel<.., F, TileList>.
extern "C" uint32_t mrt_selftest_instantiations(uint32_t *threads, uint32_t *scene_in_lds, uint32_t *feat, uint32_t cap)
{
    using namespace mrt;
    uint32_t n = 0;
    auto row = [&](u32 t, u32 l, u32 f) {
        if (n < cap) {
            if (threads) threads[n] = t;
            if (scene_in_lds) scene_in_lds[n] = l;
            if (feat) feat[n] = f;
        }
        ++n;
    };
#define MRT_CASE(T, F) row((T), 1u, (u32)(F));
#define MRT_CASE_L2(F) row(256u, 0u, (u32)(F));
    MRT_SHAPES_64 MRT_SHAPES_256 MRT_SHAPES_512 MRT_SHAPES_1024 MRT_SHAPES_L2
#undef MRT_CASE
#undef MRT_CASE_L2
    return n;
}
