// mrt_hdr.hip — gfx950 kernels of the linear float image (mrt_img_hdr), in a translation unit of their own: the
// path-tracing kernels and the u8 image path of mrt_kernels.hip are compiled exactly as without it.
//
//   hdr_v<R>    vertical pass on the means formed on the fly from the sums: thread = one element (x * 3 + c) of R consecutive
//               output rows, lanes along the row (coalesced f32 reads and writes)
//   hdr_h       horizontal pass, clamp at 0: thread = one output pixel, as lanczos3_h
//   hdr_copy    no resize: the clamped means
#include <hip/hip_runtime.h>

#include "mrt_hdr.h"
#include "mrt_kernels.h"

namespace mrt {

// Output rows per thread of the vertical pass.  Four rows at ssaa 2 span 18 source rows where four threads of one row each read
// 48: 30 % faster than one row per thread on Lanczos3, 9 % on the box (DESIGN.md §19 has both times).
constexpr u32 kHdrRows = 4;

template <u32 R>
__global__ void __launch_bounds__(256) hdr_v(MeanSrc S, float *__restrict__ dst, u32 dh, const u32 *__restrict__ left, const u32 *__restrict__ count,
                                             const float *__restrict__ weight, u32 cap)
{
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 oy0 = blockIdx.y * R;
    const u32 row = S.nw * 3u;
    if (e >= row || oy0 >= dh) return;
    float t[R];
    hdr_vertical<R>(S, e, oy0, dh, left, count, weight, cap, t);
#pragma unroll
    for (u32 r = 0; r < R; ++r) if (oy0 + r < dh) dst[(size_t)(oy0 + r) * row + e] = t[r];
}

__global__ void __launch_bounds__(256) hdr_h(const float *__restrict__ src, float *__restrict__ dst, u32 sw, u32 dw, u32 dh,
                                             const u32 *__restrict__ left, const u32 *__restrict__ count, const float *__restrict__ weight, u32 cap)
{
    const u32 ox = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 y = blockIdx.y;
    if (ox >= dw || y >= dh) return;
    float o[3];
    hdr_horizontal(src + (size_t)y * sw * 3u, left[ox], count[ox], weight + (size_t)ox * cap, o);
    float *q = dst + ((size_t)y * dw + ox) * 3u;
    q[0] = o[0]; q[1] = o[1]; q[2] = o[2];
}

__global__ void __launch_bounds__(256) hdr_copy(MeanSrc S, float *__restrict__ dst, u32 nh)
{
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 y = blockIdx.y;
    if (e >= S.nw * 3u || y >= nh) return;
    dst[(size_t)y * S.nw * 3u + e] = hdr_clamp(hdr_mean(S, y, e));
}

// ---- launchers (declared in mrt_kernels.h) ----
hipError_t launch_hdr_v(const MeanSrc &S, float *dst, u32 dh, const DevTaps &v, hipStream_t stream)
{
    hipLaunchKernelGGL((hdr_v<kHdrRows>), dim3((S.nw * 3u + 255u) / 256u, (dh + kHdrRows - 1u) / kHdrRows), dim3(256), 0, stream, S, dst, dh, v.left,
                       v.count, v.weight, v.cap);
    return hipGetLastError();
}

hipError_t launch_hdr_h(const float *src, float *dst, u32 sw, u32 dw, u32 dh, const DevTaps &h, hipStream_t stream)
{
    hipLaunchKernelGGL(hdr_h, dim3((dw + 255u) / 256u, dh), dim3(256), 0, stream, src, dst, sw, dw, dh, h.left, h.count, h.weight, h.cap);
    return hipGetLastError();
}

hipError_t launch_hdr_copy(const MeanSrc &S, float *dst, u32 nh, hipStream_t stream)
{
    hipLaunchKernelGGL(hdr_copy, dim3((S.nw * 3u + 255u) / 256u, nh), dim3(256), 0, stream, S, dst, nh);
    return hipGetLastError();
}

}  // namespace mrt
