// mrt_rays_adapt.h — per-lane body and launchers of mrt_radiance_adaptive: the path tracer on caller-supplied
// rays over a list of 8x8 tiles of an [nh][nw] ray grid, one wavefront per (listed tile, chunk phase).  Shared by the kernels of
// mrt_rays_adapt.hip and an x86 build (tests/emu/rays_adapt_probe.cpp), so that both run the same text.  A header of its own: no
// text another kernel source reads changes with it.
#pragma once
#include "mrt_rays.h"

namespace mrt {

// Lane `lane` of the wavefront that serves 8x8 tile `tile` of an nw x nh grid (the layout of listed_pixel, mrt_adapt.hip: lane =
// 8 * row + column of the tile) -> its pixel index p = y * nw + x; false for a lane outside the frame
MRT_HD bool rays_tile_pixel(u32 tile, u32 lane, u32 nw, u32 nh, u32 &p)
{
    const u32 n_tx = (nw + 7u) >> 3;
    const u32 ty = tile / n_tx, tx = tile - ty * n_tx;
    const u32 x = tx * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);
    p = y * nw + x;
    return x < nw && y < nh;
}

// Chunks phase, phase + P.k_split, ... of samples [P.sample_base, + P.n_samples) of pixel p on its supplied ray (o, d): render_pixel
// under the SuppliedRay policy with the pixel index as the hash key.  P.k_split == 1: the chunk sums are added in chunk order to
// P.accum[3 p ..], which holds the earlier rounds' sums; P.k_split >= 2: chunk sum j goes to P.partial[j * P.partial_stride + 3 p ..]
// and the listed reduction folds the planes.  A phase past the launch's chunk count traces nothing.
template <u32 FEAT>
MRT_HD void rays_tile_body(const Scn &S, u32 p, u32 phase, V3 o, V3 d, u32 &segments)
{
    RegStash st;
    LaneJob job;
    job.k = phase;
    job.word = p * 3u;                       // < 2^32: the accumulator of an [nh][nw] frame is addressed in u32 words everywhere
    const SuppliedRay pr = {o, d, p};
    render_pixel<FEAT>(S, st, 0u, 0u, job, segments, nullptr, pr);
}

#if defined(__HIPCC__) || defined(__HIP__)
// mrt_rays_adapt.hip: pt_rays_tiles<scene_in_lds, inst> (inst: pt_instantiation(256, false, features)) over the listed tiles of the
// P.nw x P.nh grid whose rays are orig, dir [nh][nw][3] on the device, P.k_split wavefronts per tile; its LDS bytes are
// rays_lds_bytes' (mrt_kernels.h)
hipError_t launch_rays_tiles(const Params &P, bool scene_in_lds, u32 inst, const TileList &tl, const float *orig, const float *dir, hipStream_t stream);
#endif

}  // namespace mrt
