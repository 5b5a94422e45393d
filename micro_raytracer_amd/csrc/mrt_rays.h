// mrt_rays.h — per-ray bodies of mrt_radiance and mrt_camera_rays: the path tracer on a caller-supplied primary
// ray, and the lens-centre camera ray of a supersampled pixel.  Shared by the kernels of mrt_rays.hip and an x86 build
// (tests/emu/rays_probe.cpp), so that both run the same text.
#pragma once
#include "../../include/mrt.h"
#include "mrt_trace.h"

namespace mrt {

// Samples [P.sample_base, + P.n_samples) of ray i: render_pixel under the SuppliedRay policy, one lane per ray (k_split == 1, no
// planes), the chunk sums added in chunk order to P.accum[3 i ..], which the caller zeroed.  key: what stands in the pixel
// index's place in the hash key.
template <u32 FEAT>
MRT_HD void rays_body(const Scn &S, u32 i, V3 o, V3 d, u32 key, u32 &segments)
{
    RegStash st;
    LaneJob job;
    job.k = 0u;
    job.word = i * 3u;                       // < 2^32: mrt_radiance limits a call to 2^30 - 1 rays
    const SuppliedRay pr = {o, d, key};
    render_pixel<FEAT>(S, st, 0u, 0u, job, segments, nullptr, pr);
}

// The ray camera_ray_centre forms for supersampled pixel (x, y): the ray of the depth AOV (aov_pixel, mrt_denoise.h) and, with
// aprt == 0, of every sample of the pixel.  F: the packed scene (the camera matrices live there)
MRT_HD void camera_ray_of(const Params &P, const float *F, u32 x, u32 y, V3 &o, V3 &d)
{
    camera_ray_centre(P, F + P.off_cam, pixel_focus(P, (float)x, (float)y), o, d);
}

// The feature sets of pt_rays (MRT_RAYS(F) is defined at each use): those of the scene-through-L2 path-tracing kernels
// (MRT_SHAPES_L2 of mrt_megakernel.h), picked by pt_instantiation(256, false, features) as launch_aov picks its own
#define MRT_RAYS_LIST \
    MRT_RAYS(F_ALL & ~F_TRI) MRT_RAYS(F_ALL) MRT_RAYS((F_ALL & ~F_TRI) | F_BVH) MRT_RAYS(F_ALL | F_BVH) \
    MRT_RAYS(F_ALL | F_VATTR) MRT_RAYS(F_ALL | F_BVH | F_VATTR) MRT_RAYS(F_ALL | F_VATTR | F_ENV) MRT_RAYS(F_ALL | F_BVH | F_VATTR | F_ENV)

}  // namespace mrt
