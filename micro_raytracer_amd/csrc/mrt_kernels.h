// mrt_kernels.h — host-callable launchers of the kernels in mrt_kernels.hip.
#pragma once
#include <hip/hip_runtime_api.h>

#include "mrt_adapt.h"     // MeanSrc: the means the image, denoiser and float-image launchers read
#include "mrt_inst.h"      // pt_instantiation: FEAT template argument of the kernel launch_pt picks; pt_lds_bytes
#include "mrt_scene.h"

namespace mrt {

// One axis of a resample on the device: per output index its first source index and tap count, `cap` weights each
// (mrt_pack.h ResampleTaps, uploaded)
struct DevTaps {
    const u32 *left, *count;
    const float *weight;
    u32 cap;
};

hipError_t configure_pt(size_t max_lds_bytes);
hipError_t launch_pt(const Params &P, u32 block_threads, bool scene_in_lds, u32 features, hipStream_t stream, const TileList *list = nullptr);
// mrt_adapt.hip: the tile-list instantiations (launch_pt with a list), their LDS attributes (configure_pt)
hipError_t launch_pt_list(const Params &P, const TileList &TL, dim3 grid, size_t lds, u32 block_threads, bool scene_in_lds, u32 inst, hipStream_t stream);
hipError_t configure_pt_list(size_t max_lds_bytes);
hipError_t launch_reduce_chunks(float *accum, const float *partial, size_t n_words, size_t stride, u32 n_chunks, hipStream_t stream);
hipError_t launch_reduce_chunks_listed(float *accum, float *half, const float *partial, const u32 *list, u32 n_listed, u32 nw, u32 nh,
                                       size_t stride, u32 n_chunks, hipStream_t stream);
hipError_t launch_adapt_eval(const float *accum, const float *half, const u32 *list, u32 n_listed, u32 nw, u32 nh, u32 n, float threshold, bool last,
                             u32 *keep, u32 *tile_count, u32 *tile_conv, u32 *list_out, u32 *n_out, hipStream_t stream);
// mrt_denoise.hip: first-hit AOVs (guide [2][nh][nw] float4, albedo [nh][nw][3], ids [nh][nw][2]) and the a-trous passes
hipError_t launch_aov(const Params &P, u32 features, float *guide, float *albedo, i32 *ids, hipStream_t stream);
// ... the same planes of caller-supplied rays (orig, dir: [nh][nw][3] on the device; mrt_aov_rays)
hipError_t launch_aov_rays(const Params &P, u32 features, const float *orig, const float *dir, float *guide, float *albedo, i32 *ids, hipStream_t stream);
hipError_t launch_denoise(const MeanSrc &S, const float *guide, const float *albedo, u32 nh, u32 passes,
                          float sc, float sn, float sp, float *e0, float *e1, float *out, hipStream_t stream, bool env = false,    // env: the context has an environment texture
                          bool wrap_x = false);                                                                                    // wrap_x: the frame is periodic in x
// mrt_denoise_var.hip: the variance-guided mode, passes >= 1; half: the adaptive half buffer, S.tile_count not null
hipError_t launch_denoise_var(const MeanSrc &S, const float *half, const float *guide, const float *albedo, u32 nh, u32 passes,
                              float sv, float sn, float sp, float firefly, float *e0, float *e1, float *out, hipStream_t stream, bool env);
hipError_t launch_scatter_rows(float *frame, const float *gathered, const u32 *rowmap, u32 n_rows, u32 row_words, hipStream_t stream);
// the tone map of the means of S [nh][S.nw][3]: tonemap_u8, or tonemap_tiles_u8 when S has per-tile counts
hipError_t launch_tonemap(const MeanSrc &S, unsigned char *out, u32 nh, float gamma, float wexp, hipStream_t stream);
hipError_t launch_lanczos_v(const unsigned char *src, float *dst, u32 sw, u32 dh, const DevTaps &v, hipStream_t stream);
hipError_t launch_lanczos_h(const float *src, unsigned char *dst, u32 sw, u32 dw, u32 dh, const DevTaps &h, hipStream_t stream);
// mrt_hdr.hip: the linear float image (mrt_img_hdr): the means of S [.][S.nw][3] through the vertical pass into dst [dh][S.nw][3],
// that through the horizontal pass and the clamp at 0 into dst [dh][dw][3]; without a resize the clamped means [nh][S.nw][3]
hipError_t launch_hdr_v(const MeanSrc &S, float *dst, u32 dh, const DevTaps &v, hipStream_t stream);
hipError_t launch_hdr_h(const float *src, float *dst, u32 sw, u32 dw, u32 dh, const DevTaps &h, hipStream_t stream);
hipError_t launch_hdr_copy(const MeanSrc &S, float *dst, u32 nh, hipStream_t stream);
// mrt_rayq.hip: the ray-query test hook (mrt_selftest_trace), instantiation `inst` at 256 threads with `lds` bytes of LDS; n rays,
// out [n][MRT_TRACE_WORDS].  rayq_has: that instantiation exists
hipError_t launch_rayq(const Params &P, bool scene_in_lds, u32 inst, size_t lds, u32 n, const float *orig, const float *dir, u32 *out, hipStream_t stream);
bool rayq_has(bool scene_in_lds, u32 inst);
// mrt_rays.hip: mrt_radiance's kernel pt_rays<scene_in_lds, inst> on n rays (inst: pt_instantiation(256, false, features)), adding
// into P.accum [n][3]; the LDS bytes a workgroup of it takes; mrt_camera_rays' kernel (either output may be null)
hipError_t launch_rays(const Params &P, bool scene_in_lds, u32 inst, u32 n, const float *orig, const float *dir, const u32 *key, hipStream_t stream);
size_t rays_lds_bytes(const Params &P, bool scene_in_lds, u32 inst);
hipError_t launch_camera_rays(const Params &P, float *orig, float *dir, hipStream_t stream);
hipError_t launch_math_selftest(int op, const float *a, const float *b, float *out, size_t n, hipStream_t stream);
// ops 16..19 of mrt_selftest_math, in the test hook's translation unit (mrt_rayq.hip)
hipError_t launch_math_selftest_ext(int op, const float *a, const float *b, float *out, size_t n, hipStream_t stream);
hipError_t launch_math_sweep(int op, unsigned long long first, unsigned long long n, u32 seed, unsigned long long *mismatches, float *example, hipStream_t stream);

}  // namespace mrt
