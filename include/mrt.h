/*
 * mrt.h — C ABI of libmrt_hip.so, the MI355X (gfx950) path-tracing backend that replaces the
 * thread-pool sampler of micro-raytracer.
 *
 * Every entry point below names the reference interface it stands in for (paths are relative
 * to the reference checkout, file:line).  The boundary is the reference's `Sampler`
 * (src/sampler.rs:11-100): `Sampler::new`, `Sampler::execute`, `Sampler::img`, and the two
 * callers `CLI::raytrace` (src/cli.rs:155-177) and `HttpServer::raytrace` (src/http.rs:136-148).
 *
 * Plain C: pointers + sizes only, no C++/torch types.  All floating point data is IEEE f32.
 * Descriptor pointers are borrowed for the duration of mrt_create only (the library deep-copies
 * into its own packed device layout); output buffers are caller-allocated.
 *
 * Threading: one mrt_ctx has a single owner at a time (like `&mut self` on Sampler); different
 * contexts may be used concurrently from different threads (HttpServer spawns one Sampler per
 * connection, src/http.rs:138,155).  mrt_last_error() is thread-local.
 */
#ifndef MRT_H
#define MRT_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRT_ABI_VERSION 3u

/* ---- error codes (reference: Result<_, String> everywhere, src/sampler.rs:80, src/cli.rs:155) ---- */
#define MRT_OK            0
#define MRT_ERR_ARG      -1   /* null / malformed argument                                   */
#define MRT_ERR_SCENE    -2   /* scene rejected: something the reference would panic on       */
#define MRT_ERR_DEVICE   -3   /* HIP / RCCL runtime failure                                   */
#define MRT_ERR_LIMIT    -4   /* scene exceeds a device-side capacity                         */
#define MRT_ERR_STATE    -5   /* call not valid in this state (e.g. img before any sample)    */

/* ---- scene description: flattened rt::Render (src/rt.rs:10-190) ------------------------------ */

/* rt::Camera, src/rt.rs:64-72.  dir is Vec4f in (w,x,y,z) order as in src/lin.rs:18-25. */
typedef struct mrt_camera {
    float pos[3];
    float dir[4];
    float fov, gamma, exp, aprt, foc;
} mrt_camera;

/* rt::Frame, src/rt.rs:75-79. */
typedef struct mrt_frame {
    uint16_t res_w, res_h;
    float ssaa;
    mrt_camera cam;
} mrt_frame;

/* rt::RayTracer, src/rt.rs:17-22 (`sampler: Uniform<f32>` is replaced by mrt_opts.seed). */
typedef struct mrt_rt {
    uint32_t bounce;
    uint32_t sample;   /* informational: the caller owns the sample loop (src/cli.rs:162) */
    float loss;
} mrt_rt;

/* rt::Texture, src/rt.rs:82-86: w*h texels of f32 RGB; dat may be NULL (`dat: None` => black). */
typedef struct mrt_texture {
    uint32_t w, h;
    const float *dat;
} mrt_texture;

/* rt::Material, src/rt.rs:89-103.  Map slots index mrt_scene.textures, -1 = None.
 * Slot order: tex, rmap, mmap, gmap, omap, emap. */
typedef struct mrt_material {
    float albedo[3];
    float rough, metal, glass, opacity, emit;
    int32_t tex, rmap, mmap, gmap, omap, emap;
} mrt_material;

/* rt::RendererInstance, src/rt.rs:147-150. */
typedef struct mrt_instance {
    float pos[3];
    float dir[4];
} mrt_instance;

/* rt::RendererKind, src/rt.rs:138-144. */
#define MRT_KIND_SPHERE   0u   /* param[0] = r                                  */
#define MRT_KIND_PLANE    1u   /* param[0..3) = n                               */
#define MRT_KIND_BOX      2u   /* param[0..3) = sizes                           */
#define MRT_KIND_TRIANGLE 3u   /* param[0..9) = vtx0, vtx1, vtx2                */
#define MRT_KIND_MESH     4u   /* tris -> n_tris * 9 floats (vtx0, vtx1, vtx2)  */

/* rt::Renderer, src/rt.rs:153-158.  The instance list is the one the reference's loader
 * produces (src/parser.rs:838-864); its order is significant (first-minimum tie rule,
 * src/rt.rs:872).  For meshes the library rebuilds the reference's depth-3 octree
 * (src/rt.rs:630-703, called from src/parser.rs:815-816) from the raw triangles. */
typedef struct mrt_renderer {
    uint32_t kind;
    float param[9];
    const float *tris;
    uint32_t n_tris;
    mrt_material mat;
    const mrt_instance *inst;
    uint32_t n_inst;
} mrt_renderer;

/* rt::Light / LightKind, src/rt.rs:161-175. */
#define MRT_LIGHT_POINT 0u   /* v = pos */
#define MRT_LIGHT_DIR   1u   /* v = dir */
typedef struct mrt_light {
    uint32_t kind;
    float v[3];
    float pwr;
    float color[3];
} mrt_light;

/* rt::Sky, src/rt.rs:178-181. */
typedef struct mrt_sky {
    float color[3];
    float pwr;
} mrt_sky;

/* rt::Scene, src/rt.rs:184-190 (`renderer_bvh` is always None in the reference, src/parser.rs:922). */
typedef struct mrt_scene {
    const mrt_renderer *renderer;
    uint32_t n_renderer;
    const mrt_light *light;
    uint32_t n_light;
    mrt_sky sky;
    const mrt_texture *textures;
    uint32_t n_textures;
} mrt_scene;

/* rt::Render, src/rt.rs:10-14. */
typedef struct mrt_render_desc {
    mrt_rt rt;
    mrt_frame frame;
    mrt_scene scene;
} mrt_render_desc;

/* ---- options: what Sampler::new(workers, n_dim) (src/sampler.rs:19) turns into ---------------- */
typedef struct mrt_opts {
    uint32_t abi_version;   /* MRT_ABI_VERSION */
    uint64_t seed;          /* the reference is unseeded (rand::thread_rng, src/rt.rs:564..1054);
                               here the result is a pure function of (desc, seed, sample index)   */
    int32_t  device;        /* HIP device ordinal for this context; -1 = current device           */
    /* Row sharding (replaces the n_dim x n_dim tile jobs of src/sampler.rs:40-41): supersampled
     * rows are dealt in blocks of shard_rows rows, block b belongs to shard (b % shard_count).
     * shard_count = 0 or 1 => this context renders the whole frame.
     * The layout (csrc/mrt_shard.h, computed in 64 bits for every 32-bit input): the effective shard_rows is
     * min(shard_rows, nh) -- a block taller than the frame owns the same rows as a block of nh rows, so every row
     * goes to shard 0 and nobody allocates for rows that do not exist;
     * padded_rows = ceil(ceil(nh / rows) / shard_count) * rows with the effective rows, or nh when shard_count == 1.
     * Hence local_rows <= padded_rows < 2 * nh; mrt_create checks the first before it allocates (MRT_ERR_ARG). */
    uint32_t shard_index;
    uint32_t shard_count;   /* 0 => 1 */
    uint32_t shard_rows;    /* 0 => default (8); values above nh are taken as nh */
    /* In-process multi-GPU (the single-process reference binary): n_devices > 1 makes one
     * sub-context per device 0..n_devices-1, row-sharded as above, gathered on device 0 by one
     * RCCL ncclGather per mrt_execute (librccl.so is loaded on demand).  Mutually exclusive with
     * shard_count > 1.  n_devices == 0 takes the count from the environment variable MRT_GPUS. */
    uint32_t n_devices;
    uint32_t flags;         /* MRT_FLAG_* */
    uint32_t reserved[4];
} mrt_opts;

#define MRT_FLAG_COUNT_SEGMENTS 1u   /* keep the per-launch path-segment counter (mrt_stats.segments): one wave reduction and
                                        one atomic per wavefront, a read-back when mrt_get_stats is called.  Implies
                                        MRT_FLAG_NO_LOOKAHEAD: a look-ahead launch traces samples of later calls, so no call could
                                        report its own segments */
#define MRT_FLAG_NO_EVENT_TIMING 2u  /* no HIP events around the kernels (mrt_stats.kernel_ms / reduce_ms stay 0): what a caller that
                                        runs one sample per call (src/cli.rs:162-170) and never asks for stats wants */
#define MRT_FLAG_NO_LOOKAHEAD 8u     /* one-sample mrt_execute calls always run their own one-sample launch.  Default: a context that
                                        sees one-sample calls arrive back to back traces the NEXT samples ahead on a second stream
                                        (2, 4, ... 32 per launch, each into a plane of its own) and a call only folds its sample into
                                        the accumulator and waits for that: same samples, added in the same order -- bit for bit the
                                        plain loop -- at the rate of batched launches; MRT_LOOKAHEAD=0 in the environment switches it
                                        off too, MRT_LOOKAHEAD=n sets the samples per launch.  Tracing ahead starts with the third
                                        consecutive one-sample call; what was traced ahead is dropped by an mrt_execute of another size,
                                        mrt_reset, mrt_set_accum*, mrt_execute_adaptive, and by nothing else: an observation, mrt_bind_accum
                                        or mrt_accum_device_ptr in the middle of a run leaves it running */
#define MRT_FLAG_DEFER 4u            /* mrt_execute only books its samples; they are traced, batched, when 1024 are booked or when
                                        the accumulator is observed or replaced (mrt_accum*, mrt_img*, mrt_set_accum*, mrt_get_stats,
                                        mrt_bind_accum).  Same samples, same image as eager execution (sums re-associated like any
                                        batched call); the Duration of a booking call is ~0.  Also set by the environment variable
                                        MRT_DEFER=1 (a non-zero number; "0" or empty is off) for unmodified callers.  Ignored while the accumulator's device memory is
                                        visible to the caller (mrt_bind_accum / mrt_accum_device_ptr).
                                        What is booked is never cut: the call that brings it to 1024 or more has ALL of it traced, its own
                                        samples included, as one launch over [count, count + booked) (1020 booked and a call of 100: one
                                        launch of 1120), and so has an observation.  An entry point of the list above traces what is booked
                                        before it checks anything else, so one that then refuses (mrt_img on a shard, an undersized
                                        mrt_bind_accum) has traced it all the same; mrt_execute_adaptive and mrt_adapt_half are not on the
                                        list and trace nothing; mrt_reset drops what is booked. */

typedef struct mrt_ctx mrt_ctx;

/* Counters of the most recent mrt_execute (reference: the Duration returned by
 * Sampler::execute, src/sampler.rs:35,77, logged at src/cli.rs:164). */
typedef struct mrt_stats {
    double   kernel_ms;      /* HIP-event time of the path-tracing kernel of the last execute    */
    double   gather_ms;      /* time of the multi-GPU gather (0 on one device)                   */
    uint64_t samples;        /* path samples traced by the last execute on this context: of the launch that traced booked samples
                                (MRT_FLAG_DEFER) all of them; mrt_reset and mrt_set_accum* leave the counters as they are */
    uint64_t segments;       /* path segments (closest-hit queries) of the last execute          */
    uint32_t launches;       /* kernel launches of the last execute                              */
    uint32_t lds_bytes;      /* LDS bytes per workgroup of the path-tracing kernel               */
    uint32_t block_threads;  /* workgroup size                                                   */
    uint32_t scene_bytes;    /* packed scene bytes staged per workgroup                          */
    uint32_t k_split;        /* lanes per pixel of the last execute (sample chunks dealt round-robin) */
    uint32_t deferred;       /* 1 when the last mrt_execute was booked under MRT_FLAG_DEFER / MRT_DEFER=1, 0 when it ran at once
                                (no deferral asked for, or the accumulator's device memory is visible to the caller) */
    double   img_ms;         /* HIP-event time of the kernels of the last mrt_img / mrt_img_ss (tone map + resize) */
    double   reduce_ms;      /* HIP-event time of reduce_chunks after the path-tracing kernel (0 when k_split == 1) */
    uint32_t kernel_features; /* which instantiation of the path-tracing kernel serves this context: its FEAT template argument
                                 (csrc/mrt_scene.h F_* bits), i.e. pt_megakernel<scene_in_lds, block_threads, kernel_features> */
    uint32_t scene_in_lds;   /* 1: every workgroup stages the packed scene in LDS; 0: it is read through L2 */
} mrt_stats;

/* Sampler::new + the first half of Sampler::execute's argument list (src/sampler.rs:19,28):
 * validates and flattens the scene, uploads it, allocates the accumulators.
 * Returns NULL on failure (see mrt_last_error / mrt_last_status). */
mrt_ctx *mrt_create(const mrt_render_desc *desc, const mrt_opts *opts);

/* Drop for Sampler. */
void mrt_destroy(mrt_ctx *ctx);

/* n_samples consecutive Sampler::execute calls (src/sampler.rs:28-78): every supersampled pixel
 * of this context's rows gets n_samples more path samples added to its accumulator and
 * last_count += n_samples.  Synchronous (like the scoped-pool join, src/sampler.rs:39-74).
 * *seconds (optional) receives the wall time, the Duration of src/sampler.rs:77. */
int mrt_execute(mrt_ctx *ctx, uint32_t n_samples, double *seconds);

/* Supersampled frame size: nw, nh of src/sampler.rs:29-30; local_rows = rows owned by this shard. */
int mrt_dims(const mrt_ctx *ctx, uint32_t *nw, uint32_t *nh, uint32_t *local_rows);

/* Sampler.colors / Sampler.last_count (src/sampler.rs:14-15): the full-frame sum of per-sample
 * radiance, rgb[nh][nw][3] f32 (rows not owned by this shard are left untouched), and the
 * number of samples accumulated so far. Either pointer may be NULL. */
int mrt_accum(mrt_ctx *ctx, float *rgb, uint32_t *count);

/* Shard-local view of the same data: rows[local_rows] = global row index of each local row;
 * rgb[local_rows][nw][3].  Either pointer may be NULL. */
int mrt_accum_local(mrt_ctx *ctx, float *rgb, uint32_t *rows);

/* Device pointer of the shard-local accumulator ([local_rows][nw][3] f32) for zero-copy
 * hand-off to a collective (one RCCL gather of these per mrt_execute batch). */
int mrt_accum_device_ptr(mrt_ctx *ctx, void **dev_ptr, size_t *bytes);

/* Rows the shard-local accumulator is allocated for: the largest local_rows over all shards of this
 * shard_count (so that equal-sized buffers can be gathered); rows past local_rows stay zero. */
int mrt_padded_rows(const mrt_ctx *ctx, uint32_t *rows);

/* Use caller-owned device memory (e.g. a torch tensor) of at least padded_rows * nw * 3 floats as the
 * shard-local accumulator from now on; current contents are copied over.  The buffer must outlive the
 * context or a later mrt_bind_accum(ctx, NULL, 0), which switches back to library-owned memory. */
int mrt_bind_accum(mrt_ctx *ctx, void *dev_ptr, size_t bytes);

/* mrt_set_accum from device memory on this context's device (e.g. the frame assembled from a gather). */
int mrt_set_accum_device(mrt_ctx *ctx, const void *dev_rgb, uint32_t count);

/* Replace the accumulator contents with a full frame (rgb[nh][nw][3]) and sample count,
 * e.g. on rank 0 after a gather, or to resume (the reference never persists `colors`).
 * A sharded context (shard_count > 1) keeps the frame and its count NEXT TO its own rows: mrt_accum, mrt_sample_counts, mrt_img*,
 * mrt_img_hdr and mrt_denoise read that frame until mrt_reset or the next mrt_set_accum*, while mrt_execute, mrt_accum_local and
 * the device pointer go on with the shard's own rows and their own count, which the call does not touch. */
int mrt_set_accum(mrt_ctx *ctx, const float *rgb, uint32_t count);

/* Sampler::img (src/sampler.rs:80-99): mean, gamma, extended Reinhard, u8 truncation, then the
 * `image` crate's Lanczos3 resize nw x nh -> res_w x res_h.  rgb8[res_h][res_w][3].
 * Needs the whole frame in this context (shard_count <= 1, or after mrt_set_accum). */
int mrt_img(mrt_ctx *ctx, uint8_t *rgb8);

/* The tone-mapped supersampled image before the resize: rgb8[nh][nw][3] (src/sampler.rs:84-96). */
int mrt_img_ss(mrt_ctx *ctx, uint8_t *rgb8);

/* `img.save(&filename)` of the reference's CLI (src/cli.rs:168,174) for the lossless formats it is used with:
 * ".ppm" (P6) and ".png" (8-bit RGB, stored deflate).  Host-only helper; returns MRT_ERR_ARG for other extensions. */
int mrt_save_image(const char *path, const uint8_t *rgb8, uint32_t w, uint32_t h);

/* Zero the accumulators and last_count (a fresh Sampler on the same scene). */
int mrt_reset(mrt_ctx *ctx);

/* Counters of the last execute.  Not const: under deferred execution this is an observation (booked samples are traced
 * first), and the HIP-event times / the segment counter are read back here, lazily. */
int mrt_get_stats(mrt_ctx *ctx, mrt_stats *out);

/* Result<_, String>'s message for the calling thread's last failed call ("" if none). */
const char *mrt_last_error(void);
int mrt_last_status(void);

uint32_t mrt_abi_version(void);

/* Number of HIP devices visible (0 if none); never initialises more than the runtime. */
int mrt_device_count(void);

/* ---- adaptive sampling: a per-tile noise threshold (not in the reference) ---------------------
 * Rounds of `step` samples; round r traces the global sample indices [r*step, (r+1)*step) of every pixel of the tiles still
 * running (a tile = 8x8 pixels of the supersampled frame, x/8, y/8; edge tiles hold only their in-frame pixels).  Every tile
 * runs until min_samples; from then on the tiles are evaluated after every second round (n = min_samples, min_samples + 2*step,
 * ...) and a tile whose error (csrc/mrt_adapt.h) is <= threshold stops there for good; none goes past max_samples.  Each
 * pixel is the uniform render's estimator at its tile's count: the accumulator bytes of a tile that stopped at n equal those
 * of an n-sample mrt_execute on the same seed.
 * Rules: step a positive multiple of 16; min_samples and max_samples positive multiples of 2*step, min <= max; threshold >= 0
 * (inf: every tile stops at min_samples); otherwise MRT_ERR_ARG. */
typedef struct mrt_adapt {
    uint32_t min_samples, max_samples, step;
    float threshold;
    uint32_t reserved[4];
} mrt_adapt;

typedef struct mrt_adapt_info {
    uint64_t samples;                          /* path samples traced by the call */
    uint32_t rounds, launches, tiles, tiles_converged, min_count, max_count;
    double   kernel_ms;                        /* HIP-event time of the path-tracing launches, summed (0 under MRT_FLAG_NO_EVENT_TIMING) */
} mrt_adapt_info;

/* One adaptive render on a context that holds no samples (fresh, or after mrt_reset; none booked under MRT_FLAG_DEFER), run
 * eagerly.  Sharded and multi-device contexts: MRT_ERR_STATE.  Afterwards mrt_img / mrt_img_ss tone-map each pixel with its
 * tile's 1/count, mrt_accum returns the sums with *count = the smallest per-pixel count, mrt_get_stats describes this call,
 * and mrt_execute returns MRT_ERR_STATE until mrt_reset, mrt_set_accum or mrt_set_accum_device returns the context to uniform
 * sampling.  info and seconds (wall time) may be NULL. */
int mrt_execute_adaptive(mrt_ctx *ctx, const mrt_adapt *a, mrt_adapt_info *info, double *seconds);

/* Samples accumulated per pixel, counts[nh][nw] (a uniform context: its count everywhere). */
int mrt_sample_counts(mrt_ctx *ctx, uint32_t *counts);

/* The half buffer H of the last adaptive call, rgb[nh][nw][3]: per pixel the sum of its even-numbered rounds' samples
 * (count/2 of them).  MRT_ERR_STATE on a context that has run no adaptive call since its last reset. */
int mrt_adapt_half(mrt_ctx *ctx, float *rgb);

/* ---- first-hit AOVs and the a-trous denoiser ---------------------------------------------------------------
 * AOVs: one camera ray per supersampled pixel through the lens centre, its closest hit.  Computed once per context on first
 * use and kept on the device (mrt_reset keeps them: they depend on scene and camera only).  Any output may be NULL:
 *   depth[nh][nw]        distance along the unit ray (+inf: miss)
 *   normal[nh][nw][3]    world-space normal as the path tracer uses it (0: miss)
 *   albedo[nh][nw][3]    material albedo x texture at the hit (miss: 0, or, on a context with an environment texture
 *                        (mrt_env), the sky E(d) the centre ray sees: sky.color x texel)
 *   renderer[nh][nw]     index into mrt_scene.renderer (-1: miss)
 *   instance[nh][nw]     index into that renderer's inst list (-1: miss)
 * Sharded and multi-device contexts return the whole frame too.  Not an observation: booked samples stay booked. */
int mrt_aov(mrt_ctx *ctx, float *depth, float *normal, float *albedo, int32_t *renderer, int32_t *instance);

/* The AOVs of a custom camera: one caller-supplied ray per supersampled pixel, orig and dir [nh][nw][3], in place
 * of the camera's lens-centre ray -- the grid a caller renders through mrt_radiance and puts back with mrt_set_accum.  The call
 * computes the planes at once and installs them as the context's AOVs: from then on mrt_aov and every filter guided by them
 * (mrt_denoise, mrt_img_denoised, mrt_img_hdr with denoise) use them; mrt_reset and mrt_set_accum* keep them.  A ray is traced as
 * given, by the rules of mrt_radiance: no shift of the origin, no normalisation (depth is the ray parameter t0, the world point
 * orig + dir * t0), any float is legal.  A miss under an environment texture has the albedo E(dir) of the supplied direction.
 *   MRT_AOV_RAYS_DEVICE   orig and dir are device pointers on the context's device
 *   MRT_AOV_WRAP_X        the grid is periodic in x (a full 360-degree panorama); kept with the planes: while it is set every
 *                         a-trous pass takes its horizontal taps at (x + s * dx) modulo nw, all 25 taps of a row inside the
 *                         frame count, and the seam is filtered like any other column
 * orig = dir = NULL with flags 0 drops the planes: the next use computes the camera's own again.  Pointers are borrowed for the
 * duration of the call.  Not an observation: the accumulator, the counts, booked samples and the statistics stay as they are.
 * MRT_ERR_ARG: a null context, exactly one of orig and dir NULL, an unknown flag, flags with NULL rays.  MRT_ERR_STATE: a
 * multi-device context; and, while such planes are installed, MRT_DN_VARIANCE in the filters above after mrt_execute_adaptive --
 * that half buffer belongs to the camera's frame.  The half buffer of mrt_radiance_adaptive (below) belongs to its rays: after
 * that call the mode serves with these planes, and only with them.  A row-sharded context takes the whole grid. */
#define MRT_AOV_RAYS_DEVICE 1u
#define MRT_AOV_WRAP_X 2u
int mrt_aov_rays(mrt_ctx *ctx, const float *orig /*[nh][nw][3]*/, const float *dir /*[nh][nw][3]*/, uint32_t flags);

/* Edge-avoiding a-trous filter (Dammertz et al. 2010) on the mean radiance, guided by the AOVs.  passes 0..8 (0: the means
 * unchanged); sigmas > 0 or +inf (+inf switches that term off); NaN or <= 0: MRT_ERR_ARG.  NULL options = the defaults.
 *
 * mode MRT_DN_VARIANCE: the colour term is driven by a per-pixel variance estimate instead of sigma_color (which
 * must still be valid, and is not used).  The estimate comes from the accumulator and the half buffer of an adaptive render, so
 * the mode needs what mrt_adapt_half needs: an mrt_execute_adaptive on this context since its last mrt_reset / mrt_set_accum*,
 * else MRT_ERR_STATE.  A uniform budget of n samples with a half buffer: mrt_execute_adaptive with threshold 0 and
 * min_samples = max_samples = n (the accumulator bytes of an n-sample mrt_execute).
 *   sigma_var   the colour term's width in standard deviations of the pixel's mean; 0: MRT_DN_SIGMA_VAR; > 0 or +inf (off)
 *   firefly     a pixel brighter than firefly x its brightest same-surface neighbour is scaled down to that before the filter;
 *               0: MRT_DN_FIREFLY; > 0; +inf: off
 * NaN or < 0: MRT_ERR_ARG.  In mode MRT_DN_ATROUS both must be 0 (MRT_ERR_ARG); any other mode: MRT_ERR_ARG. */
#define MRT_DENOISE_PASSES 5u
#define MRT_DENOISE_SIGMA_COLOR 0.5f
#define MRT_DENOISE_SIGMA_NORMAL 0.25f
#define MRT_DENOISE_SIGMA_PLANE 0.05f
#define MRT_DN_ATROUS 0u
#define MRT_DN_VARIANCE 1u
#define MRT_DN_SIGMA_VAR 4.5f
#define MRT_DN_FIREFLY 1.0f
typedef struct mrt_denoise_opts {
    uint32_t passes;
    float sigma_color, sigma_normal, sigma_plane;
    uint32_t mode;                 /* MRT_DN_ATROUS (0, the filter as it always was) or MRT_DN_VARIANCE */
    float sigma_var, firefly;      /* MRT_DN_VARIANCE only; 0: the default */
    uint32_t reserved[1];
} mrt_denoise_opts;
typedef struct mrt_denoise_info {
    double aov_ms, filter_ms;      /* HIP-event times of this call's AOV pass (0: the AOVs were cached) and of the filter */
    uint32_t passes, aov_cached;
    uint32_t reserved[2];          /* reserved[0]: the mode that ran (MRT_DN_*) */
} mrt_denoise_info;

/* The filtered means rgb[nh][nw][3].  An observation like mrt_img: booked samples are traced first; needs the whole frame
 * (unsharded, or after mrt_set_accum*) and at least one sample, else MRT_ERR_STATE; after mrt_execute_adaptive each pixel's
 * mean uses its tile's count.  info may be NULL. */
int mrt_denoise(mrt_ctx *ctx, const mrt_denoise_opts *o, float *rgb, mrt_denoise_info *info);

/* mrt_img of the filtered means: rgb8[res_h][res_w][3] (passes = 0: the bytes of mrt_img). */
int mrt_img_denoised(mrt_ctx *ctx, const mrt_denoise_opts *o, uint8_t *rgb8, mrt_denoise_info *info);

/* Test hook, host only (no device needed): what mrt_create would stage in LDS for this scene and the workgroup shape of its
 * launches -- the policy of csrc/mrt_plan.cpp as data, so that it can be checked where no GPU exists. */
typedef struct mrt_plan {
    uint32_t staging;        /* 0 whole scene | 1 warm: texels in global memory (mesh kernels: + a per-lane leaf queue) | 2 deep: only the first
                                tbvh_hot_nodes nodes of the (level-ordered) triangle-BVH table staged, triangles in global
                                memory | 3 none: everything through L2 */
    uint32_t block_threads;  /* workgroup size of the batched launches */
    uint32_t lds_bytes;      /* LDS per workgroup: staged scene + lane stash + walk areas */
    uint32_t staged_bytes;   /* the staged part of the scene */
    uint32_t scene_bytes;    /* the whole packed scene without the octree leaf lists */
    uint32_t kernel_features;/* FEAT template argument of the kernel instantiation (mrt_stats.kernel_features) */
    uint32_t tbvh_nodes;     /* triangle-BVH nodes of all meshes */
    uint32_t tbvh_hot_nodes; /* of which staged (deep level; otherwise all when staged at all) */
    uint32_t small_plain_grid; /* 1: launches of less than one sample chunk take the plain grid instead of the persistent one */
    uint32_t walk_cap;       /* entries of a lane's walk area (node stack + leaf queue of the mesh walk; 0: no mesh walk) */
    uint32_t reserved[2];
} mrt_plan;
int mrt_plan_launch(const mrt_render_desc *desc, mrt_plan *out);

/* ---- per-corner attributes of triangles and meshes (not in the reference) --------------------
 * Optional smooth shading normals and texture coordinates, one entry per corner in the order of the renderer's vertices
 * (a MRT_KIND_TRIANGLE renderer counts as n_tris = 1).  Either pointer may be NULL:
 *   uv[n_tris][3][2]   texture coordinates (finite); the hit's UV is interpolated, wrapped into [0, 1) like a plane's and looked up
 *                      like a plane's (nearest texel, or the scene's filter).  Only a renderer WITH uv may carry texture maps (mrt_material.tex ... emap).
 *   vn[n_tris][3][3]   object-space normals, any length; the shading normal is interpolated and replaces the face normal
 *                      wherever the path tracer uses one (a degenerate triangle or a zero / non-finite result: the face normal).
 * attrs[r] belongs to scene.renderer[r]; n_renderer must equal scene.n_renderer.  Attributes on a sphere, plane or box, or a
 * non-finite uv: MRT_ERR_SCENE.  Borrowed for the duration of the call only, like the descriptor. */
typedef struct mrt_tri_attrs {
    const float *uv;
    const float *vn;
} mrt_tri_attrs;

/* ---- environment texture of the sky (not in the reference) -------------------------------------
 * The texel the direction d of an escaping ray maps to multiplies sky.color, as a material's tex multiplies its albedo:
 * E(d) = sky.color x texel.  A primary miss contributes E(d), a later miss L + T x (E(d) * sky.pwr); a path that runs out of
 * bounces takes the texture's solid-angle-weighted mean in the texel's place.  Nearest texel unless filter asks for the bilinear
 * filter (below); no importance sampling.  Mappings (u is then shifted by rot and wrapped into [0, 1) like a plane's):
 *   MRT_ENV_SPHERE   the sphere renderer's UV of the direction: u = 0.5 + atan2(d.x, -d.y) / 2pi, v = 0.5 - 0.5 d.z
 *   MRT_ENV_LATLONG  equirectangular: the same u, v = acos(d.z) / pi
 * Rejected with MRT_ERR_SCENE: w == 0, h == 0, dat == NULL, a non-finite or negative texel, an unknown mapping, a non-finite rot,
 * an unknown filter; with MRT_ERR_LIMIT: more than 2^25 texels.
 *
 * Texture filters: MRT_FILTER_NEAREST is the lookup described above.  MRT_FILTER_BILINEAR blends the four texels
 * around the coordinate (texel centres at i + 0.5, f32, unfused): u repeats; v repeats too for a material texture on a plane,
 * box, triangle or mesh, and is clamped to the first / last row for the environment (the poles) and for a material texture on
 * a sphere.  A path that runs out of bounces keeps the unfiltered mean.  Selected separately for the environment
 * (mrt_env.filter) and, with one scene-wide switch, for the material textures (mrt_desc_ext.reserved[0]). */
#define MRT_ENV_SPHERE  0u
#define MRT_ENV_LATLONG 1u
#define MRT_FILTER_NEAREST  0u
#define MRT_FILTER_BILINEAR 1u
typedef struct mrt_env {
    mrt_texture tex;        /* w x h f32 RGB texels, row 0 = +z; values finite and >= 0, may exceed 1 (HDR) */
    uint32_t mapping;       /* MRT_ENV_* */
    float rot;              /* turns about +z added to u; finite */
    uint32_t filter;        /* MRT_FILTER_* (the first word of what was reserved[4]: a caller that zeroed it asks for nearest) */
    uint32_t reserved[3];
} mrt_env;

/* attrs == NULL: no attributes, whatever n_renderer says (an ext that only carries env); env == NULL: no environment.
 * reserved[0] is the MRT_FILTER_* of the scene's material textures (mrt_material.tex ... emap of every renderer; another value:
 * MRT_ERR_SCENE); on a scene in which no material has a texture map it changes nothing.  reserved[1] must be 0 (MRT_ERR_ARG). */
typedef struct mrt_desc_ext {
    uint32_t n_renderer;
    const mrt_tri_attrs *attrs;
    const mrt_env *env;
    uint32_t reserved[2];
} mrt_desc_ext;

/* mrt_create / mrt_plan_launch of a scene with attributes, an environment or filtered textures; ext == NULL (or none of them in
 * it): exactly mrt_create / mrt_plan_launch. */
mrt_ctx *mrt_create_ext(const mrt_render_desc *desc, const mrt_opts *opts, const mrt_desc_ext *ext);
int mrt_plan_launch_ext(const mrt_render_desc *desc, const mrt_desc_ext *ext, mrt_plan *out);

/* ---- radiance along caller-supplied rays: custom cameras, probes, baking ----
 * mrt_radiance path-traces ray i (origin orig[i], direction dir[i]) n_samples times, exactly as a frame's pixel is sampled, but
 * for the primary ray: it is traced as given -- no shift of the origin, no normalisation (the shading assumes unit length) -- and
 * the two lens draws are not taken; every later draw sits at its usual slot.  key[i] stands where the frame's pixel index
 * y * nw + x stands in the hash key (pix_key = mix32 of key_i + seed_lo, xor seed_hi), sample s of the ray has the path key of
 * sample s of that pixel.  rgb[i] receives the SUM of the samples in the canonical order: aligned chunks of 16 global sample
 * indices, each summed from 0, the chunk sums added in chunk order to 0.  With sample_base == 0, key == NULL and the rays of
 * mrt_camera_rays on a scene with aprt == 0 that is, bit for bit, the accumulator of a fresh context after an execute of
 * n_samples.  A primary miss contributes the raw sky colour (or the environment's texel), as in a frame.
 * The call observes and changes nothing of the context: accumulator, counts, samples booked under MRT_FLAG_DEFER, the adaptive
 * state and cached AOVs stay as they are.  Ray i is thread i of 256-thread workgroups (lane i % 64 of wavefront i / 64).  The
 * kernel carries the full feature set the scene-through-L2 kernels carry; it stages the scene in LDS when the context stages
 * the whole scene and that takes at most a quarter of the LDS, and reads it through L2 otherwise; info says what ran.
 * A sharded context serves the rays it is given (a rank passes its slice of a batch and the keys of that slice).
 * MRT_ERR_ARG: a null pointer (key may be NULL), n == 0 or n >= 2^30, n_samples == 0, sample_base + n_samples > 2^32 - 1, an
 * unknown flag, a non-zero reserved word; MRT_ERR_STATE: a multi-device context (n_devices > 1). */
#define MRT_RAYS_DEVICE 1u     /* orig, dir, key and rgb are device pointers on the context's device */
typedef struct mrt_rays {
    size_t n;                  /* 1 .. 2^30 - 1 */
    const float *orig;         /* [n][3] */
    const float *dir;          /* [n][3] */
    const uint32_t *key;       /* [n] or NULL: ray i takes key i */
    uint32_t sample_base, n_samples;   /* global sample indices [sample_base, sample_base + n_samples) */
    uint32_t flags;            /* MRT_RAYS_* */
    uint32_t reserved[3];      /* 0 */
} mrt_rays;
typedef struct mrt_rays_info {
    double kernel_ms;          /* HIP-event time of the kernel */
    uint64_t samples;          /* n * n_samples */
    uint64_t segments;         /* path segments traced */
    uint32_t kernel_features;  /* FEAT of the kernel that ran */
    uint32_t scene_in_lds;     /* 1: scene staged in LDS, 0: read through L2 */
    uint32_t lds_bytes;        /* LDS per workgroup */
    uint32_t reserved;
} mrt_rays_info;
int mrt_radiance(mrt_ctx *ctx, const mrt_rays *r, float *rgb /*[n][3]*/, mrt_rays_info *info /*may be NULL*/);

/* The lens-centre camera ray of every supersampled pixel, row-major: the ray of the depth AOV and, when aprt == 0, of every sample
 * of the pixel.  Either output may be NULL.  Host pointers.  MRT_ERR_STATE: a multi-device context. */
int mrt_camera_rays(mrt_ctx *ctx, float *orig /*[nh][nw][3]*/, float *dir /*[nh][nw][3]*/);

/* ---- adaptive sampling on caller-supplied rays: mrt_execute_adaptive for custom cameras ----
 * One ray per supersampled pixel of the context's [nh][nw] grid, traced as given by the rules of mrt_radiance.  Pixel
 * p = y * nw + x is ray p with hash key p; there is no key array.  Rounds, evaluation points, the stop rule, the rules of
 * mrt_adapt with their MRT_ERR_ARGs, and mrt_adapt_info are those of mrt_execute_adaptive.  The accumulator of a tile that
 * stopped at n holds the bytes mrt_radiance (sample_base 0, n_samples n, key NULL) gives for its rays; the half buffer holds the
 * chunk sums of the even rounds, added in chunk order to 0.  With the rays of mrt_camera_rays on a scene with aprt == 0,
 * accumulator, half buffer, counts and info (apart from times) equal those of mrt_execute_adaptive on a fresh context of the
 * same seed, bit for bit.
 * Preconditions as mrt_execute_adaptive: a context that holds no samples and has none booked; sharded and multi-device contexts:
 * MRT_ERR_STATE.  MRT_ERR_ARG: a null ctx, r, orig or dir, a broken rule, a flag other than MRT_RAYS_DEVICE (orig and dir are
 * device pointers on the context's device), a non-zero reserved word.  A refused call changes nothing; a call that fails half
 * way leaves an empty uniform context.  Runs eagerly; pointers are borrowed for the call.
 * Afterwards the context is in the adaptive state exactly as after mrt_execute_adaptive (mrt_img*, mrt_img_hdr, mrt_accum,
 * mrt_sample_counts, mrt_adapt_half, mrt_denoise, mrt_get_stats serve it; mrt_execute refuses until mrt_reset or mrt_set_accum*),
 * and it remembers that the half buffer belongs to a supplied grid: MRT_DN_VARIANCE then serves only while AOVs of mrt_aov_rays
 * are installed (MRT_ERR_STATE with the camera's own or none).  The library cannot verify that mrt_aov_rays and this call were
 * given the same rays: that is the caller's responsibility, as the frame handed to mrt_set_accum is. */
typedef struct mrt_rays_adapt {
    const float *orig;         /* [nh][nw][3] */
    const float *dir;          /* [nh][nw][3] */
    mrt_adapt    rule;
    uint32_t     flags;        /* MRT_RAYS_DEVICE or 0 */
    uint32_t     reserved[3];  /* 0 */
} mrt_rays_adapt;
int mrt_radiance_adaptive(mrt_ctx *ctx, const mrt_rays_adapt *r, mrt_adapt_info *info /*may be NULL*/, double *seconds /*may be NULL*/);

/* ---- point gathers: irradiance and SH9 light probes, lightmap baking ----
 * mrt_gather forms n_dirs rays at each of n points on the device, path-traces them by the rules of mrt_radiance and reduces the
 * radiance of each point's rays to one answer; neither the rays nor their sums leave the device.
 * Directions (csrc/mrt_gather.h, f32, unfused): a spherical Fibonacci set turned per point by a hashed angle.  Point i has the
 * point key key_base + i; rot_i = mix32(pix_key(key_base + i) + 0x85EBCA6B) with the pix_key of mrt_radiance; direction j has the
 * azimuth phi = 6.28318548f * u32_to_unit(rot_i + j * 0x9E3779B9), (s, c) = sincos(phi), and
 *   MRT_GATHER_SPHERE     z = 1 - (2j + 1) / n_dirs, q = sqrt(max(0, 1 - z z)), d = (q c, q s, z)
 *   MRT_GATHER_HEMI_COS   u = (2j + 1) / (2 n_dirs), local (sqrt(u) c, sqrt(u) s, sqrt(1 - u)), taken to the world by the branchless
 *                         frame of Duff et al. 2017 about n = normal[i] / |normal[i]|: d = (t lx + bt ly) + n lz
 * stored as formed (no renormalisation).  Ray (i, j) starts at pos[i] + d * offset (SPHERE) or pos[i] + n * offset (HEMI_COS), has
 * the hash key key_base + i * n_dirs + j (mod 2^32) and is sampled n_samples times from sample_base as mrt_radiance samples it: its
 * canonical sum S_ij gives L_ij = S_ij * (1.0f / n_samples).
 * Reduction: one wavefront per point.  Lane l adds its terms j = l, l + 64, ... in rising j from +0 -- L_ij (MEAN) or
 * L_ij.c * Y_k(d_ij) (SH9) --, the 64 partials are combined pairwise (p[l] += p[l + 32], then 16, 8, 4, 2, 1), and p[0] is scaled
 * by 1.0f / n_dirs (MEAN) or 12.566370614f / n_dirs (SH9).  Y_0..Y_8: 0.282094792, 0.488602512 (y, z, x), 1.092548431 xy,
 * 1.092548431 yz, 0.315391565 (3 zz - 1), 1.092548431 xz, 0.546274215 (xx - yy), evaluated at the stored direction.
 * A zero or non-finite normal gives NaN directions for that point and whatever their reduction gives; other points are not
 * disturbed.  The points are traced in batches of whole points (default max(1, 2^22 / n_dirs) of them, ~170 MB of workspace
 * allocated once per call); the answer does not depend on the batch size.
 * Like mrt_radiance the call observes and changes nothing of the context; a row-sharded context serves it.
 * MRT_ERR_ARG: a null ctx, g, pos or out; n outside 1 .. 2^30 - 1; n_dirs outside 1 .. 65536; n_samples == 0 or
 * sample_base + n_samples > 2^32 - 1; an unknown dist, out or flag; SH9 with HEMI_COS; HEMI_COS without normal, SPHERE with one; an
 * offset that is non-finite or negative; a non-zero reserved word; mrt_gather_rays: first + count > n.
 * MRT_ERR_STATE: a multi-device context. */
#define MRT_GATHER_SPHERE   0u   /* n_dirs directions over the whole sphere, uniform in solid angle           */
#define MRT_GATHER_HEMI_COS 1u   /* n_dirs directions over the hemisphere about normal[i], cosine-distributed */
#define MRT_GATHER_MEAN 0u       /* out[n][3]: mean radiance over the set (HEMI_COS: irradiance / pi)          */
#define MRT_GATHER_SH9  1u       /* out[n][9][3]: radiance projected on the 9 real SH of bands 0..2; SPHERE only */
typedef struct mrt_gather_desc {
    size_t n;                   /* points, 1 .. 2^30 - 1 */
    const float *pos;           /* [n][3] */
    const float *normal;        /* [n][3], any length; required for HEMI_COS, must be NULL for SPHERE */
    uint32_t n_dirs;            /* 1 .. 65536 */
    uint32_t sample_base, n_samples;   /* per ray, rules of mrt_rays */
    uint32_t dist, out;         /* MRT_GATHER_* */
    uint32_t key_base;          /* point i has point key key_base + i; ray (i, j) has hash key key_base + i * n_dirs + j (mod 2^32) */
    float    offset;            /* finite, >= 0: origin = pos + dir * offset (SPHERE), pos + unit normal * offset (HEMI_COS) */
    uint32_t batch_points;      /* 0: default; else points per internal batch (results do not depend on it) */
    uint32_t flags;             /* MRT_RAYS_DEVICE: pos, normal and the outputs are device pointers */
    uint32_t reserved[3];       /* 0 */
} mrt_gather_desc;
typedef struct mrt_gather_info {
    double gen_ms, kernel_ms, reduce_ms;     /* HIP-event times summed over batches */
    uint64_t rays, samples, segments;
    uint32_t batches, kernel_features, scene_in_lds, lds_bytes;
} mrt_gather_info;
int mrt_gather(mrt_ctx *ctx, const mrt_gather_desc *g, float *out, mrt_gather_info *info /*may be NULL*/);
/* The rays of points [first, first + count) as mrt_gather forms them: orig, dir [count][n_dirs][3], key [count][n_dirs]; any may be
 * NULL.  g->out is validated and not used. */
int mrt_gather_rays(mrt_ctx *ctx, const mrt_gather_desc *g, size_t first, size_t count, float *orig, float *dir, uint32_t *key);

/* ---- linear float image at the output resolution (not in the reference) ----
 * mrt_img tone-maps, truncates to u8 and only then resizes, as the reference does; mrt_img_hdr resamples the mean radiance itself,
 * in f32 on the device, with no tone map and no quantisation: rgb[res_h][res_w][3], linear, >= 0.
 *   mean       m = sum * (1.0f / count): the context's count, after mrt_execute_adaptive the count of the pixel's 8x8 tile
 *              (the means mrt_img and mrt_denoise form); with denoise != NULL the filtered means of mrt_denoise under those options
 *   resize     vertical pass, then horizontal pass, f32, unfused, each sum from +0 with its taps in index order
 *   output     u > 0 ? u : 0: negative filter lobes and NaN give 0, +inf stays.  nw == res_w and nh == res_h: the clamped means.
 * MRT_RESIZE_LANCZOS3 uses the taps of mrt_img, bit for bit.  MRT_RESIZE_BOX is the area average: on the common grid source pixel
 * i covers [i*dst, (i+1)*dst) and output o covers [o*src, (o+1)*src); the weight of i in o is their overlap / src, rounded once to
 * f32 -- no negative lobe, hence no ringing around a sun or an emitter; exact at integer ratios; the same rule upsamples.
 * An observation exactly like mrt_img: booked samples are traced first; needs the whole frame (unsharded, or after mrt_set_accum*)
 * and at least one sample, else MRT_ERR_STATE (and the MRT_ERR_STATEs of mrt_denoise with denoise != NULL); nothing of the context
 * changes and mrt_stats.img_ms stays as it was.  NULL options: Lanczos3 of the means.  MRT_ERR_ARG: ctx or rgb NULL, an unknown
 * filter, a non-zero reserved word, denoise options mrt_denoise would refuse. */
#define MRT_RESIZE_LANCZOS3 0u   /* the taps of mrt_img */
#define MRT_RESIZE_BOX      1u
typedef struct mrt_hdr_opts {
    uint32_t filter;                  /* MRT_RESIZE_*; another value: MRT_ERR_ARG */
    uint32_t reserved0;               /* 0 */
    const mrt_denoise_opts *denoise;  /* NULL: the means; else the filtered means, rules of mrt_denoise */
    uint32_t reserved[4];             /* 0, else MRT_ERR_ARG */
} mrt_hdr_opts;
typedef struct mrt_hdr_info {
    double resize_ms;                 /* HIP-event time of this call's kernels; 0 under MRT_FLAG_NO_EVENT_TIMING */
    mrt_denoise_info dn;              /* zeroed when denoise == NULL */
    uint32_t reserved[2];
} mrt_hdr_info;
int mrt_img_hdr(mrt_ctx *ctx, const mrt_hdr_opts *o /*NULL: defaults*/, float *rgb /*[res_h][res_w][3]*/, mrt_hdr_info *info /*may be NULL*/);

/* Write a float image rgb[h][w][3]; host only, like mrt_save_image.  The format follows the extension, any other: MRT_ERR_ARG.
 *   .pfm   "PF\n<w> <h>\n-1.0\n", then the rows bottom to top as little-endian f32 RGB, the values as given
 *   .hdr   Radiance RGBE: "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y <h> +X <w>\n", scanlines new-style run-length coded for
 *          8 <= w <= 32767 and flat otherwise.  Per pixel: NaN and negative components count as 0, +inf as FLT_MAX; with
 *          v = max(r, g, b) = f * 2^E, f in [0.5, 1): four zero bytes for v < 2^-127, else mantissas floor(c * 2^(8-E) + 0.5) (E + 1 when
 *          the largest reaches 256) and the exponent byte E + 128, saturated at 255 with mantissas capped at 255.  Rounding to
 *          nearest, because readers decode b * 2^(e-136): below the saturation a component errs by at most 2^(E-9) <= v / 256.
 * MRT_ERR_ARG: a NULL pointer, w == 0 or h == 0; MRT_ERR_STATE: the file cannot be written. */
int mrt_save_image_f32(const char *path, const float *rgb, uint32_t w, uint32_t h);

/* Test hook: run one device math-contract function elementwise on the GPU.
 * op: 0 sin, 1 cos, 2 acos, 3 atan2(a,b), 4 pow(a,b), 5 1/a, 6 sqrt(a), 7 a/b, 12 the first component of norm(a, b, 0.25);
 * 16 the longitude 0.5 + 0.5 atan2(a, -b) / pi and 17 the latitude acos(clamp(a, -1, 1)) / pi of the texture lookups, 18 / 19 the
 * two quotients a / (a + b), b / (a + b) over one reciprocal.  Element i is thread i of 256-thread workgroups (lane i % 64 of
 * wavefront i / 64).  b may be NULL for unary ops. */
int mrt_selftest_math(int device, int op, const float *a, const float *b, float *out, size_t n);

/* Test hook: closest-hit queries on caller-supplied rays, through the closest-hit code of the context's own path-tracing kernel.
 * Ray i (origin orig[i], direction dir[i], traced as given: no shift of the origin, no normalisation) is thread i of a launch of
 * 256-thread workgroups -- lane i % 64 of wavefront i / 64, so the caller composes the wavefronts; threads >= n leave before the
 * query.  The kernel stages the scene as the context's path-tracing kernel does (LDS, warm, deep or through L2, with its walk
 * areas) and is the instantiation the context would run at 256 threads (mrt_stats.kernel_features of such a context).
 * out[i][MRT_TRACE_WORDS]: [0] hit (0 / 1)  [1] the shadow query's answer on the same ray (0 / 1)  [2] renderer and [3] instance
 * as mrt_aov numbers them (0xffffffff = -1 on a miss)  [4] t0 and [5] t1 as bit patterns  [6..8] the world shading normal at t0 as
 * bit patterns (the normal plane of mrt_aov); words 4..8 are 0 on a miss.
 * MRT_ERR_ARG: n == 0, n >= 2^31 or a null pointer; MRT_ERR_STATE: a sharded or multi-device context, or a kernel instantiation
 * the hook is not built for (the message names it).  Accumulator, booked samples and cached AOVs are not touched. */
#define MRT_TRACE_WORDS 9u
int mrt_selftest_trace(mrt_ctx *ctx, size_t n, const float *orig /*[n][3]*/, const float *dir /*[n][3]*/, uint32_t *out /*[n][MRT_TRACE_WORDS]*/);

/* Test hook, host only (no device needed, like mrt_plan_launch): the list of the path-tracing kernel's compiled instantiations, one
 * row per (workgroup size, scene staged in LDS or read through L2, FEAT template argument = mrt_stats.kernel_features), expanded
 * from the same lists the launchers dispatch over; every row exists once as the full-frame kernel and once as the tile-list kernel
 * of mrt_execute_adaptive.  Writes the first min(count, cap) rows to threads[], scene_in_lds[] (0 / 1) and feat[] (each may be NULL)
 * and returns the count, whatever cap is. */
uint32_t mrt_selftest_instantiations(uint32_t *threads, uint32_t *scene_in_lds, uint32_t *feat, uint32_t cap);

/* Test hook: compare, on the device, the fast correctly rounded cores of the math contract (sqrt, 1/x, a/b and the
 * 1/sqrt(m) of Vec3f::norm, src/lin.rs:60-66) with the compiler's full IEEE expansions, on `count` inputs generated
 * from the indices first .. first+count-1: op 0 sqrt and op 1 recip take the index as the f32 bit pattern (first = 0,
 * count = 2^32 covers every float); op 2 divide and op 3 norm scale hash (seed, index) into operands.
 * *mismatches = number of differing results (NaN == NaN); example[4] = {a, b, fast, reference} of one of them. */
int mrt_selftest_sweep(int device, int op, uint64_t first, uint64_t count, uint32_t seed, uint64_t *mismatches, float *example);

#ifdef __cplusplus
}
#endif
#endif /* MRT_H */
