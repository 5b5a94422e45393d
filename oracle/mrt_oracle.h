/*
 * mrt_oracle.h — TEST INFRASTRUCTURE.  CPU restatement (plain C) of micro-raytracer's
 * path-tracing hot path: src/rt.rs, src/lin.rs, src/sampler.rs of the reference.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may build, load or
 * call this.  The product (libmrt_hip.so) never links or calls it.
 *
 * PARITY PIN STATUS: the reference has no tests, no golden vectors and no RNG seed
 * (rand::thread_rng at src/rt.rs:564,579,917,919,968,997,998,1054), and it cannot be built
 * in this environment (no Rust toolchain).  The restatement is pinned against the rendered
 * images the reference ships: doc/out0.png and doc/out1.png (deterministic scene, exact
 * to <= 1 LSB on > 99.8 % of channels) and doc/out2.png / doc/out3.png (statistical).  See
 * tests/golden/README.md and tests/test_oracle_pins.py.  RNG stream (rand 0.8.5) and the
 * `image` crate's Lanczos3 are third-party code absent from the reference tree: the
 * seeded counter RNG is build-defined => sample-level parity with the Rust
 * binary is UNPINNED (statistical only); Lanczos3 follows image 0.24's published algorithm.
 *
 * BEYOND THE REFERENCE: orc_create_ext also restates what mrt_create_ext adds to the path -- per-corner normals and UVs
 * (DESIGN.md section 14), the environment texture (section 15) and the bilinear filter (section 16) -- from the contract text
 * of those sections and of include/mrt.h, not from the kernel headers.  It indexes attributes by the description-order
 * triangle id and reads the description's f32 texels, so the packer's leaf order and texel formats are checked too.  There is
 * nothing in the reference to pin these against: they are held to the x86 build of the kernel headers and to the GPU
 * (tests/test_oracle_ext.py, tests/test_gpu_oracle_ext.py), and their elementwise pieces to the float32 numpy restatements of
 * tests/vattr_ref.py, tests/env_ref.py and tests/filter_ref.py.
 *
 * FIRST-HIT AOVS: orc_aov restates mrt_aov from DESIGN.md section 13 (lens-centre ray, closest hit, t0, world normal, albedo x
 * texture, world point, description-order ids), section 14 (shading normal, interpolated UV) and sections 15 / 16 (the albedo of
 * a miss under an environment is E(d) = sky.color (hadamard) texel, the texel the centre ray's direction d sees under the
 * environment's mapping, rot and filter -- neither sky.pwr nor the mean m enters it), not from csrc/mrt_denoise.h.  It is
 * anchored to float64 closest hits, rotated instances and camera included, and holds the x86 build of aov_pixel and the GPU to
 * bit equality on every plane (tests/test_oracle_aov.py, tests/test_gpu_oracle_aov.py, the fuzz of tests/test_fuzz_scenes.py).
 *
 * RADIANCE ON SUPPLIED RAYS: orc_radiance runs the path loop and fold of orc_execute on a first ray handed in (DESIGN.md section
 * 18: traced as given, no lens draw).  It is anchored to orc_execute and orc_trace_pixel bit for bit on the camera's own rays and
 * holds the x86 build of rays_body and the GPU's mrt_radiance to 1e-4 of max(n_samples, |sum|) per ray, with equal segment counts
 * (tests/test_radiance_oracle_host.py, tests/test_gpu_radiance_oracle.py).
 */
#ifndef MRT_ORACLE_H
#define MRT_ORACLE_H

#include <stdint.h>
#include <stddef.h>
#include "../include/mrt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orc_ctx orc_ctx;

/* Deep-copies the description; builds mesh octrees (src/parser.rs:815-816). NULL + orc_error() on reject. */
orc_ctx *orc_create(const mrt_render_desc *desc, uint64_t seed);
/* The same for a scene with attributes, an environment or filtered textures (mrt_create_ext).  ext == NULL, or an ext that
 * requests nothing: exactly orc_create.  Rejects what mrt_create_ext rejects (texture maps on a triangle / mesh without uv
 * included). */
orc_ctx *orc_create_ext(const mrt_render_desc *desc, const mrt_desc_ext *ext, uint64_t seed);
void orc_destroy(orc_ctx *c);
const char *orc_error(void);

void orc_dims(const orc_ctx *c, uint32_t *nw, uint32_t *nh);

/* n_samples x Sampler::execute (src/sampler.rs:28-78) on `threads` workers with n_dim x n_dim
 * tile jobs.  Returns wall seconds. */
double orc_execute(orc_ctx *c, uint32_t n_samples, uint32_t threads, uint32_t n_dim);

/* Same, restricted to supersampled rows [row0, row1) (for bounded CPU-baseline samples). */
double orc_execute_rows(orc_ctx *c, uint32_t n_samples, uint32_t threads, uint32_t n_dim,
                        uint32_t row0, uint32_t row1);

/* colors / last_count (src/sampler.rs:14-15). rgb[nh][nw][3]. */
void orc_accum(const orc_ctx *c, float *rgb, uint32_t *count);
void orc_set_accum(orc_ctx *c, const float *rgb, uint32_t count);
void orc_reset(orc_ctx *c);
uint64_t orc_segments(const orc_ctx *c);

/* Sampler::img (src/sampler.rs:80-99). rgb8[res_h][res_w][3]; returns 0 / -1. */
int orc_img(const orc_ctx *c, uint8_t *rgb8);
int orc_img_ss(const orc_ctx *c, uint8_t *rgb8);   /* before the resize: rgb8[nh][nw][3] */

/* One reduce_light(iter(x, y)) evaluation (src/rt.rs:937-994) for sample index s. */
void orc_trace_pixel(const orc_ctx *c, uint32_t x, uint32_t y, uint32_t s, float rgb[3], uint32_t *segments);

/* First-hit AOVs of the supersampled frame (with the additions of sections 14-16), one ray per pixel
 * through the lens centre, no random draw: depth[nh][nw] (t0 along the unit direction, +inf on a miss), normal[nh][nw][3] (the
 * world shading normal), albedo[nh][nw][3] (albedo x texture at the hit's UV), renderer[nh][nw] (index into mrt_scene.renderer),
 * instance[nh][nw] (index into that renderer's inst list), point[nh][nw][3] (o + d t0, o the shifted origin).  A miss has
 * normal, point 0 and ids -1; its albedo is 0, or with an environment E(d) = sky.color x texel, the texel being the one the
 * centre ray's direction d sees under the environment's mapping, rot and filter (no sky.pwr, not the mean).  Any output may be
 * NULL. */
void orc_aov(const orc_ctx *c, float *depth, float *normal, float *albedo, int32_t *renderer, int32_t *instance, float *point);

/* n closest-hit queries on caller-supplied rays: RayTracer::closest_hit (src/rt.rs:867-898) on the ray (orig, dir) -- a ray as
 * Ray::cast leaves it, i.e. orig is the origin the intersection routines see and is not shifted again, dir is not normalised --
 * and the shadow form of the same query.  out[i][ORC_RAY_WORDS]: [0] hit  [1] the shadow query's Some / None  [2] renderer and
 * [3] instance as orc_aov numbers them (0xffffffff on a miss)  [4] t0 and [5] t1 of the entry / exit hit as bit patterns  [6..8] the
 * world shading normal at t0 as orc_aov forms it, as bit patterns; words 4..8 are 0 on a miss. */
#define ORC_RAY_WORDS 9u
void orc_ray_query(const orc_ctx *c, size_t n, const float *orig, const float *dir, uint32_t *out);

/* Radiance along n caller-supplied rays: ray i is path-traced as given -- a ray as Ray::cast leaves it, as
 * for orc_ray_query: no shift of the origin by E, no normalisation, pwr 1, bounce 0, no lens draw -- for the samples
 * [sample_base, sample_base + n_samples) under the path key orc_path_key(seed, key[i], sample); key == NULL: key[i] = i.
 * rgb[n][3]: the samples' reduce_light values added one by one from 0, as src/sampler.rs:62-70 adds them.  segments[n] (may be
 * NULL): ray i's closest-hit queries under the kernel's stop rule -- per path, those up to and including the first hit, in path
 * order, whose emit coin comes up (the reference traces on and its fold discards the rest; orc_segments counts those too). */
void orc_radiance(const orc_ctx *c, size_t n, const float *orig, const float *dir, const uint32_t *key, uint32_t sample_base,
                  uint32_t n_samples, float *rgb, uint64_t *segments);

/* Stand-alone pieces for unit tests */
void orc_tonemap_px(const float sum[3], uint32_t count, float gamma, float exp, uint8_t out[3]);
int  orc_lanczos3_resize(const uint8_t *src, uint32_t sw, uint32_t sh, uint8_t *dst, uint32_t dw, uint32_t dh);
int  orc_lanczos3_weights(uint32_t src, uint32_t dst, uint32_t o, uint32_t *left, float *w, uint32_t cap);

/* octree of mesh renderer r flattened in traversal order: returns #leaves; for each leaf
 * rel_pos[3], size[3] and its triangle ids. Buffers may be NULL to query sizes. */
int orc_mesh_octree(const orc_ctx *c, uint32_t renderer, float *leaf_boxes /*[n][6]*/,
                    uint32_t *leaf_counts, uint32_t *ids, uint32_t ids_cap, uint32_t *n_ids);

/* RNG contract */
uint32_t orc_path_key(uint64_t seed, uint32_t pixel, uint32_t sample);
uint32_t orc_draw_u32(uint32_t path_key, uint32_t dim);
float    orc_draw_f32(uint32_t path_key, uint32_t dim);

/* math contract (elementwise) : op as in mrt_selftest_math */
void orc_math(int op, const float *a, const float *b, float *out, size_t n);

/* DESIGN.md sections 14-16, elementwise (tests/test_oracle_ext.py anchors them to the numpy restatements):
 * orc_vattr      n cases p[3], v0[3], e1[3], e2[3], vn[9], uv[6] -> the shading normal before xf_vec / norm (the face normal
 *                where the contract falls back) and the wrapped UV; either output may be NULL (then its input may be too)
 * orc_env_lookup n directions d[3] -> the texel of the w x h f32 texture each one sees (E(d) without sky.color) under
 *                mapping (MRT_ENV_*), rot and filter (MRT_FILTER_*), and its coordinate; either output may be NULL
 * orc_env_mean   the solid-angle-weighted mean m of the texture */
void orc_vattr(size_t n, const float *p, const float *v0, const float *e1, const float *e2, const float *vn, const float *uv,
               float *normal_out, float *uv_out);
void orc_env_lookup(uint32_t w, uint32_t h, const float *dat, uint32_t mapping, float rot, uint32_t filter, size_t n, const float *d,
                    float *rgb_out, float *uv_out);
void orc_env_mean(uint32_t w, uint32_t h, const float *dat, uint32_t mapping, float m_out[3]);

#ifdef __cplusplus
}
#endif
#endif
