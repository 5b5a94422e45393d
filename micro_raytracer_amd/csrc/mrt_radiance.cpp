// mrt_radiance.cpp — radiance along caller-supplied rays: mrt_radiance, mrt_camera_rays.
#include <string.h>

#include "mrt_ctx.h"

using namespace mrt;
using namespace mrt::api;

int mrt::api::rays_kernel(mrt_ctx *c, RaysKernel &k)
{
    // The scene as a kernel without F_DEEP reads it: the context's own blob, or (deep staging) the binary-BVH packing
    const FlatScene fs = flat_scene(c);
    if (!fs.blob) return g_status;
    const Packed &rp = fs.pk;
    k.P = c->P;
    if (c->aov_pk) {
        k.P = rp.P;
        k.P.seed_lo = c->P.seed_lo; k.P.seed_hi = c->P.seed_hi;
    }
    k.P.blob = fs.blob;
    k.inst = pt_instantiation(256u, false, rp.features);
    // Staged in LDS when the context stages the whole scene and four 256-thread workgroups of it -- the 4 waves per SIMD these
    // feature sets are bound to -- still fit a CU; through L2 otherwise (warm, deep and L2 contexts, MRT_SCENE_IN_L2)
    k.in_lds = c->plan.in_lds && c->plan.staging == 0u && rays_lds_bytes(k.P, true, k.inst) <= kLdsLimit / 4u;
    k.lds = rays_lds_bytes(k.P, k.in_lds, k.inst);
    return MRT_OK;
}

extern "C" {

int mrt_radiance(mrt_ctx *c, const mrt_rays *r, float *rgb, mrt_rays_info *info)
{
    if (!c || !r || !rgb || !r->orig || !r->dir) return fail(MRT_ERR_ARG, "mrt_radiance: null argument");
    if (r->n == 0 || r->n >= ((size_t)1 << 30)) return fail(MRT_ERR_ARG, "mrt_radiance: n = %zu is outside 1 .. 2^30 - 1", r->n);
    if (r->n_samples == 0) return fail(MRT_ERR_ARG, "mrt_radiance: n_samples = 0");
    if ((unsigned long long)r->sample_base + r->n_samples > 0xffffffffull)
        return fail(MRT_ERR_ARG, "mrt_radiance: samples [%u, + %u) reach past 2^32 - 1", r->sample_base, r->n_samples);
    int rc;
    if ((rc = rays_words(r->flags, r->reserved, "mrt_radiance"))) return rc;
    if (c->group) return fail(MRT_ERR_STATE, "mrt_radiance: multi-device context");
    if ((rc = set_device(c))) return rc;
    RaysKernel k;
    if ((rc = rays_kernel(c, k))) return rc;
    const size_t n = r->n;
    const bool dev = (r->flags & MRT_RAYS_DEVICE) != 0u;
    DeviceRays rays;
    DeviceMem<float> d_rgb;
    DeviceMem<u32> d_key;
    const u32 *pkey = r->key;
    float *pout = rgb;
    HIP_TRY(rays.take(r->orig, r->dir, n, dev));
    if (!dev) {
        HIP_TRY(d_rgb.alloc(n * 3u));
        pout = d_rgb.p;
        if (r->key) {
            HIP_TRY(d_key.alloc(n));
            HIP_TRY(hipMemcpy(d_key.p, r->key, n * sizeof(u32), hipMemcpyHostToDevice));
            pkey = d_key.p;
        }
    }
    // everything the kernel writes belongs to the call: the sums, and a segment counter of its own
    DeviceMem<unsigned long long> d_seg;
    HIP_TRY(alloc_counters(d_seg));
    Event e0, e1;
    HIP_TRY(create(e0));
    HIP_TRY(create(e1));
    hipStream_t st = c->stream.get();
    HIP_TRY(hipMemsetAsync(pout, 0, n * 3u * sizeof(float), st));
    k.P.n_samples = r->n_samples; k.P.sample_base = r->sample_base;
    k.P.k_split = 1u; k.P.to_planes = 0u;
    k.P.accum = pout; k.P.partial = nullptr; k.P.partial_stride = 0ull;
    k.P.count_segments = 1u; k.P.segments = d_seg.p;
    k.P.tile_counter = nullptr; k.P.persist_grid = 0u;
    HIP_TRY(hipEventRecord(e0.get(), st));
    HIP_TRY(launch_rays(k.P, k.in_lds, k.inst, (u32)n, rays.orig, rays.dir, pkey, st));
    HIP_TRY(hipEventRecord(e1.get(), st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!dev) HIP_TRY(hipMemcpy(rgb, d_rgb.p, n * 3u * sizeof(float), hipMemcpyDeviceToHost));
    if (info) {
        memset(info, 0, sizeof *info);
        float t = 0.0f;
        HIP_TRY(hipEventElapsedTime(&t, e0.get(), e1.get()));
        unsigned long long seg = 0;
        HIP_TRY(hipMemcpy(&seg, d_seg.p, sizeof seg, hipMemcpyDeviceToHost));
        info->kernel_ms = t;
        info->samples = (uint64_t)n * r->n_samples;
        info->segments = seg;
        info->kernel_features = k.inst;
        info->scene_in_lds = k.in_lds ? 1u : 0u;
        info->lds_bytes = (uint32_t)k.lds;
    }
    ok();
    return MRT_OK;
}

int mrt_camera_rays(mrt_ctx *c, float *orig, float *dir)
{
    if (!c) return fail(MRT_ERR_ARG, "mrt_camera_rays: null context");
    if (c->group) return fail(MRT_ERR_STATE, "mrt_camera_rays: multi-device context");
    int rc;
    if ((rc = set_device(c))) return rc;
    const size_t words = (size_t)c->pk.nw * c->pk.nh * 3u;
    DeviceMem<float> d_o, d_d;
    if (orig) HIP_TRY(d_o.alloc(words));
    if (dir) HIP_TRY(d_d.alloc(words));
    if (orig || dir) {
        HIP_TRY(launch_camera_rays(c->P, d_o.p, d_d.p, c->stream.get()));
        HIP_TRY(hipStreamSynchronize(c->stream.get()));
    }
    if (orig) HIP_TRY(hipMemcpy(orig, d_o.p, words * sizeof(float), hipMemcpyDeviceToHost));
    if (dir) HIP_TRY(hipMemcpy(dir, d_d.p, words * sizeof(float), hipMemcpyDeviceToHost));
    ok();
    return MRT_OK;
}

}  // extern "C"
