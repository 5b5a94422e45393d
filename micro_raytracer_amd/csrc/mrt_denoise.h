// mrt_denoise.h — per-pixel bodies of the first-hit AOV pass and of the edge-avoiding a-trous filter (mrt_aov, mrt_denoise,
// mrt_img_denoised).  Shared by the kernels of mrt_denoise.hip and, for the CPU-side unit tests, an x86 build
// (tests/emu/denoise_probe.cpp), so that both run the same text.
//
// Filter (Dammertz et al. 2010), f32 in exactly this order (-ffp-contract=off; IEEE division; max = fmaxf):
//   c_p = A_p * rc_p (the mean the tone map forms);  D_p = hit_p ? fmaxf(albedo_p, 1/256) : 1 per channel;  e_p = c_p / D_p
//   (a context with an environment texture, DESIGN.md §15: D_p = fmaxf(albedo_p, 1/256) for miss pixels too -- their albedo is E(d))
//   pass i, step s = 2^i, sc_i = sc * 4^i: for the 5x5 taps q = p + s * (dx, dy) inside the frame, dy outer, dx inner:
//     w = 0 if hit_p != hit_q, else ((k5[dx] * k5[dy] * wc) * wn) * wp  (dn_tap_weight)
//     num += w * e_q, den += w for taps with w > 0;  e'_p = den > 0 ? num / den : e_p
//   c'_p = e'_p * D_p
// On a frame periodic in x (MRT_AOV_WRAP_X) q.x = (p.x + s * dx) mod nw: all five columns of a row count.
#pragma once
#include "mrt_trace.h"

namespace mrt {

constexpr u32 kDnMaxPasses = 8;
constexpr float kDnAlbedoFloor = 1.0f / 256.0f;

// Guide of one pixel: the first hit's world normal and depth (g[0..3]), its world point and the hit flag (g[4..7]: 1 hit,
// 0 miss; -1 marks a tap outside the frame in the kernel's LDS tile, which matches no pixel)
struct DnGuide { float nx, ny, nz, t, px, py, pz, hit; };

// First-hit AOVs of one pixel: one ray through the lens centre, the closest hit of trace<false, FEAT>
struct AovPixel {
    DnGuide g;
    V3 albedo;
    i32 rend;      // renderer index (description order), -1: miss
    i32 inst;      // flat instance index of the packed scene, -1: miss
};

// ... of one ray (o, d), traced as given: the body both ray sources share -- the camera's lens-centre ray (aov_pixel) and a
// caller-supplied one (mrt_aov_rays); t is the ray parameter, the world point o + d * t0 unfused
template <u32 FEAT>
MRT_HD AovPixel aov_ray(const Scn &S, const V3 &o, const V3 &d)
{
    const Params &P = *S.P;
    Hit h;
    AovPixel a;
    if (!trace<false, FEAT>(S, ray_pre<FEAT>(o, d), h)) {
        a.g.nx = 0.0f; a.g.ny = 0.0f; a.g.nz = 0.0f; a.g.t = __builtin_inff();
        a.g.px = 0.0f; a.g.py = 0.0f; a.g.pz = 0.0f; a.g.hit = 0.0f;
        a.albedo = v3(0.0f, 0.0f, 0.0f);
        if constexpr (FEAT & F_ENV) { if (P.off_env != 0u) { float sky_pwr; a.albedo = env_color<FEAT>(S, d, sky_pwr); } }      // the backdrop the centre ray sees
        a.rend = -1; a.inst = -1;
        return a;
    }
    const Obj ob = obj_of(S, h);
    const V3 p0 = add(o, muls(d, h.t0));                 // render_pixel's p0_
    const V3 nh0 = to_object(ob, p0);
    const V3 n = hit_normal<FEAT>(S, ob, nh0, h.i0);
    a.g.nx = n.x; a.g.ny = n.y; a.g.nz = n.z; a.g.t = h.t0;
    a.g.px = p0.x; a.g.py = p0.y; a.g.pz = p0.z; a.g.hit = 1.0f;
    a.albedo = surf_color<FEAT>(S, surf_of<FEAT>(S, h, ob, nh0, h.i0));
    a.rend = h.rend; a.inst = (i32)h.inst;
    return a;
}

template <u32 FEAT>
MRT_HD AovPixel aov_pixel(const Scn &S, u32 x, u32 y)
{
    const Params &P = *S.P;
    V3 o, d;
    camera_ray_centre(P, S.F + P.off_cam, pixel_focus(P, (float)x, (float)y), o, d);
    return aov_ray<FEAT>(S, o, d);
}

// B3 spline taps, k5[dx + 2]
MRT_HD float dn_k5(int i) { return i == 0 ? 0.375f : ((i == 1 || i == -1) ? 0.25f : 0.0625f); }

// demodulation divisor of one channel (env: the context has an environment texture, a miss pixel's albedo is its backdrop)
MRT_HD float dn_demod(float albedo, float hit, bool env = false) { return (hit != 0.0f || env) ? __builtin_fmaxf(albedo, kDnAlbedoFloor) : 1.0f; }

// weight of tap q for pixel p: k = k5[dx] * k5[dy]; sc = sc_i of the pass, sn, sp as formed on the host
MRT_HD float dn_tap_weight(float k, const float *ep, const float *eq, const DnGuide &gp, const DnGuide &gq, float sc, float sn, float sp)
{
    if (gp.hit != gq.hit) return 0.0f;
    const float dr = ep[0] - eq[0], dg = ep[1] - eq[1], db = ep[2] - eq[2];
    const float wc = __builtin_fmaxf(0.0f, 1.0f - ((dr * dr + dg * dg) + db * db) * sc);
    float wn = 1.0f, wp = 1.0f;
    if (gp.hit != 0.0f) {
        const float mx = gp.nx - gq.nx, my = gp.ny - gq.ny, mz = gp.nz - gq.nz;
        wn = __builtin_fmaxf(0.0f, 1.0f - ((mx * mx + my * my) + mz * mz) * sn);
        const float ux = gq.px - gp.px, uy = gq.py - gp.py, uz = gq.pz - gp.pz;
        const float r = ((gp.nx * ux + gp.ny * uy) + gp.nz * uz) / gp.t;
        wp = __builtin_fmaxf(0.0f, 1.0f - (r * r) * sp);
    }
    return ((k * wc) * wn) * wp;
}

// running sums of one pixel's taps
struct DnAcc {
    float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f, den = 0.0f;
    MRT_HD void add(float w, const float *eq)
    {
        if (!(w > 0.0f)) return;
        n0 += w * eq[0]; n1 += w * eq[1]; n2 += w * eq[2]; den += w;
    }
    MRT_HD void result(const float *ep, float *out) const
    {
        if (den > 0.0f) { out[0] = n0 / den; out[1] = n1 / den; out[2] = n2 / den; }
        else { out[0] = ep[0]; out[1] = ep[1]; out[2] = ep[2]; }
    }
};

// The color term's 1/sigma^2 of pass i: sc * 4^i
MRT_HD float dn_pass_sc(float sc, u32 i) { return sc * (float)(1u << (2u * i)); }

// frame x of a horizontal tap on a frame periodic in x: x mod nw, a true modulo (a tap may wrap several times when 2 * step >= nw)
MRT_HD long long dn_wrap(long long x, u32 nw) { const long long m = x % (long long)nw; return m < 0 ? m + (long long)nw : m; }

// One whole pass over an nw x nh frame of e (3 floats per pixel) on the host (x86 build): out = e' of every pixel
// wrap_x (MRT_AOV_WRAP_X): the frame is periodic in x, a horizontal tap is taken at (x + step * dx) mod nw
inline void dn_pass_host(const float *e, const DnGuide *g, u32 nw, u32 nh, u32 step, float sc, float sn, float sp, float *out, bool wrap_x = false)
{
    for (u32 y = 0; y < nh; ++y)
        for (u32 x = 0; x < nw; ++x) {
            const size_t p = (size_t)y * nw + x;
            DnAcc acc;
            for (int dy = -2; dy <= 2; ++dy)
                for (int dx = -2; dx <= 2; ++dx) {
                    long long qx = (long long)x + (long long)step * dx;
                    const long long qy = (long long)y + (long long)step * dy;
                    if (wrap_x) qx = dn_wrap(qx, nw);
                    if (qx < 0 || qy < 0 || qx >= (long long)nw || qy >= (long long)nh) continue;
                    const size_t q = (size_t)qy * nw + (size_t)qx;
                    acc.add(dn_tap_weight(dn_k5(dx) * dn_k5(dy), e + 3 * p, e + 3 * q, g[p], g[q], sc, sn, sp), e + 3 * q);
                }
            acc.result(e + 3 * p, out + 3 * p);
        }
}

}  // namespace mrt
