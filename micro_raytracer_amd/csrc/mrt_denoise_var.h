// mrt_denoise_var.h — per-pixel bodies of the variance-guided denoiser mode (MRT_DN_VARIANCE of mrt_denoise / mrt_img_denoised;
// DESIGN.md §17).  Shared by the kernels of mrt_denoise_var.hip and an x86 build (tests/emu/var_probe.cpp): both run this text.
//
// The colour term of the a-trous filter (mrt_denoise.h) is driven by a per-pixel estimate of the variance of the mean, taken from
// the accumulator A and the half buffer H of an adaptive render (H: the pixel's even-numbered rounds, n/2 of its n samples).
// f32 in exactly this order (-ffp-contract=off; IEEE division; max = fmaxf), D_p and the guide terms wn, wp as mrt_denoise.h:
//   rc = 1/(float)n, rh = 1/(float)(n/2);  e = (A*rc)/D, j = (H*rh)/D, k = ((A - H)*rh)/D per channel
//   lum(v) = (0.2126f*v.r + 0.7152f*v.g) + 0.0722f*v.b;  h = (lum(j) - lum(k))*0.5f;  h2 = h finite ? h*h : 0
//   firefly, factor f: m = fmaxf of lum(e_q) over the up to 8 neighbours q inside the frame with hit_q == hit_p (unclamped e);
//     t = f*m; such a neighbour exists, lum(e_p) is finite, t >= 0 and lum(e_p) > t:  e_p *= t/lum(e_p) per channel
//   initial variance, 7x7 window inside the frame, dy outer, dx inner: wg = wn*wp (0 if hit_p != hit_q), taps with wg > 0 only:
//     v_p = sum(wg*h2_q) / sum(wg)   (sum(wg) not > 0: v_p = h2_p)
//   pass i, step s = 2^i:
//     vb_p = sum(k3*v_q) / sum(k3) over the 3x3 taps q = p + s*(dx, dy) inside the frame, k3 = k3[dx]*k3[dy], {1/4, 1/2, 1/4}
//     d = lum(e_p) - lum(e_q);  wc = fmaxf(0, 1 - ((d*d)*sv) / (vb_p + 1e-6f));  w = ((k5*wc)*wn)*wp (0 if hit_p != hit_q)
//     taps with w > 0 only: e'_p = sum(w*e_q) / sum(w), v'_p = sum((w*w)*v_q) / (sum(w)*sum(w))   (sum(w) not > 0: both unchanged)
//   c'_p = e'_p * D_p
#pragma once
#include "mrt_denoise.h"

namespace mrt {

constexpr float kDnvEps = 1e-6f;

MRT_HD float dnv_lum(const float *v) { return (0.2126f * v[0] + 0.7152f * v[1]) + 0.0722f * v[2]; }

MRT_HD bool dnv_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }      // false for NaN

// e (demodulated mean) of one pixel from its sums, albedo and hit flag at count n
MRT_HD void dnv_mean(const float *A, const float *alb, float hit, u32 n, bool env, float *e)
{
    const float rc = 1.0f / (float)n;
    for (int c = 0; c < 3; ++c) e[c] = (A[c] * rc) / dn_demod(alb[c], hit, env);
}

// h2 of one pixel: the squared half difference of its two half-buffer estimates' luminances
MRT_HD float dnv_h2(const float *A, const float *H, const float *alb, float hit, u32 n, bool env)
{
    const float rh = 1.0f / (float)(n >> 1);
    float j[3], k[3];
    for (int c = 0; c < 3; ++c) {
        const float D = dn_demod(alb[c], hit, env);
        j[c] = (H[c] * rh) / D;
        k[c] = ((A[c] - H[c]) * rh) / D;
    }
    const float h = (dnv_lum(j) - dnv_lum(k)) * 0.5f;
    return dnv_finite(h) ? h * h : 0.0f;
}

// The largest neighbour luminance so far: start at -inf, one call per neighbour with hit_q == hit_p
MRT_HD float dnv_firefly_max(float m, float lum_q) { return __builtin_fmaxf(m, lum_q); }

// The firefly clamp of e_p against the neighbour maximum m (have: at least one neighbour took part)
MRT_HD void dnv_firefly(float *e, bool have, float m, float f)
{
    const float lp = dnv_lum(e), t = f * m;
    if (!(have && dnv_finite(lp) && t >= 0.0f && lp > t)) return;
    const float sc = t / lp;
    e[0] *= sc; e[1] *= sc; e[2] *= sc;
}

// Guide terms of tap q for pixel p (dn_tap_weight's wn and wp); false: hit_p != hit_q, the tap has weight 0
MRT_HD bool dnv_guide(const DnGuide &gp, const DnGuide &gq, float sn, float sp, float &wn, float &wp)
{
    if (gp.hit != gq.hit) return false;
    wn = 1.0f; wp = 1.0f;
    if (gp.hit != 0.0f) {
        const float mx = gp.nx - gq.nx, my = gp.ny - gq.ny, mz = gp.nz - gq.nz;
        wn = __builtin_fmaxf(0.0f, 1.0f - ((mx * mx + my * my) + mz * mz) * sn);
        const float ux = gq.px - gp.px, uy = gq.py - gp.py, uz = gq.pz - gp.pz;
        const float r = ((gp.nx * ux + gp.ny * uy) + gp.nz * uz) / gp.t;
        wp = __builtin_fmaxf(0.0f, 1.0f - (r * r) * sp);
    }
    return true;
}

// running sums of the initial variance of one pixel
struct DnvInit {
    float num = 0.0f, den = 0.0f;
    MRT_HD void add(const DnGuide &gp, const DnGuide &gq, float sn, float sp, float h2q)
    {
        float wn, wp;
        if (!dnv_guide(gp, gq, sn, sp, wn, wp)) return;
        const float wg = wn * wp;
        if (!(wg > 0.0f)) return;
        num += wg * h2q; den += wg;
    }
    MRT_HD float result(float h2p) const { return den > 0.0f ? num / den : h2p; }
};

// 3x3 prefilter taps, k3[d + 1]
MRT_HD float dnv_k3(int i) { return i == 0 ? 0.5f : 0.25f; }

struct DnvBlur {
    float num = 0.0f, den = 0.0f;
    MRT_HD void add(int dx, int dy, float vq) { const float k = dnv_k3(dx) * dnv_k3(dy); num += k * vq; den += k; }
    MRT_HD float result() const { return num / den; }
};

// weight of tap q for pixel p in a pass: k = k5[dx] * k5[dy], lp / lq the luminances of e_p / e_q, vb the prefiltered variance of p
MRT_HD float dnv_tap_weight(float k, float lp, float lq, float vb, const DnGuide &gp, const DnGuide &gq, float sv, float sn, float sp)
{
    float wn, wp;
    if (!dnv_guide(gp, gq, sn, sp, wn, wp)) return 0.0f;
    const float d = lp - lq;
    const float wc = __builtin_fmaxf(0.0f, 1.0f - ((d * d) * sv) / (vb + kDnvEps));
    return ((k * wc) * wn) * wp;
}

// running sums of one pixel's taps in a pass
struct DnvAcc {
    float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f, den = 0.0f, vn = 0.0f;
    MRT_HD void add(float w, const float *eq, float vq)
    {
        if (!(w > 0.0f)) return;
        n0 += w * eq[0]; n1 += w * eq[1]; n2 += w * eq[2]; den += w; vn += (w * w) * vq;
    }
    MRT_HD void result(const float *ep, float vp, float *out, float &vout) const
    {
        if (den > 0.0f) { out[0] = n0 / den; out[1] = n1 / den; out[2] = n2 / den; vout = vn / (den * den); }
        else { out[0] = ep[0]; out[1] = ep[1]; out[2] = ep[2]; vout = vp; }
    }
};

// ---- whole frames on the host (x86 build): ev = (e.r, e.g, e.b, h2 or v) per pixel ----
// prep: e and h2 of every pixel, the firefly clamp applied (f = +inf: off)
inline void dnv_prep_host(const float *A, const float *H, const u32 *counts, const DnGuide *g, const float *alb, u32 nw, u32 nh, bool env, float f,
                          float *ev)
{
    const size_t np = (size_t)nw * nh;
    for (size_t p = 0; p < np; ++p) {
        dnv_mean(A + 3 * p, alb + 3 * p, g[p].hit, counts[p], env, ev + 4 * p);
        ev[4 * p + 3] = dnv_h2(A + 3 * p, H + 3 * p, alb + 3 * p, g[p].hit, counts[p], env);
    }
    if (!dnv_finite(f)) return;
    float *cl = new float[np * 3];
    for (u32 y = 0; y < nh; ++y)
        for (u32 x = 0; x < nw; ++x) {
            const size_t p = (size_t)y * nw + x;
            float m = -__builtin_inff();
            bool have = false;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const long long qx = (long long)x + dx, qy = (long long)y + dy;
                    if ((dx == 0 && dy == 0) || qx < 0 || qy < 0 || qx >= (long long)nw || qy >= (long long)nh) continue;
                    const size_t q = (size_t)qy * nw + (size_t)qx;
                    if (g[q].hit != g[p].hit) continue;
                    have = true;
                    m = dnv_firefly_max(m, dnv_lum(ev + 4 * q));
                }
            float e[3] = {ev[4 * p], ev[4 * p + 1], ev[4 * p + 2]};
            dnv_firefly(e, have, m, f);
            cl[3 * p] = e[0]; cl[3 * p + 1] = e[1]; cl[3 * p + 2] = e[2];
        }
    for (size_t p = 0; p < np; ++p) { ev[4 * p] = cl[3 * p]; ev[4 * p + 1] = cl[3 * p + 1]; ev[4 * p + 2] = cl[3 * p + 2]; }
    delete[] cl;
}

// initial variance: out = (e, v) of every pixel from in = (e, h2)
inline void dnv_init_host(const float *in, const DnGuide *g, u32 nw, u32 nh, float sn, float sp, float *out)
{
    for (u32 y = 0; y < nh; ++y)
        for (u32 x = 0; x < nw; ++x) {
            const size_t p = (size_t)y * nw + x;
            DnvInit acc;
            for (int dy = -3; dy <= 3; ++dy)
                for (int dx = -3; dx <= 3; ++dx) {
                    const long long qx = (long long)x + dx, qy = (long long)y + dy;
                    if (qx < 0 || qy < 0 || qx >= (long long)nw || qy >= (long long)nh) continue;
                    const size_t q = (size_t)qy * nw + (size_t)qx;
                    acc.add(g[p], g[q], sn, sp, in[4 * q + 3]);
                }
            out[4 * p] = in[4 * p]; out[4 * p + 1] = in[4 * p + 1]; out[4 * p + 2] = in[4 * p + 2];
            out[4 * p + 3] = acc.result(in[4 * p + 3]);
        }
}

// one pass at `step`: out = (e', v') of every pixel from in = (e, v)
inline void dnv_pass_host(const float *in, const DnGuide *g, u32 nw, u32 nh, u32 step, float sv, float sn, float sp, float *out)
{
    for (u32 y = 0; y < nh; ++y)
        for (u32 x = 0; x < nw; ++x) {
            const size_t p = (size_t)y * nw + x;
            DnvBlur vb;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const long long qx = (long long)x + (long long)step * dx, qy = (long long)y + (long long)step * dy;
                    if (qx < 0 || qy < 0 || qx >= (long long)nw || qy >= (long long)nh) continue;
                    vb.add(dx, dy, in[4 * ((size_t)qy * nw + (size_t)qx) + 3]);
                }
            const float b = vb.result(), lp = dnv_lum(in + 4 * p);
            DnvAcc acc;
            for (int dy = -2; dy <= 2; ++dy)
                for (int dx = -2; dx <= 2; ++dx) {
                    const long long qx = (long long)x + (long long)step * dx, qy = (long long)y + (long long)step * dy;
                    if (qx < 0 || qy < 0 || qx >= (long long)nw || qy >= (long long)nh) continue;
                    const size_t q = (size_t)qy * nw + (size_t)qx;
                    acc.add(dnv_tap_weight(dn_k5(dx) * dn_k5(dy), lp, dnv_lum(in + 4 * q), b, g[p], g[q], sv, sn, sp), in + 4 * q, in[4 * q + 3]);
                }
            acc.result(in + 4 * p, in[4 * p + 3], out + 4 * p, out[4 * p + 3]);
        }
}

}  // namespace mrt
