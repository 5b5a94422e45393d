"""TEST INFRASTRUCTURE: the variance-guided denoiser mode restated in numpy float32, in the operation order of
csrc/mrt_denoise_var.h, and the x86 build of that header (tests/emu/var_probe.cpp) behind ctypes."""
import ctypes as C

import numpy as np

from emu.build import ptr as _p, shared

f32 = np.float32
K5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], f32)
K3 = np.array([1 / 4, 1 / 2, 1 / 4], f32)
EPS = f32(1e-6)
INF = float("inf")


def _bind(L):
    fp, u32p, u32, f = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_uint32, C.c_float
    L.dv_prep.argtypes = [fp, fp, u32p, fp, fp, u32, u32, u32, f, fp]
    L.dv_filter.argtypes = [fp, fp, u32p, fp, fp, u32, u32, u32, f, f, f, f, u32, fp, fp]


def shared_probe():
    return shared("var_probe", _bind, with_pack=False)


def inv_sq(sigma):
    s = f32(sigma)
    with np.errstate(over="ignore"):
        return f32(f32(1.0) / (s * s))


def _c(a, t=f32):
    return np.ascontiguousarray(a, t)


def x86_prep(L, A, H, counts, g, alb, firefly, env=False):
    nh, nw = counts.shape
    ev = np.zeros((nh, nw, 4), f32)
    L.dv_prep(_p(_c(A)), _p(_c(H)), _p(_c(counts, np.uint32), C.c_uint32), _p(_c(g)), _p(_c(alb)), nw, nh, int(env), firefly, _p(ev))
    return ev


def x86_filter(L, A, H, counts, g, alb, passes, sv, sn, sp, firefly, env=False, want_var=False):
    """sv, sn, sp: the 1/sigma^2 (inv_sq); firefly: the factor, inf = off."""
    nh, nw = counts.shape
    out = np.zeros((nh, nw, 3), f32)
    var = np.zeros((nh, nw), f32) if want_var else None
    L.dv_filter(_p(_c(A)), _p(_c(H)), _p(_c(counts, np.uint32), C.c_uint32), _p(_c(g)), _p(_c(alb)), nw, nh, passes, sv, sn, sp, firefly,
                int(env), _p(out), _p(var) if want_var else None)
    return (out, var) if want_var else out


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    both_nan = np.isnan(a) & np.isnan(b)
    return int(np.count_nonzero((a.view(np.uint32) != b.view(np.uint32)) & ~both_nan))


# ---- numpy ---------------------------------------------------------------------------------------------------------------
def lum(v):
    return (f32(0.2126) * v[..., 0] + f32(0.7152) * v[..., 1]) + f32(0.0722) * v[..., 2]


def _shift(nh, nw, oy, ox):
    """Index arrays of the taps p + (ox, oy), clipped, and the mask of taps inside the frame."""
    ys, xs = np.arange(nh) + oy, np.arange(nw) + ox
    inside = ((ys >= 0) & (ys < nh))[:, None] & ((xs >= 0) & (xs < nw))[None, :]
    return np.clip(ys, 0, nh - 1), np.clip(xs, 0, nw - 1), inside


def _take(a, yq, xq):
    return a[yq][:, xq]


def demod(g, alb, env):
    hit = g[..., 7]
    return np.where(((hit != 0) | bool(env))[..., None], np.fmax(alb, f32(1 / 256)), f32(1.0)).astype(f32)


def np_prep(A, H, counts, g, alb, firefly, env=False):
    """(e, h2) [nh][nw][4]: the demodulated mean, firefly-clamped, and the squared half difference."""
    nh, nw = counts.shape
    hit = g[..., 7]
    with np.errstate(all="ignore"):
        D = demod(g, alb, env)
        rc = (f32(1.0) / counts.astype(f32))[..., None]
        rh = (f32(1.0) / (counts // 2).astype(f32))[..., None]
        e = (A * rc) / D
        j = (H * rh) / D
        k = ((A - H) * rh) / D
        h = (lum(j) - lum(k)) * f32(0.5)
        h2 = np.where(np.isfinite(h), h * h, f32(0)).astype(f32)
        if np.isfinite(firefly):
            le = lum(e)
            m = np.full((nh, nw), -np.inf, f32)
            have = np.zeros((nh, nw), bool)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dx == 0 and dy == 0:
                        continue
                    yq, xq, inside = _shift(nh, nw, dy, dx)
                    ok = inside & (_take(hit, yq, xq) == hit)
                    have |= ok
                    m = np.where(ok, np.fmax(m, _take(le, yq, xq)), m)
            t = f32(firefly) * m
            clamp = have & np.isfinite(le) & (t >= 0) & (le > t)
            e = np.where(clamp[..., None], e * (t / le)[..., None], e).astype(f32)
    return np.concatenate([e, h2[..., None]], -1).astype(f32)


def _guide_terms(g, yq, xq, inside, sn, sp):
    """wn, wp of every pixel's tap and the mask of taps that may have weight (inside the frame, equal hit flag)."""
    hit, n, t, x = g[..., 7], g[..., 0:3], g[..., 3], g[..., 4:7]
    hq, nq, xq_ = _take(hit, yq, xq), _take(n, yq, xq), _take(x, yq, xq)
    m = n - nq
    wn = np.fmax(f32(0), f32(1) - ((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]) * f32(sn))
    u = xq_ - x
    r = ((n[..., 0] * u[..., 0] + n[..., 1] * u[..., 1]) + n[..., 2] * u[..., 2]) / t
    wp = np.fmax(f32(0), f32(1) - (r * r) * f32(sp))
    on = hit != 0
    return np.where(on, wn, f32(1)).astype(f32), np.where(on, wp, f32(1)).astype(f32), inside & (hit == hq)


def np_init(ev, g, sn, sp):
    """(e, v): the 7x7 guide-weighted mean of h2."""
    nh, nw = ev.shape[:2]
    h2 = ev[..., 3]
    num = np.zeros((nh, nw), f32)
    den = np.zeros((nh, nw), f32)
    with np.errstate(all="ignore"):
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                yq, xq, inside = _shift(nh, nw, dy, dx)
                wn, wp, ok = _guide_terms(g, yq, xq, inside, sn, sp)
                wg = np.where(ok, wn * wp, f32(0)).astype(f32)
                use = wg > 0
                num = np.where(use, num + wg * _take(h2, yq, xq), num)
                den = np.where(use, den + wg, den)
        v = np.where(den > 0, num / den, h2).astype(f32)
    out = ev.copy()
    out[..., 3] = v
    return out


def np_pass(ev, g, step, sv, sn, sp):
    nh, nw = ev.shape[:2]
    e, v = ev[..., 0:3], ev[..., 3]
    with np.errstate(all="ignore"):
        bn = np.zeros((nh, nw), f32)
        bd = np.zeros((nh, nw), f32)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                yq, xq, inside = _shift(nh, nw, step * dy, step * dx)
                k = f32(K3[dx + 1] * K3[dy + 1])
                bn = np.where(inside, bn + k * _take(v, yq, xq), bn)
                bd = np.where(inside, bd + k, bd)
        vb = bn / bd
        le = lum(e)
        num = np.zeros_like(e)
        den = np.zeros((nh, nw), f32)
        vn = np.zeros((nh, nw), f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                yq, xq, inside = _shift(nh, nw, step * dy, step * dx)
                wn, wp, ok = _guide_terms(g, yq, xq, inside, sn, sp)
                eq, vq = _take(e, yq, xq), _take(v, yq, xq)
                d = le - _take(le, yq, xq)
                wc = np.fmax(f32(0), f32(1) - ((d * d) * f32(sv)) / (vb + EPS))
                k = f32(K5[dx + 2] * K5[dy + 2])
                w = np.where(ok, ((k * wc) * wn) * wp, f32(0)).astype(f32)
                use = w > 0
                num = np.where(use[..., None], num + w[..., None] * eq, num)
                den = np.where(use, den + w, den)
                vn = np.where(use, vn + (w * w) * vq, vn)
        on = den > 0
        e2 = np.where(on[..., None], num / den[..., None], e).astype(f32)
        v2 = np.where(on, vn / (den * den), v).astype(f32)
    return np.concatenate([e2, v2[..., None]], -1).astype(f32)


def np_chain(A, H, counts, g, alb, max_passes, sv, sn, sp, firefly, env=False):
    """The filter's output for passes = 0..max_passes (each pass's output does not depend on how many follow) and the variance
    plane after each: lists indexed by the pass count."""
    with np.errstate(all="ignore"):
        D = demod(g, alb, env)
        outs = [(A * (f32(1.0) / counts.astype(f32))[..., None]).astype(f32)]
        ev = np_init(np_prep(A, H, counts, g, alb, firefly, env), g, sn, sp)
        var = [ev[..., 3]]
        for i in range(max_passes):
            ev = np_pass(ev, g, 1 << i, sv, sn, sp)
            outs.append((ev[..., 0:3] * D).astype(f32))
            var.append(ev[..., 3])
    return outs, var


def np_filter(A, H, counts, g, alb, passes, sv, sn, sp, firefly, env=False):
    return np_chain(A, H, counts, g, alb, passes, sv, sn, sp, firefly, env)[0][passes]
