"""TEST INFRASTRUCTURE for tests/test_filter_host.py and tests/test_gpu_filter.py: the x86 probe of the bilinear texture filter
(tests/emu/filter_probe.cpp), the float32 numpy restatement of DESIGN.md §16, float64 bilinear references that share no code
with the kernels (the closed-form renders of a mirror sphere under a filtered environment and of a textured plane / sphere
under a point light) and scene builders.  Packing, AOVs and whole renders with the filter switches go through the probe of
tests/env_ref.py, whose entry points take any mrt_desc_ext."""
import copy
import ctypes as C

import numpy as np

import env_ref as E
from conftest import make_holder
from emu.build import ptr as _p, shared
from vattr_ref import camera_rays

f32 = np.float32
FMT_NONE, FMT_F32, FMT_U8 = 0, 1, 2
LUT = (np.arange(256, dtype=f32) / f32(255.0)).astype(f32)          # the packer's k/255 table
BILINEAR_MAX = f32(2.0 ** 30)


# ---- the probe ---------------------------------------------------------------------------------------------------------------
def _bind(L):
    fp, vp, u32 = C.POINTER(C.c_float), C.c_void_p, C.c_uint32
    L.fl_core.argtypes = [u32, u32, u32, vp, u32, u32, fp, fp]
    L.fl_core.restype = None
    L.fl_tex.argtypes = [u32, u32, u32, vp, u32, u32, u32, u32, fp, fp]
    L.fl_tex.restype = None
    L.fl_env.argtypes = [u32, u32, u32, vp, u32, C.c_float, u32, u32, fp, fp, fp]
    L.fl_env.restype = None
    L.fl_params_offsets.argtypes = [C.POINTER(u32)]
    L.fl_params_offsets.restype = None


def shared_probe():
    return shared("filter_probe", _bind, with_pack=False)


def params_offsets(L):
    out = (C.c_uint32 * 4)()
    L.fl_params_offsets(out)
    return dict(zip(("off_mat", "n_rend", "off_env", "off_rend"), (int(v) for v in out)))


class Tex:
    """A w x h texture as the blob holds it: fmt FMT_F32 (dat float32) or FMT_U8 (dat uint8, read through the LUT)."""

    def __init__(self, w, h, dat, fmt):
        self.w, self.h, self.fmt = w, h, fmt
        self.raw = np.ascontiguousarray(dat, np.uint8 if fmt == FMT_U8 else f32).reshape(h, w, 3)
        self.val = LUT[self.raw] if fmt == FMT_U8 else self.raw       # (h, w, 3) float32: what a fetch returns

    def ptr(self):
        return self.raw.ctypes.data_as(C.c_void_p)


def random_tex(w, h, fmt, seed):
    rng = np.random.default_rng(seed)
    if fmt == FMT_U8:
        return Tex(w, h, rng.integers(0, 256, (h, w, 3)), fmt)
    return Tex(w, h, rng.uniform(0.0, 9.0, (h, w, 3)), fmt)


def x86_core(L, t, uv, clamp_v):
    uv = np.ascontiguousarray(uv, f32)
    out = np.zeros((uv.shape[0], 3), f32)
    L.fl_core(t.w, t.h, t.fmt, t.ptr(), 1 if clamp_v else 0, uv.shape[0], _p(uv), _p(out))
    return out


def x86_tex(L, t, uv, filtered, clamp_v=False, cold=False):
    uv = np.ascontiguousarray(uv, f32)
    out = np.zeros((uv.shape[0], 3), f32)
    L.fl_tex(t.w, t.h, t.fmt, t.ptr(), 1 if filtered else 0, 1 if clamp_v else 0, 1 if cold else 0, uv.shape[0], _p(uv), _p(out))
    return out


def x86_env(L, t, mapping, rot, filtered, d):
    d = np.ascontiguousarray(d, f32)
    out, uv = np.zeros((d.shape[0], 3), f32), np.zeros((d.shape[0], 2), f32)
    L.fl_env(t.w, t.h, t.fmt, t.ptr(), E.MAPPINGS.index(mapping), float(f32(rot)), 1 if filtered else 0, d.shape[0], _p(d), _p(out), _p(uv))
    return out, uv


# ---- DESIGN.md §16 in float32 numpy, in its operation order ---------------------------------------------------------------------
def _wrap(i, n):
    """ix mod n for |ix| <= n; beyond that clamped into the texture (the contract's callers never get there)."""
    i = np.where(i < 0, i + n, i)
    i = np.where(i >= n, i - n, i)
    return np.clip(i, 0, n - 1)


def np_taps(u, v, w, h, clamp_v):
    """(ok, x0, x1, y0, y1, fx, fy) of §16 for float32 coordinates; where ok is False the other values mean nothing."""
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    with np.errstate(all="ignore"):
        x = u * f32(w) - f32(0.5)
        y = v * f32(h) - f32(0.5)
        ok = (np.abs(x) < BILINEAR_MAX) & (np.abs(y) < BILINEAR_MAX)       # false for NaN and inf
    x, y = np.where(ok, x, f32(0)).astype(f32), np.where(ok, y, f32(0)).astype(f32)
    xf, yf = np.trunc(x), np.trunc(y)
    xf = np.where(xf > x, xf - f32(1), xf).astype(f32)
    yf = np.where(yf > y, yf - f32(1), yf).astype(f32)
    fx, fy = (x - xf).astype(f32), (y - yf).astype(f32)
    ix, iy = xf.astype(np.int64), yf.astype(np.int64)
    x0 = _wrap(ix, w)
    x1 = np.where(x0 + 1 >= w, 0, x0 + 1)
    if clamp_v:
        y0, y1 = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    else:
        y0 = _wrap(iy, h)
        y1 = np.where(y0 + 1 >= h, 0, y0 + 1)
    return ok, x0, x1, y0, y1, fx, fy


def np_bilinear(t, u, v, clamp_v):
    """(colour float32 (n, 3), ok) of the filter on Tex t: every operation a float32 one, multiply then add, no FMA."""
    ok, x0, x1, y0, y1, fx, fy = np_taps(u, v, t.w, t.h, clamp_v)
    t00, t10, t01, t11 = t.val[y0, x0], t.val[y0, x1], t.val[y1, x0], t.val[y1, x1]
    fx, fy = fx[:, None], fy[:, None]
    top = t00 + fx * (t10 - t00)
    bot = t01 + fx * (t11 - t01)
    out = top + fy * (bot - top)
    assert out.dtype == f32
    return out, ok


def np_nearest(t, u, v):
    """tex_fetch's rule on Tex t."""
    idx = E.np_env_index(np.stack([np.asarray(u, f32), np.asarray(v, f32)], 1), t.w, t.h)
    return t.val.reshape(-1, 3)[idx]


def bilinear64(val, u, v, clamp_v):
    """Bilinear interpolation of the (h, w, 3) texels in float64: u repeats, v repeats or clamps; texel centres at i + 0.5."""
    val = np.asarray(val, np.float64)
    h, w = val.shape[:2]
    x, y = np.asarray(u, np.float64) * w - 0.5, np.asarray(v, np.float64) * h - 0.5
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf)[:, None], (y - yf)[:, None]
    ix, iy = xf.astype(np.int64), yf.astype(np.int64)
    x0, x1 = ix % w, (ix + 1) % w
    if clamp_v:
        y0, y1 = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    else:
        y0, y1 = iy % h, (iy + 1) % h
    top = val[y0, x0] * (1 - fx) + val[y0, x1] * fx
    bot = val[y1, x0] * (1 - fx) + val[y1, x1] * fx
    return top * (1 - fy) + bot * fy


def bound64(t, clamp_v):
    """|float32 filter - float64 filter| per channel, for coordinates in [0, 1] that are the same numbers in both:
    x = u * w - 0.5 is rounded twice, each time by at most 2^-24 of a magnitude <= w, so |dx| <= w * 2^-23 texels (|dy| <= h *
    2^-23); the interpolant is continuous and piecewise linear with slope at most Dx (Dy): the largest difference between
    horizontally (vertically) adjacent texels, wrap-around pairs included; the three lerps are 9 float32 operations on
    magnitudes <= M, the largest texel, whose errors add up to at most 12 * 2^-24 * M (top and bot: 3 each; the last lerp doubles
    what it subtracts and adds 3 of its own)."""
    val = t.val.astype(np.float64)
    dx = np.abs(val - np.roll(val, 1, axis=1)).max()
    dy = np.abs(val - np.roll(val, 1, axis=0)).max() if not clamp_v or t.h > 1 else 0.0
    return (t.w * dx + t.h * dy) * 2.0 ** -23 + 12 * 2.0 ** -24 * val.max()


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def with_filters(desc, sky=None, tex=None):
    """desc (a scenes.* dict) with "filter" on its sky and / or its scene."""
    if sky is not None:
        desc["scene"]["sky"]["filter"] = sky
    if tex is not None:
        desc["scene"]["filter"] = tex
    return desc


def one_texel_textures(desc):
    """desc with every material texture replaced by a 1 x 1 texture holding its first texel."""
    desc = copy.deepcopy(desc)
    n = 0
    for r in desc["scene"]["renderer"]:
        for k in ("tex", "rmap", "mmap", "gmap", "omap", "emap"):
            t = (r.get("mat") or {}).get(k)
            if isinstance(t, dict):
                r["mat"][k] = {"w": 1, "h": 1, "dat": [[float(c) for c in np.asarray(t["dat"], np.float64).reshape(-1, 3)[0]]]}
                n += 1
    assert n > 0
    return desc


def smooth_tex(w=16, h=8):
    """A smooth material texture, values 0.25 .. 0.95, not on the k/255 lattice (the f32 layout)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r = 0.6 + 0.3 * np.sin(2 * np.pi * x / w + 0.3) * np.cos(2 * np.pi * y / h)
    g = 0.55 + 0.3 * np.cos(2 * np.pi * x / w) * np.sin(2 * np.pi * (y + 0.5) / h)
    b = 0.6 + 0.35 * np.cos(2 * np.pi * (y + 0.5) / h + 0.2)
    return {"w": w, "h": h, "dat": np.stack([r, g, b], -1).reshape(-1, 3).astype(f32) + f32(1e-3)}


LIGHT_POS, LIGHT_PWR, LIGHT_COLOR = (0.2, -2.5, 0.3), 0.8, (1.0, 0.9, 0.8)      # close to the view axis: every visible point is lit
MAT_ALBEDO = (0.9, 0.8, 0.7)
PLANE_N, PLANE_POS = (0.0, -1.0, 1.0), (0.0, 1.0, 0.0)


def lit_scene(kind, filt, res=(96, 64), sample=2):
    """One textured renderer (rough 1, metal 0, opaque, emit 0) under one point light, black sky, bounce 0, aprt 0: every sample
    of a pixel is albedo x texture(uv) x max(n . l, 0) x light colour x light power at its first hit.  kind "sphere": r 0.5 at the
    origin; "plane": the slope z = y - 1 facing the default camera, which every camera ray hits within ~10 units."""
    mat = {"rough": 1, "metal": 0, "opacity": 1, "emit": 0, "albedo": list(MAT_ALBEDO), "tex": smooth_tex()}
    rend = {"type": "sphere", "r": 0.5, "mat": mat} if kind == "sphere" else {"type": "plane", "n": list(PLANE_N), "pos": list(PLANE_POS), "mat": mat}
    d = {"rt": {"bounce": 0, "sample": sample, "loss": 0.15},
         "frame": {"res": list(res), "ssaa": 1, "cam": {"aprt": 0}},
         "scene": {"renderer": [rend], "light": [{"type": "point", "pos": list(LIGHT_POS), "pwr": LIGHT_PWR, "color": list(LIGHT_COLOR)}],
                   "sky": {"color": [0, 0, 0], "pwr": 0.5}}}
    return with_filters(d, tex=filt)


def _lookup64(tex, u, v, clamp_v, filt, tol=1e-3):
    """(texel colour float64, near) under the filter: near = within tol texels of a place where the float32 and the float64
    lookup may land in different cells (nearest: a texel boundary; bilinear: a texel centre line)."""
    val = np.asarray(tex.dat, np.float64).reshape(tex.h, tex.w, 3)
    if filt == "bilinear":
        x, y = u * tex.w - 0.5, v * tex.h - 0.5
        near = (np.abs(x - np.round(x)) < tol) | (np.abs(y - np.round(y)) < tol)
        return bilinear64(val, u, v, clamp_v), near
    fx, fy = u * tex.w, v * tex.h
    near = (np.abs(fx - np.round(fx)) < tol) | (np.abs(fy - np.round(fy)) < tol)
    ix, iy = np.minimum(fx.astype(np.int64), tex.w - 1), np.minimum(fy.astype(np.int64), tex.h - 1)
    return val[iy, ix], near


def _ring(hit2):
    m = np.pad(hit2, 1, mode="edge")
    return (m[:-2, 1:-1] != hit2) | (m[2:, 1:-1] != hit2) | (m[1:-1, :-2] != hit2) | (m[1:-1, 2:] != hit2)


def mirror_closed_form(render):
    """env_ref.closed_form under the sky's filter: (image, hit mask, near mask, ring mask)."""
    nw, nh = render.frame.res
    sky = render.scene.sky
    o, d = camera_rays(render)
    b = np.sum(o * d, 1)
    disc = b * b - (np.sum(o * o, 1) - 0.25)
    hit = disc > 0
    t = -b - np.sqrt(np.where(hit, disc, 0.0))
    n = o + d * t[:, None]
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    refl = d - 2.0 * np.sum(d * n, 1)[:, None] * n
    look = np.where(hit[:, None], refl, d)
    uv = E.env_uv64(sky.mapping, sky.rot, look)
    texel, near = _lookup64(sky.tex, uv[:, 0], uv[:, 1], True, sky.filter)
    color = np.asarray(sky.color, np.float64)
    alb = np.asarray(render.scene.renderer[0].mat.albedo, np.float64)
    img = np.where(hit[:, None], (0.5 + alb) * color * texel * float(sky.pwr), color * texel)
    hit2 = hit.reshape(nh, nw)
    return img.reshape(nh, nw, 3), hit2, near.reshape(nh, nw), _ring(hit2)


def lit_closed_form(render):
    """Float64 image of lit_scene: (image, hit mask, near mask, ring mask)."""
    nw, nh = render.frame.res
    r = render.scene.renderer[0]
    o, d = camera_rays(render)
    if r.kind == "sphere":
        b = np.sum(o * d, 1)
        disc = b * b - (np.sum(o * o, 1) - 0.25)
        hit = disc > 0
        t = -b - np.sqrt(np.where(hit, disc, 0.0))
        p = o + d * t[:, None]
        n = p / np.linalg.norm(p, axis=1, keepdims=True)
        u = 0.5 + np.arctan2(n[:, 0], -n[:, 1]) / (2.0 * np.pi)
        v = 0.5 - 0.5 * n[:, 2]
        clamp_v = True
    else:
        nn = np.asarray(PLANE_N, np.float64) / np.linalg.norm(PLANE_N)
        pos = np.asarray(PLANE_POS, np.float64)
        den = d @ nn
        t = ((pos - o) @ nn) / den
        hit = t > 0
        p = o + d * t[:, None]
        n = np.broadcast_to(nn, p.shape)
        q = p - pos                                       # the plane's UV: the hit point relative to the instance, wrapped
        u, v = (q[:, 0] + 0.5) % 1.0, (q[:, 1] + 0.5) % 1.0
        clamp_v = False
    texel, near = _lookup64(r.mat.tex, u, v, clamp_v, render.scene.tex_filter)
    l = np.asarray(LIGHT_POS, np.float64) - p
    l /= np.linalg.norm(l, axis=1, keepdims=True)
    diff = np.maximum(np.sum(l * n, 1), 0.0)[:, None]
    img = np.asarray(MAT_ALBEDO) * texel * diff * np.asarray(LIGHT_COLOR) * LIGHT_PWR
    img = np.where(hit[:, None], img, 0.0)
    hit2 = hit.reshape(nh, nw)
    return img.reshape(nh, nw, 3), hit2, near.reshape(nh, nw), _ring(hit2)


def check_closed(mean, want, hit, near, ring, filt, label, rtol=1e-4):
    """DESIGN.md §15's check under a filter.  A pixel outside the silhouette ring is EXCLUDED when it lies within 1e-3 texels of
    a place where float32 and float64 may pick different cells -- and, under the bilinear filter, differs visibly there (beyond
    rtol; the filter is continuous, so crossing a cell border shows nothing and such a pixel is compared like any other); every
    other pixel holds rtol.  At most 2 % of each class may be excluded under the bilinear filter.  Returns {class: (excluded pixels, pixels, worst)}."""
    out = {}
    for name, cls in (("miss", ~hit), ("hit", hit)):
        lit = cls & ~ring & (np.abs(want).max(-1) > 0)
        if lit.sum() == 0:
            continue
        rel = np.zeros(hit.shape)
        rel[lit] = (np.abs(mean[lit].astype(np.float64) - want[lit]) / np.maximum(np.abs(want[lit]), 1e-300)).max(-1)
        excl = lit & near & ((rel > rtol) if filt == "bilinear" else True)
        keep = lit & ~excl
        share = float(excl.sum()) / float((cls & ~ring).sum())
        worst = float(rel[keep].max())
        print(f"{label} {filt} {name}: {int(excl.sum())} pixels ({share:.2%}) excluded, {int(keep.sum())} compared, worst relative error {worst:.2e}")
        assert share <= 0.02 or filt == "nearest", (name, share)      # (the nearest run only supplies the count to beat)
        assert keep.sum() > 100 and worst <= rtol, (name, worst)
        out[name] = (int(excl.sum()), int((cls & ~ring).sum()), worst)
    return out
