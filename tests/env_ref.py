"""TEST INFRASTRUCTURE for tests/test_env_host.py and tests/test_gpu_env.py: the x86 probe of the environment-texture code
(tests/emu/env_probe.cpp), the float32 numpy restatement of DESIGN.md §15, float64 references that share no code with the
kernels (the mapping, the texture's mean, the closed-form render of a mirror sphere under an environment), scene builders and
a Radiance RGBE encoder."""
import ctypes as C

import numpy as np

from conftest import make_holder
from emu.build import desc_ptrs as _ptrs, ptr as _p, shared
from vattr_ref import camera_rays, same_bits

f32 = np.float32
kPi = f32(3.14159274101257324)
MAPPINGS = ("sphere", "latlong")


# ---- the probe ---------------------------------------------------------------------------------------------------------------
def _bind(L):
    fp, u32p, i32p, vp, u32 = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_void_p, C.c_uint32
    L.ev_error.restype = C.c_char_p
    L.ev_uv.argtypes = [u32, u32, C.c_float, u32, u32, fp, fp, u32p]
    L.ev_uv.restype = None
    L.ev_math.argtypes = [u32, u32, fp, fp, fp]
    L.ev_math.restype = None
    L.ev_sphere_uv.argtypes = [u32, fp, fp, fp]
    L.ev_sphere_uv.restype = None
    L.ev_pack.argtypes = [vp, vp, u32p, vp, u32p, C.c_uint64]
    L.ev_sky_init.argtypes = [vp, vp, fp]
    L.ev_aov.argtypes = [vp, vp, fp, fp, i32p]
    L.ev_aov_inst.argtypes = [vp, vp, fp, fp, i32p, i32p]
    L.ev_filter.argtypes = [fp, u32p, fp, fp, u32, u32, u32, C.c_float, C.c_float, C.c_float, u32, fp]
    L.ev_filter.restype = None
    L.ev_render.argtypes = [vp, vp, C.c_uint64, u32, u32, u32, u32, fp]


def shared_probe():
    """The probe, built once per process (about a minute) for every module that uses it."""
    return shared("env_probe", _bind)


def x86_uv(L, mapping, rot, d, w, h):
    d = np.ascontiguousarray(d, f32)
    n = d.shape[0]
    uv, idx = np.zeros((n, 2), f32), np.zeros(n, np.uint32)
    L.ev_uv(n, MAPPINGS.index(mapping), float(f32(rot)), w, h, _p(d), _p(uv), _p(idx, C.c_uint32))
    return uv, idx


def x86_math(L, op, a, b=None):
    a = np.ascontiguousarray(a, f32)
    b = np.zeros_like(a) if b is None else np.ascontiguousarray(b, f32)
    out = np.zeros_like(a)
    L.ev_math({"atan2": 0, "acos": 1, "div": 2}[op], a.size, _p(a), _p(b), _p(out))
    return out


def x86_sphere_uv(L, p):
    p = np.ascontiguousarray(p, f32)
    uv, nrm = np.zeros((p.shape[0], 2), f32), np.zeros_like(p)
    L.ev_sphere_uv(p.shape[0], _p(p), _p(uv), _p(nrm))
    return uv, nrm


PACK_KEYS = ("features", "blob_words", "lds_words", "lds_words_warm", "lds_words_hot", "off_env", "params_bytes", "walk_cap")


def x86_pack(L, holder, with_ext=True):
    """(info, Params bytes, blob words) of the packed scene; a rejected scene raises ValueError((code, message))."""
    d, e = _ptrs(holder, with_ext)
    info = np.zeros(8, np.uint32)
    rc = L.ev_pack(d, e, _p(info, C.c_uint32), None, None, 0)
    if rc:
        raise ValueError((rc, L.ev_error().decode()))
    info = dict(zip(PACK_KEYS, (int(v) for v in info)))
    params = np.zeros(info["params_bytes"], np.uint8)
    blob = np.zeros(info["blob_words"], np.uint32)
    assert L.ev_pack(d, e, _p(np.zeros(8, np.uint32), C.c_uint32), params.ctypes.data_as(C.c_void_p), _p(blob, C.c_uint32), blob.size) == 0
    return info, params, blob


def x86_sky_init(L, holder):
    out = np.zeros(3, f32)
    d, e = _ptrs(holder)
    rc = L.ev_sky_init(d, e, _p(out))
    assert rc == 0, L.ev_error()
    return out


def ss_dims(holder):
    """(nw, nh) of the supersampled frame the probe writes: `(res as f32 * ssaa) as usize` (src/sampler.rs:29-30), not frame.res."""
    fr = holder.desc.frame
    return int(f32(fr.res_w) * f32(fr.ssaa)), int(f32(fr.res_h) * f32(fr.ssaa))


def x86_aov(L, holder):
    nw, nh = ss_dims(holder)
    g, alb, rend = np.zeros((nh, nw, 8), f32), np.zeros((nh, nw, 3), f32), np.zeros((nh, nw), np.int32)
    d, e = _ptrs(holder)
    rc = L.ev_aov(d, e, _p(g), _p(alb), _p(rend, C.c_int32))
    assert rc == 0, L.ev_error()
    return g, alb, rend


def x86_aov_inst(L, holder):
    """x86_aov plus the instance plane (the index within the renderer's inst list, -1 on a miss)."""
    nw, nh = ss_dims(holder)
    g, alb, rend, inst = np.zeros((nh, nw, 8), f32), np.zeros((nh, nw, 3), f32), np.zeros((nh, nw), np.int32), np.zeros((nh, nw), np.int32)
    d, e = _ptrs(holder)
    rc = L.ev_aov_inst(d, e, _p(g), _p(alb), _p(rend, C.c_int32), _p(inst, C.c_int32))
    assert rc == 0, L.ev_error()
    return g, alb, rend, inst


def x86_render(L, holder, seed, n_samples, warm=False, sample_base=0, threads=8, with_ext=True):
    nw, nh = ss_dims(holder)
    acc = np.zeros((nh, nw, 3), f32)
    d, e = _ptrs(holder, with_ext)
    rc = L.ev_render(d, e, seed, sample_base, n_samples, threads, 1 if warm else 0, _p(acc))
    assert rc == 0, L.ev_error()
    return acc


def x86_filter(L, acc, counts, guide, albedo, env, passes=5, sigma=(0.5, 0.25, 0.05)):
    """mrt_denoise's contract on the sums acc at per-pixel counts; env: the miss pixels' divisor is their albedo too."""
    nh, nw = acc.shape[:2]
    a, c = np.ascontiguousarray(acc, f32), np.ascontiguousarray(counts, np.uint32)
    g, al = np.ascontiguousarray(guide, f32), np.ascontiguousarray(albedo, f32)
    out = np.zeros((nh, nw, 3), f32)
    inv = [float(f32(1.0) / (f32(s) * f32(s))) for s in sigma]
    L.ev_filter(_p(a), _p(c, C.c_uint32), _p(g), _p(al), nw, nh, passes, inv[0], inv[1], inv[2], 1 if env else 0, _p(out))
    return out


# ---- DESIGN.md §15 in float32 numpy, in its operation order; atan2_ / acos_ elementwise from the x86 build ----------------------------
def np_env_uv(L, mapping, rot, d):
    d = np.ascontiguousarray(d, f32)
    rot = f32(rot)
    with np.errstate(all="ignore"):
        a = x86_math(L, "atan2", d[:, 0], -d[:, 1])
        u0 = f32(0.5) + (f32(0.5) * a) / kPi
        u = u0 + rot
        u = u - np.trunc(u)
        u = np.where(u < 0, f32(1.0) + u, u).astype(f32)
        if mapping == "latlong":
            z = d[:, 2]
            c = np.where(np.isnan(z), f32(-1.0), np.minimum(np.maximum(z, f32(-1.0)), f32(1.0))).astype(f32)    # maxNum: NaN -> -1
            v = x86_math(L, "acos", c) / kPi
        else:
            v = f32(0.5) - f32(0.5) * d[:, 2]
    return np.stack([u, v.astype(f32)], 1)


def np_to_index(v):
    """`f32 as usize` of tex_fetch: NaN and negatives -> 0, saturating at 2^31."""
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        out = np.where(v > 0, np.minimum(v, f32(2147483648.0)), f32(0.0))
    return out.astype(np.int64)


def np_env_index(uv, w, h):
    x, y = np_to_index(uv[:, 0] * f32(w)), np_to_index(uv[:, 1] * f32(h))
    return np.minimum(x + y * w, w * h - 1)


def env_uv64(mapping, rot, d):
    """The mapping in float64, u wrapped into [0, 1)."""
    d = np.asarray(d, np.float64)
    u = 0.5 + np.arctan2(d[:, 0], -d[:, 1]) / (2.0 * np.pi) + float(rot)
    u = u - np.floor(u)
    v = np.arccos(np.clip(d[:, 2], -1.0, 1.0)) / np.pi if mapping == "latlong" else 0.5 - 0.5 * d[:, 2]
    return np.stack([u, v], 1)


def texel64(mapping, rot, d, tex, tol=1e-3):
    """(texel rgb float64, near) of directions d on Texture tex: nearest texel; near = (u w, v h) within tol of a texel boundary."""
    uv = env_uv64(mapping, rot, d)
    fx, fy = uv[:, 0] * tex.w, uv[:, 1] * tex.h
    near = (np.abs(fx - np.round(fx)) < tol) | (np.abs(fy - np.round(fy)) < tol)
    ix, iy = np.minimum(fx.astype(np.int64), tex.w - 1), np.minimum(fy.astype(np.int64), tex.h - 1)
    return np.asarray(tex.dat, np.float64).reshape(tex.h, tex.w, 3)[iy, ix], near


def mean64(tex, mapping):
    """The texture's solid-angle-weighted mean per channel: float64, summed in row-major order (np.cumsum adds sequentially),
    weights 1 ("sphere") or cos(pi y / h) - cos(pi (y + 1) / h) of row y ("latlong")."""
    t = np.asarray(tex.dat, np.float64).reshape(tex.h, tex.w, 3)
    y = np.arange(tex.h, dtype=np.float64)
    wy = np.cos(np.pi * y / tex.h) - np.cos(np.pi * (y + 1.0) / tex.h) if mapping == "latlong" else np.ones(tex.h)
    wt = np.repeat(wy, tex.w)
    num = np.cumsum(t.reshape(-1, 3) * wt[:, None], axis=0)[-1]
    den = np.cumsum(wt)[-1]
    return num / den


# ---- scenes --------------------------------------------------------------------------------------------------------------------
def const_env(value, w=3, h=2):
    return {"w": w, "h": h, "dat": np.full((w * h, 3), value, f32)}


def with_env(desc, tex, mapping="sphere", rot=0.0, color=None):
    """desc (a scenes.* dict) with an environment texture on its sky (the sky's colour and power are kept unless given)."""
    sky = dict(desc["scene"].get("sky") or {})
    if color is not None:
        sky["color"] = [float(c) for c in color]
    sky.update({"tex": tex, "map": mapping, "rot": rot})
    desc["scene"]["sky"] = sky
    return desc


def smooth_hdr(w=61, h=31):
    """A smooth procedural HDR texture, values 0.2 .. 7."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r = 1.2 + 0.9 * np.sin(2 * np.pi * x / w + 0.4) * np.cos(np.pi * y / h)
    g = 2.0 + 1.5 * np.cos(2 * np.pi * x / w) * np.sin(np.pi * (y + 0.5) / h)
    b = 4.0 + 3.0 * np.cos(np.pi * (y + 0.5) / h)
    return {"w": w, "h": h, "dat": np.stack([r, g, b], -1).reshape(-1, 3).astype(f32)}


def checker_env(w=256, h=128, lo=0.006, hi=0.12):
    """A one-texel checker of contrast 1 : 20, fine enough that a texel covers about two pixels of the 96 x 64 frame of
    denoise_scene (fov 70: ~1.2 pixels per degree, 1.4 degrees per texel).  Every miss pixel then has the other colour within
    two pixels on both axes, so at least two of the five B3 taps per axis (weight >= 0.0625 + 0.25 of 1) lie across an edge, and
    nothing but the colour term can keep a filter that does not know the backdrop from mixing the two.  The levels are low on
    purpose: under the sky colour (0.9, 0.8, 0.7) the dark texel stays above the denoiser's albedo floor of 1/256 in every
    channel (0.7 * 0.006 = 0.0042), and the squared colour distance across an edge, 0.114^2 * (0.81 + 0.64 + 0.49) = 0.025,
    leaves the colour term (1 - d^2 * 4 * 4^i) at 0.9 in pass 0 and 0.6 in pass 1."""
    y, x = np.mgrid[0:h, 0:w]
    v = np.where((x + y) % 2 == 0, lo, hi)
    return {"w": w, "h": h, "dat": np.repeat(v.reshape(-1, 1), 3, 1).astype(f32)}


ALBEDO = (0.3, 0.25, 0.2)


def closed_form_scene(mapping, res=(96, 64), tex=None, sample=4):
    """A mirror sphere (metal 1, rough 0, opaque, emit 0), r 0.5 at the origin, default camera with aprt 0, no lights, one bounce,
    under a smooth 61 x 31 HDR environment turned by 0.137: no random draw changes a path."""
    return {
        "rt": {"bounce": 1, "sample": sample, "loss": 0.15},
        "frame": {"res": list(res), "ssaa": 1, "cam": {"aprt": 0}},
        "scene": {"renderer": [{"type": "sphere", "r": 0.5, "mat": {"metal": 1, "rough": 0, "opacity": 1, "emit": 0, "albedo": list(ALBEDO)}}],
                  "sky": {"color": [0.9, 0.8, 0.7], "pwr": 0.6, "tex": smooth_hdr() if tex is None else tex, "map": mapping, "rot": 0.137}},
    }


def closed_form(render):
    """Mean radiance of closed_form_scene in float64: a primary miss is sky.color x texel(d); a sphere pixel is
    (0.5 + albedo) x sky.color x texel(reflect(d, n)) x sky.pwr.  Returns (image, hit mask, near-boundary mask, ring mask)."""
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
    texel, near = texel64(sky.mapping, sky.rot, look, sky.tex)
    color = np.asarray(sky.color, np.float64)
    alb = np.asarray(render.scene.renderer[0].mat.albedo, np.float64)
    img = np.where(hit[:, None], (0.5 + alb) * color * texel * float(sky.pwr), color * texel)
    hit2 = hit.reshape(nh, nw)
    m = np.pad(hit2, 1, mode="edge")
    ring = (m[:-2, 1:-1] != hit2) | (m[2:, 1:-1] != hit2) | (m[1:-1, :-2] != hit2) | (m[1:-1, 2:] != hit2)
    return img.reshape(nh, nw, 3), hit2, near.reshape(nh, nw), ring


def check_closed_form(mean, render, label):
    """rtol 1e-4 on every pixel outside the silhouette ring and the texel-boundary exclusion, of which at most 2 % of each class
    may fall to the boundary rule."""
    want, hit, near, ring = closed_form(render)
    worst = {}
    for name, cls in (("miss", ~hit), ("sphere", hit)):
        share = float(np.sum(near & cls & ~ring)) / float(np.sum(cls))
        keep = cls & ~near & ~ring
        rel = np.abs(mean[keep].astype(np.float64) - want[keep]) / np.abs(want[keep])
        worst[name] = (share, float(rel.max()), int(keep.sum()))
        print(f"{label} {render.scene.sky.mapping} {name}: {share:.2%} excluded at texel boundaries, {int(keep.sum())} pixels compared, "
              f"worst relative error {rel.max():.2e}")
        assert share <= 0.02, (name, share)
        assert keep.sum() > 100 and rel.max() <= 1e-4, (name, float(rel.max()))
    return worst


# ---- Radiance RGBE encoder (the loader's counterpart, written for the tests) -------------------------------------------------------
def rgbe_bytes(px, rle):
    """px: (h, w, 4) uint8 -> the body of a Radiance picture, flat or new-style run-length scanlines (which the format only
    has for 8 <= w < 32768)."""
    h, w = px.shape[:2]
    if not rle or w < 8:
        return px.tobytes()
    out = bytearray()
    for y in range(h):
        out += bytes([2, 2, w >> 8, w & 255])
        for ch in range(4):
            row = px[y, :, ch]
            x = 0
            while x < w:
                run = 1
                while x + run < w and run < 127 and row[x + run] == row[x]:
                    run += 1
                if run >= 3:
                    out += bytes([128 + run, int(row[x])])
                    x += run
                else:
                    n = 1
                    while x + n < w and n < 128 and not (x + n + 2 < w and row[x + n] == row[x + n + 1] == row[x + n + 2]):
                        n += 1
                    out += bytes([n]) + row[x:x + n].tobytes()
                    x += n
    return bytes(out)


def write_hdr(path, px, rle, magic=b"#?RADIANCE", res_line=None):
    h, w = px.shape[:2]
    res_line = res_line or f"-Y {h} +X {w}".encode()
    with open(path, "wb") as f:
        f.write(magic + b"\n# written by the tests\nFORMAT=32-bit_rle_rgbe\n\n" + res_line + b"\n" + rgbe_bytes(px, rle))


def rgbe_decode(px):
    e = px[..., 3].astype(np.int32)
    scale = np.where(e == 0, 0.0, np.ldexp(1.0, e - 136))
    return (px[..., :3].astype(np.float64) * scale[..., None]).astype(f32).reshape(-1, 3)
