"""TEST INFRASTRUCTURE for tests/test_vattr_host.py and tests/test_gpu_vattr.py: the x86 probe of the per-corner attribute code
(tests/emu/vattr_probe.cpp), the float32 numpy restatement of DESIGN.md §14, and float64 references that share no code with
the kernels: brute-force closest hits of the lens-centre rays and the closed-form render of a one-segment path."""
import ctypes as C

import numpy as np

from emu.build import desc_ptrs as _ptrs, ptr as _p, shared

f32 = np.float32
WARM = 0xFFFFFFFF      # deep_nodes value of the probe: the warm (F_COLD) lane code on the binary triangle BVHs


# ---- the probe ---------------------------------------------------------------------------------------------------------------
def _bind(L):
    fp, u32p, i32p, vp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_void_p
    L.va_error.restype = C.c_char_p
    L.va_interp.argtypes = [C.c_uint32] + [fp] * 9
    L.va_interp.restype = None
    L.va_mix.argtypes = [C.c_uint32] + [fp] * 6
    L.va_mix.restype = None
    L.va_pack.argtypes = [vp, vp, u32p, C.c_uint32, u32p]
    L.va_aov.argtypes = [vp, vp, C.c_uint32, fp, fp, i32p]
    L.va_render.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, fp]


def shared_probe():
    return shared("vattr_probe", _bind)


PACK_KEYS = ("features", "off_vattr", "n_vattr_rows", "blob_words", "lds_words", "lds_words_warm", "lds_words_hot", "off_rend")


def x86_pack(L, holder, with_ext=True):
    d, e = _ptrs(holder, with_ext)
    info = np.zeros(8, np.uint32)
    rc = L.va_pack(d, e, None, 0, _p(info, C.c_uint32))
    if rc:
        raise ValueError((rc, L.va_error().decode()))
    info = dict(zip(PACK_KEYS, (int(v) for v in info)))
    blob = np.zeros(info["blob_words"], np.uint32)
    assert L.va_pack(d, e, _p(blob, C.c_uint32), blob.size, _p(np.zeros(8, np.uint32), C.c_uint32)) == 0
    return info, blob


def x86_aov(L, holder, deep_nodes=0):
    nw, nh = holder.desc.frame.res_w, holder.desc.frame.res_h
    g = np.zeros((nh, nw, 8), f32)
    alb = np.zeros((nh, nw, 3), f32)
    rend = np.zeros((nh, nw), np.int32)
    d, e = _ptrs(holder)
    rc = L.va_aov(d, e, deep_nodes, _p(g), _p(alb), _p(rend, C.c_int32))
    assert rc == 0, L.va_error()
    return g, alb, rend


def x86_render(L, holder, seed, n_samples, deep_nodes=0, sample_base=0, threads=8):
    nw, nh = holder.desc.frame.res_w, holder.desc.frame.res_h
    acc = np.zeros((nh, nw, 3), f32)
    d, e = _ptrs(holder)
    rc = L.va_render(d, e, seed, sample_base, n_samples, threads, deep_nodes, _p(acc))
    assert rc == 0, L.va_error()
    return acc


def x86_interp(L, p, v0, e1, e2, vn, uv):
    n = p.shape[0]
    a = [np.ascontiguousarray(x, f32) for x in (p, v0, e1, e2, vn, uv)]
    bary, nrm, tex = np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.zeros((n, 2), f32)
    L.va_interp(n, *[_p(x) for x in a], _p(bary), _p(nrm), _p(tex))
    return bary, nrm, tex


# ---- DESIGN.md §14 in float32 numpy, in its operation order ------------------------------------------------------------------------
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def np_bary(p, v0, e1, e2):
    with np.errstate(all="ignore"):
        q = p - v0
        d00, d01, d11, d20, d21 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(q, e1), _dot(q, e2)
        den = d00 * d11 - d01 * d01
        b1 = (d11 * d20 - d01 * d21) / den
        b2 = (d00 * d21 - d01 * d20) / den
    ok = (den != 0) & np.isfinite(den) & np.isfinite(b1) & np.isfinite(b2)
    return b1, b2, ok


def np_mix(b1, b2, a0, a1, a2):
    with np.errstate(all="ignore"):
        return a0 + (b1 * (a1 - a0) + b2 * (a2 - a0))


def np_normal(p, v0, e1, e2, vn):
    b1, b2, ok = np_bary(p, v0, e1, e2)
    n = np.stack([np_mix(b1, b2, vn[:, k], vn[:, 3 + k], vn[:, 6 + k]) for k in range(3)], 1)
    good = ok & np.all(np.isfinite(n), 1) & ~np.all(n == 0, 1)
    with np.errstate(all="ignore"):
        return np.where(good[:, None], n, _cross(e1, e2)).astype(f32), good


def np_uv(p, v0, e1, e2, uv):
    b1, b2, ok = np_bary(p, v0, e1, e2)
    out = []
    with np.errstate(all="ignore"):
        for k in range(2):
            x = np.where(ok, np_mix(b1, b2, uv[:, k], uv[:, 2 + k], uv[:, 4 + k]), uv[:, k]).astype(f32)
            x = x - np.trunc(x)
            out.append(np.where(x < 0, f32(1.0) + x, x).astype(f32))
    return np.stack(out, 1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---- float64 references ------------------------------------------------------------------------------------------------------
def camera_rays(render):
    """Origin and unit direction of the lens-centre ray of every pixel (default camera direction), float64."""
    fr = render.frame
    cam = fr.cam
    w, h = float(f32(f32(fr.res[0]) * f32(fr.ssaa))), float(f32(f32(fr.res[1]) * f32(fr.ssaa)))
    nw, nh = int(w), int(h)
    inv2tan = 1.0 / (2.0 * np.tan(np.radians(float(cam.fov) / 2.0)))
    yy, xx = np.mgrid[0:nh, 0:nw].astype(np.float64)
    d = np.stack([(w / h) * (xx - 0.5 * w) / w, np.full_like(xx, inv2tan), -(yy - 0.5 * h) / h], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.asarray(cam.pos, np.float64) + d * 1e-4
    return o.reshape(-1, 3), d.reshape(-1, 3)


def _candidates(oo, dd, tris):
    """The reference's candidate rule for mesh triangles (src/rt.rs:740-770), restated in float64: the
    mesh's octree is the regular 8x8x8 grid over [-M, M] per axis (M = the largest |coordinate|, src/rt.rs:630-703), a leaf
    lists the triangles with a VERTEX inside it (bounds inclusive), and a ray tests the triangles of the leaves whose box it
    passes.  So a triangle is tested when the ray passes the cell of one of its vertices -- a ray through the middle of a
    triangle that straddles cells can miss it.  oo, dd: [rays][1][3] in mesh coordinates; returns [rays][tris] bool."""
    m = np.abs(tris).reshape(-1, 3).max(0)
    cell = 2.0 * m / 8.0
    cand = np.zeros((oo.shape[0], tris.shape[0]), bool)
    with np.errstate(all="ignore"):
        inv = 1.0 / dd
        for k in range(3):
            g = (tris[:, k] + m) / cell
            lo = -m + np.clip(np.ceil(g) - 1, 0, 7) * cell                # a vertex on a cell boundary lies in both cells:
            hi = -m + (np.clip(np.floor(g), 0, 7) + 1) * cell             # the union of the two is a box again
            t1, t2 = (lo[None] - oo) * inv, (hi[None] - oo) * inv
            tn, tf = np.max(np.minimum(t1, t2), -1), np.min(np.maximum(t1, t2), -1)
            cand |= (tn <= tf) & (tf >= 0)
    return cand


def _moeller(o, d, tris, pos, s, chunk):
    tl = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    v0, e1, e2 = tl[:, 0], tl[:, 1] - tl[:, 0], tl[:, 2] - tl[:, 0]
    oo, dd = (o[s:s + chunk] - np.asarray(pos, np.float64))[:, None, :], d[s:s + chunk, None, :]
    pv = np.cross(dd, e2[None])
    det = np.sum(e1[None] * pv, -1)
    with np.errstate(all="ignore"):
        inv = 1.0 / det
        tv = oo - v0[None]
        u = np.sum(tv * pv, -1) * inv
        qv = np.cross(tv, e1[None])
        v = np.sum(dd * qv, -1) * inv
        t = np.sum(e2[None] * qv, -1) * inv
    # the barycentric weights as distances from the triangle's edges: weight x the triangle's smallest altitude
    area2 = np.linalg.norm(np.cross(e1, e2), axis=1)
    alt = area2 / np.maximum(np.maximum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)), np.linalg.norm(e2 - e1, axis=1))
    return u, v, t, (np.abs(det) > 1e-12) & _candidates(oo, dd, tl), alt[None]


def brute_hits(o, d, tris, pos, t_min=0.0, chunk=1024):
    """Moeller-Trumbore of every ray against every triangle of a mesh at pos that the reference's candidate rule lets it test
    (_candidates), float64: per ray the closest hit's distance (inf: none), triangle, its barycentric weights (b1, b2) and
    `edge` = how far the ray is from changing its answer at a triangle edge, in barycentric units: the smallest of
    (b0, b1, b2) of the hit, or for a miss the amount by which the nearest triangle in front is missed."""
    n = o.shape[0]
    best_t, best_i = np.full(n, np.inf), np.full(n, -1, np.int64)
    best_u, best_v, miss_by = np.zeros(n), np.zeros(n), np.zeros(n)
    for s in range(0, n, chunk):
        u, v, t, can, _ = _moeller(o, d, tris, pos, s, chunk)
        with np.errstate(all="ignore"):
            inside = np.minimum(np.minimum(u, v), 1.0 - u - v)
            hit = can & (inside >= 0) & (t > t_min)
        tt = np.where(hit, t, np.inf)
        k = np.argmin(tt, 1)
        r = np.arange(tt.shape[0])
        best_t[s:s + chunk], best_i[s:s + chunk] = tt[r, k], np.where(np.isfinite(tt[r, k]), k, -1)
        best_u[s:s + chunk], best_v[s:s + chunk] = u[r, k], v[r, k]
        miss_by[s:s + chunk] = -np.max(np.where(can & (t > t_min), inside, -np.inf), 1)
    edge = np.where(np.isfinite(best_t), np.minimum(np.minimum(best_u, best_v), 1.0 - best_u - best_v), miss_by)
    return best_t, best_i, best_u, best_v, edge


def any_hit_margin(o, d, tris, pos, chunk=1024):
    """Shadow rays, float64: (blocked, margin).  blocked = some triangle (that the candidate rule lets the ray test) is hit at
    t > 0; margin = how far the verdict is from flipping, as a share of the triangle (barycentric units): for a blocked ray
    the largest min(b0, b1, b2) over the triangles hit, for a clear ray the smallest amount by which a triangle in front of
    the origin is missed (+inf: none in front)."""
    n = o.shape[0]
    blocked, margin = np.zeros(n, bool), np.zeros(n)
    for s in range(0, n, chunk):
        u, v, t, can, alt = _moeller(o, d, tris, pos, s, chunk)
        with np.errstate(all="ignore"):
            inside = np.minimum(np.minimum(u, v), 1.0 - u - v)          # >= 0: the ray's line meets the triangle
        # (the triangle the ray leaves lies at t = -1e-4 cos, behind the origin; a triangle within 1e-5 of the origin is marginal)
        best = np.max(np.where(can & (t > 0), inside, -np.inf), 1)
        grazing = np.any(can & (np.abs(t) < 1e-5) & (inside > -1e-3), 1)
        blocked[s:s + chunk] = best >= 0
        margin[s:s + chunk] = np.where(grazing, 0.0, np.abs(best))
    return blocked, margin


def interp64(u, v, a):
    """a[..., 3, k] corner values -> the value at barycentric (u, v), float64."""
    a = np.asarray(a, np.float64)
    return a[:, 0] + u[:, None] * (a[:, 1] - a[:, 0]) + v[:, None] * (a[:, 2] - a[:, 0])


def texel_of(uv, tex, tol=1e-3):
    """(texel rgb float64, near) of wrapped uv on a Texture: nearest texel as tex_fetch; near = within tol texel of a boundary."""
    w, h = tex.w, tex.h
    x = uv - np.floor(uv)
    fx, fy = x[:, 0] * w, x[:, 1] * h
    near = (np.abs(fx - np.round(fx)) < tol) | (np.abs(fy - np.round(fy)) < tol)
    ix, iy = np.minimum(fx.astype(np.int64), w - 1), np.minimum(fy.astype(np.int64), h - 1)
    return np.asarray(tex.dat, np.float64).reshape(h, w, 3)[iy, ix], near


def ring(mask):
    """Pixels of a boolean image that touch (3x3) a pixel of the other value."""
    m = np.pad(mask, 1, mode="edge")
    out = np.zeros_like(mask)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out |= m[dy:dy + mask.shape[0], dx:dx + mask.shape[1]] != mask
    return out


def closed_form(render, r_index=0):
    """Mean radiance of a bounce-0, aprt-0 render of ONE smooth textured mesh (renderer r_index, one untransformed instance,
    rough 1, emit 0, opaque) under ONE point light and a black sky, float64, from the fold of src/rt.rs:964-993:
    a miss is the raw sky colour; a hit is ((albedo x texel)(1 - metal) max(l.n, 0)) x light colour x light power when the
    shadow ray from hit + 1e-4 l reaches no triangle, else 0 (rough 1: no highlight; bounce 0: the fold starts from
    sky x pwr = 0 and the path's power is 1).  Returns (image [nh][nw][3], hit mask, excluded mask by reason)."""
    rd = render.scene.renderer[r_index]
    light = render.scene.light[0]
    assert render.rt.bounce == 0 and render.frame.cam.aprt == 0 and len(render.scene.light) == 1 and light.kind == "point"
    nw, nh = render.frame.res
    pos = np.asarray(rd.inst[0][0], np.float64)
    o, d = camera_rays(render)
    t, tri, u, v, edge = brute_hits(o, d, rd.mesh, pos)
    hit = np.isfinite(t)
    img = np.zeros((nh * nw, 3))
    img[~hit] = np.asarray(render.scene.sky.color, np.float64)
    k = np.flatnonzero(hit)
    hp = o[k] + d[k] * t[k, None]
    n = interp64(u[k], v[k], np.asarray(rd.vn, np.float64)[tri[k]])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    uv = interp64(u[k], v[k], np.asarray(rd.uv, np.float64)[tri[k]])
    texel, near_texel = texel_of(uv, rd.mat.tex)
    color = np.asarray(rd.mat.albedo, np.float64) * texel
    l = np.asarray(light.v, np.float64) - hp
    l /= np.linalg.norm(l, axis=1, keepdims=True)
    ln = np.sum(l * n, 1)
    blocked, margin = any_hit_margin(hp + l * 1e-4, l, rd.mesh, pos)
    term = color * (1.0 - rd.mat.metal) * np.maximum(ln, 0.0)[:, None] * np.asarray(light.color, np.float64) * light.pwr
    img[k] = np.where((blocked | (ln <= 0))[:, None], 0.0, term)
    hit2 = hit.reshape(nh, nw)
    # (aprt 0: every sample of a pixel is the same ray, so only a ray that grazes a triangle edge can change its answer)
    excl = {"silhouette": (edge < 1e-4).reshape(nh, nw), "texel": np.zeros(nh * nw, bool), "terminator": np.zeros(nh * nw, bool)}
    excl["texel"][k] = near_texel
    excl["terminator"][k] = (np.abs(ln) < 1e-3) | ((ln > 0) & (margin < 1e-3))
    excl = {key: val.reshape(nh, nw) for key, val in excl.items()}
    return img.reshape(nh, nw, 3), hit2, excl
