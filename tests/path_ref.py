"""TEST INFRASTRUCTURE for tests/test_path_ref_host.py and tests/test_gpu_path_ref.py: the stochastic path of the reference --
the RNG contract of DESIGN.md §5, RayTracer::rand, Ray::reflect / Ray::refract with Vec3f::refract, the iterator's transmission
rule, the thin lens, the emit coin of the fold and the fold over several random bounces -- restated in plain numpy from the text
of src/rt.rs and src/lin.rs (every function cites its lines), of DESIGN.md §5 and of include/mrt.h.  It imports numpy and
core_ref alone: the deterministic pieces (closest hit, normals, UVs, texels, the six getters, light directions) are core_ref's.
Nothing here comes from the oracle, the x86 build of the kernel headers or the C sources.

As in core_ref every function takes a dtype: float64 is the reference the tests hold the code to, float32 the witness of what
plain float32 arithmetic carries on the same formulas.  The integers of the RNG are exact whatever the dtype, and so is every
coin: its probability is a float32 quantity of the reference and is computed in float32 whatever the dtype, its threshold an
integer, its outcome an integer comparison.  A coin needs no margin."""
import numpy as np

import core_ref as R

GOLD = np.uint32(0x9E3779B9)
DIM_LENS_X, DIM_LENS_Z, DIM_BOUNCE0, DIMS_PER_BOUNCE = 0, 1, 2, 8
# per bounce b the dimensions 2 + 8 b + {refl coin, u1, u2, opacity coin, refr coin, u1, u2, emit coin}
REFL_COIN, REFL_U1, REFL_U2, OPAC_COIN, REFR_COIN, REFR_U1, REFR_U2, EMIT_COIN = range(8)
DEGENERATE = 1e-3                        # |n + r v| below this: rand's normalisation divides by (almost) nothing
PI32 = np.float32(np.pi)                 # std::f32::consts::PI, src/rt.rs:998 -- the float32 number, whatever the dtype
F32, F64 = np.float32, np.float64


# ---- DESIGN.md §5 --------------------------------------------------------------------------------------------------------------------
def _u32(x):
    return np.asarray(x).astype(np.uint64).astype(np.uint32) if np.asarray(x).dtype.kind in "iu" else np.asarray(x, np.uint32)


def mix32(x):
    """lowbias32 (`mix32` = lowbias32): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16,
    all modulo 2^32."""
    x = _u32(x).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


def path_key(seed_lo, seed_hi, pixel, sample):
    """path_key = mix32((mix32(pixel + seed_lo) ^ seed_hi) + sample * 0x9E3779B9), every sum and product modulo 2^32."""
    with np.errstate(over="ignore"):
        a = mix32(_u32(pixel) + np.uint32(seed_lo)) ^ np.uint32(seed_hi)
        return mix32(a + _u32(sample) * GOLD)


def draw_u32(pk, dim):
    """draw(dim) = mix32(path_key + (dim + 1) * 0x9E3779B9)."""
    with np.errstate(over="ignore"):
        return mix32(_u32(pk) + (_u32(dim) + np.uint32(1)) * GOLD)


def uniform(u, dtype=F64):
    """(u >> 9) * 2^-23: the lattice of rand's Uniform<f32>; 23 bits, exact in float32 and float64."""
    return (_u32(u) >> np.uint32(9)).astype(dtype) * dtype(2.0 ** -23)


def threshold(p):
    """(u32)(p * 2^32) of a probability given as float64 (gen_bool takes an f64: `.into()`, src/rt.rs:968, 1054)."""
    p = np.asarray(p, F64)
    return np.minimum(np.floor(p * 4294967296.0), 4294967295.0).astype(np.uint64)


def bernoulli(p, u):
    """Bernoulli(p): p == 1 -> true, else u < (u32)(p * 2^32)."""
    p = np.asarray(p, F64)
    return (p == 1.0) | (_u32(u).astype(np.uint64) < threshold(p))


P_DIFFUSE = 0.80                         # gen_bool(0.80), src/rt.rs:564, 579: an f64 literal


def p_transmit(opacity):
    """(1.0 - opacity).min(0.85).into(), src/rt.rs:1054: float32 arithmetic, then widened."""
    return np.minimum(F32(1.0) - np.asarray(opacity).astype(F32), F32(0.85)).astype(F64)


def p_emit(emit):
    """emit.into(), src/rt.rs:966-968."""
    return np.asarray(emit).astype(F32).astype(F64)


# ---- src/rt.rs:996-1007, src/lin.rs:96-105 ----------------------------------------------------------------------------------------------
def rand_dir(n, r, u1, u2):
    """RayTracer::rand, src/rt.rs:996-1007, read literally (not contract v3 of DESIGN.md §4, whose committed bound of 3e-7 lies far
    inside the bar): th = acos(1 - 2 u1), phi = u2 * 2 * PI, v = (sin th cos phi, sin th sin phi, cos th), (n + r v).norm().
    Returns (direction, |n + r v|)."""
    T = n.dtype.type
    th = np.arccos(T(1.0) - T(2.0) * u1)
    phi = u2 * T(2.0) * T(PI32)
    v = np.stack([np.sin(th) * np.cos(phi), np.sin(th) * np.sin(phi), np.cos(th)], -1)
    w = n + r[..., None] * v
    return R.norm(w), np.sqrt(np.sum(np.asarray(w, F64) ** 2, -1))


def vec_refract(d, eta, n):
    """Vec3f::refract, src/lin.rs:96-105: cos = -n . d; k = 1 - eta^2 (1 - cos^2); k < 0 -> None; d eta + n (cos eta + sqrt k).
    Returns (vector, taken, |k| / eta^2: how far the k < 0 test is from flipping)."""
    T = d.dtype.type
    cos = R.dot(-n, d)
    k = T(1.0) - (eta * eta) * (T(1.0) - cos * cos)
    with np.errstate(invalid="ignore"):
        out = d * eta[..., None] + n * (cos * eta + np.sqrt(k))[..., None]
    return out, ~(k < 0), np.abs(np.asarray(k, F64)) / np.asarray(eta, F64) ** 2


# ---- src/rt.rs:900-954 ------------------------------------------------------------------------------------------------------------------
def frame_shape(render):
    """(nh, nw) of the supersampled frame: `as usize` of res * ssaa in float32, src/sampler.rs:19-20."""
    fr = render.frame
    return int(F32(fr.res[1]) * F32(fr.ssaa)), int(F32(fr.res[0]) * F32(fr.ssaa))


def lens_rays(render, pixel, u_x, u_z, dtype=F64):
    """RayTracer::iter and ::cast, src/rt.rs:900-954, for any aprt: the pinhole direction dir of pixel (x, y) = (pixel % nw,
    pixel / nw); the focus point p = (cam.pos + dir E) + dir foc (cast_default, then From<&Ray> at t = foc); the lens point pos =
    cam.pos + ((u_x - 0.5) aprt, 0, (u_z - 0.5) aprt), two draws, x first; new_dir = (p - pos).norm(); the ray LEAVES THE LENS
    POINT: cast_default(pos, rot_y (look new_dir)) = (pos + D E, D).  The offset is applied in camera space, before the rotation
    (src/rt.rs:916-920 precede 925-930), to the position alone."""
    T = dtype
    fr, cam = render.frame, render.frame.cam
    w32, h32 = F32(fr.res[0]) * F32(fr.ssaa), F32(fr.res[1]) * F32(fr.ssaa)
    nw = int(w32)
    w, h = T(w32), T(h32)
    pixel = np.asarray(pixel, np.int64)
    xx, yy = (pixel % nw).astype(T), (pixel // nw).astype(T)
    aspect = w / h
    tan_fov = np.tan(np.radians(T(0.5) * T(cam.fov))).astype(T)
    ux, uy = aspect * (xx - T(0.5) * w) / w, (yy - T(0.5) * h) / h
    d = R.norm(np.stack([ux, np.full_like(ux, T(1.0) / (T(2.0) * tan_fov)), -uy], -1))
    cp = R._a(cam.pos, T)
    p = (cp + d * T(R.E32)) + d * T(cam.foc)
    aprt = T(cam.aprt)
    zero = np.zeros_like(ux)
    pos = cp + np.stack([(np.asarray(u_x, T) - T(0.5)) * aprt, zero, (np.asarray(u_z, T) - T(0.5)) * aprt], -1)
    nd = R.norm(p - pos)
    D = R._mul(R.rotate_y(cam.dir, T), R._mul(R.lookat(cam.dir, T), nd))
    return pos + D * T(R.E32), D


def camera_paths(render, seed, pixel, sample, dtype=F64):
    """The primary rays of (pixel, sample): lens_rays with the draws of dimensions 0 and 1 (0, 1 = lens x, z)."""
    pk = path_key(seed & 0xFFFFFFFF, seed >> 32, pixel, sample)
    return lens_rays(render, pixel, uniform(draw_u32(pk, DIM_LENS_X), dtype), uniform(draw_u32(pk, DIM_LENS_Z), dtype), dtype)


# ---- src/rt.rs:1014-1065, 956-994 -------------------------------------------------------------------------------------------------------
MARGINS = ("decide", "gap", "texel", "box", "window", "shadow", "tir", "degenerate", "reach")
REACH = 16.0                             # core_ref.tame: |o - instance pos| <= 16; here for the hit point too (planes are infinite)


def _pick(m, a, b):
    return np.where(m[:, None] if a.ndim == 2 else m, a, b)


def trace_sample(render, seed, pixel, sample, o, d, dtype=F64):
    """One reduce_light(iter(...)) per (pixel, sample), vectorised over them, from the primary rays (o, d) as cast (the origin
    already shifted by E): RaytraceIterator::next, src/rt.rs:1014-1065, while bounce <= rt.bounce, then RayTracer::reduce_light,
    src/rt.rs:956-994, back to front with the emit coin per item.  D3: the fold is evaluated once.

    Per segment b (the ray's `bounce`), in the order of `next`:
      closest_hit -> (hit.0, hit.1), the entry and the exit hit of ONE instance; no hit ends the path;
      the light list: a shadow ray cast_default(hit.0's point, l) per light, kept when it meets nothing (1027-1046);
      next_ray = hit.0.ray.reflect(hit.0) (1049; Ray::reflect, 559-572): rough and opacity of hit.0; rough = 1 when the
        MATERIAL's metal (not the map) is 0, opacity != 0 and the 80 % coin fires -- the coin is drawn only then; n' = rand(hit.0's
        normal, rough); dir.reflect(n').norm() from hit.0's point, pwr (1 - loss.min(1)), bounce + 1;
      the transmission coin (1 - opacity of hit.0).min(0.85) (1051-1054); when it fires, hit.1.ray.refract(hit.1) (574-589):
        rough, opacity, glass of hit.1 (read at the EXIT hit's UV), the same 80 % rule with a coin of its own, n' = rand(hit.1's
        normal, rough), eta = 1 + 0.5 glass, dir.refract(eta, n') -- None when k < 0: the reflection stays -- normalised, from
        hit.1's point; on success next_ray is that and n_hit = hit.1 (1055-1058);
      the item (n_hit, lights): the fold shades with n_hit's point, normal, UV and maps and hit.0's light list.
    The fold (964-993) starts from sky.color * sky.pwr (no item at all: sky.color, 957-959); per item, last first: the emit coin
    on n_hit's emit -> the item's colour replaces everything; else ((o_col diff) (x) light.color + spec) * light.pwr over the
    list, l taken from n_hit's point, then (0.5 col + colour (x) col + l_col) * ray.pwr.

    Draws are addressed by slot: segment b draws dimension 2 + 8 b + slot, so neither the order of the draws inside
    `next` nor the fold's reversed order changes which number an item's emit coin gets.  A path is not followed behind an item
    whose emit coin fires: the fold replaces whatever lies behind it, and its decisions must not count against the sample.

    Returns a dict: rgb [n][3]; depth (items); branches: per segment a dict of bool arrays (hit, diffuse_drawn, diffuse, transmit,
    refracted, failed, refr_diffuse_drawn, refr_diffuse, emit_fired, emit_p, p_transmit, lit [lights], rough); margins: core_ref's
    (decide, gap, texel, box, window, shadow) plus tir = |k| / eta^2, degenerate = |n + r v| and reach = 16 / the largest distance
    of a segment's origin or hit points from the instance it hit (core_ref.tame's bound), each the minimum over the path."""
    T = dtype
    o, d = R._a(o, T), R._a(d, T)
    n = o.shape[0]
    fr = R.frames(render, T)
    pk = path_key(seed & 0xFFFFFFFF, seed >> 32, pixel, sample)
    sky = render.scene.sky
    alive = np.ones(n, bool)
    pwr = np.ones(n, T)
    keep = T(1.0) - min(T(render.rt.loss), T(1.0))
    marg = {k: np.full(n, np.inf) for k in MARGINS}
    items, branches = [], []

    def low(key, mask, val):
        marg[key] = np.where(mask, np.minimum(marg[key], val), marg[key])

    def dim(b, slot):
        return DIM_BOUNCE0 + DIMS_PER_BOUNCE * b + slot

    def scatter(b, coin, s1, s2, nrm, mat):
        """The part Ray::reflect and Ray::refract share (559-568, 574-583): (n', rough used, coin drawn, coin fired, |n + r v|)."""
        drawn = (mat["mat_metal"] == 0) & (mat["opacity"].astype(F32) != 0)
        fired = drawn & bernoulli(P_DIFFUSE, draw_u32(pk, dim(b, coin)))
        rough = np.where(fired, T(1.0), mat["rough"])
        with np.errstate(all="ignore"):
            nn, mag = rand_dir(nrm, rough, uniform(draw_u32(pk, dim(b, s1)), T), uniform(draw_u32(pk, dim(b, s2)), T))
        return nn, drawn, fired, mag

    for b in range(render.rt.bounce + 1):
        h = R.closest_hit(render, o, d, T, fr)
        h["hit"] = h["hit"] & alive
        hit = h["hit"]
        low("decide", alive, h["decide"]); low("gap", alive, h["gap"])
        p0, n0, uv0, face0, mb0 = R.surface(render, h, o, d, "t0", T, fr)
        p1, n1, uv1, face1, mb1 = R.surface(render, h, o, d, "t1", T, fr)
        m0, near0 = R.material(render, h, uv0, T)
        m1, near1 = R.material(render, h, uv1, T)
        last = b == render.rt.bounce                       # the next ray is cast and never traced (1018)
        # the light list, from hit.0
        ls0 = R.light_dirs(render, p0, T)
        seen, verdict = [], np.full(n, np.inf)
        for l in ls0:
            sh = R.closest_hit(render, p0 + l * T(R.E32), l, T, fr)
            seen.append(hit & ~sh["hit"])
            verdict = np.minimum(verdict, sh["any_decide"])
        # reflect
        nr, drawn0, fired0, mag0 = scatter(b, REFL_COIN, REFL_U1, REFL_U2, n0, m0)
        with np.errstate(all="ignore"):
            dr = R.norm(R.reflect(d, nr))
        # the transmission coin and refract
        pt = p_transmit(m0["opacity"])
        transmit = hit & bernoulli(pt, draw_u32(pk, dim(b, OPAC_COIN)))
        nt, drawn1, fired1, mag1 = scatter(b, REFR_COIN, REFR_U1, REFR_U2, n1, m1)
        eta = T(1.0) + T(0.5) * m1["glass"]
        with np.errstate(all="ignore"):
            dt, ok, tir = vec_refract(d, eta, nt)
            dt = R.norm(dt)
        refracted = transmit & ok
        # n_hit
        pn, nn_ = _pick(refracted, p1, p0), _pick(refracted, n1, n0)
        mat = {k: _pick(refracted, m1[k], m0[k]) for k in m0}
        e_p = p_emit(mat["emit"])
        emit_fired = hit & bernoulli(e_p, draw_u32(pk, dim(b, EMIT_COIN)))
        items.append((hit.copy(), d.copy(), pn, nn_, mat, seen, pwr.copy(), emit_fired))
        branches.append({"hit": hit.copy(), "diffuse_drawn": hit & drawn0 & ~last & ~emit_fired & ~refracted, "diffuse": hit & fired0 & ~last & ~emit_fired & ~refracted,
                         "transmit": transmit, "refracted": refracted, "failed": transmit & ~ok,
                         "refr_diffuse_drawn": transmit & drawn1, "refr_diffuse": transmit & fired1, "emit_fired": emit_fired, "emit_p": np.where(hit, e_p, 0.0),
                         "p_transmit": np.where(hit, pt, 0.0), "lit": [s & ~emit_fired for s in seen], "shadowed": [hit & ~s & ~emit_fired for s in seen],
                         "rough": np.where(hit, np.asarray(m0["rough"], F64), 0.0), "metal_skip": hit & (m0["mat_metal"] != 0) & ~last & ~emit_fired & ~refracted,
                         "opaque0": hit & (m0["opacity"].astype(F32) == 0), "mapped": hit & _mapped(render, h)})
        # margins of this segment's decisions
        low("reach", hit, REACH / np.maximum(_dist(render, h, o), np.maximum(_dist(render, h, p0), _dist(render, h, p1))))
        low("texel", hit, near0); low("box", hit, mb0["box"]); low("window", hit, mb0["window"])
        low("texel", transmit, near1); low("box", transmit, mb1["box"]); low("window", transmit, mb1["window"])
        low("shadow", hit & ~emit_fired, verdict)
        low("tir", transmit, tir)
        low("degenerate", transmit, mag1)
        low("degenerate", hit & ~refracted & ~last & ~emit_fired, mag0)
        # A ray that leaves a box or a sphere starts E |c| off it (c: the cosine between its direction and the surface IN THE
        # INSTANCE'S FRAME -- the world normal of a rotated instance is not the surface's, src/rt.rs:792).  Box::intersect decides
        # `t1 < 0` on that face's slab, Sphere::intersect `t0 < 0` from c = |q|^2 - r^2 ~ 2 r E c, each against the float32 error of the
        # hit point, ~SIGN S: core_ref's margins look at |t| = E there, which does not shrink with |c|.  The next ray and the shadow
        # rays of such a hit need |c| >= SIGN S / E.  (Plane::intersect's numerator margin already says this for planes.)
        nd = _pick(refracted, dt, dr)
        face_n = np.where(refracted, face1, face0)
        low("decide", hit & ~last & ~emit_fired, _leave(render, h, fr, o, pn, nd, face_n))
        for l in ls0:
            low("shadow", hit & ~emit_fired, _leave(render, h, fr, o, p0, l, face0))
        # the next ray: Ray::cast(point, dir, pwr (1 - loss.min(1)), bounce + 1), src/rt.rs:551-553, 571, 588
        alive = hit & ~emit_fired
        o = np.where(alive[:, None], pn + nd * T(R.E32), o)
        d = np.where(alive[:, None], nd, d)
        pwr = pwr * keep
    # reduce_light
    col = np.broadcast_to(R._a(sky.color, T) * T(sky.pwr), (n, 3)).copy()
    for hit, rd_, pn, nrm, mat, seen, pw, emit_fired in reversed(items):
        ls = R.light_dirs(render, pn, T)
        l_col = np.zeros((n, 3), T)
        for lt, l, s in zip(render.scene.light, ls, seen):
            with np.errstate(all="ignore"):
                diff = np.maximum(R.dot(l, nrm), T(0.0))
                spec = np.maximum(R.dot(rd_, R.reflect(l, nrm)), T(0.0))
                for _ in range(5):                                       # powi(32)
                    spec = spec * spec
                spec = spec * (T(1.0) - mat["rough"])
                o_col = mat["color"] * (T(1.0) - mat["metal"])[:, None]
                term = ((o_col * diff[:, None]) * R._a(lt.color, T) + spec[:, None]) * T(lt.pwr)
            l_col = l_col + np.where(s[:, None], term, T(0.0))
        with np.errstate(all="ignore"):
            new = ((T(0.5) * col + mat["color"] * col) + l_col) * pw[:, None]
        new = np.where(emit_fired[:, None], mat["color"], new)
        col = np.where(hit[:, None], new, col)
    rgb = np.where(items[0][0][:, None], col, R._a(sky.color, T))
    return {"rgb": rgb, "depth": np.sum([it[0] for it in items], 0), "branches": branches, "margins": marg}


def _leave(render, h, fr, o, p, vec, face):
    """|c| / (SIGN S / E) for rays along vec from the points p of the box and sphere hits of h (S of core_ref.box / .sphere; c: the
    direction's component on the face's axis, or its cosine with the radius, in the instance's frame); inf for other kinds."""
    out = np.full(h["hit"].shape, np.inf)
    lo = np.sqrt(np.sum(np.asarray(o, F64) ** 2, -1))
    for ri, rd in enumerate(render.scene.renderer):
        if rd.kind not in ("box", "sphere"):
            continue
        for ii, (pos, _) in enumerate(rd.inst):
            k = np.flatnonzero(h["hit"] & (h["rend"] == ri) & (h["inst"] == ii) & ((face >= 0) | (rd.kind == "sphere")))
            if k.size == 0:
                continue
            f = fr[ri][ii]
            with np.errstate(all="ignore"):
                dv = np.asarray(f.vec(vec[k]), F64)
                if rd.kind == "box":
                    S = lo[k] + np.linalg.norm(np.asarray(pos, F64)) + np.linalg.norm(np.asarray(rd.sizes, F64))
                    c = np.abs(dv[np.arange(k.size), face[k] // 2])
                else:
                    S = lo[k] + np.linalg.norm(np.asarray(pos, F64)) + float(rd.r)
                    c = np.abs(R.dot(dv, R.norm(np.asarray(f.point(p[k]) - f.pos, F64))))
            out[k] = np.where(np.isfinite(c), c, 0.0) / (S * (R.SIGN / R.E32))
    return out


def _dist(render, h, p):
    """|p - instance pos| of the instance each ray hit (1e-30 where none)."""
    pos = np.zeros(p.shape, F64)
    for ri, rd in enumerate(render.scene.renderer):
        for ii, (q, _) in enumerate(rd.inst):
            pos[h["hit"] & (h["rend"] == ri) & (h["inst"] == ii)] = np.asarray(q, F64)
    return np.where(h["hit"], np.sqrt(np.sum((np.asarray(p, F64) - pos) ** 2, -1)), 0.0) + 1e-30


def _mapped(render, h):
    """Hits on a renderer with any of the scalar maps (rmap, gmap, omap, emap)."""
    has = np.array([any(t is not None for t in (rd.mat.rmap, rd.mat.gmap, rd.mat.omap, rd.mat.emap)) for rd in render.scene.renderer] + [False])
    return has[h["rend"]]


def sound(marg):
    """The samples whose every discrete decision float32 arithmetic cannot flip: core_ref's thresholds (tame's 16 units included),
    tir >= REL, degenerate >= DEGENERATE."""
    return (marg["decide"] >= 1) & (marg["gap"] >= R.REL) & (marg["shadow"] >= 1) & (marg["texel"] >= R.TEXEL) & (marg["box"] >= R.BOX_P) & \
        (marg["window"] >= 0.5) & (marg["tir"] >= R.REL) & (marg["degenerate"] >= DEGENERATE) & (marg["reach"] >= 1)
