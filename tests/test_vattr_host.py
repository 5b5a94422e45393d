"""Per-corner normals and UVs of triangles and meshes without a GPU: the interpolation compiled for x86
(tests/emu/vattr_probe.cpp) against a float32 numpy restatement, bit for bit; the x86 AOV pass and path tracer on scenes with
attributes against float64 references that share no code with the kernels (tests/vattr_ref.py); the launch plan and packed
layout of scenes without attributes; the .obj / JSON loader."""
import ctypes as C
import json
import math

import numpy as np
import pytest

import vattr_ref as V
from conftest import make_holder
from micro_raytracer_amd._abi import F_ALL, F_VATTR

f32 = np.float32


@pytest.fixture(scope="module")
def probe():
    return V.shared_probe()


# ---- 1. interpolation: x86 build of mrt_trace.h against numpy float32 ----------------------------------------------------------------
def _random_cases(rng, n):
    v0 = rng.uniform(-2, 2, (n, 3)).astype(f32)
    e1 = (rng.uniform(-1, 1, (n, 3)) * 10.0 ** rng.uniform(-3, 1, (n, 1))).astype(f32)
    e2 = (rng.uniform(-1, 1, (n, 3)) * 10.0 ** rng.uniform(-3, 1, (n, 1))).astype(f32)
    # points inside, on the edges, at the corners and outside (also off the triangle's plane)
    kind = rng.integers(0, 5, n)
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    fold = a + b > 1
    a, b = np.where(fold, 1 - a, a), np.where(fold, 1 - b, b)
    a = np.where(kind == 1, 0.0, a)                                               # edge b1 = 0
    b = np.where(kind == 2, 1.0 - a, b)                                           # edge b1 + b2 = 1
    corner = rng.integers(0, 3, n)
    a = np.where(kind == 3, (corner == 1).astype(float), a)
    b = np.where(kind == 3, (corner == 2).astype(float), b)
    a = np.where(kind == 4, rng.uniform(-3, 3, n), a)
    b = np.where(kind == 4, rng.uniform(-3, 3, n), b)
    p = (v0 + f32(1) * (a[:, None].astype(f32) * e1) + b[:, None].astype(f32) * e2).astype(f32)
    p = np.where((kind == 4)[:, None], p + rng.normal(0, 0.1, (n, 3)).astype(f32), p).astype(f32)
    vn = rng.normal(0, 1, (n, 9)).astype(f32)
    uv = rng.uniform(-3, 3, (n, 6)).astype(f32)
    return p, v0, e1, e2, vn, uv


def test_interpolation_equals_numpy_bit_for_bit(probe):
    rng = np.random.default_rng(5)
    p, v0, e1, e2, vn, uv = _random_cases(rng, 20000)
    bary, nrm, tex = V.x86_interp(probe, p, v0, e1, e2, vn, uv)
    b1, b2, ok = V.np_bary(p, v0, e1, e2)
    assert ok.mean() > 0.99
    assert np.all(V.same_bits(bary[:, 0], b1)) and np.all(V.same_bits(bary[:, 1], b2)) and np.array_equal(bary[:, 2] != 0, ok)
    n_ref, good = V.np_normal(p, v0, e1, e2, vn)
    assert good.mean() > 0.99 and np.all(V.same_bits(nrm, n_ref))
    assert np.all(V.same_bits(tex, V.np_uv(p, v0, e1, e2, uv)))
    assert np.all((tex >= 0) & (tex <= 1))                                        # wrapped like the plane's UV


def test_equal_corners_come_back_bit_for_bit(probe):
    rng = np.random.default_rng(6)
    n = 20000
    p, v0, e1, e2, _, _ = _random_cases(rng, n)
    c = (rng.normal(0, 1, (n, 3)) * 10.0 ** rng.uniform(-6, 6, (n, 1))).astype(f32)
    t = rng.uniform(-4, 4, (n, 2)).astype(f32)
    bary, nrm, tex = V.x86_interp(probe, p, v0, e1, e2, np.tile(c, 3), np.tile(t, 3))
    ok = bary[:, 2] != 0
    assert ok.mean() > 0.99
    assert np.all(V.same_bits(nrm[ok], c[ok]))
    with np.errstate(all="ignore"):
        w = t - np.trunc(t)
        w = np.where(w < 0, f32(1) + w, w).astype(f32)
    assert np.all(V.same_bits(tex[ok], w[ok]))
    # the mix alone, weights up to 1e30 (finite): x + (b1 * 0 + b2 * 0) = x for every x but -0, which comes back as a zero
    m = 4096
    b1 = (rng.normal(0, 1, m) * 10.0 ** rng.uniform(-30, 30, m)).astype(f32)
    b2 = (rng.normal(0, 1, m) * 10.0 ** rng.uniform(-30, 30, m)).astype(f32)
    x = (rng.normal(0, 1, m) * 10.0 ** rng.uniform(-38, 38, m)).astype(f32)
    x[:8] = [0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 3.4e38, -3.4e38]
    out = np.zeros(m, f32)
    probe.va_mix(m, V._p(b1), V._p(b2), V._p(x), V._p(x), V._p(x), V._p(out))
    nz = x != 0
    assert np.all(V.same_bits(out[nz], x[nz])) and np.all(out[~nz] == 0)
    assert np.all(V.same_bits(out, V.np_mix(b1, b2, x, x, x)))


def test_degenerate_triangles_and_normals_fall_back(probe):
    inf, nan = f32(np.inf), f32(np.nan)
    z3 = np.zeros(3, f32)
    cases = []      # (p, v0, e1, e2, vn, uv, face-normal fallback expected, corner-0 uv expected)
    vn = np.array([0, 0, 1, 0, 1, 0, 1, 0, 0], f32)
    uv = np.array([0.25, 0.75, 0.5, 0.5, 0.9, 0.1], f32)
    e1, e2 = np.array([1, 0, 0], f32), np.array([0, 1, 0], f32)
    pin = np.array([0.25, 0.25, 0], f32)
    cases.append((pin, z3, e1, e1 * f32(2), vn, uv, True, True))                  # zero area: e2 parallel to e1
    cases.append((pin, z3, z3, e2, vn, uv, True, True))                           # a zero edge
    cases.append((pin, z3, e1 * f32(1e25), e2 * f32(1e25), vn, uv, True, True))   # den overflows
    cases.append((pin, z3, np.array([nan, 0, 0], f32), e2, vn, uv, True, True))   # NaN edge
    cases.append((np.array([inf, 0, 0], f32), z3, e1, e2, vn, uv, True, True))    # non-finite weights
    cases.append((pin, z3, e1, e2, np.zeros(9, f32), uv, True, False))            # zero normal
    cases.append((np.array([0.5, 0.5, 0], f32), z3, e1, e2, np.array([0, 0, 0, 1, 2, 3, -1, -2, -3], f32), uv, True, False))   # cancels to zero
    cases.append((pin, z3, e1, e2, np.array([0, 0, 1, inf, 0, 0, 0, 0, 1], f32), uv, True, False))   # non-finite normal
    cases.append((pin, z3, e1, e2, np.array([0, 0, 1, nan, 0, 0, 0, 0, 1], f32), uv, True, False))
    cases.append((pin, z3, e1, e2, vn, uv, False, False))                         # the sound one
    cols = [np.stack([c[k] for c in cases]) for k in range(6)]
    bary, nrm, tex = V.x86_interp(probe, *cols)
    n_ref, _ = V.np_normal(*cols[:5])
    assert np.all(V.same_bits(nrm, n_ref)) and np.all(V.same_bits(tex, V.np_uv(*cols[:4], cols[5])))
    for i, c in enumerate(cases):
        face = V._cross(c[2][None], c[3][None])[0]
        assert np.all(V.same_bits(nrm[i], face)) == c[6], i
        if c[7]:
            assert np.all(V.same_bits(tex[i], uv[:2])), i
        assert (bary[i, 2] == 0) == c[7], i
    assert np.allclose(nrm[-1], [0.25, 0.25, 0.5]) and np.allclose(tex[-1], [0.25 + 0.25 * 0.25 + 0.25 * 0.65, 0.75 - 0.25 * 0.25 - 0.25 * 0.65])


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def _sphere_uv(d):
    """hit_uv's sphere mapping of unit directions, float64."""
    return np.stack([0.5 + 0.5 * np.arctan2(d[:, 0], -d[:, 1]) / math.pi, 0.5 - 0.5 * d[:, 2]], 1)


def _unwrap(u):
    return np.where(u - u[:, :1] > 0.5, u - 1.0, np.where(u - u[:, :1] < -0.5, u + 1.0, u))


def analytic_sphere_scene(res=(96, 64), subdiv=3, radius=0.5):
    """An icosphere of a true sphere: vn = the normalised vertex positions, uv = hit_uv's sphere mapping of the vertices."""
    from micro_raytracer_amd import scenes
    tris = scenes.icosphere(subdiv, radius, (1.0, 1.0, 1.0))
    d = tris.reshape(-1, 3).astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    uv = _sphere_uv(d).reshape(-1, 3, 2)
    uv[:, :, 0] = _unwrap(uv[:, :, 0])
    tex = scenes.checker_texture(16, 8, 1, a=(1.0, 200 / 255.0, 100 / 255.0), b=(50 / 255.0, 100 / 255.0, 250 / 255.0))
    return {
        "rt": {"sample": 1, "bounce": 0},
        "frame": {"res": list(res), "ssaa": 1, "cam": {"pos": [0.05, -0.9, 0.1], "fov": 60, "aprt": 0}},
        "scene": {"renderer": [{"type": "mesh", "mesh": tris.tolist(), "vn": d.reshape(-1, 3, 3).tolist(), "uv": uv.tolist(),
                                "pos": [0, 0.3, 0], "mat": {"albedo": [0.9, 0.8, 0.7], "rough": 1, "tex": tex}}],
                  "light": [{"type": "point", "pos": [-0.9, -1.2, 1.1], "pwr": 1.5, "color": [1.0, 0.9, 0.8]}],
                  "sky": {"color": [0, 0, 0], "pwr": 0.5}},
    }


def _fib(n):
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = math.pi * (1 + 5 ** 0.5) * i
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)


def labelled_scene(tris, res=(96, 64)):
    """Every triangle its own constant normal (a Fibonacci-sphere point) and constant UV (the centre of its own texel, whose
    colour spells the triangle's index): the normal and albedo AOVs name the triangle that was hit."""
    tris = np.asarray(tris, f32).reshape(-1, 3, 3)
    n = tris.shape[0]
    w = 32
    h = (n + w - 1) // w
    idx = np.arange(w * h)
    dat = np.stack([(idx % 256) / 255.0, (idx // 256) / 255.0, np.full(idx.shape, 128 / 255.0)], 1)
    uv = np.stack([((np.arange(n) % w) + 0.5) / w, ((np.arange(n) // w) + 0.5) / h], 1)
    return {
        "rt": {"sample": 1, "bounce": 0},
        "frame": {"res": list(res), "ssaa": 1, "cam": {"pos": [0.013, -1.2, 0.15], "fov": 60, "aprt": 0}},
        "scene": {"renderer": [
            {"type": "plane", "n": [0, 0, 1], "pos": [0, 0, -0.5], "mat": {"rough": 1}},
            {"type": "mesh", "mesh": tris.tolist(), "vn": np.repeat(_fib(n)[:, None], 3, 1).tolist(),
             "uv": np.repeat(uv[:, None], 3, 1).tolist(), "pos": [0, 0.5, 0],
             "mat": {"rough": 1, "tex": {"w": w, "h": h, "dat": dat.tolist()}}}]},
    }


# ---- 2. first hit ----------------------------------------------------------------------------------------------------------------------
def check_analytic_aov(g, alb, rend, render):
    rd = render.scene.renderer[0]
    nw, nh = render.frame.res
    pos = np.asarray(rd.inst[0][0], np.float64)
    o, d = V.camera_rays(render)
    t, tri, u, v, edge = V.brute_hits(o, d, rd.mesh, pos)
    hit = np.isfinite(t).reshape(nh, nw)
    assert np.array_equal(rend >= 0, hit) or np.all(((rend >= 0) != hit) <= V.ring(hit))
    ok = (hit & ~V.ring(hit) & (rend >= 0)).reshape(-1)
    assert ok.sum() > 0.15 * ok.size
    k = np.flatnonzero(ok)
    n64 = V.interp64(u[k], v[k], np.asarray(rd.vn, np.float64)[tri[k]])
    n64 /= np.linalg.norm(n64, axis=1, keepdims=True)
    got = g.reshape(-1, 8)[k, 0:3].astype(np.float64)
    assert np.allclose(got, n64, rtol=1e-5, atol=1e-5), np.abs(got - n64).max()
    # closer to the sphere's own normal than the face normal is, on every compared pixel
    hp = o[k] + d[k] * t[k, None]
    true_n = (hp - pos) / np.linalg.norm(hp - pos, axis=1, keepdims=True)
    m = np.asarray(rd.mesh, np.float64)[tri[k]]
    face = np.cross(m[:, 1] - m[:, 0], m[:, 2] - m[:, 0])
    face /= np.linalg.norm(face, axis=1, keepdims=True)
    e_smooth, e_face = np.linalg.norm(got - true_n, axis=1), np.linalg.norm(face - true_n, axis=1)
    print(f"analytic sphere: {k.size} pixels, shading normal off by <= {e_smooth.max():.2e}, face normal by <= {e_face.max():.2e}")
    assert np.all(e_smooth < e_face), np.count_nonzero(e_smooth >= e_face)
    # albedo x texel at the interpolated UV
    uv = V.interp64(u[k], v[k], np.asarray(rd.uv, np.float64)[tri[k]])
    texel, near = V.texel_of(uv, rd.mat.tex)
    assert near.mean() <= 0.01, near.mean()
    want = np.asarray(rd.mat.albedo, np.float64) * texel
    assert np.allclose(alb.reshape(-1, 3)[k][~near], want[~near], rtol=1e-6, atol=0)
    # and the interpolated UV is the sphere mapping of the hit up to the chord error of the tessellation
    assert np.abs(((uv - _sphere_uv(true_n)) + 0.5) % 1.0 - 0.5)[np.abs(true_n[:, 2]) < 0.9].max() < 0.02


def test_aov_normal_and_albedo_on_an_analytic_sphere(probe):
    render, holder = make_holder(analytic_sphere_scene())
    assert holder.ext is not None
    check_analytic_aov(*V.x86_aov(probe, holder), render)


def check_labelled_aov(g, alb, rend, render, label=""):
    """The triangle the AOVs name is the one a float64 brute-force closest hit finds."""
    rd = render.scene.renderer[1]
    nw, nh = render.frame.res
    o, d = V.camera_rays(render)
    t, tri, u, v, edge = V.brute_hits(o, d, rd.mesh, np.asarray(rd.inst[0][0], np.float64))
    tp = (-0.5 - o[:, 2]) / d[:, 2]                                               # the floor plane in front of the mesh?
    mesh_first = np.isfinite(t) & ~((tp > 0) & (tp < t))
    got_mesh = (rend == 1).reshape(-1)
    table = _fib(np.asarray(rd.mesh).shape[0])
    k = np.flatnonzero(got_mesh)
    by_normal = np.argmax(g.reshape(-1, 8)[k, 0:3].astype(np.float64) @ table.T, 1)
    assert np.all(np.sum(g.reshape(-1, 8)[k, 0:3] * table[by_normal], 1) > 0.99999)
    a = np.rint(alb.reshape(-1, 3)[k].astype(np.float64) * 255.0).astype(np.int64)
    by_albedo = a[:, 0] + 256 * a[:, 1]
    assert np.array_equal(by_normal, by_albedo)                                   # both attributes come from the same row
    named = np.full(nh * nw, -1, np.int64)
    named[k] = by_normal
    want = np.where(mesh_first, tri, -1)
    # the silhouette / edge ring: the float64 hit lies within 1e-4 (barycentric) of its triangle's edge, or the pixel touches a miss
    ringed = (mesh_first & (edge < 1e-4)) | V.ring(mesh_first.reshape(nh, nw)).reshape(-1)
    bad = named != want
    n_hit = int(mesh_first.sum())
    print(f"labelled mesh {label}: {n_hit} hit pixels, {int((ringed & mesh_first).sum())} in the ring, {int(bad.sum())} differ, "
          f"{int((bad & ~ringed).sum())} of them outside the ring")
    assert n_hit > 0.1 * nh * nw
    assert np.count_nonzero(bad & ~ringed) == 0
    assert np.count_nonzero(bad) <= 0.01 * n_hit
    assert len(np.unique(want[want >= 0])) > 0.2 * table.shape[0]                # a fair share of the triangles is seen


@pytest.mark.parametrize("deep_nodes", [0, V.WARM, 1, 40])
@pytest.mark.parametrize("mesh", ["small", "bumpy967"])
def test_aov_names_the_triangle_that_was_hit(probe, mesh, deep_nodes):
    """Fails when the attribute table is not permuted with the packed triangles (binary and 4-wide packing)."""
    from micro_raytracer_amd import scenes
    tris = scenes.icosphere(2, 0.42, (1.5, 0.93, 1.08)) if mesh == "small" else scenes.bumpy_mesh(967)
    render, holder = make_holder(labelled_scene(tris))
    if deep_nodes == 40 and mesh == "small":
        deep_nodes = 8
    check_labelled_aov(*V.x86_aov(probe, holder, deep_nodes), render, f"{mesh} deep_nodes={deep_nodes}")


# ---- 3. closed-form render -------------------------------------------------------------------------------------------------------------
def check_closed_form(mean, render, label=""):
    ref, hit, excl = V.closed_form(render)
    out = excl["silhouette"] | excl["texel"] | excl["terminator"]
    n_hit = int(hit.sum())
    share = np.count_nonzero(out & hit) / n_hit
    cmp_ = ~out
    err = np.abs(mean.astype(np.float64) - ref)
    rel = err / np.maximum(np.abs(ref), 1e-300)
    lit = cmp_[..., None] & (ref > 0)
    print(f"closed form {label}: {n_hit} mesh pixels, excluded {share:.2%} "
          f"({', '.join(f'{k} {int((v & hit).sum())}' for k, v in excl.items())}); lit pixels compared {int(lit[..., 0].sum())}, "
          f"worst relative error {rel[lit].max():.2e}, worst absolute error where the reference is 0: {err[cmp_ & (ref[..., 0] == 0)].max():.2e}")
    assert n_hit > 0.15 * hit.size and lit[..., 0].sum() > 0.3 * n_hit
    assert share <= 0.02, share
    assert np.all(err[cmp_] <= 1e-4 * np.abs(ref[cmp_]))


def closed_form_scene(res=(96, 64), close=False):
    """A smooth textured ellipsoid under one point light.  close: the camera so near that the mesh fills the frame, the light
    next to it -- no silhouette and no terminator in the frame.  (float32 limits what rtol = 1e-4 can ask of them at a large
    frame: the hit distance of a facet seen at a grazing angle carries an error of ~6e-8 / cos, 7e-6 on rim facets at
    cos = 0.02, which moves the interpolated normal by 2e-5; and an interpolated, normalised float32 normal is good to
    ~4e-7, so l.n is good to 1e-4 relative only from 4e-3 up.  At 256 x 256 the far view has 17 such pixels of 38547 outside
    the stated exclusions, worst relative error 3.2e-4; the 96 x 64 frame of the x86 test samples none of them.)"""
    d = analytic_sphere_scene(res, subdiv=2, radius=0.45)
    if close:
        d["frame"]["cam"]["pos"] = [0.02, -0.55, 0.05]
        d["frame"]["cam"]["fov"] = 35
        d["scene"]["light"][0]["pos"] = [-0.15, -0.6, 0.2]
    from micro_raytracer_amd import scenes
    tris = scenes.icosphere(2, 0.45, (1.5, 0.93, 1.08))
    tuv, tvn = scenes.smooth_attrs(tris)
    m = d["scene"]["renderer"][0]
    m["mesh"], m["vn"], m["uv"] = tris.tolist(), tvn.tolist(), tuv.tolist()
    return d


@pytest.mark.parametrize("seed", [1, 2])
def test_bounce0_render_equals_the_closed_form(probe, seed):
    """bounce 0, aprt 0: the render does not depend on the seed, and equals the fold of src/rt.rs:964-993 evaluated in float64 numpy
    with brute-force triangle tests for hit and shadow."""
    render, holder = make_holder(closed_form_scene())
    acc = V.x86_render(probe, holder, seed, 4)
    check_closed_form(acc / f32(4), render, f"x86 seed {seed}")
    if seed == 2:
        assert np.array_equal(acc, V.x86_render(probe, holder, 1, 4))


# ---- 4. nothing moved for scenes without attributes ----------------------------------------------------------------------------------------
def _plan(L, holder, ext):
    from micro_raytracer_amd import _abi
    pl = _abi.Plan()
    if ext == "none":
        rc = L.mrt_plan_launch(C.cast(holder.ptr(), C.c_void_p), C.byref(pl))
    else:
        rc = L.mrt_plan_launch_ext(C.cast(holder.ptr(), C.c_void_p), ext, C.byref(pl))
    assert rc == 0, L.mrt_last_error()
    return {k: getattr(pl, k) for k, _ in pl._fields_ if k != "reserved"}


def _scene_list():
    from micro_raytracer_amd import scenes
    return {"default": scenes.default_scene(res=(64, 48)), "cornell": scenes.cornell_box(res=(64, 64)), "cornell2": scenes.cornell_box2(res=(64, 64), ssaa=1),
            "mesh": scenes.mesh_scene(res=(64, 48)), "mesh5120": scenes.mesh_scene(res=(64, 48), n_tris=5120), "mesh20480": scenes.mesh_scene(res=(64, 48), n_tris=20480),
            "minecraft": scenes.minecraft_like(res=(64, 48), ssaa=1), "grid": scenes.instance_grid(res=(64, 48)), "dof": scenes.dof_scene(res=(64, 48)),
            "sink": scenes.kitchen_sink()}


def test_plan_without_attributes_is_unchanged():
    from micro_raytracer_amd import _abi, _lib
    L = _lib.lib()
    for name, desc in _scene_list().items():
        render, holder = make_holder(desc)
        base = _plan(L, holder, "none")
        assert _plan(L, holder, None) == base, name
        ext = _abi.DescExt()
        attrs = (_abi.TriAttrs * len(render.scene.renderer))()
        ext.n_renderer, ext.attrs = len(render.scene.renderer), C.cast(attrs, C.POINTER(_abi.TriAttrs))
        assert _plan(L, holder, C.cast(C.byref(ext), C.c_void_p)) == base, name
        assert not base["kernel_features"] & F_VATTR


@pytest.mark.parametrize("n_tris", [967, 5120, 20480])
@pytest.mark.parametrize("env", [{}, {"MRT_COLD": "0"}, {"MRT_SCENE_IN_L2": "1"}, {"MRT_DEEP_NODES": "64"}, {"MRT_BLOCK_THREADS": "512"}])
def test_plan_with_attributes_differs_in_kernel_features_only(monkeypatch, n_tris, env):
    from micro_raytracer_amd import _lib, scenes
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for kw in ({"uv": False}, {"vn": False}, {}):
        desc = scenes.mesh_scene(res=(64, 48), n_tris=n_tris)
        _, smooth = make_holder(scenes.smooth_mesh_scene(res=(64, 48), n_tris=n_tris, **kw))
        if "uv" not in kw:            # the same texture tables on both sides: the mesh's texture sits on the plane's rmap slot instead
            desc["scene"]["renderer"][1]["mat"]["rmap"] = scenes.smooth_mesh_scene(res=(64, 48))["scene"]["renderer"][0]["mat"]["tex"]
        _, plain = make_holder(desc)
        a, b = _lib.plan_launch(plain), _lib.plan_launch(smooth)
        kf_a, kf_b = a.pop("kernel_features"), b.pop("kernel_features")
        assert a == b, (kw, a, b)
        assert kf_b & F_VATTR and not kf_a & F_VATTR and (kf_b & F_ALL) == F_ALL
        assert (kf_b & ~(F_VATTR | F_ALL)) == (kf_a & ~(F_VATTR | F_ALL)), (kf_a, kf_b)         # same shape markers, same instance-BVH bit


def test_packed_scene_without_attributes_is_the_same_bytes(probe):
    from micro_raytracer_amd import scenes
    REND_WORDS, REND_FLAGS, REND_VATTR, VATTR_WORDS = 16, 3, 15, 16      # csrc/mrt_scene.h
    _, plain = make_holder(scenes.mesh_scene(res=(64, 48)))
    render, smooth = make_holder(scenes.smooth_mesh_scene(res=(64, 48), uv=False))
    i0, b0 = V.x86_pack(probe, plain)
    i1, b1 = V.x86_pack(probe, smooth, with_ext=False)        # the same scene, its attributes not passed
    assert i0 == i1 and np.array_equal(b0, b1) and i0["n_vattr_rows"] == 0 and not i0["features"] & F_VATTR
    i2, b2 = V.x86_pack(probe, smooth)
    # with attributes: the table is appended behind everything else; of the old words only the renderer's flag and offset change
    assert i2["features"] == i0["features"] | F_VATTR and i2["n_vattr_rows"] == 967
    assert i2["off_vattr"] >= i0["blob_words"] - 3 and i2["blob_words"] == i2["off_vattr"] + 967 * VATTR_WORDS
    for key in ("lds_words", "lds_words_warm", "lds_words_hot", "off_rend"):
        assert i2[key] == i0[key]
    diff = np.flatnonzero(b0 != b2[:b0.size])
    assert set(diff.tolist()) == {i0["off_rend"] + REND_FLAGS, i0["off_rend"] + REND_VATTR}
    assert b2[i0["off_rend"] + REND_FLAGS] == b0[i0["off_rend"] + REND_FLAGS] | 4 and b2[i0["off_rend"] + REND_VATTR] == i2["off_vattr"]
    assert REND_VATTR < REND_WORDS
    # the rows are a permutation of the input rows (the triangles' own permutation: test_aov_names_the_triangle_that_was_hit)
    rows = b2[i2["off_vattr"]:].view(f32).reshape(-1, VATTR_WORDS)
    want = np.asarray(render.scene.renderer[0].vn, f32).reshape(-1, 9)
    assert sorted(map(bytes, rows[:, :9])) == sorted(map(bytes, want)) and np.all(rows[:, 9:] == 0)


def test_attribute_errors(probe):
    from micro_raytracer_amd import _abi, _lib, scenes
    L = _lib.lib()
    render, holder = make_holder(scenes.smooth_mesh_scene(res=(64, 48)))

    def rejected(h):
        pl = _abi.Plan()
        rc = L.mrt_plan_launch_ext(C.cast(h.ptr(), C.c_void_p), h.ext_ptr(), C.byref(pl))
        return rc, L.mrt_last_error().decode()

    assert rejected(holder)[0] == 0
    holder.ext.n_renderer = 1
    rc, msg = rejected(holder)
    assert rc == _abi.MRT_ERR_SCENE and "renderers" in msg
    render, holder = make_holder(scenes.smooth_mesh_scene(res=(64, 48)))
    render.scene.renderer[1].vn = np.zeros((1, 3, 3), f32)                        # on the plane
    rc, msg = rejected(_abi.build_desc(render))
    assert rc == _abi.MRT_ERR_SCENE and "renderer 1" in msg
    render, _ = make_holder(scenes.smooth_mesh_scene(res=(64, 48)))
    render.scene.renderer[0].uv[5, 1, 0] = np.inf
    rc, msg = rejected(_abi.build_desc(render))
    assert rc == _abi.MRT_ERR_SCENE and "renderer 0" in msg and "uv" in msg
    # a texture on a mesh that has normals but no UVs is still refused, through either entry point
    render, _ = make_holder(scenes.smooth_mesh_scene(res=(64, 48)))
    render.scene.renderer[0].uv = None
    h = _abi.build_desc(render)
    rc, msg = rejected(h)
    assert rc == _abi.MRT_ERR_SCENE and "texture maps on a triangle/mesh" in msg
    with pytest.raises(ValueError):
        V.x86_pack(probe, h)
    # a single triangle takes attributes too
    tri = {"rt": {"sample": 1, "bounce": 0}, "frame": {"res": [32, 32], "cam": {"aprt": 0}},
           "scene": {"renderer": [{"type": "triangle", "vtx": [[-1, 1, -1], [1, 1, -1], [0, 1, 1]], "vn": [[[0, -1, 0], [1, -1, 0], [0, -1, 1]]],
                                   "uv": [[[0, 0], [1, 0], [0.5, 1]]], "mat": {"tex": scenes.checker_texture(4, 4, 1)}}]}}
    r, h = make_holder(tri)
    assert rejected(h)[0] == 0
    g, alb, rend = V.x86_aov(probe, h)
    assert (rend == 0).sum() > 100 and len(np.unique(alb[rend == 0], axis=0)) == 2
    n = g[..., 0:3][rend == 0]
    assert np.ptp(n[:, 0]) > 0.3 and np.allclose(np.linalg.norm(n, axis=1), 1, atol=1e-5)


# ---- 5. loader -----------------------------------------------------------------------------------------------------------------------
OBJ = """# two groups; the loader keeps the first one with faces
v 0 0 0
v 1 0 0
v 0 1 0
v 1 1 0.5
vt 0 0
vt 1 0
vt 0 1
vt 1 0.25
vn 0 0 1
vn 0 1 1
vn 1 0 1
g first
f 1/1/1 2/2/2 3/3/3
f 2/2/2 4/4/3 3/3/1 1/1/1
f -3/-3/-2 -1/-1/-1 -2/-2/-3
g second
v 5 5 5
f 1/1/1 2/2/2 5/3/3
"""


def test_obj_loader_reads_vt_and_vn_only_when_asked(tmp_path):
    from micro_raytracer_amd import load_render
    from micro_raytracer_amd.scene import dump_render, load_obj
    (tmp_path / "m.obj").write_text(OBJ)
    (tmp_path / "bare.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//1 3//1\n")

    def scene(extra, name="m.obj"):
        return {"frame": {"res": [16, 16]}, "scene": {"renderer": [dict({"type": "mesh", "mesh": name}, **extra)]}}

    tris = load_obj(str(tmp_path / "m.obj"))
    assert tris.shape == (3, 3, 3)
    plain = load_render(scene({}), base_dir=str(tmp_path)).scene.renderer[0]
    assert plain.uv is None and plain.vn is None and np.array_equal(plain.mesh, tris)        # vn lines alone change nothing
    r = load_render(scene({"uv": True, "vn": True}), base_dir=str(tmp_path)).scene.renderer[0]
    assert np.array_equal(r.mesh, tris)
    vt = np.array([[0, 0], [1, 0], [0, 1], [1, 0.25]], f32)
    vt[:, 1] = f32(1) - vt[:, 1]                                                   # OBJ's origin is bottom left
    vn = np.array([[0, 0, 1], [0, 1, 1], [1, 0, 1]], f32)
    assert np.array_equal(r.uv, vt[[[0, 1, 2], [1, 3, 2], [1, 3, 2]]])             # negative indices count from the end
    assert np.array_equal(r.vn, vn[[[0, 1, 2], [1, 2, 0], [1, 2, 0]]])
    only = load_render(scene({"vn": True}), base_dir=str(tmp_path)).scene.renderer[0]
    assert only.uv is None and np.array_equal(only.vn, r.vn)
    with pytest.raises(ValueError, match="vt"):
        load_render(scene({"uv": True}, "bare.obj"), base_dir=str(tmp_path))
    assert load_render(scene({"vn": True}, "bare.obj"), base_dir=str(tmp_path)).scene.renderer[0].vn.shape == (1, 3, 3)
    with pytest.raises(ValueError):
        load_render({"scene": {"renderer": [{"type": "sphere", "r": 1, "vn": [[[0, 0, 1]] * 3]}]}})
    with pytest.raises(ValueError):
        load_render(scene({"vn": [[[0, 0, 1]] * 3]}), base_dir=str(tmp_path))       # 1 triangle of normals, 3 of mesh
    # JSON round trip through the dump, nested lists and the inline form
    from micro_raytracer_amd.scene import attr_to_inline
    full = load_render(scene({"uv": True, "vn": True}), base_dir=str(tmp_path))
    back = load_render(json.loads(json.dumps(dump_render(full))))
    assert np.array_equal(back.scene.renderer[0].uv, r.uv) and np.array_equal(back.scene.renderer[0].vn, r.vn)
    inl = load_render(scene({"uv": attr_to_inline(r.uv), "vn": attr_to_inline(r.vn)}), base_dir=str(tmp_path)).scene.renderer[0]
    assert np.array_equal(inl.uv, r.uv) and np.array_equal(inl.vn, r.vn)
    assert "uv" not in dump_render(load_render(scene({}), base_dir=str(tmp_path)))["scene"]["renderer"][0]


def test_fingerprint_and_descriptor_cover_the_attributes():
    from micro_raytracer_amd import _abi, load_render, scenes
    from micro_raytracer_amd.sampler import _fingerprint
    r = load_render(scenes.smooth_mesh_scene(res=(32, 32)))
    fp = _fingerprint(r)
    r.scene.renderer[0].vn = r.scene.renderer[0].vn[::-1].copy()
    assert _fingerprint(r) != fp
    h = _abi.build_desc(r)
    assert h.ext.n_renderer == 2 and bool(h.ext.attrs[0].vn) and bool(h.ext.attrs[0].uv) and not h.ext.attrs[1].vn
    assert _abi.build_desc(load_render(scenes.mesh_scene(res=(32, 32)))).ext is None
    r.scene.renderer[0].uv = r.scene.renderer[0].uv[:5]
    with pytest.raises(ValueError):
        _abi.build_desc(r)


def test_smooth_scene_attributes_are_sound():
    from micro_raytracer_amd import scenes
    tris = scenes.bumpy_mesh(967)
    uv, vn = scenes.smooth_attrs(tris)
    assert uv.shape == (967, 3, 2) and vn.shape == (967, 3, 3)
    assert np.allclose(np.linalg.norm(vn, axis=2), 1, atol=1e-6)
    t = tris.astype(np.float64)
    face = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    face /= np.linalg.norm(face, axis=1, keepdims=True)
    assert np.sum(vn * face[:, None], 2).min() > 0.5                               # vertex normals stay on their faces' side
    assert np.abs(uv[:, :, 0] - uv[:, :1, 0]).max() <= 0.5                        # no triangle spans the seam
