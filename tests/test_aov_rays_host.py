"""First-hit AOVs on caller-supplied rays and the a-trous filter on a frame periodic in x (mrt_aov_rays) without a
GPU: csrc/mrt_denoise.h compiled for x86 (tests/emu/aov_rays_probe.cpp).

1. aov_ray on the camera's own lens-centre rays is aov_pixel, and the oracle's orc_aov, bit for bit on every plane;
2. on the rays of cameras.equirect it answers what the oracle's orc_ray_query answers (hit, ids, t0 bits, normal bits), the world
   point is float32 o + d * t0 and an untextured hit has its material's albedo;
3. rays with NaN, inf and zero components meet orc_ray_query too;
4. the wrapped pass against a numpy restatement written here, its invariance under a roll of the columns, and what the flag
   changes and leaves alone against the unwrapped filter;
5, 6. the symbol list and the CLI's rules.

The helpers serve tests/test_gpu_aov_rays.py as well."""
import ctypes as C
import os

import numpy as np
import pytest

import test_denoise_host as D
from conftest import make_holder
from emu.build import desc_ptrs as _ptrs, ptr as _p, shared

f32 = np.float32
SIGMAS = ((0.5, 0.25, 0.05), (2.0, np.inf, 0.3))
WRAP_SHAPES = ((37, 9), (80, 24), (24, 8), (5, 7))          # nw x nh: 37: nw % s != 0; 24 and 5: 2 s >= nw, several wraps per tap


# ---- the probe -----------------------------------------------------------------------------------------------------------------
def _bind(L):
    fp, u32p, i32p, vp, u32 = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_void_p, C.c_uint32
    L.ar_error.restype = C.c_char_p
    L.ar_dims.argtypes = [vp, vp, u32p]
    L.ar_camera_rays.argtypes = [vp, vp, fp, fp]
    L.ar_aov_pixel.argtypes = [vp, vp, fp, fp, i32p, i32p]
    L.ar_aov_rays.argtypes = [vp, vp, C.c_uint64, fp, fp, fp, fp, i32p, i32p]
    L.ar_pass.argtypes = [fp, fp, u32, u32, u32, C.c_float, C.c_float, C.c_float, u32, fp]
    L.ar_filter.argtypes = [fp, u32p, fp, fp, u32, u32, u32, C.c_float, C.c_float, C.c_float, u32, u32, fp]


def shared_probe():
    """The probe, built once per process for both modules."""
    return shared("aov_rays_probe", _bind)


@pytest.fixture(scope="module")
def probe():
    return shared_probe()


def x86_dims(L, holder):
    v = np.zeros(2, np.uint32)
    assert L.ar_dims(*_ptrs(holder), _p(v, C.c_uint32)) == 0, L.ar_error()
    return int(v[0]), int(v[1])


def x86_camera_rays(L, holder):
    nw, nh = x86_dims(L, holder)
    o, d = np.zeros((nh, nw, 3), f32), np.zeros((nh, nw, 3), f32)
    assert L.ar_camera_rays(*_ptrs(holder), _p(o), _p(d)) == 0, L.ar_error()
    return o, d


def _planes(g, alb, rend, inst):
    return {"depth": g[..., 3], "normal": g[..., 0:3], "point": g[..., 4:7], "albedo": alb, "renderer": rend, "instance": inst,
            "hit": g[..., 7] != 0, "guide": g}


def x86_aov_pixel(L, holder):
    nw, nh = x86_dims(L, holder)
    g, alb = np.zeros((nh, nw, 8), f32), np.zeros((nh, nw, 3), f32)
    rend, inst = np.zeros((nh, nw), np.int32), np.zeros((nh, nw), np.int32)
    assert L.ar_aov_pixel(*_ptrs(holder), _p(g), _p(alb), _p(rend, C.c_int32), _p(inst, C.c_int32)) == 0, L.ar_error()
    return _planes(g, alb, rend, inst)


def x86_aov_rays(L, holder, orig, dir):
    """aov_ray on rays of any shape [..., 3]: the planes of Sampler.aov() plus point, hit and the raw guide, in the rays' shape."""
    o, d = np.ascontiguousarray(orig, f32), np.ascontiguousarray(dir, f32)
    assert o.shape == d.shape and o.shape[-1] == 3
    sh = o.shape[:-1]
    n = o.size // 3
    g, alb = np.zeros(sh + (8,), f32), np.zeros(sh + (3,), f32)
    rend, inst = np.zeros(sh, np.int32), np.zeros(sh, np.int32)
    assert L.ar_aov_rays(*_ptrs(holder), n, _p(o), _p(d), _p(g), _p(alb), _p(rend, C.c_int32), _p(inst, C.c_int32)) == 0, L.ar_error()
    return _planes(g, alb, rend, inst)


def x86_filter(L, A, counts, g, alb, passes, sc, sn, sp, wrap_x, env=False):
    nh, nw = counts.shape
    out = np.zeros((nh, nw, 3), f32)
    L.ar_filter(_p(np.ascontiguousarray(A, f32)), _p(np.ascontiguousarray(counts, np.uint32), C.c_uint32), _p(np.ascontiguousarray(g, f32)),
                _p(np.ascontiguousarray(alb, f32)), nw, nh, passes, sc, sn, sp, int(env), int(wrap_x), _p(out))
    return out


def same_planes(a, b, keys=("depth", "normal", "albedo", "point")):
    """Mismatching words per plane of two plane dicts (NaN equal to NaN), ids and hit masks included: all zeros when they agree."""
    out = {k: D.same_bits(a[k], b[k]) for k in keys if k in a and k in b}
    out.update({k: int(np.count_nonzero(a[k] != b[k])) for k in ("renderer", "instance", "hit") if k in a and k in b})
    return out


def agree(a, b, **kw):
    return not any(same_planes(a, b, **kw).values())


# ---- 1: the camera's rays ----------------------------------------------------------------------------------------------------------
def camera_scenes():
    from micro_raytracer_amd import scenes
    dof = scenes.cornell_box(res=(64, 48), sample=4)
    dof["frame"]["cam"].update({"aprt": 0.3, "foc": 1.2})
    return {"cornell": scenes.cornell_box(res=(64, 48), sample=4), "cornell_aprt": dof,
            "env": scenes.env_scene(res=(64, 40), sample=4, tex_res=(64, 32)),
            "env_bilinear": scenes.env_scene(res=(48, 32), sample=4, mapping="latlong", tex_res=(64, 32), filter="bilinear"),
            "mesh_vn_uv": scenes.smooth_mesh_scene(res=(64, 40), sample=4)}


@pytest.mark.parametrize("name", list(camera_scenes()))
def test_aov_ray_on_the_camera_rays_is_aov_pixel_and_the_oracle(probe, oracle_mod, name):
    import test_oracle_aov as T
    render, holder = make_holder(camera_scenes()[name])
    o, d = x86_camera_rays(probe, holder)
    got = x86_aov_rays(probe, holder, o, d)
    want = x86_aov_pixel(probe, holder)
    assert agree(got, want), (name, same_planes(got, want))
    assert got["hit"].sum() > 0.3 * got["hit"].size
    if "env" in name:
        miss = ~got["hit"]
        assert miss.sum() > 20 and np.all(got["albedo"][miss].max(axis=-1) > 0)          # the backdrop E(d), not 0
    T.compare_aov(f"aov_ray, camera rays, {name}", got, T.oracle_aov(oracle_mod, holder))


# ---- 2, 3: rays no pinhole forms -------------------------------------------------------------------------------------------------
def against_ray_query(label, got, words, o, d):
    """The planes of aov_ray (flat, [n]) against orc_ray_query's words 0, 2, 3, 4, 6..8 and float32 o + d * t0."""
    hit = words[:, 0] != 0
    assert np.array_equal(got["hit"], hit), label
    assert np.array_equal(got["renderer"], words[:, 2].astype(np.int32)) and np.array_equal(got["instance"], words[:, 3].astype(np.int32)), label
    assert np.all(got["renderer"][~hit] == -1) and np.all(got["instance"][~hit] == -1), label
    t0 = np.ascontiguousarray(got["depth"], f32)
    assert D.same_bits(t0[hit], np.ascontiguousarray(words[hit, 4]).view(f32)) == 0, label
    assert np.all(np.isposinf(t0[~hit])), label
    assert D.same_bits(got["normal"], np.ascontiguousarray(words[:, 6:9]).view(f32)) == 0, label
    with np.errstate(all="ignore"):
        p = (o + (d * t0[:, None]).astype(f32)).astype(f32)
    assert D.same_bits(got["point"][hit], p[hit]) == 0, label
    assert np.all(got["point"][~hit] == 0) and np.all(got["guide"][..., 7][hit] == 1) and np.all(got["guide"][..., 7][~hit] == 0), label
    return hit


def equirect_cases():
    from micro_raytracer_amd import scenes
    return {"cornell": scenes.cornell_box(res=(64, 32), sample=4), "env": scenes.env_scene(res=(64, 32), sample=4, tex_res=(64, 32))}


@pytest.mark.parametrize("name", list(equirect_cases()))
def test_equirect_rays_meet_the_oracles_ray_query(probe, oracle_mod, name):
    from micro_raytracer_amd import _abi, cameras
    render, holder = make_holder(equirect_cases()[name])
    nw, nh = x86_dims(probe, holder)
    assert (nw, nh) == (64, 32)
    o, d = cameras.equirect(render.frame.cam.pos, nw, nh)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    got = x86_aov_rays(probe, holder, o, d)
    orc = oracle_mod.Oracle(holder, seed=1)
    words = orc.ray_query(o, d)
    orc.close()
    hit = against_ray_query(name, got, words, o, d)
    if name == "cornell":
        assert hit.all()                                      # inside the box every direction ends on a wall or a sphere
    else:
        assert 0.2 < hit.mean() < 0.95
        assert np.all(got["albedo"][~hit].max(axis=-1) > 0)
    checked = 0
    for r, rd in enumerate(render.scene.renderer):
        if any(getattr(rd.mat, k) is not None for k in _abi.MAP_SLOTS):
            continue
        sel = got["renderer"] == r
        checked += int(sel.sum())
        assert np.array_equal(got["albedo"][sel], np.broadcast_to(np.asarray(rd.mat.albedo, f32), (int(sel.sum()), 3))), (name, r)
    assert checked > 0.2 * hit.size


def special_ray_cases():
    """A handful of the rays of radiance_cases.extra(): the 40 with NaN, inf and zero components and 24 ordinary ones."""
    import radiance_cases as RC
    out = {}
    for c in RC.extra():
        if c.name in ("extra/triangles_crowd", "extra/triangles_env_sphere_bilinear"):
            pick = np.r_[0:24, len(c.o) - 40:len(c.o)]
            out[c.name] = (c.desc, c.o[pick], c.d[pick])
    return out


def test_rays_with_nan_inf_and_zero_components(probe, oracle_mod):
    cases = special_ray_cases()
    assert len(cases) == 2
    for name, (desc, o, d) in cases.items():
        assert (~np.isfinite(o) | ~np.isfinite(d)).any() and (d == 0).any(), name
        _, holder = make_holder(desc)
        got = x86_aov_rays(probe, holder, o, d)
        orc = oracle_mod.Oracle(holder, seed=1)
        words = orc.ray_query(o, d)
        orc.close()
        against_ray_query(name, got, words, np.ascontiguousarray(o, f32), np.ascontiguousarray(d, f32))


# ---- 4: the wrapped pass ---------------------------------------------------------------------------------------------------------
def np_filter_wrap(A, counts, g, alb, passes, sc, sn, sp):
    """The filter of DESIGN.md §13 on a frame periodic in x (§20), float32 in its operation order: the horizontal tap of column x
    is column (x + s * dx) mod nw, every column counts; rows outside the frame are skipped."""
    nh, nw = counts.shape
    K5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], f32)
    with np.errstate(all="ignore"):
        c = A * (f32(1.0) / counts.astype(f32))[..., None]
        if passes == 0:
            return c
        hit = g[..., 7]
        Dm = np.where((hit != 0)[..., None], np.fmax(alb, f32(1 / 256)), f32(1.0))
        e = (c / Dm).astype(f32)
        n, t, x = g[..., 0:3], g[..., 3], g[..., 4:7]
        on = hit != 0
        for i in range(passes):
            s = 1 << i
            sci = f32(f32(sc) * f32(4 ** i))
            num = np.zeros_like(e)
            den = np.zeros((nh, nw), f32)
            for dy in range(-2, 3):
                ys = np.arange(nh) + s * dy
                vy = (ys >= 0) & (ys < nh)
                yq = np.clip(ys, 0, nh - 1)
                for dx in range(-2, 3):
                    xq = np.mod(np.arange(nw) + s * dx, nw)              # a true modulo: numpy's sign follows the divisor
                    eq, hq, nq, pq = e[yq][:, xq], hit[yq][:, xq], n[yq][:, xq], x[yq][:, xq]
                    k = f32(K5[dx + 2] * K5[dy + 2])
                    dc = e - eq
                    wc = np.fmax(f32(0), f32(1) - ((dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]) * sci)
                    m = n - nq
                    wn = np.fmax(f32(0), f32(1) - ((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]) * f32(sn))
                    u = pq - x
                    r = ((n[..., 0] * u[..., 0] + n[..., 1] * u[..., 1]) + n[..., 2] * u[..., 2]) / t
                    wp = np.fmax(f32(0), f32(1) - (r * r) * f32(sp))
                    w = ((k * wc) * np.where(on, wn, f32(1))) * np.where(on, wp, f32(1))
                    w = np.where(vy[:, None] & (hit == hq), w, f32(0)).astype(f32)
                    use = w > 0
                    num = np.where(use[..., None], num + w[..., None] * eq, num)
                    den = np.where(use, den + w, den)
            e = np.where((den > 0)[..., None], num / den[..., None], e).astype(f32)
        return (e * Dm).astype(f32)


def wrap_case(shape):
    nw, nh = shape
    return D.random_case(np.random.default_rng(nw * 1000 + nh), nh, nw)


def seam_reach(passes):
    """Columns from either edge the unwrapped filter's missing taps can reach after `passes` passes."""
    return 2 * sum(1 << i for i in range(passes))


@pytest.mark.parametrize("shape", WRAP_SHAPES)
def test_wrapped_filter_x86_matches_numpy(probe, shape):
    A, counts, g, alb = wrap_case(shape)
    for passes in range(1, 6):
        for sig in SIGMAS:
            sc, sn, sp = (D.inv_sq(s) for s in sig)
            got = x86_filter(probe, A, counts, g, alb, passes, sc, sn, sp, True)
            assert D.same_bits(got, np_filter_wrap(A, counts, g, alb, passes, sc, sn, sp)) == 0, (shape, passes, sig)


@pytest.mark.parametrize("shape", WRAP_SHAPES)
def test_wrapped_filter_commutes_with_a_roll_of_the_columns(probe, shape):
    A, counts, g, alb = wrap_case(shape)
    nw = shape[0]
    for passes in (1, 3, 5):
        sc, sn, sp = (D.inv_sq(s) for s in SIGMAS[1])
        base = x86_filter(probe, A, counts, g, alb, passes, sc, sn, sp, True)
        for k in (1, 7, nw - 1):
            rolled = x86_filter(probe, *(np.roll(a, k, axis=1) for a in (A, counts, g, alb)), passes, sc, sn, sp, True)
            assert D.same_bits(rolled, np.roll(base, k, axis=1)) == 0, (shape, passes, k)


@pytest.mark.parametrize("shape", WRAP_SHAPES)
def test_unwrapped_filter_is_unchanged_and_differs_at_the_seam(probe, shape):
    A, counts, g, alb = wrap_case(shape)
    nw = shape[0]
    for passes in range(1, 6):
        sc, sn, sp = (D.inv_sq(s) for s in (np.inf, np.inf, np.inf))      # every tap of the pixel's own hit class has a weight > 0
        off = x86_filter(probe, A, counts, g, alb, passes, sc, sn, sp, False)
        assert D.same_bits(off, D.np_filter(A, counts, g, alb, passes, sc, sn, sp)) == 0, (shape, passes)
        on = x86_filter(probe, A, counts, g, alb, passes, sc, sn, sp, True)
        differs = ((np.ascontiguousarray(on).view(np.uint32) != np.ascontiguousarray(off).view(np.uint32))
                   & ~(np.isnan(on) & np.isnan(off))).any(axis=(0, 2))                    # per column
        reach = seam_reach(passes)
        seam = np.zeros(nw, bool)
        seam[:reach] = True
        seam[max(nw - reach, 0):] = True
        assert differs[seam].any(), (shape, passes)                     # the flag acts ...
        assert not differs[~seam].any(), (shape, passes)                # ... and only as far as the missing taps reach


# ---- 5, 6: the symbol and the CLI ----------------------------------------------------------------------------------------------------
def test_lib_symbols_list_mrt_aov_rays():
    from conftest import ROOT
    from micro_raytracer_amd import _abi, _lib
    hdr = open(os.path.join(ROOT, "include", "mrt.h")).read()
    assert "mrt_aov_rays" in _lib.SYMBOLS and "int mrt_aov_rays(" in hdr
    assert f"#define MRT_AOV_RAYS_DEVICE {_abi.AOV_RAYS_DEVICE}u" in hdr and f"#define MRT_AOV_WRAP_X {_abi.AOV_WRAP_X}u" in hdr
    assert "#define MRT_ABI_VERSION 3" in hdr


def test_cli_pano_guides_rules(capsys):
    from micro_raytracer_amd.__main__ import main
    with pytest.raises(SystemExit):
        main(["scene.json", "--pano-guides"])
    assert "--pano-guides needs --camera equirect" in capsys.readouterr().err
    for extra in (["--denoise"], ["--aov", "x"]):
        with pytest.raises(SystemExit):
            main(["scene.json", "--camera", "equirect", *extra])
        assert "--pano-guides" in capsys.readouterr().err
    for extra in (["--adaptive", "0.1"], ["--update"], ["--denoise", "--denoise-mode", "variance"]):
        with pytest.raises(SystemExit):
            main(["scene.json", "--camera", "equirect", "--pano-guides", *extra])
        capsys.readouterr()


def test_render_equirect_guides_calls_aov_rays_with_the_same_rays():
    """cameras.render_equirect(guides=True) hands aov_rays the rays it rendered, with wrap_x; the default leaves it out."""
    from micro_raytracer_amd import cameras

    class Fake:
        nw, nh = 8, 4
        calls = []

        def create(self, render):
            return self

        def radiance(self, render, o, d, n, info=None):
            self.calls.append(("radiance", o, d))
            return np.zeros_like(o)

        def set_accum(self, rgb, n):
            self.calls.append(("set_accum", n))

        def aov_rays(self, render, o, d, *, wrap_x=False):
            self.calls.append(("aov_rays", o, d, wrap_x))

    class R:
        class rt:
            sample = 2

        class frame:
            class cam:
                pos = (0.0, 0.0, 0.0)

    s = Fake()
    cameras.render_equirect(s, R)
    assert [c[0] for c in s.calls] == ["radiance", "set_accum"]
    s.calls.clear()
    cameras.render_equirect(s, R, guides=True)
    assert [c[0] for c in s.calls] == ["radiance", "set_accum", "aov_rays"]
    assert s.calls[2][1] is s.calls[0][1] and s.calls[2][2] is s.calls[0][2] and s.calls[2][3] is True
