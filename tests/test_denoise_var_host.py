"""The variance-guided denoiser mode without a GPU: csrc/mrt_denoise_var.h compiled for x86
(tests/emu/var_probe.cpp) against the numpy float32 restatement of tests/var_ref.py, bit for bit; the filter's properties (the
mean at passes = 0, fixed points, edges that stop at zero variance and blend at a large one, the firefly clamp); its quality on
oracle renders against the a-trous mode on the same input; the Python option and CLI helpers."""
import ctypes as C
import os

import numpy as np
import pytest

import var_ref as V
from conftest import ROOT
from test_denoise_host import shared_probe as shared_dn_probe
from test_denoise_host import random_case, tonemapped, x86_aov
from test_denoise_host import x86_filter as x86_atrous

f32 = np.float32
INF = float("inf")
SN, SP = V.inv_sq(0.25), V.inv_sq(0.05)


@pytest.fixture(scope="module")
def probe():
    return V.shared_probe()


@pytest.fixture(scope="module")
def dn_probe():
    return shared_dn_probe()


def var_case(rng, nh, nw):
    """random_case of test_denoise_host with mixed 8x8 tile counts and a half buffer: 0 <= H <= A in the ordinary pixels (between
    A and 0 in the negative ones), NaN and inf in a few more."""
    A, _, g, alb = random_case(rng, nh, nw, count=64)
    tiles = rng.choice([32, 64, 96], size=((nh + 7) // 8, (nw + 7) // 8)).astype(np.uint32)
    counts = np.ascontiguousarray(np.repeat(np.repeat(tiles, 8, 0), 8, 1)[:nh, :nw])
    with np.errstate(invalid="ignore"):
        H = (A * rng.uniform(0.0, 1.0, (nh, nw, 3)).astype(f32)).astype(f32)
    sel = rng.random((nh, nw))
    H[sel < 0.01] = np.nan
    H[(sel >= 0.01) & (sel < 0.02)] = np.inf
    H[(sel >= 0.02) & (sel < 0.03)] = -np.inf
    return A, H, counts, g, alb


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 13), (67, 129)])
def test_var_filter_x86_matches_numpy(probe, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + 17)
    nh, nw = shape
    A, H, counts, g, alb = var_case(rng, nh, nw)
    assert shape != (67, 129) or len(np.unique(counts)) == 3
    for sigma_var in (4.5, 1.0, INF):
        for firefly in (1.0, 2.0, INF):
            sv = V.inv_sq(sigma_var)
            ref, ref_var = V.np_chain(A, H, counts, g, alb, 6, sv, SN, SP, firefly)
            for passes in range(7):
                got, var = V.x86_filter(probe, A, H, counts, g, alb, passes, sv, SN, SP, firefly, want_var=True)
                assert V.same_bits(got, ref[passes]) == 0, (shape, passes, sigma_var, firefly)
                assert V.same_bits(var, ref_var[passes]) == 0, (shape, passes, sigma_var, firefly)


def test_var_filter_env_and_other_guide_sigmas(probe):
    """Environment contexts demodulate miss pixels by their albedo (the backdrop) too; a guide term switched off."""
    rng = np.random.default_rng(23)
    A, H, counts, g, alb = var_case(rng, 19, 26)
    miss = g[..., 7] == 0
    alb[miss] = rng.random((int(miss.sum()), 3)).astype(f32)
    for env in (False, True):
        for sn, sp in ((SN, SP), (V.inv_sq(INF), V.inv_sq(0.3))):
            ref, _ = V.np_chain(A, H, counts, g, alb, 4, V.inv_sq(4.5), sn, sp, 1.0, env)
            for passes in (0, 1, 4):
                got = V.x86_filter(probe, A, H, counts, g, alb, passes, V.inv_sq(4.5), sn, sp, 1.0, env)
                assert V.same_bits(got, ref[passes]) == 0, (env, passes)
    on = V.x86_filter(probe, A, H, counts, g, alb, 2, V.inv_sq(4.5), SN, SP, 1.0, True)
    off = V.x86_filter(probe, A, H, counts, g, alb, 2, V.inv_sq(4.5), SN, SP, 1.0, False)
    assert V.same_bits(on[miss], off[miss]) > 0


def flat_plane(nh, nw, albedo=0.5):
    """One plane z = 2 seen head-on: equal normals, depths and albedo, so that every guide weight is 1."""
    g = np.zeros((nh, nw, 8), f32)
    g[..., 2] = 1.0
    g[..., 3] = 2.0
    yy, xx = np.mgrid[0:nh, 0:nw]
    g[..., 4] = xx * 0.01
    g[..., 5] = yy * 0.01
    g[..., 6] = 2.0
    g[..., 7] = 1.0
    return g, np.full((nh, nw, 3), albedo, f32), np.full((nh, nw), 32, np.uint32)


def test_var_passes0_is_the_mean_and_flat_frames_stay(probe):
    rng = np.random.default_rng(9)
    A, H, counts, g, alb = var_case(rng, 9, 11)
    out = V.x86_filter(probe, A, H, counts, g, alb, 0, V.inv_sq(4.5), SN, SP, 1.0)
    assert V.same_bits(out, A * (f32(1) / counts.astype(f32))[..., None]) == 0
    g, alb, counts = flat_plane(13, 17)
    A = np.full((13, 17, 3), 16.0, f32)
    for firefly in (1.0, INF):
        out, var = V.x86_filter(probe, A, A * f32(0.5), counts, g, alb, 5, V.inv_sq(4.5), SN, SP, firefly, want_var=True)
        assert np.array_equal(out, np.full_like(out, 0.5))
        assert np.all(var == 0)


def step_edge(nh=15, nw=24, lo=8.0, hi=32.0):
    """e = 0.5 | 2 (powers of two: a weighted mean of equal values is then exact), the means 0.25 | 1."""
    g, alb, counts = flat_plane(nh, nw)
    A = np.full((nh, nw, 3), lo, f32)
    A[:, nw // 2:] = hi
    return A, g, alb, counts


def test_var_zero_variance_stops_an_edge(probe):
    """H = A/2: both halves agree, the variance is zero everywhere, and a step edge in e across one plane of equal guides comes
    back unchanged on both sides -- nothing but the variance tells the two sides apart."""
    A, g, alb, counts = step_edge()
    mean = A * (f32(1) / f32(32))
    for passes in (1, 3, 5):
        out, var = V.x86_filter(probe, A, A * f32(0.5), counts, g, alb, passes, V.inv_sq(4.5), SN, SP, INF, want_var=True)
        assert np.array_equal(out, mean), passes
        assert np.all(var == 0)


def test_var_large_variance_blends_the_same_edge(probe):
    """The same edge with a large uniform |j - k|: the halves disagree by much more than the step, so the filter blends it."""
    A, g, alb, counts = step_edge()
    H = (A * f32(0.5) + f32(16.0) * f32(8.0)).astype(f32)          # h = (j - k) / 2 = 16 in e units, the step is 1.5
    mean = A * (f32(1) / f32(32))
    row, c = A.shape[0] // 2, A.shape[1] // 2
    before = float(mean[row, c, 0] - mean[row, c - 1, 0])
    out, var = V.x86_filter(probe, A, H, counts, g, alb, 3, V.inv_sq(4.5), SN, SP, INF, want_var=True)
    after = float(out[row, c, 0] - out[row, c - 1, 0])
    print(f"centre-row step {before:.4f} -> {after:.4f}")
    assert before == 0.75 and 0 <= after < 0.5 * before
    assert np.all(var > 0)


def test_var_firefly_clamp(probe):
    """One pixel at 100 x its constant neighbourhood leaves the prep step with lum == f * m to within 2 ulp (the clamp scales the
    three channels by one rounded quotient); with the clamp off it is untouched.  Its h2 is not clamped."""
    g, alb, counts = flat_plane(9, 9)
    A = np.empty((9, 9, 3), f32)
    A[:] = (8.0, 12.0, 5.0)
    A[4, 4] *= f32(100)
    H = (A * f32(0.25)).astype(f32)
    raw = V.x86_prep(probe, A, H, counts, g, alb, INF)
    m = V.lum(raw[0, 0, 0:3])
    assert V.same_bits(raw[..., 0:3], (A * (f32(1) / f32(32))) / f32(0.5)) == 0
    for f in (1.0, 2.0):
        ev = V.x86_prep(probe, A, H, counts, g, alb, f)
        got, want = V.lum(ev[4, 4, 0:3]), f32(f) * m
        assert abs(float(got) - float(want)) <= 2 * float(np.spacing(want)), (f, got, want)
        others = np.ones((9, 9), bool)
        others[4, 4] = False
        assert V.same_bits(ev[others], raw[others]) == 0             # the neighbours' maxima use the unclamped e: no cascade
        assert ev[4, 4, 3] == raw[4, 4, 3] and raw[4, 4, 3] > 9e3 * raw[0, 0, 3] > 0
        assert V.same_bits(ev, V.np_prep(A, H, counts, g, alb, f)) == 0
    # a pixel whose neighbours all belong to another surface (hit flag) is left alone
    g[4, 4, 7] = 0.0
    assert V.same_bits(V.x86_prep(probe, A, H, counts, g, alb, 1.0)[4, 4], V.x86_prep(probe, A, H, counts, g, alb, INF)[4, 4]) == 0


# ---- quality against the oracle -------------------------------------------------------------------------------------------
def quality_scenes():
    from micro_raytracer_amd import scenes
    return {"cornell_box": lambda: scenes.cornell_box(res=(160, 120), sample=32),
            "mesh_scene": lambda: scenes.mesh_scene(res=(192, 108), sample=32),
            "minecraft_like": lambda: scenes.minecraft_like(res=(192, 108), ssaa=1, sample=32),
            "dof_scene": lambda: scenes.dof_scene(res=(192, 108), sample=32)}


def oracle_case(oracle_mod, dn_probe, name, spp=32):
    """A, H, the AOVs and the tone-mapped 512-spp reference of one scene: seed 3, H = the first spp/2 samples (the even rounds of
    an adaptive render with step = spp/2); the reference seed 777."""
    from micro_raytracer_amd import _abi, load_render
    render = load_render(quality_scenes()[name]())
    holder = _abi.build_desc(render)
    nw, nh = render.frame.res
    o = oracle_mod.Oracle(holder, seed=3)
    o.execute(spp // 2)
    H = o.accum()[0].copy()
    o.execute(spp // 2)
    A, cnt = o.accum()
    assert cnt == spp
    gt = oracle_mod.Oracle(holder, seed=777)
    gt.execute(512)
    G, _ = gt.accum()
    g, alb, _, _ = x86_aov(dn_probe, holder, nw, nh)
    cam = render.frame.cam
    ref = tonemapped(G / f32(512), cam.gamma, cam.exp)
    err = lambda img: float(np.sqrt(np.mean((tonemapped(img, cam.gamma, cam.exp) - ref) ** 2)))
    return A.copy(), H, np.full((nh, nw), spp, np.uint32), g, alb, err


@pytest.mark.parametrize("name", ["cornell_box", "mesh_scene", "minecraft_like", "dof_scene"])
def test_var_quality_beats_atrous(probe, dn_probe, oracle_mod, name):
    """Both modes at their defaults on the same 32-spp oracle render: the variance mode's tone-mapped RMSE against 512 spp is the
    lower one (DESIGN.md §17 holds the measured table)."""
    from micro_raytracer_amd import _abi
    A, H, counts, g, alb, err = oracle_case(oracle_mod, dn_probe, name)
    raw = err(A / f32(32))
    sn, sp = V.inv_sq(_abi.DENOISE_SIGMA_NORMAL), V.inv_sq(_abi.DENOISE_SIGMA_PLANE)
    atrous = err(x86_atrous(dn_probe, A, counts, g, alb, _abi.DENOISE_PASSES, V.inv_sq(_abi.DENOISE_SIGMA_COLOR), sn, sp))
    var = err(V.x86_filter(probe, A, H, counts, g, alb, _abi.DENOISE_PASSES, V.inv_sq(_abi.DN_SIGMA_VAR), sn, sp, _abi.DN_FIREFLY))
    print(f"{name} 32 spp, {_abi.DENOISE_PASSES} passes: raw RMSE {raw:.4f}, a-trous {atrous:.4f} ({atrous / raw:.3f} x raw), "
          f"variance {var:.4f} ({var / raw:.3f} x raw), variance / a-trous {var / atrous:.3f}")
    assert var < atrous


# ---- Python options and CLI helpers ------------------------------------------------------------------------------------
def test_var_opts_map_to_the_struct_words():
    import re
    from micro_raytracer_amd import _abi
    assert C.sizeof(_abi.DenoiseOpts) == 32 and C.sizeof(_abi.DenoiseInfo) == 32
    words = lambda o: np.frombuffer(bytes(o), np.uint32)
    o = _abi.denoise_opts()
    assert (o.mode, o.sigma_var, o.firefly) == (0, 0.0, 0.0) and not words(o)[4:].any()        # the default call: the words it always had
    o = _abi.denoise_opts(3, mode="variance")
    assert (o.passes, o.mode, o.sigma_var, o.firefly) == (3, 1, 0.0, 0.0)                      # None -> 0, the library's default
    assert o.sigma_normal == f32(_abi.DENOISE_SIGMA_NORMAL)
    o = _abi.denoise_opts(mode="variance", sigma_var=3.0, firefly=INF)
    w = words(o)
    assert w[4] == 1 and w[5:6].view(f32)[0] == f32(3.0) and np.isposinf(w[6:7].view(f32)[0]) and w[7] == 0
    with pytest.raises(ValueError):
        _abi.denoise_opts(mode="median")
    hdr = open(os.path.join(ROOT, "include", "mrt.h")).read()
    val = {k: float(v.rstrip("uf")) for k, v in re.findall(r"#define MRT_DN_(\w+) ([0-9.]+[uf]?)", hdr)}
    assert val == {"ATROUS": _abi.DN_MODES["atrous"], "VARIANCE": _abi.DN_MODES["variance"], "SIGMA_VAR": _abi.DN_SIGMA_VAR,
                   "FIREFLY": _abi.DN_FIREFLY}
    # the struct as the header spells it
    body = re.search(r"typedef struct mrt_denoise_opts \{(.*?)\} mrt_denoise_opts;", hdr, re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in _abi.DenoiseOpts._fields_]


def test_cli_rejects_unknown_mode_and_odd_sample_counts(capsys):
    from micro_raytracer_amd.__main__ import main
    with pytest.raises(SystemExit):
        main(["scene.json", "--denoise", "--denoise-mode", "median"])
    with pytest.raises(SystemExit):
        main(["scene.json", "--denoise", "--denoise-mode", "variance", "--sample", "48"])
    assert "multiple of 32" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main(["scene.json", "--denoise", "--denoise-sigma-var", "3"])          # the a-trous mode has no sigma_var
    with pytest.raises(SystemExit):
        main(["scene.json", "--denoise", "--denoise-mode", "variance", "--denoise-firefly", "-1"])
