"""The variance-guided denoiser mode (MRT_DN_VARIANCE) on the GPU: mrt_denoise against the x86 build of
csrc/mrt_denoise_var.h (tests/emu/var_probe.cpp) bit for bit, the bytes the mode must not change, state and argument errors,
quality against the a-trous mode at 1920x1080, and a 3840x2160 frame with its filter time."""
import ctypes as C

import numpy as np
import pytest

import var_ref as V
from micro_raytracer_amd import Sampler, _abi, _lib, load_render, scenes
from test_denoise_host import shared_probe as shared_dn_probe
from test_denoise_host import tonemapped, x86_aov

pytestmark = pytest.mark.gpu
f32 = np.float32
INF = float("inf")


@pytest.fixture(scope="module")
def probe():
    return V.shared_probe()


@pytest.fixture(scope="module")
def dn_probe():
    return shared_dn_probe()


def uniform_with_half(render, seed, spp=32):
    """The bytes of the uniform spp-sample render, with a half buffer: threshold 0, min = max."""
    s = Sampler(seed=seed, device=0)
    s.execute_adaptive(render, threshold=0.0, min_samples=spp, max_samples=spp, step=16)
    return s


def x86_ref(probe, A, H, counts, g, alb, passes, sigma_var=None, sigma_normal=None, sigma_plane=None, firefly=None, env=False):
    """The x86 filter with the options as Sampler.denoise takes them (None: the default)."""
    o = _abi.denoise_opts(0, None, sigma_normal, sigma_plane)
    sv = V.inv_sq(_abi.DN_SIGMA_VAR if sigma_var is None else sigma_var)
    ff = _abi.DN_FIREFLY if firefly is None else firefly
    return V.x86_filter(probe, A, H, counts, g, alb, passes, sv, V.inv_sq(o.sigma_normal), V.inv_sq(o.sigma_plane), ff, env)


OPTION_SETS = [dict(), dict(sigma_var=1.5, sigma_normal=INF, sigma_plane=0.2)]


def check_all_passes(probe, s, g, alb, env=False, pass_list=range(7)):
    A, _ = s.accum()
    H = s.adapt_half()
    counts = s.sample_counts()
    for passes in pass_list:
        for opts in OPTION_SETS:
            for firefly in (None, INF):
                info = {}
                got = s.denoise(passes, mode="variance", firefly=firefly, info=info, **opts)
                ref = x86_ref(probe, A, H, counts, g, alb, passes, firefly=firefly, env=env, **opts)
                assert V.same_bits(got, ref) == 0, (passes, opts, firefly)
                assert info["mode"] == 1 and info["passes"] == passes
    return A, H, counts


@pytest.mark.parametrize("res", [(1, 1), (7, 5), (45, 37)])
def test_gpu_var_denoise_equals_x86(probe, dn_probe, res):
    """(1, 1): smaller than every tile and halo; (7, 5): partial edge blocks; (45, 37): 3x3 blocks whose 7x7 and 5x5 halos cross
    block borders and, at 6 passes, a step of 32 larger than a sub-image."""
    render = load_render(scenes.cornell_box(res=res, sample=32))
    s = uniform_with_half(render, 5)
    g, alb, _, _ = x86_aov(dn_probe, _abi.build_desc(render), *res)
    A, H, counts = check_all_passes(probe, s, g, alb)
    assert np.all(counts == 32)
    # the route's accumulator is the uniform render's, and the a-trous mode on it is untouched by the new words
    u = Sampler(seed=5, device=0)
    u.execute(render, n_samples=32)
    assert V.same_bits(u.accum()[0], A) == 0
    assert V.same_bits(u.denoise(), s.denoise(mode="atrous")) == 0
    u.close()
    s.close()


def test_gpu_var_denoise_textured_albedo(probe, dn_probe):
    res = (41, 29)
    render = load_render(scenes.minecraft_like(res=res, ssaa=1, sample=32))
    s = uniform_with_half(render, 6)
    g, alb, _, _ = x86_aov(dn_probe, _abi.build_desc(render), *res)
    assert len(np.unique(alb.reshape(-1, 3), axis=0)) > 50
    check_all_passes(probe, s, g, alb, pass_list=(1, 3, 5))
    s.close()


def test_gpu_var_denoise_env_backdrop(probe):
    """A context with an environment texture: miss pixels are demodulated by the backdrop the centre ray sees."""
    import env_ref as E
    from conftest import make_holder
    ep = E.shared_probe()
    render, holder = make_holder(scenes.env_scene(res=(43, 31), sample=32, bounce=8, tex_res=(64, 32)))
    s = uniform_with_half(render, 7)
    g, alb, _ = E.x86_aov(ep, holder)
    miss = g[..., 7] == 0
    assert miss.any() and (~miss).any() and (alb[miss] > 0).any()
    A, H, counts = check_all_passes(probe, s, g, alb, env=True, pass_list=(1, 3, 5))
    assert V.same_bits(s.denoise(3, mode="variance"), x86_ref(probe, A, H, counts, g, alb, 3, env=False)) > 0
    s.close()


def test_gpu_var_denoise_adaptive_mixed_counts(probe, dn_probe):
    render = load_render(scenes.cornell_box(res=(67, 45), sample=128))
    s = Sampler(seed=4, device=0)
    s.execute_adaptive(render, threshold=0.3, min_samples=32, max_samples=128, step=16)
    assert len(np.unique(s.sample_counts())) > 1
    g, alb, _, _ = x86_aov(dn_probe, _abi.build_desc(render), 67, 45)
    check_all_passes(probe, s, g, alb, pass_list=(0, 1, 3, 5))
    s.close()


def test_gpu_var_bytes_that_must_not_change():
    render = load_render(scenes.cornell_box(res=(64, 48), sample=32))
    s = uniform_with_half(render, 1)
    for passes in (0, 2, 5):
        assert V.same_bits(s.denoise(passes, mode="atrous"), s.denoise(passes)) == 0
    info = {}
    assert np.array_equal(s.img_denoised(mode="atrous", info=info), s.img_denoised())
    assert info["mode"] == 0
    assert np.array_equal(s.img_denoised(mode="variance", passes=0), s.img())
    assert not np.array_equal(s.img_denoised(mode="variance"), s.img())
    # the same call twice: the same bits
    assert V.same_bits(s.denoise(mode="variance"), s.denoise(mode="variance")) == 0
    s.close()
    # a uniform context: the a-trous mode with the option words spelled out
    u = Sampler(seed=1, device=0)
    u.execute(render, n_samples=4)
    assert V.same_bits(u.denoise(mode="atrous"), u.denoise()) == 0
    assert np.array_equal(u.img_denoised(passes=0, mode="atrous"), u.img())
    u.close()


def test_gpu_var_errors():
    render = load_render(scenes.cornell_box(res=(16, 16), sample=32))
    s = Sampler(seed=1, device=0)
    s.execute(render, n_samples=2)

    def refused(code, **kw):
        for fn in (s.denoise, s.img_denoised):
            with pytest.raises(_lib.MrtError) as e:
                fn(**kw)
            assert e.value.code == code, (kw, e.value)
        return str(e.value)

    msg = refused(_abi.MRT_ERR_STATE, mode="variance")                     # a uniform context has no half buffer
    assert "mrt_execute_adaptive" in msg and "threshold 0" in msg and "min_samples = max_samples" in msg
    refused(_abi.MRT_ERR_STATE, mode="variance", passes=0)
    s.reset()
    s.execute_adaptive(render, threshold=0.0, min_samples=32, max_samples=32, step=16)
    assert np.isfinite(s.denoise(mode="variance")).all()
    s.reset()
    refused(_abi.MRT_ERR_STATE, mode="variance")                           # after reset()
    s.execute_adaptive(render, threshold=0.0, min_samples=32, max_samples=32, step=16)
    A, cnt = s.accum()
    s.set_accum(A, cnt)
    refused(_abi.MRT_ERR_STATE, mode="variance")                           # after set_accum: H no longer belongs to A
    s.reset()
    s.execute_adaptive(render, threshold=0.0, min_samples=32, max_samples=32, step=16)
    for kw in [dict(sigma_var=float("nan")), dict(sigma_var=-1.0), dict(firefly=float("nan")), dict(firefly=-0.5)]:
        refused(_abi.MRT_ERR_ARG, mode="variance", **kw)
        refused(_abi.MRT_ERR_ARG, mode="atrous", **kw)
    refused(_abi.MRT_ERR_ARG, mode="atrous", sigma_var=4.5)
    refused(_abi.MRT_ERR_ARG, mode="atrous", firefly=1.0)
    refused(_abi.MRT_ERR_ARG, mode="variance", passes=9)
    o = _abi.denoise_opts()
    o.mode = 2                                                             # an unknown mode
    out = np.empty((16, 16, 3), f32)
    assert _lib.lib().mrt_denoise(s._ctx, C.byref(o), out.ctypes.data_as(C.POINTER(C.c_float)), None) == _abi.MRT_ERR_ARG
    out = s.denoise(mode="variance", passes=2)                             # the context still works
    assert out.shape == (16, 16, 3) and np.isfinite(out).all()
    assert np.isfinite(s.denoise(mode="variance", sigma_var=INF, firefly=INF)).all()
    s.close()


QUALITY = [("cornell", lambda: scenes.cornell_box(res=(1920, 1080), sample=32)),
           ("mesh", lambda: scenes.mesh_scene(res=(1920, 1080), sample=32)),
           ("minecraft", lambda: scenes.minecraft_like(res=(1920, 1080), ssaa=1, sample=32))]


@pytest.mark.parametrize("name,make", QUALITY, ids=[q[0] for q in QUALITY])
def test_gpu_var_quality_1080p(name, make):
    """32 spp against 1024 spp of another seed, as test_gpu_quality_1080p: the variance mode's tone-mapped RMSE is lower than the
    a-trous mode's on the same render, both at their defaults."""
    render = load_render(make())
    cam = render.frame.cam
    gt = Sampler(seed=1001, device=0)
    gt.execute(render, n_samples=1024)
    G, _ = gt.accum()
    gt.close()
    s = uniform_with_half(render, 7)
    A, _ = s.accum()
    ref = tonemapped(G / f32(1024), cam.gamma, cam.exp)
    err = lambda img: float(np.sqrt(np.mean((tonemapped(img, cam.gamma, cam.exp) - ref) ** 2)))
    raw, atrous, var = err(A / f32(32)), err(s.denoise()), err(s.denoise(mode="variance"))
    var3, atrous3, var_noff = err(s.denoise(3, mode="variance")), err(s.denoise(3)), err(s.denoise(mode="variance", firefly=INF))
    s.close()
    print(f"{name} 1080p 32 spp: raw {raw:.4f}; 5 passes: a-trous {atrous / raw:.3f} x raw, variance {var / raw:.3f} x raw "
          f"(firefly off {var_noff / raw:.3f}); 3 passes: a-trous {atrous3 / raw:.3f}, variance {var3 / raw:.3f}")
    assert var < atrous


def test_gpu_var_denoise_4k_row_bands_and_timing(probe, dn_probe):
    """A 3840x2160 frame, 5 passes: the x86 filter on three row bands with the margin the passes (2 * (2^5 - 1) rows, the 3x3
    variance prefilter reaches no further), the 7x7 variance window (3) and the 3x3 firefly clamp (1) need; the filter time
    against the a-trous mode's in the same test, each the faster of two calls (the first pays for loading its kernels)."""
    render = load_render(scenes.cornell_box(res=(1920, 1080), ssaa=2, sample=32))
    s = uniform_with_half(render, 2)
    A, _ = s.accum()
    H = s.adapt_half()
    nh, nw = A.shape[:2]
    assert (nw, nh) == (3840, 2160)
    passes = 5
    ms = {}
    for mode in ("atrous", "variance", "atrous", "variance"):
        info = {}
        out = s.denoise(passes, mode=mode, info=info)
        ms[mode] = min(ms.get(mode, INF), info["filter_ms"])
        if mode == "variance":
            got = out
    print(f"4K, 5 passes: a-trous {ms['atrous']:.3f} ms, variance {ms['variance']:.3f} ms ({ms['variance'] / ms['atrous']:.2f} x)")
    assert 0 < ms["variance"] <= 3 * ms["atrous"], ms
    s.close()
    g, alb, _, _ = x86_aov(dn_probe, _abi.build_desc(render), nw, nh)
    m = 2 * (2 ** passes - 1) + 3 + 1
    for y0, y1 in [(0, 24), (1000, 1024), (2136, 2160)]:
        b0, b1 = max(0, y0 - m), min(nh, y1 + m)
        counts = np.full((b1 - b0, nw), 32, np.uint32)
        ref = x86_ref(probe, A[b0:b1], H[b0:b1], counts, g[b0:b1], alb[b0:b1], passes)
        assert V.same_bits(got[y0:y1], ref[y0 - b0:y1 - b0]) == 0, (y0, y1)
