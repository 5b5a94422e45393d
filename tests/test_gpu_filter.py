"""The bilinear texture filter on the GPU: the F_ENV kernels with either switch against the x86 build of the same
headers at every staging level and through the instance-BVH shape, the constant-texture identities, the closed forms of
tests/filter_ref.py, adaptive sampling, row shards, a 2^25-texel filtered environment, the CLI and the denoiser's backdrop."""
import json

import numpy as np
import pytest

import env_ref as E
import filter_ref as F
from conftest import make_holder
from micro_raytracer_amd._abi import F_ALL, F_BVH, F_COLD, F_DEEP, F_ENV, F_VATTR
from test_gpu_vattr import LEVELS

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def probe():
    return E.shared_probe()


def _env(sky="bilinear", tex="bilinear", mapping="latlong", res=(96, 54), sample=16, crowd=False, tex_res=(64, 32)):
    """scenes.env_scene (a textured smooth mesh, a chrome and a glass sphere under an HDR environment) with the two filters;
    crowd: + 30 small spheres, so that the scene gets an instance BVH."""
    from micro_raytracer_amd import scenes
    d = scenes.env_scene(res=res, sample=sample, bounce=8, mapping=mapping, tex_res=tex_res, filter=sky or "nearest")
    d["scene"]["sky"]["rot"] = 0.21
    if crowd:
        inst = [[[-0.9 + 0.06 * i, 0.2 + 0.05 * (i % 5), -0.45 + 0.03 * (i % 3)], [0, 0, -1, 0]] for i in range(30)]
        d["scene"]["renderer"].append({"type": "sphere", "r": 0.025, "inst": inst, "mat": {"albedo": "#c0a030", "rough": 0.3}})
    return F.with_filters(d, tex=tex)


def _gpu(render, spp, seed, **kw):
    from micro_raytracer_amd import Sampler
    s = Sampler(seed=seed, device=0, **kw)
    s.execute(render, n_samples=spp)
    return s


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def _check_aov(aov, ref):
    g, alb, rend = ref
    assert np.array_equal(aov["renderer"], rend)
    assert _same(aov["normal"], g[..., 0:3]) and _same(aov["depth"], g[..., 3]) and _same(aov["albedo"], alb)


# ---- 6. GPU == x86, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crowd", [False, True])
def test_gpu_equals_x86_at_every_staging_level(probe, monkeypatch, crowd):
    """env_scene with both filters on, 96 x 54, 8 bounces, 16 spp: the accumulator bits of every staging level and workgroup
    size equal those of the x86 build, and so do the AOVs (filtered albedo, filtered backdrop of the miss pixels)."""
    render, holder = make_holder(_env(crowd=crowd))
    assert holder.ext.tex_filter == 1 and holder.ext.env.contents.filter == 1
    spp = 16
    ref_aov = E.x86_aov(probe, holder)
    want = E.x86_render(probe, holder, 1, spp)
    plain = E.x86_render(probe, make_holder(_env(sky=None, tex=None, crowd=crowd))[1], 1, spp)
    assert not _same(want, plain)                                   # the filters are seen
    seen = set()
    for env, markers in LEVELS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s = _gpu(render, spp, 1)
        got, cnt = s.accum()
        st = s.stats()
        aov = s.aov()
        s.close()
        for k in env:
            monkeypatch.delenv(k)
        kf = st["kernel_features"]
        assert kf & F_ENV and kf & F_VATTR and (kf & F_ALL) == F_ALL and bool(kf & F_BVH) == crowd, (env, kf)
        assert (kf & (F_COLD | F_DEEP)) == markers and bool(st["scene_in_lds"]) == ("MRT_SCENE_IN_L2" not in env), (env, st)
        seen.add((kf, st["block_threads"], st["scene_in_lds"]))
        err = float(np.abs(got - want).max()) / spp
        print(f"crowd {crowd} {env}: features {kf}, {st['block_threads']} threads, L-inf {err:.2e}, bits equal: {_same(got, want)}")
        assert cnt == spp and _same(got, want), (env, err)
        _check_aov(aov, ref_aov)
    assert len(seen) == len(LEVELS), seen


@pytest.mark.parametrize("which", ["sky", "tex"])
def test_gpu_each_filter_alone_equals_x86(probe, which):
    """One switch at a time at the planned shape: the environment's filter alone, and the material textures' filter alone on
    the scene WITHOUT an environment (the F_ENV family on the constant sky: miss albedo 0)."""
    if which == "sky":
        desc = _env(sky="bilinear", tex=None)
    else:
        desc = _env(sky=None, tex="bilinear")
        desc["scene"]["sky"] = {"color": [0.5, 0.75, 1.0], "pwr": 0.5}
    render, holder = make_holder(desc)
    want = E.x86_render(probe, holder, 2, 16)
    s = _gpu(render, 16, 2)
    got, _ = s.accum()
    st, aov = s.stats(), s.aov()
    s.close()
    assert st["kernel_features"] & F_ENV
    print(f"{which} alone: L-inf {float(np.abs(got - want).max()) / 16:.2e}, bits equal: {_same(got, want)}")
    assert _same(got, want)
    ref = E.x86_aov(probe, holder)
    _check_aov(aov, ref)
    if which == "tex":
        miss = ref[0][..., 7] == 0
        assert miss.sum() > 200 and (aov["albedo"][miss] == 0).all()


# ---- 7. constant textures ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "minecraft", "smooth_mesh"])
def test_gpu_constant_environments_render_the_same_bytes_filtered(name):
    """An all-ones and an all-twos (sky.color halved) environment: filter = bilinear gives the accumulator bits of filter =
    nearest (the same kernel), and the mean of the render without an environment within 1e-4 (another kernel)."""
    from test_env_host import SKY3, _scenes3
    make = _scenes3()[name]

    def build(tex=None, color=SKY3, filt=None):
        d = make()
        d["rt"]["bounce"] = 8
        d["scene"]["sky"] = {"color": list(color), "pwr": 0.5}
        if tex is not None:
            F.with_filters(E.with_env(d, tex, "latlong", 0.37), sky=filt)
        return make_holder(d)[0]

    s = _gpu(build(), 8, 1)
    base = s.accum()[0]
    s.close()
    for label, tex, color in (("ones", E.const_env(1.0), SKY3), ("twos", E.const_env(2.0), tuple(c / 2 for c in SKY3))):
        out = {}
        for filt in ("nearest", "bilinear"):
            s = _gpu(build(tex, color, filt), 8, 1)
            out[filt] = s.accum()[0]
            assert s.stats()["kernel_features"] & F_ENV
            s.close()
        assert _same(out["bilinear"], out["nearest"]), (name, label)
        err = float(np.abs(out["bilinear"] - base).max()) / 8
        print(f"{name} {label}: against no environment L-inf {err:.2e}, bits equal: {_same(out['bilinear'], base)}")
        assert err <= 1e-4


@pytest.mark.parametrize("name", ["minecraft", "smooth_mesh"])
def test_gpu_one_texel_textures_render_the_unfiltered_scene(probe, name):
    """Every material texture 1 x 1 and tex_filter = bilinear: the F_ENV family with no environment at run time.  Accumulator and
    AOV bits equal the x86 build's, which equal the unfiltered scene's (test_filter_host); against the GPU's own plain kernel
    the mean is within 1e-4."""
    from test_env_host import _scenes3
    d0 = F.one_texel_textures(_scenes3()[name]())
    d1 = F.with_filters(F.one_texel_textures(_scenes3()[name]()), tex="bilinear")
    for d in (d0, d1):
        d["rt"]["bounce"] = 8
    (r0, h0), (r1, h1) = make_holder(d0), make_holder(d1)
    want = E.x86_render(probe, h1, 1, 8)
    assert _same(want, E.x86_render(probe, h0, 1, 8))
    s = _gpu(r1, 8, 1)
    got, _ = s.accum()
    st, aov = s.stats(), s.aov()
    den, raw = s.denoise(), s.denoise(passes=0)
    s.close()
    assert st["kernel_features"] & F_ENV and _same(got, want)
    ref = E.x86_aov(probe, h1)
    _check_aov(aov, ref)
    miss = ref[0][..., 7] == 0
    assert (aov["albedo"][miss] == 0).all()
    s = _gpu(r0, 8, 1)
    base, _ = s.accum()
    assert not s.stats()["kernel_features"] & F_ENV
    den0 = s.denoise()
    s.close()
    err = float(np.abs(got - base).max()) / 8
    print(f"{name}: against the plain kernel L-inf {err:.2e}, bits equal: {_same(got, base)}")
    assert err <= 1e-4
    # the denoiser of such a context is the one of a context without an environment: misses demodulated by 1
    counts = np.full(got.shape[:2], 8, np.uint32)
    assert _same(den, E.x86_filter(probe, got, counts, ref[0], ref[1], env=False)) and _same(raw, got * f32(0.125))
    if _same(got, base):
        assert _same(den, den0)


# ---- 8. closed forms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapping", E.MAPPINGS)
def test_gpu_mirror_sphere_under_a_filtered_environment(mapping):
    from test_filter_host import check_mirror

    def run(render, holder):
        s = _gpu(render, 4, 1)
        acc, cnt = s.accum()
        assert cnt == 4 and s.stats()["kernel_features"] & F_ENV
        s.close()
        return acc / f32(4)
    check_mirror(run, mapping, (256, 256), "GPU 256x256")


@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_gpu_textured_surface_under_a_point_light(kind):
    from test_filter_host import check_lit

    def run(render, holder):
        s = _gpu(render, 2, 1)
        acc, _ = s.accum()
        assert bool(s.stats()["kernel_features"] & F_ENV) == (render.scene.tex_filter == "bilinear")
        s.close()
        return acc / f32(2)
    check_lit(run, kind, (256, 256), "GPU 256x256")


# ---- 9. adaptive sampling, row shards ----------------------------------------------------------------------------------------------
def test_gpu_adaptive_with_both_filters():
    """§12 with both filters on: a tile that stopped at n has the accumulator bytes of an n-sample uniform render."""
    from micro_raytracer_amd import Sampler
    from test_gpu_adaptive import np_tile_errors
    render, _ = make_holder(_env(res=(96, 64), sample=96))
    s = Sampler(seed=3, device=0)
    s.execute_adaptive(render, float("inf"), min_samples=32, max_samples=96, step=16)
    et, _, _ = np_tile_errors(s.accum()[0], s.adapt_half(), 32, 0.0)
    s.close()
    thr = float(np.median(et[np.isfinite(et)]))
    s = Sampler(seed=3, device=0)
    info = s.execute_adaptive(render, thr, min_samples=32, max_samples=96, step=16)
    assert s.stats()["kernel_features"] & F_ENV
    A, _ = s.accum()
    counts = s.sample_counts()
    s.close()
    stops = sorted(set(np.unique(counts).tolist()))
    assert len(stops) >= 2 and info["launches"] > 0, stops
    for n in stops:
        u = _gpu(render, n, 3)
        U, _ = u.accum()
        u.close()
        m = counts == n
        assert np.array_equal(A[m].view(np.uint32), U[m].view(np.uint32)), n


def test_gpu_two_row_shards_assemble_to_the_frame():
    render, _ = make_holder(_env())
    s = _gpu(render, 16, 5)
    whole = s.accum()[0]
    s.close()
    parts = np.zeros_like(whole)
    for i in (0, 1):
        s = _gpu(render, 16, 5, shard_index=i, shard_count=2)
        part, rows = s.accum_local()
        parts[rows] = part
        s.close()
    assert _same(parts, whole)


# ---- 10. the texel limit -----------------------------------------------------------------------------------------------------------------
def test_gpu_filtered_environment_at_the_texel_limit(probe):
    """An 8192 x 4096 f32 environment (2^25 texels, 403 MB: the four texel addresses need 64 bits) with filter = bilinear, 1 spp
    on a 64 x 64 frame: accumulator bits equal to the x86 build."""
    from micro_raytracer_amd import scenes
    w, h = 8192, 4096
    rng = np.random.default_rng(12)
    dat = rng.random((w * h, 3), dtype=f32)
    dat *= f32(4.0)
    dat += f32(0.001)                    # not a k/255 lattice: the f32 layout
    d = E.with_env(scenes.cornell_box(res=(64, 64), sample=1), {"w": w, "h": h, "dat": dat}, "latlong", 0.4, color=(1.0, 0.9, 0.8))
    del d["scene"]["renderer"][0], d["scene"]["renderer"][2]      # the box opened at the back and the top: paths reach the sky
    render, holder = make_holder(F.with_filters(d, sky="bilinear"))
    info, _, blob = E.x86_pack(probe, holder)
    rec = blob[info["off_env"]:info["off_env"] + 8]
    assert rec[3] == 1 and rec[7] == 1 and (int(rec[2]) + w * h * 3) * 4 > 2 ** 28
    del blob
    want = E.x86_render(probe, holder, 1, 1)
    s = _gpu(render, 1, 1)
    got, cnt = s.accum()
    assert s.stats()["kernel_features"] & F_ENV
    s.close()
    print(f"8192 x 4096 filtered environment: L-inf {float(np.abs(got - want).max()):.2e}, bits equal: {_same(got, want)}")
    assert cnt == 1 and _same(got, want)
    holder.ext.env.contents.filter = 0
    assert not _same(want, E.x86_render(probe, holder, 1, 1))


# ---- 11. CLI -----------------------------------------------------------------------------------------------------------------------------
def test_gpu_cli_filter_flags(tmp_path):
    """python -m micro_raytracer_amd with --sky-filter bilinear --tex-filter bilinear, with and without --denoise: the image of
    the same description with both filters through the Sampler; each flag alone changes the image."""
    from PIL import Image
    from micro_raytracer_amd import __main__ as cli
    from micro_raytracer_amd import load_render
    from micro_raytracer_amd.scene import dump_render
    j = dump_render(load_render(_env(sky=None, tex=None)))
    (tmp_path / "env.json").write_text(json.dumps(j))

    def run(name, *flags):
        out = tmp_path / name
        cli.main([str(tmp_path / "env.json"), "-o", str(out), *flags])
        return np.asarray(Image.open(out))

    raw = run("raw.png")
    both = run("both.png", "--sky-filter", "bilinear", "--tex-filter", "bilinear")
    assert both.shape == (54, 96, 3) and not np.array_equal(both, raw)
    assert not np.array_equal(run("sky.png", "--sky-filter", "bilinear"), raw)
    assert not np.array_equal(run("tex.png", "--tex-filter", "bilinear"), raw)
    den = run("den.png", "--sky-filter", "bilinear", "--tex-filter", "bilinear", "--denoise")
    assert den.shape == both.shape and not np.array_equal(den, both)
    render, _ = make_holder(_env())
    s = _gpu(render, 16, 1)
    assert np.array_equal(s.img(), both) and np.array_equal(s.img_denoised(), den)
    s.close()


# ---- 12. the denoiser keeps a smooth filtered backdrop -----------------------------------------------------------------------------------------
def test_gpu_denoiser_keeps_the_filtered_backdrop(probe):
    """The mirror sphere under the smooth-gradient 61 x 31 HDR backdrop with filter = bilinear: the albedo AOV of a miss is the
    filtered E(d), and miss pixels after mrt_denoise equal the undenoised mean to rtol 1e-5, the bound of
    test_env_host.check_backdrop."""
    render, holder = make_holder(F.with_filters(E.closed_form_scene("latlong", res=(96, 64)), sky="bilinear"))
    s = _gpu(render, 4, 1)
    acc, _ = s.accum()
    aov = s.aov()
    den = s.denoise()
    s.close()
    g, alb, rend = E.x86_aov(probe, holder)
    _check_aov(aov, (g, alb, rend))
    counts = np.full(acc.shape[:2], 4, np.uint32)
    assert _same(den, E.x86_filter(probe, acc, counts, g, alb, env=True))
    miss = g[..., 7] == 0
    mean = (acc * f32(0.25)).astype(np.float64)
    assert miss.sum() > 1000 and _same(alb[miss], (acc * f32(0.25))[miss])
    rel = np.abs(den[miss] - mean[miss]) / mean[miss]
    print(f"filtered backdrop: miss pixels denoised / mean - 1 <= {rel.max():.2e}")
    assert rel.max() <= 1e-5
    # nearest on the same view has texel edges in the backdrop; the filtered one is another image
    r0, _ = make_holder(E.closed_form_scene("latlong", res=(96, 64)))
    s = _gpu(r0, 4, 1)
    assert not _same(s.accum()[0], acc)
    s.close()
