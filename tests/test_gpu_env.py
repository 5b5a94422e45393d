"""The environment texture of the sky on the GPU: the F_ENV kernels against the x86 build of the same headers
(tests/emu/env_probe.cpp) at every staging level and through the instance-BVH shape, the all-ones identity, the closed-form
render of tests/env_ref.py, adaptive sampling, the denoiser's backdrop rule, row shards, and a 2^25-texel environment."""
import numpy as np
import pytest

import env_ref as E
from conftest import make_holder
from micro_raytracer_amd._abi import F_ALL, F_BVH, F_COLD, F_DEEP, F_ENV, F_VATTR
from test_gpu_vattr import LEVELS

pytestmark = pytest.mark.gpu
f32 = np.float32
TOL = 1e-4      # the project's bar: per-channel L-inf on the mean radiance


@pytest.fixture(scope="module")
def probe():
    return E.shared_probe()


def _env(mapping, res=(96, 54), sample=16, crowd=False, tex_res=(64, 32)):
    """scenes.env_scene; crowd: + 30 small spheres, so that the scene gets an instance BVH."""
    from micro_raytracer_amd import scenes
    d = scenes.env_scene(res=res, sample=sample, bounce=8, mapping=mapping, tex_res=tex_res)
    d["scene"]["sky"]["rot"] = 0.21
    if crowd:
        inst = [[[-0.9 + 0.06 * i, 0.2 + 0.05 * (i % 5), -0.45 + 0.03 * (i % 3)], [0, 0, -1, 0]] for i in range(30)]
        d["scene"]["renderer"].append({"type": "sphere", "r": 0.025, "inst": inst, "mat": {"albedo": "#c0a030", "rough": 0.3}})
    return d


def _img_holder(desc):
    """The same frame and camera for emu.img (tone map and resize), whose packer call knows neither attributes nor environments."""
    from micro_raytracer_amd import _abi
    flat, _ = make_holder(desc)
    for r in flat.scene.renderer:
        r.mat.tex = None
    flat.scene.sky.tex = None
    return _abi.build_desc(flat)


def _gpu(render, spp, seed, **kw):
    from micro_raytracer_amd import Sampler
    s = Sampler(seed=seed, device=0, **kw)
    s.execute(render, n_samples=spp)
    return s


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


@pytest.mark.parametrize("crowd", [False, True])
@pytest.mark.parametrize("mapping", E.MAPPINGS)
def test_gpu_equals_x86_at_every_staging_level(probe, monkeypatch, mapping, crowd):
    """env_scene at 96 x 54, 8 bounces, 16 spp, seeds 1 and 2: the mean radiance of every staging level and workgroup size within
    1e-4 of the x86 build, the accumulator bits of all levels identical, mrt_img / mrt_img_ss bytes equal to the x86 tone map,
    and mrt_aov bits equal to the x86 AOV pass, the albedo of miss pixels -- the backdrop -- included."""
    from emu import emu
    render, holder = make_holder(_env(mapping, crowd=crowd))
    holder_img = _img_holder(_env(mapping, crowd=crowd))
    spp = 16
    ref_aov = E.x86_aov(probe, holder)
    miss = ref_aov[0][..., 7] == 0
    assert miss.sum() > 200 and (ref_aov[1][miss] > 0).all()
    for seed in (1, 2):
        want = E.x86_render(probe, holder, seed, spp)
        ss_want, img_want = emu.img(holder_img, want, spp)
        seen = set()
        first = None
        for env, markers in LEVELS:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            s = _gpu(render, spp, seed)
            got, cnt = s.accum()
            st = s.stats()
            img, ss = s.img(), s.img_ss()
            aov = s.aov() if seed == 1 else None
            s.close()
            for k in env:
                monkeypatch.delenv(k)
            kf = st["kernel_features"]
            assert kf & F_ENV and kf & F_VATTR and (kf & F_ALL) == F_ALL and bool(kf & F_BVH) == crowd, (env, kf)
            assert (kf & (F_COLD | F_DEEP)) == markers and bool(st["scene_in_lds"]) == ("MRT_SCENE_IN_L2" not in env), (env, st)
            if "MRT_BLOCK_THREADS" in env:
                assert st["block_threads"] == int(env["MRT_BLOCK_THREADS"]), (env, st)
            seen.add((kf, st["block_threads"], st["scene_in_lds"]))
            err = float(np.abs(got - want).max()) / spp
            print(f"{mapping} crowd {crowd} seed {seed} {env}: features {kf}, {st['block_threads']} threads, L-inf {err:.2e}")
            assert cnt == spp and err <= TOL, (env, err)
            if first is None:
                first = got
            assert _same(first, got), env
            if _same(got, want):
                assert np.array_equal(ss, ss_want) and np.array_equal(img, img_want), env
            else:               # the tone map of the device's own sums, through the x86 build of mrt_post.h
                ss2, img2 = emu.img(holder_img, got, spp)
                assert np.array_equal(ss, ss2) and np.array_equal(img, img2), env
            if aov is not None:
                g, alb, rend = ref_aov
                assert np.array_equal(aov["renderer"], rend), env
                assert _same(aov["normal"], g[..., 0:3]) and _same(aov["depth"], g[..., 3]) and _same(aov["albedo"], alb), env
        assert len(seen) == len(LEVELS), seen


@pytest.mark.parametrize("name", ["cornell", "minecraft", "smooth_mesh"])
def test_gpu_ones_and_twos_render_the_constant_sky(name):
    """test_env_host.test_ones_and_twos_render_the_constant_sky_bit_for_bit on the GPU: the mean within 1e-4 of the render without an environment (which runs another instantiation, so the
    bits are reported, not asserted)."""
    from test_env_host import SKY3, _scenes3
    make = _scenes3()[name]

    def build(tex=None, mapping="sphere", rot=0.0, color=SKY3):
        d = make()
        d["rt"]["bounce"] = 8
        d["scene"]["sky"] = {"color": list(color), "pwr": 0.5}
        if tex is not None:
            E.with_env(d, tex, mapping, rot)
        return make_holder(d)[0]

    half = tuple(c / 2 for c in SKY3)
    for seed in (1, 2):
        s = _gpu(build(), 8, seed)
        base = s.accum()[0]
        assert not s.stats()["kernel_features"] & F_ENV
        s.close()
        for mapping in E.MAPPINGS:
            for rot in (0.0, 0.37):
                for label, r in (("ones", build(E.const_env(1.0), mapping, rot)), ("twos", build(E.const_env(2.0), mapping, rot, half))):
                    s = _gpu(r, 8, seed)
                    got = s.accum()[0]
                    assert s.stats()["kernel_features"] & F_ENV
                    s.close()
                    err = float(np.abs(got - base).max()) / 8
                    print(f"{name} seed {seed} {mapping} rot {rot} {label}: L-inf {err:.2e}, bits equal: {_same(got, base)}")
                    assert err <= TOL, (name, seed, mapping, rot, label, err)


@pytest.mark.parametrize("mapping", E.MAPPINGS)
def test_gpu_mirror_sphere_equals_the_closed_form(mapping):
    """The closed form of tests/env_ref.py (Checks) at 256 x 256."""
    render, _ = make_holder(E.closed_form_scene(mapping, res=(256, 256)))
    first = None
    for seed in (1, 2):
        s = _gpu(render, 4, seed)
        acc, cnt = s.accum()
        assert cnt == 4 and s.stats()["kernel_features"] & F_ENV
        s.close()
        if first is None:
            E.check_closed_form(acc / f32(4), render, "GPU 256x256")
            first = acc
        else:
            assert _same(acc, first)          # aprt 0, a mirror, no coin open: no draw reaches the image


def test_gpu_adaptive_on_the_environment_scene():
    """§12 on a scene with an environment: a tile that stopped at n has the accumulator bytes of an n-sample uniform render."""
    from micro_raytracer_amd import Sampler
    from test_gpu_adaptive import np_tile_errors
    render, _ = make_holder(_env("latlong", res=(96, 64), sample=96))
    s = Sampler(seed=3, device=0)
    s.execute_adaptive(render, float("inf"), min_samples=32, max_samples=96, step=16)
    et, nan, _ = np_tile_errors(s.accum()[0], s.adapt_half(), 32, 0.0)
    s.close()
    thr = float(np.median(et[np.isfinite(et)]))
    s = Sampler(seed=3, device=0)
    info = s.execute_adaptive(render, thr, min_samples=32, max_samples=96, step=16)
    assert s.stats()["kernel_features"] & F_ENV
    A, _ = s.accum()
    counts = s.sample_counts()
    stops = sorted(set(np.unique(counts).tolist()))
    assert len(stops) >= 2 and info["launches"] > 0, stops
    for n in stops:
        u = _gpu(render, n, 3)
        U, _ = u.accum()
        m = counts == n
        assert np.array_equal(A[m].view(np.uint32), U[m].view(np.uint32)), n
        u.close()
    assert np.array_equal(s.img_denoised(passes=0), s.img())
    s.close()


def test_gpu_denoiser_keeps_the_backdrop(probe):
    """The backdrop rule of DESIGN.md §15 on the device: mrt_denoise of the checker-environment scene, bits equal to the x86 build of the same filter on
    the device's sums, and the backdrop check of tests/test_env_host.py on the device's output."""
    from test_env_host import check_backdrop, denoise_scene
    render, holder = make_holder(denoise_scene())
    s = _gpu(render, 4, 1)
    acc, cnt = s.accum()
    aov = s.aov()
    den = s.denoise()
    raw0 = s.denoise(passes=0)
    s.close()
    g, alb, rend = E.x86_aov(probe, holder)
    assert _same(aov["albedo"], alb) and _same(aov["depth"], g[..., 3]) and np.array_equal(aov["renderer"], rend)
    counts = np.full(acc.shape[:2], 4, np.uint32)
    assert _same(den, E.x86_filter(probe, acc, counts, g, alb, env=True))
    assert _same(raw0, acc * f32(0.25))
    forced = E.x86_filter(probe, acc, counts, g, alb, env=False)
    assert not _same(den, forced)
    check_backdrop(acc, g, alb, den, forced, "GPU")


def test_gpu_two_row_shards_assemble_to_the_frame():
    render, _ = make_holder(_env("sphere", res=(96, 54), sample=16))
    s = _gpu(render, 16, 5)
    whole = s.accum()[0]
    s.close()
    parts = np.zeros_like(whole)
    for i in (0, 1):
        s = _gpu(render, 16, 5, shard_index=i, shard_count=2)
        assert s.stats()["kernel_features"] & F_ENV
        part, rows = s.accum_local()
        parts[rows] = part
        s.close()
    assert _same(parts, whole)


def test_gpu_environment_at_the_texel_limit(probe):
    """An 8192 x 4096 f32 environment -- 2^25 texels, 403 MB, texel byte offsets beyond 2^28 -- creates, renders 1 spp at
    256 x 256 and matches the x86 build within 1e-4; one texel more is MRT_ERR_LIMIT."""
    from micro_raytracer_amd import MrtError, Sampler, _abi, scenes
    w, h = 8192, 4096
    rng = np.random.default_rng(12)
    dat = rng.random((w * h, 3), dtype=f32)
    dat *= f32(4.0)
    dat += f32(0.001)                    # not a k/255 lattice: the f32 layout
    d = E.with_env(scenes.cornell_box(res=(256, 256), sample=1), {"w": w, "h": h, "dat": dat}, "latlong", 0.4, color=(1.0, 0.9, 0.8))
    del d["scene"]["renderer"][0], d["scene"]["renderer"][2]      # the box opened at the back and the top: paths reach the sky
    render, holder = make_holder(d)
    info, _, blob = E.x86_pack(probe, holder)
    rec = blob[info["off_env"]:info["off_env"] + 8]
    assert rec[3] == 1 and (int(rec[2]) + w * h * 3) * 4 > 2 ** 28
    del blob
    want = E.x86_render(probe, holder, 1, 1)
    s = _gpu(render, 1, 1)
    got, cnt = s.accum()
    assert s.stats()["kernel_features"] & F_ENV
    s.close()
    err = float(np.abs(got - want).max())
    print(f"8192 x 4096 environment: L-inf {err:.2e}, bits equal: {_same(got, want)}")
    assert cnt == 1 and err <= TOL
    holder.ext.env.contents.tex.h = h + 1
    from micro_raytracer_amd import _lib
    with pytest.raises(MrtError) as e:
        _lib.plan_launch(holder)
    assert e.value.code == _abi.MRT_ERR_LIMIT


def test_gpu_cli_renders_a_description_that_names_an_hdr(tmp_path, capsys):
    """python -m micro_raytracer_amd on scenes.env_scene written as a JSON file whose sky names a Radiance .hdr: with and without
    --denoise, and with --sky-map / --sky-rot / --sky-tex overriding the file."""
    import json
    from micro_raytracer_amd import __main__ as cli
    from micro_raytracer_amd import load_render, scenes
    from micro_raytracer_amd.scene import dump_render
    d = scenes.env_scene(res=(96, 54), sample=16, mapping="latlong", tex_res=(64, 32))
    px = np.zeros((32, 64, 4), np.uint8)                         # the sky as RGBE: shared exponent of the largest channel
    rgb = d["scene"]["sky"]["tex"]["dat"].reshape(32, 64, 3).astype(np.float64)
    m, e = np.frexp(rgb.max(-1))
    px[..., :3] = (rgb * (256.0 / np.ldexp(1.0, e))[..., None]).astype(np.uint8)
    px[..., 3] = e + 128
    E.write_hdr(tmp_path / "sky.hdr", px, rle=True)
    E.write_hdr(tmp_path / "other.hdr", px[::-1].copy(), rle=False)
    j = dump_render(load_render(d))
    j["scene"]["sky"]["tex"] = "sky.hdr"
    (tmp_path / "env.json").write_text(json.dumps(j))

    def run(name, *flags):
        out = tmp_path / name
        cli.main([str(tmp_path / "env.json"), "-o", str(out), *flags])
        from PIL import Image
        return np.asarray(Image.open(out))

    raw = run("raw.png")
    assert raw.shape == (54, 96, 3) and raw.std() > 10
    den = run("den.png", "--denoise")
    assert den.shape == raw.shape and not np.array_equal(den, raw)
    assert not np.array_equal(run("rot.png", "--sky-rot", "0.25"), raw)
    assert not np.array_equal(run("map.png", "--sky-map", "sphere"), raw)
    assert not np.array_equal(run("tex.png", "--sky-tex", str(tmp_path / "other.hdr")), raw)
    # the render is the library's: the same description through the Sampler gives the same bytes
    render = load_render(str(tmp_path / "env.json"))
    s = _gpu(render, 16, 1)
    assert np.array_equal(s.img(), raw)
    s.close()
