"""Per-corner normals and UVs of triangles and meshes on the GPU: the F_VATTR kernels against the x86 build of
the same headers (tests/emu/vattr_probe.cpp) at every staging level and through the instance-BVH shape, the closed-form render
of tests/vattr_ref.py, adaptive sampling and the denoiser on a smooth textured mesh."""
import numpy as np
import pytest

import vattr_ref as V
from conftest import make_holder
from micro_raytracer_amd._abi import F_ALL, F_BVH, F_COLD, F_DEEP, F_VATTR

pytestmark = pytest.mark.gpu
f32 = np.float32
TOL = 1e-4      # the project's bar: per-channel L-inf on the mean radiance


@pytest.fixture(scope="module")
def probe():
    return V.shared_probe()


def _smooth(res=(96, 54), sample=16, n_tris=600, crowd=False):
    """The smooth textured mesh scene; crowd: + 30 small spheres, so that the scene gets an instance BVH."""
    from micro_raytracer_amd import scenes
    d = scenes.smooth_mesh_scene(res=res, sample=sample, bounce=8, n_tris=n_tris)
    if crowd:
        inst = [[[-0.9 + 0.06 * i, 0.2 + 0.05 * (i % 5), -0.45 + 0.03 * (i % 3)], [0, 0, -1, 0]] for i in range(30)]
        d["scene"]["renderer"].append({"type": "sphere", "r": 0.025, "inst": inst, "mat": {"albedo": "#c0a030", "rough": 0.3}})
    return d


def _gpu(render, spp, seed):
    from micro_raytracer_amd import Sampler
    s = Sampler(seed=seed, device=0)
    s.execute(render, n_samples=spp)
    return s


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


LEVELS = [({"MRT_COLD": "0", "MRT_BLOCK_THREADS": t}, 0) for t in ("64", "256", "512", "1024")] + \
         [({"MRT_COLD": "1", "MRT_BLOCK_THREADS": t}, F_COLD) for t in ("256", "512", "1024")] + \
         [({"MRT_DEEP_NODES": n, "MRT_BLOCK_THREADS": t}, F_COLD | F_DEEP) for n, t in (("3", "256"), ("40", "512"), ("100000", "1024"))] + \
         [({"MRT_SCENE_IN_L2": "1"}, 0)]


@pytest.mark.parametrize("crowd", [False, True])
def test_gpu_equals_x86_at_every_staging_level(probe, monkeypatch, crowd):
    """8 bounces, 16 spp, seeds 1 and 2: the mean radiance of every staging level and workgroup size within 1e-4 of the x86
    build of the same headers, the accumulator bits of all levels identical, mrt_img bytes identical to the tone map of the
    x86 accumulator; the same for mrt_aov."""
    from emu import emu
    from micro_raytracer_amd import _abi
    render, holder = make_holder(_smooth(crowd=crowd))
    flat, _ = make_holder(_smooth(crowd=crowd))
    flat.scene.renderer[0].mat.tex = None                   # same frame and camera for emu.img (the tone map and the resize), whose
    holder_img = _abi.build_desc(flat)                      # packer call knows no attributes and would refuse the mesh's texture
    spp = 16
    ref_aov = V.x86_aov(probe, holder)
    for seed in (1, 2):
        want = V.x86_render(probe, holder, seed, spp)
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
            assert kf & F_VATTR and (kf & F_ALL) == F_ALL and bool(kf & F_BVH) == crowd, (env, kf)
            assert (kf & (F_COLD | F_DEEP)) == markers and bool(st["scene_in_lds"]) == ("MRT_SCENE_IN_L2" not in env), (env, st)
            if "MRT_BLOCK_THREADS" in env:
                assert st["block_threads"] == int(env["MRT_BLOCK_THREADS"]), (env, st)
            seen.add((kf, st["block_threads"], st["scene_in_lds"]))
            err = float(np.abs(got - want).max()) / spp
            print(f"crowd {crowd} seed {seed} {env}: features {kf}, {st['block_threads']} threads, L-inf {err:.2e}")
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
    # the attributes are seen: the same scene without them renders something else
    from micro_raytracer_amd import scenes
    plain, _ = make_holder(scenes.mesh_scene(res=(96, 54), sample=16, n_tris=600))
    if not crowd:
        s = _gpu(plain, spp, 2)
        assert not s.stats()["kernel_features"] & F_VATTR and not _same(s.accum()[0], first)
        s.close()


def test_gpu_bounce0_render_equals_the_closed_form():
    """Item 9: the closed form of tests/vattr_ref.py (float64 numpy, brute-force triangle tests) at 256 x 256, on the close view
    of the scene (test_vattr_host.closed_form_scene says why)."""
    from test_vattr_host import check_closed_form, closed_form_scene
    render, _ = make_holder(closed_form_scene(res=(256, 256), close=True))
    for seed in (1, 2):
        s = _gpu(render, 4, seed)
        acc, cnt = s.accum()
        assert s.stats()["kernel_features"] & F_VATTR
        s.close()
        if seed == 1:
            check_closed_form(acc / f32(4), render, "GPU 256x256")
            first = acc
        else:
            assert _same(acc, first)          # bounce 0, aprt 0: no draw reaches the image


def test_gpu_aov_on_the_analytic_sphere_and_the_labelled_mesh():
    from micro_raytracer_amd import Sampler, scenes
    from test_vattr_host import analytic_sphere_scene, check_analytic_aov, check_labelled_aov, labelled_scene

    def gpu_aov(render):
        s = Sampler(seed=1, device=0)
        s.execute(render, n_samples=1)
        a = s.aov()
        s.close()
        g = np.zeros(a["depth"].shape + (8,), f32)
        g[..., 0:3], g[..., 3] = a["normal"], a["depth"]
        return g, a["albedo"], a["renderer"]

    render, _ = make_holder(analytic_sphere_scene())
    check_analytic_aov(*gpu_aov(render), render)
    render, _ = make_holder(labelled_scene(scenes.bumpy_mesh(967)))
    check_labelled_aov(*gpu_aov(render), render, "GPU bumpy967")


def test_gpu_adaptive_and_denoise_on_the_smooth_mesh():
    """§12 on a scene with attributes: a tile's accumulator bytes are the uniform render's at its count; passes = 0 of the
    denoiser gives the bytes of mrt_img; the filter runs on the shading-normal / textured-albedo AOVs."""
    from micro_raytracer_amd import Sampler
    render, _ = make_holder(_smooth(res=(96, 64), sample=96))
    s = Sampler(seed=3, device=0)
    probe_run = s.execute_adaptive(render, float("inf"), min_samples=32, max_samples=96, step=16)
    assert probe_run["max_count"] == 32
    s.close()
    # a threshold between the tiles' errors: take the list launches through at least two stop counts
    from test_gpu_adaptive import np_tile_errors
    s = Sampler(seed=3, device=0)
    s.execute_adaptive(render, float("inf"), min_samples=32, max_samples=96, step=16)
    et, nan, _ = np_tile_errors(s.accum()[0], s.adapt_half(), 32, 0.0)
    s.close()
    thr = float(np.median(et[np.isfinite(et)]))
    s = Sampler(seed=3, device=0)
    info = s.execute_adaptive(render, thr, min_samples=32, max_samples=96, step=16)
    assert s.stats()["kernel_features"] & F_VATTR
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
    u = _gpu(render, 32, 3)
    assert np.array_equal(u.img_denoised(passes=0), u.img())
    raw, den = u.img(), u.img_denoised(passes=3)
    assert den.shape == raw.shape and not np.array_equal(den, raw)
    u.close()


def test_gpu_textured_mesh_without_uvs_is_still_rejected():
    from micro_raytracer_amd import MrtError, Sampler, _abi
    render, _ = make_holder(_smooth(res=(32, 32)))
    render.scene.renderer[0].uv = None
    with pytest.raises(MrtError) as e:
        Sampler(seed=1, device=0).execute(render, n_samples=1)
    assert e.value.code == _abi.MRT_ERR_SCENE
