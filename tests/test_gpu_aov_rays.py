"""mrt_aov_rays on the GPU: first-hit AOVs on caller-supplied rays and the a-trous filter on a grid periodic in x.

7.  the context's own camera rays fed back give the planes, and the denoised bytes, of a fresh context;
8.  equirect grids against the x86 build of aov_ray (tests/emu/aov_rays_probe.cpp) and the oracle's orc_ray_query, the albedo of
    a miss under an environment against mrt_radiance's one-sample answer;
9.  torch tensors on the device against host arrays;
10. the wrapped filter: a roll of the columns commutes with it, it equals the x86 chain, and far from the seam it equals the
    unwrapped filter;
11. what the call leaves alone, what it refuses;
12. quality of a denoised panorama, whole frame and seam (figures in DESIGN.md §20);
13. the CLI's --pano-guides."""
import json
import os

import numpy as np
import pytest

import test_aov_rays_host as H
from conftest import make_holder
from micro_raytracer_amd import Sampler, _abi, _lib, cameras, load_render, scenes
from test_denoise_host import inv_sq, same_bits, tonemapped

pytestmark = pytest.mark.gpu
f32 = np.float32
PLANES = ("depth", "normal", "albedo", "renderer", "instance")


@pytest.fixture(scope="module")
def probe():
    return H.shared_probe()


def default_sigmas():
    o = _abi.denoise_opts(0)
    return inv_sq(o.sigma_color), inv_sq(o.sigma_normal), inv_sq(o.sigma_plane)


def planes_differ(a, b):
    """Mismatching words per plane of two Sampler.aov() dicts (or plane dicts of the probe): all zeros when they agree."""
    return {k: (same_bits(a[k], b[k]) if a[k].dtype == f32 else int(np.count_nonzero(a[k] != b[k]))) for k in PLANES}


def assert_same_planes(a, b, label=""):
    d = planes_differ(a, b)
    assert not any(d.values()), (label, d)


# ---- 7: the camera's own rays -----------------------------------------------------------------------------------------------------
CONTEXTS = {
    "lds": ({}, lambda: scenes.cornell_box(res=(96, 64), sample=16), "all"),
    "l2": ({"MRT_SCENE_IN_L2": "1"}, lambda: scenes.cornell_box(res=(96, 64), sample=16), "none"),
    "deep_mesh": ({"MRT_DEEP_NODES": "64"}, lambda: scenes.mesh_scene(res=(53, 31), sample=16), "deep"),
}


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_camera_rays_fed_back_give_a_fresh_contexts_planes_and_denoised_bytes(monkeypatch, name):
    env, make, staging = CONTEXTS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    render = load_render(make())
    assert _lib.plan_launch(render)["staging"] == staging
    fresh = Sampler(seed=5, device=0)
    fresh.execute(render, n_samples=16)
    want, want_dn = fresh.aov(), fresh.denoise(passes=5)
    fresh.close()
    s = Sampler(seed=5, device=0).create(render)
    o, d = s.camera_rays(render)
    s.aov_rays(render, o, d)
    assert_same_planes(s.aov(), want, name)
    assert (want["renderer"] >= 0).any()
    s.execute(render, n_samples=16)
    assert same_bits(s.denoise(passes=5), want_dn) == 0
    s.close()


# ---- 8: equirect grids ---------------------------------------------------------------------------------------------------------
EQUIRECT = {
    "cornell": lambda: scenes.cornell_box(res=(96, 40), sample=4),
    "env_nearest": lambda: scenes.env_scene(res=(96, 40), sample=4, tex_res=(64, 32)),
    "env_bilinear": lambda: scenes.env_scene(res=(96, 40), sample=4, mapping="latlong", tex_res=(64, 32), filter="bilinear"),
}


@pytest.mark.parametrize("name", list(EQUIRECT))
def test_equirect_planes_equal_x86_and_the_oracle(probe, oracle_mod, name):
    render, holder = make_holder(EQUIRECT[name]())
    s = Sampler(seed=2, device=0).create(render)
    assert (s.nw, s.nh) == (96, 40)
    o, d = cameras.equirect(render.frame.cam.pos, s.nw, s.nh)
    s.aov_rays(render, o, d, wrap_x=True)
    got = s.aov()
    ref = H.x86_aov_rays(probe, holder, o, d)
    assert_same_planes(got, ref, name)
    flat = {k: np.ascontiguousarray(v).reshape((-1,) + v.shape[2:]) for k, v in ref.items()}
    orc = oracle_mod.Oracle(holder, seed=1)
    words = orc.ray_query(o.reshape(-1, 3), d.reshape(-1, 3))
    orc.close()
    hit = H.against_ray_query(name, flat, words, o.reshape(-1, 3), d.reshape(-1, 3)).reshape(s.nh, s.nw)
    assert np.array_equal(got["renderer"] >= 0, hit)
    if name == "cornell":
        assert hit.all()
    else:
        # a primary miss contributes the raw E(d): the one-sample answer of mrt_radiance on the same ray
        miss = ~hit
        assert miss.sum() > 100
        rad = s.radiance(render, o, d, 1)
        assert same_bits(got["albedo"][miss], rad[miss]) == 0
        assert np.all(got["albedo"][miss].max(axis=-1) > 0)
        # ... and the wrapped filter of a context with an environment (miss pixels demodulated by their backdrop) is the x86 chain
        s.set_accum(rad, 1)
        counts = np.ones(rad.shape[:2], np.uint32)
        for passes in (1, 5):
            want = H.x86_filter(probe, rad, counts, ref["guide"], ref["albedo"], passes, *default_sigmas(), True, env=True)
            assert same_bits(s.denoise(passes=passes), want) == 0, (name, passes)
    s.close()


# ---- 9: device tensors -----------------------------------------------------------------------------------------------------------
_DEVICE_SCRIPT = r"""
import sys
import numpy as np
import torch
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)                      # torch brings the HIP runtime up first, as in bench.py and dist.ShardedSampler
sys.path[:0] = sys.argv[1:3]
from micro_raytracer_amd import Sampler, cameras, load_render, scenes
from test_denoise_host import same_bits
render = load_render(scenes.env_scene(res=(50, 37), sample=4, tex_res=(64, 32)))
s = Sampler(seed=2, device=0).create(render)
o, d = cameras.equirect(render.frame.cam.pos, s.nw, s.nh, yaw=0.1)
s.aov_rays(render, o, d)
host = s.aov()
assert (host["renderer"] >= 0).any() and (host["renderer"] < 0).any()
s.aov_rays(render, None, None)
to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
s.aov_rays(render, to, td, wrap_x=True)
got = s.aov()
for k, v in host.items():
    assert (same_bits(got[k], v) if v.dtype == np.float32 else np.count_nonzero(got[k] != v)) == 0, k
assert np.array_equal(to.cpu().numpy(), o) and np.array_equal(td.cpu().numpy(), d)       # borrowed, not written
for bad in ((to, d), (o[:-1], d[:-1]), (to[:-1], td[:-1]), (o, None)):
    try:
        s.aov_rays(render, *bad)
    except ValueError:
        pass
    else:
        raise AssertionError("mixed or mis-shaped rays were accepted")
s.close()
print("DEVICE-OK")
"""


def test_torch_device_tensors_give_the_planes_of_host_arrays():
    """Torch tensors on the context's device (MRT_AOV_RAYS_DEVICE) against the host path.  In a child process, as the device test
    of tests/test_gpu_rays.py: torch has to bring the HIP runtime up before the library does."""
    import subprocess
    import sys
    pytest.importorskip("torch")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _DEVICE_SCRIPT, os.path.dirname(here), here], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and "DEVICE-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- 10: the wrapped filter --------------------------------------------------------------------------------------------------------
def _pano(res, seed=4, spp=16):
    render, holder = make_holder(scenes.cornell_box(res=res, sample=spp))
    s = Sampler(seed=seed, device=0).create(render)
    o, d = cameras.equirect(render.frame.cam.pos, s.nw, s.nh)
    rgb = s.radiance(render, o, d, spp)
    return render, holder, s, o, d, rgb


@pytest.mark.parametrize("res", [(80, 24), (24, 8)])
def test_wrapped_denoise_commutes_with_a_roll_and_equals_x86(probe, res):
    spp, k = 16, 7
    render, holder, s, o, d, rgb = _pano(res, spp=spp)
    s.set_accum(rgb, spp)
    s.aov_rays(render, o, d, wrap_x=True)
    out = s.denoise(passes=5)
    ro, rd, rrgb = (np.ascontiguousarray(np.roll(a, k, axis=1)) for a in (o, d, rgb))
    s.set_accum(rrgb, spp)
    s.aov_rays(render, ro, rd, wrap_x=True)
    rolled = s.denoise(passes=5)
    assert same_bits(rolled, np.roll(out, k, axis=1)) == 0
    counts = np.full(rgb.shape[:2], spp, np.uint32)
    for rays, sums, got in ((( o, d), rgb, out), ((ro, rd), rrgb, rolled)):
        ref = H.x86_aov_rays(probe, holder, *rays)
        want = H.x86_filter(probe, sums, counts, ref["guide"], ref["albedo"], 5, *default_sigmas(), True)
        assert same_bits(got, want) == 0
    # the flag acts: the unwrapped filter on the same planes gives other bytes at the seam, and the x86 chain without the flag
    s.aov_rays(render, ro, rd)
    off = s.denoise(passes=5)
    assert same_bits(off, H.x86_filter(probe, rrgb, counts, ref["guide"], ref["albedo"], 5, *default_sigmas(), False)) == 0
    assert same_bits(off[:, [0, 1, -2, -1]], rolled[:, [0, 1, -2, -1]]) > 0
    s.close()


def test_unwrapped_denoise_equals_the_wrapped_one_far_from_the_seam():
    spp, passes = 16, 5
    render, holder, s, o, d, rgb = _pano((160, 24), spp=spp)
    s.set_accum(rgb, spp)
    s.aov_rays(render, o, d, wrap_x=True)
    on = s.denoise(passes=passes)
    s.aov_rays(render, o, d)
    off = s.denoise(passes=passes)
    reach = H.seam_reach(passes)
    assert reach == 62 and s.nw - 2 * reach > 0
    assert same_bits(on[:, reach:s.nw - reach], off[:, reach:s.nw - reach]) == 0
    assert same_bits(on[:, :reach], off[:, :reach]) > 0 and same_bits(on[:, s.nw - reach:], off[:, s.nw - reach:]) > 0
    s.close()


# ---- 11: state -------------------------------------------------------------------------------------------------------------------
def test_reset_keeps_the_planes_and_null_rays_return_the_cameras():
    render = load_render(scenes.cornell_box(res=(40, 36), sample=2))
    fresh = Sampler(seed=1, device=0).create(render)
    cam = fresh.aov()
    fresh.close()
    s = Sampler(seed=1, device=0).create(render)
    o, d = cameras.equirect(render.frame.cam.pos, s.nw, s.nh)
    s.aov_rays(render, o, d, wrap_x=True)
    mine = s.aov()
    assert any(planes_differ(mine, cam).values())
    s.execute(render, n_samples=2)
    info = {}
    s.denoise(passes=1, info=info)
    assert info["aov_cached"] == 1 and info["aov_ms"] == 0
    s.reset()
    assert_same_planes(s.aov(), mine, "after reset")
    s.execute(render, n_samples=2)
    A, cnt = s.accum()
    s.set_accum(A, cnt)
    assert_same_planes(s.aov(), mine, "after set_accum")
    s.aov_rays(render, None, None)
    assert_same_planes(s.aov(), cam, "after (NULL, NULL, 0)")
    s.denoise(passes=1, info=info)
    assert info["aov_cached"] == 1
    s.close()
    # dropped before any use: the next use computes the camera's
    s = Sampler(seed=1, device=0).create(render)
    s.aov_rays(render, None, None)
    s.aov_rays(render, o, d)
    s.aov_rays(render, None, None)
    assert_same_planes(s.aov(), cam, "dropped unused")
    s.close()


def test_the_call_is_not_an_observation():
    render = load_render(scenes.cornell_box(res=(40, 36), sample=4))
    s = Sampler(seed=6, device=0, flags=_abi.FLAG_COUNT_SEGMENTS)
    s.execute(render, n_samples=4)
    o, d = cameras.equirect(render.frame.cam.pos, s.nw, s.nh)
    A0, c0 = s.accum()
    st0 = s.stats()
    s.aov_rays(render, o, d, wrap_x=True)
    A1, c1 = s.accum()
    assert c1 == c0 == 4 and same_bits(A1, A0) == 0 and s.stats() == st0
    s.close()

    # ... nor does it change what comes next, whatever the context has in flight: eager batches, samples booked under
    # MRT_FLAG_DEFER (traced by the next observation, the same samples), one-sample calls with the look-ahead running
    def run(flags, calls, with_call):
        x = Sampler(seed=6, device=0, flags=flags)
        for i, n in enumerate(calls):
            x.execute(render, n_samples=n)
            if with_call and i == len(calls) // 2:
                x.aov_rays(render, o, d, wrap_x=True)
        out = x.accum()
        x.close()
        return out

    for flags, calls in ((0, (4, 3)), (_abi.FLAG_DEFER, (4, 3)), (0, (1,) * 7)):
        (B0, n0), (B1, n1) = run(flags, calls, False), run(flags, calls, True)
        assert n0 == n1 == 7 and same_bits(B0, B1) == 0, (flags, calls)


def test_variance_mode_is_refused_on_supplied_ray_planes():
    render = load_render(scenes.cornell_box(res=(40, 36), sample=32))
    s = Sampler(seed=3, device=0)
    s.execute_adaptive(render, 0.0, min_samples=32, max_samples=32, step=16)
    want = s.denoise(mode="variance")
    o, d = s.camera_rays(render)
    s.aov_rays(render, o, d)
    for fn in (lambda: s.denoise(mode="variance"), lambda: s.img_denoised(mode="variance"), lambda: s.img_hdr(denoise=dict(mode="variance"))):
        with pytest.raises(_lib.MrtError) as e:
            fn()
        assert e.value.code == _abi.MRT_ERR_STATE and "mrt_aov_rays(ctx, NULL, NULL, 0)" in e.value.msg and "half buffer" in e.value.msg
    assert s.denoise().shape == (36, 40, 3)                # the a-trous mode serves
    s.aov_rays(render, None, None)
    assert same_bits(s.denoise(mode="variance"), want) == 0
    s.close()


def test_a_sharded_context_takes_the_whole_grid():
    render = load_render(scenes.cornell_box(res=(40, 36), sample=2))
    whole = Sampler(seed=1, device=0).create(render)
    o, d = cameras.equirect(render.frame.cam.pos, whole.nw, whole.nh)
    whole.aov_rays(render, o, d)
    want = whole.aov()
    whole.close()
    for rank in (0, 1):
        sh = Sampler(seed=1, device=0, shard_index=rank, shard_count=2).create(render)
        sh.aov_rays(render, o, d)
        assert_same_planes(sh.aov(), want, f"rank {rank}")
        sh.close()


_GROUP_SCRIPT = r"""
import os
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from micro_raytracer_amd import Sampler, _abi, _lib, load_render, scenes
os.environ["MRT_FORCE_RCCL"] = "1"              # the group path with a communicator of one device
render = load_render(scenes.cornell_box(res=(32, 16), sample=4))
g = Sampler(seed=3, n_devices=1).create(render)
o = np.zeros((g.nh, g.nw, 3), np.float32)
d = np.tile(np.asarray([0, 1, 0], np.float32), (g.nh, g.nw, 1))
try:
    g.aov_rays(render, o, d)
except _lib.MrtError as e:
    assert e.code == _abi.MRT_ERR_STATE and "mrt_aov_rays" in e.msg and "multi-device" in e.msg, e
else:
    raise AssertionError("a multi-device context served mrt_aov_rays")
assert _lib.lib().mrt_aov_rays(g._ctx, None, None, 0) == _abi.MRT_ERR_STATE
g.execute(render, n_samples=4)                  # the refused calls left the context usable
assert g.accum()[1] == 4 and g.aov()["depth"].shape == (16, 32)
g.close()
print("GROUP-REFUSES")
"""


def test_a_multi_device_context_refuses_the_call():
    """mrt_opts.n_devices: MRT_ERR_STATE, through the group path on one device (MRT_FORCE_RCCL) in a fresh interpreter, as
    tests/test_gpu_rays.py does it for mrt_radiance."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _GROUP_SCRIPT, root], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "GROUP-REFUSES" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_argument_errors():
    render = load_render(scenes.cornell_box(res=(16, 16), sample=2))
    s = Sampler(seed=1, device=0).create(render)
    o, d = s.camera_rays(render)
    L = _lib.lib()
    po, pd = o.ctypes.data, d.ctypes.data
    bad = [(None, None, None, 0), (s._ctx, po, None, 0), (s._ctx, None, pd, 0), (s._ctx, po, pd, 4), (s._ctx, po, pd, 0x80000001),
           (s._ctx, None, None, _abi.AOV_WRAP_X), (s._ctx, None, None, _abi.AOV_RAYS_DEVICE)]
    for args in bad:
        assert L.mrt_aov_rays(*args) == _abi.MRT_ERR_ARG, args
        assert L.mrt_last_error().decode().startswith("mrt_aov_rays:")
    assert L.mrt_aov_rays(s._ctx, po, pd, _abi.AOV_WRAP_X) == _abi.MRT_OK         # the context still works
    s.execute(render, n_samples=2)
    assert np.isfinite(s.denoise(passes=2)).all()
    s.close()


# ---- 12: quality -----------------------------------------------------------------------------------------------------------------
def test_quality_of_a_denoised_panorama():
    """Equirect 256x128 inside the Cornell box, 16 spp against 1024 spp of another seed, tone-mapped RMSE.  Measured on an MI355X
    (DESIGN.md §20); asserted: the denoised error is below the raw one, and over the 16 columns at the seam the wrapped filter's
    error is at most 1.1 x the unwrapped one's (a finite-sample comparison of two filters, the margin of test_gpu_denoise.py)."""
    render = load_render(scenes.cornell_box(res=(256, 128), sample=16))
    cam = render.frame.cam
    gt = Sampler(seed=1001, device=0).create(render)
    o, d = cameras.equirect(cam.pos, gt.nw, gt.nh)
    G = gt.radiance(render, o, d, 1024)
    gt.close()
    s = Sampler(seed=7, device=0)
    A = cameras.render_equirect(s, render, 16, guides=True)
    ref = tonemapped(G / f32(1024), cam.gamma, cam.exp)
    seam = np.r_[0:8, gt.nw - 8:gt.nw]
    err = lambda img, cols=slice(None): float(np.sqrt(np.mean((tonemapped(img, cam.gamma, cam.exp) - ref)[:, cols] ** 2)))
    wrapped = s.denoise()
    s.aov_rays(render, o, d)
    unwrapped = s.denoise()
    s.close()
    raw, r_on, r_off = err(A / f32(16)), err(wrapped), err(unwrapped)
    s_raw, s_on, s_off = err(A / f32(16), seam), err(wrapped, seam), err(unwrapped, seam)
    print(f"equirect cornell 256x128 16 spp: raw {raw:.4f}, wrapped {r_on:.4f} ({r_on / raw:.3f} x raw), unwrapped {r_off:.4f} "
          f"({r_off / raw:.3f} x raw); seam 16 columns: raw {s_raw:.4f}, wrapped {s_on:.4f} ({s_on / s_raw:.3f} x raw), "
          f"unwrapped {s_off:.4f} ({s_off / s_raw:.3f} x raw), wrapped / unwrapped {s_on / s_off:.3f}")
    assert r_on < raw and r_off < raw
    assert s_on <= 1.1 * s_off


# ---- 13: the CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_pano_guides(tmp_path):
    from micro_raytracer_amd import __main__ as cli
    desc = scenes.cornell_box(res=(64, 32), sample=8)
    path, out, pre = tmp_path / "box.json", tmp_path / "pano.png", tmp_path / "a"
    path.write_text(json.dumps(desc))
    cli.main([str(path), "-o", str(out), "--camera", "equirect", "--pano-guides", "--denoise", "--aov", str(pre), "--seed", "3"])
    render = load_render(desc)
    s = Sampler(seed=3)
    cameras.render_equirect(s, render, guides=True)
    cli.save(str(tmp_path / "want.png"), s.img_denoised())
    cli.save_aov(s, str(tmp_path / "w"))
    raw = s.img()
    dn = s.denoise()
    cli.save(str(tmp_path / "want.pfm"), s.img_hdr(denoise=dict(passes=_abi.DENOISE_PASSES)))
    pin = Sampler(seed=3).create(render)
    cam_aov = pin.aov()
    pin.close()
    assert any(planes_differ(s.aov(), cam_aov).values())                  # the panorama's planes, not the pinhole's
    assert not np.array_equal(s.img_denoised(), raw) and dn.shape == (32, 64, 3)
    s.close()
    read = lambda p: open(p, "rb").read()
    assert read(out) == read(tmp_path / "want.png") and read(out)[:8] == b"\x89PNG\r\n\x1a\n"
    for name in ("normal", "albedo", "depth"):
        assert read(f"{pre}.{name}.png") == read(tmp_path / f"w.{name}.png")
    cli.main([str(path), "-o", str(tmp_path / "pano.pfm"), "--camera", "equirect", "--pano-guides", "--denoise", "--seed", "3"])
    assert read(tmp_path / "pano.pfm") == read(tmp_path / "want.pfm")
