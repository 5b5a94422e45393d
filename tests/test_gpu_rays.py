"""mrt_radiance / mrt_camera_rays on the GPU: the camera's own rays give the accumulator bits of mrt_execute at
every staging level, rays no pinhole forms give the bits of the x86 build and meet the float64 core, ragged batches, device
pointers, keys, the context is left untouched, every argument error has its code, and the CLI's panorama."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import core_cases as K
import inst_cases as IC
import rays_ref as Y
from conftest import make_holder

pytestmark = pytest.mark.gpu
f32 = np.float32
F_COLD, F_DEEP = 64, 128
LDS_QUARTER = 160 * 1024 // 4


@pytest.fixture(scope="module")
def probe():
    return Y.shared_probe()


def _sampler(seed=Y.SEED, **kw):
    from micro_raytracer_amd import Sampler
    return Sampler(seed=seed, device=0, **kw)


def _frame_bits(render, spp=Y.SPP, **kw):
    """The accumulator of a fresh context after execute(spp)."""
    s = _sampler(**kw)
    s.execute(render, n_samples=spp)
    acc, cnt = s.accum()
    st = s.stats()
    s.close()
    assert cnt == spp
    return acc, st


def _rays_run(render, spp=Y.SPP):
    """(sums of radiance on the context's own camera rays, info, plan) on a fresh context."""
    from micro_raytracer_amd import _abi, _lib
    s = _sampler().create(render)
    plan = _lib.plan_launch(_abi.build_desc(render))
    o, d = s.camera_rays(render)
    info = {}
    got = s.radiance(render, o, d, spp, info=info)
    assert s.accum()[1] == 0
    s.close()
    return got, info, plan, (o, d)


def _expect_lds(plan):
    return plan["staging"] == "all" and plan["staged_bytes"] <= LDS_QUARTER


@functools.lru_cache(maxsize=None)
def _recipe_case(level):
    row = {"all": (256, True, Y.F_ALL), "warm": (256, True, Y.F_ALL | F_COLD), "deep": (256, True, Y.F_ALL | F_COLD | F_DEEP), "none": (256, False, Y.F_ALL)}[level]
    rc = IC.recipe(*row)
    return make_holder(Y._sized(IC.describe(rc.scene))), rc.env


# ---- 5: equivalence to mrt_execute --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", ["all", "warm", "deep", "none"])
def test_camera_rays_give_the_frame_at_every_staging_level(probe, monkeypatch, level):
    (render, holder), env = _recipe_case(level)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, info, plan, _ = _rays_run(render)
    frame, st = _frame_bits(render)
    assert plan["staging"] == level
    diff = int((Y.bits(got) != Y.bits(frame)).any(-1).sum())
    print(f"rays at staging level {level}: frame kernel FEAT {st['kernel_features']}, rays kernel FEAT {info['kernel_features']}, in LDS {info['scene_in_lds']} "
          f"({info['lds_bytes']} B), {info['kernel_ms']:.3f} ms, {info['segments']} segments; {diff} pixels differ")
    assert diff == 0
    assert info["scene_in_lds"] == int(_expect_lds(plan)) and (level == "all" or info["scene_in_lds"] == 0)
    assert info["kernel_features"] == Y.x86_info(probe, holder)["rays_inst"] == Y.F_ALL
    assert info["samples"] == Y.RES[0] * Y.RES[1] * Y.SPP and info["segments"] >= info["samples"]
    assert info["lds_bytes"] == ((plan["staged_bytes"] + 15) & ~15 if info["scene_in_lds"] else 0)


@pytest.mark.parametrize("name", ["cornell", "lights", "primitives", "env_vattr"])
def test_camera_rays_give_the_frame_staged_and_through_l2(probe, monkeypatch, name):
    """The four frame scenes as mrt_create plans them (the two small ones stage everything: level 0; the two with a mesh stage
    warm), then under MRT_SCENE_IN_L2: the same bits, and info says which of the two kernels ran."""
    render, holder = Y.frame_case(name)
    frame, st = _frame_bits(render)
    got, info, plan, _ = _rays_run(render)
    assert plan["staging"] == ("all" if name in ("cornell", "lights") else "warm")
    assert info["scene_in_lds"] == int(_expect_lds(plan)) == int(plan["staging"] == "all")
    assert info["kernel_features"] == Y.x86_info(probe, holder)["rays_inst"]
    assert Y.same(got, frame), int((Y.bits(got) != Y.bits(frame)).any(-1).sum())
    monkeypatch.setenv("MRT_SCENE_IN_L2", "1")
    got2, info2, plan2, _ = _rays_run(render)
    assert plan2["staging"] == "none" and info2["scene_in_lds"] == 0 and info2["lds_bytes"] == 0 and info2["kernel_features"] == info["kernel_features"]
    assert Y.same(got2, got)
    print(f"rays {name}: frame FEAT {st['kernel_features']}, rays FEAT {info['kernel_features']}; staged {info['kernel_ms']:.3f} ms ({info['lds_bytes']} B), "
          f"through L2 {info2['kernel_ms']:.3f} ms")


# ---- 6: rays no pinhole forms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Y.WINDOWS))
def test_window_rays_equal_x86_and_meet_float64(probe, name):
    render, holder, o, d, ref, img32 = Y.window_case(name)
    s = _sampler(seed=1).create(render)
    info = {}
    two = s.radiance(render, o, d, 2, info=info)
    s.close()
    want = Y.x86_radiance(probe, holder, info["kernel_features"], o, d, 2, seed=1)
    assert Y.same(two, want), int((Y.bits(two) != Y.bits(want)).any(-1).sum())
    K.compare_image(f"GPU rays window {name}", two / f32(2), ref, img32)


# ---- 7: the camera's rays through the query hook ------------------------------------------------------------------------------
def test_camera_rays_through_the_query_hook_give_the_depth_aov():
    from micro_raytracer_amd import _lib
    render, _ = Y.frame_case("primitives")
    s = _sampler().create(render)
    o, d = s.camera_rays(render)
    depth = s.aov()["depth"].reshape(-1)
    w = _lib.selftest_trace(s, o.reshape(-1, 3), d.reshape(-1, 3))
    s.close()
    hit = w["hit"]
    assert 100 < hit.sum() and 100 < (~hit).sum()
    assert np.array_equal(Y.bits(w["t0"])[hit], Y.bits(depth)[hit])
    assert np.isposinf(depth[~hit]).all() and (w["words"][~hit, 0] == 0).all()


# ---- 8: ragged batches --------------------------------------------------------------------------------------------------------
def test_ragged_batches_keep_every_rays_bits():
    render, _ = Y.frame_case("cornell")
    s = _sampler().create(render)
    o, d = (a.reshape(-1, 3) for a in s.camera_rays(render))
    whole = s.radiance(render, o, d, Y.SPP)
    for n in (1, 63, 65, 257):
        part = s.radiance(render, o[:n], d[:n], Y.SPP)
        assert part.shape == (n, 3) and Y.same(part, whole[:n]), n
    s.close()


def test_keys_and_sample_ranges_on_the_gpu():
    render, _ = Y.frame_case("cornell")
    s = _sampler().create(render)
    o, d = (a.reshape(-1, 3) for a in s.camera_rays(render))
    n = o.shape[0]
    whole = s.radiance(render, o, d, 32)
    assert Y.same(s.radiance(render, o, d, 32, key=np.arange(n)), whole)
    assert Y.same(s.radiance(render, o[::-1], d[::-1], 32, key=np.arange(n)[::-1])[::-1], whole)
    a, b = s.radiance(render, o, d, 16), s.radiance(render, o, d, 16, sample_base=16)
    assert Y.same(a + b, whole) and not Y.same(a, b)
    s.close()


# ---- 9: the context is untouched ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defer", [False, True])
def test_the_context_is_untouched(defer):
    from micro_raytracer_amd import _abi
    render, _ = Y.frame_case("cornell")
    flags = _abi.FLAG_DEFER if defer else 0

    def run(with_rays):
        s = _sampler(flags=flags)
        s.execute(render, n_samples=8)
        if with_rays:
            o, d = s.camera_rays(render)
            s.radiance(render, o, d, 24, sample_base=3)
        s.execute(render, n_samples=8)
        acc, cnt = s.accum()
        st = s.stats()
        s.close()
        return acc, cnt, (st["launches"], st["samples"], st["deferred"])

    (a, ca, sa), (b, cb, sb) = run(True), run(False)
    assert ca == cb == 16 and Y.same(a, b)
    # booked samples stay booked across the call: both executes still run as the one batch of the observation
    assert sa == sb and sa[2] == int(defer), (sa, sb)


def test_cached_aovs_survive_a_radiance_call():
    render, _ = Y.frame_case("lights")
    s = _sampler()
    s.execute(render, n_samples=8)
    before = s.aov()
    o, d = s.camera_rays(render)
    s.radiance(render, o, d, 8)
    info = {}
    s.denoise(info=info)
    after = s.aov()
    s.close()
    assert info["aov_cached"] == 1
    assert all(np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)) for k in ("depth", "normal", "albedo"))


@pytest.mark.parametrize("level", ["deep", "all"])
def test_radiance_and_aov_share_the_flat_scene_in_either_order(oracle_mod, monkeypatch, level):
    """mrt_radiance and the AOV pass read the scene as a kernel without F_DEEP reads it, through one accessor of the context: on a
    deep-staged context the binary-BVH packing, uploaded by whichever call comes first; on a context that stages everything its
    own blob.  Either order: the radiance is the frame's bits, the AOVs are the oracle's (bit-equal planes, equal ids)."""
    import test_oracle_aov as A
    from micro_raytracer_amd import _lib
    (render, holder), env = _recipe_case(level)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert _lib.plan_launch(holder)["staging"] == level
    frame, _ = _frame_bits(render)
    ref = A.oracle_aov(oracle_mod, holder)

    def run(rays_first):
        s = _sampler().create(render)
        o, d = s.camera_rays(render)
        aov = None if rays_first else s.aov()
        got = s.radiance(render, o, d, Y.SPP)
        aov = aov or s.aov()
        s.close()
        return got, aov

    (r1, a1), (r2, a2) = run(True), run(False)
    assert Y.same(r1, r2) and Y.same(r1, frame), int((Y.bits(r1) != Y.bits(frame)).any(-1).sum())
    assert set(a1) == set(a2) == {"depth", "normal", "albedo", "renderer", "instance"}
    for k in a1:
        assert np.array_equal(a1[k].view(np.uint32), a2[k].view(np.uint32)), k
    A.compare_aov(f"{level}, radiance then aov", a1, ref)
    A.compare_aov(f"{level}, aov then radiance", a2, ref)


# ---- 10: device pointers ------------------------------------------------------------------------------------------------------
_DEVICE_SCRIPT = r"""
import sys
import numpy as np
import torch
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)                      # torch brings the HIP runtime up first, as in bench.py and dist.ShardedSampler
sys.path[:0] = sys.argv[1:3]
import rays_ref as Y
from micro_raytracer_amd import Sampler
render, _ = Y.frame_case("primitives")
s = Sampler(seed=Y.SEED, device=0).create(render)
o, d = s.camera_rays(render)
host = s.radiance(render, o, d, Y.SPP)
to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
out = s.radiance(render, to, td, Y.SPP)
assert isinstance(out, torch.Tensor) and out.is_cuda and tuple(out.shape) == o.shape
assert Y.same(out.cpu().numpy(), host)
n = o.shape[0] * o.shape[1]
key = torch.arange(n, dtype=torch.int32, device=dev).flip(0)
rev = s.radiance(render, to.reshape(-1, 3).flip(0), td.reshape(-1, 3).flip(0), Y.SPP, key=key)
assert Y.same(rev.flip(0).cpu().numpy().reshape(o.shape), host)
try:
    s.radiance(render, to, d, Y.SPP)
except ValueError:
    pass
else:
    raise AssertionError("a device tensor and a host array were accepted together")
s.close()
print("device tensors ok")
"""


def test_device_tensors_give_the_host_paths_bits():
    """Torch tensors on the context's device in, a tensor with the host path's bits out (MRT_RAYS_DEVICE), keys included.  In a
    child process: torch has to bring the HIP runtime up before the library does, which no test of this process can still arrange."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _DEVICE_SCRIPT, root, os.path.join(root, "tests")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "device tensors ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 11: argument and state errors; sharded contexts ----------------------------------------------------------------------------
def _call(s, o, d, out, **kw):
    from micro_raytracer_amd import _abi, _lib
    r = _abi.Rays()
    r.n, r.orig, r.dir, r.n_samples = o.shape[0], o.ctypes.data, d.ctypes.data, 4
    null_out = kw.pop("null_out", False)
    for k, v in kw.items():
        if k == "reserved":
            r.reserved[v] = 1
        else:
            setattr(r, k, v)
    L = _lib.lib()
    rc = L.mrt_radiance(s._ctx, C.byref(r), None if null_out else C.c_void_p(out.ctypes.data), None)
    return rc, L.mrt_last_error().decode()


def test_argument_errors_have_their_code_and_a_message():
    from micro_raytracer_amd import _abi, _lib
    render, _ = Y.frame_case("cornell")
    s = _sampler().create(render)
    o, d = (np.ascontiguousarray(a.reshape(-1, 3)[:70]) for a in s.camera_rays(render))
    out = np.zeros_like(o)
    assert _call(s, o, d, out)[0] == _abi.MRT_OK
    bad = [dict(orig=None), dict(dir=None), dict(null_out=True), dict(n=0), dict(n=1 << 30), dict(n_samples=0),
           dict(sample_base=0xffffffff, n_samples=1), dict(sample_base=0xfffffff0, n_samples=16), dict(flags=2), dict(flags=0x80000001),
           dict(reserved=0), dict(reserved=1), dict(reserved=2)]
    for kw in bad:
        rc, msg = _call(s, o, d, out, **kw)
        assert rc == _abi.MRT_ERR_ARG and msg.startswith("mrt_radiance:") and len(msg) > 16, (kw, rc, msg)
    L = _lib.lib()
    assert L.mrt_radiance(s._ctx, None, C.c_void_p(out.ctypes.data), None) == _abi.MRT_ERR_ARG
    assert L.mrt_radiance(None, None, None, None) == _abi.MRT_ERR_ARG and L.mrt_camera_rays(None, None, None) == _abi.MRT_ERR_ARG
    # the last legal sample range
    rc, _ = _call(s, o, d, out, sample_base=0xffffffff - 4, n_samples=4)
    assert rc == _abi.MRT_OK
    s.close()


def test_a_sharded_context_serves_the_call():
    render, _ = Y.frame_case("lights")
    s = _sampler().create(render)
    o, d = s.camera_rays(render)
    whole = s.radiance(render, o, d, Y.SPP)
    s.close()
    for rank in (0, 1):
        sh = _sampler(shard_index=rank, shard_count=2).create(render)
        so, sd = sh.camera_rays(render)
        assert Y.same(so, o) and Y.same(sd, d)
        assert Y.same(sh.radiance(render, o, d, Y.SPP), whole)
        # a rank's slice of the batch, with the keys of the slice
        n = o.shape[0] * o.shape[1]
        sl = slice(rank * (n // 2), n // 2 + rank * (n - n // 2))
        part = sh.radiance(render, o.reshape(-1, 3)[sl], d.reshape(-1, 3)[sl], Y.SPP, key=np.arange(n)[sl])
        assert Y.same(part, whole.reshape(-1, 3)[sl])
        sh.close()


_GROUP_SCRIPT = r"""
import ctypes as C
import os
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from micro_raytracer_amd import Sampler, _abi, _lib, load_render, scenes
os.environ["MRT_FORCE_RCCL"] = "1"              # the group path with a communicator of one device
render = load_render(scenes.cornell_box(res=(32, 16), sample=4))
g = Sampler(seed=3, n_devices=1).create(render)
o = np.zeros((4, 3), np.float32)
d = np.tile(np.asarray([0, 1, 0], np.float32), (4, 1))
try:
    g.radiance(render, o, d, 4)
except _lib.MrtError as e:
    assert e.code == _abi.MRT_ERR_STATE and "mrt_radiance" in e.msg and "multi-device" in e.msg, e
else:
    raise AssertionError("a multi-device context served mrt_radiance")
assert _lib.lib().mrt_camera_rays(g._ctx, None, None) == _abi.MRT_ERR_STATE
g.execute(render, n_samples=4)                  # the refused calls left the context usable
assert g.accum()[1] == 4
g.close()
print("GROUP-REFUSES")
"""


def test_a_multi_device_context_refuses_the_call():
    """mrt_opts.n_devices: MRT_ERR_STATE with a message, through the group path on one device (MRT_FORCE_RCCL), in a fresh
    interpreter like the group test of tests/test_gpu_dist.py: the library loads librccl.so itself."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _GROUP_SCRIPT, root], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "GROUP-REFUSES" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- 12: the CLI's panorama ----------------------------------------------------------------------------------------------------
def test_cli_equirect_panorama(probe, tmp_path, monkeypatch):
    from micro_raytracer_amd import Sampler, __main__ as cli, cameras, scenes
    desc = scenes.cornell_box(res=(64, 32), sample=8)
    path, out = tmp_path / "box.json", tmp_path / "pano.png"
    path.write_text(json.dumps(desc))
    seen = []
    real = Sampler.set_accum
    monkeypatch.setattr(Sampler, "set_accum", lambda self, rgb, count: (seen.append((np.array(rgb), count)), real(self, rgb, count))[1])
    cli.main([str(path), "-o", str(out), "--camera", "equirect", "--pano-yaw", "0.125", "--seed", "3"])
    assert len(seen) == 1 and seen[0][1] == 8 and seen[0][0].shape == (32, 64, 3)
    render, holder = make_holder(desc)
    o, d = cameras.equirect(render.frame.cam.pos, 64, 32, yaw=0.125)
    want = Y.x86_radiance(probe, holder, Y.x86_info(probe, holder)["rays_inst"], o, d, 8, seed=3)
    assert Y.same(seen[0][0], want)
    assert os.path.getsize(out) > 100 and open(out, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    for extra in (["--adaptive", "0.1"], ["--denoise"], ["--aov", str(tmp_path / "a")], ["--update"]):
        with pytest.raises(SystemExit):
            cli.main([str(path), "-o", str(out), "--camera", "equirect", *extra])
