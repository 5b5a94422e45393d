"""mrt_gather / mrt_gather_rays on the GPU: a gather is the numpy reduction of mrt_radiance on its own rays, bit for
bit, for every distribution, output, batch size and sample range, through host arrays and through device tensors; the rays are those
of the x86 build; a constant sky comes back exactly; the context is left untouched; every argument error has its code and message.

Comparisons are by bits with NaN equal to NaN (gather_ref.same_bits): the point with a zero normal has NaN directions, and the sign and
payload of a NaN are not part of the contract, as in the project's other bit comparisons."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import gather_ref as G

pytestmark = pytest.mark.gpu
f32 = np.float32
SEED = 0x5DEECE66D1234567
KEY_BASE = 1000
# seven points in the Cornell box (x, y in [-1, 1], z in [-0.2, 1]): free space, next to the emitter, ON the red wall, on the floor, and
# one whose normal is zero
POS = np.array([(0.0, -0.6, 0.3), (0.5, 0.2, 0.1), (-1.0, 0.2, 0.4), (0.3, -0.3, -0.2), (-0.4, 0.6, 0.7), (0.0, 0.0, 0.5), (0.7, -0.7, 0.9)], f32)
NRM = np.array([(0, 0, 1), (0.2, 0.3, -2.0), (1, 0, 0), (0, 0, 1), (0, 0, 0), (-3, 1, 0.5), (0, 1, -0.0)], f32)
MODES = {"sphere-mean": (False, "mean"), "sphere-sh9": (False, "sh9"), "hemi-mean": (True, "mean")}


@functools.lru_cache(maxsize=None)
def _render():
    from micro_raytracer_amd import load_render, scenes
    return load_render(scenes.cornell_box(res=(16, 16), bounce=4))


@pytest.fixture(scope="module")
def sampler():
    from micro_raytracer_amd import Sampler
    s = Sampler(seed=SEED, device=0).create(_render())
    yield s
    s.close()


@pytest.fixture(scope="module")
def probe():
    return G.probe()


@functools.lru_cache(maxsize=None)
def _rays(s, hemi, n_dirs):
    return s.gather_rays(_render(), POS, NRM if hemi else None, n_dirs=n_dirs, key_base=KEY_BASE)


def _reference(s, hemi, out, n_dirs, n_samples, sample_base):
    o, d, k = _rays(s, hemi, n_dirs)
    sums = s.radiance(_render(), o, d, n_samples, sample_base=sample_base, key=k)
    return G.reduce(sums, d, n_samples, G.SH9 if out == "sh9" else G.MEAN)


# ---- composition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_samples", [16, 17])
@pytest.mark.parametrize("n_dirs", [1, 63, 65, 130])
@pytest.mark.parametrize("mode", list(MODES))
def test_gather_is_the_reduction_of_radiance_on_its_own_rays(sampler, mode, n_dirs, n_samples):
    hemi, out = MODES[mode]
    nrm = NRM if hemi else None
    for sample_base in (0, 16):
        ref = _reference(sampler, hemi, out, n_dirs, n_samples, sample_base)
        for batch_points in (0, 3):
            kw = dict(n_dirs=n_dirs, n_samples=n_samples, out=out, key_base=KEY_BASE, sample_base=sample_base, batch_points=batch_points)
            info = {}
            got = sampler.gather(_render(), POS, nrm, info=info, **kw)
            assert got.shape == ref.shape and got.dtype == f32
            assert G.same_bits(got, ref) == 0, (sample_base, batch_points, np.argwhere(got.view(np.uint32) != ref.view(np.uint32))[:4])
            assert info["batches"] == (3 if batch_points else 1) and info["rays"] == 7 * n_dirs and info["samples"] == 7 * n_dirs * n_samples
            assert info["segments"] >= 6 * n_dirs * n_samples
        # the zero normal of point 4 (NaN rays, whose radiance is whatever mrt_radiance gives) disturbs no other point
        assert np.isfinite(ref[[0, 1, 2, 3, 5, 6]]).all()


def test_gather_rays_equal_the_x86_build(sampler, probe):
    for hemi in (False, True):
        nrm = NRM if hemi else None
        for n_dirs in (1, 63, 64, 65, 130):
            o, d, k = _rays(sampler, hemi, n_dirs)
            xo, xd, xk = G.x86_rays(probe, SEED, KEY_BASE, n_dirs, G.HEMI_COS if hemi else G.SPHERE, 1e-4, POS, nrm)
            assert G.same_bits(o, xo) == 0 and G.same_bits(d, xd) == 0 and np.array_equal(k, xk), (hemi, n_dirs)
            assert k.dtype == np.uint32 and np.array_equal(k, G.keys_of(KEY_BASE, 0, 7, n_dirs))
        # a slice
        o, d, k = _rays(sampler, hemi, 65)
        o2, d2, k2 = sampler.gather_rays(_render(), POS, nrm, n_dirs=65, key_base=KEY_BASE, first=2, count=4)
        assert G.same_bits(o2, o[2:6]) == 0 and G.same_bits(d2, d[2:6]) == 0 and np.array_equal(k2, k[2:6])


_DEVICE_SCRIPT = r"""
import sys
import numpy as np
import torch
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)                      # torch brings the HIP runtime up first, as in bench.py and dist.ShardedSampler
sys.path[:0] = sys.argv[1:3]
import gather_ref as G
import test_gpu_gather as T
from micro_raytracer_amd import Sampler
render = T._render()
s = Sampler(seed=T.SEED, device=0).create(render)
t_pos, t_nrm = torch.from_numpy(T.POS).to(dev), torch.from_numpy(T.NRM).to(dev)
runs = 0
for hemi, out in T.MODES.values():
    nrm, tn = (T.NRM, t_nrm) if hemi else (None, None)
    for n_dirs in (1, 63, 65, 130):
        o, d, k = s.gather_rays(render, T.POS, nrm, n_dirs=n_dirs, key_base=T.KEY_BASE)
        to, td, tk = s.gather_rays(render, t_pos, tn, n_dirs=n_dirs, key_base=T.KEY_BASE)
        assert to.is_cuda and td.is_cuda and tk.is_cuda and tuple(tk.shape) == k.shape
        assert G.same_bits(to.cpu().numpy(), o) == 0 and G.same_bits(td.cpu().numpy(), d) == 0
        assert np.array_equal(tk.cpu().numpy().view(np.uint32), k)
        for n_samples in (16, 17):
            for sample_base in (0, 16):
                sums = s.radiance(render, to, td, n_samples, sample_base=sample_base, key=tk.view(torch.int32))
                ref = G.reduce(sums.cpu().numpy(), d, n_samples, G.SH9 if out == "sh9" else G.MEAN)
                for batch_points in (0, 3):
                    kw = dict(n_dirs=n_dirs, n_samples=n_samples, out=out, key_base=T.KEY_BASE, sample_base=sample_base, batch_points=batch_points)
                    got = s.gather(render, t_pos, tn, **kw)
                    assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == ref.shape
                    assert G.same_bits(got.cpu().numpy(), ref) == 0, (hemi, out, kw)
                    assert G.same_bits(s.gather(render, T.POS, nrm, **kw), ref) == 0, (hemi, out, kw)
                    runs += 1
try:
    s.gather(render, t_pos, T.NRM)
except ValueError:
    pass
else:
    raise AssertionError("a device tensor and a host array were accepted together")
s.close()
print("device tensors ok:", runs)
"""


def test_device_tensors_give_the_same_composition():
    """Every case of the composition test once more with positions, normals, rays, keys, sums and answers as torch tensors on the
    context's device (MRT_RAYS_DEVICE): the reduction of radiance on the gather's own rays, and the host path's bits.  In a child
    process: torch has to bring the HIP runtime up before the library does, which no test of this process can still arrange."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _DEVICE_SCRIPT, root, os.path.join(root, "tests")], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "device tensors ok: 96" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- closed form -----------------------------------------------------------------------------------------------------------------
def test_constant_sky_comes_back_exactly():
    """One sphere of radius 0.1 at (0, 0, -1000) under a sky of (0.5, 0.25, 1.0), gathered at the origin: no ray of either set meets
    the sphere, every sample is the sky colour and every step of the mean is exact (16 x colour, / 16, 64 terms, / 64)."""
    from micro_raytracer_amd import Sampler, load_render
    colour = np.array([0.5, 0.25, 1.0], f32)
    desc = {"rt": {"sample": 16, "bounce": 4}, "frame": {"res": [16, 16], "ssaa": 1, "cam": {"pos": [0, -1, 0]}},
            "scene": {"renderer": [{"type": "sphere", "r": 0.1, "pos": [0, 0, -1000]}], "sky": {"color": [0.5, 0.25, 1.0], "pwr": 0.5}}}
    render = load_render(desc)
    s = Sampler(seed=3, device=0)
    origin = np.zeros((1, 3), f32)
    hemi = s.gather(render, origin, np.array([[0, 0, 1]], f32), n_dirs=64, n_samples=16)
    sphere = s.gather(render, origin, n_dirs=64, n_samples=16)
    assert np.array_equal(hemi.view(np.uint32), colour.view(np.uint32)[None]) and np.array_equal(sphere.view(np.uint32), colour.view(np.uint32)[None])
    sh = s.gather(render, origin, n_dirs=256, n_samples=16, out="sh9")[0].astype(np.float64)
    s.close()
    c0 = 2.0 * np.sqrt(np.pi) * colour.astype(np.float64)
    print(f"SH9 of a constant sky, n_dirs 256: c_0 relative error {np.abs(sh[0] / c0 - 1.0).max():.3e}, largest |c_k| / colour {np.abs(sh[1:] / colour).max():.3e}")
    assert np.abs(sh[0] / c0 - 1.0).max() <= 1e-6
    assert (np.abs(sh[1:]) <= 2.5e-3 * colour).all()


# ---- the context ---------------------------------------------------------------------------------------------------------------
def test_a_gather_leaves_the_context_untouched_and_is_deterministic():
    from micro_raytracer_amd import Sampler
    s = Sampler(seed=SEED, device=0)
    s.execute(_render(), n_samples=16)

    def state():
        acc, cnt = s.accum()
        return [acc, np.array(cnt), s.img()] + [v for _, v in sorted(s.aov().items())]

    before = state()
    a = s.gather(_render(), POS, NRM, n_dirs=65, n_samples=16, key_base=KEY_BASE)
    sh = s.gather(_render(), POS, n_dirs=65, n_samples=16, out="sh9", key_base=KEY_BASE)
    s.gather_rays(_render(), POS, NRM, n_dirs=65)
    after = state()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    s.execute(_render(), n_samples=16)
    assert s.accum()[1] == 32
    b = s.gather(_render(), POS, NRM, n_dirs=65, n_samples=16, key_base=KEY_BASE)
    assert G.same_bits(a, b) == 0 and G.same_bits(sh, s.gather(_render(), POS, n_dirs=65, n_samples=16, out="sh9", key_base=KEY_BASE)) == 0
    other = s.gather(_render(), POS, NRM, n_dirs=65, n_samples=16, key_base=KEY_BASE + 1)
    assert G.same_bits(a[[0, 1, 2, 3, 5, 6]], other[[0, 1, 2, 3, 5, 6]]) > 0
    s.close()


def test_a_row_sharded_context_serves_the_call(sampler):
    from micro_raytracer_amd import Sampler
    s = Sampler(seed=SEED, device=0, shard_index=1, shard_count=2, shard_rows=4)
    got = s.gather(_render(), POS, NRM, n_dirs=63, n_samples=16, key_base=KEY_BASE)
    s.close()
    assert G.same_bits(got, sampler.gather(_render(), POS, NRM, n_dirs=63, n_samples=16, key_base=KEY_BASE)) == 0


# ---- argument errors -----------------------------------------------------------------------------------------------------------
def _desc(points, normals, **kw):
    from micro_raytracer_amd import _abi
    g = _abi.Gather()
    g.n, g.pos, g.normal = points.shape[0], points.ctypes.data, None if normals is None else normals.ctypes.data
    g.n_dirs, g.n_samples, g.offset = 8, 16, 1e-4
    g.dist = _abi.GATHER_SPHERE if normals is None else _abi.GATHER_HEMI_COS
    for k, v in kw.items():
        if k == "reserved":
            g.reserved[v] = 1
        else:
            setattr(g, k, v)
    return g


BAD = {
    "n == 0": (False, dict(n=0)), "n == 2^30": (False, dict(n=1 << 30)), "n_dirs == 0": (False, dict(n_dirs=0)),
    "n_dirs == 65537": (False, dict(n_dirs=65537)), "n_samples == 0": (False, dict(n_samples=0)),
    "samples past 2^32 - 1": (False, dict(sample_base=0xffffffff, n_samples=1)), "unknown dist": (True, dict(dist=2)),
    "unknown out": (False, dict(out=2)), "unknown flag": (False, dict(flags=2)), "SH9 with HEMI_COS": (True, dict(out=1)),
    "HEMI_COS without normal": (False, dict(dist=1)), "SPHERE with normal": (True, dict(dist=0)), "offset NaN": (False, dict(offset=float("nan"))),
    "offset inf": (False, dict(offset=float("inf"))), "offset < 0": (True, dict(offset=-1e-6)), "reserved[0]": (False, dict(reserved=0)),
    "reserved[2]": (True, dict(reserved=2)), "null pos": (False, dict(pos=None)),
}


@pytest.mark.parametrize("what", list(BAD))
def test_every_argument_error_has_its_code_and_message(sampler, what):
    from micro_raytracer_amd import _abi, _lib
    L = _lib.lib()
    hemi, kw = BAD[what]
    g = _desc(POS, NRM if hemi else None, **kw)
    out = np.full((7, 9, 3), 7.0, f32)
    o, d, k = np.zeros((7, 8, 3), f32), np.zeros((7, 8, 3), f32), np.zeros((7, 8), np.uint32)
    assert L.mrt_gather(sampler._ctx, C.byref(g), out.ctypes.data, None) == _abi.MRT_ERR_ARG, what
    msg = L.mrt_last_error().decode()
    assert msg.startswith("mrt_gather: ") and len(msg) > 14 and L.mrt_last_status() == _abi.MRT_ERR_ARG, (what, msg)
    assert L.mrt_gather_rays(sampler._ctx, C.byref(g), 0, 1, o.ctypes.data, d.ctypes.data, k.ctypes.data) == _abi.MRT_ERR_ARG, what
    assert L.mrt_last_error().decode().startswith("mrt_gather_rays: "), what
    assert (out == 7.0).all() and not o.any() and not k.any()


def test_null_pointers_and_slices_past_the_end(sampler):
    from micro_raytracer_amd import _abi, _lib
    L = _lib.lib()
    g = _desc(POS, None)
    out = np.zeros((7, 3), f32)
    for args in ((None, C.byref(g), out.ctypes.data, None), (sampler._ctx, None, out.ctypes.data, None), (sampler._ctx, C.byref(g), None, None)):
        assert L.mrt_gather(*args) == _abi.MRT_ERR_ARG and L.mrt_last_error().decode().startswith("mrt_gather: null")
    o = np.zeros((7, 8, 3), f32)
    for first, count in ((0, 8), (7, 1), (8, 0), (2 ** 63, 2 ** 63)):
        assert L.mrt_gather_rays(sampler._ctx, C.byref(g), first, count, o.ctypes.data, None, None) == _abi.MRT_ERR_ARG
        assert "reach past n = 7" in L.mrt_last_error().decode()
    assert L.mrt_gather_rays(sampler._ctx, C.byref(g), 7, 0, o.ctypes.data, None, None) == 0           # an empty slice at the end is legal
    assert L.mrt_gather_rays(sampler._ctx, C.byref(g), 6, 1, None, None, None) == 0                   # ... and so is asking for nothing
    assert not o.any()
    # the good descriptor does pass
    assert L.mrt_gather(sampler._ctx, C.byref(g), out.ctypes.data, None) == 0 and np.isfinite(out).all() and out.any()
    with pytest.raises(_lib.MrtError, match="MRT_GATHER_SH9 needs MRT_GATHER_SPHERE"):
        sampler.gather(_render(), POS, NRM, out="sh9")


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def test_cli_gathers_the_points_of_a_file(sampler, tmp_path):
    from micro_raytracer_amd import __main__ as cli, scenes
    (tmp_path / "box.json").write_text(json.dumps(scenes.cornell_box(res=(16, 16), bounce=4)))
    good = [0, 1, 2, 3, 5, 6]
    np.save(tmp_path / "p6.npy", np.concatenate([POS, NRM], 1)[good])
    np.save(tmp_path / "p3.npy", POS)
    base = [str(tmp_path / "box.json"), "--seed", str(SEED), "--sample", "16"]
    cli.main(base + ["--gather", str(tmp_path / "p6.npy"), "--gather-out", str(tmp_path / "e.npy"), "--gather-dirs", "63"])
    cli.main(base + ["--gather", str(tmp_path / "p3.npy"), "--gather-out", str(tmp_path / "sh.npy"), "--gather-sh"])
    assert G.same_bits(np.load(tmp_path / "e.npy"), sampler.gather(_render(), POS[good], NRM[good], n_dirs=63, n_samples=16)) == 0
    assert G.same_bits(np.load(tmp_path / "sh.npy"), sampler.gather(_render(), POS, n_dirs=64, n_samples=16, out="sh9")) == 0
    with pytest.raises(SystemExit):
        cli.main(base + ["--gather", str(tmp_path / "p6.npy"), "--gather-out", str(tmp_path / "x.npy"), "--gather-sh"])
