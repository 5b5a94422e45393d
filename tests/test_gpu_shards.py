"""Row shards at every shard_rows, against the unsharded context of the same scene, seed and sample count, bit for bit.

The default of 8 rows per block is exactly the height of a wavefront's pixel tile: there a tile never straddles a block and
`blk = ry / shard_rows` of csrc/mrt_pt_kernel.h equals the tile row.  With any other value the 64 lanes of one wavefront map
to frame rows that lie shard_count blocks apart, and the partial last block ends in the middle of a tile.  The geometries of
tests/shard_cases.py run that way through every path that hangs off the layout: the kernel's row mapping, the chunk planes
of the sample split and their fold, the look-ahead planes, mrt_accum placing a shard's rows, set_accum on a shard, the
in-process group's row map and scatter, and ShardedSampler.  The unsharded context itself is held to the CPU oracle by
test_gpu_parity.test_scene_parity; one geometry is compared with the oracle here as an anchor.

Frames are 20 pixels wide (2.5 tiles: every tile row has a ragged tile) at ssaa 1.  Shards of one geometry run one after
another on one device, at most five contexts alive at a time."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import shard_cases as SC
from conftest import ROOT, make_holder

pytestmark = pytest.mark.gpu

W, SEED = 20, 7
TOL = 1e-4                                      # the suite's bar against the oracle (mean radiance, L-inf)

_REF = {}


def _scene(nh, spp):
    from micro_raytracer_amd import scenes
    return scenes.cornell_box2(res=(W, nh), ssaa=1, sample=spp)


def _ref(nh, spp):
    """(render, whole frame) of the unsharded context: rendered once per (height, sample count), never written to."""
    from micro_raytracer_amd import Sampler
    if (nh, spp) not in _REF:
        render, _ = make_holder(_scene(nh, spp))
        s = Sampler(seed=SEED)
        s.execute(render, n_samples=spp)
        whole, cnt = s.accum()
        assert cnt == spp and (s.nw, s.nh) == (W, nh)
        s.close()
        whole.setflags(write=False)
        _REF[(nh, spp)] = (render, whole)
    return _REF[(nh, spp)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _read_device(ptr, nbytes):
    """Device memory as f32, through the HIP runtime the library itself is bound to (as test_image_path.DeviceBuffer reads)."""
    from micro_raytracer_amd import _lib
    _lib.lib()
    hip = C.CDLL(_lib.LIB_PATH)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipDeviceSynchronize() == 0
    out = np.empty(nbytes // 4, np.float32)
    assert hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2) == 0              # hipMemcpyDeviceToHost
    return out


def _accum_into_nan(s):
    """mrt_accum into a NaN-filled frame: (frame, count)."""
    from micro_raytracer_amd import _lib
    out = np.full((s.nh, s.nw, 3), np.nan, np.float32)
    cnt = C.c_uint32()
    _lib.check(_lib.lib().mrt_accum(s._ctx, out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(cnt)))
    return out, cnt.value


def _check_shard(s, nh, count, sr, r, spp, whole):
    """Everything a finished shard must satisfy; returns (rows, its rows' sums)."""
    want_rows = SC.brute_rows(nh, count, sr, r)
    pr = SC.brute_padded(nh, count, sr)
    loc, rows = s.accum_local()
    assert rows.tolist() == want_rows and s.local_rows == len(want_rows), (nh, count, sr, r, rows.tolist())
    assert s.padded_rows() == pr, (nh, count, sr, r, s.padded_rows(), pr)
    assert np.array_equal(_bits(loc), _bits(whole[want_rows])), (nh, count, sr, r)
    # mrt_accum: this shard's rows in their places, foreign rows untouched, the count also from a shard without rows
    frame, cnt = _accum_into_nan(s)
    assert cnt == spp
    foreign = np.ones(nh, bool)
    foreign[want_rows] = False
    assert np.isnan(frame[foreign]).all() and np.array_equal(_bits(frame[want_rows]), _bits(whole[want_rows])), (nh, count, sr, r)
    # the device plane: padded_rows rows, the shard's rows first, exact zeros behind them
    ptr, nbytes = s.accum_device_ptr()
    assert nbytes == pr * W * 12
    plane = _read_device(ptr, nbytes).reshape(pr, W, 3)
    assert np.array_equal(_bits(plane[:len(want_rows)]), _bits(loc))
    assert not _bits(plane[len(want_rows):]).any(), (nh, count, sr, r)
    return want_rows, loc


def _run_geometry(nh, count, sr, spp, indices=None, env_check=None):
    """Every shard of a geometry (or the listed ones), one after another; the union must be the unsharded frame, each row once."""
    from micro_raytracer_amd import Sampler
    render, whole = _ref(nh, spp)
    out = np.full_like(whole, np.nan)
    seen = np.zeros(nh, int)
    shards = {}
    for r in (range(count) if indices is None else indices):
        s = Sampler(seed=SEED, shard_index=r, shard_count=count, shard_rows=sr)
        s.execute(render, n_samples=spp)
        if env_check is not None:
            env_check(s.stats(), bool(SC.brute_rows(nh, count, sr, r)))
        rows, loc = _check_shard(s, nh, count, sr, r, spp, whole)
        s.close()
        out[rows] = loc
        seen[rows] += 1
        shards[r] = (rows, loc)
    assert (seen == 1).all(), (nh, count, sr, seen.tolist())
    assert np.array_equal(_bits(out), _bits(whole)), (nh, count, sr)
    return shards


@pytest.mark.parametrize("nh,count,sr", SC.GEOMETRIES, ids=lambda v: str(v))
def test_shards_of_every_geometry_tile_the_unsharded_frame(nh, count, sr):
    _run_geometry(nh, count, sr, 3)


def test_anchor_a_straddling_geometry_against_the_oracle(oracle_mod):
    """(23 rows, 3 shards, 5-row blocks) assembled from its shards, against the CPU oracle at the suite's bar."""
    nh, count, sr, spp = 23, 3, 5, 3
    shards = _run_geometry(nh, count, sr, spp)
    got = np.zeros((nh, W, 3), np.float32)
    for rows, loc in shards.values():
        got[rows] = loc
    _, holder = make_holder(_scene(nh, spp))
    o = oracle_mod.Oracle(holder, seed=SEED)
    o.execute(spp)
    ref, _ = o.accum()
    o.close()
    err = float(np.max(np.abs(got - ref))) / spp
    print(f"sharded frame vs oracle: L-inf of the mean {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("nh,count,sr,indices,like", SC.OVERFLOW, ids=["rows_2p32m1", "count_2p32m1_rows8", "count_2p32m1_rows9"])
def test_inputs_whose_32_bit_sums_wrapped_render_like_their_clamped_geometry(nh, count, sr, indices, like):
    """shard_rows = 2^32 - 1 and shard_count = 2^32 - 1: (nh + shard_rows - 1) and (n_blocks + shard_count - 1) wrapped to
    padded_rows = 0 under local_rows > 0.  tests/test_shard_layout_host.py holds local_rows <= padded_rows for exactly these
    inputs on the host; here they render like shard_rows = 9, respectively like 5 shards most of which are empty."""
    big = _run_geometry(nh, count, sr, 3, indices=indices)
    small = _run_geometry(*like, 3)
    for i, r in enumerate(indices):
        rows, loc = big[r]
        srows, sloc = small[min(i, like[1] - 1)]
        assert rows == srows and np.array_equal(_bits(loc), _bits(sloc)), (count, sr, r)
    assert len(big[indices[0]][0]) > 0


SHAPES = [("MRT_K_SPLIT", "1"), ("MRT_K_SPLIT", "4"), ("MRT_NO_PERSIST", "1"), ("MRT_BLOCK_THREADS", "64"),
          ("MRT_BLOCK_THREADS", "1024"), ("MRT_SCENE_IN_L2", "1"), ("MRT_MAX_CHUNKS", "1")]


@pytest.mark.parametrize("knob,value", SHAPES, ids=[f"{k}={v}" for k, v in SHAPES])
def test_launch_shapes_on_straddling_shards_give_the_same_bits(knob, value, monkeypatch):
    """40 samples (two whole 16-sample chunks and a partial one) on three straddling geometries of 23 rows, under every launch
    shape: forced lanes per pixel (the chunk planes [padded_rows][nw][3] and their fold over local_rows rows), plain grids,
    one-wavefront and sixteen-wavefront workgroups, the scene read through L2, one chunk per launch.  The reference is the
    unsharded context under no switch."""
    spp = 40
    for nh, _, _ in SC.SHAPE_GEOMETRIES:
        _ref(nh, spp)                                        # rendered before the switch is set
    monkeypatch.setenv(knob, value)

    def check(st, has_rows):
        if not has_rows:
            return
        if knob == "MRT_K_SPLIT":                            # 3 chunks: a forced split is halved until it is no more than the chunks
            assert st["k_split"] == {"1": 1, "4": 2}[value], st
        if knob == "MRT_BLOCK_THREADS":
            assert st["block_threads"] == int(value), st
        if knob == "MRT_SCENE_IN_L2":
            assert st["scene_in_lds"] == 0, st
        if knob == "MRT_MAX_CHUNKS":
            assert st["launches"] > 1, st
    for nh, count, sr in SC.SHAPE_GEOMETRIES:
        _run_geometry(nh, count, sr, spp, env_check=check)


def test_four_lanes_per_pixel_on_a_straddling_shard(monkeypatch):
    """72 samples are five chunks, so MRT_K_SPLIT=4 is taken as it stands (at 40 samples it is halved to 2)."""
    nh, count, sr, spp = 23, 3, 5, 72
    _ref(nh, spp)
    monkeypatch.setenv("MRT_K_SPLIT", "4")

    def check(st, has_rows):
        assert not has_rows or st["k_split"] == 4, st
    _run_geometry(nh, count, sr, spp, env_check=check)


def test_per_call_loop_on_shards_of_three_row_blocks():
    """12 one-sample calls on every shard of (23 rows, 3 shards, 3-row blocks): with the look-ahead (planes of padded_rows
    rows, folded over local_rows rows), without it, deferred, and into a caller-bound accumulator of padded_rows * nw * 12
    bytes.  All equal the batched shard, which equals the unsharded frame's rows."""
    from micro_raytracer_amd import Sampler, _abi
    from test_image_path import DeviceBuffer
    nh, count, sr, spp = 23, 3, 3, 12
    render, whole = _ref(nh, spp)
    batched = _run_geometry(nh, count, sr, spp)
    pr = SC.brute_padded(nh, count, sr)
    for r in range(count):
        rows, want = batched[r]
        for mode, flags in (("look-ahead", 0), ("no look-ahead", _abi.FLAG_NO_LOOKAHEAD), ("defer", _abi.FLAG_DEFER), ("bound", 0)):
            s = Sampler(seed=SEED, shard_index=r, shard_count=count, shard_rows=sr, flags=flags).create(render)
            buf = None
            if mode == "bound":
                assert s.padded_rows() == pr
                buf = DeviceBuffer(pr * W * 12, fill=7.0)
                s.bind_accum(buf.ptr.value, buf.nbytes)
            for _ in range(spp):
                s.execute(render)
            loc, got_rows = s.accum_local()
            assert got_rows.tolist() == rows and s.accum()[1] == spp, (mode, r)
            assert np.array_equal(_bits(loc), _bits(want)), (mode, r)
            if mode == "look-ahead":
                assert s.stats()["launches"] == 1                    # the calls were served from planes traced ahead
            if buf is not None:
                buf.synchronize()
                plane = buf.read().reshape(pr, W, 3)
                assert np.array_equal(_bits(plane[:len(rows)]), _bits(want)) and not _bits(plane[len(rows):]).any(), r
            s.close()
            if buf is not None:
                buf.free()


def test_mesh_scene_behind_the_staged_scene_on_five_row_blocks(monkeypatch):
    """600 triangles, 24 x 23, 2 samples, 3 shards of 5-row blocks on the deep staging level (MRT_COLD=1, MRT_DEEP_NODES=40):
    the walk area behind the staged scene with shard-mapped rows.  The reference is the unsharded context under the same
    switches (every staging level gives the same bits: test_gpu_parity)."""
    from micro_raytracer_amd import Sampler, scenes
    from micro_raytracer_amd._abi import F_COLD, F_DEEP
    monkeypatch.setenv("MRT_COLD", "1")
    monkeypatch.setenv("MRT_DEEP_NODES", "40")
    render, _ = make_holder(scenes.mesh_scene(res=(24, 23), sample=2, n_tris=600))
    w = Sampler(seed=SEED)
    w.execute(render, n_samples=2)
    whole, _ = w.accum()
    assert w.stats()["kernel_features"] & F_DEEP and (w.nw, w.nh) == (24, 23)
    w.close()
    nh, count, sr = 23, 3, 5
    out = np.full_like(whole, np.nan)
    for r in range(count):
        s = Sampler(seed=SEED, shard_index=r, shard_count=count, shard_rows=sr)
        s.execute(render, n_samples=2)
        st = s.stats()
        assert st["kernel_features"] & F_COLD and st["kernel_features"] & F_DEEP, st
        loc, rows = s.accum_local()
        assert rows.tolist() == SC.brute_rows(nh, count, sr, r) and s.padded_rows() == SC.brute_padded(nh, count, sr)
        out[rows] = loc
        s.close()
    assert np.array_equal(_bits(out), _bits(whole))


def test_observations_on_a_shard_of_three_row_blocks():
    """AOVs and mrt_radiance do not depend on the shard; the image, the float image and the denoiser need the whole frame:
    MRT_ERR_STATE before set_accum, the unsharded outputs after it; an adaptive render is refused on a shard at any time."""
    from micro_raytracer_amd import MrtError, Sampler, _abi
    nh, count, sr, spp = 23, 3, 3, 3
    render, whole = _ref(nh, spp)
    plain = Sampler(seed=SEED)
    plain.execute(render, n_samples=spp)
    s = Sampler(seed=SEED, shard_index=1, shard_count=count, shard_rows=sr)
    s.execute(render, n_samples=spp)

    def refused(fn):
        with pytest.raises(MrtError) as e:
            fn()
        assert e.value.code == _abi.MRT_ERR_STATE, e.value
    for fn in (s.img, s.img_hdr, s.denoise):
        refused(fn)
    refused(lambda: s.execute_adaptive(render, 0.0, min_samples=32, max_samples=64, step=16))
    pa, sa = plain.aov(), s.aov()
    assert set(pa) == set(sa)
    for k in pa:
        assert np.array_equal(pa[k].view(np.uint32), sa[k].view(np.uint32)), k
    orig, dirs = plain.camera_rays(render)
    orig, dirs = orig.reshape(-1, 3)[80:380], dirs.reshape(-1, 3)[80:380]              # 300 rays
    assert np.array_equal(_bits(plain.radiance(render, orig, dirs, 2)), _bits(s.radiance(render, orig, dirs, 2)))
    s.set_accum(whole, spp)
    assert np.array_equal(s.img(), plain.img())
    assert np.array_equal(_bits(s.img_hdr()), _bits(plain.img_hdr()))
    assert np.array_equal(_bits(s.denoise()), _bits(plain.denoise()))
    refused(lambda: s.execute_adaptive(render, 0.0, min_samples=32, max_samples=64, step=16))
    # the shard's own rows are still its own
    loc, rows = s.accum_local()
    assert rows.tolist() == SC.brute_rows(nh, count, sr, 1) and np.array_equal(_bits(loc), _bits(whole[rows]))
    s.close()
    plain.close()


_GROUP_SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["MRT_ROOT"]); sys.path.insert(0, os.path.join(os.environ["MRT_ROOT"], "tests"))
import shard_cases as SC
from micro_raytracer_amd import Sampler, _lib, load_render, scenes
nh, W, spp = 23, 20, 20
render = load_render(scenes.cornell_box2(res=(W, nh), ssaa=1, sample=spp))
plain = Sampler(seed=7)
plain.execute(render, n_samples=16)
plain.execute(render, n_samples=4)
ref, cnt = plain.accum()
img = plain.img()
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)

def group(n, sr, resume):
    g = Sampler(seed=7, n_devices=n, shard_rows=sr)
    g.execute(render, n_samples=16)
    g.execute(render, n_samples=4)
    got, gcnt = g.accum()
    assert gcnt == cnt == spp and np.array_equal(bits(got), bits(ref)), (n, sr)
    assert np.array_equal(g.img(), img), (n, sr)
    loc, rows = g.accum_local()
    assert list(rows) == list(range(nh)) and np.array_equal(bits(loc), bits(ref)), (n, sr)
    assert g.padded_rows() == nh
    if resume:
        g.reset()
        assert not g.accum()[0].any()
        g.set_accum(ref, cnt)
        g.execute(render, n_samples=12)
        assert np.array_equal(bits(g.accum()[0]), bits(resumed)), (n, sr)
    g.close()

os.environ["MRT_FORCE_RCCL"] = "1"
for sr in (3, 1000):
    group(1, sr, False)
print("GROUP-ONE-OK")
ndev = _lib.lib().mrt_device_count()
if ndev >= 2:
    del os.environ["MRT_FORCE_RCCL"]
    plain.execute(render, n_samples=12)
    resumed = plain.accum()[0]
    n = min(ndev, 3)
    for sr in (3, 13, nh + 1):
        assert SC.brute_padded(nh, n, sr) > len(SC.brute_rows(nh, n, sr, n - 1))        # the row map has padding to skip
        group(n, sr, True)
    print("GROUP-MULTI-OK", n)
else:
    print("GROUP-MULTI-SKIPPED", ndev)
"""

_GROUP_OUT = {}


def _group_run():
    if "out" not in _GROUP_OUT:
        env = dict(os.environ, MRT_ROOT=ROOT)
        _GROUP_OUT["out"] = subprocess.run([sys.executable, "-c", _GROUP_SCRIPT], capture_output=True, text=True, timeout=300, env=env)
    return _GROUP_OUT["out"]


def test_group_context_on_one_device_with_other_block_heights():
    """mrt_opts.n_devices = 1 under MRT_FORCE_RCCL with shard_rows 3 and 1000 (clamped to the frame's 23 rows): frame, image
    and the group's own rows equal the plain context.  A fresh interpreter without torch, like its sibling in test_gpu_dist."""
    out = _group_run()
    assert "GROUP-ONE-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]


def test_group_context_on_several_devices_row_map_padding_and_scatter():
    """n_devices = min(visible, 3) with shard_rows 3, 13 and nh + 1 on 23 rows: the first run of the row map's padding and of
    scatter_rows with rows to skip; frame, image, accum_local, and reset + set_accum + 12 more samples against the plain
    context.  Needs two visible devices (the same child process as the one-device part)."""
    out = _group_run()
    if "GROUP-MULTI-SKIPPED" in out.stdout:
        pytest.skip("one visible HIP device: the multi-device group needs at least two (" + out.stdout.strip().splitlines()[-1] + ")")
    assert out.returncode == 0 and "GROUP-MULTI-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
