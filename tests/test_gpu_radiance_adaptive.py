"""mrt_radiance_adaptive on the GPU: tile-adaptive sampling and the variance-guided denoiser on caller-supplied rays.

1. the frame yardstick: on the camera's own rays (aprt 0) the call leaves the bits of mrt_execute_adaptive;
2. the mrt_radiance yardstick on rays no camera forms: per stop count the bits of mrt_radiance, the half buffer as the fold of the
   even rounds' chunk sums, the stop decisions recomputed in numpy;
3. the result does not depend on the launch shape;
4. the state the call leaves and what it refuses;
5. MRT_DN_VARIANCE: which pairs of adaptive state and AOV planes serve;
6. quality of a variance-denoised panorama (figures in DESIGN.md §21);
7. the CLI's --pano-adaptive.

Where the issue's figures are not legal input the nearest legal ones stand in: min_samples is a multiple of 2 * step (mrt_adapt's
rule), so the step-32 runs take min 64 and max 128 where the step-16 runs take min 32 and max 64."""
import json

import numpy as np
import pytest

from micro_raytracer_amd import Sampler, _abi, _lib, cameras, load_render, scenes
from test_adaptive_host import np_tile_errors
from test_denoise_host import same_bits, tonemapped

pytestmark = pytest.mark.gpu
f32 = np.float32
SEED = 5
RES = (44, 36)                        # 6 x 5 tiles, ragged in both axes


def _render(name, res=RES, sample=64):
    desc = scenes.cornell_box(res=res, sample=sample, bounce=8) if name == "cornell" else scenes.mesh_scene(res=res, sample=sample, bounce=6)
    desc["frame"]["cam"]["aprt"] = 0
    return load_render(desc)


def _state(s, info):
    A, cnt = s.accum()
    return dict(A=A, cnt=cnt, H=s.adapt_half(), counts=s.sample_counts(), info=info)


def _frame(render, thr, step, seed=SEED, keep=False):
    s = Sampler(seed=seed, device=0)
    r = _state(s, s.execute_adaptive(render, thr, min_samples=2 * step, max_samples=4 * step, step=step))
    if keep:
        r["s"] = s
    else:
        s.close()
    return r


def _rays(render, o, d, thr, step, seed=SEED, keep=False, flags=0, lo=None, hi=None):
    s = Sampler(seed=seed, device=0, flags=flags)
    r = _state(s, s.radiance_adaptive(render, o, d, thr, min_samples=lo or 2 * step, max_samples=hi or 4 * step, step=step))
    if keep:
        r["s"] = s
    else:
        s.close()
    return r


def _median(r, n):
    et, nan, _ = np_tile_errors(r["A"], r["H"], n, 0.0)
    return float(np.median(et[~nan]))


INFO_KEYS = ("samples", "rounds", "launches", "tiles", "tiles_converged", "min_count", "max_count")


def _assert_same(a, b, label):
    assert same_bits(a["A"], b["A"]) == 0, label
    assert same_bits(a["H"], b["H"]) == 0, label
    assert np.array_equal(a["counts"], b["counts"]) and a["cnt"] == b["cnt"], label
    assert {k: a["info"][k] for k in INFO_KEYS} == {k: b["info"][k] for k in INFO_KEYS}, label


def _kernel(render, o, d):
    """What mrt_radiance reports it runs on a context of the current environment: the dispatch mrt_radiance_adaptive shares."""
    s = Sampler(seed=SEED, device=0).create(render)
    info = {}
    s.radiance(render, o[:1, :8], d[:1, :8], 1, info=info)
    s.close()
    return info["kernel_features"], info["scene_in_lds"]


# ---- 1: the frame yardstick --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [16, 32])
@pytest.mark.parametrize("name", ["cornell", "mesh"])
def test_camera_rays_give_the_bits_of_execute_adaptive(name, step, monkeypatch):
    render = _render(name, sample=4 * step)
    thr = _median(_frame(render, float("inf"), step), 2 * step)
    want = _frame(render, thr, step)
    assert want["info"]["min_count"] < want["info"]["max_count"], want["info"]
    c = Sampler(seed=SEED, device=0)
    o, d = c.camera_rays(render)
    c.close()
    got = _rays(render, o, d, thr, step)
    _assert_same(got, want, (name, step))
    staged = _kernel(render, o, d)
    with monkeypatch.context() as mp:
        mp.setenv("MRT_SCENE_IN_L2", "1")
        _assert_same(_rays(render, o, d, thr, step), want, (name, step, "L2"))
        through_l2 = _kernel(render, o, d)
    assert through_l2[0] == staged[0] and through_l2[1] == 0, (staged, through_l2)
    if name == "cornell":
        assert staged[1] == 1                     # the small scene is staged: the two runs took different kernels


# ---- 2: the mrt_radiance yardstick -------------------------------------------------------------------------------------------------
def test_equirect_rays_hold_the_bits_of_radiance_and_the_rule():
    step, lo, hi = 16, 32, 64
    render = _render("cornell", res=(40, 20), sample=hi)
    u = Sampler(seed=SEED, device=0).create(render)
    o, d = cameras.equirect(render.frame.cam.pos, u.nw, u.nh)
    chunk = [u.radiance(render, o, d, 16, sample_base=16 * j) for j in range(hi // 16)]
    whole = {n: u.radiance(render, o, d, n) for n in range(lo, hi + 1, 2 * step)}
    u.close()
    thr = _median(_rays(render, o, d, float("inf"), step), lo)
    r = _rays(render, o, d, thr, step)
    counts, info = r["counts"], r["info"]
    stops = sorted(np.unique(counts).tolist())
    assert stops == [lo, hi] and info["min_count"] == lo and info["max_count"] == hi and r["cnt"] == lo
    assert info["samples"] == int(counts.astype(np.int64).sum()) and info["tiles"] == 5 * 3
    half = {}
    for n in stops:
        m = counts == n
        assert same_bits(r["A"][m], whole[n][m]) == 0, n
        h = np.zeros_like(chunk[0])
        for j in range(0, n // 16, 2):                # step 16: round j is chunk j, the even rounds are the even chunks
            h = h + chunk[j]
        half[n] = h
        assert same_bits(r["H"][m], h[m]) == 0, n
    # the stop decisions, recomputed at the one evaluation point below the cap from mrt_radiance's sums
    _, nan, conv = np_tile_errors(whole[lo], half[lo], lo, thr)
    tc = counts[::8, ::8]
    assert np.array_equal(tc == lo, conv) and not nan.any()
    assert info["tiles_converged"] >= int(conv.sum())


# ---- 3: launch shapes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [16, 64])
def test_independent_of_the_launch_shape(step, monkeypatch):
    """MRT_K_SPLIT 1, 2, 4 at rounds of one chunk (odd rounds in place, even rounds through two planes of which one phase idles)
    and of four chunks (in place / two / four phases)."""
    render = _render("cornell", sample=4 * step)
    c = Sampler(seed=SEED, device=0).create(render)
    o, d = cameras.equirect(render.frame.cam.pos, c.nw, c.nh)
    c.close()
    thr = _median(_rays(render, o, d, float("inf"), step), 2 * step)
    base = _rays(render, o, d, thr, step)
    assert base["info"]["min_count"] < base["info"]["max_count"]
    seen = set()
    for ks in ("1", "2", "4"):
        with monkeypatch.context() as mp:
            mp.setenv("MRT_K_SPLIT", ks)
            r = _rays(render, o, d, thr, step, keep=True)
            seen.add(r["s"].stats()["k_split"])
            r["s"].close()
            for k in ("A", "H", "counts"):
                assert np.array_equal(r[k].view(np.uint32), base[k].view(np.uint32)), (ks, k)
    assert seen == ({2} if step == 16 else {2, 4}), seen          # (even rounds always go through at least two planes)
    if step == 16:
        return
    # rounds of four chunks cut into two launches each
    wide = _rays(render, o, d, float("inf"), 64, lo=128, hi=128)
    with monkeypatch.context() as mp:
        mp.setenv("MRT_K_SPLIT", "2")
        mp.setenv("MRT_MAX_CHUNKS", "2")
        cut = _rays(render, o, d, float("inf"), 64, lo=128, hi=128)
    assert cut["info"]["rounds"] == 2 and cut["info"]["launches"] == 4 and wide["info"]["launches"] < 4
    assert same_bits(cut["A"], wide["A"]) == 0 and same_bits(cut["H"], wide["H"]) == 0


@pytest.mark.parametrize("thr", [0.0, float("inf"), None])
def test_four_tiles_three_of_them_slivers(thr, monkeypatch):
    """9 x 9: one full tile, one of a single column, one of a single row, one of a single pixel -- lanes outside the frame in three
    of four wavefronts; at the median threshold (None) the later rounds list fewer than four tiles, so the last workgroup has
    wavefronts past the list."""
    render = _render("cornell", res=(9, 9))
    if thr is None:
        thr = _median(_frame(render, float("inf"), 16), 32)
    want = _frame(render, thr, 16)
    if thr not in (0.0, float("inf")):
        assert want["info"]["min_count"] < want["info"]["max_count"]
    c = Sampler(seed=SEED, device=0)
    o, d = c.camera_rays(render)
    c.close()
    _assert_same(_rays(render, o, d, thr, 16), want, thr)
    for ks in ("1", "4"):
        with monkeypatch.context() as mp:
            mp.setenv("MRT_K_SPLIT", ks)
            r = _rays(render, o, d, thr, 16)
        assert same_bits(r["A"], want["A"]) == 0 and same_bits(r["H"], want["H"]) == 0 and np.array_equal(r["counts"], want["counts"]), ks
    if thr == float("inf"):
        assert (want["counts"] == 32).all()


# ---- 4: state ----------------------------------------------------------------------------------------------------------------------
def _raises(code, fn):
    with pytest.raises(_lib.MrtError) as e:
        fn()
    assert e.value.code == code, e.value
    return e.value.msg


def test_state_after_the_call_and_what_it_refuses():
    step = 16
    render = _render("cornell", sample=64)
    thr = _median(_frame(render, float("inf"), step), 32)
    want = _frame(render, thr, step, keep=True)
    o, d = want["s"].camera_rays(render)
    got = _rays(render, o, d, thr, step, keep=True)
    s = got["s"]
    assert np.array_equal(s.img(), want["s"].img()) and np.array_equal(s.img_ss(), want["s"].img_ss())      # per-tile counts in the tone map
    assert same_bits(s.img_hdr(), want["s"].img_hdr()) == 0
    assert s.stats()["samples"] == got["info"]["samples"] and s.stats()["launches"] == got["info"]["launches"]
    want["s"].close()
    msg = _raises(_abi.MRT_ERR_STATE, lambda: s.execute(render, n_samples=1))
    assert "adaptive" in msg
    # a second adaptive call on a context that holds samples: refused, nothing changes
    _raises(_abi.MRT_ERR_STATE, lambda: s.radiance_adaptive(render, o, d, thr, min_samples=32, max_samples=64, step=step))
    again = _state(s, got["info"])
    _assert_same(again, got, "after a refusal")
    s.reset()
    A, cnt = s.accum()
    assert cnt == 0 and not A.any() and (s.sample_counts() == 0).all()
    _raises(_abi.MRT_ERR_STATE, s.adapt_half)
    s.execute(render, n_samples=4)                   # an empty uniform context again
    u = Sampler(seed=SEED, device=0)
    u.execute(render, n_samples=4)
    assert same_bits(s.accum()[0], u.accum()[0]) == 0 and s.accum()[1] == 4
    # ... which now holds samples
    A0 = s.accum()[0]
    _raises(_abi.MRT_ERR_STATE, lambda: s.radiance_adaptive(render, o, d, thr, min_samples=32, max_samples=64, step=step))
    assert same_bits(s.accum()[0], A0) == 0 and s.accum()[1] == 4
    s.close()
    # samples booked under MRT_FLAG_DEFER
    b = Sampler(seed=SEED, device=0, flags=_abi.FLAG_DEFER)
    b.execute(render, n_samples=4)
    _raises(_abi.MRT_ERR_STATE, lambda: b.radiance_adaptive(render, o, d, thr, min_samples=32, max_samples=64, step=step))
    assert same_bits(b.accum()[0], u.accum()[0]) == 0 and b.accum()[1] == 4
    b.close()
    u.close()
    # a row shard
    sh = Sampler(seed=SEED, device=0, shard_index=0, shard_count=2).create(render)
    msg = _raises(_abi.MRT_ERR_STATE, lambda: sh.radiance_adaptive(render, o, d, thr, min_samples=32, max_samples=64, step=step))
    assert "sharded" in msg
    sh.close()


def test_argument_errors():
    import ctypes as C
    render = _render("cornell", res=(16, 16))
    s = Sampler(seed=1, device=0).create(render)
    o, d = s.camera_rays(render)
    L = _lib.lib()

    def call(ctx=True, orig=True, dir=True, lo=32, hi=64, step=16, thr=0.5, flags=0, reserved=(0, 0, 0)):
        r = _abi.RaysAdapt()
        r.orig = o.ctypes.data if orig else None
        r.dir = d.ctypes.data if dir else None
        r.rule.min_samples, r.rule.max_samples, r.rule.step, r.rule.threshold = lo, hi, step, thr
        r.flags = flags
        for i, v in enumerate(reserved):
            r.reserved[i] = v
        return L.mrt_radiance_adaptive(s._ctx if ctx else None, C.byref(r), None, None)

    bad = [dict(ctx=False), dict(orig=False), dict(dir=False), dict(step=0), dict(step=8), dict(step=24), dict(lo=0), dict(lo=48), dict(hi=0),
           dict(hi=80), dict(lo=64, hi=32), dict(thr=-1.0), dict(thr=float("nan")), dict(flags=2), dict(flags=0x80000001), dict(reserved=(1, 0, 0)),
           dict(reserved=(0, 0, 7))]
    for kw in bad:
        assert call(**kw) == _abi.MRT_ERR_ARG, kw
        assert L.mrt_last_error().decode().startswith("mrt_radiance_adaptive:"), kw
    assert L.mrt_radiance_adaptive(s._ctx, None, None, None) == _abi.MRT_ERR_ARG
    A, cnt = s.accum()
    assert cnt == 0 and not A.any()                  # the refusals left the empty context empty
    assert call() == _abi.MRT_OK                     # ... and usable
    assert s.accum()[1] in (32, 64)
    s.close()


_DEVICE_SCRIPT = r"""
import sys
import numpy as np
import torch
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)                      # torch brings the HIP runtime up first, as in bench.py and dist.ShardedSampler
sys.path[:0] = sys.argv[1:3]
from micro_raytracer_amd import Sampler, cameras, load_render, scenes
from test_adaptive_host import np_tile_errors
from test_denoise_host import same_bits
desc = scenes.cornell_box(res=(44, 36), sample=64)
render = load_render(desc)


def run(o, d, thr):
    s = Sampler(seed=5, device=0)
    info = s.radiance_adaptive(render, o, d, thr, min_samples=32, max_samples=64, step=16)
    out = s.accum()[0], s.adapt_half(), s.sample_counts(), info
    s.close()
    return out


o, d = cameras.equirect(render.frame.cam.pos, 44, 36)
A, H, _, _ = run(o, d, float("inf"))
et, nan, _ = np_tile_errors(A, H, 32, 0.0)
thr = float(np.median(et[~nan]))
host = run(o, d, thr)
assert host[3]["min_count"] < host[3]["max_count"]
to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
got = run(to, td, thr)
assert same_bits(got[0], host[0]) == 0 and same_bits(got[1], host[1]) == 0 and np.array_equal(got[2], host[2])
assert np.array_equal(to.cpu().numpy(), o) and np.array_equal(td.cpu().numpy(), d)       # borrowed, not written
for bad in ((to, d), (o[:-1], d[:-1]), (to[:-1], td[:-1])):
    try:
        run(*bad, thr)
    except ValueError:
        pass
    else:
        raise AssertionError("mixed or mis-shaped rays were accepted")
print("DEVICE-OK")
"""


def test_device_tensors_give_the_bits_of_host_arrays():
    """Torch tensors on the context's device (MRT_RAYS_DEVICE) against the host path.  In a child process, as the device tests of
    tests/test_gpu_rays.py and tests/test_gpu_aov_rays.py: torch has to bring the HIP runtime up before the library does."""
    import os
    import subprocess
    import sys
    pytest.importorskip("torch")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _DEVICE_SCRIPT, os.path.dirname(here), here], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and "DEVICE-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- 5: variance mode --------------------------------------------------------------------------------------------------------------
def test_variance_mode_serves_the_matching_pairs_only():
    render = _render("cornell", res=(40, 36), sample=32)
    f = Sampler(seed=3, device=0)
    f.execute_adaptive(render, 0.0, min_samples=32, max_samples=32, step=16)
    want = f.denoise(mode="variance")                                    # frame state, the camera's planes: serves
    o, d = f.camera_rays(render)
    f.aov_rays(render, o, d)
    msg = _raises(_abi.MRT_ERR_STATE, lambda: f.denoise(mode="variance"))       # frame state, supplied planes: as before
    assert "mrt_aov_rays(ctx, NULL, NULL, 0)" in msg and "half buffer" in msg
    f.close()
    s = Sampler(seed=3, device=0)
    s.radiance_adaptive(render, o, d, 0.0, min_samples=32, max_samples=32, step=16)
    for fn in (lambda: s.denoise(mode="variance"), lambda: s.img_denoised(mode="variance"), lambda: s.img_hdr(denoise=dict(mode="variance"))):
        msg = _raises(_abi.MRT_ERR_STATE, fn)                                   # supplied state, no planes installed
        assert "mrt_aov_rays" in msg and "half buffer" in msg
    s.aov()                                                              # ... nor with the camera's own computed
    _raises(_abi.MRT_ERR_STATE, lambda: s.denoise(mode="variance"))
    assert s.denoise().shape == (36, 40, 3)                              # the a-trous mode serves either way
    s.aov_rays(render, o, d)
    got = s.denoise(mode="variance")                                     # supplied state, supplied planes: serves
    assert same_bits(got, want) == 0                                     # the camera's own rays: the frame path's bytes
    s.aov_rays(render, None, None)
    _raises(_abi.MRT_ERR_STATE, lambda: s.denoise(mode="variance"))
    # back in the uniform state the flag is gone: a frame-adaptive render on the same context serves the camera's planes
    s.reset()
    s.execute_adaptive(render, 0.0, min_samples=32, max_samples=32, step=16)
    assert same_bits(s.denoise(mode="variance"), want) == 0
    s.close()


def test_variance_mode_on_a_wrapped_equirect_grid():
    passes = 3
    render = _render("cornell", res=(80, 24), sample=32)
    s = Sampler(seed=4, device=0)
    cameras.render_equirect(s, render, guides=True, adaptive=dict(threshold=0.0))
    on = s.denoise(mode="variance", passes=passes)
    o, d = cameras.equirect(render.frame.cam.pos, s.nw, s.nh)
    s.aov_rays(render, o, d)
    off = s.denoise(mode="variance", passes=passes)
    nw = s.nw
    s.close()
    assert np.isfinite(on).all() and np.isfinite(off).all()
    reach = 2 ** (passes + 1)
    assert nw - 2 * reach > 0
    assert same_bits(on[:, reach:nw - reach], off[:, reach:nw - reach]) == 0


# ---- 6: quality --------------------------------------------------------------------------------------------------------------------
def test_quality_of_a_variance_denoised_panorama():
    """Equirect 64x32 inside the Cornell box, 32 spp against 512 spp of another seed, tone-mapped RMSE.  Measured on an MI355X
    (DESIGN.md §21); asserted: the variance-denoised error is below the raw one, and the adaptive run at the median threshold
    traces fewer samples than the uniform cap."""
    render = _render("cornell", res=(64, 32), sample=32)
    cam = render.frame.cam
    gt = Sampler(seed=1001, device=0).create(render)
    o, d = cameras.equirect(cam.pos, gt.nw, gt.nh)
    G = gt.radiance(render, o, d, 512)
    gt.close()
    s = Sampler(seed=7, device=0)
    A = cameras.render_equirect(s, render, 32, guides=True, adaptive=dict(threshold=0.0))
    assert (s.sample_counts() == 32).all()
    ref = tonemapped(G / f32(512), cam.gamma, cam.exp)
    err = lambda img: float(np.sqrt(np.mean((tonemapped(img, cam.gamma, cam.exp) - ref) ** 2)))
    raw, var, atr = err(A / f32(32)), err(s.denoise(mode="variance")), err(s.denoise())
    s.close()
    thr = _median(_rays(render, o, d, float("inf"), 16, seed=7), 32)
    ad = _rays(render, o, d, thr, 16, seed=7)
    cap = 64 * o.shape[0] * o.shape[1]
    print(f"equirect cornell 64x32 32 spp: raw {raw:.4f}, variance {var:.4f} ({var / raw:.3f} x raw), a-trous {atr:.4f} ({atr / raw:.3f} x raw); "
          f"adaptive at the median threshold: {ad['info']['samples']} of {cap} samples ({ad['info']['samples'] / cap:.3f})")
    assert var < raw
    assert ad["info"]["samples"] < cap


# ---- 7: the CLI --------------------------------------------------------------------------------------------------------------------
def test_cli_pano_adaptive(tmp_path, capsys):
    from micro_raytracer_amd import __main__ as cli
    desc = scenes.cornell_box(res=(64, 32), sample=64)
    path, out = tmp_path / "box.json", tmp_path / "x.png"
    path.write_text(json.dumps(desc))
    render = load_render(desc)
    s = Sampler(seed=3)
    o, d = cameras.equirect(render.frame.cam.pos, 64, 32)
    thr = _median(_rays(render, o, d, float("inf"), 16, seed=3), 32)
    cli.main([str(path), "-o", str(out), "--camera", "equirect", "--pano-guides", "--pano-adaptive", repr(thr), "--denoise", "--denoise-mode", "variance",
              "--seed", "3"])
    assert "adaptive: " in capsys.readouterr().out
    info = {}
    cameras.render_equirect(s, render, guides=True, adaptive=dict(threshold=thr, min_samples=32, step=16), info=info)
    assert info["min_count"] < info["max_count"]
    cli.save(str(tmp_path / "want.png"), s.img_denoised(mode="variance"))
    raw = s.img()
    s.close()
    read = lambda p: open(p, "rb").read()
    assert read(out) == read(tmp_path / "want.png") and read(out)[:8] == b"\x89PNG\r\n\x1a\n"
    cli.save(str(tmp_path / "raw.png"), raw)
    assert read(out) != read(tmp_path / "raw.png")
