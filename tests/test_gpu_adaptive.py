"""Tile-adaptive sampling (mrt_execute_adaptive) on the GPU: every tile holds the uniform render's bytes at its own count,
the samples are the oracle's, the stop rule is the one restated in numpy, the result does not depend on the launch shape,
and the context's state rules hold."""
import numpy as np
import pytest

from conftest import make_holder
from test_adaptive_host import np_tile_errors

pytestmark = pytest.mark.gpu

SEED = 5
MIN, MAX, STEP = 32, 128, 16


def _scenes():
    from micro_raytracer_amd import scenes
    return {
        "cornell128x96": scenes.cornell_box(res=(128, 96), sample=MAX, bounce=8),
        "mesh": scenes.mesh_scene(res=(96, 64), sample=MAX, bounce=6),
        "dof": scenes.dof_scene(res=(96, 64), sample=MAX, bounce=6),
        "ssaa2": scenes.cornell_box(res=(64, 48), ssaa=2, sample=MAX, bounce=8),
        "partial100x60": scenes.cornell_box(res=(100, 60), sample=MAX, bounce=8),
    }


_CACHE = {}


def _scene(name):
    if name not in _CACHE:
        _CACHE[name] = make_holder(_scenes()[name])
    return _CACHE[name]


def _adaptive(render, thr, max_samples=MAX, step=STEP, min_samples=MIN, flags=0):
    from micro_raytracer_amd import Sampler
    s = Sampler(seed=SEED, device=0, flags=flags)
    info = s.execute_adaptive(render, thr, min_samples=min_samples, max_samples=max_samples, step=step)
    A, cnt = s.accum()
    out = dict(info=info, A=A, cnt=cnt, counts=s.sample_counts(), H=s.adapt_half(), s=s)
    return out


def _tile_counts(counts):
    return counts[::8, ::8]


def _uniform(render, n):
    from micro_raytracer_amd import Sampler
    s = Sampler(seed=SEED, device=0)
    s.execute(render, n_samples=n)
    return s


def _threshold(render):
    """A threshold that stops roughly half the tiles at MIN: the median tile error of a run that stops everything there."""
    r = _adaptive(render, float("inf"))
    et, nan, _ = np_tile_errors(r["A"], r["H"], MIN, 0.0)
    r["s"].close()
    return float(np.median(et[~nan]))


def _tile_mask(counts, n):
    return counts == n


@pytest.mark.parametrize("name", ["cornell128x96", "mesh", "dof", "ssaa2", "partial100x60"])
def test_adaptive_bit_identity_oracle_and_rule(name, oracle_mod):
    render, holder = _scene(name)
    thr = _threshold(render)
    r = _adaptive(render, thr)
    A, H, counts, info = r["A"], r["H"], r["counts"], r["info"]
    tc = _tile_counts(counts)
    stops = sorted(set(np.unique(tc).tolist()))
    assert len(stops) >= 2, stops
    assert all(n % (2 * STEP) == 0 and MIN <= n <= MAX for n in stops)
    assert r["cnt"] == counts.min() == info["min_count"] and counts.max() == info["max_count"]
    nh, nw = counts.shape
    assert info["samples"] == int(counts.astype(np.int64).sum()) and info["tiles"] == tc.size
    st = r["s"].stats()
    assert st["samples"] == info["samples"] and st["launches"] == info["launches"] > 0

    # 1. bit identity with a uniform n-sample render, per stop count, accumulator and tone-mapped bytes
    ss = r["s"].img_ss()
    for n in stops:
        u = _uniform(render, n)
        U, _ = u.accum()
        m = _tile_mask(counts, n)
        assert np.array_equal(A[m], U[m]), n
        assert np.array_equal(ss[m], u.img_ss()[m]), n
        u.close()
    img = r["s"].img()
    fw, fh = render.frame.res
    assert np.array_equal(img, oracle_mod.lanczos3_resize(ss, fw, fh))

    # 2. the oracle's samples: sum over the pixel's count, and over its even rounds for H
    o = oracle_mod.Oracle(holder, seed=SEED)
    rng = np.random.default_rng(17)
    worst = worst_h = 0.0
    for p in rng.choice(nw * nh, size=64, replace=False):
        y, x = divmod(int(p), nw)
        k = int(counts[y, x])
        tot = np.zeros(3, np.float64)
        half = np.zeros(3, np.float64)
        for s_ in range(k):
            v, _ = o.trace_pixel(x, y, s_)
            tot += v
            if (s_ // STEP) % 2 == 0:
                half += v
        worst = max(worst, float(np.abs(tot - A[y, x]).max()) / k)
        worst_h = max(worst_h, float(np.abs(half - H[y, x]).max()) / (k // 2))
    o.close()
    assert worst <= 1e-4 and worst_h <= 1e-4, (worst, worst_h)

    # 3. the rule, restated from the device's A and H: a tile that stopped below MAX is converged at its count
    n_ty, n_tx = tc.shape
    for n in stops:
        if n == MAX:
            continue
        et, nan, conv = np_tile_errors(A, H, n, thr)
        assert conv[tc == n].all(), n
    # ... and a tile the full run took beyond an earlier evaluation point n' is unconverged there (run capped at n')
    for cap in range(MIN, MAX, 2 * STEP):
        c = _adaptive(render, thr, max_samples=cap)
        assert np.array_equal(c["A"][counts <= cap], A[counts <= cap])
        et, nan, conv = np_tile_errors(c["A"], c["H"], cap, thr)
        beyond = tc > cap
        assert not conv[beyond].any(), cap
        c["s"].close()
    r["s"].close()


@pytest.mark.parametrize("name", ["cornell128x96", "partial100x60"])
def test_adaptive_threshold_zero_and_inf(name):
    render, _ = _scene(name)
    r = _adaptive(render, float("inf"))
    assert (r["counts"] == MIN).all() and r["info"]["tiles_converged"] == r["info"]["tiles"]
    r["s"].close()
    z = _adaptive(render, 0.0)
    tc = _tile_counts(z["counts"])
    early = tc < MAX
    for n in set(np.unique(tc[early]).tolist()):
        et, nan, _ = np_tile_errors(z["A"], z["H"], n, 0.0)
        assert (et[tc == n] == 0).all() and not nan[tc == n].any()
    u = _uniform(render, MAX)
    U, _ = u.accum()
    m = z["counts"] == MAX
    assert m.any() and np.array_equal(z["A"][m], U[m])
    z["s"].close()
    u.close()


SHAPES = [{"MRT_BLOCK_THREADS": "64"}, {"MRT_BLOCK_THREADS": "256"}, {"MRT_BLOCK_THREADS": "1024"}, {"MRT_NO_PERSIST": "1"},
          {"MRT_SCENE_IN_L2": "1"}, {"MRT_K_SPLIT": "1"}, {"MRT_K_SPLIT": "4"}, {"MRT_MAX_CHUNKS": "1"}, "defer"]


@pytest.mark.parametrize("name,step", [("partial100x60", 16), ("partial100x60", 32), ("mesh", 16)])
def test_adaptive_independent_of_launch_shape(name, step, monkeypatch):
    from micro_raytracer_amd import _abi
    render, _ = _scene(name)
    thr = _threshold(render)
    base = _adaptive(render, thr, step=step, min_samples=2 * step)
    assert len(np.unique(base["counts"])) >= 2
    seen = set()
    for shape in SHAPES:
        with monkeypatch.context() as mp:
            flags = 0
            if shape == "defer":
                flags = _abi.FLAG_DEFER
            else:
                for k, v in shape.items():
                    mp.setenv(k, v)
            r = _adaptive(render, thr, step=step, min_samples=2 * step, flags=flags)
            st = r["s"].stats()
            seen.add((st["block_threads"], st["scene_in_lds"], st["k_split"]))
            assert np.array_equal(r["counts"], base["counts"]), shape
            assert np.array_equal(r["A"], base["A"]), shape
            assert np.array_equal(r["H"], base["H"]), shape
            r["s"].close()
    assert len(seen) >= 3, seen
    base["s"].close()


def test_adaptive_state_rules():
    from micro_raytracer_amd import MrtError, Sampler, _abi
    render, _ = _scene("partial100x60")
    s = Sampler(seed=SEED, device=0)
    s.execute_adaptive(render, 0.05, min_samples=32, max_samples=64)
    with pytest.raises(MrtError) as e:
        s.execute(render, n_samples=4)
    assert e.value.code == _abi.MRT_ERR_STATE
    with pytest.raises(MrtError) as e:                       # holds samples
        s.execute_adaptive(render, 0.05, min_samples=32, max_samples=64)
    assert e.value.code == _abi.MRT_ERR_STATE
    s.reset()
    s.execute(render, n_samples=4)                           # uniform again
    assert s.accum()[1] == 4 and (s.sample_counts() == 4).all()
    with pytest.raises(MrtError) as e:
        s.adapt_half()
    assert e.value.code == _abi.MRT_ERR_STATE
    with pytest.raises(MrtError) as e:                       # uniform samples on board
        s.execute_adaptive(render, 0.05, min_samples=32, max_samples=64)
    assert e.value.code == _abi.MRT_ERR_STATE
    s.reset()
    for bad in [dict(step=24), dict(step=0), dict(min_samples=48), dict(min_samples=0), dict(max_samples=80),
                dict(min_samples=128, max_samples=64), dict(threshold=-1.0), dict(threshold=float("nan"))]:
        kw = dict(threshold=0.05, min_samples=32, max_samples=64, step=16)
        kw.update(bad)
        with pytest.raises(MrtError) as e:
            s.execute_adaptive(render, kw.pop("threshold"), **kw)
        assert e.value.code == _abi.MRT_ERR_ARG, bad
    s.execute_adaptive(render, 0.05, min_samples=32, max_samples=64)      # nothing was changed by the refusals
    s.set_accum(*s.accum())                                  # set_accum: uniform mode again
    s.execute(render, n_samples=1)
    s.close()
    sh = Sampler(seed=SEED, device=0, shard_index=0, shard_count=2)
    with pytest.raises(MrtError) as e:
        sh.execute_adaptive(render, 0.05, min_samples=32, max_samples=64)
    assert e.value.code == _abi.MRT_ERR_STATE
    sh.close()


def test_cli_adaptive_png_equals_sampler_img(tmp_path, capsys):
    import json

    from micro_raytracer_amd import Sampler, _lib, load_render, scenes
    from micro_raytracer_amd import __main__ as cli
    desc = scenes.cornell_box(res=(64, 48), sample=16, bounce=6)
    path = tmp_path / "scene.json"
    path.write_text(json.dumps(desc))
    out = tmp_path / "cli.png"
    cli.main([str(path), "-o", str(out), "--adaptive", "0.08", "--sample", "64", "--seed", "3"])
    assert "samples traced of" in capsys.readouterr().out
    render = load_render(str(path))
    render.rt.sample = 64
    s = Sampler(seed=3)
    s.execute_adaptive(render, 0.08, min_samples=32, max_samples=64, step=16)
    ref = tmp_path / "ref.png"
    _lib.save_image(str(ref), s.img())
    s.close()
    assert out.read_bytes() == ref.read_bytes()
