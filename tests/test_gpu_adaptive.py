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


def _adaptive(render, thr, max_samples=MAX, step=STEP, min_samples=MIN, flags=0, seed=SEED):
    from micro_raytracer_amd import Sampler
    s = Sampler(seed=seed, device=0, flags=flags)
    info = s.execute_adaptive(render, thr, min_samples=min_samples, max_samples=max_samples, step=step)
    A, cnt = s.accum()
    out = dict(info=info, A=A, cnt=cnt, counts=s.sample_counts(), H=s.adapt_half(), s=s)
    return out


def _tile_counts(counts):
    return counts[::8, ::8]


def _uniform(render, n, seed=SEED):
    from micro_raytracer_amd import Sampler
    s = Sampler(seed=seed, device=0)
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


@pytest.mark.parametrize("step,k_split", [(16, 2), (48, 2), (96, 4)])
def test_adaptive_rounds_are_cut_into_bounded_launches(step, k_split, monkeypatch):
    """Each round is cut at chunk boundaries into launches of at most MRT_MAX_CHUNKS chunks; MRT_K_SPLIT lanes per pixel are
    halved to the round's chunk count (even rounds keep 2: their chunk sums go to H as well), and the reported k_split is
    the largest of any launch.  A threshold of inf with min = max pins the round count."""
    render, _ = _scene("partial100x60")
    monkeypatch.setenv("MRT_K_SPLIT", "4")
    monkeypatch.setenv("MRT_MAX_CHUNKS", "4")
    n = 4 * step
    r = _adaptive(render, float("inf"), max_samples=n, step=step, min_samples=n)
    info, st = r["info"], r["s"].stats()
    per_round = -(-(step // 16) // 4)
    assert (r["counts"] == n).all() and info["rounds"] == n // step == 4
    assert info["launches"] == st["launches"] == info["rounds"] * per_round, (info, st)
    assert st["k_split"] == k_split, st
    r["s"].close()


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


# ---- more than one adapt_compact block: the tile list is compacted by one 1024-thread workgroup in blocks of 1024 entries,
# and each block's survivors are written after the survivors of the blocks before it
BIG_MIN, BIG_MAX, BIG_STEP = 32, 96, 16


def _big_scenes():
    from micro_raytracer_amd import scenes
    # 48 x 42 = 2016 tiles each.  The Cornell box of cornell_box() is not used: its tile errors at MIN take a few hundred
    # discrete values (single paths reaching the one emitter), and hundreds of tiles tie around the 1024th.
    return {"cornell2_384x336": scenes.cornell_box2(res=(384, 336), ssaa=1, sample=BIG_MAX, bounce=8),
            "mesh_ssaa2_192x168": scenes.mesh_scene(res=(192, 168), ssaa=2, sample=BIG_MAX, bounce=6)}


@pytest.mark.parametrize("name", ["cornell2_384x336", "mesh_ssaa2_192x168"])
def test_adaptive_beyond_one_compaction_block(name, oracle_mod):
    render, _ = make_holder(_big_scenes()[name])
    n_tiles = ((render.frame.nw + 7) // 8) * ((render.frame.nh + 7) // 8)
    for seed in range(SEED, SEED + 8):
        # the tile errors at MIN; a seed whose errors tie where a threshold must separate them is passed over.  "Nearly all
        # active": the first gap above the smallest errors (black tiles all have error 0)
        kw = dict(min_samples=BIG_MIN, max_samples=BIG_MAX, step=BIG_STEP, seed=seed)
        r = _adaptive(render, float("inf"), **kw)
        e0, nan0, _ = np_tile_errors(r["A"], r["H"], BIG_MIN, 0.0)
        r["s"].close()
        assert e0.size == n_tiles > 1024 and not nan0.any()
        es = np.sort(e0.reshape(-1))
        j0 = int(np.flatnonzero(es[1:] > es[:-1])[0])
        targets = (1023, 1024, 1025, n_tiles - 1 - j0)
        if all(es[n_tiles - 1 - k] < es[n_tiles - k] for k in targets):
            break
    else:
        raise AssertionError("every seed tried has tied tile errors at a target")
    uniform = {n: _uniform(render, n, seed=seed) for n in range(BIG_MIN, BIG_MAX + 1, 2 * BIG_STEP)}
    U = {n: (u.accum()[0], u.img_ss()) for n, u in uniform.items()}
    for u in uniform.values():
        u.close()
    fw, fh = render.frame.res
    for active in targets:
        j = n_tiles - 1 - active                           # threshold = the (j+1)-th smallest error: j + 1 tiles stop at MIN
        assert es[j] < es[j + 1], (active, es[j:j + 2])
        thr = float(es[j])
        a = _adaptive(render, thr, **kw)
        counts, info, A, H = a["counts"], a["info"], a["A"], a["H"]
        tc = _tile_counts(counts)
        conv0 = e0 <= np.float32(thr)
        assert int((~conv0).sum()) == active
        assert np.array_equal(tc > BIG_MIN, ~conv0), active       # exactly the tiles numpy leaves running go on
        stops = np.unique(tc)
        assert all(n % (2 * BIG_STEP) == 0 and BIG_MIN <= n <= BIG_MAX for n in stops.tolist()), stops
        ss = a["s"].img_ss()
        for n in stops.tolist():
            m = counts == n
            assert np.array_equal(A[m], U[n][0][m]) and np.array_equal(ss[m], U[n][1][m]), (active, n)
        for n in stops.tolist():                                 # a tile stopped below MAX is converged at its count
            if n < BIG_MAX:
                assert np_tile_errors(A, H, n, thr)[2][tc == n].all(), (active, n)
        c = _adaptive(render, thr, min_samples=BIG_MIN, max_samples=2 * BIG_MIN, step=BIG_STEP, seed=seed)   # ... and one beyond 64 is not at 64
        assert not np_tile_errors(c["A"], c["H"], 2 * BIG_MIN, thr)[2][tc > 2 * BIG_MIN].any(), active
        c["s"].close()
        # the info block, replayed on the host from the counts
        at_max = tc == BIG_MAX
        conv_max = np_tile_errors(A, H, BIG_MAX, thr)[2]
        assert info["tiles"] == n_tiles
        assert info["tiles_converged"] == int((~at_max).sum() + (conv_max & at_max).sum()), active
        assert info["samples"] == int(counts.astype(np.int64).sum())
        assert info["rounds"] == int(tc.max()) // BIG_STEP
        assert info["min_count"] == tc.min() and info["max_count"] == tc.max()
        if (fw, fh) != (counts.shape[1], counts.shape[0]):
            assert np.array_equal(a["s"].img(), oracle_mod.lanczos3_resize(ss, fw, fh))
        print(f"{name} seed {seed}: {active} of {n_tiles} tiles active after the first evaluation, stops {stops.tolist()}, "
              f"{info['rounds']} rounds, {info['tiles_converged']} converged")
        a["s"].close()


# ---- a failed adaptive call leaves an empty uniform context behind (mrt_execute_adaptive's rollback)
@pytest.mark.parametrize("bound", [False, True], ids=["own", "bound"])
@pytest.mark.parametrize("knob", ["MRT_PARTIAL_LIMIT_BYTES", "MRT_PARTIAL_FAIL_ALLOC"])
def test_adaptive_failure_rolls_back_to_an_empty_uniform_context(knob, bound, monkeypatch):
    from micro_raytracer_amd import MrtError, Sampler, _abi
    from test_image_path import DeviceBuffer
    render, _ = _scene("partial100x60")
    probe = Sampler(seed=SEED, device=0).create(render)
    plane = probe.padded_rows() * probe.nw * 3 * 4                # bytes of one chunk plane
    probe.close()
    with monkeypatch.context() as mp:
        mp.setenv(knob, str(plane - 4) if knob == "MRT_PARTIAL_LIMIT_BYTES" else "1")
        s = Sampler(seed=SEED, device=0).create(render)
    t = None
    if bound:
        t = DeviceBuffer(plane, fill=3.0)
        s.bind_accum(t.ptr.value, t.nbytes)
    with pytest.raises(MrtError) as e:
        s.execute_adaptive(render, 0.05, min_samples=32, max_samples=64)
    assert e.value.code == _abi.MRT_ERR_LIMIT and "chunk planes" in e.value.msg
    with pytest.raises(MrtError) as e:
        s.img()
    assert e.value.code == _abi.MRT_ERR_STATE
    with pytest.raises(MrtError) as e:
        s.adapt_half()
    assert e.value.code == _abi.MRT_ERR_STATE
    A, cnt = s.accum()
    assert cnt == 0 and not A.any() and (s.sample_counts() == 0).all()
    if bound:
        t.synchronize()
        assert not t.read().any()
    s.execute(render, n_samples=20)
    f = _uniform(render, 20)
    A, cnt = s.accum()
    F, fcnt = f.accum()
    assert cnt == fcnt == 20 and np.array_equal(A.view(np.uint32), F.view(np.uint32))
    assert np.array_equal(s.img(), f.img())
    if bound:
        t.synchronize()
        assert np.array_equal(t.read(np.uint32).reshape(-1, s.nw, 3)[:s.nh], F.view(np.uint32))
    with pytest.raises(MrtError) as e:
        s.adapt_half()
    assert e.value.code == _abi.MRT_ERR_STATE
    f.close()
    s.close()
    if bound:
        t.free()
