"""All sixteen pt_rays_tiles kernels -- mrt_radiance_adaptive's: eight feature sets, each with the scene staged in LDS
and read through L2 -- held to mrt_radiance and to the oracle, one case of tests/radiance_adapt_cases.py per kernel: a 44 x 36
grid whose odd tiles hold wild rays beside tame ones (a tile is a wavefront), on a context created under the run's environment
with MRT_FLAG_COUNT_SEGMENTS, at min 32 / max 96 / step 16 -- the rule decides at 32 and at 64, the tile list shrinks twice -- and
the median of the reference's tile errors at 32 as the threshold.  Per case:

a. a one-sample mrt_radiance on the very context names the kernel the table expects (both calls go through rays_kernel);
b. per stop count the accumulator is mrt_radiance's sum word for word, NaN words included, and the half buffer the float32 fold
   of mrt_radiance's 16-sample chunks of the even rounds;
c. the accumulator meets orc_radiance at each pixel's stop count under radiance_cases.compare (the 1e-4 bar), no ray excluded;
d. the per-tile counts are the numpy rule's on mrt_radiance's sums at 32 and at 64; a tile with a NaN sum runs to the cap;
e. the context's segment counter is the total of mrt_radiance's over exactly the samples traced;
f. (the four kernels with F_BVH | F_VATTR) MRT_K_SPLIT = 1 and 4 change no bit;
g. a closing test: every one of the sixteen kernels answered a case."""
import os

import numpy as np
import pytest

import radiance_adapt_cases as AC
import radiance_cases as RC

pytestmark = pytest.mark.gpu
f32 = np.float32
SEED = AC.SEED
SEEN = {}          # (FEAT, scene in LDS) -> the cases that ran on that kernel
_ORACLE = {}


class Ctx:
    """A Sampler with the segment counter, created under a run's environment (read once, in mrt_create)."""

    def __init__(self, monkeypatch, render, env):
        from micro_raytracer_amd import Sampler, _abi
        for k in [k for k in os.environ if k.startswith("MRT_")]:
            monkeypatch.delenv(k)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        self.render = render
        self.s = Sampler(seed=SEED, device=0, flags=_abi.FLAG_COUNT_SEGMENTS)
        self.s.create(render)
        for k in env:
            monkeypatch.delenv(k)
        assert (self.s.nw, self.s.nh) == AC.GRID

    def radiance(self, o, d, ns, base=0, key=None):
        info = {}
        got = self.s.radiance(self.render, o, d, ns, sample_base=base, key=key, info=info)
        return got, info

    def kernel(self, o, d):
        _, info = self.radiance(o[:1, :8], d[:1, :8], 1)
        return info["kernel_features"], bool(info["scene_in_lds"])

    def adaptive(self, o, d, thr):
        info = self.s.radiance_adaptive(self.render, o, d, thr, min_samples=AC.MIN_SAMPLES, max_samples=AC.MAX_SAMPLES, step=AC.STEP)
        A, cnt = self.s.accum()
        return dict(A=A, cnt=cnt, H=self.s.adapt_half(), counts=self.s.sample_counts(), info=info, stats=self.s.stats())

    def close(self):
        self.s.close()


def oracle_sums(oracle_mod, case, n):
    """orc_radiance on the case's grid, samples [0, n), ray index = pixel index as the key: once per (grid, count) of a process."""
    k = (case.src.name, n)
    if k not in _ORACLE:
        _, holder = case.holder()
        orc = oracle_mod.Oracle(holder, seed=SEED)
        _ORACLE[k] = orc.radiance(case.o.reshape(-1, 3), case.d.reshape(-1, 3), n)[0]
        orc.close()
    return _ORACLE[k]


def yardstick(c, o, d):
    """mrt_radiance on the context: the sums at the three stop counts, the 16-sample chunks of the even rounds, the threshold."""
    whole = {n: c.radiance(o, d, n) for n in AC.STOPS}
    chunk = {j: c.radiance(o, d, AC.STEP, AC.STEP * j)[0] for j in range(0, AC.MAX_SAMPLES // AC.STEP, 2)}
    thr = AC.median_threshold(whole[AC.MIN_SAMPLES][0], chunk[0])
    return whole, chunk, thr


@pytest.mark.parametrize("name", AC.NAMES)
def test_case_holds_the_bits_of_radiance_the_rule_and_the_oracle(oracle_mod, monkeypatch, name):
    case = AC.case(name, oracle_mod)
    render, _ = case.holder()
    o, d = case.o, case.d
    c = Ctx(monkeypatch, render, case.run.env)
    # a. the kernel this case is about: the dispatch of rays_kernel on the context that then serves the adaptive call
    ran = c.kernel(o, d)
    assert ran == (case.feat, case.lds), (name, ran)
    whole, chunk, thr = yardstick(c, o, d)
    sums = {n: whole[n][0] for n in AC.STOPS}
    r = c.adaptive(o, d, thr)
    A, H, counts, info = r["A"], r["H"], r["counts"], r["info"]
    # (d.) the rule, recomputed at 32 and at 64 from mrt_radiance's sums
    want_counts = AC.rule_counts(sums, chunk, thr)
    hist = {n: int((want_counts == n).sum()) for n in AC.STOPS}
    nan = AC.nan_tiles(sums[AC.MIN_SAMPLES])
    print(f"adaptive on the GPU: {name:52s} FEAT {ran[0]:4d} in LDS {int(ran[1])} threshold {thr:.4f} tiles per count {hist} (with a NaN sum {int(nan.sum())}) "
          f"rounds {info['rounds']} launches {info['launches']} samples {info['samples']}")
    # b. the mrt_radiance yardstick, per stop count on the pixels that stopped there
    for n in AC.STOPS:
        m = counts == n
        bad = np.flatnonzero((RC.bits(A[m]) != RC.bits(sums[n][m])).any(axis=1))
        assert bad.size == 0, (name, n, [(A[m][i], sums[n][m][i]) for i in bad[:3]])
        h = AC.half_fold(chunk, n)
        bad = np.flatnonzero((RC.bits(H[m]) != RC.bits(h[m])).any(axis=1))
        assert bad.size == 0, (name, n, "half", [(H[m][i], h[m][i]) for i in bad[:3]])
    # (e.) mrt_radiance's segments over the samples traced: [0, 32) on all rays, [32, 64) and [64, 96) on the rays of the tiles that ran on
    seg = whole[AC.MIN_SAMPLES][1]["segments"]
    for base in AC.STOPS[:-1]:
        m = (counts > base).reshape(-1)
        if m.any():
            seg += c.radiance(o.reshape(-1, 3)[m], d.reshape(-1, 3)[m], 2 * AC.STEP, base, key=np.flatnonzero(m))[1]["segments"]
    c.close()
    # c. the oracle, directly: every pixel at its own stop count
    worst, same, broke = 0.0, 0, []
    for n in AC.STOPS:
        m = (counts == n).reshape(-1)
        if not m.any():
            continue
        ref = oracle_sums(oracle_mod, case, n)
        bad, w, share, _ = RC.compare(A.reshape(-1, 3)[m], ref[m], n)
        worst, same = max(worst, w), same + share * int(m.sum())
        broke += [(n, int(np.flatnonzero(m)[i]), A.reshape(-1, 3)[m][i], ref[m][i]) for i in bad[:3]]
    print(f"adaptive on the GPU: {name:52s} worst vs oracle {worst:.2e} bit-identical {same / counts.size:.4f} segments {r['stats']['segments']} "
          f"(mrt_radiance over the samples traced: {seg})")
    assert broke == [], (name, broke)
    # d. the rule's counts, the NaN tiles, the info
    assert np.array_equal(counts, want_counts[AC.tile_of_pixels() // AC.N_TX, AC.tile_of_pixels() % AC.N_TX]), (name, counts[::8, ::8], want_counts)
    assert nan.any() == case.has_nan and (counts[::8, ::8][nan] == AC.MAX_SAMPLES).all(), name
    assert info["samples"] == int(counts.astype(np.int64).sum()) and info["tiles"] == AC.N_TILES
    assert (info["min_count"], info["max_count"]) == (int(counts.min()), int(counts.max())) and r["cnt"] == info["min_count"]
    if case.noise_free:            # every tile error is exactly 0: nothing runs on (radiance_adapt_cases.NOISE_FREE)
        assert info["min_count"] == info["max_count"] == AC.MIN_SAMPLES and thr == 0.0
    else:
        assert info["min_count"] < info["max_count"], info
    # e. the segment counter
    assert r["stats"]["segments"] == seg, (name, r["stats"]["segments"], seg)
    SEEN.setdefault(ran, []).append(name)


@pytest.mark.parametrize("name", AC.BIG_NAMES)
def test_launch_shape_changes_no_bit_of_the_largest_kernels(oracle_mod, monkeypatch, name):
    """f. MRT_K_SPLIT = 1 and 4 on the kernels with the most registers and scratch (F_BVH | F_VATTR, with and without F_ENV, staged
    and through L2): the accumulator, the half buffer and the counts of the default run."""
    case = AC.case(name, oracle_mod)
    render, _ = case.holder()
    o, d = case.o, case.d
    runs = {}
    thr = None
    for ks in (None, "1", "4"):
        c = Ctx(monkeypatch, render, dict(case.run.env, **({"MRT_K_SPLIT": ks} if ks else {})))
        assert c.kernel(o, d) == (case.feat, case.lds), (name, ks)
        if thr is None:
            thr = yardstick(c, o, d)[2]
        runs[ks] = c.adaptive(o, d, thr)
        c.close()
    base = runs[None]
    assert base["info"]["min_count"] < base["info"]["max_count"]
    for ks in ("1", "4"):
        for k in ("A", "H", "counts"):
            assert np.array_equal(runs[ks][k].view(np.uint32), base[k].view(np.uint32)), (name, ks, k)
        assert runs[ks]["stats"]["segments"] == base["stats"]["segments"], (name, ks)
    print(f"adaptive on the GPU, launch shapes: {name:52s} k_split reported {[runs[k]['stats']['k_split'] for k in (None, '1', '4')]}: equal words")


def test_every_pt_rays_tiles_kernel_answered_a_case():
    """g. After the case tests (file order): each of the sixteen (FEAT, scene in LDS) kernels of pt_rays_tiles served an adaptive call
    on a context whose mrt_rays_info reported it."""
    if len(SEEN) == 0:
        pytest.skip("the case tests did not run in this session")
    want = [(f, lds) for f in RC.FEATS for lds in (True, False)]
    assert len(want) == 16
    for k in want:
        print(f"adaptive on the GPU: pt_rays_tiles FEAT {k[0]:4d} scene in {'LDS' if k[1] else 'L2 '}: {', '.join(SEEN.get(k, []))}")
    assert [k for k in want if k not in SEEN] == []
