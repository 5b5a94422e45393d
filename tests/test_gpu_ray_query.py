"""Closest-hit queries on caller-supplied rays, on the GPU: mrt_selftest_trace (csrc/mrt_rayq.hip -- the prologue of pt_megakernel,
then trace on the ray of thread i) on a context created under the environment that selects each instantiation of the hook,
against the x86 build of the same per-ray body (tests/emu/rayq_probe.cpp: bit for bit, no exclusions) and against the oracle's
orc_ray_query (the rule and the -- empty -- exclusion set of tests/test_ray_query_host.py).

What the x86 build cannot show and these tests can: the wave votes (wave_all is a ballot over 64 lanes here), the fast division
cores inside the axis scan, the LDS copy of the scene, the hot prefix of the warm and deep levels, the walk areas behind the
stash region, and the F_IDENT builds.  The wavefront of a ray is chosen by its index: ray i is lane i % 64 of wavefront i / 64."""
import os

import numpy as np
import pytest

import rayq_cases as R
import test_ray_query_host as H
from conftest import make_holder

pytestmark = pytest.mark.gpu
f32 = np.float32
SEEN = {}          # (scene in LDS, FEAT) -> cases run: the table of instantiations the family tests covered


@pytest.fixture(scope="module")
def probe():
    return R.shared_probe()


class Ctx:
    """A Sampler created under a variant's environment (read once, in mrt_create)."""

    def __init__(self, monkeypatch, render, env):
        from micro_raytracer_amd import Sampler
        for k in [k for k in os.environ if k.startswith("MRT_")]:
            monkeypatch.delenv(k)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        self.s = Sampler(seed=3, device=0)
        self.s.create(render)
        for k in env:
            monkeypatch.delenv(k)
        self.stats = self.s.stats()

    def trace(self, o, d):
        from micro_raytracer_amd import _lib
        return _lib.selftest_trace(self.s, o, d)["words"]

    def close(self):
        self.s.close()


@pytest.mark.parametrize("fam", list(R.FAMILIES))
def test_family_on_the_gpu_equals_the_x86_probe_and_the_oracle(probe, oracle_mod, monkeypatch, fam):
    for case in R.family(fam, oracle_mod):
        render, holder = make_holder(case.desc)
        ref = H.oracle_answers(oracle_mod, holder, case)
        ex = H.excluded(case)
        assert len(ref) <= 10000
        for v in case.variants:
            c = Ctx(monkeypatch, render, v.env)
            st = c.stats
            if v.feat is None:
                v.feat = st["kernel_features"]
            # the context runs the instantiation this variant is about: a test cannot pass on the wrong kernel
            assert (st["kernel_features"], bool(st["scene_in_lds"]), st["block_threads"]) == (v.feat, v.lds, 256), (case.name, v.label, st)
            got = c.trace(case.o, case.d)
            c.close()
            want, _ = R.probe_trace(probe, holder, v.cfg(), case.o, case.d)
            bad_x86 = np.flatnonzero((got != want).any(axis=1))
            bad_orc = np.flatnonzero(~R.same_words(got, ref) & ~ex)
            print(f"ray queries on the GPU: {fam:10s} {case.name:36s} {v.label:14s} kernel_features {st['kernel_features']:4d} scene_in_lds "
                  f"{st['scene_in_lds']} lds_bytes {st['lds_bytes']:6d} rays {len(ref):5d} hits {int(got[:, 0].sum()):5d} excluded {int(ex.sum())} "
                  f"worst ulp vs x86 {R.ulp_distance(got, want)} vs oracle {R.ulp_distance(got, ref)} disagreeing {bad_x86.size} / {bad_orc.size}")
            assert bad_x86.size == 0, (case.name, v.label, [(i, case.o[i], case.d[i], got[i], want[i]) for i in bad_x86[:3]])
            assert bad_orc.size == 0, (case.name, v.label, [(i, case.o[i], case.d[i], got[i], ref[i]) for i in bad_orc[:3]])
            assert (got[:, 0] == got[:, 1]).all()
            SEEN.setdefault((v.lds, v.feat), []).append(f"{fam}/{case.name}")


def test_every_instantiation_of_the_hook_was_run():
    """After the family tests (file order): each kernel of the hook's list answered at least one case, on a context that reported it."""
    if len(SEEN) == 0:
        pytest.skip("the family tests did not run in this session")
    A, B, T, M, Lg = R.F_ALL, R.F_BVH, R.F_TRI, R.F_MAPS, R.F_LIGHTS
    want = [(True, R.F_IDENT), (True, R.F_IDENT | R.F_BOX | Lg), (True, R.F_BOX | Lg), (True, R.F_IDENT | B), (True, R.FN), (True, A), (True, A | B),
            (True, A | R.F_COLD), (True, A | R.F_COLD | R.F_DEEP), (True, A | B | R.F_COLD | R.F_DEEP), (True, A | R.F_VATTR),
            (True, A | R.F_VATTR | R.F_ENV), (False, A), (False, A | B)]
    for k in want:
        print(f"ray queries on the GPU: scene in {'LDS' if k[0] else 'L2 '} kernel_features {k[1]:4d}: {', '.join(SEEN.get(k, []))}")
    assert [k for k in want if k not in SEEN] == []


# ---- wavefront composition ---------------------------------------------------------------------------------------------------------
def _axis_case(oracle_mod):
    return R.family("axis", oracle_mod)[0]


def _small_numerators(case, ref):
    """Tame rays whose numerator against the plane they hit first is below 2^-40 in magnitude: |o_k - pos_k| for the axis plane
    (renderer r of six_plane_scene) that won -- computed here from the scene description, as the scan forms it (pk + (ok - pk)) + sd."""
    rend = case.desc["scene"]["renderer"]
    small = np.zeros(len(ref), bool)
    for i in np.flatnonzero(ref[:, 0] == 1):
        r = rend[int(ref[i, 2])]
        if r["type"] != "plane":
            continue
        k = int(np.argmax(np.abs(r["n"])))
        pk = f32(r["pos"][k])
        num = (pk + (case.o[i, k] - pk)) - pk
        small[i] = abs(num) < R.WIN_LO
    return small


def test_wavefront_composition_changes_no_word(oracle_mod, monkeypatch):
    """The same rays in three orders: (a) tame rays sorted into whole wavefronts (they take the axis body and its fast division
    cores), (b) dealt so that every wavefront holds an untame lane (every vote fails: the generic body), (c) tame wavefronts in
    which some lanes have a numerator below 2^-40 against the plane they hit first (the inner vote of plane() fails for the
    wavefront at that instance).  Every ray's nine words are the same in all three, and equal the oracle's."""
    from test_axis_scan import _tame
    case = _axis_case(oracle_mod)
    render, holder = make_holder(case.desc)
    ref = H.oracle_answers(oracle_mod, holder, case)
    o, d = case.o, case.d
    n = len(o)
    tame = _tame(o, d)
    small = _small_numerators(case, ref) & tame
    assert small.sum() >= 64 and (tame & ~small).sum() >= 3000 and (~tame).sum() >= 73
    ti, ui = np.flatnonzero(tame & ~small), np.flatnonzero(~tame)
    si = np.flatnonzero(small)
    # (a) tame rays first, padded with repeats to whole wavefronts, then the rest
    pad = (-(len(ti) + len(si))) % 64
    order_a = np.concatenate([ti, si, ti[:pad], ui])
    n_tame_waves = (len(ti) + len(si) + pad) // 64
    assert _tame(o[order_a[:n_tame_waves * 64]], d[order_a[:n_tame_waves * 64]]).all()
    # (b) every wavefront: lane 0 untame (the untame rays cycled), 63 others
    rest = np.concatenate([ti, si])
    n_waves = (len(rest) + 62) // 63
    order_b = np.concatenate([np.concatenate([[ui[w % len(ui)]], rest[w * 63:(w + 1) * 63]]) for w in range(n_waves)] + [ui])
    wave_of = np.arange(len(order_b)) // 64
    assert all((~tame[order_b[wave_of == w]]).any() for w in range(wave_of.max() + 1))
    # (c) tame wavefronts, one small-numerator lane each (cycled), in lane w % 64
    per = 63
    n_waves_c = len(ti) // per
    rows = []
    for w in range(n_waves_c):
        lanes = list(ti[w * per:(w + 1) * per])
        lanes.insert(w % 64, si[w % len(si)])
        rows.append(np.array(lanes))
    order_c = np.concatenate(rows + [ti[n_waves_c * per:], si, ui])
    c = Ctx(monkeypatch, render, case.variants[0].env)
    assert c.stats["kernel_features"] == R.F_IDENT and c.stats["scene_in_lds"] == 1
    results = []
    for name, order in (("a", order_a), ("b", order_b), ("c", order_c)):
        assert len(order) <= 10000 and set(order.tolist()) == set(range(n))
        got = c.trace(o[order], d[order])
        assert R.same_words(got, ref[order]).all(), name
        # scatter back to the rays (repeats of a ray must agree with each other as well)
        back = np.zeros((n, 9), np.uint32)
        back[order] = got
        assert np.array_equal(back[order], got), name
        results.append(back)
    c.close()
    assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2])
    print(f"ray queries on the GPU, wavefront composition: {n} rays, {n_tame_waves} tame wavefronts in (a), {n_waves} mixed in (b), "
          f"{n_waves_c} with a small-numerator lane in (c): equal words")


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_partial_last_wavefront(probe, oracle_mod, monkeypatch, n):
    """Threads >= n leave before the query: the votes of the last wavefront are taken among its n % 64 live lanes."""
    case = _axis_case(oracle_mod)
    render, holder = make_holder(case.desc)
    from test_axis_scan import _tame
    tame = np.flatnonzero(_tame(case.o, case.d))
    idx = tame[:n]                                                  # tame rays only: a dead lane must not read as an untame one
    c = Ctx(monkeypatch, render, case.variants[0].env)
    got = c.trace(case.o[idx], case.d[idx])
    # a mesh context as well: the walk areas of a partial wavefront
    mcase = R.family("mesh", oracle_mod)[0]
    mrender, mholder = make_holder(mcase.desc)
    mv = mcase.variants[2]
    mc = Ctx(monkeypatch, mrender, mv.env)
    assert mc.stats["kernel_features"] == mv.feat
    mgot = mc.trace(mcase.o[:n], mcase.d[:n])
    c.close(); mc.close()
    want, _ = R.probe_trace(probe, holder, case.variants[0].cfg(), case.o[idx], case.d[idx])
    assert np.array_equal(got, want)
    mwant, _ = R.probe_trace(probe, mholder, mv.cfg(), mcase.o[:n], mcase.d[:n])
    assert np.array_equal(mgot, mwant)


# ---- the hook leaves the context alone ---------------------------------------------------------------------------------------------
def test_no_side_effects_between_two_executes(oracle_mod, monkeypatch):
    from micro_raytracer_amd import Sampler, _lib
    case = R.family("surface", oracle_mod)[0]
    desc = dict(case.desc)
    render, _ = make_holder(desc)

    def run(with_hook):
        s = Sampler(seed=9, device=0)
        s.execute(render, n_samples=3)
        a0, c0 = s.accum()
        aov0 = s.aov()
        if with_hook:
            _lib.selftest_trace(s, case.o[:2000], case.d[:2000])
            a1, c1 = s.accum()
            assert c1 == c0 and np.array_equal(a0.view(np.uint32), a1.view(np.uint32))
            aov1 = s.aov()
            for k in aov0:
                assert np.array_equal(aov0[k].view(np.uint32) if aov0[k].dtype == f32 else aov0[k], aov1[k].view(np.uint32) if aov1[k].dtype == f32 else aov1[k]), k
        s.execute(render, n_samples=2)
        a2, c2 = s.accum()
        s.close()
        return a2, c2

    a_plain, c_plain = run(False)
    a_hook, c_hook = run(True)
    assert c_plain == c_hook == 5
    assert np.array_equal(a_plain.view(np.uint32), a_hook.view(np.uint32))


def test_argument_and_state_errors(oracle_mod, monkeypatch):
    import ctypes as C

    from micro_raytracer_amd import Sampler, _abi, _lib
    case = _axis_case(oracle_mod)
    render, _ = make_holder(case.desc)
    L = _lib.lib()
    s = Sampler(seed=1, device=0)
    s.create(render)
    o, d = np.ascontiguousarray(case.o[:4]), np.ascontiguousarray(case.d[:4])
    out = np.zeros((4, 9), np.uint32)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    po, pd, pw = o.ctypes.data_as(fp), d.ctypes.data_as(fp), out.ctypes.data_as(up)
    assert L.mrt_selftest_trace(s._ctx, 0, po, pd, pw) == _abi.MRT_ERR_ARG
    assert L.mrt_selftest_trace(s._ctx, 4, None, pd, pw) == _abi.MRT_ERR_ARG
    assert L.mrt_selftest_trace(s._ctx, 4, po, None, pw) == _abi.MRT_ERR_ARG
    assert L.mrt_selftest_trace(s._ctx, 4, po, pd, None) == _abi.MRT_ERR_ARG
    assert L.mrt_selftest_trace(None, 4, po, pd, pw) == _abi.MRT_ERR_ARG
    assert L.mrt_selftest_trace(s._ctx, 4, po, pd, pw) == 0 and out[:, 0].all()
    s.close()
    # a sharded context
    s = Sampler(seed=1, device=0, shard_index=0, shard_count=2)
    s.create(render)
    with pytest.raises(_lib.MrtError) as e:
        _lib.selftest_trace(s, o, d)
    assert e.value.code == _abi.MRT_ERR_STATE and "sharded" in e.value.msg
    s.close()
    # an instantiation outside the hook's list: the sphere lattice WITH its light is F_IDENT | F_LIGHTS | F_BVH
    from micro_raytracer_amd import scenes
    render, _ = make_holder(scenes.instance_grid(res=(16, 16), sample=1, n=4))
    s = Sampler(seed=1, device=0)
    s.create(render)
    feat = s.stats()["kernel_features"]
    assert feat == R.F_IDENT | R.F_LIGHTS | R.F_BVH
    with pytest.raises(_lib.MrtError) as e:
        _lib.selftest_trace(s, o, d)
    assert e.value.code == _abi.MRT_ERR_STATE and f"FEAT {feat}" in e.value.msg
    s.close()
