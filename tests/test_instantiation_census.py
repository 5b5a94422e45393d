"""A census of the path-tracing kernel's instantiations (csrc/mrt_megakernel.h): every compiled
(workgroup size, scene in LDS or through L2, FEAT) row -- listed by the library itself, mrt_selftest_instantiations -- has a recipe
(tests/inst_cases.py) that plan_launch sends to exactly that row, or stands on an explicit UNREACHABLE list.

Without a GPU: the dispatch is closed and the recipes complete (plan_launch); every reduced feature set renders its recipe scene
on x86 (tests/emu/census_probe.cpp) bit for bit like the full set and within the oracle's bar; every recipe scene's x86 render meets
the oracle at 32 and 40 samples.  On the GPU: every reachable row runs as itself, once as pt_megakernel<b, T, F> and once over a
tile list as pt_megakernel<b, T, F, TileList>, is held to the oracle, and all rows of a scene give the same accumulator bits."""
import ctypes as C
import os

import numpy as np
import pytest

import inst_cases as IC
from inst_cases import FN, SEED, SPP, SPP_LIST
from micro_raytracer_amd import _abi, _lib
from micro_raytracer_amd._abi import F_ALL, F_BOX, F_BVH, F_COLD, F_DEEP, F_ENV, F_IDENT, F_LIGHTS, F_NOSTASH, F_TRI, F_VATTR
from test_fuzz_scenes import _check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = min(16, os.cpu_count() or 1)
ROWS = IC.rows()
BY_SCENE, ABI_ONLY = IC.census()
ALL_SCENES = {**BY_SCENE, **ABI_ONLY}
SCENES = sorted(ALL_SCENES, key=lambda s: (s.bits, s.ident, s.pad or "", s.unref))

# the instantiations of tests/emu/census_probe.cpp (cs_list must agree): MRT_PLAIN16, MRT_BVH4, the F_IDENT builds
X86_FEATS = list(range(16)) + [F_BVH, F_LIGHTS | F_BVH, FN | F_BVH, F_ALL | F_BVH] + \
    [F_IDENT, F_IDENT | F_BOX, F_IDENT | F_LIGHTS, F_IDENT | F_BOX | F_LIGHTS, F_IDENT | F_BVH, F_IDENT | F_LIGHTS | F_BVH]


# ---- the table ------------------------------------------------------------------------------------------------------------------
def test_the_hook_lists_every_compiled_case_once():
    """144 rows, none twice, in the counts per launch shape that the MRT_SHAPES_* lists give; the hook is declared and bound."""
    assert len(ROWS) == 144 and len(set(ROWS)) == len(ROWS)
    per_shape = {}
    for t, in_lds, _ in ROWS:
        per_shape[(t, in_lds)] = per_shape.get((t, in_lds), 0) + 1
    assert per_shape == {(64, True): 24, (256, True): 46, (512, True): 28, (1024, True): 38, (256, False): 8}
    L = _lib.lib()
    assert L.mrt_selftest_instantiations(None, None, None, 0) == len(ROWS)                  # the count, whatever cap is
    f = np.full(8, 0xdeadbeef, np.uint32)
    assert L.mrt_selftest_instantiations(None, None, f.ctypes.data_as(C.POINTER(C.c_uint32)), 5) == len(ROWS)
    assert [int(v) for v in f[:5]] == [r[2] for r in ROWS[:5]] and (f[5:] == 0xdeadbeef).all()   # nothing written behind cap
    assert "mrt_selftest_instantiations" in _lib.SYMBOLS
    assert "mrt_selftest_instantiations" in open(os.path.join(ROOT, "include", "mrt.h")).read()
    for t, in_lds, feat in ROWS:        # the markers only where their shapes exist
        assert not (feat & F_NOSTASH) or (t == 1024 and in_lds and not feat & F_COLD)
        assert not (feat & F_DEEP) or (feat & F_COLD and feat & F_TRI)
        assert not (feat & F_COLD) or (in_lds and t != 64)
        assert not (feat & F_ENV) or feat & F_VATTR
        assert not (feat & F_VATTR) or (feat & F_ALL) == F_ALL


# ---- plan_launch: closed dispatch, complete recipes ------------------------------------------------------------------------------
def test_recipes_reach_every_row_and_the_dispatch_is_closed():
    table = set(ROWS)
    reached = 0
    for scene, targets in BY_SCENE.items():
        _, holder = IC.build(scene)
        for row, env in targets:
            assert IC.triple(IC.plan(holder, env)) == row, (IC.name_of(scene), env)
            reached += 1
        for env in IC.witnesses(scene, targets):
            assert IC.triple(IC.plan(holder, env)) in table, (IC.name_of(scene), env)
    # the rows no description reaches: the natural recipe lands on the row the entry names, and only the unreferenced texture of
    # the ABI-only recipe moves it
    assert set(IC.UNREACHABLE) <= table
    for row, (rule, lands) in IC.UNREACHABLE.items():
        natural = IC.recipe(*row)
        assert rule and natural.scene in BY_SCENE
        assert IC.triple(IC.plan(IC.build(natural.scene)[1], natural.env)) == lands != row, row
        assert lands in table
    for scene, targets in ABI_ONLY.items():
        for row, env in targets:
            assert IC.triple(IC.plan(IC.build(scene)[1], env)) == row, (IC.name_of(scene), env)
    assert reached + len(IC.UNREACHABLE) == len(ROWS) == _lib.lib().mrt_selftest_instantiations(None, None, None, 0)
    print(f"census: {len(ROWS)} compiled, {reached} with a recipe in {len(BY_SCENE)} scenes, {len(IC.UNREACHABLE)} unreachable "
          f"({len(ABI_ONLY)} scenes through the C ABI only)")


def test_the_pads_are_the_smallest_that_reach_the_unstashed_shape():
    """Every F_NOSTASH recipe: one unit less of padding and plan_launch picks another row."""
    padded = [s for s in BY_SCENE if s.pad]
    assert len(padded) == 10
    for scene in padded:
        (row, env), = BY_SCENE[scene]
        assert row[2] & F_NOSTASH
        less = IC.triple(IC.plan(IC.build(scene, IC.PAD[scene] - 1)[1], env))
        assert less != row and less in set(ROWS), (IC.name_of(scene), less)


# ---- oracle accumulators, shared ---------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_of(oracle_mod, scene):
    if scene not in _ORACLE:
        _ORACLE[scene] = IC.oracle_accums(oracle_mod, IC.build(scene)[1], threads=THREADS)
    return _ORACLE[scene]


def _linf(got, ref, spp):
    fin = np.isfinite(ref) & np.isfinite(got)
    return float(np.abs(got[fin] - ref[fin]).max()) / spp if fin.any() else 0.0


# ---- x86: the reduced feature sets ---------------------------------------------------------------------------------------------
def _bind(L):
    u32p, vp, u32 = C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32
    L.cs_error.restype = C.c_char_p
    L.cs_list.argtypes = [u32p, u32]
    L.cs_list.restype = u32
    L.cs_features.argtypes = [vp, vp, u32p]
    L.cs_render.argtypes = [vp, vp, u32, C.c_uint64, u32, u32, C.POINTER(C.c_float)]


@pytest.fixture(scope="session")
def census_probe():
    from emu.build import shared
    return shared("census_probe", _bind)


def _x86(L, holder, inst, spp):
    import env_ref as E
    nw, nh = E.ss_dims(holder)
    acc = np.zeros((nh, nw, 3), np.float32)
    rc = L.cs_render(C.cast(holder.ptr(), C.c_void_p), holder.ext_ptr(), inst, SEED, spp, THREADS, acc.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0, (inst, L.cs_error())
    return acc


def test_the_x86_census_builds_what_it_claims(census_probe):
    f = np.zeros(64, np.uint32)
    n = census_probe.cs_list(f.ctypes.data_as(C.POINTER(C.c_uint32)), 64)
    assert [int(v) for v in f[:n]] == X86_FEATS
    table = {r[2] for r in ROWS}
    assert set(X86_FEATS) <= table                       # each one is a compiled kernel's FEAT


@pytest.mark.parametrize("feat", X86_FEATS)
def test_reduced_feature_set_is_the_full_set_without_dead_code(feat, census_probe, oracle_mod):
    """The recipe scene of a reduced feature set through its own x86 build and through the full build (F_ALL, with F_BVH where the
    scene has the instance BVH): the same uint32 accumulator; and within the oracle's bar at 40 samples."""
    scene = IC.scene_for(feat)
    _, holder = IC.build(scene)
    info = np.zeros(2, np.uint32)
    assert census_probe.cs_features(C.cast(holder.ptr(), C.c_void_p), holder.ext_ptr(), info.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    assert int(info[0]) == scene.bits and bool(info[1]) == scene.ident        # the scene has exactly the row's features
    got = _x86(census_probe, holder, feat, SPP)
    full = _x86(census_probe, holder, F_ALL | (feat & F_BVH), SPP)
    ref = oracle_of(oracle_mod, scene)[SPP]
    same = float((got.view(np.uint32) == full.view(np.uint32)).all(-1).mean())
    print(f"x86 FEAT {feat}: L-inf against the oracle {_linf(got, ref, SPP):.2e}, {same:.2%} of the pixels bit-identical to the full build")
    assert np.array_equal(got.view(np.uint32), full.view(np.uint32))
    _check(got, ref, SPP)


@pytest.mark.parametrize("scene", SCENES, ids=IC.name_of)
def test_recipe_scene_meets_the_oracle_on_x86(scene, oracle_mod):
    """Every census scene through the x86 build of the full feature set at 32 and 40 samples, against the accumulators the GPU
    tests are held to."""
    import env_ref as E
    _, holder = IC.build(scene)
    ref = oracle_of(oracle_mod, scene)
    L = E.shared_probe()
    for spp in (SPP_LIST, SPP):
        got = E.x86_render(L, holder, SEED, spp, threads=THREADS)
        print(f"{IC.name_of(scene)} {spp} spp: L-inf against the oracle {_linf(got, ref[spp], spp):.2e}")
        _check(got, ref[spp], spp)
    assert not np.array_equal(ref[SPP_LIST], ref[SPP])


# ---- the GPU: every row as itself ----------------------------------------------------------------------------------------------------
_RAN = {"uniform": set(), "list": set(), "worst": {}}


def _sampler(scene, monkeypatch):
    from micro_raytracer_amd import Sampler
    if scene.unref:                                      # the Sampler flattens the render itself: give it the holder with the extra texture
        monkeypatch.setattr(_abi, "build_desc", lambda render: IC.holder_of(render, scene))
    return Sampler(seed=SEED)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", SCENES, ids=IC.name_of)
def test_every_row_of_a_scene_runs_as_itself(scene, oracle_mod, monkeypatch):
    """Per row of the scene: 40 uniform samples and a 32-sample tile-list run (mrt_execute_adaptive, threshold 0) under the row's
    switches.  stats() reports exactly the row; both accumulators meet the oracle; every uniform run has the bits of the first,
    every list run those of a 32-sample uniform run; sample_counts is 32 everywhere."""
    render, _ = IC.build(scene)
    targets = ALL_SCENES[scene]
    ref = oracle_of(oracle_mod, scene)
    table = set(ROWS)
    first40 = first32 = None
    with IC.switches(targets[0][1]):
        s = _sampler(scene, monkeypatch)
        s.execute(render, n_samples=SPP_LIST)
        first32 = s.accum()[0]
        s.close()
    _check(first32, ref[SPP_LIST], SPP_LIST)
    runs = [(row, env) for row, env in targets] + [(None, env) for env in IC.witnesses(scene, targets)]
    for row, env in runs:
        with IC.switches(env):
            s = _sampler(scene, monkeypatch)
            s.execute(render, n_samples=SPP)
            got, cnt = s.accum()
            st = s.stats()
            s.close()
        ran = IC.triple(st)
        assert cnt == SPP and ran in table and (row is None or ran == row), (env, ran, row)
        if first40 is None:
            first40 = got
        same = float((got.view(np.uint32) == first40.view(np.uint32)).all(-1).mean())
        err = _linf(got, ref[SPP], SPP)
        print(f"{IC.name_of(scene)} {ran} pt_megakernel: k_split {st['k_split']}, lds_bytes {st['lds_bytes']}, L-inf {err:.2e}, "
              f"bit-identical {same:.2%}" + ("" if row else " (witness)"))
        _check(got, ref[SPP], SPP)
        assert np.array_equal(got.view(np.uint32), first40.view(np.uint32)), (env, ran)
        if row is None:
            continue
        _RAN["uniform"].add(row)
        with IC.switches(env):
            s = _sampler(scene, monkeypatch)
            s.execute_adaptive(render, 0.0, min_samples=SPP_LIST, max_samples=SPP_LIST, step=16)
            got, _ = s.accum()
            counts = s.sample_counts()
            st = s.stats()
            s.close()
        assert IC.triple(st) == row, (env, IC.triple(st))
        same_l = float((got.view(np.uint32) == first32.view(np.uint32)).all(-1).mean())
        err_l = _linf(got, ref[SPP_LIST], SPP_LIST)
        print(f"{IC.name_of(scene)} {row} pt_megakernel over a tile list: k_split {st['k_split']}, lds_bytes {st['lds_bytes']}, L-inf {err_l:.2e}, "
              f"bit-identical {same_l:.2%}")
        assert (counts == SPP_LIST).all()
        _check(got, ref[SPP_LIST], SPP_LIST)
        assert np.array_equal(got.view(np.uint32), first32.view(np.uint32)), (env, row)
        _RAN["list"].add(row)
        w = _RAN["worst"].setdefault((row[0], row[1]), [0.0, 1.0, 0])
        w[0], w[1], w[2] = max(w[0], err, err_l), min(w[1], same, same_l), w[2] + 1


@pytest.mark.gpu
def test_census_closing_line():
    """After the scenes above (it needs them all to have run in this process): every row that is not UNREACHABLE ran as itself
    through both kernels, and so did the UNREACHABLE ones through the C ABI."""
    for shape, (err, same, n) in sorted(_RAN["worst"].items()):
        print(f"census shape {shape}: {n} rows run, worst L-inf {err:.2e}, lowest bit-identical share {same:.2%}")
    print(f"census: {len(ROWS)} compiled, {len(_RAN['uniform'])} run as pt_megakernel, {len(_RAN['list'])} run over a tile list, "
          f"{len(IC.UNREACHABLE)} unreachable by a scene description (run through the C ABI)")
    assert _RAN["uniform"] == _RAN["list"] == set(ROWS)
