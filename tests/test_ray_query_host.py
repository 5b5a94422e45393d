"""Closest-hit queries on caller-supplied rays, CPU side: the x86 build of the device hook's per-ray body (csrc/mrt_rayq.h through
tests/emu/rayq_probe.cpp) against the oracle's orc_ray_query (oracle/mrt_oracle.c: RayTracer::closest_hit on the ray as given,
written from the reference's structure, no text shared with csrc/), on the ray families of tests/rayq_cases.py.

Rule (test_oracle_aov.compare_aov's): hit, any, renderer and instance equal; t0, t1 and the world normal bit-equal, NaN equal to
NaN.  Exclusions: none -- measured before anything was excluded, rays with zero, infinite and NaN components included, the two
sides agree on every ray of every family ("ray queries"), so the excluded share is asserted to be 0."""
import os

import numpy as np
import pytest

import rayq_cases as R
from conftest import make_holder

f32 = np.float32
MAX_EXCLUDED_SHARE = 0.01          # the issue's ceiling; the rule below excludes nothing


@pytest.fixture(scope="module")
def probe():
    return R.shared_probe()


def excluded(case):
    """The exclusion rule, on the input alone: no ray is excluded."""
    return np.zeros(case.o.shape[0], bool)


def _plan(monkeypatch, holder, variant):
    from micro_raytracer_amd import _lib
    for k in [k for k in os.environ if k.startswith("MRT_")]:
        monkeypatch.delenv(k)
    for k, v in variant.env.items():
        monkeypatch.setenv(k, v)
    pl = _lib.plan_launch(holder)
    for k in variant.env:
        monkeypatch.delenv(k)
    return pl


def oracle_answers(oracle_mod, holder, case):
    orc = oracle_mod.Oracle(holder, seed=1)
    ref = orc.ray_query(case.o, case.d)
    orc.close()
    return ref


@pytest.mark.parametrize("fam", list(R.FAMILIES))
def test_family_through_the_x86_probe_equals_the_oracle(probe, oracle_mod, monkeypatch, fam):
    rays = hits = n_excl = worst = 0
    for case in R.family(fam, oracle_mod):
        _, holder = make_holder(case.desc)
        ref = oracle_answers(oracle_mod, holder, case)
        ex = excluded(case)
        assert (ref[:, 0] == ref[:, 1]).all(), case.name                      # the shadow query answers Some exactly where the closest hit does
        assert ref[:, 0].mean() >= 0.30, (case.name, ref[:, 0].mean())
        rays += len(ref); hits += int(ref[:, 0].sum()); n_excl += int(ex.sum())
        for v in case.variants:
            pl = _plan(monkeypatch, holder, v)
            if v.feat is None:
                v.feat = pl["kernel_features"]                                # (the random crowd: whatever the plan says, one of the hook's list)
            # the environment of the variant selects the instantiation the probe runs: what the GPU test will find in mrt_stats
            assert (pl["kernel_features"], pl["staging"] != "none", pl["block_threads"]) == (v.feat, v.lds, 256), (case.name, v.label, pl)
            got, _ = R.probe_trace(probe, holder, v.cfg(), case.o, case.d)
            assert (got[:, 0] == got[:, 1]).all(), (case.name, v.label)
            bad = np.flatnonzero(~R.same_words(got, ref) & ~ex)
            u = R.ulp_distance(got, ref)
            worst = max(worst, u)
            print(f"ray queries, x86 probe vs oracle: {fam:10s} {case.name:36s} {v.label:14s} FEAT {v.feat:4d} rays {len(ref):5d} "
                  f"hits {int(ref[:, 0].sum()):5d} excluded {int(ex.sum())} worst ulp {u} disagreeing {bad.size}")
            assert bad.size == 0, (case.name, v.label, [(case.o[i], case.d[i], got[i], ref[i]) for i in bad[:3]])
    share = n_excl / rays
    print(f"ray queries, family {fam}: rays {rays} hits {hits} ({hits / rays:.1%}) excluded share {share:.4%} worst ulp {worst}")
    assert share <= MAX_EXCLUDED_SHARE and share == 0.0
    assert hits >= 0.30 * rays


def test_axis_family_holds_the_rays_the_window_guards(oracle_mod):
    """The family reaches both sides of every guard of the axis body: tame rays, rays outside the window, numerators below 2^-40."""
    from test_axis_scan import _tame
    case = R.family("axis", oracle_mod)[0]
    tame = _tame(case.o, case.d)
    assert tame.sum() > 3000 and (~tame).sum() > 100
    assert R.wild(case.o, case.d).sum() > 100


def test_axis_body_on_and_off_bit_equal(probe, oracle_mod):
    from test_axis_scan import _tame
    for case in R.family("axis", oracle_mod):
        _, holder = make_holder(case.desc)
        v = case.variants[0]
        on, n_on = R.probe_trace(probe, holder, v.cfg(axis=1), case.o, case.d)
        off, n_off = R.probe_trace(probe, holder, v.cfg(axis=0), case.o, case.d)
        assert not n_off.any()
        assert np.array_equal(n_on != 0, _tame(case.o, case.d))               # the axis body answers exactly the rays its guard admits
        assert np.array_equal(on, off), case.name


def test_mesh_walks_bit_equal(probe, oracle_mod):
    """Binary table (whole scene in LDS; warm, its leaf queue at 8 and 16 entries), 4-wide table (walk areas of 4 and 16 entries)
    and the reference's octree walk: the same words, no exclusions."""
    V = R.Variant
    for case in R.family("mesh", oracle_mod):
        bvh = case.variants[0].feat & R.F_BVH
        _, holder = make_holder(case.desc)
        base = V("lds all", R.F_ALL | bvh)
        want, _ = R.probe_trace(probe, holder, base.cfg(), case.o, case.d)
        others = [V("warm 8", R.F_ALL | bvh | R.F_COLD, walk_cap=8), V("warm 16", R.F_ALL | bvh | R.F_COLD, walk_cap=16),
                  V("deep 4", R.F_ALL | bvh | R.F_COLD | R.F_DEEP, wide=1, hot=1, walk_cap=4),
                  V("deep 16", R.F_ALL | bvh | R.F_COLD | R.F_DEEP, wide=1, hot=1000000, walk_cap=16)]
        if bvh:
            others = others[2:]                                                # (the hook has no warm kernel with the instance BVH)
        for v in others:
            got, _ = R.probe_trace(probe, holder, v.cfg(), case.o, case.d)
            assert np.array_equal(got, want), (case.name, v.label)
        if not bvh:                                                            # (d.d = NaN would reach the crowd's spheres too)
            got, _ = R.probe_trace(probe, holder, base.cfg(ref_walk=1), case.o, case.d)
            assert np.array_equal(got, want), (case.name, "reference walk")


def test_ties_family_has_equal_distance_candidates_and_the_first_wins(probe, oracle_mod):
    """From the oracle's answers: the scene without the FIRST member of every coincident group answers the same t0 bits with the
    next member -- the two best candidates were equal, and the earlier flat index won."""
    import copy
    case = next(c for c in R.family("ties", oracle_mod) if c.name == "coincident_linear")
    rend = case.desc["scene"]["renderer"]
    n0 = len(rend) - 5                                                         # the five renderers of rayq_cases._dup_renderers
    _, holder = make_holder(case.desc)
    ref = oracle_answers(oracle_mod, holder, case)
    less = copy.deepcopy(case.desc)
    lr = less["scene"]["renderer"]
    lr[n0]["inst"] = lr[n0]["inst"][1:]
    lr[n0 + 1]["inst"] = lr[n0 + 1]["inst"][1:]
    del lr[n0 + 3]
    _, holder2 = make_holder(less)
    ref2 = oracle_answers(oracle_mod, holder2, R.Case("less", less, case.o, case.d, []))
    first = (ref[:, 0] == 1) & (ref[:, 3] == 0) & np.isin(ref[:, 2], [n0, n0 + 1, n0 + 3])
    tie = first & (ref2[:, 0] == 1) & (ref2[:, 4] == ref[:, 4]) & np.isfinite(ref[:, 4].view(f32))
    # ... and the runner-up is the group's next member: the same renderer's next instance (now its first), or the coinciding renderer
    nxt = np.where(ref[:, 2] == n0 + 3, n0 + 3, ref[:, 2])                      # (renderer n0 + 4 moved down by one)
    tie &= (ref2[:, 2] == nxt) & (ref2[:, 3] == 0)
    print(f"ray queries, ties: {int(tie.sum())} rays whose two best candidates have equal t0 bits, of {int(first.sum())} won by a group's first member")
    assert tie.sum() >= 100
    assert (first & ~tie).sum() == 0                                           # a first member never wins by anything but the order
    # no ray is ever won by a later member of a group: instance > 0 of the coincident lists, or the second of the twin renderers
    later = (ref[:, 0] == 1) & (((ref[:, 3] > 0) & np.isin(ref[:, 2], [n0, n0 + 1, n0 + 2])) | np.isin(ref[:, 2], [n0 + 2, n0 + 4]))
    assert later.sum() == 0
    got, _ = R.probe_trace(probe, holder, case.variants[0].cfg(), case.o, case.d)
    assert np.array_equal(got[tie, :4], ref[tie, :4])
