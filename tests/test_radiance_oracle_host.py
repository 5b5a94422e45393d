"""mrt_radiance against the oracle, CPU side: the x86 build of pt_rays' per-ray body (csrc/mrt_rays.h through
tests/emu/rays_probe.cpp) against orc_radiance (oracle/mrt_oracle.c: the reference's path loop and fold on a ray handed in, no
text shared with csrc/), on the cases of tests/radiance_cases.py -- every one of the eight feature sets of pt_rays, rays with
zero, infinite and NaN components, origins on and inside surfaces, tangents, ties -- and the two anchors that tie orc_radiance to
what the oracle already answered for: the accumulator of orc_execute and orc_trace_pixel.

Rule (radiance_cases.compare), per ray and per component on the sums: NaN and infinity positions equal, signs of infinities
equal, elsewhere |got - ref| <= 1e-4 * max(n_samples, |ref|).  The probe's segment total equals the oracle's count under the
kernel's stop rule, exactly.  Exclusions: none; the excluded share is asserted to be 0."""
import os

import numpy as np
import pytest

import radiance_cases as RC
import rayq_cases as Q
import rays_ref as Y
from conftest import make_holder

f32 = np.float32
SEED = 3
MAX_EXCLUDED_SHARE = 0.0


@pytest.fixture(scope="module")
def probe():
    return Y.shared_probe()


def excluded(case):
    """The exclusion rule, on the input alone: no ray is excluded."""
    return np.zeros(case.o.shape[0], bool)


def permuted_keys(n):
    """A key array that is no ray's index: a seeded permutation of n distinct 32-bit words, top bit included."""
    rng = np.random.default_rng(n)
    return (rng.permutation(n).astype(np.uint32) * np.uint32(2654435761) + np.uint32(0x80000001)).astype(np.uint32)


def plan_under(monkeypatch, holder, env):
    from micro_raytracer_amd import _lib
    for k in [k for k in os.environ if k.startswith("MRT_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pl = _lib.plan_launch(holder)
    for k in env:
        monkeypatch.delenv(k)
    return pl


_ORACLE = {}


def oracle_sums(oracle_mod, holder, case, base, ns, keyed):
    """(sums, segments) of orc_radiance, computed once per (case, range, keys) of a process and left unchanged."""
    k = (case.name, base, ns, keyed)
    if k not in _ORACLE:
        orc = oracle_mod.Oracle(holder, seed=SEED)
        _ORACLE[k] = orc.radiance(case.o, case.d, ns, sample_base=base, key=permuted_keys(len(case.o)) if keyed else None)
        orc.close()
    return _ORACLE[k]


def _first_hits(oracle_mod, holder, case):
    orc = oracle_mod.Oracle(holder, seed=SEED)
    q = orc.ray_query(case.o, case.d)
    orc.close()
    return q


def _case_names():
    # the table's names without building it (collection must not render anything)
    return ["axis/six_planes", "surface/kitchen_sink_no_triangles", "surface/kitchen_sink", "mesh/mesh_kind1", "mesh/mesh_kind2", "mesh/mesh_kind3",
            "shading/kitchen_sink_plus", "mesh/mesh_kind0", "mesh/mesh_kind4", "ties/instance_grid", "ties/coincident_bvh", "ties/crowd_scene_3",
            "mesh/mesh_three_rotated_instances_crowd", "attributes/triangles", "attributes/smooth", "extra/triangles_crowd", "extra/smooth_crowd",
            "extra/triangles_env_sphere_bilinear", "attributes/env_sphere_nearest", "extra/triangles_crowd_env_latlong_nearest",
            "extra/env_sphere_bilinear_crowd"]


def test_the_table_is_what_the_names_say(oracle_mod):
    table = RC.cases(oracle_mod)
    assert [c.name for c in table] == _case_names()
    assert {c.feat for c in table} == set(RC.FEATS)
    # both kernels of every feature set have a case that expects them
    assert {(c.feat, r.lds) for c in table for r in c.runs} == {(f, l) for f in RC.FEATS for l in (True, False)}


@pytest.mark.parametrize("name", _case_names())
def test_case_through_the_x86_probe_meets_the_oracle(probe, oracle_mod, monkeypatch, name):
    case = RC.case(name, oracle_mod)
    _, holder = make_holder(case.desc)
    info = Y.x86_info(probe, holder)
    assert info["rays_inst"] == case.feat, (name, info)
    assert case.desc["frame"]["res"] == [16, 16]
    # the environments of the case put the scene where the table says: what the GPU test will find in mrt_rays_info
    for run in case.runs:
        pl = plan_under(monkeypatch, holder, run.env)
        staged = pl["staging"] == "all" and pl["staged_bytes"] <= RC.LDS_QUARTER
        assert staged == run.lds, (name, run.label, pl["staging"], pl["staged_bytes"], info["lds_words"] * 4)
    q = _first_hits(oracle_mod, holder, case)
    share = float(q[:, 0].mean())
    assert share >= 0.30, (name, share)
    ex = excluded(case)
    assert ex.sum() / len(ex) <= MAX_EXCLUDED_SHARE and ex.sum() == 0
    n, n_wild = len(case.o), int(Q.wild(case.o, case.d).sum())
    ranges = RC.RANGES + ((RC.TOP_RANGE,) if name.startswith("shading/") else ())
    for base, ns in ranges:
        for keyed in (False, True):
            key = permuted_keys(n) if keyed else None
            ref, rseg = oracle_sums(oracle_mod, holder, case, base, ns, keyed)
            feats = [info["rays_inst"]] + ([info["own_inst"]] if not keyed and info["own_inst"] != info["rays_inst"] else [])
            for feat in feats:
                got, seg = Y.x86_radiance(probe, holder, feat, case.o, case.d, ns, seed=SEED, sample_base=base, key=key, segments=True)
                bad, worst, same, nonfin = RC.compare(got, ref, ns)
                print(f"radiance, x86 probe vs oracle: {name:44s} FEAT {feat:4d} samples [{base}, +{ns}) keys {'permuted' if keyed else 'index   '} rays {n:4d} "
                      f"hit share {share:.2f} wild {n_wild:3d} non-finite {nonfin:3d} worst {worst:.2e} bit-identical {same:.4f} segments {seg} (oracle {int(rseg.sum())})")
                assert bad.size == 0, (name, feat, base, ns, keyed, [(int(i), case.o[i], case.d[i], got[i], ref[i]) for i in bad[:3]])
                assert seg == int(rseg.sum()), (name, feat, base, ns, keyed, seg, int(rseg.sum()))
                assert seg >= n * ns


# ---- the anchors of orc_radiance -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "lights", "primitives", "env_vattr"])
def test_orc_radiance_on_the_cameras_rays_gives_the_accumulator_of_orc_execute(probe, oracle_mod, name):
    """(a) aprt 0: every sample of a pixel is the lens-centre ray, (u - 0.5) * 0 added to a camera coordinate leaves its bits, and
    the lens draws that orc_radiance does not take decide nothing.  The sums, added sample by sample, are the accumulator's bits."""
    render, holder = Y.frame_case(name)
    assert render.frame.cam.aprt == 0
    o, d = (a.reshape(-1, 3) for a in Y.x86_camera_rays(probe, holder))
    orc = oracle_mod.Oracle(holder, seed=Y.SEED)
    orc.execute(Y.SPP, threads=8)
    acc = orc.accum()[0].reshape(-1, 3).copy()
    total = orc.segments
    sums, seg = orc.radiance(o, d, Y.SPP)
    orc.close()
    diff = int((RC.bits(sums) != RC.bits(acc)).any(axis=1).sum())
    print(f"orc_radiance on the camera's rays, {name}: {diff} of {len(acc)} pixels differ from orc_execute; segments {int(seg.sum())} under the kernel's rule, "
          f"{total} traced by the reference")
    assert diff == 0
    assert len(acc) * Y.SPP <= int(seg.sum()) <= total


@pytest.mark.parametrize("s", [0, 17, 2 ** 32 - 2])
def test_orc_radiance_of_one_keyed_sample_is_orc_trace_pixel(probe, oracle_mod, s):
    """(b) key = [k], sample_base = s, one sample, on pixel k's camera ray: the bits of trace_pixel(x, y, s)."""
    for name in ("cornell", "env_vattr"):
        render, holder = Y.frame_case(name)
        o, d = Y.x86_camera_rays(probe, holder)
        nh, nw = o.shape[:2]
        orc = oracle_mod.Oracle(holder, seed=Y.SEED)
        rng = np.random.default_rng(7)
        for x, y in zip(rng.integers(0, nw, 40), rng.integers(0, nh, 40)):
            k = int(y) * nw + int(x)
            sums, seg = orc.radiance(o[y, x][None], d[y, x][None], 1, sample_base=s, key=[k])
            want, total = orc.trace_pixel(int(x), int(y), s)
            assert np.array_equal(RC.bits(sums[0]), RC.bits(want)), (name, x, y, s, sums[0], want)
            assert 1 <= int(seg[0]) <= total
        orc.close()


def test_segments_stop_at_the_first_emitting_hit(oracle_mod):
    """The count under the kernel's rule: a ray that hits the emit-1 sphere first is one segment per sample, whatever the
    reference traces behind it; a ray into the empty sky is one segment too."""
    case = RC.case("shading/kitchen_sink_plus", oracle_mod)
    _, holder = make_holder(case.desc)
    q = _first_hits(oracle_mod, holder, case)
    emit_r = len(case.desc["scene"]["renderer"]) - 2
    on_emit = (q[:, 0] == 1) & (q[:, 2] == emit_r)
    miss = q[:, 0] == 0
    assert on_emit.sum() >= 100 and miss.sum() >= 20
    _, seg = oracle_sums(oracle_mod, holder, case, 7, 24, False)
    assert (seg[on_emit] == 24).all() and (seg[miss] == 24).all()
    assert (seg[~on_emit & ~miss] > 24).mean() > 0.9


# ---- the shading family holds what it claims -------------------------------------------------------------------------------------------
def test_shading_family_holds_what_it_claims(oracle_mod):
    case = RC.case("shading/kitchen_sink_plus", oracle_mod)
    _, holder = make_holder(case.desc)
    q = _first_hits(oracle_mod, holder, case)
    hit = q[:, 0] == 1
    t0, t1 = q[:, 4].view(f32), q[:, 5].view(f32)
    rend = case.desc["scene"]["renderer"]
    glass = [ri for ri, r in enumerate(rend) if r["type"] == "sphere" and r["mat"].get("glass")]
    assert len(glass) == 1 and len(rend[glass[0]]["inst"]) == 2
    for ii in range(2):
        on = hit & (q[:, 2] == glass[0]) & (q[:, 3] == ii)
        # Origins inside the glass, t0 < 0 < t1: stated on the line's two roots against the sphere, in float64 from the
        # description.  No REPORTED t0 can be negative: the reference's sphere answers None when its near root is below zero
        # (sphere_intersect, src/rt.rs:350-355), so a ray from inside misses the sphere it starts in -- asserted here too, since
        # that is the rule a path meets when a scattered ray starts inside the glass.
        c, rad = np.asarray(rend[glass[0]]["inst"][ii][0], np.float64), float(rend[glass[0]]["r"])
        oc, dd = case.o.astype(np.float64) - c, case.d.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            a, b, cc = (dd * dd).sum(1), 2.0 * (oc * dd).sum(1), (oc * oc).sum(1) - rad * rad
            disc = b * b - 4.0 * a * cc
            r0, r1 = (-b - np.sqrt(disc)) / (2.0 * a), (-b + np.sqrt(disc)) / (2.0 * a)
            inside = np.isfinite(r0) & np.isfinite(r1) & (r0 < 0) & (r1 > 0)
        print(f"shading family: glass sphere instance {ii}: {int(on.sum())} first hits, {int(inside.sum())} rays with roots t0 < 0 < t1 "
              f"(origin inside), {int((inside & on).sum())} of those answered by the sphere itself")
        assert on.sum() >= 100 and inside.sum() >= 50
        assert (inside & on).sum() == 0 and not (t0[on] < 0).any()
    emit_r, box_r = len(rend) - 2, len(rend) - 1
    assert rend[emit_r]["mat"]["emit"] == 1.0 and rend[box_r]["mat"]["opacity"] == 0.0 and rend[box_r]["mat"]["glass"] == 0.5
    floor = next(ri for ri, r in enumerate(rend) if r["type"] == "plane")
    counts = {k: int((hit & (q[:, 2] == ri)).sum()) for k, ri in (("emit-1 sphere", emit_r), ("opacity-0 box", box_r), ("floor", floor))}
    n_wild = int(Q.wild(case.o, case.d).sum())
    print(f"shading family: {len(case.o)} rays, first hits {counts}, wild {n_wild}")
    assert counts["emit-1 sphere"] >= 100 and counts["opacity-0 box"] >= 100 and counts["floor"] >= 300 and n_wild >= 100
    light = np.asarray(case.desc["scene"]["light"][-1]["pos"], np.float64)
    assert light[2] == rend[floor]["pos"][2]                                  # the light lies in the floor's plane
    # floor hits at texel boundaries (c) and near the in-plane light (d)
    on_floor = hit & (q[:, 2] == floor) & np.isfinite(t0)
    p = case.o[on_floor].astype(np.float64) + case.d[on_floor].astype(np.float64) * t0[on_floor, None]
    on_line = (np.abs(p[:, :2] * 8 - np.round(p[:, :2] * 8)) < 1e-4).any(axis=1)
    near = np.linalg.norm(p - light, axis=1) < 0.5
    print(f"shading family: {int(on_line.sum())} floor hits on a line x = k/8 or y = k/8 ({int((on_line & (p[:, :2] < 0).any(axis=1)).sum())} at a negative "
          f"coordinate), {int(near.sum())} within 0.5 of the in-plane light")
    assert on_line.sum() >= 200 and (on_line & (p[:, :2] < 0).any(axis=1)).sum() >= 50 and near.sum() >= 150
