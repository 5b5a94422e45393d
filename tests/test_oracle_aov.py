"""The first-hit AOVs (mrt_aov, DESIGN.md §13 with the additions of §14-§16) held to the CPU oracle's orc_aov, which is written
from the contract text and shares no code with csrc/mrt_denoise.h or csrc/mrt_trace.h:

a. the oracle's AOVs against float64 closest hits (test_denoise_host.np_first_hits, and a sibling with a rotated box and a sphere
   under rotated instances, so that the instance rotation of a normal is anchored to something that is neither the kernel
   nor the oracle);
b. the oracle against the x86 build of aov_pixel (tests/emu/denoise_probe.cpp for plain scenes, env_probe.cpp's ev_aov for scenes
   with an ext) on whole frames, no pixel excluded: hit masks and ids equal, depth, normal, world point and albedo BIT-EQUAL.
   The scenes: every one of test_gpu_parity.SCENES and test_oracle_ext.SCENES, 68 seeds of the plain fuzz and the extension fuzz
   of test_fuzz_scenes.ext_scene.

tests/test_gpu_oracle_aov.py runs (b) on the GPU with the same comparison."""
import os

import numpy as np
import pytest

import env_ref as E
import test_denoise_host as D
from conftest import make_holder
from micro_raytracer_amd._abi import F_BVH

f32 = np.float32
THREADS = min(16, os.cpu_count() or 1)
FLOAT_PLANES = ("depth", "normal", "point", "albedo")

# (fuzz family, seed) of the plain fuzz: random_scene 0..39, crowd_scene 0..7, ident_scene 0..9, mesh_fuzz_scene 0..9
FUZZ = [("random", k) for k in range(40)] + [("crowd", k) for k in range(8)] + [("ident", k) for k in range(10)] + [("mesh", k) for k in range(10)]


@pytest.fixture(scope="module")
def probes():
    return D.shared_probe(), E.shared_probe()


def fuzz_desc(family, seed):
    import test_fuzz_scenes as Z
    return getattr(Z, {"random": "random_scene", "crowd": "crowd_scene", "ident": "ident_scene", "mesh": "mesh_fuzz_scene", "ext": "ext_scene"}[family])(seed)


def named_scenes():
    """name -> builder of a scene dict: the 14 scenes of test_gpu_parity.SCENES and the 16 of test_oracle_ext.SCENES."""
    from micro_raytracer_amd import scenes
    import test_gpu_parity as P
    import test_oracle_ext as X
    out = {f"parity:{n}": (lambda b=b: b(scenes)) for n, b in P.SCENES.items()}
    out.update({f"ext:{n}": v[0] for n, v in X.SCENES.items()})
    return out


NAMED = list(named_scenes())


def x86_planes(probes, holder):
    """The x86 AOV pass as Sampler.aov()'s planes plus the world point and the hit flag: denoise_probe's dn_aov for a plain
    scene, env_probe's ev_aov_inst (which takes any ext) for the others."""
    dn, ev = probes
    if holder.ext_ptr() is None:
        nw, nh = E.ss_dims(holder)
        g, alb, rend, inst = D.x86_aov(dn, holder, nw, nh)
    else:
        g, alb, rend, inst = E.x86_aov_inst(ev, holder)
    return {"depth": g[..., 3], "normal": g[..., 0:3], "point": g[..., 4:7], "albedo": alb, "renderer": rend, "instance": inst,
            "hit": g[..., 7] != 0}


def ulps(a, b):
    """Worst distance of a from b in units of b's last place (0 where the bits, or both NaNs, or both infinities agree)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    if same.all():
        return 0.0
    with np.errstate(all="ignore"):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(b), f32(1e-30))).astype(np.float64)
    d = np.where(same, 0.0, np.where(np.isfinite(d), np.maximum(d, 1.0), np.inf))      # -0 against +0 counts as one
    return float(d.max())


def compare_aov(label, got, ref):
    """got (a kernel side: x86 or GPU) against ref (Oracle.aov()) on the whole frame.  The bar the CPU comparison ended with:
    every float plane bit-equal, NaN patterns included; hit masks and ids equal.  Returns the printed figures."""
    assert got["depth"].shape == ref["depth"].shape, label
    hit_ref = ref["renderer"] >= 0
    hit_got = got["hit"] if "hit" in got else got["renderer"] >= 0
    fig = {k: ulps(got[k], ref[k]) for k in FLOAT_PLANES if k in got}
    ids = int(np.count_nonzero(got["renderer"] != ref["renderer"]))
    if "instance" in got:
        ids += int(np.count_nonzero(got["instance"] != ref["instance"]))
    print(f"{label}: {ref['depth'].size} pixels, {int(hit_ref.sum())} hits, id mismatches {ids}, worst ulp " +
          ", ".join(f"{k} {v:.0f}" for k, v in fig.items()))
    assert np.array_equal(hit_got, hit_ref) and np.array_equal(np.isinf(got["depth"]), ~hit_ref), label
    assert np.array_equal(got["renderer"], ref["renderer"]), label
    if "instance" in got:
        assert np.array_equal(got["instance"], ref["instance"]), label
    assert np.all(ref["instance"][~hit_ref] == -1) and np.all((ref["instance"] >= 0) == hit_ref), label
    for k, v in fig.items():
        assert v == 0.0, (label, k, v)
    return fig, ids


def oracle_aov(oracle_mod, holder):
    o = oracle_mod.Oracle(holder)
    a = o.aov()
    assert (o.nw, o.nh) == E.ss_dims(holder)
    o.close()
    return a


# ---- a. the oracle against float64 ---------------------------------------------------------------------------------------------------
def _rot64(q):
    """The instance transform of src/rt.rs:726-727 in float64: rotate_y(-dir) . lookat(-dir, +z) (src/lin.rs:175-183, 197-208)."""
    w, x, y, z = (-float(c) for c in q)
    fwd = np.array([x, y, z]) / np.linalg.norm([x, y, z])
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    look = np.array([[right[0], -right[1], right[2]], [-fwd[0], fwd[1], -fwd[2]], [up[0], -up[1], up[2]]])
    cw = np.sqrt(1.0 - w * w)
    return np.array([[cw, 0.0, w], [0.0, 1.0, 0.0], [-w, 0.0, cw]]) @ look


def _rotated_scene():
    """A floor, one rotated box and a sphere under two rotated instances (and one unrotated), seen by a rotated camera at
    ssaa 1.5."""
    return {
        "rt": {"sample": 1, "bounce": 2},
        "frame": {"res": [47, 31], "ssaa": 1.5, "cam": {"pos": [0.1, -1.6, 0.25], "dir": [0.1, 0.15, 1, -0.2], "fov": 65}},
        "scene": {"renderer": [
            {"type": "plane", "n": [0, 0, 1], "pos": [0, 0, -0.4], "mat": {"albedo": "#808080"}},
            {"type": "box", "sizes": [0.5, 0.35, 0.3], "pos": [0.45, 0.3, -0.05], "dir": [0.3, 0.5, 1, -0.25], "mat": {"albedo": "#20c040"}},
            {"type": "sphere", "r": 0.22, "mat": {"albedo": "#ff0000"},
             "inst": [[[-0.5, 0.2, 0.0], [0.4, 0.2, -1, 0.3]], [[-0.1, 0.3, 0.35], [-0.6, 1, 0.2, 0.1]], [[-0.1, -0.2, -0.15], [0, 0, -1, 0]]]},
        ]},
    }


def np_first_hits_rotated(render):
    """np_first_hits' sibling for rotated instances and a rotated camera, float64: depth, normal, renderer, instance.  The ray in
    object space is pos + M (o - pos), M d (src/rt.rs:726-737); the object-space normal goes through the SAME matrix once more
    and is normalised (src/rt.rs:776-793)."""
    fr = render.frame
    cam = fr.cam
    w, h = f32(f32(fr.res[0]) * f32(fr.ssaa)), f32(f32(fr.res[1]) * f32(fr.ssaa))
    nw, nh = int(w), int(h)
    aspect = float(w) / float(h)
    inv2tan = 1.0 / (2.0 * np.tan(np.radians(cam.fov / 2.0)))
    yy, xx = np.mgrid[0:nh, 0:nw].astype(np.float64)
    d = np.stack([aspect * (xx - 0.5 * float(w)) / float(w), np.full_like(xx, inv2tan), -(yy - 0.5 * float(h)) / float(h)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    # the lens centre: the focus point lies on the ray, so the new direction is d again; then lookat and rotate_y of cam.dir
    cw, cx, cy, cz = (float(c) for c in cam.dir)
    fwd = np.array([cx, cy, cz]) / np.linalg.norm([cx, cy, cz])
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    look = np.array([[right[0], -right[1], right[2]], [-fwd[0], fwd[1], -fwd[2]], [up[0], -up[1], up[2]]])
    sw = np.sqrt(1.0 - cw * cw)
    d = d @ (np.array([[sw, 0.0, cw], [0.0, 1.0, 0.0], [-cw, 0.0, sw]]) @ look).T
    o = np.asarray(cam.pos, np.float64) + d * 1e-4
    best = np.full((nh, nw), np.inf)
    nrm = np.zeros((nh, nw, 3))
    rid = np.full((nh, nw), -1, np.int32)
    iid = np.full((nh, nw), -1, np.int32)
    for r, rd in enumerate(render.scene.renderer):
        for i, (pos, q) in enumerate(rd.inst):
            pos = np.asarray(pos, np.float64)
            M = _rot64(q)
            lo, ld = (o - pos) @ M.T, d @ M.T
            if rd.kind == "plane":
                n = np.asarray(rd.n, np.float64) / np.linalg.norm(rd.n)
                with np.errstate(all="ignore"):
                    t = np.nan_to_num(-(lo @ n) / (ld @ n), nan=-1.0)
                n_obj = np.broadcast_to(n, d.shape)
            elif rd.kind == "sphere":
                b = np.sum(lo * ld, -1)
                disc = b * b - (np.sum(lo * lo, -1) - rd.r ** 2)
                t = np.where(disc >= 0, -b - np.sqrt(np.maximum(disc, 0)), -1.0)
                n_obj = lo + ld * t[..., None]
            else:
                half = 0.5 * np.asarray(rd.sizes, np.float64)
                with np.errstate(divide="ignore", invalid="ignore"):
                    t1, t2 = (-half - lo) / ld, (half - lo) / ld
                tn, tf = np.max(np.minimum(t1, t2), -1), np.min(np.maximum(t1, t2), -1)
                t = np.where((tn <= tf) & (tf > 0), tn, -1.0)
                qn = (lo + ld * t[..., None]) / half
                ax = np.argmax(np.abs(qn), -1)
                n_obj = np.zeros_like(qn)
                np.put_along_axis(n_obj, ax[..., None], np.sign(np.take_along_axis(qn, ax[..., None], -1)), -1)
            n = n_obj @ M.T
            with np.errstate(all="ignore"):
                n = n / np.linalg.norm(n, axis=-1, keepdims=True)
            better = (t > 0) & (t < best)
            best[better], nrm[better], rid[better], iid[better] = t[better], n[better], r, i
    return best, nrm, rid, iid, o, d


def _check_against_float64(a, depth, nrm, rid, iid, min_share):
    """The criteria of test_aov_x86_matches_analytic with the oracle in the probe's place: rtol = atol = 1e-5, id edges excluded."""
    rend, inst = a["renderer"], a["instance"]
    edge = D.id_edges(rid, iid)
    bad_ids = (rend != rid) | (inst != iid)
    assert np.count_nonzero(bad_ids & ~edge) == 0
    assert np.count_nonzero(bad_ids) <= max(1, int(0.001 * rend.size)) or np.all(bad_ids <= edge)
    ok = ~bad_ids & ~edge & (rid >= 0)
    assert ok.sum() > min_share * rend.size
    assert np.allclose(a["depth"][ok], depth[ok], rtol=1e-5, atol=0)
    assert np.allclose(a["normal"][ok], nrm[ok], rtol=1e-5, atol=1e-5)
    miss = rend < 0
    assert np.all(np.isinf(a["depth"][miss])) and np.all(a["normal"][miss] == 0) and np.all(a["albedo"][miss] == 0) and np.all(inst[miss] == -1)
    assert np.all(a["point"][miss] == 0)
    return ok


@pytest.mark.parametrize("aprt", [None, 0.3])
def test_oracle_aov_matches_analytic(oracle_mod, aprt):
    """test_aov_x86_matches_analytic's scene and criteria, the oracle in the x86 probe's place.  aprt 0.3: the ray leaves from
    the lens centre whatever the aperture."""
    from micro_raytracer_amd import _abi, load_render
    render = load_render(D._analytic_scene(aprt))
    a = oracle_aov(oracle_mod, _abi.build_desc(render))
    depth, nrm, rid, iid = D.np_first_hits(render)
    ok = _check_against_float64(a, depth, nrm, rid, iid, 0.5)
    assert np.allclose(a["albedo"][a["renderer"] == 2], [1.0, 0.0, 0.0])
    assert {0, 1, 2, 3} <= set(np.unique(a["renderer"]).tolist()) and set(np.unique(a["instance"][a["renderer"] == 2])) == {0, 1}
    assert ok.any()


def test_oracle_aov_matches_float64_under_rotations(oracle_mod):
    """A rotated box, a sphere under rotated instances, a rotated camera, ssaa 1.5: ids, depth and normal at the float64 bar
    (rtol = atol = 1e-5, id edges excluded), and the world point against o + d t0 of the float64 ray."""
    from micro_raytracer_amd import _abi, load_render
    render = load_render(_rotated_scene())
    a = oracle_aov(oracle_mod, _abi.build_desc(render))
    assert a["depth"].shape == (46, 70)
    depth, nrm, rid, iid, o, d = np_first_hits_rotated(render)
    ok = _check_against_float64(a, depth, nrm, rid, iid, 0.5)
    assert np.allclose(a["point"][ok], (o + d * depth[..., None])[ok], rtol=1e-5, atol=1e-5)
    # every object and every instance is seen, the rotated ones on more than a handful of pixels, and a rotated sphere's normal
    # is not the unrotated one (p - pos) / r: the second pass through the matrix shows
    for r, i in ((0, 0), (1, 0), (2, 0), (2, 1), (2, 2)):
        assert np.count_nonzero(ok & (rid == r) & (iid == i)) > 40, (r, i)
    m = ok & (rid == 2) & (iid == 0)
    naive = (a["point"][m] - np.array([-0.5, 0.2, 0.0])) / 0.22
    assert np.abs(naive - nrm[m]).max() > 0.1


# ---- b. the oracle against the x86 AOV pass -------------------------------------------------------------------------------------------
def check_scene(label, oracle_mod, probes, desc):
    render, holder = make_holder(desc)
    ref = oracle_aov(oracle_mod, holder)
    got = x86_planes(probes, holder)
    fig = compare_aov(label, got, ref)
    return render, holder, ref, got, fig


@pytest.mark.parametrize("name", NAMED)
def test_oracle_aov_equals_x86_on_named_scenes(oracle_mod, probes, name):
    """Measured ("AOVs against the oracle"): 0 ulp on every plane, 0 id mismatches."""
    render, holder, ref, got, _ = check_scene(name, oracle_mod, probes, named_scenes()[name]())
    assert (ref["renderer"] >= 0).any()
    if holder.ext is not None and holder.ext.env:
        # §15: the albedo of a miss is E(d); these skies are nowhere black
        miss = ref["renderer"] < 0
        assert miss.any() and (ref["albedo"][miss] > 0).all()


@pytest.mark.parametrize("family,seed", FUZZ)
def test_oracle_aov_equals_x86_on_fuzz_scenes(oracle_mod, probes, family, seed):
    check_scene(f"{family} {seed}", oracle_mod, probes, fuzz_desc(family, seed))


def multi_crowd():
    """Four instanced renderers (12 spheres, 9 rotated boxes, 7 triangles, 5 rotated icospheres) after a floor and before a
    single sphere, on a lattice that keeps them apart: the flat instance index of the packed scene differs from the index within
    the renderer's inst list for every renderer but the first, and the instance BVH is on."""
    from micro_raytracer_amd import scenes
    grid = lambda n, x0, y, z, dx, q: [[[x0 + dx * i, y + 0.07 * (i % 3), z + 0.05 * (i % 2)], q(i)] for i in range(n)]
    ident = lambda i: [0, 0, -1, 0]
    rot = lambda i: [0.1 * (i % 5) - 0.2, 0.3 + 0.1 * i, -1, 0.2 - 0.1 * (i % 4)]
    return {
        "rt": {"sample": 1, "bounce": 2},
        "frame": {"res": [120, 68], "ssaa": 1, "cam": {"pos": [0, -2.4, 0.5], "dir": [0, 0.12, 1, 0], "fov": 62}},
        "scene": {"renderer": [
            {"type": "plane", "n": [0, 0, 1], "pos": [0, 0, -0.5], "mat": {"albedo": "#808080"}},
            {"type": "sphere", "r": 0.09, "inst": grid(12, -1.4, 0.2, 0.75, 0.25, ident), "mat": {"albedo": "#ff4020"}},
            {"type": "box", "sizes": [0.2, 0.16, 0.14], "inst": grid(9, -1.3, 0.1, 0.35, 0.32, rot), "mat": {"albedo": "#20c040"}},
            {"type": "triangle", "vtx": [[-0.1, 0, -0.1], [0.1, 0, -0.1], [0, 0.03, 0.12]], "inst": grid(7, -1.2, 0.0, 0.0, 0.4, rot), "mat": {"albedo": "#3060ff"}},
            {"type": "mesh", "mesh": [[[float(c) for c in v] for v in t] for t in scenes.icosphere(1, 0.12, (1.0, 1.3, 0.8))],
             "inst": grid(5, -1.1, -0.1, -0.3, 0.55, rot), "mat": {"albedo": "#e0d040"}},
            {"type": "sphere", "r": 0.15, "pos": [0.0, 1.2, 1.2], "mat": {"albedo": "#ffffff"}},
        ]},
    }


def check_multi_crowd_ids(a):
    """Every instance of every instanced renderer is some pixel's first hit, under its index within the renderer's list."""
    for r, n in ((1, 12), (2, 9), (3, 7), (4, 5)):
        assert set(np.unique(a["instance"][a["renderer"] == r]).tolist()) == set(range(n)), r
    assert set(np.unique(a["instance"][(a["renderer"] == 0) | (a["renderer"] == 5)]).tolist()) == {0}


def test_oracle_aov_equals_x86_on_several_instanced_renderers(oracle_mod, probes):
    render, holder, ref, got, _ = check_scene("multi_crowd", oracle_mod, probes, multi_crowd())
    check_multi_crowd_ids(ref)
    info, _, _ = E.x86_pack(probes[1], holder, with_ext=False)
    assert info["features"] & F_BVH                          # F_BVH: the instance BVH


def test_env_ref_helpers_size_their_frames_by_the_supersampled_frame(probes, oracle_mod):
    """env_ragged (37 x 23 at ssaa 1.5: the probe writes 55 x 34) through env_ref.x86_aov and x86_render."""
    import test_oracle_ext as X
    render, holder = make_holder(X.SCENES["env_ragged"][0]())
    g, alb, rend = E.x86_aov(probes[1], holder)
    assert g.shape == (34, 55, 8) and alb.shape == (34, 55, 3) and rend.shape == (34, 55)
    assert (rend[-1] >= -1).all() and (g[..., 7][rend >= 0] == 1).all()
    assert E.x86_render(probes[1], holder, 1, 1, threads=THREADS).shape == (34, 55, 3)
