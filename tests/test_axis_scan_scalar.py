"""The axis body of the closest-hit scan after its instruction diet (csrc/mrt_trace.h trace, F_IDENT).  The plane
arm has no window test in front of its division core: the packer serves only planes whose position along their axis is +-0 or at
least 2^-15, which makes a numerator 0 (a miss on either route) or at least 2^-40, and a query with a lane whose origin lies
within 2^-40 of a coordinate plane without being on it goes to the generic body before the loop (CT_AXIS_REDO).  The sphere arm
tests its root and both quotients against the window at once.  The next record is fetched without asking whether there is one
(the packer pads the AXIS table, INSTX lies behind INST).  No bit may change: every check here compares with the generic body
(MRT_AXIS_SCAN=0) as uint32.

CPU: the x86 build of the same header (tests/emu/axis_redo_probe.cpp, which also reports whether a query was handed over; wave_all
is the lane's own predicate there).  GPU: the same constructed wavefronts through mrt_selftest_trace (ray i is lane i % 64 of
wavefront i / 64), where ONE lane hands over the query of all 64, and small frames against MRT_AXIS_SCAN=0."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_holder
from emu.build import ptr as _p, shared
from test_axis_scan import _gpu, _tame, probe, x86_trace  # noqa: F401  (probe: the fixture)

f32 = np.float32
WIN_LO = f32(2.0 ** -40)
AXIS_WORDS = 2


def _bind(L):
    fp, u32p, vp, u32 = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32
    L.ar_error.restype = C.c_char_p
    L.ar_trace.argtypes = [vp, C.c_int, u32, fp, fp, u32p]
    L.ar_census.argtypes = [vp, C.c_uint64, u32, fp, C.POINTER(C.c_uint64), u32p]


@pytest.fixture(scope="module")
def redo_probe():
    return shared("axis_redo_probe", _bind)


def redo_trace(L, holder, axis, orig, dirs):
    """[n][7]: hit, flat instance, t0 bits, t1 bits, renderer, axis body chosen, query handed to the generic body."""
    orig, dirs = np.ascontiguousarray(orig, f32), np.ascontiguousarray(dirs, f32)
    out = np.zeros((orig.shape[0], 7), np.uint32)
    rc = L.ar_trace(C.cast(holder.ptr(), C.c_void_p), axis, orig.shape[0], _p(orig), _p(dirs), _p(out, C.c_uint32))
    assert rc == 0, L.ar_error()
    return out


# ---- scenes --------------------------------------------------------------------------------------------------------------------
# Instance j is THE plane: the floor z = 0 through the origin (pos_k = 0, s d = +-0), so that a ray origin of z = 1e-13 has a
# numerator below 2^-40 and z = +-0 one of exactly +-0.  The others come from a pool in this order, so that both kinds, every
# axis and both orientations appear before and after j.
FLOOR = {"type": "plane", "n": [0, 0, 1], "pos": [0, 0, 0], "mat": {"rough": 1}}
POOL = [
    {"type": "sphere", "r": 0.2, "pos": [-0.35, 0.1, 0.45], "mat": {"glass": 0.08, "opacity": 0}},
    {"type": "plane", "n": [1, 0, 0], "pos": [-1, 0, 0], "mat": {"albedo": "#ff0000", "rough": 1}},
    {"type": "sphere", "r": 0.25, "pos": [0.4, 0.3, 0.3], "mat": {"metal": 1}},
    {"type": "plane", "n": [0, -1, 0], "pos": [0, 1, 0], "mat": {"rough": 1}},
    {"type": "plane", "n": [-1, 0, 0], "pos": [1, 0, 0], "mat": {"albedo": "#00ff00", "rough": 1}},
    {"type": "sphere", "r": 0.15, "pos": [0.0, -0.3, 0.9], "mat": {"albedo": "#ffc177", "emit": 1.0}},
    {"type": "plane", "n": [0, 0, -1], "pos": [0, 0, 1.2], "mat": {"rough": 1}},
    {"type": "plane", "n": [0, 1, 0], "pos": [0, -2, 0], "mat": {"rough": 0.4, "metal": 0.5}},
    {"type": "sphere", "r": 0.2, "pos": [-0.5, -0.6, 0.2], "mat": {"albedo": "#ff0000"}},
]
CASES = [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (10, 0), (10, 4), (10, 9)]      # (instances, index of THE plane)


def scene(n, j, res=(16, 8), sample=32, bounce=8):
    rends = [dict(r) for r in POOL[:n - 1]]
    rends.insert(j, dict(FLOOR))
    assert len(rends) == n
    return {
        "rt": {"sample": sample, "bounce": bounce},
        "frame": {"res": [int(res[0]), int(res[1])], "ssaa": 1, "cam": {"exp": 0.75, "fov": 70, "gamma": 0.5, "pos": [0.05, -1.2, 0.45]}},
        "scene": {"renderer": rends},
    }


# ---- rays and wavefronts ---------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32)


def _pool_rays(seed, n=3000):
    """Tame rays from inside the room (z in [0.05, 1.15]: every plane numerator far inside the window), any direction."""
    rng = np.random.default_rng(seed)
    o = (rng.uniform(-1, 1, (n, 3)) * np.array([0.9, 0.9, 0.55]) + np.array([0, 0, 0.6])).astype(f32)
    d = _unit(rng.normal(size=(n, 3)))
    keep = _tame(o, d)
    return o[keep], d[keep]


# (origin z, direction z sign): exactly on the plane with both zeros (a miss on either route: these four hand nothing over), and
# the lanes that do: just under 2^-40 on both sides, the largest float below 2^-40, denormals
FLAGGED = [(0.0, 1), (-0.0, 1), (0.0, -1), (-0.0, -1), (1e-13, 1), (-1e-13, 1), (1e-13, -1), (-1e-13, -1),
           (float(np.nextafter(WIN_LO, f32(0))), 1), (1e-40, 1), (-1e-45, -1)]
NOT_FLAGGED = [(float(WIN_LO), 1), (-float(WIN_LO), -1), (float(np.nextafter(WIN_LO, f32(1))), 1)]      # the window's end itself


def _flag_rays(specs):
    o = np.array([(0.13 + 0.01 * i, -0.21, z) for i, (z, _) in enumerate(specs)], f32)
    d = _unit([(0.31, 0.57, s * 0.76) for _, s in specs])
    return o, d


def wavefronts(L, holder, j, n_inst):
    """Wavefronts of 64 tame rays for plane j: lane 0 exactly on the plane, lane 1 with a numerator just under 2^-40 (a different
    pair per wavefront), the other 62 lanes chosen by the winner the generic body finds for them: all before j, all after j, j
    itself or a miss, any mix; one wavefront whose lanes 0 and 1 stand at the window's end (no redo) and one without them."""
    o, d = _pool_rays(41 + 7 * n_inst + j)
    gen = redo_trace(L, holder, 0, o, d)
    hit, win = gen[:, 0] != 0, gen[:, 1].astype(int)
    classes = {"before": np.flatnonzero(hit & (win < j)), "after": np.flatnonzero(hit & (win > j)),
               "self_or_miss": np.flatnonzero(~hit | (win == j)), "any": np.arange(o.shape[0])}
    if j > 0 and n_inst > 1:
        assert classes["before"].size >= 8, (n_inst, j)
    if j < n_inst - 1:
        assert classes["after"].size >= 8, (n_inst, j)
    fo, fd = _flag_rays(FLAGGED)
    no, nd = _flag_rays(NOT_FLAGGED)
    rng = np.random.default_rng(5 + j)
    wo, wd, redo = [], [], []
    pair = 0
    for name, idx in classes.items():
        if idx.size == 0:
            continue
        for _ in range(2):
            lanes = rng.choice(idx, 62)
            a, b = pair % 4, 4 + pair % (len(FLAGGED) - 4)                # lane 0: num == +-0, lane 1: 0 < |num| < 2^-40
            pair += 1
            wo.append(np.concatenate([fo[[a, b]], o[lanes]])); wd.append(np.concatenate([fd[[a, b]], d[lanes]])); redo.append(True)
    lanes = rng.choice(classes["any"], 62)
    wo.append(np.concatenate([no[:2], o[lanes]])); wd.append(np.concatenate([nd[:2], d[lanes]])); redo.append(False)
    lanes = rng.choice(classes["any"], 64)
    wo.append(o[lanes]); wd.append(d[lanes]); redo.append(False)
    return np.concatenate(wo), np.concatenate(wd), np.array(redo)


def _same(gen, fast, o, d):
    bad = np.flatnonzero(~(gen[:, :5] == fast[:, :5]).all(axis=1))
    assert bad.size == 0, (bad[:8] // 64, bad[:8] % 64, o[bad[:4]], d[bad[:4]], gen[bad[:4]], fast[bad[:4]])


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_inst,j", CASES)
def test_flagged_lanes_are_answered_by_the_generic_body_with_the_same_bits(redo_probe, n_inst, j):
    _, holder = make_holder(scene(n_inst, j))
    o, d, _ = wavefronts(redo_probe, holder, j, n_inst)
    assert o.shape[0] % 64 == 0 and _tame(o, d).all()
    gen, fast = redo_trace(redo_probe, holder, 0, o, d), redo_trace(redo_probe, holder, 1, o, d)
    assert not gen[:, 5].any() and not gen[:, 6].any()
    assert (fast[:, 5] == 1).all()                                        # every ray enters the axis body
    _same(gen, fast, o, d)
    # exactly the rays whose numerator at plane j lies below the window without being zero are redone (per ray on x86)
    num = np.abs(o[:, 2])                                                 # |-(pos_k + (o_k - pos_k) + s d)| with pos_k = 0, s d = +-0
    assert np.array_equal(fast[:, 6] != 0, (num < WIN_LO) & (num > 0))
    assert (fast[:, 6] != 0).sum() >= 2 and (num == 0).sum() >= 2 and (fast[:, 6] == 0).sum() > 64
    if n_inst >= 3:
        assert (gen[:, 0] != 0).mean() > 0.3 and len(set(gen[gen[:, 0] != 0, 1].tolist())) >= 2


def test_every_flagged_origin_and_the_window_end(redo_probe):
    """All the flagged origins and the ones at the window's end, through the 10-instance scene with the plane in every position."""
    for j in range(10):
        _, holder = make_holder(scene(10, j))
        o, d = (np.concatenate(p) for p in zip(_flag_rays(FLAGGED), _flag_rays(NOT_FLAGGED)))
        gen, fast = redo_trace(redo_probe, holder, 0, o, d), redo_trace(redo_probe, holder, 1, o, d)
        _same(gen, fast, o, d)
        assert (fast[:, 5] == 1).all()
        assert not fast[:4, 6].any() and fast[4:len(FLAGGED), 6].all() and not fast[len(FLAGGED):, 6].any()      # (+-0: no redo)


@pytest.mark.parametrize("n_inst", [1, 2, 3, 10])
def test_both_parities_of_the_two_buffer_loop(redo_probe, probe, n_inst):
    """n = 1, 2, 3, 10: the loop leaves through its first and its second exit; random rays and a render, both bodies."""
    j = n_inst // 2
    _, holder = make_holder(scene(n_inst, j, res=(16, 8), sample=8))
    o, d = _pool_rays(3 + n_inst)
    gen, fast = redo_trace(redo_probe, holder, 0, o, d), redo_trace(redo_probe, holder, 1, o, d)
    _same(gen, fast, o, d)
    assert (fast[:, 5] == 1).all() and not fast[:, 6].any()
    assert np.array_equal(x86_trace(probe, holder, 1, o, d)[:, :5], fast[:, :5])          # (the older probe sees the same)
    if n_inst > 1:
        assert len(set(gen[gen[:, 0] != 0, 1].tolist())) >= min(n_inst, 6) - 1


def _census(L, holder, seed, spp):
    nw, nh = holder.desc.frame.res_w, holder.desc.frame.res_h
    acc = np.zeros((nh, nw, 3), f32)
    counts, info = np.zeros(3, np.uint64), np.zeros(3, np.uint32)
    rc = L.ar_census(C.cast(holder.ptr(), C.c_void_p), seed, spp, _p(acc), _p(counts, C.c_uint64), _p(info, C.c_uint32))
    assert rc == 0, L.ar_error()
    return acc, [int(c) for c in counts], dict(zip(("blob_words", "off_axis", "n_inst"), (int(v) for v in info)))


def test_one_record_past_the_end_is_inside_the_blob(redo_probe, probe):
    """The unconditional prefetch reads record n of INST (its first four words) and of AXIS: both inside the blob, the AXIS one
    inside the table's own padding -- also where the AXIS table is the last thing the kernel stages before the tables every
    scene has (transforms, materials, the k/255 table), which is every scene the axis scan serves."""
    from test_axis_scan import x86_pack
    for n_inst, j in CASES:
        _, holder = make_holder(scene(n_inst, j))
        info, blob = x86_pack(probe, holder)
        assert info["axis_scan"] == 1 and info["n_inst"] == n_inst
        end_axis = info["off_axis"] + AXIS_WORDS * (n_inst + 1)
        assert end_axis <= info["blob_words"]
        assert not blob[info["off_axis"] + AXIS_WORDS * n_inst:end_axis].any()          # the padding record is zeros
        assert info["off_inst"] + 8 * n_inst + 4 <= info["off_axis"]                    # INST's next half record: INSTX is there


def test_redo_is_rare_on_a_cornell_frame(redo_probe):
    """The census behind DESIGN.md §7: on the Cornell box every closest-hit query enters the axis body and none is redone.  A ray
    that leaves a wall at a grazing angle starts exactly on it (3 in 10^4 queries: why a zero numerator raises no flag); one
    within 2^-40 of a plane but not on it needs a plane through 0, which the Cornell box does not have."""
    from micro_raytracer_amd import scenes
    _, holder = make_holder(scenes.cornell_box(res=(32, 32), sample=8, bounce=8))
    _, (queries, entered, redone), _ = _census(redo_probe, holder, 11, 8)
    print(f"cornell 32x32 8 spp: {queries} closest-hit queries, {entered} through the axis body, {redone} redone")
    assert queries > 32 * 32 * 8 and entered > 0.99 * queries
    assert redone == 0


def test_census_render_equals_the_generic_render(redo_probe, probe):
    from test_axis_scan import x86_render
    _, holder = make_holder(scene(10, 4, res=(16, 8), sample=8))
    acc, (queries, entered, _), _ = _census(redo_probe, holder, 5, 8)
    gen, _ = x86_render(probe, holder, 0, 5, 8)
    assert entered > 0.9 * queries and np.array_equal(acc.view(np.uint32), gen.view(np.uint32))


def test_planes_next_to_a_coordinate_plane_are_not_served(probe):
    """A plane whose position along its axis is neither +-0 nor at least 2^-15 would allow numerators in (0, 2^-40): the packer
    gives such a scene no AXIS table (the generic body answers everything, as for any scene the classifier turns down)."""
    from test_axis_scan import x86_pack
    lo = 2.0 ** -15
    for z, served in ((0.0, 1), (-0.0, 1), (lo, 1), (-lo, 1), (float(np.nextafter(f32(lo), f32(0))), 0), (-1e-7, 0), (1e-30, 0), (1e-45, 0), (0.3, 1)):
        d = scene(3, 1)
        d["scene"]["renderer"][1]["pos"] = [0.25, -0.5, z]                  # the others' components are free: only pos_k counts
        _, holder = make_holder(d)
        info, _ = x86_pack(probe, holder)
        assert info["axis_scan"] == served and info["params_axis_scan"] == served, z


def _root_rays():
    """Rays at the spheres of the 10-instance scene whose disc or root numerators leave [2^-40, 2^40] or sit at its ends: tangent
    within a few ulps (disc 0 or tiny), from the centre, from the surface inwards (c == 0: a root numerator of exactly 0), huge
    and tiny directions (disc overflows / underflows), next to ordinary ones."""
    up, dn = lambda v: np.nextafter(f32(v), f32(np.inf)), lambda v: np.nextafter(f32(v), f32(-np.inf))
    o, d = [], []
    for pos, r in (((0.0, -0.3, 0.9), 0.15), ((-0.35, 0.1, 0.45), 0.2), ((0.4, 0.3, 0.3), 0.25)):
        zt = f32(f32(pos[2]) + f32(r))
        for steps in range(-3, 4):
            z = zt
            for _ in range(abs(steps)):
                z = up(z) if steps > 0 else dn(z)
            for tilt in ((1e-9, 1e-9), (2.0 ** -40, -2.0 ** -40), (1e-5, -1e-7)):
                o.append((pos[0] - 0.6, pos[1], float(z))); d.append(tuple(_unit((1.0, tilt[0], tilt[1]))))
        for dd in ((0.31, 0.57, -0.76), (-0.6, 0.3, 0.74)):
            o.append(pos); d.append(dd)                                                   # from the centre
            for k in range(3):
                for sg in (1, -1):
                    q = [f32(pos[0]), f32(pos[1]), f32(pos[2])]
                    q[k] = f32(q[k] + f32(sg * r))
                    e = [0.05, -0.03, 0.02]
                    e[k] = -sg                                                           # from the surface through the centre
                    o.append(tuple(float(v) for v in q)); d.append(tuple(_unit(e)))
            u = _unit((1, 0.5, 0.25)).astype(np.float64)                                  # every scaled component stays inside the window
            for s in (2.0 ** 30, 2.0 ** 39, 2.0 ** -30, 2.0 ** -37):
                o.append(tuple(float(v) for v in np.array(pos) - 0.5 * u + np.array([0, 0.01, 0]))); d.append(tuple(float(v) for v in u * s))
    return np.array(o, f32), np.array(d, f32)


def _root_wavefronts():
    ro, rd = _root_rays()
    po, pd = _pool_rays(77)
    rng = np.random.default_rng(9)
    wo, wd = [], []
    for w in range(0, ro.shape[0], 4):                                    # four such lanes among sixty ordinary ones
        lanes = rng.choice(po.shape[0], 64 - len(ro[w:w + 4]))
        wo.append(np.concatenate([ro[w:w + 4], po[lanes]])); wd.append(np.concatenate([rd[w:w + 4], pd[lanes]]))
    return np.concatenate(wo), np.concatenate(wd)


def test_sphere_roots_at_and_outside_the_window(redo_probe):
    _, holder = make_holder(scene(10, 4))
    o, d = _root_wavefronts()
    assert o.shape[0] % 64 == 0 and _tame(o, d).all()
    gen, fast = redo_trace(redo_probe, holder, 0, o, d), redo_trace(redo_probe, holder, 1, o, d)
    _same(gen, fast, o, d)
    assert (fast[:, 5] == 1).all() and not fast[:, 6].any()
    won = set(gen[gen[:, 0] != 0, 1].tolist())
    assert {0, 2, 6} <= won                                               # the three spheres aimed at (flat indices with the plane at 4)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def _gpu_trace(monkeypatch, render, axis, o, d):
    from micro_raytracer_amd import Sampler, _lib
    if axis:
        monkeypatch.delenv("MRT_AXIS_SCAN", raising=False)
    else:
        monkeypatch.setenv("MRT_AXIS_SCAN", "0")
    s = Sampler(seed=3, device=0)
    s.create(render)
    monkeypatch.delenv("MRT_AXIS_SCAN", raising=False)
    feat = s.stats()["kernel_features"]
    w = _lib.selftest_trace(s, o, d)["words"]
    s.close()
    return w, feat


@pytest.mark.gpu
@pytest.mark.parametrize("n_inst,j", CASES)
def test_gpu_wavefronts_with_a_flagged_lane_change_no_bit(monkeypatch, redo_probe, n_inst, j):
    """One lane on the plane and one just under 2^-40 above or below it send all 64 lanes of their wavefront through the generic
    body, whichever side of j their winner is on; the wavefronts at the window's end and without such lanes stay."""
    render, holder = make_holder(scene(n_inst, j))
    o, d, _ = wavefronts(redo_probe, holder, j, n_inst)
    assert o.shape[0] % 64 == 0 and _tame(o, d).all()                     # every wavefront takes the axis body
    fast, f_feat = _gpu_trace(monkeypatch, render, True, o, d)
    gen, g_feat = _gpu_trace(monkeypatch, render, False, o, d)
    assert f_feat == 256 and g_feat == 256
    bad = np.flatnonzero((fast != gen).any(axis=1))
    assert bad.size == 0, (bad[:8] // 64, bad[:8] % 64, o[bad[:4]], d[bad[:4]], gen[bad[:4]], fast[bad[:4]])
    # the closest-hit words are the x86 generic body's too (every renderer has one instance: the hook's instance index is 0)
    want = redo_trace(redo_probe, holder, 0, o, d)
    assert np.array_equal(fast[:, 0], want[:, 0])
    h = want[:, 0] != 0
    assert np.array_equal(fast[h][:, [2, 4, 5]], want[h][:, 1:4]) and not fast[h][:, 3].any()


@pytest.mark.gpu
@pytest.mark.parametrize("n_inst", [1, 3, 10])
def test_gpu_small_frames_change_no_bit(monkeypatch, n_inst):
    render, _ = make_holder(scene(n_inst, n_inst // 2, res=(16, 8), sample=32))
    fast, _, f_feat = _gpu(render, 32, monkeypatch, True)
    gen, _, g_feat = _gpu(render, 32, monkeypatch, False)
    assert f_feat == 256 and g_feat == 256
    assert np.isfinite(fast).all() and (n_inst < 10 or fast.any())          # (the emitter is the 10-instance scene's)
    assert np.array_equal(fast.view(np.uint32), gen.view(np.uint32))


@pytest.mark.gpu
def test_gpu_sphere_roots_at_and_outside_the_window(monkeypatch, redo_probe):
    """Wavefronts in which four lanes' disc or root numerators leave the window (the full expansions answer for all 64) or sit
    at its ends, among sixty ordinary lanes."""
    render, holder = make_holder(scene(10, 4))
    o, d = _root_wavefronts()
    assert o.shape[0] % 64 == 0 and _tame(o, d).all()
    fast, f_feat = _gpu_trace(monkeypatch, render, True, o, d)
    gen, g_feat = _gpu_trace(monkeypatch, render, False, o, d)
    assert f_feat == 256 and g_feat == 256
    bad = np.flatnonzero((fast != gen).any(axis=1))
    assert bad.size == 0, (bad[:8] // 64, bad[:8] % 64, o[bad[:4]], d[bad[:4]], gen[bad[:4]], fast[bad[:4]])
    want = redo_trace(redo_probe, holder, 0, o, d)
    assert np.array_equal(fast[:, 0], want[:, 0])
    h = (want[:, 0] != 0) & ~np.isnan(want[:, 2].view(f32))              # (a NaN distance's payload is not part of the contract)
    assert np.array_equal(fast[h][:, [2, 4, 5]], want[h][:, 1:4])
