"""The axis body of the closest-hit scan (csrc/mrt_trace.h trace, F_IDENT): scenes of untransformed spheres and
axis-aligned planes test a plane with the one component its normal selects and share three refined reciprocals per ray.  It must
change no bit: every check here compares it with the generic body (MRT_AXIS_SCAN=0) as uint32.

CPU: the x86 build of the same header (tests/emu/axis_probe.cpp; wave_all is the lane's own predicate there, so every ray
chooses its body itself) -- the packer's classification and table, single queries on adversarial rays, a small render.
GPU: a Cornell-shaped frame through both launch shapes against MRT_AXIS_SCAN=0 and the oracle, and a camera that sits on a
plane and looks along an axis (direction components of exactly 0: those wavefronts fall back to the generic body)."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_holder
from emu.build import ptr as _p, shared

f32 = np.float32
TOL = 1e-4          # tests/test_gpu_parity.py: mean radiance against the oracle, per channel, L-inf
WIN_LO, WIN_HI, AXIS_MAX = f32(2.0 ** -40), f32(2.0 ** 40), f32(2.0 ** 38)


# ---- the probe ---------------------------------------------------------------------------------------------------------------
def _bind(L):
    fp, u32p, vp, u32 = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32
    L.ax_error.restype = C.c_char_p
    L.ax_pack.argtypes = [vp, u32p, u32p, C.c_uint64]
    L.ax_trace.argtypes = [vp, C.c_int, u32, fp, fp, u32p]
    L.ax_render.argtypes = [vp, C.c_int, C.c_uint64, u32, u32, fp, C.POINTER(C.c_uint64)]


@pytest.fixture(scope="module")
def probe():
    return shared("axis_probe", _bind)


PACK_KEYS = ("features", "all_ident", "axis_scan", "params_axis_scan", "off_axis", "n_inst", "off_inst", "blob_words")


def x86_pack(L, holder):
    d = C.cast(holder.ptr(), C.c_void_p)
    info = np.zeros(8, np.uint32)
    rc = L.ax_pack(d, _p(info, C.c_uint32), None, 0)
    assert rc == 0, L.ax_error()
    info = dict(zip(PACK_KEYS, (int(v) for v in info)))
    blob = np.zeros(info["blob_words"], np.uint32)
    assert L.ax_pack(d, _p(np.zeros(8, np.uint32), C.c_uint32), _p(blob, C.c_uint32), blob.size) == 0
    return info, blob


def x86_trace(L, holder, axis, orig, dirs):
    orig, dirs = np.ascontiguousarray(orig, f32), np.ascontiguousarray(dirs, f32)
    out = np.zeros((orig.shape[0], 6), np.uint32)
    rc = L.ax_trace(C.cast(holder.ptr(), C.c_void_p), axis, orig.shape[0], _p(orig), _p(dirs), _p(out, C.c_uint32))
    assert rc == 0, L.ax_error()
    return out


def x86_render(L, holder, axis, seed, n_samples):
    nw, nh = holder.desc.frame.res_w, holder.desc.frame.res_h
    acc = np.zeros((nh, nw, 3), f32)
    seg = C.c_uint64()
    rc = L.ax_render(C.cast(holder.ptr(), C.c_void_p), axis, seed, n_samples, 4, _p(acc), C.byref(seg))
    assert rc == 0, L.ax_error()
    return acc, seg.value


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def six_plane_scene(res=(16, 16), sample=8, bounce=8):
    """A closed room of axis planes in all six orientations -- zero normal components written as -0.0, the floor through the
    origin (pos_k == 0, d == +-0) -- with spheres in front of, behind and across planes; one of glass (the exit distance t1)."""
    return {
        "rt": {"sample": sample, "bounce": bounce},
        "frame": {"res": [int(res[0]), int(res[1])], "ssaa": 1, "cam": {"exp": 0.75, "fov": 70, "gamma": 0.5, "pos": [0.05, -1.2, 0.45]}},
        "scene": {"renderer": [
            {"type": "plane", "n": [-0.0, -1, -0.0], "pos": [0, 1, 0], "mat": {"rough": 1}},
            {"type": "sphere", "r": 0.2, "pos": [-0.15, -0.4, 0.2], "mat": {"glass": 0.08, "opacity": 0}},
            {"type": "plane", "n": [1, -0.0, 0], "pos": [-1, 0, 0], "mat": {"albedo": "#ff0000", "rough": 1}},
            {"type": "plane", "n": [-1, 0, -0.0], "pos": [1, 0, 0], "mat": {"albedo": "#00ff00", "rough": 1}},
            {"type": "sphere", "r": 0.25, "pos": [0.95, 0.2, 0.4], "mat": {"metal": 1}},                 # across the x = 1 wall
            {"type": "plane", "n": [-0.0, -0.0, -1], "pos": [0, 0, 1], "mat": {"rough": 1}},
            {"type": "plane", "n": [0, 0, 1], "pos": [0, 0, 0], "mat": {"rough": 1}},                    # through the origin: d = -0
            {"type": "plane", "n": [-0.0, 2, 0], "pos": [0, -2, 0], "mat": {"rough": 0.4, "metal": 0.5}},   # not unit length: n^ is
            {"type": "sphere", "r": 0.2, "pos": [0.3, 1.5, 0.3], "mat": {"albedo": "#ff0000"}},          # behind the y = 1 wall
            {"type": "sphere", "r": 0.2, "pos": [0.4, 0.5, 0.0], "mat": {"albedo": "#ffc177", "emit": 1.0}},   # cut by the floor
            {"type": "plane", "n": [0, 0, -1], "pos": [0, 0, 0], "mat": {"rough": 1}},                   # the floor's other side: d = +0
        ]},
    }


def cornell_shaped(res=(64, 64), sample=32, bounce=8, cam_pos=(0, -1.2, 0.1)):
    from micro_raytracer_amd import scenes
    d = scenes.cornell_box(res=res, sample=sample, bounce=bounce)
    d["frame"]["cam"]["pos"] = [float(c) for c in cam_pos]
    return d


# ---- CPU: the classifier -----------------------------------------------------------------------------------------------------
def test_classifier_and_table(probe):
    from micro_raytracer_amd import scenes
    for desc, negzero in ((scenes.cornell_box(res=(16, 16), sample=1), False), (six_plane_scene(), True)):
        _, holder = make_holder(desc)
        info, blob = x86_pack(probe, holder)
        assert info["features"] == 0 and info["all_ident"] == 1          # mrt_create makes that kernel_features 256
        assert info["axis_scan"] == 1 and info["params_axis_scan"] == 1 and info["off_axis"] % 4 == 0 and info["off_axis"] > info["off_inst"]
        n = info["n_inst"]
        inst = blob[info["off_inst"]:info["off_inst"] + 8 * n].reshape(n, 8)
        tab = blob[info["off_axis"]:info["off_axis"] + 2 * n].reshape(n, 2)
        kinds = [r["type"] for r in desc["scene"]["renderer"]]
        seen_negzero = False
        for i in range(n):
            if kinds[i] == "sphere":
                assert tuple(tab[i]) == (0, 0) and inst[i, 4] & 7 == 0
                continue
            assert inst[i, 4] & 7 == 1
            nrm = inst[i, 5:8].view(f32)
            k = int(np.argmax(np.abs(nrm)))
            assert abs(nrm[k]) == 1 and tab[i, 0] == k + 1
            assert all((inst[i, 5 + j] & 0x7fffffff) == 0 for j in range(3) if j != k)
            seen_negzero |= any(inst[i, 5 + j] == 0x80000000 for j in range(3) if j != k)
            sd = inst[i, 3] ^ (inst[i, 5 + k] & 0x80000000)               # s * d: d, or d with its sign flipped
            assert tab[i, 1] == sd
            # d = (-n^).pos = -s pos_k, so s d = -pos_k (as a number: the zero's sign is the dot product's)
            assert tab[i, 1:2].view(f32)[0] == -inst[i, k:k + 1].view(f32)[0]
        assert seen_negzero == negzero                                    # the -0.0 components reach the packed normals


def _variant(edit):
    from micro_raytracer_amd import scenes
    d = scenes.cornell_box(res=(16, 16), sample=1)
    edit(d)
    return d


NOT_CLASSIFIED = {
    "tilted_plane": lambda d: d["scene"]["renderer"][0].update(n=[0, -0.8, 0.6]),
    "nearly_axis_plane": lambda d: d["scene"]["renderer"][1].update(n=[1, 1e-30, 0]),      # n^ keeps a non-zero y
    "transformed_instance": lambda d: d["scene"]["renderer"][6].update(dir=[0, 0.5, 0.5, 0]),
    "box": lambda d: d["scene"]["renderer"].append({"type": "box", "sizes": [0.2, 0.2, 0.2], "pos": [0, 0, 0.5]}),
    "light": lambda d: d["scene"].update(light=[{"type": "point", "pos": [0, 0, 0.9], "pwr": 0.5, "color": "#ffffff"}]),
    "far_sphere": lambda d: d["scene"]["renderer"][7].update(pos=[1e30, 0, 0]),
    "far_plane": lambda d: d["scene"]["renderer"][4].update(pos=[0, 0, -1e30]),
    "past_the_bound": lambda d: d["scene"]["renderer"][8].update(pos=[0, float(np.nextafter(AXIS_MAX, f32(np.inf))), 0]),
    "huge_radius": lambda d: d["scene"]["renderer"][5].update(r=1e20),
}


@pytest.mark.parametrize("name", list(NOT_CLASSIFIED))
def test_scenes_that_must_not_be_classified(probe, name):
    _, holder = make_holder(_variant(NOT_CLASSIFIED[name]))
    info, _ = x86_pack(probe, holder)
    assert info["axis_scan"] == 0 and info["params_axis_scan"] == 0 and info["off_axis"] == 0


def test_the_bound_itself_is_classified(probe):
    _, holder = make_holder(_variant(lambda d: d["scene"]["renderer"][8].update(pos=[0, float(AXIS_MAX), 0])))
    info, _ = x86_pack(probe, holder)
    assert info["axis_scan"] == 1


# ---- CPU: single queries through both bodies -----------------------------------------------------------------------------------
def _adversarial_rays():
    up, dn = lambda v: np.nextafter(f32(v), f32(np.inf)), lambda v: np.nextafter(f32(v), f32(-np.inf))
    inf, nan = f32(np.inf), f32(np.nan)
    g = (0.31, 0.57, -0.76)                                              # a generic direction, every component inside the window
    o, d = [], []

    def add(oo, dd):
        o.append(oo); d.append(dd)

    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                dd = (sx * g[0], sy * g[1], sz * g[2])
                add((1.0, 0.2, 0.3), dd); add((-1.0, 0.2, 0.3), dd)       # o_k == pos_k exactly: x walls
                add((0.3, 1.0, 0.5), dd); add((0.3, -2.0, 0.5), dd)       # y walls
                add((0.3, 0.2, 1.0), dd)                                  # ceiling
                add((0.3, 0.2, 0.0), dd); add((0.3, 0.2, -0.0), dd)       # on the plane through the origin: ro_k = +-0, d = +-0
                add((0.0, 0.0, 0.0), dd); add((-0.0, -0.0, -0.0), dd); add((0.0, -0.0, 0.5), dd); add((-0.0, 0.3, -0.0), dd)
                for tiny in (1e-13, -1e-13, 9.0e-13, float(WIN_LO), float(dn(WIN_LO)), 1e-40, -1e-40, 1e-45):      # |num| around and below 2^-40
                    add((0.3, 0.2, tiny), dd); add((1.0 + tiny if abs(tiny) > 1e-8 else 1.0, 0.2, 0.3), dd)
                    add((tiny, tiny, tiny), dd)
                add((0.3, 1.0 - 2.0 ** -24, 0.5), dd); add((float(up(1.0)), 0.2, 0.3), dd)     # one ulp off a wall
                # direction components at the window's ends and just outside
                for w in (WIN_LO, dn(WIN_LO), up(WIN_LO), WIN_HI, up(WIN_HI), dn(WIN_HI)):
                    for k in range(3):
                        e = [dd[0], dd[1], dd[2]]
                        e[k] = float(w) * (1 if dd[k] > 0 else -1)
                        add((0.1, -0.3, 0.4), tuple(e))
                add((0.1, -0.3, 0.4), (sx * float(WIN_HI), sy * float(WIN_HI), sz * float(WIN_LO)))
                add((0.1, -0.3, 0.4), (sx * float(WIN_LO), sy * float(WIN_LO), sz * float(WIN_LO)))
                # origins at the bound, beyond it, far beyond it
                for w in (AXIS_MAX, up(AXIS_MAX), dn(AXIS_MAX), f32(1e30), f32(3e38)):
                    for k in range(3):
                        e = [0.1, -0.3, 0.4]
                        e[k] = float(w) * sx
                        add(tuple(e), dd)
                add((sx * float(AXIS_MAX),) * 3, dd)
    # rays that must take the generic body: zero, infinite, NaN components
    for bad in (0.0, -0.0, inf, -inf, nan, 1e-30, 1e30):
        for k in range(3):
            e = [g[0], g[1], g[2]]
            e[k] = float(bad)
            add((0.1, -0.3, 0.4), tuple(e))
            if not (bad == 0 or abs(bad) == 1e-30):
                q = [0.1, -0.3, 0.4]
                q[k] = float(bad)
                add(tuple(q), g)
    add((0.1, -0.3, 0.4), (0.0, 1.0, 0.0)); add((0.1, -0.3, 0.4), (0.0, 0.0, -1.0)); add((nan, nan, nan), (nan, nan, nan))
    add((inf, -inf, 0.0), (0.0, -0.0, inf))
    return np.array(o, f32), np.array(d, f32)


def _tame(o, d):
    ad, ao = np.abs(d), np.abs(o)
    with np.errstate(invalid="ignore"):
        return ((ad >= WIN_LO) & (ad <= WIN_HI)).all(axis=1) & (ao <= AXIS_MAX).all(axis=1)


def test_both_scan_bodies_answer_every_ray_alike(probe):
    _, holder = make_holder(six_plane_scene())
    o, d = _adversarial_rays()
    rng = np.random.default_rng(11)
    n = 4000
    ro = rng.uniform(-1, 1, (n, 3)).astype(f32) * f32(1.2) + np.array([0, 0, 0.5], f32)
    rd = rng.normal(size=(n, 3)).astype(f32)
    rd /= np.linalg.norm(rd, axis=1, keepdims=True).astype(f32)
    ro[::7, 2] = 0.0                                                      # on the plane through the origin
    ro[::11, 0] = 1.0                                                     # on a wall
    rd[::13] *= f32(1e-9); rd[5::13] *= f32(1e9)                          # directions that are not unit length
    o, d = np.concatenate([o, ro]), np.concatenate([d, rd])
    gen = x86_trace(probe, holder, 0, o, d)
    fast = x86_trace(probe, holder, 1, o, d)
    tame = _tame(o, d)
    assert not gen[:, 5].any()                                            # MRT_AXIS_SCAN=0: the generic body answers everything
    assert np.array_equal(fast[:, 5] != 0, tame)                          # the axis body answers exactly the rays the guard admits
    assert tame.sum() > 3000 and (~tame).sum() > 100
    nan0 = np.isnan(gen[:, 2].view(f32)) & np.isnan(fast[:, 2].view(f32))
    assert not nan0[tame].any()
    same = (gen[:, :5] == fast[:, :5]).all(axis=1)
    bad = np.flatnonzero(~same)
    assert bad.size == 0, (o[bad[:4]], d[bad[:4]], gen[bad[:4]], fast[bad[:4]])
    hits = gen[tame, 0] != 0
    assert hits.mean() > 0.9                                              # a closed room: (nearly) every tame ray hits
    kinds_hit = set(gen[tame & (gen[:, 0] != 0), 1].tolist())
    assert len(kinds_hit) >= 9                                            # planes of every orientation and spheres win


def test_render_is_bit_identical_with_and_without_the_axis_body(probe, monkeypatch):
    for desc in (six_plane_scene(res=(16, 16), sample=8), cornell_shaped(res=(16, 16), sample=8)):
        _, holder = make_holder(desc)
        monkeypatch.delenv("MRT_AXIS_SCAN", raising=False)
        a, sa = x86_render(probe, holder, -1, 5, 8)                       # -1: the probe follows the environment, as mrt_create does
        monkeypatch.setenv("MRT_AXIS_SCAN", "0")
        b, sb = x86_render(probe, holder, -1, 5, 8)
        monkeypatch.delenv("MRT_AXIS_SCAN")
        assert sa == sb and sa >= 16 * 16 * 8
        assert np.isfinite(a).all() and a.any()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_x86_axis_render_equals_the_emulator_and_the_oracle_bar(probe, emu_mod, oracle_mod):
    """The probe's render (axis body) against tests/emu's (which never sets the flag) and the oracle."""
    _, holder = make_holder(six_plane_scene(res=(16, 16), sample=8))
    a, sa = x86_render(probe, holder, 1, 5, 8)
    e, se = emu_mod.render(holder, 5, 8, threads=4)
    assert sa == se and np.array_equal(a.view(np.uint32), e.view(np.uint32))
    o = oracle_mod.Oracle(holder, seed=5)
    o.execute(8)
    ref, cnt = o.accum()
    assert cnt == 8 and np.max(np.abs(a - ref)) / 8 <= TOL


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _gpu(render, spp, monkeypatch, axis, extra_one=False):
    from micro_raytracer_amd import Sampler
    if axis:
        monkeypatch.delenv("MRT_AXIS_SCAN", raising=False)
    else:
        monkeypatch.setenv("MRT_AXIS_SCAN", "0")
    s = Sampler(seed=5)
    s.execute(render, n_samples=spp)
    acc, cnt = s.accum()
    assert cnt == spp
    feats = s.stats()["kernel_features"]
    one = None
    if extra_one:
        s.execute(render, n_samples=1)                                    # less than a sample chunk: the plain-grid launch shape
        one, c1 = s.accum()
        assert c1 == spp + 1
    s.close()
    monkeypatch.delenv("MRT_AXIS_SCAN", raising=False)
    return acc, one, feats


@pytest.mark.gpu
def test_gpu_cornell_axis_scan_changes_no_bit(monkeypatch, oracle_mod):
    render, holder = make_holder(cornell_shaped(res=(64, 64), sample=32, bounce=8))
    fast, fast1, f_feat = _gpu(render, 32, monkeypatch, True, extra_one=True)
    gen, gen1, g_feat = _gpu(render, 32, monkeypatch, False, extra_one=True)
    assert f_feat == 256 and g_feat == 256
    assert np.array_equal(fast.view(np.uint32), gen.view(np.uint32))
    assert np.array_equal(fast1.view(np.uint32), gen1.view(np.uint32))
    o = oracle_mod.Oracle(holder, seed=5)
    o.execute(32)
    ref, cnt = o.accum()
    err = np.max(np.abs(fast - ref)) / 32
    print(f"axis scan, cornell 64x64 32 spp: L-inf on mean radiance against the oracle {err:.3e}")
    assert cnt == 32 and err <= TOL


@pytest.mark.gpu
def test_gpu_six_orientations_and_negative_zero_normals(monkeypatch, oracle_mod):
    render, holder = make_holder(six_plane_scene(res=(48, 40), sample=16))
    fast, _, f_feat = _gpu(render, 16, monkeypatch, True)
    gen, _, g_feat = _gpu(render, 16, monkeypatch, False)
    assert f_feat == 256 and g_feat == 256
    assert np.array_equal(fast.view(np.uint32), gen.view(np.uint32))
    o = oracle_mod.Oracle(holder, seed=5)
    o.execute(16)
    ref, _ = o.accum()
    assert np.max(np.abs(fast - ref)) / 16 <= TOL


@pytest.mark.gpu
def test_gpu_camera_on_a_plane_looking_along_an_axis(monkeypatch):
    """The camera sits exactly on the floor plane (o_k == pos_k) and looks along +y from x = 0: the centre column and row of
    pixels have direction components of exactly 0, so their wavefronts fall back to the generic body for those queries."""
    render, _ = make_holder(cornell_shaped(res=(64, 64), sample=32, bounce=8, cam_pos=(0, -1.2, -0.2)))
    fast, fast1, f_feat = _gpu(render, 32, monkeypatch, True, extra_one=True)
    gen, gen1, g_feat = _gpu(render, 32, monkeypatch, False, extra_one=True)
    assert f_feat == 256 and g_feat == 256
    assert np.isfinite(fast).all() and fast.any()
    assert np.array_equal(fast.view(np.uint32), gen.view(np.uint32))
    assert np.array_equal(fast1.view(np.uint32), gen1.view(np.uint32))
