"""The sphere arm of the axis body (csrc/mrt_trace.h trace, F_IDENT): the shifted origin pos + (o - pos) is formed
without the identity test of xf_vec, the rest is Sphere::intersect as the generic body runs it.  It must change no bit: every check
here compares with the generic body (MRT_AXIS_SCAN=0) as uint32.  The scene and the rays are the ones an order-changing sphere arm
would have to survive as well (a form that parked a lane's candidate and took its roots once per query was measured and dropped,
DESIGN.md §7): collinear spheres, two identical spheres (an exact key tie between two indices), sphere / plane pairs that return
bit-equal distances in either listing order, tangent rays, b around 1e-20, centres and origins with zeros of both signs, magnitudes
at which the discriminant overflows.

CPU: the x86 build of the same header (tests/emu/axis_probe.cpp).  GPU: constructed wavefronts through mrt_selftest_trace (ray i is
lane i % 64 of wavefront i / 64) that mix lanes for which 0, 1, 2 and more spheres pass both early returns of Sphere::intersect,
and renders through both launch shapes."""
import numpy as np
import pytest

from conftest import make_holder
from test_axis_scan import TOL, _gpu, _tame, cornell_shaped, probe, x86_render, x86_trace  # noqa: F401  (probe: the fixture)

f32 = np.float32
AXIS_MAX = f32(2.0 ** 38)
FAR_X, FAR_R = 2.0 ** 37, 2.0 ** 18


# ---- the scene -----------------------------------------------------------------------------------------------------------------
def roots_scene(res=(64, 64), sample=32, bounce=8):
    """A room of axis planes, open towards the camera, with five collinear spheres along x at z = 0.3 (indices 1, 2, 3, 5, 6; the
    middle one has zero centre components and an identical twin at index 7: an exact key tie on every ray through them), three
    collinear along y, a sphere cut by the wall listed before it, a sphere cut by the floor with a centre of zeros of both signs, a
    sphere that touches the floor listed before it and one that touches the ceiling listed after it, and a sphere 2^37 away."""
    return {
        "rt": {"sample": sample, "bounce": bounce},
        "frame": {"res": [int(res[0]), int(res[1])], "ssaa": 1, "cam": {"exp": 0.75, "fov": 70, "gamma": 0.5, "pos": [0.05, -1.3, 0.45]}},
        "scene": {"renderer": [
            {"type": "plane", "n": [0, 0, 1], "pos": [0, 0, 0], "mat": {"rough": 1}},                              # 0 floor, through the origin
            {"type": "sphere", "r": 0.2, "pos": [-0.6, 0, 0.3], "mat": {"glass": 0.08, "opacity": 0}},             # 1 (glass: t1 is used)
            {"type": "sphere", "r": 0.2, "pos": [-0.3, 0, 0.3], "mat": {"albedo": "#ff0000"}},                     # 2
            {"type": "sphere", "r": 0.2, "pos": [0, -0.0, 0.3], "mat": {"metal": 1}},                              # 3
            {"type": "plane", "n": [-1, 0, 0], "pos": [1, 0, 0], "mat": {"albedo": "#00ff00", "rough": 1}},        # 4
            {"type": "sphere", "r": 0.2, "pos": [0.3, 0, 0.3], "mat": {"rough": 1}},                               # 5
            {"type": "sphere", "r": 0.2, "pos": [0.6, 0, 0.3], "mat": {"glass": 0.08, "opacity": 0}},              # 6
            {"type": "sphere", "r": 0.2, "pos": [0, -0.0, 0.3], "mat": {"albedo": "#0000ff"}},                     # 7 = 3 again
            {"type": "plane", "n": [0, -1, 0], "pos": [0, 1, 0], "mat": {"rough": 1}},                             # 8 back wall
            {"type": "sphere", "r": 0.25, "pos": [0.4, 1.0, 0.6], "mat": {"metal": 1}},                            # 9 cut by 8
            {"type": "sphere", "r": 0.2, "pos": [-0.5, 0.5, 1.0], "mat": {"albedo": "#ffc177"}},                   # 10 touches 14
            {"type": "plane", "n": [1, 0, 0], "pos": [-1, 0, 0], "mat": {"albedo": "#ff0000", "rough": 1}},        # 11
            {"type": "sphere", "r": 0.2, "pos": [0.5, -0.5, 0.2], "mat": {"rough": 0.3, "metal": 0.5}},            # 12 touches 0
            {"type": "sphere", "r": 0.15, "pos": [-0.0, 0.6, -0.0], "mat": {"albedo": "#ffffff", "emit": 1.0}},    # 13 cut by 0
            {"type": "plane", "n": [0, 0, -1], "pos": [0, 0, 1.2], "mat": {"rough": 1}},                           # 14 ceiling
            {"type": "sphere", "r": 0.1, "pos": [-0.7, -0.6, 0.8], "mat": {"albedo": "#ffc177", "emit": 1.0}},     # 15, 16, 17 along y
            {"type": "sphere", "r": 0.1, "pos": [-0.7, -0.2, 0.8], "mat": {"rough": 1}},
            {"type": "sphere", "r": 0.1, "pos": [-0.7, 0.2, 0.8], "mat": {"metal": 1}},
            {"type": "sphere", "r": FAR_R, "pos": [FAR_X, 0, 0], "mat": {"rough": 1}},                             # 18
        ]},
    }


SPHERES = {i: (r["pos"], r["r"]) for i, r in enumerate(roots_scene()["scene"]["renderer"]) if r["type"] == "sphere"}
ROW = (1, 2, 3, 5, 6)          # the five along x


def candidates(o, d):
    """Per ray, the number of spheres that pass both early returns of Sphere::intersect, in float64: disc >= 0 and b <= 0 (rays
    whose disc or b is within rounding of zero may count differently in f32; the tests only ask for a mix)."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = np.zeros(o.shape[0], int)
    for pos, r in SPHERES.values():
        oo = o - np.array(pos, np.float64)
        b = 2 * (oo * d).sum(axis=1)
        disc = b * b - 4 * (d * d).sum(axis=1) * ((oo * oo).sum(axis=1) - r * r)
        n += (disc >= 0) & (b <= 0)
    return n


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32)


def _along_row(x0, sign, tilt=(3e-4, -2e-4), z=0.3, y=0.0):
    """A ray along the row of five from x = x0: every direction component inside the division window."""
    return (x0, y, z), tuple(_unit((sign, tilt[0], tilt[1])))


def _single_rays():
    up, dn = lambda v: np.nextafter(f32(v), f32(np.inf)), lambda v: np.nextafter(f32(v), f32(-np.inf))
    o, d = [], []

    def add(oo, dd):
        o.append(tuple(float(v) for v in oo)); d.append(tuple(float(v) for v in dd))

    # through 5 (and the twin), 3 and 2 spheres of the row, from both ends; from between them
    for x0, sg in ((-0.95, 1), (0.95, -1), (-0.15, 1), (0.15, -1), (0.15, 1), (-0.15, -1), (-0.45, 1), (0.45, -1), (0.45, 1), (-0.45, -1)):
        for tilt in ((3e-4, -2e-4), (-1e-3, 2e-3), (0.02, 0.01), (1e-9, 1e-9), (2.0 ** -40, -2.0 ** -40)):
            add(*_along_row(x0, sg, tilt))
    # the three along y, from both ends and from between
    for y0, sg in ((-0.95, 1), (0.9, -1), (-0.4, 1), (0.0, -1)):
        add((-0.7, y0, 0.8), _unit((1e-4, sg, -1e-4)))
    # origin at a centre (zero components of both signs), inside, on the surface, an ulp off it
    for pos, r in SPHERES.values():
        if r > 1:
            continue
        for dd in ((0.31, 0.57, -0.76), (-0.6, 0.3, 0.74), (0.9, -0.01, 0.02)):
            add(pos, dd); add((pos[0] + 0.5 * r, pos[1], pos[2] - 0.25 * r), dd)
            for k in range(3):
                for sg in (1, -1):
                    q = [f32(pos[0]), f32(pos[1]), f32(pos[2])]
                    q[k] = f32(q[k] + f32(sg * r))
                    add(q, dd)
                    q[k] = up(q[k]); add(q, dd)
                    q[k] = dn(dn(q[k])); add(q, dd)
    add((0.0, 0.0, 0.3), (0.31, 0.57, -0.76)); add((-0.0, -0.0, 0.3), (0.31, 0.57, -0.76)); add((0.0, 0.6, 0.0), (0.31, -0.57, 0.76))
    add((-0.0, 0.6, -0.0), (0.31, -0.57, 0.76)); add((0.0, 0.6, -0.0), (-0.31, 0.57, 0.76)); add((-0.0, 0.0, 0.0), (1e-3, 0.6, 1e-3))
    # tangent: along the top of the row (z = centre + r), the height a few ulps either side, directions that graze
    zt = f32(f32(0.3) + f32(0.2))
    for steps in range(-4, 5):
        z = zt
        for _ in range(abs(steps)):
            z = up(z) if steps > 0 else dn(z)
        for tilt in ((1e-9, 1e-9), (1e-9, -1e-9), (2.0 ** -40, 2.0 ** -40), (1e-5, 1e-7), (1e-5, -1e-7)):
            add(*_along_row(-0.95, 1, tilt, z=z)); add(*_along_row(0.95, -1, tilt, z=z))
    # b around 1e-20: from next to the centre of spheres 3 / 7 (centre x = 0, y = -0), b = 2 eps dx exactly
    for eps, dx in ((1e-9, 5e-12), (1e-9, 2.5e-12), (1e-9, 1e-11), (2e-9, 2.5e-12), (1e-8, 5e-13), (1e-10, 5e-11), (1e-9, float(up(5e-12))), (1e-9, float(dn(5e-12)))):
        for se in (1, -1):
            for sd in (1, -1):
                add((se * eps, 0.0, 0.3), (sd * dx, 0.6, 0.8)); add((se * eps, -0.0, 0.3), (sd * dx, 1e-6, -1e-6))
    # magnitudes near 2^38 / 2^40: disc overflows to inf or to inf - inf
    big = float(AXIS_MAX)
    for s in (1.0, 2.0 ** 20, 2.0 ** 30, 2.0 ** 39, 2.0 ** -20, 2.0 ** -39):
        for oo in ((big, 0.1, 0.3), (-big, 0.0, 0.3), (big, big, big), (0.1, -big, 0.3), (FAR_X - 2 * FAR_R, 0.0, 0.0), (FAR_X, 0.0, 0.0), (0.0, 0.0, 0.3)):
            for dd in ((1, 1e-3, 1e-3), (-1, 1e-3, -1e-3), (0.6, 0.6, 0.52), (-0.6, -0.6, -0.52), (1e-3, 1.0, 1e-3)):
                v = _unit(dd).astype(np.float64) * s
                if np.all(np.abs(v) <= 2.0 ** 40):
                    add(oo, v)
    add((0.1, 0.2, 0.3), (2.0 ** 40, 2.0 ** 40, -2.0 ** 40)); add((big, big, -big), (-2.0 ** 40, -2.0 ** 40, 2.0 ** 40))
    return np.array(o, f32), np.array(d, f32)


def _random_rays(n, seed):
    rng = np.random.default_rng(seed)
    ro = (rng.uniform(-1, 1, (n, 3)) * np.array([1.0, 1.3, 0.6]) + np.array([0, -0.2, 0.6])).astype(f32)
    rd = rng.normal(size=(n, 3))
    aim = rng.integers(0, 3, n)                                           # a third at a sphere, a third along the row
    keys = [k for k in SPHERES if k != 18]
    tgt = np.array([SPHERES[keys[i]][0] for i in rng.integers(0, len(keys), n)]) + rng.normal(size=(n, 3)) * 0.08
    rd[aim == 1] = (tgt - ro)[aim == 1]
    row = aim == 2
    ro[row] = (np.stack([rng.uniform(-1, 1, n), rng.normal(size=n) * 0.05, 0.3 + rng.normal(size=n) * 0.05], axis=1)).astype(f32)[row]
    rd[row] = np.stack([rng.choice([-1.0, 1.0], n), rng.normal(size=n) * 0.05, rng.normal(size=n) * 0.05], axis=1)[row]
    rd = _unit(rd)
    rd[::13] *= f32(1e-9); rd[5::13] *= f32(1e9)                          # directions that are not unit length
    ro[::17, 2] = 0.0
    return ro, rd


# ---- CPU: single queries through both bodies ------------------------------------------------------------------------------------
def _both(probe, holder, o, d):
    gen, fast = x86_trace(probe, holder, 0, o, d), x86_trace(probe, holder, 1, o, d)
    assert not gen[:, 5].any()
    assert np.array_equal(fast[:, 5] != 0, _tame(o, d))                   # the axis body answers exactly the rays the guard admits
    bad = np.flatnonzero(~(gen[:, :5] == fast[:, :5]).all(axis=1))
    assert bad.size == 0, (o[bad[:4]], d[bad[:4]], gen[bad[:4]], fast[bad[:4]])
    return gen


def test_constructed_rays_answer_alike_in_both_bodies(probe):
    _, holder = make_holder(roots_scene(res=(16, 16), sample=1))
    o, d = _single_rays()
    gen = _both(probe, holder, o, d)
    tame = _tame(o, d)
    assert tame.sum() > 700
    nc = candidates(o, d)
    assert {0, 1, 2, 3, 6} <= set(nc[tame].tolist())                      # 6: the whole row and the twin
    won = set(gen[tame & (gen[:, 0] != 0), 1].tolist())
    assert {1, 2, 3, 5, 6, 13, 15, 16, 17} <= won and 7 not in won        # the twin never wins: the earlier index keeps a tie
    t0 = gen[:, 2].view(f32)
    assert np.isnan(t0[tame & (gen[:, 0] != 0)]).any()                    # an overflowed disc: NaN roots, the smallest key, are a hit


def test_twin_spheres_tie_and_the_earlier_index_wins(probe):
    """Spheres 3 and 7 are the same sphere: every ray whose closest hit is that sphere has two candidates with one key."""
    _, holder = make_holder(roots_scene(res=(16, 16), sample=1))
    rng = np.random.default_rng(5)
    n = 1500
    ro = (rng.uniform(-1, 1, (n, 3)) * np.array([0.25, 0.9, 0.25]) + np.array([0, -0.3, 0.45])).astype(f32)
    rd = _unit(np.array([0, 0, 0.3]) + rng.normal(size=(n, 3)) * 0.1 - ro)
    gen = _both(probe, holder, ro, rd)
    assert (gen[:, 1] == 3).sum() > 700 and not (gen[:, 1] == 7).any()
    # the twin alone answers with the same bits: the tie is exact
    d7 = roots_scene(res=(16, 16), sample=1)
    d7["scene"]["renderer"][3] = {"type": "sphere", "r": 0.05, "pos": [0.9, 0.9, 1.1], "mat": {"rough": 1}}
    _, h7 = make_holder(d7)
    g7 = _both(probe, h7, ro, rd)
    m = gen[:, 1] == 3
    assert (g7[m, 1] == 7).all() and np.array_equal(g7[m, 2:4], gen[m, 2:4])


def _hexes(*v):
    return [float.fromhex(s) for s in v]


# Found by a search on the CPU (4000 rays at the sphere below; a plane with normal (-1, 0, 0) stepped in ulps around the x of the
# ray's hit point until Plane::intersect returns the bits of the sphere's t0): (plane x, origin, direction, bits of t)
TIES = [
    ("0x1.981606p-9", _hexes("-0x1.5592bep-1", "-0x1.531f5ap-1", "-0x1.039518p-4"), _hexes("0x1.52704ap-1", "0x1.615a48p-1", "0x1.2da154p-2"), 0x3f81c9d6),
    ("-0x1.182e02p-4", _hexes("-0x1.6ab0b8p-1", "-0x1.45af7ap-1", "-0x1.944cfcp-9"), _hexes("0x1.43d0d8p-1", "0x1.7115ecp-1", "0x1.22434ep-2"), 0x3f8185cd),
    ("-0x1.7d5424p-4", _hexes("-0x1.b5851cp-1", "-0x1.1646c6p-1", "-0x1.7e2c42p-5"), _hexes("0x1.679cb0p-1", "0x1.46a184p-1", "0x1.43543ap-2"), 0x3f8ac3a6),
]


@pytest.mark.parametrize("tie", range(len(TIES)))
def test_sphere_then_plane_tie_is_decided_by_the_index(probe, tie):
    """Sphere i and a LATER plane j return bit-equal t: the first minimum is the sphere, by the index term of the (key, index) rule
    alone (a scan that meets its candidates in order has it in its strict comparison; one that resolves a sphere late does not)."""
    px, o, d, bits = TIES[tie]
    sph = {"type": "sphere", "r": 0.2, "pos": [0.1, 0.2, 0.3], "mat": {"rough": 1}}
    pln = {"type": "plane", "n": [-1, 0, 0], "pos": [float.fromhex(px), 0, 0], "mat": {"rough": 1}}
    o, d = np.array([o], f32), np.array([d], f32)

    def scene(rends):
        s = roots_scene(res=(8, 8), sample=1)
        s["scene"]["renderer"] = rends
        return make_holder(s)[1]

    s_only, p_only = _both(probe, scene([sph]), o, d), _both(probe, scene([pln]), o, d)
    assert s_only[0, 0] == 1 and p_only[0, 0] == 1 and s_only[0, 2] == bits and p_only[0, 2] == bits
    assert s_only[0, 3] != bits                                           # the sphere's exit distance tells the two hits apart
    both = _both(probe, scene([sph, pln]), o, d)
    assert tuple(both[0, :4]) == (1, 0, bits, s_only[0, 3])               # the generic body's answer: the sphere, index 0
    rev = _both(probe, scene([pln, sph]), o, d)
    assert tuple(rev[0, :4]) == (1, 0, bits, bits)                        # listed the other way round the plane is the earlier one
    # and with other candidates around the pair: a sphere in front of the ray's origin side that it misses, one behind the plane
    more = [{"type": "sphere", "r": 0.2, "pos": [0.7, 0.9, 0.6], "mat": {"rough": 1}}, sph, {"type": "plane", "n": [0, 0, 1], "pos": [0, 0, -2], "mat": {"rough": 1}},
            pln, {"type": "sphere", "r": 0.3, "pos": [0.5, 0.6, 0.5], "mat": {"rough": 1}}]
    m = _both(probe, scene(more), o, d)
    assert tuple(m[0, :4]) == (1, 1, bits, s_only[0, 3])


def test_random_rays_answer_alike_in_both_bodies(probe):
    _, holder = make_holder(roots_scene(res=(16, 16), sample=1))
    o, d = _random_rays(6000, 17)
    gen = _both(probe, holder, o, d)
    nc = candidates(o, d)
    assert (nc >= 2).sum() > 1000 and (nc == 0).sum() > 300
    assert len(set(gen[gen[:, 0] != 0, 1].tolist())) >= 15


def test_x86_render_is_bit_identical_with_and_without_the_axis_body(probe):
    _, holder = make_holder(roots_scene(res=(16, 16), sample=8))
    a, sa = x86_render(probe, holder, 1, 5, 8)
    b, sb = x86_render(probe, holder, 0, 5, 8)
    assert sa == sb and sa >= 16 * 16 * 8 and np.isfinite(a).all() and a.any()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def _pool():
    """Tame rays by their number of candidates (float64 count; rays near a decision are left out)."""
    o, d = _random_rays(20000, 23)
    so, sd = _single_rays()
    o, d = np.concatenate([o, so]), np.concatenate([d, sd])
    keep = _tame(o, d)
    o, d = o[keep], d[keep]
    nc = candidates(o, d)
    return o, d, {0: np.flatnonzero(nc == 0), 1: np.flatnonzero(nc == 1), 2: np.flatnonzero(nc == 2), 3: np.flatnonzero(nc >= 3)}


def _wavefronts():
    """Wavefronts of 64 lanes by recipe: (candidate class of most lanes, class of a few lanes, how many of those)."""
    o, d, cls = _pool()
    rng = np.random.default_rng(29)
    assert all(len(v) >= 64 for v in cls.values())
    recipes = [(0, 0, 0), (1, 1, 0), (2, 2, 0), (3, 3, 0),                # nobody is a candidate; everybody is; everybody clashes
               (0, 1, 1), (0, 2, 1), (0, 3, 1), (1, 2, 1), (1, 3, 1), (1, 0, 1), (3, 0, 1), (2, 1, 3), (0, 3, 5), (1, 3, 7), (1, 2, 31), (0, 1, 32)]
    idx = []
    for most, few, k in recipes * 3:
        w = rng.choice(cls[most], 64)
        w[rng.choice(64, k, replace=False)] = rng.choice(cls[few], k)
        idx.append(w)
    for _ in range(24):                                                   # any mix
        idx.append(np.concatenate([rng.choice(cls[c], 16) for c in (0, 1, 2, 3)])[rng.permutation(64)])
    idx = np.concatenate(idx)
    return o[idx], d[idx]


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
def test_gpu_constructed_wavefronts_change_no_bit(monkeypatch, probe):
    render, holder = make_holder(roots_scene(res=(16, 16), sample=1))
    o, d = _wavefronts()
    assert o.shape[0] % 64 == 0 and _tame(o, d).all()                     # every wavefront takes the axis body
    fast, f_feat = _gpu_trace(monkeypatch, render, True, o, d)
    gen, g_feat = _gpu_trace(monkeypatch, render, False, o, d)
    assert f_feat == 256 and g_feat == 256
    bad = np.flatnonzero((fast != gen).any(axis=1))
    assert bad.size == 0, (bad[:8] // 64, bad[:8] % 64, o[bad[:4]], d[bad[:4]], gen[bad[:4]], fast[bad[:4]])
    assert fast[:, 0].mean() > 0.9
    # the closest-hit words are the x86 build's too: hit, t0, t1 of the generic body, and its flat instance index, which is the
    # renderer's here (every renderer of the scene has one instance, the hook reports the index within the renderer: 0)
    want = x86_trace(probe, holder, 0, o, d)
    assert np.array_equal(fast[:, 0], want[:, 0])
    h = want[:, 0] != 0
    assert np.array_equal(fast[h][:, [2, 4, 5]], want[h][:, 1:4]) and not fast[h][:, 3].any()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["roots_scene", "cornell"])
def test_gpu_renders_change_no_bit(monkeypatch, oracle_mod, which):
    desc = roots_scene(res=(64, 64), sample=32, bounce=8) if which == "roots_scene" else cornell_shaped(res=(64, 64), sample=32, bounce=8)
    render, holder = make_holder(desc)
    fast, fast1, f_feat = _gpu(render, 32, monkeypatch, True, extra_one=True)
    gen, gen1, g_feat = _gpu(render, 32, monkeypatch, False, extra_one=True)
    assert f_feat == 256 and g_feat == 256
    assert np.isfinite(fast).all() and fast.any()
    assert np.array_equal(fast.view(np.uint32), gen.view(np.uint32))
    assert np.array_equal(fast1.view(np.uint32), gen1.view(np.uint32))
    o = oracle_mod.Oracle(holder, seed=5)
    o.execute(32)
    ref, cnt = o.accum()
    err = np.max(np.abs(fast - ref)) / 32
    print(f"sphere arm of the axis scan, {which} 64x64 32 spp: L-inf on mean radiance against the oracle {err:.3e}")
    assert cnt == 32 and err <= TOL
