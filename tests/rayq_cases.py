"""Ray families of the ray-query tests (tests/test_ray_query_host.py, tests/test_gpu_ray_query.py): the inputs a render never
produces -- zero, infinite and NaN components, origins exactly on a surface, rays through shared edges and vertices, tangent rays,
equal-distance ties, values at the ends of the fast-division window -- as plain seeded functions.  A family is a list of Case:
one scene, one set of rays, and the Variants (kernel instantiation, the environment that makes mrt_create pick it, the x86
probe's switches) the rays are run through.  Rays are traced as given: no shift of the origin, no normalisation."""
import copy

import numpy as np

f32 = np.float32
from micro_raytracer_amd._abi import F_ALL, F_BOX, F_BVH, F_COLD, F_DEEP, F_ENV, F_IDENT, F_LIGHTS, F_MAPS, F_TRI, F_VATTR  # noqa: F401

FN = F_ALL & ~F_TRI
WIN_LO, WIN_HI = f32(2.0 ** -40), f32(2.0 ** 40)


class Variant:
    """One kernel instantiation of a case: feat / lds = what mrt_stats must report under env (MRT_BLOCK_THREADS=256 is always
    added); wide / hot / walk_cap = the x86 probe's packing switches that reproduce the context's."""

    def __init__(self, label, feat, lds=True, env=None, wide=0, hot=0, walk_cap=0):
        self.label, self.feat, self.lds = label, feat, lds
        self.env = dict(env or {})
        self.env["MRT_BLOCK_THREADS"] = "256"
        self.wide, self.hot, self.walk_cap = wide, hot, walk_cap

    def cfg(self, axis=1, ref_walk=0):
        return np.array([self.feat, axis, self.wide, self.hot, self.walk_cap, ref_walk, 0, 0], np.uint32)


class Case:
    def __init__(self, name, desc, o, d, variants):
        self.name, self.desc, self.variants = name, desc, variants
        self.o, self.d = np.ascontiguousarray(o, f32), np.ascontiguousarray(d, f32)
        assert self.o.shape == self.d.shape and self.o.shape[1] == 3


LDS_ALL = {"MRT_COLD": "0"}           # mesh scenes: the whole scene in LDS, not the warm level plan_launch prefers
L2 = {"MRT_SCENE_IN_L2": "1"}


def wild(o, d):
    """The rays outside the issue's "must agree" class: an origin or direction component that is not finite, or a non-zero one
    outside [2^-40, 2^40].  Stated on the input alone."""
    v = np.concatenate([o, d], axis=1)
    a = np.abs(v)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(v) & ((v == 0) | ((a >= WIN_LO) & (a <= WIN_HI)))
    return ~ok.all(axis=1)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-300)


def _special_components(rng, o0, d0):
    """Zero, +-inf and NaN components, one at a time, in the direction and (inf, NaN) in the origin; non-unit directions."""
    o, d = [], []
    for i in range(len(o0)):
        for bad in (0.0, -0.0, np.inf, -np.inf, np.nan):
            k = int(rng.integers(0, 3))
            e = d0[i].copy(); e[k] = bad
            o.append(o0[i]); d.append(e)
        k = int(rng.integers(0, 3))
        q = o0[i].copy(); q[k] = (np.inf, -np.inf, np.nan)[i % 3]
        o.append(q); d.append(d0[i])
        o.append(o0[i]); d.append(d0[i] * f32(1e-9))
        o.append(o0[i]); d.append(d0[i] * f32(1e9))
    return np.array(o, f32), np.array(d, f32)


# ---- axis ------------------------------------------------------------------------------------------------------------------------
def axis_rays():
    """_adversarial_rays() plus the 4000 random rays of test_both_scan_bodies_answer_every_ray_alike."""
    from test_axis_scan import _adversarial_rays
    o, d = _adversarial_rays()
    rng = np.random.default_rng(11)
    n = 4000
    ro = rng.uniform(-1, 1, (n, 3)).astype(f32) * f32(1.2) + np.array([0, 0, 0.5], f32)
    rd = rng.normal(size=(n, 3)).astype(f32)
    rd /= np.linalg.norm(rd, axis=1, keepdims=True).astype(f32)
    ro[::7, 2] = 0.0
    ro[::11, 0] = 1.0
    rd[::13] *= f32(1e-9); rd[5::13] *= f32(1e9)
    # tame rays that leave 1e-30 .. 2^-40 above or below the plane through the origin and run into it: a numerator below the
    # division window against the plane they hit first (six_plane_scene's floor, either side)
    m = 256
    so = rng.uniform(-0.8, 0.8, (m, 3)).astype(f32)
    so[:, 2] = (10.0 ** rng.uniform(-30.0, -12.1, m) * rng.choice([-1.0, 1.0], m)).astype(f32)
    sd = rng.normal(size=(m, 3)).astype(f32)
    sd /= np.linalg.norm(sd, axis=1, keepdims=True).astype(f32)
    sd[:, 2] = -np.sign(so[:, 2]) * np.maximum(np.abs(sd[:, 2]), f32(0.05))
    return np.concatenate([o, ro, so]), np.concatenate([d, rd, sd])


def axis(oracle_mod=None):
    from test_axis_scan import cornell_shaped, six_plane_scene
    o, d = axis_rays()
    v = [Variant("lds ident", F_IDENT)]
    return [Case("six_planes", six_plane_scene(), o, d, v), Case("cornell_shaped", cornell_shaped(res=(16, 16), sample=1), o, d, v)]


# ---- surface -----------------------------------------------------------------------------------------------------------------------
def _kitchen(full):
    from micro_raytracer_amd import scenes
    d = scenes.kitchen_sink(res=(16, 16), sample=1)
    if not full:
        d["scene"]["renderer"] = [r for r in d["scene"]["renderer"] if r["type"] not in ("triangle", "mesh")]
    return d


def _first_hits(oracle_mod, desc, o, d):
    from conftest import make_holder
    _, holder = make_holder(desc)
    orc = oracle_mod.Oracle(holder, seed=1)
    out = orc.ray_query(o, d)
    orc.close()
    return out


def surface_rays(oracle_mod, desc, seed):
    rng = np.random.default_rng(seed)
    R = desc["scene"]["renderer"]
    os_, ds_ = [], []

    def add(o, d):
        os_.append(np.asarray(o, f32).reshape(-1, 3)); ds_.append(np.asarray(d, f32).reshape(-1, 3))

    # origins on a surface: o + t0 d of a first query (as f32, the kernel's own p0), a new random direction
    n = 1500
    o0 = (rng.uniform(-1.2, 1.2, (n, 3)) + np.array([0, -0.6, 0.4])).astype(f32)
    tgt = rng.uniform(-0.8, 0.8, (n, 3)) + np.array([0, 0.3, -0.1])
    d0 = _unit(tgt - o0).astype(f32)
    add(o0, d0)
    first = _first_hits(oracle_mod, desc, o0, d0)
    h = first[:, 0] == 1
    t0 = first[h, 4].view(f32)
    p = (o0[h] + d0[h] * t0[:, None]).astype(f32)
    add(p, _unit(rng.normal(size=p.shape)).astype(f32))
    # spheres: tangent rays (the line touches the sphere at c + r u), and rays from inside (t0 < 0 < t1)
    for r in R:
        if r["type"] != "sphere":
            continue
        for inst in (r.get("inst") or [[r.get("pos", [0, 0, 0]), None]]):
            c, rad = np.asarray(inst[0], np.float64), float(r["r"])
            m = 40
            u = _unit(rng.normal(size=(m, 3)))
            w = _unit(np.cross(u, rng.normal(size=(m, 3))))
            s = rng.uniform(0.5, 3.0, (m, 1)) * rng.choice([-1.0, 1.0], (m, 1))
            add(c + rad * u + s * w, -np.sign(s) * w)
            add(c + rad * 0.6 * rng.uniform(-1, 1, (m, 3)) / np.sqrt(3), _unit(rng.normal(size=(m, 3))))
    # the untransformed box: rays in a face, along an edge, through a corner
    b = next(r for r in R if r["type"] == "box" and "dir" not in r)
    c, hs = np.asarray(b["pos"], np.float64), 0.5 * np.asarray(b["sizes"], np.float64)
    for k in range(3):
        for sg in (-1.0, 1.0):
            m = 30
            q = c + rng.uniform(-2, 2, (m, 3)) * hs
            q[:, k] = f32(c[k]) + sg * f32(hs[k])                      # on the face's plane
            dd = _unit(rng.normal(size=(m, 3))); dd[:, k] = 0.0; dd = _unit(dd)
            add(q, dd)
            j = (k + 1) % 3
            e = c + np.zeros((m, 3)); e[:, k] = f32(c[k]) + sg * f32(hs[k]); e[:, j] = f32(c[j]) + rng.choice([-1.0, 1.0], m) * f32(hs[j])
            i = (k + 2) % 3
            e[:, i] = c[i] + rng.uniform(-3, 3, m) * hs[i]
            ax = np.zeros((m, 3)); ax[:, i] = rng.choice([-1.0, 1.0], m)
            add(e, ax)                                               # along an edge
    corners = c + hs * np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    for cn in corners:
        q = cn + _unit(rng.normal(size=(20, 3))) * rng.uniform(0.3, 2.0, (20, 1))
        add(q, _unit(cn - q))
    # the plane: rays parallel to it, rays lying in it
    pl = next(r for r in R if r["type"] == "plane")
    z = float(pl["pos"][2])
    m = 80
    q = rng.uniform(-1, 1, (m, 3)); q[:, 2] = z + rng.uniform(0.01, 1.0, m)
    dd = rng.normal(size=(m, 3)); dd[:, 2] = 0.0
    add(q, _unit(dd))
    q = rng.uniform(-1, 1, (m, 3)); q[:, 2] = z
    dd = rng.normal(size=(m, 3)); dd[:, 2] = 0.0
    add(q, _unit(dd))
    # the triangle: rays through its edge midpoints and vertices
    for r in R:
        if r["type"] != "triangle":
            continue
        v = np.asarray(r["vtx"], np.float64) + np.asarray(r["pos"], np.float64)
        pts = np.concatenate([v, 0.5 * (v + np.roll(v, 1, axis=0)), v.mean(axis=0, keepdims=True)])
        for pt in pts:
            q = pt + _unit(rng.normal(size=(40, 3))) * rng.uniform(0.2, 2.0, (40, 1))
            add(q, _unit(pt - q))
    # zero, infinite and NaN components; directions that are not unit length
    so, sd = _special_components(rng, o0[:40], d0[:40])
    add(so, sd)
    return np.concatenate(os_), np.concatenate(ds_)


def surface(oracle_mod):
    full, plain = _kitchen(True), _kitchen(False)
    o, d = surface_rays(oracle_mod, full, 21)
    po, pd = surface_rays(oracle_mod, plain, 22)
    return [Case("kitchen_sink", full, o, d, [Variant("lds all", F_ALL, env=LDS_ALL), Variant("l2 all", F_ALL, lds=False, env=L2)]),
            Case("kitchen_sink_no_triangles", plain, po, pd, [Variant("lds fn", FN)])]


# ---- ties --------------------------------------------------------------------------------------------------------------------------
ROT = [0.3, 0.2, -1, 0.4]


def _dup_renderers():
    """Two and three instances of one renderer at the same position and direction, and two renderers that coincide."""
    two = [[[0.4, 1.0, 0.2], ROT]] * 2
    three = [[[-0.5, 1.1, 0.3], [0, 0, -1, 0]]] * 3
    return [{"type": "box", "sizes": [0.3, 0.4, 0.2], "mat": {"rough": 0.6}, "inst": two},
            {"type": "sphere", "r": 0.3, "mat": {"albedo": "#ff2020"}, "inst": three},
            {"type": "sphere", "r": 0.3, "mat": {"albedo": "#2020ff"}, "inst": three},
            {"type": "box", "sizes": [0.25, 0.25, 0.25], "pos": [0.0, 1.4, -0.1], "dir": ROT, "mat": {"metal": 1}},
            {"type": "box", "sizes": [0.25, 0.25, 0.25], "pos": [0.0, 1.4, -0.1], "dir": ROT, "mat": {"rough": 1}}]


DUP_TARGETS = np.array([[0.4, 1.0, 0.2], [-0.5, 1.1, 0.3], [0.0, 1.4, -0.1]])


def _aimed(rng, targets, n, spread):
    t = targets[rng.integers(0, len(targets), n)] + rng.uniform(-spread, spread, (n, 3))
    o = t + _unit(rng.normal(size=(n, 3))) * rng.uniform(0.8, 3.0, (n, 1))
    return o.astype(f32), _unit(t - o).astype(f32)


def _lattice_rays(rng, n, step, lo, hi, off):
    """Axis-parallel rays from lattice points (two zero direction components) and diagonal ones (one zero component)."""
    o = (rng.integers(lo, hi, (n, 3)) * step + off).astype(f32)
    d = np.zeros((n, 3))
    k = rng.integers(0, 3, n)
    d[np.arange(n), k] = rng.choice([-1.0, 1.0], n)
    diag = rng.random(n) < 0.4
    d[diag, (k[diag] + 1) % 3] = rng.choice([-1.0, 1.0], int(diag.sum()))
    return o, d.astype(f32)


def ties(oracle_mod=None):
    import edge_cases
    from micro_raytracer_amd import scenes
    from test_fuzz_scenes import crowd_scene
    out = []
    rng = np.random.default_rng(31)
    ec = edge_cases.cases()
    # linear scan: the kitchen sink plus the coincident renderers
    d = scenes.kitchen_sink(res=(16, 16), sample=1)
    d["scene"]["renderer"] += _dup_renderers()
    o1, d1 = _aimed(rng, DUP_TARGETS, 1500, 0.25)
    o2, d2 = _aimed(rng, np.array([[0.0, 0.3, 0.0]]), 500, 0.8)
    so, sd = _special_components(rng, o1[:20], d1[:20])
    out.append(Case("coincident_linear", d, np.concatenate([o1, o2, so]), np.concatenate([d1, d2, sd]), [Variant("lds all", F_ALL, env=LDS_ALL)]))
    # instance BVH: the same renderers among 80 boxes and spheres (tests/edge_cases.py), in LDS and through L2
    d = copy.deepcopy(ec["bvh_mixed_rotated_and_coincident"])
    d["frame"]["res"] = [16, 16]
    d["scene"]["renderer"] += _dup_renderers()[:1] + _dup_renderers()[3:]
    o1, d1 = _aimed(rng, DUP_TARGETS[[0, 2, 0, 2, 0]], 1200, 0.25)
    o1b, d1b = _aimed(rng, np.array([[0.4, 1.0, 0.2]]), 600, 0.3)          # edge_cases' own coincident spheres
    o2, d2 = _aimed(rng, np.array([[0.0, 0.0, 0.0]]), 800, 3.0)
    so, sd = _special_components(rng, o1[:20], d1[:20])
    out.append(Case("coincident_bvh", d, np.concatenate([o1, o1b, o2, so]), np.concatenate([d1, d1b, d2, sd]),
                    [Variant("lds all bvh", F_ALL | F_BVH, env=LDS_ALL), Variant("l2 all bvh", F_ALL | F_BVH, lds=False, env=L2)]))
    # the sphere lattice without its light: F_IDENT | F_BVH; rays along the lattice rows (BVH split planes), zero components
    d = scenes.instance_grid(res=(16, 16), sample=1, n=6)
    d["scene"]["light"] = []
    o1, d1 = _lattice_rays(rng, 1200, 0.5, -2, 8, np.array([0.0, 0.0, 0.0]))
    o1b, d1b = _lattice_rays(rng, 600, 0.25, -4, 16, np.array([0.0, 0.0, 0.0]))      # between the rows too: the cell boundaries
    o2, d2 = _aimed(rng, np.array([[1.25, 1.25, 1.25]]), 1200, 1.5)
    out.append(Case("instance_grid", d, np.concatenate([o1, o1b, o2]), np.concatenate([d1, d1b, d2]), [Variant("lds ident bvh", F_IDENT | F_BVH)]))
    # a random crowd
    d = crowd_scene(3)
    o1, d1 = _aimed(rng, np.array([[0.0, 0.0, 0.0]]), 2000, 3.0)
    out.append(Case("crowd_scene_3", d, o1, d1, [Variant("lds crowd", None, env=LDS_ALL)]))
    # identities that differ in the sign of a zero (must stay off F_IDENT) / one sign everywhere (must take F_IDENT)
    for name, feat in (("mixed", F_BOX | F_LIGHTS), ("uniform", F_IDENT | F_BOX | F_LIGHTS)):
        o1, d1 = _lattice_rays(rng, 1200, 0.5, -4, 5, np.array([0.0, 0.0, 0.0]))
        o2, d2 = _aimed(rng, np.array([[0.0, 0.8, 0.0]]), 800, 1.0)
        out.append(Case(f"ident_zero_signs_{name}", ec[f"ident_zero_signs_{name}"], np.concatenate([o1, o2]), np.concatenate([d1, d2]),
                        [Variant("lds " + name, feat)]))
    return out


# ---- mesh --------------------------------------------------------------------------------------------------------------------------
def _mesh_desc(tris, inst, crowd=False):
    """The mesh (one renderer, `inst` its instances), a textured plane far below and a light: the full feature set, so that
    every staging level has a kernel at 256 threads."""
    from micro_raytracer_amd import scenes
    rend = [{"type": "mesh", "mesh": [[[float(c) for c in v] for v in t] for t in tris], "inst": inst, "mat": {"rough": 0.5}},
            {"type": "plane", "n": [0, 0, 1], "pos": [0, 0, -60.0], "mat": {"rough": 1, "tex": scenes.checker_texture(4, 4, 1)}}]
    if crowd:
        rend.append({"type": "sphere", "r": 0.05, "mat": {"rough": 0.3},
                     "inst": [[[-1.5 + 0.1 * i, 0.3 * ((i % 5) - 2), 0.2 * ((i % 3) - 1)], [0, 0, -1, 0]] for i in range(30)]})
    return {"rt": {"sample": 1, "bounce": 2}, "frame": {"res": [8, 8], "ssaa": 1, "cam": {"pos": [0, -4, 0]}},
            "scene": {"renderer": rend, "light": [{"type": "point", "pos": [0, -3, 2], "pwr": 0.5, "color": "#ffffff"}]}}


def mesh_variants(bvh=False):
    b = F_BVH if bvh else 0
    return [Variant("lds all", F_ALL | b, env=LDS_ALL),
            Variant("warm", F_ALL | b | F_COLD, env={"MRT_COLD": "1"}),
            Variant("deep 3/4", F_ALL | b | F_COLD | F_DEEP, env={"MRT_DEEP_NODES": "3", "MRT_WALK_CAP": "4"}, wide=1, hot=3, walk_cap=4),
            Variant("deep 40/6", F_ALL | b | F_COLD | F_DEEP, env={"MRT_DEEP_NODES": "40", "MRT_WALK_CAP": "6"}, wide=1, hot=40, walk_cap=6),
            Variant("l2", F_ALL | b, lds=False, env=L2)]


def mesh(oracle_mod=None):
    from mesh_probe import random_mesh, rays_for
    out = []
    for kind in range(5):
        rng = np.random.default_rng(100 + kind)
        tris = np.asarray(random_mesh(rng, kind), f32)
        pos = [float(x) for x in rng.uniform(-0.5, 0.5, 3)] if kind % 2 else [0.0, 0.0, 0.0]
        o, d = rays_for(rng, tris, 2000)
        o = np.ascontiguousarray(o + np.asarray(pos, f32))
        out.append(Case(f"mesh_kind{kind}", _mesh_desc(tris, [[pos, [0, 0, -1, 0]]]), o, d, mesh_variants()))
    rng = np.random.default_rng(105)
    tris = np.asarray(random_mesh(rng, 1), f32)
    inst = [[[0.0, 0.0, 0.0], [0.3, 0.2, -1, 0.4]], [[1.2, 0.4, 0.1], [-0.5, 0.1, -1, -0.3]], [[-1.1, -0.3, 0.2], [0.1, 0.7, -1, 1.2]]]
    o, d = rays_for(rng, tris, 2000)
    o = np.ascontiguousarray(o + np.array([i[0] for i in inst], f32)[rng.integers(0, 3, 2000)])
    out.append(Case("mesh_three_rotated_instances", _mesh_desc(tris, inst), o, d, mesh_variants()))
    out.append(Case("mesh_three_rotated_instances_crowd", _mesh_desc(tris, inst, crowd=True), o, d, [mesh_variants(bvh=True)[3]]))
    return out


# ---- attributes ----------------------------------------------------------------------------------------------------------------------
def _vertex_edge_rays(rng, tris, pos, n):
    """Rays at vertices (a corner weight of 1), edge midpoints and edge points (a weight of 0) and centroids of random triangles."""
    t = np.asarray(tris, np.float64)[rng.integers(0, len(tris), n)] + np.asarray(pos, np.float64)
    k = rng.integers(0, 4, n)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    s = rng.uniform(0, 1, (n, 1))
    tgt = np.where((k == 0)[:, None], a, np.where((k == 1)[:, None], 0.5 * (a + b), np.where((k == 2)[:, None], b + s * (c - b), (a + b + c) / 3)))
    tgt = np.where((rng.random(n) < 0.3)[:, None], tgt.astype(f32).astype(np.float64), tgt)      # the stored vertex itself
    o = tgt + _unit(rng.normal(size=(n, 3))) * rng.uniform(0.3, 2.5, (n, 1))
    return o.astype(f32), _unit(tgt - o).astype(f32)


def attributes(oracle_mod=None):
    import test_oracle_ext as X
    out = []
    rng = np.random.default_rng(41)
    for name, desc, feat in (("smooth", X.smooth(), F_ALL | F_VATTR), ("env_sphere_nearest", X.env("sphere", "nearest"), F_ALL | F_VATTR | F_ENV)):
        desc = copy.deepcopy(desc)
        desc["frame"]["res"] = [16, 16]
        m = desc["scene"]["renderer"][0]
        o, d = _vertex_edge_rays(rng, m["mesh"], m["pos"], 3000)
        out.append(Case(name, desc, o, d, [Variant("lds vattr" + (" env" if feat & F_ENV else ""), feat, env=LDS_ALL)]))
    # single triangles with vn + uv, vn only, uv only, vn all zero (the face normal), under rotated instances
    desc = copy.deepcopy(X.triangles())
    desc["frame"]["res"] = [16, 16]
    os_, ds_ = [], []
    for r in desc["scene"]["renderer"]:
        if r["type"] != "triangle" or "dir" in r:
            continue
        o, d = _vertex_edge_rays(rng, [r["vtx"]], r["pos"], 500)
        os_.append(o); ds_.append(d)
    o, d = _aimed(rng, np.array([[0.0, 0.45, 0.0]]), 1000, 0.8)              # the rotated ones and the floor
    out.append(Case("triangles", desc, np.concatenate(os_ + [o]), np.concatenate(ds_ + [d]), [Variant("lds vattr", F_ALL | F_VATTR, env=LDS_ALL)]))
    return out


# ---- running a case: the x86 probe, the oracle, the comparison rules ---------------------------------------------------------------
def _bind(L):
    import ctypes as C
    fp, u32p, vp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_void_p
    L.rq_error.restype = C.c_char_p
    L.rq_pack.argtypes = [vp, vp, C.c_uint32, u32p]
    L.rq_trace.argtypes = [vp, vp, u32p, C.c_uint32, fp, fp, u32p, u32p]


def shared_probe():
    """tests/emu/rayq_probe.cpp, built once per process and loaded with ctypes; skips the test where there is no g++."""
    from emu.build import shared
    return shared("rayq_probe", _bind)


def probe_trace(L, holder, cfg, o, d):
    """(words uint32 [n][9] with the instance numbered within its renderer, as the hook returns it; axis-body count [n])."""
    import ctypes as C
    u32p = C.POINTER(C.c_uint32)
    o, d = np.ascontiguousarray(o, f32), np.ascontiguousarray(d, f32)
    cfg = np.ascontiguousarray(cfg, np.uint32)
    out = np.zeros((o.shape[0], 10), np.uint32)
    ext = holder.ext_ptr() if hasattr(holder, "ext_ptr") else None
    info = np.zeros(8, np.uint32)
    rc = L.rq_pack(C.cast(holder.ptr(), C.c_void_p), ext, int(cfg[2]), info.ctypes.data_as(u32p))
    assert rc == 0, (rc, L.rq_error())
    first = np.zeros(max(1, int(info[4])), np.uint32)
    rc = L.rq_trace(C.cast(holder.ptr(), C.c_void_p), ext, cfg.ctypes.data_as(u32p), o.shape[0], o.ctypes.data_as(C.POINTER(C.c_float)),
                    d.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(u32p), first.ctypes.data_as(u32p))
    assert rc == 0, (rc, L.rq_error())
    w = out[:, :9].copy()
    h = w[:, 0] == 1
    w[h, 3] -= first[w[h, 2]]
    return w, out[:, 9]


def same_words(a, b):
    """Per ray: hit, any and ids equal; t0, t1 and the normal bit-equal, NaN equal to NaN (test_oracle_aov.compare_aov's rule)."""
    eq = a == b
    fa, fb = a[:, 4:].view(f32), b[:, 4:].view(f32)
    eq[:, 4:] |= np.isnan(fa) & np.isnan(fb)
    return eq.all(axis=1)


def ulp_distance(a, b):
    """Largest distance in ulps between the finite float words (t0, t1, normal) of rays both sides hit."""
    both = (a[:, 0] == 1) & (b[:, 0] == 1)
    fa, fb = a[both, 4:].view(f32), b[both, 4:].view(f32)
    fin = np.isfinite(fa) & np.isfinite(fb)
    ka = a[both, 4:].astype(np.int64); kb = b[both, 4:].astype(np.int64)
    ka = np.where(ka & 0x80000000, 0x80000000 - ka, ka); kb = np.where(kb & 0x80000000, 0x80000000 - kb, kb)
    return int(np.abs(ka - kb)[fin].max()) if fin.any() else 0


FAMILIES = {"axis": axis, "surface": surface, "ties": ties, "mesh": mesh, "attributes": attributes}
_cache = {}


def family(name, oracle_mod):
    """The cases of a family, built once per process."""
    if name not in _cache:
        _cache[name] = FAMILIES[name](oracle_mod)
    return _cache[name]
