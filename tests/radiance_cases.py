"""Cases of the radiance-against-the-oracle tests (tests/test_radiance_oracle_host.py, tests/test_gpu_radiance_oracle.py): rays no
pinhole camera forms, path-traced by mrt_radiance and by the oracle's orc_radiance.  A case is one scene, one set
of rays (traced as given: no shift of the origin, no normalisation), the feature set pt_rays must run on it and the environments
under which mrt_rays_info must report it staged in LDS or read through L2.  The ray families are those of tests/rayq_cases.py
(unchanged), five scenes that reach the feature sets those leave out, and `shading`: rays aimed at what happens behind the first
hit.  Frames are 16 x 16 (nothing reads the frame), a case holds at most 5000 rays."""
import copy

import numpy as np

import rayq_cases as Q
from rayq_cases import F_ALL, F_BVH, F_ENV, F_TRI, F_VATTR, L2, LDS_ALL

f32 = np.float32
FN = F_ALL & ~F_TRI
MAX_RAYS = 5000
LDS_QUARTER = 160 * 1024 // 4           # mrt_radiance stages a level-0 scene of at most kLdsLimit / 4 bytes
# the eight feature sets of pt_rays (MRT_RAYS_LIST of csrc/mrt_rays.h), each built staged and through L2: sixteen kernels
FEATS = (FN, F_ALL, FN | F_BVH, F_ALL | F_BVH, F_ALL | F_VATTR, F_ALL | F_BVH | F_VATTR, F_ALL | F_VATTR | F_ENV, F_ALL | F_BVH | F_VATTR | F_ENV)
RANGES = ((0, 1), (7, 24))              # (sample_base, n_samples); the second is unaligned at both ends and crosses a chunk of 16
TOP_RANGE = (2 ** 32 - 1 - 40, 40)      # the last legal samples (the `shading` case, x86 only)


class Run:
    """One context of a case: the environment it is created under and what mrt_rays_info must then report."""

    def __init__(self, label, env, lds):
        self.label, self.lds = label, lds
        self.env = dict(env)
        self.env["MRT_BLOCK_THREADS"] = "256"


class RCase:
    def __init__(self, name, desc, o, d, feat, runs):
        self.name, self.desc, self.feat, self.runs = name, desc, feat, runs
        self.o, self.d = np.ascontiguousarray(o, f32), np.ascontiguousarray(d, f32)
        assert self.o.shape == self.d.shape and self.o.shape[1] == 3 and len(self.o) <= MAX_RAYS, (name, self.o.shape)


def _staged(env=LDS_ALL):
    return Run("lds", env, True)


def _over(env=LDS_ALL):
    """Asked to stage everything, and read through L2 all the same: the plan is not level 0, or the scene is over 40 KB."""
    return Run("l2 (plan)", env, False)


def _forced():
    return Run("l2 (env)", L2, False)


# ---- the families of rayq_cases ----------------------------------------------------------------------------------------------------
def _from(fam, name, oracle_mod):
    return next(c for c in Q.family(fam, oracle_mod) if c.name == name)


def _reuse(fam, name, oracle_mod, feat, runs):
    c = _from(fam, name, oracle_mod)
    desc = copy.deepcopy(c.desc)
    desc["frame"]["res"] = [16, 16]
    return RCase(f"{fam}/{name}", desc, c.o[:MAX_RAYS], c.d[:MAX_RAYS], feat, runs)


# ---- five scenes for the feature sets the ray-query families leave out ---------------------------------------------------------------
def _extra_rays(desc, seed):
    """_vertex_edge_rays on every mesh (1500) and every untransformed triangle (300), _aimed at the middle of the scene (1500),
    and the special components of 40 of them."""
    rng = np.random.default_rng(seed)
    os_, ds_ = [], []
    for r in desc["scene"]["renderer"]:
        if r["type"] == "mesh":
            o, d = Q._vertex_edge_rays(rng, r["mesh"], r.get("pos", [0, 0, 0]), 1500)
        elif r["type"] == "triangle" and "dir" not in r:
            o, d = Q._vertex_edge_rays(rng, [r["vtx"]], r["pos"], 300)
        else:
            continue
        os_.append(o); ds_.append(d)
    o, d = Q._aimed(rng, np.array([[0.0, 0.45, 0.0]]), 1500, 1.5)
    os_.append(o); ds_.append(d)
    o, d = np.concatenate(os_), np.concatenate(ds_)
    pick = rng.choice(len(o), 40, replace=False)
    so, sd = Q._special_components(rng, o[pick], d[pick])
    return np.concatenate([o, so]), np.concatenate([d, sd])


def _extra(name, desc, seed, feat, runs):
    desc = copy.deepcopy(desc)
    desc["frame"]["res"] = [16, 16]
    o, d = _extra_rays(desc, seed)
    return RCase("extra/" + name, desc, o, d, feat, runs)


def _with_sky(desc, of):
    desc = copy.deepcopy(desc)
    desc["scene"]["sky"] = copy.deepcopy(of["scene"]["sky"])
    return desc


def extra(oracle_mod=None):
    import test_oracle_ext as X
    V, B, E = F_VATTR, F_BVH, F_ENV
    return [
        _extra("triangles_crowd", X._crowd(X.triangles()), 51, F_ALL | B | V, [_staged()]),
        _extra("smooth_crowd", X.smooth(crowd=True), 52, F_ALL | B | V, [_over()]),
        _extra("triangles_env_sphere_bilinear", _with_sky(X.triangles(), X.env("sphere", "bilinear")), 53, F_ALL | V | E, [_staged()]),
        _extra("triangles_crowd_env_latlong_nearest", _with_sky(X._crowd(X.triangles()), X.env("latlong", "nearest")), 54, F_ALL | B | V | E, [_staged()]),
        _extra("env_sphere_bilinear_crowd", X.env("sphere", "bilinear", crowd=True), 55, F_ALL | B | V | E, [_over()]),
    ]


# ---- shading: what happens behind the first hit ------------------------------------------------------------------------------------
EMIT_ONE = {"type": "sphere", "r": 0.15, "pos": [-0.9, -0.5, 0.0], "mat": {"emit": 1.0, "albedo": "#ffc080"}}
CLEAR_BOX = {"type": "box", "sizes": [0.3, 0.3, 0.3], "pos": [1.0, -0.6, -0.15], "mat": {"opacity": 0.0, "glass": 0.5, "rough": 0.2}}
FLOOR_Z = -0.4
PLANE_LIGHT = {"type": "point", "pos": [0.3, -0.8, FLOOR_Z], "pwr": 0.4, "color": "#ffffff"}


def shading_desc():
    """The kitchen sink plus a sphere whose emit coin always comes up (p == 1: no draw decides it), a box whose refraction coin
    sits at the 0.85 cap (opacity 0), and a point light in the floor's plane: from a floor hit the light vector, the shadow ray
    and the floor itself lie in one plane."""
    from micro_raytracer_amd import scenes
    d = scenes.kitchen_sink(res=(16, 16), sample=1)
    d["scene"]["renderer"] += [copy.deepcopy(EMIT_ONE), copy.deepcopy(CLEAR_BOX)]
    d["scene"]["light"].append(copy.deepcopy(PLANE_LIGHT))
    return d


def sphere_instances(desc):
    """(renderer index, instance index, centre, radius) of every sphere instance."""
    out = []
    for ri, r in enumerate(desc["scene"]["renderer"]):
        if r["type"] != "sphere":
            continue
        for ii, inst in enumerate(r.get("inst") or [[r.get("pos", [0, 0, 0]), None]]):
            out.append((ri, ii, np.asarray(inst[0], np.float64), float(r["r"])))
    return out


def shading_rays(desc, seed=61):
    rng = np.random.default_rng(seed)
    os_, ds_ = [], []

    def add(o, d):
        os_.append(np.asarray(o, f32).reshape(-1, 3)); ds_.append(np.asarray(d, f32).reshape(-1, 3))

    for _, _, c, rad in sphere_instances(desc):
        # (a) grazing incidence: the line passes the centre at r (1 - 10^-u)
        m = 100
        w = Q._unit(rng.normal(size=(m, 3)))
        u = Q._unit(np.cross(w, rng.normal(size=(m, 3))))
        b = rad * (1.0 - 10.0 ** -rng.uniform(0.3, 7.0, (m, 1)))
        add(c + b * u - rng.uniform(0.5, 2.5, (m, 1)) * w, w)
        # (b) the six axis points (the poles and the seam of the spherical UV of an unrotated sphere), and origins inside
        for k in range(3):
            for sg in (-1.0, 1.0):
                pt = c.copy(); pt[k] += sg * rad
                q = pt + Q._unit(rng.normal(size=(20, 3)) + 2.0 * sg * np.eye(3)[k]) * rng.uniform(0.3, 2.0, (20, 1))
                add(q, Q._unit(pt - q))
        m = 80
        add(c + rad * 0.9 * rng.uniform(-1, 1, (m, 3)) / np.sqrt(3), Q._unit(rng.normal(size=(m, 3))))

    def to_floor(pts):
        up = rng.normal(size=pts.shape); up[:, 2] = np.abs(up[:, 2]) + 0.3
        q = pts + Q._unit(up) * rng.uniform(0.4, 2.0, (len(pts), 1))
        add(q, Q._unit(pts - q))

    # (c) floor hits on the lines x = k / 8 and y = k / 8, either sign: the plane's UV at texel boundaries
    m = 400
    p = np.stack([rng.uniform(-1.5, 1.5, m), rng.uniform(-1.5, 1.5, m), np.full(m, FLOOR_Z)], 1)
    p[np.arange(m), rng.integers(0, 2, m)] = rng.integers(-12, 13, m) / 8.0
    to_floor(p)
    # (d) floor points around the light that lies in the floor
    m = 300
    lp = np.asarray(PLANE_LIGHT["pos"], np.float64)
    r, a = 0.5 * np.sqrt(rng.uniform(0, 1, m)), rng.uniform(0, 2 * np.pi, m)
    to_floor(lp + np.stack([r * np.cos(a), r * np.sin(a), np.zeros(m)], 1))
    # (e) the two new renderers
    for tgt in (EMIT_ONE["pos"], CLEAR_BOX["pos"]):
        add(*Q._aimed(rng, np.array([tgt], np.float64), 400, 0.1))
    # (f) zero, infinite and NaN components, non-unit directions
    o, d = np.concatenate(os_), np.concatenate(ds_)
    pick = rng.choice(len(o), 30, replace=False)
    so, sd = Q._special_components(rng, o[pick], d[pick])
    return np.concatenate([o, so]), np.concatenate([d, sd])


def shading(oracle_mod=None):
    desc = shading_desc()
    o, d = shading_rays(desc)
    return [RCase("shading/kitchen_sink_plus", desc, o, d, F_ALL, [_staged()])]


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def table(oracle_mod):
    """Every case, in the order of the issue's table (FEAT ascending)."""
    B, V, E = F_BVH, F_VATTR, F_ENV
    deep = Q.mesh_variants()[2]
    cases = [
        _reuse("axis", "six_planes", oracle_mod, FN, [_staged({}), _forced()]),
        _reuse("surface", "kitchen_sink_no_triangles", oracle_mod, FN, [_staged({}), _forced()]),
        _reuse("surface", "kitchen_sink", oracle_mod, F_ALL, [_staged(), _forced()]),
        _reuse("mesh", "mesh_kind1", oracle_mod, F_ALL, [_staged()]),
        _reuse("mesh", "mesh_kind2", oracle_mod, F_ALL, [_staged()]),
        _reuse("mesh", "mesh_kind3", oracle_mod, F_ALL, [_staged()]),
        shading(oracle_mod)[0],
        # the deep-staged context reads the flat packing it keeps for the kernels without F_DEEP
        _reuse("mesh", "mesh_kind0", oracle_mod, F_ALL, [_over(), Run("l2 (deep)", {k: v for k, v in deep.env.items() if k != "MRT_BLOCK_THREADS"}, False)]),
        _reuse("mesh", "mesh_kind4", oracle_mod, F_ALL, [_over()]),
        _reuse("ties", "instance_grid", oracle_mod, FN | B, [_staged({}), _forced()]),
        _reuse("ties", "coincident_bvh", oracle_mod, F_ALL | B, [_staged(), _forced()]),
        _reuse("ties", "crowd_scene_3", oracle_mod, F_ALL | B, [_staged()]),
        _reuse("mesh", "mesh_three_rotated_instances_crowd", oracle_mod, F_ALL | B, [_staged()]),
        _reuse("attributes", "triangles", oracle_mod, F_ALL | V, [_staged(), _forced()]),
        _reuse("attributes", "smooth", oracle_mod, F_ALL | V, [_over()]),
    ]
    ex = extra(oracle_mod)
    cases += ex[:2]
    cases += [ex[2], _reuse("attributes", "env_sphere_nearest", oracle_mod, F_ALL | V | E, [_over()])]
    cases += ex[3:]
    return cases


_cache = {}


def cases(oracle_mod):
    """The table, built once per process."""
    if "table" not in _cache:
        _cache["table"] = table(oracle_mod)
    return _cache["table"]


def case(name, oracle_mod):
    return next(c for c in cases(oracle_mod) if c.name == name)


# ---- the comparison rule -------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def compare(got, ref, n_samples):
    """The rule, per ray and per component, on the sums: NaN where the reference has NaN, an infinity of the same sign where it
    has one, elsewhere |got - ref| <= 1e-4 * max(n_samples, |ref|) -- the parity bar of DESIGN.md §3 on the mean, relative for a
    ray brighter than 1 per sample.  Returns (rays that break it, the worst |got - ref| / max(n_samples, |ref|), the share of
    bit-identical rays, the count of rays with a non-finite component in the reference)."""
    got, ref = np.asarray(got, f32).reshape(-1, 3), np.asarray(ref, f32).reshape(-1, 3)
    g, r = got.astype(np.float64), ref.astype(np.float64)
    nan_ok = np.isnan(g) == np.isnan(r)
    inf_ok = (np.isinf(g) == np.isinf(r)) & (~np.isinf(r) | (np.sign(g) == np.sign(r)))
    fin = np.isfinite(g) & np.isfinite(r)
    rel = np.zeros_like(g)
    with np.errstate(invalid="ignore"):
        rel[fin] = np.abs(g[fin] - r[fin]) / np.maximum(float(n_samples), np.abs(r[fin]))
    ok = nan_ok & inf_ok & (rel <= 1e-4)
    same = (bits(got) == bits(ref)).all(axis=1)
    return np.flatnonzero(~ok.all(axis=1)), float(rel.max()) if rel.size else 0.0, float(same.mean()), int((~np.isfinite(r)).any(axis=1).sum())
