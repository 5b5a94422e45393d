"""Cases of the tests that hold pt_rays_tiles -- the kernel of mrt_radiance_adaptive -- to mrt_radiance and the
oracle: tests/test_radiance_adaptive_host.py (x86) and tests/test_gpu_radiance_adaptive_oracle.py.  One case per (FEAT, scene
staged in LDS | read through L2) pair, sixteen in all, each a run radiance_cases.table declares, with the case's rays laid out as
one 44 x 36 grid: 6 x 5 tiles of 8 x 8, the right column 4 pixels wide, the bottom row 4 pixels high, a 4 x 4 corner tile.  A
pt_rays_tiles wavefront is a tile, so the grid decides which lanes share a wave vote:

- the case's tame rays (~rayq_cases.wild) fill the grid in case order;
- in every tile with an odd index a seeded generator replaces 1 to 8 in-frame pixels with wild rays of the case (a component that
  is NaN, infinite or outside the fast-division window): wild lanes beside tame ones, and beside lanes outside the frame in the
  sliver tiles; the even tiles stay tame;
- the corner tile (29) holds a wild ray, and some tile a wild ray whose mrt_radiance sum is NaN: a tile that never converges
  (in the eleven cases whose scene can give a NaN sum at all: NO_NAN_SUM).

These placement facts are asserted where a grid is built, from the rays and the x86 build of mrt_radiance's ray body alone."""
import copy

import numpy as np

import radiance_cases as RC
import rayq_cases as Q
import rays_ref as Y
from conftest import make_holder
from rayq_cases import F_ALL, F_BVH, F_ENV, F_VATTR

f32 = np.float32
SEED = 3                                # the contexts' seed (that of tests/test_radiance_oracle_host.py)
GRID = (44, 36)                         # RES of tests/test_gpu_radiance_adaptive.py
N_TX, N_TY = (GRID[0] + 7) // 8, (GRID[1] + 7) // 8
N_TILES = N_TX * N_TY
CORNER = N_TILES - 1
MIN_SAMPLES, MAX_SAMPLES, STEP = 32, 96, 16
STOPS = (32, 64, 96)

# (FEAT, scene in LDS) -> (case of radiance_cases.table, label of the run): the table, next to its names so that collection
# renders nothing
B, V, E = F_BVH, F_VATTR, F_ENV
TABLE = [
    (RC.FN, True, "surface/kitchen_sink_no_triangles", "lds"),
    (RC.FN, False, "surface/kitchen_sink_no_triangles", "l2 (env)"),
    (F_ALL, True, "surface/kitchen_sink", "lds"),
    (F_ALL, False, "mesh/mesh_kind0", "l2 (deep)"),             # rays_kernel's aov_pk branch: the flat packing's Params
    (RC.FN | B, True, "ties/instance_grid", "lds"),
    (RC.FN | B, False, "ties/instance_grid", "l2 (env)"),
    (F_ALL | B, True, "mesh/mesh_three_rotated_instances_crowd", "lds"),
    (F_ALL | B, False, "ties/coincident_bvh", "l2 (env)"),
    (F_ALL | V, True, "attributes/triangles", "lds"),
    (F_ALL | V, False, "attributes/smooth", "l2 (plan)"),       # _over(): asked to stage, read through L2 all the same
    (F_ALL | B | V, True, "extra/triangles_crowd", "lds"),
    (F_ALL | B | V, False, "extra/smooth_crowd", "l2 (plan)"),
    (F_ALL | V | E, True, "extra/triangles_env_sphere_bilinear", "lds"),
    (F_ALL | V | E, False, "attributes/env_sphere_nearest", "l2 (plan)"),
    (F_ALL | B | V | E, True, "extra/triangles_crowd_env_latlong_nearest", "lds"),
    (F_ALL | B | V | E, False, "extra/env_sphere_bilinear_crowd", "l2 (plan)"),
]
NAMES = [f"{name} [{label}]" for _, _, name, label in TABLE]
# one grid per feature set (the x86 build has no LDS): the staged cases
FEAT_NAMES = [n for n, (_, lds, _, _) in zip(NAMES, TABLE) if lds]
# the kernels with the most registers and scratch: the launch-shape test
BIG_NAMES = [n for n, (f, _, _, _) in zip(NAMES, TABLE) if f in (F_ALL | B | V, F_ALL | B | V | E)]
# The scenes in which no ray gives a NaN sum: they have no point light, and nothing else in the path turns a non-finite ray into a
# NaN (tried on 200 tame rays of each: directions times 2^41, 1e19, 1e20, 3e38 and 1e-44, a zero direction, origins times 1e30, a
# 3e38 or infinite component in either, two infinite components).  For the kernels (FN | F_BVH, both), (F_ALL | F_BVH, L2),
# (F_ALL | F_VATTR | F_ENV, L2) and (F_ALL | F_BVH | F_VATTR | F_ENV, L2) the table of radiance_cases declares no other run, so
# their grids hold wild lanes but no NaN sum; case() asserts the list both ways.
NO_NAN_SUM = ("ties/instance_grid", "ties/coincident_bvh", "attributes/env_sphere_nearest", "extra/env_sphere_bilinear_crowd")
# The scene without noise: every sample of a ray of ties/instance_grid (the only scene of the table that runs FN | F_BVH) has the
# same value, so every tile error is exactly 0 at any count, the median threshold is 0 and the rule stops all 30 tiles at 32.
# Nothing can give its two kernels a second stop count; they are held to everything else.  case() asserts this both ways too.
NOISE_FREE = ("ties/instance_grid",)


def tile_mask(t):
    """The in-frame pixels of tile t, bool [nh][nw]."""
    m = np.zeros((GRID[1], GRID[0]), bool)
    ty, tx = divmod(t, N_TX)
    m[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = True
    return m


def tiles_mask(tiles):
    m = np.zeros((GRID[1], GRID[0]), bool)
    for t in tiles:
        m |= tile_mask(int(t))
    return m


def tile_of_pixels():
    """The tile index of every pixel, [nh][nw]."""
    y, x = np.mgrid[0:GRID[1], 0:GRID[0]]
    return (y // 8) * N_TX + x // 8


class ACase:
    """One (FEAT, staged | L2) pair: the case's scene at a 44 x 36 frame, the run's environment, the grid of rays."""

    def __init__(self, name, feat, lds, src, run):
        self.name, self.feat, self.lds, self.src, self.run = name, feat, lds, src, run
        desc = copy.deepcopy(src.desc)
        # the frame whose supersampled size (res * ssaa in float32, truncated: scene.Frame.nw) is the grid's
        ssaa = f32(desc["frame"].get("ssaa", 1.0))
        res = [next((r for r in range(1, g + 1) if int(f32(r) * ssaa) == g), None) for g in GRID]
        assert None not in res, (name, float(ssaa))
        desc["frame"]["res"] = res
        self.desc = desc
        self.o, self.d, self.wild = _grid(src)
        self._holder = None
        self._x86 = {}

    def holder(self):
        """(render, holder), one per case."""
        if self._holder is None:
            self._holder = make_holder(self.desc)
        return self._holder

    def x86(self, base, ns, segments=False):
        """Samples [base, + ns) of the grid through the x86 build of mrt_radiance's ray body, [nh][nw][3] (with segments: and the
        batch's segment total); computed once and left unchanged."""
        k = (base, ns)
        if k not in self._x86:
            probe = Y.shared_probe()
            _, holder = self.holder()
            info = Y.x86_info(probe, holder)
            assert (info["nw"], info["nh"]) == GRID and info["rays_inst"] == self.feat, (self.name, info)
            self._x86[k] = Y.x86_radiance(probe, holder, self.feat, self.o, self.d, ns, seed=SEED, sample_base=base, segments=True)
        sums, seg = self._x86[k]
        return (sums, seg) if segments else sums


HUGE = f32(2.0 ** 41)                   # a unit direction times this has a component above the fast-division window's 2^40


def wild_pool(src, rng):
    """The wild rays a grid draws from, formed from the case's own o, d: the case's wild rays as they stand (eight of the thirteen
    scenes have some), the special components (rayq_cases._special_components: an infinite or NaN component in the direction or the
    origin) of 40 of its tame rays, and 160 of its tame rays with the direction scaled by 2^41.  The last kind is what gives
    NaN sums: no ray with a NaN or infinite component does in any of these scenes (it misses everything, or its hit point lights
    nothing), a huge direction reaches the lights' falloff with an overflow."""
    wild = Q.wild(src.o, src.d)
    ti, wi = np.flatnonzero(~wild), np.flatnonzero(wild)
    pick = rng.choice(ti, 40, replace=False)
    so, sd = Q._special_components(rng, src.o[pick], src.d[pick])
    pick = rng.choice(ti, 160, replace=False)
    with np.errstate(over="ignore"):
        o = np.concatenate([src.o[wi], so, src.o[pick]]).astype(f32)
        d = np.concatenate([src.d[wi], sd, src.d[pick] * HUGE]).astype(f32)
    keep = Q.wild(o, d)
    assert keep.sum() >= 300, (src.name, int(keep.sum()))
    return o[keep], d[keep]


def _grid(src):
    """The 44 x 36 grid of a case of radiance_cases: (o, d [nh][nw][3], wild [nh][nw]), chosen from the case's o, d alone."""
    nw, nh = GRID
    ti = np.flatnonzero(~Q.wild(src.o, src.d))
    assert len(ti) >= nw * nh, (src.name, len(ti))
    o, d = (np.ascontiguousarray(a[ti[:nw * nh]].reshape(nh, nw, 3), f32) for a in (src.o, src.d))
    rng = np.random.default_rng([N_TILES, len(src.o)])
    wo, wd = wild_pool(src, rng)
    for t in range(1, N_TILES, 2):
        ys, xs = np.nonzero(tile_mask(t))
        k = int(rng.integers(1, 9))
        at = rng.choice(len(ys), k, replace=False)
        frm = rng.choice(len(wo), k, replace=False)
        o[ys[at], xs[at]], d[ys[at], xs[at]] = wo[frm], wd[frm]
    # the placement facts that the rays alone decide
    w = Q.wild(o.reshape(-1, 3), d.reshape(-1, 3)).reshape(nh, nw)
    per_tile = np.bincount(tile_of_pixels()[w], minlength=N_TILES)
    assert (per_tile[0::2] == 0).all() and ((per_tile[1::2] >= 1) & (per_tile[1::2] <= 8)).all(), (src.name, per_tile)
    assert CORNER % 2 == 1 and per_tile[CORNER] >= 1 and tile_mask(CORNER).sum() == 16
    return o, d, w


_cache = {}


def case(name, oracle_mod):
    """The case of a name of NAMES, built once per process.  Building it runs 32 samples of the grid through the x86 ray body: some
    tile holds a wild ray whose sum is NaN, unless the scene is one of NO_NAN_SUM."""
    if name not in _cache:
        feat, lds, src_name, label = TABLE[NAMES.index(name)]
        src = RC.case(src_name, oracle_mod)
        run = next(r for r in src.runs if r.label == label)
        assert src.feat == feat and run.lds == lds, (name, src.feat, run.lds)
        # the two runs of one case share its grid and its x86 sums
        twin = next((c for c in _cache.values() if c.src is src), None)
        c = ACase(name, feat, lds, src, run)
        if twin is not None:
            assert RC.bits(c.o).tobytes() == RC.bits(twin.o).tobytes()
            c._holder, c._x86 = twin.holder(), twin._x86
        nan_sum = np.isnan(c.x86(0, MIN_SAMPLES)).any(axis=-1)
        c.has_nan = bool((nan_sum & c.wild).any())
        from test_adaptive_host import np_tile_errors
        et, nan, _ = np_tile_errors(c.x86(0, MIN_SAMPLES), c.x86(0, STEP), MIN_SAMPLES, 0.0)
        c.noise_free = bool(not nan.any() and (et == 0).all())
        assert c.noise_free == (src_name in NOISE_FREE), (name, et)
        assert c.has_nan == (src_name not in NO_NAN_SUM), (name, int(nan_sum.sum()))
        _cache[name] = c
    return _cache[name]


def nan_tiles(sums):
    """bool [n_ty][n_tx]: the tiles that hold a pixel whose sum has a NaN word."""
    bad = np.isnan(sums).any(axis=-1)
    return np.bincount(tile_of_pixels()[bad], minlength=N_TILES).reshape(N_TY, N_TX) > 0


def half_fold(chunk, n):
    """The half buffer at count n of a step-16 run: the float32 fold of the 16-sample chunks of the even rounds, in order (as test 2
    of tests/test_gpu_radiance_adaptive.py forms it).  chunk: j -> samples [16 j, 16 j + 16)."""
    h = np.zeros_like(chunk[0])
    for j in range(0, n // 16, 2):
        h = h + chunk[j]
    return h


def rule_counts(whole, chunk, thr):
    """The per-tile stop counts [n_ty][n_tx] of min 32 / max 96 / step 16 at threshold thr, from the sums whole[32], whole[64] and
    the chunks 0 and 2, with the numpy rule of tests/test_adaptive_host.py at the two evaluation points below the cap."""
    from test_adaptive_host import np_tile_errors
    counts = np.full((N_TY, N_TX), MAX_SAMPLES, np.uint32)
    running = np.ones((N_TY, N_TX), bool)
    for n in STOPS[:-1]:
        _, _, conv = np_tile_errors(whole[n], half_fold(chunk, n), n, thr)
        counts[running & conv] = n
        running &= ~conv
    return counts


def median_threshold(whole32, chunk0):
    """The median of the non-NaN tile errors at 32 samples."""
    from test_adaptive_host import np_tile_errors
    et, nan, _ = np_tile_errors(whole32, chunk0, MIN_SAMPLES, 0.0)
    assert (~nan).any()
    return float(np.median(et[~nan]))
