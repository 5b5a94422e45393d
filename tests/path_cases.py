"""Scenes and comparison rules of tests/test_path_ref_host.py and tests/test_gpu_path_ref.py: small frames (48 x 27 or less, 8
samples each) whose every (pixel, sample) tests/path_ref.py answers in float64, each with the least geometry that reaches its
branch of the stochastic path ("the stochastic path").  Paths are short: float32 divergence grows with every bounce,
and faster off spheres.

Rules, the same on CPU and GPU.  A sample is compared only when every margin of its path holds core_ref's thresholds, tir >= REL
and degenerate >= 1e-3 (path_ref.sound); margins may exclude at most 25 % of a case's samples; compared samples hold the project's
parity bar, 1e-4 relative per channel or 1e-4 absolute where the channel is below 1; every branch of BRANCHES needs at least 200
compared samples over the suite.  The excluded share and the branch counts depend on path_ref in float64 and on the inputs alone."""
import functools

import numpy as np

import core_cases as K
import path_ref as P
from conftest import make_holder

f32 = np.float32
BAR = 1e-4
MAX_EXCLUDED = 0.25
MIN_BRANCH = 200
SAMPLES = 8
SEED = (0x5EED << 32) | 0x00C0FFEE        # a nonzero high word
RES = (48, 27)


def _tex(w, h, seed, lo, hi):
    """Texels k / 255 (exact in float32) drawn from [lo, hi]."""
    rng = np.random.default_rng(seed)
    return {"w": w, "h": h, "dat": [[float(f32(round(c * 255) / 255)) for c in t] for t in rng.uniform(lo, hi, (w * h, 3))]}


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
ROOM_LIGHTS = [{"type": "point", "pos": [0.2, -0.4, 1.7], "pwr": 0.8, "color": [1.0, 0.9, 0.8]},
               {"type": "dir", "dir": [-0.3, 0.5, -1.0], "pwr": 0.3, "color": [0.8, 0.9, 1.0]}]
SKY = {"color": [0.5, 0.6, 0.9], "pwr": 0.8}
# Every scene sits around the origin of the coordinates and within a few units of it: the float32 error of a hit grows with |o| +
# |pos|, and with it the share of scattered rays that leave their surface too flat to be told from rays that enter it.


def _room(mat):
    """Five planes that enclose nothing: a floor, a back wall, a left wall and two shallow ramps that rise from the floor towards +x
    and towards the camera.  Planes are infinite and the shadow query has no distance limit (src/rt.rs:1036), so inside four walls,
    or under a ceiling, no shadow ray ever escapes and no hit is ever lit; this corner is open upwards, to the right and to the front,
    and has lit and shadowed regions under both lights."""
    pl = lambda n, pos, c: {"type": "plane", "n": n, "pos": pos, "mat": dict(mat, albedo=c)}
    return [pl([0, 0, 1], [0, 0, -0.55], "#c0c0c0"), pl([-0.3, 0, 1], [0.55, 0, -0.55], "#e0e0e0"), pl([1, 0, 0], [-0.85, 0, 0], "#e06050"),
            pl([0, 0.25, 1], [0, -0.7, -0.55], "#50c060"), pl([0, -1, 0], [0, 1.0, 0], "#d0d0f0")]


def diffuse_room(bounce=2, loss=0.15):
    """Five planes and a box, dielectric, rough 0.3, a point and a directional light: the 80 % coin both ways, rand with r = rough
    and r = 1, lit and shadowed later hits.  A small room: a scattered ray starts E |cos| off its surface, and whether it leaves or
    enters is sound only while that exceeds the float32 error of the hit point, which grows with the room."""
    rend = _room({"rough": 0.3}) + [{"type": "box", "sizes": [0.36, 0.36, 0.5], "pos": [0.2, 0.3, -0.3], "dir": K.ROT_A, "mat": {"albedo": "#e0c060", "rough": 0.3}}]
    return {"rt": {"bounce": bounce, "sample": SAMPLES, "loss": loss},
            "frame": {"res": list(RES), "ssaa": 1, "cam": {"pos": [-0.05, -1.35, 0.1], "dir": [0, 0.08, 1, -0.1], "aprt": 0, "fov": 70}},
            "scene": {"renderer": rend, "light": [dict(ROOM_LIGHTS[0], pos=[0.1, -0.25, 1.0]), ROOM_LIGHTS[1]], "sky": SKY}}


def rough_metal():
    """metal = 1 with rough 0.2 (sphere) and 0.6 (floor): no diffuse coin is drawn, and its slot is skipped, not shifted."""
    rend = [{"type": "plane", "n": [0, 0, 1], "pos": [0, 0, -0.8], "mat": {"albedo": "#d0c0b0", "rough": 0.6, "metal": 1}},
            {"type": "sphere", "r": 0.9, "pos": [0.2, 0.4, 0.1], "mat": {"albedo": "#e0e0ff", "rough": 0.2, "metal": 1}},
            {"type": "plane", "n": [0, -1, 0], "pos": [0, 2.0, 0], "mat": {"albedo": "#80c0ff", "rough": 1.0}}]
    return {"rt": {"bounce": 2, "sample": SAMPLES, "loss": 0.15},
            "frame": {"res": list(RES), "ssaa": 1, "cam": {"pos": [0, -2.8, 0.9], "dir": [0, 0, 1, -0.3], "aprt": 0, "fov": 55}},
            "scene": {"renderer": rend, "light": ROOM_LIGHTS, "sky": SKY}}


def glass():
    """Spheres and boxes with opacity 0 and 0.4 and glass 0, 0.6 and 1 in front of a textured wall: the transmission coin at both
    its caps (0.85 and 1 - 0.4), the exit-hit rule, opacity == 0 switching the diffuse coin off, refractions that fail (glass 1:
    eta = 1.5 makes k < 0 common on the way out)."""
    g = lambda c, op, gl, rough: {"albedo": c, "rough": rough, "opacity": op, "glass": gl}
    rend = [{"type": "plane", "n": [0, -1, 0], "pos": [0, 1.9, 0], "mat": {"albedo": "#ffffff", "rough": 1.0, "tex": _tex(6, 4, 21, 0.2, 1.0)}},
            {"type": "plane", "n": [0, 0, 1], "pos": [0, 0, -0.9], "mat": {"albedo": "#b0b0b0", "rough": 1.0}},
            {"type": "sphere", "r": 0.7, "pos": [-1.3, 0.0, -0.1], "mat": g("#ffd0d0", 0.0, 0.6, 0.05)},
            {"type": "sphere", "r": 0.5, "pos": [-0.1, 0.3, 0.75], "mat": g("#d0ffd0", 0.4, 1.0, 0.1)},
            {"type": "box", "sizes": [1.1, 0.8, 1.1], "pos": [0.7, 0.0, -0.3], "dir": K.ROT_B, "mat": g("#d0d0ff", 0.0, 1.0, 0.05)},
            {"type": "box", "sizes": [0.7, 0.6, 0.7], "pos": [1.6, 0.6, 0.8], "mat": g("#ffffd0", 0.4, 0.0, 0.1)}]
    return {"rt": {"bounce": 3, "sample": SAMPLES, "loss": 0.15},
            "frame": {"res": list(RES), "ssaa": 1, "cam": {"pos": [0.1, -3.0, 0.3], "dir": [0, 0, 1, 0], "aprt": 0, "fov": 60}},
            "scene": {"renderer": rend, "light": ROOM_LIGHTS[:1], "sky": SKY}}


def omap_emap():
    """A plane and a sphere whose omap, emap, gmap and rmap texels take several values strictly between 0 and 1: per-hit coin
    probabilities from texels, read at the exit hit's UV after a refraction."""
    maps = lambda s: {"omap": _tex(4, 3, s, 0.25, 0.9), "emap": _tex(3, 2, s + 1, 0.1, 0.6), "gmap": _tex(2, 2, s + 2, 0.1, 0.9), "rmap": _tex(3, 3, s + 3, 0.1, 0.6)}
    rend = [{"type": "plane", "n": [0, 0, 1], "pos": [0.2, 0.1, -0.7], "mat": dict({"albedo": "#e0d0c0"}, **maps(31))},
            {"type": "sphere", "r": 0.8, "pos": [0.1, 0.3, 0.2], "dir": K.ROT_A, "mat": dict({"albedo": "#c0e0ff", "tex": _tex(8, 4, 30, 0.3, 1.0)}, **maps(41))},
            {"type": "plane", "n": [0, -1, 0], "pos": [0, 2.1, 0], "mat": {"albedo": "#ffffff", "rough": 1.0, "tex": _tex(5, 4, 22, 0.2, 1.0)}}]
    return {"rt": {"bounce": 2, "sample": SAMPLES, "loss": 0.15},
            "frame": {"res": list(RES), "ssaa": 1, "cam": {"pos": [0, -3.0, 0.9], "dir": [0, 0, 1, -0.3], "aprt": 0, "fov": 55}},
            "scene": {"renderer": rend, "light": ROOM_LIGHTS[:1], "sky": SKY}}


def emit_partial():
    """emit 0.25 and 0.75: the emit coin of the fold on material scalars strictly between 0 and 1, on first and later items."""
    rend = [{"type": "plane", "n": [0, 0, 1], "pos": [0, 0, -0.8], "mat": {"albedo": "#c0d0c0", "rough": 0.5, "emit": 0.25}},
            {"type": "box", "sizes": [1.2, 0.8, 1.0], "pos": [0.3, 0.3, -0.1], "dir": K.ROT_A, "mat": {"albedo": "#ffc080", "rough": 0.4, "emit": 0.75}},
            {"type": "plane", "n": [0, -1, 0], "pos": [0, 2.1, 0], "mat": {"albedo": "#a0a0ff", "rough": 1.0}}]
    return {"rt": {"bounce": 1, "sample": SAMPLES, "loss": 0.15},
            "frame": {"res": list(RES), "ssaa": 1, "cam": {"pos": [0, -3.0, 0.8], "dir": [0, 0, 1, -0.3], "aprt": 0, "fov": 55}},
            "scene": {"renderer": rend, "light": ROOM_LIGHTS, "sky": SKY}}


def lens(aprt, bounce):
    """A textured floor and three spheres at three depths under a point light, seen from above through a thin lens by a rolled camera
    at ssaa 1.5 (32 x 18 -> 48 x 27): the two lens draws, the ray leaving the lens point."""
    rend = [{"type": "plane", "n": [0, 0, 1], "pos": [0.3, 0.2, -0.6], "mat": {"albedo": "#ffffff", "rough": 0.9, "tex": _tex(4, 4, 51, 0.3, 1.0)}},
            {"type": "sphere", "r": 0.4, "pos": [-0.9, -0.8, -0.2], "mat": {"albedo": "#ff8060", "rough": 0.7}},
            {"type": "sphere", "r": 0.5, "pos": [0.1, 0.4, -0.1], "mat": {"albedo": "#60ff80", "rough": 0.7}},
            {"type": "sphere", "r": 0.6, "pos": [1.2, 1.8, 0.0], "mat": {"albedo": "#6080ff", "rough": 0.7}}]
    return {"rt": {"bounce": bounce, "sample": SAMPLES, "loss": 0.15},
            "frame": {"res": [32, 18], "ssaa": 1.5, "cam": {"pos": [0, -2.6, 1.6], "dir": [0.2, 0.1, 1, -0.6], "aprt": aprt, "foc": 3.4, "fov": 55}},
            "scene": {"renderer": rend, "light": [{"type": "point", "pos": [-0.5, -0.5, 2.0], "pwr": 0.8, "color": [1.0, 0.9, 0.8]}], "sky": SKY}}


CASES = {"diffuse_room": diffuse_room, "rough_metal": rough_metal, "glass": glass, "omap_emap": omap_emap, "emit_partial": emit_partial,
         "lens/aprt0.05_b1": lambda: lens(0.05, 1), "lens/aprt0.5_b0": lambda: lens(0.5, 0),
         "loss/0.15_b3": lambda: diffuse_room(3, 0.15), "loss/1.5_b3": lambda: diffuse_room(3, 1.5)}
PINHOLE = [n for n in CASES if not n.startswith("lens")]


@functools.lru_cache(maxsize=None)
def case(name):
    """A dict, computed once, shared and left unchanged: render, holder, shape (nh, nw), pixel and sample [n] (every pixel at
    samples 0 .. SAMPLES - 1, sample-major), the primary rays o, d in float64, ref (path_ref.trace_sample in float64), rgb32 (the
    same in float32, from float32 primary rays), keep (path_ref.sound of the float64 margins)."""
    render, holder = make_holder(CASES[name]())
    nh, nw = P.frame_shape(render)
    assert nh * nw <= 48 * 27
    pixel = np.tile(np.arange(nh * nw, dtype=np.uint32), SAMPLES)
    sample = np.repeat(np.arange(SAMPLES, dtype=np.uint32), nh * nw)
    o, d = P.camera_paths(render, SEED, pixel, sample, np.float64)
    ref = P.trace_sample(render, SEED, pixel, sample, o, d, np.float64)
    o32, d32 = P.camera_paths(render, SEED, pixel, sample, np.float32)
    rgb32 = P.trace_sample(render, SEED, pixel, sample, o32, d32, np.float32)["rgb"]
    return {"name": name, "render": render, "holder": holder, "shape": (nh, nw), "pixel": pixel, "sample": sample, "o": o, "d": d, "ref": ref,
            "rgb32": rgb32, "keep": P.sound(ref["margins"])}


# ---- rules -------------------------------------------------------------------------------------------------------------------------
def compare(label, c, got):
    """got [SAMPLES][nh][nw][3] (or [n][3] in the case's order) against the float64 samples.  Prints the figures, then asserts."""
    want = c["ref"]["rgb"]
    got = np.asarray(got, np.float64).reshape(want.shape)
    keep = c["keep"]
    bar = BAR * np.maximum(np.abs(want), 1.0)
    err = np.abs(got - want) / bar
    err32 = np.abs(c["rgb32"].astype(np.float64) - want) / bar
    n = keep.size
    worst, worst32 = float(err[keep].max()) * BAR, float(err32[keep].max()) * BAR
    print(f"path_ref {label} {c['name']}: {n} samples, excluded {int((~keep).sum())} ({(~keep).mean():.1%}), compared {int(keep.sum())}; worst error "
          f"{worst:.2e} of max(|want|, 1) (bar {BAR:.0e}), float32 numpy {worst32:.2e}")
    assert (~keep).sum() <= MAX_EXCLUDED * n, (c["name"], int((~keep).sum()), n)
    bad = np.flatnonzero(((err > 1) | ~np.isfinite(got)).any(1) & keep)
    assert bad.size == 0, (label, c["name"], len(bad), [(int(c["pixel"][i]), int(c["sample"][i]), got[i].tolist(), want[i].tolist()) for i in bad[:4]])
    return worst, worst32


BRANCHES = ["80 % coin fires (rand with r = 1)", "80 % coin drawn, does not fire (rand with r = rough)", "metal: no diffuse coin", "opacity 0: no diffuse coin",
            "later hit lit", "later hit shadowed", "transmission coin at the 0.85 cap fires", "transmission coin at the 0.85 cap does not fire",
            "transmission coin below the cap fires", "transmission coin below the cap does not fire", "refraction taken: the exit hit is shaded",
            "refraction failed (k < 0): the reflection stays", "refraction's own 80 % coin fires", "refraction's own 80 % coin drawn, does not fire",
            "transmission probability from an omap texel, fires", "emit probability from an emap texel, fires", "emit probability from an emap texel, does not fire",
            "exit hit's UV on a mapped surface", "emit scalar in (0, 1) fires", "emit scalar in (0, 1) does not fire", "emit coin fires on a later item",
            "lens, bounce 0", "lens, bounce 1", "three items", "four items", "loss < 1, two or more items", "loss >= 1, two or more items"]


def branches(c):
    """Compared samples per branch of BRANCHES that the case reaches, from the float64 answer alone."""
    ref, keep, render = c["ref"], c["keep"], c["render"]
    out = dict.fromkeys(BRANCHES, 0)

    def add(key, mask):
        out[key] += int((mask & keep).sum())

    cap = float(f32(0.85))
    for b, br in enumerate(ref["branches"]):
        add(BRANCHES[0], br["diffuse"])
        add(BRANCHES[1], br["diffuse_drawn"] & ~br["diffuse"] & (br["rough"] > 0) & (br["rough"] < 1))
        add(BRANCHES[2], br["metal_skip"])
        add(BRANCHES[3], br["opaque0"])
        if b >= 1:
            add(BRANCHES[4], np.any(br["lit"], 0))
            add(BRANCHES[5], np.any(br["shadowed"], 0))
            add("emit coin fires on a later item", br["emit_fired"])
        at_cap, below = br["hit"] & (br["p_transmit"] == cap), br["hit"] & (br["p_transmit"] > 0) & (br["p_transmit"] < cap)
        add(BRANCHES[6], at_cap & br["transmit"]); add(BRANCHES[7], at_cap & ~br["transmit"])
        add(BRANCHES[8], below & br["transmit"]); add(BRANCHES[9], below & ~br["transmit"])
        add(BRANCHES[10], br["refracted"]); add(BRANCHES[11], br["failed"])
        add(BRANCHES[12], br["refr_diffuse"]); add(BRANCHES[13], br["refr_diffuse_drawn"] & ~br["refr_diffuse"])
        frac = (br["emit_p"] > 0) & (br["emit_p"] < 1)
        add(BRANCHES[14], br["mapped"] & below & br["transmit"])
        add(BRANCHES[15], br["mapped"] & frac & br["emit_fired"]); add(BRANCHES[16], br["mapped"] & frac & br["hit"] & ~br["emit_fired"])
        add(BRANCHES[17], br["mapped"] & br["refracted"])
        add(BRANCHES[18], ~br["mapped"] & frac & br["emit_fired"]); add(BRANCHES[19], ~br["mapped"] & frac & br["hit"] & ~br["emit_fired"])
    if render.frame.cam.aprt != 0:
        add(f"lens, bounce {render.rt.bounce}", np.ones(keep.size, bool))
    add("three items", ref["depth"] == 3); add("four items", ref["depth"] == 4)
    add("loss < 1, two or more items" if render.rt.loss < 1 else "loss >= 1, two or more items", ref["depth"] >= 2)
    return out


def print_branches(title, total):
    for key in BRANCHES:
        print(f"path_ref coverage, {title}: {key:62s} {total.get(key, 0):6d}")
    short = {k: total.get(k, 0) for k in BRANCHES if total.get(k, 0) < MIN_BRANCH}
    assert short == {}, (title, short)


def total_branches(tables):
    total = dict.fromkeys(BRANCHES, 0)
    for t in tables:
        for k, v in t.items():
            total[k] += v
    return total


# ---- coin frequencies against closed forms ---------------------------------------------------------------------------------------------
# Three scenes of 32 x 32 pixels under a uniform sky, in which one sample of a pixel takes one of two values a threshold tells
# apart, 4096 samples per pixel.  n = 1024 x 4096 = 4 194 304 coins of probability p per scene.
FREQ_RES, FREQ_SAMPLES, FREQ_SEED = (32, 32), 4096, 7
_SKY = {"color": [0.5, 0.6, 0.9], "pwr": 0.8}
_FCAM = {"pos": [0, -2.0, 0.0], "dir": [0, 0, 1, 0], "aprt": 0, "fov": 30}


def _freq(rend, bounce, light=()):
    return {"rt": {"bounce": bounce, "sample": 1, "loss": 0.15}, "frame": {"res": list(FREQ_RES), "ssaa": 1, "cam": dict(_FCAM)},
            "scene": {"renderer": rend, "light": list(light), "sky": dict(_SKY)}}


def freq_scenes():
    """name -> (description, p, which side of `split` the coin's heads fall on (+1: above), channel, split, (value of heads, of tails)).

    emit: a wall of emit 0.3 and colour (1, 0, 0) fills the frame, bounce 0, no light.  Heads (p = f32(0.3) widened): the colour,
      red 1.  Tails: 0.5 col + colour (x) col with col = sky.color sky.pwr, red 1.5 * 0.4 = 0.6.  Split at 0.8.
    transmit: a wall-sized box of opacity 0.5, glass 0 (eta = 1: k = cos^2 >= 0, no refraction fails), rough 1, colour (1, 1, 1),
      lit from the camera's side by a directional light along +y, bounce 0.  Tails: hit.0, whose normal -y faces the light: 1.5 col +
      diff * pwr with diff = 1, red 0.6 + 0.9.  Heads (p = min(1 - 0.5, 0.85) = 0.5): hit.1, normal +y, diff = 0
      and spec * (1 - rough) = 0: red 0.6.  Split at 0.8.
    diffuse: a wall of metal 0, rough 0 faces the camera, an emit-1 plane of colour (0, 0, 0) stands behind the camera, bounce 1 (at
      bounce 0 the reflected ray is cast and never traced, src/rt.rs:1018: no radiance depends on the 80 % coin there).  Tails: rand(n, 0)
      = n, the mirror direction comes back and meets the emitter: col = 0, red 0.  Heads: r = 1; with cos th = 1 - 2 u1 uniform, n' =
      (n + v).norm() has half the polar angle of v, so dir.reflect(n') is v's rotation: uniform on the sphere whatever dir is.  It
      points behind the wall, where nothing is, with probability 1/2: red 1.5 * 0.4 = 0.6.  p = floor(0.8 2^32) / 2^32 / 2 = 0.4 (the
      lattice of u1 moves it by < 2^-23).  Split at 0.3."""
    wall = lambda mat: [{"type": "box", "sizes": [8.0, 1.0, 8.0], "pos": [0, 3.0, 0], "mat": mat}]
    p_emit = float(f32(0.3))
    p_diff = float(np.floor(0.8 * 2.0 ** 32) / 2.0 ** 32) * 0.5
    mirror = [{"type": "plane", "n": [0, -1, 0], "pos": [0, 3.0, 0], "mat": {"albedo": "#ffffff", "rough": 0, "metal": 0}},
              {"type": "plane", "n": [0, 1, 0], "pos": [0, -4.0, 0], "mat": {"albedo": "#000000", "rough": 1, "emit": 1}}]
    return {"emit": (_freq(wall({"albedo": "#ff0000", "rough": 1, "emit": 0.3}), 0), p_emit, +1, 0, 0.8, (1.0, 0.6)),
            "transmit": (_freq(wall({"albedo": "#ffffff", "rough": 1, "opacity": 0.5, "glass": 0}), 0, [{"type": "dir", "dir": [0, 1, 0], "pwr": 0.9, "color": [1, 1, 1]}]), 0.5, -1, 0, 0.8, (0.6, 1.5)),
            "diffuse": (_freq(mirror, 1), p_diff, +1, 0, 0.3, (0.6, 0.0))}


def freq_check(label, heads, p):
    """heads: bool [samples][pixels].  With n = pixels * samples coins of probability p, q = 1 - p:
      total: the count is binomial(n, p), sigma = sqrt(n p q) (n = 4 194 304, p = 0.5: 1024; p = 0.3: 938.5; p = 0.4: 1003.3);
      per pixel: c_i ~ binomial(m, p), m = samples; X = sum_i (c_i - m p)^2 / (m p q) has mean k = pixels and variance
        2 k + (1 - 6 p q) k / (m p q) (the binomial's fourth moment; the second term is below 0.2 here), so sigma = sqrt(2 k) = 45.3
        at k = 1024: |X - 1024| <= 5 sigma = 226.3; keys that collide across pixels make counts equal or the sum too wide;
      lag 1 over the sample index: r = sum over pixels and s of (x_s - p)(x_s+1 - p) / (N p q), N = k (m - 1) pairs; independent
        coins give mean 0 and variance 1 / N (each term has variance (p q)^2, the terms are uncorrelated), sigma = 1 / sqrt(N) =
        4.88e-4 at N = 1024 * 4095: |r| <= 5 sigma = 2.44e-3."""
    m, k = heads.shape
    n, q = m * k, 1.0 - p
    total = int(heads.sum())
    z_total = (total - n * p) / np.sqrt(n * p * q)
    c = heads.sum(0).astype(np.float64)
    chi = float(((c - m * p) ** 2).sum() / (m * p * q))
    z_chi = (chi - k) / np.sqrt(2.0 * k)
    x = heads.astype(np.float64) - p
    pairs = k * (m - 1)
    r = float((x[:-1] * x[1:]).sum() / (pairs * p * q))
    z_r = r * np.sqrt(pairs)
    print(f"path_ref coin frequencies {label}: p {p:.6f}, n {n}; heads {total} ({z_total:+.2f} sigma); chi-square over {k} pixels {chi:.1f} ({z_chi:+.2f} sigma); "
          f"lag-1 autocorrelation {r:+.2e} ({z_r:+.2f} sigma); bar 5 sigma each")
    assert abs(z_total) <= 5 and abs(z_chi) <= 5 and abs(z_r) <= 5, (label, z_total, z_chi, z_r)
    return z_total, z_chi, z_r
