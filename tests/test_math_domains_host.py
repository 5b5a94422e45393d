"""sincos_, acos_, atan2_ and the expressions built on them over their whole domains, without a GPU: the x86
build of csrc/mrt_math.h against the oracle bit for bit on every family of tests/math_cases.py, the oracle against numpy float64
(the accuracy figures of section 4's table are asserted here), the invariants the texture lookups rest on, and the signed-zero
table of divergence D2.  The GPU side of the same families is tests/test_gpu_math_domains.py.

One pass over the families (the `survey` fixture) feeds every test of this file: each family is generated, run and reduced once."""
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import math_cases as mc

f32 = np.float32
HOST_CHUNK = 1 << 24          # float64 temporaries of a chunk stay at 128 MiB
WORKERS = min(16, os.cpu_count() or 1)

# Worst error of the oracle against numpy float64 over families 1-9, as measured (the `survey` prints them), rounded up to the
# next 0.25 ulp resp. 1e-8: the functions are deterministic, the margin only absorbs another choice of random mantissas.
#   sin 9.03e-8 (sincos_wide), cos 9.25e-8 (sincos_lattice) absolute; acos 1.282 ulp (acos_dense); atan2 3.091 ulp (atan2_exponents)
BAR = {"sin": 1.0e-7, "cos": 1.0e-7, "acos": 1.5, "atan2": 3.25}
TEXEL_WIDTHS = (2, 7, 64, 4096)


def _split(n, parts):
    b = np.linspace(0, n, parts + 1).astype(np.int64)
    return [(int(b[i]), int(b[i + 1])) for i in range(parts) if b[i + 1] > b[i]]


def _par(pool, fn, n):
    """fn(lo, hi) over WORKERS slices of range(n) (ctypes and numpy's loops release the GIL)."""
    return list(pool.map(lambda r: fn(*r), _split(n, WORKERS)))


def _math(pool, mod, op, a, b):
    out = np.empty_like(a)

    def part(lo, hi):
        out[lo:hi] = mod.math(op, a[lo:hi], None if b is None else b[lo:hi])
    _par(pool, part, a.size)
    return out


def _ulps(got, ref64):
    """|got - ref| in ulp of the correctly rounded f32 result."""
    with np.errstate(all="ignore"):
        r32 = ref64.astype(f32)
        return np.abs(got.astype(np.float64) - ref64) / np.spacing(np.abs(r32)).astype(np.float64)


def _err64(op, got, a, b):
    """Per-element error of the oracle's result against numpy float64 on the float64 values of the f32 inputs: absolute for
    sin / cos (op 0, 1; their results pass through zero), ulp for acos and atan2; NaN where the function is not defined (|x| beyond
    65536 resp. 1, a NaN operand).  atan2's reference takes +-0 as the same input, as the contract does (section 6, D2)."""
    x = a.astype(np.float64)
    with np.errstate(all="ignore"):
        if op in (0, 1):
            e = np.abs(got.astype(np.float64) - (np.sin(x) if op == 0 else np.cos(x)))
            return np.where(np.abs(x) <= 65536.0, e, np.nan)
        if op == 2:
            return np.where(np.abs(x) <= 1.0, _ulps(got, np.arccos(x)), np.nan)
        y = b.astype(np.float64)
        return _ulps(got, np.arctan2(x + 0.0, y + 0.0))


FUNC = {0: "sin", 1: "cos", 2: "acos", 3: "atan2"}


def _worst(pool, op, got, a, b):
    def part(lo, hi):
        e = _err64(op, got[lo:hi], a[lo:hi], None if b is None else b[lo:hi])
        if np.isnan(e).all():
            return (-1.0, 0)
        k = int(np.nanargmax(e))
        return (float(e[k]), lo + k)
    return max(_par(pool, part, a.size))


@pytest.fixture(scope="module")
def survey(oracle_mod, emu_mod):
    """name -> dict(n, mismatches, example, seconds, worst {function: (error, a, b)}, ...) over every family of math_cases.CHECKS."""
    out = {}
    with ThreadPoolExecutor(max_workers=WORKERS) as pool:
        for name, (ops, gen) in mc.CHECKS.items():
            t0 = time.perf_counter()
            st = out[name] = dict(n=0, mismatches=0, example=None, worst={}, results={}, mono_violations=0, outside=0, not_nan=0)
            last = {}
            for c in gen(HOST_CHUNK):
                st["n"] += c.a.size
                for op in ops:
                    o = _math(pool, oracle_mod, op, c.a, c.b)
                    g = _math(pool, emu_mod, op, c.a, c.b)
                    bad = ~mc.same_bits(g, o)
                    if bad.any():
                        st["mismatches"] += int(np.count_nonzero(bad))
                        k = int(np.flatnonzero(bad)[0])
                        st["example"] = st["example"] or (c.name, op, c.a[k], None if c.b is None else c.b[k], g[k], o[k])
                    if op in FUNC and not name.startswith("lane_orders"):
                        e, k = _worst(pool, op, o, c.a, c.b)
                        if e > st["worst"].get(FUNC[op], (-1.0,))[0]:
                            st["worst"][FUNC[op]] = (e, float(c.a[k]), None if c.b is None else float(c.b[k]))
                        with np.errstate(invalid="ignore"):
                            undefined = ~(np.abs(c.a) <= (65536.0 if op < 2 else 1.0)) if op < 3 else (np.isnan(c.a) | np.isnan(c.b))
                        st["not_nan"] += int(np.count_nonzero(undefined & ~np.isnan(o)))
                    if name == "acos_dense":
                        # pattern order: x grows for the positive half (acos must not grow), falls for the negative half (must not fall)
                        for tag, r in (("oracle", o), ("x86", g)):
                            key = (tag, c.first >> 31)
                            d = np.diff(r.astype(np.float64), prepend=last.get(key, float(r[0])))
                            st["mono_violations"] += int(np.count_nonzero(d > 0 if c.first >> 31 == 0 else d < 0))
                            last[key] = float(r[-1])
                    if op in (16, 17):
                        for r in (o, g):
                            with np.errstate(invalid="ignore"):
                                st["outside"] += int(np.count_nonzero(~np.isnan(r) & ~((r >= 0.0) & (r <= 1.0))))
                            if op == 16:
                                st["not_nan"] += int(np.count_nonzero(np.isnan(r) & ~(np.isnan(c.a) | np.isnan(c.b))))
                            else:
                                st["not_nan"] += int(np.count_nonzero(np.isnan(r)))         # the clamp is maxNum / minNum: NaN -> -1
                    if name in ("sincos_lattice", "lane_orders_atan2", "lane_orders_acos", "unit_components", "uv_longitude") or c.a.size <= 4096:
                        st["results"][(c.name, op)] = (c, o, g)
            st["seconds"] = time.perf_counter() - t0
            w = ", ".join(f"{k} {v[0]:.4g} at {v[1]!r}" + ("" if v[2] is None else f", {v[2]!r}") for k, v in st["worst"].items())
            print(f"{name}: ops {ops}, {st['n']} inputs, x86 mismatches {st['mismatches']}, {st['seconds']:.1f} s" + (f"; worst vs float64: {w}" if w else ""))
    return out


@pytest.mark.parametrize("name", list(mc.CHECKS))
def test_x86_build_equals_the_oracle_bit_for_bit(name, survey):
    """emu_math (csrc/mrt_math.h compiled for x86) == orc_math on every input of the family and every op it is run through; a NaN
    equals any NaN, nothing is excluded."""
    st = survey[name]
    assert st["n"] > 0
    assert st["mismatches"] == 0, f"{name}: {st['mismatches']} results differ over {st['n']} inputs x {len(mc.CHECKS[name][0])} ops, first (chunk, op, a, b, x86, oracle) = {st['example']}"


def _worst_over(survey, fn):
    return max((st["worst"][fn] for st in survey.values() if fn in st["worst"]), key=lambda v: v[0])


@pytest.mark.parametrize("fn", ["sin", "cos", "acos", "atan2"])
def test_oracle_accuracy_against_float64(fn, survey):
    """The worst error over families 1-9 against np.sin / np.cos / np.arccos / np.arctan2 in float64 stays at the figure DESIGN.md
    section 4 states (BAR); outside its domain every function gives NaN."""
    e, a, b = _worst_over(survey, fn)
    print(f"{fn}: worst {e:.4g} {'absolute' if fn in ('sin', 'cos') else 'ulp'} at a={a!r} b={b!r}; bar {BAR[fn]}")
    assert e <= BAR[fn], (fn, e, a, b)
    assert sum(st["not_nan"] for st in survey.values()) == 0


def test_lookup_coordinates_stay_inside_the_unit_interval(survey, oracle_mod, emu_mod):
    """Op 16 (hit_uv / env_uv's u) lies in [0, 1] for every pair of families 8 and 9 without a NaN operand (and is NaN only with one);
    op 17 (env_uv's latlong v) lies in [0, 1] for every input, NaN included, and is exactly 0 at +1 and 1 at -1: the poles."""
    for name in ("uv_longitude", "uv_latitude"):
        assert survey[name]["outside"] == 0 and survey[name]["not_nan"] == 0, (name, survey[name])
    for mod in (oracle_mod, emu_mod):
        v = mod.math(17, np.array([1.0, -1.0, 1.5, -np.inf, np.inf], f32))
        assert list(v.view(np.uint32)) == list(np.array([0.0, 1.0, 0.0, 1.0, 0.0], f32).view(np.uint32))


def test_sin_cos_of_the_lattice_have_unit_length(survey):
    """sin^2 + cos^2 - 1 in float64 over all 2^23 phi of the path tracer, within the bound test_contract_v3_polar_angle uses."""
    for which in (1, 2):
        s = survey["sincos_lattice"]["results"][("sincos_lattice", 0)][which].astype(np.float64)
        c = survey["sincos_lattice"]["results"][("sincos_lattice", 1)][which].astype(np.float64)
        d = np.abs(s * s + c * c - 1.0).max()
        print(f"sin^2 + cos^2 - 1 over the lattice: {d:.3e}")
        assert d <= 2e-7


def test_acos_is_monotone_over_every_pattern(survey):
    """acos never grows with x over all patterns of 2^-13 <= |x| <= 1, on the oracle and on the x86 build."""
    assert survey["acos_dense"]["n"] == 2 * (13 * (1 << 23) + 1)
    assert survey["acos_dense"]["mono_violations"] == 0


def test_signed_zeros_of_atan2_are_pinned(oracle_mod, emu_mod):
    """The contract takes +0 and -0 as one input: atan2_(y, x) on {+-0, +-1}^2, with libm's value (the
    reference's f32::atan2) where it differs:

        y \\ x     +0       -0            +1          -1
        +0         0        0 (libm pi)   0           pi
        -0         0 (-0)   0 (libm -pi)  0 (-0)      pi (libm -pi)
        +1         pi/2     pi/2          pi/4        pi - pi/4
        -1        -pi/2    -pi/2         -pi/4       -(pi - pi/4)

    Every zero result is +0.  At (+-0, -1) -- a sphere's v = (+-0, 1, z), a sky direction (+-0, 1, z) -- u is 1.0 where the
    reference has 1.0 for +0 and 0.0 for -0: the last texel column instead of the first under D4's clamp."""
    p, h, q = mc.kPi, f32(1.57079637050628662), f32(0.785398185253143311)
    z = f32(0.0)
    n0 = -0.0
    table = [(0.0, 0.0, z), (0.0, n0, z), (0.0, 1.0, z), (0.0, -1.0, p),
             (n0, 0.0, z), (n0, n0, z), (n0, 1.0, z), (n0, -1.0, p),
             (1.0, 0.0, h), (1.0, n0, h), (1.0, 1.0, q), (1.0, -1.0, p - q),
             (-1.0, 0.0, -h), (-1.0, n0, -h), (-1.0, 1.0, -q), (-1.0, -1.0, -(p - q))]
    y = np.array([k[0] for k in table], f32)
    x = np.array([k[1] for k in table], f32)
    want = np.array([k[2] for k in table], f32)
    for mod in (oracle_mod, emu_mod):
        got = mod.math(3, y, x)
        assert list(got.view(np.uint32)) == list(want.view(np.uint32)), (got, want)
        # op 16 negates its second operand itself: (a, b) = (+-0, 1) is atan2_(+-0, -1)
        u = mod.math(16, np.array([0.0, -0.0], f32), np.array([1.0, 1.0], f32))
        assert list(u) == [1.0, 1.0]
    with np.errstate(all="ignore"):
        libm = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    differs = [i for i, (w, l) in enumerate(zip(want, libm)) if not (abs(float(w) - l) < 1e-6 and np.signbit(w) == np.signbit(l))]
    assert differs == [1, 4, 5, 6, 7]          # (+0, -0) and the whole row of y = -0: the entries the docstring marks


def test_texel_flips_of_the_sphere_u_are_counted(survey):
    """How many of family 9's inputs land in another texel column than the float64 u would give, to_index(u w) for w in
    TEXEL_WIDTHS (DESIGN.md section 4 carries the counts).  The float64 u takes +-0 as the contract does; the inputs whose u the
    sign of a zero moves are counted apart.  A figure, not a bound: only the bookkeeping is asserted."""
    c, o, g = survey["uv_longitude"]["results"][("uv_longitude:unit", 16)]
    a, b = c.a.astype(np.float64), c.b.astype(np.float64)
    u64 = 0.5 + 0.5 * np.arctan2(a + 0.0, -b + 0.0) / np.pi
    u64_libm = 0.5 + 0.5 * np.arctan2(a, -b) / np.pi
    for w in TEXEL_WIDTHS:
        idx = np.minimum((o * f32(w)).astype(np.int64), w - 1)
        i64 = np.minimum((u64 * w).astype(np.int64), w - 1)
        i64l = np.minimum((u64_libm * w).astype(np.int64), w - 1)
        print(f"w = {w}: {np.count_nonzero(idx != i64)} of {o.size} inputs in another column than float64, "
              f"{np.count_nonzero(i64 != i64l)} more moved by the sign of a zero")
        assert 0 <= idx.min() and idx.max() <= w - 1
    assert np.array_equal(o.view(np.uint32), g.view(np.uint32))


def test_lane_orders_hold_the_same_values(survey):
    """Family 10 on the x86 build and the oracle: every value's result is the same word in every layout (on a CPU trivially so; the
    GPU test asserts the same thing of the device, this one that the bookkeeping the comparison rests on is right)."""
    for fam, pools in (("lane_orders_atan2", mc.lane_pools_atan2()), ("lane_orders_acos", mc.lane_pools_acos())):
        op = mc.CHECKS[fam][0][0]
        seen = np.full(2 * mc.POOL, -1, np.int64)          # the first word met for each value of the two pools
        for lname, idx in mc.lane_layouts().items():
            c, o, g = survey[fam]["results"][(f"{fam}:{lname}", op)]
            for r in (o, g):
                word = np.where(np.isnan(r), np.uint32(0x7fc00000), r.view(np.uint32)).astype(np.int64)
                fresh = seen[idx] < 0
                seen[idx[fresh]] = word[fresh]
                assert np.array_equal(seen[idx], word), (fam, lname)
        assert (seen >= 0).all()


def test_generators_deliver_what_they_promise():
    """Counts the families state: exponent coverage (5), both sides of each threshold (6), the window's ends (7), and exactly one
    resp. 63 untame lanes in every wavefront of the lane orders (10)."""
    y, x, ey, ex = mc.atan2_exponents_draw()
    assert y.size == 1 << 24
    assert np.bincount(ey, minlength=255).min() >= 1 << 12 and np.bincount(ex, minlength=255).min() >= 1 << 12
    assert np.array_equal(mc.pattern(y) >> 23 & 0xff, ey) and np.array_equal(mc.pattern(x) >> 23 & 0xff, ex)

    y, x, which = mc.atan2_thresholds_draw()
    with np.errstate(all="ignore"):
        t = np.abs(y) / np.abs(x)                     # the oracle's own y / x: the host FPU
    for k, thr in enumerate((mc.T_LO, mc.T_HI, f32(1.0))):
        above, below = np.count_nonzero((which == k) & (t > thr)), np.count_nonzero((which == k) & (t < thr))
        at = np.count_nonzero((which == k) & (t == thr))
        print(f"threshold {thr!r}: {above} above, {below} below, {at} on it")
        assert above >= 1 << 16 and below + at >= 1 << 16 and at >= 16

    y, x, part = mc.atan2_window_draw()
    ey, ex = (mc.pattern(y) >> 23 & 0xff).astype(np.int64), (mc.pattern(x) >> 23 & 0xff).astype(np.int64)
    with np.errstate(all="ignore"):
        et = (mc.pattern(np.abs(y) / np.abs(x)) >> 23 & 0xff).astype(np.int64) - 127
    for end in (-mc.WIN_E, mc.WIN_E):
        for d in range(-2, 3):
            assert np.count_nonzero((part == 0) & (et == end + d)) >= 1 << 12, (end, d)
            assert np.count_nonzero((part == 1) & ((ey - 127 == end + d) | (ex - 127 == end + d)) & (np.abs(et) < mc.WIN_E)) >= 1 << 12, (end, d)
        for v in (y, x):
            assert np.count_nonzero(np.abs(v) == f32(2.0 ** end)) >= 16
    assert (np.abs(et[part == 0]) >= mc.WIN_E - 3).all() and (np.abs(et[part == 1]) <= 4).all()

    for pools, mask in ((mc.lane_pools_atan2(), lambda p: mc.tame_mask_atan2(p[0], p[1])), (mc.lane_pools_acos(), lambda p: mc.tame_mask_acos(p[0]))):
        tame, untame = pools
        assert mask(tame).all() and not mask(untame).any()
    lay = mc.lane_layouts()
    untame = {k: (v >= mc.POOL) for k, v in lay.items()}
    s = untame["sorted"].reshape(-1, mc.WAVE).sum(axis=1)
    assert set(s) == {0, mc.WAVE} and np.count_nonzero(s == 0) == 63
    assert (untame["one_untame"].reshape(-1, mc.WAVE).sum(axis=1) == 1).all()
    assert (untame["one_tame"].reshape(-1, mc.WAVE).sum(axis=1) == 63).all()
    for k in ("sorted", "one_untame", "one_tame"):
        assert np.array_equal(np.unique(lay[k]), np.arange(2 * mc.POOL))          # every value of both pools, in every layout
    for n in mc.LANE_NS:
        assert lay[f"one_untame[:{n}]"].size == n and lay[f"one_tame[:{n}]"].size == n
    assert untame["one_untame[:1]"].sum() == 0 and untame["one_tame[:1]"].sum() == 1       # a lone tame lane, a lone untame lane
