"""Input families of the math-contract domain tests (tests/test_math_domains_host.py, tests/test_gpu_math_domains.py): the whole
domains of sincos_, acos_ and atan2_ (csrc/mrt_math.h) and of the expressions their call sites build on them,
as plain seeded functions.  A family is a generator of Chunk(name, a, b): f32 arrays of at most `chunk` elements (b is None for
the unary functions).  Element i of a chunk is thread i of the device's elementwise kernel -- lane i % 64 of wavefront i / 64 --,
so the order inside a chunk composes the wavefronts, which is what the lane-order family is about.

  1 sincos_lattice     2 sincos_wide      3 acos_dense       4 acos_rest        5 atan2_exponents   6 atan2_thresholds
  7 atan2_window       8 atan2_specials   9 unit_components  10 lane_orders_*   11 uv_ops (ops 16, 17)
  12 two_roots (ops 18, 19)               13 norm_scale (op 12)

CHECKS maps a family name to (ops, generator): the ops of mrt_selftest_math / emu_math / orc_math that family is run through."""
import numpy as np

f32 = np.float32
kPi = f32(3.14159274101257324)
CHUNK = 1 << 26
WAVE = 64
# the two range limits of atan_pos_ as f32 (tan(pi/8), tan(3 pi/8)) and the fast window of sqrt_ / recip_ / div_
T_LO, T_HI = f32(0.4142135623730950), f32(2.414213562373095)
WIN_E = 40


class Chunk:
    def __init__(self, name, a, b=None, first=None):
        self.name = name
        self.a = np.ascontiguousarray(a, f32)
        self.b = None if b is None else np.ascontiguousarray(b, f32)
        self.first = first                       # acos_dense: the bit pattern of a[0] (the chunk is consecutive patterns)
        assert self.b is None or self.b.shape == self.a.shape


def bits(sign, e, m):
    """f32 from sign bit, biased exponent and mantissa (arrays or scalars)."""
    return ((np.asarray(sign, np.uint32) << np.uint32(31)) | (np.asarray(e, np.uint32) << np.uint32(23)) | np.asarray(m, np.uint32)).view(f32)


def pattern(x):
    return np.asarray(x, f32).view(np.uint32)


def both_signs(x):
    x = np.asarray(x, f32)
    return np.concatenate([x, -x])


def ulp_step(x, k):
    """The f32 k patterns away from x in magnitude (k may be negative); x finite and non-zero."""
    x = np.asarray(x, f32)
    return (pattern(x).astype(np.int64) + k).astype(np.uint32).view(f32)


def strided_mantissas(rng, n_random=1 << 12):
    """2^12 mantissas on a regular stride with both ends, plus n_random random ones."""
    return np.concatenate([np.arange(0, 1 << 23, 1 << 11), [(1 << 23) - 1], rng.integers(0, 1 << 23, n_random)]).astype(np.uint32)


def every_exponent(e_lo, e_hi, mantissas):
    """Positive f32 over the biased exponents e_lo..e_hi (inclusive) with the given mantissas each."""
    e = np.arange(e_lo, e_hi + 1, dtype=np.uint32)[:, None] << np.uint32(23)
    return (e | mantissas[None, :].astype(np.uint32)).reshape(-1).view(f32)


SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000,
                     0x3f800000, 0xbf800000, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7fc00000], np.uint32).view(f32)


# ---- 1, 2: sincos_ ----------------------------------------------------------------------------------------------------------------
def sincos_lattice(chunk=CHUNK):
    """Every phi the path tracer forms (rand_normal, mrt_trace.h): (u2 * 2) * kPi in f32, u2 on the 2^-23 lattice of [0, 1)."""
    u2 = (np.arange(1 << 23, dtype=np.float64) * 2.0 ** -23).astype(f32)
    yield Chunk("sincos_lattice", (u2 * f32(2.0)) * kPi)


def sincos_wide(chunk=CHUNK):
    """The contract's whole domain |x| <= 65536 and its outside: every exponent from 0 to that of 65536 (above 65536 itself the
    contract says NaN), 65536 +- 1 ulp, inf, NaN, and the f32 nearest to k pi/2 with its two neighbours for every k up to 41722
    (the last multiple below 65536 + pi/2): the quadrant boundaries, where floor_(fma_(x, 2/pi, 0.5)) decides."""
    rng = np.random.default_rng(202)
    x = every_exponent(0, 127 + 16, strided_mantissas(rng))
    edge = np.concatenate([ulp_step(f32(65536.0), np.array([-1, 0, 1])), [f32(np.inf), f32(np.nan)]]).astype(f32)
    k = np.arange(1, 41722 + 1, dtype=np.float64)          # step 1: 3 * 41722 * 2 values, the family stays under 2^22
    q = (k * (np.pi / 2)).astype(f32)
    quad = np.concatenate([ulp_step(q, -1), q, ulp_step(q, 1)])
    out = both_signs(np.concatenate([x, edge, quad]))
    assert out.size < 1 << 22
    yield Chunk("sincos_wide", out)


# ---- 3, 4: acos_ ------------------------------------------------------------------------------------------------------------------
ACOS_DENSE_LO = (127 - 13) << 23           # 2^-13: below it the polynomial term is under half an ulp of pi/2
ONE = 127 << 23


def acos_dense(chunk=CHUNK):
    """Every pattern with 2^-13 <= |x| <= 1, positive then negative, in pattern order."""
    for sign in (0, 1):
        for first in range(ACOS_DENSE_LO, ONE + 1, chunk):
            last = min(first + chunk, ONE + 1)
            p = np.arange(first, last, dtype=np.uint32) | np.uint32(sign << 31)
            yield Chunk("acos_dense", p.view(f32), first=int(p[0]))


def acos_rest(chunk=CHUNK):
    """Exponents 0 .. that of 2^-13 with 2^12 + 1 mantissas each; +-0.5 and +-1 with their +-1 and +-2 ulp neighbours (1 + 1 ulp
    and 1 + 2 ulp are outside the domain: NaN); 2, inf, NaN."""
    rng = np.random.default_rng(204)
    x = every_exponent(0, 127 - 13, strided_mantissas(rng, 0))
    near = np.concatenate([ulp_step(f32(0.5), np.arange(-2, 3)), ulp_step(f32(1.0), np.arange(-2, 3))])
    edge = np.array([2.0, np.inf, np.nan], f32)
    yield Chunk("acos_rest", both_signs(np.concatenate([x, near, edge])))


# ---- 5 .. 9: atan2_ (a = y, b = x) --------------------------------------------------------------------------------------------------
def _draw(rng, e, n=None):
    n = e.size if n is None else n
    return bits(rng.integers(0, 2, n), e, rng.integers(0, 1 << 23, n))


def atan2_exponents_draw(n=1 << 24):
    rng = np.random.default_rng(205)
    ey, ex = rng.integers(0, 255, n, dtype=np.uint32), rng.integers(0, 255, n, dtype=np.uint32)
    return _draw(rng, ey), _draw(rng, ex), ey, ex


def atan2_exponents(chunk=CHUNK):
    """2^24 pairs, both biased exponents uniform over 0..254 (zero and denormals to the largest finite), random signs, mantissas."""
    y, x, ey, ex = atan2_exponents_draw()
    assert np.bincount(ey, minlength=255).min() >= 1 << 12 and np.bincount(ex, minlength=255).min() >= 1 << 12
    yield Chunk("atan2_exponents", y, x)


def atan2_thresholds_draw(n=1 << 20):
    """y = the f32 nearest to t x, t one of atan_pos_'s range limits or 1 (where its middle range's argument changes sign), moved
    by -2^10 .. 2^10 ulp.  Returns y, x and which t (0, 1, 2)."""
    rng = np.random.default_rng(206)
    x = _draw(rng, rng.integers(1, 255, n, dtype=np.uint32))
    which = rng.integers(0, 3, n)
    t = ulp_step(np.array([T_LO, T_HI, f32(1.0)], f32)[which], rng.integers(-(1 << 10), (1 << 10) + 1, n))
    with np.errstate(over="ignore", under="ignore"):
        y = (t.astype(np.float64) * x.astype(np.float64)).astype(f32)
    y = np.where(rng.integers(0, 2, n) == 1, -y, y).astype(f32)
    return y, x, which


def atan2_thresholds(chunk=CHUNK):
    y, x, _ = atan2_thresholds_draw()
    yield Chunk("atan2_thresholds", y, x)


def atan2_window_draw(n=1 << 18):
    """The ends of the fast window [2^-40, 2^40] of recip_ / div_.  Part 0: pairs whose ratio's exponent is within +-2 of -40 and
    of +40 (atan_pos_'s recip_(t) sits at the window's end), operands anywhere that allows it.  Part 1: an operand within +-2
    exponents of 2^-40 or 2^40 and the ratio inside the window (div_(|y|, |x|) sits at the end).  Every 8th pair of either part
    has the mantissa of a power of two, so that exactly 2^-40 and 2^40 occur.  Returns y, x, part."""
    rng = np.random.default_rng(207)
    part = (np.arange(2 * n) >= n).astype(np.int64)
    end = np.where(rng.integers(0, 2, 2 * n) == 1, WIN_E, -WIN_E) + rng.integers(-2, 3, 2 * n)
    # part 0: ey - ex = end, ex anywhere with both exponents normal
    ex0 = rng.integers(1 + 44, 254 - 44, 2 * n)
    ey0 = ex0 + end
    # part 1: one operand at the end, the other within 2^+-3 of it
    ex1 = 127 + end
    ey1 = ex1 + rng.integers(-3, 4, 2 * n)
    swap = rng.integers(0, 2, 2 * n) == 1
    ex1, ey1 = np.where(swap, ey1, ex1), np.where(swap, ex1, ey1)
    ex, ey = np.where(part == 0, ex0, ex1).astype(np.uint32), np.where(part == 0, ey0, ey1).astype(np.uint32)
    y, x = _draw(rng, ey), _draw(rng, ex)
    pow2 = (np.arange(2 * n) % 8) == 0
    y = np.where(pow2, (pattern(y) & np.uint32(0xff800000)).view(f32), y).astype(f32)
    x = np.where(pow2 & (np.arange(2 * n) % 16 == 0), (pattern(x) & np.uint32(0xff800000)).view(f32), x).astype(f32)
    return y, x, part


def atan2_window(chunk=CHUNK):
    y, x, _ = atan2_window_draw()
    yield Chunk("atan2_window", y, x)


def atan2_specials(chunk=CHUNK):
    """{+-0, +-min denormal, +-max denormal, +-min normal, +-1, +-max finite, +-inf, NaN} x itself."""
    y, x = np.meshgrid(SPECIALS, SPECIALS, indexing="ij")
    yield Chunk("atan2_specials", y.reshape(-1), x.reshape(-1))


def np_norm(v):
    """norm of lin.rs:60-66 in float32 numpy, in its operation order: v * (1 / sqrt(x x + y y + z z))."""
    v = np.asarray(v, f32)
    m = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    return (v * (f32(1.0) / np.sqrt(m))[:, None]).astype(f32)


def unit_vectors(n=1 << 20):
    """norm of n random vectors; one in eight has one or two components exactly +-0, one in sixteen a component below 2^-40 of
    the largest.  These are the v of hit_uv's sphere branch; (v.x, -v.y) go to atan2_, v.z to env_uv's acos_."""
    rng = np.random.default_rng(209)
    v = rng.normal(size=(n, 3)).astype(f32)
    i = np.arange(n)
    zero = i % 8 == 0
    k = rng.integers(0, 3, n)
    v[zero, k[zero]] = np.where(rng.integers(0, 2, n) == 1, f32(-0.0), f32(0.0))[zero]
    two = i % 16 == 0
    k2 = (k + 1 + rng.integers(0, 2, n)) % 3
    v[two, k2[two]] = np.where(rng.integers(0, 2, n) == 1, f32(-0.0), f32(0.0))[two]
    tiny = i % 16 == 5
    big = np.abs(v).max(axis=1)
    scale = np.ldexp(f32(1.0), -rng.integers(41, 140, n)).astype(f32)
    with np.errstate(under="ignore"):
        v[tiny, k[tiny]] = (v[tiny, k[tiny]] / np.abs(v[tiny, k[tiny]]) * big[tiny] * scale[tiny] * f32(0.99)).astype(f32)
    return np_norm(v)


def unit_components(chunk=CHUNK):
    v = unit_vectors()
    yield Chunk("unit_components", v[:, 0], -v[:, 1])


# ---- 10: lane orders ----------------------------------------------------------------------------------------------------------------
# Tame = every operand and ratio inside the window and one branch of atan_pos_ (the middle one, whose div_ then runs its core under
# a full mask); untame = specials, ratios and operands outside the window, and the other two branches.  Two pools of 63 * 64 values
# each; a layout is an order of pool indices (tame i, untame 4032 + i).  No two of the layouts below can hold the same number of
# copies of a value (one holds 63 tame lanes per untame one, the other the inverse), so what they share is the SET of values: every
# layout holds every value of both pools at least once, and a value's result must be the same word wherever it stands.
POOL = 63 * WAVE


def lane_pools_atan2():
    rng = np.random.default_rng(210)
    n = POOL
    x = _draw(rng, rng.integers(127 - 30, 127 + 30, n, dtype=np.uint32))
    t = rng.uniform(0.5, 2.0, n)
    y = (t * x.astype(np.float64)).astype(f32) * np.where(rng.integers(0, 2, n) == 1, f32(-1), f32(1))
    tame = (y.astype(f32), x)
    sy, sx = np.meshgrid(SPECIALS, SPECIALS, indexing="ij")
    uy, ux = [sy.reshape(-1)], [sx.reshape(-1)]
    m = (n - sy.size) // 4
    xx = _draw(rng, rng.integers(127 - 30, 127 + 30, 4 * m + 3, dtype=np.uint32))
    r = np.concatenate([np.ldexp(rng.uniform(1, 2, m), rng.integers(41, 60, m)),          # ratio above the window: recip_ falls back
                        np.ldexp(rng.uniform(1, 2, m), -rng.integers(41, 60, m)),         # ratio below it
                        rng.uniform(2.5, 1000.0, m), rng.uniform(1e-3, 0.4, n - sy.size - 3 * m)])     # the other two branches
    with np.errstate(over="ignore", under="ignore"):
        uy.append((r * xx[:r.size].astype(np.float64)).astype(f32))
    ux.append(xx[:r.size])
    untame = (np.concatenate(uy).astype(f32), np.concatenate(ux).astype(f32))
    assert tame[0].size == n and untame[0].size == n
    return tame, untame


def lane_pools_acos():
    rng = np.random.default_rng(211)
    n = POOL
    tame = (_draw(rng, rng.integers(127 - 13, 127, n, dtype=np.uint32)), None)
    edge = np.concatenate([ulp_step(f32(1.0), np.arange(0, 3)), np.array([2.0, np.inf, np.nan, 0.0, 1e-45, 1e-39, 3e38], f32)]).astype(f32)
    edge = both_signs(edge)
    reps = -(-n // edge.size)
    untame = (np.tile(edge, reps)[:n], None)
    return tame, untame


def tame_mask_atan2(y, x):
    """The definition above, stated on the values: window, ratio (host FPU, the oracle's own y / x) and branch."""
    with np.errstate(all="ignore"):
        ay, ax = np.abs(y), np.abs(x)
        t = ay / ax
        lo, hi = f32(2.0 ** -WIN_E), f32(2.0 ** WIN_E)
        win = (ay >= lo) & (ay <= hi) & (ax >= lo) & (ax <= hi)
        return win & (t > T_LO) & (t <= T_HI) & ((t - f32(1)) != 0)        # (t == 1 sends a zero numerator to the middle range's div_)


def tame_mask_acos(x):
    with np.errstate(all="ignore"):
        a = np.abs(x)
        return (a >= f32(2.0 ** -13)) & (a < f32(1.0))


LANE_NS = (1, 63, 65, 257)


def lane_layouts():
    """name -> pool indices.  sorted: the tame pool in 63 whole wavefronts, then the untame pool in 63; one_untame: 4032 wavefronts
    of 63 tame lanes and one untame lane (at lane (7 w + 3) % 64); one_tame: the inverse; and the first n elements of the last two
    for n in LANE_NS, which leaves a partial last wavefront."""
    t, u = np.arange(POOL), POOL + np.arange(POOL)
    out = {"sorted": np.concatenate([t, u])}
    for name, few, many in (("one_untame", u, t), ("one_tame", t, u)):
        w = np.arange(POOL)
        lay = many[(w[:, None] * WAVE + np.arange(WAVE)[None, :]) % POOL]
        lay[w, (7 * w + 3) % WAVE] = few
        out[name] = lay.reshape(-1)
        for n in LANE_NS:
            out[f"{name}[:{n}]"] = out[name][:n].copy()
    return out


def _lane_orders(fn_name, pools):
    tame, untame = pools
    va = np.concatenate([tame[0], untame[0]])
    vb = None if tame[1] is None else np.concatenate([tame[1], untame[1]])
    for name, idx in lane_layouts().items():
        yield Chunk(f"{fn_name}:{name}", va[idx], None if vb is None else vb[idx])


def lane_orders_atan2(chunk=CHUNK):
    yield from _lane_orders("lane_orders_atan2", lane_pools_atan2())


def lane_orders_acos(chunk=CHUNK):
    yield from _lane_orders("lane_orders_acos", lane_pools_acos())


# ---- 11 .. 13: the op checks ----------------------------------------------------------------------------------------------------------
def uv_longitude(chunk=CHUNK):
    """op 16 takes (v.x, v.y) and negates the second itself, as hit_uv and env_uv do."""
    v = unit_vectors()
    y, x = np.meshgrid(SPECIALS, SPECIALS, indexing="ij")
    yield Chunk("uv_longitude:unit", v[:, 0], v[:, 1])
    yield Chunk("uv_longitude:specials", y.reshape(-1), x.reshape(-1))


def uv_latitude(chunk=CHUNK):
    """op 17 on v.z of the unit vectors (exactly +-1 at the poles), the specials and acos_rest's values (the clamp's two sides)."""
    yield Chunk("uv_latitude:unit", unit_vectors()[:, 2])
    yield Chunk("uv_latitude:specials", SPECIALS)
    for c in acos_rest():
        yield Chunk("uv_latitude:acos_rest", c.a)


def operand_pairs(name, seed, n=1 << 22):
    """Half with both exponents inside the fast window (whole wavefronts take the cores), half raw bit patterns (zeros, denormals,
    infinities, NaNs: the expansion), in alternating blocks of 2^12 so that both kinds of wavefront and their borders occur."""
    rng = np.random.default_rng(seed)
    def windowed():
        return _draw(rng, rng.integers(127 - WIN_E, 127 + WIN_E, n, dtype=np.uint32))
    def raw():
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(f32)
    block = (np.arange(n) >> 12) & 1
    a = np.where(block == 0, windowed(), raw()).astype(f32)
    b = np.where(block == 0, windowed(), raw()).astype(f32)
    # raw patterns inside windowed wavefronts: one lane in 4096 of the windowed blocks
    lone = (np.arange(n) % 4099 == 7)
    a = np.where(lone, raw(), a).astype(f32)
    yield Chunk(name, a, b)


def two_roots(chunk=CHUNK):
    yield from operand_pairs("two_roots", 212)


def norm_scale(chunk=CHUNK):
    yield from operand_pairs("norm_scale", 213)


CHECKS = {
    "sincos_lattice": ((0, 1), sincos_lattice),
    "sincos_wide": ((0, 1), sincos_wide),
    "acos_dense": ((2,), acos_dense),
    "acos_rest": ((2,), acos_rest),
    "atan2_exponents": ((3,), atan2_exponents),
    "atan2_thresholds": ((3,), atan2_thresholds),
    "atan2_window": ((3,), atan2_window),
    "atan2_specials": ((3,), atan2_specials),
    "unit_components": ((3,), unit_components),
    "lane_orders_atan2": ((3,), lane_orders_atan2),
    "lane_orders_acos": ((2,), lane_orders_acos),
    "uv_longitude": ((16,), uv_longitude),
    "uv_latitude": ((17,), uv_latitude),
    "two_roots": ((18, 19), two_roots),
    "norm_scale": ((12,), norm_scale),
}


def same_bits(g, o):
    """Bit for bit, a NaN equal to any NaN (payloads are not part of the contract)."""
    return (g.view(np.uint32) == o.view(np.uint32)) | (np.isnan(g) & np.isnan(o))
