"""The fast correctly rounded cores of the math contract (csrc/mrt_math.h: sqrt_, recip_, div_, recip_sqrt_) against
IEEE arithmetic.

The reference's sqrt / recip / divide are Rust f32 operations, i.e. IEEE correctly rounded (src/lin.rs:60-66,
src/rt.rs:335-359, 400-412); the oracle computes them with the host FPU.  On the device a wavefront whose operands all
lie inside the exponent window [2^-40, 2^40] runs the bare refinement sequences instead of the compiler's full
expansions.  Checked here:
  * on the device (mrt_selftest_sweep): every one of the 2^32 f32 bit patterns for sqrt and recip, 10^10 operand pairs
    for divide and 2^32 vectors for the norm scale -- fast core == compiler expansion, bit for bit;
  * against the host FPU (numpy, the arithmetic the oracle uses): every 2^32 pattern for sqrt and recip and 2^28 pairs
    for divide through mrt_selftest_math.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("op,name,count", [(0, "sqrt", 1 << 32), (1, "recip", 1 << 32), (2, "divide", 10_000_000_000),
                                            (3, "norm scale", 1 << 32)])
def test_fast_cores_equal_the_compiler_expansions_on_device(op, name, count):
    from micro_raytracer_amd import _lib
    mis, ex = _lib.selftest_sweep(op, 0, count, seed=12345)
    print(f"{name}: {count} inputs, {mis} mismatches")
    assert mis == 0, f"{name}: {mis} mismatches, e.g. a={ex[0]!r} b={ex[1]!r} fast={ex[2]!r} ieee={ex[3]!r}"


def _same(g, o):
    return (g.view(np.uint32) == o.view(np.uint32)) | (np.isnan(g) & np.isnan(o))


def test_sqrt_and_recip_equal_the_host_fpu_on_every_f32():
    """All 2^32 bit patterns, 2^26 per call, against numpy's sqrt and 1/x (correctly rounded, the oracle's arithmetic)."""
    from micro_raytracer_amd import _lib
    step = 1 << 26
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        for first in range(0, 1 << 32, step):
            x = np.arange(first, first + step, dtype=np.uint64).astype(np.uint32).view(np.float32)
            g = _lib.selftest_math(6, x)
            bad = ~_same(g, np.sqrt(x))
            assert not bad.any(), f"sqrt: {np.count_nonzero(bad)} mismatches from pattern {first:#x}, x={x[bad][:3]} gpu={g[bad][:3]}"
            g = _lib.selftest_math(5, x)
            bad = ~_same(g, one / x)
            assert not bad.any(), f"recip: {np.count_nonzero(bad)} mismatches from pattern {first:#x}, x={x[bad][:3]} gpu={g[bad][:3]}"


def test_divide_equals_the_host_fpu_on_random_pairs():
    """2^28 pairs: half with exponents inside the fast window (whole wavefronts take the core), half raw bit patterns."""
    from micro_raytracer_amd import _lib
    rng = np.random.default_rng(7)
    n = 1 << 24
    with np.errstate(all="ignore"):
        for rep in range(16):
            if rep % 2 == 0:
                def draw():
                    e = rng.integers(127 - 40, 127 + 40, n, dtype=np.uint32)
                    return ((rng.integers(0, 2, n, dtype=np.uint32) << 31) | (e << 23) | rng.integers(0, 1 << 23, n, dtype=np.uint32)).view(np.float32)
                a, b = draw(), draw()
            else:
                a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
                b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
            g = _lib.selftest_math(7, a, b)
            bad = ~_same(g, a / b)
            assert not bad.any(), f"divide: {np.count_nonzero(bad)} mismatches, a={a[bad][:3]} b={b[bad][:3]} gpu={g[bad][:3]}"


# ---- pow_ (csrc/mrt_math.h), the tone map's x^gamma, against the oracle's om_powf: the tone-map bytes follow it bit for bit
_POW_CHUNK = 1 << 26


def _pow_mismatches(x, g, oracle_mod, pool):
    """(count, examples) of pow_(x, g) on the device against om_powf, NaN equal to NaN; the oracle side split over the pool
    (ctypes releases the GIL)."""
    from micro_raytracer_amd import _lib
    dev = _lib.selftest_math(4, x, g)
    ref = np.empty_like(x)
    bounds = np.linspace(0, x.size, 17).astype(np.int64)

    def part(i):
        lo, hi = bounds[i], bounds[i + 1]
        ref[lo:hi] = oracle_mod.math(4, x[lo:hi], g[lo:hi])
    list(pool.map(part, range(16)))
    bad = ~_same(dev, ref)
    return int(np.count_nonzero(bad)), (x[bad][:3], g[bad][:3], dev[bad][:3], ref[bad][:3])


def test_pow_equals_the_oracle_on_every_non_negative_f32_at_gamma_0_8(oracle_mod):
    """All 2^31 non-negative f32 patterns (zeros, denormals, +inf and NaNs included) at the loader's default gamma 0.8, in
    chunks of 2^26, every mantissa (no striding)."""
    import time
    from concurrent.futures import ThreadPoolExecutor
    g = np.full(_POW_CHUNK, 0.8, np.float32)
    t0 = time.perf_counter()
    total = 0
    with ThreadPoolExecutor(max_workers=16) as pool:
        for first in range(0, 1 << 31, _POW_CHUNK):
            x = np.arange(first, first + _POW_CHUNK, dtype=np.uint32).view(np.float32)
            mis, ex = _pow_mismatches(x, g, oracle_mod, pool)
            total += mis
            assert mis == 0, f"pow at gamma 0.8: {mis} mismatches from pattern {first:#x}: x, g, gpu, oracle = {ex}"
    print(f"pow gamma 0.8: 2^31 inputs, {total} mismatches, {time.perf_counter() - t0:.1f} s")


def _every_exponent(mantissas):
    """x over all 256 biased exponents (0: zero and denormals, 255: +inf and NaNs) with the given mantissas each."""
    e = np.arange(256, dtype=np.uint32)[:, None] << 23
    return (e | mantissas[None, :].astype(np.uint32)).reshape(-1).view(np.float32)


@pytest.mark.parametrize("gamma", [0.4, 1 / 2.2, 1.0, 2.2, 0.0, -0.5])
def test_pow_equals_the_oracle_over_every_exponent(gamma, oracle_mod):
    """Every exponent of x with 2^12 + 2^12 mantissas (a regular stride with both ends, and random ones) at the camera gammas
    the loader accepts."""
    from concurrent.futures import ThreadPoolExecutor
    rng = np.random.default_rng(int(abs(gamma) * 1000) + 3)
    m = np.concatenate([np.arange(0, 1 << 23, 1 << 11), [(1 << 23) - 1, 1, 2],
                        rng.integers(0, 1 << 23, 1 << 12)]).astype(np.uint32)
    x = _every_exponent(m)
    g = np.full(x.size, gamma, np.float32)
    with ThreadPoolExecutor(max_workers=16) as pool:
        mis, ex = _pow_mismatches(x, g, oracle_mod, pool)
    print(f"pow gamma {gamma}: {x.size} inputs, {mis} mismatches")
    assert mis == 0, f"pow at gamma {gamma}: {mis} mismatches: x, g, gpu, oracle = {ex}"


def test_pow_equals_the_oracle_on_random_pairs(oracle_mod):
    """2^24 (x, gamma) pairs, gamma uniform in [-4, 4], x's exponent uniform over all 256 (2^16 mantissas each on average);
    one x in 8 negative."""
    from concurrent.futures import ThreadPoolExecutor
    rng = np.random.default_rng(29)
    n = 1 << 24
    e = rng.integers(0, 256, n, dtype=np.uint32)
    sign = (rng.integers(0, 8, n) == 0).astype(np.uint32) << 31
    x = (sign | (e << 23) | rng.integers(0, 1 << 23, n, dtype=np.uint32)).view(np.float32)
    g = rng.uniform(-4.0, 4.0, n).astype(np.float32)
    assert np.bincount(e, minlength=256).min() >= 1 << 12
    with ThreadPoolExecutor(max_workers=16) as pool:
        mis, ex = _pow_mismatches(x, g, oracle_mod, pool)
    print(f"pow random pairs: {n} inputs, {mis} mismatches")
    assert mis == 0, f"pow on random pairs: {mis} mismatches: x, g, gpu, oracle = {ex}"
