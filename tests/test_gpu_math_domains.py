"""sincos_, acos_, atan2_ and the expressions built on them (csrc/mrt_math.h) on the device over their whole
domains: mrt_selftest_math against the oracle on every family of tests/math_cases.py, bit for bit, a NaN equal to any NaN, nothing
excluded.  The families put zeros, denormals, infinities, NaNs and ratios outside the fast window of recip_ / div_ / sqrt_ into
wavefronts of ordinary values, so that the wave votes of those cores are taken under partial exec masks, inside atan_pos_'s
divergent branches and next to a neighbour's special case; the lane-order family states that directly.  Ops 16..19 run in the test
hook's translation unit (math_selftest_ext, csrc/mrt_rayq.hip).  tests/test_math_domains_host.py holds the same families to the
x86 build and states the accuracy of the contract itself."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import math_cases as mc

pytestmark = pytest.mark.gpu
f32 = np.float32


def _oracle(pool, oracle_mod, op, a, b):
    """orc_math over a 16-worker pool (ctypes releases the GIL)."""
    ref = np.empty_like(a)
    bounds = np.linspace(0, a.size, 17).astype(np.int64)

    def part(i):
        lo, hi = bounds[i], bounds[i + 1]
        if hi > lo:
            ref[lo:hi] = oracle_mod.math(op, a[lo:hi], None if b is None else b[lo:hi])
    list(pool.map(part, range(16)))
    return ref


def _example(c, bad, dev, ref):
    k = np.flatnonzero(bad)[:3]
    return f"{c.name}: lanes {list(k % mc.WAVE)} of wavefronts {list(k // mc.WAVE)}: a={c.a[k]} b={None if c.b is None else c.b[k]} gpu={dev[k]} oracle={ref[k]}"


@pytest.mark.parametrize("name", list(mc.CHECKS))
def test_device_equals_the_oracle_bit_for_bit(name, oracle_mod):
    from micro_raytracer_amd import _lib
    ops, gen = mc.CHECKS[name]
    t0 = time.perf_counter()
    n = mis = 0
    first = None
    with ThreadPoolExecutor(max_workers=16) as pool:
        for c in gen(mc.CHUNK):
            assert c.a.size <= mc.CHUNK
            n += c.a.size
            for op in ops:
                dev = _lib.selftest_math(op, c.a, c.b)
                bad = ~mc.same_bits(dev, _oracle(pool, oracle_mod, op, c.a, c.b))
                if bad.any():
                    mis += int(np.count_nonzero(bad))
                    first = first or f"op {op}, " + _example(c, bad, dev, _oracle(pool, oracle_mod, op, c.a, c.b))
    print(f"{name}: ops {ops}, {n} inputs, {mis} mismatches, {time.perf_counter() - t0:.1f} s")
    assert mis == 0, f"{name}: {mis} of {n} inputs differ; {first}"


@pytest.mark.parametrize("fam,pools", [("lane_orders_atan2", mc.lane_pools_atan2), ("lane_orders_acos", mc.lane_pools_acos)])
def test_a_value_gives_the_same_word_in_every_lane_order(fam, pools, oracle_mod):
    """Family 10: the values of a tame and an untame pool sorted into whole wavefronts, with exactly one untame lane per wavefront,
    with 63 of them, and cut at n = 1, 63, 65, 257.  Every value's result is the oracle's word for it in every layout, and the same
    word between the layouts -- whatever its neighbours make the wave votes say."""
    from micro_raytracer_amd import _lib
    op = mc.CHECKS[fam][0][0]
    tame, untame = pools()
    va = np.concatenate([tame[0], untame[0]])
    vb = None if tame[1] is None else np.concatenate([tame[1], untame[1]])
    want = oracle_mod.math(op, va, vb)
    want = np.where(np.isnan(want), np.uint32(0x7fc00000), want.view(np.uint32))
    t0 = time.perf_counter()
    n = mis = 0
    words = {}
    for lname, idx in mc.lane_layouts().items():
        a, b = np.ascontiguousarray(va[idx]), None if vb is None else np.ascontiguousarray(vb[idx])
        dev = _lib.selftest_math(op, a, b)
        word = np.where(np.isnan(dev), np.uint32(0x7fc00000), dev.view(np.uint32))
        bad = word != want[idx]
        n += idx.size
        mis += int(np.count_nonzero(bad))
        assert not bad.any(), f"{fam}:{lname}: {np.count_nonzero(bad)} differ from the oracle, " + _example(mc.Chunk(lname, a, b), bad, dev, want[idx].view(f32))
        words[lname] = (idx, word)
    # between the orders: one word per value of the pools
    seen = np.full(va.size, -1, np.int64)
    for lname, (idx, word) in words.items():
        fresh = seen[idx] < 0
        seen[idx[fresh]] = word[fresh]
        moved = seen[idx] != word
        assert not moved.any(), f"{fam}:{lname}: {np.count_nonzero(moved)} values give another word than in an earlier layout, pool indices {idx[moved][:4]}"
    assert (seen >= 0).all()
    print(f"{fam}: {n} inputs in {len(words)} layouts, {mis} mismatches, {time.perf_counter() - t0:.1f} s")


def test_norm_and_the_two_roots_equal_the_host_fpu():
    """Op 12 (norm(v3(a, b, 0.25)).x: recip_sqrt_) and ops 18 / 19 (div2_(a, b, a + b): the sphere's two roots over one reciprocal)
    against the same expressions in float32 numpy -- correctly rounded sqrt and divide in the reference's operation order, the
    arithmetic the oracle uses."""
    from micro_raytracer_amd import _lib
    one = f32(1.0)
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        for name, ops in (("norm_scale", {12: lambda a, b: a * (one / np.sqrt((a * a + b * b) + f32(0.0625)))}),
                          ("two_roots", {18: lambda a, b: a / (a + b), 19: lambda a, b: b / (a + b)})):
            for c in mc.CHECKS[name][1](mc.CHUNK):
                for op, fn in ops.items():
                    dev = _lib.selftest_math(op, c.a, c.b)
                    ref = fn(c.a, c.b).astype(f32)
                    bad = ~mc.same_bits(dev, ref)
                    print(f"{name} op {op}: {c.a.size} inputs, {np.count_nonzero(bad)} mismatches against the host FPU")
                    assert not bad.any(), f"op {op}: {np.count_nonzero(bad)} differ; " + _example(c, bad, dev, ref)
    print(f"{time.perf_counter() - t0:.1f} s")
