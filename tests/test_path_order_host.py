"""Kernels without lights and maps decide a path's end before its scatter and share one pair of draws between scattering and
regenerated lanes (csrc/mrt_trace.h render_pixel).  The order changes no bit: the x86 build of the same header
(tests/emu) renders the frames of tests/path_order_cases.py to the words that the commit before the reorder rendered
(tests/golden/path_order_x86_*.npy, recorded by tests/golden/make_path_order_pins.py), NaN bits included, and the oracle --
the independent text -- agrees at the bar of tests/test_gpu_parity.py."""
import functools

import numpy as np
import pytest

import path_order_cases as pc
from conftest import make_holder

TOL = 1e-4          # tests/test_gpu_parity.py: mean radiance against the oracle, per channel, L-inf


@functools.lru_cache(maxsize=None)
def _x86(name):
    from emu import emu
    _, first, n, _ = pc.FRAMES[name]
    _, holder = make_holder(pc.desc_of(name))
    acc, seg = emu.render(holder, pc.SEED, n, sample_base=first)
    acc.setflags(write=False)
    return acc, seg


@pytest.mark.parametrize("name", list(pc.FRAMES))
def test_frame_renders_the_parents_words(emu_mod, name):
    """Reordered kernels (F_IDENT, F_BOX) and, as controls, one kernel with lights and one with maps, whose text did not move."""
    got = pc.words(_x86(name)[0])
    want = pc.load_pin("x86", name)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{name}: {len(bad)} words differ, first at {bad[0]}: {got[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}"


def test_two_calls_that_cut_a_chunk_render_the_parents_words(emu_mod):
    """Samples [0, 7) then [7, 40) into one accumulator (tests/test_gpu_path_order.py says why this is not the frame of 40)."""
    _, holder = make_holder(pc.desc_of("cornell_40"))
    acc, _ = emu_mod.render(holder, pc.SEED, 7)
    acc, _ = emu_mod.render(holder, pc.SEED, 33, sample_base=7, accum=acc)
    assert np.array_equal(pc.words(acc), pc.load_pin("x86", "split_7_33"))


def test_pins_are_not_trivial():
    """Every frame's pin holds light, the whole-wave extremes hold what they claim, and the split frame is part of the whole one."""
    for name in pc.FRAMES:
        a = pc.load_pin("x86", name).view(np.float32)
        assert np.isfinite(a).all() and (a > 0).any(), name
    sky = pc.load_pin("x86", "sky").view(np.float32)
    assert (sky == sky[0, 0]).all()                                     # every sample of every pixel is the raw sky colour
    assert not np.array_equal(pc.load_pin("x86", "cornell_40"), pc.load_pin("x86", "cornell_7_33"))
    assert not np.array_equal(pc.load_pin("x86", "cornell_b0"), pc.load_pin("x86", "cornell_b1"))
    assert not np.array_equal(pc.load_pin("x86", "coin_a0"), pc.load_pin("x86", "coin_a005"))


def test_whole_wave_extremes_count_their_segments(emu_mod):
    """Sky only: one segment per sample.  Closed room, no emitter: a path runs to the bounce cut, bounce + 1 segments -- but for
    the few that a rough scatter sends through a wall, so the mean stays above bounce segments."""
    assert _x86("sky")[1] == 8 * 8 * 20
    assert 8 * 8 * 20 * 5 < _x86("closed")[1] <= 8 * 8 * 20 * (5 + 1)


@pytest.mark.parametrize("name", [n for n in pc.FRAMES if pc.FRAMES[n][1] == 0])
def test_frame_meets_the_oracle(emu_mod, oracle_mod, name):
    _, _, n, _ = pc.FRAMES[name]
    _, holder = make_holder(pc.desc_of(name))
    o = oracle_mod.Oracle(holder, seed=pc.SEED)
    o.execute(n)
    ref, _ = o.accum()
    err = float(np.max(np.abs(_x86(name)[0] - ref))) / n
    print(f"{name}: mean radiance against the oracle, L-inf {err:.3e}")
    assert err <= TOL, (name, err)
