"""The end-before-scatter order of render_pixel on the GPU (csrc/mrt_trace.h): the frames of
tests/path_order_cases.py through Sampler give the words that the commit before the reorder gave.  That commit's GPU words
equalled its x86 words on every frame (tests/golden/make_path_order_pins.py gpu), so the x86 pins serve here too; the
tile-list kernel, which has no x86 counterpart, has a pin of its own, recorded on the GPU from the same commit."""
import functools

import numpy as np
import pytest

import path_order_cases as pc

pytestmark = pytest.mark.gpu


def _sampler():
    from micro_raytracer_amd import Sampler
    return Sampler(seed=pc.SEED, device=0)


@functools.lru_cache(maxsize=None)
def _render(name):
    from micro_raytracer_amd import load_render
    return load_render(pc.desc_of(name))


def _same(got, want, what):
    got = pc.words(got)
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[0]}: {got[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}"


@pytest.mark.parametrize("name", list(pc.FRAMES))
def test_frame_renders_the_parents_words(name):
    _, first, n, feat = pc.FRAMES[name]
    s = _sampler().create(_render(name))
    if first:
        s.set_accum(np.zeros((s.nh, s.nw, 3), np.float32), first)
    s.execute(_render(name), n_samples=n)
    got, cnt = s.accum()
    st = s.stats()
    s.close()
    assert cnt == first + n and st["kernel_features"] == feat
    _same(got, pc.load_pin("x86", name), name)


def test_split_calls_equal_one_call():
    """execute(7) then execute(33) against execute(40): the second call starts and stops inside a chunk.

    The two calls cut chunk 0 -- samples 0..6 go to the accumulator as one sum, samples 7..15 as another -- and the canonical
    order adds a chunk's samples from 0 (mrt_trace.h), so the cut reassociates that one sum: the commit before the reorder
    gives 4 words of this frame that differ from execute(40)'s by one unit in the last place (and so does this one: the same
    words).  What holds, and is asserted: the words of the two calls are the parent's words of the same two calls; they meet
    execute(40) within the rounding of the one reassociated sum -- each order rounds at most 16 + 3 times, every partial sum of
    non-negative samples is at most the final one, so 2 * 19 * 2^-24 of it; and a cut at a chunk end, 16 + 24, changes no bit."""
    s = _sampler()
    s.execute(_render("cornell_40"), n_samples=7)
    s.execute(_render("cornell_40"), n_samples=33)
    got, cnt = s.accum()
    s.close()
    assert cnt == 40
    _same(got, pc.load_pin("x86", "split_7_33"), "7 + 33")
    whole = pc.load_pin("x86", "cornell_40").view(np.float32)
    err = np.abs(got - whole)
    print(f"7 + 33 against 40: {int((pc.words(got) != pc.words(whole)).sum())} words differ, worst {float((err / np.maximum(whole, 1e-30)).max()):.3e} relative")
    assert (err <= 38 * 2.0 ** -24 * whole).all()
    s = _sampler()
    s.execute(_render("cornell_40"), n_samples=16)
    s.execute(_render("cornell_40"), n_samples=24)
    got, cnt = s.accum()
    s.close()
    assert cnt == 40
    _same(got, pc.load_pin("x86", "cornell_40"), "16 + 24")


def test_single_sample_calls_equal_one_call():
    """Five execute(1) calls (the look-ahead planes of the per-call path, Params.to_planes) are execute(5)."""
    a, b = _sampler(), _sampler()
    for _ in range(5):
        a.execute(_render("cornell_40"), n_samples=1)
    b.execute(_render("cornell_40"), n_samples=5)
    got, want = a.accum(), b.accum()
    a.close()
    b.close()
    assert got[1] == want[1] == 5
    _same(got[0], pc.words(want[0]), "5 x 1")


def test_tile_list_kernel_renders_the_parents_words():
    s = _sampler()
    s.execute_adaptive(_render("cornell_40"), 0.0, min_samples=32, max_samples=64, step=16)
    got, _ = s.accum()
    counts = s.sample_counts()
    s.close()
    assert (counts == 64).all()                  # threshold 0: no tile stops early, four rounds of the tile-list kernel
    _same(got, pc.load_pin("gpu", "adaptive"), "adaptive")


def test_camera_rays_give_the_frame():
    """mrt_radiance on the camera's own rays of the Cornell frame with aprt 0, where every sample of a pixel starts on that one
    ray: the frame's words.  (The radiance kernels all carry lights and maps, so their text did not move; the frame comes from
    the reordered F_IDENT kernel.)"""
    s = _sampler().create(_render("cornell_a0"))
    o, d = s.camera_rays(_render("cornell_a0"))
    got = s.radiance(_render("cornell_a0"), o, d, 40)
    s.close()
    _same(got, pc.load_pin("x86", "cornell_a0"), "radiance")
