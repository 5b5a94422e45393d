"""The band planner of a tapered launch (csrc/mrt_plan.cpp plan_bands) on the host.

A launch's chunks are cut into contiguous bands: listed ones, each at least two chunks, longest first, then single chunks.
Whatever the chunk count, the tile count, the resident wavefronts and the MRT_BANDS knob, the bands cover every chunk exactly
once, in order, with non-increasing lengths, and the rule is the one DESIGN.md derives: with `rem` chunks left, a band of
floor(rem * tiles / (tiles + 4 * slots)) chunks, and single chunks from where that falls below two."""
import ctypes as C
import itertools

import pytest

from emu.build import shared

CHUNKS = [1, 2, 3, 4, 5, 63, 64]
# (tiles, slots): the headline frame, the 512 x 512 frame, a 44 x 20 frame, one tile of a tile list, a frame just below the
# size that is not split, and a device that reports no slot
SHAPES = [(32400, 8192), (4096, 8192), (18, 8192), (1, 8192), (99999, 8192), (32400, 0), (300, 96)]


def _bind(L):
    L.bp_plan.restype = C.c_uint32
    L.bp_plan.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint32)]
    L.bp_max_bands.restype = C.c_uint32


@pytest.fixture(scope="module")
def probe():
    return shared("bands_probe", _bind)


def plan(L, n_chunks, tiles, slots, bands=None):
    """(listed [(first, len)], tail, items, entries the knob parsed)"""
    m = L.bp_max_bands()
    out = (C.c_uint32 * (3 + 2 * m))()
    k = L.bp_plan(n_chunks, tiles, slots, bands.encode() if bands is not None else None, out)
    n = out[0]
    assert n <= m
    return [(out[3 + i], out[3 + m + i]) for i in range(n)], out[1], out[2], k


def check_cover(listed, tail, items, n_chunks):
    """every chunk once, in order; listed bands of two chunks or more, non-increasing; single chunks behind them"""
    at = 0
    prev = None
    for first, ln in listed:
        assert first == at and ln >= 2 and (prev is None or ln <= prev), (listed, n_chunks)
        at += ln
        prev = ln
    assert at == tail <= n_chunks and items == len(listed) + (n_chunks - tail), (listed, tail, items, n_chunks)
    covered = [c for first, ln in listed for c in range(first, first + ln)] + list(range(tail, n_chunks))
    assert covered == list(range(n_chunks))


@pytest.mark.parametrize("tiles,slots", SHAPES)
def test_rule_covers_every_chunk_once_and_tapers(probe, tiles, slots):
    m = probe.bp_max_bands()
    for n in CHUNKS + [22, 150]:                     # 150 chunks cut at 64 per launch: launches of 64, 64 and 22
        listed, tail, items, k = plan(probe, n, tiles, slots)
        assert k == 0
        check_cover(listed, tail, items, n)
        # the rule, band by band
        at = 0
        for first, ln in listed:
            assert ln == (n - at) * tiles // (tiles + 4 * slots)
            at += ln
        if len(listed) < m and at < n:
            assert (n - at) * tiles // (tiles + 4 * slots) < 2      # ... and it ends in single chunks where the rule says so


def test_rule_at_the_benchmark_sizes(probe):
    # 1080p x 1024 samples: 64 chunks, 240 x 135 tiles, 256 CUs x 32 wavefronts
    assert plan(probe, 64, 32400, 8192)[:3] == ([(0, 31), (31, 16), (47, 8), (55, 4), (59, 2)], 61, 8)
    # 512 x 512 x 64 samples: 4 chunks, 4096 tiles: one chunk per item, as with four interleaved phases
    assert plan(probe, 4, 4096, 8192)[:3] == ([], 0, 4)
    # an adaptive round of one or two chunks over a short tile list: single chunks
    for n, tiles in itertools.product((1, 2), (1, 7, 18)):
        assert plan(probe, n, tiles, 8192)[:3] == ([], 0, n)


@pytest.mark.parametrize("bands,n,want", [
    ("48,8,4,2,1,1", 64, ([(0, 48), (48, 8), (56, 4), (60, 2)], 62, 6)),
    ("48,8,4,2,1,1", 10, ([(0, 10)], 10, 1)),                  # cut to the launch's chunks
    ("48,8,4,2,1,1", 50, ([(0, 48), (48, 2)], 50, 2)),
    ("64", 64, ([(0, 64)], 64, 1)),                            # a single band of all chunks
    ("64", 1, ([], 0, 1)),
    ("1", 5, ([], 0, 5)),                                      # all ones
    ("1,1,1,1,1", 5, ([], 0, 5)),
    ("3,2,1", 6, ([(0, 3), (3, 2)], 5, 3)),
    ("4", 6, ([(0, 4)], 4, 3)),                                # behind the list: single chunks
    ("2,2,2,2,2,2,2,2", 20, ([(2 * i, 2) for i in range(8)], 16, 12)),
])
def test_forced_bands(probe, bands, n, want):
    listed, tail, items, k = plan(probe, n, 32400, 8192, bands)
    assert k == len(bands.split(","))
    check_cover(listed, tail, items, n)
    assert (listed, tail, items) == want


@pytest.mark.parametrize("bands", ["", "0", "3,4", "8,x", "4,,2", "2,2,2,2,2,2,2,2,2", "-1"])
def test_invalid_band_lists_are_ignored(probe, bands):
    """Not a list of positive, non-increasing lengths, or more listed bands than the table holds: the rule applies."""
    assert plan(probe, 64, 32400, 8192, bands) == plan(probe, 64, 32400, 8192)
