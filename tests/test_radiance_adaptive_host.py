"""mrt_radiance_adaptive without a GPU: the per-lane body of csrc/mrt_rays_adapt.h, built for x86 (tests/emu/rays_adapt_probe.cpp),
holds one round over a tile list to the x86 ray body of mrt_radiance at every launch shape; the ABI struct, the header, the CLI
rules and cameras.render_equirect(adaptive=...).  The same round on one 44 x 36 grid per feature set of pt_rays_tiles
(tests/radiance_adapt_cases.py: wild rays beside tame ones in every odd tile), and the preconditions of
tests/test_gpu_radiance_adaptive_oracle.py, from the x86 ray body's sums alone."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import radiance_adapt_cases as AC
import rays_ref as Y
from conftest import make_holder
from emu.build import ptr as _p, shared

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = (12, 10)                       # 2 x 2 tiles: the right column 4 pixels wide, the lower row 2 pixels high
LISTED = [3, 0, 2]                    # tile 1 is left out; the list is in no particular order
# ... of the 30 tiles of the 44 x 36 grids: 17 entries (with four wavefronts to a workgroup, a launch has wavefronts past the list
# at k_split 1 and 2), odd (wild) and even tiles, the corner and both sliver edges listed and left out
LISTED_GRID = [29, 3, 14, 0, 23, 8, 27, 11, 5, 16, 21, 24, 1, 18, 7, 26, 13]


def _bind(L):
    fp, u32p, vp, u32 = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32
    L.ra_error.restype = C.c_char_p
    L.ra_round.argtypes = [vp, vp, u32, C.c_uint64, u32, u32, u32, u32, u32p, fp, fp, fp, fp, C.POINTER(C.c_uint64)]


@pytest.fixture(scope="module")
def adapt_probe():
    return shared("rays_adapt_probe", _bind)


def _round(L, holder, feat, base, n, k_split, tiles, o, d, accum, half, seed=Y.SEED):
    t = np.ascontiguousarray(tiles, np.uint32)
    seg = C.c_uint64(0)
    rc = L.ra_round(*Y._ptrs(holder), feat, seed, base, n, k_split, t.size, _p(t, C.c_uint32), _p(o), _p(d), _p(accum),
                    None if half is None else _p(half), C.byref(seg))
    assert rc == 0, L.ra_error()
    return int(seg.value)


def test_one_round_over_a_tile_list_equals_the_ray_body(adapt_probe):
    """Samples [16, 48) -- two chunks -- of three of the four tiles of a ragged 12 x 10 grid of equirect rays, on top of an
    accumulator that holds chunk 0: direct (k_split 1) and through the planes with the listed reduction (k_split 2, 4) give
    chunk 0 + chunk 1 + chunk 2 of the x86 mrt_radiance body, added in that order in float32; the half buffer receives the same
    two chunk sums; unlisted pixels keep their bytes; the segment totals agree."""
    from micro_raytracer_amd import cameras, scenes
    render, holder = make_holder(Y._sized(scenes.cornell_box(bounce=6), res=GRID, spp=48))
    rays = Y.shared_probe()
    info = Y.x86_info(rays, holder)
    assert (info["nw"], info["nh"]) == GRID
    feat = info["rays_inst"]
    o, d = cameras.equirect(render.frame.cam.pos, *GRID)
    chunk = []
    segs = []
    for j in range(3):
        c, s = Y.x86_radiance(rays, holder, feat, o, d, 16, sample_base=16 * j, segments=True)
        chunk.append(c)
        segs.append(s)
    listed = np.zeros((GRID[1], GRID[0]), bool)
    n_tx = (GRID[0] + 7) // 8
    for t in LISTED:
        ty, tx = divmod(t, n_tx)
        listed[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = True
    assert listed.any() and not listed.all()
    want = np.where(listed[..., None], (chunk[0] + chunk[1]) + chunk[2], chunk[0])
    h0 = np.full_like(chunk[0], f32(0.375))
    want_h = np.where(listed[..., None], (h0 + chunk[1]) + chunk[2], h0)
    # the segments of the listed pixels only: the ray body on those rays alone
    m = listed.reshape(-1)
    seg_listed = sum(Y.x86_radiance(rays, holder, feat, o.reshape(-1, 3)[m], d.reshape(-1, 3)[m], 16, sample_base=16 * j,
                                    key=np.flatnonzero(m), segments=True)[1] for j in (1, 2))
    for k_split in (1, 2, 4):
        acc = chunk[0].copy()
        half = None if k_split == 1 else h0.copy()
        seg = _round(adapt_probe, holder, feat, 16, 32, k_split, LISTED, o, d, acc, half)
        diff = int((Y.bits(acc) != Y.bits(want)).any(-1).sum())
        print(f"k_split {k_split}: {diff} of {acc.shape[0] * acc.shape[1]} pixels differ, {seg} segments against {seg_listed}")
        assert diff == 0
        assert seg == seg_listed
        if half is not None:
            assert Y.same(half, want_h)
    # a launch with more phases than chunks (an even round of one chunk goes through two): the idle phase traces nothing
    acc = chunk[0].copy()
    half = h0.copy()
    _round(adapt_probe, holder, feat, 16, 16, 2, LISTED, o, d, acc, half)
    assert Y.same(acc, np.where(listed[..., None], chunk[0] + chunk[1], chunk[0]))
    assert Y.same(half, np.where(listed[..., None], h0 + chunk[1], h0))


@pytest.mark.parametrize("name", AC.FEAT_NAMES)
def test_one_round_over_a_tile_list_on_a_grid_of_every_feature_set(adapt_probe, oracle_mod, name):
    """The round of the test above -- samples [16, 48) on top of chunk 0, k_split 1, 2 and 4 -- on the 44 x 36 grid of one case per
    feature set of MRT_RAYS_LIST, over 17 of its 30 tiles in no particular order.  Expected, from the x86 mrt_radiance body: the
    accumulator is chunk 0 + chunk 1 + chunk 2 in float32 in that order, word for word, NaN words included; the half buffer
    holds the same fold; unlisted pixels keep their bytes; the segment total is that of the listed rays."""
    case = AC.case(name, oracle_mod)
    _, holder = case.holder()
    o, d = case.o, case.d
    assert len(set(LISTED_GRID)) == len(LISTED_GRID) < AC.N_TILES and LISTED_GRID != sorted(LISTED_GRID) and AC.CORNER in LISTED_GRID
    chunk = [case.x86(16 * j, 16) for j in range(3)]
    listed = AC.tiles_mask(LISTED_GRID)
    assert (listed & case.wild).any() and (~listed & case.wild).any()
    nan_words = int(np.isnan(chunk[1][listed]).sum())
    assert (nan_words > 0) == case.has_nan
    with np.errstate(invalid="ignore"):
        want = np.where(listed[..., None], (chunk[0] + chunk[1]) + chunk[2], chunk[0])
        h0 = np.full_like(chunk[0], f32(0.375))
        want_h = np.where(listed[..., None], (h0 + chunk[1]) + chunk[2], h0)
    m = listed.reshape(-1)
    rays = Y.shared_probe()
    seg_listed = sum(Y.x86_radiance(rays, holder, case.feat, o.reshape(-1, 3)[m], d.reshape(-1, 3)[m], 16, seed=AC.SEED, sample_base=16 * j,
                                    key=np.flatnonzero(m), segments=True)[1] for j in (1, 2))
    for k_split in (1, 2, 4):
        acc = chunk[0].copy()
        half = None if k_split == 1 else h0.copy()
        seg = _round(adapt_probe, holder, case.feat, 16, 32, k_split, LISTED_GRID, o, d, acc, half, seed=AC.SEED)
        diff = int((Y.bits(acc) != Y.bits(want)).any(-1).sum())
        print(f"one round, x86: {name:52s} FEAT {case.feat:4d} k_split {k_split}: {diff} of {m.size} pixels differ ({int(m.sum())} listed, "
              f"{int(case.wild.sum())} wild, {nan_words} NaN words in chunk 1 of the listed), {seg} segments against {seg_listed}")
        assert diff == 0
        assert seg == seg_listed
        if half is not None:
            assert Y.same(half, want_h)


def test_preconditions_of_the_gpu_oracle_tests(oracle_mod):
    """What tests/test_gpu_radiance_adaptive_oracle.py needs in order to say anything, from the x86 mrt_radiance body's sums at 32, 64
    and 96 samples and the numpy rule alone: at the threshold those tests take (the median of the non-NaN tile errors at 32) every
    case has at least two distinct stop counts (but the two of the scene without noise, AC.NOISE_FREE), all three counts occur
    across the table, and a tile with a NaN sum never stops before the cap."""
    seen = {}
    for name in AC.NAMES:
        case = AC.case(name, oracle_mod)
        whole = {n: case.x86(0, n) for n in AC.STOPS}
        chunk = {j: case.x86(16 * j, 16) for j in (0, 2)}
        thr = AC.median_threshold(whole[32], chunk[0])
        counts = AC.rule_counts(whole, chunk, thr)
        hist = {n: int((counts == n).sum()) for n in AC.STOPS}
        nan = AC.nan_tiles(whole[32])
        print(f"stop counts from the x86 sums: {name:52s} threshold {thr:.4f} tiles per count {hist} tiles with a NaN sum {int(nan.sum())}")
        assert sum(hist.values()) == AC.N_TILES, (name, hist)
        if case.noise_free:           # (the one scene of FN | F_BVH: every tile error is exactly 0, nothing runs on)
            assert hist[AC.MIN_SAMPLES] == AC.N_TILES and thr == 0.0, (name, hist, thr)
        else:
            assert sum(v > 0 for v in hist.values()) >= 2, (name, hist)
        assert nan.any() == case.has_nan and np.array_equal(nan, AC.nan_tiles(whole[96])) and (counts[nan] == AC.MAX_SAMPLES).all(), name
        for n, v in hist.items():
            seen[n] = seen.get(n, 0) + v
    assert all(seen[n] > 0 for n in AC.STOPS), seen


def test_header_declares_the_call_and_abi_matches():
    from micro_raytracer_amd import _abi, _lib
    hdr = open(os.path.join(ROOT, "include", "mrt.h")).read()
    assert "int mrt_radiance_adaptive(mrt_ctx *ctx, const mrt_rays_adapt *r, mrt_adapt_info *info" in hdr
    assert "} mrt_rays_adapt;" in hdr and "#define MRT_ABI_VERSION 3u" in hdr
    assert "#define MRT_RAYS_DEVICE 1u" in hdr and _abi.RAYS_DEVICE == 1
    assert "mrt_radiance_adaptive" in _lib.SYMBOLS
    assert [n for n, _ in _abi.RaysAdapt._fields_] == ["orig", "dir", "rule", "flags", "reserved"]
    assert _abi.RaysAdapt.rule.offset == 16 and _abi.RaysAdapt.flags.offset == 48 and _abi.RaysAdapt.reserved.offset == 52


def test_struct_size_is_the_c_compilers(tmp_path):
    from micro_raytracer_amd import _abi
    cc = shutil.which("gcc") or shutil.which("cc") or pytest.skip("no C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "mrt.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(mrt_rays_adapt), sizeof(mrt_adapt), sizeof(mrt_adapt_info)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert sizes == [C.sizeof(_abi.RaysAdapt), C.sizeof(_abi.Adapt), C.sizeof(_abi.AdaptInfo)], sizes


def test_cli_pano_adaptive_rules(capsys):
    from micro_raytracer_amd.__main__ import main
    with pytest.raises(SystemExit):
        main(["scene.json", "--pano-adaptive", "0.1"])
    assert "--pano-adaptive needs --camera equirect" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main(["scene.json", "--camera", "equirect", "--pano-guides", "--denoise", "--denoise-mode", "variance"])
    assert "--pano-adaptive" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main(["scene.json", "--camera", "equirect", "--pano-guides", "--adaptive", "0.1"])
    assert "--pano-adaptive" in capsys.readouterr().err
    for bad in (["--pano-adaptive", "-1"], ["--pano-adaptive", "nan"], ["--pano-adaptive", "0.1", "--step", "24"]):
        with pytest.raises(SystemExit):
            main(["scene.json", "--camera", "equirect", *bad])
        capsys.readouterr()
    # variance mode still needs the guides of the panorama's rays
    with pytest.raises(SystemExit):
        main(["scene.json", "--camera", "equirect", "--pano-adaptive", "0.1", "--denoise", "--denoise-mode", "variance"])
    assert "--pano-guides" in capsys.readouterr().err


class _Fake:
    nw, nh = 8, 4

    def __init__(self):
        self.calls = []

    def create(self, render):
        return self

    def radiance(self, render, o, d, n, info=None):
        self.calls.append(("radiance", o, d, n))
        return np.zeros_like(o)

    def set_accum(self, rgb, n):
        self.calls.append(("set_accum", n))

    def radiance_adaptive(self, render, o, d, threshold, min_samples=32, max_samples=None, step=16):
        self.calls.append(("radiance_adaptive", o, d, threshold, min_samples, max_samples, step))
        return {"samples": 7, "rounds": 2}

    def accum(self):
        self.calls.append(("accum",))
        return np.ones((self.nh, self.nw, 3), f32), 32

    def aov_rays(self, render, o, d, *, wrap_x=False):
        self.calls.append(("aov_rays", o, d, wrap_x))


class _R:
    class rt:
        sample = 64

    class frame:
        class cam:
            pos = [0.0, 0.0, 1.0]


def test_render_equirect_adaptive_calls_radiance_adaptive_once():
    from micro_raytracer_amd import cameras
    s = _Fake()
    info = {}
    rgb = cameras.render_equirect(s, _R, adaptive=dict(threshold=0.25, min_samples=32, step=16), guides=True, info=info)
    names = [c[0] for c in s.calls]
    assert names.count("radiance_adaptive") == 1 and "radiance" not in names and "set_accum" not in names
    ra = next(c for c in s.calls if c[0] == "radiance_adaptive")
    assert ra[3:] == (0.25, 32, 64, 16)
    ar = next(c for c in s.calls if c[0] == "aov_rays")
    assert ar[1] is ra[1] and ar[2] is ra[2] and ar[3] is True          # the guides of the very rays that were sampled
    assert info == {"samples": 7, "rounds": 2} and rgb.shape == (4, 8, 3)
    with pytest.raises(ValueError):
        cameras.render_equirect(_Fake(), _R, adaptive=dict(min_samples=32))
    with pytest.raises(ValueError):
        cameras.render_equirect(_Fake(), _R, adaptive=dict(threshold=0.1, cap=3))


def test_render_equirect_without_adaptive_makes_the_calls_it_made():
    from micro_raytracer_amd import cameras
    s = _Fake()
    cameras.render_equirect(s, _R, n_samples=2)
    assert [c[0] for c in s.calls] == ["radiance", "set_accum"] and s.calls[0][3] == 2 and s.calls[1][1] == 2
