"""Adaptive sampling without a GPU: the stop rule of csrc/mrt_adapt.h (compiled for x86) against a numpy float32
restatement, bit for bit; the C ABI's argument handling; the header; the CLI's argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from emu.build import shared

f32 = np.float32


def _bind(L):
    fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    L.adapt_pixel_errors.argtypes = [fp, fp, C.c_uint32, C.c_uint32, C.c_uint32, fp]
    L.adapt_tile_errors.argtypes = [fp, fp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, fp, u32p, u32p]


@pytest.fixture(scope="module")
def probe():
    return shared("adapt_probe", _bind, with_pack=False)


def np_pixel_errors(A, H, n):
    """The formula of the issue / DESIGN.md, in float32, in its operation order."""
    rc = f32(1.0) / f32(n)
    rh = f32(1.0) / f32(n // 2)
    with np.errstate(invalid="ignore", over="ignore"):
        I = A * rc
        J = H * rh
        num = (np.abs(I[..., 0] - J[..., 0]) + np.abs(I[..., 1] - J[..., 1])) + np.abs(I[..., 2] - J[..., 2])
        den = f32(1e-4) + np.sqrt((I[..., 0] + I[..., 1]) + I[..., 2])
        return (num / den).astype(f32)


def np_tile_errors(A, H, n, thr):
    e = np_pixel_errors(A, H, n)
    nh, nw = e.shape
    n_ty, n_tx = (nh + 7) // 8, (nw + 7) // 8
    et = np.zeros((n_ty, n_tx), f32)
    nan = np.zeros((n_ty, n_tx), bool)
    for ty in range(n_ty):
        for tx in range(n_tx):
            t = e[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]
            nan[ty, tx] = np.isnan(t).any()
            ok = t[~np.isnan(t)]
            et[ty, tx] = ok.max() if ok.size else f32(0)
    return et, nan, ~nan & (et <= f32(thr))


def _frames(rng, nh, nw, n):
    """A, H sums of n and n/2 samples with all-zero pixels, very large radiance, NaN and infinities mixed in."""
    mean = rng.gamma(0.6, 0.3, size=(nh, nw, 3)).astype(f32)
    A = (mean * f32(n)).astype(f32)
    H = (A * f32(0.5) * rng.uniform(0.7, 1.3, size=A.shape).astype(f32)).astype(f32)
    A[0:8, 0:8] = 0.0
    H[0:8, 0:8] = 0.0                                    # an all-black tile: error exactly 0
    A[3, 20] = 0.0                                       # a black pixel next to lit ones (H may be nonzero there)
    A[9, 9] = 3e38; H[9, 9] = 1e38                        # very large radiance, finite
    A[10, 17] = 3.3e38; H[10, 17] = 1.0                 # huge means against a tiny half
    A[12, 3, 2] = np.float32(np.inf)                     # inf - inf -> NaN
    H[12, 3, 2] = np.float32(np.inf)
    A[nh - 1, nw - 1, 0] = np.nan                        # NaN in a partial edge tile
    H[17, 30, 2] = np.nan
    A[20, 5] = 1e-30; H[20, 5] = 1e-30                  # denormal means
    return A, H


@pytest.mark.parametrize("nh,nw,n", [(21, 37, 32), (64, 64, 96), (24, 33, 2048), (40, 45, 4294967264)])
def test_stop_rule_matches_numpy_bit_for_bit(probe, nh, nw, n):
    rng = np.random.default_rng(nh * 1000 + nw)
    A, H = _frames(rng, nh, nw, n)
    e = np.empty((nh, nw), f32)
    fp = C.POINTER(C.c_float)
    probe.adapt_pixel_errors(A.ctypes.data_as(fp), H.ctypes.data_as(fp), nw, nh, n, e.ctypes.data_as(fp))
    ref = np_pixel_errors(A, H, n)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(e), nan)              # (NaN payloads are not part of the rule)
    assert np.array_equal(e[~nan].view(np.uint32), ref[~nan].view(np.uint32))
    assert np.isnan(e).any() and (e == 0).any() and np.isinf(e).sum() + np.isnan(e).sum() > 1
    n_ty, n_tx = (nh + 7) // 8, (nw + 7) // 8
    for thr in (0.0, 0.05, 0.3, float("inf")):
        et = np.empty((n_ty, n_tx), f32)
        nan = np.empty((n_ty, n_tx), np.uint32)
        conv = np.empty((n_ty, n_tx), np.uint32)
        probe.adapt_tile_errors(A.ctypes.data_as(fp), H.ctypes.data_as(fp), nw, nh, n, thr, et.ctypes.data_as(fp),
                                nan.ctypes.data_as(C.POINTER(C.c_uint32)), conv.ctypes.data_as(C.POINTER(C.c_uint32)))
        ret, rnan, rconv = np_tile_errors(A, H, n, thr)
        assert np.array_equal(et.view(np.uint32), ret.view(np.uint32))
        assert np.array_equal(nan.astype(bool), rnan)
        assert np.array_equal(conv.astype(bool), rconv), thr
        assert not conv[rnan].any()                       # a NaN pixel never lets its tile stop
    assert conv[0, 0] == 1                                 # (thr = inf) the black tile; and at thr = 0 too:
    _, _, c0 = np_tile_errors(A, H, n, 0.0)
    assert c0[0, 0]


def test_adaptive_entry_points_without_device():
    from micro_raytracer_amd import _abi, _lib
    L = _lib.lib()
    a = _abi.Adapt(32, 128, 16, 0.1)
    assert L.mrt_execute_adaptive(None, C.byref(a), None, None) == _abi.MRT_ERR_ARG
    assert L.mrt_execute_adaptive(None, None, None, None) == _abi.MRT_ERR_ARG
    assert L.mrt_sample_counts(None, None) == _abi.MRT_ERR_ARG
    assert L.mrt_adapt_half(None, None) == _abi.MRT_ERR_ARG
    assert "null" in L.mrt_last_error().decode()


def test_header_declares_adaptive_abi():
    from micro_raytracer_amd import _abi, _lib
    hdr = open(os.path.join(ROOT, "include", "mrt.h")).read()
    for name in ("mrt_execute_adaptive", "mrt_sample_counts", "mrt_adapt_half"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SYMBOLS
    assert "typedef struct mrt_adapt {" in hdr and "} mrt_adapt_info;" in hdr
    assert C.sizeof(_abi.Adapt) == 32
    assert C.sizeof(_abi.AdaptInfo) == 8 + 6 * 4 + 8              # u64, six u32, double
    assert _abi.AdaptInfo.kernel_ms.offset == 32
    assert re.search(r"#define MRT_ABI_VERSION 3u", hdr)


@pytest.mark.parametrize("argv", [["--adaptive", "0.1", "--update"], ["--adaptive", "0.1", "--step", "24"],
                                  ["--adaptive", "-1"]])
def test_cli_rejects_bad_adaptive_arguments_before_any_device(argv, monkeypatch, capsys):
    from micro_raytracer_amd import __main__ as cli

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(cli, "Sampler", no_device)
    monkeypatch.setattr(cli, "load_render", no_device)
    with pytest.raises(SystemExit) as e:
        cli.main(["does-not-exist.json"] + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "adaptive" in err or "step" in err
