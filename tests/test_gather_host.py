"""Point gathers without a GPU: the x86 build of csrc/mrt_gather.h against a float64 restatement of its direction
contract, the quadrature the set gives, its reduction against numpy bit for bit, the struct layouts, the argument errors that are
refused before a device is touched, probes.py and the CLI's own refusals."""
import ctypes as C

import numpy as np
import pytest

import gather_ref as G

f32 = np.float32
SEED = 0x5DEECE66D1234567
N_DIRS = [1, 63, 64, 65, 130, 65536]
# Bars of the f32 text against float64: four times what the x86 build shows on the cases below (printed by the tests; DESIGN.md §22
# has the figures): 7.67e-7 / 1.44e-7 for a SPHERE component and | |d| - 1 | (the component at n_dirs = 65536, where q = sqrt(1 - z z)
# cancels next to the poles; 3.3e-7 up to 130 directions), 2.97e-7 / 2.80e-7 for HEMI_COS, 1.57e-7 for the frame.
BAR_SPHERE_COMP, BAR_SPHERE_LEN = 3.1e-6, 5.8e-7
BAR_HEMI_COMP, BAR_HEMI_LEN = 1.2e-6, 1.12e-6
BAR_FRAME = 6.3e-7


@pytest.fixture(scope="module")
def probe():
    return G.probe()


def normals():
    """+-x, +-y, +-z, vectors with z = -0.0 and next to (0, 0, -1) / (0, 0, +1), lengths far from 1, and random ones"""
    rng = np.random.default_rng(7)
    fixed = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
             (1, 0, -0.0), (0, 1, -0.0), (-1, 1, -0.0), (1, 0, 0.0), (1e-4, 0, -1), (0, -1e-4, -1), (1e-4, 1e-4, 1), (1e-20, 0, -1),
             (3e-3, -2e-3, -1e-7), (250.0, -10.0, 3.0), (1e-12, 2e-12, -1e-12)]
    return np.concatenate([np.array(fixed, f32), rng.standard_normal((15, 3)).astype(f32)])


def _measure(probe, dist, n_dirs, nrm):
    n = 5 if nrm is None else nrm.shape[0]
    pos = np.zeros((n, 3), f32)
    _, d, _ = G.x86_rays(probe, SEED, 11, n_dirs, dist, 0.0, pos, nrm)
    ref = G.dirs64(SEED, 11, n, n_dirs, dist, nrm)
    d = d.astype(np.float64)
    return d, ref, float(np.abs(d - ref).max()), float(np.abs(np.sqrt((d * d).sum(-1)) - 1.0).max())


@pytest.mark.parametrize("n_dirs", N_DIRS)
def test_sphere_directions_meet_float64(probe, n_dirs):
    _, _, comp, length = _measure(probe, G.SPHERE, n_dirs, None)
    print(f"SPHERE n_dirs {n_dirs}: component error {comp:.3e}, | |d| - 1 | {length:.3e}")
    assert comp <= BAR_SPHERE_COMP and length <= BAR_SPHERE_LEN


@pytest.mark.parametrize("n_dirs", N_DIRS)
def test_hemisphere_directions_meet_float64_and_stay_above_the_surface(probe, n_dirs):
    nrm = normals() if n_dirs < 65536 else normals()[::3]
    d, _, comp, length = _measure(probe, G.HEMI_COS, n_dirs, nrm)
    unit, _, _ = G.frame64(nrm)
    cos = (d * unit[:, None, :]).sum(-1)
    print(f"HEMI_COS n_dirs {n_dirs}: component error {comp:.3e}, | |d| - 1 | {length:.3e}, smallest cosine {cos.min():.3e}")
    assert comp <= BAR_HEMI_COMP and length <= BAR_HEMI_LEN
    assert (cos >= 0.0).all()


def test_frame_is_orthonormal(probe):
    nrm = normals()
    n, t, bt = (v.astype(np.float64) for v in G.x86_frame(probe, nrm))
    n64, t64, bt64 = G.frame64(nrm)
    err = max(float(np.abs(a - b).max()) for a, b in ((n, n64), (t, t64), (bt, bt64)))
    dots = [np.abs((a * b).sum(-1)).max() for a, b in ((n, t), (n, bt), (t, bt))]
    lens = [np.abs(np.sqrt((a * a).sum(-1)) - 1.0).max() for a in (n, t, bt)]
    hand = np.abs(np.cross(t, bt) - n).max()
    print(f"frame: error against float64 {err:.3e}, largest dot {max(dots):.3e}, largest | |v| - 1 | {max(lens):.3e}, | t x bt - n | {hand:.3e}")
    assert max(err, *dots, *lens, hand) <= BAR_FRAME


def test_zero_and_non_finite_normals_give_nan_for_their_point_only(probe):
    nrm = np.array([(0, 0, 1), (0, 0, 0), (np.nan, 0, 1), (np.inf, 0, 0), (0, 1, 0)], f32)
    pos = np.arange(15, dtype=f32).reshape(5, 3)
    o, d, _ = G.x86_rays(probe, SEED, 0, 63, G.HEMI_COS, 0.25, pos, nrm)
    assert np.isnan(d[1:4]).all() and np.isnan(o[1:4]).any(-1).all()
    alone = G.x86_rays(probe, SEED, 0, 63, G.HEMI_COS, 0.25, pos, np.where(np.isfinite(nrm) & (np.abs(nrm).sum(-1, keepdims=True) > 0), nrm, 1).astype(f32))
    for i in (0, 4):
        assert G.same_bits(d[i], alone[1][i]) == 0 and G.same_bits(o[i], alone[0][i]) == 0


def test_keys_origins_and_slices(probe):
    rng = np.random.default_rng(3)
    pos = rng.standard_normal((9, 3)).astype(f32)
    nrm = rng.standard_normal((9, 3)).astype(f32)
    for dist, nm in ((G.SPHERE, None), (G.HEMI_COS, nrm)):
        o, d, k = G.x86_rays(probe, SEED, 0xfffffff0, 65, dist, 0.5, pos, nm)
        assert np.array_equal(k, G.keys_of(0xfffffff0, 0, 9, 65))                  # wraps past 2^32
        along = d if nm is None else np.broadcast_to(G.x86_frame(probe, nm)[0][:, None, :], d.shape)
        assert G.same_bits(o, pos[:, None, :] + along * f32(0.5)) == 0
        o2, d2, k2 = G.x86_rays(probe, SEED, 0xfffffff0, 65, dist, 0.5, pos, nm, first=4, count=3)
        assert G.same_bits(o2, o[4:7]) == 0 and G.same_bits(d2, d[4:7]) == 0 and np.array_equal(k2, k[4:7])
        if nm is None:
            other = G.x86_rays(probe, SEED, 0xfffffff1, 65, dist, 0.5, pos, nm)[1]
            assert G.same_bits(other[:-1], d[1:]) == 0                           # a point's turn follows its key, not its index
        assert G.same_bits(G.x86_rays(probe, SEED + 1, 0xfffffff0, 65, dist, 0.5, pos, nm)[1], d) > 0


# ---- quadrature ------------------------------------------------------------------------------------------------------------------
def test_quadrature_of_a_constant_radiance_in_float64():
    from micro_raytracer_amd import probes
    d = G.dirs64(SEED, 0, 37, 256, G.SPHERE)
    c = 4.0 * np.pi / 256.0 * probes.sh9_basis(d).sum(1)
    print(f"n_dirs 256, 37 rotations: | c_0 - 2 sqrt(pi) | {np.abs(c[:, 0] - 2.0 * np.sqrt(np.pi)).max():.3e}, largest |c_k|, k >= 1: {np.abs(c[:, 1:]).max():.3e}")
    # with the exact Y_0 = 1 / (2 sqrt(pi)) the set integrates a constant exactly; the contract's 9-digit constant is within 1e-9 of it
    assert np.abs(c[:, 0] * (0.5 / np.sqrt(np.pi) / probes.Y0) - 2.0 * np.sqrt(np.pi)).max() <= 1e-14
    assert np.abs(c[:, 0] - 2.0 * np.sqrt(np.pi)).max() <= 1e-8
    assert np.abs(c[:, 1:]).max() <= 2.5e-3
    nrm = normals()
    h = G.dirs64(SEED, 0, nrm.shape[0], 256, G.HEMI_COS, nrm)
    cos = (h * G.frame64(nrm)[0][:, None, :]).sum(-1).mean(1)
    print(f"HEMI_COS n_dirs 256: mean cosine - 2/3 within {np.abs(cos - 2.0 / 3.0).max():.3e}")
    assert np.abs(cos - 2.0 / 3.0).max() <= 1e-3


def test_quadrature_of_the_f32_text(probe):
    """The same through the x86 build, end to end: constant sums of 16 samples, the probe's own directions and reduction"""
    from micro_raytracer_amd import probes
    pos = np.zeros((37, 3), f32)
    _, d, _ = G.x86_rays(probe, SEED, 0, 256, G.SPHERE, 0.0, pos)
    sums = np.broadcast_to(np.array([8.0, 4.0, 16.0], f32), d.shape)
    sh = G.x86_reduce(probe, sums, d, 16, G.SH9).astype(np.float64)
    colour = np.array([0.5, 0.25, 1.0])
    assert np.abs(sh[:, 0] / (2.0 * np.sqrt(np.pi) * colour) - 1.0).max() <= 1e-6
    assert (np.abs(sh[:, 1:]) <= 2.5e-3 * colour).all()
    assert np.array_equal(G.x86_reduce(probe, sums, d, 16, G.MEAN), np.broadcast_to(colour.astype(f32), (37, 3)))
    irr = probes.sh9_irradiance(sh, np.array([0.0, 0.0, 1.0]))
    assert np.abs(irr / (np.pi * colour) - 1.0).max() <= 4e-3               # band 1 and 2 leak at most 2.5e-3 x their factors


# ---- reduction -------------------------------------------------------------------------------------------------------------------
def crafted_sums(n_points, n_dirs, rng):
    s = (rng.standard_normal((n_points, n_dirs, 3)) * 10.0 ** rng.uniform(-30, 30, (n_points, n_dirs, 1))).astype(f32)
    s[0] = rng.uniform(0, 4, (n_dirs, 3)).astype(f32)                       # an ordinary point
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.0e38, -3.0e38, 1e-45], f32)
    for pt in range(1, n_points):
        idx = rng.integers(0, n_dirs, 3)
        s[pt, idx, rng.integers(0, 3, 3)] = rng.choice(special, 3)
    s[1] = -0.0                                                             # every term -0: the answer is +0 * scale
    s[4, 0, 1], s[5, 0, 2] = np.nan, -np.inf
    if n_points > 2:
        s[2, :, 0] = np.inf
    return s


@pytest.mark.parametrize("out", [G.MEAN, G.SH9])
@pytest.mark.parametrize("n_dirs", [1, 63, 64, 65, 130])
def test_reduction_equals_numpy_bit_for_bit(probe, n_dirs, out):
    rng = np.random.default_rng(100 * n_dirs + out)
    n_points = 12
    sums = crafted_sums(n_points, n_dirs, rng)
    _, d, _ = G.x86_rays(probe, SEED, 5, n_dirs, G.SPHERE, 0.0, np.zeros((n_points, 3), f32))
    d[3] = np.nan                                                           # the directions of a point with a broken normal
    for n_samples in (16, 17):
        got, ref = G.x86_reduce(probe, sums, d, n_samples, out), G.reduce(sums, d, n_samples, out)
        assert G.same_bits(got, ref) == 0, (n_samples, np.argwhere(got.view(np.uint32) != ref.view(np.uint32))[:4])
        assert np.isfinite(got[0]).all() and (out == G.SH9 or (got[1].view(np.uint32) == 0).all())
        assert np.isnan(got).any() and np.isinf(got).any()


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_python_mirrors_the_struct_layouts(probe):
    from micro_raytracer_amd import _abi
    w = np.zeros(6, np.uint32)
    probe.gp_layout(w.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert list(w) == [C.sizeof(_abi.Gather), _abi.Gather.n_dirs.offset, _abi.Gather.reserved.offset, C.sizeof(_abi.GatherInfo),
                       _abi.GatherInfo.rays.offset, _abi.GatherInfo.lds_bytes.offset]


def test_null_arguments_are_refused_before_the_device_is_touched():
    from micro_raytracer_amd import _abi, _lib
    L = _lib.lib()
    g = _abi.Gather()
    out = np.zeros(3, f32)
    assert L.mrt_gather(None, C.byref(g), out.ctypes.data, None) == _abi.MRT_ERR_ARG
    assert b"mrt_gather: null" in L.mrt_last_error() and L.mrt_last_status() == _abi.MRT_ERR_ARG
    assert L.mrt_gather(None, None, out.ctypes.data, None) == _abi.MRT_ERR_ARG
    assert L.mrt_gather_rays(None, C.byref(g), 0, 0, None, None, None) == _abi.MRT_ERR_ARG
    assert b"mrt_gather_rays: null" in L.mrt_last_error()
    assert {"mrt_gather", "mrt_gather_rays"} <= set(_lib.SYMBOLS)


def test_sampler_refuses_an_unknown_output_without_a_context():
    from micro_raytracer_amd import Sampler
    with pytest.raises(ValueError, match="sh4"):
        Sampler()._gather_desc("gather", np.zeros((2, 3), f32), None, 64, 16, "sh4", 0, 1e-4, 0, 0)
    keep, g, dev = Sampler()._gather_desc("gather", np.zeros((2, 5, 3)), np.ones((2, 5, 3)), 7, 3, "mean", -1, 0.5, 2, 4)
    assert (g.n, g.n_dirs, g.n_samples, g.sample_base, g.dist, g.out, g.key_base, g.batch_points, g.flags, dev) == \
        (10, 7, 3, 2, _hemi(), 0, 0xffffffff, 4, 0, False)
    assert g.pos == keep[0].ctypes.data and g.normal == keep[1].ctypes.data and keep[0].dtype == f32


def _hemi():
    from micro_raytracer_amd import _abi
    return _abi.GATHER_HEMI_COS


# ---- probes.py and the CLI -------------------------------------------------------------------------------------------------------
def test_probes_module():
    from micro_raytracer_amd import probes
    rng = np.random.default_rng(1)
    d = rng.standard_normal((4000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # the basis is orthonormal over the sphere (Monte Carlo, 4000 directions: ~ 1 / sqrt(4000) x a few)
    gram = 4.0 * np.pi * probes.sh9_basis(d).T @ probes.sh9_basis(d) / 4000
    assert np.abs(gram - np.eye(9)).max() < 0.12
    assert np.allclose(probes.sh9_basis(d), G.sh9_f32(d.astype(f32)), atol=1e-6)
    # a radiance that is a band-limited function is returned by its own coefficients
    sh = rng.standard_normal((9, 3))
    assert np.allclose(probes.sh9_eval(sh, d), probes.sh9_basis(d) @ sh)
    # E(n) = integral of L(w) max(0, n.w): for L = a + b (w.m) it is pi a + (2 pi / 3) b (n.m)
    m, n = np.array([0.0, 0.6, 0.8]), np.array([1.0, 0.0, 0.0])
    sh = np.zeros((9, 3))
    sh[0] = 2.0 / probes.Y0
    sh[[3, 1, 2]] = (0.5 * m / probes.Y1)[:, None]
    assert np.allclose(probes.sh9_irradiance(sh, n), np.pi * 2.0 + 2.0 * np.pi / 3.0 * 0.5 * (n @ m))
    pos, nrm = probes.lightmap_grid((-1, -1, 0), (2, 0, 0), (0, 4, 0), 4, 2)
    assert pos.shape == nrm.shape == (2, 4, 3) and pos.dtype == nrm.dtype == f32
    assert np.array_equal(pos[0, 0], f32([-0.75, 0.0, 0.0])) and np.array_equal(pos[1, 3], f32([0.75, 2.0, 0.0]))
    assert (nrm == f32([0, 0, 1])).all()
    with pytest.raises(ValueError):
        probes.lightmap_grid((0, 0, 0), (1, 0, 0), (2, 0, 0), 2, 2)


@pytest.mark.parametrize("argv", [["x.json", "--gather", "p.npy"], ["x.json", "--gather-out", "o.npy"], ["x.json", "--gather-sh"],
                                  ["x.json", "--gather-dirs", "8"]])
def test_cli_refuses_half_a_gather(argv, capsys):
    from micro_raytracer_amd import __main__ as cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2 and "--gather" in capsys.readouterr().err
