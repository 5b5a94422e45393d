"""mrt_radiance without a GPU: the per-ray body of csrc/mrt_rays.h, built for x86 (tests/emu/rays_probe.cpp).  The camera's own rays
reproduce the frame bit for bit; rays no pinhole forms meet the float64 core; keys and sample ranges compose; cameras.equirect
is what it documents."""
import numpy as np
import pytest

import core_cases as K
import env_ref as E
import rays_ref as Y

f32 = np.float32


@pytest.fixture(scope="module")
def probe():
    return Y.shared_probe()


def _check(got, ref, spp):
    """The oracle's bar on accumulators (tests/test_fuzz_scenes.py): 1e-4 of the mean, scaled by the brightest mean above 1."""
    assert (np.isnan(got) == np.isnan(ref)).all()
    fin = np.isfinite(ref)
    scale = max(1.0, float(np.abs(ref[fin]).max()) / spp)
    worst = float(np.abs(got[fin] - ref[fin]).max()) / spp
    print(f"worst difference of the means against the oracle {worst:.2e} (bar {1e-4 * scale:.1e})")
    assert worst <= 1e-4 * scale


@pytest.mark.parametrize("name", ["cornell", "lights", "primitives", "env_vattr"])
def test_camera_rays_reproduce_the_frame(probe, oracle_mod, name):
    """The x86 camera rays through the x86 ray body at 40 samples: the bits of the x86 frame render (render_pixel under its camera
    policy), through the scene's own feature set and through the covering one pt_rays runs; within the oracle's bar."""
    render, holder = Y.frame_case(name)
    info = Y.x86_info(probe, holder)
    assert (info["nw"], info["nh"]) == Y.RES and render.frame.cam.aprt == 0
    if name == "cornell":
        assert info["axis_scan"] == 1 and info["own_inst"] == Y.F_IDENT          # planes and spheres: the frame takes the axis scan
    if name == "env_vattr":
        assert info["rays_inst"] == Y.F_ALL | Y.F_VATTR | Y.F_ENV
    frame = E.x86_render(E.shared_probe(), holder, Y.SEED, Y.SPP)
    o, d = Y.x86_camera_rays(probe, holder)
    for feat in sorted({info["own_inst"], info["rays_inst"]}):
        got = Y.x86_radiance(probe, holder, feat, o, d, Y.SPP)
        diff = int((Y.bits(got) != Y.bits(frame)).any(-1).sum())
        print(f"rays {name} FEAT {feat}: {diff} of {got.shape[0] * got.shape[1]} pixels differ from the x86 frame")
        assert diff == 0
    orc = oracle_mod.Oracle(holder, seed=Y.SEED)
    orc.execute(Y.SPP, threads=8)
    ref = orc.accum()[0].copy()
    orc.close()
    _check(frame, ref, Y.SPP)


@pytest.mark.parametrize("name", list(Y.WINDOWS))
def test_window_rays_against_float64(probe, name):
    """A 96 x 40 lat-long window from the scene's camera position, elevations off the floor's horizon: the mean of two samples
    under core_cases.compare_image unchanged, against core_ref.render_image on the same rays."""
    render, holder, o, d, ref, img32 = Y.window_case(name)
    feat = Y.x86_info(probe, holder)["rays_inst"]
    one = Y.x86_radiance(probe, holder, feat, o, d, 1, seed=1)
    two = Y.x86_radiance(probe, holder, feat, o, d, 2, seed=1)
    det = ~ref["random"]
    assert np.array_equal(Y.bits(one + one)[det], Y.bits(two)[det])
    K.compare_image(f"x86 rays window {name}", two / f32(2), ref, img32)


def test_keys_and_sample_ranges(probe):
    """On the Cornell box, whose every path scatters at random: a ray's key, not its place in the batch, seeds it; sample ranges
    that end on chunk boundaries add up to the whole range bit for bit."""
    render, holder = Y.frame_case("cornell")
    feat = Y.x86_info(probe, holder)["rays_inst"]
    o, d = (a.reshape(-1, 3) for a in Y.x86_camera_rays(probe, holder))
    n = o.shape[0]
    whole = Y.x86_radiance(probe, holder, feat, o, d, 32)
    assert Y.same(Y.x86_radiance(probe, holder, feat, o, d, 32, key=np.arange(n)), whole)
    rev = Y.x86_radiance(probe, holder, feat, o[::-1], d[::-1], 32, key=np.arange(n)[::-1])
    assert Y.same(rev[::-1], whole)
    assert not Y.same(Y.x86_radiance(probe, holder, feat, o[::-1], d[::-1], 32)[::-1], whole)      # the key, not the position, seeds a ray
    a = Y.x86_radiance(probe, holder, feat, o, d, 16)
    b = Y.x86_radiance(probe, holder, feat, o, d, 16, sample_base=16)
    assert Y.same(a + b, whole) and not Y.same(a, b)


def test_equirect_is_what_it_documents():
    from micro_raytracer_amd import cameras
    pos = [0.3, -1.2, 0.7]
    o, d = cameras.equirect(pos, 64, 32)
    assert o.dtype == f32 and d.dtype == f32 and o.shape == d.shape == (32, 64, 3)
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1.0).max() <= 2.0 ** -23
    assert np.array_equal(o, np.asarray(pos, f32) + d * f32(0.0001))
    # the two centre columns straddle +y; azimuth grows towards +x; row 0 is the upper elevation; a row has one elevation
    mid = d[:, 31:33].astype(np.float64)
    assert (mid[..., 1] > 0).all() and np.allclose(mid[:, 0, 0], -mid[:, 1, 0]) and (mid[:, 1, 0] > 0).all()
    assert (np.diff(d[:, 0, 2].astype(np.float64)) < 0).all() and d[0, 0, 2] > 0.99 and d[-1, 0, 2] < -0.99
    assert np.abs(d[..., 2] - d[:, :1, 2]).max() <= 2.0 ** -23
    el = np.degrees(np.arcsin(d[:, 0, 2].astype(np.float64)))
    assert np.allclose(el, 90.0 - (np.arange(32) + 0.5) * 180.0 / 32, atol=1e-4)
    # yaw in turns: a quarter turn brings the centre to +x; a window keeps its elevations
    _, q = cameras.equirect(pos, 64, 32, yaw=0.25)
    assert np.allclose(q[16, 31:33, 0].astype(np.float64).mean(), np.cos(np.radians(90.0 - 16.5 * 180 / 32)) * np.cos(np.pi / 64), atol=1e-6)
    assert (q[:, 31:33, 0] > 0).all() and np.allclose(q[:, 31, 1], -q[:, 32, 1], atol=1e-7)
    _, w = cameras.equirect(pos, 96, 40, elevation=(-80.0, -25.0))
    elw = np.degrees(np.arcsin(w[:, 5, 2].astype(np.float64)))
    assert np.allclose(elw, -25.0 - (np.arange(40) + 0.5) * 55.0 / 40, atol=1e-4)
