"""The linear float image on the device (mrt_img_hdr): crafted accumulators put in with mrt_set_accum against the
numpy restatement of tests/hdr_ref.py, bit for bit, for both filters; per-tile counts after an adaptive render; the denoised
source; state and argument errors; and the probe loop -- a panorama saved as .hdr lights a second scene."""
import ctypes as C

import numpy as np
import pytest

import hdr_ref as H
from conftest import make_holder

pytestmark = pytest.mark.gpu
f32 = np.float32


def _sampler(res, ssaa, **kw):
    from micro_raytracer_amd import Sampler
    render, _ = make_holder(H.desc(res, ssaa))
    return Sampler(seed=1, device=0, **kw).create(render), render


# ---- crafted frames ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,ssaa", H.SHAPES, ids=lambda v: str(v))
def test_crafted_frames_equal_the_restatement(oracle_mod, res, ssaa):
    s, _ = _sampler(res, ssaa)
    nw, nh = H.ss_dims(res, ssaa)
    assert (s.nw, s.nh) == (nw, nh)
    resized = (nw, nh) != tuple(res)
    for name, sums, count in H.contents(nh, nw, seed=nw * 7 + nh):
        s.set_accum(sums, count)
        before = s.img()
        m = H.mean(sums, count)
        for filt in H.FILTERS:
            want = H.img_hdr(oracle_mod, m, res, filt)
            info = {}
            got = s.img_hdr(filter=filt, info=info)
            bad = got.view(np.uint32) != want.view(np.uint32)
            print(f"{res} ssaa {ssaa} {name} {filt}: {int(bad.sum())} words differ, resize_ms {info['resize_ms']:.4f}")
            assert got.shape == (res[1], res[0], 3) and not bad.any(), (name, filt, np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])
            assert info["resize_ms"] > 0
        if name == "spike" and resized and ssaa > 1:       # the clamp and the box claim are exercised
            assert H.img_hdr(oracle_mod, m, res, "lanczos3", pre_clamp=True).min() < 0
            assert H.img_hdr(oracle_mod, m, res, "box", pre_clamp=True).min() >= 0
        if not resized and name != "nan":                  # non-negative sums, no resize: the means of mrt_denoise(passes = 0)
            assert H.same(s.img_hdr(), s.denoise(passes=0)) and H.same(s.img_hdr(filter="box"), s.denoise(passes=0))
        # an observation: the accumulator, its count and the 8-bit image are as before
        acc, cnt = s.accum()
        assert H.same(acc, sums) and cnt == count and np.array_equal(s.img(), before)
    s.close()


# ---- per-tile counts -------------------------------------------------------------------------------------------------------------
AD_MIN, AD_MAX, AD_STEP, AD_SEED = 32, 128, 16, 5


def _threshold(render):
    """As tests/test_image_path.py chooses its own: a quantile of the tile errors at AD_MIN"""
    from micro_raytracer_amd import Sampler
    from test_adaptive_host import np_tile_errors
    s = Sampler(seed=AD_SEED, device=0)
    s.execute_adaptive(render, float("inf"), min_samples=AD_MIN, max_samples=AD_MAX, step=AD_STEP)
    et, nan, _ = np_tile_errors(s.accum()[0], s.adapt_half(), AD_MIN, 0.0)
    s.close()
    return float(np.quantile(et[~nan], 0.5))


def test_adaptive_render_uses_per_tile_counts(oracle_mod):
    from micro_raytracer_amd import Sampler, scenes
    res = (24, 24)
    render, _ = make_holder(scenes.cornell_box(res=res, ssaa=2, sample=AD_MAX, bounce=8))
    s = Sampler(seed=AD_SEED, device=0)
    info = s.execute_adaptive(render, _threshold(render), min_samples=AD_MIN, max_samples=AD_MAX, step=AD_STEP)
    assert info["min_count"] != info["max_count"], info          # else the test is void
    sums, counts = s.accum()[0], s.sample_counts()
    m = H.mean(sums, counts)
    assert not H.same(m, H.mean(sums, int(counts.min())))
    for filt in H.FILTERS:
        assert H.same(s.img_hdr(filter=filt), H.img_hdr(oracle_mod, m, res, filt)), filt
    assert np.array_equal(s.sample_counts(), counts) and H.same(s.accum()[0], sums)
    s.close()


def test_consumers_of_one_accumulator_agree_on_every_count():
    """Tone map, denoiser, float image and mrt_sample_counts read one frame of sums through one statement of a pixel's 1/count
    (csrc/mrt_adapt.h MeanSrc): on a 13x11 frame -- 2x2 tiles, the right column 5 pixels wide, the bottom row 3 high -- whose
    tiles stop at different counts they give the same means, bit for bit.  Threshold 0.35: on the x86 build (tests/emu render,
    np_tile_errors) the tile errors are 0.451, 0.327, 0.486, 0.436 at 64 samples and 0.403, -, 0.397, 0.272 at 96, none below
    0.45 at 32: counts 128, 64, 128, 96."""
    from micro_raytracer_amd import Sampler, scenes
    render, _ = make_holder(scenes.cornell_box(res=(13, 11), sample=AD_MAX, bounce=8))
    s = Sampler(seed=AD_SEED, device=0)
    s.execute_adaptive(render, 0.35, min_samples=AD_MIN, max_samples=AD_MAX, step=AD_STEP)
    assert (s.nw, s.nh) == (13, 11)
    sums, counts = s.accum()[0], s.sample_counts()
    print("tile counts", counts[::8, ::8].tolist())
    assert counts.shape == (11, 13) and len(np.unique(counts)) >= 2, np.unique(counts)
    for ty in range(2):                                           # one count per 8x8 tile, the partial ones included
        for tx in range(2):
            assert len(np.unique(counts[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8])) == 1
    mean = sums * (f32(1.0) / counts.astype(f32))[..., None]
    assert mean.dtype == f32
    assert H.same(s.denoise(passes=0), mean)
    hdr = s.img_hdr()
    assert H.same(hdr, np.where(mean > 0, mean, f32(0.0)))
    assert H.same(s.img_hdr(filter="box"), hdr)                   # no resize: the filter does not matter
    assert np.array_equal(s.img_ss(), s.img_denoised(passes=0))
    assert np.array_equal(s.img(), s.img_ss())                    # output size = supersampled size
    s.close()


# ---- the denoised source -----------------------------------------------------------------------------------------------------------
def test_denoised_source(oracle_mod):
    from micro_raytracer_amd import Sampler, scenes
    res = (32, 32)
    render, _ = make_holder(scenes.cornell_box(res=res, ssaa=2, sample=16, bounce=8))
    s = Sampler(seed=2, device=0)
    s.execute(render, n_samples=16)
    for filt in H.FILTERS:
        info = {}
        got = s.img_hdr(filter=filt, denoise={"passes": 2}, info=info)
        assert H.same(got, H.img_hdr(oracle_mod, s.denoise(passes=2), res, filt)), filt
        assert info["passes"] == 2 and info["filter_ms"] > 0 and info["resize_ms"] > 0
        plain = s.img_hdr(filter=filt)
        assert H.same(s.img_hdr(filter=filt, denoise={"passes": 0}), plain) and not H.same(got, plain)
    sums, cnt = s.accum()
    assert cnt == 16 and H.same(s.img_hdr(), H.img_hdr(oracle_mod, H.mean(sums, 16), res, "lanczos3"))
    s.close()


# ---- state and arguments -----------------------------------------------------------------------------------------------------------
def test_state_and_argument_errors():
    from micro_raytracer_amd import MrtError, Sampler, _abi, _lib
    L = _lib.lib()
    res, ssaa = (12, 8), 2.0
    s, render = _sampler(res, ssaa)
    with pytest.raises(MrtError) as e:
        s.img_hdr()
    assert e.value.code == _abi.MRT_ERR_STATE and "mrt_img_hdr" in e.value.msg and "no samples" in e.value.msg
    with pytest.raises(MrtError) as e:
        s.img_hdr(denoise={"passes": 1})
    assert e.value.code == _abi.MRT_ERR_STATE
    s.execute(render)
    out = np.zeros((res[1], res[0], 3), f32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    assert L.mrt_img_hdr(s._ctx, None, fp, None) == 0 and H.same(out, s.img_hdr())          # NULL options: Lanczos3 of the means

    def call(edit, rgb=fp):
        o = _abi.HdrOpts()
        edit(o)
        return L.mrt_img_hdr(s._ctx, C.byref(o), rgb, None)

    assert call(lambda o: None) == 0
    assert call(lambda o: setattr(o, "filter", 2)) == _abi.MRT_ERR_ARG and "filter" in L.mrt_last_error().decode()
    assert call(lambda o: setattr(o, "filter", 0xffffffff)) == _abi.MRT_ERR_ARG
    assert call(lambda o: setattr(o, "reserved0", 1)) == _abi.MRT_ERR_ARG
    for k in range(4):
        def edit(o, k=k):
            o.reserved[k] = 7
        assert call(edit) == _abi.MRT_ERR_ARG and "reserved" in L.mrt_last_error().decode()
    assert call(lambda o: None, None) == _abi.MRT_ERR_ARG
    with pytest.raises(MrtError) as e:                                  # denoise options mrt_denoise would refuse
        s.img_hdr(denoise={"passes": 9})
    assert e.value.code == _abi.MRT_ERR_ARG
    with pytest.raises(ValueError):
        s.img_hdr(filter="cubic")
    assert s.accum()[1] == 1                                            # the refused calls left the context as it was
    s.close()

    # a sharded context holds only its own rows until the whole frame is put in
    sh, render = _sampler(res, ssaa, shard_index=0, shard_count=2)
    sh.execute(render)
    with pytest.raises(MrtError) as e:
        sh.img_hdr()
    assert e.value.code == _abi.MRT_ERR_STATE and "own rows" in e.value.msg
    full = np.full((sh.nh, sh.nw, 3), 0.5, f32)
    sh.set_accum(full, 2)
    assert (sh.img_hdr(filter="box") == f32(0.25)).all()
    sh.close()


def test_booked_samples_are_traced_first():
    from micro_raytracer_amd import Sampler, _abi, scenes
    render, _ = make_holder(scenes.cornell_box(res=(12, 8), ssaa=2, sample=2))       # a lit scene: the image is not black
    d = Sampler(seed=1, device=0, flags=_abi.FLAG_DEFER).create(render)
    d.execute(render)
    d.execute(render)                                                   # both only booked: nothing has observed the context yet
    got = d.img_hdr()                                                   # without the booked samples: MRT_ERR_STATE, no samples
    assert d.stats()["deferred"] == 1 and d.accum()[1] == 2
    e = Sampler(seed=1, device=0)
    e.execute(render, n_samples=2)
    assert H.same(d.accum()[0], e.accum()[0]) and H.same(got, e.img_hdr()) and got.max() > 0
    d.close()
    e.close()


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------
def test_cli_writes_float_outputs(tmp_path):
    """--camera equirect -o probe.hdr writes a panorama that --sky-tex loads; -o out.pfm holds Sampler.img_hdr's floats, with
    --resize box, --update and --denoise as well."""
    import json
    from micro_raytracer_amd import Sampler, __main__ as cli, load_render, scenes
    from micro_raytracer_amd.scene import read_hdr
    desc = scenes.cornell_box(res=(24, 12), ssaa=2, sample=4)
    path = tmp_path / "box.json"
    path.write_text(json.dumps(desc))
    probe = tmp_path / "probe.hdr"
    cli.main([str(path), "-o", str(probe), "--camera", "equirect", "--resize", "box", "--seed", "3"])
    tex = read_hdr(str(probe))
    assert (tex.w, tex.h) == (24, 12) and tex.dat.max() > 0
    render = load_render(desc)
    for extra, kw in (([], {}), (["--resize", "box"], {"filter": "box"}), (["--update"], {}),
                      (["--denoise", "--denoise-passes", "2"], {"denoise": {"passes": 2}})):
        out = tmp_path / "out.pfm"
        cli.main([str(path), "-o", str(out), "--seed", "3", "--sky-tex", str(probe), "--sky-map", "latlong", *extra])
        lit = load_render(desc)
        lit.scene.sky.tex, lit.scene.sky.mapping = read_hdr(str(probe)), "latlong"
        s = Sampler(seed=3)
        if "--update" in extra:                                         # the CLI's per-sample loop
            for _ in range(4):
                s.execute(lit)
        else:
            s.execute(lit, n_samples=4)
        assert H.same(H.read_pfm(out), s.img_hdr(**kw)), extra
        s.close()
    assert render.scene.sky.tex is None


# ---- the probe loop ----------------------------------------------------------------------------------------------------------------
def test_a_saved_panorama_lights_another_scene(tmp_path):
    from micro_raytracer_amd import Sampler, _lib, cameras, load_render, scenes
    from micro_raytracer_amd.scene import read_hdr
    res = (32, 16)
    d = scenes.env_scene(res=res, sample=4, tex_res=(64, 32))
    d["frame"]["ssaa"] = 1
    render = load_render(d)
    s = Sampler(seed=7, device=0)
    cameras.render_equirect(s, render)
    pano = s.img_hdr(filter="box")
    assert pano.shape == (16, 32, 3) and pano.max() > 1.0              # a primary miss returns the sky texel: u8 would clip it
    assert H.same(pano, H.clamp(H.mean(*s.accum())))
    s.close()
    path = tmp_path / "probe.hdr"
    _lib.save_image_f32(path, pano)
    tex = read_hdr(str(path))
    assert (tex.w, tex.h) == (32, 16)
    texels = tex.dat.reshape(16, 32, 3)
    v = pano.max(-1, keepdims=True).astype(np.float64)
    assert (np.abs(texels.astype(np.float64) - pano) <= v / 256).all()
    assert H.same(texels, H.rgbe_decode(H.rgbe_encode(pano)))

    # scene B: nothing but a small sphere below the camera, under the loaded panorama (lat-long, nearest texel)
    color = np.array([0.5, 1.0, 0.25], f32)
    b = H.desc((8, 8))
    b["scene"]["renderer"][0]["pos"] = [0, 0, -50]
    b["scene"]["sky"] = {"color": color.tolist(), "pwr": 1.0, "tex": {"w": tex.w, "h": tex.h, "dat": tex.dat.tolist()}, "map": "latlong", "rot": 0.0}
    rb = load_render(b)
    assert rb.scene.sky.tex is not None and rb.scene.sky.mapping == "latlong" and rb.scene.sky.filter == "nearest"
    cols, rows = np.array([0, 5, 11, 16, 21, 26, 30, 31]), np.array([0, 2, 4, 6, 7, 9, 12, 14])   # eight pixel centres, all above the sphere
    o, dirs = cameras.equirect(rb.frame.cam.pos, 32, 16)
    rays_o, rays_d = o[rows, cols], dirs[rows, cols]
    # the texel each ray looks up, by the lat-long mapping of the sky in float64: u = 0.5 + atan2(d.x, -d.y) / 2pi, v = acos(d.z) / pi.
    # u runs against the panorama's azimuth, so column x reads texel column (15 - x) mod 32 of its own row -- at the texel's centre.
    dd = rays_d.astype(np.float64)
    u, v = (0.5 + np.arctan2(dd[:, 0], -dd[:, 1]) / (2 * np.pi)) % 1.0 * 32, np.arccos(dd[:, 2]) / np.pi * 16
    assert (np.abs(u % 1 - 0.5) < 1e-3).all() and (np.abs(v % 1 - 0.5) < 1e-3).all()
    tx, ty = np.floor(u).astype(int), np.floor(v).astype(int)
    assert np.array_equal(tx, (15 - cols) % 32) and np.array_equal(ty, rows)
    t = Sampler(seed=3, device=0)
    got = t.radiance(rb, rays_o, rays_d, 1)
    t.close()
    want = (color[None, :] * texels[ty, tx]).astype(f32)
    assert H.same(got, want) and want.max() > 0, (got, want)
