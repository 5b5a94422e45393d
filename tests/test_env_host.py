"""The environment texture of the sky without a GPU: the mapping of the x86 build of csrc/mrt_trace.h against a
float32 numpy restatement and the float64 formula, the packer's layout and mean, x86 renders that an all-ones environment must
not change, the closed-form render of a mirror sphere, the API's rejections, the loader (JSON, Radiance .hdr) and the
denoiser's backdrop rule."""
import ctypes as C
import json

import numpy as np
import pytest

import env_ref as E
from conftest import make_holder
from micro_raytracer_amd._abi import F_ALL, F_ENV, F_VATTR

f32 = np.float32


@pytest.fixture(scope="module")
def probe():
    return E.shared_probe()


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


# ---- 1. the mapping ------------------------------------------------------------------------------------------------------------
def _directions():
    rng = np.random.default_rng(15)
    d = rng.normal(size=(100000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
    seam = np.array([[0.0, 1.0, 0.0], [-0.0, 1.0, 0.0], [0.0, 0.6, 0.8], [-0.0, 0.6, 0.8], [0.0, 0.6, -0.8], [-0.0, 0.6, -0.8]], f32)
    poles = np.array([[0, 0, 1], [0, 0, -1], [1e-20, -1e-20, 1], [-0.0, 0.0, 1.0], [0.0, -0.0, -1.0]], f32)
    over = np.array([[0, 0, 1 + 2.0 ** -23], [0, 0, -1 - 2.0 ** -23], [1e-4, 1e-4, 1 + 2.0 ** -23]], f32)
    return d, axes, seam, poles, over


@pytest.mark.parametrize("mapping", E.MAPPINGS)
def test_env_uv_is_the_contract_bit_for_bit(probe, mapping):
    """env_uv of the x86 build against the float32 restatement of §15 (atan2_ / acos_ taken elementwise from the same build)
    bit for bit, and within 2e-6 of the float64 formula.  The seam (d.x = +0 / -0, d.y > 0: u0 = 1 and 0) lands in column 0.
    NaN directions trap nowhere: (NaN, NaN, 1) reads texel 0 under both mappings; for the all-NaN direction the contract's
    own clamp (fmax_ is maxNum: NaN -> -1) makes v = 1 under "latlong", i.e. the last texel, and texel 0 under "sphere"."""
    rnd, axes, seam, poles, over = _directions()
    w, h = 64, 32
    for rot in (0.0, 0.37, -1.25):
        d = np.concatenate([rnd, axes, seam, poles, over])
        got, idx = E.x86_uv(probe, mapping, rot, d, w, h)
        want = E.np_env_uv(probe, mapping, rot, d)
        assert E.same_bits(got, want).all(), (mapping, rot, d[~E.same_bits(got, want).all(1)][:4])
        assert np.array_equal(idx.astype(np.int64), E.np_env_index(want, w, h))
        assert idx.max() < w * h and (got[:, 0] >= 0).all() and (got[:, 0] < 1).all()
        # float64: compare on the circle (u = 0 and u = 1 - eps are neighbours); poles have no azimuth
        ref = E.env_uv64(mapping, rot, d.astype(np.float64))
        ok = np.hypot(d[:, 0], d[:, 1]) > 1e-3
        du = np.abs(got[:, 0].astype(np.float64) - ref[:, 0])
        du = np.minimum(du, 1.0 - du)
        dv = np.abs(got[:, 1].astype(np.float64) - ref[:, 1])
        print(f"{mapping} rot {rot}: |du| <= {du[ok].max():.2e}, |dv| <= {dv.max():.2e}")
        assert du[ok].max() <= 2e-6 and dv[ok & (np.abs(d[:, 2]) <= 1)].max() <= 2e-6
    # the seam at rot = 0: both signs of zero land in column 0
    got, idx = E.x86_uv(probe, mapping, 0.0, seam, w, h)
    assert (idx % w == 0).all(), idx
    assert got[0, 0] == 0.0 and got[1, 0] == 0.0
    # d.z beyond 1 by an ulp: row 0 (latlong: the clamp; sphere: a negative v truncates to 0)
    _, idx = E.x86_uv(probe, mapping, 0.0, over[:1], w, h)
    assert idx[0] < w
    nan = np.array([[np.nan, np.nan, 1.0], [np.nan, np.nan, np.nan]], f32)
    _, idx = E.x86_uv(probe, mapping, 0.0, nan, w, h)
    assert idx[0] == 0 and idx[1] == (w * h - 1 if mapping == "latlong" else 0)
    assert np.array_equal(idx.astype(np.int64), E.np_env_index(E.np_env_uv(probe, mapping, 0.0, nan), w, h))


def test_sphere_mapping_is_the_sphere_renderers_uv(probe):
    """"sphere", rot 0: env_uv(d) == hit_uv of a unit sphere at the origin for the hit point d, wherever norm(d) returns d."""
    rnd, axes, seam, poles, _ = _directions()
    d = np.concatenate([rnd, axes, seam, poles[:2]])
    uv_s, nrm = E.x86_sphere_uv(probe, d)
    fixed = E.same_bits(nrm, d).all(1)
    assert fixed.sum() > 1000
    uv_e, _ = E.x86_uv(probe, "sphere", 0.0, d, 8, 8)
    # hit_uv's u is not wrapped: u0 = 1 on the seam is the environment's u = 0
    u_s = np.where(uv_s[:, 0] == 1.0, f32(0.0), uv_s[:, 0])
    assert E.same_bits(u_s[fixed], uv_e[fixed, 0]).all() and E.same_bits(uv_s[fixed, 1], uv_e[fixed, 1]).all()


# ---- 2. packing ------------------------------------------------------------------------------------------------------------------
def test_packing_leaves_the_staged_scene_alone(probe):
    from micro_raytracer_amd import _abi, _lib, scenes
    base = scenes.smooth_mesh_scene(res=(64, 48), sample=4, n_tris=300)
    _, h0 = make_holder(base)
    # no environment: the blob and the kernel's parameter block are those of a scene packed without the ext's env field
    info0, p0, b0 = E.x86_pack(probe, h0)
    assert info0["off_env"] == 0 and not info0["features"] & F_ENV
    for plain in (scenes.cornell_box(res=(32, 32)), scenes.default_scene(res=(32, 32))):
        _, hp = make_holder(plain)
        assert hp.ext is None
        i1, p1, b1 = E.x86_pack(probe, hp, with_ext=False)
        ext = _abi.DescExt()                              # an ext that carries nothing
        hp.ext = ext
        i2, p2, b2 = E.x86_pack(probe, hp)
        assert i1 == i2 and np.array_equal(p1, p2) and np.array_equal(b1, b2)
    rng = np.random.default_rng(3)
    big = {"w": 1024, "h": 512, "dat": rng.uniform(0.0, 9.0, (1024 * 512, 3)).astype(f32)}
    one = {"w": 1, "h": 1, "dat": np.array([[0.5, 2.0, 7.0]], f32)}
    plans = []
    for tex in (one, big):
        r, h = make_holder(E.with_env(scenes.smooth_mesh_scene(res=(64, 48), sample=4, n_tris=300), tex, "latlong", 0.25))
        info, params, blob = E.x86_pack(probe, h)
        assert info["features"] & F_ENV and info["features"] & F_VATTR and info["off_env"] >= info["lds_words"]
        for k in ("lds_words", "lds_words_warm", "lds_words_hot", "walk_cap"):
            assert info[k] == info0[k], k
        assert np.array_equal(blob[:info0["lds_words"]], b0[:info0["lds_words"]])          # everything a kernel may stage
        rec = blob[info["off_env"]:info["off_env"] + 8]
        assert (rec[0], rec[1], rec[3], rec[4]) == (tex["w"], tex["h"], 1, 1) and rec[5:7].view(f32).tolist() == [0.25, 0.5]
        off = int(rec[2])
        assert off >= info["lds_words"] and np.array_equal(blob[off:off + tex["w"] * tex["h"] * 3].view(f32), tex["dat"].reshape(-1))
        plans.append(_lib.plan_launch(h))
    for k in ("staging", "staged_bytes", "scene_bytes", "walk_cap", "block_threads", "lds_bytes"):
        assert plans[0][k] == plans[1][k], (k, plans)
    assert plans[1]["kernel_features"] & F_ENV and (plans[1]["kernel_features"] & F_ALL) == F_ALL
    assert not _lib.plan_launch(h0)["kernel_features"] & F_ENV
    # texels that are all k/255 take the RGB8 layout
    u8 = {"w": 5, "h": 3, "dat": (rng.integers(0, 256, (15, 3)).astype(f32) / f32(255.0))}
    _, h = make_holder(E.with_env(scenes.cornell_box(res=(32, 32)), u8))
    info, _, blob = E.x86_pack(probe, h)
    rec = blob[info["off_env"]:info["off_env"] + 8]
    assert rec[3] == 2 and rec[2] % 4 == 0
    got = blob.view(np.uint8)[int(rec[2]):int(rec[2]) + 45]
    assert np.array_equal(got, np.rint(u8["dat"].reshape(-1) * 255).astype(np.uint8))


@pytest.mark.parametrize("mapping", E.MAPPINGS)
def test_exhausted_paths_take_the_weighted_mean(probe, mapping):
    from micro_raytracer_amd import scenes
    rng = np.random.default_rng(7)
    tex = {"w": 7, "h": 5, "dat": rng.uniform(0.0, 12.0, (35, 3)).astype(f32)}
    d = E.with_env(scenes.cornell_box(res=(32, 32)), tex, mapping, 0.1, color=(0.9, 0.8, 0.7))
    d["scene"]["sky"]["pwr"] = 0.6
    r, h = make_holder(d)
    m = E.mean64(r.scene.sky.tex, mapping).astype(f32)
    want = (np.array([0.9, 0.8, 0.7], f32) * m) * f32(0.6)
    got = E.x86_sky_init(probe, h)
    assert _same(got, want), (got, want)
    if mapping == "latlong":      # the weights matter: the plain mean is something else
        assert not _same(m, E.mean64(r.scene.sky.tex, "sphere").astype(f32))


# ---- 3. an all-ones environment changes nothing ----------------------------------------------------------------------------------
def _scenes3():
    from micro_raytracer_amd import scenes
    return {"cornell": lambda: scenes.cornell_box(res=(40, 32), sample=8),
            "minecraft": lambda: scenes.minecraft_like(res=(40, 24), ssaa=1, sample=8),
            "smooth_mesh": lambda: scenes.smooth_mesh_scene(res=(40, 24), sample=8, n_tris=300)}


SKY3 = (0.5, 0.75, 1.0)


@pytest.mark.parametrize("name", ["cornell", "minecraft", "smooth_mesh"])
def test_ones_and_twos_render_the_constant_sky_bit_for_bit(probe, name):
    """8 bounces, 8 spp, seeds 1 and 2: an all-ones 3 x 2 environment, and an all-twos one with sky.color halved, give the
    accumulator of the render without an environment, bit for bit (all products are exact), for both mappings and two rots."""
    make = _scenes3()[name]

    def build(tex=None, mapping="sphere", rot=0.0, color=SKY3):
        d = make()
        d["rt"]["bounce"] = 8
        d["scene"]["sky"] = {"color": list(color), "pwr": 0.5}
        if tex is not None:
            E.with_env(d, tex, mapping, rot)
        return make_holder(d)[1]

    half = tuple(c / 2 for c in SKY3)
    for seed in (1, 2):
        h = build()
        base = E.x86_render(probe, h, seed, 8)
        assert np.isfinite(base).all() and base.max() > 0
        black = E.x86_render(probe, build(color=(0, 0, 0)), seed, 8)
        assert not _same(base, black)                                # the sky is seen at all
        for mapping in E.MAPPINGS:
            for rot in (0.0, 0.37):
                ones = E.x86_render(probe, build(E.const_env(1.0), mapping, rot), seed, 8)
                assert _same(ones, base), (name, seed, mapping, rot, "ones")
                twos = E.x86_render(probe, build(E.const_env(2.0), mapping, rot, half), seed, 8)
                assert _same(twos, base), (name, seed, mapping, rot, "twos")
    # and an environment that is not constant is seen
    tex = {"w": 3, "h": 2, "dat": np.array([[1, 1, 1], [3, 0.5, 1], [1, 1, 1], [0.2, 1, 2], [1, 1, 1], [1, 4, 1]], f32)}
    assert not _same(E.x86_render(probe, build(tex), 1, 8), E.x86_render(probe, build(), 1, 8))


# ---- 4. closed form ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapping", E.MAPPINGS)
def test_mirror_sphere_under_an_environment_equals_the_closed_form(probe, mapping):
    """The closed form of tests/env_ref.py (Checks) on the x86 build, 96 x 64: at most 2 % of the pixels of each
    class may fall to the texel-boundary exclusion (a float64 model of this set-up puts 0.2 % .. 0.9 % there)."""
    render, holder = make_holder(E.closed_form_scene(mapping))
    acc = E.x86_render(probe, holder, 1, 4)
    E.check_closed_form(acc / f32(4), render, "x86 96x64")
    assert _same(acc, E.x86_render(probe, holder, 2, 4))             # no draw reaches the image
    assert _same(acc, E.x86_render(probe, holder, 1, 4, warm=True))


# ---- 5. API edges -------------------------------------------------------------------------------------------------------------------
def _plan_error(holder):
    from micro_raytracer_amd import MrtError, _lib
    with pytest.raises(MrtError) as e:
        _lib.plan_launch(holder)
    return e.value.code, e.value.msg


def test_api_rejections_name_the_field():
    """Every rejection by its code and a message that names the field; an ext that carries an environment only.  (Sharding is a
    property of mrt_opts, which mrt_plan_launch_ext does not take: environments on contexts with shard_count = 2 are created and
    rendered in tests/test_gpu_env.py::test_gpu_two_row_shards_assemble_to_the_frame.)"""
    from micro_raytracer_amd import _abi, _lib, scenes

    def holder(tex=None, mapping="sphere", rot=0.0):
        tex = E.const_env(1.0) if tex is None else tex
        return make_holder(E.with_env(scenes.cornell_box(res=(32, 32)), tex, mapping, rot))[1]

    def expect(h, code, *words):
        got, msg = _plan_error(h)
        assert got == code and all(w in msg for w in words), (got, msg)

    h = holder(); h.ext.env.contents.tex.w = 0
    expect(h, _abi.MRT_ERR_SCENE, "env.tex", "0x2")
    h = holder(); h.ext.env.contents.tex.h = 0
    expect(h, _abi.MRT_ERR_SCENE, "env.tex", "3x0")
    h = holder(); h.ext.env.contents.tex.dat = None
    expect(h, _abi.MRT_ERR_SCENE, "env.tex.dat")
    for bad in (np.nan, np.inf, -1e-3):
        t = E.const_env(1.0); t["dat"][4, 1] = bad
        expect(holder(t), _abi.MRT_ERR_SCENE, "env.tex", "texel (1, 1)")
    h = holder(); h.ext.env.contents.mapping = 2
    expect(h, _abi.MRT_ERR_SCENE, "env.mapping")
    for bad in (np.nan, np.inf):
        h = holder(); h.ext.env.contents.rot = bad
        expect(h, _abi.MRT_ERR_SCENE, "env.rot")
    # more than 2^25 texels: the limit (the data is never read: w x h is checked first)
    h = holder(); h.ext.env.contents.tex.w, h.ext.env.contents.tex.h = 8192, 4097
    expect(h, _abi.MRT_ERR_LIMIT, "env.tex", "2^25")
    # an ext with an environment only: attrs NULL, n_renderer anything
    h = holder(mapping="latlong", rot=0.5)
    assert not h.ext.attrs
    h.ext.n_renderer = 77
    assert _lib.plan_launch(h)["kernel_features"] & F_ENV
    # negative zero is a legal texel, so is HDR
    t = E.const_env(1.0); t["dat"][0, 0] = -0.0; t["dat"][1, 1] = 6e4
    assert _lib.plan_launch(holder(t))["kernel_features"] & F_ENV
    # layout of mrt_desc_ext: env takes the first two words of what was reserved[4]
    assert C.sizeof(_abi.DescExt) == 32 and _abi.DescExt.env.offset == 16 and _abi.DescExt.reserved.offset == 24
    assert C.sizeof(_abi.Env) == 40


# ---- 6. loader ----------------------------------------------------------------------------------------------------------------------
def test_json_round_trip_and_fingerprint():
    from micro_raytracer_amd import load_render, scenes
    from micro_raytracer_amd.scene import dump_render
    from micro_raytracer_amd.sampler import _fingerprint
    d = scenes.env_scene(res=(32, 24), sample=2, mapping="latlong", tex_res=(16, 8))
    d["scene"]["sky"]["rot"] = 0.3
    r = load_render(d)
    assert r.scene.sky.mapping == "latlong" and r.scene.sky.rot == float(f32(0.3)) and r.scene.sky.tex.dat.max() >= 40
    text = json.dumps(dump_render(r))
    r2 = load_render(json.loads(text))
    assert _same(r2.scene.sky.tex.dat, r.scene.sky.tex.dat) and (r2.scene.sky.tex.w, r2.scene.sky.tex.h) == (16, 8)
    assert r2.scene.sky.mapping == "latlong" and r2.scene.sky.rot == r.scene.sky.rot
    assert _fingerprint(load_render(json.loads(text))) == _fingerprint(r2)
    # a sky without a texture dumps as before
    plain = load_render(scenes.cornell_box(res=(32, 32)))
    assert set(dump_render(plain)["scene"]["sky"]) == {"color", "pwr"}
    # the fingerprint sees a texel, the mapping, the rotation
    fp = _fingerprint(r2)
    r2.scene.sky.tex.dat[5, 1] += f32(0.5)
    assert _fingerprint(r2) != fp
    r2 = load_render(json.loads(text)); r2.scene.sky.mapping = "sphere"
    assert _fingerprint(r2) != fp
    r2 = load_render(json.loads(text)); r2.scene.sky.rot = 0.25
    assert _fingerprint(r2) != fp
    r2 = load_render(json.loads(text)); r2.scene.sky.tex = None
    assert _fingerprint(r2) != fp
    with pytest.raises(ValueError):
        load_render({"scene": {"sky": {"tex": E.const_env(1.0), "map": "cube"}}})


@pytest.mark.parametrize("rle", [False, True])
def test_hdr_reader(tmp_path, rle):
    from micro_raytracer_amd import load_render
    from micro_raytracer_amd.scene import Texture
    rng = np.random.default_rng(11)
    w, h = 37, 9
    px = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    px[2, 3:20] = (7, 7, 7, 130)                 # long runs
    px[4, :, 3] = 0                              # e = 0: black, whatever the mantissas
    px[5, 0] = (255, 255, 255, 255)
    px[6, :] = (1, 0, 200, 1)
    p = tmp_path / "sky.hdr"
    E.write_hdr(p, px, rle)
    t = Texture.from_json("sky.hdr", str(tmp_path))
    assert (t.w, t.h) == (w, h) and t.dat.dtype == np.float32 and _same(t.dat, E.rgbe_decode(px))
    assert (t.dat[4 * w:5 * w] == 0).all() and t.dat.max() > 1e30
    if rle:
        assert len(E.rgbe_bytes(px, True)) != px.size
    one = np.array([[[128, 64, 32, 129]]], np.uint8)
    E.write_hdr(p, one, rle, magic=b"#?RGBE")
    t = Texture.from_json("sky.hdr", str(tmp_path))
    assert (t.w, t.h) == (1, 1) and t.dat.tolist() == [[1.0, 0.5, 0.25]]
    # through a render description
    (tmp_path / "s.json").write_text(json.dumps({"scene": {"sky": {"color": [1, 1, 1], "tex": "sky.hdr", "map": "latlong"}}}))
    r = load_render(str(tmp_path / "s.json"))
    assert r.scene.sky.tex.dat.tolist() == [[1.0, 0.5, 0.25]] and r.scene.sky.mapping == "latlong"
    E.write_hdr(p, one, rle, res_line=b"+Y 1 +X 1")
    with pytest.raises(ValueError):
        Texture.from_json("sky.hdr", str(tmp_path))
    E.write_hdr(p, one, rle, magic=b"#?PNG")
    with pytest.raises(ValueError):
        Texture.from_json("sky.hdr", str(tmp_path))
    # truncated files: ValueError wherever the cut falls (header, resolution line, scanline marker, inside a run)
    E.write_hdr(p, px, rle)
    whole = p.read_bytes()
    body = len(whole) - len(E.rgbe_bytes(px, rle))
    for cut in sorted({5, 20, body - 3, body, body + 1, body + 2, body + 3, body + 4, body + 5, body + 40, len(whole) - 1}):
        p.write_bytes(whole[:cut])
        with pytest.raises(ValueError):
            Texture.from_json("sky.hdr", str(tmp_path))


def test_cli_sky_flags_need_a_texture(tmp_path, capsys):
    """--sky-map / --sky-rot on a description without an environment texture are refused, not ignored (before any device work)."""
    from micro_raytracer_amd import __main__ as cli
    from micro_raytracer_amd import scenes
    (tmp_path / "plain.json").write_text(json.dumps(scenes.cornell_box(res=(32, 32), sample=1)))
    for flags in (["--sky-map", "latlong"], ["--sky-rot", "0.25"]):
        with pytest.raises(SystemExit) as e:
            cli.main([str(tmp_path / "plain.json"), "-o", str(tmp_path / "o.png"), *flags])
        assert e.value.code == 2 and "--sky-tex" in capsys.readouterr().err


# ---- 7. the denoiser keeps a detailed backdrop -----------------------------------------------------------------------------------------
def denoise_scene(res=(96, 64)):
    return E.closed_form_scene("sphere", res=res, tex=E.checker_env(), sample=4)


def check_backdrop(acc, guide, albedo, den_env, den_forced, label):
    """Primary-miss pixels of the denoised image equal the undenoised mean to rtol 1e-5; with the miss divisor forced to 1 every
    miss pixel next to a checker edge (a 4-neighbour, itself a miss, with another texel) moves by more than 10 %, on the dark and
    on the bright side of the edge (x86 build: dark 930 % and more, bright 46 % and more)."""
    mean = (acc * f32(0.25)).astype(np.float64)
    miss = guide[..., 7] == 0
    assert miss.sum() > 1000 and (~miss).sum() > 300
    assert _same(albedo[miss], (acc * f32(0.25))[miss])              # the AOV of a miss is its backdrop E(d)
    rel = np.abs(den_env[miss] - mean[miss]) / mean[miss]
    print(f"{label}: miss pixels denoised / mean - 1 <= {rel.max():.2e}")
    assert rel.max() <= 1e-5
    lum = mean[..., 0]
    dark = np.zeros_like(miss)                      # miss pixels with a brighter miss 4-neighbour, and the bright ones next to them
    bright = np.zeros_like(miss)
    for sl_a, sl_b in ((np.s_[:-1], np.s_[1:]), (np.s_[:, :-1], np.s_[:, 1:])):
        both = miss[sl_a] & miss[sl_b]
        dark[sl_a] |= both & (lum[sl_a] < lum[sl_b]); bright[sl_b] |= both & (lum[sl_a] < lum[sl_b])
        dark[sl_b] |= both & (lum[sl_b] < lum[sl_a]); bright[sl_a] |= both & (lum[sl_b] < lum[sl_a])
    moved = np.abs(den_forced - mean) / mean
    md, mb = moved[dark & ~bright], moved[bright & ~dark]
    print(f"{label}: divisor forced to 1: {md.shape[0]} dark-side edge pixels move by {md.min():.1%} .. {md.max():.1%}, "
          f"{mb.shape[0]} bright-side ones by {mb.min():.1%} .. {mb.max():.1%} (median {np.median(mb):.1%})")
    # (contrast 1 : 20: a pixel that takes a share f of its weight from across the edge moves by 19 f on the dark side and by
    # 0.95 f on the bright side; env_ref.checker_env says why f is large for every pixel of this checker)
    assert md.shape[0] > 100 and md.min() > 0.10
    assert mb.shape[0] > 100 and mb.min() > 0.10


def test_denoiser_keeps_the_backdrop(probe):
    render, holder = make_holder(denoise_scene())
    acc = E.x86_render(probe, holder, 1, 4)
    g, alb, rend = E.x86_aov(probe, holder)
    counts = np.full(acc.shape[:2], 4, np.uint32)
    den = E.x86_filter(probe, acc, counts, g, alb, env=True)
    forced = E.x86_filter(probe, acc, counts, g, alb, env=False)
    check_backdrop(acc, g, alb, den, forced, "x86")
    # a context without an environment: the filter is what it was (miss albedo 0, divisor 1)
    d = denoise_scene()
    del d["scene"]["sky"]["tex"], d["scene"]["sky"]["map"], d["scene"]["sky"]["rot"]
    _, h0 = make_holder(d)
    _, alb0, _ = E.x86_aov(probe, h0)
    assert (alb0[g[..., 7] == 0] == 0).all()
