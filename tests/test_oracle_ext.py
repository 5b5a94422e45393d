"""The CPU oracle's restatement of mrt_create_ext (oracle/mrt_oracle.c orc_create_ext; DESIGN.md §14 per-corner attributes,
§15 environment texture, §16 bilinear filter), which is written from the contract text and shares no code with the kernel
headers:

a. its elementwise pieces bit for bit against the float32 numpy restatements of vattr_ref / env_ref / filter_ref;
b. the identities the contract states, inside the oracle;
c. FULL PATHS: the oracle against the x86 build of the kernel headers (tests/emu/env_probe.cpp, which takes any mrt_desc_ext) on
   whole frames, no pixel excluded, at the project's bar of 1e-4 per-channel L-inf on the mean radiance (BASELINE.json
   north_star).  A logic error in mrt_trace.h or mrt_pack.cpp that the GPU-vs-x86 tests compile into both sides shows here.

tests/test_gpu_oracle_ext.py runs the scenes of (c) on the GPU."""
import os
import types

import numpy as np
import pytest

import env_ref as E
import filter_ref as F
import vattr_ref as V
from conftest import make_holder

f32 = np.float32
TOL = 1e-4                                   # north_star: per-channel L-inf on the mean radiance
THREADS = min(16, os.cpu_count() or 1)       # oracle and probe workers: never more than a command's share of the machine
RES = (96, 54)


@pytest.fixture(scope="module")
def probe():
    return E.shared_probe()


def _same(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
CROWD = [[[-0.9 + 0.06 * i, 0.2 + 0.05 * (i % 5), -0.45 + 0.03 * (i % 3)], [0, 0, -1, 0]] for i in range(30)]


def _crowd(d):
    """+ 30 small spheres: the scene gets an instance BVH (as test_gpu_vattr._smooth(crowd=True))."""
    d["scene"]["renderer"].append({"type": "sphere", "r": 0.025, "inst": CROWD, "mat": {"albedo": "#c0a030", "rough": 0.3}})
    return d


def smooth(sample=16, crowd=False):
    from micro_raytracer_amd import scenes
    d = scenes.smooth_mesh_scene(res=RES, sample=sample, bounce=8, n_tris=967)
    return _crowd(d) if crowd else d


def glass_instanced():
    """A glass icosphere with area-weighted corner normals, three rotated and translated instances: the shading normal at the
    exit hit (Hit::i1), the refraction through it, xf_vec of an interpolated normal."""
    from micro_raytracer_amd import scenes
    from test_gpu_parity import _glass_mesh_instances
    d = _glass_mesh_instances(scenes)
    d["frame"]["res"] = list(RES)
    d["rt"].update({"sample": 16, "bounce": 8})
    m = d["scene"]["renderer"][0]
    tris = scenes.icosphere(2, 0.3, (1.0, 1.2, 0.9))
    assert tris.shape[0] == 320 and m["mat"]["glass"] == 0.4 and m["mat"]["opacity"] == 0.2 and m["mat"]["rough"] == 0.1 and len(m["inst"]) == 3
    m["vn"] = scenes.smooth_attrs(tris)[1].tolist()
    return d


def _tex(w, h, rgb):
    return {"w": w, "h": h, "dat": np.ascontiguousarray(rgb, f32).reshape(w * h, 3)}


def _grey(w, h, v):
    return _tex(w, h, np.repeat(np.asarray(v, f32).reshape(-1, 1), 3, 1))


def six_maps(filt):
    """smooth_mesh_scene's mesh with all six maps read through its interpolated UVs, each map a texture of its own size.  The
    scalar maps differ per channel (y, z are not x), so a lookup that takes another channel shows.  omap holds 0, 128/255 and 1
    (the refraction coin's probability is min(1 - opacity, 0.85): 0.85, 0.498 and 0), emap 0, 0, 0.5 and 1 (never, never, a fair
    coin, always): both coins go both ways.  omap and emap are exactly k/255 (the packer's RGB8 layout), the others are not."""
    rng = np.random.default_rng(11)
    d = smooth()

    def scalar(w, h, x):
        x = np.asarray(x, f32).reshape(-1)
        return _tex(w, h, np.stack([x, f32(1.0) - x, (x * f32(0.5) + f32(0.25)).astype(f32)], 1))

    k = np.array([0, 128, 255], f32) / f32(255.0)
    d["scene"]["renderer"][0]["mat"] = {
        "albedo": [0.9, 0.85, 0.8], "rough": 0.5, "metal": 0.0, "glass": 0.2, "opacity": 0.5, "emit": 0.0,
        "tex": _tex(7, 5, rng.uniform(0.2, 1.0, (35, 3))),
        "rmap": scalar(16, 8, rng.uniform(0.0, 1.0, 128)),
        "mmap": scalar(3, 2, [0.0, 0.9, 0.3, 1.0, 0.0, 0.6]),
        "gmap": scalar(1, 1, [0.3]),
        "omap": scalar(5, 9, k[rng.integers(0, 3, 45)]),
        "emap": scalar(2, 2, [0.0, 0.0, 128.0 / 255.0, 1.0]),
    }
    if filt != "nearest":
        d["scene"]["filter"] = filt
    return d


def triangles():
    """Five single `triangle` renderers over a textured floor: vn + uv, vn only, uv only, vn all zero (the face normal), UVs
    below 0 and above 1 (the wrap); two of them under a rotated instance.  A MRT_KIND_TRIANGLE hit carries no triangle id."""
    rng = np.random.default_rng(12)
    d = smooth()
    sc = d["scene"]
    floor = sc["renderer"][1]
    t0 = np.array([[-0.3, 0.0, -0.2], [0.3, 0.0, -0.2], [0.0, 0.05, 0.3]])
    vn = [[[-0.5, -1.0, -0.3], [0.5, -1.0, -0.3], [0.0, -1.0, 0.6]]]
    tex = _tex(7, 5, rng.uniform(0.2, 1.0, (35, 3)))
    tex2 = _tex(3, 2, rng.uniform(0.2, 1.0, (6, 3)))
    tex3 = _tex(5, 9, rng.uniform(0.2, 1.0, (45, 3)))

    def tri(pos, scale=1.0, dirv=None, **kw):
        r = {"type": "triangle", "vtx": (t0 * scale).tolist(), "pos": pos, "mat": kw.pop("mat")}
        if dirv is not None:
            r["dir"] = dirv
        r.update(kw)
        return r

    sc["renderer"] = [
        tri([-0.75, 0.55, 0.1], mat={"rough": 0.4, "tex": tex}, vn=vn, uv=[[[0.1, 0.2], [0.9, 0.3], [0.4, 0.95]]]),
        tri([0.0, 0.45, 0.2], 1.2, [0.3, 0.2, -1, 0.25], mat={"rough": 0.1, "metal": 0.8, "albedo": [0.9, 0.8, 0.6]}, vn=vn),
        tri([0.75, 0.6, 0.1], mat={"rough": 1, "tex": tex2}, uv=[[[0.0, 0.0], [1.0, 0.0], [0.5, 1.0]]]),
        tri([-0.4, 0.35, -0.25], 0.8, mat={"rough": 0.3, "albedo": [0.6, 0.9, 0.7]}, vn=np.zeros((1, 3, 3)).tolist()),
        tri([0.45, 0.3, -0.2], 0.9, [-0.4, 0.3, -1, -0.2], mat={"rough": 0.6, "tex": tex3}, vn=vn, uv=[[[-1.7, -0.4], [2.6, 0.3], [0.2, 3.1]]]),
        floor,
    ]
    return d


ENV_ROT = 0.21


def env(mapping, filt, lights=False, bounce=8, crowd=False, res=RES, ssaa=1):
    from micro_raytracer_amd import scenes
    d = scenes.env_scene(res=res, sample=16, bounce=bounce, mapping=mapping, tex_res=(64, 32), filter=filt)
    d["frame"]["ssaa"] = ssaa
    d["scene"]["sky"]["rot"] = ENV_ROT
    if lights:          # the fold L + T x (E(d) * sky.pwr) with light terms in L
        d["scene"]["light"] = [{"type": "point", "pos": [-0.5, -1, 0.5], "pwr": 0.5, "color": "#ffffff"},
                               {"type": "dir", "dir": [0.3, 0.5, -1.0], "pwr": 0.3, "color": "#c0d0ff"}]
    return _crowd(d) if crowd else d


def material_filter_only():
    """tex_filter = bilinear and no environment: the F_ENV kernel family with Params.off_env == 0.  A textured sphere (v
    clamped), a textured plane (v repeats) and a textured box, scalar maps included."""
    from micro_raytracer_amd import scenes
    rng = np.random.default_rng(13)
    return {
        "rt": {"sample": 16, "bounce": 8, "loss": 0.1},
        "frame": {"res": list(RES), "ssaa": 1, "cam": {"pos": [0.0, -1.4, 0.3], "fov": 60, "aprt": 0.008, "foc": 1.4}},
        "scene": {
            "filter": "bilinear",
            "renderer": [
                {"type": "plane", "n": [0, 0, 1], "pos": [0, 0, -0.4], "mat": {"rough": 1, "tex": F.smooth_tex(16, 8)}},
                {"type": "sphere", "r": 0.35, "pos": [-0.45, 0.3, -0.05], "dir": [0.3, 0.2, 1, 0.1],
                 "mat": {"rough": 0.4, "tex": _tex(7, 5, rng.uniform(0.2, 1.0, (35, 3))), "rmap": _grey(5, 9, rng.uniform(0, 1, 45))}},
                {"type": "box", "sizes": [0.45, 0.4, 0.5], "pos": [0.5, 0.4, -0.1], "dir": [0.25, 0.6, 1, -0.2],
                 "mat": {"tex": scenes._atlas_texture(16, 12, seed=3), "omap": _grey(3, 2, [1, 0.5, 1, 0.25, 1, 0.75])}},
            ],
            "light": [{"type": "point", "pos": [-0.8, -1.0, 0.9], "pwr": 0.4, "color": "#ffe0c0"}],
            "sky": {"color": [0.3, 0.4, 0.6], "pwr": 0.4},
        },
    }


# name -> (builder, samples, seeds)
SCENES = {
    "smooth": (smooth, 16, (1, 2)),
    "smooth_24spp": (lambda: smooth(sample=24), 24, (1,)),                 # crosses the 16-sample accumulation chunk
    "glass_inst": (glass_instanced, 16, (1, 2)),
    "maps_nearest": (lambda: six_maps("nearest"), 16, (1, 2)),
    "maps_bilinear": (lambda: six_maps("bilinear"), 16, (1, 2)),
    "triangles": (triangles, 16, (1, 2)),
    "env_sphere_nearest": (lambda: env("sphere", "nearest"), 16, (1, 2)),
    "env_sphere_bilinear": (lambda: env("sphere", "bilinear"), 16, (1, 2)),
    "env_latlong_nearest": (lambda: env("latlong", "nearest"), 16, (1, 2)),
    "env_latlong_bilinear": (lambda: env("latlong", "bilinear"), 16, (1, 2)),
    "env_lights": (lambda: env("latlong", "bilinear", lights=True), 16, (1, 2)),
    "env_bounce2": (lambda: env("sphere", "nearest", bounce=2), 16, (1, 2)),   # most paths exhaust: the mean in E(d)'s place
    "matfilter_noenv": (material_filter_only, 16, (1, 2)),
    "smooth_crowd": (lambda: smooth(crowd=True), 16, (1, 2)),
    "env_crowd": (lambda: env("sphere", "bilinear", crowd=True), 16, (1, 2)),
    "env_ragged": (lambda: env("sphere", "bilinear", res=(37, 23), ssaa=1.5), 16, (1, 2)),   # 55 x 34: ragged against the 8 x 8 tiles
}


def oracle_render(oracle_mod, holder, seed, spp):
    o = oracle_mod.Oracle(holder, seed=seed)
    o.execute(spp, threads=THREADS)
    ref, cnt = o.accum()
    assert cnt == spp
    return o, ref


def compare(label, got, ref, spp):
    """Whole frame, nothing excluded: equal NaN patterns, L-inf on the mean radiance <= TOL (absolute, HDR scenes included)."""
    assert got.shape == ref.shape
    assert (np.isnan(got) == np.isnan(ref)).all(), label
    err = float(np.nanmax(np.abs(got - ref))) / spp if np.isfinite(ref).any() else 0.0
    same = float(np.mean(_same(got, ref).all(-1)))
    # the same difference in units of the accumulated sum's last place: what an HDR scene's absolute error has to be read against
    with np.errstate(all="ignore"):
        ulps = float(np.nanmax(np.abs(got - ref) / np.spacing(np.maximum(np.abs(ref), f32(1e-30)))))
    print(f"{label}: L-inf on mean radiance {err:.3e} ({ulps:.0f} ulp of the sum), bit-identical pixels {same:.4f}, "
          f"largest mean {float(np.nanmax(ref)) / spp:.3g}")
    assert err <= TOL, (label, err)
    return err, same


def x86_frame(L, holder, seed, spp, shape):
    """env_ref.x86_render (which sizes its frame by the supersampled size) on this module's worker count."""
    acc = E.x86_render(L, holder, seed, spp, threads=THREADS)
    assert acc.shape == tuple(shape)
    return acc


# ---- a. the elementwise pieces against the numpy restatements ------------------------------------------------------------------------
def _degenerate_cases():
    inf, nan = f32(np.inf), f32(np.nan)
    z3 = np.zeros(3, f32)
    vn = np.array([0, 0, 1, 0, 1, 0, 1, 0, 0], f32)
    uv = np.array([0.25, 0.75, 0.5, 0.5, 0.9, 0.1], f32)
    e1, e2 = np.array([1, 0, 0], f32), np.array([0, 1, 0], f32)
    pin = np.array([0.25, 0.25, 0], f32)
    cases = [
        (pin, z3, e1, e1 * f32(2), vn, uv), (pin, z3, z3, e2, vn, uv), (pin, z3, e1 * f32(1e25), e2 * f32(1e25), vn, uv),
        (pin, z3, np.array([nan, 0, 0], f32), e2, vn, uv), (np.array([inf, 0, 0], f32), z3, e1, e2, vn, uv),
        (pin, z3, e1, e2, np.zeros(9, f32), uv), (np.array([0.5, 0.5, 0], f32), z3, e1, e2, np.array([0, 0, 0, 1, 2, 3, -1, -2, -3], f32), uv),
        (pin, z3, e1, e2, np.array([0, 0, 1, inf, 0, 0, 0, 0, 1], f32), uv), (pin, z3, e1, e2, np.array([0, 0, 1, nan, 0, 0, 0, 0, 1], f32), uv),
        (pin, z3, e1, e2, vn, np.array([-0.25, -3.5, 1.0, 2.0, 7.75, -0.0], f32)), (pin, z3, e1, e2, vn, uv),
    ]
    return [np.stack([c[k] for c in cases]) for k in range(6)]


def test_interpolation_equals_the_numpy_restatement_bit_for_bit(oracle_mod):
    """§14: orc_vattr against vattr_ref.np_normal / np_uv on test_vattr_host's random cases (points inside, on edges, at corners,
    outside and off the plane; UVs in -3 .. 3) and on degenerate triangles, zero and non-finite normals."""
    from test_vattr_host import _random_cases
    cols = _random_cases(np.random.default_rng(5), 20000)
    cols = [np.concatenate([a, b]).astype(f32) for a, b in zip(cols, _degenerate_cases())]
    nrm, tex = oracle_mod.vattr(*cols)
    n_ref, good = V.np_normal(*cols[:5])
    assert 0.99 < good.mean() < 1.0                      # both the interpolated normal and the fall-back are exercised
    assert _same(nrm, n_ref).all(), np.flatnonzero(~_same(nrm, n_ref).all(1))[:8]
    want = V.np_uv(*cols[:4], cols[5])
    assert _same(tex, want).all(), np.flatnonzero(~_same(tex, want).all(1))[:8]
    assert ((tex >= 0) & (tex <= 1)).all() and (cols[5].min() < 0) and (cols[5].max() > 1)


@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
@pytest.mark.parametrize("mapping", E.MAPPINGS)
def test_environment_lookup_equals_the_numpy_restatement_bit_for_bit(oracle_mod, probe, mapping, filt):
    """§15 / §16: orc_env_lookup against env_ref.np_env_uv + filter_ref.np_nearest / np_bilinear (clamp_v, nearest where the
    filter falls back) on 10^5 directions plus axes, seam, poles, d.z beyond 1 and NaNs."""
    from micro_raytracer_amd import _abi
    from test_env_host import _directions
    nan = np.array([[np.nan, np.nan, 1.0], [np.nan, np.nan, np.nan], [0.3, np.nan, 0.2], [np.inf, 0.0, 0.0]], f32)
    d = np.concatenate([*_directions(), nan]).astype(f32)
    for (w, h), rot in (((64, 32), 0.21), ((7, 5), -1.25), ((1, 1), 0.0)):
        t = F.random_tex(w, h, F.FMT_F32, 3)
        rgb, uv = oracle_mod.env_lookup(w, h, t.raw, _abi.ENV_MAPPINGS[mapping], rot, _abi.FILTERS[filt], d)
        uv_ref = E.np_env_uv(probe, mapping, rot, d)
        assert _same(uv, uv_ref).all(), (w, h, rot)
        want = F.np_nearest(t, uv_ref[:, 0], uv_ref[:, 1])
        if filt == "bilinear":
            out, ok = F.np_bilinear(t, uv_ref[:, 0], uv_ref[:, 1], True)
            assert 0 < (~ok).sum() < 8                    # the NaN coordinates take the nearest rule
            want = np.where(ok[:, None], out, want)
        bad = ~_same(rgb, want).all(1)
        assert not bad.any(), (w, h, rot, d[bad][:4], rgb[bad][:4], want[bad][:4])


@pytest.mark.parametrize("mapping", E.MAPPINGS)
def test_mean_equals_the_float64_mean(oracle_mod, mapping):
    from micro_raytracer_amd import _abi
    rng = np.random.default_rng(7)
    for w, h in ((7, 5), (64, 32), (1, 1), (3, 17)):
        dat = rng.uniform(0.0, 12.0, (w * h, 3)).astype(f32)
        want = E.mean64(types.SimpleNamespace(w=w, h=h, dat=dat), mapping).astype(f32)
        got = oracle_mod.env_mean(w, h, dat, _abi.ENV_MAPPINGS[mapping])
        assert _same(got, want).all(), (w, h, got, want)


# ---- b. identities inside the oracle ---------------------------------------------------------------------------------------------------
def test_an_ext_that_requests_nothing_is_orc_create(oracle_mod):
    from micro_raytracer_amd import _abi, scenes
    for desc in (scenes.kitchen_sink(res=(48, 32), sample=4), scenes.mesh_scene(res=(48, 27), sample=2, n_tris=300)):
        render, holder = make_holder(desc)
        assert holder.ext is None
        spp = render.rt.sample
        _, base = oracle_render(oracle_mod, holder, 3, spp)
        holder.ext = _abi.DescExt()
        _, got = oracle_render(oracle_mod, holder, 3, spp)
        assert _same(got, base).all()
        holder.ext.n_renderer = holder.desc.scene.n_renderer              # an attribute table with no attribute in it
        attrs = (_abi.TriAttrs * holder.desc.scene.n_renderer)()
        holder.keep.append(attrs)
        import ctypes as C
        holder.ext.attrs = C.cast(attrs, C.POINTER(_abi.TriAttrs))
        _, got = oracle_render(oracle_mod, holder, 3, spp)
        assert _same(got, base).all()


def test_oracle_of_a_scene_with_attributes_renders_them(oracle_mod):
    """Oracle(holder) goes through orc_create_ext whenever the holder has an ext: the smooth textured mesh is no longer
    rejected, and it is not the faceted, untextured render."""
    from micro_raytracer_amd import scenes
    _, holder = make_holder(scenes.smooth_mesh_scene(res=(48, 27), sample=4, n_tris=300))
    _, got = oracle_render(oracle_mod, holder, 1, 4)
    _, flat = oracle_render(oracle_mod, make_holder(scenes.mesh_scene(res=(48, 27), sample=4, n_tris=300))[1], 1, 4)
    assert not _same(got, flat).all()
    d = scenes.smooth_mesh_scene(res=(48, 27), sample=4, n_tris=300, uv=False)
    d["scene"]["renderer"][0]["mat"]["tex"] = scenes.checker_texture(8, 8, 2)
    with pytest.raises(ValueError, match="textured triangle/mesh"):        # maps without UVs stay rejected
        oracle_mod.Oracle(make_holder(d)[1])


@pytest.mark.parametrize("mapping", E.MAPPINGS)
def test_all_ones_environment_is_the_constant_sky(oracle_mod, mapping):
    """§15, §16: an all-ones environment, filtered or not, gives the bits of the render without one; all-twos under a halved
    sky colour too."""
    from micro_raytracer_amd import scenes

    def build(tex=None, filt="nearest", color=(0.5, 0.75, 1.0)):
        d = scenes.smooth_mesh_scene(res=(48, 27), sample=8, n_tris=300)
        d["scene"]["sky"] = {"color": list(color), "pwr": 0.5}
        if tex is not None:
            E.with_env(d, tex, mapping, 0.37)
            d["scene"]["sky"]["filter"] = filt
        return make_holder(d)[1]

    _, base = oracle_render(oracle_mod, build(), 2, 8)
    assert np.isfinite(base).all() and base.max() > 0
    for filt in ("nearest", "bilinear"):
        assert _same(oracle_render(oracle_mod, build(E.const_env(1.0), filt), 2, 8)[1], base).all(), filt
        assert _same(oracle_render(oracle_mod, build(E.const_env(2.0), filt, (0.25, 0.375, 0.5)), 2, 8)[1], base).all(), filt
    assert not _same(oracle_render(oracle_mod, build(E.smooth_hdr(7, 5)), 2, 8)[1], base).all()


def test_one_texel_textures_render_the_same_filtered(oracle_mod):
    """§16: four equal texels come back bit for bit, so 1 x 1 textures render the same bytes under tex_filter = bilinear."""
    from micro_raytracer_amd import scenes
    for desc in (scenes.kitchen_sink(res=(48, 32), sample=4), scenes.smooth_mesh_scene(res=(48, 27), sample=4, n_tris=300)):
        one = F.one_texel_textures(desc)
        spp = one["rt"]["sample"]
        _, base = oracle_render(oracle_mod, make_holder(one)[1], 2, spp)
        holder = make_holder(F.with_filters(one, tex="bilinear"))[1]
        assert holder.ext is not None and holder.ext.tex_filter == 1
        assert _same(oracle_render(oracle_mod, holder, 2, spp)[1], base).all()
    # and the filter is seen where texels differ
    full = scenes.kitchen_sink(res=(48, 32), sample=4)
    _, a = oracle_render(oracle_mod, make_holder(full)[1], 2, 4)
    _, b = oracle_render(oracle_mod, make_holder(F.with_filters(scenes.kitchen_sink(res=(48, 32), sample=4), tex="bilinear"))[1], 2, 4)
    assert not _same(a, b).all()


# ---- c. full paths: the oracle against the x86 build of the kernel headers ------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_oracle_equals_the_x86_lane_code_on_full_paths(oracle_mod, probe, name):
    """Measured ("extension scenes"): L-inf <= 1.2e-7 on the scenes without an environment, <= 3.8e-6 under
    env_scene's HDR sky (sums up to 800: at most 5 ulp of a pixel's accumulated sum everywhere)."""
    build, spp, seeds = SCENES[name]
    render, holder = make_holder(build())
    assert holder.ext is not None and render.rt.bounce == (2 if name == "env_bounce2" else 8)
    for seed in seeds:
        o, ref = oracle_render(oracle_mod, holder, seed, spp)
        got = x86_frame(probe, holder, seed, spp, ref.shape)
        compare(f"{name} seed {seed} x86", got, ref, spp)
        assert np.nanmax(ref) > 0
