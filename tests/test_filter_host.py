"""The bilinear texture filter without a GPU: the x86 build of the lookups of csrc/mrt_trace.h against a float32
numpy restatement (bit for bit) and float64 bilinear interpolation (within a derived bound), the packer's two flags, x86 renders
that a constant texture must not change whatever the filter, closed-form renders of a mirror sphere under a filtered
environment and of a textured plane / sphere under a point light, the API's rejections, JSON, fingerprint and CLI."""
import ctypes as C
import json

import numpy as np
import pytest

import env_ref as E
import filter_ref as F
from conftest import make_holder
from micro_raytracer_amd._abi import F_ALL, F_BVH, F_ENV, F_VATTR

f32 = np.float32
SIZES = [(1, 1), (1, 7), (7, 1), (61, 31), (1024, 512)]


@pytest.fixture(scope="module")
def probe():
    return F.shared_probe()


@pytest.fixture(scope="module")
def env_probe():
    return E.shared_probe()


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def _edge_coords(w, h):
    """Texel centres, u = 0, u just below 1, u = 1, the poles v = 0 / 1 and their neighbours."""
    below = np.nextafter(f32(1), f32(0))
    above0 = np.nextafter(f32(0), f32(1))
    us = np.array([0.0, above0, 0.5 / w, 1.0 - 0.5 / w, below, 1.0, 0.5, 0.25], f32)
    vs = np.array([0.0, above0, 0.5 / h, 1.0 - 0.5 / h, below, 1.0, 0.5, 0.75], f32)
    return np.stack(np.meshgrid(us, vs), -1).reshape(-1, 2).astype(f32)


# ---- 1. the lookup ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bilinear_is_the_contract_bit_for_bit(probe, size):
    """tex_bilinear and tex_fetch_bilinear of the x86 build against the float32 restatement of §16 on 10^5 random coordinates
    plus the edges, f32 and RGB8 texels, v clamped and repeated, bit for bit; against float64 bilinear interpolation within
    filter_ref.bound64; NaN and infinite coordinates take the nearest rule's texel."""
    w, h = size
    rng = np.random.default_rng(16)
    uv = np.concatenate([rng.random((100000, 2), dtype=f32), _edge_coords(w, h)])
    bad = np.array([[np.nan, 0.5], [0.5, np.nan], [np.inf, 0.5], [0.5, -np.inf], [np.nan, np.nan], [3e38, 0.5], [0.25, -3e38]], f32)
    for fmt in (F.FMT_F32, F.FMT_U8):
        t = F.random_tex(w, h, fmt, seed=w * 7 + h + fmt)
        for clamp_v in (False, True):
            got = F.x86_core(probe, t, uv, clamp_v)
            want, ok_np = F.np_bilinear(t, uv[:, 0], uv[:, 1], clamp_v)
            assert ok_np.all()
            assert _same(got, want), (size, fmt, clamp_v, uv[(got.view(np.uint32) != want.view(np.uint32)).any(1)][:4])
            for cold in (False, True):
                assert _same(F.x86_tex(probe, t, uv, True, clamp_v, cold), want)
            ref = F.bilinear64(t.val, uv[:, 0], uv[:, 1], clamp_v)
            err, bound = float(np.abs(got.astype(np.float64) - ref).max()), F.bound64(t, clamp_v)
            print(f"{w}x{h} fmt {fmt} clamp_v {clamp_v}: |f32 - f64| <= {err:.3e}, bound {bound:.3e}")
            assert err <= bound
            # the result lies between the smallest and the largest of its four texels: no overshoot beyond rounding
            assert got.min() >= t.val.min() - bound and got.max() <= t.val.max() + bound
            # coordinates that are not finite (or beyond 2^30 texels): the nearest rule's texel, trapping nowhere
            assert not F.np_taps(bad[:, 0], bad[:, 1], w, h, clamp_v)[0].any()
            near = F.x86_tex(probe, t, bad, False)
            assert _same(F.x86_tex(probe, t, bad, True, clamp_v), near) and _same(near, F.np_nearest(t, bad[:, 0], bad[:, 1]))
            assert _same(F.x86_core(probe, t, bad, clamp_v), near)
            # finite coordinates outside [0, 1]: still the restatement, and inside the texture
            far = np.array([[-0.75, 0.5], [1.5, 0.5], [0.5, -0.6], [0.5, 1.7], [17.0, -23.0], [-1e6, 1e6]], f32)
            assert _same(F.x86_core(probe, t, far, clamp_v), F.np_bilinear(t, far[:, 0], far[:, 1], clamp_v)[0])
    # a texture without texels stays black
    none = F.Tex(w, h, np.zeros((h, w, 3)), F.FMT_F32)
    none.fmt = F.FMT_NONE
    assert (F.x86_tex(probe, none, uv[:100], True) == 0).all()


def test_the_three_consequences(probe):
    """Exact texel centres of a power-of-two texture return that texel's bits (fx = fy = 0), which is also what the nearest
    rule returns there; four equal texels come back bit for bit whatever fx and fy; under clamp_v a coordinate above the first
    row's centres (iy = -1) gives row 0's horizontal blend whatever fy, and below the last row's the last row's."""
    rng = np.random.default_rng(5)
    for fmt in (F.FMT_F32, F.FMT_U8):
        t = F.random_tex(1024, 512, fmt, seed=fmt)
        ix, iy = rng.integers(0, 1024, 20000), rng.integers(0, 512, 20000)
        uv = np.stack([(ix + 0.5) / 1024.0, (iy + 0.5) / 512.0], 1).astype(f32)
        for clamp_v in (False, True):
            got = F.x86_tex(probe, t, uv, True, clamp_v)
            assert _same(got, t.val[iy, ix]) and _same(got, F.x86_tex(probe, t, uv, False))
        # the poles: v in [0, 0.5 / h) and (1 - 0.5 / h, 1]
        u = rng.random(5000, dtype=f32)
        for v_lo, v_hi, row in ((0.0, 0.5 / 512, 0), (1 - 0.5 / 512, 1.0, 511)):
            v = (v_lo + (v_hi - v_lo) * rng.random(5000)).astype(f32)
            got = F.x86_tex(probe, t, np.stack([u, v], 1), True, True)
            _, x0, x1, _, _, fx, _ = F.np_taps(u, v, 1024, 512, True)
            top = t.val[row, x0] + fx[:, None] * (t.val[row, x1] - t.val[row, x0])
            assert _same(got, top)
            # ... while a repeating v blends the first row with the last one there
            assert not _same(F.x86_tex(probe, t, np.stack([u, v], 1), True, False), top)
    uv = rng.random((20000, 2), dtype=f32)
    for value in ([0.5, 2.0, 7.0], [1.0, 1.0, 1.0], [1e-30, 6e4, 0.0]):
        for w, h in ((1, 1), (5, 3)):
            t = F.Tex(w, h, np.broadcast_to(np.array(value, f32), (h, w, 3)), F.FMT_F32)
            for clamp_v in (False, True):
                assert _same(F.x86_tex(probe, t, uv, True, clamp_v), np.broadcast_to(np.array(value, f32), (20000, 3)))


@pytest.mark.parametrize("mapping", E.MAPPINGS)
def test_filtered_environment_is_the_contract(probe, mapping):
    """env_color with the filter flag: sky.color x bilinear(env_uv(d)) with v clamped, bit for bit on 10^5 directions, the seam,
    the poles and NaNs (which read the nearest rule's texel); the seam wraps: both signs of d.x = 0 give the same colour; without
    the flag the bits are the nearest texel's."""
    rng = np.random.default_rng(15)
    d = rng.normal(size=(100000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    seam = np.array([[0.0, 1.0, 0.0], [-0.0, 1.0, 0.0], [0.0, 0.6, 0.8], [-0.0, 0.6, 0.8], [0.0, 0.6, -0.8], [-0.0, 0.6, -0.8]], f32)
    poles = np.array([[0, 0, 1], [0, 0, -1], [1e-20, -1e-20, 1], [0, 0, 1 + 2.0 ** -23], [0, 0, -1 - 2.0 ** -23]], f32)
    nan = np.array([[np.nan, np.nan, 1.0], [np.nan, np.nan, np.nan], [0.0, 1.0, np.inf]], f32)
    dirs = np.concatenate([d, seam, poles, nan])
    for fmt, (w, h) in ((F.FMT_F32, (61, 31)), (F.FMT_U8, (64, 32)), (F.FMT_F32, (1, 1))):
        t = F.random_tex(w, h, fmt, seed=3 + fmt)
        for rot in (0.0, 0.37):
            got, uv = F.x86_env(probe, t, mapping, rot, True, dirs)
            want, ok = F.np_bilinear(t, uv[:, 0], uv[:, 1], True)
            want = np.where(ok[:, None], want, F.np_nearest(t, uv[:, 0], uv[:, 1]))
            assert _same(got, want), (mapping, rot, fmt)
            # a NaN d.x / d.y makes u NaN; an infinite d.z makes the sphere mapping's v infinite and is clamped away by latlong's
            assert ok[:-3].all() and not ok[-3:-1].any() and bool(ok[-1]) == (mapping == "latlong")
            plain, _ = F.x86_env(probe, t, mapping, rot, False, dirs)
            assert _same(plain, F.np_nearest(t, uv[:, 0], uv[:, 1]))
            if (w, h) == (1, 1):
                assert _same(got, plain)
            else:
                assert not _same(got, plain)
        got, _ = F.x86_env(probe, t, mapping, 0.0, True, seam)
        assert _same(got[0::2], got[1::2])


# ---- 2. packing ------------------------------------------------------------------------------------------------------------------
def _mesh():
    from micro_raytracer_amd import scenes
    return scenes.smooth_mesh_scene(res=(64, 48), sample=4, n_tris=300)


def _pack(env_probe, desc, ext_edit=None):
    from micro_raytracer_amd import _lib
    r, h = make_holder(desc)
    if ext_edit is not None:
        ext_edit(h)
    info, params, blob = E.x86_pack(env_probe, h)
    return r, h, info, params, blob, _lib.plan_launch(h)


def _diff_words(a, b):
    assert a.shape == b.shape
    return set(np.nonzero(a != b)[0].tolist())


def test_packing_sets_two_flags_and_nothing_else(probe, env_probe):
    """ENV word 7 bit 0 and MAT word 14 bit 0 are the whole difference between a filtered and an unfiltered packing: every other
    blob word (the texels among them), Params, lds_words*, walk_cap and the plan are equal."""
    from micro_raytracer_amd import scenes
    off = F.params_offsets(probe)
    rng = np.random.default_rng(3)
    tex = {"w": 64, "h": 32, "dat": rng.uniform(0.0, 9.0, (64 * 32, 3)).astype(f32)}
    plan_keys = ("staging", "staged_bytes", "scene_bytes", "walk_cap", "block_threads", "lds_bytes", "tbvh_nodes", "tbvh_hot_nodes", "small_plain_grid")

    def mats(params, blob):
        """word index of MAT word 14 of every material, and whether the material has a map"""
        off_mat, n = int(params.view(np.uint32)[off["off_mat"] // 4]), int(params.view(np.uint32)[off["n_rend"] // 4])
        idx = [off_mat + 16 * k + 14 for k in range(n)]
        has = [bool((blob[off_mat + 16 * k + 8:off_mat + 16 * k + 14].view(np.int32) >= 0).any()) for k in range(n)]
        return idx, has

    # (a) the environment's filter: one bit of the ENV record
    _, _, i0, p0, b0, pl0 = _pack(env_probe, E.with_env(_mesh(), tex, "latlong", 0.25))
    _, _, i1, p1, b1, pl1 = _pack(env_probe, F.with_filters(E.with_env(_mesh(), tex, "latlong", 0.25), sky="bilinear"))
    assert i0 == i1 and np.array_equal(p0, p1) and pl0 == pl1
    assert _diff_words(b0, b1) == {i0["off_env"] + 7} and b0[i0["off_env"] + 7] == 0 and b1[i0["off_env"] + 7] == 1
    # (b) the material textures' filter without an environment: MAT word 14 of the materials that have a map; the F_ENV family
    mixed = False
    def spheres_too():            # env_scene's geometry under a constant sky: its plane and its two spheres carry no map
        d = scenes.env_scene(res=(64, 48), sample=4, tex_res=(4, 2))
        d["scene"]["sky"] = {"color": [0.5, 0.75, 1.0], "pwr": 0.5}
        return d

    for make in (_mesh, lambda: scenes.minecraft_like(res=(40, 24), ssaa=1, sample=8), spheres_too, lambda: F.lit_scene("sphere", None)):
        _, h0, i0, p0, b0, pl0 = _pack(env_probe, make())
        assert h0.desc.scene.n_textures > 0 and not i0["features"] & F_ENV
        _, h1, i1, p1, b1, pl1 = _pack(env_probe, F.with_filters(make(), tex="bilinear"))
        assert h1.ext.tex_filter == 1
        assert i1["features"] == i0["features"] | F_ENV | F_VATTR and i1["off_env"] == 0
        assert {k: v for k, v in i1.items() if k != "features"} == {k: v for k, v in i0.items() if k != "features"}
        assert np.array_equal(p0, p1)
        idx, has = mats(p0, b0)
        assert any(has)
        mixed = mixed or not all(has)
        assert _diff_words(b0, b1) == {w for w, m in zip(idx, has) if m}
        # bit 0: filtered; with it bit 1 on a sphere's material (v clamps); 0 where the material has no map
        off_rend = int(p0.view(np.uint32)[off["off_rend"] // 4])
        sphere = [int(b0[off_rend + 16 * k]) == 0 for k in range(len(idx))]
        assert all(b0[w] == 0 for w in idx) and all(b1[w] == ((3 if sp else 1) if m else 0) for w, m, sp in zip(idx, has, sphere))
        # the plan: what is staged and the launch shape stay; the LDS total holds the lane stash too, whose size belongs to the
        # kernel family (the Minecraft-shaped scene gives up the 16-slot stash of its 6-wave kernel for the full set's 7 slots)
        full = (pl0["kernel_features"] & F_ALL) == F_ALL
        assert all(pl0[k] == pl1[k] for k in plan_keys if k != "lds_bytes" or full), (pl0, pl1)
        assert pl1["lds_bytes"] <= pl0["lds_bytes"]
        assert pl1["kernel_features"] & F_ENV and (pl1["kernel_features"] & F_ALL) == F_ALL and not pl0["kernel_features"] & F_ENV
        assert (pl1["kernel_features"] & F_BVH) == (pl0["kernel_features"] & F_BVH)
    assert mixed                  # some scene has a material without maps, whose word stays 0
    # (c) both
    _, _, i0, p0, b0, pl0 = _pack(env_probe, E.with_env(_mesh(), tex))
    _, _, i1, p1, b1, pl1 = _pack(env_probe, F.with_filters(E.with_env(_mesh(), tex), sky="bilinear", tex="bilinear"))
    idx, has = mats(p0, b0)
    assert i0 == i1 and np.array_equal(p0, p1) and pl0 == pl1
    assert _diff_words(b0, b1) == {i0["off_env"] + 7} | {w for w, m in zip(idx, has) if m}


def test_a_filter_with_nothing_to_act_on_is_no_request(env_probe):
    """tex_filter = BILINEAR on scenes without a textured material (with and without an environment) and an ext without env:
    blob, Params, plan and kernel_features are those of the scene without the switch."""
    from micro_raytracer_amd import _abi, scenes

    def ask(h):
        if h.ext is None:
            h.ext = _abi.DescExt()
        h.ext.tex_filter = _abi.FILTER_BILINEAR

    for make in (lambda: scenes.cornell_box(res=(32, 32)), lambda: scenes.default_scene(res=(32, 32)),
                 lambda: E.with_env(scenes.cornell_box(res=(32, 32)), E.const_env(1.0))):
        _, h0, i0, p0, b0, pl0 = _pack(env_probe, make())
        assert h0.desc.scene.n_textures == 0
        _, h1, i1, p1, b1, pl1 = _pack(env_probe, make(), ask)
        assert h1.ext.tex_filter == 1 and i0 == i1 and np.array_equal(p0, p1) and np.array_equal(b0, b1) and pl0 == pl1
        if h0.ext is None:
            assert not pl1["kernel_features"] & F_ENV and not i1["features"] & F_ENV
    # Python does not even build an ext for it
    r, h = make_holder(F.with_filters(scenes.cornell_box(res=(32, 32)), tex="bilinear"))
    assert r.scene.tex_filter == "bilinear" and h.ext is None


# ---- 3. a constant texture renders the same bytes under either filter ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "minecraft", "smooth_mesh"])
def test_constant_environments_render_the_constant_sky_when_filtered(env_probe, name):
    """§15's three scenes, 8 bounces, 8 spp: an all-ones environment, and an all-twos one with sky.color halved, with
    filter = bilinear give the accumulator bits of the render without an environment; the AOVs' miss albedo is the sky colour."""
    from test_env_host import SKY3, _scenes3
    make = _scenes3()[name]

    def build(tex=None, mapping="sphere", rot=0.0, color=SKY3):
        d = make()
        d["rt"]["bounce"] = 8
        d["scene"]["sky"] = {"color": list(color), "pwr": 0.5}
        if tex is not None:
            F.with_filters(E.with_env(d, tex, mapping, rot), sky="bilinear")
        return make_holder(d)[1]

    half = tuple(c / 2 for c in SKY3)
    base = E.x86_render(env_probe, build(), 1, 8)
    assert np.isfinite(base).all() and base.max() > 0
    g0, alb0, rend0 = E.x86_aov(env_probe, build())
    for mapping, rot in (("sphere", 0.0), ("latlong", 0.37)):
        h1, h2 = build(E.const_env(1.0), mapping, rot), build(E.const_env(2.0), mapping, rot, half)
        assert h1.ext.env.contents.filter == 1
        assert _same(E.x86_render(env_probe, h1, 1, 8), base), (name, mapping, "ones")
        assert _same(E.x86_render(env_probe, h2, 1, 8), base), (name, mapping, "twos")
        g, alb, rend = E.x86_aov(env_probe, h1)
        miss = g[..., 7] == 0
        assert _same(g, g0) and np.array_equal(rend, rend0) and _same(alb[~miss], alb0[~miss])
        if miss.any():
            assert _same(alb[miss], np.broadcast_to(np.array(SKY3, f32), alb[miss].shape))


@pytest.mark.parametrize("name", ["minecraft", "smooth_mesh"])
def test_one_texel_textures_render_the_same_bytes_when_filtered(env_probe, name):
    """Every material texture replaced by a 1 x 1 texture: tex_filter = bilinear renders the accumulator and AOV bits of the
    unfiltered scene -- through the F_ENV lane code with no environment (constant sky, miss albedo 0), at both staging levels
    of the x86 lane code."""
    from test_env_host import _scenes3
    d0 = F.one_texel_textures(_scenes3()[name]())
    d0["rt"]["bounce"] = 8
    d1 = F.with_filters(F.one_texel_textures(_scenes3()[name]()), tex="bilinear")
    d1["rt"]["bounce"] = 8
    (_, h0), (_, h1) = make_holder(d0), make_holder(d1)
    i0, i1 = E.x86_pack(env_probe, h0)[0], E.x86_pack(env_probe, h1)[0]
    assert not i0["features"] & F_ENV and i1["features"] & F_ENV and i1["off_env"] == 0
    for seed in (1, 2):
        base = E.x86_render(env_probe, h0, seed, 8)
        assert base.max() > 0
        assert _same(E.x86_render(env_probe, h1, seed, 8), base), (name, seed)
        assert _same(E.x86_render(env_probe, h1, seed, 8, warm=True), base), (name, seed, "warm")
    a0, a1 = E.x86_aov(env_probe, h0), E.x86_aov(env_probe, h1)
    assert _same(a0[0], a1[0]) and _same(a0[1], a1[1]) and np.array_equal(a0[2], a1[2])
    miss = a1[0][..., 7] == 0
    assert (a1[1][miss] == 0).all()
    # and the switch is seen where textures are not constant
    d2 = F.with_filters(_scenes3()[name](), tex="bilinear")
    assert not _same(E.x86_render(env_probe, make_holder(d2)[1], 1, 8), E.x86_render(env_probe, make_holder(_scenes3()[name]())[1], 1, 8))


# ---- 4. closed forms ---------------------------------------------------------------------------------------------------------------
def check_mirror(render_fn, mapping, res, label):
    """§15's mirror sphere under the smooth 61 x 31 HDR map with filter = bilinear against float64 bilinear interpolation of the
    same texels; the nearest run of the same view for the count its exclusion rule needs.  render_fn(render, holder) -> mean."""
    out = {}
    for filt in ("nearest", "bilinear"):
        render, holder = make_holder(F.with_filters(E.closed_form_scene(mapping, res=res), sky=filt))
        want, hit, near, ring = F.mirror_closed_form(render)
        out[filt] = F.check_closed(render_fn(render, holder), want, hit, near, ring, filt, f"{label} {mapping}")
    for cls in ("miss", "hit"):
        assert out["bilinear"][cls][0] < out["nearest"][cls][0], (cls, out)      # only the silhouette remains
    return out


def check_lit(render_fn, kind, res, label):
    out = {}
    for filt in ("nearest", "bilinear"):
        render, holder = make_holder(F.lit_scene(kind, filt, res=res))
        want, hit, near, ring = F.lit_closed_form(render)
        mean = render_fn(render, holder)
        assert (mean[~hit & ~ring] == 0).all()
        out[filt] = F.check_closed(mean, want, hit, near, ring, filt, f"{label} {kind}")
    assert out["bilinear"]["hit"][0] < out["nearest"]["hit"][0], out
    return out


@pytest.mark.parametrize("mapping", E.MAPPINGS)
def test_mirror_sphere_under_a_filtered_environment_equals_the_closed_form(env_probe, mapping):
    def run(render, holder):
        acc = E.x86_render(env_probe, holder, 1, 4)
        assert _same(acc, E.x86_render(env_probe, holder, 2, 4))             # no draw reaches the image
        return acc / f32(4)
    check_mirror(run, mapping, (96, 64), "x86 96x64")


@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_textured_surface_under_a_point_light_equals_the_closed_form(env_probe, kind):
    """Material `tex` at bounce 0: albedo x texture(uv) x max(n . l, 0) x light, the texture looked up nearest and bilinearly
    (a sphere clamps v, a plane repeats it), against float64."""
    def run(render, holder):
        return E.x86_render(env_probe, holder, 1, 2) / f32(2)
    check_lit(run, kind, (96, 64), "x86 96x64")


# ---- 5. API, JSON, fingerprint, CLI -----------------------------------------------------------------------------------------------
def test_api_rejections_name_the_field():
    from micro_raytracer_amd import MrtError, _abi, _lib, scenes

    def holder():
        return make_holder(F.with_filters(E.with_env(_mesh(), E.const_env(1.0)), sky="bilinear", tex="bilinear"))[1]

    def expect(h, code, *words):
        with pytest.raises(MrtError) as e:
            _lib.plan_launch(h)
        assert e.value.code == code and all(w in e.value.msg for w in words), (e.value.code, e.value.msg)

    h = holder()
    assert h.ext.tex_filter == 1 and h.ext.env.contents.filter == 1 and _lib.plan_launch(h)["kernel_features"] & F_ENV
    for bad in (2, 7, 0xffffffff):
        h = holder(); h.ext.env.contents.filter = bad
        expect(h, _abi.MRT_ERR_SCENE, "env.filter")
        h = holder(); h.ext.tex_filter = bad
        expect(h, _abi.MRT_ERR_SCENE, "tex_filter", "reserved[0]")
    h = holder(); h.ext.reserved[1] = 1
    expect(h, _abi.MRT_ERR_ARG, "reserved[1]")
    # a bad tex_filter is refused even where it would have nothing to act on
    _, h = make_holder(scenes.cornell_box(res=(32, 32)))
    h.ext = _abi.DescExt(); h.ext.tex_filter = 3
    expect(h, _abi.MRT_ERR_SCENE, "tex_filter")
    # the ABI keeps its shape: the filter is the first word of what was mrt_env.reserved[4]; mrt_desc_ext is untouched
    assert C.sizeof(_abi.Env) == 40 and _abi.Env.filter.offset == 24 and _abi.Env.reserved.offset == 28
    assert C.sizeof(_abi.DescExt) == 32 and _abi.DescExt.reserved.offset == 24
    assert (_abi.FILTER_NEAREST, _abi.FILTER_BILINEAR) == (0, 1) and _lib.lib().mrt_abi_version() == 3


def test_json_round_trip_and_fingerprint():
    from micro_raytracer_amd import load_render, scenes
    from micro_raytracer_amd.sampler import _fingerprint
    from micro_raytracer_amd.scene import dump_render
    d = F.with_filters(scenes.env_scene(res=(32, 24), sample=2, tex_res=(16, 8), filter="bilinear"), tex="bilinear")
    r = load_render(d)
    assert r.scene.sky.filter == "bilinear" and r.scene.tex_filter == "bilinear"
    j = dump_render(r)
    assert j["scene"]["filter"] == "bilinear" and j["scene"]["sky"]["filter"] == "bilinear"
    text = json.dumps(j)
    r2 = load_render(json.loads(text))
    assert r2.scene.sky.filter == "bilinear" and r2.scene.tex_filter == "bilinear"
    assert _fingerprint(load_render(json.loads(text))) == _fingerprint(r2)
    # the defaults are not written, and env_scene's default is nearest
    plain = load_render(scenes.env_scene(res=(32, 24), sample=2, tex_res=(16, 8)))
    assert plain.scene.sky.filter == "nearest" and plain.scene.tex_filter == "nearest"
    jp = dump_render(plain)
    assert "filter" not in jp["scene"] and "filter" not in jp["scene"]["sky"]
    # the fingerprint sees either switch
    fp = _fingerprint(r2)
    r2.scene.sky.filter = "nearest"
    assert _fingerprint(r2) != fp
    r2.scene.sky.filter = "bilinear"; r2.scene.tex_filter = "nearest"
    assert _fingerprint(r2) != fp
    for where, bad in (("sky", {"scene": {"sky": {"filter": "cubic"}}}), ("scene", {"scene": {"filter": "trilinear"}})):
        with pytest.raises(ValueError, match="filter") as e:
            load_render(bad)
        assert where in str(e.value)
    r.scene.sky.filter = "cubic"
    from micro_raytracer_amd import _abi
    with pytest.raises(ValueError, match="sky filter"):
        _abi.build_desc(r)


def test_cli_filter_flags(tmp_path, capsys):
    """--sky-filter without an environment texture is refused like --sky-map (before any device work); unknown values are
    argument errors."""
    from micro_raytracer_amd import __main__ as cli
    from micro_raytracer_amd import scenes
    (tmp_path / "plain.json").write_text(json.dumps(scenes.cornell_box(res=(32, 32), sample=1)))
    with pytest.raises(SystemExit) as e:
        cli.main([str(tmp_path / "plain.json"), "-o", str(tmp_path / "o.png"), "--sky-filter", "bilinear"])
    assert e.value.code == 2 and "--sky-tex" in capsys.readouterr().err
    for flag in ("--sky-filter", "--tex-filter"):
        with pytest.raises(SystemExit) as e:
            cli.main([str(tmp_path / "plain.json"), "-o", str(tmp_path / "o.png"), flag, "cubic"])
        assert e.value.code == 2 and "cubic" in capsys.readouterr().err
