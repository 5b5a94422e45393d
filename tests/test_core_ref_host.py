"""The deterministic core against a float64 restatement of the reference, CPU side: the oracle (Oracle.execute / accum, ray_query)
and the x86 build of the kernel headers (emu.render, rayq_cases.probe_trace) against tests/core_ref.py on the scenes and ray sets
of tests/core_cases.py, under the comparison rules stated there ("the deterministic core").  Oracle, kernel headers
and core_ref are three readings of src/rt.rs; core_ref shares no code with the other two."""
import functools

import numpy as np
import pytest

import core_cases as K
import core_ref as R
import rayq_cases as Q
from conftest import make_holder

f32 = np.float32
IMAGES = dict(K.image_cases())
RAY_SCENES = {"primitives": K.primitives, "lights": K.lights}
TABLE = {"image": {}, "rays": {}}          # branch coverage gathered by the tests of this module, asserted by the last one


@functools.lru_cache(maxsize=None)
def image_case(name):
    """(render, holder, float64 render, float32 render's image): computed once, shared and left unchanged."""
    render, holder = make_holder(IMAGES[name])
    ref = R.render_image(render, np.float64)
    img32 = R.render_image(render, np.float32)["img"]
    assert ref["shape"][0] * ref["shape"][1] <= 96 * 64
    return render, holder, ref, img32


@functools.lru_cache(maxsize=None)
def ray_case(name):
    desc = RAY_SCENES[name]()
    render, holder = make_holder(desc)
    ref = image_case("primitives" if name == "primitives" else "lights/view0")[2]
    o, d = K.ray_set(desc, ref, 7 if name == "primitives" else 8)
    return render, holder, o, d


def two_samples_are_twice_one(one, two, ref):
    """aprt 0: every sample of a pixel whose path draws no random number that matters is the same ray, to the last bit."""
    same = ~ref["random"]
    assert same.sum() >= 0.5 * same.size
    assert np.array_equal((one + one)[same].view(np.uint32), two[same].view(np.uint32))


@pytest.fixture(scope="module")
def probe():
    return Q.shared_probe()


def oracle_image(oracle_mod, holder, ref):
    orc = oracle_mod.Oracle(holder, seed=1)
    orc.execute(1, threads=4)
    one = orc.accum()[0].copy()
    orc.execute(1, threads=4)
    two, cnt = orc.accum()
    orc.close()
    assert cnt == 2
    two_samples_are_twice_one(one, two, ref)
    return two / f32(2)


# ---- the restatement's own pieces ------------------------------------------------------------------------------------------------------
def test_identity_direction_is_the_identity_and_the_matrices_are_orthogonal():
    """Vec4f::backward() as an instance direction and (0, 0, 1, 0) as a camera direction give identity matrices (src/lin.rs:175-208
    with their signs); every direction of the cases gives orthogonal ones, so the normal's trip BACK through the same matrices
    (src/rt.rs:792) is not the inverse of the trip in: for a rotated instance it is another rotation."""
    f = R.Frame([0, 0, 0], K.IDENT, np.float64)
    assert np.array_equal(f.rot @ f.look, np.eye(3))
    assert np.array_equal(R.rotate_y([0, 0, 1, 0]) @ R.lookat([0, 0, 1, 0]), np.eye(3))
    for d in (K.ROT_A, K.ROT_B):
        f = R.Frame([0, 0, 0], d, np.float64)
        m = f.rot @ f.look
        assert np.allclose(m @ m.T, np.eye(3), atol=1e-12) and not np.allclose(m @ m, np.eye(3), atol=1e-3)


def test_candidate_rule_equals_vattr_refs():
    """core_ref._cells at pad 0 (leaves merged to their unique boxes) gives the candidates of vattr_ref._candidates."""
    from vattr_ref import _candidates
    tris = np.asarray(K.icosphere(0.6), np.float64)
    rng = np.random.default_rng(3)
    o = rng.uniform(-1.5, 1.5, (3000, 3))
    d = rng.normal(size=(3000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    mine = R._cells(o, d, tris, (0.0,))[0]
    assert mine.any() and not mine.all()
    assert np.array_equal(mine, _candidates(o[:, None, :], d[:, None, :], tris))


def test_box_branches_z_overrides_the_chain_for_the_normal_only():
    """src/rt.rs:429-441 against 487-515: on the +x / +z edge the normal is +z (`} if` after the chain) and the UV is +x's (the
    chain returns)."""
    face, uv_face, second, window, _ = R.box_face(np.array([[1.0, 0.2, 1.0], [1.0, 0.2, 0.3], [0.1, -1.0, -1.0], [0.5, 0.5, 0.5]]))
    assert face.tolist() == [4, 0, 5, -1] and uv_face.tolist() == [0, 0, 3, -1]
    assert second[0] == 0 and second[1] > 0.69


# ---- images ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(IMAGES))
def test_oracle_image_against_float64(oracle_mod, name):
    render, holder, ref, img32 = image_case(name)
    got = oracle_image(oracle_mod, holder, ref)
    keep = K.compare_image(f"oracle {name}", got, ref, img32)
    tab = K.image_branches(render, ref, keep, with_lights=name.startswith("lights"))
    TABLE["image"][name] = tab
    print(f"core_ref coverage {name}: " + ", ".join(f"{k} {v}" for k, v in tab.items() if v))


@pytest.mark.parametrize("name", list(IMAGES))
def test_x86_kernel_headers_image_against_float64(oracle_mod, emu_mod, name):
    render, holder, ref, img32 = image_case(name)
    one, _ = emu_mod.render(holder, 1, 1)
    two, _ = emu_mod.render(holder, 1, 2)
    two_samples_are_twice_one(one, two, ref)
    K.compare_image(f"x86 kernel headers {name}", two / f32(2), ref, img32, oracle_mean=oracle_image(oracle_mod, holder, ref).astype(np.float64))


def test_boxed_light_is_never_lit():
    """A point light inside a box: every shadow ray towards it meets the box (from inside too: t0 < 0 is a hit), so the float64
    fold never sees it, anywhere in either frame."""
    for name in ("lights/view0", "lights/view1"):
        ref = image_case(name)[2]
        assert not ref["vis"][0][K.BOXED_LIGHT].any()
        assert ref["items"][0][0].sum() > 1000


# ---- rays ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RAY_SCENES))
def test_oracle_ray_query_against_float64(oracle_mod, name):
    render, holder, o, d = ray_case(name)
    orc = oracle_mod.Oracle(holder, seed=1)
    words = orc.ray_query(o, d)
    orc.close()
    h, ok = K.compare_words(f"oracle {name}", words, o, d, render)
    TABLE["rays"][name] = K.ray_branches(render, h, ok)


@pytest.mark.parametrize("name", list(RAY_SCENES))
def test_x86_ray_query_body_against_float64(probe, oracle_mod, name):
    from micro_raytracer_amd import _lib
    render, holder, o, d = ray_case(name)
    feat = _lib.plan_launch(holder)["kernel_features"]
    words, _ = Q.probe_trace(probe, holder, Q.Variant("default plan", feat).cfg(), o, d)
    orc = oracle_mod.Oracle(holder, seed=1)
    ref = orc.ray_query(o, d)
    orc.close()
    K.compare_words(f"x86 ray-query body {name} (FEAT {feat})", words, o, d, render, oracle_words=ref)


@functools.lru_cache(maxsize=None)
def edge_case():
    desc = K.primitives()
    render, holder = make_holder(desc)
    o, d = K.edge_strip_rays(desc, 9)
    return render, holder, o, d


def test_box_edge_strips_oracle_and_x86_take_the_z_face(probe, oracle_mod):
    """Where p.z lies inside 1 +- E on an upright face, the `} if` of src/rt.rs:435 makes the normal the z face's.  The image and
    ray rules above exclude box edges (their margin is stated against the window's ends); these rays sit in the MIDDLE of the
    window instead, and are held to the float64 normal under a margin of their own (core_cases.compare_edge_words)."""
    from micro_raytracer_amd import _lib
    render, holder, o, d = edge_case()
    orc = oracle_mod.Oracle(holder, seed=1)
    K.compare_edge_words("oracle, box edge strips", orc.ray_query(o, d), o, d, render)
    orc.close()
    feat = _lib.plan_launch(holder)["kernel_features"]
    words, _ = Q.probe_trace(probe, holder, Q.Variant("default plan", feat).cfg(), o, d)
    K.compare_edge_words(f"x86 ray-query body (FEAT {feat}), box edge strips", words, o, d, render)


def test_ray_sets_hold_what_they_are_meant_to(oracle_mod):
    """Origins inside the large box and inside a sphere, the fold's own shadow rays, no pathological input."""
    for name in RAY_SCENES:
        render, holder, o, d = ray_case(name)
        assert np.isfinite(o).all() and np.isfinite(d).all() and not Q.wild(o, d).any()
        assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)
        h = R.closest_hit(render, o, d)
        if name == "primitives":
            assert (h["hit"] & (h["t0"] < 0)).sum() >= 500         # from inside the large box


# ---- coverage: the conditions that keep the tests above from hiding a failure ----------------------------------------------------------------
def test_every_branch_is_compared(oracle_mod):
    """Compared pixels per branch over all frames, tame rays per branch over both ray sets: each >= 100.  The masks are properties
    of the float64 answer alone."""
    for name in IMAGES:
        if name not in TABLE["image"]:
            render, holder, ref, img32 = image_case(name)
            _, _, keep = K.masks(ref)
            TABLE["image"][name] = K.image_branches(render, ref, keep, with_lights=name.startswith("lights"))
    for name in RAY_SCENES:
        if name not in TABLE["rays"]:
            render, holder, o, d = ray_case(name)
            h, ok = R.ray_words(render, o, d)
            TABLE["rays"][name] = K.ray_branches(render, h, ok)
    for kind, wanted in (("image", K.IMAGE_BRANCHES), ("rays", K.RAY_BRANCHES)):
        total = {}
        for tab in TABLE[kind].values():
            for k, v in tab.items():
                total[k] = total.get(k, 0) + v
        K.print_branches("compared pixels" if kind == "image" else "tame rays", total, wanted)
    lit = sum(t.get(f"light {K.BOXED_LIGHT} lit", 0) for t in TABLE["image"].values())
    assert lit == 0
