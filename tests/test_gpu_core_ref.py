"""The deterministic core on the GPU against a float64 restatement of the reference: Sampler.execute / accum and
_lib.selftest_trace against tests/core_ref.py on the scenes and ray sets of tests/core_cases.py, under the comparison rules stated
there and shared with tests/test_core_ref_host.py ("the deterministic core").  Contexts take the plan the scene
selects by default; the lights scene is run once more with the scene read through L2 (MRT_SCENE_IN_L2=1).  Every test prints its
worst error, what plain float32 numpy carries on the same formulas, and its L-inf against the oracle."""
import os

import numpy as np
import pytest

import core_cases as K
import core_ref as R
import test_core_ref_host as H

pytestmark = pytest.mark.gpu
f32 = np.float32
L2 = {"MRT_SCENE_IN_L2": "1"}
TABLE = {"image": {}, "rays": {}}


class Ctx:
    """A Sampler whose context is created under env (read once, in mrt_create)."""

    def __init__(self, monkeypatch, render, env):
        from micro_raytracer_amd import Sampler
        for k in [k for k in os.environ if k.startswith("MRT_")]:
            monkeypatch.delenv(k)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        self.s = Sampler(seed=1, device=0)
        self.s.create(render)
        for k in env:
            monkeypatch.delenv(k)
        self.stats = self.s.stats()
        assert bool(self.stats["scene_in_lds"]) == ("MRT_SCENE_IN_L2" not in env), self.stats

    def close(self):
        self.s.close()


def gpu_image(monkeypatch, render, ref, env):
    c = Ctx(monkeypatch, render, env)
    c.s.execute(render, n_samples=1)
    one = c.s.accum()[0].copy()
    c.s.execute(render, n_samples=1)
    two, cnt = c.s.accum()
    st = c.stats
    c.close()
    assert cnt == 2
    H.two_samples_are_twice_one(one, two, ref)
    return two / f32(2), st


def check_image(monkeypatch, oracle_mod, name, env, label):
    render, holder, ref, img32 = H.image_case(name)
    got, st = gpu_image(monkeypatch, render, ref, env)
    orc = H.oracle_image(oracle_mod, holder, ref).astype(np.float64)
    where = f"GPU {label} (kernel_features {st['kernel_features']}, {st['block_threads']} threads, scene_in_lds {st['scene_in_lds']})"
    keep = K.compare_image(f"{where} {name}", got, ref, img32, oracle_mean=orc)
    return render, ref, keep


@pytest.mark.parametrize("name", list(H.IMAGES))
def test_gpu_image_against_float64(monkeypatch, oracle_mod, name):
    render, ref, keep = check_image(monkeypatch, oracle_mod, name, {}, "default plan")
    TABLE["image"][name] = K.image_branches(render, ref, keep, with_lights=name.startswith("lights"))


@pytest.mark.parametrize("name", ["lights/view0", "lights/view1"])
def test_gpu_lights_image_through_l2_against_float64(monkeypatch, oracle_mod, name):
    check_image(monkeypatch, oracle_mod, name, L2, "scene through L2")


@pytest.mark.parametrize("name,env", [("primitives", {}), ("lights", {}), ("lights", L2)])
def test_gpu_ray_query_against_float64(monkeypatch, oracle_mod, name, env):
    from micro_raytracer_amd import _lib
    render, holder, o, d = H.ray_case(name)
    assert len(o) <= 10000
    c = Ctx(monkeypatch, render, env)
    st = c.stats
    words = _lib.selftest_trace(c.s, o, d)["words"]
    c.close()
    orc = oracle_mod.Oracle(holder, seed=1)
    ref = orc.ray_query(o, d)
    orc.close()
    assert (words[:, 0] == words[:, 1]).all()
    h, ok = K.compare_words(f"GPU {name} (kernel_features {st['kernel_features']}, scene_in_lds {st['scene_in_lds']})", words, o, d, render, oracle_words=ref)
    if not env:
        TABLE["rays"][name] = K.ray_branches(render, h, ok)


def test_gpu_box_edge_strips_take_the_z_face(monkeypatch):
    """The strips where Box::normal's z test overrides its chain (test_core_ref_host: the same rays, the same rule)."""
    from micro_raytracer_amd import _lib
    render, holder, o, d = H.edge_case()
    c = Ctx(monkeypatch, render, {})
    words = _lib.selftest_trace(c.s, o, d)["words"]
    c.close()
    K.compare_edge_words(f"GPU (kernel_features {c.stats['kernel_features']}), box edge strips", words, o, d, render)


def test_gpu_every_branch_was_compared():
    """Compared pixels and tame rays per branch over the tests above, each >= 100 (a frame or ray set that did not run in this
    session is counted from its masks, which are properties of the float64 answer alone)."""
    for name in H.IMAGES:
        if name not in TABLE["image"]:
            render, _, ref, _ = H.image_case(name)
            TABLE["image"][name] = K.image_branches(render, ref, K.masks(ref)[2], with_lights=name.startswith("lights"))
    for name in H.RAY_SCENES:
        if name not in TABLE["rays"]:
            render, _, o, d = H.ray_case(name)
            TABLE["rays"][name] = K.ray_branches(render, *R.ray_words(render, o, d))
    for kind, wanted in (("image", K.IMAGE_BRANCHES), ("rays", K.RAY_BRANCHES)):
        total = {}
        for tab in TABLE[kind].values():
            for k, v in tab.items():
                total[k] = total.get(k, 0) + v
        K.print_branches("GPU, compared pixels" if kind == "image" else "GPU, tame rays", total, wanted)
