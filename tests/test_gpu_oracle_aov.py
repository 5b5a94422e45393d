"""mrt_aov on the GPU against the CPU oracle's orc_aov (written from the contract text of DESIGN.md §13-§16; it shares no code
with csrc/mrt_denoise.h): Sampler.aov() of the 30 named scenes of tests/test_oracle_aov.py, whole frames, at the bar the x86
comparison ended with -- hit masks, renderer and instance ids equal, depth, normal and albedo bit-equal -- plus a deep-staged
mesh context (the AOV pass's second packing), a context with the scene read through L2, and several instanced renderers (the
host's mapping from the flat instance index to the index within the renderer's inst list).  The frames are the named scenes' own: 160 x 90 at the widest, 128 x 128 (cornell2, 64 x 64 at ssaa 2) the most pixels."""
import numpy as np
import pytest

import test_oracle_aov as A
from conftest import make_holder

pytestmark = pytest.mark.gpu


def gpu_against_oracle(label, oracle_mod, desc):
    from micro_raytracer_amd import Sampler
    render, holder = make_holder(desc)
    assert render.frame.nw * render.frame.nh <= 128 * 128
    ref = A.oracle_aov(oracle_mod, holder)
    s = Sampler(seed=3, device=0)
    s.create(render)
    got = s.aov()
    s.close()
    assert set(got) == {"depth", "normal", "albedo", "renderer", "instance"}
    A.compare_aov(label + " GPU", got, ref)
    return render, got, ref


@pytest.mark.parametrize("name", A.NAMED)
def test_gpu_aov_equals_the_oracle_on_named_scenes(oracle_mod, name):
    """Measured on an MI355X ("AOVs against the oracle")."""
    _, got, ref = gpu_against_oracle(name, oracle_mod, A.named_scenes()[name]())
    assert (ref["renderer"] >= 0).any()


def test_gpu_aov_equals_the_oracle_deep_staged(oracle_mod, monkeypatch):
    """MRT_DEEP_NODES: the path tracer's scene has 4-wide triangle BVHs, the AOV pass packs the scene a second time."""
    from micro_raytracer_amd import _lib, scenes
    monkeypatch.setenv("MRT_DEEP_NODES", "64")
    desc = scenes.smooth_mesh_scene(res=(53, 31), sample=4, n_tris=967)
    assert _lib.plan_launch(make_holder(desc)[0])["staging"] == "deep"
    gpu_against_oracle("smooth mesh, deep", oracle_mod, desc)


@pytest.mark.parametrize("name", ["ext:glass_inst", "ext:env_latlong_bilinear"])
def test_gpu_aov_equals_the_oracle_with_the_scene_in_l2(oracle_mod, monkeypatch, name):
    from micro_raytracer_amd import _lib
    monkeypatch.setenv("MRT_SCENE_IN_L2", "1")
    desc = A.named_scenes()[name]()
    p = _lib.plan_launch(make_holder(desc)[0])
    assert (p["staging"], p["staged_bytes"]) == ("none", 0), p
    gpu_against_oracle(name + ", MRT_SCENE_IN_L2", oracle_mod, desc)


def test_gpu_aov_instance_ids_of_several_instanced_renderers(oracle_mod):
    _, got, ref = gpu_against_oracle("multi_crowd", oracle_mod, A.multi_crowd())
    A.check_multi_crowd_ids(got)
