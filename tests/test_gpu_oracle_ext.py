"""The extension features on the GPU against the CPU oracle (oracle/mrt_oracle.c orc_create_ext, written from the contract text
of DESIGN.md §14-§16): the scenes of tests/test_oracle_ext.py through Sampler at the plan's default shape, whole frames, the
project's bar of 1e-4 per-channel L-inf on the mean radiance, image bytes identical when the oracle is fed the GPU's
accumulator.  The staging levels are bit-identical to one another (tests/test_gpu_vattr.py, test_gpu_env.py, test_gpu_filter.py),
so one level per scene is enough; scenes 2 and 5 run once more with the scene read through L2."""
import numpy as np
import pytest

from conftest import make_holder
from micro_raytracer_amd._abi import F_BVH, F_ENV, F_VATTR
from test_oracle_ext import SCENES, compare, oracle_render

pytestmark = pytest.mark.gpu

ENV_FAMILY = {n for n in SCENES if n.startswith("env_")} | {"maps_bilinear", "matfilter_noenv"}      # an environment, or filtered maps


@pytest.fixture(scope="module")
def refs(oracle_mod):
    """(render, oracle, reference accumulator) per (scene, seed): computed once, shared by the two tests, never changed."""
    cache = {}

    def get(name, seed):
        if (name, seed) not in cache:
            build, spp, _ = SCENES[name]
            render, holder = make_holder(build())
            o, ref = oracle_render(oracle_mod, holder, seed, spp)
            ref.setflags(write=False)
            cache[(name, seed)] = (render, o, ref)
        return cache[(name, seed)]

    return get


def _check(name, seed, refs, label, expect_lds):
    from micro_raytracer_amd import Sampler
    spp = SCENES[name][1]
    render, o, ref = refs(name, seed)
    s = Sampler(seed=seed)
    s.execute(render, n_samples=spp)
    got, cnt = s.accum()
    st = s.stats()
    ss, img = s.img_ss(), s.img()
    s.close()
    kf = st["kernel_features"]
    assert cnt == spp and kf & F_VATTR and bool(kf & F_ENV) == (name in ENV_FAMILY) and bool(kf & F_BVH) == name.endswith("_crowd"), (name, kf)
    if expect_lds is not None:
        assert bool(st["scene_in_lds"]) == expect_lds, st
    compare(f"{name} seed {seed} {label} (features {kf}, {st['block_threads']} threads, scene in {'LDS' if st['scene_in_lds'] else 'L2'})", got, ref, spp)
    # Sampler::img: identical bytes from identical accumulators
    o.set_accum(got, cnt)
    assert np.array_equal(ss, o.img_ss()) and np.array_equal(img, o.img()), name
    o.set_accum(ref, cnt)


@pytest.mark.parametrize("name", list(SCENES))
def test_gpu_equals_the_oracle_on_full_paths(refs, name):
    """Measured on an MI355X (DESIGN.md §3, table "extension scenes")."""
    for seed in SCENES[name][2]:
        _check(name, seed, refs, "GPU", None)


@pytest.mark.parametrize("name", ["glass_inst", "env_latlong_bilinear"])
def test_gpu_equals_the_oracle_with_the_scene_in_l2(refs, monkeypatch, name):
    monkeypatch.setenv("MRT_SCENE_IN_L2", "1")
    _check(name, 1, refs, "GPU, MRT_SCENE_IN_L2", False)
