"""mrt_radiance on the GPU against the oracle and the x86 build, on rays no pinhole camera forms: the cases of
tests/radiance_cases.py, each on a context created under the environment that puts its scene in LDS or behind L2, so that all
sixteen pt_rays kernels answer at least one case.  Per case and context: mrt_rays_info names the kernel the table
expects; the sums are the x86 probe's bits, NaN bits included; the segment counter is the probe's total and the oracle's count
under the kernel's stop rule; and the sums meet the oracle under the rule of tests/test_radiance_oracle_host.py, no exclusions.

What the x86 build cannot show and these tests can: the wave votes of the fast division and sqrt cores inside shading when a
wavefront holds wild lanes, the LDS copy of the scene, the spills and scratch of the F_BVH kernels, the L2 path.  The wavefront of
a ray is chosen by its index: ray i is lane i % 64 of wavefront i / 64."""
import os

import numpy as np
import pytest

import radiance_cases as RC
import rayq_cases as Q
import rays_ref as Y
import test_radiance_oracle_host as H
from conftest import make_holder

pytestmark = pytest.mark.gpu
f32 = np.float32
SEED = H.SEED
SEEN = {}          # (FEAT, scene in LDS) -> the cases that ran on that kernel


@pytest.fixture(scope="module")
def probe():
    return Y.shared_probe()


class Ctx:
    """A Sampler created under a run's environment (read once, in mrt_create)."""

    def __init__(self, monkeypatch, render, env):
        from micro_raytracer_amd import Sampler
        for k in [k for k in os.environ if k.startswith("MRT_")]:
            monkeypatch.delenv(k)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        self.render = render
        self.s = Sampler(seed=SEED, device=0)
        self.s.create(render)
        for k in env:
            monkeypatch.delenv(k)

    def radiance(self, o, d, ns, base=0, key=None):
        info = {}
        got = self.s.radiance(self.render, o, d, ns, sample_base=base, key=key, info=info)
        return got, info

    def close(self):
        self.s.close()


@pytest.mark.parametrize("name", H._case_names())
def test_case_on_the_gpu_equals_the_x86_probe_and_meets_the_oracle(probe, oracle_mod, monkeypatch, name):
    case = RC.case(name, oracle_mod)
    render, holder = make_holder(case.desc)
    assert H.excluded(case).sum() == 0
    n = len(case.o)
    x86 = {(base, ns): Y.x86_radiance(probe, holder, case.feat, case.o, case.d, ns, seed=SEED, sample_base=base, segments=True) for base, ns in RC.RANGES}
    for run in case.runs:
        c = Ctx(monkeypatch, render, run.env)
        for base, ns in RC.RANGES:
            got, info = c.radiance(case.o, case.d, ns, base)
            # the call ran the kernel this run is about: a case cannot pass on the wrong one
            assert (info["kernel_features"], info["scene_in_lds"]) == (case.feat, int(run.lds)), (name, run.label, info)
            want, seg = x86[(base, ns)]
            ref, rseg = H.oracle_sums(oracle_mod, holder, case, base, ns, False)
            diff = np.flatnonzero((RC.bits(got) != RC.bits(want)).any(axis=1))
            bad, worst, same, nonfin = RC.compare(got, ref, ns)
            print(f"radiance on the GPU: {name:44s} {run.label:10s} FEAT {info['kernel_features']:4d} in LDS {info['scene_in_lds']} ({info['lds_bytes']:6d} B) "
                  f"samples [{base}, +{ns}) rays {n:4d} non-finite {nonfin:3d} differ from x86 {diff.size} worst vs oracle {worst:.2e} bit-identical {same:.4f} "
                  f"segments {info['segments']} (x86 {seg}, oracle {int(rseg.sum())}) {info['kernel_ms']:.3f} ms")
            assert diff.size == 0, (name, run.label, base, ns, [(int(i), case.o[i], case.d[i], got[i], want[i]) for i in diff[:3]])
            assert info["segments"] == seg == int(rseg.sum()), (name, run.label, base, ns)
            assert bad.size == 0, (name, run.label, base, ns, [(int(i), case.o[i], case.d[i], got[i], ref[i]) for i in bad[:3]])
        c.close()
        SEEN.setdefault((case.feat, run.lds), []).append(f"{name} [{run.label}]")


def test_wavefront_composition_changes_no_bit(probe, oracle_mod, monkeypatch):
    """The same rays, keyed by their original index, in three orders: (a) tame rays packed into whole wavefronts, then the wild
    ones; (b) one wild ray in lane w % 64 of every wavefront w; (c) reversed.  A wild lane switches its wavefront to the full
    division and sqrt expansions; the tame lanes beside it must not change a bit.  Scattered back, every ray's three words are
    the same in all three orders, and the x86 probe's."""
    case = RC.case("surface/kitchen_sink", oracle_mod)
    render, holder = make_holder(case.desc)
    o, d = case.o, case.d
    n = len(o)
    wild = Q.wild(o, d)
    ti, wi = np.flatnonzero(~wild), np.flatnonzero(wild)
    assert len(wi) >= 100 and len(ti) >= 2000
    pad = (-len(ti)) % 64
    order_a = np.concatenate([ti, ti[:pad], wi])
    assert not wild[order_a[:len(ti) + pad]].any()
    rows = []
    for w in range((len(ti) + 62) // 63):
        lanes = list(ti[w * 63:(w + 1) * 63])
        lanes.insert(min(w % 64, len(lanes)), wi[w % len(wi)])
        rows.append(np.array(lanes))
    order_b = np.concatenate(rows + [wi])
    wave_of = np.arange(len(order_b)) // 64
    assert all(wild[order_b[wave_of == w]].any() for w in range(wave_of.max() + 1))
    order_c = np.arange(n)[::-1]
    ns = 24
    want = Y.x86_radiance(probe, holder, case.feat, o, d, ns, seed=SEED, sample_base=7, key=np.arange(n))
    c = Ctx(monkeypatch, render, case.runs[0].env)
    results = []
    for label, order in (("a", order_a), ("b", order_b), ("c", order_c)):
        assert len(order) <= 2 * RC.MAX_RAYS and set(order.tolist()) == set(range(n))
        got, info = c.radiance(o[order], d[order], ns, 7, key=order.astype(np.uint32))
        assert (info["kernel_features"], info["scene_in_lds"]) == (case.feat, 1)
        back = np.zeros((n, 3), np.uint32)
        back[order] = RC.bits(got)
        assert np.array_equal(back[order], RC.bits(got)), label                # repeats of a ray agree with each other as well
        results.append(back)
    c.close()
    for label, back in zip("abc", results):
        diff = np.flatnonzero((back != RC.bits(want)).any(axis=1))
        assert diff.size == 0, (label, [(int(i), o[i], d[i], back[i], RC.bits(want)[i]) for i in diff[:3]])
    print(f"radiance on the GPU, wavefront composition: {n} rays, {len(wi)} wild; {(len(ti) + pad) // 64} tame wavefronts in (a), {len(rows)} with one wild "
          f"lane in (b), reversed in (c): equal words, the x86 probe's")


@pytest.mark.parametrize("name", ["surface/kitchen_sink", "ties/coincident_bvh"])
def test_partial_batches_keep_every_rays_bits(oracle_mod, monkeypatch, name):
    """Threads >= n stay out of the body and of every wave vote: the first n rays alone give the bits they have in the full batch."""
    case = RC.case(name, oracle_mod)
    render, _ = make_holder(case.desc)
    c = Ctx(monkeypatch, render, case.runs[0].env)
    whole, info = c.radiance(case.o, case.d, 24, 7)
    assert (info["kernel_features"], info["scene_in_lds"]) == (case.feat, 1)
    for n in (1, 63, 65, 257):
        part, _ = c.radiance(case.o[:n], case.d[:n], 24, 7)
        assert part.shape == (n, 3) and np.array_equal(RC.bits(part), RC.bits(whole[:n])), (name, n)
    c.close()


def test_every_pt_rays_kernel_answered_a_case():
    """After the case tests (file order): each of the sixteen (FEAT, scene in LDS) kernels of MRT_RAYS_LIST ran at least one case, on
    a call whose mrt_rays_info reported it."""
    if len(SEEN) == 0:
        pytest.skip("the case tests did not run in this session")
    want = [(f, lds) for f in RC.FEATS for lds in (True, False)]
    assert len(want) == 16
    for k in want:
        print(f"radiance on the GPU: pt_rays FEAT {k[0]:4d} scene in {'LDS' if k[1] else 'L2 '}: {', '.join(SEEN.get(k, []))}")
    assert [k for k in want if k not in SEEN] == []
