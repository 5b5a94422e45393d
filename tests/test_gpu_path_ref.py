"""The stochastic path on the GPU against a float64 restatement of the reference: per-sample radiance through the pt_rays kernels
(Sampler.radiance on Sampler.camera_rays, one sample at sample base s, the pixel index as the key) and through the megakernel
(Sampler.execute of one sample into a zeroed accumulator whose count is s: the only route that runs the lens), against
tests/path_ref.py on the scenes of tests/path_cases.py, under the rules stated there and shared with tests/test_path_ref_host.py
("the stochastic path").  One glass case and one map case run once more with the scene read through L2.  Then the
frequencies of the emit, transmission and 80 % coins over 4096 samples of 32 x 32 pixels against closed forms.  Every test prints
its worst error next to what plain float32 numpy carries on the same formulas."""
import os

import numpy as np
import pytest

import path_cases as C
import test_path_ref_host as H

pytestmark = pytest.mark.gpu
f32 = np.float32
L2 = {"MRT_SCENE_IN_L2": "1"}
TABLE = {}


class Ctx:
    """A Sampler of seed `seed` whose context is created under env (read once, in mrt_create); reused across samples."""

    def __init__(self, monkeypatch, render, env, seed):
        from micro_raytracer_amd import Sampler
        for k in [k for k in os.environ if k.startswith("MRT_")]:
            monkeypatch.delenv(k)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        self.render = render
        self.s = Sampler(seed=seed, device=0)
        self.s.create(render)
        for k in env:
            monkeypatch.delenv(k)
        self.stats = self.s.stats()
        assert bool(self.stats["scene_in_lds"]) == ("MRT_SCENE_IN_L2" not in env), self.stats
        self.where = f"kernel_features {self.stats['kernel_features']}, {self.stats['block_threads']} threads, scene_in_lds {self.stats['scene_in_lds']}"

    def megakernel_samples(self, n):
        """Sample s of every pixel alone, s < n: the accumulator is replaced by zeros with count s, then one sample is executed."""
        zero = np.zeros((self.s.nh, self.s.nw, 3), f32)
        out = []
        for s in range(n):
            self.s.set_accum(zero, s)
            self.s.execute(self.render, n_samples=1)
            acc, cnt = self.s.accum()
            assert cnt == s + 1
            out.append(acc.copy())
        return np.stack(out)

    def radiance_samples(self, n):
        o, d = self.s.camera_rays(self.render)
        key = np.arange(self.s.nh * self.s.nw, dtype=np.uint32).reshape(self.s.nh, self.s.nw)
        info = {}
        out = np.stack([self.s.radiance(self.render, o, d, 1, sample_base=s, key=key, info=info) for s in range(n)])
        return out, o, d, info

    def close(self):
        self.s.close()


@pytest.mark.parametrize("name", C.PINHOLE)
def test_gpu_radiance_samples_against_float64(monkeypatch, name):
    c = C.case(name)
    g = Ctx(monkeypatch, c["render"], {}, C.SEED)
    got, o, d, info = g.radiance_samples(C.SAMPLES)
    g.close()
    n = o.size // 3
    # the rays the kernel was given are the float64 primary rays, to float32
    assert np.abs(o.reshape(-1, 3) - c["o"][:n]).max() <= 1e-6 and np.abs(d.reshape(-1, 3) - c["d"][:n]).max() <= 1e-6
    C.compare(f"GPU pt_rays (kernel_features {info['kernel_features']}, scene_in_lds {info['scene_in_lds']})", c, got)
    TABLE[name] = C.branches(c)


@pytest.mark.parametrize("name", list(C.CASES))
def test_gpu_megakernel_samples_against_float64(monkeypatch, name):
    c = C.case(name)
    g = Ctx(monkeypatch, c["render"], {}, C.SEED)
    got = g.megakernel_samples(C.SAMPLES)
    g.close()
    C.compare(f"GPU megakernel ({g.where})", c, got)
    TABLE[name] = C.branches(c)


@pytest.mark.parametrize("name", ["glass", "omap_emap"])
def test_gpu_samples_through_l2_against_float64(monkeypatch, name):
    c = C.case(name)
    g = Ctx(monkeypatch, c["render"], L2, C.SEED)
    got = g.megakernel_samples(C.SAMPLES)
    rays, _, _, info = g.radiance_samples(C.SAMPLES)
    g.close()
    assert info["scene_in_lds"] == 0
    C.compare(f"GPU megakernel, scene through L2 ({g.where})", c, got)
    C.compare(f"GPU pt_rays, scene through L2 (kernel_features {info['kernel_features']})", c, rays)


# ---- coin frequencies against closed forms (path_cases.freq_scenes, freq_check: each sigma is derived there from n and p) ------------------
@pytest.mark.parametrize("name", ["emit", "transmit", "diffuse"])
def test_gpu_coin_frequencies(monkeypatch, name):
    """4096 samples of 32 x 32 pixels through Sampler.radiance, read back in 64 chunks of 64 one-sample calls (a call returns the
    SUM of its samples, so the per-sample coins that the lag-1 statistic needs take one call each).  Total within 5 sigma of the
    binomial, chi-square of the per-pixel counts within 5 sigma of its mean, lag-1 autocorrelation over the sample index within 5
    sigma of zero; the contract's own hash holds the same bounds on the CPU (test_contract_hash_holds_the_frequency_bounds), and
    the GPU's coins are the contract's coins and its values the scene's two values, sample by sample, on every sample contract_heads
    calls sound (all but the 80 % scene's scattered directions too flat along the wall to leave it soundly, ~5 %)."""
    from conftest import make_holder
    desc, p, side, channel, split, values = C.freq_scenes()[name]
    render, _ = make_holder(desc)
    g = Ctx(monkeypatch, render, {}, C.FREQ_SEED)
    o, d = g.s.camera_rays(render)
    n = o.size // 3
    assert n == 1024
    key = np.arange(n, dtype=np.uint32).reshape(o.shape[:2])
    heads = np.zeros((C.FREQ_SAMPLES, n), bool)
    off = np.zeros((C.FREQ_SAMPLES, n), bool)
    for chunk in range(64):
        vals = np.stack([g.s.radiance(render, o, d, 1, sample_base=64 * chunk + k, key=key) for k in range(64)])[..., channel].reshape(64, n)
        h = (vals > split) if side > 0 else (vals < split)
        heads[64 * chunk:64 * chunk + 64] = h
        off[64 * chunk:64 * chunk + 64] = np.abs(vals.astype(np.float64) - np.where(h, values[0], values[1])) > 1e-6
    g.close()
    C.freq_check(f"GPU, {name}", heads, p)
    want, _, sound = H.contract_heads(name)
    differ = ((heads != want) | off) & sound
    print(f"path_ref coin frequencies GPU {name}: sound samples {int(sound.sum())} of {sound.size}; among them off the scene's two values "
          f"{int((off & sound).sum())}, coin differs from the contract's own {int(((heads != want) & sound).sum())}; among the others {int((off & ~sound).sum())} and "
          f"{int(((heads != want) & ~sound).sum())}")
    assert differ.sum() == 0 and sound.mean() >= 0.9


def test_gpu_every_branch_was_compared():
    """Compared samples per branch over the tests above, each >= 200 (a case that did not run in this session is counted from its
    margins, which are properties of the float64 answer alone)."""
    for name in C.CASES:
        if name not in TABLE:
            TABLE[name] = C.branches(C.case(name))
    C.print_branches("GPU, compared samples", C.total_branches(TABLE.values()))
