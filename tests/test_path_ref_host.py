"""The stochastic path against a float64 restatement of the reference, CPU side: the oracle (orc_path_key / orc_draw_*,
Oracle.trace_pixel) and the x86 build of the kernel headers (emu.render at a sample base, the per-ray body of mrt_radiance) against
tests/path_ref.py on the scenes of tests/path_cases.py, under the rules stated there ("the stochastic path").  Oracle,
kernel headers and path_ref are three readings of src/rt.rs and of DESIGN.md §5; path_ref shares no code with the other two."""
import numpy as np
import pytest

import path_cases as C
import path_ref as P
import rays_ref as Y

f32 = np.float32
TABLE = {}


# ---- DESIGN.md §5 ----------------------------------------------------------------------------------------------------------------------
def rng_tuples():
    """(seed, pixel, sample, dim) tuples: random ones plus seeds with a nonzero high word, pixel + seed_lo wrapping past 2^32 and
    sample counts near 2^32."""
    rng = np.random.default_rng(11)
    n = 3000
    seed = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    seed[:300] &= np.uint64(0xFFFFFFFF)                               # high word 0
    pixel = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    pixel[300:900] = rng.integers(0, 1 << 21, 600)
    wrap = slice(900, 1500)                                          # pixel + seed_lo >= 2^32
    pixel[wrap] = (np.uint64(2 ** 32) - (seed[wrap] & np.uint64(0xFFFFFFFF)) + rng.integers(0, 1 << 16, 600).astype(np.uint64)).astype(np.uint32)
    pixel[900], seed[900] = np.uint32(0xFFFFFFFF), np.uint64((7 << 32) | 0xFFFFFFFF)
    sample = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    sample[1500:2100] = (2 ** 32 - 1 - rng.integers(0, 64, 600)).astype(np.uint32)
    sample[2100:2400] = rng.integers(0, 4096, 300)
    dim = rng.integers(0, 2 + 8 * 64, n).astype(np.uint32)
    dim[:100] = np.arange(100)
    assert ((seed >> np.uint64(32)) != 0).sum() > 2000 and (sample >= 2 ** 32 - 64).sum() >= 600
    assert ((pixel[wrap].astype(np.uint64) + (seed[wrap] & np.uint64(0xFFFFFFFF))) >= 2 ** 32).all()
    return seed, pixel, sample, dim


def test_rng_restatement_equals_the_oracle_bit_for_bit(oracle_mod):
    seed, pixel, sample, dim = rng_tuples()
    L = oracle_mod.lib()
    pk = P.path_key((seed & np.uint64(0xFFFFFFFF)).astype(np.uint32), (seed >> np.uint64(32)).astype(np.uint32), pixel, sample)
    u = P.draw_u32(pk, dim)
    for T in (np.float32, np.float64):
        assert P.uniform(u, T).dtype == T
    want_pk = np.array([oracle_mod.path_key(int(s), int(p), int(k)) for s, p, k in zip(seed, pixel, sample)], np.uint32)
    assert np.array_equal(pk, want_pk)
    want_u = np.array([oracle_mod.draw_u32(int(k), int(d)) for k, d in zip(want_pk, dim)], np.uint32)
    assert np.array_equal(u, want_u)
    want_f = np.array([L.orc_draw_f32(int(k), int(d)) for k, d in zip(want_pk, dim)], np.float32)
    assert np.array_equal(P.uniform(u, np.float32).view(np.uint32), want_f.view(np.uint32))
    assert np.array_equal(P.uniform(u, np.float64), want_f.astype(np.float64))
    assert P.uniform(u).max() < 1.0 and np.array_equal(P.uniform(np.uint32([0, 511, 512, 2 ** 32 - 1])), [0.0, 0.0, 2.0 ** -23, 1.0 - 2.0 ** -23])


def test_bernoulli_thresholds():
    """p in {0, 2^-32, 0.8, 0.85, 1 - 2^-24, 1} against u in {0, threshold - 1, threshold, 2^32 - 1}: true below the threshold
    floor(p 2^32), false from it on, p == 1 always true.  0.8 is the f64 literal (threshold floor(0.8 2^32) = 3435973836), 0.85 the
    float32 number widened (3650722304, not floor(0.85 2^32) = 3650722201)."""
    top = 2 ** 32 - 1
    for p, thr in ((0.0, 0), (2.0 ** -32, 1), (0.8, 3435973836), (float(f32(0.85)), 3650722304), (1.0 - 2.0 ** -24, 2 ** 32 - 256), (1.0, None)):
        if thr is None:
            assert P.bernoulli(p, np.uint32([0, 1, top])).all()
            continue
        assert int(P.threshold(p)) == thr, (p, int(P.threshold(p)))
        us = sorted({0, max(thr - 1, 0), thr, top})
        assert P.bernoulli(p, np.uint32(us)).tolist() == [u < thr for u in us], (p, us)
    assert float(P.p_transmit(f32(0.0))) == float(f32(0.85)) and float(P.p_transmit(f32(0.4))) == float(f32(1.0) - f32(0.4))
    assert float(P.p_transmit(f32(1.0))) == 0.0 and float(P.p_emit(0.25)) == 0.25
    assert int(P.threshold(0.85)) == 3650722201


def test_vec_refract_and_rand_dir_pieces():
    """Vec3f::refract at normal incidence passes straight through for any eta; at eta 1.5 from inside (cos = -n . d < 0) it fails
    beyond asin(1 / 1.5); rand with r = 0 is n; |n + r v| is returned as the degenerate margin."""
    d = np.array([[0.0, 1.0, 0.0], [0.8, 0.6, 0.0], [0.6, 0.8, 0.0]])
    n = np.array([[0.0, 1.0, 0.0]] * 3)
    out, ok, k = P.vec_refract(d, np.full(3, 1.5), n)
    assert ok.tolist() == [True, False, True]                          # sin = 0.8 > 2/3 fails, 0.6 < 2/3 passes
    assert np.allclose(out[0] / np.linalg.norm(out[0]), [0, -1, 0]) or np.allclose(out[0] / np.linalg.norm(out[0]), [0, 1, 0])
    assert np.allclose(k, np.abs(1 - 2.25 * (1 - np.array([1.0, 0.36, 0.64]))) / 2.25)
    nn, mag = P.rand_dir(n, np.zeros(3), np.array([0.1, 0.5, 0.9]), np.array([0.2, 0.4, 0.6]))
    assert np.array_equal(nn, n) and np.array_equal(mag, np.ones(3))
    nn, mag = P.rand_dir(n[:1], np.ones(1), np.array([0.5]), np.array([0.75]))      # v = (0, -1, 0) up to rounding: n + v ~ 0
    assert mag[0] < 1e-6


# ---- per-sample radiance ---------------------------------------------------------------------------------------------------------------
def oracle_samples(oracle_mod, c):
    orc = oracle_mod.Oracle(c["holder"], seed=C.SEED)
    nh, nw = c["shape"]
    assert (orc.nh, orc.nw) == (nh, nw)
    got = np.array([orc.trace_pixel(int(p) % nw, int(p) // nw, int(s))[0] for p, s in zip(c["pixel"], c["sample"])], np.float32)
    orc.close()
    return got


@pytest.mark.parametrize("name", list(C.CASES))
def test_oracle_samples_against_float64(oracle_mod, name):
    c = C.case(name)
    C.compare("oracle", c, oracle_samples(oracle_mod, c))
    TABLE[name] = C.branches(c)


def x86_samples(emu_mod, c):
    """Sample s of every pixel alone: one emu.render of one sample at sample base s into a zeroed accumulator."""
    return np.stack([emu_mod.render(c["holder"], C.SEED, 1, sample_base=s)[0] for s in range(C.SAMPLES)])


@pytest.mark.parametrize("name", list(C.CASES))
def test_x86_kernel_headers_samples_against_float64(emu_mod, name):
    c = C.case(name)
    C.compare("x86 kernel headers", c, x86_samples(emu_mod, c))


@pytest.mark.parametrize("name", ["diffuse_room", "lens/aprt0.5_b0"])
def test_x86_kernel_headers_sample_zero_of_other_seeds(emu_mod, name):
    """emu.render(h, seed, 1) is sample 0 at that seed: seeds with a zero and a nonzero high word, one sample each."""
    c = C.case(name)
    nh, nw = c["shape"]
    pixel, sample = np.arange(nh * nw, dtype=np.uint32), np.zeros(nh * nw, np.uint32)
    for seed in (3, (9 << 32) | 3):
        o, d = P.camera_paths(c["render"], seed, pixel, sample)
        ref = P.trace_sample(c["render"], seed, pixel, sample, o, d)
        o32, d32 = P.camera_paths(c["render"], seed, pixel, sample, np.float32)
        cc = {"name": f"{name} seed {seed:#x}", "ref": ref, "keep": P.sound(ref["margins"]), "pixel": pixel, "sample": sample,
              "rgb32": P.trace_sample(c["render"], seed, pixel, sample, o32, d32, np.float32)["rgb"]}
        C.compare("x86 kernel headers", cc, emu_mod.render(c["holder"], seed, 1)[0])


@pytest.fixture(scope="module")
def rays_probe():
    return Y.shared_probe()


@pytest.mark.parametrize("name", C.PINHOLE)
def test_x86_radiance_body_samples_against_float64(rays_probe, name):
    """The per-ray body of mrt_radiance on the float32 primary rays, sample base s, the pixel index as the key."""
    c = C.case(name)
    nh, nw = c["shape"]
    feat = Y.x86_info(rays_probe, c["holder"])["rays_inst"]
    o, d = c["o"][:nh * nw].astype(f32), c["d"][:nh * nw].astype(f32)
    key = np.arange(nh * nw, dtype=np.uint32)
    got = np.stack([Y.x86_radiance(rays_probe, c["holder"], feat, o, d, 1, seed=C.SEED, sample_base=s, key=key) for s in range(C.SAMPLES)])
    C.compare(f"x86 radiance body (FEAT {feat})", c, got)


# ---- conditions, not measurements ------------------------------------------------------------------------------------------------------
def test_cases_reach_their_branches():
    """From path_ref in float64 and the inputs alone, no code under test involved: margins exclude at most 25 % of every case's
    samples, every branch of path_cases.BRANCHES has at least 200 compared samples over the suite, and float32 numpy itself holds
    the bar on every case (a case on which it did not would be ill-conditioned)."""
    tabs = []
    for name in C.CASES:
        c = C.case(name)
        keep = c["keep"]
        want = c["ref"]["rgb"]
        err32 = float((np.abs(c["rgb32"].astype(np.float64) - want) / np.maximum(np.abs(want), 1.0))[keep].max())
        m = c["ref"]["margins"]
        print(f"path_ref case {name}: {keep.size} samples, excluded {int((~keep).sum())} ({(~keep).mean():.1%}), float32 numpy {err32:.2e}; items per path "
              f"{np.bincount(c['ref']['depth']).tolist()}; smallest compared tir {m['tir'][keep].min():.2e}, degenerate {m['degenerate'][keep].min():.2e}")
        assert np.isfinite(want).all()
        assert (~keep).sum() <= C.MAX_EXCLUDED * keep.size, (name, int((~keep).sum()))
        assert err32 <= C.BAR, (name, err32)
        tabs.append(C.branches(c))
    C.print_branches("compared samples", C.total_branches(tabs))


# ---- coin frequencies: the statistics of the contract's own hash ---------------------------------------------------------------------------
def contract_heads(name):
    """The coin of frequency scene `name` from path_ref's RNG alone: (heads, p, sound), bool [samples][pixels].  sound: the samples
    whose value float32 arithmetic cannot change -- all of them, but in the 80 % scene the scattered directions that leave the wall
    flatter than path_ref's rule for leaving rays allows (|cos| < SIGN S / E, S = |hit point| + |wall pos|: the ray starts E |cos|
    off the wall, less than the float32 error of the hit point, and may meet the wall again or pass it on either side)."""
    desc, p = C.freq_scenes()[name][:2]
    n = C.FREQ_RES[0] * C.FREQ_RES[1]
    pixel = np.tile(np.arange(n, dtype=np.uint32), C.FREQ_SAMPLES)
    sample = np.repeat(np.arange(C.FREQ_SAMPLES, dtype=np.uint32), n)
    pk = P.path_key(C.FREQ_SEED & 0xFFFFFFFF, C.FREQ_SEED >> 32, pixel, sample)
    slot = lambda k: P.draw_u32(pk, P.DIM_BOUNCE0 + k)
    sound = np.ones(pixel.size, bool)
    if name == "emit":
        heads = P.bernoulli(P.p_emit(f32(0.3)), slot(P.EMIT_COIN))
    elif name == "transmit":
        heads = P.bernoulli(P.p_transmit(f32(0.5)), slot(P.OPAC_COIN))
    else:
        from conftest import make_holder
        render, _ = make_holder(desc)
        wall = render.scene.renderer[0]
        pos, nrm = np.asarray(wall.inst[0][0], np.float64), np.asarray(wall.n, np.float64)
        o, d = P.lens_rays(render, pixel, np.zeros(pixel.size), np.zeros(pixel.size))
        hit = o + d * (P.R.dot(pos - o, nrm) / P.R.dot(d, nrm))[:, None]
        nn, _ = P.rand_dir(np.broadcast_to(nrm, d.shape), np.ones(pixel.size), P.uniform(slot(P.REFL_U1)), P.uniform(slot(P.REFL_U2)))
        cos = P.R.dot(P.R.reflect(d, nn), nrm)
        fired = P.bernoulli(P.P_DIFFUSE, slot(P.REFL_COIN))
        heads = fired & (cos < 0)
        sound = ~fired | (np.abs(cos) >= (np.linalg.norm(hit, axis=1) + np.linalg.norm(pos)) * (P.R.SIGN / P.R.E32))
    return heads.reshape(C.FREQ_SAMPLES, n), p, sound.reshape(C.FREQ_SAMPLES, n)


@pytest.mark.parametrize("name", ["emit", "transmit", "diffuse"])
def test_contract_hash_holds_the_frequency_bounds(name):
    heads, p, sound = contract_heads(name)
    C.freq_check(f"path_ref RNG, {name}", heads, p)
    assert sound.mean() >= 0.9


@pytest.mark.parametrize("name", ["emit", "transmit", "diffuse"])
def test_frequency_scenes_take_their_two_values(emu_mod, name):
    """The first 4 samples of a frequency scene, from path_ref.trace_sample and from the x86 kernel headers: every pixel takes one
    of the two values the scene's docstring derives, and the side of the split is the coin contract_heads computes (on its sound
    samples)."""
    from conftest import make_holder
    desc, p, side, channel, split, values = C.freq_scenes()[name]
    render, holder = make_holder(desc)
    n = C.FREQ_RES[0] * C.FREQ_RES[1]
    pixel, sample = np.tile(np.arange(n, dtype=np.uint32), 4), np.repeat(np.arange(4, dtype=np.uint32), n)
    o, d = P.camera_paths(render, C.FREQ_SEED, pixel, sample)
    ref = P.trace_sample(render, C.FREQ_SEED, pixel, sample, o, d)["rgb"][:, channel].reshape(4, n)
    x86 = np.stack([emu_mod.render(holder, C.FREQ_SEED, 1, sample_base=s)[0] for s in range(4)])[..., channel].reshape(4, n).astype(np.float64)
    want, _, sound = contract_heads(name)
    want, sound = want[:4], sound[:4]
    for label, got in (("path_ref", ref), ("x86 kernel headers", x86)):
        heads = (got > split) if side > 0 else (got < split)
        assert np.abs(got - np.where(heads, values[0], values[1]))[sound].max() <= 1e-6, (label, np.unique(np.round(got, 4)))
        assert np.array_equal(heads[sound], want[sound]), (label, int((heads != want).sum()))
