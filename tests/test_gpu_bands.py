"""Tapered items of the band kernels change no bit.

A sample-split launch of the Cornell box's kernel family cuts its chunks into contiguous bands, long ones first.  Every chunk
sum depends on (pixel key, sample indices) alone, goes to a plane of its own and is folded in chunk order, so the accumulator
must hold the bytes of the interleaved items (MRT_K_SPLIT=4, the schedule before the bands) and of the direct launch
(MRT_K_SPLIT=1), and the launch must trace the same segments.

Frames are 44 x 20: 6 x 3 wave tiles whose right column (4 of 8 pixels) and bottom row (4 of 8 rows) are partial.  87 samples
are five full chunks and seven samples; 41 more start mid-chunk.  A frame this small tapers down to single chunks by the
rule, so the listed bands are forced through MRT_BANDS."""
import numpy as np
import pytest

from conftest import make_holder

pytestmark = pytest.mark.gpu

W, H, SEED = 44, 20, 9
OLD, DIRECT = {"MRT_K_SPLIT": "4"}, {"MRT_K_SPLIT": "1"}
NEW = [{}, {"MRT_BANDS": "3,2,1"}]                          # the rule (single chunks at this size); listed bands and single chunks
_CACHE = {}


def _desc(name):
    from micro_raytracer_amd import scenes
    if name == "cornell":
        return scenes.cornell_box(res=(W, H), sample=128, bounce=8)
    if name == "boxes":                                     # F_IDENT | F_BOX
        return scenes.cornell_box2(res=(W, H), ssaa=1, sample=128, bounce=8)
    d = scenes.instance_grid(res=(W, H), sample=128, bounce=8, n=6)      # F_BVH without lights: a crowd of 216 spheres
    d["scene"]["light"] = []
    d["scene"]["sky"] = {"color": "#8090ff", "pwr": 0.8}
    return d


def _scene(name):
    if name not in _CACHE:
        _CACHE[name] = make_holder(_desc(name))[0]
    return _CACHE[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _render(mp, name, calls, env):
    """(accumulator bits, segments of the last call, stats) of `calls` executes under `env`."""
    from micro_raytracer_amd import Sampler, _abi
    with mp.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        s = Sampler(seed=SEED, device=0, flags=_abi.FLAG_COUNT_SEGMENTS)
        seg = []
        for n in calls:
            s.execute(_scene(name), n_samples=n)
            seg.append(s.stats()["segments"])
        st = s.stats()
        a, cnt = s.accum()
        assert cnt == sum(calls)
        s.close()
    return _bits(a), seg, st


_REF = {}


def _ref(mp, name, calls, env=DIRECT):
    key = (name, calls, tuple(env.items()))
    if key not in _REF:
        b, seg, st = _render(mp, name, calls, env)
        b.setflags(write=False)
        _REF[key] = (b, seg, st)
    return _REF[key]


@pytest.mark.parametrize("calls", [(87,), (87, 41)])
def test_band_schedules_hold_the_bits_and_the_segments(calls, monkeypatch):
    ref, seg, st1 = _ref(monkeypatch, "cornell", calls)
    old, seg_old, st4 = _ref(monkeypatch, "cornell", calls, OLD)
    assert st1["k_split"] == 1 and st4["k_split"] > 1 and st1["block_threads"] == 256
    assert np.array_equal(old, ref) and seg_old == seg
    for env in NEW:
        got, seg_new, st = _render(monkeypatch, "cornell", calls, env)
        assert st["k_split"] > 1 and st["block_threads"] == 256 and st["kernel_features"] == st1["kernel_features"], st
        assert np.array_equal(got, ref), (env, int((got != ref).sum()))
        assert seg_new == seg, (env, seg_new, seg)


def test_band_launches_cut_by_max_chunks(monkeypatch):
    ref, seg, _ = _ref(monkeypatch, "cornell", (87,))
    for env in NEW:
        got, seg_new, st = _render(monkeypatch, "cornell", (87,), dict(env, MRT_MAX_CHUNKS="4"))
        assert st["launches"] == 2 and st["k_split"] > 1, st
        assert np.array_equal(got, ref) and seg_new == seg, env


@pytest.mark.parametrize("bands", ["6", "1,1,1,1,1,1", "3,2,1", "4", "2,2,2,2"])
def test_forced_bands(bands, monkeypatch):
    """A single band of all chunks, single chunks only, a taper, a band that leaves single chunks behind it, equal bands."""
    ref, seg, _ = _ref(monkeypatch, "cornell", (87, 41))
    for env in [{}]:
        got, seg_new, st = _render(monkeypatch, "cornell", (87, 41), dict(env, MRT_BANDS=bands))
        assert st["k_split"] > 1
        assert np.array_equal(got, ref) and seg_new == seg, bands


def test_band_launches_of_two_shards(monkeypatch):
    ref, _, _ = _ref(monkeypatch, "cornell", (87,))
    whole = ref.reshape(H, W, 3)
    for env in NEW:
        seen = np.zeros(H, int)
        for r in range(2):
            from micro_raytracer_amd import Sampler
            with monkeypatch.context() as m:
                for k, v in env.items():
                    m.setenv(k, v)
                s = Sampler(seed=SEED, device=0, shard_index=r, shard_count=2, shard_rows=8)
                s.execute(_scene("cornell"), n_samples=87)
                loc, rows = s.accum_local()
                assert s.stats()["k_split"] > 1
                s.close()
            assert np.array_equal(_bits(loc), whole[rows]), (env, r)
            seen[rows] += 1
        assert (seen == 1).all()


@pytest.mark.parametrize("name", ["boxes", "bvh"])
def test_band_kernels_of_the_family(name, monkeypatch):
    from micro_raytracer_amd._abi import F_BOX, F_BVH, F_LIGHTS
    ref, seg, st1 = _ref(monkeypatch, name, (87,))
    old, seg_old, _ = _ref(monkeypatch, name, (87,), OLD)
    assert np.array_equal(old, ref) and seg_old == seg
    want = F_BOX if name == "boxes" else F_BVH
    assert st1["kernel_features"] & want and not st1["kernel_features"] & F_LIGHTS and st1["block_threads"] == 256, st1
    for env in NEW:
        got, seg_new, st = _render(monkeypatch, name, (87,), env)
        assert st["k_split"] > 1 and st["kernel_features"] == st1["kernel_features"]
        assert np.array_equal(got, ref) and seg_new == seg, (name, env)


def test_adaptive_round_over_a_tile_list(monkeypatch):
    """Rounds of 32 samples, two chunks each: the first two cover every tile, the later ones the tiles of a list; even rounds feed
    the half buffer."""
    from micro_raytracer_amd import Sampler

    def run(env):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            s = Sampler(seed=SEED, device=0)
            info = s.execute_adaptive(_scene("cornell"), thr, min_samples=64, max_samples=128, step=32)
            out = (_bits(s.accum()[0]), s.sample_counts(), _bits(s.adapt_half()), info["launches"], s.stats()["k_split"])
            s.close()
        return out

    thr = float("inf")
    a0 = run(DIRECT)
    # a threshold between the tiles' errors, so that the second and third rounds run over a list: the median tile error
    from test_adaptive_host import np_tile_errors
    et, nan, _ = np_tile_errors(a0[0].view(np.float32), a0[2].view(np.float32), 64, 0.0)
    thr = float(np.median(et[~nan]))
    base = run(DIRECT)
    assert len(np.unique(base[1])) >= 2
    for env in [OLD] + NEW:
        got = run(env)
        assert got[4] > 1, env
        assert np.array_equal(got[1], base[1]) and np.array_equal(got[0], base[0]) and np.array_equal(got[2], base[2]), env
