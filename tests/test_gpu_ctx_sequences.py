"""Contexts held to the state model (tests/ctx_model.py) under seeded call sequences (tests/ctx_sequences.py).

After every call the status is the model's (after a refusal mrt_last_status too).  At every observation the count and the
per-pixel counts are the model's, and the accumulator, as uint32, is that of a PLAIN TWIN: a fresh MRT_FLAG_NO_LOOKAHEAD,
non-deferred context with a library-owned accumulator and the same seed, fed the model's restored contents and logical launch
log and nothing else; image bytes, the float image and denoise(passes = 0) are the twin's.  Every fifth observation and the
last one are held to the CPU oracle as well (Oracle.set_accum of the restored frame, then execute over the log's ranges) at the
parity bar 1e-4 * max(1, |ref|) on the mean with equal NaN patterns: that catches what subject and twin would share.
After an adaptive call the counts are those np_tile_errors gives on plain renders, every tile that stopped at n has the bits
of a plain execute(n), and the images are those of a fresh context that ran the same adaptive call and nothing else.
"""
import numpy as np
import pytest

import ctx_model as M
import ctx_sequences as Q
from conftest import make_holder
from test_adaptive_host import np_tile_errors
from test_image_path import DeviceBuffer

pytestmark = pytest.mark.gpu

f32 = np.float32
CTX_SEED = 5
TOL = 1e-4
ANCHOR_EVERY = 5
WORST = {"oracle": 0.0}

_FRAMES, _PLAIN, _ORACLE_AT, _ADAPTIVE, _PROBES = {}, {}, {}, {}, {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == f32 else np.ascontiguousarray(a)


def same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    ne = bits(got) != bits(want)
    if ne.any():
        at = tuple(int(i) for i in np.argwhere(ne)[0])
        flat = np.flatnonzero(ne)
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.size} elements differ, the first at {at}: got {got[at]!r}, want {want[at]!r} "
                             f"(flat indices {int(flat[0])} .. {int(flat[-1])}; {int((got[ne] == 0).sum())} of the differing are 0)")


def frame(name):
    if name not in _FRAMES:
        from micro_raytracer_amd import scenes
        f = Q.FRAMES[name]
        render, holder = make_holder(getattr(scenes, f["scene"])(res=f["res"], ssaa=f["ssaa"], sample=1, bounce=Q.BOUNCE))
        assert (render.frame.nw, render.frame.nh) == (f["nw"], f["nh"])
        _FRAMES[name] = (render, holder)
    return _FRAMES[name]


def sampler(name, flags=0, **kw):
    from micro_raytracer_amd import Sampler
    return Sampler(seed=CTX_SEED, device=0, flags=flags, **kw).create(frame(name)[0])


def plain(name, n):
    """What a fresh plain context holds after execute(n): computed once per frame and count."""
    if (name, n) not in _PLAIN:
        s = sampler(name, M.FLAG_NO_LOOKAHEAD)
        s.execute(frame(name)[0], n_samples=n)
        _PLAIN[name, n] = dict(accum=s.accum()[0], img_ss=s.img_ss(), dn0=s.denoise(passes=0))
        s.close()
    return _PLAIN[name, n]


def oracle_at(oracle_mod, name, n):
    if (name, n) not in _ORACLE_AT:
        o = oracle_mod.Oracle(frame(name)[1], seed=CTX_SEED)
        o.execute(n, threads=8)
        _ORACLE_AT[name, n] = o.accum()[0]
        o.close()
    return _ORACLE_AT[name, n]


def probes(name):
    """The 65 camera rays of mrt_radiance, their radiance and the AOVs, from a fresh context."""
    if name not in _PROBES:
        render = frame(name)[0]
        s = sampler(name, M.FLAG_NO_LOOKAHEAD)
        o, d = (a.reshape(-1, 3)[:65].copy() for a in s.camera_rays(render))
        _PROBES[name] = dict(o=o, d=d, rad=s.radiance(render, o, d, 4, sample_base=3), aov=s.aov())
        s.close()
    return _PROBES[name]


def held_to_oracle(what, got, ref, count):
    """The parity bar on the mean: 1e-4 * max(1, |ref|), equal NaN patterns.  Returns the worst error over the bar's scale."""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN patterns differ"
    g, r = got.astype(np.float64) / count, ref.astype(np.float64) / count
    fin = np.isfinite(r)
    if not fin.any():
        return 0.0
    rel = np.abs(g - r)[fin] / np.maximum(1.0, np.abs(r[fin]))
    worst = float(rel.max())
    WORST["oracle"] = max(WORST["oracle"], worst)
    assert worst <= TOL, f"{what}: mean off the oracle by {worst:.3e} x max(1, |ref|) at {tuple(int(i) for i in np.argwhere(fin)[int(rel.argmax())])}"
    return worst


# ---- adaptive calls ---------------------------------------------------------------------------------------------------------------
def resolve_adaptive(name, call):
    """(the call with a number for its threshold, the per-tile stop counts the header's rule gives): min = max or an infinite
    threshold stop every tile at min_samples; otherwise (32, 64, 16) the one evaluation is at n = 32, on the accumulator of a
    plain execute(32) and the half buffer of its even round, a plain execute(16) -- np_tile_errors says which tiles stop."""
    _, thr, mn, mx, step = call
    f = Q.FRAMES[name]
    n_tiles = -(-f["nw"] // 8) * -(-f["nh"] // 8)
    if mn == mx or thr == float("inf"):
        return call, [mn] * n_tiles
    assert (mn, mx, step) == (32, 64, 16)
    A, H = plain(name, 32)["accum"], plain(name, 16)["accum"]
    if thr == "median":
        et, nan, _ = np_tile_errors(A, H, 32, 0.0)
        thr = float(np.median(et[~nan]))
    _, _, conv = np_tile_errors(A, H, 32, thr)
    tiles = np.where(conv, 32, 64).reshape(-1)
    assert thr <= 0 or len(set(tiles.tolist())) == 2, "the median threshold splits the tiles"
    return ("adaptive", thr, mn, mx, step), [int(t) for t in tiles]


def adaptive_ref(oracle_mod, name, call, tiles):
    """What a context holds after this adaptive call, from plain renders tile by tile (the header's rule), and the images of a
    fresh context that ran the call and nothing else -- after its accumulator, counts, tone-mapped frame and means have been
    held to the plain renders."""
    key = (name,) + tuple(call[1:])
    if key in _ADAPTIVE:
        return _ADAPTIVE[key]
    render, _ = frame(name)
    f = Q.FRAMES[name]
    n_tx = -(-f["nw"] // 8)
    counts = np.array([[tiles[(y // 8) * n_tx + x // 8] for x in range(f["nw"])] for y in range(f["nh"])], np.uint32)
    ref = dict(counts=counts)
    for k in ("accum", "img_ss", "dn0"):
        ref[k] = np.zeros_like(plain(name, 32)[k])
        for n in sorted(set(tiles)):
            ref[k][counts == n] = plain(name, n)[k][counts == n]
    ref["img"] = ref["img_ss"] if tuple(f["res"]) == (f["nw"], f["nh"]) else oracle_mod.lanczos3_resize(ref["img_ss"], *f["res"])
    t = sampler(name, M.FLAG_NO_LOOKAHEAD)
    info = t.execute_adaptive(render, call[1], min_samples=call[2], max_samples=call[3], step=call[4])
    same("adaptive twin counts", t.sample_counts(), counts)
    same("adaptive twin accum", t.accum()[0], ref["accum"])
    same("adaptive twin img_ss", t.img_ss(), ref["img_ss"])
    same("adaptive twin img", t.img(), ref["img"])
    same("adaptive twin means", t.denoise(passes=0), ref["dn0"])
    ref["half"], ref["img_hdr"] = t.adapt_half(), t.img_hdr()
    m32 = counts == 32
    same("adaptive twin half buffer of the tiles that stopped at 32", ref["half"][m32], plain(name, 16)["accum"][m32])
    ref["samples"] = int(counts.astype(np.int64).sum())
    assert info["samples"] == ref["samples"] and info["min_count"] == counts.min() and info["max_count"] == counts.max()
    t.close()
    _ADAPTIVE[key] = ref
    return ref


# ---- subject, twin, oracle --------------------------------------------------------------------------------------------------------
class Subject:
    def __init__(self, name, variant, monkeypatch):
        v = Q.VARIANTS[variant]
        sh = v.get("shard", (0, 1, 8))
        with monkeypatch.context() as mp:
            for k, val in v.get("env", {}).items():
                mp.setenv(k, val)
            self.s = sampler(name, v["flags"], shard_index=sh[0], shard_count=sh[1], shard_rows=sh[2])
        self.render = frame(name)[0]
        self.name = name
        self.buffers = []                                   # everything bound or copied from stays allocated until close()
        self.bound_buf = None
        self.need = self.s.padded_rows() * self.s.nw * 3 * 4

    def close(self):
        self.s.close()
        for b in self.buffers:
            b.free()

    def call(self, call, frames):
        """(status, value) of one call; the value of an observation is what it returned."""
        from micro_raytracer_amd import _lib
        from micro_raytracer_amd._lib import MrtError
        s, kind = self.s, call[0]
        try:
            if kind == "execute":
                return _lib.lib().mrt_execute(s._ctx, call[1], None), None
            if kind == "burst":
                for _ in range(call[1]):
                    rc = _lib.lib().mrt_execute(s._ctx, 1, None)
                    if rc:
                        return rc, None
                return M.OK, None
            if kind in ("accum", "save"): return M.OK, s.accum()
            if kind == "accum_local": return M.OK, s.accum_local()
            if kind == "img": return M.OK, s.img()
            if kind == "img_ss": return M.OK, s.img_ss()
            if kind == "img_hdr": return M.OK, s.img_hdr()
            if kind == "denoise": return M.OK, s.denoise(passes=0)
            if kind == "sample_counts": return M.OK, s.sample_counts()
            if kind == "stats": return M.OK, s.stats()
            if kind == "reset": return M.OK, s.reset()
            if kind == "set_accum":
                return M.OK, s.set_accum(*frames[call[1]])
            if kind == "set_accum_device":
                rgb, cnt = frames[call[1]]
                b = DeviceBuffer(rgb.nbytes)
                self.buffers.append(b)
                b.write(rgb)
                return M.OK, s.set_accum_device(b.ptr.value, cnt)
            if kind == "bind":
                b = DeviceBuffer(self.need if call[1] == "fit" else self.need - 4)      # the only undersized buffer: the refused one
                self.buffers.append(b)
                s.bind_accum(b.ptr.value, b.nbytes)
                self.bound_buf = b
                return M.OK, None
            if kind == "unbind":
                s.bind_accum(0, 0)
                self.bound_buf = None
                return M.OK, None
            if kind == "device_ptr": return M.OK, s.accum_device_ptr()
            if kind == "adaptive":
                return M.OK, s.execute_adaptive(self.render, call[1], min_samples=call[2], max_samples=call[3], step=call[4])
            if kind == "adapt_half": return M.OK, s.adapt_half()
            if kind == "radiance":
                p = probes(self.name)
                return M.OK, s.radiance(self.render, p["o"], p["d"], 4, sample_base=3)
            if kind == "aov": return M.OK, s.aov()
        except MrtError as e:
            return e.code, None
        raise ValueError(call)


class Follower:
    """The model's restored contents and logical launch log, replayed and nothing else: on a plain twin context, or on the oracle."""

    def __init__(self, reset, set_accum, execute, count):
        self.reset, self.set_accum, self.execute, self.count = reset, set_accum, execute, count
        self.epoch, self.applied = 0, 0

    def follow(self, m, frames):
        if self.epoch != m.epoch:
            self.reset() if m.restored is None else self.set_accum(*frames[m.restored[0]])
            self.epoch, self.applied = m.epoch, 0
        for base, n in m.log[self.applied:]:
            assert self.count() == base, f"the launch log continues at sample {base}, its follower is at {self.count()}"
            self.execute(n)
        self.applied = len(m.log)


def synth_frame(src, nw, nh):
    _, seed, count = src
    rng = np.random.default_rng(seed)
    rgb = (rng.gamma(0.6, 0.4, size=(nh, nw, 3)) * count).astype(f32)
    rgb[rng.integers(nh), rng.integers(nw)] = 0.0
    return rgb, count


def run_sequence(name, variant, calls, label, oracle_mod, monkeypatch):
    from micro_raytracer_amd import _lib
    render, holder = frame(name)
    f = Q.FRAMES[name]
    nw, nh = f["nw"], f["nh"]
    m = Q.model_of(name, variant)
    subj = Subject(name, variant, monkeypatch)
    tw = sampler(name, M.FLAG_NO_LOOKAHEAD)
    twin = Follower(tw.reset, tw.set_accum, lambda n: tw.execute(render, n_samples=n), lambda: tw.accum()[1])
    orc = oracle_mod.Oracle(holder, seed=CTX_SEED)
    oracle = Follower(orc.reset, orc.set_accum, lambda n: orc.execute(n, threads=8), lambda: orc.accum()[1])
    imgtwin = None                                          # a sharded subject that received a whole frame: its images
    frames = {}
    rows = np.array(m.rows, np.int64)
    others = np.setdiff1d(np.arange(nh), rows)
    aref = None
    n_obs, prev_accum, worst = 0, None, 0.0
    i = -1
    try:
        assert (subj.s.nw, subj.s.nh, subj.s.local_rows, subj.s.padded_rows()) == (nw, nh, len(m.rows), m.padded_rows)
        for i, call in enumerate(calls):
            kind = call[0]
            tiles = None
            if kind in ("set_accum", "set_accum_device") and call[1][0] == "synth":
                frames.setdefault(call[1], synth_frame(call[1], nw, nh))
            if kind == "adaptive":
                call, tiles = resolve_adaptive(name, call)
            want = m.apply(call, tile_counts=tiles)
            rc, val = subj.call(call, frames)
            assert rc == want, f"status {rc}, the model says {want}"
            if rc != M.OK:
                assert _lib.lib().mrt_last_status() == want, f"mrt_last_status {_lib.lib().mrt_last_status()} after a refusal with {want}"
                continue
            if kind == "adaptive":
                aref = adaptive_ref(oracle_mod, name, call, tiles)
                assert val["samples"] == aref["samples"] and val["min_count"] == m.frame_count
            elif kind == "adapt_half":
                same("adapt_half", val, aref["half"])
            elif kind == "radiance":
                same("radiance", val, probes(name)["rad"])
            elif kind == "aov":
                for k, a in probes(name)["aov"].items():
                    same(f"aov {k}", val[k], a)
            if kind not in M.OBSERVATIONS:
                continue

            # ---- an observation: what the subject must hold now ----
            n_obs += 1
            anchor = n_obs % ANCHOR_EVERY == 0 or i == len(calls) - 1
            adaptive = m.adaptive is not None
            if adaptive:
                own = aref["accum"]
                counts = aref["counts"]
                same("the model's per-pixel counts", np.array(m.pixel_counts(), np.uint32), counts)
            else:
                twin.follow(m, frames)
                own = tw.accum()[0]
                counts = np.full((nh, nw), m.frame_count, np.uint32)
            if m.full:                                      # a shard shows the frame it received; its own rows go on underneath
                whole = frames[m.full[0]][0]
                if imgtwin is None:
                    imgtwin = sampler(name, M.FLAG_NO_LOOKAHEAD)
                imgtwin.set_accum(whole, m.full[1])
                images = imgtwin
            else:
                whole = own.copy()
                whole[others] = 0.0
                images = tw
            if kind in ("accum", "save"):
                assert val[1] == m.frame_count, f"count {val[1]}, the model says {m.frame_count}"
                same("accumulator", val[0], whole)
                state = (m.epoch, len(m.log), m.full)
                if prev_accum is not None and prev_accum[0] == state:
                    same("accumulator against the previous observation (nothing in between changed it)", val[0], prev_accum[1])
                prev_accum = (state, val[0])
                if kind == "save":
                    frames["slot", call[1]] = (val[0].copy(), val[1])
            elif kind == "accum_local":
                assert np.array_equal(val[1], rows), f"rows {val[1]}"
                same("the shard's own rows", val[0], own[rows])
            elif kind == "sample_counts":
                same("sample_counts", val, counts)
            elif kind == "stats":
                assert (val["samples"], val["deferred"]) == (m.stats_samples, m.stats_deferred), \
                    f"stats samples {val['samples']} deferred {val['deferred']}, the model says {m.stats_samples} and {m.stats_deferred}"
            elif adaptive:
                same(kind, val, aref[{"denoise": "dn0"}.get(kind, kind)])
            else:
                same(kind, val, {"img": images.img, "img_ss": images.img_ss, "img_hdr": images.img_hdr, "denoise": lambda: images.denoise(passes=0)}[kind]())
            got_count = subj.s.accum()[1]
            assert got_count == m.frame_count, f"count {got_count}, the model says {m.frame_count}"
            same("sample_counts", subj.s.sample_counts(), counts)
            loc = subj.s.accum_local()[0]
            same("the accumulator's own rows", loc, own[rows])
            if subj.bound_buf is not None:                  # the caller's memory holds the rows at every return
                same("the bound buffer", subj.bound_buf.read()[:loc.size].reshape(loc.shape), loc)
            if anchor and m.count:
                if adaptive:
                    for n in sorted(set(m.adaptive)):
                        mask = counts == n
                        worst = max(worst, held_to_oracle(f"tiles that stopped at {n}", loc[mask], oracle_at(oracle_mod, name, n)[mask], n))
                else:
                    oracle.follow(m, frames)
                    ref, cnt = orc.accum()
                    assert cnt == m.count
                    worst = max(worst, held_to_oracle("accumulator", loc, ref[rows], m.count))
    except AssertionError as e:
        diff = str(e).splitlines()[0] if str(e) else "assertion"
        raise AssertionError(f"{label}, variant {variant}, frame {name}: call {i} {calls[i] if 0 <= i < len(calls) else ''}: {diff}\n"
                             f"replay: calls = {list(calls[:i + 1])!r}") from e
    finally:
        subj.close()
        tw.close()
        orc.close()
        if imgtwin is not None:
            imgtwin.close()
    print(f"{label} {variant} {name}: {len(calls)} calls, {n_obs} observations, {m.count} samples at the end, oracle worst {worst:.3e}")


@pytest.mark.parametrize("variant", list(Q.VARIANTS))
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_generated_sequence(seed, variant, oracle_mod, monkeypatch):
    run_sequence(Q.frame_of(seed), variant, Q.generate(seed, variant), f"seed {seed}", oracle_mod, monkeypatch)


@pytest.mark.parametrize("name,variant", Q.named_cases())
def test_named_sequence(name, variant, oracle_mod, monkeypatch):
    frame_name, calls = Q.named(name)
    run_sequence(frame_name, variant, Q.prefix_of(variant) + calls, name, oracle_mod, monkeypatch)


def test_worst_oracle_error_of_the_file():
    """Not a check of its own: the largest error against the oracle that the tests above met, next to the bar they hold."""
    print(f"call sequences: worst error against the oracle {WORST['oracle']:.3e} x max(1, |ref|), bar {TOL:.0e}")
    assert WORST["oracle"] <= TOL
