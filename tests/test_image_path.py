"""Sampler::img at its input edges: the tone map (tonemap_u8, and tonemap_tiles_u8 of adaptive renders) and the Lanczos3
resize (lanczos3_v / lanczos3_h) on crafted accumulators, bit for bit against the CPU oracle.

Natural renders give the tone map modest non-negative sums and the resize smooth images.  Here the sums sit on the u8
level boundaries of the tone map (found by bisection over f32 bit patterns against the oracle) and their f32 neighbours,
mixed with NaN, infinities, signed zeros, negatives, denormals and FLT_MAX, at counts up to 2^32-1 and camera values the
loader accepts but natural scenes never use.  The resize sees 0/255 checkerboards, single pixels, hard border edges and
random bytes at every ssaa from 0.5 to 4, on frames down to 1x1; the set of cases is checked to drive both clamps of the
output conversion and a value that is exactly .5 before rounding.

CPU part: the x86 build of the kernels' per-element bodies (tests/emu, mrt_post.h + lanczos3_taps) against the oracle.
GPU part: the same cases through Sampler.set_accum / img_ss / img, and the per-tile tone map of an adaptive render into a
caller-bound accumulator.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import make_holder

f32 = np.float32

GAMMAS = (0.8, 0.4, 1.0, 2.2, 0.0, -0.5)
EXPS = (0.2, 0.0, 0.85, 1.0, 1.5)                  # exp = 1.0: wexp = (1 - exp)^2 = 0.  The loader refuses none of these.
COUNTS = (1, 3, 1024, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 31) - 1, (1 << 32) - 1)
SSAAS = (0.5, 0.75, 1.3, 1.5, 2.0, 2.5, 3.0, 4.0)
RESOLUTIONS = ((1, 1), (1, 9), (9, 1), (3, 2), (2, 3), (7, 5), (13, 11), (23, 4), (37, 31))
PATTERNS = ("checker1", "checker2", "bright", "dark", "border", "zero", "full", "random")
TONEMAP_RES = (23, 17)                             # 391 pixels: not a multiple of the 256-thread workgroup

_FLT_MAX = np.finfo(f32).max
SPECIALS = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, -1e-3, -_FLT_MAX, -1e-45, 1e-45, 1e-40, 1.1754942e-38,
                     np.finfo(f32).tiny, 1.0, 255.0, _FLT_MAX, np.nextafter(_FLT_MAX, f32(0)), 3e38, 1e30], f32)


def desc(res, ssaa=1.0, gamma=0.8, exp=0.2, sample=1):
    """A one-sphere render whose camera carries (gamma, exp); the image path never looks at the scene."""
    return {"rt": {"sample": sample, "bounce": 1},
            "frame": {"res": [int(res[0]), int(res[1])], "ssaa": ssaa, "cam": {"pos": [0, -1, 0], "gamma": gamma, "exp": exp}},
            "scene": {"renderer": [{"type": "sphere", "r": 0.3, "pos": [0, 0.5, 0]}]}}


def ss_dims(res, ssaa):
    """(nw, nh) of the supersampled frame: (res as f32 * ssaa) as usize."""
    return int(f32(res[0]) * f32(ssaa)), int(f32(res[1]) * f32(ssaa))


_HOLDERS = {}


def holder_of(res, ssaa=1.0, gamma=0.8, exp=0.2):
    k = (tuple(res), float(ssaa), float(gamma), float(exp))
    if k not in _HOLDERS:
        _HOLDERS[k] = make_holder(desc(res, ssaa, gamma, exp))
    return _HOLDERS[k]


class DeviceBuffer:
    """Caller-owned device memory for mrt_bind_accum, from the HIP runtime libmrt_hip.so itself is bound to.  (A torch
    tensor would do in a process of its own, but torch carries a second copy of the HIP runtime, and it finds no GPU in a
    process where the library's runtime is already up -- as in a pytest session.)  The hip* symbols are looked up through
    the library's own handle, which searches the library and then its dependencies, so they come from the runtime the
    library uses even when another test has loaded torch's copy into the process as well."""

    def __init__(self, nbytes, fill=None):
        from micro_raytracer_amd import _lib
        _lib.lib()
        self.hip = C.CDLL(_lib.LIB_PATH)                     # a second handle of the loaded library: its own argtypes
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.nbytes = nbytes
        self.ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), nbytes) == 0
        if fill is not None:
            self.write(np.full(nbytes // 4, fill, f32))

    def write(self, host):
        host = np.ascontiguousarray(host)
        assert host.nbytes <= self.nbytes
        assert self.hip.hipMemcpy(self.ptr, host.ctypes.data, host.nbytes, 1) == 0        # hipMemcpyHostToDevice
        self.synchronize()

    def read(self, dtype=f32):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype)
        assert self.hip.hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0         # hipMemcpyDeviceToHost
        return out

    def synchronize(self):
        assert self.hip.hipDeviceSynchronize() == 0

    def free(self):
        if self.ptr:
            self.hip.hipFree(self.ptr)
            self.ptr = C.c_void_p()


# ---------------------------------------------------------------- the inverse tone map
_TABLES = {}


def level_table(oracle_mod, gamma, exp, count):
    """(sums, reached): sums[L] = the f32 sum at which the oracle's tone map at (gamma, exp, count) steps from below L to L
    or more, found by bisection over non-negative f32 bit patterns (the map is monotone for gamma > 0);
    reached[L] = whether the tone map of sums[L] is exactly L (False: no f32 sum gives L).  All 256 levels bisect at once,
    one oracle img_ss per step."""
    key = (float(gamma), float(exp), int(count))
    if key in _TABLES:
        return _TABLES[key]
    assert gamma > 0
    _, h = holder_of((16, 16), 1.0, gamma, exp)
    o = oracle_mod.Oracle(h)

    def levels(pat):
        s = np.asarray(pat, np.uint32).view(f32)
        o.set_accum(np.repeat(s, 3).reshape(16, 16, 3), count)
        return o.img_ss()[..., 0].reshape(-1).astype(np.int64)

    # upper end: a mean of 2^40 maps to 255 for every camera here, and below it pow_ and the Reinhard curve stay finite
    hi_sum = f32(float(count) * 2.0 ** 40)
    lo = np.zeros(256, np.int64)
    hi = np.full(256, int(np.array(hi_sum, f32).view(np.uint32)), np.int64)
    assert levels(lo)[0] == 0 and levels(hi)[0] == 255
    target = np.arange(256)
    for _ in range(34):
        mid = (lo + hi) // 2
        up = levels(mid) >= target
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid)
    hi[0] = 0
    assert (hi - lo <= 1)[1:].all()
    got = levels(hi)
    below = levels(np.maximum(hi - 1, 0))
    assert (got >= target).all() and (below[1:] < target[1:]).all()
    o.close()
    _TABLES[key] = (hi.astype(np.uint32).view(f32), got == target)
    return _TABLES[key]


def boundary_values(oracle_mod, gamma, exp, count):
    """Every reached level's boundary sum, its f32 neighbours, and the specials."""
    g = gamma if gamma > 0 else 0.8                   # gamma <= 0 is not monotone: use gamma 0.8's boundaries as inputs
    sums, reached = level_table(oracle_mod, g, exp, count)
    b = sums[reached]
    return np.concatenate([b, np.nextafter(b, f32(np.inf)), np.nextafter(b, f32(-np.inf)), SPECIALS]).astype(f32)


def crafted_frame(values, nh, nw, seed):
    """An (nh, nw, 3) accumulator holding every value at least once (if it fits), in a shuffled order."""
    rng = np.random.default_rng(seed)
    n = nh * nw * 3
    reps = -(-n // values.size)
    flat = np.tile(values, reps)[:n] if values.size <= n else values[:n]
    if values.size <= n:
        flat = flat.copy()
        flat[:values.size] = values
    return rng.permutation(flat).reshape(nh, nw, 3)


def tonemap_cases(oracle_mod):
    """(gamma, exp, count, accum) over every camera and count: the crafted frames of TONEMAP_RES."""
    nw, nh = TONEMAP_RES
    for gi, gamma in enumerate(GAMMAS):
        for ei, exp in enumerate(EXPS):
            for ci, count in enumerate(COUNTS):
                v = boundary_values(oracle_mod, gamma, exp, count)
                yield gamma, exp, count, crafted_frame(v, nh, nw, seed=gi * 100 + ei * 10 + ci)


# ---------------------------------------------------------------- resize patterns
def u8_pattern(name, nh, nw, seed=0):
    y, x = np.mgrid[0:nh, 0:nw]
    img = np.zeros((nh, nw, 3), np.uint8)
    if name == "checker1":
        img[...] = (((x + y) % 2) * 255)[..., None]
        img[..., 1] = 255 - img[..., 1]
    elif name == "checker2":
        img[...] = ((((x // 2) + (y // 2)) % 2) * 255)[..., None]
    elif name == "bright":
        img[nh // 2, nw // 2] = 255
        img[0, nw - 1, 1] = 255
    elif name == "dark":
        img[...] = 255
        img[nh // 2, nw // 2] = 0
        img[nh - 1, 0, 2] = 0
    elif name == "border":                           # a hard edge on each side, one per channel
        img[:, 0, 0] = 255
        img[0, :, 1] = 255
        img[nh - 1, :, 2] = 255
        img[:, nw - 1, 2] = 255
    elif name == "full":
        img[...] = 255
    elif name == "random":
        img[...] = np.random.default_rng(seed).integers(0, 256, (nh, nw, 3), dtype=np.uint8)
    else:
        assert name == "zero"
    return img


def resize_cases():
    """(res, ssaa, pattern); frames whose res * ssaa truncates to 0 are refused by the loader and left out."""
    for res in RESOLUTIONS:
        for ssaa in SSAAS:
            nw, nh = ss_dims(res, ssaa)
            if nw == 0 or nh == 0:
                continue
            for p in PATTERNS:
                yield res, ssaa, p


def accum_for(oracle_mod, img):
    """A count-1 accumulator whose tone map (camera gamma 0.8, exp 0.2) is img; unreachable levels move to the next
    reachable one."""
    sums, reached = level_table(oracle_mod, 0.8, 0.2, 1)
    lv = np.arange(256)
    ok = lv[reached]
    nearest = ok[np.minimum(np.searchsorted(ok, lv), ok.size - 1)]
    want = nearest[img]
    return sums[want].astype(f32), want.astype(np.uint8)


def lanczos_weights(oracle_mod, src, dst):
    """[(left, weights f32[n])] per output index, from the oracle's orc_lanczos3_weights."""
    L = oracle_mod.lib()
    cap = int(2.0 * 3.0 * max(1.0, src / dst)) + 8
    out = []
    for o in range(dst):
        w = np.zeros(cap, f32)
        left = C.c_uint32()
        n = L.orc_lanczos3_weights(src, dst, o, C.byref(left), w.ctypes.data_as(C.POINTER(C.c_float)), cap)
        assert n > 0
        out.append((left.value, w[:n].copy()))
    return out


def resize_pre_round(oracle_mod, ss, rw, rh):
    """The oracle's horizontal_sample results before clamping and rounding, restated in numpy (f32, same order)."""
    nh, nw = ss.shape[:2]
    src = ss.astype(f32)
    tmp = np.zeros((rh, nw, 3), f32)
    for oy, (left, w) in enumerate(lanczos_weights(oracle_mod, nh, rh)):
        t = np.zeros((nw, 3), f32)
        for i, wi in enumerate(w):
            t = (t + src[left + i] * wi).astype(f32)
        tmp[oy] = t
    out = np.zeros((rh, rw, 3), f32)
    for ox, (left, w) in enumerate(lanczos_weights(oracle_mod, nw, rw)):
        t = np.zeros((rh, 3), f32)
        for i, wi in enumerate(w):
            t = (t + tmp[:, left + i] * wi).astype(f32)
        out[:, ox] = t
    return out


def round_u8(t):
    """clamp to [0, 255], round half away from zero"""
    c = np.clip(t, f32(0), f32(255))
    fl = np.floor(c)
    return np.where(c - fl >= f32(0.5), fl + 1, fl).astype(np.uint8)


# ---------------------------------------------------------------- CPU: x86 build of the kernel bodies against the oracle
def test_level_table_is_a_set_of_boundaries(oracle_mod):
    for gamma in (0.8, 2.2):
        for exp in (0.2, 1.0):
            for count in (1, (1 << 32) - 1):
                sums, reached = level_table(oracle_mod, gamma, exp, count)
                assert reached[0] and reached[255] and sums[0] == 0
                assert (np.diff(sums.view(np.uint32)[reached].astype(np.int64)) > 0).all()
                for L in np.flatnonzero(reached)[1:]:
                    assert oracle_mod.tonemap_px(np.full(3, sums[L]), count, gamma, exp)[0] == L
                    assert oracle_mod.tonemap_px(np.full(3, np.nextafter(sums[L], f32(0))), count, gamma, exp)[0] < L
    sums, reached = level_table(oracle_mod, 0.8, 0.2, 1)
    assert reached.all()                              # the resize patterns need every level at count 1
    _, r1 = level_table(oracle_mod, 0.8, 1.0, 1)
    assert r1.sum() == 2                              # wexp = 0: 0 or 255 only


def test_tonemap_edges_x86_equal_oracle(oracle_mod, emu_mod):
    mism = 0
    for gamma, exp, count, acc in tonemap_cases(oracle_mod):
        _, h = holder_of(TONEMAP_RES, 1.0, gamma, exp)
        o = oracle_mod.Oracle(h)
        o.set_accum(acc, count)
        ref = o.img_ss()
        ss, img = emu_mod.img(h, acc, count)
        bad = ss != ref
        mism += int(np.count_nonzero(bad))
        assert not bad.any(), (gamma, exp, count, acc[bad][:4], ss[bad][:4], ref[bad][:4])
        assert np.array_equal(img, o.img())
        o.close()
    assert mism == 0


def test_tonemap_edges_reach_every_kind_of_output(oracle_mod):
    """The crafted frames hit 0, 255 and a middle level under each camera with gamma > 0 and wexp > 0."""
    nw, nh = TONEMAP_RES
    for gamma in (0.8, 0.4, 1.0, 2.2):
        for exp in (0.2, 0.0, 0.85, 1.5):
            _, h = holder_of(TONEMAP_RES, 1.0, gamma, exp)
            o = oracle_mod.Oracle(h)
            seen = set()
            for count in COUNTS:
                o.set_accum(crafted_frame(boundary_values(oracle_mod, gamma, exp, count), nh, nw, 0), count)
                seen |= set(np.unique(o.img_ss()).tolist())
            o.close()
            assert {0, 255} <= seen and len(seen) > 200, (gamma, exp, len(seen))


def test_lanczos_patterns_x86_equal_oracle(oracle_mod, emu_mod):
    low = high = half = 0
    mism = 0
    for res, ssaa, pat in resize_cases():
        nw, nh = ss_dims(res, ssaa)
        _, h = holder_of(res, ssaa)
        acc, want = accum_for(oracle_mod, u8_pattern(pat, nh, nw, seed=nw * 131 + nh))
        o = oracle_mod.Oracle(h)
        o.set_accum(acc, 1)
        ref_ss = o.img_ss()
        assert np.array_equal(ref_ss, want), (res, ssaa, pat)
        ref = o.img()
        o.close()
        ss, img = emu_mod.img(h, acc, 1)
        assert np.array_equal(ss, ref_ss)
        mism += int(np.count_nonzero(img != ref))
        assert np.array_equal(img, ref), (res, ssaa, pat, np.argwhere(img != ref)[:4])
        if (nw, nh) != tuple(res):
            t = resize_pre_round(oracle_mod, ref_ss, res[0], res[1])
            assert np.array_equal(round_u8(t), ref), (res, ssaa, pat)
            low += int(np.count_nonzero(t < 0))
            high += int(np.count_nonzero(t > 255))
            half += int(np.count_nonzero((t >= 0) & (t <= 255) & (t - np.floor(t) == f32(0.5))))
    print(f"lanczos: {mism} mismatches; pre-round values below 0: {low}, above 255: {high}, exactly .5: {half}")
    assert mism == 0
    assert low > 0 and high > 0 and half > 0, (low, high, half)


# ---------------------------------------------------------------- GPU: the same cases through the device image path
@pytest.mark.gpu
def test_tonemap_edges_gpu_equal_oracle(oracle_mod):
    from micro_raytracer_amd import Sampler
    mism = 0
    ctx = {}
    for gamma, exp, count, acc in tonemap_cases(oracle_mod):
        render, h = holder_of(TONEMAP_RES, 1.0, gamma, exp)
        if (gamma, exp) not in ctx:
            for s, o in ctx.values():
                s.close()
                o.close()
            ctx = {(gamma, exp): (Sampler(seed=1, device=0).create(render), oracle_mod.Oracle(h))}
        s, o = ctx[(gamma, exp)]
        s.set_accum(acc, count)
        o.set_accum(acc, count)
        ss, ref = s.img_ss(), o.img_ss()
        bad = ss != ref
        mism += int(np.count_nonzero(bad))
        assert not bad.any(), (gamma, exp, count, acc[bad][:4], ss[bad][:4], ref[bad][:4])
        assert np.array_equal(s.img(), o.img())
    for s, o in ctx.values():
        s.close()
        o.close()
    print(f"tone map edges on the device: {mism} mismatches")


@pytest.mark.gpu
def test_lanczos_patterns_gpu_equal_oracle(oracle_mod):
    """Every pattern on one context per frame: the taps and buffers of img_prepare are built by the first img() and reused by
    every later one, after set_accum changes the accumulator.  The first pattern's img() is also taken twice."""
    from micro_raytracer_amd import Sampler
    mism = 0
    by_frame = {}
    for res, ssaa, pat in resize_cases():
        by_frame.setdefault((res, ssaa), []).append(pat)
    for (res, ssaa), pats in by_frame.items():
        nw, nh = ss_dims(res, ssaa)
        render, h = holder_of(res, ssaa)
        s = Sampler(seed=1, device=0).create(render)
        o = oracle_mod.Oracle(h)
        for i, pat in enumerate(pats):
            acc, want = accum_for(oracle_mod, u8_pattern(pat, nh, nw, seed=nw * 131 + nh))
            s.set_accum(acc, 1)
            o.set_accum(acc, 1)
            ss = s.img_ss()
            assert np.array_equal(ss, want), (res, ssaa, pat)
            ref = o.img()
            img = s.img()
            mism += int(np.count_nonzero(img != ref))
            assert np.array_equal(img, ref), (res, ssaa, pat, np.argwhere(img != ref)[:4])
            if i == 0:
                assert np.array_equal(s.img(), ref), (res, ssaa, pat, "second img()")
        s.close()
        o.close()
    print(f"lanczos patterns on the device: {mism} mismatches")


# ---------------------------------------------------------------- GPU: the per-tile tone map of an adaptive render
AD_MIN, AD_MAX, AD_STEP, AD_SEED = 32, 128, 16, 5


def _adaptive_threshold(render):
    """A threshold that leaves at least three distinct tile counts: a quantile of the tile errors at AD_MIN."""
    from micro_raytracer_amd import Sampler
    from test_adaptive_host import np_tile_errors
    s = Sampler(seed=AD_SEED, device=0)
    s.execute_adaptive(render, float("inf"), min_samples=AD_MIN, max_samples=AD_MAX, step=AD_STEP)
    et, nan, _ = np_tile_errors(s.accum()[0], s.adapt_half(), AD_MIN, 0.0)
    s.close()
    for q in (0.3, 0.5, 0.15, 0.7):
        thr = float(np.quantile(et[~nan], q))
        t = Sampler(seed=AD_SEED, device=0)
        t.execute_adaptive(render, thr, min_samples=AD_MIN, max_samples=AD_MAX, step=AD_STEP)
        n = len(np.unique(t.sample_counts()))
        t.close()
        if n >= 3:
            return thr
    raise AssertionError("no threshold leaves three tile counts")


@pytest.mark.gpu
@pytest.mark.parametrize("res,ssaa", [((100, 60), 1.0), ((64, 48), 1.5)])
def test_adaptive_into_bound_accumulator_and_tile_tonemap(res, ssaa, oracle_mod):
    from micro_raytracer_amd import Sampler, scenes
    render, holder = make_holder(scenes.cornell_box(res=res, ssaa=ssaa, sample=AD_MAX, bounce=8))
    thr = _adaptive_threshold(render)

    # 1-2. an adaptive render into caller memory equals the same render into the library's own accumulator
    s = Sampler(seed=AD_SEED, device=0).create(render)
    rows, nw, nh = s.padded_rows(), s.nw, s.nh
    t = DeviceBuffer(rows * nw * 3 * 4, fill=7.0)
    s.bind_accum(t.ptr.value, t.nbytes)
    info = s.execute_adaptive(render, thr, min_samples=AD_MIN, max_samples=AD_MAX, step=AD_STEP)
    counts = s.sample_counts()
    stops = np.unique(counts)
    assert len(stops) >= 3, stops
    A, cnt = s.accum()
    t.synchronize()
    bound = t.read().reshape(rows, nw, 3)
    assert np.array_equal(bound[:nh].view(np.uint32), A.view(np.uint32))
    assert (bound[nh:] == 0).all()                           # padding rows: cleared with the rest, never written
    u = Sampler(seed=AD_SEED, device=0)
    uinfo = u.execute_adaptive(render, thr, min_samples=AD_MIN, max_samples=AD_MAX, step=AD_STEP)
    assert np.array_equal(u.accum()[0].view(np.uint32), A.view(np.uint32))
    assert np.array_equal(u.sample_counts(), counts) and np.array_equal(u.adapt_half(), s.adapt_half())
    assert np.array_equal(u.img_ss(), s.img_ss())
    assert {k: v for k, v in uinfo.items() if k not in ("kernel_ms", "seconds")} == \
        {k: v for k, v in info.items() if k not in ("kernel_ms", "seconds")}
    u.close()

    # 3. crafted sums written straight into the bound tensor: each pixel tone-mapped at its own tile's count
    cam = render.frame.cam
    acc = np.zeros((nh, nw, 3), f32)
    for i, n in enumerate(stops):
        v = boundary_values(oracle_mod, cam.gamma, cam.exp, int(n))
        m = counts == n
        acc[m] = crafted_frame(v, nh, nw, seed=i)[m]
    t.write(acc)                                             # the first nh rows; hipMemcpy, then the device synchronised
    ss = s.img_ss()
    want = np.zeros_like(ss)
    o = oracle_mod.Oracle(holder)
    for n in stops:
        o.set_accum(acc, int(n))
        m = counts == n
        want[m] = o.img_ss()[m]
    o.close()
    bad = ss != want
    print(f"per-tile tone map {res} ssaa {ssaa}: counts {stops.tolist()}, {int(np.count_nonzero(bad))} mismatches")
    assert not bad.any(), (np.argwhere(bad)[:4], acc[bad][:4], ss[bad][:4], want[bad][:4])
    fw, fh = render.frame.res
    assert np.array_equal(s.img(), oracle_mod.lanczos3_resize(ss, fw, fh))
    assert s.accum()[1] == cnt == counts.min()
    s.close()
    t.free()
