"""TEST INFRASTRUCTURE: a numpy restatement of the linear float image (mrt_img_hdr) and of its writers -- the f32
mean, the two resize passes as per-tap loops over float32 arrays (unfused, taps in index order, sums from +0), the clamp, the
box taps in Python integers, the RGBE encode / decode and a PFM parser -- with the frames and contents the CPU and the GPU tests
share.  Lanczos3 weights come from the oracle's orc_lanczos3_weights, as tests/test_image_path.py takes them."""
import ctypes as C
import math

import numpy as np

f32 = np.float32
FLT_MAX = float(np.finfo(f32).max)

# (res, ssaa): a downsample by 2, a ratio of 1.5, an upsample, 520 supersampled columns (1560 row elements: both kernels run a
# second, partial workgroup of 256 threads), and no resize
SHAPES = (((12, 8), 2.0), ((10, 6), 1.5), ((8, 8), 0.5), ((260, 3), 2.0), ((16, 16), 1.0))
FILTERS = ("lanczos3", "box")


def ss_dims(res, ssaa):
    """(nw, nh) of the supersampled frame: (res as f32 * ssaa) as usize."""
    return int(f32(res[0]) * f32(ssaa)), int(f32(res[1]) * f32(ssaa))


def desc(res, ssaa=1.0, sample=1):
    """A one-sphere render; the image path never looks at the scene."""
    return {"rt": {"sample": sample, "bounce": 1},
            "frame": {"res": [int(res[0]), int(res[1])], "ssaa": ssaa, "cam": {"pos": [0, -1, 0]}},
            "scene": {"renderer": [{"type": "sphere", "r": 0.3, "pos": [0, 0.5, 0]}]}}


def same(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- contents ----------------------------------------------------------------------------------------------------------------------
def contents(nh, nw, seed):
    """[(name, sums f32 [nh][nw][3], count)]: random values in [0, 4) at both counts, a 1e4 spike on a zero field, one NaN pixel,
    one +inf pixel, denormals."""
    rng = np.random.default_rng(seed)
    rand = lambda: (rng.random((nh, nw, 3), dtype=f32) * f32(4.0)).astype(f32)
    spike = np.zeros((nh, nw, 3), f32)
    spike[nh // 2, nw // 2] = 1e4
    nan = rand()
    nan[nh // 3, nw // 3, 1] = np.nan
    inf = rand()
    inf[(2 * nh) // 3, (2 * nw) // 3] = np.inf
    den = rng.integers(1, 1 << 22, (nh, nw, 3)).astype(np.uint32).view(f32)       # every value below FLT_MIN
    return [("random1", rand(), 1), ("random37", rand(), 37), ("spike", spike, 1), ("nan", nan, 1), ("inf", inf, 37),
            ("denormal1", den, 1), ("denormal37", den.copy(), 37)]


# ---- the mean ------------------------------------------------------------------------------------------------------------------------
def mean(sums, count):
    """m = A * rc, rc = 1.0f / (float)count; count: an int, or uint32 [nh][nw] per-pixel counts (each pixel its tile's)"""
    rc = f32(1.0) / (np.asarray(count, np.uint32).astype(f32)[..., None] if np.ndim(count) else f32(count))
    with np.errstate(all="ignore"):
        return (np.asarray(sums, f32) * rc).astype(f32)


def tile_counts(pixel_counts):
    """uint32 [ceil(nh/8)][ceil(nw/8)]: the count of each 8x8 tile (of its first pixel; the tile's pixels share it)"""
    return np.ascontiguousarray(pixel_counts[::8, ::8], np.uint32)


# ---- taps: [(left, weights f32[n])] per output index --------------------------------------------------------------------------------
def lanczos_taps(oracle_mod, src, dst):
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


def box_taps(src, dst):
    """Source pixel i covers [i*dst, (i+1)*dst), output o covers [o*src, (o+1)*src): exact in Python integers; the weight is the
    overlap over src as a double (true division of two ints is correctly rounded), rounded once to f32."""
    out = []
    for o in range(dst):
        left, right = (o * src) // dst, -((-(o + 1) * src) // dst)
        w = [min((i + 1) * dst, (o + 1) * src) - max(i * dst, o * src) for i in range(left, right)]
        assert all(v > 0 for v in w) and sum(w) == src
        out.append((left, np.array([f32(v / src) for v in w], f32)))
    return out


def taps(oracle_mod, filter, src, dst):
    return lanczos_taps(oracle_mod, src, dst) if filter == "lanczos3" else box_taps(src, dst)


# ---- the two passes and the clamp ----------------------------------------------------------------------------------------------------
def resample(m, vt, ht):
    """u before the clamp: vertical pass, then horizontal pass, f32, one rounded product and one rounded add per tap"""
    m = np.asarray(m, f32)
    nh, nw, _ = m.shape
    with np.errstate(all="ignore"):
        t = np.zeros((len(vt), nw, 3), f32)
        for oy, (left, w) in enumerate(vt):
            acc = np.zeros((nw, 3), f32)
            for i, wi in enumerate(w):
                acc = (acc + (m[left + i] * f32(wi)).astype(f32)).astype(f32)
            t[oy] = acc
        u = np.zeros((len(vt), len(ht), 3), f32)
        for ox, (left, w) in enumerate(ht):
            acc = np.zeros((len(vt), 3), f32)
            for i, wi in enumerate(w):
                acc = (acc + (t[:, left + i] * f32(wi)).astype(f32)).astype(f32)
            u[:, ox] = acc
    return u


def clamp(u):
    """u > 0 ? u : 0: negative lobes, -0 and NaN give +0, +inf stays"""
    with np.errstate(invalid="ignore"):
        return np.where(u > 0, u, f32(0.0)).astype(f32)


def img_hdr(oracle_mod, m, res, filter, pre_clamp=False):
    """mrt_img_hdr of the means m [nh][nw][3] at the output resolution res = (w, h)"""
    nh, nw, _ = m.shape
    if (nw, nh) == tuple(res):
        u = np.asarray(m, f32)
    else:
        u = resample(m, taps(oracle_mod, filter, nh, res[1]), taps(oracle_mod, filter, nw, res[0]))
    return u if pre_clamp else clamp(u)


# ---- RGBE ----------------------------------------------------------------------------------------------------------------------------
def rgbe_encode(rgb):
    """uint8 [..., 4] of float32 [..., 3] by the rule of mrt_save_image_f32: round to nearest, in double"""
    rgb = np.asarray(rgb, f32)
    flat = rgb.reshape(-1, 3)
    out = np.zeros((flat.shape[0], 4), np.uint8)
    for k, px in enumerate(flat):
        c = [0.0 if (math.isnan(x) or x < 0) else min(float(x), FLT_MAX) for x in px]
        v = max(c)
        if v < 2.0 ** -127:
            continue
        E = math.frexp(v)[1]
        man = lambda: [math.floor(math.ldexp(x, 8 - E) + 0.5) for x in c]
        b = man()
        if max(b) >= 256:
            E += 1
            b = man()
        if E + 128 > 255:
            E = 127
            b = [min(x, 255) for x in man()]
        out[k] = (*b, E + 128)
    return out.reshape(rgb.shape[:-1] + (4,))


def rgbe_decode(px):
    """float32 [..., 3] of uint8 [..., 4]: b * 2^(e - 136), 0 for e == 0 -- exact in f32"""
    e = px[..., 3].astype(np.int32)
    scale = np.where(e == 0, f32(0.0), np.ldexp(f32(1.0), e - 136)).astype(f32)
    return (px[..., :3].astype(f32) * scale[..., None]).astype(f32)


# ---- PFM -----------------------------------------------------------------------------------------------------------------------------
def read_pfm(path):
    """float32 [h][w][3], top row first, of a colour PFM with a negative (little-endian) scale"""
    buf = open(path, "rb").read()
    parts, pos = [], 0
    for _ in range(3):
        end = buf.index(b"\n", pos)
        parts.append(buf[pos:end])
        pos = end + 1
    assert parts[0] == b"PF" and parts[2] == b"-1.0", parts
    w, h = (int(x) for x in parts[1].split())
    assert len(buf) - pos == w * h * 12
    return np.frombuffer(buf, "<f4", w * h * 3, pos).reshape(h, w, 3)[::-1].copy()
