"""TEST INFRASTRUCTURE: numpy restatements of the contracts of mrt_gather (csrc/mrt_gather.h) and the x86 probe of
that header.

    dirs64 / frame64    the direction set and the frame in float64 (exact hash and lattice, libm sin / cos): what the f32 text is
                        measured against
    reduce              the reduction in f32, operation for operation: what the x86 build and the GPU must equal bit for bit
    probe / x86_*       tests/emu/gather_probe.cpp through tests/emu/build.py
"""
import ctypes as C

import numpy as np

from emu import build as B

f32 = np.float32
u32 = np.uint32
SPHERE, HEMI_COS = 0, 1
MEAN, SH9 = 0, 1
GOLD, ROT = 0x9E3779B9, 0x85EBCA6B
TWO_PI_F32 = float(f32(6.28318548))
M32 = 0xffffffff


# ---- hash ----------------------------------------------------------------------------------------------------------------------
def mix32(x):
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def seed_words(seed):
    return seed & M32, (seed >> 32) & M32


def rot_of(seed, key_base, i):
    lo, hi = seed_words(seed)
    pix_key = mix32((np.asarray(i, np.uint64) + key_base + lo) & M32) ^ hi
    return mix32((pix_key + ROT) & M32)


def keys_of(key_base, first, count, n_dirs):
    i = np.arange(first, first + count, dtype=np.uint64)[:, None]
    j = np.arange(n_dirs, dtype=np.uint64)[None, :]
    return ((key_base + i * n_dirs + j) & M32).astype(u32)


# ---- float64 restatement ---------------------------------------------------------------------------------------------------------
def frame64(n):
    """(unit n, t, bt) of Duff et al.'s frame about normals [..., 3], float64"""
    n = np.asarray(n, np.float64)
    n = n / np.sqrt((n * n).sum(-1, keepdims=True))
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    sg = np.copysign(1.0, z)
    a = -1.0 / (sg + z)
    b = x * y * a
    t = np.stack([1.0 + sg * x * x * a, sg * b, -sg * x], -1)
    bt = np.stack([b, sg + y * y * a, -y], -1)
    return n, t, bt


def dirs64(seed, key_base, n_points, n_dirs, dist, normal=None, first=0):
    """The directions [n_points][n_dirs][3] of points first .. in float64.  The hash, the 23-bit lattice and the f32 constant
    6.28318548 are the contract's own and exact here; everything after them is float64."""
    i = np.arange(first, first + n_points, dtype=np.uint64)
    rot = rot_of(seed, key_base, i)[:, None]
    j = np.arange(n_dirs, dtype=np.uint64)[None, :]
    a = (rot + j * GOLD) & M32
    phi = TWO_PI_F32 * ((a >> 9).astype(np.float64) * 2.0 ** -23)
    s, c = np.sin(phi), np.cos(phi)
    jj = (2.0 * j.astype(np.float64) + 1.0)
    if dist == SPHERE:
        z = 1.0 - jj / n_dirs
        q = np.sqrt(np.maximum(0.0, 1.0 - z * z))
        return np.stack([q * c, q * s, np.broadcast_to(z, c.shape)], -1)
    u = jj / (2.0 * n_dirs)
    lx, ly, lz = np.sqrt(u) * c, np.sqrt(u) * s, np.broadcast_to(np.sqrt(1.0 - u), c.shape)
    n, t, bt = (v[first:first + n_points, None, :] for v in frame64(normal))
    return t * lx[..., None] + bt * ly[..., None] + n * lz[..., None]


# ---- f32 reduction, bit for bit ----------------------------------------------------------------------------------------------------
def sh9_f32(d):
    """Y_0..Y_8 at the stored directions d [..., 3] as csrc/mrt_gather.h gather_sh9 spells them, f32 [..., 9]"""
    d = np.asarray(d, f32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    c1, c2 = f32(0.488602512), f32(1.092548431)
    return np.stack([np.full_like(x, f32(0.282094792)), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z),
                     f32(0.315391565) * (f32(3.0) * (z * z) - f32(1.0)), c2 * (x * z), f32(0.546274215) * (x * x - y * y)], -1)


def reduce(sums, dirs, n_samples, out):
    """sums, dirs [n_points][n_dirs][3] f32 -> [n_points][3] (MEAN) or [n_points][9][3] (SH9): lane l adds its terms j = l, l + 64,
    ... in rising j from +0, the 64 partials are combined pairwise at distances 32, 16, 8, 4, 2, 1, the result is scaled.
    Lanes and rows without a term add +0, which changes no partial: a partial starts at +0 and so is never -0."""
    sums, dirs = np.ascontiguousarray(sums, f32), np.ascontiguousarray(dirs, f32)
    n_points, n_dirs = sums.shape[:2]
    with np.errstate(all="ignore"):
        L = sums * (f32(1.0) / f32(n_samples))
        if out == SH9:
            terms = (L[:, :, None, :] * sh9_f32(dirs)[:, :, :, None]).reshape(n_points, n_dirs, 27)
            scale = f32(12.566370614) / f32(n_dirs)
        else:
            terms = L
            scale = f32(1.0) / f32(n_dirs)
        rows = (n_dirs + 63) // 64
        pad = np.zeros((n_points, rows * 64, terms.shape[2]), f32)
        pad[:, :n_dirs] = terms
        p = np.zeros((n_points, 64, terms.shape[2]), f32)
        for r in range(rows):
            p = p + pad[:, r * 64:(r + 1) * 64]
        off = 32
        while off:
            p = p[:, :off] + p[:, off:2 * off]
            off >>= 1
        res = p[:, 0] * scale
    return res.reshape((n_points, 9, 3) if out == SH9 else (n_points, 3))


def same_bits(a, b):
    """Words that differ between two f32 arrays, NaN equal to NaN: a NaN's sign and payload are not part of the contract, as in the
    project's other bit comparisons (what inf - inf or 0 * inf returns is the instruction set's choice; x86 makes 0xffc00000)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    assert a.shape == b.shape, (a.shape, b.shape)
    both_nan = np.isnan(a) & np.isnan(b)
    return int(np.count_nonzero((a.view(u32) != b.view(u32)) & ~both_nan))


# ---- the x86 probe -----------------------------------------------------------------------------------------------------------------
def _bind(L):
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    L.gp_rays.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, fp, fp, C.c_uint32, C.c_uint32, fp, fp, up]
    L.gp_rays.restype = None
    L.gp_frame.argtypes = [fp, fp, fp, fp]
    L.gp_frame.restype = None
    L.gp_reduce.argtypes = [C.c_uint32, fp, fp, C.c_uint32, C.c_uint32, C.c_uint32, fp]
    L.gp_layout.argtypes = [up]
    L.gp_layout.restype = None


def probe():
    return B.shared("gather_probe", _bind, with_pack=False, pthread=False)


def x86_rays(L, seed, key_base, n_dirs, dist, offset, pos, normal=None, first=0, count=None):
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    count = pos.shape[0] - first if count is None else count
    nrm = None if normal is None else np.ascontiguousarray(normal, f32).reshape(-1, 3)
    o, d = np.empty((count, n_dirs, 3), f32), np.empty((count, n_dirs, 3), f32)
    k = np.empty((count, n_dirs), u32)
    lo, hi = seed_words(seed)
    L.gp_rays(lo, hi, key_base, n_dirs, dist, offset, B.ptr(pos), None if nrm is None else B.ptr(nrm), first, count, B.ptr(o), B.ptr(d),
              B.ptr(k, C.c_uint32))
    return o, d, k


def x86_frame(L, normal):
    normal = np.ascontiguousarray(normal, f32).reshape(-1, 3)
    n, t, bt = (np.empty_like(normal) for _ in range(3))
    for i in range(normal.shape[0]):
        L.gp_frame(B.ptr(normal[i]), B.ptr(n[i]), B.ptr(t[i]), B.ptr(bt[i]))
    return n, t, bt


def x86_reduce(L, sums, dirs, n_samples, out):
    sums, dirs = np.ascontiguousarray(sums, f32), np.ascontiguousarray(dirs, f32)
    n_points, n_dirs = sums.shape[:2]
    res = np.empty((n_points, 9, 3) if out == SH9 else (n_points, 3), f32)
    assert L.gp_reduce(out, B.ptr(sums), B.ptr(dirs), n_points, n_dirs, n_samples, B.ptr(res)) == 0
    return res
