"""Reading what Sampler.gather returns, numpy only: the 9 real spherical harmonics of bands 0..2 in the order and
with the constants of mrt_gather (include/mrt.h), the radiance and the irradiance an SH9 probe stands for, and the texel grid of a
rectangular lightmap."""
import numpy as np

Y0 = 0.282094792        # 1 / (2 sqrt(pi))
Y1 = 0.488602512        # sqrt(3 / (4 pi))
Y2 = 1.092548431        # sqrt(15 / (4 pi))
Y20 = 0.315391565       # sqrt(5 / (16 pi))
Y22 = 0.546274215       # sqrt(15 / (16 pi))
# Ramamoorthi & Hanrahan 2001: the clamped-cosine kernel scales band l by A_l = pi, 2 pi / 3, pi / 4
BAND_FACTORS = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)


def sh9_basis(d):
    """Y_0..Y_8 at the directions d [..., 3] (unit length assumed) -> float64 [..., 9]"""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full_like(x, Y0), Y1 * y, Y1 * z, Y1 * x, Y2 * x * y, Y2 * y * z, Y20 * (3.0 * z * z - 1.0), Y2 * x * z,
                     Y22 * (x * x - y * y)], axis=-1)


def sh9_eval(sh, d):
    """The radiance the coefficients sh [..., 9, 3] stand for in the directions d [..., 3] -> float64 [..., 3]"""
    return np.einsum("...k,...kc->...c", sh9_basis(d), np.asarray(sh, np.float64))


def sh9_irradiance(sh, n):
    """The irradiance on a surface with unit normal n [..., 3] under the radiance of sh [..., 9, 3] -> float64 [..., 3]: each
    band scaled by its clamped-cosine factor (pi, 2 pi / 3, pi / 4).  Divided by pi it is what a HEMI_COS gather's mean estimates."""
    return np.einsum("...k,...kc->...c", sh9_basis(n) * BAND_FACTORS, np.asarray(sh, np.float64))


def lightmap_grid(origin, du, dv, w, h):
    """The texel centres of a w x h lightmap on the rectangle origin + s du + t dv (s, t in [0, 1]) and its normal:
    (pos float32 [h][w][3], normal float32 [h][w][3]); texel (x, y) sits at s = (x + 0.5) / w, t = (y + 0.5) / h and the normal is
    du x dv, normalised."""
    origin, du, dv = (np.asarray(a, np.float64) for a in (origin, du, dv))
    if w <= 0 or h <= 0:
        raise ValueError("lightmap_grid: w and h are positive")
    n = np.cross(du, dv)
    if not np.linalg.norm(n) > 0.0:
        raise ValueError("lightmap_grid: du and dv are parallel")
    s = (np.arange(w) + 0.5) / w
    t = (np.arange(h) + 0.5) / h
    pos = origin + s[None, :, None] * du + t[:, None, None] * dv
    normal = np.broadcast_to(n / np.linalg.norm(n), pos.shape)
    return pos.astype(np.float32), np.ascontiguousarray(normal, np.float32)
