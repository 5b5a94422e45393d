"""Cameras the reference does not have, as ray grids for Sampler.radiance (mrt_radiance): the caller forms the
primary rays, the path tracer behind a frame does the rest.  A grid of the frame's supersampled size goes back into the context
with set_accum, so that the tone map, the Lanczos3 resize and the writers produce the image as for any frame."""
import numpy as np

E = np.float32(0.0001)        # const E of the reference (src/rt.rs:7): a cast ray starts E along its direction


def equirect(pos, nw, nh, *, yaw=0.0, elevation=(-90.0, 90.0)):
    """(orig, dir), float32 [nh][nw][3], of an nw x nh lat-long grid seen from pos (z is up).  Column x has the azimuth
    2 pi ((x + 0.5) / nw - 0.5 + yaw) -- yaw in turns -- measured from +y towards +x, so the centre of the grid looks along +y
    turned by yaw; row y has the elevation upper - (y + 0.5) / nh (upper - lower) of elevation = (lower, upper) in degrees: row 0
    is the upper one.  Directions are formed in float64, normalised and rounded to float32; orig = pos + dir * E in float32, where
    the reference's own rays start."""
    lo, hi = (float(e) for e in elevation)
    az = 2.0 * np.pi * ((np.arange(nw, dtype=np.float64) + 0.5) / nw - 0.5 + float(yaw))
    el = np.radians(hi - (np.arange(nh, dtype=np.float64) + 0.5) / nh * (hi - lo))
    d = np.empty((nh, nw, 3), np.float64)
    d[..., 0] = np.cos(el)[:, None] * np.sin(az)[None, :]
    d[..., 1] = np.cos(el)[:, None] * np.cos(az)[None, :]
    d[..., 2] = np.sin(el)[:, None]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d = d.astype(np.float32)
    o = np.asarray(pos, np.float32).reshape(1, 1, 3) + d * E
    return o, d


def render_equirect(sampler, render, n_samples=None, *, yaw=0.0, elevation=(-90.0, 90.0), info=None, guides=False, adaptive=None):
    """Render the supersampled grid of render's frame as a panorama from its camera position (cam.dir, fov and aprt play no
    part) and put the sums into the sampler's context as n_samples accumulated samples: img() / img_ss() / the writers follow.
    guides: also install the first-hit AOVs of the same rays (Sampler.aov_rays), so that aov() and the denoisers belong to the
    panorama and not to the pinhole camera; the grid spans the full azimuth, so the filter wraps its horizontal taps (wrap_x).
    adaptive: a dict with `threshold` and optionally `min_samples` (32) and `step` (16): the grid is sampled tile-adaptively on
    these rays (Sampler.radiance_adaptive) with n_samples as the cap, which leaves the context in the adaptive state -- per-tile
    counts, and a half buffer that denoise(mode="variance") reads once guides is set; info then receives mrt_adapt_info.
    Returns the sums, float32 [nh][nw][3]."""
    n = int(render.rt.sample if n_samples is None else n_samples)
    sampler.create(render)
    o, d = equirect(render.frame.cam.pos, sampler.nw, sampler.nh, yaw=yaw, elevation=elevation)
    if adaptive is not None:
        unknown = set(adaptive) - {"threshold", "min_samples", "step"}
        if unknown or "threshold" not in adaptive:
            raise ValueError(f"render_equirect: adaptive is a dict of threshold, min_samples, step; got {sorted(adaptive)}")
        res = sampler.radiance_adaptive(render, o, d, adaptive["threshold"], min_samples=adaptive.get("min_samples", 32), max_samples=n,
                                        step=adaptive.get("step", 16))
        if info is not None:
            info.update(res)
        rgb = sampler.accum()[0]
    else:
        rgb = sampler.radiance(render, o, d, n, info=info)
        sampler.set_accum(rgb, n)
    if guides:
        sampler.aov_rays(render, o, d, wrap_x=True)       # equirect() always spans the full turn
    return rgb
