"""Python mirror of the reference's `Sampler` (src/sampler.rs:11-100) over the C ABI.

Same three entry points, same meaning:
    Sampler(workers, n_dim)              Sampler::new      (src/sampler.rs:19)
    execute(scene, frame, rt) -> secs    Sampler::execute  (src/sampler.rs:28)   one sample pass
    img(frame) -> uint8 [h][w][3]        Sampler::img      (src/sampler.rs:80)
`workers` / `n_dim` (the thread-pool size and tile grid of the CPU implementation) have no
meaning on the GPU and are accepted for signature compatibility only.  The context is created
lazily on the first execute, because the scene and frame only arrive then, exactly as the
Rust shim in INTEGRATION.md does.
"""
from __future__ import annotations

import ctypes as C
import math
import zlib

import numpy as np

from . import _abi, _lib
from .scene import Render


def _fingerprint(render: Render):
    """What the device context was built from, cheap enough to recompute on every execute (the reference's
    Sampler::execute receives scene, frame and rt on every call, src/sampler.rs:28): every scalar and small vector by
    value; bulk arrays (mesh triangles, texels, long instance lists) by shape, dtype and a CRC of a strided sample of
    at most ~4 K elements -- an in-place edit of a few elements of a large array between two sample elements is NOT
    seen (call Sampler.invalidate() after such an edit); anything that replaces, resizes or rewrites the array is.
    Bulk data that is not an ndarray (a Python list assigned after load_render) is converted and hashed whole on every
    call: correct, but slow -- keep bulk data as ndarrays, as load_render leaves it."""
    def arr(a):
        if a is None:
            return None
        if not isinstance(a, np.ndarray):
            a = np.asarray(a)
            return (a.shape, a.dtype.str, zlib.crc32(a.tobytes()))
        if a.size <= 64:
            return a.tobytes()
        flat = a.reshape(-1)
        step = max(1, flat.size // 4096)
        return (a.shape, a.dtype.str, zlib.crc32(np.ascontiguousarray(flat[::step]).tobytes()), zlib.crc32(flat[-16:].tobytes()))

    def tex(t):
        return None if t is None else (t.w, t.h, arr(t.dat))

    def insts(lst):
        if len(lst) <= 16:
            return tuple((arr(p), arr(d)) for p, d in lst)
        step = max(1, len(lst) // 64)
        return (len(lst), tuple((arr(p), arr(d)) for p, d in lst[::step]), arr(lst[-1][0]), arr(lst[-1][1]))

    cam = render.frame.cam
    out = [render.rt.bounce, render.rt.loss, tuple(render.frame.res), render.frame.ssaa,
           arr(cam.pos), arr(cam.dir), cam.fov, cam.gamma, cam.exp, cam.aprt, cam.foc,
           arr(render.scene.sky.color), render.scene.sky.pwr]
    sky = render.scene.sky
    if getattr(sky, "tex", None) is not None:
        out.append(("env", tex(sky.tex), sky.mapping, sky.rot, getattr(sky, "filter", "nearest")))
    out.append(("tex_filter", getattr(render.scene, "tex_filter", "nearest")))
    for l in render.scene.light:
        out.append((l.kind, arr(l.v), l.pwr, arr(l.color)))
    for o in render.scene.renderer:
        m = o.mat
        out.append((o.kind, o.r, arr(o.n), arr(o.sizes), arr(o.vtx), arr(o.mesh), arr(o.uv), arr(o.vn), arr(m.albedo), m.rough, m.metal, m.glass,
                    m.opacity, m.emit, tuple(tex(getattr(m, k)) for k in _abi.MAP_SLOTS), insts(o.inst)))
    return tuple(out)


def _ray_args(fn, orig, dir, shape, key=None, mixed=None):
    """A pair of ray arrays as the C ABI takes them, for the caller named fn.  shape: what both must be ((nh, nw, 3)), or None for
    any [..., 3] with equal shapes.  key: optional 32-bit words, one per ray.  mixed: the caller's text for inputs that are not all
    on one side.  Numpy arrays go through the host; torch tensors on a device are read in place, after a synchronize of that
    device (the library launches on a stream of its own).  Returns (keep, (orig_ptr, dir_ptr, key_ptr), on_device): keep holds the
    contiguous f32 orig and dir, then the key words if any, and must outlive the call the pointers go to."""
    def check(so, sd):
        if shape is None:
            if so != sd or so[-1] != 3:
                raise ValueError(f"{fn}: orig and dir are [..., 3]")
        elif so != shape or sd != shape:
            raise ValueError(f"{fn}: orig and dir are {shape}, got {so} and {sd}")

    dev = type(orig).__module__.split(".")[0] == "torch"
    if dev:
        import torch
        if not (orig.is_cuda and getattr(dir, "is_cuda", False)) or (key is not None and not getattr(key, "is_cuda", False)):
            raise ValueError(mixed or f"{fn}: orig and dir are both tensors on the context's device, or both host arrays")
        check(tuple(orig.shape), tuple(dir.shape))
        keep = (orig.to(torch.float32).contiguous(), dir.to(torch.float32).contiguous())
        if key is not None:
            words = (torch.int32, getattr(torch, "uint32", torch.int32))          # the same 32 bits either way
            keep += ((key if key.dtype in words else key.to(torch.int64).to(torch.int32)).contiguous(),)
    else:
        keep = (np.ascontiguousarray(orig, np.float32), np.ascontiguousarray(dir, np.float32))
        check(keep[0].shape, keep[1].shape)
        if key is not None:
            keep += (np.ascontiguousarray(key, np.uint32),)
    if key is not None and math.prod(keep[2].shape) != math.prod(keep[0].shape[:-1]):
        raise ValueError(f"{fn}: one key per ray")
    if dev:
        torch.cuda.synchronize(keep[0].device)
    return keep, [a.data_ptr() if dev else a.ctypes.data for a in keep] + [None] * (key is None), dev


def _fill_rule(a, render, threshold, min_samples, max_samples, step):
    """The stop rule of both adaptive calls into an _abi.Adapt (max_samples of None: render.rt.sample)"""
    a.min_samples = int(min_samples)
    a.max_samples = int(render.rt.sample if max_samples is None else max_samples)
    a.step = int(step)
    a.threshold = float(threshold)


def _adapt_out(info, secs) -> dict:
    """mrt_adapt_info as a dict plus the wall time ("seconds")"""
    return {**_abi.as_dict(info), "seconds": secs.value}


def _dn_info(info, di):
    """mrt_denoise_info (and "mode", its reserved[0]) into the caller's dict, if there is one"""
    if info is not None:
        info.update(_abi.as_dict(di), mode=int(di.reserved[0]))


class Sampler:
    def __init__(self, workers: int = 24, n_dim: int = 64, *, seed: int = 1, device: int = -1,
                 shard_index: int = 0, shard_count: int = 1, shard_rows: int = 8, n_devices: int = 0, flags: int = 0):
        self.workers, self.n_dim = workers, n_dim
        self.seed, self.device = seed, device
        self.shard_index, self.shard_count, self.shard_rows = shard_index, shard_count, shard_rows
        self.n_devices = n_devices      # > 1: one process drives that many GPUs (RCCL gather inside mrt_execute)
        self.flags = flags              # _abi.FLAG_COUNT_SEGMENTS: keep the path-segment counter (stats()["segments"])
        self._ctx = None
        self._holder = None
        self._render = None             # strong reference: the context belongs to THIS description (id() of a dead
        self._print = None              # temporary is reused by CPython), and to its contents at creation time
        self._bound = None              # (device pointer, bytes) of a caller-owned accumulator (bind_accum), re-applied after a rebuild
        self.nw = self.nh = self.local_rows = 0
        self.res = (0, 0)

    # -- context -----------------------------------------------------------------------------
    def _ensure(self, render: Render):
        fp = _fingerprint(render)
        if self._ctx is not None and render is self._render and fp == self._print:
            return
        # Another description, or this one edited in place: the device context is rebuilt from what is passed NOW.
        # Like the reference's Sampler, what has been accumulated so far is kept when the supersampled frame keeps
        # its size (src/sampler.rs:60-70 adds into the same map whatever the scene); a different size starts afresh.
        # A context that owns only some rows (shard_count > 1) or several devices has no entry point that restores
        # its rows and their sample count, so rebuilding it with samples on board would silently desynchronise the
        # caller's view (the bound buffer, ShardedSampler.count): that is an error, not a quiet restart.
        carry = None
        bound = self._bound
        if self._ctx is not None:
            same_size = (self.nw, self.nh) == (render.frame.nw, render.frame.nh)
            whole = self.shard_count == 1 and self.n_devices <= 1
            if not whole and self._count() > 0:
                raise _lib.MrtError(_abi.MRT_ERR_STATE, "the render description changed under a sharded / multi-device context that "
                                    "already holds samples: create a new Sampler (or reset() first)")
            if whole and same_size:
                carry = self.accum()
            if not same_size:
                bound = None                 # the caller's buffer was sized for the old frame
        self.close()
        L = _lib.lib()
        self._holder = _abi.build_desc(render)
        opts = _abi.Opts()
        opts.abi_version = _abi.ABI_VERSION
        opts.seed = self.seed
        opts.device = self.device
        opts.shard_index, opts.shard_count, opts.shard_rows = self.shard_index, self.shard_count, self.shard_rows
        opts.n_devices = self.n_devices
        opts.flags = self.flags
        if self._holder.ext is None:
            ctx = L.mrt_create(C.cast(self._holder.ptr(), C.c_void_p), C.byref(opts))
        else:                   # per-corner uv / vn on a triangle or mesh, an environment texture on the sky, or filtered textures
            ctx = L.mrt_create_ext(C.cast(self._holder.ptr(), C.c_void_p), C.byref(opts), self._holder.ext_ptr())
        if not ctx:
            raise _lib.MrtError(L.mrt_last_status(), L.mrt_last_error().decode())
        self._ctx, self._render, self._print = ctx, render, fp
        nw, nh, lr = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _lib.check(L.mrt_dims(ctx, C.byref(nw), C.byref(nh), C.byref(lr)))
        self.nw, self.nh, self.local_rows = nw.value, nh.value, lr.value
        self.res = tuple(render.frame.res)
        if bound is not None:
            self.bind_accum(*bound)          # the new context renders into the caller's buffer again (zeroed by the bind)
        if carry is not None and carry[1] > 0:
            self.set_accum(*carry)

    def _count(self) -> int:
        cnt = C.c_uint32()
        _lib.check(_lib.lib().mrt_accum(self._ctx, None, C.byref(cnt)))
        return cnt.value

    def invalidate(self):
        """Force the next execute to rebuild the device context from the description it is given (after an in-place
        edit of bulk data the fingerprint cannot see)."""
        self._print = None

    def close(self):
        if self._ctx is not None:
            _lib.lib().mrt_destroy(self._ctx)
            self._ctx = None
        self._render = self._print = None
        self._bound = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the reference's API -----------------------------------------------------------------
    def execute(self, scene_or_render, frame=None, rt=None, n_samples: int = 1) -> float:
        """One Sampler::execute pass (n_samples > 1: that many consecutive passes in one launch).

        Accepts either a whole Render, or (scene, frame, rt) like the reference."""
        render = scene_or_render if isinstance(scene_or_render, Render) else Render(rt=rt, frame=frame, scene=scene_or_render)
        if not isinstance(scene_or_render, Render):
            # keep one Render object per (scene, frame, rt) triple so the context is reused across passes
            k = (id(scene_or_render), id(frame), id(rt))
            if getattr(self, "_triple_key", None) == k:
                render = self._triple_render
            else:
                self._triple_key, self._triple_render = k, render
        self._ensure(render)
        secs = C.c_double()
        _lib.check(_lib.lib().mrt_execute(self._ctx, n_samples, C.byref(secs)))
        return secs.value

    def execute_adaptive(self, render: Render, threshold: float, min_samples: int = 32, max_samples=None, step: int = 16) -> dict:
        """Tile-adaptive sampling (mrt_execute_adaptive): rounds of `step` samples; from `min_samples` on, every 8x8 tile whose
        noise estimate is <= `threshold` after an even number of rounds stops, none goes past `max_samples` (default
        render.rt.sample).  Needs a context without samples (a fresh Sampler, or reset()).  Returns mrt_adapt_info as a dict
        plus the wall time ("seconds")."""
        self._ensure(render)
        a = _abi.Adapt()
        _fill_rule(a, render, threshold, min_samples, max_samples, step)
        info = _abi.AdaptInfo()
        secs = C.c_double()
        _lib.check(_lib.lib().mrt_execute_adaptive(self._ctx, C.byref(a), C.byref(info), C.byref(secs)))
        return _adapt_out(info, secs)

    def sample_counts(self) -> np.ndarray:
        """Samples accumulated per supersampled pixel, uint32 [nh][nw]."""
        self._need()
        out = np.empty((self.nh, self.nw), np.uint32)
        _lib.check(_lib.lib().mrt_sample_counts(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def adapt_half(self) -> np.ndarray:
        """The half buffer of the last adaptive call: per pixel the f32 sum of its even-numbered rounds, [nh][nw][3]."""
        self._need()
        out = np.empty((self.nh, self.nw, 3), np.float32)
        _lib.check(_lib.lib().mrt_adapt_half(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def img(self, frame=None) -> np.ndarray:
        self._need()
        out = np.empty((self.res[1], self.res[0], 3), np.uint8)
        _lib.check(_lib.lib().mrt_img(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def aov(self) -> dict:
        """First-hit AOVs of the supersampled frame (mrt_aov): depth f32 [nh][nw] (inf: miss), normal and albedo f32
        [nh][nw][3], renderer and instance int32 [nh][nw] (indices into the scene's renderers and that renderer's instances,
        -1: miss).  Computed once per context and kept; after aov_rays() the planes of those rays."""
        self._need()
        out = {"depth": np.empty((self.nh, self.nw), np.float32), "normal": np.empty((self.nh, self.nw, 3), np.float32),
               "albedo": np.empty((self.nh, self.nw, 3), np.float32), "renderer": np.empty((self.nh, self.nw), np.int32),
               "instance": np.empty((self.nh, self.nw), np.int32)}
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        _lib.check(_lib.lib().mrt_aov(self._ctx, out["depth"].ctypes.data_as(fp), out["normal"].ctypes.data_as(fp),
                                      out["albedo"].ctypes.data_as(fp), out["renderer"].ctypes.data_as(ip),
                                      out["instance"].ctypes.data_as(ip)))
        return out

    def aov_rays(self, render: Render, orig, dir, *, wrap_x: bool = False):
        """Install the first-hit AOVs of a custom camera (mrt_aov_rays): orig and dir of shape [nh][nw][3], one
        ray per supersampled pixel, traced as given.  From then on aov(), denoise(), img_denoised() and img_hdr(denoise=...) use
        these planes; reset() and set_accum() keep them.  wrap_x: the grid is periodic in x (a full 360-degree panorama), the
        filter takes its horizontal taps modulo the width.  Numpy arrays go through the host, torch tensors on the context's
        device are read in place.  aov_rays(render, None, None) returns to the camera's own AOVs.  Nothing else of the context
        changes."""
        self._ensure(render)
        L = _lib.lib()
        if orig is None and dir is None:
            if wrap_x:
                raise ValueError("aov_rays: wrap_x without rays")
            _lib.check(L.mrt_aov_rays(self._ctx, None, None, 0))
            return
        if orig is None or dir is None:
            raise ValueError("aov_rays: orig and dir are both given, or both None")
        keep, (po, pd, _), dev = _ray_args("aov_rays", orig, dir, (self.nh, self.nw, 3))
        _lib.check(L.mrt_aov_rays(self._ctx, po, pd, (_abi.AOV_WRAP_X if wrap_x else 0) | (_abi.AOV_RAYS_DEVICE if dev else 0)))
        del keep

    def denoise(self, passes=_abi.DENOISE_PASSES, sigma_color=None, sigma_normal=None, sigma_plane=None, info=None, mode="atrous",
                sigma_var=None, firefly=None) -> np.ndarray:
        """The accumulated means filtered by the AOV-guided a-trous filter (mrt_denoise), f32 [nh][nw][3].  info: a dict that
        receives mrt_denoise_info (and "mode").  mode "variance": the colour term follows a per-pixel variance estimate from the
        half buffer, so it needs an execute_adaptive() on this context (threshold=0, min_samples=max_samples=n for a uniform
        budget) -- or, with the guides of aov_rays(), a radiance_adaptive() on the same rays; sigma_var / firefly of None take the library's defaults, firefly=float("inf") switches the clamp off."""
        self._need()
        o = _abi.denoise_opts(passes, sigma_color, sigma_normal, sigma_plane, mode, sigma_var, firefly)
        out = np.empty((self.nh, self.nw, 3), np.float32)
        di = _abi.DenoiseInfo()
        _lib.check(_lib.lib().mrt_denoise(self._ctx, C.byref(o), out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(di)))
        _dn_info(info, di)
        return out

    def img_denoised(self, passes=_abi.DENOISE_PASSES, sigma_color=None, sigma_normal=None, sigma_plane=None, info=None, mode="atrous",
                     sigma_var=None, firefly=None) -> np.ndarray:
        """img() of the denoised means (mrt_img_denoised), uint8 [res_h][res_w][3]; the options of denoise()."""
        self._need()
        o = _abi.denoise_opts(passes, sigma_color, sigma_normal, sigma_plane, mode, sigma_var, firefly)
        out = np.empty((self.res[1], self.res[0], 3), np.uint8)
        di = _abi.DenoiseInfo()
        _lib.check(_lib.lib().mrt_img_denoised(self._ctx, C.byref(o), out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(di)))
        _dn_info(info, di)
        return out

    def img_hdr(self, filter="lanczos3", denoise=None, info=None) -> np.ndarray:
        """The linear float image (mrt_img_hdr), float32 [res_h][res_w][3]: the mean radiance resampled in f32 to the
        output resolution, no tone map, no quantisation, clamped at 0.  filter "lanczos3" (the taps of img()) or "box" (area
        average, no ringing around a sun: what a light probe wants).  denoise: None for the means, or a dict of denoise()
        arguments for the filtered means.  info: a dict that receives resize_ms and, with denoise, mrt_denoise_info."""
        self._need()
        if filter not in _abi.RESIZE_FILTERS:
            raise ValueError(f"resize filter `{filter}`: expected one of {sorted(_abi.RESIZE_FILTERS)}")
        o = _abi.HdrOpts()
        o.filter = _abi.RESIZE_FILTERS[filter]
        dn = None
        if denoise is not None:
            dn = _abi.denoise_opts(**denoise)
            o.denoise = C.pointer(dn)
        out = np.empty((self.res[1], self.res[0], 3), np.float32)
        hi = _abi.HdrInfo()
        _lib.check(_lib.lib().mrt_img_hdr(self._ctx, C.byref(o), out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(hi)))
        if info is not None:
            info["resize_ms"] = hi.resize_ms
            if dn is not None:
                _dn_info(info, hi.dn)
        return out

    # -- radiance along caller-supplied rays (mrt_radiance) --------------------
    def camera_rays(self, render: Render):
        """(orig, dir), float32 [nh][nw][3]: the lens-centre camera ray of every supersampled pixel (mrt_camera_rays) -- with
        aprt == 0 the ray of every sample of the pixel."""
        self._ensure(render)
        o, d = (np.empty((self.nh, self.nw, 3), np.float32) for _ in range(2))
        fp = C.POINTER(C.c_float)
        _lib.check(_lib.lib().mrt_camera_rays(self._ctx, o.ctypes.data_as(fp), d.ctypes.data_as(fp)))
        return o, d

    def radiance(self, render: Render, orig, dir, n_samples: int, *, sample_base: int = 0, key=None, info=None):
        """Path-trace caller-supplied rays (mrt_radiance): orig and dir of shape [..., 3] -> the f32 SUM of samples
        [sample_base, sample_base + n_samples) of every ray in the canonical order, in the rays' shape.  Rays are traced as given
        (no shift of the origin, no normalisation).  key (uint32, the rays' shape without the 3; default: the ray's flat index)
        stands where a frame's pixel index stands in the random numbers.  Numpy arrays go through the host; torch tensors on the
        context's device are read and written in place on the device and a tensor comes back.  info: a dict that receives
        mrt_rays_info.  Nothing of the context changes."""
        self._ensure(render)
        r = _abi.Rays()
        r.sample_base, r.n_samples = int(sample_base), int(n_samples)
        keep, (r.orig, r.dir, r.key), dev = _ray_args("radiance", orig, dir, None, key,
                                                      "radiance: orig, dir and key are all tensors on the context's device, or all host arrays")
        r.n, r.flags = math.prod(keep[0].shape[:-1]), _abi.RAYS_DEVICE if dev else 0
        out = keep[0].new_empty(keep[0].shape) if dev else np.empty_like(keep[0])
        ri = _abi.RaysInfo()
        _lib.check(_lib.lib().mrt_radiance(self._ctx, C.byref(r), C.c_void_p(out.data_ptr() if dev else out.ctypes.data), C.byref(ri)))
        del keep
        if info is not None:
            info.update(_abi.as_dict(ri))
        return out

    def radiance_adaptive(self, render: Render, orig, dir, threshold: float, min_samples: int = 32, max_samples=None, step: int = 16) -> dict:
        """execute_adaptive() on a custom camera (mrt_radiance_adaptive): orig and dir of shape [nh][nw][3], one ray
        per supersampled pixel, traced as given with the pixel index as the hash key; rounds, rule and the returned dict are
        those of execute_adaptive().  Needs a context without samples.  Afterwards the context holds the adaptive render of these
        rays: accum(), sample_counts(), adapt_half(), img*() and denoise() serve it, and denoise(mode="variance") works once
        aov_rays() has installed the guides of the same rays.  Numpy arrays go through the host (one upload per call), torch
        tensors on the context's device are read in place."""
        self._ensure(render)
        r = _abi.RaysAdapt()
        _fill_rule(r.rule, render, threshold, min_samples, max_samples, step)
        keep, (r.orig, r.dir, _), dev = _ray_args("radiance_adaptive", orig, dir, (self.nh, self.nw, 3))
        r.flags = _abi.RAYS_DEVICE if dev else 0
        info = _abi.AdaptInfo()
        secs = C.c_double()
        _lib.check(_lib.lib().mrt_radiance_adaptive(self._ctx, C.byref(r), C.byref(info), C.byref(secs)))
        del keep
        return _adapt_out(info, secs)

    # -- point gathers (mrt_gather) --------------------------------------------
    def _gather_desc(self, fn, pos, normal, n_dirs, n_samples, out, key_base, offset, sample_base, batch_points):
        """(keep, desc, on_device) of both gather calls: pos (and normal) by the rules of _ray_args, flattened to [n][3]"""
        if out not in _abi.GATHER_OUTS:
            raise ValueError(f"{fn}: out `{out}`: expected one of {sorted(_abi.GATHER_OUTS)}")
        keep, (pp, pn, _), dev = _ray_args(fn, pos, pos if normal is None else normal, None,
                                           mixed=f"{fn}: pos and normal are both tensors on the context's device, or both host arrays")
        g = _abi.Gather()
        g.n, g.pos, g.normal = math.prod(keep[0].shape[:-1]), pp, None if normal is None else pn
        g.n_dirs, g.n_samples, g.sample_base = int(n_dirs), int(n_samples), int(sample_base)
        g.dist = _abi.GATHER_SPHERE if normal is None else _abi.GATHER_HEMI_COS
        g.out, g.key_base, g.offset, g.batch_points = _abi.GATHER_OUTS[out], int(key_base) & 0xffffffff, float(offset), int(batch_points)
        g.flags = _abi.RAYS_DEVICE if dev else 0
        return keep, g, dev

    def gather(self, render: Render, pos, normal=None, n_dirs: int = 64, n_samples: int = 16, out: str = "mean", key_base: int = 0,
               offset: float = 1e-4, sample_base: int = 0, batch_points: int = 0, info=None):
        """Gather radiance at points (mrt_gather): pos of shape [..., 3]; n_dirs rays per point over the whole sphere (normal None)
        or cosine-distributed over the hemisphere about normal [..., 3] (any length), each path-traced n_samples times, formed,
        traced and reduced on the device.  out "mean": f32 [..., 3], the mean radiance over the set (with a normal: irradiance /
        pi); "sh9" (sphere only): f32 [..., 9, 3], the radiance projected on the 9 real spherical harmonics of bands 0..2
        (probes.sh9_eval, probes.sh9_irradiance read them).  Point i has the key key_base + i; rays start offset along their
        direction (sphere) or along the unit normal (hemisphere).  Numpy arrays go through the host; torch tensors on the
        context's device are read and written in place on the device and a tensor comes back.  info: a dict that receives
        mrt_gather_info.  Nothing of the context changes."""
        self._ensure(render)
        keep, g, dev = self._gather_desc("gather", pos, normal, n_dirs, n_samples, out, key_base, offset, sample_base, batch_points)
        shape = tuple(keep[0].shape[:-1]) + ((9, 3) if out == "sh9" else (3,))
        res = keep[0].new_empty(shape) if dev else np.empty(shape, np.float32)
        gi = _abi.GatherInfo()
        _lib.check(_lib.lib().mrt_gather(self._ctx, C.byref(g), C.c_void_p(res.data_ptr() if dev else res.ctypes.data), C.byref(gi)))
        del keep
        if info is not None:
            info.update(_abi.as_dict(gi))
        return res

    def gather_rays(self, render: Render, pos, normal=None, n_dirs: int = 64, key_base: int = 0, offset: float = 1e-4, first: int = 0,
                    count=None):
        """(orig, dir, key) of the rays gather() forms for points [first, first + count) of the flattened pos (mrt_gather_rays):
        f32 [count][n_dirs][3] twice and the hash keys uint32 [count][n_dirs] -- what radiance(orig, dir, n, key=key) takes.  count
        None: every point from first on.  Numpy in, numpy out; torch tensors on the context's device in, tensors out."""
        self._ensure(render)
        keep, g, dev = self._gather_desc("gather_rays", pos, normal, n_dirs, 1, "mean", key_base, offset, 0, 0)
        count = g.n - int(first) if count is None else int(count)
        if first < 0 or count < 0:
            raise ValueError("gather_rays: first and count are >= 0")
        shape = (count, int(n_dirs))
        if dev:
            import torch
            o, d = keep[0].new_empty(shape + (3,)), keep[0].new_empty(shape + (3,))
            k = torch.empty(shape, dtype=getattr(torch, "uint32", torch.int32), device=keep[0].device)
            ptrs = [C.c_void_p(a.data_ptr()) for a in (o, d, k)]
        else:
            o, d, k = np.empty(shape + (3,), np.float32), np.empty(shape + (3,), np.float32), np.empty(shape, np.uint32)
            ptrs = [C.c_void_p(a.ctypes.data) for a in (o, d, k)]
        _lib.check(_lib.lib().mrt_gather_rays(self._ctx, C.byref(g), int(first), count, *ptrs))
        del keep
        return o, d, k

    # -- extras of the C ABI -----------------------------------------------------------------
    def _need(self):
        if self._ctx is None:
            raise _lib.MrtError(_abi.MRT_ERR_STATE, "no context: call execute() first")

    def img_ss(self) -> np.ndarray:
        self._need()
        out = np.empty((self.nh, self.nw, 3), np.uint8)
        _lib.check(_lib.lib().mrt_img_ss(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def accum(self):
        """(colors, last_count): full-frame f32 sums [nh][nw][3] (rows of other shards are zero)."""
        self._need()
        out = np.zeros((self.nh, self.nw, 3), np.float32)
        cnt = C.c_uint32()
        _lib.check(_lib.lib().mrt_accum(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(cnt)))
        return out, cnt.value

    def accum_local(self):
        self._need()
        out = np.zeros((self.local_rows, self.nw, 3), np.float32)
        rows = np.zeros(self.local_rows, np.uint32)
        _lib.check(_lib.lib().mrt_accum_local(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float)),
                                              rows.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out, rows

    def accum_device_ptr(self):
        self._need()
        p, n = C.c_void_p(), C.c_size_t()
        _lib.check(_lib.lib().mrt_accum_device_ptr(self._ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    def padded_rows(self) -> int:
        self._need()
        n = C.c_uint32()
        _lib.check(_lib.lib().mrt_padded_rows(self._ctx, C.byref(n)))
        return n.value

    def bind_accum(self, dev_ptr, nbytes):
        """Render into caller-owned device memory (a torch tensor's data_ptr()) from now on."""
        self._need()
        _lib.check(_lib.lib().mrt_bind_accum(self._ctx, C.c_void_p(dev_ptr), nbytes))
        self._bound = (dev_ptr, nbytes) if dev_ptr else None

    def set_accum_device(self, dev_ptr, count):
        self._need()
        _lib.check(_lib.lib().mrt_set_accum_device(self._ctx, C.c_void_p(dev_ptr), int(count)))

    def create(self, render):
        """Create the context without rendering (Sampler::new + scene upload)."""
        self._ensure(render)
        return self

    def set_accum(self, rgb, count):
        self._need()
        rgb = np.ascontiguousarray(rgb, np.float32)
        if rgb.shape != (self.nh, self.nw, 3):
            raise ValueError(f"expected {(self.nh, self.nw, 3)}, got {rgb.shape}")
        _lib.check(_lib.lib().mrt_set_accum(self._ctx, rgb.ctypes.data_as(C.POINTER(C.c_float)), int(count)))

    def reset(self):
        self._need()
        _lib.check(_lib.lib().mrt_reset(self._ctx))

    def stats(self) -> dict:
        self._need()
        st = _abi.Stats()
        _lib.check(_lib.lib().mrt_get_stats(self._ctx, C.byref(st)))
        return _abi.as_dict(st)


def raytrace(render: Render, *, seed=1, update=None, batch=None, **kw):
    """CLI::raytrace / HttpServer::raytrace (src/cli.rs:155-177, src/http.rs:136-148): the per-sample loop
    followed by img().  `update(sample_index, image)` mirrors --update; `batch` fuses that many passes
    into one launch when no per-sample image is needed."""
    s = Sampler(kw.pop("workers", 24), kw.pop("n_dim", 64), seed=seed, **kw)
    n = render.rt.sample
    if update is None:
        step = batch or n
        done = 0
        while done < n:
            k = min(step, n - done)
            s.execute(render, n_samples=k)
            done += k
    else:
        for i in range(n):
            s.execute(render)
            update(i, s.img())
    out = s.img()
    s.close()
    return out
