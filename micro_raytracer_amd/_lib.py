"""Loader of libmrt_hip.so (the C ABI of include/mrt.h).  Fails loudly: there is no fallback path."""
import ctypes as C
import os
import subprocess

from . import _abi

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MRT_LIB") or os.path.join(_PKG, "libmrt_hip.so")   # MRT_LIB: experiment builds only
_LIB = None

# every symbol include/mrt.h declares
SYMBOLS = (
    "mrt_create", "mrt_destroy", "mrt_execute", "mrt_dims", "mrt_accum", "mrt_accum_local", "mrt_accum_device_ptr",
    "mrt_set_accum", "mrt_img", "mrt_img_ss", "mrt_reset", "mrt_get_stats", "mrt_last_error", "mrt_last_status",
    "mrt_abi_version", "mrt_device_count", "mrt_selftest_math", "mrt_padded_rows", "mrt_bind_accum",
    "mrt_set_accum_device", "mrt_save_image", "mrt_selftest_sweep", "mrt_plan_launch",
    "mrt_execute_adaptive", "mrt_sample_counts", "mrt_adapt_half",
    "mrt_aov", "mrt_denoise", "mrt_img_denoised",
    "mrt_create_ext", "mrt_plan_launch_ext",
    "mrt_selftest_trace", "mrt_selftest_instantiations",
    "mrt_radiance", "mrt_camera_rays",
    "mrt_img_hdr", "mrt_save_image_f32",
    "mrt_aov_rays",
    "mrt_radiance_adaptive",
    "mrt_gather", "mrt_gather_rays",
)


class MrtError(RuntimeError):
    """Err(String) of the reference's Result<_, String> (src/sampler.rs:80, src/cli.rs:155) + the ABI status code."""

    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code
        self.msg = msg


def build(force=False):
    """Compile libmrt_hip.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    csrc = os.path.join(_PKG, "csrc")
    args = ["make", "-C", csrc]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(micro_raytracer_amd has no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp, u32, u32p, f32p, u8p = C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    L.mrt_create.restype = vp
    L.mrt_create.argtypes = [vp, C.POINTER(_abi.Opts)]
    L.mrt_create_ext.restype = vp
    L.mrt_create_ext.argtypes = [vp, C.POINTER(_abi.Opts), vp]
    L.mrt_plan_launch_ext.argtypes = [vp, vp, C.POINTER(_abi.Plan)]
    L.mrt_destroy.restype = None
    L.mrt_destroy.argtypes = [vp]
    L.mrt_execute.argtypes = [vp, u32, C.POINTER(C.c_double)]
    L.mrt_execute_adaptive.argtypes = [vp, C.POINTER(_abi.Adapt), C.POINTER(_abi.AdaptInfo), C.POINTER(C.c_double)]
    L.mrt_sample_counts.argtypes = [vp, u32p]
    L.mrt_adapt_half.argtypes = [vp, f32p]
    L.mrt_aov.argtypes = [vp, f32p, f32p, f32p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.mrt_denoise.argtypes = [vp, C.POINTER(_abi.DenoiseOpts), f32p, C.POINTER(_abi.DenoiseInfo)]
    L.mrt_img_denoised.argtypes = [vp, C.POINTER(_abi.DenoiseOpts), u8p, C.POINTER(_abi.DenoiseInfo)]
    L.mrt_dims.argtypes = [vp, u32p, u32p, u32p]
    L.mrt_accum.argtypes = [vp, f32p, u32p]
    L.mrt_accum_local.argtypes = [vp, f32p, u32p]
    L.mrt_accum_device_ptr.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.mrt_set_accum.argtypes = [vp, f32p, u32]
    L.mrt_img.argtypes = [vp, u8p]
    L.mrt_img_ss.argtypes = [vp, u8p]
    L.mrt_reset.argtypes = [vp]
    L.mrt_get_stats.argtypes = [vp, C.POINTER(_abi.Stats)]
    L.mrt_last_error.restype = C.c_char_p
    L.mrt_last_status.restype = C.c_int
    L.mrt_abi_version.restype = u32
    L.mrt_device_count.restype = C.c_int
    L.mrt_padded_rows.argtypes = [vp, u32p]
    L.mrt_bind_accum.argtypes = [vp, vp, C.c_size_t]
    L.mrt_set_accum_device.argtypes = [vp, vp, u32]
    L.mrt_save_image.argtypes = [C.c_char_p, u8p, u32, u32]
    L.mrt_plan_launch.argtypes = [vp, C.POINTER(_abi.Plan)]
    L.mrt_selftest_math.argtypes = [C.c_int, C.c_int, f32p, f32p, f32p, C.c_size_t]
    L.mrt_selftest_sweep.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, u32, C.POINTER(C.c_uint64), f32p]
    L.mrt_selftest_trace.argtypes = [vp, C.c_size_t, f32p, f32p, u32p]
    L.mrt_selftest_instantiations.argtypes = [u32p, u32p, u32p, u32]
    L.mrt_radiance.argtypes = [vp, C.POINTER(_abi.Rays), vp, C.POINTER(_abi.RaysInfo)]
    L.mrt_camera_rays.argtypes = [vp, f32p, f32p]
    L.mrt_radiance_adaptive.argtypes = [vp, C.POINTER(_abi.RaysAdapt), C.POINTER(_abi.AdaptInfo), C.POINTER(C.c_double)]
    L.mrt_gather.argtypes = [vp, C.POINTER(_abi.Gather), vp, C.POINTER(_abi.GatherInfo)]
    L.mrt_gather_rays.argtypes = [vp, C.POINTER(_abi.Gather), C.c_size_t, C.c_size_t, vp, vp, vp]
    L.mrt_selftest_instantiations.restype = u32
    L.mrt_aov_rays.argtypes = [vp, vp, vp, u32]
    L.mrt_img_hdr.argtypes = [vp, C.POINTER(_abi.HdrOpts), f32p, C.POINTER(_abi.HdrInfo)]
    L.mrt_save_image_f32.argtypes = [C.c_char_p, f32p, u32, u32]
    _LIB = L
    return L


def check(rc):
    if rc != 0:
        L = lib()
        raise MrtError(rc, L.mrt_last_error().decode())


def plan_launch(render_or_holder):
    """What mrt_create would stage in LDS for this scene and the launch shape it would take (host only, no device needed)."""
    h = render_or_holder if hasattr(render_or_holder, "ptr") else _abi.build_desc(render_or_holder)
    pl = _abi.Plan()
    ext = h.ext_ptr() if hasattr(h, "ext_ptr") else None
    if ext is None:
        check(lib().mrt_plan_launch(C.cast(h.ptr(), C.c_void_p), C.byref(pl)))
    else:
        check(lib().mrt_plan_launch_ext(C.cast(h.ptr(), C.c_void_p), ext, C.byref(pl)))
    d = {k: getattr(pl, k) for k, _ in pl._fields_ if k != "reserved"}
    d["staging"] = _abi.STAGING[pl.staging]
    return d


def selftest_math(op, a, b=None, device=0):
    import numpy as np
    a = np.ascontiguousarray(a, np.float32)
    out = np.empty_like(a)
    bp = None
    if b is not None:
        b = np.ascontiguousarray(b, np.float32)
        bp = b.ctypes.data_as(C.POINTER(C.c_float))
    check(lib().mrt_selftest_math(device, op, a.ctypes.data_as(C.POINTER(C.c_float)), bp,
                                  out.ctypes.data_as(C.POINTER(C.c_float)), a.size))
    return out


def selftest_sweep(op, first, count, seed=1, device=0):
    """(mismatches, example[4]) of mrt_selftest_sweep: fast IEEE cores vs the compiler's expansions, on the device."""
    import numpy as np
    mis = C.c_uint64()
    ex = np.zeros(4, np.float32)
    check(lib().mrt_selftest_sweep(device, op, first, count, seed, C.byref(mis), ex.ctypes.data_as(C.POINTER(C.c_float))))
    return mis.value, ex


def selftest_trace(sampler_or_ctx, orig, dir):
    """mrt_selftest_trace: closest-hit queries on caller-supplied rays through the context's own kernel instantiation.  Ray i is
    lane i % 64 of wavefront i / 64.  Returns a dict of arrays over the n rays: hit, any (bool), renderer, instance (int32, -1 on
    a miss), t0, t1 (float32), normal (float32 [n][3]) and words, the raw uint32 [n][TRACE_WORDS] output."""
    import numpy as np
    ctx = getattr(sampler_or_ctx, "_ctx", sampler_or_ctx)
    if ctx is None:
        raise MrtError(_abi.MRT_ERR_STATE, "selftest_trace: the sampler has no context yet")
    orig, dir = np.ascontiguousarray(orig, np.float32), np.ascontiguousarray(dir, np.float32)
    if orig.ndim != 2 or orig.shape[1] != 3 or orig.shape != dir.shape:
        raise ValueError("selftest_trace: orig and dir are [n][3]")
    n = orig.shape[0]
    w = np.zeros((n, _abi.TRACE_WORDS), np.uint32)
    f32p = C.POINTER(C.c_float)
    check(lib().mrt_selftest_trace(ctx, n, orig.ctypes.data_as(f32p), dir.ctypes.data_as(f32p), w.ctypes.data_as(C.POINTER(C.c_uint32))))
    return {"hit": w[:, 0] != 0, "any": w[:, 1] != 0, "renderer": w[:, 2].astype(np.int32), "instance": w[:, 3].astype(np.int32),
            "t0": w[:, 4].view(np.float32), "t1": w[:, 5].view(np.float32), "normal": w[:, 6:9].view(np.float32), "words": w}


def selftest_instantiations():
    """mrt_selftest_instantiations: the compiled instantiations of the path-tracing kernel as a list of
    (block_threads, scene_in_lds, kernel_features) in the order of the launchers' lists.  Host only."""
    import numpy as np
    L = lib()
    n = L.mrt_selftest_instantiations(None, None, None, 0)
    t, l, f = (np.zeros(n, np.uint32) for _ in range(3))
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    if L.mrt_selftest_instantiations(p(t), p(l), p(f), n) != n:
        raise MrtError(_abi.MRT_ERR_STATE, "selftest_instantiations: the count changed between two calls")
    return [(int(a), bool(b), int(c)) for a, b, c in zip(t, l, f)]


def save_image(path, rgb8):
    """img.save(filename) (src/cli.rs:168,174) for .ppm / .png."""
    import numpy as np
    a = np.ascontiguousarray(rgb8, np.uint8)
    check(lib().mrt_save_image(str(path).encode(), a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0]))


def save_image_f32(path, rgb):
    """A float image [h][w][3] as a Radiance .hdr (RGBE, rounded to nearest) or a .pfm (the f32 values as given):
    mrt_save_image_f32."""
    import numpy as np
    a = np.ascontiguousarray(rgb, np.float32)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"save_image_f32: expected [h][w][3], got {a.shape}")
    check(lib().mrt_save_image_f32(str(path).encode(), a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[1], a.shape[0]))
