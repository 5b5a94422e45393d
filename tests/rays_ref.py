"""TEST INFRASTRUCTURE for tests/test_rays_host.py and tests/test_gpu_rays.py: the x86 probe of mrt_radiance's per-ray body
(tests/emu/rays_probe.cpp), the scenes and ray sets both modules share, and the float64 yardstick of rays no pinhole forms:
core_ref.render_image with its only source of rays, core_ref.camera_rays, replaced by the window's."""
import ctypes as C
import functools

import numpy as np

import core_cases as K
import core_ref as R
from conftest import make_holder
from emu.build import desc_ptrs as _ptrs, ptr as _p, shared

f32 = np.float32
RES, SPP, SEED = (50, 37), 40, 5          # 1850 rays: a partial last wavefront and workgroup; chunks of 16, 16, 8
WIN = (96, 40)                            # the lat-long windows of the float64 comparison
F_TRI, F_ALL, F_BVH, F_IDENT, F_VATTR, F_ENV = 2, 15, 16, 256, 512, 1024


# ---- the probe ---------------------------------------------------------------------------------------------------------------
def _bind(L):
    fp, u32p, vp, u32 = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32
    L.ry_error.restype = C.c_char_p
    L.ry_info.argtypes = [vp, vp, u32p]
    L.ry_camera_rays.argtypes = [vp, vp, fp, fp]
    L.ry_radiance.argtypes = [vp, vp, u32, C.c_uint64, u32, u32, u32, fp, fp, u32p, u32, fp, C.POINTER(C.c_uint64)]


def shared_probe():
    """The probe, built once per process (half a minute) for every module that uses it."""
    return shared("rays_probe", _bind)


INFO_KEYS = ("nw", "nh", "features", "own_inst", "rays_inst", "axis_scan", "lds_words")


def x86_info(L, holder):
    v = np.zeros(8, np.uint32)
    rc = L.ry_info(*_ptrs(holder), _p(v, C.c_uint32))
    assert rc == 0, L.ry_error()
    return dict(zip(INFO_KEYS, (int(x) for x in v)))


def x86_camera_rays(L, holder):
    i = x86_info(L, holder)
    o, d = np.zeros((i["nh"], i["nw"], 3), f32), np.zeros((i["nh"], i["nw"], 3), f32)
    rc = L.ry_camera_rays(*_ptrs(holder), _p(o), _p(d))
    assert rc == 0, L.ry_error()
    return o, d


def x86_radiance(L, holder, feat, orig, dir, n_samples, seed=SEED, sample_base=0, key=None, threads=8, segments=False):
    """The sums; with segments=True, (sums, the batch's segment total as mrt_rays_info.segments counts it)."""
    o, d = np.ascontiguousarray(orig, f32), np.ascontiguousarray(dir, f32)
    out = np.zeros_like(o)
    k = None if key is None else np.ascontiguousarray(key, np.uint32)
    seg = C.c_uint64(0)
    rc = L.ry_radiance(*_ptrs(holder), feat, seed, sample_base, n_samples, o.size // 3, _p(o), _p(d), None if k is None else _p(k, C.c_uint32),
                       threads, _p(out), C.byref(seg) if segments else None)
    assert rc == 0, L.ry_error()
    return (out, int(seg.value)) if segments else out


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def _sized(desc, res=RES, spp=SPP):
    desc["frame"]["res"], desc["frame"]["ssaa"] = list(res), 1
    desc["frame"]["cam"]["aprt"] = 0
    desc["rt"]["sample"] = spp
    return desc


def frame_descs():
    """The four scenes whose camera rays must reproduce the frame, 50 x 37, aprt 0."""
    from micro_raytracer_amd import scenes
    env = scenes.env_scene(res=RES, sample=SPP, bounce=4, mapping="latlong", tex_res=(32, 16))
    env["scene"]["sky"]["rot"] = 0.21
    return {"cornell": _sized(scenes.cornell_box(bounce=6)), "lights": _sized(K.lights(0)), "primitives": _sized(K.primitives()), "env_vattr": _sized(env)}


@functools.lru_cache(maxsize=None)
def frame_case(name):
    """(render, holder) of a frame scene: one object per scene, shared and left unchanged."""
    return make_holder(frame_descs()[name])


WINDOWS = {"lights": (lambda: K.lights(0, WIN), (-80.0, -25.0)), "mirrors": (lambda: K.mirrors(2, 0.15, WIN), (-80.0, -25.0)),
           "primitives": (lambda: K.primitives(WIN), (-60.0, 30.0))}


@functools.lru_cache(maxsize=None)
def window_case(name):
    """(render, holder, orig, dir, float64 render, float32 render's image) of a 96 x 40 lat-long window from the scene's camera
    position: directions formed in float64 and rounded to float32 (cameras.equirect), the float64 core on those very rays."""
    from micro_raytracer_amd import cameras
    make, elev = WINDOWS[name]
    render, holder = make_holder(make())
    o, d = cameras.equirect(render.frame.cam.pos, WIN[0], WIN[1], elevation=elev)
    saved = R.camera_rays
    R.camera_rays = lambda rd, dtype=np.float64: (o.reshape(-1, 3).astype(dtype), d.reshape(-1, 3).astype(dtype), (WIN[1], WIN[0]))
    try:
        ref = R.render_image(render, np.float64)
        img32 = R.render_image(render, np.float32)["img"]
    finally:
        R.camera_rays = saved
    return render, holder, o, d, ref, img32
