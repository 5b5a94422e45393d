"""ctypes mirror of include/mrt.h (the C-ABI boundary) and the flattening of a loaded
render description into the POD `mrt_render_desc`.

The same descriptor feeds libmrt_hip.so (product) and, in tests only, the CPU oracle.
Reference types mirrored: rt::Render and everything under it, /root/reference src/rt.rs:10-190.
"""
import ctypes as C

import numpy as np

ABI_VERSION = 3

KIND_SPHERE, KIND_PLANE, KIND_BOX, KIND_TRIANGLE, KIND_MESH = range(5)
LIGHT_POINT, LIGHT_DIR = 0, 1
KIND_IDS = {"sphere": KIND_SPHERE, "plane": KIND_PLANE, "box": KIND_BOX, "triangle": KIND_TRIANGLE, "mesh": KIND_MESH}

MRT_OK, MRT_ERR_ARG, MRT_ERR_SCENE, MRT_ERR_DEVICE, MRT_ERR_LIMIT, MRT_ERR_STATE = 0, -1, -2, -3, -4, -5
TRACE_WORDS = 9          # MRT_TRACE_WORDS: words per ray of mrt_selftest_trace
FLAG_COUNT_SEGMENTS, FLAG_NO_EVENT_TIMING, FLAG_DEFER, FLAG_NO_LOOKAHEAD = 1, 2, 4, 8
# the F_* bits of csrc/mrt_scene.h, as mrt_stats.kernel_features and mrt_plan.kernel_features report them: scene features
# (F_ALL = the first four), the instance BVH, the launch-shape markers, then F_IDENT, F_VATTR, F_ENV
# (_lib.selftest_instantiations() lists the combinations that exist as kernels: mrt_selftest_instantiations)
F_BOX, F_TRI, F_MAPS, F_LIGHTS, F_ALL, F_BVH = 1, 2, 4, 8, 15, 16
F_NOSTASH, F_COLD, F_DEEP, F_IDENT, F_VATTR, F_ENV = 32, 64, 128, 256, 512, 1024


class Camera(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("dir", C.c_float * 4), ("fov", C.c_float), ("gamma", C.c_float),
                ("exp", C.c_float), ("aprt", C.c_float), ("foc", C.c_float)]


class Frame(C.Structure):
    _fields_ = [("res_w", C.c_uint16), ("res_h", C.c_uint16), ("ssaa", C.c_float), ("cam", Camera)]


class Rt(C.Structure):
    _fields_ = [("bounce", C.c_uint32), ("sample", C.c_uint32), ("loss", C.c_float)]


class Texture(C.Structure):
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("dat", C.POINTER(C.c_float))]


class Material(C.Structure):
    _fields_ = [("albedo", C.c_float * 3), ("rough", C.c_float), ("metal", C.c_float), ("glass", C.c_float),
                ("opacity", C.c_float), ("emit", C.c_float), ("tex", C.c_int32), ("rmap", C.c_int32),
                ("mmap", C.c_int32), ("gmap", C.c_int32), ("omap", C.c_int32), ("emap", C.c_int32)]


class Instance(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("dir", C.c_float * 4)]


class Renderer(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("param", C.c_float * 9), ("tris", C.POINTER(C.c_float)),
                ("n_tris", C.c_uint32), ("mat", Material), ("inst", C.POINTER(Instance)), ("n_inst", C.c_uint32)]


class Light(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("v", C.c_float * 3), ("pwr", C.c_float), ("color", C.c_float * 3)]


class Sky(C.Structure):
    _fields_ = [("color", C.c_float * 3), ("pwr", C.c_float)]


class Scene(C.Structure):
    _fields_ = [("renderer", C.POINTER(Renderer)), ("n_renderer", C.c_uint32), ("light", C.POINTER(Light)),
                ("n_light", C.c_uint32), ("sky", Sky), ("textures", C.POINTER(Texture)), ("n_textures", C.c_uint32)]


class RenderDesc(C.Structure):
    _fields_ = [("rt", Rt), ("frame", Frame), ("scene", Scene)]


class Opts(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("seed", C.c_uint64), ("device", C.c_int32),
                ("shard_index", C.c_uint32), ("shard_count", C.c_uint32), ("shard_rows", C.c_uint32),
                ("n_devices", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("gather_ms", C.c_double), ("samples", C.c_uint64),
                ("segments", C.c_uint64), ("launches", C.c_uint32), ("lds_bytes", C.c_uint32),
                ("block_threads", C.c_uint32), ("scene_bytes", C.c_uint32), ("k_split", C.c_uint32), ("deferred", C.c_uint32), ("img_ms", C.c_double),
                ("reduce_ms", C.c_double), ("kernel_features", C.c_uint32), ("scene_in_lds", C.c_uint32)]


RAYS_DEVICE = 1          # MRT_RAYS_DEVICE: the rays, keys and sums of mrt_radiance are device pointers
AOV_RAYS_DEVICE = 1      # MRT_AOV_RAYS_DEVICE: the rays of mrt_aov_rays are device pointers
AOV_WRAP_X = 2           # MRT_AOV_WRAP_X: their grid is periodic in x


class Rays(C.Structure):
    _fields_ = [("n", C.c_size_t), ("orig", C.c_void_p), ("dir", C.c_void_p), ("key", C.c_void_p),
                ("sample_base", C.c_uint32), ("n_samples", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class RaysInfo(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("samples", C.c_uint64), ("segments", C.c_uint64), ("kernel_features", C.c_uint32),
                ("scene_in_lds", C.c_uint32), ("lds_bytes", C.c_uint32), ("reserved", C.c_uint32)]


GATHER_SPHERE, GATHER_HEMI_COS = 0, 1        # MRT_GATHER_*: mrt_gather_desc.dist
GATHER_MEAN, GATHER_SH9 = 0, 1               # ... and .out
GATHER_OUTS = {"mean": GATHER_MEAN, "sh9": GATHER_SH9}


class Gather(C.Structure):
    """mrt_gather_desc: the points of mrt_gather / mrt_gather_rays, their direction set and the reduction"""
    _fields_ = [("n", C.c_size_t), ("pos", C.c_void_p), ("normal", C.c_void_p), ("n_dirs", C.c_uint32), ("sample_base", C.c_uint32),
                ("n_samples", C.c_uint32), ("dist", C.c_uint32), ("out", C.c_uint32), ("key_base", C.c_uint32), ("offset", C.c_float),
                ("batch_points", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class GatherInfo(C.Structure):
    _fields_ = [("gen_ms", C.c_double), ("kernel_ms", C.c_double), ("reduce_ms", C.c_double), ("rays", C.c_uint64), ("samples", C.c_uint64),
                ("segments", C.c_uint64), ("batches", C.c_uint32), ("kernel_features", C.c_uint32), ("scene_in_lds", C.c_uint32),
                ("lds_bytes", C.c_uint32)]


class Plan(C.Structure):
    _fields_ = [("staging", C.c_uint32), ("block_threads", C.c_uint32), ("lds_bytes", C.c_uint32), ("staged_bytes", C.c_uint32),
                ("scene_bytes", C.c_uint32), ("kernel_features", C.c_uint32), ("tbvh_nodes", C.c_uint32), ("tbvh_hot_nodes", C.c_uint32),
                ("small_plain_grid", C.c_uint32), ("walk_cap", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class TriAttrs(C.Structure):
    _fields_ = [("uv", C.POINTER(C.c_float)), ("vn", C.POINTER(C.c_float))]


ENV_SPHERE, ENV_LATLONG = 0, 1
ENV_MAPPINGS = {"sphere": ENV_SPHERE, "latlong": ENV_LATLONG}


FILTER_NEAREST, FILTER_BILINEAR = 0, 1
FILTERS = {"nearest": FILTER_NEAREST, "bilinear": FILTER_BILINEAR}


class Env(C.Structure):
    _fields_ = [("tex", Texture), ("mapping", C.c_uint32), ("rot", C.c_float), ("filter", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class DescExt(C.Structure):
    _fields_ = [("n_renderer", C.c_uint32), ("attrs", C.POINTER(TriAttrs)), ("env", C.POINTER(Env)), ("reserved", C.c_uint32 * 2)]

    @property
    def tex_filter(self):
        """MRT_FILTER_* of the scene's material textures: word 0 of `reserved` (word 1 must stay 0)."""
        return int(self.reserved[0])

    @tex_filter.setter
    def tex_filter(self, value):
        self.reserved[0] = int(value)


class Adapt(C.Structure):
    _fields_ = [("min_samples", C.c_uint32), ("max_samples", C.c_uint32), ("step", C.c_uint32), ("threshold", C.c_float),
                ("reserved", C.c_uint32 * 4)]


class AdaptInfo(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("rounds", C.c_uint32), ("launches", C.c_uint32), ("tiles", C.c_uint32),
                ("tiles_converged", C.c_uint32), ("min_count", C.c_uint32), ("max_count", C.c_uint32), ("kernel_ms", C.c_double)]


class RaysAdapt(C.Structure):
    """mrt_rays_adapt: the rays of mrt_radiance_adaptive (one per supersampled pixel) and its rule"""
    _fields_ = [("orig", C.c_void_p), ("dir", C.c_void_p), ("rule", Adapt), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class DenoiseOpts(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float),
                ("mode", C.c_uint32), ("sigma_var", C.c_float), ("firefly", C.c_float), ("reserved", C.c_uint32 * 1)]


class DenoiseInfo(C.Structure):
    _fields_ = [("aov_ms", C.c_double), ("filter_ms", C.c_double), ("passes", C.c_uint32), ("aov_cached", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


# defaults of mrt_denoise_opts (include/mrt.h MRT_DENOISE_*)
DENOISE_PASSES, DENOISE_SIGMA_COLOR, DENOISE_SIGMA_NORMAL, DENOISE_SIGMA_PLANE = 5, 0.5, 0.25, 0.05


# modes of mrt_denoise_opts (MRT_DN_*) and the variance mode's defaults (MRT_DN_SIGMA_VAR, MRT_DN_FIREFLY), which a 0 word selects
DN_MODES = {"atrous": 0, "variance": 1}
DN_SIGMA_VAR, DN_FIREFLY = 4.5, 1.0


def denoise_opts(passes=DENOISE_PASSES, sigma_color=None, sigma_normal=None, sigma_plane=None, mode="atrous", sigma_var=None,
                 firefly=None) -> DenoiseOpts:
    """mrt_denoise_opts; a sigma of None takes its default, float("inf") switches that term off.  mode "variance" (an adaptive
    render's half buffer drives the colour term): sigma_var / firefly of None are the struct's 0 word, the library's default;
    firefly float("inf") switches the firefly clamp off."""
    if mode not in DN_MODES:
        raise ValueError(f"denoise mode `{mode}`: expected one of {sorted(DN_MODES)}")
    o = DenoiseOpts()
    o.passes = int(passes)
    o.sigma_color = DENOISE_SIGMA_COLOR if sigma_color is None else float(sigma_color)
    o.sigma_normal = DENOISE_SIGMA_NORMAL if sigma_normal is None else float(sigma_normal)
    o.sigma_plane = DENOISE_SIGMA_PLANE if sigma_plane is None else float(sigma_plane)
    o.mode = DN_MODES[mode]
    o.sigma_var = 0.0 if sigma_var is None else float(sigma_var)
    o.firefly = 0.0 if firefly is None else float(firefly)
    return o


# resize filters of mrt_img_hdr (MRT_RESIZE_*)
RESIZE_LANCZOS3, RESIZE_BOX = 0, 1
RESIZE_FILTERS = {"lanczos3": RESIZE_LANCZOS3, "box": RESIZE_BOX}


class HdrOpts(C.Structure):
    _fields_ = [("filter", C.c_uint32), ("reserved0", C.c_uint32), ("denoise", C.POINTER(DenoiseOpts)), ("reserved", C.c_uint32 * 4)]


class HdrInfo(C.Structure):
    _fields_ = [("resize_ms", C.c_double), ("dn", DenoiseInfo), ("reserved", C.c_uint32 * 2)]


def as_dict(s) -> dict:
    """A ctypes struct's fields by name, without its `reserved` words"""
    return {k: getattr(s, k) for k, _ in s._fields_ if k != "reserved"}


STAGING = ("all", "warm", "deep", "none")
MAP_SLOTS = ("tex", "rmap", "mmap", "gmap", "omap", "emap")


def _f3(dst, src):
    for i in range(3):
        dst[i] = float(np.float32(src[i]))


def _f4(dst, src):
    for i in range(4):
        dst[i] = float(np.float32(src[i]))


def _filter_id(name, what):
    if name not in FILTERS:
        raise ValueError(f"{what} `{name}`: expected one of {sorted(FILTERS)}")
    return FILTERS[name]


class DescHolder:
    """Owns a RenderDesc together with every array it points into."""

    def __init__(self):
        self.desc = RenderDesc()
        self.ext = None        # mrt_desc_ext when a triangle / mesh renderer carries per-corner uv / vn, the sky a texture or the
                               # material textures a filter, else None
        self.keep = []

    def ptr(self):
        return C.byref(self.desc)

    def ext_ptr(self):
        """The mrt_desc_ext argument of mrt_create_ext / mrt_plan_launch_ext (None: NULL)."""
        return None if self.ext is None else C.cast(C.byref(self.ext), C.c_void_p)


def build_desc(render) -> DescHolder:
    """Flatten a loaded render (micro_raytracer_amd.scene.Render) into mrt_render_desc.

    Renderer order and per-renderer instance order are preserved: ties in the reference's
    closest-hit `min_by` resolve to the first candidate (src/rt.rs:872).
    """
    h = DescHolder()
    d = h.desc
    d.rt.bounce = int(render.rt.bounce)
    d.rt.sample = int(render.rt.sample)
    d.rt.loss = float(np.float32(render.rt.loss))
    fr = render.frame
    d.frame.res_w, d.frame.res_h = int(fr.res[0]), int(fr.res[1])
    d.frame.ssaa = float(np.float32(fr.ssaa))
    cam = fr.cam
    _f3(d.frame.cam.pos, cam.pos)
    _f4(d.frame.cam.dir, cam.dir)
    for k in ("fov", "gamma", "exp", "aprt", "foc"):
        setattr(d.frame.cam, k, float(np.float32(getattr(cam, k))))

    sc = render.scene
    # textures: de-duplicated by object identity
    tex_index = {}
    tex_list = []

    def tex_id(t):
        if t is None:
            return -1
        key = id(t)
        if key not in tex_index:
            tex_index[key] = len(tex_list)
            tex_list.append(t)
        return tex_index[key]

    rends = (Renderer * max(1, len(sc.renderer)))()
    attrs = (TriAttrs * max(1, len(sc.renderer)))()
    any_attr = False
    for i, r in enumerate(sc.renderer):
        o = rends[i]
        n_tris = 1 if r.kind == "triangle" else (np.asarray(r.mesh).reshape(-1, 9).shape[0] if r.kind == "mesh" else 0)
        for key, width in (("uv", 2), ("vn", 3)):
            a = getattr(r, key, None)
            if a is None:
                continue
            a = np.ascontiguousarray(np.asarray(a, np.float32))
            if n_tris and a.size != n_tris * 3 * width:
                raise ValueError(f"renderer {i}: {key} has {a.size} floats, {n_tris} triangle(s) need {n_tris * 3 * width}")
            h.keep.append(a)
            setattr(attrs[i], key, a.ctypes.data_as(C.POINTER(C.c_float)))
            any_attr = True
        o.kind = KIND_IDS[r.kind]
        params = np.zeros(9, np.float32)
        if r.kind == "sphere":
            params[0] = r.r
        elif r.kind == "plane":
            params[:3] = r.n
        elif r.kind == "box":
            params[:3] = r.sizes
        elif r.kind == "triangle":
            params[:] = np.asarray(r.vtx, np.float32).reshape(9)
        for k in range(9):
            o.param[k] = float(params[k])
        if r.kind == "mesh":
            tris = np.ascontiguousarray(np.asarray(r.mesh, np.float32).reshape(-1, 9))
            h.keep.append(tris)
            o.tris = tris.ctypes.data_as(C.POINTER(C.c_float))
            o.n_tris = tris.shape[0]
        m = r.mat
        _f3(o.mat.albedo, m.albedo)
        for k in ("rough", "metal", "glass", "opacity", "emit"):
            setattr(o.mat, k, float(np.float32(getattr(m, k))))
        for k in MAP_SLOTS:
            setattr(o.mat, k, tex_id(getattr(m, k)))
        insts = (Instance * max(1, len(r.inst)))()
        for j, (pos, direc) in enumerate(r.inst):
            _f3(insts[j].pos, pos)
            _f4(insts[j].dir, direc)
        h.keep.append(insts)
        o.inst = C.cast(insts, C.POINTER(Instance))
        o.n_inst = len(r.inst)
    h.keep.append(rends)
    d.scene.renderer = C.cast(rends, C.POINTER(Renderer))
    d.scene.n_renderer = len(sc.renderer)
    if any_attr:
        h.keep.append(attrs)
        h.ext = DescExt()
        h.ext.n_renderer = len(sc.renderer)
        h.ext.attrs = C.cast(attrs, C.POINTER(TriAttrs))

    lights = (Light * max(1, len(sc.light)))()
    for i, l in enumerate(sc.light):
        lights[i].kind = LIGHT_POINT if l.kind == "point" else LIGHT_DIR
        _f3(lights[i].v, l.v)
        lights[i].pwr = float(np.float32(l.pwr))
        _f3(lights[i].color, l.color)
    h.keep.append(lights)
    d.scene.light = C.cast(lights, C.POINTER(Light))
    d.scene.n_light = len(sc.light)

    _f3(d.scene.sky.color, sc.sky.color)
    d.scene.sky.pwr = float(np.float32(sc.sky.pwr))
    sky_tex = getattr(sc.sky, "tex", None)
    if sky_tex is not None:               # the environment texture (mrt_env)
        mapping = getattr(sc.sky, "mapping", "sphere")
        if mapping not in ENV_MAPPINGS:
            raise ValueError(f"sky map `{mapping}`: expected one of {sorted(ENV_MAPPINGS)}")
        env = Env()
        env.tex.w, env.tex.h = int(sky_tex.w), int(sky_tex.h)
        if sky_tex.dat is not None:
            arr = np.ascontiguousarray(np.asarray(sky_tex.dat, np.float32).reshape(-1, 3))
            if arr.shape[0] != env.tex.w * env.tex.h:
                raise ValueError(f"sky tex: {arr.shape[0]} texels for {env.tex.w} x {env.tex.h}")
            h.keep.append(arr)
            env.tex.dat = arr.ctypes.data_as(C.POINTER(C.c_float))
        env.mapping = ENV_MAPPINGS[mapping]
        env.rot = float(np.float32(getattr(sc.sky, "rot", 0.0)))
        env.filter = _filter_id(getattr(sc.sky, "filter", "nearest"), "sky filter")
        h.keep.append(env)
        if h.ext is None:
            h.ext = DescExt()
        h.ext.env = C.pointer(env)

    texs = (Texture * max(1, len(tex_list)))()
    for i, t in enumerate(tex_list):
        texs[i].w, texs[i].h = int(t.w), int(t.h)
        if t.dat is not None:
            arr = np.ascontiguousarray(np.asarray(t.dat, np.float32).reshape(-1, 3))
            h.keep.append(arr)
            texs[i].dat = arr.ctypes.data_as(C.POINTER(C.c_float))
    h.keep.append(texs)
    d.scene.textures = C.cast(texs, C.POINTER(Texture))
    d.scene.n_textures = len(tex_list)
    # the filter of the material textures: carried by the ext only when some material has a texture for it to act on
    tex_filter = _filter_id(getattr(sc, "tex_filter", "nearest"), "scene filter")
    if tex_filter != FILTER_NEAREST and tex_list:
        if h.ext is None:
            h.ext = DescExt()
        h.ext.tex_filter = tex_filter
    return h
