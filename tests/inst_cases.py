"""TEST INFRASTRUCTURE for tests/test_instantiation_census.py: one recipe per compiled instantiation of the path-tracing kernel.

The table of instantiations comes from the library (_lib.selftest_instantiations: the MRT_SHAPES_* lists of csrc/mrt_megakernel.h,
expanded).  recipe(threads, scene_in_lds, feat) names the smallest scene -- built from the feature bits -- and the environment
switches under which plan_launch sends that scene to exactly that row.  Rows that share a scene are siblings: they must give the
same accumulator bits.  UNREACHABLE lists the rows no scene description reaches, with the rule that keeps scenes away and the row
the natural recipe lands on instead; ABI_ONLY says how a caller of the C ABI still selects them."""
import contextlib
import ctypes as C
import os
from collections import namedtuple

import numpy as np

from micro_raytracer_amd import _abi, _lib, scenes
from micro_raytracer_amd._abi import F_ALL, F_BOX, F_BVH, F_COLD, F_DEEP, F_ENV, F_IDENT, F_LIGHTS, F_MAPS, F_NOSTASH, F_TRI, F_VATTR

FN = F_ALL & ~F_TRI
SCENE_BITS = F_ALL | F_BVH | F_VATTR | F_ENV

# Frame and sampling of every census run: 44 x 28 supersampled pixels = 5.5 x 3.5 wave tiles (a 1024-thread workgroup of 4 x 4
# tiles has wavefronts without a pixel and wavefronts with half of them); 40 samples = two whole 16-sample chunks and a partial one
RES, SSAA, BOUNCE, SEED = (22, 14), 2, 6, 20261018
SPP, SPP_LIST = 40, 32
KNOBS = ("MRT_BLOCK_THREADS", "MRT_SCENE_IN_L2", "MRT_COLD", "MRT_DEEP_NODES")
DEEP_NODES = "40"

# A scene of the census: the feature bits it is built from, whether every instance is untransformed (the F_IDENT builds), what
# pads it until only a 1024-thread workgroup without the lane stash fits (None | "tex" | "crowd" | "mesh"), and whether its
# holder carries a texture that no material references (texels without F_MAPS: the C ABI only)
Scene = namedtuple("Scene", "bits ident pad unref")
Recipe = namedtuple("Recipe", "scene env")

# The smallest pads under which plan_launch picks the F_NOSTASH shape, found with plan_launch (find_pad below; the census test
# holds that the size below lands elsewhere): texture columns of the 64-row padding texture, spheres of the crowd, triangles
PAD = {
    Scene(FN, False, "tex", False): 692, Scene(F_ALL, False, "tex", False): 620,
    Scene(F_BVH, False, "crowd", False): 1432, Scene(F_LIGHTS | F_BVH, False, "crowd", False): 1432,
    Scene(FN | F_BVH, False, "tex", False): 680, Scene(F_ALL | F_BVH, False, "tex", False): 607,
    Scene(F_ALL | F_VATTR, False, "mesh", False): 1529, Scene(F_ALL | F_BVH | F_VATTR, False, "mesh", False): 1502,
    Scene(F_ALL | F_VATTR | F_ENV, False, "mesh", False): 1529, Scene(F_ALL | F_BVH | F_VATTR | F_ENV, False, "mesh", False): 1502,
}


def rows():
    return _lib.selftest_instantiations()


def small_pick(feat):
    """The two instance-BVH feature sets without box, triangle or map code."""
    return bool(feat & F_BVH) and (feat & (F_BOX | F_TRI | F_MAPS | F_VATTR)) == 0


def scene_for(feat):
    """The scene whose features are exactly the row's bits."""
    pad = None
    if feat & F_NOSTASH:
        pad = "crowd" if small_pick(feat) else ("mesh" if feat & F_VATTR else "tex")
    return Scene(feat & SCENE_BITS, bool(feat & F_IDENT), pad, False)


def switches_for(threads, scene_in_lds, feat):
    if not scene_in_lds:
        return {"MRT_SCENE_IN_L2": "1"}
    env = {"MRT_DEEP_NODES": DEEP_NODES} if feat & F_DEEP else {"MRT_COLD": "1" if feat & F_COLD else "0"}
    if not feat & F_NOSTASH:                       # (a forced shape never takes the marker: plan_launch has to choose it)
        env["MRT_BLOCK_THREADS"] = str(threads)
    return env


def recipe(threads, scene_in_lds, feat):
    return Recipe(scene_for(feat), switches_for(threads, scene_in_lds, feat))


# ---- rows no scene description reaches ------------------------------------------------------------------------------------------
# row -> (the rule, where the natural recipe lands).  The warm level needs something to leave out of LDS: texels
# (staging_level: has_warm = lds_words_warm < lds_words) or a mesh walk.  A sphere / plane crowd has no mesh, and the packer only
# emits texels for textures of the scene's texture table, which the loader fills from the materials' maps -- and a material map
# sets F_MAPS, with which pt_instantiation's `pick` is the big feature set.  So MRT_COLD=1 changes nothing for such a crowd.
_WARM_RULE = ("staging_level: warm_ok needs has_warm (texels or a mesh walk); a scene description only has texels through a material "
              "map, and F_MAPS makes pt_instantiation pick the big set")
UNREACHABLE = {(t, True, f | F_BVH | F_COLD): (_WARM_RULE, (t, True, f | F_BVH)) for t in (256, 512, 1024) for f in (0, F_LIGHTS)}


def abi_recipe(threads, scene_in_lds, feat):
    """How the C ABI still selects an UNREACHABLE row: the crowd with one texture in mrt_scene.textures that no material uses."""
    assert (threads, scene_in_lds, feat) in UNREACHABLE
    return Recipe(scene_for(feat)._replace(unref=True), switches_for(threads, scene_in_lds, feat))


# ---- the scenes -----------------------------------------------------------------------------------------------------------------
_IDENT_DIR = [-0.0, -0.0, -1, -0.0]          # the loader's default: one identity, zeros of one sign (mrt_pack.cpp all_ident)
_TILT = [0.25, 0.6, 1, -0.2]


def _k255(a):
    return (np.asarray(a, np.float32) / np.float32(255)).astype(np.float32)


def _checker(w, h):
    y, x = np.mgrid[0:h, 0:w]
    k = np.where((x // 2 + y // 2) % 2 == 0, 230, 60)
    return {"w": int(w), "h": int(h), "dat": _k255(np.stack([k, k * 0 + 200, 255 - k], -1).reshape(-1, 3))}


def _crowd(n):
    """n small spheres on a lattice behind and above the other objects."""
    i = np.arange(n)
    p = np.stack([-1.4 + 0.19 * (i % 16), 0.15 + 0.21 * ((i // 16) % 16), -0.3 + 0.17 * (i // 256) + 0.05 * (i % 3)], 1)
    return [[[float(c) for c in q], _IDENT_DIR] for q in p.astype(np.float32)]


def describe(scene, pad_size=None):
    """The render description (the loader's dict) of a census scene."""
    bits, ident = scene.bits, scene.ident
    n_pad = pad_size if pad_size is not None else (PAD[scene] if scene.pad else None)
    tilt = {} if ident else {"dir": _TILT}
    floor = {"rough": 1, "albedo": [0.8, 0.8, 0.75]}
    if bits & F_MAPS:
        floor["tex"] = _checker(n_pad, 64) if scene.pad == "tex" else _checker(8, 8)
    rend = [
        {"type": "plane", "n": [0, 0, 1], "pos": [0, 0, -0.4], "mat": floor},
        {"type": "plane", "n": [0, -1, 0], "pos": [0, 1.3, 0], "mat": {"albedo": [0.7, 0.3, 0.25], "rough": 0.6}, **({} if ident else {"dir": [0.1, 0.15, -1, 0.2]})},
        {"type": "sphere", "r": 0.25, "pos": [-0.45, 0.1, -0.1], "mat": {"glass": 0.3, "opacity": 0.2}},
        {"type": "sphere", "r": 0.2, "pos": [0.5, 0.3, 0.0], "mat": {"metal": 1, "rough": 0.2, "albedo": [0.9, 0.8, 0.5]}},
        {"type": "sphere", "r": 0.1, "pos": [0.1, -0.2, 0.55], "mat": {"emit": 0.8, "albedo": [1.0, 0.9, 0.7]}},
    ]
    if bits & F_BOX:
        rend.append({"type": "box", "sizes": [0.35, 0.3, 0.4], "pos": [0.1, 0.6, -0.2], "mat": {"albedo": [0.4, 0.6, 0.9], "rough": 0.4}, **tilt})
    if bits & F_TRI:
        tri = {"type": "triangle", "vtx": [[0.6, 0.3, -0.25], [0.1, 0.35, 0.55], [-0.4, 0.25, -0.2]], "pos": [0.0, 0.4, 0.2],
               "mat": {"albedo": [1.0, 0.8, 0.4], "rough": 0.5}}
        if bits & F_VATTR:
            tri["vn"] = [[[0.1, -1.0, 0.2], [0.0, -2.0, -0.3], [-0.2, -0.5, 0.1]]]
            tri["uv"] = [[[0.0, 0.0], [1.5, 0.2], [0.3, 2.0]]]
            tri["mat"]["tex"] = _checker(5, 3)
        rend.append(tri)
        if (bits & F_ALL) == F_ALL:
            # the full set: a mesh too, so that the scene has a walk area at the warm level and a deep level
            tris = scenes.big_mesh(n_pad) if scene.pad == "mesh" else scenes.icosphere(1, 0.22, (1.0, 1.0, 1.3))
            mesh = {"type": "mesh", "mesh": np.asarray(tris, np.float32), "pos": [-0.25, -0.25, 0.3], "mat": {"albedo": [0.75, 1.0, 0.75], "rough": 0.8}, **tilt}
            if bits & F_VATTR:
                uv, vn = scenes.smooth_attrs(tris)
                mesh["uv"], mesh["vn"] = uv, vn
                mesh["mat"]["tex"] = _checker(6, 4)
            rend.append(mesh)
    if bits & F_BVH:
        rend.append({"type": "sphere", "r": 0.07, "mat": {"albedo": [0.9, 0.9, 0.3], "rough": 0.7}, "inst": _crowd(n_pad if scene.pad == "crowd" else 24)})
    light = []
    if bits & F_LIGHTS:
        light = [{"type": "point", "pos": [-0.8, -1.0, 0.9], "pwr": 0.4, "color": [1.0, 0.88, 0.75]},
                 {"type": "dir", "dir": [0.3, 0.5, -1.0], "pwr": 0.3, "color": [0.75, 0.8, 1.0]}]
    sky = {"color": [0.3, 0.4, 0.6], "pwr": 0.5}
    if bits & F_ENV:
        rng = np.random.default_rng(5)
        sky.update({"tex": {"w": 4, "h": 3, "dat": (6.0 * rng.uniform(0, 1, (12, 3)) ** 2).astype(np.float32)}, "map": "latlong", "rot": 0.3})
    return {"rt": {"sample": SPP, "bounce": BOUNCE, "loss": 0.1},
            "frame": {"res": list(RES), "ssaa": SSAA, "cam": {"pos": [0.1, -1.6, 0.35], "dir": [0.05, 0.1, 1, -0.1], "fov": 65, "gamma": 0.7, "exp": 0.5,
                                                               "aprt": 0.01, "foc": 1.5}},
            "scene": {"renderer": rend, "light": light, "sky": sky}}


def _add_unreferenced_texture(h):
    """One more entry in the holder's texture table, used by no material."""
    sc = h.desc.scene
    n = sc.n_textures
    texs = (_abi.Texture * (n + 1))()
    for i in range(n):
        texs[i].w, texs[i].h, texs[i].dat = sc.textures[i].w, sc.textures[i].h, sc.textures[i].dat
    arr = np.ascontiguousarray(_checker(4, 4)["dat"])
    texs[n].w, texs[n].h, texs[n].dat = 4, 4, arr.ctypes.data_as(C.POINTER(C.c_float))
    h.keep += [arr, texs]
    sc.textures, sc.n_textures = C.cast(texs, C.POINTER(_abi.Texture)), n + 1


_BUILT = {}


def build(scene, pad_size=None):
    """(render, holder) of a census scene; one object per scene, so that a Sampler keeps telling it from the others."""
    key = (scene, pad_size)
    if key not in _BUILT:
        from micro_raytracer_amd import scene as loader
        render = loader.load_render(describe(scene, pad_size))
        holder = holder_of(render, scene)
        if pad_size is not None:
            return render, holder
        _BUILT[key] = (render, holder)
    return _BUILT[key]


_build_desc = _abi.build_desc          # (a test may put holder_of in its place for a Sampler: keep the real one)


def holder_of(render, scene):
    h = _build_desc(render)
    if scene.unref:
        _add_unreferenced_texture(h)
    return h


@contextlib.contextmanager
def switches(env):
    """The library's launch knobs set to exactly env (the others unset), restored afterwards."""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def triple(d):
    """(block_threads, scene_in_lds, kernel_features) of a plan_launch or stats() dict."""
    in_lds = d["scene_in_lds"] != 0 if "scene_in_lds" in d else d["staging"] != "none"
    return int(d["block_threads"]), bool(in_lds), int(d["kernel_features"])


def plan(holder, env):
    with switches(env):
        return _lib.plan_launch(holder)


def find_pad(scene, target, lo, hi):
    """The smallest pad size in [lo, hi] at which plan_launch, under the target's switches, reports the target."""
    env = switches_for(*target)
    lands = lambda n: triple(plan(build(scene, n)[1], env))
    # (in the order of growing scenes: the stashed shapes of the whole-scene level, F_NOSTASH, then a colder level or L2)
    beyond = lambda n: (lambda t: not t[1] or bool(t[2] & (F_NOSTASH | F_COLD)))(lands(n))
    assert beyond(hi) and not beyond(lo), (scene, lands(lo), lands(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if beyond(mid) else (mid, hi)
    assert lands(hi) == tuple(target), (scene, hi, lands(hi))
    return hi


def census():
    """{scene: [(row, env), ...]} over every row a description reaches, {scene: [(row, env)]} of the ABI-only recipes."""
    by_scene, abi_only = {}, {}
    for row in rows():
        if row in UNREACHABLE:
            r = abi_recipe(*row)
            abi_only.setdefault(r.scene, []).append((row, r.env))
        else:
            r = recipe(*row)
            by_scene.setdefault(r.scene, []).append((row, r.env))
    return by_scene, abi_only


def witnesses(scene, targets):
    """Further launches of a scene whose bits must equal its rows': the scene read through L2, and for an F_IDENT scene the
    64-thread shape, which has no F_IDENT build (MRT_BLOCK_THREADS moves the scene to the plain one)."""
    have = {tuple(sorted(env.items())) for _, env in targets}
    out = [{"MRT_SCENE_IN_L2": "1"}] + ([{"MRT_COLD": "0", "MRT_BLOCK_THREADS": "64"}] if scene.ident else [])
    return [e for e in out if tuple(sorted(e.items())) not in have]


def name_of(scene):
    names = ((F_BOX, "box"), (F_TRI, "tri"), (F_MAPS, "maps"), (F_LIGHTS, "lights"), (F_BVH, "bvh"), (F_VATTR, "vattr"), (F_ENV, "env"))
    s = "+".join(n for b, n in names if scene.bits & b) or "plain"
    return s + ("-ident" if scene.ident else "") + (f"-pad_{scene.pad}" if scene.pad else "") + ("-unref" if scene.unref else "")


def oracle_accums(oracle_mod, holder, threads=None):
    """{32: accumulator, 40: accumulator} of the oracle for a census scene: one run, read after 32 and after 40 samples."""
    o = oracle_mod.Oracle(holder, seed=SEED)
    out = {}
    o.execute(SPP_LIST, threads=threads)
    out[SPP_LIST] = o.accum()[0].copy()
    o.execute(SPP - SPP_LIST, threads=threads)
    out[SPP] = o.accum()[0].copy()
    o.close()
    for a in out.values():
        a.setflags(write=False)
    return out
