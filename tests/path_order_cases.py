"""TEST INFRASTRUCTURE: the frames of tests/test_path_order_host.py and tests/test_gpu_path_order.py, and of the script that
records their pins (tests/golden/make_path_order_pins.py).

Kernels without lights and maps decide a path's end before its scatter and take one pair of draws for scattering and
regenerated lanes (csrc/mrt_trace.h render_pixel).  That order must change no bit, so every frame here is pinned as
uint32 words recorded from the commit BEFORE the reorder.  The frames are the smallest that reach each seam of the loop."""
import copy
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 11


def coin_scene(aprt=0.0):
    """24x16, 48 spp, untransformed planes and spheres (the F_IDENT kernel): every coin of the loop open somewhere.
    opacity 0 and 0.5 with glass 0.5 (refraction, and total internal reflection: the second scatter pass); emit 0.3 on a sphere
    and on a plane, emit 1 (the p == 1 rule); metal 0, 0.5, 1; rough 0 and 1."""
    cam = {"exp": 0.75, "fov": 70, "gamma": 0.5, "pos": [0.05, -1.2, 0.3]}
    if aprt:
        cam.update({"aprt": float(aprt), "foc": 1.0})
    return {
        "rt": {"sample": 48, "bounce": 6},
        "frame": {"res": [24, 16], "ssaa": 1, "cam": cam},
        "scene": {"renderer": [
            {"type": "plane", "n": [0, -1, 0], "pos": [0, 1, 0], "mat": {"rough": 1, "emit": 0.3, "albedo": "#ffe0a0"}},
            {"type": "plane", "n": [1, 0, 0], "pos": [-1, 0, 0], "mat": {"albedo": "#ff0000", "rough": 1}},
            {"type": "plane", "n": [-1, 0, 0], "pos": [1, 0, 0], "mat": {"albedo": "#00ff00", "rough": 0, "metal": 0.5}},
            {"type": "plane", "n": [0, 0, 1], "pos": [0, 0, -0.2], "mat": {"rough": 0}},
            {"type": "sphere", "r": 0.22, "pos": [-0.3, -0.3, 0.05], "mat": {"glass": 0.5, "opacity": 0}},
            {"type": "sphere", "r": 0.2, "pos": [0.25, -0.45, 0.0], "mat": {"glass": 0.5, "opacity": 0.5, "rough": 0}},
            {"type": "sphere", "r": 0.2, "pos": [0.55, 0.1, 0.0], "mat": {"metal": 1}},
            {"type": "sphere", "r": 0.18, "pos": [-0.55, 0.3, 0.0], "mat": {"albedo": "#80a0ff", "emit": 0.3, "rough": 1}},
            {"type": "sphere", "r": 0.15, "pos": [0.0, 0.5, 0.6], "mat": {"albedo": "#ffc177", "emit": 1.0}},
            {"type": "sphere", "r": 0.15, "pos": [0.1, 0.2, -0.05], "mat": {"metal": 0.5, "rough": 1}},
        ]},
    }


def sky_scene():
    """8x8, nothing in view: every lane misses, ends and regenerates in every iteration."""
    return {
        "rt": {"sample": 20, "bounce": 4},
        "frame": {"res": [8, 8], "ssaa": 1, "cam": {"exp": 0.75, "fov": 40, "gamma": 0.5, "pos": [0, -1.2, 0.1]}},
        "scene": {"renderer": [{"type": "sphere", "r": 0.1, "pos": [0, -5, 0]}],          # behind the camera
                  "sky": {"color": "#4080c0", "pwr": 0.5}},
    }


def closed_scene():
    """8x8 inside a closed room of six planes without an emitter: hardly a lane ends before the bounce cut (a rough scatter
    sends a few paths through a wall)."""
    walls = [([0, -1, 0], [0, 1, 0]), ([0, 1, 0], [0, -2, 0]), ([1, 0, 0], [-1, 0, 0]), ([-1, 0, 0], [1, 0, 0]),
             ([0, 0, -1], [0, 0, 1]), ([0, 0, 1], [0, 0, -0.5])]
    return {
        "rt": {"sample": 20, "bounce": 5},
        "frame": {"res": [8, 8], "ssaa": 1, "cam": {"exp": 0.75, "fov": 60, "gamma": 0.5, "pos": [0, -1.2, 0.1]}},
        # (the sky is never seen: its colour is what the reference folds a cut path from, so the frame is not black)
        "scene": {"renderer": [{"type": "plane", "n": n, "pos": p, "mat": {"rough": 1, "albedo": "#c0c0c0"}} for n, p in walls],
                  "sky": {"color": "#ffe0c0", "pwr": 0.5}},
    }


def lit_scene():
    """A kernel with lights (untouched text): the default scene's sphere and point light over a plane."""
    from micro_raytracer_amd import scenes
    d = scenes.default_scene(res=(16, 12), sample=12, bounce=4)
    d["scene"]["renderer"].append({"type": "plane", "n": [0, 0, 1], "pos": [0, 0, -0.5], "mat": {"rough": 1}})
    d["scene"]["sky"] = {"color": "#203040", "pwr": 0.5}
    return d


def maps_scene():
    """A kernel with maps (untouched text): a checker floor under a glass and an emitting sphere, no lights."""
    from micro_raytracer_amd import scenes
    return {
        "rt": {"sample": 12, "bounce": 4},
        "frame": {"res": [16, 12], "ssaa": 1, "cam": {"exp": 0.75, "fov": 60, "gamma": 0.5, "pos": [0, -1.2, 0.2]}},
        "scene": {"renderer": [
            {"type": "plane", "n": [0, 0, 1], "pos": [0, 0, -0.3], "mat": {"rough": 1, "tex": scenes.checker_texture(8, 8, 2)}},
            {"type": "sphere", "r": 0.25, "pos": [-0.3, 0, 0], "mat": {"glass": 0.3, "opacity": 0.2}},
            {"type": "sphere", "r": 0.2, "pos": [0.35, 0.2, 0], "mat": {"albedo": "#ffc177", "emit": 0.5}},
        ], "sky": {"color": "#ffffff", "pwr": 0.4}},
    }


def _cornell(bounce):
    from micro_raytracer_amd import scenes
    return scenes.cornell_box(res=(32, 32), sample=40, bounce=bounce)


def _cornell_pinhole():
    """The Cornell frame with aprt 0: every sample of a pixel starts on the pixel's one camera ray (mrt_camera_rays)."""
    d = _cornell(8)
    d["frame"]["cam"]["aprt"] = 0
    return d


def _box2():
    from micro_raytracer_amd import scenes
    return scenes.cornell_box2(res=(24, 24), ssaa=1, sample=24, bounce=16)


# name -> (scene description, first sample, number of samples, kernel_features the frame must run at scene-in-LDS, 256 threads)
# 40 spp crosses two chunk ends (16, 32) and stops unaligned; [7, +33) starts unaligned as well
FRAMES = {
    "cornell_40": (lambda: _cornell(8), 0, 40, 256),
    "cornell_7_33": (lambda: _cornell(8), 7, 33, 256),
    "cornell_b0": (lambda: _cornell(0), 0, 40, 256),          # the cut in the first hit's iteration
    "cornell_b1": (lambda: _cornell(1), 0, 40, 256),
    "cornell_a0": (_cornell_pinhole, 0, 40, 256),
    "coin_a0": (lambda: coin_scene(0.0), 0, 48, 256),
    "coin_a005": (lambda: coin_scene(0.05), 0, 48, 256),
    "box2": (_box2, 0, 24, 1),                                # F_BOX: a rotated box, so not an F_IDENT scene
    "sky": (sky_scene, 0, 20, 256),
    "closed": (closed_scene, 0, 20, 256),
    "lit": (lit_scene, 0, 12, 256 | 8),
    "maps": (maps_scene, 0, 12, 4),
}


def desc_of(name):
    return copy.deepcopy(FRAMES[name][0]())


def pin_path(kind, name):
    return os.path.join(GOLDEN, f"path_order_{kind}_{name}.npy")


def load_pin(kind, name):
    return np.load(pin_path(kind, name))


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
