"""Seeded random scenes (every primitive kind, random materials / maps / rotations / lights / cameras) through the
parity bars: the kernel's lane code on x86 against the oracle for many seeds, a few of them on the GPU.  ext_scene draws the
extension features of DESIGN.md §14-§16 too (corner normals and UVs, maps on triangles and meshes, the environment texture,
both filters); its accumulators and its first-hit AOVs (tests/test_oracle_aov.py) are held to the oracle."""
import os

import numpy as np
import pytest

from conftest import make_holder
from micro_raytracer_amd._abi import F_BVH


def random_scene(seed):
    from micro_raytracer_amd import scenes
    rng = np.random.default_rng(seed)
    u = lambda a, b, n=None: rng.uniform(a, b, n)
    def vec(a, b): return [float(x) for x in u(a, b, 3)]
    def quat(): return [float(x) for x in np.r_[u(-0.9, 0.9), rng.normal(size=3)]] if rng.random() < 0.4 else [0, 0, -1, 0]
    def smap(w, h): return {"w": w, "h": h, "dat": [[float(k) / 255] * 3 for k in rng.integers(0, 256, w * h)]}
    def cmap(w, h): return {"w": w, "h": h, "dat": [[float(c) / 255 for c in rng.integers(0, 256, 3)] for _ in range(w * h)]}
    def mat(textured_ok):
        m = {"albedo": [float(x) for x in u(0.1, 1.0, 3)], "rough": float(rng.choice([0, 0.3, 1])), "metal": float(rng.choice([0, 0, 0.7, 1])),
             "glass": float(rng.choice([0, 0.1, 0.8])), "opacity": float(rng.choice([1, 1, 0.5, 0])), "emit": float(rng.choice([0, 0, 0, 0.4, 1]))}
        if textured_ok and rng.random() < 0.4:
            for k in ("tex", "rmap", "mmap", "gmap", "omap", "emap"):
                if rng.random() < 0.35:
                    m[k] = cmap(int(rng.integers(1, 9)), int(rng.integers(1, 9))) if k == "tex" else smap(int(rng.integers(1, 6)), int(rng.integers(1, 6)))
        return m
    rend = []
    for _ in range(int(rng.integers(1, 9))):
        kind = rng.choice(["sphere", "plane", "box", "triangle", "mesh"], p=[0.3, 0.2, 0.25, 0.15, 0.1])
        o = {"type": str(kind), "mat": mat(kind in ("sphere", "plane", "box"))}
        if kind == "sphere": o["r"] = float(u(0.1, 0.6))
        elif kind == "plane": o["n"] = vec(-1, 1)
        elif kind == "box": o["sizes"] = [float(x) for x in u(0.1, 1.2, 3)]
        elif kind == "triangle": o["vtx"] = [vec(-0.8, 0.8) for _ in range(3)]
        else: o["mesh"] = [[[float(c) for c in v] for v in t] for t in scenes.icosphere(int(rng.integers(0, 2)), float(u(0.2, 0.5)))]
        if rng.random() < 0.3:
            o["inst"] = [[vec(-1.5, 1.5), quat()] for _ in range(int(rng.integers(1, 4)))]
        else:
            o["pos"] = vec(-1.2, 1.2)
            o["dir"] = quat()
        rend.append(o)
    lights = []
    for _ in range(int(rng.integers(0, 3))):
        lights.append({"type": "point", "pos": vec(-2, 2), "pwr": float(u(0.1, 0.8)), "color": [float(x) for x in u(0.3, 1, 3)]} if rng.random() < 0.6
                      else {"type": "dir", "dir": vec(-1, 1), "pwr": float(u(0.1, 0.8)), "color": [float(x) for x in u(0.3, 1, 3)]})
    return {
        "rt": {"sample": int(rng.integers(1, 5)), "bounce": int(rng.integers(0, 7)), "loss": float(u(0, 0.5))},
        "frame": {"res": [int(rng.integers(3, 29)), int(rng.integers(3, 21))], "ssaa": float(rng.choice([1, 1, 2, 1.5, 0.75])),
                  "cam": {"pos": vec(-0.5, 0.5)[:1] + [float(u(-3, -1.5))] + [float(u(-0.3, 0.6))], "dir": [float(u(-0.3, 0.3)), float(u(-0.3, 0.3)), 1.0, float(u(-0.3, 0.3))],
                          "fov": float(u(40, 90)), "gamma": float(u(0.4, 1.0)), "exp": float(u(0.1, 0.85)), "aprt": float(rng.choice([0.0, 0.001, 0.02])), "foc": float(u(0.5, 50))}},
        "scene": {"renderer": rend, "light": lights, "sky": {"color": [float(x) for x in u(0, 0.6, 3)], "pwr": float(u(0, 1))}},
    }


def crowd_scene(seed):
    """random_scene with 4-40 extra instances per non-plane renderer: enough to switch on the instance BVH."""
    d = random_scene(seed)
    rng = np.random.default_rng(seed + 77777)
    for o in d["scene"]["renderer"]:
        if o["type"] == "plane":
            continue
        base = o.pop("inst", None) or [[o.pop("pos", [0, 0, 0]), o.pop("dir", [0, 0, -1, 0])]]
        o.pop("pos", None); o.pop("dir", None)
        inst = list(base)
        for _ in range(int(rng.integers(4, 40))):
            q = [float(x) for x in np.r_[rng.uniform(-0.9, 0.9), rng.normal(size=3)]] if rng.random() < 0.3 else [0, 0, -1, 0]
            inst.append([[float(x) for x in rng.uniform(-3, 3, 3)], q])
        o["inst"] = inst
    d["frame"]["res"] = [int(rng.integers(6, 20)), int(rng.integers(6, 14))]
    return d


def ident_scene(seed):
    """random_scene with every instance untransformed, on a half-unit lattice, no maps; half of the cameras are axis-aligned
    pinholes on a lattice point: rays and shifted origins with zero components everywhere (the F_IDENT kernels, mrt_trace.h)."""
    d = random_scene(seed)
    rng = np.random.default_rng(seed + 4242)
    keep = []
    for o in d["scene"]["renderer"]:
        if o["type"] in ("mesh", "triangle"):
            continue                                      # (plain kernels only: planes, spheres, boxes)
        o.pop("dir", None)
        if "inst" in o:
            # (the loader's default dir, which the objects without `inst` get: one identity, zeros of one sign, so that the scene
            # takes the F_IDENT kernels -- mrt_pack.cpp all_ident; tests/edge_cases.py has the mixed signs)
            o["inst"] = [[[float(round(c * 2) / 2) for c in i[0]], [-0.0, -0.0, -1, -0.0]] for i in o["inst"]]
        elif "pos" in o:
            o["pos"] = [float(round(c * 2) / 2) for c in o["pos"]]
        o.get("mat", {}).pop("tex", None)
        for k in ("rmap", "mmap", "gmap", "omap", "emap"):
            o.get("mat", {}).pop(k, None)
        keep.append(o)
    d["scene"]["renderer"] = keep or [{"type": "sphere", "r": 0.5}]
    if rng.random() < 0.5:                                # camera on the lattice, looking straight down +y, pinhole
        cam = d["frame"]["cam"]
        cam["pos"] = [0.0, -2.0, 0.0]; cam["dir"] = [0, 0, 1, 0]; cam["aprt"] = 0.0
    return d


def _fuzz_mesh(rng, n):
    """n triangles (300-1500) of one of the kinds tests/mesh_probe.py draws, at the sizes that fill the triangle BVH: a lobed
    icosphere, a plain one, a soup of large triangles, small triangles with huge, duplicate and degenerate ones, vertices on
    a quarter-unit grid (on octree cell boundaries)."""
    from micro_raytracer_amd import scenes
    kind = int(rng.integers(0, 5))
    if kind == 0:
        t = scenes.bumpy_mesh(n, seed=int(rng.integers(0, 1000)))
    elif kind == 1:
        t = scenes.icosphere(3, float(rng.uniform(0.3, 0.6)), tuple(rng.uniform(0.6, 1.4, 3)))[:n]
    elif kind == 2:
        t = rng.uniform(-0.6, 0.6, (n, 3, 3))
    elif kind == 3:
        t = rng.uniform(-0.6, 0.6, (n, 1, 3)) + rng.uniform(-0.05, 0.05, (n, 3, 3))
        t[::17] = rng.uniform(-0.8, 0.8, t[::17].shape)
        t[3::29] = t[2::29][: len(t[3::29])]
        t[5::31, 1] = t[5::31, 0]
    else:
        t = rng.integers(-3, 4, (n, 3, 3)) / 4.0
    return [[[float(c) for c in v] for v in tri] for tri in np.asarray(t, np.float32)]


def mesh_fuzz_scene(seed):
    """random_scene's materials, lights and cameras around 1-3 meshes of 300-1500 triangles (the triangle-BVH walks: deep
    levels, full walk areas), some of them in rotated and translated instances, some glass or translucent; small frames."""
    d = random_scene(seed)
    rng = np.random.default_rng(seed + 31337)
    rend = [o for o in d["scene"]["renderer"] if o["type"] in ("plane", "sphere", "box")][:2]
    for _ in range(int(rng.integers(1, 4))):
        m = {"albedo": [float(x) for x in rng.uniform(0.2, 1.0, 3)], "rough": float(rng.choice([0, 0.3, 1])), "metal": float(rng.choice([0, 0.7])),
             "glass": float(rng.choice([0, 0.3, 0.9])), "opacity": float(rng.choice([1, 1, 0.5, 0.1])), "emit": float(rng.choice([0, 0, 0.5]))}
        o = {"type": "mesh", "mesh": _fuzz_mesh(rng, int(rng.integers(300, 1501))), "mat": m}
        if rng.random() < 0.5:
            o["inst"] = [[[float(x) for x in rng.uniform(-1, 1, 3)],
                          [float(x) for x in np.r_[rng.uniform(-0.9, 0.9), rng.normal(size=3)]] if rng.random() < 0.7 else [0, 0, -1, 0]]
                         for _ in range(int(rng.integers(1, 4)))]
        else:
            o["pos"] = [float(x) for x in rng.uniform(-0.8, 0.8, 3)]
            o["dir"] = [float(x) for x in np.r_[rng.uniform(-0.9, 0.9), rng.normal(size=3)]] if rng.random() < 0.5 else [0, 0, -1, 0]
        rend.append(o)
    d["scene"]["renderer"] = rend
    d["frame"]["res"] = [int(rng.integers(6, 17)), int(rng.integers(5, 12))]
    d["frame"]["ssaa"] = 1
    d["rt"]["sample"] = int(rng.integers(1, 3))
    return d


MAPS = ("tex", "rmap", "mmap", "gmap", "omap", "emap")


def _ext_attrs(rng, tris):
    """(vn, uv) for the triangles tris [n][3][3]; either may be None.  vn: the face normal per corner, scaled by 0.01 .. 20
    (unnormalised) and bent by up to half its length; about one triangle in five flipped against the face, about one corner
    in ten all-zero (a whole triangle of zeros now and then: the face-normal fall-back).  uv: -3 .. 3."""
    t = np.asarray(tris, np.float64)
    n = t.shape[0]
    vn = uv = None
    if rng.random() < 0.7:
        face = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        ln = np.linalg.norm(face, axis=1, keepdims=True)
        face = np.where(ln > 0, face / np.where(ln > 0, ln, 1.0), [0.0, 0.0, 1.0])
        vn = face[:, None, :] + rng.uniform(-0.5, 0.5, (n, 3, 3))
        vn *= np.exp(rng.uniform(np.log(0.01), np.log(20.0), (n, 3, 1)))
        vn[rng.random(n) < 0.2] *= -1.0
        vn[rng.random((n, 3)) < 0.1] = 0.0
        vn[rng.random(n) < 0.03] = 0.0
    if rng.random() < 0.7:
        uv = rng.uniform(-3.0, 3.0, (n, 3, 2))
    as_list = lambda a: None if a is None else np.asarray(a, np.float32).astype(float).tolist()
    return as_list(vn), as_list(uv)


def _ext_map(rng, key):
    """A material map of 1..8 x 1..8 texels: colours for `tex`, equal channels for the scalar maps; k/255 values (the packer's
    RGB8 layout) or, for the maps that are not coins, any f32 in [0, 1]."""
    w, h = int(rng.integers(1, 9)), int(rng.integers(1, 9))
    if key in ("omap", "emap") or rng.random() < 0.5:
        v = rng.integers(0, 256, (w * h, 3)) / 255.0
    else:
        v = rng.uniform(0.0, 1.0, (w * h, 3))
    if key != "tex":
        v = np.repeat(v[:, :1], 3, 1)
    return {"w": w, "h": h, "dat": np.asarray(v, np.float32).astype(float).tolist()}


def ext_scene(seed):
    """random_scene plus 0-2 of mesh_fuzz_scene's meshes at 300-600 triangles; every triangle and mesh randomly gets vn and / or
    uv (_ext_attrs), those with uv any of the six maps; the material filter and an environment texture (1..9 x 1..9 texels, one
    in six 1 x 1, f32 values up to 50, either mapping, rot in -2 .. 2, either filter) at random.  Every fourth seed gets
    crowd_scene's extra instances (the instance BVH).  Frames stay at random_scene's sizes."""
    d = random_scene(seed)
    rng = np.random.default_rng(seed + 90001)
    rend = d["scene"]["renderer"]
    for _ in range(int(rng.integers(0, 3))):
        m = {"albedo": [float(x) for x in rng.uniform(0.2, 1.0, 3)], "rough": float(rng.choice([0, 0.3, 1])), "metal": float(rng.choice([0, 0.7])),
             "glass": float(rng.choice([0, 0.3, 0.9])), "opacity": float(rng.choice([1, 1, 0.5, 0.1])), "emit": float(rng.choice([0, 0, 0.5]))}
        o = {"type": "mesh", "mesh": _fuzz_mesh(rng, int(rng.integers(300, 601))), "mat": m,
             "pos": [float(x) for x in rng.uniform(-0.8, 0.8, 3)],
             "dir": [float(x) for x in np.r_[rng.uniform(-0.9, 0.9), rng.normal(size=3)]] if rng.random() < 0.5 else [0, 0, -1, 0]}
        rend.insert(int(rng.integers(0, len(rend) + 1)), o)
    if not any(o["type"] in ("triangle", "mesh") for o in rend):
        rend.append({"type": "triangle", "vtx": [[float(x) for x in rng.uniform(-0.8, 0.8, 3)] for _ in range(3)],
                     "pos": [float(x) for x in rng.uniform(-0.6, 0.6, 3)], "mat": {"albedo": [0.8, 0.7, 0.6], "rough": 0.5}})
    for o in rend:
        if o["type"] not in ("triangle", "mesh"):
            continue
        vn, uv = _ext_attrs(rng, [o["vtx"]] if o["type"] == "triangle" else o["mesh"])
        if vn is not None:
            o["vn"] = vn
        if uv is not None:
            o["uv"] = uv
            for k in MAPS:
                if rng.random() < 0.4:
                    o["mat"][k] = _ext_map(rng, k)
    if rng.random() < 0.5:
        d["scene"]["filter"] = "bilinear"
    if rng.random() < 0.65:
        w, h = (1, 1) if rng.random() < 1 / 6 else (int(rng.integers(1, 10)), int(rng.integers(1, 10)))
        dat = 50.0 * rng.uniform(0.0, 1.0, (w * h, 3)) ** 3          # mostly dim, a few texels near env_scene's sun (50)
        d["scene"]["sky"].update({"tex": {"w": w, "h": h, "dat": np.asarray(dat, np.float32).astype(float).tolist()},
                                  "map": str(rng.choice(["sphere", "latlong"])), "rot": float(rng.uniform(-2.0, 2.0)),
                                  "filter": str(rng.choice(["nearest", "bilinear"]))})
    if seed % 4 == 3:
        for o in rend:
            if o["type"] == "plane":
                continue
            base = o.pop("inst", None) or [[o.get("pos", [0, 0, 0]), o.get("dir", [0, 0, -1, 0])]]
            o.pop("pos", None); o.pop("dir", None)
            inst = list(base)
            for _ in range(int(rng.integers(4, 16))):
                q = [float(x) for x in np.r_[rng.uniform(-0.9, 0.9), rng.normal(size=3)]] if rng.random() < 0.3 else [0, 0, -1, 0]
                inst.append([[float(x) for x in rng.uniform(-3, 3, 3)], q])
            o["inst"] = inst
    return d


EXT_SEEDS = list(range(44))                               # fixed: test_ext_scene_generator_covers_what_it_claims holds on exactly these
EXT_GPU_SEEDS = [0, 3, 5, 7, 14, 15, 19, 23, 26, 31, 38, 43]
THREADS = min(16, os.cpu_count() or 1)


def _check(got, ref, spp):
    assert (np.isnan(got) == np.isnan(ref)).all()
    fin = np.isfinite(ref)
    if fin.any():
        scale = max(1.0, float(np.abs(ref[fin]).max()) / spp)
        assert np.abs(got[fin] - ref[fin]).max() / spp <= 1e-4 * scale


@pytest.mark.parametrize("seed", list(range(40)) + [1000 + k for k in range(8)] + [2000 + k for k in range(4)])
def test_fuzz_kernel_headers_on_x86(seed, oracle_mod, emu_mod):
    render, h = make_holder(ident_scene(seed - 2000) if seed >= 2000 else (crowd_scene(seed - 1000) if seed >= 1000 else random_scene(seed)))
    spp = render.rt.sample
    o = oracle_mod.Oracle(h, seed=seed)
    o.execute(spp)
    ref, _ = o.accum()
    got, _ = emu_mod.render(h, seed, spp)
    _check(got, ref, spp)
    o.set_accum(got, spp)
    ss, out = emu_mod.img(h, got, spp)
    assert np.array_equal(ss, o.img_ss()) and np.array_equal(out, o.img())


# ---- the extension fuzz -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def aov_probes():
    import env_ref as E
    import test_denoise_host as D
    return D.shared_probe(), E.shared_probe()


def _frame_only(desc):
    """The frame and camera of desc around one sphere: what the image path (tone map, Lanczos3) of the x86 build needs, for
    scenes its plain packer does not take."""
    return {"rt": dict(desc["rt"]), "frame": desc["frame"], "scene": {"renderer": [{"type": "sphere", "r": 0.5}]}}


def _ext_tags(desc, features, first_hit_renderer):
    """What one ext_scene exercises, as a set of names."""
    tags = set()
    for r in desc["scene"]["renderer"]:
        if r["type"] not in ("triangle", "mesh"):
            continue
        v, u = "vn" in r, "uv" in r
        tags.add("vn+uv" if v and u else "vn only" if v else "uv only" if u else "no attributes")
        if v and (np.abs(np.asarray(r["vn"])).sum(-1) == 0).any():
            tags.add("zero corner normal")
        if r["type"] == "mesh":
            tags.update(f"mesh {k}" for k in MAPS if isinstance(r["mat"].get(k), dict))
    sky = desc["scene"]["sky"]
    if "tex" in sky:
        tags.add(f"env {sky['map']} {sky['filter']}")
        if sky["tex"]["w"] * sky["tex"]["h"] == 1:
            tags.add("env 1x1")
        if (first_hit_renderer < 0).any():
            tags.add("env with miss pixels")
    if features & F_BVH:
        tags.add("instance BVH")
    tags.add("tex_filter " + desc["scene"].get("filter", "nearest"))
    return tags


EXT_MUST_OCCUR = ["vn only", "uv only", "vn+uv", "zero corner normal", *[f"mesh {k}" for k in MAPS],
                  *[f"env {m} {f}" for m in ("sphere", "latlong") for f in ("nearest", "bilinear")], "env 1x1", "env with miss pixels",
                  "instance BVH", "tex_filter nearest", "tex_filter bilinear"]


def test_ext_scene_generator_covers_what_it_claims(oracle_mod, aov_probes):
    """Every seed of EXT_SEEDS is taken by orc_create_ext and by the packer (none skipped), carries an ext, and over the seeds
    every entry of EXT_MUST_OCCUR occurs -- over the GPU subset EXT_GPU_SEEDS as well."""
    import env_ref as E
    seen, seen_gpu = {}, set()
    for seed in EXT_SEEDS:
        desc = ext_scene(seed)
        render, h = make_holder(desc)
        assert h.ext_ptr() is not None, seed
        o = oracle_mod.Oracle(h, seed=seed)               # raises if orc_create_ext rejects
        info, _, _ = E.x86_pack(aov_probes[1], h)         # raises if the packer rejects
        res, ssaa = desc["frame"]["res"], desc["frame"]["ssaa"]
        assert 3 <= res[0] <= 28 and 3 <= res[1] <= 20 and ssaa in (1, 2, 1.5, 0.75)        # random_scene's sizes
        tags = _ext_tags(desc, info["features"], o.aov()["renderer"])
        o.close()
        for t in tags:
            seen.setdefault(t, []).append(seed)
        if seed in EXT_GPU_SEEDS:
            seen_gpu |= tags
    print({t: len(v) for t, v in sorted(seen.items())})
    assert len(EXT_SEEDS) >= 40 and len(set(EXT_SEEDS)) == len(EXT_SEEDS) and set(EXT_GPU_SEEDS) <= set(EXT_SEEDS)
    for t in EXT_MUST_OCCUR:
        assert t in seen, t
    for t in EXT_MUST_OCCUR:
        assert t in seen_gpu, ("GPU subset", t)


@pytest.mark.parametrize("seed", EXT_SEEDS)
def test_fuzz_ext_kernel_headers_on_x86(seed, oracle_mod, emu_mod, aov_probes):
    """ext_scene through the x86 lane code (env_probe's ev_render, which takes any ext) against the oracle: the accumulator at
    _check's bar, the image bytes from equal accumulators, and the first-hit AOVs bit for bit (test_oracle_aov.compare_aov)."""
    import env_ref as E
    import test_oracle_aov as A
    desc = ext_scene(seed)
    render, h = make_holder(desc)
    spp = render.rt.sample
    o = oracle_mod.Oracle(h, seed=seed)
    o.execute(spp, threads=THREADS)
    ref, _ = o.accum()
    got = E.x86_render(aov_probes[1], h, seed, spp, threads=THREADS)
    assert got.shape == ref.shape
    _check(got, ref, spp)
    o.set_accum(got, spp)
    ss, out = emu_mod.img(make_holder(_frame_only(desc))[1], got, spp)
    assert np.array_equal(ss, o.img_ss()) and np.array_equal(out, o.img())
    A.compare_aov(f"ext {seed}", A.x86_planes(aov_probes, h), o.aov())


@pytest.mark.gpu
@pytest.mark.parametrize("seed", EXT_GPU_SEEDS)
def test_fuzz_ext_gpu(seed, oracle_mod):
    """ext_scene on the GPU against the oracle: accumulator (_check), image bytes, first-hit AOVs."""
    from micro_raytracer_amd import Sampler
    import test_oracle_aov as A
    render, h = make_holder(ext_scene(seed))
    spp = render.rt.sample
    o = oracle_mod.Oracle(h, seed=seed)
    o.execute(spp, threads=THREADS)
    ref, _ = o.accum()
    s = Sampler(seed=seed)
    s.execute(render, n_samples=spp)
    got, _ = s.accum()
    _check(got, ref, spp)
    o.set_accum(got, spp)
    assert np.array_equal(s.img_ss(), o.img_ss()) and np.array_equal(s.img(), o.img())
    A.compare_aov(f"ext {seed} GPU", s.aov(), o.aov())
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", list(range(0, 40, 3)) + [1000, 1001, 1002, 1004] + [2000 + k for k in range(10)])
def test_fuzz_gpu(seed, oracle_mod):
    from micro_raytracer_amd import Sampler
    render, h = make_holder(ident_scene(seed - 2000) if seed >= 2000 else (crowd_scene(seed - 1000) if seed >= 1000 else random_scene(seed)))
    spp = render.rt.sample
    o = oracle_mod.Oracle(h, seed=seed)
    o.execute(spp)
    ref, _ = o.accum()
    s = Sampler(seed=seed)
    s.execute(render, n_samples=spp)
    got, _ = s.accum()
    _check(got, ref, spp)
    o.set_accum(got, spp)
    assert np.array_equal(s.img_ss(), o.img_ss()) and np.array_equal(s.img(), o.img())
    import test_oracle_aov as A
    A.compare_aov(f"fuzz {seed} GPU", s.aov(), o.aov())
    s.close()
