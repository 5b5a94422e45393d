"""Offline GPU fuzz (not collected by pytest): libmrt_hip.so against the oracle on many random and crowd scenes.
Usage (on the GPU box): python tests/fuzz_gpu_offline.py FIRST LAST [crowd|ident|deep|plain] [BLOCK_THREADS]
`ident`: random scenes with every instance untransformed and an axis-aligned pinhole camera on a lattice point half of the time
(the F_IDENT kernels; rays and shifted origins with zero components take the reference's mat-vecs).
`deep`: meshes of 300-1500 triangles (mesh_fuzz_scene) on the deep-level kernels, 3 / 7 / 40 staged triangle-BVH nodes and
walk areas of 4 / 6 / 16 entries by seed (MRT_DEEP_NODES, MRT_WALK_CAP).
BLOCK_THREADS forces the workgroup size of every context (MRT_BLOCK_THREADS)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from conftest import make_holder  # noqa: E402
from test_fuzz_scenes import random_scene, crowd_scene, ident_scene, mesh_fuzz_scene, _check  # noqa: E402


def main():
    import importlib
    from micro_raytracer_amd import Sampler
    first, last = int(sys.argv[1]), int(sys.argv[2])
    crowd = len(sys.argv) > 3 and sys.argv[3] == "crowd"
    ident = len(sys.argv) > 3 and sys.argv[3] == "ident"
    deep = len(sys.argv) > 3 and sys.argv[3] == "deep"
    if len(sys.argv) > 4:
        os.environ["MRT_BLOCK_THREADS"] = sys.argv[4]

    oracle_mod = importlib.import_module("oracle.oracle")
    bad = 0
    worst = 0.0
    shapes = {}
    for seed in range(first, last):
        if deep:
            os.environ["MRT_DEEP_NODES"] = ("3", "7", "40")[seed % 3]      # (at least every mesh root: mesh_fuzz_scene has 1-3)
            os.environ["MRT_WALK_CAP"] = ("4", "6", "16")[seed // 3 % 3]
        render, h = make_holder(mesh_fuzz_scene(seed) if deep else ident_scene(seed) if ident else (crowd_scene(seed) if crowd else random_scene(seed)))
        spp = render.rt.sample
        o = oracle_mod.Oracle(h, seed=seed)
        o.execute(spp)
        ref, _ = o.accum()
        s = Sampler(seed=seed).create(render)
        s.execute(render, n_samples=spp)
        got, cnt = s.accum()
        st = s.stats()
        key = (st["block_threads"], st["kernel_features"]) if ident or deep else st["block_threads"]
        shapes[key] = shapes.get(key, 0) + 1
        try:
            _check(got, ref, spp)
            fin = np.isfinite(ref)
            if fin.any():
                worst = max(worst, float(np.abs(got[fin] - ref[fin]).max()) / spp)
            o.set_accum(got, cnt)
            assert np.array_equal(s.img_ss(), o.img_ss()) and np.array_equal(s.img(), o.img())
        except AssertionError as e:
            bad += 1
            print("MISMATCH seed", seed, e, flush=True)
        s.close()
        o.close()
    print(f"GPU fuzz seeds {first}..{last} crowd={crowd} ident={ident} deep={deep} threads={os.environ.get('MRT_BLOCK_THREADS', 'default')}: {bad} mismatches, worst L-inf on mean radiance {worst:.3e}, launch shapes {shapes}", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main())
