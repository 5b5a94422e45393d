"""The measurements of DESIGN.md section 22 on one MI355X: a 256 x 256 lightmap on the Cornell box's floor, 64 directions, 16 samples --
mrt_gather with device pointers against the same job composed on the host, the shares of its parts, mrt_radiance's kernel time on
the same rays, and SH9 probes against the HEMI_COS gather.

    python profiles/gather_measure.py [OUT.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch

dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gather_ref as G
from micro_raytracer_amd import Sampler, load_render, probes, scenes

render = load_render(scenes.cornell_box(res=(16, 16)))
s = Sampler(seed=1, device=0).create(render)
pos, nrm = probes.lightmap_grid((-1, -1, -0.2), (2, 0, 0), (0, 2, 0), 256, 256)
pos, nrm = pos.reshape(-1, 3), nrm.reshape(-1, 3)
t_pos, t_nrm = torch.from_numpy(pos).to(dev), torch.from_numpy(nrm).to(dev)
res = {"points": int(pos.shape[0]), "n_dirs": 64, "n_samples": 16}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


# device path: warm-up, then three timed calls
info = {}
s.gather(render, t_pos[:4096], t_nrm[:4096], n_dirs=64, n_samples=16)
runs = []
for _ in range(3):
    info = {}
    got, ms = wall(lambda: s.gather(render, t_pos, t_nrm, n_dirs=64, n_samples=16, info=info))
    runs.append({"wall_ms": ms, **{k: info[k] for k in ("gen_ms", "kernel_ms", "reduce_ms", "batches", "segments", "scene_in_lds", "kernel_features")}})
res["device"] = runs
got = got.cpu().numpy()
print("device", runs, flush=True)

# the same job composed on the host: rays to numpy, radiance through the host, numpy reduce
comp = []
for _ in range(2):
    (o, d, k), t_rays = wall(lambda: s.gather_rays(render, pos, nrm, n_dirs=64))
    ri = {}
    sums, t_rad = wall(lambda: s.radiance(render, o, d, 16, key=k, info=ri))
    ref, t_red = wall(lambda: G.reduce(sums, d, 16, G.MEAN))
    comp.append({"rays_ms": t_rays, "radiance_ms": t_rad, "numpy_reduce_ms": t_red, "wall_ms": t_rays + t_rad + t_red, "radiance_kernel_ms": ri["kernel_ms"]})
res["host_composed"] = comp
res["composed_differs_words"] = G.same_bits(got, ref)
print("host", comp, res["composed_differs_words"], flush=True)

# mrt_radiance on the same rays, on the device, alternating with the gather
alt = []
to, td, tk = s.gather_rays(render, t_pos, t_nrm, n_dirs=64)
for _ in range(3):
    ri, gi = {}, {}
    s.radiance(render, to, td, 16, key=tk.view(torch.int32), info=ri)
    s.gather(render, t_pos, t_nrm, n_dirs=64, n_samples=16, info=gi)
    alt.append({"radiance_kernel_ms": ri["kernel_ms"], "gather_kernel_ms": gi["kernel_ms"]})
res["same_kernel"] = alt
print("alt", alt, flush=True)
del to, td, tk

# SH9 probes at the same points against the HEMI_COS gather
sh = s.gather(render, t_pos, n_dirs=64, n_samples=16, out="sh9").cpu().numpy()
e_sh = probes.sh9_irradiance(sh, nrm.astype(np.float64)) / np.pi
rel = np.abs(e_sh - got) / np.maximum(got, 1e-3)
res["sh9_vs_hemi"] = {"hemi_mean": got.mean(0).tolist(), "sh9_irradiance_over_pi_mean": e_sh.mean(0).tolist(),
                      "median_rel": float(np.median(rel)), "p95_rel": float(np.percentile(rel, 95))}
print("sh9", res["sh9_vs_hemi"], flush=True)
s.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
