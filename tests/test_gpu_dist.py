"""The N > 1 bench path on a one-GPU box: two ranks (gloo, both on device 0) render their row shards with the HIP
kernel, gather to rank 0, and the assembled frame equals the single-context frame bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_two_ranks_on_one_gpu_rehearsal():
    """Plain `python bench.py --gpus 2` (no torchrun, no WORLD_SIZE): bench.py starts its ranks itself."""
    env = dict(os.environ, MRT_DIST_BACKEND="gloo", MRT_SHARE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--workload", "cornell_512_64spp_b8", "--no-cpu-baseline"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["value"] > 0 and d["scaling"] == "strong"
    assert d["config"]["samples_per_step"] == 512 * 512 * 64
    r = d["roofline"]
    assert r["gather_ms"] > 0 and 0 < r["kernel_ms_rank_min"] <= r["kernel_ms_rank_max"]
    assert r["bound"] == "valu_issue" and r["hbm"]["bound"] == "hbm" and 0 < r["frac"] < 1
    # what the process group saw: the first real SCALE record has to explain itself
    ds = d["dist"]
    assert ds["backend"] == "gloo" and ds["world_size"] == 2 and [x["rank"] for x in ds["devices"]] == [0, 1]
    assert ds["distinct_devices"] == 1 and all(x["device_index"] == 0 for x in ds["devices"])      # the rehearsal layout, and it says so
    assert ds["gather_bytes_per_rank"] == 256 * 512 * 12 and ds["use_all_gather"] is False


def test_bench_many_ranks_rehearsal_of_the_scale_run():
    """What the driver's SCALE run does, as far as one GPU allows: plain `python bench.py --gpus N` on the headline frame
    (1920x1080, reduced spp), fresh child processes, every rank on device 0, the gather staged through gloo.  N = 4, not
    8: the GPU box admits at most 6 processes on its card at once, and this pytest process and the launcher's agent are
    two of them (a 5-rank run was killed by the box's process guard); the 8-rank frame is covered by
    tests/test_dist_gloo.py (CPU tensors) and by the in-process shard probe."""
    n = 4
    env = dict(os.environ, MRT_DIST_BACKEND="gloo", MRT_SHARE_DEVICE="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "HSA_ENABLE_IPC_MODE_LEGACY"):
        env.pop(k, None)                      # bench.py sets HSA_ENABLE_IPC_MODE_LEGACY itself, before importing torch
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "1", "--spp", "64"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == n and d["steps"] == 1 and d["value"] > 0 and d["scaling"] == "strong"
    assert d["config"]["workload"] == "cornell_1080p_1024spp_b8" and d["config"]["samples_per_step"] == 1920 * 1080 * 64
    r = d["roofline"]
    assert r["gather_ms"] > 0 and 0 < r["kernel_ms_rank_min"] <= r["kernel_ms_rank_max"]
    assert r["pmc_stale"] is False and r["traffic"] is None          # --spp override: nothing is replayed from a profile
    assert r["bound"] == "valu_issue" and r["frac_source"] == "flop_model" and r["frac"] == r["valu_model_frac"]
    ds = d["dist"]
    assert ds["backend"] == "gloo" and ds["world_size"] == n and len(ds["devices"]) == n
    assert ds["gather_bytes_per_rank"] == 272 * 1920 * 12            # 135 blocks of 8 rows over 4 ranks: 34 blocks = 272 padded rows
    assert "cpu_baseline" not in d                                    # rank 0 at N = 1 only


def test_bench_under_torchrun_still_works():
    """The driver's form: python -m torch.distributed.run ... bench.py --gpus 2."""
    env = dict(os.environ, MRT_DIST_BACKEND="gloo", MRT_SHARE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29731", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
           "--workload", "cornell_512_64spp_b8", "--no-cpu-baseline"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["value"] > 0


def _worker(rank, world, port, out_path, res=(160, 100), shard_rows=8):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    from micro_raytracer_amd import load_render, scenes
    from micro_raytracer_amd.dist import ShardedSampler
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    render = load_render(scenes.cornell_box2(res=res, ssaa=1, sample=3))
    ss = ShardedSampler(render, rank, world, 0, seed=6, shard_rows=shard_rows)
    ss.execute(2)
    ss.execute(1)
    if rank == 0:
        torch.cuda.synchronize()
        np.save(out_path, ss.frame.cpu().numpy())
        np.save(out_path + ".img.npy", ss.img())
    dist.barrier()
    ss.close()
    dist.destroy_process_group()


def _three_ranks_equal_single_context(tmp_path, port, res=(160, 100), shard_rows=8):
    import torch.multiprocessing as mp
    from micro_raytracer_amd import Sampler, load_render, scenes
    out = str(tmp_path / "frame.npy")
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 3, port, out, res, shard_rows)) for r in range(3)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    render = load_render(scenes.cornell_box2(res=res, ssaa=1, sample=3))
    s = Sampler(seed=6)
    s.execute(render, n_samples=3)
    ref, _ = s.accum()
    assert np.array_equal(np.load(out), ref)
    assert np.array_equal(np.load(out + ".img.npy"), s.img())


def test_sharded_sampler_three_ranks_equal_single_context(tmp_path):
    _three_ranks_equal_single_context(tmp_path, 29733)


def test_sharded_sampler_three_ranks_on_five_row_blocks(tmp_path):
    """The same three ranks on a 20 x 23 frame dealt in 5-row blocks (5 blocks, the last of 3 rows; buffers of 10 rows):
    ShardedSampler's own layout, which it asserts equal to the library's, places the gathered rows."""
    _three_ranks_equal_single_context(tmp_path, 29735, res=(20, 23), shard_rows=5)


_GROUP_SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["MRT_ROOT"])
from micro_raytracer_amd import Sampler, load_render, scenes
render = load_render(scenes.cornell_box2(res=(120, 72), ssaa=1, sample=20))
plain = Sampler(seed=3)
plain.execute(render, n_samples=16)
plain.execute(render, n_samples=4)
ref, cnt = plain.accum()
os.environ["MRT_FORCE_RCCL"] = "1"
g = Sampler(seed=3, n_devices=1, flags=1)
g.execute(render, n_samples=16)
st = g.stats()
assert st["samples"] == 120 * 72 * 16 and st["segments"] > 0
g.execute(render, n_samples=4)
g.execute(render, n_samples=0)            # joins the gather without a kernel: its stream is not synchronised by exec_finish,
assert g.stats()["samples"] == 0          # so the gather events are waited for explicitly (ADVICE r3: hipErrorNotReady)
got, gcnt = g.accum()
assert gcnt == cnt == 20
assert np.array_equal(got, ref)
assert np.array_equal(g.img(), plain.img())
loc, rows = g.accum_local()
assert np.array_equal(loc, ref) and list(rows) == list(range(72))
g.reset()
g.set_accum(ref, cnt)                     # resume: push a frame back into the shards, keep sampling
g.execute(render, n_samples=12)
plain.execute(render, n_samples=12)
assert np.array_equal(g.accum()[0], plain.accum()[0])
d = Sampler(seed=3, n_devices=1, flags=4)        # MRT_FLAG_DEFER on the group: 20 per-sample calls, one gathered batch at the observation
for _ in range(20):
    d.execute(render)
got, dcnt = d.accum()
assert dcnt == 20 and np.array_equal(got, ref)
assert d.stats()["launches"] == 1
print("GROUP-OK")
"""


def test_in_process_group_context_rccl_gather_on_one_device():
    """mrt_opts.n_devices: the single-process multi-GPU path (sub-contexts + one ncclGather + row scatter), exercised
    with a communicator of one device; frame, image and a resumed render equal the plain context bit for bit.
    Runs in a fresh interpreter without torch, like the reference's binary: librccl.so is loaded by the library itself
    (a process that already holds PyTorch's bundled RCCL / HIP runtime is not the deployment this path is for)."""
    env = dict(os.environ, MRT_ROOT=ROOT)
    out = subprocess.run([sys.executable, "-c", _GROUP_SCRIPT], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "GROUP-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
