"""Item schedules of a sample-split launch, replayed from per-path segment counts (not collected by pytest).

    make -C tests/emu libsched.so && python tests/emu/sched_items.py [tiles] [samples]

Segments per path are recorded on the CPU (sched_probe.cpp probe_paths) for a few 8x8 tiles of the 1080p Cornell box and
replayed through the ways a launch can deal one tile's 64 pixels x n chunks of 16 samples to wavefronts:
  k_split K      today's items: a lane owns a pixel and every K-th chunk
  bands          a lane owns a pixel; items are contiguous bands of chunks (plan_bands of mrt_plan.cpp, or a forced list)
  pool           the 64 lanes of a wavefront share an item's (pixel, chunk) jobs, chunk-major, a lane takes the next when its
                 chunk ends (tried on the GPU and dropped: DESIGN.md section 7)
  ideal          every lane always busy
An item lasts as many wave iterations as its slowest lane has segments.  Part 1 prints, per schedule, the lanes on per
iteration and the wave iterations relative to k_split 8: what a wavefront issues.  Part 2 deals the items of a whole frame --
its tiles drawn from the probed ones -- to the device's wavefront slots in launch order, each slot taking the next item when
it is free, and prints the time of the last slot relative to k_split 8: what the launch takes.

What the GPU says: the wave iterations are right -- SQ_INSTS_VALU and SQ_WAVE_CYCLES fall as column 2
says -- and so is the launch time of the tapers whose first band is at most half the launch (31,16,8,4,2: 0.978 here, 0.980
measured).  The steeper tapers end LATER on the GPU than k_split 8 (42,14,5,2,1: 1.005; 56,7,1: 1.07) where this model has
them ahead: thirty probed tiles dealt round-robin do not carry the frame's spread of tile costs, so part 2 understates the
drain behind a long band.  The pool's gain in column 2 did not survive its cost per iteration on the GPU."""
import ctypes as C
import heapq
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from micro_raytracer_amd import _abi, load_render, scenes  # noqa: E402

L = C.CDLL(os.path.join(HERE, "libsched.so"))
CHUNK = 16


def chunk_costs(desc, tx, ty, S, cap=24):
    """segments of chunk j of pixel p of tile (tx, ty): [64][S / 16]"""
    hd = _abi.build_desc(load_render(desc))
    out = np.zeros((64 * S, cap), np.uint32)
    nit = np.zeros(64 * S, np.uint32)
    L.probe_paths(C.cast(hd.ptr(), C.c_void_p), C.c_uint64(1), S, tx * 8, ty * 8, 8, 8, cap,
                  out.ctypes.data_as(C.POINTER(C.c_uint32)), nit.ctypes.data_as(C.POINTER(C.c_uint32)))
    return nit.reshape(64, S // CHUNK, CHUNK).sum(axis=2).astype(np.int64)


def owned(c, chunks):
    """wave iterations of an item whose lane p traces `chunks` of pixel p"""
    return int(c[:, chunks].sum(axis=1).max())


def pooled(c, chunks):
    """... whose 64 lanes share the jobs (pixel, chunk), chunk-major, lane l starting on job l"""
    free = [(int(c[p, chunks[0]]), p) for p in range(64)]
    heapq.heapify(free)
    for j in chunks[1:]:
        for p in range(64):
            t, lane = heapq.heappop(free)
            heapq.heappush(free, (t + int(c[p, j]), lane))
    return max(t for t, _ in free)


def k_split_items(n, k):
    return [list(range(i, n, k)) for i in range(k)]


def band_items(n, bands):
    items, at = [], 0
    for b in bands:
        b = min(b, n - at)
        if b < 1:
            break
        items.append(list(range(at, at + b)))
        at += b
    return items + [[j] for j in range(at, n)]


def rule(n, tiles, slots, slack=4):
    """plan_bands of mrt_plan.cpp"""
    bands, rem = [], n
    while rem and len(bands) < 8:
        b = rem * tiles // (tiles + slack * slots)
        if b < 2:
            break
        bands.append(b)
        rem -= b
    return bands


def launch_time(costs, items, tiles, slots, cost_of):
    """time of the last of `slots` slots when the items of `tiles` tiles are drawn item-major, in order"""
    free = [0] * slots
    heapq.heapify(free)
    per_tile = [[cost_of(c, it) for it in items] for c in costs]
    end = 0
    for i in range(len(items)):
        for t in range(tiles):
            at = heapq.heappop(free) + per_tile[(t * 7919) % len(costs)][i]
            end = max(end, at)
            heapq.heappush(free, at)
    return end


if __name__ == "__main__":
    n_tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    S = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    n = S // CHUNK
    desc = scenes.cornell_box(res=(1920, 1080), sample=S, bounce=8)
    grid = [(x, y) for y in range(7, 135, 27) for x in range(10, 240, 40)][:n_tiles]
    costs = [chunk_costs(desc, tx, ty, S) for tx, ty in grid]
    total = sum(int(c.sum()) for c in costs)
    TILES, SLOTS = 240 * 135, 256 * 32
    scheds = [(f"k_split {k}", k_split_items(n, k), owned) for k in (1, 2, 4, 8, 16) if k <= n]
    lists = [[48, 8, 4, 2, 1, 1], [56, 7, 1], [42, 14, 5, 2, 1], [36, 15, 7, 3, 1], rule(n, TILES, SLOTS), [21, 14, 9, 6, 4, 3, 2], [32, 16, 16], [8] * 8]
    scheds += [("bands " + ",".join(map(str, b)), band_items(n, b), owned) for b in lists]
    scheds += [("pool, one band of all chunks", band_items(n, [n]), pooled), ("pool per band 48,8,4,2,1,1", band_items(n, lists[0]), pooled),
               ("pool per band " + ",".join(map(str, lists[4])), band_items(n, lists[4]), pooled)]
    print(f"{len(costs)} tiles, {S} samples per pixel, {total / (len(costs) * 64 * S):.2f} segments per sample; frame of {TILES} tiles on {SLOTS} slots")
    print(f"{'schedule':44s} {'lanes on':>9s} {'wave iterations':>16s} {'launch time':>12s}")
    rows = [(name, sum(cost_of(c, i) for c in costs for i in items), launch_time(costs, items, TILES, SLOTS, cost_of)) for name, items, cost_of in scheds]
    base_it, base_t = next(((it, t) for name, it, t in rows if name == "k_split 8"), rows[0][1:])
    for name, it, t in rows:
        print(f"{name:44s} {total / (64 * it):9.3f} {it / base_it:16.3f} {t / base_t:12.3f}")
    print(f"{'every lane always busy':44s} {1.0:9.3f} {total / 64 / base_it:16.3f} {total / 64 * TILES / len(costs) / SLOTS / base_t:12.3f}")
