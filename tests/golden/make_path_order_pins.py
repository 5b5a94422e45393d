"""Records tests/golden/path_order_*.npy: the accumulators of the frames of tests/path_order_cases.py as uint32 words.

The pins hold what the commit BEFORE the end-before-scatter order of render_pixel computed, so the script is run in a checkout
of that commit (with this file and tests/path_order_cases.py copied in):

    python tests/golden/make_path_order_pins.py x86            # the x86 lane harness (tests/emu)
    python tests/golden/make_path_order_pins.py gpu            # Sampler on cuda:0, the library of that checkout

`--out DIR` writes elsewhere.  x86 writes path_order_x86_<frame>.npy and path_order_x86_split_7_33.npy (two calls into one accumulator).  gpu says whether that library's words equal the x86 pins
(exit status 1 if not) and writes the pin of the one call without an x86 counterpart, path_order_gpu_adaptive.npy.  The GPU's
words equalled the x86 words on every frame when the pins were recorded, so the x86 files serve tests/test_gpu_path_order.py."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import path_order_cases as pc  # noqa: E402


def x86_frame(name):
    from conftest import make_holder
    from emu import emu
    _, first, n, _ = pc.FRAMES[name]
    _, holder = make_holder(pc.desc_of(name))
    acc, _ = emu.render(holder, pc.SEED, n, sample_base=first)
    return pc.words(acc)


def gpu_frame(name):
    from micro_raytracer_amd import Sampler, load_render
    _, first, n, feat = pc.FRAMES[name]
    render = load_render(pc.desc_of(name))
    s = Sampler(seed=pc.SEED, device=0)
    try:
        s.create(render)
        if first:
            s.set_accum(np.zeros((s.nh, s.nw, 3), np.float32), first)
        s.execute(render, n_samples=n)
        assert s.stats()["kernel_features"] == feat, (name, s.stats()["kernel_features"])
        return pc.words(s.accum()[0])
    finally:
        s.close()


def x86_split():
    """Samples [0, 7) then [7, 40) of the Cornell frame into one accumulator: two calls that cut chunk 0."""
    from conftest import make_holder
    from emu import emu
    _, holder = make_holder(pc.desc_of("cornell_40"))
    acc, _ = emu.render(holder, pc.SEED, 7)
    acc, _ = emu.render(holder, pc.SEED, 33, sample_base=7, accum=acc)
    return pc.words(acc)


def gpu_split():
    from micro_raytracer_amd import Sampler, load_render
    render = load_render(pc.desc_of("cornell_40"))
    s = Sampler(seed=pc.SEED, device=0)
    try:
        s.execute(render, n_samples=7)
        s.execute(render, n_samples=33)
        return pc.words(s.accum()[0])
    finally:
        s.close()


def gpu_adaptive():
    """mrt_execute_adaptive on the Cornell frame: threshold 0, so every tile runs the tile-list kernel to max_samples."""
    from micro_raytracer_amd import Sampler, load_render
    render = load_render(pc.desc_of("cornell_40"))
    s = Sampler(seed=pc.SEED, device=0)
    try:
        s.execute_adaptive(render, 0.0, min_samples=32, max_samples=64, step=16)
        return pc.words(s.accum()[0])
    finally:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("x86", "gpu"))
    ap.add_argument("--out", default=pc.GOLDEN)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.what == "x86":
        for name in pc.FRAMES:
            np.save(os.path.join(a.out, os.path.basename(pc.pin_path("x86", name))), x86_frame(name))
        np.save(os.path.join(a.out, "path_order_x86_split_7_33.npy"), x86_split())
        return 0
    differ = [name for name in pc.FRAMES if not np.array_equal(gpu_frame(name), pc.load_pin("x86", name))]
    if not np.array_equal(gpu_split(), pc.load_pin("x86", "split_7_33")):
        differ.append("split_7_33")
    print("GPU words equal the x86 pins on every frame" if not differ else f"GPU words differ from the x86 pins on {differ}")
    np.save(os.path.join(a.out, "path_order_gpu_adaptive.npy"), gpu_adaptive())
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
