"""Harness entry point (not the reference's CLI, which stays Rust): render a reference-format JSON description.

    python -m micro_raytracer_amd scene.json -o out.png [--sample N] [--bounce N] [--seed S] [--update]
                                  [--adaptive THRESHOLD [--min-sample N] [--step N]]

Mirrors CLI::raytrace (src/cli.rs:155-177): per-sample loop with optional --update saves, then the final image.
--adaptive renders with a per-tile noise threshold instead (Sampler.execute_adaptive), --sample being the cap.
"""
import argparse
import sys
import time

from . import _lib, load_render
from .sampler import Sampler


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m micro_raytracer_amd")
    ap.add_argument("full", help="full render description (JSON, the reference's schema)")
    ap.add_argument("-o", "--output", default="out.png", help=".png or .ppm")
    ap.add_argument("--sample", type=int)
    ap.add_argument("--bounce", type=int)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("-u", "--update", action="store_true", help="save the image after every sample pass")
    ap.add_argument("--adaptive", type=float, metavar="THRESHOLD",
                    help="tile-adaptive sampling: 8x8 tiles stop once their noise estimate is <= THRESHOLD (--sample is the cap)")
    ap.add_argument("--min-sample", type=int, default=32, help="--adaptive: samples every tile takes (default 32)")
    ap.add_argument("--step", type=int, default=16, help="--adaptive: samples per round, a multiple of 16 (default 16)")
    a = ap.parse_args(argv)
    if a.adaptive is not None:
        if a.update:
            ap.error("--update cannot be combined with --adaptive")
        if a.step <= 0 or a.step % 16:
            ap.error(f"--step {a.step} is not a positive multiple of 16")
        if not a.adaptive >= 0.0:
            ap.error("--adaptive THRESHOLD must be >= 0")
    render = load_render(a.full)
    if a.sample is not None:
        render.rt.sample = a.sample
    if a.bounce is not None:
        render.rt.bounce = a.bounce
    s = Sampler(seed=a.seed)
    t0 = time.perf_counter()
    if a.adaptive is not None:
        info = s.execute_adaptive(render, a.adaptive, min_samples=a.min_sample, max_samples=render.rt.sample, step=a.step)
        uniform = s.nw * s.nh * render.rt.sample
        print(f"adaptive: {info['samples']} samples traced of {uniform} uniform ({info['samples'] / uniform:.1%}), "
              f"{info['tiles_converged']} of {info['tiles']} tiles converged, per-pixel counts {info['min_count']}..{info['max_count']}")
    elif a.update:
        for _ in range(render.rt.sample):
            s.execute(render)
            _lib.save_image(a.output, s.img())
    else:
        s.execute(render, n_samples=render.rt.sample)
    _lib.save_image(a.output, s.img())
    st = s.stats()
    print(f"done: {s.nw}x{s.nh} x {render.rt.sample} spp in {time.perf_counter() - t0:.3f} s -> {a.output} "
          f"({st['block_threads']}-thread workgroups, {st['lds_bytes']} B LDS)", file=sys.stderr)


if __name__ == "__main__":
    main()
