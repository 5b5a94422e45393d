"""Harness entry point (not the reference's CLI, which stays Rust): render a reference-format JSON description.

    python -m micro_raytracer_amd scene.json -o out.png [--sample N] [--bounce N] [--seed S] [--update]
                                  [--adaptive THRESHOLD [--min-sample N] [--step N]]
                                  [--denoise [--denoise-passes N] [--denoise-mode atrous|variance] [--denoise-sigma-var S]
                                   [--denoise-firefly F]] [--aov PREFIX]
                                  [--sky-tex FILE] [--sky-map sphere|latlong] [--sky-rot TURNS] [--sky-filter nearest|bilinear]
                                  [--tex-filter nearest|bilinear]
                                  [--camera pinhole|equirect [--pano-yaw TURNS] [--pano-guides] [--pano-adaptive THRESHOLD]]
                                  [--resize lanczos3|box]
                                  [--gather POINTS.npy --gather-out OUT.npy [--gather-dirs D] [--gather-sh]]

Mirrors CLI::raytrace (src/cli.rs:155-177): per-sample loop with optional --update saves, then the final image.
--adaptive renders with a per-tile noise threshold instead (Sampler.execute_adaptive), --sample being the cap.
--denoise saves the image of the AOV-guided a-trous filter (Sampler.img_denoised) instead of the raw means; --aov writes the
first-hit normal, albedo and depth as PREFIX.normal.png, PREFIX.albedo.png and PREFIX.depth.png.
--denoise-mode variance drives the filter's colour term by a per-pixel variance estimate from the adaptive half buffer; without
--adaptive the render then goes through execute_adaptive(threshold=0, min = max = --sample, step 16), the bytes of the uniform
render, so --sample must be a multiple of 32.  --denoise-sigma-var and --denoise-firefly (inf: off) tune that mode.
--sky-tex / --sky-map / --sky-rot override the description's environment texture (an image file or a Radiance .hdr), its
mapping and its rotation about +z; --sky-filter / --tex-filter choose the filter of the environment texture and of the material
textures (nearest texel, or bilinear).
--camera equirect renders the frame's supersampled grid as a full lat-long panorama from cam.pos through Sampler.radiance
(cameras.render_equirect), turned by --pano-yaw; cam.dir, fov and aprt are ignored.  --pano-guides also forms the first-hit AOVs
on the panorama's own rays (Sampler.aov_rays, the filter wrapping across the seam); only with it do --denoise (mode atrous) and
--aov go together with --camera equirect.  --pano-adaptive THRESHOLD samples the panorama tile-adaptively on its own rays
(Sampler.radiance_adaptive) with --min-sample, --step and --sample as the cap, and prints the adaptive: line; it leaves the half
buffer of the panorama's grid behind, so with --pano-guides it makes --denoise --denoise-mode variance legal (--pano-adaptive 0 is
the uniform budget with a half buffer).  Variance mode takes no horizontal taps across the seam.
-o out.hdr / out.pfm saves the linear float image (Sampler.img_hdr: the mean radiance at the output resolution, no tone map, no
quantisation; with --denoise the filtered means) as a Radiance picture or a PFM; --resize chooses its filter, Lanczos3 with the
taps of the 8-bit image or the box (area) average a light probe wants.  A panorama written with --camera equirect -o probe.hdr is
what --sky-tex probe.hdr --sky-map latlong loads.
--gather POINTS.npy gathers radiance at points instead of rendering a frame (Sampler.gather): the file holds [n][3] positions (rays
over the whole sphere) or [n][6], position plus normal (cosine-distributed rays over the hemisphere, the mean is irradiance / pi);
--gather-dirs rays per point (default 64), --sample path samples per ray; --gather-out receives float32 [n][3], or with
--gather-sh (positions only) the SH9 probes [n][9][3].  No image is written.
"""
import argparse
import sys
import time

import numpy as np

from . import _abi, _lib, cameras, load_render
from .sampler import Sampler
from .scene import Texture


def is_float_output(path):
    return path.lower().endswith((".hdr", ".pfm"))


def image(s, a):
    dn = dict(passes=a.denoise_passes, mode=a.denoise_mode, sigma_var=a.denoise_sigma_var, firefly=a.denoise_firefly)
    if is_float_output(a.output):
        return s.img_hdr(filter=a.resize or "lanczos3", denoise=dn if a.denoise else None)
    if not a.denoise:
        return s.img()
    return s.img_denoised(**dn)


def save(path, img):
    """uint8 images through mrt_save_image (.png, .ppm), float32 ones through mrt_save_image_f32 (.hdr, .pfm)"""
    (_lib.save_image_f32 if img.dtype == np.float32 else _lib.save_image)(path, img)


def aov_images(aov):
    """The first-hit AOVs as 8-bit images: normal * 0.5 + 0.5, albedo, depth normalised over its finite values."""
    def u8(x):
        return (np.clip(np.nan_to_num(x, nan=0.0), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    d = aov["depth"].astype(np.float64)
    fin = np.isfinite(d)
    dn = np.zeros_like(d)
    if fin.any():
        lo, hi = d[fin].min(), d[fin].max()
        dn[fin] = (d[fin] - lo) / (hi - lo) if hi > lo else 0.0
    return {"normal": u8(aov["normal"] * 0.5 + 0.5), "albedo": u8(aov["albedo"]),
            "depth": np.ascontiguousarray(np.repeat(u8(dn)[..., None], 3, axis=2))}


def save_aov(s, prefix):
    for name, img in aov_images(s.aov()).items():
        _lib.save_image(f"{prefix}.{name}.png", np.ascontiguousarray(img))


def adaptive_line(info, uniform):
    return (f"adaptive: {info['samples']} samples traced of {uniform} uniform ({info['samples'] / uniform:.1%}), "
            f"{info['tiles_converged']} of {info['tiles']} tiles converged, per-pixel counts {info['min_count']}..{info['max_count']}")


def gather(ap, a, s, render, t0):
    """--gather: the points of a.gather through Sampler.gather into a.gather_out"""
    pts = np.load(a.gather)
    if pts.ndim != 2 or pts.shape[1] not in (3, 6) or pts.shape[0] == 0:
        ap.error(f"--gather {a.gather}: expected [n][3] or [n][6], got {pts.shape}")
    if a.gather_sh and pts.shape[1] == 6:
        ap.error("--gather-sh projects the whole sphere: the points file must hold positions only ([n][3])")
    pts = pts.astype(np.float32)
    info = {}
    out = s.gather(render, pts[:, :3], pts[:, 3:] if pts.shape[1] == 6 else None, n_dirs=64 if a.gather_dirs is None else a.gather_dirs,
                   n_samples=render.rt.sample, out="sh9" if a.gather_sh else "mean", info=info)
    np.save(a.gather_out, out)
    print(f"done: {pts.shape[0]} points x {info['rays'] // pts.shape[0]} rays x {render.rt.sample} spp in {time.perf_counter() - t0:.3f} s -> "
          f"{a.gather_out} (gen {info['gen_ms']:.3f} ms, trace {info['kernel_ms']:.3f} ms, reduce {info['reduce_ms']:.3f} ms, "
          f"{info['batches']} batches)", file=sys.stderr)
    s.close()


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m micro_raytracer_amd")
    ap.add_argument("full", help="full render description (JSON, the reference's schema)")
    ap.add_argument("-o", "--output", default="out.png", help=".png or .ppm; .hdr or .pfm: the linear float image")
    ap.add_argument("--sample", type=int)
    ap.add_argument("--bounce", type=int)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("-u", "--update", action="store_true", help="save the image after every sample pass")
    ap.add_argument("--adaptive", type=float, metavar="THRESHOLD",
                    help="tile-adaptive sampling: 8x8 tiles stop once their noise estimate is <= THRESHOLD (--sample is the cap)")
    ap.add_argument("--min-sample", type=int, default=32, help="--adaptive: samples every tile takes (default 32)")
    ap.add_argument("--step", type=int, default=16, help="--adaptive: samples per round, a multiple of 16 (default 16)")
    ap.add_argument("--denoise", action="store_true", help="save the denoised image (AOV-guided a-trous filter)")
    ap.add_argument("--denoise-passes", type=int, default=_abi.DENOISE_PASSES,
                    help=f"--denoise: filter passes, 0..8 (default {_abi.DENOISE_PASSES})")
    ap.add_argument("--denoise-mode", choices=sorted(_abi.DN_MODES), default="atrous",
                    help="--denoise: atrous (fixed colour sigma) or variance (colour term from the adaptive half buffer)")
    ap.add_argument("--denoise-sigma-var", type=float, metavar="S",
                    help=f"--denoise-mode variance: colour width in standard deviations (default {_abi.DN_SIGMA_VAR})")
    ap.add_argument("--denoise-firefly", type=float, metavar="F",
                    help=f"--denoise-mode variance: firefly clamp factor, inf: off (default {_abi.DN_FIREFLY})")
    ap.add_argument("--aov", metavar="PREFIX", help="also write PREFIX.normal.png, PREFIX.albedo.png and PREFIX.depth.png")
    ap.add_argument("--sky-tex", metavar="FILE", help="environment texture of the sky: an image file or a Radiance .hdr")
    ap.add_argument("--sky-map", choices=("sphere", "latlong"), help="mapping of the environment texture")
    ap.add_argument("--sky-rot", type=float, metavar="TURNS", help="rotation of the environment about +z, in turns")
    ap.add_argument("--sky-filter", choices=("nearest", "bilinear"), help="filter of the environment texture")
    ap.add_argument("--tex-filter", choices=("nearest", "bilinear"), help="filter of the material textures")
    ap.add_argument("--camera", choices=("pinhole", "equirect"), default="pinhole",
                    help="equirect: the frame's supersampled grid as a 360 x 180 degree panorama from cam.pos; the description's "
                         "cam.dir, fov and aprt are ignored")
    ap.add_argument("--pano-yaw", type=float, metavar="TURNS", help="--camera equirect: the centre column looks along +y turned by TURNS")
    ap.add_argument("--pano-guides", action="store_true",
                    help="--camera equirect: first-hit AOVs on the panorama's rays, so that --denoise (atrous) and --aov apply to it")
    ap.add_argument("--pano-adaptive", type=float, metavar="THRESHOLD",
                    help="--camera equirect: tile-adaptive sampling on the panorama's rays (--min-sample, --step, --sample as the cap); "
                         "with --pano-guides it allows --denoise-mode variance")
    ap.add_argument("--resize", choices=sorted(_abi.RESIZE_FILTERS), help="filter of a .hdr / .pfm output's resize (default lanczos3)")
    ap.add_argument("--gather", metavar="POINTS.npy", help="gather radiance at the points of this file ([n][3], or [n][6] with normals) "
                                                           "instead of rendering; needs --gather-out")
    ap.add_argument("--gather-out", metavar="OUT.npy", help="--gather: where the float32 answers go")
    ap.add_argument("--gather-dirs", type=int, metavar="D", help="--gather: rays per point (default 64)")
    ap.add_argument("--gather-sh", action="store_true", help="--gather: SH9 probes [n][9][3] instead of the mean radiance (positions only)")
    a = ap.parse_args(argv)
    if a.gather is None:
        if a.gather_out is not None or a.gather_dirs is not None or a.gather_sh:
            ap.error("--gather-out / --gather-dirs / --gather-sh need --gather")
    elif a.gather_out is None:
        ap.error("--gather needs --gather-out")
    if a.resize is not None and not is_float_output(a.output):
        ap.error("--resize needs a .hdr or .pfm output: the 8-bit image is resized as the reference resizes it")
    if a.camera == "equirect":
        if a.adaptive is not None:
            ap.error("--camera equirect cannot be combined with --adaptive, which samples the camera's own rays; use --pano-adaptive")
        if a.update:
            ap.error("--camera equirect cannot be combined with --update")
        for name, on in (("--denoise", a.denoise), ("--aov", a.aov is not None)):
            if on and not a.pano_guides:
                ap.error(f"--camera equirect cannot be combined with {name} unless --pano-guides forms the AOVs on the panorama's rays")
        if a.pano_guides and a.denoise and a.denoise_mode != "atrous" and a.pano_adaptive is None:
            ap.error("--pano-guides: --denoise-mode variance reads a half buffer of the panorama's grid, which only --pano-adaptive "
                     "THRESHOLD leaves behind (0: the uniform budget); or use --denoise-mode atrous")
        if a.pano_adaptive is not None:
            if a.step <= 0 or a.step % 16:
                ap.error(f"--step {a.step} is not a positive multiple of 16")
            if not a.pano_adaptive >= 0.0:
                ap.error("--pano-adaptive THRESHOLD must be >= 0")
    elif a.pano_yaw is not None:
        ap.error("--pano-yaw needs --camera equirect")
    elif a.pano_adaptive is not None:
        ap.error("--pano-adaptive needs --camera equirect")
    elif a.pano_guides:
        ap.error("--pano-guides needs --camera equirect")
    if not 0 <= a.denoise_passes <= 8:
        ap.error(f"--denoise-passes {a.denoise_passes} is not in 0..8")
    variance = a.denoise and a.denoise_mode == "variance"
    if not variance and (a.denoise_sigma_var is not None or a.denoise_firefly is not None):
        ap.error("--denoise-sigma-var / --denoise-firefly need --denoise --denoise-mode variance")
    for name, v in (("--denoise-sigma-var", a.denoise_sigma_var), ("--denoise-firefly", a.denoise_firefly)):
        if v is not None and not v > 0.0:
            ap.error(f"{name} {v} is not > 0")
    if variance and a.adaptive is None and a.pano_adaptive is None:
        if a.update:
            ap.error("--update cannot be combined with --denoise-mode variance")
        if a.sample is not None and (a.sample <= 0 or a.sample % 32):
            ap.error(f"--sample {a.sample} is not a positive multiple of 32: --denoise-mode variance renders through "
                     "execute_adaptive(threshold=0, min = max = --sample, step=16), whose rounds come in pairs of 16 samples")
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
    if a.sky_tex is not None:
        render.scene.sky.tex = Texture.from_json(a.sky_tex)
    if render.scene.sky.tex is None and (a.sky_map is not None or a.sky_rot is not None or a.sky_filter is not None):
        ap.error("--sky-map / --sky-rot / --sky-filter need an environment texture: \"tex\" on the description's \"sky\", or --sky-tex")
    if a.sky_map is not None:
        render.scene.sky.mapping = a.sky_map
    if a.sky_rot is not None:
        render.scene.sky.rot = float(np.float32(a.sky_rot))
    if a.sky_filter is not None:
        render.scene.sky.filter = a.sky_filter
    if a.tex_filter is not None:
        render.scene.tex_filter = a.tex_filter
    s = Sampler(seed=a.seed)
    t0 = time.perf_counter()
    if a.gather is not None:
        return gather(ap, a, s, render, t0)
    if a.camera == "equirect":
        if a.pano_adaptive is None:
            cameras.render_equirect(s, render, yaw=a.pano_yaw or 0.0, guides=a.pano_guides)
        else:
            info = {}
            cameras.render_equirect(s, render, yaw=a.pano_yaw or 0.0, guides=a.pano_guides, info=info,
                                    adaptive=dict(threshold=a.pano_adaptive, min_samples=a.min_sample, step=a.step))
            print(adaptive_line(info, s.nw * s.nh * render.rt.sample))
    elif a.adaptive is not None:
        info = s.execute_adaptive(render, a.adaptive, min_samples=a.min_sample, max_samples=render.rt.sample, step=a.step)
        print(adaptive_line(info, s.nw * s.nh * render.rt.sample))
    elif variance:
        if render.rt.sample <= 0 or render.rt.sample % 32:
            ap.error(f"the description's sample count {render.rt.sample} is not a positive multiple of 32, which --denoise-mode variance "
                     "needs (execute_adaptive with min = max = the sample count, step 16); pass --sample")
        s.execute_adaptive(render, 0.0, min_samples=render.rt.sample, max_samples=render.rt.sample, step=16)
    elif a.update:
        for _ in range(render.rt.sample):
            s.execute(render)
            save(a.output, image(s, a))
    else:
        s.execute(render, n_samples=render.rt.sample)
    save(a.output, image(s, a))
    if a.aov:
        save_aov(s, a.aov)
    st = s.stats()
    print(f"done: {s.nw}x{s.nh} x {render.rt.sample} spp in {time.perf_counter() - t0:.3f} s -> {a.output} "
          f"({st['block_threads']}-thread workgroups, {st['lds_bytes']} B LDS)", file=sys.stderr)


if __name__ == "__main__":
    main()
