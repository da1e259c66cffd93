#!/usr/bin/env python3
"""What variance-guided filtering of accumulated path frames costs, which of its two iteration
kernels is faster at which step, how much nearer the converged frame it brings a sequence of
one-sample frames than accumulate and accumulate + denoise do, and which sigma_luminance does that
best. Writes profiles/svgf.txt (or --out).

On the current device, with tools/denoise_probe.py's protocol (device events round the call, 5
warm-up calls, the median of --reps calls, three such medians: their middle and their range):
  * timing, per scene at 640x480 and 1920x1080, over 8 real path frames of a static camera:
      - mrt_svgf_accumulate against mrt_temporal_accumulate in the same run (both linear): the fused
        launch reads 16 and writes 16 compulsory bytes per pixel more (148 -> 180);
      - the variance launch (mrt_svgf_filter, 0 iterations) on frame 1's moments, where every hit
        takes the 7 x 7 path, and on frame 8's, where almost none does;
      - each iteration with the direct kernel (variant 1) and the LDS-staged one (variant 2): step
        2^k's launch is t(k + 1 iterations) - t(k iterations), as DESIGN section 16 took its own. The
        staged kernel wins a step where it is faster by more than the summed ranges;
      - the whole of Renderer.svgf's launches (features, mrt_svgf_accumulate, mrt_svgf_filter at 5
        iterations) against the pair it replaces (features, mrt_temporal_accumulate, features again,
        mrt_denoise_filter at 5 iterations, as Renderer.accumulate and Renderer.denoise run them).
  * quality, per scene at 640x480, depth 4, over tools/temporal_probe.py's six sequences (static,
    pans of 1, 4 and 16 pixels, moving followed and not followed): the MSE of the float image
    against S = --converged of the last camera and vertices, after 8 frames of S = 1, for the
    accumulated frame, accumulate + denoise at its defaults, and svgf over sigma_luminance in
    {1, 2, 4, 8, 16}; the default is the value with the lowest mean ratio to the accumulated frame
    among those that make no sequence worse than it.
These are measurements, not gates; the defaults (mrt.svgf.SIGMA_LUMINANCE_DEFAULT,
csrc/svgf_limits.hpp's kTiledDefaultMaxStep) are set from them by hand.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "gpu-ray-tracing_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

import bench  # noqa: E402
from mrt import _lib  # noqa: E402
from mrt.denoise import ITERATIONS_DEFAULT, SIGMA_COLOR_DEFAULT, Denoiser  # noqa: E402
from mrt.svgf import SIGMA_LUMINANCE_DEFAULT, SvgfAccumulator  # noqa: E402
from mrt.temporal import MAX_HISTORY_DEFAULT, NORMAL_COS_DEFAULT, SIGMA_PLANE_FRACTION_DEFAULT, world_to_screen  # noqa: E402
from temporal_probe import FRAMES, HBM_BYTES_PER_S, box_of, displaced, mse, render, renderer_of, sequences, three_medians  # noqa: E402

SIGMAS = [1.0, 2.0, 4.0, 8.0, 16.0]
STEPS = 5      # iterations timed: steps 1 .. 16, the staged kernel's range


# ---- timing ------------------------------------------------------------------------------------------------------------
def timing(name, entry, w, h, reps, out):
    wr = out.write
    scene = entry["scene"]
    cam, _ = scene.camera()
    r = renderer_of(entry, 1)
    dev, n = r.gen.device, w * h
    acc = SvgfAccumulator(dev)
    matrix = world_to_screen(cam, w, h)
    sigma = box_of(scene.arrays()[0])[2] * SIGMA_PLANE_FRACTION_DEFAULT
    blended = torch.empty((n, 4), dtype=torch.float32, device=dev)
    first = None
    for k in range(FRAMES):
        image = render(r, cam, w, h)
        acc.accumulate(r.primary, r.slot_to_id, r.gen.normals, r._recon.material, w, h, matrix, (0.5, 0.5), image,
                       image_out=blended, sigma_plane=sigma)
        if k == 0:
            first = (blended.clone(), acc.current["moments"].clone())
    torch.cuda.synchronize()
    lib, stream = _lib.trace_lib(), torch.cuda.current_stream().cuda_stream or None
    cur, prev = acc.sets[acc._cur], acc.sets[1 - acc._cur]     # write the set that is not the last frame's
    o, px = torch.empty_like(image), torch.empty(n, dtype=torch.int32, device=dev)
    scratch = [torch.empty_like(image) for _ in range(2)]
    wr(f"   {name} {w}x{h}\n")

    def accumulate(params, export):
        p = params()
        p.width, p.height, p.havePrev, p.maxHistory, p.variant = w, h, 1, MAX_HISTORY_DEFAULT, 1
        p.normalCos, p.sigmaPlane = NORMAL_COS_DEFAULT, sigma
        for i in range(16):
            p.prevWorldToScreen[i] = float(matrix[i])
        p.prevSubpixel[0] = p.prevSubpixel[1] = 0.5
        p.image, p.guide, p.albedo = image.data_ptr(), prev["guide"].data_ptr(), prev["albedo"].data_ptr()
        p.prevGuide, p.prevHistory = prev["guide"].data_ptr(), prev["history"].data_ptr()
        p.history, p.imageOut, p.pixels = cur["history"].data_ptr(), o.data_ptr(), px.data_ptr()
        if params is _lib.SvgfAccumulateParams:
            p.prevMoments, p.moments = prev["moments"].data_ptr(), cur["moments"].data_ptr()
        return lambda: _lib.check(export(C.byref(p), stream))
    plain, fused = accumulate(_lib.TemporalParams, lib.mrt_temporal_accumulate), accumulate(_lib.SvgfAccumulateParams, lib.mrt_svgf_accumulate)
    (tp, plo, phi), (tf, flo, fhi) = three_medians(plain, reps), three_medians(fused, reps)
    wr(f"      accumulate (linear): mrt_temporal_accumulate {tp:.4f} ms ({plo:.4f} .. {phi:.4f}) = {100 * n * 148 / (tp * 1e-3) / HBM_BYTES_PER_S:.1f} % "
       f"of 8 TB/s; mrt_svgf_accumulate {tf:.4f} ms ({flo:.4f} .. {fhi:.4f}) = {100 * n * 180 / (tf * 1e-3) / HBM_BYTES_PER_S:.1f} %; "
       f"ratio {tf / tp:.3f} for 180 / 148 = {180 / 148:.3f} of the compulsory bytes\n")

    def svgf_filter(iterations, variant, source, moments):
        q = _lib.SvgfFilterParams()
        q.width, q.height, q.iterations, q.normalSquarings, q.variant = w, h, iterations, 7, variant
        q.sigmaLuminance, q.sigmaPlane = SIGMA_LUMINANCE_DEFAULT, sigma
        q.image, q.guide, q.albedo, q.moments = source.data_ptr(), prev["guide"].data_ptr(), prev["albedo"].data_ptr(), moments.data_ptr()
        q.scratch[0], q.scratch[1] = scratch[0].data_ptr(), scratch[1].data_ptr()
        q.imageOut, q.pixels = o.data_ptr(), px.data_ptr()
        return lambda: _lib.check(lib.mrt_svgf_filter(C.byref(q), stream))
    last = prev["moments"]
    hit = prev["guide"][:, 3] != 0
    (t1, l1, h1), (t8, l8, h8) = (three_medians(svgf_filter(0, 0, src, mom), reps) for src, mom in (first, (blended, last)))
    wr(f"      variance launch: frame 1 ({float((first[1][hit, 3] < 4).float().mean()):.3f} of the hits take the 7 x 7 path) {t1:.4f} ms "
       f"({l1:.4f} .. {h1:.4f}); frame 8 ({float((last[hit, 3] < 4).float().mean()):.3f}) {t8:.4f} ms ({l8:.4f} .. {h8:.4f})\n")
    total = {(variant, k): three_medians(svgf_filter(k, variant, blended, last), reps) for variant in (1, 2) for k in range(STEPS + 1)}
    wr(f"      {'step':>5s} {'direct ms':>22s} {'staged ms':>22s}   the faster, and by how much against the summed ranges\n")
    winners = []
    for k in range(STEPS):
        d = {}
        for variant in (1, 2):
            (a, alo, ahi), (b, blo, bhi) = total[variant, k + 1], total[variant, k]
            d[variant] = (a - b, (ahi - alo) + (bhi - blo))
        (td, rd), (ts, rs) = d[1], d[2]
        spread = max(rd, rs)
        verdict = "staged" if td - ts > spread else ("direct" if ts - td > spread else "neither (within the range)")
        winners.append((1 << k, verdict))
        wr(f"      {1 << k:5d} {td:10.4f} (+-{rd:.4f}) {ts:10.4f} (+-{rs:.4f})   {verdict}: direct - staged = {td - ts:+.4f} ms\n")
    (a, alo, ahi), (b, blo, bhi) = total[1, STEPS], total[2, STEPS]
    wr(f"      {STEPS} iterations, whole call: direct {a:.4f} ms ({alo:.4f} .. {ahi:.4f}), staged {b:.4f} ms ({blo:.4f} .. {bhi:.4f})\n")
    # the whole of Renderer.svgf against Renderer.accumulate + Renderer.denoise, launch for launch
    dn = Denoiser(dev)

    def features():
        dn.set_frame(r.primary, r.slot_to_id, r.gen.normals, r._recon.material, w, h)
    features()
    g = _lib.DenoiseParams()
    g.width, g.height, g.iterations, g.normalSquarings, g.sigmaColor, g.sigmaPlane = w, h, ITERATIONS_DEFAULT, 7, SIGMA_COLOR_DEFAULT, sigma
    g.image, g.guide, g.albedo, g.imageOut, g.pixels = blended.data_ptr(), dn.guide.data_ptr(), dn.albedo.data_ptr(), o.data_ptr(), px.data_ptr()
    g.scratch[0], g.scratch[1] = scratch[0].data_ptr(), scratch[1].data_ptr()
    shipped = svgf_filter(ITERATIONS_DEFAULT, 0, blended, last)

    def pair():
        features()
        plain()
        features()
        _lib.check(lib.mrt_denoise_filter(C.byref(g), stream))

    def whole():
        features()
        fused()
        shipped()
    (tw, wlo, whi), (tq, qlo, qhi) = three_medians(whole, reps), three_medians(pair, reps)
    wr(f"      the whole: svgf (features, accumulate with moments, variance and {ITERATIONS_DEFAULT} iterations, the shipped variant) {tw:.4f} ms "
       f"({wlo:.4f} .. {whi:.4f}); accumulate + denoise (features twice, as the Renderer runs them) {tq:.4f} ms ({qlo:.4f} .. {qhi:.4f}); "
       f"ratio {tw / tq:.3f}\n")
    out.flush()
    return winners


# ---- quality -----------------------------------------------------------------------------------------------------------
def quality(name, entry, converged, out):
    wr = out.write
    scene = entry["scene"]
    cam, _ = scene.camera()
    w, h = 640, 480
    v0, tris, _ = scene.arrays()
    diagonal = box_of(v0)[2]
    sigma = diagonal * SIGMA_PLANE_FRACTION_DEFAULT
    wr(f"== {name}: {scene.num_triangles} triangles, {w}x{h}, depth 4, box diagonal {diagonal:.4g}; {FRAMES} frames of S = 1 against "
       f"S = {converged}; accumulate + denoise and svgf per sigma_luminance, each / the accumulated frame\n")
    ratios = {}
    for label, cams, follow in sequences(cam, h):
        moving = follow is not None
        steps = [displaced(v0, 0.02 * k / (FRAMES - 1)) for k in range(FRAMES)] if moving else None
        ref_r = renderer_of(entry, converged)
        if moving:
            ref_r.set_vertices(steps[-1])
        ref = render(ref_r, cams[-1], w, h)[:, :3].double()
        del ref_r
        r = renderer_of(entry, 1)
        dev = r.gen.device
        acc = SvgfAccumulator(dev)
        tri = torch.from_numpy(tris).to(dev)
        blended, o = (torch.empty((w * h, 4), dtype=torch.float32, device=dev) for _ in range(2))
        previous = torch.from_numpy(v0).to(dev)
        for k in range(FRAMES):
            current = previous
            if moving:
                current = torch.from_numpy(steps[k]).to(dev)
                r.set_vertices(current)
            image = render(r, cams[k], w, h)
            motion = dict(triangles=tri, vertices=current, prev_vertices=previous) if follow and k else {}
            acc.accumulate(r.primary, r.slot_to_id, r.gen.normals, r._recon.material, w, h, world_to_screen(cams[k], w, h), (0.5, 0.5),
                           image, image_out=blended, sigma_plane=sigma, **motion)
            previous = current
        torch.cuda.synchronize()
        base = mse(blended, ref)
        r.denoise(blended, image_out=o)
        torch.cuda.synchronize()
        ratios.setdefault("denoise", {})[label] = mse(o, ref) / base
        for s in SIGMAS:
            acc.filter(blended, image_out=o, sigma_luminance=s, sigma_plane=sigma)
            torch.cuda.synchronize()
            ratios.setdefault(s, {})[label] = mse(o, ref) / base
        hit = acc.current["guide"][:, 3] != 0
        short = float((acc.current["moments"][hit, 3] < 4).float().mean())
        wr(f"   {label:22s} last frame alone {mse(image, ref):.6g}; accumulated {base:.6g}; accumulate + denoise {ratios['denoise'][label]:.4f}; svgf "
           + ", ".join(f"{s:g}: {ratios[s][label]:.4f}" for s in SIGMAS) + f"; hits with fewer than 4 frames {short:.3f}\n")
        out.flush()
        print(f"{name} {label} done", flush=True)
        del acc
        torch.cuda.empty_cache()
    return ratios


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="bunny,hairball")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--converged", type=int, default=1024)
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--bvh-cache", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "mrt_bvhcache"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "svgf.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("svgf_probe needs a GPU: a time taken anywhere else says nothing")
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda").cpu()   # the device is initialised before anything is timed
    scenes = bench.SceneCache(1, 0, args.bvh_cache)
    names = args.scenes.split(",")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        out.write(f"tools/svgf_probe.py on {torch.cuda.get_device_name(0)}, medians of {args.reps}, three medians: middle (lowest .. highest)\n\n")
        out.write(f"== timing: frame {FRAMES} of a static camera (every hit reprojects 1:1); a step's launch is t(k + 1 iterations) - t(k iterations)\n")
        winners = []
        for name in names:
            for w, h in ((640, 480), (1920, 1080)):
                winners.append(timing(name, scenes.get(name), w, h, max(5, args.reps), out))
                print(f"{name} {w}x{h} timed", flush=True)
        staged = [step for step in (1, 2, 4, 8, 16) if all(dict(ws)[step] == "staged" for ws in winners)]
        out.write(f"   the staged kernel wins on every scene and size at steps {staged}\n\n")
        if args.skip_quality:
            return
        table = {}
        for name in names:
            for key, per in quality(name, scenes.get(name), args.converged, out).items():
                for label, ratio in per.items():
                    table.setdefault(key, {})[f"{name} {label}"] = ratio
        out.write("\n== defaults: MSE / the accumulated frame's over the twelve sequences: mean, worst\n")
        for key, per in table.items():
            what = "accumulate + denoise" if key == "denoise" else f"svgf, sigma_luminance {key:g}"
            out.write(f"   {what:28s} mean {statistics.mean(per.values()):.4f} worst {max(per.values()):.4f}"
                      f"{'   <- shipped' if key == SIGMA_LUMINANCE_DEFAULT else ''}\n")
        ok = {k: per for k, per in table.items() if k != "denoise" and max(per.values()) <= 1.0}
        if ok:
            best = min(ok, key=lambda k: statistics.mean(ok[k].values()))
            out.write(f"lowest mean ratio among the {len(ok)} values that made no sequence worse than the accumulated frame: sigma_luminance {best:g} "
                      f"(mean {statistics.mean(ok[best].values()):.4f})\n")
        else:
            out.write("no sigma_luminance left every sequence no worse than its accumulated frame: 4 ships as provisional\n")


if __name__ == "__main__":
    main()
