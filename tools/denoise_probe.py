#!/usr/bin/env python3
"""What the path frame's denoiser costs, which of its two filter kernels is faster at which step,
and which settings denoise best. Writes profiles/denoise.txt (or --out).

On the current device, with tools/path_probe.py's protocol (device events round the call, 5 warm-up
calls, the median of --reps calls, three such medians: their middle and their range) and its light:
  * timing, on the first scene at 640x480 and 1920x1080 (a real path frame's image and features):
    the features call; the filter at 1 .. 8 iterations with the direct kernel (variant 1) and with
    the LDS-staged kernel at every step it fits (variant 2, steps 1 .. 16). One call is one launch
    per iteration, so step 2^k's launch is reported as t(k + 1 iterations) - t(k iterations); the
    difference also holds what turning launch k - 1 from a last into a middle launch saves (16 bytes
    read and 20 written per pixel less). The staged kernel wins a step where its difference is
    below the direct one's by more than the larger of the two ranges. Compulsory bytes (48 read
    and 16 written per pixel and iteration) over the time as a share of 8 TB/s.
  * the share: per scene at 640x480, S = 8, depth 4, the whole denoise (features + 5 iterations, the
    shipped variant) against the summed trace time of the same frame.
  * quality: per scene at 640x480, the MSE of the float image (r, g, b over all pixels) against a
    converged frame (same camera, S = --converged) before and after denoising, at S in {1, 4, 8},
    over sigma_color in {0.25, 0.5, 1, 2, 4} and sigma_plane in {1/50, 1/200, 1/1000} of the scene
    box's diagonal; the setting with the lowest mean ratio over scenes and S.
These are measurements, not gates; the defaults (mrt.denoise, csrc/denoise_limits.hpp's
kTiledDefaultMaxStep) are set from them by hand.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from mrt import _lib  # noqa: E402
from mrt.denoise import Denoiser  # noqa: E402
from mrt.raygen import RAY_PATH  # noqa: E402
from mrt.renderer import GlibcRand, Renderer  # noqa: E402
from mrt.tracer import Tracer  # noqa: E402

HBM_BYTES_PER_S = 8e12
DEPTH = 4
SIGMA_COLORS = [0.25, 0.5, 1.0, 2.0, 4.0]
PLANE_FRACTIONS = [1 / 50, 1 / 200, 1 / 1000]


def event_ms(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    z.record()
    torch.cuda.synchronize()
    return a.elapsed_time(z)


def three_medians(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    lo, mid, hi = sorted(statistics.median(event_ms(fn) for _ in range(reps)) for _ in range(3))
    return mid, lo, hi


def light_of(scene):
    v, _, _ = scene.arrays()
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    return (tuple(float(x) for x in lo + (hi - lo) * np.array([0.5, 0.9, 0.9])), float(0.1 * np.linalg.norm(hi - lo)),
            float(np.linalg.norm(hi - lo)))


def renderer_of(entry, samples):
    scene = entry["scene"]
    tracer = Tracer(0)
    tracer.set_bvh(entry["gbvh"])
    light, radius, _ = light_of(scene)
    r = Renderer(tracer, scene, rand=GlibcRand())
    r.set_params(RAY_PATH, samples, depth=DEPTH, light_pos=light, light_radius=radius)
    return r


def render(r, cam, w, h):
    """One path frame: (float image, summed trace ms)."""
    r.begin_frame(cam, w, h)
    px = torch.zeros(w * h, dtype=torch.int32, device=r.gen.device)
    img = torch.zeros((w * h, 4), dtype=torch.float32, device=r.gen.device)
    ms = 0.0
    while r.next_batch():
        ms += r.trace_batch()
        r.update_result(px, img)
    torch.cuda.synchronize()
    return img, ms


def filter_call(dn, image, out, px, iterations, variant, sigma_color=1.0, sigma_plane=1.0):
    p = _lib.DenoiseParams()
    p.width, p.height, p.iterations, p.normalSquarings, p.variant = dn.w, dn.h, iterations, 7, variant
    p.sigmaColor, p.sigmaPlane = sigma_color, sigma_plane
    p.image, p.guide, p.albedo = image.data_ptr(), dn.guide.data_ptr(), dn.albedo.data_ptr()
    p.scratch[0], p.scratch[1] = dn.scratch[0].data_ptr(), dn.scratch[1].data_ptr()
    p.imageOut, p.pixels = out.data_ptr(), px.data_ptr()
    lib = _lib.trace_lib()
    stream = torch.cuda.current_stream().cuda_stream or None
    return lambda: _lib.check(lib.mrt_denoise_filter(C.byref(p), stream))


def timing(entry, w, h, reps, out):
    wr = out.write
    scene = entry["scene"]
    cam, _ = scene.camera()
    r = renderer_of(entry, 1)
    image, _ = render(r, cam, w, h)
    _, _, diagonal = light_of(scene)
    dn = Denoiser(r.gen.device)
    n = w * h

    def features():
        dn.set_frame(r.primary, r.slot_to_id, r.gen.normals, r._recon.material, w, h)
    t, lo, hi = three_medians(features, reps)
    moved = n * (4 + 32 + 16 + 48)
    wr(f"   {w}x{h}: features {t:.4f} ms ({lo:.4f} .. {hi:.4f}); {moved / 1e6:.1f} MB compulsory = "
       f"{100 * moved / (t * 1e-3) / HBM_BYTES_PER_S:.1f} % of 8 TB/s\n")
    o, px = torch.empty_like(image), torch.empty(n, dtype=torch.int32, device=image.device)
    total = {}
    for variant, label in ((1, "direct"), (2, "staged")):
        for iterations in range(0, 9):
            total[variant, iterations] = three_medians(filter_call(dn, image, o, px, iterations, variant, 1.0, diagonal / 200), reps)
    wr(f"      {'step':>5s} {'direct ms':>22s} {'staged ms':>22s}   the faster, and by how much against the larger range\n")
    winners = []
    for k in range(8):
        step = 1 << k
        d = {}
        for variant in (1, 2):
            (a, alo, ahi), (b, blo, bhi) = total[variant, k + 1], total[variant, k]
            base = b if k else 0.0
            d[variant] = (a - base, (ahi - alo) + ((bhi - blo) if k else 0.0))
        (td, rd), (ts, rs) = d[1], d[2]
        byts = n * 64
        if step <= 16:
            spread = max(rd, rs)
            verdict = "staged" if td - ts > spread else ("direct" if ts - td > spread else "neither (within the range)")
            winners.append((step, verdict))
            wr(f"      {step:5d} {td:10.4f} (+-{rd:.4f}) {ts:10.4f} (+-{rs:.4f})   {verdict}: direct - staged = {td - ts:+.4f} ms, "
               f"range {spread:.4f}; direct {100 * byts / (td * 1e-3) / HBM_BYTES_PER_S:.1f} %, staged "
               f"{100 * byts / (ts * 1e-3) / HBM_BYTES_PER_S:.1f} % of 8 TB/s\n")
        else:
            wr(f"      {step:5d} {td:10.4f} (+-{rd:.4f}) {'(direct: no tile)':>22s}   direct {100 * byts / (td * 1e-3) / HBM_BYTES_PER_S:.1f} % of 8 TB/s\n")
    for iterations in (0, 1, 5, 8):
        (a, alo, ahi), (b, blo, bhi) = total[1, iterations], total[2, iterations]
        wr(f"      {iterations} iterations, whole call: direct {a:.4f} ms ({alo:.4f} .. {ahi:.4f}), staged up to step 16 {b:.4f} ms "
           f"({blo:.4f} .. {bhi:.4f})\n")
    out.flush()
    return winners


def share_and_quality(name, entry, reps, converged, out):
    wr = out.write
    scene = entry["scene"]
    cam, _ = scene.camera()
    w, h = 640, 480
    _, _, diagonal = light_of(scene)
    wr(f"== {name}: {scene.num_triangles} triangles, {w}x{h}, depth {DEPTH}, box diagonal {diagonal:.4g}\n")
    r = renderer_of(entry, 8)
    image, trace_ms = render(r, cam, w, h)
    image, trace_ms = render(r, cam, w, h)    # the second frame: the autotuner has seen the batches
    o = torch.empty_like(image)
    t, lo, hi = three_medians(lambda: r.denoise(image, image_out=o), reps)
    wr(f"   S = 8: the frame's traces {trace_ms:.3f} ms; Renderer.denoise (features + 5 iterations, the shipped variant) {t:.4f} ms "
       f"({lo:.4f} .. {hi:.4f}) = {100 * t / trace_ms:.1f} % of the traces\n")
    out.flush()
    ref, _ = render(renderer_of(entry, converged), cam, w, h)
    ref = ref[:, :3].double()
    ratios = {}
    for samples in (1, 4, 8):
        rs = renderer_of(entry, samples)
        noisy, _ = render(rs, cam, w, h)
        before = float(((noisy[:, :3].double() - ref) ** 2).mean())
        wr(f"   S = {samples}: MSE against S = {converged} before {before:.6g}; after / before, rows sigma_color, columns sigma_plane "
           f"= diagonal / 50, / 200, / 1000:\n")
        for sc in SIGMA_COLORS:
            row = []
            for frac in PLANE_FRACTIONS:
                rs.denoise(noisy, image_out=o, sigma_color=sc, sigma_plane=diagonal * frac)
                torch.cuda.synchronize()
                after = float(((o[:, :3].double() - ref) ** 2).mean())
                ratios[samples, sc, frac] = after / before
                row.append(f"{after / before:8.4f}")
            wr(f"      {sc:5.2f} {' '.join(row)}\n")
        out.flush()
    return ratios


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="bunny,hairball")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--converged", type=int, default=1024)
    ap.add_argument("--bvh-cache", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "mrt_bvhcache"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "denoise.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("denoise_probe needs a GPU: a time taken anywhere else says nothing")
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda").cpu()   # the device is initialised before anything is timed
    scenes = bench.SceneCache(1, 0, args.bvh_cache)
    names = args.scenes.split(",")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        out.write(f"tools/denoise_probe.py on {torch.cuda.get_device_name(0)}, medians of {args.reps}, three medians: middle (lowest .. highest)\n\n")
        out.write(f"== timing on {names[0]}: per step, t(k + 1 iterations) - t(k iterations) of one mrt_denoise_filter call\n")
        winners = [timing(scenes.get(names[0]), w, h, max(5, args.reps), out) for w, h in ((640, 480), (1920, 1080))]
        staged = [step for step in (1, 2, 4, 8, 16) if all(dict(ws)[step] == "staged" for ws in winners)]
        out.write(f"   the staged kernel wins at both sizes at steps {staged}\n\n")
        ratios = {}
        for name in names:
            for key, v in share_and_quality(name, scenes.get(name), max(5, args.reps), args.converged, out).items():
                ratios.setdefault(key[1:], []).append(v)
        best = min(ratios, key=lambda k: statistics.mean(ratios[k]))
        out.write(f"\nlowest mean MSE ratio over scenes and S: sigma_color {best[0]}, sigma_plane = diagonal / {1 / best[1]:.0f} "
                  f"(mean {statistics.mean(ratios[best]):.4f}, worst {max(ratios[best]):.4f})\n")


if __name__ == "__main__":
    main()
