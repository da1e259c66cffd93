#!/usr/bin/env python3
"""What the temporal accumulation of path frames costs, which of its two launch shapes is faster,
how much nearer the converged frame it brings a sequence of one-sample frames, and which settings
do that best. Writes profiles/temporal.txt (or --out).

On the current device, with tools/denoise_probe.py's protocol (device events round the call, 5
warm-up calls, the median of --reps calls, three such medians: their middle and their range):
  * timing, per scene at 640x480 and 1920x1080 (a real path frame's image, guide and history, the
    second frame of a static camera, so every hit reprojects 1:1): mrt_temporal_motion;
    mrt_temporal_accumulate in the linear (variant 1) and the tiled (variant 2) shape, with and
    without prevPosition; each against its compulsory bytes at 8 TB/s (accumulate: 112 read and 36
    written per pixel, 16 more read with prevPosition; motion: 52 read and 16 written per slot) and
    against one launch of the filter (mrt_denoise_filter, 1 iteration) measured in the same run. A
    shape wins where it is faster by more than the larger of the two ranges. The features call is
    timed too: Renderer.accumulate and Renderer.denoise each compute the frame's guide.
  * quality, per scene at 640x480, depth 4: the MSE of the float image (r, g, b over all pixels)
    against a converged frame of the sequence's last camera and vertices (S = --converged), for 8
    accumulated frames of S = 1 against the last frame alone, over
      static          the scene's camera (also against one frame of S = 8)
      pan 1, 4, 16    the camera turned by about that many pixels per frame
      moving          a set_vertices displacement growing to 2 % of the box per sequence
                      (tools/animate_probe.py's), with and without prev_vertices
    each also followed by Renderer.denoise's filter; the share of hit pixels that found history and
    the mean history length of the last frame.
  * defaults: the same sequences over max_history in {8, 32, 128}, normal_cos in {0.8, 0.9, 0.98}
    and the plane tolerance in {1/50, 1/200, 1/1000} of the box's diagonal; DESIGN section 16's rule:
    the lowest mean ratio among the settings that made no sequence worse than its last frame alone.
These are measurements, not gates; the defaults (mrt.temporal, csrc/temporal_limits.hpp's
kDefaultTiled) are set from them by hand.
"""
from __future__ import annotations

import argparse
import ctypes as C
import itertools
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "gpu-ray-tracing_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import mrt  # noqa: E402
from mrt import _lib  # noqa: E402
from mrt.denoise import Denoiser  # noqa: E402
from mrt.raygen import RAY_PATH  # noqa: E402
from mrt.renderer import GlibcRand, Renderer  # noqa: E402
from mrt.temporal import (MAX_HISTORY_DEFAULT, NORMAL_COS_DEFAULT, SIGMA_PLANE_FRACTION_DEFAULT, TemporalAccumulator,  # noqa: E402
                          world_to_screen)
from mrt.tracer import Tracer  # noqa: E402

HBM_BYTES_PER_S = 8e12
DEPTH, FRAMES = 4, 8
MAX_HISTORIES, NORMAL_COSINES, PLANE_FRACTIONS = [8, 32, 128], [0.8, 0.9, 0.98], [1 / 50, 1 / 200, 1 / 1000]
DEFAULT = (MAX_HISTORY_DEFAULT, NORMAL_COS_DEFAULT, SIGMA_PLANE_FRACTION_DEFAULT)


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


def box_of(v):
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    return lo, hi, float(np.linalg.norm(hi - lo))


def displaced(v, amplitude):      # tools/animate_probe.py's
    lo, hi = v.min(axis=0), v.max(axis=0)
    size = float((hi - lo).max())
    phase = (v[:, [1, 2, 0]] - lo[[1, 2, 0]]) / np.float32(size) * np.float32(2 * np.pi)
    return np.ascontiguousarray(v + np.float32(amplitude * size) * np.sin(phase), np.float32)   # row-major whatever the index made


def renderer_of(entry, samples):
    scene = entry["scene"]
    tracer = Tracer(0)
    tracer.set_bvh(entry["gbvh"])
    lo, hi, diagonal = box_of(scene.arrays()[0])
    r = Renderer(tracer, scene, rand=GlibcRand())
    r.set_params(RAY_PATH, samples, depth=DEPTH, light_pos=tuple(float(x) for x in lo + (hi - lo) * np.array([0.5, 0.9, 0.9])),
                 light_radius=0.1 * diagonal)
    return r


def render(r, cam, w, h):
    r.begin_frame(cam, w, h)
    px = torch.zeros(w * h, dtype=torch.int32, device=r.gen.device)
    img = torch.zeros((w * h, 4), dtype=torch.float32, device=r.gen.device)
    while r.next_batch():
        r.trace_batch()
        r.update_result(px, img)
    return img


def turned(cam, angle):
    f, up = np.asarray(cam.forward, np.float64), np.asarray(cam.up, np.float64)
    f = f / np.linalg.norm(f)
    side = np.cross(f, up / np.linalg.norm(up))
    g = f * np.cos(angle) + side * np.sin(angle)
    return mrt.Camera(cam.position, tuple(float(x) for x in g), cam.up, cam.fov, cam.near, cam.far)


def mse(a, ref):
    return float(((a[:, :3].double() - ref) ** 2).mean())


# ---- timing ------------------------------------------------------------------------------------------------------------
def timing(name, entry, w, h, reps, out):
    wr = out.write
    scene = entry["scene"]
    cam, _ = scene.camera()
    r = renderer_of(entry, 1)
    dev, n = r.gen.device, w * h
    acc = TemporalAccumulator(dev)
    matrix = world_to_screen(cam, w, h)
    v = torch.from_numpy(scene.arrays()[0]).to(dev)
    tri = torch.from_numpy(scene.arrays()[1]).to(dev)
    sigma = box_of(scene.arrays()[0])[2] * SIGMA_PLANE_FRACTION_DEFAULT
    for _ in range(2):      # the second frame has a previous one; zero motion through prevPosition
        image = render(r, cam, w, h)
        acc.accumulate(r.primary, r.slot_to_id, r.gen.normals, r._recon.material, w, h, matrix, (0.5, 0.5), image,
                       triangles=tri, vertices=v, prev_vertices=v, sigma_plane=sigma)
    torch.cuda.synchronize()
    lib, stream = _lib.trace_lib(), torch.cuda.current_stream().cuda_stream or None
    cur, prev = acc.sets[acc._cur], acc.sets[1 - acc._cur]     # write the set that is not the last frame's
    slots = r.primary.size

    def motion():
        _lib.check(lib.mrt_temporal_motion(slots, r.slot_to_id.data_ptr(), r.primary.rays.data_ptr(), r.primary.results.data_ptr(),
                                           tri.data_ptr(), tri.shape[0], v.data_ptr(), v.data_ptr(), v.shape[0], n,
                                           acc.prev_position.data_ptr(), stream))
    t, lo, hi = three_medians(motion, reps)
    moved = slots * 68
    wr(f"   {name} {w}x{h}: motion {t:.4f} ms ({lo:.4f} .. {hi:.4f}); {moved / 1e6:.1f} MB compulsory = "
       f"{100 * moved / (t * 1e-3) / HBM_BYTES_PER_S:.1f} % of 8 TB/s\n")
    o, px = torch.empty_like(image), torch.empty(n, dtype=torch.int32, device=dev)

    def accumulate(variant, with_position):
        p = _lib.TemporalParams()
        p.width, p.height, p.havePrev, p.maxHistory, p.variant = w, h, 1, MAX_HISTORY_DEFAULT, variant
        p.normalCos, p.sigmaPlane = NORMAL_COS_DEFAULT, sigma
        for i in range(16):
            p.prevWorldToScreen[i] = float(matrix[i])
        p.prevSubpixel[0] = p.prevSubpixel[1] = 0.5
        p.image, p.guide, p.albedo = image.data_ptr(), prev["guide"].data_ptr(), prev["albedo"].data_ptr()
        p.prevPosition = acc.prev_position.data_ptr() if with_position else None
        p.prevGuide, p.prevHistory = prev["guide"].data_ptr(), prev["history"].data_ptr()
        p.history, p.imageOut, p.pixels = cur["history"].data_ptr(), o.data_ptr(), px.data_ptr()
        return lambda: _lib.check(lib.mrt_temporal_accumulate(C.byref(p), stream))
    dn = Denoiser(dev)

    def features():
        dn.set_frame(r.primary, r.slot_to_id, r.gen.normals, r._recon.material, w, h)
    tf, flo, fhi = three_medians(features, reps)
    q = _lib.DenoiseParams()
    q.width, q.height, q.iterations, q.normalSquarings, q.sigmaColor, q.sigmaPlane = w, h, 1, 7, 0.5, sigma
    q.image, q.guide, q.albedo, q.imageOut, q.pixels = image.data_ptr(), dn.guide.data_ptr(), dn.albedo.data_ptr(), o.data_ptr(), px.data_ptr()
    ts, slo, shi = three_medians(lambda: _lib.check(lib.mrt_denoise_filter(C.byref(q), stream)), reps)
    wr(f"      the filter's step-1 launch {ts:.4f} ms ({slo:.4f} .. {shi:.4f}); features {tf:.4f} ms ({flo:.4f} .. {fhi:.4f}), "
       f"computed by accumulate and again by denoise\n")
    verdicts = []
    for with_position in (False, True):
        (tl, llo, lhi), (tt, tlo, thi) = (three_medians(accumulate(variant, with_position), reps) for variant in (1, 2))
        byts = n * (148 + (16 if with_position else 0))
        spread = max(lhi - llo, thi - tlo)
        verdict = "tiled" if tl - tt > spread else ("linear" if tt - tl > spread else "neither (within the range)")
        verdicts.append(verdict)
        wr(f"      accumulate {'with' if with_position else 'without'} prevPosition: linear {tl:.4f} ms ({llo:.4f} .. {lhi:.4f}) = "
           f"{100 * byts / (tl * 1e-3) / HBM_BYTES_PER_S:.1f} % of 8 TB/s, {tl / ts:.2f} x the filter launch; tiled {tt:.4f} ms "
           f"({tlo:.4f} .. {thi:.4f}) = {100 * byts / (tt * 1e-3) / HBM_BYTES_PER_S:.1f} %, {tt / ts:.2f} x; {verdict}: "
           f"linear - tiled = {tl - tt:+.4f} ms, range {spread:.4f}\n")
    out.flush()
    return verdicts


# ---- quality -----------------------------------------------------------------------------------------------------------
def sequences(cam, h):
    per_pixel = np.radians(cam.fov) / h
    yield "static", [cam] * FRAMES, None
    for pixels in (1, 4, 16):
        yield f"pan {pixels}", [turned(cam, per_pixel * pixels * (k - (FRAMES - 1))) for k in range(FRAMES)], None
    yield "moving, followed", [cam] * FRAMES, True
    yield "moving, not followed", [cam] * FRAMES, False


def quality(name, entry, converged, out):
    wr = out.write
    scene = entry["scene"]
    cam, _ = scene.camera()
    w, h = 640, 480
    v0, tris, _ = scene.arrays()
    diagonal = box_of(v0)[2]
    settings = [DEFAULT] + [s for s in itertools.product(MAX_HISTORIES, NORMAL_COSINES, PLANE_FRACTIONS) if s != DEFAULT]
    wr(f"== {name}: {scene.num_triangles} triangles, {w}x{h}, depth {DEPTH}, box diagonal {diagonal:.4g}; {FRAMES} frames of S = 1 "
       f"against S = {converged}\n")
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
        accs = [TemporalAccumulator(dev) for _ in settings]
        tri = torch.from_numpy(tris).to(dev)
        o = torch.empty((w * h, 4), dtype=torch.float32, device=dev)
        previous = torch.from_numpy(v0).to(dev)
        for k in range(FRAMES):
            current = previous
            if moving:
                current = torch.from_numpy(steps[k]).to(dev)
                r.set_vertices(current)
            image = render(r, cams[k], w, h)
            matrix = world_to_screen(cams[k], w, h)
            motion = dict(triangles=tri, vertices=current, prev_vertices=previous) if follow and k else {}
            for acc, (max_history, normal_cos, fraction) in zip(accs, settings):
                acc.accumulate(r.primary, r.slot_to_id, r.gen.normals, r._recon.material, w, h, matrix, (0.5, 0.5), image, image_out=o,
                               max_history=max_history, normal_cos=normal_cos, sigma_plane=diagonal * fraction, **motion)
                if k == FRAMES - 1:
                    torch.cuda.synchronize()
                    if (max_history, normal_cos, fraction) == DEFAULT:
                        blended = o.clone()
                    ratios.setdefault((max_history, normal_cos, fraction), {})[label] = mse(o, ref)
            previous = current
        single = mse(image, ref)
        for key in ratios:
            ratios[key][label] /= single
        hit = accs[0].current["guide"][:, 3] != 0
        length = accs[0].history_length()[hit]
        # the defaults' last frame, through the filter, against the last frame alone through the filter
        dn_single, dn_blend = torch.empty_like(o), torch.empty_like(o)
        r.denoise(image, image_out=dn_single)
        r.denoise(blended, image_out=dn_blend)
        torch.cuda.synchronize()
        line = (f"   {label:22s} last frame alone {single:.6g}; accumulated (defaults) / alone {ratios[DEFAULT][label]:.4f}; "
                f"hits with history {float((length > 1).float().mean()):.3f}, mean length {float(length.mean()):.2f}; "
                f"denoised alone {mse(dn_single, ref):.6g}, accumulated then denoised {mse(dn_blend, ref):.6g}")
        if label == "static":
            eight = render(renderer_of(entry, 8), cam, w, h)
            line += f"; one frame of S = 8: {mse(eight, ref) / single:.4f} of S = 1"
        wr(line + "\n")
        out.flush()
        del accs
        torch.cuda.empty_cache()
    return ratios


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="bunny,hairball")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--converged", type=int, default=1024)
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--bvh-cache", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "mrt_bvhcache"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "temporal.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("temporal_probe needs a GPU: a time taken anywhere else says nothing")
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda").cpu()   # the device is initialised before anything is timed
    scenes = bench.SceneCache(1, 0, args.bvh_cache)
    names = args.scenes.split(",")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        out.write(f"tools/temporal_probe.py on {torch.cuda.get_device_name(0)}, medians of {args.reps}, three medians: middle (lowest .. highest)\n\n")
        out.write("== timing: the second frame of a static camera (every hit reprojects 1:1)\n")
        verdicts = []
        for name in names:
            for w, h in ((640, 480), (1920, 1080)):
                verdicts += timing(name, scenes.get(name), w, h, max(5, args.reps), out)
        shape = "tiled" if all(v == "tiled" for v in verdicts) else "linear"
        out.write(f"   verdicts {verdicts}: variant 0 should be the {shape} shape (the linear one unless the tiled one wins everywhere)\n\n")
        if args.skip_quality:
            return
        table = {}
        for name in names:
            for key, per in quality(name, scenes.get(name), args.converged, out).items():
                for label, ratio in per.items():
                    table.setdefault(key, {})[f"{name} {label}"] = ratio
        out.write("\n== defaults: accumulated / last frame alone per setting (max_history, normal_cos, plane fraction): mean, worst\n")
        for key, per in sorted(table.items(), key=lambda kv: statistics.mean(kv[1].values())):
            out.write(f"   {key[0]:4d} {key[1]:.2f} 1/{1 / key[2]:<5.0f} mean {statistics.mean(per.values()):.4f} worst {max(per.values()):.4f}"
                      f"{'   <- shipped' if key == DEFAULT else ''}\n")
        ok = {k: per for k, per in table.items() if max(per.values()) <= 1.0}
        if ok:
            best = min(ok, key=lambda k: statistics.mean(ok[k].values()))
            out.write(f"lowest mean ratio among the {len(ok)} settings that made no sequence worse: max_history {best[0]}, normal_cos {best[1]}, "
                      f"plane fraction 1/{1 / best[2]:.0f} (mean {statistics.mean(ok[best].values()):.4f})\n")
        else:
            out.write("no setting left every sequence no worse than its last frame alone: the most conservative one ships "
                      "(max_history 8, normal_cos 0.98, plane fraction 1/1000)\n")


if __name__ == "__main__":
    main()
