#!/usr/bin/env python3
"""What keeping a moving scene on the device costs, and whether the tree's cost tells when a
refitted tree should be rebuilt. Writes profiles/animate.txt (or --out).

Per scene (bunny, hairball; --scenes), on the current device, the vertices displaced by a smooth
field (a sine of the other coordinates, one period over the scene) of amplitude 0, 2, 5, 10 and
20 % of the scene's largest extent. Per step, all legs in one run:
  * mrt_scene_attributes (normals, shaded and material colours; device ms by events, median of
    --calls calls) and the distinct bytes it touches over that time (12 per vertex read once; per
    triangle 12 index + 16 diffuse read, 12 + 4 + 4 written; the calls repeat on the same
    buffers, so whatever fits the caches stays there), against the host route: the vertices copied back,
    mrth_scene_attributes, the three tables uploaded (wall ms, median of 3);
  * mrt_tracer_tree_cost: wall ms of the blocking form (one readback) and device ms of the
    stream-ordered form;
  * the SAH cost (Cn = Ct = 1) of the device LBVH of the undisplaced vertices refitted to the
    displaced ones, over that of a fresh device build of the displaced ones;
  * the 1024x768 primary batch on the refitted tree and on the rebuilt tree: each tracer on the
    schedule its autotuner settled on that tree, medians of --reps launches, the two legs
    alternating --rounds times, the median of the legs' medians; the rebuild's wall ms
    (mrt_tracer_build_info) and the primary batches after which it has paid for itself.
No ratio is assumed to separate anything: the table is what was measured.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gpu-ray-tracing_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mrt  # noqa: E402
import mrt.host  # noqa: E402
from mrt.raygen import scene_attributes  # noqa: E402
from mrt.tracer import RayBuffer, Tracer  # noqa: E402

AMPLITUDES = (0.0, 0.02, 0.05, 0.10, 0.20)
BYTES_PER_TRIANGLE, BYTES_PER_VERTEX = 12 + 16 + 12 + 4 + 4, 12


def displaced(v, amplitude):
    lo, hi = v.min(axis=0), v.max(axis=0)
    size = float((hi - lo).max())
    phase = (v[:, [1, 2, 0]] - lo[[1, 2, 0]]) / np.float32(size) * np.float32(2 * np.pi)
    return (v + np.float32(amplitude * size) * np.sin(phase)).astype(np.float32)


def settle(tracer, rb):
    for _ in range(700):
        tracer.trace_batch(rb)
        if tracer.last_info["autotune_locked"]:
            break


def event_ms(fn, calls):
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def wall_ms(fn, calls):
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def probe(name, reps, rounds, calls, out):
    w = out.write
    dev = torch.device("cuda", 0)
    scene = mrt.Scene.synthetic(name, 0, 1)
    v, t, _ = scene.arrays()
    nt = len(t)
    cam, _ = scene.camera()
    rays, _ = mrt.primary_rays(cam, 1024, 768)
    dt = torch.from_numpy(t).to(dev)
    dv = torch.from_numpy(v).to(dev)
    diffuse = scene.tri_diffuse()
    dd = torch.from_numpy(diffuse).to(dev)
    normals = torch.empty((nt, 3), dtype=torch.float32, device=dev)
    shaded = torch.empty(nt, dtype=torch.int32, device=dev)
    material = torch.empty(nt, dtype=torch.int32, device=dev)
    refit_tracer, fresh_tracer = Tracer(0), Tracer(0)
    rb_refit, rb_fresh = RayBuffer(rays, need_closest_hit=True), RayBuffer(rays, need_closest_hit=True)
    w(f"== {name}: {nt} triangles, {len(v)} vertices; device LBVH, max_leaf_size 4\n")
    w("   step   attributes: device ms (GB/s) | host route ms   tree_cost: blocking ms | device ms   "
      "SAH refitted / rebuilt = ratio   trace ms: refitted | rebuilt = ratio   rebuild ms (batches to pay)\n")
    for amplitude in AMPLITUDES:
        v2 = displaced(v, amplitude)
        dv2 = torch.from_numpy(v2).to(dev)

        attr_ms = event_ms(lambda: scene_attributes(dv2, dt, dd, normals, shaded, material), calls)

        def host_route():
            back = dv2.cpu().numpy()
            a = mrt.host.scene_attributes(back, t, diffuse)
            return [torch.from_numpy(a[k].view(np.int32) if k != "normals" else a[k]).to(dev)
                    for k in ("normals", "shaded", "material")]
        host_ms = wall_ms(host_route, 3)

        refit_tracer.build(dv, dt, max_leaf_size=4, on_device=True)
        refit_tracer.refit(dv2, dt)
        fresh_tracer.build(dv2, dt, max_leaf_size=4, on_device=True)
        build_ms = fresh_tracer.build_info()["wall_ms"]
        cost_wall = wall_ms(lambda: refit_tracer.tree_cost(), calls)
        cost_dev = event_ms(lambda: refit_tracer.tree_cost(sync=False), calls)
        sah_refit, sah_fresh = refit_tracer.tree_cost()["sah"], fresh_tracer.tree_cost()["sah"]

        settle(refit_tracer, rb_refit)
        settle(fresh_tracer, rb_fresh)
        legs_refit, legs_fresh = [], []
        for _ in range(rounds):
            legs_refit.append(statistics.median(refit_tracer.trace_batch(rb_refit) for _ in range(reps)))
            legs_fresh.append(statistics.median(fresh_tracer.trace_batch(rb_fresh) for _ in range(reps)))
        ms_refit, ms_fresh = statistics.median(legs_refit), statistics.median(legs_fresh)
        pays = f"{build_ms / (ms_refit - ms_fresh):.0f}" if ms_refit > ms_fresh else "never"
        w(f"   {100 * amplitude:4.0f} %   {attr_ms:8.4f} ({(nt * BYTES_PER_TRIANGLE + len(v) * BYTES_PER_VERTEX) / attr_ms / 1e6:7.1f}) | {host_ms:9.2f}   "
          f"{cost_wall:8.4f} | {cost_dev:8.4f}   {sah_refit:10.3f} / {sah_fresh:10.3f} = {sah_refit / sah_fresh:6.3f}   "
          f"{ms_refit:8.4f} | {ms_fresh:8.4f} = {ms_refit / ms_fresh:6.3f}   {build_ms:7.2f} ({pays})\n")
        out.flush()
        print(f"{name} {amplitude}: done", flush=True)
    w("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="bunny,hairball")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "animate.txt"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda").cpu()   # the device is initialised before anything is timed
    with open(args.out, "w") as out:
        out.write(f"tools/animate_probe.py on {torch.cuda.get_device_name(0)}, default config (wide 1, autotune 1)\n\n")
        for name in args.scenes.split(","):
            probe(name, max(10, args.reps), max(1, args.rounds), max(3, args.calls), out)


if __name__ == "__main__":
    main()
