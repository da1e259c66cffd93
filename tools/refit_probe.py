#!/usr/bin/env python3
"""Cost of a device refit (Tracer.refit) next to the only other route to new vertex
positions — a host SBVH build, an upload and a bind — and what the refit's looser
boxes cost a trace. Writes profiles/refit.txt (or --out).

Per scene (bunny, hairball; --scenes), on the current device:
  * build / upload / bind: mrth_bvh_build, the three buffers to the device, mrt_tracer_bind
    (wall clock, each on its own);
  * refit: events around Tracer.refit with moved vertices, median of --reps after a warm-up
    (the first refit also builds the plan: timed apart);
  * levels, launches, plan bytes (mrt_tracer_refit_info);
  * bytes a refit has to read and write, counted from the tree (below), and the time
    they take at 8 TB/s;
  * the 1024x768 primary batch traced before any refit and after a refit with UNMOVED
    vertices (same Woop rows, looser boxes where the SBVH builder had clipped): median
    kernel ms of --reps launches on the settled schedule, and their ratio.

Bytes counted (R = triangle refs in leaves, N = inner nodes, N + 1 leaves, W = wide nodes):
  leaves  read 64 N (records) + 16 per Woop slot (terminator walk) + 4 R (triIndex) + 12 R
          (triangles) + 36 R (vertices); write 48 R (rows) + 24 (N + 1) (boxes) + 2 N (flags)
  levels  read 4 N (order) + 50 (N - 1) (child record's boxes, flags); write 25 (N - 1)
  wide    read 16 W (map) + 24 per present child; write 24 per present child
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gpu-ray-tracing_amd"))

import torch  # noqa: E402

import mrt  # noqa: E402
from mrt.tracer import GpuBvh, RayBuffer, Tracer, refit_plan  # noqa: E402

HBM_BYTES_PER_S = 8e12


def moved(v):
    lo, hi = v.min(0), v.max(0)
    size = float((hi - lo).max())
    u = (v - lo) / size
    d = np.stack([np.sin(6.0 * u[:, 1] + 1.0), np.cos(5.0 * u[:, 2] + 0.5), np.sin(4.0 * u[:, 0] + 2.0)], 1)
    return (v + np.float32(0.1 * size) * d).astype(np.float32)


def settled_ms(tracer, rb, reps):
    for _ in range(700):
        tracer.trace_batch(rb)
        if tracer.last_info["autotune_locked"]:
            break
    return statistics.median(tracer.trace_batch(rb) for _ in range(reps)), tracer.last_info["autotune_locked"]


def probe(name, reps, out):
    scene = mrt.Scene.synthetic(name, 0, 1)
    v, t, _ = scene.arrays()
    t0 = time.perf_counter()
    bvh = mrt.Bvh.build(scene)
    build_s = time.perf_counter() - t0
    nodes, woop, tri = bvh.buffers()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g = GpuBvh((nodes, woop, tri))
    torch.cuda.synchronize()
    upload_s = time.perf_counter() - t0
    tracer = Tracer(0)
    t0 = time.perf_counter()
    tracer.set_bvh(g)
    bind_s = time.perf_counter() - t0

    cam, _ = scene.camera()
    rays, _ = mrt.primary_rays(cam, 1024, 768)
    rb = RayBuffer(rays, need_closest_hit=True)
    before_ms, locked0 = settled_ms(tracer, rb, reps)
    hits0 = rb.results_numpy()[:, 0].copy()

    dev = g.device
    dv, dv2, dt = (torch.from_numpy(a).to(dev) for a in (v, moved(v), t))
    torch.cuda.synchronize()
    saved = tracer.schedules()
    t0 = time.perf_counter()
    tracer.refit(dv, dt)   # unmoved vertices; builds the plan
    torch.cuda.synchronize()
    first_s = time.perf_counter() - t0
    kept = tracer.schedules() == saved
    after_ms, locked1 = settled_ms(tracer, rb, reps)
    same = int((rb.results_numpy()[:, 0] == hits0).sum())

    for _ in range(3):
        tracer.refit(dv2, dt)
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tracer.refit(dv2, dt)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    refit_ms = statistics.median(times)
    info = tracer.refit_info()

    n_nodes, slots = len(nodes) // 16, len(woop) // 4
    refs = (slots - (n_nodes + 1)) // 3
    _, offsets, src = refit_plan(nodes)
    n_wide, present = len(src) // 4, int((src >= 0).sum())
    leaves_b = 64 * n_nodes + 16 * slots + (4 + 12 + 36) * refs + 48 * refs + 24 * (n_nodes + 1) + 2 * n_nodes
    levels_b = 4 * n_nodes + 75 * (n_nodes - 1)
    wide_b = 16 * n_wide + 48 * present
    total_b = leaves_b + levels_b + wide_b
    floor_ms = total_b / HBM_BYTES_PER_S * 1e3
    big = int((np.diff(offsets)[1:] > 1024).sum())

    w = out.write
    w(f"== {name}: {len(t)} triangles, {refs} refs in {n_nodes + 1} leaves, {n_nodes} inner nodes, {n_wide} wide nodes\n")
    w(f"   buffers {nodes.nbytes + woop.nbytes + tri.nbytes} B (nodes {nodes.nbytes}, woop {woop.nbytes}, triIndex {tri.nbytes})\n")
    w(f"   refit              {refit_ms:9.3f} ms  (median of {reps}, min {min(times):.3f}, max {max(times):.3f}; events around the call)\n")
    w(f"   first refit        {first_s * 1e3:9.1f} ms  (wall; builds the plan: nodes to the host, levels, uploads)\n")
    w(f"   levels {info['levels']}, launches {info['launches']} (1 leaves + {big} big levels + 1 tail + 1 wide), "
      f"plan {info['plan_bytes']} B, skipped {info['skipped_refs']}\n")
    w(f"   bytes read+written {total_b} (leaves {leaves_b}, levels {levels_b}, wide {wide_b}): "
      f"{floor_ms:.4f} ms at 8 TB/s, refit / that = {refit_ms / floor_ms:.1f}x\n")
    w(f"   rebuild route      build {build_s * 1e3:9.1f} ms + upload {upload_s * 1e3:7.1f} ms + bind {bind_s * 1e3:8.1f} ms "
      f"= {(build_s + upload_s + bind_s) * 1e3:.1f} ms (and the autotuner's schedules are forgotten)\n")
    w(f"   refit vs rebuild   {(build_s + upload_s + bind_s) * 1e3 / refit_ms:.0f}x\n")
    w(f"   trace 1024x768 primary: before {before_ms:.4f} ms (locked {locked0}), after a refit with unmoved vertices "
      f"{after_ms:.4f} ms (locked {locked1}); after / before = {after_ms / before_ms:.3f}; same hit ids {same} of {len(hits0)}\n")
    w(f"   schedules kept across the refit: {kept} ({len(saved)} settled)\n\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="bunny,hairball")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "refit.txt"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda").cpu()   # the device is initialised before anything is timed
    with open(args.out, "w") as out:
        out.write(f"tools/refit_probe.py on {torch.cuda.get_device_name(0)}, default config (wide 1, autotune 1)\n\n")
        for name in args.scenes.split(","):
            probe(name, max(10, args.reps), out)


if __name__ == "__main__":
    main()
