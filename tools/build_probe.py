#!/usr/bin/env python3
"""Cost of a device LBVH build (Tracer.build) next to the route it replaces — a host SBVH
build, an upload and a bind — and what the LBVH's lower quality costs a trace. Writes
profiles/build.txt (or --out).

Per scene (bunny, hairball; --scenes), on the current device:
  * the SBVH route: mrth_bvh_build, the three buffers to the device, mrt_tracer_bind (wall
    clock, each on its own), and the 1024x768 primary batch on that tree: median kernel ms of
    --reps launches on the settled schedule;
  * per max_leaf_size 1, 2, 4, 8 the device build with the vertices and triangles already on
    the device, after one untimed build: the call's wall ms (median of --builds calls, the
    phases of that call), the event-timed device phases (keys + sort, hierarchy + emission,
    boxes + rows), the host plan and the bind, records / leaves / levels / scratch, and the
    same primary batch on the built tree with its ratio to the SBVH's;
  * both routes of the derived data side by side (--routes-out, profiles/device_bind.txt): the
    host route (mrt_tracer_bind / mrt_tracer_build: level plan and 4-wide collapse on the CPU) and
    the device route (mrt_tracer_bind_device / mrt_tracer_build_device, csrc/wide_kernel.hip) for
    the bind of the SBVH, the build at the default leaf size, the bind of that built tree and the
    first refit after either bind: wall ms (median of --builds), the phases, the launch and
    readback counts, and the primary batch on the array either route derived.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gpu-ray-tracing_amd"))

import torch  # noqa: E402

import mrt  # noqa: E402
from mrt.tracer import GpuBvh, RayBuffer, Tracer  # noqa: E402

LEAF_SIZES = (1, 2, 4, 8)


def settled_ms(tracer, rb, reps):
    for _ in range(700):
        tracer.trace_batch(rb)
        if tracer.last_info["autotune_locked"]:
            break
    return statistics.median(tracer.trace_batch(rb) for _ in range(reps)), tracer.last_info["autotune_locked"]


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median_of(builds, fn):
    """(median wall ms, what fn returned on that call)."""
    runs = []
    for _ in range(builds):
        box = []
        runs.append((wall_ms(lambda: box.append(fn())), box[0]))
    return sorted(runs, key=lambda r: r[0])[len(runs) // 2]


def derive_line(d):
    return (f"plan/wide on device {d['on_device_plan']}/{d['on_device_wide']}, {d['launches']} launches, "
            f"{d['readbacks']} readbacks, {d['depth_levels']} depth levels, device topology {d['topo_ms']:.3f} + "
            f"collapse {d['collapse_ms']:.3f} + emission {d['emit_ms']:.3f} ms, scratch {d['scratch_bytes']} B")


def bind_routes(tracer, label, g, dv, dt, rb, reps, builds, w):
    """Bind, first refit and trace of one tree on both routes."""
    trace = {}
    for route, on_device in (("host", False), ("device", True)):
        ms, _ = median_of(builds, lambda: tracer.set_bvh(g, on_device=on_device))
        info, d = tracer.bind_info(), tracer.derive_info()
        w(f"   {label} bind, {route:6s} route   wall {ms:9.3f} ms; wide {info['wide_bytes']} B, stack bound "
          f"{info['stack_bound']}\n")
        if on_device:
            w(f"        {derive_line(d)}\n")
        wide = tracer.wide_nodes()
        try:
            trace[route] = settled_ms(tracer, rb, reps)
        except mrt._lib.MrtError as e:
            trace[route] = (float("nan"), str(e))
        trace[route] += (wide,)
    same = bool((trace["host"][2] == trace["device"][2]).all()) if trace["host"][2].shape == trace["device"][2].shape else False
    w(f"        trace 1024x768 primary: host route {trace['host'][0]:.4f} ms, device route {trace['device'][0]:.4f} ms; "
      f"the two wide arrays are {'the same bytes' if same else 'DIFFERENT'}\n")
    # the first refit after either bind, after the traces: a refit of an SBVH loosens its boxes in place
    for route, on_device in (("host", False), ("device", True)):
        tracer.set_bvh(g, on_device=on_device)
        first = wall_ms(lambda: tracer.refit(dv, dt))
        again = statistics.median(wall_ms(lambda: tracer.refit(dv, dt)) for _ in range(5))
        r, d = tracer.refit_info(), tracer.derive_info()
        w(f"   {label} first refit after the {route} bind {first:9.3f} ms, later refits {again:.3f} ms ({r['launches']} "
          f"launches, {r['levels']} levels); its plan: "
          f"{'installed by the bind' if on_device else derive_line(d) if d['on_device_plan'] else 'made on the host'}\n")


def build_routes(tracer, dv, dt, builds, w):
    for route, on_device in (("host", False), ("device", True)):
        tracer.build(dv, dt, on_device=on_device)   # untimed
        ms, info = median_of(builds, lambda: (tracer.build(dv, dt, on_device=on_device), tracer.build_info())[1])
        dev_ms = info["sort_ms"] + info["emit_ms"] + info["fit_ms"]
        w(f"   LBVH build L=4, {route:6s} route   wall {ms:9.3f} ms (the call's own {info['wall_ms']:.3f}) = device "
          f"build {dev_ms:.3f} + plan {info['plan_ms']:.3f} + bind {info['bind_ms']:.3f} + rest; records "
          f"{info['records']}, levels {info['levels']}\n")
        if on_device:
            w(f"        {derive_line(tracer.derive_info())}\n")


def probe(name, reps, builds, out, routes=None):
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
    route_ms = (build_s + upload_s + bind_s) * 1e3

    cam, _ = scene.camera()
    rays, _ = mrt.primary_rays(cam, 1024, 768)
    rb = RayBuffer(rays, need_closest_hit=True)
    sbvh_ms, locked = settled_ms(tracer, rb, reps)
    hits0 = rb.results_numpy()[:, 0].copy()

    w = out.write
    w(f"== {name}: {len(t)} triangles, {len(v)} vertices\n")
    w(f"   SBVH route         build {build_s * 1e3:9.1f} ms + upload {upload_s * 1e3:7.1f} ms + bind {bind_s * 1e3:8.1f} ms "
      f"= {route_ms:.1f} ms; {len(nodes) // 16} records, {nodes.nbytes + woop.nbytes + tri.nbytes} B\n")
    w(f"   SBVH trace 1024x768 primary {sbvh_ms:.4f} ms (locked {locked})\n")

    dev = g.device
    dv, dt = torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev)
    if routes is not None:
        r = routes.write
        r(f"== {name}: {len(t)} triangles, {len(v)} vertices; SBVH {len(nodes) // 16} records\n")
        bind_routes(tracer, "SBVH", g, dv, dt, rb, reps, builds, r)
        build_routes(tracer, dv, dt, builds, r)
        lbvh = tracer.build(dv, dt)
        bind_routes(tracer, "LBVH", lbvh, dv, dt, rb, reps, builds, r)
        r("\n")
        routes.flush()
        del lbvh
    del g
    tracer.build(dv, dt)   # untimed: the first call loads the build's code objects
    for leaf in LEAF_SIZES:
        infos = []
        for _ in range(builds):
            tracer.build(dv, dt, max_leaf_size=leaf)
            infos.append(tracer.build_info())
        info = sorted(infos, key=lambda i: i["wall_ms"])[len(infos) // 2]
        try:
            lbvh_ms, locked = settled_ms(tracer, rb, reps)
        except mrt._lib.MrtError as e:   # a tree too deep for the traversal stack: recorded, not hidden
            lbvh_ms, locked = float("nan"), str(e)
        same = int((rb.results_numpy()[:, 0] == hits0).sum())
        dev_ms = info["sort_ms"] + info["emit_ms"] + info["fit_ms"]
        w(f"   L={leaf}  build wall {info['wall_ms']:8.2f} ms = device {dev_ms:7.3f} (keys+sort {info['sort_ms']:.3f}, "
          f"hierarchy+emission {info['emit_ms']:.3f}, boxes+rows {info['fit_ms']:.3f}) + host plan {info['plan_ms']:.2f} "
          f"+ bind {info['bind_ms']:.2f} + rest; SBVH route / build = {route_ms / info['wall_ms']:.0f}x\n")
        w(f"        records {info['records']}, leaves {info['leaves']}, levels {info['levels']}, scratch "
          f"{info['scratch_bytes']} B, skipped {info['skipped_refs']}; wall min {min(i['wall_ms'] for i in infos):.2f} "
          f"max {max(i['wall_ms'] for i in infos):.2f} of {builds}\n")
        w(f"        trace 1024x768 primary {lbvh_ms:.4f} ms (locked {locked}); LBVH / SBVH = {lbvh_ms / sbvh_ms:.3f}; "
          f"same hit ids {same} of {len(hits0)}\n")
        out.flush()
    w("\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="bunny,hairball")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--builds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "build.txt"))
    ap.add_argument("--routes-out", default=os.path.join(REPO, "profiles", "device_bind.txt"),
                    help="the host and device routes side by side ('' = skip)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda").cpu()   # the device is initialised before anything is timed
    head = f"tools/build_probe.py on {torch.cuda.get_device_name(0)}, default config (wide 1, autotune 1)\n\n"
    with open(args.out, "w") as out, open(args.routes_out or os.devnull, "w") as routes:
        out.write(head)
        routes.write(head)
        for name in args.scenes.split(","):
            probe(name, max(10, args.reps), max(1, args.builds), out, routes if args.routes_out else None)


if __name__ == "__main__":
    main()
