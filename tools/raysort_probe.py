#!/usr/bin/env python3
"""Does sorting a secondary batch by the reference's Morton key (RayBuffer.morton_sort,
mrt_ray_sort) pay for itself? Writes profiles/raysort.txt (or --out).

Per batch (hairball diffuse 640x480 and 1920x1080, sponza diffuse, conference AO; --workloads), on
the current device, every leg in one run on one tree:
  * the batch as generated, traced on its own Tracer handle after the autotuner settled;
  * the batch sorted at drop_levels 0, 8 and 15 and, for the diffuse batches, in both box modes
    (0 = origins and end points, the reference's; 1 = origins only), each traced on a handle of
    its own: a sorted and an unsorted batch of one size share the autotuner's key, so one handle
    would time both on whichever schedule it settled first.
Reported: the sort's time (events around mrt_ray_sort, median of --reps) next to its byte floor
at 8 TB/s, each trace's time (median of --reps kernel times, three such medians: the middle one
and their range), and (sort + sorted trace) / unsorted trace. The unsorted medians' range is the
run-to-run spread: a ratio inside 1 +- that spread is reported as no gain. No speed-up is assumed.

The byte floor counts what the launches must move per ray: the box pass reads the ray (32 B), the
key pass reads it again and writes six words (56), every sort pass gathers a word through the
permutation (4 + 8 read, 8 written) and sorts (word, slot) pairs (12 read, 12 written, once: a
radix sort of more than one digit moves them once per digit), the reorder reads a slot and a ray
and writes a ray and two map entries (76): 164 + 44 * passes bytes.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "gpu-ray-tracing_amd"))

import torch  # noqa: E402

import bench  # noqa: E402
from mrt.tracer import Tracer  # noqa: E402

WORKLOADS = ["hairball-diffuse-640x480", "hairball-diffuse-1920x1080", "sponza-diffuse-640x480", "conference-ao-640x480"]
DROPS = (0, 8, 15)
HBM_BYTES_PER_MS = 8e12 / 1e3


def passes(drop):
    return (6 * (25 - drop) + 63) // 64


def floor_ms(n, drop):
    return n * (164 + 44 * passes(drop)) / HBM_BYTES_PER_MS


def settle(tracer, rb):
    for _ in range(700):
        tracer.trace_batch(rb)
        if tracer.last_info["autotune_locked"]:
            return True
    return False


def trace_ms(tracer, rb, reps):
    """Three medians of reps kernel times: (middle, lowest, highest)."""
    meds = sorted(statistics.median(tracer.trace_batch(rb) for _ in range(reps)) for _ in range(3))
    return meds[1], meds[0], meds[2]


def sort_ms(rb, drop, box, reps):
    times = []
    for _ in range(reps + 3):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = rb.morton_sort(drop_levels=drop, box=box)
        z.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(z))
    return statistics.median(times[3:]), out


def probe(name, scenes, reps, out):
    w = out.write
    e = scenes.get(bench.workload_spec(name)[0])
    base = Tracer(0)
    b = bench.Batches(name, e["scene"], e["gbvh"], base)
    rb = b.batches[0][0]
    n = rb.size
    locked = settle(base, rb)
    u, ulo, uhi = trace_ms(base, rb, reps)
    spread = (uhi - ulo) / u
    sched = base.last_info["autotune_candidate"]
    w(f"== {name}: {n} rays ({b.batches[0][1]} from primary hits), {e['gbvh'].node_bytes // 64} nodes\n")
    w(f"   {'as generated':22s} trace {u:8.4f} ms ({ulo:.4f} .. {uhi:.4f}: spread {100 * spread:.1f} %), "
      f"schedule {sched}{'' if locked else ' (not settled)'}\n")
    # what must not change: a closest hit's t as bits; of an any-hit ray only whether it hit
    ref = rb.results[:, 1].clone() if rb.need_closest_hit else rb.results[:, 0] >= 0
    for box in ((0, 1) if b.kind == "diffuse" else (0,)):
        for drop in DROPS:
            s_ms, (srb, id_to_slot, _) = sort_ms(rb, drop, box, reps)
            tracer = Tracer(0)
            tracer.set_bvh(e["gbvh"])
            locked = settle(tracer, srb)
            t, tlo, thi = trace_ms(tracer, srb, reps)
            back = srb.results[id_to_slot.long()]
            same = bool(torch.equal(back[:, 1] if rb.need_closest_hit else back[:, 0] >= 0, ref))
            ratio = (s_ms + t) / u
            verdict = "gain" if ratio < 1 - spread else ("loss" if ratio > 1 + spread else "no gain (inside the spread)")
            w(f"   box {box} drop_levels {drop:2d}: sort {s_ms:7.4f} ms ({passes(drop)} passes; floor {floor_ms(n, drop):.4f} ms, "
              f"{s_ms / floor_ms(n, drop):.1f} x); trace {t:8.4f} ms ({tlo:.4f} .. {thi:.4f}) = {t / u:.3f} x, schedule "
              f"{tracer.last_info['autotune_candidate']}{'' if locked else ' (not settled)'}; (sort + trace) / unsorted "
              f"{ratio:.3f}: {verdict}; results equal {same}\n")
            out.flush()
            del tracer, srb
    w("\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bvh-cache", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "mrt_bvhcache"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "raysort.txt"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda").cpu()   # the device is initialised before anything is timed
    scenes = bench.SceneCache(1, 0, args.bvh_cache)
    with open(args.out, "w") as out:
        out.write(f"tools/raysort_probe.py on {torch.cuda.get_device_name(0)}, default config (wide 1, autotune 1), "
                  f"medians of {args.reps}\n\n")
        for name in args.workloads.split(","):
            probe(name, scenes, max(5, args.reps), out)


if __name__ == "__main__":
    main()
