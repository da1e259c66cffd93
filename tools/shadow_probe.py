#!/usr/bin/env python3
"""What a shadow batch costs next to an AO batch of the same frame. Writes profiles/shadow.txt (or
--out).

Per scene (--scenes: bunny and one large scene) at 640x480 with 8 and 32 samples, on the current
device, for the frame's first RayGen::batching batch (at most 2^21 rays):
  * generation: DeviceRayGen.shadow next to DeviceRayGen.ao over the same traced primaries and the
    same input range — device events around the call, --reps calls after 5 warm-up calls, the
    median. The bytes a generator must write (32 per ray) over that time, as a share of 8 TB/s:
    the input side (40 bytes per input ray, shared by its S samples) is left out of the floor.
  * any-hit trace: the shadow batch next to the AO batch, each on a Tracer handle of its own (the
    two batches are any-hit, secondary and of one size, so they share the autotuner's key: one
    handle would time both on whichever schedule it settled first), after the autotuner settled —
    three medians of --reps kernel times: the middle one, and their range as the run's spread.
    Rates are in rays of the batch per second; the live rays (tmax >= 0: their primary hit) and
    the blocked share are printed next to them, because a dead ray costs next to nothing and the
    two batches need not be equally hard.
The light sits inside the scene's box (at 0.5, 0.9, 0.9 of its extent) with a radius of 0.1 of the
box's diagonal. These are measurements, not gates.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "gpu-ray-tracing_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from mrt.raygen import DeviceRayGen  # noqa: E402
from mrt.renderer import MAX_BATCH_RAYS  # noqa: E402
from mrt.tracer import Tracer  # noqa: E402

HBM_BYTES_PER_S = 8e12
W, H = 640, 480
SAMPLES = (8, 32)


def event_ms(fn, reps, warmup=5):
    """Median device time of fn() over reps calls after warmup calls; returns (ms, last result)."""
    times, out = [], None
    for k in range(warmup + reps):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        z.record()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(z))
    return statistics.median(times), out


def settle(tracer, rb):
    for _ in range(700):
        tracer.trace_batch(rb)
        if tracer.last_info["autotune_locked"]:
            return True
    return False


def trace_ms(tracer, rb, reps):
    meds = sorted(statistics.median(tracer.trace_batch(rb) for _ in range(reps)) for _ in range(3))
    return meds[1], meds[0], meds[2]


def light_of(scene):
    v, _, _ = scene.arrays()
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    return tuple(float(x) for x in lo + (hi - lo) * np.array([0.5, 0.9, 0.9])), float(0.1 * np.linalg.norm(hi - lo))


def probe(name, scenes, reps, out):
    w = out.write
    e = scenes.get(name)
    scene, gbvh = e["scene"], e["gbvh"]
    cam, ao_radius = scene.camera()
    light, radius = light_of(scene)
    gen = DeviceRayGen(scene)
    base = Tracer(0)
    base.set_bvh(gbvh)
    primary, _ = gen.primary(cam, W, H)
    base.trace_batch(primary, exact_rcp=True)
    hits = gen.count_hits(primary)
    w(f"== {name}: {scene.num_triangles} triangles, {W}x{H}, {hits} of {W * H} primaries hit; light {light} radius {radius:.4g}, "
      f"AO radius {ao_radius:.4g}\n")
    for samples in SAMPLES:
        count = min(primary.size, MAX_BATCH_RAYS // samples)
        n = count * samples
        sh_ms, sh = event_ms(lambda: gen.shadow(primary, samples, light, radius, count=count), reps)
        ao_ms, ao = event_ms(lambda: gen.ao(primary, samples, ao_radius, count=count), reps)
        w(f"   S = {samples:2d}: the first batch, {count} primaries, {n} rays ({32 * n / 1e6:.1f} MB)\n")
        for label, ms in (("shadow", sh_ms), ("ao", ao_ms)):
            w(f"      generate {label:6s} {ms:8.4f} ms  {32 * n / (ms * 1e-3) / 1e12:6.3f} TB/s written = "
              f"{100 * 32 * n / (ms * 1e-3) / HBM_BYTES_PER_S:5.1f} % of 8 TB/s\n")
        w(f"      shadow / ao generation time {sh_ms / ao_ms:.3f}\n")
        rates = {}
        for label, rb in (("shadow", sh), ("ao", ao)):
            tracer = Tracer(0)
            tracer.set_bvh(gbvh)
            locked = settle(tracer, rb)
            t, tlo, thi = trace_ms(tracer, rb, reps)
            live = int((rb.rays[:, 7] >= 0).sum().item())
            blocked = int((rb.results[:, 0] >= 0).sum().item())
            rates[label] = n / t / 1e3
            w(f"      trace {label:6s} {t:8.4f} ms ({tlo:.4f} .. {thi:.4f}: spread {100 * (thi - tlo) / t:.1f} %)  "
              f"{n / t / 1e3:8.1f} Mrays/s; live {live} ({live / t / 1e3:.1f} Mrays/s), blocked {blocked} "
              f"({100 * blocked / max(live, 1):.1f} % of live), schedule {tracer.last_info['autotune_candidate']}"
              f"{'' if locked else ' (not settled)'}\n")
            del tracer
        w(f"      shadow / ao trace rate {rates['shadow'] / rates['ao']:.3f}\n")
        out.flush()
        del sh, ao
    w("\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="bunny,hairball")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bvh-cache", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "mrt_bvhcache"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shadow.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shadow_probe needs a GPU: a time taken anywhere else says nothing")
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda").cpu()   # the device is initialised before anything is timed
    scenes = bench.SceneCache(1, 0, args.bvh_cache)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        out.write(f"tools/shadow_probe.py on {torch.cuda.get_device_name(0)}, default config (wide 1, autotune 1), "
                  f"medians of {args.reps}\n\n")
        for name in args.scenes.split(","):
            probe(name, scenes, max(5, args.reps), out)


if __name__ == "__main__":
    main()
