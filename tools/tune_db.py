"""Builds gpu-ray-tracing_amd/mrt/tuned_schedules.json, the saved autotuner choices the
bench locks at bind (the same schedule every run).

The in-library autotuner ranks candidates from 246-317 launches (csrc/tune.cpp; more with
asynchronous launches in flight: 256-328 measured) interleaved with each other, early in
a process while clocks still ramp; here every candidate is timed in steady state instead: the GPU is warmed first, each candidate is locked in turn
(mrt_tracer_tune_import) and timed over interleaved rounds of back-to-back launches
(HIP events): the eight ray-distribution schedules, each also with every stage-2
modifier (spec_slack 4 / 6, the frontier tail toggled, 16 lane groups), then the two fastest against the
fixed rule again; a challenger replaces the rule only when its median is 3 % faster
(csrc/tune.cpp kTuneMargin).

  python tools/tune_db.py [--workload W ...] [--rounds 5] [--launches 20] [--out PATH]

--backfill sweeps the backfilled static grids instead (cfg.backfill, csrc/launch_plan.cpp), a
dimension the in-library tuner does not explore and saved schedules reach by import only: for
the static schedules, k in {1, 2, 3} rays per lane x a residency cap of {2, 3, 4, 5} workgroups
per CU x tail_lanes in {0, 8, 16} x {no modifier, each stage-2 modifier}, against the persistent
static schedules under the same modifiers and against the schedule saved today. In a backfilled
launch every wave "cannot refill" after its last round, so the frontier tail fires in every wave:
tail_lanes is a first-class knob there. A winner replaces the saved schedule only when its median
is --margin faster, re-timed interleaved with it; tail_lanes 8 is a tracer setting no saved code
carries, so it is reported and never written.

The same sweep covers the one-shot kernels (cfg.oneshot, cfg.deal_block; csrc/deal_common.hpp): every
k = 1 grid at a cap of 4 and 5 workgroups per CU also runs with oneshot = 1 at deal_block 0 (the
contiguous chunks: the same deal as today's kernel, so the difference is the kernel's code alone)
and 10, 11, 12 (block-cyclic over the XCD groups: the deal alone, against deal_block 0). The final
re-times, interleaved with the saved schedule, the best one-shot schedule, today's kernel on that
same schedule, and the one-shot kernel on it at each deal.
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "gpu-ray-tracing_amd"))

MARGIN = 0.03
N_SCHEDULES, STAGE2 = 8, 5


def variant_key(any_hit, exact, lds_stack=16, nodes=1, tail=False, secondary=False):
    """The tuning key (mrt_api.cpp variant_key, csrc/tune.cpp) of a speculative, stats-free launch: variant_key() | 512 for a
    MRT_TRACE_SECONDARY batch."""
    return (int(any_hit) | 2 | (4 if exact else 0) | ({8: 0, 16: 1, 32: 2}[lds_stack] << 4) | (nodes << 6)
            | (256 if tail else 0) | (512 if secondary else 0))


STATIC_SCHEDULES = {0: 20, 5: 16, 6: 12, 1: 8}   # stage-1 schedule: its waves/CU (csrc/tune.cpp tune_candidate)
BACKFILL_K, BACKFILL_CAPS, BACKFILL_TAILS = (1, 2, 3), (2, 3, 4, 5), (0, 8, 16)
ONESHOT_CAPS, ONESHOT_DEALS = (4, 5), (0, 10, 11, 12)
ONESHOT_BIT, DEAL_SHIFT = 1 << 23, 27


def backfill_code(code16, k, cap):
    """mrt_tuned_schedule.candidate: the 16-bit code | k << 16 | cap << 24 (include/mrt.h)."""
    return code16 | (k << 16) | (cap << 24)


def oneshot_code(code, deal):
    """A k = 1 code with the one-shot bit (23) and the deal's block log2 (bits 27-30)."""
    return code | ONESHOT_BIT | (deal << DEAL_SHIFT)


def is_oneshot(c):
    return bool(c & ONESHOT_BIT)


def code_name(c):
    s = f"{c & 0xff}/{(c >> 8) & 0xff}"
    s += f" k{(c >> 16) & 0x7f} cap{(c >> 24) & 7}" if c >> 16 else ""
    return s + (f" oneshot b{(c >> DEAL_SHIFT) & 15}" if is_oneshot(c) else "")


def sweep_backfill(args, wl, tracer, b, store, fingerprint, exact):
    """The --backfill sweep of one workload; returns the candidate written, or None."""
    import torch
    import bench
    from mrt import _lib
    launches = [tracer.launcher(rb, exact_rcp=exact) for rb, _ in b.batches]
    default_tail = tracer.config()["tail_lanes"]

    def keys_now():
        cfg = tracer.config()
        tail = cfg["tail_lanes"] > 0 and cfg["wide"] == 1
        return sorted({(rb.size, variant_key(not rb.need_closest_hit, exact, tail=tail, secondary=rb.secondary))
                       for rb, _ in b.batches})

    def timed(items):
        """items: (tail_lanes, code); interleaved rounds, the median of each."""
        t = {it: [] for it in items}
        for r in range(args.rounds + 1):
            tail_set = None
            for it in items:
                tail, code = it
                if tail != tail_set:
                    tracer.set_config(tail_lanes=tail)
                    tail_set = tail
                tracer.load_schedules([(n, v, code, _lib.MRT_TUNE_VERSION) for n, v in keys_now()])
                for go in launches * 3:
                    go()
                a_, z_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a_.record()
                for _ in range(args.launches):
                    for go in launches:
                        go()
                z_.record()
                torch.cuda.synchronize()
                if r:
                    t[it].append(a_.elapsed_time(z_) / args.launches)
        return {it: float(np.median(v)) for it, v in t.items()}

    try:
        keys = keys_now()
        saved = {(n, v): c for n, v, c, _ in store.entries(fingerprint)}
        incumbent = (default_tail, saved.get(keys[0], 0))
        mods = [None] + list(range(N_SCHEDULES, N_SCHEDULES + STAGE2))
        items = [incumbent]
        for tail in BACKFILL_TAILS:
            for m in mods:
                for sched in STATIC_SCHEDULES:
                    items.append((tail, sched if m is None else m | (sched << 8)))
                for k in BACKFILL_K:
                    for cap in BACKFILL_CAPS:
                        code = backfill_code(1 if m is None else m | (1 << 8), k, cap)
                        items.append((tail, code))
                        if k == 1 and cap in ONESHOT_CAPS:
                            items += [(tail, oneshot_code(code, deal)) for deal in ONESHOT_DEALS]
        items = sorted(set(items))
        s1 = timed(items)
        print(f"{wl} exact={exact}: backfill sweep, ms per launch (tail_lanes, code = locked/schedule k cap); "
              f"saved {code_name(incumbent[1])} {s1[incumbent]:.4f}")
        for tail in BACKFILL_TAILS:
            for k in (0,) + BACKFILL_K:
                row = {it: v for it, v in s1.items()
                       if it[0] == tail and ((it[1] >> 16) & 0x7f) == k and not is_oneshot(it[1])}
                best = sorted(row, key=row.get)[:4]
                print(f"  tail {tail:2d} k {k}: " + "  ".join(f"{code_name(c)}:{row[(t_, c)]:.4f}" for t_, c in best))
            for deal in ONESHOT_DEALS:
                row = {it: v for it, v in s1.items()
                       if it[0] == tail and is_oneshot(it[1]) and (it[1] >> DEAL_SHIFT) & 15 == deal}
                best = sorted(row, key=row.get)[:4]
                print(f"  tail {tail:2d} oneshot b{deal}: " + "  ".join(f"{code_name(c)}:{row[(t_, c)]:.4f}" for t_, c in best))
        for m in mods:   # the k x cap grid of each modifier at the default tail
            for k in BACKFILL_K:
                print(f"  grid mod {m} k {k} tail {default_tail}: " + " ".join(
                    f"cap{cap}:{s1[(default_tail, backfill_code(1 if m is None else m | (1 << 8), k, cap))]:.4f}"
                    for cap in BACKFILL_CAPS))
        # the two fastest of each kind against the saved schedule again, interleaved
        filled = sorted((it for it in s1 if it[1] >> 16 and not is_oneshot(it[1])), key=s1.get)[:2]
        resident = sorted((it for it in s1 if not it[1] >> 16), key=s1.get)[:2]
        # the best one-shot schedule at the default tail (a saved code carries no tail of its own), today's
        # kernel on that schedule, and the one-shot kernel on it at every deal: deal 0 against today's
        # kernel is the code generation alone, the cyclic deals against deal 0 the deal alone
        shots = sorted((it for it in s1 if is_oneshot(it[1]) and it[0] == default_tail), key=s1.get)[:1]
        family = []
        for t_, c in shots:
            plain = c & ~(ONESHOT_BIT | (15 << DEAL_SHIFT))
            family += [(t_, plain)] + [(t_, oneshot_code(plain, deal)) for deal in ONESHOT_DEALS]
        s2 = timed(sorted(set([incumbent] + filled + resident + shots + family)))
        print("  final: " + "  ".join(f"tail {t_} {code_name(c)}:{v:.4f}" for (t_, c), v in sorted(s2.items(), key=lambda kv: kv[1])))
        for t_, c in shots:
            plain = c & ~(ONESHOT_BIT | (15 << DEAL_SHIFT))
            base, shot0 = s2[(t_, plain)], s2[(t_, oneshot_code(plain, 0))]
            print(f"  one-shot on {code_name(plain)}: today's kernel {base:.4f}, one-shot b0 {shot0:.4f} "
                  f"({100 * (base / shot0 - 1):+.1f} % code generation); " + "  ".join(
                      f"b{d} {s2[(t_, oneshot_code(plain, d))]:.4f} ({100 * (shot0 / s2[(t_, oneshot_code(plain, d))] - 1):+.1f} % deal)"
                      for d in ONESHOT_DEALS[1:]))
        writable = [it for it in s2 if it[0] == default_tail]   # a saved code carries no tail_lanes of its own
        best = min(writable, key=s2.get)
        if best != incumbent and s2[best] < (1 - args.margin) * s2[incumbent]:
            tracer.set_config(tail_lanes=default_tail)
            tracer.load_schedules([(n, v, best[1], _lib.MRT_TUNE_VERSION) for n, v in keys_now()])
            store.update(fingerprint, tracer.schedules())
            print(f"  -> {code_name(best[1])} ({bench.schedule_name(best[1] & 0xffff)}), "
                  f"{100 * (s2[incumbent] / s2[best] - 1):.1f} % faster than the saved schedule: written", flush=True)
            return best[1]
        print(f"  -> the saved schedule stays (best {code_name(best[1])} is within {100 * args.margin:.0f} %)", flush=True)
        return None
    finally:
        tracer.set_config(tail_lanes=default_tail)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="append")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--fast-rcp", action="store_true", help="tune the v_rcp_f32 variant too")
    ap.add_argument("--out", default=None)
    ap.add_argument("--out-cells", default=None,
                    help="also write each workload's own choice (JSON: workload -> keys, candidate): two ray types of "
                         "one BVH and batch size share a key in --out, the last tuned wins there")
    ap.add_argument("--margin", type=float, default=MARGIN,
                    help="how much faster (median) a candidate must be to replace the rule (the library's 3 %%)")
    ap.add_argument("--backfill", action="store_true",
                    help="sweep the backfilled static grids (k x residency cap x tail_lanes x modifiers) instead")
    args = ap.parse_args()
    import torch
    import bench
    from mrt import _lib
    from mrt.schedules import DEFAULT_PATH, ScheduleStore
    from mrt.tracer import Tracer
    torch.cuda.set_device(0)
    out = args.out or DEFAULT_PATH
    store = ScheduleStore(out if os.path.exists(out) else "")
    store.path = out
    tracer = Tracer(0)
    scenes = bench.SceneCache(1, 0, os.path.join(os.environ.get("TMPDIR", "/tmp"), "mrt_bvhcache"))
    wls = args.workload or [bench.HEADLINE] + bench.EXTRA_N1
    bench.STORE = None
    cells = {}
    for wl in wls:
        e = scenes.get(bench.workload_spec(wl)[0])
        b = bench.Batches(wl, e["scene"], e["gbvh"], tracer)
        for exact in ([True, False] if args.fast_rcp else [True]):
            if args.backfill:
                chosen = sweep_backfill(args, wl, tracer, b, store, e["gbvh"].fingerprint, exact)
                if chosen is not None:
                    cells[f"{wl}{'' if exact else ':fast'}"] = {"fingerprint": e["gbvh"].fingerprint, "candidate": chosen}
                continue
            launches = [tracer.launcher(rb, exact_rcp=exact) for rb, _ in b.batches]
            cfg = tracer.config()
            tail = cfg["tail_lanes"] > 0 and cfg["wide"] == 1   # the library's with_tail()
            keys = sorted({(rb.size, variant_key(not rb.need_closest_hit, exact, tail=tail, secondary=rb.secondary))
                           for rb, _ in b.batches})

            def lock(code):
                tracer.load_schedules([(n, v, code, _lib.MRT_TUNE_VERSION) for n, v in keys])

            def timed(codes):
                t = {c: [] for c in codes}
                for r in range(args.rounds + 1):
                    for c in codes:
                        lock(c)
                        for go in launches * 3:
                            go()
                        # one event pair around back-to-back launches (an event between
                        # launches fences the caches)
                        a_, z_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a_.record()
                        for _ in range(args.launches):
                            for go in launches:
                                go()
                        z_.record()
                        torch.cuda.synchronize()
                        if r:
                            t[c].append(a_.elapsed_time(z_) / args.launches)
                return {c: float(np.median(v)) for c, v in t.items()}

            # warm the clocks on the rule
            lock(0)
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.5:
                for go in launches:
                    go()
                torch.cuda.synchronize()
            # the candidate equal to the fixed rule (csrc/tune.cpp effective_cfg): the global queue for a
            # BVH above the Infinity Cache, 12 waves/CU up to 3 rays per lane of a 16-wave grid, else 16
            g = e["gbvh"]
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            big = g.node_bytes + g.woop_bytes > bench.MALL_BYTES
            rule_c = 0 if not big else (4 if b.batches[0][0].size <= 3 * cus * 16 * 64 else 3)
            # every schedule, and every schedule with each stage-2 modifier (spec_slack 4, 6, the
            # frontier tail toggled): the in-library tuner only modifies its stage-1 winner, which
            # misses e.g. per-XCD queues without the tail on bunny primary 1024x768
            codes = list(range(N_SCHEDULES)) + [(N_SCHEDULES + k) | (c << 8) for c in range(N_SCHEDULES)
                                                for k in range(STAGE2)]
            s1 = timed(codes)
            best = min(s1, key=s1.get)
            # the two best against each other again (the sweep's medians are one sample each)
            top2 = sorted(s1, key=s1.get)[:2]
            s2 = timed(sorted(set([rule_c] + top2)))
            best2 = min(s2, key=s2.get)
            chosen = best2 if s2[best2] < (1 - args.margin) * s2[rule_c] else rule_c
            lock(chosen)
            store.update(e["gbvh"].fingerprint, tracer.schedules())
            cells[f"{wl}{'' if exact else ':fast'}"] = {"fingerprint": e["gbvh"].fingerprint,
                                                       "keys": [list(k) for k in keys], "candidate": chosen}
            print(f"{wl} exact={exact}: rule {rule_c} {s1[rule_c]:.4f} ms; sweep "
                  + " ".join(f"{c & 0xff}/{c >> 8}:{v:.4f}" for c, v in sorted(s1.items(), key=lambda kv: kv[1])[:6])
                  + "; final " + " ".join(f"{c & 0xff}/{c >> 8}:{v:.4f}" for c, v in s2.items())
                  + f" -> {chosen & 0xff}/{chosen >> 8} ({bench.schedule_name(chosen)})", flush=True)
    store.save(out)
    print(f"wrote {out}")
    if args.out_cells:
        import json
        with open(args.out_cells, "w") as f:
            json.dump({"version": _lib.MRT_TUNE_VERSION, "cells": cells}, f, indent=1)
        print(f"wrote {args.out_cells}")


if __name__ == "__main__":
    main()
