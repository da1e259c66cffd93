"""The live-first block order (mrt_shard_blocks, order 1) on the strong-scaling frame's primary
results (hairball 1920x1080, 8 spp = 16.6 M secondary rays), device time by HIP events:

  one-workgroup path   1 024-ray blocks, 16 200 blocks: bench.py's shard_order_ms. Several groups
                       of `reps` launches, so two builds of the library (MRT_LIB_DIR) can be compared
                       against the spread of one build's own groups;
  tiled path           256-ray blocks (64 800 blocks, 4 tiles) and 64-ray blocks (259 200 blocks,
                       16 tiles) against the torch route — mrt.dist.live_block_weights +
                       shard_blocks_device with that priority — the two alternated launch by launch,
                       `reps` launches each after a warm-up; the two lists are compared.

  python tools/shard_order_probe.py [reps] [groups]"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gpu-ray-tracing_amd"))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from mrt import _lib  # noqa: E402
from mrt.dist import live_block_weights, shard_blocks_device  # noqa: E402
from mrt.raygen import RAY_DIFFUSE  # noqa: E402
from mrt.renderer import GlibcRand, Renderer  # noqa: E402
from mrt.tracer import Tracer  # noqa: E402


def timed(fn):
    ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev[0].record()
    out = fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]), out


def summary(ms):
    s = sorted(ms)
    return f"median {s[len(s) // 2]:.4f} min {s[0]:.4f} max {s[-1]:.4f} ms"


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    groups = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    cfg = bench.STRONG
    scenes = bench.SceneCache(1, 0, os.path.join(os.environ.get("TMPDIR", "/tmp"), "mrt_bvhcache"))
    e = scenes.get(cfg["scene"])
    tr = Tracer(0)
    bench.bind(tr, e["gbvh"])
    cam, _ = e["scene"].camera()
    r = Renderer(tr, e["scene"], max_batch=cfg["max_batch"], rand=GlibcRand())
    r.set_params(RAY_DIFFUSE, cfg["spp"])
    r.begin_frame(cam, cfg["w"], cfg["h"])
    spp, n = cfg["spp"], r.primary.size * cfg["spp"]
    hit = float((r.primary.results[:, 0] >= 0).float().mean())
    print(f"library {os.path.relpath(_lib.TRACE_LIB_PATH, REPO)}; {cfg['name']}: {n} rays, "
          f"primary hit fraction {hit:.3f}", flush=True)

    def library(block):
        return r.gen.shard_blocks(r.primary, spp, block, 1, 0, 1)

    def torch_route(block):
        w = live_block_weights(r.primary.results, spp, block)
        return shard_blocks_device(n, 1, 0, block, priority=w, device=w.device)

    block = cfg["block"]
    for _ in range(5):
        library(block)
    for g in range(groups):
        ms = [timed(lambda: library(block))[0] for _ in range(reps)]
        print(f"one workgroup: {block}-ray blocks, {-(-n // block)} blocks, group {g}: library {summary(ms)}", flush=True)

    for block in (256, 64):
        nb = -(-n // block)
        try:
            lib_blocks, _ = library(block)
        except _lib.MrtError as err:
            lib_blocks = None
            print(f"tiled: {block}-ray blocks, {nb} blocks: library refused: {err}", flush=True)
        for _ in range(5):
            torch_route(block)
            if lib_blocks is not None:
                library(block)
        lib_ms, torch_ms = [], []
        for _ in range(reps):
            t, (tb, _) = timed(lambda: torch_route(block))
            torch_ms.append(t)
            if lib_blocks is not None:
                t, (lib_blocks, _) = timed(lambda: library(block))
                lib_ms.append(t)
        print(f"tiled: {block}-ray blocks, {nb} blocks, {-(-nb // 16384)} tiles: torch route {summary(torch_ms)}", flush=True)
        if lib_blocks is not None:
            print(f"tiled: {block}-ray blocks, {nb} blocks, {-(-nb // 16384)} tiles: library     {summary(lib_ms)}; "
                  f"lists equal: {bool(torch.equal(lib_blocks, tb))}", flush=True)


if __name__ == "__main__":
    main()
