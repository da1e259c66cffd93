"""The frame path's planning on the CPU: a rank's share of a frame's blocks, the path its block list
takes to its order, the block ray generator's checks and grid, the hit count's partials and the
1-D grids (csrc/frame_plan.cpp, what csrc/frame_api.cpp launches with), and the live-first sort
key (csrc/live_key_common.hpp, compiled by g++ here and by hipcc into block_live_kernel).

lib/frame_plan_driver (tests/cpp/frame_plan_driver.cpp, built by `make` with the host compiler
alone) prints what is asserted here. The same source is built once more with
-fsanitize=address,undefined and run over the same cases: a stand-alone program. That run is what
the cases at INT32_MAX are for: the arithmetic they reach was done in int before the plan existed.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from mrt import dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gpu-ray-tracing_amd")
DRIVER = os.path.join(PKG, "lib", "frame_plan_driver")
SOURCES = [os.path.join(REPO, "tests", "cpp", "frame_plan_driver.cpp"), os.path.join(PKG, "csrc", "frame_plan.cpp")]

INT32_MAX = 2**31 - 1
OK, INVALID_ARG, TOO_LARGE = 0, 1, 5                 # include/mrt.h
NONE, LIST, ONE_WORKGROUP, TILED = 0, 1, 2, 3        # frame_plan.hpp OrderPath
THREADS, TILE_RAYS, ORDER_MAX, KEY_MAX, COUNT_BLOCKS = 256, 1024, 16384, 4095, 1024   # frame_limits.hpp


def ceil_div(n, d):
    return -(-n // d)


def run(driver, *ops):
    """One process for a list of ops (each a tuple of the op's name and its numbers): a dict per
    line of k=v output (why: the rest of the line), a list of ints for the lines that are numbers."""
    assert os.path.exists(driver), f"{driver} is missing: `make -C gpu-ray-tracing_amd` builds it"
    args = [str(a) for op in ops for a in op]
    p = subprocess.run([driver, *args], capture_output=True, text=True)
    assert p.returncode == 0, f"{driver} {args}: exit {p.returncode}\n{p.stderr}"
    out = []
    for line, op in zip(p.stdout.splitlines(), ops):
        name, _, rest = line.partition(" ")
        assert name == op[0]
        if "=" not in rest:
            out.append([int(w) for w in rest.split()])
            continue
        rest, _, why = rest.partition(" why=")
        d = {k: int(v) for k, v in (w.split("=", 1) for w in rest.split())}
        if name == "aoblocks":
            d["why"] = why
        out.append(d)
    assert len(out) == len(ops)
    return out


# ---------------------------------------------------------------- extent
EXTENT_BLOCKS = [1, 13, 1024]
WORLDS = [1, 3, 8]


def check_extent(driver, block):
    totals = sorted({0, 1, block - 1, block, block + 1, 7 * block + 3})
    cases = [(total, world, rank) for total in totals for world in WORLDS for rank in range(world)]
    got = run(driver, *[("extent", total, 1, block, world, rank) for total, world, rank in cases])
    rays = {}
    for (total, world, rank), x in zip(cases, got):
        listed = dist.shard_blocks(total, world, rank, block)
        assert x["rc"] == OK and x["total"] == total and x["nb"] == ceil_div(total, block)
        assert x["mine"] == len(listed), (total, world, rank)
        assert x["rays"] == sum(min(block, total - int(b) * block) for b in listed), (total, world, rank)
        assert x["last"] == int(len(listed) > 0 and int(listed[-1]) == x["nb"] - 1)
        rays[total, world] = rays.get((total, world), 0) + x["rays"]
    for (total, world), s in rays.items():
        assert s == total, f"the ranks' rays of {total} over {world} sum to {s}"


def check_extent_limits(driver):
    big, most, split = run(driver, ("extent", 65536, 32768, 1024, 2, 0), ("extent", INT32_MAX, 1, 1024, 2, 1),
                           ("extent", 46341, 46341, 7, 3, 2))
    assert big["rc"] == TOO_LARGE and big["mine"] == 0 and big["rays"] == 0        # 2^31 rays
    assert most["rc"] == OK and most["total"] == INT32_MAX and most["nb"] == 2097152
    assert most["mine"] == 1048576 and most["last"] == 1 and most["rays"] == 1048576 * 1024 - 1
    assert split["rc"] == TOO_LARGE                                                  # 46341^2 = 2^31 + 4633


@pytest.mark.parametrize("block", EXTENT_BLOCKS)
def test_extent_is_the_hosts_shard(block):
    check_extent(DRIVER, block)


def test_extent_at_the_frame_limit():
    check_extent_limits(DRIVER)


# ---------------------------------------------------------------- order path
def check_paths(driver):
    none, lst, one, tiled = run(driver, ("order", 0, 1), ("order", 5000, 0), ("order", ORDER_MAX, 1),
                                ("order", ORDER_MAX + 1, 1))
    assert none == dict(path=NONE, grid=0, tiles=0, table_words=0, words=0, bytes=0)
    assert lst == dict(path=LIST, grid=ceil_div(5000, THREADS), tiles=0, table_words=0, words=0, bytes=0)
    assert one == dict(path=ONE_WORKGROUP, grid=ORDER_MAX // 4, tiles=0, table_words=0, words=0, bytes=0)
    words = 4096 * 2 + 16385
    assert tiled == dict(path=TILED, grid=ceil_div(16385, 4), tiles=2, table_words=4096 * 2, words=words, bytes=4 * words)
    assert run(driver, ("order", 0, 0))[0]["path"] == NONE
    # the longest list there is: every ray of the largest frame its own block, one rank
    x, = run(driver, ("extent", INT32_MAX, 1, 1, 1, 0))
    assert x["rc"] == OK and x["mine"] == INT32_MAX and x["rays"] == INT32_MAX
    p, = run(driver, ("order", x["mine"], 1))
    assert p["path"] == TILED and p["tiles"] == 131072 and p["grid"] == ceil_div(INT32_MAX * 64, THREADS)
    assert p["table_words"] == (KEY_MAX + 1) * 131072 and p["words"] == p["table_words"] + INT32_MAX
    assert p["bytes"] == ((KEY_MAX + 1) * ceil_div(INT32_MAX, ORDER_MAX) + INT32_MAX) * 4
    q, = run(driver, ("order", INT32_MAX, 0))
    assert q["path"] == LIST and q["grid"] == ceil_div(INT32_MAX, THREADS)


def test_order_paths():
    check_paths(DRIVER)


# ---------------------------------------------------------------- the live-first key
KEY_BLOCKS = [1, 64, 4094, 4095, 4096, 8000, 65536]


def check_keys(driver, block):
    keys, = run(driver, ("keys", block))
    keys = np.asarray(keys, dtype=np.int64)
    assert len(keys) == block + 1
    assert np.array_equal(keys, -dist.live_priority(np.arange(block + 1), block)), "not the host's restatement"
    assert np.all(np.diff(keys) <= 0), "more live rays, larger key"
    assert keys.min() >= 0 and keys.max() <= KEY_MAX - 1, "a full block's key reaches the partial block's"
    assert keys[block] == 0 and keys[0] == min(block, KEY_MAX - 1)
    partial = run(driver, ("key", block, 0, 1), ("key", block, block // 2, 1), ("key", block, block, 1))
    assert partial == [[KEY_MAX]] * 3, "the partial last block sorts last"


@pytest.mark.parametrize("block", KEY_BLOCKS)
def test_key_is_the_hosts_live_priority(block):
    assert dist.KEY_MAX == KEY_MAX - 1
    check_keys(DRIVER, block)


# ---------------------------------------------------------------- the block ray generator
def ao(inputs=1000, samples=8, batches=1, batch_inputs=1000, blocks=3, block=1000, out=3000):
    return ("aoblocks", inputs, samples, batches, batch_inputs, blocks, block, out)


def check_ao_refusals(driver):
    refusals = [
        (ao(samples=0), INVALID_ARG, "bad ray/sample/block count"),
        (ao(inputs=-1), INVALID_ARG, "bad ray/sample/block count"),
        (ao(out=-1), INVALID_ARG, "bad ray/sample/block count"),
        (ao(inputs=65536, samples=32768, batch_inputs=65536), TOO_LARGE, "too many frame rays"),
        (ao(batches=3, batch_inputs=250), INVALID_ARG, "fewer batch seeds than batches"),
        (ao(blocks=9, out=8000), INVALID_ARG, "more blocks listed than the frame has"),
        (ao(out=1999), INVALID_ARG, "numOutRays does not match the listed blocks"),
        (ao(out=3001), INVALID_ARG, "numOutRays does not match the listed blocks"),
        (ao(blocks=0, out=1), INVALID_ARG, "numOutRays does not match the listed blocks"),
        # the checks come in this order: a frame that is too large and short of seeds is too large
        (ao(inputs=65536, samples=32768, batches=0), TOO_LARGE, "too many frame rays"),
        (ao(batches=0, blocks=9), INVALID_ARG, "fewer batch seeds than batches"),
    ]
    for (_, rc, why), p in zip(refusals, run(driver, *[r[0] for r in refusals])):
        assert (p["rc"], p["why"]) == (rc, why)


def check_ao_accepted(driver):
    low, high, all_, none, most = run(driver, ao(out=2000), ao(out=3000), ao(blocks=8, out=8000), ao(blocks=0, out=0),
                                      ao(inputs=INT32_MAX // 4, samples=4, batches=1, batch_inputs=INT32_MAX, blocks=2097152,
                                         block=1024, out=INT32_MAX - 3))
    for p, out in ((low, 2000), (high, 3000), (all_, 8000)):
        assert p == dict(rc=OK, total=8000, need=1, empty=0, tiled=0, grid=ceil_div(out, THREADS), in_args=1, why="")
    assert none["rc"] == OK and none["empty"] == 1 and none["grid"] == 0
    assert most["rc"] == OK and most["tiled"] == 1 and most["grid"] == 2097152 and most["total"] == INT32_MAX - 3
    # the seeds: 256 batches ride in the arguments, 257 need the table
    fit, table, spare = run(driver, ao(inputs=2560, batches=257, batch_inputs=10, blocks=1, block=30000, out=20480),
                            ao(inputs=2561, batches=257, batch_inputs=10, blocks=1, block=30000, out=20488),
                            ao(inputs=2560, batches=256, batch_inputs=10, blocks=1, block=30000, out=20480))
    assert (fit["rc"], fit["need"], fit["in_args"]) == (OK, 256, 1) and fit == spare
    assert (table["rc"], table["need"], table["in_args"]) == (OK, 257, 0)


# (block, samples) on both sides of each condition of the tiled generator: the block a multiple
# of the tile, whole input rays per tile, at most 256 input rays per tile, at most 256 samples
TILED_CASES = [(1024, 8, True), (1023, 8, False), (2048, 8, True), (1536, 8, False),
               (1024, 3, False), (1024, 4, True), (1024, 2, False), (1024, 1, False),
               (1024, 256, True), (1024, 512, False), (1024, 1024, False), (3072, 64, True)]


def check_ao_tiled(driver):
    inputs = 4099
    ops = [ao(inputs=inputs, samples=s, batch_inputs=inputs, blocks=ceil_div(inputs * s, b), block=b, out=inputs * s)
           for b, s, _ in TILED_CASES]
    for (b, s, tiled), p in zip(TILED_CASES, run(driver, *ops)):
        assert p["rc"] == OK and p["tiled"] == int(tiled), (b, s)
        assert p["grid"] == ceil_div(inputs * s, TILE_RAYS if tiled else THREADS), (b, s)


def test_ao_blocks_refusals():
    check_ao_refusals(DRIVER)


def test_ao_blocks_accepted_and_seeds():
    check_ao_accepted(DRIVER)


def test_ao_blocks_tiled_choice_and_grid():
    check_ao_tiled(DRIVER)


# ---------------------------------------------------------------- the hit count and the 1-D grids
COUNTS = [0, 1, 255, 256, 257, 262144, 262145, INT32_MAX]


def check_counts(driver):
    for n, c in zip(COUNTS, run(driver, *[("count", n) for n in COUNTS])):
        per, blocks = c["per_block"], c["blocks"]
        assert per % THREADS == 0 and blocks <= COUNT_BLOCKS, n
        assert blocks * per >= n > (blocks - 1) * per, n      # covered, and the last block is not empty
        assert per >= THREADS and (blocks == 0) == (n == 0), n
    grids = run(driver, *[("grid", n) for n in COUNTS], ("grid", INT32_MAX, TILE_RAYS), ("grid", INT32_MAX * 64),
                ("grid", 2**32, THREADS), ("grid", 2**40, 1), ("grid", -1))
    assert grids[:len(COUNTS)] == [[ceil_div(n, THREADS)] for n in COUNTS]
    assert grids[len(COUNTS):] == [[ceil_div(INT32_MAX, TILE_RAYS)], [ceil_div(INT32_MAX * 64, THREADS)], [2**24], [-1], [-1]]


def test_count_partials_and_grids():
    check_counts(DRIVER)


# ---------------------------------------------------------------- the same cases under the sanitizers
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host compiler"
    exe = str(tmp_path_factory.mktemp("frame_plan_san") / "frame_plan_driver_san")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I" + os.path.join(REPO, "include"), "-o", exe, *SOURCES], check=True)
    return exe


def test_the_cases_under_address_and_undefined_sanitizers(sanitized):
    for block in EXTENT_BLOCKS:
        check_extent(sanitized, block)
    check_extent_limits(sanitized)
    check_paths(sanitized)
    for block in KEY_BLOCKS:
        check_keys(sanitized, block)
    check_ao_refusals(sanitized)
    check_ao_accepted(sanitized)
    check_ao_tiled(sanitized)
    check_counts(sanitized)
