"""The one-shot deal on the CPU: which lane of a one-shot grid (cfg.oneshot) traces which ray
(csrc/deal_common.hpp, compiled by g++ here and by hipcc into the one-shot kernels), the grid the
launch plan sizes for it (csrc/launch_plan.cpp), its fallbacks, and the saved-schedule bits that
carry oneshot and deal_block (csrc/tune.cpp).

lib/deal_driver (tests/cpp/deal_driver.cpp, built by `make` with the host compiler alone) plans the
grid, enumerates every launched lane and prints the counts asserted here. The same source is built
once more with -fsanitize=address,undefined and run over the same cases: a stand-alone program.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gpu-ray-tracing_amd")
DRIVER = os.path.join(PKG, "lib", "deal_driver")
SOURCES = [os.path.join(REPO, "tests", "cpp", "deal_driver.cpp"), os.path.join(PKG, "csrc", "launch_plan.cpp"),
           os.path.join(PKG, "csrc", "tune.cpp")]

RAYS = [1, 63, 64, 65, 1000, 1023, 1024, 1025, 8191, 8192, 8193, 65537, 73729, 76800, 786432]
BLOCKS = [0, 6, 8, 10, 13]
LANE_GROUPS = [1, 2, 16]
VERSION = 11


def run(driver, *args):
    assert os.path.exists(driver), f"{driver} is missing: `make -C gpu-ray-tracing_amd` builds it"
    p = subprocess.run([driver, *map(str, args)], capture_output=True, text=True)
    assert p.returncode == 0, f"{driver} {args}: exit {p.returncode}\n{p.stderr}"
    return [{k: int(v) for k, v in (w.split("=", 1) for w in line.split()[1:])} for line in p.stdout.splitlines()]


def chunk(n, b):
    """Positions per XCD group: roundup64(ceil(n / 8)), or ceil(ceil(n / 2^b) / 8) blocks."""
    if b == 0:
        return (-(-n // 8) + 63) // 64 * 64
    return -(-(-(-n // (1 << b))) // 8) << b


def check_deal(d, n, b):
    assert d["oneshot"] == 1
    assert d["blocks"] % 8 == 0 and d["blocks"] == 8 * -(-chunk(n, b) // 256)
    assert d["lanes"] == d["blocks"] * 256 and d["lanes"] >= n
    assert d["spill_ints"] == 48 * d["lanes"], "the slab does not cover the launched lanes"
    assert d["dealt"] == n and d["twice"] == 0 and d["missing"] == 0, "not every ray exactly once"
    assert d["past"] == 0, "a lane was dealt an index outside the batch"
    assert d["group_bad"] == 0, "a ray is not in group (ray >> b) % 8"
    assert d["ref_bad"] == 0, "b = 0 differs from the first strided round"


# One CU with one workgroup resident: a grid is at least eight workgroups, so every batch is
# oversubscribed there and is planned one-shot, down to a single ray.
@pytest.mark.parametrize("groups", LANE_GROUPS)
@pytest.mark.parametrize("b", BLOCKS)
@pytest.mark.parametrize("n", RAYS)
def test_every_ray_dealt_exactly_once(n, b, groups):
    (d,) = run(DRIVER, "deal", n, b, groups.bit_length() - 1, 1, 4, 1, 48)
    check_deal(d, n, b)


@pytest.mark.parametrize("b", BLOCKS)
@pytest.mark.parametrize("n", [65537, 73729, 76800, 786432])
def test_grid_on_the_device_shape(n, b):
    """256 CUs at 4 waves/CU: 65 536 resident lanes, every n here is oversubscribed."""
    (d,) = run(DRIVER, "deal", n, b, 1, 256, 4, 5, 48)
    check_deal(d, n, b)


def test_chunk_may_exceed_an_eighth_of_the_batch():
    (d,) = run(DRIVER, "deal", 65537, 13, 0, 256, 4, 5, 48)   # 9 blocks of 8192: two per group
    assert d["blocks"] == 8 * 2 * 8192 // 256 and d["lanes"] == 131072 and d["dealt"] == 65537


# ---------------------------------------------------------------- fallbacks
def test_batch_that_fits_the_resident_grid_is_todays_plan():
    with_, without = run(DRIVER, "plan", 131072, 10, 256, 8, 8, 48)
    assert with_ == without and with_["oneshot"] == 0 and with_["backfill"] == 0 and with_["blocks"] == 512


def test_slab_cap_that_forces_more_rays_per_lane_is_todays_plan():
    # 786 432 lanes * 48 ints * 4 B = 151 MB: a 64 MB cap asks for k = 3, which is not one-shot
    with_, without = run(DRIVER, "plan", 786432, 10, 256, 8, 8, 48, 64 << 20)
    assert with_ == without and with_["oneshot"] == 0 and with_["backfill"] == 3
    # and the chunk's round-up counts: 65 537 rays in 8192-ray blocks launch 131 072 lanes
    with_, without = run(DRIVER, "plan", 65537, 13, 256, 4, 5, 48, 131071 * 48 * 4)
    assert with_ == without and with_["oneshot"] == 0 and with_["backfill"] == 1
    with_, _ = run(DRIVER, "plan", 65537, 13, 256, 4, 5, 48, 131072 * 48 * 4)
    assert with_["oneshot"] == 1 and with_["spill_ints"] == 131072 * 48


def test_one_shot_plan_keeps_the_residency_cap():
    with_, without = run(DRIVER, "plan", 786432, 10, 256, 20, 8, 48)
    assert with_["oneshot"] == 1 and with_["deal_block"] == 10 and with_["blocks"] == 3072
    assert (with_["per_cu"], with_["dyn"], with_["backfill"]) == (without["per_cu"], without["dyn"], 1)
    assert with_["per_cu"] == 5 and with_["dyn"] > 0


@pytest.mark.parametrize("b", [1, 5, 16, -1])
def test_block_outside_the_range_is_not_planned(b):
    with_, without = run(DRIVER, "plan", 786432, b, 256, 20, 8, 48)
    assert with_["oneshot"] == 0 and {**with_, "deal_block": 0} == without


# ---------------------------------------------------------------- saved schedules
BACKFILLED = 268 | 1 << 16 | 5 << 24   # 2 lane groups at slack 6 on the 8-waves/CU schedule, k = 1, cap 5


def code(c):
    (d,) = run(DRIVER, "code", c)
    return d


@pytest.mark.parametrize("deal", [0, 6, 10, 11, 12, 15])
def test_one_shot_bits_round_trip(deal):
    c = BACKFILLED | 1 << 23 | deal << 27
    d = code(c)
    assert d["rc"] == 0 and d["exported"] == c and c > 0
    assert (d["backfill"], d["oneshot"], d["deal_block"], d["waves"]) == (1, 1, deal, 20)
    assert d["info"] == 268, "autotune_candidate is the 16-bit code"


@pytest.mark.parametrize("c", [0, 5, 268, 11 | 5 << 8, BACKFILLED, 1 | 3 << 16, 64 << 16 | 5 << 24])
def test_old_codes_decode_as_before(c):
    d = code(c)
    assert d["rc"] == 0 and d["exported"] == c and d["oneshot"] == 0 and d["deal_block"] == 0
    assert d["backfill"] == (c >> 16) & 0x7f


@pytest.mark.parametrize("c", [268 | 1 << 23,                               # one-shot without a backfill
                               268 | 2 << 16 | 1 << 23,                     # or with k = 2
                               BACKFILLED | 10 << 27,                       # a deal without one-shot
                               BACKFILLED | 1 << 23 | 1 << 27, BACKFILLED | 1 << 23 | 5 << 27,   # blocks below 2^6
                               2 | 1 << 16 | 1 << 23,                       # a queue schedule
                               -1, BACKFILLED | 1 << 23 | 1 << 31])         # the sign bit
def test_bad_one_shot_codes_are_refused(c):
    if c >= 1 << 31:
        c -= 1 << 32
    d = code(c)
    assert d["rc"] == 1 and d["keys"] == 0


# ---------------------------------------------------------------- the same cases under the sanitizers
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host compiler"
    exe = str(tmp_path_factory.mktemp("deal_san") / "deal_driver_san")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I" + os.path.join(REPO, "include"), "-o", exe, *SOURCES], check=True)
    return exe


def test_the_cases_under_address_and_undefined_sanitizers(sanitized):
    for n in RAYS:
        for b in BLOCKS:
            for groups in LANE_GROUPS:
                (d,) = run(sanitized, "deal", n, b, groups.bit_length() - 1, 1, 4, 1, 48)
                check_deal(d, n, b)
    for c in (BACKFILLED | 1 << 23 | 10 << 27, 268, BACKFILLED | 10 << 27, -1):
        run(sanitized, "code", c)
    run(sanitized, "plan", 786432, 10, 256, 20, 8, 48)
    run(sanitized, "plan", 1 << 30, 15, 256, 20, 8, 0)
