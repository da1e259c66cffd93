"""The launch plan (csrc/launch_plan.cpp) on the CPU: the grid, the residency cap and the spill
slab of a trace launch, persistent or backfilled (cfg.backfill), and the launch configuration
behind mrt_tracer_set_config (defaults, sentinels, valid ranges, waves per CU).

lib/launch_plan_driver (tests/cpp/launch_plan_driver.cpp, built by `make` from launch_plan.cpp
alone with the host compiler: that it links shows the unit has no HIP in it) prints the plan
for figures given on its command line. The saved-schedule bits that carry a backfill go
through lib/tune_driver's import / export, as tests/test_tune.py's do.
"""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "gpu-ray-tracing_amd", "lib")
PLAN_DRIVER = os.path.join(LIB, "launch_plan_driver")
TUNE_DRIVER = os.path.join(LIB, "tune_driver")

CUS = 256
STATIC_LDS = 8192          # a kernel of 8 KB static LDS that the registers admit 8 times per CU
OCC = 8
SPILL_CAP = 256 << 20
VERSION = 11               # MRT_TUNE_VERSION


def run(driver, *args):
    assert os.path.exists(driver), f"{driver} is missing: `make -C gpu-ray-tracing_amd` builds it"
    out = subprocess.run([driver, *map(str, args)], capture_output=True, text=True, check=True).stdout
    return [(line.split()[0], dict(w.split("=", 1) for w in line.split()[1:] if "=" in w), line)
            for line in out.splitlines()]


def plan(rays, k, waves=8, cus=CUS, static=STATIC_LDS, lds=160 << 10, occ=OCC, entries=48, cap=None):
    args = ["plan", rays, k, cus, waves, static, lds, occ, entries] + ([cap] if cap is not None else [])
    (_, kv, _), = run(PLAN_DRIVER, *args)
    return {key: int(v) for key, v in kv.items()}


def roundup8(x):
    return (x + 7) // 8 * 8


RAYS = [1, 63, 64, 65, 2047, 2048, 2049, 76800, 786432, 16588800]


@pytest.mark.parametrize("k", [1, 2, 3, 64])
@pytest.mark.parametrize("rays", RAYS)
def test_grid_is_a_multiple_of_8_and_covers_the_batch_in_k_rounds(rays, k):
    # one workgroup resident on a one-CU device: every grid of eight or more is backfilled
    p = plan(rays, k, waves=4, cus=1, entries=0)
    assert p["per_cu"] == 1
    assert p["backfill"] == k
    assert p["blocks"] % 8 == 0
    assert p["blocks"] * 256 * k >= rays, "k rounds of the grid do not cover the batch"
    assert p["blocks"] == roundup8(-(-(-(-rays // k)) // 256))
    assert (p["blocks"] - 8) * 256 * k < rays, "more than a round-up's worth of empty workgroups"


@pytest.mark.parametrize("k", [1, 2, 3, 64])
@pytest.mark.parametrize("rays", RAYS)
def test_grid_on_the_device_shape(rays, k):
    """256 CUs at 8 waves/CU (512 resident workgroups): a grid of more workgroups is backfilled,
    one that fits is the persistent plan."""
    p = plan(rays, k)
    want = roundup8(-(-(-(-rays // k)) // 256))
    if want <= 512:
        assert p == plan(rays, 0)
    else:
        assert p["backfill"] >= k and p["blocks"] % 8 == 0 and p["blocks"] * 256 * p["backfill"] >= rays


@pytest.mark.parametrize("rays,k", [(1, 1), (131072, 1), (131073, 2), (786432, 6), (786432, 64)])
def test_a_grid_that_fits_is_the_persistent_plan_unchanged(rays, k):
    p, persistent = plan(rays, k), plan(rays, 0)
    assert p == persistent
    assert p == dict(blocks=512, backfill=0, per_cu=2, dyn=0, spill_ints=48 * 512 * 256)


def test_one_ray_past_the_resident_grid_is_backfilled():
    p = plan(131073, 1)
    assert p["backfill"] == 1 and p["blocks"] == 520 and p["per_cu"] == 2
    assert p["spill_ints"] == 48 * 520 * 256


@pytest.mark.parametrize("lds", [160 << 10, 64 << 10])
@pytest.mark.parametrize("cap", [1, 2, 3, 4, 5])
def test_dynamic_lds_gives_exactly_the_asked_blocks_per_cu(cap, lds):
    p = plan(16588800, 1, waves=4 * cap, lds=lds, entries=0)
    assert p["backfill"] == 1 and p["per_cu"] == cap
    total = STATIC_LDS + p["dyn"]
    assert p["dyn"] > 0 and total <= lds
    assert lds // total == cap, f"{total} bytes per workgroup admit {lds // total} per CU"
    (_, _, line), = run(PLAN_DRIVER, "dyn", cap, STATIC_LDS, lds)
    assert line == f"dyn {p['dyn']}"


def test_no_dynamic_lds_when_the_code_object_already_gives_the_residency():
    assert plan(16588800, 1, waves=20, occ=5)["dyn"] == 0          # the register limit is the cap asked for
    assert plan(16588800, 1, waves=32, occ=5)["per_cu"] == 5       # and it bounds what can be asked
    # 40 KB of static LDS admit four workgroups of a 160 KB CU on their own
    (_, _, line), = run(PLAN_DRIVER, "dyn", 4, 40 << 10, 160 << 10)
    assert line == "dyn 0"
    # and never five: no dynamic size gives that residency, so the plan stays persistent
    (_, _, line), = run(PLAN_DRIVER, "dyn", 5, 40 << 10, 160 << 10)
    assert line == "dyn -1"
    assert plan(16588800, 1, waves=20, static=40 << 10, occ=8)["backfill"] == 0


@pytest.mark.parametrize("rays,k", [(16588800, 1), (16588800, 3), (786432, 1), (1 << 30, 1)])
def test_spill_cap_raises_k_and_the_result_fits(rays, k):
    p = plan(rays, k, entries=48)
    assert p["backfill"] >= k or p["backfill"] == 0   # 0: no k fits, the persistent grid
    assert p["spill_ints"] * 4 <= SPILL_CAP
    assert p["spill_ints"] == 48 * p["blocks"] * 256
    if p["backfill"] > 0:
        assert p["blocks"] * 256 * p["backfill"] >= rays
    if p["backfill"] > k:   # the smallest k that fits: one less would not
        assert 48 * roundup8(-(-(-(-rays // (p["backfill"] - 1))) // 256)) * 256 * 4 > SPILL_CAP
    if rays == 16588800 and k == 1:
        # 48 ints per lane: at most 1 398 101 lanes, so 16.6 M rays need k = 12
        assert p["backfill"] == 12
    if rays == 786432:
        assert p["backfill"] == 1   # 786 432 lanes * 192 B = 151 MB fit
    if rays == 1 << 30:
        assert p["backfill"] == 0   # no k up to 64 fits: the persistent grid


def test_a_smaller_spill_cap_and_none_needed():
    assert plan(786432, 1, entries=48, cap=64 << 20)["backfill"] == 3
    assert plan(16588800, 1, entries=0)["backfill"] == 1   # nothing to spill (the LDS ring holds the stack)


# ---------------------------------------------------------------- launch configuration (cfg, waves)
# What mrt_tracer_set_config does before it touches the handle: resolve the "library default"
# sentinels, then validate. The expected values are the library's before this code moved out of the
# HIP glue (default_cfg, the sentinel lines of mrt_tracer_set_config, valid_cfg, grid_waves_per_cu).
DEFAULTS = dict(waves_per_cu=0, fetch_threshold=0, num_queues=-1, lds_stack=16, lane_groups=1, wide=1, spec_slack=2,
                static_rounds=1, autotune=1, tail_lanes=16, queue_shared=0, queue_block=0, ray_sort=0, queue_xcc_mask=0,
                backfill=0, oneshot=0, deal_block=0)


def cfg(**fields):
    """(accepted, the resolved configuration) of the default configuration with `fields` set."""
    (tag, kv, _), = run(PLAN_DRIVER, "cfg", *[f"{k}={v}" for k, v in fields.items()])
    assert tag == "cfg"
    out = {k: int(v) for k, v in kv.items()}
    return out.pop("rc") == 0, out


def ids(c):
    return ",".join(f"{k}={v}" for k, v in c.items()) or "defaults"


def test_default_configuration():
    assert cfg() == (True, DEFAULTS)
    assert len(DEFAULTS) == 17   # every field of mrt_launch_cfg (the driver asserts its own list against the struct)


@pytest.mark.parametrize("field", ["waves_per_cu", "num_queues", "lds_stack", "lane_groups", "static_rounds"])
def test_zero_is_the_library_default(field):
    assert cfg(**{field: 0}) == (True, DEFAULTS)
    # and a negative value is no sentinel there: -1 is num_queues' own default, out of range elsewhere
    ok, c = cfg(**{field: -1})
    assert c == {**DEFAULTS, field: -1} and ok == (field == "num_queues")


@pytest.mark.parametrize("value", [-1, -7])
@pytest.mark.parametrize("field", ["wide", "spec_slack", "autotune", "tail_lanes", "queue_shared", "queue_block",
                                   "queue_xcc_mask", "ray_sort", "backfill", "oneshot", "deal_block"])
def test_negative_is_the_library_default(field, value):
    assert cfg(**{field: value}) == (True, DEFAULTS)


def test_sentinels_resolve_next_to_set_fields_and_fetch_threshold_has_none():
    assert cfg(backfill=1, oneshot=1, deal_block=11, tail_lanes=-1, lds_stack=0, wide=-1) == \
        (True, {**DEFAULTS, "backfill": 1, "oneshot": 1, "deal_block": 11})
    assert cfg(backfill=1, oneshot=-1, deal_block=-1) == (True, {**DEFAULTS, "backfill": 1})
    assert cfg(fetch_threshold=-1) == (False, {**DEFAULTS, "fetch_threshold": -1})
    assert cfg(wide=0, autotune=0, tail_lanes=0, spec_slack=0) == \
        (True, {**DEFAULTS, "wide": 0, "autotune": 0, "tail_lanes": 0, "spec_slack": 0})   # 0 is a value there


# The dicts tests/test_gpu_backfill.py and tests/test_gpu_oneshot.py (test_invalid_combinations_are_refused)
# hand to mrt_tracer_set_config on a device and see refused.
REFUSED = [dict(backfill=1, num_queues=1), dict(backfill=3, num_queues=8), dict(backfill=1, ray_sort=1), dict(backfill=65),
           dict(oneshot=1, backfill=0), dict(oneshot=1, backfill=2), dict(oneshot=1, backfill=1, num_queues=1),
           dict(oneshot=1, backfill=1, ray_sort=1), dict(oneshot=2, backfill=1), dict(oneshot=0, backfill=1, deal_block=10),
           dict(oneshot=1, backfill=1, deal_block=5), dict(oneshot=1, backfill=1, deal_block=16),
           dict(oneshot=1, backfill=1, deal_block=1024)]


@pytest.mark.parametrize("c", REFUSED, ids=ids)
def test_invalid_combinations_are_refused(c):
    assert len(REFUSED) == 13
    assert cfg(**c) == (False, {**DEFAULTS, **c})   # nothing to resolve in them: refused as given


# The configurations the set_config calls of tests/test_gpu_backfill.py, tests/test_gpu_oneshot.py and the
# ray-sort cases of tests/test_gpu_parity.py (test_launch_configs_do_not_change_results) set.
ONESHOT = dict(waves_per_cu=4, backfill=1, oneshot=1, autotune=0)
ACCEPTED = (
    [dict(waves_per_cu=4, backfill=k, lane_groups=g, tail_lanes=t, autotune=0)
     for k in (1, 2, 3) for g in (1, 2, 16) for t in (0, 16)] +
    [dict(waves_per_cu=4, backfill=1, autotune=0), dict(waves_per_cu=8, backfill=1, autotune=0)] +
    [dict(waves_per_cu=4, backfill=1, lds_stack=8, wide=w, tail_lanes=t, autotune=0) for w, t in ((0, 0), (1, 0), (1, 16))] +
    [dict(waves_per_cu=4, backfill=k, lds_stack=8, wide=0, autotune=0) for k in (0, 1)] +
    [dict(waves_per_cu=4 * cap, backfill=1, autotune=0) for cap in (1, 2, 3, 4, 5)] +
    [dict(autotune=1, waves_per_cu=0, backfill=0, lane_groups=1, num_queues=-1, lds_stack=16, wide=1, tail_lanes=16),
     dict(backfill=2), dict(backfill=-1)] +
    [dict(ONESHOT, deal_block=b, lane_groups=g, tail_lanes=t) for b in (0, 6, 10, 13) for g in (1, 2, 16) for t in (0, 16)] +
    [dict(ONESHOT, deal_block=b) for b in (6, 10, 13)] +
    [dict(ONESHOT, oneshot=0, deal_block=0), dict(ONESHOT, deal_block=10, lds_stack=8)] +
    [dict(ONESHOT, deal_block=10, lds_stack=16, wide=1, tail_lanes=t) for t in (0, 16)] +
    [dict(waves_per_cu=4, lds_stack=16, wide=0, autotune=0, deal_block=0, backfill=k, oneshot=k) for k in (0, 1)] +
    [dict(autotune=1, waves_per_cu=0, backfill=0, oneshot=0, deal_block=0, lane_groups=1, num_queues=-1, lds_stack=16,
          wide=1, tail_lanes=16),
     dict(backfill=1, oneshot=1, deal_block=11), dict(oneshot=-1, deal_block=-1)] +
    [dict(ray_sort=1), dict(ray_sort=1, tail_lanes=0), dict(ray_sort=1, waves_per_cu=4), dict(ray_sort=1, lane_groups=16),
     dict(ray_sort=1, waves_per_cu=8, lds_stack=8)])


@pytest.mark.parametrize("c", ACCEPTED, ids=ids)
def test_configurations_the_gpu_tests_set_are_accepted(c):
    ok, got = cfg(**c)
    assert ok
    assert got == {**DEFAULTS, **{k: (DEFAULTS[k] if v < 0 and k != "num_queues" else v) for k, v in c.items()}}


# Every range of valid_cfg: the last value inside and the first outside, on each side.
@pytest.mark.parametrize("field,inside,outside", [
    ("waves_per_cu", [4, 32], [-1, 1, 3, 33]),                 # 0 (auto) or 4..32
    ("fetch_threshold", [0, 64], [-1, 65]),
    ("num_queues", [-1, 1, 8], [-2, 9]),                       # 0 is the sentinel
    ("lds_stack", [8, 16, 32], [-1, 4, 7, 9, 12, 24, 33, 64]),
    ("lane_groups", [1, 2, 64], [-1, 3, 63, 65, 128]),         # a power of two up to 64
    ("wide", [0, 2], [3]),
    ("spec_slack", [0, 63], [64]),
    ("static_rounds", [1, 64], [-1, 65]),
    ("autotune", [0, 1], [2]),
    ("tail_lanes", [0, 16], [17]),
    ("queue_shared", [0, 100], [101]),
    ("queue_block", [0, 64, 1 << 20], [1, 32, 63, 65, 96, (1 << 20) + 1, 1 << 21]),   # 0 or a power of two 64..2^20
    ("queue_xcc_mask", [0, 15], [16]),
    ("ray_sort", [0, 1], [2]),
    ("backfill", [0, 1, 64], [65]),
    ("oneshot", [0], [1, 2]),                                  # alone: oneshot needs backfill = 1
    ("deal_block", [0], [6, 15]),                              # alone: the deal's blocks are the one-shot kernels'
])
def test_range_limits(field, inside, outside):
    for v in inside:
        assert cfg(**{field: v}) == (True, {**DEFAULTS, field: v}), f"{field}={v} refused"
    for v in outside:
        assert cfg(**{field: v}) == (False, {**DEFAULTS, field: v}), f"{field}={v} accepted"


def test_range_limits_of_the_one_shot_fields():
    for b, ok in ((0, True), (5, False), (6, True), (15, True), (16, False)):
        assert cfg(oneshot=1, backfill=1, deal_block=b)[0] == ok, f"deal_block={b}"
    assert cfg(oneshot=1, backfill=1)[0] and not cfg(oneshot=2, backfill=1)[0]
    assert not cfg(oneshot=1, backfill=2)[0] and not cfg(oneshot=1, backfill=0)[0]


def waves(rays, num_queues, waves_per_cu=0, cus=CUS):
    (_, _, line), = run(PLAN_DRIVER, "waves", cus, rays, num_queues, waves_per_cu)
    assert line.split()[0] == "waves"
    return int(line.split()[1])


def test_waves_per_cu_a_batch_gets():
    """grid_waves_per_cu on 256 CUs, from the library's code before it moved."""
    for rays in (1, 76800, 524288, 524289, 12582912, 1 << 30):
        assert waves(rays, -1) == 20              # static rounds: kStridedWaves, whatever the batch
        assert waves(rays, -1, 12) == 12 and waves(rays, 1, 12) == 12   # an explicit setting, in both modes
    assert waves(524288, 1) == 32                 # one ray per lane at full occupancy: 32 * 64 * 256 lanes
    assert waves(524289, 1) == 8                  # one more: 12 rays per lane, at least 8 waves
    assert waves(3145728, 1) == 16
    assert waves(12582912, 1) == 32
    assert waves(1 << 30, 8) == 32                # never above 32
    assert waves(2048, 1, cus=1) == 32 and waves(2049, 1, cus=0) == 8   # a device reporting no CUs counts as one


# ---------------------------------------------------------------- saved schedules (tune_driver)
def tune(*args):
    return run(TUNE_DRIVER, *args)


def imported(code, rays=786432, variant=342):
    lines = tune("import", 1, rays, variant, code, VERSION, "export")
    rc = int(lines[0][1]["rc"])
    return rc, int(lines[0][1]["keys"]), [int(kv["candidate"]) for tag, kv, _ in lines if tag == "exported"]


@pytest.mark.parametrize("code", [268 | 1 << 16 | 2 << 24, 1 | 3 << 16, 0 | 64 << 16 | 5 << 24, 13 - 3 | 5 << 8 | 2 << 16,
                                  6 | 6 << 8 | 1 << 16 | 7 << 24])
def test_backfill_bits_round_trip_import_to_export(code):
    assert imported(code) == (0, 1, [code])


@pytest.mark.parametrize("code", [0, 5, 3 | 3 << 8, 11 | 5 << 8, 12 | 1 << 8, 10 | 7 << 8])
def test_old_codes_import_as_before(code):
    assert imported(code) == (0, 1, [code])


def test_a_saved_backfill_keeps_the_sixteen_bit_info_code_and_sets_the_cap():
    lines = tune("import", 1, 786432, 342, 268 | 1 << 16 | 3 << 24, VERSION, "launch", 786432, 342, 1)
    (l,) = [kv for tag, kv, _ in lines if tag == "launch"]
    assert (l["cand"], l["info"], l["locked"], l["waves"], l["queues"]) == ("12", "0x10c", "1", "12", "-1")
    lines = tune("import", 1, 786432, 342, 268, VERSION, "launch", 786432, 342, 1)
    (l,) = [kv for tag, kv, _ in lines if tag == "launch"]
    assert (l["cand"], l["info"], l["locked"], l["waves"]) == ("12", "0x10c", "1", "8")


@pytest.mark.parametrize("code", [268 | 1 << 27, 268 | 1 << 16 | 1 << 27, 268 | 1 << 30, -1,       # bits above the fields
                                  268 | 65 << 16, 268 | 255 << 16,                                  # k > 64
                                  2 | 1 << 16, 3 | 3 << 8 | 1 << 16, 8 | 4 << 8 | 2 << 16, 7 | 1 << 16,   # queue schedules
                                  11 | 2 << 8 | 1 << 16 | 2 << 24,
                                  268 | 2 << 24,                                                    # a cap without a backfill
                                  13 | 1 << 8 | 1 << 16, 12 | 8 << 8 | 1 << 16])                    # the 16-bit checks still hold
def test_bad_backfill_codes_are_refused_with_nothing_imported(code):
    rc, keys, out = imported(code)
    assert rc == 1 and keys == 0 and out == []
    # and a good entry next to a bad one is not imported either
    lines = tune("import", 2, 1000, 342, 268 | 1 << 16, VERSION, 786432, 342, code, VERSION, "export")
    assert int(lines[0][1]["rc"]) == 1 and int(lines[0][1]["keys"]) == 0
