"""Backfilled static launches (cfg.backfill, csrc/launch_plan.cpp): a grid sized from the
batch, whose workgroups take k rays per lane and end, with the hardware dispatcher filling the
freed slots. Same kernels, same rays, same results: every ray traced exactly once and equal
to the oracle; what changes is the grid, the residency cap and the spill slab's size."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import kat  # noqa: E402
import oracle_lib as O  # noqa: E402
from test_gpu_parity import assert_valid_hits, scene_setup  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)   # bench.schedule_name

SENTINEL = 0x5A5A5A5A
# At waves_per_cu = 4 one workgroup is resident per CU: 256 lanes per CU.
RESIDENT_LANES_PER_CU = 256


@pytest.fixture(scope="module")
def tracer():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mrt.tracer import Tracer
    return Tracer(0)


@pytest.fixture()
def restore(tracer):
    saved = tracer.config()
    yield
    tracer.set_config(**saved)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def backfill_grid_waves(n, k):
    blocks = -(-(-(-n // k)) // 256)
    return (blocks + 7) // 8 * 8 * 4


def trace(tracer, bufs, rays, any_hit, bind=True):
    """One blocking exact speculative trace into sentinel-filled results: an untraced ray shows."""
    from mrt.tracer import GpuBvh, RayBuffer
    if bind:
        tracer.set_bvh(GpuBvh(bufs))
    rb = RayBuffer(rays, need_closest_hit=not any_hit)
    rb.results.fill_(SENTINEL)
    tracer.trace_batch(rb, exact_rcp=True)
    r = rb.results_numpy()
    assert (r[:, 2:] == SENTINEL).all(), "RayResult padding was overwritten"
    assert not ((r[:, 0] == SENTINEL) & (r[:, 1] == SENTINEL)).any(), "a ray was not traced"
    return r


def assert_matches_oracle(rays, res, want, bufs, any_hit):
    """Closest hits bit-identical in t, ids identical except at exact-t ties (those valid hits);
    any-hit rays hit/miss identical and every differing hit valid."""
    if any_hit:
        assert_valid_hits(rays, res, want, bufs)
        return
    assert np.array_equal(res[:, 1], want[:, 1]), "closest-hit t differs"
    ties = np.nonzero(res[:, 0] != want[:, 0])[0]
    bad = O.invalid_hits(rays, res, bufs[1], bufs[2], which=ties)
    assert len(bad) == 0, f"{len(bad)} of {len(ties)} differing ids are not valid hits at the same t"


# ---------------------------------------------------------------- every ray once, oracle parity
# bunny primary 320x240 and conference AO 256x192 at waves_per_cu = 4 (65 536 resident lanes on
# 256 CUs: the bunny batch at k = 1 is the smallest oversubscribed grid there is; the others fit
# the resident grid and must run the persistent plan unchanged), and conference AO 640x480, whose
# grid is oversubscribed at every k, for the any-hit kernels.
@pytest.mark.parametrize("tail", [0, 16])
@pytest.mark.parametrize("groups", [1, 2, 16])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("wl", [("bunny", 320, 240, "primary"), ("conference", 256, 192, "ao")],
                         ids=lambda w: "-".join(map(str, w)))
def test_every_ray_traced_once(tracer, restore, wl, k, groups, tail):
    bufs, rays, any_hit, want, _ = scene_setup(*wl)
    tracer.set_config(waves_per_cu=4, backfill=k, lane_groups=groups, tail_lanes=tail, autotune=0)
    res = trace(tracer, bufs, rays, any_hit)
    assert_matches_oracle(rays, res, want, bufs, any_hit)
    info = tracer.last_info
    assert info["num_queues"] == 0 and info["stack_overflows"] == 0
    n = len(rays)
    oversubscribed = backfill_grid_waves(n, k) > cus() * RESIDENT_LANES_PER_CU // 64
    assert info["backfill"] == (k if oversubscribed else 0)
    assert info["grid_waves"] == (backfill_grid_waves(n, k) if oversubscribed else cus() * 4)
    if cus() == 256:
        assert oversubscribed == (n == 76800 and k == 1)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_every_any_hit_ray_traced_once_oversubscribed(tracer, restore, k):
    bufs, rays, any_hit, want, _ = scene_setup("conference", 640, 480, "ao")
    tracer.set_config(waves_per_cu=4, backfill=k, lane_groups=2, tail_lanes=16, autotune=0)
    res = trace(tracer, bufs, rays, any_hit)
    assert_matches_oracle(rays, res, want, bufs, any_hit)
    if cus() <= 256:
        assert tracer.last_info["backfill"] == k
        assert tracer.last_info["grid_waves"] == backfill_grid_waves(len(rays), k)


# ---------------------------------------------------------------- ragged and tiny batches
@pytest.mark.parametrize("n", [1, 63, 65, 1000, 4097, 65537])
def test_ragged_and_tiny_batches(tracer, restore, n):
    """Grids below eight workgroups' worth of rays, empty workgroups after the round-up to a
    multiple of eight, and one ray past the 65 536 resident lanes of waves_per_cu = 4."""
    bufs, rays, any_hit, want, _ = scene_setup("bunny", 320, 240, "primary")
    tracer.set_config(waves_per_cu=4, backfill=1, autotune=0)
    res = trace(tracer, bufs, rays[:n], False)
    assert_matches_oracle(rays[:n], res, want[:n], bufs, False)
    if n > cus() * RESIDENT_LANES_PER_CU:
        assert tracer.last_info["backfill"] == 1
        assert tracer.last_info["grid_waves"] == backfill_grid_waves(n, 1)
    else:
        assert tracer.last_info["backfill"] == 0 and tracer.last_info["dyn_lds_bytes"] == 0


# ---------------------------------------------------------------- spill under an oversubscribed grid
def comb_batch(depth):
    bufs, ray, expect = kat.scene_comb(depth)
    n = cus() * RESIDENT_LANES_PER_CU + 1000   # more rays than the resident lanes at waves_per_cu = 4
    return bufs, np.stack([ray] * n), expect


@pytest.mark.parametrize("wide,tail", [(0, 0), (1, 0), (1, 16)])
@pytest.mark.parametrize("depth", [40, 63])
def test_spill_slab_of_the_launched_grid(tracer, restore, depth, wide, tail):
    """Deep comb rays with an 8-entry LDS ring push through the spill slab, which is indexed by
    the launched lane: it has to be sized for the launched grid. The hand answer (which the
    oracle reproduces) for every ray, no overflow."""
    bufs, rays, expect = comb_batch(depth)
    want, _, _ = O.trace(rays[:1], *bufs)
    assert want[0, 0] == expect[0] and want[0, 1] == kat.f2i(expect[1])
    tracer.set_config(waves_per_cu=4, backfill=1, lds_stack=8, wide=wide, tail_lanes=tail, autotune=0)
    res = trace(tracer, bufs, rays, False)
    assert tracer.last_info["backfill"] == 1 and tracer.last_info["stack_overflows"] == 0
    assert tracer.last_info["lds_stack_entries"] == 8
    assert (res[:, 0] == want[0, 0]).all() and (res[:, 1] == want[0, 1]).all()


def test_overflow_reported_as_by_the_persistent_launch(tracer, restore):
    """Depth 70 overflows the reference's 64-entry stack in the binary order: the backfilled
    launch counts exactly the overflows the persistent launch counts."""
    from mrt import _lib
    from mrt.tracer import GpuBvh, RayBuffer
    bufs, rays, _ = comb_batch(70)
    counts = []
    for k in (0, 1):
        tracer.set_config(waves_per_cu=4, backfill=k, lds_stack=8, wide=0, autotune=0)
        tracer.set_bvh(GpuBvh(bufs))
        rb = RayBuffer(rays, need_closest_hit=True)
        info = _lib.TraceInfo()
        rc = tracer.lib.mrt_tracer_trace_timed(tracer._h, rb.rays.data_ptr(), rb.results.data_ptr(), rb.size,
                                               _lib.MRT_TRACE_EXACT_RCP, None, None, C.byref(info))
        assert rc == _lib.MRT_ERR_STACK_OVERFLOW
        assert info.backfill == k
        counts.append(info.stack_overflows)
    assert counts[0] > 0 and counts[0] == counts[1]


# ---------------------------------------------------------------- residency
@pytest.mark.parametrize("cap", [1, 2, 3, 4, 5])
def test_residency_cap_is_reported(tracer, restore, cap):
    """waves_per_cu = 4 * cap caps a backfilled launch at cap workgroups per CU (dynamic LDS,
    confirmed by the occupancy query): last_info reports it, and the results are the oracle's."""
    bufs, rays, any_hit, want, _ = scene_setup("bunny", 320, 240, "primary")
    reps = -(-(cus() * 256 * 5 + 1) // len(rays))   # more rays than five workgroups per CU hold
    big, big_want = np.tile(rays, (reps, 1)), np.tile(want, (reps, 1))
    tracer.set_config(waves_per_cu=4 * cap, backfill=1, autotune=0)
    res = trace(tracer, bufs, big, False)
    info = tracer.last_info
    assert info["backfill"] == 1 and info["blocks_per_cu"] == cap
    assert info["grid_waves"] == backfill_grid_waves(len(big), 1)
    assert info["dyn_lds_bytes"] >= 0
    assert_matches_oracle(big, res, big_want, bufs, False)


def test_batch_that_fits_runs_the_persistent_plan(tracer, restore):
    bufs, rays, any_hit, want, _ = scene_setup("bunny", 320, 240, "primary")
    tracer.set_config(waves_per_cu=8, backfill=1, autotune=0)   # 131 072 resident lanes on 256 CUs
    n = min(len(rays), cus() * 512)
    res = trace(tracer, bufs, rays[:n], False)
    info = tracer.last_info
    assert info["backfill"] == 0 and info["dyn_lds_bytes"] == 0 and info["blocks_per_cu"] == 2
    assert info["grid_waves"] == cus() * 8
    assert_matches_oracle(rays[:n], res, want[:n], bufs, False)


# ---------------------------------------------------------------- saved schedule
def test_saved_schedule_carries_backfill_and_cap(tracer, restore):
    """A saved schedule with k = 1 and a cap of 2 workgroups per CU in the candidate's upper bits:
    the launch reports both, still reports the 16-bit autotune_candidate bench.schedule_name
    decodes, and computes what the same schedule computes on the persistent grid."""
    import bench
    from mrt import _lib
    from mrt.tracer import GpuBvh
    bufs, rays, any_hit, want, _ = scene_setup("bunny", 640, 480, "primary")
    tracer.set_config(autotune=1, waves_per_cu=0, backfill=0, lane_groups=1, num_queues=-1, lds_stack=16, wide=1,
                      tail_lanes=16)
    # variant_key (csrc/mrt_api.cpp): speculative | exact rcp | 16 LDS entries | exact 4-wide | tail
    variant = 2 | 4 | (1 << 4) | (1 << 6) | 256
    code16 = 12 | (1 << 8)   # 2 lane groups at slack 6 on the 8-waves/CU static schedule
    out = {}
    for name, code in (("persistent", code16), ("backfilled", code16 | (1 << 16) | (2 << 24))):
        tracer.set_bvh(GpuBvh(bufs))
        tracer.load_schedules([(len(rays), variant, code, _lib.MRT_TUNE_VERSION)])
        assert tracer.schedules() == [(len(rays), variant, code, _lib.MRT_TUNE_VERSION)]
        out[name] = trace(tracer, bufs, rays, False, bind=False)
        info = tracer.last_info
        assert info["autotune_locked"] == 1 and info["autotune_candidate"] == code16
        assert isinstance(bench.schedule_name(info["autotune_candidate"]), str)
        assert info["blocks_per_cu"] == 2
        if name == "backfilled":
            assert info["backfill"] == 1 and info["grid_waves"] == backfill_grid_waves(len(rays), 1)
        else:
            assert info["backfill"] == 0 and info["grid_waves"] == cus() * 8 and info["dyn_lds_bytes"] == 0
    assert bench.schedule_name(code16) == bench.schedule_name(tracer.last_info["autotune_candidate"])
    assert_matches_oracle(rays, out["persistent"], want, bufs, False)
    assert_matches_oracle(rays, out["backfilled"], want, bufs, False)
    assert np.array_equal(out["persistent"][:, 1], out["backfilled"][:, 1])


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("cfg", [dict(backfill=1, num_queues=1), dict(backfill=3, num_queues=8),
                                 dict(backfill=1, ray_sort=1), dict(backfill=65)],
                         ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_invalid_combinations_are_refused(tracer, restore, cfg):
    from mrt import _lib
    before = tracer.config()
    c = _lib.LaunchCfg(**{**before, **cfg})
    assert tracer.lib.mrt_tracer_set_config(tracer._h, C.byref(c)) == _lib.MRT_ERR_INVALID_ARG
    assert tracer.config() == before   # nothing was set, and no launch was made


def test_default_is_the_persistent_grid(tracer, restore):
    assert tracer.config()["backfill"] == 0
    tracer.set_config(backfill=2)
    assert tracer.config()["backfill"] == 2
    tracer.set_config(backfill=-1)
    assert tracer.config()["backfill"] == 0
