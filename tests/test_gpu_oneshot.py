"""One-shot launches (cfg.oneshot, cfg.deal_block): the backfilled grid of one ray per lane run by
the one-shot kernels (csrc/trace_kernel.hip, ONESHOT), whose lanes compute their ray once in closed
form (csrc/deal_common.hpp), contiguous or block-cyclic over the XCD groups. Same rays, same
results: every ray traced exactly once and equal to the oracle; what changes is the kernel, the
grid and which lane traces which ray. Every case runs at waves_per_cu = 4 (one workgroup per CU
resident), backfill = 1, oneshot = 1, autotune = 0."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import kat  # noqa: E402
import oracle_lib as O  # noqa: E402
from test_gpu_backfill import (RESIDENT_LANES_PER_CU, assert_matches_oracle, backfill_grid_waves, comb_batch, cus,  # noqa: E402
                               restore, trace, tracer)  # noqa: E402,F401
from test_gpu_parity import scene_setup  # noqa: E402

BASE = dict(waves_per_cu=4, backfill=1, oneshot=1, autotune=0)


def oneshot_grid_waves(n, b):
    """8 * ceil(c / 256) workgroups of four waves, c positions per XCD group (deal_common.hpp)."""
    if b == 0:
        c = (-(-n // 8) + 63) // 64 * 64
    else:
        c = -(-(-(-n // (1 << b))) // 8) << b
    return 8 * -(-c // 256) * 4


def resident_lanes():
    return cus() * RESIDENT_LANES_PER_CU


def assert_oneshot(info, n, b):
    assert info["oneshot"] == 1 and info["deal_block"] == b and info["backfill"] == 1
    assert info["grid_waves"] == oneshot_grid_waves(n, b)
    assert info["num_queues"] == 0 and info["stack_overflows"] == 0


# ---------------------------------------------------------------- every ray once, oracle parity
@pytest.mark.parametrize("tail", [0, 16])
@pytest.mark.parametrize("groups", [1, 2, 16])
@pytest.mark.parametrize("block", [0, 6, 10, 13])
def test_bunny_primary_every_ray_once(tracer, restore, block, groups, tail):
    """76 800 rays: the smallest oversubscribed grid on 256 CUs."""
    bufs, rays, any_hit, want, _ = scene_setup("bunny", 320, 240, "primary")
    tracer.set_config(**BASE, deal_block=block, lane_groups=groups, tail_lanes=tail)
    res = trace(tracer, bufs, rays, any_hit)
    assert_matches_oracle(rays, res, want, bufs, any_hit)
    if len(rays) > resident_lanes():
        assert_oneshot(tracer.last_info, len(rays), block)
    else:
        assert tracer.last_info["oneshot"] == 0 and tracer.last_info["deal_block"] == 0


def test_conference_ao_any_hit(tracer, restore):
    bufs, rays, any_hit, want, _ = scene_setup("conference", 640, 480, "ao")
    assert any_hit
    tracer.set_config(**BASE, deal_block=10, lane_groups=2, tail_lanes=16)
    res = trace(tracer, bufs, rays, any_hit)
    assert_matches_oracle(rays, res, want, bufs, any_hit)
    if len(rays) > resident_lanes():
        assert_oneshot(tracer.last_info, len(rays), 10)


# ---------------------------------------------------------------- ragged prefixes
@pytest.mark.parametrize("block", [6, 10, 13])
@pytest.mark.parametrize("extra", [1, 64, 70001, 73729], ids=["resident+1", "resident+64", "70001", "73729"])
def test_ragged_prefixes(tracer, restore, extra, block):
    """Block counts that are no multiple of 8 and last blocks of one ray; the deal's chunk exceeds
    ceil(n / 8), so lanes past the batch must trace nothing."""
    bufs, rays, any_hit, want, _ = scene_setup("bunny", 320, 240, "primary")
    n = resident_lanes() + extra if extra <= 64 else extra
    n = min(n, len(rays))
    tracer.set_config(**BASE, deal_block=block)
    res = trace(tracer, bufs, rays[:n], False)
    assert_matches_oracle(rays[:n], res, want[:n], bufs, False)
    if n > resident_lanes():
        assert_oneshot(tracer.last_info, n, block)
    else:
        assert tracer.last_info["oneshot"] == 0


def test_prefix_that_fits_the_resident_grid_runs_todays_launch(tracer, restore):
    bufs, rays, any_hit, want, _ = scene_setup("bunny", 320, 240, "primary")
    n = min(len(rays), resident_lanes())
    tracer.set_config(**BASE, deal_block=10)
    res = trace(tracer, bufs, rays[:n], False)
    info = dict(tracer.last_info)
    assert info["oneshot"] == 0 and info["deal_block"] == 0 and info["backfill"] == 0 and info["dyn_lds_bytes"] == 0
    tracer.set_config(**{**BASE, "oneshot": 0}, deal_block=0)
    ref = trace(tracer, bufs, rays[:n], False)
    assert np.array_equal(res, ref)
    assert {k: v for k, v in info.items() if k != "kernel_ms"} == \
           {k: v for k, v in tracer.last_info.items() if k != "kernel_ms"}
    assert_matches_oracle(rays[:n], res, want[:n], bufs, False)


def test_variant_without_a_one_shot_sibling_runs_todays_kernel(tracer, restore):
    """lds_stack 8 has no one-shot kernels: the backfilled launch of the persistent kernel, reported."""
    bufs, rays, any_hit, want, _ = scene_setup("bunny", 320, 240, "primary")
    tracer.set_config(**BASE, deal_block=10, lds_stack=8)
    res = trace(tracer, bufs, rays, False)
    assert_matches_oracle(rays, res, want, bufs, False)
    info = tracer.last_info
    assert info["oneshot"] == 0 and info["deal_block"] == 0 and info["lds_stack_entries"] == 8
    if len(rays) > resident_lanes():
        assert info["backfill"] == 1 and info["grid_waves"] == backfill_grid_waves(len(rays), 1)


# ---------------------------------------------------------------- deep stacks
@pytest.mark.parametrize("tail", [0, 16])
@pytest.mark.parametrize("depth", [40, 63])
def test_spill_slab_of_the_one_shot_grid(tracer, restore, depth, tail):
    """Deep comb rays push past the 16-entry LDS ring into the spill slab, indexed by the launched
    lane of the one-shot grid. The hand answer (which the oracle reproduces), no overflow."""
    bufs, rays, expect = comb_batch(depth)
    want, _, _ = O.trace(rays[:1], *bufs)
    assert want[0, 0] == expect[0] and want[0, 1] == kat.f2i(expect[1])
    tracer.set_config(**BASE, deal_block=10, lds_stack=16, wide=1, tail_lanes=tail)
    res = trace(tracer, bufs, rays, False)
    assert_oneshot(tracer.last_info, len(rays), 10)
    assert tracer.last_info["lds_stack_entries"] == 16
    assert (res[:, 0] == want[0, 0]).all() and (res[:, 1] == want[0, 1]).all()


def test_overflow_reported_as_by_the_persistent_launch(tracer, restore):
    """A comb deeper than the wide traversal's capacity cannot be bound with wide nodes; the binary
    order overflows the reference's 64 entries at depth 70 and has no one-shot kernels, so a
    cfg.oneshot launch of it is today's launch and counts exactly what the persistent one counts."""
    from mrt import _lib
    from mrt.tracer import GpuBvh, RayBuffer
    bufs, rays, _ = comb_batch(70)
    counts = []
    for cfg in (dict(backfill=0, oneshot=0), dict(backfill=1, oneshot=1)):
        tracer.set_config(waves_per_cu=4, lds_stack=16, wide=0, autotune=0, deal_block=0, **cfg)
        tracer.set_bvh(GpuBvh(bufs))
        rb = RayBuffer(rays, need_closest_hit=True)
        info = _lib.TraceInfo()
        rc = tracer.lib.mrt_tracer_trace_timed(tracer._h, rb.rays.data_ptr(), rb.results.data_ptr(), rb.size,
                                               _lib.MRT_TRACE_EXACT_RCP, None, None, C.byref(info))
        assert rc == _lib.MRT_ERR_STACK_OVERFLOW
        assert info.oneshot == 0 and info.backfill == cfg["backfill"]
        counts.append(info.stack_overflows)
    assert counts[0] > 0 and counts[0] == counts[1]


# ---------------------------------------------------------------- saved schedule
def test_saved_schedule_carries_the_one_shot_bits(tracer, restore):
    """Bit 23 (one-shot) and bits 27-30 (the deal's block log2) of a saved candidate: exported as
    imported, reported by the launch, autotune_candidate still the 16-bit code, and the same t as
    the same schedule without the bits."""
    import bench
    from mrt import _lib
    from mrt.tracer import GpuBvh
    bufs, rays, any_hit, want, _ = scene_setup("bunny", 640, 480, "primary")
    tracer.set_config(autotune=1, waves_per_cu=0, backfill=0, oneshot=0, deal_block=0, lane_groups=1, num_queues=-1,
                      lds_stack=16, wide=1, tail_lanes=16)
    variant = 2 | 4 | (1 << 4) | (1 << 6) | 256   # variant_key (csrc/mrt_api.cpp), as in test_gpu_backfill
    code16 = 12 | (1 << 8)                        # 2 lane groups at slack 6 on the 8-waves/CU static schedule
    backfilled = code16 | (1 << 16) | (2 << 24)
    out = {}
    for name, code in (("backfilled", backfilled), ("oneshot", backfilled | (1 << 23) | (10 << 27))):
        tracer.set_bvh(GpuBvh(bufs))
        tracer.load_schedules([(len(rays), variant, code, _lib.MRT_TUNE_VERSION)])
        assert tracer.schedules() == [(len(rays), variant, code, _lib.MRT_TUNE_VERSION)]
        out[name] = trace(tracer, bufs, rays, False, bind=False)
        info = tracer.last_info
        assert info["autotune_locked"] == 1 and info["autotune_candidate"] == code16
        assert isinstance(bench.schedule_name(info["autotune_candidate"]), str)
        assert info["blocks_per_cu"] == 2 and info["backfill"] == 1
        if name == "oneshot":
            assert info["oneshot"] == 1 and info["deal_block"] == 10
            assert info["grid_waves"] == oneshot_grid_waves(len(rays), 10)
        else:
            assert info["oneshot"] == 0 and info["deal_block"] == 0
            assert info["grid_waves"] == backfill_grid_waves(len(rays), 1)
    assert_matches_oracle(rays, out["oneshot"], want, bufs, False)
    assert np.array_equal(out["oneshot"][:, 1], out["backfilled"][:, 1])


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("cfg", [dict(oneshot=1, backfill=0), dict(oneshot=1, backfill=2),
                                 dict(oneshot=1, backfill=1, num_queues=1), dict(oneshot=1, backfill=1, ray_sort=1),
                                 dict(oneshot=2, backfill=1), dict(oneshot=0, backfill=1, deal_block=10),
                                 dict(oneshot=1, backfill=1, deal_block=5), dict(oneshot=1, backfill=1, deal_block=16),
                                 dict(oneshot=1, backfill=1, deal_block=1024)],
                         ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_invalid_combinations_are_refused(tracer, restore, cfg):
    from mrt import _lib
    before = tracer.config()
    c = _lib.LaunchCfg(**{**before, **cfg})
    assert tracer.lib.mrt_tracer_set_config(tracer._h, C.byref(c)) == _lib.MRT_ERR_INVALID_ARG
    assert tracer.config() == before   # nothing was set, and no launch was made


def test_defaults_are_off(tracer, restore):
    assert tracer.config()["oneshot"] == 0 and tracer.config()["deal_block"] == 0
    tracer.set_config(backfill=1, oneshot=1, deal_block=11)
    assert (tracer.config()["oneshot"], tracer.config()["deal_block"]) == (1, 11)
    tracer.set_config(oneshot=-1, deal_block=-1)
    assert tracer.config()["oneshot"] == 0 and tracer.config()["deal_block"] == 0


# ---------------------------------------------------------------- determinism
def test_two_identical_launches_are_byte_identical(tracer, restore):
    bufs, rays, any_hit, want, _ = scene_setup("bunny", 320, 240, "primary")
    tracer.set_config(**BASE, deal_block=10, lane_groups=2, tail_lanes=16)
    a = trace(tracer, bufs, rays, False)
    b = trace(tracer, bufs, rays, False, bind=False)
    assert a.tobytes() == b.tobytes()
