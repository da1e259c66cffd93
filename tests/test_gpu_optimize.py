"""Treelet restructuring on the device (mrt_tracer_optimize / Tracer.optimize,
csrc/treelet_kernel.hip) against its CPU statement (Bvh.optimize, tests/test_optimize.py).

  * device == host: the bound nodes after the call are the host's byte for byte, at 1 and 3
    rounds, on every tree of optimize_util.TREES; Woop rows and triIndex are untouched;
  * the derived data are the new tree's: the 4-wide array, the installed plan, the stack bound;
  * traces on the new tree: the per-lane exact order bit for bit with the oracle, counters
    included; the production kernels' closest t as before the call, any-hit answers genuine;
  * a refit straight after needs no plan step and equals the host refit of the optimized tree;
  * settled schedules survive; the three refusals leave every byte.

"random" 9000 at max_leaf_size 4 (3242 records) has height levels 1-6 (755 .. 68 records) above
the 64-record threshold between a launch per level and the one-workgroup tail, which takes the
other eight; at max_leaf_size 1 level 1 has 1988 records, more than the refit's 1024. In "copies"
every Morton code is equal; "one" and "n_eq_l_plus_1" are a single record. The four trees of
leaf_util.NATURAL (optimize_util.BIG_LEAVES) have leaves of up to 17 and up to 33 triangles: the
derived leaf counts of the new tree include 9 to 15 and the 0 of a longer leaf.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import optimize_util as U  # noqa: E402
import oracle_lib as O  # noqa: E402
import refit_util as R  # noqa: E402
from mrt import _lib  # noqa: E402
from mrt.tracer import GpuBvh, RayBuffer, Tracer, refit_plan  # noqa: E402


@pytest.fixture(scope="module")
def tracer():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    t = Tracer(0)
    t.set_config(wide=1)
    return t


def bind(tracer, bufs, wide=1):
    tracer.set_config(wide=wide)
    g = GpuBvh(tuple(np.array(b) for b in bufs))
    tracer.set_bvh(g)
    return g


def download(g):
    torch.cuda.synchronize()
    return g.nodes.cpu().numpy(), g.woop.cpu().numpy(), g.tri_index.cpu().numpy()


def host_wide(nodes, woop):
    """mrt_derive_wide_nodes, form 1, leaf counts from the Woop array: what a bind derives."""
    lib = _lib.trace_lib()
    n, w = np.ascontiguousarray(nodes, np.int32), np.ascontiguousarray(woop, np.int32)
    size = C.c_int64()
    assert lib.mrt_derive_wide_nodes(n.ctypes.data, n.nbytes, w.ctypes.data, w.nbytes, 1, None, 0, C.byref(size)) == 0
    wide = np.zeros(size.value // 4, np.uint32)
    assert lib.mrt_derive_wide_nodes(n.ctypes.data, n.nbytes, w.ctypes.data, w.nbytes, 1, wide.ctypes.data, wide.nbytes,
                                     C.byref(size)) == 0
    return wide


# ---- 1. device equals host, 2. derived data ------------------------------------------------------
@pytest.mark.parametrize("rounds", U.ROUNDS)
@pytest.mark.parametrize("name", list(U.TREES))
def test_device_equals_host(tracer, name, rounds):
    _, _, bufs = U.TREES[name]()
    want, host_info = U.host_optimized(name, rounds)
    g = bind(tracer, bufs)
    info = tracer.optimize(rounds)
    nodes, woop, tri = download(g)
    assert np.array_equal(nodes, want)
    assert np.array_equal(woop, bufs[1]) and np.array_equal(tri, bufs[2])
    assert info["rounds"] == rounds and info["levels"] == host_info["levels"]
    assert info["considered"] == host_info["considered"] and info["rewritten"] == host_info["rewritten"]
    assert info["wall_ms"] > 0 and info["scratch_bytes"] >= 48 * len(want) // 16
    # the derived data are the new tree's
    plan = refit_plan(want)
    got = tracer.refit_plan()
    assert got is not None and all(np.array_equal(a, b) for a, b in zip(got, plan))
    assert tracer.refit_info()["levels"] == len(plan[1]) - 1
    assert R.same_bits_or_nan(tracer.wide_nodes(), host_wide(want, bufs[1]))
    bound = tracer.bind_info()
    fresh = Tracer(0)
    fresh.set_config(wide=1)
    fresh.set_bvh(GpuBvh(tuple(np.array(b) for b in (want, bufs[1], bufs[2]))))
    expect = fresh.bind_info()
    assert {k: bound[k] for k in bound if k != "bind_ms"} == {k: expect[k] for k in expect if k != "bind_ms"}


def test_levels_above_the_launch_thresholds(tracer):
    for name, above in (("random9000-L4", 64), ("random9000-L1", 1024)):
        _, _, bufs = U.TREES[name]()
        _, offsets, _ = refit_plan(bufs[0], wide=False)
        upper = np.diff(offsets)[1:]
        assert upper[0] > above
        bind(tracer, bufs)
        info = tracer.optimize(1)
        # one launch per level above 64 records, one workgroup for the rest
        assert info["launches"] == int((upper > 64).sum()) + int((upper <= 64).any())
        assert info["device_ms"] > 0


def test_wide_0_and_2_behave_as_a_device_bind(tracer):
    _, _, bufs = U.TREES["random1500-L4"]()
    want, _ = U.host_optimized("random1500-L4", 1)
    for wide in (0, 2):
        g = bind(tracer, bufs, wide)
        tracer.optimize(1)
        assert np.array_equal(download(g)[0], want)
        assert tracer.bind_info()["wide_format"] == wide
        got = tracer.refit_plan()
        assert np.array_equal(got[0], refit_plan(want)[0])
        d = tracer.derive_info()
        assert d["on_device_plan"] == 1 and d["on_device_wide"] == 0
    tracer.set_config(wide=1)


# ---- 3. traces ---------------------------------------------------------------------------------------
def check_closest(rays, got, want, woop, tri):
    assert np.array_equal(got[:, 1], want[:, 1])
    diff = np.nonzero(got[:, 0] != want[:, 0])[0]
    assert len(O.invalid_hits(rays, got, woop, tri, which=diff)) == 0


TRACED = ["hairball3-L4", "random1500-L1", "random9000-L4", "copies-L1", "flat-L4", "sbvh-hairball3", "edge-signed_zero",
          "edge-nonfinite", "one-L4"] + U.BIG_LEAVES


@pytest.mark.parametrize("name", TRACED)
def test_per_lane_exact_mode_is_bit_identical_with_counters(tracer, name):
    _, _, bufs = U.TREES[name]()
    want_nodes, _ = U.host_optimized(name, 3)
    rays, min_hits = U.rays_for(name)
    bind(tracer, bufs)
    tracer.optimize(3)
    for any_hit in (False, True):
        want, st, _ = O.trace(rays, want_nodes, bufs[1], bufs[2], any_hit=any_hit, stats=True)
        assert (want[:, 0] != -1).sum() >= min_hits
        rb = RayBuffer(rays, need_closest_hit=not any_hit)
        tracer.trace_batch(rb, exact_rcp=True, speculative=False, stats=True)
        assert np.array_equal(rb.results_numpy()[:, :2], want[:, :2])
        assert np.array_equal(rb.stats.cpu().numpy()[:, :3], st[:, :3])


@pytest.mark.parametrize("mode", ["wide0", "wide1", "wide2", "wide1_fast_rcp"])
@pytest.mark.parametrize("name", TRACED)
def test_production_kernels_see_the_same_scene(tracer, name, mode):
    """Closest t bit for bit what the same kernel found before the call (the Woop rows are the
    same, so a triangle's t is), ids up to exact-t ties, any-hit answers genuine hits."""
    _, _, bufs = U.TREES[name]()
    rays, min_hits = U.rays_for(name)
    wide = {"wide0": 0, "wide1": 1, "wide2": 2, "wide1_fast_rcp": 1}[mode]
    exact = mode != "wide1_fast_rcp"
    bind(tracer, bufs, wide)
    before = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(before, exact_rcp=exact)
    before = before.results_numpy().copy()
    assert (before[:, 0] != -1).sum() >= min_hits
    tracer.optimize(3)
    after = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(after, exact_rcp=exact)
    ulps = 0 if exact else 1
    got = after.results_numpy()
    assert np.array_equal(got[:, 1], before[:, 1])
    diff = np.nonzero(got[:, 0] != before[:, 0])[0]
    assert len(O.invalid_hits(rays, got, bufs[1], bufs[2], which=diff, rcp_ulps=ulps)) == 0
    ah = RayBuffer(rays, need_closest_hit=False)
    tracer.trace_batch(ah, exact_rcp=exact)
    res = ah.results_numpy()
    assert np.array_equal(res[:, 0] == -1, before[:, 0] == -1)
    assert len(O.invalid_hits(rays, res, bufs[1], bufs[2], rcp_ulps=ulps)) == 0
    tracer.set_config(wide=1)


# ---- 4. refit after optimize ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random1500-L4", "random9000-L4", "sbvh-hairball3"])
def test_a_refit_after_optimize_equals_the_host_refit(tracer, name):
    v, t, bufs = U.TREES[name]()
    want_nodes, _ = U.host_optimized(name, 1)
    v2 = R.displaced(v)
    want = R.host_refit((want_nodes, bufs[1], bufs[2]), v2, t)
    g = bind(tracer, bufs)
    assert tracer.refit_plan() is None
    tracer.optimize(1)
    levels = len(refit_plan(want_nodes, wide=False)[1]) - 1
    assert tracer.refit_info()["levels"] == levels   # installed: no refit has run, no plan copy
    wide_before = tracer.wide_nodes()
    tracer.refit(v2, t)
    nodes, woop, tri = download(g)
    assert np.array_equal(woop, want[1]) and R.same_nodes(nodes, want[0]) and np.array_equal(tri, bufs[2])
    R.check_wide(wide_before, tracer.wide_nodes(), want_nodes, nodes)
    assert tracer.refit_info()["skipped_refs"] == 0
    # and optimizing the refitted tree equals the host doing the same
    again = tracer.optimize(1)
    host = U.mrt.Bvh.from_buffers(*want)
    host_info = host.optimize(1)
    assert np.array_equal(download(g)[0], host.buffers()[0]) and again["rewritten"] == host_info["rewritten"]


# ---- 5. schedules ------------------------------------------------------------------------------------------
def test_settled_schedules_survive(tracer):
    _, _, bufs = U.TREES["random1500-L4"]()
    rays, _ = U.rays_for("random1500-L4")
    bind(tracer, bufs)
    rb = RayBuffer(np.array(rays), need_closest_hit=True)
    for _ in range(700):   # settle this batch size's schedule
        tracer.trace_batch(rb, exact_rcp=True)
        if tracer.last_info["autotune_locked"]:
            break
    saved = tracer.schedules()
    assert any(n == rb.size for n, _, _, _ in saved)
    tracer.optimize(2)
    assert tracer.schedules() == saved
    tracer.trace_batch(rb, exact_rcp=True)
    assert tracer.last_info["autotune_locked"]


# ---- 6. refusals ---------------------------------------------------------------------------------------------
def test_the_three_refusals_leave_every_byte(tracer):
    lib = _lib.trace_lib()
    h = C.c_void_p()
    assert lib.mrt_tracer_create(0, C.byref(h)) == 0
    assert lib.mrt_tracer_optimize(h, None, None) == _lib.MRT_ERR_NOT_BOUND
    info = _lib.OptimizeInfo()
    assert lib.mrt_tracer_optimize_info(h, C.byref(info)) == 0 and info.rounds == 0
    lib.mrt_tracer_destroy(h)

    _, _, bufs = U.TREES["random1500-L4"]()
    g = bind(tracer, bufs)
    wide = tracer.wide_nodes()
    for rounds in (-1, 9):
        params = _lib.OptimizeParams(rounds=rounds)
        assert lib.mrt_tracer_optimize(tracer._h, C.byref(params), None) == _lib.MRT_ERR_INVALID_ARG
    assert np.array_equal(download(g)[0], bufs[0]) and np.array_equal(tracer.wide_nodes(), wide)

    # a chain of 1100 records: more depth levels than the device derivation takes
    import test_gpu_refit as TR
    verts, tris, chain = TR.chain_tree(_lib.MRT_DERIVE_MAX_LEVELS + 76, np.random.default_rng(9))
    chain = R.host_refit(chain, verts, tris)
    g = bind(tracer, chain)
    wide, bound = tracer.wide_nodes(), tracer.bind_info()
    assert lib.mrt_tracer_optimize(tracer._h, None, None) == _lib.MRT_ERR_TOO_LARGE
    assert np.array_equal(download(g)[0], chain[0]) and np.array_equal(tracer.wide_nodes(), wide)
    assert tracer.bind_info() == bound   # the bind stands
