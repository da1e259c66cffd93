"""Leaves of 9 to 33 triangles on the device: kat.leaf_gallery() and the four natural trees of
leaf_util (SBVHs built with min_leaf 17 and 33), whose CPU side is tests/test_leaf_sizes.py.
Every kernel of mrt_trace_kernel_keys traces the gallery and random1500-min17 in
test_gpu_variants.py, and Tracer.optimize runs on the natural trees in test_gpu_optimize.py
(optimize_util.BIG_LEAVES); here:

  * the frontier tail on its own (wide 1, tail_lanes 16): a leaf's remainder goes back on the
    list as a new ref with its count less four, so leaves of 5, 8 / 9, 12 / 13, 15, 16 (count 0:
    the terminator), 17, 20 and 33 walk every branch of that arithmetic. At spec_slack 63 a batch
    of at most 16 rays is in the tail after its first node step: every gallery ray 1, 5 and 16
    times over, and the shuffled gallery 3 and 16 rays at a time; the whole gallery runs the main
    loop first. Closest hits are the hand answers bit for bit, any hits within the allowed sets;
  * set_bvh(on_device=True) derives the host bind's 4-wide bytes (counts 9 to 15 and 0 included),
    bind_info and plan, at wide 0, 1 and 2;
  * Tracer.refit equals the host refit, a refit back restores every byte, and traces after the
    refit equal the oracle of the refitted tree;
  * the kernels of test_gpu_ref_trees.KERNELS (backfill and one-shot among them) on the two
    trees with leaves of up to 33.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import kat  # noqa: E402
import leaf_util as LU  # noqa: E402
import oracle_lib as O  # noqa: E402
import refit_util as R  # noqa: E402
import test_gpu_ref_trees as RT  # noqa: E402
from mrt.tracer import GpuBvh, RayBuffer, Tracer, refit_plan  # noqa: E402

SENTINEL = 0x5A5A5A5A
TAIL = 256   # the kernel key's bit of the frontier-tail variants (include/mrt.h)
NATURAL = list(LU.NATURAL)


@pytest.fixture(scope="module")
def tracer():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Tracer(0)


@pytest.fixture()
def restore(tracer):
    saved = tracer.config()
    yield
    tracer.set_config(**saved)


def gpu(bufs):
    return GpuBvh(tuple(np.array(b) for b in bufs))


def download(g):
    torch.cuda.synchronize()
    return g.nodes.cpu().numpy(), g.woop.cpu().numpy(), g.tri_index.cpu().numpy()


# ---- the frontier tail -------------------------------------------------------------------------
def check_gallery(res, n, any_hit):
    """res: the gallery's n rays tiled cyclically. Closest: the hand answer; any hit: the allowed set."""
    g = LU.gallery()
    assert (res[:, 2:] == SENTINEL).all(), "RayResult padding was overwritten"
    for i, mode, exact, allowed in g["hand"]:
        if mode != any_hit or i >= len(res):
            continue
        got = {(int(k), int(t)) for k, t in res[i::n, :2]}
        ok = {exact} if allowed is None else allowed
        assert got <= {(k, kat.f2i(t)) for k, t in ok}, f"ray {i} ({describe(i)}): {got}, allowed {ok}"


def describe(i):
    for kind, n, _, idx in LU.gallery()["leaves"]:
        if i in idx:
            return f"{kind} leaf of {n}, its ray {idx.index(i)}"


# spec_slack: a wave turns from its inner nodes to its postponed leaves once at most this many
# lanes are without one, and leaves the main loop for the tail only between two such turns. At the
# default (2) a batch of one ray goes to the tail after its first node step, but five copies walk
# down together and test their leaf in the main loop's counted loop. At 63 every node step is a
# turn: any batch of at most tail_lanes rays is in the tail after its first step and meets its leaf
# there; 17 copies stay in the main loop, which they leave together.
SLACKS = [-1, 63]


def tail_config(tracer, slack):
    tracer.set_config(wide=1, tail_lanes=16, autotune=0, spec_slack=slack)
    tracer.set_bvh(gpu(LU.gallery()["bufs"]))
    assert tracer.bind_info()["wide_format"] == 1


def trace_in_launches(tracer, rays, size, any_hit):
    """rays traced `size` at a time, one blocking launch each, into sentinel-filled results."""
    rb = RayBuffer(rays, need_closest_hit=not any_hit)
    rb.results.fill_(SENTINEL)
    for lo in range(0, len(rays), size):
        tracer.trace_batch(rb.view(lo, min(lo + size, len(rays))), exact_rcp=True)
        assert tracer.last_info["stack_overflows"] == 0 and tracer.last_kernel_key & TAIL
    return rb.results_numpy()


@pytest.mark.parametrize("any_hit", [False, True], ids=["closest", "any"])
@pytest.mark.parametrize("slack", SLACKS, ids=["slack-default", "slack63"])
@pytest.mark.parametrize("copies", [1, 5, 16, 17])
def test_frontier_tail_one_ray_at_a_time(tracer, restore, copies, slack, any_hit):
    """Every ray of every leaf in a launch of its own, `copies` times over: one group of 64 lanes
    (16 entries a step), eight groups of 8, sixteen of 4 (one entry a step, four triangles)."""
    g = LU.gallery()
    n = len(g["rays"])
    tail_config(tracer, slack)
    res = trace_in_launches(tracer, np.repeat(g["rays"], copies, axis=0), copies, any_hit)
    check_gallery(res.reshape(n, copies, 4).transpose(1, 0, 2).reshape(-1, 4), n, any_hit)   # tiled cyclically


@pytest.mark.parametrize("any_hit", [False, True], ids=["closest", "any"])
@pytest.mark.parametrize("size", [3, 16])
def test_frontier_tail_on_leaves_of_mixed_sizes(tracer, restore, size, any_hit):
    """The gallery's rays shuffled and traced `size` at a time at spec_slack 63: a wave's rays are
    in the tail together on leaves of different lengths, the short ones finish first and the
    groups of the others widen mid-leaf (a remainder ref moves with its window)."""
    g = LU.gallery()
    n = len(g["rays"])
    order = np.random.default_rng(33).permutation(n)
    tail_config(tracer, 63)
    res = np.empty((n, 4), np.int32)
    res[order] = trace_in_launches(tracer, g["rays"][order], size, any_hit)
    check_gallery(res, n, any_hit)


@pytest.mark.parametrize("any_hit", [False, True], ids=["closest", "any"])
@pytest.mark.parametrize("slack", SLACKS, ids=["slack-default", "slack63"])
@pytest.mark.parametrize("total", [130, 386])
def test_frontier_tail_after_the_main_loop(tracer, restore, total, slack, any_hit):
    """130 rays: two waves and two rays of the row leaves; 386: the whole gallery and two rays
    more. The rays of a full wave walk down together and test their leaves in the tail variant's
    main loop; only the last two rays finish in the tail."""
    g = LU.gallery()
    n = len(g["rays"])
    tail_config(tracer, slack)
    res = trace_in_launches(tracer, np.resize(g["rays"], (total, 8)), total, any_hit)
    check_gallery(res, n, any_hit)


# ---- derived data on the device ------------------------------------------------------------------
def strip(info):
    return {k: v for k, v in info.items() if k != "bind_ms"}


@pytest.mark.parametrize("wide", [0, 1, 2])
@pytest.mark.parametrize("name", LU.NAMES)
def test_device_bind_equals_host_bind(tracer, restore, name, wide):
    bufs = LU.buffers(name)
    tracer.set_config(wide=wide)
    tracer.set_bvh(gpu(bufs))
    want, info, plan = tracer.wide_nodes(), tracer.bind_info(), refit_plan(bufs[0], wide=wide == 1)
    assert info["wide_format"] == wide and (want.size > 0) == (wide != 0)
    tracer.set_bvh(gpu(bufs), on_device=True)
    got = tracer.wide_nodes()
    assert got.size == want.size and R.same_bits_or_nan(got, want), RT.first_difference(got, want)
    assert strip(tracer.bind_info()) == strip(info)
    installed = tracer.refit_plan()
    assert installed is not None
    assert np.array_equal(installed[0], plan[0]) and np.array_equal(installed[1], plan[1])
    if wide == 1:
        assert np.array_equal(installed[2], plan[2])
    else:
        assert installed[2] is None
    d = tracer.derive_info()
    assert d["on_device_plan"] == 1 and d["on_device_wide"] == (1 if wide == 1 else 0)


# ---- refit ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def moved(name):
    """(vertices, moved vertices, triangles, built buffers, host-refitted buffers), computed once."""
    v, t, bufs = LU.built(name)
    v2 = R.displaced(v)
    return v, v2, t, bufs, R.host_refit(bufs, v2, t)


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("name", NATURAL)
def test_device_refit_equals_host_refit_and_back(tracer, restore, name, wide):
    v, v2, t, bufs, want = moved(name)
    tracer.set_config(wide=wide)
    g = gpu(bufs)
    tracer.set_bvh(g)
    wide_before = tracer.wide_nodes()
    tracer.refit(v2, t)
    nodes, woop, tri = download(g)
    assert np.array_equal(woop, want[1])
    assert R.same_nodes(nodes, want[0])
    assert np.array_equal(tri, bufs[2])
    assert tracer.refit_info()["skipped_refs"] == 0
    if wide:
        R.check_wide(wide_before, tracer.wide_nodes(), bufs[0], nodes)
    else:
        assert tracer.wide_nodes().size == 0
    # back at the built vertices: the Woop rows are the built ones again, the boxes those of a host
    # refit of the built tree to its own vertices (whole triangles' boxes: the builder clips), and a
    # second round trip changes not a byte
    tracer.refit(v, t)
    back = download(g)
    home = R.host_refit(bufs, v, t)
    assert np.array_equal(back[1], bufs[1]) and np.array_equal(back[2], bufs[2])
    assert R.same_nodes(back[0], home[0])
    wide_home = tracer.wide_nodes()
    tracer.refit(v2, t)
    tracer.refit(v, t)
    again = download(g)
    assert all(np.array_equal(a, b) for a, b in zip(again, back))
    assert np.array_equal(tracer.wide_nodes(), wide_home)
    assert tracer.refit_info()["skipped_refs"] == 0


@pytest.mark.parametrize("mode", ["wide0", "wide1", "wide2", "lockstep_off"])
@pytest.mark.parametrize("name", NATURAL)
def test_traces_after_a_refit_equal_the_oracle(tracer, restore, name, mode):
    _, v2, t, bufs, (nodes, woop, tri) = moved(name)
    wide = {"wide0": 0, "wide1": 1, "wide2": 2, "lockstep_off": 1}[mode]
    tracer.set_config(wide=wide)
    tracer.set_bvh(gpu(bufs))
    tracer.refit(v2, t)
    if mode == "wide2":
        assert tracer.bind_info()["wide_format"] == 2   # derived again from the refitted nodes
    rays = R.frame_rays(v2)
    rb = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(rb, exact_rcp=True, speculative=mode != "lockstep_off")
    want, _, _ = O.trace(rays, nodes, woop, tri)
    assert (want[:, 0] != -1).sum() >= 16
    got = rb.results_numpy()
    assert np.array_equal(got[:, 1], want[:, 1])
    diff = np.nonzero(got[:, 0] != want[:, 0])[0]
    assert len(O.invalid_hits(rays, got, woop, tri, which=diff)) == 0
    ah = RayBuffer(rays, need_closest_hit=False)
    tracer.trace_batch(ah, exact_rcp=True, speculative=mode != "lockstep_off")
    brute = O.brute_force(rays, woop, tri, any_hit=True)
    assert np.array_equal(ah.results_numpy()[:, 0] == -1, brute[:, 0] == -1)


# ---- the kernels of test_gpu_ref_trees on leaves of up to 33 --------------------------------------
@functools.lru_cache(maxsize=None)
def answers(name):
    rays = LU.rays_for(name)
    bufs = LU.buffers(name)
    closest = O.trace(rays, *bufs, threads=8)[0]
    anyhit = O.trace(rays, *bufs, any_hit=True, threads=8)[0]
    for a in (closest, anyhit):
        a.setflags(write=False)
    return rays, closest, anyhit


@pytest.mark.parametrize("kernel", list(RT.KERNELS))
@pytest.mark.parametrize("name", ["random1500-min33", "hairball3-min33"])
def test_the_kernels_of_the_reference_trees_equal_the_oracle(tracer, restore, name, kernel):
    rays, closest, anyhit = answers(name)
    bufs = LU.buffers(name)
    assert (closest[:, 0] != -1).sum() >= 32 and (closest[3072:, 0] != -1).any()
    RT.check_kernel(tracer, kernel, bufs, rays, closest, anyhit)
