"""Device LBVH build and device refit (csrc/lbvh_kernel.hip, csrc/refit_kernel.hip) at the numeric
edges of geometry and of size, against the host build / refit and the CPU oracle.

Geometry (lbvh_util.edge_geometry): zero-area triangles, an 800-triangle soup scaled by 2^-31,
2^-40, 2^-130 (denormal), 2^30 and 2^40, NaN and infinite vertices, a flat grid with signed zeros.

  * device build == host build at max_leaf_size 1, 4, 8: sizes, triIndex, Woop rows and nodes,
    a NaN equal to a NaN (the bits of a NaN an operation makes differ between x86 and gfx950,
    refit_util.same_bits_or_nan); two device builds give identical bytes, NaNs included;
  * device refit == host refit: the soup's tree refitted to each geometry at wide 0 and 1, the
    exact 4-wide array gathered from the refitted boxes, and back to the soup's bytes;
  * traces equal the oracle (t bit for bit, ids up to exact-t ties, any-hit as brute force) at
    wide 0, 1, 2 and in the per-lane order. With NaN or infinite vertices the binary orders are
    still bit-identical; the wide orders must report genuine hits, none farther than the
    oracle's, and hit every ray the oracle hits;
  * the wide = 2 fallback: a refit or build whose boxes are not finite derives the exact 4-wide
    array, which stays after a refit back to finite vertices;
  * sizes: 2..1025 triangles around the 256-thread workgroup boundaries of the hierarchy, flag,
    record and slot kernels, and 262 145 triangles (the bounds kernel's grid-stride loop, rocPRIM's
    large sort and scan, a refit with several per-level launches).
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mrt  # noqa: E402
import lbvh_util as L  # noqa: E402
import oracle_lib as O  # noqa: E402
import refit_util as R  # noqa: E402
from mrt.tracer import GpuBvh, RayBuffer, Tracer, refit_plan  # noqa: E402

SOUP_KINDS = [k for k in L.EDGE_GEOMETRY if k != "signed_zero"]   # the soup's topology
FINITE_KINDS = [k for k in L.EDGE_GEOMETRY if k != "nonfinite"]
MODES = {"wide0": 0, "wide1": 1, "wide2": 2, "lockstep_off": 1}


@pytest.fixture(scope="module")
def tracer():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Tracer(0)


def download(g):
    torch.cuda.synchronize()
    return g.nodes.cpu().numpy(), g.woop.cpu().numpy(), g.tri_index.cpu().numpy()


def bind(tracer, bufs, wide):
    tracer.set_config(wide=wide)
    g = GpuBvh(tuple(np.array(b) for b in bufs))
    tracer.set_bvh(g)
    return g


def same_buffers(got, want):
    """Sizes and triIndex equal, Woop rows as bits and boxes as values, a NaN equal to a NaN."""
    return tuple(a.nbytes for a in got) == tuple(a.nbytes for a in want) and np.array_equal(got[2], want[2]) and \
        R.same_bits_or_nan(got[1], want[1]) and R.same_nodes(got[0], want[0])


def check_closest(rays, got, want, woop, tri):
    """t bit for bit; ids equal except where two triangles tie at the same t bits."""
    assert np.array_equal(got[:, 1], want[:, 1])
    diff = np.nonzero(got[:, 0] != want[:, 0])[0]
    assert len(O.invalid_hits(rays, got, woop, tri, which=diff)) == 0


def check_wide_order(rays, got, want, woop, tri):
    """What a wide traversal may answer where boxes are not finite: every result genuine (a hit
    some triangle reproduces, a miss at tmax), none farther than the oracle's, every ray the
    oracle hits hit. Returns the number of rays whose result is closer than the oracle's."""
    assert len(O.invalid_hits(rays, got, woop, tri)) == 0
    gt, wt = got[:, 1].view(np.float32), want[:, 1].view(np.float32)
    assert not np.isnan(gt).any() and (gt <= wt).all()
    assert (got[want[:, 0] != -1, 0] != -1).all()
    return int((gt < wt).sum())


# ---- a. the build ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", L.LEAF_SIZES)
@pytest.mark.parametrize("kind", L.EDGE_GEOMETRY)
def test_device_build_equals_host_build(tracer, kind, max_leaf):
    """denormal is the case that fails if lbvh_kernel.hip or refit_kernel.hip is ever built with
    denormal flushing: flushed centroid bounds have extent 0, so every key is 0 and the order is
    the index order, and flushed box planes are 0 where the host's are denormal."""
    v, t, want = L.host_edge(kind, max_leaf)
    tracer.set_config(wide=1)
    first = download(tracer.build(v, t, max_leaf_size=max_leaf))
    assert tuple(a.nbytes for a in first) == tuple(a.nbytes for a in want)   # the written sizes
    assert np.array_equal(first[2], want[2])
    assert R.same_bits_or_nan(first[1], want[1])
    assert R.same_nodes(first[0], want[0])
    info = tracer.build_info()
    assert info["skipped_refs"] == 0 and info["max_leaf_size"] == max_leaf
    second = download(tracer.build(v, t, max_leaf_size=max_leaf))
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()   # one device: NaNs bit for bit too


# ---- b. the refit ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refit_case(kind):
    """(bound buffers, their vertices, the vertices to refit to, triangles, the host refit)."""
    if kind == "signed_zero":   # its own tree, refitted to every z sign flipped
        v0, t, bufs = L.host_edge(kind, 4)
        v1 = v0.copy()
        v1[:, 2] = -v1[:, 2]
    else:
        v0, t, bufs = L.host_edge("soup", 4)
        v1 = L.edge_geometry(kind)[0]
    return bufs, v0, v1, t, R.host_refit(bufs, v1, t)


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("kind", L.EDGE_GEOMETRY)
def test_device_refit_equals_host_refit(tracer, kind, wide):
    """denormal fails here too if refit_kernel.hip is built with denormal flushing (box planes)."""
    bufs, v0, v1, t, want = refit_case(kind)
    g = bind(tracer, bufs, wide)
    wide_before = tracer.wide_nodes()
    tracer.refit(v1, t)
    got = download(g)
    assert same_buffers(got, want)
    assert tracer.refit_info()["skipped_refs"] == 0
    if kind != "signed_zero":
        assert not np.array_equal(got[1], bufs[1]), "the refit moved nothing"
    if wide:
        assert tracer.bind_info()["wide_format"] == 1
        R.check_wide(wide_before, tracer.wide_nodes(), bufs[0], got[0])
    else:
        assert tracer.wide_nodes().size == 0
    tracer.refit(v0, t)
    back = download(g)
    assert np.array_equal(back[1], bufs[1]) and R.same_nodes(back[0], bufs[0]) and np.array_equal(back[2], bufs[2])
    if wide:
        R.check_wide(wide_before, tracer.wide_nodes(), bufs[0], back[0])


# ---- c. traces ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", FINITE_KINDS)
def test_traces_after_a_build_equal_the_oracle(tracer, kind, mode):
    v, t = L.edge_geometry(kind)
    tracer.set_config(wide=MODES[mode])
    nodes, woop, tri = download(tracer.build(v, t))   # the default leaf size
    rays = L.edge_rays(kind)
    rb = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(rb, exact_rcp=True, speculative=mode != "lockstep_off")
    assert tracer.last_info["stack_overflows"] == 0
    want, _, _ = O.trace(rays, nodes, woop, tri)
    hits = int((want[:, 0] != -1).sum())
    print(f"{kind} {mode}: the oracle sees {hits} hits")
    assert hits >= L.edge_min_hits(kind)
    if kind in L.SEES_NOTHING:   # every Woop row is +-0 or NaN: no ray hits, by construction
        assert hits == 0
    check_closest(rays, rb.results_numpy(), want, woop, tri)
    ah = RayBuffer(rays, need_closest_hit=False)
    tracer.trace_batch(ah, exact_rcp=True, speculative=mode != "lockstep_off")
    brute = O.brute_force(rays, woop, tri, any_hit=True)
    assert np.array_equal(ah.results_numpy()[:, 0] == -1, brute[:, 0] == -1)


@pytest.mark.parametrize("mode", list(MODES))
def test_traces_of_nonfinite_geometry(tracer, mode):
    """NaN vertices enter no box, infinite ones make boxes infinite. The binary orders equal the
    oracle bit for bit. The 4-wide orders skip binary ancestors, so where an ancestor's planes
    are not finite they may only find MORE than the oracle: genuine hits, none farther."""
    v, t = L.edge_geometry("nonfinite")
    tracer.set_config(wide=MODES[mode])
    nodes, woop, tri = download(tracer.build(v, t))
    if mode == "wide2":
        assert tracer.bind_info()["wide_format"] == 1   # infinite boxes do not quantize
    rays = L.edge_rays("nonfinite")
    rb = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(rb, exact_rcp=True, speculative=mode != "lockstep_off")
    assert tracer.last_info["stack_overflows"] == 0
    want, _, _ = O.trace(rays, nodes, woop, tri)
    hits = int((want[:, 0] != -1).sum())
    assert hits >= 16
    got = rb.results_numpy()
    if mode in ("wide0", "lockstep_off"):
        check_closest(rays, got, want, woop, tri)
        print(f"nonfinite {mode}: the oracle sees {hits} hits")
    else:
        closer = check_wide_order(rays, got, want, woop, tri)
        print(f"nonfinite {mode}: the oracle sees {hits} hits, {closer} wide results closer than the oracle's")
    brute = O.brute_force(rays, woop, tri)
    assert np.array_equal(want[:, 1], brute[:, 1])   # and the oracle itself misses nothing
    ah = RayBuffer(rays, need_closest_hit=False)
    tracer.trace_batch(ah, exact_rcp=True, speculative=mode != "lockstep_off")
    assert np.array_equal(ah.results_numpy()[:, 0] == -1, brute[:, 0] == -1)


# ---- d. the wide = 2 fallback ---------------------------------------------------------------
def test_wide2_falls_back_to_the_exact_array_and_keeps_it(tracer):
    bufs, v0, v1, t, want = refit_case("nonfinite")
    g = bind(tracer, bufs, 2)
    assert tracer.bind_info()["wide_format"] == 2
    tracer.refit(v1, t)
    assert tracer.bind_info()["wide_format"] == 1   # an infinite box does not quantize
    nodes, woop, tri = download(g)
    assert same_buffers((nodes, woop, tri), want)
    rays = L.edge_rays("nonfinite")
    rb = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(rb, exact_rcp=True)
    assert tracer.last_info["stack_overflows"] == 0
    expect, _, _ = O.trace(rays, nodes, woop, tri)
    assert (expect[:, 0] != -1).sum() >= 16
    closer = check_wide_order(rays, rb.results_numpy(), expect, woop, tri)
    print(f"after the fallback: {closer} wide results closer than the oracle's")
    # back to finite vertices: the exact array stays (mrt.h), updated in place
    tracer.refit(v0, t)
    assert tracer.bind_info()["wide_format"] == 1
    nodes, woop, tri = download(g)
    assert np.array_equal(woop, bufs[1]) and R.same_nodes(nodes, bufs[0])
    rb = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(rb, exact_rcp=True)
    expect, _, _ = O.trace(rays, nodes, woop, tri)
    assert (expect[:, 0] != -1).sum() >= 16
    check_closest(rays, rb.results_numpy(), expect, woop, tri)
    tracer.set_bvh(g)   # a rebind derives the quantized form again
    assert tracer.bind_info()["wide_format"] == 2
    v, t = L.edge_geometry("nonfinite")
    tracer.build(v, t)
    assert tracer.bind_info()["wide_format"] == 1


# ---- e. sizes -------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", [1, 8])
@pytest.mark.parametrize("n", [2, 3, 9, 256, 257, 258, 1024, 1025])
def test_sizes_around_the_workgroup_boundaries(tracer, n, max_leaf):
    v, t = L._soup(n, 100 + n)
    want = mrt.Bvh.build_lbvh(mrt.Scene.from_arrays(v, t), max_leaf).buffers()
    tracer.set_config(wide=1)
    got = download(tracer.build(v, t, max_leaf_size=max_leaf))
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    assert tracer.build_info()["skipped_refs"] == 0


def test_262145_triangles(tracer):
    """One triangle more than the bounds kernel's 1024 x 256 threads. Device against host by
    bits is the check: the Python restatements are too slow at this size."""
    n = 262145
    v, t = L._soup(n, 31)
    host = mrt.Bvh.build_lbvh(mrt.Scene.from_arrays(v, t), 4).buffers()
    tracer.set_config(wide=1)
    g = tracer.build(v, t, max_leaf_size=4)
    nodes, woop, tri = download(g)
    for a, b in zip((nodes, woop, tri), host):
        assert a.tobytes() == b.tobytes()
    info = tracer.build_info()
    assert info["skipped_refs"] == 0 and info["records"] == len(nodes) // 16
    assert info["slots"] == len(tri) == len(woop) // 4 == 3 * n + info["leaves"]
    assert info["leaves"] == (nodes.reshape(-1, 16)[:, 12:14] < 0).sum()
    _, offsets, _ = refit_plan(nodes, wide=False)
    assert info["levels"] == len(offsets) - 1
    v2 = R.displaced(v)
    want = R.host_refit(host, v2, t)
    tracer.refit(v2, t)
    nodes, woop, tri = download(g)
    for a, b in zip((nodes, woop, tri), want):
        assert a.tobytes() == b.tobytes()
    upper = np.diff(offsets)[1:]
    assert (upper > 1024).sum() >= 2
    rinfo = tracer.refit_info()
    # the leaves, every level above 1024 nodes, the one-workgroup tail, the wide gather
    assert rinfo["launches"] == 1 + int((upper > 1024).sum()) + int((upper <= 1024).any()) + 1
    assert rinfo["levels"] == len(offsets) - 1 and rinfo["skipped_refs"] == 0
    rays = R.frame_rays(v2)
    rb = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(rb, exact_rcp=True)
    expect, _, _ = O.trace(rays, *want)
    assert (expect[:, 0] != -1).sum() >= 16
    check_closest(rays, rb.results_numpy(), expect, want[1], want[2])
