"""Device refit (mrt_tracer_refit, csrc/refit_kernel.hip) against the host refit
(mrth_bvh_refit) and the CPU oracle.

  * device == host: with moved vertices the bound buffers equal the host refit's (nodes as
    float values, Woop as bits, triIndex untouched) at wide 0 and 1; the copied-out exact
    4-wide array equals the mapped Compact2 boxes bit for bit and keeps its refs;
  * traces after a refit find what the oracle finds in the host-refitted buffers (exact
    reciprocal; wide 0, 1, 2 and the per-lane order), any-hit answers agree with brute force;
  * a hand-made chain of depth 40 (one node per level, numbered children-first, leaves of
    1 and 8 triangles) and a one-triangle scene (the wrapper and its empty leaf);
  * on one stream without a sync: refit -> trace -> refit back -> trace; the autotuner's
    schedules survive;
  * an out-of-range triIndex entry or vertex index is skipped and counted, never read through.

The scenes have 183-730 inner nodes: no multiple of the 256-thread workgroup, several
one-node levels, every level inside the one-workgroup tail launch except level 0.
"random" 9000 (5119 nodes) adds a level 1 of 1236 nodes, above the 1024-node threshold
between the per-level launch and the tail launch (level 2 has 726).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mrt  # noqa: E402
import oracle_lib as O  # noqa: E402
import refit_util as R  # noqa: E402
from mrt.tracer import GpuBvh, RayBuffer, Tracer, refit_plan  # noqa: E402

ALPHA = 1e-5


@pytest.fixture(scope="module")
def tracer():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Tracer(0)


def bind(tracer, bufs, wide):
    tracer.set_config(wide=wide)
    g = GpuBvh(tuple(np.array(b) for b in bufs))
    tracer.set_bvh(g)
    return g


def download(g):
    torch.cuda.synchronize()
    return g.nodes.cpu().numpy(), g.woop.cpu().numpy(), g.tri_index.cpu().numpy()


_MOVED = {}


def moved(name, param):
    """(moved vertices, triangles, built buffers, host-refitted buffers), computed once."""
    if (name, param) not in _MOVED:
        v, t, bufs, _ = R.built(name, param, ALPHA)
        v2 = R.displaced(v)
        _MOVED[name, param] = (v, v2, t, bufs, R.host_refit(bufs, v2, t))
    return _MOVED[name, param]


check_wide = R.check_wide


BIG_LEVEL = ("random", 9000)


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("name,param", R.SCENES + [BIG_LEVEL])
def test_device_refit_equals_host_refit(tracer, name, param, wide):
    _, v2, t, bufs, want = moved(name, param)
    g = bind(tracer, bufs, wide)
    wide_before = tracer.wide_nodes()
    tracer.refit(v2, t)
    nodes, woop, tri = download(g)
    assert np.array_equal(woop, want[1])
    assert R.same_nodes(nodes, want[0])
    assert np.array_equal(tri, bufs[2])
    _, offsets, _ = refit_plan(bufs[0])
    info = tracer.refit_info()
    assert info["levels"] == len(offsets) - 1
    upper = np.diff(offsets)[1:]
    if (name, param) == BIG_LEVEL:
        assert upper[0] > 1024 >= upper[1]
    # the leaves, every level above 1024 nodes, the one-workgroup tail, the wide gather
    assert info["launches"] == 1 + int((upper > 1024).sum()) + int((upper <= 1024).any()) + wide
    assert info["skipped_refs"] == 0
    assert info["plan_bytes"] >= 6 * len(nodes) // 16
    if wide:
        check_wide(wide_before, tracer.wide_nodes(), bufs[0], nodes)
    else:
        assert tracer.wide_nodes().size == 0


def check_closest(rays, got, want, woop, tri):
    """t bit for bit; ids equal except where two triangles tie at the same t bits."""
    assert np.array_equal(got[:, 1], want[:, 1])
    diff = np.nonzero(got[:, 0] != want[:, 0])[0]
    assert len(O.invalid_hits(rays, got, woop, tri, which=diff)) == 0


@pytest.mark.parametrize("mode", ["wide0", "wide1", "wide2", "lockstep_off"])
@pytest.mark.parametrize("name,param", R.SCENES + [BIG_LEVEL])
def test_traces_after_a_refit_equal_the_oracle(tracer, name, param, mode):
    _, v2, t, bufs, (nodes, woop, tri) = moved(name, param)
    wide = {"wide0": 0, "wide1": 1, "wide2": 2, "lockstep_off": 1}[mode]
    bind(tracer, bufs, wide)
    tracer.refit(v2, t)
    if mode == "wide2":
        assert tracer.bind_info()["wide_format"] == 2   # derived again from the refitted nodes
    rays = R.frame_rays(v2)
    rb = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(rb, exact_rcp=True, speculative=mode != "lockstep_off")
    want, _, _ = O.trace(rays, nodes, woop, tri)
    assert (want[:, 0] != -1).sum() >= 16
    check_closest(rays, rb.results_numpy(), want, woop, tri)
    ah = RayBuffer(rays, need_closest_hit=False)
    tracer.trace_batch(ah, exact_rcp=True, speculative=mode != "lockstep_off")
    brute = O.brute_force(rays, woop, tri, any_hit=True)
    assert np.array_equal(ah.results_numpy()[:, 0] == -1, brute[:, 0] == -1)


# ---- hand-made trees --------------------------------------------------------------------
def chain_tree(depth, rng):
    """A chain: node d has leaf d as one child and node d + 1 as the other (the last node two
    leaves), so every height level holds one node. Leaves hold 1 or 8 triangles. Node 0 is the
    root; the others are numbered children-first. Boxes start as zeros: the refit writes them."""
    index_of = [0] + [depth - d for d in range(1, depth)]   # depth d -> record
    sizes = [8 if d % 3 == 0 else 1 for d in range(depth + 1)]
    nt = sum(sizes)
    centres = rng.uniform(-1, 1, (nt, 1, 3))
    verts = (centres + rng.uniform(-0.15, 0.15, (nt, 3, 3))).reshape(-1, 3).astype(np.float32)
    tris = np.arange(nt * 3, dtype=np.int32).reshape(-1, 3)
    woop, tri_index, leaf_ref, first = [], [], [], 0
    for n in sizes:
        leaf_ref.append(~(len(woop) // 4))
        for k in range(first, first + n):
            woop += list(mrt.woopify(*verts[tris[k]]).view(np.int32).reshape(-1))
            tri_index += [k, 0, 0]
        woop += [R.TERMINATOR] * 4
        tri_index += [0]
        first += n
    nodes = np.zeros((depth, 16), np.int32)
    for d in range(depth):
        rec = nodes[index_of[d]]
        inner = index_of[d + 1] * 4 if d + 1 < depth else leaf_ref[depth]
        rec[12], rec[13] = (leaf_ref[d], inner) if d % 2 else (inner, leaf_ref[d])
    return verts, tris, (nodes.reshape(-1), np.array(woop, np.int32), np.array(tri_index, np.int32))


@pytest.mark.parametrize("wide", [0, 1])
def test_hand_made_chain_of_depth_40(tracer, wide):
    verts, tris, bufs = chain_tree(40, np.random.default_rng(5))
    v2 = R.displaced(verts)
    want = R.host_refit(bufs, v2, tris)
    ref_nodes, ref_woop = R.np_refit(*bufs, v2, tris)
    assert np.array_equal(want[1], ref_woop) and R.same_nodes(want[0], ref_nodes)
    g = bind(tracer, bufs, wide)
    wide_before = tracer.wide_nodes()
    tracer.refit(v2, tris)
    nodes, woop, tri = download(g)
    assert np.array_equal(woop, want[1])
    assert R.same_nodes(nodes, want[0])
    assert np.array_equal(tri, bufs[2])
    assert tracer.refit_info()["levels"] == 40
    if wide:
        check_wide(wide_before, tracer.wide_nodes(), bufs[0], nodes)
    rays = R.frame_rays(v2)
    rb = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(rb, exact_rcp=True)
    brute = O.brute_force(rays, woop, tri)
    assert (brute[:, 0] != -1).sum() >= 16
    check_closest(rays, rb.results_numpy(), brute, woop, tri)


@pytest.mark.parametrize("wide", [0, 1])
def test_one_triangle_scene_keeps_its_empty_leaf(tracer, wide):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    t = np.array([[0, 1, 2]], np.int32)
    bufs = mrt.Bvh.build(mrt.Scene.from_arrays(v, t)).buffers()
    assert len(bufs[0]) == 16 and len(R.leaf_slots(bufs[1], bufs[0][13])) == 0   # the wrapper, an empty leaf
    v2 = (v * 1.5 + np.float32(0.25)).astype(np.float32)
    want = R.host_refit(bufs, v2, t)
    assert np.array_equal(R.boxes(want[0])[0, 1], R.boxes(bufs[0])[0, 1])   # the empty leaf's box stays
    g = bind(tracer, bufs, wide)
    tracer.refit(v2, t)
    nodes, woop, tri = download(g)
    assert np.array_equal(woop, want[1]) and R.same_nodes(nodes, want[0]) and np.array_equal(tri, bufs[2])
    info = tracer.refit_info()
    assert info["levels"] == 1 and info["launches"] == 1 + wide
    rays = R.frame_rays(v2)
    rb = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(rb, exact_rcp=True)
    brute = O.brute_force(rays, woop, tri)
    assert (brute[:, 0] == 0).sum() >= 16
    assert np.array_equal(rb.results_numpy()[:, :2], brute[:, :2])


def test_refit_before_bind_is_refused():
    import ctypes as C
    from mrt import _lib
    lib = _lib.trace_lib()
    h = C.c_void_p()
    assert lib.mrt_tracer_create(0, C.byref(h)) == 0
    dummy = torch.zeros(9, device="cuda")
    assert lib.mrt_tracer_refit(h, dummy.data_ptr(), 3, dummy.data_ptr(), 1, None) == _lib.MRT_ERR_NOT_BOUND
    info = _lib.RefitInfo()
    assert lib.mrt_tracer_refit_info(h, C.byref(info)) == 0 and info.levels == 0 and info.launches == 0
    lib.mrt_tracer_destroy(h)


# ---- ordering -------------------------------------------------------------------------
def test_refits_and_traces_in_stream_order_keep_the_schedules(tracer):
    v, v2, t, bufs, (nodes2, woop2, tri2) = moved("random", 1500)
    dev = torch.device("cuda", 0)
    bind(tracer, bufs, 1)
    rays = R.frame_rays(v2)
    first = RayBuffer(rays, need_closest_hit=True)
    for _ in range(700):   # settle this batch size's schedule (246-328 launches)
        tracer.trace_batch(first, exact_rcp=True)
        if tracer.last_info["autotune_locked"]:
            break
    saved = tracer.schedules()
    assert any(n == first.size for n, _, _, _ in saved)
    before = first.results_numpy().copy()
    dv, dv2, dt = (torch.from_numpy(np.array(a)).to(dev) for a in (v, v2, t))
    a, b = RayBuffer(rays, need_closest_hit=True), RayBuffer(rays, need_closest_hit=True)
    tracer.refit(dv, dt)   # builds the plan (the one synchronous step); the vertices are the built ones
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    tracer.refit(dv2, dt, stream=stream)
    tracer.trace_async(a, exact_rcp=True, stream=stream)
    tracer.refit(dv, dt, stream=stream)
    tracer.trace_async(b, exact_rcp=True, stream=stream)
    stream.synchronize()
    want, _, _ = O.trace(rays, nodes2, woop2, tri2)
    check_closest(rays, a.results_numpy(), want, woop2, tri2)
    # back at the built vertices: the Woop rows are the built ones again, the boxes may be looser
    assert np.array_equal(b.results_numpy()[:, :2], before[:, :2])
    assert tracer.schedules() == saved


# ---- out-of-range references --------------------------------------------------------------
def test_out_of_range_references_are_skipped_and_counted(tracer):
    v, v2, t, bufs, want = moved("random", 1500)
    nodes0, woop0, tri0 = bufs
    refs = nodes0.reshape(-1, 16)[:, 12:14]
    leaves = refs[refs < 0]
    tri_bad = tri0.copy()
    skip = set()
    for ref, bad in zip(leaves[[3, len(leaves) // 2, len(leaves) - 2]], (len(t), -3, 2**31 - 1)):
        slots = R.leaf_slots(woop0, ref)
        tri_bad[slots[-1]] = bad   # a one-triangle leaf is emptied, a longer one loses its last triangle
        skip.add(slots[-1])
    t_bad = t.copy()
    victim = int(tri0[R.leaf_slots(woop0, leaves[7])[0]])
    t_bad[victim, 2] = len(v)
    all_slots = {s for ref in leaves for s in R.leaf_slots(woop0, ref)}
    skip |= {s for s in all_slots if tri_bad[s] == victim}
    g = bind(tracer, (nodes0, woop0, tri_bad), 1)
    tracer.refit(v2, t_bad)
    nodes, woop, tri = download(g)
    assert tracer.refit_info()["skipped_refs"] == len(skip)
    assert tracer.refit_info()["skipped_refs"] == 0   # reset by the call
    assert np.array_equal(tri, tri_bad)
    exp_nodes, exp_woop = R.np_refit(nodes0, woop0, tri_bad, v2, t_bad, skip=skip)
    assert np.array_equal(woop, exp_woop)   # every other triangle refitted, the skipped ones as they were
    for s in skip:
        assert np.array_equal(woop.reshape(-1, 4)[s:s + 3], woop0.reshape(-1, 4)[s:s + 3])
    assert R.same_nodes(nodes, exp_nodes)
