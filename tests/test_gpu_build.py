"""Device LBVH build (mrt_tracer_build, csrc/lbvh_kernel.hip) against the host build
(mrth_bvh_build_lbvh) and the CPU oracle.

  * device == host for max_leaf_size 1, 4, 8 on every scene and edge shape of
    tests/test_lbvh.py: nodes as float values (refit_util.same_nodes), Woop and triIndex as
    bits, the written sizes; two builds of one input give identical bytes;
  * traces after a build equal the oracle's traversal of the downloaded buffers (exact
    reciprocal; wide 0, 1, 2 and the per-lane order), any-hit answers agree with brute force;
  * build -> refit with displaced vertices -> trace equals host LBVH + host refit + oracle;
  * a second build with another triangle count rebinds; a capacity that is too small is
    refused and the earlier tree still traces; a triangle with an out-of-range vertex index is
    counted and hit by nothing while every other triangle traces; build_info matches the buffers.

"random" 9000 needs a multi-block sort and has a level above the refit's 1024-node launch
threshold; the others (183-1500 triangles) are no multiple of a workgroup.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import lbvh_util as L  # noqa: E402
import oracle_lib as O  # noqa: E402
import refit_util as R  # noqa: E402
from mrt import _lib  # noqa: E402
from mrt.tracer import RayBuffer, Tracer, refit_plan  # noqa: E402

SCENE_IDS = [f"{n}{p}" for n, p in L.SCENES]
CASES = [(n, p) for n, p in L.SCENES] + [(k, None) for k in L.EDGE_SHAPES]
CASE_IDS = SCENE_IDS + L.EDGE_SHAPES


@pytest.fixture(scope="module")
def tracer():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Tracer(0)


def download(g):
    torch.cuda.synchronize()
    return g.nodes.cpu().numpy(), g.woop.cpu().numpy(), g.tri_index.cpu().numpy()


def check_closest(rays, got, want, woop, tri):
    """t bit for bit; ids equal except where two triangles tie at the same t bits."""
    assert np.array_equal(got[:, 1], want[:, 1])
    diff = np.nonzero(got[:, 0] != want[:, 0])[0]
    assert len(O.invalid_hits(rays, got, woop, tri, which=diff)) == 0


@pytest.mark.parametrize("max_leaf", L.LEAF_SIZES)
@pytest.mark.parametrize("name,param", CASES, ids=CASE_IDS)
def test_device_build_equals_host_build(tracer, name, param, max_leaf):
    v, t, want = L.host_lbvh(name, param, max_leaf)
    tracer.set_config(wide=1)
    g = tracer.build(v, t, max_leaf_size=max_leaf)
    nodes, woop, tri = download(g)
    assert (nodes.nbytes, woop.nbytes, tri.nbytes) == tuple(a.nbytes for a in want)   # the written sizes
    assert np.array_equal(tri, want[2])
    assert np.array_equal(woop, want[1])
    assert R.same_nodes(nodes, want[0])
    info = tracer.build_info()
    assert info["skipped_refs"] == 0 and info["max_leaf_size"] == max_leaf


@pytest.mark.parametrize("name,param", [L.BIG, ("copies", None)], ids=["random9000", "copies"])
def test_two_builds_give_identical_bytes(tracer, name, param):
    v, t, _ = L.host_lbvh(name, param, 4)
    first = download(tracer.build(v, t, max_leaf_size=4))
    second = download(tracer.build(v, t, max_leaf_size=4))
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("mode", ["wide0", "wide1", "wide2", "lockstep_off"])
@pytest.mark.parametrize("name,param", L.SCENES, ids=SCENE_IDS)
def test_traces_after_a_build_equal_the_oracle(tracer, name, param, mode):
    v, t = L.scene_arrays(name, param)
    tracer.set_config(wide={"wide0": 0, "wide1": 1, "wide2": 2, "lockstep_off": 1}[mode])
    nodes, woop, tri = download(tracer.build(v, t))   # the default leaf size
    assert tracer.build_info()["max_leaf_size"] == _lib.MRT_LBVH_DEFAULT_MAX_LEAF
    rays = R.frame_rays(v)
    rb = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(rb, exact_rcp=True, speculative=mode != "lockstep_off")
    want, _, _ = O.trace(rays, nodes, woop, tri)
    assert (want[:, 0] != -1).sum() >= 16
    check_closest(rays, rb.results_numpy(), want, woop, tri)
    ah = RayBuffer(rays, need_closest_hit=False)
    tracer.trace_batch(ah, exact_rcp=True, speculative=mode != "lockstep_off")
    brute = O.brute_force(rays, woop, tri, any_hit=True)
    assert np.array_equal(ah.results_numpy()[:, 0] == -1, brute[:, 0] == -1)


@pytest.mark.parametrize("name,param", [("random", 1500), L.BIG], ids=["random1500", "random9000"])
def test_build_then_refit(tracer, name, param):
    v, t, host = L.host_lbvh(name, param, 4)
    v2 = R.displaced(v)
    want = R.host_refit(host, v2, t)
    tracer.set_config(wide=1)
    g = tracer.build(v, t, max_leaf_size=4)
    tracer.refit(v2, t)
    nodes, woop, tri = download(g)
    assert np.array_equal(woop, want[1]) and R.same_nodes(nodes, want[0]) and np.array_equal(tri, want[2])
    assert tracer.refit_info()["levels"] == tracer.build_info()["levels"]
    rays = R.frame_rays(v2)
    rb = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(rb, exact_rcp=True)
    expect, _, _ = O.trace(rays, *want)
    assert (expect[:, 0] != -1).sum() >= 16
    check_closest(rays, rb.results_numpy(), expect, want[1], want[2])


def test_a_second_build_rebinds(tracer):
    tracer.set_config(wide=1)
    va, ta = L.scene_arrays("random", 1500)
    vb, tb = L.scene_arrays("sphere", 12)
    assert len(ta) != len(tb)
    tracer.build(va, ta)
    first = tracer.build_info()
    nodes, woop, tri = download(tracer.build(vb, tb))
    second = tracer.build_info()
    assert second["slots"] == len(tri) != first["slots"]
    rays = R.frame_rays(vb)
    rb = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(rb, exact_rcp=True)
    want, _, _ = O.trace(rays, nodes, woop, tri)
    assert (want[:, 0] != -1).sum() >= 16
    check_closest(rays, rb.results_numpy(), want, woop, tri)


def test_a_capacity_that_is_too_small_is_refused_and_the_earlier_tree_stands(tracer):
    tracer.set_config(wide=1)
    v, t = L.scene_arrays("sphere", 12)
    g = tracer.build(v, t)
    rays = R.frame_rays(v)
    before = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(before, exact_rcp=True)
    dev = g.device
    dv = torch.from_numpy(np.array(v)).to(dev)
    dt = torch.from_numpy(np.array(t)).to(dev)
    cap = [C.c_int64(), C.c_int64(), C.c_int64()]
    lib = _lib.trace_lib()
    assert lib.mrt_lbvh_sizes(len(t), *map(C.byref, cap)) == 0
    bufs = [torch.full((c.value // 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev) for c in cap]
    out = [C.c_int64(), C.c_int64(), C.c_int64()]
    for short in range(3):
        caps = [c.value - (16 if i == short else 0) for i, c in enumerate(cap)]
        rc = lib.mrt_tracer_build(tracer._h, dv.data_ptr(), len(v), dt.data_ptr(), len(t), None, bufs[0].data_ptr(),
                                  caps[0], bufs[1].data_ptr(), caps[1], bufs[2].data_ptr(), caps[2],
                                  *map(C.byref, out), None)
        assert rc == _lib.MRT_ERR_TOO_LARGE
    torch.cuda.synchronize()
    assert all(bool((b == 0x5A5A5A5A).all()) for b in bufs)   # nothing written
    after = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(after, exact_rcp=True)
    assert np.array_equal(after.results_numpy()[:, :2], before.results_numpy()[:, :2])
    assert (before.results_numpy()[:, 0] != -1).sum() >= 16


def test_an_out_of_range_vertex_index_is_counted_and_hit_by_nothing(tracer):
    tracer.set_config(wide=1)
    v, t = L.scene_arrays("random", 1500)
    rays = R.frame_rays(v)
    tracer.build(v, t)
    clean = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(clean, exact_rcp=True)
    hit_ids, counts = np.unique(clean.hit_ids()[clean.hit_ids() >= 0], return_counts=True)
    victim = int(hit_ids[np.argmax(counts)])   # the triangle most rays see
    bad = np.array(t)
    bad[victim, 1] = len(v)
    nodes, woop, tri = download(tracer.build(v, bad))
    assert tracer.build_info()["skipped_refs"] == 1
    z_slots, _ = R.leaf_walk(nodes, woop)   # from the leaf refs: a U or V row may start with -0.0 too
    ids = tri[z_slots]
    assert np.array_equal(np.sort(ids), np.arange(len(t)))
    rows = woop.view(np.float32).reshape(-1, 4)
    got_rows = np.stack([rows[z_slots], rows[z_slots + 1], rows[z_slots + 2]], 1).reshape(-1, 12)
    want_rows = R.np_woopify(v[t[ids, 0]], v[t[ids, 1]], v[t[ids, 2]])
    want_rows[ids == victim] = 0.0   # the skipped triangle keeps zeroed rows
    assert np.array_equal(got_rows.view(np.int32), want_rows.view(np.int32))
    rb = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(rb, exact_rcp=True)
    got = rb.results_numpy()
    want, _, _ = O.trace(rays, nodes, woop, tri)
    check_closest(rays, got, want, woop, tri)
    brute = O.brute_force(rays, woop, tri)
    assert np.array_equal(got[:, 1], brute[:, 1])
    assert not (got[:, 0] == victim).any()
    # rays that saw another triangle first still see it at the same distance
    others = clean.hit_ids() != victim
    assert np.array_equal(got[others, 1], clean.results_numpy()[others, 1])


@pytest.mark.parametrize("name,param,max_leaf", [("hairball", 3, 1), (*L.BIG, 8), ("one", None, 4)],
                         ids=["hairball3-1", "random9000-8", "one-4"])
def test_build_info_matches_the_buffers(tracer, name, param, max_leaf):
    v, t, _ = L.host_lbvh(name, param, max_leaf)
    tracer.set_config(wide=1)
    nodes, woop, tri = download(tracer.build(v, t, max_leaf_size=max_leaf))
    info = tracer.build_info()
    print(info)
    assert info["records"] == len(nodes) // 16
    assert info["slots"] == len(tri) == len(woop) // 4 == 3 * len(t) + info["leaves"]
    refs = nodes.reshape(-1, 16)[:, 12:14]
    assert info["leaves"] == (refs < 0).sum()
    _, offsets, _ = refit_plan(nodes, wide=False)
    assert info["levels"] == len(offsets) - 1
    assert info["scratch_bytes"] > 0 and info["wall_ms"] > 0
    assert info["wall_ms"] >= info["plan_ms"] + info["bind_ms"]
