"""The refit plan and the exact 4-wide array derived on the device (mrt_tracer_bind_device /
mrt_tracer_build_device, csrc/wide_kernel.hip) against the host derivation they replace. Valid
trees only: trees that are none are refused on the CPU (tests/test_wide_plan.py).

  * after set_bvh(on_device=True) the wide array equals the host bind's as bits, bind_info equals
    it but for bind_ms, and the installed plan equals mrt_refit_plan's order, offsets and source map;
  * build(on_device=True) writes the bytes build() writes and derives the same wide array;
  * the plan is installed by the bind or build itself, and a refit through it equals the host refit;
  * traces after a device bind equal the oracle at wide 0, 1 and, through the reported host
    fallback, 2; a second device bind rebinds; set_config re-derives the host's array;
  * derive_info reports both parts on the device and far fewer readbacks than nodes;
  * a tree of more than MRT_DERIVE_MAX_LEVELS depth levels goes through the host path in a device
    bind and in the first refit, with the host's results, and the info says so;
  * a device bind that refuses its tree leaves the tracer unbound, and a good bind follows;
  * the source map of a host bind goes to the device once, and stays over a set_config that keeps
    cfg.wide.

scene_complete(12) has depth levels of 1 .. 2048 nodes: levels 0-10 run chained in one workgroup,
level 11 (2048 nodes, above the 1024-node threshold) in a launch of its own.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import kat  # noqa: E402
import lbvh_util as L  # noqa: E402
import oracle_lib as O  # noqa: E402
import refit_util as R  # noqa: E402
import test_wide_plan as WP  # noqa: E402
from mrt import _lib  # noqa: E402
from mrt.tracer import GpuBvh, RayBuffer, Tracer, refit_plan  # noqa: E402

ALPHA = 1e-5


@pytest.fixture(scope="module")
def tracer():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    t = Tracer(0)
    t.set_config(wide=1)
    return t


def gpu(bufs):
    return GpuBvh(tuple(np.array(b) for b in bufs))


TREES = {
    "one": lambda: L.host_lbvh("one", None, 4)[2],
    "n_eq_l_plus_1": lambda: L.host_lbvh("n_eq_l_plus_1", None, 4)[2],
    "copies": lambda: L.host_lbvh("copies", None, 4)[2],
    "flat": lambda: L.host_lbvh("flat", None, 4)[2],
    "comb40": lambda: kat.scene_comb(40)[0],
    "comb70": lambda: kat.scene_comb(70)[0],
    "complete12": lambda: kat.scene_complete(12)[0],
    "random1500": lambda: R.built("random", 1500, ALPHA)[2],
    "random9000": lambda: R.built("random", 9000, ALPHA)[2],
    "hairball3": lambda: R.built("hairball", 3, ALPHA)[2],
}
TREES.update({f"edge-{kind}": (lambda kind=kind: L.host_edge(kind, 4)[2]) for kind in L.EDGE_GEOMETRY})

_HOST = {}


def host_side(tracer, name):
    """(buffers, the host bind's wide array, its bind_info, mrt_refit_plan), computed once."""
    if name not in _HOST:
        bufs = TREES[name]()
        tracer.set_config(wide=1)
        tracer.set_bvh(gpu(bufs))
        _HOST[name] = (bufs, tracer.wide_nodes(), tracer.bind_info(), refit_plan(bufs[0]))
    return _HOST[name]


def same_info(a, b):
    return {k: v for k, v in a.items() if k != "bind_ms"} == {k: v for k, v in b.items() if k != "bind_ms"}


def same_plan(got, want):
    assert got is not None, "no plan is installed"
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if want[2] is None or got[2] is None:
        assert got[2] is None and want[2] is None
    else:
        assert np.array_equal(got[2], want[2])


@pytest.mark.parametrize("name", list(TREES))
def test_device_bind_equals_host_bind(tracer, name):
    bufs, wide, info, plan = host_side(tracer, name)
    tracer.set_config(wide=1)
    tracer.set_bvh(gpu(bufs), on_device=True)
    got = tracer.wide_nodes()
    assert got.size == wide.size and R.same_bits_or_nan(got, wide)
    assert same_info(tracer.bind_info(), info)
    same_plan(tracer.refit_plan(), plan)
    d = tracer.derive_info()
    assert d["on_device_plan"] == 1 and d["on_device_wide"] == 1
    assert d["levels"] == len(plan[1]) - 1 and d["wide_nodes"] == wide.size // 32
    assert tracer.refit_info()["levels"] == len(plan[1]) - 1   # installed: no refit has run
    if name == "complete12":
        # init; topology: levels 0-10 chained, level 11, the empty frontier; heights: level 11, the
        # chain; the sort and the level starts; roots, sizes and numbers: two each; the emission
        assert d["depth_levels"] == 12 and d["launches"] == 1 + 3 + 2 + 2 + 6 + 1


def test_plan_only_at_wide_0(tracer):
    bufs, _, _, plan = host_side(tracer, "random1500")
    tracer.set_config(wide=0)
    tracer.set_bvh(gpu(bufs), on_device=True)
    assert tracer.wide_nodes().size == 0
    got = tracer.refit_plan()
    assert np.array_equal(got[0], plan[0]) and np.array_equal(got[1], plan[1]) and got[2] is None
    d = tracer.derive_info()
    assert d["on_device_plan"] == 1 and d["on_device_wide"] == 0 and d["wide_nodes"] == 0
    tracer.set_config(wide=1)


# ---- build ------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", L.LEAF_SIZES)
@pytest.mark.parametrize("scene", ["random1500", "copies", "one", "nonfinite"])
def test_device_build_writes_the_bytes_of_build(tracer, scene, max_leaf):
    if scene == "random1500":
        v, t = L.scene_arrays("random", 1500)
    elif scene == "nonfinite":
        v, t = L.edge_geometry(scene)
    else:
        v, t = L.edge_shape(scene, max_leaf)
    tracer.set_config(wide=1)
    a = tracer.build(v, t, max_leaf_size=max_leaf)
    want = [x.cpu().numpy() for x in (a.nodes, a.woop, a.tri_index)]
    wide, info = tracer.wide_nodes(), tracer.bind_info()
    assert tracer.refit_plan() is None   # the host route: its plan was the build's scratch
    b = tracer.build(v, t, max_leaf_size=max_leaf, on_device=True)
    got = [x.cpu().numpy() for x in (b.nodes, b.woop, b.tri_index)]
    for g, w in zip(got, want):
        assert g.shape == w.shape and R.same_bits_or_nan(g, w)
    assert R.same_bits_or_nan(tracer.wide_nodes(), wide) and same_info(tracer.bind_info(), info)
    same_plan(tracer.refit_plan(), refit_plan(want[0]))
    built = tracer.build_info()
    assert tracer.refit_info()["levels"] == built["levels"] > 0
    d = tracer.derive_info()
    assert d["on_device_plan"] == 1 and d["on_device_wide"] == 1


# ---- the installed plan ---------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["bind", "build"])
def test_refit_through_the_installed_plan_equals_the_host_refit(tracer, how):
    tracer.set_config(wide=1)
    if how == "bind":
        v, t, bufs, _ = R.built("random", 1500, ALPHA)
        g = gpu(bufs)
        tracer.set_bvh(g, on_device=True)
    else:
        v, t = L.scene_arrays("random", 1500)
        g = tracer.build(v, t, on_device=True)
        bufs = tuple(x.cpu().numpy() for x in (g.nodes, g.woop, g.tri_index))
    assert tracer.refit_info()["levels"] > 0
    wide_before = tracer.wide_nodes()
    v2 = R.displaced(v)
    want = R.host_refit(bufs, v2, t)
    tracer.refit(v2, t)
    torch.cuda.synchronize()
    nodes, woop, tri = (x.cpu().numpy() for x in (g.nodes, g.woop, g.tri_index))
    assert R.same_bits_or_nan(woop, want[1]) and R.same_bits_or_nan(nodes, want[0])
    assert np.array_equal(tri, bufs[2])
    R.check_wide(wide_before, tracer.wide_nodes(), bufs[0], nodes)
    assert tracer.refit_info()["skipped_refs"] == 0


def test_first_refit_after_a_host_bind_makes_its_plan_on_the_device(tracer):
    v, t, bufs, _ = R.built("random", 9000, ALPHA)
    tracer.set_config(wide=1)
    g = gpu(bufs)
    tracer.set_bvh(g)
    assert tracer.refit_plan() is None
    tracer.refit(v, t)
    same_plan(tracer.refit_plan(), refit_plan(bufs[0]))
    d = tracer.derive_info()
    assert d["on_device_plan"] == 1 and d["on_device_wide"] == 0


# ---- traces ---------------------------------------------------------------------------------------
def check_closest(rays, got, want, woop, tri):
    assert np.array_equal(got[:, 1], want[:, 1])
    diff = np.nonzero(got[:, 0] != want[:, 0])[0]
    assert len(O.invalid_hits(rays, got, woop, tri, which=diff)) == 0


_ORACLE = {}


def oracle(name, param):
    if (name, param) not in _ORACLE:
        v, _, bufs, _ = R.built(name, param, ALPHA)
        rays = R.frame_rays(v)
        _ORACLE[name, param] = (bufs, rays, O.trace(rays, *bufs)[0])
    return _ORACLE[name, param]


@pytest.mark.parametrize("wide", [0, 1, 2])
@pytest.mark.parametrize("name,param", [("random", 1500), ("hairball", 3)])
def test_traces_after_a_device_bind_equal_the_oracle(tracer, name, param, wide):
    bufs, rays, want = oracle(name, param)
    assert (want[:, 0] != -1).sum() >= 16
    tracer.set_config(wide=wide)
    tracer.set_bvh(gpu(bufs), on_device=True)
    d = tracer.derive_info()
    assert d["on_device_plan"] == 1 and d["on_device_wide"] == (1 if wide == 1 else 0)
    assert tracer.bind_info()["wide_format"] == wide   # 2: the quantized array through the host path
    rb = RayBuffer(rays, need_closest_hit=True)
    tracer.trace_batch(rb, exact_rcp=True)
    check_closest(rays, rb.results_numpy(), want, bufs[1], bufs[2])
    tracer.set_config(wide=1)


# ---- rebind and config ----------------------------------------------------------------------------
def test_a_second_device_bind_rebinds_and_set_config_rederives(tracer):
    tracer.set_config(wide=1)
    for name in ("random1500", "comb40", "random1500"):
        bufs, wide, info, plan = host_side(tracer, name)
        tracer.set_bvh(gpu(bufs), on_device=True)
        assert R.same_bits_or_nan(tracer.wide_nodes(), wide) and same_info(tracer.bind_info(), info)
        same_plan(tracer.refit_plan(), plan)
    tracer.set_config(wide=0)
    assert tracer.wide_nodes().size == 0
    tracer.set_config(wide=1)
    assert R.same_bits_or_nan(tracer.wide_nodes(), wide) and same_info(tracer.bind_info(), info)
    # the plan was dropped with the setting; the next refit makes it again, source map included
    v, t, _, _ = R.built("random", 1500, ALPHA)
    before = tracer.wide_nodes()
    tracer.refit(R.displaced(v), t)
    torch.cuda.synchronize()
    same_plan(tracer.refit_plan(), plan)
    R.check_wide(before, tracer.wide_nodes(), bufs[0], tracer.bvh.nodes.cpu().numpy())


def test_set_config_that_keeps_wide_keeps_the_device_array_and_its_map(tracer):
    """The source map of a device bind lives only on the device: a plan made again after
    set_config must still find it."""
    v, t, bufs, _ = R.built("random", 1500, ALPHA)
    _, wide, _, plan = host_side(tracer, "random1500")
    tracer.set_config(wide=1)
    g = gpu(bufs)
    tracer.set_bvh(g, on_device=True)
    tracer.set_config(spec_slack=tracer.config()["spec_slack"])   # drops the plan, keeps the array
    assert tracer.refit_plan() is None
    assert R.same_bits_or_nan(tracer.wide_nodes(), wide)
    tracer.refit(R.displaced(v), t)
    torch.cuda.synchronize()
    same_plan(tracer.refit_plan(), plan)
    R.check_wide(wide, tracer.wide_nodes(), bufs[0], g.nodes.cpu().numpy())


def test_the_source_map_of_a_host_bind_is_uploaded_once(tracer):
    """The host-bound route of the test above: the first plan takes the map to the device, where
    it stays with its array when set_config drops the plan."""
    v, t, bufs, _ = R.built("random", 1500, ALPHA)
    _, wide, _, plan = host_side(tracer, "random1500")
    tracer.set_config(wide=1)
    g = gpu(bufs)
    tracer.set_bvh(g)
    v2 = R.displaced(v)
    tracer.refit(v2, t)
    first_bytes, first_plan = tracer.refit_info()["plan_bytes"], tracer.refit_plan()
    same_plan(first_plan, plan)
    assert first_bytes == len(plan[0]) * 4 + len(plan[1]) * 4 + len(plan[0]) * 2 + 8 + plan[2].size * 4
    tracer.set_config(spec_slack=tracer.config()["spec_slack"])   # drops the plan, keeps the array and its map
    assert tracer.refit_plan() is None
    tracer.refit(v2, t)
    torch.cuda.synchronize()
    assert tracer.refit_info()["plan_bytes"] == first_bytes
    same_plan(tracer.refit_plan(), first_plan)
    R.check_wide(wide, tracer.wide_nodes(), bufs[0], g.nodes.cpu().numpy())


# ---- above MRT_DERIVE_MAX_LEVELS depth levels: the host path ----------------------------------------
_CHAIN = []


def deep_chain():
    """(vertices, triangles, buffers) of a chain of 1100 records, boxes fitted: more depth levels
    than the device derivation takes."""
    if not _CHAIN:
        import test_gpu_refit as TR
        verts, tris, bufs = TR.chain_tree(_lib.MRT_DERIVE_MAX_LEVELS + 76, np.random.default_rng(9))
        _CHAIN.append((verts, tris, tuple(R.host_refit(bufs, verts, tris))))
    return _CHAIN[0]


@pytest.mark.parametrize("wide", [1, 0])
def test_device_bind_of_a_tree_too_deep_is_the_host_bind(tracer, wide):
    _, _, bufs = deep_chain()
    tracer.set_config(wide=wide)
    tracer.set_bvh(gpu(bufs))
    want, info = tracer.wide_nodes(), tracer.bind_info()   # with or without an array: the stack bound decides
    tracer.set_bvh(gpu(bufs), on_device=True)
    d = tracer.derive_info()
    assert d["on_device_plan"] == 0 and d["on_device_wide"] == 0
    got = tracer.wide_nodes()
    assert got.size == want.size and R.same_bits_or_nan(got, want)
    assert same_info(tracer.bind_info(), info)
    assert tracer.refit_plan() is None
    tracer.set_config(wide=1)


@pytest.mark.parametrize("how", ["host", "device"])
def test_first_refit_of_a_tree_too_deep_plans_on_the_host(tracer, how):
    verts, tris, bufs = deep_chain()
    tracer.set_config(wide=1)
    g = gpu(bufs)
    tracer.set_bvh(g, on_device=how == "device")
    wide_before = tracer.wide_nodes()
    v2 = R.displaced(verts)
    want = R.host_refit(bufs, v2, tris)
    tracer.refit(v2, tris)
    torch.cuda.synchronize()
    nodes, woop, tri = (x.cpu().numpy() for x in (g.nodes, g.woop, g.tri_index))
    assert R.same_bits_or_nan(nodes, want[0]) and R.same_bits_or_nan(woop, want[1])
    assert np.array_equal(tri, bufs[2])
    order, offsets, src = refit_plan(bufs[0])
    got = tracer.refit_plan()
    assert got is not None and np.array_equal(got[0], order) and np.array_equal(got[1], offsets)
    if wide_before.size:
        assert got[2] is not None and np.array_equal(got[2], src)
        R.check_wide(wide_before, tracer.wide_nodes(), bufs[0], nodes)
    else:
        assert got[2] is None
    assert tracer.derive_info()["on_device_plan"] == 0
    assert tracer.refit_info()["skipped_refs"] == 0


# ---- a refused device bind --------------------------------------------------------------------------
# test_wide_plan.malformed()'s cases whose child refs all stay inside the node array
REFUSED = ["reached twice", "cycle to the root", "cycle to the parent", "unreachable", "one record, self cycle",
           "two records, second unreachable"]


def test_the_refused_cases_are_those_with_every_ref_inside_the_array():
    assert sorted(REFUSED) == sorted(k for k, (_, why) in WP.malformed().items() if why in (WP.TWICE, WP.UNREACHED))


@pytest.mark.parametrize("name", REFUSED)
def test_a_refused_device_bind_leaves_the_tracer_unbound(tracer, name):
    bufs, wide, info, plan = host_side(tracer, "random1500")
    nodes, why = WP.malformed()[name]
    tracer.set_config(wide=1)
    tracer.set_bvh(gpu(bufs), on_device=True)
    with pytest.raises(_lib.MrtError) as e:
        tracer.set_bvh(gpu((nodes.reshape(-1), bufs[1], bufs[2])), on_device=True)
    assert f"mrt error {_lib.MRT_ERR_INVALID_ARG} " in str(e.value)
    assert str(e.value).endswith(why) and WP.host_reason(nodes).endswith(why)   # the host's reason
    rb = RayBuffer(R.frame_rays(R.built("random", 1500, ALPHA)[0], 8, 8), need_closest_hit=True)
    assert tracer.lib.mrt_tracer_trace(tracer._h, rb.rays.data_ptr(), rb.results.data_ptr(), rb.size, 0, None,
                                       None) == _lib.MRT_ERR_NOT_BOUND
    assert tracer.wide_nodes().size == 0
    assert tracer.refit_info()["levels"] == 0
    levels, nsrc = C.c_int32(-1), C.c_int64(-1)
    assert tracer.lib.mrt_tracer_copy_refit_plan(tracer._h, None, None, 0, C.byref(levels), None, 0, C.byref(nsrc)) == 0
    assert levels.value == 0 and nsrc.value == 0 and tracer.refit_plan() is None
    tracer.set_bvh(gpu(bufs), on_device=True)
    assert R.same_bits_or_nan(tracer.wide_nodes(), wide) and same_info(tracer.bind_info(), info)
    same_plan(tracer.refit_plan(), plan)


# ---- info -----------------------------------------------------------------------------------------
def test_derive_info_counts_far_fewer_readbacks_than_nodes(tracer):
    bufs, wide, _, plan = host_side(tracer, "random9000")
    tracer.set_config(wide=1)
    tracer.set_bvh(gpu(bufs), on_device=True)
    d = tracer.derive_info()
    nodes = len(bufs[0]) // 16
    assert d["on_device_plan"] == 1 and d["on_device_wide"] == 1
    assert 0 < d["readbacks"] < nodes and d["readbacks"] <= d["depth_levels"] + 8
    assert 0 < d["launches"] <= 6 * d["depth_levels"] + 4
    assert d["levels"] == len(plan[1]) - 1 and d["wide_nodes"] == wide.size // 32
    assert d["scratch_bytes"] >= 48 * nodes and d["wall_ms"] > 0
    assert d["topo_ms"] > 0 and d["collapse_ms"] > 0 and d["emit_ms"] > 0
