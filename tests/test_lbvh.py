"""The linear BVH build on the CPU: mrth_bvh_build_lbvh (csrc/host/lbvh.cpp over
csrc/lbvh_common.hpp), the CPU statement of the device build (mrt_tracer_build).

  * per scene and max_leaf_size 1, 4, 8: mrt_refit_plan accepts the nodes; the records are the
    radix-tree nodes of more than max_leaf_size triangles, numbered in Karras order, the root
    record 0; every triangle lies in exactly one leaf of 1..max_leaf_size triangles; the leaf
    of rank r at sorted position p owns slots 3p + r up to its terminator at 3(last + 1) + r;
    triIndex holds the ids at the Z rows' slots and zeros elsewhere (lbvh_util.check_tree,
    against a top-down restatement of the tree in Python integers);
  * the sorted leaf sequence is a stable argsort of the keys restated in numpy float32;
  * a refit with the build's own vertices is a fixed point (refit_util.np_refit), one with
    displaced vertices equals mrth_bvh_refit;
  * the oracle's traversal of the tree finds what brute force finds;
  * edge shapes: 1, L and L + 1 triangles, 300 copies of one triangle, a flat scene;
  * geometry at the numeric edges (lbvh_util.edge_geometry: zero-area triangles, scales from
    denormal to overflowing, NaN and infinite vertices, signed zeros): the same four properties,
    NaN rows and boxes compared as NaN;
  * the device entry points check their arguments without a device.
"""
import ctypes as C

import numpy as np
import pytest

import mrt
import lbvh_util as L
import oracle_lib as O
import refit_util as R
from mrt import _lib

SCENE_IDS = [f"{n}{p}" for n, p in L.SCENES]


@pytest.mark.parametrize("max_leaf", L.LEAF_SIZES)
@pytest.mark.parametrize("name,param", L.SCENES, ids=SCENE_IDS)
def test_host_lbvh_is_the_specified_tree(name, param, max_leaf):
    v, t, bufs = L.host_lbvh(name, param, max_leaf)
    got = L.check_tree(bufs, v, t, max_leaf)
    print(f"{name} {param} L={max_leaf}: {got}")
    assert got["records"] == len(bufs[0]) // 16 and got["slots"] == 3 * len(t) + got["leaves"]


@pytest.mark.parametrize("name,param", L.SCENES, ids=SCENE_IDS)
def test_leaf_sequence_is_a_stable_argsort_of_the_numpy_keys(name, param):
    v, t, (_, woop, tri) = L.host_lbvh(name, param, 4)
    live = np.asarray(woop).reshape(-1, 4)[:, 0] != R.TERMINATOR
    assert np.array_equal(tri[live][::3], np.argsort(L.np_codes(v, t), kind="stable"))


@pytest.mark.parametrize("max_leaf", L.LEAF_SIZES)
@pytest.mark.parametrize("name,param", R.SCENES, ids=SCENE_IDS[:len(R.SCENES)])
def test_refit_is_a_fixed_point(name, param, max_leaf):
    v, t, bufs = L.host_lbvh(name, param, max_leaf)
    nodes, woop = R.np_refit(*bufs, v, t)
    assert R.same_nodes(nodes, bufs[0])
    assert np.array_equal(woop, bufs[1])
    v2 = R.displaced(v)
    moved = R.host_refit(bufs, v2, t)
    want_nodes, want_woop = R.np_refit(*bufs, v2, t)
    assert not np.array_equal(moved[1], bufs[1]), "the displacement moved nothing"
    assert R.same_nodes(moved[0], want_nodes)
    assert np.array_equal(moved[1], want_woop)
    assert np.array_equal(moved[2], bufs[2])


def test_refit_is_a_fixed_point_above_the_level_threshold():
    """9000 triangles: the numpy refit at the leaf size with the fewest leaves (it walks leaf by
    leaf in Python), the C++ refit at the others."""
    for max_leaf in L.LEAF_SIZES:
        v, t, bufs = L.host_lbvh(*L.BIG, max_leaf)
        again = R.np_refit(*bufs, v, t) if max_leaf == 8 else R.host_refit(bufs, v, t)[:2]
        assert R.same_nodes(again[0], bufs[0]) and np.array_equal(again[1], bufs[1])


@pytest.mark.parametrize("max_leaf", L.LEAF_SIZES)
@pytest.mark.parametrize("name,param", L.SCENES, ids=SCENE_IDS)
def test_oracle_traversal_finds_what_brute_force_finds(name, param, max_leaf):
    v, _, bufs = L.host_lbvh(name, param, max_leaf)
    L.trace_like_brute_force(O, R.frame_rays(v), bufs)


@pytest.mark.parametrize("max_leaf", L.LEAF_SIZES)
@pytest.mark.parametrize("kind", L.EDGE_SHAPES)
def test_edge_shapes(kind, max_leaf):
    v, t, bufs = L.host_lbvh(kind, None, max_leaf)
    got = L.check_tree(bufs, v, t, max_leaf)
    print(f"{kind} L={max_leaf}: {got}")
    assert got["levels"] >= 1   # the height, as mrt_refit_plan reports it
    if kind == "copies" and max_leaf == 1:
        assert got["records"] == 299 and got["levels"] == 9   # 300 keys split by index bits: ceil(log2 300)
    if kind == "flat":
        assert (L.np_codes(v, t) & np.uint64(0x1249249249249249)).max() == 0   # no z bits
    nodes, woop = R.np_refit(*bufs, v, t)
    assert R.same_nodes(nodes, bufs[0]) and np.array_equal(woop, bufs[1])
    hits = 1 if kind == "one" else 4
    L.trace_like_brute_force(O, R.frame_rays(v), bufs, min_hits=hits)


# ---- geometry at the numeric edges (lbvh_util.edge_geometry) ----------------------------------
# U and V rows of -0.0 are legitimate where triangles have zero area or the rows underflow.
LOOSE_TERMINATORS = ("degenerate", "tiny40", "denormal")


@pytest.mark.parametrize("max_leaf", [1, 8])
@pytest.mark.parametrize("kind", L.EDGE_GEOMETRY)
def test_edge_geometry_host_lbvh_is_the_specified_tree(kind, max_leaf):
    v, t, bufs = L.host_edge(kind, max_leaf)
    got = L.check_tree(bufs, v, t, max_leaf, strict_terminators=kind not in LOOSE_TERMINATORS)
    print(f"{kind} L={max_leaf}: {got}")
    assert got["records"] == len(bufs[0]) // 16 and got["slots"] == 3 * len(t) + got["leaves"]


@pytest.mark.parametrize("kind", L.EDGE_GEOMETRY)
def test_edge_geometry_leaf_sequence_is_a_stable_argsort_of_the_numpy_keys(kind):
    """denormal: ext is denormal; nonfinite: centroids and ext are NaN or infinite."""
    v, t, (nodes, woop, tri) = L.host_edge(kind, 1)
    z, _ = R.leaf_walk(nodes, woop)
    codes = L.np_codes(v, t)
    assert np.array_equal(tri[z], np.argsort(codes, kind="stable"))
    assert len(np.unique(codes)) > len(t) // 2   # the keys still separate the triangles


@pytest.mark.parametrize("max_leaf", [1, 8])
@pytest.mark.parametrize("kind", L.EDGE_GEOMETRY)
def test_edge_geometry_refit_is_a_fixed_point(kind, max_leaf):
    v, t, bufs = L.host_edge(kind, max_leaf)
    nodes, woop = R.np_refit(*bufs, v, t)
    assert R.same_nodes(nodes, bufs[0])
    assert R.same_bits_or_nan(woop, bufs[1])
    again = R.host_refit(bufs, v, t)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, bufs))   # one machine: NaNs bit for bit too


@pytest.mark.parametrize("max_leaf", [1, 8])
@pytest.mark.parametrize("kind", L.EDGE_GEOMETRY)
def test_edge_geometry_oracle_traversal_finds_what_brute_force_finds(kind, max_leaf):
    _, _, bufs = L.host_edge(kind, max_leaf)
    got = L.trace_like_brute_force(O, L.edge_rays(kind), bufs, min_hits=L.edge_min_hits(kind))
    hits = int((got[:, 0] != -1).sum())
    print(f"{kind} L={max_leaf}: {hits} hits")
    if kind in L.SEES_NOTHING:   # every Woop row is +-0 or NaN: t is NaN and no ray hits, by construction
        assert hits == 0


def test_default_leaf_size_and_bad_leaf_sizes():
    v, t = L.scene_arrays("sphere", 12)
    scene = mrt.Scene.from_arrays(v, t)
    default = mrt.Bvh.build_lbvh(scene).buffers()
    want = L.host_lbvh("sphere", 12, _lib.MRT_LBVH_DEFAULT_MAX_LEAF)[2]
    assert all(np.array_equal(a, b) for a, b in zip(default, want))
    for bad in (-1, 9):
        with pytest.raises(_lib.MrtError, match="max_leaf_size"):
            mrt.Bvh.build_lbvh(scene, bad)


def test_device_entry_points_check_their_arguments_without_a_device():
    lib = _lib.trace_lib()
    sizes = [C.c_int64(), C.c_int64(), C.c_int64()]
    refs = [C.byref(s) for s in sizes]
    for n, records, slots in ((1, 1, 5), (2, 1, 9), (3, 2, 13), (9000, 8999, 36001)):
        assert lib.mrt_lbvh_sizes(n, *refs) == 0
        assert [s.value for s in sizes] == [records * 64, slots * 16, slots * 4]
    largest = (2**28 - 2) // 4
    assert lib.mrt_lbvh_sizes(largest, *refs) == 0 and sizes[1].value // 16 < 2**28
    assert lib.mrt_lbvh_sizes(largest + 1, *refs) == _lib.MRT_ERR_TOO_LARGE
    assert lib.mrt_lbvh_sizes(0, *refs) == _lib.MRT_ERR_INVALID_ARG
    assert lib.mrt_lbvh_sizes(5, None, refs[1], refs[2]) == _lib.MRT_ERR_INVALID_ARG

    def build(n, leaf, tracer=None, ptr=None):
        p = _lib.LbvhParams(max_leaf_size=leaf)
        return lib.mrt_tracer_build(tracer, ptr, 3, ptr, n, C.byref(p), ptr, 1 << 40, ptr, 1 << 40, ptr, 1 << 40,
                                    refs[0], refs[1], refs[2], None)
    assert build(1, 4) == _lib.MRT_ERR_INVALID_ARG                       # null tracer and buffers
    assert build(0, 4, ptr=C.c_void_p(256)) == _lib.MRT_ERR_INVALID_ARG  # N < 1
    assert build(1, 9, ptr=C.c_void_p(256)) == _lib.MRT_ERR_INVALID_ARG  # max_leaf_size outside 0..8
    assert build(1, -1, ptr=C.c_void_p(256)) == _lib.MRT_ERR_INVALID_ARG
    assert build(largest + 1, 4, ptr=C.c_void_p(256)) == _lib.MRT_ERR_TOO_LARGE   # scalars are checked first
    assert lib.mrt_tracer_build_info(None, None) == _lib.MRT_ERR_INVALID_ARG
