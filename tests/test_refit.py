"""Refit of Compact2 buffers for moved vertices, on the CPU: mrth_bvh_refit
(csrc/host/refit.cpp), the refit plan (mrt_refit_plan, csrc/refit_plan.cpp) and the
wide-child source map of the bind-time collapse (csrc/wide_bvh.cpp).

  * identity: without spatial splits (split_alpha 2: refs == tris) a refit with the scene's
    own vertices changes nothing (boxes as float values, everything else as bits);
  * containment: with the default splits the builder's clipped leaf boxes become whole-
    triangle boxes: every refitted box contains the built one, Woop rows stay bit-identical;
  * moved vertices: the host refit equals a numpy restatement (refit_util.np_refit), and the
    oracle's traversal of the refitted tree finds what brute force over the refitted Woop
    rows finds (t bit for bit, ids up to exact-t ties);
  * geometry at the numeric edges (lbvh_util.edge_geometry): a refit of the soup's tree to
    zero-area, scaled, NaN and infinite vertices equals the numpy restatement with NaNs
    compared as NaNs, traces like brute force, and a refit back restores every byte;
  * plan: every node once, inner children in strictly lower levels, for the serialiser's
    numbering and for a renumbered tree; each mapped Compact2 box is the wide child's planes;
  * errors: an out-of-range vertex index or triIndex entry is refused and nothing is written.
"""
import ctypes as C

import numpy as np
import pytest

import mrt
import lbvh_util as L
import oracle_lib as O
import refit_util as R
from mrt import _lib
from mrt.tracer import refit_plan

SENTINEL = 0x76543210
NO_SPLITS = 2.0
DEFAULT_ALPHA = 1e-5


@pytest.mark.parametrize("name,param", R.SCENES)
def test_identity_without_spatial_splits(name, param):
    v, t, bufs, stats = R.built(name, param, NO_SPLITS)
    assert stats["tri_refs"] == len(t), "split_alpha 2 must not split"
    nodes, woop, tri = R.host_refit(bufs, v, t)
    assert R.same_nodes(nodes, bufs[0])
    assert np.array_equal(woop, bufs[1])
    assert np.array_equal(tri, bufs[2])


@pytest.mark.parametrize("name,param", [("random", 1500), ("hairball", 3)])
def test_refitted_boxes_contain_the_built_ones(name, param):
    v, t, bufs, stats = R.built(name, param, DEFAULT_ALPHA)
    assert stats["tri_refs"] > len(t), "the default build of this scene has spatial splits"
    nodes, woop, tri = R.host_refit(bufs, v, t)
    assert np.array_equal(woop, bufs[1])
    assert np.array_equal(tri, bufs[2])
    assert np.array_equal(nodes.reshape(-1, 16)[:, 12:], bufs[0].reshape(-1, 16)[:, 12:])
    new, old = R.boxes(nodes), R.boxes(bufs[0])
    assert (new[:, :, 0::2] <= old[:, :, 0::2]).all() and (new[:, :, 1::2] >= old[:, :, 1::2]).all()
    looser = ((new != old).any(axis=(1, 2))).sum()
    print(f"{name}: {looser} of {len(new)} nodes looser after the refit")
    assert looser > 0   # whole triangles where the builder had clipped


@pytest.fixture(scope="module", params=R.SCENES, ids=lambda s: s[0])
def moved(request):
    name, param = request.param
    v, t, bufs, _ = R.built(name, param, DEFAULT_ALPHA)
    v2 = R.displaced(v)
    return v2, t, bufs, R.host_refit(bufs, v2, t)


def test_moved_vertices_equal_the_numpy_restatement(moved):
    v2, t, bufs, (nodes, woop, tri) = moved
    want_nodes, want_woop = R.np_refit(*bufs, v2, t)
    assert not np.array_equal(woop, bufs[1]), "the displacement moved nothing"
    assert np.array_equal(woop, want_woop)
    assert R.same_nodes(nodes, want_nodes)
    assert np.array_equal(tri, bufs[2])


def test_moved_vertices_trace_like_brute_force(moved):
    v2, _, _, (nodes, woop, tri) = moved
    rays = R.frame_rays(v2)
    got, _, _ = O.trace(rays, nodes, woop, tri)
    want = O.brute_force(rays, woop, tri)
    print(f"{(want[:, 0] != -1).sum()} of {len(rays)} rays hit")
    assert (want[:, 0] != -1).sum() >= 16, "the frame misses the moved scene"
    assert np.array_equal(got[:, 1], want[:, 1])   # t bit for bit
    diff = np.nonzero(got[:, 0] != want[:, 0])[0]   # two triangles at the same t bits
    assert len(O.invalid_hits(rays, got, woop, tri, which=diff)) == 0


# ---- geometry at the numeric edges ------------------------------------------------------
SOUP_KINDS = [k for k in L.EDGE_GEOMETRY if k != "signed_zero"]   # the soup's topology


@pytest.mark.parametrize("max_leaf", [1, 8])
@pytest.mark.parametrize("kind", SOUP_KINDS)
def test_refit_to_edge_geometry_equals_the_numpy_restatement(kind, max_leaf):
    """The soup's tree refitted to collapsed, scaled or non-finite vertices, and back. A NaN
    coordinate enters no box (it would cull the finite triangles beside it); an infinite one does."""
    v0, t, bufs = L.host_edge("soup", max_leaf)
    v, _ = L.edge_geometry(kind)
    nodes, woop, tri = R.host_refit(bufs, v, t)
    want_nodes, want_woop = R.np_refit(*bufs, v, t)
    assert not np.array_equal(woop, bufs[1]), "the refit moved nothing"
    assert R.same_bits_or_nan(woop, want_woop)
    assert R.same_nodes(nodes, want_nodes)
    assert np.array_equal(tri, bufs[2])
    if kind == "nonfinite":
        b = R.boxes(nodes)
        assert not np.isnan(b).any() and np.isinf(b).any()
    back = R.host_refit((nodes, woop, tri), v0, t)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(back, bufs))   # nothing sticks


@pytest.mark.parametrize("kind", SOUP_KINDS)
def test_refitted_edge_geometry_traces_like_brute_force(kind):
    _, t, bufs = L.host_edge("soup", 4)
    refitted = R.host_refit(bufs, L.edge_geometry(kind)[0], t)
    got = L.trace_like_brute_force(O, L.edge_rays(kind), refitted, min_hits=L.edge_min_hits(kind))
    if kind in L.SEES_NOTHING:   # every Woop row is +-0 or NaN: no ray hits, by construction
        assert (got[:, 0] == -1).all()


# ---- the plan -------------------------------------------------------------------------
def renumbered(nodes):
    """The same tree with records 1.. in reverse order (children may precede parents)."""
    n = np.array(nodes, np.int32).reshape(-1, 16)
    k = len(n)
    new_of = np.concatenate([[0], np.arange(k - 1, 0, -1)]).astype(np.int64)   # old -> new
    out = np.empty_like(n)
    out[new_of] = n
    for w in (12, 13):
        ref = out[:, w]
        inner = ref >= 0
        ref[inner] = (new_of[ref[inner] // 4] * 4).astype(np.int32)
    return out.reshape(-1)


def check_levels(nodes, order, offsets):
    n = np.asarray(nodes, np.int32).reshape(-1, 16)
    assert np.array_equal(np.sort(order), np.arange(len(n)))   # every node exactly once
    assert offsets[0] == 0 and offsets[-1] == len(n) and (np.diff(offsets) > 0).all()
    level = np.empty(len(n), np.int64)
    for h in range(len(offsets) - 1):
        level[order[offsets[h]:offsets[h + 1]]] = h
    for i in range(len(n)):
        below = [level[r // 4] for r in n[i, 12:14] if r >= 0]
        assert level[i] == (1 + max(below) if below else 0)   # so every inner child is strictly lower
    assert (np.diff(np.diff(offsets)) <= 0).all()   # level sizes never grow with the height


@pytest.mark.parametrize("name,param", R.SCENES)
def test_plan_levels_and_wide_source_map(name, param):
    _, _, bufs, _ = R.built(name, param, DEFAULT_ALPHA)
    for nodes in (bufs[0], renumbered(bufs[0])):
        order, offsets, src = refit_plan(nodes)
        check_levels(nodes, order, offsets)
        # a freshly derived exact 4-wide array: each mapped Compact2 box is the child's planes, bit for bit
        size = C.c_int64()
        lib = _lib.trace_lib()
        n = np.ascontiguousarray(nodes, np.int32)
        assert lib.mrt_derive_wide_nodes(n.ctypes.data, n.nbytes, None, 0, 1, None, 0, C.byref(size)) == 0
        wide = np.zeros(size.value // 4, np.uint32)
        assert lib.mrt_derive_wide_nodes(n.ctypes.data, n.nbytes, None, 0, 1, wide.ctypes.data, wide.nbytes,
                                         C.byref(size)) == 0
        wide = wide.reshape(-1, 32)
        assert src.shape == (len(wide) * 4,)
        src = src.reshape(-1, 4)
        assert np.array_equal(src < 0, wide[:, 24:28] == SENTINEL)
        rec = n.reshape(-1, 16)
        for c in range(4):
            have = src[:, c] >= 0
            node, side = src[have, c] >> 1, src[have, c] & 1
            words = np.where(side[:, None] == 0, R.box_words(0), R.box_words(1))
            want = rec[node[:, None], words].view(np.uint32)                        # lo.x hi.x lo.y hi.y lo.z hi.z
            base = [(2 * k + (c >> 1)) * 4 + (c & 1) * 2 + e for k in range(3) for e in (0, 1)]
            assert np.array_equal(wide[have][:, base], want)


def test_plan_refuses_what_is_not_a_tree():
    _, _, bufs, _ = R.built("sphere", 12, DEFAULT_ALPHA)
    lib = _lib.trace_lib()
    levels = C.c_int32()

    def rc(nodes):
        n = np.ascontiguousarray(nodes, np.int32)
        return lib.mrt_refit_plan(n.ctypes.data, n.nbytes, None, None, 0, C.byref(levels), None, 0, None)
    assert rc(bufs[0]) == 0 and levels.value > 3
    unreachable = np.concatenate([bufs[0], bufs[0][:16]])
    assert rc(unreachable) == _lib.MRT_ERR_INVALID_ARG
    outside = bufs[0].copy().reshape(-1, 16)
    inner = np.argwhere(outside[:, 12:14] >= 0)[-1]
    outside[inner[0], 12 + inner[1]] = len(outside) * 4
    assert rc(outside) == _lib.MRT_ERR_INVALID_ARG
    twice = bufs[0].copy().reshape(-1, 16)
    refs = np.argwhere(twice[:, 12:14] >= 0)
    twice[refs[-1][0], 12 + refs[-1][1]] = twice[refs[0][0], 12 + refs[0][1]]
    assert rc(twice) == _lib.MRT_ERR_INVALID_ARG


def test_device_entry_points_check_their_arguments_without_a_device():
    lib = _lib.trace_lib()
    assert lib.mrt_tracer_refit(None, None, 0, None, 0, None) == _lib.MRT_ERR_INVALID_ARG
    assert lib.mrt_tracer_refit_info(None, None) == _lib.MRT_ERR_INVALID_ARG
    assert lib.mrt_tracer_copy_wide_nodes(None, None, 0, None) == _lib.MRT_ERR_INVALID_ARG


# ---- errors ---------------------------------------------------------------------------
def test_out_of_range_references_are_refused_and_nothing_is_written():
    v, t, bufs, _ = R.built("random", 1500, DEFAULT_ALPHA)
    v2 = R.displaced(v)

    def refused(bufs_in, verts, tris):
        bvh = mrt.Bvh.from_buffers(*bufs_in)
        with pytest.raises(_lib.MrtError, match="out of range"):
            bvh.refit(verts, tris)
        for got, want in zip(bvh.buffers(), bufs_in):
            assert np.array_equal(got, want)

    for bad in (len(v), -1):
        tris = t.copy()
        tris[len(t) // 2, 1] = bad
        refused(bufs, v2, tris)
    refused(bufs, v2[:-1], t)            # the last vertex is used by some triangle
    refs = bufs[0].reshape(-1, 16)[:, 12:14]
    leaves = refs[refs < 0]
    for bad in (len(t), -5):
        tri = bufs[2].copy()
        tri[R.leaf_slots(bufs[1], leaves[len(leaves) // 2])[0]] = bad
        refused((bufs[0], bufs[1], tri), v2, t)
    refused(bufs, v2, t[:-1])            # triIndex refers to the last triangle
