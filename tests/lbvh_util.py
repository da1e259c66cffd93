"""Shared by tests/test_lbvh.py and tests/test_gpu_build.py: the scenes and edge shapes of
the linear BVH build, its keys restated in numpy (float32, one rounding per operation), and
a checker that walks the emitted Compact2 buffers against a top-down restatement of the
radix tree, independent of the library's binary searches."""
import bisect
import functools

import numpy as np

import mrt
import refit_util as R
from mrt.tracer import refit_plan

F = np.float32
LEAF_SIZES = [1, 4, 8]
BIG = ("random", 9000)   # a multi-block sort, and a level above the refit's 1024-node launch threshold
SCENES = R.SCENES + [BIG]


@functools.lru_cache(maxsize=None)
def scene_arrays(name, param):
    v, t, _ = mrt.Scene.synthetic(name, param, 1).arrays()
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t


def _soup(n, seed, flat=False):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1, 1, (n, 1, 3))
    v = (centres + rng.uniform(-0.2, 0.2, (n, 3, 3))).astype(np.float32)
    if flat:
        # Every box centre at z = 0.25 exactly (lo + hi = 0.5), so that axis has extent 0. The
        # triangles themselves are tilted: overlapping coplanar ones would tie at hit distances
        # one ulp apart, which the traversal's box culling and brute force resolve differently.
        a = (np.round(rng.uniform(0.0625, 0.125, n) * 2**16) / 2**16).astype(np.float32)   # 0.25 +- a is exact
        v[:, 0, 2] = F(0.25) - a
        v[:, 1, 2] = F(0.25) + a
        v[:, 2, 2] = F(0.25) + a * rng.uniform(-0.5, 0.5, n).astype(np.float32)
    return v.reshape(-1, 3), np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def edge_shape(kind, max_leaf):
    """(vertices, triangles) of an edge shape; cached, read-only."""
    if kind == "one":
        v, t = _soup(1, 11)
    elif kind == "n_eq_l":
        v, t = _soup(max_leaf, 12)
    elif kind == "n_eq_l_plus_1":
        v, t = _soup(max_leaf + 1, 13)
    elif kind == "copies":   # 300 copies of one triangle: all codes equal, the index tie-break
        v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], np.float32)
        t = np.tile(np.array([[0, 1, 2]], np.int32), (300, 1))
    elif kind == "flat":
        v, t = _soup(700, 14, flat=True)
    else:
        raise KeyError(kind)
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t


EDGE_SHAPES = ["one", "n_eq_l", "n_eq_l_plus_1", "copies", "flat"]


@functools.lru_cache(maxsize=None)
def host_lbvh(kind_or_name, param, max_leaf):
    """(vertices, triangles, (nodes, woop, triIndex)) of the host LBVH; cached, read-only.
    param None: an edge shape."""
    v, t = edge_shape(kind_or_name, max_leaf) if param is None else scene_arrays(kind_or_name, param)
    bufs = mrt.Bvh.build_lbvh(mrt.Scene.from_arrays(v, t), max_leaf).buffers()
    for a in bufs:
        a.setflags(write=False)
    return v, t, bufs


# ---- the keys in numpy -------------------------------------------------------------------
def np_codes(v, t):
    """The 63-bit Morton code per triangle as Python-int-exact uint64."""
    p = np.asarray(v, np.float32)[np.asarray(t)]
    c = (p.min(1) + p.max(1)) * F(0.5)
    lo, hi = c.min(0), c.max(0)
    ext = hi - lo
    code = np.zeros(len(p), np.uint64)
    for k in range(3):
        q = np.zeros(len(p), np.uint64)
        if ext[k] > 0:
            f = (c[:, k] - lo[k]) / ext[k] * F(2097152.0)
            assert f.dtype == np.float32
            q = np.minimum(np.where(f >= 0, f, 0).astype(np.uint64), 2097151).astype(np.uint64)
        for bit in range(21):
            code |= ((q >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + (2 - k))
    return code


# ---- the tree, top-down ------------------------------------------------------------------
def expected_tree(codes_sorted, max_leaf):
    """The radix tree over keys (code, sorted position), split top-down at the highest
    differing bit: {"kept": [(karras index, first, last, split)], "leaves": [(first, last)]}
    with leaves in sorted order. Needs more than max_leaf keys."""
    n = len(codes_sorted)
    keys = [(int(c) << 32) | i for i, c in enumerate(codes_sorted)]
    kept, leaves = [], []
    stack = [(0, 0, n - 1)]
    while stack:
        index, f, l = stack.pop()
        d = (keys[f] ^ keys[l]).bit_length()
        g = bisect.bisect_left(keys, ((keys[f] >> (d - 1)) + 1) << (d - 1), f, l + 1) - 1
        kept.append((index, f, l, g))
        for cf, cl, ci in ((f, g, g), (g + 1, l, g + 1)):
            if cl - cf + 1 > max_leaf:
                stack.append((ci, cf, cl))
            else:
                leaves.append((cf, cl))
    return {"kept": sorted(kept), "leaves": sorted(leaves)}


def check_tree(bufs, v, t, max_leaf):
    """Every property of the specification that the buffers alone show; returns
    {"records", "leaves", "slots", "levels"}."""
    nodes, woop, tri = (np.asarray(a, np.int32) for a in bufs)
    n = len(t)
    rec = nodes.reshape(-1, 16)
    w = woop.reshape(-1, 4)
    assert len(tri) == len(w)
    assert (rec[:, 14:] == 0).all()
    _, offsets, _ = refit_plan(nodes, wide=False)   # mrt_refit_plan accepts the nodes: a tree
    codes = np_codes(v, t)
    order = np.argsort(codes, kind="stable")            # equal codes stay in index order
    codes_sorted = codes[order]
    term = (w == R.TERMINATOR).all(1)
    assert np.array_equal(term, w[:, 0] == R.TERMINATOR)   # a terminator is four words 0x80000000

    if n <= max_leaf:
        assert len(rec) == 1 and len(w) == 3 * n + 2
        assert rec[0, 12] == ~0 and rec[0, 13] == ~(3 * n + 1)
        assert np.array_equal(np.nonzero(term)[0], [3 * n, 3 * n + 1])
        want_tri = np.zeros(len(w), np.int32)
        want_tri[0:3 * n:3] = order
        assert np.array_equal(tri, want_tri)
        assert np.array_equal(R.boxes(nodes)[0, 0], R.boxes(nodes)[0, 1])   # the empty leaf copies child 0's box
        return {"records": 1, "leaves": 2, "slots": len(w), "levels": len(offsets) - 1}

    want = expected_tree(codes_sorted, max_leaf)
    leaves = want["leaves"]
    assert len(rec) == len(want["kept"])                # Karras nodes with more than max_leaf triangles
    assert len(w) == 3 * n + len(leaves)
    rank_of_leaf = {f: r for r, (f, _) in enumerate(leaves)}
    record_of = {index: r for r, (index, _, _, _) in enumerate(want["kept"])}   # rank in Karras-index order
    assert want["kept"][0][0] == 0                      # the root is record 0
    want_tri = np.zeros(len(w), np.int32)
    want_term = np.zeros(len(w), bool)
    for r, (f, l) in enumerate(leaves):
        assert 1 <= l - f + 1 <= max_leaf
        want_tri[3 * f + r:3 * (l + 1) + r:3] = order[f:l + 1]
        want_term[3 * (l + 1) + r] = True
    assert np.array_equal(tri, want_tri)                # sorted order at the Z rows' slots, zeros elsewhere
    assert np.array_equal(term, want_term)
    assert np.array_equal(np.sort(tri[~term][::3]), np.arange(n))   # every triangle in exactly one leaf, once
    for index, f, l, g in want["kept"]:
        refs = rec[record_of[index], 12:14]
        for ref, (cf, cl, ci) in zip(refs, ((f, g, g), (g + 1, l, g + 1))):
            if cl - cf + 1 > max_leaf:
                assert ref == 4 * record_of[ci]
            else:
                assert ref == ~(3 * cf + rank_of_leaf[cf])
    return {"records": len(rec), "leaves": len(leaves), "slots": len(w), "levels": len(offsets) - 1}


def trace_like_brute_force(O, rays, bufs, min_hits=16):
    """The oracle's traversal finds what brute force finds: t bit for bit, ids up to exact-t ties."""
    nodes, woop, tri = bufs
    got, _, _ = O.trace(rays, nodes, woop, tri)
    want = O.brute_force(rays, woop, tri)
    assert (want[:, 0] != -1).sum() >= min_hits, "the frame misses the scene"
    assert np.array_equal(got[:, 1], want[:, 1])
    diff = np.nonzero(got[:, 0] != want[:, 0])[0]
    assert len(O.invalid_hits(rays, got, woop, tri, which=diff)) == 0
    return got
