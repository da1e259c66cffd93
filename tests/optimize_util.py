"""Shared by tests/test_optimize.py and tests/test_gpu_optimize.py: the trees the treelet
restructuring is tried on, the host result computed once per (tree, rounds), and the properties
of a Compact2 node array that a restructuring must keep, restated in numpy."""
import functools

import numpy as np

import lbvh_util as L
import leaf_util as LU
import mrt
import refit_util as R

ALPHA = 1e-5
ROUNDS = [1, 3]
# The trees of the issue's table: host LBVH at max_leaf_size 4.
TABLED = [("hairball", 3), ("random", 1500), ("sphere", 12), ("random", 9000)]

# name -> () -> (vertices, triangles, (nodes, woop, triIndex)), all cached and read-only
TREES = {}
for _name, _param in L.SCENES:
    for _leaf in L.LEAF_SIZES:
        TREES[f"{_name}{_param}-L{_leaf}"] = (lambda n=_name, p=_param, l=_leaf: L.host_lbvh(n, p, l))
# a one-record tree and a tree of height 0 have nothing to do; copies is the deepest; flat has an axis of extent 0
for _kind, _leaf in (("one", 4), ("n_eq_l_plus_1", 4), ("copies", 1), ("copies", 4), ("flat", 4)):
    TREES[f"{_kind}-L{_leaf}"] = (lambda k=_kind, l=_leaf: L.host_lbvh(k, None, l))
for _kind in L.EDGE_GEOMETRY:
    TREES[f"edge-{_kind}"] = (lambda k=_kind: L.host_edge(k, 4))
for _name, _param in R.SCENES:
    TREES[f"sbvh-{_name}{_param}"] = (lambda n=_name, p=_param: R.built(n, p, ALPHA)[:3])
# SBVHs whose leaves hold up to 17 and up to 33 triangles (leaf_util.NATURAL)
BIG_LEAVES = [f"sbvh-{_name}" for _name in LU.NATURAL]
for _name in LU.NATURAL:
    TREES[f"sbvh-{_name}"] = (lambda n=_name: LU.built(n))


def is_lbvh(name):
    return not name.startswith("sbvh-")


@functools.lru_cache(maxsize=None)
def host_optimized(name, rounds):
    """(nodes after Bvh.optimize(rounds), its info) of TREES[name]; cached, read-only."""
    _, _, bufs = TREES[name]()
    bvh = mrt.Bvh.from_buffers(*bufs)
    info = bvh.optimize(rounds)
    nodes, woop, tri = bvh.buffers()
    assert np.array_equal(woop, bufs[1]) and np.array_equal(tri, bufs[2])   # Woop rows and triIndex are not its to touch
    nodes.setflags(write=False)
    return nodes, info


def rays_for(name):
    v = TREES[name]()[0]
    if name.startswith("edge-"):
        kind = name[len("edge-"):]
        return L.edge_rays(kind), L.edge_min_hits(kind)
    few = {"one": 1, "n_eq_l_plus_1": 4, "copies": 4}   # tests/test_lbvh.py's counts for these shapes
    return R.frame_rays(v), few.get(name.split("-")[0], 16)


def objective(nodes):
    """The float64 sum of the areas dx*dy + dy*dz + dz*dx of every inner child's box."""
    b = R.boxes(nodes).astype(np.float64)
    refs = np.ascontiguousarray(nodes).view(np.int32).reshape(-1, 16)[:, 12:14]
    d = b[..., 1::2] - b[..., 0::2]
    area = d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]
    return float(area[refs >= 0].sum())


def leaf_multiset(nodes):
    """The (leaf ref, six box words) rows of every leaf slot, sorted."""
    rec = np.ascontiguousarray(nodes).view(np.int32).reshape(-1, 16)
    rows = []
    for side in range(2):
        leaf = rec[:, 12 + side] < 0
        rows.append(np.concatenate([rec[leaf, 12 + side][:, None], rec[leaf][:, R.box_words(side)]], 1))
    rows = np.concatenate(rows)
    return rows[np.lexsort(rows.T[::-1])]


def not_unions(nodes):
    """The (child ref, six box words) of every inner slot whose box is not, bit for bit, the
    refit's union (refit_util.box_min / box_max, child 0's then child 1's) of the two boxes in
    the child's record."""
    rec = np.ascontiguousarray(nodes).view(np.int32).reshape(-1, 16)
    b = R.boxes(nodes)
    out = set()
    for side in range(2):
        inner = np.nonzero(rec[:, 12 + side] >= 0)[0]
        child = rec[inner, 12 + side] // 4
        c0, c1 = b[child, 0], b[child, 1]
        want = np.empty_like(c0)
        want[:, 0::2] = R.box_min(c0[:, 0::2], c1[:, 0::2])
        want[:, 1::2] = R.box_max(c0[:, 1::2], c1[:, 1::2])
        have = b[inner, side]
        bad = (want.view(np.int32) != have.view(np.int32)).any(1)
        for n in inner[bad]:
            out.add((int(rec[n, 12 + side]),) + tuple(int(x) for x in rec[n, R.box_words(side)]))
    return out


def check_still_a_tree(before, after):
    """Everything a restructuring must keep, from the two node arrays alone."""
    from mrt.tracer import refit_plan
    before = np.ascontiguousarray(before).view(np.int32)
    after = np.ascontiguousarray(after).view(np.int32)
    assert after.shape == before.shape
    refit_plan(after, wide=False)   # mrt_refit_plan accepts the nodes: a tree
    assert (after.reshape(-1, 16)[:, 14:] == 0).all()
    assert np.array_equal(leaf_multiset(after), leaf_multiset(before))
    assert not_unions(after) <= not_unions(before)
