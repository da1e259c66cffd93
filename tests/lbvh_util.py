"""Shared by tests/test_lbvh.py and tests/test_gpu_build.py: the scenes and edge shapes of
the linear BVH build, its keys restated in numpy (float32, one rounding per operation), and
a checker that walks the emitted Compact2 buffers against a top-down restatement of the
radix tree, independent of the library's binary searches; and the edge geometry shared with
tests/test_refit.py and tests/test_gpu_edge_geometry.py: degenerate triangles, scales from
denormal to overflowing, non-finite vertices, signed zeros (edge_geometry)."""
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


# ---- geometry at the numeric edges ---------------------------------------------------------
EDGE_GEOMETRY = ["degenerate", "tiny31", "tiny40", "denormal", "huge30", "huge40", "nonfinite", "signed_zero"]
SEES_NOTHING = ("tiny40", "denormal", "huge40")   # every Woop row is +-0 or NaN: no ray can hit
EDGE_SCALE = {"tiny31": -31, "tiny40": -40, "denormal": -130, "huge30": 30, "huge40": 40}
FLT_MIN = np.finfo(np.float32).tiny


def _degenerate(v):
    """120 of the 800 triangles made zero-area: 40 with two equal vertices, 40 collinear, 40 points.
    The collinear ones are v0, v0 + e, v0 + 2e on a 2^-10 grid, so both edges and every product
    of the cross product are exact and the determinant is 0, not merely small."""
    v = v.reshape(-1, 3, 3).copy()
    pick = np.random.default_rng(5).choice(len(v), 120, replace=False)
    v[pick[:40], 1] = v[pick[:40], 0]
    v0 = np.round(v[pick[40:80], 0] * 1024) / 1024
    e = np.round((v[pick[40:80], 1] - v[pick[40:80], 0]) * 1024) / 1024
    e[(e == 0).all(1)] = 1 / 1024
    v[pick[40:80], 0], v[pick[40:80], 1], v[pick[40:80], 2] = v0, v0 + e, v0 + 2 * e
    v[pick[80:], 1] = v[pick[80:], 2] = v[pick[80:], 0]
    return v.reshape(-1, 3)


def _nonfinite(v):
    """10 triangles each with NaN in vertex 0's x, NaN in vertex 2's y, +inf in vertex 1's z,
    -inf in vertex 2's x."""
    v = v.reshape(-1, 3, 3).copy()
    pick = np.random.default_rng(6).choice(len(v), 40, replace=False)
    v[pick[0:10], 0, 0] = np.nan
    v[pick[10:20], 2, 1] = np.nan
    v[pick[20:30], 1, 2] = np.inf
    v[pick[30:40], 2, 0] = -np.inf
    return v.reshape(-1, 3)


def _signed_zero():
    """A 32 x 32 grid of pairwise disjoint triangles in the plane z = 0 (one per unit cell, inside
    it), z = -0.0 at a random half of the vertices: a flat scene without overlaps, so no ties."""
    rng = np.random.default_rng(7)
    cell = np.stack(np.meshgrid(np.arange(32.0), np.arange(32.0), indexing="ij"), -1).reshape(-1, 1, 2)
    corner = np.array([[0.1, 0.1], [0.8, 0.15], [0.2, 0.85]]) + rng.uniform(0, 0.1, (1024, 3, 2))
    v = np.zeros((1024, 3, 3), np.float32)
    v[:, :, :2] = cell + corner
    v[:, :, 2] = np.where(rng.permutation(3072).reshape(1024, 3) < 1536, -0.0, 0.0)
    return v.reshape(-1, 3), np.arange(3072, dtype=np.int32).reshape(-1, 3)


def _edge_precondition(kind, v, t):
    """A fixture that drifts fails here instead of passing vacuously (on the host build, L = 4)."""
    nodes, woop, tri = mrt.Bvh.build_lbvh(mrt.Scene.from_arrays(v, t), 4).buffers()
    z, _ = R.leaf_walk(nodes, woop)
    rows = woop.view(np.float32).reshape(-1, 4)
    tri_rows = np.stack([rows[z], rows[z + 1], rows[z + 2]], 1).reshape(len(z), 12)
    if kind == "degenerate":   # a U or V row that a scan of first words would take for a terminator
        uv = np.concatenate([z + 1, z + 2])
        assert (woop.reshape(-1, 4)[uv, 0] == R.TERMINATOR).any()
        assert (tri_rows == 0).all(1).sum() >= 100
    if kind == "tiny31":
        assert np.isinf(tri_rows).any()
    if kind == "tiny40":
        assert (tri_rows == 0).all()
    if kind == "denormal":
        planes = np.abs(R.boxes(nodes))
        assert ((planes > 0) & (planes < FLT_MIN)).any()            # a flushed plane would be 0
        assert not np.array_equal(tri[z], np.arange(len(t)))        # flushed keys would all be 0: index order
    if kind == "huge30":
        assert np.isfinite(tri_rows).all()
    if kind == "huge40":
        assert np.isnan(tri_rows).any(1).all() and np.isfinite(R.boxes(nodes)).all()
    if kind == "nonfinite":
        assert np.isnan(tri_rows).any(1).sum() >= 40 and np.isinf(R.boxes(nodes)).any()
    if kind == "signed_zero":
        zplanes = R.boxes(nodes)[:, :, 4:]
        assert (zplanes == 0).all() and np.signbit(zplanes).any() and not np.signbit(zplanes).all()


@functools.lru_cache(maxsize=None)
def edge_geometry(kind):
    """(vertices, triangles) of geometry at a numeric edge; cached, read-only. All but
    signed_zero are the 800-triangle soup _soup(800, 21), so they share a topology."""
    v, t = _soup(800, 21)
    if kind == "soup":
        pass
    elif kind == "degenerate":
        v = _degenerate(v)
    elif kind in EDGE_SCALE:
        v = np.ldexp(v, EDGE_SCALE[kind]).astype(np.float32)   # exact, but for 2^-130's denormals
    elif kind == "nonfinite":
        v = _nonfinite(v)
    elif kind == "signed_zero":
        v, t = _signed_zero()
    else:
        raise KeyError(kind)
    v = np.ascontiguousarray(v, np.float32)
    _edge_precondition(kind, v, t)
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t


@functools.lru_cache(maxsize=None)
def host_edge(kind, max_leaf):
    """(vertices, triangles, (nodes, woop, triIndex)) of the host LBVH of an edge geometry; cached, read-only."""
    v, t = edge_geometry(kind)
    bufs = mrt.Bvh.build_lbvh(mrt.Scene.from_arrays(v, t), max_leaf).buffers()
    for a in bufs:
        a.setflags(write=False)
    return v, t, bufs


@functools.lru_cache(maxsize=None)
def edge_rays(kind):
    """The 64 x 48 frame of refit_util.frame_rays on the geometry's own scale; read-only. A
    camera cannot be fitted to non-finite vertices: that kind is seen from the soup's camera."""
    rays = R.frame_rays(edge_geometry("soup" if kind == "nonfinite" else kind)[0])
    rays.setflags(write=False)
    return rays


def edge_min_hits(kind):
    """16 where the frame must see the geometry; 0 where no ray can hit (SEES_NOTHING)."""
    return 0 if kind in SEES_NOTHING else 16


# ---- the keys in numpy -------------------------------------------------------------------
def np_codes(v, t):
    """The 63-bit Morton code per triangle as Python-int-exact uint64, after the comments of
    lbvh_common.hpp: the centroid is (bmin + bmax) * 0.5 with bmin / bmax folded over vertices
    0, 1, 2 by (a < b) ? a : b; a NaN centroid never enters the bounds; q is 0 unless ext > 0,
    else min(2097151, (uint32)((c - lo) / ext * 2097152)) with a NaN to 0."""
    p = np.asarray(v, np.float32)[np.asarray(t)]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = (R.fw_min(R.fw_min(p[:, 0], p[:, 1]), p[:, 2]) + R.fw_max(R.fw_max(p[:, 0], p[:, 1]), p[:, 2])) * F(0.5)
        lo = np.fmin.reduce(c, 0, initial=F(np.inf))    # fmin / fmax drop a NaN
        hi = np.fmax.reduce(c, 0, initial=F(-np.inf))
        ext = hi - lo
    code = np.zeros(len(p), np.uint64)
    for k in range(3):
        q = np.zeros(len(p), np.uint64)
        if ext[k] > 0:
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                f = (c[:, k] - lo[k]) / ext[k] * F(2097152.0)
            assert f.dtype == np.float32
            q = np.where(f >= 0, np.minimum(f, F(2097151.0)), F(0)).astype(np.uint64)   # a NaN is not >= 0
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


def check_tree(bufs, v, t, max_leaf, strict_terminators=True):
    """Every property of the specification that the buffers alone show; returns
    {"records", "leaves", "slots", "levels"}. The terminators and the Z rows' slots are those a
    walk from the leaf refs finds (refit_util.leaf_walk). strict_terminators: besides, no other
    slot has a first word 0x80000000; false only for geometry with zero-area triangles or rows
    that underflow, whose U and V rows may be -0.0."""
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
    z_slots, term_slots = R.leaf_walk(nodes, woop)
    assert len(np.unique(z_slots)) == len(z_slots) and len(np.unique(term_slots)) == len(term_slots)
    assert 3 * len(z_slots) + len(term_slots) == len(w)    # the leaves tile the array
    term = np.zeros(len(w), bool)
    term[term_slots] = True
    assert not term[z_slots].any() and not term[z_slots + 1].any() and not term[z_slots + 2].any()
    assert (w[term] == R.TERMINATOR).all()                 # a terminator is four words 0x80000000
    if strict_terminators:
        assert np.array_equal(term, w[:, 0] == R.TERMINATOR)   # and nothing else starts with that word
        assert np.array_equal(term, (w == R.TERMINATOR).all(1))

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
    assert np.array_equal(np.nonzero(~term)[0][::3], z_slots)
    assert np.array_equal(np.sort(tri[z_slots]), np.arange(n))      # every triangle in exactly one leaf, once
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
