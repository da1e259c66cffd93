"""What the scene-attribute and tree-cost tests share: a numpy restatement of csrc/scene_common.hpp
written from its definition (float32 step by step, the square root taken by the double sqrt and
rounded to float32, which is the correctly rounded float32 root), the hand-made edge triangles,
and a float64 restatement of the tree's area sums."""
import numpy as np

F = np.float32
DEFAULT_DIFFUSE = np.array([0.75, 0.75, 0.75, 1.0], F)


def _dot(a, b):
    r = np.zeros(a.shape[:-1], F)
    for k in range(3):
        r = (r + (a[..., k] * b[..., k]).astype(F)).astype(F)
    return r


def _normalize(a):
    with np.errstate(all="ignore"):
        length = np.sqrt(_dot(a, a).astype(np.float64)).astype(F)
        rcp = np.where(length != 0, (F(1.0) / length).astype(F), F(0.0)).astype(F)
        s = (F(1.0) * rcp).astype(F)
        return (a * s[..., None]).astype(F)


def normals(v, t):
    """float32 [nt, 3] and the skipped mask; every index of t must be usable or masked."""
    v = np.asarray(v, F).reshape(-1, 3)
    t = np.asarray(t, np.int32).reshape(-1, 3)
    bad = ((t < 0) | (t >= len(v))).any(axis=1)
    safe = np.where(bad[:, None], 0, t) if len(v) else np.zeros_like(t)
    vv = v if len(v) else np.zeros((1, 3), F)
    with np.errstate(all="ignore"):
        v0, v1, v2 = vv[safe[:, 0]], vv[safe[:, 1]], vv[safe[:, 2]]
        a, b = (v1 - v0).astype(F), (v2 - v0).astype(F)
        c = np.stack([((a[:, 1] * b[:, 2]).astype(F) - (a[:, 2] * b[:, 1]).astype(F)).astype(F),
                      ((a[:, 2] * b[:, 0]).astype(F) - (a[:, 0] * b[:, 2]).astype(F)).astype(F),
                      ((a[:, 0] * b[:, 1]).astype(F) - (a[:, 1] * b[:, 0]).astype(F)).astype(F)], axis=1)
        n = _normalize(c)
    n[bad] = 0.0
    return n, bad


def to_abgr(c):
    """uint32 per row of float32 [n, 4]: the host Vec4f::toABGR."""
    c = np.asarray(c, F)
    out = np.zeros(len(c), np.uint32)
    for i, row in enumerate(c):
        r = 0
        for k in range(4):
            x = row[k]
            lo = x if x > 0 else F(0.0)          # a NaN goes to 0
            cl = lo if lo < 1 else F(1.0)
            q = int(float(cl) * 2.0 ** 56)
            r |= ((((q * 255) >> 55) + 1) >> 1) << (8 * k)
        out[i] = r
    return out


def colors(n, diffuse=None):
    """(material, shaded) uint32 [nt] of normals n and diffuse float32 [nt, 4] (None: the default)."""
    d = np.tile(DEFAULT_DIFFUSE, (len(n), 1)) if diffuse is None else np.asarray(diffuse, F).reshape(-1, 4)
    light = _normalize(np.array([[1.0, 2.0, 3.0]], F))[0]
    with np.errstate(all="ignore"):
        k = ((_dot(n, np.broadcast_to(light, n.shape)) * F(0.5)).astype(F) + F(0.5)).astype(F)
        c = np.concatenate([(d[:, :3] * k[:, None]).astype(F), np.ones((len(n), 1), F)], axis=1)
    return to_abgr(d), to_abgr(c)


def restated(v, t, diffuse=None):
    n, bad = normals(v, t)
    mat, sh = colors(n, diffuse)
    return {"normals": n, "material": mat, "shaded": sh, "skipped": int(bad.sum())}


# name -> three vertices (or None where the triangle is given by indices below)
EDGE_TRIANGLES = [
    ("unit_xy", [(0, 0, 0), (1, 0, 0), (0, 1, 0)]),            # normal (0, 0, 1)
    ("unit_yz", [(0, 0, 0), (0, 1, 0), (0, 0, 1)]),            # normal (1, 0, 0)
    ("unit_zx", [(0, 0, 0), (0, 0, 1), (1, 0, 0)]),            # normal (0, 1, 0)
    ("unit_xy_flipped", [(0, 0, 0), (0, 1, 0), (1, 0, 0)]),    # normal (0, 0, -1)
    ("zero_area", [(0.5, -2, 3)] * 3),                         # rcp(0) = 0: normal 0
    ("collinear", [(0, 0, 0), (1, 1, 1), (2, 2, 2)]),
    ("nan_coordinate", [(0, 0, 0), (1, float("nan"), 0), (0, 1, 0)]),
    ("inf_coordinate", [(0, 0, 0), (float("inf"), 0, 0), (0, 1, 0)]),
    ("huge", [(0, 0, 0), (1e20, 0, 0), (0, 1e20, 0)]),         # the cross product overflows: NaN normal
    ("huge_mixed", [(-1e20, 1e20, 0), (1e20, 3e19, 1e20), (2e19, -1e20, 1e20)]),
    ("denormal", [(0, 0, 0), (1e-40, 0, 0), (0, 1e-40, 0)]),   # denormal edges, the cross product underflows to 0
    ("denormal_edge", [(1e-39, 0, 0), (3e-39, 1, 0), (1e-39, 0, 1)]),   # a denormal edge component that counts
    ("tiny", [(0, 0, 0), (1e-19, 0, 0), (0, 1e-19, 0)]),       # the cross product is denormal, its square 0
]
HAND_NORMALS = {"unit_xy": (0, 0, 1), "unit_yz": (1, 0, 0), "unit_zx": (0, 1, 0), "unit_xy_flipped": (0, 0, -1),
                "zero_area": (0, 0, 0), "collinear": (0, 0, 0)}


def edge_mesh():
    """(vertices, triangles, names): the edge triangles, then two with a vertex index of -1 and
    of numVertices."""
    v, t, names = [], [], []
    for name, tri in EDGE_TRIANGLES:
        t.append([len(v), len(v) + 1, len(v) + 2])
        v.extend(tri)
        names.append(name)
    nv = len(v)
    t += [[0, -1, 1], [1, 2, nv]]
    names += ["index_minus_one", "index_num_vertices"]
    return np.array(v, F), np.array(t, np.int32), names


def same_bits_or_nan(a, b):
    """Float arrays equal as bits, a NaN equal to any NaN (the bits of a NaN an operation makes
    differ between x86 and gfx950)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    both_nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | both_nan).all())


def random_diffuse(nt, seed=5):
    return np.random.default_rng(seed).random((nt, 4), dtype=F)


def mixed_mesh(count=1500, seed=3):
    """random(count) with the edge triangles mixed in at scattered positions, and per-triangle
    diffuse colours: (vertices, triangles, diffuse)."""
    import mrt
    v, t, _ = mrt.Scene.synthetic("random", count, seed).arrays()
    ev, et, _ = edge_mesh()
    et = np.where(et < 0, et, et + len(v))      # -1 stays; len(ev) becomes the merged array's numVertices
    vv = np.concatenate([v, ev]).astype(F)
    tt = np.concatenate([t, et]).astype(np.int32)
    order = np.random.default_rng(seed).permutation(len(tt))
    tt = tt[order]
    return vv, tt, random_diffuse(len(tt))


# ---------------------------------------------------------------- tree cost
TERMINATOR = 0x80000000


def leaf_triangles(ref, woop):
    slots = len(woop) // 4
    s, count = ~int(ref), 0
    z = woop.view(np.uint32)
    while s + 2 < slots and z[4 * s] != TERMINATOR:
        count += 1
        s += 3
    return count


def tree_cost(nodes, woop):
    """The float64 restatement: areas dx*dy + dy*dz + dz*dx in double from the float32 planes."""
    rec = np.ascontiguousarray(nodes).view(np.int32).reshape(-1, 16)
    f = rec.view(F).astype(np.float64)
    woop = np.ascontiguousarray(woop).view(np.int32)
    out = {"root_area": 0.0, "inner_area": 0.0, "leaf_area": 0.0, "leaf_tri_area": 0.0, "records": len(rec),
           "leaves": 0, "triangles": 0, "skipped": 0}
    inner, leaf, leaf_tri = [], [], []

    def area(lo, hi):
        with np.errstate(all="ignore"):
            d = hi - lo
            a = d[0] * d[1] + d[1] * d[2] + d[2] * d[0]
        return a, bool((lo <= hi).all() and np.isfinite(a))

    def box(n, side):
        lo = np.array([f[n, 4 * side], f[n, 4 * side + 2], f[n, 8 + 2 * side]])
        hi = np.array([f[n, 4 * side + 1], f[n, 4 * side + 3], f[n, 9 + 2 * side]])
        return lo, hi
    for n in range(len(rec)):
        for side in range(2):
            a, ok = area(*box(n, side))
            ref = rec[n, 12 + side]
            out["skipped"] += 0 if ok else 1
            if ref >= 0:
                if ok:
                    inner.append(a)
                continue
            count = leaf_triangles(ref, woop)
            out["leaves"] += 1
            out["triangles"] += count
            if ok:
                leaf.append(a)
                leaf_tri.append(a * count)
    (lo0, hi0), (lo1, hi1) = box(0, 0), box(0, 1)
    with np.errstate(all="ignore"):
        lo = np.where((lo0 < lo1) | np.isnan(lo1), lo0, lo1)     # woop::box_min / box_max
        hi = np.where((hi0 > hi1) | np.isnan(hi1), hi0, hi1)
    a, ok = area(lo, hi)
    if ok:
        out["root_area"] = a
        inner.append(a)
    else:
        out["skipped"] += 1
    import math
    out["inner_area"], out["leaf_area"], out["leaf_tri_area"] = math.fsum(inner), math.fsum(leaf), math.fsum(leaf_tri)
    return out


def assert_cost_close(got, want, what=""):
    """Counts equal; each sum within records * 2^-52 relative: all terms are non-negative and each
    double addition errs by at most 2^-53 relative, so two summation orders of at most 2 * records
    + 1 terms cannot differ by more."""
    for k in ("records", "leaves", "triangles", "skipped"):
        assert got[k] == want[k], f"{what}: {k} {got[k]} != {want[k]}"
    bound = want["records"] * 2.0 ** -52
    for k in ("root_area", "inner_area", "leaf_area", "leaf_tri_area"):
        g, w = got[k], want[k]
        assert abs(g - w) <= bound * abs(w), f"{what}: {k} {g!r} vs {w!r} (bound {bound:g} relative)"
