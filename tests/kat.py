"""Hand-built Compact2 BVHs with known answers (shared by the CPU oracle tests
and the GPU parity tests).

Every triangle here is an axis-aligned right triangle with power-of-two
extents, so its Woop rows (the inverse of [v0-v2, v1-v2, n, v2],
reference CudaBVH.cc:361-380) are exact in float32 and every expected t below
is exactly representable: the answers are computed by hand, not by the code
under test.
"""
from __future__ import annotations

import numpy as np

SENTINEL = 0x76543210
NEG_ZERO = np.int32(-2147483648)   # 0x80000000: the -0.0 terminator


def f2i(x: float) -> int:
    return int(np.float32(x).view(np.int32))


def woop_rows(v0, v1, v2):
    """Exact Woop rows (Z, U, V) via float64 inverse (exact for these triangles)."""
    v0, v1, v2 = (np.asarray(v, np.float64) for v in (v0, v1, v2))
    e0, e1 = v0 - v2, v1 - v2
    n = np.cross(e0, e1)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = e0, e1, n, v2
    inv = np.linalg.inv(m)
    z = np.array([inv[2, 0], inv[2, 1], inv[2, 2], -inv[2, 3]])
    rows = np.stack([z, inv[0], inv[1]]).astype(np.float32)
    assert np.all(rows.astype(np.float64) == np.stack([z, inv[0], inv[1]])), "triangle is not exactly representable"
    rows[0, 0] = rows[0, 0] + np.float32(0.0)   # -0.0 -> +0.0 in Z.x (CudaBVH.cc:316-317)
    return rows


class Compact2Builder:
    """Tiny explicit Compact2 writer: inner nodes are (box0, box1, child0, child1)."""

    def __init__(self):
        self.nodes = []      # list of 16-int records
        self.woop = []       # list of 4-float rows
        self.tri_index = []

    def leaf(self, tris):
        """tris: list of (id, v0, v1, v2). Returns the ~offset child reference."""
        ref = ~len(self.woop)
        for tid, v0, v1, v2 in tris:
            for r in woop_rows(v0, v1, v2):
                self.woop.append(r.view(np.int32))
            self.tri_index += [tid, 0, 0]
        self.woop.append(np.full(4, NEG_ZERO, np.int32))
        self.tri_index.append(0)
        return ref

    def reserve_inner(self):
        idx = len(self.nodes)
        self.nodes.append(None)
        return idx

    def set_inner(self, idx, box0, box1, c0, c1):
        (l0, h0), (l1, h1) = box0, box1
        f = np.array([l0[0], h0[0], l0[1], h0[1], l1[0], h1[0], l1[1], h1[1], l0[2], h0[2], l1[2], h1[2]],
                     np.float32).view(np.int32)
        self.nodes[idx] = np.concatenate([f, np.array([c0, c1, 0, 0], np.int32)])
        return idx * 4   # float4 index

    def buffers(self):
        nodes = np.concatenate(self.nodes).astype(np.int32)
        woop = np.concatenate(self.woop).astype(np.int32)
        return nodes, woop, np.array(self.tri_index, np.int32)


def ray(o, d, tmin=0.0, tmax=100.0):
    return np.array([o[0], o[1], o[2], tmin, d[0], d[1], d[2], tmax], np.float32)


def scene_two_floors(pad=0.0):
    """Root with two leaves.
    leaf A (child 0): tri 7 = unit right triangle in the plane z = 0,
                      tri 3 = the same footprint at z = -2.
    leaf B (child 1): tri 5 = right triangle of leg 2 in the plane z = -1, shifted to x in [2, 4].
    pad widens leaf A's box in x and y, so that a ray just outside a triangle's edge still
    reaches the triangle test.
    """
    b = Compact2Builder()
    root = b.reserve_inner()
    A = b.leaf([(7, (0, 0, 0), (1, 0, 0), (0, 1, 0)),
                (3, (0, 0, -2), (1, 0, -2), (0, 1, -2))])
    B = b.leaf([(5, (2, 0, -1), (4, 0, -1), (2, 2, -1))])
    b.set_inner(root, ((-pad, -pad, -2), (1 + pad, 1 + pad, 0)), ((2, 0, -1), (4, 2, -1)), A, B)
    return b.buffers()


def scene_two_floors_padded():
    """scene_two_floors with leaf A's box half a unit wider on every side in x and y: the edge
    and vertex cases are decided by the triangle test's compares, not by a box face."""
    return scene_two_floors(0.5)


def scene_near_second():
    """Root with two leaves whose boxes and triangles disagree about what is near, for a ray
    down -z from z = 1 through (0.25, 0.25):
    child 0: box z = -1 (entered at t = 2), tri 30 in the plane z = -1 (t = 2);
    child 1: box z in [-3, 0.5] (entered at t = 0.5), tri 31 in the plane z = -3 (t = 4).
    c1min < c0min, so the binary order enters child 1 first and tests tri 31 before tri 30."""
    b = Compact2Builder()
    root = b.reserve_inner()
    near = b.leaf([(30, (0, 0, -1), (1, 0, -1), (0, 1, -1))])
    far = b.leaf([(31, (0, 0, -3), (1, 0, -3), (0, 1, -3))])
    b.set_inner(root, ((0, 0, -1), (1, 1, -1)), ((0, 0, -3), (1, 1, 0.5)), near, far)
    return b.buffers()


def scene_tie_one_leaf():
    """Two coincident triangles (20 then 21, plane z = -1) in one leaf; the sibling leaf holds
    tri 22 far to the side."""
    b = Compact2Builder()
    root = b.reserve_inner()
    pair = b.leaf([(20, (0, 0, -1), (1, 0, -1), (0, 1, -1)),
                   (21, (0, 0, -1), (1, 0, -1), (0, 1, -1))])
    side = b.leaf([(22, (2, 0, -1), (4, 0, -1), (2, 2, -1))])
    b.set_inner(root, ((0, 0, -1), (1, 1, -1)), ((2, 0, -1), (4, 2, -1)), pair, side)
    return b.buffers()


def scene_tie_two_leaves():
    """The same coincident pair, tri 20 in child 0 and tri 21 in child 1, under equal boxes:
    c0min == c1min, so the binary order does not swap and enters child 0 first."""
    b = Compact2Builder()
    root = b.reserve_inner()
    first = b.leaf([(20, (0, 0, -1), (1, 0, -1), (0, 1, -1))])
    second = b.leaf([(21, (0, 0, -1), (1, 0, -1), (0, 1, -1))])
    box = ((0, 0, -1), (1, 1, -1))
    b.set_inner(root, box, box, first, second)
    return b.buffers()


def scene_deep():
    """Inner root -> inner child -> two leaves, plus a leaf sibling:
    exercises push/pop ordering. Triangles are stacked along -z at x,y in [0,1]."""
    b = Compact2Builder()
    root = b.reserve_inner()
    inner = b.reserve_inner()
    near = b.leaf([(10, (0, 0, -1), (1, 0, -1), (0, 1, -1))])
    far = b.leaf([(11, (0, 0, -3), (1, 0, -3), (0, 1, -3))])
    side = b.leaf([(12, (0, 0, -2), (1, 0, -2), (0, 1, -2))])
    cinner = b.set_inner(inner, ((0, 0, -1), (1, 1, -1)), ((0, 0, -3), (1, 1, -3)), near, far)
    b.set_inner(root, ((0, 0, -3), (1, 1, -1)), ((0, 0, -2), (1, 1, -2)), cinner, side)
    return b.buffers()


# (name, scene builder, rays, any_hit, expected [(id, t)]) — hand-derived.
def cases():
    out = []
    two = scene_two_floors
    down = (0, 0, -1)
    out.append(("closest: near floor", two, [ray((0.25, 0.25, 1), down)], False, [(7, 1.0)]))
    out.append(("closest: far leaf only", two, [ray((2.5, 0.5, 1), down)], False, [(5, 2.0)]))
    out.append(("miss keeps tmax", two, [ray((8, 8, 1), down, tmax=50.0)], False, [(-1, 50.0)]))
    out.append(("tmin skips the near floor", two, [ray((0.25, 0.25, 1), down, tmin=1.5)], False, [(3, 3.0)]))
    out.append(("tmax cuts before the far floor", two, [ray((0.25, 0.25, 1), down, tmin=1.5, tmax=2.5)], False,
                [(-1, 2.5)]))
    out.append(("tmin == tmax never hits", two, [ray((0.25, 0.25, 1), down, tmin=1.0, tmax=1.0)], False,
                [(-1, 1.0)]))
    out.append(("degenerate AO ray tmax=-1", two, [ray((0.25, 0.25, 1), down, tmin=0.0, tmax=-1.0)], True,
                [(-1, -1.0)]))
    out.append(("upward ray from below", two, [ray((0.25, 0.25, -4), (0, 0, 1))], False, [(3, 2.0)]))
    out.append(("any-hit stops at the first tested (tri 7 before 3)", two, [ray((0.25, 0.25, 1), down)], True,
                [(7, 1.0)]))
    out.append(("any-hit from below: first tested in the leaf is still 7", two,
                [ray((0.25, 0.25, -4), (0, 0, 1))], True, [(7, 4.0)]))
    out.append(("outside the triangle (u+v>1)", two, [ray((0.75, 0.75, 1), down)], False, [(-1, 100.0)]))
    out.append(("parallel ray misses (2^-80 clamp)", two, [ray((-1, 0.25, 0.0 + 0.5), (1, 0, 0))], False,
                [(-1, 100.0)]))
    deep = scene_deep
    out.append(("deep: nearest of three stacked", deep, [ray((0.25, 0.25, 0), down)], False, [(10, 1.0)]))
    out.append(("deep: tmin=1.5 -> middle (other subtree)", deep, [ray((0.25, 0.25, 0), down, tmin=1.5)], False,
                [(12, 2.0)]))
    out.append(("deep: tmin=2.5 -> farthest", deep, [ray((0.25, 0.25, 0), down, tmin=2.5)], False, [(11, 3.0)]))
    out.append(("deep: from below, nearest is 11", deep, [ray((0.25, 0.25, -5), (0, 0, 1))], False, [(11, 2.0)]))
    out += boundary_cases()
    return out


def boundary_cases():
    """The compare boundaries of the reference's tests (t > tmin && t < hitT, u >= 0, v >= 0,
    u + v <= 1, cmax >= cmin), each from both sides.

    Tri 7 is v0 = (0, 0, 0), v1 = (1, 0, 0), v2 = (0, 1, 0): a point (x, y) of its plane has
    u = 1 - x - y (along v0 - v2) and v = x (along v1 - v2), so u = 0 is the hypotenuse, v = 0
    the edge x = 0 and u + v = 1 the edge y = 0; v2 is (u, v) = (0, 0), v0 is (1, 0), v1 is
    (0, 1). Every coordinate below is a sum of a few powers of two, so u, v and u + v are exact.
    Tri 3 repeats the footprint at z = -2, so a ray outside an edge fails the same compare twice."""
    out = []
    pad = scene_two_floors_padded
    two = scene_two_floors
    down = (0, 0, -1)
    e = 2.0 ** -20
    for name, xy in (("edge u = 0", (0.5, 0.5)), ("edge v = 0", (0.0, 0.5)), ("edge u + v = 1", (0.5, 0.0)),
                     ("vertex v2 (u = v = 0)", (0.0, 1.0)), ("vertex v0 (u = 1)", (0.0, 0.0)),
                     ("vertex v1 (v = 1)", (1.0, 0.0))):
        out.append((f"{name} hits", pad, [ray((*xy, 1), down)], False, [(7, 1.0)]))
    for name, xy in (("u = -2^-20", (0.5, 0.5 + e)), ("v = -2^-20", (-e, 0.5)), ("u + v = 1 + 2^-20", (0.5, -e))):
        out.append((f"outside an edge ({name}) misses", pad, [ray((*xy, 1), down)], False, [(-1, 100.0)]))
    one = np.float32(1.0)
    below, above = float(np.nextafter(one, np.float32(0))), float(np.nextafter(one, np.float32(2)))
    out.append(("t == tmin is excluded: the far floor", two, [ray((0.25, 0.25, 1), down, tmin=1.0)], False, [(3, 3.0)]))
    out.append(("tmin one ulp below t: found", two, [ray((0.25, 0.25, 1), down, tmin=below)], False, [(7, 1.0)]))
    out.append(("t == tmax is excluded, tmax kept", two, [ray((0.25, 0.25, 1), down, tmax=1.0)], False, [(-1, 1.0)]))
    out.append(("tmax one ulp above t: found", two, [ray((0.25, 0.25, 1), down, tmax=above)], False, [(7, 1.0)]))
    # in the plane z = -2 of tri 3, along +x: Oz = 0 and Dz = 0, t = 0 * inf = NaN fails t > tmin;
    # tri 7 (Oz = 2, Dz = 0) gives t = inf, which fails t < hitT
    out.append(("in-plane ray (0 * inf = NaN) misses", two, [ray((-1, 0.25, -2), (1, 0, 0))], False, [(-1, 100.0)]))
    # from inside leaf A's box between the floors: tri 7 is at t = -0.5, tri 3 at t = 1.5 >= tmax
    out.append(("hit behind the origin is a miss", two, [ray((0.25, 0.25, -0.5), down, tmax=1.0)], False, [(-1, 1.0)]))
    out.append(("tmax = +inf: hit", two, [ray((0.25, 0.25, 1), down, tmax=np.inf)], False, [(7, 1.0)]))
    out.append(("tmax = +inf: miss keeps +inf", two, [ray((8, 8, 1), down, tmax=np.inf)], False, [(-1, np.inf)]))
    out.append(("direction components of -0.0", two, [ray((0.25, 0.25, 1), (-0.0, -0.0, -1))], False, [(7, 1.0)]))
    out.append(("closest hit in the child entered second", scene_near_second, [ray((0.25, 0.25, 1), down)], False,
                [(30, 2.0)]))
    return out


# (name, scene builder, rays, any_hit, per-lane [(id, t)], allowed [{(id, t), ...}]): cases whose answer
# depends on the order in which triangles are tested. The per-lane Compact2 traversal (and the oracle)
# tests them in the reference's binary order and gives exactly the per-lane answer (closest hit keeps
# the first of equal t: the compare is a strict t < hitT); any other kernel may test them in another
# order and return any member of the allowed set, whose t is still exact.
def tie_cases():
    out = []
    down = (0, 0, -1)
    r = [ray((0.25, 0.25, 1), down)]
    pair = [{(20, 2.0), (21, 2.0)}]
    for any_hit in (False, True):
        kind = "any" if any_hit else "closest"
        out.append((f"tie in one leaf ({kind})", scene_tie_one_leaf, r, any_hit, [(20, 2.0)], pair))
        out.append((f"tie across sibling leaves ({kind})", scene_tie_two_leaves, r, any_hit, [(20, 2.0)], pair))
    # the any-hit twin of "closest hit in the child entered second": child 1 (tri 31) is entered first
    out.append(("any-hit returns the first tested, the farther one", scene_near_second, r, True, [(31, 4.0)],
                [{(30, 2.0), (31, 4.0)}]))
    return out


# ---- the leaf gallery: leaves of 1 to 33 triangles with known answers ---------------------------
GALLERY_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, 20, 33)
GALLERY_CELL = 8.0      # cell c lies in y in [8c, 8c + 1]: seven units of nothing between two cells
GALLERY_LEVELS = 5      # 32 cells under a balanced binary tree: five inner nodes above every leaf


def gallery_cells():
    """(kind, L) per cell, in y order and in the order of the Woop array: a row leaf and a stack
    leaf per size, the 16-triangle row first (a leaf too long for a count opens the array) and
    the 33-triangle stack last (nothing follows its terminator)."""
    rows = [("row", n) for n in GALLERY_SIZES]
    rows.insert(0, rows.pop(GALLERY_SIZES.index(16)))
    return rows + [("stack", n) for n in GALLERY_SIZES]


def leaf_gallery():
    """One Compact2 tree whose 32 leaves hold 1 to 33 triangles, every coordinate a multiple of
    1/8, and rays that put the deciding triangle at every list position of every leaf.

    Each leaf has a cell of its own in y, so a ray down -z aimed at one leaf enters no other
    leaf's box, and at each of the five levels above it exactly one child box (the boxes are the
    exact unions of their cells, disjoint in y between siblings).

    Row leaf of L: list position p is the unit right triangle at x in [2p, 2p + 1] in the plane
    z = -1. Ray p comes down on it from z = 1: the only hit, t = 2, whatever the mode or the order.
    One more ray comes down between two triangles (beside the hypotenuse of the only one, L = 1),
    inside the leaf's box: L rejects, a miss that keeps tmax.

    Stack leaf of L: one footprint, list position k in the plane z = -1 - (L - 1 - k) / 4: the
    farthest first. From z = 1 position k is hit at t = 2 + (L - 1 - k) / 4. The full ray's
    closest hit is the last position at t = 2; an any-hit ray takes the first accepted in the
    order tested: position 0 in list order. The short ray j (tmax = 2 + j / 4 + 1 / 8) can
    accept only the j + 1 nearest, positions L - 1 - j and later: the closest is the last still,
    the first accepted in list order position L - 1 - j, after L - 1 - j tested rejects. A
    closest-hit ray cannot leave a leaf it entered (at t = 2 < tmax) before its end: L triangles
    tested, one leaf finished, five binary nodes fetched; at least two 4-wide nodes, each of which
    takes in at most three of the five binary ones.

    Returns a dict: bufs; rays float32 [384, 8]; hand [(ray, any_hit, exact (id, t), allowed set
    or None)] and bounds [(ray, any_hit, binary nodes, wide nodes, triangles, leaves)] as
    test_gpu_variants.Batch takes them; leaves [(kind, L, leaf ref, ray indices)]."""
    b = Compact2Builder()
    cells = gallery_cells()
    assert len(cells) == 1 << GALLERY_LEVELS
    next_id = [100]
    ids, refs = {}, {}

    def cell_box(c):
        kind, n = cells[c]
        y = GALLERY_CELL * c
        if kind == "row":
            return ((0, y, -1), (2 * n - 1, y + 1, -1))
        return ((0, y, -1 - (n - 1) / 4), (1, y + 1, -1))

    def make_leaf(c):
        kind, n = cells[c]
        y = GALLERY_CELL * c
        tris = []
        for k in range(n):
            x, z = (2.0 * k, -1.0) if kind == "row" else (0.0, -1.0 - (n - 1 - k) / 4)
            tris.append((next_id[0], (x, y, z), (x + 1, y, z), (x, y + 1, z)))
            next_id[0] += 7   # distinct, and no id its own list position
        ids[c] = [t[0] for t in tris]
        refs[c] = b.leaf(tris)
        return refs[c]

    def union(lo, hi):
        boxes = [cell_box(c) for c in range(lo, hi)]
        return (tuple(min(bx[0][a] for bx in boxes) for a in range(3)),
                tuple(max(bx[1][a] for bx in boxes) for a in range(3)))

    def build(lo, hi):
        if hi - lo == 1:
            return make_leaf(lo)
        idx = b.reserve_inner()
        mid = (lo + hi) // 2
        c0, c1 = build(lo, mid), build(mid, hi)
        return b.set_inner(idx, union(lo, mid), union(mid, hi), c0, c1)

    build(0, len(cells))
    bufs = b.buffers()
    assert ~refs[0] == 0 and len(ids[0]) == 16                           # a long leaf opens the Woop array
    assert ~refs[len(cells) - 1] + 3 * 33 + 1 == len(bufs[1]) // 4       # and the longest one ends it

    down = (0, 0, -1)
    rays, hand, bounds, leaves = [], [], [], []
    for c, (kind, n) in enumerate(cells):
        y = GALLERY_CELL * c + 0.25
        first = len(rays)
        if kind == "row":
            for p in range(n):
                for any_hit in (False, True):
                    hand.append((len(rays), any_hit, (ids[c][p], 2.0), None))
                rays.append(ray((2 * p + 0.25, y, 1), down))
            xy = (2 * ((n - 2) // 2) + 1.5, y) if n > 1 else (0.75, y + 0.5)
            for any_hit in (False, True):
                hand.append((len(rays), any_hit, (-1, 100.0), None))
            rays.append(ray((*xy, 1), down))
        else:
            at = [(ids[c][k], 2.0 + (n - 1 - k) / 4) for k in range(n)]   # (id, t) per list position
            for tmax, eligible in [(100.0, 0)] + [(2.0 + j / 4 + 0.125, n - 1 - j) for j in range(n)]:
                i = len(rays)
                hand.append((i, False, at[n - 1], None))
                hand.append((i, True, at[eligible], set(at[eligible:])))
                bounds.append((i, False, GALLERY_LEVELS, 2, n, 1))
                rays.append(ray((0.25, y, 1), down, tmax=tmax))
        leaves.append((kind, n, refs[c], list(range(first, len(rays)))))
    return dict(bufs=bufs, rays=np.stack(rays), hand=hand, bounds=bounds, leaves=leaves)


def scene_comb(depth):
    """A comb of `depth` inner nodes for a stack-depth test (reference STACK_SIZE 64,
    kepler_dynamic_fetch.cu:47). Inner node k (k < depth-1) has child 0 = inner
    node k+1 (its box entered at t = k + 1.5) and child 1 = leaf k (entered at
    t = k + 2), so a ray down -z through (0.25, 0.25) goes near and pushes one
    leaf per level: `depth` pushes before the first pop. Leaf k holds triangle k
    in the plane z = -(k+1) (t = k + 2); the last inner node holds leaves
    depth-1 and depth. Closest hit: triangle 0 at t = 2 (hand answer).
    Returns (buffers, ray, (id, t))."""
    b = Compact2Builder()
    inner = [b.reserve_inner() for _ in range(depth)]
    bottom = -(depth + 2.0)

    def tri_leaf(k):
        z = -(k + 1.0)
        return b.leaf([(k, (0, 0, z), (1, 0, z), (0, 1, z))])

    def leaf_box(k):
        return ((0, 0, -(k + 1.0)), (1, 1, -(k + 1.0)))

    for k in range(depth - 1, -1, -1):
        if k == depth - 1:
            b.set_inner(inner[k], leaf_box(k), leaf_box(k + 1), tri_leaf(k), tri_leaf(k + 1))
        else:
            child_box = ((0, 0, bottom), (1, 1, -(k + 1.0) + 0.5))
            b.set_inner(inner[k], child_box, leaf_box(k), inner[k + 1] * 4, tri_leaf(k))
    return b.buffers(), ray((0.25, 0.25, 1), (0, 0, -1), tmax=1000.0), (0, 2.0)


def scene_complete(depth, hit_last=False):
    """A complete binary tree of `depth` inner levels whose nested boxes
    ([0,2]^2 x [0, 1 - level/64], so a level's boxes are larger than the next
    level's) all hold (0.5, 0.5), one triangle per leaf (2^depth leaves): the
    4-wide derivation collapses it level pair by level pair into a complete 4-ary
    tree of depth/2 levels, every child of every node hit by a ray down -z through
    (0.5, 0.5). Each leaf's
    triangle is a small one in the corner (missed), except, with hit_last, the
    last leaf's: a leg-2 triangle in the plane z = 0.5 (t = 1.5 from z = 2).
    ADVICE r3: a frontier that expands many entries per step must still fit such a
    ray's list in the stack. Returns (buffers, ray, (id, t))."""
    b = Compact2Builder()
    leaves = 1 << depth
    counter = [0]

    def leaf():
        k = counter[0]
        counter[0] += 1
        z = 0.25 + 0.5 * (k % 2)
        if hit_last and k == leaves - 1:
            return b.leaf([(k, (0, 0, 0.5), (2, 0, 0.5), (0, 2, 0.5))])
        return b.leaf([(k, (0, 0, z), (0.125, 0, z), (0, 0.125, z))])

    def build(level):
        idx = b.reserve_inner()
        c = [build(level + 1) if level + 1 < depth else leaf() for _ in range(2)]
        box = ((0, 0, 0), (2, 2, 1.0 - (level + 1) / 64.0))
        return b.set_inner(idx, box, box, c[0], c[1])

    build(0)
    expect = (leaves - 1, 1.5) if hit_last else (-1, 1000.0)
    return b.buffers(), ray((0.5, 0.5, 2), (0, 0, -1), tmax=1000.0), expect
