"""Shared by tests/test_refit.py and tests/test_gpu_refit.py: the small scenes, a smooth
vertex displacement, and a refit of Compact2 buffers restated in numpy, independent of
the library's C++ (float32 operations in the reference's order: numpy rounds every
float32 operation once, never contracts, and divides correctly rounded)."""
import functools

import numpy as np

import mrt

TERMINATOR = np.int32(-2147483648)   # x bits 0x80000000
F = np.float32

# (scene, param): 183-730 inner nodes, so no multiple of a workgroup, several one-node levels
SCENES = [("random", 1500), ("sphere", 12), ("hairball", 3)]


@functools.lru_cache(maxsize=None)
def built(name, param, split_alpha):
    """(vertices, triangles, (nodes, woop, triIndex), stats) of a synthetic scene; cached, read-only."""
    scene = mrt.Scene.synthetic(name, param, 1)
    v, t, _ = scene.arrays()
    bvh = mrt.Bvh.build(scene, split_alpha=split_alpha)
    bufs = bvh.buffers()
    for a in (v, t) + tuple(bufs):
        a.setflags(write=False)
    return v, t, bufs, bvh.stats()


def displaced(v):
    """A smooth displacement of about 10 % of the scene's size."""
    v = np.asarray(v, np.float32)
    lo, hi = v.min(0), v.max(0)
    size = float((hi - lo).max())
    u = (v - lo) / max(size, 1e-20)
    d = np.stack([np.sin(6.0 * u[:, 1] + 1.0), np.cos(5.0 * u[:, 2] + 0.5), np.sin(4.0 * u[:, 0] + 2.0)], 1)
    return (v + F(0.1 * size) * d).astype(np.float32)


def frame_rays(vertices, w=64, h=48):
    """A w x h primary frame from a camera looking at the middle vertex from a quarter of
    the scene's size away (the synthetic scenes' own cameras see little of a three-tube
    hairball, whose tubes are thinner than a pixel from outside its box)."""
    v = np.asarray(vertices, np.float32)
    size = float((v.max(0) - v.min(0)).max())
    back = np.array([0.3, 0.2, 1.0]) / np.linalg.norm([0.3, 0.2, 1.0])
    cam = mrt.host.Camera(tuple(v[len(v) // 2] + 0.25 * size * back), tuple(-back), (0.0, 1.0, 0.0), 50.0,
                          1e-3 * size, 100.0 * size)
    return mrt.primary_rays(cam, w, h)[0]


# ---- the Woop transform in numpy ----------------------------------------------------
def _det3(s):
    return (s[0][0] * s[1][1] * s[2][2] - s[0][0] * s[1][2] * s[2][1] + s[1][0] * s[2][1] * s[0][2]
            - s[1][0] * s[2][2] * s[0][1] + s[2][0] * s[0][1] * s[1][2] - s[2][0] * s[0][2] * s[1][1])


@np.errstate(all="ignore")   # rows that overflow, underflow or are NaN are results here, not accidents
def np_woopify(v0, v1, v2):
    """Rows Z, U, V as float32 [n, 12] (guard included) of triangles v0, v1, v2 float32 [n, 3]:
    the cofactor inverse of [v0-v2, v1-v2, cross, v2] with the reference's quirk (d sums
    4 * det, the result is r * rcp(d) * 4)."""
    v0, v1, v2 = (np.asarray(x, np.float32).reshape(-1, 3) for x in (v0, v1, v2))
    n = len(v0)
    e0, e1 = v0 - v2, v1 - v2
    cr = np.stack([e0[:, 1] * e1[:, 2] - e0[:, 2] * e1[:, 1], e0[:, 2] * e1[:, 0] - e0[:, 0] * e1[:, 2],
                   e0[:, 0] * e1[:, 1] - e0[:, 1] * e1[:, 0]], 1)
    zero, one = np.zeros(n, np.float32), np.ones(n, np.float32)
    cols = [list(e0.T) + [zero], list(e1.T) + [zero], list(cr.T) + [zero], list(v2.T) + [one]]
    a = lambda r, c: cols[c][r]   # noqa: E731
    inv = [[None] * 4 for _ in range(4)]   # inv[r][c]
    d = np.zeros(n, np.float32)
    si = F(1)
    for i in range(4):
        sj = si
        for j in range(4):
            sub = [[a(k if k < j else k + 1, l if l < i else l + 1) for l in range(3)] for k in range(3)]
            dd = _det3(sub) * sj
            inv[i][j] = dd
            d = d + dd * a(j, i)
            sj = -sj
        si = -si
    rd = np.where(d != 0, F(1) / d, F(0)).astype(np.float32)
    inv = [[(inv[r][c] * rd) * F(4) for c in range(4)] for r in range(4)]
    rows = np.stack([inv[2][0], inv[2][1], inv[2][2], -inv[2][3]] + inv[0] + inv[1], 1).astype(np.float32)
    rows[rows[:, 0] == 0, 0] = 0.0   # -0.0 in Z.x would read as a terminator
    return rows


# ---- FW::min / FW::max --------------------------------------------------------------------
def fw_min(a, b):
    """(a < b) ? a : b elementwise: a NaN in a is dropped, a NaN in b is kept."""
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(a) < np.asarray(b), a, b).astype(np.float32)


def fw_max(a, b):
    """(a > b) ? a : b elementwise."""
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(a) > np.asarray(b), a, b).astype(np.float32)


def box_min(a, b):
    """woop_common.hpp's box_min: (a < b) ? a : b with a NaN b dropped too, so no NaN enters a box."""
    with np.errstate(invalid="ignore"):
        return np.where((np.asarray(a) < np.asarray(b)) | np.isnan(b), a, b).astype(np.float32)


def box_max(a, b):
    with np.errstate(invalid="ignore"):
        return np.where((np.asarray(a) > np.asarray(b)) | np.isnan(b), a, b).astype(np.float32)


FLT_MAX = np.finfo(np.float32).max


def fold_box(points):
    """(lo, hi) of float32 [k, 3] points grown one by one, in order, onto the FLT_MAX-empty box."""
    lo, hi = np.full(3, FLT_MAX, np.float32), np.full(3, -FLT_MAX, np.float32)
    for p in points:
        lo, hi = box_min(lo, p), box_max(hi, p)
    return lo, hi


# ---- Compact2 accessors -----------------------------------------------------------------
def box_words(child):
    """The six words (lo.x, hi.x, lo.y, hi.y, lo.z, hi.z) of child 0 / 1 in a 16-word record."""
    return [4 * child, 4 * child + 1, 4 * child + 2, 4 * child + 3, 8 + 2 * child, 9 + 2 * child]


def boxes(nodes):
    """float32 [n, 2, 6] (lo.x, hi.x, lo.y, hi.y, lo.z, hi.z) per child."""
    f = np.ascontiguousarray(nodes).view(np.float32).reshape(-1, 16)
    return np.stack([f[:, box_words(0)], f[:, box_words(1)]], 1)


def leaf_slots(woop, ref):
    """First slots of the triangles of leaf ref (< 0): steps of three up to the terminator."""
    w = np.ascontiguousarray(woop).view(np.int32).reshape(-1, 4)
    s, out = ~int(ref), []
    while w[s, 0] != TERMINATOR:
        out.append(s)
        s += 3
    return out


def leaf_walk(nodes, woop):
    """(z_slots, terminators) as sorted int64 arrays: every leaf ref in the nodes walked from
    its first slot in steps of three up to the slot whose first word is 0x80000000. Only Z
    rows are looked at, as the library and the kernels do: a U or V row of a zero-area
    triangle is (r * 0) * 4, which may be -0.0 in its first word or in all four."""
    refs = np.ascontiguousarray(nodes).view(np.int32).reshape(-1, 16)[:, 12:14]
    w0 = np.ascontiguousarray(woop).view(np.int32).reshape(-1, 4)[:, 0]
    z, term = [], []
    for ref in refs[refs < 0]:
        s = ~int(ref)
        while w0[s] != TERMINATOR:
            z.append(s)
            s += 3
        term.append(s)
    return np.sort(np.asarray(z, np.int64)), np.sort(np.asarray(term, np.int64))


def np_refit(nodes, woop, tri_index, vertices, triangles, skip=()):
    """(nodes, woop) refitted: every leaf's rows from triIndex -> triangle -> vertices. Boxes
    are folded with woop_common.hpp's box_min / box_max ((a < b) ? a : b, a NaN dropped) in
    the library's order: a leaf's triangles in slot order, vertices 0, 1, 2 onto the FLT_MAX-
    empty box; an inner box is child 0's union child 1's, bottom-up. For finite vertices that
    is the min / max (a zero's sign is the order's); a NaN coordinate enters no box. An empty
    leaf keeps its box and adds nothing above it. skip: first slots of triangles to leave out (the
    device refit's treatment of an out-of-range reference: old rows, not in the box)."""
    nodes = np.array(nodes, np.int32).reshape(-1, 16)
    woop = np.array(woop, np.int32).reshape(-1, 4)
    nf = nodes.view(np.float32)
    v = np.asarray(vertices, np.float32)
    t = np.asarray(triangles, np.int32)

    def subtree(n):
        """Refits node n; returns the box of everything below it, or None."""
        whole = None
        for side in range(2):
            ref = int(nodes[n, 12 + side])
            if ref >= 0:
                box = subtree(ref // 4)
            else:
                slots = [s for s in leaf_slots(woop, ref) if s not in skip]
                box = None
                if slots:
                    tris = t[np.asarray(tri_index)[slots]]
                    rows = np_woopify(v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]])
                    for s, r in zip(slots, rows):
                        woop[s:s + 3] = r.view(np.int32).reshape(3, 4)
                    box = fold_box(v[tris.reshape(-1)])
            if box is None:
                continue
            nf[n, box_words(side)] = np.stack([box[0], box[1]], 1).reshape(-1)
            whole = box if whole is None else (box_min(whole[0], box[0]), box_max(whole[1], box[1]))
        return whole

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    subtree(0)
    return nodes.reshape(-1), woop.reshape(-1)


def same_bits_or_nan(a, b):
    """Every 32-bit word equal, or a NaN as float32 on both sides (the payload and sign of a
    NaN an operation makes differ between x86 and gfx950: 0xFFC00000 and 0x7FC00000)."""
    a = np.ascontiguousarray(a).view(np.int32)
    b = np.ascontiguousarray(b).view(np.int32)
    if a.shape != b.shape:
        return False
    fa, fb = a.view(np.float32), b.view(np.float32)
    return bool(((a == b) | (np.isnan(fa) & np.isnan(fb))).all())


def same_nodes(a, b):
    """Boxes as float values (-0.0 == 0.0; a NaN equals a NaN), words 12-15 as bits."""
    a = np.ascontiguousarray(a).view(np.int32).reshape(-1, 16)
    b = np.ascontiguousarray(b).view(np.int32).reshape(-1, 16)
    if a.shape != b.shape or not np.array_equal(a[:, 12:], b[:, 12:]):
        return False
    fa, fb = a[:, :12].view(np.float32), b[:, :12].view(np.float32)
    return bool(((fa == fb) | (np.isnan(fa) & np.isnan(fb))).all())


def check_wide(wide_before, wide_after, nodes_before, nodes_after):
    """The exact 4-wide array after a refit: refs and absent children as before, every present
    child's planes the refitted Compact2 box the collapse of the ORIGINAL nodes mapped it to."""
    from mrt.tracer import refit_plan
    _, _, src = refit_plan(nodes_before)
    before, after = wide_before.reshape(-1, 32), wide_after.reshape(-1, 32)
    src = src.reshape(-1, 4)
    assert len(src) == len(after)
    assert np.array_equal(after[:, 24:], before[:, 24:])
    rec = np.ascontiguousarray(nodes_after).view(np.uint32).reshape(-1, 16)
    for c in range(4):
        base = [(2 * k + (c >> 1)) * 4 + (c & 1) * 2 + e for k in range(3) for e in (0, 1)]
        have = src[:, c] >= 0
        node, side = src[have, c] >> 1, src[have, c] & 1
        words = np.where(side[:, None] == 0, box_words(0), box_words(1))
        assert np.array_equal(after[have][:, base], rec[node[:, None], words])
        assert np.array_equal(after[~have][:, base], before[~have][:, base])   # NaN planes untouched


def host_refit(bufs, vertices, triangles):
    """mrth_bvh_refit on a copy of bufs -> (nodes, woop, triIndex)."""
    bvh = mrt.Bvh.from_buffers(*bufs)
    bvh.refit(vertices, triangles)
    return bvh.buffers()
