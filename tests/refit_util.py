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
    with np.errstate(divide="ignore", invalid="ignore"):
        rd = np.where(d != 0, F(1) / d, F(0)).astype(np.float32)
    inv = [[(inv[r][c] * rd) * F(4) for c in range(4)] for r in range(4)]
    rows = np.stack([inv[2][0], inv[2][1], inv[2][2], -inv[2][3]] + inv[0] + inv[1], 1).astype(np.float32)
    rows[rows[:, 0] == 0, 0] = 0.0   # -0.0 in Z.x would read as a terminator
    return rows


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


def np_refit(nodes, woop, tri_index, vertices, triangles, skip=()):
    """(nodes, woop) refitted: every leaf's rows from triIndex -> triangle -> vertices, leaf
    boxes the min/max of whole triangles, inner boxes unions bottom-up; an empty leaf keeps
    its box and adds nothing above it. skip: first slots of triangles to leave out (the
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
                    p = v[tris.reshape(-1)]
                    box = (p.min(0), p.max(0))
            if box is None:
                continue
            nf[n, box_words(side)] = np.stack([box[0], box[1]], 1).reshape(-1)
            whole = box if whole is None else (np.minimum(whole[0], box[0]), np.maximum(whole[1], box[1]))
        return whole

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    subtree(0)
    return nodes.reshape(-1), woop.reshape(-1)


def same_nodes(a, b):
    """Boxes as float values (-0.0 == 0.0), words 12-15 as bits."""
    a = np.ascontiguousarray(a).view(np.int32).reshape(-1, 16)
    b = np.ascontiguousarray(b).view(np.int32).reshape(-1, 16)
    return a.shape == b.shape and np.array_equal(a[:, 12:], b[:, 12:]) and \
        np.array_equal(a[:, :12].view(np.float32), b[:, :12].view(np.float32))


def host_refit(bufs, vertices, triangles):
    """mrth_bvh_refit on a copy of bufs -> (nodes, woop, triIndex)."""
    bvh = mrt.Bvh.from_buffers(*bufs)
    bvh.refit(vertices, triangles)
    return bvh.buffers()
