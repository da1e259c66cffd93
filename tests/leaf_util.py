"""Shared by tests/test_leaf_sizes.py, tests/test_gpu_leaf_sizes.py and the batches of
tests/test_gpu_variants.py: trees whose leaves hold more than 8 triangles. The host SBVH builder
makes them when min_leaf is raised (a node of at most min_leaf references becomes a leaf), and
kat.leaf_gallery() is the hand-made one. The leaf sizes are counted here from the node refs and
the terminators alone."""
import functools

import numpy as np

import kat
import lbvh_util as L
import mrt
import refit_util as R

ALPHA = 1e-5
MAX_LEAF = 64

# name -> (scene, param, min_leaf)
NATURAL = {
    "random1500-min17": ("random", 1500, 17),
    "random1500-min33": ("random", 1500, 33),
    "hairball3-min33": ("hairball", 3, 33),
    "random9000-min17": ("random", 9000, 17),
}
NAMES = ["gallery"] + list(NATURAL)
MAX_RECORDS = 1630   # no tree here is larger


@functools.lru_cache(maxsize=None)
def built(name):
    """(vertices, triangles, (nodes, woop, triIndex)) of a natural big-leaf tree; cached, read-only."""
    scene_name, param, min_leaf = NATURAL[name]
    v, t = L.scene_arrays(scene_name, param)
    bufs = mrt.Bvh.build(mrt.Scene.synthetic(scene_name, param, 1), max_leaf=MAX_LEAF, min_leaf=min_leaf,
                         split_alpha=ALPHA).buffers()
    for a in bufs:
        a.setflags(write=False)
    assert len(bufs[0]) // 16 <= MAX_RECORDS
    return v, t, bufs


@functools.lru_cache(maxsize=None)
def gallery():
    g = kat.leaf_gallery()
    for a in g["bufs"] + (g["rays"],):
        a.setflags(write=False)
    return g


def buffers(name):
    return gallery()["bufs"] if name == "gallery" else built(name)[2]


def leaf_sizes(nodes, woop):
    """{leaf ref: triangles} of every leaf ref in the nodes: the slots from ~ref in steps of three
    whose first word is not the terminator's."""
    refs = np.ascontiguousarray(nodes).view(np.int32).reshape(-1, 16)[:, 12:14]
    w0 = np.ascontiguousarray(woop).view(np.int32).reshape(-1, 4)[:, 0]
    out = {}
    for ref in refs[refs < 0]:
        s = ~int(ref)
        n = 0
        while w0[s + 3 * n] != R.TERMINATOR:
            n += 1
        out[int(ref)] = n
    return out


def histogram(sizes):
    """{leaf size: leaves} from leaf_sizes' dict."""
    values, counts = np.unique(list(sizes.values()), return_counts=True)
    return {int(v): int(c) for v, c in zip(values, counts)}


@functools.lru_cache(maxsize=None)
def true_sizes(name):
    """{leaf ref: triangles}: the gallery's by construction, a natural tree's by leaf_sizes."""
    if name == "gallery":
        return {int(ref): n for _, n, ref, _ in gallery()["leaves"]}
    _, _, bufs = built(name)
    return leaf_sizes(bufs[0], bufs[1])


def check_histogram(name, h):
    """What each natural tree must hold for the tests on it to cover what they say they cover: a
    builder or a scene that drifts fails here."""
    long_ones = sum(c for n, c in h.items() if n >= 16)
    if name == "random1500-min17":
        assert all(h.get(n, 0) >= 1 for n in (5, 8, 9, 12, 13, 15, 16, 17)) and max(h) == 17, h
    elif name == "random1500-min33":
        assert long_ones >= 60 and max(h) == 33, h
    elif name == "hairball3-min33":
        assert long_ones >= 40 and sum(c for n, c in h.items() if 9 <= n <= 15) >= 10, h
    elif name == "random9000-min17":
        assert all(h.get(n, 0) >= 1 for n in (4, 5, 8, 9, 12, 13, 15, 16, 17)), h
    else:
        raise KeyError(name)


def incoherent_rays(vertices, triangles, n, seed):
    """n rays from random points of the bounding box grown by a quarter towards random points of
    random triangles (the thin tubes of a hairball are hit by little else), the target at t = 1,
    with random tmin in [0, 0.3] and tmax in [0.4, 1.5]: some end before their target."""
    v = np.asarray(vertices, np.float64)
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0), v.max(0)
    grow = 0.25 * (hi - lo).max()
    a = rng.uniform(lo - grow, hi + grow, (n, 3))
    corners = v[np.asarray(triangles)[rng.integers(0, len(triangles), n)]]
    bary = rng.dirichlet((1.0, 1.0, 1.0), n)
    b = (corners * bary[:, :, None]).sum(1)
    rays = np.concatenate([a, rng.uniform(0.0, 0.3, (n, 1)), b - a, rng.uniform(0.4, 1.5, (n, 1))], 1)
    return np.ascontiguousarray(rays, np.float32)


@functools.lru_cache(maxsize=None)
def rays_for(name):
    """The rays a tree is traced with; read-only. The gallery: its own. A natural tree: the
    64 x 48 frame of refit_util.frame_rays and 1000 incoherent rays."""
    if name == "gallery":
        return gallery()["rays"]
    v, t, _ = built(name)
    rays = np.concatenate([R.frame_rays(v), incoherent_rays(v, t, 1000, 17)])
    rays.setflags(write=False)
    return rays
