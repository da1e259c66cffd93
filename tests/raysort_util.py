"""Shared by tests/test_raysort.py and tests/test_gpu_raysort.py: a numpy restatement of the ray
sort's key and order, written from the definition in include/mrt.h (mrt_ray_sort) and
csrc/raysort_common.hpp, the random and the edge batches both files sort, and the comparison of two
sorts' outputs.

The restatement is float32 numpy, one ufunc per operation: IEEE arithmetic with no contraction,
correctly rounded division and square root, denormals kept. The key is put together bit by bit
from its definition (bit 6 i + c of the key is bit i of component c) and ordered as a Python
integer, which shares nothing with the library's interleave and 64-bit words."""
import functools

import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
ORIGIN_CAP, DIRECTION_CAP = 1 << 24, 1 << 21


def np_box(rays, mode):
    """(lo.xyz, hi.xyz): from +-FLT_MAX, every origin and (mode 0) end point o + d * tmax; fmin /
    fmax, so a NaN never enters."""
    rays = np.asarray(rays, F).reshape(-1, 8)
    pts = [rays[:, 0:3]]
    if mode == 0:
        with np.errstate(all="ignore"):
            step = rays[:, 4:7] * rays[:, 7:8]
            pts.append(rays[:, 0:3] + step)
    p = np.concatenate(pts)
    lo = np.fmin.reduce(np.concatenate([np.full((1, 3), FLT_MAX, F), p]))
    hi = np.fmax.reduce(np.concatenate([np.full((1, 3), -FLT_MAX, F), p]))
    return np.concatenate([lo, hi]).astype(F)


def np_conv(x, cap):
    """NaN -> 0, x <= 0 -> 0, x >= cap -> cap, else truncation."""
    out = np.zeros(x.shape, np.uint32)
    with np.errstate(invalid="ignore"):
        pos = x > 0
        big = pos & (x >= F(cap))
    mid = pos & ~big
    out[big] = cap
    out[mid] = np.trunc(x[mid]).astype(np.uint32)
    return out


def np_components(rays, box):
    """uint32 [n, 6]: q.x, q.y, q.z, r.x, r.y, r.z."""
    rays = np.asarray(rays, F).reshape(-1, 8)
    lo, hi = box[0:3], box[3:6]
    o, d = rays[:, 0:3], rays[:, 4:7]
    with np.errstate(all="ignore"):
        a = (o - lo) / (hi - lo)
        sq = d * d
        length = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
        b = (d / length[:, None] + F(1.0)) * F(0.5)
        q = np_conv(a * F(256.0) * F(65536.0), ORIGIN_CAP)
        r = np_conv(b * F(32.0) * F(65536.0), DIRECTION_CAP)
    assert a.dtype == F and b.dtype == F and length.dtype == F
    return np.concatenate([q, r], axis=1)


def np_keys(comp):
    """uint32 [n, 6]: hash[w] holds key bits 32 w .. 32 w + 31."""
    n = len(comp)
    bits = np.zeros((n, 192), np.uint64)
    for i in range(32):
        for c in range(6):
            bits[:, 6 * i + c] = (comp[:, c] >> np.uint32(i)) & np.uint32(1)
    hash_ = np.zeros((n, 6), np.uint64)
    for w in range(6):
        for k in range(32):
            hash_[:, w] |= bits[:, 32 * w + k] << np.uint64(k)
    return hash_.astype(np.uint32)


def key_ints(keys):
    """The keys as Python integers."""
    return [sum(int(k[w]) << (32 * w) for w in range(6)) for k in np.asarray(keys, np.uint32).reshape(-1, 6)]


def np_order(keys, drop_levels):
    """Ascending by key >> (6 * drop_levels), ties by ascending input slot."""
    ints = key_ints(keys)
    return np.array(sorted(range(len(ints)), key=lambda i: (ints[i] >> (6 * drop_levels), i)), np.int32)


def np_ray_sort(rays, slot_to_id=None, drop_levels=0, box=0):
    """The whole sort as mrt.host.ray_sort returns it, and the permutation."""
    rays = np.ascontiguousarray(rays, F).reshape(-1, 8)
    n = len(rays)
    bx = np_box(rays, box)
    keys = np_keys(np_components(rays, bx))
    perm = np_order(keys, drop_levels)
    ids = perm if slot_to_id is None else np.asarray(slot_to_id, np.int32)[perm]
    id_to_slot = np.full(n, -1, np.int32)
    ok = (ids >= 0) & (ids < n)
    id_to_slot[ids[ok]] = np.nonzero(ok)[0].astype(np.int32)
    return {"rays": rays[perm], "id_to_slot": id_to_slot, "slot_to_id": ids.astype(np.int32), "keys": keys,
            "box": bx, "perm": perm}


def components_of(keys):
    """De-interleaves keys uint32 [n, 6] into the six components, uint32 [n, 6]."""
    comp = np.zeros((len(keys), 6), np.uint64)
    for j, v in enumerate(key_ints(keys)):
        for c in range(6):
            comp[j, c] = sum(((v >> (6 * i + c)) & 1) << i for i in range(32))
    return comp.astype(np.uint32)


def assert_same_sort(got, want, what=""):
    """Keys as bits, the box as float values (the sign of a zero is free), rays as uint32, both maps."""
    assert np.array_equal(np.asarray(got["keys"]).view(np.uint32).reshape(-1, 6), want["keys"]), f"{what}: keys"
    assert np.array_equal(np.asarray(got["box"], F), want["box"]), f"{what}: box {got['box']} != {want['box']}"
    assert np.array_equal(np.ascontiguousarray(got["rays"], F).view(np.uint32),
                          np.ascontiguousarray(want["rays"], F).view(np.uint32)), f"{what}: rays"
    assert np.array_equal(got["slot_to_id"], want["slot_to_id"]), f"{what}: slot_to_id"
    assert np.array_equal(got["id_to_slot"], want["id_to_slot"]), f"{what}: id_to_slot"


# ---- batches --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_rays(n, seed=7):
    """n random rays with mixed tmax, every seventh -1 (a degenerate ray of a missed primary). Read-only."""
    rng = np.random.default_rng(seed + n)
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = rng.uniform(-10, 10, (n, 3))
    d = rng.normal(size=(n, 3))
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 7] = rng.choice(np.array([0.5, 5.0, 1e3, 1e18], F), n)
    rays[::7, 7] = -1.0
    rays[1::5, 4:7] *= F(3.5)      # not every direction is a unit vector
    rays.setflags(write=False)
    return rays


def shuffled_ids(n, seed=11):
    return np.random.default_rng(seed + n).permutation(n).astype(np.int32)


def _ray(o, d, tmax=1.0):
    return [o[0], o[1], o[2], 0.0, d[0], d[1], d[2], tmax]


EDGE_LABELS = ["plain", "NaN origin.x", "+inf origin.y", "-inf origin.z", "zero direction", "NaN direction.y",
               "1e-30 direction", "inf tmax", "denormal squares", "denormal origin", "plain far", "NaN tmax",
               "zero direction, inf tmax"]


@functools.lru_cache(maxsize=None)
def edge_batches():
    """name -> rays float32 [n, 8], read-only. `edges` holds one ray per EDGE_LABELS entry among
    ordinary ones; `edges_finite` the same without the infinite origins and the infinite tmax (which
    make the box infinite and send every origin component of the batch to 0); `identical` 64 copies
    of one ray (hi == lo on every axis); `flat` a batch whose origins share one y."""
    nan, inf = np.nan, np.inf
    edges = [
        _ray((1.0, 2.0, 3.0), (0.0, 0.6, -0.8)),
        _ray((nan, 2.0, 3.0), (1.0, 0.0, 0.0)),
        _ray((1.0, inf, 3.0), (0.0, 1.0, 0.0)),
        _ray((1.0, 2.0, -inf), (0.0, 0.0, 1.0)),
        _ray((-1.0, 0.5, 2.0), (0.0, 0.0, 0.0)),
        _ray((0.5, -2.0, 1.0), (1.0, nan, 0.0)),
        _ray((2.0, 2.0, 2.0), (1e-30, 0.0, 0.0)),
        _ray((0.0, 1.0, 0.0), (0.0, 0.0, -1.0), inf),
        _ray((3.0, -1.0, 0.25), (1e-20, 1e-20, 0.0)),
        _ray((1e-40, -1e-41, 1e-39), (0.3, 0.4, 0.5)),
        _ray((-4.0, 5.0, -6.0), (-0.6, 0.0, 0.8), 7.5),
        _ray((0.25, 0.75, -0.5), (0.0, 1.0, 0.0), nan),
        _ray((0.5, 0.5, 0.5), (0.0, 0.0, 0.0), inf),
    ]
    assert len(edges) == len(EDGE_LABELS)
    edges = np.array(edges, F)
    finite = np.array([r for k, r in enumerate(edges) if k not in (2, 3, 7, 12)], F)
    filler = random_rays(51, seed=3)
    out = {
        "edges": np.concatenate([edges, filler]),
        "edges_finite": np.concatenate([finite, filler]),
        "identical": np.tile(np.array(_ray((1.5, -2.5, 3.5), (0.6, 0.0, -0.8), 2.0), F), (64, 1)),
        "flat": random_rays(65, seed=5).copy(),
    }
    out["flat"][:, 1] = F(0.75)
    out["flat"][:, 5] = F(0.0)      # and no end point leaves the plane
    for a in out.values():
        a.setflags(write=False)
    return out
