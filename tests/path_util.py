"""Shared by tests/test_path.py and tests/test_gpu_path.py: an independent model of a path frame's
vertex step, accumulation and resolve, the tables both are checked on, and a whole-frame driver
that takes the trace as a callback.

The model restates the contract of mrt_path_extend / _accumulate / _resolve from the text of
include/mrt.h, not from csrc/path_common.hpp. It works on numpy float32 arrays over all slots at
once, one IEEE operation at a time in the documented order, in uint32 for the hash; the pieces the
contract borrows from mrt_raygen_shadow and mrt_reconstruct_lit (the shadow ray of an origin, the
cosine k, fromABGR / toABGR) are light_util's, themselves written from the reference's kernel text.
`Model` has mrt.host's three signatures, so the frame driver runs either.
"""
import functools

import numpy as np

import frame_util as U
import light_util as L

F = np.float32
U32 = np.uint32
GOLDEN = 0x9E3779B9
SIN = [F(x) for x in (1.5707963267948966, -0.6459640975062462, 0.07969262624616703, -0.004681754135318687,
                      0.00016044118478735975)]
COS = [F(x) for x in (-1.2337005501361697, 0.253669507901048, -0.020863480763352957, 0.0009192602748394263,
                      -2.5202042373060596e-05)]


# ---- the model ------------------------------------------------------------------------------------
def hash_words(seed, vertex, keys):
    """uint32 [n, 3] after two mixes of (seed + vertex * 0x9e3779b9 + key, g, g), and [n, 3] after a third."""
    a = ((np.asarray(keys, np.uint64) + np.uint64(seed & 0xFFFFFFFF) + np.uint64((vertex * GOLDEN) & 0xFFFFFFFF))
         & np.uint64(0xFFFFFFFF)).astype(U32)
    g = np.full_like(a, GOLDEN)
    two = L.jenkins_mix(*L.jenkins_mix(a, g, g))
    three = L.jenkins_mix(*two)
    return np.stack(two, axis=1), np.stack(three, axis=1)


@functools.lru_cache(maxsize=None)
def halton23(num):
    """The Halton (2, 3) points of indices < num as mrt_raygen_ao computes them: float32 [num, 2]."""
    out = np.zeros((num, 2), F)
    for s in range(num):
        x, add, k = F(0.0), F(1.0), s + 1
        while k:
            add = add * F(0.5)
            if k & 1:
                x = x + add
            k >>= 1
        y, add, k = F(0.0), F(1.0), s + 1
        while k:
            add = add * (F(1.0) / F(3.0))
            y = y + F(k % 3) * add
            k //= 3
        out[s] = (x, y)
    out.setflags(write=False)
    return out


def sincos_turn(u):
    """(cos, sin) of 2 pi u for float32 u in [0, 1), by the contract's reduction and polynomials."""
    u = np.asarray(u, F)
    v = u * F(4.0)
    q = v.astype(np.int32)
    f = v - q.astype(F)
    up = f > F(0.5)
    f = np.where(up, f - F(1.0), f)
    q = np.where(up, q + 1, q)
    g = f * f
    s = f * (SIN[0] + g * (SIN[1] + g * (SIN[2] + g * (SIN[3] + g * SIN[4]))))
    c = F(1.0) + g * (COS[0] + g * (COS[1] + g * (COS[2] + g * (COS[3] + g * COS[4]))))
    k = q & 3
    return np.choose(k, [c, -s, -c, s]).astype(F), np.choose(k, [s, c, -s, -c]).astype(F)


def fw_max(a, b):
    return np.where(a > b, a, b)


def normalized(v):
    return v * (F(1.0) * L.rcp(np.sqrt(L.dot3(v, v))))[:, None]


def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def wrap(p):
    return np.where(p >= F(1.0), p - F(1.0), p)


def bounce_dirs(nf, s, shift, num_samples):
    h = halton23(num_samples)[s]
    u1, u2 = wrap(h[:, 0] + shift[:, 0]), wrap(h[:, 1] + shift[:, 1])
    c, sn = sincos_turn(u2)
    r = np.sqrt(u1)
    x, y = r * c, r * sn
    z = np.sqrt(fw_max(F(1.0) - x * x - y * y, F(0.0)))
    na = np.abs(nf)
    nm = fw_max(fw_max(na[:, 0], na[:, 1]), na[:, 2])
    zero = np.zeros(len(nf), F)
    perp = np.stack([nf[:, 1], -nf[:, 0], zero], axis=1)
    by_x = np.stack([-nf[:, 2], zero, nf[:, 0]], axis=1)
    by_z = np.stack([zero, nf[:, 2], -nf[:, 1]], axis=1)
    perp = np.where((nm == na[:, 2])[:, None], by_z, np.where((nm == na[:, 0])[:, None], by_x, perp))
    perp = normalized(perp)
    biperp = cross(nf, perp)
    return normalized((perp * x[:, None] + biperp * y[:, None]) + nf * z[:, None])


def shadow_rays_at(origin, ids, offset, s, num_samples, light, radius):
    """mrt_raygen_shadow's ray from `origin` for sample s[j] of num_samples and offset[j]."""
    q = np.concatenate([L.sobol2d(num_samples), L.hammersley(num_samples)[:, None]], axis=1)[s]
    p = wrap(q + offset)
    pos = p * F(2.0) - F(1.0)
    d = (np.asarray(light, F)[None, :] + F(radius) * pos) - origin
    length = np.sqrt(L.dot3(d, d))
    out = np.zeros((len(origin), 8), F)
    out[:, 0:3] = origin
    out[:, 4:7] = d * (F(1.0) * L.rcp(length))[:, None]
    out[:, 7] = np.where(ids == -1, F(-1.0), length)
    return out


class Model:
    """mrt.host.path_extend / path_accumulate / path_resolve, from the contract."""

    @staticmethod
    def path_extend(rays, results, state, radiance, normals, material, vertex, depth, num_samples, seed, light_pos,
                    light_radius, light_color=(1.0, 1.0, 1.0), sky=(0.2, 0.4, 0.8), max_dist=1.0e30, compact=True,
                    num_slots=None):
        S = num_samples
        rays = np.ascontiguousarray(rays, F).reshape(-1, 8)
        results = np.ascontiguousarray(results).view(np.int32).reshape(-1, 4)
        normals, material = np.asarray(normals, F).reshape(-1, 3), np.asarray(material).view(U32).reshape(-1)
        if num_slots is None:
            num_slots = len(rays) * S if vertex == 0 else len(rays)
        n = num_slots
        slots = np.arange(n)
        if vertex == 0:
            at, thr, task, live = slots // S, np.ones((n, 3), F), slots.astype(np.int32), np.ones(n, bool)
        else:
            st = np.ascontiguousarray(state).view(np.int32).reshape(-1, 4)[:n]
            at, thr, task = slots, np.ascontiguousarray(st[:, :3]).view(F), st[:, 3]
            live = (task >= 0) & (task < len(radiance))
        r, res = rays[at], results[at]
        ids = res[:, 0]
        hit = live & (ids >= 0) & (ids < len(material))
        with np.errstate(all="ignore"):
            if vertex >= 1:
                gone = live & ~hit
                radiance[task[gone], :3] += thr[gone] * np.asarray(sky, F)[None, :]
            h = np.flatnonzero(hit)
            r, res, ids, thr, task, key = r[h], res[h], ids[h], thr[h], task[h], (at[h] if vertex == 0 else task[h])
            origin = L.backed_off(r, L.result_t(res))
            nrm = normals[ids]
            nf = np.where((L.dot3(nrm, r[:, 4:7]) > 0)[:, None], -nrm, nrm)
            thr = thr * L.from_abgr(material[ids])[:, :3]
            two, three = hash_words(seed, vertex, key)
            s = task % S
            shadow = shadow_rays_at(origin, ids, two.astype(F) * L.TWO_M32, s, S, light_pos, light_radius)
            to_light = np.asarray(light_pos, F)[None, :] - origin
            c = L.dot3(nf, normalized(to_light))
            k = np.where(c > 0, c, F(0.0)).astype(F)
            pending = thr * np.asarray(light_color, F)[None, :] * k[:, None]
            bounce = None
            if vertex < depth:
                bounce = np.zeros((len(h), 8), F)
                bounce[:, 0:3] = origin
                bounce[:, 4:7] = bounce_dirs(nf, s, three[:, :2].astype(F) * L.TWO_M32, S)
                bounce[:, 7] = F(max_dist)
        dest = np.arange(len(h)) if compact else h
        out = {"shadow": np.zeros((n, 8), F), "pending": np.zeros((n, 4), F),
               "rays": np.zeros((n, 8), F) if vertex < depth else None, "state": np.zeros((n, 4), np.int32)}
        if not compact:
            out["shadow"][:, 7] = -1.0
            out["state"][:, 3] = -1
            if out["rays"] is not None:
                out["rays"][:, 7] = -1.0
        out["shadow"][dest] = shadow
        out["pending"][dest, :3] = pending
        if bounce is not None:
            out["rays"][dest] = bounce
        out["state"][dest, :3] = thr.view(np.int32)
        out["state"][dest, 3] = task
        out["live"] = len(h)
        return out

    @staticmethod
    def path_accumulate(state, pending, shadow_results, radiance, num_slots=None):
        st = np.ascontiguousarray(state).view(np.int32).reshape(-1, 4)
        n = len(st) if num_slots is None else num_slots
        task = st[:n, 3]
        ids = np.ascontiguousarray(shadow_results).view(np.int32).reshape(-1, 4)[:n, 0]
        sel = (task >= 0) & (task < len(radiance)) & (ids == -1)
        with np.errstate(all="ignore"):
            radiance[task[sel], :3] += np.asarray(pending, F).reshape(-1, 4)[:n][sel, :3]
        return radiance

    @staticmethod
    def path_resolve(num_samples, slot_to_id, primary_results, radiance, num_pixels, first_primary=0, num_primary=None,
                     pixels=None, image=None, want_image=False):
        rad = np.asarray(radiance, F).reshape(-1, 4)
        if num_primary is None:
            num_primary = len(rad) // num_samples
        rad = rad[:num_primary * num_samples].reshape(num_primary, num_samples, 4)
        total = np.zeros((num_primary, 3), F)
        with np.errstate(all="ignore"):
            for s in range(num_samples):
                total = total + rad[:, s, :3]
            value = np.concatenate([total * (F(1.0) / F(num_samples)), np.ones((num_primary, 1), F)], axis=1)
        sl = slice(first_primary, first_primary + num_primary)
        miss = np.ascontiguousarray(primary_results).view(np.int32).reshape(-1, 4)[sl, 0] == -1
        value[miss] = np.array([0.2, 0.4, 0.8, 1.0], F)
        pixels = np.zeros(num_pixels, U32) if pixels is None else pixels
        pixels[np.asarray(slot_to_id)[sl]] = L.to_abgr(value)
        if image is None and want_image:
            image = np.zeros((num_pixels, 4), F)
        if image is not None:
            image[np.asarray(slot_to_id)[sl]] = value
            return pixels, image
        return pixels


# ---- equality ---------------------------------------------------------------------------------------
def same_floats(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(U.same_bits_or_nan(a.view(F), b.view(F)).all())


def same_step(got, want, live_only=False):
    """Two path_extend outputs: the live count, and every buffer bit for bit (a NaN equal to a NaN).
    live_only compares the first `live` entries (a device buffer's tail is not written)."""
    if got["live"] != want["live"]:
        return f"live {got['live']} != {want['live']}"
    m = want["live"] if live_only else None
    for name in ("shadow", "pending", "rays", "state"):
        a, b = got[name], want[name]
        if (a is None) != (b is None):
            return f"{name}: one side has none"
        if a is None:
            continue
        if name == "state":   # throughput as floats, the task as an integer
            if not np.array_equal(a[:m, 3], b[:m, 3]):
                return "state: tasks differ"
            a, b = np.ascontiguousarray(a[:m, :3]), np.ascontiguousarray(b[:m, :3])
        if not same_floats(a[:m], b[:m]):
            bad = np.flatnonzero(~U.same_bits_or_nan(a[:m].view(F), b[:m].view(F)).all(axis=1))
            return f"{name}: rows {bad[:8]} differ"
    return ""


# ---- the edge table ---------------------------------------------------------------------------------------
EDGE_SAMPLES = [1, 2, 3, 64, 257]
EDGE_LIGHT = dict(light_pos=(1.5, -2.0, 3.25), light_radius=0.75, light_color=(1.0, 0.5, 0.25), sky=(0.2, 0.4, 0.8),
                  max_dist=100.0)
NUM_TRIS = 64


@functools.lru_cache(maxsize=None)
def edge_tables():
    """(normals float32 [64, 3], material uint32 [64]), read-only. Normals 0..11 are the edges:
    +-z, zero, NaN, +-x, +-y, one NaN component, and the ties |x| == |z|, |x| == |y| == |z|, |y| == |z|
    at which the order of the perpendicular's tests decides; the rest random unit vectors. The
    colours are frame_util's, whose first 36 take every channel through 0, 1, 127, 128, 254, 255."""
    rng = np.random.default_rng(15)
    normals = rng.normal(size=(NUM_TRIS, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(F)
    r2, r3 = 1 / np.sqrt(2), 1 / np.sqrt(3)
    normals[:12] = [(0, 0, 1), (0, 0, -1), (0, 0, 0), (np.nan,) * 3, (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0),
                    (0.6, np.nan, 0.8), (r2, 0, r2), (r3, r3, r3), (0, r2, r2)]
    material, _ = U.colour_tables()
    normals.setflags(write=False)
    return normals, material


EDGE_IDS = [-1, 0, 5, NUM_TRIS - 1, 2, 3, 8, 9, 10, 11, 1, 4, 6, 7]
EDGE_T = [0.0, 1.0, np.inf, np.nan, 1e-39, 1e-4, 2.5]
EDGE_DIRS = [(0.0, 0.0, -1.0), (0.6, 0.0, -0.8), (-0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]


@functools.lru_cache(maxsize=None)
def edge_inputs():
    """392 input rays (rays float32 [n, 8], results int32 [n, 4]), read-only: every t x id x direction
    of the table; from the second half on the origin's y is a denormal, which neither side flushes."""
    rows = []
    for t in EDGE_T:
        for i in EDGE_IDS:
            for d in EDGE_DIRS:
                k = len(rows)
                rows.append(((0.25 - d[0] + 0.125 * (k % 5), 1e-39 if k >= 196 else 0.25 - d[1], -d[2]), d, i, t))
    rays, res = U._inputs(rows)
    rays.setflags(write=False)
    res.setflags(write=False)
    return rays, res


def edge_state(rng, n, num_paths, dead_every=0):
    """n states: a permutation's tasks (every path at one slot at most), throughputs in [0, 1] with
    some exact 0, 1 and denormal entries; every dead_every-th slot dead (task -1)."""
    thr = rng.random((n, 3)).astype(F)
    thr[0::11] = 1.0
    thr[3::13, 1] = 0.0
    thr[5::17, 2] = 1e-39
    st = np.zeros((n, 4), np.int32)
    st[:, :3] = thr.view(np.int32)
    st[:, 3] = rng.permutation(num_paths)[:n]
    if dead_every:
        st[dead_every - 1::dead_every, 3] = -1
    return st


def survivor_patterns(n, rng):
    """(label, hit mask) for n slots: the patterns the compaction is checked on."""
    idx = np.arange(n)
    out = [("all", np.ones(n, bool)), ("none", np.zeros(n, bool)), ("first", idx == 0), ("last", idx == n - 1),
           ("alternating", idx % 2 == 0), ("one per 257", idx % 257 == 256)]
    for pct in (1, 50, 99):
        out.append((f"random {pct}%", rng.random(n) < pct / 100.0))
    return out


def slots_for(mask, rng):
    """Rays, results for a survivor mask: table rays recycled, hits with random ids and t, misses -1."""
    rays, _ = edge_inputs()
    n = len(mask)
    r = np.ascontiguousarray(rays[np.arange(n) % len(rays)])
    res = np.zeros((n, 4), np.int32)
    res[:, 0] = np.where(mask, rng.integers(0, NUM_TRIS, n), -1)
    res[:, 1] = rng.uniform(0.5, 3.0, n).astype(F).view(np.int32)
    return r, res


# ---- (seed, vertex, key) whose words convert to exactly 2^32 ---------------------------------------------------
def find_wrap_edges(limit=1 << 27, chunk=1 << 22):
    """{word index: first hash input}: inputs x = seed + vertex * 0x9e3779b9 + key whose
    word `index` of the five used (offset a, b, c; shift a', b') is >= 0xFFFFFF80, so that its float
    conversion is 2^32 and the offset or shift exactly 1."""
    found = {}
    for lo in range(0, limit, chunk):
        x = np.arange(lo, lo + chunk, dtype=np.uint64)
        two, three = hash_words(0, 0, x)
        words = np.concatenate([two, three[:, :2]], axis=1)
        for w in range(5):
            if w not in found:
                at = np.flatnonzero(words[:, w] >= 0xFFFFFF80)
                if len(at):
                    found[w] = int(x[at[0]])
        if len(found) == 5:
            break
    return found


# word index -> the first hash input with that word >= 0xFFFFFF80: found by find_wrap_edges(limit=1 << 29),
# asserted by test_path.py before it relies on them. Words 0..2 are light_util.WRAP_EDGES' inputs: at
# vertex 0 the offset is the shadow frame's.
WRAP_INPUTS = {0: 15341454, 1: 49039794, 2: 56569215, 3: 466537, 4: 20384635}


# ---- a whole frame with the trace as a callback ------------------------------------------------------------------
def render_batch(impl, trace, prim, pres, first, count, normals, material, num_samples, depth, seed, compact, scalars,
                 feed=None, log=None):
    """One batch's radiance [count * S, 4] by impl (Model or mrt.host). trace(rays, any_hit) ->
    results int32 [m, 4]. feed(vertex, kind, m), where given, supplies the results instead (a device's
    own). log, a list, receives (vertex, step dict, radiance after accumulate) copies."""
    n = count * num_samples
    radiance = np.zeros((n, 4), F)
    rays, res, state, slots, stats = prim[first:first + count], pres[first:first + count], None, n, []
    for b in range(depth + 1):
        step = impl.path_extend(rays, res, state, radiance, normals, material, vertex=b, depth=depth,
                                num_samples=num_samples, seed=seed, compact=compact, num_slots=slots, **scalars)
        stats.append(step["live"])
        m = step["live"] if compact else slots
        if step["live"] == 0:
            if log is not None:
                log.append((b, step, radiance.copy()))
            break
        sres = feed(b, "shadow", m) if feed else trace(step["shadow"][:m], True)
        impl.path_accumulate(step["state"], step["pending"], sres, radiance, num_slots=m)
        if log is not None:
            log.append((b, step, radiance.copy()))
        if b < depth:
            rays, state, slots = step["rays"][:m], step["state"][:m], m
            res = feed(b, "bounce", m) if feed else trace(rays, False)
    return radiance, stats


def render_frame(impl, trace, prim, pres, slot_to_id, num_pixels, normals, material, num_samples, depth, seeds,
                 batch_inputs, compact, scalars, want_image=False):
    """The whole frame batch by batch (RayGen::batching): pixels (and the float image), and the
    live counts of every batch."""
    pixels, image, stats = np.zeros(num_pixels, U32), (np.zeros((num_pixels, 4), F) if want_image else None), []
    for k, first in enumerate(range(0, len(prim), batch_inputs)):
        count = min(batch_inputs, len(prim) - first)
        radiance, st = render_batch(impl, trace, prim, pres, first, count, normals, material, num_samples, depth,
                                    seeds[k], compact, scalars)
        stats.append(st)
        impl.path_resolve(num_samples, slot_to_id, pres, radiance, num_pixels, first_primary=first, num_primary=count,
                          pixels=pixels, image=image)
    return (pixels, image, stats) if want_image else (pixels, stats)
