"""Shared by tests/test_sampling.py and tests/test_gpu_sampling.py: float64 references of the light,
bounce and AO samplers with a first-order error bound per sample, and the closed forms the frames
of known expectation are held to. numpy only.

The restatements are written from the text of include/mrt.h (mrt_raygen_shadow, mrt_path_extend,
mrt_raygen_ao), not from the float32 models of light_util / path_util: the Jenkins words are exact
integers, a word's offset is word / 2^32 (no conversion), the radical inverses are exact fractions,
cos and sin are libm's. What they read (rays, t, normals, light, seed) are the float32 values the
kernels read, promoted.

The bound. Every quantity is a pair `E(v, e)`: v the float64 value, e a bound on |float32 result - v|.
An operation gives v = op(a.v, b.v) and, with eps = 2^-24 (one rounding, relative, per operation),
    a + b      e = p + eps (|v| + p),           p = a.e + b.e
    a * b      e = p + eps (|v| + p),           p = |a.v| b.e + |b.v| a.e + a.e b.e
    sqrt(a)    e = p + eps (|v| + p),           p = min(a.e / (sqrt(a.v) + sqrt(max(a.v - a.e, 0))), sqrt(a.v + a.e))
    1 / a      e = p + eps (|v| + p),           p = a.e / (|a.v| (|a.v| - a.e))
    cos, sin   e = a.e + f                      f the routine's own absolute error (below)
    2^k a, -a  e = 2^k a.e, a.e                 exact operations
so the conditioning 1 / (2 sqrt(u1)) of the disk radius and 1 / (2 sqrt(1 - u1)) of z, 2 pi times the
error of u2, and (|origin| + |target|) eps / radius of a light position recovered from a ray all come
out of the values the reference itself passes through; no constant is fitted. The sources of error
that are not roundings of an operation:
    a hash word's conversion to float32       2^-25 (half an ulp below 2^32, times 2^-32)
    1.0f / 3.0f, the float32 pi, 1e-4f        |constant - float32(constant)|
    the polynomial cos / sin of a path        9e-8 (measured 8.96e-8 over all multiples of 2^-24)
    cosf / sinf of the AO generator           4 ulp of 1 = 4 * 2^-23: OpenCL's bound for a device's cos and
                                              sin, which covers glibc's (under 1 ulp) on the host
A wrap `if (p >= 1) p -= 1` is a jump: where the float64 sum lies within its own bound of 1 the
float32 side may land on the other side of it, so such a slot is `edge` and no bound applies to it
(the tests count these slots). cos and sin of the wrapped u2 are continuous: no jump there.
"""
import functools

import numpy as np

EPS = 2.0 ** -24
GOLDEN = 0x9E3779B9
POLY_ERR = 9e-8
LIBM_ERR = 4 * 2.0 ** -23
_M = np.uint64(0xFFFFFFFF)


# ---- value-and-bound arithmetic -------------------------------------------------------------------
class E:
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.asarray(e, np.float64) + np.zeros_like(self.v)

    @staticmethod
    def _r(v, p):
        return E(v, p + EPS * (np.abs(v) + p))

    def __add__(self, o):
        return E._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return E._r(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return E._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __neg__(self):
        return E(-self.v, self.e)

    def scaled(self, k):
        """Times a power of two: exact."""
        return E(self.v * k, self.e * abs(k))

    def sqrt(self):
        a = np.maximum(self.v, 0.0)
        den = np.sqrt(a) + np.sqrt(np.maximum(a - self.e, 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where(den > 0, self.e / np.where(den > 0, den, 1.0), np.inf)
        return E._r(np.sqrt(a), np.minimum(p, np.sqrt(a + self.e)))

    def rcp(self):
        a = np.abs(self.v)
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where(a > self.e, self.e / (a * (a - self.e)), np.inf)
            return E._r(1.0 / self.v, p)

    def max0(self):
        """max(a, 0): 1-Lipschitz, no rounding."""
        return E(np.maximum(self.v, 0.0), self.e)

    def cos(self, f):
        return E(np.cos(self.v), self.e + f)

    def sin(self, f):
        return E(np.sin(self.v), self.e + f)


def exact(x):
    return E(np.asarray(x, np.float64))


def const(x):
    """A real constant the code holds as its float32 rounding."""
    return E(x, abs(float(np.float32(x)) - x))


def dot(a, b):
    r = a[0] * b[0]   # the sum starts from 0: 0 + p is exact
    r = r + a[1] * b[1]
    return r + a[2] * b[2]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def normalized(a):
    s = dot(a, a).sqrt().rcp()   # 1 * rcp(length): the product with 1 is exact
    return [c * s for c in a]


def vec(a):
    """float32 [n, 3] -> three exact E."""
    a = np.asarray(a)
    return [exact(a[:, k]) for k in range(3)]


# ---- the hash, exact ------------------------------------------------------------------------------
def jenkins(a, b, c):
    """jenkinsMix on uint64 arrays holding 32-bit words."""
    def step(x, y, z, shift, left):
        x = (x - y - z) & _M
        return x ^ (((z << np.uint64(shift)) & _M) if left else (z >> np.uint64(shift)))
    for s1, s2, s3 in ((13, 8, 13), (12, 16, 5), (3, 10, 15)):
        a = step(a, b, c, s1, False)
        b = step(b, c, a, s2, True)
        c = step(c, a, b, s3, False)
    return a, b, c


def hash_words(x):
    """Words (a, b, c) after two mixes of (x mod 2^32, g, g) and (a', b', c') after a third: uint64 [n, 3] each."""
    a = np.asarray(x, np.uint64) & _M
    g = np.full_like(a, GOLDEN)
    two = jenkins(*jenkins(a, g, g))
    return np.stack(two, 1), np.stack(jenkins(*two), 1)


def path_hash_input(seed, vertex, key):
    return (np.asarray(key, np.uint64) + np.uint64(seed & 0xFFFFFFFF) + np.uint64((vertex * GOLDEN) & 0xFFFFFFFF)) & _M


def unit(words):
    """word / 2^32 in [0, 1), exact in float64; the float32 side converts first: 2^-25."""
    return E(words.astype(np.float64) * 2.0 ** -32, 2.0 ** -25)


# ---- the low-discrepancy points, exact ---------------------------------------------------------------
def radical_inverse(i, base):
    i, num, den = int(i), 0, 1
    while i:
        num, den = num * base + i % base, den * base
        i //= base
    return num / den


@functools.lru_cache(maxsize=None)
def halton23(num):
    """([num] base-2 inverses of s + 1: exact in float32 too; E of the base-3 ones, whose float32 loop
    multiplies by the rounded third once per digit): the bound runs the loop in E arithmetic."""
    h2 = np.array([radical_inverse(s + 1, 2) for s in range(num)])
    third, v3, e3 = const(1.0 / 3.0), [], []
    for s in range(num):
        y, yadd, k = exact(0.0), exact(1.0), s + 1
        while k:
            yadd = yadd * third
            y = y + exact(float(k % 3)) * yadd
            k //= 3
        v3.append(radical_inverse(s + 1, 3))
        e3.append(float(y.e) + abs(float(y.v) - v3[-1]))
    return h2, np.array(v3), np.array(e3)


@functools.lru_cache(maxsize=None)
def sobol2d(num):
    """The reference's sobol2D with its `r2 ^= v2 << 1`: [num, 2], multiples of 2^-32 and exact."""
    out = np.zeros((num, 2))
    for i in range(num):
        r1, r2, v1, v2, k = 0, 0, 1 << 31, 3 << 30, i
        while k:
            if k & 1:
                r1 ^= v1
                r2 ^= (v2 << 1) & 0xFFFFFFFF
            v1 |= v1 >> 1
            v2 ^= v2 >> 1
            k >>= 1
        out[i] = (r1 / 2.0 ** 32, r2 / 2.0 ** 32)
    return out


def wrapped(p):
    """(p mod 1 after one wrap, edge): edge where the sum is within its bound of the jump at 1."""
    over = p.v >= 1.0
    return E(np.where(over, p.v - 1.0, p.v), p.e), np.abs(p.v - 1.0) <= p.e


# ---- the samplers -------------------------------------------------------------------------------------
def backed_off(rays, t):
    back = (exact(t) - const(1.0e-4)).max0()
    o, d = vec(rays[:, 0:3]), vec(rays[:, 4:7])
    return [o[k] + d[k] * back for k in range(3)]


def cube_positions(words2, s, num_samples):
    """pos of slots with offset words words2 [n, 3] and sample s [n]: three E in [-1, 1), and edge."""
    sob = sobol2d(num_samples)[s]
    ham = E._r((s + 0.5) / num_samples, 0.0)
    off = unit(words2)
    pos, edge = [], np.zeros(len(s), bool)
    for k, q in enumerate((exact(sob[:, 0]), exact(sob[:, 1]), ham)):
        p, e = wrapped(q + E(off.v[:, k], off.e[:, k]))
        pos.append(p.scaled(2.0) - exact(1.0))
        edge |= e
    return pos, edge


def shadow_from(origin, pos, ids, light, radius):
    """(ray [n, 8] values, [n, 8] bounds) of mrt_raygen_shadow's ray from `origin` to the cube position."""
    light, radius = np.asarray(light, np.float32), exact(np.float32(radius))
    d = [(exact(light[k]) + radius * pos[k]) - origin[k] for k in range(3)]
    length = dot(d, d).sqrt()
    s = length.rcp()
    n = len(ids)
    v, e = np.zeros((n, 8)), np.zeros((n, 8))
    for k in range(3):
        v[:, k], e[:, k] = origin[k].v, origin[k].e
        c = d[k] * s
        v[:, 4 + k], e[:, 4 + k] = c.v, c.e
    v[:, 7], e[:, 7] = np.where(ids == -1, -1.0, length.v), np.where(ids == -1, 0.0, length.e)
    return v, e


def shadow_rays(rays, results, num_samples, light, radius, seed):
    """mrt_raygen_shadow: {v, e: [n * S, 8], edge: [n * S], pos: [n * S, 3]}; output ray j * S + s."""
    rays, results = np.asarray(rays, np.float32).reshape(-1, 8), np.asarray(results).view(np.int32).reshape(-1, 4)
    S, n = num_samples, len(rays)
    at, s = np.repeat(np.arange(n), S), np.tile(np.arange(S), n)
    two, _ = hash_words(np.arange(n, dtype=np.uint64) + np.uint64(seed & 0xFFFFFFFF))
    origin = backed_off(rays[at], results[at, 1].view(np.float32))
    pos, edge = cube_positions(two[at], s, S)
    v, e = shadow_from(origin, pos, results[at, 0], light, radius)
    return {"v": v, "e": e, "edge": edge, "pos": np.stack([p.v for p in pos], 1)}


def facing(normal, d):
    """The normal turned against the ray, by the float32 rule; `clear`: the float64 dot product is away
    from 0 by more than its own bound, so both precisions turn it the same way."""
    c = dot(vec(normal), vec(d))
    return np.where((c.v > 0)[:, None], -normal, normal).astype(np.float32), np.abs(c.v) > c.e


def tangent_frame(nf):
    """perp / biperp of float32 normals [n, 3] by the contract's branch rule (the comparisons are of
    the float32 inputs themselves: no bound enters): two lists of three E."""
    na = np.abs(nf)
    nm = np.where(np.where(na[:, 0] > na[:, 1], na[:, 0], na[:, 1]) > na[:, 2],
                  np.where(na[:, 0] > na[:, 1], na[:, 0], na[:, 1]), na[:, 2])
    zero = np.zeros(len(nf), np.float32)
    by_z, by_x = nm == na[:, 2], nm == na[:, 0]
    perp = np.stack([nf[:, 1], -nf[:, 0], zero], 1)
    perp = np.where(by_z[:, None], np.stack([zero, nf[:, 2], -nf[:, 1]], 1),
                    np.where(by_x[:, None], np.stack([-nf[:, 2], zero, nf[:, 0]], 1), perp))
    perp = normalized(vec(perp))
    return perp, cross(vec(nf), perp)


def bounce_dirs(nf, s, words3, num_samples):
    """mrt_path_extend's bounce direction: three E, edge, and the float64 (u1, u2) and shift."""
    h2, h3, e3 = halton23(num_samples)
    sh = unit(words3)
    u1, edge = wrapped(exact(h2[s]) + E(sh.v[:, 0], sh.e[:, 0]))
    u2, _ = wrapped(E(h3[s], e3[s]) + E(sh.v[:, 1], sh.e[:, 1]))
    turn = u2.scaled(2.0 * np.pi)   # the code never forms the angle: 2 pi times the error of u2
    cs, sn = turn.cos(POLY_ERR), turn.sin(POLY_ERR)
    r = u1.sqrt()
    x, y = r * cs, r * sn
    z = ((exact(1.0) - x * x) - y * y).max0().sqrt()
    perp, biperp = tangent_frame(nf)
    n = vec(nf)
    d = normalized([(perp[k] * x + biperp[k] * y) + n[k] * z for k in range(3)])
    return d, edge, np.stack([u1.v, u2.v], 1), sh.v[:, :2]


def path_extend(rays, results, tasks, normals, vertex, depth, num_samples, seed, light, radius, max_dist):
    """One vertex step of slots that all hit (the caller passes the survivors' rays, results and tasks):
    {shadow_v, shadow_e, bounce_v, bounce_e: [n, 8] (bounce None at vertex == depth), edge_shadow,
    edge_bounce, clear, nf, pos, u, shift}."""
    rays, results = np.asarray(rays, np.float32).reshape(-1, 8), np.asarray(results).view(np.int32).reshape(-1, 4)
    S, tasks = num_samples, np.asarray(tasks, np.int64)
    s = tasks % S
    key = tasks // S if vertex == 0 else tasks
    two, three = hash_words(path_hash_input(seed, vertex, key))
    ids = results[:, 0]
    origin = backed_off(rays, results[:, 1].view(np.float32))
    nf, clear = facing(np.asarray(normals, np.float32)[ids], rays[:, 4:7])
    pos, edge_shadow = cube_positions(two, s, S)
    sv, se = shadow_from(origin, pos, ids, light, radius)
    out = {"shadow_v": sv, "shadow_e": se, "edge_shadow": edge_shadow, "clear": clear, "nf": nf,
           "pos": np.stack([p.v for p in pos], 1), "bounce_v": None, "bounce_e": None,
           "offset": two.astype(np.float64) * 2.0 ** -32}
    if vertex < depth:
        d, edge, u, shift = bounce_dirs(nf, s, three, S)
        bv, be = np.zeros((len(rays), 8)), np.zeros((len(rays), 8))
        for k in range(3):
            bv[:, k], be[:, k] = origin[k].v, origin[k].e
            bv[:, 4 + k], be[:, 4 + k] = d[k].v, d[k].e
        bv[:, 7] = np.float32(max_dist)
        out.update(bounce_v=bv, bounce_e=be, edge_bounce=edge, u=u, shift=shift)
    return out


def ao_rays(rays, results, normals, num_samples, max_dist, seed):
    """mrt_raygen_ao: {v, e: [n * S, 8], clear: [n * S], nf: [n * S, 3], angle: [n] the hash angle / 2 pi}."""
    rays, results = np.asarray(rays, np.float32).reshape(-1, 8), np.asarray(results).view(np.int32).reshape(-1, 4)
    S, n = num_samples, len(rays)
    ids = results[:, 0]
    normal = np.tile(np.array([1, 0, 0], np.float32), (n, 1))
    inside = (ids >= 0) & (ids < len(normals))
    normal[inside] = np.asarray(normals, np.float32)[ids[inside]]
    nf, clear = facing(normal, rays[:, 4:7])
    origin = backed_off(rays, results[:, 1].view(np.float32))
    perp, biperp = tangent_frame(nf)
    two, _ = hash_words(np.arange(n, dtype=np.uint64) + np.uint64(seed & 0xFFFFFFFF))
    hc = two[:, 2].astype(np.float64)
    two_pi = const(np.pi).scaled(2.0)
    # the float32 side converts the word (half an ulp: at most 128), multiplies, and scales by 2^-32
    angle = (two_pi * E(hc, 0.5 * 2.0 ** np.maximum(np.floor(np.log2(np.maximum(hc, 1.0))) - 23, 0))).scaled(2.0 ** -32)
    ca, sa = angle.cos(LIBM_ERR), angle.sin(LIBM_ERR)
    t0 = [perp[k] * ca + biperp[k] * sa for k in range(3)]
    t1 = [perp[k] * (-sa) + biperp[k] * ca for k in range(3)]
    nn = vec(nf)
    h2, h3, e3 = halton23(S)
    v, e = np.zeros((n, S, 8)), np.zeros((n, S, 8))
    for s in range(S):
        a2 = two_pi * E(h3[s], e3[s])
        r = exact(h2[s]).sqrt()
        x, y = r * a2.cos(LIBM_ERR), r * a2.sin(LIBM_ERR)
        z = ((exact(1.0) - x * x) - y * y).sqrt()
        d = normalized([(t0[k] * x + t1[k] * y) + nn[k] * z for k in range(3)])
        for k in range(3):
            v[:, s, k], e[:, s, k] = origin[k].v, origin[k].e
            v[:, s, 4 + k], e[:, s, 4 + k] = d[k].v, d[k].e
        v[:, s, 7] = np.where(ids == -1, -1.0, np.float32(max_dist))
    return {"v": v.reshape(-1, 8), "e": e.reshape(-1, 8), "clear": np.repeat(clear, S), "nf": np.repeat(nf, S, axis=0),
            "angle": hc * 2.0 ** -32}


def local_frame(nf):
    """(perp, biperp, nf) as float64 [n, 3] each: the frame a direction is read back in."""
    perp, biperp = tangent_frame(nf)
    return np.stack([c.v for c in perp], 1), np.stack([c.v for c in biperp], 1), np.asarray(nf, np.float64)


# ---- closed forms ----------------------------------------------------------------------------------------
def form_factor(px, py, c, x0, x1, y0, y1):
    """The form factor of a surface point at (px, py), its normal towards the plane, to the parallel
    rectangle [x0, x1] x [y0, y1] at distance c: the four-corner sum F = G(x1 - px, y1 - py) -
    G(x0 - px, y1 - py) - G(x1 - px, y0 - py) + G(x0 - px, y0 - py), G(a, b) = sgn(a) sgn(b) H(|a|, |b|),
    H(a, b) = (1 / 2 pi) [a / sqrt(a^2 + c^2) atan(b / sqrt(a^2 + c^2)) + b / sqrt(b^2 + c^2) atan(a / sqrt(b^2 + c^2))]."""
    px, py, c = np.asarray(px, np.float64), np.asarray(py, np.float64), np.asarray(c, np.float64)

    def G(a, b):
        sa, sb = np.abs(a), np.abs(b)
        ra, rb = np.sqrt(sa * sa + c * c), np.sqrt(sb * sb + c * c)
        return np.sign(a) * np.sign(b) * (sa / ra * np.arctan(sb / ra) + sb / rb * np.arctan(sa / rb)) / (2.0 * np.pi)
    return G(x1 - px, y1 - py) - G(x0 - px, y1 - py) - G(x1 - px, y0 - py) + G(x0 - px, y0 - py)


def gauss_legendre(lo, hi, n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (hi - lo) * x + 0.5 * (hi + lo), 0.5 * (hi - lo) * w


def form_factor_quadrature(px, py, c, x0, x1, y0, y1, n=200):
    """The same by brute force: the integral of cos cos' / (pi r^2) = c^2 / (pi r^4) over the rectangle."""
    x, wx = gauss_legendre(x0, x1, n)
    y, wy = gauss_legendre(y0, y1, n)
    r2 = (x[:, None] - px) ** 2 + (y[None, :] - py) ** 2 + c * c
    return float((wx[:, None] * wy[None, :] * c * c / (np.pi * r2 * r2)).sum())


def visible_share(px, pz, edge_x, edge_z, cx, cz, R):
    """The share of the square [cx - R, cx + R] x [cz - R, cz + R] in (X, Z) that a receiver at
    (px, pz) sees past a straight edge at (edge_x, edge_z) parallel to y, the occluder reaching from the
    edge towards -x: the points whose line of sight crosses z = edge_z at x > edge_x. The square is
    clipped by the line through the receiver and the edge (one Sutherland-Hodgman pass) and the area
    is the clipped polygon's (shoelace). px: array; the rest scalars."""
    out = np.zeros(len(px))
    corners = [(cx - R, cz - R), (cx + R, cz - R), (cx + R, cz + R), (cx - R, cz + R)]
    for i, (x, z) in enumerate(zip(np.asarray(px, np.float64), np.broadcast_to(np.asarray(pz, np.float64), np.shape(px)))):
        ex, ez = edge_x - x, edge_z - z   # visible side: cross((ex, ez), (X - x, Z - z)) < 0, i.e. to the +x side of the line going up
        side = [ex * (Z - z) - ez * (X - x) for X, Z in corners]
        poly = []
        for k in range(4):
            a, b, sa, sb = corners[k], corners[(k + 1) % 4], side[k], side[(k + 1) % 4]
            if sa <= 0:
                poly.append(a)
            if (sa < 0 < sb) or (sb < 0 < sa):
                t = sa / (sa - sb)
                poly.append((a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1])))
        area = 0.0
        for k in range(len(poly)):
            (x1, z1), (x2, z2) = poly[k], poly[(k + 1) % len(poly)]
            area += x1 * z2 - x2 * z1
        out[i] = abs(area) / 2.0 / (4.0 * R * R)
    return out


def two_bounce_term(px, py, pz, occ, height, floor, n):
    """The integral over the occluder's underside (the rectangle occ = (x0, x1, y0, y1) at z = height)
    of K(p, q) (1 - F_floor(q)) dq for receivers p = (px, py, pz) on the floor looking up: K = cos cos' /
    (pi r^2) = c^2 / (pi r^4), c = height - pz; F_floor(q) the form factor of q, looking down, to the
    rectangle floor = (x0, x1, y0, y1) at distance `height`. An n x n Gauss-Legendre rule."""
    x, wx = gauss_legendre(occ[0], occ[1], n)
    y, wy = gauss_legendre(occ[2], occ[3], n)
    qx, qy = np.meshgrid(x, y, indexing="ij")
    w = (wx[:, None] * wy[None, :] * (1.0 - form_factor(qx, qy, height, *floor))).reshape(-1)
    qx, qy = qx.reshape(-1), qy.reshape(-1)
    px, py, pz = (np.asarray(a, np.float64) for a in (px, py, pz))
    out = np.zeros(len(px))
    for lo in range(0, len(px), 512):
        sl = slice(lo, lo + 512)
        c = (height - pz[sl])[:, None]
        r2 = (qx[None, :] - px[sl, None]) ** 2 + (qy[None, :] - py[sl, None]) ** 2 + c * c
        out[sl] = (c * c / (np.pi * r2 * r2) * w[None, :]).sum(axis=1)
    return out


# ---- statistics ----------------------------------------------------------------------------------------------
CHI2_1E6 = {255: 377.078, 63: 131.370}   # the 1 - 10^-6 quantiles, from the chi-square distribution's tables


def chi2_quantile_1e6(k):
    """The 1 - 10^-6 quantile of chi-square with k degrees of freedom, tabulated."""
    return CHI2_1E6[k]


def wilson_hilferty_1e6(k):
    """The same by Wilson and Hilferty's cube, k (1 - 2 / (9k) + z sqrt(2 / (9k)))^3 with z = 4.753424 the
    normal quantile: the check on the table's entries (it lies 0.17 and 0.37 above them)."""
    a = 2.0 / (9.0 * k)
    return k * (1.0 - a + 4.753424 * np.sqrt(a)) ** 3


def chi2_uniform(cells, num_cells):
    counts = np.bincount(cells, minlength=num_cells).astype(np.float64)
    want = len(cells) / num_cells
    return float(((counts - want) ** 2 / want).sum())


def z_score(x, mean, variance):
    return float((x.mean() - mean) / np.sqrt(variance / len(x)))


def pearson(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))
