"""Shared by tests/test_light.py and tests/test_gpu_light.py: an independent model of the area
light's shadow rays and of the lit reconstruction, and the tables both are checked on.

The ray model restates the reference's rayGenShadowKernel (RayGenKernels.cu:231-293, with jenkinsMix,
hammersley and sobol2D, :36-75) from the kernel's text, not from csrc/light_common.hpp; the pixel
model restates the contract of mrt_reconstruct_lit (include/mrt.h) with the reference's device
fromABGR / toABGR (RendererKernels.cu:38-56). Both work elementwise on numpy float32 arrays, one
IEEE operation at a time in the kernel's order, and in uint32 for the mix and the Sobol words; a
framework vector operation is spelled out as the framework evaluates it (VectorBase::dot sums from
0, normalized() multiplies by 1 * rcp(length), rcp(0) = 0, max(a, b) = a > b ? a : b).
"""
import functools

import numpy as np

import frame_util as U

F = np.float32
U32 = np.uint32
INT_MIN, INT_MAX = -2**31, 2**31 - 1
TWO_M32 = F(2.0 ** -32)


# ---- the model: shadow rays --------------------------------------------------------------------
def jenkins_mix(a, b, c):
    """jenkinsMix (RayGenKernels.cu:36-47) on uint32 arrays; returns the mixed words."""
    a, b, c = (np.array(x, U32) for x in (a, b, c))
    with np.errstate(over="ignore"):
        a -= b; a -= c; a ^= c >> U32(13)
        b -= c; b -= a; b ^= a << U32(8)
        c -= a; c -= b; c ^= b >> U32(13)
        a -= b; a -= c; a ^= c >> U32(12)
        b -= c; b -= a; b ^= a << U32(16)
        c -= a; c -= b; c ^= b >> U32(5)
        a -= b; a -= c; a ^= c >> U32(3)
        b -= c; b -= a; b ^= a << U32(10)
        c -= a; c -= b; c ^= b >> U32(15)
    return a, b, c


def hash_words(seed_plus_task):
    """The three words after two mixes of (seed + task, 0x9e3779b9, 0x9e3779b9): uint32 [n, 3]."""
    a = np.atleast_1d(np.asarray(seed_plus_task, np.uint64) & np.uint64(0xFFFFFFFF)).astype(U32)
    g = np.full_like(a, 0x9E3779B9)
    a, b, c = jenkins_mix(*jenkins_mix(a, g, g))
    return np.stack([a, b, c], axis=1)


def offsets(seed, tasks):
    """(F32)hash * exp2(-32) per word: float32 [n, 3]. The conversion rounds to nearest even."""
    words = hash_words(np.asarray(tasks, np.uint64) + np.uint64(seed & 0xFFFFFFFF))
    return words.astype(F) * TWO_M32


def sobol2d(num):
    """sobol2D(i) for i < num: float32 [num, 2]."""
    out = np.zeros((num, 2), F)
    for i in range(num):
        r1, r2, v1, v2, k = 0, 0, 1 << 31, 3 << 30, i
        while k:
            if k & 1:
                r1 ^= v1
                r2 ^= (v2 << 1) & 0xFFFFFFFF
            v1 |= v1 >> 1
            v2 ^= v2 >> 1
            k >>= 1
        out[i] = (F(U32(r1)) * TWO_M32, F(U32(r2)) * TWO_M32)
    return out


def hammersley(num):
    return (np.arange(num).astype(F) + F(0.5)) / F(num)


def positions(off, num):
    """pos of every (input ray, sample): float32 [n, num, 3] in the cube [-1, 1)."""
    q = np.concatenate([sobol2d(num), hammersley(num)[:, None]], axis=1)   # [num, 3]
    p = q[None, :, :] + off[:, None, :]
    p = np.where(p >= F(1.0), p - F(1.0), p)
    p = p * F(2.0)
    return p - F(1.0)


def dot3(a, b):
    r = F(0.0) + a[..., 0] * b[..., 0]
    r = r + a[..., 1] * b[..., 1]
    return r + a[..., 2] * b[..., 2]


def rcp(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x != 0, F(1.0) / x, F(0.0)).astype(F)


def backed_off(rays, t):
    """inRay.origin + inRay.direction * fmaxf(t - epsilon, 0)."""
    back = np.fmax(t - F(1.0e-4), F(0.0))
    return rays[:, 0:3] + rays[:, 4:7] * back[:, None]


def result_t(results):
    return np.ascontiguousarray(results[:, 1]).view(F)


def shadow_rays(rays, results, num_samples, light, radius, seed, tasks=None):
    """The kernel's output for input ray j hashing seed + tasks[j] (default: j): float32
    [n * num_samples, 8], and the positions float32 [n, num_samples, 3]."""
    rays = np.ascontiguousarray(rays, F).reshape(-1, 8)
    results = np.ascontiguousarray(results, np.int32).reshape(-1, 4)
    n = len(rays)
    tasks = np.arange(n) if tasks is None else np.asarray(tasks)
    light, radius = np.asarray(light, F), F(radius)
    with np.errstate(all="ignore"):
        origin = backed_off(rays, result_t(results))
        pos = positions(offsets(seed, tasks), num_samples)
        target = light[None, None, :] + radius * pos
        d = target - origin[:, None, :]
        length = np.sqrt(dot3(d, d))
        direction = d * (F(1.0) * rcp(length))[..., None]
        out = np.empty((n, num_samples, 8), F)
        out[:, :, 0:3] = origin[:, None, :]
        out[:, :, 3] = 0.0
        out[:, :, 4:7] = direction
        out[:, :, 7] = np.where(results[:, 0:1] == -1, F(-1.0), length)
    return out.reshape(-1, 8), pos


# ---- the model: lit pixels ---------------------------------------------------------------------
def from_abgr(c):
    c = np.asarray(c, U32)
    k = F(1.0) / F(255.0)
    return np.stack([(c & 0xFF).astype(F) * k, ((c >> 8) & 0xFF).astype(F) * k, ((c >> 16) & 0xFF).astype(F) * k,
                     (c >> 24).astype(F) * k], axis=-1)


def to_abgr(v):
    with np.errstate(invalid="ignore"):
        b = (np.fmin(np.fmax(v, F(0.0)), F(1.0)) * F(255.0)).astype(U32)   # truncates
    return b[..., 0] | b[..., 1] << 8 | b[..., 2] << 16 | b[..., 3] << 24


BACKGROUND = int(to_abgr(np.array([0.2, 0.4, 0.8, 1.0], F)))


def lit_factor(rays, results, normals, light):
    """k per primary: max(dot(nf, l), 0); rows whose id is -1 get 0 and are not looked up."""
    rays = np.ascontiguousarray(rays, F).reshape(-1, 8)
    ids = results[:, 0]
    with np.errstate(all="ignore"):
        origin = backed_off(rays, result_t(results))
        to_light = np.asarray(light, F)[None, :] - origin
        l = to_light * (F(1.0) * rcp(np.sqrt(dot3(to_light, to_light))))[:, None]
        nf = np.asarray(normals, F)[np.where(ids == -1, 0, ids)]
        nf = np.where((dot3(nf, rays[:, 4:7]) > 0)[:, None], -nf, nf)
        c = dot3(nf, l)
        return np.where(c > 0, c, F(0.0)).astype(F)


def lit_pixels(num_samples, slot_to_id, primary_rays, primary_results, batch_results, normals, material, light,
               num_pixels, batch_id_to_slot=None, first_primary=0, num_primary=None, pixels=None):
    """mrt_reconstruct_lit's pixels, untouched ones 0 (or `pixels`' own)."""
    n = num_samples
    pres = np.ascontiguousarray(primary_results, np.int32).reshape(-1, 4)
    bres = np.ascontiguousarray(batch_results, np.int32).reshape(-1, 4)
    if num_primary is None:
        num_primary = len(bres) // n
    sl = slice(first_primary, first_primary + num_primary)
    pres, prays = pres[sl], np.ascontiguousarray(primary_rays, F).reshape(-1, 8)[sl]
    at = np.arange(num_primary * n) if batch_id_to_slot is None else np.asarray(batch_id_to_slot)[:num_primary * n]
    unblocked = (bres[at, 0].reshape(num_primary, n) == -1).sum(axis=1)
    v = unblocked.astype(F) * (F(1.0) / F(n))
    k = lit_factor(prays, pres, normals, light)
    with np.errstate(all="ignore"):
        kv = k * v
        m = from_abgr(np.asarray(material, U32)[np.where(pres[:, 0] == -1, 0, pres[:, 0])])
        colour = np.stack([m[:, 0] * kv, m[:, 1] * kv, m[:, 2] * kv, np.ones_like(kv)], axis=1)
    px = np.where(pres[:, 0] == -1, U32(BACKGROUND), to_abgr(colour)).astype(U32)
    out = np.zeros(num_pixels, U32) if pixels is None else pixels
    out[np.asarray(slot_to_id)[sl]] = px
    return out


# ---- A. the generator's edge table --------------------------------------------------------------
EDGE_COUNTS = [1, 255, 256, 257]
EDGE_FIRSTS = [0, 1, 255]
EDGE_SAMPLES = [1, 3, 64, 257]
EDGE_SEEDS = [1, 0xFFFFFFF0]   # the second: seed + task wraps at task 16
EDGE_IDS = [-1, 0, 5, -2, INT_MIN, INT_MAX]
EDGE_T = U.EDGE_T              # 0, 5e-5, 1e-4, 1.0001e-4, 1, inf, NaN, -1, 1e-39
EDGE_DIRS = [(0.0, 0.0, -1.0), (0.6, 0.0, -0.8), (-0.0, 1.0, 0.0)]
ORDINARY_LIGHT = ((1.5, -2.0, 3.25), 0.75)
# (seed + task, word) whose mixed word converts to 2^32, so that the offset is exactly 1.0; found
# with a numpy search over the mix, asserted by test_light.py before it relies on them
WRAP_EDGES = [(15341454, 0, 0xFFFFFF8D), (49039794, 1, 0xFFFFFFD5), (56569215, 2, 0xFFFFFFAD)]


@functools.lru_cache(maxsize=None)
def edge_inputs():
    """512 input rays (rays float32 [512, 8], results int32 [512, 4]), read-only: every id x t x
    direction of the table (162 rows), repeated from other origins up to max(first) + max(count)."""
    rows = []
    k = 0
    while len(rows) < max(EDGE_FIRSTS) + max(EDGE_COUNTS):
        for t in EDGE_T:
            for i in EDGE_IDS:
                for d in EDGE_DIRS:
                    # the second round's y is a denormal, which neither side flushes
                    rows.append(((0.25 - d[0] + 0.125 * k, 1e-39 if k == 1 else 0.25 - d[1], -d[2]), d, i, t))
        k += 1
    rays, res = U._inputs(rows[:max(EDGE_FIRSTS) + max(EDGE_COUNTS)])
    rays.setflags(write=False)
    res.setflags(write=False)
    return rays, res


def lights():
    """(label, position, radius, ray) of the table's lights. `ray`, where not None, is the input
    ray (a hit with t = 1) whose own backed-off origin the light sits on."""
    rays, res = edge_inputs()
    own = int(np.nonzero((res[:, 0] != -1) & (result_t(res) == 1.0))[0][0])
    on_origin = tuple(float(x) for x in backed_off(rays[own:own + 1], result_t(res[own:own + 1]))[0])
    return [("ordinary", ORDINARY_LIGHT[0], ORDINARY_LIGHT[1], None),
            ("radius0", (1.5, -2.0, 3.25), 0.0, None),
            ("on-origin", on_origin, 0.0, own),
            ("1e30", (1e30, -1e30, 1e30), 0.5, None),
            ("nan", (0.5, float("nan"), 1.0), 0.25, None)]


def same_rays(a, b):
    """Bit for bit, a NaN equal to a NaN (the bits of a NaN an operation makes differ between
    x86 and gfx950)."""
    a, b = np.asarray(a, F).reshape(-1, 8), np.asarray(b, F).reshape(-1, 8)
    return a.shape == b.shape and bool(U.same_bits_or_nan(a, b).all())


# ---- B. the lit reconstruction's synthetic table ---------------------------------------------------
LIT_FIRSTS = [0, 1, 255, 256]
LIT_COUNT = 300   # primaries per batch: two workgroups of the device kernel, the second partial


@functools.lru_cache(maxsize=None)
def lit_table():
    """64 triangles' normals (the first eight at the edges: +z, -z, zero, NaN, +x, -x, +y, one NaN
    component), frame_util's material table, and 256 + LIT_COUNT primaries (rays, results, pixel
    table), read-only. Every primary looks down or slants down from z = 1 and ends at t = 1, so a
    light at the height of the backed-off points (LIT_LIGHTS[0]) is at right angles to the +-z
    normals: k = 0."""
    rng = np.random.default_rng(77)
    normals = rng.normal(size=(64, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(F)
    normals[:8] = [(0, 0, 1), (0, 0, -1), (0, 0, 0), (np.nan,) * 3, (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0.6, np.nan, 0.8)]
    material, _ = U.colour_tables()
    n = max(LIT_FIRSTS) + LIT_COUNT
    rays = np.zeros((n, 8), F)
    rays[:, 0] = rng.uniform(-2, 2, n)
    rays[:, 1] = rng.uniform(-2, 2, n)
    rays[:, 2] = 1.0
    rays[:, 4:7] = (0.0, 0.0, -1.0)
    slant = np.arange(n) % 3 == 2
    rays[slant, 4:7] = (0.6, 0.0, -0.8)
    rays[:, 7] = 100.0
    ids = rng.integers(0, 64, n)
    ids[np.arange(n) % 4 == 0] = np.arange(n)[np.arange(n) % 4 == 0] // 4 % 8   # the edge normals, often
    ids[rng.random(n) < 0.15] = -1
    res = U.results(ids)
    res[:, 1] = np.full(n, 1.0, F).view(np.int32)
    num_pixels = n + 9
    s2i = rng.permutation(num_pixels)[:n].astype(np.int32)
    for a in (normals, rays, res, s2i):
        a.setflags(write=False)
    return normals, material, rays, res, s2i, num_pixels


def lit_lights():
    """The light level with the straight-down primaries' backed-off points, and an ordinary one."""
    z0 = F(1.0) + F(-1.0) * (F(1.0) - F(1.0e-4))
    return [(5.0, 0.25, float(z0)), (1.0, 2.0, 3.0)]


def batch_ids(rng, count, n):
    """Shadow results of count primaries, n rays each: all reached, none reached, and mixtures."""
    ids = np.where(rng.random((count, n)) < 0.5, -1, rng.integers(0, 64, (count, n)))
    ids[0::7] = -1
    ids[1::7] = 3
    return ids.reshape(-1).astype(np.int32)


def lit_case(first, n, permuted, light, rng):
    """The keyword arguments (mrt.host.reconstruct_lit's and lit_pixels') of one batch of LIT_COUNT
    primaries from `first` on; permuted: the results live at shuffled slots and batch_id_to_slot
    finds them."""
    normals, material, rays, res, s2i, num_pixels = lit_table()
    ids = batch_ids(rng, LIT_COUNT, n)
    b2s, stored = None, ids
    if permuted:
        b2s = rng.permutation(len(ids)).astype(np.int32)
        stored = np.empty_like(ids)
        stored[b2s] = ids
    return dict(num_samples=n, slot_to_id=s2i, primary_rays=rays, primary_results=res, batch_results=U.results(stored),
                normals=normals, material=material, light=light, num_pixels=num_pixels, batch_id_to_slot=b2s,
                first_primary=first, num_primary=LIT_COUNT)
