"""Shared by tests/test_denoise.py and tests/test_gpu_denoise.py: an independent model of the path
frame's denoiser and the tables both are checked on.

The model restates the contract of mrt_denoise_features / mrt_denoise_filter from the text of
include/mrt.h, not from csrc/denoise_common.hpp. It works on numpy float32 arrays over all pixels
at once, one IEEE operation at a time in the documented order; the 25 taps are 25 shifted views
of the frame, visited dy outer and dx inner. fromABGR / toABGR are light_util's, themselves written
from the reference's kernel text. `Model` has mrt.host's two signatures.
"""
import functools

import numpy as np

import frame_util as U
import light_util as L

F = np.float32
U32 = np.uint32
H = [F(0.375), F(0.25), F(0.0625)]


def dot(a, b):
    r = F(0.0) + a[..., 0] * b[..., 0]
    r = r + a[..., 1] * b[..., 1]
    return r + a[..., 2] * b[..., 2]


def constants(iterations, sigma_color, sigma_plane):
    """invPlane and invColor2[k], in float32."""
    with np.errstate(all="ignore"):
        inv_plane = F(1.0) / F(sigma_plane)
        inv_color2 = []
        for k in range(iterations):
            s = F(sigma_color) * F(2.0 ** -k)
            inv_color2.append(F(1.0) / (s * s))
    return inv_plane, inv_color2


class Model:
    """mrt.host.denoise_features / denoise_filter, from the contract."""

    @staticmethod
    def denoise_features(slot_to_id, primary_rays, primary_results, normals, material, num_pixels, guide=None, albedo=None):
        p = np.asarray(slot_to_id, np.int32).reshape(-1)
        rays = np.ascontiguousarray(primary_rays, F).reshape(-1, 8)
        res = np.ascontiguousarray(primary_results).view(np.int32).reshape(-1, 4)
        normals, material = np.asarray(normals, F).reshape(-1, 3), np.asarray(material).view(U32).reshape(-1)
        guide = np.zeros((num_pixels, 8), F) if guide is None else guide
        albedo = np.zeros((num_pixels, 4), F) if albedo is None else albedo
        keep = np.flatnonzero((p >= 0) & (p < num_pixels))
        p, rays, ids, t = p[keep], rays[keep], res[keep, 0], np.ascontiguousarray(res[keep, 1]).view(F)
        hit = (ids >= 0) & (ids < len(material))
        guide[p[~hit]] = 0.0
        albedo[p[~hit]] = 1.0
        p, rays, ids, t = p[hit], rays[hit], ids[hit], t[hit]
        with np.errstate(all="ignore"):
            n, d = normals[ids], rays[:, 4:7]
            nf = np.where((dot(n, d) > 0)[:, None], -n, n)
            x = rays[:, 0:3] + d * t[:, None]
        rec = np.zeros((len(p), 8), F)
        rec[:, 0:3], rec[:, 3], rec[:, 4:7] = nf, 1.0, x
        guide[p] = rec
        alb = L.from_abgr(material[ids])
        alb[:, 3] = 1.0
        albedo[p] = alb
        return guide, albedo

    @staticmethod
    def denoise_filter(image, guide, albedo, width, height, iterations=5, sigma_color=1.0, sigma_plane=1.0,
                       normal_squarings=7, want_image=True, want_pixels=True):
        w, h = width, height
        img = np.ascontiguousarray(image, F).reshape(h, w, 4)
        g = np.ascontiguousarray(guide, F).reshape(h, w, 8)
        alb = np.ascontiguousarray(albedo, F).reshape(h, w, 4)[..., :3]
        hit = g[..., 3] != 0
        n_p, x_p = g[..., 0:3], g[..., 4:7]
        inv_plane, inv_color2 = constants(iterations, sigma_color, sigma_plane)
        ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
        with np.errstate(all="ignore"):
            c = np.where(hit[..., None], np.where(alb > 0, img[..., :3] / alb, F(0.0)), img[..., :3]).astype(F)
            for k in range(iterations):
                s = 1 << k
                total, wsum = np.zeros((h, w, 3), F), np.zeros((h, w), F)
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        qy, qx = ys + dy * s, xs + dx * s
                        inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                        qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                        gq, cq = g[qy, qx], c[qy, qx]
                        use = inside & (gq[..., 3] != 0)
                        a = dot(n_p, gq[..., 0:3])
                        a = np.where(a > 0, a, F(0.0))
                        for _ in range(normal_squarings):
                            a = a * a
                        dpl = dot(n_p, gq[..., 4:7] - x_p) * inv_plane
                        wz = F(1.0) / (F(1.0) + dpl * dpl)
                        e = cq - c
                        dc2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
                        wc = F(1.0) / (F(1.0) + dc2 * inv_color2[k])
                        wt = (((H[abs(dx)] * H[abs(dy)]) * a) * wz) * wc
                        total = np.where(use[..., None], total + wt[..., None] * cq, total)
                        wsum = np.where(use, wsum + wt, wsum)
                c = np.where((hit & (wsum > 0))[..., None], total / wsum[..., None], c).astype(F)
            r = np.where(hit[..., None], c * alb, c).astype(F)
        out = np.concatenate([r, img[..., 3:4]], axis=2).reshape(-1, 4) if want_image else None
        px = L.to_abgr(np.concatenate([r, np.ones((h, w, 1), F)], axis=2).reshape(-1, 4)) if want_pixels else None
        return out, px


def same_floats(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(U.same_bits_or_nan(a.view(F), b.view(F)).all())


# ---- the tables ---------------------------------------------------------------------------------------
# A few normals many pixels share (so that weights are not all 0), the edges among them: a pair at
# exactly 90 degrees, one beyond, zero, NaN.
NORMALS = np.array([(0, 0, 1), (0, 0, 1), (0, 0, 1), (1, 0, 0), (0, 0, -1), (0.6, 0, 0.8), (0, 0, 0), (0, 1, 0),
                    (np.nan, 0, 1), (-0.6, 0, 0.8)], F)
GUIDE_KINDS = ["hits", "misses", "checker", "mixed", "zero-normals"]
FRAMES = [(1, 1), (1, 7), (7, 1), (3, 3), (17, 15), (97, 83)]


def make_guide(w, h, kind, rng):
    """float32 [w*h, 8]: the normals of the kind, hit flags, positions near the plane z = 0.05 * x."""
    n = w * h
    ys, xs = np.divmod(np.arange(n), w)
    g = np.zeros((n, 8), F)
    pick = rng.integers(0, len(NORMALS), n) if kind == "mixed" else np.zeros(n, int)
    if kind == "zero-normals":
        pick[:] = 6
    g[:, 0:3] = NORMALS[pick]
    g[:, 3] = 1.0
    g[:, 4], g[:, 5] = xs * F(0.1), ys * F(0.1)
    g[:, 6] = (F(0.05) * xs + rng.normal(size=n) * 0.01).astype(F)
    if kind == "misses":
        g[:] = 0.0
    if kind in ("checker", "mixed"):
        g[(xs + ys) % 2 == 1] = 0.0
    return g


def make_albedo(n, rng):
    """Channels of 0, 1/255 and 1 (the bytes 0, 1, 255 through fromABGR), w = 1."""
    a = L.from_abgr(np.array([0x000000, 0x010101, 0xFFFFFF], U32))[rng.integers(0, 3, (n, 3)), np.arange(3)[None, :]]
    return np.concatenate([a, np.ones((n, 1), F)], axis=1).astype(F)


def make_image(n, rng, edges=True):
    """Colours in [0, 1.5) with, where edges, entries of 0, a denormal, 1e30, inf and NaN; w random."""
    img = (rng.random((n, 4)) * 1.5).astype(F)
    if edges:
        for k, v in enumerate((0.0, 1e-39, 1e30, np.inf, np.nan)):
            at = np.arange(k, n, 11 + 2 * k)
            img[at, (at + k) % 3] = v
    return img


def make_case(w, h, kind, seed, edges=True):
    rng = np.random.default_rng(seed)
    return make_image(w * h, rng, edges), make_guide(w, h, kind, rng), make_albedo(w * h, rng)


@functools.lru_cache(maxsize=None)
def feature_tables():
    """(normals float32 [8, 3], material uint32 [8]), read-only."""
    normals = np.array([(0, 0, 1), (0, 0, -1), (0, 0, 0), (np.nan, 0, 1), (1, 0, 0), (0.6, 0, 0.8), (0, 1e-39, 1), (0, -1, 0)], F)
    material = np.array([0xFF000000, 0xFF010101, 0xFFFFFFFF, 0x00BF7F3F, 0xFF00FF01, 0x12345678, 0xFFBFBFBF, 0xFF0100FF], U32)
    normals.setflags(write=False)
    material.setflags(write=False)
    return normals, material


def feature_inputs(num_slots, num_pixels, seed):
    """(slot_to_id, rays, results) of num_slots primaries over num_pixels pixels: distinct pixels, ids
    -1, 0..7, 8 (outside the tables) and a huge one, t of 0, a denormal, inf and NaN among them, and
    some slots whose pixel is -1 or num_pixels (skipped)."""
    rng = np.random.default_rng(seed)
    s2i = rng.permutation(num_pixels)[:num_slots].astype(np.int32)
    s2i[3::17] = -1
    s2i[5::19] = num_pixels
    rays = rng.normal(size=(num_slots, 8)).astype(F)
    rays[1::7, 1] = 1e-39
    res = np.zeros((num_slots, 4), np.int32)
    res[:, 0] = rng.integers(-1, 9, num_slots)
    res[2::23, 0] = 0x7FFFFFFF
    t = rng.uniform(0.0, 5.0, num_slots).astype(F)
    for k, v in enumerate((0.0, 1e-39, np.inf, np.nan)):
        t[k::13] = v
    res[:, 1] = t.view(np.int32)
    res[:, 2:] = 7   # padding nobody reads
    return s2i, rays, res
