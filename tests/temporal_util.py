"""Shared by tests/test_temporal.py, tests/test_gpu_temporal.py and the temporal stream tables: an
independent model of the temporal accumulation and the tables all are checked on.

The model restates the contract of mrt_temporal_motion / mrt_temporal_accumulate from the text of
include/mrt_temporal.h, not from csrc/temporal_common.hpp. It works on numpy float32 arrays over
all slots or pixels at once, one IEEE operation at a time in the documented order; the four taps
are four gathers, visited j outer and i inner. fromABGR / toABGR are light_util's. `Model` has
mrt.host's two signatures.
"""
import numpy as np

import denoise_util as D
import light_util as L

F = np.float32
U32 = np.uint32
dot = D.dot


class Model:
    """mrt.host.temporal_motion / temporal_accumulate, from the contract."""

    @staticmethod
    def temporal_motion(slot_to_id, primary_rays, primary_results, triangles, vertices, prev_vertices, num_pixels,
                        prev_position=None):
        p = np.asarray(slot_to_id, np.int32).reshape(-1)
        rays = np.ascontiguousarray(primary_rays, F).reshape(-1, 8)
        res = np.ascontiguousarray(primary_results).view(np.int32).reshape(-1, 4)
        tri = np.asarray(triangles, np.int32).reshape(-1, 3)
        v, pv = np.asarray(vertices, F).reshape(-1, 3), np.asarray(prev_vertices, F).reshape(-1, 3)
        out = np.zeros((num_pixels, 4), F) if prev_position is None else prev_position
        keep = np.flatnonzero((p >= 0) & (p < num_pixels))
        p, rays, ids, t = p[keep], rays[keep], res[keep, 0], np.ascontiguousarray(res[keep, 1]).view(F)
        hit = (ids >= 0) & (ids < len(tri))
        idx = tri[np.where(hit, ids, 0)] if len(tri) else np.zeros((len(ids), 3), np.int32)
        hit &= ((idx >= 0) & (idx < len(v))).all(axis=1)
        out[p[~hit]] = 0.0
        p, rays, idx, t = p[hit], rays[hit], idx[hit], t[hit]
        with np.errstate(all="ignore"):
            x = rays[:, 0:3] + rays[:, 4:7] * t[:, None]
            v0, v1, v2 = v[idx[:, 0]], v[idx[:, 1]], v[idx[:, 2]]
            q0, q1, q2 = pv[idx[:, 0]], pv[idx[:, 1]], pv[idx[:, 2]]
            e0, e1, r = v1 - v0, v2 - v0, x - v0
            d00, d01, d11, d20, d21 = dot(e0, e0), dot(e0, e1), dot(e1, e1), dot(r, e0), dot(r, e1)
            den = d00 * d11 - d01 * d01
            b1 = (d11 * d20 - d01 * d21) / den
            b2 = (d00 * d21 - d01 * d20) / den
            b0 = (F(1.0) - b1) - b2
            moved = (q0 * b0[:, None] + q1 * b1[:, None]) + q2 * b2[:, None]
        rec = np.ones((len(p), 4), F)
        rec[:, 0:3] = np.where((den > 0)[:, None], moved, x)
        out[p] = rec
        return out

    @staticmethod
    def temporal_accumulate(image, guide, albedo, width, height, prev_guide=None, prev_history=None,
                            prev_world_to_screen=None, prev_subpixel=(0.5, 0.5), prev_position=None, max_history=32,
                            normal_cos=0.8, sigma_plane=1.0, want_image=True, want_pixels=True, have_prev=None):
        w, h = width, height
        n = w * h
        img = np.ascontiguousarray(image, F).reshape(n, 4)
        g = np.ascontiguousarray(guide, F).reshape(n, 8)
        alb = np.ascontiguousarray(albedo, F).reshape(n, 4)[:, :3]
        have_prev = (prev_guide is not None and prev_history is not None) if have_prev is None else have_prev
        hit = g[:, 3] != 0
        with np.errstate(all="ignore"):
            c = np.where(hit[:, None], np.where(alb > 0, img[:, :3] / alb, F(0.0)), img[:, :3]).astype(F)
            out, length = c.copy(), np.ones(n, F)
            if have_prev:
                pg = np.ascontiguousarray(prev_guide, F).reshape(n, 8)
                ph = np.ascontiguousarray(prev_history, F).reshape(n, 4)
                m = np.asarray(prev_world_to_screen, F).reshape(16)
                ok = hit.copy()
                xw = g[:, 4:7]
                if prev_position is not None:
                    pp = np.ascontiguousarray(prev_position, F).reshape(n, 4)
                    ok &= pp[:, 3] != 0
                    xw = pp[:, 0:3]

                def clip(i):
                    r = F(0.0) + m[i] * xw[:, 0]
                    r = r + m[4 + i] * xw[:, 1]
                    r = r + m[8 + i] * xw[:, 2]
                    return r + m[12 + i] * F(1.0)
                cx, cy, cw = clip(0), clip(1), clip(3)
                ok &= cw > 0
                sx = ((cx / cw + F(1.0)) * F(0.5)) * F(w) - F(prev_subpixel[0])
                sy = ((cy / cw + F(1.0)) * F(0.5)) * F(h) - F(prev_subpixel[1])
                ok &= (sx > -1) & (sx < w) & (sy > -1) & (sy < h)
                sx, sy = np.where(ok, sx, F(0.0)), np.where(ok, sy, F(0.0))
                fx, fy = np.floor(sx), np.floor(sy)
                ix, iy = fx.astype(np.int64), fy.astype(np.int64)
                ax, ay = sx - fx, sy - fy
                inv_plane = F(1.0) / F(sigma_plane)
                total, wsum = np.zeros((n, 4), F), np.zeros(n, F)
                for j in (0, 1):
                    for i in (0, 1):
                        qx, qy = ix + i, iy + j
                        inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                        bw = (ax if i else F(1.0) - ax) * (ay if j else F(1.0) - ay)
                        q = np.clip(qy, 0, h - 1) * w + np.clip(qx, 0, w - 1)
                        gq, hq = pg[q], ph[q]
                        use = ok & inside & (bw != 0) & (gq[:, 3] != 0)
                        use &= dot(g[:, 0:3], gq[:, 0:3]) >= F(normal_cos)
                        use &= np.abs(dot(gq[:, 0:3], gq[:, 4:7] - xw)) * inv_plane <= 1
                        total = np.where(use[:, None], total + bw[:, None] * hq, total)
                        wsum = np.where(use, wsum + bw, wsum)
                found = ok & (wsum > 0)
                hst = total / wsum[:, None]
                n1 = hst[:, 3] + F(1.0)
                cap = np.where(n1 < F(max_history), n1, F(max_history)).astype(F)
                alpha = F(1.0) / cap
                blended = hst[:, :3] + (c - hst[:, :3]) * alpha[:, None]
                out = np.where(found[:, None], blended, c).astype(F)
                length = np.where(found, cap, F(1.0)).astype(F)
            r = np.where(hit[:, None], out * alb, out).astype(F)
        history = np.concatenate([out, length[:, None]], axis=1).astype(F)
        image_out = np.concatenate([r, img[:, 3:4]], axis=1) if want_image else None
        px = L.to_abgr(np.concatenate([r, np.ones((n, 1), F)], axis=1)) if want_pixels else None
        return history, image_out, px


same_floats = D.same_floats


# ---- the tables ---------------------------------------------------------------------------------------
FRAMES = [(1, 1), (1, 7), (7, 1), (33, 9), (97, 83)]
GUIDE_KINDS = ["hits", "misses", "checker", "mixed", "zero-normals"]
MAX_HISTORIES = [1, 2, 32]


def screen_matrix(w, h, scale=1.0, shift=(0.0, 0.0), subpixel=(0.5, 0.5), wz=0.0):
    """Column-major float32 [16]: the position (X, Y, Z) lands at sx = X * scale + shift[0], sy = Y *
    scale + shift[1] given the same subpixel, with clip.w = 1 + wz * Z. With w, h and scale powers
    of two and a shift of quarter pixels every term is exact."""
    m = np.zeros((4, 4), np.float64)
    m[0, 0], m[0, 3] = 2.0 * scale / w, 2.0 * (shift[0] + subpixel[0]) / w - 1.0
    m[1, 1], m[1, 3] = 2.0 * scale / h, 2.0 * (shift[1] + subpixel[1]) / h - 1.0
    m[2, 2] = 1.0
    m[3, 2], m[3, 3] = wz, 1.0
    return np.ascontiguousarray(m.T.reshape(16), F)


def make_history(n, rng):
    """Demodulated colours in [0, 1.5) with the image table's edge values, lengths 1 .. 40 (above
    the largest maxHistory of the tables) with a 0, a NaN and an infinity among them."""
    hst = D.make_image(n, rng)
    hst[:, 3] = rng.integers(1, 41, n).astype(F)
    for k, v in enumerate((0.0, np.nan, np.inf)):
        hst[k + 2::29, 3] = v
    return hst


def make_frame(w, h, kind, seed, max_history=32, have_prev=True, moving=False, shift=(0.3, -0.6)):
    """Keyword arguments of temporal_accumulate for one call of the table: this frame's image,
    guide and albedo, the previous guide (of the same kind, so that normals agree often) and
    history, a matrix that takes a guide's position (0.1 x, 0.1 y, z) back to its pixel plus
    `shift`, with a clip.w that falls a little with z, and where `moving` a prevPosition table
    with the edges: w == 0, NaN, behind the camera, sx at exactly -1, just inside, w - 1 and w."""
    rng = np.random.default_rng(seed + 7)
    n = w * h
    image, guide, albedo = D.make_case(w, h, kind, seed)
    kw = dict(image=image, guide=guide, albedo=albedo, width=w, height=h, max_history=max_history, normal_cos=0.9,
              sigma_plane=0.05, have_prev=have_prev)
    if not have_prev:
        return kw
    prev_guide = D.make_guide(w, h, kind, rng)
    if kind in ("hits", "mixed"):
        prev_guide[1::5, 0:3] = D.NORMALS[rng.integers(0, len(D.NORMALS), len(prev_guide[1::5]))]
        prev_guide[2::7, 3] = 0.0
    sub = (0.25, 0.875)
    kw.update(prev_guide=prev_guide, prev_history=make_history(n, rng), prev_subpixel=sub,
              prev_world_to_screen=screen_matrix(w, h, 10.0, shift, sub, wz=-0.02))
    if moving:
        pp = np.concatenate([guide[:, 4:7], np.ones((n, 1), F)], axis=1).astype(F)
        pp[:, 0:2] += (rng.random((n, 2)) * 0.2 - 0.1).astype(F)
        pp[:, 2] = guide[:, 6]
        pp[3::13, 3] = 0.0
        pp[5::17, 1] = np.nan
        pp[7::19, 2] = 60.0           # clip.w = 1 - 1.2 < 0
        pp[9::23, 2] = 50.0           # clip.w = 0
        for k, sx in enumerate((-1.0, -0.999, w - 1.0, float(w), w - 0.001)):
            at = np.arange(11 + k, n, 31)
            pp[at, 0] = F((sx - shift[0]) / 10.0)
            pp[at, 2] = 0.0
        kw["prev_position"] = pp
    return kw


def motion_inputs(num_slots, num_pixels, seed):
    """(slot_to_id, rays, results, triangles, vertices, prev_vertices): D.feature_inputs' slots over
    a table of 9 triangles, the edges among them: a zero-area one (den 0), a sliver whose den rounds
    below 0 or to 0, one with a NaN vertex, one with a vertex index outside the table, one negative."""
    s2i, rays, res = D.feature_inputs(num_slots, num_pixels, seed)
    rng = np.random.default_rng(seed + 1000)
    v = rng.normal(size=(24, 3)).astype(F)
    v[3] = v[4] = v[5]                                 # triangle 1: a point
    v[7] = v[6] + (v[8] - v[6]) * F(0.5) + F(1e-8)     # triangle 2: a sliver
    v[10, 1] = np.nan                                  # triangle 3
    tri = np.arange(24, dtype=np.int32).reshape(8, 3).copy()
    tri[4, 2] = 24                                     # outside
    tri[5, 0] = -1
    tri = np.concatenate([tri, np.array([[0, 5, 9]], np.int32)])
    res[:, 0] = np.random.default_rng(seed + 2000).integers(-1, 10, num_slots)
    res[2::23, 0] = 0x7FFFFFFF
    pv = (v * F(1.25) + rng.normal(size=v.shape).astype(F) * F(0.1)).astype(F)
    return s2i, rays, res, tri, v, pv
