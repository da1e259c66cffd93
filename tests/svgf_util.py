"""Shared by tests/test_svgf.py, tests/test_gpu_svgf.py and the svgf stream tables: an independent
model of the variance-guided filter and the tables all are checked on.

The model restates the contract of mrt_svgf_accumulate / mrt_svgf_filter from the text of
include/mrt_svgf.h (and, for the steps that header takes over, include/mrt_temporal.h), not from
csrc/svgf_common.hpp. It works on numpy float32 arrays over all pixels at once, one IEEE operation
at a time in the documented order; the taps of a window are shifted views of the frame, visited dy
outer and dx inner. toABGR is light_util's. `Model` has mrt.host's two signatures.
"""
import numpy as np

import denoise_util as D
import light_util as L
import temporal_util as TU

F = np.float32
U32 = np.uint32
dot = D.dot
same_floats = D.same_floats
LUM = (F(0.2126), F(0.7152), F(0.0722))


def lum(c):
    r = F(0.0) + LUM[0] * c[..., 0]
    r = r + LUM[1] * c[..., 1]
    return r + LUM[2] * c[..., 2]


def pos(x):
    return np.where(x > 0, x, F(0.0)).astype(F)


class Model:
    """mrt.host.svgf_accumulate / svgf_filter, from the contract."""

    @staticmethod
    def svgf_accumulate(image, guide, albedo, width, height, prev_guide=None, prev_history=None, prev_moments=None,
                        prev_world_to_screen=None, prev_subpixel=(0.5, 0.5), prev_position=None, max_history=32,
                        normal_cos=0.8, sigma_plane=1.0, want_image=True, want_pixels=True, have_prev=None):
        w, h = width, height
        n = w * h
        img = np.ascontiguousarray(image, F).reshape(n, 4)
        g = np.ascontiguousarray(guide, F).reshape(n, 8)
        alb = np.ascontiguousarray(albedo, F).reshape(n, 4)[:, :3]
        if have_prev is None:
            have_prev = prev_guide is not None and prev_history is not None and prev_moments is not None
        hit = g[:, 3] != 0
        with np.errstate(all="ignore"):
            c = np.where(hit[:, None], np.where(alb > 0, img[:, :3] / alb, F(0.0)), img[:, :3]).astype(F)
            l1 = lum(c)
            l2 = l1 * l1
            out, length = c.copy(), np.ones(n, F)
            m1, m2 = l1.copy(), l2.copy()
            if have_prev:
                pg = np.ascontiguousarray(prev_guide, F).reshape(n, 8)
                ph = np.ascontiguousarray(prev_history, F).reshape(n, 4)
                pm = np.ascontiguousarray(prev_moments, F).reshape(n, 4)
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
                total, mtotal, wsum = np.zeros((n, 4), F), np.zeros((n, 2), F), np.zeros(n, F)
                for j in (0, 1):
                    for i in (0, 1):
                        qx, qy = ix + i, iy + j
                        inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                        bw = (ax if i else F(1.0) - ax) * (ay if j else F(1.0) - ay)
                        q = np.clip(qy, 0, h - 1) * w + np.clip(qx, 0, w - 1)
                        gq = pg[q]
                        use = ok & inside & (bw != 0) & (gq[:, 3] != 0)
                        use &= dot(g[:, 0:3], gq[:, 0:3]) >= F(normal_cos)
                        use &= np.abs(dot(gq[:, 0:3], gq[:, 4:7] - xw)) * inv_plane <= 1
                        total = np.where(use[:, None], total + bw[:, None] * ph[q], total)
                        mtotal = np.where(use[:, None], mtotal + bw[:, None] * pm[q, :2], mtotal)
                        wsum = np.where(use, wsum + bw, wsum)
                found = ok & (wsum > 0)
                hst, hm = total / wsum[:, None], mtotal / wsum[:, None]
                n1 = hst[:, 3] + F(1.0)
                cap = np.where(n1 < F(max_history), n1, F(max_history)).astype(F)
                alpha = F(1.0) / cap
                out = np.where(found[:, None], hst[:, :3] + (c - hst[:, :3]) * alpha[:, None], c).astype(F)
                m1 = np.where(found, hm[:, 0] + (l1 - hm[:, 0]) * alpha, l1).astype(F)
                m2 = np.where(found, hm[:, 1] + (l2 - hm[:, 1]) * alpha, l2).astype(F)
                length = np.where(found, cap, F(1.0)).astype(F)
            r = np.where(hit[:, None], out * alb, out).astype(F)
        history = np.concatenate([out, length[:, None]], axis=1).astype(F)
        moments = np.stack([m1, m2, np.zeros(n, F), length], axis=1).astype(F)
        image_out = np.concatenate([r, img[:, 3:4]], axis=1) if want_image else None
        px = L.to_abgr(np.concatenate([r, np.ones((n, 1), F)], axis=1)) if want_pixels else None
        return history, moments, image_out, px

    @staticmethod
    def svgf_filter(image, guide, albedo, moments, width, height, iterations=5, sigma_luminance=4.0, sigma_plane=1.0,
                    normal_squarings=7, want_image=True, want_pixels=True, want_variance=True):
        w, h = width, height
        img = np.ascontiguousarray(image, F).reshape(h, w, 4)
        g = np.ascontiguousarray(guide, F).reshape(h, w, 8)
        alb = np.ascontiguousarray(albedo, F).reshape(h, w, 4)[..., :3]
        mom = np.ascontiguousarray(moments, F).reshape(h, w, 4)
        hit = g[..., 3] != 0
        n_p, x_p = g[..., 0:3], g[..., 4:7]
        ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]

        def taps(radius, step):
            for dy in range(-radius, radius + 1):
                for dx in range(-radius, radius + 1):
                    qy, qx = ys + dy * step, xs + dx * step
                    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                    yield dx, dy, np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1), inside

        def geometry(gq):
            a = dot(n_p, gq[..., 0:3])
            a = np.where(a > 0, a, F(0.0))
            for _ in range(normal_squarings):
                a = a * a
            dpl = dot(n_p, gq[..., 4:7] - x_p) * inv_plane
            return a, F(1.0) / (F(1.0) + dpl * dpl)

        with np.errstate(all="ignore"):
            inv_plane = F(1.0) / F(sigma_plane)
            sl2 = F(sigma_luminance) * F(sigma_luminance)
            c = np.where(hit[..., None], np.where(alb > 0, img[..., :3] / alb, F(0.0)), img[..., :3]).astype(F)
            # 1. the variance launch
            m1, m2, length = mom[..., 0], mom[..., 1], mom[..., 3]
            own = pos(m2 - m1 * m1)
            s1, s2, wsum = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
            for dx, dy, qy, qx, inside in taps(3, 1):
                gq, mq = g[qy, qx], mom[qy, qx]
                use = inside & (gq[..., 3] != 0)
                a, wz = geometry(gq)
                wt = a * wz
                s1 = np.where(use, s1 + wt * mq[..., 0], s1)
                s2 = np.where(use, s2 + wt * mq[..., 1], s2)
                wsum = np.where(use, wsum + wt, wsum)
            scale = F(4.0) / length
            M1, M2 = s1 / wsum, s2 / wsum
            spatial = np.where(wsum > 0, pos(M2 - M1 * M1) * scale, own * scale)
            v = np.where(hit, np.where(length >= 4, own, spatial), F(0.0)).astype(F)
            # 2. the iterations
            for k in range(iterations):
                s = 1 << k
                gs, gv = np.zeros((h, w), F), np.zeros((h, w), F)
                for dx, dy, qy, qx, inside in taps(1, 1):
                    use = inside & (g[qy, qx][..., 3] != 0)
                    gw = (F(0.25), F(0.125), F(0.0625))[abs(dx) + abs(dy)]
                    gv = np.where(use, gv + gw * v[qy, qx], gv)
                    gs = np.where(use, gs + gw, gs)
                vt = np.where(gs > 0, gv / gs, v)
                inv_l = F(1.0) / (sl2 * vt + F(1e-8))
                lp = lum(c)
                total, sv, wsum = np.zeros((h, w, 3), F), np.zeros((h, w), F), np.zeros((h, w), F)
                for dx, dy, qy, qx, inside in taps(2, s):
                    gq, cq, vq = g[qy, qx], c[qy, qx], v[qy, qx]
                    use = inside & (gq[..., 3] != 0)
                    a, wz = geometry(gq)
                    dl = lum(cq) - lp
                    wl = F(1.0) / (F(1.0) + (dl * dl) * inv_l)
                    wt = (((D.H[abs(dx)] * D.H[abs(dy)]) * a) * wz) * wl
                    total = np.where(use[..., None], total + wt[..., None] * cq, total)
                    sv = np.where(use, sv + (wt * wt) * vq, sv)
                    wsum = np.where(use, wsum + wt, wsum)
                take = hit & (wsum > 0)
                c = np.where(take[..., None], total / wsum[..., None], c).astype(F)
                v = np.where(take, sv / (wsum * wsum), v).astype(F)
            r = np.where(hit[..., None], c * alb, c).astype(F)
        out = np.concatenate([r, img[..., 3:4]], axis=2).reshape(-1, 4) if want_image else None
        px = L.to_abgr(np.concatenate([r, np.ones((h, w, 1), F)], axis=2).reshape(-1, 4)) if want_pixels else None
        return out, px, (v.reshape(-1).copy() if want_variance else None)


# ---- the tables ---------------------------------------------------------------------------------------
FRAMES = TU.FRAMES + [(3, 2)]     # the temporal tables' sizes, and one that every window and stencil overhangs on all sides
GUIDE_KINDS = TU.GUIDE_KINDS
MAX_HISTORIES = TU.MAX_HISTORIES
ITERATIONS = [0, 1, 2, 3, 4, 5]


def make_moments(n, rng):
    """Moments (m1, m2, 0, N): m1 and m2 in [0, 1.5) with the image table's edge values (0, a
    denormal, 1e30, inf, NaN; m2 below m1 * m1 among them, which pos() clips), lengths 1 .. 8 so that
    both sides of N >= 4 are common, with a 0, a NaN and an infinity among them."""
    m = D.make_image(n, rng)
    m[:, 2] = 0.0
    m[:, 3] = rng.integers(1, 9, n).astype(F)
    for k, v in enumerate((0.0, np.nan, np.inf, 3.0, 4.0)):
        m[k + 2::29, 3] = v
    return m


def make_accumulate(w, h, kind, seed, **kw):
    """TU.make_frame's keyword arguments with the previous moments."""
    args = TU.make_frame(w, h, kind, seed, **kw)
    if args["have_prev"]:
        args["prev_moments"] = make_moments(w * h, np.random.default_rng(seed + 70))
    return args


def make_filter(w, h, kind, seed, sigma_luminance=4.0):
    """Keyword arguments of svgf_filter for one call of the table."""
    image, guide, albedo = D.make_case(w, h, kind, seed)
    return dict(image=image, guide=guide, albedo=albedo, moments=make_moments(w * h, np.random.default_rng(seed + 71)), width=w,
                height=h, sigma_luminance=sigma_luminance, sigma_plane=0.05, normal_squarings=2)
