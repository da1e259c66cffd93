"""The temporal accumulation on the CPU: mrth_temporal_motion and mrth_temporal_accumulate
(csrc/host/temporal.cpp over csrc/temporal_common.hpp), the CPU statements of mrt_temporal_motion /
mrt_temporal_accumulate, against the independent numpy model of tests/temporal_util.py, bit for bit
(a NaN equal to a NaN); known answers that are exact by construction; the running mean's error
bound; the reprojection through a rigid translation; the quality condition on the
floor-and-occluder scene; the plan (csrc/temporal_plan.cpp) through lib/temporal_driver; the host
functions as a stand-alone program under -fsanitize=address,undefined
(tests/cpp/temporal_driver.cpp; nothing is preloaded); world_to_screen; and the host argument
checks. None needs a device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mrt
import mrt.host
from mrt import _lib

import denoise_util as D
import oracle_lib as O
import path_util as P
import temporal_util as TU
import test_path as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gpu-ray-tracing_amd")
F = np.float32
DRIVER = os.path.join(PKG, "lib", "temporal_driver")


def same_result(got, want):
    assert TU.same_floats(got[0], want[0]), "history"
    assert (got[1] is None) == (want[1] is None) and (got[2] is None) == (want[2] is None)
    if want[1] is not None:
        assert TU.same_floats(got[1], want[1]), "image"
    if want[2] is not None:
        assert np.array_equal(got[2], want[2]), "pixels"


# ---------------------------------------------------------------- 1. the host statements against the model
@pytest.mark.parametrize("frame", TU.FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("kind", TU.GUIDE_KINDS)
def test_host_accumulate_equals_the_model(frame, kind):
    w, h = frame
    seen = {"found": 0, "nan": 0, "long": 0}
    for max_history in TU.MAX_HISTORIES:
        for have_prev, moving in ((False, False), (True, False), (True, True)):
            kw = TU.make_frame(w, h, kind, seed=w * 131 + h + max_history, max_history=max_history, have_prev=have_prev,
                               moving=moving)
            got = mrt.host.temporal_accumulate(**kw)
            want = TU.Model.temporal_accumulate(**kw)
            same_result(got, want)
            assert TU.same_floats(got[1][:, 3], kw["image"][:, 3])            # w is carried
            only_px = mrt.host.temporal_accumulate(want_image=False, **kw)
            neither = mrt.host.temporal_accumulate(want_image=False, want_pixels=False, **kw)
            assert only_px[1] is None and neither[1] is None and neither[2] is None
            assert np.array_equal(only_px[2], got[2]) and TU.same_floats(neither[0], got[0])
            length = got[0][:, 3]
            assert ((length >= 1) & (length <= max_history)).all()
            if not have_prev:
                assert (length == 1).all()
            seen["found"] += int((length > 1).sum())
            seen["long"] += int((length == max_history).sum()) if max_history > 1 else 0
            seen["nan"] += int(np.isnan(got[0]).sum())
    if kind == "misses":
        assert seen["found"] == 0
    elif w * h > 60 and kind != "zero-normals":
        assert seen["found"] > 0 and seen["long"] > 0 and seen["nan"] > 0   # the table reached the blend, the cap and a NaN


@pytest.mark.parametrize("shape", [(1, 1), (300, 400), (400, 400), (5000, 5003)], ids=str)
def test_host_motion_equals_the_model(shape):
    slots, pixels = shape
    s2i, rays, res, tri, v, pv = TU.motion_inputs(slots, pixels, seed=slots)
    sentinel = np.full((pixels, 4), 7.5, F)
    got = mrt.host.temporal_motion(s2i, rays, res, tri, v, pv, pixels, sentinel.copy())
    want = TU.Model.temporal_motion(s2i, rays, res, tri, v, pv, pixels, sentinel.copy())
    assert TU.same_floats(got, want)
    named = np.zeros(pixels, bool)
    named[s2i[(s2i >= 0) & (s2i < pixels)]] = True
    assert (got[~named] == 7.5).all() and np.isin(got[named, 3], (0.0, 1.0)).all()
    if slots > 1:
        ids = np.full(pixels, -99)
        keep = (s2i >= 0) & (s2i < pixels)
        ids[s2i[keep]] = res[keep, 0]
        assert (got[np.isin(ids, (4, 5, -1, 9, 0x7FFFFFFF))] == 0).all()   # a vertex index outside the table, a miss
        assert (got[ids == 0, 3] == 1).all() and np.isnan(got[ids == 3]).any()
        # the point-like triangle keeps x: den is 0
        at = np.flatnonzero(ids == 1)
        slot_of = {int(p): i for i, p in enumerate(s2i) if 0 <= p < pixels}
        for p in at[:5]:
            i = slot_of[int(p)]
            with np.errstate(all="ignore"):
                x = rays[i, 0:3] + rays[i, 4:7] * res[i, 1:2].view(F)
            assert TU.same_floats(got[p, :3], x)


# ---------------------------------------------------------------- 2. known answers, exact by construction
KW, KH = 64, 8


def plane(w=KW, h=KH, z=0.0, normal=(0.0, 0.0, 1.0)):
    """Pixel (px, py) sees the position (px, py, z): with screen_matrix(w, h) it reprojects to itself."""
    n = w * h
    ys, xs = np.divmod(np.arange(n), w)
    g = np.zeros((n, 8), F)
    g[:, 0:3], g[:, 3], g[:, 4], g[:, 5], g[:, 6] = normal, 1.0, xs, ys, z
    return g


def ones(n):
    return np.ones((n, 4), F)


def accumulate(impl, image, guide, prev_guide=None, prev_history=None, shift=(0.0, 0.0), albedo=None, **kw):
    n = KW * KH
    args = dict(prev_world_to_screen=TU.screen_matrix(KW, KH, 1.0, shift), max_history=32, normal_cos=0.9, sigma_plane=0.5)
    args.update(kw)
    return impl.temporal_accumulate(image, guide, ones(n) if albedo is None else albedo, KW, KH, prev_guide, prev_history, **args)


IMPLS = pytest.mark.parametrize("impl", [mrt.host, TU.Model], ids=["host", "model"])


@IMPLS
def test_known_answer_an_identity_reprojection_counts_the_frames(impl):
    n = KW * KH
    image = np.tile(np.array([0.25, 0.5, 0.75, 0.125], F), (n, 1))
    albedo = ones(n)
    albedo[:, :3] = np.array([191, 127, 255], F) * (F(1) / F(255))
    g, hst = plane(), None
    for frame in range(1, 7):
        hst, out, _ = accumulate(impl, image, g, g if hst is not None else None, hst, albedo=albedo, max_history=4)
        assert (hst[:, 3] == min(frame, 4)).all()
        assert np.array_equal(hst[:, :3], np.tile(hst[0, :3], (n, 1)))        # a constant stays one
        assert np.abs(out[:, :3] / image[:, :3] - 1.0).max() <= 2e-7 and np.array_equal(out[:, 3], image[:, 3])


@IMPLS
def test_known_answer_a_whole_pixel_shift_moves_the_history(impl):
    n = KW * KH
    rng = np.random.default_rng(5)
    prev = rng.random((n, 4)).astype(F)
    prev[:, 3] = 5.0
    image = np.zeros((n, 4), F)
    # the point pixel x sees now was seen through pixel x - 3 then
    hst, _, _ = accumulate(impl, image, plane(), plane(), prev, shift=(-3.0, 0.0))
    hst, prev = hst.reshape(KH, KW, 4), prev.reshape(KH, KW, 4)
    want = prev[:, :-3, :3] + (F(0.0) - prev[:, :-3, :3]) * (F(1.0) / F(6.0))
    assert np.array_equal(hst[:, 3:, :3], want) and (hst[:, 3:, 3] == 6).all()
    assert (hst[:, :3, 3] == 1).all() and (hst[:, :3, :3] == 0).all()         # the columns that enter the frame


@IMPLS
@pytest.mark.parametrize("fraction", [0.5, 0.25])
def test_known_answer_a_fraction_of_a_pixel_weights_two_taps(impl, fraction):
    n = KW * KH
    prev = np.zeros((n, 4), F)
    prev[:, 0] = np.arange(n) % KW          # a ramp in x: the bilinear value is x - fraction
    prev[:, 3] = 31.0
    hst, _, _ = accumulate(impl, np.zeros((n, 4), F), plane(), plane(), prev, shift=(-fraction, 0.0), max_history=1 << 20)
    hst = hst.reshape(KH, KW, 4)
    xs = np.arange(1, KW, dtype=F)
    want = (xs - F(fraction)) + (F(0.0) - (xs - F(fraction))) * (F(1.0) / F(32.0))
    assert np.array_equal(hst[:, 1:, 0], np.tile(want, (KH, 1))) and (hst[:, 1:, 3] == 32).all()
    # column 0 has one tap inside the frame: the weights are renormalised, the value is that tap's
    assert (hst[:, 0, 3] == 32).all() and (hst[:, 0, 0] == 0).all()


@IMPLS
def test_known_answer_nothing_crosses_a_right_angle_or_leaves_the_plane(impl):
    n = KW * KH
    prev = np.full((n, 4), 9.0, F)
    image = np.zeros((n, 4), F)
    wall = plane(normal=(1.0, 0.0, 0.0))
    hst, _, _ = accumulate(impl, image, plane(), wall, prev)
    assert (hst[:, 3] == 1).all() and (hst[:, :3] == 0).all()
    behind = plane(z=0.75)                  # the previous surface 0.75 off the point's plane, tolerance 0.5
    hst, _, _ = accumulate(impl, image, plane(), behind, prev)
    assert (hst[:, 3] == 1).all()
    hst, _, _ = accumulate(impl, image, plane(), plane(z=0.5), prev)          # exactly at the tolerance: taken
    assert (hst[:, 3] == 10).all()
    tilted = plane(normal=(0.0, 0.6, 0.8))  # cos 0.8 < 0.9
    hst, _, _ = accumulate(impl, image, plane(), tilted, prev)
    assert (hst[:, 3] == 1).all()
    hst, _, _ = accumulate(impl, image, plane(), tilted, prev, normal_cos=0.8)
    assert (hst[:, 3] > 1).any()


@IMPLS
def test_known_answer_misses_neither_receive_nor_give(impl):
    n = KW * KH
    rng = np.random.default_rng(6)
    image = rng.random((n, 4)).astype(F)
    prev = np.full((n, 4), 3.0, F)
    g, pg = plane(), plane()
    odd = (np.arange(n) % KW) % 2 == 1
    g[odd & (np.arange(n) < n // 2)] = 0.0       # current misses in the upper half
    pg[odd & (np.arange(n) >= n // 2)] = 0.0     # previous misses in the lower half
    albedo = np.full((n, 4), 0.5, F)
    hst, out, _ = accumulate(impl, image, g, pg, prev, albedo=albedo)
    miss = g[:, 3] == 0
    assert (hst[miss, 3] == 1).all() and np.array_equal(hst[miss, :3], image[miss, :3])
    assert np.array_equal(out[miss], image[miss])                              # not demodulated, not blended
    gave_none = (pg[:, 3] == 0) & ~miss
    assert (hst[gave_none, 3] == 1).all() and (hst[~miss & ~gave_none, 3] == 4).all()
    # half a pixel off, a hit pixel between a hit and a miss takes the hit's history alone
    hst, _, _ = accumulate(impl, image, g, pg, prev, shift=(-0.5, 0.0), albedo=albedo)
    lower = ~miss & (np.arange(n) >= n // 2) & (np.arange(n) % KW > 0)
    assert (hst[lower, 3] == 4).all() and np.isfinite(hst).all()


@IMPLS
def test_known_answer_a_history_of_one_returns_the_frame(impl):
    n = KW * KH
    image, guide, albedo = D.make_case(KW, KH, "mixed", seed=8)
    prev = TU.make_history(n, np.random.default_rng(9))
    with_prev = accumulate(impl, image, guide, guide, prev, albedo=albedo, max_history=1, shift=(-0.25, 0.5))
    without = accumulate(impl, image, guide, albedo=albedo, max_history=1)
    found = ~np.isnan(with_prev[0][:, :3]).any(axis=1) | np.isnan(without[0][:, :3]).any(axis=1)
    assert (with_prev[0][:, 3] == 1).all()
    # hst + (c - hst) * 1 is c wherever hst is finite and the difference does not round
    exact = np.isfinite(prev[:, :3]).all(axis=1) & found
    assert exact.sum() > n // 4
    near = np.isclose(with_prev[0][exact, :3], without[0][exact, :3], rtol=1e-6, atol=1e-6, equal_nan=True)
    assert near.all()
    zero = np.zeros((n, 4), F)
    zero[:, 3] = 7.0
    a = accumulate(impl, image, guide, guide, zero, albedo=albedo, max_history=1)       # hst = 0: c - 0 + 0 is c, bit for bit
    assert TU.same_floats(a[0], without[0]) and TU.same_floats(a[1], without[1]) and np.array_equal(a[2], without[2])


# ---------------------------------------------------------------- 3. the running mean
@IMPLS
def test_the_running_mean_is_the_mean_within_the_rounding_bound(impl):
    """N identity-reprojected frames of independent values in [0, 1]: history = hst + (c - hst) / N
    rounds three times a step, each by at most 2^-24 of a value no larger than the largest input, so
    the result is within 4 N 2^-24 max|value| of the float64 mean."""
    n, N = KW * KH, 32
    rng = np.random.default_rng(10)
    frames = rng.random((N, n, 4)).astype(F)
    g, hst = plane(), None
    for k in range(N):
        hst, _, _ = accumulate(impl, frames[k], g, g if k else None, hst, max_history=N)
    mean = frames[:, :, :3].astype(np.float64).mean(axis=0)
    err = float(np.abs(hst[:, :3].astype(np.float64) - mean).max())
    bound = 4 * N * 2.0 ** -24 * float(frames.max())
    print(f"running mean of {N} frames: max error {err:.3g}, bound {bound:.3g}")
    assert (hst[:, 3] == N).all() and err <= bound


# ---------------------------------------------------------------- 4. motion through a rigid translation
def test_motion_through_a_rigid_translation_gives_back_the_shifted_point():
    """random1500 translated rigidly by s, the primary hits of a small frame by the oracle: the
    previous position of a hit at x is x - s. Error: the five dot products carry a relative error
    of 3 * 2^-24 each of |e|^2 (three products and three sums of terms of one sign or bounded by
    |e|^2), den loses another few through its cancellation, which the division by den amplifies by
    d00 d11 / den = 1 / sin^2 of the corner angle. So a barycentric coordinate is off by about
    16 * 2^-24 / sin^2, and the point by that times the triangle's extent E, plus 4 ulp of the
    coordinates' magnitude M from the interpolation itself: the bound is (16 E / sin^2 + 4 M) 2^-24,
    evaluated per hit; triangles with sin^2 < 1e-3 are left out of the maximum and only checked
    to land within their extent."""
    scene = mrt.Scene.synthetic("random", 1500, 1)
    v, tri, _ = scene.arrays()
    nodes, woop, tidx = mrt.Bvh.build(scene).buffers()
    cam, _ = scene.camera()
    w, h = 48, 32
    rays, s2i = mrt.primary_rays(cam, w, h)
    res = O.trace(rays, nodes, woop, tidx)[0]
    shift = np.array([0.375, -1.25, 2.5], F)
    pv = (v - shift).astype(F)
    got = mrt.host.temporal_motion(s2i, rays, res, tri, v, pv, w * h)
    assert TU.same_floats(got, TU.Model.temporal_motion(s2i, rays, res, tri, v, pv, w * h))
    ids, t = res[:, 0], np.ascontiguousarray(res[:, 1]).view(F)
    hit = ids >= 0
    assert hit.sum() > 200 and (got[s2i[~hit]] == 0).all() and (got[s2i[hit], 3] == 1).all()
    x = (rays[hit, 0:3] + rays[hit, 4:7] * t[hit, None]).astype(np.float64)
    corners = v[tri[ids[hit]]].astype(np.float64)                      # [k, 3, 3]
    e0, e1 = corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]
    d00, d01, d11 = (e0 * e0).sum(1), (e0 * e1).sum(1), (e1 * e1).sum(1)
    sin2 = (d00 * d11 - d01 * d01) / (d00 * d11)
    extent = np.sqrt(np.maximum(d00, d11))
    magnitude = np.abs(np.concatenate([corners.reshape(len(corners), -1), (corners - shift).reshape(len(corners), -1)], axis=1)).max(1)
    err = np.abs(got[s2i[hit], :3].astype(np.float64) - (x - shift.astype(np.float64))).max(1)
    # pv itself is rounded: v - shift in float32 is off by half an ulp of its magnitude per corner
    bound = (16 * extent / sin2 + 4 * magnitude) * 2.0 ** -24 + 0.5 * 2.0 ** -23 * magnitude
    fat = sin2 >= 1e-3
    print(f"rigid translation: {int(hit.sum())} hits, {int(fat.sum())} on fat triangles; max error {err[fat].max():.3g}, "
          f"max error / bound {float((err[fat] / bound[fat]).max()):.3g}, in ulp of the extent {float((err[fat] / (extent[fat] * 2.0 ** -23)).max()):.3g}")
    assert fat.sum() > 150 and (err[fat] <= bound[fat]).all()
    assert (err[~fat] <= extent[~fat] + magnitude[~fat] * 1e-5).all()


# ---------------------------------------------------------------- 5. quality, as a condition
QW, QH = 64, 48


def test_quality_eight_accumulated_frames_are_nearer_the_converged_one():
    """The floor-and-occluder scene of tests/test_denoise.py at its size, static camera: 8 frames of
    S = 1 with the renderer's consecutive seeds, accumulated with the defaults. The accumulated
    frame's MSE against the S = 256 frame is below 0.25 of the mean MSE of the single frames (0.125
    for independent frames; the cap leaves 2x for history rejected at the shadow's and the
    occluder's edges)."""
    from mrt.renderer import GlibcRand
    from mrt.temporal import MAX_HISTORY_DEFAULT, NORMAL_COS_DEFAULT, SIGMA_PLANE_FRACTION_DEFAULT, world_to_screen
    tris = T.rect(0.0, -4.0, 4.0, -3.0, 5.0) + T.fan(1.0, 1.0, (0.3, 0.4))
    scene, bufs, normals, material = T.world_of(tris)
    d = np.array([0.0, 5.0, -3.5])
    cam = mrt.host.Camera((0.0, -5.0, 4.0), tuple(d / np.linalg.norm(d)), (0.0, 0.0, 1.0), 45.0, 0.01, 100.0)
    prim, s2i = mrt.primary_rays(cam, QW, QH)
    trace = T.oracle_trace(bufs)
    pres = trace(prim, False)
    n = QW * QH

    def frame(samples, seed):
        return P.render_frame(mrt.host, trace, prim, pres, s2i, n, normals, material, samples, 1, [seed], n, True, T.KNOWN,
                              want_image=True)[1]
    ref = frame(256, 12)[:, :3].astype(np.float64)
    guide, albedo = mrt.host.denoise_features(s2i, prim, pres, normals, material, n)
    v = scene.arrays()[0].astype(np.float64)
    sigma_plane = float(np.linalg.norm(v.max(axis=0) - v.min(axis=0))) * SIGMA_PLANE_FRACTION_DEFAULT
    matrix = world_to_screen(cam, QW, QH)
    rand = GlibcRand()
    hst, out, singles = None, None, []
    for k in range(8):
        image = frame(1, rand())
        singles.append(float(((image[:, :3] - ref) ** 2).mean()))
        hst, out, _ = mrt.host.temporal_accumulate(image, guide, albedo, QW, QH, guide if k else None, hst, matrix, (0.5, 0.5),
                                                   max_history=MAX_HISTORY_DEFAULT, normal_cos=NORMAL_COS_DEFAULT,
                                                   sigma_plane=sigma_plane)
    hit = guide[:, 3] != 0
    after, before = float(((out[:, :3] - ref) ** 2).mean()), float(np.mean(singles))
    print(f"occluder 64x48, 8 x S=1 against S=256: mean single-frame MSE {before:.6g}, accumulated {after:.6g} "
          f"(ratio {after / before:.3f}); hits with history {float((hst[hit, 3] > 1).mean()):.3f}, mean length {float(hst[hit, 3].mean()):.2f}")
    assert 500 < hit.sum() and before > 0 and after < 0.25 * before


# ---------------------------------------------------------------- 6. the plan
def bits(x):
    return int(np.array(x, F).view(np.uint32))


def plan(w, h, max_history=32, normal_cos=0.9, sigma_plane=1.0, variant=0):
    out = subprocess.run([DRIVER, "plan", str(w), str(h), str(max_history), str(bits(normal_cos)), str(bits(sigma_plane)),
                          str(variant)], capture_output=True, text=True, check=True).stdout
    return [int(x) for x in out.split()]


def test_the_plan_checks_in_the_documented_order():
    bad, big = _lib.MRT_ERR_INVALID_ARG, _lib.MRT_ERR_TOO_LARGE
    assert plan(64, 48)[0] == 0
    for kw in (dict(w=0), dict(h=0), dict(w=-1), dict(max_history=0), dict(max_history=-5), dict(sigma_plane=0.0),
               dict(sigma_plane=-1.0), dict(sigma_plane=np.nan), dict(normal_cos=np.nan), dict(variant=3), dict(variant=-1)):
        args = dict(w=64, h=48)
        args.update(kw)
        assert plan(**args)[0] == bad, kw
    for kw in (dict(w=8193, h=8192), dict(w=64, h=48, max_history=(1 << 20) + 1)):
        assert plan(**kw)[0] == big, kw
    assert plan(8192, 8192, max_history=1 << 20)[0] == 0 and plan(1 << 26, 1)[0] == 0 and plan(1, 1 << 26)[0] == 0
    assert plan(8, 8, normal_cos=np.inf, sigma_plane=np.inf)[0] == 0 and plan(8, 8, normal_cos=-2.0, sigma_plane=1e-45)[0] == 0
    # shape before limits
    assert plan(8193, 8192, sigma_plane=0.0)[0] == bad and plan(0, 5, max_history=1 << 21)[0] == bad

    def motion(*args):
        return [int(x) for x in subprocess.run([DRIVER, "plan-motion", *map(str, args)], capture_output=True, text=True,
                                               check=True).stdout.split()]
    assert motion(0, 5, 5, 9) == [0, 1, 0] and motion(9, 5, 5, 0)[:2] == [0, 1]
    assert motion(1, 0, 0, 1) == [0, 0, 1] and motion(257, 5, 5, 9) == [0, 0, 2]
    assert motion(1 << 26, 1, 1, 1 << 26) == [0, 0, 1 << 18]
    for args in ((-1, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 1, -1), (-1, 1, 1, (1 << 26) + 1)):
        assert motion(*args)[0] == bad, args
    for args in (((1 << 26) + 1, 1, 1, 1), (1, 1, 1, (1 << 26) + 1)):
        assert motion(*args)[0] == big, args


@pytest.mark.parametrize("sigma", [1.0, 0.37, 3.4e38, 1e-30, 1e-45])
def test_the_plan_sizes_both_shapes_and_inverts_the_plane_tolerance(sigma):
    tw, th = _lib.MRT_TEMPORAL_TILE
    with np.errstate(all="ignore"):
        inv = bits(F(1.0) / F(sigma))
    for w, h in ((1, 1), (31, 7), (32, 8), (33, 9), (64, 4), (65, 5), (97, 83), (1920, 1080)):
        assert plan(w, h, sigma_plane=sigma, variant=1) == [0, 0, -(-w * h // 256), 0, 0, inv]
        tx, ty = -(-w // tw), -(-h // th)
        assert plan(w, h, sigma_plane=sigma, variant=2) == [0, 1, tx * ty, tx, ty, inv]
        assert plan(w, h, sigma_plane=sigma, variant=0) in (plan(w, h, sigma_plane=sigma, variant=1), plan(w, h, sigma_plane=sigma, variant=2))


# ---------------------------------------------------------------- 7. the same code under the sanitizers
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host compiler"
    exe = str(tmp_path_factory.mktemp("temporal_san") / "temporal_driver_san")
    sources = [os.path.join(REPO, "tests", "cpp", "temporal_driver.cpp"), os.path.join(PKG, "csrc", "host", "temporal.cpp"),
               os.path.join(PKG, "csrc", "host", "host_error.cpp"), os.path.join(PKG, "csrc", "temporal_plan.cpp")]
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(REPO, "include"),
                    "-o", exe, *sources], check=True)
    return exe


def test_host_functions_under_address_and_undefined_sanitizers(sanitized, tmp_path):
    def put(name, a):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(np.ascontiguousarray(a).tobytes())
        return path

    def run(args, what):
        r = subprocess.run([sanitized, *args], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, f"{what}: exit {r.returncode}\n{r.stderr[-3000:]}"

    for slots, pixels in ((1, 1), (300, 400), (5000, 5003)):
        s2i, rays, res, tri, v, pv = TU.motion_inputs(slots, pixels, seed=slots)
        out = str(tmp_path / "pp.bin")
        run(["motion", str(pixels), put("s2i.bin", s2i), put("rays.bin", rays), put("res.bin", res), put("tri.bin", tri),
             put("v.bin", v), put("pv.bin", pv), out], "motion")
        assert TU.same_floats(np.fromfile(out, F).reshape(-1, 4), mrt.host.temporal_motion(s2i, rays, res, tri, v, pv, pixels))
    for (w, h), kind, max_history, have_prev, moving in (((1, 1), "hits", 32, True, True), ((1, 7), "checker", 2, True, False),
                                                         ((7, 1), "mixed", 1, True, True), ((33, 9), "mixed", 32, False, False),
                                                         ((33, 9), "zero-normals", 2, True, True), ((97, 83), "mixed", 32, True, True),
                                                         ((97, 83), "hits", 2, True, False)):
        kw = TU.make_frame(w, h, kind, seed=w + h, max_history=max_history, have_prev=have_prev, moving=moving)
        words = np.concatenate([np.array([w, h, int(have_prev), max_history, bits(kw["normal_cos"]), bits(kw["sigma_plane"])], np.uint32),
                                kw.get("prev_world_to_screen", np.zeros(16, F)).view(np.uint32),
                                np.array(kw.get("prev_subpixel", (0.5, 0.5)), F).view(np.uint32)])
        want = mrt.host.temporal_accumulate(**kw)
        for want_image, want_pixels in ((True, True), (True, False), (False, True), (False, False)):
            oh, oi, op = str(tmp_path / "hst.bin"), str(tmp_path / "out.bin"), str(tmp_path / "px.bin")
            run(["accumulate", put("scalars.bin", words), put("image.bin", kw["image"]), put("guide.bin", kw["guide"]),
                 put("albedo.bin", kw["albedo"]), put("pp.bin", kw["prev_position"]) if moving else "-",
                 put("pg.bin", kw["prev_guide"]) if have_prev else "-", put("ph.bin", kw["prev_history"]) if have_prev else "-",
                 oh, oi if want_image else "-", op if want_pixels else "-"], f"accumulate {w}x{h} {kind}")
            assert TU.same_floats(np.fromfile(oh, F).reshape(-1, 4), want[0])
            if want_image:
                assert TU.same_floats(np.fromfile(oi, F).reshape(-1, 4), want[1])
            if want_pixels:
                assert np.array_equal(np.fromfile(op, np.uint32), want[2])


# ---------------------------------------------------------------- 8. world_to_screen
def test_world_to_screen_takes_every_pixel_centre_back():
    """Every pixel centre of a 64 x 48 frame, at three depths along its primary ray, comes back
    within 0.01 pixel. The residue (0.0026 pixel here, the same at every depth and in float64) is
    not the inverse's: a primary ray starts at the camera's position and aims at a point of the
    near plane 0.01 away, so the float32 rounding of the two bends it by about 1e-4 rad off the
    matrix's own line of sight."""
    from mrt.raygen import nscreen_to_world
    from mrt.temporal import world_to_screen
    w, h = 64, 48
    step = 1
    cam = mrt.host.Camera((1.0, -5.0, 4.0), (0.1, 0.8, -0.59), (0.0, 0.0, 1.0), 45.0, 0.01, 100.0)
    m = world_to_screen(cam, w, h)
    rays, s2i = mrt.primary_rays(cam, w, h)
    worst = 0.0
    for t in (0.5, 7.0, 90.0):
        x = (rays[::step, 0:3] + rays[::step, 4:7] * F(t)).astype(F)
        n = len(x)
        g = np.zeros((n, 8), F)
        g[:, 3], g[:, 4:7] = 1.0, x
        # through the host statement's own arithmetic: a 1 x n frame whose history is read at sx
        clip = np.stack([sum(m[j * 4 + i] * (x[:, j] if j < 3 else F(1.0)) for j in range(4)) for i in range(4)], axis=1)
        assert (clip[:, 3] > 0).all()
        sx = (clip[:, 0] / clip[:, 3] + 1) * 0.5 * w - 0.5
        sy = (clip[:, 1] / clip[:, 3] + 1) * 0.5 * h - 0.5
        px, py = s2i[::step] % w, s2i[::step] // w
        worst = max(worst, float(np.abs(sx - px).max()), float(np.abs(sy - py).max()))
    print(f"world_to_screen {w}x{h}: worst round trip {worst:.4g} pixel")
    assert worst <= 0.01
    behind = np.append(np.array(cam.position) - np.array(cam.forward), 1.0)
    assert float(m.reshape(4, 4).T[3] @ behind) < 0
    flat = mrt.host.Camera((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 45.0, 0.01, 100.0)
    try:
        nscreen_to_world(flat, w, h)
    except _lib.MrtError:
        return
    with pytest.raises(_lib.MrtError):
        world_to_screen(flat, w, h)


# ---------------------------------------------------------------- 9. the argument checks, the names
def test_host_exports_refuse_bad_arguments_and_write_nothing():
    lib = _lib.host_lib()
    w, h = 5, 4
    n = w * h
    kw = TU.make_frame(w, h, "hits", seed=1, moving=True)
    hst, out, px = np.full((n, 4), 7.5, F), np.full((n, 4), 7.5, F), np.full(n, 77, np.uint32)

    def params(**over):
        p = _lib.TemporalParams()
        p.width, p.height, p.havePrev, p.maxHistory, p.normalCos, p.sigmaPlane = w, h, 1, 32, 0.9, 1.0
        for i in range(16):
            p.prevWorldToScreen[i] = float(kw["prev_world_to_screen"][i])
        p.image, p.guide, p.albedo = kw["image"].ctypes.data, kw["guide"].ctypes.data, kw["albedo"].ctypes.data
        p.prevPosition, p.prevGuide, p.prevHistory = kw["prev_position"].ctypes.data, kw["prev_guide"].ctypes.data, kw["prev_history"].ctypes.data
        p.history, p.imageOut, p.pixels = hst.ctypes.data, out.ctypes.data, px.ctypes.data
        for k, v in over.items():
            setattr(p, k, v)
        return p
    assert lib.mrth_temporal_accumulate(None) == 1
    for over in (dict(width=0), dict(height=-1), dict(maxHistory=0), dict(maxHistory=(1 << 20) + 1), dict(sigmaPlane=0.0),
                 dict(sigmaPlane=float("nan")), dict(normalCos=float("nan")), dict(variant=3), dict(image=None), dict(guide=None),
                 dict(albedo=None), dict(history=None), dict(prevGuide=None), dict(prevHistory=None)):
        assert lib.mrth_temporal_accumulate(C.byref(params(**over))) == 1, over
        assert lib.mrth_last_error()
        assert (hst == 7.5).all() and (out == 7.5).all() and (px == 77).all(), over
    # without a previous frame its buffers may be missing; so may either output, or both, and prevPosition
    assert lib.mrth_temporal_accumulate(C.byref(params(havePrev=0, prevGuide=None, prevHistory=None, imageOut=None, pixels=None))) == 0
    assert (hst[:, 3] == 1).all() and (out == 7.5).all() and (px == 77).all()
    assert lib.mrth_temporal_accumulate(C.byref(params(prevPosition=None))) == 0 and (out != 7.5).any() and (px != 77).any()
    with pytest.raises(_lib.MrtError):
        mrt.host.temporal_accumulate(kw["image"], kw["guide"], kw["albedo"], w + 1, h)
    s2i, rays, res, tri, v, pv = TU.motion_inputs(9, 12, seed=2)
    pp = np.full((12, 4), 7.5, F)
    args = [9, s2i.ctypes.data, rays.ctypes.data, res.ctypes.data, tri.ctypes.data, len(tri), v.ctypes.data, pv.ctypes.data,
            len(v), 12, pp.ctypes.data]
    for at, bad in ((0, -1), (5, -1), (8, -1), (9, -1), (0, (1 << 26) + 1), (9, (1 << 26) + 1), (1, None), (2, None), (3, None),
                    (4, None), (6, None), (7, None), (10, None)):
        broken = list(args)
        broken[at] = bad
        assert lib.mrth_temporal_motion(*broken) == 1, at
        assert (pp == 7.5).all(), at
    for at in (0, 9):   # no slot, no pixel: fine, nothing written
        empty = list(args)
        empty[at] = 0
        assert lib.mrth_temporal_motion(*empty) == 0 and (pp == 7.5).all()
    assert lib.mrth_temporal_motion(*args) == 0 and (pp != 7.5).any()


def test_the_python_constants_are_the_headers():
    text = open(os.path.join(PKG, "csrc", "temporal_limits.hpp")).read()
    for name, value in (("kMaxPixels = 1 << 26", _lib.MRT_TEMPORAL_MAX_PIXELS == 1 << 26),
                        ("kMaxHistory = 1 << 20", _lib.MRT_TEMPORAL_MAX_HISTORY == 1 << 20),
                        ("kTileW = 32, kTileH = 8", _lib.MRT_TEMPORAL_TILE == (32, 8))):
        assert name in text and value, name
    assert C.sizeof(_lib.TemporalParams) == 8 * 4 + 18 * 4 + 9 * C.sizeof(C.c_void_p)
    for header, struct in (("mrt_temporal.h", "mrt_temporal_params"), ("mrt_host.h", "mrth_temporal_params")):
        import re
        body = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
        body = re.search(r"typedef struct " + struct + r"\s*\{(.*?)\}\s*" + struct + ";", body, flags=re.S).group(1)
        fields = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[\d+\])?\s*;", body)
        assert fields == [n for n, _ in _lib.TemporalParams._fields_], header


def test_the_accumulator_refuses_tensors_it_would_misread():
    """Before anything reaches the device: vertices in another memory layout (what numpy hands back
    for an expression over a fancy-indexed array), another dtype, too few of them."""
    torch = pytest.importorskip("torch")
    from mrt.temporal import TemporalAccumulator
    from mrt.tracer import RayBuffer
    cpu = torch.device("cpu")
    acc = TemporalAccumulator(cpu)
    n = 12
    primary = RayBuffer(torch.zeros((n, 8)), device=cpu)
    s2i = torch.arange(n, dtype=torch.int32)
    normals, material = torch.zeros((2, 3)), torch.zeros(2, dtype=torch.int32)
    image = torch.zeros((n, 4))
    tri = torch.zeros((2, 3), dtype=torch.int32)
    v = torch.zeros((5, 3))

    def call(**kw):
        args = dict(triangles=tri, vertices=v, prev_vertices=v.clone())
        args.update(kw)
        acc.accumulate(primary, s2i, normals, material, 4, 3, np.zeros(16, F), (0.5, 0.5), image, **args)
    for kw in (dict(vertices=torch.zeros((3, 5)).T), dict(prev_vertices=torch.zeros((3, 5)).T), dict(vertices=v.double()),
               dict(triangles=tri.long()), dict(triangles=torch.zeros((3, 2), dtype=torch.int32).T), dict(triangles=None),
               dict(vertices=None), dict(prev_vertices=torch.zeros((4, 3))), dict(triangles=torch.zeros((3, 3), dtype=torch.int32))):
        with pytest.raises(_lib.MrtError):
            call(**kw)
    with pytest.raises(_lib.MrtError):
        acc.accumulate(primary, s2i, normals, material, 4, 3, np.zeros(16, F), (0.5, 0.5), image[:, :3])
    assert not acc.sets and not acc._have_prev          # nothing was reserved, nothing counted as a frame
