"""The variance-guided filter on the CPU: mrth_svgf_accumulate and mrth_svgf_filter
(csrc/host/svgf.cpp over csrc/svgf_common.hpp), the CPU statements of mrt_svgf_accumulate /
mrt_svgf_filter, against the independent numpy model of tests/svgf_util.py, bit for bit (a NaN equal
to a NaN); the accumulation against mrth_temporal_accumulate, bit for bit; known answers; the
quality conditions on the floor-and-occluder sequence of tests/test_temporal.py; the plan
(csrc/svgf_plan.cpp) through lib/svgf_driver; the host functions as a stand-alone program under
-fsanitize=address,undefined (tests/cpp/svgf_driver.cpp; nothing is preloaded); the host argument
checks; and the struct layouts. None needs a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mrt
import mrt.host
from mrt import _lib

import denoise_util as D
import path_util as P
import svgf_util as SU
import temporal_util as TU
import test_path as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gpu-ray-tracing_amd")
F = np.float32
DRIVER = os.path.join(PKG, "lib", "svgf_driver")


def same(got, want, names):
    assert len(got) == len(want) == len(names)
    for g, w, name in zip(got, want, names):
        assert (g is None) == (w is None), name
        if w is not None:
            assert SU.same_floats(g, w) if w.dtype == F else np.array_equal(g, w), name


ACC_NAMES = ("history", "moments", "image", "pixels")
FILTER_NAMES = ("image", "pixels", "variance")


# ---------------------------------------------------------------- 1. the host statements against the model
@pytest.mark.parametrize("frame", SU.FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("kind", SU.GUIDE_KINDS)
def test_host_accumulate_equals_the_model_and_the_temporal_statement(frame, kind):
    w, h = frame
    seen = {"found": 0, "nan": 0}
    for max_history in SU.MAX_HISTORIES:
        for have_prev, moving in ((False, False), (True, False), (True, True)):
            kw = SU.make_accumulate(w, h, kind, seed=w * 131 + h + max_history, max_history=max_history, have_prev=have_prev,
                                    moving=moving)
            got = mrt.host.svgf_accumulate(**kw)
            same(got, SU.Model.svgf_accumulate(**kw), ACC_NAMES)
            temporal = mrt.host.temporal_accumulate(**{k: v for k, v in kw.items() if k != "prev_moments"})
            same((got[0], got[2], got[3]), temporal, ("history", "image", "pixels"))
            assert SU.same_floats(got[1][:, 3], got[0][:, 3]) and (got[1][:, 2] == 0).all()    # one length, nothing in z
            only_px = mrt.host.svgf_accumulate(want_image=False, **kw)
            assert only_px[2] is None and np.array_equal(only_px[3], got[3]) and SU.same_floats(only_px[1], got[1])
            seen["found"] += int((got[1][:, 3] > 1).sum())
            seen["nan"] += int(np.isnan(got[1][:, :2]).sum())
    if kind == "misses":
        assert seen["found"] == 0
    elif w * h > 60 and kind != "zero-normals":
        assert seen["found"] > 0 and seen["nan"] > 0      # the table reached the blend and a NaN moment


@pytest.mark.parametrize("frame", SU.FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("kind", SU.GUIDE_KINDS)
def test_host_filter_equals_the_model(frame, kind):
    w, h = frame
    for iterations in SU.ITERATIONS:
        kw = SU.make_filter(w, h, kind, seed=w + 7 * h + iterations)
        got = mrt.host.svgf_filter(iterations=iterations, **kw)
        same(got, SU.Model.svgf_filter(iterations=iterations, **kw), FILTER_NAMES)
        assert SU.same_floats(got[0][:, 3], kw["image"][:, 3])            # w is carried
        hit = kw["guide"][:, 3] != 0
        assert (got[2][~hit] == 0).all() and not (got[2] < 0).any()       # a miss has no variance, nobody a negative one
        if iterations in (0, 3):
            for want in ((True, False, False), (False, True, True), (False, True, False)):
                part = mrt.host.svgf_filter(iterations=iterations, want_image=want[0], want_pixels=want[1], want_variance=want[2], **kw)
                same(part, [g if on else None for g, on in zip(got, want)], FILTER_NAMES)
    if w * h > 60 and kind in ("hits", "mixed", "checker"):
        length = kw["moments"][hit, 3]
        assert (length >= 4).any() and (length < 4).any() and np.isnan(length).any() and np.isinf(length).any()


@pytest.mark.parametrize("sigma", [1e-30, 0.25, 4.0, 1e25])
def test_host_filter_equals_the_model_at_the_ends_of_sigma_luminance(sigma):
    """A sigma whose square underflows to 0 leaves invL = 1e8 everywhere; one whose square overflows
    makes invL 0 wherever there is variance and a NaN (0 * inf) where there is none."""
    kw = SU.make_filter(33, 9, "mixed", seed=4, sigma_luminance=sigma)
    same(mrt.host.svgf_filter(iterations=3, **kw), SU.Model.svgf_filter(iterations=3, **kw), FILTER_NAMES)


# ---------------------------------------------------------------- 2. known answers
KW, KH = 64, 8


def plane(w=KW, h=KH):
    """Pixel (px, py) sees the position (px, py, 0) with the normal +z: with screen_matrix(w, h) it reprojects to itself."""
    n = w * h
    ys, xs = np.divmod(np.arange(n), w)
    g = np.zeros((n, 8), F)
    g[:, 2], g[:, 3], g[:, 4], g[:, 5] = 1.0, 1.0, xs, ys
    return g


def ones(n):
    return np.ones((n, 4), F)


def grey(values):
    return np.stack([values, values, values, np.ones_like(values)], axis=1).astype(F)


def moments_of(n, m1, m2, length):
    m = np.zeros((n, 4), F)
    m[:, 0], m[:, 1], m[:, 3] = m1, m2, length
    return m


IMPLS = pytest.mark.parametrize("impl", [mrt.host, SU.Model], ids=["host", "model"])


def run_static(impl, frames, max_history):
    """Identity-reprojected frames over the plane: the list of (history, moments) after each."""
    g, hst, mom, out = plane(), None, None, []
    matrix = TU.screen_matrix(KW, KH)
    for k, image in enumerate(frames):
        hst, mom, _, _ = impl.svgf_accumulate(image, g, ones(KW * KH), KW, KH, g if k else None, hst, mom, matrix,
                                              max_history=max_history, normal_cos=0.9, sigma_plane=0.5)
        out.append((hst, mom))
    return out


@IMPLS
def test_known_answer_a_static_sequence_gives_the_mean_the_mean_square_and_the_variance(impl):
    """K = 8 identity-reprojected grey frames of independent values l_k in [0, 1] (M = their largest).
    lum((l, l, l)) is three products and two sums of positive terms: within 3 * 2^-24 M of l, and its
    square within 8 * 2^-24 M^2 of l^2. A running mean rounds three times a step (DESIGN section 18:
    4 K 2^-24 of the largest value), so
        |m1 - mean(l)|   <= e1 = (4 K + 3) 2^-24 M
        |m2 - mean(l^2)| <= e2 = (4 K + 8) 2^-24 M^2
    and var = pos(m2 - m1 * m1), with two more roundings of values below M^2, is within
        e2 + 2 M e1 + e1^2 + 2 * 2^-24 M^2
    of the float64 population variance of the same K values."""
    n, K = KW * KH, 8
    rng = np.random.default_rng(21)
    values = rng.random((K, n)).astype(F)
    steps = run_static(impl, [grey(v) for v in values], max_history=32)
    hst, mom = steps[-1]
    v64 = values.astype(np.float64)
    M = float(values.max())
    e1, e2 = (4 * K + 3) * 2.0 ** -24 * M, (4 * K + 8) * 2.0 ** -24 * M * M
    err1 = float(np.abs(mom[:, 0] - v64.mean(axis=0)).max())
    err2 = float(np.abs(mom[:, 1] - (v64 ** 2).mean(axis=0)).max())
    _, _, var = impl.svgf_filter(grey(hst[:, 0]), plane(), ones(n), mom, KW, KH, iterations=0, sigma_plane=0.5)
    bound = e2 + 2 * M * e1 + e1 * e1 + 2 * 2.0 ** -24 * M * M
    errv = float(np.abs(var - v64.var(axis=0)).max())
    print(f"static sequence of {K}: m1 error {err1:.3g} (bound {e1:.3g}), m2 {err2:.3g} ({e2:.3g}), variance {errv:.3g} ({bound:.3g})")
    assert (mom[:, 3] == K).all() and err1 <= e1 and err2 <= e2 and errv <= bound
    assert float(var.min()) > 0.001       # eight random values are not all alike


@IMPLS
def test_known_answer_the_lengths_count_to_max_history_and_are_the_colour_historys(impl):
    n = KW * KH
    rng = np.random.default_rng(22)
    frames = [grey(rng.random(n).astype(F)) for _ in range(7)]
    for k, (hst, mom) in enumerate(run_static(impl, frames, max_history=5)):
        assert (mom[:, 3] == min(k + 1, 5)).all() and np.array_equal(mom[:, 3], hst[:, 3])


def lonely(n, at):
    g = np.zeros((n, 8), F)
    g[at] = plane()[at]
    return g


@IMPLS
@pytest.mark.parametrize("variance", [0.0, 0.5])
def test_known_answer_a_pixel_alone_in_its_stencil_keeps_its_colour_and_variance(impl, variance):
    """Every tap but the centre is a miss: sum / wsum is (w c) / w and sv / (wsum * wsum) is (w^2 v)
    / w^2 with w = 9/64, exact for values of a few bits, through every iteration."""
    n = KW * KH
    at = 3 * KW + 20
    image = np.zeros((n, 4), F)
    image[at] = (0.5, 0.25, 0.75, 0.125)
    mom = moments_of(n, 0.5, 0.25 + variance, 4.0)
    out, _, var = impl.svgf_filter(image, lonely(n, at), ones(n), mom, KW, KH, iterations=5, sigma_plane=0.5)
    assert np.array_equal(out[at], image[at]) and var[at] == variance and (np.delete(var, at) == 0).all()


@IMPLS
def test_known_answer_nothing_crosses_a_luminance_step_where_the_variance_is_zero(impl):
    """A flat plane, grey 0.25 left of a vertical line and 0.75 right of it, variance 0 everywhere:
    invL = 1 / 1e-8f, so a tap across the step (|dl| = d = 0.5) has wl = 1 / (1 + d^2 invL) against
    1 on its own side. A pixel's result is a convex combination: its own side's taps weigh at least
    the centre's 9/64, the other side's at most (sum of hw <= 1) * wl, so one iteration moves a value
    by at most leak = d * wl * 64 / 9 (3.6e-8 here) plus the rounding of a weighted mean of 25 nearly
    equal values, 27 * 2^-24 of the value. The variance stays 0 (sv sums w^2 * 0), so every iteration
    is in the same position with values that have moved by the bound so far; d shrinks by twice
    that, which changes wl by a relative 1e-6. After 5 iterations: 5 * (1.001 leak + 27 * 2^-24 * 0.75)."""
    n = KW * KH
    xs = np.arange(n) % KW
    left = xs < KW // 2
    image = grey(np.where(left, F(0.25), F(0.75)))
    mom = moments_of(n, 0.0, 0.0, 4.0)
    out, _, var = impl.svgf_filter(image, plane(), ones(n), mom, KW, KH, iterations=5, sigma_plane=0.5)
    d, inv_l = 0.5, 1.0 / float(F(1e-8))
    leak = d / (1.0 + d * d * inv_l) * 64.0 / 9.0
    bound = 5 * (1.001 * leak + 27 * 2.0 ** -24 * 0.75)
    worst = max(float(np.abs(out[left, :3] - 0.25).max()), float(np.abs(out[~left, :3] - 0.75).max()))
    print(f"luminance step: worst move {worst:.3g}, bound {bound:.3g}")
    assert worst <= bound and (var == 0).all()


@IMPLS
def test_known_answer_a_uniform_variance_shrinks_by_the_sum_of_the_squared_taps(impl):
    """A flat constant image with the variance 1 everywhere: every weight is hw (a = wz = wl = 1), the
    weights sum to 1 in the interior, and the new variance is sum(hw^2) = (0.375^2 + 2 * 0.25^2 + 2 *
    0.0625^2)^2 = (35 / 128)^2. Every hw^2 is a multiple of 2^-16 and every partial sum is below 1, so
    the float sum is exact."""
    n = KW * KH
    image = grey(np.full(n, 0.5, F))
    mom = moments_of(n, 0.0, 1.0, 4.0)
    out, _, var = impl.svgf_filter(image, plane(), ones(n), mom, KW, KH, iterations=1, sigma_plane=0.5)
    var = var.reshape(KH, KW)
    assert (var[2:-2, 2:-2] == (35.0 / 128.0) ** 2).all() and np.array_equal(out, image)
    assert (var[0] > (35.0 / 128.0) ** 2).all()       # an edge row has fewer taps to average over


@IMPLS
@pytest.mark.parametrize("length", [1.0, 2.0, 3.0])
def test_known_answer_a_short_history_among_equal_moments_scales_its_own_variance(impl, length):
    """Every moment of the window is (0.5, 0.75): M1 = (k * 0.5) / k and M2 = (k * 0.75) / k are exact
    for the k <= 49 taps of weight 1, so the variance is pos(0.75 - 0.25) * (4 / N), the pixel's own formula."""
    n = KW * KH
    mom = moments_of(n, 0.5, 0.75, length)
    _, _, var = impl.svgf_filter(grey(np.full(n, 0.5, F)), plane(), ones(n), mom, KW, KH, iterations=0, sigma_plane=0.5)
    assert (var == F(0.5) * (F(4.0) / F(length))).all()
    mom[:, 3] = 4.0                                      # at 4 the scale is gone
    _, _, var = impl.svgf_filter(grey(np.full(n, 0.5, F)), plane(), ones(n), mom, KW, KH, iterations=0, sigma_plane=0.5)
    assert (var == 0.5).all()


# ---------------------------------------------------------------- 3. quality, as conditions
QW, QH = 64, 48
# Recorded on this sequence (printed below): accumulated 7.44e-4, accumulate +
# denoise_filter 6.94e-4, svgf 1.03e-4: 0.138 of the accumulated frame and 0.148 of the pair (at the
# provisional sigma_luminance 4, before the sweep chose 2: 2.97e-4, 0.399 and 0.428). The sequence is
# deterministic (fixed seeds, host arithmetic), so the margin has no noise to cover, and at 0.15
# svgf has room to spare: the margin is 1, "no worse than the pair it replaces".
MARGIN_OVER_THE_PAIR = 1.0


def test_quality_svgf_beats_the_accumulated_frame_and_keeps_up_with_accumulate_then_denoise():
    """The floor-and-occluder sequence of tests/test_temporal.py: 8 frames of S = 1 with the
    renderer's consecutive seeds, a static camera, against the S = 256 frame. The SVGF frame's MSE
    is below the accumulated, unfiltered frame's (strictly), and not above MARGIN_OVER_THE_PAIR
    times that of accumulate followed by denoise_filter at its shipped defaults. Both yardsticks are
    the existing statements' outputs."""
    from mrt.denoise import ITERATIONS_DEFAULT, SIGMA_COLOR_DEFAULT
    from mrt.renderer import GlibcRand
    from mrt.svgf import SIGMA_LUMINANCE_DEFAULT
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
    settings = dict(max_history=MAX_HISTORY_DEFAULT, normal_cos=NORMAL_COS_DEFAULT, sigma_plane=sigma_plane)
    hst = mom = hst_t = None
    for k in range(8):
        image = frame(1, rand())
        hst, mom, acc, _ = mrt.host.svgf_accumulate(image, guide, albedo, QW, QH, guide if k else None, hst, mom, matrix,
                                                    (0.5, 0.5), **settings)
        hst_t, acc_t, _ = mrt.host.temporal_accumulate(image, guide, albedo, QW, QH, guide if k else None, hst_t, matrix,
                                                       (0.5, 0.5), **settings)
    assert SU.same_floats(acc, acc_t)
    filtered, _, var = mrt.host.svgf_filter(acc, guide, albedo, mom, QW, QH, sigma_luminance=SIGMA_LUMINANCE_DEFAULT,
                                            sigma_plane=sigma_plane)
    pair, _ = mrt.host.denoise_filter(acc_t, guide, albedo, QW, QH, iterations=ITERATIONS_DEFAULT, sigma_color=SIGMA_COLOR_DEFAULT,
                                      sigma_plane=sigma_plane)

    def mse(x):
        return float(((x[:, :3] - ref) ** 2).mean())
    print(f"occluder 64x48, 8 x S=1 against S=256: accumulated {mse(acc):.6g}, accumulate + denoise {mse(pair):.6g}, svgf {mse(filtered):.6g} "
          f"(svgf / accumulated {mse(filtered) / mse(acc):.3f}, svgf / pair {mse(filtered) / mse(pair):.3f}); mean variance {float(var.mean()):.4g}")
    assert mse(filtered) < mse(acc)
    assert mse(filtered) <= MARGIN_OVER_THE_PAIR * mse(pair)


# ---------------------------------------------------------------- 4. the plan
def bits(x):
    return int(np.array(x, F).view(np.uint32))


def plan(w, h, iterations=5, squarings=7, sigma_luminance=4.0, sigma_plane=1.0, variant=0):
    out = subprocess.run([DRIVER, "plan", str(w), str(h), str(iterations), str(squarings), str(bits(sigma_luminance)),
                          str(bits(sigma_plane)), str(variant)], capture_output=True, text=True, check=True).stdout
    rows = [[int(x) for x in line.split()] for line in out.splitlines()]
    return rows[0], rows[1:]


def test_the_plan_checks_in_the_documented_order():
    bad, big = _lib.MRT_ERR_INVALID_ARG, _lib.MRT_ERR_TOO_LARGE
    assert plan(64, 48)[0][0] == 0
    for kw in (dict(w=0), dict(h=0), dict(w=-1), dict(iterations=-1), dict(squarings=-1), dict(variant=3), dict(variant=-1),
               dict(sigma_luminance=0.0), dict(sigma_luminance=-1.0), dict(sigma_luminance=np.nan), dict(sigma_plane=0.0),
               dict(sigma_plane=np.nan)):
        args = dict(w=64, h=48)
        args.update(kw)
        assert plan(**args)[0][0] == bad, kw
    for kw in (dict(w=8193, h=8192), dict(w=64, h=48, iterations=9), dict(w=64, h=48, squarings=11)):
        assert plan(**kw)[0][0] == big, kw
    assert plan(8192, 8192, iterations=8, squarings=10)[0][0] == 0 and plan(1 << 26, 1)[0][0] == 0
    assert plan(8, 8, sigma_luminance=np.inf, sigma_plane=1e-45)[0][0] == 0
    # shape before limits
    assert plan(8193, 8192, sigma_luminance=0.0)[0][0] == bad and plan(0, 5, iterations=9)[0][0] == bad


@pytest.mark.parametrize("sigma", [4.0, 0.37, 1e-30, 3e19])
def test_the_plan_sizes_both_shapes_and_squares_the_luminance_tolerance(sigma):
    tw, th = _lib.MRT_SVGF_TILE
    rw, rr = _lib.MRT_SVGF_ROW_TILE
    with np.errstate(all="ignore"):
        inv, sl2 = bits(F(1.0) / F(0.37)), bits(F(sigma) * F(sigma))
    for w, h in ((1, 1), (31, 7), (32, 8), (33, 9), (64, 4), (65, 5), (97, 83), (1920, 1080)):
        tx, ty = -(-w // tw), -(-h // th)
        head, direct = plan(w, h, 8, sigma_luminance=sigma, sigma_plane=0.37, variant=1)
        assert head == [0, tx * ty, tx, inv, sl2]
        assert direct == [[1 << k, 0, tx * ty, tx, ty, 0, 0] for k in range(8)]
        _, staged = plan(w, h, 8, sigma_luminance=sigma, sigma_plane=0.37, variant=2)
        for k, row in enumerate(staged):
            s = 1 << k
            if s > _lib.MRT_SVGF_TILED_MAX_STEP:
                assert row == direct[k]
                continue
            residues = min(s, h)
            groups = -(-(-(-h // s)) // rr)
            assert row == [s, 1, -(-w // rw) * residues * groups, -(-w // rw), residues * groups, residues, 8 * (rw + 4 * s) * 48]
        shipped = plan(w, h, 8, sigma_luminance=sigma, sigma_plane=0.37, variant=0)[1]
        assert all(row in (direct[k], staged[k]) for k, row in enumerate(shipped))
    assert plan(64, 48, 0)[1] == [] and len(plan(64, 48, 3)[1]) == 3


# ---------------------------------------------------------------- 5. the same code under the sanitizers
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host compiler"
    exe = str(tmp_path_factory.mktemp("svgf_san") / "svgf_driver_san")
    sources = [os.path.join(REPO, "tests", "cpp", "svgf_driver.cpp"), os.path.join(PKG, "csrc", "host", "svgf.cpp"),
               os.path.join(PKG, "csrc", "host", "host_error.cpp"), os.path.join(PKG, "csrc", "svgf_plan.cpp"),
               os.path.join(PKG, "csrc", "temporal_plan.cpp")]
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

    for (w, h), kind, max_history, have_prev, moving in (((1, 1), "hits", 32, True, True), ((3, 2), "checker", 2, True, False),
                                                         ((7, 1), "mixed", 1, True, True), ((33, 9), "mixed", 32, False, False),
                                                         ((97, 83), "mixed", 32, True, True)):
        kw = SU.make_accumulate(w, h, kind, seed=w + h, max_history=max_history, have_prev=have_prev, moving=moving)
        words = np.concatenate([np.array([w, h, int(have_prev), max_history, bits(kw["normal_cos"]), bits(kw["sigma_plane"])], np.uint32),
                                kw.get("prev_world_to_screen", np.zeros(16, F)).view(np.uint32),
                                np.array(kw.get("prev_subpixel", (0.5, 0.5)), F).view(np.uint32)])
        want = mrt.host.svgf_accumulate(**kw)
        for want_image, want_pixels in ((True, True), (False, False)):
            oh, om, oi, op = (str(tmp_path / name) for name in ("hst.bin", "mom.bin", "out.bin", "px.bin"))
            run(["accumulate", put("scalars.bin", words), put("image.bin", kw["image"]), put("guide.bin", kw["guide"]),
                 put("albedo.bin", kw["albedo"]), put("pp.bin", kw["prev_position"]) if moving else "-",
                 put("pg.bin", kw["prev_guide"]) if have_prev else "-", put("ph.bin", kw["prev_history"]) if have_prev else "-",
                 put("pm.bin", kw["prev_moments"]) if have_prev else "-", oh, om, oi if want_image else "-",
                 op if want_pixels else "-"], f"accumulate {w}x{h} {kind}")
            assert SU.same_floats(np.fromfile(oh, F).reshape(-1, 4), want[0]) and SU.same_floats(np.fromfile(om, F).reshape(-1, 4), want[1])
            if want_image:
                assert SU.same_floats(np.fromfile(oi, F).reshape(-1, 4), want[2])
            if want_pixels:
                assert np.array_equal(np.fromfile(op, np.uint32), want[3])
    for (w, h), kind, iterations in (((1, 1), "hits", 5), ((3, 2), "hits", 3), ((1, 7), "checker", 1), ((33, 9), "mixed", 0),
                                     ((33, 9), "zero-normals", 2), ((97, 83), "mixed", 5)):
        kw = SU.make_filter(w, h, kind, seed=w + h)
        words = np.array([w, h, iterations, kw["normal_squarings"], bits(kw["sigma_luminance"]), bits(kw["sigma_plane"])], np.uint32)
        want = mrt.host.svgf_filter(iterations=iterations, **kw)
        for wants in ((True, True, True), (False, True, False)):
            outs = [str(tmp_path / name) for name in ("out.bin", "px.bin", "var.bin")]
            run(["filter", put("scalars.bin", words), put("image.bin", kw["image"]), put("guide.bin", kw["guide"]),
                 put("albedo.bin", kw["albedo"]), put("mom.bin", kw["moments"]), *[o if on else "-" for o, on in zip(outs, wants)]],
                f"filter {w}x{h} {kind} {iterations}")
            if wants[0]:
                assert SU.same_floats(np.fromfile(outs[0], F).reshape(-1, 4), want[0])
                assert SU.same_floats(np.fromfile(outs[2], F), want[2])
            assert np.array_equal(np.fromfile(outs[1], np.uint32), want[1])


# ---------------------------------------------------------------- 6. the argument checks, the layouts
def test_host_exports_refuse_bad_arguments_in_order_and_write_nothing():
    lib = _lib.host_lib()
    w, h = 5, 4
    n = w * h
    kw = SU.make_accumulate(w, h, "hits", seed=1, moving=True)
    outs = {k: np.full((n, 4), 7.5, F) for k in ("history", "moments", "imageOut")}
    px = np.full(n, 77, np.uint32)

    def untouched():
        return all((a == 7.5).all() for a in outs.values()) and (px == 77).all()

    def acc(**over):
        p = _lib.SvgfAccumulateParams()
        p.width, p.height, p.havePrev, p.maxHistory, p.normalCos, p.sigmaPlane = w, h, 1, 32, 0.9, 1.0
        for i in range(16):
            p.prevWorldToScreen[i] = float(kw["prev_world_to_screen"][i])
        p.image, p.guide, p.albedo = kw["image"].ctypes.data, kw["guide"].ctypes.data, kw["albedo"].ctypes.data
        p.prevPosition, p.prevGuide = kw["prev_position"].ctypes.data, kw["prev_guide"].ctypes.data
        p.prevHistory, p.prevMoments = kw["prev_history"].ctypes.data, kw["prev_moments"].ctypes.data
        p.history, p.moments, p.imageOut, p.pixels = (outs["history"].ctypes.data, outs["moments"].ctypes.data,
                                                      outs["imageOut"].ctypes.data, px.ctypes.data)
        for k, v in over.items():
            setattr(p, k, v)
        return p
    assert lib.mrth_svgf_accumulate(None) == 1
    for over in (dict(width=0), dict(height=-1), dict(maxHistory=0), dict(maxHistory=(1 << 20) + 1), dict(sigmaPlane=0.0),
                 dict(sigmaPlane=float("nan")), dict(normalCos=float("nan")), dict(variant=3), dict(image=None), dict(guide=None),
                 dict(albedo=None), dict(history=None), dict(moments=None), dict(prevGuide=None), dict(prevHistory=None),
                 dict(prevMoments=None)):
        assert lib.mrth_svgf_accumulate(C.byref(acc(**over))) == 1, over
        assert lib.mrth_last_error() and untouched(), over
    # a scalar check comes before a pointer check: the message is the plan's
    assert lib.mrth_svgf_accumulate(C.byref(acc(width=0, image=None))) == 1 and b"frame size" in lib.mrth_last_error()
    assert lib.mrth_svgf_accumulate(C.byref(acc(havePrev=0, prevGuide=None, prevHistory=None, prevMoments=None, imageOut=None,
                                                pixels=None))) == 0
    assert (outs["moments"][:, 3] == 1).all() and (outs["imageOut"] == 7.5).all() and (px == 77).all()

    fk = SU.make_filter(w, h, "hits", seed=2)
    scratch = [np.full((n, 4), 7.5, F) for _ in range(2)]
    out, var = np.full((n, 4), 7.5, F), np.full(n, 7.5, F)
    px[:] = 77

    def clean():
        return all((a == 7.5).all() for a in (*scratch, out, var)) and (px == 77).all()

    def flt(**over):
        p = _lib.SvgfFilterParams()
        p.width, p.height, p.iterations, p.normalSquarings, p.sigmaLuminance, p.sigmaPlane = w, h, 3, 2, 4.0, 1.0
        p.image, p.guide, p.albedo, p.moments = (fk[k].ctypes.data for k in ("image", "guide", "albedo", "moments"))
        p.scratch[0], p.scratch[1] = scratch[0].ctypes.data, scratch[1].ctypes.data
        p.imageOut, p.pixels, p.varianceOut = out.ctypes.data, px.ctypes.data, var.ctypes.data
        for k, v in over.items():
            if k.startswith("scratch"):
                p.scratch[int(k[-1])] = v
            else:
                setattr(p, k, v)
        return p
    assert lib.mrth_svgf_filter(None) == 1
    for over in (dict(width=0), dict(height=0), dict(iterations=-1), dict(iterations=9), dict(normalSquarings=-1),
                 dict(normalSquarings=11), dict(variant=3), dict(sigmaLuminance=0.0), dict(sigmaLuminance=float("nan")),
                 dict(sigmaPlane=0.0), dict(image=None), dict(guide=None), dict(albedo=None), dict(moments=None), dict(scratch0=None),
                 dict(scratch1=None), dict(imageOut=None, pixels=None)):
        assert lib.mrth_svgf_filter(C.byref(flt(**over))) == 1, over
        assert lib.mrth_last_error() and clean(), over
    assert lib.mrth_svgf_filter(C.byref(flt(sigmaLuminance=0.0, image=None))) == 1 and b"sigmaLuminance" in lib.mrth_last_error()
    # a scratch buffer that the iteration count does not need may be missing; so may the variance and one of the two images
    assert lib.mrth_svgf_filter(C.byref(flt(iterations=1, scratch1=None, varianceOut=None, imageOut=None))) == 0
    assert (px != 77).any() and (out == 7.5).all() and (var == 7.5).all() and (scratch[1] == 7.5).all()
    assert lib.mrth_svgf_filter(C.byref(flt(iterations=0, scratch0=None, scratch1=None, pixels=None))) == 0 and (var != 7.5).any()
    with pytest.raises(_lib.MrtError):
        mrt.host.svgf_filter(fk["image"], fk["guide"], fk["albedo"], fk["moments"], w + 1, h)


def struct_fields(header, struct):
    body = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    body = re.search(r"typedef struct " + struct + r"\s*\{(.*?)\}\s*" + struct + ";", body, flags=re.S).group(1)
    return re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[\d+\])?\s*;", body)


def test_the_struct_layouts_and_constants_are_the_headers():
    for header, prefix in (("mrt_svgf.h", "mrt"), ("mrt_host.h", "mrth")):
        assert struct_fields(header, prefix + "_svgf_accumulate_params") == [n for n, _ in _lib.SvgfAccumulateParams._fields_], header
        assert struct_fields(header, prefix + "_svgf_filter_params") == [n for n, _ in _lib.SvgfFilterParams._fields_], header
    # the accumulation's struct begins as the temporal one does
    assert struct_fields("mrt_svgf.h", "mrt_svgf_accumulate_params")[:19] == struct_fields("mrt_temporal.h", "mrt_temporal_params")
    ptr = C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.SvgfAccumulateParams) == 8 * 4 + 18 * 4 + 11 * ptr and C.sizeof(_lib.SvgfFilterParams) == 8 * 4 + 10 * ptr
    text = open(os.path.join(PKG, "csrc", "svgf_limits.hpp")).read()
    for name, value in (("kTileW = 32, kTileH = 8", _lib.MRT_SVGF_TILE == (32, 8)),
                        ("kRowTileW = 64, kRowTileRows = 4", _lib.MRT_SVGF_ROW_TILE == (64, 4)),
                        ("kTiledMaxStep = 16", _lib.MRT_SVGF_TILED_MAX_STEP == 16),
                        ("kMaxIterations = 8", _lib.MRT_SVGF_MAX_ITERATIONS == 8),
                        ("kMaxSquarings = 10", _lib.MRT_SVGF_MAX_SQUARINGS == 10)):
        assert name in text and value, name
    declared = set(re.findall(r"\b(mrt_svgf_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mrt_svgf.h")).read(), flags=re.S)))
    assert declared == {n for n, _, _ in _lib.SVGF_SYMBOLS} and all(hasattr(_lib.trace_lib(), n) for n in declared)


def test_the_accumulator_is_the_temporal_one_with_a_filter():
    """Without a device: the subclass adds `filter` and nothing public else, and refuses to filter before a frame."""
    torch = pytest.importorskip("torch")
    from mrt.svgf import SvgfAccumulator
    from mrt.temporal import TemporalAccumulator
    assert issubclass(SvgfAccumulator, TemporalAccumulator)
    assert [k for k in vars(SvgfAccumulator) if not k.startswith("_")] == ["filter"]
    acc = SvgfAccumulator(torch.device("cpu"))
    with pytest.raises(_lib.MrtError):
        acc.filter(torch.zeros((12, 4)))
