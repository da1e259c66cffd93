"""The path frame's denoiser on the CPU: mrth_denoise_features and mrth_denoise_filter
(csrc/host/denoise.cpp over csrc/denoise_common.hpp), the CPU statements of mrt_denoise_features /
mrt_denoise_filter, against the independent numpy model of tests/denoise_util.py, bit for bit (a
NaN equal to a NaN); known answers that pin the weights, the step and the halo; the quality
condition on the floor-and-occluder scene; the plan (csrc/denoise_plan.cpp) through
lib/denoise_driver; the host functions as a stand-alone program under -fsanitize=address,undefined
(tests/cpp/denoise_driver.cpp; nothing is preloaded); and the host argument checks. None needs a
device."""
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
import path_util as P
import test_path as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gpu-ray-tracing_amd")
F = np.float32
DRIVER = os.path.join(PKG, "lib", "denoise_driver")
SETTINGS = [(0, 7), (1, 0), (5, 7), (8, 10), (5, 1)]   # (iterations, normalSquarings): 0, 1, 5, 8 and 0, 1, 7, 10


# ---------------------------------------------------------------- 1. the host statements against the model
@pytest.mark.parametrize("frame", D.FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("kind", D.GUIDE_KINDS)
def test_host_filter_equals_the_model(frame, kind):
    w, h = frame
    seen = {"nan": 0, "changed": 0}
    for iterations, squarings in SETTINGS:
        image, guide, albedo = D.make_case(w, h, kind, seed=w * 131 + h)
        kw = dict(iterations=iterations, sigma_color=0.7, sigma_plane=0.3, normal_squarings=squarings)
        got = mrt.host.denoise_filter(image, guide, albedo, w, h, **kw)
        want = D.Model.denoise_filter(image, guide, albedo, w, h, **kw)
        assert D.same_floats(got[0], want[0]), (iterations, squarings)
        assert np.array_equal(got[1], want[1]), (iterations, squarings)
        assert D.same_floats(got[0][:, 3], image[:, 3])            # w is carried
        only_px = mrt.host.denoise_filter(image, guide, albedo, w, h, want_image=False, **kw)
        only_img = mrt.host.denoise_filter(image, guide, albedo, w, h, want_pixels=False, **kw)
        assert only_px[0] is None and only_img[1] is None
        assert np.array_equal(only_px[1], got[1]) and D.same_floats(only_img[0], got[0])
        seen["nan"] += int(np.isnan(got[0]).sum())
        seen["changed"] += int((got[0][:, :3] != image[:, :3]).sum())
    if kind == "misses":    # nothing is filtered and nothing modulated: the image comes back
        assert seen["changed"] == seen["nan"]
    elif w * h > 1:
        assert seen["changed"] > 0
    assert w * h < 11 or seen["nan"] > 0   # the table's NaN and inf colours reached the arithmetic


@pytest.mark.parametrize("shape", [(1, 1), (300, 400), (400, 400), (5000, 5003)], ids=str)
def test_host_features_equal_the_model(shape):
    slots, pixels = shape
    normals, material = D.feature_tables()
    s2i, rays, res = D.feature_inputs(slots, pixels, seed=slots)
    sentinel_g, sentinel_a = np.full((pixels, 8), 7.5, F), np.full((pixels, 4), 7.5, F)
    got = mrt.host.denoise_features(s2i, rays, res, normals, material, pixels, sentinel_g.copy(), sentinel_a.copy())
    want = D.Model.denoise_features(s2i, rays, res, normals, material, pixels, sentinel_g.copy(), sentinel_a.copy())
    assert D.same_floats(got[0], want[0]) and D.same_floats(got[1], want[1])
    named = np.zeros(pixels, bool)
    named[s2i[(s2i >= 0) & (s2i < pixels)]] = True
    assert (got[0][~named] == 7.5).all() and (got[1][~named] == 7.5).all()   # skipped slots and unnamed pixels: untouched
    assert (got[0][named, 7] == 0).all() and (got[1][named, 3] == 1).all()
    if slots > 1:
        hit = got[0][named, 3] == 1
        assert hit.any() and (~hit).any() and np.isnan(got[0][named]).any()
        assert (got[1][named][~hit] == 1).all() and (got[0][named][~hit] == 0).all()


# ---------------------------------------------------------------- 2. known answers
def plane_guide(w, h, z=0.0):
    n = w * h
    ys, xs = np.divmod(np.arange(n), w)
    g = np.zeros((n, 8), F)
    g[:, 2], g[:, 3], g[:, 4], g[:, 5], g[:, 6] = 1.0, 1.0, xs * F(0.25), ys * F(0.25), z
    return g


def ones(n):
    return np.ones((n, 4), F)


@pytest.mark.parametrize("impl", [mrt.host, D.Model], ids=["host", "model"])
def test_known_answer_a_constant_image_on_a_plane_comes_back(impl):
    w, h = 23, 19
    image = np.tile(np.array([0.3, 0.6, 0.9, 0.5], F), (w * h, 1))
    albedo = ones(w * h)
    albedo[:, :3] = np.array([191, 127, 255], F) * (F(1) / F(255))
    for iterations in (1, 5):
        out, _ = impl.denoise_filter(image, plane_guide(w, h), albedo, w, h, iterations=iterations, sigma_color=0.5,
                                     sigma_plane=0.1)
        assert np.abs(out / image - 1.0).max() <= 1e-6


@pytest.mark.parametrize("impl", [mrt.host, D.Model], ids=["host", "model"])
@pytest.mark.parametrize("squarings", [1, 7])
def test_known_answer_nothing_crosses_a_right_angle(impl, squarings):
    """A floor (normal +z) beside a wall (normal +x) whose colours are 1e30: the weight across the
    edge is exactly 0 (the normal term is 0, the colour term 1 / inf = 0), so every floor pixel comes
    out as with the wall removed (its pixels misses), bit for bit."""
    w, h = 24, 9
    rng = np.random.default_rng(4)
    guide = plane_guide(w, h)
    wall = (np.arange(w * h) % w) >= 14
    guide[wall, 0:3] = (1.0, 0.0, 0.0)
    image = (rng.random((w * h, 4))).astype(F)
    image[wall, :3] = 1e30
    without = guide.copy()
    without[wall] = 0.0
    kw = dict(iterations=4, sigma_color=1.0, sigma_plane=0.5, normal_squarings=squarings)
    a, _ = impl.denoise_filter(image, guide, ones(w * h), w, h, **kw)
    b, _ = impl.denoise_filter(image, without, ones(w * h), w, h, **kw)
    assert np.array_equal(a[~wall].view(np.uint32), b[~wall].view(np.uint32))
    assert (a[~wall, :3] != image[~wall, :3]).any() and (a[~wall, :3] < 2.0).all()


@pytest.mark.parametrize("impl", [mrt.host, D.Model], ids=["host", "model"])
def test_known_answer_misses_neither_change_nor_leak(impl):
    w, h = 17, 15
    image, guide, albedo = D.make_case(w, h, "checker", seed=3, edges=False)
    miss = guide[:, 3] == 0
    loud = image.copy()
    loud[miss, :3] = 1e30
    kw = dict(iterations=5, sigma_color=0.7, sigma_plane=0.3)
    a, _ = impl.denoise_filter(loud, guide, albedo, w, h, **kw)
    b, _ = impl.denoise_filter(image, guide, albedo, w, h, **kw)
    assert np.array_equal(a[miss].view(np.uint32), loud[miss].view(np.uint32))
    assert np.array_equal(a[~miss].view(np.uint32), b[~miss].view(np.uint32))


@pytest.mark.parametrize("impl", [mrt.host, D.Model], ids=["host", "model"])
@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_known_answer_an_impulse_spreads_by_the_step_and_the_halo(impl, iterations):
    """With the colour term off (sigmaColor^2 overflows) on one plane the filter is the B3 spline
    cascade: after N iterations an impulse is nonzero exactly within +-2 (2^N - 1) of its pixel."""
    w, h, cx, cy = 35, 33, 17, 16
    image = np.zeros((w * h, 4), F)
    image[cy * w + cx, :3] = 1.0
    out, _ = impl.denoise_filter(image, plane_guide(w, h), ones(w * h), w, h, iterations=iterations, sigma_color=1e30,
                                 sigma_plane=1.0)
    reach = 2 * (2 ** iterations - 1)
    ys, xs = np.divmod(np.arange(w * h), w)
    inside = (np.abs(xs - cx) <= reach) & (np.abs(ys - cy) <= reach)
    assert (~inside).any()
    assert (out[inside, :3] > 0).all() and (out[~inside, :3] == 0).all()


@pytest.mark.parametrize("impl", [mrt.host, D.Model], ids=["host", "model"])
@pytest.mark.parametrize("distance,sigma", [(0.5, 0.25), (1.0, 1.0), (0.01, 0.2)])
def test_known_answer_the_weight_between_two_parallel_planes(impl, distance, sigma):
    """Two pixels on parallel planes D apart, colours 0 and 1, the colour term off: pixel 0 becomes
    (h1 h0 wz) / (h0 h0 + h1 h0 wz), so wz = 0.375 out / (0.25 (1 - out)) = 1 / (1 + (D / sigma)^2)."""
    guide = plane_guide(2, 1)
    guide[1, 6] = distance
    image = np.array([[0, 0, 0, 1], [1, 1, 1, 1]], F)
    out, _ = impl.denoise_filter(image, guide, ones(2), 2, 1, iterations=1, sigma_color=1e30, sigma_plane=sigma)
    o = float(out[0, 0])
    wz = 0.375 * o / (0.25 * (1.0 - o))
    want = 1.0 / (1.0 + (distance / sigma) ** 2)
    assert abs(wz / want - 1.0) <= 1e-6, (wz, want)


# ---------------------------------------------------------------- 3. quality, as a condition
QW, QH = 64, 48


def occluder_frames():
    """The floor-and-occluder scene of test_path's known answers seen by a camera, 64 x 48, depth 1,
    every trace by the oracle, rendered by the host path functions at S = 2 and S = 256."""
    tris = T.rect(0.0, -4.0, 4.0, -3.0, 5.0) + T.fan(1.0, 1.0, (0.3, 0.4))
    scene, bufs, normals, material = T.world_of(tris)
    d = np.array([0.0, 5.0, -3.5])
    cam = mrt.host.Camera((0.0, -5.0, 4.0), tuple(d / np.linalg.norm(d)), (0.0, 0.0, 1.0), 45.0, 0.01, 100.0)
    prim, s2i = mrt.primary_rays(cam, QW, QH)
    trace = T.oracle_trace(bufs)
    pres = trace(prim, False)
    images = {}
    for samples, seed in ((2, 11), (256, 12)):
        _, image, _ = P.render_frame(mrt.host, trace, prim, pres, s2i, QW * QH, normals, material, samples, 1, [seed],
                                     QW * QH, True, T.KNOWN, want_image=True)
        images[samples] = image
    guide, albedo = mrt.host.denoise_features(s2i, prim, pres, normals, material, QW * QH)
    v = scene.arrays()[0].astype(np.float64)
    return images, guide, albedo, float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))


def test_quality_the_denoised_frame_is_nearer_the_converged_one():
    """MSE against the S = 256 frame: the denoised S = 2 frame's is smaller than the S = 2 frame's.
    Run on the host with the defaults (5 iterations, mrt.denoise's sigma_color and fraction of the
    diagonal); profiles/denoise.txt holds the figures this prints."""
    from mrt.denoise import SIGMA_COLOR_DEFAULT, SIGMA_PLANE_FRACTION_DEFAULT
    images, guide, albedo, diagonal = occluder_frames()
    hit = guide[:, 3] != 0
    assert 500 < hit.sum() and 0.0 < diagonal
    out, _ = mrt.host.denoise_filter(images[2], guide, albedo, QW, QH, iterations=5, sigma_color=SIGMA_COLOR_DEFAULT,
                                     sigma_plane=diagonal * SIGMA_PLANE_FRACTION_DEFAULT)
    ref = images[256][:, :3].astype(np.float64)
    before = float(((images[2][:, :3] - ref) ** 2).mean())
    after = float(((out[:, :3] - ref) ** 2).mean())
    print(f"occluder 64x48 S=2 against S=256: MSE {before:.6g} -> {after:.6g} (ratio {after / before:.3f})")
    assert before > 0 and after < before


# ---------------------------------------------------------------- 4. the plan
def bits(x):
    return int(np.array(x, F).view(np.uint32))


def plan(w, h, iterations, squarings, sigma_color, sigma_plane, variant=0):
    out = subprocess.run([DRIVER, "plan", str(w), str(h), str(iterations), str(squarings), str(bits(sigma_color)),
                          str(bits(sigma_plane)), str(variant)], capture_output=True, text=True, check=True).stdout
    lines = [[int(x) for x in line.split()] for line in out.splitlines()]
    return lines[0], lines[1:]


def test_the_plan_checks_in_the_documented_order():
    bad, big = _lib.MRT_ERR_INVALID_ARG, _lib.MRT_ERR_TOO_LARGE
    ok = (64, 48, 5, 7, 1.0, 1.0)

    def rc(**kw):
        names = ("w", "h", "iterations", "squarings", "sigma_color", "sigma_plane")
        args = dict(zip(names, ok))
        variant = kw.pop("variant", 0)
        args.update(kw)
        return plan(*[args[n] for n in names], variant)[0][0]
    assert rc() == 0
    for kw in (dict(w=0), dict(h=0), dict(w=-1), dict(iterations=-1), dict(squarings=-1), dict(sigma_color=0.0),
               dict(sigma_color=-1.0), dict(sigma_color=np.nan), dict(sigma_plane=0.0), dict(sigma_plane=np.nan),
               dict(variant=3), dict(variant=-1)):
        assert rc(**kw) == bad, kw
    for kw in (dict(w=8193, h=8192), dict(iterations=9), dict(squarings=11)):
        assert rc(**kw) == big, kw
    assert rc(w=8192, h=8192, iterations=8, squarings=10) == 0 and rc(w=1 << 26, h=1) == 0 and rc(w=1, h=1 << 26) == 0
    assert rc(sigma_color=np.inf, sigma_plane=np.inf) == 0 and rc(sigma_color=1e-45) == 0
    # shape before limits: a bad shape with a size above the limit is a bad shape
    assert rc(iterations=9, sigma_plane=0.0) == bad and rc(w=0, squarings=11) == bad

    def features(*args):
        return [int(x) for x in subprocess.run([DRIVER, "plan-features", *map(str, args)], capture_output=True,
                                               text=True, check=True).stdout.split()]
    assert features(0, 5, 9) == [0, 1, 0] and features(9, 5, 0)[:2] == [0, 1]
    assert features(1, 0, 1) == [0, 0, 1] and features(257, 5, 9) == [0, 0, 2]
    assert features(1 << 26, 1, 1 << 26) == [0, 0, 1 << 18]
    for args in ((-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, 1, (1 << 26) + 1)):
        assert features(*args)[0] == bad, args
    for args in (((1 << 26) + 1, 1, 1), (1, 1, (1 << 26) + 1)):
        assert features(*args)[0] == big, args


def test_the_plan_sizes_the_grids_and_the_tiles():
    tw, th = _lib.MRT_DENOISE_TILE
    head, steps = plan(97, 83, 8, 7, 1.0, 1.0, variant=1)
    assert head[:2] == [0, 8] and [s[0] for s in steps] == [1 << k for k in range(8)]
    for s in steps:   # direct: ceil(w / 32) x ceil(h / 8) tiles
        assert s[1:5] == [0, 4 * 11, 4, 11]
    assert (tw, th) == (32, 8)
    _, steps = plan(97, 83, 8, 7, 1.0, 1.0, variant=2)
    for step, tiled, grid, tx, ty, residues, lds, _ in steps:
        assert tiled == (step <= 16)
        if tiled:   # 64 columns x 4 rows of one residue; min(step, h) residues; 8 staged rows of 64 + 4 step records
            rows = -(-83 // step)
            assert (tx, residues, ty, grid) == (2, step, step * -(-rows // 4), 2 * step * -(-rows // 4))
            assert lds == 8 * (64 + 4 * step) * 48 <= 64 * 1024
    _, steps = plan(70, 3, 5, 7, 1.0, 1.0, variant=2)    # fewer rows than the step: one residue per row
    assert [s[5] for s in steps[:5]] == [1, 2, 3, 3, 3] and [s[4] for s in steps[:5]] == [1, 2, 3, 3, 3]
    head, steps = plan(5, 5, 0, 7, 1.0, 1.0)
    assert head[1] == 1 and steps[0][1:5] == [0, 1, 1, 1]       # iterations 0: one launch of the direct geometry
    # the default variant stages exactly the steps the measurements chose, a subset of what fits
    _, default = plan(97, 83, 8, 7, 1.0, 1.0, variant=0)
    _, fits = plan(97, 83, 8, 7, 1.0, 1.0, variant=2)
    assert all(d[1] <= f[1] for d, f in zip(default, fits))


@pytest.mark.parametrize("sigma", [1.0, 0.37, 3e19, 1e30, 3.4e38, 1e-19, 1e-22, 1e-30, 1e-45])
def test_the_plan_constants_where_the_square_overflows_and_underflows(sigma):
    head, steps = plan(8, 8, 8, 7, sigma, 0.3)
    inv_plane, inv_color2 = D.constants(8, sigma, 0.3)
    assert head[2] == bits(inv_plane)
    assert [s[7] for s in steps] == [bits(x) for x in inv_color2]
    if sigma >= 1e30:
        assert inv_color2[0] == 0.0          # s^2 overflows: the colour term is off
    if sigma <= 1e-30:
        assert np.isinf(inv_color2[7])       # s^2 underflows to 0


# ---------------------------------------------------------------- 5. the same code under the sanitizers
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host compiler"
    exe = str(tmp_path_factory.mktemp("denoise_san") / "denoise_driver_san")
    sources = [os.path.join(REPO, "tests", "cpp", "denoise_driver.cpp"), os.path.join(PKG, "csrc", "host", "denoise.cpp"),
               os.path.join(PKG, "csrc", "host", "host_error.cpp"), os.path.join(PKG, "csrc", "denoise_plan.cpp")]
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

    normals, material = D.feature_tables()
    for slots, pixels in ((1, 1), (300, 400), (5000, 5003)):
        s2i, rays, res = D.feature_inputs(slots, pixels, seed=slots)
        g, a = str(tmp_path / "guide.bin"), str(tmp_path / "albedo.bin")
        run(["features", str(pixels), put("s2i.bin", s2i), put("rays.bin", rays), put("res.bin", res),
             put("normals.bin", normals), put("material.bin", material), g, a], "features")
        want = mrt.host.denoise_features(s2i, rays, res, normals, material, pixels)
        assert D.same_floats(np.fromfile(g, F).reshape(-1, 8), want[0]) and D.same_floats(np.fromfile(a, F).reshape(-1, 4), want[1])
    for (w, h), kind, (iterations, squarings) in (((1, 1), "hits", (5, 7)), ((1, 7), "checker", (8, 10)), ((7, 1), "mixed", (2, 1)),
                                                  ((17, 15), "mixed", (0, 7)), ((17, 15), "zero-normals", (1, 0)),
                                                  ((97, 83), "mixed", (8, 7)), ((97, 83), "checker", (3, 7))):
        image, guide, albedo = D.make_case(w, h, kind, seed=w + h)
        words = np.array([w, h, iterations, squarings, bits(0.7), bits(0.3)], np.uint32)
        for want_image, want_pixels in ((True, True), (True, False), (False, True)):
            oi, op = str(tmp_path / "out.bin"), str(tmp_path / "px.bin")
            run(["filter", put("scalars.bin", words), put("image.bin", image), put("guide.bin", guide),
                 put("albedo.bin", albedo), oi if want_image else "-", op if want_pixels else "-"], f"filter {w}x{h} {kind}")
            want = mrt.host.denoise_filter(image, guide, albedo, w, h, iterations, 0.7, 0.3, squarings)
            if want_image:
                assert D.same_floats(np.fromfile(oi, F).reshape(-1, 4), want[0])
            if want_pixels:
                assert np.array_equal(np.fromfile(op, np.uint32), want[1])


# ---------------------------------------------------------------- 6. the argument checks, the names
def test_host_exports_refuse_bad_arguments_and_write_nothing():
    lib = _lib.host_lib()
    w, h = 5, 4
    image, guide, albedo = D.make_case(w, h, "hits", seed=1)
    out, px, s0, s1 = np.full((w * h, 4), 7.5, F), np.full(w * h, 77, np.uint32), np.zeros((w * h, 4), F), np.zeros((w * h, 4), F)

    def params(**kw):
        p = _lib.DenoiseParams()
        p.width, p.height, p.iterations, p.normalSquarings, p.sigmaColor, p.sigmaPlane = w, h, 5, 7, 1.0, 1.0
        p.image, p.guide, p.albedo = image.ctypes.data, guide.ctypes.data, albedo.ctypes.data
        p.scratch[0], p.scratch[1], p.imageOut, p.pixels = s0.ctypes.data, s1.ctypes.data, out.ctypes.data, px.ctypes.data
        for k, v in kw.items():
            if k.startswith("scratch"):
                p.scratch[int(k[-1])] = v
            else:
                setattr(p, k, v)
        return p
    assert lib.mrth_denoise_filter(None) == 1
    for kw in (dict(width=0), dict(height=-1), dict(iterations=-1), dict(iterations=9), dict(normalSquarings=11),
               dict(sigmaColor=0.0), dict(sigmaPlane=float("nan")), dict(variant=3), dict(image=None), dict(guide=None),
               dict(albedo=None), dict(scratch0=None), dict(scratch1=None), dict(imageOut=None, pixels=None)):
        assert lib.mrth_denoise_filter(C.byref(params(**kw))) == 1, kw
        assert _lib.host_lib().mrth_last_error()
        assert (out == 7.5).all() and (px == 77).all(), kw
    # a scratch image the iteration count does not use may be missing
    assert lib.mrth_denoise_filter(C.byref(params(iterations=2, scratch1=None))) == 0
    assert lib.mrth_denoise_filter(C.byref(params(iterations=1, scratch0=None, scratch1=None, pixels=None))) == 0
    assert (out != 7.5).all() and (px != 77).any()
    with pytest.raises(_lib.MrtError):
        mrt.host.denoise_filter(image, guide, albedo, w + 1, h)
    normals, material = D.feature_tables()
    s2i, rays, res = D.feature_inputs(9, 12, seed=2)
    g, a = np.full((12, 8), 7.5, F), np.full((12, 4), 7.5, F)
    args = [9, s2i.ctypes.data, rays.ctypes.data, res.ctypes.data, normals.ctypes.data, material.ctypes.data, 8, 12,
            g.ctypes.data, a.ctypes.data]
    for at, v in ((0, -1), (6, -1), (7, -1), (0, (1 << 26) + 1), (1, None), (2, None), (3, None), (4, None), (5, None),
                  (8, None), (9, None)):
        bad = list(args)
        bad[at] = v
        assert lib.mrth_denoise_features(*bad) == 1, at
        assert (g == 7.5).all() and (a == 7.5).all(), at
    for at, v in ((0, 0), (7, 0)):   # no slot, no pixel: fine, nothing written
        empty = list(args)
        empty[at] = v
        assert lib.mrth_denoise_features(*empty) == 0 and (g == 7.5).all()
    assert lib.mrth_denoise_features(*args) == 0 and (g != 7.5).any()


def test_the_python_constants_are_the_headers():
    text = open(os.path.join(PKG, "csrc", "denoise_limits.hpp")).read()
    for name, value in (("kMaxPixels = 1 << 26", _lib.MRT_DENOISE_MAX_PIXELS == 1 << 26),
                        ("kMaxIterations = 8", _lib.MRT_DENOISE_MAX_ITERATIONS == 8),
                        ("kMaxSquarings = 10", _lib.MRT_DENOISE_MAX_SQUARINGS == 10),
                        ("kTileW = 32, kTileH = 8", _lib.MRT_DENOISE_TILE == (32, 8)),
                        ("kRowTileW = 64, kRowTileRows = 4", _lib.MRT_DENOISE_ROW_TILE == (64, 4))):
        assert name in text and value, name
    assert C.sizeof(_lib.DenoiseParams) == 32 + 7 * C.sizeof(C.c_void_p)
