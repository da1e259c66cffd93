"""The frame path on the CPU against references that do not share its code (tests/frame_util.py):

  * primary rays (mrt.primary_rays: raygen_common.hpp primary_ray on the matrix of
    host/raygen.cpp) against a float64 pinhole model written from the geometry
    (raygen_oracle.primary_dirs), on the 23 reference signatures and four hand cameras, seven
    sizes and three subpixel positions; hand-derived directions with no model at all; near / far
    moved without moving a direction;
  * the AO / diffuse generator (mrt.ao_rays) against the numpy restatement of the reference's
    kernel (raygen_oracle.ao_rays) on the edge table: zero, NaN and tied normals, t from 0 to
    NaN, ids outside the scene, dot(n, d) == +-0, a seed that wraps.
"""
import dataclasses

import numpy as np
import pytest

import mrt
import frame_util as U
import raygen_oracle as RO


# ---- A. primary rays ---------------------------------------------------------------------------
def test_the_bound_is_four_times_the_measured_error_and_a_tenth_of_a_pixel_at_most():
    """Measures what frame_util.CAMERA_ERR_MEASURED records, over exactly the cases tested."""
    worst, where = 0.0, None
    for label, cam, w, h in U.camera_cases():
        for sp in U.SUBPIXELS:
            rays, s2i = mrt.primary_rays(cam, w, h, subpixel=sp)
            e = U.primary_error(rays, cam, w, h, sp, s2i)
            if e > worst:
                worst, where = e, (label, w, h, sp)
        assert 0.1 * U.pixel_pitch(cam, w, h) > U.CAMERA_BOUND
    print(f"worst component error of the host's primary directions: {worst:.3e} at {where}")
    # the recorded figure is the measured one (a libm whose tanf differs by an ulp moves the
    # cancellation's error by a few per cent at most), not a loose one
    assert 0.9 * U.CAMERA_ERR_MEASURED <= worst <= 1.05 * U.CAMERA_ERR_MEASURED
    dropped = U.dropped_camera_cases()
    print(f"dropped (pitch below ten bounds): {dropped}")
    assert {label for label, _, _ in dropped} == {"fov1"} and len(dropped) == 5
    assert len(U.camera_cases()) == 27 * 7 - 5


@pytest.mark.parametrize("label,cam", U.all_cameras(), ids=[label for label, _ in U.all_cameras()])
def test_primary_rays_match_the_pinhole_model(label, cam):
    cases = U.camera_cases(((label, cam),))
    assert cases
    for _, _, w, h in cases:
        table = mrt.pixel_table(w, h)
        assert np.array_equal(np.sort(table), np.arange(w * h))
        for sp in U.SUBPIXELS:
            rays, s2i = mrt.primary_rays(cam, w, h, subpixel=sp)
            assert np.array_equal(s2i, table)
            assert U.primary_error(rays, cam, w, h, sp, s2i) <= U.CAMERA_BOUND
            assert np.abs(np.linalg.norm(rays[:, 4:7].astype(np.float64), axis=1) - 1).max() < 1e-6


def test_the_model_tells_the_errors_it_is_there_for():
    """A mirrored image, a flipped row order, the field of view on the long side, half a pixel and a
    square-pixel aspect each move some direction of the model by far more than the bound, at every
    tested size with more than one pixel: the bound cannot hide them."""
    cam = U.HAND_CAMERAS[1][1]
    for w, h in U.SIZES[1:]:
        good = RO.primary_dirs(cam, w, h)
        grid = good.reshape(h, w, 3)
        wrong = {"mirrored": grid[:, ::-1], "rows flipped": grid[::-1],
                 "half a pixel": RO.primary_dirs(cam, w, h, 0.0, 0.5).reshape(h, w, 3)}
        for name, bad in wrong.items():
            assert np.abs(bad - grid).max() > 10 * U.CAMERA_BOUND, (name, w, h)
        if w != h:
            T, m, M = np.tan(np.radians(cam.fov) / 2), min(w, h), max(w, h)
            # the corner pixel's tangent along the long side: (M / m) T (1 - 1 / M) with the field of view on
            # the short side, T (1 - 1 / M) with it on the long side
            assert (M / m - 1) * T * (1 - 1 / M) > 10 * U.CAMERA_BOUND


def _dirs_by_pixel(cam, w, h):
    rays, s2i = mrt.primary_rays(cam, w, h)
    out = np.empty((w * h, 3), np.float32)
    out[s2i] = rays[:, 4:7]
    return out.reshape(h, w, 3)


def test_hand_derived_directions():
    """Camera at the origin looking down -z, up +y, fov 90: tan(45 deg) = 1, so the short side of
    the frame spans [-1, 1] at distance 1. 2 x 2: pixel centres at +-0.5 in x and y, x negative
    for px = 0 (left), y negative for py = 0 (row 0 is the bottom row). 4 x 2: the long side spans
    [-2, 2], centres at -1.5, -0.5, 0.5, 1.5 in x and +-0.5 in y. 2 x 4: the same in y."""
    cam = U.HAND_CAMERAS[2][1]
    assert (cam.position, cam.forward, cam.up, cam.fov) == ((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 90.0)

    def unit(x, y):
        v = np.array([x, y, -1.0])
        return v / np.linalg.norm(v)

    for w, h, xs, ys in ((2, 2, (-0.5, 0.5), (-0.5, 0.5)), (4, 2, (-1.5, -0.5, 0.5, 1.5), (-0.5, 0.5)),
                         (2, 4, (-0.5, 0.5), (-1.5, -0.5, 0.5, 1.5))):
        got = _dirs_by_pixel(cam, w, h)
        for py, y in enumerate(ys):
            for px, x in enumerate(xs):
                assert np.abs(got[py, px] - unit(x, y)).max() < 1e-6, (w, h, px, py)
    # 1 x 1 is the forward direction itself
    assert np.abs(_dirs_by_pixel(cam, 1, 1)[0, 0] - [0, 0, -1]).max() < 1e-6


@pytest.mark.parametrize("label,cam", [U.all_cameras()[0], U.all_cameras()[5], U.all_cameras()[14]] + U.HAND_CAMERAS[1:],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_near_and_far_move_no_direction(label, cam):
    """The clip planes cancel out of a pinhole camera's directions; in float32 they leave the
    inverse's rounding, which the bound covers."""
    for w, h in ((7, 5), (64, 48)):
        base, _ = mrt.primary_rays(cam, w, h)
        for near, far in ((0.05, 500.0), (1.0, 50.0)):
            moved, _ = mrt.primary_rays(dataclasses.replace(cam, near=near, far=far), w, h)
            assert np.abs(moved[:, 4:7] - base[:, 4:7]).max() <= U.CAMERA_BOUND
            assert (moved[:, 7] == np.float32(far)).all()


# ---- B. the AO / diffuse generator at its edge inputs ----------------------------------------------
def test_the_oracle_at_the_edges_it_was_corrected_for():
    """Hand answers for the two places where the restatement used to differ from the kernel."""
    _, _, normals = U.edge_scene()
    rays = np.array([[0.25, 0.25, 1, 0, 0, 0, -1, 100]] * 3, np.float32)
    res = U.results([0, 1, 0])
    res[:, 1].view(np.float32)[:] = [np.nan, 1.0, 1.0]
    out = RO.ao_rays(rays, res, normals, 1, 10.0, 1)
    # a NaN t: fmaxf(NaN - eps, 0) = 0, the origin is the input ray's
    assert np.array_equal(out["origin"][0], [0.25, 0.25, 1.0])
    # a zero normal: rcp(0) = 0, the direction is (0, 0, 0), not NaN
    assert np.array_equal(out["dir"][1], [0.0, 0.0, 0.0]) and np.array_equal(out["normal"][1], [0, 0, 0])
    # an ordinary row beside them: backed off 1e-4, a unit direction in the upper hemisphere
    assert np.array_equal(out["origin"][2], [0.25, 0.25, np.float32(1.0) - np.float32(np.float32(1.0) - np.float32(1e-4))])
    assert abs(np.linalg.norm(out["dir"][2]) - 1) < 1e-12 and out["dir"][2][2] > 0


def test_ids_outside_the_scene_follow_the_documented_rule():
    """include/mrt.h (mrt_raygen_ao): an id outside [0, numTris) takes the normal (1, 0, 0); only -1
    is a miss (tmax = -1)."""
    _, _, normals = U.edge_scene()
    ids = [-1, 6, -2, U.INT_MIN, U.INT_MAX]
    rays = np.array([[0.25, 0.25, 1, 0, 0.6, 0, -0.8, 100]] * len(ids), np.float32)
    res = U.results(ids)
    res[:, 1].view(np.float32)[:] = 1.0
    out = RO.ao_rays(rays, res, normals, 1, 10.0, 1)
    assert np.array_equal(out["normal"], [[-1, 0, 0]] * len(ids))     # flipped to face the ray's origin
    assert out["tmax"].tolist() == [-1.0, 10.0, 10.0, 10.0, 10.0]
    scene = mrt.Scene.from_arrays(*U.edge_scene()[:2])
    host = mrt.ao_rays(rays, res, scene, 10.0, 1, 1)
    assert host[:, 7].tolist() == [-1.0, 10.0, 10.0, 10.0, 10.0]


@pytest.mark.parametrize("samples", U.EDGE_SAMPLES)
@pytest.mark.parametrize("seed", U.EDGE_SEEDS)
def test_host_ao_rays_equal_the_oracle_on_the_edge_table(seed, samples):
    v, t, normals = U.edge_scene()
    rays, res, labels = U.edge_inputs()
    assert len(rays) == 495
    host = mrt.ao_rays(rays, res, mrt.Scene.from_arrays(v, t), U.EDGE_MAX_DIST, samples, seed)
    want = RO.ao_rays(rays, res, normals, samples, U.EDGE_MAX_DIST, seed)
    stats = U.compare_ao(host, want, 4e-6)
    print(f"seed {seed:#x} S {samples}: {stats}")
    # the table is not vacuous: most rows are finite unit directions
    assert stats["unit_dir"] > 0.8 * stats["rays"] and stats["nan_dir"] == stats["zero_dir"] == 45 * samples
    unit = np.linalg.norm(want["dir"], axis=1)
    assert np.allclose(unit[~np.isnan(unit) & (unit != 0)], 1.0, atol=1e-12)
    # every group of the table holds finite rows; the NaN rows are the NaN normal's and nothing else's
    per_ray = np.isnan(want["dir"]).any(1).reshape(-1, samples).all(1)
    assert np.array_equal(per_ray, labels[:, 1] == U.EDGE_IDS.index(2))
    if seed == U.EDGE_SEEDS[1]:
        assert seed + len(rays) > 2**32   # the hash input wraps inside the table


def test_host_ao_rays_equal_the_oracle_on_tied_normals():
    """|x| == |z| and three-way ties: the kernel tests z, then x, then takes y."""
    v, t, normals = U.tie_scene()
    rays, res = U.tie_inputs()
    host = mrt.ao_rays(rays, res, mrt.Scene.from_arrays(v, t), U.EDGE_MAX_DIST, 3, 1)
    stats = U.compare_ao(host, RO.ao_rays(rays, res, normals, 3, U.EDGE_MAX_DIST, 1), 4e-6)
    assert stats["unit_dir"] == stats["rays"] == 3 * len(rays)


def test_frame_seeds_restate_the_batching():
    """One oracle call with per-ray seeds equals the batches' own calls."""
    _, _, normals = U.edge_scene()
    rays, res, _ = U.edge_inputs()
    seeds = [7, 0xFFFFFFFE, 123456789]
    whole = RO.ao_rays(rays, res, normals, 2, 10.0, U.frame_seeds(seeds, 200, len(rays)))
    for k, s in enumerate(seeds):
        part = RO.ao_rays(rays[200 * k:200 * (k + 1)], res[200 * k:200 * (k + 1)], normals, 2, 10.0, s)
        assert np.array_equal(part["dir"], whole["dir"][400 * k:400 * (k + 1)], equal_nan=True)
