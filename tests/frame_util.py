"""Shared by tests/test_frame_edges.py and tests/test_gpu_frame_edges.py: the cameras, sizes and
bound of the primary-ray comparison with the float64 pinhole model (oracle/raygen_oracle.py
primary_dirs); the edge table of the AO/diffuse generator (a six-triangle scene whose normals are
ordinary, zero, NaN, axis-aligned and tied, crossed with hit distances, ids and directions at
their edges) and a NaN-aware comparison with the oracle; synthetic results and a colour table
for reconstruct and the hit count; and the ctypes mirrors of the reference's launcher inputs."""
import ctypes as C
import functools
import os

import numpy as np

import mrt
import raygen_oracle as RO

F = np.float32
INT_MIN, INT_MAX = -2**31, 2**31 - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera_signatures.txt")


# ---- A. cameras ----------------------------------------------------------------------------
def signature_cameras():
    """The 23 cameras of tests/golden/camera_signatures.txt as (label, Camera)."""
    out = []
    for line in open(GOLDEN):
        if line.startswith("#") or not line.strip():
            continue
        scene, sig = line.rstrip("\n").split("\t")
        out.append((f"sig{len(out)}-{scene}", mrt.Camera.from_signature(sig)))
    return out


def _unit(v):
    v = np.asarray(v, np.float64)
    return tuple(float(x) for x in (v / np.linalg.norm(v)).astype(np.float32))


# fov 1, 45, 90, 170; up is not perpendicular to forward in two of them (the camera's own
# orthogonalisation is part of what is checked), forward is not a unit vector in one
HAND_CAMERAS = [
    ("fov1", mrt.host.Camera((1.0, 2.0, 3.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 1.0, 0.1, 100.0)),
    ("fov45", mrt.host.Camera((-3.0, 0.5, 7.0), _unit((0.3, -0.2, -0.9)), (0.0, 1.0, 0.0), 45.0, 0.01, 500.0)),
    ("fov90", mrt.host.Camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 90.0, 0.1, 100.0)),
    ("fov170", mrt.host.Camera((0.5, -4.0, 2.0), (2.0, 2.0, 0.0), _unit((0.1, 0.0, 1.0)), 170.0, 1.0, 50.0)),
]
SIZES = [(1, 1), (2, 2), (7, 5), (5, 7), (64, 48), (48, 64), (128, 16)]
SUBPIXELS = [(0.5, 0.5), (0.0, 0.0), (0.25, 0.875)]

# Worst component error of the host's primary directions (float32 matrix chain and 4 x 4 inverse)
# against the float64 pinhole model over every camera, size and subpixel position below, measured
# on the CPU (test_frame_edges.py prints it): 1.80e-4, at the fourth conference signature, 5 x 7.
# The conference and sibenik cameras stand some ten units from the origin with near = 0.01: the
# inverse places a pixel's world point 0.02 in front of the camera, and subtracting the position
# cancels four digits (the other cameras stay below 4e-5). The bound is four times the worst.
CAMERA_ERR_MEASURED = 1.80e-4
CAMERA_BOUND = 4 * CAMERA_ERR_MEASURED
# A tenth of the pixel pitch 2 T / min(w, h) must stay above the bound, or half a pixel could hide
# in it. The 1-degree camera's pitch is below ten bounds at every size above 2 x 2: those five
# pairs are dropped (camera_cases), the camera stays at 1 x 1 and 2 x 2. Every other pair holds.


def pixel_pitch(cam, w, h):
    return 2.0 * np.tan(float(F(cam.fov)) * np.pi / 360.0) / min(w, h)


@functools.lru_cache(maxsize=None)
def all_cameras():
    return tuple(signature_cameras() + HAND_CAMERAS)


def camera_cases(cameras=None, sizes=SIZES):
    """(label, cam, w, h) of every pair whose pixel pitch is more than ten bounds."""
    cams = all_cameras() if cameras is None else cameras
    return [(label, cam, w, h) for label, cam in cams for w, h in sizes if 0.1 * pixel_pitch(cam, w, h) > CAMERA_BOUND]


def dropped_camera_cases():
    return [(label, w, h) for label, cam in all_cameras() for w, h in SIZES
            if not 0.1 * pixel_pitch(cam, w, h) > CAMERA_BOUND]


def model_rays(cam, w, h, subpixel, slot_to_id):
    """The model's directions in slot order."""
    return RO.primary_dirs(cam, w, h, *subpixel)[np.asarray(slot_to_id)]


def primary_error(rays, cam, w, h, subpixel, slot_to_id):
    """Worst component error of the rays' directions against the model; origin, tmin and tmax
    must be the camera's position, 0 and far exactly."""
    rays = np.asarray(rays, np.float32).reshape(-1, 8)
    assert len(rays) == w * h
    assert (rays[:, 0:3] == np.array(cam.position, np.float32)).all()
    assert (rays[:, 3] == 0).all() and (rays[:, 7] == F(cam.far)).all()
    return float(np.abs(rays[:, 4:7].astype(np.float64) - model_rays(cam, w, h, subpixel, slot_to_id)).max())


# ---- B. the AO / diffuse generator's edge table ------------------------------------------------
EDGE_T = [0.0, 5e-5, 1e-4, 1.0001e-4, 1.0, np.inf, np.nan, -1.0, 1e-39]
EDGE_IDS = [-1, 0, 1, 2, 3, 4, 5, 6, -2, INT_MIN, INT_MAX]
EDGE_DIRS = [(0.0, 0.0, -1.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (-0.0, 0.0, -1.0), (0.6, 0.0, -0.8)]
EDGE_SEEDS = [1, 0xFFFFFFF0]   # the second: seed + task wraps at task 16
EDGE_SAMPLES = [1, 3, 256]
EDGE_MAX_DIST = 10.0
NORMAL_KINDS = ["z-facing", "zero", "NaN", "-y", "|x| == |y|", "|y| == |z|"]


@functools.lru_cache(maxsize=None)
def edge_scene():
    """(vertices, triangles, normals) of the six triangles, read-only. Every edge is a small
    integer or half-integer vector, so the cross products are exact and the ties are ties."""
    tris = np.array([
        [(-2, -2, 0), (4, -2, 0), (-2, 4, 0)],            # normal (0, 0, 1)
        [(0, 0, 2), (1, 0, 2), (2, 0, 2)],                # collinear: the cross product is 0, the normal 0
        [(np.nan, 1, 3), (1, 1, 3), (0, 2, 3)],           # a NaN vertex: the normal is NaN
        [(-2, 2, -1), (4, 2, -1), (-2, 2, 5)],            # normal (0, -1, 0)
        [(3, -1, -1), (0, 2, -1), (3, -1, 3)],            # normal (1, 1, 0) / sqrt 2
        [(-2, -1, 2.5), (2, -1, 2.5), (-2, 1, 0.5)],      # normal (0, 1, 1) / sqrt 2
    ], np.float32)
    v = np.ascontiguousarray(tris.reshape(-1, 3))
    t = np.arange(18, dtype=np.int32).reshape(6, 3)
    n = mrt.Scene.from_arrays(v, t).arrays()[2]
    # a fixture that drifts fails here instead of passing vacuously
    assert np.array_equal(n[0], [0, 0, 1]) and np.array_equal(n[1], [0, 0, 0]) and np.isnan(n[2]).all()
    assert np.array_equal(n[3], [0, -1, 0])
    assert n[4, 0] == n[4, 1] > 0 and n[4, 2] == 0 and n[5, 1] == n[5, 2] > 0 and n[5, 0] == 0
    for a in (v, t, n):
        a.setflags(write=False)
    return v, t, n


def _inputs(rows):
    """rows of (origin, direction, id, t) -> (rays float32 [n, 8], results int32 [n, 4])."""
    rays = np.zeros((len(rows), 8), np.float32)
    res = np.zeros((len(rows), 4), np.int32)
    for k, (o, d, i, t) in enumerate(rows):
        rays[k] = (*o, 0.0, *d, 100.0)
        res[k, 0] = i
        res[k, 1:2].view(np.float32)[0] = t
    return rays, res


@functools.lru_cache(maxsize=None)
def edge_inputs():
    """The 9 x 11 x 5 = 495 input rays (t outermost, then id, then direction), read-only, and a
    label (t index, id index, direction index) per ray. A ray starts one unit before the point
    (0.25, 0.25, 0) of triangle 0; the fourth direction's origin has a denormal y, which the
    device flushes and the host keeps."""
    rows, labels = [], []
    for ti, t in enumerate(EDGE_T):
        for ii, i in enumerate(EDGE_IDS):
            for di, d in enumerate(EDGE_DIRS):
                o = [0.25 - d[0], 0.25 - d[1], 0.0 - d[2]]
                if di == 3:
                    o[1] = 1e-39
                rows.append((o, d, i, t))
                labels.append((ti, ii, di))
    rays, res = _inputs(rows)
    labels = np.array(labels)
    for a in (rays, res, labels):
        a.setflags(write=False)
    return rays, res, labels


TIE_NORMALS = [(1, 0, 1), (1, 0, -1), (-1, 0, 1), (1, 1, 1), (-1, 1, 1), (1, -1, -1), (-1, -1, 1)]


@functools.lru_cache(maxsize=None)
def tie_scene():
    """Triangles whose normals tie on |x| == |z| and on all three axes, which the six-triangle table
    does not hold: the only ties where the order of the kernel's two tests (z first, then x)
    decides the perpendicular. (vertices, triangles, normals), read-only."""
    tris = []
    for n in TIE_NORMALS:
        n = np.array(n)
        e1 = np.array([n[1], -n[0], 0]) if (n[0] or n[1]) else np.array([1, 0, 0])
        e2 = np.cross(n, e1)   # e1 x e2 = n |e1|^2, in integers
        v0 = np.array([1, 2, 3])
        tris.append([v0, v0 + e1, v0 + e2])
    v = np.ascontiguousarray(np.array(tris, np.float32).reshape(-1, 3))
    t = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    nrm = mrt.Scene.from_arrays(v, t).arrays()[2]
    for got, want in zip(nrm, TIE_NORMALS):
        assert np.array_equal(np.sign(got), want) and len(set(np.abs(got[np.array(want) != 0]))) == 1
    for a in (v, t, nrm):
        a.setflags(write=False)
    return v, t, nrm


@functools.lru_cache(maxsize=None)
def tie_inputs():
    """Each tie triangle seen from above and from below (the normal as it is, and flipped)."""
    rows = [((0.25, 0.25, -d[2]), d, i, 1.0) for i in range(len(TIE_NORMALS)) for d in ((0.0, 0.0, -1.0), (0.0, 0.0, 1.0))]
    rays, res = _inputs(rows)
    rays.setflags(write=False)
    res.setflags(write=False)
    return rays, res


def frame_seeds(seeds, batch_inputs, n):
    """Per input ray p of a frame cut into batches of batch_inputs rays, the seed s with
    s + p == seeds[p // batch_inputs] + p % batch_inputs (mod 2^32): the oracle hashes seed + task,
    so one call with these covers the whole frame of RayGen::batching."""
    p = np.arange(n, dtype=np.int64)
    k = p // batch_inputs
    return ((np.asarray(seeds, np.int64)[k] - k * batch_inputs) & 0xFFFFFFFF).astype(np.uint64)


def same_bits_or_nan(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def compare_ao(got, want, dir_tol):
    """Generated rays float32 [n, 8] against the oracle's dict: origin, tmin and tmax bit for bit
    (a NaN equal to a NaN: the bits of a NaN an operation makes differ between x86 and gfx950),
    directions within dir_tol where the oracle's are finite and NaN exactly where the oracle's
    are. Returns the counts that show what the comparison rested on."""
    got = np.asarray(got, np.float32).reshape(-1, 8)
    assert len(got) == len(want["dir"])
    bad = ~same_bits_or_nan(got[:, 0:3], want["origin"])
    assert not bad.any(), f"origin differs at rays {np.nonzero(bad.any(1))[0][:8]}"
    assert np.array_equal(got[:, 3].view(np.uint32), want["tmin"].view(np.uint32))
    bad = got[:, 7].view(np.uint32) != want["tmax"].astype(np.float32).view(np.uint32)
    assert not bad.any(), f"tmax differs at rays {np.nonzero(bad)[0][:8]}"
    wd = want["dir"]
    nan = np.isnan(wd)
    assert np.isfinite(wd[~nan]).all()
    assert np.array_equal(np.isnan(got[:, 4:7]), nan), \
        f"NaN pattern differs at rays {np.nonzero((np.isnan(got[:, 4:7]) != nan).any(1))[0][:8]}"
    err = np.abs(got[:, 4:7].astype(np.float64) - wd)
    worst = float(err[~nan].max()) if (~nan).any() else 0.0
    assert worst <= dir_tol, f"direction error {worst:.3g} at ray {np.nonzero((err > dir_tol) & ~nan)[0][:8]}"
    finite = ~nan.any(1)
    zero = finite & (wd == 0).all(1)
    return {"rays": len(got), "nan_dir": int(nan.any(1).sum()), "zero_dir": int(zero.sum()),
            "unit_dir": int((finite & ~zero).sum()), "nan_origin": int(np.isnan(want["origin"]).any(1).sum()),
            "max_dir_err": worst}


# ---- C. synthetic results ----------------------------------------------------------------------
def results(ids):
    r = np.zeros((len(ids), 4), np.int32)
    r[:, 0] = ids
    return r


@functools.lru_cache(maxsize=None)
def colour_tables():
    """(material, shaded): 64 ABGR colours each. Entries 0..35 take every channel through the
    bytes 0, 1, 127, 128, 254, 255 (red and green in all 36 pairs), the rest are random. Read-only."""
    rng = np.random.default_rng(64)
    edge = np.array([0, 1, 127, 128, 254, 255], np.uint32)
    i = np.arange(36)
    out = []
    for k in range(2):
        ch = rng.integers(0, 256, (64, 4)).astype(np.uint32)
        ch[:36, 0] = edge[i % 6]
        ch[:36, 1] = edge[i // 6]
        ch[:36, 2] = edge[(i + i // 6 + k) % 6]
        ch[:36, 3] = edge[(2 * i + i // 6 + k) % 6]
        table = ch[:, 0] | ch[:, 1] << 8 | ch[:, 2] << 16 | ch[:, 3] << 24
        table.setflags(write=False)
        out.append(table)
    return tuple(out)


# ---- the reference's launcher inputs (include/mrt.h) ----------------------------------------------
class RayGenPrimaryInput(C.Structure):
    """RayGenKernels.hh:40-51 (mrt.h mrt_raygen_primary_input)."""
    _fields_ = [("origin", C.c_float * 3), ("nscreenToWorld", C.c_float * 16), ("w", C.c_int32), ("h", C.c_int32),
                ("maxDist", C.c_float), ("rays", C.c_void_p), ("idToSlot", C.c_void_p), ("slotToID", C.c_void_p),
                ("indexToPixel", C.c_void_p)]


class RayGenAOInput(C.Structure):
    """RayGenKernels.hh:55-68 (mrt.h mrt_raygen_ao_input)."""
    _fields_ = [("firstInputSlot", C.c_int32), ("numInputRays", C.c_int32), ("numSamples", C.c_int32),
                ("maxDist", C.c_float), ("randomSeed", C.c_uint32), ("inRays", C.c_void_p),
                ("inResults", C.c_void_p), ("outRays", C.c_void_p), ("outIDToSlot", C.c_void_p),
                ("outSlotToID", C.c_void_p), ("normals", C.c_void_p)]


class CountHitsInput(C.Structure):
    """RendererKernels.hh:65-70 (mrt.h mrt_count_hits_input)."""
    _fields_ = [("numRays", C.c_int32), ("rayResults", C.c_void_p), ("raysPerThread", C.c_int32)]
