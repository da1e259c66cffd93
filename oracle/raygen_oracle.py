"""TEST INFRASTRUCTURE ONLY (imported by tests/, never by the product path).

An independent numpy restatement of the reference's AO / diffuse ray generator
rayGenAOKernel (src/rt/ray/RayGenKernels.cu:117-227) and of its Jenkins hash
(RayGenKernels.cu:36-47), written from the reference source without reusing the
product's raygen_common.hpp, so the device generator (csrc/raygen_kernel.hip) is
checked against something other than its own header.

And primary_dirs: the primary ray directions of a pinhole camera in float64, written from
the geometry (no camera matrix, no inverse), so the matrix chain of host/raygen.cpp and
raygen_common.hpp's primary_ray have a ground truth.

Per input ray i of a batch (task index i, input slot first + i):
  origin  = o + d * fmaxf(t - 1e-4, 0)                       (:138-139, float32 mul then add; 0 for a NaN t)
  normal  = normals[id] (or (1,0,0) for a miss), flipped to face the viewer  (:143-147)
  perp    = the normal's perpendicular on its largest axis, times rcp(length) with rcp(0) = 0;
            biperp = n x perp                                 (:151-158)
  angle   = 2 pi * jenkins(seed + i) * 2^-32                   (:162-167)
  sample s: Halton(2,3) point (s + 1) warped onto the cosine hemisphere,
            dir = normalize(x t0 + y t1 + z n), tmin = 0, tmax = maxDist (or -1 for a miss)

Returned in float64 next to the float32 fields that are exact restatements
(origin, tmin, tmax, the normal and the hash angle); the directions involve
cosf/sinf, which differ between the device and libm, so tests compare them with a
tolerance.
"""
from __future__ import annotations

import numpy as np

PI_F32 = np.float32(3.14159265358979323846)


def jenkins_mix(a, b, c):
    """RayGenKernels.cu:36-47 on uint32 arrays (wrapping)."""
    def step(x, y, z, shift, left):
        x = (x - y - z) & 0xFFFFFFFF
        x ^= ((z << shift) & 0xFFFFFFFF) if left else (z >> shift)
        return x
    a = step(a, b, c, 13, False); b = step(b, c, a, 8, True); c = step(c, a, b, 13, False)
    a = step(a, b, c, 12, False); b = step(b, c, a, 16, True); c = step(c, a, b, 5, False)
    a = step(a, b, c, 3, False); b = step(b, c, a, 10, True); c = step(c, a, b, 15, False)
    return a, b, c


def hash_angle(seed, n: int) -> np.ndarray:
    """float32 rotation angle of tasks 0..n-1 (RayGenKernels.cu:162-167). seed: one uint32, or one
    per task (a frame of several batches, each with its own seed and task numbers)."""
    a = (np.asarray(seed, np.uint64) + np.arange(n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    b = np.full(n, 0x9E3779B9, np.uint64)
    c = np.full(n, 0x9E3779B9, np.uint64)
    a, b, c = jenkins_mix(a, b, c)
    a, b, c = jenkins_mix(a, b, c)
    two_pi = np.float32(2.0) * PI_F32
    return (two_pi * c.astype(np.float32)) * np.float32(2.0 ** -32)


def halton23(i: int):
    """Base-2 / base-3 radical inverses of i + 1 in the kernel's float32 accumulation order."""
    x, xadd, h = np.float32(0), np.float32(1), i + 1
    while h:
        xadd = np.float32(xadd * np.float32(0.5))
        if h & 1:
            x = np.float32(x + xadd)
        h >>= 1
    y, yadd, h = np.float32(0), np.float32(1), i + 1
    third = np.float32(1.0) / np.float32(3.0)
    while h:
        yadd = np.float32(yadd * third)
        y = np.float32(y + np.float32(h % 3) * yadd)
        h //= 3
    return x, y


def fw_max(a, b):
    """The framework's max, (a > b) ? a : b: a NaN in a gives b, a NaN in b stays."""
    return np.where(a > b, a, b)


def flush(a):
    """float32 values with denormals flushed to a zero of their sign (a device built FTZ)."""
    a = np.asarray(a, np.float32)
    return np.where(np.abs(a) < np.finfo(np.float32).tiny, np.copysign(np.float32(0), a), a).astype(np.float32)


def rcp(x):
    """The framework's rcp: 1 / x, and 0 at 0 (Math.hh; a NaN stays a NaN)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x != 0, 1.0 / np.where(x != 0, x, 1.0), 0.0)


def normalized(v):
    """VectorBase::normalized: v * rcp(length), so a zero vector stays zero instead of becoming NaN."""
    with np.errstate(invalid="ignore", over="ignore"):
        return v * rcp(np.sqrt((v * v).sum(axis=1, keepdims=True)))


def primary_dirs(cam, w: int, h: int, jx: float = 0.5, jy: float = 0.5) -> np.ndarray:
    """Primary ray directions of a pinhole camera, float64 [w * h, 3] indexed by pixel id py * w + px,
    written from the geometry (no matrix, no inverse): the field of view fov_deg spans the shorter
    side of the frame (fitToView(-1, 2, size), Math.cc:66-75), x grows along right = forward x up,
    y along the camera's up, row 0 is the bottom row. cam: position / forward / up / fov (float32
    field values); (jx, jy) the sample position inside the pixel."""
    f = np.array([np.float32(v) for v in cam.forward], np.float64)
    up = np.array([np.float32(v) for v in cam.up], np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    T = np.tan(float(np.float32(cam.fov)) * np.pi / 360.0)
    m = min(w, h)
    pixel = np.arange(w * h)
    nx = 2.0 * (pixel % w + float(jx)) / w - 1.0
    ny = 2.0 * (pixel // w + float(jy)) / h - 1.0
    d = f[None, :] + r[None, :] * (nx * (w / m) * T)[:, None] + u[None, :] * (ny * (h / m) * T)[:, None]
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def ao_rays(in_rays: np.ndarray, in_results: np.ndarray, normals: np.ndarray, num_samples: int, max_dist: float,
            seed: int, ftz: bool = False):
    """Restated rayGenAOKernel over one batch. in_rays float32 [n, 8], in_results int32 [n, 4],
    normals float32 [tris, 3]. Returns a dict of arrays (per output ray unless noted).

    At the edges of its inputs the kernel's own operations decide, and this follows them:
      * the back-off is fmaxf(t - eps, 0), which is 0 for a NaN t: where(t - eps > 0, t - eps, 0);
      * normalize is v * rcp(length) with rcp(0) = 0: a zero normal gives a zero perpendicular and
        zero directions, not NaN;
      * the maxima over |normal| are the framework's (a > b) ? a : b.
    An id outside [-1, numTris) is read out of bounds by the reference; the product's documented rule
    (include/mrt.h, mrt_raygen_ao) is the contract here: normal (1, 0, 0), and only id == -1 is a miss.
    ftz: the device flushes denormals; flush the inputs and the float32 intermediates of the fields
    compared bit for bit (origin)."""
    rays = np.ascontiguousarray(in_rays, np.float32).reshape(-1, 8)
    res = np.ascontiguousarray(in_results).view(np.int32).reshape(-1, 4)
    normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    n = len(rays)
    fz = flush if ftz else (lambda a: np.asarray(a, np.float32))
    o, d = fz(rays[:, 0:3]), fz(rays[:, 4:7])
    t = fz(res[:, 1].view(np.float32))
    ids = res[:, 0]
    with np.errstate(invalid="ignore", over="ignore"):
        tb = fz(t - np.float32(1e-4))
        back = np.where(tb > 0, tb, np.float32(0.0)).astype(np.float32)
        origin = fz(o + fz(d * back[:, None]))
    miss = ids == -1
    inside = (ids >= 0) & (ids < len(normals))
    nrm = np.tile(np.array([1, 0, 0], np.float32), (n, 1))
    nrm[inside] = fz(normals[ids[inside]])
    with np.errstate(invalid="ignore", over="ignore"):
        facing = (((nrm[:, 0] * d[:, 0]).astype(np.float32) + (nrm[:, 1] * d[:, 1]).astype(np.float32))
                  .astype(np.float32) + (nrm[:, 2] * d[:, 2]).astype(np.float32)).astype(np.float32)
        nrm = np.where((facing > 0)[:, None], -nrm, nrm).astype(np.float32)
        na = np.abs(nrm)
        nm = fw_max(fw_max(na[:, 0], na[:, 1]), na[:, 2])
        perp = np.stack([nrm[:, 1], -nrm[:, 0], np.zeros(n, np.float32)], 1)
        z_axis = nm == na[:, 2]
        x_axis = ~z_axis & (nm == na[:, 0])
        perp[z_axis] = np.stack([np.zeros(z_axis.sum(), np.float32), nrm[z_axis, 2], -nrm[z_axis, 1]], 1)
        perp[x_axis] = np.stack([-nrm[x_axis, 2], np.zeros(x_axis.sum(), np.float32), nrm[x_axis, 0]], 1)
        perp64 = normalized(perp.astype(np.float64))
        n64 = nrm.astype(np.float64)
        biperp = np.cross(n64, perp64)
        angle = hash_angle(seed, n).astype(np.float64)
        t0 = perp64 * np.cos(angle)[:, None] + biperp * np.sin(angle)[:, None]
        t1 = perp64 * -np.sin(angle)[:, None] + biperp * np.cos(angle)[:, None]
        dirs = np.empty((n, num_samples, 3))
        for s in range(num_samples):
            hx, hy = halton23(s)
            a2 = 2.0 * np.pi * float(hy)
            r = np.sqrt(float(hx))
            x, y = r * np.cos(a2), r * np.sin(a2)
            z = np.sqrt(max(0.0, 1.0 - x * x - y * y))
            dirs[:, s] = normalized(x * t0 + y * t1 + z * n64)
    out = {
        "origin": np.repeat(origin, num_samples, axis=0),
        "tmin": np.zeros(n * num_samples, np.float32),
        "tmax": np.repeat(np.where(miss, np.float32(-1.0), np.float32(max_dist)), num_samples),
        "normal": np.repeat(nrm, num_samples, axis=0),
        "dir": dirs.reshape(-1, 3),
        "angle": np.repeat(hash_angle(seed, n), num_samples),
    }
    return out
