"""Temporal accumulation of path frames on one device (mrt_temporal_motion /
mrt_temporal_accumulate of include/mrt_temporal.h, which states the arithmetic):
TemporalAccumulator keeps the previous frame's guide and history and blends every new frame into
the running mean found where each pixel's surface point was then.

    world_to_screen(cam, w, h)       the matrix a frame is reprojected through: the inverse of the
                                     primary rays' nscreen-to-world matrix
    TemporalAccumulator.accumulate   one frame: guide, motion (where the geometry moved), blend

Nothing here takes a stream: every call runs on torch's current stream
(torch.cuda.current_stream(device)) and passes it down, so what is allocated and filled here is
ordered with the launches by construction. To run on a side stream s, wrap the call in
`with torch.cuda.stream(s)`. Nothing waits on the host. Bit-identical to the host statements
mrt.host.temporal_motion / temporal_accumulate given the same inputs.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .host import Camera
from .raygen import nscreen_to_world
from .tracer import RayBuffer

# The sweep's best (profiles/temporal.txt): of the settings that made none of the twelve
# measured sequences worse than its last frame alone, the one with the lowest mean MSE ratio. The
# longest running mean was not told apart by sequences of 8 frames and keeps its provisional value;
# the plane tolerance is a fraction of the diagonal of the scene's box.
MAX_HISTORY_DEFAULT = 32
NORMAL_COS_DEFAULT = 0.8
SIGMA_PLANE_FRACTION_DEFAULT = 1.0 / 50.0


def world_to_screen(cam: Camera, w: int, h: int) -> np.ndarray:
    """The world-to-screen matrix of a w x h frame of cam (float32 [16], column-major): the inverse
    of nscreen_to_world, taken in float64 and rounded to float32, negated as a whole where the point
    one unit in front of the camera gets a negative w (so that clip.w > 0 means in front). A singular
    matrix raises MrtError."""
    m = nscreen_to_world(cam, w, h).astype(np.float64).reshape(4, 4).T   # (r, c) at m[c * 4 + r]
    if not np.isfinite(m).all() or not np.isfinite(np.linalg.cond(m)) or np.linalg.cond(m) > 1.0e15:
        raise _lib.MrtError("world_to_screen: the camera's matrix is singular")
    inv = np.linalg.inv(m)
    f = np.asarray(cam.forward, np.float64)
    ahead = np.append(np.asarray(cam.position, np.float64) + f / max(np.linalg.norm(f), 1.0e-300), 1.0)
    if (inv @ ahead)[3] < 0:
        inv = -inv
    return np.ascontiguousarray(inv.T.reshape(16), np.float32)


class TemporalAccumulator:
    """Two guide / albedo / history sets of one frame size that ping-pong, the previous positions of
    a moving scene's hits, and the previous frame's matrix, subpixel and size."""

    def __init__(self, device=None):
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.trace_lib()
        self.w = self.h = 0
        self.sets: list[dict] = []
        self.prev_position: torch.Tensor | None = None
        self._cur = 0            # the set the next frame writes
        self._have_prev = False
        self._prev_matrix = np.zeros(16, np.float32)
        self._prev_subpixel = (0.5, 0.5)

    def _stream(self) -> int | None:
        return torch.cuda.current_stream(self.device).cuda_stream or None

    def reset(self) -> None:
        """Forget the history: the next frame starts a new running mean."""
        self._have_prev = False

    def _reserve(self, w: int, h: int) -> None:
        if (w, h) == (self.w, self.h) and self.sets:
            return
        if w < 1 or h < 1 or w * h > _lib.MRT_TEMPORAL_MAX_PIXELS:
            raise _lib.MrtError(f"an accumulated frame has 1 .. {_lib.MRT_TEMPORAL_MAX_PIXELS} pixels")
        n = w * h
        self.sets = [self._new_set(n) for _ in range(2)]
        self.prev_position = None
        self.w, self.h = w, h
        self._have_prev = False      # another frame size starts over

    def _new_set(self, n: int) -> dict:
        return {"guide": torch.empty((n, 8), dtype=torch.float32, device=self.device),
                "albedo": torch.empty((n, 4), dtype=torch.float32, device=self.device),
                "history": torch.empty((n, 4), dtype=torch.float32, device=self.device)}

    @property
    def current(self) -> dict:
        """The last accumulated frame's guide, albedo and history (the next frame's previous set)."""
        return self.sets[1 - self._cur]

    def accumulate(self, primary: RayBuffer, slot_to_id: torch.Tensor, normals: torch.Tensor, material: torch.Tensor,
                   w: int, h: int, cam_matrix, subpixel, image: torch.Tensor, pixels: torch.Tensor | None = None,
                   image_out: torch.Tensor | None = None, triangles: torch.Tensor | None = None,
                   vertices: torch.Tensor | None = None, prev_vertices: torch.Tensor | None = None,
                   max_history: int = MAX_HISTORY_DEFAULT, normal_cos: float = NORMAL_COS_DEFAULT,
                   sigma_plane: float = 1.0, variant: int = 0):
        """One w x h frame: its guide from the traced primary batch (mrt_denoise_features, with the
        current per-triangle normals and ABGR colours), the previous position of every hit where
        prev_vertices is given (with triangles int32 [nt, 3] and vertices float32 [nv, 3], all on the
        device), then the blend of `image` (float32 [w*h, 4], mrt_path_resolve's) into the history
        reprojected through the previous call's cam_matrix and subpixel. The result goes to pixels
        (int32 ABGR bits [w*h]) and / or image_out (float32 [w*h, 4], not `image` itself); with
        neither given, pixels is allocated. cam_matrix and subpixel are this frame's
        (world_to_screen, begin_frame's) and are remembered for the next call. The first call, a
        call after reset() and a call with another frame size reproject nothing. Returns
        (pixels, image_out). Runs on torch's current stream: to use a side stream s, call under
        `with torch.cuda.stream(s)`."""
        w, h = int(w), int(h)
        n = w * h
        if slot_to_id.numel() != primary.size:
            raise _lib.MrtError("slot_to_id must hold one pixel id per primary ray")
        if normals is None or material is None or normals.numel() != 3 * material.numel():
            raise _lib.MrtError("the accumulator needs one float32 normal and one ABGR colour per triangle")
        if image.dtype != torch.float32 or image.numel() != 4 * n or not image.is_contiguous():
            raise _lib.MrtError(f"the image is a contiguous float32 [{n}, 4] tensor")
        if (pixels is not None and pixels.numel() != n) or (image_out is not None and image_out.numel() != 4 * n):
            raise _lib.MrtError("pixels and image_out hold one entry per pixel of the frame")
        moving = prev_vertices is not None
        if moving and (triangles is None or vertices is None or vertices.numel() != prev_vertices.numel() or
                       triangles.numel() != 3 * material.numel()):
            raise _lib.MrtError("prev_vertices needs the triangles and as many current vertices")
        if moving and not (triangles.dtype == torch.int32 and triangles.is_contiguous() and
                           all(t.dtype == torch.float32 and t.is_contiguous() for t in (vertices, prev_vertices))):
            raise _lib.MrtError("triangles is a contiguous int32 [nt, 3] tensor, vertices and prev_vertices contiguous float32 [nv, 3]")
        m = np.ascontiguousarray(cam_matrix, np.float32).reshape(16)
        self._reserve(w, h)
        s = self._stream()
        cur, prev = self.sets[self._cur], self.sets[1 - self._cur]
        if primary.size != n:    # pixels without a slot: a miss's record
            cur["guide"].zero_()
            cur["albedo"].fill_(1.0)
        _lib.check(self.lib.mrt_denoise_features(primary.size, slot_to_id.data_ptr(), primary.rays.data_ptr(),
                                                 primary.results.data_ptr(), normals.data_ptr(), material.data_ptr(),
                                                 material.numel(), n, cur["guide"].data_ptr(), cur["albedo"].data_ptr(), s))
        if moving:
            if self.prev_position is None:
                self.prev_position = torch.zeros((n, 4), dtype=torch.float32, device=self.device)
            elif primary.size != n:
                self.prev_position.zero_()
            _lib.check(self.lib.mrt_temporal_motion(primary.size, slot_to_id.data_ptr(), primary.rays.data_ptr(),
                                                    primary.results.data_ptr(), triangles.data_ptr(), material.numel(),
                                                    vertices.data_ptr(), prev_vertices.data_ptr(), vertices.numel() // 3, n,
                                                    self.prev_position.data_ptr(), s))
        if pixels is None and image_out is None:
            pixels = torch.zeros(n, dtype=torch.int32, device=self.device)
        p = self._params()
        p.width, p.height, p.havePrev, p.maxHistory = w, h, int(self._have_prev), int(max_history)
        p.normalCos, p.sigmaPlane, p.variant = float(normal_cos), float(sigma_plane), int(variant)
        for i in range(16):
            p.prevWorldToScreen[i] = float(self._prev_matrix[i])
        p.prevSubpixel[0], p.prevSubpixel[1] = float(self._prev_subpixel[0]), float(self._prev_subpixel[1])
        p.image, p.guide, p.albedo = image.data_ptr(), cur["guide"].data_ptr(), cur["albedo"].data_ptr()
        p.prevPosition = self.prev_position.data_ptr() if moving else None
        p.prevGuide, p.prevHistory = prev["guide"].data_ptr(), prev["history"].data_ptr()
        p.history = cur["history"].data_ptr()
        p.imageOut = None if image_out is None else image_out.data_ptr()
        p.pixels = None if pixels is None else pixels.data_ptr()
        self._launch(p, cur, prev, s)
        self._cur = 1 - self._cur
        self._have_prev = True
        self._prev_matrix, self._prev_subpixel = m.copy(), (float(subpixel[0]), float(subpixel[1]))
        return pixels, image_out

    _params = _lib.TemporalParams    # what _launch takes: a subclass that carries more per pixel has more fields

    def _launch(self, p, cur: dict, prev: dict, s) -> None:
        """The frame's last launch, from the filled parameters and the two sets, on stream s."""
        _lib.check(self.lib.mrt_temporal_accumulate(C.byref(p), s))

    def history_length(self) -> torch.Tensor:
        """The current history's length per pixel (float32 [w*h]): a view of its w plane."""
        if not self._have_prev:
            raise _lib.MrtError("TemporalAccumulator.history_length before accumulate")
        return self.current["history"][:, 3]
