"""The path frame's denoiser on one device (mrt_denoise_features / mrt_denoise_filter of
include/mrt.h, which states the arithmetic): Denoiser owns the guide, albedo and scratch buffers
of one frame size and runs the edge-avoiding a-trous filter over a resolved float image.

    set_frame(primary, slot_to_id, normals, material, w, h)   the frame's features, from its traced
                                                              primary batch
    run(image, pixels=..., image_out=...)                     the filter

Both are enqueued on the stream with no host sync. Bit-identical to the host statements
mrt.host.denoise_features / denoise_filter given the same inputs.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import torch

from . import _lib
from .tracer import RayBuffer, _stream_ptr

ITERATIONS_DEFAULT = 5         # Dammertz et al. 2010: a 5 x 5 kernel at steps 1 .. 16
NORMAL_SQUARINGS_DEFAULT = 7   # the normal weight's exponent 128
# The sweep's best (profiles/denoise.txt): of the settings that made none of the seven
# measured frames worse, the one with the lowest mean MSE ratio. The colour sigma is in units of the
# demodulated image, sigma_plane a fraction of the scene box's diagonal (which moved the mean by
# less than 0.002: the sweep does not tell the three fractions apart).
SIGMA_COLOR_DEFAULT = 0.5
SIGMA_PLANE_FRACTION_DEFAULT = 1.0 / 50.0


class Denoiser:
    """The guide records, albedos and two ping-pong images of one frame size, and the two calls."""

    def __init__(self, device=None):
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.trace_lib()
        self.w = self.h = 0
        self.guide = self.albedo = None
        self.scratch: list[torch.Tensor] = []
        self._have_frame = False

    def _reserve(self, w: int, h: int) -> None:
        if (w, h) == (self.w, self.h) and self.guide is not None:
            return
        if w < 1 or h < 1 or w * h > _lib.MRT_DENOISE_MAX_PIXELS:
            raise _lib.MrtError(f"a denoised frame has 1 .. {_lib.MRT_DENOISE_MAX_PIXELS} pixels")
        n = w * h
        self.guide = torch.empty((n, 8), dtype=torch.float32, device=self.device)
        self.albedo = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        self.scratch = [torch.empty((n, 4), dtype=torch.float32, device=self.device) for _ in range(2)]
        self.w, self.h = w, h

    def set_frame(self, primary: RayBuffer, slot_to_id: torch.Tensor, normals: torch.Tensor, material: torch.Tensor,
                  w: int, h: int, stream=None) -> None:
        """The features of a w x h frame from its traced primary batch (rays and closest-hit
        results), the pixel of every slot, and the current per-triangle normals (float32 [nt, 3])
        and ABGR colours (int32 [nt]) on the device. Pixels no slot names are misses. Passing
        stream= alone is enough: the fill for those pixels runs on that stream."""
        if slot_to_id.numel() != primary.size:
            raise _lib.MrtError("slot_to_id must hold one pixel id per primary ray")
        if normals is None or material is None or normals.numel() != 3 * material.numel():
            raise _lib.MrtError("the denoiser needs one float32 normal and one ABGR colour per triangle")
        self._reserve(int(w), int(h))
        s = _stream_ptr(stream)
        if primary.size != w * h:    # pixels without a slot: a miss's record
            with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
                self.guide.zero_()
                self.albedo.fill_(1.0)
        _lib.check(self.lib.mrt_denoise_features(primary.size, slot_to_id.data_ptr(), primary.rays.data_ptr(),
                                                 primary.results.data_ptr(), normals.data_ptr(), material.data_ptr(),
                                                 material.numel(), w * h, self.guide.data_ptr(), self.albedo.data_ptr(), s))
        self._have_frame = True

    def run(self, image: torch.Tensor, pixels: torch.Tensor | None = None, image_out: torch.Tensor | None = None,
            iterations: int = ITERATIONS_DEFAULT, sigma_color: float = SIGMA_COLOR_DEFAULT, sigma_plane: float = 1.0,
            normal_squarings: int = NORMAL_SQUARINGS_DEFAULT, stream=None):
        """Filter `image` (float32 [w*h, 4], mrt_path_resolve's) into pixels (int32 ABGR bits
        [w*h]) and / or image_out (float32 [w*h, 4]); with neither given, pixels is allocated.
        Returns (pixels, image_out). Neither may be `image` itself. sigma_color is in units of the
        demodulated image, sigma_plane in scene units (Renderer.denoise derives it from the scene's box).
        Passing stream= alone is enough: pixels made here are zeroed on that stream."""
        if not self._have_frame:
            raise _lib.MrtError("Denoiser.run before set_frame")
        n = self.w * self.h
        if image.dtype != torch.float32 or image.numel() != 4 * n or not image.is_contiguous():
            raise _lib.MrtError(f"the image is a contiguous float32 [{n}, 4] tensor")
        if pixels is None and image_out is None:
            with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
                pixels = torch.zeros(n, dtype=torch.int32, device=self.device)
        if (pixels is not None and pixels.numel() != n) or (image_out is not None and image_out.numel() != 4 * n):
            raise _lib.MrtError("pixels and image_out hold one entry per pixel of the frame")
        p = _lib.DenoiseParams()
        p.width, p.height, p.iterations, p.normalSquarings = self.w, self.h, int(iterations), int(normal_squarings)
        p.sigmaColor, p.sigmaPlane = float(sigma_color), float(sigma_plane)
        p.image, p.guide, p.albedo = image.data_ptr(), self.guide.data_ptr(), self.albedo.data_ptr()
        p.scratch[0], p.scratch[1] = self.scratch[0].data_ptr(), self.scratch[1].data_ptr()
        p.imageOut = None if image_out is None else image_out.data_ptr()
        p.pixels = None if pixels is None else pixels.data_ptr()
        _lib.check(self.lib.mrt_denoise_filter(C.byref(p), _stream_ptr(stream)))
        return pixels, image_out

