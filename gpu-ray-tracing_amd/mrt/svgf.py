"""Variance-guided filtering of accumulated path frames on one device (mrt_svgf_accumulate /
mrt_svgf_filter of include/mrt_svgf.h, which states the arithmetic): SvgfAccumulator is
mrt.temporal's TemporalAccumulator with the luminance moments carried along in the same launch,
and a filter whose colour weight follows each pixel's own variance.

    SvgfAccumulator.accumulate   TemporalAccumulator's: one frame's guide, motion and blend, with
                                 the moments (inherited; its last launch is mrt_svgf_accumulate)
    SvgfAccumulator.filter       the variance launch and the a-trous iterations over the frame
                                 accumulate just wrote

Nothing here takes a stream: every call runs on torch's current stream
(torch.cuda.current_stream(device)) and passes it down, so what is allocated and filled here is
ordered with the launches by construction. To run on a side stream s, wrap the call in
`with torch.cuda.stream(s)`. Nothing waits on the host. Bit-identical to the host statements
mrt.host.svgf_accumulate / svgf_filter given the same inputs.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .temporal import TemporalAccumulator

ITERATIONS_DEFAULT = 5         # Schied et al. 2017: a 5 x 5 kernel at steps 1 .. 16
NORMAL_SQUARINGS_DEFAULT = 7   # the normal weight's exponent 128, mrt.denoise's
# The sweep's best (profiles/svgf.txt): of the values around Schied et al.'s 4 that made none of the
# twelve measured sequences worse than its accumulated frame, the one with the lowest mean MSE ratio.
SIGMA_LUMINANCE_DEFAULT = 2.0


class SvgfAccumulator(TemporalAccumulator):
    """TemporalAccumulator's two sets with a moments record each, and the filter's two scratch images."""

    _params = _lib.SvgfAccumulateParams

    def __init__(self, device=None):
        super().__init__(device)
        self._scratch: list[torch.Tensor] = []

    def _new_set(self, n: int) -> dict:
        s = super()._new_set(n)
        s["moments"] = torch.empty((n, 4), dtype=torch.float32, device=self.device)
        return s

    def _launch(self, p, cur: dict, prev: dict, s) -> None:
        p.prevMoments, p.moments = prev["moments"].data_ptr(), cur["moments"].data_ptr()
        _lib.check(self.lib.mrt_svgf_accumulate(C.byref(p), s))

    def filter(self, image: torch.Tensor, pixels: torch.Tensor | None = None, image_out: torch.Tensor | None = None,
               variance_out: torch.Tensor | None = None, iterations: int = ITERATIONS_DEFAULT,
               sigma_luminance: float = SIGMA_LUMINANCE_DEFAULT, sigma_plane: float = 1.0,
               normal_squarings: int = NORMAL_SQUARINGS_DEFAULT, variant: int = 0):
        """Filter `image` (float32 [w*h, 4]: the image_out of the last accumulate) with that
        frame's guide, albedo and moments into pixels (int32 ABGR bits [w*h]) and / or image_out
        (float32 [w*h, 4], not `image` itself); with neither given, pixels is allocated.
        variance_out (float32 [w*h]) receives the filtered variance of the demodulated luminance.
        sigma_luminance is in standard deviations of that luminance, sigma_plane in scene units.
        Returns (pixels, image_out). Runs on torch's current stream: to use a side stream s, call
        under `with torch.cuda.stream(s)`."""
        if not self._have_prev:
            raise _lib.MrtError("SvgfAccumulator.filter before accumulate")
        n = self.w * self.h
        if image.dtype != torch.float32 or image.numel() != 4 * n or not image.is_contiguous():
            raise _lib.MrtError(f"the image is a contiguous float32 [{n}, 4] tensor")
        if (pixels is not None and pixels.numel() != n) or (image_out is not None and image_out.numel() != 4 * n) or \
                (variance_out is not None and (variance_out.numel() != n or variance_out.dtype != torch.float32)):
            raise _lib.MrtError("pixels, image_out and variance_out hold one entry per pixel of the frame")
        if pixels is None and image_out is None:
            pixels = torch.zeros(n, dtype=torch.int32, device=self.device)
        if not self._scratch or self._scratch[0].numel() != 4 * n:    # the first call, another frame size
            self._scratch = [torch.empty((n, 4), dtype=torch.float32, device=self.device) for _ in range(2)]
        cur = self.current
        p = _lib.SvgfFilterParams()
        p.width, p.height, p.iterations, p.normalSquarings = self.w, self.h, int(iterations), int(normal_squarings)
        p.sigmaLuminance, p.sigmaPlane, p.variant = float(sigma_luminance), float(sigma_plane), int(variant)
        p.image, p.guide, p.albedo, p.moments = (image.data_ptr(), cur["guide"].data_ptr(), cur["albedo"].data_ptr(),
                                                 cur["moments"].data_ptr())
        p.scratch[0], p.scratch[1] = self._scratch[0].data_ptr(), self._scratch[1].data_ptr()
        p.imageOut = None if image_out is None else image_out.data_ptr()
        p.pixels = None if pixels is None else pixels.data_ptr()
        p.varianceOut = None if variance_out is None else variance_out.data_ptr()
        _lib.check(self.lib.mrt_svgf_filter(C.byref(p), self._stream()))
        return pixels, image_out
