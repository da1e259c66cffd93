"""Multi-bounce diffuse paths on one device (mrt_path_extend / _accumulate / _resolve of
include/mrt.h, which states the arithmetic): PathIntegrator owns the buffers of one batch of paths
and runs its vertices through a Tracer.

Per vertex b = 0..depth of a batch:
    extend(b)        one vertex step of every slot: light sample, pending contribution, bounce ray,
                     new state, the survivors compacted in stable order (or in place); then one
                     4-byte readback of the live count, because a trace takes its ray count on the host
    trace_shadow()   any-hit trace of the live shadow rays
    accumulate()     radiance += pending where the light was reached
    trace_bounce()   closest-hit trace of the live bounce rays (b < depth)
resolve() then averages a primary's S radiances into its pixel. Bit-identical to the host
statements mrt.host.path_extend / path_accumulate / path_resolve given the same trace results.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .host import path_params
from .tracer import RayBuffer, Tracer, _on_stream, _stream_ptr

MAX_PATHS = _lib.MRT_PATH_MAX_PATHS
MAX_DEPTH = _lib.MRT_PATH_MAX_DEPTH


class PathIntegrator:
    """The ping-pong ray, result and state buffers, the shadow batch, the pending contributions
    and the radiance accumulator of one batch of paths, and the calls that advance them."""

    def __init__(self, tracer: Tracer, device=None):
        self.tracer = tracer
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.trace_lib()
        self._capacity = 0
        self.num_paths = self.num_slots = self.live = 0
        self.vertex = -1
        self.stats: list[int] = []   # live counts per vertex of the current batch

    def _reserve(self, n: int) -> None:
        if n <= self._capacity:
            return
        dev = self.device

        def f32(cols):
            return torch.empty((n, cols), dtype=torch.float32, device=dev)

        def i32(cols):
            return torch.empty((n, cols), dtype=torch.int32, device=dev)
        self.rays, self.results, self.state = [f32(8), f32(8)], [i32(4), i32(4)], [i32(4), i32(4)]
        self.shadow_rays, self.shadow_results, self.pending, self.radiance = f32(8), i32(4), f32(4), f32(4)
        self.live_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self._capacity = n

    def begin(self, primary: RayBuffer, first: int, count: int, num_samples: int, depth: int, seed: int,
              normals: torch.Tensor, material: torch.Tensor, light_pos, light_radius: float,
              light_color=(1.0, 1.0, 1.0), sky=(0.2, 0.4, 0.8), max_dist: float = 1.0e30, compact: bool = False) -> None:
        """Start the paths of the traced input rays [first, first + count) of `primary`,
        num_samples each. normals: float32 [nt, 3], material: int32 [nt] ABGR, on the device."""
        n = count * num_samples
        if first < 0 or count < 0 or first + count > primary.size:
            raise _lib.MrtError(f"input range [{first}, {first + count}) outside the {primary.size}-ray batch")
        if not 0 <= depth <= MAX_DEPTH or num_samples < 1 or n > MAX_PATHS:
            raise _lib.MrtError(f"a path batch takes depth 0..{MAX_DEPTH} and at most {MAX_PATHS} paths")
        if normals is None or material is None or normals.numel() != 3 * material.numel():
            raise _lib.MrtError("a path batch needs one float32 normal and one ABGR colour per triangle")
        self._reserve(max(n, 1))
        self.primary, self.first, self.count = primary, first, count
        self.num_samples, self.depth, self.compact = num_samples, depth, bool(compact)
        self.normals, self.material = normals, material
        self._scalars = dict(depth=depth, num_samples=num_samples, seed=seed, light_pos=light_pos,
                             light_radius=light_radius, light_color=light_color, sky=sky, max_dist=max_dist,
                             compact=compact)
        self.num_paths = self.num_slots = self.live = n
        self.vertex, self._cur, self.stats = -1, 0, []
        self.radiance[:max(n, 1)].zero_()

    def extend_async(self, vertex: int, stream=None) -> None:
        """The vertex step over the current slots, enqueued with no host sync. The bounce rays and
        states land in the other half of the ping-pong pair, which trace_bounce makes the current
        one; the live count lands in self.live_count (device int32). Every launch goes to `stream`
        and nothing is allocated here, so passing stream= alone is enough."""
        n, cur, nxt = self.num_slots, self._cur, 1 - self._cur
        p = path_params(vertex, **self._scalars)
        p.triNormals, p.triMaterialColor, p.numTris = self.normals.data_ptr(), self.material.data_ptr(), self.material.numel()
        p.numSlots, p.numPaths = n, self.num_paths
        if vertex == 0:
            p.inRays = self.primary.rays.data_ptr() + 32 * self.first
            p.inResults = self.primary.results.data_ptr() + 16 * self.first
            p.inState = None
        else:
            p.inRays, p.inResults, p.inState = (self.rays[cur].data_ptr(), self.results[cur].data_ptr(),
                                                self.state[cur].data_ptr())
        p.outShadowRays, p.outPending = self.shadow_rays.data_ptr(), self.pending.data_ptr()
        p.outRays, p.outState = self.rays[nxt].data_ptr(), self.state[nxt].data_ptr()
        p.radiance, p.liveCount = self.radiance.data_ptr(), self.live_count.data_ptr()
        _lib.check(self.lib.mrt_path_extend(C.byref(p), _stream_ptr(stream)))
        self.vertex = vertex

    def extend(self, vertex: int, stream=None) -> int:
        """extend_async, then one blocking 4-byte readback of the live count, which it returns: a
        trace takes its ray count on the host. The readback runs ON `stream`, after the step, so
        passing stream= alone is enough, whatever torch's current stream is."""
        self.extend_async(vertex, stream)
        with _on_stream(stream):
            self.live = int(self.live_count.item()) if self.num_slots else 0
        self.stats.append(self.live)
        if self.compact:
            self.num_slots = self.live
        return self.live

    def shadow_batch(self) -> RayBuffer:
        m = self.num_slots
        return RayBuffer(self.shadow_rays[:m], need_closest_hit=False, device=self.device,
                         results=self.shadow_results[:m], secondary=True)

    def bounce_batch(self) -> RayBuffer:
        m, nxt = self.num_slots, 1 - self._cur
        return RayBuffer(self.rays[nxt][:m], need_closest_hit=True, device=self.device, results=self.results[nxt][:m],
                         secondary=True)

    def trace_shadow(self, exact_rcp: bool = True) -> float:
        return self.tracer.trace_batch(self.shadow_batch(), exact_rcp=exact_rcp) if self.num_slots else 0.0

    def accumulate(self, stream=None) -> None:
        """radiance += pending where the slot's shadow ray reached the light (mrt_path_accumulate),
        enqueued on `stream` with no host sync; nothing is allocated, so stream= alone is enough."""
        m, nxt = self.num_slots, 1 - self._cur
        _lib.check(self.lib.mrt_path_accumulate(m, self.num_paths, self.state[nxt].data_ptr(), self.pending.data_ptr(),
                                                self.shadow_results.data_ptr(), self.radiance.data_ptr(),
                                                _stream_ptr(stream)))

    def trace_bounce(self, exact_rcp: bool = True) -> float:
        """Trace the bounce rays extend wrote and make them the current rays."""
        ms = self.tracer.trace_batch(self.bounce_batch(), exact_rcp=exact_rcp) if self.num_slots else 0.0
        self._cur = 1 - self._cur
        return ms

    def run(self, exact_rcp: bool = True) -> float:
        """Every vertex of the batch; stops early when no path is live. Returns the sum of the
        traces' milliseconds."""
        ms = 0.0
        for b in range(self.depth + 1):
            if self.extend(b) == 0:
                break
            ms += self.trace_shadow(exact_rcp)
            self.accumulate()
            if b < self.depth:
                ms += self.trace_bounce(exact_rcp)
        return ms

    def resolve(self, slot_to_id: torch.Tensor, num_pixels: int, pixels: torch.Tensor | None = None,
                image: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """The batch's pixels (int32 ABGR bits) at slot_to_id[first + i]; image (float32
        [num_pixels, 4], optional) gets the unclamped values. Enqueued on `stream` with no host
        sync; pixels made here are zeroed on that stream, so passing stream= alone is enough."""
        if slot_to_id.numel() != self.primary.size:
            raise _lib.MrtError("slot_to_id must hold one pixel id per primary ray")
        if pixels is None:
            with _on_stream(stream):
                pixels = torch.zeros(num_pixels, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.mrt_path_resolve(self.num_samples, self.first, self.count, slot_to_id.data_ptr(),
                                             self.primary.results.data_ptr(), self.radiance.data_ptr(),
                                             pixels.data_ptr(), None if image is None else image.data_ptr(),
                                             _stream_ptr(stream)))
        return pixels
