"""Device-side mirror of the reference's tracing classes, over lib/libmrt.so.

  GpuBvh     <- CudaBVH      (src/rt/cuda/CudaBVH.cc:55-116): Compact2 buffers resident in HBM
  RayBuffer  <- RayBuffer    (src/rt/ray/RayBuffer.cc:53-81): Ray[n] in, RayResult[n] out, on device
  Tracer     <- CudaTracer   (src/rt/cuda/CudaTracer.cc:84-177): setBVH / traceBatch(RayBuffer&) -> ms

Device memory and streams come from PyTorch (plumbing); every launch goes
through the C-ABI of include/mrt.h. There is no CPU path: without a GPU the
Tracer constructor raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np
import torch

from . import _lib
from .host import Bvh, tree_cost_dict


def _stream_ptr(stream) -> int | None:
    if stream is None:
        stream = torch.cuda.current_stream()
    return stream.cuda_stream or None


def _on_stream(stream):
    """`stream` as torch's current stream for the length of a `with` block (nothing where stream is
    None: the current stream stays). Every method that takes stream= runs under it, so that what
    it allocates, fills, uploads and reads back is ordered on the stream its launches go to:
    passing stream= alone is enough, whatever torch's current stream is."""
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


class GpuBvh:
    """Compact2 node / Woop / triIndex buffers uploaded to the current device."""

    def __init__(self, bvh: Bvh | tuple, device=None):
        """bvh: a host Bvh, or (nodes, woop, triIndex) as int32 numpy arrays or tensors
        (device tensors, e.g. from mrt.dist.replicate_buffers, are bound in place)."""
        nodes, woop, tri = bvh.buffers() if isinstance(bvh, Bvh) else bvh
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())

        def upload(a):
            if isinstance(a, torch.Tensor):
                return a.to(dev, torch.int32).contiguous()
            return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
        self.nodes, self.woop, self.tri_index = upload(nodes), upload(woop), upload(tri)
        self.device = dev

    @property
    def node_bytes(self) -> int:
        return self.nodes.numel() * 4

    @property
    def woop_bytes(self) -> int:
        return self.woop.numel() * 4

    @property
    def tri_index_bytes(self) -> int:
        return self.tri_index.numel() * 4

    @property
    def total_bytes(self) -> int:
        return self.node_bytes + self.woop_bytes + self.tri_index_bytes


class RayBuffer:
    """Ray[n] (32 B) and RayResult[n] (16 B) arrays on the device.

    needClosestHit selects the trace mode exactly like the reference
    (anyHit = !needClosestHit, CudaTracer.cc:172)."""

    def __init__(self, rays, need_closest_hit: bool = True, device=None, results: torch.Tensor | None = None,
                 secondary: bool = False):
        """results: an existing int32 [n, 4] device tensor to write into (e.g. a
        slice of a larger RayResult array, for the shards of one RayBuffer).
        secondary: the rays are AO / diffuse / later-bounce rays (a tuning hint, MRT_TRACE_SECONDARY:
        the autotuner keeps their schedule apart from a primary batch of the same size)."""
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        if isinstance(rays, torch.Tensor):
            self.rays = rays.to(dev, torch.float32).contiguous().view(-1, 8)
        else:
            self.rays = torch.from_numpy(np.ascontiguousarray(rays, np.float32).reshape(-1, 8)).to(dev)
        if results is None:
            results = torch.zeros((self.rays.shape[0], 4), dtype=torch.int32, device=dev)
        elif tuple(results.shape) != (self.rays.shape[0], 4) or not results.is_contiguous() or \
                results.dtype != torch.int32:
            raise ValueError("results must be a contiguous int32 [n, 4] tensor matching the rays")
        self.results = results
        self.need_closest_hit = need_closest_hit
        self.secondary = bool(secondary)
        self.stats = None

    def view(self, lo: int, hi: int) -> "RayBuffer":
        """Rays [lo, hi) of this buffer as a RayBuffer sharing its rays and results."""
        return RayBuffer(self.rays[lo:hi], self.need_closest_hit, self.rays.device, self.results[lo:hi],
                         secondary=self.secondary)

    def morton_sort(self, slot_to_id: torch.Tensor | None = None, drop_levels: int = 0, box: int = 0, stream=None,
                    want_keys: bool = False):
        """RayBuffer::mortonSort (RayBuffer.cc:256-324) on the device, stream-ordered with no host
        sync (mrt_ray_sort): a new RayBuffer of this one's rays in the order of the reference's
        Morton key >> (6 * drop_levels), ties by slot; box 0 takes the key's box over origins and
        end points (the reference), 1 over origins only. slot_to_id: this buffer's int32 ids
        (None = the identity). Returns (sorted RayBuffer, id_to_slot, slot_to_id) — id_to_slot
        starts at -1 and is what reconstruct takes as batch_id_to_slot — and, with want_keys,
        also keys (uint32 bits as int32 [n, 6], in this buffer's order) and box (float32 [6]).
        The new buffer keeps need_closest_hit and secondary and has fresh results. Passing stream=
        alone is enough: the tensors returned are allocated, and id_to_slot and the new results
        filled, on that stream."""
        dev = self.rays.device
        n = self.size
        if dev.type != "cuda":
            raise _lib.MrtError("morton_sort needs rays on a HIP device (mrt.host.ray_sort sorts host rays)")
        if slot_to_id is not None and (slot_to_id.dtype != torch.int32 or tuple(slot_to_id.shape) != (n,) or
                                       slot_to_id.device != dev or not slot_to_id.is_contiguous()):
            raise _lib.MrtError("morton_sort: slot_to_id must be a contiguous int32 [n] tensor on the rays' device")
        with _on_stream(stream):
            out = torch.empty_like(self.rays)
            id_to_slot = torch.full((n,), -1, dtype=torch.int32, device=dev)
            new_slot_to_id = torch.empty(n, dtype=torch.int32, device=dev)
            keys = torch.empty((n, 6), dtype=torch.int32, device=dev) if want_keys else None
            box_out = torch.empty(6, dtype=torch.float32, device=dev) if want_keys else None
            params = _lib.RaySortParams(drop_levels=int(drop_levels), box=int(box))
            _lib.check(_lib.trace_lib().mrt_ray_sort(
                self.rays.data_ptr(), None if slot_to_id is None else slot_to_id.data_ptr(), n, C.byref(params),
                out.data_ptr(), id_to_slot.data_ptr(), new_slot_to_id.data_ptr(),
                None if keys is None else keys.data_ptr(), None if box_out is None else box_out.data_ptr(),
                _stream_ptr(stream)))
            rb = RayBuffer(out, self.need_closest_hit, dev, secondary=self.secondary)
        if want_keys:
            return rb, id_to_slot, new_slot_to_id, keys, box_out
        return rb, id_to_slot, new_slot_to_id

    @property
    def size(self) -> int:
        return int(self.rays.shape[0])

    def results_numpy(self) -> np.ndarray:
        return self.results.cpu().numpy()

    def hit_ids(self) -> np.ndarray:
        return self.results_numpy()[:, 0]

    def hit_t(self) -> np.ndarray:
        return self.results_numpy()[:, 1].view(np.float32)


def tree_cost_from_tensor(t: torch.Tensor) -> dict:
    """The dict Tracer.tree_cost(sync=True) gives, from the device tensor its sync=False form
    returned (blocking copy; synchronise the stream it was enqueued on first)."""
    raw = t.cpu().numpy().tobytes()
    return tree_cost_dict(_lib.TreeCost.from_buffer_copy(raw))


def refit_plan(nodes, wide: bool = True):
    """Host-only (mrt_refit_plan): (order int32[n], level offsets int64[levels + 1], wide
    source map int32[4 * wide nodes] or None) of a Compact2 node array."""
    lib = _lib.trace_lib()
    n = np.ascontiguousarray(nodes).view(np.int32)
    order = np.empty(n.size // 16, np.int32)
    levels = C.c_int32()
    _lib.check(lib.mrt_refit_plan(n.ctypes.data, n.nbytes, None, None, 0, C.byref(levels), None, 0, None))
    offsets = np.empty(levels.value + 1, np.int64)
    nsrc = C.c_int64()
    _lib.check(lib.mrt_refit_plan(n.ctypes.data, n.nbytes, order.ctypes.data, offsets.ctypes.data, len(offsets),
                                  C.byref(levels), None, 0, C.byref(nsrc) if wide else None))
    src = None
    if wide:
        src = np.empty(nsrc.value, np.int32)
        _lib.check(lib.mrt_refit_plan(n.ctypes.data, n.nbytes, None, None, 0, C.byref(levels), src.ctypes.data,
                                      src.size, C.byref(nsrc)))
    return order, offsets, src


class Tracer:
    """Persistent-wave BVH tracer for one HIP device (mirror of CudaTracer)."""

    def __init__(self, device: int | None = None):
        if not torch.cuda.is_available():
            raise RuntimeError("mrt.Tracer needs a HIP device; there is no CPU fallback")
        self.lib = _lib.trace_lib()
        self.device = torch.cuda.current_device() if device is None else int(device)
        h = C.c_void_p()
        _lib.check(self.lib.mrt_tracer_create(self.device, C.byref(h)))
        self._h = h
        self.bvh: GpuBvh | None = None

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self.lib.mrt_tracer_destroy(self._h)
            self._h = C.c_void_p()

    # -- configuration -------------------------------------------------------
    def config(self) -> dict:
        c = _lib.LaunchCfg()
        _lib.check(self.lib.mrt_tracer_get_config(self._h, C.byref(c)))
        return {k: getattr(c, k) for k, _ in c._fields_}

    def set_config(self, **kw) -> None:
        cur = self.config()
        cur.update(kw)
        c = _lib.LaunchCfg(**cur)
        _lib.check(self.lib.mrt_tracer_set_config(self._h, C.byref(c)))

    def bind_info(self) -> dict:
        """What the last bind derived: wall ms, wide-node bytes/format, stack capacity."""
        b = _lib.BindInfo()
        _lib.check(self.lib.mrt_tracer_bind_info(self._h, C.byref(b)))
        return {k: getattr(b, k) for k, _ in b._fields_}

    @property
    def last_kernel_key(self) -> int:
        """The key (include/mrt.h) of the kernel the most recent trace launched; -1 before any."""
        return int(self.lib.mrt_tracer_last_kernel_key(self._h))

    def schedules(self) -> list:
        """The autotuner's settled schedules [(num_rays, variant, candidate, version)]."""
        n = C.c_int32()
        _lib.check(self.lib.mrt_tracer_tune_export(self._h, None, 0, C.byref(n)))
        arr = (_lib.TunedSchedule * max(1, n.value))()
        _lib.check(self.lib.mrt_tracer_tune_export(self._h, arr, n.value, C.byref(n)))
        return [(e.num_rays, e.variant, e.candidate, e.version) for e in arr[:n.value]]

    def load_schedules(self, entries) -> None:
        """Lock schedules saved by schedules() from an earlier run on the same BVH
        (call after set_bvh: binding forgets them)."""
        entries = list(entries)
        arr = (_lib.TunedSchedule * max(1, len(entries)))(*[_lib.TunedSchedule(*e) for e in entries])
        _lib.check(self.lib.mrt_tracer_tune_import(self._h, arr, len(entries)))

    # -- CudaTracer API --------------------------------------------------------
    def set_bvh(self, bvh: GpuBvh, on_device: bool = False, stream=None) -> None:
        """setBVH + bind_CudaBVHTexture (CudaTracer.cc:142-146); re-binding is allowed.
        on_device: derive the 4-wide array and the refit plan on the device, on `stream`
        (mrt_tracer_bind_device: the same array; a tree that is none raises and leaves the
        tracer unbound)."""
        args = (self._h, bvh.nodes.data_ptr(), bvh.node_bytes, bvh.woop.data_ptr(), bvh.woop_bytes,
                bvh.tri_index.data_ptr(), bvh.tri_index_bytes)
        if on_device:
            self.bvh = None
            _lib.check(self.lib.mrt_tracer_bind_device(*args, _stream_ptr(stream)))
        else:
            _lib.check(self.lib.mrt_tracer_bind(*args))
        self.bvh = bvh

    def derive_info(self) -> dict:
        """The last device bind, device build or device-made refit plan: which parts were derived
        on the device, levels, wide nodes, launches, readbacks, phase and wall ms, scratch bytes
        (mrt_tracer_derive_info)."""
        d = _lib.DeriveInfo()
        _lib.check(self.lib.mrt_tracer_derive_info(self._h, C.byref(d)))
        return {k: getattr(d, k) for k, _ in d._fields_}

    def refit_plan(self):
        """Blocking copy of the installed refit plan in mrt.tracer.refit_plan's shapes: (order,
        level offsets, wide source map or None); None when no plan is installed."""
        if self.bvh is None:
            return None
        levels, nsrc = C.c_int32(), C.c_int64()
        _lib.check(self.lib.mrt_tracer_copy_refit_plan(self._h, None, None, 0, C.byref(levels), None, 0, C.byref(nsrc)))
        if levels.value == 0:
            return None
        order = np.empty(self.bvh.node_bytes // 64, np.int32)
        offsets = np.empty(levels.value + 1, np.int64)
        src = np.empty(nsrc.value, np.int32)
        _lib.check(self.lib.mrt_tracer_copy_refit_plan(self._h, order.ctypes.data, offsets.ctypes.data, len(offsets),
                                                       C.byref(levels), src.ctypes.data if src.size else None,
                                                       src.size, C.byref(nsrc)))
        return order, offsets, (src if src.size else None)

    # -- refit (moving geometry, fixed topology) ---------------------------------
    def refit(self, vertices, triangles, stream=None) -> None:
        """Refit the bound BVH in place for moved vertices (mrt_tracer_refit): stream-ordered,
        no host sync after the first call. vertices float32 [nv, 3], triangles int32 [nt, 3]
        (the triangles the BVH was built over) as device tensors; numpy arrays are uploaded.
        Writes the bound GpuBvh's nodes and woop tensors. Passing stream= alone is enough: an upload
        or a conversion of the arguments is ordered on that stream too."""
        if self.bvh is None:
            raise _lib.MrtError("Tracer: No BVH!")
        dev = self.bvh.device

        def on_device(a, dtype, np_dtype):
            if isinstance(a, torch.Tensor):
                return a.to(dev, dtype).contiguous().view(-1, 3)
            a = np.ascontiguousarray(a, np_dtype).reshape(-1, 3)
            return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
        with _on_stream(stream):
            v = on_device(vertices, torch.float32, np.float32)
            t = on_device(triangles, torch.int32, np.int32)
            _lib.check(self.lib.mrt_tracer_refit(self._h, v.data_ptr(), v.shape[0], t.data_ptr(), t.shape[0],
                                                 _stream_ptr(stream)))
        self._refit_inputs = (v, t)   # the launches may still read them

    def refit_info(self) -> dict:
        """Blocking: levels, launches of the last refit, plan bytes, and the out-of-range
        references skipped since the last call (mrt_tracer_refit_info)."""
        r = _lib.RefitInfo()
        _lib.check(self.lib.mrt_tracer_refit_info(self._h, C.byref(r)))
        return {k: getattr(r, k) for k, _ in r._fields_}

    def tree_cost(self, stream=None, sync: bool = True):
        """The bound tree's area sums, summed on the device (mrt_tracer_tree_cost): root_area,
        inner_area, leaf_area, leaf_tri_area, records, leaves, triangles, skipped, and
        sah = (Cn * inner_area + Ct * leaf_tri_area) / root_area (mrt.host.tree_cost_dict). Ordered
        after a refit on `stream`. sync=True blocks for one 64-byte readback and returns the dict;
        sync=False enqueues only and returns an 8-word float64 device tensor holding the
        mrt_tree_cost bytes (mrt.tracer.tree_cost_from_tensor reads it after a sync), allocated on
        `stream`: passing stream= alone is enough in both forms."""
        if self.bvh is None:
            raise _lib.MrtError("Tracer: No BVH!")
        if sync:
            c = _lib.TreeCost()
            _lib.check(self.lib.mrt_tracer_tree_cost(self._h, C.byref(c), None, _stream_ptr(stream)))
            return tree_cost_dict(c)
        with _on_stream(stream):
            out = torch.empty(8, dtype=torch.float64, device=self.bvh.device)
            _lib.check(self.lib.mrt_tracer_tree_cost(self._h, None, out.data_ptr(), _stream_ptr(stream)))
        return out

    # -- re-optimise (treelet restructuring) ---------------------------------------
    def optimize(self, rounds: int = 1, stream=None) -> dict:
        """Re-optimise the bound BVH's topology in place on the device by treelet restructuring
        (mrt_tracer_optimize): blocking. rounds passes (1..8); after the last one the refit plan
        and the 4-wide array are derived again on the device and installed, the settled schedules
        stay. Writes the bound GpuBvh's nodes tensor, the bytes Bvh.optimize writes. Returns
        mrt_tracer_optimize_info: rounds, levels, launches, per round the treelets considered
        and rewritten, device and wall ms, scratch bytes."""
        if self.bvh is None:
            raise _lib.MrtError("Tracer: No BVH!")
        params = _lib.OptimizeParams(rounds=int(rounds))
        _lib.check(self.lib.mrt_tracer_optimize(self._h, C.byref(params), _stream_ptr(stream)))
        o = _lib.OptimizeInfo()
        _lib.check(self.lib.mrt_tracer_optimize_info(self._h, C.byref(o)))
        out = {k: getattr(o, k) for k, _ in o._fields_}
        out["considered"] = list(o.considered[:o.rounds])
        out["rewritten"] = list(o.rewritten[:o.rounds])
        return out

    # -- device build (new geometry, no host BVH) ---------------------------------
    def build(self, vertices, triangles, max_leaf_size=None, stream=None, on_device: bool = False) -> GpuBvh:
        """Build a linear BVH of the triangles on the device and bind it (mrt_tracer_build):
        blocking. vertices float32 [nv, 3], triangles int32 [nt, 3] as device tensors; numpy
        arrays are uploaded. Returns the bound GpuBvh, its tensors trimmed to the bytes written
        (views of buffers sized by mrt_lbvh_sizes). max_leaf_size 1..8 (None = the default).
        Faster than mrt.Bvh.build + upload by orders of magnitude, slower to trace (no SAH, no
        spatial splits): for new or re-meshed geometry; Tracer.refit covers moved vertices.
        on_device: the level plan and the bind's 4-wide array are derived on the device too
        (mrt_tracer_build_device: the same bytes, no node array crosses to the host).
        Passing stream= alone is enough: the uploads and the tree's tensors are ordered on it."""
        dev = torch.device("cuda", self.device)

        def to_device(a, dtype, np_dtype):
            if isinstance(a, torch.Tensor):
                return a.to(dev, dtype).contiguous().view(-1, 3)
            a = np.ascontiguousarray(a, np_dtype).reshape(-1, 3)
            return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
        with _on_stream(stream):
            v = to_device(vertices, torch.float32, np.float32)
            t = to_device(triangles, torch.int32, np.int32)
            cap = [C.c_int64(), C.c_int64(), C.c_int64()]
            _lib.check(self.lib.mrt_lbvh_sizes(t.shape[0], *map(C.byref, cap)))
            nodes, woop, tri = (torch.empty(c.value // 4, dtype=torch.int32, device=dev) for c in cap)
            params = _lib.LbvhParams(max_leaf_size=int(max_leaf_size or 0))
            out = [C.c_int64(), C.c_int64(), C.c_int64()]
            fn = self.lib.mrt_tracer_build_device if on_device else self.lib.mrt_tracer_build
            _lib.check(fn(self._h, v.data_ptr(), v.shape[0], t.data_ptr(), t.shape[0],
                          C.byref(params), nodes.data_ptr(), cap[0].value, woop.data_ptr(),
                          cap[1].value, tri.data_ptr(), cap[2].value, *map(C.byref, out),
                          _stream_ptr(stream)))
        bvh = GpuBvh.__new__(GpuBvh)
        bvh.nodes, bvh.woop, bvh.tri_index = (a[:o.value // 4] for a, o in zip((nodes, woop, tri), out))
        bvh.device = dev
        self.bvh = bvh
        return bvh

    def build_info(self) -> dict:
        """The last build: wall / plan / bind ms on the host, sort / emit / fit ms on the device,
        records, leaves, slots, levels, scratch bytes, skipped references (mrt_tracer_build_info)."""
        b = _lib.BuildInfo()
        _lib.check(self.lib.mrt_tracer_build_info(self._h, C.byref(b)))
        return {k: getattr(b, k) for k, _ in b._fields_}

    def wide_nodes(self) -> np.ndarray:
        """Blocking copy of the derived 4-wide node array as uint32 (empty with wide = 0)."""
        n = C.c_int64()
        _lib.check(self.lib.mrt_tracer_copy_wide_nodes(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value // 4, np.uint32)
        if n.value:
            _lib.check(self.lib.mrt_tracer_copy_wide_nodes(self._h, out.ctypes.data, out.nbytes, C.byref(n)))
        return out

    def flags(self, rays: RayBuffer, exact_rcp=False, speculative=True, stats=False) -> int:
        f = 0 if rays.need_closest_hit else _lib.MRT_TRACE_ANY_HIT
        if exact_rcp:
            f |= _lib.MRT_TRACE_EXACT_RCP
        if not speculative:
            f |= _lib.MRT_TRACE_LOCKSTEP_OFF
        if stats:
            f |= _lib.MRT_TRACE_STATS
        if getattr(rays, "secondary", False):
            f |= _lib.MRT_TRACE_SECONDARY
        return f

    def trace_async(self, rays: RayBuffer, exact_rcp=False, speculative=True, stats=False, stream=None) -> None:
        """Stream-ordered trace of the whole batch (no host sync). Passing stream= alone is enough:
        a stats tensor it makes is zeroed on that stream."""
        if self.bvh is None:
            raise _lib.MrtError("Tracer: No BVH!")   # CudaTracer.cc:129-130
        f = self.flags(rays, exact_rcp, speculative, stats)
        sp = None
        if stats:
            if rays.stats is None or rays.stats.shape[0] != rays.size:
                with _on_stream(stream):
                    rays.stats = torch.zeros((rays.size, 4), dtype=torch.int32, device=rays.rays.device)
            sp = rays.stats.data_ptr()
        _lib.check(self.lib.mrt_tracer_trace(self._h, rays.rays.data_ptr(), rays.results.data_ptr(), rays.size, f,
                                             sp, _stream_ptr(stream)))

    def launcher(self, rays: RayBuffer, exact_rcp=False, speculative=True, stream=None):
        """A zero-argument callable that re-issues trace_async(rays, ...) with every
        argument resolved once: one C call per launch, for tight launch loops."""
        if self.bvh is None:
            raise _lib.MrtError("Tracer: No BVH!")
        fn, h = self.lib.mrt_tracer_trace, self._h
        args = (rays.rays.data_ptr(), rays.results.data_ptr(), rays.size, self.flags(rays, exact_rcp, speculative),
                None, _stream_ptr(stream))
        check = _lib.check

        def launch():
            rc = fn(h, *args)
            if rc:
                check(rc)
        launch.stream = stream if stream is not None else torch.cuda.current_stream()
        return launch

    def trace_batch(self, rays: RayBuffer, exact_rcp=False, speculative=True, stats=False, stream=None) -> float:
        """CudaTracer::traceBatch: blocking, returns the launch's milliseconds (0 for no rays). The
        launch runs on `stream`, and so does the zeroing of a stats tensor it makes."""
        if self.bvh is None:
            raise _lib.MrtError("Tracer: No BVH!")
        f = self.flags(rays, exact_rcp, speculative, stats)
        sp = None
        if stats:
            if rays.stats is None or rays.stats.shape[0] != rays.size:
                with _on_stream(stream):
                    rays.stats = torch.zeros((rays.size, 4), dtype=torch.int32, device=rays.rays.device)
            sp = rays.stats.data_ptr()
        info = _lib.TraceInfo()
        _lib.check(self.lib.mrt_tracer_trace_timed(self._h, rays.rays.data_ptr(), rays.results.data_ptr(), rays.size,
                                                   f, sp, _stream_ptr(stream), C.byref(info)))
        self.last_info = {k: getattr(info, k) for k, _ in info._fields_}
        return float(info.kernel_ms)
