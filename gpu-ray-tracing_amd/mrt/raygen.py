"""Device ray generation and hit counting (mirror of the reference's RayGen,
src/rt/ray/RayGen.cc:50-120, and countHitsKernel, RendererKernels.cu:112-162),
over the mrt_raygen_* / mrt_count_hits entry points of include/mrt.h.

The per-ray arithmetic is the host generator's (mrt.host.primary_rays /
ao_rays): primary rays come out bit-identical, AO/diffuse directions within a
few ulp (device cosf/sinf). Pixel tables and the camera matrix are computed on
the host, as in the reference (PixelTable.cc, Renderer.cc:126-129).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .host import AO_SEED, Camera, Scene, _light3, pixel_table
from .tracer import RayBuffer, _on_stream, _stream_ptr


def nscreen_to_world(cam: Camera, w: int, h: int) -> np.ndarray:
    out = (C.c_float * 16)()
    c = cam.to_c()
    _lib.check_host(_lib.host_lib().mrth_camera_nscreen_to_world(C.byref(c), w, h, out))
    return np.array(out, np.float32)


def _geometry_on_device(dev, vertices, triangles, diffuse):
    """vertices float32 [nv, 3], triangles int32 [nt, 3], diffuse float32 [nt, 4] or None as
    contiguous tensors on dev; numpy input is uploaded (as in Tracer.refit)."""
    def on_device(a, dtype, np_dtype, cols):
        if isinstance(a, torch.Tensor):
            return a.to(dev, dtype).contiguous().view(-1, cols)
        a = np.ascontiguousarray(a, np_dtype).reshape(-1, cols)
        return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)
    v = on_device(vertices, torch.float32, np.float32, 3)
    t = on_device(triangles, torch.int32, np.int32, 3)
    d = None if diffuse is None else on_device(diffuse, torch.float32, np.float32, 4)
    if d is not None and d.shape[0] != t.shape[0]:
        raise _lib.MrtError("set_geometry: diffuse must hold 4 floats per triangle")
    return v, t, d


def scene_attributes(vertices: torch.Tensor, triangles: torch.Tensor, diffuse: torch.Tensor | None = None,
                     normals: torch.Tensor | None = None, shaded: torch.Tensor | None = None,
                     material: torch.Tensor | None = None, skipped: torch.Tensor | None = None, stream=None) -> None:
    """mrt_scene_attributes over device tensors, written into the outputs given (float32 [nt, 3],
    int32 [nt], int32 [nt]; at least one) on `stream`, with no host sync. skipped: an int64
    device tensor the count of triangles with an out-of-range vertex index is ADDED to."""
    def ptr(a):
        return None if a is None else a.data_ptr()
    _lib.check(_lib.trace_lib().mrt_scene_attributes(ptr(vertices), vertices.shape[0], ptr(triangles),
                                                     triangles.shape[0], ptr(diffuse), ptr(normals), ptr(shaded),
                                                     ptr(material), ptr(skipped), _stream_ptr(stream)))


class DeviceRayGen:
    """RayGen on one device: primary rays, AO/diffuse rays, hit counts."""

    def __init__(self, scene: Scene | None = None, device=None):
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.trace_lib()
        self._tables = {}
        self.normals = None
        self.num_tris = 0
        if scene is not None:
            _, _, normals = scene.arrays()
            self.normals = torch.from_numpy(np.ascontiguousarray(normals, np.float32)).to(self.device)
            self.num_tris = scene.num_triangles

    def set_geometry(self, vertices, triangles, diffuse=None, stream=None) -> None:
        """The triangle normals of moved (or new) vertices, computed on the device
        (mrt_scene_attributes) on `stream` with no host sync: what ao / ao_blocks shoot their
        hemispheres round from then on. vertices float32 [nv, 3], triangles int32 [nt, 3] as
        device tensors; numpy arrays are uploaded. The normal tensor is rewritten in place; a
        first call, or another triangle count, allocates it. diffuse is not needed here (the
        signature is DeviceReconstructor.set_geometry's). Passing stream= alone is enough: uploads
        and a new normal tensor are ordered on that stream."""
        with _on_stream(stream):
            v, t, _ = _geometry_on_device(self.device, vertices, triangles, None)
            nt = t.shape[0]
            if self.normals is None or self.normals.shape[0] != nt:
                self.normals = torch.empty((nt, 3), dtype=torch.float32, device=self.device)
                self.num_tris = nt
            scene_attributes(v, t, normals=self.normals, stream=stream)
        self._geometry_inputs = (v, t)   # the launch may still read them

    def _table(self, w: int, h: int) -> torch.Tensor:
        if (w, h) not in self._tables:
            self._tables[(w, h)] = torch.from_numpy(pixel_table(w, h)).to(self.device)
        return self._tables[(w, h)]

    def primary(self, cam: Camera, w: int, h: int, stream=None, subpixel=(0.5, 0.5)) -> tuple[RayBuffer, torch.Tensor]:
        """RayGen::primary: w*h closest-hit rays in Morton pixel order + slot->pixel ids.
        subpixel: sample position inside each pixel (the reference's is the centre).
        Passing stream= alone is enough: the pixel table's first upload, the tensors returned and
        the zeroing of the new buffer's results are ordered on that stream."""
        m = nscreen_to_world(cam, w, h)
        origin = np.array(cam.position, np.float32)
        with _on_stream(stream):
            rays = torch.empty((w * h, 8), dtype=torch.float32, device=self.device)
            slot_to_id = torch.empty(w * h, dtype=torch.int32, device=self.device)
            _lib.check(self.lib.mrt_raygen_primary_subpixel(m.ctypes.data_as(C.POINTER(C.c_float)),
                                                            origin.ctypes.data_as(C.POINTER(C.c_float)), float(cam.far), w,
                                                            h, float(subpixel[0]), float(subpixel[1]),
                                                            self._table(w, h).data_ptr(), rays.data_ptr(),
                                                            slot_to_id.data_ptr(), None, _stream_ptr(stream)))
            return RayBuffer(rays, need_closest_hit=True, device=self.device), slot_to_id

    def ao(self, rays: RayBuffer, num_samples: int, max_dist: float, seed: int = AO_SEED, closest_hit: bool = False,
           stream=None, first: int = 0, count: int | None = None) -> RayBuffer:
        """RayGen::ao over a traced batch: num_samples hemisphere rays per input ray
        (any-hit for AO; closest_hit=True with max_dist=far is the diffuse bounce).
        first/count select the input rays [first, first + count) — one batch of
        RayGen::batching (RayGen.cc:77-120: firstInputSlot, numInputRays); the
        rotation hash and the output slots count from the batch's first ray. Passing stream= alone
        is enough: the new buffer is allocated, and its results zeroed, on that stream."""
        if self.normals is None:
            raise _lib.MrtError("DeviceRayGen.ao needs the scene's triangle normals (pass scene=)")
        n = rays.size - first if count is None else count
        if first < 0 or n < 0 or first + n > rays.size:
            raise _lib.MrtError(f"input range [{first}, {first + n}) outside the {rays.size}-ray batch")
        with _on_stream(stream):
            out = torch.empty((n * num_samples, 8), dtype=torch.float32, device=self.device)
            _lib.check(self.lib.mrt_raygen_ao(rays.rays.data_ptr() + 32 * first, rays.results.data_ptr() + 16 * first, n,
                                              self.normals.data_ptr(), self.num_tris, num_samples, float(max_dist),
                                              seed & 0xFFFFFFFF, out.data_ptr(), None, None, _stream_ptr(stream)))
            return RayBuffer(out, need_closest_hit=closest_hit, device=self.device, secondary=True)

    def ao_blocks(self, rays: RayBuffer, num_samples: int, max_dist: float, seeds, batch_inputs: int,
                  blocks: torch.Tensor, block_rays: int, num_rays: int, closest_hit: bool = False,
                  stream=None) -> RayBuffer:
        """The frame's AO/diffuse rays for a list of blocks of its ray order (mrt_raygen_ao_blocks):
        the rays RayGen::batching's batches (batch_inputs input rays each, seeded by seeds[k])
        hold at positions blocks[i] * block_rays + [0, block_rays), concatenated in list order —
        e.g. one rank's shard of the frame in its trace order, generated directly. blocks: int32
        device tensor; num_rays: the rays listed (a partial last block of the frame, when listed,
        must be the last entry: mrt.dist.shard_blocks_device keeps it there). Any number of
        batches: above 256 the seeds are read from stream-ordered device scratch. Passing stream=
        alone is enough: the new buffer is allocated, and its results zeroed, on that stream."""
        if self.normals is None:
            raise _lib.MrtError("DeviceRayGen.ao_blocks needs the scene's triangle normals (pass scene=)")
        if blocks.dtype != torch.int32 or blocks.dim() != 1 or blocks.device != torch.device(self.device):
            raise _lib.MrtError("ao_blocks: blocks must be a 1-D int32 tensor on the generator's device")
        sd = (C.c_uint32 * max(1, len(seeds)))(*[s & 0xFFFFFFFF for s in seeds])
        with _on_stream(stream):
            out = torch.empty((num_rays, 8), dtype=torch.float32, device=self.device)
            _lib.check(self.lib.mrt_raygen_ao_blocks(rays.rays.data_ptr(), rays.results.data_ptr(), rays.size,
                                                     self.normals.data_ptr(), self.num_tris, num_samples, float(max_dist),
                                                     C.cast(sd, C.c_void_p), len(seeds), batch_inputs, blocks.data_ptr(),
                                                     blocks.numel(), block_rays, num_rays, out.data_ptr(),
                                                     _stream_ptr(stream)))
            return RayBuffer(out, need_closest_hit=closest_hit, device=self.device, secondary=True)

    def shadow(self, rays: RayBuffer, num_samples: int, light, light_radius: float, seed: int = AO_SEED,
               stream=None, first: int = 0, count: int | None = None) -> RayBuffer:
        """RayGen::shadow over a traced batch (mrt_raygen_shadow): num_samples any-hit rays per
        input ray from the traced point towards samples of an area light at `light` (a cube of
        half-side light_radius), each with tmax = the distance to its sample (-1 where the input
        ray missed). first/count select the input rays [first, first + count), one batch of
        RayGen::batching; the offset hash and the output slots count from the batch's first ray.
        Bit-identical to mrt.host.shadow_rays. Passing stream= alone is enough: the new buffer is
        allocated, and its results zeroed, on that stream."""
        n = rays.size - first if count is None else count
        if first < 0 or n < 0 or first + n > rays.size:
            raise _lib.MrtError(f"input range [{first}, {first + n}) outside the {rays.size}-ray batch")
        with _on_stream(stream):
            out = torch.empty((n * num_samples, 8), dtype=torch.float32, device=self.device)
            _lib.check(self.lib.mrt_raygen_shadow(rays.rays.data_ptr() + 32 * first, rays.results.data_ptr() + 16 * first,
                                                  n, num_samples, _light3(light), float(light_radius), seed & 0xFFFFFFFF,
                                                  out.data_ptr(), None, None, _stream_ptr(stream)))
            return RayBuffer(out, need_closest_hit=False, device=self.device, secondary=True)

    def shadow_blocks(self, rays: RayBuffer, num_samples: int, light, light_radius: float, seeds, batch_inputs: int,
                      blocks: torch.Tensor, block_rays: int, num_rays: int, stream=None) -> RayBuffer:
        """The frame's shadow rays for a list of blocks of its ray order (mrt_raygen_shadow_blocks):
        ao_blocks' contract with shadow's rays, bit-identical to the batches' at those positions.
        Passing stream= alone is enough, as in ao_blocks."""
        if blocks.dtype != torch.int32 or blocks.dim() != 1 or blocks.device != torch.device(self.device):
            raise _lib.MrtError("shadow_blocks: blocks must be a 1-D int32 tensor on the generator's device")
        sd = (C.c_uint32 * max(1, len(seeds)))(*[s & 0xFFFFFFFF for s in seeds])
        with _on_stream(stream):
            out = torch.empty((num_rays, 8), dtype=torch.float32, device=self.device)
            _lib.check(self.lib.mrt_raygen_shadow_blocks(rays.rays.data_ptr(), rays.results.data_ptr(), rays.size,
                                                         num_samples, _light3(light), float(light_radius),
                                                         C.cast(sd, C.c_void_p), len(seeds), batch_inputs,
                                                         blocks.data_ptr(), blocks.numel(), block_rays, num_rays,
                                                         out.data_ptr(), _stream_ptr(stream)))
            return RayBuffer(out, need_closest_hit=False, device=self.device, secondary=True)

    def shard_blocks(self, primary: RayBuffer, num_samples: int, block_rays: int, world: int, rank: int,
                     order: int = 1, stream=None) -> tuple[torch.Tensor, int]:
        """mrt_shard_blocks: rank's blocks (block i to rank i % world) of the frame's AO/diffuse
        ray order, in frame order (order 0) or live blocks first (1: decreasing live rays from
        the primary pass's results, ties in frame order, a partial last block last), as an int32
        device tensor, and the rays they hold. Any number of blocks per rank (the frame holds at
        most 2^31 - 1 rays): up to 16 384 are ordered by two small launches; a longer list in
        16 384-entry tiles, four launches and 5 bytes per block + 16 KB per tile of scratch taken and
        returned on the stream. No host sync either way. Passing stream= alone is enough: the list
        is allocated on that stream."""
        n = C.c_int32(0)
        m = C.c_int64(0)
        _lib.check(self.lib.mrt_shard_blocks(None, primary.size, num_samples, block_rays, world, rank, 0, None, 0,
                                             C.byref(n), C.byref(m), None))
        with _on_stream(stream):
            blocks = torch.empty(max(1, n.value), dtype=torch.int32, device=self.device)
            _lib.check(self.lib.mrt_shard_blocks(primary.results.data_ptr(), primary.size, num_samples, block_rays, world,
                                                 rank, order, blocks.data_ptr(), blocks.numel(), C.byref(n), C.byref(m),
                                                 _stream_ptr(stream)))
        return blocks[:n.value], m.value

    def count_hits_async(self, rays: RayBuffer, stream=None) -> torch.Tensor:
        """Device int32 scalar: results with id >= 0 (no host sync), allocated on `stream`: passing
        stream= alone is enough. Read it on that stream, or after synchronising it."""
        with _on_stream(stream):
            out = torch.empty(1, dtype=torch.int32, device=self.device)
            _lib.check(self.lib.mrt_count_hits(rays.results.data_ptr(), rays.size, out.data_ptr(), _stream_ptr(stream)))
        return out

    def count_hits(self, rays: RayBuffer, stream=None) -> int:
        """count_hits_async, then one blocking 4-byte readback ON `stream`, so the count is that of
        the results as the work enqueued on `stream` before this call left them: passing stream=
        alone is enough, whatever torch's current stream is."""
        with _on_stream(stream):
            return int(self.count_hits_async(rays, stream).item())


RAY_PRIMARY, RAY_AO, RAY_DIFFUSE, RAY_SHADOW, RAY_PATH = 0, 1, 2, 3, 4


class DeviceReconstructor:
    """Renderer's reconstruction step on one device (reference Renderer.cc:421-445 +
    reconstructKernel, RendererKernels.cu:60-108): traced batches -> ABGR pixels in HBM."""

    def __init__(self, scene: Scene | None, device=None):
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.trace_lib()
        self.material = self.shaded = None   # scene None: set_geometry makes them
        if scene is not None:
            mat, sh = scene.tri_colors()
            self.material = torch.from_numpy(mat.view(np.int32)).to(self.device)
            self.shaded = torch.from_numpy(sh.view(np.int32)).to(self.device)

    def set_geometry(self, vertices, triangles, diffuse=None, stream=None) -> None:
        """The shaded and material colours of moved (or new) vertices, computed on the device
        (mrt_scene_attributes) on `stream` with no host sync. vertices float32 [nv, 3], triangles
        int32 [nt, 3], diffuse float32 [nt, 4] (Scene.tri_diffuse(); None = the default material)
        as device tensors; numpy arrays are uploaded. The colour tensors are rewritten in place;
        a first call, or another triangle count, allocates them. Passing stream= alone is enough:
        uploads and new colour tensors are ordered on that stream."""
        with _on_stream(stream):
            v, t, d = _geometry_on_device(self.device, vertices, triangles, diffuse)
            nt = t.shape[0]
            if self.shaded is None or self.shaded.shape[0] != nt:
                self.material = torch.empty(nt, dtype=torch.int32, device=self.device)
                self.shaded = torch.empty(nt, dtype=torch.int32, device=self.device)
            scene_attributes(v, t, d, shaded=self.shaded, material=self.material, stream=stream)
        self._geometry_inputs = (v, t, d)   # the launch may still read them

    def reconstruct(self, ray_type: int, primary: RayBuffer, slot_to_id: torch.Tensor, num_pixels: int,
                    batch: RayBuffer | None = None, num_samples: int = 1, pixels: torch.Tensor | None = None,
                    batch_id_to_slot: torch.Tensor | None = None, stream=None, first_primary: int = 0) -> torch.Tensor:
        """num_pixels int32 (ABGR bits) pixels; batch defaults to the primary batch.
        AO/diffuse batches hold num_samples rays per primary ray (mrt_raygen_ao's layout);
        a batch of RayGen::batching covers the primaries [first_primary, first_primary +
        batch.size / num_samples) (Renderer::updateResult, Renderer.cc:421-445). Passing stream=
        alone is enough: pixels made here are zeroed on that stream."""
        if batch is None:
            batch = primary
        if ray_type == RAY_PRIMARY and (num_samples != 1 or batch.size != primary.size or first_primary):
            raise _lib.MrtError("primary reconstruction takes the primary batch with one ray per pixel")
        if batch.size % num_samples:
            raise _lib.MrtError(f"batch holds {batch.size} rays, not a multiple of {num_samples}")
        n_primary = batch.size // num_samples
        if first_primary < 0 or first_primary + n_primary > primary.size:
            raise _lib.MrtError(f"batch covers primaries [{first_primary}, {first_primary + n_primary}) "
                                f"outside the {primary.size}-ray primary batch")
        if slot_to_id.numel() != primary.size:
            raise _lib.MrtError("slot_to_id must hold one pixel id per primary ray")
        if pixels is None:
            with _on_stream(stream):
                pixels = torch.zeros(num_pixels, dtype=torch.int32, device=self.device)
        b2s = None if batch_id_to_slot is None else batch_id_to_slot.data_ptr()
        _lib.check(self.lib.mrt_reconstruct(ray_type, num_samples, first_primary, n_primary, slot_to_id.data_ptr(),
                                            primary.results.data_ptr(), b2s, batch.results.data_ptr(),
                                            self.material.data_ptr(), self.shaded.data_ptr(), pixels.data_ptr(),
                                            _stream_ptr(stream)))
        return pixels

    def reconstruct_lit(self, primary: RayBuffer, slot_to_id: torch.Tensor, num_pixels: int, batch: RayBuffer,
                        num_samples: int, normals: torch.Tensor, light, pixels: torch.Tensor | None = None,
                        batch_id_to_slot: torch.Tensor | None = None, stream=None, first_primary: int = 0) -> torch.Tensor:
        """A traced shadow batch into pixels (mrt_reconstruct_lit): per primary of the batch, the
        share of its num_samples shadow rays that reached the light, times the cosine between the
        hit triangle's normal (normals: float32 [nt, 3] on the device, DeviceRayGen.normals) and
        the direction to `light`, times the triangle's material colour; the background where the
        primary missed. The batch covers the primaries [first_primary, first_primary + batch.size
        / num_samples), as in reconstruct. Bit-identical to mrt.host.reconstruct_lit. Passing
        stream= alone is enough: pixels made here are zeroed on that stream."""
        if batch.size % num_samples:
            raise _lib.MrtError(f"batch holds {batch.size} rays, not a multiple of {num_samples}")
        n_primary = batch.size // num_samples
        if first_primary < 0 or first_primary + n_primary > primary.size:
            raise _lib.MrtError(f"batch covers primaries [{first_primary}, {first_primary + n_primary}) "
                                f"outside the {primary.size}-ray primary batch")
        if slot_to_id.numel() != primary.size:
            raise _lib.MrtError("slot_to_id must hold one pixel id per primary ray")
        if normals is None or normals.dtype != torch.float32 or normals.numel() != 3 * self.material.numel():
            raise _lib.MrtError("reconstruct_lit needs one float32 normal per triangle of the colour table")
        if pixels is None:
            with _on_stream(stream):
                pixels = torch.zeros(num_pixels, dtype=torch.int32, device=self.device)
        b2s = None if batch_id_to_slot is None else batch_id_to_slot.data_ptr()
        _lib.check(self.lib.mrt_reconstruct_lit(num_samples, first_primary, n_primary, slot_to_id.data_ptr(),
                                                primary.rays.data_ptr(), primary.results.data_ptr(), b2s,
                                                batch.results.data_ptr(), normals.data_ptr(), self.material.data_ptr(),
                                                _light3(light), pixels.data_ptr(), _stream_ptr(stream)))
        return pixels
