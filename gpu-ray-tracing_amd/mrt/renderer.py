"""Frame orchestration on one device: the reference Renderer (src/rt/cuda/Renderer.cc:44-300)
and RayGen's batching (src/rt/ray/RayGen.cc:77-142) over the C-ABI.

  beginFrame      Renderer.cc:112-152   primary rays (Morton order) in one RayBuffer; for AO /
                                        diffuse frames they are traced first (untimed pre-pass)
  getTotalNumRays Renderer.cc:221-238   w*h for primary; primary hits * samples otherwise
  nextBatch       Renderer.cc:242-291   the next <= maxBatchSize rays (RayGen::batching,
                                        RayGen.cc:124-142): primaries [lo, hi) with
                                        hi = min(n, lo + maxBatch / numSamples), numSamples rays each,
                                        seeded by the next glibc rand() (RayGen.cc:106); with
                                        sortSecondary (Renderer.hh:67, Renderer.cc:287-288; off by
                                        default, as the reference's App leaves it) an AO / diffuse
                                        batch is then Morton-sorted (RayBuffer.morton_sort)
  traceBatch      Renderer.cc:295-300   CudaTracer::traceBatch of the current batch -> ms
  updateResult    Renderer.cc:421-445   reconstructKernel of the batch into the frame's pixels

A fourth ray type, RAY_SHADOW, runs the generator the reference wrote and never launched
(RayGen::shadow, RayGen.cc:147-183): batches of any-hit rays from the primary hits towards an area
light, batched and seeded like AO, reconstructed by DeviceReconstructor.reconstruct_lit.

A fifth, RAY_PATH, carries the same batches of primary hits through up to `depth` diffuse bounces
with a light sample at every vertex (mrt.path.PathIntegrator): next_batch starts a
batch's paths, trace_batch runs its vertices, update_result resolves it. accumulate blends the
resolved frame into the history of the frames before it (mrt.temporal), denoise filters it;
svgf does both with the luminance variance carried along to guide the filter (mrt.svgf).

The reference draws every AO/diffuse batch seed from the C library's rand()
(RayGen.cc:106; App never seeds it, so the sequence starts at glibc's
1804289383); GlibcRand restates glibc's TYPE_3 generator so batch k of a frame
gets the same seed here. Batches above 2^21 rays never exist: a frame of any
size and sample count is traced as several launches, like the reference.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .denoise import SIGMA_PLANE_FRACTION_DEFAULT, Denoiser
from .host import Camera, Scene
from .path import PathIntegrator
from . import svgf as _svgf
from . import temporal as _temporal
from .raygen import RAY_AO, RAY_DIFFUSE, RAY_PATH, RAY_PRIMARY, RAY_SHADOW, DeviceRayGen, DeviceReconstructor
from .tracer import RayBuffer, Tracer, _on_stream

MAX_BATCH_RAYS = 1 << 21   # Renderer.cc:46 m_raygen(1 << 21)
# Whether a RAY_PATH frame compacts its live paths between vertices unless set_params says
# otherwise. On: the compacted batch was faster than the in-place one on bunny (0.71x) and hairball
# (0.85x) by far more than the range of three medians (profiles/path.txt).
PATH_COMPACT_DEFAULT = True


class _PathBatch:
    """What Renderer.batch holds for a RAY_PATH batch: its size (paths), nothing to trace by itself."""

    def __init__(self, size: int):
        self.size = size


class GlibcRand:
    """glibc rand() (random_r TYPE_3: additive feedback r[i] = r[i-31] + r[i-3] over a
    table seeded by 16807 * r mod (2^31 - 1), first 310 outputs discarded, >> 1)."""

    def __init__(self, seed: int = 1):
        r = [seed & 0xFFFFFFFF]
        for i in range(1, 31):
            prev = r[-1] - (1 << 32) if r[-1] >= (1 << 31) else r[-1]
            hi, lo = divmod(prev, 127773) if prev >= 0 else (-((-prev) // 127773), -((-prev) % 127773))
            word = 16807 * lo - 2836 * hi
            r.append(word + 2147483647 if word < 0 else word)
        r += r[:3]
        for _ in range(310):
            r.append((r[-31] + r[-3]) & 0xFFFFFFFF)
        self._r = r[-34:]

    def __call__(self) -> int:
        v = (self._r[-31] + self._r[-3]) & 0xFFFFFFFF
        self._r = self._r[1:] + [v]
        return v >> 1


def batching(num_input: int, num_samples: int, start: int, max_batch: int = MAX_BATCH_RAYS):
    """RayGen::batching (RayGen.cc:124-142): the next input range [lo, hi) from `start`,
    or None when every input ray is done."""
    if num_samples < 1 or max_batch < num_samples:
        raise _lib.MrtError(f"batching: {num_samples} samples do not fit a {max_batch}-ray batch")
    if start >= num_input:
        return None
    lo = start
    return lo, min(num_input, lo + max_batch // num_samples)


class Renderer:
    """Renderer.cc on one device: one frame = a primary RayBuffer plus, for AO and
    diffuse, a sequence of <= max_batch-ray secondary batches."""

    def __init__(self, tracer: Tracer, scene: Scene, max_batch: int = MAX_BATCH_RAYS, exact_rcp: bool = True,
                 rand: GlibcRand | None = None):
        self.tracer = tracer
        self.scene = scene
        self.max_batch = int(max_batch)
        self.exact_rcp = exact_rcp
        self.rand = rand if rand is not None else GlibcRand()
        self.gen = DeviceRayGen(scene)
        self._recon = None
        self.ray_type, self.num_samples, self.ao_radius = RAY_PRIMARY, 1, 5.0
        self.light_pos, self.light_radius = (0.0, 0.0, 0.0), 0.0
        self.depth, self.light_color, self.sky, self.compact = 1, (1.0, 1.0, 1.0), (0.2, 0.4, 0.8), PATH_COMPACT_DEFAULT
        self._paths: PathIntegrator | None = None
        self.path_stats: list[int] = []   # the last path batch's live counts per vertex
        self._denoiser: Denoiser | None = None   # made by the first denoise()
        self._diagonal: float | None = None      # of the scene's box, for the default sigma_plane of denoise and accumulate
        # accumulate: made by the first call; from then on set_vertices keeps the vertices of its
        # last call (_vertices) and those the last accumulated frame saw (_motion_from, until the
        # next accumulate has reprojected through them)
        self._temporal: _temporal.TemporalAccumulator | None = None
        # svgf: its own accumulator (with moments) and accumulated image; the vertex bookkeeping is
        # shared, and _accumulated_by is whichever of the two saw the last frame: the other's history is stale
        self._svgf: _svgf.SvgfAccumulator | None = None
        self._svgf_image: torch.Tensor | None = None
        self._accumulated_by: _temporal.TemporalAccumulator | None = None
        self._vertices = self._motion_from = None
        self._moved_unseen = False    # a set_vertices before the first accumulate: its vertices were not kept
        self._temporal_tris = -1      # the triangle count the history was accumulated over
        self._subpixel = (0.5, 0.5)
        self.primary: RayBuffer | None = None
        self.slot_to_id: torch.Tensor | None = None
        self.batch: RayBuffer | None = None
        self.batch_start = 0      # first ray of the current batch in the frame's secondary-ray sequence
        self._next_input = 0      # RayGen's m_aoStartIdx
        self._new_batch = True
        self._seeds: list[int] = []   # this frame's batch seeds, drawn from rand() in batch order
        self.sort_secondary, self.sort_drop_levels, self.sort_box = False, 0, 0
        self.batch_id_to_slot: torch.Tensor | None = None   # of a sorted batch; None = the identity layout
        # set_vertices: the scene's triangles and diffuse colours on the device, the tree it rebuilt,
        # and the SAH cost its rebuild decision compares against (of the GpuBvh _baseline_of)
        self._triangles = self._diffuse = self._built = None
        self._baseline_sah, self._baseline_of = None, None

    def set_params(self, ray_type: int = RAY_PRIMARY, num_samples: int = 1, ao_radius: float = 5.0,
                   sort_secondary: bool = False, sort_drop_levels: int = 0, sort_box: int = 0,
                   light_pos=(0.0, 0.0, 0.0), light_radius: float = 0.0, depth: int = 1,
                   light_color=(1.0, 1.0, 1.0), sky=(0.2, 0.4, 0.8), compact: bool | None = None) -> None:
        """sort_secondary: Morton-sort every AO / diffuse / shadow batch before it is traced (the
        reference's sortSecondary); sort_drop_levels / sort_box: RayBuffer.morton_sort's drop_levels
        and box. light_pos / light_radius: the area light of a RAY_SHADOW frame (a cube of half-side
        light_radius round light_pos, as the reference samples it); the other types ignore them.
        RAY_PATH also takes depth (bounces after the primary hit, 0..64), light_color, sky (what a
        path that leaves the scene collects) and compact (None: PATH_COMPACT_DEFAULT): whether the
        live paths are compacted between vertices or kept in place; it cannot be sorted."""
        if ray_type not in (RAY_PRIMARY, RAY_AO, RAY_DIFFUSE, RAY_SHADOW, RAY_PATH):
            raise _lib.MrtError(f"unknown ray type {ray_type}")
        if len(tuple(light_pos)) != 3 or len(tuple(light_color)) != 3 or len(tuple(sky)) != 3:
            raise _lib.MrtError("light_pos, light_color and sky are three floats each")
        if ray_type == RAY_PATH and sort_secondary:
            raise _lib.MrtError("a RAY_PATH frame's batches are not sorted (sort_secondary)")
        if ray_type == RAY_PATH and not 0 <= int(depth) <= _lib.MRT_PATH_MAX_DEPTH:
            raise _lib.MrtError(f"depth {depth} outside 0..{_lib.MRT_PATH_MAX_DEPTH}")
        if not 0 <= int(sort_drop_levels) <= 24 or int(sort_box) not in (0, 1):
            raise _lib.MrtError(f"sort_drop_levels {sort_drop_levels} outside 0..24 or sort_box {sort_box} outside 0..1")
        self.ray_type, self.num_samples, self.ao_radius = ray_type, int(num_samples), float(ao_radius)
        self.light_pos, self.light_radius = tuple(float(x) for x in light_pos), float(light_radius)
        self.depth, self.compact = int(depth), PATH_COMPACT_DEFAULT if compact is None else bool(compact)
        self.light_color, self.sky = tuple(float(x) for x in light_color), tuple(float(x) for x in sky)
        self.sort_secondary, self.sort_drop_levels, self.sort_box = bool(sort_secondary), int(sort_drop_levels), int(sort_box)

    def set_vertices(self, vertices, stream=None, rebuild_above: float | None = None) -> dict:
        """Moved vertices of the scene's triangles (float32 [nv, 3], a device tensor; a numpy array
        is uploaded): the tracer's bound tree is refitted (Tracer.refit) and the normals and
        colours the frame path reads are recomputed on the device (set_geometry of the ray
        generator and the reconstructor), all on `stream`, nothing crossing to the host. Frames
        begun afterwards on that stream see the moved scene. Passing stream= alone is enough: the
        uploads and conversions made here are ordered on that stream too.
        rebuild_above=r: the refitted tree's SAH cost is then read (Tracer.tree_cost: one blocking
        64-byte readback) and, where it exceeds r times the baseline, the tree is rebuilt from the
        moved vertices (Tracer.build(..., on_device=True); the renderer keeps the GpuBvh alive) and
        the new tree's cost becomes the baseline. The baseline is the cost of the tree as it stood
        when this renderer first read one for the bound GpuBvh (so: pass rebuild_above from the
        first call on, and it is the built or bound tree's). None (the default) never rebuilds,
        reads no cost and adds no sync: no ratio has been shown to pay in general.
        Returns {"rebuilt", "sah", "ratio"}: the refitted tree's cost and its ratio to the baseline
        (what the decision was taken on), None where no cost was read."""
        if self.tracer.bvh is None:
            raise _lib.MrtError("Renderer.set_vertices: the tracer has no BVH")
        dev = self.gen.device
        with _on_stream(stream):   # uploads and conversions go to the stream the launches run on
            if self._triangles is None:
                _, tris, _ = self.scene.arrays()
                self._triangles = torch.from_numpy(tris).to(dev)
                self._diffuse = torch.from_numpy(self.scene.tri_diffuse()).to(dev)
            if self._recon is None:
                self._recon = DeviceReconstructor(self.scene)
            if isinstance(vertices, torch.Tensor):
                v = vertices.to(dev, torch.float32).contiguous().view(-1, 3)
            else:
                v = torch.from_numpy(np.array(vertices, np.float32).reshape(-1, 3)).to(dev)
            if self._temporal is not None or self._svgf is not None:   # the previous frame's vertices, for the reprojection
                self._keep_motion(v, dev)
            else:
                self._moved_unseen = True
        if rebuild_above is not None and self._baseline_of is not self.tracer.bvh:
            self._baseline_sah, self._baseline_of = self.tracer.tree_cost(stream)["sah"], self.tracer.bvh
        self.tracer.refit(v, self._triangles, stream=stream)
        self.gen.set_geometry(v, self._triangles, stream=stream)
        self._recon.set_geometry(v, self._triangles, self._diffuse, stream=stream)
        out = {"rebuilt": False, "sah": None, "ratio": None}
        if rebuild_above is None:
            return out
        out["sah"] = self.tracer.tree_cost(stream)["sah"]
        if out["sah"] is not None and self._baseline_sah:
            out["ratio"] = out["sah"] / self._baseline_sah
        if out["ratio"] is not None and out["ratio"] > rebuild_above:
            self._built = self.tracer.build(v, self._triangles, stream=stream, on_device=True)
            self._baseline_sah, self._baseline_of = self.tracer.tree_cost(stream)["sah"], self.tracer.bvh
            out["rebuilt"] = True
        return out

    def _keep_motion(self, v: torch.Tensor, dev) -> None:
        """set_vertices after the first accumulate() or svgf(): a device clone of v (made on the stream
        set_vertices runs on) becomes the current vertices; the ones before it, those the last
        accumulated frame saw, are kept until the next accumulate. Before any set_vertices they are
        the scene's vertices as loaded. Vertices that an earlier set_vertices brought and nobody
        kept cannot be reprojected from: the history starts over."""
        if self._vertices is None:
            if self._moved_unseen:
                for acc in (self._temporal, self._svgf):
                    if acc is not None:
                        acc.reset()
            else:
                self._vertices = torch.from_numpy(self.scene.arrays()[0]).to(dev)
        if self._motion_from is None:
            self._motion_from = self._vertices
        self._vertices = v.clone()
        self._moved_unseen = False

    def begin_frame(self, cam: Camera, w: int, h: int, subpixel=(0.5, 0.5)) -> None:
        self.cam, self.w, self.h = cam, w, h
        self._subpixel = (float(subpixel[0]), float(subpixel[1]))
        self.primary, self.slot_to_id = self.gen.primary(cam, w, h, subpixel=subpixel)
        if self.ray_type != RAY_PRIMARY:
            self.tracer.trace_batch(self.primary, exact_rcp=self.exact_rcp)
        self.batch, self.batch_start, self._next_input, self._new_batch = None, 0, 0, True
        self.batch_id_to_slot = None
        self._seeds = []

    def total_num_rays(self) -> int:
        if self.ray_type == RAY_PRIMARY:
            return self.primary.size
        return self.gen.count_hits(self.primary) * self.num_samples

    def next_batch(self) -> bool:
        if self.batch is not None:
            self.batch_start += self.batch.size
        self.batch = None
        self.batch_id_to_slot = None
        if self.ray_type == RAY_PRIMARY:
            if not self._new_batch:
                return False
            self._new_batch = False
            self.batch = self.primary
            return True
        rng = batching(self.primary.size, self.num_samples, self._next_input, self.max_batch)
        if rng is None:
            return False
        lo, hi = rng
        self._next_input = hi
        seed = self.batch_seeds(lo // self._batch_inputs() + 1)[-1]
        if self.ray_type == RAY_PATH:
            self._begin_paths(lo, hi, seed)
            return True
        if self.ray_type == RAY_SHADOW:
            self.batch = self.gen.shadow(self.primary, self.num_samples, self.light_pos, self.light_radius,
                                         seed=seed, first=lo, count=hi - lo)
        else:
            self.batch = self.gen.ao(self.primary, self.num_samples, self._max_dist(), seed=seed,
                                     closest_hit=self.ray_type == RAY_DIFFUSE, first=lo, count=hi - lo)
        if self.sort_secondary:    # Renderer.cc:287-288
            self.batch, self.batch_id_to_slot, _ = self.batch.morton_sort(drop_levels=self.sort_drop_levels,
                                                                          box=self.sort_box)
        return True

    def _begin_paths(self, lo: int, hi: int, seed: int) -> None:
        """Start the paths of primaries [lo, hi). self.batch becomes the batch's shadow rays of
        vertex 0 once trace_batch has made them; until then it is a placeholder of the batch's size,
        which is what batch_start advances by."""
        if self._recon is None:
            self._recon = DeviceReconstructor(self.scene)
        if self._paths is None:
            self._paths = PathIntegrator(self.tracer, self.gen.device)
        self._paths.begin(self.primary, lo, hi - lo, self.num_samples, self.depth, seed, self.gen.normals,
                          self._recon.material, self.light_pos, self.light_radius, self.light_color, self.sky,
                          self.cam.far, self.compact)
        self.batch = _PathBatch((hi - lo) * self.num_samples)
        self.path_stats = self._paths.stats

    def _max_dist(self) -> float:
        return self.ao_radius if self.ray_type == RAY_AO else self.cam.far

    def _batch_inputs(self) -> int:
        return self.max_batch // self.num_samples      # RayGen::batching's primaries per batch

    def num_batches(self) -> int:
        """Secondary batches of the frame (RayGen::batching, RayGen.cc:124-142)."""
        return -(-self.primary.size // self._batch_inputs()) if self.ray_type != RAY_PRIMARY else 1

    def batch_seeds(self, count: int | None = None) -> list[int]:
        """The seeds of the frame's first `count` (default: all) secondary batches: one
        rand() per batch in batch order (RayGen.cc:106), drawn once per frame and shared by
        next_batch and secondary_blocks, so both see the same sequence."""
        count = self.num_batches() if count is None else count
        while len(self._seeds) < count:
            self._seeds.append(self.rand())
        return self._seeds[:count]

    def secondary_blocks(self, blocks: torch.Tensor, num_rays: int, block_rays: int, stream=None) -> RayBuffer:
        """The frame's AO/diffuse rays at a list of block_rays-ray blocks of its ray order
        (the order next_batch's batches hold them in), generated directly in list order on the
        device (mrt_raygen_ao_blocks) — a rank's shard of the frame, or the whole frame with
        its costly blocks first, with no frame-order buffer and no gather. Bit-identical to
        the same positions of the batches. num_rays: the rays listed (mrt.dist.shard_blocks_device).
        A frame of any number of batches (any max_batch next_batch accepts): above 256 the
        generator reads the batch seeds from device scratch instead of its arguments."""
        if self.ray_type == RAY_PATH:
            raise _lib.MrtError("secondary_blocks: a RAY_PATH frame is not generated in blocks")
        if self.ray_type == RAY_PRIMARY or self.primary is None:
            raise _lib.MrtError("secondary_blocks needs an AO, diffuse or shadow frame (set_params, begin_frame)")
        if self.ray_type == RAY_SHADOW:
            return self.gen.shadow_blocks(self.primary, self.num_samples, self.light_pos, self.light_radius,
                                          self.batch_seeds(), self._batch_inputs(), blocks, block_rays, num_rays,
                                          stream=stream)
        return self.gen.ao_blocks(self.primary, self.num_samples, self._max_dist(), self.batch_seeds(),
                                  self._batch_inputs(), blocks, block_rays, num_rays,
                                  closest_hit=self.ray_type == RAY_DIFFUSE, stream=stream)

    def shard(self, world: int, rank: int, block_rays: int, order: int = 1, stream=None) -> RayBuffer:
        """Rank's shard of the frame's AO/diffuse rays for a world-rank job, generated in its
        trace order on the device: block i of block_rays rays to rank i % world, live blocks
        first (order 1) or in frame order (0) — mrt_shard_blocks, then secondary_blocks. Two
        ranks' shards hold disjoint rays; together, the frame (mrt.dist.gather_results with
        block=block_rays and priority=mrt.dist.live_priority(...) puts results back). Any
        block_rays >= 1 and any number of batches: the limit is the frame's, 2^31 - 1 rays (a
        shard of more than 16 384 blocks is ordered in tiles, with stream-ordered scratch)."""
        if self.ray_type == RAY_PATH:
            raise _lib.MrtError("shard: sharded RAY_PATH frames are not supported")
        if self.ray_type == RAY_PRIMARY or self.primary is None:
            raise _lib.MrtError("shard needs an AO, diffuse or shadow frame (set_params, begin_frame)")
        blocks, n = self.gen.shard_blocks(self.primary, self.num_samples, block_rays, world, rank, order, stream)
        return self.secondary_blocks(blocks, n, block_rays, stream)

    def trace_batch(self) -> float:
        if self.batch is None:
            raise _lib.MrtError("Renderer.trace_batch without a batch (call next_batch)")
        if self.ray_type == RAY_PATH:   # every vertex of the batch: the sum of its traces' milliseconds
            ms = self._paths.run(exact_rcp=self.exact_rcp)
            self.path_stats = self._paths.stats
            return ms
        return self.tracer.trace_batch(self.batch, exact_rcp=self.exact_rcp)

    def update_result(self, pixels: torch.Tensor | None = None, image: torch.Tensor | None = None) -> torch.Tensor:
        """reconstructKernel of the current batch into `pixels` (w*h ABGR int32). image: a RAY_PATH
        frame's unclamped values (float32 [w*h, 4]), optional; the other types ignore it."""
        if self._recon is None:
            self._recon = DeviceReconstructor(self.scene)
        n = 1 if self.ray_type == RAY_PRIMARY else self.num_samples
        if self.ray_type == RAY_PATH:
            return self._paths.resolve(self.slot_to_id, self.w * self.h, pixels=pixels, image=image)
        if self.ray_type == RAY_SHADOW:   # the generator's normals: the ones set_vertices keeps current
            return self._recon.reconstruct_lit(self.primary, self.slot_to_id, self.w * self.h, self.batch, n,
                                               self.gen.normals, self.light_pos, pixels=pixels,
                                               first_primary=self.batch_start // n,
                                               batch_id_to_slot=self.batch_id_to_slot)
        return self._recon.reconstruct(self.ray_type, self.primary, self.slot_to_id, self.w * self.h, self.batch,
                                       num_samples=n, pixels=pixels, first_primary=self.batch_start // n,
                                       batch_id_to_slot=self.batch_id_to_slot)

    def denoise(self, image: torch.Tensor, pixels: torch.Tensor | None = None, image_out: torch.Tensor | None = None,
                sigma_plane: float | None = None, stream=None, **settings):
        """The edge-avoiding wavelet filter (mrt.denoise.Denoiser) over a RAY_PATH frame's
        float image, called after the frame's last update_result(pixels, image=image): the denoised
        frame goes to pixels (w*h ABGR int32) and / or image_out (float32 [w*h, 4], not `image`
        itself); returns (pixels, image_out). The guide comes from the frame's own primary batch
        and the current normals and colours, so a frame after set_vertices is guided by the moved
        scene. settings: Denoiser.run's iterations, sigma_color and normal_squarings. sigma_plane
        None: SIGMA_PLANE_FRACTION_DEFAULT of the diagonal of the scene's box (of its vertices as
        loaded). Nothing waits on the host."""
        if self.ray_type != RAY_PATH:
            raise _lib.MrtError("Renderer.denoise: only a RAY_PATH frame is denoised")
        if self.primary is None or self._recon is None:
            raise _lib.MrtError("Renderer.denoise before begin_frame and the frame's batches")
        if self._denoiser is None:
            self._denoiser = Denoiser(self.gen.device)
        if sigma_plane is None:
            sigma_plane = self._default_sigma_plane(SIGMA_PLANE_FRACTION_DEFAULT)
        self._denoiser.set_frame(self.primary, self.slot_to_id, self.gen.normals, self._recon.material, self.w, self.h,
                                 stream=stream)
        return self._denoiser.run(image, pixels=pixels, image_out=image_out, sigma_plane=sigma_plane, stream=stream,
                                  **settings)

    def _default_sigma_plane(self, fraction: float) -> float:
        if self._diagonal is None:
            v = self.scene.arrays()[0].astype(np.float64)
            self._diagonal = float(np.linalg.norm(v.max(axis=0) - v.min(axis=0))) if len(v) else 1.0
        return max(self._diagonal, 1.0e-30) * fraction

    def accumulate(self, image: torch.Tensor, pixels: torch.Tensor | None = None, image_out: torch.Tensor | None = None,
                   sigma_plane: float | None = None, reset: bool = False, **settings):
        """Temporal accumulation (mrt.temporal.TemporalAccumulator) of a RAY_PATH frame's
        float image, called after the frame's last update_result(pixels, image=image) and before
        denoise, whose input is then image_out: the frame is blended into the running mean of the
        frames accumulated before it, found where each pixel's surface point was in the previous
        one, through the camera's motion and, after a set_vertices between the two frames, the
        triangles' motion. The result goes to pixels (w*h ABGR int32) and / or image_out (float32
        [w*h, 4], not `image` itself); returns (pixels, image_out). settings:
        TemporalAccumulator.accumulate's max_history, normal_cos and variant. sigma_plane None:
        mrt.temporal.SIGMA_PLANE_FRACTION_DEFAULT of the diagonal of the scene's box (of its vertices
        as loaded). reset=True, another frame size and another triangle count (a Tracer.build in
        between) start a new history. It takes no stream: it runs on torch's current stream, so to
        use a side stream s call it under `with torch.cuda.stream(s)`. Nothing waits on the host."""
        self._check_accumulable("accumulate")
        if self._temporal is None:
            self._temporal = _temporal.TemporalAccumulator(self.gen.device)
        return self._accumulate_with(self._temporal, image, pixels, image_out, sigma_plane, reset, settings)

    def _check_accumulable(self, what: str) -> None:
        if self.ray_type != RAY_PATH:
            raise _lib.MrtError(f"Renderer.{what}: only a RAY_PATH frame is accumulated")
        if self.primary is None or self._recon is None:
            raise _lib.MrtError(f"Renderer.{what} before begin_frame and the frame's batches")

    def _accumulate_with(self, acc, image, pixels, image_out, sigma_plane, reset, settings):
        """accumulate's and svgf's common part: the restart rules, the vertices the last accumulated
        frame saw, and acc.accumulate. A frame that the other accumulator saw last restarts acc's
        history: what acc holds is from before that frame."""
        material = self._recon.material
        if reset or material.numel() != self._temporal_tris or self._accumulated_by is not acc:
            acc.reset()
        if sigma_plane is None:
            sigma_plane = self._default_sigma_plane(_temporal.SIGMA_PLANE_FRACTION_DEFAULT)
        prev = self._motion_from
        if prev is not None and (prev.numel() != self._vertices.numel() or self._triangles.numel() != 3 * material.numel()):
            prev = None               # another mesh: nothing to reproject through
            acc.reset()
        out = acc.accumulate(self.primary, self.slot_to_id, self.gen.normals, material, self.w, self.h,
                             _temporal.world_to_screen(self.cam, self.w, self.h), self._subpixel, image,
                             pixels=pixels, image_out=image_out, triangles=self._triangles,
                             vertices=self._vertices, prev_vertices=prev, sigma_plane=sigma_plane, **settings)
        self._motion_from, self._temporal_tris, self._accumulated_by = None, material.numel(), acc
        return out

    def svgf(self, image: torch.Tensor, pixels: torch.Tensor | None = None, image_out: torch.Tensor | None = None,
             sigma_plane: float | None = None, reset: bool = False, **settings):
        """Variance-guided filtering (mrt.svgf.SvgfAccumulator) of a RAY_PATH frame's float
        image, called after the frame's last update_result(pixels, image=image) in place of
        accumulate and denoise: the frame is accumulated as accumulate does, with the moments of
        its luminance beside the colour, and then filtered with a colour weight that follows each
        pixel's variance. The result goes to pixels (w*h ABGR int32) and / or image_out (float32
        [w*h, 4], not `image` itself); returns (pixels, image_out). settings: accumulate's
        max_history and normal_cos, SvgfAccumulator.filter's iterations, sigma_luminance,
        normal_squarings and variance_out, and variant, which both take. sigma_plane and the
        restarts are accumulate's; the two share the vertices set_vertices keeps, and a frame
        after one that the other accumulated starts a new history. It takes no stream: it runs on
        torch's current stream, so to use a side stream s call it under `with torch.cuda.stream(s)`.
        Nothing waits on the host."""
        self._check_accumulable("svgf")
        unknown = set(settings) - {"max_history", "normal_cos", "variant", "iterations", "sigma_luminance", "normal_squarings",
                                   "variance_out"}
        if unknown:
            raise _lib.MrtError(f"Renderer.svgf: unknown settings {sorted(unknown)}")
        if self._svgf is None:
            self._svgf = _svgf.SvgfAccumulator(self.gen.device)
        n = self.w * self.h
        if self._svgf_image is None or self._svgf_image.numel() != 4 * n:
            self._svgf_image = torch.empty((n, 4), dtype=torch.float32, device=self.gen.device)
        if sigma_plane is None:
            sigma_plane = self._default_sigma_plane(_temporal.SIGMA_PLANE_FRACTION_DEFAULT)
        blend = {k: settings[k] for k in ("max_history", "normal_cos", "variant") if k in settings}
        self._accumulate_with(self._svgf, image, None, self._svgf_image, sigma_plane, reset, blend)
        rest = {k: settings[k] for k in ("iterations", "sigma_luminance", "normal_squarings", "variance_out", "variant")
                if k in settings}
        return self._svgf.filter(self._svgf_image, pixels=pixels, image_out=image_out, sigma_plane=sigma_plane, **rest)

    def batches(self):
        """Every batch of the frame (generated, not traced) as (RayBuffer, first ray) pairs."""
        out = []
        while self.next_batch():
            out.append((self.batch, self.batch_start))
        return out
