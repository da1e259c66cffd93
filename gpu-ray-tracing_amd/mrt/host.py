"""Host-side producers of the trace inputs (scenes, SBVH/Compact2, rays).

Thin wrappers over lib/libmrt_host.so (include/mrt_host.h); every array is a
numpy array in the reference's binary layout:
  rays     float32 [n, 8]  (orig.xyz, tmin, dir.xyz, tmax)     src/rt/Util.hh:64-73
  results  int32   [n, 4]  (id, t bits, pad, pad)              src/rt/Util.hh:79-89
  nodes    int32   [k*16]  Compact2 inner nodes (64 B each)    src/rt/cuda/CudaBVH.hh:40-55
  woop     int32   [m*4]   Woop rows + (-0,-0,-0,-0) terminators
  triIndex int32   [m]     original triangle id per woop float4 slot
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib

# glibc's first rand() with the default seed: the reference's AO seed (RayGen.cc:106).
AO_SEED = 1804289383


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


@dataclass
class Camera:
    position: tuple
    forward: tuple
    up: tuple
    fov: float
    near: float
    far: float

    @classmethod
    def from_signature(cls, sig: str) -> "Camera":
        """CameraControls::decodeSignature (CameraControls.cc:374-419): the reference App's
        --camera text, e.g. the signatures of grtcmdline.txt. The signature's speed and
        keepAligned are kept as attributes."""
        c = _lib.HostCamera()
        speed, keep = C.c_float(), C.c_int32()
        _lib.check_host(_lib.host_lib().mrth_camera_decode_signature(sig.encode(), C.byref(c), C.byref(speed),
                                                                     C.byref(keep)))
        cam = cls(tuple(c.position), tuple(c.forward), tuple(c.up), c.fov_deg, c.near_dist, c.far_dist)
        cam.speed, cam.keep_aligned = float(speed.value), bool(keep.value)
        return cam

    def to_c(self) -> _lib.HostCamera:
        c = _lib.HostCamera()
        for i in range(3):
            c.position[i] = self.position[i]
            c.forward[i] = self.forward[i]
            c.up[i] = self.up[i]
        c.fov_deg, c.near_dist, c.far_dist = self.fov, self.near, self.far
        return c


class Scene:
    """A flattened triangle scene (reference src/rt/Scene.cc:35-83)."""

    def __init__(self, handle: int, name: str):
        self._h = C.c_void_p(handle)
        self.name = name
        # bound now: at interpreter exit the module's globals may already be gone when __del__ runs
        self._destroy = _lib.host_lib().mrth_scene_destroy

    @classmethod
    def synthetic(cls, name: str, param: int = 0, seed: int = 1) -> "Scene":
        h = C.c_void_p()
        _lib.check_host(_lib.host_lib().mrth_scene_synthetic(name.encode(), param, seed, C.byref(h)))
        return cls(h.value, name)

    @classmethod
    def from_obj(cls, path: str) -> "Scene":
        h = C.c_void_p()
        _lib.check_host(_lib.host_lib().mrth_scene_load_obj(path.encode(), C.byref(h)))
        return cls(h.value, path)

    @classmethod
    def from_arrays(cls, vertices, triangles, name: str = "arrays") -> "Scene":
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        h = C.c_void_p()
        _lib.check_host(_lib.host_lib().mrth_scene_from_arrays(_ptr(v), len(v), _ptr(t), len(t), C.byref(h)))
        return cls(h.value, name)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._destroy(self._h)
            self._h = C.c_void_p()

    @property
    def handle(self):
        return self._h

    @property
    def num_triangles(self) -> int:
        return int(_lib.host_lib().mrth_scene_num_triangles(self._h))

    @property
    def num_vertices(self) -> int:
        return int(_lib.host_lib().mrth_scene_num_vertices(self._h))

    def arrays(self):
        nv, nt = self.num_vertices, self.num_triangles
        v = np.empty((nv, 3), np.float32)
        t = np.empty((nt, 3), np.int32)
        n = np.empty((nt, 3), np.float32)
        _lib.check_host(_lib.host_lib().mrth_scene_copy_arrays(self._h, _ptr(v), _ptr(t), _ptr(n)))
        return v, t, n

    def hash(self) -> int:
        """Scene::hash (Scene.cc:93-101)."""
        return int(_lib.host_lib().mrth_scene_hash(self._h))

    def tri_colors(self):
        """(material, shaded) ABGR uint32 per triangle (Scene::Scene, reference Scene.cc:47-80)."""
        nt = self.num_triangles
        mat = np.empty(nt, np.uint32)
        sh = np.empty(nt, np.uint32)
        _lib.check_host(_lib.host_lib().mrth_scene_tri_colors(self._h, _ptr(mat), _ptr(sh)))
        return mat, sh

    def tri_diffuse(self) -> np.ndarray:
        """Each triangle's material diffuse colour, float32 [nt, 4] (mrth_scene_tri_diffuse): the
        OBJ's .mtl Kd / d, or the default (0.75, 0.75, 0.75, 1); scene_attributes' diffuse input."""
        out = np.empty((self.num_triangles, 4), np.float32)
        _lib.check_host(_lib.host_lib().mrth_scene_tri_diffuse(self._h, _ptr(out)))
        return out

    def camera(self):
        c = _lib.HostCamera()
        ao = C.c_float()
        _lib.check_host(_lib.host_lib().mrth_scene_camera(self._h, C.byref(c), C.byref(ao)))
        cam = Camera(tuple(c.position), tuple(c.forward), tuple(c.up), c.fov_deg, c.near_dist, c.far_dist)
        return cam, float(ao.value)


class Bvh:
    """Compact2 BVH buffers on the host (reference CudaBVH, BVHLayout_Compact2)."""

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)
        self._destroy = _lib.host_lib().mrth_bvh_destroy   # bound now, as in Scene

    @classmethod
    def build(cls, scene: Scene, max_leaf: int = 8, min_leaf: int = 1, split_alpha: float = 1e-5,
              threads: int = 0) -> "Bvh":
        p = _lib.BuildParams()
        _lib.host_lib().mrth_default_build_params(C.byref(p))
        p.max_leaf_size, p.min_leaf_size, p.split_alpha, p.threads = max_leaf, min_leaf, split_alpha, threads
        h = C.c_void_p()
        _lib.check_host(_lib.host_lib().mrth_bvh_build(scene.handle, C.byref(p), C.byref(h)))
        return cls(h.value)

    @classmethod
    def build_lbvh(cls, scene: Scene, max_leaf_size: int = 0) -> "Bvh":
        """A linear BVH (mrth_bvh_build_lbvh): Morton order, Karras hierarchy, leaves of at most
        max_leaf_size triangles (1..8; 0 = the default). The CPU statement of Tracer.build, whose
        bytes it reproduces; far faster to build than build(), slower to trace."""
        h = C.c_void_p()
        _lib.check_host(_lib.host_lib().mrth_bvh_build_lbvh(scene.handle, int(max_leaf_size), C.byref(h)))
        return cls(h.value)

    @staticmethod
    def _params(max_leaf=8, min_leaf=1, split_alpha=1e-5, threads=0):
        p = _lib.BuildParams()
        _lib.host_lib().mrth_default_build_params(C.byref(p))
        p.max_leaf_size, p.min_leaf_size, p.split_alpha, p.threads = max_leaf, min_leaf, split_alpha, threads
        return p

    @classmethod
    def cache_name(cls, scene: Scene, max_leaf: int = 8, min_leaf: int = 1, split_alpha: float = 1e-5) -> str:
        """The reference's bvhcache file name for this scene and build, "%08x.dat" of
        hashBits(scene, platform, build params, layout) (Renderer.cc:178-186)."""
        buf = C.create_string_buffer(16)
        _lib.check_host(_lib.host_lib().mrth_bvh_cache_name(scene.handle, C.byref(cls._params(max_leaf, min_leaf,
                                                                                              split_alpha)), buf))
        return buf.value.decode()

    @classmethod
    def load_or_build(cls, scene: Scene, cache_dir: str = "bvhcache", **build) -> "Bvh":
        """Renderer::getCudaBVH (Renderer.cc:157-217): read <cache_dir>/<cache_name>.dat when it
        exists, otherwise build the SBVH and write it there (creating the directory)."""
        import os
        build_keys = {k: build[k] for k in ("max_leaf", "min_leaf", "split_alpha") if k in build}
        path = os.path.join(cache_dir, cls.cache_name(scene, **build_keys))
        if os.path.exists(path):
            return cls.load(path)
        bvh = cls.build(scene, **build)
        os.makedirs(cache_dir, exist_ok=True)
        bvh.save(path)
        return bvh

    @classmethod
    def load(cls, path: str) -> "Bvh":
        h = C.c_void_p()
        _lib.check_host(_lib.host_lib().mrth_bvh_load(path.encode(), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_buffers(cls, nodes: np.ndarray, woop: np.ndarray, tri_index: np.ndarray) -> "Bvh":
        n = np.ascontiguousarray(nodes).view(np.int32)
        w = np.ascontiguousarray(woop).view(np.int32)
        t = np.ascontiguousarray(tri_index, dtype=np.int32)
        h = C.c_void_p()
        _lib.check_host(_lib.host_lib().mrth_bvh_from_buffers(_ptr(n), n.nbytes, _ptr(w), w.nbytes, _ptr(t),
                                                               t.nbytes, C.byref(h)))
        return cls(h.value)

    def save(self, path: str) -> None:
        _lib.check_host(_lib.host_lib().mrth_bvh_save(self._h, path.encode()))

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            self._destroy(self._h)
            self._h = C.c_void_p()

    def buffers(self):
        """(nodes, woop, triIndex) as int32 numpy copies."""
        pn, pw, pt = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nb, wb, tb = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check_host(_lib.host_lib().mrth_bvh_buffers(self._h, C.byref(pn), C.byref(nb), C.byref(pw),
                                                         C.byref(wb), C.byref(pt), C.byref(tb)))

        def grab(p, nbytes):
            if nbytes == 0:
                return np.zeros(0, np.int32)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), shape=(nbytes // 4,)).copy()

        return grab(pn, nb.value), grab(pw, wb.value), grab(pt, tb.value)

    def refit(self, vertices, triangles) -> None:
        """Refit in place for moved vertices of the triangles the BVH was built over
        (mrth_bvh_refit): new Woop rows, leaf boxes from whole triangles, inner boxes
        bottom-up; the topology, triIndex and the terminators stay."""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        _lib.check_host(_lib.host_lib().mrth_bvh_refit(self._h, _ptr(v), len(v), _ptr(t), len(t)))

    def optimize(self, rounds: int = 1) -> dict:
        """Re-optimise the topology in place by treelet restructuring (mrth_bvh_optimize): rounds
        passes (1..8) over the height levels, below every record the 7-leaf treelet rebuilt as
        the topology of smallest inner-box area when that is strictly smaller. Leaves, Woop rows
        and triIndex stay. The CPU statement of Tracer.optimize, whose bytes it reproduces.
        Returns rounds, levels, and per round the treelets considered and rewritten, wall ms."""
        info = _lib.HostOptimizeInfo()
        _lib.check_host(_lib.host_lib().mrth_bvh_optimize(self._h, int(rounds), C.byref(info)))
        return {"rounds": info.rounds, "levels": info.levels, "considered": list(info.considered[:info.rounds]),
                "rewritten": list(info.rewritten[:info.rounds]), "wall_ms": info.wall_ms}

    def tree_cost(self) -> dict:
        """The tree's area sums (mrth_bvh_tree_cost; the CPU statement of Tracer.tree_cost) and
        the SAH cost they give: see tree_cost_dict."""
        c = _lib.TreeCost()
        _lib.check_host(_lib.host_lib().mrth_bvh_tree_cost(self._h, C.byref(c)))
        return tree_cost_dict(c)

    def stats(self) -> dict:
        s = _lib.BvhStats()
        _lib.check_host(_lib.host_lib().mrth_bvh_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}


# The reference's default SAH costs of a node and of a triangle (Platform.hh:42-43: 1.f, 1.f).
SAH_NODE_COST = 1.0
SAH_TRIANGLE_COST = 1.0


def tree_cost_dict(c: "_lib.TreeCost") -> dict:
    """mrt_tree_cost's fields plus sah = (Cn * inner_area + Ct * leaf_tri_area) / root_area with
    the reference's Platform defaults Cn = Ct = 1 (Platform.hh:42-43); None where root_area is 0."""
    out = {k: getattr(c, k) for k, _ in c._fields_}
    out["sah"] = ((SAH_NODE_COST * c.inner_area + SAH_TRIANGLE_COST * c.leaf_tri_area) / c.root_area
                  if c.root_area > 0.0 else None)
    return out


def scene_attributes(vertices, triangles, diffuse=None, normals: bool = True, shaded: bool = True,
                     material: bool = True) -> dict:
    """A scene's per-triangle tables over plain arrays (mrth_scene_attributes; the CPU statement
    of mrt_scene_attributes, whose bits it gives): normals float32 [nt, 3], shaded and material
    ABGR uint32 [nt] (each only when asked for), and skipped, the triangles with a vertex index
    outside the vertex array (normal (0, 0, 0)). diffuse: float32 [nt, 4], None = the default
    material."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    d = None if diffuse is None else np.ascontiguousarray(diffuse, np.float32).reshape(-1, 4)
    if d is not None and len(d) != len(t):
        raise _lib.MrtError("diffuse must hold 4 floats per triangle")
    out = {}
    if normals:
        out["normals"] = np.zeros((len(t), 3), np.float32)
    if shaded:
        out["shaded"] = np.zeros(len(t), np.uint32)
    if material:
        out["material"] = np.zeros(len(t), np.uint32)
    skipped = C.c_int64(0)

    def ptr(a):
        return _ptr(a) if a is not None and a.size else None
    _lib.check_host(_lib.host_lib().mrth_scene_attributes(ptr(v), len(v), ptr(t), len(t), ptr(d),
                                                          _ptr(out["normals"]) if normals else None,
                                                          _ptr(out["shaded"]) if shaded else None,
                                                          _ptr(out["material"]) if material else None,
                                                          C.byref(skipped)))
    out["skipped"] = int(skipped.value)
    return out


def woopify(v0, v1, v2) -> np.ndarray:
    a = [(C.c_float * 3)(*map(float, v)) for v in (v0, v1, v2)]
    out = (C.c_float * 12)()
    _lib.host_lib().mrth_woopify(a[0], a[1], a[2], out)
    return np.array(out, np.float32).reshape(3, 4)


def pixel_table(w: int, h: int) -> np.ndarray:
    out = np.empty(w * h, np.int32)
    _lib.check_host(_lib.host_lib().mrth_pixel_table(w, h, _ptr(out)))
    return out


def primary_rays(cam: Camera, w: int, h: int, subpixel=(0.5, 0.5)):
    """RayGen::primary (RayGen.cc:50-72): w*h rays in Morton pixel order + slot->pixel ids.
    subpixel: sample position inside each pixel (the reference's is the centre)."""
    rays = np.empty((w * h, 8), np.float32)
    slot_to_id = np.empty(w * h, np.int32)
    c = cam.to_c()
    if tuple(subpixel) == (0.5, 0.5):
        _lib.check_host(_lib.host_lib().mrth_primary_rays(C.byref(c), w, h, _ptr(rays), _ptr(slot_to_id)))
    else:
        _lib.check_host(_lib.host_lib().mrth_primary_rays_subpixel(C.byref(c), w, h, float(subpixel[0]),
                                                                   float(subpixel[1]), _ptr(rays), _ptr(slot_to_id)))
    return rays, slot_to_id


def ao_rays(primary: np.ndarray, primary_results: np.ndarray, scene: Scene, max_dist: float,
            num_samples: int = 1, seed: int = AO_SEED) -> np.ndarray:
    p = np.ascontiguousarray(primary, np.float32)
    r = np.ascontiguousarray(primary_results).view(np.int32).reshape(-1, 4)
    out = np.empty((len(p) * num_samples, 8), np.float32)
    _lib.check_host(_lib.host_lib().mrth_ao_rays(_ptr(p), _ptr(r), len(p), scene.handle, num_samples,
                                                 float(max_dist), seed & 0xFFFFFFFF, _ptr(out)))
    return out


def count_hits(results: np.ndarray) -> int:
    r = np.ascontiguousarray(results).view(np.int32).reshape(-1, 4)
    return int(_lib.host_lib().mrth_count_hits(_ptr(r), len(r)))


def _light3(light):
    a = np.asarray(light, np.float32).reshape(-1)
    if a.shape != (3,):
        raise _lib.MrtError("a light position is three floats")
    return (C.c_float * 3)(*a.tolist())


def shadow_rays(rays: np.ndarray, results: np.ndarray, num_samples: int, light, light_radius: float,
                seed: int = AO_SEED, first: int = 0, count: int | None = None) -> np.ndarray:
    """RayGen::shadow on the host (mrth_shadow_rays; the CPU statement of DeviceRayGen.shadow,
    whose bits it gives): num_samples rays per input ray of [first, first + count) towards an
    area light at `light` (a cube of half-side light_radius), tmax the distance to each sample.
    The offset hash counts from the batch's first ray."""
    p = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    r = np.ascontiguousarray(results).view(np.int32).reshape(-1, 4)
    n = len(p) - first if count is None else count
    if first < 0 or n < 0 or first + n > len(p) or len(r) != len(p):
        raise _lib.MrtError(f"input range [{first}, {first + n}) outside the {len(p)}-ray batch")
    out = np.empty((n * num_samples, 8), np.float32)
    _lib.check_host(_lib.host_lib().mrth_shadow_rays(p.ctypes.data + 32 * first, r.ctypes.data + 16 * first, n,
                                                     num_samples, _light3(light), float(light_radius),
                                                     seed & 0xFFFFFFFF, _ptr(out) if out.size else None))
    return out


def reconstruct_lit(num_samples: int, slot_to_id, primary_rays, primary_results, batch_results, normals, material,
                    light, num_pixels: int, batch_id_to_slot=None, first_primary: int = 0,
                    num_primary: int | None = None, pixels: np.ndarray | None = None) -> np.ndarray:
    """mrth_reconstruct_lit (the CPU statement of DeviceReconstructor.reconstruct_lit, whose bits
    it gives): num_pixels uint32 ABGR pixels, untouched ones 0 (or `pixels`' own)."""
    s2i = np.ascontiguousarray(slot_to_id, np.int32)
    pr = np.ascontiguousarray(primary_rays, np.float32).reshape(-1, 8)
    pres = np.ascontiguousarray(primary_results).view(np.int32).reshape(-1, 4)
    bres = np.ascontiguousarray(batch_results).view(np.int32).reshape(-1, 4)
    nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    mat = np.ascontiguousarray(material).view(np.uint32).reshape(-1)
    b2s = None if batch_id_to_slot is None else np.ascontiguousarray(batch_id_to_slot, np.int32)
    if num_primary is None:
        num_primary = len(bres) // num_samples
    if (first_primary < 0 or first_primary + num_primary > len(pr) or len(pres) != len(pr) or len(s2i) != len(pr)
            or len(bres) < num_primary * num_samples or (b2s is not None and len(b2s) < num_primary * num_samples)):
        raise _lib.MrtError("reconstruct_lit: the batch does not fit the primary batch")
    if pixels is None:
        pixels = np.zeros(num_pixels, np.uint32)
    _lib.check_host(_lib.host_lib().mrth_reconstruct_lit(num_samples, first_primary, num_primary, _ptr(s2i), _ptr(pr),
                                                         _ptr(pres), None if b2s is None else _ptr(b2s), _ptr(bres),
                                                         _ptr(nrm), _ptr(mat), _light3(light), _ptr(pixels)))
    return pixels


def path_params(vertex: int, depth: int, num_samples: int, seed: int, light_pos, light_radius: float,
                light_color=(1.0, 1.0, 1.0), sky=(0.2, 0.4, 0.8), max_dist: float = 1.0e30,
                compact: bool = True) -> "_lib.PathExtendParams":
    """The scalar part of mrt_path_extend_params / mrth_path_extend_params; the caller sets the
    tables, counts and buffers."""
    p = _lib.PathExtendParams()
    p.vertex, p.depth, p.numSamples, p.seed = int(vertex), int(depth), int(num_samples), seed & 0xFFFFFFFF
    for name, v in (("lightPos", light_pos), ("lightColor", light_color), ("sky", sky)):
        a = np.asarray(v, np.float32).reshape(-1)
        if a.shape != (3,):
            raise _lib.MrtError(f"path: {name} is three floats")
        setattr(p, name, (C.c_float * 3)(*a.tolist()))
    p.lightRadius, p.maxDist, p.compact = float(light_radius), float(max_dist), int(bool(compact))
    return p


def path_extend(rays, results, state, radiance, normals, material, vertex: int, depth: int, num_samples: int,
                seed: int, light_pos, light_radius: float, light_color=(1.0, 1.0, 1.0), sky=(0.2, 0.4, 0.8),
                max_dist: float = 1.0e30, compact: bool = True, num_slots: int | None = None) -> dict:
    """mrth_path_extend (the CPU statement of mrt_path_extend, whose bits it gives): one vertex of
    a batch's paths. At vertex 0 rays / results are the batch's input rays (slot i starts from
    input i // num_samples; num_slots defaults to inputs * num_samples) and state is None; later
    they hold one entry per slot. radiance (float32 [paths, 4]) is added to in place. Returns
    shadow, pending, rays (None at vertex == depth) and state as arrays of num_slots entries
    (compact: the survivors first, the rest zero) and live, the survivor count."""
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    res = np.ascontiguousarray(results).view(np.int32).reshape(-1, 4)
    nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    mat = np.ascontiguousarray(material).view(np.uint32).reshape(-1)
    if radiance.dtype != np.float32 or radiance.ndim != 2 or radiance.shape[1] != 4 or not radiance.flags.c_contiguous:
        raise _lib.MrtError("path_extend: radiance is a contiguous float32 [paths, 4] array")
    if num_slots is None:
        num_slots = len(r) * num_samples if vertex == 0 else len(r)
    inputs = -(-num_slots // max(1, num_samples)) if vertex == 0 else num_slots
    st = None if state is None else np.ascontiguousarray(state).view(np.int32).reshape(-1, 4)
    if len(r) < inputs or len(res) < inputs or len(nrm) != len(mat) or (st is not None and len(st) < num_slots):
        raise _lib.MrtError("path_extend: the buffers do not hold the slots")
    p = path_params(vertex, depth, num_samples, seed, light_pos, light_radius, light_color, sky, max_dist, compact)
    out = {"shadow": np.zeros((num_slots, 8), np.float32), "pending": np.zeros((num_slots, 4), np.float32),
           "rays": np.zeros((num_slots, 8), np.float32) if vertex < depth else None,
           "state": np.zeros((num_slots, 4), np.int32)}
    live = np.full(1, -1, np.int32)
    p.triNormals, p.triMaterialColor, p.numTris = _ptr(nrm), _ptr(mat), len(mat)
    p.numSlots, p.numPaths = num_slots, len(radiance)
    p.inRays, p.inResults, p.inState = _ptr(r), _ptr(res), None if st is None else _ptr(st)
    p.outShadowRays, p.outPending, p.outState = _ptr(out["shadow"]), _ptr(out["pending"]), _ptr(out["state"])
    p.outRays = None if out["rays"] is None else _ptr(out["rays"])
    p.radiance, p.liveCount = _ptr(radiance), _ptr(live)
    _lib.check_host(_lib.host_lib().mrth_path_extend(C.byref(p)))
    out["live"] = int(live[0]) if num_slots else 0
    return out


def path_accumulate(state, pending, shadow_results, radiance, num_slots: int | None = None) -> np.ndarray:
    """mrth_path_accumulate: radiance[task] += pending where the slot's shadow result has id -1,
    over the first num_slots slots (default: all of state), in place."""
    st = np.ascontiguousarray(state).view(np.int32).reshape(-1, 4)
    pd = np.ascontiguousarray(pending, np.float32).reshape(-1, 4)
    res = np.ascontiguousarray(shadow_results).view(np.int32).reshape(-1, 4)
    n = len(st) if num_slots is None else num_slots
    if radiance.dtype != np.float32 or radiance.ndim != 2 or radiance.shape[1] != 4 or not radiance.flags.c_contiguous:
        raise _lib.MrtError("path_accumulate: radiance is a contiguous float32 [paths, 4] array")
    if n > len(st) or n > len(pd) or n > len(res):
        raise _lib.MrtError("path_accumulate: the buffers do not hold the slots")
    _lib.check_host(_lib.host_lib().mrth_path_accumulate(n, len(radiance), _ptr(st), _ptr(pd), _ptr(res), _ptr(radiance)))
    return radiance


def path_resolve(num_samples: int, slot_to_id, primary_results, radiance, num_pixels: int, first_primary: int = 0,
                 num_primary: int | None = None, pixels: np.ndarray | None = None, image: np.ndarray | None = None,
                 want_image: bool = False):
    """mrth_path_resolve: the batch's pixels (uint32 [num_pixels], untouched ones 0 or `pixels`'
    own) and, with want_image or image, the unclamped float32 [num_pixels, 4] values."""
    s2i = np.ascontiguousarray(slot_to_id, np.int32)
    pres = np.ascontiguousarray(primary_results).view(np.int32).reshape(-1, 4)
    rad = np.ascontiguousarray(radiance, np.float32).reshape(-1, 4)
    if num_primary is None:
        num_primary = len(rad) // num_samples
    if first_primary < 0 or first_primary + num_primary > len(pres) or len(s2i) != len(pres) or \
            len(rad) < num_primary * num_samples:
        raise _lib.MrtError("path_resolve: the batch does not fit the primary batch")
    if pixels is None:
        pixels = np.zeros(num_pixels, np.uint32)
    if image is None and want_image:
        image = np.zeros((num_pixels, 4), np.float32)
    _lib.check_host(_lib.host_lib().mrth_path_resolve(num_samples, first_primary, num_primary, _ptr(s2i), _ptr(pres),
                                                      _ptr(rad), _ptr(pixels), None if image is None else _ptr(image)))
    return (pixels, image) if image is not None else pixels


def denoise_features(slot_to_id, primary_rays, primary_results, normals, material, num_pixels: int,
                     guide: np.ndarray | None = None, albedo: np.ndarray | None = None):
    """mrth_denoise_features (the CPU statement of mrt_denoise_features, whose bits it gives): the
    guide records (float32 [num_pixels, 8]: normal, hit flag, position, 0) and albedos (float32
    [num_pixels, 4]) of a traced primary batch, at slot_to_id's pixels. Pixels no slot names keep
    what `guide` / `albedo` held (zeros where none is passed)."""
    s2i = np.ascontiguousarray(slot_to_id, np.int32).reshape(-1)
    r = np.ascontiguousarray(primary_rays, np.float32).reshape(-1, 8)
    res = np.ascontiguousarray(primary_results).view(np.int32).reshape(-1, 4)
    nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    mat = np.ascontiguousarray(material).view(np.uint32).reshape(-1)
    if len(r) != len(s2i) or len(res) != len(s2i) or len(nrm) != len(mat):
        raise _lib.MrtError("denoise_features: one ray and one result per slot, one normal per colour")
    if guide is None:
        guide = np.zeros((num_pixels, 8), np.float32)
    if albedo is None:
        albedo = np.zeros((num_pixels, 4), np.float32)
    for name, a, cols in (("guide", guide, 8), ("albedo", albedo, 4)):
        if a.dtype != np.float32 or a.shape != (num_pixels, cols) or not a.flags.c_contiguous:
            raise _lib.MrtError(f"denoise_features: {name} is a contiguous float32 [{num_pixels}, {cols}] array")
    _lib.check_host(_lib.host_lib().mrth_denoise_features(len(s2i), _ptr(s2i), _ptr(r), _ptr(res), _ptr(nrm), _ptr(mat),
                                                          len(mat), num_pixels, _ptr(guide), _ptr(albedo)))
    return guide, albedo


def denoise_filter(image, guide, albedo, width: int, height: int, iterations: int = 5, sigma_color: float = 1.0,
                   sigma_plane: float = 1.0, normal_squarings: int = 7, want_image: bool = True,
                   want_pixels: bool = True):
    """mrth_denoise_filter (the CPU statement of mrt_denoise_filter, whose bits it gives): the
    a-trous filter over a width x height float image. Returns (image_out float32 [w*h, 4] or None,
    pixels uint32 [w*h] or None)."""
    n = int(width) * int(height)
    img = np.ascontiguousarray(image, np.float32).reshape(-1, 4)
    gd = np.ascontiguousarray(guide, np.float32).reshape(-1, 8)
    alb = np.ascontiguousarray(albedo, np.float32).reshape(-1, 4)
    if width < 1 or height < 1 or len(img) != n or len(gd) != n or len(alb) != n:
        raise _lib.MrtError("denoise_filter: image, guide and albedo hold one entry per pixel of the frame")
    p = _lib.DenoiseParams()
    p.width, p.height, p.iterations, p.normalSquarings = int(width), int(height), int(iterations), int(normal_squarings)
    p.sigmaColor, p.sigmaPlane = float(np.float32(sigma_color)), float(np.float32(sigma_plane))
    scratch = [np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)]
    out = np.zeros((n, 4), np.float32) if want_image else None
    pixels = np.zeros(n, np.uint32) if want_pixels else None
    p.image, p.guide, p.albedo = _ptr(img), _ptr(gd), _ptr(alb)
    p.scratch[0], p.scratch[1] = _ptr(scratch[0]), _ptr(scratch[1])
    p.imageOut, p.pixels = (None if out is None else _ptr(out)), (None if pixels is None else _ptr(pixels))
    _lib.check_host(_lib.host_lib().mrth_denoise_filter(C.byref(p)))
    return out, pixels


def temporal_motion(slot_to_id, primary_rays, primary_results, triangles, vertices, prev_vertices, num_pixels: int,
                    prev_position: np.ndarray | None = None):
    """mrth_temporal_motion (the CPU statement of mrt_temporal_motion, whose bits it gives): where
    every primary hit's surface point was in the previous frame (float32 [num_pixels, 4]: the
    position and 1, zeros at a miss), at slot_to_id's pixels. Pixels no slot names keep what
    `prev_position` held (zeros where none is passed)."""
    s2i = np.ascontiguousarray(slot_to_id, np.int32).reshape(-1)
    r = np.ascontiguousarray(primary_rays, np.float32).reshape(-1, 8)
    res = np.ascontiguousarray(primary_results).view(np.int32).reshape(-1, 4)
    tri = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    pv = np.ascontiguousarray(prev_vertices, np.float32).reshape(-1, 3)
    if len(r) != len(s2i) or len(res) != len(s2i) or len(v) != len(pv):
        raise _lib.MrtError("temporal_motion: one ray and one result per slot, one previous vertex per vertex")
    if prev_position is None:
        prev_position = np.zeros((num_pixels, 4), np.float32)
    if prev_position.dtype != np.float32 or prev_position.shape != (num_pixels, 4) or not prev_position.flags.c_contiguous:
        raise _lib.MrtError(f"temporal_motion: prev_position is a contiguous float32 [{num_pixels}, 4] array")
    _lib.check_host(_lib.host_lib().mrth_temporal_motion(len(s2i), _ptr(s2i), _ptr(r), _ptr(res), _ptr(tri) if len(tri) else None,
                                                         len(tri), _ptr(v) if len(v) else None, _ptr(pv) if len(v) else None,
                                                         len(v), num_pixels, _ptr(prev_position)))
    return prev_position


def temporal_accumulate(image, guide, albedo, width: int, height: int, prev_guide=None, prev_history=None,
                        prev_world_to_screen=None, prev_subpixel=(0.5, 0.5), prev_position=None, max_history: int = 32,
                        normal_cos: float = 0.8, sigma_plane: float = 1.0, want_image: bool = True,
                        want_pixels: bool = True, have_prev: bool | None = None):
    """mrth_temporal_accumulate (the CPU statement of mrt_temporal_accumulate, whose bits it gives):
    one frame of the running mean over a width x height float image. have_prev None: whether
    prev_guide and prev_history are given. Returns (history float32 [w*h, 4], image_out float32
    [w*h, 4] or None, pixels uint32 [w*h] or None)."""
    n = int(width) * int(height)
    img = np.ascontiguousarray(image, np.float32).reshape(-1, 4)
    gd = np.ascontiguousarray(guide, np.float32).reshape(-1, 8)
    alb = np.ascontiguousarray(albedo, np.float32).reshape(-1, 4)
    pg = None if prev_guide is None else np.ascontiguousarray(prev_guide, np.float32).reshape(-1, 8)
    ph = None if prev_history is None else np.ascontiguousarray(prev_history, np.float32).reshape(-1, 4)
    pp = None if prev_position is None else np.ascontiguousarray(prev_position, np.float32).reshape(-1, 4)
    if width < 1 or height < 1 or any(a is not None and len(a) != n for a in (img, gd, alb, pg, ph, pp)):
        raise _lib.MrtError("temporal_accumulate: every buffer holds one entry per pixel of the frame")
    p = _lib.TemporalParams()
    p.width, p.height, p.maxHistory = int(width), int(height), int(max_history)
    p.havePrev = int(pg is not None and ph is not None) if have_prev is None else int(bool(have_prev))
    p.normalCos, p.sigmaPlane = float(np.float32(normal_cos)), float(np.float32(sigma_plane))
    m = np.zeros(16, np.float32) if prev_world_to_screen is None else np.asarray(prev_world_to_screen, np.float32).reshape(16)
    for i in range(16):
        p.prevWorldToScreen[i] = float(m[i])
    p.prevSubpixel[0], p.prevSubpixel[1] = float(np.float32(prev_subpixel[0])), float(np.float32(prev_subpixel[1]))
    history = np.zeros((n, 4), np.float32)
    out = np.zeros((n, 4), np.float32) if want_image else None
    pixels = np.zeros(n, np.uint32) if want_pixels else None
    p.image, p.guide, p.albedo = _ptr(img), _ptr(gd), _ptr(alb)
    p.prevPosition = None if pp is None else _ptr(pp)
    p.prevGuide, p.prevHistory = (None if pg is None else _ptr(pg)), (None if ph is None else _ptr(ph))
    p.history = _ptr(history)
    p.imageOut, p.pixels = (None if out is None else _ptr(out)), (None if pixels is None else _ptr(pixels))
    _lib.check_host(_lib.host_lib().mrth_temporal_accumulate(C.byref(p)))
    return history, out, pixels


def svgf_accumulate(image, guide, albedo, width: int, height: int, prev_guide=None, prev_history=None, prev_moments=None,
                    prev_world_to_screen=None, prev_subpixel=(0.5, 0.5), prev_position=None, max_history: int = 32,
                    normal_cos: float = 0.8, sigma_plane: float = 1.0, want_image: bool = True,
                    want_pixels: bool = True, have_prev: bool | None = None):
    """mrth_svgf_accumulate (the CPU statement of mrt_svgf_accumulate, whose bits it gives):
    temporal_accumulate with the luminance moments carried along. have_prev None: whether
    prev_guide, prev_history and prev_moments are given. Returns (history float32 [w*h, 4], moments
    float32 [w*h, 4], image_out float32 [w*h, 4] or None, pixels uint32 [w*h] or None)."""
    n = int(width) * int(height)
    img = np.ascontiguousarray(image, np.float32).reshape(-1, 4)
    gd = np.ascontiguousarray(guide, np.float32).reshape(-1, 8)
    alb = np.ascontiguousarray(albedo, np.float32).reshape(-1, 4)
    pg = None if prev_guide is None else np.ascontiguousarray(prev_guide, np.float32).reshape(-1, 8)
    ph = None if prev_history is None else np.ascontiguousarray(prev_history, np.float32).reshape(-1, 4)
    pm = None if prev_moments is None else np.ascontiguousarray(prev_moments, np.float32).reshape(-1, 4)
    pp = None if prev_position is None else np.ascontiguousarray(prev_position, np.float32).reshape(-1, 4)
    if width < 1 or height < 1 or any(a is not None and len(a) != n for a in (img, gd, alb, pg, ph, pm, pp)):
        raise _lib.MrtError("svgf_accumulate: every buffer holds one entry per pixel of the frame")
    p = _lib.SvgfAccumulateParams()
    p.width, p.height, p.maxHistory = int(width), int(height), int(max_history)
    p.havePrev = int(pg is not None and ph is not None and pm is not None) if have_prev is None else int(bool(have_prev))
    p.normalCos, p.sigmaPlane = float(np.float32(normal_cos)), float(np.float32(sigma_plane))
    m = np.zeros(16, np.float32) if prev_world_to_screen is None else np.asarray(prev_world_to_screen, np.float32).reshape(16)
    for i in range(16):
        p.prevWorldToScreen[i] = float(m[i])
    p.prevSubpixel[0], p.prevSubpixel[1] = float(np.float32(prev_subpixel[0])), float(np.float32(prev_subpixel[1]))
    history, moments = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    out = np.zeros((n, 4), np.float32) if want_image else None
    pixels = np.zeros(n, np.uint32) if want_pixels else None
    p.image, p.guide, p.albedo = _ptr(img), _ptr(gd), _ptr(alb)
    p.prevPosition = None if pp is None else _ptr(pp)
    p.prevGuide, p.prevHistory = (None if pg is None else _ptr(pg)), (None if ph is None else _ptr(ph))
    p.prevMoments = None if pm is None else _ptr(pm)
    p.history, p.moments = _ptr(history), _ptr(moments)
    p.imageOut, p.pixels = (None if out is None else _ptr(out)), (None if pixels is None else _ptr(pixels))
    _lib.check_host(_lib.host_lib().mrth_svgf_accumulate(C.byref(p)))
    return history, moments, out, pixels


def svgf_filter(image, guide, albedo, moments, width: int, height: int, iterations: int = 5, sigma_luminance: float = 4.0,
                sigma_plane: float = 1.0, normal_squarings: int = 7, want_image: bool = True, want_pixels: bool = True,
                want_variance: bool = True):
    """mrth_svgf_filter (the CPU statement of mrt_svgf_filter, whose bits it gives): the variance
    of every pixel from its moments and the variance-guided a-trous filter over a width x height
    accumulated image. Returns (image_out float32 [w*h, 4] or None, pixels uint32 [w*h] or None,
    variance float32 [w*h] or None)."""
    n = int(width) * int(height)
    img = np.ascontiguousarray(image, np.float32).reshape(-1, 4)
    gd = np.ascontiguousarray(guide, np.float32).reshape(-1, 8)
    alb = np.ascontiguousarray(albedo, np.float32).reshape(-1, 4)
    mom = np.ascontiguousarray(moments, np.float32).reshape(-1, 4)
    if width < 1 or height < 1 or len(img) != n or len(gd) != n or len(alb) != n or len(mom) != n:
        raise _lib.MrtError("svgf_filter: image, guide, albedo and moments hold one entry per pixel of the frame")
    p = _lib.SvgfFilterParams()
    p.width, p.height, p.iterations, p.normalSquarings = int(width), int(height), int(iterations), int(normal_squarings)
    p.sigmaLuminance, p.sigmaPlane = float(np.float32(sigma_luminance)), float(np.float32(sigma_plane))
    scratch = [np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)]
    out = np.zeros((n, 4), np.float32) if want_image else None
    pixels = np.zeros(n, np.uint32) if want_pixels else None
    variance = np.zeros(n, np.float32) if want_variance else None
    p.image, p.guide, p.albedo, p.moments = _ptr(img), _ptr(gd), _ptr(alb), _ptr(mom)
    p.scratch[0], p.scratch[1] = _ptr(scratch[0]), _ptr(scratch[1])
    p.imageOut, p.pixels = (None if out is None else _ptr(out)), (None if pixels is None else _ptr(pixels))
    p.varianceOut = None if variance is None else _ptr(variance)
    _lib.check_host(_lib.host_lib().mrth_svgf_filter(C.byref(p)))
    return out, pixels, variance


def ray_sort(rays, slot_to_id=None, drop_levels: int = 0, box: int = 0) -> dict:
    """RayBuffer::mortonSort on the host (mrth_ray_sort; the CPU statement of
    RayBuffer.morton_sort, whose bits it reproduces): the batch in the order of the reference's
    Morton key >> (6 * drop_levels), ties by input slot. box 0 takes the key's box over origins
    and end points (the reference), 1 over origins only. Returns numpy arrays: rays float32
    [n, 8], id_to_slot and slot_to_id int32 [n] (id_to_slot starts at -1: an id outside [0, n)
    writes no entry), keys uint32 [n, 6] in INPUT order, box float32 [6] (lo.xyz, hi.xyz)."""
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    n = len(r)
    s2i = None if slot_to_id is None else np.ascontiguousarray(slot_to_id, np.int32)
    if s2i is not None and s2i.shape != (n,):
        raise _lib.MrtError("slot_to_id must hold one id per ray")
    out = {"rays": np.zeros((n, 8), np.float32), "id_to_slot": np.full(n, -1, np.int32),
           "slot_to_id": np.zeros(n, np.int32), "keys": np.zeros((n, 6), np.uint32), "box": np.zeros(6, np.float32)}
    params = _lib.RaySortParams(drop_levels=int(drop_levels), box=int(box))
    _lib.check_host(_lib.host_lib().mrth_ray_sort(_ptr(r) if n else None, None if s2i is None else _ptr(s2i), n,
                                                  C.byref(params), _ptr(out["rays"]) if n else None,
                                                  _ptr(out["id_to_slot"]), _ptr(out["slot_to_id"]),
                                                  _ptr(out["keys"]), _ptr(out["box"])))
    return out


def write_ppm(path: str, pixels: np.ndarray, w: int, h: int, flip: bool = True) -> None:
    """Binary PPM (P6) of w*h ABGR uint32 pixels indexed y*w + x (the reference's
    PBO, Renderer.cc:221-238). flip=True writes row h-1 first: the reference drew
    the PBO with GL, whose row 0 is the bottom of the window."""
    px = np.ascontiguousarray(pixels, np.uint32).reshape(h, w)
    if flip:
        px = px[::-1]
    rgb = np.stack([px & 0xFF, (px >> 8) & 0xFF, (px >> 16) & 0xFF], axis=-1).astype(np.uint8)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(rgb.tobytes())
