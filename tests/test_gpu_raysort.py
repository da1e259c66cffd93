"""The device ray sort (mrt_ray_sort, csrc/raysort_kernel.hip) against its CPU statement
(mrth_ray_sort, which tests/test_raysort.py pins to a numpy restatement of the key): keys, box,
rays and both id maps, over the sizes at which the launches change shape, every pass count of the
LSD sort, both box modes, the edge rays, identical rays and ids outside [0, n); then what the sort
is for: a sorted batch traces to the unsorted batch's results, the Renderer's sort_secondary frames
equal its unsorted ones, and the reference-compatible launchers do the three steps one by one."""
import ctypes as C

import numpy as np
import pytest
import torch

import mrt
import mrt.host
from mrt import _lib

import raysort_util as U

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = -123456789


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def dev_sort(gpu, rays, ids=None, drop=0, box=0):
    """RayBuffer.morton_sort of host rays, as the dict mrt.host.ray_sort returns."""
    from mrt.tracer import RayBuffer
    rb = RayBuffer(torch.from_numpy(np.array(rays, F)).to(gpu), need_closest_hit=False, secondary=True)
    s2i = None if ids is None else torch.from_numpy(np.array(ids, np.int32)).to(gpu)
    out, id_to_slot, slot_to_id, keys, bx = rb.morton_sort(s2i, drop, box, want_keys=True)
    assert out.secondary and not out.need_closest_hit and out.size == rb.size
    assert out.results.shape == (rb.size, 4) and out.results.data_ptr() != rb.results.data_ptr()
    return {"rays": out.rays.cpu().numpy(), "id_to_slot": id_to_slot.cpu().numpy(), "slot_to_id": slot_to_id.cpu().numpy(),
            "keys": keys.cpu().numpy().view(np.uint32), "box": bx.cpu().numpy()}


# ---------------------------------------------------------------- 1. device equals host
# 1: one ray; 63 / 64 / 65: around a wave; 256 / 257: around a workgroup; 70 001: 274 workgroups of
# the box reduction (more than two) and more than one rocPRIM tile. drop_levels 0, 4 and 15: the
# three-, two- and one-pass sorts.
@pytest.mark.parametrize("drop", [0, 4, 15])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 70001])
def test_device_equals_host(gpu, n, drop):
    rays = U.random_rays(n)
    for box in (0, 1):
        for ids in (None, U.shuffled_ids(n)):
            want = mrt.host.ray_sort(rays, ids, drop, box)
            got = dev_sort(gpu, rays, ids, drop, box)
            U.assert_same_sort(got, want, f"n={n} drop={drop} box={box} ids={'shuffled' if ids is not None else 'NULL'}")
            if ids is None:
                assert sorted(got["slot_to_id"].tolist()) == list(range(n))


# ---------------------------------------------------------------- 2. the CPU edge batches
@pytest.mark.parametrize("name", sorted(U.edge_batches()))
def test_edge_batches_equal_the_host(gpu, name):
    """Denormal squares and origins, NaN and infinite components, zero directions: a flushed
    denormal or a contracted multiply-add on the device would give another key."""
    rays = U.edge_batches()[name]
    for box in (0, 1):
        for drop in (0, 24):
            U.assert_same_sort(dev_sort(gpu, rays, None, drop, box), mrt.host.ray_sort(rays, None, drop, box),
                               f"{name} box={box} drop={drop}")


# ---------------------------------------------------------------- 3. identical rays
def test_identical_rays_keep_their_order(gpu):
    rays = np.tile(np.array([[1.5, -2.5, 3.5, 0.0, 0.6, 0.0, -0.8, 2.0]], F), (4096, 1))
    for drop in (0, 4, 15):
        got = dev_sort(gpu, rays, None, drop, 0)
        assert np.array_equal(got["slot_to_id"], np.arange(4096)) and np.array_equal(got["id_to_slot"], np.arange(4096))
        assert (got["keys"] == got["keys"][0]).all()


# ---------------------------------------------------------------- 4. ids outside [0, n)
def test_ids_outside_the_batch_are_never_an_index(gpu):
    """Ids n and -1 in place of two of a permutation's: outIdToSlot is a view eight entries inside
    a sentinel-filled tensor, so a missing guard shows as a changed sentinel beside it."""
    n = 257
    rays = U.random_rays(n)
    ids = U.shuffled_ids(n)
    absent = [int(ids[5]), int(ids[200])]
    assert 0 not in absent and n - 1 not in absent          # the sentinels beside the view are not theirs
    ids[5], ids[200] = n, -1
    d_rays = torch.from_numpy(rays.copy()).to(gpu)
    d_ids = torch.from_numpy(ids).to(gpu)
    out = torch.empty_like(d_rays)
    big = torch.full((n + 16,), SENTINEL, dtype=torch.int32, device=gpu)
    view = big[8:8 + n]
    slot_to_id = torch.empty(n, dtype=torch.int32, device=gpu)
    _lib.check(_lib.trace_lib().mrt_ray_sort(d_rays.data_ptr(), d_ids.data_ptr(), n, None, out.data_ptr(), view.data_ptr(),
                                             slot_to_id.data_ptr(), None, None, None))
    torch.cuda.synchronize()
    want = mrt.host.ray_sort(rays, ids)
    got = big.cpu().numpy()
    assert (got[:8] == SENTINEL).all() and (got[8 + n:] == SENTINEL).all()
    assert np.array_equal(slot_to_id.cpu().numpy(), want["slot_to_id"]) and {n, -1} <= set(want["slot_to_id"].tolist())
    inner = got[8:8 + n]
    assert (inner[absent] == SENTINEL).all() and (inner == SENTINEL).sum() == 2
    present = np.setdiff1d(np.arange(n), absent)
    assert np.array_equal(inner[present], want["id_to_slot"][present])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want["rays"].view(np.uint32))


# ---------------------------------------------------------------- 5. sorted trace equals unsorted trace
@pytest.fixture(scope="module")
def scene(gpu):
    """2 500 random triangles (the scene of tests/golden's diffuse fixture): primary rays hit and miss."""
    from mrt.tracer import GpuBvh, Tracer
    sc = mrt.Scene.synthetic("random", 2500, 1)
    tracer = Tracer(0)
    tracer.set_bvh(GpuBvh(mrt.Bvh.build(sc).buffers()))
    return sc, tracer


def test_sorted_trace_equals_unsorted_trace(gpu, scene):
    from mrt.raygen import DeviceRayGen
    sc, tracer = scene
    cam, _ = sc.camera()
    gen = DeviceRayGen(sc)
    primary, _ = gen.primary(cam, 64, 48)
    tracer.trace_batch(primary, exact_rcp=True)
    hits = int((primary.results[:, 0] >= 0).sum())
    assert 0 < hits < primary.size
    batch = gen.ao(primary, 4, cam.far, closest_hit=True)
    assert batch.size == 12288
    for drop, box in ((0, 0), (8, 1)):
        sorted_batch, id_to_slot, slot_to_id = batch.morton_sort(drop_levels=drop, box=box)
        assert sorted_batch.need_closest_hit and sorted_batch.secondary
        order = slot_to_id.cpu().numpy()
        assert sorted(order.tolist()) == list(range(batch.size)) and not np.array_equal(order, np.arange(batch.size))
        back = id_to_slot.long()
        # per lane, in the single-ray order: {id, t} as bits
        tracer.trace_batch(batch, exact_rcp=True, speculative=False)
        tracer.trace_batch(sorted_batch, exact_rcp=True, speculative=False)
        assert int((batch.results[:, 0] >= 0).sum()) > 100
        assert torch.equal(sorted_batch.results[back, :2], batch.results[:, :2])
        # the default speculative mode: t as bits (ids may differ where two triangles tie at one t)
        tracer.trace_batch(batch)
        tracer.trace_batch(sorted_batch)
        assert torch.equal(sorted_batch.results[back, 1], batch.results[:, 1])


# ---------------------------------------------------------------- 6. the Renderer
def test_renderer_sort_secondary_frames(gpu, scene):
    from mrt.renderer import GlibcRand, Renderer
    sc, tracer = scene
    cam, ao = sc.camera()
    w, h, samples = 64, 48, 4

    def frame(ray_type, sort, results_from=None):
        r = Renderer(tracer, sc, max_batch=8192, rand=GlibcRand())
        r.set_params(ray_type, samples, ao, sort_secondary=sort, sort_drop_levels=0, sort_box=1 if ray_type == 2 else 0)
        r.begin_frame(cam, w, h)
        assert r.num_batches() == 2
        pixels = torch.zeros(w * h, dtype=torch.int32, device=gpu)
        kept = []
        while r.next_batch():
            assert (r.batch_id_to_slot is not None) == sort
            if results_from is None:
                r.trace_batch()
            else:   # the unsorted batch's results, put into slot order on the host
                res = results_from[len(kept)].cpu().numpy()
                i2s = r.batch_id_to_slot.cpu().numpy()
                assert sorted(i2s.tolist()) == list(range(r.batch.size))
                moved = np.zeros_like(res)
                moved[i2s] = res
                r.batch.results.copy_(torch.from_numpy(moved).to(gpu))
            kept.append(r.batch.results.clone())
            r.update_result(pixels)
        assert len(kept) == 2
        return pixels.cpu().numpy(), kept

    # AO: pixels use hit or miss only, so they do not depend on which of two tied triangles was hit
    plain, _ = frame(1, False)
    assert len(set(plain.tolist())) >= 4                    # background and some of the five levels of 4 samples
    assert np.array_equal(frame(1, True)[0], plain)
    # diffuse: the wiring alone, with no second trace and so no tie
    plain, results = frame(2, False)
    assert len(set(plain.tolist())) > 8
    assert np.array_equal(frame(2, True, results_from=results)[0], plain)


# ---------------------------------------------------------------- 7. the reference's launchers
@pytest.mark.parametrize("n", [257, 4099])
def test_compat_launchers(gpu, n):
    lib = _lib.trace_lib()
    rays = U.random_rays(n)
    ids = U.shuffled_ids(n)
    want = mrt.host.ray_sort(rays, ids, 0, 0)
    d_rays = torch.from_numpy(rays.copy()).to(gpu)
    shape = (C.c_int32 * 2)(32, 8)

    flt_max = float(np.finfo(F).max)
    box = _lib.FindAABBOutput((C.c_float * 3)(*[flt_max] * 3), (C.c_float * 3)(*[-flt_max] * 3))
    lib.launch_findAABBKernel((n - 1) // 32 + 1, shape, C.byref(_lib.FindAABBInput(n, 32, d_rays.data_ptr())), C.byref(box))
    assert np.array_equal(np.array(list(box.aabbLo) + list(box.aabbHi), F), want["box"])
    # folding: a box that already holds more keeps it
    wide = _lib.FindAABBOutput((C.c_float * 3)(-1e30, 0.0, flt_max), (C.c_float * 3)(1e30, 0.0, -flt_max))
    lib.launch_findAABBKernel(1, shape, C.byref(_lib.FindAABBInput(n, 32, d_rays.data_ptr())), C.byref(wide))
    assert (wide.aabbLo[0], wide.aabbHi[0]) == (F(-1e30), F(1e30)) and wide.aabbLo[2] == want["box"][2]
    assert wide.aabbLo[1] == want["box"][1] and wide.aabbHi[1] == want["box"][4]

    keys = torch.full((n, 7), SENTINEL, dtype=torch.int32, device=gpu)
    lib.launch_genMortonKeysKernel(n, shape, C.byref(_lib.GenMortonKeysInput(n, box.aabbLo, box.aabbHi, d_rays.data_ptr(),
                                                                           keys.data_ptr())))
    k = keys.cpu().numpy()
    assert np.array_equal(k[:, 0], np.arange(n)) and np.array_equal(k[:, 1:].view(np.uint32), want["keys"])

    hash_ = k[:, 1:].view(np.uint32)
    order = np.lexsort([hash_[:, w] for w in range(6)])     # word 5 most significant; stable
    d_sorted = torch.from_numpy(np.ascontiguousarray(k[order])).to(gpu)
    d_ids = torch.from_numpy(ids).to(gpu)
    out = torch.empty_like(d_rays)
    id_to_slot = torch.full((n,), -1, dtype=torch.int32, device=gpu)
    slot_to_id = torch.empty(n, dtype=torch.int32, device=gpu)
    lib.launch_reorderRaysKernel(n, C.byref(_lib.ReorderRaysInput(n, d_sorted.data_ptr(), d_rays.data_ptr(), d_ids.data_ptr(),
                                                                 out.data_ptr(), id_to_slot.data_ptr(), slot_to_id.data_ptr())))
    got = {"rays": out.cpu().numpy(), "id_to_slot": id_to_slot.cpu().numpy(), "slot_to_id": slot_to_id.cpu().numpy(),
           "keys": hash_, "box": want["box"]}
    U.assert_same_sort(got, want, "launchers")
