"""The block path past its two former ceilings: mrt_shard_blocks' live-first order for lists
longer than the 16 384 entries one workgroup sorts in LDS (tile sort -> histogram scan ->
scatter), and mrt_raygen_ao_blocks for frames of more than 256 batches (seeds read from
device memory). The expected order is the host deal,
shard_blocks(priority=live_priority(live_block_weights(...))); the expected rays are the
frame's RayGen::batching batches."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mrt  # noqa: E402
from mrt import _lib  # noqa: E402
from mrt.dist import (live_block_weights, live_priority, shard_blocks, shard_blocks_device, shard_spans,  # noqa: E402
                      spans_index)

POISON = -0x5A5A5A5B
TILE = 16384          # list entries one workgroup sorts


def hit_pattern(name: str, n: int) -> np.ndarray:
    rng = np.random.default_rng(20261019)
    if name == "random 0.6":
        return rng.random(n) < 0.6
    if name == "random":
        return rng.random(n) < 0.5
    if name == "halves":                   # first half miss, second half hit
        return np.arange(n) >= n // 2
    if name == "alternating":
        return np.arange(n) % 2 == 0
    if name == "ramp":                     # hit density 0 -> 1 along the frame
        return rng.random(n) < np.arange(n) / n
    if name == "all hit":
        return np.ones(n, bool)
    if name == "all miss":
        return np.zeros(n, bool)
    raise KeyError(name)


def primary_results(hit: np.ndarray) -> torch.Tensor:
    res = np.zeros((len(hit), 4), np.int32)
    res[:, 0] = np.where(hit, 5, -1)
    return torch.from_numpy(res).cuda()


def library_deal(res, num_primary, samples, block, world, rank, order, capacity=None):
    """(rc, the whole poisoned buffer as numpy, numBlocks, numRays) of one mrt_shard_blocks call."""
    lib = _lib.trace_lib()
    n, m = C.c_int32(-1), C.c_int64(-1)
    _lib.check(lib.mrt_shard_blocks(None, num_primary, samples, block, world, rank, 0, None, 0, C.byref(n),
                                    C.byref(m), None))
    size = n.value
    buf = torch.full((size + 64,), POISON, dtype=torch.int32, device="cuda")
    n2, m2 = C.c_int32(-1), C.c_int64(-1)
    rc = lib.mrt_shard_blocks(res.data_ptr(), num_primary, samples, block, world, rank, order, buf.data_ptr(),
                              size if capacity is None else capacity, C.byref(n2), C.byref(m2), None)
    assert (n2.value, m2.value) == (size, m.value)           # the same with and without a buffer
    return rc, buf.cpu().numpy(), size, m.value


SYNTHETIC = [
    # numPrimary, S, blockRays, world, hit pattern, the order differs from frame order
    (16384, 1, 1, 1, "random 0.6", True),        # the one-workgroup path, control
    (16385, 1, 1, 1, "random 0.6", True),        # a second tile of one entry
    (32768, 1, 1, 1, "halves", True),            # every entry crosses a tile boundary
    (32769, 1, 1, 1, "halves", True),
    (49160, 1, 1, 1, "alternating", True),       # four tiles (the last short), two keys, ties only
    (76800, 8, 8, 1, "random", True),            # 76 800 blocks, two keys
    (76800, 3, 13, 1, "ramp", True),             # 17 724 blocks, 14 keys, a partial last block of 1 ray
    (76800, 8, 11, 3, "ramp", True),             # 55 855 blocks, > 18 000 per rank, partial (6 rays) on rank 0
    (76800, 8, 32, 1, "all hit", False),         # identity
    (76800, 8, 32, 1, "all miss", False),
    (1 << 22, 16, 4000, 1, "ramp", True),        # 16 778 blocks, keys across all three digits, partial last
    (1 << 22, 32, 8000, 1, "ramp", True),        # 16 778 blocks, quantized keys
]


@pytest.mark.gpu
@pytest.mark.parametrize("num_primary,samples,block,world,pattern,reordered", SYNTHETIC)
def test_shard_order_equals_the_host_deal(num_primary, samples, block, world, pattern, reordered):
    """Every rank's list, numBlocks and numRays, in frame order (0) and live blocks first (1),
    equal the host deal; nothing is written past the list."""
    hit = hit_pattern(pattern, num_primary)
    res = primary_results(hit)
    total = num_primary * samples
    prio = live_priority(live_block_weights(torch.from_numpy(res.cpu().numpy()), samples, block), block)
    moved = False
    for order in (0, 1):
        for rank in range(world):
            want = shard_blocks(total, world, rank, block, priority=prio if order else None)
            rc, buf, n, rays = library_deal(res, num_primary, samples, block, world, rank, order)
            assert rc == 0, _lib.trace_lib().mrt_last_error_detail().decode()
            assert n == len(want)
            assert rays == int(np.sum(np.minimum(total, (want + 1) * block) - want * block))
            got = buf[:n]
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (f"order {order} rank {rank}: {bad.size} of {n} entries differ, first at {bad[:1]}: "
                                   f"got {got[bad[:4]]}, want {want[bad[:4]]}")
            assert (buf[n:] == POISON).all(), "written past the list"
            if order:
                moved |= not np.array_equal(want, np.arange(rank, -(-total // block), world))
    assert moved == reordered          # the case sorts something (or, all hit / all miss, nothing)


@pytest.mark.gpu
@pytest.mark.parametrize("num_primary,capacity", [(76800, 76799), (76800, TILE), (100, 99)])
def test_capacity_below_the_shard_writes_nothing(num_primary, capacity):
    res = primary_results(hit_pattern("random", num_primary))
    for order in (0, 1):
        rc, buf, n, rays = library_deal(res, num_primary, 8, 8, 1, 0, order, capacity=capacity)
        assert rc == 5                                        # MRT_ERR_TOO_LARGE
        assert (n, rays) == (num_primary, num_primary * 8)
        assert (buf == POISON).all()


@pytest.mark.gpu
def test_a_long_list_outside_device_memory_is_refused_before_any_launch():
    """The tiled path asks the runtime what lies behind its pointers first: pageable host memory
    as the block list is refused like a capacity that is too small, as the results as an invalid
    argument; neither buffer is touched."""
    lib = _lib.trace_lib()
    num_primary = 76800                                       # 8 spp, 8-ray blocks: 76 800 blocks
    res = primary_results(hit_pattern("random", num_primary))
    host_list = np.full(num_primary, POISON, np.int32)
    host_res = np.zeros((num_primary, 4), np.int32)
    dev_list = torch.full((num_primary,), POISON, dtype=torch.int32, device="cuda")
    n, m = C.c_int32(-1), C.c_int64(-1)
    assert lib.mrt_shard_blocks(res.data_ptr(), num_primary, 8, 8, 1, 0, 1, host_list.ctypes.data, num_primary,
                                C.byref(n), C.byref(m), None) == 5            # MRT_ERR_TOO_LARGE
    assert lib.mrt_shard_blocks(host_res.ctypes.data, num_primary, 8, 8, 1, 0, 1, dev_list.data_ptr(), num_primary,
                                C.byref(n), C.byref(m), None) == _lib.MRT_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (host_list == POISON).all() and bool((dev_list == POISON).all())
    assert (n.value, m.value) == (num_primary, num_primary * 8)


# ---------------------------------------------------------------- a real frame


@pytest.fixture(scope="module")
def sponza():
    from mrt.tracer import GpuBvh, Tracer
    scene = mrt.Scene.synthetic("sponza", 0, 1)
    bufs = mrt.Bvh.build(scene).buffers()
    t = Tracer(0)
    t.set_bvh(GpuBvh(bufs))
    return scene, t


@pytest.mark.gpu
def test_live_first_shard_of_a_real_frame(sponza):
    """320x240 sponza, 8 spp diffuse, 32-ray blocks: 19 200 blocks (two tiles). The whole
    frame as one live-first shard holds the batches' rays at the host deal's positions, and
    its traced {id, t}, put back by the same spans, equal the batches traced one by one."""
    from mrt.renderer import Renderer
    scene, t = sponza
    cam, ao = scene.camera()
    samples, w, h, block = 8, 320, 240, 32
    r = Renderer(t, scene, max_batch=1 << 18)                 # three batches
    r.set_params(2, samples, ao)
    r.begin_frame(cam, w, h)
    hit = r.primary.results[:, 0] >= 0
    assert bool(hit.any()) and not bool(hit.all())            # the order has something to do
    n = w * h * samples
    rays, results = [], []
    while r.next_batch():
        r.trace_batch()
        rays.append(r.batch.rays)
        results.append(r.batch.results[:, :2].clone())
    frame, frame_res = torch.cat(rays), torch.cat(results)
    assert frame.shape[0] == n and len(rays) == 3

    prio = live_priority(live_block_weights(r.primary.results, samples, block).cpu(), block)
    want = shard_blocks(n, 1, 0, block, priority=prio)
    assert len(want) == 19200 > TILE and bool((want != np.arange(len(want))).any())
    blocks, m = r.gen.shard_blocks(r.primary, samples, block, 1, 0, 1)
    assert m == n and np.array_equal(blocks.cpu().numpy(), want)

    shard = r.shard(1, 0, block, order=1)
    idx = spans_index(shard_spans(n, 1, 0, block, None, prio), "cuda")
    assert shard.size == n == idx.numel()
    assert torch.equal(shard.rays, frame.index_select(0, idx))
    t.trace_batch(shard, exact_rcp=r.exact_rcp)
    back = torch.full((n, 2), POISON, dtype=torch.int32, device="cuda")
    back.index_copy_(0, idx, shard.results[:, :2].contiguous())
    assert torch.equal(back, frame_res)


# ---------------------------------------------------------------- the generator past 256 batches


@pytest.mark.gpu
@pytest.mark.parametrize("ray_type,samples,w,h,max_batch,batches,block,world", [
    (2, 8, 320, 240, 2048, 300, 1024, 3),     # the tiled kernel
    (1, 3, 97, 61, 64, 282, 100, 2),          # the per-ray kernel, ragged
    (1, 1, 97, 61, 23, 258, 64, 1),           # just past the in-argument seeds
    (1, 1, 97, 61, 24, 247, 64, 1),           # control: the in-argument seeds
])
def test_secondary_blocks_of_a_frame_of_many_batches(sponza, ray_type, samples, w, h, max_batch, batches, block,
                                                     world):
    """Each rank's shard of a real permutation of the frame's blocks is bit-identical to the
    frame's batches at its positions; the shards together hold every ray once."""
    from mrt.renderer import Renderer
    scene, t = sponza
    cam, ao = scene.camera()
    r = Renderer(t, scene, max_batch=max_batch)
    r.set_params(ray_type, samples, ao)
    r.begin_frame(cam, w, h)
    n = w * h * samples
    assert r.num_batches() == batches
    frame = torch.cat([b.rays for b, _ in r.batches()])       # seeds drawn here, in batch order
    assert frame.shape[0] == n
    nblocks = -(-n // block)
    prio = np.random.default_rng(11).integers(0, 1000, size=nblocks)
    pdev = torch.from_numpy(prio).cuda()
    seen = torch.zeros(n, dtype=torch.int32, device="cuda")
    for rank in range(world):
        blocks, m = shard_blocks_device(n, world, rank, block, priority=pdev, device="cuda")
        assert not np.array_equal(blocks.cpu().numpy(), np.arange(rank, nblocks, world))   # a real permutation
        shard = r.secondary_blocks(blocks, m, block)
        assert shard.secondary and shard.need_closest_hit == (ray_type == 2)
        idx = spans_index(shard_spans(n, world, rank, block, None, prio), "cuda")
        assert shard.size == m == idx.numel()
        assert torch.equal(shard.rays, frame.index_select(0, idx)), f"rank {rank}: shard rays differ"
        seen.index_add_(0, idx, torch.ones_like(idx, dtype=torch.int32))
    assert bool((seen == 1).all())
