"""The frame path's kernels (csrc/raygen_kernel.hip) against references that do not share their
code, at the edges of their inputs (tests/frame_util.py):

  * primary_kernel against the float64 pinhole model, under the bound measured on the CPU;
  * the five AO / diffuse generators (ao_kernel, ao_per_sample_kernel, ao_blocks_kernel with seeds
    in its arguments and in a table, ao_blocks_tiled_kernel likewise) against the numpy
    restatement of the reference's kernel on the edge table, the block forms bit for bit against
    the batch form, and the generated rays traced on the table's own scene;
  * reconstruct (tiled and gathering) and the hit count on synthetic results, against the C
    oracle and a count in numpy.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mrt  # noqa: E402
import frame_util as U  # noqa: E402
import oracle_lib as O  # noqa: E402
import raygen_oracle as RO  # noqa: E402

DIR_TOL = 1e-5   # the bound tests/test_renderer.py holds the device generator to against this oracle


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def upload(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- A. primary rays ---------------------------------------------------------------------------
GPU_CAMERAS = [U.all_cameras()[3], U.all_cameras()[5], U.all_cameras()[14]] + U.HAND_CAMERAS
GPU_SIZES = [(2, 2), (7, 5), (64, 48), (128, 16)]   # 2 x 2: the one size the 1-degree camera keeps


@pytest.mark.parametrize("label,cam", GPU_CAMERAS, ids=[label for label, _ in GPU_CAMERAS])
def test_device_primary_rays_match_the_pinhole_model(dev, label, cam):
    from mrt.raygen import DeviceRayGen
    g = DeviceRayGen()
    cases = U.camera_cases(((label, cam),), GPU_SIZES)
    assert cases and (label == "fov1" or len(cases) == 4)
    for _, _, w, h in cases:
        for sp in U.SUBPIXELS:
            rb, s2i = g.primary(cam, w, h, subpixel=sp)
            s2i = s2i.cpu().numpy()
            assert np.array_equal(s2i, mrt.pixel_table(w, h))
            err = U.primary_error(rb.rays.cpu().numpy(), cam, w, h, sp, s2i)
            assert err <= U.CAMERA_BOUND, (w, h, sp, err)


def test_reference_primary_launcher_matches_the_model_and_the_pixel_table(dev):
    from mrt.raygen import nscreen_to_world
    label, cam = U.all_cameras()[3]
    w, h = 64, 48
    rays = torch.zeros((w * h, 8), dtype=torch.float32, device=dev)
    s2i = torch.full((w * h,), -1, dtype=torch.int32, device=dev)
    i2s = torch.full((w * h,), -1, dtype=torch.int32, device=dev)
    table = upload(mrt.pixel_table(w, h), dev)
    inp = U.RayGenPrimaryInput((C.c_float * 3)(*cam.position), (C.c_float * 16)(*nscreen_to_world(cam, w, h)), w, h,
                               float(cam.far), rays.data_ptr(), i2s.data_ptr(), s2i.data_ptr(), table.data_ptr())
    mrt._lib.trace_lib().launch_rayGenPrimaryKernel(w * h, C.byref(inp))
    want_table = mrt.pixel_table(w, h)
    assert np.array_equal(s2i.cpu().numpy(), want_table)
    inverse = np.empty(w * h, np.int32)
    inverse[want_table] = np.arange(w * h, dtype=np.int32)
    assert np.array_equal(i2s.cpu().numpy(), inverse)
    assert U.primary_error(rays.cpu().numpy(), cam, w, h, (0.5, 0.5), want_table) <= U.CAMERA_BOUND


# ---- B. the AO / diffuse generators --------------------------------------------------------------
@pytest.fixture(scope="module")
def table(dev):
    """The edge table on the device: (generator, input RayBuffer, rays, results, normals)."""
    from mrt.raygen import DeviceRayGen
    from mrt.tracer import RayBuffer
    v, t, normals = U.edge_scene()
    rays, res, _ = U.edge_inputs()
    g = DeviceRayGen(mrt.Scene.from_arrays(v, t))
    assert g.num_tris == 6
    rb = RayBuffer(rays)
    rb.results.copy_(upload(res, dev))
    return g, rb, rays, res, normals


@pytest.mark.parametrize("samples", U.EDGE_SAMPLES)   # 1: ao_kernel; 3 and 256: ao_per_sample_kernel
@pytest.mark.parametrize("seed", U.EDGE_SEEDS)
def test_batch_generators_equal_the_oracle_on_the_edge_table(table, seed, samples):
    g, rb, rays, res, normals = table
    got = g.ao(rb, samples, U.EDGE_MAX_DIST, seed=seed).rays.cpu().numpy()
    want = RO.ao_rays(rays, res, normals, samples, U.EDGE_MAX_DIST, seed, ftz=True)
    stats = U.compare_ao(got, want, DIR_TOL)
    print(f"seed {seed:#x} S {samples}: {stats}")
    assert stats["nan_dir"] == stats["zero_dir"] == 45 * samples
    # the device flushed the denormal origin the host keeps: ftz = True is what made this pass
    assert (got[:, 1] == 0).any() and (RO.ao_rays(rays, res, normals, 1, 1.0, seed)["origin"][:, 1] == np.float32(1e-39)).any()


def test_batch_generators_equal_the_oracle_on_tied_normals(dev):
    from mrt.raygen import DeviceRayGen
    from mrt.tracer import RayBuffer
    v, t, normals = U.tie_scene()
    rays, res = U.tie_inputs()
    g = DeviceRayGen(mrt.Scene.from_arrays(v, t))
    rb = RayBuffer(rays)
    rb.results.copy_(upload(res, dev))
    for samples in (1, 3):
        got = g.ao(rb, samples, U.EDGE_MAX_DIST, seed=1).rays.cpu().numpy()
        stats = U.compare_ao(got, RO.ao_rays(rays, res, normals, samples, U.EDGE_MAX_DIST, 1, ftz=True), DIR_TOL)
        assert stats["unit_dir"] == stats["rays"]


def batched_frame(g, rb, samples, seeds, batch_inputs):
    """The frame's rays as RayGen::batching makes them: one mrt_raygen_ao per batch."""
    parts = []
    for k, first in enumerate(range(0, rb.size, batch_inputs)):
        count = min(batch_inputs, rb.size - first)
        parts.append(g.ao(rb, samples, U.EDGE_MAX_DIST, seed=seeds[k], first=first, count=count).rays)
    return torch.cat(parts).cpu().numpy()


def listed(frame, blocks, block_rays):
    return np.concatenate([frame[b * block_rays:(b + 1) * block_rays] for b in blocks])


def block_list(total, block_rays, seed):
    """Every block of the frame in a shuffled order, the partial last block last."""
    nb = -(-total // block_rays)
    order = np.random.default_rng(seed).permutation(nb - 1) if total % block_rays else np.random.default_rng(seed).permutation(nb)
    if total % block_rays:
        order = np.append(order, nb - 1)
    return order.astype(np.int32)


# (block rays, samples, tiled): 100-ray blocks with a partial last block; 1024-ray blocks, whose
# workgroups take the tiled kernel when a tile holds at most 256 whole input rays (S = 1: 1024 input
# rays per tile, so that size stays with the plain kernel) and whose last tile runs past numInput
BLOCK_CASES = [(100, 3, False), (1024, 1, False), (1024, 4, True), (1024, 256, True)]


@pytest.mark.parametrize("block_rays,samples,tiled", BLOCK_CASES)
def test_block_generators_equal_the_batches_and_the_oracle(table, dev, block_rays, samples, tiled):
    g, rb, rays, res, normals = table
    seeds = [U.EDGE_SEEDS[1], 1, 0x9E3779B9]
    batch_inputs = 200   # batches of 200, 200 and 95 input rays
    total = rb.size * samples
    assert tiled == (block_rays % 1024 == 0 and 1024 % samples == 0 and 1024 // samples <= 256)
    assert total % block_rays, "the frame's last block is partial"
    frame = batched_frame(g, rb, samples, seeds, batch_inputs)
    want = RO.ao_rays(rays, res, normals, samples, U.EDGE_MAX_DIST, U.frame_seeds(seeds, batch_inputs, rb.size), ftz=True)
    U.compare_ao(frame, want, DIR_TOL)
    blocks = block_list(total, block_rays, 3)
    got = g.ao_blocks(rb, samples, U.EDGE_MAX_DIST, seeds, batch_inputs, upload(blocks, dev), block_rays, total)
    got = got.rays.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), listed(frame, blocks, block_rays).view(np.uint32))
    # a proper sublist too: the first two listed blocks and the partial one
    if len(blocks) > 3:
        sub = blocks[[0, 1, -1]]
        n_out = 2 * block_rays + total - (len(blocks) - 1) * block_rays
        part = g.ao_blocks(rb, samples, U.EDGE_MAX_DIST, seeds, batch_inputs, upload(sub, dev), block_rays, n_out)
        assert np.array_equal(part.rays.cpu().numpy().view(np.uint32), listed(frame, sub, block_rays).view(np.uint32))


@pytest.mark.parametrize("block_rays,samples", [(100, 3), (1024, 4)])   # ao_blocks_kernel<true>, ao_blocks_tiled_kernel<true>
def test_block_generators_with_a_seed_table(table, dev, block_rays, samples):
    """One input ray per batch: 495 batches, more than a launch's arguments carry."""
    g, rb, rays, res, normals = table
    seeds = [int(s) for s in np.random.default_rng(9).integers(0, 2**32, rb.size)]
    seeds[7], seeds[300] = 0xFFFFFFFF, 0
    assert len(seeds) > 256
    total = rb.size * samples
    blocks = block_list(total, block_rays, 4)
    got = g.ao_blocks(rb, samples, U.EDGE_MAX_DIST, seeds, 1, upload(blocks, dev), block_rays, total).rays.cpu().numpy()
    want = RO.ao_rays(rays, res, normals, samples, U.EDGE_MAX_DIST, U.frame_seeds(seeds, 1, rb.size), ftz=True)
    inverse = np.empty_like(got)
    at = np.concatenate([np.arange(b * block_rays, min((b + 1) * block_rays, total)) for b in blocks])
    inverse[at] = got
    U.compare_ao(inverse, want, DIR_TOL)
    # the two forms agree bit for bit with each other (the other block size)
    other = 1024 if block_rays == 100 else 100
    blocks2 = block_list(total, other, 5)
    got2 = g.ao_blocks(rb, samples, U.EDGE_MAX_DIST, seeds, 1, upload(blocks2, dev), other, total).rays.cpu().numpy()
    assert np.array_equal(got2.view(np.uint32), listed(inverse, blocks2, other).view(np.uint32))


def test_reference_ao_launcher_with_a_first_input_slot(table, dev):
    """launch_rayGenAOKernel passes the normals unbounded, as the reference does: the ids stay in
    [-1, numTris) here (include/mrt.h)."""
    g, rb, rays, res, normals = table
    keep = np.nonzero((res[:, 0] >= -1) & (res[:, 0] < 6))[0]
    assert len(keep) == 7 * 45
    pad = 13   # input rays before the batch, with ids that must not be read
    in_rays = np.concatenate([np.full((pad, 8), np.nan, np.float32), rays[keep]])
    in_res = np.concatenate([U.results([5] * pad), res[keep]])
    d_rays, d_res = upload(in_rays, dev), upload(in_res, dev)
    for samples in (1, 3):
        n = len(keep)
        out = torch.zeros((n * samples, 8), dtype=torch.float32, device=dev)
        o2s = torch.full((n * samples,), -1, dtype=torch.int32, device=dev)
        s2o = torch.full((n * samples,), -1, dtype=torch.int32, device=dev)
        inp = U.RayGenAOInput(pad, n, samples, U.EDGE_MAX_DIST, U.EDGE_SEEDS[1], d_rays.data_ptr(), d_res.data_ptr(),
                              out.data_ptr(), o2s.data_ptr(), s2o.data_ptr(), g.normals.data_ptr())
        mrt._lib.trace_lib().launch_rayGenAOKernel(n, C.byref(inp))
        want = RO.ao_rays(rays[keep], res[keep], normals, samples, U.EDGE_MAX_DIST, U.EDGE_SEEDS[1], ftz=True)
        U.compare_ao(out.cpu().numpy(), want, DIR_TOL)
        ident = np.arange(n * samples, dtype=np.int32)
        assert np.array_equal(o2s.cpu().numpy(), ident) and np.array_equal(s2o.cpu().numpy(), ident)


def test_generated_edge_rays_trace_like_the_oracle(table, dev):
    """The table's rays, NaN and zero directions and NaN origins among them, traced on the table's
    own scene (a zero-area triangle and a NaN vertex in its BVH)."""
    from mrt.tracer import GpuBvh, Tracer
    g, rb, rays, res, normals = table
    v, t, _ = U.edge_scene()
    nodes, woop, tri = mrt.Bvh.build_lbvh(mrt.Scene.from_arrays(v, t)).buffers()
    tracer = Tracer(0)
    tracer.set_bvh(GpuBvh((nodes, woop, tri)))
    sec = g.ao(rb, 3, U.EDGE_MAX_DIST, seed=1, closest_hit=True)
    tracer.trace_batch(sec, exact_rcp=True)
    assert tracer.last_info["stack_overflows"] == 0
    gen = sec.rays.cpu().numpy()
    got = sec.results_numpy()
    want, _, _ = O.trace(gen, nodes, woop, tri)
    hit = want[:, 0] != -1
    print(f"the oracle sees {int(hit.sum())} hits among {len(gen)} rays")
    assert hit.sum() >= 100 and (~hit).sum() >= 100
    assert U.same_bits_or_nan(got[:, 1].view(np.float32), want[:, 1].view(np.float32)).all()
    diff = np.nonzero(got[:, 0] != want[:, 0])[0]
    assert len(O.invalid_hits(gen, got, woop, tri, which=diff)) == 0
    # NaN and zero directions come back as the oracle reports them: misses that keep tmax
    odd = np.isnan(gen[:, 4:7]).any(1) | (gen[:, 4:7] == 0).all(1)
    assert odd.sum() == 2 * 45 * 3
    assert np.array_equal(got[odd, 0], want[odd, 0]) and (want[odd, 0] == -1).all()
    assert np.array_equal(got[odd, 1].view(np.float32), gen[odd, 7])


# ---- C. reconstruct and the hit count on synthetic results -----------------------------------------
@pytest.fixture(scope="module")
def rec(dev):
    from mrt.raygen import DeviceReconstructor
    mat, sh = U.colour_tables()
    r = object.__new__(DeviceReconstructor)   # the colour tables are the test's, not a scene's
    r.device, r.lib = dev, mrt._lib.trace_lib()
    r.material, r.shaded = upload(mat.view(np.int32), dev), upload(sh.view(np.int32), dev)
    return r


def buffer_of(ids, dev):
    from mrt.tracer import RayBuffer
    rb = RayBuffer(np.zeros((len(ids), 8), np.float32))
    rb.results.copy_(upload(U.results(ids), dev))
    return rb


def check_reconstruct(rec, dev, ray_type, n, prim_ids, batch_ids, s2i, num_pixels, first=0, num_primary=None):
    """Tiled path, gathering path (explicit identity batch_id_to_slot) and the C oracle, bit for bit."""
    mat, sh = U.colour_tables()
    prim, batch = buffer_of(prim_ids, dev), buffer_of(batch_ids, dev)
    d_s2i = upload(np.asarray(s2i, np.int32), dev)
    tiled = rec.reconstruct(ray_type, prim, d_s2i, num_pixels, batch=batch, num_samples=n, first_primary=first)
    ident = torch.arange(len(batch_ids), dtype=torch.int32, device=dev)
    gathered = rec.reconstruct(ray_type, prim, d_s2i, num_pixels, batch=batch, num_samples=n, first_primary=first,
                               batch_id_to_slot=ident)
    want = O.reconstruct(ray_type, n, s2i, U.results(prim_ids), U.results(batch_ids), mat, sh, num_pixels,
                         first_primary=first, num_primary=num_primary)
    tiled, gathered = tiled.cpu().numpy().view(np.uint32), gathered.cpu().numpy().view(np.uint32)
    assert np.array_equal(tiled, want), f"tiled: pixels {np.nonzero(tiled != want)[0][:8]}"
    assert np.array_equal(gathered, want), f"gathering: pixels {np.nonzero(gathered != want)[0][:8]}"
    count = len(batch_ids) // n
    touched = np.zeros(num_pixels, bool)
    touched[np.asarray(s2i)[first:first + count]] = True
    assert (tiled[~touched] == 0).all()
    assert ((tiled >> 24)[(want >> 24) == 255] == 255).all()
    return tiled


def random_ids(rng, n, miss=0.3):
    return np.where(rng.random(n) < miss, -1, rng.integers(0, 64, n)).astype(np.int32)


@pytest.mark.parametrize("num_primary", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("ray_type", [1, 2], ids=["ao", "diffuse"])
def test_reconstruct_at_the_workgroup_and_tile_boundaries(rec, dev, ray_type, num_primary):
    """256 primaries per workgroup, 16 samples per LDS tile."""
    rng = np.random.default_rng(1000 * ray_type + num_primary)
    num_pixels = num_primary + 7
    s2i = rng.permutation(num_pixels)[:num_primary].astype(np.int32)
    prim_ids = random_ids(rng, num_primary)
    seen = set()
    for n in (1, 2, 15, 16, 17, 32, 33, 255):
        pix = check_reconstruct(rec, dev, ray_type, n, prim_ids, random_ids(rng, num_primary * n, 0.5), s2i, num_pixels)
        seen.update(pix.tolist())
    assert len(seen) > min(num_primary, 20)   # images, not constants


@pytest.mark.parametrize("first", [1, 255, 256])
def test_reconstruct_of_a_later_batch(rec, dev, first):
    """A batch of RayGen::batching that covers primaries [first, first + 257) of a longer frame."""
    rng = np.random.default_rng(first)
    count, num_primary = 257, first + 257 + 5
    num_pixels = num_primary + 3
    s2i = rng.permutation(num_pixels)[:num_primary].astype(np.int32)
    prim_ids = random_ids(rng, num_primary)
    for ray_type in (1, 2):
        for n in (3, 17):
            check_reconstruct(rec, dev, ray_type, n, prim_ids, random_ids(rng, count * n, 0.5), s2i, num_pixels,
                              first=first, num_primary=count)


def test_reconstruct_averages_truncate_like_the_reference(rec, dev):
    """All-miss, all-hit and alternating batches for every n in 1..64: (n * 1.0f) * (1.0f / n) * 255
    truncated is 254 for some n (the C oracle decides which), not a rounded 255."""
    prim_ids = [3, 40, -1]
    levels = set()
    for n in range(1, 65):
        rows = [np.full(n, -1), np.full(n, 5), np.where(np.arange(n) % 2, 5, -1)]
        batch_ids = np.concatenate(rows * 3).astype(np.int32)   # the three patterns under each primary
        s2i = np.arange(9, dtype=np.int32)[::-1].copy()
        for ray_type in (1, 2):
            pix = check_reconstruct(rec, dev, ray_type, n, np.repeat(prim_ids, 3), batch_ids, s2i, 9)
            if ray_type == 1:
                levels.add(int(pix[8] & 0xFF))   # all-miss under a hit primary: white, or one below it
    assert levels == {254, 255}


def test_reconstruct_primary_with_a_permuted_table(rec, dev):
    rng = np.random.default_rng(5)
    mat, sh = U.colour_tables()
    for num_primary in (1, 256, 257):
        num_pixels = num_primary + 4
        s2i = rng.permutation(num_pixels)[:num_primary].astype(np.int32)
        ids = random_ids(rng, num_primary)
        prim = buffer_of(ids, dev)
        d_s2i = upload(s2i, dev)
        want = O.reconstruct(0, 1, s2i, U.results(ids), U.results(ids), mat, sh, num_pixels)
        got = rec.reconstruct(0, prim, d_s2i, num_pixels).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want)
        # the reference's form: the batch slot of a pixel id through batchIdToSlot
        i2s = np.zeros(num_pixels, np.int32)
        i2s[s2i] = np.arange(num_primary, dtype=np.int32)
        got = rec.reconstruct(0, prim, d_s2i, num_pixels, batch_id_to_slot=upload(i2s, dev)).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want)
        assert (got[s2i[ids == -1]] == 0xFFCC6633).all()   # the background, truncated: 51, 102, 204, 255


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 65537])
def test_count_hits_at_the_id_edges(dev, n):
    from mrt.raygen import DeviceRayGen
    rng = np.random.default_rng(n)
    ids = rng.choice(np.array([U.INT_MIN, -2, -1, 0, 1, U.INT_MAX], np.int64), n).astype(np.int32)
    rb = buffer_of(ids, dev)
    want = int((ids >= 0).sum())
    assert n < 6 or 0 < want < n
    assert DeviceRayGen().count_hits(rb) == want
    lib = mrt._lib.trace_lib()
    for shape, per_thread in (((32, 8), 16), ((64, 4), 1)):   # launch shapes the reference might pass
        blk = (C.c_int32 * 2)(*shape)
        cnt = U.CountHitsInput(n, rb.results.data_ptr() if n else None, per_thread)
        assert lib.launch_countHitsKernel(n, blk, C.byref(cnt)) == want
