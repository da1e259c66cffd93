"""A shadow frame on the device (csrc/light_kernel.hip) against its CPU statement and the independent
model (tests/light_util.py, which tests/test_light.py holds the CPU statement to):

  * mrt_raygen_shadow equals mrth_shadow_rays bit for bit over the generator's edge table;
  * mrt_raygen_shadow_blocks equals the batches' rays bit for bit: blocks of 64 and 1000 rays with a
    partial last block, shuffled lists, a seed table of more than 256 batches, and 1 to 3 ranks
    through Renderer.shard on a frame of three batches;
  * mrt_reconstruct_lit equals mrth_reconstruct_lit bit for bit on the synthetic table;
  * a known answer: a floor, a square occluder and a point light, blocked and lit points derived
    by hand, and a blocker behind the light that changes nothing;
  * the trace contract of shadow batches (each ray with its own finite tmax, converging on the
    light): hit or miss equals the oracle's for every ray, in the production mode and per lane,
    every reported triangle re-verified — the AO batches' rules;
  * a Renderer frame, batch by batch, against the model's reconstruction of the whole frame from
    the oracle's results, before and after set_vertices.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mrt  # noqa: E402
import mrt.host  # noqa: E402
import light_util as L  # noqa: E402
import oracle_lib as O  # noqa: E402
import ref_meshes  # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def upload(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def buffer_of(rays, res, dev):
    from mrt.tracer import RayBuffer
    rb = RayBuffer(np.ascontiguousarray(rays, F))
    rb.results.copy_(upload(res, dev))
    return rb


# ---- A. the batch generator -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(dev):
    from mrt.raygen import DeviceRayGen
    rays, res = L.edge_inputs()
    return DeviceRayGen(), buffer_of(rays, res, dev), rays, res


@pytest.mark.parametrize("seed", L.EDGE_SEEDS)
@pytest.mark.parametrize("samples", L.EDGE_SAMPLES)
def test_device_shadow_rays_equal_the_host_on_the_edge_table(table, samples, seed):
    g, rb, rays, res = table
    for label, light, radius, _ in L.lights():
        for first in L.EDGE_FIRSTS:
            for count in L.EDGE_COUNTS:
                got = g.shadow(rb, samples, light, radius, seed=seed, first=first, count=count)
                assert not got.need_closest_hit and got.secondary
                want = mrt.host.shadow_rays(rays, res, samples, light, radius, seed=seed, first=first, count=count)
                assert L.same_rays(got.rays.cpu().numpy(), want), (label, first, count)


def test_device_shadow_rays_at_the_wrap_edges_and_the_identity_maps(table, dev):
    g, rb, rays, res = table
    light, radius = L.ORDINARY_LIGHT
    for seed_plus_task, _, _ in L.WRAP_EDGES:
        got = g.shadow(rb, 3, light, radius, seed=seed_plus_task - 2, count=3).rays.cpu().numpy()
        assert L.same_rays(got, L.shadow_rays(rays[:3], res[:3], 3, light, radius, seed_plus_task - 2)[0])
    for samples in (1, 3):
        n = 257 * samples
        out = torch.zeros((n, 8), dtype=torch.float32, device=dev)
        i2s = torch.full((n,), -1, dtype=torch.int32, device=dev)
        s2i = torch.full((n,), -1, dtype=torch.int32, device=dev)
        mrt._lib.check(mrt._lib.trace_lib().mrt_raygen_shadow(rb.rays.data_ptr(), rb.results.data_ptr(), 257, samples,
                                                              mrt.host._light3(light), radius, 1, out.data_ptr(),
                                                              i2s.data_ptr(), s2i.data_ptr(), None))
        ident = np.arange(n, dtype=np.int32)
        assert np.array_equal(i2s.cpu().numpy(), ident) and np.array_equal(s2i.cpu().numpy(), ident)
        assert L.same_rays(out.cpu().numpy(), mrt.host.shadow_rays(rays, res, samples, light, radius, seed=1, count=257))


# ---- B. the block generator ---------------------------------------------------------------------------
def batched_frame(g, rb, samples, light, radius, seeds, batch_inputs):
    parts = []
    for k, first in enumerate(range(0, rb.size, batch_inputs)):
        count = min(batch_inputs, rb.size - first)
        parts.append(g.shadow(rb, samples, light, radius, seed=seeds[k], first=first, count=count).rays)
    return torch.cat(parts).cpu().numpy()


def listed(frame, blocks, block_rays):
    return np.concatenate([frame[b * block_rays:(b + 1) * block_rays] for b in blocks])


def block_list(total, block_rays, seed):
    """Every block of the frame in a shuffled order, the partial last block last."""
    nb = -(-total // block_rays)
    full = nb - 1 if total % block_rays else nb
    order = np.random.default_rng(seed).permutation(full)
    return (np.append(order, nb - 1) if total % block_rays else order).astype(np.int32)


@pytest.mark.parametrize("block_rays,samples", [(64, 3), (1000, 3), (1000, 64), (64, 1)])
def test_block_generator_equals_the_batches(table, dev, block_rays, samples):
    g, rb, rays, res = table
    rb, rays, res = rb.view(0, 509), rays[:509], res[:509]   # 509 inputs: no sample count here makes whole blocks
    light, radius = L.ORDINARY_LIGHT
    seeds = [L.EDGE_SEEDS[1], 1, 0x9E3779B9]
    batch_inputs = 200   # batches of 200, 200 and 109 input rays
    total = rb.size * samples
    frame = batched_frame(g, rb, samples, light, radius, seeds, batch_inputs)
    # the batches are the model's, with the batch's own seed and task
    p = np.arange(rb.size)
    for k in range(3):
        sel = p // batch_inputs == k
        want, _ = L.shadow_rays(rays[sel], res[sel], samples, light, radius, seeds[k])
        assert L.same_rays(frame.reshape(rb.size, samples, 8)[sel], want)
    blocks = block_list(total, block_rays, 3)
    assert total % block_rays, "the frame's last block is partial"
    got = g.shadow_blocks(rb, samples, light, radius, seeds, batch_inputs, upload(blocks, dev), block_rays, total)
    assert not got.need_closest_hit and got.secondary
    assert L.same_rays(got.rays.cpu().numpy(), listed(frame, blocks, block_rays))
    # a proper sublist: the first two listed blocks and the last one
    if len(blocks) > 3:
        sub = blocks[[0, 1, -1]]
        n_out = sum(min(block_rays, total - int(b) * block_rays) for b in sub)
        part = g.shadow_blocks(rb, samples, light, radius, seeds, batch_inputs, upload(sub, dev), block_rays, n_out)
        assert L.same_rays(part.rays.cpu().numpy(), listed(frame, sub, block_rays))


def test_block_generator_with_a_seed_table(table, dev):
    """One input ray per batch: 512 batches, more than a launch's arguments carry."""
    g, rb, rays, res = table
    light, radius = L.ORDINARY_LIGHT
    seeds = [int(s) for s in np.random.default_rng(9).integers(0, 2**32, rb.size)]
    seeds[7], seeds[300] = 0xFFFFFFFF, 0
    assert len(seeds) > 256
    samples, block_rays = 3, 100
    total = rb.size * samples
    assert total % block_rays
    blocks = block_list(total, block_rays, 4)
    got = g.shadow_blocks(rb, samples, light, radius, seeds, 1, upload(blocks, dev), block_rays, total).rays.cpu().numpy()
    want = np.concatenate([L.shadow_rays(rays[p:p + 1], res[p:p + 1], samples, light, radius, seeds[p])[0]
                           for p in range(rb.size)])
    assert L.same_rays(got, listed(want, blocks, block_rays))


# ---- C. the lit reconstruction ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rec(dev):
    from mrt.raygen import DeviceReconstructor
    normals, material, rays, res, s2i, num_pixels = L.lit_table()
    r = object.__new__(DeviceReconstructor)   # the tables are the test's, not a scene's
    r.device, r.lib = dev, mrt._lib.trace_lib()
    r.material = upload(material.view(np.int32), dev)
    r.shaded = None
    return r, upload(normals, dev), buffer_of(rays, res, dev), upload(s2i, dev)


@pytest.mark.parametrize("first", L.LIT_FIRSTS)
def test_device_reconstruct_lit_equals_the_host(rec, dev, first):
    r, d_normals, primary, d_s2i = rec
    rng = np.random.default_rng(first)
    for light in L.lit_lights():
        for n in range(1, 65):
            for permuted in (False, True):
                case = L.lit_case(first, n, permuted, light, rng)
                batch = buffer_of(np.zeros((len(case["batch_results"]), 8), F), case["batch_results"], dev)
                b2s = upload(case["batch_id_to_slot"], dev) if permuted else None
                got = r.reconstruct_lit(primary, d_s2i, case["num_pixels"], batch, n, d_normals, light,
                                        batch_id_to_slot=b2s, first_primary=first)
                want = mrt.host.reconstruct_lit(**case)
                got = got.cpu().numpy().view(np.uint32)
                assert np.array_equal(got, want), (n, permuted, np.nonzero(got != want)[0][:8])


# ---- D. a known answer -----------------------------------------------------------------------------------
def rect(z, x0, x1, y0, y1):
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    return [[a, b, c], [a, c, d]]


def fan(z, half, hub):
    """The square [-half, half]^2 as four triangles round an interior point."""
    h = (hub[0], hub[1], z)
    c = [(-half, -half, z), (half, -half, z), (half, half, z), (-half, half, z)]
    return [[h, c[k], c[(k + 1) % 4]] for k in range(4)]


KNOWN_X = [0.0, 0.5, -0.5, 2.0, -2.0, 3.0, -3.0]
KNOWN_LIGHT = (0.0, 0.0, 2.0)


@pytest.mark.parametrize("behind", [False, True], ids=["plain", "blocker-behind-the-light"])
def test_known_answer_floor_occluder_and_point_light(dev, behind):
    """A floor of two triangles at z = 0 over [-4, 4] x [-3, 5], a square occluder at z = 1 over
    [-1, 1]^2 (four triangles round (0.3, 0.4): no primary and no shadow ray of the test meets an
    edge inside either, the floor's diagonal crossing y = 0 at x = -1 and the occluder's spokes at
    x = -0.07 and 0.5 where the rays cross at 0 and +-0.25), a point light at (0, 0, 2). Primaries
    go straight down from z = 0.5 onto (x, 0, 0). Seen from the light the occluder's shadow
    on the floor is [-2, 2]^2, so x = 0 and +-0.5 are blocked (their rays cross z = 1 at x / 2) and
    +-3 are lit. x = +-2 is no point away from the shadow's edge: it lies on the geometric edge, and
    is lit only because the ray starts 1e-4 above the floor: it crosses z = 1 at |x| = 2 (1 - (1 - 1e-4) / (2 - 1e-4)) = 1.00005, 5e-5 outside
    the occluder, some 400 float32 ulps: decided, and the oracle's trace says the same. At a lit
    point k = cos of the angle between the floor's normal and the light = 2 / sqrt(x^2 + 4) (with
    the back-off: (2 - 1e-4) / sqrt(x^2 + (2 - 1e-4)^2), 2e-5 away at the most), and the pixel is the
    material's byte 191 (0.75 rounded) times k, truncated. A second occluder behind the light, at
    z = 3, changes nothing: each ray's tmax ends at the light."""
    from mrt.raygen import DeviceRayGen, DeviceReconstructor
    from mrt.tracer import GpuBvh, RayBuffer, Tracer
    tris = rect(0.0, -4.0, 4.0, -3.0, 5.0) + fan(1.0, 1.0, (0.3, 0.4)) + (rect(3.0, -5.0, 5.0, -5.0, 5.0) if behind else [])
    v = np.array(tris, F).reshape(-1, 3)
    t = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    scene = mrt.Scene.from_arrays(v, t)
    bufs = mrt.Bvh.build_lbvh(scene).buffers()
    tracer = Tracer(0)
    tracer.set_bvh(GpuBvh(bufs))
    samples = 4
    prim = np.array([[x, 0.0, 0.5, 0.0, 0.0, 0.0, -1.0, 10.0] for x in KNOWN_X], F)
    primary = RayBuffer(prim)
    tracer.trace_batch(primary, exact_rcp=True)
    pres = primary.results_numpy()
    assert np.isin(pres[:, 0], (0, 1)).all() and (pres[:, 1].view(F) == 0.5).all()   # the floor, at t = 0.5
    g = DeviceRayGen(scene)
    sh = g.shadow(primary, samples, KNOWN_LIGHT, 0.0, seed=1)
    rays = sh.rays.cpu().numpy()
    assert L.same_rays(rays, L.shadow_rays(prim, pres, samples, KNOWN_LIGHT, 0.0, 1)[0])
    z = 2.0 - (0.5 - (0.5 - 1e-4))
    want_tmax = np.repeat(np.sqrt(np.array(KNOWN_X) ** 2 + z * z), samples)
    assert np.abs(rays[:, 7] - want_tmax).max() <= 4 * 2.4e-7   # a few ulps of a length below 4
    for speculative in (True, False):
        tracer.trace_batch(sh, exact_rcp=True, speculative=speculative)
        got = sh.results_numpy()
        blocked = np.repeat(np.abs(KNOWN_X) < 1.0, samples)
        assert np.array_equal(got[:, 0] != -1, blocked)
        assert np.isin(got[blocked, 0], (2, 3, 4, 5)).all()                      # by the occluder
        want, _, _ = O.trace(rays, *bufs, any_hit=True)
        assert np.array_equal(want[:, 0] != -1, blocked)
        assert len(O.invalid_hits(rays, got, bufs[1], bufs[2])) == 0
    rec = DeviceReconstructor(scene)
    s2i = torch.arange(len(KNOWN_X), dtype=torch.int32, device=dev)
    px = rec.reconstruct_lit(primary, s2i, len(KNOWN_X), sh, samples, g.normals, KNOWN_LIGHT).cpu().numpy().view(np.uint32)
    material = scene.tri_colors()[0]
    assert (material[:2] == 0xFFBFBFBF).all()
    for x, p in zip(KNOWN_X, px):
        k = 2.0 / np.sqrt(x * x + 4.0) if abs(x) > 1.0 else 0.0
        level = 191.0 * k
        assert abs(level - round(level)) > 0.02 or k == 0.0        # 191 * 2e-5 cannot cross an integer
        byte = int(np.floor(level))
        assert p == (0xFF000000 | byte << 16 | byte << 8 | byte), (x, hex(int(p)), byte)
    assert np.array_equal(px, mrt.host.reconstruct_lit(samples, np.arange(len(KNOWN_X)), prim, pres, got, g.normals.cpu().numpy(),
                                                       material, KNOWN_LIGHT, len(KNOWN_X)))


# ---- E. the trace contract and the Renderer's frame --------------------------------------------------------
W, H, SAMPLES = 64, 48, 4


def soup_world(name):
    if name == "random1500":
        v, t = ref_meshes.MESHES["random1500"]()
        scene = mrt.Scene.from_arrays(v, t)
        cam = mrt.host.Camera((0.3, 0.2, 4.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 45.0, 0.01, 100.0)
    else:
        scene = mrt.Scene.synthetic("bunny", 0, 1)
        cam, _ = scene.camera()
    v, t, _ = scene.arrays()
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    light = tuple(float(x) for x in (lo + (hi - lo) * np.array([0.5, 0.9, 0.9])).astype(F))   # inside the box, near its top front edge
    radius = float(F(0.1 * np.linalg.norm(hi - lo)))
    return {"scene": scene, "cam": cam, "v": v, "t": t, "bvh": mrt.Bvh.build_lbvh(scene), "light": light, "radius": radius}


@pytest.fixture(scope="module")
def worlds(dev):
    return {}


def world_of(worlds, name):
    if name not in worlds:
        worlds[name] = soup_world(name)
    return worlds[name]


def shadow_renderer(world, max_batch):
    from mrt.raygen import RAY_SHADOW
    from mrt.renderer import GlibcRand, Renderer
    from mrt.tracer import GpuBvh, Tracer
    tracer = Tracer(0)
    tracer.set_bvh(GpuBvh(world["bvh"].buffers()), on_device=True)
    r = Renderer(tracer, world["scene"], max_batch=max_batch, rand=GlibcRand())
    r.set_params(RAY_SHADOW, SAMPLES, light_pos=world["light"], light_radius=world["radius"])
    return r


@pytest.mark.parametrize("name", ["random1500", "bunny"])
def test_shadow_batches_trace_like_the_oracle(worlds, name):
    world = world_of(worlds, name)
    bufs = world["bvh"].buffers()
    r = shadow_renderer(world, 1 << 21)
    r.begin_frame(world["cam"], W, H)
    assert r.next_batch() and r.batch.size == W * H * SAMPLES and not r.batch.need_closest_hit
    rays = r.batch.rays.cpu().numpy()
    live = rays[:, 7] >= 0
    assert live.sum() >= 1000 and np.isfinite(rays[live, 7]).all()
    # every live ray ends inside the light's cube, on its own sample
    end = rays[live, 0:3].astype(np.float64) + rays[live, 4:7].astype(np.float64) * rays[live, 7:8].astype(np.float64)
    assert np.abs(end - np.array(world["light"])).max() <= world["radius"] * (1 + 1e-4)
    want, _, _ = O.trace(rays, *bufs, any_hit=True, threads=8)
    hit = want[:, 0] != -1
    print(f"{name}: {int(hit.sum())} of {int(live.sum())} live shadow rays are blocked")
    assert hit.sum() >= 100 and (live & ~hit).sum() >= 100
    for speculative in (True, False):
        r.tracer.trace_batch(r.batch, exact_rcp=True, speculative=speculative)
        assert r.tracer.last_info["stack_overflows"] == 0
        got = r.batch.results_numpy()
        assert np.array_equal(got[:, 0] != -1, hit), f"speculative={speculative}: hit/miss differs"
        assert np.array_equal(got[~hit, 1], want[~hit, 1])
        diff = np.nonzero((got[:, 0] != want[:, 0]) | (got[:, 1] != want[:, 1]))[0]
        assert len(O.invalid_hits(rays, got, bufs[1], bufs[2], which=diff)) == 0
        if not speculative:
            assert np.array_equal(got[:, :2], want[:, :2])   # the per-lane order is the oracle's


def model_frame(world, bvh_bufs, vertices, cam, seeds, batch_inputs):
    """The whole frame from the model and the oracle: primary rays from the host, every trace by the
    oracle, shadow rays and pixels by light_util. Returns (pixels, shadow rays, primary results)."""
    prim, s2i = mrt.primary_rays(cam, W, H)
    pres, _, _ = O.trace(prim, *bvh_bufs, threads=8)
    parts = []
    for k, first in enumerate(range(0, len(prim), batch_inputs)):
        sl = slice(first, min(first + batch_inputs, len(prim)))
        parts.append(L.shadow_rays(prim[sl], pres[sl], SAMPLES, world["light"], world["radius"], seeds[k])[0])
    rays = np.concatenate(parts)
    sres, _, _ = O.trace(rays, *bvh_bufs, any_hit=True, threads=8)
    normals = mrt.host.scene_attributes(vertices, world["t"], shaded=False, material=False)["normals"]
    material = world["scene"].tri_colors()[0]
    px = L.lit_pixels(SAMPLES, s2i, prim, pres, sres, normals, material, world["light"], W * H)
    return px, rays, pres


def render_by_batches(r, cam):
    from mrt.renderer import GlibcRand
    r.rand = GlibcRand()
    r.begin_frame(cam, W, H)
    px, batches = None, []
    while r.next_batch():
        r.trace_batch()
        px = r.update_result(px)
        batches.append(r.batch)
    torch.cuda.synchronize()
    return px.cpu().numpy().view(np.uint32), batches


def test_renderer_shadow_frame_equals_the_model_before_and_after_set_vertices(worlds):
    world = world_of(worlds, "random1500")
    r = shadow_renderer(world, 8192)   # 2048 primaries per batch: batches of 2048 and 1024
    v = world["v"]
    moved = (v + F(0.2) * np.sin(F(3.0) * v[:, ::-1])).astype(F)
    host_bvh = mrt.Bvh.build_lbvh(world["scene"])
    frames = []
    for vertices in (v, moved):
        if vertices is moved:
            r.set_vertices(moved)
            host_bvh.refit(moved, world["t"])
        got, batches = render_by_batches(r, world["cam"])
        assert [b.size for b in batches] == [2048 * SAMPLES, 1024 * SAMPLES]
        seeds = r.batch_seeds()
        assert seeds[0] == mrt.AO_SEED and len(seeds) == 2
        want, rays, pres = model_frame(world, host_bvh.buffers(), vertices, world["cam"], seeds, 2048)
        assert np.array_equal(r.primary.results_numpy()[:, :2], pres[:, :2])
        assert L.same_rays(torch.cat([b.rays for b in batches]).cpu().numpy(), rays)
        assert np.array_equal(got, want), f"{int((got != want).sum())} pixels differ"
        lit = (got != L.BACKGROUND) & (got != 0xFF000000)
        assert lit.sum() >= 200 and (got == L.BACKGROUND).sum() >= 50
        frames.append(got)
    assert not np.array_equal(frames[0], frames[1])


@pytest.mark.parametrize("block_rays", [64, 1000])
def test_renderer_shards_of_a_three_batch_shadow_frame(worlds, dev, block_rays):
    """61 x 47 primaries, 3 samples, at most 3000 rays per batch: batches of 1000, 1000 and 867 inputs,
    8601 rays, whose last block is partial at both block sizes. Every rank's shard, live blocks first
    and in frame order, holds the batches' rays at its blocks, and the ranks' blocks are the frame's."""
    from mrt.raygen import RAY_SHADOW
    world = world_of(worlds, "random1500")
    r = shadow_renderer(world, 3000)
    w, h, samples = 61, 47, 3
    r.set_params(RAY_SHADOW, samples, light_pos=world["light"], light_radius=world["radius"])
    r.begin_frame(world["cam"], w, h)
    parts = r.batches()
    assert [b.size for b, _ in parts] == [3000, 3000, 2601]
    frame = torch.cat([b.rays for b, _ in parts]).cpu().numpy()
    total = len(frame)
    assert total % block_rays
    for world_size in (1, 2, 3):
        for order in (0, 1):
            seen = []
            for rank in range(world_size):
                blocks, n = r.gen.shard_blocks(r.primary, samples, block_rays, world_size, rank, order)
                shard = r.shard(world_size, rank, block_rays, order=order)
                blocks = blocks.cpu().numpy()
                assert shard.size == n and not shard.need_closest_hit
                assert L.same_rays(shard.rays.cpu().numpy(), listed(frame, blocks, block_rays))
                seen += blocks.tolist()
            assert sorted(seen) == list(range(-(-total // block_rays)))
    # a shuffled list of every block through secondary_blocks
    blocks = block_list(total, block_rays, 11)
    got = r.secondary_blocks(upload(blocks, dev), total, block_rays)
    assert L.same_rays(got.rays.cpu().numpy(), listed(frame, blocks, block_rays))
