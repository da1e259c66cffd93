"""A path frame on the device (csrc/path_kernel.hip) against its CPU statement and the independent
model (tests/path_util.py, which tests/test_path.py holds the CPU statement to):

  * mrt_path_extend, mrt_path_accumulate and mrt_path_resolve equal mrth_path_* bit for bit over the
    edge table, and over slot counts that cross every boundary of the compaction (a wave, a
    workgroup, a round of the scan) under every survivor pattern, the device live count included;
  * compacted and in-place frames give the same radiance bits;
  * whole Renderer frames of three batches on two scenes, vertex by vertex: after each trace the host
    statement and the model are fed the device's own results, and state, rays, radiance and pixels
    are equal bit for bit; once more after set_vertices;
  * the trace contract of the new batches: bounce batches closest-hit, shadow batches any-hit, against
    the oracle in the production mode and per lane;
  * the CPU known answers, rendered on the device.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mrt  # noqa: E402
import mrt.host  # noqa: E402
from mrt import _lib  # noqa: E402
import light_util as L  # noqa: E402
import oracle_lib as O  # noqa: E402
import path_util as P  # noqa: E402
import ref_meshes  # noqa: E402
import test_path as T  # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def upload(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)


def device_extend(dev, rays, results, state, radiance, normals, material, vertex, depth, num_samples, seed, compact,
                  num_slots=None, **scalars):
    """mrt_path_extend with mrt.host.path_extend's arguments and result; radiance is updated in place.
    Every output starts as zeros, so what the device leaves unwritten compares like the host's."""
    import ctypes as C
    n = num_slots if num_slots is not None else (len(rays) * num_samples if vertex == 0 else len(rays))
    d = {k: upload(v, dev) for k, v in dict(rays=rays, results=results, normals=normals, radiance=radiance,
                                            material=np.asarray(material).view(np.int32)).items()}
    st = None if state is None else upload(state, dev)
    out = {"shadow": torch.zeros((max(n, 1), 8), dtype=torch.float32, device=dev),
           "pending": torch.zeros((max(n, 1), 4), dtype=torch.float32, device=dev),
           "rays": torch.zeros((max(n, 1), 8), dtype=torch.float32, device=dev) if vertex < depth else None,
           "state": torch.zeros((max(n, 1), 4), dtype=torch.int32, device=dev)}
    live = torch.full((1,), -1, dtype=torch.int32, device=dev)
    p = mrt.host.path_params(vertex, depth, num_samples, seed, compact=compact, **scalars)
    p.triNormals, p.triMaterialColor, p.numTris = d["normals"].data_ptr(), d["material"].data_ptr(), len(material)
    p.numSlots, p.numPaths = n, len(radiance)
    p.inRays, p.inResults, p.inState = d["rays"].data_ptr(), d["results"].data_ptr(), None if st is None else st.data_ptr()
    p.outShadowRays, p.outPending, p.outState = out["shadow"].data_ptr(), out["pending"].data_ptr(), out["state"].data_ptr()
    p.outRays = None if out["rays"] is None else out["rays"].data_ptr()
    p.radiance, p.liveCount = d["radiance"].data_ptr(), live.data_ptr()
    _lib.check(_lib.trace_lib().mrt_path_extend(C.byref(p), None))
    torch.cuda.synchronize()
    got = {k: None if v is None else v.cpu().numpy()[:n] for k, v in out.items()}
    got["live"] = int(live.item()) if n else 0
    radiance[...] = d["radiance"].cpu().numpy()
    return got


# ---- A. each entry point against its host statement ----------------------------------------------------
@pytest.mark.parametrize("compact", [True, False], ids=["compact", "in-place"])
@pytest.mark.parametrize("samples", P.EDGE_SAMPLES)
def test_device_extend_equals_the_host_on_the_edge_table(dev, samples, compact):
    normals, material = P.edge_tables()
    rng = np.random.default_rng(samples)
    depth = 2
    for vertex in (0, 1, depth):
        for seed in (1, 0xFFFFFFF0, (0xFFFFFFF0 - vertex * P.GOLDEN) & 0xFFFFFFFF):
            rays, res, state, paths, slots = T.edge_case(rng, vertex, samples, not compact)
            radiance = rng.random((paths, 4)).astype(F)
            r_dev, r_host = radiance.copy(), radiance.copy()
            kw = dict(vertex=vertex, depth=depth, num_samples=samples, seed=seed, compact=compact, **P.EDGE_LIGHT)
            got = device_extend(dev, rays, res, state, r_dev, normals, material, **kw)
            want = mrt.host.path_extend(rays, res, state, r_host, normals, material, **kw)
            assert P.same_step(got, want) == "", (vertex, seed)
            assert P.same_floats(r_dev, r_host)
            assert want["live"] > 0 and np.isnan(want["shadow"]).any()


def test_device_extend_at_the_wrap_edges(dev):
    normals, material = P.edge_tables()
    rays, res = P.edge_inputs()
    hits = np.flatnonzero(res[:, 0] >= 0)[:8]
    rays, res = np.ascontiguousarray(rays[hits]), np.ascontiguousarray(res[hits])
    for word, x in P.WRAP_INPUTS.items():
        for vertex in (0, 1):
            state = None
            if vertex:
                state = P.edge_state(np.random.default_rng(word), 8, 8)
                state[:, 3] = np.arange(8)
            kw = dict(vertex=vertex, depth=2, num_samples=3, seed=(x - vertex * P.GOLDEN - 5) & 0xFFFFFFFF, compact=True,
                      **P.EDGE_LIGHT)
            got = device_extend(dev, rays, res, state, np.zeros((24, 4), F), normals, material, **kw)
            want = mrt.host.path_extend(rays, res, state, np.zeros((24, 4), F), normals, material, **kw)
            assert P.same_step(got, want) == "", (word, vertex)


# a wave, a workgroup, and one slot more than the scan workgroup takes in a single round
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1000, _lib.MRT_PATH_SCAN_ROUND_SLOTS + 1]


@pytest.mark.parametrize("n", COUNTS)
def test_compaction_across_every_boundary_and_survivor_pattern(dev, n):
    normals, material = P.edge_tables()
    rng = np.random.default_rng(n)
    paths = n + 17
    for label, mask in P.survivor_patterns(n, rng):
        rays, res = P.slots_for(mask, rng)
        state = P.edge_state(rng, n, paths, dead_every=0)
        for compact in (True, False):
            r_dev, r_host = np.zeros((paths, 4), F), np.zeros((paths, 4), F)
            kw = dict(vertex=1, depth=3, num_samples=3, seed=7, compact=compact, num_slots=n, **P.EDGE_LIGHT)
            got = device_extend(dev, rays, res, state, r_dev, normals, material, **kw)
            want = mrt.host.path_extend(rays, res, state, r_host, normals, material, **kw)
            assert got["live"] == int(mask.sum()) == want["live"], (label, compact)
            assert P.same_step(got, want) == "", (label, compact)
            assert P.same_floats(r_dev, r_host), (label, compact)
            if compact and n:   # the survivors, in slot order, and nothing behind them
                assert np.array_equal(got["state"][:got["live"], 3], state[np.flatnonzero(mask), 3]), label
                assert (got["state"][got["live"]:] == 0).all() and (got["shadow"][got["live"]:] == 0).all(), label


def test_device_accumulate_and_resolve_equal_the_host(dev):
    lib = _lib.trace_lib()
    rng = np.random.default_rng(8)
    for n, paths in ((1, 1), (257, 300), (1000, 1000), (70000, 80000)):
        state = P.edge_state(rng, n, paths, dead_every=5)
        pending = rng.random((n, 4)).astype(F)
        pending[::9, 0] = np.nan
        pending[1::9, 1] = 1e-39
        sres = np.zeros((n, 4), np.int32)
        sres[:, 0] = np.where(rng.random(n) < 0.5, -1, rng.integers(0, 64, n))
        radiance = rng.random((paths, 4)).astype(F)
        d = [upload(a, dev) for a in (state, pending, sres, radiance)]
        _lib.check(lib.mrt_path_accumulate(n, paths, *(t.data_ptr() for t in d), None))
        want = mrt.host.path_accumulate(state, pending, sres, radiance.copy())
        assert P.same_floats(d[3].cpu().numpy(), want)
    for samples in P.EDGE_SAMPLES:
        for first in (0, 1, 255):
            count = 300
            radiance = (rng.random((count * samples, 4)) * 1.5).astype(F)
            radiance[::31, 1] = np.nan
            radiance[5::37, 2] = -0.25
            pres = np.zeros((first + count, 4), np.int32)
            pres[:, 0] = np.where(rng.random(first + count) < 0.2, -1, 3)
            pixels = first + count + 9
            s2i = rng.permutation(pixels)[:first + count].astype(np.int32)
            d = [upload(a, dev) for a in (s2i, pres, radiance)]
            px = torch.zeros(pixels, dtype=torch.int32, device=dev)
            img = torch.zeros((pixels, 4), dtype=torch.float32, device=dev)
            _lib.check(lib.mrt_path_resolve(samples, first, count, *(t.data_ptr() for t in d), px.data_ptr(), img.data_ptr(),
                                            None))
            wp, wi = mrt.host.path_resolve(samples, s2i, pres, radiance, pixels, first_primary=first, num_primary=count,
                                           want_image=True)
            assert np.array_equal(px.cpu().numpy().view(np.uint32), wp) and P.same_floats(img.cpu().numpy(), wi)
            px2 = torch.zeros(pixels, dtype=torch.int32, device=dev)   # without the float image
            _lib.check(lib.mrt_path_resolve(samples, first, count, *(t.data_ptr() for t in d), px2.data_ptr(), None, None))
            assert torch.equal(px, px2)


# ---- B. whole frames through the Renderer -------------------------------------------------------------------------
W, H, SAMPLES, DEPTH = 64, 48, 3, 3
MAX_BATCH = 3300          # 1100 primaries per batch: batches of 1100, 1100 and 872
LIGHT_COLOR, SKY = (1.0, 0.9, 0.8), (0.2, 0.4, 0.8)


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
    light = tuple(float(x) for x in (lo + (hi - lo) * np.array([0.5, 0.9, 0.9])).astype(F))
    return {"scene": scene, "cam": cam, "v": v, "t": t, "bvh": mrt.Bvh.build_lbvh(scene), "light": light,
            "radius": float(F(0.1 * np.linalg.norm(hi - lo)))}


@pytest.fixture(scope="module")
def worlds(dev):
    return {}


def world_of(worlds, name):
    if name not in worlds:
        worlds[name] = soup_world(name)
    return worlds[name]


def path_renderer(world, max_batch, compact, samples=SAMPLES, depth=DEPTH):
    from mrt.raygen import RAY_PATH
    from mrt.renderer import GlibcRand, Renderer
    from mrt.tracer import GpuBvh, Tracer
    tracer = Tracer(0)
    tracer.set_bvh(GpuBvh(world["bvh"].buffers()), on_device=True)
    r = Renderer(tracer, world["scene"], max_batch=max_batch, rand=GlibcRand())
    r.set_params(RAY_PATH, samples, depth=depth, light_pos=world["light"], light_radius=world["radius"],
                 light_color=LIGHT_COLOR, sky=SKY, compact=compact)
    return r


def render(r, cam, dev):
    """The frame through next_batch / trace_batch / update_result: pixels, image, stats per batch."""
    from mrt.renderer import GlibcRand
    r.rand = GlibcRand()
    r.begin_frame(cam, W, H)
    px = torch.zeros(W * H, dtype=torch.int32, device=dev)
    img = torch.zeros((W * H, 4), dtype=torch.float32, device=dev)
    stats, sizes, ms = [], [], 0.0
    while r.next_batch():
        sizes.append(r.batch.size)
        ms += r.trace_batch()
        r.update_result(px, img)
        stats.append(list(r.path_stats))
    torch.cuda.synchronize()
    return px.cpu().numpy().view(np.uint32), img.cpu().numpy(), stats, sizes, ms


def render_stepwise(r, cam, dev):
    """The same frame with the integrator's steps called one by one, recording after each what the
    device holds: per batch a list of per-vertex dicts."""
    from mrt.renderer import GlibcRand
    r.rand = GlibcRand()
    r.begin_frame(cam, W, H)
    px = torch.zeros(W * H, dtype=torch.int32, device=dev)
    img = torch.zeros((W * H, 4), dtype=torch.float32, device=dev)
    batches = []
    while r.next_batch():
        g = r._paths
        rec = {"first": g.first, "count": g.count, "vertices": []}
        for b in range(g.depth + 1):
            slots = g.num_slots
            live = g.extend(b)
            m, nxt = g.num_slots, 1 - g._cur
            v = {"slots": slots, "live": live, "m": m, "shadow": g.shadow_rays[:m].cpu().numpy(),
                 "pending": g.pending[:m].cpu().numpy(), "state": g.state[nxt][:m].cpu().numpy(),
                 "rays": g.rays[nxt][:m].cpu().numpy() if b < g.depth else None,
                 "radiance_after_extend": g.radiance[:g.num_paths].cpu().numpy()}
            rec["vertices"].append(v)
            if live == 0:
                break
            g.trace_shadow(exact_rcp=True)
            v["shadow_results"] = g.shadow_results[:m].cpu().numpy()
            g.accumulate()
            v["radiance"] = g.radiance[:g.num_paths].cpu().numpy()
            if b < g.depth:
                g.trace_bounce(exact_rcp=True)
                v["bounce_results"] = g.results[g._cur][:m].cpu().numpy()
        r.update_result(px, img)
        batches.append(rec)
    torch.cuda.synchronize()
    return px.cpu().numpy().view(np.uint32), img.cpu().numpy(), batches


def replay(impl, r, world, vertices, batches, compact):
    """The frame by impl (mrt.host or the model) from the device's primary results and, after each
    trace, the device's own results: every vertex's records, the radiance and the pixels are compared
    with what the device held."""
    prim, pres = r.primary.rays.cpu().numpy(), r.primary.results_numpy()
    s2i = r.slot_to_id.cpu().numpy()
    normals = mrt.host.scene_attributes(vertices, world["t"], shaded=False, material=False)["normals"]
    material = world["scene"].tri_colors()[0]
    scalars = dict(light_pos=world["light"], light_radius=world["radius"], light_color=LIGHT_COLOR, sky=SKY,
                   max_dist=float(world["cam"].far))
    seeds = r.batch_seeds()
    px, img = np.zeros(W * H, np.uint32), np.zeros((W * H, 4), F)
    for k, rec in enumerate(batches):
        def feed(b, kind, m, rec=rec):
            res = rec["vertices"][b][kind + "_results"]
            assert len(res) == m
            return res
        log = []
        radiance, stats = P.render_batch(impl, None, prim, pres, rec["first"], rec["count"], normals, material, SAMPLES,
                                         DEPTH, seeds[k], compact, scalars, feed=feed, log=log)
        assert stats == [v["live"] for v in rec["vertices"]], (k, stats)
        for (b, step, rad), v in zip(log, rec["vertices"]):
            m = v["m"]
            got = {"live": v["live"], "shadow": v["shadow"], "pending": v["pending"], "state": v["state"], "rays": v["rays"]}
            want = {"live": step["live"], "shadow": step["shadow"][:m], "pending": step["pending"][:m],
                    "state": step["state"][:m], "rays": None if step["rays"] is None else step["rays"][:m]}
            assert P.same_step(got, want) == "", (k, b)
            assert P.same_floats(v.get("radiance", v["radiance_after_extend"]), rad), (k, b)
        impl.path_resolve(SAMPLES, s2i, pres, radiance, W * H, first_primary=rec["first"], num_primary=rec["count"],
                          pixels=px, image=img)
    return px, img


@pytest.mark.parametrize("name", ["random1500", "bunny"])
def test_renderer_path_frames_equal_the_host_and_the_model_vertex_by_vertex(worlds, dev, name):
    world = world_of(worlds, name)
    v = world["v"]
    moved = (v + F(0.2) * np.sin(F(3.0) * v[:, ::-1])).astype(F)
    frames = []
    for compact in (True, False):
        r = path_renderer(world, MAX_BATCH, compact)
        for vertices in ((v, moved) if compact and name == "random1500" else (v,)):
            if vertices is moved:
                r.set_vertices(moved)
            px, img, batches = render_stepwise(r, world["cam"], dev)
            assert [b["count"] for b in batches] == [1100, 1100, 872]
            assert r.batch_seeds()[0] == mrt.AO_SEED and len(r.batch_seeds()) == 3
            for impl in (mrt.host, P.Model):
                want_px, want_img = replay(impl, r, world, vertices, batches, compact)
                assert np.array_equal(px, want_px), f"{int((px != want_px).sum())} pixels differ"
                assert P.same_floats(img, want_img)
            # trace_batch runs the same steps
            px2, img2, stats, sizes, ms = render(r, world["cam"], dev)
            assert np.array_equal(px, px2) and P.same_floats(img, img2) and ms > 0
            assert sizes == [1100 * SAMPLES, 1100 * SAMPLES, 872 * SAMPLES]
            assert stats == [[x["live"] for x in b["vertices"]] for b in batches]
            assert all(a >= b for s in stats for a, b in zip(s, s[1:]))   # a batch only thins out
            assert sum(s[0] for s in stats) > sum(s[-1] for s in stats if len(s) == DEPTH + 1) > 0   # and some paths reach the last vertex
            print(f"{name} compact={compact}: live counts per batch {stats}")
            assert len(np.unique(px)) > 100 and (px == L.BACKGROUND).sum() >= 50
            frames.append((compact, vertices is moved, px, img, stats))
    # compacted and in-place: the same bits
    (_, _, px_c, img_c, st_c), (_, _, px_i, img_i, st_i) = [f for f in frames if not f[1]]
    assert np.array_equal(px_c, px_i) and P.same_floats(img_c, img_i) and st_c == st_i
    if name == "random1500":
        assert not np.array_equal(frames[0][2], frames[1][2])   # the moved scene is another picture


@pytest.mark.parametrize("name", ["random1500", "bunny"])
def test_path_batches_trace_like_the_oracle(worlds, dev, name):
    """Bounce batches are closest-hit (t equal to the oracle's, the id equal or an exact-t tie the
    re-intersection confirms), shadow batches any-hit (hit or miss equal, every differing hit
    re-verified), in the production mode and per lane, at every vertex of a frame's single batch."""
    world = world_of(worlds, name)
    bufs = world["bvh"].buffers()
    r = path_renderer(world, 1 << 21, True, depth=2)
    r.begin_frame(world["cam"], W, H)
    assert r.next_batch()
    g = r._paths
    checked = {"shadow": 0, "bounce": 0, "blocked": 0, "bounce_hits": 0}
    for b in range(3):
        assert g.extend(b) > 0
        for kind, rb in (("shadow", g.shadow_batch()), ("bounce", g.bounce_batch())) if b < 2 else (("shadow", g.shadow_batch()),):
            assert rb.need_closest_hit == (kind == "bounce") and rb.size == g.live
            rays = rb.rays.cpu().numpy()
            want, _, _ = O.trace(rays, *bufs, any_hit=kind == "shadow", threads=8)
            for speculative in (True, False):
                r.tracer.trace_batch(rb, exact_rcp=True, speculative=speculative)
                assert r.tracer.last_info["stack_overflows"] == 0
                got = rb.results_numpy()
                assert np.array_equal(got[:, 0] != -1, want[:, 0] != -1), (kind, b, speculative)
                if kind == "bounce":
                    assert np.array_equal(got[:, 1], want[:, 1]), (kind, b, speculative)
                diff = np.nonzero((got[:, 0] != want[:, 0]) | (got[:, 1] != want[:, 1]))[0]
                assert len(O.invalid_hits(rays, got, bufs[1], bufs[2], which=diff)) == 0, (kind, b, speculative)
                if not speculative:
                    assert np.array_equal(got[:, :2], want[:, :2])   # the per-lane order is the oracle's
            checked[kind] += len(rays)
            checked["blocked" if kind == "shadow" else "bounce_hits"] += int((want[:, 0] != -1).sum())
        g.accumulate()
        if b < 2:
            g._cur = 1 - g._cur   # what trace_bounce does after its trace
    print(f"{name}: {checked}")
    # enough of each kind for the comparison to mean something (the bunny stand-in fills a third of a 64x48 frame)
    assert checked["shadow"] > 1000 and checked["bounce"] > 1000 and checked["blocked"] > 50 and checked["bounce_hits"] > 50, checked


# ---- C. the known answers, on the device ---------------------------------------------------------------------------
class Device:
    """mrt.host's three signatures over the device entry points, for test_path's known answers."""

    def __init__(self, dev):
        self.dev = dev

    def path_extend(self, rays, results, state, radiance, normals, material, **kw):
        return device_extend(self.dev, rays, results, state, radiance, normals, material, **kw)

    def path_accumulate(self, state, pending, shadow_results, radiance, num_slots=None):
        n = len(state) if num_slots is None else num_slots
        d = [upload(a, self.dev) for a in (state, pending, shadow_results, radiance)]
        _lib.check(_lib.trace_lib().mrt_path_accumulate(n, len(radiance), *(t.data_ptr() for t in d), None))
        radiance[...] = d[3].cpu().numpy()
        return radiance

    def path_resolve(self, num_samples, slot_to_id, primary_results, radiance, num_pixels, first_primary=0,
                     num_primary=None, pixels=None, image=None, want_image=False):
        if num_primary is None:
            num_primary = len(radiance) // num_samples
        d = [upload(a, self.dev) for a in (np.asarray(slot_to_id, np.int32), primary_results, radiance)]
        px = torch.zeros(num_pixels, dtype=torch.int32, device=self.dev)
        img = torch.zeros((num_pixels, 4), dtype=torch.float32, device=self.dev)
        _lib.check(_lib.trace_lib().mrt_path_resolve(num_samples, first_primary, num_primary, *(t.data_ptr() for t in d),
                                                     px.data_ptr(), img.data_ptr(), None))
        px = px.cpu().numpy().view(np.uint32)
        return (px, img.cpu().numpy()) if want_image else px


def test_known_answers_on_the_device(dev):
    impl = Device(dev)
    for depth in (1, 3):
        T.test_known_answer_floor_under_an_open_sky(impl, depth)
    T.test_known_answer_floor_and_occluder(impl)
    T.test_known_answer_closed_box_without_light(impl)


def test_depth_0_is_the_shadow_frame_on_the_device(worlds, dev):
    """Depth 0, sky 0, lightColor 1 through the Renderer: within 1 per channel of its RAY_SHADOW frame
    of the same seed, and built from the same shadow rays bit for bit."""
    from mrt.raygen import RAY_PATH, RAY_SHADOW
    from mrt.renderer import GlibcRand
    world = world_of(worlds, "random1500")
    r = path_renderer(world, 1 << 21, True)
    frames = {}
    for ray_type in (RAY_SHADOW, RAY_PATH):
        r.rand = GlibcRand()
        r.set_params(ray_type, 4, depth=0, light_pos=world["light"], light_radius=world["radius"], sky=(0.0, 0.0, 0.0), compact=True)
        r.begin_frame(world["cam"], W, H)
        assert r.next_batch()
        if ray_type == RAY_SHADOW:
            shadow_rays = r.batch.rays.cpu().numpy()
        r.trace_batch()
        frames[ray_type] = r.update_result().cpu().numpy().view(np.uint32)
        assert not r.next_batch()
    live = shadow_rays[:, 7] >= 0
    n = int(live.sum())
    assert r.path_stats == [n] and L.same_rays(r._paths.shadow_rays[:n].cpu().numpy(), shadow_rays[live])
    assert np.abs(T.channels(frames[RAY_PATH]) - T.channels(frames[RAY_SHADOW])).max() <= 1
    assert len(np.unique(frames[RAY_PATH])) > 50
