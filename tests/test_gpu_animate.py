"""Frames that follow moved vertices without the host: DeviceRayGen.set_geometry,
DeviceReconstructor.set_geometry and Renderer.set_vertices.

  * stream order: on one non-default stream, with no sync in between, Tracer.refit, both
    set_geometry calls, primary ray generation, trace, ao, trace and reconstruct give, value for
    value, the pixels of a Renderer made from scratch from a host Scene of the moved vertices and
    bound to a copy of the same refitted tree — primary and AO (4 samples) at 64x48. The device
    normals are bit-equal to the host's, so the AO rays are the same rays.
  * Renderer.set_vertices: there and back restores the original frame; rebuild_above=0.0 rebuilds
    and the frame is that of a fresh Renderer on Tracer.build of the moved vertices; 1e30 never
    rebuilds and reports a ratio >= 1 for a displaced scene; the default reads no cost."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mrt  # noqa: E402
from mrt.raygen import RAY_AO, RAY_PRIMARY, DeviceRayGen, DeviceReconstructor  # noqa: E402
from mrt.renderer import GlibcRand, Renderer  # noqa: E402
from mrt.tracer import GpuBvh, Tracer  # noqa: E402

F = np.float32
W, H, SAMPLES = 64, 48, 4


@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    scene = mrt.Scene.synthetic("random", 1500, 1)
    v, t, _ = scene.arrays()
    moved = (v + F(0.2) * np.sin(F(3.0) * v[:, ::-1])).astype(F)
    cam, ao_radius = scene.camera()
    return {"scene": scene, "bvh": mrt.Bvh.build_lbvh(scene), "v": v, "t": t, "moved": moved, "cam": cam,
            "ao_radius": ao_radius}


def bound_tracer(bufs):
    tracer = Tracer(0)
    tracer.set_bvh(GpuBvh(bufs), on_device=True)      # the refit plan is installed: a refit never waits
    return tracer


def render(r, cam, ray_type=RAY_PRIMARY, samples=1, radius=5.0):
    r.rand = GlibcRand()
    r.set_params(ray_type, samples, radius)
    r.begin_frame(cam, W, H)
    px = None
    while r.next_batch():
        r.trace_batch()
        px = r.update_result(px)
    torch.cuda.synchronize()
    return px.cpu().numpy()


@pytest.mark.parametrize("ray_type", [RAY_PRIMARY, RAY_AO])
def test_one_stream_no_sync_equals_a_renderer_made_from_scratch(world, ray_type):
    dev = torch.device("cuda", 0)
    tracer = bound_tracer(world["bvh"])
    gen, recon = DeviceRayGen(world["scene"]), DeviceReconstructor(world["scene"])
    v = torch.from_numpy(world["moved"]).to(dev)
    t = torch.from_numpy(world["t"]).to(dev)
    cam, radius = world["cam"], world["ao_radius"]
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):      # the tensors the calls allocate belong to s
        tracer.refit(v, t, stream=s)
        gen.set_geometry(v, t, stream=s)
        recon.set_geometry(v, t, stream=s)
        primary, slot_to_id = gen.primary(cam, W, H, stream=s)
        tracer.trace_async(primary, exact_rcp=True, stream=s)
        if ray_type == RAY_PRIMARY:
            px = recon.reconstruct(RAY_PRIMARY, primary, slot_to_id, W * H, stream=s)
        else:
            ao = gen.ao(primary, SAMPLES, radius, stream=s)
            tracer.trace_async(ao, exact_rcp=True, stream=s)
            px = recon.reconstruct(RAY_AO, primary, slot_to_id, W * H, ao, num_samples=SAMPLES, stream=s)
    s.synchronize()
    got = px.cpu().numpy()
    refitted = tuple(a.cpu().numpy().copy() for a in (tracer.bvh.nodes, tracer.bvh.woop, tracer.bvh.tri_index))

    scratch = Renderer(bound_tracer(refitted), mrt.Scene.from_arrays(world["moved"], world["t"]))
    want = render(scratch, cam, ray_type, SAMPLES if ray_type == RAY_AO else 1, radius)
    assert np.array_equal(got, want)
    hit = int((primary.hit_ids() >= 0).sum())
    assert 0 < hit < W * H                              # the frame shows triangles and background
    # and the moved scene is another picture than the one the tables were uploaded for
    still = render(Renderer(bound_tracer(world["bvh"]), world["scene"]), cam, ray_type,
                   SAMPLES if ray_type == RAY_AO else 1, radius)
    assert not np.array_equal(got, still)
    # the tables are the host's: normals bit for bit, colours exactly
    host = mrt.Scene.from_arrays(world["moved"], world["t"])
    assert gen.normals.cpu().numpy().tobytes() == host.arrays()[2].tobytes()
    mat, sh = host.tri_colors()
    assert np.array_equal(recon.shaded.cpu().numpy().view(np.uint32), sh)
    assert np.array_equal(recon.material.cpu().numpy().view(np.uint32), mat)


def test_set_vertices_there_and_back_restores_the_frame(world):
    r = Renderer(bound_tracer(world["bvh"]), world["scene"])
    first = render(r, world["cam"])
    out = r.set_vertices(world["moved"])
    assert out == {"rebuilt": False, "sah": None, "ratio": None}      # the default reads no cost
    assert out["ratio"] is None
    there = render(r, world["cam"])
    assert not np.array_equal(there, first)
    other = bound_tracer(world["bvh"])
    other.refit(world["moved"], world["t"])
    torch.cuda.synchronize()
    assert np.array_equal(there, render(Renderer(other, mrt.Scene.from_arrays(world["moved"], world["t"])), world["cam"]))
    r.set_vertices(torch.from_numpy(world["v"]).to("cuda:0"))
    assert np.array_equal(render(r, world["cam"]), first)
    # AO too: the normals went back
    ao_first = render(Renderer(bound_tracer(world["bvh"]), world["scene"]), world["cam"], RAY_AO, SAMPLES, world["ao_radius"])
    assert np.array_equal(render(r, world["cam"], RAY_AO, SAMPLES, world["ao_radius"]), ao_first)


def test_set_vertices_rebuild_above(world):
    r = Renderer(bound_tracer(world["bvh"]), world["scene"])
    out = r.set_vertices(world["moved"], rebuild_above=1e30)
    print("never:", out)
    assert out["rebuilt"] is False and out["ratio"] >= 1.0 and out["sah"] > 0
    bound = r.tracer.bvh
    out = r.set_vertices(world["moved"], rebuild_above=0.0)
    print("always:", out)
    assert out["rebuilt"] is True and out["ratio"] >= 1.0
    assert r.tracer.bvh is not bound and r._built is r.tracer.bvh
    got = render(r, world["cam"])
    fresh_tracer = Tracer(0)
    fresh_tracer.build(world["moved"], world["t"], on_device=True)
    want = render(Renderer(fresh_tracer, mrt.Scene.from_arrays(world["moved"], world["t"])), world["cam"])
    assert np.array_equal(got, want)
    # the rebuilt tree is the new baseline: the same vertices again give ratio 1
    out = r.set_vertices(world["moved"], rebuild_above=1e30)
    assert out["rebuilt"] is False and out["ratio"] == pytest.approx(1.0, rel=1e-9)
