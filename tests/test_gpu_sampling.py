"""The checks of tests/test_sampling.py on the device: mrt_raygen_shadow, mrt_path_extend and
mrt_raygen_ao against the float64 restatements with their per-sample bounds, the distributions of
what they sample, and Renderer frames (RAY_PATH, float image) against their closed-form expectation.
The largest launch is 65 536 slots, the largest frame 96 x 72 x 8 paths at depth 2 on 6 triangles.
The path and light kernels give the host's bits, so their worst error-to-bound ratios must EQUAL the
host's; the AO generator's cosf / sinf are the device's own and its ratio is its own."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mrt  # noqa: E402
import mrt.host  # noqa: E402
import test_gpu_path as G  # noqa: E402
import test_path as TP  # noqa: E402
import test_sampling as T  # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def impl():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda", 0)

    def buffer_of(rays, res):
        from mrt.tracer import RayBuffer
        rb = RayBuffer(np.array(rays, F))   # a copy: the tables are read-only
        rb.results.copy_(G.upload(res, dev))
        return rb

    class Device:
        name = "device"

        @staticmethod
        def shadow(rays, res, S, light, radius, seed):
            from mrt.raygen import DeviceRayGen
            return DeviceRayGen().shadow(buffer_of(rays, res), S, light, radius, seed=seed).rays.cpu().numpy()

        @staticmethod
        def extend(rays, results, state, radiance, normals, material, **kw):
            return G.device_extend(dev, rays, results, state, radiance, normals, material, **kw)

        @staticmethod
        def ao(rays, res, scene, S, max_dist, seed):
            from mrt.raygen import DeviceRayGen
            return DeviceRayGen(scene).ao(buffer_of(rays, res), S, max_dist, seed=seed).rays.cpu().numpy()

    Device.dev = dev
    return Device


# ---- A and B: each sample against float64, and the distributions ----------------------------------------
@pytest.mark.parametrize("which", list(T.SEEDS))
def test_light_sampler_on_the_device(impl, which):
    assert T.check_light_sampler(impl, which) == T.check_light_sampler(T.Host, which)


@pytest.mark.parametrize("which", list(T.SEEDS))
@pytest.mark.parametrize("vertex", [0, 1, T.DEPTH])
def test_vertex_step_on_the_device(impl, vertex, which):
    got, want = T.check_vertex_step(impl, vertex, which), T.check_vertex_step(T.Host, vertex, which)
    assert got == want   # the same bits: the same ratios and the same statistics


def test_bounces_are_independent_on_the_device(impl):
    T.check_independence(impl)


@pytest.mark.parametrize("S,a,b", [(6, 1, 1), (36, 2, 2)])
def test_a_pixels_paths_fall_one_per_cell_on_the_device(impl, S, a, b):
    T.check_strata(impl, S, a, b)


def test_sobol_pair_on_the_device(impl):
    found = T.check_sobol_pair(impl)
    assert all(counts == [1] for per_j in found.values() for counts in per_j)


@pytest.mark.parametrize("seed", [1, 0xFFFFFFF0])
def test_ao_rays_on_the_device(impl, seed):
    T.check_ao(impl, seed)


def test_ao_hash_angle_on_the_device(impl):
    T.check_ao_hash_angle(impl)


# ---- C. frames with a closed-form expectation, through the Renderer --------------------------------------
def device_frame(dev, name):
    from mrt.raygen import RAY_PATH, RAY_SHADOW
    from mrt.renderer import GlibcRand, Renderer
    from mrt.tracer import GpuBvh, Tracer
    f = T.FRAMES[name]
    scene, bufs, _, material = TP.world_of(f["tris"])
    assert (material == 0xFFBFBFBF).all()
    tracer = Tracer(0)
    tracer.set_bvh(GpuBvh(bufs), on_device=True)
    r = Renderer(tracer, scene, max_batch=1 << 21, rand=GlibcRand())
    cam = mrt.host.Camera(*T.CAMERA)
    s = f["scalars"]
    frames = {}
    for ray_type in (RAY_PATH, RAY_SHADOW) if name == "penumbra" else (RAY_PATH,):
        r.rand = GlibcRand()
        r.set_params(ray_type, T.SAMPLES, depth=f["depth"], light_pos=s["light_pos"], light_radius=s["light_radius"],
                     light_color=s["light_color"], sky=s["sky"], compact=True)
        r.begin_frame(cam, T.W, T.H)
        px = torch.zeros(T.W * T.H, dtype=torch.int32, device=dev)
        img = torch.zeros((T.W * T.H, 4), dtype=torch.float32, device=dev)
        batches = 0
        while r.next_batch():
            r.trace_batch()
            r.update_result(px, img)
            batches += 1
        torch.cuda.synchronize()
        assert batches == 1 and r.batch_seeds()[0] == mrt.AO_SEED
        frames[ray_type] = (px.cpu().numpy().view(np.uint32), img.cpu().numpy())
    prim, pres, s2i = r.primary.rays.cpu().numpy(), r.primary.results_numpy(), r.slot_to_id.cpu().numpy()
    px, image = frames[RAY_PATH]
    return prim, pres, s2i, px, image, frames[RAY_SHADOW][0] if name == "penumbra" else None


@pytest.mark.parametrize("name", list(T.FRAMES))
def test_frame_mean_against_its_closed_form_on_the_device(impl, name):
    T.check_frame(name, *device_frame(impl.dev, name), "device")
