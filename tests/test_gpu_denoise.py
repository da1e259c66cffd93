"""The path frame's denoiser on the device (csrc/denoise_kernel.hip) against its CPU statement
(csrc/host/denoise.cpp, which tests/test_denoise.py holds to the independent model):

  * mrt_denoise_features and mrt_denoise_filter equal mrth_denoise_* bit for bit, the filter with
    the direct kernel, with the LDS-staged kernel wherever it fits and with the plan's own choice,
    over frames at, one under and one over both kernels' tile extents, frames wider and taller than
    a tile and its halos at the largest step, and every combination of outputs;
  * every rejected argument returns its code and leaves sentinel-filled outputs untouched;
  * whole Renderer.denoise frames of three batches on two scenes, and once more after set_vertices:
    the host statement fed the device's own image and primary results gives the same guide, albedo,
    image and pixels;
  * a frame that is not denoised is the frame of a renderer that never made a Denoiser;
  * the other ray types are refused.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mrt  # noqa: E402
import mrt.host  # noqa: E402
from mrt import _lib  # noqa: E402
import denoise_util as D  # noqa: E402
import test_gpu_path as G  # noqa: E402

F = np.float32
SENTINEL_F, SENTINEL_PX = 7.5, 77


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def upload(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)


def filter_params(d, w, h, iterations, sigma_color, sigma_plane, squarings, variant, out, px, scratch):
    p = _lib.DenoiseParams()
    p.width, p.height, p.iterations, p.normalSquarings = w, h, iterations, squarings
    p.sigmaColor, p.sigmaPlane, p.variant = float(F(sigma_color)), float(F(sigma_plane)), variant
    p.image, p.guide, p.albedo = d["image"].data_ptr(), d["guide"].data_ptr(), d["albedo"].data_ptr()
    p.scratch[0], p.scratch[1] = scratch[0].data_ptr(), scratch[1].data_ptr()
    p.imageOut = None if out is None else out.data_ptr()
    p.pixels = None if px is None else px.data_ptr()
    return p


def device_filter(dev, image, guide, albedo, w, h, iterations, sigma_color, sigma_plane, squarings, variant=0,
                  want_image=True, want_pixels=True):
    """mrt_denoise_filter with mrt.host.denoise_filter's arguments and result."""
    n = w * h
    d = {k: upload(v, dev) for k, v in dict(image=image, guide=guide, albedo=albedo).items()}
    out = torch.full((n, 4), SENTINEL_F, dtype=torch.float32, device=dev) if want_image else None
    px = torch.full((n,), SENTINEL_PX, dtype=torch.int32, device=dev) if want_pixels else None
    scratch = [torch.zeros((n, 4), dtype=torch.float32, device=dev) for _ in range(2)]
    p = filter_params(d, w, h, iterations, sigma_color, sigma_plane, squarings, variant, out, px, scratch)
    _lib.check(_lib.trace_lib().mrt_denoise_filter(C.byref(p), None))
    torch.cuda.synchronize()
    return (None if out is None else out.cpu().numpy()), (None if px is None else px.cpu().numpy().view(np.uint32))


# ---- 1. each entry point against its host statement --------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (255, 300), (256, 256), (257, 300), (5000, 5003)], ids=str)
def test_device_features_equal_the_host(dev, shape):
    slots, pixels = shape
    normals, material = D.feature_tables()
    s2i, rays, res = D.feature_inputs(slots, pixels, seed=slots)
    d = [upload(a, dev) for a in (s2i, rays, res, normals, material.view(np.int32))]
    guide = torch.full((pixels, 8), SENTINEL_F, dtype=torch.float32, device=dev)
    albedo = torch.full((pixels, 4), SENTINEL_F, dtype=torch.float32, device=dev)
    _lib.check(_lib.trace_lib().mrt_denoise_features(slots, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                                     d[4].data_ptr(), len(material), pixels, guide.data_ptr(),
                                                     albedo.data_ptr(), None))
    torch.cuda.synchronize()
    want = mrt.host.denoise_features(s2i, rays, res, normals, material, pixels, np.full((pixels, 8), SENTINEL_F, F),
                                     np.full((pixels, 4), SENTINEL_F, F))
    assert D.same_floats(guide.cpu().numpy(), want[0]) and D.same_floats(albedo.cpu().numpy(), want[1])


# The direct kernel's tile is 32 x 8 pixels, the staged one's 64 columns x 4 rows a step apart: each
# axis one under, at and one over both extents; and frames wider and taller than a staged tile and
# its two halos at the largest step (97 x 83 at 5 iterations: 64 + 4 * 16 columns; 300 x 270 at 8).
FILTER_CASES = [(1, 1, 5, "hits"), (1, 7, 5, "mixed"), (7, 1, 5, "mixed"),
                (31, 7, 5, "mixed"), (32, 8, 5, "checker"), (33, 9, 5, "mixed"),
                (63, 3, 5, "mixed"), (64, 4, 5, "hits"), (65, 5, 5, "mixed"),
                (97, 83, 5, "mixed"), (300, 270, 8, "mixed"), (97, 83, 0, "mixed"), (65, 9, 1, "zero-normals"),
                (64, 8, 2, "misses")]


@pytest.mark.parametrize("case", FILTER_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}-{c[3]}")
def test_device_filter_equals_the_host_in_every_variant(dev, case):
    w, h, iterations, kind = case
    image, guide, albedo = D.make_case(w, h, kind, seed=w * 131 + h)
    squarings = 7 if iterations != 1 else 0
    args = (image, guide, albedo, w, h, iterations, 0.7, 0.3, squarings)
    want_img, want_px = mrt.host.denoise_filter(*args)
    for variant in (0, 1, 2):
        got_img, got_px = device_filter(dev, *args, variant=variant)
        assert D.same_floats(got_img, want_img), f"variant {variant}: rows " \
            f"{np.flatnonzero(~D.U.same_bits_or_nan(got_img, want_img).all(axis=1))[:8]} differ"
        assert np.array_equal(got_px, want_px), variant
        only_px = device_filter(dev, *args, variant=variant, want_image=False)
        only_img = device_filter(dev, *args, variant=variant, want_pixels=False)
        assert np.array_equal(only_px[1], want_px) and D.same_floats(only_img[0], want_img), variant
    assert w * h < 11 or kind == "misses" or np.isnan(want_img).any() or iterations == 0


# ---- 2. rejections ---------------------------------------------------------------------------------------
def test_device_filter_refuses_bad_arguments_and_writes_nothing(dev):
    lib = _lib.trace_lib()
    bad, big = _lib.MRT_ERR_INVALID_ARG, _lib.MRT_ERR_TOO_LARGE
    w, h = 40, 9
    n = w * h
    image, guide, albedo = D.make_case(w, h, "hits", seed=1)
    d = {k: upload(v, dev) for k, v in dict(image=image, guide=guide, albedo=albedo).items()}
    out = torch.full((n + 1, 4), SENTINEL_F, dtype=torch.float32, device=dev)
    px = torch.full((n,), SENTINEL_PX, dtype=torch.int32, device=dev)
    scratch = [torch.full((n, 4), SENTINEL_F, dtype=torch.float32, device=dev) for _ in range(2)]

    def rc(**kw):
        p = filter_params(d, w, h, 5, 1.0, 1.0, 7, 0, out, px, scratch)
        for k, v in kw.items():
            if k.startswith("scratch"):
                p.scratch[int(k[-1])] = v
            else:
                setattr(p, k, v)
        return lib.mrt_denoise_filter(C.byref(p), None)

    def untouched():
        torch.cuda.synchronize()
        return bool((out == SENTINEL_F).all() and (px == SENTINEL_PX).all() and all((s == SENTINEL_F).all() for s in scratch))
    assert lib.mrt_denoise_filter(None, None) == bad
    cases = [(dict(width=0), bad), (dict(height=0), bad), (dict(width=-3), bad), (dict(iterations=-1), bad),
             (dict(normalSquarings=-1), bad), (dict(sigmaColor=0.0), bad), (dict(sigmaColor=float("nan")), bad),
             (dict(sigmaPlane=-1.0), bad), (dict(sigmaPlane=float("nan")), bad), (dict(variant=3), bad),
             (dict(width=8193, height=8192), big), (dict(iterations=9), big), (dict(normalSquarings=11), big),
             (dict(iterations=9, sigmaPlane=0.0), bad),   # shape before limits
             (dict(image=None), bad), (dict(guide=None), bad), (dict(albedo=None), bad), (dict(scratch0=None), bad),
             (dict(scratch1=None), bad), (dict(imageOut=None, pixels=None), bad),
             (dict(image=d["image"].data_ptr() + 4), bad), (dict(guide=d["guide"].data_ptr() + 8), bad),
             (dict(albedo=d["albedo"].data_ptr() + 4), bad), (dict(scratch0=scratch[0].data_ptr() + 4), bad),
             (dict(scratch1=scratch[1].data_ptr() + 12), bad), (dict(imageOut=out.data_ptr() + 4), bad),
             # an output or a scratch image over an input, and two of them over each other
             (dict(imageOut=d["image"].data_ptr()), bad), (dict(imageOut=d["image"].data_ptr() + 16 * (n - 1)), bad),
             (dict(pixels=d["guide"].data_ptr()), bad), (dict(scratch0=d["albedo"].data_ptr()), bad),
             (dict(scratch1=d["image"].data_ptr()), bad), (dict(scratch1=scratch[0].data_ptr()), bad),
             (dict(imageOut=scratch[0].data_ptr()), bad), (dict(pixels=out.data_ptr()), bad),
             (dict(pixels=scratch[1].data_ptr() + 16 * (n - 1)), bad)]
    for kw, code in cases:
        assert rc(**kw) == code, kw
        assert untouched(), kw
    # what an iteration count does not use is not checked; an adjacent output is no overlap
    assert rc(iterations=1, scratch0=None, scratch1=d["image"].data_ptr()) == 0
    assert rc(iterations=2, scratch1=None, imageOut=out.data_ptr() + 16) == 0
    torch.cuda.synchronize()
    assert (px != SENTINEL_PX).any()


def test_device_features_refuse_bad_arguments_and_write_nothing(dev):
    lib = _lib.trace_lib()
    bad, big = _lib.MRT_ERR_INVALID_ARG, _lib.MRT_ERR_TOO_LARGE
    normals, material = D.feature_tables()
    slots, pixels = 64, 80
    s2i, rays, res = D.feature_inputs(slots, pixels, seed=2)
    d = [upload(a, dev) for a in (s2i, rays, res, normals, material.view(np.int32))]
    guide = torch.full((pixels, 8), SENTINEL_F, dtype=torch.float32, device=dev)
    albedo = torch.full((pixels, 4), SENTINEL_F, dtype=torch.float32, device=dev)
    args = [slots, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), len(material), pixels,
            guide.data_ptr(), albedo.data_ptr(), None]
    cases = [((0, -1), bad), ((6, -1), bad), ((7, -1), bad), ((0, (1 << 26) + 1), big), ((7, (1 << 26) + 1), big)]
    cases += [((at, None), bad) for at in (1, 2, 3, 4, 5, 8, 9)]
    cases += [((2, args[2] + 4), bad), ((3, args[3] + 8), bad), ((8, args[8] + 4), bad), ((9, args[9] + 4), bad),
              ((8, args[2]), bad), ((9, args[3]), bad), ((8, args[4]), bad), ((9, args[8]), bad), ((8, args[9]), bad)]
    for (at, v), code in cases:
        call = list(args)
        call[at] = v
        assert lib.mrt_denoise_features(*call) == code, (at, v)
        torch.cuda.synchronize()
        assert bool((guide == SENTINEL_F).all() and (albedo == SENTINEL_F).all()), (at, v)
    for at in (0, 7):   # no slot, no pixel: fine, nothing launched
        call = list(args)
        call[at] = 0
        assert lib.mrt_denoise_features(*call) == 0
    torch.cuda.synchronize()
    assert bool((guide == SENTINEL_F).all())
    assert lib.mrt_denoise_features(*args) == 0
    torch.cuda.synchronize()
    assert bool((guide != SENTINEL_F).any())


# ---- 3. whole frames through Renderer.denoise -------------------------------------------------------------------------
def host_denoise(r, world, vertices, img, **settings):
    """The host statement over the device's own primary results and resolved image."""
    from mrt.denoise import SIGMA_PLANE_FRACTION_DEFAULT
    prim, pres, s2i = r.primary.rays.cpu().numpy(), r.primary.results_numpy(), r.slot_to_id.cpu().numpy()
    normals = mrt.host.scene_attributes(vertices, world["t"], shaded=False, material=False)["normals"]
    material = world["scene"].tri_colors()[0]
    guide, albedo = mrt.host.denoise_features(s2i, prim, pres, normals, material, G.W * G.H)
    v = world["v"].astype(np.float64)
    sigma_plane = float(np.linalg.norm(v.max(axis=0) - v.min(axis=0))) * SIGMA_PLANE_FRACTION_DEFAULT
    out, px = mrt.host.denoise_filter(img, guide, albedo, G.W, G.H, sigma_plane=sigma_plane, **settings)
    return guide, albedo, out, px


@pytest.mark.parametrize("name", ["random1500", "bunny"])
def test_renderer_denoise_equals_the_host_on_the_devices_own_frame(dev, name):
    from mrt.denoise import ITERATIONS_DEFAULT, NORMAL_SQUARINGS_DEFAULT, SIGMA_COLOR_DEFAULT
    world = G.soup_world(name)
    v = world["v"]
    moved = (v + F(0.2) * np.sin(F(3.0) * v[:, ::-1])).astype(F)
    r = G.path_renderer(world, G.MAX_BATCH, True)
    with pytest.raises(_lib.MrtError):
        r.denoise(torch.zeros((G.W * G.H, 4), dtype=torch.float32, device=dev))   # before begin_frame
    guides = []
    for vertices in (v, moved):
        if vertices is moved:
            r.set_vertices(moved)
        px, img, stats, sizes, _ = G.render(r, world["cam"], dev)
        assert len(sizes) == 3
        d_img = upload(img, dev)
        d_px = torch.full((G.W * G.H,), SENTINEL_PX, dtype=torch.int32, device=dev)
        d_out = torch.full((G.W * G.H, 4), SENTINEL_F, dtype=torch.float32, device=dev)
        got = r.denoise(d_img, pixels=d_px, image_out=d_out)
        torch.cuda.synchronize()
        assert got[0] is d_px and got[1] is d_out
        guide, albedo, out, want_px = host_denoise(r, world, vertices, img, iterations=ITERATIONS_DEFAULT,
                                                   sigma_color=SIGMA_COLOR_DEFAULT, normal_squarings=NORMAL_SQUARINGS_DEFAULT)
        assert D.same_floats(r._denoiser.guide.cpu().numpy(), guide) and D.same_floats(r._denoiser.albedo.cpu().numpy(), albedo)
        assert D.same_floats(d_out.cpu().numpy(), out)
        assert np.array_equal(d_px.cpu().numpy().view(np.uint32), want_px)
        assert D.same_floats(d_img.cpu().numpy(), img)                       # the input image is read only
        hit = guide[:, 3] != 0
        assert 500 < hit.sum() < G.W * G.H and (out[hit, :3] != img[hit, :3]).any()
        assert np.array_equal(out[~hit].view(np.uint32), img[~hit].view(np.uint32))   # the background is left alone
        # pixels alone, with other settings
        only_px, none = r.denoise(d_img, iterations=2, sigma_color=0.5, normal_squarings=3)
        torch.cuda.synchronize()
        _, _, _, want2 = host_denoise(r, world, vertices, img, iterations=2, sigma_color=0.5, normal_squarings=3)
        assert none is None and np.array_equal(only_px.cpu().numpy().view(np.uint32), want2)
        guides.append(guide)
    assert not np.array_equal(guides[0], guides[1])   # the moved scene guides the second frame


# ---- 4. no existing behaviour changes ---------------------------------------------------------------------------------
def test_a_frame_that_is_not_denoised_is_unchanged(dev):
    world = G.soup_world("random1500")
    plain = G.path_renderer(world, G.MAX_BATCH, True)
    want_px, want_img, want_stats, _, _ = G.render(plain, world["cam"], dev)
    assert plain._denoiser is None
    r = G.path_renderer(world, G.MAX_BATCH, True)
    px, img, stats, _, _ = G.render(r, world["cam"], dev)
    assert r._denoiser is None                      # rendering makes no denoiser
    assert np.array_equal(px, want_px) and D.same_floats(img, want_img) and stats == want_stats
    r.denoise(upload(img, dev))
    assert r._denoiser is not None
    px2, img2, stats2, _, _ = G.render(r, world["cam"], dev)   # and having one changes no later frame
    assert np.array_equal(px2, want_px) and D.same_floats(img2, want_img) and stats2 == want_stats


# ---- 5. wrong ray types ---------------------------------------------------------------------------------------------
def test_renderer_denoise_refuses_the_other_ray_types(dev):
    from mrt.raygen import RAY_AO, RAY_DIFFUSE, RAY_PRIMARY, RAY_SHADOW
    world = G.soup_world("random1500")
    r = G.path_renderer(world, 1 << 21, True)
    image = torch.zeros((G.W * G.H, 4), dtype=torch.float32, device=dev)
    for ray_type in (RAY_PRIMARY, RAY_AO, RAY_DIFFUSE, RAY_SHADOW):
        r.set_params(ray_type, 2, light_pos=world["light"], light_radius=world["radius"])
        r.begin_frame(world["cam"], G.W, G.H)
        assert r.next_batch()
        r.trace_batch()
        r.update_result()
        with pytest.raises(_lib.MrtError):
            r.denoise(image)
    assert r._denoiser is None
