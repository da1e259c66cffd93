"""The temporal accumulation on the device (csrc/temporal_kernel.hip) against its CPU statement
(csrc/host/temporal.cpp, which tests/test_temporal.py holds to the independent model):

  * mrt_temporal_motion and mrt_temporal_accumulate equal mrth_temporal_* bit for bit, the
    accumulation in both launch shapes and the plan's own choice, over the host tests' table and
    frames at, one under and one over both shapes' extents, with every combination of outputs, with
    and without prevPosition;
  * every rejected argument returns its code and leaves sentinel-filled outputs untouched;
  * whole Renderer.accumulate sequences of four frames of three batches on two scenes (a static
    camera, a panning one, a set_vertices between two frames), and once more with Renderer.denoise
    after each: the host statements fed the device's own image, primary results and previous
    buffers give the same guide, prevPosition, history, image and pixels;
  * a renderer that never accumulates renders the same bytes and keeps no vertex clone;
  * the other ray types are refused; reset=True and another frame size start over.
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
import temporal_util as TU  # noqa: E402
import test_gpu_path as G  # noqa: E402

F = np.float32
SENTINEL_F, SENTINEL_PX = 7.5, 77
FRAMES = [(1, 1), (31, 7), (32, 8), (33, 9), (63, 3), (64, 4), (65, 5), (97, 83)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def upload(a, dev):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)


def accumulate_params(d, kw, variant, history, out, px):
    p = _lib.TemporalParams()
    p.width, p.height, p.havePrev, p.maxHistory = kw["width"], kw["height"], int(kw["have_prev"]), kw["max_history"]
    p.normalCos, p.sigmaPlane, p.variant = float(F(kw["normal_cos"])), float(F(kw["sigma_plane"])), variant
    m = kw.get("prev_world_to_screen", np.zeros(16, F))
    for i in range(16):
        p.prevWorldToScreen[i] = float(m[i])
    sub = kw.get("prev_subpixel", (0.5, 0.5))
    p.prevSubpixel[0], p.prevSubpixel[1] = float(F(sub[0])), float(F(sub[1]))
    for field, key in (("image", "image"), ("guide", "guide"), ("albedo", "albedo"), ("prevPosition", "prev_position"),
                       ("prevGuide", "prev_guide"), ("prevHistory", "prev_history")):
        setattr(p, field, d[key].data_ptr() if key in d else None)
    p.history = history.data_ptr()
    p.imageOut = None if out is None else out.data_ptr()
    p.pixels = None if px is None else px.data_ptr()
    return p


BUFFERS = ("image", "guide", "albedo", "prev_position", "prev_guide", "prev_history")


def device_accumulate(dev, kw, variant=0, want_image=True, want_pixels=True):
    """mrt_temporal_accumulate with mrt.host.temporal_accumulate's arguments and result."""
    n = kw["width"] * kw["height"]
    d = {k: upload(kw[k], dev) for k in BUFFERS if kw.get(k) is not None}
    history = torch.full((n, 4), SENTINEL_F, dtype=torch.float32, device=dev)
    out = torch.full((n, 4), SENTINEL_F, dtype=torch.float32, device=dev) if want_image else None
    px = torch.full((n,), SENTINEL_PX, dtype=torch.int32, device=dev) if want_pixels else None
    p = accumulate_params(d, kw, variant, history, out, px)
    _lib.check(_lib.trace_lib().mrt_temporal_accumulate(C.byref(p), None))
    torch.cuda.synchronize()
    for k, t in d.items():
        assert np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(kw[k], F).view(np.uint32)), k   # read only
    return (history.cpu().numpy(), None if out is None else out.cpu().numpy(),
            None if px is None else px.cpu().numpy().view(np.uint32))


def same_result(got, want, what):
    assert TU.same_floats(got[0], want[0]), (what, "history")
    if got[1] is not None:
        assert TU.same_floats(got[1], want[1]), (what, "image")
    if got[2] is not None:
        assert np.array_equal(got[2], want[2]), (what, "pixels")


# ---- 1. each entry point against its host statement --------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_device_accumulate_equals_the_host_in_every_variant(dev, frame):
    w, h = frame
    outputs = [(True, False), (False, True), (False, False)]
    turn = 0
    for kind in TU.GUIDE_KINDS:
        for max_history, have_prev, moving in ((32, True, True), (2, True, False), (1, True, True), (32, False, False)):
            kw = TU.make_frame(w, h, kind, seed=w * 131 + h + max_history, max_history=max_history, have_prev=have_prev,
                               moving=moving)
            want = mrt.host.temporal_accumulate(**kw)
            for variant in (0, 1, 2):
                same_result(device_accumulate(dev, kw, variant), want, (kind, max_history, have_prev, moving, variant))
            want_image, want_pixels = outputs[turn % 3]
            got = device_accumulate(dev, kw, 1 + turn % 2, want_image, want_pixels)
            assert (got[1] is None) == (not want_image) and (got[2] is None) == (not want_pixels)
            same_result(got, want, (kind, max_history, have_prev, moving, "outputs", want_image, want_pixels))
            turn += 1


@pytest.mark.parametrize("shape", [(1, 3), (255, 300), (256, 300), (257, 300), (5000, 5003)], ids=str)
def test_device_motion_equals_the_host(dev, shape):
    slots, pixels = shape
    s2i, rays, res, tri, v, pv = TU.motion_inputs(slots, pixels, seed=slots)
    d = [upload(a, dev) for a in (s2i, rays, res, tri, v, pv)]
    pp = torch.full((pixels, 4), SENTINEL_F, dtype=torch.float32, device=dev)
    _lib.check(_lib.trace_lib().mrt_temporal_motion(slots, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                                    len(tri), d[4].data_ptr(), d[5].data_ptr(), len(v), pixels, pp.data_ptr(), None))
    torch.cuda.synchronize()
    want = mrt.host.temporal_motion(s2i, rays, res, tri, v, pv, pixels, np.full((pixels, 4), SENTINEL_F, F))
    got = pp.cpu().numpy()
    assert TU.same_floats(got, want)
    assert (got == SENTINEL_F).all(axis=1).sum() >= pixels - slots       # pixels no slot names are untouched


# ---- 2. rejections ---------------------------------------------------------------------------------------
def test_device_accumulate_refuses_bad_arguments_and_writes_nothing(dev):
    lib = _lib.trace_lib()
    bad, big = _lib.MRT_ERR_INVALID_ARG, _lib.MRT_ERR_TOO_LARGE
    w, h = 40, 9
    n = w * h
    kw = TU.make_frame(w, h, "hits", seed=1, moving=True)
    d = {k: upload(kw[k], dev) for k in BUFFERS}
    history = torch.full((n + 1, 4), SENTINEL_F, dtype=torch.float32, device=dev)
    out = torch.full((n + 1, 4), SENTINEL_F, dtype=torch.float32, device=dev)
    px = torch.full((n,), SENTINEL_PX, dtype=torch.int32, device=dev)

    def rc(**over):
        p = accumulate_params(d, kw, 0, history, out, px)
        for k, v in over.items():
            setattr(p, k, v)
        return lib.mrt_temporal_accumulate(C.byref(p), None)

    def untouched():
        torch.cuda.synchronize()
        return bool((history == SENTINEL_F).all() and (out == SENTINEL_F).all() and (px == SENTINEL_PX).all())
    assert lib.mrt_temporal_accumulate(None, None) == bad
    ptr = {k: t.data_ptr() for k, t in d.items()}
    cases = [(dict(width=0), bad), (dict(height=0), bad), (dict(width=-3), bad), (dict(maxHistory=0), bad),
             (dict(sigmaPlane=0.0), bad), (dict(sigmaPlane=-1.0), bad), (dict(sigmaPlane=float("nan")), bad),
             (dict(normalCos=float("nan")), bad), (dict(variant=3), bad), (dict(variant=-1), bad),
             (dict(width=8193, height=8192), big), (dict(maxHistory=(1 << 20) + 1), big),
             (dict(maxHistory=(1 << 20) + 1, sigmaPlane=0.0), bad),   # shape before limits
             (dict(image=None), bad), (dict(guide=None), bad), (dict(albedo=None), bad), (dict(history=None), bad),
             (dict(prevGuide=None), bad), (dict(prevHistory=None), bad),
             (dict(image=ptr["image"] + 4), bad), (dict(guide=ptr["guide"] + 8), bad), (dict(albedo=ptr["albedo"] + 4), bad),
             (dict(prevPosition=ptr["prev_position"] + 4), bad), (dict(prevGuide=ptr["prev_guide"] + 8), bad),
             (dict(prevHistory=ptr["prev_history"] + 12), bad), (dict(history=history.data_ptr() + 4), bad),
             (dict(imageOut=out.data_ptr() + 4), bad),
             # an output over an input, and two outputs over each other
             (dict(history=ptr["prev_history"]), bad), (dict(history=ptr["image"]), bad),
             (dict(history=ptr["prev_guide"] + 32 * (n - 1) + 16), bad), (dict(imageOut=ptr["image"]), bad),
             (dict(imageOut=ptr["prev_position"] + 16 * (n - 1)), bad), (dict(pixels=ptr["guide"]), bad),
             (dict(pixels=ptr["albedo"]), bad), (dict(imageOut=history.data_ptr()), bad), (dict(pixels=out.data_ptr()), bad),
             (dict(pixels=history.data_ptr() + 16 * (n - 1)), bad)]
    for over, code in cases:
        assert rc(**over) == code, over
        assert untouched(), over
    # without a previous frame its buffers are not checked; an adjacent output is no overlap
    assert rc(havePrev=0, prevGuide=None, prevHistory=ptr["image"], imageOut=None, pixels=None, history=history.data_ptr() + 16) == 0
    torch.cuda.synchronize()
    assert bool((history[1:, 3] == 1).all() and (history[0] == SENTINEL_F).all() and (out == SENTINEL_F).all())
    assert rc(prevPosition=None) == 0
    torch.cuda.synchronize()
    assert (px != SENTINEL_PX).any()


def test_device_motion_refuses_bad_arguments_and_writes_nothing(dev):
    lib = _lib.trace_lib()
    bad, big = _lib.MRT_ERR_INVALID_ARG, _lib.MRT_ERR_TOO_LARGE
    slots, pixels = 64, 80
    s2i, rays, res, tri, v, pv = TU.motion_inputs(slots, pixels, seed=2)
    d = [upload(a, dev) for a in (s2i, rays, res, tri, v, pv)]
    pp = torch.full((pixels, 4), SENTINEL_F, dtype=torch.float32, device=dev)
    args = [slots, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), len(tri), d[4].data_ptr(), d[5].data_ptr(),
            len(v), pixels, pp.data_ptr(), None]
    cases = [((0, -1), bad), ((5, -1), bad), ((8, -1), bad), ((9, -1), bad), ((0, (1 << 26) + 1), big), ((9, (1 << 26) + 1), big)]
    cases += [((at, None), bad) for at in (1, 2, 3, 4, 6, 7, 10)]
    cases += [((2, args[2] + 4), bad), ((3, args[3] + 8), bad), ((10, args[10] + 4), bad)]
    cases += [((10, args[at]), bad) for at in (1, 2, 3, 4, 6, 7)]
    for (at, value), code in cases:
        call = list(args)
        call[at] = value
        assert lib.mrt_temporal_motion(*call) == code, (at, value)
        torch.cuda.synchronize()
        assert bool((pp == SENTINEL_F).all()), (at, value)
    for at in (0, 9):   # no slot, no pixel: fine, nothing launched
        call = list(args)
        call[at] = 0
        assert lib.mrt_temporal_motion(*call) == 0
    torch.cuda.synchronize()
    assert bool((pp == SENTINEL_F).all())
    assert lib.mrt_temporal_motion(*args) == 0
    torch.cuda.synchronize()
    assert bool((pp != SENTINEL_F).any())


# ---- 3. whole sequences through Renderer.accumulate --------------------------------------------------------------------
SAMPLES, DEPTH, FRAMES_PER_SEQUENCE = 2, 2, 4
MAX_BATCH = SAMPLES * 1100      # 1100 primaries per batch: batches of 1100, 1100 and 872


def render(r, cam, dev, subpixel=(0.5, 0.5)):
    """One frame with the renderer's next seeds: (image tensor, batches)."""
    r.begin_frame(cam, G.W, G.H, subpixel=subpixel)
    px = torch.zeros(G.W * G.H, dtype=torch.int32, device=dev)
    img = torch.zeros((G.W * G.H, 4), dtype=torch.float32, device=dev)
    batches = 0
    while r.next_batch():
        r.trace_batch()
        r.update_result(px, img)
        batches += 1
    return img, batches


def panned(cam, k):
    if k == 0:
        return cam
    f = np.asarray(cam.forward, np.float64)
    side = np.cross(f, np.asarray(cam.up, np.float64))
    f = f + side * (0.02 * k)
    return mrt.host.Camera(cam.position, tuple(f / np.linalg.norm(f)), cam.up, cam.fov, cam.near, cam.far)


@pytest.mark.parametrize("denoise", [False, True], ids=["accumulate", "accumulate+denoise"])
@pytest.mark.parametrize("sequence", ["static", "pan", "set_vertices"])
@pytest.mark.parametrize("name", ["random1500", "bunny"])
def test_renderer_accumulate_equals_the_host_on_the_devices_own_frames(dev, name, sequence, denoise):
    from mrt.denoise import ITERATIONS_DEFAULT, NORMAL_SQUARINGS_DEFAULT, SIGMA_COLOR_DEFAULT
    from mrt.denoise import SIGMA_PLANE_FRACTION_DEFAULT as DENOISE_FRACTION
    from mrt.temporal import MAX_HISTORY_DEFAULT, NORMAL_COS_DEFAULT, SIGMA_PLANE_FRACTION_DEFAULT
    world = G.soup_world(name)
    v, n = world["v"], G.W * G.H
    moved = (v + F(0.05) * np.sin(F(3.0) * v[:, ::-1])).astype(F)
    diagonal = float(np.linalg.norm(v.astype(np.float64).max(axis=0) - v.astype(np.float64).min(axis=0)))
    material = world["scene"].tri_colors()[0]
    r = G.path_renderer(world, MAX_BATCH, True, samples=SAMPLES, depth=DEPTH)
    with pytest.raises(_lib.MrtError):
        r.accumulate(torch.zeros((n, 4), dtype=torch.float32, device=dev))      # before begin_frame
    vertices, found = v, []
    for k in range(FRAMES_PER_SEQUENCE):
        previous_vertices = None
        if sequence == "set_vertices" and k == 2:
            r.set_vertices(moved)
            previous_vertices, vertices = v, moved
        cam = panned(world["cam"], k) if sequence == "pan" else world["cam"]
        subpixel = (0.5, 0.5) if sequence != "pan" else (0.25 + 0.125 * k, 0.75 - 0.125 * k)
        d_img, batches = render(r, cam, dev, subpixel)
        assert batches == 3
        before = None
        if k:
            t = r._temporal
            before = dict(guide=t.current["guide"].cpu().numpy(), history=t.current["history"].cpu().numpy(),
                          matrix=t._prev_matrix.copy(), subpixel=t._prev_subpixel)
        d_px = torch.full((n,), SENTINEL_PX, dtype=torch.int32, device=dev)
        d_out = torch.full((n, 4), SENTINEL_F, dtype=torch.float32, device=dev)
        got = r.accumulate(d_img, pixels=d_px, image_out=d_out)
        torch.cuda.synchronize()
        assert got[0] is d_px and got[1] is d_out
        img = d_img.cpu().numpy()
        prim, pres, s2i = r.primary.rays.cpu().numpy(), r.primary.results_numpy(), r.slot_to_id.cpu().numpy()
        normals = mrt.host.scene_attributes(vertices, world["t"], shaded=False, material=False)["normals"]
        guide, albedo = mrt.host.denoise_features(s2i, prim, pres, normals, material, n)
        pp = None
        if previous_vertices is not None:
            pp = mrt.host.temporal_motion(s2i, prim, pres, world["t"], vertices, previous_vertices, n)
            assert TU.same_floats(r._temporal.prev_position.cpu().numpy(), pp)
            assert (pp[:, 3] == 1).sum() > 500
        kw = dict(max_history=MAX_HISTORY_DEFAULT, normal_cos=NORMAL_COS_DEFAULT, sigma_plane=diagonal * SIGMA_PLANE_FRACTION_DEFAULT)
        if before is None:
            want = mrt.host.temporal_accumulate(img, guide, albedo, G.W, G.H, **kw)
        else:
            want = mrt.host.temporal_accumulate(img, guide, albedo, G.W, G.H, before["guide"], before["history"], before["matrix"],
                                                before["subpixel"], pp, **kw)
        assert TU.same_floats(r._temporal.current["guide"].cpu().numpy(), guide)
        assert TU.same_floats(r._temporal.current["albedo"].cpu().numpy(), albedo)
        same_result((r._temporal.current["history"].cpu().numpy(), d_out.cpu().numpy(), d_px.cpu().numpy().view(np.uint32)), want,
                    (name, sequence, k))
        assert TU.same_floats(d_img.cpu().numpy(), img)                        # the input image is read only
        assert TU.same_floats(r._temporal.history_length().cpu().numpy(), want[0][:, 3])
        hit = guide[:, 3] != 0
        found.append(float((want[0][hit, 3] > 1).mean()))
        assert np.array_equal(want[1][~hit].view(np.uint32), img[~hit].view(np.uint32))     # the background is left alone
        if denoise:
            d_final = torch.full((n, 4), SENTINEL_F, dtype=torch.float32, device=dev)
            r.denoise(d_out, image_out=d_final)
            torch.cuda.synchronize()
            final, _ = mrt.host.denoise_filter(want[1], guide, albedo, G.W, G.H, iterations=ITERATIONS_DEFAULT,
                                               sigma_color=SIGMA_COLOR_DEFAULT, sigma_plane=diagonal * DENOISE_FRACTION,
                                               normal_squarings=NORMAL_SQUARINGS_DEFAULT, want_pixels=False)
            assert D.same_floats(d_final.cpu().numpy(), final)
    print(f"{name} {sequence}: share of hits with history per frame {[round(x, 3) for x in found]}")
    # a static camera brings every point back to its own pixel (within the 0.01 pixel of world_to_screen's
    # round trip), where the surface is its own: every hit finds its history. A pan and a moved soup find
    # what stays on one surface and in sight between two frames: some, not all (the shares are printed)
    assert found[0] == 0.0 and min(found[1:]) > (0.99 if sequence == "static" else 0.0)
    if sequence == "set_vertices":
        assert min(found[1], found[3]) > 0.99         # the frames without a motion between them are static ones


# ---- 4. no existing behaviour changes ---------------------------------------------------------------------------------
def test_a_renderer_that_never_accumulates_is_unchanged_and_keeps_no_clone(dev):
    world = G.soup_world("random1500")
    v = world["v"]
    moved = (v + F(0.05) * np.sin(F(3.0) * v[:, ::-1])).astype(F)
    plain = G.path_renderer(world, G.MAX_BATCH, True)
    plain.set_vertices(moved)
    want_px, want_img, want_stats, _, _ = G.render(plain, world["cam"], dev)
    assert plain._temporal is None and plain._vertices is None and plain._motion_from is None
    r = G.path_renderer(world, G.MAX_BATCH, True)
    img0 = G.render(r, world["cam"], dev)[1]
    r.accumulate(upload(img0, dev))
    assert r._temporal is not None
    r.set_vertices(moved)                                   # from now on the vertices are kept
    assert r._vertices is not None and r._motion_from is not None
    assert np.array_equal(r._motion_from.cpu().numpy(), v) and np.array_equal(r._vertices.cpu().numpy(), moved)
    px, img, stats, _, _ = G.render(r, world["cam"], dev)   # and accumulating changes no later frame
    assert np.array_equal(px, want_px) and D.same_floats(img, want_img) and stats == want_stats


# ---- 5. wrong ray types, starting over ---------------------------------------------------------------------------------
def test_renderer_accumulate_refuses_the_other_ray_types(dev):
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
            r.accumulate(image)
    assert r._temporal is None


def test_reset_and_another_frame_size_start_over(dev):
    world = G.soup_world("random1500")
    r = G.path_renderer(world, 1 << 21, True, samples=1, depth=1)

    def frame(w, h, **kw):
        r.begin_frame(world["cam"], w, h)
        px = torch.zeros(w * h, dtype=torch.int32, device=dev)
        img = torch.zeros((w * h, 4), dtype=torch.float32, device=dev)
        while r.next_batch():
            r.trace_batch()
            r.update_result(px, img)
        r.accumulate(img, **kw)
        torch.cuda.synchronize()
        return r._temporal.history_length().cpu().numpy()
    assert frame(G.W, G.H).max() == 1
    assert frame(G.W, G.H).max() == 2
    assert frame(G.W, G.H, max_history=2).max() == 2 and frame(G.W, G.H).max() == 3
    assert frame(G.W, G.H, reset=True).max() == 1
    assert frame(G.W, G.H).max() == 2
    assert frame(32, 24).max() == 1 and frame(32, 24).max() == 2
    assert frame(G.W, G.H).max() == 1
