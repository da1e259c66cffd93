"""The variance-guided filter on the device (csrc/svgf_kernel.hip) against its CPU statement
(csrc/host/svgf.cpp, which tests/test_svgf.py holds to the independent model):

  * mrt_svgf_accumulate and mrt_svgf_filter equal mrth_svgf_* bit for bit in every variant, over the
    host tests' tables and frames at, one under and one over both launch shapes' extents (32 x 8
    tiles; 64 columns by 4 rows a step apart at steps 1 .. 16, whose halo leaves the frame on every
    side; a frame narrower than one halo), with every combination of outputs;
  * mrt_svgf_accumulate's history, image and pixels equal mrt_temporal_accumulate's on the device;
  * every rejected argument returns its code and leaves sentinel-filled outputs untouched;
  * whole Renderer.svgf sequences of four frames of three batches on two scenes (a static camera, a
    panning one, a set_vertices between two frames): the host statements fed the device's own
    image, primary results and previous buffers give the same guide, history, moments, image and pixels;
  * a sequence that alternates Renderer.accumulate and Renderer.svgf restarts at every change and
    equals the host's replay of exactly that;
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
import svgf_util as SU  # noqa: E402
import test_gpu_path as G  # noqa: E402
import test_gpu_temporal as GT  # noqa: E402

F = np.float32
SENTINEL_F, SENTINEL_PX = GT.SENTINEL_F, GT.SENTINEL_PX
# 32 x 8 tiles: 31x7, 32x8, 33x9. Staged tiles of 64 columns by 4 rows a step s apart (4 s rows): 63x3,
# 64x4, 65x5 at step 1; 63x63, 64x64, 65x65 at step 16 (and 8 tiles of step 2, 4 of 4, 2 of 8); every
# one is narrower than 64 + 4 s, so the halo leaves the frame on both sides, above and below. 5x70 and
# 1x1 are narrower than one halo of step 4 and up; 97x83 has more than one tile in both directions.
FRAMES = [(1, 1), (31, 7), (32, 8), (33, 9), (63, 3), (64, 4), (65, 5), (5, 70), (63, 63), (64, 64), (65, 65), (97, 83)]
upload = GT.upload


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def full(dev, shape, value, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device=dev)


def read_only(d, kw):
    for k, t in d.items():
        assert np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(kw[k], F).view(np.uint32)), k


ACC_BUFFERS = GT.BUFFERS + ("prev_moments",)


def accumulate_params(d, kw, variant, history, moments, out, px):
    p = _lib.SvgfAccumulateParams()
    p.width, p.height, p.havePrev, p.maxHistory = kw["width"], kw["height"], int(kw["have_prev"]), kw["max_history"]
    p.normalCos, p.sigmaPlane, p.variant = float(F(kw["normal_cos"])), float(F(kw["sigma_plane"])), variant
    m = kw.get("prev_world_to_screen", np.zeros(16, F))
    for i in range(16):
        p.prevWorldToScreen[i] = float(m[i])
    sub = kw.get("prev_subpixel", (0.5, 0.5))
    p.prevSubpixel[0], p.prevSubpixel[1] = float(F(sub[0])), float(F(sub[1]))
    for field, key in (("image", "image"), ("guide", "guide"), ("albedo", "albedo"), ("prevPosition", "prev_position"),
                       ("prevGuide", "prev_guide"), ("prevHistory", "prev_history"), ("prevMoments", "prev_moments")):
        setattr(p, field, d[key].data_ptr() if key in d else None)
    p.history, p.moments = history.data_ptr(), moments.data_ptr()
    p.imageOut = None if out is None else out.data_ptr()
    p.pixels = None if px is None else px.data_ptr()
    return p


def device_accumulate(dev, kw, variant=0, want_image=True, want_pixels=True):
    """mrt_svgf_accumulate with mrt.host.svgf_accumulate's arguments and result."""
    n = kw["width"] * kw["height"]
    d = {k: upload(kw[k], dev) for k in ACC_BUFFERS if kw.get(k) is not None}
    history, moments = full(dev, (n, 4), SENTINEL_F), full(dev, (n, 4), SENTINEL_F)
    out = full(dev, (n, 4), SENTINEL_F) if want_image else None
    px = full(dev, (n,), SENTINEL_PX, torch.int32) if want_pixels else None
    p = accumulate_params(d, kw, variant, history, moments, out, px)
    _lib.check(_lib.trace_lib().mrt_svgf_accumulate(C.byref(p), None))
    torch.cuda.synchronize()
    read_only(d, kw)
    return (history.cpu().numpy(), moments.cpu().numpy(), None if out is None else out.cpu().numpy(),
            None if px is None else px.cpu().numpy().view(np.uint32))


FILTER_BUFFERS = ("image", "guide", "albedo", "moments")


def filter_params(d, kw, iterations, variant, scratch, out, px, var):
    p = _lib.SvgfFilterParams()
    p.width, p.height, p.iterations, p.normalSquarings = kw["width"], kw["height"], iterations, kw["normal_squarings"]
    p.sigmaLuminance, p.sigmaPlane, p.variant = float(F(kw["sigma_luminance"])), float(F(kw["sigma_plane"])), variant
    p.image, p.guide, p.albedo, p.moments = (d[k].data_ptr() for k in FILTER_BUFFERS)
    for i, t in enumerate(scratch):
        p.scratch[i] = None if t is None else t.data_ptr()
    p.imageOut = None if out is None else out.data_ptr()
    p.pixels = None if px is None else px.data_ptr()
    p.varianceOut = None if var is None else var.data_ptr()
    return p


def device_filter(dev, kw, iterations, variant=0, want_image=True, want_pixels=True, want_variance=True):
    """mrt_svgf_filter with mrt.host.svgf_filter's arguments and result; only the scratch buffers the
    iteration count needs exist."""
    n = kw["width"] * kw["height"]
    d = {k: upload(kw[k], dev) for k in FILTER_BUFFERS}
    scratch = [full(dev, (n, 4), SENTINEL_F) if iterations > i else None for i in range(2)]
    out = full(dev, (n, 4), SENTINEL_F) if want_image else None
    px = full(dev, (n,), SENTINEL_PX, torch.int32) if want_pixels else None
    var = full(dev, (n,), SENTINEL_F) if want_variance else None
    p = filter_params(d, kw, iterations, variant, scratch, out, px, var)
    _lib.check(_lib.trace_lib().mrt_svgf_filter(C.byref(p), None))
    torch.cuda.synchronize()
    read_only(d, kw)
    return (None if out is None else out.cpu().numpy(), None if px is None else px.cpu().numpy().view(np.uint32),
            None if var is None else var.cpu().numpy())


def same_result(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        if g is not None:
            assert SU.same_floats(g, w) if w.dtype == F else np.array_equal(g, w), (what, k)


# ---- 1. each entry point against its host statement --------------------------------------------------------
@pytest.mark.parametrize("frame", GT.FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_device_accumulate_equals_the_host_and_the_temporal_export_in_every_variant(dev, frame):
    w, h = frame
    outputs = [(True, False), (False, True), (False, False)]
    turn = 0
    for kind in SU.GUIDE_KINDS:
        for max_history, have_prev, moving in ((32, True, True), (2, True, False), (1, True, True), (32, False, False)):
            kw = SU.make_accumulate(w, h, kind, seed=w * 131 + h + max_history, max_history=max_history, have_prev=have_prev,
                                    moving=moving)
            want = mrt.host.svgf_accumulate(**kw)
            for variant in (0, 1, 2):
                got = device_accumulate(dev, kw, variant)
                same_result(got, want, (kind, max_history, have_prev, moving, variant))
                temporal = GT.device_accumulate(dev, {k: v for k, v in kw.items() if k != "prev_moments"}, variant)
                same_result((got[0], got[2], got[3]), temporal, (kind, max_history, "the temporal export", variant))
            want_image, want_pixels = outputs[turn % 3]
            got = device_accumulate(dev, kw, 1 + turn % 2, want_image, want_pixels)
            assert (got[2] is None) == (not want_image) and (got[3] is None) == (not want_pixels)
            same_result(got, want, (kind, max_history, have_prev, moving, "outputs", want_image, want_pixels))
            turn += 1


OUTPUTS = [(True, True, True), (True, True, False), (True, False, True), (True, False, False), (False, True, True), (False, True, False)]


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_device_filter_equals_the_host_in_every_variant(dev, frame):
    w, h = frame
    turn = 0
    for kind in SU.GUIDE_KINDS:
        for iterations in SU.ITERATIONS:
            if kind not in ("mixed", "hits") and iterations not in (0, 5):
                continue
            kw = SU.make_filter(w, h, kind, seed=w + 7 * h + iterations)
            want = mrt.host.svgf_filter(iterations=iterations, **kw)
            for variant in (0, 1, 2):
                same_result(device_filter(dev, kw, iterations, variant), want, (kind, iterations, variant))
            wants = OUTPUTS[turn % len(OUTPUTS)]
            got = device_filter(dev, kw, iterations, 1 + turn % 2, *wants)
            assert [g is not None for g in got] == list(wants)
            same_result(got, want, (kind, iterations, "outputs", wants))
            turn += 1


def test_device_filter_at_the_ends_of_sigma_luminance(dev):
    for sigma in (1e-30, 0.25, 1e25):
        kw = SU.make_filter(65, 9, "mixed", seed=4, sigma_luminance=sigma)
        want = mrt.host.svgf_filter(iterations=3, **kw)
        for variant in (1, 2):
            same_result(device_filter(dev, kw, 3, variant), want, (sigma, variant))


# ---- 2. rejections ---------------------------------------------------------------------------------------
def test_device_accumulate_refuses_bad_arguments_and_writes_nothing(dev):
    lib = _lib.trace_lib()
    bad, big = _lib.MRT_ERR_INVALID_ARG, _lib.MRT_ERR_TOO_LARGE
    w, h = 40, 9
    n = w * h
    kw = SU.make_accumulate(w, h, "hits", seed=1, moving=True)
    d = {k: upload(kw[k], dev) for k in ACC_BUFFERS}
    history, moments, out = (full(dev, (n + 1, 4), SENTINEL_F) for _ in range(3))
    px = full(dev, (n,), SENTINEL_PX, torch.int32)

    def rc(**over):
        p = accumulate_params(d, kw, 0, history, moments, out, px)
        for k, v in over.items():
            setattr(p, k, v)
        return lib.mrt_svgf_accumulate(C.byref(p), None)

    def untouched():
        torch.cuda.synchronize()
        return bool((history == SENTINEL_F).all() and (moments == SENTINEL_F).all() and (out == SENTINEL_F).all() and
                    (px == SENTINEL_PX).all())
    assert lib.mrt_svgf_accumulate(None, None) == bad
    ptr = {k: t.data_ptr() for k, t in d.items()}
    cases = [(dict(width=0), bad), (dict(height=0), bad), (dict(maxHistory=0), bad), (dict(sigmaPlane=0.0), bad),
             (dict(sigmaPlane=float("nan")), bad), (dict(normalCos=float("nan")), bad), (dict(variant=3), bad), (dict(variant=-1), bad),
             (dict(width=8193, height=8192), big), (dict(maxHistory=(1 << 20) + 1), big),
             (dict(maxHistory=(1 << 20) + 1, sigmaPlane=0.0), bad),   # shape before limits
             (dict(width=8193, height=8192, image=None), big),       # limits before pointers
             (dict(image=None), bad), (dict(guide=None), bad), (dict(albedo=None), bad), (dict(history=None), bad),
             (dict(moments=None), bad), (dict(prevGuide=None), bad), (dict(prevHistory=None), bad), (dict(prevMoments=None), bad),
             (dict(image=ptr["image"] + 4), bad), (dict(prevMoments=ptr["prev_moments"] + 4), bad),
             (dict(prevHistory=ptr["prev_history"] + 12), bad), (dict(history=history.data_ptr() + 4), bad),
             (dict(moments=moments.data_ptr() + 8), bad), (dict(imageOut=out.data_ptr() + 4), bad),
             # an output over an input, and two outputs over each other
             (dict(moments=ptr["prev_moments"]), bad), (dict(moments=ptr["prev_history"]), bad), (dict(history=ptr["prev_moments"]), bad),
             (dict(moments=ptr["image"]), bad), (dict(moments=ptr["prev_guide"] + 32 * (n - 1) + 16), bad),
             (dict(history=ptr["prev_history"]), bad), (dict(imageOut=ptr["prev_moments"] + 16 * (n - 1)), bad),
             (dict(pixels=ptr["prev_moments"]), bad), (dict(moments=history.data_ptr()), bad), (dict(imageOut=moments.data_ptr()), bad),
             (dict(pixels=moments.data_ptr() + 16 * (n - 1)), bad)]
    for over, code in cases:
        assert rc(**over) == code, over
        assert untouched(), over
    # without a previous frame its buffers are not checked; an adjacent output is no overlap
    assert rc(havePrev=0, prevGuide=None, prevHistory=None, prevMoments=ptr["image"], imageOut=None, pixels=None,
              moments=moments.data_ptr() + 16) == 0
    torch.cuda.synchronize()
    assert bool((moments[1:, 3] == 1).all() and (moments[0] == SENTINEL_F).all() and (history[:n, 3] == 1).all())
    assert bool((history[n] == SENTINEL_F).all() and (out == SENTINEL_F).all() and (px == SENTINEL_PX).all())
    assert rc(prevPosition=None) == 0
    torch.cuda.synchronize()
    assert (px != SENTINEL_PX).any()


def test_device_filter_refuses_bad_arguments_and_writes_nothing(dev):
    lib = _lib.trace_lib()
    bad, big = _lib.MRT_ERR_INVALID_ARG, _lib.MRT_ERR_TOO_LARGE
    w, h = 40, 9
    n = w * h
    kw = SU.make_filter(w, h, "hits", seed=2)
    d = {k: upload(kw[k], dev) for k in FILTER_BUFFERS}
    scratch = [full(dev, (n + 1, 4), SENTINEL_F) for _ in range(2)]
    out = full(dev, (n + 1, 4), SENTINEL_F)
    px, var = full(dev, (n,), SENTINEL_PX, torch.int32), full(dev, (n + 4,), SENTINEL_F)

    def rc(iterations=3, **over):
        p = filter_params(d, kw, iterations, 0, scratch, out, px, var)
        for k, v in over.items():
            if k.startswith("scratch"):
                p.scratch[int(k[-1])] = v
            else:
                setattr(p, k, v)
        return lib.mrt_svgf_filter(C.byref(p), None)

    def untouched():
        torch.cuda.synchronize()
        return bool(all((t == SENTINEL_F).all() for t in (*scratch, out, var)) and (px == SENTINEL_PX).all())
    assert lib.mrt_svgf_filter(None, None) == bad
    ptr = {k: t.data_ptr() for k, t in d.items()}
    s0, s1 = scratch[0].data_ptr(), scratch[1].data_ptr()
    cases = [(dict(width=0), bad), (dict(height=0), bad), (dict(iterations=-1), bad), (dict(normalSquarings=-1), bad),
             (dict(variant=3), bad), (dict(variant=-1), bad), (dict(sigmaLuminance=0.0), bad), (dict(sigmaLuminance=-4.0), bad),
             (dict(sigmaLuminance=float("nan")), bad), (dict(sigmaPlane=0.0), bad), (dict(sigmaPlane=float("nan")), bad),
             (dict(width=8193, height=8192), big), (dict(iterations=9), big), (dict(normalSquarings=11), big),
             (dict(iterations=9, sigmaLuminance=0.0), bad),     # shape before limits
             (dict(iterations=9, image=None), big),             # limits before pointers
             (dict(image=None), bad), (dict(guide=None), bad), (dict(albedo=None), bad), (dict(moments=None), bad),
             (dict(scratch0=None), bad), (dict(scratch1=None), bad), (dict(imageOut=None, pixels=None), bad),
             (dict(image=ptr["image"] + 4), bad), (dict(guide=ptr["guide"] + 8), bad), (dict(albedo=ptr["albedo"] + 4), bad),
             (dict(moments=ptr["moments"] + 4), bad), (dict(scratch0=s0 + 4), bad), (dict(scratch1=s1 + 8), bad),
             (dict(imageOut=out.data_ptr() + 4), bad),
             # an output or scratch buffer over an input, and over each other
             (dict(scratch0=ptr["image"]), bad), (dict(scratch1=ptr["moments"]), bad), (dict(imageOut=ptr["image"]), bad),
             (dict(imageOut=ptr["moments"] + 16 * (n - 1)), bad), (dict(pixels=ptr["guide"]), bad), (dict(varianceOut=ptr["moments"]), bad),
             (dict(varianceOut=ptr["albedo"] + 16 * n - 4), bad), (dict(scratch1=s0), bad), (dict(imageOut=s1), bad),
             (dict(varianceOut=s0 + 16 * (n - 1)), bad), (dict(pixels=out.data_ptr()), bad), (dict(varianceOut=out.data_ptr()), bad)]
    for over, code in cases:
        args = dict(over)
        assert rc(args.pop("iterations", 3), **args) == code, over
        assert untouched(), over
    # a scratch buffer that the iteration count does not need is not checked; an adjacent output is no overlap
    assert rc(1, scratch1=ptr["image"] + 4, imageOut=out.data_ptr() + 16, varianceOut=var.data_ptr() + 16, pixels=None) == 0
    torch.cuda.synchronize()
    assert bool((out[0] == SENTINEL_F).all() and (out[1:] != SENTINEL_F).any() and (var[:4] == SENTINEL_F).all() and
                (var[4:] != SENTINEL_F).all() and (scratch[1] == SENTINEL_F).all() and (scratch[0][n] == SENTINEL_F).all())
    assert rc(0, scratch0=None, scratch1=None, imageOut=None, varianceOut=None) == 0
    torch.cuda.synchronize()
    assert (px != SENTINEL_PX).any()


# ---- 3. whole sequences through Renderer.svgf ------------------------------------------------------------------------
def host_frame(r, world, vertices, previous_vertices, img, before, material, diagonal):
    """One frame by the host statements from the device's own image and primary results and the
    previous frame's device buffers (`before`, None where the history starts): guide, albedo,
    prevPosition and svgf_accumulate's four results."""
    from mrt.temporal import MAX_HISTORY_DEFAULT, NORMAL_COS_DEFAULT, SIGMA_PLANE_FRACTION_DEFAULT
    n = G.W * G.H
    prim, pres, s2i = r.primary.rays.cpu().numpy(), r.primary.results_numpy(), r.slot_to_id.cpu().numpy()
    normals = mrt.host.scene_attributes(vertices, world["t"], shaded=False, material=False)["normals"]
    guide, albedo = mrt.host.denoise_features(s2i, prim, pres, normals, material, n)
    pp = None
    if previous_vertices is not None:
        pp = mrt.host.temporal_motion(s2i, prim, pres, world["t"], vertices, previous_vertices, n)
    kw = dict(max_history=MAX_HISTORY_DEFAULT, normal_cos=NORMAL_COS_DEFAULT, sigma_plane=diagonal * SIGMA_PLANE_FRACTION_DEFAULT)
    if before is None:
        return guide, albedo, pp, kw, None
    return guide, albedo, pp, kw, dict(prev_guide=before["guide"], prev_history=before["history"],
                                       prev_world_to_screen=before["matrix"], prev_subpixel=before["subpixel"], prev_position=pp)


def snapshot(acc, with_moments):
    out = dict(guide=acc.current["guide"].cpu().numpy(), history=acc.current["history"].cpu().numpy(),
               matrix=acc._prev_matrix.copy(), subpixel=acc._prev_subpixel)
    if with_moments:
        out["moments"] = acc.current["moments"].cpu().numpy()
    return out


@pytest.mark.parametrize("sequence", ["static", "pan", "set_vertices"])
@pytest.mark.parametrize("name", ["random1500", "bunny"])
def test_renderer_svgf_equals_the_host_on_the_devices_own_frames(dev, name, sequence):
    from mrt.svgf import ITERATIONS_DEFAULT, NORMAL_SQUARINGS_DEFAULT, SIGMA_LUMINANCE_DEFAULT
    world = G.soup_world(name)
    v, n = world["v"], G.W * G.H
    moved = (v + F(0.05) * np.sin(F(3.0) * v[:, ::-1])).astype(F)
    diagonal = float(np.linalg.norm(v.astype(np.float64).max(axis=0) - v.astype(np.float64).min(axis=0)))
    material = world["scene"].tri_colors()[0]
    r = G.path_renderer(world, GT.MAX_BATCH, True, samples=GT.SAMPLES, depth=GT.DEPTH)
    with pytest.raises(_lib.MrtError):
        r.svgf(torch.zeros((n, 4), dtype=torch.float32, device=dev))      # before begin_frame
    vertices, found, short = v, [], []
    for k in range(GT.FRAMES_PER_SEQUENCE):
        previous_vertices = None
        if sequence == "set_vertices" and k == 2:
            r.set_vertices(moved)
            previous_vertices, vertices = v, moved
        cam = GT.panned(world["cam"], k) if sequence == "pan" else world["cam"]
        subpixel = (0.5, 0.5) if sequence != "pan" else (0.25 + 0.125 * k, 0.75 - 0.125 * k)
        d_img, batches = GT.render(r, cam, dev, subpixel)
        assert batches == 3
        before = snapshot(r._svgf, True) if k else None
        d_px, d_out, d_var = full(dev, (n,), SENTINEL_PX, torch.int32), full(dev, (n, 4), SENTINEL_F), full(dev, (n,), SENTINEL_F)
        got = r.svgf(d_img, pixels=d_px, image_out=d_out, variance_out=d_var)
        torch.cuda.synchronize()
        assert got[0] is d_px and got[1] is d_out
        img = d_img.cpu().numpy()
        guide, albedo, pp, kw, prev = host_frame(r, world, vertices, previous_vertices, img, before, material, diagonal)
        if prev is not None:
            prev["prev_moments"] = before["moments"]
        if pp is not None:
            assert SU.same_floats(r._svgf.prev_position.cpu().numpy(), pp) and (pp[:, 3] == 1).sum() > 500
        hst, mom, acc, _ = mrt.host.svgf_accumulate(img, guide, albedo, G.W, G.H, want_pixels=False, **(prev or {}), **kw)
        cur = r._svgf.current
        assert SU.same_floats(cur["guide"].cpu().numpy(), guide) and SU.same_floats(cur["albedo"].cpu().numpy(), albedo)
        assert SU.same_floats(cur["history"].cpu().numpy(), hst), (name, sequence, k, "history")
        assert SU.same_floats(cur["moments"].cpu().numpy(), mom), (name, sequence, k, "moments")
        assert SU.same_floats(r._svgf_image.cpu().numpy(), acc), (name, sequence, k, "accumulated image")
        want = mrt.host.svgf_filter(acc, guide, albedo, mom, G.W, G.H, iterations=ITERATIONS_DEFAULT,
                                    sigma_luminance=SIGMA_LUMINANCE_DEFAULT, sigma_plane=kw["sigma_plane"],
                                    normal_squarings=NORMAL_SQUARINGS_DEFAULT)
        same_result((d_out.cpu().numpy(), d_px.cpu().numpy().view(np.uint32), d_var.cpu().numpy()), want, (name, sequence, k))
        assert SU.same_floats(d_img.cpu().numpy(), img)                        # the input image is read only
        hit = guide[:, 3] != 0
        found.append(float((hst[hit, 3] > 1).mean()))
        short.append(float((mom[hit, 3] < 4).mean()))
        assert np.array_equal(want[0][~hit].view(np.uint32), img[~hit].view(np.uint32))     # the background is left alone
    print(f"{name} {sequence}: share of hits with history per frame {[round(x, 3) for x in found]}, with fewer than 4 frames {[round(x, 3) for x in short]}")
    assert found[0] == 0.0 and min(found[1:]) > (0.99 if sequence == "static" else 0.0)
    assert short[0] == 1.0 and (short[3] < 0.01 if sequence == "static" else True)   # both variance paths ran


def test_alternating_accumulate_and_svgf_restarts_the_history_at_every_change(dev):
    """accumulate, svgf, svgf, accumulate, accumulate, svgf over a static camera: a frame that follows
    one of the other kind finds no history (the other accumulator's buffers are not read, its own
    are from before that frame), one that follows its own kind finds it; every frame equals the
    host's replay of exactly that."""
    from mrt.svgf import SIGMA_LUMINANCE_DEFAULT
    world = G.soup_world("random1500")
    v, n = world["v"], G.W * G.H
    diagonal = float(np.linalg.norm(v.astype(np.float64).max(axis=0) - v.astype(np.float64).min(axis=0)))
    material = world["scene"].tri_colors()[0]
    r = G.path_renderer(world, GT.MAX_BATCH, True, samples=1, depth=1)
    kinds = ["accumulate", "svgf", "svgf", "accumulate", "accumulate", "svgf"]
    longest = []
    for k, kind in enumerate(kinds):
        if k == 4:
            r.set_vertices(v)          # the shared bookkeeping: the same vertices again, reprojected through
        d_img, _ = GT.render(r, world["cam"], dev)
        follows = k > 0 and kinds[k - 1] == kind
        acc = r._svgf if kind == "svgf" else r._temporal
        before = snapshot(acc, kind == "svgf") if follows else None
        d_out = full(dev, (n, 4), SENTINEL_F)
        getattr(r, kind)(d_img, image_out=d_out)
        torch.cuda.synchronize()
        img = d_img.cpu().numpy()
        guide, albedo, pp, kw, prev = host_frame(r, world, v, v if k == 4 else None, img, before, material, diagonal)
        assert (pp is None) == (k != 4)
        if kind == "svgf":
            if prev is not None:
                prev["prev_moments"] = before["moments"]
            hst, mom, image, _ = mrt.host.svgf_accumulate(img, guide, albedo, G.W, G.H, want_pixels=False, **(prev or {}), **kw)
            want = mrt.host.svgf_filter(image, guide, albedo, mom, G.W, G.H, sigma_luminance=SIGMA_LUMINANCE_DEFAULT,
                                        sigma_plane=kw["sigma_plane"], want_pixels=False, want_variance=False)[0]
            assert SU.same_floats(r._svgf.current["moments"].cpu().numpy(), mom), (k, kind)
        else:
            hst, want, _ = mrt.host.temporal_accumulate(img, guide, albedo, G.W, G.H, want_pixels=False, **(prev or {}), **kw)
        assert SU.same_floats((r._svgf if kind == "svgf" else r._temporal).current["history"].cpu().numpy(), hst), (k, kind)
        assert SU.same_floats(d_out.cpu().numpy(), want), (k, kind)
        longest.append(float(hst[:, 3].max()))
    assert longest == [1, 1, 2, 1, 2, 1]


def test_renderer_svgf_refuses_the_other_ray_types_and_unknown_settings(dev):
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
            r.svgf(image)
    assert r._svgf is None
    r = G.path_renderer(world, 1 << 21, True, samples=1, depth=1)
    d_img, _ = GT.render(r, world["cam"], dev)
    with pytest.raises(_lib.MrtError):
        r.svgf(d_img, sigma_color=1.0)
    assert r._svgf is None
