"""Stream order of the variance-guided filter (DESIGN sections 17 and 21): every stream-taking export
of include/mrt_svgf.h and every public callable of mrt.svgf, with Renderer.svgf, under the
stalled-stream protocol of tests/stream_util.py, as tests/test_gpu_temporal_stream.py holds the
temporal accumulation to it. The exports take the stream as an argument; the Python callables take
none and run on torch's current stream, so a wrapper's call enters `with torch.cuda.stream(s)`
itself. tests/test_svgf_table.py checks without a device that the two tables are complete and that
every decoy is valid input with another result.
"""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mrt  # noqa: E402
import mrt.host  # noqa: E402
from mrt import _lib  # noqa: E402
from mrt.svgf import SIGMA_LUMINANCE_DEFAULT  # noqa: E402
import denoise_util as D  # noqa: E402
import stream_util as S  # noqa: E402
import svgf_util as SU  # noqa: E402
import test_gpu_temporal_stream as TS  # noqa: E402

F, U32 = np.float32, np.uint32
p, sp, on = TS.p, TS.sp, TS.on

RAW = []        # (export, label, builder of a stream_util.Case)
WRAPPERS = []   # (qualified name of the callable, label, builder)


def raw(export, label="", **kw):
    def deco(fn):
        RAW.append((export, label, functools.partial(fn, **kw)))
        return fn
    return deco


def wrapper(name, label="", **kw):
    def deco(fn):
        WRAPPERS.append((name, label, functools.partial(fn, wrapper=name, **kw)))
        return fn
    return deco


def lib():
    return _lib.trace_lib()


# ---- the raw exports ---------------------------------------------------------------------------------------------------
FRAME = (65, 9)   # one column more than two 32-pixel tiles and than one 64-column tile, one row more than one 32 x 8 tile
ACC_BUFFERS = TS.BUFFERS + ("prev_moments",)


@raw("mrt_svgf_accumulate", label="linear", variant=1)
@raw("mrt_svgf_accumulate", label="tiled", variant=2)
def case_accumulate(variant):
    w, h = FRAME
    n = w * h
    frames = [SU.make_accumulate(w, h, "checker", seed=seed, moving=True) for seed in (66, 67)]
    real, decoy = ({k: kw[k] for k in ACC_BUFFERS} for kw in frames)
    scalars = frames[0]
    assert np.array_equal(scalars["prev_world_to_screen"], frames[1]["prev_world_to_screen"])

    def call(b, s, ctx):
        q = _lib.SvgfAccumulateParams()
        q.width, q.height, q.havePrev, q.maxHistory, q.variant = w, h, 1, scalars["max_history"], variant
        q.normalCos, q.sigmaPlane = float(F(scalars["normal_cos"])), float(F(scalars["sigma_plane"]))
        for i in range(16):
            q.prevWorldToScreen[i] = float(scalars["prev_world_to_screen"][i])
        q.prevSubpixel[0], q.prevSubpixel[1] = (float(F(x)) for x in scalars["prev_subpixel"])
        q.image, q.guide, q.albedo = p(b["image"]), p(b["guide"]), p(b["albedo"])
        q.prevPosition, q.prevGuide, q.prevHistory = p(b["prev_position"]), p(b["prev_guide"]), p(b["prev_history"])
        q.prevMoments = p(b["prev_moments"])
        q.history, q.moments, q.imageOut, q.pixels = p(b["history"]), p(b["moments"]), p(b["out"]), p(b["pixels"])
        _lib.check(lib().mrt_svgf_accumulate(C.byref(q), sp(s)))

    def twin(x):
        hst, mom, out, px = mrt.host.svgf_accumulate(**dict(scalars, **x))
        assert (mom[:, 3] > 1).sum() > n // 10
        return {"history": hst, "moments": mom, "out": out, "pixels": px}
    outs = {"history": ((n, 4), F), "moments": ((n, 4), F), "out": ((n, 4), F), "pixels": ((n,), U32)}
    return S.Case(f"svgf_accumulate variant {variant}", real, decoy, outs, call, twin)


FILTER_BUFFERS = ("image", "guide", "albedo", "moments")
ITERATIONS = 3    # steps 1, 2 and 4: both scratch buffers, and three staged tile geometries


@raw("mrt_svgf_filter", label="direct", variant=1)
@raw("mrt_svgf_filter", label="staged", variant=2)
def case_filter(variant):
    w, h = FRAME
    n = w * h
    frames = [SU.make_filter(w, h, "checker", seed=seed) for seed in (68, 69)]
    real, decoy = ({k: kw[k] for k in FILTER_BUFFERS} for kw in frames)
    scalars = frames[0]

    def call(b, s, ctx):
        q = _lib.SvgfFilterParams()
        q.width, q.height, q.iterations, q.normalSquarings, q.variant = w, h, ITERATIONS, scalars["normal_squarings"], variant
        q.sigmaLuminance, q.sigmaPlane = float(F(scalars["sigma_luminance"])), float(F(scalars["sigma_plane"]))
        q.image, q.guide, q.albedo, q.moments = (p(b[k]) for k in FILTER_BUFFERS)
        q.scratch[0], q.scratch[1] = p(b["scratch0"]), p(b["scratch1"])
        q.imageOut, q.pixels, q.varianceOut = p(b["out"]), p(b["pixels"]), p(b["variance"])
        _lib.check(lib().mrt_svgf_filter(C.byref(q), sp(s)))

    def twin(x):
        out, px, var = mrt.host.svgf_filter(iterations=ITERATIONS, **dict(scalars, **x))
        return {"out": out, "pixels": px, "variance": var}
    # the scratch images are watched like outputs (nothing may reach them early) and compared with nothing
    outs = {"scratch0": ((n, 4), F), "scratch1": ((n, 4), F), "out": ((n, 4), F), "pixels": ((n,), U32), "variance": ((n,), F)}
    return S.Case(f"svgf_filter variant {variant}", real, decoy, outs, call, twin)


# ---- the Python callables -------------------------------------------------------------------------------------------------
SIGMA_PLANE, NORMAL_COS, SUBPIXELS = TS.SIGMA_PLANE, TS.NORMAL_COS, TS.SUBPIXELS


def host_frames(frames, normals, material, matrices):
    """The host statements over a list of frames (dicts of TS.wrapper_inputs): the last frame's
    guide, history, moments, filtered pixels and variance."""
    w, h = TS.MOTION_FRAME
    n = w * h
    guide = hst = mom = acc = None
    for k, x in enumerate(frames):
        prev_guide, prev_hst, prev_mom = guide, hst, mom
        guide, albedo = mrt.host.denoise_features(x["s2i"], x["rays"], x["results"], normals, material, n,
                                                  np.zeros((n, 8), F), np.ones((n, 4), F))
        hst, mom, acc, _ = mrt.host.svgf_accumulate(x["image"], guide, albedo, w, h, prev_guide, prev_hst, prev_mom,
                                                    matrices[k - 1] if k else None, SUBPIXELS[k - 1] if k else (0.5, 0.5),
                                                    sigma_plane=SIGMA_PLANE, normal_cos=NORMAL_COS, want_pixels=False)
    _, px, var = mrt.host.svgf_filter(acc, guide, albedo, mom, w, h, sigma_luminance=SIGMA_LUMINANCE_DEFAULT, sigma_plane=SIGMA_PLANE,
                                      want_image=False)
    return {"guide": guide, "history": hst, "moments": mom, "pixels": px, "variance": var}


@wrapper("SvgfAccumulator.filter")
@wrapper("Renderer.svgf", renderer=True)
def case_wrapper(wrapper=None, renderer=False):
    """Frame 0 is accumulated in prepare, from inputs of its own; the gated call accumulates and
    filters frame 1 under `with torch.cuda.stream(s)` and nothing else."""
    from mrt.temporal import world_to_screen
    normals, material = D.feature_tables()
    w, h = TS.MOTION_FRAME
    n = w * h
    (first, _), (real, _), (decoy, _) = (TS.wrapper_inputs(seed) for seed in (3, 1, 2))
    for d in (first, real, decoy):
        d.pop("vertices"), d.pop("prev_vertices")
    cams = TS.cameras()
    matrices = [world_to_screen(c, w, h) for c in cams]

    def prepare(dev, b):
        from mrt.raygen import RAY_PATH, DeviceReconstructor
        from mrt.renderer import Renderer
        from mrt.svgf import SvgfAccumulator
        from mrt.tracer import RayBuffer, Tracer
        import frame_util as U
        ctx = {"normals": S._upload(normals, dev), "material": S._upload(material, dev)}
        f = {k: S._upload(v, dev) for k, v in first.items()}
        ctx["first"] = f
        primary0, primary1 = RayBuffer(f["rays"], results=f["results"]), RayBuffer(b["rays"], results=b["results"])
        if renderer:
            v, t, _ = U.edge_scene()
            r = Renderer(Tracer(0), mrt.Scene.from_arrays(v, t))
            r.set_params(RAY_PATH, 1)
            r._recon = DeviceReconstructor(None)
            r._recon.material, r.gen.normals = ctx["material"], ctx["normals"]
            r.primary, r.slot_to_id, r.w, r.h, r.cam, r._subpixel = primary0, f["s2i"], w, h, cams[0], SUBPIXELS[0]
            r.svgf(f["image"], sigma_plane=SIGMA_PLANE, normal_cos=NORMAL_COS)
            r.primary, r.slot_to_id, r.cam, r._subpixel = primary1, b["s2i"], cams[1], SUBPIXELS[1]
            ctx["renderer"] = r
        else:
            acc = SvgfAccumulator(dev)
            ctx["accumulated"] = torch.empty((n, 4), dtype=torch.float32, device=dev)
            acc.accumulate(primary0, f["s2i"], ctx["normals"], ctx["material"], w, h, matrices[0], SUBPIXELS[0], f["image"],
                           image_out=ctx["accumulated"], sigma_plane=SIGMA_PLANE, normal_cos=NORMAL_COS)
            acc.filter(ctx["accumulated"], sigma_plane=SIGMA_PLANE)      # the scratch images exist before the stall
            ctx["acc"], ctx["primary"] = acc, primary1
        return ctx

    def call(b, s, ctx):
        with on(s):
            if renderer:
                r = ctx["renderer"]
                px, _ = r.svgf(b["image"], sigma_plane=SIGMA_PLANE, normal_cos=NORMAL_COS, variance_out=b["variance"])
                acc = r._svgf
            else:
                acc = ctx["acc"]
                acc.accumulate(ctx["primary"], b["s2i"], ctx["normals"], ctx["material"], w, h, matrices[1], SUBPIXELS[1], b["image"],
                               image_out=ctx["accumulated"], sigma_plane=SIGMA_PLANE, normal_cos=NORMAL_COS)
                px, _ = acc.filter(ctx["accumulated"], variance_out=b["variance"], sigma_plane=SIGMA_PLANE)
            return {"pixels": px, "guide": acc.current["guide"], "history": acc.current["history"], "moments": acc.current["moments"]}

    def twin(x):
        out = host_frames([first, x], normals, material, matrices)
        found = int((out["moments"][:, 3] > 1).sum())
        print(f"{wrapper}: {found} pixels found history")
        assert found > 10, "the case reprojects nothing"
        return out
    return S.Case(f"{wrapper}", real, decoy, {"variance": ((n,), F)}, call, twin, prepare=prepare)


# ---- the tests ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    S.calibrate(device)
    return device


@pytest.fixture(scope="module")
def streams(dev):
    """The stalled stream and the snapshot stream: neither is torch's current stream."""
    return torch.cuda.Stream(dev), torch.cuda.Stream(dev)


def ids(table):
    return [f"{name}-{label}".rstrip("-").replace(" ", "_") for name, label, _ in table]


@pytest.mark.parametrize("export,label,build", RAW, ids=ids(RAW))
def test_raw_export_keeps_stream_order_behind_a_stalled_stream(dev, streams, export, label, build):
    S.run(build(), dev, streams)


@pytest.mark.parametrize("method,label,build", WRAPPERS, ids=ids(WRAPPERS))
def test_the_current_stream_alone_orders_the_callable(dev, streams, method, label, build):
    """Called under `with torch.cuda.stream(s)` while torch's current stream outside is the default
    one: the launches and what the callable allocates and fills are all ordered on s."""
    assert torch.cuda.current_stream().cuda_stream != streams[0].cuda_stream
    S.run(build(), dev, streams)
    assert torch.cuda.current_stream().cuda_stream != streams[0].cuda_stream
