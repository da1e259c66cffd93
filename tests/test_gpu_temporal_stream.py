"""Stream order of the temporal accumulation (DESIGN sections 17 and 18): every stream-taking export
of include/mrt_temporal.h and every public callable of mrt.temporal, with Renderer.accumulate, under
the stalled-stream protocol of tests/stream_util.py. The exports take the stream as an argument;
the Python callables take none and run on torch's current stream, so a wrapper's call enters
`with torch.cuda.stream(s)` itself: what it allocates, fills and launches must then be ordered on s
with nothing else said. tests/test_temporal_table.py checks without a device that the two tables
are complete and that every decoy is valid input with another result.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mrt  # noqa: E402
import mrt.host  # noqa: E402
from mrt import _lib  # noqa: E402
import denoise_util as D  # noqa: E402
import stream_util as S  # noqa: E402
import temporal_util as TU  # noqa: E402

F, U32 = np.float32, np.uint32

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


def p(t):
    return None if t is None else t.data_ptr()


def sp(stream):
    return None if stream is None else stream.cuda_stream


def on(stream):
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def sentinel(shape, dtype):
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, S.SENTINEL, np.uint8).view(dtype).reshape(shape)


# ---- the raw exports ---------------------------------------------------------------------------------------------------
MOTION_FRAME = (20, 15)      # 300 pixels, 257 slots: two workgroups, the second partial; 43 pixels no slot names
SLOTS = 257


def motion_case_inputs(seed):
    s2i, rays, res, tri, v, pv = TU.motion_inputs(SLOTS, MOTION_FRAME[0] * MOTION_FRAME[1], seed)
    return {"s2i": s2i, "rays": rays, "results": res, "vertices": v, "prev_vertices": pv}, tri


@raw("mrt_temporal_motion")
def case_motion():
    pixels = MOTION_FRAME[0] * MOTION_FRAME[1]
    real, tri = motion_case_inputs(1)
    decoy, _ = motion_case_inputs(2)

    def prepare(dev, b):
        return {"tri": S._upload(tri, dev)}

    def call(b, s, ctx):
        _lib.check(lib().mrt_temporal_motion(SLOTS, p(b["s2i"]), p(b["rays"]), p(b["results"]), p(ctx["tri"]), len(tri),
                                             p(b["vertices"]), p(b["prev_vertices"]), len(real["vertices"]), pixels,
                                             p(b["prev_position"]), sp(s)))

    def twin(x):
        return {"prev_position": mrt.host.temporal_motion(x["s2i"], x["rays"], x["results"], tri, x["vertices"], x["prev_vertices"],
                                                          pixels, sentinel((pixels, 4), F))}
    return S.Case("temporal_motion", real, decoy, {"prev_position": ((pixels, 4), F)}, call, twin, prepare=prepare)


ACCUMULATE_FRAME = (65, 9)   # one column more than two tiles, one row more than one: partial workgroups in both shapes
BUFFERS = ("image", "guide", "albedo", "prev_position", "prev_guide", "prev_history")


@raw("mrt_temporal_accumulate", label="linear", variant=1)
@raw("mrt_temporal_accumulate", label="tiled", variant=2)
def case_accumulate(variant):
    w, h = ACCUMULATE_FRAME
    n = w * h
    frames = [TU.make_frame(w, h, "checker", seed=seed, moving=True) for seed in (66, 67)]
    real, decoy = ({k: kw[k] for k in BUFFERS} for kw in frames)
    scalars = frames[0]
    assert np.array_equal(scalars["prev_world_to_screen"], frames[1]["prev_world_to_screen"])

    def call(b, s, ctx):
        q = _lib.TemporalParams()
        q.width, q.height, q.havePrev, q.maxHistory, q.variant = w, h, 1, scalars["max_history"], variant
        q.normalCos, q.sigmaPlane = float(F(scalars["normal_cos"])), float(F(scalars["sigma_plane"]))
        for i in range(16):
            q.prevWorldToScreen[i] = float(scalars["prev_world_to_screen"][i])
        q.prevSubpixel[0], q.prevSubpixel[1] = (float(F(x)) for x in scalars["prev_subpixel"])
        q.image, q.guide, q.albedo = p(b["image"]), p(b["guide"]), p(b["albedo"])
        q.prevPosition, q.prevGuide, q.prevHistory = p(b["prev_position"]), p(b["prev_guide"]), p(b["prev_history"])
        q.history, q.imageOut, q.pixels = p(b["history"]), p(b["out"]), p(b["pixels"])
        _lib.check(lib().mrt_temporal_accumulate(C.byref(q), sp(s)))

    def twin(x):
        hst, out, px = mrt.host.temporal_accumulate(**dict(scalars, **x))
        assert (hst[:, 3] > 1).sum() > n // 10
        return {"history": hst, "out": out, "pixels": px}
    outs = {"history": ((n, 4), F), "out": ((n, 4), F), "pixels": ((n,), U32)}
    return S.Case(f"temporal_accumulate variant {variant}", real, decoy, outs, call, twin)


# ---- the Python callables -------------------------------------------------------------------------------------------------
SIGMA_PLANE = 2.0
NORMAL_COS = -1.0            # random rays over eight normals: every normal that is a number passes
SUBPIXELS = ((0.5, 0.5), (0.25, 0.875), (0.625, 0.375))


def cameras():
    return [mrt.host.Camera((0.2 * k, -0.1 * k, 8.0), (0.0, 0.02 * k, -1.0), (0.0, 1.0, 0.0), 60.0, 0.01, 100.0) for k in range(3)]


def wrapper_inputs(seed):
    real, tri = motion_case_inputs(seed)
    return dict(real, image=D.make_image(MOTION_FRAME[0] * MOTION_FRAME[1], np.random.default_rng(seed))), tri[:8]


def host_frames(frames, normals, material, tri, matrices, reset_before=()):
    """The host statements over a list of frames (dicts of wrapper_inputs, `moving` among the
    keys): the last frame's guide, history and pixels."""
    w, h = MOTION_FRAME
    n = w * h
    guide = hst = px = None
    for k, x in enumerate(frames):
        prev_guide, prev_hst = (None, None) if k in reset_before else (guide, hst)
        guide, albedo = mrt.host.denoise_features(x["s2i"], x["rays"], x["results"], normals, material, n,
                                                  np.zeros((n, 8), F), np.ones((n, 4), F))
        pp = None
        if x.get("moving"):
            pp = mrt.host.temporal_motion(x["s2i"], x["rays"], x["results"], tri, x["vertices"], x["prev_vertices"], n)
        hst, _, px = mrt.host.temporal_accumulate(x["image"], guide, albedo, w, h, prev_guide, prev_hst,
                                                  matrices[k - 1] if k else None, SUBPIXELS[k - 1] if k else (0.5, 0.5), pp,
                                                  sigma_plane=SIGMA_PLANE, normal_cos=NORMAL_COS, want_image=False)
    return {"guide": guide, "history": hst, "pixels": px, "length": hst[:, 3].copy()}


@wrapper("TemporalAccumulator.accumulate", label="static")
@wrapper("TemporalAccumulator.accumulate", label="moving", moving=True)
@wrapper("TemporalAccumulator.reset", reset=True)
@wrapper("TemporalAccumulator.history_length")
@wrapper("world_to_screen", twice=True)
@wrapper("Renderer.accumulate", renderer=True)
def case_wrapper(wrapper=None, moving=False, reset=False, twice=False, renderer=False):
    """Frame 0 is accumulated in prepare, from inputs of its own; the gated call accumulates frame 1
    (after a reset(); or twice: the second reprojects through the matrix world_to_screen made inside
    the window) under `with torch.cuda.stream(s)` and nothing else."""
    from mrt.temporal import world_to_screen
    normals, material = D.feature_tables()
    w, h = MOTION_FRAME
    first, tri = wrapper_inputs(3)
    real, _ = wrapper_inputs(1)
    decoy, _ = wrapper_inputs(2)
    cams = cameras()
    matrices = [world_to_screen(c, w, h) for c in cams]

    def prepare(dev, b):
        from mrt.raygen import RAY_PATH, DeviceReconstructor
        from mrt.renderer import Renderer
        from mrt.temporal import TemporalAccumulator
        from mrt.tracer import RayBuffer, Tracer
        import frame_util as U
        ctx = {"normals": S._upload(normals, dev), "material": S._upload(material, dev), "tri": S._upload(tri, dev)}
        f = {k: S._upload(v, dev) for k, v in first.items()}
        ctx["first"] = f
        primary0, primary1 = RayBuffer(f["rays"], results=f["results"]), RayBuffer(b["rays"], results=b["results"])
        if renderer:
            v, t, _ = U.edge_scene()
            tracer = Tracer(0)
            r = Renderer(tracer, mrt.Scene.from_arrays(v, t))
            r.set_params(RAY_PATH, 1)
            r._recon = DeviceReconstructor(None)
            r._recon.material, r.gen.normals = ctx["material"], ctx["normals"]
            r.primary, r.slot_to_id, r.w, r.h, r.cam, r._subpixel = primary0, f["s2i"], w, h, cams[0], SUBPIXELS[0]
            r.accumulate(f["image"], sigma_plane=SIGMA_PLANE, normal_cos=NORMAL_COS)
            r.primary, r.slot_to_id, r.cam, r._subpixel = primary1, b["s2i"], cams[1], SUBPIXELS[1]
            ctx["renderer"] = r
        else:
            acc = TemporalAccumulator(dev)
            acc.accumulate(primary0, f["s2i"], ctx["normals"], ctx["material"], w, h, matrices[0], SUBPIXELS[0], f["image"],
                           sigma_plane=SIGMA_PLANE, normal_cos=NORMAL_COS)
            ctx["acc"], ctx["primary"] = acc, primary1
        return ctx

    def call(b, s, ctx):
        with on(s):
            if renderer:
                r = ctx["renderer"]
                px, _ = r.accumulate(b["image"], sigma_plane=SIGMA_PLANE, normal_cos=NORMAL_COS)
                acc = r._temporal
            else:
                acc = ctx["acc"]
                if reset:
                    acc.reset()
                motion = dict(triangles=ctx["tri"], vertices=b["vertices"], prev_vertices=b["prev_vertices"]) if moving else {}
                for k in (1, 2) if twice else (1,):
                    px, _ = acc.accumulate(ctx["primary"], b["s2i"], ctx["normals"], ctx["material"], w, h,
                                           world_to_screen(cams[k], w, h), SUBPIXELS[k], b["image"], sigma_plane=SIGMA_PLANE, normal_cos=NORMAL_COS,
                                           **motion)
            return {"pixels": px, "guide": acc.current["guide"], "history": acc.current["history"], "length": acc.history_length()}

    def twin(x):
        frames = [first, dict(x, moving=moving)] + ([dict(x)] if twice else [])
        out = host_frames(frames, normals, material, tri, matrices, reset_before=(1,) if reset else ())
        print(f"{wrapper}: {int((out['length'] > 1).sum())} pixels found history")
        assert reset or (out["length"] > 1).sum() > 10, "the case reprojects nothing"
        return out
    if not moving:
        for d in (real, decoy):
            d.pop("vertices"), d.pop("prev_vertices")
    return S.Case(f"{wrapper} {'moving' if moving else ''}", real, decoy, {}, call, twin, prepare=prepare)


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
