"""Every export of include/mrt.h that takes a `void* stream`, and every stream= method of mrt/*.py,
held to stream order behind a stalled stream (tests/stream_util.py has the protocol, DESIGN section
17 the contract): the inputs reach the device only behind a stall on the stream the call is given,
while torch's current stream is another one. A launch that went to the NULL or to torch's current
stream reads the decoy or writes before the stall ends; a call that waits on the host although it
promises not to leaves the stream idle. One table row per export (RAW) and per method (WRAPPERS);
tests/test_stream_table.py checks on the CPU that the rows are exactly the exports and the methods,
and that every decoy's host-twin result differs from the real one.

The expected values are the host twins' (mrt.host.*, the oracle), bit for bit where the twin gives
bits. Where it does not: the AO generators go through the device's cosf / sinf and are held to the
restated kernel within the 1e-5 the frame-edge tests use; mrt_trace has no exact-reciprocal flag, so
its t is held to 1e-4 relative (v_rcp_f32 is good to 1 ulp, a hit distance a few operations from it)
and its ids to the oracle's on 99 % of the rays (a grazing ray may flip: the renderer tests allow
0.2 %), while its decoy agrees on less than 90 %.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mrt  # noqa: E402
import mrt.host  # noqa: E402
from mrt import _lib  # noqa: E402
import denoise_util as D  # noqa: E402
import frame_util as U  # noqa: E402
import light_util as L  # noqa: E402
import oracle_lib as O  # noqa: E402
import path_util as P  # noqa: E402
import raygen_oracle as RO  # noqa: E402
import raysort_util as RS  # noqa: E402
import refit_util as R  # noqa: E402
import scene_attr_util as SA  # noqa: E402
import stream_util as S  # noqa: E402
import test_denoise as TD  # noqa: E402
import test_path as T  # noqa: E402

F, I32, U32 = np.float32, np.int32, np.uint32
EXACT_PER_LANE = _lib.MRT_TRACE_EXACT_RCP | _lib.MRT_TRACE_LOCKSTEP_OFF   # the oracle's order and bits
DIR_TOL = 1e-5        # tests/test_gpu_frame_edges.py's bound on the device AO generator


def lib():
    return _lib.trace_lib()


def p(t):
    return None if t is None else t.data_ptr()


def sp(stream):
    return None if stream is None else stream.cuda_stream


def sentinel(shape, dtype):
    """What an untouched output holds."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, S.SENTINEL, np.uint8).view(dtype).reshape(shape)


def rev(a):
    return np.ascontiguousarray(a[::-1])


def guarded(check):
    """An asserting comparison as a message."""
    def same(got, want):
        try:
            check(got, want)
        except AssertionError as e:
            return str(e) or "differs"
        return ""
    return same


def ftz(a):
    a = a.copy()
    a[np.abs(a) < F(1.1754944e-38)] = 0.0
    return a


def light3(light):
    return mrt.host._light3(light)


# ---- the two tables ---------------------------------------------------------------------------------
RAW = []        # (export, label, builder of a stream_util.Case)
WRAPPERS = []   # (qualified name of the method, label, builder)


def raw(export, label="", **kw):
    def deco(fn):
        RAW.append((export, label, functools.partial(fn, **kw)))
        return fn
    return deco


def wrapper(name, label="", **kw):
    def deco(fn):
        WRAPPERS.append((name, label, functools.partial(fn, wrapper=name.split(".")[-1], **kw)))
        return fn
    return deco


def new_tracer():
    from mrt.tracer import Tracer
    t = Tracer(0)
    t.set_config(autotune=0)     # one schedule: the exploring launches time themselves
    return t


# ---- a small bound tree ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tree_world():
    """random(1500)'s SBVH, its vertices moved, both refitted on the host, and a 24 x 16 frame of rays."""
    v, t, bufs, _ = R.built("random", 1500, 1e-5)
    moved = R.displaced(v)
    w = dict(v=v, t=t, bufs=bufs, moved=moved, refit0=R.host_refit(bufs, v, t), refit1=R.host_refit(bufs, moved, t),
             rays=R.frame_rays(v, 24, 16), rays_moved=R.frame_rays(moved, 24, 16))
    hits = (O.trace(w["rays"], *w["refit0"])[0][:, 0] != -1).mean()
    assert 0.1 < hits < 1.0, hits      # the frame sees the scene, and its edge
    return w


def bind(dev, b, tree=("nodes", "woop", "tri"), on_device=False):
    """A tracer bound to the case's own (gated) tree tensors."""
    from mrt.tracer import GpuBvh
    t = new_tracer()
    t.set_bvh(GpuBvh(tuple(b[k] for k in tree)), on_device=on_device)
    return t


def oracle_results(rays, tree, any_hit=False):
    return np.ascontiguousarray(O.trace(rays, *tree, any_hit=any_hit)[0][:, :2]).view(I32)


def same_results(got, want, pad=S.SENTINEL * 0x01010101 - (1 << 32)):
    """{id, t} of every ray; the trace leaves the two pad words alone (pad: what they held)."""
    g = np.asarray(got["results"]).view(I32)
    if not np.array_equal(g[:, :2], want["results"]):
        return f"results: {int((g[:, :2] != want['results']).any(1).sum())} rays differ"
    return "" if (g[:, 2:] == pad).all() else "results: pad words written"


@raw("mrt_tracer_trace")
@raw("mrt_tracer_trace_timed", timed=True)
@wrapper("Tracer.trace_async")
@wrapper("Tracer.launcher")
@wrapper("Tracer.trace_batch")
@wrapper("trace_shard", label="contiguous")
@wrapper("trace_shard", label="blocks", block=64)
def case_trace(timed=False, wrapper=None, block=0):
    w = tree_world()
    n = len(w["rays"])
    tree = w["refit0"]

    def prepare(dev, b):
        from mrt.tracer import GpuBvh, RayBuffer
        t = new_tracer()
        t.set_bvh(GpuBvh(tree))
        return {"t": t, "rb": RayBuffer(b["rays"], need_closest_hit=True, results=b.get("results"))}

    def call(b, s, ctx):
        t, rb = ctx["t"], ctx["rb"]
        if wrapper == "trace_async":
            t.trace_async(rb, exact_rcp=True, speculative=False, stream=s)
        elif wrapper == "launcher":
            t.launcher(rb, exact_rcp=True, speculative=False, stream=s)()
        elif wrapper == "trace_batch":
            assert t.trace_batch(rb, exact_rcp=True, speculative=False, stream=s) > 0
        elif wrapper == "trace_shard":
            from mrt.dist import trace_shard
            t.flags = lambda rays, exact_rcp=False, speculative=True, stats=False: EXACT_PER_LANE
            if block == 0:
                assert trace_shard(t, rb, 1, 0, max_rays=100, stream=s) == (0, n)
            else:   # a live-first order of the blocks: the rays are gathered first
                local = trace_shard(t, rb, 1, 0, max_rays=100, stream=s, block=block, priority=np.arange(-(-n // block)))
                return {"local": local.results}
        elif timed:
            info = _lib.TraceInfo()
            _lib.check(lib().mrt_tracer_trace_timed(t._h, p(b["rays"]), p(b["results"]), n, EXACT_PER_LANE, None, sp(s),
                                                    C.byref(info)))
            assert info.kernel_ms > 0
        else:
            _lib.check(lib().mrt_tracer_trace(t._h, p(b["rays"]), p(b["results"]), n, EXACT_PER_LANE, None, sp(s)))

    def twin(x):
        return {"results": oracle_results(x["rays"], tree)}

    def same(got, want):
        if "local" in got:   # the shard's results, in shard_spans order
            from mrt.dist import shard_spans, spans_index
            idx = spans_index(shard_spans(n, 1, 0, block, None, np.arange(-(-n // block)))).numpy()
            return same_results({"results": got["local"]}, {"results": want["results"][idx]}, pad=0)   # a fresh buffer's
        return same_results(got, want)
    blocking = timed or wrapper == "trace_batch"
    outs = {} if (wrapper == "trace_shard" and block) else {"results": ((n, 4), I32)}   # else: the local buffer's
    return S.Case(f"trace {wrapper or ('timed' if timed else 'async')} {block}", {"rays": w["rays"]}, {"rays": rev(w["rays"])},
                  outs, call, twin, same=same, distinct=lambda a, b: not np.array_equal(a["results"], b["results"]),
                  prepare=prepare, blocking=blocking)


@raw("mrt_trace")
def case_compat_trace():
    w = tree_world()
    n = len(w["rays"])
    tree = w["refit0"]

    def prepare(dev, b):
        bufs = [S._upload(a, dev) for a in tree]
        _lib.check(lib().mrt_bind_bvh(p(bufs[0]), bufs[0].numel() * 4, p(bufs[1]), bufs[1].numel() * 4, p(bufs[2]),
                                      bufs[2].numel() * 4))
        return bufs

    def call(b, s, ctx):
        ms = C.c_float(-1.0)
        _lib.check(lib().mrt_trace(p(b["rays"]), p(b["results"]), n, 0, sp(s), C.byref(ms)))
        assert ms.value > 0

    def agreement(got, want):
        g, w_ = np.asarray(got).view(I32)[:, :2], want
        same_id = g[:, 0] == w_[:, 0]
        both = same_id & (w_[:, 0] != -1)
        tg, tw = g[both, 1].view(F).astype(np.float64), w_[both, 1].view(F).astype(np.float64)
        return float(same_id.mean()), float((np.abs(tg - tw) / np.abs(tw)).max()) if both.any() else 0.0

    def same(got, want):
        ids, t_err = agreement(got["results"], want["results"])
        return "" if ids >= 0.99 and t_err <= 1e-4 else f"ids agree on {ids:.4f} of the rays, t within {t_err:.3g}"
    return S.Case("mrt_trace", {"rays": w["rays"]}, {"rays": rev(w["rays"])}, {"results": ((n, 4), I32)}, call,
                  lambda x: {"results": oracle_results(x["rays"], tree)}, same=same,
                  distinct=lambda a, b: agreement(a["results"], b["results"])[0] < 0.9, prepare=prepare,
                  finish=lambda ctx: lib().mrt_unbind_bvh(), blocking=True)


def same_tree(got, want):
    if not R.same_nodes(got["nodes"], want["nodes"]):
        return "nodes differ"
    if "woop" in want and not R.same_bits_or_nan(got["woop"], want["woop"]):
        return "woop differs"
    return ""


@raw("mrt_tracer_refit")
@wrapper("Tracer.refit")
def case_refit(wrapper=None):
    w = tree_world()
    start = w["refit0"]    # what the first, plan-building refit (of the unmoved vertices) leaves

    def prepare(dev, b):
        t = bind(dev, b)
        tris = S._upload(w["t"], dev)
        t.refit(S._upload(w["v"], dev), tris)
        return {"t": t, "tris": tris, "wide": t.wide_nodes()}

    def call(b, s, ctx):
        if wrapper:
            ctx["t"].refit(b["vertices"], ctx["tris"], stream=s)
        else:
            _lib.check(lib().mrt_tracer_refit(ctx["t"]._h, p(b["vertices"]), len(w["v"]), p(ctx["tris"]), len(w["t"]), sp(s)))

    def twin(x):
        nodes, woop, _ = R.host_refit(w["bufs"], x["vertices"], w["t"])
        return {"nodes": nodes, "woop": woop}

    def same(got, want):
        msg = same_tree(got, want)
        if msg == "" and "wide" in got:   # the 4-wide copy follows the refitted boxes
            msg = guarded(lambda g, x: R.check_wide(g["wide_before"], g["wide"], start[0], x["nodes"]))(got, want)
        return msg
    real = {"vertices": w["moved"], "nodes": start[0], "woop": start[1], "tri": start[2]}
    decoy = dict(real, vertices=w["v"])
    return S.Case(f"refit {wrapper or ''}", real, decoy, {}, call, twin, same=same, inout=("nodes", "woop"), prepare=prepare,
                  collect=lambda ctx: {"wide": ctx["t"].wide_nodes(), "wide_before": ctx["wide"]})


def cost_of(c):
    return mrt.host.tree_cost_dict(c)


@raw("mrt_tracer_tree_cost", label="device")
@raw("mrt_tracer_tree_cost", label="host", host=True)
@wrapper("Tracer.tree_cost", label="async")
@wrapper("Tracer.tree_cost", label="sync", host=True)
def case_tree_cost(host=False, wrapper=None):
    w = tree_world()

    def prepare(dev, b):
        return {"t": bind(dev, b)}

    def call(b, s, ctx):
        if wrapper:
            out = ctx["t"].tree_cost(stream=s, sync=host)
            if host:
                ctx["cost"] = out
                return None
            return {"cost": out}
        c = _lib.TreeCost()
        _lib.check(lib().mrt_tracer_tree_cost(ctx["t"]._h, C.byref(c) if host else None, None if host else p(b["cost"]),
                                              sp(s)))
        ctx["cost"] = cost_of(c)

    def twin(x):
        return mrt.Bvh.from_buffers(x["nodes"], x["woop"], x["tri"]).tree_cost()

    def same(got, want):
        g = got["host"].item() if "host" in got else cost_of(_lib.TreeCost.from_buffer_copy(np.asarray(got["cost"]).tobytes()))
        return guarded(lambda a, b: SA.assert_cost_close(a, b))(g, want)
    real = dict(zip(("nodes", "woop", "tri"), w["refit1"]))
    decoy = dict(zip(("nodes", "woop", "tri"), w["refit0"]))
    outs = {} if host or wrapper else {"cost": ((8,), np.float64)}
    return S.Case(f"tree_cost {'host' if host else 'device'} {wrapper or ''}", real, decoy, outs, call, twin, same=same,
                  distinct=lambda a, b: a["inner_area"] != b["inner_area"], prepare=prepare, blocking=host,
                  collect=(lambda ctx: {"host": np.array(ctx["cost"], dtype=object)}) if host else None)


def host_wide(nodes, woop):
    """The exact 4-wide array a bind derives (mrt_derive_wide_nodes, host only)."""
    n, w = np.ascontiguousarray(nodes).view(I32), np.ascontiguousarray(woop).view(I32)
    size = C.c_int64()
    _lib.check(lib().mrt_derive_wide_nodes(n.ctypes.data, n.nbytes, w.ctypes.data, w.nbytes, 1, None, 0, C.byref(size)))
    out = np.zeros(size.value // 4, U32)
    _lib.check(lib().mrt_derive_wide_nodes(n.ctypes.data, n.nbytes, w.ctypes.data, w.nbytes, 1, out.ctypes.data, out.nbytes,
                                           C.byref(size)))
    return out


@raw("mrt_tracer_bind_device")
@wrapper("Tracer.set_bvh")
def case_bind_device(wrapper=None):
    w = tree_world()

    def prepare(dev, b):
        return {"t": new_tracer(), "b": b}

    def call(b, s, ctx):
        t = ctx["t"]
        if wrapper:
            from mrt.tracer import GpuBvh
            t.set_bvh(GpuBvh((b["nodes"], b["woop"], b["tri"])), on_device=True, stream=s)
        else:
            _lib.check(lib().mrt_tracer_bind_device(t._h, p(b["nodes"]), b["nodes"].numel() * 4, p(b["woop"]),
                                                    b["woop"].numel() * 4, p(b["tri"]), b["tri"].numel() * 4, sp(s)))

    def same(got, want):
        return "" if R.same_bits_or_nan(got["wide"], want["wide"]) else "the derived 4-wide array differs"
    real = dict(zip(("nodes", "woop", "tri"), w["refit1"]))
    decoy = dict(zip(("nodes", "woop", "tri"), w["refit0"]))
    return S.Case(f"bind_device {wrapper or ''}", real, decoy, {}, call, lambda x: {"wide": host_wide(x["nodes"], x["woop"])},
                  same=same, prepare=prepare, collect=lambda ctx: {"wide": ctx["t"].wide_nodes()}, blocking=True)


@raw("mrt_tracer_build")
@raw("mrt_tracer_build_device", on_device=True)
@wrapper("Tracer.build", label="host plan")
@wrapper("Tracer.build", label="device plan", on_device=True)
def case_build(on_device=False, wrapper=None):
    w = tree_world()
    nt = len(w["t"])
    cap = [C.c_int64(), C.c_int64(), C.c_int64()]
    _lib.check(lib().mrt_lbvh_sizes(nt, *map(C.byref, cap)))
    names = ("nodes", "woop", "tri")

    def prepare(dev, b):
        return {"t": new_tracer(), "tris": S._upload(w["t"], dev)}

    def call(b, s, ctx):
        t = ctx["t"]
        if wrapper:
            g = t.build(b["vertices"], ctx["tris"], stream=s, on_device=on_device)
            return {"nodes": g.nodes, "woop": g.woop, "tri": g.tri_index}
        out = [C.c_int64(), C.c_int64(), C.c_int64()]
        fn = lib().mrt_tracer_build_device if on_device else lib().mrt_tracer_build
        _lib.check(fn(t._h, p(b["vertices"]), len(w["v"]), p(ctx["tris"]), nt, None, p(b["nodes"]), cap[0].value,
                      p(b["woop"]), cap[1].value, p(b["tri"]), cap[2].value, *map(C.byref, out), sp(s)))
        ctx["bytes"] = [o.value for o in out]

    def twin(x):
        return dict(zip(names, mrt.Bvh.build_lbvh(mrt.Scene.from_arrays(x["vertices"], w["t"])).buffers()))

    def same(got, want):
        for k in names:
            g = np.asarray(got[k]).view(I32).reshape(-1)
            if "bytes" in got and int(got["bytes"][names.index(k)]) != want[k].nbytes:
                return f"{k}: {got['bytes']} bytes written"
            g = g[:len(want[k])]
            ok = R.same_nodes(g, want[k]) if k == "nodes" else (R.same_bits_or_nan(g, want[k]) if k == "woop"
                                                               else np.array_equal(g, want[k]))
            if not ok:
                return f"{k} differs"
        return ""
    outs = {} if wrapper else {k: ((c.value // 4,), I32) for k, c in zip(names, cap)}
    return S.Case(f"build {'device' if on_device else 'host'} plan {wrapper or ''}", {"vertices": w["moved"]},
                  {"vertices": w["v"]}, outs, call, twin, same=same, prepare=prepare, blocking=True,
                  collect=None if wrapper else (lambda ctx: {"bytes": np.array(ctx["bytes"])}))


@raw("mrt_tracer_optimize")
@wrapper("Tracer.optimize")
def case_optimize(wrapper=None):
    w = tree_world()
    names = ("nodes", "woop", "tri")

    def lbvh(v):   # one triangle per leaf: the record count does not depend on the order
        return dict(zip(names, mrt.Bvh.build_lbvh(mrt.Scene.from_arrays(v, w["t"]), 1).buffers()))

    def prepare(dev, b):
        return {"t": bind(dev, b)}

    def call(b, s, ctx):
        if wrapper:
            assert ctx["t"].optimize(1, stream=s)["rounds"] == 1
        else:
            params = _lib.OptimizeParams(rounds=1)
            _lib.check(lib().mrt_tracer_optimize(ctx["t"]._h, C.byref(params), sp(s)))

    def twin(x):
        bvh = mrt.Bvh.from_buffers(x["nodes"], x["woop"], x["tri"])
        assert sum(bvh.optimize(1)["rewritten"]) > 0
        return {"nodes": bvh.buffers()[0]}
    real, decoy = lbvh(w["moved"]), lbvh(w["v"])
    # the export rewrites nodes in place, but from gated contents: it is no in-out buffer of the protocol's
    return S.Case(f"optimize {wrapper or ''}", real, decoy, {}, call, twin,
                  same=lambda got, want: "" if R.same_bits_or_nan(got["nodes"], want["nodes"]) else "nodes differ",
                  prepare=prepare, blocking=True, rewritten=("nodes",),
                  collect=lambda ctx: {"nodes": ctx["t"].bvh.nodes.cpu().numpy()})


# ---- ray generation ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mori_camera():
    return mrt.Scene.synthetic("mori", 0, 1).camera()[0]


@raw("mrt_raygen_primary")
@raw("mrt_raygen_primary_subpixel", subpixel=(0.25, 0.875))
@wrapper("DeviceRayGen.primary", subpixel=(0.25, 0.875))
def case_primary(subpixel=None, wrapper=None):
    from mrt.raygen import nscreen_to_world
    cam, (w, h) = mori_camera(), (64, 9)
    n = w * h
    table = mrt.pixel_table(w, h)
    m, origin = nscreen_to_world(cam, w, h), np.array(cam.position, F)

    def prepare(dev, b):
        from mrt.raygen import DeviceRayGen
        g = DeviceRayGen()
        g._tables[(w, h)] = b["table"]     # the generator's cached pixel table is the gated one
        return g

    def call(b, s, g):
        if wrapper:
            rb, s2i = g.primary(cam, w, h, stream=s, subpixel=subpixel)
            return {"rays": rb.rays, "slot_to_id": s2i, "results": rb.results}
        cm, co = m.ctypes.data_as(C.POINTER(C.c_float)), origin.ctypes.data_as(C.POINTER(C.c_float))
        tail = (p(b["table"]), p(b["rays"]), p(b["slot_to_id"]), p(b["id_to_slot"]), sp(s))
        if subpixel:
            _lib.check(lib().mrt_raygen_primary_subpixel(cm, co, float(cam.far), w, h, *map(float, subpixel), *tail))
        else:
            _lib.check(lib().mrt_raygen_primary(cm, co, float(cam.far), w, h, *tail))

    def twin(x):
        rays, s2i = mrt.host.primary_rays(cam, w, h, subpixel or (0.5, 0.5))
        by_pixel = np.empty_like(rays)
        by_pixel[s2i] = rays
        inverse = np.empty(n, I32)
        inverse[x["table"]] = np.arange(n, dtype=I32)
        out = {"rays": ftz(by_pixel[x["table"]]), "slot_to_id": x["table"]}
        return dict(out, results=np.zeros((n, 4), I32)) if wrapper else dict(out, id_to_slot=inverse)
    outs = {} if wrapper else {"rays": ((n, 8), F), "slot_to_id": ((n,), I32), "id_to_slot": ((n,), I32)}
    return S.Case(f"primary {subpixel} {wrapper or ''}", {"table": table}, {"table": rev(table)}, outs, call, twin,
                  prepare=prepare)


def block_list(total, block_rays, seed):
    """Every block of the frame in a shuffled order, the partial last block last."""
    nb = -(-total // block_rays)
    full = nb - 1 if total % block_rays else nb
    order = np.random.default_rng(seed).permutation(full)
    return (np.append(order, nb - 1) if total % block_rays else order).astype(I32)


def listed_at(blocks, block_rays, total):
    return np.concatenate([np.arange(b * block_rays, min((b + 1) * block_rays, total)) for b in blocks])


def many_seeds(n):
    seeds = [int(s) for s in np.random.default_rng(9).integers(0, 2**32, n)]
    seeds[7], seeds[n - 5] = 0xFFFFFFFF, 0
    return seeds


@raw("mrt_raygen_ao")
@raw("mrt_raygen_ao_blocks", label="3 batches", batch_inputs=200)
@raw("mrt_raygen_ao_blocks", label="495 batches", batch_inputs=1)
@wrapper("DeviceRayGen.ao")
@wrapper("DeviceRayGen.ao_blocks", batch_inputs=1)
def case_ao(batch_inputs=0, wrapper=None):
    """The frame-edge table; with batch_inputs, the block generator over the frame's batches (more than
    256 of them: the seeds travel through stream-ordered scratch)."""
    v, t, normals = U.edge_scene()
    rays, res, _ = U.edge_inputs()
    n, samples, block_rays = len(rays), 3, 100
    total = n * samples
    seeds = [1] if not batch_inputs else ([U.EDGE_SEEDS[1], 1, 0x9E3779B9] if batch_inputs == 200 else many_seeds(n))
    assert not batch_inputs or (len(seeds) > 256) == (batch_inputs == 1) and total % block_rays
    real = {"in_rays": rays, "in_results": res, "normals": normals}
    decoy = {"in_rays": rev(rays), "in_results": rev(res), "normals": normals.copy()}
    if batch_inputs:
        real["blocks"], decoy["blocks"] = block_list(total, block_rays, 3), block_list(total, block_rays, 4)

    def prepare(dev, b):
        from mrt.raygen import DeviceRayGen
        from mrt.tracer import RayBuffer
        g = DeviceRayGen()
        g.normals, g.num_tris = b["normals"], len(normals)
        return {"g": g, "rb": RayBuffer(b["in_rays"], results=b["in_results"])}

    def call(b, s, ctx):
        g, rb = ctx["g"], ctx["rb"]
        if wrapper == "ao":
            out = g.ao(rb, samples, U.EDGE_MAX_DIST, seed=seeds[0], stream=s)
            return {"out": out.rays, "results": out.results}
        if wrapper == "ao_blocks":
            out = g.ao_blocks(rb, samples, U.EDGE_MAX_DIST, seeds, batch_inputs, b["blocks"], block_rays, total, stream=s)
            return {"out": out.rays, "results": out.results}
        if not batch_inputs:
            _lib.check(lib().mrt_raygen_ao(p(b["in_rays"]), p(b["in_results"]), n, p(b["normals"]), len(normals), samples,
                                           U.EDGE_MAX_DIST, seeds[0], p(b["out"]), p(b["id_to_slot"]), p(b["slot_to_id"]),
                                           sp(s)))
            return None
        sd = (C.c_uint32 * len(seeds))(*seeds)
        _lib.check(lib().mrt_raygen_ao_blocks(p(b["in_rays"]), p(b["in_results"]), n, p(b["normals"]), len(normals), samples,
                                              U.EDGE_MAX_DIST, C.cast(sd, C.c_void_p), len(seeds), batch_inputs, p(b["blocks"]),
                                              len(real["blocks"]), block_rays, total, p(b["out"]), sp(s)))

    def twin(x):
        seed = U.frame_seeds(seeds, batch_inputs, n) if batch_inputs else seeds[0]
        at = listed_at(x["blocks"], block_rays, total) if batch_inputs else np.arange(total)
        return {"oracle": RO.ao_rays(x["in_rays"], x["in_results"], x["normals"], samples, U.EDGE_MAX_DIST, seed, ftz=True),
                "at": at}

    def check(got, want):
        frame = np.empty((total, 8), F)
        frame[want["at"]] = np.asarray(got["out"]).view(F)
        U.compare_ao(frame, want["oracle"], DIR_TOL)
        for k in ("id_to_slot", "slot_to_id"):
            assert k not in got or np.array_equal(got[k], np.arange(total)), k
        assert "results" not in got or not np.asarray(got["results"]).any(), "the new buffer's results are not zero"

    def distinct(a, b):
        return not np.array_equal(a["at"], b["at"]) or not np.array_equal(a["oracle"]["tmax"], b["oracle"]["tmax"])
    outs = {} if wrapper else {"out": ((total, 8), F)}
    if not wrapper and not batch_inputs:
        outs.update(id_to_slot=((total,), I32), slot_to_id=((total,), I32))
    return S.Case(f"ao {batch_inputs} {wrapper or ''}", real, decoy, outs, call, twin, same=guarded(check), distinct=distinct,
                  prepare=prepare)


def shadow_frame(rays, res, samples, light, radius, seeds, batch_inputs):
    """The frame's shadow rays as RayGen::batching's batches hold them, on the host."""
    parts = []
    for k, first in enumerate(range(0, len(rays), batch_inputs)):
        parts.append(mrt.host.shadow_rays(rays, res, samples, light, radius, seed=seeds[k], first=first,
                                          count=min(batch_inputs, len(rays) - first)))
    return np.concatenate(parts)


@raw("mrt_raygen_shadow")
@raw("mrt_raygen_shadow_blocks", label="3 batches", batch_inputs=200)
@raw("mrt_raygen_shadow_blocks", label="512 batches", batch_inputs=1)
@wrapper("DeviceRayGen.shadow")
@wrapper("DeviceRayGen.shadow_blocks", batch_inputs=1)
@wrapper("Renderer.secondary_blocks", batch_inputs=200)
@wrapper("Renderer.shard", batch_inputs=200)
def case_shadow(batch_inputs=0, wrapper=None):
    rays, res = L.edge_inputs()
    light, radius = L.ORDINARY_LIGHT
    n, samples, block_rays = len(rays), 3, 100
    total = n * samples
    renderer = wrapper in ("secondary_blocks", "shard")
    if renderer:   # the renderer draws its batch seeds itself, one rand() per batch
        from mrt.renderer import GlibcRand
        rand = GlibcRand()
        seeds = [rand() for _ in range(-(-n // batch_inputs))]
    else:
        seeds = [1] if not batch_inputs else ([L.EDGE_SEEDS[1], 1, 0x9E3779B9] if batch_inputs == 200 else many_seeds(n))
    assert not batch_inputs or (len(seeds) > 256) == (batch_inputs == 1) and total % block_rays
    real, decoy = {"in_rays": rays, "in_results": res}, {"in_rays": rev(rays), "in_results": rev(res)}
    if batch_inputs and wrapper != "shard":
        real["blocks"], decoy["blocks"] = block_list(total, block_rays, 3), block_list(total, block_rays, 4)

    def prepare(dev, b):
        from mrt.raygen import RAY_SHADOW, DeviceRayGen
        from mrt.renderer import GlibcRand, Renderer
        from mrt.tracer import RayBuffer
        rb = RayBuffer(b["in_rays"], results=b["in_results"])
        if not renderer:
            return {"g": DeviceRayGen(), "rb": rb}
        v, t, _ = U.edge_scene()
        r = Renderer(new_tracer(), mrt.Scene.from_arrays(v, t), max_batch=batch_inputs * samples, rand=GlibcRand())
        r.set_params(RAY_SHADOW, samples, light_pos=light, light_radius=radius)
        r.primary = rb
        return {"r": r}

    def call(b, s, ctx):
        if wrapper == "shadow":
            out = ctx["g"].shadow(ctx["rb"], samples, light, radius, seed=seeds[0], stream=s)
        elif wrapper == "shadow_blocks":
            out = ctx["g"].shadow_blocks(ctx["rb"], samples, light, radius, seeds, batch_inputs, b["blocks"], block_rays,
                                         total, stream=s)
        elif wrapper == "secondary_blocks":
            out = ctx["r"].secondary_blocks(b["blocks"], total, block_rays, stream=s)
        elif wrapper == "shard":
            out = ctx["r"].shard(1, 0, block_rays, order=1, stream=s)
        elif not batch_inputs:
            _lib.check(lib().mrt_raygen_shadow(p(b["in_rays"]), p(b["in_results"]), n, samples, light3(light), radius, seeds[0],
                                               p(b["out"]), p(b["id_to_slot"]), p(b["slot_to_id"]), sp(s)))
            return None
        else:
            sd = (C.c_uint32 * len(seeds))(*seeds)
            _lib.check(lib().mrt_raygen_shadow_blocks(p(b["in_rays"]), p(b["in_results"]), n, samples, light3(light), radius,
                                                      C.cast(sd, C.c_void_p), len(seeds), batch_inputs, p(b["blocks"]),
                                                      len(real["blocks"]), block_rays, total, p(b["out"]), sp(s)))
            return None
        assert out.size == total and not out.need_closest_hit
        return {"out": out.rays, "results": out.results}

    def twin(x):
        if not batch_inputs:
            ident = np.arange(total, dtype=I32)
            out = {"out": mrt.host.shadow_rays(x["in_rays"], x["in_results"], samples, light, radius, seed=seeds[0])}
            return dict(out, results=np.zeros((total, 4), I32)) if wrapper else dict(out, id_to_slot=ident, slot_to_id=ident)
        frame = shadow_frame(x["in_rays"], x["in_results"], samples, light, radius, seeds, batch_inputs)
        blocks = x["blocks"] if wrapper != "shard" else live_first(x["in_results"], samples, block_rays)
        out = {"out": frame[listed_at(blocks, block_rays, total)]}
        return dict(out, results=np.zeros((total, 4), I32)) if wrapper else out
    outs = {} if wrapper else {"out": ((total, 8), F)}
    if not wrapper and not batch_inputs:
        outs.update(id_to_slot=((total,), I32), slot_to_id=((total,), I32))
    return S.Case(f"shadow {batch_inputs} {wrapper or ''}", real, decoy, outs, call, twin, prepare=prepare)


def live_first(results, samples, block_rays, world=1, rank=0):
    """mrt_shard_blocks' live-first list by the host deal (mrt.dist)."""
    from mrt.dist import live_block_weights, live_priority, shard_blocks
    res = torch.from_numpy(np.ascontiguousarray(results).view(I32).reshape(-1, 4).copy())
    prio = live_priority(live_block_weights(res, samples, block_rays), block_rays)
    return shard_blocks(len(res) * samples, world, rank, block_rays, priority=prio).astype(I32)


# 300 primaries: one workgroup's LDS sort, two launches. 16 385 one-ray blocks: the smallest frame and
# block size that give one rank more than the 16 384 entries a workgroup sorts, so the tiled path's
# four launches and its scratch.
@raw("mrt_shard_blocks", label="two launches", num_primary=300, samples=3, block_rays=7)
@raw("mrt_shard_blocks", label="tiled", num_primary=16385, samples=1, block_rays=1)
@wrapper("DeviceRayGen.shard_blocks", num_primary=16385, samples=1, block_rays=1)
def case_shard_blocks(num_primary, samples, block_rays, wrapper=None):
    hit = np.random.default_rng(num_primary).random(num_primary) < 0.6
    nblocks = -(-num_primary * samples // block_rays)
    assert (nblocks > 16384) == (num_primary == 16385)

    def results_of(h):
        res = np.zeros((num_primary, 4), I32)
        res[:, 0] = np.where(h, 5, -1)
        return res

    def prepare(dev, b):
        from mrt.raygen import DeviceRayGen
        from mrt.tracer import RayBuffer
        return {"g": DeviceRayGen(), "rb": RayBuffer(torch.zeros((num_primary, 8), device=dev), results=b["results"])}

    def call(b, s, ctx):
        if wrapper:
            blocks, m = ctx["g"].shard_blocks(ctx["rb"], samples, block_rays, 1, 0, 1, stream=s)
            assert m == num_primary * samples
            return {"blocks": blocks}
        n, m = C.c_int32(-1), C.c_int64(-1)
        _lib.check(lib().mrt_shard_blocks(p(b["results"]), num_primary, samples, block_rays, 1, 0, 1, p(b["blocks"]), nblocks,
                                          C.byref(n), C.byref(m), sp(s)))
        assert (n.value, m.value) == (nblocks, num_primary * samples)
    return S.Case(f"shard_blocks {nblocks} {wrapper or ''}", {"results": results_of(hit)}, {"results": results_of(~hit)},
                  {} if wrapper else {"blocks": ((nblocks,), I32)}, call,
                  lambda x: {"blocks": live_first(x["results"], samples, block_rays)}, prepare=prepare)


# ---- the ray sort -------------------------------------------------------------------------------------------------
def sort_check(got, want):
    got = dict(got)
    if "keys" not in got:   # the library's own scratch held them
        got.update(keys=want["keys"], box=want["box"])
    RS.assert_same_sort(got, want)


# 4 099 rays: 17 workgroups of the box reduction, a partial last one. drop_levels 0, 4, 15: three, two and
# one radix passes. given: the caller's key and box buffers instead of the library's scratch.
@raw("mrt_ray_sort", label="3 passes, own keys", drop=0, given=False)
@raw("mrt_ray_sort", label="2 passes, own keys", drop=4, given=False)
@raw("mrt_ray_sort", label="1 pass, own keys", drop=15, given=False)
@raw("mrt_ray_sort", label="3 passes, given keys", drop=0, given=True)
@raw("mrt_ray_sort", label="2 passes, given keys", drop=4, given=True)
@raw("mrt_ray_sort", label="1 pass, given keys", drop=15, given=True)
@wrapper("RayBuffer.morton_sort", drop=0, given=True)
def case_ray_sort(drop, given, wrapper=None):
    n = 4099
    real = {"in_rays": RS.random_rays(n), "ids": RS.shuffled_ids(n)}
    decoy = {"in_rays": RS.random_rays(n, seed=8), "ids": RS.shuffled_ids(n, seed=12)}

    def call(b, s, ctx):
        if wrapper:
            from mrt.tracer import RayBuffer
            rb = RayBuffer(b["in_rays"], need_closest_hit=False, secondary=True)
            out, i2s, s2i, keys, box = rb.morton_sort(b["ids"], drop, 0, stream=s, want_keys=True)
            return {"rays": out.rays, "id_to_slot": i2s, "slot_to_id": s2i, "keys": keys, "box": box, "results": out.results}
        params = _lib.RaySortParams(drop_levels=drop, box=0)
        _lib.check(lib().mrt_ray_sort(p(b["in_rays"]), p(b["ids"]), n, C.byref(params), p(b["rays"]), p(b["id_to_slot"]),
                                      p(b["slot_to_id"]), p(b.get("keys")), p(b.get("box")), sp(s)))

    def check(got, want):
        sort_check(got, want)
        assert "results" not in got or not np.asarray(got["results"]).any(), "the new buffer's results are not zero"
    outs = {} if wrapper else {"rays": ((n, 8), F), "id_to_slot": ((n,), I32), "slot_to_id": ((n,), I32)}
    if given and not wrapper:
        outs.update(keys=((n, 6), U32), box=((6,), F))
    return S.Case(f"ray_sort drop {drop} {'given' if given else 'own'} keys {wrapper or ''}", real, decoy, outs, call,
                  lambda x: mrt.host.ray_sort(x["in_rays"], x["ids"], drop, 0), same=guarded(check),
                  distinct=lambda a, b: guarded(sort_check)(a, b) != "")


# ---- hit counts and the reconstructions ----------------------------------------------------------------------------
@raw("mrt_count_hits")
@wrapper("DeviceRayGen.count_hits_async")
@wrapper("DeviceRayGen.count_hits")
def case_count_hits(wrapper=None):
    n = 1000
    rng = np.random.default_rng(5)
    real = U.results(np.where(rng.random(n) < 0.37, rng.integers(0, 1 << 30, n), -1).astype(I32))
    decoy = U.results(np.where(rng.random(n) < 0.6, 3, -2).astype(I32))

    def prepare(dev, b):
        from mrt.raygen import DeviceRayGen
        from mrt.tracer import RayBuffer
        return {"g": DeviceRayGen(), "rb": RayBuffer(torch.zeros((n, 8), device=dev), results=b["results"])}

    def call(b, s, ctx):
        if wrapper == "count_hits":
            return {"count": [ctx["g"].count_hits(ctx["rb"], stream=s)]}    # what the method returns to the host
        if wrapper:
            return {"count": ctx["g"].count_hits_async(ctx["rb"], stream=s)}
        _lib.check(lib().mrt_count_hits(p(b["results"]), n, p(b["count"]), sp(s)))
    return S.Case(f"count_hits {wrapper or ''}", {"results": real}, {"results": decoy}, {} if wrapper else {"count": ((1,), I32)},
                  call, lambda x: {"count": np.array([mrt.host.count_hits(x["results"])], I32)}, prepare=prepare,
                  blocking=wrapper == "count_hits")


def random_ids(rng, n, miss=0.3):
    return np.where(rng.random(n) < miss, -1, rng.integers(0, 64, n)).astype(I32)


@raw("mrt_reconstruct")
@wrapper("DeviceReconstructor.reconstruct")
def case_reconstruct(wrapper=None):
    mat, sh = U.colour_tables()
    first, count, n, ray_type = 1, 300, 3, 1
    num_primary, num_pixels = first + count + 5, first + count + 12

    def inputs(seed):
        rng = np.random.default_rng(seed)
        return {"s2i": rng.permutation(num_pixels)[:num_primary].astype(I32), "primary": U.results(random_ids(rng, num_primary)),
                "batch": U.results(random_ids(rng, count * n, 0.5))}

    def prepare(dev, b):
        from mrt.raygen import DeviceReconstructor
        from mrt.tracer import RayBuffer
        r = DeviceReconstructor(None)
        r.material, r.shaded = S._upload(mat, dev), S._upload(sh, dev)
        zeros = torch.zeros((num_primary, 8), device=dev)
        return {"r": r, "primary": RayBuffer(zeros, results=b["primary"]),
                "batch": RayBuffer(torch.zeros((count * n, 8), device=dev), results=b["batch"])}

    def call(b, s, ctx):
        r = ctx["r"]
        if wrapper:
            return {"pixels": r.reconstruct(ray_type, ctx["primary"], b["s2i"], num_pixels, batch=ctx["batch"], num_samples=n,
                                            stream=s, first_primary=first)}
        _lib.check(lib().mrt_reconstruct(ray_type, n, first, count, p(b["s2i"]), p(b["primary"]), None, p(b["batch"]),
                                         p(r.material), p(r.shaded), p(b["pixels"]), sp(s)))

    def twin(x):
        pix = O.reconstruct(ray_type, n, x["s2i"], x["primary"], x["batch"], mat, sh, num_pixels, first_primary=first,
                            num_primary=count)
        if not wrapper:   # pixels the batch does not name keep what they held
            untouched = np.ones(num_pixels, bool)
            untouched[x["s2i"][first:first + count]] = False
            pix[untouched] = sentinel(1, U32)[0]
        return {"pixels": pix}
    return S.Case(f"reconstruct {wrapper or ''}", inputs(1), inputs(2), {} if wrapper else {"pixels": ((num_pixels,), U32)},
                  call, twin, prepare=prepare)


@raw("mrt_reconstruct_lit")
@wrapper("DeviceReconstructor.reconstruct_lit")
def case_reconstruct_lit(wrapper=None):
    normals, material, rays, res, s2i, num_pixels = L.lit_table()
    first, n, light = 1, 3, L.lit_lights()[1]
    real = L.lit_case(first, n, True, light, np.random.default_rng(3))
    fake = L.lit_case(first, n, True, light, np.random.default_rng(4))
    names = {"batch": "batch_results", "b2s": "batch_id_to_slot"}

    def prepare(dev, b):
        from mrt.raygen import DeviceReconstructor
        from mrt.tracer import RayBuffer
        r = DeviceReconstructor(None)
        r.material = S._upload(material, dev)
        primary = RayBuffer(rays.copy())
        primary.results.copy_(S._upload(res, dev))
        return {"r": r, "normals": S._upload(normals, dev), "s2i": S._upload(s2i, dev), "primary": primary,
                "batch": RayBuffer(torch.zeros((len(real["batch_results"]), 8), device=dev), results=b["batch"])}

    def call(b, s, ctx):
        r, primary = ctx["r"], ctx["primary"]
        if wrapper:
            return {"pixels": r.reconstruct_lit(primary, ctx["s2i"], num_pixels, ctx["batch"], n, ctx["normals"], light,
                                                batch_id_to_slot=b["b2s"], stream=s, first_primary=first)}
        _lib.check(lib().mrt_reconstruct_lit(n, first, L.LIT_COUNT, p(ctx["s2i"]), p(primary.rays), p(primary.results),
                                             p(b["b2s"]), p(b["batch"]), p(ctx["normals"]), p(r.material), light3(light),
                                             p(b["pixels"]), sp(s)))

    def twin(x):
        kw = dict(real, batch_results=x["batch"], batch_id_to_slot=x["b2s"])
        return {"pixels": mrt.host.reconstruct_lit(pixels=np.zeros(num_pixels, U32) if wrapper else sentinel(num_pixels, U32), **kw)}
    return S.Case(f"reconstruct_lit {wrapper or ''}", {k: real[v] for k, v in names.items()},
                  {k: fake[v] for k, v in names.items()}, {} if wrapper else {"pixels": ((num_pixels,), U32)}, call, twin,
                  prepare=prepare)


# ---- paths -------------------------------------------------------------------------------------------------------------
# vertex 0 over the edge table (1 176 slots), vertex 1 over 257 slots (one more than a workgroup of the
# count launch), compacted and in place: count, scan and step, with their scratch; liveCount is an output.
@raw("mrt_path_extend", label="vertex 0", vertex=0, compact=True)
@raw("mrt_path_extend", label="vertex 1 compact", vertex=1, compact=True)
@raw("mrt_path_extend", label="vertex 1 in place", vertex=1, compact=False)
@wrapper("PathIntegrator.extend_async", vertex=0, compact=True)
@wrapper("PathIntegrator.extend", vertex=0, compact=True)
def case_path_extend(vertex, compact, wrapper=None):
    normals, material = P.edge_tables()
    rng = np.random.default_rng(31 + vertex)
    samples, depth = 3, 2
    if vertex == 0:
        rays, res, state, paths, slots = T.edge_case(rng, 0, samples, False)
    else:
        slots, paths = 257, 300
        rays, res = P.slots_for(rng.random(slots) < 0.5, rng)
        state = P.edge_state(rng, slots, paths)
    start = np.zeros((paths, 4), F) if wrapper else rng.random((paths, 4)).astype(F)
    kw = dict(vertex=vertex, depth=depth, num_samples=samples, seed=7, compact=compact, **P.EDGE_LIGHT)
    real = {"rays": rays, "results": res}
    decoy = {"rays": np.roll(rays, 2, axis=0), "results": np.roll(res, 1, axis=0)}
    if state is not None:
        real["state"], decoy["state"] = state, np.roll(state, 3, axis=0)
    if not wrapper:
        real["radiance"], decoy["radiance"] = start, start.copy()

    def prepare(dev, b):
        tables = {"normals": S._upload(normals, dev), "material": S._upload(material, dev)}
        if wrapper:
            from mrt.path import PathIntegrator
            from mrt.tracer import RayBuffer
            g = PathIntegrator(None, dev)
            g.begin(RayBuffer(b["rays"], results=b["results"]), 0, len(rays), samples, depth, 7, tables["normals"],
                    tables["material"], P.EDGE_LIGHT["light_pos"], P.EDGE_LIGHT["light_radius"], P.EDGE_LIGHT["light_color"],
                    P.EDGE_LIGHT["sky"], P.EDGE_LIGHT["max_dist"], compact)
            tables["g"] = g
        return tables

    def call(b, s, ctx):
        if wrapper:
            g = ctx["g"]
            if wrapper == "extend":
                live = [g.extend(0, stream=s)]     # what the method returns to the host
            else:
                g.extend_async(0, stream=s)
                live = g.live_count
            return {"shadow": g.shadow_rays[:slots], "pending": g.pending[:slots], "rays_out": g.rays[1][:slots],
                    "state_out": g.state[1][:slots], "live": live, "radiance": g.radiance[:paths]}
        q = mrt.host.path_params(**kw)
        q.triNormals, q.triMaterialColor, q.numTris = p(ctx["normals"]), p(ctx["material"]), len(material)
        q.numSlots, q.numPaths = slots, paths
        q.inRays, q.inResults, q.inState = p(b["rays"]), p(b["results"]), p(b.get("state"))
        q.outShadowRays, q.outPending, q.outRays, q.outState = p(b["shadow"]), p(b["pending"]), p(b["rays_out"]), p(b["state_out"])
        q.radiance, q.liveCount = p(b["radiance"]), p(b["live"])
        _lib.check(lib().mrt_path_extend(C.byref(q), sp(s)))

    def twin(x):
        rad = x.get("radiance", start).copy()
        step = mrt.host.path_extend(x["rays"], x["results"], x.get("state"), rad, normals, material, num_slots=slots, **kw)
        return {"step": step, "radiance": rad}

    def same(got, want):
        step = {"shadow": got["shadow"], "pending": got["pending"], "rays": got["rays_out"], "state": got["state_out"],
                "live": int(np.asarray(got["live"]).reshape(-1)[0])}
        msg = P.same_step(step, want["step"], live_only=compact)
        return msg or ("" if P.same_floats(got["radiance"], want["radiance"]) else "radiance differs")

    def distinct(a, b):
        return P.same_step(a["step"], b["step"]) != ""
    outs = {} if wrapper else {"shadow": ((slots, 8), F), "pending": ((slots, 4), F), "rays_out": ((slots, 8), F),
                               "state_out": ((slots, 4), I32), "live": ((1,), I32)}
    return S.Case(f"path_extend vertex {vertex} {'compact' if compact else 'in place'} {wrapper or ''}", real, decoy, outs, call,
                  twin, same=same, distinct=distinct, inout=() if wrapper else ("radiance",), prepare=prepare,
                  blocking=wrapper == "extend")


@raw("mrt_path_accumulate")
@wrapper("PathIntegrator.accumulate")
def case_path_accumulate(wrapper=None):
    rng = np.random.default_rng(8)
    n, paths = 300, 320
    state, pending = P.edge_state(rng, n, paths, dead_every=5), rng.random((n, 4)).astype(F)
    pending[::9, 0], pending[1::9, 1] = np.nan, 1e-39
    sres = U.results(np.where(rng.random(n) < 0.5, -1, rng.integers(0, 64, n)).astype(I32))
    radiance = rng.random((paths, 4)).astype(F)
    real = {"state": state, "pending": pending, "sres": sres, "radiance": radiance}
    decoy = {"state": state.copy(), "pending": np.roll(pending, 1, axis=0), "sres": np.roll(sres, 2, axis=0),
             "radiance": radiance.copy()}

    def call(b, s, ctx):
        if wrapper:
            from mrt.path import PathIntegrator
            g = PathIntegrator(None, b["state"].device)
            g.num_slots, g.num_paths, g._cur = n, paths, 0
            g.state, g.pending, g.shadow_results, g.radiance = [None, b["state"]], b["pending"], b["sres"], b["radiance"]
            g.accumulate(stream=s)
        else:
            _lib.check(lib().mrt_path_accumulate(n, paths, p(b["state"]), p(b["pending"]), p(b["sres"]), p(b["radiance"]), sp(s)))
    return S.Case(f"path_accumulate {wrapper or ''}", real, decoy, {}, call,
                  lambda x: {"radiance": mrt.host.path_accumulate(x["state"], x["pending"], x["sres"], x["radiance"].copy())},
                  inout=("radiance",))


@raw("mrt_path_resolve")
@wrapper("PathIntegrator.resolve")
def case_path_resolve(wrapper=None):
    samples, first, count = 3, 1, 300
    pixels = first + count + 9

    def inputs(seed):
        rng = np.random.default_rng(seed)
        radiance = (rng.random((count * samples, 4)) * 1.5).astype(F)
        radiance[::31, 1], radiance[5::37, 2] = np.nan, -0.25
        return {"s2i": rng.permutation(pixels)[:first + count].astype(I32),
                "primary": U.results(np.where(rng.random(first + count) < 0.2, -1, 3).astype(I32)), "radiance": radiance}

    def call(b, s, ctx):
        if wrapper:
            from mrt.path import PathIntegrator
            from mrt.tracer import RayBuffer
            g = PathIntegrator(None, b["s2i"].device)
            g.num_samples, g.first, g.count, g.radiance = samples, first, count, b["radiance"]
            g.primary = RayBuffer(ctx, results=b["primary"])
            return {"pixels": g.resolve(b["s2i"], pixels, stream=s)}
        _lib.check(lib().mrt_path_resolve(samples, first, count, p(b["s2i"]), p(b["primary"]), p(b["radiance"]), p(b["pixels"]),
                                          p(b["image"]), sp(s)))

    def twin(x):
        if wrapper:
            return {"pixels": mrt.host.path_resolve(samples, x["s2i"], x["primary"], x["radiance"], pixels, first_primary=first,
                                                    num_primary=count)}
        px, img = mrt.host.path_resolve(samples, x["s2i"], x["primary"], x["radiance"], pixels, first_primary=first,
                                        num_primary=count, pixels=sentinel(pixels, U32), image=sentinel((pixels, 4), F))
        return {"pixels": px, "image": img}
    return S.Case(f"path_resolve {wrapper or ''}", inputs(1), inputs(2),
                  {} if wrapper else {"pixels": ((pixels,), U32), "image": ((pixels, 4), F)}, call, twin,
                  prepare=lambda dev, b: torch.zeros((first + count, 8), device=dev))


# ---- the denoiser ----------------------------------------------------------------------------------------------------
FEATURE_FRAME = (20, 15)     # 300 pixels, 257 slots: two workgroups, the second partial; 43 pixels no slot names


def feature_case_inputs(seed):
    s2i, rays, res = D.feature_inputs(257, FEATURE_FRAME[0] * FEATURE_FRAME[1], seed=seed)
    return {"s2i": s2i, "rays": rays, "results": res}


@raw("mrt_denoise_features")
@wrapper("Denoiser.set_frame")
def case_denoise_features(wrapper=None):
    normals, material = D.feature_tables()
    w, h = FEATURE_FRAME
    pixels = w * h

    def prepare(dev, b):
        from mrt.tracer import RayBuffer
        return {"normals": S._upload(normals, dev), "material": S._upload(material, dev),
                "primary": RayBuffer(b["rays"], results=b["results"])}

    def call(b, s, ctx):
        if wrapper:
            from mrt.denoise import Denoiser
            d = Denoiser(b["s2i"].device)
            d.set_frame(ctx["primary"], b["s2i"], ctx["normals"], ctx["material"], w, h, stream=s)
            return {"guide": d.guide, "albedo": d.albedo}
        _lib.check(lib().mrt_denoise_features(257, p(b["s2i"]), p(b["rays"]), p(b["results"]), p(ctx["normals"]), p(ctx["material"]),
                                              len(material), pixels, p(b["guide"]), p(b["albedo"]), sp(s)))

    def twin(x):   # pixels no slot names: a miss's record through the wrapper, else what the buffers held
        guide = np.zeros((pixels, 8), F) if wrapper else sentinel((pixels, 8), F)
        albedo = np.ones((pixels, 4), F) if wrapper else sentinel((pixels, 4), F)
        g, a = mrt.host.denoise_features(x["s2i"], x["rays"], x["results"], normals, material, pixels, guide, albedo)
        return {"guide": g, "albedo": a}
    return S.Case(f"denoise_features {wrapper or ''}", feature_case_inputs(1), feature_case_inputs(2),
                  {} if wrapper else {"guide": ((pixels, 8), F), "albedo": ((pixels, 4), F)}, call, twin, prepare=prepare)


FILTER_FRAME = (65, 9)       # one column more than a staged tile, one row more than a direct one
FILTER_SIGMAS = (0.7, 0.3)


@functools.lru_cache(maxsize=None)
def mixed_iterations():
    """The smallest iteration count whose launch chain, by the host-side plan (csrc/denoise_plan.cpp
    through lib/denoise_driver), holds both the LDS-staged and the direct kernel."""
    for iterations in range(2, _lib.MRT_DENOISE_MAX_ITERATIONS + 1):
        head, steps = TD.plan(*FILTER_FRAME, iterations, 7, *FILTER_SIGMAS, 0)
        assert head[:2] == [0, iterations]      # MRT_OK, one launch per iteration
        if {s[1] for s in steps[:iterations]} == {0, 1}:
            return iterations
    raise AssertionError("no iteration count mixes the two kernels at this frame size")


@raw("mrt_denoise_filter", label="staged and direct")
@raw("mrt_denoise_filter", label="modulate only", iterations=0)
@wrapper("Denoiser.run")
def case_denoise_filter(iterations=None, wrapper=None):
    w, h = FILTER_FRAME
    n = w * h
    iterations = mixed_iterations() if iterations is None else iterations

    def inputs(seed):
        return dict(zip(("image", "guide", "albedo"), D.make_case(w, h, "mixed", seed=seed)))

    def call(b, s, ctx):
        if wrapper:
            from mrt.denoise import Denoiser
            d = Denoiser(b["image"].device)
            d._reserve(w, h)
            d.guide, d.albedo, d._have_frame = b["guide"], b["albedo"], True
            px, _ = d.run(b["image"], iterations=iterations, sigma_color=FILTER_SIGMAS[0], sigma_plane=FILTER_SIGMAS[1], stream=s)
            return {"pixels": px}
        q = _lib.DenoiseParams()
        q.width, q.height, q.iterations, q.normalSquarings = w, h, iterations, 7
        q.sigmaColor, q.sigmaPlane, q.variant = float(F(FILTER_SIGMAS[0])), float(F(FILTER_SIGMAS[1])), 0
        q.image, q.guide, q.albedo = p(b["image"]), p(b["guide"]), p(b["albedo"])
        q.scratch[0], q.scratch[1] = p(b["scratch0"]), p(b["scratch1"])
        q.imageOut, q.pixels = p(b["out"]), p(b["pixels"])
        _lib.check(lib().mrt_denoise_filter(C.byref(q), sp(s)))

    def twin(x):
        out, px = mrt.host.denoise_filter(x["image"], x["guide"], x["albedo"], w, h, iterations, *FILTER_SIGMAS, 7)
        return {"pixels": px} if wrapper else {"out": out, "pixels": px}
    # the two scratch images are outputs too: an early middle launch shows in them
    outs = {} if wrapper else {"out": ((n, 4), F), "pixels": ((n,), U32), "scratch0": ((n, 4), F), "scratch1": ((n, 4), F)}
    return S.Case(f"denoise_filter {iterations} iterations {wrapper or ''}", inputs(66), inputs(67), outs, call, twin)


@wrapper("Renderer.denoise")
def case_renderer_denoise(wrapper=None):
    """The renderer's two denoiser calls on one stream: features of its primary batch, then the filter."""
    normals, material = D.feature_tables()
    w, h = FEATURE_FRAME
    pixels = w * h

    def inputs(seed):
        return dict(feature_case_inputs(seed), image=D.make_image(pixels, np.random.default_rng(seed)))

    def prepare(dev, b):
        from mrt.raygen import RAY_PATH, DeviceReconstructor
        from mrt.renderer import Renderer
        from mrt.tracer import RayBuffer
        v, t, _ = U.edge_scene()
        r = Renderer(new_tracer(), mrt.Scene.from_arrays(v, t))
        r.set_params(RAY_PATH, 1)
        r.primary, r.slot_to_id, r.w, r.h = RayBuffer(b["rays"], results=b["results"]), b["s2i"], w, h
        r._recon = DeviceReconstructor(None)
        r._recon.material, r.gen.normals = S._upload(material, dev), S._upload(normals, dev)
        return r

    def call(b, s, r):
        px, _ = r.denoise(b["image"], sigma_plane=FILTER_SIGMAS[1], stream=s, iterations=2, sigma_color=FILTER_SIGMAS[0])
        return {"pixels": px}

    def twin(x):
        g, a = mrt.host.denoise_features(x["s2i"], x["rays"], x["results"], normals, material, pixels,
                                         np.zeros((pixels, 8), F), np.ones((pixels, 4), F))
        return {"pixels": mrt.host.denoise_filter(x["image"], g, a, w, h, 2, *FILTER_SIGMAS, 7)[1]}
    return S.Case("Renderer.denoise", inputs(1), inputs(2), {}, call, twin, prepare=prepare)


# ---- a moving scene ----------------------------------------------------------------------------------------------------
@raw("mrt_scene_attributes")
@wrapper("scene_attributes")
@wrapper("DeviceRayGen.set_geometry", kind="generator")
@wrapper("DeviceReconstructor.set_geometry", kind="reconstructor")
def case_scene_attributes(wrapper=None, kind=None):
    v, t, diffuse = SA.mixed_mesh()
    nt = len(t)
    real = {"vertices": v, "triangles": t, "diffuse": diffuse}
    decoy = {"vertices": (v * F(2.0) + F(0.25)).astype(F)[:, ::-1].copy(), "triangles": t.copy(), "diffuse": np.roll(diffuse, 1, axis=0)}
    if not wrapper:
        real["skipped"], decoy["skipped"] = np.zeros(1, np.int64), np.zeros(1, np.int64)

    def call(b, s, ctx):
        from mrt import raygen
        if wrapper == "scene_attributes":
            out = {"normals": torch.empty((nt, 3), device=b["vertices"].device),
                   "shaded": torch.empty(nt, dtype=torch.int32, device=b["vertices"].device)}
            raygen.scene_attributes(b["vertices"], b["triangles"], b["diffuse"], normals=out["normals"], shaded=out["shaded"], stream=s)
            return out
        if kind == "generator":
            g = raygen.DeviceRayGen()
            g.set_geometry(b["vertices"], b["triangles"], stream=s)
            return {"normals": g.normals}
        if wrapper:
            r = raygen.DeviceReconstructor(None)
            r.set_geometry(b["vertices"], b["triangles"], b["diffuse"], stream=s)
            return {"shaded": r.shaded, "material": r.material}
        _lib.check(lib().mrt_scene_attributes(p(b["vertices"]), len(v), p(b["triangles"]), nt, p(b["diffuse"]), p(b["normals"]),
                                              p(b["shaded"]), p(b["material"]), p(b["skipped"]), sp(s)))

    def twin(x):
        out = mrt.host.scene_attributes(x["vertices"], x["triangles"], x["diffuse"])
        out["skipped"] = np.array([out["skipped"]], np.int64)
        assert out["skipped"][0] > 0
        return out

    def same(got, want):
        return S.same_outputs(got, {k: want[k] for k in want if k in got})
    outs = {} if wrapper else {"normals": ((nt, 3), F), "shaded": ((nt,), U32), "material": ((nt,), U32)}
    return S.Case(f"scene_attributes {wrapper or ''}", real, decoy, outs, call, twin, same=same,
                  distinct=lambda a, b: S.same_outputs(a, b) != "", inout=() if wrapper else ("skipped",))


@wrapper("Renderer.set_vertices")
def case_set_vertices(wrapper=None):
    """Refit, normals and colours of moved vertices, all behind one stream= argument."""
    w = tree_world()
    start = w["refit0"]

    def prepare(dev, b):
        from mrt.renderer import Renderer
        t = bind(dev, b)
        r = Renderer(t, mrt.Scene.synthetic("random", 1500, 1))
        r.set_vertices(S._upload(w["v"], dev))      # the plan-building first refit, and the uploads of the scene
        return r

    def call(b, s, r):
        assert r.set_vertices(b["vertices"], stream=s) == {"rebuilt": False, "sah": None, "ratio": None}
        return {"normals": r.gen.normals, "shaded": r._recon.shaded, "material": r._recon.material}

    def twin(x):
        nodes, woop, _ = R.host_refit(w["bufs"], x["vertices"], w["t"])
        attr = mrt.host.scene_attributes(x["vertices"], w["t"], mrt.Scene.synthetic("random", 1500, 1).tri_diffuse())
        return {"nodes": nodes, "woop": woop, "normals": attr["normals"], "shaded": attr["shaded"], "material": attr["material"]}

    def same(got, want):
        return same_tree(got, want) or S.same_outputs(got, {k: want[k] for k in ("normals", "shaded", "material")})
    real = {"vertices": w["moved"], "nodes": start[0], "woop": start[1], "tri": start[2]}
    return S.Case("Renderer.set_vertices", real, dict(real, vertices=w["v"]), {}, call, twin, same=same,
                  inout=("nodes", "woop"), prepare=prepare)


# ---- the tests ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    S.calibrate(device)
    t0 = time.perf_counter()
    yield device
    torch.cuda.synchronize()
    stalls = [x for _, _, u in S.LOG for x in u] or [0.0]
    print(f"\nstream order: {len(S.LOG)} cases in {time.perf_counter() - t0:.1f} s; {S._RATE[str(device)]:.0f} sleep cycles per ms; "
          f"stalls {min(stalls):.2f} .. {max(stalls):.2f} ms, {sum(stalls):.0f} ms in all; "
          f"repeated with four times the stall: {[n for n, _, u in S.LOG if len(u) > 1]}")


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
def test_stream_argument_alone_orders_the_wrapper(dev, streams, method, label, build):
    """stream=s while torch's current stream is the default one: the launches, what the method allocates
    and what it reads back to the host (count_hits, extend's live count) are all ordered on s."""
    assert torch.cuda.current_stream().cuda_stream != streams[0].cuda_stream
    S.run(build(), dev, streams)


def test_control_a_null_stream_launch_is_noticed(dev, streams):
    """The protocol can fail: mrt_scene_attributes (one launch, no scratch, every index range-checked)
    called on the NULL stream while its inputs are gated on the stalled stream writes its outputs
    before the stall ends, and they are the decoy's. The decoy is valid input: nothing faults."""
    r = S.run(case_scene_attributes(), dev, streams, control=True)
    assert set(r.early) >= {"normals", "shaded", "material"}
    print(f"control: written while stalled {r.early}; the result is the decoy's")


def case_chain():
    """refit, trace, shadow rays, trace, lit reconstruction: five exports on one stream, nothing
    synchronised in between, each reading what its predecessor wrote."""
    w = tree_world()
    start, tri = w["refit0"], w["bufs"][2]
    n, samples, seed = len(w["rays"]), 2, 11
    lo, hi = w["v"].min(0), w["v"].max(0)
    light = tuple(float(x) for x in (lo + (hi - lo) * np.array([0.5, 0.9, 0.9], F)).astype(F))
    radius = float(F(0.1 * np.linalg.norm(hi - lo)))
    rng = np.random.default_rng(17)
    num_pixels = n + 7
    s2i = rng.permutation(num_pixels)[:n].astype(I32)
    material = rng.integers(0, 1 << 32, len(w["t"]), dtype=np.uint64).astype(U32)
    normals = mrt.host.scene_attributes(w["moved"], w["t"], shaded=False, material=False)["normals"]

    def prepare(dev, b):
        t = bind(dev, b)
        tris = S._upload(w["t"], dev)
        t.refit(S._upload(w["v"], dev), tris)
        return {"t": t, "tris": tris, "s2i": S._upload(s2i, dev), "material": S._upload(material, dev),
                "normals": S._upload(normals, dev)}

    def call(b, s, ctx):
        h, q = ctx["t"]._h, sp(s)
        _lib.check(lib().mrt_tracer_refit(h, p(b["vertices"]), len(w["v"]), p(ctx["tris"]), len(w["t"]), q))
        _lib.check(lib().mrt_tracer_trace(h, p(b["primary"]), p(b["primary_results"]), n, EXACT_PER_LANE, None, q))
        _lib.check(lib().mrt_raygen_shadow(p(b["primary"]), p(b["primary_results"]), n, samples, light3(light), radius, seed,
                                           p(b["shadow"]), None, None, q))
        _lib.check(lib().mrt_tracer_trace(h, p(b["shadow"]), p(b["shadow_results"]), n * samples,
                                          EXACT_PER_LANE | _lib.MRT_TRACE_ANY_HIT, None, q))
        _lib.check(lib().mrt_reconstruct_lit(samples, 0, n, p(ctx["s2i"]), p(b["primary"]), p(b["primary_results"]), None,
                                             p(b["shadow_results"]), p(ctx["normals"]), p(ctx["material"]), light3(light),
                                             p(b["pixels"]), q))

    def twin(x):
        nodes, woop, _ = R.host_refit(w["bufs"], x["vertices"], w["t"])
        pres = O.trace(x["primary"], nodes, woop, tri)[0]
        shadow = mrt.host.shadow_rays(x["primary"], pres, samples, light, radius, seed=seed)
        sres = O.trace(shadow, nodes, woop, tri, any_hit=True)[0]
        pixels = mrt.host.reconstruct_lit(samples, s2i, x["primary"], pres, sres, normals, material, light, num_pixels,
                                          pixels=sentinel(num_pixels, U32))
        return {"nodes": nodes, "woop": woop, "primary_results": np.ascontiguousarray(pres[:, :2]).view(I32), "shadow": shadow,
                "shadow_results": np.ascontiguousarray(sres[:, :2]).view(I32), "pixels": pixels}

    def same(got, want):
        msg = same_tree(got, want)
        for k in ("primary_results", "shadow_results"):
            msg = msg or same_results({"results": got[k]}, {"results": want[k]}).replace("results", k)
        return msg or S.same_outputs(got, {k: want[k] for k in ("shadow", "pixels")})
    real = {"vertices": w["moved"], "primary": w["rays_moved"], "nodes": start[0], "woop": start[1], "tri": start[2]}
    decoy = dict(real, vertices=w["v"], primary=rev(w["rays"]))
    outs = {"primary_results": ((n, 4), I32), "shadow": ((n * samples, 8), F), "shadow_results": ((n * samples, 4), I32),
            "pixels": ((num_pixels,), U32)}
    def misses(count):   # a result a later launch indexes a table by starts as a miss, its pad words as the sentinel
        rows = sentinel((count, 4), I32)
        rows[:, 0], rows[:, 1] = -1, 0
        return rows
    return S.Case("chain", real, decoy, outs, call, twin, same=same, inout=("nodes", "woop"), prepare=prepare,
                  fill={"primary_results": misses(n), "shadow_results": misses(n * samples)})


def test_chain_of_five_exports_on_one_stalled_stream(dev, streams):
    case = case_chain()
    want, _ = case.want()
    lit = want["pixels"][want["pixels"] != sentinel(1, U32)[0]]
    assert (want["primary_results"][:, 0] != -1).any() and (want["shadow_results"][:, 0] == -1).any() and len(np.unique(lit)) > 8
    S.run(case, dev, streams)
