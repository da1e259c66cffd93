"""The stream-order protocol of tests/test_gpu_stream_order.py.

Every export of include/mrt.h that takes a `void* stream` promises that its launches run on that
stream, most also that the call does not wait on the host. A test on an idle stream cannot tell: a
launch that went to the NULL stream would still find its inputs. Here the stream is stalled first:

  setup     the device input buffers hold a DECOY (valid inputs of the same shapes whose host-twin
            result differs from the real one, asserted on the CPU), the real inputs wait in staging
            tensors, every output is filled with a sentinel byte, the device is synchronised;
  enqueue   on a side stream s that is not torch's current stream: a stall (torch.cuda._sleep),
            device-to-device copies of the staging tensors over the input buffers, the export;
  stalled   a second side stream copies every output to the host: all sentinel (nothing ran early),
            and then s is still busy (the call returned without waiting, and the stall covered the
            whole window);
  after     s is synchronised: the outputs equal the host twin of the REAL inputs, the inputs are
            unchanged.

A launch on another stream reads the decoy, or writes before the stall ends; either shows. Blocking
exports skip the middle step: they wait the stall out themselves, and their inputs are still gated.

The stall is not a threshold. It is 20 times the host wall time of the enqueue and the snapshot in
an unstalled dry run of the same case (which is also the plain side-stream run), four times that
once more where s had already finished, never above 2 s; inconclusive twice is a failure.
"""
import time

import numpy as np

import frame_util as U

SENTINEL = 0xA5
MAX_STALL_MS = 2000.0
STALL_FACTOR, RETRY_FACTOR = 20.0, 4.0
F = np.float32


class Case:
    """One call of one export, host side only (no device is touched before run()).

    real, decoy  name -> numpy array: what the export's device input buffers hold (same shapes).
    outs         name -> (shape, numpy dtype): device output buffers, sentinel-filled.
    inout        names of real / decoy that the export also writes (radiance, a bound tree's nodes):
                 real and decoy hold the same start value there; while stalled they must still hold
                 what they held before the enqueue.
    twin(inputs) -> the expected outputs (any form `same` understands) of a dict like real / decoy.
    same(got, want) -> "" or what differs; got: name -> numpy array of every out and inout buffer
                 plus what collect() adds.
    distinct(a, b) -> whether two twin results differ (default: same(a, b) != "").
    prepare(dev, buffers) -> ctx: binds handles and the like on the current stream, before the
                 synchronise; buffers: name -> device tensor (inputs, holding the decoy, and outputs).
    call(buffers, stream, ctx): the export, on the torch stream given (None: the NULL stream); raises
                 where it fails. A wrapper's call returns name -> tensor or host value of what the
                 method allocated and returned; these join `got` after the stream is synchronised.
    collect(ctx) -> name -> numpy array: results that are not device buffers (a host struct).
    finish(ctx): releases what prepare took.
    blocking     the export waits for the device by design.
    fill         name -> numpy array: what an output holds at the start instead of the sentinel bytes,
                 for an output that a later launch of the same call indexes by (a chain's results):
                 valid values, so that even a misordered launch addresses nothing out of range.
    rewritten    names of real / decoy that a blocking export rewrites from their gated contents (the
                 nodes mrt_tracer_optimize restructures): left out of the inputs-unchanged check.
    """

    def __init__(self, name, real, decoy, outs, call, twin, same=None, distinct=None, inout=(), prepare=None,
                 collect=None, finish=None, blocking=False, rewritten=(), fill=None):
        assert set(real) == set(decoy) and set(inout) <= set(real) and not set(outs) & set(real), name
        for k in real:
            real[k], decoy[k] = np.ascontiguousarray(real[k]), np.ascontiguousarray(decoy[k])
            assert real[k].shape == decoy[k].shape and real[k].dtype == decoy[k].dtype, (name, k)
            if k in inout:
                assert real[k].tobytes() == decoy[k].tobytes(), (name, k)
        self.name, self.real, self.decoy, self.outs, self.inout = name, real, decoy, dict(outs), tuple(inout)
        self.call, self.twin, self.same = call, twin, same if same is not None else same_outputs
        self.distinct = distinct if distinct is not None else (lambda a, b: self.same(a, b) != "")
        self.prepare, self.collect, self.finish, self.blocking = prepare, collect, finish, blocking
        self.rewritten = tuple(rewritten)
        self.fill = {k: np.ascontiguousarray(v) for k, v in (fill or {}).items()}
        assert set(self.fill) <= set(self.outs), name
        self._want = None

    def want(self):
        """(twin of the real inputs, twin of the decoy), once; the two must differ."""
        if self._want is None:
            real = self.twin({k: v.copy() for k, v in self.real.items()})
            decoy = self.twin({k: v.copy() for k, v in self.decoy.items()})
            assert any(self.real[k].tobytes() != self.decoy[k].tobytes() for k in self.real), f"{self.name}: the decoy is the input"
            assert self.distinct(real, decoy), f"{self.name}: the decoy's result is the real one"
            self._want = (real, decoy)
        return self._want


def same_outputs(got, want):
    """Every array of want against got's: float32 as bits with a NaN equal to a NaN (the bits of a
    NaN an operation makes differ between x86 and gfx950), anything else exactly."""
    for k, w in want.items():
        g, w = np.asarray(got[k]), np.asarray(w)
        if g.shape != w.shape:
            return f"{k}: shape {g.shape} != {w.shape}"
        if w.dtype == F:
            ok = U.same_bits_or_nan(g.view(F), w)
        elif g.dtype.itemsize == w.dtype.itemsize:
            ok = np.ascontiguousarray(g).view(w.dtype) == w     # torch has no uint32: the bits
        else:
            ok = g.astype(np.int64) == w.astype(np.int64)
        if not np.all(ok):
            return f"{k}: {int(np.size(ok) - np.count_nonzero(ok))} of {np.size(ok)} entries differ, first at {np.argwhere(~np.asarray(ok))[:3].tolist()}"
    return ""


# ---- the stall --------------------------------------------------------------------------------------
_RATE = {}


def calibrate(dev):
    """_sleep cycles per millisecond on dev, timed with events over a fixed sleep (no clock rate is
    assumed); measured once per process and device."""
    import torch
    key = str(dev)
    if key not in _RATE:
        cycles = 20_000_000
        torch.cuda._sleep(1000)     # the first launch loads the kernel
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        assert ms > 0.05, f"a sleep of {cycles} cycles took {ms} ms"
        _RATE[key] = cycles / ms
        print(f"stream_util: {_RATE[key]:.0f} sleep cycles per ms ({cycles} cycles in {ms:.3f} ms)")
    return _RATE[key]


# ---- one run ------------------------------------------------------------------------------------------
def _torch_dtype(dt):
    import torch
    return {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32, np.dtype(np.uint32): torch.int32,
            np.dtype(np.int64): torch.int64, np.dtype(np.float64): torch.float64, np.dtype(np.uint8): torch.uint8}[np.dtype(dt)]


def _upload(a, dev):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to(dev)


def _host(t):
    return t.cpu().numpy()


def scrub(dev, streams):
    """Fills the caching allocator's free blocks with the sentinel, on torch's current stream and on
    each of `streams` (the allocator keeps a pool per stream). A tensor that a wrapper allocates in the
    stalled run would otherwise come back holding what the dry run left in the same block: the right
    answer, which a readback that does not wait for the work would then return by accident."""
    import torch
    for s in (None,) + tuple(streams):
        with torch.cuda.stream(s) if s is not None else _nothing():
            held = [torch.full((size // 4,), -0x5A5A5A5B, dtype=torch.int32, device=dev)
                    for size in (512 << k for k in range(15)) for _ in range(4)]     # 512 B .. 8 MiB
            del held
    torch.cuda.synchronize()


class _nothing:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


class Round:
    """What one enqueue left behind."""


def run_once(case, dev, streams, cycles, null_stream=False):
    """Steps 3 to 13 once, with a stall of `cycles` (0: the dry run). Returns a Round: wall_ms (host
    time of the enqueue and the snapshot), still (s was busy after the snapshot; None where the export
    blocks), early (what the snapshot found written), got (the final buffers), inputs (the final
    input buffers)."""
    import torch
    s, side = streams
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream and s.cuda_stream != 0
    buf = {k: _upload(v, dev) for k, v in case.decoy.items()}
    staging = {k: _upload(v, dev) for k, v in case.real.items()}
    for k, (shape, dt) in case.outs.items():
        if k in case.fill:
            buf[k] = _upload(case.fill[k], dev)
            assert tuple(buf[k].shape) == tuple(shape), k
            continue
        t = torch.empty(shape, dtype=_torch_dtype(dt), device=dev)
        t.view(torch.uint8).fill_(SENTINEL)
        buf[k] = t
    ctx = case.prepare(dev, buf) if case.prepare else None
    watched = list(case.outs) + list(case.inout)
    pinned = {k: torch.empty(buf[k].shape, dtype=buf[k].dtype, pin_memory=True) for k in watched}
    torch.cuda.synchronize()
    before = {k: _host(buf[k]) for k in case.inout}
    scrub(dev, streams)
    r = Round()
    try:
        t0 = time.perf_counter()
        with torch.cuda.stream(s):
            if cycles:
                torch.cuda._sleep(int(cycles))
            for k, v in staging.items():
                buf[k].copy_(v, non_blocking=True)
        ret = case.call(buf, None if null_stream else s, ctx)   # torch's current stream is not s here
        r.still, r.early = None, []
        if not case.blocking:
            with torch.cuda.stream(side):
                for k in watched:
                    pinned[k].copy_(buf[k], non_blocking=True)
            side.synchronize()
            r.still = not s.query()
        r.wall_ms = (time.perf_counter() - t0) * 1e3
        if not case.blocking:
            for k in case.outs:
                if k in case.fill:
                    untouched = pinned[k].numpy().tobytes() == case.fill[k].tobytes()
                else:
                    untouched = bool((pinned[k].view(torch.uint8) == SENTINEL).all())
                if not untouched:
                    r.early.append(k)
            for k in case.inout:
                if pinned[k].numpy().tobytes() != before[k].tobytes():
                    r.early.append(k)
        s.synchronize()
        if null_stream:
            torch.cuda.synchronize()
        r.got = {k: _host(buf[k]) for k in watched}
        for k, v in (ret or {}).items():     # what a wrapper allocated and returned
            r.got[k] = _host(v) if isinstance(v, torch.Tensor) else np.asarray(v)
        r.inputs = {k: _host(buf[k]) for k in case.real if k not in case.inout and k not in case.rewritten}
        if case.collect:
            r.got.update(case.collect(ctx))
    finally:
        torch.cuda.synchronize()
        if case.finish:
            case.finish(ctx)
    return r


def inputs_unchanged(case, r):
    for k, v in r.inputs.items():
        assert v.tobytes() == case.real[k].tobytes(), f"{case.name}: the input buffer {k} does not hold the real input"


LOG = []    # (case, dry wall ms, stalls used in ms): printed, and collected for the summary


def run(case, dev, streams, control=False):
    """The whole protocol for one case. control: the export is called on the NULL stream on purpose,
    and the protocol must notice: outputs written while s is stalled, and the decoy's result."""
    rate = calibrate(dev)
    want_real, want_decoy = case.want()
    dry = run_once(case, dev, streams, 0)
    msg = case.same(dry.got, want_real)
    assert msg == "", f"{case.name}: the plain side-stream run differs from the host twin: {msg}"
    inputs_unchanged(case, dry)
    stall_ms, used = min(MAX_STALL_MS, STALL_FACTOR * dry.wall_ms), []
    for attempt in range(2):
        used.append(stall_ms)
        r = run_once(case, dev, streams, stall_ms * rate, null_stream=control)
        if case.blocking or r.still:
            break
        stall_ms = min(MAX_STALL_MS, RETRY_FACTOR * stall_ms)
    LOG.append((case.name, dry.wall_ms, used))
    print(f"stream_util: {case.name}: dry run {dry.wall_ms:.3f} ms on the host, stalls {[round(x, 2) for x in used]} ms"
          f"{' (blocking)' if case.blocking else ''}{' (control)' if control else ''}")
    if not case.blocking:
        assert r.still, f"{case.name}: inconclusive twice: the stream had finished a {used[-1]:.1f} ms stall after the snapshot " \
                        f"(the call or the snapshot waited; enqueue and snapshot took {r.wall_ms:.1f} ms)"
    if control:
        assert r.early, f"{case.name}: called on the NULL stream, yet nothing was written while the stream was stalled"
        # an in-out buffer is gated like an input: the staging copy, which runs after the stall, has
        # overwritten what the early launch added to it
        r.got = {k: v for k, v in r.got.items() if k not in case.inout}
        msg = case.same(r.got, want_decoy)
        assert msg == "", f"{case.name}: called on the NULL stream, the result is not the decoy's: {msg}"
        assert case.same(r.got, want_real) != ""
        inputs_unchanged(case, r)
        return r
    assert not r.early, f"{case.name}: written while the stream was stalled: {r.early}"
    msg = case.same(r.got, want_real)
    if msg:
        decoy = case.same(r.got, want_decoy) == ""
        raise AssertionError(f"{case.name}: after the stall the result differs from the host twin of the real inputs"
                             f"{' (it is the decoy result: a launch read its inputs early)' if decoy else ''}: {msg}")
    inputs_unchanged(case, r)
    return r
