"""mrt_scene_attributes (csrc/scene_kernel.hip) against its CPU statement, mrth_scene_attributes:
bit for bit at 1, 63, 64, 65 triangles, at the kernel's workgroup size and one either side, and
on random(1500) with the hand-made edge triangles mixed in (zero-area, collinear, out-of-range
indices, NaN, infinite, overflowing and denormal coordinates) and per-triangle diffuse colours.

No input is left out on account of the denormal mode: this part of the library is built without
denormal flushing (include/mrt.h), and the edge triangles include denormal edges. Normals are
compared as bits with a NaN equal to any NaN — the bits of a NaN an operation makes differ between
x86 and gfx950, which is no arithmetic difference; the colours are integers and compared exactly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mrt  # noqa: E402
import mrt.host  # noqa: E402
from mrt import _lib  # noqa: E402
from mrt.raygen import scene_attributes  # noqa: E402

import scene_attr_util as U  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def kernel_constant(name):
    text = open(os.path.join(REPO, "gpu-ray-tracing_amd", "csrc", "scene_kernel.hpp")).read()
    return int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))


BLOCK = kernel_constant("kSceneBlock")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def mixed():
    v, t, d = U.mixed_mesh(1500)
    return v, t, d, mrt.host.scene_attributes(v, t, d)


def run(dev, v, t, d=None, which=("normals", "shaded", "material"), skipped=None, out=None, stream=None):
    """The device call over uploaded arrays; returns the outputs asked for as numpy arrays."""
    tv, tt = torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev)
    td = None if d is None else torch.from_numpy(d).to(dev)
    nt = len(t)
    out = out if out is not None else {
        "normals": torch.full((nt, 3), 7.0, dtype=torch.float32, device=dev),
        "shaded": torch.full((nt,), 0x55, dtype=torch.int32, device=dev),
        "material": torch.full((nt,), 0x55, dtype=torch.int32, device=dev)}
    scene_attributes(tv, tt, td, **{k: out[k] for k in which}, skipped=skipped, stream=stream)
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in out}


def assert_same(got, want, which=("normals", "shaded", "material"), what=""):
    if "normals" in which:
        assert U.same_bits_or_nan(got["normals"], want["normals"]), what
    for k in ("shaded", "material"):
        if k in which:
            assert np.array_equal(got[k].view(np.uint32), want[k]), (what, k)


@pytest.mark.parametrize("count", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1])
def test_equals_the_host_twin_at_the_wave_and_workgroup_edges(dev, mixed, count):
    v, t, d, _ = mixed
    t, d = t[:count], d[:count]
    got = run(dev, v, t, d)
    assert_same(got, mrt.host.scene_attributes(v, t, d), what=f"{count} triangles")


def test_equals_the_host_twin_on_random_with_the_edge_triangles(dev, mixed):
    v, t, d, want = mixed
    assert want["skipped"] == 2 and np.isnan(want["normals"]).any()
    skipped = torch.zeros(1, dtype=torch.int64, device=dev)
    got = run(dev, v, t, d, skipped=skipped)
    assert_same(got, want)
    assert int(skipped.item()) == 2
    # the default material
    assert_same(run(dev, v, t, None), mrt.host.scene_attributes(v, t, None), what="default material")


@pytest.mark.parametrize("which", [("normals",), ("shaded",), ("material",), ("shaded", "material"), ("normals", "material")])
def test_each_optional_output_may_be_null(dev, mixed, which):
    v, t, d, want = mixed
    got = run(dev, v, t, d, which=which)
    assert_same(got, want, which)
    for k in {"normals", "shaded", "material"} - set(which):      # untouched
        assert (got[k] == (7.0 if k == "normals" else 0x55)).all()


def test_skipped_is_added_to_not_overwritten(dev):
    v, t, _ = U.edge_mesh()
    skipped = torch.full((1,), 40, dtype=torch.int64, device=dev)
    run(dev, v, t, skipped=skipped)
    assert int(skipped.item()) == 42
    run(dev, v, t, skipped=skipped)
    assert int(skipped.item()) == 44
    # every triangle of three waves and a bit skipped: one count per triangle, whatever the wave
    bad = np.full((200, 3), -5, np.int32)
    run(dev, v, bad, skipped=skipped)
    assert int(skipped.item()) == 244


def test_outputs_written_in_place_over_a_previous_call(dev, mixed):
    v, t, d, want = mixed
    nt = len(t)
    out = {"normals": torch.empty((nt, 3), dtype=torch.float32, device=dev),
           "shaded": torch.empty(nt, dtype=torch.int32, device=dev), "material": torch.empty(nt, dtype=torch.int32, device=dev)}
    moved = (v + F(0.25)).astype(F)[::-1].copy()       # other vertices behind every index
    first = run(dev, moved, t, None, out=out)
    assert not np.array_equal(first["shaded"].view(np.uint32), want["shaded"])
    ptrs = [out[k].data_ptr() for k in out]
    got = run(dev, v, t, d, out=out)
    assert ptrs == [out[k].data_ptr() for k in out]
    assert_same(got, want)


def test_stream_ordered_on_a_side_stream(dev, mixed):
    v, t, d, want = mixed
    s = torch.cuda.Stream(device=dev)
    got = run(dev, v, t, d, stream=s)
    assert_same(got, want)


def test_zero_triangles_launch_nothing_and_bad_arguments_are_refused(dev):
    lib = _lib.trace_lib()
    v = torch.zeros((3, 3), dtype=torch.float32, device=dev)
    n = torch.full((4, 3), 7.0, dtype=torch.float32, device=dev)
    assert lib.mrt_scene_attributes(v.data_ptr(), 3, None, 0, None, n.data_ptr(), None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (n.cpu().numpy() == 7.0).all()
    t = torch.zeros((1, 3), dtype=torch.int32, device=dev)
    assert lib.mrt_scene_attributes(v.data_ptr(), 3, t.data_ptr(), 1, None, None, None, None, None, None) == _lib.MRT_ERR_INVALID_ARG
    assert lib.mrt_scene_attributes(v.data_ptr(), 3, t.data_ptr(), -1, None, n.data_ptr(), None, None, None, None) == _lib.MRT_ERR_INVALID_ARG
    assert lib.mrt_scene_attributes(v.data_ptr(), 3, t.data_ptr(), 1 << 26, None, n.data_ptr(), None, None, None, None) == _lib.MRT_ERR_TOO_LARGE
    torch.cuda.synchronize()
    assert (n.cpu().numpy() == 7.0).all()
    # no vertices at all: every triangle is skipped, none read
    skipped = torch.zeros(1, dtype=torch.int64, device=dev)
    assert lib.mrt_scene_attributes(v.data_ptr(), 0, t.data_ptr(), 1, None, n.data_ptr(), None, None, skipped.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert int(skipped.item()) == 1 and (n[0].cpu().numpy() == 0).all() and (n[1:].cpu().numpy() == 7.0).all()
