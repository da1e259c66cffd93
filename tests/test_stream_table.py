"""The tables of tests/test_gpu_stream_order.py are complete, checked without a device: its raw rows
are exactly the exports of include/mrt.h whose parameter list has a `void* stream` (parsed from the
header text), its wrapper rows exactly the functions and methods of mrt/*.py that take `stream`
(found with inspect). An export or a method added later cannot arrive without a stream-order test.
The host half of every row runs here too: each case's decoy is valid input of the same shapes whose
host-twin result differs from the real one."""
import importlib
import inspect
import os
import pkgutil
import re

import pytest

pytest.importorskip("torch")

import mrt  # noqa: E402
import test_gpu_stream_order as G  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mrt.h")


def stream_exports():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    found, every = set(), set()
    for m in re.finditer(r"\b(\w+)\s*\(([^(){};]*)\)\s*;", text):
        name, params = m.group(1), [" ".join(q.split()) for q in m.group(2).split(",")]
        every.add(name)
        if any(re.fullmatch(r"void\s*\*\s*stream", q) for q in params):
            found.add(name)
    return found, every


def test_the_header_is_parsed():
    found, every = stream_exports()
    assert {"mrt_tracer_create", "mrt_version", "mrt_refit_plan", "launch_tracingKernel"} <= every
    assert {"mrt_tracer_trace", "mrt_ray_sort", "mrt_path_extend", "mrt_trace"} <= found
    assert not {"mrt_tracer_bind", "mrt_tracer_refit_info", "mrt_selftest_exact_rcp"} & found


def test_every_stream_taking_export_has_a_row_and_every_row_is_one():
    found, _ = stream_exports()
    rows = {export for export, _, _ in G.RAW}
    assert rows == found, f"without a row: {sorted(found - rows)}; rows that are no stream-taking export: {sorted(rows - found)}"


def stream_methods():
    """'Class.method' and 'function' of everything defined in mrt/*.py with a parameter named stream."""
    out = set()
    for info in pkgutil.iter_modules(mrt.__path__):
        mod = importlib.import_module(f"mrt.{info.name}")
        for name, obj in vars(mod).items():
            if getattr(obj, "__module__", None) != mod.__name__ or name.startswith("_"):
                continue      # imported names, and the package's own helpers (_stream_ptr, _on_stream)
            if inspect.isfunction(obj) and "stream" in inspect.signature(obj).parameters:
                out.add(name)
            if inspect.isclass(obj):
                for attr, fn in vars(obj).items():
                    if inspect.isfunction(fn) and "stream" in inspect.signature(fn).parameters:
                        out.add(f"{name}.{attr}")
    return out


def test_every_stream_method_of_the_package_has_a_row_and_every_row_is_one():
    found = stream_methods()
    assert {"DeviceRayGen.count_hits", "PathIntegrator.extend", "Denoiser.run", "Tracer.refit"} <= found
    rows = {method for method, _, _ in G.WRAPPERS}
    assert rows == found, f"without a row: {sorted(found - rows)}; rows that are no stream= method: {sorted(rows - found)}"


def test_the_documented_blocking_exports_are_the_blocking_rows():
    blocking = {export for export, _, build in G.RAW if build().blocking}
    assert blocking == {"mrt_tracer_build", "mrt_tracer_bind_device", "mrt_tracer_build_device", "mrt_tracer_optimize",
                        "mrt_tracer_trace_timed", "mrt_trace", "mrt_tracer_tree_cost"}
    # mrt_tracer_tree_cost blocks with a host output only: its device-output row does not
    assert any(not build().blocking for export, _, build in G.RAW if export == "mrt_tracer_tree_cost")


CASES = [(f"{name}-{label}", build) for name, label, build in G.RAW + G.WRAPPERS] + [("chain", G.case_chain)]


@pytest.mark.parametrize("name,build", CASES, ids=[name.rstrip("-").replace(" ", "_") for name, _ in CASES])
def test_the_decoy_is_valid_input_with_another_result(name, build):
    case = build()
    real, decoy = case.want()      # asserts that the inputs and the twins' results differ
    assert not case.distinct(real, real) and not case.distinct(decoy, decoy)    # and the comparison can say "equal"
    for k, a in case.real.items():
        assert a.shape == case.decoy[k].shape and a.dtype == case.decoy[k].dtype, k


def test_the_filter_row_mixes_the_two_kernels_by_the_plan():
    import test_denoise as TD
    it = G.mixed_iterations()
    head, steps = TD.plan(*G.FILTER_FRAME, it, 7, *G.FILTER_SIGMAS, 0)
    assert head[1] == it and {s[1] for s in steps[:it]} == {0, 1}
    _, fewer = TD.plan(*G.FILTER_FRAME, it - 1, 7, *G.FILTER_SIGMAS, 0)
    assert len({s[1] for s in fewer[:it - 1]}) == 1, "a smaller iteration count mixes them too"
    print(f"65 x 9: {it} iterations, staged flags {[s[1] for s in steps[:it]]}")
