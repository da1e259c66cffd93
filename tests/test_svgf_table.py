"""The tables of tests/test_gpu_svgf_stream.py are complete, checked without a device: its raw rows
are exactly the exports of include/mrt_svgf.h, each of which takes a `void* stream` last (parsed from
the header text, as tests/test_stream_table.py parses mrt.h), its wrapper rows exactly the public
functions and methods of mrt.svgf plus Renderer.svgf. None of those callables takes a `stream`
(tests/test_stream_table.py's table of stream= methods is closed): they run on torch's current
stream and say so. The host half of every row runs here too: each case's decoy is valid input of
the same shapes whose host-twin result differs from the real one."""
import inspect
import os
import re

import pytest

pytest.importorskip("torch")

import mrt.svgf  # noqa: E402
from mrt.renderer import Renderer  # noqa: E402
import test_gpu_svgf_stream as G  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mrt_svgf.h")


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


def test_the_header_is_parsed_and_every_export_takes_the_stream_last():
    found, every = stream_exports()
    assert found == every == {"mrt_svgf_accumulate", "mrt_svgf_filter"}
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for name in found:
        params = re.search(r"\b" + name + r"\s*\(([^(){};]*)\)\s*;", text).group(1).split(",")
        assert re.fullmatch(r"void\s*\*\s*stream", " ".join(params[-1].split())), name


def test_every_stream_taking_export_has_a_row_and_every_row_is_one():
    found, _ = stream_exports()
    rows = {export for export, _, _ in G.RAW}
    assert rows == found, f"without a row: {sorted(found - rows)}; rows that are no stream-taking export: {sorted(rows - found)}"


def public_callables():
    """'Class.method' and 'function' of everything public defined in mrt/svgf.py, with Renderer.svgf."""
    mod = mrt.svgf
    out = {"Renderer.svgf": Renderer.svgf}
    for name, obj in vars(mod).items():
        if getattr(obj, "__module__", None) != mod.__name__ or name.startswith("_"):
            continue
        if inspect.isfunction(obj):
            out[name] = obj
        if inspect.isclass(obj):
            for attr, fn in vars(obj).items():
                if inspect.isfunction(fn) and not attr.startswith("_"):
                    out[f"{name}.{attr}"] = fn
    return out


def test_every_public_callable_has_a_row_and_every_row_is_one():
    found = public_callables()
    assert {"SvgfAccumulator.filter", "Renderer.svgf"} <= set(found)
    rows = {method for method, _, _ in G.WRAPPERS}
    assert rows == set(found), f"without a row: {sorted(set(found) - rows)}; rows that are no public callable: {sorted(rows - set(found))}"


def test_no_callable_takes_a_stream_and_each_says_where_it_runs():
    for name, fn in public_callables().items():
        assert "stream" not in inspect.signature(fn).parameters, name
        assert "torch.cuda.stream(s)" in fn.__doc__, name
    assert "torch.cuda.stream(s)" in mrt.svgf.__doc__


def test_the_temporal_names_are_unchanged():
    """mrt.svgf subclasses TemporalAccumulator through private hooks: mrt.temporal's public names are what they were."""
    import mrt.temporal
    from mrt.temporal import TemporalAccumulator
    assert sorted(k for k in vars(TemporalAccumulator) if not k.startswith("_")) == ["accumulate", "current", "history_length", "reset"]
    assert sorted(k for k, v in vars(mrt.temporal).items() if getattr(v, "__module__", None) == "mrt.temporal") == \
        ["TemporalAccumulator", "world_to_screen"]


CASES = [(f"{name}-{label}", build) for name, label, build in G.RAW + G.WRAPPERS]


@pytest.mark.parametrize("name,build", CASES, ids=[name.rstrip("-").replace(" ", "_") for name, _ in CASES])
def test_the_decoy_is_valid_input_with_another_result(name, build):
    case = build()
    real, decoy = case.want()      # asserts that the inputs and the twins' results differ
    assert not case.distinct(real, real) and not case.distinct(decoy, decoy)    # and the comparison can say "equal"
    for k, a in case.real.items():
        assert a.shape == case.decoy[k].shape and a.dtype == case.decoy[k].dtype, k
