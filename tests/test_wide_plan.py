"""The device derivation's level scheme on the CPU: the refit plan and the exact 4-wide array as
csrc/wide_kernel.hip derives them, level by level, run sequentially by lib/wide_plan_driver
(tests/cpp/wide_plan_driver.cpp, host compiler only) through the same per-node steps
(csrc/wide_common.hpp) the kernels call.

  * on every valid tree the driver's order, level offsets, wide array, source map and stack bound
    equal mrt_refit_plan's and mrt_derive_wide_nodes' (form 1, leaf counts included) bit for bit,
    whichever way a level's nodes are walked; the stack bound equals a walk of the host's array;
  * a tree that is none (a ref past the array, a ref that is no multiple of 4, a record reached
    twice, a cycle back to an ancestor, an unreachable record) is refused with refit_levels'
    reason, and the walk ends (the driver runs under a timeout);
  * the same cases once more with the driver built with -fsanitize=address,undefined: a
    stand-alone program, nothing preloaded.
"""
import ctypes as C
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gpu-ray-tracing_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kat  # noqa: E402
import lbvh_util as L  # noqa: E402
import refit_util as R  # noqa: E402
from mrt import _lib  # noqa: E402
from mrt.tracer import refit_plan  # noqa: E402

DRIVER = os.path.join(PKG, "lib", "wide_plan_driver")
SOURCE = os.path.join(REPO, "tests", "cpp", "wide_plan_driver.cpp")
SENTINEL = 0x76543210
ALPHA = 1e-5


def derive_host(nodes, woop):
    """mrt_derive_wide_nodes form 1 with the Woop array: the tracer's own array."""
    lib = _lib.trace_lib()
    nodes, woop = np.ascontiguousarray(nodes), np.ascontiguousarray(woop)
    size = C.c_int64(0)
    assert lib.mrt_derive_wide_nodes(nodes.ctypes.data, nodes.nbytes, woop.ctypes.data, woop.nbytes, 1, None, 0,
                                     C.byref(size)) == 0
    out = np.zeros(size.value // 4, np.uint32)
    assert lib.mrt_derive_wide_nodes(nodes.ctypes.data, nodes.nbytes, woop.ctypes.data, woop.nbytes, 1,
                                     out.ctypes.data, out.nbytes, C.byref(size)) == 0
    return out


def stack_bound(wide):
    """wide_stack_bound restated: the most entries on the stack below any node, a node pushing
    all its present children but the one it enters."""
    w = wide.reshape(-1, 32)
    bound, todo = 0, [(0, 0)]
    while todo:
        node, depth = todo.pop()
        refs = w[node, 24:28].astype(np.int64)
        present = int((refs != SENTINEL).sum())
        below = depth + max(0, present - 1)
        bound = max(bound, below)
        todo += [(int(r) // 8, below) for r in refs if r != SENTINEL and r < 2**31]
    return bound


def run_driver(driver, tmp, nodes, woop, reverse=False):
    """The driver's line, and on "ok" (order, offsets, wide, src, bound)."""
    assert os.path.exists(driver), f"{driver} is missing: `make -C gpu-ray-tracing_amd` builds it"
    npath, wpath, opath = (os.path.join(str(tmp), f) for f in ("nodes.bin", "woop.bin", "out.bin"))
    np.ascontiguousarray(nodes, np.int32).tofile(npath)
    if woop is not None:
        np.ascontiguousarray(woop, np.int32).tofile(wpath)
    p = subprocess.run([driver, npath, wpath if woop is not None else "-", opath] + (["reverse"] if reverse else []),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, f"{driver}: exit {p.returncode}\n{p.stdout}\n{p.stderr}"
    line = p.stdout.strip()
    if not line.startswith("ok"):
        return line, None
    raw = np.fromfile(opath, np.int32)
    levels, nwide, bound, n = (int(x) for x in raw[:4])
    at = 4
    order, at = raw[at:at + n], at + n
    offsets, at = raw[at:at + levels + 1], at + levels + 1
    wide, at = raw[at:at + 32 * nwide].view(np.uint32), at + 32 * nwide
    src, at = raw[at:at + 4 * nwide], at + 4 * nwide
    assert at == len(raw)
    return line, (order, offsets, wide, src, bound)


def check_equal(driver, tmp, nodes, woop):
    want_order, want_offsets, want_src = refit_plan(nodes)
    want_wide = derive_host(nodes, woop)
    for reverse in (False, True):
        line, got = run_driver(driver, tmp, nodes, woop, reverse)
        assert got is not None, line
        order, offsets, wide, src, bound = got
        assert np.array_equal(order, want_order)
        assert np.array_equal(offsets, want_offsets)
        assert np.array_equal(src, want_src)
        assert wide.shape == want_wide.shape and np.array_equal(wide, want_wide)   # as bits, NaN planes included
        assert bound == stack_bound(want_wide)


# ---- the trees ----------------------------------------------------------------------------
def hand_built(records):
    """1: two leaves. 2: an inner child and a leaf. 3: two inner children. Distinct boxes."""
    b = kat.Compact2Builder()
    idx = [b.reserve_inner() for _ in range(records)]
    k = [0]

    def leaf():
        z = -(k[0] + 1.0)
        k[0] += 1
        return b.leaf([(k[0], (0, 0, z), (1, 0, z), (0, 1, z))])

    def box(i):
        return ((0, 0, -(i + 2.0)), (1 + i, 1, -1.0))

    for i in range(records - 1, 0, -1):
        b.set_inner(idx[i], box(i), box(i + 3), leaf(), leaf())
    if records == 1:
        b.set_inner(idx[0], box(0), box(1), leaf(), leaf())
    elif records == 2:
        b.set_inner(idx[0], box(0), box(1), idx[1] * 4, leaf())
    else:
        b.set_inner(idx[0], box(0), box(1), idx[1] * 4, idx[2] * 4)
    return b.buffers()


def identical_boxes(n_inner=61, seed=3):
    """A random binary tree whose every box is the same: every area ties, the first index wins."""
    rng = np.random.default_rng(seed)
    b = kat.Compact2Builder()
    box = ((0, 0, -1), (1, 1, 0))
    budget = [n_inner]

    def leaf():
        return b.leaf([(0, (0, 0, -1), (1, 0, -1), (0, 1, -1))])

    def build():
        idx = b.reserve_inner()
        budget[0] -= 1
        kids = []
        for _ in range(2):
            kids.append(build() if budget[0] > 0 and rng.random() < 0.7 else leaf())
        return b.set_inner(idx, box, box, kids[0], kids[1])

    build()
    return b.buffers()


def nan_and_infinite_boxes():
    """The SBVH of random 1500 with a NaN plane in every 7th child box and an infinite one in every
    11th: a NaN area is never picked, an infinite one always."""
    nodes, woop, tri = R.built("random", 1500, ALPHA)[2]
    f = np.array(nodes, np.int32).reshape(-1, 16).view(np.float32)
    f[::7, 1] = np.nan      # child 0's hi.x
    f[3::7, 10] = np.nan    # child 1's lo.z
    f[::11, 5] = np.inf     # child 1's hi.x
    f[5::11, 0] = -np.inf   # child 0's lo.x
    return f.view(np.int32).reshape(-1), woop, tri


def valid_trees():
    out = [(f"hand{r}", lambda r=r: hand_built(r)) for r in (1, 2, 3)]
    out += [("nan-inf-boxes", nan_and_infinite_boxes)]
    out += [(f"comb{d}", lambda d=d: kat.scene_comb(d)[0]) for d in (40, 70)]
    out += [("complete12", lambda: kat.scene_complete(12)[0]), ("identical", identical_boxes)]
    out += [(f"sbvh-{name}{param}", lambda name=name, param=param: R.built(name, param, ALPHA)[2])
            for name, param in R.SCENES]
    for leaf in L.LEAF_SIZES:
        out += [(f"lbvh{leaf}-{kind}", lambda kind=kind, leaf=leaf: L.host_lbvh(kind, None, leaf)[2])
                for kind in L.EDGE_SHAPES]
        out += [(f"lbvh{leaf}-{kind}", lambda kind=kind, leaf=leaf: L.host_edge(kind, leaf)[2])
                for kind in L.EDGE_GEOMETRY]
    return out


VALID = valid_trees()


@pytest.mark.parametrize("name,make", VALID, ids=[n for n, _ in VALID])
def test_level_scheme_equals_the_host_derivation(tmp_path, name, make):
    nodes, woop, _ = make()
    check_equal(DRIVER, tmp_path, nodes, woop)


def test_edge_geometry_has_nan_and_infinite_boxes():
    """The fixtures the equality above leans on: a NaN area is never picked, an infinite one wins."""
    planes = R.boxes(L.host_edge("nonfinite", 4)[2][0])
    assert np.isinf(planes).any()
    wide = derive_host(*L.host_edge("nonfinite", 4)[2][:2]).reshape(-1, 32)
    assert np.isnan(wide[:, :24].view(np.float32)).any()   # the absent children's planes


def test_without_woop_the_leaf_refs_carry_no_counts(tmp_path):
    nodes, woop, _ = R.built("random", 1500, ALPHA)[2]
    line, got = run_driver(DRIVER, tmp_path, nodes, None)
    assert got is not None, line
    lib = _lib.trace_lib()
    n = np.ascontiguousarray(nodes)
    size = C.c_int64(0)
    want = np.zeros(len(got[2]), np.uint32)
    assert lib.mrt_derive_wide_nodes(n.ctypes.data, n.nbytes, None, 0, 1, want.ctypes.data, want.nbytes,
                                     C.byref(size)) == 0
    assert np.array_equal(got[2], want)


# ---- trees that are none ----------------------------------------------------------------------
OUTSIDE = "a child ref points outside the node array"
TWICE = "a node record is reached twice (not a tree)"
UNREACHED = "a node record is not reachable from node 0"


@functools.lru_cache(maxsize=None)
def malformed():
    """{name: (nodes, refit_levels' reason)}: one defect each, most in the SBVH of random 1500."""
    base = np.array(R.built("random", 1500, ALPHA)[2][0], np.int32).reshape(-1, 16)
    n = len(base)
    inner = np.argwhere(base[:, 12:14] >= 0)   # (record, side) of the inner refs
    # an inner ref in the middle of the array whose child has an inner child itself
    rec, side = next((int(r), int(s)) for r, s in inner[len(inner) // 2:] if (base[base[r, 12 + s] // 4, 12:14] >= 0).any())
    out = {}
    for name, ref in (("past the array", 4 * n), ("far past the array", 2**31 - 4), ("no multiple of 4", 4 * 5 + 2)):
        t = base.copy()
        t[rec, 12 + side] = ref
        out[name] = (t, OUTSIDE)
    # a record reached twice: two parents share a child (the other child's subtree is lost)
    a, b = (tuple(int(x) for x in inner[k]) for k in (3, len(inner) - 2))
    t = base.copy()
    t[b[0], 12 + b[1]] = t[a[0], 12 + a[1]]
    out["reached twice"] = (t, TWICE)
    # a cycle back to an ancestor: a deep record points at the root, another at its own parent
    t = base.copy()
    t[rec, 12 + side] = 0
    out["cycle to the root"] = (t, TWICE)
    t = base.copy()
    child = int(t[rec, 12 + side]) // 4
    t[child, 12 + int(np.argwhere(t[child, 12:14] >= 0)[0][0])] = 4 * rec
    out["cycle to the parent"] = (t, TWICE)
    # an unreachable record: a ref replaced by a leaf
    t = base.copy()
    t[rec, 12 + side] = int(t[:, 12:14][t[:, 12:14] < 0][0])
    out["unreachable"] = (t, UNREACHED)
    # the smallest ones
    one = np.array(hand_built(1)[0], np.int32).reshape(-1, 16)
    for name, ref, why in (("one record, self cycle", 0, TWICE), ("one record, ref past it", 4, OUTSIDE)):
        t = one.copy()
        t[0, 12] = ref
        out[name] = (t, why)
    out["two records, second unreachable"] = (np.concatenate([one, one]), UNREACHED)
    return out


MALFORMED = ["past the array", "far past the array", "no multiple of 4", "reached twice", "cycle to the root",
             "cycle to the parent", "unreachable", "one record, self cycle", "one record, ref past it",
             "two records, second unreachable"]


def host_reason(nodes):
    lib = _lib.trace_lib()
    n = np.ascontiguousarray(nodes, np.int32).reshape(-1)
    levels = C.c_int32()
    rc = lib.mrt_refit_plan(n.ctypes.data, n.nbytes, None, None, 0, C.byref(levels), None, 0, None)
    assert rc == _lib.MRT_ERR_INVALID_ARG
    return lib.mrt_last_error_detail().decode()


def test_the_list_of_defects_is_complete():
    assert sorted(malformed()) == sorted(MALFORMED)


@pytest.mark.parametrize("name", MALFORMED)
def test_a_tree_that_is_none_is_refused_with_the_hosts_reason(tmp_path, name):
    nodes, why = malformed()[name]
    assert host_reason(nodes).endswith(why)
    for reverse in (False, True):
        line, got = run_driver(DRIVER, tmp_path, nodes.reshape(-1), None, reverse)
        assert got is None and line == "refused " + why


# ---- the same cases under the sanitizers -------------------------------------------------------
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host compiler"
    exe = str(tmp_path_factory.mktemp("wide_plan_san") / "wide_plan_driver_san")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe, SOURCE], check=True)
    return exe


def test_the_cases_under_address_and_undefined_sanitizers(sanitized, tmp_path):
    for name, make in VALID:
        if name.startswith("lbvh") and not name.startswith("lbvh4"):
            continue   # one leaf size of the LBVHs is enough here
        nodes, woop, _ = make()
        check_equal(sanitized, tmp_path, nodes, woop)
    for nodes, why in malformed().values():
        line, got = run_driver(sanitized, tmp_path, nodes.reshape(-1), None)
        assert got is None and line == "refused " + why
