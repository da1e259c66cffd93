"""The area sums of a Compact2 tree on the CPU: mrth_bvh_tree_cost / Bvh.tree_cost
(csrc/host/scene_attr.cpp), the CPU statement of mrt_tracer_tree_cost, against a numpy float64
restatement written from the definition (tests/scene_attr_util.py)."""
import numpy as np
import pytest

import mrt
from mrt import _lib

import scene_attr_util as U

F = np.float32


def lbvh(count, leaf, seed=1):
    scene = mrt.Scene.synthetic("random", count, seed)
    return scene, mrt.Bvh.build_lbvh(scene, leaf)


def check(bvh, what):
    nodes, woop, _ = bvh.buffers()
    got = bvh.tree_cost()
    want = U.tree_cost(nodes, woop)
    U.assert_cost_close(got, want, what)
    if want["root_area"] > 0:      # Cn = Ct = 1
        assert got["sah"] == pytest.approx((want["inner_area"] + want["leaf_tri_area"]) / want["root_area"], rel=1e-12)
    else:
        assert got["sah"] is None
    return got


@pytest.mark.parametrize("leaf", [1, 4])
def test_lbvh_of_random_equals_the_restatement(leaf):
    scene, bvh = lbvh(1500, leaf)
    got = check(bvh, f"lbvh leaf {leaf}")
    assert got["triangles"] == 1500 and got["skipped"] == 0
    assert got["leaves"] == got["records"] + 1
    if leaf == 1:
        assert got["records"] == 1499 and got["leaf_area"] == got["leaf_tri_area"]
    assert 0 < got["root_area"] < got["inner_area"]


def test_one_record_tree():
    v = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 2), (3, 1, 1)], F)
    t = np.array([(0, 1, 2), (0, 1, 3), (2, 3, 4)], np.int32)
    bvh = mrt.Bvh.build_lbvh(mrt.Scene.from_arrays(v, t), 4)
    got = check(bvh, "one record")
    assert got["records"] == 1 and got["triangles"] == 3
    # nothing refers to a record: the inner sum is the root's own area
    assert got["inner_area"] == got["root_area"] == 3 * 1 + 1 * 2 + 2 * 3


def test_sbvh_of_sphere():
    scene = mrt.Scene.synthetic("sphere", 8)
    got = check(mrt.Bvh.build(scene), "sbvh sphere")
    assert got["triangles"] >= scene.num_triangles       # spatial splits may duplicate references


def test_after_a_refit_to_displaced_vertices():
    scene, bvh = lbvh(1500, 4)
    before = bvh.tree_cost()
    v, t, _ = scene.arrays()
    moved = (v + F(0.2) * np.sin(F(3.0) * v[:, ::-1])).astype(F)
    bvh.refit(moved, t)
    after = check(bvh, "refitted")
    assert after["records"] == before["records"] and after["triangles"] == before["triangles"]
    assert after["sah"] != before["sah"]


def test_nan_and_inverted_boxes_are_skipped_and_in_no_sum():
    _, bvh = lbvh(1500, 4)
    nodes, woop, tri = bvh.buffers()
    clean = bvh.tree_cost()
    refs = nodes.reshape(-1, 16)[:, 12:14]
    inner_slot = next((n, s) for n in range(1, len(refs)) for s in range(2) if refs[n, s] >= 0)
    leaf_slot = next((n, s) for n in range(1, len(refs)) for s in range(2) if refs[n, s] < 0 and n != inner_slot[0])
    patched = nodes.copy()
    f = patched.view(F).reshape(-1, 16)
    n, s = inner_slot
    f[n, 4 * s + 1] = np.nan                                            # a NaN plane on an inner slot
    n, s = leaf_slot
    f[n, 8 + 2 * s], f[n, 9 + 2 * s] = f[n, 9 + 2 * s] + 1, f[n, 8 + 2 * s]   # z lo above z hi on a leaf slot
    got = check(mrt.Bvh.from_buffers(patched, woop, tri), "patched")
    assert got["skipped"] == 2
    assert got["leaves"] == clean["leaves"] and got["triangles"] == clean["triangles"]
    assert got["inner_area"] < clean["inner_area"] and got["leaf_area"] < clean["leaf_area"]
    # an infinite plane, and a root whose union is not finite
    inf = nodes.copy()
    inf.view(F).reshape(-1, 16)[0, 1] = np.inf
    got = check(mrt.Bvh.from_buffers(inf, woop, tri), "infinite root")
    assert got["skipped"] == 2 and got["root_area"] == 0.0 and got["sah"] is None


def test_argument_checks():
    lib = _lib.host_lib()
    assert lib.mrth_bvh_tree_cost(None, None) == _lib.MRT_ERR_INVALID_ARG
    _, bvh = lbvh(10, 4)
    assert lib.mrth_bvh_tree_cost(bvh._h, None) == _lib.MRT_ERR_INVALID_ARG
