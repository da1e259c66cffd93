"""Leaves of 9 to 33 triangles on the CPU (no GPU here; tests/test_gpu_leaf_sizes.py has the
device's side). The builders' defaults and the LBVH's limit keep every other tree of the suite
at 8 triangles a leaf or fewer, but a caller may bind Compact2 leaves of any length, and a
4-wide leaf ref carries its count only up to 15 (wide::wide_leaf_ref: 0 = find the terminator).

  * the hand answers and forced counts of kat.leaf_gallery() hold in the oracle, and the oracle
    finds what brute force finds on the gallery and on the four natural trees of leaf_util;
  * the natural trees hold the leaf sizes the tests lean on (leaf_util.check_histogram);
  * mrt_derive_wide_nodes, both forms: a leaf ref's count is the leaf's true size (the gallery's
    by construction, a natural tree's counted from the terminators) up to 15 and 0 above, its
    slot the Compact2 ref's; the checks of test_wide_nodes.py hold on these trees;
  * the level scheme of the device derivation (lib/wide_plan_driver) gives the host's bytes;
  * the host refit equals the numpy restatement, and Bvh.optimize keeps the leaves.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kat  # noqa: E402
import lbvh_util as L  # noqa: E402
import leaf_util as LU  # noqa: E402
import optimize_util as U  # noqa: E402
import oracle_lib as O  # noqa: E402
import refit_util as R  # noqa: E402
import test_wide_nodes as WN  # noqa: E402
import test_wide_plan as WP  # noqa: E402

NATURAL = list(LU.NATURAL)
LEAF_ADDR_BITS = 27


# ---- the gallery -------------------------------------------------------------------------------
def test_the_gallery_holds_every_size_twice_and_is_exact():
    g = LU.gallery()
    sizes = sorted(n for _, n, _, _ in g["leaves"])
    assert sizes == sorted(2 * list(kat.GALLERY_SIZES))
    assert LU.leaf_sizes(g["bufs"][0], g["bufs"][1]) == LU.true_sizes("gallery")
    rays = g["rays"]
    assert len(rays) == 2 * (sum(kat.GALLERY_SIZES) + len(kat.GALLERY_SIZES))
    assert sorted(i for _, _, _, idx in g["leaves"] for i in idx) == list(range(len(rays)))
    # every coordinate a multiple of 1/8 (kat.woop_rows has asserted that the rows are exact)
    assert np.array_equal(rays * 8, np.round(rays * 8))
    boxes = R.boxes(g["bufs"][0])
    assert np.array_equal(boxes * 8, np.round(boxes * 8))


def test_the_gallery_puts_the_deciding_triangle_at_every_list_position():
    """From the hand answers alone: each triangle of each leaf is some ray's closest hit (row) or
    some ray's per-lane any-hit answer (stack: the first accepted, after its position's rejects)."""
    g = LU.gallery()
    tri = g["bufs"][2]
    for kind, n, ref, idx in g["leaves"]:
        ids = [int(tri[~ref + 3 * k]) for k in range(n)]
        assert len(set(ids)) == n
        mine = [h for h in g["hand"] if h[0] in idx]
        if kind == "row":
            closest = [h[2][0] for h in mine if not h[1]]
            assert closest == ids + [-1]
        else:
            first = [h[2][0] for h in mine if h[1]]
            assert first == [ids[0]] + ids[::-1]
            assert all(h[2][0] == ids[-1] for h in mine if not h[1])
            assert [len(h[3]) for h in mine if h[1]] == [n] + list(range(1, n + 1))


def test_the_gallerys_hand_answers_and_bounds_hold_in_the_oracle():
    g = LU.gallery()
    for any_hit in (False, True):
        want, st, _ = O.trace(g["rays"], *g["bufs"], any_hit=any_hit, stats=True)
        for i, mode, exact, allowed in g["hand"]:
            if mode == any_hit:
                assert (want[i, 0], want[i, 1]) == (exact[0], kat.f2i(exact[1])), (i, any_hit)
                assert allowed is None or exact in allowed
        for i, mode, nodes2, _, tris, leaves in g["bounds"]:
            if mode == any_hit:
                assert tuple(st[i, :3]) == (nodes2, tris, leaves), (i, st[i])


@pytest.mark.parametrize("name", LU.NAMES)
def test_the_oracle_finds_what_brute_force_finds(name):
    bufs = LU.buffers(name)
    if name == "gallery":
        rays, min_hits = LU.gallery()["rays"], sum(kat.GALLERY_SIZES)
    else:
        rays, min_hits = R.frame_rays(LU.built(name)[0]), 16
    L.trace_like_brute_force(O, rays, bufs, min_hits)
    got = O.trace(rays, *bufs, any_hit=True)[0]
    want = O.brute_force(rays, bufs[1], bufs[2], any_hit=True)
    assert np.array_equal(got[:, 0] == -1, want[:, 0] == -1)


# ---- the natural trees -------------------------------------------------------------------------
@pytest.mark.parametrize("name", NATURAL)
def test_the_natural_trees_hold_the_leaf_sizes(name):
    h = LU.histogram(LU.true_sizes(name))
    print(name, len(LU.built(name)[2][0]) // 16, "records,", sum(h.values()), "leaves:", h)
    LU.check_histogram(name, h)
    _, _, bufs = LU.built(name)
    z, term = R.leaf_walk(bufs[0], bufs[1])
    assert 3 * len(z) + len(term) == len(bufs[1]) // 4   # the leaves tile the Woop array
    assert sum(n * c for n, c in h.items()) == len(z)


# ---- the 4-wide derivation ---------------------------------------------------------------------
@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("name", LU.NAMES)
def test_leaf_refs_carry_the_true_counts(name, form):
    nodes, woop, _ = LU.buffers(name)
    true = LU.true_sizes(name)
    stride, refs_off = (32, 24) if form == 1 else (16, 12)
    refs = WN.derive(nodes, form, woop).reshape(-1, stride)[:, refs_off:refs_off + 4].view(np.int32)
    leaf = (~refs[refs < 0]).astype(np.int64)
    slot, count = leaf & ((1 << LEAF_ADDR_BITS) - 1), leaf >> LEAF_ADDR_BITS
    assert sorted(~slot) == sorted(true)                          # the slot bits are the Compact2 refs'
    size = np.array([true[int(~s)] for s in slot])
    assert np.array_equal(count, np.where(size <= 15, size, 0)), \
        sorted({(int(n), int(c)) for n, c in zip(size, count) if c != (n if n <= 15 else 0)})
    if name != "hairball3-min33":   # (its leaves hold 12 or 24) both sides of the 15 / 16 boundary are there
        assert (size == 15).any() and (size == 16).any() and ((size >= 9) & (size <= 14)).any()
    # without the Woop array: no counts, the Compact2 refs themselves
    plain = WN.derive(nodes, form).reshape(-1, stride)[:, refs_off:refs_off + 4].view(np.int32)
    assert sorted(plain[plain < 0]) == sorted(true)


@pytest.mark.parametrize("name", LU.NAMES)
def test_the_checks_of_test_wide_nodes_hold(name):
    nodes, woop, _ = LU.buffers(name)
    nodes = np.ascontiguousarray(nodes).view(np.int32).reshape(-1)
    woop = np.ascontiguousarray(woop).view(np.int32).reshape(-1)
    trees = (nodes, WN.derive(nodes, 1), WN.derive(nodes, 2), woop)
    WN.test_both_forms_have_the_same_children(trees)
    WN.test_exact_form_keeps_the_compact2_boxes(trees)
    WN.test_quantized_boxes_contain_the_exact_boxes(trees)
    WN.test_leaf_refs_carry_their_triangle_counts(trees)


@pytest.mark.parametrize("name", LU.NAMES)
def test_level_scheme_equals_the_host_derivation(tmp_path, name):
    nodes, woop, _ = LU.buffers(name)
    WP.check_equal(WP.DRIVER, tmp_path, nodes, woop)


# ---- refit and optimize ------------------------------------------------------------------------
@pytest.mark.parametrize("name", NATURAL)
def test_host_refit_equals_the_numpy_restatement(name):
    v, t, bufs = LU.built(name)
    v2 = R.displaced(v)
    nodes, woop, tri = R.host_refit(bufs, v2, t)
    want_nodes, want_woop = R.np_refit(*bufs, v2, t)
    assert not np.array_equal(woop, bufs[1]), "the displacement moved nothing"
    assert np.array_equal(woop, want_woop)
    assert R.same_nodes(nodes, want_nodes)
    assert np.array_equal(tri, bufs[2])
    assert LU.leaf_sizes(nodes, woop) == LU.true_sizes(name)   # no Z row became a terminator, none was lost
    back = R.host_refit((nodes, woop, tri), v, t)
    assert np.array_equal(back[1], bufs[1])


@pytest.mark.parametrize("rounds", U.ROUNDS)
@pytest.mark.parametrize("name", NATURAL)
def test_optimize_keeps_the_leaves(name, rounds):
    _, _, bufs = LU.built(name)
    nodes, info = U.host_optimized("sbvh-" + name, rounds)
    U.check_still_a_tree(bufs[0], nodes)
    assert np.array_equal(U.leaf_multiset(nodes), U.leaf_multiset(bufs[0]))
    assert LU.leaf_sizes(nodes, bufs[1]) == LU.true_sizes(name)
    assert info["rounds"] == rounds
    if name != "hairball3-min33":
        assert info["rewritten"][0] > 0, "nothing was restructured: the test shows nothing"
