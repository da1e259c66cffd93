"""Every instantiated traversal kernel (mrt_trace_kernel_keys: 136) on the hand-derived answers of
tests/kat.py, on stacks that spill, on a tree every node of which must be visited, on the
special-value, on-surface and incoherent rays of test_gpu_parity.py, and on leaves of up to 33
triangles (kat.leaf_gallery and an SBVH built with min_leaf 17); and the edge rays across the
launch schedules on the four production kernels.

Each case sets the configuration that selects one kernel, checks after every launch that this
kernel's function is the one that ran (Tracer.last_kernel_key: a fallback to a sibling fails), and
holds the results to the contract of its family (the docstring of
test_gpu_parity.py, test_gpu_backfill.assert_matches_oracle):

  per-lane Compact2, exact rcp    id, t and the counters bit-identical to the oracle;
  speculative Compact2 and the    closest-hit t bit-identical, ids identical except at exact-t ties
  exact 4-wide kernels, exact     (each a valid hit); any-hit hit/miss identical, every differing
  rcp (tail, one-shot included)   hit valid;
  quantized 4-wide, exact rcp     an oracle hit never becomes a miss; a differing closest hit is a
                                  valid hit no farther than the oracle's, at most max(2, n / 10^4)
                                  of them on the primary and incoherent rays (no cap on the
                                  special-value and on-surface rays); any-hit as above;
  fast rcp, every family          hand answers bit-exact; rays with a NaN or an infinity in them:
                                  hit/miss as the oracle, hits valid with 1/Dz one ulp off; the
                                  others: every mismatch a tie or decided by the reciprocal's
                                  rounding (classify_fast_rcp "other" == 0), |dt| <= 2 ulp on equal
                                  ids, a miss keeps tmax's bits;
  STATS kernels                   {id, t} byte-identical to the sibling without counters, every
                                  counter row written over its poison, a hit has tested a triangle
                                  (and, closest hit, finished a leaf: an any-hit ray leaves the leaf
                                  at its hit before the terminator, as the oracle's counter does), a
                                  ray that enters a root child has fetched a node, and the rays whose
                                  traversal is forced (kat.scene_complete) have at least its counts.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kat  # noqa: E402
import leaf_util  # noqa: E402
import oracle_lib as O  # noqa: E402
from test_abi import expected_kernel_keys  # noqa: E402
from test_gpu_backfill import SENTINEL, assert_matches_oracle, cus, restore, tracer  # noqa: E402,F401
from test_gpu_parity import (assert_valid_hits, fuzz_rays, on_surface_rays, scene_setup, special_rays,  # noqa: E402
                             ulp_diff)

POISON = 0x6B6B6B6B
ANY, SPEC, EXACT, STATS, TAIL, ONESHOT = 1, 2, 4, 8, 256, 512
COMPACT2, WIDE4, WIDE4Q = 0, 1, 2
COMPLETE_DEPTH = 12


def key_fields(key):
    return dict(any_hit=bool(key & ANY), spec=bool(key & SPEC), exact=bool(key & EXACT), stats=bool(key & STATS),
                lds=8 << ((key >> 4) & 3), nodes=(key >> 6) & 3, tail=bool(key & TAIL), oneshot=bool(key & ONESHOT))


def key_name(key):
    f = key_fields(key)
    return "-".join([("compact2", "wide4", "wide4q")[f["nodes"]], f"S{f['lds']}", "any" if f["any_hit"] else "closest",
                     "spec" if f["spec"] else "lane", "exact" if f["exact"] else "fast"] +
                    [n for n in ("stats", "tail", "oneshot") if f[n]])


def key_config(key):
    """The launch configuration that selects exactly this kernel."""
    f = key_fields(key)
    return dict(autotune=0, waves_per_cu=4, lds_stack=f["lds"], wide=f["nodes"], tail_lanes=16 if f["tail"] else 0,
                backfill=1 if f["oneshot"] else 0, oneshot=1 if f["oneshot"] else 0,
                deal_block=10 if f["oneshot"] else 0)


# ---------------------------------------------------------------- the batches (CPU only)
class Batch:
    """Rays against one BVH. hand: (ray, any_hit, exact (id, t) or None, allowed {(id, t)} or None):
    the per-lane kernel gives `exact`; any other kernel gives `exact` too unless an `allowed` set
    names the answers another test order may give. bounds: (ray, any_hit, binary nodes, wide nodes,
    triangles, leaves) every correct traversal of that ray reaches at least. nonfinite: rays with a
    NaN or an infinity among the special-value rays. capped: the rays the quantized count cap covers."""

    def __init__(self, name, bufs, rays):
        self.name, self.bufs, self.rays = name, bufs, np.ascontiguousarray(rays, np.float32)
        n = len(self.rays)
        self.hand, self.bounds = [], []
        self.nonfinite, self.capped = np.zeros(n, bool), np.zeros(n, bool)
        self._oracle = {}

    def oracle(self, any_hit):
        if any_hit not in self._oracle:
            want, st, _ = O.trace(self.rays, *self.bufs, any_hit=any_hit, stats=True, threads=8)
            want.setflags(write=False)
            st.setflags(write=False)
            self._oracle[any_hit] = (want, st)
        return self._oracle[any_hit]


_BATCHES = []


def batches():
    if _BATCHES:
        return _BATCHES
    # kat.cases() and kat.tie_cases(), one batch per hand-built scene
    by_scene = {}
    for name, scene, rays, any_hit, expected in kat.cases():
        by_scene.setdefault(scene, []).extend((r, any_hit, e, None) for r, e in zip(rays, expected))
    for name, scene, rays, any_hit, per_lane, allowed in kat.tie_cases():
        by_scene.setdefault(scene, []).extend((r, any_hit, e, a) for r, e, a in zip(rays, per_lane, allowed))
    for scene, items in by_scene.items():
        b = Batch(scene.__name__, scene(), np.stack([it[0] for it in items]))
        b.hand = [(i, it[1], it[2], it[3]) for i, it in enumerate(items)]
        _BATCHES.append(b)
    # 40 pushes before the first pop: spills at every LDS stack size; 130 rays = two waves and two rays
    bufs, ray, expect = kat.scene_comb(40)
    b = Batch("comb40", bufs, np.stack([ray] * 130))
    comb_any = {(k, k + 2.0) for k in range(41)}
    b.hand = [(i, False, expect, None) for i in range(130)] + [(i, True, None, comb_any) for i in range(130)]
    _BATCHES.append(b)
    # every box of the complete tree holds the ray and is entered before t = 1.1875, the only hit
    # (t = 1.5) is in the last leaf: no order can cull a node, so every node, triangle and leaf is
    # visited. The short ray (tmax = 1 + 17/128) is culled below binary level 8 and misses; it ends
    # while the others are under way, so in a tail kernel their groups are rebuilt mid-traversal.
    d = COMPLETE_DEPTH
    bufs, ray, expect = kat.scene_complete(d, hit_last=True)
    short = ray.copy()
    short[7] = 1.0 + 17.0 / 128.0
    b = Batch(f"complete{d}", bufs, np.stack([short, ray, ray]))
    for any_hit in (False, True):
        b.hand += [(0, any_hit, (-1, float(short[7])), None), (1, any_hit, expect, None), (2, any_hit, expect, None)]
    wide_nodes = (4 ** (d // 2) - 1) // 3
    b.bounds = [(i, False, 2 ** d - 1, wide_nodes, 2 ** d, 2 ** d) for i in (1, 2)] + \
               [(i, True, d, d // 2, 1, 0) for i in (1, 2)]
    _BATCHES.append(b)
    # primary, special-value, on-surface and incoherent rays on two stand-in scenes
    for scene in ("bunny", "hairball:800"):
        bufs, base, _, _, _ = scene_setup(scene, 64, 48, "primary")
        special = special_rays(base)
        parts = [base, special, on_surface_rays(base, bufs), fuzz_rays(scene, 2000, 1)[1]]
        b = Batch(scene, bufs, np.concatenate(parts))
        lo = len(base)
        b.nonfinite[lo:lo + len(special)] = ~np.isfinite(special).all(axis=1)
        b.capped[:lo] = True
        b.capped[len(b.rays) - 2000:] = True
        _BATCHES.append(b)
    # leaves of 1 to 33 triangles (every other batch: 8 at the most), the deciding triangle at every
    # list position: the counted leaf loop's two exits, counts 9 to 15 and the 0 of a longer leaf,
    # the tail's chunks of four, the uncounted loops' prefetch past the end of the Woop array
    g = leaf_util.gallery()
    b = Batch("leaf-gallery", tuple(np.array(a) for a in g["bufs"]), g["rays"])
    b.hand, b.bounds = list(g["hand"]), list(g["bounds"])
    _BATCHES.append(b)
    # an SBVH with leaves of 5 to 17 triangles, a 64 x 48 frame and 1000 incoherent rays; no count
    # cap: every differing quantized result must be a valid closer hit
    name = "random1500-min17"
    _BATCHES.append(Batch(name, tuple(np.array(a) for a in leaf_util.buffers(name)), leaf_util.rays_for(name)))
    return _BATCHES


_EDGE = []


def edge_batch():
    """§4: the special-value and on-surface rays on hairball:800 (built once)."""
    if _EDGE:
        return _EDGE[0]
    bufs, base, _, _, _ = scene_setup("hairball:800", 64, 48, "primary")
    special = special_rays(base)
    b = Batch("hairball:800 edge rays", bufs, np.concatenate([special, on_surface_rays(base, bufs)]))
    b.nonfinite[:len(special)] = ~np.isfinite(special).all(axis=1)
    _EDGE.append(b)
    return b


def test_batches_agree_with_the_oracle_on_the_cpu():
    """No GPU: the hand answers and forced counts of every batch hold in the oracle (which walks
    the per-lane order), and the rays under the quantized count cap are few enough for the cap to
    be its floor of 2: a kernel cannot hide a third differing ray behind the batch's size."""
    for b in batches():
        for any_hit in (False, True):
            want, st = b.oracle(any_hit)
            for i, mode, exact, allowed in b.hand:
                if mode == any_hit and exact is not None:
                    assert (want[i, 0], want[i, 1]) == (exact[0], kat.f2i(exact[1])), (b.name, i)
                if mode == any_hit and allowed is not None:
                    assert (want[i, 0], want[i, 1]) in {(k, kat.f2i(t)) for k, t in allowed}, (b.name, i)
            for i, mode, nodes2, _, tris, leaves in b.bounds:
                if mode == any_hit:
                    assert st[i, 0] >= nodes2 and st[i, 1] >= tris and st[i, 2] >= leaves, (b.name, i)
                    if not any_hit:   # the forced traversal is exactly the whole tree
                        assert tuple(st[i, :3]) == (nodes2, tris, leaves)
        if b.capped.any():
            assert 5000 <= b.capped.sum() < 20000 and max(2, int(b.capped.sum()) // 10000) == 2
            assert b.nonfinite.sum() >= 10 * 192
    short = [b for b in batches() if b.name.startswith("complete")][0].oracle(False)[1][0]
    assert tuple(short[:3]) == (2 ** 9 - 1, 0, 0)   # binary levels 0..8, never a leaf


# ---------------------------------------------------------------- launching
_DEVICE = {}


def device_rays(b, n):
    """The batch's rays on the device, tiled cyclically to n rays (cached)."""
    k = (b.name, n)
    if k not in _DEVICE:
        _DEVICE[k] = torch.from_numpy(np.resize(b.rays, (n, 8))).cuda()
    return _DEVICE[k]


def device_bvh(b):
    from mrt.tracer import GpuBvh
    k = (b.name, "bvh")
    if k not in _DEVICE:
        _DEVICE[k] = GpuBvh(b.bufs)
    return _DEVICE[k]


def launch(tracer, b, n, key):
    """One blocking trace of the kernel `key` into sentinel-filled results and poisoned counters;
    the kernel that ran must be that kernel."""
    from mrt.tracer import RayBuffer
    f = key_fields(key)
    rb = RayBuffer(device_rays(b, n), need_closest_hit=not f["any_hit"])
    rb.results.fill_(SENTINEL)
    if f["stats"]:
        rb.stats = torch.full((n, 4), POISON, dtype=torch.int32, device=rb.rays.device)
    tracer.trace_batch(rb, exact_rcp=f["exact"], speculative=f["spec"], stats=f["stats"])
    ran = tracer.last_kernel_key
    assert ran == key, f"{b.name}: asked for {key_name(key)}, {key_name(ran) if ran >= 0 else ran} ran"
    assert tracer.last_info["stack_overflows"] == 0
    r = rb.results_numpy()
    assert (r[:, 2:] == SENTINEL).all(), "RayResult padding was overwritten"
    assert not ((r[:, 0] == SENTINEL) & (r[:, 1] == SENTINEL)).any(), f"{b.name}: a ray was not traced"
    return r, (rb.stats.cpu().numpy() if f["stats"] else None)


# ---------------------------------------------------------------- the contracts
def differing(res, want):
    return np.nonzero((res[:, 0] != want[:, 0]) | (res[:, 1] != want[:, 1]))[0]


def as_float(col):
    return np.ascontiguousarray(col).view(np.float32)


def quantized_extra_hits(rays, res, want, bufs, which, rcp_ulps):
    """Of the rays `which`, those the quantized nodes may answer differently: their boxes contain
    the binary boxes, so the traversal may find a hit the oracle's slab test culled. Such a result
    is a hit, a valid one, and no farther than the oracle's."""
    hit = res[which, 0] != -1
    closer = as_float(res[which, 1]) <= as_float(want[which, 1])
    cand = which[hit & closer]
    bad = set(O.invalid_hits(rays, res, bufs[1], bufs[2], which=cand, rcp_ulps=rcp_ulps).tolist())
    return np.array([i for i in cand if i not in bad], np.int64)


def check_exact(f, rays, res, want, bufs, capped):
    any_hit = f["any_hit"]
    if f["nodes"] == COMPACT2 and not f["spec"]:
        assert np.array_equal(res[:, :2], want[:, :2]), "per-lane order: not bit-identical to the oracle"
    elif f["nodes"] != WIDE4Q:
        assert_matches_oracle(rays, res, want, bufs, any_hit)
    elif any_hit:
        assert_valid_hits(rays, res, want, bufs)
    else:
        assert not ((want[:, 0] != -1) & (res[:, 0] == -1)).any(), "quantized nodes lost an oracle hit"
        diff = differing(res, want)
        ok = quantized_extra_hits(rays, res, want, bufs, diff, 0)
        assert len(ok) == len(diff), f"{len(diff) - len(ok)} differing quantized-node results are not valid closer hits"
        n_capped = int(capped.sum())
        if n_capped:
            assert int(capped[diff].sum()) <= max(2, n_capped // 10000), f"{int(capped[diff].sum())} rays differ"


def check_fast(f, rays, res, want, bufs, nonfinite):
    nodes, woop, tri = bufs
    miss = res[:, 0] == -1
    assert np.array_equal(res[miss, 1], np.ascontiguousarray(rays[miss, 7]).view(np.int32)), "a miss lost tmax's bits"
    nf = np.nonzero(nonfinite)[0]
    assert np.array_equal(res[nf, 0] == -1, want[nf, 0] == -1), "non-finite rays: hit/miss differs"
    d = nf[(res[nf, 0] != want[nf, 0]) | (res[nf, 1] != want[nf, 1])]
    assert len(O.invalid_hits(rays, res, woop, tri, which=d, rcp_ulps=1)) == 0, "non-finite rays: an invalid hit"
    fin = np.nonzero(~nonfinite)[0]
    r, g, w = rays[fin], res[fin].copy(), want[fin]
    if f["nodes"] == WIDE4Q and not f["any_hit"]:
        d = np.nonzero((g[:, 0] != w[:, 0]) | (ulp_diff(g[:, 1], w[:, 1]) > 2))[0]
        ok = quantized_extra_hits(r, g, w, bufs, d, 1)
        g[ok] = w[ok]
    if f["any_hit"]:
        c = O.classify_any_hit_flips(r, g, w, woop, tri)
        assert c["other"] == 0, c
        same = (g[:, 0] == -1) == (w[:, 0] == -1)
        d = np.nonzero(same & ((g[:, 0] != w[:, 0]) | (g[:, 1] != w[:, 1])))[0]
        assert len(O.invalid_hits(r, g, woop, tri, which=d, rcp_ulps=1)) == 0, "an invalid any-hit result"
    else:
        c = O.classify_fast_rcp(r, g, w, woop, tri)
        assert c["other"] == 0 and c["unclassified"] == 0, c
        same = (w[:, 0] != -1) & (g[:, 0] == w[:, 0])
        assert ulp_diff(g[same, 1], w[same, 1]).max(initial=0) <= 2


def check_hand(f, b, res):
    n = len(b.rays)
    per_lane = f["nodes"] == COMPACT2 and not f["spec"]
    for i, mode, exact, allowed in b.hand:
        if mode != f["any_hit"]:
            continue
        got = {(int(k), int(t)) for k, t in res[i::n, :2]}   # every copy of the ray
        if exact is not None and (per_lane or allowed is None):
            assert got == {(exact[0], kat.f2i(exact[1]))}, f"{b.name} ray {i}: {got}, hand answer {exact}"
        else:
            assert got <= {(k, kat.f2i(t)) for k, t in allowed}, f"{b.name} ray {i}: {got} not among {allowed}"


def check_stats(f, b, rays, res, st, ost):
    n = len(b.rays)
    assert (st[:, :3] != POISON).all(), "a traced ray's counters were not written"
    hit = res[:, 0] != -1
    assert (st[hit, 1] >= 1).all(), "a hit without a tested triangle"
    if not f["any_hit"]:
        assert (st[hit, 2] >= 1).all(), "a closest hit without a finished leaf"
    entered = (rays[:, 3] < rays[:, 7]) & ((ost[:, 0] >= 2) | (ost[:, 1] >= 1))
    assert (st[entered, 0] >= 1).all(), "a ray inside a root child's box without a fetched node"
    if f["nodes"] == COMPACT2 and not f["spec"] and f["exact"]:
        assert np.array_equal(st[:, :3], ost[:, :3]), "per-lane counters differ from the oracle's"
    for i, mode, nodes2, nodes4, tris, leaves in b.bounds:
        if mode == f["any_hit"]:
            rows = st[i::n]
            low = (nodes2 if f["nodes"] == COMPACT2 else nodes4, tris, leaves)
            assert (rows[:, :3] >= np.array(low)).all(), f"{b.name} ray {i}: counters {rows[0, :3]} below {low}"


def check_batch(f, b, res, st):
    """res (and st) hold the batch's rays tiled cyclically: every copy answers to the contract."""
    n, total = len(b.rays), len(res)
    src = np.arange(total) % n
    want, ost = b.oracle(f["any_hit"])
    rays, want, ost = b.rays[src], want[src], ost[src]
    check_hand(f, b, res)
    if f["exact"]:
        check_exact(f, rays, res, want, b.bufs, b.capped[src])
    else:
        check_fast(f, rays, res, want, b.bufs, b.nonfinite[src])
    if f["stats"]:
        check_stats(f, b, rays, res, st, ost)


# ---------------------------------------------------------------- §3: every kernel
@pytest.mark.gpu
@pytest.mark.parametrize("key", expected_kernel_keys(), ids=key_name)
def test_kernel_variant(tracer, restore, key):
    f = key_fields(key)
    tracer.set_config(**key_config(key))
    for b in batches():
        # one-shot: ragged and past the resident grid (256 lanes per CU at 4 waves per CU)
        n = cus() * 256 + 4097 if f["oneshot"] else len(b.rays)
        tracer.set_bvh(device_bvh(b))
        res, st = launch(tracer, b, n, key)
        if f["oneshot"]:
            assert tracer.last_info["oneshot"] == 1 and tracer.last_info["deal_block"] == 10
        if f["stats"]:
            plain, _ = launch(tracer, b, n, key & ~STATS)
            assert res[:, :2].tobytes() == plain[:, :2].tobytes(), f"{b.name}: results differ from the kernel without counters"
        check_batch(f, b, res, st)


# ---------------------------------------------------------------- §4: edge rays across the schedules
PRODUCTION = SPEC | EXACT | 1 << 4 | WIDE4 << 6
SCHEDULES = [dict(lane_groups=16), dict(lane_groups=64, waves_per_cu=4), dict(ray_sort=1),
             dict(num_queues=8, queue_block=64), dict(num_queues=8, queue_shared=15, fetch_threshold=48),
             dict(num_queues=-1, fetch_threshold=16), dict(tail_lanes=1), dict(spec_slack=0), dict(spec_slack=63),
             dict(backfill=1), dict(backfill=3)]


@pytest.mark.gpu
@pytest.mark.parametrize("any_hit", [False, True], ids=["closest", "any"])
@pytest.mark.parametrize("tail", [0, 16], ids=["notail", "tail"])
@pytest.mark.parametrize("cfg", SCHEDULES, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_edge_rays_across_the_schedules(tracer, restore, cfg, tail, any_hit):
    if "tail_lanes" in cfg and not tail:
        cfg = dict(cfg, tail_lanes=0)   # the kernel without the tail has one setting: off
    cfg = {**dict(autotune=0, wide=1, lds_stack=16, tail_lanes=tail), **cfg}
    key = PRODUCTION | (ANY if any_hit else 0) | (TAIL if cfg["tail_lanes"] else 0)
    b = edge_batch()
    k = cfg.get("backfill", 0)
    if k:   # past the resident grid at k rays per lane, ragged
        cfg["waves_per_cu"] = 4
    n = k * cus() * 256 + 4097 if k else len(b.rays)
    tracer.set_config(**cfg)
    tracer.set_bvh(device_bvh(b))
    res, _ = launch(tracer, b, n, key)
    if k:
        assert tracer.last_info["backfill"] == k and tracer.last_info["num_queues"] == 0
    check_batch(key_fields(key), b, res, None)

