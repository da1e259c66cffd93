"""The refit, derive and traversal kernels on trees that no code of this project built: the
reference's own .dat files of tests/golden/ref/ (written by its compiled SplitBVHBuilder and
CudaBVH; see tests/test_ref_host.py). Only committed files are read.

  random300     an ordinary tree
  slivers200    652 references to 200 triangles: duplicated references, clipped boxes
  degenerate90  zero-area rows; the point triangles never entered the tree
  coincident40  1240 references to 40 equal triangles: equal boxes, every hit a tie
  tiny100       coordinates of 1e-30: rows and box products in the denormal range, a 50-level chain
  coplanar      2364 references to 240 triangles: the deepest of the well-formed trees
  guard60       coordinates of 1e-12: every row a signed zero, 25 Z rows kept from reading as
                terminators by the -0.0 -> +0.0 guard alone

  * device refit (csrc/refit_kernel.hip, which compiles woop_common.hpp) with the scene's own
    vertices: the Woop rows come back as the reference's CudaBVH wrote them, at wide 0 and 1, as
    bits (refit_util.same_bits_or_nan: the one documented x86 / gfx950 difference is the sign of a
    NaN an operation makes). So do the nodes where the reference's boxes are boxes of whole
    triangles; where the builder clipped references they are the independent numpy refit's
    (test_ref_host.py says why they cannot be the reference's);
  * set_bvh(on_device=True) derives the 4-wide bytes and the refit plan of the host route;
  * 2 048 rays per tree through the four production kernels, exact reciprocal, per-lane order
    (the one-shot kernels have none: theirs is the speculative order).
"""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mrt  # noqa: E402
import oracle_lib as O  # noqa: E402
import ref_meshes as M  # noqa: E402
import refit_util as U  # noqa: E402
from mrt.tracer import GpuBvh, RayBuffer, Tracer, refit_plan  # noqa: E402

TREES = ["random300", "slivers200", "degenerate90", "coincident40", "tiny100", "coplanar", "guard60"]
CLIPPED = {"slivers200", "coincident40", "coplanar"}      # more references than triangles
RESIDENT_LANES_PER_CU = 256

KERNELS = {
    "compact2": dict(wide=0),
    "wide-exact": dict(wide=1),
    "oneshot": dict(wide=1, waves_per_cu=4, backfill=1, oneshot=1, autotune=0, deal_block=10),
    "quantized": dict(wide=2),
}


@pytest.fixture(scope="module")
def tracer():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return Tracer(0)


@pytest.fixture()
def restore(tracer):
    saved = tracer.config()
    yield
    tracer.set_config(**saved)


@functools.lru_cache(maxsize=None)
def tree(name):
    """((nodes, woop, triIndex) of the reference's .dat, the scene's vertices, triangles, camera)."""
    with open(os.path.join(M.GOLDEN_REF, name + ".dat"), "rb") as f:
        layout, nodes, woop, tri = M.split_dat(f.read())
    assert layout == 5
    scene = mrt.Scene.from_obj(M.obj_path(name))
    v, t, _ = scene.arrays()
    for a in (nodes, woop, tri, v, t):
        a.setflags(write=False)
    return (nodes, woop, tri), v, t, scene.camera()[0]


def gpu(bufs):
    return GpuBvh(tuple(np.array(b) for b in bufs))


def download(g):
    torch.cuda.synchronize()
    return g.nodes.cpu().numpy(), g.woop.cpu().numpy(), g.tri_index.cpu().numpy()


def first_difference(a, b):
    a, b = (np.ascontiguousarray(x).view(np.uint32).reshape(-1) for x in (a, b))
    i = np.nonzero(a != b)[0]
    return "equal" if not i.size else f"{i.size} words differ, first at {i[0]}: {a[i[0]]:#010x} against {b[i[0]]:#010x}"


# ---- device refit against the reference's bytes ----------------------------------------------

@functools.lru_cache(maxsize=None)
def refitted_nodes(name):
    """What a refit with unchanged vertices must leave in the nodes: the reference's own bytes, or
    where references were clipped the numpy refit's (whole triangles' boxes)."""
    bufs, v, t, _ = tree(name)
    if name not in CLIPPED:
        return bufs[0]
    nodes, woop = U.np_refit(*bufs, v, t)
    assert np.array_equal(woop, bufs[1])
    return nodes


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("name", TREES)
def test_device_refit_keeps_the_reference_bytes(tracer, restore, name, wide):
    bufs, v, t, _ = tree(name)
    tracer.set_config(wide=wide)
    g = gpu(bufs)
    tracer.set_bvh(g)
    wide_before = tracer.wide_nodes()
    tracer.refit(v, t)
    nodes, woop, tri = download(g)
    assert np.array_equal(tri, bufs[2])
    assert U.same_bits_or_nan(woop, bufs[1]), f"{name} woop: " + first_difference(woop, bufs[1])
    want = refitted_nodes(name)
    assert U.same_bits_or_nan(nodes, want), f"{name} nodes: " + first_difference(nodes, want)
    assert tracer.refit_info()["skipped_refs"] == 0
    if wide:
        U.check_wide(wide_before, tracer.wide_nodes(), bufs[0], nodes)


# ---- device derivation against the host's on foreign trees -------------------------------------

# Levels of inner nodes in each committed tree. coplanar (489 nodes) is the depth stress among
# the well-formed ones; tiny100 is deeper still: areas of 1e-60 underflow to zero, every SAH is 0,
# and the reference builder (ours after it) strings its 51 nodes into a chain of 50 levels.
DEPTH_LEVELS = {"random300": 9, "slivers200": 10, "degenerate90": 6, "coincident40": 12, "tiny100": 50, "coplanar": 13,
                "guard60": 6}


def depth_levels(nodes):
    """Levels of inner nodes below the root, the root's included."""
    refs = np.ascontiguousarray(nodes).view(np.int32).reshape(-1, 16)[:, 12:14]
    level, frontier = 0, [0]
    while frontier:
        level += 1
        frontier = [int(r) // 4 for n in frontier for r in refs[n] if r >= 0]
    return level


@pytest.mark.parametrize("name", TREES)
def test_device_derivation_equals_the_hosts(tracer, restore, name):
    bufs = tree(name)[0]
    tracer.set_config(wide=1)
    tracer.set_bvh(gpu(bufs))
    wide, info, plan = tracer.wide_nodes(), tracer.bind_info(), refit_plan(bufs[0])
    tracer.set_bvh(gpu(bufs), on_device=True)
    got = tracer.wide_nodes()
    assert got.size == wide.size and U.same_bits_or_nan(got, wide), first_difference(got, wide)
    strip = lambda d: {k: x for k, x in d.items() if k != "bind_ms"}
    assert strip(tracer.bind_info()) == strip(info)
    order, offsets, src = tracer.refit_plan()
    assert np.array_equal(order, plan[0]) and np.array_equal(offsets, plan[1]) and np.array_equal(src, plan[2])
    d = tracer.derive_info()
    assert d["on_device_plan"] == 1 and d["on_device_wide"] == 1
    assert d["levels"] == len(plan[1]) - 1 and d["wide_nodes"] == wide.size // 32
    assert d["depth_levels"] == depth_levels(bufs[0]) == DEPTH_LEVELS[name]


# ---- traversal on reference-built trees -----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rays_and_answers(name):
    """2 048 rays: 32 x 32 from the scene's camera, and 1 024 between random points of the
    bounding box (grown by a quarter) with random tmin and tmax; the oracle's closest and any-hit
    answers on the reference's buffers, and the brute force's over every row of the Woop buffer."""
    bufs, v, t, cam = tree(name)
    frame = mrt.primary_rays(cam, 32, 32)[0]
    if not np.isfinite(frame).all():       # tiny100: the scene's own camera underflows
        frame = U.frame_rays(v, 32, 32)
    rng = np.random.default_rng(len(name) * 1000 + len(v))
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    grow = 0.25 * (hi - lo).max()          # one length for all axes: the coplanar scene has no height
    a = rng.uniform(lo - grow, hi + grow, (1024, 3))
    b = rng.uniform(lo - grow, hi + grow, (1024, 3))
    rand = np.concatenate([a, rng.uniform(0.0, 0.3, (1024, 1)), b - a, rng.uniform(0.4, 1.5, (1024, 1))], 1)
    rays = np.ascontiguousarray(np.concatenate([frame, rand.astype(np.float32)]), np.float32)
    assert np.isfinite(rays).all()
    closest = O.trace(rays, *bufs)[0]
    anyhit = O.trace(rays, *bufs, any_hit=True)[0]
    brute = O.brute_force(rays, bufs[1], bufs[2])
    brute_any = O.brute_force(rays, bufs[1], bufs[2], any_hit=True)
    for x in (rays, closest, anyhit, brute, brute_any):
        x.setflags(write=False)
    return rays, closest, anyhit, brute, brute_any


@pytest.mark.parametrize("name", TREES)
def test_the_oracle_on_reference_trees_equals_brute_force(name):
    """No GPU in this one: the answers the kernels are held to are those of testing every
    triangle, so a reference tree loses no hit (clipped boxes included)."""
    rays, closest, anyhit, brute, brute_any = rays_and_answers(name)
    bufs = tree(name)[0]
    assert np.array_equal(closest[:, 1], brute[:, 1])
    ties = np.nonzero(closest[:, 0] != brute[:, 0])[0]
    assert len(O.invalid_hits(rays, closest, bufs[1], bufs[2], which=ties)) == 0
    assert np.array_equal(anyhit[:, 0] == -1, brute_any[:, 0] == -1)
    hits = int((closest[:, 0] != -1).sum())
    if name in ("tiny100", "guard60"):
        # Nothing can be hit there: the determinant of every Woop matrix underflows to zero (in tiny100
        # the cross product of two 1e-30 edges already does). What the kernels are held to is 2 048
        # misses: down a 50-level chain of denormal-range boxes, and through leaves whose rows are zeros.
        assert hits == 0
    else:
        assert 32 <= hits < len(rays), hits
        assert (closest[1024:, 0] != -1).any()


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", TREES)
def test_traces_on_reference_trees_equal_the_oracle(tracer, restore, name, kernel):
    rays, closest, anyhit, _, _ = rays_and_answers(name)
    check_kernel(tracer, kernel, tree(name)[0], rays, closest, anyhit)


def check_kernel(tracer, kernel, bufs, rays, closest, anyhit):
    """One of KERNELS on a tree, against the oracle's closest and any-hit answers (shared with
    tests/test_gpu_leaf_sizes.py)."""
    reps = 1
    if kernel == "oneshot":     # that kernel runs only grids larger than the resident lanes
        resident = torch.cuda.get_device_properties(0).multi_processor_count * RESIDENT_LANES_PER_CU
        reps = resident // len(rays) + 1
    batch = np.tile(rays, (reps, 1))
    tracer.set_config(**KERNELS[kernel])
    tracer.set_bvh(gpu(bufs))
    assert tracer.bind_info()["wide_format"] == KERNELS[kernel]["wide"]
    for any_hit, want in ((False, closest), (True, anyhit)):
        rb = RayBuffer(batch, need_closest_hit=not any_hit)
        # per-lane order everywhere but in the one-shot kernels, which exist in the speculative order only
        tracer.trace_batch(rb, exact_rcp=True, speculative=kernel == "oneshot")
        if kernel == "oneshot":
            assert tracer.last_info["oneshot"] == 1
        assert tracer.last_info["stack_overflows"] == 0
        got = rb.results_numpy()
        want = np.tile(want, (reps, 1))
        if any_hit:
            assert np.array_equal(got[:, 0] == -1, want[:, 0] == -1), "hit/miss differs"
            reported = np.nonzero(got[:, 0] != -1)[0]
            assert len(O.invalid_hits(batch, got, bufs[1], bufs[2], which=reported)) == 0
            continue
        assert np.array_equal(got[:, 1], want[:, 1]), "closest-hit t: " + first_difference(got[:, 1], want[:, 1])
        ties = np.nonzero(got[:, 0] != want[:, 0])[0]
        if kernel == "compact2":
            assert ties.size == 0          # the reference's own order: the oracle's triangle, ties included
        # elsewhere the allowed-set rule of kat.tie_cases: another triangle only with the same exact t
        assert len(O.invalid_hits(batch, got, bufs[1], bufs[2], which=ties)) == 0
