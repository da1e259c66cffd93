"""A path frame on the CPU: mrth_path_extend, mrth_path_accumulate and mrth_path_resolve
(csrc/host/path.cpp over csrc/path_common.hpp), the CPU statements of mrt_path_extend / _accumulate /
_resolve, against the independent numpy model of tests/path_util.py, bit for bit (a NaN equal to a
NaN) over the edge table there; the polynomial sine and cosine against double precision over all
2^24 multiples of 2^-24; stable compaction; in-place against compacted radiance; known answers with
every trace done by the oracle; the host functions as a stand-alone program under
-fsanitize=address,undefined (tests/cpp/path_driver.cpp; nothing is preloaded); and the argument
checks of the host and the device exports, none of which needs a device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mrt
import mrt.host
from mrt import _lib

import light_util as L
import oracle_lib as O
import path_util as P
import ref_meshes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gpu-ray-tracing_amd")
F = np.float32
DRIVER = os.path.join(PKG, "lib", "path_driver")


# ---------------------------------------------------------------- 1. the hash's wrap edges
def test_the_wrap_inputs_are_what_the_table_says():
    """A word >= 0xFFFFFF80 converts to 2^32: the light sample's offset, or the bounce's shift, is
    exactly 1.0 and `p >= 1` wraps whatever the sample."""
    assert sorted(P.WRAP_INPUTS) == [0, 1, 2, 3, 4]
    for word, x in P.WRAP_INPUTS.items():
        two, three = P.hash_words(x, 0, [0])
        words = np.concatenate([two, three[:, :2]], axis=1)[0]
        assert int(words[word]) >= 0xFFFFFF80, (word, x, [hex(int(w)) for w in words])
        assert (words[word:word + 1].astype(F) * L.TWO_M32)[0] == F(1.0)
        # the same input reached through the vertex and the key
        for vertex, key in ((1, 3), (2, 0x7FFFFFFF)):
            seed = (x - vertex * P.GOLDEN - key) & 0xFFFFFFFF
            again, _ = P.hash_words(seed, vertex, [key])
            assert np.array_equal(again, two)


# ---------------------------------------------------------------- 2. the host statement against the model
def edge_case(rng, vertex, samples, in_place):
    """Inputs of one extend call on the edge table: (rays, results, state, paths, slots)."""
    rays, res = P.edge_inputs()
    if vertex == 0:
        return rays, res, None, len(rays) * samples, len(rays) * samples
    paths = len(rays) + 50
    return rays, res, P.edge_state(rng, len(rays), paths, dead_every=7 if in_place else 0), paths, len(rays)


def both(call, radiance, **kw):
    """(host output, model output, host radiance, model radiance) of one extend call."""
    r_host, r_model = radiance.copy(), radiance.copy()
    got = mrt.host.path_extend(radiance=r_host, **call, **kw)
    want = P.Model.path_extend(radiance=r_model, **call, **kw)
    return got, want, r_host, r_model


@pytest.mark.parametrize("compact", [True, False], ids=["compact", "in-place"])
@pytest.mark.parametrize("samples", P.EDGE_SAMPLES)
def test_host_extend_equals_the_model_on_the_edge_table(samples, compact):
    normals, material = P.edge_tables()
    rng = np.random.default_rng(samples)
    depth = 2
    seen = {"nan": 0, "dead": 0, "escaped": 0, "survivors": 0}
    for vertex in (0, 1, depth):
        for seed in (1, 0xFFFFFFF0, (0xFFFFFFF0 - vertex * P.GOLDEN) & 0xFFFFFFFF):   # the sums wrap at key 16
            rays, res, state, paths, slots = edge_case(rng, vertex, samples, not compact)
            radiance = rng.random((paths, 4)).astype(F)
            call = dict(rays=rays, results=res, state=state, normals=normals, material=material)
            got, want, r_host, r_model = both(call, radiance, vertex=vertex, depth=depth, num_samples=samples, seed=seed,
                                              compact=compact, **P.EDGE_LIGHT)
            assert P.same_step(got, want) == "", (vertex, seed)
            assert P.same_floats(r_host, r_model)
            assert (got["rays"] is None) == (vertex == depth)
            ids = res[:, 0] if vertex else np.repeat(res[:, 0], samples)
            alive = np.ones(slots, bool) if state is None else state[:, 3] >= 0
            hit = alive & (ids >= 0)
            assert got["live"] == hit.sum()
            seen["survivors"] += got["live"]
            seen["dead"] += int((~alive).sum())
            seen["nan"] += int(np.isnan(got["shadow"]).any(axis=1).sum())
            changed = ~(r_host.view(np.uint32) == radiance.view(np.uint32)).all(axis=1)
            seen["escaped"] += int(changed.sum())
            assert vertex >= 1 or not changed.any()          # a primary miss adds nothing
            assert (r_host[:, 3] == radiance[:, 3]).all()    # the fourth float is nobody's
            if not compact:   # every slot keeps its place; a slot without a survivor is dead
                assert (got["state"][~hit, 3] == -1).all() and (got["shadow"][~hit, 7] == -1).all()
                assert (got["pending"][~hit] == 0).all()
    assert seen["survivors"] and seen["escaped"] and seen["nan"] and (compact or seen["dead"]), seen


def test_host_extend_at_the_wrap_edges():
    normals, material = P.edge_tables()
    rays, res = P.edge_inputs()
    hits = np.flatnonzero(res[:, 0] >= 0)[:8]
    rays, res = np.ascontiguousarray(rays[hits]), np.ascontiguousarray(res[hits])
    for word, x in P.WRAP_INPUTS.items():
        for samples in (1, 3):
            # vertex 0: the key is the input ray's index, 5; vertex 1: the key is the task, 5 too
            for vertex in (0, 1):
                seed = (x - vertex * P.GOLDEN - 5) & 0xFFFFFFFF
                state = None
                if vertex:
                    state = P.edge_state(np.random.default_rng(word), 8, 8)
                    state[:, 3] = np.arange(8)
                radiance = np.zeros((8 * samples, 4), F)
                call = dict(rays=rays, results=res, state=state, normals=normals, material=material)
                got, want, _, _ = both(call, radiance, vertex=vertex, depth=2, num_samples=samples, seed=seed,
                                       compact=True, **P.EDGE_LIGHT)
                assert P.same_step(got, want) == "", (word, vertex, samples)
                assert got["live"] == (8 * samples if vertex == 0 else 8)


def test_host_accumulate_and_resolve_equal_the_model():
    rng = np.random.default_rng(8)
    for n, paths in ((1, 1), (257, 300), (1000, 1000)):
        state = P.edge_state(rng, n, paths, dead_every=5)
        pending = rng.random((n, 4)).astype(F)
        pending[::9, 0] = np.nan
        pending[1::9, 1] = 1e-39
        sres = np.zeros((n, 4), np.int32)
        sres[:, 0] = np.where(rng.random(n) < 0.5, -1, rng.integers(0, 64, n))
        radiance = rng.random((paths, 4)).astype(F)
        got = mrt.host.path_accumulate(state, pending, sres, radiance.copy())
        want = P.Model.path_accumulate(state, pending, sres, radiance.copy())
        assert P.same_floats(got, want) and not P.same_floats(got, radiance)
    for samples in P.EDGE_SAMPLES:
        for first in (0, 1, 255):
            count = 300
            radiance = (rng.random((count * samples, 4)) * 1.5).astype(F)   # some sums above 1: clamped in the pixel only
            radiance[::31, 1] = np.nan
            radiance[5::37, 2] = -0.25
            pres = np.zeros((first + count, 4), np.int32)
            pres[:, 0] = np.where(rng.random(first + count) < 0.2, -1, 3)
            pixels = first + count + 9
            s2i = rng.permutation(pixels)[:first + count].astype(np.int32)
            kw = dict(num_samples=samples, slot_to_id=s2i, primary_results=pres, radiance=radiance, num_pixels=pixels,
                      first_primary=first, num_primary=count, want_image=True)
            gp, gi = mrt.host.path_resolve(**kw)
            wp, wi = P.Model.path_resolve(**kw)
            assert np.array_equal(gp, wp) and P.same_floats(gi, wi)
            miss = s2i[first:][pres[first:, 0] == -1]
            assert (gp[miss] == L.BACKGROUND).all() and np.isnan(gi).any() and (samples > 1 or np.nanmax(gi) > 1.0)
            untouched = np.ones(pixels, bool)
            untouched[s2i[first:]] = False
            assert (gp[untouched] == 0).all() and (gi[untouched] == 0).all()


# ---------------------------------------------------------------- 3. the polynomial sine and cosine
def test_polynomial_sine_and_cosine_over_all_multiples_of_2_to_the_minus_24():
    """The header's routine, run by the stand-alone driver: the largest error against the double
    functions is within 1e-6 (measured 8.96e-8), and its bits are the model's."""
    out = subprocess.run([DRIVER, "sincos"], capture_output=True, text=True, check=True).stdout.split()
    worst_cos, worst_sin, checksum = float(out[0]), float(out[1]), int(out[2])
    print(f"max |cos error| {worst_cos:.3g}, max |sin error| {worst_sin:.3g}")
    assert worst_cos <= 1e-6 and worst_sin <= 1e-6
    u = np.arange(1 << 24, dtype=np.float64) * 2.0 ** -24
    c, s = P.sincos_turn(u.astype(F))
    assert np.abs(c - np.cos(2 * np.pi * u)).max() <= 1e-6 and np.abs(s - np.sin(2 * np.pi * u)).max() <= 1e-6
    total = int(c.view(np.uint32).astype(np.uint64).sum() + np.uint64(3) * s.view(np.uint32).astype(np.uint64).sum())
    assert total % (1 << 64) == checksum
    # the quarter turns are exact
    for turn, want in ((0.0, (1, 0)), (0.25, (0, 1)), (0.5, (-1, 0)), (0.75, (0, -1))):
        got = P.sincos_turn(np.array([turn], F))
        assert (float(got[0][0]), float(got[1][0])) == want


# ---------------------------------------------------------------- 4. stable compaction
def test_host_compaction_is_stable():
    normals, material = P.edge_tables()
    rng = np.random.default_rng(4)
    n = 1000
    for label, mask in P.survivor_patterns(n, rng):
        rays, res = P.slots_for(mask, rng)
        state = P.edge_state(rng, n, n + 17)
        got = mrt.host.path_extend(rays, res, state, np.zeros((n + 17, 4), F), normals, material, vertex=1, depth=3,
                                   num_samples=3, seed=7, compact=True, **P.EDGE_LIGHT)
        where = np.flatnonzero(mask)
        assert got["live"] == len(where), label
        assert np.array_equal(got["state"][:len(where), 3], state[where, 3]), label
        assert (got["state"][len(where):] == 0).all(), label   # nothing is written past the survivors


# ---------------------------------------------------------------- 5. known answers, traced by the oracle
def world_of(tris):
    v = np.array(tris, F).reshape(-1, 3)
    t = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    scene = mrt.Scene.from_arrays(v, t)
    bufs = mrt.Bvh.build_lbvh(scene).buffers()
    return scene, bufs, scene.arrays()[2], scene.tri_colors()[0]


def oracle_trace(bufs):
    def trace(rays, any_hit):
        return O.trace(np.ascontiguousarray(rays, F), *bufs, any_hit=any_hit, threads=8)[0]
    return trace


def rect(z, x0, x1, y0, y1):
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    return [[a, b, c], [a, c, d]]


def fan(z, half, hub):
    h = (hub[0], hub[1], z)
    c = [(-half, -half, z), (half, -half, z), (half, half, z), (-half, half, z)]
    return [[h, c[k], c[(k + 1) % 4]] for k in range(4)]


KNOWN_X = [0.0, 0.5, -0.5, 2.0, -2.0, 3.0, -3.0]
KNOWN = dict(light_pos=(0.0, 0.0, 2.0), light_radius=0.0, light_color=(1.0, 0.5, 0.25), sky=(0.2, 0.4, 0.8), max_dist=100.0)
ALBEDO = 191.0 / 255.0   # the default material's 0.75 as a byte


def known_frame(impl, tris, samples, depth, compact):
    scene, bufs, normals, material = world_of(tris)
    assert (material == 0xFFBFBFBF).all()
    prim = np.array([[x, 0.0, 0.5, 0.0, 0.0, 0.0, -1.0, 10.0] for x in KNOWN_X], F)
    trace = oracle_trace(bufs)
    pres = trace(prim, False)
    assert np.isin(pres[:, 0], (0, 1)).all() and (pres[:, 1].view(F) == 0.5).all()
    log = []
    radiance, stats = P.render_batch(impl, trace, prim, pres, 0, len(prim), normals, material, samples, depth, 1, compact,
                                     KNOWN, log=log)
    px, image = impl.path_resolve(samples, np.arange(len(prim), dtype=np.int32), pres, radiance, len(prim), want_image=True)
    return px, image, stats, log


def channels(px):
    return np.stack([px & 0xFF, (px >> 8) & 0xFF, (px >> 16) & 0xFF], axis=1).astype(np.int64)


@pytest.mark.parametrize("impl", [mrt.host, P.Model], ids=["host", "model"])
@pytest.mark.parametrize("depth", [1, 3])
def test_known_answer_floor_under_an_open_sky(impl, depth):
    """A floor at z = 0, primaries straight down onto (x, 0, 0), a point light at (0, 0, 2). Every
    bounce leaves the scene whatever the random numbers (the floor is all there is, and a bounce
    starts 1e-4 above it heading up or level), so each path collects the light at vertex 0 and the
    sky at vertex 1: the pixel is albedo * (sky + lightColor * k), k = h / sqrt(x^2 + h^2) with h =
    2 - 1e-4 the light's height above the backed-off point. Each channel is within 1 of that in
    double: truncation turns a few float32 ulps into one step at the most."""
    samples = 4
    px, image, stats, _ = known_frame(impl, rect(0.0, -4.0, 4.0, -3.0, 5.0), samples, depth, True)
    assert stats == [len(KNOWN_X) * samples, 0]
    h = 2.0 - 1e-4
    for x, p, v in zip(KNOWN_X, channels(px), image):
        k = h / np.sqrt(x * x + h * h)
        want = ALBEDO * (np.array(KNOWN["sky"]) + np.array(KNOWN["light_color"]) * k)
        assert np.abs(p - np.minimum(want, 1.0) * 255.0).max() <= 1.0, (x, p, want * 255)
        assert np.abs(v[:3] - want).max() <= 1e-5 and v[3] == 1.0
    assert (px >> 24 == 255).all()


@pytest.mark.parametrize("impl", [mrt.host, P.Model], ids=["host", "model"])
def test_known_answer_floor_and_occluder(impl):
    """The shadow frame's occluder (z = 1 over [-1, 1]^2) over the floor, depth 1. Seen from the light its
    shadow is [-2, 2]^2: x = 0 and +-0.5 are blocked and get no light term, +-3 are lit; x = +-2 is lit
    by the 1e-4 back-off alone (derived in test_gpu_light.py). A bounce may now meet the occluder's
    underside, which faces away from the light (k = 0) and ends the path at depth 1 without sky: of a
    pixel's S paths, e escape (counted from the oracle's results of the logged bounce rays), and the
    pixel is albedo * (lightColor * k * lit + sky * e / S): a blocked point gets albedo * sky alone, as
    far as its bounces escape, and never more."""
    samples = 8
    tris = rect(0.0, -4.0, 4.0, -3.0, 5.0) + fan(1.0, 1.0, (0.3, 0.4))
    px, image, stats, log = known_frame(impl, tris, samples, 1, True)
    n = len(KNOWN_X) * samples
    assert stats[0] == n and 0 < stats[1] < n    # some bounces meet the occluder, most leave
    (_, step0, _), (_, step1, _) = log
    met = np.zeros(n, int)
    met[step1["state"][:stats[1], 3]] = 1          # the tasks alive at vertex 1
    escaped = samples - met.reshape(-1, samples).sum(axis=1)
    h = 2.0 - 1e-4
    for x, p, v, e in zip(KNOWN_X, channels(px), image, escaped):
        lit = abs(x) > 1.0
        k = h / np.sqrt(x * x + h * h) if lit else 0.0
        want = ALBEDO * (np.array(KNOWN["light_color"]) * k + np.array(KNOWN["sky"]) * e / samples)
        assert np.abs(p - np.minimum(want, 1.0) * 255.0).max() <= 1.0, (x, p, want * 255)
        if not lit:
            assert (v[:3] <= ALBEDO * np.array(KNOWN["sky"]) + 1e-6).all()
    assert (escaped[np.abs(KNOWN_X) < 1.0] < samples).all() and (escaped > 0).all()   # under the occluder some of each pixel's bounces meet it


def box(half):
    """The cube [-half, half]^3 as 12 triangles over 8 shared corners."""
    c = [(x, y, z) for x in (-half, half) for y in (-half, half) for z in (-half, half)]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return [[c[a], c[b], c[d]] for a, b, d, _ in quads] + [[c[a], c[d], c[e]] for a, _, d, e in quads]


@pytest.mark.parametrize("impl", [mrt.host, P.Model], ids=["host", "model"])
def test_known_answer_closed_box_without_light(impl):
    """Seen from inside a closed box with lightColor 0 every pixel is black and no path ever leaves:
    the live count stays at all paths through every vertex (a path through a crack would collect
    the sky)."""
    scene, bufs, normals, material = world_of(box(1.0))
    rng = np.random.default_rng(2)
    d = rng.normal(size=(40, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    prim = np.zeros((40, 8), F)
    prim[:, 0:3] = (0.1, -0.2, 0.3)
    prim[:, 4:7] = d
    prim[:, 7] = 100.0
    trace = oracle_trace(bufs)
    pres = trace(prim, False)
    assert (pres[:, 0] >= 0).all()
    samples, depth = 3, 3
    scalars = dict(KNOWN, light_color=(0.0, 0.0, 0.0), light_pos=(0.0, 0.0, 0.5))
    for compact in (True, False):
        radiance, stats = P.render_batch(impl, trace, prim, pres, 0, 40, normals, material, samples, depth, 9, compact, scalars)
        assert stats == [40 * samples] * (depth + 1)
        px = impl.path_resolve(samples, np.arange(40, dtype=np.int32), pres, radiance, 40)
        assert (px == 0xFF000000).all()


W, H = 64, 48


@pytest.fixture(scope="module")
def soup():
    v, t = ref_meshes.MESHES["random1500"]()
    scene = mrt.Scene.from_arrays(v, t)
    cam = mrt.host.Camera((0.3, 0.2, 4.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 45.0, 0.01, 100.0)
    bufs = mrt.Bvh.build_lbvh(scene).buffers()
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    light = tuple(float(x) for x in (lo + (hi - lo) * np.array([0.5, 0.9, 0.9])).astype(F))
    prim, s2i = mrt.primary_rays(cam, W, H)
    trace = oracle_trace(bufs)
    return dict(scene=scene, cam=cam, bufs=bufs, normals=scene.arrays()[2], material=scene.tri_colors()[0], light=light,
                radius=float(F(0.1 * np.linalg.norm(hi - lo))), prim=prim, s2i=s2i, pres=trace(prim, False), trace=trace)


def test_depth_0_is_the_shadow_frame(soup):
    """Depth 0, sky 0 and lightColor 1: built from the shadow frame's own rays (bit for bit), each
    channel is within 1 of the RAY_SHADOW frame of the same seed: that one multiplies the material
    by k * (u / S) once, this one sums S products."""
    w = soup
    samples, seed = 4, mrt.AO_SEED
    scalars = dict(light_pos=w["light"], light_radius=w["radius"], light_color=(1.0, 1.0, 1.0), sky=(0.0, 0.0, 0.0),
                   max_dist=100.0)
    log = []
    radiance, stats = P.render_batch(mrt.host, w["trace"], w["prim"], w["pres"], 0, W * H, w["normals"], w["material"],
                                     samples, 0, seed, True, scalars, log=log)
    hits = int((w["pres"][:, 0] != -1).sum())
    assert stats == [hits * samples] and 500 < hits < W * H
    rays = mrt.host.shadow_rays(w["prim"], w["pres"], samples, w["light"], w["radius"], seed=seed)
    live = np.repeat(w["pres"][:, 0] != -1, samples)
    assert L.same_rays(log[0][1]["shadow"][:hits * samples], rays[live])
    sres = w["trace"](rays, True)
    want = mrt.host.reconstruct_lit(samples, w["s2i"], w["prim"], w["pres"], sres, w["normals"], w["material"], w["light"], W * H)
    got = mrt.host.path_resolve(samples, w["s2i"], w["pres"], radiance, W * H)
    assert np.abs(channels(got) - channels(want)).max() <= 1 and (got >> 24 == 255).all()
    assert len(np.unique(got)) > 50


def test_in_place_and_compacted_frames_give_the_same_bits(soup):
    w = soup
    scalars = dict(light_pos=w["light"], light_radius=w["radius"], light_color=(1.0, 0.9, 0.8), sky=(0.2, 0.4, 0.8),
                   max_dist=100.0)
    seeds = [mrt.AO_SEED, 846930886, 1681692777]
    out = {}
    for impl in (mrt.host, P.Model):
        for compact in (True, False):
            out[impl, compact] = P.render_frame(impl, w["trace"], w["prim"], w["pres"], w["s2i"], W * H, w["normals"],
                                                w["material"], 3, 3, seeds, 1100, compact, scalars, want_image=True)
    px, image, stats = out[mrt.host, True]
    for key, (p, i, s) in out.items():
        assert np.array_equal(p, px) and P.same_floats(i, image) and s == stats, key
    assert len(stats) == 3 and all(s[0] > s[-1] > 0 for s in stats)   # three batches that thin out
    assert len(np.unique(px)) > 100


# ---------------------------------------------------------------- 6. the same code under the sanitizers
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host compiler"
    exe = str(tmp_path_factory.mktemp("path_san") / "path_driver_san")
    sources = [os.path.join(REPO, "tests", "cpp", "path_driver.cpp"), os.path.join(PKG, "csrc", "host", "path.cpp"),
               os.path.join(PKG, "csrc", "host", "host_error.cpp"), os.path.join(PKG, "csrc", "path_plan.cpp")]
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(REPO, "include"),
                    "-o", exe, *sources], check=True)
    return exe


def test_host_functions_under_address_and_undefined_sanitizers(sanitized, tmp_path):
    def put(name, a):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(np.ascontiguousarray(a).tobytes())
        return path

    def run(args, what):
        r = subprocess.run([sanitized, *args], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, f"{what}: exit {r.returncode}\n{r.stderr[-3000:]}"

    normals, material = P.edge_tables()
    rng = np.random.default_rng(6)
    e = P.EDGE_LIGHT
    prefix = str(tmp_path / "out")
    for vertex, samples, compact, seed in ((0, 3, 1, 1), (0, 257, 0, 0xFFFFFFF0), (1, 64, 1, 0xFFFFFFF0), (1, 2, 0, 5), (2, 3, 1, 7)):
        rays, res, state, paths, slots = edge_case(rng, vertex, samples, not compact)
        radiance = rng.random((paths, 4)).astype(F)
        words = np.zeros(18, np.uint32)
        words[[0, 1, 2, 3, 15, 16, 17]] = [vertex, 2, samples, seed, compact, slots, paths]
        words[4:15] = np.array([*e["light_pos"], e["light_radius"], *e["light_color"], *e["sky"], e["max_dist"]], F).view(np.uint32)
        run(["extend", put("scalars.bin", words), put("normals.bin", normals), put("material.bin", material),
             put("rays.bin", rays), put("res.bin", res), put("state.bin", state) if state is not None else "-",
             put("radiance.bin", radiance), prefix], f"extend at vertex {vertex}")
        want_rad = radiance.copy()
        want = mrt.host.path_extend(rays, res, state, want_rad, normals, material, vertex=vertex, depth=2,
                                    num_samples=samples, seed=seed, compact=bool(compact), **e)
        got = {"shadow": np.fromfile(prefix + ".shadow", F).reshape(-1, 8), "pending": np.fromfile(prefix + ".pending", F).reshape(-1, 4),
               "rays": np.fromfile(prefix + ".rays", F).reshape(-1, 8) if vertex < 2 else None,
               "state": np.fromfile(prefix + ".state", np.int32).reshape(-1, 4), "live": int(np.fromfile(prefix + ".live", np.int32)[0])}
        assert P.same_step(got, want) == "" and P.same_floats(np.fromfile(prefix + ".radiance", F).reshape(-1, 4), want_rad)
        m = want["live"] if compact else slots
        sres = np.zeros((m, 4), np.int32)
        sres[:, 0] = np.where(rng.random(m) < 0.5, -1, 3)
        out = str(tmp_path / "acc.bin")
        run(["accumulate", str(m), str(paths), put("state.bin", want["state"][:m]), put("pending.bin", want["pending"][:m]),
             put("sres.bin", sres), put("radiance.bin", want_rad), out], "accumulate")
        assert P.same_floats(np.fromfile(out, F).reshape(-1, 4), mrt.host.path_accumulate(want["state"], want["pending"], sres,
                                                                                          want_rad.copy(), num_slots=m))
    for samples, first, count in ((1, 0, 300), (257, 255, 3), (3, 1, 256)):
        radiance = rng.random((count * samples, 4)).astype(F)
        pres = np.zeros((first + count, 4), np.int32)
        pres[::4, 0] = -1
        pixels = first + count + 5
        s2i = rng.permutation(pixels)[:first + count].astype(np.int32)
        out, img = str(tmp_path / "px.bin"), str(tmp_path / "img.bin")
        run(["resolve", str(samples), str(first), str(count), put("s2i.bin", s2i), put("res.bin", pres),
             put("radiance.bin", radiance), str(pixels), out, img], "resolve")
        wp, wi = mrt.host.path_resolve(samples, s2i, pres, radiance, pixels, first_primary=first, num_primary=count, want_image=True)
        assert np.array_equal(np.fromfile(out, np.uint32), wp) and P.same_floats(np.fromfile(img, F).reshape(-1, 4), wi)


# ---------------------------------------------------------------- 7. the plan, the argument checks, the names
def test_the_plan_sizes_the_grid_the_scan_and_the_scratch():
    def plan(*args):
        return [int(x) for x in subprocess.run([DRIVER, "plan", *map(str, args)], capture_output=True, text=True,
                                               check=True).stdout.split()]
    round_slots = _lib.MRT_PATH_SCAN_ROUND_SLOTS
    assert plan(0, 3, 3, 0, 0) == [0, 1, 0, 0, 0]
    assert plan(0, 3, 3, 1, 1) == [0, 0, 1, 1, 4]
    assert plan(1, 3, 3, 257, 300) == [0, 0, 2, 1, 8]
    assert plan(1, 3, 3, round_slots, round_slots) == [0, 0, 1024, 1, 4096]
    assert plan(1, 3, 3, round_slots + 1, round_slots + 1) == [0, 0, 1025, 2, 4100]
    assert plan(0, 64, 1, _lib.MRT_PATH_MAX_PATHS, _lib.MRT_PATH_MAX_PATHS)[:2] == [0, 0]
    assert plan(0, 65, 1, 1, 1)[0] == _lib.MRT_ERR_TOO_LARGE
    assert plan(0, 3, 1, _lib.MRT_PATH_MAX_PATHS + 1, _lib.MRT_PATH_MAX_PATHS + 1)[0] == _lib.MRT_ERR_TOO_LARGE
    for bad in ((-1, 3, 3, 1, 1), (4, 3, 3, 1, 1), (0, -1, 3, 1, 1), (0, 3, 0, 1, 1), (0, 3, 3, -1, 1), (0, 3, 3, 6, 5)):
        assert plan(*bad)[0] == _lib.MRT_ERR_INVALID_ARG, bad


def extend_params(**kw):
    """Params every check passes on but for what kw changes; the pointers are never dereferenced."""
    p = mrt.host.path_params(1, 3, 2, 1, (0, 0, 1), 0.5)
    p.numTris, p.numSlots, p.numPaths = 10, 100, 200
    names = ["triNormals", "triMaterialColor", "inRays", "inResults", "inState", "outShadowRays", "outPending", "outRays",
             "outState", "radiance", "liveCount"]
    for k, name in enumerate(names):
        setattr(p, name, 0x100000 * (k + 1))
    for name, v in kw.items():
        setattr(p, name, v)
    return p


def test_argument_checks_of_the_host_and_device_exports():
    host, dev = _lib.host_lib(), _lib.trace_lib()
    bad, large = _lib.MRT_ERR_INVALID_ARG, _lib.MRT_ERR_TOO_LARGE
    one = C.c_void_p(0x100000)
    for name, fn, code in (("host", lambda p: host.mrth_path_extend(C.byref(p)), {bad: 1, large: 1}),
                           ("device", lambda p: dev.mrt_path_extend(C.byref(p), None), {bad: bad, large: large})):
        assert fn(extend_params(numSlots=0, inRays=None, radiance=None)) == 0, name    # nothing to do, nothing looked at
        for kw in (dict(numSlots=-1), dict(numPaths=-1), dict(numSamples=0), dict(depth=-1), dict(vertex=4), dict(vertex=-1),
                   dict(vertex=0, numPaths=99), dict(numTris=-1)):
            assert fn(extend_params(**kw)) == code[bad], (name, kw)
        for kw in (dict(depth=65), dict(numSlots=_lib.MRT_PATH_MAX_PATHS + 1, numPaths=_lib.MRT_PATH_MAX_PATHS + 1),
                   dict(numPaths=_lib.MRT_PATH_MAX_PATHS + 1)):
            assert fn(extend_params(**kw)) == code[large], (name, kw)
        for ptr in ("triNormals", "triMaterialColor", "inRays", "inResults", "inState", "outShadowRays", "outPending",
                    "outRays", "outState", "radiance", "liveCount"):
            assert fn(extend_params(**{ptr: None})) == code[bad], (name, ptr)
    assert host.mrth_path_extend(None) == 1 and dev.mrt_path_extend(None, None) == bad
    # the device's own: alignment, and overlap of an output with an input or another output
    for ptr in ("inRays", "inState", "outShadowRays", "outPending", "outRays", "outState", "radiance"):
        assert dev.mrt_path_extend(C.byref(extend_params(**{ptr: 0x100008})), None) == bad, ptr
    p = extend_params()
    for a, b in (("outRays", "inRays"), ("outState", "inState"), ("outShadowRays", "outRays"), ("outPending", "inResults"),
                 ("radiance", "inRays")):
        assert dev.mrt_path_extend(C.byref(extend_params(**{a: getattr(p, b) + 16 * 99})), None) == bad, (a, b)
    # the last vertex writes no bounce ray: outRays may be NULL and is not checked
    assert dev.mrt_path_extend(C.byref(extend_params(vertex=3, outRays=None, numSlots=0)), None) == 0

    assert host.mrth_path_accumulate(0, 0, None, None, None, None) == 0
    assert dev.mrt_path_accumulate(0, 0, None, None, None, None, None) == 0
    assert host.mrth_path_accumulate(-1, 1, one, one, one, one) == 1 and dev.mrt_path_accumulate(-1, 1, one, one, one, one, None) == bad
    assert dev.mrt_path_accumulate(_lib.MRT_PATH_MAX_PATHS + 1, 1, one, one, one, one, None) == large
    for k in range(4):
        args = [one] * 4
        args[k] = None
        assert host.mrth_path_accumulate(1, 1, *args) == 1 and dev.mrt_path_accumulate(1, 1, *args, None) == bad
    assert dev.mrt_path_accumulate(1, 1, C.c_void_p(0x100008), one, one, one, None) == bad

    assert host.mrth_path_resolve(1, 0, 0, None, None, None, None, None) == 0
    assert dev.mrt_path_resolve(1, 0, 0, None, None, None, None, None, None) == 0
    for shape in ((0, 0, 1), (1, -1, 1), (1, 0, -1)):
        assert host.mrth_path_resolve(*shape, one, one, one, one, None) == 1
        assert dev.mrt_path_resolve(*shape, one, one, one, one, None, None) == bad
    assert dev.mrt_path_resolve(1 << 12, 0, 1 << 12, one, one, one, one, None, None) == large
    for k in range(4):
        args = [one] * 4
        args[k] = None
        assert host.mrth_path_resolve(1, 0, 1, *args, None) == 1 and dev.mrt_path_resolve(1, 0, 1, *args, None, None) == bad

    # the ray type exists, and mrt_reconstruct refuses it as it refuses the shadow type
    from mrt.raygen import RAY_PATH
    text = open(os.path.join(REPO, "include", "mrt.h")).read()
    assert "MRT_RAY_SHADOW = 3, MRT_RAY_PATH = 4" in text and RAY_PATH == 4
    assert dev.mrt_reconstruct(4, 1, 0, 1, one, one, None, one, one, one, one, None) == bad
    limits = open(os.path.join(PKG, "csrc", "path_limits.hpp")).read()
    assert f"kMaxPaths = 1 << {_lib.MRT_PATH_MAX_PATHS.bit_length() - 1};" in limits and "kMaxDepth = 64;" in limits
    assert "kScanThreads = 1024;" in limits and _lib.MRT_PATH_SCAN_ROUND_SLOTS == 1024 * 256


def test_renderer_refuses_to_sort_or_shard_a_path_frame():
    from mrt.raygen import RAY_PATH
    from mrt.renderer import PATH_COMPACT_DEFAULT, Renderer
    r = Renderer.__new__(Renderer)   # no device: set_params and the refusals look at nothing else
    r.set_params(RAY_PATH, 8, depth=4, light_pos=(0, 1, 2), light_radius=0.5)
    assert (r.ray_type, r.num_samples, r.depth, r.compact) == (RAY_PATH, 8, 4, PATH_COMPACT_DEFAULT)
    assert r.light_color == (1.0, 1.0, 1.0) and r.sky == (0.2, 0.4, 0.8)
    with pytest.raises(_lib.MrtError):
        r.set_params(RAY_PATH, 8, sort_secondary=True)
    with pytest.raises(_lib.MrtError):
        r.set_params(RAY_PATH, 8, depth=65)
    r.primary = None
    with pytest.raises(_lib.MrtError, match="RAY_PATH"):
        r.secondary_blocks(None, 0, 64)
    with pytest.raises(_lib.MrtError, match="RAY_PATH"):
        r.shard(2, 0, 64)
