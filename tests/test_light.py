"""An area light's shadow rays and the lit reconstruction on the CPU: mrth_shadow_rays and
mrth_reconstruct_lit (csrc/host/light.cpp over csrc/light_common.hpp), the CPU statements of
mrt_raygen_shadow and mrt_reconstruct_lit, against the independent numpy model of
tests/light_util.py, bit for bit (a NaN equal to a NaN) on the tables there; the model's own
properties (the wrap edge of the offset, positions inside the cube); the argument checks of the
host and the device exports, none of which needs a device; and the two host functions built as a
stand-alone program with -fsanitize=address,undefined (tests/cpp/light_driver.cpp; nothing is
preloaded)."""
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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gpu-ray-tracing_amd")
F = np.float32


# ---------------------------------------------------------------- 1. the model's own edges
def test_the_wrap_edges_are_what_the_table_says_and_stay_inside_the_cube():
    """A mixed word >= 0xFFFFFF80 converts to 2^32: the offset is exactly 1.0, `p >= 1` wraps every
    sample, and pos stays in [-1, 1)."""
    for seed_plus_task, word, value in L.WRAP_EDGES:
        words = L.hash_words([seed_plus_task])[0]
        assert int(words[word]) == value, (seed_plus_task, [hex(int(w)) for w in words])
        assert value >= 0xFFFFFF80
        off = L.offsets(seed_plus_task, [0])
        assert off[0, word] == F(1.0) and (off >= 0).all() and (off <= 1).all()
        # as a seed with task 0, and as seed 1 with the task that reaches it
        for seed, task in ((seed_plus_task, 0), (1, seed_plus_task - 1)):
            for samples in (1, 3, 64):
                pos = L.positions(L.offsets(seed, [task]), samples)
                assert (pos >= -1).all() and (pos < 1).all()
                # wrapped by exactly 1: the sample's own coordinate, mapped, but for the bits that
                # q + 1 rounds away (half an ulp of [1, 2), doubled)
                q = L.sobol2d(samples)[:, word] if word < 2 else L.hammersley(samples)
                assert np.abs(pos[0, :, word].astype(np.float64) - (2.0 * q.astype(np.float64) - 1.0)).max() <= 2.0 ** -23


def test_model_sequences_against_hand_values():
    """sobol2D's first points (the second coordinate with the kernel's `v2 << 1`) and hammersley."""
    s = L.sobol2d(5)
    assert s[:, 0].tolist() == [0.0, 0.5, 0.75, 0.25, 0.875]
    # v2 = 3 << 30, 5 << 29 (0xA0000000), 15 << 28: << 1 in 32 bits gives 0x80000000, 0x40000000, 0xE0000000
    assert s[:, 1].tolist() == [0.0, 0.5, 0.25, 0.75, 0.875]
    assert L.hammersley(4).tolist() == [0.125, 0.375, 0.625, 0.875]
    a, b, c = L.jenkins_mix([0], [0], [0])
    assert (int(a[0]), int(b[0]), int(c[0])) == (0, 0, 0)


# ---------------------------------------------------------------- 2. the host generator against the model
@pytest.mark.parametrize("seed", L.EDGE_SEEDS)
@pytest.mark.parametrize("samples", L.EDGE_SAMPLES)
def test_host_shadow_rays_equal_the_model_on_the_edge_table(samples, seed):
    rays, res = L.edge_inputs()
    seen = {"zero_dir": 0, "nan": 0, "dead": 0, "inf_tmax": 0}
    for label, light, radius, own in L.lights():
        for first in L.EDGE_FIRSTS:
            for count in L.EDGE_COUNTS:
                got = mrt.host.shadow_rays(rays, res, samples, light, radius, seed=seed, first=first, count=count)
                want, pos = L.shadow_rays(rays[first:first + count], res[first:first + count], samples, light, radius, seed)
                assert L.same_rays(got, want), (label, first, count)
                assert (pos >= -1).all() and (pos < 1).all()
                ids = np.repeat(res[first:first + count, 0], samples)
                assert ((got[:, 7] == -1) == (ids == -1)).all()
                assert (got[:, 3] == 0).all()
                seen["zero_dir"] += int((got[:, 4:7] == 0).all(axis=1).sum())
                seen["nan"] += int(np.isnan(got).any(axis=1).sum())
                seen["dead"] += int((ids == -1).sum())
                seen["inf_tmax"] += int(np.isinf(got[:, 7]).sum())
                if label == "radius0":     # all S rays of an input are equal
                    g = got.reshape(count, samples, 8)
                    assert L.same_rays(g, np.repeat(g[:, :1], samples, axis=1))
                if label == "on-origin" and first <= own < first + count:
                    g = got.reshape(count, samples, 8)[own - first]
                    assert (g[:, 4:7] == 0).all() and (g[:, 7] == 0).all()
                if label == "1e30":        # an infinite length: zero directions, tmax inf on live rays
                    finite_origin = np.isfinite(got[:, 0:3]).all(axis=1)
                    assert (got[finite_origin, 4:7] == 0).all()
                    assert np.isinf(got[finite_origin & (ids != -1), 7]).all()
    assert all(v > 0 for v in seen.values()), seen


def test_host_shadow_rays_at_the_wrap_edges():
    rays, res = L.edge_inputs()
    light, radius = L.ORDINARY_LIGHT
    for seed_plus_task, _, _ in L.WRAP_EDGES:
        for samples in (1, 3, 64):
            got = mrt.host.shadow_rays(rays, res, samples, light, radius, seed=seed_plus_task, count=3)
            assert L.same_rays(got, L.shadow_rays(rays[:3], res[:3], samples, light, radius, seed_plus_task)[0])
            # the same hash reached through the task: seed = the value - 2, task 2
            got = mrt.host.shadow_rays(rays, res, samples, light, radius, seed=seed_plus_task - 2, count=3)
            want, _ = L.shadow_rays(rays[:3], res[:3], samples, light, radius, seed_plus_task - 2)
            assert L.same_rays(got, want)


# ---------------------------------------------------------------- 3. the host reconstruction against the model
@pytest.mark.parametrize("first", L.LIT_FIRSTS)
def test_host_reconstruct_lit_equals_the_model(first):
    rng = np.random.default_rng(first)
    normals, material, rays, res, s2i, num_pixels = L.lit_table()
    levels = set()
    for light in L.lit_lights():
        for n in range(1, 65):
            for permuted in (False, True):
                case = L.lit_case(first, n, permuted, light, rng)
                got = mrt.host.reconstruct_lit(**case)
                want = L.lit_pixels(**case)
                assert np.array_equal(got, want), (n, permuted, np.nonzero(got != want)[0][:8])
                touched = np.zeros(num_pixels, bool)
                touched[s2i[first:first + L.LIT_COUNT]] = True
                assert (got[~touched] == 0).all() and ((got[touched] >> 24) == 255).all()
                levels.update((got[touched] & 0xFF).tolist())
    assert len(levels) > 20   # images, not constants


def test_lit_factor_is_zero_at_right_angles_and_for_zero_and_nan_normals():
    normals, material, rays, res, s2i, num_pixels = L.lit_table()
    light = L.lit_lights()[0]
    k = L.lit_factor(rays, res, normals, light)
    ids = res[:, 0]
    down = rays[:, 4] == 0
    for tri in (0, 1):    # +-z normals, the light level with the point
        assert (ids[down] == tri).any() and (k[down & (ids == tri)] == 0).all()
    for tri in (2, 3, 7):  # zero, NaN, one NaN component
        assert (ids == tri).any() and (k[ids == tri] == 0).all()
    assert (k[(ids == 4) | (ids == 5)] > 0).any()   # +-x normals: one of the two faces the light
    # and the pixels there are black with alpha 1, whatever the samples say
    case = L.lit_case(0, 4, False, light, np.random.default_rng(1))
    got = mrt.host.reconstruct_lit(**case)
    sel = np.nonzero(np.isin(ids[:L.LIT_COUNT], (2, 3, 7)))[0]
    assert len(sel) and (got[s2i[sel]] == 0xFF000000).all()
    assert (got[s2i[np.nonzero(ids[:L.LIT_COUNT] == -1)[0]]] == L.BACKGROUND).all() and L.BACKGROUND == 0xFFCC6633


# ---------------------------------------------------------------- 4. argument checks (no device needed)
def test_argument_checks_of_the_host_and_device_exports():
    host, dev = _lib.host_lib(), _lib.trace_lib()
    one = C.c_void_p(16)   # never dereferenced, 16-byte aligned
    light = (C.c_float * 3)(0, 0, 1)
    bad = 1
    assert host.mrth_shadow_rays(None, None, 0, 1, None, 0.0, 1, None) == 0
    assert host.mrth_shadow_rays(one, one, -1, 1, light, 0.0, 1, one) == bad
    assert host.mrth_shadow_rays(one, one, 1, 0, light, 0.0, 1, one) == bad
    for k in range(4):
        args = [one, one, light, one]
        args[k] = None
        assert host.mrth_shadow_rays(args[0], args[1], 1, 1, args[2], 0.0, 1, args[3]) == bad
    assert host.mrth_reconstruct_lit(1, 0, 0, None, None, None, None, None, None, None, None, None) == 0
    assert host.mrth_reconstruct_lit(0, 0, 1, one, one, one, None, one, one, one, light, one) == bad
    assert host.mrth_reconstruct_lit(1, -1, 1, one, one, one, None, one, one, one, light, one) == bad
    assert host.mrth_reconstruct_lit(1, 0, -1, one, one, one, None, one, one, one, light, one) == bad

    bad = _lib.MRT_ERR_INVALID_ARG
    assert dev.mrt_raygen_shadow(None, None, 0, 1, None, 0.0, 1, None, None, None, None) == 0
    assert dev.mrt_raygen_shadow(one, one, -1, 1, light, 0.0, 1, one, None, None, None) == bad
    assert dev.mrt_raygen_shadow(one, one, 1, 0, light, 0.0, 1, one, None, None, None) == bad
    for k in range(4):
        args = [one, one, light, one]
        args[k] = None
        assert dev.mrt_raygen_shadow(args[0], args[1], 1, 1, args[2], 0.0, 1, args[3], None, None, None) == bad
    assert dev.mrt_raygen_shadow(one, one, 1 << 20, 1 << 12, light, 0.0, 1, one, None, None, None) == _lib.MRT_ERR_TOO_LARGE
    assert dev.mrt_raygen_shadow(C.c_void_p(8), one, 1, 1, light, 0.0, 1, one, None, None, None) == bad   # alignment
    seeds = (C.c_uint32 * 1)(1804289383)
    sp = C.cast(seeds, C.c_void_p)
    # mrt_raygen_ao_blocks' checks (tests/test_abi.py): nothing listed, too many blocks, a wrong ray
    # count, fewer seeds than batches
    assert dev.mrt_raygen_shadow_blocks(None, None, 100, 2, light, 0.0, sp, 1, 1000, None, 0, 64, 0, None, None) == 0
    assert dev.mrt_raygen_shadow_blocks(one, one, 100, 2, light, 0.0, sp, 1, 1000, one, 5, 64, 5 * 64, one, None) == bad
    assert dev.mrt_raygen_shadow_blocks(one, one, 100, 2, light, 0.0, sp, 1, 1000, one, 2, 64, 2 * 64 + 1, one, None) == bad
    assert dev.mrt_raygen_shadow_blocks(one, one, 100, 2, light, 0.0, sp, 1, 30, one, 1, 64, 64, one, None) == bad
    assert dev.mrt_raygen_shadow_blocks(one, one, 100, 2, None, 0.0, sp, 1, 1000, one, 1, 64, 64, one, None) == bad
    assert dev.mrt_reconstruct_lit(1, 0, 0, None, None, None, None, None, None, None, None, None, None) == 0
    assert dev.mrt_reconstruct_lit(0, 0, 1, one, one, one, None, one, one, one, light, one, None) == bad
    assert dev.mrt_reconstruct_lit(1, -1, 1, one, one, one, None, one, one, one, light, one, None) == bad
    for k in range(8):
        args = [one, one, one, one, one, one, light, one]
        args[k] = None
        assert dev.mrt_reconstruct_lit(1, 0, 1, args[0], args[1], args[2], None, *args[3:], None) == bad
    # the ray type exists, and mrt_reconstruct still refuses it
    from mrt.raygen import RAY_SHADOW
    text = open(os.path.join(REPO, "include", "mrt.h")).read()
    assert "MRT_RAY_SHADOW = 3" in text and RAY_SHADOW == 3
    assert dev.mrt_reconstruct(3, 1, 0, 1, one, one, None, one, one, one, one, None) == bad


# ---------------------------------------------------------------- 5. the same code under the sanitizers
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host compiler"
    exe = str(tmp_path_factory.mktemp("light_san") / "light_driver_san")
    sources = [os.path.join(REPO, "tests", "cpp", "light_driver.cpp"), os.path.join(PKG, "csrc", "host", "light.cpp"),
               os.path.join(PKG, "csrc", "host", "host_error.cpp")]
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(REPO, "include"),
                    "-o", exe, *sources], check=True)
    return exe


def test_both_host_functions_under_address_and_undefined_sanitizers(sanitized, tmp_path):
    def put(name, a):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(np.ascontiguousarray(a).tobytes())
        return path

    rays, res = L.edge_inputs()
    out = str(tmp_path / "out.bin")
    for label, light, radius, _ in L.lights():
        for first, count, samples, seed in ((0, 257, 3, 1), (255, 1, 257, 0xFFFFFFF0), (1, 256, 64, 0xFFFFFFF0)):
            args = [sanitized, "shadow", put("rays.bin", rays[first:first + count]), put("res.bin", res[first:first + count]),
                    str(count), str(samples), put("light.bin", np.array([*light, radius], F)), str(seed), out]
            r = subprocess.run(args, capture_output=True, text=True)
            assert r.returncode == 0 and not r.stderr, f"{label}: exit {r.returncode}\n{r.stderr[-3000:]}"
            got = np.fromfile(out, F).reshape(-1, 8)
            want = mrt.host.shadow_rays(rays, res, samples, light, radius, seed=seed, first=first, count=count)
            assert L.same_rays(got, want), label
    rng = np.random.default_rng(3)
    for first in (0, 256):
        for n, permuted in ((1, False), (17, True), (64, False)):
            case = L.lit_case(first, n, permuted, L.lit_lights()[1], rng)
            end = first + L.LIT_COUNT
            args = [sanitized, "lit", str(n), str(first), str(L.LIT_COUNT), put("s2i.bin", case["slot_to_id"][:end]),
                    put("rays.bin", case["primary_rays"][:end]), put("res.bin", case["primary_results"][:end]),
                    put("b2s.bin", case["batch_id_to_slot"]) if permuted else "-", put("batch.bin", case["batch_results"]),
                    put("normals.bin", case["normals"]), put("material.bin", case["material"]),
                    put("light.bin", np.array(case["light"], F)), str(case["num_pixels"]), out]
            r = subprocess.run(args, capture_output=True, text=True)
            assert r.returncode == 0 and not r.stderr, f"lit {first} {n}: exit {r.returncode}\n{r.stderr[-3000:]}"
            assert np.array_equal(np.fromfile(out, np.uint32), mrt.host.reconstruct_lit(**case))
