"""The host chain held to the reference's own compiled code, byte for byte.

tests/golden/ref/ holds what oracle/_ref/ref_host wrote: the reference's OBJ importer, Scene,
SplitBVHBuilder, CudaBVH (Compact2), stream writer, hash, pixel table and camera decoder, compiled
from the reference tree by oracle/Makefile and run over the meshes of tests/ref_meshes.py. No code
of this project took part in them. Everything here compares bytes with ==, NaN bits included.

The tests of the first part read the committed fixtures only and never skip. The second part
(`needs_ref_host`) runs where the binary has been built and skips elsewhere; it keeps the fixtures
from drifting and covers what is too large to commit.
"""
import os
import sys

import numpy as np
import pytest

import mrt
import ref_meshes as R
import refit_util as U

G = R.GOLDEN_REF
RESULTS = R.load_results()
CASE_IDS = [c[0] for c in R.CASES]
CASES = {c[0]: c for c in R.CASES}


def data(name):
    with open(os.path.join(G, name), "rb") as f:
        return f.read()


obj_path = R.obj_path


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.nbytes == b.nbytes and a.tobytes() == b.tobytes()


def first_difference(a, b):
    a, b = bits(a).reshape(-1), bits(b).reshape(-1)
    if a.size != b.size:
        return f"sizes {a.size} and {b.size} words"
    i = np.nonzero(a != b)[0]
    return "equal" if not i.size else f"{i.size} words differ, first at {i[0]}: {a[i[0]]:#010x} against {b[i[0]]:#010x}"


def ref_scene(mesh):
    info = RESULTS["scenes"][mesh]
    return R.split_scene(data(mesh + ".scene.bin"), info["num_triangles"], info["num_vertices"]), info


def parse_obj(path):
    """The .obj read with a correctly rounding number parser and no renumbering."""
    v, t = [], []
    with open(path) as f:
        for line in f:
            p = line.split()
            if p[0] == "v":
                v.append([float(x) for x in p[1:]])
            elif p[0] == "f":
                t.append([int(x) - 1 for x in p[1:]])
    return np.array(v, np.float32), np.array(t, np.int32)


def build_params(case):
    _, mesh, min_leaf, max_leaf, alpha = CASES[case]
    return mesh, dict(min_leaf=min_leaf, max_leaf=max_leaf, split_alpha=alpha)


# ---- the fixtures themselves ---------------------------------------------------------------

def test_fixture_directory_holds_every_table_entry():
    have = set(os.listdir(G))
    want = {"ref_results.json"}
    want |= {m + ".obj.gz" for m in R.MESHES} | {m + ".scene.bin" for m in R.MESHES} | {c + ".dat" for c in CASE_IDS}
    assert want <= have, sorted(want - have)
    assert set(RESULTS["scenes"]) == set(R.MESHES) and set(RESULTS["cases"]) == set(CASE_IDS)
    sizes = {f: os.path.getsize(os.path.join(G, f)) for f in have}
    assert max(sizes.values()) < 200 * 1000, max(sizes, key=sizes.get)
    assert sum(sizes.values()) < 1500 * 1000
    # the table holds what it was asked to hold
    for tag in ("nosplit", "maxleaf4", "minleaf2"):
        assert {f"slivers200-{tag}", f"random300-{tag}"} <= set(CASE_IDS)
    assert RESULTS["scenes"]["smallest"]["num_triangles"] == R.SMALLEST_REF_SAFE == 3


def test_no_mesh_holds_a_nan_or_an_infinity():
    for mesh in R.MESHES:
        v, _ = parse_obj(obj_path(mesh))
        assert np.isfinite(v).all(), mesh


def test_the_parameter_sets_and_the_slivers_do_what_they_are_there_for():
    """Spatial splits happen on the slivers (more references than triangles) and not with
    split_alpha = 1; the other parameter sets build other trees than the defaults."""
    c = RESULTS["cases"]
    assert c["slivers200"]["num_tris"] > 3 * c["slivers200"]["num_triangles"]
    assert c["slivers200-nosplit"]["num_tris"] == c["slivers200-nosplit"]["num_triangles"] == 200
    assert data("slivers200-maxleaf4.dat") != data("slivers200.dat") != data("slivers200-nosplit.dat")
    assert data("slivers200-minleaf2.dat") != data("slivers200.dat")
    assert data("random300-minleaf2.dat") != data("random300.dat")
    assert len({c[k]["cache_name"] for k in c}) == len(c)


# ---- OBJ importer, scene flattening, hash --------------------------------------------------

@pytest.mark.parametrize("mesh", list(R.MESHES))
def test_scene_from_obj_equals_the_reference_scene(mesh):
    (t, n, mat, sh, v), info = ref_scene(mesh)
    scene = mrt.Scene.from_obj(obj_path(mesh))
    assert (scene.num_triangles, scene.num_vertices) == (info["num_triangles"], info["num_vertices"])
    v2, t2, n2 = scene.arrays()
    mat2, sh2 = scene.tri_colors()
    assert same_bytes(t, t2), "triangle vertex indices: " + first_difference(t, t2)
    assert same_bytes(v, v2), "vertex positions: " + first_difference(v, v2)
    assert same_bytes(n, n2), "normals: " + first_difference(n, n2)
    assert same_bytes(mat, mat2), "material colours: " + first_difference(mat, mat2)
    assert same_bytes(sh, sh2), "shaded colours: " + first_difference(sh, sh2)
    assert "%08x" % scene.hash() == info["scene_hash"]


def test_overflowed_normals_shade_black_as_in_the_reference():
    """big100: the cross products overflow, every normal is NaN, and the framework's clamp
    (min(max(v, 0), 1) on `a > b ? a : b`) turns the NaN shade into 0. This decides the scene
    hash and with it the bvhcache file name."""
    (t, n, mat, sh, v), info = ref_scene("big100")
    assert np.isnan(n).all() and (sh == 0xFF000000).all() and (mat == 0xFFBFBFBF).all()
    _, sh2 = mrt.Scene.from_obj(obj_path("big100")).tri_colors()
    assert (sh2 == 0xFF000000).all()


@pytest.mark.parametrize("mesh", list(R.MESHES))
def test_from_arrays_and_from_obj(mesh):
    """Scene.from_arrays takes positions and indices as they are. The reference's importer does
    two things to an .obj that a plain reading of the same text does not (and nothing else: no
    welding of equal positions, the same default material, no normals kept):
      - its number parser (String.cc:452-509) accumulates decimals in float32, so the text of a
        float32 comes back up to a few ulps off unless it is a short dyadic number;
      - it numbers vertices in order of first use by a face (MeshWavefrontIO.cc:317-348).
    So from_arrays of the importer's own positions and indices hashes like from_obj, always; from_arrays
    of the plainly parsed text does so exactly when neither of the two changed anything."""
    scene = mrt.Scene.from_obj(obj_path(mesh))
    v, t, n = scene.arrays()
    again = mrt.Scene.from_arrays(v, t)
    assert again.hash() == scene.hash()
    assert same_bytes(again.arrays()[2], n) and same_bytes(again.tri_colors()[1], scene.tri_colors()[1])

    pv, pt = parse_obj(obj_path(mesh))
    unchanged = same_bytes(pv, v) and same_bytes(pt, t)
    assert (mrt.Scene.from_arrays(pv, pt).hash() == scene.hash()) == unchanged
    assert unchanged == (mesh in ("coincident9", "coincident40")), "the table should hold both kinds"
    if pv.shape == v.shape and same_bytes(pt, t):
        ulps = np.abs(pv.view(np.int32).astype(np.int64) - v.view(np.int32))
        assert ulps.max() <= 4           # the parser's error, not another vertex


def test_the_importer_renumbers_vertices_by_first_use():
    pv, pt = parse_obj(obj_path("grid20x20"))
    v, t, _ = mrt.Scene.from_obj(obj_path("grid20x20")).arrays()
    assert t[0].tolist() == [0, 1, 2] and pt[0].tolist() != [0, 1, 2]
    assert same_bytes(v[t], pv[pt])      # integers and eighths parse exactly: same triangles, other numbering


# ---- SBVH builder, Compact2 layout, Woop rows, cache name, .dat writer ------------------------

@pytest.mark.parametrize("threads", [0, 1, 3])
@pytest.mark.parametrize("case", CASE_IDS)
def test_build_and_save_equal_the_reference_dat(case, threads, tmp_path):
    mesh, params = build_params(case)
    scene = mrt.Scene.from_obj(obj_path(mesh))
    out = str(tmp_path / "ours.dat")
    mrt.Bvh.build(scene, threads=threads, **params).save(out)
    want = data(case + ".dat")
    with open(out, "rb") as f:
        got = f.read()
    if got != want:
        names = ("nodes", "woop", "triIndex")
        diff = [f"{k}: {first_difference(a, b)}" for k, a, b in zip(names, R.split_dat(got)[1:], R.split_dat(want)[1:])]
        raise AssertionError(f"{case}, threads={threads}: " + "; ".join(diff))


@pytest.mark.parametrize("case", CASE_IDS)
def test_cache_name_equals_the_reference(case):
    mesh, params = build_params(case)
    assert mrt.Bvh.cache_name(mrt.Scene.from_obj(obj_path(mesh)), **params) == RESULTS["cases"][case]["cache_name"]


@pytest.mark.parametrize("case", CASE_IDS)
def test_load_reads_the_reference_dat(case, tmp_path):
    raw = data(case + ".dat")
    layout, nodes, woop, tri = R.split_dat(raw)
    info = RESULTS["cases"][case]
    assert layout == 5 and (nodes.nbytes, woop.nbytes, tri.nbytes) == (info["nodes_bytes"], info["woop_bytes"],
                                                                      info["tri_index_bytes"])
    bvh = mrt.Bvh.load(os.path.join(G, case + ".dat"))
    for got, want in zip(bvh.buffers(), (nodes, woop, tri)):
        assert same_bytes(got, want)
    out = str(tmp_path / "again.dat")
    bvh.save(out)
    with open(out, "rb") as f:
        assert f.read() == raw


@pytest.mark.parametrize("case", CASE_IDS)
def test_stats_equal_the_reference_stats(case):
    """BVH::Stats and mrth_bvh_stats report four quantities in common."""
    mesh, params = build_params(case)
    s = mrt.Bvh.build(mrt.Scene.from_obj(obj_path(mesh)), **params).stats()
    info = RESULTS["cases"][case]
    assert s["inner_nodes"] == info["num_inner_nodes"]
    assert s["leaf_nodes"] == info["num_leaf_nodes"]
    assert s["tri_refs"] == info["num_tris"]
    assert int(np.float32(s["sah_cost"]).view(np.uint32)) == info["sah_cost_bits"]
    assert info["branching_factor"] == 2 and info["num_child_nodes"] == 2 * info["num_inner_nodes"]
    assert info["nodes_bytes"] == 64 * info["num_inner_nodes"]


# ---- the reference's CudaBVH arithmetic judging woop_common.hpp ------------------------------

def boxes_are_whole_triangles(case):
    """Whether the reference's boxes in this tree are the boxes of whole triangles, which is what
    a refit computes. Not where the spatial splits clipped a reference (the trees with more
    references than triangles), and not in big100, where the SAH overflows and the reference
    builder (and ours after it) leaves inverted, empty boxes on inner nodes."""
    info = RESULTS["cases"][case]
    return info["num_tris"] <= info["num_triangles"] and CASES[case][1] != "big100"


@pytest.mark.parametrize("case", CASE_IDS)
def test_host_refit_of_a_reference_tree_keeps_the_reference_bytes(case):
    """mrth_bvh_refit with the scene's own vertices recomputes every Woop row and every box of a
    tree that the reference built. The Woop rows must come out as the reference's CudaBVH wrote
    them, to the bit, in every tree, and every copy of a triangle that the spatial splits
    referenced several times must agree. So must all 64 bytes of every node wherever the
    reference's boxes are those of whole triangles (boxes_are_whole_triangles). Elsewhere refit
    cannot give the reference's boxes back, by its contract (mrt_host.h: the whole triangle's box
    also where the builder had clipped the reference): first difference slivers200 node word 49
    (node 3, c0.hi.x), ours 0x3f3a613b (0.72805, the triangle's) against 0x3e90ed60 (0.28306, clipped).
    There the boxes are the independent numpy refit's, to the bit, and contain the reference's."""
    mesh, _ = build_params(case)
    _, ref_nodes, ref_woop, ref_tri = R.split_dat(data(case + ".dat"))
    v, t, _ = mrt.Scene.from_obj(obj_path(mesh)).arrays()
    bvh = mrt.Bvh.load(os.path.join(G, case + ".dat"))
    bvh.refit(v, t)
    nodes, woop, tri = bvh.buffers()
    assert same_bytes(tri, ref_tri)
    assert same_bytes(woop, ref_woop), f"{case} woop: " + first_difference(woop, ref_woop)

    rows = {}
    for slot in R.triangle_slots(ref_woop):
        rows.setdefault(int(tri[slot]), set()).add(woop[4 * slot:4 * slot + 12].tobytes())
    assert all(len(r) == 1 for r in rows.values())
    assert len(rows) < RESULTS["cases"][case]["num_tris"] or boxes_are_whole_triangles(case) or mesh == "big100"

    if boxes_are_whole_triangles(case):
        assert same_bytes(nodes, ref_nodes), f"{case} nodes: " + first_difference(nodes, ref_nodes)
        return
    assert not same_bytes(nodes, ref_nodes)
    want_nodes, want_woop = U.np_refit(ref_nodes, ref_woop, ref_tri, v, t)
    assert same_bytes(nodes, want_nodes), f"{case} nodes: " + first_difference(nodes, want_nodes)
    assert same_bytes(want_woop, ref_woop)
    a, b = nodes.reshape(-1, 16), ref_nodes.reshape(-1, 16)
    assert same_bytes(a[:, 12:], b[:, 12:])
    ours, theirs = U.boxes(nodes), U.boxes(ref_nodes)          # [n, 2, (lo.x hi.x lo.y hi.y lo.z hi.z)]
    if mesh == "big100":
        assert (theirs[:, :, 0::2] > theirs[:, :, 1::2]).any()       # inverted boxes in the reference's tree
    else:
        assert (ours[:, :, 0::2] <= theirs[:, :, 0::2]).all() and (ours[:, :, 1::2] >= theirs[:, :, 1::2]).all()


def test_which_trees_hold_duplicated_references():
    dup = {c for c in CASE_IDS if RESULTS["cases"][c]["num_tris"] > RESULTS["cases"][c]["num_triangles"]}
    assert dup == {"random1500", "coincident40", "coplanar", "slivers200", "slivers200-maxleaf4", "slivers200-minleaf2"}


# ---- the smaller prize: pixel table and camera signature -------------------------------------

@pytest.mark.parametrize("size", sorted(RESULTS["pixel_tables"]))
def test_pixel_table_equals_the_reference(size):
    w, h = map(int, size.split("x"))
    both = np.frombuffer(data(f"pixeltable_{size}.bin"), np.int32)
    index_to_pixel, pixel_to_index = both[:w * h], both[w * h:]
    got = mrt.pixel_table(w, h)
    assert same_bytes(got, index_to_pixel)
    assert np.array_equal(pixel_to_index[index_to_pixel], np.arange(w * h))


@pytest.mark.parametrize("sig", sorted(RESULTS["cameras"]), ids=lambda s: s[:12])
def test_camera_signature_decodes_as_in_the_reference(sig):
    want = RESULTS["cameras"][sig]
    cam = mrt.Camera.from_signature(sig)
    f32 = lambda x: [int(b) for b in np.atleast_1d(np.asarray(x, np.float32)).view(np.uint32)]
    assert f32(cam.position) == want["position"] and f32(cam.forward) == want["forward"] and f32(cam.up) == want["up"]
    assert f32(cam.fov) + f32(cam.near) + f32(cam.far) == [want["fov"], want["near"], want["far"]]
    assert f32(cam.speed) == [want["speed"]] and cam.keep_aligned == bool(want["keep_aligned"])


# ---- with the binary present -----------------------------------------------------------------

needs_ref_host = pytest.mark.skipif(not os.path.exists(R.REF_HOST),
                                    reason="oracle/_ref/ref_host is not built (no reference tree on this machine)")


@needs_ref_host
def test_fixtures_regenerate_to_the_committed_bytes(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(G)))
    import make_ref_golden
    make_ref_golden.generate(str(tmp_path))
    made = sorted(os.listdir(tmp_path))
    assert set(made) == {f for f in os.listdir(G) if not f.endswith(".obj.gz")}
    for f in made:
        with open(tmp_path / f, "rb") as h:
            assert h.read() == data(f), f


@needs_ref_host
@pytest.mark.parametrize("case", ["random300", "slivers200", "big100", "tiny100", "degenerate90", "smallest"])
def test_the_reference_reads_what_save_writes(case, tmp_path):
    mesh, params = build_params(case)
    ours, back = str(tmp_path / "ours.dat"), str(tmp_path / "back.dat")
    mrt.Bvh.build(mrt.Scene.from_obj(obj_path(mesh)), **params).save(ours)
    info = R.run_ref(["reload", ours, back], case)
    assert info["layout"] == 5
    with open(ours, "rb") as a, open(back, "rb") as b:
        assert a.read() == b.read()


@needs_ref_host
def test_hash_buffer_equals_the_reference_on_files(tmp_path):
    for n in list(range(0, 26)) + [1000, 4099]:
        p = tmp_path / f"h{n}"
        p.write_bytes(bytes((i * 37 + 11) & 0xFF for i in range(n)))
        want = R.run_ref(["hash", p], f"{n} bytes")["hash_buffer"]
        buf = p.read_bytes()
        assert "%08x" % mrt._lib.host_lib().mrth_fw_hash_buffer(buf, n) == want, n


def both_routes(scene, what, tmp_path, **params):
    v, t, _ = scene.arrays()
    obj, ref, ours = (str(tmp_path / f"{what}.{ext}") for ext in ("obj", "ref.dat", "ours.dat"))
    R.write_obj(obj, v, t)
    info = R.run_ref(["bvh", obj, ref], what)
    loaded = mrt.Scene.from_obj(obj)
    mrt.Bvh.build(loaded, **params).save(ours)
    with open(ours, "rb") as a, open(ref, "rb") as b:
        got, want = a.read(), b.read()
    assert got == want, f"{what}: " + "; ".join(first_difference(x, y) for x, y in zip(R.split_dat(got)[1:],
                                                                                         R.split_dat(want)[1:]))
    assert mrt.Bvh.cache_name(loaded, **params) == info["cache_name"]
    return info, len(want)


@needs_ref_host
@pytest.mark.parametrize("name,param", [("mori", 0), ("random", 20000)])
def test_larger_scenes_build_to_the_reference_bytes(name, param, tmp_path):
    """The only multi-second test here: some 6 s of reference build in all."""
    both_routes(mrt.Scene.synthetic(name, param, 1), f"{name}{param}", tmp_path)


@needs_ref_host
def test_the_oversize_coplanar_case(tmp_path):
    """Too large to commit (about 1 MB for 300 triangles): the runaway spatial splits on coplanar
    triangles are the reference's own behaviour, reproduced reference for reference."""
    n, extent = R.COPLANAR_OVERSIZE
    info, size = both_routes(mrt.Scene.from_arrays(*R.coplanar(n, extent)), "coplanar-oversize", tmp_path)
    assert size > 200 * 1000 and info["num_tris"] > 10 * n
