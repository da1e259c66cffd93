"""The meshes on which the reference's own compiled host code (oracle/_ref/ref_host, built by
oracle/Makefile where the reference tree is present) judges this project's host chain.

MESHES maps a name to (vertices float32 [n,3], indices int32 [m,3]); CASES lists every build
(case id, mesh, min_leaf, max_leaf, split_alpha). tests/golden/make_ref_golden.py writes each
mesh as <name>.obj, commits it gzipped (<name>.obj.gz, the same bytes) and runs the binary over
it; the tests read the committed files through obj_path(), so the fixtures do not hang on numpy's
random stream staying what it is.

No mesh holds a NaN or an infinite coordinate: the reference's builder has no guard against
them, and a hung oracle proves nothing.

The reference program dies (SIGSEGV) on scenes of one and of two triangles, and survives three
(SMALLEST_REF_SAFE, found by trying 1, 2, 3 with the binary). One- and two-triangle scenes stay
covered by this project's own tests (test_gpu_edge_geometry.py, test_refit.py, test_lbvh.py);
the reference is not "fixed" to reach them.
"""
import functools
import gzip
import os
import tempfile

import numpy as np

GOLDEN_REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref")
REF_HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "ref_host")

SMALLEST_REF_SAFE = 3
# Coplanar triangles make the spatial splits run away, in the reference's builder and in ours
# alike, and erratically in the count: with extent 0.5, 240 triangles make a 183 KB .dat (the
# largest below 200 KB among the counts up to 250 in steps of 5: make_ref_golden.py
# --coplanar-search) while 245 make 83 KB. 300 triangles of extent 2 make 994 KB, too large to
# commit: that case runs only where the binary is present.
COPLANAR_COMMITTED = 240
COPLANAR_OVERSIZE = (300, 2.0)

DEFAULT_PARAMS = (1, 8, 1e-5)
# split_alpha = 1: no spatial splits; max_leaf = 4; min_leaf = 2.
PARAM_SETS = {"nosplit": (1, 8, 1.0), "maxleaf4": (1, 4, 1e-5), "minleaf2": (2, 8, 1e-5)}


def _soup(tris):
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    return tris.reshape(-1, 3), np.arange(3 * len(tris), dtype=np.int32).reshape(-1, 3)


def random_soup(n, seed, extent=0.15, quantum=None):
    rng = np.random.default_rng(seed)
    tris = rng.uniform(-1, 1, (n, 1, 3)) + rng.uniform(-extent, extent, (n, 3, 3))
    if quantum:
        tris = np.round(tris / quantum) * quantum     # shorter decimals: keeps the .obj small
    return _soup(tris)


def coincident(n):
    return _soup(np.tile(np.array([[0.25, 0.5, 0.125], [1.5, 0.75, 0.375], [0.5, 1.75, 0.625]], np.float32), (n, 1, 1)))


def degenerate_mix(n=90, seed=7):
    """A third proper triangles, a third zero-area (collinear) ones, a third zero-length (a point)."""
    rng = np.random.default_rng(seed)
    k = n // 3
    proper = rng.uniform(-1, 1, (k, 1, 3)) + rng.uniform(-0.2, 0.2, (k, 3, 3))
    a = rng.uniform(-1, 1, (k, 3)).astype(np.float32)
    d = rng.uniform(-0.25, 0.25, (k, 3)).astype(np.float32)
    line = np.stack([a, a + d, a + 2 * d], axis=1)            # float32 sums: collinear up to rounding
    line[::2, 2] = line[::2, 1]                               # every other one has two equal vertices too
    p = rng.uniform(-1, 1, (n - 2 * k, 1, 3))
    point = np.repeat(p, 3, axis=1)
    tris = np.concatenate([proper, line, point]).astype(np.float32)
    return _soup(tris[rng.permutation(n)])


def same_centroid(n=30, seed=11):
    rng = np.random.default_rng(seed)
    tris = rng.integers(-64, 65, (n, 3, 3)).astype(np.float32)
    tris[:, 2] = -(tris[:, 0] + tris[:, 1])                   # exact: every centroid is the origin
    return _soup(tris / 64)


def slivers(n=200, seed=13):
    """Long thin parallel diagonals, stacked across their length: the case that forces spatial
    splits (the reference duplicates them into some 600 references)."""
    rng = np.random.default_rng(seed)
    along, across = np.array([1, 1, 0]) / np.sqrt(2), np.array([1, -1, 0]) / np.sqrt(2)
    a = np.linspace(-1, 1, n)[:, None] * across + rng.uniform(-0.05, 0.05, (n, 3))
    half = rng.uniform(0.5, 1.0, (n, 1)) * along
    w = rng.uniform(-0.004, 0.004, (n, 3))
    return _soup(np.stack([a - half, a + half, a + half + w], axis=1))


def scaled(scale, n=100, seed=17):
    v, t = random_soup(n, seed)
    return (v * np.float32(scale)).astype(np.float32), t


def grid(nx=20, ny=20):
    """One triangle per cell of an nx-by-ny grid over shared (indexed) vertices."""
    xs, ys = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    v = np.stack([xs, ys, (xs * 3 + ys * 5) % 7 / 8], axis=-1).reshape(-1, 3).astype(np.float32)
    vid = lambda i, j: i * (ny + 1) + j
    t = [[vid(i, j), vid(i + 1, j), vid(i, j + 1)] for i in range(nx) for j in range(ny)]
    return v, np.array(t, np.int32)


def indexed_repeats(seed=19):
    """An indexed mesh whose index list repeats triples (whole, rotated and reversed) and holds
    degenerate ones: (i, i, j) and (i, i, i)."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
    t = [list(rng.choice(40, 3, replace=False)) for _ in range(60)]
    t += [t[k] for k in (0, 0, 5, 9)]
    t += [t[3][1:] + t[3][:1], t[4][::-1]]
    t += [[k, k, k + 1] for k in range(0, 12, 2)] + [[k, k, k] for k in (7, 7, 21)]
    t = np.array(t, np.int32)
    return v, t[rng.permutation(len(t))]


def coplanar(n, extent=0.5, seed=23):
    rng = np.random.default_rng(seed)
    tris = rng.uniform(-1, 1, (n, 1, 3)) + rng.uniform(-extent, extent, (n, 3, 3))
    tris[:, :, 1] = 0
    return _soup(tris)


MESHES = {
    "random300": lambda: random_soup(300, 1),
    "random1500": lambda: random_soup(1500, 2, quantum=1 / 256),
    "coincident9": lambda: coincident(9),
    "coincident40": lambda: coincident(40),
    "degenerate90": degenerate_mix,
    "samecentroid30": same_centroid,
    "slivers200": slivers,
    "big100": lambda: scaled(1e30),
    "tiny100": lambda: scaled(1e-30),
    "grid20x20": grid,
    "indexed": indexed_repeats,
    "coplanar": lambda: coplanar(COPLANAR_COMMITTED),
    "smallest": lambda: random_soup(SMALLEST_REF_SAFE, 29),
    # Coordinates of 1e-12: areas are fine (1e-24), but the Woop matrix's determinant (1e-48)
    # underflows to zero, its reciprocal is taken as 0 (Math.hh:113) and every row is a zero
    # with the sign of its cofactor. 25 of the 60 Z rows would start with -0.0, the terminator's
    # mark, but for the -0.0 -> +0.0 guard (CudaBVH.cc:316-317): no other mesh here needs it.
    "guard60": lambda: scaled(1e-12, n=60, seed=31),
}

CASES = [(name, name) + DEFAULT_PARAMS for name in MESHES]
CASES += [(f"{mesh}-{tag}", mesh) + p for mesh in ("slivers200", "random300") for tag, p in PARAM_SETS.items()]


def write_obj(path, vertices, indices):
    """%.9g prints a float32 so that a correctly rounding reader gets it back; whatever the
    reference's own number parser makes of the text, both sides read the same file."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    assert np.isfinite(v).all(), "no NaN or infinite coordinates: the reference's builder has no guard"
    with open(path, "w") as f:
        for p in v:
            f.write("v %.9g %.9g %.9g\n" % tuple(float(x) for x in p))
        for t in np.asarray(indices).reshape(-1, 3):
            f.write("f %d %d %d\n" % tuple(int(i) + 1 for i in t))


def pack_obj(path, mesh):
    """Commit an .obj: the same bytes gzipped, with no name or time in the header."""
    with open(path, "rb") as f, open(os.path.join(GOLDEN_REF, mesh + ".obj.gz"), "wb") as out:
        with gzip.GzipFile(filename="", mode="wb", fileobj=out, mtime=0) as z:
            z.write(f.read())


@functools.lru_cache(maxsize=None)
def _unpacked():
    return tempfile.TemporaryDirectory(prefix="ref_obj_")


@functools.lru_cache(maxsize=None)
def obj_path(mesh):
    """The committed <mesh>.obj.gz as a file (the importers take paths), unpacked once a process."""
    path = os.path.join(_unpacked().name, mesh + ".obj")
    with gzip.open(os.path.join(GOLDEN_REF, mesh + ".obj.gz"), "rb") as z, open(path, "wb") as f:
        f.write(z.read())
    return path


def load_results():
    """ref_results.json: one JSON line [section, key, what the binary printed] per run."""
    import json
    results = {"scenes": {}, "cases": {}, "pixel_tables": {}, "cameras": {}}
    with open(os.path.join(GOLDEN_REF, "ref_results.json")) as f:
        for line in f:
            section, key, value = json.loads(line)
            results[section][key] = value
    return results


def run_ref(args, what):
    """Run oracle/_ref/ref_host; its JSON line. A timeout, a signal or an error fails the test
    and names the mesh."""
    import json
    import subprocess
    try:
        r = subprocess.run([REF_HOST] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    except subprocess.TimeoutExpired:
        raise AssertionError(f"ref_host {args[0]} timed out on {what}")
    assert r.returncode == 0, f"ref_host {args[0]} on {what}: exit status {r.returncode}\n{r.stderr[-500:]}"
    return json.loads(r.stdout.strip().splitlines()[-1])


def split_dat(data: bytes):
    """A reference .dat (CudaBVH::serialize): S32 layout, then three Buffers, each an S64 byte
    count and the bytes. Returns (layout, nodes, woop, triIndex) with int32 arrays."""
    layout = int(np.frombuffer(data, np.int32, 1, 0)[0])
    ofs, out = 4, []
    for _ in range(3):
        n = int(np.frombuffer(data, np.int64, 1, ofs)[0])
        out.append(np.frombuffer(data, np.int32, n // 4, ofs + 8).copy())
        ofs += 8 + n
    assert ofs == len(data)
    return (layout, *out)


def split_scene(data: bytes, nt: int, nv: int):
    """ref_host scene's dump: the five Scene buffers in declaration order."""
    a = np.frombuffer(data, np.uint8)
    cuts = np.cumsum([0, nt * 12, nt * 12, nt * 4, nt * 4, nv * 12])
    assert cuts[-1] == len(a)
    part = [a[cuts[i]:cuts[i + 1]] for i in range(5)]
    return (part[0].view(np.int32).reshape(-1, 3), part[1].view(np.float32).reshape(-1, 3), part[2].view(np.uint32),
            part[3].view(np.uint32), part[4].view(np.float32).reshape(-1, 3))


def triangle_slots(woop):
    """First Woop slot of every triangle reference, in buffer order: a leaf's references take
    three slots each, then one terminator slot whose first word is -0.0 (a reference's first
    word never is: CudaBVH.cc:316-317 turns it into +0.0)."""
    first = np.ascontiguousarray(woop).view(np.uint32).reshape(-1, 4)[:, 0]
    slots, s = [], 0
    while s < len(first):
        if first[s] == 0x80000000:
            s += 1
        else:
            slots.append(s)
            s += 3
    assert s == len(first)
    return slots
