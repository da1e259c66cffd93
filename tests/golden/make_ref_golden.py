"""Regenerate tests/golden/ref/: the fixtures written by the reference's own compiled host code.

    make -C oracle                                   # builds oracle/_ref/ref_host where the reference tree is
    python tests/golden/make_ref_golden.py           # rewrites every fixture from tests/ref_meshes.py
    python tests/golden/make_ref_golden.py --from-obj OUT       # the committed .obj.gz files -> OUT (what the tests do)
    python tests/golden/make_ref_golden.py --coplanar-search    # the largest coplanar count under 200 KB
    python tests/golden/make_ref_golden.py --smallest-search    # the smallest count the reference survives

Per mesh: <name>.obj.gz (the input, gzipped), <name>.scene.bin (ref_host scene). Per case: <case>.dat
(ref_host bvh). ref_results.json holds the binary's JSON lines, the pixel tables' sizes and the camera
signatures decoded by CameraControls::decodeSignature; pixeltable_<w>x<h>.bin the two pixel tables.
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_meshes as R  # noqa: E402

PIXEL_TABLES = [(8, 8), (13, 9), (24, 40), (33, 17), (64, 48)]
LIMIT = 200 * 1000


def camera_signatures():
    out = []
    with open(os.path.join(HERE, "camera_signatures.txt")) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                sig = line.rstrip("\n").split("\t")[1]
                if sig not in out:
                    out.append(sig)
    return out


def generate(out_dir):
    """Run the binary over the committed .obj.gz files; every other fixture lands in out_dir."""
    lines = []
    for name in R.MESHES:
        lines.append(("scenes", name, R.run_ref(["scene", R.obj_path(name), os.path.join(out_dir, name + ".scene.bin")],
                                                name)))
    for case, mesh, min_leaf, max_leaf, alpha in R.CASES:
        lines.append(("cases", case, R.run_ref(["bvh", R.obj_path(mesh), os.path.join(out_dir, case + ".dat"), min_leaf,
                                                max_leaf, repr(alpha)], case)))
    for w, h in PIXEL_TABLES:
        lines.append(("pixel_tables", f"{w}x{h}", R.run_ref(["pixeltable", w, h,
                                                             os.path.join(out_dir, f"pixeltable_{w}x{h}.bin")], f"{w}x{h}")))
    for sig in camera_signatures():
        lines.append(("cameras", sig, R.run_ref(["camera", sig], sig)))
    with open(os.path.join(out_dir, "ref_results.json"), "w") as f:
        for line in lines:
            f.write(json.dumps(line, sort_keys=True) + "\n")


def dat_size(vertices, indices, what):
    with tempfile.TemporaryDirectory() as d:
        obj, dat = os.path.join(d, "m.obj"), os.path.join(d, "m.dat")
        R.write_obj(obj, vertices, indices)
        r = subprocess.run([R.REF_HOST, "bvh", obj, dat], capture_output=True, timeout=60)
        return os.path.getsize(dat) if r.returncode == 0 else r.returncode


def main():
    assert os.path.exists(R.REF_HOST), "build oracle/_ref/ref_host first (make -C oracle, with the reference tree present)"
    if sys.argv[1:2] == ["--from-obj"]:
        generate(sys.argv[2])
        return
    if sys.argv[1:2] == ["--coplanar-search"]:
        for n in range(10, 301, 5):
            size = dat_size(*R.coplanar(n), f"coplanar {n}")
            print(n, size, flush=True)
            if size >= LIMIT:
                break
        return
    if sys.argv[1:2] == ["--smallest-search"]:
        for n in range(1, 6):
            print(n, dat_size(*R.random_soup(n, 29), f"random {n}"), "(negative: killed by that signal)")
        return
    os.makedirs(R.GOLDEN_REF, exist_ok=True)
    with tempfile.TemporaryDirectory() as d:
        for name, make in R.MESHES.items():
            R.write_obj(os.path.join(d, name + ".obj"), *make())
            R.pack_obj(os.path.join(d, name + ".obj"), name)
    generate(R.GOLDEN_REF)
    total = 0
    for f in sorted(os.listdir(R.GOLDEN_REF)):
        size = os.path.getsize(os.path.join(R.GOLDEN_REF, f))
        total += size
        print(f"{size:8d} {f}" + ("   OVER THE 200 KB LIMIT" if size >= LIMIT else ""))
    print(f"{total:8d} total")


if __name__ == "__main__":
    main()
