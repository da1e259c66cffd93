"""The pointer checks the C-ABI exports share (csrc/api_checks.hpp): 16-byte alignment, whether two
buffers share a byte, and the two questions an export asks of its buffer tables — does an output
overlap an input, do two outputs overlap.

lib/api_checks_driver (tests/cpp/api_checks_driver.cpp, built by `make` with the host compiler
alone: that it compiles is the check that the header is free of HIP) prints what is asserted here,
over small literal addresses that are never dereferenced. The same source is built once more with
-fsanitize=address,undefined and run over the same cases: a stand-alone program. That run is what
the range ending at the last byte of the address space is for: start + bytes of it wraps to 0.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "gpu-ray-tracing_amd")
DRIVER = os.path.join(PKG, "lib", "api_checks_driver")
SOURCES = [os.path.join(REPO, "tests", "cpp", "api_checks_driver.cpp")]

TOP = 2**64            # one past the last byte of the address space


def run(driver, *ops):
    """One process for a list of ops (each a tuple of the op's name and its numbers): per line of
    output, a list of ints, or a dict for the k=v lines."""
    assert os.path.exists(driver), f"{driver} is missing: `make -C gpu-ray-tracing_amd` builds it"
    args = [str(a) for op in ops for a in op]
    p = subprocess.run([driver, *args], capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, f"{driver} {args}: exit {p.returncode}\n{p.stderr}"
    out = []
    for line, op in zip(p.stdout.splitlines(), ops):
        name, _, rest = line.partition(" ")
        assert name == op[0]
        if "=" in rest:
            out.append({k: int(v) for k, v in (w.split("=", 1) for w in rest.split())})
        else:
            out.append([int(w) for w in rest.split()])
    assert len(out) == len(ops)
    return out


def shares_a_byte(a, na, b, nb):
    """The definition, in integers that do not wrap."""
    return int(a != 0 and b != 0 and na > 0 and nb > 0 and a < b + nb and b < a + na)


# (a, bytes of a, b, bytes of b, whether they overlap)
PAIRS = [
    (0x1000, 64, 0x1000, 64, 1),          # identical
    (0x1000, 256, 0x1040, 16, 1),         # containment
    (0x1040, 16, 0x1000, 256, 1),
    (0x1000, 64, 0x103F, 64, 1),          # one byte shared at a's end
    (0x1000, 64, 0x0FC1, 64, 1),          # one byte shared at a's start
    (0x1000, 64, 0x1040, 64, 0),          # exactly adjacent, above and below
    (0x1000, 64, 0x0FC0, 64, 0),
    (0x1000, 1, 0x1001, 1, 0),
    (0x1000, 1, 0x1000, 1, 1),
    (0, 64, 0x1000, 64, 0),               # a null pointer never overlaps
    (0x1000, 64, 0, 64, 0),
    (0, 64, 0, 64, 0),
    (0, 2**40, 0x1000, 64, 0),            # not even where a range from address 0 would hold the other
    (0x1000, 0, 0x1000, 64, 0),           # a zero or negative length never overlaps
    (0x1000, 64, 0x1000, 0, 0),
    (0x1000, -64, 0x1000, 64, 0),
    (0x1000, 64, 0x1010, -1, 0),
    (0x1000, -(2**63), 0x1000, 64, 0),
    (TOP - 64, 64, 16, 64, 0),            # ends at the last byte of the address space: start + bytes is 0
    (TOP - 64, 64, 16, 2**40, 0),
    (TOP - 64, 64, TOP - 1, 1, 1),
    (TOP - 64, 64, TOP - 65, 1, 0),
    (TOP - 64, 64, TOP - 65, 2, 1),
    (16, 2**63 - 1, TOP - 64, 64, 0),     # the longest length there is stops short of it
    (16, 2**63 - 1, 2**63 + 14, 2, 1),
    (16, 2**63 - 1, 2**63 + 15, 2, 0),
]


def check_pairs(driver):
    for (a, na, b, nb, want), got in zip(PAIRS, run(driver, *[("overlap", a, na, b, nb) for a, na, b, nb, _ in PAIRS])):
        assert want == shares_a_byte(a, na, b, nb), "the case contradicts the definition"
        assert got == [want, want], (hex(a), na, hex(b), nb)      # and the answer is symmetric


def check_sweep(driver):
    """Every placement of a short range against [0x100, 0x108): before, touching, inside, past."""
    cases = [(0x100, 8, b, nb) for b in range(0xF8, 0x110) for nb in (1, 3, 8, 16)]
    for (a, na, b, nb), got in zip(cases, run(driver, *[("overlap", *c) for c in cases])):
        want = shares_a_byte(a, na, b, nb)
        assert got == [want, want], (hex(b), nb)


# three inputs and three outputs, 64 bytes each, far apart; a case moves one buffer
INS = [(0x10000, 64), (0x20000, 64), (0x30000, 64)]
OUTS = [(0x40000, 64), (0x50000, 64), (0x60000, 64)]


def table(ins=INS, outs=OUTS):
    return ("table", *[w for span in (*ins, *outs) for w in span])


def moved(spans, i, span):
    return [span if k == i else s for k, s in enumerate(spans)]


def check_tables(driver):
    cases = [(table(), dict(oi=0, oo=0, any=0))]
    for o in range(3):
        for i in range(3):     # output o over the last byte of input i: only the first question fires
            cases.append((table(outs=moved(OUTS, o, (INS[i][0] + 63, 64))), dict(oi=1, oo=0, any=1)))
        for o2 in range(o + 1, 3):   # output o2 over the last byte of output o: only the second
            cases.append((table(outs=moved(OUTS, o2, (OUTS[o][0] + 63, 64))), dict(oi=0, oo=1, any=1)))
            cases.append((table(outs=moved(OUTS, o, (OUTS[o2][0] + 63, 64))), dict(oi=0, oo=1, any=1)))
    cases += [
        (table(ins=moved(INS, 0, (0x20000, 64))), dict(oi=0, oo=0, any=0)),          # two inputs may overlap
        (table(outs=moved(OUTS, 1, (0, 2**40))), dict(oi=0, oo=0, any=0)),           # an absent output
        (table(outs=moved(OUTS, 1, (0x10000, 0))), dict(oi=0, oo=0, any=0)),         # an empty one
        (table(outs=[(0x10000, 64), (0x10020, 64), (0x60000, 64)]), dict(oi=1, oo=1, any=1)),   # both at once
        (table(outs=moved(OUTS, 2, (TOP - 64, 64))), dict(oi=0, oo=0, any=0)),       # no wrap onto the low buffers
    ]
    for (op, want), got in zip(cases, run(driver, *[c[0] for c in cases])):
        assert got == want, op


ALIGNED = [(0, 1), (16, 1), (0x100000, 1), (8, 0), (0x100008, 0), (1, 0), (15, 0), (17, 0), (TOP - 16, 1), (TOP - 1, 0)]


def check_aligned(driver):
    assert run(driver, *[("aligned", a) for a, _ in ALIGNED]) == [[want] for _, want in ALIGNED]


def test_overlap_on_pairs_of_ranges():
    check_pairs(DRIVER)


def test_overlap_sweep_across_a_range():
    check_sweep(DRIVER)


def test_each_question_fires_alone_on_a_table():
    check_tables(DRIVER)


def test_aligned16():
    check_aligned(DRIVER)


# ---------------------------------------------------------------- the same cases under the sanitizers
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host compiler"
    exe = str(tmp_path_factory.mktemp("api_checks_san") / "api_checks_driver_san")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I" + os.path.join(REPO, "include"), "-o", exe, *SOURCES], check=True)
    return exe


def test_the_cases_under_address_and_undefined_sanitizers(sanitized):
    check_pairs(sanitized)
    check_sweep(sanitized)
    check_tables(sanitized)
    check_aligned(sanitized)
