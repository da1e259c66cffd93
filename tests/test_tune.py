"""The launch-schedule autotuner (csrc/tune.cpp) on the CPU.

lib/tune_driver (tests/cpp/tune_driver.cpp, built by `make` from tune.cpp alone with the
host compiler: that it links shows the unit has no HIP in it) plays launches against the
tuner under a time model from its command line. The sequences in
tests/golden/tune_sequences.json were recorded from the code as it was moved out of
mrt_api.cpp, before any restructuring; `python tests/test_tune.py --record` wrote them.
"""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, "gpu-ray-tracing_amd", "lib", "tune_driver")
GOLDEN = os.path.join(REPO, "tests", "golden", "tune_sequences.json")

SCHEDULES, STAGE2, STAGE3, RUN, SAMPLES = 8, 5, 6, 4, 8
BASE = "1.0,.95,1.2,1.3,1.3,.90,1.1,1.4"
KEY = ["1000", "7", "1"]          # rays, variant, stream of the scenarios' one key
# name: (time model, rays) — rule 0 unless said otherwise
SCENARIOS = {
    "equal": ([], "1000"),
    "equal-rule3": (["--bvh-mb", "512", "--rule", "3"], "2000000"),
    "sched5-2pct": (["--base", "1,1,1,1,1,.98,1,1"], "1000"),
    "mods-1pct-slower": (["--base", BASE, "--mod", "1.01,1.01,1.01,1.01,1.01"], "1000"),
    "mod3-10pct": (["--base", BASE, "--mod", "1,1,1,.9,1"], "1000"),
    "mod3-30pct-on-6": (["--base", BASE, "--mod", "1,1,1,.9,1", "--pair", "6:3:.7"], "1000"),
    "pair-1-4": (["--base", BASE, "--pair", "1:4:.8"], "1000"),
}
LAGS = (0, 3, 12)
LAUNCHES = 400
# scenario: (locked candidate, autotune_candidate, exported candidate), the issue's figures
SETTLED = {
    "equal": (0, 0x0, 0),
    "equal-rule3": (3, 0x3, 3 | 3 << 8),
    "sched5-2pct": (0, 0x0, 0),
    "mods-1pct-slower": (5, 0x5, 5 | 5 << 8),
    "mod3-10pct": (11, 0x50b, 11 | 5 << 8),
    "mod3-30pct-on-6": (11, 0x60b, 11 | 6 << 8),
    "pair-1-4": (12, 0x10c, 12 | 1 << 8),
}


def drive(*args):
    """The driver's output lines as lists of words; key=value words become dict entries."""
    assert os.path.exists(DRIVER), f"{DRIVER} is missing: `make -C gpu-ray-tracing_amd` builds it"
    out = subprocess.run([DRIVER, *map(str, args)], capture_output=True, text=True, check=True).stdout
    lines = []
    for line in out.splitlines():
        words = line.split()
        lines.append((words[0], dict(w.split("=", 1) for w in words[1:] if "=" in w), line))
    return lines


def launches(lines):
    return [kv for tag, kv, _ in lines if tag == "launch"]


def states(lines):
    return [kv for tag, kv, _ in lines if tag == "state"]


def scenario(name, lag, n=LAUNCHES):
    model, rays = SCENARIOS[name]
    return drive(*model, "--lag", lag, "launch", rays, *KEY[1:], n, "export")


def tokens(lines):
    return " ".join(f"{l['cand']}:{l['info']}:{l['locked']}:{l['slot']}" for l in launches(lines))


def first_locked(ls):
    return next(i for i, l in enumerate(ls) if l["locked"] == "1")


@pytest.fixture(scope="module")
def runs():
    return {(name, lag): scenario(name, lag) for name in SCENARIOS for lag in LAGS}


@pytest.mark.parametrize("lag", LAGS)
@pytest.mark.parametrize("name", SCENARIOS)
def test_sequence_is_the_recorded_one(runs, name, lag):
    """Candidate, reported encoding, locked flag and timing slot of every launch."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert tokens(runs[name, lag]) == golden[f"{name} lag {lag}"]


def stage_order(first, count):
    """A stage's launches until every candidate has SAMPLES timings read by the next launch: whole
    cycles of runs of RUN, the last run cut after the launch that brings the last sample."""
    cycles = -(-SAMPLES // (RUN - 1))
    order = [c for _ in range(cycles) for c in range(first, first + count) for _ in range(RUN)]
    return order[:len(order) - (RUN - 1 - (SAMPLES - (cycles - 1) * (RUN - 1)))]


def test_exploration_order(runs):
    ls = launches(runs["mod3-10pct", 0])
    cands = [int(l["cand"]) for l in ls]
    timed = [l["slot"] != "-1" for l in ls]
    untimed_cycle = [c for c in range(SCHEDULES) for _ in range(RUN)]
    stage1 = untimed_cycle + stage_order(0, SCHEDULES)
    assert len(stage1) == 127 and stage1[-3:] == [7, 7, 7] and stage1[-4] == 6   # the last run: 3 launches
    assert cands[:127] == stage1
    stage2 = stage_order(SCHEDULES, 2 * STAGE2)
    assert cands[127:246] == stage2 and len(stage2) == 119 and stage2[-4:] == [16, 17, 17, 17]
    stage3 = stage_order(SCHEDULES + 2 * STAGE2, STAGE3)
    assert cands[246:317] == stage3 and stage3[-4:] == [22, 23, 23, 23]
    assert first_locked(ls) == 317 and all(l["locked"] == "1" and l["cand"] == "11" for l in ls[317:])
    # timed: never in the first cycle, never the first launch of a run, never once locked
    pos = 0
    for i in range(317):
        if i in (127, 246):
            pos = 0
        assert timed[i] == (i >= SCHEDULES * RUN and pos % RUN != 0), i
        pos += 1
    assert not any(timed[317:])
    # the stage changes are seen by launches 127, 246 and 317
    st = states(runs["mod3-10pct", 0])
    assert [(s["stage1"], s["stage1b"], s["stage2"], s["locked"]) for s in st] == [
        ("-1", "-1", "-1", "-1"), ("5", "1", "-1", "-1"), ("5", "1", "11", "-1"), ("5", "1", "11", "11")]
    assert st[2]["s3mod"] == "3" and st[2]["s3sched"] == "0,2,3,4,6,7"


def test_no_modifier_clears_the_margin_locks_after_stage_2(runs):
    ls = launches(runs["equal", 0])
    assert first_locked(ls) == 246
    assert [int(l["cand"]) for l in ls[:246]] == ([c for c in range(SCHEDULES) for _ in range(RUN)]
                                                  + stage_order(0, SCHEDULES) + stage_order(SCHEDULES, 2 * STAGE2))


@pytest.mark.parametrize("lag", LAGS)
@pytest.mark.parametrize("name", SCENARIOS)
def test_settled_choice(runs, name, lag):
    """The same final choice whatever the completion lag."""
    lines = runs[name, lag]
    locked, info, exported = SETTLED[name]
    last = launches(lines)[-1]
    assert (last["locked"], int(last["cand"]), int(last["info"], 16)) == ("1", locked, info)
    ex = [kv for tag, kv, _ in lines if tag == "exported"]
    assert [(int(e["candidate"]), e["version"]) for e in ex] == [(exported, "11")]


def test_stage_winners(runs):
    def final(name):
        s = states(runs[name, 0])
        return s[1]["stage1"], s[1]["stage1b"], s[-1]
    assert final("equal")[:2] == ("0", "1")
    assert final("equal-rule3")[:2] == ("3", "0")
    assert final("sched5-2pct")[:2] == ("0", "5")         # inside the margin the rule stays
    assert final("mods-1pct-slower")[:2] == ("5", "1")
    s1, s1b, last = final("mod3-30pct-on-6")
    assert (s1, s1b, last["stage2"], last["stage1"], last["locked"]) == ("5", "1", "11", "6", "11")
    s1, s1b, last = final("pair-1-4")                     # the runner-up's copy wins, stored canonically
    assert (s1, s1b, last["stage2"], last["stage1"], last["locked"]) == ("5", "1", "17", "1", "12")


def test_no_completion_ever():
    """The 16 slots fill up, launches go on cycling untimed, nothing locks."""
    ls = launches(drive("--lag", "never", "launch", *KEY, 300))
    slots = [int(l["slot"]) for l in ls]
    assert sorted(s for s in slots if s >= 0) == list(range(16))
    assert all(s == -1 for s in slots[SCHEDULES * RUN + 22:])     # 16 timed launches in runs of 1 + 3
    assert all(l["locked"] == "0" for l in ls)
    assert [int(l["cand"]) for l in ls] == [c for _ in range(10) for c in range(SCHEDULES) for _ in range(RUN)][:300]
    assert ls[-1]["explored"] == "300"


def cfg_lines(lines, tag):
    return [kv for t, kv, _ in lines if t == tag]


def test_schedule_table_known_answers():
    rows = cfg_lines(drive("--xcds", 8, "schedules"), "schedule")
    got = [(int(r["queues"]), int(r["threshold"]), int(r["waves"]), int(r["block"]), int(r["shared"])) for r in rows]
    # waves 0 without queues: the static strided rounds' own 20 waves/CU (kStridedWaves, applied by grid_blocks)
    assert rows[0]["strided_waves"] == "20"
    assert got == [(-1, 0, 0, 0, 0), (-1, 0, 8, 0, 0), (8, 56, 20, 8192, 0), (1, 48, 16, 0, 0), (1, 48, 12, 0, 0),
                   (-1, 0, 16, 0, 0), (-1, 0, 12, 0, 0), (1, 48, 20, 0, 0)]
    assert all(r["groups"] == "1" and r["slack"] == "2" and r["tail"] == "16" for r in rows)
    assert cfg_lines(drive("--xcds", 1, "schedules"), "schedule")[2]["queues"] == "1"
    assert cfg_lines(drive("--xcds", 32, "schedules"), "schedule")[2]["queues"] == "8"


@pytest.mark.parametrize("mb,rays,index", [(512, 307200, 4), (512, 786432, 4), (512, 786433, 3), (512, 2073600, 3),
                                           (256, 2073600, 0), (100, 307200, 0)])
def test_rule_agrees_with_the_table(mb, rays, index):
    """The table row the rule maps to is the rule's own configuration (256 CUs: 3 rays per lane
    of the 16-wave grid are 786 432 rays)."""
    lines = drive("--bvh-mb", mb, "--cus", 256, "rule", rays)
    assert lines[0][1]["index"] == str(index)
    assert lines[1][1] == lines[2][1]
    want = {0: ("-1", "0", "0"), 3: ("1", "48", "16"), 4: ("1", "48", "12")}[index]
    assert (lines[1][1]["queues"], lines[1][1]["threshold"], lines[1][1]["waves"]) == want


def test_modifiers_respect_caller_set_knobs():
    def mod(k, *cfg):
        return cfg_lines(drive(*cfg, "modifier", 1, k), "modifier")[0]
    assert [mod(k)["slack"] for k in range(5)] == ["4", "6", "2", "2", "6"]
    assert [mod(k)["tail"] for k in range(5)] == ["16", "16", "0", "16", "16"]
    assert [mod(k)["groups"] for k in range(5)] == ["1", "1", "1", "16", "2"]
    assert all(mod(k)["waves"] == "8" for k in range(5))
    slack = ("cfg", "spec_slack", 5)
    assert [mod(k, *slack)["slack"] for k in (0, 1, 4)] == ["5", "5", "5"] and mod(4, *slack)["groups"] == "1"
    assert mod(2, "cfg", "tail_lanes", 8)["tail"] == "8"
    # a distribution knob set by the caller: not tuned at all
    for knob in (("lane_groups", 2), ("num_queues", 1), ("waves_per_cu", 8), ("fetch_threshold", 32), ("autotune", 0)):
        assert launches(drive("cfg", *knob, "launch", *KEY))[0]["cand"] == "-1", knob
    assert launches(drive("flags", 8, "launch", *KEY))[0]["cand"] == "-1"      # MRT_TRACE_STATS


def imp(*entries):
    return ["import", len(entries)] + [x for e in entries for x in (*e, 11)]


def test_inheritance_takes_the_nearest_settled_size():
    table = imp((32000, 7, 1), (34000, 7, 5))
    def first(rays, variant=7, flags=0):
        return launches(drive(*table, "flags", flags, "launch", rays, variant, 1))[0]
    assert (first(33100)["cand"], first(33100)["locked"]) == ("5", "1")
    assert first(32900)["cand"] == "1"
    assert first(33000)["cand"] == "1"                    # a tie: the smaller batch size
    assert first(31000)["cand"] == "1"                    # gap * 32 == the settled size
    assert (first(30999)["cand"], first(30999)["locked"]) == ("0", "0")
    assert first(35062)["cand"] == "5" and first(35063)["locked"] == "0"
    assert first(33100, variant=3)["locked"] == "0"       # another variant
    assert first(33100, flags=16)["locked"] == "0"        # no inheritance across the secondary class
    sec = launches(drive(*imp((32000, 7 | 512, 1)), "flags", 16, "launch", 32100, 7, 1, "flags", 0, "launch", 32200, 7, 1))
    assert [l["locked"] for l in sec] == ["1", "0"]


def test_inherited_entries_are_not_exported_imported_ones_are():
    lines = drive(*imp((32000, 7, 5 | 5 << 8)), "launch", 32100, 7, 1, "export", *imp((32100, 7, 3 | 3 << 8)), "export")
    assert [kv["inherited"] for kv in states(lines)] == ["1"]
    exports = [kv["n"] for tag, kv, _ in lines if tag == "export"]
    assert exports == ["1", "2"]
    ex = [(kv["rays"], kv["candidate"]) for tag, kv, _ in lines if tag == "exported"]
    assert ex == [("32000", str(5 | 5 << 8)), ("32000", str(5 | 5 << 8)), ("32100", str(3 | 3 << 8))]


def test_second_stream():
    before = launches(drive("launch", *KEY, 5, "launch", 1000, 7, 2, "launch", *KEY, 2))
    assert [l["cand"] for l in before] == ["0", "0", "0", "0", "1", "-1", "-1", "-1"]   # the rule, and it stays
    assert before[4]["explored"] == "5"
    after = launches(drive(*imp((1000, 7, 11 | 5 << 8)), "launch", *KEY, "launch", 1000, 7, 2, "launch", *KEY))
    assert [(l["cand"], l["info"], l["locked"]) for l in after] == [("11", "0x50b", "1")] * 3


def test_the_65th_key_gets_the_rule():
    ops = [x for i in range(65) for x in ("launch", 100000 * (i + 1), 7, 1)]
    ls = launches(drive(*ops, *imp((7, 7, 0))))
    assert [l["cand"] for l in ls] == ["0"] * 64 + ["-1"]
    assert cfg_lines(drive(*ops, *imp((7, 7, 0))), "import")[0]["rc"] == "5"         # MRT_ERR_TOO_LARGE


@pytest.mark.parametrize("bad", [(1000, 7, 0, 10), (1000, 7, 0, 12), (0, 7, 0, 11), (-5, 7, 0, 11), (1000, 7, 13, 11),
                                 (1000, 7, 12 | 8 << 8, 11), (1000, 7, -1, 11)])
def test_import_refuses_bad_entries_and_changes_nothing(bad):
    lines = drive("import", 2, 2000, 7, 12 | 7 << 8, 11, *bad, "export")
    assert cfg_lines(lines, "import")[0] == {"rc": "1", "keys": "0"}                   # MRT_ERR_INVALID_ARG
    assert cfg_lines(lines, "export")[0]["n"] == "0"
    good = drive("import", 1, 2000, 7, 12 | 7 << 8, 11, "export")
    assert cfg_lines(good, "import")[0] == {"rc": "0", "keys": "1"}
    assert cfg_lines(good, "exported")[0]["candidate"] == str(12 | 7 << 8)


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    with open(GOLDEN, "w") as f:
        json.dump({f"{name} lag {lag}": tokens(scenario(name, lag)) for name in SCENARIOS for lag in LAGS}, f, indent=0)
        f.write("\n")
