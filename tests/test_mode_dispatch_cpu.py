"""The launch scaffold of the single-kernel modes (volume-renderer_amd/csrc/mode_dispatch.h) on the CPU: which template instance
each runtime combination of layout, filter, flag, 64-bit offsets and reslice mode reaches -- an axis no frame can show (skipping
on and off, 64-bit offsets on a small volume give identical frames) -- the 16x16-pixel tile counts and the two division modes.
tests/mode_dispatch/dispatch_check.cpp is compiled with g++ and the address and undefined-behaviour sanitizers, linked with
launch_plan.cpp (and what it needs), and run once per scenario; it prints one JSON line."""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "volume-renderer_amd" / "csrc"
CHECK = ROOT / "tests" / "mode_dispatch" / "dispatch_check.cpp"
UNITS = ["launch_plan.cpp", "tile_schedule.cpp", "launch_tuner.cpp"]
SANITIZE = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SIZES = [0, 1, 15, 16, 17]


@pytest.fixture(scope="module")
def dispatch_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mode_dispatch") / "dispatch_check"
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SANITIZE + ["-I", str(CSRC), str(CHECK)] + [str(CSRC / u) for u in UNITS] + ["-o", str(exe)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, "building dispatch_check failed:\n" + proc.stdout + proc.stderr

    def run(scenario):
        p = subprocess.run([str(exe), scenario], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (scenario, p.returncode, p.stdout, p.stderr)   # (any sanitizer report ends the program with an error)
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 1, p.stdout
        return json.loads(lines[0])

    return run


def test_the_header_names_no_hip_header(dispatch_check):
    """the fixture built it with plain g++, no HIP header on the include path; none is named either"""
    for f in ("mode_dispatch.h", "launch_plan.h", "vr_frame.h"):
        assert not [ln for ln in (CSRC / f).read_text().splitlines() if ln.startswith("#include") and "hip" in ln.lower()], f


def test_every_combination_reaches_its_own_instance(dispatch_check):
    r = dispatch_check("sweep")
    # layout x filter x flag x big x mode, as digits LAYOUT FILTER FLAG MODE BIG of the instance that ran
    want = [lay * 10000 + fil * 1000 + flag * 100 + mode * 10 + big
            for lay in (0, 1) for fil in (0, 1) for flag in (0, 1) for big in (0, 1) for mode in (0, 1, 2)]
    assert len(want) == 48 and len(set(want)) == 48
    assert r["calls"] == 48                   # one instance per combination, none twice
    assert r["asked"] == want
    assert r["got"] == want                   # each combination maps to itself (-1: the two levels disagreed)
    assert r["not_zero"] == 11021             # layout 2, filter -1, big_offsets 7, mode 5: "not 0" is 1, past the last mode is the last
    assert r["order"] == 201 and r["no_axis"] == 7


def test_tile_counts(dispatch_check):
    r = dispatch_check("tiles")
    ceil16 = {0: 0, 1: 1, 15: 1, 16: 1, 17: 2}
    assert r["tiles16"] == [ceil16[n] for n in SIZES]
    assert r["x"] == [ceil16[w] for w in SIZES for _ in SIZES]          # widths outer, rows inner
    assert r["y"] == [ceil16[rows] for _ in SIZES for rows in SIZES]    # rows = row_end - row_begin, wherever the range starts
    # 40 image rows in stripes of 8 over 2 ranks: rank 0 holds stripes 0, 2, 4 = 24 local rows, rank 1 stripes 1, 3 = 16; width 17
    assert r["striped"] == [2, 2, 2, 1]


def test_division_modes(dispatch_check):
    r = dispatch_check("divmodes")            # DIV_UNIT 0, DIV_CERT 1, DIV_EXACT 2, in that order
    assert r["texcoord"] == [1, 1, 2]         # certified unless exact
    assert r["window"] == [2, 1, 2]           # exact unless certified
