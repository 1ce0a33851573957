"""rayGeometryKey (volume-renderer_amd/csrc/launch_plan.cpp): the key under which the ray-ordered sample stream of a still view
(vr_stream.hip) stays valid.  tests/ray_geometry_key/key_check.cpp is compiled with g++ together with launch_plan.cpp,
tile_schedule.cpp and launch_tuner.cpp, with the address and undefined-behaviour sanitizers, like tests/test_launch_plan_cpu.py;
it changes one field of a launch at a time and says whether the key moved.  Everything that decides WHICH voxel a sample reads
must move it; window, alpha, transfer function, accumulation switch, target and packed copy must not -- they render from the
same stream."""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "volume-renderer_amd" / "csrc"
CHECK = ROOT / "tests" / "ray_geometry_key" / "key_check.cpp"
UNITS = ["launch_plan.cpp", "tile_schedule.cpp", "launch_tuner.cpp"]
SANITIZE = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

GEOMETRY = ([f"cam{i}" for i in range(21)] + ["img_w", "img_h", "row_begin", "row_end", "col_lim", "row_lim", "stripe_rows", "stripe_index",
            "stripe_count", "nx", "ny", "nz"] + [f"{f}{a}" for a in range(3) for f in ("half", "pmin", "pmax", "ext", "rext")] +
            ["step", "max_steps", "view_top", "view_bottom", "divmode_tc", "layout", "bytes_per_voxel", "generation", "generation_high_word"])
NOT_GEOMETRY = ["window", "alpha", "tf_len", "accum", "fb_compact", "fb_format", "pk12_base", "mip", "variant_bits"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ray_geometry_key") / "key_check"
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SANITIZE + ["-I", str(CSRC), str(CHECK)] + [str(CSRC / u) for u in UNITS] + ["-o", str(exe)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, "building key_check failed:\n" + proc.stdout + proc.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)   # (any sanitizer report ends the program with an error)
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_two_launches_of_one_geometry_have_one_key(report):
    assert report["same"] == 1
    # 21 camera floats, 9 image / row / stripe words, 3 dimensions, 15 box floats, step, cap, 2 view switches, 3 config words, 2 of the generation
    assert report["words"] == 21 + 9 + 3 + 15 + 1 + 1 + 2 + 3 + 2


def test_every_field_that_decides_a_samples_voxel_changes_the_key(report):
    assert sorted(report["changes"]) == sorted(GEOMETRY)
    assert [n for n in GEOMETRY if report["changes"][n] != 1] == []


def test_what_only_classifies_or_stores_keeps_the_key(report):
    assert sorted(report["keeps"]) == sorted(NOT_GEOMETRY)
    assert [n for n in NOT_GEOMETRY if report["keeps"][n] != 0] == []


def test_eligibility(report):
    # a fast-kernel frame with a tile table | the skipping switch on | TRILINEAR | no tile table
    assert report["eligible"] == [1, 0, 0, 0]
