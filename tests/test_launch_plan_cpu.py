"""The rules that decide what a launch runs (volume-renderer_amd/csrc/launch_plan.cpp) and when the tile tables are built again
(tile_schedule.cpp: tileTablesStale, skipOrderSignature) on the CPU: tests/launch_plan/plan_check.cpp is compiled with g++ --
together with launch_plan.cpp, tile_schedule.cpp and launch_tuner.cpp, with the address and undefined-behaviour sanitizers --
and run once per scenario; it prints one JSON line.  Every expected value below is worked by hand from the rule written beside
it, on both sides of each threshold; tests/test_launch_plan_gpu.py and tests/test_work_model_gpu.py see the same rules only
through what a frame reports.

Candidate bits: 1 relay kernel, 2 pipelined loop, 4 four-sample batches (NEAREST); staged shape << 3 (TRILINEAR)."""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "volume-renderer_amd" / "csrc"
CHECK = ROOT / "tests" / "launch_plan" / "plan_check.cpp"
UNITS = ["launch_plan.cpp", "tile_schedule.cpp", "launch_tuner.cpp"]
SANITIZE = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("launch_plan") / "plan_check"
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SANITIZE + ["-I", str(CSRC), str(CHECK)] + [str(CSRC / u) for u in UNITS] + ["-o", str(exe)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, "building plan_check failed:\n" + proc.stdout + proc.stderr

    def run(scenario):
        p = subprocess.run([str(exe), scenario], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (scenario, p.returncode, p.stdout, p.stderr)   # (any sanitizer report ends the program with an error)
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 1, p.stdout
        return json.loads(lines[0])

    return run


def test_the_rules_compile_without_hip():
    """plain g++, no HIP header on the include path, none named"""
    for unit in ("launch_plan.cpp", "tile_schedule.cpp"):
        proc = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", str(CSRC / unit)], capture_output=True, text=True)
        assert proc.returncode == 0, proc.stdout + proc.stderr
    for f in ("launch_plan.h", "launch_plan.cpp", "tile_schedule.h", "tile_schedule.cpp", "launch_tuner.h", "vr_frame.h"):
        assert not [ln for ln in (CSRC / f).read_text().splitlines() if ln.startswith("#include") and "hip" in ln.lower()], f


def test_first_guess_nearest(plan_check):
    r = plan_check("nearest")
    # relay kernel: active tiles < (aligned ? 256 : 1024) * clamp(longest / 1000, 0.15, 1); aligned: alignment >= 0.92.
    # Rows: aligned 1045 samples (scale 1: 255 | 256), oblique 1045 (1023 | 1024), aligned 262 (256 * 0.262 = 67.07: 67 | 68),
    # aligned 50 (the scale clamps at 0.15: 38.4: 38 | 39).  alpha < 0.5: pipelined loop (2); alpha >= 0.5: short batches (4)
    assert r["alpha_002"] == [3, 2] * 4
    assert r["alpha_05"] == [5, 4] * 4
    assert r["variant2"] == [0, 0]            # never the relay; no pipelined loop or short batches outside variant 0
    assert r["variant3"] == [1, 1]            # always the relay
    assert r["variant5"] == [2, 2, 2]         # pipelined, no relay, whatever alpha and the tile count
    assert r["variant1"] == [1, 0]            # the relay bit follows the tiles; neither the pipelined loop nor short batches


def test_first_guess_trilinear(plan_check):
    r = plan_check("trilinear")
    # largest dimension <= 640 and a small table: shape 6; else 8-bit volumes: whole layers (1) at any pose
    assert r["small"] == [6, 1, 1, 1]         # 640 + table | 641, u8 oblique | 640 without the table | 641, u8 aligned
    # u16: whole layers while the alignment is >= 0.985: dir (0.17, 0, 1) -> 0.98586, (0.18, 0, 1) -> 0.98418, whose ratios 0.18, 0 give 3
    assert r["u16_whole_layers"] == [1, 3]
    # below: 4 when mid / max > 0.7 and min / max > 0.55, else 3: (0.6, 0.8, 1) | (0.5, 0.8, 1) | (0.6, 0.69, 1)
    assert r["u16_ratios"] == [4, 3, 3]
    # tall tiles need 32 consecutive local rows to be 32 image rows: stripes of 16 rows x 2 ranks take 3, of 32 rows 4 again
    assert r["u16_stripes"] == [3, 4]
    assert r["variants"] == [3, 0, 6]         # a non-zero kernel variant: the shape set before stays
    # half layers without both per-axis copies, variant 0: the batched kernel where it can run (0), else whole layers (1)
    assert r["fallback"] == [0, 0, 1, 1, 3, 4, 3, 1, 6]


def test_candidates(plan_check):
    r = plan_check("candidates")
    # NEAREST: prior (without the relay bit when it cannot run), 4 or 2 by alpha >= 0.5, 0, 1 when the relay can run
    assert r["nearest_prior3"] == [3, 2, 0, 1]
    assert r["nearest_prior5_alpha1"] == [5, 4, 0, 1]
    assert r["big_offsets_prior3"] == [2, 0] and r["skipping_prior3"] == [2, 0]
    assert r["grid_without_skipping_prior3"] == [3, 2, 0, 1]
    assert r["generic_only"] == []            # fewer than two candidates: nothing to tune (the rules never produce exactly one)
    # TRILINEAR: nothing without the apron copy; else prior, 1 << 3, 5 << 3, then each optional entry under its condition
    assert r["tri_no_apron"] == []
    assert r["tri_base"] == [8, 40, 0]        # grey mode: the batched kernel can run
    assert r["tri_tf"] == [8, 40]             # a transfer function: it cannot
    assert r["tri_small"] == [8, 40, 48]      # 6 << 3 needs the small table
    assert r["tri_copies"] == [8, 40, 24]     # 3 << 3 needs both per-axis copies ...
    assert r["tri_copies_tall"] == [8, 40, 24, 32]   # ... 4 << 3 the tall table too
    assert r["tri_one_copy_tall"] == [8, 40]
    assert r["tri_u8_oblique_tall"] == [8, 40, 32]   # u8, alignment < 0.92, tall table: whole layers on tall tiles
    assert r["tri_u8_aligned_tall"] == [8, 40] and r["tri_u8_oblique_no_tall"] == [8, 40]
    assert r["tri_everything_prior16"] == [16, 8, 40, 48, 0, 24, 32]   # the longest list: 7 <= kTuneCand, the guard behind the array untouched
    assert r["tri_prior_first"] == [32, 8, 40, 48, 0, 24]              # the prior first, no duplicate of it


def test_choice_bits_and_apply_are_inverse(plan_check):
    r = plan_check("bits")
    assert r["not_inverse"] == []             # NEAREST 0 .. 7, TRILINEAR shapes 0 .. 6
    assert r["trilinear_then_nearest"] == [32, 3]   # the same L: tri_slab << 3 under TRILINEAR, the three NEAREST bits otherwise


def test_zero_alpha_threshold(plan_check):
    r = plan_check("alpha")                   # [ok, thresh] per value (NEAREST), then for the table's whole run (TRILINEAR)
    assert r["alpha_zero"] == [1, 65535, 1, 65535]
    assert r["grey_ramp"] == [1, 37, 1, 37]   # min_val
    assert r["ten_transparent"] == [1, 9, 1, 9]     # window 0 .. 255: value e reads entry e
    assert r["entry0_visible"] == [0, 0, 0, 0]
    # window 0 .. 2: values 0, 1, 2 read entries 0, 128, 255, all transparent: 2; the leading run ends at entry 64: only value 0
    assert r["window_0_2"] == [1, 2, 1, 0]


def test_skip_grid_limits(plan_check):
    r = plan_check("grid")                    # [ok, cells x, y, z, total]; cells = ceil(n / 8)
    assert r["small"] == [1, 13, 8, 2, 208]
    assert r["x_last"] == [1, 2 ** 24 - 1, 1, 1, 2 ** 24 - 1] and r["x_first"] == [0, 2 ** 24, 1, 1, 2 ** 24]        # cells x < 2^24
    assert r["yz_last"] == [1, 1, 4096, 4095, 4096 * 4095] and r["yz_first"] == [0, 1, 4096, 4096, 2 ** 24]           # cells y * z < 2^24
    assert r["total_last"] == [1, 129, 4096, 4064, 2147352576] and r["total_first"] == [0, 129, 4096, 4065, 2147880960]   # 2 bytes a cell < 2^32
    # NEAREST: 4 * (largest voxel advance per step) + 0.6 <= 8: 1.84375 -> 7.975, 1.859375 -> 8.0375; the last two: the same
    # frame whose 128-voxel axis lies along an extent of 2 (0.93 a step) or, in the rotated views, of 1
    assert r["batch_reach"] == [1, 0, 1, 0]


def test_rebuild_rule(plan_check):
    r = plan_check("rebuild")                 # 1 = build the tables again
    assert r["camera"] == [0, 0, 1, 1, 1, 1]  # unmoved | one entry by 0.05 | by 0.0500001 | by -0.0500001 | a NaN first | a NaN last
    assert r["key_and_table"] == [1, 1]
    assert r["tall"] == [1, 0, 0, 1] and r["small"] == [1, 0, 1]   # a missing table rebuilds only when it is needed
    # 1 + thresh * 32 / (exact_max + 1): 32nds of the data's range, never 0
    assert r["signature"] == [1, 1, 2, 32, 1, 32, 97]
    assert r["signature_changes"] == [0, 1, 1, 1, 1, 1]   # same | next 32nd | skipping off | skipping on | dropped (-1) | dropped, now geometric
