"""The measured work model's state machine (volume-renderer_amd/csrc/launch_tuner.cpp: vr::LaunchTuner, vr::launchTuneKey) on
the CPU: tests/launch_tuner/tuner_check.cpp is compiled with g++ -- together with launch_tuner.cpp and tile_schedule.cpp, with
the address and undefined-behaviour sanitizers -- and run once per scenario with synthetic millisecond values; it prints one
JSON line.  The rules asserted here are the ones tests/test_work_model_gpu.py can only see statistically: passing through,
the 2 % tie rule, bursts, a lost measurement, stale generations, the one re-validation, eviction, the blob's checks, the
key's buckets."""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "volume-renderer_amd" / "csrc"
CHECK = ROOT / "tests" / "launch_tuner" / "tuner_check.cpp"
SANITIZE = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def tuner_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("launch_tuner") / "tuner_check"
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SANITIZE + ["-I", str(CSRC), str(CHECK), str(CSRC / "launch_tuner.cpp"),
                                                                          str(CSRC / "tile_schedule.cpp"), "-o", str(exe)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, "building tuner_check failed:\n" + proc.stdout + proc.stderr

    def run(scenario):
        p = subprocess.run([str(exe), scenario], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (scenario, p.returncode, p.stdout, p.stderr)   # (any sanitizer report ends the program with an error)
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 1, p.stdout
        return json.loads(lines[0])

    return run


def test_launch_tuner_compiles_without_hip():
    """plain g++, no HIP header on the include path"""
    proc = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", str(CSRC / "launch_tuner.cpp")], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    for f in ("launch_tuner.h", "launch_tuner.cpp"):
        assert not [ln for ln in (CSRC / f).read_text().splitlines() if ln.startswith("#include") and "hip" in ln.lower()], f


def test_a_key_passing_through_gets_no_decision(tuner_check):
    r = tuner_check("pass")
    assert r["alternating_decided"] == [0] * 12 and r["alternating_entries"] == 0          # A B A B ...: never an entry
    assert r["run_decided"] == [0, 0, 0, 0, 0, 1] and r["run_measure"] == [0, 0, 0, 0, 0, 1]   # A A B A A | A
    assert r["run_entries"] == 1 and r["run_entry_is_A"]
    assert r["third_decided"] and r["third_measure"] and r["third_trial"] and r["third_key"] == 100


def test_settling_and_the_tie_rule(tuner_check):
    r = tuner_check("settle")
    assert r["rival_0985"] == 4                       # 1.5 % faster than the heuristic's candidate: not enough
    assert r["rival_097"] == 0                        # 3 % faster: wins
    assert r["rivals_09_08"] == 1 and r["rivals_08_09"] == 0   # between rivals the lower time
    assert r["heuristic_fastest"] == 4
    assert r["minimum_counts"] == 0                   # minima 1.0 (heuristic), 0.9, 0.95
    assert r["measurements_per_candidate"] == [2, 2, 2]
    assert r["after_decided"] and r["after_cand"] == 0 and not r["after_measure"] and not r["after_trial"]


def test_a_burst_launches_two_measurements_per_candidate(tuner_check):
    r = tuner_check("burst")
    assert r["measure"] == [1] * 6 + [0] * 5          # ncand x 2 picks measure, then none
    assert sorted(r["cand"][:6]) == [0, 0, 1, 1, 4, 4]
    assert r["cand"][6:] == [4] * 5                   # before any result: the heuristic's candidate
    assert r["trial"] == [1] * 11
    assert r["issued"] == [2, 2, 2] and r["tries"] == [0, 0, 0]
    assert r["full_measure"] == [0] * 8 and r["full_cand"] == [4] * 8 and r["full_issued"] == [0, 0, 0]   # every event pair taken


def test_a_lost_measurement_is_launched_again(tuner_check):
    r = tuner_check("lost")
    assert r["launched"] == 6 and not r["waiting_measure"]
    assert not r["rearm_measure"] and r["rearm_cand"] == 4 and r["issued_after_rearm"] == [0, 0, 0]   # one call re-arms
    assert r["again_measure"]                         # the next measures again
    assert r["measured_after"] == 6 and r["settled"] == 0


def test_stale_results_change_nothing(tuner_check):
    r = tuner_check("stale")
    assert r["revalidating"] and r["generation_changed"]
    assert r["counts_after_stale_results"] == 0 and r["settled_after_stale_results"] == -1
    assert r["evicted"] and r["recreated"] and r["recreated_generation_differs"]
    assert r["recreated_counts_after_stale_results"] == 0 and r["recreated_settled"] == -1


def test_the_one_revalidation(tuner_check):
    r = tuner_check("reval")
    assert r["settled_first"] == 0
    assert r["fired_at"] == 96                        # kTuneRevalidateFrames decided calls after settling
    assert r["firing_decided"] and r["firing_cand"] == 0 and not r["firing_measure"]   # it still runs the old settled candidate, reported as a trial
    assert r["next_measure"] and r["next_trial"]
    assert r["remeasured"] == 6 and r["settled_second"] == 1
    assert r["trials_afterwards"] == 0 and r["other_picks_afterwards"] == 0            # never a second time
    assert r["imported"] == 1 and r["imported_trials"] == 0 and r["imported_other_picks"] == 0   # never for an imported entry


def test_eviction_of_the_least_recently_used_eighth(tuner_check):
    r = tuner_check("evict")
    assert r["entries_before"] == 512 and r["new_decided"]
    assert r["entries_after"] == 512 - 64 + 1
    assert r["missing"] == list(range(32, 96))        # keys 0 .. 31 were used again: the next 64 oldest go
    assert r["survivors_changed"] == 0


def test_the_choices_blob(tuner_check):
    r = tuner_check("blob")
    assert r["sizeof_header"] == 88 and r["sizeof_record"] == 56
    assert r["need"] == 88 + 5 * 56                   # settled entries only
    assert r["need_small_buffer"] == r["need"] and r["small_buffer_untouched"]
    assert r["magic"] and r["ascending"] == [1, 1, 1, 1]
    assert r["accepted"] == 5 and r["entries"] == 5 and r["round_trip_identical"] and r["imported_state"]
    assert r["accepted_again"] == 5 and r["entries_again"] == 5
    assert r["other_build"] == 0 and r["other_device"] == 0 and r["entries_after_foreign"] == 0
    assert r["bad_magic"] == -1 and r["bad_magic_other_build"] == -1 and r["bad_version"] == -1      # -1: std::invalid_argument
    assert r["short_87"] == -1 and r["cut_in_records"] == -1 and r["cut_in_records_other_build"] == -1
    assert r["entries_after_refused"] == 0
    assert r["mixed_accepted"] == 2 and r["mixed_present"] == [0, 1, 0, 0, 1, 0, 0]   # ncand 1, 9, 0 and a settled value that is no candidate are skipped
    assert r["mixed_settled_2"] == 0 and r["mixed_settled_5"] == 48
    assert r["many_accepted"] == 512 and r["many_entries"] == 512


def test_the_keys_buckets(tuner_check):
    r = tuner_check("keys")
    assert r["deterministic"]
    assert r["alpha_002_002239_same"] and r["width_4095_3856_same"]      # the slider drag of test_work_model_gpu.py: one entry
    assert r["alpha_05_1_same"] and r["alpha_002_006_same"] and r["alpha_002_01_differ"] and r["alpha_05_differs_from_002"]
    assert r["width_4095_2047_differ"]
    assert r["nx_differs"] and r["filter_differs"] and r["layout_differs"] and r["prior_differs"]
    assert r["rows_differ"] and r["active_tiles_bucket_same"] and r["active_tiles_differ"]
