"""bench.py's plain command line measures the headline and nothing else (what takes runs of its own waits for --full), and
--dump-outputs DIR writes the frame of the last timed step so that two builds can be compared output for output."""
import importlib
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def _bench():
    if str(ROOT) not in sys.path:
        sys.path.insert(0, str(ROOT))
    return importlib.import_module("bench")


def test_plain_command_line_is_lean_and_extras_implies_full(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse_args()
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--extras"])
    assert bench.parse_args().full is True
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse_args()
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_writes_the_whole_frame_when_it_fits(tmp_path):
    bench = _bench()
    frame = np.random.default_rng(1).random((24, 40, 4), dtype=np.float32)
    bench.dump_outputs(tmp_path / "d", frame)
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == ["frame.npy"]
    got = np.load(tmp_path / "d" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, frame)


def test_dump_outputs_samples_the_same_rows_of_a_large_frame(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 << 10)
    frame = np.random.default_rng(2).random((512, 64, 4), dtype=np.float32)      # 512 KiB: eight times the limit
    bench.dump_outputs(tmp_path / "a", frame)
    bench.dump_outputs(tmp_path / "b", frame.copy())
    rows = np.load(tmp_path / "a" / "frame_rows.npy")
    index = np.load(tmp_path / "a" / "frame_row_index.npy")
    assert not (tmp_path / "a" / "frame.npy").exists()
    assert rows.dtype == np.float32 and index.dtype == np.float64
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 << 10 and len(index) > 0
    assert np.array_equal(rows, frame[index.astype(np.int64)]) and np.all(np.diff(index) > 0)
    assert np.array_equal(index, np.load(tmp_path / "b" / "frame_row_index.npy"))          # seeded: the same sample every run


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_frame(oracle, tmp_path):
    """config 0 of BASELINE.json (64^3 uint8 sphere, 256x256) through the plain command line: the line holds the headline
    fields and none of --full's, and DIR/frame.npy is the frame the oracle renders"""
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--clock-ramp-frames", "0",
           "--synth", "sphere", "--volume", "64", "--bytes", "1", "--width", "256", "--height", "256", "--alpha", "1.0",
           "--dump-outputs", str(tmp_path / "out")]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ))
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert proc.returncode == 0 and len(lines) == 1, (proc.returncode, proc.stdout[-1500:], proc.stderr[-2500:])
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["unit"] == "Msamples/s" and rec["dtype"] == "f32"
    assert "cpu_baseline" not in rec and "extras" not in rec and "measured_stream_read" not in rec["roofline"]
    got = np.load(tmp_path / "out" / "frame.npy")
    want, _ = oracle.render(oracle.gen_sphere_u8(64, 28), oracle.OracleParams(256, 256))
    assert got.dtype == np.float32 and got.shape == want.shape
    assert float(np.max(np.abs(got - want))) <= 1e-4
