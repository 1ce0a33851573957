"""Device time of vr_rank_filter_volume, one JSON line per case, each beside its floor and beside a Gaussian pass of its radius.

Cases: cfg3 (1024^3 u16 noise ball) and cfg4 (2048^3 u8), each with ERODE at r = 1 and r = 4, OPEN at r = 2 and the 3x3x3
MEDIAN.  Bricked layout.  kernel_ms = median (and min) of `--reps` calls after `--warmup` untimed ones (sustained clocks), each
the HIP-event time of the call's passes (vr_get_rank_filter_ms: first launch to last; allocations and the range scan excluded).
floor_ms = passes x (one read + one write of the volume) / the vr_measure_stream_read rate of the same process; x_floor =
kernel_ms / floor_ms.  The yardstick is relative: a minimum pass does less arithmetic and moves a fraction of the bytes of a
Gaussian pass of equal radius, so gaussian_pass_ms is vr_smooth_volume's time per pass at a sigma with that radius (r - 0.5) / 3,
on the same volume in the same process, and rank_pass_ms / gaussian_pass_ms should stay below 1.
The cfg3 single operations also check 500 sampled voxels against the CPU definition, tests/rank_ref/rank_ref.c.

    python tools/rank_ms.py [--reps 7] [--warmup 2] [--out profiles/rank_ms.json] [--no-cfg4] [--only NAME]

--only NAME runs that one case without the reference check and the Gaussian: the shape for a rocprofv3 pass.
"""
from __future__ import annotations

import argparse
import importlib
import importlib.util
import json
import statistics
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

_spec = importlib.util.spec_from_file_location("rank_ref_binding", ROOT / "tests" / "rank_ref" / "binding.py")
rank_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rank_ref)

CELLS = {
    "cfg3": dict(dims=(1024, 1024, 1024), bytes=2, seed=0xC0FFEE),
    "cfg4": dict(dims=(2048, 2048, 2048), bytes=1, seed=0x9E3779B9),
}
OPS = [("erode_r1", rank_ref.ERODE, 1), ("erode_r4", rank_ref.ERODE, 4), ("open_r2", rank_ref.OPEN, 2), ("median_3x3x3", rank_ref.MEDIAN, 1)]
CASES = [dict(name=f"{cell}_{name}", cell=cell, op=op, r=r) for cell in CELLS for name, op, r in OPS]


def timed(call, read_ms, warmup, reps):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(reps):
        call()
        ms.append(read_ms())
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cfg4", action="store_true")
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    vra = importlib.import_module("volume-renderer_amd")
    R = vra.renderer
    todo = [c for c in CASES if not (args.no_cfg4 and c["cell"] == "cfg4")]
    if args.only:
        todo = [c for c in todo if c["name"] == args.only]
        if not todo:
            raise SystemExit(f"--only: no case {args.only}; known: {[c['name'] for c in CASES]}")
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        lib = None if args.only else rank_ref.build(tmp)
        for cell, cfg in CELLS.items():
            mine = [c for c in todo if c["cell"] == cell]
            if not mine:
                continue
            nx, ny, nz = cfg["dims"]
            with vra.RendererCore(0) as r:
                r.setup((64, 48))
                assert r.loadShader("VolumeRenderer.cs")
                r.setLayout(R.LAYOUT_BRICKED)
                r.generateSynthetic(R.SYNTH_NOISE_BALL, cfg["dims"], cfg["bytes"], cfg["seed"])
                check = lib is not None and cell == "cfg3"
                vol = r.readVolume() if check else None
                gbps = r.measureStreamRead(5)
                vol_bytes = nx * ny * nz * cfg["bytes"]
                gaussian = {}                                 # radius -> ms per pass
                for c in mine:
                    op, rad = c["op"], c["r"]
                    passes = 1 if op == rank_ref.MEDIAN else (6 if op in (rank_ref.OPEN, rank_ref.CLOSE) else 3)
                    med, low = timed(lambda: r.rankFilterVolume(op, rad), r.rankFilterMs, args.warmup, args.reps)
                    floor_ms = passes * 2.0 * vol_bytes / (gbps * 1e9) * 1e3
                    d = dict(case=c["name"], volume=f"{nx}x{ny}x{nz} u{8 * cfg['bytes']} noise ball", layout="bricked", op=rank_ref_name(op),
                             radius=[rad] * 3, passes=passes, reps=args.reps, kernel_ms=round(med, 4), kernel_ms_min=round(low, 4),
                             stream_read_gbps=round(gbps, 1), floor_ms=round(floor_ms, 4), x_floor=round(med / floor_ms, 2))
                    if check and op != rank_ref.OPEN:
                        rng = np.random.default_rng(7)
                        ijk = np.stack([rng.integers(0, n, 500) for n in (nx, ny, nz)], axis=1).astype(np.int32)
                        ijk[0] = (0, 0, 0); ijk[1] = (nx - 1, ny - 1, nz - 1)
                        want = rank_ref.rank_points(lib, vol, op, rad, ijk)
                        got = r.readVolume()[ijk[:, 2], ijk[:, 1], ijk[:, 0]]
                        d["sampled_voxels_bit_exact"] = bool(np.array_equal(got, want))
                    r.rankFilterVolume(R.VR_RANK_OFF, 0)
                    if op != rank_ref.MEDIAN and not args.only:
                        if rad not in gaussian:
                            sigma = (rad - 0.5) / 3.0             # ceil(3 sigma) = rad
                            g_med, _ = timed(lambda: r.smoothVolume(sigma_voxels=sigma), r.smoothingMs, args.warmup, args.reps)
                            r.smoothVolume(sigma_voxels=0.0)
                            gaussian[rad] = g_med / 3.0
                        d["rank_pass_ms"] = round(med / passes, 4)
                        d["gaussian_pass_ms"] = round(gaussian[rad], 4)
                        d["rank_over_gaussian"] = round(med / passes / gaussian[rad], 3)
                    s = json.dumps(d)
                    print(s, flush=True)
                    lines.append(s)
                del vol
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines) + "\n")


def rank_ref_name(op):
    return {rank_ref.ERODE: "erode", rank_ref.DILATE: "dilate", rank_ref.OPEN: "open", rank_ref.CLOSE: "close", rank_ref.MEDIAN: "median"}[op]


if __name__ == "__main__":
    main()
