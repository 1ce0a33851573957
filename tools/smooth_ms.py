"""Device time of vr_smooth_volume, one JSON line per case, each beside its one-read-one-write floor.

Cases: cfg3 (1024^3 u16 noise ball) at sigma 1 and 3; cfg4 (2048^3 u8) at sigma 1; cfg3 with the anisotropic (2, 2, 0).
Bricked layout.  kernel_ms = median (and min) of `--reps` calls after `--warmup` untimed ones (sustained clocks), each the
HIP-event time of the call's passes (vr_get_smoothing_ms: first launch to last, every slab; allocations and the range scan
excluded).  floor_ms = 2 x the volume's bytes / the vr_measure_stream_read rate of the same process: what one kernel that read
every voxel once and wrote it once would take.  x_floor = kernel_ms / floor_ms.  fp32_traffic_floor_ms is the same rate applied
to the bytes the passes move by design (voxels in, fp32 planes between the passes, voxels out; halo re-reads not counted).
The cfg3 cases also check 500 sampled voxels against the CPU definition, tests/smooth_ref/smooth_ref.c.

    python tools/smooth_ms.py [--reps 9] [--warmup 3] [--out profiles/smooth_ms.json] [--no-cfg4] [--only NAME]

--only NAME runs that one case without the reference check: the shape for a rocprofv3 pass.
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

_spec = importlib.util.spec_from_file_location("smooth_ref_binding", ROOT / "tests" / "smooth_ref" / "binding.py")
smooth_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(smooth_ref)

CELLS = {
    "cfg3": dict(dims=(1024, 1024, 1024), bytes=2, seed=0xC0FFEE),
    "cfg4": dict(dims=(2048, 2048, 2048), bytes=1, seed=0x9E3779B9),
}
CASES = [
    dict(name="cfg3_sigma1", cell="cfg3", sigma=(1.0, 1.0, 1.0)),
    dict(name="cfg3_sigma3", cell="cfg3", sigma=(3.0, 3.0, 3.0)),
    dict(name="cfg3_sigma_2_2_0", cell="cfg3", sigma=(2.0, 2.0, 0.0)),
    dict(name="cfg4_sigma1", cell="cfg4", sigma=(1.0, 1.0, 1.0)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
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
        lib = None if args.only else smooth_ref.build(tmp)
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
                floor_ms = 2.0 * vol_bytes / (gbps * 1e9) * 1e3
                for c in mine:
                    sig = c["sigma"]
                    passes = sum(1 for s in sig if s > 0)
                    for _ in range(args.warmup):
                        r.smoothVolume(sigma_voxels=sig)
                    ms = []
                    for _ in range(args.reps):
                        r.smoothVolume(sigma_voxels=sig)
                        ms.append(r.smoothingMs())
                    med = statistics.median(ms)
                    moved = 2 * vol_bytes + 2 * (passes - 1) * nx * ny * nz * 4
                    d = dict(case=c["name"], volume=f"{nx}x{ny}x{nz} u{8 * cfg['bytes']} noise ball", layout="bricked", sigma=list(sig),
                             radius=[int(np.ceil(3 * s)) for s in sig], passes=passes, reps=args.reps, kernel_ms=round(med, 4),
                             kernel_ms_min=round(min(ms), 4), stream_read_gbps=round(gbps, 1), floor_ms=round(floor_ms, 4),
                             x_floor=round(med / floor_ms, 2), fp32_traffic_floor_ms=round(moved / (gbps * 1e9) * 1e3, 4),
                             x_fp32_traffic_floor=round(med / (moved / (gbps * 1e9) * 1e3), 2))
                    if check:
                        rng = np.random.default_rng(7)
                        ijk = np.stack([rng.integers(0, n, 500) for n in (nx, ny, nz)], axis=1).astype(np.int32)
                        ijk[0] = (0, 0, 0); ijk[1] = (nx - 1, ny - 1, nz - 1)
                        want = smooth_ref.smooth_points(lib, vol, tuple(vra.smooth_weights(s) if s > 0 else None for s in sig), ijk)
                        got = r.readVolume()[ijk[:, 2], ijk[:, 1], ijk[:, 0]]
                        d["sampled_voxels_bit_exact"] = bool(np.array_equal(got, want))
                    s = json.dumps(d)
                    print(s, flush=True)
                    lines.append(s)
                del vol
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
