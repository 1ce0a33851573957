"""Device time of vr_label_components and of the filtered extraction, one JSON line per case, beside the streaming floor.

Cases: cfg3 (1024^3 u16 noise ball) and cfg4 (2048^3 u8; 2^33 voxels: the 64-bit parents), both after smoothVolume(sigma = 2), at
the iso values of profiles/mesh_ms.json.  Bricked layout, VR_QUIRK_U16_OFFSET off (iso in stored units).
label_ms = median (and min) of `--reps` calls after `--warmup` untimed ones, each the HIP-event time of the call's kernels
(vr_get_components_ms: tile pass, seam pass, flatten, scan, labels, records; allocations and read-backs excluded).
floor_ms = (the volume's bytes + 4 bytes a voxel of labels) / the vr_measure_stream_read rate of the same process: one read of
every voxel, one write of every label.  x_floor = label_ms / floor_ms.
extract_ms: vr_extract_isosurface; extract_all_selected_ms: vr_extract_components with every component selected (the same
mesh: what the filtered predicate costs); extract_largest_ms: keeping the largest component only.  All vr_get_mesh_ms.
At full size the labels are not compared voxel by voxel: the records' voxel counts must sum to the host's count of voxels >= iso,
and the first voxels must ascend.  cpu_ref_256_ms is the CPU restatement (tests/components_ref/components_ref.c, one thread) on
the central 256^3 voxels, for scale; the device labelling of that crop (a second handle) is compared with it bit for bit.

    python tools/components_ms.py [--reps 5] [--warmup 2] [--out profiles/components_ms.json] [--no-cfg4] [--only NAME]
"""
from __future__ import annotations

import argparse
import importlib
import importlib.util
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

_spec = importlib.util.spec_from_file_location("components_ref_binding", ROOT / "tests" / "components_ref" / "binding.py")
comp_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(comp_ref)

CASES = [
    dict(name="cfg3_sigma2", dims=(1024, 1024, 1024), bytes=2, seed=0xC0FFEE, iso=2057),
    dict(name="cfg4_sigma2", dims=(2048, 2048, 2048), bytes=1, seed=0x9E3779B9, iso=128),
]
SIGMA = (2.0, 2.0, 2.0)
CROP = 256


def timed(reps, warmup, call, read_ms):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(reps):
        out = call()
        ms.append(read_ms())
    return out, round(statistics.median(ms), 4), round(min(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cfg4", action="store_true")
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    vra = importlib.import_module("volume-renderer_amd")
    R = vra.renderer
    todo = [c for c in CASES if not (args.no_cfg4 and c["name"].startswith("cfg4"))]
    if args.only:
        todo = [c for c in todo if c["name"] == args.only]
        if not todo:
            raise SystemExit(f"--only: no case {args.only}; known: {[c['name'] for c in CASES]}")
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        lib = comp_ref.build(tmp)
        for c in todo:
            nx, ny, nz = c["dims"]
            iso = c["iso"]
            with vra.RendererCore(0) as r:
                r.setup((64, 48))
                assert r.loadShader("VolumeRenderer.cs")
                r.setLayout(R.LAYOUT_BRICKED)
                r.setQuirks(0)
                r.generateSynthetic(R.SYNTH_NOISE_BALL, c["dims"], c["bytes"], c["seed"])
                r.smoothVolume(sigma_voxels=SIGMA)
                gbps = r.measureStreamRead(5)
                n, label_ms, label_min = timed(args.reps, args.warmup, lambda: r.labelComponents(iso), r.componentsMs)
                info = r.componentsInfo()
                rec = r.readComponents()
                vol_bytes = nx * ny * nz * c["bytes"]
                floor_ms = (vol_bytes + 4 * nx * ny * nz) / (gbps * 1e9) * 1e3
                d = dict(case=c["name"], volume=f"{nx}x{ny}x{nz} u{8 * c['bytes']} noise ball", layout="bricked", sigma=list(SIGMA), iso=iso,
                         parent_bits=32 if nx * ny * nz < 2 ** 32 - 1 else 64, components=n, inside_voxels=info["inside"],
                         largest_voxels=int(rec["voxels"].max(initial=0)), one_voxel_components=int((rec["voxels"] == 1).sum()),
                         reps=args.reps, label_ms=label_ms, label_ms_min=label_min, stream_read_gbps=round(gbps, 1),
                         floor_ms=round(floor_ms, 4), x_floor=round(label_ms / floor_ms, 2))
                full, d["extract_ms"], _ = timed(args.reps, args.warmup, lambda: r.extractIsosurface(iso), r.meshMs)
                same, d["extract_all_selected_ms"], _ = timed(args.reps, args.warmup, r.extractComponents, r.meshMs)
                d["vertices"], d["triangles"] = full
                d["all_selected_same_counts"] = bool(same == full)
                d["selected_largest"] = r.selectComponents(0, 1)
                kept, d["extract_largest_ms"], _ = timed(args.reps, args.warmup, r.extractComponents, r.meshMs)
                d["largest_vertices"], d["largest_triangles"] = kept
                r.freeMesh()
                vol = r.readVolume()
                d["host_inside_voxels"] = int(np.count_nonzero(vol >= iso))
                d["voxel_counts_sum_to_host_count"] = bool(int(rec["voxels"].sum()) == d["host_inside_voxels"] == info["inside"])
                d["first_voxels_ascend"] = bool(np.all(np.diff(rec["first_voxel"].astype(np.int64)) > 0))
                o = [(m - CROP) // 2 for m in (nx, ny, nz)]
                crop = np.ascontiguousarray(vol[o[2]:o[2] + CROP, o[1]:o[1] + CROP, o[0]:o[0] + CROP])
                del vol
            t0 = time.perf_counter()
            want_labels, want_rec = comp_ref.label(lib, crop, float(iso))
            d["cpu_ref_256_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            d["cpu_ref_256_components"] = int(want_rec["voxels"].size)
            with vra.RendererCore(0) as q:
                q.setup((64, 48))
                assert q.loadShader("VolumeRenderer.cs")
                q.setLayout(R.LAYOUT_BRICKED)
                q.setQuirks(0)
                q.setVolume(crop, (1.0, 1.0, 1.0))
                q.labelComponents(iso)
                d["gpu_256_label_ms"] = round(q.componentsMs(), 4)
                got = q.readComponents()
                d["crop_labels_bit_exact"] = bool(np.array_equal(q.readLabels(), want_labels) and
                                                  all(np.array_equal(got[k], want_rec[k]) for k in ("voxels", "first_voxel", "bbox")))
            s = json.dumps(d)
            print(s, flush=True)
            lines.append(s)
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
