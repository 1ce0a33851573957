"""Device time of vr_simplify_mesh, one JSON line per (case, cell), each beside its streaming floor.

Cases: the meshes of profiles/mesh_ms.json -- cfg3 (1024^3 u16 noise ball) and cfg4 (2048^3 u8), both after smoothVolume(sigma = 2),
at that file's iso values, spacing 1 -- simplified on cells of 2 and of 4 voxel spacings.  Bricked layout, VR_QUIRK_U16_OFFSET off.
Every timed call simplifies a fresh extraction (untimed).  kernel_ms = median (and min) of `--reps` calls after `--warmup` untimed
ones, each the HIP-event time of the call's kernels and device sorts (vr_get_simplify_ms; allocations and read-backs excluded).
floor_ms = (the input mesh's bytes read once + the output mesh's bytes written once) / the vr_measure_stream_read rate of the same
process.  x_floor = kernel_ms / floor_ms.  --check also compares cfg3's results with the CPU restatement
(tests/simplify_ref/simplify_ref.c) bit for bit.

    python tools/simplify_ms.py [--reps 5] [--warmup 2] [--out profiles/simplify_ms.json] [--no-cfg4] [--only NAME] [--cells 2 4] [--check]

--only NAME --cells C --reps 1 --warmup 0 is the shape for a rocprofv3 --kernel-trace --stats pass (a run of its own).
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

_spec = importlib.util.spec_from_file_location("simplify_ref_binding", ROOT / "tests" / "simplify_ref" / "binding.py")
simp_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(simp_ref)

CASES = [
    dict(name="cfg3_sigma2", dims=(1024, 1024, 1024), bytes=2, seed=0xC0FFEE, iso=2057),
    dict(name="cfg4_sigma2", dims=(2048, 2048, 2048), bytes=1, seed=0x9E3779B9, iso=128),
]
SIGMA = (2.0, 2.0, 2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cfg4", action="store_true")
    ap.add_argument("--only", default=None)
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0])
    ap.add_argument("--check", action="store_true")
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
        lib = simp_ref.build(tmp) if args.check else None
        for c in todo:
            nx, ny, nz = c["dims"]
            with vra.RendererCore(0) as r:
                r.setup((64, 48))
                assert r.loadShader("VolumeRenderer.cs")
                r.setLayout(R.LAYOUT_BRICKED)
                r.setQuirks(0)
                r.generateSynthetic(R.SYNTH_NOISE_BALL, c["dims"], c["bytes"], c["seed"])
                r.smoothVolume(sigma_voxels=SIGMA)
                gbps = r.measureStreamRead(5)
                nv, nt = r.extractIsosurface(c["iso"])
                extract_ms = r.meshMs()
                source = r.readMesh() if lib is not None and c["name"].startswith("cfg3") else None
                for cell in args.cells:
                    ms, counts = [], None
                    for i in range(args.warmup + args.reps):
                        assert r.extractIsosurface(c["iso"]) == (nv, nt)
                        out = r.simplifyMesh(cell)
                        assert counts in (None, out)
                        counts = out
                        if i >= args.warmup:
                            ms.append(r.simplifyMs())
                    med = statistics.median(ms)
                    in_bytes, out_bytes = 24 * nv + 12 * nt, 24 * counts[0] + 12 * counts[1]
                    floor_ms = (in_bytes + out_bytes) / (gbps * 1e9) * 1e3
                    d = dict(case=c["name"], volume=f"{nx}x{ny}x{nz} u{8 * c['bytes']} noise ball", sigma=list(SIGMA), iso=c["iso"], cell=cell,
                             vertices_in=nv, triangles_in=nt, vertices_out=counts[0], triangles_out=counts[1],
                             triangles_ratio=round(counts[1] / nt, 4), mesh_bytes_in=in_bytes, mesh_bytes_out=out_bytes, reps=args.reps,
                             kernel_ms=round(med, 4), kernel_ms_min=round(min(ms), 4), extract_ms=round(extract_ms, 4),
                             stream_read_gbps=round(gbps, 1), floor_ms=round(floor_ms, 4), x_floor=round(med / floor_ms, 2))
                    if source is not None:
                        want, _ = simp_ref.simplify(lib, source, cell)
                        got = r.readMesh()
                        d["bit_exact_with_cpu_restatement"] = bool(all(g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))
                                                                       for g, w in zip(got, want)))
                    s = json.dumps(d)
                    print(s, flush=True)
                    lines.append(s)
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
