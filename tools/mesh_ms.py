"""Device time of vr_extract_isosurface, one JSON line per case, each beside its streaming floor.

Cases: cfg3 (1024^3 u16 noise ball) and cfg4 (2048^3 u8), both after smoothVolume(sigma = 2) -- the raw noise ball's surface
exceeds the 32-bit index range -- at the first of a few iso values (fractions of the smoothed volume's range) that yields
between 10^6 and 10^8 triangles.  Bricked layout, VR_QUIRK_U16_OFFSET off (iso in stored units).  kernel_ms = median (and min)
of `--reps` calls after `--warmup` untimed ones (sustained clocks), each the HIP-event time of the call's kernels
(vr_get_mesh_ms: the counting pass plus the emitting pass, every slab; allocations excluded).  floor_ms = (the volume's bytes +
the mesh's bytes) / the vr_measure_stream_read rate of the same process: one read of every voxel, one write of the mesh.
x_floor = kernel_ms / floor_ms.  cpu_ref_256_ms is the CPU restatement (tests/mesh_ref/mesh_ref.c, one thread) on 256^3 voxels
around the mesh's middle vertex (the volume's centre lies inside the ball: no surface there), for scale; the device mesh of that
crop (a second handle) is compared with it bit for bit.

    python tools/mesh_ms.py [--reps 9] [--warmup 3] [--out profiles/mesh_ms.json] [--no-cfg4] [--only NAME]

--only NAME runs that one case without the crop: the shape for a rocprofv3 pass.
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

_spec = importlib.util.spec_from_file_location("mesh_ref_binding", ROOT / "tests" / "mesh_ref" / "binding.py")
mesh_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mesh_ref)

CASES = [
    dict(name="cfg3_sigma2", dims=(1024, 1024, 1024), bytes=2, seed=0xC0FFEE),
    dict(name="cfg4_sigma2", dims=(2048, 2048, 2048), bytes=1, seed=0x9E3779B9),
]
SIGMA = (2.0, 2.0, 2.0)
FRACTIONS = (0.5, 0.35, 0.65, 0.25, 0.75, 0.15, 0.85)
CROP = 256


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
    todo = [c for c in CASES if not (args.no_cfg4 and c["name"].startswith("cfg4"))]
    if args.only:
        todo = [c for c in todo if c["name"] == args.only]
        if not todo:
            raise SystemExit(f"--only: no case {args.only}; known: {[c['name'] for c in CASES]}")
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        lib = None if args.only else mesh_ref.build(tmp)
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
                lo, hi = r.dataset_range
                iso, counts, tried = None, None, []
                for f in FRACTIONS:
                    cand = int(round(lo + f * (hi - lo)))
                    try:
                        nv, nt = r.extractIsosurface(cand)
                    except vra.VRError as e:
                        tried.append(dict(iso=cand, refused=e.code))
                        r.takeMessage()
                        continue
                    tried.append(dict(iso=cand, vertices=nv, triangles=nt))
                    if 10 ** 6 <= nt <= 10 ** 8:
                        iso, counts = cand, (nv, nt)
                        break
                if iso is None:
                    print(json.dumps(dict(case=c["name"], error="no iso value with 1e6 .. 1e8 triangles", tried=tried)), flush=True)
                    continue
                for _ in range(args.warmup):
                    r.extractIsosurface(iso)
                ms = []
                for _ in range(args.reps):
                    assert r.extractIsosurface(iso) == counts
                    ms.append(r.meshMs())
                med = statistics.median(ms)
                vol_bytes = nx * ny * nz * c["bytes"]
                mesh_bytes = 24 * counts[0] + 12 * counts[1]
                floor_ms = (vol_bytes + mesh_bytes) / (gbps * 1e9) * 1e3
                d = dict(case=c["name"], volume=f"{nx}x{ny}x{nz} u{8 * c['bytes']} noise ball", layout="bricked", sigma=list(SIGMA),
                         dataset_range=[lo, hi], iso=iso, vertices=counts[0], triangles=counts[1], mesh_bytes=mesh_bytes, reps=args.reps,
                         kernel_ms=round(med, 4), kernel_ms_min=round(min(ms), 4), stream_read_gbps=round(gbps, 1),
                         floor_ms=round(floor_ms, 4), x_floor=round(med / floor_ms, 2), iso_values_tried=tried)
                if lib is not None:
                    vol = r.readVolume()
                    mid = r.readMesh()[0][counts[0] // 2]           # spacing 1: millimetres are voxel indices
                    o = [int(min(max(int(m) - CROP // 2, 0), n - CROP)) for m, n in zip(mid, (nx, ny, nz))]
                    d["crop_origin"] = o
                    crop = np.ascontiguousarray(vol[o[2]:o[2] + CROP, o[1]:o[1] + CROP, o[0]:o[0] + CROP])
                    del vol
                    t0 = time.perf_counter()
                    want = mesh_ref.extract(lib, crop, float(iso), (1.0, 1.0, 1.0))
                    d["cpu_ref_256_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    d["cpu_ref_256_triangles"] = int(want[2].shape[0])
                    with vra.RendererCore(0) as q:
                        q.setup((64, 48))
                        assert q.loadShader("VolumeRenderer.cs")
                        q.setLayout(R.LAYOUT_BRICKED)
                        q.setQuirks(0)
                        q.setVolume(crop, (1.0, 1.0, 1.0))
                        q.extractIsosurface(iso)
                        got = q.readMesh()
                        d["gpu_256_kernel_ms"] = round(q.meshMs(), 4)
                    d["crop_mesh_bit_exact"] = bool(all(g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))
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
