"""Device time of vr_smooth_mesh, one JSON line per mesh, each step beside its streaming floor.

Meshes: those of profiles/simplify_ms.json -- cfg3 (1024^3 u16 noise ball) and cfg4 (2048^3 u8), both after smoothVolume(sigma = 2),
at that file's iso values, spacing 1 -- as extracted (cell 0) and simplified on cells of 2 and of 4 voxel spacings.  Bricked layout,
VR_QUIRK_U16_OFFSET off.  Every timed call smooths a fresh extraction (and simplification), both untimed, with lambda 0.5, mu -0.53 and
the boundary fixed.  build_ms and iterate_ms = medians of `--reps` calls at 10 iterations after `--warmup` untimed ones, each the
HIP-event time vr_get_mesh_smooth_ms reports (the graph; the steps and normals; allocations and read-backs excluded).
step_ms = (iterate_ms at 10 iterations - iterate_ms at 1 iteration) / 18: the 18 steps the longer call adds, free of the
face vectors, the corner sort and the normals.  floor_ms = per step one read and one write of the positions as stored (12 bytes a
vertex each) plus one read of the rows (8 bytes a vertex) and of the neighbour indices (4 bytes a distinct directed pair: counted on
the host where the mesh has at most --count-pairs-below triangles, else 3 T, every edge in two triangles), over the
vr_measure_stream_read rate of the same process.  x_floor = step_ms / floor_ms.
The last line is a 256^3 u16 noise ball's mesh (sigma 2) on the device and by the CPU restatement
(tests/mesh_smooth_ref/mesh_smooth_ref.c, one thread), compared bit for bit.

    python tools/mesh_smooth_ms.py [--reps 5] [--warmup 2] [--out profiles/mesh_smooth_ms.json] [--no-cfg4] [--only NAME] [--cells 0 2 4] [--no-cpu]

--only NAME --cells C --reps 1 --warmup 0 --no-cpu is the shape for a rocprofv3 --kernel-trace --stats pass (a run of its own).
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

_spec = importlib.util.spec_from_file_location("mesh_smooth_ref_binding", ROOT / "tests" / "mesh_smooth_ref" / "binding.py")
smooth_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(smooth_ref)

CASES = [
    dict(name="cfg3_sigma2", dims=(1024, 1024, 1024), bytes=2, seed=0xC0FFEE, iso=2057),
    dict(name="cfg4_sigma2", dims=(2048, 2048, 2048), bytes=1, seed=0x9E3779B9, iso=128),
]
CPU_CASE = dict(name="cpu_256", dims=(256, 256, 256), bytes=2, seed=0xC0FFEE, iso=2057)
SIGMA = (2.0, 2.0, 2.0)
ITERATIONS, LAM, MU, FIX = 10, 0.5, -0.53, True


def distinct_pairs(tri: np.ndarray) -> int:
    t = tri.astype(np.uint64)
    lo, hi = np.minimum(t, np.roll(t, -1, axis=1)), np.maximum(t, np.roll(t, -1, axis=1))
    edges = np.unique((lo << np.uint64(32) | hi).ravel())
    return 2 * int(edges.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cfg4", action="store_true")
    ap.add_argument("--only", default=None)
    ap.add_argument("--cells", type=float, nargs="+", default=[0.0, 2.0, 4.0])
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--count-pairs-below", type=int, default=5000000)
    args = ap.parse_args()
    vra = importlib.import_module("volume-renderer_amd")
    R = vra.renderer
    todo = [c for c in CASES if not (args.no_cfg4 and c["name"].startswith("cfg4"))]
    if args.only:
        todo = [c for c in todo if c["name"] == args.only]
        if not todo:
            raise SystemExit(f"--only: no case {args.only}; known: {[c['name'] for c in CASES]}")
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    def resident(r, c):
        r.setup((64, 48))
        assert r.loadShader("VolumeRenderer.cs")
        r.setLayout(R.LAYOUT_BRICKED)
        r.setQuirks(0)
        r.generateSynthetic(R.SYNTH_NOISE_BALL, c["dims"], c["bytes"], c["seed"])
        r.smoothVolume(sigma_voxels=SIGMA)

    for c in todo:
        nx, ny, nz = c["dims"]
        with vra.RendererCore(0) as r:
            resident(r, c)
            gbps = r.measureStreamRead(5)
            for cell in args.cells:
                def fresh():
                    r.extractIsosurface(c["iso"])
                    if cell > 0:
                        r.simplifyMesh(cell)
                    return r.meshInfo()
                info = fresh()
                nv, nt = info["vertices"], info["triangles"]
                exact = nt <= args.count_pairs_below
                pairs = distinct_pairs(r.readMesh()[2]) if exact else 3 * nt
                times = {ITERATIONS: ([], []), 1: ([], [])}
                fixed = None
                for iterations, (build, iterate) in times.items():
                    for i in range(args.warmup + args.reps):
                        fresh()
                        n_fixed = r.smoothMesh(iterations, LAM, MU, FIX)
                        assert fixed in (None, n_fixed)
                        fixed = n_fixed
                        if i >= args.warmup:
                            ms = r.meshSmoothMs()
                            build.append(ms["build_ms"])
                            iterate.append(ms["iterate_ms"])
                build_ms, iterate_ms = statistics.median(times[ITERATIONS][0] + times[1][0]), statistics.median(times[ITERATIONS][1])
                step_ms = (iterate_ms - statistics.median(times[1][1])) / (2 * (ITERATIONS - 1))
                step_bytes = 2 * 12 * nv + 8 * nv + 4 * pairs
                floor_ms = step_bytes / (gbps * 1e9) * 1e3
                emit(dict(case=c["name"], volume=f"{nx}x{ny}x{nz} u{8 * c['bytes']} noise ball", sigma=list(SIGMA), iso=c["iso"], cell=cell,
                          vertices=nv, triangles=nt, fixed_vertices=fixed, distinct_pairs=pairs, distinct_pairs_counted=exact,
                          iterations=ITERATIONS, lam=LAM, mu=MU, fix_boundary=FIX, reps=args.reps,
                          build_ms=round(build_ms, 4), iterate_ms=round(iterate_ms, 4), iterate_ms_min=round(min(times[ITERATIONS][1]), 4),
                          iterate_ms_1_iteration=round(statistics.median(times[1][1]), 4), step_ms=round(step_ms, 5),
                          step_bytes=step_bytes, stream_read_gbps=round(gbps, 1), floor_ms=round(floor_ms, 5), x_floor=round(step_ms / floor_ms, 2)))
    if not args.no_cpu and not args.only:
        c = CPU_CASE
        with tempfile.TemporaryDirectory() as tmp, vra.RendererCore(0) as r:
            lib = smooth_ref.build(tmp)
            resident(r, c)
            nv, nt = r.extractIsosurface(c["iso"])
            source = r.readMesh()
            r.smoothMesh(ITERATIONS, LAM, MU, FIX)               # (the first call also loads the code object)
            r.extractIsosurface(c["iso"])
            fixed = r.smoothMesh(ITERATIONS, LAM, MU, FIX)
            ms = r.meshSmoothMs()
            got = r.readMesh()
            t0 = time.perf_counter()
            want, want_fixed = smooth_ref.smooth(lib, source, ITERATIONS, LAM, MU, FIX)
            cpu_ms = (time.perf_counter() - t0) * 1e3
            same = bool(all(g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want)))
            emit(dict(case=c["name"], volume="256x256x256 u16 noise ball", sigma=list(SIGMA), iso=c["iso"], cell=0.0, vertices=nv, triangles=nt,
                      fixed_vertices=fixed, iterations=ITERATIONS, lam=LAM, mu=MU, fix_boundary=FIX, build_ms=round(ms["build_ms"], 4),
                      iterate_ms=round(ms["iterate_ms"], 4), cpu_restatement_ms=round(cpu_ms, 1),
                      cpu_over_device=round(cpu_ms / (ms["build_ms"] + ms["iterate_ms"]), 1),
                      bit_exact_with_cpu_restatement=same and fixed == int(want_fixed.sum())))
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
