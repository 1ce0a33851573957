"""The ray-ordered sample stream of a still view (vr_set_ray_stream, vr_stream.hip): what a replayed frame costs beside the gather
kernels' frame of the same state, what the build costs and what it holds resident -- one JSON document.

Shapes: cfg3 (bench.py's headline: 1024^3 u16 noise ball, 1920x1080, window [0,4095], alpha 0.004), the cfg1 shape (256^3 u8
sphere, 1280x720, alpha 1) and the cfg2 shape (512x512x452 u16, 1920x1080, window [1000,5095], alpha 0.05).  Per shape, after
150 untimed frames (sustained clocks), tools/quick_ms.py's method -- the mean HIP-event kernel time of `--reps` blocking frames:
  gather_ms     vr_set_ray_stream 0: the measured choice's gather kernel (what the first frame of a new view costs)
  replay_ms     vr_set_ray_stream 2, vr_set_ray_stream_pack 0: raymarch_stream_kernel (the unpacked stream)
  build_ms      wall time of the frame that builds (count pass, scan, the blocking read-back, allocation, record pass) minus a
                replayed frame's wall time; build_ms_again: a rebuild into the kept allocation (after a camera nudge)
  stream_bytes  vr_get_ray_stream_bytes; padding = the stream's sample bytes / (samples of the frame x bytes per voxel)
  floor_ms      stream_bytes / the vr_measure_stream_read rate of the same process
  bit_identical the replayed frame equals the gathered one, view(uint32)
  by_table_mode vr_set_ray_stream_table 0, 1 and 2 (never / automatic / wherever eligible) on the same stream: replay_ms, whether
                the hybrid classification was the path taken, and the frame against the gathered one; replay_ms above is mode 1's
16-bit shapes also, under `packed` (vr_set_ray_stream_pack 2: raymarch_stream12_kernel, 12 bits per sample): replay_ms, build_ms (a
build into the kept, larger allocation), stream_bytes (of a fresh handle's allocation: the model's packed size), floor_ms, x_floor,
bit_identical, and automatic_packs -- whether the default mode packs this shape.
cfg3 also: nudged_ms -- the camera nudged every frame in the default mode (the gather kernel, the key comparison on the host).

    python tools/stream_ms.py [--reps 40] [--out profiles/stream_ms.json] [--only cfg3]
"""
from __future__ import annotations

import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = {
    "cfg3": dict(size=(1920, 1080), synth="ball", dims=(1024, 1024, 1024), bytes=2, param=0x9E3779B9, window=(0, 4095), alpha=0.004),
    "cfg1_shape": dict(size=(1280, 720), synth="sphere", dims=(256, 256, 256), bytes=1, param=112, window=(0, 255), alpha=1.0),
    "cfg2_shape": dict(size=(1920, 1080), synth="ball", dims=(512, 512, 452), bytes=2, param=0x9E3779B9, window=(1000, 5095), alpha=0.05),
}


def kernel_ms(r, n):
    r.render(); r.kernelMsTake()
    for _ in range(n):
        r.render()
    return r.kernelMsTake() / n


def table_modes(r, reps, gathered):
    """the replayed frame under every table mode; leaves the default mode set"""
    res = {}
    for m in (0, 1, 2):
        r.setRayStreamTable(m)
        res[str(m)] = {"replay_ms": round(kernel_ms(r, reps), 4), "hybrid": r.rayStreamTableUsed(),
                       "bit_identical": bool(np.array_equal(r.readPixels().view(np.uint32), gathered.view(np.uint32)))}
    r.setRayStreamTable(1)
    return res


def wall_ms(r):
    r.synchronize()
    t0 = time.perf_counter()
    r.render()
    return (time.perf_counter() - t0) * 1e3


def measure(vra, name, s, reps):
    R = vra.renderer
    with vra.RendererCore(0) as r:
        r.setup(s["size"]); r.loadShader("VolumeRenderer.cs"); r.setQuirks(0)
        r.generateSynthetic(R.SYNTH_SPHERE_U8 if s["synth"] == "sphere" else R.SYNTH_NOISE_BALL, s["dims"], s["bytes"], s["param"])
        r.setWindow(*s["window"]); r.setAlpha(s["alpha"])
        r.setRayStream(0)
        r.setRayStreamPack(0)
        for _ in range(150):
            r.renderAsync()
        r.synchronize()
        out = {"gather_ms": round(kernel_ms(r, reps), 4), "gather_kernel": r.last_kernel_name, "launch_choice": r.last_launch_choice}
        gathered = r.readPixels().copy()
        samples = r.countSamples()
        copies = r.residentBytes()[1]
        r.setRayStream(2)
        built = wall_ms(r)
        replay_wall = min(wall_ms(r) for _ in range(5))
        out["build_ms"] = round(built - replay_wall, 3)
        out["replay_ms"] = round(kernel_ms(r, reps), 4)
        out["replay_kernel"] = r.last_kernel_name
        out["bit_identical"] = bool(np.array_equal(r.readPixels().view(np.uint32), gathered.view(np.uint32)))
        out["by_table_mode"] = table_modes(r, reps, gathered)
        out["stream_bytes"] = r.rayStreamBytes()
        out["copies_bytes_before"] = copies
        out["copies_bytes_with_stream"] = r.residentBytes()[1]
        w, h = s["size"]
        blocks = ((w + 31) // 32) * 4 * ((h + 15) // 16) * 2
        sample_bytes = out["stream_bytes"] - blocks * 64 * 2 - (blocks + 1) * 8 - 16
        out["samples_per_frame"] = samples
        out["padding"] = round(sample_bytes / (samples * s["bytes"]), 4)
        gbps = r.measureStreamRead(5)
        out["measured_stream_read_gbps"] = round(gbps, 1)
        out["floor_ms"] = round(out["stream_bytes"] / (gbps * 1e9) * 1e3, 4)
        out["x_floor"] = round(out["replay_ms"] / out["floor_ms"], 2)
        out["speedup"] = round(out["gather_ms"] / out["replay_ms"], 2)
        r.cameraOrient(0.0, 0.0005, 0.0)                               # a new view: the stream is rebuilt into the kept allocation
        out["build_ms_again"] = round(wall_ms(r) - replay_wall, 3)
        out["builds"] = r.rayStreamBuilds()
        if s["bytes"] == 2:
            r.setRayStream(0)                                          # (the nudged view: its own gathered frame to compare with)
            r.render()
            gathered = r.readPixels().copy()
            r.setRayStream(2)
            r.setRayStreamPack(2)
            built = wall_ms(r)
            replay_wall = min(wall_ms(r) for _ in range(5))
            pk = {"build_ms": round(built - replay_wall, 3), "replay_ms": round(kernel_ms(r, reps), 4), "replay_kernel": r.last_kernel_name}
            pk["bit_identical"] = bool(np.array_equal(r.readPixels().view(np.uint32), gathered.view(np.uint32)))
            pk["by_table_mode"] = table_modes(r, reps, gathered)
            # the packed size from the unpacked one (the allocation on this handle is the kept, larger one): groups of 8 instead
            # of 4 need the blocks' lengths, so it is read from a handle that only ever built the packed stream -- below
            pk["stream_bytes_allocated_here"] = r.rayStreamBytes()
            r.setRayStreamPack(1)
            r.render()
            pk["automatic_packs"] = r.last_kernel_name == pk["replay_kernel"]
            out["packed"] = pk
        if name == "cfg3":
            r.setRayStream(1)
            runs = []
            for _ in range(5):
                r.kernelMsTake()
                for i in range(60):
                    r.cameraOrient(0.0, 0.0005 * (1 if i % 2 else -1), 0.0)
                    r.render()
                runs.append(round(r.kernelMsTake() / 60, 4))
            out["nudged_ms_runs"] = runs
            out["nudged_kernel"] = r.last_kernel_name
            out["builds_after_nudging"] = r.rayStreamBuilds()
    if "packed" in out:
        with vra.RendererCore(0) as r:                                 # a fresh handle: the packed stream's own allocation
            r.setup(s["size"]); r.loadShader("VolumeRenderer.cs"); r.setQuirks(0)
            r.generateSynthetic(R.SYNTH_NOISE_BALL, s["dims"], s["bytes"], s["param"])
            r.setWindow(*s["window"]); r.setAlpha(s["alpha"])
            r.setRayStreamPack(2); r.setRayStream(2)
            built = wall_ms(r)
            replay_wall = min(wall_ms(r) for _ in range(5))
            pk = out["packed"]
            pk["build_ms_fresh"] = round(built - replay_wall, 3)       # (includes the first allocation)
            pk["stream_bytes"] = r.rayStreamBytes()
            pk["floor_ms"] = round(pk["stream_bytes"] / (out["measured_stream_read_gbps"] * 1e9) * 1e3, 4)
            pk["x_floor"] = round(pk["replay_ms"] / pk["floor_ms"], 2)
            pk["speedup_over_unpacked"] = round(out["replay_ms"] / pk["replay_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    vra = importlib.import_module("volume-renderer_amd")
    doc = {}
    for name, s in SHAPES.items():
        if args.only and name != args.only:
            continue
        doc[name] = measure(vra, name, s, args.reps)
        print(json.dumps({name: doc[name]}), flush=True)
    if args.out:
        Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
