"""Kernel time of the first-hit isosurface mode (vr_set_isosurface), one JSON line per cell.

Cells at the cfg3 size (1024^3 u16 noise ball, 1920x1080): default and off-axis pose x NEAREST / TRILINEAR x skipping off / on x
three iso values in stored units -- 2048 (the outer shell), 4000 (the core only), 5000 (above the maximum: no hit) -- and one cfg4
cell (2048^3 u8, 3840x2160).  kernel_ms = median of `--frames` HIP-event-timed frames after `--warmup` untimed ones; every cell
also checks its frame (RGBA bits, depth bits, sample counts) against the CPU definition, tests/iso_ref/iso_ref.c, on sampled rows.

    python tools/iso_ms.py [--frames 20] [--warmup 5] [--out profiles/iso_ms.json] [--no-cfg4]
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

_spec = importlib.util.spec_from_file_location("iso_ref_binding", ROOT / "tests" / "iso_ref" / "binding.py")
iso_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(iso_ref)

POSES = {"default": (0.0, 0.0), "offaxis": (0.5, 0.7)}


def cam_block(oracle, pose):
    c = oracle.Camera()
    z, a = POSES[pose]
    if z or a:
        c.orient(0.0, z, a)
    return c.block()


def time_frames(r, frames, warmup):
    for _ in range(warmup):
        r.render()
    r.kernelMsTake()
    ms = []
    for _ in range(frames):
        r.render()
        ms.append(r.kernelMsTake())
    return statistics.median(ms), min(ms), max(ms)


def check_rows(r, vol, oracle, lib, iso, cam, filt, rows):
    w, h = r.framebuffer_size
    rgba, depth = r.readPixels(), r.readDepth()
    _, spp = r.countSamples(per_pixel=True)
    hits = int(np.isfinite(depth).sum())
    for y in rows:
        want = iso_ref.render(lib, vol, oracle.OracleParams(w, h, cam=cam, filter=filt, row_begin=y, row_end=y + 1), iso)
        ok = (np.array_equal(rgba[y].view(np.uint32), want[0][y].view(np.uint32)) and
              np.array_equal(depth[y].view(np.uint32), want[1][y].view(np.uint32)) and np.array_equal(spp[y], want[2][y]))
        if not ok:
            return False, hits
    return True, hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cfg4", action="store_true")
    args = ap.parse_args()
    vra = importlib.import_module("volume-renderer_amd")
    import oracle

    R = vra.renderer
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as tmp:
        lib = iso_ref.build(tmp)
        with vra.RendererCore(0) as r:
            r.setup((1920, 1080))
            assert r.loadShader("VolumeRenderer.cs")
            r.setLayout(R.LAYOUT_BRICKED)
            r.generateSynthetic(R.SYNTH_NOISE_BALL, (1024, 1024, 1024), 2, 0xC0FFEE)
            vol = r.readVolume()
            for pose in POSES:
                cam = cam_block(oracle, pose)
                r.setCameraBlock(cam)
                for filt in (0, 1):
                    r.setFilter(filt)
                    for stored in (2048, 4000, 5000):
                        r.setIsosurface(True, stored - 1000)
                        for skip in (False, True):
                            r.setSkipEmpty(skip)
                            med, lo, hi = time_frames(r, args.frames, args.warmup)
                            ok, hits = check_rows(r, vol, oracle, lib, stored - 1000, cam, filt, (270, 540, 810))
                            emit(dict(cell="cfg3", volume="1024^3 u16 noise ball", image="1920x1080", pose=pose,
                                      filter=["NEAREST", "TRILINEAR"][filt], skip=skip, iso_stored=stored, kernel_ms=round(med, 4),
                                      kernel_ms_min=round(lo, 4), kernel_ms_max=round(hi, 4), frames=args.frames, hit_pixels=hits,
                                      kernel=r.last_kernel_name, rows_checked=3, rows_bit_exact=ok))
            del vol
        if not args.no_cfg4:
            with vra.RendererCore(0) as r:
                r.setup((3840, 2160))
                assert r.loadShader("VolumeRenderer.cs")
                r.setLayout(R.LAYOUT_BRICKED)
                r.generateSynthetic(R.SYNTH_NOISE_BALL, (2048, 2048, 2048), 1, 0x9E3779B9)
                vol = r.readVolume()
                cam = cam_block(oracle, "default")
                r.setCameraBlock(cam)
                r.setSkipEmpty(True)
                r.setIsosurface(True, 128)
                med, lo, hi = time_frames(r, max(args.frames // 2, 3), args.warmup)
                ok, hits = check_rows(r, vol, oracle, lib, 128, cam, 0, (1080,))
                emit(dict(cell="cfg4", volume="2048^3 u8 noise ball", image="3840x2160", pose="default", filter="NEAREST", skip=True,
                          iso_stored=128, kernel_ms=round(med, 4), kernel_ms_min=round(lo, 4), kernel_ms_max=round(hi, 4),
                          frames=max(args.frames // 2, 3), hit_pixels=hits, kernel=r.last_kernel_name, rows_checked=1, rows_bit_exact=ok))
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
