"""Kernel time of gradient-lit compositing (vr_set_shading), one JSON line per case, each beside its unshaded composite frame
measured in the same process on the same renderer.

Cases: cfg3 (1024^3 u16 noise ball, 1920x1080) NEAREST and TRILINEAR on the grey ramp over the whole data range (every
non-zero sample is shaded: the worst case); cfg3 NEAREST and TRILINEAR with a transfer function and skipping; the cfg2 shape
(512x512x452 u16, 1920x1080) NEAREST on the grey ramp; cfg4 (2048^3 u8, 3840x2160) NEAREST with a transfer function and
skipping.  Alpha 0.004 (the headline's), default coefficients (0.15, 0.65, 0.2, 16).  kernel_ms = median (and min) of
`--frames` HIP-event-timed frames after `--warmup` untimed ones; samples come from vr_count_samples; the cfg3 cases also check
their middle row (RGBA bits, counts) against the CPU definition, tests/shade_ref/shade_ref.c.

    python tools/shade_ms.py [--frames 30] [--warmup 10] [--out profiles/shade_ms.json] [--no-cfg4] [--only NAME]

--only NAME times the shaded frame of that one case (no unshaded frame, no reference check): the shape for a rocprofv3 pass.
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

_spec = importlib.util.spec_from_file_location("shade_ref_binding", ROOT / "tests" / "shade_ref" / "binding.py")
shade_ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(shade_ref)

CELLS = {
    "cfg3": dict(dims=(1024, 1024, 1024), bytes=2, size=(1920, 1080), seed=0xC0FFEE),
    "cfg2": dict(dims=(512, 512, 452), bytes=2, size=(1920, 1080), seed=0x1234),
    "cfg4": dict(dims=(2048, 2048, 2048), bytes=1, size=(3840, 2160), seed=0x9E3779B9),
}
TF_ISO = [0, 60, 140, 255]
TF_RGBA = [[0.2, 0.9, 0.1, 0.0], [0.9, 0.3, 0.2, 0.4], [1.0, 0.8, 0.6, 0.8], [0.5, 0.5, 1.0, 1.0]]
ALPHA = 0.004


def cases(cfg4=True):
    out = [dict(cell="cfg3", filter=0, tf=False), dict(cell="cfg3", filter=1, tf=False),
           dict(cell="cfg3", filter=0, tf=True), dict(cell="cfg3", filter=1, tf=True),
           dict(cell="cfg2", filter=0, tf=False)]
    if cfg4:
        out.append(dict(cell="cfg4", filter=0, tf=True))
    for c in out:
        c["name"] = f"{c['cell']}_{['nearest', 'trilinear'][c['filter']]}_{'tf_skip' if c['tf'] else 'grey'}"
    return out


def time_frames(r, frames, warmup):
    for _ in range(warmup):
        r.render()
    r.kernelMsTake()
    ms = []
    for _ in range(frames):
        r.render()
        ms.append(r.kernelMsTake())
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cfg4", action="store_true")
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    vra = importlib.import_module("volume-renderer_amd")
    oracle = importlib.import_module("oracle")
    R = vra.renderer
    todo = cases(not args.no_cfg4)
    if args.only:
        todo = [c for c in todo if c["name"] == args.only]
        if not todo:
            raise SystemExit(f"--only: no case {args.only}; known: {[c['name'] for c in cases()]}")
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    blob = ROOT / "profiles" / "launch_choices.bin"
    with tempfile.TemporaryDirectory() as tmp:
        lib = shade_ref.build(tmp)
        for cell, cfg in CELLS.items():
            mine = [c for c in todo if c["cell"] == cell]
            if not mine:
                continue
            w, h = cfg["size"]
            with vra.RendererCore(0) as r:
                r.setup((w, h))
                assert r.loadShader("VolumeRenderer.cs")
                r.setLayout(R.LAYOUT_BRICKED)
                imported = r.importChoices(blob.read_bytes()) if blob.exists() else 0
                r.generateSynthetic(R.SYNTH_NOISE_BALL, cfg["dims"], cfg["bytes"], cfg["seed"])
                check_row = cell == "cfg3" and not args.only
                vol = r.readVolume() if check_row else None
                # the grey ramp over the whole stored range (u16: HU -1000 .. 3095 = stored 0 .. 4095)
                lo_w, hi_w = (-1000, 3095) if cfg["bytes"] == 2 else (0, 255)
                off = 1000 if cfg["bytes"] == 2 else 0
                r.setWindow(lo_w, hi_w)
                r.setAlpha(ALPHA)
                cam = oracle.Camera().block()
                r.setCameraBlock(cam)
                for c in mine:
                    r.setFilter(c["filter"])
                    r.setSkipEmpty(c["tf"])
                    r.setTransferFunction(TF_ISO, TF_RGBA) if c["tf"] else r.setTransferFunction()
                    d = dict(case=c["name"], volume=f"{'x'.join(map(str, cfg['dims']))} u{8 * cfg['bytes']} noise ball", image=f"{w}x{h}",
                             filter=["NEAREST", "TRILINEAR"][c["filter"]], transfer_function=c["tf"], skip_empty=c["tf"], alpha=ALPHA,
                             coefficients=[0.15, 0.65, 0.2, 16], frames=args.frames, choices_imported=int(imported))
                    if not args.only:
                        r.setShading(False)
                        med, lo = time_frames(r, args.frames, args.warmup + 10)     # (+10: the measured choice settles first)
                        d.update(composite_ms=round(med, 4), composite_ms_min=round(lo, 4), composite_kernel=r.last_kernel_name)
                    r.setShading(True)
                    med, lo = time_frames(r, args.frames, args.warmup)
                    samples = r.countSamples()
                    d.update(kernel_ms=round(med, 4), kernel_ms_min=round(lo, 4), samples=int(samples),
                             gsamples_per_s=round(samples / (med * 1e-3) / 1e9, 2), kernel=r.last_kernel_name)
                    if "composite_ms" in d:
                        d["x_composite"] = round(d["kernel_ms"] / d["composite_ms"], 2)
                    if vol is not None:
                        y = h // 2
                        got = (r.readPixels()[y:y + 1], r.countSamples(per_pixel=True)[1][y:y + 1])
                        p = oracle.OracleParams(w, h, cam=cam, alpha_scale=ALPHA, min_val=lo_w + off, max_val=hi_w + off, filter=c["filter"],
                                                tf_rgba=r.getTransferLut() if c["tf"] else None, row_begin=y, row_end=y + 1)
                        want = shade_ref.render(lib, vol, p)
                        d["row_bit_exact"] = bool(np.array_equal(got[0].view(np.uint32), want[0][y:y + 1].view(np.uint32)) and
                                                  np.array_equal(got[1], want[1][y:y + 1]))
                    emit(d)
                r.setShading(False)
                del vol
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
