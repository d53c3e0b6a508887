#!/usr/bin/env python3
"""GPU tool: what face alignment costs next to detection (DESIGN.md "Face alignment"; writes profiles/align_bench.json).

Workload: 256 seeded 448 x 448 frames resident in HBM, fp16 engine.  Three calls are timed in alternation, each in windows of
at least --min-seconds after warm-up, median of three windows:
  detect      rf_detect_batch_device
  fused       rf_detect_align_batch_device (crops into a device buffer, matrices to the host)
  standalone  rf_align_batch_device on the faces `detect` returned (same outputs)
A separate `rocprofv3 --kernel-trace` run of this file (--trace-child) gives the alignment kernel's own time; bytes are counted
from shapes: 3 S^2 written per face, and the source footprint of a crop, 3 S^2 / det(forward matrix) bytes (the area the crop
covers in the source frame, what has to come from HBM once).

usage: python tools/align_bench.py [--out profiles/align_bench.json] [--crop 112] [--max-faces 8] [--min-seconds 0.5] [--no-trace]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK = 8e12        # bytes / s, MI355X


class Workload:
    def __init__(self, n, crop, max_faces, batch):
        import torch
        import retinaface_amd
        from retinaface_amd import _lib
        from retinaface_amd.frames import synth_frames
        assert torch.cuda.is_available(), "this tool measures: it needs the GPU"
        self.torch, self._lib = torch, _lib
        self.n, self.S, self.mf = n, crop, max_faces
        self.frames = torch.from_numpy(np.stack(synth_frames(448, 448, n, config=1))).cuda()
        torch.cuda.synchronize()
        self.det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", 0.4, precision=retinaface_amd.PRECISION_FP16,
                                             net_hw=(448, 448), model_stem="mnet-deconv-0517", max_batch=batch)
        self.lib, self.h = self.det._lib, self.det._h
        self.cap = self.det.max_detections
        self.ptrs = (C.c_void_p * n)(*[self.frames[i].data_ptr() for i in range(n)])
        self.rows, self.cols = (C.c_int * n)(*[448] * n), (C.c_int * n)(*[448] * n)
        self.steps = (C.c_int * n)(*[448 * 3] * n)
        self.out = (_lib.rf_face * (n * self.cap))()
        self.counts = (C.c_int * n)()
        self.d_crops = torch.zeros((n * max_faces * crop * crop * 3,), dtype=torch.uint8, device="cuda")
        self.mats = np.zeros((n, max_faces, 6), np.float64)
        self.mats_p = self.mats.ctypes.data_as(C.POINTER(C.c_double))

    def detect(self):
        self._lib.check(self.lib.rf_detect_batch_device(self.h, self.ptrs, self.rows, self.cols, self.steps, self.n, 0.5, self.out, self.cap,
                                                        self.counts), self.h)

    def fused(self):
        self._lib.check(self.lib.rf_detect_align_batch_device(self.h, self.ptrs, self.rows, self.cols, self.steps, self.n, 0.5, self.out, self.cap,
                                                              self.counts, self.S, self.mf, C.c_void_p(self.d_crops.data_ptr()), None,
                                                              self.mats_p), self.h)

    def standalone(self):
        self._lib.check(self.lib.rf_align_batch_device(self.h, self.ptrs, self.rows, self.cols, self.steps, self.n, self.out, self.cap, self.counts,
                                                       None, self.S, self.mf, C.c_void_p(self.d_crops.data_ptr()), None, self.mats_p), self.h)

    def faces(self):
        return int(sum(min(c, self.mf) for c in self.counts))


def window(fn, min_seconds):
    t0 = time.perf_counter()
    calls = 0
    while True:
        fn()                      # every call is synchronous: it returns after its device work has finished
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / calls


def trace_child(args):
    w = Workload(args.n, args.crop, args.max_faces, args.batch)
    for _ in range(3):
        w.detect(); w.fused(); w.standalone()
    for _ in range(20):
        w.fused(); w.standalone()


def kernel_time_from_trace(args):
    """average duration (s) of the alignment kernel's dispatches in a rocprofv3 kernel trace of --trace-child, and their count"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "align", "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--n", str(args.n), "--crop", str(args.crop), "--max-faces", str(args.max_faces),
               "--batch", str(args.batch)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed:\n" + r.stderr[-2000:])
        durs = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "align_kernel" in row.get("Kernel_Name", ""):
                    durs.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-9)
        if not durs:
            raise RuntimeError("no align_kernel dispatch in the kernel trace")
        return statistics.mean(durs), statistics.median(durs), len(durs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"))
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--crop", type=int, default=112)
    ap.add_argument("--max-faces", type=int, default=8)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    args = ap.parse_args()
    if args.trace_child:
        return trace_child(args)

    w = Workload(args.n, args.crop, args.max_faces, args.batch)
    calls = {"detect": w.detect, "fused": w.fused, "standalone": w.standalone}
    for _ in range(5):                          # warm-up: every shape, graph capture, scratch allocation
        for fn in calls.values():
            fn()
    faces = w.faces()
    samples = {k: [] for k in calls}
    for _ in range(3):                          # alternate, so drift hits all three alike
        for k, fn in calls.items():
            samples[k].append(window(fn, args.min_seconds))
    med = {k: statistics.median(v) for k, v in samples.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in samples.items()}
    S = args.crop
    det2 = np.array([w.mats[i, k, 0] * w.mats[i, k, 4] - w.mats[i, k, 1] * w.mats[i, k, 3]
                     for i in range(args.n) for k in range(min(w.counts[i], args.max_faces))])
    footprint = float((3.0 * S * S / det2[det2 > 0]).sum())
    res = {
        "tool": "tools/align_bench.py", "frames": args.n, "net": "448x448", "precision": "fp16", "model": "mnet-deconv-0517",
        "max_batch": args.batch, "crop_size": S, "max_faces": args.max_faces, "faces_per_call": faces,
        "window_seconds": args.min_seconds, "windows": 3,
        "call_ms": {k: med[k] * 1e3 for k in med},
        "call_ms_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
        "relative_spread": spread,
        "fused_minus_detect_ms": (med["fused"] - med["detect"]) * 1e3,
        "fused_le_detect_plus_standalone": bool(med["fused"] <= med["detect"] + med["standalone"]),
        "faces_per_second": {"fused": faces / med["fused"], "standalone": faces / med["standalone"]},
        "us_per_face": {"fused_minus_detect": (med["fused"] - med["detect"]) / max(faces, 1) * 1e6,
                        "standalone": med["standalone"] / max(faces, 1) * 1e6},
        "bytes_written_per_face": 3 * S * S, "bytes_written_per_call": 3 * S * S * faces,
        "source_footprint_bytes_per_call": footprint,
    }
    if not args.no_trace:
        # (this process keeps its handle idle meanwhile; the traced child opens its own)
        avg, mid, n_disp = kernel_time_from_trace(args)
        res["align_kernel"] = {"source": "rocprofv3 --kernel-trace --stats, separate run", "dispatches": n_disp,
                               "avg_us": avg * 1e6, "median_us": mid * 1e6,
                               "us_per_face": avg / max(faces, 1) * 1e6,
                               "hbm_fraction_of_8TBps": (footprint + 3 * S * S * faces) / avg / HBM_PEAK}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
