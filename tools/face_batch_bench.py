#!/usr/bin/env python3
"""GPU tool: what a recogniser-ready face batch costs next to detection, next to the u8 crops, and next to the conversion a
caller would otherwise write (DESIGN.md "Face batches"; writes profiles/face_batch_bench.json).

Workload as tools/align_bench.py: 256 seeded 448 x 448 frames resident in HBM, fp16 engine, S = 112, max_faces 8.  Five calls are
timed in alternation, each in windows of at least --min-seconds after warm-up, median of three windows:
  detect        (a) rf_detect_batch_device
  align         (b) rf_detect_align_batch_device (u8 slot array into a device buffer, matrices to the host)
  align_torch   (c) (b) + what a caller writes today in torch to get the dense fp16 RGB CHW tensor: gather of the occupied slots,
                    permute, flip, float, sub, mul, half -- then a device synchronise, so that (c) ends where (d) ends
  batch_f16     (d) rf_detect_face_batch_device, fp16 RGB CHW into a device buffer, matrices to the host
  batch_f32         the same in fp32
A separate `rocprofv3 --kernel-trace` run of this file (--trace-child) gives the two new kernels' own times; bytes are counted
from shapes as in align_bench.py: the source footprint of the crops (read once from HBM) + the tensor bytes written.

usage: python tools/face_batch_bench.py [--out profiles/face_batch_bench.json] [--min-seconds 0.5] [--no-trace]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from align_bench import HBM_PEAK, Workload, window  # noqa: E402


class FaceWorkload(Workload):
    def __init__(self, n, crop, max_faces, batch):
        super().__init__(n, crop, max_faces, batch)
        import retinaface_amd
        torch = self.torch
        self.capacity = n * max_faces
        self.specs, self.d_tensor = {}, {}
        for dtype, tdt in (("f16", torch.float16), ("f32", torch.float32)):
            self.specs[dtype] = retinaface_amd.face_batch_spec(crop, dtype, True, max_faces=max_faces, capacity=self.capacity)
            self.d_tensor[dtype] = torch.zeros((self.capacity, 3, crop, crop), dtype=tdt, device="cuda")
        self.offsets = (C.c_int * (n + 1))()
        self.pmats = np.zeros((self.capacity, 6), np.float64)
        self.pmats_p = self.pmats.ctypes.data_as(C.POINTER(C.c_double))
        self.slots = self.d_crops.view(n * max_faces, crop, crop, 3)

    def batch(self, dtype):
        self._lib.check(self.lib.rf_detect_face_batch_device(self.h, self.ptrs, self.rows, self.cols, self.steps, self.n, 0.5, self.out, self.cap,
                                                             self.counts, C.byref(self.specs[dtype]), C.c_void_p(self.d_tensor[dtype].data_ptr()),
                                                             None, self.pmats_p, self.offsets), self.h)

    def batch_f16(self):
        self.batch("f16")

    def batch_f32(self):
        self.batch("f32")

    def align_torch(self):
        torch = self.torch
        self.fused()
        idx = [i * self.mf + k for i in range(self.n) for k in range(min(self.counts[i], self.mf))]
        idx = torch.tensor(idx, dtype=torch.long).cuda()
        x = self.slots[idx].permute(0, 3, 1, 2).flip(1).float().sub(127.5).mul(1.0 / 128.0).half()
        torch.cuda.synchronize()
        return x


def trace_child(args):
    w = FaceWorkload(args.n, args.crop, args.max_faces, args.batch)
    for _ in range(3):
        w.detect(); w.batch_f16(); w.batch_f32()
    for _ in range(20):
        w.batch_f16(); w.batch_f32()


def kernel_times_from_trace(args):
    """per kernel-name fragment: (mean, median, dispatches) of its durations (s) in a rocprofv3 kernel trace of --trace-child"""
    def which(kn):                 # demangled ("face_batch_kernel<_Float16, true>") or mangled ("face_batch_kernelIDF16_Lb1E") names
        if "face_scan_kernel" in kn:
            return "scan"
        if "face_batch_kernel" not in kn:
            return None
        return "f16" if ("Float16" in kn or "DF16" in kn) else "f32" if ("<float" in kn or "IfLb" in kn) else None
    durs = {"f16": [], "f32": [], "scan": []}
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "face_batch", "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--n", str(args.n), "--crop", str(args.crop), "--max-faces", str(args.max_faces),
               "--batch", str(args.batch)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed:\n" + r.stderr[-2000:])
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                k = which(row.get("Kernel_Name", ""))
                if k:
                    durs[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-9)
    if not durs["f16"] or not durs["f32"]:
        raise RuntimeError("no face_batch_kernel dispatch in the kernel trace")
    return {k: (statistics.mean(v), statistics.median(v), len(v)) for k, v in durs.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_batch_bench.json"))
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

    w = FaceWorkload(args.n, args.crop, args.max_faces, args.batch)
    calls = {"detect": w.detect, "align": w.fused, "align_torch": w.align_torch, "batch_f16": w.batch_f16, "batch_f32": w.batch_f32}
    for _ in range(5):                          # warm-up: every shape, graph capture, scratch allocation, torch's kernels
        for fn in calls.values():
            fn()
    # the two routes to the fp16 tensor agree (torch computes (v - 127.5) / 128 exactly as well: every step is exact in fp32)
    w.batch_f16()
    faces = int(w.offsets[args.n])
    same = bool(w.torch.equal(w.align_torch(), w.d_tensor["f16"][:faces]))
    samples = {k: [] for k in calls}
    for _ in range(3):                          # alternate, so drift hits all alike
        for k, fn in calls.items():
            samples[k].append(window(fn, args.min_seconds))
    med = {k: statistics.median(v) for k, v in samples.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in samples.items()}
    S = args.crop
    det2 = w.pmats[:faces, 0] * w.pmats[:faces, 4] - w.pmats[:faces, 1] * w.pmats[:faces, 3]
    footprint = float((3.0 * S * S / det2[det2 > 0]).sum())
    added = {k: (med[k] - med["detect"]) * 1e3 for k in med if k != "detect"}
    worst_spread_ms = max(spread[k] * med[k] for k in ("align_torch", "batch_f16")) * 1e3
    res = {
        "tool": "tools/face_batch_bench.py", "frames": args.n, "net": "448x448", "precision": "fp16", "model": "mnet-deconv-0517",
        "max_batch": args.batch, "crop_size": S, "max_faces": args.max_faces, "faces_per_call": faces,
        "window_seconds": args.min_seconds, "windows": 3,
        "call_ms": {k: med[k] * 1e3 for k in med},
        "call_ms_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
        "relative_spread": spread,
        "added_over_detect_ms": added,
        "torch_route_equals_face_batch": same,
        "batch_f16_minus_align_torch_ms": (med["batch_f16"] - med["align_torch"]) * 1e3,
        "batch_f16_beats_align_torch_by_more_than_the_spread": bool(med["align_torch"] - med["batch_f16"] > worst_spread_ms),
        "added_cost_ratio_to_align": {k: added[k] / added["align"] if added["align"] > 0 else None for k in ("batch_f16", "batch_f32")},
        "bytes_written_per_face": {"u8": 3 * S * S, "f16": 6 * S * S, "f32": 12 * S * S},
        "source_footprint_bytes_per_call": footprint,
    }
    if not args.no_trace:
        # (this process keeps its handle idle meanwhile; the traced child opens its own)
        res["kernels"] = {"source": "rocprofv3 --kernel-trace --stats, separate run"}
        for k, (avg, mid, n_disp) in kernel_times_from_trace(args).items():
            e = {"dispatches": n_disp, "avg_us": avg * 1e6, "median_us": mid * 1e6}
            if k != "scan":
                moved = footprint + (6 if k == "f16" else 12) * S * S * faces
                e.update({"us_per_face": avg / max(faces, 1) * 1e6, "bytes_moved": moved, "hbm_fraction_of_8TBps": moved / avg / HBM_PEAK})
            res["kernels"][k] = e
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
