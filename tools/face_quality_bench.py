#!/usr/bin/env python3
"""GPU tool: what a quality gate in front of the face batch costs on the device, next to the ungated call and next to what a caller
writes today (DESIGN.md "Face quality"; writes profiles/face_quality_bench.json).

Workload as tools/face_batch_bench.py: 256 seeded 448 x 448 frames resident in HBM, fp16 engine, S = 112, max_faces 8, fp16 RGB CHW
into a device buffer, matrices to the host.  Four calls are timed in alternation, each in windows of at least --min-seconds after
warm-up, median of three windows:
  ungated       (a) rf_detect_face_batch_device
  gated_null    (b) rf_detect_face_batch_gated_device, gate NULL, records to the host
  gated_half    (c) the same with min_sharpness = the median sharpness tests/face_quality_ref.py computes for those detections
  torch_route   (d) what a caller does today: the u8 face batch (rf_detect_face_batch_device, RF_FACES_U8_HWC) + the same statistic and
                    selection in torch -- luma, Laplacian, integer sums, variance in double, mask, gather, permute, flip, float,
                    sub, mul, half -- then a device synchronise, so that (d) ends where (c) ends.  Its tensor must equal (c)'s.
A separate `rocprofv3 --kernel-trace --stats` run of this file (--trace-child) gives the new kernels' own times.

usage: python tools/face_quality_bench.py [--out profiles/face_quality_bench.json] [--min-seconds 0.5] [--no-trace]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from align_bench import window  # noqa: E402
from face_batch_bench import FaceWorkload  # noqa: E402


class QualityWorkload(FaceWorkload):
    def __init__(self, n, crop, max_faces, batch):
        super().__init__(n, crop, max_faces, batch)
        import retinaface_amd
        torch = self.torch
        self.rfa = retinaface_amd
        self.quality = np.zeros((n, max_faces), retinaface_amd.QUALITY_DTYPE)
        self.quality_p = self.quality.ctypes.data_as(C.POINTER(self._lib.rf_face_quality))
        self.gate = None
        self.threshold = 0.0
        self.spec_u8 = retinaface_amd.face_batch_spec(crop, "u8", False, max_faces=max_faces, capacity=self.capacity)
        self.d_u8 = torch.zeros((self.capacity, crop, crop, 3), dtype=torch.uint8, device="cuda")
        self.offsets_u8 = (C.c_int * (n + 1))()

    def set_gate(self, min_sharpness):
        self.threshold = float(np.float32(min_sharpness))
        self.gate = self.rfa.face_gate(min_sharpness=self.threshold)

    def ungated(self):
        self.batch("f16")

    def gated(self, gate):
        self._lib.check(self.lib.rf_detect_face_batch_gated_device(
            self.h, self.ptrs, self.rows, self.cols, self.steps, self.n, 0.5, self.out, self.cap, self.counts, C.byref(self.specs["f16"]),
            C.c_void_p(self.d_tensor["f16"].data_ptr()), None, self.pmats_p, self.offsets, C.byref(gate) if gate is not None else None,
            self.quality_p), self.h)

    def gated_null(self):
        self.gated(None)

    def gated_half(self):
        self.gated(self.gate)

    def torch_route(self):
        torch = self.torch
        self._lib.check(self.lib.rf_detect_face_batch_device(self.h, self.ptrs, self.rows, self.cols, self.steps, self.n, 0.5, self.out, self.cap,
                                                             self.counts, C.byref(self.spec_u8), C.c_void_p(self.d_u8.data_ptr()), None,
                                                             self.pmats_p, self.offsets_u8), self.h)
        faces = int(self.offsets_u8[self.n])
        u8 = self.d_u8[:faces]
        c = u8.to(torch.int32)
        y = (29 * c[..., 0] + 150 * c[..., 1] + 77 * c[..., 2] + 128) >> 8
        lap = (4 * y[:, 1:-1, 1:-1] - y[:, 1:-1, :-2] - y[:, 1:-1, 2:] - y[:, :-2, 1:-1] - y[:, 2:, 1:-1]).to(torch.int64)
        s1, s2 = lap.sum(dim=(1, 2)), (lap * lap).sum(dim=(1, 2))
        cnt = (self.S - 2) ** 2
        sharp = (cnt * s2 - s1 * s1).to(torch.float64) / (float(cnt) * float(cnt))
        keep = sharp >= self.threshold
        x = u8[keep].permute(0, 3, 1, 2).flip(1).float().sub(127.5).mul(1.0 / 128.0).half()
        torch.cuda.synchronize()
        return x


def reference_median_sharpness(w):
    """the median sharpness tests/face_quality_ref.py gives the faces the ungated call packs"""
    import face_quality_ref as fqr
    from retinaface_amd.frames import synth_frames
    frames = synth_frames(448, 448, w.n, config=1)
    w.ungated()
    faces = np.ctypeslib.as_array(C.cast(w.out, C.POINTER(C.c_float)), shape=(w.n, w.cap, 15))
    rows = [faces[i, :min(w.counts[i], w.cap)].copy() for i in range(w.n)]
    recs = fqr.records(frames, rows, None, size=w.S, max_faces=w.mf)
    sharp = np.concatenate([r["sharpness"] for r in recs])
    return float(np.median(sharp)), recs


def trace_child(args):
    w = QualityWorkload(args.n, args.crop, args.max_faces, args.batch)
    w.set_gate(args.threshold)
    for _ in range(3):
        w.ungated(); w.gated_half()
    for _ in range(20):
        w.gated_half()


def kernel_times_from_trace(args, threshold):
    names = {"face_quality_kernel": "quality", "face_gate_scan_kernel": "gate_scan", "face_batch_kernel": "tensor"}
    durs = {v: [] for v in names.values()}
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "face_quality", "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--n", str(args.n), "--crop", str(args.crop), "--max-faces", str(args.max_faces),
               "--batch", str(args.batch), "--threshold", repr(threshold)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed:\n" + r.stderr[-2000:])
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for frag, key in names.items():
                    if frag in row.get("Kernel_Name", ""):
                        durs[key].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-9)
    if not durs["quality"]:
        raise RuntimeError("no face_quality_kernel dispatch in the kernel trace")
    return {k: (statistics.mean(v), statistics.median(v), len(v)) for k, v in durs.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_quality_bench.json"))
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--crop", type=int, default=112)
    ap.add_argument("--max-faces", type=int, default=8)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--threshold", type=float, default=0.0)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    args = ap.parse_args()
    if args.trace_child:
        return trace_child(args)

    w = QualityWorkload(args.n, args.crop, args.max_faces, args.batch)
    median, recs = reference_median_sharpness(w)
    w.set_gate(median)
    calls = {"ungated": w.ungated, "gated_null": w.gated_null, "gated_half": w.gated_half, "torch_route": w.torch_route}
    for _ in range(5):                          # warm-up: every shape, graph capture, scratch allocation, torch's kernels
        for fn in calls.values():
            fn()
    total = sum(len(r) for r in recs)
    w.gated_null()
    null_ok = int(w.offsets[args.n]) == total and all(
        w.quality[i, :len(r)].tobytes() == r.tobytes() for i, r in enumerate(recs))         # device records = the reference's, bytes
    w.gated_half()
    kept = int(w.offsets[args.n])
    same = bool(w.torch.equal(w.torch_route(), w.d_tensor["f16"][:kept]))
    samples = {k: [] for k in calls}
    for _ in range(3):                          # alternate, so drift hits all alike
        for k, fn in calls.items():
            samples[k].append(window(fn, args.min_seconds))
    med = {k: statistics.median(v) for k, v in samples.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in samples.items()}
    res = {
        "tool": "tools/face_quality_bench.py", "frames": args.n, "net": "448x448", "precision": "fp16", "model": "mnet-deconv-0517",
        "max_batch": args.batch, "crop_size": args.crop, "max_faces": args.max_faces, "faces_considered": total, "faces_kept": kept,
        "min_sharpness": w.threshold, "window_seconds": args.min_seconds, "windows": 3,
        "call_ms": {k: med[k] * 1e3 for k in med},
        "call_ms_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
        "relative_spread": spread,
        "added_over_ungated_ms": {k: (med[k] - med["ungated"]) * 1e3 for k in med if k != "ungated"},
        "null_gate_records_equal_reference": bool(null_ok),
        "torch_route_equals_gated_half": same,
        "gated_half_minus_torch_route_ms": (med["gated_half"] - med["torch_route"]) * 1e3,
    }
    if not args.no_trace:
        # (this process keeps its handle idle meanwhile; the traced child opens its own)
        res["kernels"] = {"source": "rocprofv3 --kernel-trace --stats, separate run"}
        for k, (avg, mid, n_disp) in kernel_times_from_trace(args, w.threshold).items():
            res["kernels"][k] = {"dispatches": n_disp, "avg_us": avg * 1e6, "median_us": mid * 1e6}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
