#!/usr/bin/env python3
"""GPU tool: what antialiased (supersampled) face crops cost next to the plain face batch of the same frames (DESIGN.md
"Antialiased face crops"; writes profiles/face_aa_bench.json).

Two sets, both on the fp16 engine at 448 x 448, S = 112, max_faces 8, fp16 RGB CHW into a device buffer, matrices to the host:
  set A   the 256 seeded 448 x 448 frames of tools/align_bench.py: faces about the size of their crop, almost every k is 1
  set B   32 of those frames enlarged x4 by pixel repetition (1792 x 1792, oversize: the engine shrinks them, the crops are sampled
          at full resolution): faces about four times their crop
Per set three calls are timed in alternation, each in windows of at least --min-seconds after warm-up, median of three windows:
  detect      rf_detect_batch_device
  plain       rf_detect_face_batch_device, antialias = 0
  antialias   rf_detect_face_batch_device, antialias = 1 (aa_max: --aa-max, 0 = the default 4)
and the histogram of the supersampling factor k over the packed faces is recorded (rf_face_aa_factor).  A separate
`rocprofv3 --kernel-trace --stats` run of this file (--trace-child) gives the plain and the antialiased tensor kernel's own times.

usage: python tools/face_aa_bench.py [--out profiles/face_aa_bench.json] [--min-seconds 0.5] [--no-trace]
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

from align_bench import window  # noqa: E402

SETS = {"A": (256, 1), "B": (32, 4)}          # frames, enlargement


class AaWorkload:
    def __init__(self, n, enlarge, crop, max_faces, batch, aa_max):
        import torch
        import retinaface_amd
        from retinaface_amd import _lib
        from retinaface_amd.frames import synth_frames
        assert torch.cuda.is_available(), "this tool measures: it needs the GPU"
        self.torch, self._lib, self.rfa = torch, _lib, retinaface_amd
        self.n, self.S, self.mf, self.aa_max = n, crop, max_faces, aa_max
        side = 448 * enlarge
        small = torch.from_numpy(np.stack(synth_frames(448, 448, n, config=1))).cuda()
        self.frames = small.repeat_interleave(enlarge, dim=1).repeat_interleave(enlarge, dim=2).contiguous()
        torch.cuda.synchronize()
        self.det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", 0.4, precision=retinaface_amd.PRECISION_FP16,
                                             net_hw=(448, 448), model_stem="mnet-deconv-0517", max_batch=batch)
        self.lib, self.h = self.det._lib, self.det._h
        self.cap = self.det.max_detections
        self.scale = self.det.frame_scale(side, side)
        self.ptrs = (C.c_void_p * n)(*[self.frames[i].data_ptr() for i in range(n)])
        self.rows, self.cols = (C.c_int * n)(*[side] * n), (C.c_int * n)(*[side] * n)
        self.steps = (C.c_int * n)(*[side * 3] * n)
        self.out = (_lib.rf_face * (n * self.cap))()
        self.counts = (C.c_int * n)()
        self.capacity = n * max_faces
        self.spec = {aa: retinaface_amd.face_batch_spec(crop, "f16", True, max_faces=max_faces, capacity=self.capacity, antialias=bool(aa),
                                                        aa_max=aa_max) for aa in (0, 1)}
        self.d_tensor = {aa: torch.zeros((self.capacity, 3, crop, crop), dtype=torch.float16, device="cuda") for aa in (0, 1)}
        self.offsets = (C.c_int * (n + 1))()
        self.pmats = np.zeros((self.capacity, 6), np.float64)
        self.pmats_p = self.pmats.ctypes.data_as(C.POINTER(C.c_double))

    def detect(self):
        self._lib.check(self.lib.rf_detect_batch_device(self.h, self.ptrs, self.rows, self.cols, self.steps, self.n, 0.5, self.out, self.cap,
                                                        self.counts), self.h)

    def batch(self, aa):
        self._lib.check(self.lib.rf_detect_face_batch_device(self.h, self.ptrs, self.rows, self.cols, self.steps, self.n, 0.5, self.out, self.cap,
                                                             self.counts, C.byref(self.spec[aa]), C.c_void_p(self.d_tensor[aa].data_ptr()),
                                                             None, self.pmats_p, self.offsets), self.h)

    def plain(self):
        self.batch(0)

    def antialias(self):
        self.batch(1)

    def k_histogram(self):
        """the supersampling factor of every packed face of the most recent call"""
        faces = np.ctypeslib.as_array(C.cast(self.out, C.POINTER(C.c_float)), shape=(self.n, self.cap, 15))
        hist = {}
        for i in range(self.n):
            for f in faces[i, :min(self.counts[i], self.mf, self.cap)]:
                k = self.rfa.face_aa_factor(f, self.scale, self.S, self.aa_max)
                hist[k] = hist.get(k, 0) + 1
        return hist


def trace_child(args):
    n, enlarge = SETS[args.set]
    w = AaWorkload(n, enlarge, args.crop, args.max_faces, args.batch, args.aa_max)
    for _ in range(3):
        w.detect(); w.plain(); w.antialias()
    for _ in range(20):
        w.plain(); w.antialias()


def kernel_times_from_trace(args, name):
    """(mean, median, dispatches) of the durations (s) of the plain and the antialiased fp16 tensor kernel in a rocprofv3 kernel trace"""
    def which(kn):                 # demangled ("face_batch_kernel<_Float16, true, true>") or mangled ("...IDF16_Lb1ELb1EE...") names
        if "face_batch_kernel" not in kn:
            return None
        return "antialias" if ("true, true>" in kn or "Lb1ELb1E" in kn) else "plain"
    durs = {"plain": [], "antialias": []}
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "face_aa", "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--set", name, "--crop", str(args.crop), "--max-faces", str(args.max_faces),
               "--batch", str(args.batch), "--aa-max", str(args.aa_max)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed:\n" + r.stderr[-2000:])
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                k = which(row.get("Kernel_Name", ""))
                if k:
                    durs[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-9)
    if not durs["plain"] or not durs["antialias"]:
        raise RuntimeError("no face_batch_kernel dispatch of both instances in the kernel trace")
    return {k: (statistics.mean(v), statistics.median(v), len(v)) for k, v in durs.items()}


def measure(args, name):
    n, enlarge = SETS[name]
    w = AaWorkload(n, enlarge, args.crop, args.max_faces, args.batch, args.aa_max)
    calls = {"detect": w.detect, "plain": w.plain, "antialias": w.antialias}
    for _ in range(5):                          # warm-up: every shape, graph capture, scratch allocation
        for fn in calls.values():
            fn()
    w.antialias()
    faces = int(w.offsets[n])
    hist = w.k_histogram()
    w.plain()
    differ = not bool(w.torch.equal(w.d_tensor[0][:faces], w.d_tensor[1][:faces]))
    samples = {k: [] for k in calls}
    for _ in range(3):                          # alternate, so drift hits all alike
        for k, fn in calls.items():
            samples[k].append(window(fn, args.min_seconds))
    med = {k: statistics.median(v) for k, v in samples.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in samples.items()}
    mean_k2 = sum(k * k * c for k, c in hist.items()) / max(sum(hist.values()), 1)
    res = {
        "frames": n, "frame_size": f"{448 * enlarge}x{448 * enlarge}", "frame_scale": w.scale, "faces_per_call": faces,
        "k_histogram": {str(k): hist[k] for k in sorted(hist)}, "mean_k_squared": mean_k2,
        "call_ms": {k: med[k] * 1e3 for k in med},
        "call_ms_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
        "relative_spread": spread,
        "added_over_detect_ms": {k: (med[k] - med["detect"]) * 1e3 for k in ("plain", "antialias")},
        "antialias_minus_plain_ms": (med["antialias"] - med["plain"]) * 1e3,
        "antialias_minus_plain_within_the_spread": bool(abs(med["antialias"] - med["plain"]) <=
                                                        max(spread[k] * med[k] for k in ("plain", "antialias"))),
        "antialias_share_of_its_call": (med["antialias"] - med["detect"]) / med["antialias"],
        "tensors_differ": differ,
    }
    w.det.close()
    del w
    if not args.no_trace:
        res["kernels"] = {"source": "rocprofv3 --kernel-trace --stats, separate run"}
        times = kernel_times_from_trace(args, name)
        for k, (avg, mid, n_disp) in times.items():
            res["kernels"][k] = {"dispatches": n_disp, "avg_us": avg * 1e6, "median_us": mid * 1e6}
        res["kernels"]["antialias_over_plain"] = times["antialias"][0] / times["plain"][0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_aa_bench.json"))
    ap.add_argument("--crop", type=int, default=112)
    ap.add_argument("--max-faces", type=int, default=8)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--aa-max", type=int, default=0)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    ap.add_argument("--set", choices=sorted(SETS), default="A")
    args = ap.parse_args()
    if args.trace_child:
        return trace_child(args)
    res = {"tool": "tools/face_aa_bench.py", "net": "448x448", "precision": "fp16", "model": "mnet-deconv-0517", "max_batch": args.batch,
           "crop_size": args.crop, "max_faces": args.max_faces, "aa_max": args.aa_max or 4, "window_seconds": args.min_seconds, "windows": 3,
           "sets": {name: measure(args, name) for name in sorted(SETS)}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
