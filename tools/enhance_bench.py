#!/usr/bin/env python3
"""GPU tool: what low-light detection costs next to what a caller could do without it (DESIGN.md "Low-light detection"; writes
profiles/enhance_bench.json).

Three sets on the fp16 engine (mnet25): eight device-resident 448 x 448 frames (seeded synthetic frames with pasted faces on a photo
background) at gain 0.06, one 1280 x 896 frame (the padded base frame) at gain 0.06, and the eight 448 x 448 frames as they are (lit:
the apply kernel's copy path; two of their 392 tiles are dark).  Per set, three calls are timed in
alternation, each in windows of at least --min-seconds after warm-up, median of three windows with the spread beside it:
  fused       rf_detect_enhanced_batch_device, default spec, the copies in the engine's block
  plain       rf_detect_batch_device on the same (dark) frames, as before
  by_hand     the host path the call replaces: download the frames, rf_enhance_host, upload, one plain call (its result is checked
              against the fused call's bytes)
The two enhance kernels alone come from a rocprofv3 kernel trace of a child process (--trace-child): enhance_lut_kernel and
enhance_apply_kernel of rf_enhance_device over the set, next to rotate_frames_kernel over the same frames in the same run (one
quarter turn each: one launch of the rotation call for the eight frames, rf_rotate_device for the single one).  GB/s are the bytes
the pass has to move (the LUT kernel reads the frames once; the apply kernel reads and writes them) over kernel time, beside the
copy rate DESIGN.md section 4 quotes for this GPU.
--ab-parent-tree DIR: DIR holds a built tree of the parent commit.  The plain call of every set and `bench.py --gpus 1 --steps 2000
--warmup 400` are then run through the parent's tree and this one in alternation, in child processes, and both series are recorded
with the rule: this commit's medians lie within the parent's own runs widened by the larger of their difference and 1 %.
No speed-up is promised: the file records what was measured.

usage: python tools/enhance_bench.py [--out profiles/enhance_bench.json] [--min-seconds 0.5] [--no-trace] [--ab-parent-tree DIR]
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
TREE = ROOT
if "--tree" in sys.argv:                        # a child of the A/B: the package (and its library) of another tree
    TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

NMS = 0.4
SETS = {"8x448x448": (8, 448, 448, 0.06), "1x1280x896": (1, 896, 1280, 0.06), "8x448x448_lit": (8, 448, 448, 1.0)}       # frames, rows, cols, gain
TRACE_WARM, TRACE_CALLS = 3, 20
COPY_PEAK_TBPS = 6.3                            # "the measured copy rate is 6.3" TB/s


def window(fn, min_seconds):
    t0 = time.perf_counter()
    calls = 0
    while True:
        fn()                      # every call is synchronous: it returns after its device work has finished
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / calls


def dark_frames(name):
    from retinaface_amd.frames import padded_base_frame, synth_frames
    n, rows, cols, gain = SETS[name]
    src = synth_frames(rows, cols, n, config=700, faces=[1, 3, 5], background="photo") if n > 1 else [padded_base_frame()]
    return [np.clip(np.rint(f.astype(np.float64) * gain), 0, 255).astype(np.uint8) for f in src]


class Workload:
    """one set on one engine; only `plain` is used when the tree is another commit's"""
    def __init__(self, name, batch):
        import torch
        import retinaface_amd
        from retinaface_amd import _lib
        assert torch.cuda.is_available(), "this tool measures: it needs the GPU"
        self.torch, self._lib, self.rfa = torch, _lib, retinaface_amd
        n, rows, cols, self.gain = SETS[name]
        self.n, self.rows, self.cols = n, rows, cols
        self.host = dark_frames(name)
        self.frames = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in self.host]
        self.copies = [torch.zeros_like(f) for f in self.frames]
        torch.cuda.synchronize()
        self.det = retinaface_amd.RetinaFace(os.path.join(TREE, "assets"), "net3", NMS, precision=retinaface_amd.PRECISION_FP16,
                                             net_hw=(rows, cols), model_stem="mnet25", max_batch=batch)
        self.lib, self.h = self.det._lib, self.det._h
        self.cap = self.det.max_detections
        self.ptrs = (C.c_void_p * n)(*[f.data_ptr() for f in self.frames])
        self.cptrs = (C.c_void_p * n)(*[f.data_ptr() for f in self.copies])
        self.r, self.c, self.s = (C.c_int * n)(*[rows] * n), (C.c_int * n)(*[cols] * n), (C.c_int * n)(*[3 * cols] * n)
        self.out = (_lib.rf_face * (n * self.cap))()
        self.counts, self.tiles = (C.c_int * n)(), (C.c_int * n)()
        self.hand = None

    def plain(self, ptrs=None):
        self._lib.check(self.lib.rf_detect_batch_device(self.h, ptrs or self.ptrs, self.r, self.c, self.s, self.n, 0.5, self.out, self.cap,
                                                        self.counts), self.h)

    def fused(self):
        self._lib.check(self.lib.rf_detect_enhanced_batch_device(self.h, self.ptrs, self.r, self.c, self.s, self.n, 0.5, None, self.out, self.cap,
                                                                 self.counts, None, None, self.tiles), self.h)

    def enhance(self):
        self._lib.check(self.lib.rf_enhance_device(self.h, None, self.ptrs, self.r, self.c, self.s, self.n, self.cptrs, self.s, self.tiles), self.h)

    def rotate(self):
        """rotate_frames_kernel over the same frames, one launch: a quarter turn of each"""
        if self.n > 1:
            self.det.detect_rotated_device([f.data_ptr() for f in self.frames], [self.rows] * self.n, [self.cols] * self.n, 0.5, rots=2)
        else:
            self.det.rotate_device(self.frames[0].data_ptr(), self.rows, self.cols, 1, self.copies[0].data_ptr())

    def by_hand(self):
        torch = self.torch
        host = [f.cpu().numpy() for f in self.frames]                                   # download
        up = [torch.from_numpy(self.rfa.enhance_host(f)[0]).cuda() for f in host]        # enhance on the host, upload
        torch.cuda.synchronize()
        self.plain((C.c_void_p * self.n)(*[u.data_ptr() for u in up]))
        self.hand = self.faces()

    def faces(self):
        a = np.ctypeslib.as_array(C.cast(self.out, C.POINTER(C.c_float)), shape=(self.n, self.cap, 15))
        return [a[i, :min(self.counts[i], self.cap)].copy() for i in range(self.n)]


def stats(samples):
    med = statistics.median(samples)
    return {"ms": med * 1e3, "samples_ms": [x * 1e3 for x in samples], "relative_spread": (max(samples) - min(samples)) / med}


def measure(name, args):
    w = Workload(name, args.batch)
    calls = {"fused": w.fused, "plain": w.plain, "by_hand": w.by_hand}
    for _ in range(3):                          # warm-up: every launch size, graph capture, scratch allocation
        for fn in calls.values():
            fn()
    w.plain()
    found = {"plain": [int(w.counts[i]) for i in range(w.n)]}
    w.fused()
    fused = w.faces()
    found["fused"] = [int(w.counts[i]) for i in range(w.n)]
    tiles = [int(w.tiles[i]) for i in range(w.n)]
    w.by_hand()
    same = all(a.tobytes() == b.tobytes() for a, b in zip(fused, w.hand))
    samples = {k: [] for k in calls}
    for _ in range(3):                          # alternate, so drift hits all alike
        for k, fn in calls.items():
            samples[k].append(window(fn, args.min_seconds))
    res = {"frames": w.n, "frame_size": f"{w.cols}x{w.rows}", "gain": w.gain, "faces_per_frame": found, "tiles_enhanced": tiles,
           "fused_equals_by_hand": bool(same), "call": {k: stats(v) for k, v in samples.items()}}
    med = {k: res["call"][k]["ms"] for k in calls}
    res["fused_minus_plain_ms"] = med["fused"] - med["plain"]
    res["fused_over_plain"] = med["fused"] / med["plain"]
    res["by_hand_over_fused"] = med["by_hand"] / med["fused"]
    w.det.close()
    return res


def trace_child(args):
    """per set: TRACE_WARM + TRACE_CALLS rf_enhance_device calls (one LUT and one apply launch each), then as many rotate launches"""
    for name in SETS:
        w = Workload(name, args.batch)
        for _ in range(TRACE_WARM + TRACE_CALLS):
            w.enhance()
        for _ in range(TRACE_WARM + TRACE_CALLS):
            w.rotate()
        w.det.close()


def kernel_times_from_trace(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "enh", "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--batch", str(args.batch)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed:\n" + r.stderr[-2000:])
        got = {"enhance_lut_kernel": [], "enhance_apply_kernel": [], "rotate_frames_kernel": []}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for key in got:
                    if key in row.get("Kernel_Name", ""):
                        got[key].append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-9))
    per = TRACE_WARM + TRACE_CALLS
    got = {k: [d for _, d in sorted(v)] for k, v in got.items()}
    if any(len(v) != per * len(SETS) for v in got.values()):
        raise RuntimeError("unexpected dispatch counts in the kernel trace: " + str({k: len(v) for k, v in got.items()}))
    us = lambda v: {"median_us": statistics.median(v) * 1e6, "min_us": min(v) * 1e6, "max_us": max(v) * 1e6, "dispatches": len(v)}  # noqa: E731
    res = {}
    for i, (name, (n, rows, cols, _)) in enumerate(SETS.items()):
        part = {k: v[i * per + TRACE_WARM:(i + 1) * per] for k, v in got.items()}
        frame_bytes = n * rows * cols * 3
        lut, app, rot = (statistics.median(part[k]) for k in ("enhance_lut_kernel", "enhance_apply_kernel", "rotate_frames_kernel"))
        res[name] = {"enhance_lut_kernel": us(part["enhance_lut_kernel"]), "enhance_apply_kernel": us(part["enhance_apply_kernel"]),
                     "rotate_frames_kernel_quarter_turn": us(part["rotate_frames_kernel"]), "frame_bytes": frame_bytes,
                     "lut_GBps_read": frame_bytes / lut * 1e-9, "apply_GBps_read_plus_written": 2 * frame_bytes / app * 1e-9,
                     "rotate_GBps_read_plus_written": 2 * frame_bytes / rot * 1e-9,
                     "both_enhance_kernels_us": (lut + app) * 1e6, "both_over_rotate": (lut + app) / rot,
                     "copy_peak_GBps": COPY_PEAK_TBPS * 1e3,
                     "lut_share_of_copy_peak": frame_bytes / lut * 1e-12 / COPY_PEAK_TBPS,
                     "apply_share_of_copy_peak": 2 * frame_bytes / app * 1e-12 / COPY_PEAK_TBPS}
    return res


def plain_child(args):
    """the plain call of every set through the tree named by --tree: one JSON line"""
    res = {}
    for name in SETS:
        w = Workload(name, args.batch)
        for _ in range(10):
            w.plain()
        res[name] = [window(w.plain, args.min_seconds) * 1e3 for _ in range(3)]
        w.det.close()
    print("PLAIN " + json.dumps(res))


def within(parent, this):
    """the rule: every figure of this commit inside the parent's own runs widened by the larger of their difference and 1 %"""
    a = max((max(parent) - min(parent)) / statistics.mean(parent), 0.01)
    return bool(min(parent) * (1 - a) <= min(this) and max(this) <= max(parent) * (1 + a)), a


def ab(args):
    trees = {"parent": os.path.abspath(args.ab_parent_tree), "this": ROOT}
    order = ["parent", "this", "parent", "this"]
    plain = {k: {name: [] for name in SETS} for k in trees}
    for who in order:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-child", "--tree", trees[who], "--batch", str(args.batch),
                            "--min-seconds", str(args.min_seconds)], capture_output=True, text=True, timeout=600, cwd=trees[who])
        if r.returncode != 0:
            raise RuntimeError(who + ": plain child failed:\n" + r.stderr[-2000:])
        line = [x for x in r.stdout.splitlines() if x.startswith("PLAIN ")][-1]
        for name, v in json.loads(line[6:]).items():
            plain[who][name].append(statistics.median(v))
    bench = {k: [] for k in trees}
    for who in ["parent", "this"] * 3:
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2000", "--warmup", "400"], capture_output=True, text=True,
                           timeout=900, cwd=trees[who])
        if r.returncode != 0:
            raise RuntimeError(who + ": bench.py failed:\n" + r.stderr[-2000:])
        line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
        bench[who].append(json.loads(line)["value"])
    res = {"what": "the plain call (rf_detect_batch_device, median ms of three windows per run) and bench.py --gpus 1 --steps 2000 --warmup 400 "
                   "(faces/s), the parent commit's tree and this commit's in alternation in one job.  The rule: this commit's medians lie within "
                   "[min(parent) x (1 - a), max(parent) x (1 + a)], a = max(the parent runs' relative difference, 1 %).",
           "order_plain": order, "order_bench": ["parent", "this"] * 3, "plain_call_ms": plain, "bench_faces_per_s": bench, "within": {}}
    for name in SETS:
        ok, a = within(plain["parent"][name], plain["this"][name])
        res["within"]["plain " + name] = {"ok": ok, "allowed": a}
    ok, a = within(bench["parent"], bench["this"])
    res["within"]["bench.py"] = {"ok": ok, "allowed": a}
    res["all_within"] = all(v["ok"] for v in res["within"].values())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enhance_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    ap.add_argument("--plain-child", action="store_true")
    ap.add_argument("--tree", default=None, help="(children of the A/B) the tree whose package and library are measured")
    ap.add_argument("--ab-parent-tree", default=None, help="a built tree of the parent commit: the plain call and bench.py are run through it "
                    "and through this tree in alternation")
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args)
        return
    if args.plain_child:
        plain_child(args)
        return
    res = {"tool": "tools/enhance_bench.py", "precision": "fp16", "model": "mnet25", "max_batch": args.batch, "window_seconds": args.min_seconds,
           "windows": 3, "spec": "defaults: tile 64, clip 2048, dark_below 64", "sets": {name: measure(name, args) for name in SETS}}
    if not args.no_trace:
        res["kernels"] = kernel_times_from_trace(args)
    if args.ab_parent_tree:
        res["parent_ab"] = ab(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
