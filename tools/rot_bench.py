#!/usr/bin/env python3
"""GPU tool: what rotation-robust detection costs and finds next to what a caller could do without it (DESIGN.md "Rotation-robust
detection"; writes profiles/rot_bench.json).

Eight device-resident 448 x 448 frames (seeded synthetic frames with pasted faces) on the fp16 engine (mnet25).  Five calls are timed
in alternation, each in windows of at least --min-seconds after warm-up, median of three windows with the spread beside it:
  rot         (a) rf_detect_rot_batch_device, all four rotations
  plain       (b) rf_detect_batch_device on the frames, as before
  passes      (c) rf_detect_batch_device on the 32 frames [f0, rot1(f0), rot2(f0), rot3(f0), f1, ...] with the rotations made
              BEFOREHAND: the floor under any caller -- the fused call adds the rotate, gather and merge launches to it
  by_hand     (d) the host path the call replaces: download the frames, np.rot90 three times each, upload, one plain call over the 32,
              the merge of tests/rot_ref.py on the host (its result is checked against the fused call's bytes)
  tta         the flip-TTA call, for (f): `plain` and `tta` beside the same two numbers of another build's tools/tta_bench.py
              (--other-tta-bench FILE, e.g. the parent commit's)
(e) the rotate launches alone come from a rocprofv3 kernel trace of a child process (--trace-child): the rotate_frames_kernel
dispatches of a call with all 24 rotations (two launches: 16 + 8), of a call with the 16 transposes only (rots = 10), of a call with the 8
half turns only (rots = 4), and mirror_rows_kernel over the same 8 frames (the TTA call's launch; x 3 for the same bytes).
The detection counts of the claim (the window (0, 832) of the base frame turned four ways, threshold 0.6) are recorded too.
No speed-up is promised: the file records what was measured.

usage: python tools/rot_bench.py [--out profiles/rot_bench.json] [--min-seconds 0.5] [--no-trace] [--other-tta-bench FILE]
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

NET, NMS, N = 448, 0.4, 8
TRACE_WARM, TRACE_CALLS = 3, 20


class RotWorkload:
    def __init__(self, batch):
        import torch
        import retinaface_amd
        import rot_ref
        from retinaface_amd import _lib
        from retinaface_amd.frames import synth_frames
        assert torch.cuda.is_available(), "this tool measures: it needs the GPU"
        self.torch, self._lib, self.rr, self.rfa = torch, _lib, rot_ref, retinaface_amd
        n = self.n = N
        self.host = synth_frames(NET, NET, n, config=1)
        self.frames = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in self.host]
        self.copies = [torch.from_numpy(rot_ref.rotate(f, k)).cuda() for f in self.host for k in (1, 2, 3)]
        torch.cuda.synchronize()
        self.det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", NMS, precision=retinaface_amd.PRECISION_FP16,
                                             net_hw=(NET, NET), model_stem="mnet25", max_batch=batch)
        self.lib, self.h = self.det._lib, self.det._h
        self.cap = self.det.max_detections
        self.spec = retinaface_amd.rot_spec()
        self.tta_spec = retinaface_amd.tta_spec()
        self.ptrs = (C.c_void_p * n)(*[f.data_ptr() for f in self.frames])
        self.r, self.c, self.s = (C.c_int * n)(*[NET] * n), (C.c_int * n)(*[NET] * n), (C.c_int * n)(*[3 * NET] * n)
        self.out = (_lib.rf_face * (n * self.cap))()
        self.counts, self.frame_rot = (C.c_int * n)(), (C.c_int * n)()
        self.score = (C.c_float * (4 * n))()
        self.votes, self.src = (C.c_int * (n * self.cap))(), (C.c_int * (n * self.cap))()
        self.pr, self.pc, self.ps = (C.c_int * (4 * n))(*[NET] * (4 * n)), (C.c_int * (4 * n))(*[NET] * (4 * n)), (C.c_int * (4 * n))(*[3 * NET] * (4 * n))
        self.pptrs = self.pass_ptrs(self.frames, self.copies)
        self.pout = (_lib.rf_face * (4 * n * self.cap))()
        self.pcounts = (C.c_int * (4 * n))()
        self.hand = None

    def pass_ptrs(self, frames, copies):
        ptrs = []
        for i, f in enumerate(frames):
            ptrs += [f.data_ptr()] + [copies[3 * i + j].data_ptr() for j in range(3)]
        return (C.c_void_p * (4 * self.n))(*ptrs)

    def rot(self, spec=None):
        self._lib.check(self.lib.rf_detect_rot_batch_device(self.h, self.ptrs, self.r, self.c, self.s, self.n, 0.5, C.byref(spec or self.spec),
                                                            self.out, self.cap, self.counts, self.votes, self.src, self.frame_rot, self.score), self.h)

    def tta(self):
        self._lib.check(self.lib.rf_detect_tta_batch_device(self.h, self.ptrs, self.r, self.c, self.s, self.n, 0.5, C.byref(self.tta_spec),
                                                            self.out, self.cap, self.counts, self.votes, self.src), self.h)

    def plain(self):
        self._lib.check(self.lib.rf_detect_batch_device(self.h, self.ptrs, self.r, self.c, self.s, self.n, 0.5, self.out, self.cap,
                                                        self.counts), self.h)

    def passes(self, pptrs=None):
        self._lib.check(self.lib.rf_detect_batch_device(self.h, pptrs or self.pptrs, self.pr, self.pc, self.ps, 4 * self.n, 0.5, self.pout,
                                                        self.cap, self.pcounts), self.h)

    def by_hand(self):
        n, cap, rr, torch = self.n, self.cap, self.rr, self.torch
        host = [f.cpu().numpy() for f in self.frames]                                   # download
        copies = [torch.from_numpy(rr.rotate(f, k)).cuda() for f in host for k in (1, 2, 3)]          # np.rot90 three times, upload
        torch.cuda.synchronize()
        self.passes(self.pass_ptrs(self.frames, copies))
        faces = np.ctypeslib.as_array(C.cast(self.pout, C.POINTER(C.c_float)), shape=(n, 4, cap, 15))
        res = []
        for i in range(n):
            per = [faces[i, k, :min(self.pcounts[4 * i + k], cap)].copy() for k in range(4)]
            res.append(rr.merge(NET, NET, per, NET, NET, NMS, cap)[0])
        self.hand = res

    def rot_faces(self):
        a = np.ctypeslib.as_array(C.cast(self.out, C.POINTER(C.c_float)), shape=(self.n, self.cap, 15))
        return [a[i, :min(self.counts[i], self.cap)].copy() for i in range(self.n)]


def measure(args):
    w = RotWorkload(args.batch)
    n = w.n
    calls = {"rot": w.rot, "plain": w.plain, "passes": w.passes, "by_hand": w.by_hand, "tta": w.tta}
    for _ in range(3):                          # warm-up: every launch size, graph capture, scratch allocation
        for fn in calls.values():
            fn()
    w.plain()
    found = {"plain": [int(w.counts[i]) for i in range(n)]}
    w.rot()
    rot = w.rot_faces()
    found["rot"] = [int(w.counts[i]) for i in range(n)]
    frame_rot = [int(w.frame_rot[i]) for i in range(n)]
    w.by_hand()
    found["by_hand"] = [len(f) for f in w.hand]
    same = all(a.tobytes() == b.tobytes() for a, b in zip(rot, w.hand))
    samples = {k: [] for k in calls}
    for _ in range(3):                          # alternate, so drift hits all alike
        for k, fn in calls.items():
            samples[k].append(window(fn, args.min_seconds))
    med = {k: statistics.median(v) for k, v in samples.items()}
    res = {
        "frames": n, "frame_size": f"{NET}x{NET}", "faces_per_frame": found, "frame_rot": frame_rot, "rot_equals_by_hand": bool(same),
        "call_ms": {k: med[k] * 1e3 for k in med},
        "call_ms_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
        "relative_spread": {k: (max(v) - min(v)) / med[k] for k, v in samples.items()},
        "rot_over_plain": med["rot"] / med["plain"],
        "passes_over_rot": med["passes"] / med["rot"],
        "by_hand_over_rot": med["by_hand"] / med["rot"],
    }
    w.det.close()
    return res


def claim():
    """the window (0, 832) of the base frame turned by kf = 0..3, threshold 0.6: what the rotation call and the plain call find"""
    import torch
    import retinaface_amd
    import rot_ref
    from retinaface_amd.frames import padded_base_frame
    det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", NMS, precision=retinaface_amd.PRECISION_FP16, net_hw=(NET, NET),
                                    model_stem="mnet25")
    frames = [rot_ref.rotate(padded_base_frame()[0:448, 832:1280], kf) for kf in range(4)]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()
    ptrs = [d.data_ptr() for d in dev]
    got, votes, src = det.detect_rotated_device(ptrs, [NET] * 4, [NET] * 4, 0.6, return_votes=True)
    plain = det.detect_device(ptrs, [NET] * 4, [NET] * 4, 0.6)
    res = {"window": [0, 832], "threshold": 0.6, "frame_turned_by": [0, 1, 2, 3],
           "rot_faces": [len(g) for g in got], "rot_scores": [[round(d.score, 4) for d in g] for g in got],
           "src_rot": [[int(s) for s in v] for v in src], "frame_rot": list(det.frame_rot),
           "plain_faces": [len(p) for p in plain], "plain_scores": [[round(d.score, 4) for d in p] for p in plain]}
    det.close()
    return res


def trace_child(args):
    """four phases of TRACE_WARM + TRACE_CALLS calls each, in this order: all 24 rotations (two rotate launches per call), the 16
    transposes (one), the 8 half turns (one), the TTA call (one mirror launch)"""
    w = RotWorkload(args.batch)
    for rots in (15, 10, 4):
        sp = w.rfa.rot_spec(rots)
        for _ in range(TRACE_WARM + TRACE_CALLS):
            w.rot(sp)
    for _ in range(TRACE_WARM + TRACE_CALLS):
        w.tta()
    w.det.close()


def kernel_times_from_trace(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "rot", "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--batch", str(args.batch)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed:\n" + r.stderr[-2000:])
        rot, mir = [], []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Kernel_Name", "")
                rec = (int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-9)
                if "rotate_frames_kernel" in name:
                    rot.append(rec)
                elif "mirror_rows_kernel" in name:
                    mir.append(rec)
    rot = [d for _, d in sorted(rot)]
    mir = [d for _, d in sorted(mir)]
    per = TRACE_WARM + TRACE_CALLS
    if len(rot) != 4 * per or len(mir) != per:
        raise RuntimeError(f"unexpected dispatch counts in the kernel trace: rotate {len(rot)}, mirror {len(mir)}")
    all24 = [rot[2 * i] + rot[2 * i + 1] for i in range(TRACE_WARM, per)]
    t16 = rot[2 * per + TRACE_WARM:3 * per]
    h8 = rot[3 * per + TRACE_WARM:4 * per]
    m8 = mir[TRACE_WARM:]
    us = lambda v: {"median_us": statistics.median(v) * 1e6, "min_us": min(v) * 1e6, "max_us": max(v) * 1e6, "dispatch_groups": len(v)}  # noqa: E731
    frame_bytes = 2 * NET * NET * 3                                            # read + written per frame-rotation
    res = {"rotate_24_rotations_two_launches": us(all24), "rotate_16_transposes_one_launch": us(t16), "rotate_8_half_turns_one_launch": us(h8),
           "mirror_8_frames_one_launch": us(m8), "bytes_moved_per_frame_rotation": frame_bytes}
    m = statistics.median(m8)
    res["mirror_x3_us"] = 3 * m * 1e6
    res["rotate24_over_mirror_x3"] = statistics.median(all24) / (3 * m)
    res["transpose_per_frame_over_mirror_per_frame"] = (statistics.median(t16) / 16) / (m / 8)
    res["half_turn_per_frame_over_mirror_per_frame"] = (statistics.median(h8) / 8) / (m / 8)
    res["transpose_GBps"] = 16 * frame_bytes / statistics.median(t16) * 1e-9
    res["mirror_GBps"] = 8 * frame_bytes / m * 1e-9
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rot_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    ap.add_argument("--other-tta-bench", default=None, help="the JSON another build's tools/tta_bench.py wrote (e.g. the parent commit's): its "
                    "plain and TTA call times at 448x448 are recorded beside this build's")
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args)
        return
    res = {"tool": "tools/rot_bench.py", "net": "448x448", "precision": "fp16", "model": "mnet25", "max_batch": args.batch,
           "window_seconds": args.min_seconds, "windows": 3, "calls": measure(args), "claim": claim()}
    if not args.no_trace:
        res["rotate_launch"] = kernel_times_from_trace(args)
    if args.other_tta_bench:
        other = json.load(open(args.other_tta_bench))["sets"]["448x448"]
        res["other_build"] = {"source": "tools/tta_bench.py of the other build, set 448x448 (the same frames and engine options)",
                              "call_ms": {k: other["call_ms"][k] for k in ("plain", "tta")},
                              "relative_spread": {k: other["relative_spread"][k] for k in ("plain", "tta")},
                              "this_over_other": {k: res["calls"]["call_ms"][k] / other["call_ms"][k] for k in ("plain", "tta")}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
