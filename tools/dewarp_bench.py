#!/usr/bin/env python3
"""GPU tool: what fisheye detection costs and finds next to what a caller could do without it (DESIGN.md "Fisheye detection"; writes
profiles/dewarp_bench.json).

Eight device-resident 1024 x 1024 equidistant fisheye frames (the poster scene of tests/test_dewarp_host.py, turned and mirrored) with a
ring of 4 views of 448 x 448 on the fp16 engine (mnet25).  Four calls are timed in alternation, each in windows of at least
--min-seconds after warm-up, median of three windows with the spread beside it:
  dewarp      (a) rf_detect_dewarp_batch_device
  plain       (b) rf_detect_batch_device on the eight frames, shrunk to the net as always: what a caller without the call gets
  views       (c) rf_detect_batch_device on the 32 views made BEFOREHAND: the floor under any caller -- the fused call adds the dewarp,
              gather and merge launches to it and will not beat it; `dewarp_over_views` says by how much it misses
  by_hand     (d) the host path the call replaces: download the frames, numpy remap (tests/dewarp_ref.py), upload, one plain call over
              the 32 views, the merge of tests/dewarp_ref.py on the host (its result is checked against the fused call's bytes)
(e) the dewarp launches alone come from a rocprofv3 kernel trace of a child process (--trace-child): the dewarp_views_kernel dispatches
of the fused call (32 views: two launches of 16), next to the rotate_frames_kernel dispatches of a rotation call that makes 32
rotations of 448 x 448 frames (16 frames, rots = 6: a transpose and a half turn each, two launches of 16): the same output bytes.
The detection counts of the claim (threshold 0.6) are recorded too.  No speed-up is promised: the file records what was measured.

usage: python tools/dewarp_bench.py [--out profiles/dewarp_bench.json] [--min-seconds 0.5] [--no-trace]
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

NET, NMS, N, V, SIZE = 448, 0.4, 8, 4, 1024
F = 0.98 * SIZE / np.pi
POSTERS = ((30, 440), (30, 0), (200, 300), (0, 832))
TRACE_WARM, TRACE_CALLS = 3, 20


def scenes():
    """the scene of the claim and seven more made from it by turning and mirroring"""
    import dewarp_ref as dr
    from retinaface_amd.frames import padded_base_frame
    base = padded_base_frame()
    posters = [np.ascontiguousarray(base[y:y + NET, x:x + NET]) for y, x in POSTERS]
    s = dr.poster_scene(posters, SIZE, F, dr.ring(V, 55.0, 60.0), NET, NET)
    m = s[:, ::-1]
    return [np.ascontiguousarray(f) for f in (s, np.rot90(s, 1), m, np.rot90(s, 2), s[::-1], np.rot90(s, 3), np.rot90(m, 1), np.rot90(m, 3))], posters


class DewarpWorkload:
    def __init__(self, batch):
        import torch
        import retinaface_amd
        import dewarp_ref
        from retinaface_amd import _lib
        assert torch.cuda.is_available(), "this tool measures: it needs the GPU"
        self.torch, self._lib, self.dr, self.rfa = torch, _lib, dewarp_ref, retinaface_amd
        n = self.n = N
        self.host, self.posters = scenes()
        self.frames = [torch.from_numpy(f).cuda() for f in self.host]
        self.det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", NMS, precision=retinaface_amd.PRECISION_FP16,
                                             net_hw=(NET, NET), model_stem="mnet25", max_batch=batch)
        self.lib, self.h = self.det._lib, self.det._h
        self.cap = self.det.max_detections
        self.spec = retinaface_amd.dewarp_spec(f=F, cx=(SIZE - 1) / 2, cy=(SIZE - 1) / 2, ring=V, pitch=55.0, hfov=60.0)
        self.dw = self.det.dewarper(SIZE, SIZE, spec=self.spec)
        self.mesh = self.dw.mesh
        self.copies = [torch.from_numpy(dewarp_ref.warp(f, m, NET, NET)).cuda() for f in self.host for m in self.mesh]
        torch.cuda.synchronize()
        self.ptrs = (C.c_void_p * n)(*[f.data_ptr() for f in self.frames])
        self.r, self.c, self.s = (C.c_int * n)(*[SIZE] * n), (C.c_int * n)(*[SIZE] * n), (C.c_int * n)(*[3 * SIZE] * n)
        self.out = (_lib.rf_face * (n * self.cap))()
        self.counts = (C.c_int * n)()
        self.votes, self.src = (C.c_int * (n * self.cap))(), (C.c_int * (n * self.cap))()
        p = V * n
        self.pr, self.pc, self.ps = (C.c_int * p)(*[NET] * p), (C.c_int * p)(*[NET] * p), (C.c_int * p)(*[3 * NET] * p)
        self.pptrs = (C.c_void_p * p)(*[t.data_ptr() for t in self.copies])
        self.pout = (_lib.rf_face * (p * self.cap))()
        self.pcounts = (C.c_int * p)()
        self.hand = None
        # the rotate kernel over the same output bytes: 16 frames of 448 x 448, two rotations each
        self.small = [torch.from_numpy(np.ascontiguousarray(f[100:100 + NET, 300:300 + NET])).cuda() for f in self.host for _ in range(2)]
        self.sptrs = [t.data_ptr() for t in self.small]

    def dewarp(self):
        self._lib.check(self.lib.rf_detect_dewarp_batch_device(self.dw._d, self.ptrs, self.r, self.c, self.s, self.n, 0.5, C.byref(self.spec),
                                                               self.out, self.cap, self.counts, self.votes, self.src, None), self.h)

    def plain(self):
        self._lib.check(self.lib.rf_detect_batch_device(self.h, self.ptrs, self.r, self.c, self.s, self.n, 0.5, self.out, self.cap,
                                                        self.counts), self.h)

    def views(self, pptrs=None):
        self._lib.check(self.lib.rf_detect_batch_device(self.h, pptrs or self.pptrs, self.pr, self.pc, self.ps, V * self.n, 0.5, self.pout,
                                                        self.cap, self.pcounts), self.h)

    def by_hand(self):
        n, cap, dr, torch = self.n, self.cap, self.dr, self.torch
        host = [f.cpu().numpy() for f in self.frames]                                                   # download
        copies = [torch.from_numpy(dr.warp(f, m, NET, NET)).cuda() for f in host for m in self.mesh]    # numpy remap, upload
        torch.cuda.synchronize()
        self.views((C.c_void_p * (V * n))(*[t.data_ptr() for t in copies]))
        faces = np.ctypeslib.as_array(C.cast(self.pout, C.POINTER(C.c_float)), shape=(n, V, cap, 15))
        res = []
        for i in range(n):
            per = [faces[i, v, :min(self.pcounts[V * i + v], cap)].copy() for v in range(V)]
            res.append(dr.merge(self.mesh, NET, NET, per, NET, NET, NMS, cap)[0])
        self.hand = res

    def rot32(self):
        self.det.detect_rotated_device(self.sptrs, [NET] * 16, [NET] * 16, 0.5, rots=6)

    def dewarp_faces(self):
        a = np.ctypeslib.as_array(C.cast(self.out, C.POINTER(C.c_float)), shape=(self.n, self.cap, 15))
        return [a[i, :min(self.counts[i], self.cap)].copy() for i in range(self.n)]


def measure(args):
    w = DewarpWorkload(args.batch)
    n = w.n
    calls = {"dewarp": w.dewarp, "plain": w.plain, "views": w.views, "by_hand": w.by_hand}
    for _ in range(3):                          # warm-up: every launch size, graph capture, scratch allocation
        for k, fn in calls.items():
            fn()
    w.plain()
    found = {"plain": [int(w.counts[i]) for i in range(n)]}
    w.dewarp()
    got = w.dewarp_faces()
    found["dewarp"] = [int(w.counts[i]) for i in range(n)]
    w.by_hand()
    found["by_hand"] = [len(f) for f in w.hand]
    same = all(a.tobytes() == b.tobytes() for a, b in zip(got, w.hand))
    samples = {k: [] for k in calls}
    for _ in range(3):                          # alternate, so drift hits all alike
        for k, fn in calls.items():
            samples[k].append(window(fn, args.min_seconds))
    med = {k: statistics.median(v) for k, v in samples.items()}
    res = {
        "frames": n, "frame_size": f"{SIZE}x{SIZE}", "views": V, "view_size": f"{NET}x{NET}", "faces_per_frame": found,
        "dewarp_equals_by_hand": bool(same),
        "call_ms": {k: med[k] * 1e3 for k in med},
        "call_ms_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
        "relative_spread": {k: (max(v) - min(v)) / med[k] for k, v in samples.items()},
        "dewarp_over_plain": med["dewarp"] / med["plain"],
        "dewarp_over_views": med["dewarp"] / med["views"],
        "dewarp_minus_views_ms": (med["dewarp"] - med["views"]) * 1e3,
        "by_hand_over_dewarp": med["by_hand"] / med["dewarp"],
    }
    # the claim: threshold 0.6, the scene itself and its posters
    det, torch = w.det, w.torch
    dev = [torch.from_numpy(p).cuda() for p in w.posters]
    torch.cuda.synchronize()
    faces, votes, src = det.detect_dewarped_device([w.frames[0].data_ptr()], w.dw, 0.6, return_votes=True)
    plain = det.detect_device([w.frames[0].data_ptr()], [SIZE], [SIZE], 0.6)
    posters = det.detect_device([d.data_ptr() for d in dev], [NET] * V, [NET] * V, 0.6)
    res_claim = {"posters": [list(p) for p in POSTERS], "threshold": 0.6, "dewarp_faces": len(faces[0]),
                 "dewarp_scores": [round(d.score, 4) for d in faces[0]], "src_view": [int(s) for s in src[0]],
                 "faces_on_the_posters_themselves": [len(p) for p in posters], "plain_faces": len(plain[0]),
                 "plain_scores": [round(d.score, 4) for d in plain[0]]}
    w.det.close()
    return res, res_claim


def trace_child(args):
    """two phases of TRACE_WARM + TRACE_CALLS calls each: the fused call (two dewarp launches of 16 views per call), the rotation call
    over 16 frames with rots = 6 (two rotate launches of 16 rotations per call)"""
    w = DewarpWorkload(args.batch)
    for _ in range(TRACE_WARM + TRACE_CALLS):
        w.dewarp()
    for _ in range(TRACE_WARM + TRACE_CALLS):
        w.rot32()
    w.det.close()


def kernel_times_from_trace(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "dewarp", "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--batch", str(args.batch)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed:\n" + r.stderr[-2000:])
        dew, rot = [], []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Kernel_Name", "")
                rec = (int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-9)
                if "dewarp_views" in name:
                    dew.append(rec)
                elif "rotate_frames_kernel" in name:
                    rot.append(rec)
    dew = [d for _, d in sorted(dew)]
    rot = [d for _, d in sorted(rot)]
    per = TRACE_WARM + TRACE_CALLS
    if len(dew) != 2 * per or len(rot) != 2 * per:
        raise RuntimeError(f"unexpected dispatch counts in the kernel trace: dewarp {len(dew)}, rotate {len(rot)}")
    d32 = [dew[2 * i] + dew[2 * i + 1] for i in range(TRACE_WARM, per)]
    r32 = [rot[2 * i] + rot[2 * i + 1] for i in range(TRACE_WARM, per)]
    us = lambda v: {"median_us": statistics.median(v) * 1e6, "min_us": min(v) * 1e6, "max_us": max(v) * 1e6, "dispatch_groups": len(v)}  # noqa: E731
    out_bytes = V * N * NET * NET * 3
    return {"dewarp_32_views_two_launches": us(d32), "rotate_32_rotations_two_launches": us(r32), "output_bytes": out_bytes,
            "dewarp_ns_per_output_byte": statistics.median(d32) / out_bytes * 1e9, "rotate_ns_per_output_byte": statistics.median(r32) / out_bytes * 1e9,
            "dewarp_over_rotate": statistics.median(d32) / statistics.median(r32),
            "dewarp_output_GBps": out_bytes / statistics.median(d32) * 1e-9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dewarp_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args)
        return
    calls, claim = measure(args)
    res = {"tool": "tools/dewarp_bench.py", "net": "448x448", "precision": "fp16", "model": "mnet25", "max_batch": args.batch,
           "window_seconds": args.min_seconds, "windows": 3, "calls": calls, "claim": claim}
    if not args.no_trace:
        res["dewarp_launch"] = kernel_times_from_trace(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
