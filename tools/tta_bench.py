#!/usr/bin/env python3
"""GPU tool: what flip test-time augmentation costs and finds next to what a caller could do without it (DESIGN.md "Flip test-time
augmentation"; writes profiles/tta_bench.json).

Two sets of eight device-resident frames on the fp16 engine (mnet25) at 448 x 448:
  448x448     seeded synthetic frames with pasted faces
  1280x896    the 2 x 2 mosaic of the half-size base frame (24 faces of 50-58 px each), shrunk to the net by the engine
Per set four calls are timed in alternation, each in windows of at least --min-seconds after warm-up, median of three windows:
  tta         rf_detect_tta_batch_device
  plain       rf_detect_batch_device on the frames, as before
  passes      rf_detect_batch_device on the 2n frames [f0, mirror(f0), f1, ...] with the mirrors made BEFOREHAND: the floor under any
              by-hand caller, who also has to mirror
  by_hand     passes, then un-flip and vote on the host in numpy (the arithmetic of tests/tta_ref.py; its result is checked against
              the TTA call's bytes)
and the faces each finds are counted.  The merge is also timed alone on constructed faces, as the whole rf_tta_merge_device call
(upload, gather, merge, copy-out) at 4096 singletons and at one cluster of 4096 members, next to the same call on two candidates;
--merge-only runs one of those cases under a kernel trace, which gives vote_merge_kernel alone.
No speed-up is promised: the file records what was measured.

usage: python tools/tta_bench.py [--out profiles/tta_bench.json] [--min-seconds 0.5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from align_bench import window  # noqa: E402

NET, NMS = 448, 0.4
SETS = {"448x448": (448, 448, 8), "1280x896": (896, 1280, 8)}


def build_frames(name, n):
    import tile_ref
    from retinaface_amd.frames import padded_base_frame, synth_frames
    if name == "448x448":
        return synth_frames(448, 448, n, config=1)
    return [tile_ref.mosaic(padded_base_frame())] * n


class TtaWorkload:
    def __init__(self, name, rows, cols, n, batch):
        import torch
        import retinaface_amd
        import tta_ref
        from retinaface_amd import _lib
        assert torch.cuda.is_available(), "this tool measures: it needs the GPU"
        self.torch, self._lib, self.tr = torch, _lib, tta_ref
        self.rows, self.cols, self.n = rows, cols, n
        host = build_frames(name, n)
        self.frames = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in host]
        self.mirrors = [torch.from_numpy(tta_ref.mirror(f)).cuda() for f in host]
        torch.cuda.synchronize()
        self.det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", NMS, precision=retinaface_amd.PRECISION_FP16,
                                             net_hw=(NET, NET), model_stem="mnet25", max_batch=batch)
        self.lib, self.h = self.det._lib, self.det._h
        self.cap = self.det.max_detections
        self.spec = retinaface_amd.tta_spec()
        self.scale = tta_ref.frame_scale(rows, cols, NET, NET)
        step = cols * 3
        self.ptrs = (C.c_void_p * n)(*[f.data_ptr() for f in self.frames])
        self.r, self.c, self.s = (C.c_int * n)(*[rows] * n), (C.c_int * n)(*[cols] * n), (C.c_int * n)(*[step] * n)
        self.out = (_lib.rf_face * (n * self.cap))()
        self.counts = (C.c_int * n)()
        self.votes, self.src = (C.c_int * (n * self.cap))(), (C.c_int * (n * self.cap))()
        both = [t.data_ptr() for pair in zip(self.frames, self.mirrors) for t in pair]
        self.pptrs = (C.c_void_p * (2 * n))(*both)
        self.pr, self.pc, self.ps = (C.c_int * (2 * n))(*[rows] * (2 * n)), (C.c_int * (2 * n))(*[cols] * (2 * n)), (C.c_int * (2 * n))(*[step] * (2 * n))
        self.pout = (_lib.rf_face * (2 * n * self.cap))()
        self.pcounts = (C.c_int * (2 * n))()
        self.hand = None

    def tta(self):
        self._lib.check(self.lib.rf_detect_tta_batch_device(self.h, self.ptrs, self.r, self.c, self.s, self.n, 0.5, C.byref(self.spec),
                                                            self.out, self.cap, self.counts, self.votes, self.src), self.h)

    def plain(self):
        self._lib.check(self.lib.rf_detect_batch_device(self.h, self.ptrs, self.r, self.c, self.s, self.n, 0.5, self.out, self.cap,
                                                        self.counts), self.h)

    def passes(self):
        self._lib.check(self.lib.rf_detect_batch_device(self.h, self.pptrs, self.pr, self.pc, self.ps, 2 * self.n, 0.5, self.pout,
                                                        self.cap, self.pcounts), self.h)

    def by_hand(self):
        n, cap, tr = self.n, self.cap, self.tr
        self.passes()
        faces = np.ctypeslib.as_array(C.cast(self.pout, C.POINTER(C.c_float)), shape=(n, 2, cap, 15))
        c = np.float32(self.cols - 1)
        res = []
        for i in range(n):
            rows_, gs = [], []
            for p in range(2):
                k = min(self.pcounts[2 * i + p], cap)
                f = faces[i, p, :k].copy()
                f[:, 1:] = f[:, 1:] * self.scale
                if p:                                      # un-flip: box sides and landmark pairs change places
                    g = f.copy()
                    f[:, 1], f[:, 3] = c - g[:, 3], c - g[:, 1]
                    f[:, 5:10] = c - g[:, [6, 5, 7, 9, 8]]
                    f[:, 10:15] = g[:, [11, 10, 12, 14, 13]]
                rows_.append(f)
                gs.append(p * cap + np.arange(k))
            cand, g = np.concatenate(rows_), np.concatenate(gs)
            res.append(tr.merge_candidates(cand, g, NMS, cap)[0])
        self.hand = res

    def tta_faces(self):
        a = np.ctypeslib.as_array(C.cast(self.out, C.POINTER(C.c_float)), shape=(self.n, self.cap, 15))
        return [a[i, :min(self.counts[i], self.cap)].copy() for i in range(self.n)]


def measure(args, name):
    rows, cols, n = SETS[name]
    w = TtaWorkload(name, rows, cols, n, args.batch)
    calls = {"tta": w.tta, "plain": w.plain, "passes": w.passes, "by_hand": w.by_hand}
    for _ in range(3):                          # warm-up: every launch size, graph capture, scratch allocation
        for fn in calls.values():
            fn()
    w.plain()
    found = {"plain": [int(w.counts[i]) for i in range(n)]}
    w.tta()
    tta = w.tta_faces()
    found["tta"] = [int(w.counts[i]) for i in range(n)]
    votes = [[int(w.votes[i * w.cap + k]) for k in range(min(w.counts[i], w.cap))] for i in range(n)]
    w.by_hand()
    found["by_hand"] = [len(f) for f in w.hand]
    same = all(a.tobytes() == b.tobytes() for a, b in zip(tta, w.hand))
    samples = {k: [] for k in calls}
    for _ in range(3):                          # alternate, so drift hits all alike
        for k, fn in calls.items():
            samples[k].append(window(fn, args.min_seconds))
    med = {k: statistics.median(v) for k, v in samples.items()}
    res = {
        "frames": n, "frame_size": f"{cols}x{rows}", "frame_scale": float(w.scale),
        "faces_per_frame": found, "faces_with_two_votes": [sum(1 for v in vs if v >= 2) for vs in votes], "tta_equals_by_hand": bool(same),
        "call_ms": {k: med[k] * 1e3 for k in med},
        "call_ms_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
        "relative_spread": {k: (max(v) - min(v)) / med[k] for k, v in samples.items()},
        "tta_over_plain": med["tta"] / med["plain"],
        "passes_over_tta": med["passes"] / med["tta"],
        "by_hand_over_tta": med["by_hand"] / med["tta"],
    }
    w.det.close()
    return res


def measure_merge(args, only=None):
    """the whole rf_tta_merge_device call on constructed faces: 2 candidates, 4096 singletons, one cluster of 4096 members.
    only: run just that case, 50 calls and no timing (the child of a kernel-trace run)"""
    import retinaface_amd
    md = 4096
    det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", NMS, precision=retinaface_amd.PRECISION_FP16, net_hw=(NET, NET),
                                    model_stem="mnet25", max_batch=1, coalesce=1, lanes=1, max_detections=md)
    rng = np.random.default_rng(0)

    def faces(count, clustered):
        f = np.zeros((count, 15), np.float32)
        j = np.arange(count)
        f[:, 0] = np.sort(rng.uniform(0.5, 1, count).astype(np.float32))[::-1]
        x = rng.uniform(-2, 2, count) + 200 if clustered else 3.0 + 10 * (j % 64)
        y = rng.uniform(-2, 2, count) + 150 if clustered else 3.0 + 10 * (j // 64)
        wh = 60.0 if clustered else 5.0
        f[:, 1], f[:, 2], f[:, 3], f[:, 4] = x, y, x + wh, y + wh
        f[:, 5:10] = f[:, 1:2] + wh * np.array([0.3, 0.7, 0.5, 0.35, 0.65], np.float32)
        f[:, 10:15] = f[:, 2:3] + wh * np.array([0.4, 0.4, 0.6, 0.8, 0.8], np.float32)
        return f
    out = {}
    for name, count, clustered in (("two_candidates", 2, True), ("singletons_4096", 4096, False), ("one_cluster_4096", 4096, True)):
        if only and name != only:
            continue
        f = faces(count, clustered)
        # all candidates in pass 0 of a 448 x 448 frame: nothing is mirrored, so the singletons stay disjoint
        sp = retinaface_amd.tta_spec()
        flat = np.zeros((2, md, 15), np.float32)
        flat[0, :count] = f
        pc = (C.c_int * 2)(count, 0)
        res = (retinaface_amd._lib.rf_face * md)()
        counts, votes, src = (C.c_int * 1)(), (C.c_int * md)(), (C.c_int * md)()
        one = (C.c_int * 1)(448)

        def call():
            retinaface_amd._lib.check(det._lib.rf_tta_merge_device(det._h, one, one, 1, C.byref(sp), flat.ctypes.data_as(C.POINTER(retinaface_amd._lib.rf_face)),
                                                                   pc, res, md, counts, votes, src), det._h)
        for _ in range(3):
            call()
        if only:
            for _ in range(50):
                call()
            continue
        samples = [window(call, args.min_seconds) for _ in range(3)]
        out[name] = {"candidates": count, "heads": int(counts[0]), "largest_cluster": int(max(votes[:max(int(counts[0]), 1)])),
                     "call_ms": statistics.median(samples) * 1e3, "call_ms_samples": [s * 1e3 for s in samples]}
    det.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--merge-only", default=None, help="run 50 rf_tta_merge_device calls of one merge case and exit: for "
                    "`rocprofv3 --kernel-trace --stats -- python tools/tta_bench.py --merge-only one_cluster_4096`, which gives vote_merge_kernel alone")
    args = ap.parse_args()
    if args.merge_only:
        measure_merge(args, args.merge_only)
        return
    res = {"tool": "tools/tta_bench.py", "net": "448x448", "precision": "fp16", "model": "mnet25", "max_batch": args.batch,
           "window_seconds": args.min_seconds, "windows": 3,
           "sets": {name: measure(args, name) for name in SETS},
           "merge_call": measure_merge(args)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
