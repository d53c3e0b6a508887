#!/usr/bin/env python3
"""GPU tool: what zoom-pyramid detection costs and finds next to what a caller could do without it (DESIGN.md "Zoom-pyramid
detection"; writes profiles/pyramid_bench.json).

Two sets of eight device-resident frames on the fp16 engine (mnet25) at 448 x 448, default pyramid spec (1x and 2x):
  mosaic336x480   the 3 x 3 mosaic of the base frame shrunk eight times (54 faces of 11 to 14 px): 9 passes per frame
  synth448x448    seeded synthetic frames with pasted faces: 10 passes per frame
Per set five calls are timed in alternation, each in windows of at least --min-seconds after warm-up, median of three windows:
  pyramid     rf_detect_pyramid_batch_device
  plain       rf_detect_batch_device on the frames, as before
  tiled       rf_detect_tiled_batch_device on the frames (overlap 128, edge 8, full-frame pass on)
  passes      rf_detect_batch_device over the passes of all frames -- 1x views, and zoom tiles made BEFOREHAND: the floor under the
              pyramid call, which adds the zoom, gather and merge launches
  by_hand     numpy zoom of every tile and its upload, passes, then mapping and vote on the host in numpy (the arithmetic of
              tests/pyramid_ref.py; its result is checked against the pyramid call's bytes)
and the faces each finds are counted.  --zoom-only runs 50 pyramid calls of one set and nothing else: under
`rocprofv3 --kernel-trace --stats` that gives zoom_tile_kernel (and the pyramid's pass_gather_kernel) alone; `derived` holds the bytes one call's zoom
launches must move (every tile written once, every source frame read once) for the comparison with HBM peak.
No speed-up is promised: the file records what was measured.

usage: python tools/pyramid_bench.py [--out profiles/pyramid_bench.json] [--min-seconds 0.5] [--zoom-only SET]
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
SETS = {"mosaic336x480": (336, 480, 8), "synth448x448": (448, 448, 8)}
HBM_PEAK_BYTES_PER_S = 8.0e12      # MI355X: 8 TB/s


def build_frames(name, n):
    import pyramid_ref
    from retinaface_amd.frames import padded_base_frame, synth_frames
    if name == "synth448x448":
        return synth_frames(448, 448, n, config=1)
    return [pyramid_ref.mosaic(padded_base_frame())] * n


def merge_by_hand(plan, rows, cols, faces, counts, cap):
    """edge rule (edge 8), mapping and vote of one frame on the host, one pass at a time: faces (passes, cap, 15), counts per pass"""
    import pyramid_ref as pr
    import tta_ref
    f32 = np.float32
    xs, ys = [1, 3, 5, 6, 7, 8, 9], [2, 4, 10, 11, 12, 13, 14]
    cand, gs = [], []
    for p, (z, x0, y0, tw, th) in enumerate(tuple(int(v) for v in q) for q in plan):
        k = min(counts[p], cap)
        f = faces[p, :k].copy()
        g = p * cap + np.arange(k)
        if pr.is_full(plan[p], rows, cols, NET, NET):
            f[:, 1:] = f[:, 1:] * tta_ref.frame_scale(rows, cols, NET, NET)
        else:                                                # the edge rule against the virtual frame, then the mapping
            keep = np.ones(k, bool)
            if x0 > 0:
                keep &= ~(f[:, 1] < f32(8))
            if y0 > 0:
                keep &= ~(f[:, 2] < f32(8))
            if x0 + tw < z * cols:
                keep &= ~(f[:, 3] > f32(tw - 1 - 8))
            if y0 + th < z * rows:
                keep &= ~(f[:, 4] > f32(th - 1 - 8))
            f, g = f[keep], g[keep]
            f[:, xs] = f[:, xs] + f32(x0)
            f[:, ys] = f[:, ys] + f32(y0)
            if z > 1:
                f[:, 1:] = f[:, 1:] * (f32(1) / f32(z)) - f32(z - 1) / f32(2 * z)
        cand.append(f)
        gs.append(g)
    return tta_ref.merge_candidates(np.concatenate(cand), np.concatenate(gs), NMS, cap)[0]


class PyramidWorkload:
    def __init__(self, name, rows, cols, n, batch):
        import torch
        import pyramid_ref
        import retinaface_amd
        import tta_ref
        from retinaface_amd import _lib
        assert torch.cuda.is_available(), "this tool measures: it needs the GPU"
        self.torch, self._lib, self.pr, self.tr = torch, _lib, pyramid_ref, tta_ref
        self.rows, self.cols, self.n = rows, cols, n
        self.host = build_frames(name, n)
        self.frames = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in self.host]
        self.plan = pyramid_ref.plan(rows, cols, NET, NET)
        self.P = len(self.plan)
        self.zoomed = [[p for p in self.plan if p[0] > 1] for _ in range(n)]
        self.tiles = [[torch.from_numpy(pyramid_ref.zoom(f, int(p[0]), *(int(v) for v in p[1:]))).cuda() for p in self.plan if p[0] > 1]
                      for f in self.host]
        torch.cuda.synchronize()
        self.det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", NMS, precision=retinaface_amd.PRECISION_FP16,
                                             net_hw=(NET, NET), model_stem="mnet25", max_batch=batch)
        self.lib, self.h = self.det._lib, self.det._h
        self.cap = self.det.max_detections
        self.spec = retinaface_amd.pyramid_spec()
        self.tspec = retinaface_amd.tile_spec(128, 8, True)
        step = cols * 3
        self.ptrs = (C.c_void_p * n)(*[f.data_ptr() for f in self.frames])
        self.r, self.c, self.s = (C.c_int * n)(*[rows] * n), (C.c_int * n)(*[cols] * n), (C.c_int * n)(*[step] * n)
        self.out = (_lib.rf_face * (n * self.cap))()
        self.counts = (C.c_int * n)()
        self.votes, self.src = (C.c_int * (n * self.cap))(), (C.c_int * (n * self.cap))()
        pp, pr_, pc, ps = [], [], [], []
        for i in range(n):
            at = 0
            for z, x0, y0, tw, th in (tuple(int(v) for v in p) for p in self.plan):
                if z == 1:
                    pp.append(self.frames[i].data_ptr() + y0 * step + 3 * x0); ps.append(step)
                else:
                    pp.append(self.tiles[i][at].data_ptr()); ps.append(3 * tw)
                    at += 1
                pr_.append(th); pc.append(tw)
        m = n * self.P
        self.m = m
        self.pptrs, self.pr_, self.pc, self.ps = (C.c_void_p * m)(*pp), (C.c_int * m)(*pr_), (C.c_int * m)(*pc), (C.c_int * m)(*ps)
        self.pout = (_lib.rf_face * (m * self.cap))()
        self.pcounts = (C.c_int * m)()
        self.hand = None
        self.zoom_bytes_written = n * sum(int(p[3]) * int(p[4]) * 3 for p in self.plan if p[0] > 1)
        self.zoom_bytes_read = n * rows * cols * 3

    def pyramid(self):
        self._lib.check(self.lib.rf_detect_pyramid_batch_device(self.h, self.ptrs, self.r, self.c, self.s, self.n, 0.5, C.byref(self.spec),
                                                                self.out, self.cap, self.counts, self.votes, self.src), self.h)

    def plain(self):
        self._lib.check(self.lib.rf_detect_batch_device(self.h, self.ptrs, self.r, self.c, self.s, self.n, 0.5, self.out, self.cap,
                                                        self.counts), self.h)

    def tiled(self):
        self._lib.check(self.lib.rf_detect_tiled_batch_device(self.h, self.ptrs, self.r, self.c, self.s, self.n, 0.5, C.byref(self.tspec),
                                                              self.out, self.cap, self.counts, self.src), self.h)

    def passes(self):
        self._lib.check(self.lib.rf_detect_batch_device(self.h, self.pptrs, self.pr_, self.pc, self.ps, self.m, 0.5, self.pout,
                                                        self.cap, self.pcounts), self.h)

    def by_hand(self):
        n, cap, pr = self.n, self.cap, self.pr
        for i in range(n):                                   # the zoom on the host, into the tiles' device memory
            for t, p in zip(self.tiles[i], self.zoomed[i]):
                t.copy_(self.torch.from_numpy(pr.zoom(self.host[i], int(p[0]), *(int(v) for v in p[1:]))))
        self.torch.cuda.synchronize()
        self.passes()
        faces = np.ctypeslib.as_array(C.cast(self.pout, C.POINTER(C.c_float)), shape=(n, self.P, cap, 15))
        self.hand = [merge_by_hand(self.plan, self.rows, self.cols, faces[i], [self.pcounts[i * self.P + p] for p in range(self.P)], cap)
                     for i in range(n)]

    def call_faces(self):
        a = np.ctypeslib.as_array(C.cast(self.out, C.POINTER(C.c_float)), shape=(self.n, self.cap, 15))
        return [a[i, :min(self.counts[i], self.cap)].copy() for i in range(self.n)]


def measure(args, name):
    rows, cols, n = SETS[name]
    w = PyramidWorkload(name, rows, cols, n, args.batch)
    calls = {"pyramid": w.pyramid, "plain": w.plain, "tiled": w.tiled, "passes": w.passes, "by_hand": w.by_hand}
    for _ in range(3):                          # warm-up: every launch size, graph capture, scratch allocation
        for fn in calls.values():
            fn()
    found = {}
    w.plain()
    found["plain"] = [int(w.counts[i]) for i in range(n)]
    w.tiled()
    found["tiled"] = [int(w.counts[i]) for i in range(n)]
    w.pyramid()
    pyr = w.call_faces()
    found["pyramid"] = [int(w.counts[i]) for i in range(n)]
    votes = [[int(w.votes[i * w.cap + k]) for k in range(min(w.counts[i], w.cap))] for i in range(n)]
    w.by_hand()
    found["by_hand"] = [len(f) for f in w.hand]
    same = all(a.tobytes() == b.tobytes() for a, b in zip(pyr, w.hand))
    samples = {k: [] for k in calls}
    for _ in range(3):                          # alternate, so drift hits all alike
        for k, fn in calls.items():
            samples[k].append(window(fn, args.min_seconds))
    med = {k: statistics.median(v) for k, v in samples.items()}
    res = {
        "frames": n, "frame_size": f"{cols}x{rows}", "passes_per_frame": w.P, "zoom_tiles_per_frame": len(w.zoomed[0]),
        "faces_per_frame": found, "faces_with_two_or_more_votes": [sum(1 for v in vs if v >= 2) for vs in votes],
        "pyramid_equals_by_hand": bool(same),
        "call_ms": {k: med[k] * 1e3 for k in med},
        "call_ms_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
        "relative_spread": {k: (max(v) - min(v)) / med[k] for k, v in samples.items()},
        "pyramid_over_plain": med["pyramid"] / med["plain"],
        "pyramid_over_tiled": med["pyramid"] / med["tiled"],
        "pyramid_minus_passes_ms": (med["pyramid"] - med["passes"]) * 1e3,
        "pyramid_over_passes": med["pyramid"] / med["passes"],
        "by_hand_over_pyramid": med["by_hand"] / med["pyramid"],
        "derived": {"zoom_bytes_written_per_call": w.zoom_bytes_written, "zoom_bytes_read_per_call": w.zoom_bytes_read,
                    "zoom_us_at_hbm_peak": (w.zoom_bytes_written + w.zoom_bytes_read) / HBM_PEAK_BYTES_PER_S * 1e6,
                    "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S},
    }
    w.det.close()
    return res


def zoom_only(args):
    rows, cols, n = SETS[args.zoom_only]
    w = PyramidWorkload(args.zoom_only, rows, cols, n, args.batch)
    for _ in range(53):
        w.pyramid()
    w.det.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--zoom-only", default=None, help="run 53 pyramid calls of one set and exit: for `rocprofv3 --kernel-trace --stats -- "
                    "python tools/pyramid_bench.py --zoom-only mosaic336x480`, which gives zoom_tile_kernel alone")
    args = ap.parse_args()
    if args.zoom_only:
        zoom_only(args)
        return
    res = {"tool": "tools/pyramid_bench.py", "net": "448x448", "precision": "fp16", "model": "mnet25", "max_batch": args.batch,
           "window_seconds": args.min_seconds, "windows": 3, "spec": "default: levels 3 (1x and 2x), overlap 112, edge 8, vote on",
           "sets": {name: measure(args, name) for name in SETS}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
