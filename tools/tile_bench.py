#!/usr/bin/env python3
"""GPU tool: what tiled detection costs and finds next to the two things a caller could do before it (DESIGN.md "Tiled detection";
writes profiles/tile_bench.json).

Two sets of device-resident frames on the fp16 engine at 448 x 448 (overlap 128, edge 8, full-frame pass on):
  1280x896    8 copies of the 2 x 2 mosaic of the half-size base frame (24 faces of 50-58 px each; 13 passes per frame)
  3840x2160   2 frames tiled from the same half-size frame (6 x 5 repetitions cut to 2160 rows; 85 passes per frame)
Per set three calls are timed in alternation, each in windows of at least --min-seconds after warm-up, median of three windows:
  tiled       rf_detect_tiled_batch_device
  by_hand     the caller-side equivalent without it: rf_detect_batch_device on the ROI views, then edge rule, mapping and merge on the
              host (vectorised numpy: the arithmetic of tests/tile_ref.py; its result is checked against the tiled call's bytes)
  views       the device half of by_hand alone (rf_detect_batch_device on the ROI views, results on the host): what any caller-side
              merge, however fast, has to pay before it starts
  shrunk      rf_detect_batch_device on the whole frames, as before: every frame shrunk to the net
and the faces each finds are counted.  No speed-up is promised: the file records what was measured.
With the default options (max_batch 32, coalesce 8) the engine coalesces all passes of a call into ONE launch; --coalesce 1 (with
--batch 8, --lanes 2 or 3) makes a call many launches over several lanes, the setting in which the merge waits for other lanes.

usage: python tools/tile_bench.py [--out profiles/tile_bench.json] [--min-seconds 0.5]
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

NET, OV, EDGE, NMS = 448, 128, 8, 0.4
SETS = {"1280x896": (896, 1280, 8), "3840x2160": (2160, 3840, 2)}


def build_frame(rows, cols):
    import tile_ref
    from retinaface_amd.frames import padded_base_frame
    half = tile_ref.mosaic(padded_base_frame())[:448, :640]
    reps = (-(-rows // 448), -(-cols // 640), 1)
    return np.ascontiguousarray(np.tile(half, reps)[:rows, :cols])


class TileWorkload:
    def __init__(self, rows, cols, n, batch, coalesce=0, lanes=0):
        import torch
        import retinaface_amd
        import tile_ref
        from retinaface_amd import _lib
        assert torch.cuda.is_available(), "this tool measures: it needs the GPU"
        self.torch, self._lib, self.tr = torch, _lib, tile_ref
        self.rows, self.cols, self.n = rows, cols, n
        frame = torch.from_numpy(build_frame(rows, cols)).cuda()
        self.frames = [frame.clone() for _ in range(n)]
        torch.cuda.synchronize()
        self.det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", 0.4, precision=retinaface_amd.PRECISION_FP16,
                                             net_hw=(NET, NET), model_stem="mnet25", max_batch=batch, coalesce=coalesce, lanes=lanes)
        self.lib, self.h = self.det._lib, self.det._h
        self.cap = self.det.max_detections
        self.spec = retinaface_amd.tile_spec(OV, EDGE, True, 0)
        self.tiles = tile_ref.plan(rows, cols, NET, NET, OV, True)
        self.scale = tile_ref.frame_scale(rows, cols, NET, NET)
        P, step = len(self.tiles), cols * 3
        self.P = P
        self.ptrs = (C.c_void_p * n)(*[f.data_ptr() for f in self.frames])
        self.r, self.c, self.s = (C.c_int * n)(*[rows] * n), (C.c_int * n)(*[cols] * n), (C.c_int * n)(*[step] * n)
        self.out = (_lib.rf_face * (n * self.cap))()
        self.counts = (C.c_int * n)()
        self.src = (C.c_int * (n * self.cap))()
        views = [(f.data_ptr() + int(t[1]) * step + 3 * int(t[0]), int(t[3]), int(t[2])) for f in self.frames for t in self.tiles]
        self.vptrs = (C.c_void_p * (n * P))(*[v[0] for v in views])
        self.vr, self.vc = (C.c_int * (n * P))(*[v[1] for v in views]), (C.c_int * (n * P))(*[v[2] for v in views])
        self.vs = (C.c_int * (n * P))(*[step] * (n * P))
        self.vout = (_lib.rf_face * (n * P * self.cap))()
        self.vcounts = (C.c_int * (n * P))()
        self.hand = None

    def tiled(self):
        self._lib.check(self.lib.rf_detect_tiled_batch_device(self.h, self.ptrs, self.r, self.c, self.s, self.n, 0.5, C.byref(self.spec),
                                                              self.out, self.cap, self.counts, self.src), self.h)

    def shrunk(self):
        self._lib.check(self.lib.rf_detect_batch_device(self.h, self.ptrs, self.r, self.c, self.s, self.n, 0.5, self.out, self.cap,
                                                        self.counts), self.h)

    def views(self):
        self._lib.check(self.lib.rf_detect_batch_device(self.h, self.vptrs, self.vr, self.vc, self.vs, self.n * self.P, 0.5, self.vout,
                                                        self.cap, self.vcounts), self.h)

    def by_hand(self):
        n, P, cap, tr = self.n, self.P, self.cap, self.tr
        self.views()
        faces = np.ctypeslib.as_array(C.cast(self.vout, C.POINTER(C.c_float)), shape=(n, P, cap, 15))
        f32 = np.float32
        res = []
        for i in range(n):
            rows_, gs = [], []
            for t in range(P):
                k = min(self.vcounts[i * P + t], cap)
                if not k:
                    continue
                f = faces[i, t, :k].copy()
                x0, y0, tw, th = (int(v) for v in self.tiles[t])
                if t == P - 1:                                     # the full-frame pass
                    f[:, 1:] = f[:, 1:] * self.scale
                    keep = np.ones(k, bool)
                else:
                    keep = ~(((x0 > 0) & (f[:, 1] < f32(EDGE))) | ((y0 > 0) & (f[:, 2] < f32(EDGE))) |
                             ((x0 + tw < self.cols) & (f[:, 3] > f32(tw - 1 - EDGE))) | ((y0 + th < self.rows) & (f[:, 4] > f32(th - 1 - EDGE))))
                    f[:, [1, 3, 5, 6, 7, 8, 9]] += f32(x0)
                    f[:, [2, 4, 10, 11, 12, 13, 14]] += f32(y0)
                rows_.append(f[keep])
                gs.append(t * cap + np.nonzero(keep)[0])
            cand = np.concatenate(rows_) if rows_ else np.zeros((0, 15), f32)
            g = np.concatenate(gs) if gs else np.zeros(0, np.int64)
            res.append(cand[tr.nms(cand, g, NMS)] if len(cand) else cand)
        self.hand = res

    def tiled_faces(self):
        a = np.ctypeslib.as_array(C.cast(self.out, C.POINTER(C.c_float)), shape=(self.n, self.cap, 15))
        return [a[i, :min(self.counts[i], self.cap)].copy() for i in range(self.n)]


def measure(args, name):
    rows, cols, n = SETS[name]
    w = TileWorkload(rows, cols, n, args.batch, args.coalesce, args.lanes)
    calls = {"tiled": w.tiled, "by_hand": w.by_hand, "views": w.views, "shrunk": w.shrunk}
    for _ in range(3):                          # warm-up: every launch size, graph capture, scratch allocation
        for fn in calls.values():
            fn()
    w.shrunk()
    found = {"shrunk": [int(w.counts[i]) for i in range(n)]}
    w.tiled()
    tiled = w.tiled_faces()
    found["tiled"] = [int(w.counts[i]) for i in range(n)]
    w.by_hand()
    found["by_hand"] = [len(f) for f in w.hand]
    same = all(a.tobytes() == b[:len(a)].tobytes() for a, b in zip(tiled, w.hand))
    samples = {k: [] for k in calls}
    for _ in range(3):                          # alternate, so drift hits all alike
        for k, fn in calls.items():
            samples[k].append(window(fn, args.min_seconds))
    med = {k: statistics.median(v) for k, v in samples.items()}
    res = {
        "frames": n, "frame_size": f"{cols}x{rows}", "passes_per_frame": w.P, "frame_scale": float(w.scale),
        "faces_per_frame": found, "tiled_equals_by_hand": bool(same),
        "call_ms": {k: med[k] * 1e3 for k in med},
        "call_ms_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
        "relative_spread": {k: (max(v) - min(v)) / med[k] for k, v in samples.items()},
        "by_hand_over_tiled": med["by_hand"] / med["tiled"],
        "views_over_tiled": med["views"] / med["tiled"],
        "tiled_over_shrunk": med["tiled"] / med["shrunk"],
    }
    w.det.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--coalesce", type=int, default=0, help="chunks merged per launch (0 = the engine's default; 1 = one launch per max_batch images)")
    ap.add_argument("--lanes", type=int, default=0, help="launches in flight (0 = the engine's default: 3)")
    args = ap.parse_args()
    res = {"tool": "tools/tile_bench.py", "net": "448x448", "precision": "fp16", "model": "mnet25", "max_batch": args.batch, "coalesce": args.coalesce, "lanes": args.lanes,
           "overlap": OV, "edge": EDGE, "full_frame": True, "window_seconds": args.min_seconds, "windows": 3,
           "sets": {name: measure(args, name) for name in SETS}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
