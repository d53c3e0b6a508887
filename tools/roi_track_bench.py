#!/usr/bin/env python3
"""GPU tool: what tracked region detection costs next to the same schedule composed by hand and next to tiling every frame (DESIGN.md
"Tracked region detection"; writes profiles/roi_track_bench.json).

The two workloads of tools/roi_bench.py on the fp16 engine (mnet25, net 448, grid 4), device-resident frames, one stream per frame,
trackers of max_tracks 16 and 64.  Three schedules of four frame sets each are timed in alternation, in windows of at least
--min-seconds after warm-up, median of three windows with the spread beside it; the figure is ms per frame set (the schedule / 4):
  fused    a tiled key frame + rf_track_update_device, then three rf_detect_track_roi_batch_device calls
  by_hand  a tiled key frame + rf_track_update_device, then three times rf_roi_from_faces on the host over the faces of the frame
           before, rf_detect_roi_batch_device and rf_track_update_device
  tiled    rf_detect_tiled_batch_device + rf_track_update_device on every frame
The kernels alone come from a rocprofv3 kernel trace of a child process (--trace-child): the roi_track_cells_kernel dispatch and the
roi_atlas_kernel dispatches of a tracked region call (sized for x1/4, void cells for the free slots), and the roi_atlas_kernel dispatches
of the plain region call over the regions of the same tracks (sized by the host from the levels, no void cells).
--parent-lib: the plain region call, the tiled call and the plain call through the parent commit's library and through this one's, in
alternating child processes.  No speed-up is promised: the file records what was measured.

usage: python tools/roi_track_bench.py [--out profiles/roi_track_bench.json] [--min-seconds 0.5] [--no-trace]
"""
import argparse
import csv
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
from roi_bench import NET, NMS, frame_sets  # noqa: E402

TRACE_WARM, TRACE_CALLS = 2, 10
MAX_TRACKS = (16, 64)


class Workload:
    def __init__(self, batch):
        import torch
        import retinaface_amd
        assert torch.cuda.is_available(), "this tool measures: it needs the GPU"
        self.torch, self.rfa = torch, retinaface_amd
        self.det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", NMS, precision=retinaface_amd.PRECISION_FP16,
                                             net_hw=(NET, NET), model_stem="mnet25", max_batch=batch)
        self.sets = {}
        for name, frames in frame_sets().items():
            dev = [torch.from_numpy(f).cuda() for f in frames]
            torch.cuda.synchronize()
            self.sets[name] = dict(dev=dev, ptrs=[d.data_ptr() for d in dev], rows=[f.shape[0] for f in frames], cols=[f.shape[1] for f in frames],
                                   streams=list(range(len(frames))))

    def tracker(self, s, max_tracks):
        return self.det.tracker(len(s["ptrs"]), max_tracks=max_tracks)

    def key(self, s, trk):
        faces = self.det.detect_tiled_device(s["ptrs"], s["rows"], s["cols"], 0.5)
        trk.update(s["streams"], faces)
        return faces

    def fused(self, s, trk):
        self.key(s, trk)
        for _ in range(3):
            out = trk.detect_tracked_rois_device(s["ptrs"], s["rows"], s["cols"], s["streams"], 0.5)
        return out[0]

    def by_hand(self, s, trk):
        faces = self.key(s, trk)
        for _ in range(3):
            rois = [self.rfa.rois_from_faces(f)[:256] for f in faces]
            faces = self.det.detect_rois_device(s["ptrs"], s["rows"], s["cols"], rois, 0.5)
            trk.update(s["streams"], faces)
        return faces

    def tiled(self, s, trk):
        for _ in range(4):
            faces = self.key(s, trk)
        return faces


def measure(args):
    w = Workload(args.batch)
    out = {}
    for name, s in w.sets.items():
        for T in MAX_TRACKS:
            trks = {k: w.tracker(s, T) for k in ("fused", "by_hand", "tiled")}
            calls = {"fused": lambda: w.fused(s, trks["fused"]), "by_hand": lambda: w.by_hand(s, trks["by_hand"]), "tiled": lambda: w.tiled(s, trks["tiled"])}
            for _ in range(3):
                for fn in calls.values():
                    fn()
            found = {k: [len(x) for x in fn()] for k, fn in calls.items()}
            live = {k: [int((t.read(i)[0]["id"] != 0).sum()) for i in s["streams"]] for k, t in trks.items()}
            samples = {k: [] for k in calls}
            for _ in range(3):                      # alternate, so drift hits all alike
                for k, fn in calls.items():
                    samples[k].append(window(fn, args.min_seconds) / 4)
            med = {k: statistics.median(v) for k, v in samples.items()}
            out["%s/max_tracks_%d" % (name, T)] = {
                "passes_of_a_tracked_region_call": len(s["ptrs"]) * -(-T // 16),
                "faces_per_frame_of_the_last_frame_set": found, "live_tracks_per_stream": live,
                "ms_per_frame_set": {k: med[k] * 1e3 for k in med},
                "ms_per_frame_set_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
                "relative_spread": {k: (max(v) - min(v)) / med[k] for k, v in samples.items()},
                "fused_over_by_hand": med["fused"] / med["by_hand"], "fused_over_tiled": med["fused"] / med["tiled"],
                "by_hand_over_tiled": med["by_hand"] / med["tiled"],
            }
            for t in trks.values():
                t.close()
    w.det.close()
    return out


def trace_child(args):
    w = Workload(args.batch)
    for name, s in w.sets.items():
        for T in MAX_TRACKS:
            trk = w.tracker(s, T)
            w.key(s, trk)
            for _ in range(TRACE_WARM + TRACE_CALLS):
                faces = trk.detect_tracked_rois_device(s["ptrs"], s["rows"], s["cols"], s["streams"], 0.5)[0]
            rois = [w.rfa.rois_from_faces(f)[:256] for f in faces]
            for _ in range(TRACE_WARM + TRACE_CALLS):
                w.det.detect_rois_device(s["ptrs"], s["rows"], s["cols"], rois, 0.5)
            trk.close()
    w.det.close()


def kernel_times_from_trace(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "roi_track", "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--batch", str(args.batch)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed:\n" + r.stderr[-2000:])
        rec = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Kernel_Name", "")
                kind = "plan" if "roi_track_cells" in name else "atlas" if "roi_atlas" in name else None
                if kind:
                    rec.append((int(row["Start_Timestamp"]), kind, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-9))
    rec.sort()
    # the dispatches in order: per configuration, per tracked call one plan dispatch and then its atlas dispatches; then the plain
    # region calls' atlas dispatches.  Calls are told apart by the plan dispatches; the host-planned calls have equal dispatch counts.
    us = lambda v: {"median_us": statistics.median(v) * 1e6, "min_us": min(v) * 1e6, "max_us": max(v) * 1e6, "calls": len(v)}  # noqa: E731
    per = TRACE_WARM + TRACE_CALLS
    res, at = {}, 0
    for name, frames in (("8x1280x896", 8), ("2x3840x2160", 2)):
        for T in MAX_TRACKS:
            plan, atlas_tracked = [], []
            for _ in range(per):
                if at >= len(rec) or rec[at][1] != "plan":
                    raise RuntimeError("unexpected dispatch order in the kernel trace at %d" % at)
                plan.append(rec[at][2])
                at += 1
                t = 0.0
                launches = 0
                while at < len(rec) and rec[at][1] == "atlas" and launches < -(-(frames * -(-T // 16)) // 16):
                    t += rec[at][2]
                    at += 1
                    launches += 1
                atlas_tracked.append(t)
            rest = []
            while at < len(rec) and rec[at][1] == "atlas":
                rest.append(rec[at][2])
                at += 1
            if len(rest) % per:
                raise RuntimeError("unexpected number of host-planned atlas dispatches: %d" % len(rest))
            k = len(rest) // per
            host = [sum(rest[i * k:(i + 1) * k]) for i in range(per)]
            res["%s/max_tracks_%d" % (name, T)] = {
                "plan_launch": us(plan[TRACE_WARM:]), "atlas_launches_of_a_tracked_call": us(atlas_tracked[TRACE_WARM:]),
                "atlas_launches_of_the_plain_region_call_over_the_same_tracks": us(host[TRACE_WARM:]),
                "atlas_dispatches_per_call": {"tracked": -(-(frames * -(-T // 16)) // 16), "plain": k}}
    return res


def ab_child(lib_path, min_seconds):
    """the plain, the tiled and the plain region call over the 8x1280x896 set through a library given by path, bound by hand: a library
    of the parent commit lacks the newer symbols"""
    import ctypes as C
    import torch
    from retinaface_amd._lib import rf_face, rf_options, rf_roi, rf_roi_spec, rf_tile_spec
    frames = frame_sets()["8x1280x896"]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()
    n, cap = len(frames), 256
    lib = C.CDLL(lib_path)
    o = rf_options()
    o.struct_size, o.precision, o.net_h, o.net_w, o.max_batch, o.model_stem = C.sizeof(rf_options), 1, NET, NET, 32, b"mnet25"
    h = C.c_void_p()
    PI = C.POINTER(C.c_int)
    lib.rf_create.argtypes = [C.c_char_p, C.c_char_p, C.c_float, C.POINTER(rf_options), C.POINTER(C.c_void_p)]
    lib.rf_detect_batch_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), PI, PI, PI, C.c_int, C.c_float, C.POINTER(rf_face), C.c_int, PI]
    lib.rf_detect_tiled_batch_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), PI, PI, PI, C.c_int, C.c_float, C.POINTER(rf_tile_spec),
                                                 C.POINTER(rf_face), C.c_int, PI, PI]
    lib.rf_detect_roi_batch_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), PI, PI, PI, C.c_int, C.POINTER(rf_roi), PI, C.c_float,
                                               C.POINTER(rf_roi_spec), C.POINTER(rf_face), C.c_int, PI, PI, PI, C.c_void_p]
    lib.rf_roi_from_faces.argtypes = [C.POINTER(rf_face), C.c_int, C.c_float, C.c_int, C.POINTER(rf_roi)]
    lib.rf_destroy.argtypes = [C.c_void_p]
    assert lib.rf_create(os.path.join(ROOT, "assets").encode(), b"net3", NMS, C.byref(o), C.byref(h)) == 0
    ptrs = (C.c_void_p * n)(*[f.data_ptr() for f in dev])
    r, c, s = (C.c_int * n)(*[896] * n), (C.c_int * n)(*[1280] * n), (C.c_int * n)(*[3840] * n)
    out, counts = (rf_face * (n * cap))(), (C.c_int * n)()

    def plain():
        assert lib.rf_detect_batch_device(h, ptrs, r, c, s, n, 0.5, out, cap, counts) == 0

    def tiled():
        assert lib.rf_detect_tiled_batch_device(h, ptrs, r, c, s, n, 0.5, None, out, cap, counts, None) in (0, -6)
    tiled()
    rois, rc = (rf_roi * (n * cap))(), (C.c_int * n)()
    at = 0
    for i in range(n):                              # the regions of every frame: its own faces as the tiled call finds them
        k = lib.rf_roi_from_faces(C.cast(C.byref(out, i * cap * C.sizeof(rf_face)), C.POINTER(rf_face)), min(counts[i], cap), 1.0, 0,
                                  C.cast(C.byref(rois, at * C.sizeof(rf_roi)), C.POINTER(rf_roi)))
        assert k >= 0
        rc[i] = k
        at += k

    def region():
        assert lib.rf_detect_roi_batch_device(h, ptrs, r, c, s, n, rois, rc, 0.5, None, out, cap, counts, None, None, None) in (0, -6)
    fns = {"plain": plain, "tiled": tiled, "region": region}
    for _ in range(10):
        for fn in fns.values():
            fn()
    res = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            res[k].append(window(fn, min_seconds) * 1e3)
    lib.rf_destroy(h)
    print(json.dumps(res))


def ab(args):
    import retinaface_amd
    libs = (("parent", os.path.abspath(args.parent_lib)), ("this", retinaface_amd.lib_path()))
    samples = {name: {"plain": [], "tiled": [], "region": []} for name, _ in libs}
    for _ in range(3):                          # alternating child processes, one library each
        for name, path in libs:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", path, "--min-seconds", str(args.min_seconds)],
                                   capture_output=True, text=True, timeout=300)
            if child.returncode != 0:
                raise RuntimeError("the child of the %s library failed:\n%s" % (name, child.stderr[-2000:]))
            got = json.loads(child.stdout.strip().splitlines()[-1])
            for k in got:
                samples[name][k] += got[k]
    doc = {"tool": "tools/roi_track_bench.py --parent-lib",
           "calls": "rf_detect_batch_device, rf_detect_tiled_batch_device and rf_detect_roi_batch_device, 8 frames of 1280x896, fp16 mnet25",
           "call_ms_samples": samples}
    for k in ("plain", "tiled", "region"):
        p, t = samples["parent"][k], samples["this"][k]
        doc[k] = {"parent_median_ms": statistics.median(p), "this_median_ms": statistics.median(t),
                  "this_over_parent": statistics.median(t) / statistics.median(p),
                  "parent_spread": (max(p) - min(p)) / statistics.median(p), "this_spread": (max(t) - min(t)) / statistics.median(t),
                  "difference_within_the_parents_spread": abs(statistics.median(t) - statistics.median(p)) <= max(p) - min(p)}
    with open(args.ab_out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_track_bench.json"))
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "roi_track_bench_ab.json"))
    ap.add_argument("--parent-lib", default=None, help="libretinaface_amd.so built from the parent commit: its plain, tiled and region calls are timed against this one's")
    ap.add_argument("--ab-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args)
        return
    if args.ab_child:
        ab_child(args.ab_child, args.min_seconds)
        return
    if args.parent_lib:
        ab(args)
        return
    res = {"tool": "tools/roi_track_bench.py", "net": "448x448", "precision": "fp16", "model": "mnet25", "grid": 4, "max_batch": args.batch,
           "window_seconds": args.min_seconds, "windows": 3, "schedules": measure(args)}
    if not args.no_trace:
        res["kernels"] = kernel_times_from_trace(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
