#!/usr/bin/env python3
"""GPU tool: what a follow step costs next to the detection call it stands in for (DESIGN.md "Followed tracks"; writes
profiles/follow_bench.json and, with --parent-lib, profiles/follow_bench_ab.json).

Eight device-resident frames on the fp16 engine (mnet25, max_batch 8), one frame per stream of an 8-stream tracker, at 448 x 448 (the
synthetic frames of the other benches) and at 1280 x 896 (the base frame, shifted a few pixels per stream), with the faces the detector
finds there.  Timed in alternation, each in windows of at least --min-seconds after warm-up, median of three windows, ms per call:
  tracked   rf_detect_track_batch_device on a plain tracker: detection on every frame
  key       rf_detect_track_follow_batch_device: the same plus the keep launch
  follow    rf_track_follow_device: search and step launches, no forward pass (max_run is set high so every call really searches)
  schedule  key, follow, follow, follow -- as ms per frame set, against `tracked`
The search and step launches alone are timed by HIP events (rf_follow_last_launch_ms) on constructed tables with every slot live: 8
streams x 64 slots and 1 stream x 256 slots, 10-pixel faces (q = 1) on a 448 x 448 frame.  With --parent-lib (a libretinaface_amd.so
built from the parent commit) the plain tracked call of that library and of this one are timed in alternating child processes.  No
ratio is promised: the files record what was measured.

usage: python tools/follow_bench.py [--out profiles/follow_bench.json] [--min-seconds 0.5] [--parent-lib PATH]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from align_bench import window  # noqa: E402

N, CAP = 8, 256


def frames_448():
    from retinaface_amd.frames import synth_frames
    return [np.ascontiguousarray(f) for f in synth_frames(448, 448, N, config=1)]


def frames_1280():
    from retinaface_amd.frames import padded_base_frame
    base = padded_base_frame()
    return [np.ascontiguousarray(np.roll(base, (2 * i, 3 * i), (0, 1))) for i in range(N)]


def to_device(frames):
    import torch
    assert torch.cuda.is_available(), "this tool measures: it needs the GPU"
    dev = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()
    return dev


def tracked_child(lib_path, min_seconds):
    """the plain tracked call through a library given by path, bound by hand: a library of the parent commit lacks the newer symbols"""
    import torch  # noqa: F401  (one HIP runtime in the process, as retinaface_amd._lib does)
    from retinaface_amd._lib import rf_face, rf_options, rf_track, rf_track_tag
    dev = to_device(frames_448())
    lib = C.CDLL(lib_path)
    o = rf_options()
    o.struct_size, o.precision, o.net_h, o.net_w, o.max_batch, o.model_stem = C.sizeof(rf_options), 1, 448, 448, N, b"mnet25"
    h, t = C.c_void_p(), C.c_void_p()
    PI = C.POINTER(C.c_int)
    lib.rf_create.argtypes = [C.c_char_p, C.c_char_p, C.c_float, C.POINTER(rf_options), C.POINTER(C.c_void_p)]
    lib.rf_tracker_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.rf_detect_track_batch_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), PI, PI, PI, C.c_int, C.c_float, C.POINTER(rf_face), C.c_int, PI,
                                                 C.c_void_p, PI, C.POINTER(rf_track_tag), C.POINTER(rf_track), C.c_int, PI]
    lib.rf_tracker_destroy.argtypes = [C.c_void_p]
    lib.rf_destroy.argtypes = [C.c_void_p]
    assert lib.rf_create(os.path.join(ROOT, "assets").encode(), b"net3", 0.4, C.byref(o), C.byref(h)) == 0
    assert lib.rf_tracker_create(h, None, N, C.byref(t)) == 0
    ptrs = (C.c_void_p * N)(*[f.data_ptr() for f in dev])
    r, c, s = (C.c_int * N)(*[448] * N), (C.c_int * N)(*[448] * N), (C.c_int * N)(*[448 * 3] * N)
    out, counts, streams = (rf_face * (N * CAP))(), (C.c_int * N)(), (C.c_int * N)(*range(N))
    tags, ended, ec = (rf_track_tag * (N * CAP))(), (rf_track * (N * 64))(), (C.c_int * N)()

    def call():
        assert lib.rf_detect_track_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts, t, streams, tags, ended, 64, ec) == 0
    for _ in range(20):
        call()
    samples = [window(call, min_seconds) * 1e3 for _ in range(3)]
    lib.rf_tracker_destroy(t)
    lib.rf_destroy(h)
    print(json.dumps({"call_ms_samples": samples}))


def stats(v):
    m = statistics.median(v)
    return {"median": m, "min": min(v), "max": max(v), "relative_spread": (max(v) - min(v)) / m if m else 0.0, "samples": len(v)}


def measure_calls(rfa, frames, hw, min_seconds):
    dev = to_device(frames)
    rows, cols = frames[0].shape[:2]
    det = rfa.RetinaFace(os.path.join(ROOT, "assets"), "net3", 0.4, precision=rfa.PRECISION_FP16, net_hw=hw, model_stem="mnet25", max_batch=N)
    args = ([d.data_ptr() for d in dev], [rows] * N, [cols] * N)
    streams = list(range(N))
    plain = det.tracker(N)
    trk = det.tracker(N, follow=dict(max_run=65536))
    sched = det.tracker(N, follow=dict(max_run=65536))
    got, _, _ = det.detect_track_follow_device(*args, trk, streams, 0.5)
    faces = [len(d) for d in got]
    followed = [len(f) for f in trk.follow_device(*args, streams)[0]]

    def schedule():
        det.detect_track_follow_device(*args, sched, streams, 0.5)
        for _ in range(3):
            sched.follow_device(*args, streams)
    calls = {"tracked": lambda: det.detect_tracked_device(*args, plain, streams, 0.5),
             "key": lambda: det.detect_track_follow_device(*args, trk, streams, 0.5),
             "follow": lambda: trk.follow_device(*args, streams),
             "schedule": schedule}
    for _ in range(10):
        for fn in calls.values():
            fn()
    samples = {k: [] for k in calls}
    for _ in range(3):                          # alternate, so drift hits all alike
        for k, fn in calls.items():
            samples[k].append(window(fn, min_seconds) * 1e3 / (4 if k == "schedule" else 1))
    launch = []
    for _ in range(50):
        trk.follow_device(*args, streams)
        launch.append(trk.follow_last_launch_ms())
    med = {k: statistics.median(v) for k, v in samples.items()}
    res = {"frame": "%dx%d" % (cols, rows), "net": "%dx%d" % (hw[1], hw[0]), "frames": N, "faces_per_frame": faces, "followed_per_frame": followed,
           "call_ms": {k: stats(v) for k, v in samples.items()},
           "note": "schedule is ms per set of 8 frames averaged over key + 3 follow calls; the other rows are ms per call of 8 frames",
           "follow_over_tracked": med["follow"] / med["tracked"], "key_over_tracked": med["key"] / med["tracked"],
           "schedule_over_tracked": med["schedule"] / med["tracked"],
           "search_and_step_launches_ms_hip_events": stats(launch)}
    for t in (plain, trk, sched):
        t.close()
    det.close()
    return res


def measure_launches(rfa):
    """every slot live: a grid of 10-pixel faces on one 448 x 448 frame per stream"""
    det = rfa.RetinaFace(os.path.join(ROOT, "assets"), "net3", 0.4, precision=rfa.PRECISION_FP16, net_hw=(448, 448), model_stem="mnet25", max_batch=N)
    frames = frames_448()
    dev = to_device(frames)
    out = {}
    for n_streams, T in ((8, 64), (1, 256)):
        trk = det.tracker(n_streams, follow=dict(max_run=65536, max_mad=255), max_tracks=T)
        rowsf = np.zeros((T, 15), np.float32)
        for j in range(T):
            x, y = 4 + 27 * (j % 16), 4 + 27 * (j // 16)
            rowsf[j, :5] = (0.99 - 0.003 * j, x, y, x + 10, y + 10)
        args = ([d.data_ptr() for d in dev[:n_streams]], [448] * n_streams, [448] * n_streams)
        streams = list(range(n_streams))
        trk.update_follow(*args, streams, [rowsf] * n_streams)
        ms = []
        for _ in range(60):
            faces, _, _ = trk.follow_device(*args, streams)
            ms.append(trk.follow_last_launch_ms())
        assert all(len(f) == T for f in faces), "not every slot was followed"
        out["%d_streams_x_%d_slots" % (n_streams, T)] = dict(stats(ms[10:]), radius=8, q=1, searches_per_call=n_streams * T)
        trk.close()
    det.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "follow_bench.json"))
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "follow_bench_ab.json"))
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--parent-lib", default=None, help="libretinaface_amd.so built from the parent commit: its plain tracked call is timed against this one's")
    ap.add_argument("--tracked-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.tracked_child:
        tracked_child(args.tracked_child, args.min_seconds)
        return
    import retinaface_amd as rfa
    res = {"tool": "tools/follow_bench.py", "precision": "fp16", "model": "mnet25", "max_batch": N, "window_seconds": args.min_seconds, "windows": 3,
           "follow_spec": {"radius": 8, "max_mad": 16, "max_run": 65536},
           "at_448": measure_calls(rfa, frames_448(), (448, 448), args.min_seconds),
           "at_1280x896": measure_calls(rfa, frames_1280(), (448, 448), args.min_seconds),
           "launches_alone": measure_launches(rfa)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if args.parent_lib:
        this_lib = rfa.lib_path()
        ab = {"parent": [], "this": []}
        for _ in range(3):                      # alternating child processes, one library each
            for name, path in (("parent", args.parent_lib), ("this", this_lib)):
                child = subprocess.run([sys.executable, os.path.abspath(__file__), "--tracked-child", path, "--min-seconds", str(args.min_seconds)],
                                       capture_output=True, text=True, timeout=300)
                if child.returncode != 0:
                    raise RuntimeError("the child of the %s library failed:\n%s" % (name, child.stderr[-2000:]))
                ab[name] += json.loads(child.stdout.strip().splitlines()[-1])["call_ms_samples"]
        doc = {"tool": "tools/follow_bench.py --parent-lib", "call": "rf_detect_track_batch_device, 8 frames of 448x448, fp16 mnet25, plain tracker",
               "call_ms": {k: stats(v) for k, v in ab.items()},
               "this_over_parent": statistics.median(ab["this"]) / statistics.median(ab["parent"])}
        lo = min(min(ab["parent"]), min(ab["this"]))
        doc["medians_within_the_runs_own_spread"] = abs(statistics.median(ab["this"]) - statistics.median(ab["parent"])) <= max(
            max(ab["parent"]) - min(ab["parent"]), max(ab["this"]) - min(ab["this"]), 0.0 * lo)
        with open(args.ab_out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(json.dumps(doc))


if __name__ == "__main__":
    main()
