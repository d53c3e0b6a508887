#!/usr/bin/env python3
"""GPU tool: what motion-predicted tracks cost next to the plain tracker (DESIGN.md "Motion-predicted tracks"; writes
profiles/motion_bench.json).

Three things are measured, each with and without motion in alternating windows after warm-up, median of three windows:
  launch    the track launch alone, by HIP events around it in rf_track_update_device (rf_track_last_launch_ms), on the same constructed
            faces for both trackers: 8 streams x 32 faces x 64 slots (one image per stream and call) and 1 stream x 256 faces x 256 slots.
            The faces sit on a grid that drifts two pixels a call, back and forth, so every face matches its track in every call.  A
            window is --launches calls; its figure is the median launch time.
  call      rf_detect_track_batch_device over eight device-resident 448 x 448 frames on the fp16 engine (mnet25, max_batch 8), one frame
            per stream of an 8-stream tracker, in windows of at least --min-seconds, as ms per call
  parent    with --parent-lib (a libretinaface_amd.so built from the parent commit): the plain tracked call of that library and of this
            one, in alternating child processes of three windows each.  The kernel is the same, so the two must agree within the spread
            between the windows.
No cost figure is promised: the file records what was measured.

usage: python tools/motion_bench.py [--out profiles/motion_bench.json] [--min-seconds 0.5] [--launches 200] [--parent-lib PATH]
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
from track_bench import CAP, N, NET, device_frames  # noqa: E402

SHAPES = ((8, 32, 64), (1, 256, 256))          # streams, faces per image, slots
PERIOD = 16


def grid_faces(m, t):
    """m faces (15 floats each) on a 16 x 16 grid of 40-pixel cells, shifted 2 * t pixels; scores descend"""
    j = np.arange(m)
    rows = np.zeros((m, 15), np.float32)
    x, y = 40.0 * (j % 16) + 2.0 * t, 40.0 * (j // 16)
    rows[:, 0] = 0.99 - 0.001 * j
    rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = x, y, x + 30, y + 30
    rows[:, 5:10] = x[:, None] + 30 * np.array([0.3, 0.7, 0.5, 0.35, 0.65], np.float32)
    rows[:, 10:15] = y[:, None] + 30 * np.array([0.4, 0.4, 0.6, 0.8, 0.8], np.float32)
    return rows


def spread(windows):
    return (max(windows) - min(windows)) / statistics.median(windows)


def measure_launch(det, args):
    from retinaface_amd import _lib
    from retinaface_amd._lib import rf_face, rf_track, rf_track_tag
    lib, h = det._lib, det._h
    out = {}
    for n_streams, m, slots in SHAPES:
        trackers = {"plain": det.tracker(n_streams, max_tracks=slots), "motion": det.tracker(n_streams, max_tracks=slots, motion=True)}
        steps = [np.ascontiguousarray(np.broadcast_to(grid_faces(m, t if t < PERIOD else 2 * PERIOD - t), (n_streams, m, 15)))
                 for t in range(2 * PERIOD)]
        counts = (C.c_int * n_streams)(*[m] * n_streams)
        streams = (C.c_int * n_streams)(*range(n_streams))
        tags, ended, ecounts = (rf_track_tag * (n_streams * m))(), (rf_track * (n_streams * 8))(), (C.c_int * n_streams)()
        ms = C.c_float()
        at = {k: 0 for k in trackers}

        def one(name):
            faces = steps[at[name] % len(steps)]
            at[name] += 1
            _lib.check(lib.rf_track_update_device(h, trackers[name]._t, streams, n_streams, faces.ctypes.data_as(C.POINTER(rf_face)), m, counts,
                                                  None, None, CAP, tags, ended, 8, ecounts), h)
            _lib.check(lib.rf_track_last_launch_ms(h, C.byref(ms)), h)
            return float(ms.value)
        for _ in range(50):
            for name in trackers:
                one(name)
        wins = {k: [] for k in trackers}
        for _ in range(3):                      # alternate, so drift hits both alike
            for name in trackers:
                wins[name].append(statistics.median(one(name) for _ in range(args.launches)))
        live = {k: int((t.read(0)[0]["id"] != 0).sum()) for k, t in trackers.items()}
        samples = int(trackers["motion"].read_motion(0)["samples"].min()) if m >= slots else None
        for t in trackers.values():
            t.close()
        med = {k: statistics.median(v) for k, v in wins.items()}
        out["%dx%dx%d" % (n_streams, m, slots)] = {
            "streams": n_streams, "faces": m, "slots": slots, "launches_per_window": args.launches, "live_tracks_stream0": live,
            "fewest_velocity_samples_stream0": samples,
            "launch_ms": med, "launch_ms_windows": wins, "relative_spread": {k: spread(v) for k, v in wins.items()},
            "motion_over_plain": med["motion"] / med["plain"], "motion_minus_plain_us": (med["motion"] - med["plain"]) * 1e3,
        }
    return out


def tracked_call(lib, h, tracker, frames):
    from retinaface_amd._lib import rf_face, rf_track, rf_track_tag
    ptrs = (C.c_void_p * N)(*[f.data_ptr() for f in frames])
    r, c, s = (C.c_int * N)(*[NET] * N), (C.c_int * N)(*[NET] * N), (C.c_int * N)(*[NET * 3] * N)
    out, counts = (rf_face * (N * CAP))(), (C.c_int * N)()
    streams = (C.c_int * N)(*range(N))
    tags, ended, ecounts = (rf_track_tag * (N * CAP))(), (rf_track * (N * 64))(), (C.c_int * N)()

    def call():
        assert lib.rf_detect_track_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts, tracker, streams, tags, ended, 64, ecounts) == 0
    return call, counts


def measure_call(det, frames, args):
    trackers = {"plain": det.tracker(N), "motion": det.tracker(N, motion=True)}
    calls = {k: tracked_call(det._lib, det._h, t._t, frames)[0] for k, t in trackers.items()}
    for _ in range(20):
        for fn in calls.values():
            fn()
    wins = {k: [] for k in calls}
    for _ in range(3):
        for k, fn in calls.items():
            wins[k].append(window(fn, args.min_seconds) * 1e3)
    for t in trackers.values():
        t.close()
    med = {k: statistics.median(v) for k, v in wins.items()}
    return {"frames": N, "streams": N, "call_ms": med, "call_ms_windows": wins, "relative_spread": {k: spread(v) for k, v in wins.items()},
            "motion_over_plain": med["motion"] / med["plain"]}


def tracked_child(lib_path, min_seconds):
    """the plain tracked call through a library given by path, bound by hand: a library of the parent commit lacks the newer symbols"""
    import torch  # noqa: F401  (one HIP runtime in the process, as retinaface_amd._lib does)
    from retinaface_amd._lib import rf_face, rf_options, rf_track, rf_track_tag
    frames = device_frames()
    lib = C.CDLL(lib_path)
    o = rf_options()
    o.struct_size, o.precision, o.net_h, o.net_w, o.max_batch, o.model_stem = C.sizeof(rf_options), 1, NET, NET, N, b"mnet25"
    h, t = C.c_void_p(), C.c_void_p()
    P = C.POINTER
    lib.rf_create.argtypes = [C.c_char_p, C.c_char_p, C.c_float, P(rf_options), P(C.c_void_p)]
    lib.rf_tracker_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, P(C.c_void_p)]
    lib.rf_tracker_destroy.argtypes = [C.c_void_p]
    lib.rf_destroy.argtypes = [C.c_void_p]
    lib.rf_detect_track_batch_device.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_int), P(C.c_int), P(C.c_int), C.c_int, C.c_float, P(rf_face), C.c_int,
                                                 P(C.c_int), C.c_void_p, P(C.c_int), P(rf_track_tag), P(rf_track), C.c_int, P(C.c_int)]
    assert lib.rf_create(os.path.join(ROOT, "assets").encode(), b"net3", 0.4, C.byref(o), C.byref(h)) == 0
    assert lib.rf_tracker_create(h, None, N, C.byref(t)) == 0
    call, counts = tracked_call(lib, h, t, frames)
    for _ in range(20):
        call()
    samples = [window(call, min_seconds) * 1e3 for _ in range(3)]
    lib.rf_tracker_destroy(t)
    lib.rf_destroy(h)
    print(json.dumps({"call_ms_windows": samples, "faces": [int(counts[i]) for i in range(N)]}))


def measure(args):
    import retinaface_amd
    frames = device_frames()
    det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", 0.4, precision=retinaface_amd.PRECISION_FP16, net_hw=(NET, NET),
                                    model_stem="mnet25", max_batch=N)
    res = {"track_launch": measure_launch(det, args), "tracked_call": measure_call(det, frames, args)}
    det.close()
    if args.parent_lib:
        this_lib = retinaface_amd.lib_path()
        ab = {"parent": [], "this": []}
        for _ in range(3):                      # alternating child processes, one library each
            for name, path in (("parent", args.parent_lib), ("this", this_lib)):
                child = subprocess.run([sys.executable, os.path.abspath(__file__), "--tracked-child", path, "--min-seconds", str(args.min_seconds)],
                                       capture_output=True, text=True, timeout=300)
                if child.returncode != 0:
                    raise RuntimeError("the child of the %s library failed:\n%s" % (name, child.stderr[-2000:]))
                ab[name] += json.loads(child.stdout.strip().splitlines()[-1])["call_ms_windows"]
        med = {k: statistics.median(v) for k, v in ab.items()}
        res["plain_tracked_ab"] = {"call_ms": med, "call_ms_windows": ab, "relative_spread": {k: spread(v) for k, v in ab.items()},
                                   "this_over_parent": med["this"] / med["parent"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_bench.json"))
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--parent-lib", default=None, help="libretinaface_amd.so built from the parent commit: its plain tracked call is timed against this one's")
    ap.add_argument("--tracked-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.tracked_child:
        tracked_child(args.tracked_child, args.min_seconds)
        return
    res = {"tool": "tools/motion_bench.py", "net": "448x448", "precision": "fp16", "model": "mnet25", "max_batch": N, "window_seconds": args.min_seconds,
           "windows": 3}
    res.update(measure(args))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
