#!/usr/bin/env python3
"""GPU tool: what tracking costs next to the plain detect call (DESIGN.md "Face tracks"; writes profiles/track_bench.json).

Eight device-resident 448 x 448 frames on the fp16 engine (mnet25, max_batch 8), one frame per stream of an 8-stream tracker.  Two calls
are timed in alternation, each in windows of at least --min-seconds after warm-up, median of three windows:
  tracked   rf_detect_track_batch_device
  plain     rf_detect_batch_device on the same frames, in the same process
and, with --parent-lib (a libretinaface_amd.so built from the parent commit), the plain call of that library in a child process of its
own.  The track launch alone is timed by HIP events around the launch of rf_track_update_device on the faces the plain call returned
(rf_track_last_launch_ms).  No cost figure is promised: the file records what was measured.

usage: python tools/track_bench.py [--out profiles/track_bench.json] [--min-seconds 0.5] [--parent-lib PATH]
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

NET, N, CAP = 448, 8, 256


def device_frames():
    import torch
    from retinaface_amd.frames import synth_frames
    assert torch.cuda.is_available(), "this tool measures: it needs the GPU"
    frames = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in synth_frames(NET, NET, N, config=1)]
    torch.cuda.synchronize()
    return frames


def plain_child(lib_path, min_seconds):
    """the plain call through a library given by path, bound by hand: a library of the parent commit lacks the newer symbols"""
    import torch  # noqa: F401  (one HIP runtime in the process, as retinaface_amd._lib does)
    from retinaface_amd._lib import rf_face, rf_options
    frames = device_frames()
    lib = C.CDLL(lib_path)
    o = rf_options()
    o.struct_size, o.precision, o.net_h, o.net_w, o.max_batch, o.model_stem = C.sizeof(rf_options), 1, NET, NET, N, b"mnet25"
    h = C.c_void_p()
    lib.rf_create.argtypes = [C.c_char_p, C.c_char_p, C.c_float, C.POINTER(rf_options), C.POINTER(C.c_void_p)]
    assert lib.rf_create(os.path.join(ROOT, "assets").encode(), b"net3", 0.4, C.byref(o), C.byref(h)) == 0
    lib.rf_detect_batch_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                           C.c_float, C.POINTER(rf_face), C.c_int, C.POINTER(C.c_int)]
    lib.rf_destroy.argtypes = [C.c_void_p]
    ptrs = (C.c_void_p * N)(*[f.data_ptr() for f in frames])
    r, c, s = (C.c_int * N)(*[NET] * N), (C.c_int * N)(*[NET] * N), (C.c_int * N)(*[NET * 3] * N)
    out, counts = (rf_face * (N * CAP))(), (C.c_int * N)()

    def plain():
        assert lib.rf_detect_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts) == 0
    for _ in range(20):
        plain()
    samples = [window(plain, min_seconds) for _ in range(3)]
    lib.rf_destroy(h)
    print(json.dumps({"call_ms_samples": [x * 1e3 for x in samples], "faces": [int(counts[i]) for i in range(N)]}))


def measure(args):
    import retinaface_amd
    from retinaface_amd import _lib
    from retinaface_amd._lib import rf_face, rf_track, rf_track_tag
    frames = device_frames()
    det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", 0.4, precision=retinaface_amd.PRECISION_FP16, net_hw=(NET, NET),
                                    model_stem="mnet25", max_batch=N)
    trk = det.tracker(N)
    lib, h = det._lib, det._h
    ptrs = (C.c_void_p * N)(*[f.data_ptr() for f in frames])
    r, c, s = (C.c_int * N)(*[NET] * N), (C.c_int * N)(*[NET] * N), (C.c_int * N)(*[NET * 3] * N)
    out, counts = (rf_face * (N * CAP))(), (C.c_int * N)()
    streams = (C.c_int * N)(*range(N))
    tags, ended, ecounts = (rf_track_tag * (N * CAP))(), (rf_track * (N * 64))(), (C.c_int * N)()

    def plain():
        _lib.check(lib.rf_detect_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts), h)

    def tracked():
        _lib.check(lib.rf_detect_track_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts, trk._t, streams, tags, ended, 64, ecounts), h)

    def update():
        _lib.check(lib.rf_track_update_device(h, trk._t, streams, N, out, CAP, counts, None, None, CAP, tags, ended, 64, ecounts), h)
    calls = {"tracked": tracked, "plain": plain}
    for _ in range(20):
        for fn in calls.values():
            fn()
    samples = {k: [] for k in calls}
    for _ in range(3):                          # alternate, so drift hits all alike
        for k, fn in calls.items():
            samples[k].append(window(fn, args.min_seconds))
    med = {k: statistics.median(v) for k, v in samples.items()}
    plain()
    faces = [int(counts[i]) for i in range(N)]
    launch, ms = [], C.c_float()
    for _ in range(50):
        update()
        _lib.check(lib.rf_track_last_launch_ms(h, C.byref(ms)), h)
        launch.append(float(ms.value))
    update_call = window(update, args.min_seconds)
    live = [int((trk.read(i)[0]["id"] != 0).sum()) for i in range(N)]
    res = {
        "frames": N, "streams": N, "faces_per_frame": faces, "live_tracks_per_stream": live,
        "call_ms": {k: med[k] * 1e3 for k in med},
        "call_ms_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
        "relative_spread": {k: (max(v) - min(v)) / med[k] for k, v in samples.items()},
        "images_per_s": {k: N / med[k] for k in med},
        "tracked_over_plain_throughput": med["plain"] / med["tracked"],
        "track_launch_ms_hip_events": {"median": statistics.median(launch), "min": min(launch), "max": max(launch), "launches": len(launch)},
        "track_update_call_ms": update_call * 1e3,
    }
    trk.close()
    det.close()
    if args.parent_lib:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-child", args.parent_lib, "--min-seconds", str(args.min_seconds)],
                               capture_output=True, text=True, timeout=300)
        if child.returncode != 0:
            raise RuntimeError("the parent-library child failed:\n" + child.stderr[-2000:])
        p = json.loads(child.stdout.strip().splitlines()[-1])
        pm = statistics.median(p["call_ms_samples"])
        res["parent_plain"] = {"call_ms": pm, "call_ms_samples": p["call_ms_samples"], "images_per_s": N / (pm * 1e-3), "faces_per_frame": p["faces"]}
        res["plain_over_parent_plain_throughput"] = pm / res["call_ms"]["plain"]
        res["tracked_over_parent_plain_throughput"] = pm / res["call_ms"]["tracked"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_bench.json"))
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--parent-lib", default=None, help="libretinaface_amd.so built from the parent commit: its plain call is timed in a child process")
    ap.add_argument("--plain-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.plain_child:
        plain_child(args.plain_child, args.min_seconds)
        return
    res = {"tool": "tools/track_bench.py", "net": "448x448", "precision": "fp16", "model": "mnet25", "max_batch": N, "window_seconds": args.min_seconds,
           "windows": 3}
    res.update(measure(args))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
