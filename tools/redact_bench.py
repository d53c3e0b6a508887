#!/usr/bin/env python3
"""GPU tool: what redaction costs next to the plain detect call (DESIGN.md "Face redaction"; writes profiles/redact_bench.json).

Eight device-resident frames on the fp16 engine (mnet25, max_batch 8): the 448 x 448 synthetic set of tools/track_bench.py and one
8 x 1280 x 896 set (the fixture photo).  A redacting call changes its frames -- pixelated faces are not found again -- so every timed
call that writes frames first restores them with one device-to-device copy, and the plain call is timed both ways: `plain` (no
restore, comparable with the parent commit) and `restore+plain` (the base line of everything that redacts).  Calls are timed in
alternation, each in windows of at least --min-seconds after warm-up, median of three windows:
  plain              rf_detect_batch_device
  restore+plain      the copy, then rf_detect_batch_device
  restore+redact     the copy, then rf_detect_redact_batch_device
  restore+tracked    the copy, then rf_detect_track_redact_batch_device (one frame per stream)
  restore+by_hand    the copy, then what a caller does without this feature: rf_detect_batch_device, frames to the host, rf_redact_host
                     on each, frames back to the device
and, with --parent-lib (a libretinaface_amd.so built from the parent commit), the plain call of that library in a child process.
The redaction launches alone are timed by HIP events around the launches of rf_redact_device on the faces the plain call returned
(rf_redact_last_launch_ms).  No cost figure is promised: the file records what was measured.

usage: python tools/redact_bench.py [--out profiles/redact_bench.json] [--min-seconds 0.5] [--parent-lib PATH]
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


def measure_set(det, frames, min_seconds):
    """frames: N equal-sized numpy frames"""
    import torch
    from retinaface_amd import _lib, redact_host
    from retinaface_amd._lib import rf_face, rf_track, rf_track_tag
    rows, cols = frames[0].shape[:2]
    orig = torch.from_numpy(np.stack(frames)).cuda()
    work = orig.clone()
    torch.cuda.synchronize()
    lib, h = det._lib, det._h
    fb = rows * cols * 3
    ptrs = (C.c_void_p * N)(*[work.data_ptr() + i * fb for i in range(N)])
    r, c, s = (C.c_int * N)(*[rows] * N), (C.c_int * N)(*[cols] * N), (C.c_int * N)(*[cols * 3] * N)
    out, counts = (rf_face * (N * CAP))(), (C.c_int * N)()
    pixels = (C.c_int32 * (N * CAP))()
    rcounts = (C.c_int * N)()
    streams = (C.c_int * N)(*range(N))
    tags, ended, ecounts = (rf_track_tag * (N * CAP))(), (rf_track * (N * 64))(), (C.c_int * N)()
    trk = det.tracker(N)
    scale = (C.c_float * N)(*[det.frame_scale(rows, cols)] * N)
    host = np.zeros((N, rows, cols, 3), np.uint8)

    def restore():
        work.copy_(orig)
        torch.cuda.synchronize()

    def plain():
        _lib.check(lib.rf_detect_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts), h)

    def restore_plain():
        restore()
        plain()

    def restore_redact():
        restore()
        _lib.check(lib.rf_detect_redact_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts, None, pixels), h)

    def restore_tracked():
        restore()
        _lib.check(lib.rf_detect_track_redact_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts, trk._t, streams, tags, ended, 64, ecounts,
                                                           None, pixels, rcounts), h)

    def restore_by_hand():
        restore()
        plain()
        host[:] = work.cpu().numpy()
        rows15 = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_float)), shape=(N, CAP, 15))
        for i in range(N):
            redact_host(host[i], rows15[i, :min(counts[i], CAP)], float(scale[i]))
        work.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()

    def restore_standalone():
        restore()
        _lib.check(lib.rf_redact_device(h, ptrs, r, c, s, N, out, CAP, counts, scale, None, None, None, pixels, rcounts), h)

    calls = {"plain": plain, "restore+plain": restore_plain, "restore+redact": restore_redact, "restore+tracked": restore_tracked,
             "restore+by_hand": restore_by_hand}
    for _ in range(10):
        for fn in calls.values():
            fn()
    samples = {k: [] for k in calls}
    for _ in range(3):                          # alternate, so drift hits all alike
        for k, fn in calls.items():
            samples[k].append(window(fn, min_seconds))
    med = {k: statistics.median(v) for k, v in samples.items()}
    restore_plain()
    faces = [int(counts[i]) for i in range(N)]
    launch, ms = [], C.c_float()
    for _ in range(50):
        restore_plain()
        counts_now = [int(counts[i]) for i in range(N)]
        restore_standalone()
        _lib.check(lib.rf_redact_last_launch_ms(h, C.byref(ms)), h)
        launch.append(float(ms.value))
    owned = int(np.ctypeslib.as_array(pixels).sum())
    trk.close()
    return {
        "frames": N, "rows": rows, "cols": cols, "faces_per_frame": faces, "faces_per_frame_at_the_launch_timing": counts_now,
        "pixels_owned_per_call": owned,
        "call_ms": {k: med[k] * 1e3 for k in med},
        "call_ms_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
        "relative_spread": {k: (max(v) - min(v)) / med[k] for k, v in samples.items()},
        "redaction_cost_ms_derived": {"fused": (med["restore+redact"] - med["restore+plain"]) * 1e3,
                                      "tracked": (med["restore+tracked"] - med["restore+plain"]) * 1e3,
                                      "by_hand": (med["restore+by_hand"] - med["restore+plain"]) * 1e3},
        "by_hand_over_fused_call_time": med["restore+by_hand"] / med["restore+redact"],
        "redact_launches_ms_hip_events": {"median": statistics.median(launch), "min": min(launch), "max": max(launch), "launches": len(launch)},
    }


def measure(args):
    import retinaface_amd
    from retinaface_amd.frames import padded_base_frame, synth_frames
    det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", 0.4, precision=retinaface_amd.PRECISION_FP16, net_hw=(NET, NET),
                                    model_stem="mnet25", max_batch=N)
    res = {"448x448": measure_set(det, [np.ascontiguousarray(f) for f in synth_frames(NET, NET, N, config=1)], args.min_seconds)}
    big = padded_base_frame()
    res["1280x896"] = measure_set(det, [big] * N, args.min_seconds)
    det.close()
    if args.parent_lib:
        child = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "track_bench.py"), "--plain-child", args.parent_lib,
                                "--min-seconds", str(args.min_seconds)], capture_output=True, text=True, timeout=300)
        if child.returncode != 0:
            raise RuntimeError("the parent-library child failed:\n" + child.stderr[-2000:])
        p = json.loads(child.stdout.strip().splitlines()[-1])
        pm = statistics.median(p["call_ms_samples"])
        res["parent_plain_448x448"] = {"call_ms": pm, "call_ms_samples": p["call_ms_samples"],
                                       "relative_spread": (max(p["call_ms_samples"]) - min(p["call_ms_samples"])) / pm,
                                       "faces_per_frame": p["faces"]}
        res["plain_over_parent_plain_call_time"] = res["448x448"]["call_ms"]["plain"] / pm
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "redact_bench.json"))
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--parent-lib", default=None, help="libretinaface_amd.so built from the parent commit: its plain call is timed in a child process")
    args = ap.parse_args()
    res = {"tool": "tools/redact_bench.py", "net": "448x448", "precision": "fp16", "model": "mnet25", "max_batch": N,
           "window_seconds": args.min_seconds, "windows": 3}
    res.update(measure(args))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
