#!/usr/bin/env python3
"""GPU tool: what the overlay costs next to the plain detect call (DESIGN.md "Overlays"; writes profiles/overlay_bench.json).

The workload of tools/redact_bench.py: eight device-resident 448 x 448 synthetic frames on the fp16 engine (mnet25, max_batch 8), 21
faces in all.  An overlay changes its frames, so every timed call that writes frames first restores them with one device-to-device
copy, and the plain call is timed both ways.  Calls are timed in alternation, each in windows of at least --min-seconds after warm-up,
median of three windows:
  plain              rf_detect_batch_device
  restore+plain      the copy, then rf_detect_batch_device
  restore+overlay    the copy, then rf_detect_overlay_batch_device (the defaults: the reference's look)
  restore+labelled   the copy, then rf_detect_overlay_batch_device with score labels and alpha 128
  restore+by_hand    the copy, then what a caller does without this feature: rf_detect_batch_device, frames to the host, rf_overlay_host
                     on each, frames back to the device
The overlay launches alone are timed by HIP events around the two launches of rf_overlay_device on the faces the plain call returned
(rf_overlay_last_launch_ms), for the defaults and for labels plus alpha, and next to them -- same run, same frames, same faces -- the
launches of rf_redact_device (pixelation, rf_redact_last_launch_ms).
With --parent-lib (a libretinaface_amd.so built from the parent commit) the plain call and the plain TRACKED call
(rf_detect_track_batch_device, one frame per stream) are timed through this commit's library and through the parent's, each in a child
process of its own, twice in alternation; both exist in both libraries.  No cost figure is promised: the file records what was measured.

usage: python tools/overlay_bench.py [--out profiles/overlay_bench.json] [--min-seconds 0.5] [--parent-lib PATH]
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
from track_bench import device_frames  # noqa: E402

NET, N, CAP = 448, 8, 256


def tracked_child(lib_path, min_seconds):
    """the plain and the plain tracked call through a library given by path, bound by hand: a library of the parent commit lacks the
    newer symbols"""
    import torch  # noqa: F401  (one HIP runtime in the process, as retinaface_amd._lib does)
    from retinaface_amd._lib import rf_face, rf_options, rf_track, rf_track_tag
    frames = device_frames()
    lib = C.CDLL(lib_path)
    o = rf_options()
    o.struct_size, o.precision, o.net_h, o.net_w, o.max_batch, o.model_stem = C.sizeof(rf_options), 1, NET, NET, N, b"mnet25"
    h, t = C.c_void_p(), C.c_void_p()
    P = C.POINTER
    lib.rf_create.argtypes = [C.c_char_p, C.c_char_p, C.c_float, P(rf_options), P(C.c_void_p)]
    assert lib.rf_create(os.path.join(ROOT, "assets").encode(), b"net3", 0.4, C.byref(o), C.byref(h)) == 0
    lib.rf_detect_batch_device.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_int), P(C.c_int), P(C.c_int), C.c_int, C.c_float, P(rf_face), C.c_int,
                                           P(C.c_int)]
    lib.rf_tracker_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, P(C.c_void_p)]
    lib.rf_tracker_destroy.argtypes = [C.c_void_p]
    lib.rf_tracker_destroy.restype = None
    lib.rf_detect_track_batch_device.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_int), P(C.c_int), P(C.c_int), C.c_int, C.c_float, P(rf_face),
                                                 C.c_int, P(C.c_int), C.c_void_p, P(C.c_int), P(rf_track_tag), P(rf_track), C.c_int, P(C.c_int)]
    lib.rf_destroy.argtypes = [C.c_void_p]
    lib.rf_destroy.restype = None
    assert lib.rf_tracker_create(h, None, N, C.byref(t)) == 0
    ptrs = (C.c_void_p * N)(*[f.data_ptr() for f in frames])
    r, c, s = (C.c_int * N)(*[NET] * N), (C.c_int * N)(*[NET] * N), (C.c_int * N)(*[NET * 3] * N)
    out, counts = (rf_face * (N * CAP))(), (C.c_int * N)()
    streams = (C.c_int * N)(*range(N))
    tags, ended, ecounts = (rf_track_tag * (N * CAP))(), (rf_track * (N * 64))(), (C.c_int * N)()

    def plain():
        assert lib.rf_detect_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts) == 0

    def tracked():
        assert lib.rf_detect_track_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts, t, streams, tags, ended, 64, ecounts) == 0
    for _ in range(20):
        plain()
        tracked()
    samples = {"plain": [], "tracked": []}
    for _ in range(3):
        samples["plain"].append(window(plain, min_seconds) * 1e3)
        samples["tracked"].append(window(tracked, min_seconds) * 1e3)
    lib.rf_tracker_destroy(t)
    lib.rf_destroy(h)
    print(json.dumps({"call_ms_samples": samples, "faces": [int(counts[i]) for i in range(N)]}))


def measure_set(det, frames, min_seconds):
    """frames: N equal-sized numpy frames"""
    import torch
    from retinaface_amd import _lib, overlay_host, overlay_spec
    from retinaface_amd._lib import rf_face
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
    scale = (C.c_float * N)(*[det.frame_scale(rows, cols)] * N)
    host = np.zeros((N, rows, cols, 3), np.uint8)
    labelled = overlay_spec(label=1, alpha=128)

    def restore():
        work.copy_(orig)
        torch.cuda.synchronize()

    def plain():
        _lib.check(lib.rf_detect_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts), h)

    def restore_plain():
        restore()
        plain()

    def restore_overlay():
        restore()
        _lib.check(lib.rf_detect_overlay_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts, None, pixels), h)

    def restore_labelled():
        restore()
        _lib.check(lib.rf_detect_overlay_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts, C.byref(labelled), pixels), h)

    def restore_by_hand():
        restore()
        plain()
        host[:] = work.cpu().numpy()
        rows15 = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_float)), shape=(N, CAP, 15))
        for i in range(N):
            overlay_host(host[i], rows15[i, :min(counts[i], CAP)], float(scale[i]))
        work.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()

    calls = {"plain": plain, "restore+plain": restore_plain, "restore+overlay": restore_overlay, "restore+labelled": restore_labelled,
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
    launch = {"overlay_defaults": [], "overlay_labels_alpha": [], "pixelate_defaults": []}
    painted = {}
    ms = C.c_float()
    for _ in range(50):                          # the three launch timings in alternation, each on restored frames and the same faces
        for key, spec in (("overlay_defaults", None), ("overlay_labels_alpha", C.byref(labelled))):
            restore()
            _lib.check(lib.rf_overlay_device(h, ptrs, r, c, s, N, out, None, CAP, counts, scale, spec, None, None, pixels, rcounts), h)
            _lib.check(lib.rf_overlay_last_launch_ms(h, C.byref(ms)), h)
            launch[key].append(float(ms.value))
            painted[key] = int(np.ctypeslib.as_array(pixels).sum())
        restore()
        _lib.check(lib.rf_redact_device(h, ptrs, r, c, s, N, out, CAP, counts, scale, None, None, None, pixels, rcounts), h)
        _lib.check(lib.rf_redact_last_launch_ms(h, C.byref(ms)), h)
        launch["pixelate_defaults"].append(float(ms.value))
        painted["pixelate_defaults"] = int(np.ctypeslib.as_array(pixels).sum())
    return {
        "frames": N, "rows": rows, "cols": cols, "faces_per_frame": faces, "pixels_written_per_call": painted,
        "call_ms": {k: med[k] * 1e3 for k in med},
        "call_ms_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
        "relative_spread": {k: (max(v) - min(v)) / med[k] for k, v in samples.items()},
        "overlay_cost_ms_derived": {"fused": (med["restore+overlay"] - med["restore+plain"]) * 1e3,
                                    "fused_labelled": (med["restore+labelled"] - med["restore+plain"]) * 1e3,
                                    "by_hand": (med["restore+by_hand"] - med["restore+plain"]) * 1e3},
        "by_hand_over_fused_call_time": med["restore+by_hand"] / med["restore+overlay"],
        "launches_ms_hip_events": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "launches": len(v)} for k, v in launch.items()},
    }


def children(args):
    """plain and tracked call through this commit's library and the parent's: child processes, this | parent | this | parent"""
    import retinaface_amd
    libs = {"this_commit": retinaface_amd.lib_path(), "parent_commit": args.parent_lib}
    runs = {k: {"plain": [], "tracked": []} for k in libs}
    faces = {}
    for _ in range(2):
        for k, path in libs.items():
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--tracked-child", path, "--min-seconds", str(args.min_seconds)],
                                   capture_output=True, text=True, timeout=300)
            if child.returncode != 0:
                raise RuntimeError("the child of %s failed:\n%s" % (k, child.stderr[-2000:]))
            p = json.loads(child.stdout.strip().splitlines()[-1])
            for call in ("plain", "tracked"):
                runs[k][call] += p["call_ms_samples"][call]
            faces[k] = p["faces"]
    res = {}
    for k in libs:
        res[k] = {call: {"call_ms": statistics.median(v), "call_ms_samples": v, "relative_spread": (max(v) - min(v)) / statistics.median(v)}
                  for call, v in runs[k].items()}
        res[k]["faces_per_frame"] = faces[k]
    for call in ("plain", "tracked"):
        res[call + "_this_over_parent_call_time"] = res["this_commit"][call]["call_ms"] / res["parent_commit"][call]["call_ms"]
    return res


def measure(args):
    import retinaface_amd
    from retinaface_amd.frames import synth_frames
    det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", 0.4, precision=retinaface_amd.PRECISION_FP16, net_hw=(NET, NET),
                                    model_stem="mnet25", max_batch=N)
    res = {"448x448": measure_set(det, [np.ascontiguousarray(f) for f in synth_frames(NET, NET, N, config=1)], args.min_seconds)}
    det.close()
    if args.parent_lib:
        res["against_the_parent_commit_448x448"] = children(args)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_bench.json"))
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--parent-lib", default=None, help="libretinaface_amd.so built from the parent commit: its plain and tracked calls are timed in child processes")
    ap.add_argument("--tracked-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.tracked_child:
        tracked_child(args.tracked_child, args.min_seconds)
        return
    res = {"tool": "tools/overlay_bench.py", "net": "448x448", "precision": "fp16", "model": "mnet25", "max_batch": N,
           "window_seconds": args.min_seconds, "windows": 3}
    res.update(measure(args))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
