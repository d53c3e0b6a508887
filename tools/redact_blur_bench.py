#!/usr/bin/env python3
"""GPU tool: what blur redaction costs next to pixelation and the plain detect call (DESIGN.md "Blur redaction"; writes
profiles/redact_blur_bench.json).

The frames of tools/redact_bench.py: eight device-resident 448 x 448 synthetic frames and eight 1280 x 896 ones (the fixture photo) on
the fp16 engine (mnet25, max_batch 8).  A redacting call changes its frames, so every timed call that writes frames first restores
them with one device-to-device copy.  Calls are timed in alternation, each in windows of at least --min-seconds after warm-up, median
of three windows, the spread recorded:
  restore+plain            the copy, then rf_detect_batch_device
  restore+redact           the copy, then rf_detect_redact_batch_device, pixelating (blur = 0)
  restore+blur1 / +blur3   the same call with blur = 1 / 3
  restore+tracked_blur3    the copy, then rf_detect_track_redact_batch_device with blur = 3 (one frame per stream)
  restore+by_hand_blur3    the copy, then what a caller does without the fused call: rf_detect_batch_device, frames to the host,
                           rf_redact_host with blur = 3 on each, frames back to the device
The redaction launches alone are timed by HIP events around the launches of rf_redact_device on the faces the plain call returned
(rf_redact_last_launch_ms), for pixelation and for blur = 3.  Also recorded, not asserted: how many of the original faces a second
plain detection still finds (IoU > 0.5) after pixelation and after blur = 3.
With --parent-lib (a libretinaface_amd.so built from the parent commit) restore+plain and the pixelating restore+redact are timed
through that library AND through this commit's, each in a child process of its own that binds the library by hand, so the two are
measured by the same code.  No cost figure is promised: the file records what was measured.

usage: python tools/redact_blur_bench.py [--out profiles/redact_blur_bench.json] [--min-seconds 0.5] [--parent-lib PATH]
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


def frame_sets():
    from retinaface_amd.frames import padded_base_frame, synth_frames
    return {"448x448": [np.ascontiguousarray(f) for f in synth_frames(NET, NET, N, config=1)], "1280x896": [padded_base_frame()] * N}


def timed(calls, min_seconds, warm=10):
    for _ in range(warm):
        for fn in calls.values():
            fn()
    samples = {k: [] for k in calls}
    for _ in range(3):                          # alternate, so drift hits all alike
        for k, fn in calls.items():
            samples[k].append(window(fn, min_seconds))
    med = {k: statistics.median(v) for k, v in samples.items()}
    return {"call_ms": {k: med[k] * 1e3 for k in med}, "call_ms_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
            "relative_spread": {k: (max(v) - min(v)) / med[k] for k, v in samples.items()}}, med


def iou(a, b):
    iw, ih = min(a[2], b[2]) - max(a[0], b[0]), min(a[3], b[3]) - max(a[1], b[1])
    if iw <= 0 or ih <= 0:
        return 0.0
    inter = iw * ih
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def child(lib_path, min_seconds):
    """restore+plain and the pixelating restore+redact through a library given by path, bound by hand (a library of the parent commit
    lacks nothing these two need)"""
    import torch
    from retinaface_amd._lib import rf_face, rf_options
    lib = C.CDLL(lib_path)
    o = rf_options()
    o.struct_size, o.precision, o.net_h, o.net_w, o.max_batch, o.model_stem = C.sizeof(rf_options), 1, NET, NET, N, b"mnet25"
    h = C.c_void_p()
    PP = C.POINTER
    lib.rf_create.argtypes = [C.c_char_p, C.c_char_p, C.c_float, PP(rf_options), PP(C.c_void_p)]
    assert lib.rf_create(os.path.join(ROOT, "assets").encode(), b"net3", 0.4, C.byref(o), C.byref(h)) == 0
    lib.rf_detect_batch_device.argtypes = [C.c_void_p, PP(C.c_void_p), PP(C.c_int), PP(C.c_int), PP(C.c_int), C.c_int, C.c_float, PP(rf_face),
                                           C.c_int, PP(C.c_int)]
    lib.rf_detect_redact_batch_device.argtypes = lib.rf_detect_batch_device.argtypes + [C.c_void_p, PP(C.c_int32)]
    lib.rf_destroy.argtypes = [C.c_void_p]
    res = {}
    for name, frames in frame_sets().items():
        rows, cols = frames[0].shape[:2]
        orig = torch.from_numpy(np.stack(frames)).cuda()
        work = orig.clone()
        torch.cuda.synchronize()
        fb = rows * cols * 3
        ptrs = (C.c_void_p * N)(*[work.data_ptr() + i * fb for i in range(N)])
        r, c, s = (C.c_int * N)(*[rows] * N), (C.c_int * N)(*[cols] * N), (C.c_int * N)(*[cols * 3] * N)
        out, counts, pixels = (rf_face * (N * CAP))(), (C.c_int * N)(), (C.c_int32 * (N * CAP))()

        def restore():
            work.copy_(orig)
            torch.cuda.synchronize()

        def restore_plain():
            restore()
            assert lib.rf_detect_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts) == 0

        def restore_redact():
            restore()
            assert lib.rf_detect_redact_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts, None, pixels) == 0

        res[name], _ = timed({"restore+plain": restore_plain, "restore+redact": restore_redact}, min_seconds)
    lib.rf_destroy(h)
    print(json.dumps(res))


def measure_set(det, frames, min_seconds):
    """frames: N equal-sized numpy frames"""
    import torch
    from retinaface_amd import _lib, redact_host, redact_spec
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
    spec = {b: redact_spec(blur=b) for b in (0, 1, 3)}

    def restore():
        work.copy_(orig)
        torch.cuda.synchronize()

    def plain():
        _lib.check(lib.rf_detect_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts), h)

    def restore_plain():
        restore()
        plain()

    def fused(b):
        def fn():
            restore()
            _lib.check(lib.rf_detect_redact_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts, C.byref(spec[b]), pixels), h)
        return fn

    def restore_tracked():
        restore()
        _lib.check(lib.rf_detect_track_redact_batch_device(h, ptrs, r, c, s, N, 0.5, out, CAP, counts, trk._t, streams, tags, ended, 64, ecounts,
                                                           C.byref(spec[3]), pixels, rcounts), h)

    def restore_by_hand():
        restore()
        plain()
        host[:] = work.cpu().numpy()
        rows15 = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_float)), shape=(N, CAP, 15))
        for i in range(N):
            redact_host(host[i], rows15[i, :min(counts[i], CAP)], float(scale[i]), blur=3)
        work.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()

    def standalone(b):
        restore()
        _lib.check(lib.rf_redact_device(h, ptrs, r, c, s, N, out, CAP, counts, scale, C.byref(spec[b]), None, None, pixels, rcounts), h)

    calls = {"restore+plain": restore_plain, "restore+redact": fused(0), "restore+blur1": fused(1), "restore+blur3": fused(3),
             "restore+tracked_blur3": restore_tracked, "restore+by_hand_blur3": restore_by_hand}
    res, med = timed(calls, min_seconds)
    restore_plain()
    faces = [int(counts[i]) for i in range(N)]
    boxes = [[tuple(np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_float)), shape=(N, CAP, 15))[i, k, 1:5]) for k in range(faces[i])]
             for i in range(N)]
    ms = C.c_float()
    launches, owned, found = {}, {}, {}
    for name, b in (("pixelate", 0), ("blur3", 3)):
        ts = []
        for _ in range(50):
            restore_plain()
            standalone(b)
            _lib.check(lib.rf_redact_last_launch_ms(h, C.byref(ms)), h)
            ts.append(float(ms.value))
        launches[name] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "launches": len(ts)}
        owned[name] = int(np.ctypeslib.as_array(pixels).sum())
        plain()                                 # a second detection, on the redacted frames
        again = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_float)), shape=(N, CAP, 15))
        hit = sum(any(iou(bx, tuple(again[i, k, 1:5])) > 0.5 for k in range(min(counts[i], CAP))) for i in range(N) for bx in boxes[i])
        found[name] = {"original_faces": sum(faces), "found_again_iou_over_0.5": int(hit)}
    trk.close()
    res.update({
        "frames": N, "rows": rows, "cols": cols, "faces_per_frame": faces, "pixels_owned_per_call": owned,
        "cost_over_restore_plus_plain_ms": {k: (med[k] - med["restore+plain"]) * 1e3 for k in med if k != "restore+plain"},
        "by_hand_over_fused_blur3_call_time": med["restore+by_hand_blur3"] / med["restore+blur3"],
        "by_hand_over_fused_blur3_cost": (med["restore+by_hand_blur3"] - med["restore+plain"]) / max(med["restore+blur3"] - med["restore+plain"], 1e-9),
        "redact_launches_ms_hip_events": launches,
        "blur3_launches_over_pixelate_launches": launches["blur3"]["median"] / launches["pixelate"]["median"],
        "faces_found_again_after_redaction": found,
    })
    return res


def run_child(lib_path, min_seconds):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib_path, "--min-seconds", str(min_seconds)], capture_output=True,
                       text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError("the child for %s failed:\n%s" % (lib_path, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def measure(args):
    import retinaface_amd
    det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", 0.4, precision=retinaface_amd.PRECISION_FP16, net_hw=(NET, NET),
                                    model_stem="mnet25", max_batch=N)
    res = {name: measure_set(det, frames, args.min_seconds) for name, frames in frame_sets().items()}
    det.close()
    if args.parent_lib:
        res["children"] = {"parent": run_child(os.path.abspath(args.parent_lib), args.min_seconds),
                           "this_commit": run_child(retinaface_amd.lib_path(), args.min_seconds)}
        res["this_commit_over_parent_call_time"] = {
            name: {k: res["children"]["this_commit"][name]["call_ms"][k] / res["children"]["parent"][name]["call_ms"][k]
                   for k in ("restore+plain", "restore+redact")} for name in ("448x448", "1280x896")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "redact_blur_bench.json"))
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--parent-lib", default=None, help="libretinaface_amd.so built from the parent commit: timed in a child process, like this commit's")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.min_seconds)
        return
    res = {"tool": "tools/redact_blur_bench.py", "net": "448x448", "precision": "fp16", "model": "mnet25", "max_batch": N,
           "window_seconds": args.min_seconds, "windows": 3}
    res.update(measure(args))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
