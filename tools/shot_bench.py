#!/usr/bin/env python3
"""GPU tool: what the best-shot gallery costs next to the calls around it (DESIGN.md "Best-shot gallery"; writes profiles/shot_bench.json).

Eight device-resident 448 x 448 frames on the fp16 engine (mnet25, max_batch 8), one frame per stream of an 8-stream tracker with
max_missed 0.  A call with the face-bearing frames (A) is followed by a call with eight blank frames (B): in A every track is born and
its best shot kept, in B every track ends and its shot is delivered, so both shot launches do real work in every cycle.  Four things
are timed in alternation, each in windows of at least --min-seconds after warm-up, median of three windows, as ms per call (half a cycle):
  shots     rf_detect_track_shots_batch_device with a gate (u8 HWC 112 gallery, shots to host memory)
  floor     rf_detect_track_face_batch_device with tensor = NULL and the same gate: the same work without the gallery
  plain     rf_detect_batch_device
  by_hand   rf_detect_track_face_batch_device with the full u8 tensor copied to the host, plus a numpy table that keeps each track's
            best crop by the tags and hands it over when the track ends: what a caller has to write without the gallery
by_hand's delivered crops are checked equal to the fused call's.  The two shot launches alone are timed by HIP events around them in
rf_track_shots_device on the faces the plain call returned (rf_shot_last_launch_ms).  With --parent-lib (a libretinaface_amd.so built
from the parent commit) the plain call of that library and of this one are timed in alternating child processes.  No cost figure is
promised: the file records what was measured.

usage: python tools/shot_bench.py [--out profiles/shot_bench.json] [--min-seconds 0.5] [--parent-lib PATH]
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

NET, N, CAP, CROP, CE = 448, 8, 256, 112, 8
BPF = CROP * CROP * 3


def measure(args):
    import torch
    import retinaface_amd
    from retinaface_amd import _lib
    from retinaface_amd._lib import rf_face, rf_face_quality, rf_shot, rf_track, rf_track_tag
    from retinaface_amd.detector import QUALITY_DTYPE, TRACK_DTYPE, TRACK_TAG_DTYPE, face_batch_spec, face_gate
    frames = device_frames()
    blank = torch.zeros((NET, NET, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", 0.4, precision=retinaface_amd.PRECISION_FP16, net_hw=(NET, NET),
                                    model_stem="mnet25", max_batch=N)
    spec = dict(max_missed=-1, min_hits=1)
    lib, h = det._lib, det._h
    pa = (C.c_void_p * N)(*[f.data_ptr() for f in frames])
    pb = (C.c_void_p * N)(*[blank.data_ptr()] * N)
    r, c, s = (C.c_int * N)(*[NET] * N), (C.c_int * N)(*[NET] * N), (C.c_int * N)(*[NET * 3] * N)
    out, counts = (rf_face * (N * CAP))(), (C.c_int * N)()
    streams = (C.c_int * N)(*range(N))
    tags = np.zeros((N, CAP), TRACK_TAG_DTYPE)
    ended = np.zeros((N, CE), TRACK_DTYPE)
    ecounts = np.zeros(N, np.int32)
    quality = np.zeros((N, CAP), QUALITY_DTYPE)
    shots = np.zeros((N, CE, BPF), np.uint8)
    info = (rf_shot * (N * CE))()
    tensor = np.zeros((N * CAP, BPF), np.uint8)
    offsets = (C.c_int * (N + 1))()
    gate = face_gate(min_sharpness=1e-6)
    fsp = face_batch_spec(CROP, "u8", False, max_faces=CAP, capacity=N * CAP)
    tg, en, ec = tags.ctypes.data_as(C.POINTER(rf_track_tag)), ended.ctypes.data_as(C.POINTER(rf_track)), ecounts.ctypes.data_as(C.POINTER(C.c_int))
    ql = quality.ctypes.data_as(C.POINTER(rf_face_quality))
    t_shots = det.tracker(N, **spec).enable_shots(crop_size=CROP, dtype="u8", rgb=False, max_faces=CAP)
    t_floor, t_hand, t_alone = det.tracker(N, **spec), det.tracker(N, **spec), det.tracker(N, **spec).enable_shots(crop_size=CROP, dtype="u8", rgb=False, max_faces=CAP)

    def fused(p):
        _lib.check(lib.rf_detect_track_shots_batch_device(h, p, r, c, s, N, 0.5, out, CAP, counts, t_shots._t, streams, tg, en, CE, ec, C.byref(gate),
                                                          ql, None, shots.ctypes.data, info), h)

    def floor(p):
        _lib.check(lib.rf_detect_track_face_batch_device(h, p, r, c, s, N, 0.5, out, CAP, counts, C.byref(fsp), None, None, None, offsets,
                                                         C.byref(gate), ql, t_floor._t, streams, tg, en, CE, ec), h)

    def plain(p):
        _lib.check(lib.rf_detect_batch_device(h, p, r, c, s, N, 0.5, out, CAP, counts), h)

    table, handed = {}, []

    def by_hand(p):
        _lib.check(lib.rf_detect_track_face_batch_device(h, p, r, c, s, N, 0.5, out, CAP, counts, C.byref(fsp), None, tensor.ctypes.data, None, offsets,
                                                         C.byref(gate), ql, t_hand._t, streams, tg, en, CE, ec), h)
        for i in range(N):
            k = min(int(counts[i]), CAP)
            if k:
                kept = quality[i, :k]["flags"] == 0
                packed = offsets[i] + np.cumsum(kept) - 1
                for j in np.nonzero((tags[i, :k]["flags"] & 4) != 0)[0]:
                    table[(i, int(tags[i, j]["id"]))] = tensor[packed[j]].copy()
            for e in range(min(int(ecounts[i]), CE)):
                handed.append(table.pop((i, int(ended[i, e]["id"])), None))

    # by_hand hands over the bytes the fused call delivers
    fused(pa); fused(pb)
    by_hand(pa); by_hand(pb)
    n_shots = int(sum(min(int(x), CE) for x in ecounts))
    got = [shots[i, e] for i in range(N) for e in range(min(int(ecounts[i]), CE))]
    assert n_shots == len(handed) > 0 and all(a is not None and a.tobytes() == b.tobytes() for a, b in zip(handed, got)), "by_hand differs"
    calls = {"shots": fused, "floor": floor, "plain": plain, "by_hand": by_hand}

    def cycle(fn):
        def run():
            fn(pa)
            fn(pb)
            handed.clear()
        return run
    for _ in range(10):
        for fn in calls.values():
            cycle(fn)()
    samples = {k: [] for k in calls}
    for _ in range(3):                          # alternate, so drift hits all alike
        for k, fn in calls.items():
            samples[k].append(window(cycle(fn), args.min_seconds) / 2)
    med = {k: statistics.median(v) for k, v in samples.items()}
    # the two shot launches alone: keep (frames A: every track is born) and deliver (frames B: every track ends)
    plain(pa)
    faces = [int(counts[i]) for i in range(N)]
    zero = (C.c_int * N)()
    launch, ms = {"keep_step": [], "deliver_step": []}, C.c_float()
    for _ in range(50):
        for name, p, cnt in (("keep_step", pa, counts), ("deliver_step", pb, zero)):
            _lib.check(lib.rf_track_shots_device(h, t_alone._t, p, r, c, s, N, streams, out, CAP, cnt, None, None, tg, en, CE, ec, None,
                                                 shots.ctypes.data, info), h)
            _lib.check(lib.rf_shot_last_launch_ms(h, C.byref(ms)), h)
            launch[name].append(float(ms.value))
    res = {
        "frames": N, "streams": N, "faces_per_frame_A": faces, "shots_per_cycle": n_shots, "crop": CROP, "format": "u8 HWC",
        "call_ms": {k: med[k] * 1e3 for k in med},
        "call_ms_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
        "relative_spread": {k: (max(v) - min(v)) / med[k] for k, v in samples.items()},
        "shots_over_floor": med["shots"] / med["floor"], "shots_over_by_hand": med["shots"] / med["by_hand"],
        "shots_over_plain": med["shots"] / med["plain"], "shots_minus_floor_ms": (med["shots"] - med["floor"]) * 1e3,
        "by_hand_equals_fused": True,
        "shot_launches_ms_hip_events": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "launches": len(v)} for k, v in launch.items()},
    }
    for t in (t_shots, t_floor, t_hand, t_alone):
        t.close()
    det.close()
    if args.parent_lib:
        this_lib = retinaface_amd.lib_path()
        ab = {"parent": [], "this": []}
        for _ in range(3):                      # alternating child processes, one library each
            for name, path in (("parent", args.parent_lib), ("this", this_lib)):
                child = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "track_bench.py"), "--plain-child", path, "--min-seconds",
                                        str(args.min_seconds)], capture_output=True, text=True, timeout=300)
                if child.returncode != 0:
                    raise RuntimeError("the child of the %s library failed:\n%s" % (name, child.stderr[-2000:]))
                ab[name].append(statistics.median(json.loads(child.stdout.strip().splitlines()[-1])["call_ms_samples"]))
        res["plain_ab_call_ms"] = ab
        res["plain_this_over_parent"] = statistics.median(ab["this"]) / statistics.median(ab["parent"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shot_bench.json"))
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--parent-lib", default=None, help="libretinaface_amd.so built from the parent commit: its plain call is timed against this one's")
    args = ap.parse_args()
    res = {"tool": "tools/shot_bench.py", "net": "448x448", "precision": "fp16", "model": "mnet25", "max_batch": N, "window_seconds": args.min_seconds,
           "windows": 3}
    res.update(measure(args))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
