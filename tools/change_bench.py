#!/usr/bin/env python3
"""GPU tool: what change regions cost (DESIGN.md "Change regions"; writes profiles/change_bench.json).

Kernels alone, from a rocprofv3 kernel trace of a child process (--trace-child), medians over the dispatches after warm-up:
  change_blocks_kernel over 8 x 1280 x 896 (B = 16) and 2 x 3840 x 2160 (B = 32), with the bytes it reads per second, next to
  enhance_lut_kernel over the same frames in the same run -- it also reads every pixel once -- and the ratio of the two;
  change_regions_kernel on a 128 x 128 grid (1024 x 1024, B = 8): an empty mask, a typical mask (a few blobs) and a one-block-wide
  spiral through the whole grid, without dilation.
Schedules (fp16 mnet25, net 448, grid 4, device frames, one stream per frame, max_tracks 10 and max_regions 6: one pass), timed in
alternation in windows of at least --min-seconds, median of three windows with the spread; ms per frame set (the schedule / 4):
  change   a tiled key frame + rf_track_update_device, then three rf_detect_change_roi_batch_device calls with the tracker
  tracked  the same with rf_detect_track_roi_batch_device: it misses newcomers until the next key frame
  tiled    rf_detect_tiled_batch_device + rf_track_update_device on every frame
The frame sets repeat their frames, so no block changes after the seeding call: the figure is the cost of the schedule, not of a
newcomer's extra region (tests/test_change_gpu.py holds the newcomer's case).  Not measured by this tool, and recorded as pending
in the file: the existing calls through the parent commit's library in alternation.  No speed-up is promised.

usage: python tools/change_bench.py [--out profiles/change_bench.json] [--min-seconds 0.5] [--no-trace]
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

TRACE_WARM, TRACE_CALLS = 3, 20
HBM_PEAK = 8.0e12                                   # bytes per second, MI355X
BLOCK_OF = {"8x1280x896": 16, "2x3840x2160": 32}
GRID = 128                                          # the regions kernel's cases: GRID x GRID blocks of 8 pixels


def spiral(n):
    m = np.zeros((n, n), np.uint8)
    x = y = turns = 0
    dx, dy = 1, 0
    m[0, 0] = 1
    while turns < 2:
        nx, ny, fx, fy = x + dx, y + dy, x + 2 * dx, y + 2 * dy
        if 0 <= nx < n and 0 <= ny < n and not m[ny, nx] and not (0 <= fx < n and 0 <= fy < n and m[fy, fx]):
            x, y, turns = nx, ny, 0
            m[y, x] = 1
        else:
            dx, dy, turns = -dy, dx, turns + 1
    return m


def region_masks():
    typical = np.zeros((GRID, GRID), np.uint8)
    for k, (y, x, h, w) in enumerate(((10, 12, 6, 5), (40, 90, 9, 7), (70, 30, 4, 12), (100, 100, 8, 8), (20, 60, 3, 3))):
        typical[y:y + h, x:x + w] = 1
    return {"empty": np.zeros((GRID, GRID), np.uint8), "typical": typical, "spiral": spiral(GRID)}


def mask_frame(mask, B):
    return np.repeat(np.repeat(mask, B, 0), B, 1)[:, :, None].repeat(3, 2) * np.uint8(255)


def engine(batch):
    import torch
    import retinaface_amd
    assert torch.cuda.is_available(), "this tool measures: it needs the GPU"
    det = retinaface_amd.RetinaFace(os.path.join(ROOT, "assets"), "net3", NMS, precision=retinaface_amd.PRECISION_FP16, net_hw=(NET, NET),
                                    model_stem="mnet25", max_batch=batch)
    return torch, det


def device_set(torch, frames):
    dev = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]
    torch.cuda.synchronize()
    return dict(dev=dev, ptrs=[d.data_ptr() for d in dev], rows=[f.shape[0] for f in frames], cols=[f.shape[1] for f in frames],
                streams=list(range(len(frames))))


def trace_child(args):
    """the dispatches the parent counts: per frame set 1 + WARM + CALLS change calls (blocks + regions each), then WARM + CALLS enhance
    calls (lut + apply each); then per regions case 1 + WARM + CALLS change calls"""
    torch, det = engine(args.batch)
    per = TRACE_WARM + TRACE_CALLS
    for name, frames in frame_sets().items():
        a = device_set(torch, frames)
        b = device_set(torch, [255 - f for f in frames])                  # every block changes on every call
        chg = det.changer(a["rows"][0], a["cols"][0], len(frames), block=BLOCK_OF[name])
        for k in range(per + 1):
            s = a if k % 2 == 0 else b
            chg.regions_device(s["ptrs"], s["rows"], s["cols"], s["streams"])
        chg.close()
        dst = [torch.empty_like(d) for d in a["dev"]]
        for k in range(per):
            s = a if k % 2 == 0 else b
            det.enhance_device(s["ptrs"], s["rows"], s["cols"], [d.data_ptr() for d in dst])
    zero = device_set(torch, [np.zeros((GRID * 8, GRID * 8, 3), np.uint8)])
    for name, mask in region_masks().items():
        m = device_set(torch, [mask_frame(mask, 8)])
        chg = det.changer(GRID * 8, GRID * 8, 1, block=8, dilate=2, min_blocks=1)
        for k in range(per + 1):                                          # zero, mask, zero, ..: the same blocks change on every call
            s = zero if k % 2 == 0 else m
            chg.regions_device(s["ptrs"], s["rows"], s["cols"], s["streams"])
        chg.close()
    det.close()


def kernel_times_from_trace(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "change", "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--batch", str(args.batch)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed:\n" + r.stderr[-2000:])
        rec = {"change_blocks": [], "change_regions": [], "enhance_lut": [], "enhance_apply": []}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for kind in rec:
                    if kind + "_kernel" in row.get("Kernel_Name", ""):
                        rec[kind].append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-9))
    for v in rec.values():
        v.sort()
    us = lambda v: {"median_us": statistics.median(v) * 1e6, "min_us": min(v) * 1e6, "max_us": max(v) * 1e6, "calls": len(v)}  # noqa: E731
    per = TRACE_WARM + TRACE_CALLS
    sets, cases = list(frame_sets().items()), list(region_masks().items())
    want = {"change_blocks": (per + 1) * (len(sets) + len(cases)), "change_regions": (per + 1) * (len(sets) + len(cases)), "enhance_lut": per * len(sets)}
    for k, n in want.items():
        if len(rec[k]) != n:
            raise RuntimeError("unexpected number of %s dispatches in the kernel trace: %d, not %d" % (k, len(rec[k]), n))
    res = {}
    for i, (name, frames) in enumerate(sets):
        nbytes = sum(f.shape[0] * f.shape[1] * 3 for f in frames)
        blocks = [d for _, d in rec["change_blocks"][i * (per + 1) + 1 + TRACE_WARM:(i + 1) * (per + 1)]]
        regions = [d for _, d in rec["change_regions"][i * (per + 1) + 1 + TRACE_WARM:(i + 1) * (per + 1)]]
        lut = [d for _, d in rec["enhance_lut"][i * per + TRACE_WARM:(i + 1) * per]]
        bps, lps = nbytes / statistics.median(blocks), nbytes / statistics.median(lut)
        res[name] = {"block": BLOCK_OF[name], "frame_bytes": nbytes, "change_blocks_kernel": us(blocks), "enhance_lut_kernel": us(lut),
                     "change_regions_kernel_every_block_changed": us(regions),
                     "change_blocks_bytes_per_second": bps, "change_blocks_fraction_of_hbm_peak": bps / HBM_PEAK,
                     "enhance_lut_bytes_per_second": lps, "change_blocks_time_over_enhance_lut_time": statistics.median(blocks) / statistics.median(lut)}
    for j, (name, mask) in enumerate(cases):
        i = len(sets) + j
        regions = [d for _, d in rec["change_regions"][i * (per + 1) + 1 + TRACE_WARM:(i + 1) * (per + 1)]]
        res["regions_kernel/%dx%d/%s" % (GRID, GRID, name)] = {"marked_blocks": int(mask.sum()), "change_regions_kernel": us(regions)}
    return res


def schedules(args):
    torch, det = engine(args.batch)
    out = {}
    for name, frames in frame_sets().items():
        s = device_set(torch, frames)

        def key(trk):
            faces = det.detect_tiled_device(s["ptrs"], s["rows"], s["cols"], 0.5)
            trk.update(s["streams"], faces)
            return faces
        trks = {k: det.tracker(len(frames), max_tracks=10) for k in ("change", "tracked", "tiled")}
        chg = det.changer(s["rows"][0], s["cols"][0], len(frames), block=BLOCK_OF[name], max_regions=6)

        def change():
            key(trks["change"])
            for _ in range(3):
                r = chg.detect_changed_device(s["ptrs"], s["rows"], s["cols"], s["streams"], tracker=trks["change"])
            return r[0]

        def tracked():
            key(trks["tracked"])
            for _ in range(3):
                r = trks["tracked"].detect_tracked_rois_device(s["ptrs"], s["rows"], s["cols"], s["streams"], 0.5)
            return r[0]

        def tiled():
            for _ in range(4):
                r = key(trks["tiled"])
            return r
        calls = {"change": change, "tracked": tracked, "tiled": tiled}
        for _ in range(3):
            for fn in calls.values():
                fn()
        found = {k: [len(x) for x in fn()] for k, fn in calls.items()}
        samples = {k: [] for k in calls}
        for _ in range(3):                          # alternate, so drift hits all alike
            for k, fn in calls.items():
                samples[k].append(window(fn, args.min_seconds) / 4)
        med = {k: statistics.median(v) for k, v in samples.items()}
        out[name] = {"faces_per_frame_of_the_last_frame_set": found, "ms_per_frame_set": {k: med[k] * 1e3 for k in med},
                     "ms_per_frame_set_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
                     "relative_spread": {k: (max(v) - min(v)) / med[k] for k, v in samples.items()},
                     "change_over_tracked": med["change"] / med["tracked"], "change_over_tiled": med["change"] / med["tiled"]}
        chg.close()
        for t in trks.values():
            t.close()
    det.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "change_bench.json"))
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    args = ap.parse_args()
    if args.trace_child:
        trace_child(args)
        return
    res = {"tool": "tools/change_bench.py", "hbm_peak_bytes_per_second": HBM_PEAK,
           "pending": ["the plain, tiled, region and tracked-region calls and bench.py through the parent commit's library in alternation"]}
    res["schedules"] = schedules(args)
    if args.no_trace:
        res["pending"].append("the kernels alone (--no-trace)")
    else:
        try:
            res["kernels"] = kernel_times_from_trace(args)
        except Exception as e:                       # the file still records what was measured
            res["pending"].append("the kernels alone: " + str(e)[-400:])
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
