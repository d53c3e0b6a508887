#!/usr/bin/env python3
"""GPU tool: what region detection costs next to the tiled call and the plain call (DESIGN.md "Region detection"; writes
profiles/roi_bench.json).

Two workloads on the fp16 engine (mnet25, net 448), device-resident frames:
  8x1280x896    the base frame and seven mirrored / flipped / shifted copies
  2x3840x2160   the base frame tiled 3 x 3 and cut to 4K, and its mirror
The regions of every frame are its own faces as the TILED call finds them, grown by a quarter (rf_roi_from_faces), packed at the default
grid 4.  Three calls are timed in alternation, each in windows of at least --min-seconds after warm-up, median of three windows with the
spread beside it:
  roi      rf_detect_roi_batch_device
  tiled    rf_detect_tiled_batch_device
  plain    rf_detect_batch_device (the frames shrunk to the net)
and the schedule "a tiled key frame, then three region frames" is derived per frame set: (tiled + 3 roi) / 4.
The kernels alone come from a rocprofv3 kernel trace of a child process (--trace-child): the roi_atlas_kernel dispatches of the two
region calls, and -- for the kernel's cost per output byte at each level -- rf_roi_atlas_device over sixteen 448 x 448 views of one cell
(grid 1) whose regions are sized to land on one level each, next to zoom_tile_kernel (sixteen 448 x 448 windows at 2x) and
dewarp_views_kernel (sixteen 448 x 448 views) over the same output bytes.
No speed-up is promised: the file records what was measured.

usage: python tools/roi_bench.py [--out profiles/roi_bench.json] [--min-seconds 0.5] [--no-trace]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from align_bench import window  # noqa: E402

NET, NMS = 448, 0.4
TRACE_WARM, TRACE_CALLS = 2, 10
LEVEL_SIDES = {2: 112, 1: 224, 0: 448, -1: 896, -2: 1792}          # a square region of this side fills a 448 cell at that level


def frame_sets():
    from retinaface_amd.frames import padded_base_frame
    base = padded_base_frame()
    hd = [base, base[:, ::-1], base[::-1], base[::-1, ::-1], np.roll(base, 37, 1), np.roll(base, -53, 1), np.roll(base[:, ::-1], 91, 1), np.roll(base, 211, 1)]
    big = np.tile(base, (3, 3, 1))[:2160, :3840]
    return {"8x1280x896": [np.ascontiguousarray(f) for f in hd], "2x3840x2160": [np.ascontiguousarray(big), np.ascontiguousarray(big[:, ::-1])]}


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
            ptrs, rows, cols = [d.data_ptr() for d in dev], [f.shape[0] for f in frames], [f.shape[1] for f in frames]
            tiled = self.det.detect_tiled_device(ptrs, rows, cols, 0.5)
            rois = [retinaface_amd.rois_from_faces(t)[:256] for t in tiled]
            self.sets[name] = dict(dev=dev, ptrs=ptrs, rows=rows, cols=cols, rois=rois, tiled_faces=[len(t) for t in tiled])

    def roi(self, s):
        return self.det.detect_rois_device(s["ptrs"], s["rows"], s["cols"], s["rois"], 0.5)

    def tiled(self, s):
        return self.det.detect_tiled_device(s["ptrs"], s["rows"], s["cols"], 0.5)

    def plain(self, s):
        return self.det.detect_device(s["ptrs"], s["rows"], s["cols"], 0.5)

    def level_views(self, level):
        """sixteen views of one cell each, every region at `level`: 16 x 448 x 448 x 3 output bytes"""
        s = self.sets["2x3840x2160"]
        side = LEVEL_SIDES[level]
        rois = [(100 + 190 * k, 60 + 17 * k, side, side) for k in range(16)]
        if not hasattr(self, "scratch"):
            self.scratch = self.torch.zeros((16 * NET * NET * 3,), dtype=self.torch.uint8, device="cuda")
        self.det.roi_atlas_device(s["ptrs"][0], 2160, 3840, rois, self.scratch.data_ptr(), NET, NET, grid=1, max_zoom=4)

    def zoom16(self):
        s = self.sets["2x3840x2160"]
        for k in range(16):
            self.det.zoom_device(s["ptrs"][0], 2160, 3840, 2, 200 + 380 * k, 120 + 34 * k, NET, NET, self.scratch.data_ptr() + k * NET * NET * 3)

    def dewarp16(self):
        if not hasattr(self, "dw"):
            sp = self.rfa.dewarp_spec(f=0.98 * 1024 / np.pi, cx=511.5, cy=511.5, ring=16, pitch=55.0, hfov=60.0)
            self.dw = self.det.dewarper(1024, 1024, spec=sp)
            self.fish = self.torch.from_numpy(np.ascontiguousarray(frame_sets()["2x3840x2160"][0][:1024, :1024])).cuda()
        for v in range(16):
            self.det.dewarp_device(self.dw, v, self.fish.data_ptr(), self.scratch.data_ptr() + v * NET * NET * 3)


def measure(args):
    w = Workload(args.batch)
    out = {}
    for name, s in w.sets.items():
        calls = {"roi": lambda: w.roi(s), "tiled": lambda: w.tiled(s), "plain": lambda: w.plain(s)}
        for _ in range(3):                      # warm-up: every launch size, graph capture, scratch allocation
            for fn in calls.values():
                fn()
        found = {k: [len(x) for x in fn()] for k, fn in calls.items()}
        samples = {k: [] for k in calls}
        for _ in range(3):                      # alternate, so drift hits all alike
            for k, fn in calls.items():
                samples[k].append(window(fn, args.min_seconds))
        med = {k: statistics.median(v) for k, v in samples.items()}
        gg = 16
        out[name] = {
            "regions_per_frame": [len(r) for r in s["rois"]], "roi_passes": sum(-(-len(r) // gg) for r in s["rois"]),
            "tiled_passes": sum(len(w.rfa.tile_plan(r, c, NET, NET)) for r, c in zip(s["rows"], s["cols"])),
            "faces_per_frame": found,
            "call_ms": {k: med[k] * 1e3 for k in med},
            "call_ms_samples": {k: [x * 1e3 for x in v] for k, v in samples.items()},
            "relative_spread": {k: (max(v) - min(v)) / med[k] for k, v in samples.items()},
            "roi_over_tiled": med["roi"] / med["tiled"], "roi_over_plain": med["roi"] / med["plain"],
            "schedule_key_plus_three_region_frames_ms_per_frame_set": (med["tiled"] + 3 * med["roi"]) / 4 * 1e3,
        }
    w.det.close()
    return out


def trace_child(args):
    w = Workload(args.batch)
    for name in ("8x1280x896", "2x3840x2160"):
        for _ in range(TRACE_WARM + TRACE_CALLS):
            w.roi(w.sets[name])
    for level in (2, 1, 0, -1, -2):
        for _ in range(TRACE_WARM + TRACE_CALLS):
            w.level_views(level)
    for _ in range(TRACE_WARM + TRACE_CALLS):
        w.zoom16()
    for _ in range(TRACE_WARM + TRACE_CALLS):
        w.dewarp16()
    w.det.close()


def kernel_times_from_trace(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "roi", "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--batch", str(args.batch)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed:\n" + r.stderr[-2000:])
        rec = {"roi_atlas": [], "zoom_tile": [], "dewarp_views": []}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for key in rec:
                    if key in row.get("Kernel_Name", ""):
                        rec[key].append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-9))
    atlas = [d for _, d in sorted(rec["roi_atlas"])]
    zoom = [d for _, d in sorted(rec["zoom_tile"])]
    dew = [d for _, d in sorted(rec["dewarp_views"])]
    per = TRACE_WARM + TRACE_CALLS
    if len(atlas) != 7 * per or len(zoom) < 16 * per or len(dew) != 16 * per:
        raise RuntimeError(f"unexpected dispatch counts in the kernel trace: atlas {len(atlas)}, zoom {len(zoom)}, dewarp {len(dew)}")
    us = lambda v: {"median_us": statistics.median(v) * 1e6, "min_us": min(v) * 1e6, "max_us": max(v) * 1e6, "dispatches": len(v)}  # noqa: E731
    out_bytes = 16 * NET * NET * 3
    res = {"atlas_launch_of_the_call": {"8x1280x896": us(atlas[TRACE_WARM:per]), "2x3840x2160": us(atlas[per + TRACE_WARM:2 * per])},
           "output_bytes_of_sixteen_views": out_bytes, "ns_per_output_byte": {}}
    for i, level in enumerate((2, 1, 0, -1, -2)):
        v = atlas[(2 + i) * per + TRACE_WARM:(3 + i) * per]
        res["ns_per_output_byte"]["roi_atlas_level_%+d" % level] = statistics.median(v) / out_bytes * 1e9
    zoom = zoom[-16 * per:]
    z16 = [sum(zoom[16 * i:16 * i + 16]) for i in range(TRACE_WARM, per)]
    d16 = [sum(dew[16 * i:16 * i + 16]) for i in range(TRACE_WARM, per)]
    res["ns_per_output_byte"]["zoom_tile_2x_sixteen_launches"] = statistics.median(z16) / out_bytes * 1e9
    res["ns_per_output_byte"]["dewarp_views_sixteen_launches"] = statistics.median(d16) / out_bytes * 1e9
    n = res["ns_per_output_byte"]
    res["quarter_over_one"] = n["roi_atlas_level_-2"] / n["roi_atlas_level_+0"]
    return res


def ab_child(lib_path, min_seconds):
    """the plain and the tiled call over the 8x1280x896 set through a library given by path, bound by hand: a library of the parent
    commit lacks the newer symbols"""
    import ctypes as C
    import torch
    from retinaface_amd._lib import rf_face, rf_options, rf_tile_spec
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
    lib.rf_destroy.argtypes = [C.c_void_p]
    assert lib.rf_create(os.path.join(ROOT, "assets").encode(), b"net3", NMS, C.byref(o), C.byref(h)) == 0
    ptrs = (C.c_void_p * n)(*[f.data_ptr() for f in dev])
    r, c, s = (C.c_int * n)(*[896] * n), (C.c_int * n)(*[1280] * n), (C.c_int * n)(*[3840] * n)
    out, counts = (rf_face * (n * cap))(), (C.c_int * n)()

    def plain():
        assert lib.rf_detect_batch_device(h, ptrs, r, c, s, n, 0.5, out, cap, counts) == 0

    def tiled():
        assert lib.rf_detect_tiled_batch_device(h, ptrs, r, c, s, n, 0.5, None, out, cap, counts, None) in (0, -6)
    for _ in range(10):
        plain()
        tiled()
    res = {"plain": [], "tiled": []}
    for _ in range(3):
        res["plain"].append(window(plain, min_seconds) * 1e3)
        res["tiled"].append(window(tiled, min_seconds) * 1e3)
    lib.rf_destroy(h)
    print(json.dumps(res))


def ab(args):
    import retinaface_amd
    libs = (("parent", args.parent_lib), ("this", retinaface_amd.lib_path()))
    samples = {name: {"plain": [], "tiled": []} for name, _ in libs}
    for _ in range(3):                          # alternating child processes, one library each
        for name, path in libs:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", path, "--min-seconds", str(args.min_seconds)],
                                   capture_output=True, text=True, timeout=300)
            if child.returncode != 0:
                raise RuntimeError("the child of the %s library failed:\n%s" % (name, child.stderr[-2000:]))
            got = json.loads(child.stdout.strip().splitlines()[-1])
            for k in got:
                samples[name][k] += got[k]
    doc = {"tool": "tools/roi_bench.py --parent-lib", "calls": "rf_detect_batch_device and rf_detect_tiled_batch_device, 8 frames of 1280x896, fp16 mnet25",
           "call_ms_samples": samples}
    for k in ("plain", "tiled"):
        p, t = samples["parent"][k], samples["this"][k]
        doc[k] = {"parent_median_ms": statistics.median(p), "this_median_ms": statistics.median(t),
                  "this_over_parent": statistics.median(t) / statistics.median(p),
                  "parent_spread": (max(p) - min(p)) / statistics.median(p), "this_spread": (max(t) - min(t)) / statistics.median(t),
                  "medians_within_the_runs_own_spread": abs(statistics.median(t) - statistics.median(p)) <= max(max(p) - min(p), max(t) - min(t))}
    with open(args.ab_out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_bench.json"))
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "roi_bench_ab.json"))
    ap.add_argument("--parent-lib", default=None, help="libretinaface_amd.so built from the parent commit: its plain and tiled calls are timed against this one's")
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
    res = {"tool": "tools/roi_bench.py", "net": "448x448", "precision": "fp16", "model": "mnet25", "max_batch": args.batch,
           "window_seconds": args.min_seconds, "windows": 3, "workloads": measure(args)}
    if not args.no_trace:
        res["kernels"] = kernel_times_from_trace(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
