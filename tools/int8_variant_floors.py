#!/usr/bin/env python3
"""The int8 arithmetic's distance to the fp32 oracle on the photometric variants (tests/frame_variants.py), measured on the CPU -- the
floors of tests/test_gpu_parity.py::test_int8_on_photometric_variants -- and how often each variant drives an int8 epilogue into its top
clamp (the saturation coverage tests/test_int8_oracle.py asserts).

Per frame: the fp32 oracle's front end (mobilenet0_relu2_fwd, where the int8 engine's float stem hands over) quantised with the
calibration scale, continued with oracle/int8_forward.py, decoded + NMS'd with the oracle's plain-C post-processing, and matched against
the fp32 oracle's detections with tests/int8_contract.py.  No GPU:
    python tools/int8_variant_floors.py [--frames 16] [--out floors.json]"""
import argparse
import json
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frame_variants as fv                                      # noqa: E402
import oracle_cache                                              # noqa: E402
from int8_contract import frame_rows, summarize                  # noqa: E402
from oracle import build as obuild                               # noqa: E402
from oracle.caffe_forward import HEAD_STRIDES, head_names        # noqa: E402
from oracle.caffe_io import read_rfw                             # noqa: E402
from oracle.int8_forward import Int8Net                          # noqa: E402
from oracle.pipeline import OracleDetector                       # noqa: E402
from oracle.retinaface_post import preprocess_trt_identity       # noqa: E402

START = "mobilenet0_relu2_fwd"           # the int8 engine's first int8 activation (its float stem ends with block 0)
Det = namedtuple("Det", "score rect anchor_index")


def int8_acts(q: Int8Net, od: OracleDetector, frame: np.ndarray, hw=fv.HW):
    """every int8 activation of the integer oracle continued from the quantised fp32 front end (+ '__heads__')"""
    blobs = od.forward(preprocess_trt_identity(frame, hw[0], hw[1]), keep_all=True)
    return q.forward_from(START, q.quantise_blob(START, blobs[START][0].transpose(1, 2, 0)))


def top_fractions(acts) -> dict:
    """tensor -> fraction of its quanta at the top code 127 (depthwise intermediates are stored as q - 128: 127 there is 255)"""
    return {n: float((a == 127).mean()) for n, a in acts.items() if n not in ("__heads__", START)}


def is_depthwise(name: str) -> bool:
    return name.startswith("mobilenet0_relu") and int(name[len("mobilenet0_relu"):].split("_")[0]) % 2 == 1


def int8_detections(acts, hw=fv.HW, thr=0.5):
    heads = acts["__heads__"]
    _, _, kept, kidx = obuild.decode_nms([heads[n] for s in HEAD_STRIDES for n in head_names(s)], hw[0], hw[1], thr, 0.4)
    return [Det(float(r[0]), tuple(float(v) for v in r[1:5]), int(a)) for r, a in zip(kept, kidx)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=fv.FRAMES)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    res = {}
    for stem in ("mnet-deconv-0517", "mnet25"):
        net = read_rfw(os.path.join(ROOT, "assets", stem + ".rfw"))
        od, q = OracleDetector(net), Int8Net(net)
        for name in fv.ALL:
            frames, top = [], {}
            for i, f in enumerate(fv.variant_frames(name, args.frames)):
                acts = int8_acts(q, od, f)
                for n, v in top_fractions(acts).items():
                    top[n] = max(top.get(n, 0.0), v)
                got = int8_detections(acts)
                ref = oracle_cache.detect(od, stem, f, fv.HW, fv.VARIANTS[name].config, fv.FACES, i)
                frames.append(dict(same_count=len(got) == len(ref.detections), rows=frame_rows(got, ref)))
            s = summarize(frames)
            blk = max((v, n) for n, v in top.items() if not is_depthwise(n))
            dw = max((v, n) for n, v in top.items() if is_depthwise(n))
            s.update(top_block=blk, top_depthwise=dw)
            res.setdefault(stem, {})[name] = s
            print(f"{stem:16s} {name:8s} same count {s['same_count']}/{s['frames']} unmatched {s['unmatched']}  same-anchor IoU worst "
                  f"{s['anchor_iou_worst']:.4f}  agreement {s['anchor_agreement']:.3f}  | at 127: block {blk[0]:.4f} ({blk[1]})  "
                  f"depthwise {dw[0]:.4f} ({dw[1]})", flush=True)
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
