#!/usr/bin/env python3
"""Freeze the zoom-pyramid golden from the CPU oracle into tests/golden/pyramid_mosaic.npz (run where the oracle runs).

The frame is tests/pyramid_ref.mosaic: the padded base frame averaged over 8 x 8 blocks and placed 3 x 3, 336 x 480 with 54 faces of
11 to 14 px.  Per stem the nine passes of the default pyramid plan (net 448 x 448: two 1x tiles, the full-frame pass, six 2x zoom
tiles) go through the oracle and tests/pyramid_ref.merge at NMS 0.4.

The threshold is chosen here, not in the test: the first of 0.50, 0.49, 0.51, 0.48 ... at which the oracle's merge still gives 54 faces
and NO anchor of any pass has its foreground probability inside the fp16 score-noise band around the threshold (tools/make_golden.py
band(): |p - thr| <= 2e-3, the derivation of tests/golden/threshold_bands.npz) -- so an fp16 engine whose scores are within that noise of
the oracle's sees the same candidates in every pass.

  <stem>/threshold   the chosen threshold (float32)
  <stem>/faces       the oracle's merged faces, (54, 15) float32 in merge order
  <stem>/votes, <stem>/src_pass
  <stem>/scores      the scores of all pass results, concatenated in plan order (float32); <stem>/pass_counts: how many per pass
  <stem>/in_band     anchors inside the band over all passes at that threshold (0 when a clean threshold exists)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pyramid_ref as pr  # noqa: E402
from make_golden import band  # noqa: E402
from oracle.caffe_io import read_rfw  # noqa: E402
from oracle.pipeline import OracleDetector  # noqa: E402
from retinaface_amd.frames import padded_base_frame  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pyramid_mosaic.npz")
NET = (448, 448)
NMS = 0.4
MD = 256
FACES = 54


def run(det, images, thr):
    results = [det.detect(im, thr, NMS, net_hw=NET) for im in images]
    passes = [r.rows() for r in results]
    merged = pr.merge(336, 480, passes, *NET, NMS, MD)
    return passes, merged, sum(band(r.heads, thr) for r in results)


def main():
    frame = pr.mosaic(padded_base_frame())
    assert frame.shape == (336, 480, 3)
    images = [np.ascontiguousarray(v) for v in pr.images(frame, pr.plan(336, 480, *NET))]
    assert len(images) == 9
    d = {}
    for stem in ("mnet-deconv-0517", "mnet25"):
        det = OracleDetector(read_rfw(os.path.join(ROOT, "assets", stem + ".rfw")))
        chosen = None
        tried = []
        for step in range(0, 41):
            for thr in ((0.5,) if step == 0 else (0.5 - step / 100, 0.5 + step / 100)):
                passes, merged, inside = run(det, images, thr)
                tried.append((thr, merged[1], inside))
                if merged[1] == FACES and inside == 0:
                    chosen = (thr, passes, merged, inside)
                    break
            if chosen:
                break
        print(stem, "tried (threshold, merged faces, anchors in band):", tried)
        if not chosen:
            thr = 0.5
            passes, merged, inside = run(det, images, thr)
            chosen = (thr, passes, merged, inside)
            print(stem, "NO clean threshold: the golden is minted at 0.5 with", inside, "anchors in the band")
        thr, passes, merged, inside = chosen
        d[stem + "/threshold"] = np.float32(thr)
        d[stem + "/faces"] = merged[0]
        d[stem + "/votes"] = merged[2]
        d[stem + "/src_pass"] = merged[3]
        d[stem + "/scores"] = np.concatenate([p[:, 0] for p in passes]).astype(np.float32)
        d[stem + "/pass_counts"] = np.array([len(p) for p in passes], np.int32)
        d[stem + "/in_band"] = np.int32(inside)
        print(stem, "threshold", thr, "faces", merged[1], "pass counts", [len(p) for p in passes], "in band", inside)
    np.savez_compressed(OUT, **d)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
