#!/usr/bin/env python3
"""Mint tests/golden/contract_oracle_1280x896.npz: the fp32 oracle's results on the 1280 x 896 frames of the fp16 and int8 contracts
(tests/test_gpu_parity.py, tests/int8_contract.py) -- see tests/oracle_cache.py.  Runs the CPU oracle only (no GPU, no /root/reference):
    python tools/make_contract_golden.py            (~3 minutes on 8 cores)
    python tools/make_contract_golden.py --variants (tests/golden/contract_oracle_variants.npz: the photometric variants of
                                                     tests/frame_variants.py, 448 x 448, FRAMES per variant per model; ~1 minute)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_cache                                              # noqa: E402
from int8_contract import HELD_OUT_FACES, PLAN                   # noqa: E402
from oracle.caffe_io import read_rfw                              # noqa: E402
from oracle.pipeline import OracleDetector                        # noqa: E402
from retinaface_amd.frames import synth_frames                    # noqa: E402


def variants():
    import frame_variants as fv
    out = {}
    t0 = time.time()
    for stem in ("mnet-deconv-0517", "mnet25"):
        od = OracleDetector(read_rfw(os.path.join(ROOT, "assets", stem + ".rfw")))
        for name in fv.ALL:
            for i, f in enumerate(fv.variant_frames(name)):
                ref = od.detect(f, 0.5, 0.4, net_hw=fv.HW)
                out[f"{fv.frame_key(stem, name, i)}/blob"] = oracle_cache.pack_blob(oracle_cache.pack(ref, f))
        print(f"{stem}: {len(out)} frames so far, {time.time() - t0:.0f} s", flush=True)
    np.savez_compressed(oracle_cache.GOLDEN_VARIANTS, **out)
    print("wrote", oracle_cache.GOLDEN_VARIANTS, os.path.getsize(oracle_cache.GOLDEN_VARIANTS), "bytes,", len(out), "frames")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", action="store_true", help="mint the photometric variants' file instead of the 1280 x 896 one")
    if ap.parse_args().variants:
        return variants()
    out = {}
    t0 = time.time()
    for stem in ("mnet-deconv-0517", "mnet25"):
        od = OracleDetector(read_rfw(os.path.join(ROOT, "assets", stem + ".rfw")))
        for hw, batches in PLAN:
            if hw[0] * hw[1] <= 512 * 512:
                continue                                         # small frames stay live
            for faces in (None, HELD_OUT_FACES):                 # the fp16 contract's frames / the int8 contract's (held-out faces)
                for nb, cfg in batches:
                    for i, f in enumerate(synth_frames(hw[0], hw[1], nb, config=cfg, faces=faces)):
                        ref = od.detect(f, 0.5, 0.4, net_hw=hw)
                        key = oracle_cache.frame_key(stem, hw, cfg, faces, i)
                        for k, v in oracle_cache.pack(ref, f).items():
                            out[f"{key}/{k}"] = v
        print(f"{stem}: {len(out) // 6} frames so far, {time.time() - t0:.0f} s", flush=True)
    np.savez_compressed(oracle_cache.GOLDEN, **out)
    print("wrote", oracle_cache.GOLDEN, os.path.getsize(oracle_cache.GOLDEN), "bytes,", len(out) // 6, "frames")


if __name__ == "__main__":
    main()
