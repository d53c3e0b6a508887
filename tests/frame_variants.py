"""Photometric variants of the contract frames: the parity tests off the mid-grey happy path.

Every contract frame of tests/test_gpu_parity.py comes from retinaface_amd/frames.py:synth_frames -- a mid-grey canvas, N(0, 8) noise
and fixture faces at their native brightness, the same kind of frame the int8 calibration and stem2's DC-centring constants (weights.h:
the response to a flat frame of 128) were tuned on.  The variants below move the whole frame (faces included) off that band: darker,
brighter, gamma-bent, low and high contrast, a black or white canvas, a photo background and a uniform-noise canvas.  Each one is
synth_frames(448, 448, ...) on the held-out faces [1, 3, 5] (so the fp16 and int8 tests share frames and oracle results) with its own
canvas / background, a per-pixel transform applied after the faces are pasted (round half to even, clipped to 0..255), and its own config
number, so tests/oracle_cache.py's frame keys stay unique.  The fp32 oracle's results on the first FRAMES frames of every variant are
minted into tests/golden/contract_oracle_variants.npz (tools/make_contract_golden.py --variants)."""
from typing import Callable, Dict, List, NamedTuple, Optional

import numpy as np

HW = (448, 448)
FACES = [1, 3, 5]
FRAMES = 16                   # per variant (both models see the same frames)


def _lut(fn) -> Callable[[np.ndarray], np.ndarray]:
    x = np.arange(256, dtype=np.float64)
    table = np.clip(np.rint(fn(x)), 0, 255).astype(np.uint8)
    return lambda img: table[img]


class Variant(NamedTuple):
    config: int
    canvas: float
    background: Optional[str]
    transform: Optional[Callable[[np.ndarray], np.ndarray]]


VARIANTS: Dict[str, Variant] = {
    "dark": Variant(700, 128, None, _lut(lambda x: 0.4 * x)),
    "bright": Variant(701, 128, None, _lut(lambda x: 1.6 * x)),
    "gamma05": Variant(702, 128, None, _lut(lambda x: 255.0 * (x / 255.0) ** 0.5)),
    "gamma20": Variant(703, 128, None, _lut(lambda x: 255.0 * (x / 255.0) ** 2.0)),
    "lowcon": Variant(704, 128, None, _lut(lambda x: 128.0 + 0.4 * (x - 128.0))),
    "highcon": Variant(705, 128, None, _lut(lambda x: 128.0 + 1.8 * (x - 128.0))),
    "black": Variant(706, 0, None, None),
    "white": Variant(707, 255, None, None),
    "photo": Variant(708, 128, "photo", None),
    "noise": Variant(709, 128, "uniform", None),
    # stress: the uniform-noise canvas at contrast x3.  None of the ten variants above puts 0.1 % of a depthwise intermediate's quanta
    # at the int8 top code (tools/int8_variant_floors.py: at most 0.08 %, `noise`); this one does (0.4-0.6 % of relu3, 0.11-0.15 % of
    # relu4), so the int8 bit-exact test exercises the saturating epilogues (tests/test_int8_oracle.py asserts that it still does)
    "noise3": Variant(710, 128, "uniform", _lut(lambda x: 128.0 + 3.0 * (x - 128.0))),
}
NAMES = tuple(n for n in VARIANTS if n != "noise3")       # the photometric set (fp16 contract, per-layer checks)
STRESS = ("noise3",)                                       # int8 saturation stress (int8 tests only)
ALL = NAMES + STRESS


def variant_frames(name: str, n: int = FRAMES, hw=HW) -> List[np.ndarray]:
    """The first n frames of variant `name` at net size hw (BGR uint8, C-contiguous)."""
    from retinaface_amd.frames import synth_frames
    v = VARIANTS[name]
    frames = synth_frames(hw[0], hw[1], n, config=v.config, faces=FACES, canvas=v.canvas, background=v.background)
    return [np.ascontiguousarray(v.transform(f)) if v.transform is not None else f for f in frames]


def frame_key(stem: str, name: str, i: int, hw=HW) -> str:
    """tests/oracle_cache.py key of frame i of a variant (the variant's config number keeps it apart from every plain frame's)."""
    import oracle_cache
    return oracle_cache.frame_key(stem, hw, VARIANTS[name].config, FACES, i)
