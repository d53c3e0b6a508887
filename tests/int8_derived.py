"""Derived calibration tables and one derived weight set for the int8 engine's parity tests (numpy only, no GPU).

The int8 engine's bar is bit-exactness against oracle/int8_forward.py on ANY weights and ANY table, so inputs nobody has measured need
no tolerance -- they only have to reach the branches the shipped models leave cold.  The shipped tables carry 25 % head-room, so the top
clamp of every requantising epilogue is (almost) never reached, and no shipped convolution has an all-zero weight row.  Everything here
is derived at run time from a `NetSpec` as `oracle.caffe_io.read_rfw` returns it; nothing is stored.

Tables (`derive(net, name)`), each from the model's OWN shipped table.  Factors are powers of two applied in float32, hence exact:

  pc_half     every line x 0.5                       per-channel path; every tensor reaches its top code at 352 x 608
  pc_quarter  every line x 0.25                      deeper saturation; the float front end's clamp is reached by a wide margin
  pc_coarse   every line x 4                         the low end: nothing saturates, few distinct quanta
  pc_ragged   each line x a seeded choice of {0.25, 0.5, 1, 2}: neighbouring channels clamp differently, and the per-channel max-merge
              of the three tensors of each FPN add sees scales that really differ
  pt_quarter  only the lines without '#', x 0.25     per-tensor path (scalar ratios in the fused upsample + add, fp32 blend)
  pt_eighth   only the lines without '#', x 0.125    per-tensor path, > 256 candidates at threshold 0.02 (int8-tied scores)

Weight set `degenerate` (shipped table): all-zero weight rows in five dense convolutions, all-zero taps in three depthwise channels, and
on one pointwise convolution's BN-scale two channels with beta = 1e4 (saturated everywhere) and two with negated gamma.  Nothing before
`mobilenet0_conv5_fwd` changes: the engine's float front end may run through `relu4`, and it is the pinned input of the parity test.

Every derivation returns a copy with `int8_qweights = {}`: calibrated weights belong to the grid of the table (and the weights) they
were chosen under.
"""
from __future__ import annotations

import copy
import struct
import zlib
from typing import Dict

import numpy as np

F32 = np.float32
SEED = 20240517

TABLES = ("pc_half", "pc_quarter", "pc_coarse", "pc_ragged", "pt_quarter", "pt_eighth")
WEIGHT_SETS = ("degenerate",)
ALL = TABLES + WEIGHT_SETS

_FACTOR = {"pc_half": 0.5, "pc_quarter": 0.25, "pc_coarse": 4.0, "pt_quarter": 0.25, "pt_eighth": 0.125}
RAGGED_FACTORS = (0.25, 0.5, 1.0, 2.0)

# `degenerate`: (layer, how many output channels lose their whole weight row)
ZERO_ROWS = (("mobilenet0_conv8_fwd", 3), ("rf_c2_lateral", 3), ("rf_c1_aggr", 3), ("rf_c3_det_context_conv3_2", 2),
             ("face_rpn_bbox_pred_stride16", 1))
ZERO_TAPS = ("mobilenet0_conv9_fwd", 3)                 # depthwise: three channels with nine zero taps
BN_EDGES = "mobilenet0_conv12_fwd"                      # pointwise: beta = 1e4 on two channels, gamma negated on two others
BETA_HUGE = F32(1e4)


def _scaled(v: float, f: float) -> float:
    return float(F32(v) * F32(f))          # a power of two times a float32: exact (no table value is near the subnormals)


def derive_table(scales: Dict[str, float], name: str) -> Dict[str, float]:
    """The derived table `name` of a shipped per-channel table (file order kept)."""
    if name not in TABLES:
        raise KeyError(name)
    if name.startswith("pt_"):
        return {k: _scaled(v, _FACTOR[name]) for k, v in scales.items() if "#" not in k}
    if name == "pc_ragged":
        rng = np.random.default_rng(SEED)
        pick = rng.integers(0, len(RAGGED_FACTORS), len(scales))
        return {k: _scaled(v, RAGGED_FACTORS[int(p)]) for (k, v), p in zip(scales.items(), pick)}
    return {k: _scaled(v, _FACTOR[name]) for k, v in scales.items()}


def write_table(scales: Dict[str, float], path: str) -> None:
    """The reference's calibration-cache text format, as tools/calibrate_int8.py writes it: the `TRT-...` header, then
    `name: <big-endian float32 hex>` lines."""
    with open(path, "w") as f:
        f.write("TRT-5102-EntropyCalibration2\n")
        for k, v in scales.items():
            f.write(f"{k}: {struct.pack('>f', F32(v)).hex()}\n")


def _bn_scale_of(net, conv: str):
    """the Scale layer behind the BatchNorm that consumes `conv`'s top"""
    top = net.layer(conv).tops[0]
    names = [l.name for l in net.layers]
    for l in net.layers[names.index(conv) + 1:]:
        if l.type == "BatchNorm" and l.bottoms and l.bottoms[0] == top:
            return net.layer(l.name + "_scale")
    raise KeyError(f"no BatchNorm behind '{conv}'")


def _channels(layer: str, cout: int, n: int) -> np.ndarray:
    """n distinct seeded channel indices of a layer with `cout` outputs (valid for any model that has the layer)"""
    rng = np.random.default_rng([SEED, zlib.crc32(layer.encode())])
    return np.sort(rng.choice(cout, n, replace=False))


def degenerate_edits(net) -> Dict[str, np.ndarray]:
    """What `degenerate` changes: layer (with a `:zero` / `:beta` / `:gamma` tag) -> the output channels it touches."""
    ed = {}
    for name, n in ZERO_ROWS + (ZERO_TAPS,):
        ed[name + ":zero"] = _channels(name, net.layer(name).blobs[0].shape[0], n)
    four = _channels(BN_EDGES, net.layer(BN_EDGES).blobs[0].shape[0], 4)
    ed[BN_EDGES + ":beta"], ed[BN_EDGES + ":gamma"] = four[:2], four[2:]
    return ed


def derive(net, name: str):
    """A copy of `net` (a NetSpec) under the derived set `name`, without calibrated weights."""
    if name in TABLES:
        out = copy.copy(net)                       # the layers are shared and stay untouched
        out.int8_scales = derive_table(net.int8_scales, name)
        out.int8_qweights = {}
        return out
    if name != "degenerate":
        raise KeyError(name)
    out = copy.deepcopy(net)
    out.int8_qweights = {}
    for key, ch in degenerate_edits(out).items():
        layer, what = key.split(":")
        if what == "zero":
            out.layer(layer).blobs[0][ch] = 0
            continue
        sl = _bn_scale_of(out, layer)
        if what == "beta":
            assert sl.scale_bias
            sl.blobs[1].reshape(-1)[ch] = BETA_HUGE
        else:
            sl.blobs[0].reshape(-1)[ch] *= F32(-1)
    return out
