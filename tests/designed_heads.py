"""Designed head outputs for the decode + NMS tests (numpy only, no GPU): pass-through ("wire") weight sets and painted frames.

decode_anchor, the tail of head_kernel and nms_kernel have only ever seen the head blobs two trained networks emit for natural frames, so
no candidate count ever sat on a boundary and no two anchors ever tied.  There is no API that injects head blobs; the heads are driven
through the weights and the frame instead.  Everything here is derived at run time from a `NetSpec` as `oracle.caffe_io.read_rfw` returns
it (the way tests/int8_derived.py derives its sets); nothing is stored.

The wire set (`wire_net`).  Every Convolution / Deconvolution weight and bias is 0, except:
  mobilenet0_conv0_fwd      output channel c reads ONE tap of ONE colour: wire c = (colour, dy, dx) of WIRES, w[c, colour, 1 + dy, 1 + dx] = 1
                            (dy, dx in {0, 1}: no wire reads padding)
  depthwise convs           centre tap 1
  dense convs of the trunk  channel c -> channel c (c = 0..7) at the centre tap: the pointwise convs, the three laterals / rf_c1_red_conv, the
                            two aggr convs and the three det_conv1 -- except on the stride-16 path, see below
  context convs             stay 0
  upsampling deconvolutions keep their shipped weights: the engine fuses them as THE fixed bilinear kernel and refuses any other.  What they
                            add to the next finer stride must therefore miss the wires there: rf_c2_lateral writes channels 8..15,
                            rf_c2_aggr reads those and writes 16..23, rf_c2_det_conv1 reads those and writes 0..7; the upsampled stride-32
                            lateral (channels 0..7) and the upsampled rf_c2_aggr (16..23) meet weights that are 0
  every BatchNorm mean 0, variance 1, factor 1; every Scale gamma 1, beta 0
Channel c of rf_c{1,2,3}_det_concat_relu at cell (i, j) of stride s is then the frame's pixel (s i + dy, s j + dx), colour as wired, times
1 / sqrt(1 + eps) per BatchNorm on the way; all other channels are exactly 0.  A painted 0 arrives as an exact 0 on every stride.

The heads are 1 x 1 convs on that tensor; a head set (HEAD_SETS) writes them as bias + sum(weight * wire) per stride and anchor.  All sets
use the same wiring (anchor a of a cell, wires of that cell's pixel):
  foreground logit   -0.25 * GATE_a + SC / 8 + SF / 4096      the gate is INVERTED: painted 0 = on (an exact 0 reaches the head, so equal
                                                              score wires give bit-equal logits on every stride), 255 = off (logit < -59)
  dw = dh            (SZ - SN) / 32                           0 -> the anchor's own size exactly (expf(0) = 1); -3 -> 0.8 px for the 16-px anchor
  dx, dy             +DX / 32, +DY / 32 for anchor 1; -DX / 32, -DY / 32 for anchor 0: both directions from two wires, 0 exact
  landmarks          from the bias alone (LMK), up to 6 anchor widths away: outside the frame for every border cell
  background logits  0;  a stride a set does not use has foreground bias -30
  `std`      stride 8 only (anchor 0: 32 px, anchor 1: 16 px): per-anchor gates make every candidate count reachable.  Anchor 0 has
             foreground bias 2^-13, half a step of SF: the two anchors of a cell read the same score wires and would tie otherwise
  `tied`     `std` without that bias: both anchors of a cell, and all cells painted alike, tie exactly
  `strides`  all three strides, foreground bias 1: a gate painted on a stride-32 cell's pixel opens the coincident cells of stride 16 and 8
             too, and with the score wires at 0 the logit is the bias on every stride (a nonzero wire would differ by the BatchNorms passed)

Candidates are read at threshold THR = 0.02 (logit -3.9): an open gate gives logit >= 0, a closed one <= -59, so the count is the number of
open gates in fp32 and fp16 alike (more than 3 logits of margin on either side).

Four anchors per cell ("net3a": ratios 1 and 1.5, anchors 2 and 3 of stride 8 are 26 x 40 and 13 x 20 px, the latter at fractional
coordinates).  conv0 has eight channels, hence eight wires: the A = 4 sets (HEAD_SETS4) spend four on gates and give up SF and SN --
wire 3 is GATE2, wire 7 is GATE3.  The heads of the net are widened first (net3a_models.widen_heads: shapes only, every weight is then
written here):
  foreground logit   bias_a - 0.25 * GATE_a + SC / 32         256 score levels over logits 0 .. 8; the anchors of a cell read the same SC and are
                                                              told apart by bias_a, a multiple of 1 / 128 (a quarter of a level): 1024 distinct logits
  dw, dh             SZ * DWW4[a], SZ * DHW4[a]               0 -> the anchor's own width AND height exactly
  dx, dy             DX * DXW4[a], DY * DYW4[a]               negative for anchors 0, 2, positive for anchors 1, 3
  landmarks          from the bias alone (LMK4[a] = LMK * (1 + a / 4)): x and y offsets differ, so a landmark y computed with the width
                     lands elsewhere
                     -- eight weights and ten biases per anchor, all different from those of the three other anchors of the cell
  `std4`     stride 8 only, foreground biases 3/128, 1/128, 0, 2/128 for anchors 0 .. 3: within a cell the order is 0, 3, 1, 2
  `tied4`    `std4` with all four biases 0: the four anchors of a cell tie exactly
  `strides4` all three strides, foreground bias 1 + the `std4` bias + one score level per stride (0, 1/32, 2/32: coincident cells read the
             same score pixel and must not tie): a gate painted on a stride-32 cell's pixel opens the coincident cells of stride 16 and 8; a
             gate on a stride-8 cell with an odd coordinate opens that cell alone

SCENARIOS is the table: name -> Scenario(net, heads, frame builder, condition).  `check(sc, cand, cidx, kept, kidx)` asserts a scenario's
condition on a restatement result (oracle.build.decode_nms), whoever produced the head blobs: a scenario that silently missed its regime
fails.  Tie conditions (`ties=True`) are only asserted where the caller says the blobs are fp32.
"""
from __future__ import annotations

import copy
from typing import Callable, Dict, NamedTuple, Optional, Tuple

import numpy as np

F32 = np.float32
R, G, B = 0, 1, 2                                             # the net's input planes (RGB); a BGR frame holds colour c at index 2 - c
WIRES = ((R, 0, 0), (G, 0, 0), (B, 0, 0), (R, 0, 1), (G, 0, 1), (B, 0, 1), (R, 1, 0), (G, 1, 0))
GATE0, GATE1, SC, SF, SZ, DX, DY, SN = range(8)               # what the head sets read from each wire
GATE = (GATE0, GATE1)
OFF = 255                                                     # a closed gate
THR = 0.02
NMS = 0.4
SMALL, LARGE = (128, 160), (384, 384)                         # stride-8 maps 16 x 20 (640 anchors) and 48 x 48 (4608 anchors)
STRIDES = (32, 16, 8)
ANCHOR_PX = {32: (512, 256), 16: (128, 64), 8: (32, 16)}
LMK = tuple(F32(v) for k in range(5) for v in ((k - 2) * 3.0, (2 - k) * 2.5))          # x0, y0, .. x4, y4 in anchor widths

# dense convs off the backbone: layer -> (first input channel, first output channel) of its eight wires
TRUNK_DENSE = {"rf_c3_lateral": (0, 0), "rf_c3_det_conv1": (0, 0), "rf_c2_lateral": (0, 8), "rf_c2_aggr": (8, 16), "rf_c2_det_conv1": (16, 0),
               "rf_c1_red_conv": (0, 0), "rf_c1_aggr": (0, 0), "rf_c1_det_conv1": (0, 0)}


def _anchor(a: int, bias: float = 0.0):
    sgn = F32(1 if a == 1 else -1)
    return dict(fg=(F32(bias), {GATE[a]: F32(-0.25), SC: F32(1 / 8), SF: F32(1 / 4096)}),
                dx=(F32(0), {DX: sgn / F32(32)}), dy=(F32(0), {DY: sgn / F32(32)}),
                dw=(F32(0), {SZ: F32(1 / 32), SN: F32(-1 / 32)}), dh=(F32(0), {SZ: F32(1 / 32), SN: F32(-1 / 32)}), lmk=LMK)


HEAD_SETS = {"std": {8: (_anchor(0, 2.0 ** -13), _anchor(1))},
             "tied": {8: (_anchor(0), _anchor(1))},
             "strides": {s: (_anchor(0, 1.0), _anchor(1, 1.0)) for s in STRIDES}}


# four anchors per cell: wires 3 (SF) and 7 (SN) become the gates of anchors 2 and 3
GATE2, GATE3 = SF, SN
GATE4 = (GATE0, GATE1, GATE2, GATE3)
RATIOS4 = (1.0, 1.5)                                          # "net3a"
FG_BIAS4 = tuple(F32(v / 128) for v in (3, 1, 0, 2))          # order within a cell: anchors 0, 3, 1, 2
STRIDE_BIAS4 = {32: F32(0), 16: F32(1 / 32), 8: F32(2 / 32)}  # `strides4`: coincident cells of the three strides read ONE score pixel; one level apart


# Every box and landmark row of a cell differs from every other: a kernel that took anchor a ^ 2's (or a ^ 1's) channels, or dy for dx, or
# dh for dw, decodes other numbers.  All dyadic, so a wire painted 0 still gives the anchor itself exactly.
DXW4 = tuple(F32(v) for v in (-1 / 32, 1 / 32, -1 / 64, 1 / 16))
DYW4 = tuple(F32(v) for v in (-1 / 64, 1 / 16, -1 / 32, 1 / 32))
DWW4 = tuple(F32(v) for v in (1 / 32, 3 / 128, 1 / 64, 5 / 128))
DHW4 = tuple(F32(v) for v in (3 / 128, 1 / 32, 5 / 128, 1 / 64))
LMK4 = tuple(tuple(F32(v * (1 + a / 4)) for v in LMK) for a in range(4))      # multiples of 1 / 8: products with 13 .. 512 stay exact


def _anchor4(a: int, bias: float):
    return dict(fg=(F32(bias), {GATE4[a]: F32(-0.25), SC: F32(1 / 32)}),
                dx=(F32(0), {DX: DXW4[a]}), dy=(F32(0), {DY: DYW4[a]}),
                dw=(F32(0), {SZ: DWW4[a]}), dh=(F32(0), {SZ: DHW4[a]}), lmk=LMK4[a])


HEAD_SETS4 = {"std4": {8: tuple(_anchor4(a, FG_BIAS4[a]) for a in range(4))},
              "tied4": {8: tuple(_anchor4(a, 0.0) for a in range(4))},
              "strides4": {s: tuple(_anchor4(a, 1.0 + STRIDE_BIAS4[s] + FG_BIAS4[a]) for a in range(4)) for s in STRIDES}}


def wire_net(net, heads: Optional[str] = None):
    """A copy of `net` (a NetSpec) under the wire set, without calibrated weights; `heads` names a head set (None: heads all 0).  A set of
    HEAD_SETS4 gets heads of four anchors per cell."""
    if heads in HEAD_SETS4:
        from net3a_models import widen_heads
        out = widen_heads(net)
    else:
        out = copy.deepcopy(net)
    out.int8_qweights = {}
    for l in out.layers:
        if l.type == "Convolution":
            for b in l.blobs:
                b[...] = 0
            w = l.blobs[0]
            k = l.kernel // 2
            if l.name == "mobilenet0_conv0_fwd":
                assert w.shape == (8, 3, 3, 3) and l.stride == 2 and l.pad == 1
                for c, (colour, dy, dx) in enumerate(WIRES):
                    w[c, colour, 1 + dy, 1 + dx] = 1
            elif l.group > 1:
                assert l.group == l.num_output and w.shape[1] == 1
                w[:, 0, k, k] = 1
            elif l.name.startswith("mobilenet0_conv") or l.name in TRUNK_DENSE:
                cin, cout = TRUNK_DENSE.get(l.name, (0, 0))
                for c in range(len(WIRES)):
                    w[cout + c, cin + c, k, k] = 1
        elif l.type == "BatchNorm":
            l.blobs[0][...] = 0
            l.blobs[1][...] = 1
            l.blobs[2][...] = 1
        elif l.type == "Scale":
            l.blobs[0][...] = 1
            if l.scale_bias:
                l.blobs[1][...] = 0
    if heads is not None:
        set_heads(out, HEAD_SETS4[heads] if heads in HEAD_SETS4 else HEAD_SETS[heads])
    return out


def set_heads(net, head_set) -> None:
    """Write a head set into the (zeroed) head convolutions of a wire net."""
    for s in STRIDES:
        cls, box, lmk = (net.layer(f"face_rpn_{n}_stride{s}") for n in ("cls_score", "bbox_pred", "landmark_pred"))
        na = cls.blobs[0].shape[0] // 2
        assert na in (2, 4) and box.blobs[0].shape[0] == 4 * na and lmk.blobs[0].shape[0] == 10 * na
        assert s not in head_set or len(head_set[s]) == na, (s, na)
        for a in range(na):
            spec = head_set[s][a] if s in head_set else None
            if spec is None:
                cls.blobs[1].reshape(-1)[na + a] = -30          # Reshape (2, -1): the na background maps first, then the foreground maps
                continue
            rows = [(cls, na + a, spec["fg"])] + [(box, a * 4 + c, spec[n]) for c, n in enumerate(("dx", "dy", "dw", "dh"))]
            for layer, ch, (bias, taps) in rows:
                layer.blobs[1].reshape(-1)[ch] = bias
                for wire, wt in taps.items():
                    layer.blobs[0][ch, wire, 0, 0] = wt
            lmk.blobs[1].reshape(-1)[a * 10:a * 10 + 10] = spec["lmk"]


def wire_view(frame: np.ndarray, stride: int, wire: int) -> np.ndarray:
    """The pixels wire `wire` reads at stride `stride`: a writable (h / stride, w / stride) view of a BGR frame."""
    colour, dy, dx = WIRES[wire]
    return frame[dy::stride, dx::stride, 2 - colour]


def paint(hw: Tuple[int, int], stride: int, wires: Dict[int, np.ndarray], gates=GATE) -> np.ndarray:
    """A BGR uint8 frame of size hw: every gate closed, every other wire 0, then `wires` {wire: uint8 array over the cells of `stride`}."""
    frame = np.zeros((hw[0], hw[1], 3), np.uint8)
    for g in gates:
        wire_view(frame, 8, g)[...] = OFF
    for wire, values in wires.items():
        v = wire_view(frame, stride, wire)
        v[...] = np.broadcast_to(np.asarray(values, np.uint8), v.shape)
    return frame


# ------------------------------------------------------------------------------------------------------------ frames
def _cells(hw, stride=8, interior=False):
    h, w = hw[0] // stride, hw[1] // stride
    m = 1 if interior else 0
    return [(i, j) for i in range(m, h - m) for j in range(m, w - m)]


def _slots(hw, n, interior=False):
    """The first n (anchor, i, j) of the stride-8 map: anchor 1 (16 px) over the cells, then anchor 0 (32 px)."""
    cells = _cells(hw, 8, interior)
    slots = [(1, i, j) for i, j in cells] + [(0, i, j) for i, j in cells]
    assert n <= len(slots), (n, len(slots))
    return slots[:n]


def _blank(hw):
    h, w = hw[0] // 8, hw[1] // 8
    return {k: np.zeros((h, w), np.uint8) for k in (SC, SF, SZ, SN, DX, DY)} | {g: np.full((h, w), OFF, np.uint8) for g in GATE}


SIZE_PATTERN = ((0, 49), (0, 0), (29, 0), (20, 0))           # (SZ, SN): 3.5 / 16 / 40 / 30 px for the 16-px anchor, twice that for the 32-px one
TINY, MID, HUGE = (0, 49), (29, 0), (96, 0)                   # 16-px anchor: 3.5 px (no two boxes meet), 40 px, 321 px (clipped on every border)
MID64 = (20, 0)                                               # 30 px: 64 boxes on 64 neighbouring cells still keep 16 or more


def counts_frame(hw, n, saturated=0):
    """n open gates; the score level of a cell is a bijection of its rank (8192 levels over two wires: logits 0 .. 4), box sizes follow
    SIZE_PATTERN so that some neighbours suppress each other.  `saturated`: that many cells get SC = 255 (logit 31.9: score 1.0f)."""
    w = _blank(hw)
    for r, (a, i, j) in enumerate(_slots(hw, n)):
        w[GATE[a]][i, j] = 0
    for r, (i, j) in enumerate(_cells(hw)):
        level = (r * 2731) % 8192
        w[SC][i, j], w[SF][i, j] = (255, 0) if r < saturated else (level >> 8, level & 255)
        w[SZ][i, j], w[SN][i, j] = SIZE_PATTERN[(3 * i + 5 * j) % 4]
    return paint(hw, 8, w)


def ties_frame(hw, n, size):
    """n open gates on interior cells, ONE score (SC = 8: logit 1), one box size."""
    w = _blank(hw)
    for a, i, j in _slots(hw, n, interior=True):
        w[GATE[a]][i, j] = 0
    w[SC][...] = 8
    w[SZ][...], w[SN][...] = size
    return paint(hw, 8, w)


def strides_frame(hw):
    """Head set `strides`: the gates of the interior stride-32 cells open, which opens the coincident cells of stride 16 and 8; one score."""
    h, w = hw[0] // 32, hw[1] // 32
    gate = np.full((h, w), OFF, np.uint8)
    gate[1:-1, 1:-1] = 0
    return paint(hw, 32, {GATE0: gate, GATE1: gate})


LANE63_TAIL = ((12, 14), (12, 15), (13, 14), (13, 15))


def lane63_frame(hw=SMALL):
    """63 tiny boxes with the best scores, far from the rest; then four 40-px boxes on neighbouring cells, scores descending: sorted position 63
    is kept, positions 64 .. 66 overlap it (IoU 0.47 .. 0.67) and nothing else."""
    w = _blank(hw)
    best = [(i, j) for i in range(1, 7) for j in range(1, 12)][:63]
    for r, (i, j) in enumerate(best):
        w[GATE1][i, j], w[SC][i, j], w[SF][i, j] = 0, 31, 255 - r
        w[SZ][i, j], w[SN][i, j] = TINY
    for r, (i, j) in enumerate(LANE63_TAIL):
        w[GATE1][i, j], w[SC][i, j], w[SF][i, j] = 0, 8, 255 - r
        w[SZ][i, j], w[SN][i, j] = MID
    return paint(hw, 8, w)


def edges_frame(hw=SMALL):
    """decode_anchor's edges, both anchors open on each cell: dw = dh = -3 (0.8 px: x2 - x1 < 0), sizes that clip on all four borders, dx / dy
    that carry the box outside the frame on either side (anchor 1 right / down, anchor 0 left / up); landmarks lie outside anyway."""
    w = _blank(hw)
    spots = {(2, 2): {SN: 96}, (2, 6): {SN: 64}, (8, 10): {SZ: 112}, (8, 4): {SZ: 255}, (4, 12): {DX: 255}, (12, 4): {DY: 255},
             (5, 5): {DX: 255, DY: 255, SZ: 40}, (0, 0): {}, (15, 19): {}, (0, 19): {SZ: 16}, (15, 0): {SZ: 16}, (10, 15): {DX: 70, SN: 96}}
    for r, ((i, j), kv) in enumerate(spots.items()):
        w[GATE0][i, j] = w[GATE1][i, j] = 0
        w[SC][i, j], w[SF][i, j] = 2 * r, 17 * r
        for k, v in kv.items():
            w[k][i, j] = v
    return paint(hw, 8, w)


def sparse_frame(hw, n):
    """n tiny boxes with distinct scores: all kept."""
    w = _blank(hw)
    for r, (a, i, j) in enumerate(_slots(hw, n, interior=True)):
        w[GATE[a]][i, j], w[SC][i, j], w[SF][i, j] = 0, 4 + r % 16, r
    w[SZ][...], w[SN][...] = TINY
    return paint(hw, 8, w)


def pairs_frame(hw=SMALL):
    """Pairs of neighbouring 30-px / 40-px boxes (IoU around 0.5), pairs far apart: material for an IoU threshold at equality."""
    w = _blank(hw)
    for r, (i, j) in enumerate(((2, 2), (2, 12), (10, 3), (10, 13))):
        for d in (0, 1):
            w[GATE1][i, j + d], w[SC][i, j + d], w[SF][i, j + d] = 0, 20 - 4 * d, 10 * r + d
            w[SZ][i, j + d] = (29, 20)[(r + d) % 2]
    return paint(hw, 8, w)


def exact_frame(hw, n):
    """n open gates, every regression wire 0: each box is its anchor EXACTLY (expf(0) = 1, 0 * width = 0) whatever the device's expf rounds
    like, so rows of an overflowing launch can be compared bit for bit.  Distinct score levels per cell."""
    w = _blank(hw)
    for a, i, j in _slots(hw, n):
        w[GATE[a]][i, j] = 0
    for r, (i, j) in enumerate(_cells(hw)):
        level = (r * 2731) % 8192
        w[SC][i, j], w[SF][i, j] = level >> 8, level & 255
    return paint(hw, 8, w)


# ------------------------------------------------------------------------------------------------------------ the table
class Scenario(NamedTuple):
    hw: Tuple[int, int]
    heads: str
    frame: Callable[[], np.ndarray]
    n: Optional[int] = None              # exact candidate count at THR
    kept: Optional[str] = None           # "all" | "some" (0 < kept < n) | "between" (16 <= kept < n) | "few" (0 < kept < 16)
    one_score: bool = False              # fp32: a single distinct score
    extra: Optional[str] = None          # a named condition of `check`
    max_tie: int = 1                     # the largest group of equal scores the design makes (1: all distinct; the reference's std::sort
                                         # leaves the order of equal scores open, so its build is compared only where groups stay small)
    na: int = 2                          # anchors per cell: 2 ("net3") or 4 ("net3a")
    expect: Optional[Callable[[], list]] = None      # the global anchor indices of the candidates, ascending, where the design names them


SCENARIOS: Dict[str, Scenario] = {}
for _n in (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4095, 4096):
    _hw = SMALL if _n <= 513 else LARGE
    SCENARIOS[f"counts{_n}"] = Scenario(_hw, "std", (lambda hw=_hw, n=_n: counts_frame(hw, n)), n=_n,
                                        kept="some" if _n >= 63 else None)
for _n in (64, 257, 4096):
    _hw = SMALL if _n <= 513 else LARGE
    for _tag, _size, _kept in (("tiny", TINY, "all"), ("mid", MID if _n > 64 else MID64, "between"), ("huge", HUGE, "few")):
        SCENARIOS[f"ties{_n}_{_tag}"] = Scenario(_hw, "tied", (lambda hw=_hw, n=_n, s=_size: ties_frame(hw, n, s)), n=_n, kept=_kept,
                                                 one_score=True, max_tie=_n)
SCENARIOS["strides"] = Scenario(SMALL, "strides", lambda: strides_frame(SMALL), n=36, one_score=True, extra="strides", max_tie=36)
SCENARIOS["saturated"] = Scenario(SMALL, "std", lambda: counts_frame(SMALL, 200, saturated=70), n=200, kept="some", extra="saturated", max_tie=70)
SCENARIOS["lane63"] = Scenario(SMALL, "std", lane63_frame, n=67, extra="lane63")
SCENARIOS["edges"] = Scenario(SMALL, "std", edges_frame, n=24, extra="edges")
SCENARIOS["pairs"] = Scenario(SMALL, "std", pairs_frame, n=8, extra="pairs")
SCENARIOS["kept8"] = Scenario(SMALL, "std", lambda: sparse_frame(SMALL, 8), n=8, kept="all")
SCENARIOS["kept9"] = Scenario(SMALL, "std", lambda: sparse_frame(SMALL, 9), n=9, kept="all")
SCENARIOS["exact64"] = Scenario(SMALL, "std", lambda: exact_frame(SMALL, 64), n=64, kept="some")
SCENARIOS["exact65"] = Scenario(SMALL, "std", lambda: exact_frame(SMALL, 65), n=65, kept="some")
SCENARIOS["exact4608"] = Scenario(LARGE, "std", lambda: exact_frame(LARGE, 4608), n=4608, kept="some")
MIXED = (0, 1, 64, 65, 257, 4096)                             # one launch: the frames of these counts, all painted at LARGE
for _n in MIXED:
    SCENARIOS[f"mixed{_n}"] = Scenario(LARGE, "std", (lambda n=_n: counts_frame(LARGE, n)), n=_n, kept="some" if _n >= 63 else None)


# ------------------------------------------------------------------------------------------------------------ four anchors per cell
SIZES4 = ((128, 160), (96, 160))                             # stride-8 maps 16 x 20 (blocks of 64 pixels filled exactly) and 12 x 20; on the
                                                              # second the last block of every level is partial: 15, 60 and 240 cells


def network_of(sc) -> str:
    return "net3a" if sc.na == 4 else "net3"


def ratios_of(sc) -> Tuple[float, ...]:
    return RATIOS4 if sc.na == 4 else (1.0,)


def _blank4(hw):
    h, w = hw[0] // 8, hw[1] // 8
    return {k: np.zeros((h, w), np.uint8) for k in (SC, SZ, DX, DY)} | {g: np.full((h, w), OFF, np.uint8) for g in GATE4}


def _paint4(hw, w):
    return paint(hw, 8, w, gates=GATE4)


def _levels4(hw, w):
    """distinct score levels and distinct (DX, DY) per stride-8 cell: SC a bijection of the cell's rank (maps of up to 256 cells are all
    distinct; the scenarios open fewer cells than that), DX, DY below 64 (up to 2 anchor sizes)"""
    for r, (i, j) in enumerate(_cells(hw)):
        w[SC][i, j] = (r * 37) % 256
        w[DX][i, j], w[DY][i, j] = (7 * i + 3 * j) % 64, (5 * i + 11 * j + 1) % 64


def global_index(hw, stride, a, i, j, na=4) -> int:
    """anchor_offset(stride) + a * h * w + cell of the net of size hw"""
    off = anchor_offsets(hw, na)[stride]
    h, w = hw[0] // stride, hw[1] // stride
    return off + a * h * w + i * w + j


def alone_cells(hw):
    """The stride-8 cells the `alone` frames open: every cell with both coordinates a multiple of 4 (which opens the coincident stride-32
    and stride-16 cells), the stride-16 cells (2, 2 + 4k) (stride-8 cells (4, 4 + 8k): not on the stride-32 grid) and the stride-8 cells
    (odd, odd) of every sixth column."""
    h, w = hw[0] // 8, hw[1] // 8
    cells = {(i, j) for i in range(0, h, 4) for j in range(0, w, 4)} | {(4 * 1, 4 + 8 * k) for k in range(w // 8)}
    cells |= {(2, 6 + 8 * k) for k in range((w - 6 + 7) // 8)} | {(i, j) for i in range(1, h, 4) for j in range(1, w, 6)}
    return sorted(cells)


def alone_frame(hw, a):
    """Head set `strides4`: the gate of anchor a alone, on alone_cells; distinct DX, DY and score level per cell."""
    w = _blank4(hw)
    _levels4(hw, w)
    for r, (i, j) in enumerate(alone_cells(hw)):
        w[GATE4[a]][i, j], w[SC][i, j] = 0, 3 * r          # every third level: the strides' biases (STRIDE_BIAS4) fill the two between
    assert 3 * r <= 255
    return _paint4(hw, w)


def alone_expect(hw, a):
    idx = []
    for i, j in alone_cells(hw):
        for s in STRIDES:
            q = s // 8
            if i % q == 0 and j % q == 0:
                idx.append(global_index(hw, s, a, i // q, j // q))
    return sorted(idx)


def all4_cells(hw):
    h, w = hw[0] // 8, hw[1] // 8
    return [(i, j) for i in (3, h - 4) for j in (3, w - 4)]


def all4_frame(hw, tied=False):
    """All four gates open on four cells far apart (`std4`: four distinct scores per cell; `tied4`: one score on all sixteen), every
    regression wire 0: each box is its anchor exactly, and the square and the tall box of one cell overlap (IoU 0.675)."""
    w = _blank4(hw)
    for r, (i, j) in enumerate(all4_cells(hw)):
        for g in GATE4:
            w[g][i, j] = 0
        w[SC][i, j] = 8 if tied else 16 + 40 * r
    if tied:
        w[SC][...] = 8
    return _paint4(hw, w)


def asym_cells(hw):
    h, w = hw[0] // 8, hw[1] // 8
    return [(i, j) for i in (4, h - 5) for j in (5, 10, w - 6)]


def asym_frame(hw):
    """Anchors 2 (26 x 40) and 3 (13 x 20) alone, on interior cells far apart: dx = -0.625 / +2.5, dy = -0.25 / +0.25 (DX = 40, DY = 8),
    dw = dh = 0."""
    w = _blank4(hw)
    for r, (i, j) in enumerate(asym_cells(hw)):
        w[GATE2][i, j] = w[GATE3][i, j] = 0
        w[SC][i, j], w[DX][i, j], w[DY][i, j] = 10 + 30 * r, 40, 8
    return _paint4(hw, w)


def clip4_frame(hw):
    """All four anchors on the four corner cells (the non-square anchors clip on every border; anchor 3 of the top-left cell keeps its
    fractional x1 = 1.5), on a cell whose boxes are 50 .. 20000 times the anchor (clipped on all four borders), and on cells whose DX / DY carry
    the boxes outside: to the left / above for anchors 0 and 2, to the right / below for anchors 1 and 3 -- clipped on ONE side only, which
    leaves x2 - x1 < 0 (y2 - y1 < 0)."""
    w = _blank4(hw)
    h, ww = hw[0] // 8, hw[1] // 8
    spots = {(0, 0): {}, (0, ww - 1): {}, (h - 1, 0): {}, (h - 1, ww - 1): {}, (h // 2, ww // 2): {SZ: 255}, (3, 5): {DX: 255}, (5, 13): {DY: 255},
             (h - 3, 9): {DX: 255, DY: 255, SZ: 20}, (1, 1): {SZ: 40}, (h - 2, ww - 2): {DX: 30, DY: 90}}
    for r, ((i, j), kv) in enumerate(spots.items()):
        for g in GATE4:
            w[g][i, j] = 0
        w[SC][i, j] = 5 + 23 * r
        for k, v in kv.items():
            w[k][i, j] = v
    return _paint4(hw, w)


def _slots4(hw, n):
    """the first n (anchor, i, j): the four anchors of a cell, then the next cell of the stride-8 map (row-major)"""
    slots = [(a, i, j) for i, j in _cells(hw) for a in range(4)]
    assert n <= len(slots)
    return slots[:n]


def count4_frame(hw, n):
    """n open gates, every regression wire 0 (each box is its anchor EXACTLY: rows of an overflowing launch compare bit for bit), a distinct
    score level per cell."""
    w = _blank4(hw)
    assert n <= 4 * 256
    for r, (i, j) in enumerate(_cells(hw)):
        w[SC][i, j] = (r * 37) % 256
    for a, i, j in _slots4(hw, n):
        w[GATE4[a]][i, j] = 0
    return _paint4(hw, w)


def sparse4_frame(hw, n):
    """n boxes that do not meet, the anchors in turn: all kept."""
    w = _blank4(hw)
    h, ww = hw[0] // 8, hw[1] // 8
    cells = [(i, j) for i in range(1, h, 5)[:3] for j in range(1, ww, 5)]
    assert n <= len(cells)
    for r, (i, j) in enumerate(cells[:n]):
        w[GATE4[r % 4]][i, j], w[SC][i, j] = 0, 20 + 9 * r
    return _paint4(hw, w)


def tag4(hw) -> str:
    return f"{hw[0]}x{hw[1]}"


for _hw in SIZES4:                                            # the A = 4 scenarios, per size: a4_<what>_<size>; SCENARIOS4 lists their names
    _t = tag4(_hw)
    for _a in range(4):
        SCENARIOS[f"a4_alone{_a}_{_t}"] = Scenario(_hw, "strides4", (lambda hw=_hw, a=_a: alone_frame(hw, a)), extra=f"alone{_a}", na=4,
                                                   expect=(lambda hw=_hw, a=_a: alone_expect(hw, a)))
    SCENARIOS[f"a4_all_{_t}"] = Scenario(_hw, "std4", (lambda hw=_hw: all4_frame(hw)), n=16, extra="all4", na=4)
    SCENARIOS[f"a4_alltied_{_t}"] = Scenario(_hw, "tied4", (lambda hw=_hw: all4_frame(hw, tied=True)), n=16, one_score=True, extra="all4", max_tie=16, na=4)
    SCENARIOS[f"a4_asym_{_t}"] = Scenario(_hw, "std4", (lambda hw=_hw: asym_frame(hw)), n=12, kept="all", extra="asym", na=4)
    SCENARIOS[f"a4_clip_{_t}"] = Scenario(_hw, "std4", (lambda hw=_hw: clip4_frame(hw)), n=40, extra="clip4", na=4)
    for _n in (64, 65, 300):
        SCENARIOS[f"a4_count{_n}_{_t}"] = Scenario(_hw, "std4", (lambda hw=_hw, n=_n: count4_frame(hw, n)), n=_n, kept="some", na=4)
    for _n in (8, 9):
        SCENARIOS[f"a4_kept{_n}_{_t}"] = Scenario(_hw, "std4", (lambda hw=_hw, n=_n: sparse4_frame(hw, n)), n=_n, kept="all", na=4)
SCENARIOS4 = [n for n in SCENARIOS if n.startswith("a4_")]


def anchor_numbers(idx, hw, na):
    """global anchor indices -> (stride, anchor number within the cell, cell index) arrays"""
    idx = np.asarray(idx, np.int64)
    st, an, gp = (np.full(idx.shape, -1, np.int64) for _ in range(3))
    offs = anchor_offsets(hw, na)
    for s in STRIDES:
        cells = (hw[0] // s) * (hw[1] // s)
        m = (idx >= offs[s]) & (idx < offs[s] + na * cells)
        st[m], an[m], gp[m] = s, (idx[m] - offs[s]) // cells, (idx[m] - offs[s]) % cells
    assert (st > 0).all()
    return st, an, gp


def base_anchors4():
    from oracle.retinaface_post import base_anchors
    return base_anchors(RATIOS4)


def swap_moves(row, idx, hw) -> float:
    """By how many pixels the box centre of candidate `row` (anchor `idx` of a four-anchor net) would move if bbox_pred multiplied dx by the
    anchor's height and dy by its width: |dx| * |height - width| and |dy| * |width - height|, the larger; dx, dy recovered from the row."""
    st, an, gp = (int(v[0]) for v in anchor_numbers([idx], hw, 4))
    b = base_anchors4()[st][an].astype(np.float64)
    ww = hw[1] // st
    width, height = b[2] - b[0] + 1, b[3] - b[1] + 1
    ctr_x, ctr_y = b[0] + 0.5 * (width - 1) + st * (gp % ww), b[1] + 0.5 * (height - 1) + st * (gp // ww)
    dx = (0.5 * (float(row[1]) + float(row[3])) - ctr_x) / width
    dy = (0.5 * (float(row[2]) + float(row[4])) - ctr_y) / height
    return max(abs(dx) * abs(height - width), abs(dy) * abs(height - width))


def iou_f32(a, b) -> np.float32:
    """IoU of two boxes (x1, y1, x2, y2) with the +1 convention in float32, the restatement's op order (rf_post_ref.c rfo_nms); 0 where the
    restatement skips the pair."""
    a, b = [F32(v) for v in a], [F32(v) for v in b]
    area1 = (a[2] - a[0] + F32(1)) * (a[3] - a[1] + F32(1))
    x, y = max(a[0], b[0]), max(a[1], b[1])
    w = min(a[2], b[2]) - x + F32(1)
    h = min(a[3], b[3]) - y + F32(1)
    if w <= 0 or h <= 0:
        return F32(0)
    area2 = (b[2] - b[0] + F32(1)) * (b[3] - b[1] + F32(1))
    inter = w * h
    return F32(inter / (area1 + area2 - inter))


def sorted_candidates(cand, cidx):
    """candidate rows and anchors in the NMS order: score descending, anchor index ascending"""
    order = np.lexsort((cidx, -cand[:, 0].astype(np.float64)))
    return cand[order], cidx[order]


def anchor_offsets(hw, na=2):
    offs, acc = {}, 0
    for s in STRIDES:
        offs[s] = acc
        acc += na * (hw[0] // s) * (hw[1] // s)
    return offs


def check(sc: Scenario, cand, cidx, kept, kidx, ties: bool = True, nms: float = NMS) -> None:
    """Assert the scenario's condition on a restatement result at THR (cand / cidx: candidates in decode order, kept / kidx: after NMS)."""
    n, k = len(cidx), len(kidx)
    if sc.n is not None:
        assert n == sc.n, (n, sc.n)
    if sc.kept == "all":
        assert k == n, (k, n)
    elif sc.kept == "some":
        assert 0 < k < n, (k, n)
    elif sc.kept == "between":
        assert 16 <= k < n, (k, n)
    elif sc.kept == "few":
        assert 0 < k < 16, (k, n)
    if sc.max_tie == 1 and ties:
        assert len(np.unique(cand[:, 0])) == n, (len(np.unique(cand[:, 0])), n)      # designed distinct: the order is the scores' alone
    if sc.one_score and ties:
        assert len(np.unique(cand[:, 0])) == 1, np.unique(cand[:, 0])
        assert np.array_equal(kidx, np.sort(kidx))                           # all tied: the order is the anchor index alone
    if sc.extra == "strides" and ties:
        offs = anchor_offsets(sc.hw)
        per = [int(((cidx >= offs[s]) & (cidx < offs[s] + 2 * (sc.hw[0] // s) * (sc.hw[1] // s))).sum()) for s in STRIDES]
        assert per == [12, 12, 12], per                                      # equal scores on all three strides
    if sc.extra == "saturated" and ties:
        assert int((cand[:, 0] == F32(1)).sum()) >= 65, int((cand[:, 0] == F32(1)).sum())
    if sc.extra == "lane63":
        srt, sidx = sorted_candidates(cand, cidx)
        assert kidx[:64].tolist() == sidx[:64].tolist() and int(sidx[64]) not in kidx.tolist()
        assert iou_f32(srt[63, 1:5], srt[64, 1:5]) > F32(nms)
        assert all(iou_f32(srt[p, 1:5], srt[64, 1:5]) == 0 for p in range(63))      # position 63 alone suppresses position 64
    if sc.extra == "edges":
        w = cand[:, 3] - cand[:, 1]
        assert ((w < 0) & (w > -1) & (cand[:, 1] > 0) & (cand[:, 3] < sc.hw[1] - 1)).any()      # a box below one pixel, nothing clipped
        assert (cand[:, 1] == 0).any() and (cand[:, 2] == 0).any() and (cand[:, 3] == sc.hw[1] - 1).any() and (cand[:, 4] == sc.hw[0] - 1).any()
        full = (cand[:, 1] == 0) & (cand[:, 2] == 0) & (cand[:, 3] == sc.hw[1] - 1) & (cand[:, 4] == sc.hw[0] - 1)
        assert full.any()                                                    # one box clipped on all four borders
        assert (cand[:, 1] > sc.hw[1] - 1).any() and (cand[:, 2] > sc.hw[0] - 1).any()      # carried outside right / below: x1, y1 are not clipped there
        assert (cand[:, 3] < 0).any() and (cand[:, 4] < 0).any()             # carried outside left / above: x2, y2 are not clipped there
        assert (cand[:, 5:10] < 0).any() and (cand[:, 5:10] > sc.hw[1]).any() and (cand[:, 10:15] < 0).any() and (cand[:, 10:15] > sc.hw[0]).any()
    if sc.extra == "pairs":
        srt, _ = sorted_candidates(cand, cidx)
        i, j = pairs_pick(srt)
        assert F32(0.2) < iou_f32(srt[i, 1:5], srt[j, 1:5]) < F32(0.8)
    if sc.na == 4:
        check4(sc, cand, cidx, kept, kidx, ties, nms)


def check4(sc: Scenario, cand, cidx, kept, kidx, ties: bool, nms: float) -> None:
    """The conditions of the four-anchor scenarios."""
    hw = sc.hw
    st, an, gp = anchor_numbers(cidx, hw, 4)
    kst, kan, kgp = anchor_numbers(kidx, hw, 4)
    if sc.expect is not None:
        assert sorted(cidx.tolist()) == sc.expect(), (sorted(cidx.tolist()), sc.expect())
    if sc.extra and sc.extra.startswith("alone"):
        a = int(sc.extra[5:])
        assert (an == a).all() and (kan == a).all()               # every index is anchor_offset + a * hw + gp of the one open anchor
        for s in STRIDES:
            assert (st == s).sum() >= 3 and (kst == s).sum() >= 1, (s, int((st == s).sum()), int((kst == s).sum()))
        c8 = cand[st == 8]                                        # (the 512- and 128-px anchors of the coarser strides clip to the frame)
        assert len(np.unique(c8[:, 1:5], axis=0)) == len(c8)      # distinct DX, DY per cell: no two boxes alike
        assert len(np.unique(cand[:, 5:15], axis=0)) == len(cand)
    if sc.extra == "all4":
        cells = sorted(set(gp.tolist()))
        assert len(cells) == 4 and all(sorted(an[gp == c].tolist()) == [0, 1, 2, 3] for c in cells)      # all four survive decode
        assert 0 < len(kidx) < len(cidx)
        for c in cells:
            rows = {int(a): cand[(gp == c) & (an == a)][0] for a in range(4)}
            assert iou_f32(rows[0][1:5], rows[2][1:5]) > F32(nms) and iou_f32(rows[1][1:5], rows[3][1:5]) > F32(nms)      # square and tall overlap
            assert iou_f32(rows[0][1:5], rows[1][1:5]) < F32(nms) and iou_f32(rows[2][1:5], rows[3][1:5]) < F32(nms)
            if ties:
                # NMS across the four: the better of each (square, tall) pair stays -- anchors 0 and 3 by score, 0 and 1 by index when tied
                want = [0, 1] if sc.one_score else [0, 3]
                assert sorted(kan[kgp == c].tolist()) == want, (c, kan[kgp == c].tolist())
                if not sc.one_score:
                    order = [int(a) for a in an[gp == c][np.argsort(-cand[gp == c, 0].astype(np.float64))]]
                    assert order == [0, 3, 1, 2], order              # the order inside a cell: the foreground biases
    if sc.extra == "asym":
        assert set(an.tolist()) == {2, 3} and (st == 8).all()
        bw, bh = cand[:, 3] - cand[:, 1] + 1, cand[:, 4] - cand[:, 2] + 1
        # dw = dh = 0: the anchor's own 26 x 40 / 13 x 20 (the centre is no dyadic number any more, so the corners round: 1e-3 px)
        assert np.abs(bw - np.where(an == 2, 26, 13)).max() < 1e-3 and np.abs(bh - np.where(an == 2, 40, 20)).max() < 1e-3
        for row, i in zip(kept, kidx):
            assert swap_moves(row, int(i), hw) > 1.0, (int(i), swap_moves(row, int(i), hw))      # width taken for height moves it by > 1 px
        assert np.abs(cand[:, 5:10] - cand[:, 10:15]).min() > 1.0  # LMK: every landmark's x differs from its y
    if sc.extra == "clip4":
        H, W = hw
        for a in (2, 3):
            c = cand[an == a]
            assert (c[:, 1] == 0).any() and (c[:, 2] == 0).any() and (c[:, 3] == W - 1).any() and (c[:, 4] == H - 1).any(), a
            assert ((c[:, 1] == 0) & (c[:, 2] == 0) & (c[:, 3] == W - 1) & (c[:, 4] == H - 1)).any(), a      # clipped on all four borders
            assert (c[:, 3] - c[:, 1] < 0).any() and (c[:, 4] - c[:, 2] < 0).any(), a                        # x2 - x1 < 0 after clipping
        c = cand[an == 3]
        assert ((c[:, 1] % 1 == 0.5) & (c[:, 3] % 1 == 0.5)).any()                                         # the fractional anchor, unclipped in x
        c = cand[(an == 0) | (an == 2)]
        assert (c[:, 3] < 0).any() and (c[:, 4] < 0).any()          # carried outside left / above: x2, y2 are not clipped there
        c = cand[(an == 1) | (an == 3)]
        assert (c[:, 1] > W - 1).any() and (c[:, 2] > H - 1).any()  # carried outside right / below: x1, y1 are not clipped there
    if sc.extra is None:
        assert set(an.tolist()) == {0, 1, 2, 3} or len(cidx) < 4
        assert set(kan.tolist()) == {0, 1, 2, 3} or sc.kept != "all" or len(kidx) < 4


def pairs_pick(srt):
    """The pair of `pairs` whose IoU becomes the second engine's NMS threshold: the best box and the one box that overlaps it."""
    hit = [j for j in range(1, len(srt)) if iou_f32(srt[0, 1:5], srt[j, 1:5]) > 0]
    assert len(hit) == 1, hit
    return 0, hit[0]
