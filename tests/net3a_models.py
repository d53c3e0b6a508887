"""A four-anchor model for the "net3a" preset, derived at run time from a `NetSpec` (numpy only, no GPU); nothing is stored.

The reference ships no model with four anchors per cell, so the heads of a shipped two-anchor model are widened (`widen_heads`).  Anchors 0
and 1 keep their trained rows.  Anchors 2 and 3 take the rows of anchors 1 and 0 -- crosswise -- and every one of their 32 rows per stride
(2 class, 4 box, 10 landmark rows per anchor) is multiplied element by element by its own seeded vector over the 64 input channels, its bias
by its own seeded factor.  A kernel that read anchor a's class, box or landmark channels for anchor a + 2 (or a ^ 1, or a ^ 2) therefore
returns other numbers, and no row of a stride is another row of it, or another row times one common factor (`rows_are_distinct`).

The two class rows of a new anchor share ONE vector, so its logit difference is the donor's with every input channel's contribution scaled
by 0.85 .. 1.0: the scores stay where trained scores lie, and on the fixture crops every anchor index has candidates at thresholds 0.5 and
0.02 (asserted where the model is used).  Box and landmark rows vary by 0.75 .. 1.25 per element.

The trained 16-px-scale anchor (anchor 1, and anchor 2 that starts from it) passes 0.02 on a handful of cells of the small fixture crops
and 0.5 on none, so the foreground bias of anchors 1 and 2 is raised by FG_SHIFT (4.5 and 4.25 logits: what scored above 0.011 / 0.014
now passes 0.5).  This is the one change to a row of anchors 0 and 1.

Channel layout of the heads (caffe prototxt, A anchors): class score [background 0..A-1 | foreground 0..A-1], box a * 4 + (dx, dy, dw, dh),
landmark a * 10 + (x0, y0, .. x4, y4); Reshape(., 2A, -1, .) behind the two-class softmax.
"""
from __future__ import annotations

import copy
import zlib

import numpy as np

F32 = np.float32
SEED = 20240517
STRIDES = (32, 16, 8)
RATIOS = (1.0, 1.5)                      # "net3a"
DONOR = {2: 1, 3: 0}                     # new anchor -> the anchor whose rows it starts from
CLS_RANGE = (0.85, 1.0)
FG_SHIFT = {1: F32(4.5), 2: F32(4.25)}   # added to the foreground bias: see the module text
REG_RANGE = (0.75, 1.25)


def _rng(*key):
    return np.random.default_rng([SEED] + [zlib.crc32(str(k).encode()) for k in key])


def _vary(w, b, lo, hi, *key):
    """rows `w` (n, 64, 1, 1) times a seeded (n, 64) array in [lo, hi), biases `b` (n,) times a seeded (n,) array in [lo, hi)"""
    rng = _rng(*key)
    fw = rng.uniform(lo, hi, w.shape).astype(F32)
    fb = rng.uniform(lo, hi, b.shape).astype(F32)
    return (w * fw).astype(F32), (b * fb).astype(F32)


def widen_heads(net):
    """A copy of `net` (a two-anchor NetSpec, either stem) whose heads carry four anchors per cell, without calibrated weights.  Every blob
    keeps its name, so the shipped calibration table still applies."""
    out = copy.deepcopy(net)
    out.int8_qweights = {}
    for s in STRIDES:
        cls = out.layer(f"face_rpn_cls_score_stride{s}")
        w, b = cls.blobs[0], cls.blobs[1].reshape(-1)
        assert w.shape == (4, 64, 1, 1), w.shape
        bg, fg, bbg, bfg = [w[0:2]], [w[2:4]], [b[0:2]], [b[2:4]]
        for a, d in DONOR.items():
            rng = _rng("cls", s, a)
            v = rng.uniform(*CLS_RANGE, (1, 64, 1, 1)).astype(F32)          # one vector for the background and the foreground row
            fb = rng.uniform(*CLS_RANGE, 2).astype(F32)
            bg.append(w[d:d + 1] * v)
            fg.append(w[2 + d:3 + d] * v)
            bbg.append(b[d:d + 1] * fb[0])
            bfg.append(b[2 + d:3 + d] * fb[1])
        bfg = np.concatenate(bfg).astype(F32)
        for a, shift in FG_SHIFT.items():
            bfg[a] += shift
        cls.blobs[0] = np.concatenate(bg + fg).astype(F32)
        cls.blobs[1] = np.concatenate(bbg + [bfg]).astype(F32).reshape(cls.blobs[1].shape[:-1] + (8,))
        cls.num_output = 8
        back = out.layer(f"face_rpn_cls_prob_reshape_stride{s}")           # Reshape(., 2A, -1, .) after the 2-class softmax
        assert 4 in back.reshape_dims
        back.reshape_dims = [8 if d == 4 else d for d in back.reshape_dims]
        for name, per in ((f"face_rpn_bbox_pred_stride{s}", 4), (f"face_rpn_landmark_pred_stride{s}", 10)):
            l = out.layer(name)
            w, b = l.blobs[0], l.blobs[1].reshape(-1)
            assert w.shape == (2 * per, 64, 1, 1), (name, w.shape)
            ws, bs = [w], [b]
            for a, d in DONOR.items():
                nw, nb = _vary(w[d * per:(d + 1) * per], b[d * per:(d + 1) * per], *REG_RANGE, name, a)
                ws.append(nw)
                bs.append(nb)
            l.blobs[0] = np.concatenate(ws).astype(F32)
            l.blobs[1] = np.concatenate(bs).astype(F32).reshape(l.blobs[1].shape[:-1] + (4 * per,))
            l.num_output = 4 * per
    return out


def head_rows(net, stride: int) -> np.ndarray:
    """the 16A rows of a stride's three head convolutions, (16A, 65): 64 weights and the bias"""
    rows = []
    for n in ("cls_score", "bbox_pred", "landmark_pred"):
        l = net.layer(f"face_rpn_{n}_stride{stride}")
        rows.append(np.concatenate([l.blobs[0].reshape(l.blobs[0].shape[0], -1), l.blobs[1].reshape(-1, 1)], axis=1))
    return np.concatenate(rows).astype(np.float64)


def rows_are_distinct(rows: np.ndarray) -> bool:
    """No two rows equal, and none another row times one common factor: the normalised rows (unit length, first nonzero element positive)
    are pairwise different in at least one element by more than rounding."""
    assert np.abs(rows).max(1).min() > 0
    unit = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    first = unit[np.arange(len(unit)), (unit != 0).argmax(1)]
    unit = unit * np.sign(first)[:, None]
    gap = np.abs(unit[:, None, :] - unit[None, :, :]).max(-1)
    gap[np.arange(len(unit)), np.arange(len(unit))] = 1.0
    return bool(gap.min() > 1e-4)


def anchors_of(idx, hw, na: int = 4):
    """global anchor indices -> the anchor number `an` of each (index = offset(stride) + an * h * w + cell)"""
    idx = np.asarray(idx, np.int64)
    an = np.full(idx.shape, -1, np.int64)
    off = 0
    for s in STRIDES:
        cells = (hw[0] // s) * (hw[1] // s)
        m = (idx >= off) & (idx < off + na * cells)
        an[m] = (idx[m] - off) // cells
        off += na * cells
    assert (an >= 0).all()
    return an


def write_model_dir(nets, path: str) -> str:
    """`path` filled with the widened model of every stem of `nets` (stem -> NetSpec), under the shipped file names; the calibration table
    travels inside the .rfw.  Returns `path`."""
    import os
    from oracle.caffe_io import write_rfw
    for stem, net in nets.items():
        write_rfw(widen_heads(net), os.path.join(path, stem + ".rfw"))
    return path


def anchors_with_candidates(prob_blobs, thr: float, na: int = 4):
    """The anchor numbers that have a candidate: prob_blobs are the cls_prob blobs (N, 2A, H, W) of the strides, any images."""
    return {a for p in prob_blobs for a in range(na) if (np.asarray(p)[:, na + a] > thr).any()}
