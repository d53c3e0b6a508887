"""The four-anchor model of tests/net3a_models.py on the CPU (no GPU): `widen_heads` gives 64 head channels per stride that are all
distinct, on both stems; the fp32 oracle finds candidates of every anchor number 0..3 at thresholds 0.5 and 0.02 on the frames the GPU
tests judge; and on those natural head blobs the plain-C restatement with the ratios of "net3a" (the judge of the GPU tests) equals the
numpy restatement and, where it is present, the reference build's own postProcess bit for bit."""
import numpy as np
import pytest

import launch_ref as lr
import net3a_models as nm
from conftest import STEMS
from oracle import build as obuild
from oracle import build_ref
from oracle import retinaface_post as post
from oracle.caffe_forward import HEAD_STRIDES, CaffeNet, head_names

THRESHOLDS = (0.5, 0.02)


@pytest.fixture(scope="module")
def wide(nets):
    return {s: nm.widen_heads(nets[s]) for s in STEMS}


@pytest.mark.parametrize("stem", STEMS)
def test_widened_heads_have_64_distinct_channels(nets, wide, stem):
    """16A = 64 rows per stride, none equal to another or to another times one factor (before the widening the same holds of the 32);
    anchors 0 and 1 keep their box and landmark rows and their class weights; nothing but the heads changes; no calibrated weights."""
    net, w = nets[stem], wide[stem]
    assert w.int8_qweights == {} and w.int8_scales == net.int8_scales and [l.name for l in w.layers] == [l.name for l in net.layers]
    for s in nm.STRIDES:
        rows = nm.head_rows(w, s)
        assert rows.shape == (64, 65)
        assert nm.rows_are_distinct(rows) and nm.rows_are_distinct(nm.head_rows(net, s))
        doubled = np.concatenate([nm.head_rows(net, s)] * 2)
        assert not nm.rows_are_distinct(doubled)                                  # what a model widened by copying looks like
        for name, per in (("bbox_pred", 4), ("landmark_pred", 10)):
            a, b = net.layer(f"face_rpn_{name}_stride{s}"), w.layer(f"face_rpn_{name}_stride{s}")
            assert np.array_equal(b.blobs[0][:2 * per], a.blobs[0]) and np.array_equal(b.blobs[1].reshape(-1)[:2 * per], a.blobs[1].reshape(-1))
        a, b = net.layer(f"face_rpn_cls_score_stride{s}"), w.layer(f"face_rpn_cls_score_stride{s}")
        assert np.array_equal(b.blobs[0][[0, 1, 4, 5]], a.blobs[0])
    heads = {f"face_rpn_{n}_stride{s}" for n in ("cls_score", "bbox_pred", "landmark_pred") for s in nm.STRIDES}
    for a, b in zip(net.layers, w.layers):
        if a.name not in heads:
            assert all(np.array_equal(x, y) for x, y in zip(a.blobs, b.blobs)), a.name


@pytest.mark.parametrize("stem", STEMS)
def test_every_anchor_has_candidates_and_the_restatements_agree(wide, base_frame, stem):
    """The three frames of each interval / int8 case (64 x 96, 96 x 160), fp32 oracle heads of the widened model: candidates of every
    anchor number at 0.5 and at 0.02 in every call; C restatement == numpy restatement == the reference build under "net3a"."""
    net = CaffeNet(wide[stem])
    for hw in lr.SMALL_SIZES:
        seen = {t: set() for t in THRESHOLDS}
        for f in lr.case_frames(base_frame, hw):
            blobs = net.forward(post.preprocess_trt_identity(f, *hw))
            heads = {n: blobs[n] for s in HEAD_STRIDES for n in head_names(s)}
            h9 = [heads[n][0] for s in HEAD_STRIDES for n in head_names(s)]
            assert h9[0].shape[0] == 8 and h9[1].shape[0] == 16 and h9[2].shape[0] == 40
            for thr in THRESHOLDS:
                cand, cidx, kept, kidx = obuild.decode_nms(h9, hw[0], hw[1], thr, 0.4, ratios=nm.RATIOS)
                seen[thr] |= set(nm.anchors_of(cidx, hw).tolist())
                assert seen[thr] >= nm.anchors_with_candidates([h9[0][None], h9[3][None], h9[6][None]], thr)
                cands = post.decode(heads, hw[0], hw[1], thr, ratios=nm.RATIOS)
                dets = post.nms(list(cands), 0.4)
                assert [d.anchor_index for d in cands] == cidx.tolist() and [d.anchor_index for d in dets] == kidx.tolist()
                assert np.array_equal(np.stack([d.as_row() for d in dets]), kept)
                if build_ref.available():
                    r = build_ref.ReferenceRetinaFace(hw[0], hw[1], max_batch=1, network="net3a", head_anchors=4)
                    try:
                        r.set_heads(0, h9)
                        assert np.array_equal(r.postprocess(0, thr), kept)
                    finally:
                        r.close()
        assert all(seen[t] == {0, 1, 2, 3} for t in THRESHOLDS), (stem, hw, seen)
