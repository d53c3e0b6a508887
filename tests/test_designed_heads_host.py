"""tests/designed_heads.py on the CPU oracle alone (no GPU): the wire sets really are wires, and every scenario of the table reaches the
condition the GPU tests (tests/test_designed_heads_gpu.py) rely on -- candidate counts on the regime boundaries, exact ties, lane 63,
decode's edges -- by the reference restatements alone.  The numpy restatement (OracleDetector.detect) and the plain-C one
(oracle.build.decode_nms) must agree on candidates, kept anchors and order, ties included; the reference build's own postProcess
(oracle/build_ref.py) is compared bit for bit where it is present and the scenario's scores are distinct.  The four-anchor scenarios
(a4_*) go the same way with the ratios of "net3a": the C restatement takes them as an argument, and the reference build is created
with network "net3a"."""
import numpy as np
import pytest

import designed_heads as dh
from conftest import STEMS
from oracle import build as obuild
from oracle import build_ref
from oracle.caffe_forward import HEAD_STRIDES, head_names
from oracle.retinaface_post import preprocess_trt_identity

# eps of the 27 backbone BatchNorms is 1e-5, of the FPN / SSH ones 2e-5; at most 27 + 3 lie between the frame and a head input, each a
# factor (1 + eps)^-1/2 >= 1 - eps / 2, so a wire arrives within 27 * 0.5e-5 + 3 * 1e-5 = 1.65e-4 of the pixel, relative; fp32 rounding of
# 30 multiplications adds at most 30 * 6e-8.  Measured: 8.6e-5 .. 1.6e-4.
WIRE_REL = 1.65e-4 + 30 * 6e-8


@pytest.fixture(scope="module")
def wired(nets):
    from oracle.pipeline import OracleDetector
    return {k: OracleDetector(dh.wire_net(nets["mnet25"], k)) for k in list(dh.HEAD_SETS) + list(dh.HEAD_SETS4)}


@pytest.mark.parametrize("stem", STEMS)
def test_the_wire_set_carries_pixels_to_the_head_inputs(nets, stem):
    """64 x 96, a seeded random frame: channel c of rf_c{3,2,1}_det_concat_relu equals frame[dy::s, dx::s, colour of wire c] within the
    BatchNorm factors, a painted 0 arrives as an exact 0, and channels 8..63 are exactly 0 -- on both shipped stems."""
    from oracle.caffe_forward import CaffeNet
    hw = (64, 96)
    frame = np.random.default_rng(20240517).integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)
    frame[:32, :32] = 0
    blobs = CaffeNet(dh.wire_net(nets[stem])).forward(preprocess_trt_identity(frame, *hw), keep_all=True)
    for s, level in zip(dh.STRIDES, (3, 2, 1)):
        t = blobs[f"rf_c{level}_det_concat_relu"][0]
        assert t.shape == (64, hw[0] // s, hw[1] // s)
        assert not t[len(dh.WIRES):].any()
        for c in range(len(dh.WIRES)):
            want = dh.wire_view(frame, s, c).astype(np.float64)
            assert want.any() and not want.all()
            assert np.all(np.abs(t[c] - want) <= WIRE_REL * want), (stem, s, c, float(np.abs(t[c] - want).max()))
    for n in (f"face_rpn_{k}_stride{s}" for s in dh.STRIDES for k in ("cls_score", "bbox_pred", "landmark_pred")):
        assert not blobs[n].any()                                              # heads not set: all 0


def _oracle_heads(od, sc):
    blobs = od.forward(preprocess_trt_identity(sc.frame(), *sc.hw))
    return [blobs[n][0] for s in HEAD_STRIDES for n in head_names(s)]


# mixed4096 is counts4096's frame: its numpy NMS (13 s) is not repeated
ROWS = [n for n in dh.SCENARIOS if n != "mixed4096"]


@pytest.mark.parametrize("name", ROWS)
def test_scenario_reaches_its_condition_on_the_oracle(wired, name):
    """The oracle's heads for the scenario's frame, decoded by the C restatement: the scenario's condition holds (designed_heads.check).
    The numpy restatement gives the same candidates in the same order and keeps the same anchors in the same order, bit for bit.  Where
    the reference build is present and no two candidates tie (its std::sort leaves the order of equal scores open) its postProcess returns
    the same rows."""
    from oracle import retinaface_post as post
    from oracle.pipeline import OracleDetector
    sc = dh.SCENARIOS[name]
    od = wired[sc.heads]
    h9 = _oracle_heads(od, sc)
    ratios = dh.ratios_of(sc)
    assert h9[0].shape[0] == 2 * sc.na and len(ratios) * 2 == sc.na
    cand, cidx, kept, kidx = obuild.decode_nms(h9, sc.hw[0], sc.hw[1], dh.THR, dh.NMS, ratios=ratios)
    dh.check(sc, cand, cidx, kept, kidx)
    assert isinstance(od, OracleDetector)
    names = [n for s in HEAD_STRIDES for n in head_names(s)]
    cands = post.decode({n: a[None] for n, a in zip(names, h9)}, sc.hw[0], sc.hw[1], dh.THR, ratios=ratios)
    dets = post.nms(list(cands), dh.NMS)
    assert [d.anchor_index for d in cands] == cidx.tolist()
    assert [d.anchor_index for d in dets] == kidx.tolist()
    rows = lambda ds: np.stack([d.as_row() for d in ds]) if ds else np.zeros((0, 15), np.float32)
    assert np.array_equal(rows(dets), kept)
    assert np.array_equal(rows(cands), cand)
    if sc.na == 2:                                                             # and the detector call itself, which decodes "net3"
        ref = od.detect(sc.frame(), dh.THR, dh.NMS, net_hw=sc.hw)
        assert ref.anchor_indices().tolist() == kidx.tolist() and np.array_equal(ref.rows(), kept)
    print(f"designed heads (oracle) {name}: {len(cidx)} candidates, {len(kidx)} kept, {len(np.unique(cand[:, 0]))} distinct scores")
    if build_ref.available() and sc.max_tie <= REF_MAX_TIE:
        r = build_ref.ReferenceRetinaFace(sc.hw[0], sc.hw[1], network=dh.network_of(sc), head_anchors=sc.na)
        try:
            r.set_heads(0, h9)
            assert np.array_equal(r.postprocess(0, dh.THR), kept)             # all 15 floats of every face, in order
        finally:
            r.close()


REF_MAX_TIE = 16


def test_the_four_anchor_scenarios_are_compared_with_the_reference_build():
    """Every a4_* scenario stays within REF_MAX_TIE, so none is left out of the comparison above where the reference build is present."""
    assert dh.SCENARIOS4 and all(dh.SCENARIOS[n].max_tie <= REF_MAX_TIE and dh.SCENARIOS[n].na == 4 for n in dh.SCENARIOS4)


@pytest.mark.parametrize("hw", dh.SIZES4, ids=dh.tag4)
def test_swapping_width_and_height_moves_the_asymmetric_boxes(wired, hw):
    """`a4_asym`: bbox_pred restated with `width` and `height` exchanged in the centre terms moves every kept box by more than 1 px -- four
    orders of magnitude beyond the 1e-4 px of the GPU judge -- and landmark_pred with `height` replaced by `width` moves every kept
    landmark y by more than 1 px.  dh.swap_moves, which the GPU test applies to the device's rows, predicts the box figure."""
    from oracle import retinaface_post as post
    sc = dh.SCENARIOS[f"a4_asym_{dh.tag4(hw)}"]
    h9 = _oracle_heads(wired[sc.heads], sc)
    cand, cidx, kept, kidx = obuild.decode_nms(h9, hw[0], hw[1], dh.THR, dh.NMS, ratios=dh.RATIOS4)
    assert len(kidx) == 12
    base = post.base_anchors(dh.RATIOS4)[8]
    st, an, gp = dh.anchor_numbers(kidx, hw, 4)
    w8 = hw[1] // 8
    for row, i, a, g in zip(kept, kidx, an, gp):
        anchor = base[a] + np.array([8 * (g % w8), 8 * (g // w8)] * 2, np.float32)
        reg = [h9[7][a * 4 + c].reshape(-1)[g] for c in range(4)]
        pts = [h9[8][a * 10 + c].reshape(-1)[g] for c in range(10)]
        good = np.array(post.clip_box(post.bbox_pred(anchor, reg), hw[1], hw[0]))
        assert np.array_equal(good, row[1:5])
        x1, y1, x2, y2 = anchor
        turned = np.array([x1, y1, x1 + (y2 - y1), y1 + (x2 - x1)], np.float32)      # the anchor with width and height exchanged ...
        bad = np.array(post.bbox_pred(turned, reg))
        ctr = lambda b: np.array([b[0] + b[2], b[1] + b[3]]) / 2
        shift = ctr(turned) - ctr(anchor)                                           # ... recentred: what is left is dx * height, dy * width
        moved = np.abs(ctr(bad) - shift - ctr(good)).max()
        assert moved > 1.0 and abs(moved - dh.swap_moves(row, int(i), hw)) < 1e-2, moved
        ys = np.array(post.landmark_pred(anchor, pts)[1])
        assert np.array_equal(ys, row[10:15])
        width, height = x2 - x1 + 1, y2 - y1 + 1
        ys_bad = np.array([np.float32(pts[2 * k + 1]) * width + (y1 + 0.5 * (height - 1)) for k in range(5)])
        assert np.abs(ys_bad - ys)[[0, 1, 3, 4]].min() > 1.0                         # (landmark 2 has offset 0 in y)


def test_pairs_iou_is_a_threshold_that_decides(wired):
    """`pairs`: with nms_threshold equal to the fp32 IoU of the picked pair the second box stays (`>` is strict), one float below it goes --
    in the C restatement, which is the judge of the GPU test at that threshold."""
    sc = dh.SCENARIOS["pairs"]
    h9 = _oracle_heads(wired[sc.heads], sc)
    cand, cidx, _, _ = obuild.decode_nms(h9, sc.hw[0], sc.hw[1], dh.THR, dh.NMS)
    srt, sidx = dh.sorted_candidates(cand, cidx)
    i, j = dh.pairs_pick(srt)
    iou = dh.iou_f32(srt[i, 1:5], srt[j, 1:5])
    at = obuild.decode_nms(h9, sc.hw[0], sc.hw[1], dh.THR, float(iou))[3].tolist()
    below = obuild.decode_nms(h9, sc.hw[0], sc.hw[1], dh.THR, float(np.nextafter(iou, np.float32(0))))[3].tolist()
    assert int(sidx[i]) in at and int(sidx[j]) in at
    assert int(sidx[i]) in below and int(sidx[j]) not in below
