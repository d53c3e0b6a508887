"""decode_anchor, the tail of head_kernel and nms_kernel on DESIGNED head outputs (`-m gpu`): candidate counts on every boundary of the
three sort regimes, exact score ties, the cap and max_det bounds, thresholds at equality and boxes at decode's edges -- none of which the
head blobs of the trained networks ever produce.  The heads are driven through pass-through weight sets and painted frames
(tests/designed_heads.py, whose SCENARIOS table names every frame used here); tests/test_designed_heads_host.py shows on the CPU oracle
that each scenario reaches its condition.

The judge is the existing one (test_postprocessing_is_exact_given_the_gpu_head_blobs): the device's OWN head blobs go into the plain-C
restatement; candidate counts equal, kept anchor indices equal in order, scores np.array_equal, every other field within 1e-4 px.  No
oracle forward runs here and no tolerance is new.  Each scenario's condition is asserted again on the restatement's result for the
device's blobs (designed_heads.check), so a frame that missed its regime on the device fails; tie conditions only for fp32.  Engines: fp32
and fp16 on mnet25's structure; every test checks an eager engine (keep_outputs) and then requires the default engine (graph replay) to
return byte-identical detections.

The four-anchor scenarios (a4_*, "net3a" engines on widened wire sets, 128 x 160 and 96 x 160) go through the same judge; the restatement
is given the preset's ratios, nothing else differs."""
import time

import numpy as np
import pytest

import designed_heads as dh
from oracle import build as obuild
from oracle.caffe_forward import HEAD_STRIDES, head_names
from test_gpu_parity import _key, rfa  # noqa: F401  (rfa: fixture)

pytestmark = pytest.mark.gpu

FP32, FP16 = 0, 1
PRECS = [FP32, FP16]
STEM = "mnet25"
SC = dh.SCENARIOS


@pytest.fixture
def packed(nets, tmp_path):
    """pack(head set) -> the directory that holds the wire set with those heads as mnet25.rfw"""
    def pack(heads):
        from oracle.caffe_io import read_rfw, write_rfw
        d = tmp_path / heads
        d.mkdir(exist_ok=True)
        path = str(d / (STEM + ".rfw"))
        write_rfw(dh.wire_net(nets[STEM], heads), path)
        assert read_rfw(path).int8_qweights == {}
        return str(d)
    return pack


def _engine(rfa, model_dir, prec, hw, nms=dh.NMS, eager=False, network="net3", **kw):
    if eager:
        kw.update(keep_outputs=True, use_graph=False)
    kw.setdefault("max_batch", 1)
    kw.setdefault("max_detections", 4096)
    return rfa.RetinaFace(model_dir, network, nms, precision=prec, net_hw=hw, model_stem=STEM, plan_cache=False, **kw)


def _rows(got):
    return np.stack([d.as_row() for d in got]) if got else np.zeros((0, 15), np.float32)


def _restate(det, img, hw, thr, nms, ratios=(1.0,)):
    heads9 = [det.get_output(n, img) for s in HEAD_STRIDES for n in head_names(s)]
    return obuild.decode_nms(heads9, hw[0], hw[1], thr, nms, ratios=ratios)


def _judge(det, hw, got, thr=dh.THR, nms=dh.NMS, img=0, max_det=None, ratios=(1.0,)):
    """The device's detections of image `img` against the restatement fed the device's own head blobs."""
    cand, cidx, kept, kidx = _restate(det, img, hw, thr, nms, ratios)
    assert det.last_candidate_counts(img + 1)[img] == len(cidx)
    want_idx, want = (kidx, kept) if max_det is None else (kidx[:max_det], kept[:max_det])
    assert [d.anchor_index for d in got] == want_idx.tolist()
    rows = _rows(got)
    assert np.array_equal(rows[:, 0], want[:, 0])
    assert np.abs(rows - want).max(initial=0.0) <= 1e-4
    return cand, cidx, kept, kidx


def _iou_matrix(a, b):
    """float32 +1-convention IoU of every box of a with every box of b, the restatement's op order; 0 where it skips the pair"""
    one = np.float32(1)
    area1 = ((a[:, 2] - a[:, 0] + one) * (a[:, 3] - a[:, 1] + one))[:, None]
    area2 = ((b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one))[None, :]
    x = np.maximum(a[:, None, 0], b[None, :, 0])
    y = np.maximum(a[:, None, 1], b[None, :, 1])
    w = np.minimum(a[:, None, 2], b[None, :, 2]) - x + one
    h = np.minimum(a[:, None, 3], b[None, :, 3]) - y + one
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = inter / (area1 + area2 - inter)
    return np.where((w <= 0) | (h <= 0), np.float32(0), iou)


def _assert_overflow(det, hw, got, true_n, nms=dh.NMS, ratios=(1.0,)):
    """More candidates than the cap: which of them won a slot is not deterministic.  What must hold: truncated, the true count, every
    returned row bit-equal to a candidate of the restatement, (score desc, anchor asc) order, and no row suppressing another."""
    cand, cidx, _, _ = _restate(det, 0, hw, dh.THR, nms, ratios)
    assert det.truncated
    assert len(cidx) == true_n and det.last_candidate_counts(1)[0] == true_n
    assert len(got) > 0
    rows, idx = _rows(got), np.array([d.anchor_index for d in got])
    where = {int(a): i for i, a in enumerate(cidx)}
    assert len(set(idx.tolist())) == len(idx) and all(int(a) in where for a in idx)
    assert np.array_equal(rows.view(np.uint32), cand[[where[int(a)] for a in idx]].view(np.uint32))
    order = np.lexsort((idx, -rows[:, 0].astype(np.float64)))
    assert np.array_equal(order, np.arange(len(idx)))
    for lo in range(0, len(rows), 512):
        m = _iou_matrix(rows[lo:lo + 512, 1:5], rows[:, 1:5])
        m[np.arange(len(m)), lo + np.arange(len(m))] = 0
        assert not (m > np.float32(nms)).any()


def _run_rows(rfa, packed, prec, hw, names, after=None, **kw):
    """Each named scenario's frame through an eager engine (judged, condition checked), then through the default engine (byte-identical);
    one pair of engines per head set the scenarios name.  `after(det, results, frames)` runs extra checks on the eager `std` engine.
    Returns {name: restatement result}."""
    res = {}
    for heads in dict.fromkeys(SC[n].heads for n in names):
        res.update(_run_set(rfa, packed(heads), prec, hw, [n for n in names if SC[n].heads == heads], after if heads == "std" else None, **kw))
    return res


def _run_set(rfa, model_dir, prec, hw, names, after, **kw):
    frames = {n: SC[n].frame() for n in names}
    eager, res = {}, {}
    assert len({SC[n].na for n in names}) == 1 and all(SC[n].hw == hw for n in names)
    ratios = dh.ratios_of(SC[names[0]])
    kw["network"] = dh.network_of(SC[names[0]])
    det = _engine(rfa, model_dir, prec, hw, eager=True, **kw)
    try:
        for n in names:
            t0 = time.perf_counter()
            got = det.detect(frames[n], dh.THR)
            ms = (time.perf_counter() - t0) * 1e3
            res[n] = _judge(det, hw, got, ratios=ratios)
            assert not det.truncated, n
            dh.check(SC[n], *res[n], ties=prec == FP32)
            eager[n] = _key([got])
            print(f"designed heads {('fp32', 'fp16')[prec]} {n}: {len(res[n][1])} candidates, {len(got)} kept, {len(np.unique(res[n][0][:, 0]))} "
                  f"distinct scores, detect {ms:.2f} ms")
        if after:
            after(det, res, frames)
    finally:
        det.close()
    det = _engine(rfa, model_dir, prec, hw, **kw)
    try:
        for n in names:
            assert _key([det.detect(frames[n], dh.THR)]) == eager[n], n
            assert not det.truncated
    finally:
        det.close()
    return res


SMALL_ROWS = [f"counts{n}" for n in (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513)] + \
             [f"ties{n}_{t}" for n in (64, 257) for t in ("tiny", "mid", "huge")] + ["saturated", "lane63", "edges"]
LARGE_ROWS = ["counts4095", "counts4096", "ties4096_tiny", "ties4096_mid", "ties4096_huge"]


@pytest.mark.parametrize("prec", PRECS)
def test_counts_ties_lane63_and_decode_edges_on_the_small_net(rfa, packed, prec):
    """128 x 160 (640 stride-8 anchors): candidate counts 0, 1, 63 | 64 | 65, 255 | 256 | 257, 511 | 512 | 513 (single-wave rank sort, 256-thread
    rank sort, bitonic network with 1, 0 and 511 pad keys); 64 and 257 candidates of ONE score at three box sizes (all kept / some / one);
    scores saturated to 1.0f; a survivor at lane 63 of the first 64-block that suppresses position 64; decode at its edges.  Then the
    threshold at equality: `detect` again with a score read from the device's prob blob -- that anchor is no candidate."""
    def threshold_equality(det, res, frames):
        cand, cidx = res["counts65"][:2]
        s = np.sort(cand[:, 0])[32]
        got = det.detect(frames["counts65"], float(s))
        c2, i2, _, _ = _judge(det, dh.SMALL, got, thr=float(s))
        assert len(i2) == int((cand[:, 0] > s).sum()) == 32 and int(cidx[cand[:, 0] == s][0]) not in i2.tolist()
    _run_rows(rfa, packed, prec, dh.SMALL, SMALL_ROWS, after=threshold_equality)


@pytest.mark.parametrize("prec", PRECS)
def test_counts_and_ties_at_4096_on_the_large_net(rfa, packed, prec):
    """384 x 384 (4608 stride-8 anchors): 4095 and 4096 candidates (bitonic network with one pad key and with none, the cap reached and not
    exceeded); 4096 candidates of one score: a walk with 4096 survivors, one that enters 64-blocks fully suppressed, one with a single
    survivor.  Then the default cap exceeded: all 4608 gates open."""
    _run_rows(rfa, packed, prec, dh.LARGE, LARGE_ROWS)
    model = packed("std")
    frame = SC["exact4608"].frame()
    for eager in (True, False):
        det = _engine(rfa, model, prec, dh.LARGE, eager=True) if eager else _engine(rfa, model, prec, dh.LARGE, keep_outputs=True)
        try:
            _assert_overflow(det, dh.LARGE, det.detect(frame, dh.THR), 4608)
        finally:
            det.close()


@pytest.mark.parametrize("prec", PRECS)
def test_ties_across_strides(rfa, packed, prec):
    """All three strides wired to one score on coincident cells: 36 candidates, 12 per stride; the order among them is the GLOBAL anchor
    index (anchor_offset of each stride)."""
    _run_rows(rfa, packed, prec, dh.SMALL, ["strides"])


@pytest.mark.parametrize("prec", PRECS)
def test_iou_threshold_at_equality(rfa, packed, prec):
    """A second engine whose nms_threshold IS the fp32 IoU (+1 convention, the restatement's op order) of the best box and the one box that
    overlaps it: `iou > thr` is false at equality, so both stay; one float below, the second goes.  Restatement and device must agree."""
    model = packed("std")
    frame = SC["pairs"].frame()
    res = _run_rows(rfa, packed, prec, dh.SMALL, ["pairs"])["pairs"]
    srt, sidx = dh.sorted_candidates(res[0], res[1])
    i, j = dh.pairs_pick(srt)
    iou = dh.iou_f32(srt[i, 1:5], srt[j, 1:5])
    for thr, stays in ((iou, True), (np.nextafter(iou, np.float32(0)), False)):
        det = _engine(rfa, model, prec, dh.SMALL, nms=float(thr), eager=True)
        try:
            got = det.detect(frame, dh.THR)
            _, _, _, kidx = _judge(det, dh.SMALL, got, nms=float(thr))
            assert (int(sidx[j]) in kidx.tolist()) == stays and int(sidx[i]) in kidx.tolist(), (float(thr), stays)
            want = _key([got])
        finally:
            det.close()
        det = _engine(rfa, model, prec, dh.SMALL, nms=float(thr))
        try:
            assert _key([det.detect(frame, dh.THR)]) == want
        finally:
            det.close()


@pytest.mark.parametrize("prec", PRECS)
def test_max_detections_bound(rfa, packed, prec):
    """max_detections = 8: eight survivors fill the block without truncation; nine report `truncated` and return the restatement's first 8."""
    model = packed("std")
    frames = {n: SC[n].frame() for n in ("kept8", "kept9")}
    want = {}
    for eager in (True, False):
        det = _engine(rfa, model, prec, dh.SMALL, eager=eager, max_detections=8)
        try:
            for n, over in (("kept8", False), ("kept9", True), ("kept8", False)):
                got = det.detect(frames[n], dh.THR)
                assert det.truncated == over and len(got) == 8, (n, det.truncated, len(got))
                if eager:
                    res = _judge(det, dh.SMALL, got, max_det=8)
                    dh.check(SC[n], *res, ties=prec == FP32)
                    want[n] = _key([got])
                else:
                    assert _key([got]) == want[n]
        finally:
            det.close()


@pytest.mark.parametrize("prec", PRECS)
def test_candidate_cap_bound(rfa, packed, prec):
    """max_candidates = 64: 64 candidates fill the cap exactly (not truncated, judged in full); 65 overflow it (`slot < cap`, `n > cap`); then
    64 again: the counter was re-armed."""
    model = packed("std")
    frames = {n: SC[n].frame() for n in ("exact64", "exact65")}
    want = None
    for eager in (True, False):
        det = _engine(rfa, model, prec, dh.SMALL, eager=True, max_candidates=64) if eager else \
            _engine(rfa, model, prec, dh.SMALL, keep_outputs=True, max_candidates=64)
        try:
            for n in ("exact64", "exact65", "exact64"):
                got = det.detect(frames[n], dh.THR)
                if n == "exact65":
                    _assert_overflow(det, dh.SMALL, got, 65)
                    continue
                assert not det.truncated
                res = _judge(det, dh.SMALL, got)
                dh.check(SC[n], *res, ties=prec == FP32)
                want = want or _key([got])
                assert _key([got]) == want
        finally:
            det.close()


@pytest.mark.parametrize("prec", PRECS)
def test_mixed_regimes_in_one_launch(rfa, packed, prec):
    """The frames of 0, 1, 64, 65, 257 and 4096 candidates in ONE detectBatchImages call of a max_batch 8 engine, in that order and reversed:
    one NMS workgroup per image, each in another regime (the early exit of waves 1..3 beside full workgroups), the counters re-armed between
    the calls.  Every image is judged inside its launch and equals its solo result byte for byte."""
    model = packed("std")
    names = [f"mixed{n}" for n in dh.MIXED]
    frames = [SC[n].frame() for n in names]
    det = _engine(rfa, model, prec, dh.LARGE, eager=True, max_batch=8)
    try:
        got = det.detectBatchImages(frames, dh.THR)
        assert not det.truncated
        for i, n in enumerate(names):
            dh.check(SC[n], *_judge(det, dh.LARGE, got[i], img=i), ties=prec == FP32)
        want = _key(got)
        assert _key(det.detectBatchImages(frames[::-1], dh.THR)) == want[::-1]
        assert [_key([det.detect(f, dh.THR)])[0] for f in frames] == want
    finally:
        det.close()
    det = _engine(rfa, model, prec, dh.LARGE, max_batch=8)
    try:
        assert [_key([det.detect(f, dh.THR)])[0] for f in frames] == want
        assert _key(det.detectBatchImages(frames, dh.THR)) == want
        assert _key(det.detectBatchImages(frames[::-1], dh.THR)) == want[::-1]
        assert _key(det.detectBatchImages(frames, dh.THR)) == want
    finally:
        det.close()


# ------------------------------------------------------------------------------------------------------------ four anchors per cell
SIZES4 = dh.SIZES4
A4_ROWS = [f"a4_alone{a}" for a in range(4)] + ["a4_all", "a4_alltied", "a4_asym", "a4_clip", "a4_count300"]


def _a4(name, hw):
    return f"{name}_{dh.tag4(hw)}"


@pytest.mark.parametrize("hw", SIZES4, ids=dh.tag4)
@pytest.mark.parametrize("prec", PRECS)
def test_four_anchor_head_on_designed_outputs(rfa, packed, prec, hw):
    """head_kernel<T, 4> and decode_anchor on the non-square anchors of "net3a": each anchor's gate alone on all three strides (every index
    is anchor_offset + a * hw + gp of the open anchor, with distinct dx, dy per cell); all four anchors of a cell with distinct scores and
    tied (the square and the tall box of a cell overlap: NMS across the four); dx != dy on the 26 x 40 and 13 x 20 anchors, where taking
    the width for the height moves a box by more than 1 px; clipping on all four borders with x2 - x1 < 0; 300 candidates (the bitonic
    path).  128 x 160 fills the blocks of 64 pixels of the stride-8 map exactly; at 96 x 160 the last block of every level is partial."""
    res = _run_rows(rfa, packed, prec, hw, [_a4(n, hw) for n in A4_ROWS])
    for a in range(4):
        cidx = res[_a4(f"a4_alone{a}", hw)][1]
        assert sorted(cidx.tolist()) == SC[_a4(f"a4_alone{a}", hw)].expect()


@pytest.mark.parametrize("hw", SIZES4, ids=dh.tag4)
@pytest.mark.parametrize("prec", PRECS)
def test_four_anchor_max_detections_bound(rfa, packed, prec, hw):
    """test_max_detections_bound at A = 4: eight survivors (two of each anchor) fill max_detections = 8, nine report `truncated`."""
    model = packed("std4")
    names = [_a4(n, hw) for n in ("a4_kept8", "a4_kept9")]
    frames = {n: SC[n].frame() for n in names}
    want = {}
    for eager in (True, False):
        det = _engine(rfa, model, prec, hw, eager=eager, network="net3a", max_detections=8)
        try:
            for n, over in ((names[0], False), (names[1], True), (names[0], False)):
                got = det.detect(frames[n], dh.THR)
                assert det.truncated == over and len(got) == 8, (n, det.truncated, len(got))
                if eager:
                    res = _judge(det, hw, got, max_det=8, ratios=dh.RATIOS4)
                    dh.check(SC[n], *res, ties=prec == FP32)
                    want[n] = _key([got])
                else:
                    assert _key([got]) == want[n]
        finally:
            det.close()


@pytest.mark.parametrize("hw", SIZES4, ids=dh.tag4)
@pytest.mark.parametrize("prec", PRECS)
def test_four_anchor_candidate_cap_bound(rfa, packed, prec, hw):
    """test_candidate_cap_bound at A = 4: 64 candidates (sixteen cells, all four anchors) fill max_candidates = 64 exactly, 65 overflow it,
    then 64 again."""
    model = packed("std4")
    n64, n65 = _a4("a4_count64", hw), _a4("a4_count65", hw)
    frames = {n: SC[n].frame() for n in (n64, n65)}
    want = None
    for eager in (True, False):
        det = _engine(rfa, model, prec, hw, eager=True, network="net3a", max_candidates=64) if eager else \
            _engine(rfa, model, prec, hw, keep_outputs=True, network="net3a", max_candidates=64)
        try:
            for n in (n64, n65, n64):
                got = det.detect(frames[n], dh.THR)
                if n == n65:
                    _assert_overflow(det, hw, got, 65, ratios=dh.RATIOS4)
                    continue
                assert not det.truncated
                res = _judge(det, hw, got, ratios=dh.RATIOS4)
                dh.check(SC[n], *res, ties=prec == FP32)
                want = want or _key([got])
                assert _key([got]) == want
        finally:
            det.close()
