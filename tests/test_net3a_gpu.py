"""The four-anchor head path ("net3a": head_kernel<T, 4>, its weight packers over 64 output channels, the non-square anchors) end to end
on natural frames (`-m gpu`), on the widened shipped models of tests/net3a_models.py -- 64 distinct head channels per stride, both stems.

  int8    bit for bit against oracle/int8_forward.py of the same spec (raw heads, every int8 activation, candidates and detections), at
          64 x 96 and 96 x 160, thresholds 0.5 and 0.02, images 0 and 2 of a three-image launch judged inside it
  batch   nineteen distinct 64 x 96 frames in one call of a max_batch 8 engine (chunks 8 + 8 + 3), fp32, fp16 and int8 at threshold
          0.02: every image equals, as bytes, its single-image call
Every anchor number 0..3 occurs among the candidates of the judged frames at each threshold: asserted on the device's own blobs.
The fp32 / fp16 head launches are judged in tests/test_launch_interval_gpu.py, decode and NMS on designed heads in
tests/test_designed_heads_gpu.py.  No tolerance here is new: the bars are those of test_edge_net_sizes_every_precision at two anchors."""
import numpy as np
import pytest

import net3a_models as nm
from conftest import STEMS
from oracle.caffe_forward import HEAD_STRIDES, head_names
from test_gpu_parity import _assert_int8_image_bit_exact, _edge_frame, _key, rfa  # noqa: F401  (rfa: fixture)

pytestmark = pytest.mark.gpu

FP32, FP16, INT8 = 0, 1, 2
SIZES = ((64, 96), (96, 160))
THRESHOLDS = (0.5, 0.02)


@pytest.fixture(scope="module")
def model_dir(nets, tmp_path_factory):
    """the widened models of both stems, written at run time (nothing is stored), read back with the oracle's own reader"""
    from oracle.caffe_io import read_rfw
    d = nm.write_model_dir(nets, str(tmp_path_factory.mktemp("net3a")))
    specs = {s: read_rfw(f"{d}/{s}.rfw") for s in STEMS}
    assert all(n.int8_qweights == {} and n.int8_scales for n in specs.values())
    return d, specs


def _engine(rfa, d, stem, prec, hw, **kw):
    kw.setdefault("max_detections", 1024)
    return rfa.RetinaFace(d, "net3a", 0.4, precision=prec, net_hw=hw, model_stem=stem, plan_cache=False, **kw)


def _candidate_anchors(det, n_images, thr):
    probs = [np.stack([det.get_output(head_names(s)[0], i) for i in range(n_images)]) for s in HEAD_STRIDES]
    return nm.anchors_with_candidates(probs, thr)


@pytest.mark.parametrize("hw", SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("stem", STEMS)
def test_int8_four_anchor_engine_is_bit_exact(rfa, model_dir, base_frame, stem, hw):
    """The int8 head packer over 64 output channels (per-channel mult / bias) and head_kernel<int8_t, 4>: three distinct frames in one
    launch, images 0 and 2 judged inside it at both thresholds.  Then the default engine (graph replay) returns the same bytes."""
    from oracle.int8_forward import Int8Net
    d, specs = model_dir
    q = Int8Net(specs[stem])
    frames = [_edge_frame(base_frame, hw, k) for k in range(3)]
    det = _engine(rfa, d, stem, INT8, hw, max_batch=8, keep_outputs=True, use_graph=False)
    eager = {}
    try:
        for thr in THRESHOLDS:
            res = det.detectBatchImages(frames, thr)
            assert not det.truncated and det.get_output(head_names(8)[0], 0).shape[0] == 8
            kept = [_assert_int8_image_bit_exact(det, q, img, hw, thr, res[img], ratios=nm.RATIOS) for img in (0, 2)]
            assert _candidate_anchors(det, 3, thr) == {0, 1, 2, 3}, thr
            print(f"int8 net3a {stem} {hw[0]}x{hw[1]} thr {thr}: bit-exact, {det.last_candidate_counts(3)} candidates, {kept} kept (images 0, 2)")
            eager[thr] = _key(res)
    finally:
        det.close()
    det = _engine(rfa, d, stem, INT8, hw, max_batch=8)
    try:
        for thr in THRESHOLDS:
            assert _key(det.detectBatchImages(frames, thr)) == eager[thr], thr
    finally:
        det.close()


@pytest.mark.parametrize("prec", [FP32, FP16, INT8], ids=["fp32", "fp16", "int8"])
@pytest.mark.parametrize("stem", STEMS)
def test_four_anchor_batch_composition(rfa, model_dir, base_frame, stem, prec):
    """Nineteen distinct 64 x 96 frames through a max_batch 8 engine (8 + 8 + 3): image i of a launch reads its own 64 head channels and
    writes its own candidates -- every image's result equals its single-image call byte for byte."""
    d, _ = model_dir
    hw = (64, 96)
    frames = [_edge_frame(base_frame, hw, k) for k in range(19)]
    assert len({f.tobytes() for f in frames}) == 19
    det = _engine(rfa, d, stem, prec, hw, max_batch=8, keep_outputs=True, use_graph=False)
    try:
        batch = det.detectBatchImages(frames, 0.02)
        assert not det.truncated
        single, seen = [], set()
        for f in frames:
            single.append(det.detect(f, 0.02))
            seen |= _candidate_anchors(det, 1, 0.02)
        assert _key(batch) == _key(single)
        assert seen == {0, 1, 2, 3} and sum(len(r) for r in batch) >= 19
    finally:
        det.close()
