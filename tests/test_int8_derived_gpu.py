"""The int8 engine held BIT-exact to oracle/int8_forward.py on the derived calibration tables and the derived weight set of
tests/int8_derived.py (`-m gpu`).  The shipped tables (25 % head-room) and the trained weights leave the top clamp of every requantising
epilogue, the per-tensor path of mnet25, the zero-row branches of the weight packer and the > 256-candidate NMS path with int8 scores
cold; these sets reach them, and the bar on any table and any weights is exactness, so no tolerance is invented here.  What the sets
reach is asserted on the reference alone in tests/test_int8_oracle.py (the coverage conditions), and again below on the device's own
blobs.  The <= 1 LSB / 2 % front-end bar of the shipped-table tests is NOT applied: it belongs to the shipped scale.  fp32 / fp16
engines on derived weights are out of scope."""
import numpy as np
import pytest

import int8_derived as drv
from conftest import STEMS
from oracle.retinaface_post import preprocess_trt_identity
from test_gpu_parity import _assert_int8_image_bit_exact, _edge_frame, _int8_start_blob, _key, rfa  # noqa: F401  (rfa: fixture)

pytestmark = pytest.mark.gpu

INT8 = 2
HW = (352, 608)               # odd partial tiles; at 64 x 96 one or two tensors stay unsaturated under the same tables
SMALL = (64, 96)
THRESHOLDS = (0.5, 0.02)


def _packed(nets, stem, name, tmp_path):
    """the derived set packed into <tmp_path>/<stem>.rfw; the oracle is built from that file with the oracle's own reader"""
    from oracle.caffe_io import read_rfw, write_rfw
    from oracle.int8_forward import Int8Net
    path = str(tmp_path / (stem + ".rfw"))
    write_rfw(drv.derive(nets[stem], name), path)
    net = read_rfw(path)
    assert net.int8_qweights == {}
    q = Int8Net(net)
    forward, seen = q.forward_from, {}

    def forward_once(blob, x):          # the same start blob (one frame, two thresholds) is continued once
        key = (blob, x.shape, x.tobytes())
        if key not in seen:
            seen[key] = forward(blob, x)
        return seen[key]
    q.forward_from = forward_once
    return q


def _engine(rfa, tmp_path, stem, hw, **kw):
    return rfa.RetinaFace(str(tmp_path), "net3", 0.4, precision=INT8, net_hw=hw, model_stem=stem, plan_cache=False, **kw)


@pytest.mark.parametrize("name", drv.ALL)
@pytest.mark.parametrize("stem", STEMS)
def test_int8_engine_is_bit_exact_on_derived_sets(rfa, nets, oracles, base_frame, tmp_path, stem, name):
    """One 352 x 608 frame, eager, thresholds 0.5 and 0.02: every int8 activation the engine exposes, the raw heads, candidates and
    detections against the integer oracle built from the same container (_assert_int8_image_bit_exact).
      pc_half, pt_quarter  every exposed tensor holds its top code somewhere ON THE DEVICE: the pass covers each epilogue's top clamp
                           (the depthwise mids and `_plus` tensors never leave the kernels; the oracle has them at their top code on
                           this frame -- tests/test_int8_oracle.py -- so a missing clamp there changes the tensors behind them)
      pc_quarter           the float front end's clamp: the first int8 blob is 127 wherever the fp32 oracle is >= 135 quanta (127 + 8:
                           twice the 4 quanta that the <= 1 LSB bar at the shipped scale allows at a quarter of it), >= 1000 positions
      pt_eighth            > 256 candidates at 0.02 without truncation (max_detections 512): the NMS kernel's bitonic path
    Then the default engine (graph replay, coalescing) must give the byte-identical detections of the eager run that was checked."""
    q = _packed(nets, stem, name, tmp_path)
    assert q.per_channel == (not name.startswith("pt_"))
    frame = _edge_frame(base_frame, HW)
    cap = dict(max_detections=512) if name == "pt_eighth" else {}
    det = _engine(rfa, tmp_path, stem, HW, max_batch=1, keep_outputs=True, use_graph=False, **cap)
    try:
        eager, kept = [], []
        for thr in THRESHOLDS:
            got = det.detect(frame, thr)
            kept.append(_assert_int8_image_bit_exact(det, q, 0, HW, thr, got))
            assert not det.truncated
            eager.append(_key([got]))
        ncand = det.last_candidate_counts(1)[0]
        start = _int8_start_blob(det)
        x = det.debug_activation(start + "#raw", 0)
        acts = q.forward_from(start, x.astype(np.int8))
        exposed = {}
        for n in acts:
            if n == "__heads__":
                continue
            try:
                exposed[n] = det.debug_activation(n + "#raw", 0)
            except RuntimeError:
                continue
        top = sum(int((a == 127).sum()) for a in exposed.values()) / sum(a.size for a in exposed.values())
        print(f"int8 derived {stem} {name}: bit-exact from {start}; {top:.4f} of the device's {len(exposed)} exposed tensors' quanta at the top code; "
              f"{ncand} candidates at {THRESHOLDS[1]}, {kept[0]} / {kept[1]} detections at {THRESHOLDS[0]} / {THRESHOLDS[1]}")
        if name in ("pc_half", "pt_quarter"):
            assert len(exposed) >= 22, sorted(exposed)            # the start blob + the >= 21 the bit-exact helper compared
            cold = [n for n, a in exposed.items() if not (a == 127).any()]
            assert not cold, cold
        if name == "pc_quarter":
            r = oracles[stem].forward(preprocess_trt_identity(frame, *HW), keep_all=True)[start][0].transpose(1, 2, 0).astype(np.float32)
            over = (r * (np.float32(1) / q.scale_of_blob[start]).reshape(1, 1, -1)).astype(np.float32) >= 135
            assert over.sum() >= 1000, int(over.sum())
            assert np.all(x[over] == 127), (int((x[over] != 127).sum()), int(over.sum()), float(x[over].min()))
        if name == "pt_eighth":
            assert ncand > 256 and kept[1] > 0, (ncand, kept)
    finally:
        det.close()
    det = _engine(rfa, tmp_path, stem, HW, max_batch=1, **cap)
    try:
        for thr, want in zip(THRESHOLDS, eager):
            assert _key([det.detect(frame, thr)]) == want, thr
            assert not det.truncated
    finally:
        det.close()


@pytest.mark.parametrize("name", ["degenerate", "pc_quarter"])
@pytest.mark.parametrize("stem", STEMS)
def test_int8_derived_sets_multi_image(rfa, nets, base_frame, tmp_path, stem, name):
    """Three distinct 64 x 96 frames in one call of a max_batch 8 engine (a partly filled launch, maps of 2 x 3 at stride 32): every
    image bit-exact inside its launch, on the dead / saturated channels of `degenerate` and under the deep saturation of `pc_quarter`."""
    q = _packed(nets, stem, name, tmp_path)
    frames = [_edge_frame(base_frame, SMALL, k) for k in range(3)]
    det = _engine(rfa, tmp_path, stem, SMALL, max_batch=8, keep_outputs=True, use_graph=False)
    try:
        res = det.detectBatchImages(frames, 0.02)
        for i in range(3):
            _assert_int8_image_bit_exact(det, q, i, SMALL, 0.02, res[i])
    finally:
        det.close()
