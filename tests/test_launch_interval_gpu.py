"""Per-launch parity of the fp32 and fp16 engines (`-m gpu`): every launch judged ALONE against the float64 model of tests/launch_ref.py.

The launch's inputs are the device's own stored tensors (debug_activation, or the frame), its constants are what the packer emitted
(rf_plan_folded), and every element of every stored output must lie inside the interval the arithmetic allows -- no element excluded,
nothing relative to the tensor's range, and therefore valid on weights nobody trained (`degenerate`, `ragged`).  Three distinct frames per
call, all three judged: every launch indexes images beyond the first.  (A launch walks tiles across images only where it has more tiles
than resident workgroups, which none does at these sizes: test_tile_walk_gpu.py forces the walk at the same sizes and holds every stored
tensor to the bytes judged here, and test_gpu_parity.py's batch-composition tests hold the production grids end to end at full size.)  Sizes: 64 x 96 (every tile of every kernel partial, a 2 x 3
stride-32 map), 96 x 160 (odd tile counts, 3 x 5), 352 x 608 (mnet25: the odd-partial-tile size, and the only size here whose stride-8
map is large enough for the fp16 engine's warp-specialised rf_c1_aggr instance; mnet-deconv-0517 runs that one launch there).
After each eager engine is judged, the default engine (graph replay) must return byte-identical detections on the same frames.
The four-anchor head launches ("net3a" engines on the widened models of tests/net3a_models.py) are judged the same way at the two small sizes.
"""
import os

import numpy as np
import pytest

import launch_ref as lr
import net3a_models as nm
from conftest import ASSETS, STEMS

pytestmark = pytest.mark.gpu

FP32, FP16 = lr.FP32, lr.FP16
PNAME = {FP32: "fp32", FP16: "fp16"}
SMALL, BIG = lr.SMALL_SIZES, lr.BIG_SIZE
STATS = []           # every judged output of the session, written out by the last test of the module


@pytest.fixture(scope="module")
def rfa(built_lib):
    import retinaface_amd
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need the GPU box"
    return retinaface_amd


@pytest.fixture(scope="module")
def model_dirs(nets, tmp_path_factory):
    """weight set -> model directory (shipped: the assets; derived: written at run time, nothing is stored)"""
    dirs = lr.weight_set_dirs(nets, ASSETS, lambda name: str(tmp_path_factory.mktemp(name)))
    dirs["net3a"] = nm.write_model_dir(nets, str(tmp_path_factory.mktemp("net3a")))
    return dirs


_consts = {}


def consts(lib, model_dir, stem, prec):
    key = (model_dir, stem, prec)
    if key not in _consts:
        _consts[key] = lr.Consts(lib, model_dir, stem, prec)
    return _consts[key]


def _key(res):
    return [[(d.anchor_index, d.as_row().tobytes()) for d in r] for r in res]


def _device_blobs(det, launches, frames):
    names = set()
    for L in launches:
        names.update(L.ins)
        names.update(b for b, _ in L.outs)
    blobs = {}
    for n in names:
        if n == "frame":
            blobs[n] = lr.frame_input(frames)
        elif n.startswith("face_rpn_"):
            blobs[n] = np.stack([det.get_output(n, i) for i in range(len(frames))]).astype(np.float64)
        else:
            blobs[n] = np.stack([det.debug_activation(n, i) for i in range(len(frames))]).astype(np.float64)
    return blobs


def _judge_engine(rfa, built_lib, model_dir, ws, stem, prec, hw, base_frame, only=None, network="net3", replay=None):
    """`network`: the preset the engines are created with (the model must carry its anchors); `replay`: compare the default engine's
    detections too (default: where every launch was judged)."""
    frames = lr.case_frames(base_frame, hw)
    k = consts(built_lib, model_dir, stem, prec)
    launches = [L for L in lr.launches(prec) if only is None or L.name in only]
    det = rfa.RetinaFace(model_dir, network, 0.4, precision=prec, net_hw=hw, model_stem=stem, keep_outputs=True, use_graph=False,
                         plan_cache=False, max_batch=8)
    try:
        eager = det.detectBatchImages(frames, 0.5)
        blobs = _device_blobs(det, launches, frames)
    finally:
        det.close()
    failures = []
    for L in launches:
        for v in lr.judge_launch(k, L, blobs):
            STATS.append(dict(weights=ws, model=stem, precision=PNAME[prec], size=f"{hw[0]}x{hw[1]}", launch=v.launch, blob=v.blob,
                              elements=v.n, share_exact=v.share_exact, median_width_ulps=v.median_width_ulps,
                              max_dev_over_gamma=v.max_dev_over_gamma, outside=v.n_fail))
            print(f"{ws} {stem} {PNAME[prec]} {hw[0]}x{hw[1]} {v.launch:11s} {v.blob:42s} n {v.n:8d}  lo==hi {v.share_exact:.3f}  "
                  f"median width {v.median_width_ulps:9.2f} ulp  max|v-zmid|/gamma {v.max_dev_over_gamma:.4f}  outside {v.n_fail}")
            if not v.ok:
                failures.append(v.message())
    assert not failures, "\n".join(failures[:8])
    if only is None if replay is None else replay:
        # the default engine (graph replay) must return the eager engine's detections byte for byte
        det = rfa.RetinaFace(model_dir, network, 0.4, precision=prec, net_hw=hw, model_stem=stem, plan_cache=False, max_batch=8)
        try:
            assert _key(det.detectBatchImages(frames, 0.5)) == _key(eager)
        finally:
            det.close()
    return blobs


SHIPPED = lr.SHIPPED_CASES


@pytest.mark.parametrize("prec", [FP32, FP16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("stem,hw", SHIPPED, ids=[f"{s}-{h}x{w}" for s, (h, w) in SHIPPED])
def test_every_launch_inside_its_interval_shipped_weights(rfa, built_lib, model_dirs, base_frame, stem, hw, prec):
    _judge_engine(rfa, built_lib, model_dirs["shipped"], "shipped", stem, prec, hw, base_frame)


def test_warp_specialised_aggregation_instance_on_the_other_model(rfa, built_lib, model_dirs, base_frame):
    """kernels.hip conv3_select: fp16 maps of >= 48 x 48 pixels with even sides run rf_c1_aggr on conv3x3_up_dma_kernel, which no small size
    reaches.  mnet25 covers it at 352 x 608; mnet-deconv-0517 runs that launch alone there."""
    _judge_engine(rfa, built_lib, model_dirs["shipped"], "shipped", "mnet-deconv-0517", FP16, BIG, base_frame, only=("aggr1",))


NET3A = [(stem, hw) for stem in STEMS for hw in SMALL]


@pytest.mark.parametrize("prec", [FP32, FP16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("stem,hw", NET3A, ids=[f"{s}-{h}x{w}" for s, (h, w) in NET3A])
def test_four_anchor_head_launches_inside_their_intervals(rfa, built_lib, model_dirs, base_frame, stem, hw, prec):
    """head_kernel<T, 4> (64 output channels, one wave per 16 of them, all 256 threads in the softmax; the fp16 hi + lo head weights over
    64 rows): head0, head1 and head2 of "net3a" engines on the widened shipped weights, three frames per call, every element inside its
    interval.  Every anchor number has a candidate at 0.5 and at 0.02 among the judged frames."""
    blobs = _judge_engine(rfa, built_lib, model_dirs["net3a"], "net3a", stem, prec, hw, base_frame, only=("head0", "head1", "head2"),
                          network="net3a", replay=True)
    probs = [blobs[lr.head_names(s)[0]] for s in lr.STRIDES]
    assert probs[0].shape[1] == 8
    for thr in (0.5, 0.02):
        assert nm.anchors_with_candidates(probs, thr) == {0, 1, 2, 3}, thr


DERIVED = lr.DERIVED_CASES


@pytest.mark.parametrize("prec", [FP32, FP16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("ws", ["degenerate", "ragged"])
@pytest.mark.parametrize("stem,hw", DERIVED, ids=[f"{s}-{h}x{w}" for s, (h, w) in DERIVED])
def test_every_launch_inside_its_interval_derived_weights(rfa, built_lib, model_dirs, base_frame, stem, hw, ws, prec):
    _judge_engine(rfa, built_lib, model_dirs[ws], ws, stem, prec, hw, base_frame)


@pytest.mark.parametrize("prec", [FP32, FP16], ids=["fp32", "fp16"])
def test_kernel_instances_of_the_bench_sizes_run_at_the_judged_sizes(rfa, prec):
    """The kernel instance names the engine reports (rf_profile) at 448 x 448 and 1280 x 896 are all launched at the judged sizes.  (The
    names carry the channel configuration and the aggregation conv's tile; the one instance chosen by map AREA, the fp16 warp-specialised
    rf_c1_aggr, does not show in the name and is covered by size: see the test above.)"""
    import torch

    def names(hw):
        det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=prec, net_hw=hw, model_stem="mnet25", plan_cache=False, max_batch=8)
        try:
            frames = torch.zeros((1,) + hw + (3,), dtype=torch.uint8, device="cuda")
            return {p["kernel"] for p in det.profile([frames[0].data_ptr()], iters=1)}
        finally:
            det.close()
    judged = set().union(*(names(hw) for hw in SMALL + (BIG,)))
    bench = names((448, 448)) | names((1280, 896))
    print(f"{PNAME[prec]} kernel instances at the judged sizes: {sorted(judged)}")
    assert bench <= judged, sorted(bench - judged)


def test_report_launch_interval_statistics():
    """Not an assertion on the device: writes the session's per-launch statistics where a run can collect them."""
    import json
    out = os.environ.get("RF_LAUNCH_INTERVALS_JSON")
    if out and STATS:
        with open(out, "w") as f:
            json.dump(STATS, f, indent=0)
    print(f"{len(STATS)} launch outputs judged, {sum(s['outside'] > 0 for s in STATS)} with elements outside")
