"""Tiled, TTA, pyramid and rotation detection share one pass-call path in the engine: one per-lane pass table and gather event, one
inputs-ready event, one device block for host frames.  Here the modes follow each other on ONE handle whose calls really split into
launches over three lanes, with refused calls and the stand-alone merges in between, and every result must be the bytes the same
call returns on a fresh handle with the same options -- which test_tile_gpu.py, test_tta_gpu.py, test_pyramid_gpu.py and
test_rot_gpu.py pin to the numpy references."""
import numpy as np
import pytest

from conftest import ASSETS
from test_gpu_align import FP16, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_tta_gpu import SPLIT3, windows  # noqa: F401  (windows: fixture)

pytestmark = pytest.mark.gpu


def handle(rfa):
    det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", **SPLIT3)
    assert det.max_batch == 8 and det.num_slots() == 3
    return det


def frozen(x):
    """a result as something == compares byte for byte"""
    if isinstance(x, (list, tuple)):
        return tuple(frozen(v) for v in x)
    if hasattr(x, "as_row"):
        return np.asarray(x.as_row(), np.float32).tobytes()
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        return (x.shape, x.dtype.str, x.tobytes())
    return x


def test_modes_back_to_back_on_one_handle_equal_fresh_handles(rfa, windows, crop448):
    """Every call below carries more than 24 passes: launches of 8 over three lanes, so at least one lane is reused within the call
    (its pass table rewritten, its gather event recorded again) and the merge waits for the other lanes on the device."""
    seven = list(windows) + [crop448]
    dev = to_device(seven)
    ptrs = [d.data_ptr() for d in dev]

    def device_args(n):
        return [ptrs[i % 7] for i in range(n)], [448] * n, [448] * n

    per_frame = {"tiled": len(rfa.tile_plan(448, 448, 448, 448)), "tta": 2, "pyramid": len(rfa.pyramid_plan(448, 448, 448, 448)), "rot": 4}
    n_of = {mode: 24 // p + 1 for mode, p in per_frame.items()}
    n_of["rot"] = 7
    assert all(n_of[m] * per_frame[m] > 24 for m in per_frame), (n_of, per_frame)
    host13 = [seven[i % 7] for i in range(n_of["tta"])]

    def tiled(det):
        return det.detect_tiled_device(*device_args(n_of["tiled"]), 0.5, return_tiles=True), det.tiled_counts

    def tta(det):
        return det.detect_tta(host13, 0.5, return_votes=True), det.tta_counts

    def pyramid(det):
        return det.detect_pyramid_device(*device_args(n_of["pyramid"]), 0.5, return_votes=True), det.pyramid_counts

    def rot(det):
        return det.detect_rotated_device(*device_args(7), 0.5, return_votes=True), det.rot_counts, det.frame_rot, det.rot_score

    def fused(det):
        return det.detect_tiled_face_batch_device(*device_args(n_of["tiled"]), 0.5, crop_size=112, dtype="f16"), det.tiled_counts

    steps = (("tiled", tiled), ("tta", tta), ("pyramid", pyramid), ("rot", rot), ("tiled", fused))

    # the stand-alone merges: three frames, every pass of frame i brings the faces the plain call finds in frame i
    def passes(mode, faces):
        return [448] * 3, [448] * 3, [[faces[i]] * per_frame[mode] for i in range(3)]

    merges = (lambda det, f: (det.tile_merge(*passes("tiled", f), return_tiles=True), det.tiled_counts),
              lambda det, f: (det.tta_merge(*passes("tta", f), return_votes=True), det.tta_counts),
              lambda det, f: (det.pyramid_merge(*passes("pyramid", f), return_votes=True), det.pyramid_counts),
              lambda det, f: (det.rot_merge(*passes("rot", f), return_votes=True), det.rot_counts))

    refused = (lambda det: det.detect_tiled_device(*device_args(1), 0.5, max_faces=4097),
               lambda det: det.detect_tta([seven[0]], 0.5, max_faces=4097),
               lambda det: det.detect_pyramid_device(*device_args(1), 0.5, max_faces=4097),
               lambda det: det.detect_rotated_device(*device_args(1), 0.5, max_faces=4097))

    # the references: each call on a fresh handle of its own
    def fresh(call, *args):
        ref = handle(rfa)
        try:
            return call(ref, *args)
        finally:
            ref.close()

    faces = [rows_of(d) for d in fresh(lambda det: det.detect_device(ptrs, [448] * 7, [448] * 7, 0.5)) if d][:3]
    assert len(faces) == 3
    want = [frozen(fresh(call)) for _, call in steps]
    want_merges = [frozen(fresh(call, faces)) for call in merges]
    assert len(set(want)) == len(want) and len(set(want_merges)) == 4       # different results: a stale table or block would show

    det = handle(rfa)
    plain = det.detect_device(ptrs, [448] * 7, [448] * 7, 0.5)
    for k, (mode, call) in enumerate(steps):
        before = det.launch_stats()
        assert frozen(call(det)) == want[k], (k, mode)
        after = det.launch_stats()
        assert after["images"] - before["images"] == n_of[mode] * per_frame[mode] > 24 and after["launches"] - before["launches"] >= 4, (k, mode)
    for call in refused:
        with pytest.raises(rfa.RFError) as e:
            call(det)
        assert e.value.status == -1
    assert [frozen(call(det, faces)) for call in merges] == want_merges
    for k, (mode, call) in reversed(list(enumerate(steps))):
        assert frozen(call(det)) == want[k], (k, mode, "reverse")
    assert det.detect_device(ptrs, [448] * 7, [448] * 7, 0.5) == plain
    det.close()
