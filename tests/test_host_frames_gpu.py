"""Every entry point that takes host frames marshals them one way: a frame whose pixels are not dense is copied, and the copy has to
live until the C call has returned -- the upload reads it.  Here each of those calls gets a batch of a mirrored view (the copy path)
and an empty frame, and must return what it returns for the same pixels handed over dense: the detections and every extra output.
The two calls that write into the caller's frames cannot take a copy and must refuse the view instead."""
import numpy as np
import pytest

import schedule_ref as sr
from conftest import ASSETS
from test_gpu_align import FP16, rfa  # noqa: F401  (rfa: fixture)
from test_pass_calls_gpu import frozen

pytestmark = pytest.mark.gpu

THR = 0.02                             # low enough that the small net finds faces in the cut-out


@pytest.fixture(scope="module")
def det(rfa):
    d = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=sr.NET_HW, model_stem="mnet25")
    yield d
    d.close()


@pytest.fixture(scope="module")
def batches(base_frame):
    """(the batch with the mirrored view, the same batch with that frame dense)"""
    view = sr.edge_frame(base_frame, sr.NET_HW)[:, ::-1]
    assert view.strides[1] == -3 and not view.flags.c_contiguous
    return [view, None], [np.ascontiguousarray(view), None]


def identity_mesh(det):
    """one view that is the frame itself: node (i, j) looks at source pixel (16 i, 16 j), in 1/256 px"""
    ny, nx = det.net_h // 16 + 1, det.net_w // 16 + 1
    mesh = np.zeros((1, ny, nx, 2), np.int32)
    mesh[0, :, :, 0] = np.arange(nx)[None, :] * 16 * 256
    mesh[0, :, :, 1] = np.arange(ny)[:, None] * 16 * 256
    return mesh


def calls(det):
    """name -> call(imgs): the result and every attribute the call leaves behind"""
    dw = det.dewarper(sr.NET_HW[0], sr.NET_HW[1], mesh=identity_mesh(det))

    def tracked(imgs):
        trk = det.tracker(1)
        res = det.detect_tracked(imgs, trk, [0, -1], THR)
        out = res, det.last_out, det.last_counts, trk.truncated
        trk.close()
        return out

    def shots(imgs):
        trk = det.tracker(1).enable_shots(crop_size=32, dtype="u8")
        res = det.detect_track_shots(imgs, trk, [0, -1], THR, return_quality=True)
        out = res, det.last_out, det.last_counts, trk.truncated
        trk.close()
        return out

    return {
        "detectBatchImages": lambda imgs: det.detectBatchImages(imgs, THR),
        "detect_pad32": lambda imgs: det.detect_pad32(imgs, THR),
        "detect_aligned": lambda imgs: det.detect_aligned(imgs, THR, crop_size=32),
        "detect_face_batch": lambda imgs: (det.detect_face_batch(imgs, THR, crop_size=32, dtype="u8", return_quality=True), det.faces_truncated),
        "detect_tiled": lambda imgs: (det.detect_tiled(imgs, THR, return_tiles=True), det.tiled_counts),
        "detect_tracked": tracked,
        "detect_track_shots": shots,
        "detect_tta": lambda imgs: (det.detect_tta(imgs, THR, return_votes=True), det.tta_counts),
        "detect_rotated": lambda imgs: (det.detect_rotated(imgs, THR, return_votes=True), det.rot_counts, det.frame_rot, det.rot_score),
        "detect_dewarped": lambda imgs: (det.detect_dewarped(imgs, dw, THR, return_votes=True), det.dewarp_counts),
        "detect_enhanced": lambda imgs: (det.detect_enhanced(imgs, THR), det.tiles_enhanced),
        "detect_pyramid": lambda imgs: (det.detect_pyramid(imgs, THR, return_votes=True), det.pyramid_counts),
    }


def test_a_copied_view_gives_what_the_dense_frame_gives(det, batches):
    viewed, dense = batches
    before = viewed[0].copy()
    plain = det.detectBatchImages(dense, THR)
    assert len(plain) == 2 and len(plain[0]) > 0 and plain[1] == []
    for name, call in calls(det).items():
        got = frozen((call(viewed), det.truncated))
        want = frozen((call(dense), det.truncated))
        assert got == want, name
    assert np.array_equal(viewed[0], before)


def test_the_in_place_calls_refuse_what_they_would_have_to_copy(det, batches):
    viewed, dense = batches
    for call in (det.detect_redacted, det.detect_overlay):
        with pytest.raises(ValueError, match="frames must be uint8 H x W x 3 with dense pixels"):
            call(viewed, THR)
    frozen_frame = dense[0].copy()
    frozen_frame.flags.writeable = False
    with pytest.raises(ValueError, match="frames are redacted in place: they must be writeable"):
        det.detect_redacted([frozen_frame, None], THR)
    with pytest.raises(ValueError, match="frames are drawn into in place: they must be writeable"):
        det.detect_overlay([frozen_frame, None], THR)
    # dense and writeable, they are taken: same detections as the plain call on the untouched pixels
    plain = det.detectBatchImages(dense, THR)
    for call in (det.detect_redacted, det.detect_overlay):
        assert frozen(call([dense[0].copy(), None], THR)) == frozen(plain)
