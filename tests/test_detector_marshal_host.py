"""The marshalling helpers of retinaface_amd/detector.py, on their own (no library, no GPU): the one host-frame rule and who keeps a
copy alive, the one device-frame block, and the pass block whose counts carry the truncation signal."""
import ctypes as C

import numpy as np
import pytest

from retinaface_amd import detector as D


def frame(rows=6, cols=5, channels=3):
    return np.arange(rows * cols * channels, dtype=np.uint8).reshape(rows, cols, channels)


def as_array(ptr, rows, cols, step):
    """the (rows, cols, 3) pixels a C callee would read through (ptr, rows, cols, step)"""
    flat = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=((rows - 1) * step + cols * 3,))
    return np.lib.stride_tricks.as_strided(flat, (rows, cols, 3), (step, 3, 1))


@pytest.mark.parametrize("view", [frame()[:, ::-1], frame(channels=4)[:, :, :3], frame()[:, ::2]], ids=["mirrored", "bgra", "every_other"])
def test_pixels_that_are_not_dense_are_copied_and_the_copy_is_kept(view):
    assert view.strides[1] != 3
    (ptrs, rows, cols, steps, n), keep = D._host_frames([view])
    assert n == 1 and len(keep) == 1 and keep[0] is not view and keep[0].flags.c_contiguous
    assert ptrs[0] == keep[0].ctypes.data and (rows[0], cols[0], steps[0]) == (view.shape[0], view.shape[1], 3 * view.shape[1])
    assert np.array_equal(keep[0], view) and np.array_equal(as_array(ptrs[0], rows[0], cols[0], steps[0]), view)


def test_a_row_pitched_view_with_dense_pixels_is_taken_as_it_is():
    wide = frame(6, 9)
    view = wide[1:5, 2:7]
    assert view.strides == (27, 3, 1) and not view.flags.c_contiguous
    (ptrs, rows, cols, steps, n), keep = D._host_frames([frame(), view])
    assert n == 2 and keep[1] is view and ptrs[1] == view.ctypes.data
    assert (rows[1], cols[1], steps[1]) == (4, 5, 27) and steps[0] == 15
    assert np.array_equal(as_array(ptrs[1], rows[1], cols[1], steps[1]), view)


def test_none_and_empty_frames_are_null_frames():
    (ptrs, rows, cols, steps, n), keep = D._host_frames([None, np.zeros((0, 0, 3), np.uint8), frame(), np.zeros((0, 4, 3), np.float32)])
    assert n == 4 and len(keep) == 1
    for i in (0, 1, 3):                                   # (an empty frame is not looked at: its dtype does not matter)
        assert (ptrs[i], rows[i], cols[i], steps[i]) == (None, 0, 0, 0)
    assert ptrs[2] == keep[0].ctypes.data


def test_an_empty_batch_still_gives_arrays_to_pass():
    (ptrs, rows, cols, steps, n), keep = D._host_frames([])
    assert n == 0 and keep == [] and len(ptrs) == len(rows) == len(cols) == len(steps) == 1
    assert D._host_frames([], in_place="redacted").args[4] == 0
    p, r, c, s = D._device_frames([], [], [])
    assert len(p) == len(r) == len(c) == len(s) == 1


@pytest.mark.parametrize("bad", [frame().astype(np.float32), frame(channels=4), frame()[:, :, 0], frame()[:, :, :2]],
                         ids=["float32", "four_channels", "two_dims", "two_channels"])
def test_wrong_dtype_or_channels_is_refused(bad):
    with pytest.raises(ValueError, match=r"^frames must be uint8 H x W x 3 \(CV_8UC3, BGR\)$"):
        D._host_frames([frame(), bad])
    with pytest.raises(ValueError, match=r"^frames must be uint8 H x W x 3 with dense pixels \(CV_8UC3, BGR\)$"):
        D._host_frames([frame(), bad], in_place="redacted")


def test_in_place_nothing_is_copied_so_loose_pixels_and_read_only_frames_are_refused():
    dense = r"^frames must be uint8 H x W x 3 with dense pixels \(CV_8UC3, BGR\)$"
    for view in (frame()[:, ::-1], frame(channels=4)[:, :, :3]):
        with pytest.raises(ValueError, match=dense):
            D._host_frames([view], in_place="redacted")
    frozen = frame()
    frozen.flags.writeable = False
    with pytest.raises(ValueError, match="^frames are redacted in place: they must be writeable$"):
        D._host_frames([frozen], in_place="redacted")
    with pytest.raises(ValueError, match="^frames are drawn into in place: they must be writeable$"):
        D._host_frames([frozen], in_place="drawn into")
    assert D._host_frames([frozen]).keep[0] is frozen     # a call that only reads takes it
    # a row-pitched view is written through as it is
    view = frame(6, 9)[1:5, 2:7]
    (ptrs, rows, cols, steps, n), keep = D._host_frames([view, None], in_place="drawn into")
    assert ptrs[0] == view.ctypes.data and steps[0] == 27 and ptrs[1] is None and keep[0] is view


def test_device_frames_default_to_dense_rows_and_take_null_pointers():
    p, r, c, s = D._device_frames([4096, 0, None], [7, 0, 0], [5, 0, 9])
    assert list(p) == [4096, None, None] and list(r) == [7, 0, 0] and list(c) == [5, 0, 9] and list(s) == [15, 0, 27]
    p, r, c, s = D._device_frames([4096, 8192], [7, 7], [5, 5], steps=[16, 64])
    assert list(s) == [16, 64] and isinstance(p, C.Array) and p._type_ is C.c_void_p and s._type_ is C.c_int


def test_pack_passes_cuts_the_block_but_not_the_count():
    md = 3
    faces = np.arange(5 * 15, dtype=np.float32).reshape(5, 15)
    det = D.Detection(0.5, (1, 2, 3, 4), (5,) * 5, (6,) * 5, 7)
    flat, counts = D._pack_passes([faces, faces[:2], [], [det]], md)
    assert flat.shape == (4, md, 15) and flat.dtype == np.float32 and flat.flags.c_contiguous
    assert list(counts[:4]) == [5, 2, 0, 1]               # 5 > md: the C side reports the truncation from this
    assert np.array_equal(flat[0], faces[:md]) and np.array_equal(flat[1, :2], faces[:2]) and not flat[1, 2:].any() and not flat[2].any()
    assert np.array_equal(flat[3, 0], det.as_row())
    flat, counts = D._pack_passes([], md)
    assert flat.shape == (1, md, 15) and len(counts) >= 1 and counts[0] == 0


def test_one_row_makes_one_detection():
    row = np.array([0.75, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14], np.float32) / np.float32(3)
    d = D._detection(row)
    assert d.anchor_index == -1 and D._detection(row, 9).anchor_index == 9
    assert all(type(v) is float for v in (d.score,) + d.rect + d.xs + d.ys)
    assert d.as_row().tobytes() == row.tobytes() and len(d.rect) == 4 and len(d.xs) == len(d.ys) == 5
