"""Face alignment, host side (no GPU): the numpy restatement tests/align_ref.py is pinned by digests of the crops it produces
for the golden detections, and rf_align_matrix -- the same transform code the kernel runs, compiled for the host -- must equal
it bit for bit."""
import ctypes as C
import glob
import hashlib
import os

import numpy as np
import pytest

import align_ref
from conftest import GOLDEN, golden
from retinaface_amd import _lib, align_matrix

PINS = {
    ("mnet25", 112): "adb1fa7cf338560d3f64826992d00dfc06b1a19e88f268040d3f6db9ae5c746a",
    ("mnet25", 128): "c87514a83c2c7f5e68d8167ec6c171b8b8eabfb94d7d0b2596fc5196ebb79949",
    ("mnet-deconv-0517", 112): "c98865375eeb6c021277c46f8970162b4d9f7acc511b1e23f6525abc374b7426",
    ("mnet-deconv-0517", 128): "148e5018d399f781beb547be582a0f8dfb14076f88280292d14b4ba570075d72",
}
PIN_SCALED = "6476cda8a0a28f12f2bf211bc88138af1662b88891f842d10d92871041e3273c"
PIN_MATRIX = ["0x1.8c26e42e73217p-1", "-0x1.141ea4e63938ep-3", "-0x1.44a21a216a917p+9",
              "0x1.141ea4e63938ep-3", "0x1.8c26e42e73217p-1", "-0x1.4dd2531bf6fdap+7"]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _native_matrix(lib, row, cs, size):
    f = _lib.rf_face.from_buffer_copy(np.asarray(row, np.float32).tobytes())
    m = (C.c_double * 6)(*([7.0] * 6))
    st = lib.rf_align_matrix(C.byref(f), C.c_float(cs), size, m)
    return st, np.array(m, np.float64)


def _golden_rows():
    rows = []
    for pat in ("fixture_*", "crop448_*", "synth448_*"):
        for path in sorted(glob.glob(os.path.join(GOLDEN, pat + ".npz"))):
            z = np.load(path)
            for k in z.files:
                if k.startswith("det") and not k.endswith("_idx") and z[k].ndim == 2 and z[k].shape[1] == 15:
                    rows.extend(z[k])
    return np.array(rows, np.float32)


@pytest.mark.parametrize("stem,size", sorted(PINS))
def test_align_ref_reproduces_the_pinned_crops(stem, size, base_frame):
    assert _sha(base_frame) == "2f8ae7b818ce7d11a98ca112e192e2e22cd3739deae601a286a4b271e007b61f"
    cr, _ = align_ref.crops(base_frame, golden(f"fixture_{stem}.npz")["det"], 1.0, size)
    assert cr.shape == (6, size, size, 3)
    assert _sha(cr) == PINS[(stem, size)]


def test_align_ref_reproduces_the_scaled_pin_and_the_matrix(base_frame):
    det = golden("fixture_mnet25.npz")["det"]
    small = det.copy()
    small[:, 5:] = (det[:, 5:] / np.float32(2.5)).astype(np.float32)
    cr, _ = align_ref.crops(base_frame, small, 2.5, 112)
    assert _sha(cr) == PIN_SCALED
    ok, fwd = align_ref.align_matrix(det[0], 1.0, 112)
    assert ok and [float(v).hex() for v in fwd] == PIN_MATRIX


def test_native_matrix_equals_align_ref_on_every_golden_detection(built_lib):
    rows = _golden_rows()
    assert len(rows) >= 40
    for size in (96, 112, 128):
        for cs in (1.0, 2.5, float(np.float32(1280) / np.float32(448))):
            for r in rows:
                st, got = _native_matrix(built_lib, r, cs, size)
                ok, want = align_ref.align_matrix(r, cs, size)
                assert st == 1 and ok
                assert np.array_equal(got, want), (size, cs, got, want)


def test_native_matrix_pin(built_lib):
    st, got = _native_matrix(built_lib, golden("fixture_mnet25.npz")["det"][0], 1.0, 112)
    assert st == 1 and [float(v).hex() for v in got] == PIN_MATRIX


def test_degenerate_faces_are_invalid(built_lib):
    same = np.zeros(15, np.float32)
    same[5:10], same[10:15] = 100.0, 50.0
    nan = golden("fixture_mnet25.npz")["det"][0].copy()
    nan[7] = np.nan
    inf = golden("fixture_mnet25.npz")["det"][0].copy()
    inf[12] = np.inf
    for row in (same, nan, inf):
        st, got = _native_matrix(built_lib, row, 1.0, 112)
        assert st == 0 and np.array_equal(got, np.zeros(6))
        ok, want = align_ref.align_matrix(row, 1.0, 112)
        assert not ok and np.array_equal(want, np.zeros(6))
        cr, _ = align_ref.crop(np.full((64, 64, 3), 200, np.uint8), row, 1.0, 112)
        assert not cr.any()


def test_bad_arguments_are_refused(built_lib):
    row = golden("fixture_mnet25.npz")["det"][0]
    for size in (8, 15, 513, 1000, -112):
        st, _ = _native_matrix(built_lib, row, 1.0, size)
        assert st == _lib.RF_ERR_INVALID_ARG, size
    for size in (16, 512):
        assert _native_matrix(built_lib, row, 1.0, size)[0] == 1
    m = (C.c_double * 6)()
    f = _lib.rf_face()
    assert built_lib.rf_align_matrix(None, 1.0, 112, m) == _lib.RF_ERR_INVALID_ARG
    assert built_lib.rf_align_matrix(C.byref(f), 1.0, 112, None) == _lib.RF_ERR_INVALID_ARG
    with pytest.raises(_lib.RFError):
        align_matrix(row, 1.0, 8)


def test_known_similarity_is_recovered(built_lib):
    """The template pushed through the inverse of a known similarity M: the definition's arithmetic (align_ref, float64 points)
    recovers M to 1e-9; rf_align_matrix sees the same points rounded to float32 (rf_face holds floats), equals align_ref on
    them bit for bit and is M up to that rounding (2^-24 relative on coordinates of up to ~1500 pixels, times the scale)."""
    tx, ty = np.array(align_ref.TEMPLATE_X), np.array(align_ref.TEMPLATE_Y)
    for size, ang, sc, ox, oy in ((112, 0.3, 0.8, -310.0, -200.0), (128, -1.1, 2.2, 40.0, -700.0), (96, 3.0, 0.25, 250.0, 30.0)):
        k = size / 112.0
        a, b = sc * np.cos(ang), sc * np.sin(ang)
        known = np.array([a, -b, ox, b, a, oy])
        qx, qy = tx * k - ox, ty * k - oy            # q = [a -b; b a] p + t  =>  p = R^-1 (q - t)
        d = a * a + b * b
        px, py = (a * qx + b * qy) / d, (-b * qx + a * qy) / d
        ok, fwd, _ = align_ref.estimate_points(px, py, size)
        assert ok and np.abs(fwd - known).max() <= 1e-9, (fwd, known)
        row = np.zeros(15, np.float32)
        row[5:10], row[10:15] = px, py
        st, got = _native_matrix(built_lib, row, 1.0, size)
        assert st == 1 and np.array_equal(got, align_ref.align_matrix(row, 1.0, size)[1])
        assert np.abs(got - known).max() <= 1e-3 * max(1.0, sc), (got, known)


def test_template_landmarks_give_the_top_left_block(built_lib):
    rng = np.random.default_rng(7)
    frame = rng.integers(0, 256, size=(300, 400, 3), dtype=np.uint8)
    for size in (112, 224):                      # S / 112 integral or not: the template times k is exact only in float64
        k = np.float64(size) / 112.0
        row = np.zeros(15, np.float32)
        row[5:10] = np.array(align_ref.TEMPLATE_X) * k
        row[10:15] = np.array(align_ref.TEMPLATE_Y) * k
        cr, fwd = align_ref.crop(frame, row, 1.0, size)
        st, got = _native_matrix(built_lib, row, 1.0, size)
        assert st == 1 and np.array_equal(got, fwd)
        assert np.allclose(fwd, [1, 0, 0, 0, 1, 0], atol=1e-4)
        assert np.array_equal(cr, frame[:size, :size])


def test_python_align_matrix_wrapper(built_lib):
    from retinaface_amd import Detection
    r = golden("fixture_mnet25.npz")["det"][1]
    ok, m = align_matrix(r, 2.5, 96)
    want = align_ref.align_matrix(r, 2.5, 96)[1].reshape(2, 3)
    assert ok and m.shape == (2, 3) and np.array_equal(m, want)
    d = Detection(float(r[0]), tuple(r[1:5]), tuple(r[5:10]), tuple(r[10:15]), -1)
    assert np.array_equal(align_matrix(d, 2.5, 96)[1], want)
