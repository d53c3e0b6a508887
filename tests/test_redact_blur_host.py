"""Blur redaction on the host (no GPU): rf_redact_host with rf_redact_spec.blur -- the code the blur kernel's pieces come from, compiled
for the host -- against tests/redact_blur_ref.py byte for byte (the whole frame, the bytes around a view, pixels), one property per
test, the refusals, and the stand-alone C++ program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import redact_blur_ref as rb
import redact_ref as rr
from conftest import ROOT
from retinaface_amd import _lib
from test_redact_host import BIG, face_at, noise, seeded_faces, views

f32 = np.float32


def check_host(frame, faces, scale=1.0, **spec):
    """rf_redact_host on a copy that keeps the view's layout against the blur reference: the whole frame, the bytes around a view, pixels"""
    import retinaface_amd as rfa
    base = frame.base if frame.base is not None else frame
    base_copy = np.array(base, copy=True)
    off = frame.ctypes.data - base.ctypes.data
    got = np.lib.stride_tricks.as_strided(base_copy.reshape(-1)[off:], frame.shape, frame.strides)
    assert got.ctypes.data - base_copy.ctypes.data == off and np.array_equal(got, frame)
    px, trunc = rfa.redact_host(got, faces, scale, **spec)
    sp = rb.Spec(**spec)
    want, wpx, true = rb.redact_image(sp, frame, faces, scale)
    assert got.tobytes() == want.tobytes(), int((got != want).sum())
    k = min(len(faces), sp.max_regions)
    assert px[:k].tobytes() == wpx[:k].tobytes()
    assert trunc == (true > sp.max_regions)
    outside = np.ones(base.shape, bool)
    np.lib.stride_tricks.as_strided(outside.reshape(-1)[off:], frame.shape, frame.strides)[:] = False
    assert np.array_equal(base_copy[outside], np.asarray(base)[outside])      # nothing outside the view was written
    return got, px


@pytest.mark.parametrize("shape", (rr.RECT, rr.ELLIPSE))
@pytest.mark.parametrize("cells", (1, 2, 8, 64))
@pytest.mark.parametrize("blur", (1, 2, 3))
def test_frames_equal_the_reference(built_lib, blur, cells, shape):
    """48 x 64 with a padded step, 1 x 1 (a blur of one pixel), a 33 x 31 ROI view at an odd pointer; cells = 1 on 48 x 64 makes the
    radius larger than the frame: every tap is clamped"""
    for name, frame in views().items():
        rows, cols = frame.shape[:2]
        rng = np.random.default_rng(blur * 16 + cells * 2 + shape)
        for k in (0, 1, 5):
            check_host(frame, seeded_faces(rng, rows, cols, k), blur=blur, shape=shape, cells=cells)
        got, px = check_host(frame, face_at(-3.0, -2.0, cols / 2.0, rows / 2.0)[None], BIG, blur=blur, shape=shape, cells=cells)
        assert px[0] > 0
    sp = rb.Spec(cells=1)
    assert rb.radius(rr.region(sp, (-3.0, -2.0, 32.0, 24.0), BIG, 48, 64)) == 64 > 48


def test_blur_changes_noise_and_differs_from_pixelation(built_lib):
    frame = views()["48x64 padded"]
    face = face_at(10.0, 8.0, 40.0, 38.0)[None]
    blurred, px = check_host(frame, face, blur=3)
    import retinaface_amd as rfa
    pixelated = np.ascontiguousarray(frame).copy()
    rfa.redact_host(pixelated, face)
    assert px[0] > 0 and not np.array_equal(blurred, frame) and not np.array_equal(blurred, pixelated)


def test_a_constant_frame_is_unchanged_and_its_pixels_are_owned(built_lib):
    import retinaface_amd as rfa
    flat = np.full((48, 64, 3), (255, 1, 128), np.uint8)
    faces = seeded_faces(np.random.default_rng(2), 48, 64, 5)
    for blur in (1, 2, 3):
        for cells in (1, 3, 8):
            got = flat.copy()
            px, _ = rfa.redact_host(got, faces, cells=cells, blur=blur)
            assert np.array_equal(got, flat) and px.sum() > 0


def test_one_pass_equals_a_brute_force_double_loop(built_lib):
    """blur = 1 written out: for every pixel of the region, the rounded mean over x of the original row, then over y of those"""
    frame = np.ascontiguousarray(views()["48x64 padded"])
    rows, cols = frame.shape[:2]
    face = face_at(-4.0, 30.0, 20.0, 52.0)[None]                      # crosses the left and the bottom side
    got, _ = check_host(frame, face, blur=1, cells=4, margin=-1.0)
    r = rr.region(rr.Spec(cells=4, margin=-1.0), face[0, 1:5], 1.0, rows, cols)
    rho = min(r.c, 64)
    n = 2 * rho + 1
    assert rho == 7 and r.cx0 == 0 and r.cy1 == rows          # W = 25, H = 23: c = 7
    for y in range(r.cy0, r.cy1):
        for x in range(r.cx0, r.cx1):
            for ch in range(3):
                col = []
                for dy in range(-rho, rho + 1):
                    yy = min(max(y + dy, 0), rows - 1)
                    s = sum(int(frame[yy, min(max(x + dx, 0), cols - 1), ch]) for dx in range(-rho, rho + 1))
                    col.append((s + rho) // n)
                assert got[y, x, ch] == (sum(col) + rho) // n, (x, y, ch)


@pytest.mark.parametrize("blur", (1, 3))
def test_a_region_across_each_frame_side(built_lib, blur):
    frame = views()["48x64 padded"]
    for box in ((-8.0, 10.0, 6.0, 20.0), (59.0, 10.0, 73.0, 20.0), (10.0, -6.0, 20.0, 4.0), (10.0, 45.0, 20.0, 56.0), (-5.0, -5.0, 70.0, 52.0)):
        for cells in (2, 8):
            got, px = check_host(frame, face_at(*box)[None], blur=blur, cells=cells)
            assert px[0] > 0 and not np.array_equal(got, frame)


def test_overlapping_regions_the_lower_index_radius_wins(built_lib):
    """a large region (rho 20) and a small one (rho 4) that overlap, in both orders: inside the overlap the value is the lower index's
    blur, and the counts add up to the union"""
    frame = noise(90, 120, 6)
    big, small = face_at(10.0, 5.0, 89.0, 84.0), face_at(70.0, 40.0, 84.0, 54.0)
    sp = rb.Spec(blur=2, margin=-1.0, cells=4)
    regs = [rr.region(sp, f[1:5], 1.0, 90, 120) for f in (big, small)]
    assert [rb.radius(r) for r in regs] == [20, 4]
    masks = []
    for r in regs:
        m = np.zeros((90, 120), bool)
        m[r.cy0:r.cy1, r.cx0:r.cx1] = True
        masks.append(m)
    both = masks[0] & masks[1]
    assert both.any()
    for order in ((big, small), (small, big)):
        got, px = check_host(frame, np.stack(order), blur=2, margin=-1.0, cells=4)
        first = regs[0] if order[0] is big else regs[1]
        assert np.array_equal(got[both], rb.blurred(frame, rb.radius(first), 2)[both])
        assert px.sum() == (masks[0] | masks[1]).sum()
    a, _ = check_host(frame, np.stack((big, small)), blur=2, margin=-1.0, cells=4)
    b, _ = check_host(frame, np.stack((small, big)), blur=2, margin=-1.0, cells=4)
    assert not np.array_equal(a[both], b[both])


def test_a_large_region_reaches_the_radius_cap(built_lib):
    """600 x 600 in a 700 x 700 frame at cells = 8: c = 75, rho = 64"""
    frame = noise(700, 700, 7)
    face = face_at(50.0, 50.0, 649.0, 649.0)[None]
    r = rr.region(rr.Spec(margin=-1.0), face[0, 1:5], 1.0, 700, 700)
    assert r.c == 75 and rb.radius(r) == 64
    got, px = check_host(frame, face, blur=3, margin=-1.0)
    assert px[0] == 600 * 600 and np.array_equal(got[50:650, 50:650], rb.blurred(frame, 64, 3)[50:650, 50:650])


def test_max_regions_cuts_the_list(built_lib):
    frame = views()["48x64 padded"]
    faces = seeded_faces(np.random.default_rng(8), 48, 64, 6)
    import retinaface_amd as rfa
    got = np.ascontiguousarray(frame).copy()
    _, trunc = rfa.redact_host(got, faces, max_regions=4, blur=2)
    assert trunc
    check_host(frame, faces, max_regions=4, blur=2)
    check_host(frame, faces, max_regions=6, blur=2)
    f = (_lib.rf_face * 6).from_buffer_copy(np.ascontiguousarray(faces).tobytes())
    sp = rfa.redact_spec(max_regions=4, blur=2)
    buf = np.ascontiguousarray(frame).copy()
    assert built_lib.rf_redact_host(C.byref(sp), buf.ctypes.data, 48, 64, 192, f, 6, 1.0, None) == _lib.RF_ERR_TRUNCATED


def test_refusals(built_lib):
    import retinaface_amd as rfa
    lib = built_lib
    frame = noise(8, 8, 1)
    f = _lib.rf_face.from_buffer_copy(face_at(1.0, 1.0, 5.0, 5.0).tobytes())
    out = (C.c_int * 9)()
    for kw in (dict(blur=4), dict(blur=255), dict(blur=1, mode=rr.FILL), dict(blur=3, mode=rr.FILL, fill=(1, 2, 3)), dict(blur=1, mode=2)):
        sp = rfa.redact_spec(**kw)
        assert lib.rf_redact_region(C.byref(sp), C.byref(f), 1.0, 8, 8, out) == _lib.RF_ERR_INVALID_ARG, kw
        before = frame.copy()
        assert lib.rf_redact_host(C.byref(sp), frame.ctypes.data, 8, 8, 24, C.byref(f), 1, 1.0, None) == _lib.RF_ERR_INVALID_ARG, kw
        assert np.array_equal(frame, before)
    for blur in (1, 2, 3):
        sp = rfa.redact_spec(blur=blur)
        assert lib.rf_redact_region(C.byref(sp), C.byref(f), 1.0, 8, 8, out) == 1
    assert C.sizeof(_lib.rf_redact_spec) == 32 and _lib.rf_redact_spec.blur.offset == 23


def test_blur_zero_set_explicitly_gives_the_bytes_of_pixelation(built_lib):
    import retinaface_amd as rfa
    for name, frame in views().items():
        rows, cols = frame.shape[:2]
        faces = seeded_faces(np.random.default_rng(3), rows, cols, 4)
        for mode in (rr.PIXELATE, rr.FILL):
            got = np.ascontiguousarray(frame).copy()
            px, _ = rfa.redact_host(got, faces, mode=mode, blur=0, cells=3, fill=(4, 5, 6))
            want, wpx, _ = rr.redact_image(rr.Spec(mode=mode, cells=3, fill=(4, 5, 6)), np.ascontiguousarray(frame), faces)
            assert got.tobytes() == want.tobytes() and px[:4].tobytes() == wpx[:4].tobytes()


def test_host_program_under_sanitizers(tmp_path):
    """tests/csrc/test_redact_blur_host.cpp: redact.h compiled into a stand-alone program with the address and undefined-behaviour
    sanitizers -- regions at all four borders and a radius larger than the frame against a naive loop; the halo's index clamp is
    where an out-of-bounds read would be"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    clang = os.path.join(rocm, "llvm", "bin", "clang++")                   # the compiler the library is built with
    clang = clang if os.path.exists(clang) else shutil.which("clang++")
    assert clang, "no clang++ next to hipcc"
    exe = str(tmp_path / "test_redact_blur_host")
    subprocess.check_call([clang, "-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "test_redact_blur_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
