"""Overlays on the host (no GPU): rf_overlay_region and rf_overlay_host -- the code the kernels run, compiled for the host -- against
tests/overlay_ref.py byte for byte, the glyphs against pictures, the cases where the code can go wrong, the refusals, and the
stand-alone sanitizer program over overlay.h."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import overlay_ref as ov
from conftest import ROOT
from retinaface_amd import _lib
from test_redact_host import BIG, face_at, noise, seeded_faces, views

f32 = np.float32
NAN, INF = float("nan"), float("inf")


def full_face(x1, y1, x2, y2, score=0.9):
    """a face with the five points where a face has them"""
    r = face_at(x1, y1, x2, y2, score)
    w, h = x2 - x1, y2 - y1
    r[5:10] = [x1 + 0.3 * w, x1 + 0.7 * w, x1 + 0.5 * w, x1 + 0.35 * w, x1 + 0.65 * w]
    r[10:15] = [y1 + 0.35 * h, y1 + 0.35 * h, y1 + 0.55 * h, y1 + 0.75 * h, y1 + 0.75 * h]
    return r


def with_points(faces):
    return np.stack([full_face(*f[1:5], f[0]) for f in faces]) if len(faces) else np.zeros((0, 15), f32)


def check_host(frame, faces, scale=1.0, ids=None, **spec):
    """rf_overlay_host on a copy that keeps the view's layout against the reference: the whole frame (and the bytes around a view) and
    pixels"""
    import retinaface_amd as rfa
    base = frame.base if frame.base is not None else frame
    base_copy = np.array(base, copy=True)
    off = frame.ctypes.data - base.ctypes.data
    got = np.lib.stride_tricks.as_strided(base_copy.reshape(-1)[off:], frame.shape, frame.strides)
    assert got.ctypes.data - base_copy.ctypes.data == off and np.array_equal(got, frame)
    px, trunc = rfa.overlay_host(got, faces, scale, ids=ids, **spec)
    sp = ov.Spec(**spec)
    want, wpx, true = ov.overlay_image(sp, frame, faces, scale, ids)
    assert got.tobytes() == want.tobytes(), int((got != want).any(2).sum())
    k = min(len(faces), sp.max_regions)
    assert px[:k].tobytes() == wpx[:k].tobytes()
    assert trunc == (true > sp.max_regions)
    outside = np.ones(base.shape, bool)
    np.lib.stride_tricks.as_strided(outside.reshape(-1)[off:], frame.shape, frame.strides)[:] = False
    assert np.array_equal(base_copy[outside], np.asarray(base)[outside])      # nothing outside the view was written
    return got, px


def test_struct_size():
    assert C.sizeof(_lib.rf_overlay_spec) == 40


# ---------------------------------------------------------------------------------------------- 1. glyphs
PICTURES = {
    0: (".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."),
    1: ("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."),
    2: (".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####"),
    3: ("#####", "...#.", "..#..", "...#.", "....#", "#...#", ".###."),
    4: ("...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#."),
    5: ("#####", "#....", "####.", "....#", "....#", "#...#", ".###."),
    6: ("..##.", ".#...", "#....", "####.", "#...#", "#...#", ".###."),
    7: ("#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."),
    8: (".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."),
    9: (".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##.."),
}


@pytest.mark.parametrize("digit", range(10))
def test_each_glyph_at_font_scale_1_is_its_picture(built_lib, digit):
    """id = the digit (10 for 0: ids are labelled mod 1 000 000 without leading zeros, so 0 is drawn as the second digit of 10)"""
    import retinaface_amd as rfa
    frame = np.zeros((30, 30, 3), np.uint8)
    track_id = digit if digit else 10
    px, _ = rfa.overlay_host(frame, [face_at(5.0, 15.0, 20.0, 25.0)], ids=[track_id], label=ov.LABEL_ID, font_scale=1, radius=-1,
                             thickness=1, box=(1, 1, 1), text=(9, 9, 9))
    n = 2 if digit == 0 else 1
    left, top = 5, 15 - 9                                              # o = 0: the plate's left edge is x0, its rows end above y0
    plate = frame[top:top + 9, left:left + 1 + 6 * n, 0]
    assert (plate[0] == 1).all() and (plate[8] == 1).all() and (plate[:, 0] == 1).all() and (plate[:, 6] == 1).all()
    cell = plate[1:8, 1 + 6 * (n - 1):6 + 6 * (n - 1)]
    got = tuple("".join("#" if v == 9 else "." for v in row) for row in cell)
    assert got == PICTURES[digit], "\n".join(got)
    assert set(np.unique(cell)) <= {1, 9}
    assert tuple("".join("#" if (ov.GLYPHS[digit][gy] >> (4 - gx)) & 1 else "." for gx in range(5)) for gy in range(7)) == PICTURES[digit]


# ---------------------------------------------------------------------------------------------- 2. records
def test_region_records(built_lib):
    import retinaface_amd as rfa
    f = full_face(10.5, 12.25, 30.75, 33.0, 0.93)
    ok, r = rfa.overlay_region(f, 48, 64, label=ov.LABEL_SCORE)
    assert ok and list(r[:4]) == [10, 12, 30, 33] and r[8] == 2 and r[9] == 9 | (3 << 4)
    assert (r[10], r[11]) == (9, 11) and r[12] == 255 << 16 and r[13] == 31     # 12 - 1 - 18 < 0: the plate flips inside
    ok, r = rfa.overlay_region(f, 480, 640, coord_scale=BIG, track_id=1000007, label=ov.LABEL_ID, color_by_id=True, thickness=5)
    want = ov.Region(ov.Spec(label=ov.LABEL_ID, color_by_id=True, thickness=5), f, BIG, 1000007)
    assert ok and list(r[:4]) == [want.x0, want.y0, want.x1, want.y1] and r[8] == 1 and r[9] == 7
    assert r[12] == 255 | (128 << 8)                                           # palette[7] = (255, 128, 0)
    assert (r[10], r[11]) == (want.x0 - 2, want.y0 - 2 - 18)
    assert [(int(r[14 + k]), int(r[19 + k])) for k in range(5)] == want.centres
    for bad in ((NAN, 1, 5, 5), (1, 1, INF, 5), (9, 1, 5, 5), (1, -INF, 5, INF)):
        ok, r = rfa.overlay_region(face_at(*bad), 48, 64)
        assert not ok and not r.any()
    ok, r = rfa.overlay_region(face_at(-1e9, -1e9, 1e9, 1e9), 48, 64)
    assert ok and list(r[:4]) == [-4096, -4096, 8192, 8192]
    lib = rfa.load_library()
    sp = rfa.overlay_spec()
    face = _lib.rf_face.from_buffer_copy(f.tobytes())
    out = (C.c_int32 * 24)()
    assert lib.rf_overlay_region(C.byref(sp), None, 0, 1.0, 4, 4, out) == -1
    assert lib.rf_overlay_region(C.byref(sp), C.byref(face), 0, 1.0, -1, 4, out) == -1
    assert lib.rf_overlay_region(None, C.byref(face), 0, 1.0, 4, 4, out) == 1


# ---------------------------------------------------------------------------------------------- 3. whole frames
SPECS = (dict(), dict(label=ov.LABEL_SCORE, alpha=128), dict(label=ov.LABEL_ID, color_by_id=True, thickness=3, radius=4, font_scale=1),
         dict(thickness=16, radius=16, font_scale=8, label=ov.LABEL_ID), dict(thickness=1, radius=-1, alpha=1))


@pytest.mark.parametrize("spec", SPECS)
def test_host_shapes_and_seeded_faces_equal_the_reference(built_lib, spec):
    for name, frame in views().items():
        rng = np.random.default_rng(len(name))
        faces = with_points(seeded_faces(rng, frame.shape[0], frame.shape[1], 6))
        ids = [0, 7, 999999, 1000000, 12, 345]
        got, px = check_host(frame, faces, ids=ids, **spec)
        assert px.sum() > 0 and not np.array_equal(got, frame)
        check_host(frame, faces, scale=BIG, ids=ids, **spec)
    check_host(noise(0, 0), [face_at(1.0, 1.0, 5.0, 5.0)], **spec)


def border_boxes(rows, cols):
    r, c = float(rows), float(cols)
    return [(-50.0, -50.0, -20.0, -30.0), (c + 10, 5.0, c + 30, 9.0), (5.0, r + 100, 9.0, r + 120),          # wholly outside
            (-8.0, 10.0, 6.0, 20.0), (c - 5, 10.0, c + 9, 20.0), (10.0, -6.0, 20.0, 4.0), (10.0, r - 3, 20.0, r + 8),      # each border
            (-4.0, -4.0, 7.0, 6.0), (c - 6, -3.0, c + 5, 8.0), (-5.0, r - 7, 6.0, r + 4), (c - 7, r - 6, c + 3, r + 5),    # each corner
            (-20.0, -30.0, c + 40, r + 50), (0.0, 0.0, c - 1, r - 1), (-0.5, -0.5, c - 0.5, r - 0.5)]                      # around / on the frame


@pytest.mark.parametrize("spec", (dict(), dict(thickness=5, radius=6, label=ov.LABEL_SCORE, alpha=200)))
def test_boxes_outside_and_across_every_border_and_corner(built_lib, spec):
    frame = views()["48x64 padded"]
    for b in border_boxes(48, 64):
        check_host(frame, [full_face(*b)], **spec)
    got, px = check_host(frame, [full_face(*b) for b in border_boxes(48, 64)[:3]], radius=-1)
    assert not px.any() and np.array_equal(got, frame)


def test_lines_thick_outlines_non_finite_values_and_the_clamp(built_lib):
    frame = views()["48x64 padded"]
    for b in ((10.0, 10.0, 10.0, 30.0), (10.0, 20.0, 40.0, 20.0), (7.0, 7.0, 7.0, 7.0)):                    # w = 0, h = 0, a point
        for t in (1, 2, 3):
            got, px = check_host(frame, [face_at(*b)], thickness=t, radius=-1)
            assert px[0] == (int(b[2] - b[0]) + 1 + 2 * (t // 2)) * (int(b[3] - b[1]) + 1 + 2 * (t // 2))      # no inner rectangle: all of O
    # t larger than the box: the outline is all of O
    got, px = check_host(frame, [face_at(20.0, 20.0, 25.0, 24.0)], thickness=16, radius=-1)
    assert px[0] == (6 + 16) * (5 + 16)
    got, px = check_host(frame, [face_at(20.0, 20.0, 30.0, 23.0)], thickness=4, radius=-1)                  # empty along y only
    assert px[0] == (11 + 4) * (4 + 4)
    got, px = check_host(frame, [face_at(20.0, 20.0, 30.0, 24.0)], thickness=4, radius=-1)                  # an inner rectangle of 7 x 1
    assert px[0] == (11 + 4) * (5 + 4) - 7
    # NaN / inf in a box coordinate paints nothing, discs and label included; a reversed box likewise
    for bad in ((NAN, 1, 5, 5), (1, NAN, 5, 5), (1, 1, NAN, 5), (1, 1, 5, NAN), (-INF, 1, 5, 5), (1, 1, INF, 5), (1, -INF, 5, INF),
                (20, 5, 10, 9), (5, 20, 9, 10), (-3e38, 0, 3e38, 4)):                       # the last: a width that overflows
        f = full_face(10.0, 10.0, 30.0, 30.0)
        f[1:5] = bad
        got, px = check_host(frame, [f], label=ov.LABEL_SCORE)
        assert px[0] == 0 and np.array_equal(got, frame), bad
    # NaN or inf in one landmark skips that disc only
    for k in range(5):
        for axis, v in ((5, NAN), (10, INF), (5, -INF)):
            f = full_face(10.0, 8.0, 50.0, 40.0)
            f[axis + k] = v
            got, px = check_host(frame, [f], radius=3)
            whole, wpx = check_host(frame, [full_face(10.0, 8.0, 50.0, 40.0)], radius=3)
            assert wpx[0] - px[0] == 29                                                                    # a disc of radius 3
    # coordinates beyond the clamp: box and points
    f = full_face(-1e9, -5000.0, 1e9, 9000.0)
    f[5], f[10], f[6], f[11] = 1e9, 1e9, -1e9, 20.0
    check_host(frame, [f, full_face(-5000.0, 10.0, 30.0, 9000.0)])
    check_host(frame, [face_at(1.0, 1.0, 2.0, 2.0)], scale=3e38)


def test_labels_flip_at_the_top_and_are_cut_at_the_right(built_lib):
    frame = views()["48x64 padded"]
    spec = dict(label=ov.LABEL_ID, font_scale=2, radius=-1)
    for y1 in (17.0, 18.0, 19.0, 20.0, 0.0, -30.0):                                # PH = 18, o = 1: the plate flips when y0 - 1 - 18 < 0
        got, px = check_host(frame, [face_at(20.0, y1, 40.0, y1 + 20.0)], ids=[7], **spec)
    got, px = check_host(frame, [face_at(50.0, 30.0, 60.0, 44.0)], ids=[999999], **spec)      # PW = 74: cut at the right edge
    assert (got[29 - 18:29, 49:] != frame[29 - 18:29, 49:]).any(2).all()
    check_host(frame, [face_at(-30.0, 30.0, 10.0, 44.0)], ids=[123456], **spec)               # ... and at the left
    # ids 0, 7, 999 999 and 1 000 000 (which reads 0); negative ids and ids = None have no label
    for track_id, n in ((0, 0), (-3, 0), (7, 1), (999999, 6), (1000000, 1), (1000007, 1), (2 ** 40 + 123456, None)):
        import retinaface_amd as rfa
        ok, r = rfa.overlay_region(face_at(20.0, 30.0, 40.0, 44.0), 48, 64, track_id=track_id, label=ov.LABEL_ID)
        want = len(ov.Region(ov.Spec(label=ov.LABEL_ID), face_at(20.0, 30.0, 40.0, 44.0), 1.0, track_id).digits)
        assert r[8] == want and (n is None or n == want)
        check_host(views()["33x31 roi"], [face_at(5.0, 20.0, 20.0, 28.0)], ids=[track_id], label=ov.LABEL_ID, font_scale=1)
    check_host(frame, [face_at(20.0, 30.0, 40.0, 44.0)], ids=None, label=ov.LABEL_ID)
    # scores 0, 0.999, 1.0, NaN and the ones a clamp must catch
    for score, digits in ((0.0, 0), (0.999, 99), (1.0, 99), (NAN, 0), (0.5, 50), (-2.0, 0), (INF, 99), (-INF, 0), (0.07, 7), (1e30, 99)):
        import retinaface_amd as rfa
        ok, r = rfa.overlay_region(face_at(20.0, 30.0, 40.0, 44.0, score), 48, 64, label=ov.LABEL_SCORE)
        assert r[8] == 2 and (r[9] & 15) * 10 + (r[9] >> 4) == digits, score
        check_host(views()["33x31 roi"], [face_at(5.0, 20.0, 20.0, 28.0, score)], label=ov.LABEL_SCORE, font_scale=1)


@pytest.mark.parametrize("alpha", (1, 128, 255))
def test_overlapping_regions_lowest_index_wins_and_alpha_blends_the_original_once(built_lib, alpha):
    frame = views()["48x64 padded"]
    two = [full_face(10.0, 14.0, 40.0, 40.0, 0.9), full_face(25.0, 20.0, 55.0, 44.0, 0.8)]
    three = two + [full_face(5.0, 22.0, 60.0, 30.0, 0.7)]
    for faces, ids in ((two, [1, 2]), (three, [1, 2, 3]), (three[::-1], [3, 2, 1])):
        spec = dict(alpha=alpha, label=ov.LABEL_ID, color_by_id=True, thickness=3, radius=3)
        got, px = check_host(frame, faces, ids=ids, **spec)
        # every changed byte is one blend of the original: no pixel was painted twice
        sp = ov.Spec(**spec)
        colours = [sp.point, sp.text] + [ov.PALETTE[i & 7] for i in ids]
        changed = (got != frame).any(2)
        for y, x in zip(*np.nonzero(changed)):
            assert any(all((int(frame[y, x, c]) * (255 - alpha) + col[c] * alpha + 127) // 255 == got[y, x, c] for c in range(3))
                       for col in colours)
        alone, apx = check_host(frame, faces[:1], ids=ids[:1], **spec)
        assert px[0] == apx[0] and px[1] < check_host(frame, faces[1:2], ids=ids[1:2], **spec)[1][0]
        assert changed.sum() <= px.sum()


def test_max_regions_1_with_two_faces_is_truncated_with_the_first_face_drawn(built_lib):
    import retinaface_amd as rfa
    frame = views()["48x64 padded"]
    faces = [full_face(5.0, 5.0, 20.0, 20.0), full_face(30.0, 20.0, 50.0, 40.0)]
    got, px = check_host(frame, faces, max_regions=1)
    one, _ = check_host(frame, faces[:1])
    assert np.array_equal(got, one)
    work = np.array(frame, copy=True)
    assert rfa.overlay_host(work, faces, max_regions=1)[1] is True


def test_defaults_are_the_reference_look(built_lib):
    """cv::rectangle(.., Scalar(0,0,255), 2) and cv::circle(.., 1, Scalar(0,255,0), 2): a red two-pixel ring around the box, green dots"""
    import retinaface_amd as rfa
    frame = np.full((60, 80, 3), 77, np.uint8)
    px, _ = rfa.overlay_host(frame, [full_face(20.0, 15.0, 60.0, 45.0)])
    red = (frame == (0, 0, 255)).all(2)
    ring = np.zeros((60, 80), bool)
    ring[14:47, 19:62] = True
    ring[16:45, 21:60] = False
    green = (frame == (0, 255, 0)).all(2)
    assert np.array_equal(red, ring & ~green) and green.sum() == 5 * 13 and px[0] == ring.sum() + green.sum() - (ring & green).sum()
    assert ((frame == 77).all(2) | red | green).all()
    frame[:] = 77
    rfa.overlay_host(frame, [full_face(20.0, 15.0, 60.0, 45.0)], colors_set=True, radius=-1)      # an explicit black
    assert np.array_equal((frame == 0).all(2), ring)


def test_every_refusal_leaves_the_frame_unchanged(built_lib):
    import retinaface_amd as rfa
    frame = noise(20, 20)
    work = frame.copy()
    faces = [full_face(2.0, 2.0, 15.0, 15.0)]
    bad = [dict(thickness=17), dict(thickness=-1), dict(radius=17), dict(label=3), dict(label=-1), dict(font_scale=9), dict(font_scale=-1),
           dict(max_regions=1025), dict(max_regions=-1)]
    for kw in bad:
        with pytest.raises(rfa.RFError) as e:
            rfa.overlay_host(work, faces, **kw)
        assert e.value.status == -1, kw
        with pytest.raises(rfa.RFError):
            rfa.overlay_region(faces[0], 20, 20, **kw)
    lib = rfa.load_library()
    ptr, fp = C.c_void_p(work.ctypes.data), np.stack(faces).ctypes.data_as(C.POINTER(_lib.rf_face))
    for field, v in (("struct_size", 36), ("colors_set", 2), ("color_by_id", 2)):
        sp = rfa.overlay_spec()
        setattr(sp, field, v)
        assert lib.rf_overlay_host(C.byref(sp), ptr, 20, 20, 60, fp, None, 1, 1.0, None) == -1, field
    sp = rfa.overlay_spec()
    assert lib.rf_overlay_host(C.byref(sp), ptr, 20, 20, 59, fp, None, 1, 1.0, None) == -1          # step < cols * 3
    assert lib.rf_overlay_host(C.byref(sp), ptr, 20, 20, 60, None, None, 1, 1.0, None) == -1        # faces missing
    assert lib.rf_overlay_host(C.byref(sp), ptr, 20, 20, 60, fp, None, -1, 1.0, None) == -1
    assert lib.rf_overlay_host(C.byref(sp), ptr, -1, 20, 60, fp, None, 1, 1.0, None) == -1
    assert np.array_equal(work, frame)
    assert lib.rf_overlay_host(None, ptr, 20, 20, 60, fp, None, 1, 1.0, None) == 0 and not np.array_equal(work, frame)


# ---------------------------------------------------------------------------------------------- 4. overlay.h under the sanitizers
def test_overlay_h_under_address_and_undefined_sanitizers(tmp_path):
    """tests/csrc/test_overlay_host.cpp includes overlay.h alone, has its own main and runs as a program of its own: clipped regions on
    every side, an odd pointer with a padded step inside guard bytes, every spec extreme"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    clang = os.path.join(rocm, "llvm", "bin", "clang++")                   # the compiler the library is built with
    clang = clang if os.path.exists(clang) else shutil.which("clang++")
    assert clang, "no clang++ next to hipcc"
    exe = str(tmp_path / "test_overlay_host")
    subprocess.check_call([clang, "-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "test_overlay_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "overlay host ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
