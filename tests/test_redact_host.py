"""Face redaction on the host (no GPU): rf_redact_region and rf_redact_host -- the code the kernels run, compiled for the host -- against
tests/redact_ref.py byte for byte, then the properties the definition promises and a constructed face."""
import ctypes as C

import numpy as np
import pytest

import redact_ref as rr
from retinaface_amd import _lib

f32 = np.float32
BIG = float(f32(1280) / f32(448))


def face_at(x1, y1, x2, y2, score=0.9):
    r = np.zeros(15, f32)
    r[0], r[1], r[2], r[3], r[4] = score, x1, y1, x2, y2
    return r


def native_region(lib, box, scale, rows, cols, **spec):
    import retinaface_amd as rfa
    sp = rfa.redact_spec(**spec)
    f = _lib.rf_face.from_buffer_copy(face_at(*box).tobytes())
    out = (C.c_int * 9)()
    st = lib.rf_redact_region(C.byref(sp), C.byref(f), float(scale), rows, cols, out)
    return st, np.array(out, np.int32)


def noise(rows, cols, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)


def views(seed=1):
    """the frames of the host cases: 48 x 64 with a padded step, 1 x 1, a 33 x 31 ROI view at an odd pointer"""
    padded = np.zeros((48, 70, 3), np.uint8)
    padded[:] = noise(48, 70, seed)
    parent = noise(40, 50, seed + 1)
    roi = parent[3:36, 5:36]
    assert roi.ctypes.data % 2 == 1                                          # 3 * 150 + 15 = 465 bytes into an aligned block
    return {"48x64 padded": padded[:, :64], "1x1": noise(1, 1, seed + 2), "33x31 roi": roi}


def seeded_faces(rng, rows, cols, k):
    out = []
    for _ in range(k):
        w, h = rng.uniform(0.5, max(cols * 0.8, 1.0)), rng.uniform(0.5, max(rows * 0.8, 1.0))
        x, y = rng.uniform(-w / 2, cols - w / 2), rng.uniform(-h / 2, rows - h / 2)
        out.append(face_at(x, y, x + w, y + h, rng.uniform(0.5, 1)))
    return np.stack(out) if out else np.zeros((0, 15), f32)


def check_host(frame, faces, scale=1.0, **spec):
    """rf_redact_host on a copy that keeps the view's layout against the reference: the whole frame (and the bytes around a view) and
    pixels"""
    import retinaface_amd as rfa
    base = frame.base if frame.base is not None else frame
    base_copy = np.array(base, copy=True)
    off = frame.ctypes.data - base.ctypes.data
    got = np.lib.stride_tricks.as_strided(base_copy.reshape(-1)[off:], frame.shape, frame.strides)
    assert got.ctypes.data - base_copy.ctypes.data == off and np.array_equal(got, frame)
    px, trunc = rfa.redact_host(got, faces, scale, **spec)
    sp = rr.Spec(**spec)
    want, wpx, true = rr.redact_image(sp, frame, faces, scale)
    assert got.tobytes() == want.tobytes(), int((got != want).sum())
    k = min(len(faces), sp.max_regions)
    assert px[:k].tobytes() == wpx[:k].tobytes()
    assert trunc == (true > sp.max_regions)
    outside = np.ones(base.shape, bool)
    np.lib.stride_tricks.as_strided(outside.reshape(-1)[off:], frame.shape, frame.strides)[:] = False
    assert np.array_equal(base_copy[outside], np.asarray(base)[outside])      # nothing outside the view was written
    return got, px


# ---------------------------------------------------------------------------------------------- 1. regions
def test_struct_size():
    assert C.sizeof(_lib.rf_redact_spec) == 32


def edge_boxes(rows, cols):
    """boxes one ulp either side of an integer coordinate, across each frame side, wholly outside, larger than the frame, at +-1e9,
    non-finite, and reversed"""
    up, dn = (lambda v: float(np.nextafter(f32(v), f32(np.inf)))), (lambda v: float(np.nextafter(f32(v), f32(-np.inf))))
    boxes = []
    for v in (10.0, 20.0, 0.0, float(cols), float(rows)):
        for x in (dn(v), v, up(v)):
            boxes += [(x, 5.0, x + 7.0, 12.0), (3.0, x, 9.0, x + 4.0), (2.0, 2.0, x, x)]
    boxes += [(-8.0, 10.0, 6.0, 20.0), (cols - 5.0, 10.0, cols + 9.0, 20.0), (10.0, -6.0, 20.0, 4.0), (10.0, rows - 3.0, 20.0, rows + 8.0)]
    boxes += [(-50.0, -50.0, -20.0, -30.0), (cols + 10.0, 5.0, cols + 30.0, 9.0), (5.0, rows + 100.0, 9.0, rows + 120.0),
              (-300.0, 5.0, -200.0, 9.0)]
    boxes += [(-20.0, -30.0, cols + 40.0, rows + 50.0), (-5000.0, -5000.0, 9000.0, 9000.0)]
    boxes += [(-1e9, 5.0, 1e9, 9.0), (5.0, -1e9, 9.0, 1e9), (1e9, 1e9, 2e9, 2e9), (-2e9, -2e9, -1e9, -1e9), (3e38, 0.0, 3.3e38, 4.0),
              (-3e38, 0.0, 3e38, 4.0)]
    nan, inf = float("nan"), float("inf")
    boxes += [(nan, 1.0, 5.0, 5.0), (1.0, nan, 5.0, 5.0), (1.0, 1.0, nan, 5.0), (1.0, 1.0, 5.0, nan), (-inf, 1.0, 5.0, 5.0),
              (1.0, 1.0, inf, 5.0), (1.0, -inf, 5.0, inf)]
    boxes += [(20.0, 5.0, 10.0, 9.0), (5.0, 20.0, 9.0, 10.0), (7.0, 7.0, 7.0, 7.0)]
    return boxes


@pytest.mark.parametrize("margin", (-1.0, 0.0, 1.0, 0.37))
@pytest.mark.parametrize("scale", (1.0, BIG))
def test_regions_equal_the_reference(built_lib, margin, scale):
    rows, cols = 48, 64
    rng = np.random.default_rng(5)
    boxes = edge_boxes(rows, cols) + [tuple(f[1:5]) for f in seeded_faces(rng, rows, cols, 200)]
    n_valid = 0
    for cells in (0, 1, 64):
        sp = rr.Spec(margin=margin, cells=cells)
        for b in boxes:
            st, got = native_region(built_lib, b, scale, rows, cols, margin=margin, cells=cells)
            want = rr.region(sp, f32(b), scale, rows, cols)
            assert st == int(want.valid), (b, st)
            assert got.tobytes() == want.as_row().tobytes(), (b, got, want.as_row())
            if want.valid:
                n_valid += 1
                assert want.ux1 - want.ux0 >= 1 and want.uy1 - want.uy0 >= 1 and -4096 <= want.ux0 and want.ux1 <= 8193
    assert n_valid > 600


def test_margin_values(built_lib):
    for margin, want in ((-1.0, (10, 10, 21, 31)), (0.0, (8, 6, 23, 35)), (1.0, (0, -10, 31, 51))):
        st, got = native_region(built_lib, (10.0, 10.0, 20.0, 30.0), 1.0, 100, 100, margin=margin)
        assert st == 1 and tuple(got[:4]) == want, (margin, got)


# ---------------------------------------------------------------------------------------------- 2. whole frames
@pytest.mark.parametrize("shape", (rr.RECT, rr.ELLIPSE))
@pytest.mark.parametrize("mode", (rr.PIXELATE, rr.FILL))
@pytest.mark.parametrize("cells", (1, 2, 8, 64))
def test_frames_equal_the_reference(built_lib, shape, mode, cells):
    for name, frame in views().items():
        rows, cols = frame.shape[:2]
        rng = np.random.default_rng(cells * 4 + shape * 2 + mode)
        for k in (0, 1, 5):
            faces = seeded_faces(rng, rows, cols, k)
            check_host(frame, faces, mode=mode, shape=shape, cells=cells, fill=(9, 200, 31))
        # a box that covers the frame and more, with a coordinate scale
        check_host(frame, face_at(-3.0, -2.0, cols / 2.0, rows / 2.0)[None], BIG, mode=mode, shape=shape, cells=cells, fill=(1, 2, 3))


def test_cells_larger_than_the_region_and_c_of_one_are_the_identity(built_lib):
    """the identity is c = 1, which the definition gives when `cells` is at least the region's longer side; `cells` = 1 is the other
    end, one cell per region (the region's mean), and is compared with the reference in test_frames_equal_the_reference"""
    frame = views()["48x64 padded"]
    faces = np.stack([face_at(10.0, 10.0, 15.0, 14.0), face_at(30.0, 20.0, 33.0, 40.0)])
    for cells in (8, 64):           # regions 8 x 6 and 5 x 29 pixels at margin 0.2
        got, px = check_host(frame, faces[:1], cells=cells)
        assert np.array_equal(got, frame) and px[0] > 0
    got, _ = check_host(frame, faces, cells=64, shape=rr.ELLIPSE)
    assert np.array_equal(got, frame)
    got, _ = check_host(frame, faces, cells=64)
    assert np.array_equal(got, frame)


def test_an_ellipse_stays_inside_its_rectangle_and_a_single_pixel_is_owned(built_lib):
    frame = views()["48x64 padded"]
    faces = seeded_faces(np.random.default_rng(11), 48, 64, 4)
    got_e, px_e = check_host(frame, faces, mode=rr.FILL, shape=rr.ELLIPSE, fill=(255, 0, 255))
    got_r, px_r = check_host(frame, faces, mode=rr.FILL, shape=rr.RECT, fill=(255, 0, 255))
    changed_e, changed_r = (got_e != frame).any(2), (got_r != frame).any(2)
    assert not (changed_e & ~changed_r).any() and px_e.sum() < px_r.sum()
    # W = H = 1: margin none, a box inside one pixel
    one = face_at(20.25, 30.25, 20.5, 30.5)[None]
    st, reg = native_region(built_lib, one[0, 1:5], 1.0, 48, 64, margin=-1.0)
    assert st == 1 and tuple(reg[:4]) == (20, 30, 21, 31)
    got, px = check_host(frame, one, mode=rr.FILL, shape=rr.ELLIPSE, margin=-1.0, fill=(7, 8, 9))
    assert px[0] == 1 and tuple(got[30, 20]) == (7, 8, 9)


def test_overlapping_regions_go_to_the_lower_index_and_every_pixel_is_written_once(built_lib):
    frame = views()["48x64 padded"]
    three = np.stack([face_at(10.0, 10.0, 30.0, 30.0), face_at(20.0, 15.0, 45.0, 35.0), face_at(5.0, 25.0, 50.0, 40.0)])
    for faces in (three[:2], three):
        for shape in (rr.RECT, rr.ELLIPSE):
            sp = rr.Spec(shape=shape, mode=rr.FILL, margin=-1.0)
            got, px = check_host(frame, faces, shape=shape, mode=rr.FILL, margin=-1.0, fill=(0, 0, 0))
            masks = []
            for f in faces:
                r = rr.region(sp, f[1:5], 1.0, 48, 64)
                m = np.zeros((48, 64), bool)
                m[r.cy0:r.cy1, r.cx0:r.cx1] = rr.mask(sp, r)
                masks.append(m)
            union = np.logical_or.reduce(masks)
            assert px.sum() == union.sum()                                     # once each: the counts add up to the union
            assert px[0] == masks[0].sum() and px[1] == (masks[1] & ~masks[0]).sum()
            assert (masks[0] & masks[1]).any()
    # pixelate: where 0 and 1 overlap, the value is region 0's cell
    got, _ = check_host(frame, three, margin=-1.0, cells=2)
    sp = rr.Spec(margin=-1.0, cells=2)
    r0 = rr.region(sp, three[0, 1:5], 1.0, 48, 64)
    assert np.array_equal(got[r0.cy0:r0.cy1, r0.cx0:r0.cx1], rr.cell_image(frame, r0))


def test_fill_twice_is_idempotent_and_a_constant_frame_is_unchanged(built_lib):
    import retinaface_amd as rfa
    frame = np.ascontiguousarray(views()["48x64 padded"])
    faces = seeded_faces(np.random.default_rng(2), 48, 64, 5)
    once = frame.copy()
    rfa.redact_host(once, faces, mode=rr.FILL, shape=rr.ELLIPSE, fill=(3, 4, 5))
    twice = once.copy()
    rfa.redact_host(twice, faces, mode=rr.FILL, shape=rr.ELLIPSE, fill=(3, 4, 5))
    assert np.array_equal(once, twice) and not np.array_equal(once, frame)
    flat = np.full((48, 64, 3), (255, 1, 128), np.uint8)
    for cells in (1, 3, 8):
        got = flat.copy()
        px, _ = rfa.redact_host(got, faces, cells=cells)
        assert np.array_equal(got, flat) and px.sum() > 0


def test_a_cell_sum_beyond_16_bits(built_lib):
    """one cell of 300 x 300 pixels of value 255: a channel sum of 22 950 000"""
    frame = np.full((300, 300, 3), 255, np.uint8)
    frame[::2, ::2] = 254
    got, px = check_host(frame, face_at(0.0, 0.0, 299.0, 299.0)[None], cells=1, margin=-1.0)
    assert px[0] == 90000 and len(np.unique(got.reshape(-1, 3), axis=0)) == 1 and tuple(got[0, 0]) == (255, 255, 255)


def test_max_regions_cuts_the_list(built_lib):
    frame = views()["48x64 padded"]
    faces = seeded_faces(np.random.default_rng(8), 48, 64, 6)
    check_host(frame, faces, max_regions=4)
    check_host(frame, faces, max_regions=6)


def test_refusals(built_lib):
    import retinaface_amd as rfa
    lib = built_lib
    frame = np.zeros((8, 8, 3), np.uint8)
    f = _lib.rf_face.from_buffer_copy(face_at(1.0, 1.0, 5.0, 5.0).tobytes())
    out = (C.c_int * 9)()
    bad = [dict(mode=2), dict(mode=-1), dict(shape=2), dict(cells=65), dict(cells=-1), dict(margin=1.5), dict(margin=float("nan")),
           dict(margin=float("inf")), dict(max_regions=1025), dict(max_regions=-1)]
    for kw in bad:
        sp = rfa.redact_spec(**kw)
        assert lib.rf_redact_region(C.byref(sp), C.byref(f), 1.0, 8, 8, out) == _lib.RF_ERR_INVALID_ARG, kw
        before = frame.copy()
        assert lib.rf_redact_host(C.byref(sp), frame.ctypes.data, 8, 8, 24, C.byref(f), 1, 1.0, None) == _lib.RF_ERR_INVALID_ARG, kw
        assert np.array_equal(frame, before)
    sp = rfa.redact_spec()
    sp.struct_size = 28
    assert lib.rf_redact_region(C.byref(sp), C.byref(f), 1.0, 8, 8, out) == _lib.RF_ERR_INVALID_ARG
    sp = rfa.redact_spec()
    assert lib.rf_redact_region(C.byref(sp), None, 1.0, 8, 8, out) == _lib.RF_ERR_INVALID_ARG
    assert lib.rf_redact_region(C.byref(sp), C.byref(f), 1.0, 8, 8, None) == _lib.RF_ERR_INVALID_ARG
    assert lib.rf_redact_region(None, C.byref(f), 1.0, 8, 8, out) == 1                       # NULL spec: all defaults
    assert lib.rf_redact_host(C.byref(sp), frame.ctypes.data, 8, 8, 23, C.byref(f), 1, 1.0, None) == _lib.RF_ERR_INVALID_ARG    # step < cols * 3
    assert lib.rf_redact_host(C.byref(sp), frame.ctypes.data, 8, 8, 24, None, 1, 1.0, None) == _lib.RF_ERR_INVALID_ARG
    assert lib.rf_redact_host(C.byref(sp), frame.ctypes.data, 8, 8, 24, C.byref(f), -1, 1.0, None) == _lib.RF_ERR_INVALID_ARG
    assert lib.rf_redact_host(C.byref(sp), None, 0, 0, 0, C.byref(f), 1, 1.0, None) == 0     # an empty frame is skipped
    assert not frame.any()


# ---------------------------------------------------------------------------------------------- 3. a constructed face
def test_a_pasted_face_is_covered_and_the_rest_of_the_frame_is_untouched(built_lib, base_frame):
    """one 2 x 2-averaged face patch on a grey frame, redacted at its own box"""
    import retinaface_amd as rfa
    patch = base_frame[60:260, 500:700].astype(np.uint16)
    small = ((patch[0::2, 0::2] + patch[0::2, 1::2] + patch[1::2, 0::2] + patch[1::2, 1::2] + 2) // 4).astype(np.uint8)      # 100 x 100
    frame = np.full((240, 320, 3), 128, np.uint8)
    frame[70:170, 110:210] = small
    box = face_at(110.0, 70.0, 209.0, 169.0)
    for shape in (rr.RECT, rr.ELLIPSE):
        got, px = check_host(frame, box[None], shape=shape)
        r = rr.region(rr.Spec(), box[1:5], 1.0, 240, 320)
        outside = np.ones((240, 320), bool)
        outside[r.cy0:r.cy1, r.cx0:r.cx1] = False
        assert np.array_equal(got[outside], frame[outside])
        inside = got[r.cy0:r.cy1, r.cx0:r.cx1][rr.mask(rr.Spec(shape=shape), r)]
        assert len(np.unique(inside.reshape(-1, 3), axis=0)) <= 64
        assert px[0] == len(inside) and not np.array_equal(got[70:170, 110:210], small)
