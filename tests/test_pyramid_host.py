"""Zoom-pyramid detection on the host (no GPU): rf_zoom_host, rf_pyramid_plan, rf_pyramid_map_face and rf_pyramid_merge_host -- the code
the kernels run, compiled for the host -- against tests/pyramid_ref.py byte for byte, the refusals, and the 3 x 3 mosaic of the base
frame shrunk eight times (54 faces of 11 to 14 px) end to end through the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import pyramid_ref as pr
import tile_ref
from retinaface_amd import (_lib, pyramid_map_face, pyramid_merge_host, pyramid_plan, pyramid_spec, tile_map_face, zoom_host)

MD = 256
NMS = 0.4
NET = (448, 448)
ZOOM_SHAPES = ((1, 1), (1, 2), (3, 5), (7, 9), (113, 161))


def noise(rows, cols, seed=0):
    return np.random.default_rng(seed + 1000 * rows + cols).integers(0, 256, (rows, cols, 3), dtype=np.uint8)


def windows(rows, cols, z):
    """(x0, y0, tw, th) of the enlarged frame: whole, and windows touching every border and none (where the frame has room)"""
    W, H = z * cols, z * rows
    out = {(0, 0, W, H), (0, 0, max(W // 2, 1), max(H // 2, 1)), (W - max(W // 2, 1), H - max(H // 2, 1), max(W // 2, 1), max(H // 2, 1)),
           (0, H - 1, W, 1), (W - 1, 0, 1, H)}
    if W >= 4 and H >= 4:
        out |= {(1, 1, W - 2, H - 2), (W // 4, 1, W // 2, H - 2), (1, H // 4, W - 2, H // 2), (0, 1, 3, 2), (W - 3, H - 3, 3, 2)}
    if W >= 16:
        out |= {(3, 2, 5, 3), (W - 9, 1, 7, H - 2), (2, 0, 12, H)}
    return sorted(out)


# ---------------------------------------------------------------------------------------------- zoom
@pytest.mark.parametrize("z", (2, 4))
@pytest.mark.parametrize("shape", ZOOM_SHAPES)
def test_zoom_equals_the_reference_byte_for_byte(shape, z):
    rows, cols = shape
    frame = noise(rows, cols)
    whole = pr.zoom(frame, z)
    assert whole.shape == (z * rows, z * cols, 3)
    for x0, y0, tw, th in windows(rows, cols, z):
        want = pr.zoom(frame, z, x0, y0, tw, th)
        assert np.array_equal(want, whole[y0:y0 + th, x0:x0 + tw])                    # a tile is a window of the zoomed frame
        assert zoom_host(frame, z, x0, y0, tw, th).tobytes() == want.tobytes(), (shape, z, x0, y0, tw, th)
    # a pitched source (an ROI view at an odd offset) and a pitched destination whose guard bytes stay
    big = noise(rows + 2, cols + 3, 7)
    view = big[1:1 + rows, 2:2 + cols]
    x0, y0, tw, th = windows(rows, cols, z)[-1]
    dst = np.full((th + 2, tw + 5, 3), 0xA5, np.uint8)
    zoom_host(view, z, x0, y0, tw, th, out=dst[1:1 + th, 2:2 + tw])
    assert np.array_equal(dst[1:1 + th, 2:2 + tw], pr.zoom(np.ascontiguousarray(view), z, x0, y0, tw, th))
    guard = dst.copy()
    guard[1:1 + th, 2:2 + tw] = 0xA5
    assert (guard == 0xA5).all()


@pytest.mark.parametrize("z", (2, 4))
def test_zoom_properties(z):
    for v in (0, 1, 127, 254, 255):                                                   # a constant frame stays constant
        flat = np.full((7, 9, 3), v, np.uint8)
        assert (zoom_host(flat, z) == v).all() and (pr.zoom(flat, z) == v).all()
    frame = noise(7, 9, 3)
    up = pr.zoom(frame, z)
    assert np.array_equal(up[0, 0], frame[0, 0]) and np.array_equal(up[-1, -1], frame[-1, -1])        # the clamp at the frame border
    if z == 2:                                                                        # weights 3/4, 1/4 between two centres
        a, b = frame[3, 4].astype(int), frame[3, 5].astype(int)
        c, d = frame[4, 4].astype(int), frame[4, 5].astype(int)
        assert np.array_equal(up[7, 9], ((3 * a + b) * 3 + (3 * c + d) + 8) >> 4)
    # mirroring commutes with the zoom: the weights are symmetric
    assert np.array_equal(pr.zoom(np.ascontiguousarray(frame[:, ::-1]), z), pr.zoom(frame, z)[:, ::-1])


def test_zoom_refusals():
    lib = _lib.load_library()
    src, dst = noise(3, 5), np.zeros((40, 40, 3), np.uint8)
    ok = (src.ctypes.data, 3, 5, 15, 2, 0, 0, 10, 6, dst.ctypes.data, 120)
    assert lib.rf_zoom_host(*ok) == 0
    for i, bad in ((4, 1), (4, 3), (4, 8), (5, -1), (6, -1), (5, 1), (6, 1), (7, 11), (8, 7), (3, 14), (10, 29), (1, -1), (7, -1)):
        args = list(ok)
        args[i] = bad
        assert lib.rf_zoom_host(*args) == _lib.RF_ERR_INVALID_ARG, (i, bad)
    assert lib.rf_zoom_host(None, 3, 5, 15, 2, 0, 0, 10, 6, dst.ctypes.data, 120) == _lib.RF_ERR_INVALID_ARG
    assert lib.rf_zoom_host(src.ctypes.data, 3, 5, 15, 2, 0, 0, 0, 6, None, 0) == 0   # an empty window writes nothing


# ---------------------------------------------------------------------------------------------- plan
PLAN_CASES = [
    # rows, cols, net_h, net_w
    (1, 1, 448, 448), (50, 70, 448, 448), (112, 160, 448, 448), (224, 224, 448, 448), (225, 224, 448, 448), (224, 225, 448, 448),
    (336, 480, 448, 448), (448, 448, 448, 448), (449, 448, 448, 448), (448, 449, 448, 448), (500, 700, 448, 448), (896, 1280, 448, 448),
    (100, 1280, 448, 448), (1080, 1920, 320, 640), (160, 320, 320, 640), (161, 321, 320, 640), (80, 160, 320, 640),
]


@pytest.mark.parametrize("levels", (0, 1, 2, 3, 4, 5, 6, 7))
@pytest.mark.parametrize("overlap,full", ((0, True), (128, True), (-1, False)))
def test_plan_equals_the_reference(levels, overlap, full):
    for rows, cols, nh, nw in PLAN_CASES:
        want = pr.plan(rows, cols, nh, nw, levels, overlap, full)
        got = pyramid_plan(rows, cols, nh, nw, levels, overlap, full)
        assert got.dtype == want.dtype and np.array_equal(got, want), (rows, cols, nh, nw, levels)
        lv = levels or 3
        # the pass order: 1x in rf_tile_plan's order, then 2x, then 4x, each row-major without a full-frame pass
        assert list(got[:, 0]) == sorted(got[:, 0]) and set(got[:, 0]) == {z for b, z in enumerate(pr.ZOOMS) if lv >> b & 1}
        for b, z in enumerate(pr.ZOOMS):
            if lv >> b & 1:
                assert np.array_equal(got[got[:, 0] == z][:, 1:], tile_ref.plan(z * rows, z * cols, nh, nw, overlap, full and z == 1))


def test_plan_of_the_mosaic_and_defaults():
    lib = _lib.load_library()
    p = pyramid_plan(336, 480, *NET)
    assert len(p) == 9 and list(p[:, 0]) == [1, 1, 1, 2, 2, 2, 2, 2, 2]
    assert np.array_equal(p[2], (1, 0, 0, 480, 336)) and np.array_equal(p[3], (2, 0, 0, 448, 448)) and np.array_equal(p[8], (2, 512, 224, 448, 448))
    assert lib.rf_pyramid_plan(None, 336, 480, 448, 448, None, 0) == 9                # a NULL spec is the default spec
    assert len(pyramid_plan(112, 160, *NET)) == 2 and len(pyramid_plan(112, 160, *NET, levels=7)) == 1 + 1 + 2
    assert np.array_equal(pyramid_plan(0, 0, *NET), [[1, 0, 0, 0, 0]])                # an empty frame: one pass that finds nothing
    out = (C.c_int * 10)(*([-7] * 10))                                                # cap_passes bounds what is written
    assert lib.rf_pyramid_plan(None, 336, 480, 448, 448, out, 1) == 9 and list(out) == [1, 0, 0, 448, 336, -7, -7, -7, -7, -7]


def test_plan_refusals():
    lib = _lib.load_library()

    def native(rows, cols, nh=448, nw=448, **fields):
        sp = pyramid_spec()
        for k, v in fields.items():
            setattr(sp, k, v)
        return lib.rf_pyramid_plan(C.byref(sp), rows, cols, nh, nw, None, 0)

    assert native(336, 480) == 9
    for fields in (dict(levels=8), dict(levels=-1), dict(struct_size=24), dict(struct_size=32), dict(struct_size=20), dict(vote=3),
                   dict(vote=-1), dict(max_faces=-1), dict(max_faces=4097), dict(full_frame=3), dict(overlap=448), dict(edge=224)):
        assert native(336, 480, **fields) == _lib.RF_ERR_INVALID_ARG, fields
    for fields in (dict(levels=7), dict(vote=2), dict(max_faces=4096), dict(edge=223), dict(overlap=447, levels=1)):
        assert native(336, 480, **fields) > 0, fields
    assert native(-1, 10) == -1 and native(4096, 4096) == -1 and native(336, 480, 0, 448) == -1
    # more than 1024 passes: 1x alone fits (1 + ... ) but the levels together do not
    assert native(1000, 1000, 64, 64, levels=1) == 21 * 21 + 1 and native(1000, 1000, 64, 64, levels=3) == -1
    with pytest.raises(ValueError):
        pr.plan(1000, 1000, 64, 64, 3)
    # the 1 GiB cap on the zoom tiles: 88 + 336 tiles of 3 MiB at a 1024 x 1024 net
    assert native(3072, 4096, 1024, 1024, levels=1) == 5 * 4 + 1
    assert native(3072, 4096, 1024, 1024, levels=2) == 88 and native(3072, 4096, 1024, 1024, levels=4) == 336
    assert 88 * 3 * 1024 * 1024 < pr.MAX_ZOOM_BYTES < (88 + 336) * 3 * 1024 * 1024
    assert native(3072, 4096, 1024, 1024, levels=6) == -1 and native(3072, 4096, 1024, 1024, levels=7) == -1
    with pytest.raises(ValueError):
        pr.plan(3072, 4096, 1024, 1024, 6)
    with pytest.raises(_lib.RFError):
        pyramid_plan(3072, 4096, 1024, 1024, 6)


# ---------------------------------------------------------------------------------------------- mapping
def face_at(x1, y1, x2, y2, score=0.9):
    f = np.zeros(15, np.float32)
    f[0] = score
    f[1:5] = (x1, y1, x2, y2)
    f[5:10] = np.linspace(x1, x2, 5, dtype=np.float32) + np.float32(0.3)
    f[10:15] = np.linspace(y1, y2, 5, dtype=np.float32) + np.float32(0.7)
    return f


def edge_faces(tw, th, e):
    """boxes on every side of a tile: inside, on the band's boundary and one ulp either side of it"""
    out = [face_at(tw * 0.25 + 0.5, th * 0.25 + 0.25, tw * 0.5 + 0.75, th * 0.5 + 0.5), face_at(0, 0, tw - 1, th - 1)]
    lo, hx, hy = np.float32(e), np.float32(tw - 1 - e), np.float32(th - 1 - e)
    mx, my = tw * 0.5, th * 0.5
    for v in (lo, np.nextafter(lo, np.float32(-1)), np.nextafter(lo, np.float32(1e9))):
        out.append(face_at(v, my * 0.5, mx, my))
        out.append(face_at(mx * 0.5, v, mx, my))
    for v in (hx, np.nextafter(hx, np.float32(0)), np.nextafter(hx, np.float32(1e9))):
        out.append(face_at(mx * 0.5, my * 0.5, v, my))
    for v in (hy, np.nextafter(hy, np.float32(0)), np.nextafter(hy, np.float32(1e9))):
        out.append(face_at(mx * 0.5, my * 0.5, mx, v))
    return out


@pytest.mark.parametrize("levels,rows,cols", ((2, 500, 700), (4, 336, 480), (3, 336, 480), (7, 500, 700), (6, 50, 70)))
@pytest.mark.parametrize("edge", (-1, 0, 8))
def test_map_face_equals_the_reference_bit_for_bit(levels, rows, cols, edge):
    passes = pr.plan(rows, cols, *NET, levels, 128)
    ed = tile_ref.resolve(*NET, 128, edge)[1]
    kept = dropped = 0
    for p, (z, x0, y0, tw, th) in enumerate(tuple(int(v) for v in q) for q in passes):
        for f in edge_faces(min(tw, 448), min(th, 448), ed):
            want = pr.map_face(f, p, rows, cols, *NET, levels, 128, edge)
            got = pyramid_map_face(f, p, rows, cols, *NET, levels, 128, edge)
            assert (got is None) == (want is None), (p, f[1:5])
            if want is None:
                dropped += 1
                continue
            kept += 1
            assert got.tobytes() == want.tobytes(), (p, f[1:5])
            if z == 1:                                                                # a 1x pass is rf_tile_map_face, unchanged
                assert got.tobytes() == tile_map_face(f, p, rows, cols, *NET, 128, edge).tobytes()
    assert kept and (dropped or len(passes) == 1 or (rows, cols) == (50, 70))


def test_map_face_is_the_pixel_centre_correspondence():
    # 2x: a zoomed pixel X lies at (X - 0.5) / 2 of the source; 4x: (X - 1.5) / 4
    f = face_at(100, 40, 180, 120)
    m = pyramid_map_face(f, 0, 112, 160, *NET, levels=2)
    assert m[0] == f[0] and m[1] == np.float32(49.75) and m[2] == np.float32(19.75) and m[3] == np.float32(89.75)
    m = pyramid_map_face(f, 1, 336, 480, *NET, levels=4, overlap=128)                 # tile 1 of the 4x plan: x0 = 294
    p = pr.plan(336, 480, *NET, 4, 128)[1]
    assert tuple(p[:3]) == (4, 294, 0) and m[1] == np.float32((100 + 294) / 4 - 0.375) and m[2] == np.float32(40 / 4 - 0.375)
    with pytest.raises(_lib.RFError):
        pyramid_map_face(f, 2, 112, 160, *NET)                                        # the default plan has passes 0 and 1


# ---------------------------------------------------------------------------------------------- merge
def empty():
    return np.zeros((0, 15), np.float32)


def check_host(passes, rows, cols, thr=NMS, md=MD, levels=0, overlap=0, edge=0, full_frame=True, max_faces=0, vote=True, cap=None):
    """rf_pyramid_merge_host against pyramid_ref.merge, byte for byte; returns the reference tuple"""
    want = pr.merge(rows, cols, passes, *NET, thr, md, levels, overlap, edge, full_frame, max_faces, vote)
    faces, count, votes, src, truncated = pyramid_merge_host(passes, rows, cols, *NET, thr, md, levels, overlap, edge, full_frame,
                                                             max_faces, vote, cap)
    limit = min(max_faces or md, cap if cap is not None else md)
    assert count == want[1]
    assert faces.tobytes() == want[0][:limit].tobytes()
    assert list(votes) == list(want[2][:limit]) and list(src) == list(want[3][:limit])
    assert truncated == (count > limit or any(len(p) > md for p in passes))
    return want


def in_zoom(f, z):
    """the face of the single zoom tile of a small frame that maps to f: v' = z v + (z - 1) / 2 (exact on a quarter-pixel grid)"""
    g = f.copy()
    g[..., 1:] = g[..., 1:] * np.float32(z) + np.float32((z - 1) / 2)
    return g


def test_merge_of_zero_one_and_two_candidates():
    rows, cols = 112, 160                                                             # default plan: pass 0 (1x), pass 1 (2x)
    a = face_at(40, 30, 52, 44, 0.9)
    assert check_host([empty(), empty()], rows, cols)[1] == 0
    want = check_host([a[None], empty()], rows, cols)
    assert want[1] == 1 and want[0].tobytes() == a[None].tobytes() and list(want[2]) == [1] and list(want[3]) == [0]
    want = check_host([empty(), in_zoom(a, 2)[None]], rows, cols)
    assert want[1] == 1 and want[0].tobytes() == a[None].tobytes() and list(want[3]) == [1]
    # a face seen at both levels: one head with two votes, between the two and nearer the heavier one
    b = face_at(41, 30.5, 53, 44.5, 0.8)
    for vote in (True, False):
        want = check_host([a[None], in_zoom(b, 2)[None]], rows, cols, vote=vote)
        assert want[1] == 1 and list(want[2]) == [2] and list(want[3]) == [0] and want[0][0][0] == a[0]
        if vote:
            assert a[1] < want[0][0][1] < b[1] and abs(float(want[0][0][1]) - (0.9 * 40 + 0.8 * 41) / 1.7) < 1e-4
        else:
            assert want[0].tobytes() == a[None].tobytes()
    # two distant faces at two levels: two heads
    far = face_at(100, 60, 112, 74, 0.95)
    want = check_host([a[None], in_zoom(far, 2)[None]], rows, cols)
    assert want[1] == 2 and list(want[3]) == [1, 0] and list(want[2]) == [1, 1]


def test_merge_breaks_equal_scores_by_g_and_cuts():
    rows, cols = 112, 160
    a = face_at(40, 30, 52, 44, 0.75)
    b = face_at(41, 30, 53, 44, 0.75)
    # equal scores across levels: the lower pass index heads the cluster, whichever face it holds
    assert list(check_host([a[None], in_zoom(b, 2)[None]], rows, cols, vote=False)[0][0][1:2]) == [a[1]]
    assert list(check_host([b[None], in_zoom(a, 2)[None]], rows, cols, vote=False)[0][0][1:2]) == [b[1]]
    want = check_host([empty(), in_zoom(a, 2)[None], in_zoom(b, 4)[None]], 100, 112, levels=7, vote=False)     # one pass per level
    assert want[1] == 1 and list(want[3]) == [1] and want[0][0][1] == a[1]
    # cuts: max_faces and cap keep the first of the merge order, the count stays true
    many = np.stack([face_at(10 + 20 * i, 10, 20 + 20 * i, 22, 0.6 + 0.05 * i) for i in range(6)])
    for kw in (dict(max_faces=2), dict(cap=3), dict(max_faces=4, cap=1), dict(cap=0)):
        want = check_host([many, in_zoom(many, 2)], rows, cols, **kw)
        assert want[1] == 6
    # a pass holding more than max_detections is cut and reported
    faces, count, votes, src, truncated = pyramid_merge_host([many, empty()], rows, cols, *NET, NMS, 4)
    assert truncated and count == 4 and faces.tobytes() == pr.merge(rows, cols, [many[:4], empty()], *NET, NMS, 4)[0].tobytes()


@pytest.mark.parametrize("rows,cols,overlap", ((997, 1009, 128), (500, 700, 0), (300, 200, 0)))
def test_levels_1_without_vote_is_the_tiled_merge(rows, cols, overlap):
    rng = np.random.default_rng(rows)
    tiles = tile_ref.plan(rows, cols, *NET, overlap, True)
    passes = []
    for x0, y0, tw, th in tiles:
        k = int(rng.integers(0, 12))
        xy = rng.uniform(0, 400, (k, 2)).astype(np.float32)
        wh = rng.uniform(10, 80, (k, 2)).astype(np.float32)
        sc = np.sort(rng.uniform(0.5, 1, k).astype(np.float32))[::-1]
        passes.append(np.stack([face_at(x, y, x + w, y + h, s) for (x, y), (w, h), s in zip(xy, wh, sc)]) if k else empty())
    want = tile_ref.merge(rows, cols, passes, *NET, NMS, MD, overlap, 8, True)
    got = check_host(passes, rows, cols, levels=1, overlap=overlap, edge=8, vote=False)
    assert got[1] == want[1] and got[0].tobytes() == want[0].tobytes() and list(got[3]) == list(want[2]) and got[4] == want[3]


# ---------------------------------------------------------------------------------------------- the mosaic through the oracle
def placed_faces(stem_det):
    """centres of the 54 placed faces: the base frame's six (golden fixture), shrunk eight times (a small pixel X covers base pixels
    8X .. 8X + 7, centre 8X + 3.5), in each of the 3 x 3 copies of 112 x 160"""
    cx = ((stem_det[:, 1] + stem_det[:, 3]) / 2 - 3.5) / 8
    cy = ((stem_det[:, 2] + stem_det[:, 4]) / 2 - 3.5) / 8
    return [(x + 160 * i, y + 112 * j) for j in range(3) for i in range(3) for x, y in zip(cx, cy)]


@pytest.mark.parametrize("stem", ("mnet25", "mnet-deconv-0517"))
def test_mosaic_through_the_oracle(oracles, base_frame, stem):
    from conftest import golden
    frame = pr.mosaic(base_frame)
    assert frame.shape == (336, 480, 3)
    oracle = oracles[stem]
    plain = oracle.detect(frame, 0.5, NMS, net_hw=NET).rows()
    passes = pr.plan(336, 480, *NET)
    assert len(passes) == 9
    results = [oracle.detect(np.ascontiguousarray(v), 0.5, NMS, net_hw=NET).rows() for v in pr.images(frame, passes)]
    faces, count, votes, src, ncand = pr.merge(336, 480, results, *NET, NMS, MD)
    assert count == len(faces) == 54
    assert len(plain) < 54                                                            # measured: 28 (mnet25) and 19 (mnet-deconv-0517)
    centres = placed_faces(golden("fixture_%s.npz" % stem)["det"])
    assert len(centres) == 54
    for cx, cy in centres:                                                            # every placed face once, no duplicate
        assert sum(1 for f in faces if f[1] <= cx <= f[3] and f[2] <= cy <= f[4]) == 1, (cx, cy)
    got = pyramid_merge_host(results, 336, 480, *NET, NMS, MD)
    assert got[1] == 54 and got[0].tobytes() == faces.tobytes() and list(got[2]) == list(votes) and list(got[3]) == list(src)
