"""Tiled detection, host side (no GPU): rf_tile_plan and rf_tile_map_face -- the plan, edge rule and mapping the gather kernel runs,
compiled for the host -- must equal tests/tile_ref.py; the plan covers every pixel with the promised overlap; bad specs are refused;
the reference's merge has the properties the definition states (ties broken by g, strict >, the single-tile plan is the identity);
and on the CPU oracle the 2 x 2 mosaic of the half-size base frame, whose 24 faces a shrunk pass partly loses, is found whole."""
import ctypes as C

import numpy as np
import pytest

import tile_ref as tr
from retinaface_amd import _lib, tile_map_face, tile_plan, tile_spec

NET = (448, 448)


def native_plan(rows, cols, net_h, net_w, overlap=0, full_frame=True, **kw):
    lib = _lib.load_library()
    sp = tile_spec(overlap, 0, full_frame, **kw)
    return lib.rf_tile_plan(C.byref(sp), rows, cols, net_h, net_w, None, 0)


PLAN_CASES = [
    # rows, cols, net_h, net_w
    (448, 448, 448, 448), (300, 200, 448, 448), (1, 1, 448, 448),           # L <= N
    (449, 448, 448, 448), (448, 449, 448, 448), (449, 449, 448, 448),       # L = N + 1
    (896, 448, 448, 448), (448, 1344, 448, 448), (896, 1344, 448, 448),     # exact multiples, each axis on its own
    (997, 448, 448, 448), (448, 1009, 448, 448), (997, 1009, 448, 448),     # primes
    (300, 1280, 448, 448),                                                  # fits in one dimension only
    (896, 1280, 448, 448), (2160, 3840, 448, 448), (3072, 4096, 448, 448),
    (1080, 1920, 320, 640), (641, 1283, 320, 640),                          # a net that is not square
]


@pytest.mark.parametrize("overlap", (-1, 0, 128, 447))
@pytest.mark.parametrize("full", (True, False))
def test_plan_equals_the_reference(overlap, full):
    for rows, cols, nh, nw in PLAN_CASES:
        if overlap >= min(nh, nw):
            continue
        try:
            want = tr.plan(rows, cols, nh, nw, overlap, full)
        except ValueError:                                                           # overlap N - 1 on a large frame: too many passes
            assert overlap == 447 and native_plan(rows, cols, nh, nw, overlap, full) == -1
            continue
        got = tile_plan(rows, cols, nh, nw, overlap, full)
        assert got.dtype == want.dtype and np.array_equal(got, want), (rows, cols, nh, nw, overlap, full)
        assert native_plan(rows, cols, nh, nw, overlap, full) == len(want)
    assert len(tr.plan(3072, 4096, 448, 448, 0, True)) == 12 * 9 + 1
    assert len(tr.plan(896, 1280, 448, 448, 128, True)) == 13 and len(tr.plan(896, 1280, 448, 448, 192, True)) == 16
    assert np.array_equal(tr.plan(300, 1280, 448, 448)[0], (0, 0, 448, 300))


@pytest.mark.parametrize("overlap", (-1, 0, 128, 447))
def test_plan_properties(overlap):
    for rows, cols, nh, nw in PLAN_CASES:
        if overlap >= min(nh, nw) or (overlap == 447 and native_plan(rows, cols, nh, nw, overlap, True) < 0):
            continue
        ov = tr.resolve(nh, nw, overlap)[0]
        tiles = tile_plan(rows, cols, nh, nw, overlap, False)
        for L, N, o, s in ((cols, nw, 0, 2), (rows, nh, 1, 3)):
            seg = sorted(set((int(t[o]), int(t[s])) for t in tiles))
            assert seg[0][0] == 0 and seg[-1][0] + seg[-1][1] == L
            assert all(size == min(L, N) for _, size in seg)
            for (a, sa), (b, _) in zip(seg, seg[1:]):
                assert a < b and a + sa - b >= ov, (rows, cols, overlap, seg)       # neighbours overlap by at least ov: no pixel is left out
        nx = len(set(int(t[0]) for t in tiles))
        assert all(np.array_equal(tiles[i][:2], (sorted(set(int(t[0]) for t in tiles))[i % nx], sorted(set(int(t[1]) for t in tiles))[i // nx]))
                   for i in range(len(tiles)))                                       # row-major: t = ty * nx + tx
        fits = rows <= nh and cols <= nw
        with_full = tile_plan(rows, cols, nh, nw, overlap, True)
        assert len(with_full) == len(tiles) + (0 if fits else 1)
        if not fits:
            assert np.array_equal(with_full[-1], (0, 0, cols, rows)) and np.array_equal(with_full[:-1], tiles)
        else:
            assert len(tiles) == 1 and np.array_equal(tiles[0], (0, 0, cols, rows))


def test_plan_refusals():
    lib = _lib.load_library()
    assert native_plan(896, 1280, 448, 448) == 13                                    # the default spec: overlap 112
    assert lib.rf_tile_plan(None, 896, 1280, 448, 448, None, 0) == 13                # a NULL spec is the default spec
    assert native_plan(449, 449, 448, 448, overlap=448) == -1 and native_plan(449, 449, 448, 448, overlap=447) == 5
    assert native_plan(896, 1280, 320, 640, overlap=320) == -1                       # >= min(net)
    for field, bad in (("struct_size", 16), ("struct_size", 24), ("max_faces", -1), ("max_faces", 4097), ("full_frame", 3), ("full_frame", -1)):
        sp = tile_spec()
        setattr(sp, field, bad)
        assert lib.rf_tile_plan(C.byref(sp), 896, 1280, 448, 448, None, 0) == -1, (field, bad)
    for ok in (dict(max_faces=1), dict(max_faces=4096)):
        assert native_plan(896, 1280, 448, 448, **ok) == 13
    for edge, want in ((223, 13), (224, -1), (100000, -1)):                          # a band of half the net would drop every interior face
        sp = tile_spec(0, edge)
        assert lib.rf_tile_plan(C.byref(sp), 896, 1280, 448, 448, None, 0) == want, edge
    with pytest.raises(ValueError):
        tr.resolve(448, 448, 0, 224)
    sp = tile_spec(0, 160)
    assert lib.rf_tile_plan(C.byref(sp), 1080, 1920, 320, 640, None, 0) == -1 and tr.resolve(320, 640, 0, 159) == (80, 159)
    assert native_plan(3072, 4096, 64, 64) == -1                                     # 85 x 64 tiles: more than 1024 passes
    assert native_plan(3072, 4096, 448, 448) == 109
    assert native_plan(4096, 4096, 448, 448) == -1 and native_plan(-1, 10, 448, 448) == -1      # frame limits
    assert native_plan(896, 1280, 0, 448) == -1
    with pytest.raises(_lib.RFError):
        tile_plan(3072, 4096, 64, 64)
    xy = (C.c_int * 8)(*([-7] * 8))                                                  # cap_tiles bounds what is written
    sp = tile_spec(128)
    assert lib.rf_tile_plan(C.byref(sp), 896, 1280, 448, 448, xy, 1) == 13 and list(xy) == [0, 0, 448, 448, -7, -7, -7, -7]


def face_at(x1, y1, x2, y2, score=0.9):
    f = np.zeros(15, np.float32)
    f[0] = score
    f[1:5] = (x1, y1, x2, y2)
    f[5:10] = np.linspace(x1, x2, 5, dtype=np.float32) + np.float32(0.3)
    f[10:15] = np.linspace(y1, y2, 5, dtype=np.float32) + np.float32(0.7)
    return f


def edge_faces(tw=448, th=448):
    """boxes around every side of a tile: inside, on the band's boundary for edge 8 and 0, one ulp either side of it"""
    out = [face_at(100.5, 120.25, 180.75, 200.5)]
    for e in (8, 0, 1):
        lo, hx, hy = np.float32(e), np.float32(tw - 1 - e), np.float32(th - 1 - e)
        for v in (lo, np.nextafter(lo, np.float32(-1)), np.nextafter(lo, np.float32(1e9))):
            out.append(face_at(v, 100, 200, 210))
            out.append(face_at(100, v, 200, 210))
        for v in (hx, np.nextafter(hx, np.float32(0)), np.nextafter(hx, np.float32(1e9))):
            out.append(face_at(100, 110, v, 210))
        for v in (hy, np.nextafter(hy, np.float32(0)), np.nextafter(hy, np.float32(1e9))):
            out.append(face_at(100, 110, 200, v))
    out.append(face_at(0, 0, 447, 447))
    out.append(face_at(3.3, 2.2, 445.1, 446.9))
    return out


@pytest.mark.parametrize("edge", (-1, 0, 8))
def test_map_face_equals_the_reference_bit_for_bit(edge):
    kept = dropped = 0
    for rows, cols, overlap in ((997, 1009, 128), (896, 1280, 128), (300, 1280, 0), (449, 449, -1)):
        tiles = tr.plan(rows, cols, 448, 448, overlap, True)
        for t in range(len(tiles)):
            tw, th = int(tiles[t][2]), int(tiles[t][3])
            for f in edge_faces(min(tw, 448), min(th, 448)):
                want = tr.map_face(f, t, rows, cols, 448, 448, overlap, edge, True)
                got = tile_map_face(f, t, rows, cols, 448, 448, overlap, edge, True)
                assert (got is None) == (want is None), (rows, cols, t, f[1:5])
                if want is not None:
                    assert got.tobytes() == want.tobytes(), (rows, cols, t, f[1:5])
                    kept += 1
                else:
                    dropped += 1
    assert kept and dropped                                                          # both outcomes occur for every edge width
    # frame sides never drop, interior sides do: the corner tiles of a 3 x 3 plan against its centre tile
    tiles = tr.plan(997, 1009, 448, 448, 128, False)
    assert len(tiles) == 9
    touching = face_at(0, 0, 447, 447)
    for t, want_kept in ((0, False), (4, False), (8, False)):
        assert (tr.map_face(touching, t, 997, 1009, 448, 448, 128, 8, False) is not None) == want_kept
    left_top = face_at(0, 0, 100, 100)
    assert tr.map_face(left_top, 0, 997, 1009, 448, 448, 128, 8, False) is not None        # a frame corner
    assert tr.map_face(left_top, 4, 997, 1009, 448, 448, 128, 8, False) is None
    assert tr.map_face(left_top, 1, 997, 1009, 448, 448, 128, 8, False) is None            # interior left side, frame top
    assert tr.map_face(face_at(100, 0, 200, 100), 1, 997, 1009, 448, 448, 128, 8, False) is not None
    # the band's boundary is kept: x1 == edge, x2 == tw - 1 - edge
    on = face_at(8, 8, 439, 439)
    m = tr.map_face(on, 4, 997, 1009, 448, 448, 128, 8, False)
    assert m is not None and m[1] == np.float32(8) + np.float32(tiles[4][0]) and m[0] == on[0]
    assert tr.map_face(face_at(np.nextafter(np.float32(8), np.float32(0)), 8, 439, 439), 4, 997, 1009, 448, 448, 128, 8, False) is None
    assert tr.map_face(face_at(8, 8, np.nextafter(np.float32(439), np.float32(1e9)), 439), 4, 997, 1009, 448, 448, 128, 8, False) is None
    # the full-frame pass: nothing is dropped, one fp32 multiply by a scale that is not representable
    sc = tr.frame_scale(896, 1280, 448, 448)
    assert sc == np.float32(1280) / np.float32(448) and float(sc) != 1280 / 448
    full = tr.map_face(touching, 12, 896, 1280, 448, 448, 128, 8, True)
    assert full[0] == touching[0] and np.array_equal(full[1:], touching[1:] * sc)
    assert tile_map_face(touching, 12, 896, 1280, 448, 448, 128, 8, True).tobytes() == full.tobytes()
    with pytest.raises(_lib.RFError):
        tile_map_face(touching, 13, 896, 1280, 448, 448, 128, 8, True)


def test_merge_properties():
    rows, cols = 997, 1009
    tiles = tr.plan(rows, cols, 448, 448, 128, True)
    passes = [np.zeros((0, 15), np.float32) for _ in tiles]
    # the same face seen by two tiles with EQUAL scores: the lower g wins, whichever order the passes come in
    x0a, x0b = int(tiles[0][0]), int(tiles[1][0])
    a = face_at(300 - x0a, 100, 380 - x0a, 200, 0.75)
    b = face_at(300 - x0b, 100, 380 - x0b, 200, 0.75)
    passes[0], passes[1] = a[None], b[None]
    faces, count, src, ncand = tr.merge(rows, cols, passes, 448, 448, 0.4, 256, 128, 8, True)
    assert count == 1 and ncand == 2 and list(src) == [0] and faces[0][1] == np.float32(300)
    # k breaks ties inside a pass; two distant faces with equal scores keep the pass's order
    passes[0] = np.stack([face_at(20, 20, 60, 60, 0.5), face_at(200, 200, 260, 260, 0.5)])
    passes[1] = np.zeros((0, 15), np.float32)
    faces, count, src, _ = tr.merge(rows, cols, passes, 448, 448, 0.4, 256, 128, 8, True)
    assert count == 2 and faces[0][1] == 20 and faces[1][1] == 200
    # an IoU exactly AT the threshold is kept (strict >): 10 x 10 boxes shifted by 5 have IoU 50 / 150 = 1 / 3 in fp32
    p = np.stack([face_at(100, 100, 109, 109, 0.9), face_at(105, 100, 114, 109, 0.8)])
    thr = float(np.float32(50) / np.float32(150))
    one = [p] + [np.zeros((0, 15), np.float32)] * 12
    assert tr.merge(rows, cols, one, 448, 448, thr, 256, 128, 8, True)[1] == 2
    assert tr.merge(rows, cols, one, 448, 448, float(np.nextafter(np.float32(thr), np.float32(0))), 256, 128, 8, True)[1] == 1
    # the single-tile plan: what comes in goes out (a detect result is already the fixed point of its NMS)
    from conftest import golden
    det = golden("crop448_mnet25.npz")["det"]
    faces, count, src, ncand = tr.merge(448, 448, [det], 448, 448, 0.4, 256)
    assert count == ncand == len(det) and faces.tobytes() == det.tobytes() and not src.any()
    # max_faces cuts the list, the count stays true
    faces, count, _, _ = tr.merge(448, 448, [det], 448, 448, 0.4, 256, max_faces=1)
    assert count == len(det) > 1 and faces.tobytes() == det[:1].tobytes()


@pytest.mark.parametrize("stem", ("mnet25", "mnet-deconv-0517"))
def test_mosaic_through_the_oracle(oracles, base_frame, stem):
    frame = tr.mosaic(base_frame)
    assert frame.shape == (896, 1280, 3)
    oracle = oracles[stem]
    native = oracle.detect(frame, 0.5, 0.4, net_hw=(896, 1280)).rows()
    assert len(native) == 24
    tiles = tr.plan(896, 1280, 448, 448, 128, True)
    assert len(tiles) == 13
    passes = [oracle.detect(v, 0.5, 0.4, net_hw=NET).rows() for v in tr.views(frame, tiles)]
    assert len(passes[12]) < 24                                                      # the shrunk pass alone loses faces
    faces, count, src, _ = tr.merge(896, 1280, passes, 448, 448, 0.4, 256, 128, 8, True)
    assert count == len(faces) == 24
    best_native = [max(tr.iou_plus1(n[1:5], f[1:5]) for f in faces) for n in native]
    best_tiled = [max(tr.iou_plus1(n[1:5], f[1:5]) for n in native) for f in faces]
    assert min(best_native) >= 0.5 and min(best_tiled) >= 0.5, (min(best_native), min(best_tiled))
    assert len(set(int(np.argmax([tr.iou_plus1(n[1:5], f[1:5]) for f in faces])) for n in native)) == 24      # one tiled face each
