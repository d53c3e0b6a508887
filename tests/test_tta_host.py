"""Flip test-time augmentation on the host (no GPU): rf_tta_map_face and rf_tta_merge_host -- the code the kernels run, compiled for
the host -- against tests/tta_ref.py byte for byte on constructed faces, the refusals, and crop448 with its mirror end to end through
the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import tta_ref as tr
from retinaface_amd import _lib, tta_map_face, tta_merge_host, tta_spec

MD = 256
NMS = 0.4
NET = (448, 448)
LM_X = np.array([0.3, 0.7, 0.5, 0.35, 0.65], np.float32)
LM_Y = np.array([0.4, 0.4, 0.6, 0.8, 0.8], np.float32)


def face(x1, y1, w, h, score):
    """a face in whatever coordinates the caller means, landmarks at fixed fractions of the box (left and right differ)"""
    f = np.zeros(15, np.float32)
    f[0] = score
    f[1:5] = (x1, y1, x1 + w, y1 + h)
    f[5:10] = f[1] + np.float32(w) * LM_X
    f[10:15] = f[2] + np.float32(h) * LM_Y
    return f


def quarter(f):
    """coordinates on a quarter-pixel grid: c - (c - x) == x exactly, so the mapping of pass 1 is its own inverse at scale 1"""
    g = f.copy()
    g[1:] = np.round(g[1:] * 4) / 4
    return g


def in_pass1(f, cols):
    """the face of the MIRRORED pass that maps to f (quarter-pixel coordinates, a frame that fits the net)"""
    return tr.map_face(f, 1, 448, cols, *NET)


def as_passes(pass0, pass1):
    return [np.stack(p).astype(np.float32) if len(p) else np.zeros((0, 15), np.float32) for p in (pass0, pass1)]


def check_host(passes, rows=448, cols=448, thr=NMS, md=MD, **kw):
    """rf_tta_merge_host against tta_ref.merge, byte for byte; returns the reference tuple"""
    vote = kw.get("vote", True)
    want = tr.merge(rows, cols, passes, *NET, thr, md, vote, kw.get("max_faces", 0))
    faces, count, votes, src, truncated = tta_merge_host(passes, rows, cols, *NET, thr, md, flip=len(passes) == 2, **kw)
    limit = min(kw.get("max_faces", 0) or md, kw["cap"] if kw.get("cap") is not None else md)
    assert count == want[1]
    assert faces.tobytes() == want[0][:limit].tobytes()
    assert list(votes) == list(want[2][:limit]) and list(src) == list(want[3][:limit])
    assert truncated == (count > limit or any(len(p) > md for p in passes))
    return want


# ---------------------------------------------------------------------------------------------- mapping
@pytest.mark.parametrize("cols", (1, 2, 448, 449, 1280, 4096))
def test_map_face_equals_the_reference_bit_for_bit(cols):
    rng = np.random.default_rng(cols)
    rows = {1: 1, 2: 7, 448: 448, 449: 300, 1280: 896, 4096: 3072}[cols]
    for net in (NET, (3072, 4096)):                         # the second net holds every frame: scale exactly 1
        scale = tr.frame_scale(rows, cols, *net)
        assert (scale == 1) == (net != NET or cols <= 448)
        if cols == 1280 and net == NET:
            assert scale == np.float32(1280) / np.float32(448)
        faces = [face(0.0, 0.0, float(cols - 1), float(rows - 1), 0.99),            # coordinates at 0 and at cols - 1
                 face(float(cols - 1), 0.0, 0.0, 1.0, 0.5)]
        for _ in range(20):
            f = rng.uniform(-20, net[1] + 20, 15).astype(np.float32)
            f[0] = np.float32(rng.uniform(0.5, 1))
            faces.append(f)
        for f in faces:
            for p in (0, 1):
                got = tta_map_face(f, p, rows, cols, *net)
                assert got.tobytes() == tr.map_face(f, p, rows, cols, *net).tobytes(), (cols, net, p)
            if scale == 1:
                assert tta_map_face(f, 0, rows, cols, *net).tobytes() == f.tobytes()


def test_map_face_mirrors_and_swaps_the_landmark_pairs():
    cols = 449
    f = face(100.0, 50.0, 40.0, 60.0, 0.75)
    m = tta_map_face(f, 1, 300, cols, 3072, 4096)
    c = np.float32(cols - 1)
    assert m[0] == f[0] and m[1] == c - f[3] and m[3] == c - f[1] and m[2] == f[2] and m[4] == f[4]
    assert list(m[5:10]) == [c - f[6], c - f[5], c - f[7], c - f[9], c - f[8]]
    assert list(m[10:15]) == [f[11], f[10], f[12], f[14], f[13]]
    assert m[5] < m[6] and m[8] < m[9]                      # the left eye stays on the left
    # integer coordinates, scale 1: mapping twice gives the original bytes
    g = np.arange(15, dtype=np.float32) * 7 + 3
    for cols in (1, 2, 448, 449, 1280, 4096):
        twice = tta_map_face(tta_map_face(g, 1, 1, cols, 3072, 4096), 1, 1, cols, 3072, 4096)
        assert twice.tobytes() == g.tobytes()


def test_map_face_refusals():
    lib = _lib.load_library()
    f, g = _lib.rf_face(), _lib.rf_face()
    for args in ((448, 448, 448, 448, 2), (448, 448, 448, 448, -1), (0, 448, 448, 448, 0), (448, 0, 448, 448, 0), (448, 448, 0, 448, 0),
                 (4097, 3072, 448, 448, 0)):
        assert lib.rf_tta_map_face(*args, C.byref(f), C.byref(g)) == _lib.RF_ERR_INVALID_ARG, args
    assert lib.rf_tta_map_face(448, 448, 448, 448, 0, None, C.byref(g)) == _lib.RF_ERR_INVALID_ARG
    assert lib.rf_tta_map_face(448, 448, 448, 448, 1, C.byref(f), C.byref(g)) == 0


# ---------------------------------------------------------------------------------------------- merge
def test_merge_of_zero_one_and_two_candidates():
    a = quarter(face(100, 100, 40, 40, 0.9))
    assert check_host(as_passes([], []))[1] == 0
    want = check_host(as_passes([a], []))
    assert want[1] == 1 and want[0].tobytes() == a[None].tobytes() and list(want[2]) == [1] and list(want[3]) == [0]
    want = check_host(as_passes([], [in_pass1(a, 448)]))
    assert want[1] == 1 and want[0].tobytes() == a[None].tobytes() and list(want[3]) == [1]
    b = quarter(face(102, 101, 40, 40, 0.8))
    want = check_host(as_passes([a], [in_pass1(b, 448)]))
    assert want[1] == 1 and list(want[2]) == [2] and want[0][0][0] == a[0]
    assert a[1] < want[0][0][1] < b[1]                      # between the two, nearer the heavier one
    assert abs(float(want[0][0][1]) - (0.9 * 100 + 0.8 * 102) / 1.7) < 1e-4
    far = quarter(face(300, 300, 40, 40, 0.95))
    want = check_host(as_passes([a], [in_pass1(far, 448)]))
    assert want[1] == 2 and list(want[2]) == [1, 1] and list(want[3]) == [1, 0]


def test_singletons_keep_their_bytes():
    rng = np.random.default_rng(1)
    grid = [face(8 + 44 * (j % 10) + float(rng.integers(0, 4)) / 4, 8 + 44 * (j // 10) + 0.25, 30 + float(rng.uniform(0, 5)), 33.3,
                 0.5 + float(rng.integers(1, 32)) / 64) for j in range(100)]
    grid = [quarter(f) for f in grid]
    p0 = sorted(grid[::2], key=lambda f: -f[0])
    p1 = sorted((in_pass1(f, 448) for f in grid[1::2]), key=lambda f: -f[0])
    passes = as_passes(p0, p1)
    want = check_host(passes)
    cand, g = tr.candidates(448, 448, passes, *NET, MD)
    assert want[1] == 100 and (want[2] == 1).all()
    assert sorted(r.tobytes() for r in want[0]) == sorted(r.tobytes() for r in cand)        # (s * v) / s == v
    # a frame larger than the net: the scale multiplies first, singletons still keep the bytes of their mapped candidate
    passes = as_passes(sorted(grid, key=lambda f: -f[0]), [])
    want = check_host(passes, rows=896, cols=1280)
    cand, g = tr.candidates(896, 1280, passes, *NET, MD)
    assert want[1] == 100 and (want[2] == 1).all() and cand[0][1] != passes[0][0][1] and sorted(r.tobytes() for r in want[0]) == sorted(r.tobytes() for r in cand)


def cluster_passes(count, seed=2, cols=448):
    """`count` faces around one place, dealt over the two passes in score order"""
    rng = np.random.default_rng(seed)
    fs = [quarter(face(200 + float(rng.uniform(-3, 3)), 150 + float(rng.uniform(-3, 3)), 60 + float(rng.uniform(-2, 2)), 70, 0.5 + float(rng.integers(1, 32)) / 64))
          for _ in range(count)]
    fs[0][0] = np.float32(0.999)                           # the head
    p0 = sorted(fs[::2], key=lambda f: -f[0])
    p1 = sorted((in_pass1(f, cols) for f in fs[1::2]), key=lambda f: -f[0])
    return as_passes(p0, p1)


def test_one_cluster_of_300():
    want = check_host(cluster_passes(300))
    assert want[1] == 1 and list(want[2]) == [300] and want[0][0][0] == np.float32(0.999)
    assert 197 < want[0][0][1] < 203


def test_chain_threshold_and_ties():
    a, b, c = (quarter(face(100 + 15 * j, 100, 40, 40, 0.9 - 0.1 * j)) for j in range(3))
    assert tr.iou_plus1(a[1:5], b[1:5]) > NMS > tr.iou_plus1(a[1:5], c[1:5]) and tr.iou_plus1(b[1:5], c[1:5]) > NMS
    want = check_host(as_passes([a, c], [in_pass1(b, 448)]))
    assert want[1] == 2 and list(want[2]) == [2, 1] and want[0][1].tobytes() == c.tobytes()          # B joins A, C is its own head
    # an IoU exactly AT the threshold is not a member (strict >): 10 x 10 boxes shifted by 5 have IoU 50 / 150 in fp32
    p, q = face(100, 100, 9, 9, 0.9), face(105, 100, 9, 9, 0.8)
    thr = float(np.float32(50) / np.float32(150))
    assert list(check_host(as_passes([p], [in_pass1(q, 448)]), thr=thr)[2]) == [1, 1]
    assert list(check_host(as_passes([p], [in_pass1(q, 448)]), thr=float(np.nextafter(np.float32(thr), np.float32(0))))[2]) == [2]
    # equal scores across the passes: g decides, so pass 0 heads the cluster whichever box is which
    for first, second in ((a, b), (b, a)):
        x, y = first.copy(), second.copy()
        x[0] = y[0] = np.float32(0.75)
        want = check_host(as_passes([x], [in_pass1(y, 448)]))
        assert want[1] == 1 and list(want[3]) == [0] and list(want[2]) == [2]
    # ... and k inside a pass
    x, y = a.copy(), b.copy()
    x[0] = y[0] = np.float32(0.75)
    want = check_host(as_passes([y, x], []), vote=False)
    assert want[1] == 1 and want[0][0].tobytes() == y.tobytes()


def test_vote_on_and_off_give_the_same_heads_and_cuts_are_reported():
    rng = np.random.default_rng(5)
    fs = []
    for j in range(40):                                    # 40 places, 1..6 faces each
        x, y = 10 + 70 * (j % 6), 10 + 60 * (j // 6)
        for _ in range(int(rng.integers(1, 7))):
            fs.append(quarter(face(x + float(rng.uniform(-4, 4)), y + float(rng.uniform(-4, 4)), 40, 44, 0.5 + float(rng.integers(1, 32)) / 64)))
    p0 = sorted(fs[::2], key=lambda f: -f[0])
    p1 = sorted((in_pass1(f, 448) for f in fs[1::2]), key=lambda f: -f[0])
    passes = as_passes(p0, p1)
    on = check_host(passes)
    off = check_host(passes, vote=False)
    assert on[1] == off[1] == 40 and list(on[2]) == list(off[2]) and list(on[3]) == list(off[3]) and max(on[2]) > 2
    assert on[0][:, 0].tobytes() == off[0][:, 0].tobytes() and on[0].tobytes() != off[0].tobytes()
    cand, g = tr.candidates(448, 448, passes, *NET, MD)
    assert {r.tobytes() for r in off[0]} <= {r.tobytes() for r in cand}
    # max_faces and cap cut the list; the count stays true and the call says so
    check_host(passes, max_faces=7)
    check_host(passes, cap=5)
    check_host(passes, max_faces=9, cap=3)
    check_host(passes, cap=0)
    # flip off: one pass; a pass count above max_detections is clamped and reported
    check_host(passes[:1])
    check_host(passes, md=16)
    assert tta_merge_host(passes, 448, 448, *NET, NMS, 16)[4]


def test_merge_refusals():
    lib = _lib.load_library()
    faces = (_lib.rf_face * (2 * MD))()
    pc = (C.c_int * 2)(0, 0)
    out = (_lib.rf_face * MD)()
    count = C.c_int(-7)

    def call(sp, rows=448, cols=448, nh=448, nw=448, md=MD, faces=faces, pc=pc, out=out, cap=MD, count=C.byref(count)):
        return lib.rf_tta_merge_host(sp, rows, cols, nh, nw, 0.4, md, faces, pc, out, cap, count, None, None)
    assert call(None) == 0 and count.value == 0
    good = tta_spec()
    assert call(C.byref(good)) == 0
    for field, value in (("struct_size", 12), ("struct_size", 20), ("flip", 3), ("flip", -1), ("vote", 3), ("vote", -1), ("max_faces", 4097),
                         ("max_faces", -1)):
        sp = tta_spec()
        setattr(sp, field, value)
        count.value = -7
        assert call(C.byref(sp)) == _lib.RF_ERR_INVALID_ARG and count.value == -7, (field, value)
    for kw in (dict(md=0), dict(md=4097), dict(nh=0), dict(rows=-1), dict(rows=4097, cols=3072), dict(faces=None), dict(pc=None), dict(count=None),
               dict(cap=-1), dict(out=None), dict(pc=(C.c_int * 2)(0, -1))):
        assert call(None, **kw) == _lib.RF_ERR_INVALID_ARG, kw
    assert call(None, out=None, cap=0) == 0
    with pytest.raises(_lib.RFError):
        tta_merge_host([np.zeros((0, 15), np.float32)], 448, 448, *NET, NMS, MD)             # flip on wants two passes


# ---------------------------------------------------------------------------------------------- end to end through the CPU oracle
@pytest.mark.parametrize("stem", ("mnet25", "mnet-deconv-0517"))
def test_crop448_and_its_mirror_through_the_oracle(oracles, crop448, stem):
    oracle = oracles[stem]
    plain = oracle.detect(crop448, 0.5, NMS, net_hw=NET).rows()
    flipped = oracle.detect(tr.mirror(crop448), 0.5, NMS, net_hw=NET).rows()
    assert len(plain) == 2 == len(flipped)
    passes = [plain, flipped]
    want = check_host(passes)
    assert want[1] == 2 and list(want[2]) == [2, 2]
    back = np.stack([tr.map_face(f, 1, 448, 448, *NET) for f in flipped])
    for f in plain:                                        # the mirrored pass, mapped back, lands on the plain faces: box and landmarks
        k = int(np.argmax([tr.iou_plus1(f[1:5], b[1:5]) for b in back]))
        assert tr.iou_plus1(f[1:5], back[k][1:5]) >= 0.9
        assert np.abs(f[5:15] - back[k][5:15]).max() < 0.08 * (f[3] - f[1])
        assert max(tr.iou_plus1(f[1:5], m[1:5]) for m in want[0]) >= 0.9
