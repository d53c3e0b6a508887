"""Rotation-robust detection on the host (no GPU): rf_rot_map_face, rf_rotate_host and rf_rot_merge_host -- the code the kernels run,
compiled for the host -- against tests/rot_ref.py and np.rot90 byte for byte, the orientation outputs, the refusals, a window of the
base frame turned four ways end to end through the CPU oracle, and rot.h on its own under the address and UB sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import rot_ref as rr
from conftest import ROOT
from retinaface_amd import _lib, rot_map_face, rot_merge_host, rot_spec, rotate_host
from test_tta_host import face, quarter

MD = 256
NMS = 0.4
NET = (448, 448)
WIDE = (896, 1280)             # at this net a 896 x 1280 frame fits and its odd passes (1280 x 896) are shrunk


# ---------------------------------------------------------------------------------------------- mapping
@pytest.mark.parametrize("shape", ((1, 1), (7, 2), (448, 448), (300, 449), (896, 1280), (3072, 4096)))
def test_map_face_equals_the_reference_bit_for_bit(shape):
    rows, cols = shape
    rng = np.random.default_rng(rows * 5000 + cols)
    c, r = float(cols - 1), float(rows - 1)
    for net in (NET, WIDE):
        even, odd = rr.frame_scale(rows, cols, *net), rr.frame_scale(cols, rows, *net)
        if shape == (896, 1280) and net == WIDE:
            assert even == 1 and odd > 1                    # the passes of one frame do not share a scale
        faces = [face(0.0, 0.0, c, r, 0.99), face(0.0, 0.0, r, c, 0.98), face(c, r, 0.0, 0.0, 0.5), face(r, c, 0.0, 0.0, 0.5)]
        for _ in range(20):
            f = rng.uniform(-20, max(net) + 20, 15).astype(np.float32)
            f[0] = np.float32(rng.uniform(0.5, 1))
            faces.append(f)
        for f in faces:
            for k in range(4):
                got = rot_map_face(f, k, rows, cols, *net)
                assert got.tobytes() == rr.map_face(f, k, rows, cols, *net).tobytes(), (shape, net, k)
            if even == 1:
                assert rot_map_face(f, 0, rows, cols, *net).tobytes() == f.tobytes()


def test_map_face_turns_points_and_keeps_the_landmark_order():
    rows, cols = 300, 449
    c, r = np.float32(cols - 1), np.float32(rows - 1)
    big = (3072, 4096)
    f = face(100.0, 50.0, 40.0, 60.0, 0.75)
    m1, m2, m3 = (rot_map_face(f, k, rows, cols, *big) for k in (1, 2, 3))
    assert list(m1[1:5]) == [c - f[4], f[1], c - f[2], f[3]] and list(m1[5:10]) == list(c - f[10:15]) and list(m1[10:15]) == list(f[5:10])
    assert list(m2[1:5]) == [c - f[3], r - f[4], c - f[1], r - f[2]] and list(m2[5:10]) == list(c - f[5:10]) and list(m2[10:15]) == list(r - f[10:15])
    assert list(m3[1:5]) == [f[2], r - f[3], f[4], r - f[1]] and list(m3[5:10]) == list(f[10:15]) and list(m3[10:15]) == list(r - f[5:10])
    for m in (m1, m2, m3):
        assert m[0] == f[0] and m[1] < m[3] and m[2] < m[4]
    # the pixel the mapping names is the pixel np.rot90 moved: a marked pixel of pass k maps back to where it was in the frame
    for rows, cols in ((5, 9), (7, 3), (4, 4)):
        frame = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
        for k in range(4):
            turned = np.rot90(frame, k)
            for y in range(turned.shape[0]):
                for x in range(turned.shape[1]):
                    p = np.zeros(15, np.float32)
                    p[5], p[10] = x, y
                    m = rot_map_face(p, k, rows, cols, *big)
                    assert frame[int(m[10]), int(m[5])] == turned[y, x]


@pytest.mark.parametrize("shape", ((448, 448), (300, 449), (7, 2)))
def test_mapping_a_pass_after_its_inverse_returns_the_face(shape):
    rows, cols = shape
    rng = np.random.default_rng(3)
    big = (3072, 4096)
    for k in range(4):
        pr, pc = rr.pass_shape(k, rows, cols)
        for _ in range(25):
            f = quarter(face(float(rng.uniform(-10, cols)), float(rng.uniform(-10, rows)), float(rng.uniform(1, 90)), float(rng.uniform(1, 90)), 0.8))
            f[1:] += np.float32(0)                          # rounding can leave -0.0, whose sign no subtraction returns
            in_pass = rot_map_face(f, (4 - k) % 4, pr, pc, *big)
            assert in_pass.tobytes() == rr.unmap_face(f, k, rows, cols).tobytes()
            assert rot_map_face(in_pass, k, rows, cols, *big).tobytes() == f.tobytes(), (shape, k)


def test_map_face_refusals():
    lib = _lib.load_library()
    f, g = _lib.rf_face(), _lib.rf_face()
    for args in ((448, 448, 448, 448, 4), (448, 448, 448, 448, -1), (0, 448, 448, 448, 0), (448, 0, 448, 448, 0), (448, 448, 0, 448, 0),
                 (4097, 3072, 448, 448, 0)):
        assert lib.rf_rot_map_face(*args, C.byref(f), C.byref(g)) == _lib.RF_ERR_INVALID_ARG, args
    assert lib.rf_rot_map_face(448, 448, 448, 448, 0, None, C.byref(g)) == _lib.RF_ERR_INVALID_ARG
    assert lib.rf_rot_map_face(448, 448, 448, 448, 3, C.byref(f), C.byref(g)) == 0


# ---------------------------------------------------------------------------------------------- rotation
EDGES = (1, 2, 3, 5, 64, 65)


@pytest.mark.parametrize("rows", EDGES)
def test_rotate_host_equals_rot90(rows):
    rng = np.random.default_rng(rows)
    for cols in EDGES:
        frame = rng.integers(0, 256, size=(rows, cols, 3), dtype=np.uint8)
        wide = rng.integers(0, 256, size=(rows, cols + 3, 3), dtype=np.uint8)
        wide[:, :cols] = frame
        for k in range(4):
            want = np.rot90(frame, k)
            assert np.array_equal(rotate_host(frame, k), want), (rows, cols, k)
            assert np.array_equal(rotate_host(wide[:, :cols], k), want)                  # a pitched source
            dr, dc = want.shape[:2]
            buf = np.full((dr, dc + 2, 3), 0xAB, np.uint8)                                # a pitched destination
            got = rotate_host(frame, k, out=buf[:, :dc])
            assert got.base is buf or got is buf[:, :dc] or np.shares_memory(got, buf)
            assert np.array_equal(buf[:, :dc], want) and (buf[:, dc:] == 0xAB).all(), (rows, cols, k)


def test_rotate_host_refusals():
    lib = _lib.load_library()
    src, dst = np.zeros((4, 6, 3), np.uint8), np.zeros((6, 4, 3), np.uint8)
    call = lambda k=1, step=18, dstep=12, s=src.ctypes.data, d=dst.ctypes.data, rows=4, cols=6: lib.rf_rotate_host(s, rows, cols, step, k, d, dstep)  # noqa: E731
    assert call() == 0
    for kw in (dict(k=4), dict(k=-1), dict(step=17), dict(dstep=11), dict(s=None), dict(d=None), dict(rows=-1), dict(k=2, dstep=17)):
        assert call(**kw) == _lib.RF_ERR_INVALID_ARG, kw
    assert call(rows=0) == 0 and call(k=2, dstep=18) == 0


# ---------------------------------------------------------------------------------------------- merge
def deal(faces, rows, cols, rots=15, net=NET, md=MD):
    """frame-space faces dealt in turn over the passes of `rots` through the inverse mapping (and, where a pass is shrunk, divided by
    its scale), each pass in score order"""
    ks = rr.rot_list(rots)
    passes = [[] for _ in ks]
    for j, f in enumerate(faces):
        p = j % len(ks)
        g = rr.unmap_face(f, ks[p], rows, cols)
        g[1:] = g[1:] / rr.frame_scale(*rr.pass_shape(ks[p], rows, cols), *net)
        passes[p].append(g)
    out = []
    for p in passes:
        p = sorted(p, key=lambda f: -f[0])
        assert len(p) <= md
        out.append(np.stack(p).astype(np.float32) if p else np.zeros((0, 15), np.float32))
    return out


def mixed_faces(seed, want, cols=448, rows=448):
    """`want` candidates: places that hold one to six faces around one spot, every fifth place a chain (A-B and B-C overlap, A-C do
    not), scores from 31 values so that ties abound"""
    rng = np.random.default_rng(seed)
    score = lambda: np.float32(0.5) + np.float32(rng.integers(1, 32)) / np.float32(64)  # noqa: E731
    per_row = max(1, (cols - 60) // 70)
    faces, j = [], 0
    while len(faces) < want:
        x, y = 10.0 + 70 * (j % per_row), 10.0 + 60 * (j // per_row)
        if j % 5 == 4:
            group = [quarter(face(x + 15 * t, y, 40, 40, score())) for t in range(3)]
        else:
            group = [quarter(face(x + float(rng.uniform(-4, 4)), y + float(rng.uniform(-4, 4)), 40, 44, score())) for _ in range(int(rng.integers(1, 7)))]
        faces += group[:want - len(faces)]
        j += 1
    return faces


def check_host(passes, rows=448, cols=448, thr=NMS, md=MD, net=NET, **kw):
    """rf_rot_merge_host against rot_ref.merge, byte for byte, the orientation outputs included; returns the reference tuple"""
    rots, vote, mf = kw.get("rots", 0), kw.get("vote", False), kw.get("max_faces", 0)
    limit = min(mf or md, kw["cap"] if kw.get("cap") is not None else md)
    want = rr.merge(rows, cols, passes, *net, thr, md, vote, mf, rots, cap=limit)
    faces, count, votes, src, truncated, frame_rot, score = rot_merge_host(passes, rows, cols, *net, thr, md, **kw)
    assert count == want[1]
    assert faces.tobytes() == want[0][:limit].tobytes()
    assert list(votes) == list(want[2][:limit]) and list(src) == list(want[3][:limit])
    assert truncated == (count > limit or any(len(p) > md for p in passes))
    assert frame_rot == want[5] and score.tobytes() == want[6].tobytes()
    return want


def test_merge_of_zero_one_and_two_candidates():
    a = quarter(face(100, 100, 40, 40, 0.9))
    none = np.zeros((0, 15), np.float32)
    want = check_host([none] * 4)
    assert want[1] == 0 and want[5] == -1 and not want[6].any()
    for k in range(4):
        passes = [none] * 4
        passes[k] = rr.unmap_face(a, k, 448, 448)[None]
        want = check_host(passes)
        assert want[1] == 1 and want[0].tobytes() == a[None].tobytes() and list(want[3]) == [k] and want[5] == k
        assert want[6][k] == a[0] and want[6].sum() == a[0]
    b = quarter(face(102, 101, 40, 40, 0.8))
    passes = [a[None], none, none, rr.unmap_face(b, 3, 448, 448)[None]]
    want = check_host(passes)                                   # vote off, the default: the head keeps its bytes
    assert want[1] == 1 and list(want[2]) == [2] and want[0][0].tobytes() == a.tobytes()
    want = check_host(passes, vote=True)
    assert want[1] == 1 and a[1] < want[0][0][1] < b[1]
    # the default spec is vote off and all four rotations
    lib = _lib.load_library()
    flat = np.zeros((4, MD, 15), np.float32)
    flat[0, 0], flat[3, 0] = passes[0][0], passes[3][0]
    out, count = (_lib.rf_face * MD)(), C.c_int()
    assert lib.rf_rot_merge_host(None, 448, 448, 448, 448, NMS, MD, flat.ctypes.data_as(C.POINTER(_lib.rf_face)), (C.c_int * 4)(1, 0, 0, 1), out, MD,
                                 C.byref(count), None, None, None, None) == 0
    assert count.value == 1 and bytes(out[0])[:60] == a.tobytes()


def test_chains_ties_and_the_rotation_as_tie_break():
    a, b, c = (quarter(face(100 + 15 * j, 100, 40, 40, 0.9 - 0.1 * j)) for j in range(3))
    none = np.zeros((0, 15), np.float32)
    un = lambda f, k: rr.unmap_face(f, k, 448, 448)  # noqa: E731
    want = check_host([np.stack([a, c]), un(b, 1)[None], none, none], vote=True)
    assert want[1] == 2 and list(want[2]) == [2, 1] and want[0][1].tobytes() == c.tobytes()          # B joins A, C is its own head
    # equal scores across the passes: g decides, so the LOWER rotation heads the cluster whichever box is which
    for first, second in ((a, b), (b, a)):
        x, y = first.copy(), second.copy()
        x[0] = y[0] = np.float32(0.75)
        want = check_host([none, none, un(x, 2)[None], un(y, 3)[None]])
        assert want[1] == 1 and list(want[3]) == [2] and list(want[2]) == [2] and want[5] == 2
    # g is k * max_detections + j with k the ROTATION, not the ordinal of the pass: with rots = 8 the one pass is rotation 3
    want = check_host([un(a, 3)[None]], rots=8)
    assert list(want[3]) == [3] and want[5] == 3 and want[0][0].tobytes() == a.tobytes()


@pytest.mark.parametrize("rots", (15, 5, 8, 1))
@pytest.mark.parametrize("vote", (False, True))
def test_merge_equals_the_reference_on_dealt_faces(rots, vote):
    faces = mixed_faces(7 + rots, 180)
    passes = deal(faces, 448, 448, rots)
    want = check_host(passes, rots=rots, vote=vote)
    assert 0 < want[1] < 180 and want[2].max() >= 3 and (want[2] == 1).any() and set(want[3].tolist()) <= set(rr.rot_list(rots))
    if rots == 15:
        assert set(want[3].tolist()) == {0, 1, 2, 3}
    # max_faces and cap cut the list (and the orientation sums with it); the count stays true and the call says so
    check_host(passes, rots=rots, vote=vote, max_faces=7)
    check_host(passes, rots=rots, vote=vote, cap=5)
    check_host(passes, rots=rots, vote=vote, max_faces=9, cap=3)
    check_host(passes, rots=rots, vote=vote, cap=0)
    # a pass count above max_detections is clamped and reported
    check_host(passes, rots=rots, vote=vote, md=16)
    assert rot_merge_host(passes, 448, 448, *NET, NMS, 16, rots=rots)[4]


def test_merge_of_frames_of_other_shapes():
    # a 300 x 211 frame: c and r differ, the odd passes are 211 x 300
    faces = mixed_faces(31, 60, cols=211, rows=300)
    for vote in (False, True):
        want = check_host(deal(faces, 300, 211), rows=300, cols=211, vote=vote)
        assert 0 < want[1] < 60 and len(set(want[3].tolist())) >= 3
    # a 896 x 1280 frame at the 448 net: every pass is shrunk, all by the same scale
    faces = mixed_faces(32, 120, cols=1280, rows=896)
    for vote in (False, True):
        want = check_host(deal(faces, 896, 1280), rows=896, cols=1280, vote=vote)
        assert 0 < want[1] < 120 and want[2].max() >= 3
    # ... and at a 896 x 1280 net: only the odd passes are shrunk
    passes = deal(faces, 896, 1280, net=WIDE)
    want = check_host(passes, rows=896, cols=1280, net=WIDE, vote=True)
    assert 0 < want[1] < 120 and want[2].max() >= 3


def test_orientation_sums_ties_and_empty_frames():
    none = np.zeros((0, 15), np.float32)
    spots = [quarter(face(20 + 90 * j, 30, 40, 40, 0.75)) for j in range(4)]
    un = lambda f, k: rr.unmap_face(f, k, 448, 448)  # noqa: E731
    # one head per rotation, equal scores: a four-way tie goes to the lowest k present
    want = check_host([un(spots[k], k)[None] for k in range(4)])
    assert want[1] == 4 and want[5] == 0 and list(want[6]) == [np.float32(0.75)] * 4
    want = check_host([none, un(spots[1], 1)[None], none, un(spots[3], 3)[None]])
    assert want[5] == 1
    # two weaker heads outweigh one stronger head
    lo = [quarter(face(20 + 90 * j, 200, 40, 40, 0.625)) for j in range(2)]
    hi = quarter(face(300, 300, 40, 40, 0.9375))
    want = check_host([hi[None], none, np.stack([un(f, 2) for f in lo]), none])
    assert want[5] == 2 and want[6][2] == np.float32(1.25) and want[6][0] == np.float32(0.9375)
    # ... unless the cut leaves only the strongest: the outputs describe the EMITTED heads
    want = check_host([hi[None], none, np.stack([un(f, 2) for f in lo]), none], max_faces=1)
    assert want[5] == 0 and want[6][2] == 0
    assert check_host([none] * 4)[5] == -1
    assert check_host([hi[None], none, none, none], cap=0)[5] == -1


def test_merge_refusals():
    lib = _lib.load_library()
    faces = (_lib.rf_face * (4 * MD))()
    pc = (C.c_int * 4)(0, 0, 0, 0)
    out = (_lib.rf_face * MD)()
    count = C.c_int(-7)

    def call(sp, rows=448, cols=448, nh=448, nw=448, md=MD, faces=faces, pc=pc, out=out, cap=MD, count=C.byref(count)):
        return lib.rf_rot_merge_host(sp, rows, cols, nh, nw, 0.4, md, faces, pc, out, cap, count, None, None, None, None)
    assert call(None) == 0 and count.value == 0
    assert call(C.byref(rot_spec())) == 0 and call(C.byref(rot_spec(rots=15, vote=True, max_faces=4096))) == 0
    for field, value in (("struct_size", 12), ("struct_size", 20), ("rots", 16), ("rots", -1), ("vote", 3), ("vote", -1), ("max_faces", 4097),
                         ("max_faces", -1)):
        sp = rot_spec()
        setattr(sp, field, value)
        count.value = -7
        assert call(C.byref(sp)) == _lib.RF_ERR_INVALID_ARG and count.value == -7, (field, value)
    for kw in (dict(md=0), dict(md=4097), dict(nh=0), dict(rows=-1), dict(rows=4097, cols=3072), dict(faces=None), dict(pc=None), dict(count=None),
               dict(cap=-1), dict(out=None), dict(pc=(C.c_int * 4)(0, 0, 0, -1))):
        assert call(None, **kw) == _lib.RF_ERR_INVALID_ARG, kw
    assert call(None, out=None, cap=0) == 0
    with pytest.raises(_lib.RFError):
        rot_merge_host([np.zeros((0, 15), np.float32)] * 2, 448, 448, *NET, NMS, MD)             # all four rotations want four passes
    assert C.sizeof(_lib.rf_rot_spec) == 16


# ---------------------------------------------------------------------------------------------- end to end through the CPU oracle
def test_a_window_turned_four_ways_through_the_oracle(oracles, base_frame):
    """The claim: mnet25, 448 net, threshold 0.6, the window (0, 832) of the base frame turned by kf = 0..3 quarter turns.  The plain
    pass finds 2, 1, 1, 0 faces; the merge of four passes finds both faces in every frame, from the pass that turns the frame upright."""
    oracle = oracles["mnet25"]
    window = np.ascontiguousarray(base_frame[0:448, 832:1280])
    plain_total = merged_total = 0
    upright = None
    for kf in range(4):
        frame = rr.rotate(window, kf)
        passes = [oracle.detect(rr.rotate(frame, k), 0.6, NMS, net_hw=NET).rows() for k in range(4)]
        plain_total += len(passes[0])
        want = check_host(passes)
        up = (4 - kf) % 4
        assert want[1] == 2 and list(want[3]) == [up, up] and want[5] == up, (kf, want[1], want[3], want[5])
        merged_total += want[1]
        # the faces are the upright frame's faces, moved into this frame
        if kf == 0:
            upright = want[0]
        else:
            back = np.stack([rr.map_face(f, up, 448, 448, *NET) for f in passes[up]])
            assert want[0].tobytes() == back.tobytes()
            turned = np.stack([rr.unmap_face(f, kf, 448, 448) for f in upright])      # where the upright faces are in this frame
            for f in want[0]:
                assert max(rr.tta_ref.iou_plus1(f[1:5], t[1:5]) for t in turned) >= 0.9
    assert merged_total == 8 > plain_total


# ---------------------------------------------------------------------------------------------- the sanitizer program
def test_rotate_and_map_under_address_and_ub_sanitizers(tmp_path):
    """tests/csrc/test_rot_host.cpp: rot_rotate_host on the edge shapes in exactly-sized heap buffers and rot_map_face round trips, host
    code only, built with -fsanitize=address,undefined.  No GPU and no library: rot.h is compiled into the program."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")                        # for <hip/hip_runtime.h>, which rot.h includes
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "test_rot_host")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "test_rot_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
