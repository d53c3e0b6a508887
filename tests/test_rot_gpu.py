"""Rotation-robust detection on the GPU: the rotate kernel against np.rot90, the gather and merge kernels against tests/rot_ref.py byte
for byte on constructed faces (no forward pass), the fused call against its own parts (ONE rf_detect_batch_device call over
[f0, rot1(f0), rot2(f0), rot3(f0), f1, ...] + the reference merge), the claim (a window turned four ways), the refusals, and the C++ class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rot_ref as rr
from conftest import ASSETS, ROOT
from test_gpu_align import FP16, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_rot_host import deal, mixed_faces
from test_tta_gpu import BIG, INT8, MD, NET, NMS, SPLIT2, SPLIT3, WINDOWS, big_engine, odd_view
from test_tta_host import face, quarter

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- 1. the rotate kernel
# the tile edge (64) and its neighbours, widths that are no multiple of 4, degenerate axes, more than one tile per axis
PAIRS = ((1, 129), (129, 1), (63, 65), (65, 63), (64, 64), (1, 1), (2, 3), (3, 2), (5, 5), (5, 64), (64, 5), (63, 63), (65, 65), (129, 129),
         (2, 129), (129, 3), (64, 65), (65, 64), (63, 129), (129, 64), (3, 63))


@pytest.mark.parametrize("k", (0, 1, 2, 3))
def test_rotate_device_equals_rot90(rfa, k):
    import torch
    det = engine(rfa)
    rng = np.random.default_rng(k)
    for rows, cols in PAIRS:
        frame = rng.integers(0, 256, size=(rows, cols, 3), dtype=np.uint8)
        want = np.rot90(frame, k)
        dr, dc = want.shape[:2]
        dense = to_device([frame])[0]
        keep, rptr, rstep = odd_view(frame)
        for sptr, sstep in ((dense.data_ptr(), 3 * cols), (rptr, rstep)):
            for pad, shift in ((0, 0), (7, 1)):                      # a dense destination; a pitched one at an odd pointer
                dstep = 3 * dc + pad
                dst = torch.full((dr * dstep + 8,), 0xAB, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                det.rotate_device(sptr, rows, cols, k, dst.data_ptr() + shift, step=sstep, dst_step=dstep)
                got = dst.cpu().numpy()
                body = got[shift:shift + dr * dstep].reshape(dr, dstep)
                assert np.array_equal(body[:, :3 * dc].reshape(dr, dc, 3), want), (rows, cols, k, pad, shift)
                assert (body[:, 3 * dc:] == 0xAB).all() and (got[:shift] == 0xAB).all() and (got[shift + dr * dstep:] == 0xAB).all()


def test_rotate_device_of_a_whole_frame_and_refusals(rfa, base_frame):
    import torch
    det = engine(rfa)
    dev = to_device([base_frame])[0]
    dst = torch.zeros_like(dev).view(-1)
    for k in range(4):
        det.rotate_device(dev.data_ptr(), 896, 1280, k, dst.data_ptr())
        assert np.array_equal(dst.cpu().numpy().reshape(np.rot90(base_frame, k).shape), np.rot90(base_frame, k)), k
        # a window of it as a pitched view: many workgroups, an unaligned source
        det.rotate_device(dev.data_ptr() + 30 * 3840 + 3 * 441, 300, 449, k, dst.data_ptr(), step=3840)
        want = np.rot90(base_frame[30:330, 441:890], k)
        assert np.array_equal(dst.cpu().numpy()[:300 * 449 * 3].reshape(want.shape), want), k
    for bad in (dict(k=1, dst_step=3 * 896 - 1), dict(k=2, dst_step=3 * 1280 - 1), dict(k=1, step=3 * 1280 - 1), dict(k=4), dict(k=-1)):
        with pytest.raises(rfa.RFError) as e:
            det.rotate_device(dev.data_ptr(), 896, 1280, bad.pop("k"), dst.data_ptr(), **bad)
        assert e.value.status == -1
    with pytest.raises(rfa.RFError):
        det.rotate_device(dev.data_ptr(), 896, 1280, 1, 0)


# ---------------------------------------------------------------------------------------------- 2. merge with constructed faces
def check_merge_call(det, frames, md=BIG, **kw):
    """frames: (rows, cols, passes); one rf_rot_merge_device call against rot_ref per frame, byte for byte, votes, rotations and the
    orientation outputs included"""
    rows, cols = [f[0] for f in frames], [f[1] for f in frames]
    dets, votes, src = det.rot_merge(rows, cols, [f[2] for f in frames], return_votes=True, **kw)
    counts = list(det.rot_counts)
    limit = min(kw.get("max_faces", 0) or md, kw.get("cap_per_image", md))
    assert det.truncated == any(c > limit for c in counts)
    for i, (r, c, passes) in enumerate(frames):
        want = rr.merge(r, c, passes, NET, NET, NMS, md, kw.get("vote", False), kw.get("max_faces", 0), kw.get("rots", 0), cap=limit)
        faces = want[0][:limit]
        assert counts[i] == want[1], (i, counts[i], want[1], want[4])
        assert rows_of(dets[i]).tobytes() == faces.tobytes(), (i, want[4])
        assert list(votes[i]) == list(want[2][:limit]) and list(src[i]) == list(want[3][:limit]), i
        assert det.frame_rot[i] == want[5] and det.rot_score[i].tobytes() == want[6].tobytes(), i
    return dets, votes, src, counts


def test_merge_of_constructed_faces_equals_the_reference(rfa):
    det = big_engine(rfa)
    assert det.max_detections == BIG
    made = {}

    def frame(want, seed, shape=(448, 448), rots=15):
        key = (want, seed, shape, rots)
        if key not in made:
            made[key] = shape + (deal(mixed_faces(seed, want, shape[1], shape[0]), shape[0], shape[1], rots, md=BIG),)
        return made[key]
    # the three sort regimes and their boundaries, three frames per call, frames of other sizes (a scale above 1 among them)
    calls = ([frame(0, 1), frame(1, 2), frame(64, 3, (300, 211)), frame(257, 5, (896, 1280))],
             [frame(65, 4), frame(1000, 6)])
    heads = []
    for frames in calls:
        for vote in (False, True):
            dets, votes, src, counts = check_merge_call(det, frames, vote=vote)
        heads += counts
        again = det.rot_merge([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], vote=True, return_votes=True)
        assert again[0] == dets and all(np.array_equal(a, b) for a, b in zip(again[1], votes))      # the counters re-armed, no order leaks
    assert heads[0] == 0 and heads[1] == 1 and all(0 < k < w for k, w in zip(heads[2:], (64, 257, 65, 1000)))
    want = rr.merge(*frame(1000, 6)[:2], frame(1000, 6)[2], NET, NET, NMS, BIG, True)
    assert want[2].max() >= 5 and (want[2] == 1).any() and set(want[3].tolist()) == {0, 1, 2, 3}
    # subsets of the rotations: two passes per frame, one pass per frame (rotation 3: g says so)
    for rots in (5, 8):
        for vote in (False, True):
            dets, votes, src, counts = check_merge_call(det, [frame(257, 7, rots=rots), frame(64, 8, (300, 211), rots=rots)], rots=rots, vote=vote)
        assert {int(s) for v in src for s in v} == set(rr.rot_list(rots))
    # a smaller max_faces and a smaller cap_per_image: counts stay true, the orientation outputs describe what was emitted
    check_merge_call(det, [frame(257, 5, (896, 1280)), frame(1000, 6)], max_faces=7)
    assert det.truncated
    check_merge_call(det, [frame(65, 4)], cap_per_image=5)
    assert det.truncated and det.rot_counts[0] > 5


def test_merge_overflow_is_reported_and_leaves_the_other_frame_exact(rfa):
    det = big_engine(rfa)
    rng = np.random.default_rng(9)
    grid = [quarter(face(3.0 + 10 * (j % 64) + 0.0, 3.0 + 10 * (j // 64), 5.5, 6.25, np.float32(0.5) + np.float32(rng.integers(1, 32)) / np.float32(64)))
            for j in range(4500)]
    big = (800, 800, deal(grid, 800, 800, md=BIG))
    assert sum(len(p) for p in big[2]) == 4500 > rr.tta_ref.MERGE_CAP
    other = (448, 448, deal(mixed_faces(11, 300), 448, 448, md=BIG))
    want = rr.merge(*other[:2], other[2], NET, NET, NMS, BIG)
    for order in ((0, 1), (1, 0)):
        frames = [[big, other][k] for k in order]
        dets, votes, src = det.rot_merge([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], return_votes=True)
        assert det.truncated
        i = order.index(1)
        assert det.rot_counts[i] == want[1] and rows_of(dets[i]).tobytes() == want[0].tobytes()
        assert list(votes[i]) == list(want[2]) and list(src[i]) == list(want[3]) and det.frame_rot[i] == want[5]
    check_merge_call(det, [other])                         # the counters were re-armed: the next call is exact


# ---------------------------------------------------------------------------------------------- 3. fused call against its own parts
@pytest.fixture(scope="module")
def turned(base_frame):
    """the six windows, each turned by another number of quarter turns"""
    return [rr.rotate(base_frame[y:y + 448, x:x + 448], i % 4) for i, (y, x) in enumerate(WINDOWS)]


def parts_of_call(det, frames, thr=0.5, rots=0, md=MD, **kw):
    """frames: (ptr, rows, cols, step, pixels) of one rotation call (ptr 0: an empty frame).  rot_ref.merge, per frame, over what ONE
    rf_detect_batch_device call returns for [f0, rot1(f0), rot2(f0), rot3(f0), f1, ...] -- the call the engine itself makes; the
    rotations are made with numpy and uploaded densely.  One call, because the last bits of an image's result can depend on what
    shares its launch."""
    ks = rr.rot_list(rots)
    copies = to_device([rr.rotate(f[4], k) for f in frames if f[0] for k in ks if k])
    ptrs, rows, cols, steps, at = [], [], [], [], 0
    for ptr, r, c, st, _ in frames:
        for k in ks:
            if not ptr:
                ptrs.append(0); rows.append(0); cols.append(0); steps.append(0)
            elif k == 0:
                ptrs.append(ptr); rows.append(r); cols.append(c); steps.append(st)
            else:
                pr, pc = rr.pass_shape(k, r, c)
                ptrs.append(copies[at].data_ptr()); rows.append(pr); cols.append(pc); steps.append(3 * pc)
                at += 1
    res = det.detect_device(ptrs, rows, cols, thr, steps=steps)
    assert not det.truncated
    out = []
    for i, (ptr, r, c, _, _) in enumerate(frames):
        passes = [rows_of(x) for x in res[len(ks) * i:len(ks) * (i + 1)]]
        out.append((rr.merge(r, c, passes, det.net_h, det.net_w, NMS, md, kw.get("vote", False), kw.get("max_faces", 0), rots) if ptr else None, passes))
    return out


def check_rot(det, got, votes, src, i, want):
    if want is None:
        assert got[i] == [] and det.rot_counts[i] == 0 and det.frame_rot[i] == -1 and not det.rot_score[i].any()
        return
    assert det.rot_counts[i] == want[1] and rows_of(got[i]).tobytes() == want[0].tobytes(), (i, det.rot_counts[i], want[1])
    assert list(votes[i]) == list(want[2]) and list(src[i]) == list(want[3]), i
    assert det.frame_rot[i] == want[5] and det.rot_score[i].tobytes() == want[6].tobytes(), i


def run_and_check(det, frames, thr=0.5, **kw):
    want = parts_of_call(det, frames, thr, **kw)
    got, votes, src = det.detect_rotated_device([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], thr,
                                                steps=[f[3] for f in frames], return_votes=True, **kw)
    assert not det.truncated
    for i in range(len(frames)):
        check_rot(det, got, votes, src, i, want[i][0])
    return got, votes, src, want


@pytest.mark.parametrize("prec,kw", ((FP16, {}), (FP16, SPLIT2), (FP16, SPLIT3), (INT8, {})))
def test_fused_call_equals_the_merge_of_its_own_passes(rfa, turned, base_frame, prec, kw):
    """kw = {}: the whole call is one coalesced launch.  SPLIT2 / SPLIT3: the 24 passes of six frames cross launches and lanes -- the
    merge waits for the other lanes' gathers on the device, and every lane waits for the rotate kernel."""
    det = engine(rfa, prec=prec, **kw)
    if kw:
        assert det.max_batch == 8 and det.num_slots() == kw["lanes"]
    dev = to_device(turned)
    frames = [(d.data_ptr(), 448, 448, 3 * 448, w) for d, w in zip(dev, turned)]
    ptrs = [f[0] for f in frames]
    plain = det.detect_device(ptrs, [448] * 6, [448] * 6, 0.5)
    got, votes, src, want = run_and_check(det, frames)
    assert sum(len(g) for g in got) >= 6 and len({int(s) for v in src for s in v}) >= 3        # heads came from several rotations
    # the first frame alone: four passes, one launch
    first = run_and_check(det, frames[:1])[0]
    # repeats give identical bytes
    for _ in range(2):
        again = det.detect_rotated_device(ptrs, [448] * 6, [448] * 6, 0.5, return_votes=True)
        assert again[0] == got and all(np.array_equal(a, b) for a, b in zip(again[2], src))
    # vote on, a subset of the rotations, a smaller max_faces, an empty frame in the middle of the batch
    run_and_check(det, frames[:3], vote=True)
    run_and_check(det, frames[:4], rots=5)
    run_and_check(det, frames[:2] + [(0, 0, 0, 0, None)] + frames[2:4])
    cut = det.detect_rotated_device([frames[0][0]], [448], [448], 0.5, max_faces=1)
    assert det.truncated and det.rot_counts == [len(first[0])] and cut[0] == first[0][:1] and len(first[0]) > 1
    # a frame whose odd passes have another shape: 300 x 448, its passes 1 and 3 are 448 x 300
    strip = np.ascontiguousarray(turned[0][40:340])
    sdev = to_device([strip])[0]
    run_and_check(det, [(sdev.data_ptr(), 300, 448, 3 * 448, strip), frames[1]])
    # rots = 1, vote off: rf_detect_batch_device times the scale (1 here), byte for byte; the ordinary call is what it was
    assert det.detect_device(ptrs, [448] * 6, [448] * 6, 0.5) == plain
    off, voff, soff = det.detect_rotated_device(ptrs, [448] * 6, [448] * 6, 0.5, rots=1, return_votes=True)
    assert [rows_of(o).tobytes() for o in off] == [rows_of(p).tobytes() for p in plain] and det.rot_counts == [len(p) for p in plain]
    assert all((v == 1).all() and not s.any() for v, s in zip(voff, soff))
    tta = det.detect_tta_device(ptrs, [448] * 6, [448] * 6, 0.5, flip=False, vote=False)
    assert tta == off
    if prec != FP16:
        return
    # an oversize frame (every pass shrunk, the odd ones 1280 x 896) with frames that fit, in one call
    big = to_device([base_frame])[0]
    gb, vb, sb, wb = run_and_check(det, [(big.data_ptr(), 896, 1280, 3 * 1280, base_frame)] + frames[:2])
    assert len(gb[0]) >= 4 and max(d.rect[2] for d in gb[0]) > 448
    # pitched and ROI device frames: an odd pointer and an odd step; a window of the big frame as a view
    keep, rptr, rstep = odd_view(turned[0])
    win = np.ascontiguousarray(base_frame[30:478, 440:888])
    run_and_check(det, [(rptr, 448, 448, rstep, turned[0]), (big.data_ptr() + 30 * 3840 + 3 * 440, 448, 448, 3840, win)] + frames[1:3])
    # host frames: uploaded once, densely; an empty frame in between
    hgot, hvotes, hsrc = det.detect_rotated([turned[0], None, turned[1]], 0.5, return_votes=True)
    hwant = parts_of_call(det, [frames[0], (0, 0, 0, 0, None), frames[1]])
    for i in range(3):
        check_rot(det, hgot, hvotes, hsrc, i, hwant[i][0])
    assert det.detect_device(ptrs, [448] * 6, [448] * 6, 0.5) == plain


# ---------------------------------------------------------------------------------------------- 4. the claim
def test_a_window_turned_four_ways_is_found_and_its_orientation_told(rfa, base_frame):
    """fp16 mnet25, threshold 0.6, the window (0, 832) turned by kf = 0..3: the rotation call finds both faces in every frame, every head
    from the pass that turns the frame upright; the plain call finds fewer.  The oracle's nearest score to 0.6 is 0.636: a margin of
    0.036, 18 x the suite's SCORE_NOISE of 2e-3."""
    det = engine(rfa)
    frames = [rr.rotate(base_frame[0:448, 832:1280], kf) for kf in range(4)]
    dev = to_device(frames)
    ptrs = [d.data_ptr() for d in dev]
    got, votes, src = det.detect_rotated_device(ptrs, [448] * 4, [448] * 4, 0.6, return_votes=True)
    plain = det.detect_device(ptrs, [448] * 4, [448] * 4, 0.6)
    print("rotation call:", [len(g) for g in got], "src_rot:", [list(s) for s in src], "frame_rot:", det.frame_rot, "plain call:", [len(p) for p in plain])
    for kf in range(4):
        up = (4 - kf) % 4
        assert len(got[kf]) == 2 and list(src[kf]) == [up, up] and det.frame_rot[kf] == up, kf
    assert sum(len(p) for p in plain) < 8


# ---------------------------------------------------------------------------------------------- 5. refusals, multi-device
def rot_calls(det, ptr, spec_kw):
    return (lambda: det.detect_rotated_device([ptr], [448], [448], 0.5, **spec_kw),
            lambda: det.detect_rotated([np.zeros((448, 448, 3), np.uint8)], 0.5, **spec_kw),
            lambda: det.rot_merge([448], [448], [[np.zeros((0, 15), np.float32)] * 4], **spec_kw))


def test_bad_specs_are_refused_and_leave_the_handle_usable(rfa, crop448):
    det = engine(rfa)
    dev = to_device([crop448])[0]
    before = det.detect_rotated_device([dev.data_ptr()], [448], [448], 0.5)
    plain = det.detect_device([dev.data_ptr()], [448], [448], 0.5)
    for bad in (dict(max_faces=4097), dict(max_faces=-1)):
        for call in rot_calls(det, dev.data_ptr(), bad):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1, bad
    cnt, out = (C.c_int * 1)(), (rfa._lib.rf_face * MD)()
    args = (det._h, (C.c_void_p * 1)(dev.data_ptr()), (C.c_int * 1)(448), (C.c_int * 1)(448), (C.c_int * 1)(1344), 1, 0.5)
    tail = (out, MD, cnt, None, None, None, None)
    for field, value in (("struct_size", 12), ("rots", 16), ("rots", -1), ("vote", 3), ("vote", -1)):
        sp = rfa.rot_spec()
        setattr(sp, field, value)
        assert det._lib.rf_detect_rot_batch_device(*args, C.byref(sp), *tail) == -1, field
    assert det._lib.rf_detect_rot_batch_device(*args, None, None, MD, cnt, None, None, None, None) == -1          # out is null
    frame_rot, score = (C.c_int * 1)(-7), (C.c_float * 4)()
    assert det._lib.rf_detect_rot_batch_device(*args, None, out, MD, cnt, None, None, frame_rot, score) == 0      # a NULL spec: the defaults
    assert cnt[0] == len(before[0]) == 2 and frame_rot[0] == 0 and score[0] > 1 and not any(score[1:])           # ... and a NULL src_rot
    assert det.detect_rotated_device([dev.data_ptr()], [448], [448], 0.5) == before
    assert det.detect_device([dev.data_ptr()], [448], [448], 0.5) == plain


def test_multi_device_handles_refuse_rotation(rfa, crop448):
    det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", devices=[0, 0])
    try:
        dev = to_device([crop448])[0]
        for call in rot_calls(det, dev.data_ptr(), {}) + (lambda: det.rotate_device(dev.data_ptr(), 448, 448, 1, dev.data_ptr()),):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -5
        assert len(det.detect_device([dev.data_ptr()], [448], [448], 0.5)[0]) >= 1
    finally:
        det.close()


# ---------------------------------------------------------------------------------------------- 6. the C++ class
def test_cpp_class_detect_rotated(rfa, turned, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_rot.cpp")
    exe = str(tmp_path / "test_rot")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    raw, out = str(tmp_path / "frame.raw"), str(tmp_path / "out.bin")
    turned[1].tofile(raw)
    det = engine(rfa)
    for rots, vote, mf in ((0, 0, 0), (15, 1, 1), (5, 2, 0)):
        r = subprocess.run([exe, ASSETS, "mnet25", "448", "448", raw, "448", "448", "0.5", str(rots), str(vote), str(mf), out],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        blob = open(out, "rb").read()
        n = int(np.frombuffer(blob, np.int32, 1)[0])
        assert n == 3
        want, wv, ws = det.detect_rotated([turned[1], None, turned[1]], 0.5, rots=rots, vote=vote == 1, max_faces=mf, return_votes=True)
        pos = 4
        for i in range(n):
            k = int(np.frombuffer(blob, np.int32, 1, pos)[0])
            faces = np.frombuffer(blob, np.float32, k * 15, pos + 4).reshape(k, 15)
            votes = np.frombuffer(blob, np.int32, k, pos + 4 + 60 * k)
            srcs = np.frombuffer(blob, np.int32, k, pos + 4 + 64 * k)
            frame_rot = int(np.frombuffer(blob, np.int32, 1, pos + 4 + 68 * k)[0])
            score = np.frombuffer(blob, np.float32, 4, pos + 8 + 68 * k)
            pos += 24 + 68 * k
            assert faces.tobytes() == rows_of(want[i]).tobytes() and list(votes) == list(wv[i]) and list(srcs) == list(ws[i]), i
            assert frame_rot == det.frame_rot[i] and score.tobytes() == det.rot_score[i].tobytes(), i
            assert k == (0 if i == 1 else len(want[0])) and (mf == 0 or i == 1 or k == mf)
        assert pos == len(blob)
