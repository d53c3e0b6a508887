"""Flip test-time augmentation on the GPU: the mirror kernel against frame[:, ::-1], the gather and voting merge kernels against
tests/tta_ref.py byte for byte on constructed faces (no forward pass), the fused call against its own parts (ONE rf_detect_batch_device
call over [f0, mirror(f0), f1, ...] + the reference merge), the refusals, and the C++ class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tile_ref
import tta_ref as tr
from conftest import ASSETS, ROOT
from test_face_aa_gpu import roi_view
from test_gpu_align import FP16, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_tta_host import as_passes, face, in_pass1, quarter

pytestmark = pytest.mark.gpu

INT8 = 2
NET = 448
MD = 256                       # max_detections of the cached engines
BIG = 4096                     # ... and of the engine of the merge tests: two passes can then hold 4096 candidates and more
NMS = 0.4
# as in test_tile_gpu.py: with the default options a call is ONE coalesced launch; these engines really split a call into launches of
# at most 8 images over two / three lanes, so a frame's two passes can ride on different launches and streams
SPLIT2 = dict(max_batch=8, coalesce=1, lanes=2)
SPLIT3 = dict(max_batch=8, coalesce=1, lanes=3)


# ---------------------------------------------------------------------------------------------- 1. the mirror kernel
def odd_view(frame):
    """the frame on the device as an ROI of a wider buffer: an odd pointer and an odd step, whatever the width"""
    import torch
    h, w = frame.shape[:2]
    step = w * 3 + 13 + (w % 2)
    dev = to_device([frame])[0]
    wide = torch.zeros((h + 1, step), dtype=torch.uint8, device="cuda")
    wide.view(-1)[1:1 + h * step].view(h, step)[:, :w * 3] = dev.view(h, w * 3)
    torch.cuda.synchronize()
    assert (wide.data_ptr() + 1) % 2 == 1 and step % 2 == 1
    return wide, wide.data_ptr() + 1, step


@pytest.mark.parametrize("rows", (1, 7))
def test_mirror_device_equals_the_flipped_frame(rfa, rows):
    import torch
    det = engine(rfa)
    rng = np.random.default_rng(rows)
    for cols in (1, 2, 3, 5, 21, 63, 64, 65, 447, 449):
        frame = rng.integers(0, 256, size=(rows, cols, 3), dtype=np.uint8)
        want = frame[:, ::-1]
        dense = to_device([frame])[0]
        keep, rptr, rstep = odd_view(frame)
        for sptr, sstep in ((dense.data_ptr(), 3 * cols), (rptr, rstep)):
            for pad, shift in ((0, 0), (5, 0), (7, 1), (2, 3)):          # dense; pitched destinations, some at odd pointers
                dstep = 3 * cols + pad
                dst = torch.full((rows * dstep + 8,), 0xAB, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                det.mirror_device(sptr, rows, cols, dst.data_ptr() + shift, step=sstep, dst_step=dstep)
                got = dst.cpu().numpy()
                body = got[shift:shift + rows * dstep].reshape(rows, dstep)
                assert np.array_equal(body[:, :3 * cols].reshape(rows, cols, 3), want), (cols, pad, shift)
                assert (body[:, 3 * cols:] == 0xAB).all() and (got[:shift] == 0xAB).all() and (got[shift + rows * dstep:] == 0xAB).all()


def test_mirror_device_of_a_whole_frame_and_refusals(rfa, base_frame):
    import torch
    det = engine(rfa)
    dev = to_device([base_frame])[0]
    dst = torch.zeros_like(dev)
    det.mirror_device(dev.data_ptr(), 896, 1280, dst.data_ptr())
    assert np.array_equal(dst.cpu().numpy(), base_frame[:, ::-1])
    # a window of it as a pitched view: many workgroups, an unaligned source
    det.mirror_device(dev.data_ptr() + 30 * 3840 + 3 * 441, 300, 449, dst.data_ptr(), step=3840)
    assert np.array_equal(dst.cpu().numpy().reshape(-1)[:300 * 449 * 3].reshape(300, 449, 3), base_frame[30:330, 441:890][:, ::-1])
    for bad in (dict(dst_step=3 * 1280 - 1), dict(step=3 * 1280 - 1)):
        with pytest.raises(rfa.RFError):
            det.mirror_device(dev.data_ptr(), 896, 1280, dst.data_ptr(), **bad)
    with pytest.raises(rfa.RFError):
        det.mirror_device(dev.data_ptr(), 896, 1280, 0)


# ---------------------------------------------------------------------------------------------- 2. merge with constructed faces
def score31(rng):
    return np.float32(0.5) + np.float32(rng.integers(1, 32)) / np.float32(64)          # 31 distinct scores: ties abound


def deal(faces, cols=448, md=BIG):
    """frame-space faces dealt alternately over the two passes (the second through the inverse mapping), each in score order"""
    p0 = sorted(faces[::2], key=lambda f: -f[0])
    p1 = sorted((in_pass1(f, cols) for f in faces[1::2]), key=lambda f: -f[0])
    assert len(p0) <= md and len(p1) <= md
    return as_passes(p0, p1)


def mixed_frame(seed, want, cols=448):
    """`want` candidates: places that hold one to six faces around one spot, every fifth place a chain (A-B and B-C overlap, A-C do
    not), scores from 31 values"""
    rng = np.random.default_rng(seed)
    faces, j = [], 0
    while len(faces) < want:
        x, y = 10.0 + 70 * (j % 40), 10.0 + 60 * (j // 40)
        if j % 5 == 4:
            group = [quarter(face(x + 15 * k, y, 40, 40, score31(rng))) for k in range(3)]
        else:
            group = [quarter(face(x + float(rng.uniform(-4, 4)), y + float(rng.uniform(-4, 4)), 40, 44, score31(rng))) for _ in range(int(rng.integers(1, 7)))]
        faces += group[:want - len(faces)]
        j += 1
    return deal(faces, cols)


def singletons(count):
    rng = np.random.default_rng(count)
    return deal([quarter(face(3.0 + 10 * (j % 64) + float(rng.integers(0, 4)) / 4, 3.0 + 10 * (j // 64), 5.5, 6.25, score31(rng))) for j in range(count)])


def one_cluster(count):
    rng = np.random.default_rng(count)
    fs = [quarter(face(200 + float(rng.uniform(-3, 3)), 150 + float(rng.uniform(-3, 3)), 60 + float(rng.uniform(-2, 2)), 70, score31(rng))) for _ in range(count)]
    fs[0][0] = np.float32(0.999)
    return deal(fs)


def big_engine(rfa):
    return engine(rfa, max_detections=BIG, max_batch=1, coalesce=1, lanes=1)


def check_merge_call(det, frames, md=BIG, **kw):
    """frames: (rows, cols, passes); one rf_tta_merge_device call against tta_ref per frame, byte for byte, votes and passes included"""
    rows, cols = [f[0] for f in frames], [f[1] for f in frames]
    dets, votes, src = det.tta_merge(rows, cols, [f[2] for f in frames], return_votes=True, **kw)
    counts = list(det.tta_counts)
    limit = min(kw.get("max_faces", 0) or md, kw.get("cap_per_image", md))
    assert det.truncated == any(c > limit for c in counts)
    for i, (r, c, passes) in enumerate(frames):
        want = tr.merge(r, c, passes, NET, NET, NMS, md, kw.get("vote", True), kw.get("max_faces", 0))
        faces = want[0][:limit]
        assert counts[i] == want[1], (i, counts[i], want[1], want[4])
        assert rows_of(dets[i]).tobytes() == faces.tobytes(), (i, want[4])
        assert list(votes[i]) == list(want[2][:limit]) and list(src[i]) == list(want[3][:limit]), i
    return dets, votes, src, counts


def test_merge_of_constructed_faces_equals_the_reference(rfa):
    det = big_engine(rfa)
    assert det.max_detections == BIG
    made = {}

    def frame(want, seed, shape=(448, 448)):
        if (want, seed) not in made:
            made[(want, seed)] = shape + (mixed_frame(seed, want, shape[1]),)
        return made[(want, seed)]
    # the three sort regimes and their boundaries, three frames per call, frames of other sizes (a scale above 1 among them)
    calls = ([frame(0, 1), frame(1, 2), frame(64, 3, (300, 211))],
             [frame(65, 4), frame(256, 5, (896, 1280)), frame(257, 6)],
             [frame(1000, 7), frame(64, 8), frame(4096, 9)])
    heads = []
    for frames in calls:
        dets, votes, src, counts = check_merge_call(det, frames)
        heads += counts
        again = det.tta_merge([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], return_votes=True)
        assert again[0] == dets and all(np.array_equal(a, b) for a, b in zip(again[1], votes))      # the counters re-armed, no order leaks
    assert heads[0] == 0 and heads[1] == 1 and all(0 < k < w for k, w in zip(heads[2:], (64, 65, 256, 257, 1000, 64, 4096)))
    # ties, chains and real clusters occurred
    r, c, passes = frame(1000, 7)
    cand, g = tr.candidates(r, c, passes, NET, NET, BIG)
    want = tr.merge(r, c, passes, NET, NET, NMS, BIG)
    assert len(set(cand[:, 0].tolist())) <= 31 and want[2].max() >= 5 and (want[2] == 1).any() and set(want[3].tolist()) == {0, 1}
    # vote off: the detector's greedy NMS on the same candidates, and the same heads as with vote on
    dets, votes, src, counts = check_merge_call(det, [frame(1000, 7), frame(257, 6)], vote=False)
    keep = tile_ref.nms(cand, g, NMS)
    assert rows_of(dets[0]).tobytes() == cand[keep].tobytes() and list(votes[0]) == list(want[2]) and list(src[0]) == list(want[3])
    # a smaller max_faces and a smaller cap_per_image: counts stay true
    check_merge_call(det, [frame(257, 6), frame(1000, 7)], max_faces=7)
    assert det.truncated
    check_merge_call(det, [frame(65, 4)], cap_per_image=5)
    assert det.truncated and det.tta_counts[0] > 5
    # flip off: one pass per frame
    single = [(448, 448, [frame(257, 6)[2][0]]), (896, 1280, [frame(256, 5)[2][1]])]
    check_merge_call(det, single, flip=False)


def test_merge_of_singletons_and_of_one_large_cluster(rfa):
    det = big_engine(rfa)
    s = (448, 448, singletons(4096))
    dets, votes, src, counts = check_merge_call(det, [s])
    cand, _ = tr.candidates(448, 448, s[2], NET, NET, BIG)
    assert counts == [4096] and (votes[0] == 1).all() and sorted(r.tobytes() for r in rows_of(dets[0])) == sorted(r.tobytes() for r in cand)
    c = (448, 448, one_cluster(1000))
    dets, votes, src, counts = check_merge_call(det, [c, s, c])
    assert counts == [1, 4096, 1] and list(votes[0]) == [1000]


def test_merge_overflow_is_reported_and_leaves_the_other_frame_exact(rfa):
    det = big_engine(rfa)
    rng = np.random.default_rng(9)
    grid = [quarter(face(3.0 + 10 * (j % 64), 3.0 + 10 * (j // 64), 5.5, 6.25, score31(rng))) for j in range(4500)]
    big = (448, 448, deal(grid))
    assert sum(len(p) for p in big[2]) == 4500 > tr.MERGE_CAP
    other = (448, 448, mixed_frame(11, 300))
    want = tr.merge(*other[:2], other[2], NET, NET, NMS, BIG)
    for order in ((0, 1), (1, 0)):
        frames = [[big, other][k] for k in order]
        dets, votes, src = det.tta_merge([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], return_votes=True)
        assert det.truncated
        i = order.index(1)
        assert det.tta_counts[i] == want[1] and rows_of(dets[i]).tobytes() == want[0].tobytes()
        assert list(votes[i]) == list(want[2]) and list(src[i]) == list(want[3])
    check_merge_call(det, [other])                         # the counters were re-armed: the next call is exact


# ---------------------------------------------------------------------------------------------- 3. fused call against its own parts
WINDOWS = ((30, 440), (30, 0), (400, 800), (200, 300), (448, 100), (0, 832))


@pytest.fixture(scope="module")
def windows(base_frame):
    return [np.ascontiguousarray(base_frame[y:y + 448, x:x + 448]) for y, x in WINDOWS]


def parts_of_call(det, frames, thr=0.5, flip=True, md=MD, **kw):
    """frames: (ptr, rows, cols, step, pixels) of one TTA call (ptr 0: an empty frame).  tta_ref.merge, per frame, over what ONE
    rf_detect_batch_device call returns for [f0, mirror(f0), f1, ...] -- the call the engine itself makes; the mirrors are made on the
    host and uploaded densely.  One call, because the last bits of an image's result can depend on what shares its launch."""
    mirrors = to_device([tr.mirror(f[4]) for f in frames if f[0]])
    ptrs, rows, cols, steps, at = [], [], [], [], 0
    for ptr, r, c, st, _ in frames:
        ptrs.append(ptr); rows.append(r if ptr else 0); cols.append(c if ptr else 0); steps.append(st if ptr else 0)
        if flip:
            ptrs.append(mirrors[at].data_ptr() if ptr else 0); rows.append(rows[-1]); cols.append(cols[-1]); steps.append(3 * cols[-1])
        at += 1 if ptr else 0
    res = det.detect_device(ptrs, rows, cols, thr, steps=steps)
    assert not det.truncated
    per = 2 if flip else 1
    out = []
    for i, (ptr, r, c, _, _) in enumerate(frames):
        passes = [rows_of(x) for x in res[per * i:per * i + per]]
        out.append((tr.merge(r, c, passes, det.net_h, det.net_w, NMS, md, kw.get("vote", True), kw.get("max_faces", 0)) if ptr else None, passes))
    return out


def check_tta(got, votes, src, counts, i, want):
    if want is None:
        assert got[i] == [] and counts[i] == 0
        return
    assert counts[i] == want[1] and rows_of(got[i]).tobytes() == want[0].tobytes(), (i, counts[i], want[1])
    assert list(votes[i]) == list(want[2]) and list(src[i]) == list(want[3]), i


def run_and_check(det, frames, **kw):
    want = parts_of_call(det, frames, **kw)
    got, votes, src = det.detect_tta_device([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], 0.5,
                                            steps=[f[3] for f in frames], return_votes=True, **kw)
    assert not det.truncated
    for i in range(len(frames)):
        check_tta(got, votes, src, det.tta_counts, i, want[i][0])
    return got, votes, src, want


@pytest.mark.parametrize("prec,kw", ((FP16, {}), (FP16, SPLIT2), (FP16, SPLIT3), (INT8, {})))
def test_fused_call_equals_the_merge_of_its_own_passes(rfa, windows, base_frame, prec, kw):
    """kw = {}: the whole call is one coalesced launch.  SPLIT2 / SPLIT3: the 12 passes of six frames cross launches and lanes -- the
    merge waits for the other lanes' gathers on the device, and every lane waits for the mirror kernels."""
    det = engine(rfa, prec=prec, **kw)
    if kw:
        assert det.max_batch == 8 and det.num_slots() == kw["lanes"]
    dev = to_device(windows)
    frames = [(d.data_ptr(), 448, 448, 3 * 448, w) for d, w in zip(dev, windows)]
    plain = det.detect_device([f[0] for f in frames], [448] * 6, [448] * 6, 0.5)
    got, votes, src, want = run_and_check(det, frames)
    assert sum(len(g) for g in got) >= 6 and max(int(v.max()) for v in votes if len(v)) == 2
    # the first frame alone: two passes, one launch
    first = run_and_check(det, frames[:1])[0]
    # repeats give identical bytes
    for _ in range(2):
        again = det.detect_tta_device([f[0] for f in frames], [448] * 6, [448] * 6, 0.5, return_votes=True)
        assert again[0] == got and all(np.array_equal(a, b) for a, b in zip(again[1], votes))
    # vote off, a smaller max_faces, an empty frame in the batch
    off3 = run_and_check(det, frames[:3], vote=False)[0]
    assert off3 != got[:3] and [[d.score for d in o] for o in off3] == [[d.score for d in g] for g in got[:3]]        # voting moved boxes, not heads
    run_and_check(det, frames[:2] + [(0, 0, 0, 0, None)] + frames[2:4])
    cut = det.detect_tta_device([frames[0][0]], [448], [448], 0.5, max_faces=1)
    assert det.truncated and det.tta_counts == [len(first[0])] and cut[0] == first[0][:1] and len(first[0]) > 1
    # flip off: rf_detect_batch_device times the scale (1 here), byte for byte
    assert det.detect_device([f[0] for f in frames], [448] * 6, [448] * 6, 0.5) == plain       # the ordinary call is what it was
    off, voff, soff = det.detect_tta_device([f[0] for f in frames], [448] * 6, [448] * 6, 0.5, flip=False, return_votes=True)
    assert [rows_of(o).tobytes() for o in off] == [rows_of(p).tobytes() for p in plain] and det.tta_counts == [len(p) for p in plain]
    assert all((v == 1).all() and not s.any() for v, s in zip(voff, soff))
    if prec != FP16:
        return
    # an oversize frame (shrunk in both passes) with frames that fit, in one call
    big = to_device([base_frame])[0]
    mixed = [(big.data_ptr(), 896, 1280, 3 * 1280, base_frame)] + frames[:2]
    gb, vb, sb, wb = run_and_check(det, mixed)
    assert len(gb[0]) >= 4 and int(vb[0].max()) == 2 and max(d.rect[2] for d in gb[0]) > 448
    off = det.detect_tta_device([big.data_ptr()], [896], [1280], 0.5, flip=False)
    scaled = rows_of(det.detect_device([big.data_ptr()], [896], [1280], 0.5)[0])
    scaled[:, 1:] = scaled[:, 1:] * tr.frame_scale(896, 1280, NET, NET)
    assert rows_of(off[0]).tobytes() == scaled.tobytes()
    # pitched and ROI device frames: an odd pointer and an odd step; a window of the big frame as a view
    keep, rptr, rstep = roi_view(windows[0])
    run_and_check(det, [(rptr, 448, 448, rstep, windows[0]), (big.data_ptr() + 30 * 3840 + 3 * 440, 448, 448, 3840, windows[0])] + frames[1:3])
    # host frames: uploaded once, densely; an empty frame in between
    hgot, hvotes, hsrc = det.detect_tta([windows[0], None, windows[1]], 0.5, return_votes=True)
    hwant = parts_of_call(det, [frames[0], (0, 0, 0, 0, None), frames[1]])
    for i in range(3):
        check_tta(hgot, hvotes, hsrc, det.tta_counts, i, hwant[i][0])
    assert det.detect_device([f[0] for f in frames], [448] * 6, [448] * 6, 0.5) == plain


# ---------------------------------------------------------------------------------------------- 4. refusals
def tta_calls(det, ptr, spec_kw):
    return (lambda: det.detect_tta_device([ptr], [448], [448], 0.5, **spec_kw),
            lambda: det.detect_tta([np.zeros((448, 448, 3), np.uint8)], 0.5, **spec_kw),
            lambda: det.tta_merge([448], [448], [[np.zeros((0, 15), np.float32)] * 2], **spec_kw))


def test_bad_specs_are_refused_and_leave_the_handle_usable(rfa, crop448):
    det = engine(rfa)
    dev = to_device([crop448])[0]
    before = det.detect_tta_device([dev.data_ptr()], [448], [448], 0.5)
    plain = det.detect_device([dev.data_ptr()], [448], [448], 0.5)
    for bad in (dict(max_faces=4097), dict(max_faces=-1)):
        for call in tta_calls(det, dev.data_ptr(), bad):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1, bad
    cnt, out = (C.c_int * 1)(), (rfa._lib.rf_face * MD)()
    args = (det._h, (C.c_void_p * 1)(dev.data_ptr()), (C.c_int * 1)(448), (C.c_int * 1)(448), (C.c_int * 1)(1344), 1, 0.5)
    for field, value in (("struct_size", 12), ("flip", 3), ("vote", -1)):
        sp = rfa.tta_spec()
        setattr(sp, field, value)
        assert det._lib.rf_detect_tta_batch_device(*args, C.byref(sp), out, MD, cnt, None, None) == -1, field
    assert det._lib.rf_detect_tta_batch_device(*args, None, None, MD, cnt, None, None) == -1          # out is null
    assert det._lib.rf_detect_tta_batch_device(*args, None, out, MD, cnt, None, None) == 0 and cnt[0] == len(before[0])       # a NULL spec: the defaults
    assert det.detect_tta_device([dev.data_ptr()], [448], [448], 0.5) == before and len(before[0]) == 2
    assert det.detect_device([dev.data_ptr()], [448], [448], 0.5) == plain


def test_multi_device_handles_refuse_tta(rfa, crop448):
    det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", devices=[0, 0])
    try:
        dev = to_device([crop448])[0]
        for call in tta_calls(det, dev.data_ptr(), {}) + (lambda: det.mirror_device(dev.data_ptr(), 448, 448, dev.data_ptr()),):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -5
        assert len(det.detect_device([dev.data_ptr()], [448], [448], 0.5)[0]) >= 1
    finally:
        det.close()


# ---------------------------------------------------------------------------------------------- 5. the C++ class
def test_cpp_class_detect_tta(rfa, windows, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_tta.cpp")
    exe = str(tmp_path / "test_tta")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    raw, out = str(tmp_path / "frame.raw"), str(tmp_path / "out.bin")
    windows[0].tofile(raw)
    det = engine(rfa)
    for flip, vote, mf in ((1, 1, 0), (0, 2, 1), (2, 0, 0)):
        r = subprocess.run([exe, ASSETS, "mnet25", "448", "448", raw, "448", "448", "0.5", str(flip), str(vote), str(mf), out],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        blob = open(out, "rb").read()
        n = int(np.frombuffer(blob, np.int32, 1)[0])
        assert n == 3
        pos, faces, votes, srcs = 4, [], [], []
        for _ in range(n):
            k = int(np.frombuffer(blob, np.int32, 1, pos)[0])
            faces.append(np.frombuffer(blob, np.float32, k * 15, pos + 4).reshape(k, 15))
            votes.append(np.frombuffer(blob, np.int32, k, pos + 4 + 60 * k))
            srcs.append(np.frombuffer(blob, np.int32, k, pos + 4 + 64 * k))
            pos += 4 + 68 * k
        assert pos == len(blob)
        want, wv, ws = det.detect_tta([windows[0], None, windows[0]], 0.5, flip=flip != 2, vote=vote != 2, max_faces=mf, return_votes=True)
        assert len(faces[0]) == (mf or 2) and len(faces[1]) == 0
        for i in range(n):
            assert faces[i].tobytes() == rows_of(want[i]).tobytes() and list(votes[i]) == list(wv[i]) and list(srcs[i]) == list(ws[i]), i
