"""Tiled detection on the GPU: the gather and merge kernels against tests/tile_ref.py byte for byte on constructed faces (no forward
pass), the fused call against its own parts (rf_detect_batch_device on the ROI views + the reference merge), the fits-the-net
invariant, the 24-face mosaic end to end, the fused face batch against rf_face_batch_gated_device on the tiled result, the refusals,
and the C++ class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tile_ref as tr
from conftest import ASSETS, ROOT, golden
from test_face_aa_gpu import roi_view, same, same_records
from test_gpu_align import FP16, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)

pytestmark = pytest.mark.gpu

INT8 = 2
NET = 448
MD = 256                       # max_detections of the cached engines
NMS = 0.4
OV, EDGE = 128, 8
# With the default options a call of more than max_batch images is coalesced into ONE launch of up to max_batch x coalesce = 256
# images, so every pass of a call rides on one launch of one lane.  These engines really split a call: launches of at most 8 images,
# alternating over two lanes (13 passes = 2 launches, 27 = 4 with both lanes reused after a harvest) or spread over three.
SPLIT2 = dict(max_batch=8, coalesce=1, lanes=2)
SPLIT3 = dict(max_batch=8, coalesce=1, lanes=3)


def split_engine(rfa, kw, **more):
    det = engine(rfa, **more, **kw)
    if kw:
        assert det.max_batch == 8 and det.num_slots() == kw["lanes"]       # coalesce 1: a launch holds at most 8 of the 13 passes
    return det


# ---------------------------------------------------------------------------------------------- 1. merge with constructed faces
def box_face(rng, x1, y1, w, h):
    f = np.zeros(15, np.float32)
    f[0] = np.float32(0.5) + np.float32(rng.integers(1, 32)) / np.float32(64)       # 31 distinct scores: ties across tiles abound
    f[1:5] = (x1, y1, x1 + w, y1 + h)
    f[5:10] = f[1] + np.float32(w) * np.array([0.3, 0.7, 0.5, 0.35, 0.65], np.float32)
    f[10:15] = f[2] + np.float32(h) * np.array([0.4, 0.4, 0.6, 0.8, 0.8], np.float32)
    return f


def constructed_frame(seed, rows, cols, want, full=True):
    """per-pass faces of one frame whose SURVIVING candidates number exactly `want`: faces on every side of every tile (dropped on
    interior sides, kept on frame sides), pairs that two tiles see shifted a little (IoU above the threshold) or a lot (below),
    then faces well inside their tile until the count is reached.  Scores come from 31 values, so equal scores across tiles occur."""
    rng = np.random.default_rng(seed)
    tiles = tr.plan(rows, cols, NET, NET, OV, full)
    T = len(tiles) - (1 if tr.has_full(rows, cols, NET, NET, full) else 0)
    passes = [[] for _ in tiles]

    def survivors():
        return tr.candidates(rows, cols, passes, NET, NET, MD, OV, EDGE, full)[0].shape[0]
    if want >= 64:
        for t in range(T):
            tw, th = int(tiles[t][2]), int(tiles[t][3])
            if tw < 100 or th < 100:
                continue
            for x1, y1, w, h in ((0.0, 50.0, 40.0, 40.0), (3.5, 150.0, 30.0, 30.0), (60.0, 0.0, 40.0, 40.0), (160.0, 7.5, 30.0, 30.0),
                                 (tw - 41.0, 60.0, 40.0, 40.0), (tw - 36.0, 200.0, 30.0, 30.0), (70.0, th - 41.0, 40.0, 40.0),
                                 (170.0, th - 35.5, 30.0, 30.0), (8.0, 8.0, 30.0, 30.0), (tw - 39.0, th - 39.0, 30.0, 30.0)):
                passes[t].append(box_face(rng, x1, y1, w, h))
        if T >= 2 and int(tiles[1][0]) > 0:                        # tiles 0 and 1 overlap in x: the same source box in both
            xa, xb = int(tiles[0][0]), int(tiles[1][0])
            for j, shift in enumerate((1.0, 20.0, 2.5, 26.0)):        # 30-pixel boxes: IoU 0.88, 0.22, 0.73, 0.08
                sx = xb + 12.0 + 34.0 * j
                if sx - xa + 30 > int(tiles[0][2]) - EDGE - 1:
                    break
                a = box_face(rng, sx - xa, 250.0, 30.0, 30.0)
                b = box_face(rng, sx - xb + shift, 250.0, 30.0, 30.0)
                b[0] = a[0] if j % 2 == 0 else b[0]
                passes[0].append(a)
                passes[1].append(b)
        if len(passes) > T:                                        # the full-frame pass: boxes in shrunk coordinates, up to the net's border
            for _ in range(8):
                passes[T].append(box_face(rng, float(rng.integers(0, 300)), float(rng.integers(0, 200)), 20.0, 20.0))
    have = survivors()
    assert have <= want, (have, want)
    t = 0
    while have < want:
        if len(passes[t]) < MD:
            tw, th = int(tiles[t][2]), int(tiles[t][3])
            if t >= T:
                tw, th = 400, 280
            w, h = float(rng.integers(16, 50)), float(rng.integers(16, 50))
            x1 = float(rng.integers(EDGE + 1, max(EDGE + 2, tw - EDGE - 2 - int(w)))) + float(rng.integers(0, 4)) / 4
            y1 = float(rng.integers(EDGE + 1, max(EDGE + 2, th - EDGE - 2 - int(h)))) + float(rng.integers(0, 4)) / 4
            passes[t].append(box_face(rng, x1, y1, w, h))
            have += 1
        t = (t + 1) % len(passes)
    out = []
    for p in passes:
        a = np.stack(p) if p else np.zeros((0, 15), np.float32)
        out.append(a[np.argsort(-a[:, 0], kind="stable")] if len(a) else a)         # a pass's result is in score order
    assert survivors() == want
    return out


def check_merge_call(det, frames, **kw):
    """frames: (rows, cols, passes); one rf_tile_merge_device call against tile_ref per frame, byte for byte"""
    rows, cols = [f[0] for f in frames], [f[1] for f in frames]
    dets, tiles = det.tile_merge(rows, cols, [f[2] for f in frames], overlap=OV, edge=EDGE, return_tiles=True, **kw)
    counts = list(det.tiled_counts)
    limit = min(kw.get("max_faces", 0) or MD, kw.get("cap_per_image", MD))
    assert det.truncated == any(c > limit for c in counts)                 # a list that was cut is reported, the counts stay true
    for i, (r, c, passes) in enumerate(frames):
        want, count, src, ncand = tr.merge(r, c, passes, NET, NET, NMS, MD, OV, EDGE, True, kw.get("max_faces", 0))
        want = want[:kw["cap_per_image"]] if "cap_per_image" in kw else want
        assert counts[i] == count, (i, counts[i], count, ncand)
        assert rows_of(dets[i]).tobytes() == want.tobytes(), (i, ncand)
        assert list(tiles[i]) == list(src[:len(want)]), i
    return dets, tiles, counts


SHAPES = {"2x2": (700, 750), "3x1": (300, 1009), "fit": (448, 448)}


def test_merge_of_constructed_faces_equals_the_reference(rfa):
    det = engine(rfa)
    assert len(tr.plan(700, 750, NET, NET, OV)) == 5 and len(tr.plan(300, 1009, NET, NET, OV)) == 4
    assert [int(t[0]) for t in tr.plan(300, 1009, NET, NET, OV)[:3]] == [0, 280, 561] and int(tr.plan(700, 750, NET, NET, OV)[3][1]) == 252
    made = {}

    def frame(shape, want, seed):
        key = (shape, want)
        if key not in made:
            made[key] = SHAPES[shape] + (constructed_frame(seed, *SHAPES[shape], want),)
        return made[key]
    # the three sort regimes of the merge and their boundaries, three frames with different plans per call, empty passes included
    calls = ([frame("2x2", 0, 1), frame("3x1", 1, 2), frame("fit", 64, 3)],
             [frame("2x2", 65, 4), frame("3x1", 256, 5), frame("2x2", 257, 6)],
             [frame("2x2", 1000, 7), frame("3x1", 64, 8)])
    kept = []
    for frames in calls:
        dets, tiles, counts = check_merge_call(det, frames)
        kept += counts
        again = det.tile_merge([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], overlap=OV, edge=EDGE, return_tiles=True)
        assert again[0] == dets and all(np.array_equal(a, b) for a, b in zip(again[1], tiles))      # the append order does not leak
    assert kept[0] == 0 and kept[1] == 1 and all(0 < k <= w for k, w in zip(kept[2:], (64, 65, 256, 257, 1000, 64)))
    # suppression across tiles happened, and so did both outcomes of the edge rule and ties between tiles
    r, c, passes = frame("2x2", 257, 6)
    cand, g = tr.candidates(r, c, passes, NET, NET, MD, OV, EDGE)
    assert sum(len(p) for p in passes) > len(cand) == 257 > tr.merge(r, c, passes, NET, NET, NMS, MD, OV, EDGE)[1]
    assert len(set(cand[:, 0].tolist())) < 40
    # a smaller max_faces and a smaller cap_per_image: counts stay true
    check_merge_call(det, [frame("2x2", 257, 6), frame("3x1", 256, 5)], max_faces=7)
    assert det.truncated
    check_merge_call(det, [frame("2x2", 65, 4)], cap_per_image=5)
    assert det.truncated and det.tiled_counts[0] > 5


def test_merge_overflow_is_reported_and_leaves_the_other_frame_exact(rfa):
    det = engine(rfa)
    rng = np.random.default_rng(9)
    tiles = tr.plan(2000, 2000, NET, NET, OV)
    assert len(tiles) == 37
    grid = [box_face(rng, 12.0 + 26 * (j % 16), 12.0 + 26 * (j // 16), 20.0, 20.0) for j in range(MD)]      # 256 disjoint boxes, all inside the band
    big = [np.stack(grid)] * 36 + [np.zeros((0, 15), np.float32)]
    assert tr.candidates(2000, 2000, big, NET, NET, MD, OV, EDGE)[0].shape[0] == 36 * MD > tr.MERGE_CAP
    other = (700, 750, constructed_frame(11, 700, 750, 300))
    for order in ((0, 1), (1, 0)):
        frames = [(2000, 2000, big), other]
        frames = [frames[k] for k in order]
        dets, tiles_, = det.tile_merge([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], overlap=OV, edge=EDGE, return_tiles=True)
        assert det.truncated
        i = order.index(1)
        want, count, src, _ = tr.merge(*other[:2], other[2], NET, NET, NMS, MD, OV, EDGE)
        assert det.tiled_counts[i] == count and rows_of(dets[i]).tobytes() == want.tobytes() and list(tiles_[i]) == list(src)
    check_merge_call(det, [other])                                         # the counters were re-armed: the next call is exact


# ---------------------------------------------------------------------------------------------- 2. fused call against its own parts
@pytest.fixture(scope="module")
def mosaic(base_frame):
    m = tr.mosaic(base_frame)
    m.setflags(write=False)
    return m


def parts_of_call(det, frames, full=True, overlap=OV, edge=EDGE, thr=0.5):
    """frames: (ptr, rows, cols, step) of one tiled call.  tile_ref.merge, per frame, over what ONE rf_detect_batch_device call returns
    for the views of all frames in plan order -- the call the engine itself makes.  (One call for brevity: a view's result does not
    depend on what shares its launch -- a view that fits the net is read where it lies even when the oversize full-frame pass puts the
    resize kernel into the launch -- which test_fused_call_equals_the_merge_of_its_own_passes checks pass by pass.)"""
    plans = [tr.plan(r, c, det.net_h, det.net_w, overlap, full) for _, r, c, _ in frames]
    ptrs = [p + int(t[1]) * st + 3 * int(t[0]) for (p, _, _, st), tiles in zip(frames, plans) for t in tiles]
    res = det.detect_device(ptrs, [int(t[3]) for tiles in plans for t in tiles], [int(t[2]) for tiles in plans for t in tiles], thr,
                            steps=[st for (_, _, _, st), tiles in zip(frames, plans) for _ in tiles])
    assert not det.truncated
    out, at = [], 0
    for (_, r, c, _), tiles in zip(frames, plans):
        passes = [rows_of(x) for x in res[at:at + len(tiles)]]
        at += len(tiles)
        out.append((tr.merge(r, c, passes, det.net_h, det.net_w, NMS, MD, overlap, edge, full), passes))
    return out


def parts(det, ptr, rows, cols, step, **kw):
    return parts_of_call(det, [(ptr, rows, cols, step)], **kw)[0]


def check_tiled(got, tiles, counts, i, want):
    faces, count, src, _ = want
    assert counts[i] == count and rows_of(got[i]).tobytes() == faces.tobytes() and list(tiles[i]) == list(src), (i, counts[i], count)


@pytest.mark.parametrize("prec,kw", ((FP16, {}), (FP16, SPLIT2), (FP16, SPLIT3), (INT8, {}), (INT8, SPLIT2)))
def test_fused_call_equals_the_merge_of_its_own_passes(rfa, mosaic, crop448, prec, kw):
    """kw = {}: the whole call is one coalesced launch.  SPLIT2 / SPLIT3: the 13 passes of a frame cross launches and lanes -- the
    gathers of one frame append from two streams, the merge waits for the other lanes' gathers on the device, and in the three-frame
    call the pinned pass table of a lane is reused after its harvest."""
    det = split_engine(rfa, kw, prec=prec)
    dev = to_device([mosaic, crop448])
    ptr = dev[0].data_ptr()
    want, passes = parts(det, ptr, 896, 1280, 3 * 1280)
    assert len(passes) == 13 and sum(len(p) for p in passes) > want[1] >= 20
    got, tiles = det.detect_tiled_device([ptr], [896], [1280], 0.5, overlap=OV, edge=EDGE, return_tiles=True)
    assert not det.truncated
    check_tiled(got, tiles, det.tiled_counts, 0, want)
    assert len(set(tiles[0].tolist())) > 4                                 # faces come from many tiles
    # two such frames and one that fits the net, in one call: 27 passes (one launch by default, four launches under SPLIT2 / SPLIT3)
    small = det.detect_device([dev[1].data_ptr()], [448], [448], 0.5)[0]
    got3, tiles3 = det.detect_tiled_device([ptr, dev[1].data_ptr(), ptr], [896, 448, 896], [1280, 448, 1280], 0.5, overlap=OV, edge=EDGE,
                                           return_tiles=True)
    want3 = parts_of_call(det, [(ptr, 896, 1280, 3 * 1280), (dev[1].data_ptr(), 448, 448, 3 * 448), (ptr, 896, 1280, 3 * 1280)])
    for i in range(3):
        check_tiled(got3, tiles3, det.tiled_counts, i, want3[i][0])
    check_tiled(got3, tiles3, det.tiled_counts, 0, want)                   # frame 0 starts the call: chunked as the single-frame call
    assert rows_of(got3[1]).tobytes() == rows_of(small).tobytes() and len(small) >= 1 and not tiles3[1].any()
    assert len(got3[2]) == len(got3[0]) == 24
    # full_frame off
    want_off, _ = parts(det, ptr, 896, 1280, 3 * 1280, full=False)
    got_off, tiles_off = det.detect_tiled_device([ptr], [896], [1280], 0.5, overlap=OV, edge=EDGE, full_frame=False, return_tiles=True)
    check_tiled(got_off, tiles_off, det.tiled_counts, 0, want_off)
    assert max(tiles_off[0]) < 12
    # repeats give identical bytes: with several streams appending, the append order varies and must not show
    for _ in range(3):
        r3 = det.detect_tiled_device([ptr, dev[1].data_ptr(), ptr], [896, 448, 896], [1280, 448, 1280], 0.5, overlap=OV, edge=EDGE, return_tiles=True)
        assert r3[0] == got3 and all(np.array_equal(a, b) for a, b in zip(r3[1], tiles3))
    if prec != FP16:
        return
    # the frame as an odd-pointer, odd-step ROI
    keep, rptr, rstep = roi_view(mosaic)
    want_roi, passes_roi = parts(det, rptr, 896, 1280, rstep)
    got_roi, tiles_roi = det.detect_tiled_device([rptr], [896], [1280], 0.5, steps=[rstep], overlap=OV, edge=EDGE, return_tiles=True)
    check_tiled(got_roi, tiles_roi, det.tiled_counts, 0, want_roi)
    # Every pass detected ALONE gives the bytes it gives inside the call's launches, whatever shares them and however the call is split:
    # only the oversize full-frame pass is read from the resize canvas, a view that fits is read where it lies.  (Until the scheduler
    # tests, a launch that held an oversize frame read every image from the canvas: the one-launch call then gave the aligned frame and
    # the odd view the same bytes, and each of them other bytes than the same view in a launch without the full-frame pass.)
    for p0, st, ps in ((ptr, 3 * 1280, passes), (rptr, rstep, passes_roi)):
        for t, rows_in_call in zip(tr.plan(896, 1280, det.net_h, det.net_w, OV, True), ps):
            alone = det.detect_device([p0 + int(t[1]) * st + 3 * int(t[0])], [int(t[3])], [int(t[2])], 0.5, steps=[st])[0]
            assert rows_of(alone).tobytes() == rows_in_call.tobytes(), (st, list(t))
    assert len(got_roi[0]) == want[1]
    # host frames: uploaded once, the tiles are views of the copy; an empty frame in between
    hgot, htiles = det.detect_tiled([mosaic, None, crop448], 0.5, overlap=OV, edge=EDGE, return_tiles=True)
    check_tiled(hgot, htiles, det.tiled_counts, 0, want)
    assert hgot[1] == [] and rows_of(hgot[2]).tobytes() == rows_of(small).tobytes()
    # the default spec (overlap 112, 13 passes as well) and a repeat: identical bytes
    d1 = det.detect_tiled_device([ptr], [896], [1280], 0.5)
    want_def, _ = parts(det, ptr, 896, 1280, 3 * 1280, overlap=0, edge=0)
    assert rows_of(d1[0]).tobytes() == want_def[0].tobytes() and det.detect_tiled_device([ptr], [896], [1280], 0.5) == d1
    # the ordinary calls are what they were
    assert det.detect_device([dev[1].data_ptr()], [448], [448], 0.5)[0] == small


# ---------------------------------------------------------------------------------------------- 3. invariant
def test_a_frame_that_fits_the_net_gives_the_plain_result(rfa, crop448):
    det = engine(rfa)
    dev = to_device([crop448, np.ascontiguousarray(crop448[:300, :211])])
    ptrs, rows, cols = [d.data_ptr() for d in dev], [448, 300], [448, 211]
    plain = det.detect_device(ptrs, rows, cols, 0.5)
    for kw in ({}, dict(overlap=OV, edge=EDGE, full_frame=False), dict(overlap=-1, edge=-1)):
        got, tiles = det.detect_tiled_device(ptrs, rows, cols, 0.5, return_tiles=True, **kw)
        assert [rows_of(g).tobytes() for g in got] == [rows_of(p).tobytes() for p in plain] and len(got[0]) >= 1
        assert det.tiled_counts == [len(p) for p in plain] and not any(t.any() for t in tiles)


# ---------------------------------------------------------------------------------------------- 4. end to end
def test_mosaic_end_to_end(rfa, mosaic):
    det = engine(rfa)
    dev = to_device([mosaic])[0]
    tiled = rows_of(det.detect_tiled_device([dev.data_ptr()], [896], [1280], 0.5, overlap=OV, edge=EDGE)[0])
    assert len(tiled) == 24 == det.tiled_counts[0]
    native = rows_of(det.detect_pad32([mosaic], 0.5)[0])
    shrunk = det.detect_device([dev.data_ptr()], [896], [1280], 0.5)[0]
    best = [max(tr.iou_plus1(n[1:5], t[1:5]) for t in tiled) for n in native]
    print(f"tiled {len(tiled)} faces, native-size {len(native)}, shrunk pass {len(shrunk)}; worst IoU of a native-size face against the tiled set {min(best):.4f}")
    assert len(native) >= 20
    assert min(best) >= 0.8, f"worst IoU against the native-size result {min(best):.4f} (floor 0.8)"


# ---------------------------------------------------------------------------------------------- 5. tiled face batch
@pytest.mark.parametrize("kw", ({}, SPLIT2))
def test_tiled_face_batch_equals_the_face_batch_of_the_tiled_result(rfa, mosaic, crop448, kw):
    det = split_engine(rfa, kw)
    dev = to_device([mosaic])[0]
    args = ([dev.data_ptr()], [896], [1280])
    tiled = det.detect_tiled_device(*args, 0.5, overlap=OV, edge=EDGE)
    faces = [rows_of(tiled[0])]
    assert len(faces[0]) == 24
    base = det.face_batch(*args, faces, crop_size=112, dtype="f16", return_quality=True, max_faces=MD)
    gate = dict(min_sharpness=float(np.float32(np.median(base[4][0]["sharpness"]))))
    for capacity in (10, 64):
        for g in (None, gate):
            kw = dict(crop_size=112, dtype="f16", capacity=capacity, gate=g, return_quality=True)
            want = det.face_batch(*args, faces, max_faces=MD, **kw)
            want_trunc = det.faces_truncated
            got = det.detect_tiled_face_batch_device(*args, 0.5, overlap=OV, edge=EDGE, **kw)
            assert got[0] == tiled
            assert same(got[1], want[1]) and np.array_equal(got[2], want[2]) and list(got[3]) == list(want[3]) and same_records(got[4], want[4])
            assert det.faces_truncated == want_trunc == (int(want[3][1]) > capacity) and det.truncated == want_trunc
            if g is None:
                assert int(got[3][1]) == 24 and (capacity == 10) == det.faces_truncated
            else:
                assert 0 < int(got[3][1]) < 24
        # the ungated entry: the same tensor, no records
        plain = det.detect_tiled_face_batch_device(*args, 0.5, overlap=OV, edge=EDGE, crop_size=112, dtype="f16", capacity=capacity)
        ref = det.face_batch(*args, faces, crop_size=112, dtype="f16", capacity=capacity, max_faces=MD)
        assert len(plain) == 4 and same(plain[1], ref[1]) and np.array_equal(plain[2], ref[2]) and list(plain[3]) == list(ref[3])
    # max_faces of either spec bounds the faces per frame
    cut = det.detect_tiled_face_batch_device(*args, 0.5, overlap=OV, edge=EDGE, tile_max_faces=5, max_faces=9, crop_size=112, dtype="f16")
    ref5 = det.face_batch(*args, [faces[0][:5]], crop_size=112, dtype="f16", max_faces=9)
    assert list(cut[3]) == [0, 5] and same(cut[1], ref5[1]) and det.tiled_counts == [24] and len(cut[0][0]) == 5
    # three frames in one call (27 passes; four launches under SPLIT2): the face batch follows the merge of ALL of them
    small = to_device([crop448])[0]
    args3 = ([dev.data_ptr(), small.data_ptr(), dev.data_ptr()], [896, 448, 896], [1280, 448, 1280])
    tiled3 = det.detect_tiled_device(*args3, 0.5, overlap=OV, edge=EDGE)
    kw3 = dict(crop_size=112, dtype="f16", gate=gate, return_quality=True, max_faces=6)
    want3 = det.face_batch(*args3, [rows_of(d) for d in tiled3], **kw3)
    got3 = det.detect_tiled_face_batch_device(*args3, 0.5, overlap=OV, edge=EDGE, **kw3)
    assert got3[0] == tiled3 and len(tiled3[1]) >= 1 and tiled3[0] == tiled[0] and len(tiled3[2]) == 24
    assert same(got3[1], want3[1]) and np.array_equal(got3[2], want3[2]) and list(got3[3]) == list(want3[3]) and same_records(got3[4], want3[4])
    assert 0 < int(got3[3][1]) < int(got3[3][3])


# ---------------------------------------------------------------------------------------------- 6. refusals
def tiled_calls(det, ptr, spec_kw):
    return (lambda: det.detect_tiled_device([ptr], [448], [448], 0.5, **spec_kw),
            lambda: det.detect_tiled([np.zeros((448, 448, 3), np.uint8)], 0.5, **spec_kw),
            lambda: det.tile_merge([448], [448], [[np.zeros((0, 15), np.float32)]], **spec_kw),
            lambda: det.detect_tiled_face_batch_device([ptr], [448], [448], 0.5, **{("tile_max_faces" if k == "max_faces" else k): v
                                                                                      for k, v in spec_kw.items()}))


def test_bad_specs_are_refused_and_leave_the_handle_usable(rfa, crop448):
    det = engine(rfa)
    dev = to_device([crop448])[0]
    before = det.detect_device([dev.data_ptr()], [448], [448], 0.5)[0]
    # "Golden bytes": the only golden of this frame is the fp32 oracle's result, and no fp16 golden exists.  So the call after the
    # refusals is compared byte for byte with the same call BEFORE them, and that result is tied to the golden only by face count and
    # IoU >= 1 - 1e-3 (the fp16 contract) -- a weaker check than a byte comparison against a stored fp16 result would be.
    gold = golden("crop448_mnet25.npz")["det"]
    assert len(before) == len(gold) and all(tr.iou_plus1(b.rect, g[1:5]) >= 1 - 1e-3 for b, g in zip(before, gold))
    for bad in (dict(overlap=448), dict(overlap=10000), dict(max_faces=4097), dict(max_faces=-1), dict(edge=224)):
        for call in tiled_calls(det, dev.data_ptr(), bad):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1, bad
    sp = rfa.tile_spec()
    sp.struct_size = 16
    cnt, out = (C.c_int * 1)(), (rfa._lib.rf_face * MD)()
    st = det._lib.rf_detect_tiled_batch_device(det._h, (C.c_void_p * 1)(dev.data_ptr()), (C.c_int * 1)(448), (C.c_int * 1)(448), (C.c_int * 1)(1344),
                                               1, 0.5, C.byref(sp), out, MD, cnt, None)
    assert st == -1
    import torch
    large = torch.zeros((3000, 3000, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(rfa.RFError):                                       # a plan of more than 1024 passes
        det.detect_tiled_device([large.data_ptr()], [3000], [3000], 0.5, overlap=440)
    assert det.detect_device([dev.data_ptr()], [448], [448], 0.5)[0] == before
    assert det.detect_tiled_device([dev.data_ptr()], [448], [448], 0.5)[0] == [rfa.Detection(d.score, d.rect, d.xs, d.ys, -1) for d in before]


def test_multi_device_handles_refuse_tiled_detection(rfa, crop448):
    det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", devices=[0, 0])
    try:
        dev = to_device([crop448])[0]
        for call in tiled_calls(det, dev.data_ptr(), {}):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -5
        assert len(det.detect_device([dev.data_ptr()], [448], [448], 0.5)[0]) >= 1
    finally:
        det.close()


# ---------------------------------------------------------------------------------------------- 7. the C++ class
def test_cpp_class_detect_tiled(rfa, mosaic, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_tile.cpp")
    exe = str(tmp_path / "test_tile")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    raw, out = str(tmp_path / "frame.raw"), str(tmp_path / "out.bin")
    mosaic.tofile(raw)
    det = engine(rfa)
    for overlap, edge, full, mf in ((OV, EDGE, 1, 0), (0, 0, 2, 7)):
        r = subprocess.run([exe, ASSETS, "mnet25", "448", "448", raw, "896", "1280", "0.5", str(overlap), str(edge), str(full), str(mf), out],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        blob = open(out, "rb").read()
        n = int(np.frombuffer(blob, np.int32, 1)[0])
        assert n == 3
        pos, faces, srcs = 4, [], []
        for _ in range(n):
            k = int(np.frombuffer(blob, np.int32, 1, pos)[0])
            faces.append(np.frombuffer(blob, np.float32, k * 15, pos + 4).reshape(k, 15))
            srcs.append(np.frombuffer(blob, np.int32, k, pos + 4 + 60 * k))
            pos += 4 + 64 * k
        assert pos == len(blob)
        want, tiles = det.detect_tiled([mosaic, None, mosaic], 0.5, overlap=overlap, edge=edge, full_frame=full == 1, max_faces=mf, return_tiles=True)
        assert len(faces[0]) == (mf or 24) and len(faces[1]) == 0
        for i in range(n):
            assert faces[i].tobytes() == rows_of(want[i]).tobytes() and list(srcs[i]) == list(tiles[i]), i
