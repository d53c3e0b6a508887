"""Tracked region detection on the GPU: the plan kernel against rf_roi_cells_from_tracks and tests/roi_track_ref.py byte for byte, void
cells through the atlas kernel, the fused call against its own parts (ONE rf_detect_batch_device call over the reference's views + the
reference's face rule, merge and frame step), the prefix identity with the plain region call, a tracked region call of 32 passes
between a tiled and a plain region call on a handle that splits its launches, the refusals (which change nothing), and the C++ class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import motion_ref as mr
import roi_ref as rr
import roi_track_ref as rtr
import track_ref as tr
from conftest import ASSETS, ROOT
from test_gpu_align import FP16, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_roi_gpu import regions, scene  # noqa: F401  (scene: fixture)
from test_track_gpu import check_tables, tr_scale
from test_track_host import by_score, face
from test_tta_gpu import NET, NMS, SPLIT3, odd_view

pytestmark = pytest.mark.gpu
f32 = np.float32
VOID_ROI = (0, 0, 0, 0)
EMPTY = np.zeros(0, tr.FACE)


def ref_streams(n, motion=None, **kw):
    spec = tr.Spec(**kw)
    return [mr.Stream(spec, mr.Spec(*motion)) if motion is not None else tr.Stream(spec) for _ in range(n)]


def ref_step(stream, rows, scale=1.0):
    fn = mr.step if isinstance(stream, mr.Stream) else tr.step
    rows = np.asarray(rows, np.float32).reshape(-1, 15)
    return fn(stream, tr.faces_array(rows) if len(rows) else EMPTY, scale)


def check_state(trk, ref):
    check_tables(trk, ref)
    if isinstance(ref[0], mr.Stream):
        for s, r in enumerate(ref):
            assert trk.read_motion(s).tobytes() == r.motion.tobytes(), s


def update(trk, ref, streams, per_image):
    """rf_track_update_device with designed faces (source pixels), mirrored on the reference"""
    trk.update(streams, [by_score(f) if len(f) else EMPTY for f in per_image], cap_per_image=64, cap_ended=16)
    for s, f in zip(streams, per_image):
        if s >= 0:
            ref_step(ref[s], tr.rows_of(by_score(f)) if len(f) else np.zeros((0, 15), np.float32))
    check_state(trk, ref)


def spread(n, x0=30.0, size=40.0):
    return [face(0.99 - 0.001 * k, x0 + 97.0 * (k % 12) + 0.25 * k, 20.0 + 83.0 * (k // 12), size + (k % 7) * 9.5) for k in range(n)]


def void_cells(T):
    return np.array([rtr.VOID_CELL] * T, np.int32)


# ---------------------------------------------------------------------------------------------- 1. the plan kernel
@pytest.mark.parametrize("motion", (None, (0.5, 8), (1.0, -1)))
@pytest.mark.parametrize("max_tracks", (1, 16, 17))
def test_plan_kernel_equals_the_host_code_and_the_reference(rfa, max_tracks, motion):
    """three streams in one call with a stream -1 image between them: a live prefix with holes (max_missed = 1 and steps that omit
    faces) and, with motion, a velocity (two steps with displaced faces); boxes roi_from_face refuses; a free table"""
    det = engine(rfa)
    kw = dict(max_tracks=max_tracks, max_missed=1, min_hits=1)
    trk = det.tracker(3, motion=dict(alpha=motion[0], horizon=motion[1]) if motion else None, **kw)
    ref = ref_streams(3, motion, **kw)
    try:
        rows = spread(max(max_tracks - 2, 1))
        update(trk, ref, [0, 1], [rows, spread(3, 500.0, 200.0)])
        for t in (1, 2):                                         # every third face is omitted and ends; the others move 5 px a frame
            moved = [r + f32(5 * t) * (np.arange(15) > 0) * (np.arange(15) < 10) for k, r in enumerate(rows) if k % 3 != 1]
            update(trk, ref, [0], [[np.asarray(m, np.float32) for m in moved]])
        live = ref[0].table["id"] != 0
        assert max_tracks == 1 or (live[0] and not live[1])
        if motion and motion[1] > 0:
            assert ref[0].motion["samples"][0] == 2 and ref[0].motion["vx"][0] == 5
        wild = [face(0.9, 10.0, 10.0, 30.0) for _ in range(3)]   # stream 1 gets boxes that are not finite / beyond 2^20 in free slots
        wild[0][1] = np.nan
        wild[1][3] = np.inf
        wild[2][1:5] = (4e6, 0, 4e6 + 5, 5)
        for k, w in enumerate(wild):
            w[0] = 0.5 - 0.01 * k
        update(trk, ref, [1], [spread(3, 500.0, 200.0) + wild])
        for margin, grid, mz in ((None, 4, 0), (1 / 256, 2, 4), (1.5, 1, 1)):
            streams = [0, -1, 1, 2]
            got = trk.roi_cells(streams, margin, grid, mz)
            assert got.shape == (4, max_tracks, 8)
            for i, s in enumerate(streams):
                if s < 0:
                    assert np.array_equal(got[i], void_cells(max_tracks))
                    continue
                table = trk.read(s)[0]
                host = rfa.roi_cells_from_tracks(table, NET, NET, motion=trk.read_motion(s) if motion else None,
                                                 mspec=dict(alpha=motion[0], horizon=motion[1]) if motion else None, margin=margin, grid=grid, max_zoom=mz)
                want = rtr.stream_cells(ref[s], 0 if margin is None else int(round(margin * 256)), NET, NET, grid, mz)
                assert np.array_equal(got[i], host) and np.array_equal(got[i], want), (i, s, margin, grid)
            assert np.array_equal(got[3], void_cells(max_tracks))                 # stream 2 never stepped: a free table
            live1 = ref[1].table["id"] != 0
            assert max_tracks < 16 or (int(live1.sum()) == 6 and int((got[2][live1, 7] == rtr.VOID).sum()) == 3)      # the refused boxes are void
        check_state(trk, ref)                                                      # the plan kernel changes nothing
    finally:
        trk.close()


# ---------------------------------------------------------------------------------------------- 2. void cells on the device
@pytest.mark.parametrize("view", ((32, 16, 2), (64, 48, 4), (448, 448, 4)))
def test_atlas_device_with_void_cells(rfa, view):
    """void cells first, last and between real ones of every level, one of them next to a x1/4 cell whose whole tiles take the staged
    path; a dense source and a pitched one at an odd address; a dense destination and a pitched one at an odd address, 0xAB around"""
    import torch
    det = engine(rfa)
    vw, vh, grid = view
    cw, ch = vw // grid, vh // grid
    rows, cols = 300, 640
    frame = np.random.default_rng(vw).integers(1, 256, (rows, cols, 3), dtype=np.uint8)      # no zero byte: a zero pixel was not read
    quarter = (20, 10, min(4 * cw - 8, 600), min(4 * ch - 8, 280))                              # x1/4, its source box inside the frame
    real = [quarter, (100, 40, 2 * cw - 2, 2 * ch - 2), (300, 100, cw, ch), (5, 7, max(cw // 2, 1), max(ch // 2, 1)), (-6, 60, cw // 4 or 1, ch // 4 or 1),
            (600, 280, 3 * cw, ch)]
    rois, nxt = [], 0
    for k in range(grid * grid + 3):
        void = k % 3 == 0 or k == grid * grid + 2
        rois.append(VOID_ROI if void else real[nxt % len(real)])
        nxt += not void
    assert rois[0] == VOID_ROI and rois[1] == quarter
    cells = np.array([rtr.VOID_CELL if r == VOID_ROI else tuple(r) + rr.plan_one(r, cw, ch, 4) for r in rois], np.int32)
    assert cells[1, 4] == -2 and not cells[1, 7] and len(set(cells[:, 4].tolist())) >= (5 if grid == 4 else 4)
    want = rtr.atlas(frame, cells, vw, vh, grid)
    P = len(want)
    assert P == 2 and np.array_equal(rfa.roi_atlas_host(frame, rois, vw, vh, grid, 4), want)
    assert not want[0, :ch, :cw].any() and want[0, :ch, cw:2 * cw].any()                      # the void cell next to the x1/4 cell
    dense = to_device([frame])[0]
    keep, rptr, rstep = odd_view(frame)
    for sptr, sstep, pad, shift in ((dense.data_ptr(), 3 * cols, 0, 0), (rptr, rstep, 7, 1)):
        dstep = 3 * vw + pad
        dst = torch.full((P * vh * dstep + 8,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        det.roi_atlas_device(sptr, rows, cols, rois, dst.data_ptr() + shift, vw, vh, step=sstep, dst_step=dstep, grid=grid, max_zoom=4)
        got = dst.cpu().numpy()
        body = got[shift:shift + P * vh * dstep].reshape(P * vh, dstep)
        assert np.array_equal(body[:, :3 * vw].reshape(P, vh, vw, 3), want), (view, pad, shift)
        assert (body[:, 3 * vw:] == 0xAB).all() and (got[:shift] == 0xAB).all() and (got[shift + P * vh * dstep:] == 0xAB).all()
    with pytest.raises(rfa.RFError):
        det.roi_atlas_device(dense.data_ptr(), rows, cols, [(0, 0, 0, 5)], dst.data_ptr(), vw, vh)       # empty, but not the void region


# ---------------------------------------------------------------------------------------------- 3. the fused call against its own parts
def key_call(det, trk, ref, dev, frames, streams, thr=0.5):
    """rf_detect_track_batch_device, mirrored on the reference (coord_scale = the frame's scale: tracks in source pixels)"""
    shapes = [f.shape for f in frames]
    got, tags, ended = det.detect_tracked_device([d.data_ptr() for d in dev], [s[0] for s in shapes], [s[1] for s in shapes], trk, streams, thr)
    for i, s in enumerate(streams):
        if s >= 0:
            ref_step(ref[s], rows_of(got[i]), tr_scale(det, shapes[i][0], shapes[i][1]))
    check_state(trk, ref)
    return got


def parts_of_call(det, ref, frames, streams, thr, margin, grid, max_zoom, vote, max_faces):
    """The comparison target.  Per image: the cells the reference plans from the reference stream; ONE plain call over the reference's
    views of all images in call order; roi_track_ref's face rule and merge; the reference step.  Returns (per image: (faces, count,
    votes, src, tags, ended, cells), the views, whether a step overflowed)"""
    md, T = det.max_detections, ref[0].spec.max_tracks
    mq = 0 if margin is None else int(round(margin * 256))
    plans, views = [], []
    for f, s in zip(frames, streams):
        cells = rtr.stream_cells(ref[s], mq, NET, NET, grid, max_zoom) if f is not None and s >= 0 else None
        plans.append(cells)
        if cells is not None:
            views += list(rtr.atlas(f, cells, NET, NET, grid))
    dev = to_device(views)
    res = det.detect_device([d.data_ptr() for d in dev], [NET] * len(dev), [NET] * len(dev), thr) if views else []
    assert not det.truncated
    out, q, over = [], 0, False
    PP = rr.passes_of(T, grid)
    none = (np.zeros((0, 15), np.float32), 0, np.zeros(0, np.int32), np.zeros(0, np.int32))
    for f, s, cells in zip(frames, streams, plans):
        if s < 0:
            out.append(none + (np.zeros(0, tr.TAG), np.zeros(0, tr.TRACK), void_cells(T)))
            continue
        merged = none
        if cells is not None:
            merged = rtr.merge(cells, [rows_of(x) for x in res[q:q + PP]], NET, NET, NMS, md, grid, vote, max_faces)[:4]
            q += PP
        tags, ended, o = rtr.step(ref[s], merged[0], max_faces or md)
        over = over or o
        out.append(tuple(merged) + (tags, ended, cells if cells is not None else void_cells(T)))
    assert q == len(res)
    return out, views, over


def check_call(det, trk, ref, frames, streams, call, thr=0.5, margin=None, grid=0, max_zoom=0, vote=False, max_faces=0, views=None):
    """one tracked region call (call(**kw) makes it) against its parts: out, counts, src_roi, votes, cells, tags, ended lists, then
    rf_tracker_read and rf_tracker_read_motion of every stream"""
    want, ref_views, over = parts_of_call(det, ref, frames, streams, thr, margin, grid, max_zoom, vote, max_faces)
    got, tags, ended, votes, src = call(threshold=thr, margin=margin, grid=grid, max_zoom=max_zoom, vote=vote, max_faces=max_faces, return_src_roi=True)
    cap = max_faces or det.max_detections
    for i, w in enumerate(want):
        faces, count, wv, ws, wt, we, wc = w
        assert det.roi_counts[i] == count and rows_of(got[i]).tobytes() == faces.tobytes(), (i, det.roi_counts[i], count)
        assert list(votes[i]) == list(wv) and list(src[i]) == list(ws), i
        assert np.array_equal(trk.last_cells[i], wc), i
        assert tags[i].tobytes() == wt.tobytes() and ended[i].tobytes() == we.tobytes(), i
        assert trk.last_ended_counts[i] == len(we)
        if streams[i] < 0:
            assert not trk.last_tags[i].view(np.uint8).any()
    assert det.truncated == trk.truncated == (over or any(w[1] > cap for w in want))
    check_state(trk, ref)
    if views is not None:
        have = views.cpu().numpy()[:len(ref_views) * NET * NET * 3].reshape(len(ref_views), NET, NET, 3)
        assert all(np.array_equal(h, v) for h, v in zip(have, ref_views)) and (views.cpu().numpy()[len(ref_views) * NET * NET * 3:] == 0xAB).all()
    return got, tags, src


@pytest.mark.parametrize("max_tracks,motion", ((16, None), (17, None), (16, (0.5, 8))))
@pytest.mark.parametrize("stem", ("mnet25", "mnet-deconv-0517"))
def test_fused_call_equals_its_own_parts(rfa, scene, stem, max_tracks, motion):
    """a key call on frames of 896 x 1280 and 200 x 240 over three streams, holes, then tracked region calls: device frames with
    d_views; a NULL frame whose stream ages and whose tracks end on the second call; a stream -1 image; max_tracks = 17 at grid 4
    (the second pass has one cell); vote on; a pitched frame at an odd pointer; host frames; a cap that cuts"""
    import torch
    det = engine(rfa, stem=stem)
    big, small, own = scene
    kw = dict(max_tracks=max_tracks, max_missed=1, min_hits=2)
    trk = det.tracker(3, motion=dict(alpha=motion[0], horizon=motion[1]) if motion else None, **kw)
    ref = ref_streams(3, motion, **kw)
    try:
        dev = to_device([big, small])
        key = key_call(det, trk, ref, [dev[0], dev[1], dev[0]], [big, small, big], [0, 2, 1])
        assert len(key[0]) >= 4 and len(key[1]) >= 1
        # holes: two steps on stream 0 that omit the track of slot 1 end it; the others move by (3, 2) a step
        for t in (1, 2):
            lasts = [np.frombuffer(r["last"].tobytes(), np.float32).copy() for k, r in enumerate(ref[0].table) if r["id"] != 0 and k != 1]
            moved = []
            for r in lasts:
                r[[1, 3, 5, 6, 7, 8, 9]] += f32(3)
                r[[2, 4, 10, 11, 12, 13, 14]] += f32(2)
                moved.append(r)
            update(trk, ref, [0], [moved])
        assert ref[0].table["id"][1] == 0 and ref[0].table["id"][0] != 0 and ref[0].table["id"][2] != 0
        frames, streams = [big, small, None, big], [0, 2, 1, -1]
        ptrs, rows, cols = [dev[0].data_ptr(), dev[1].data_ptr(), 0, dev[0].data_ptr()], [896, 200, 0, 896], [1280, 240, 0, 1280]
        PP = rr.passes_of(max_tracks, 4)
        assert PP == (1 if max_tracks == 16 else 2)
        views = torch.full((2 * PP * NET * NET * 3 + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        live1 = int((ref[1].table["id"] != 0).sum())
        got, tags, src = check_call(det, trk, ref, frames, streams, views=views,
                                    call=lambda **k: trk.detect_tracked_rois_device(ptrs, rows, cols, streams, views_ptr=views.data_ptr(), **k))
        assert len(got[0]) >= 3 and len(got[1]) >= 1 and got[2] == [] and got[3] == []
        assert not (tags[0]["flags"] & tr.NEW).any() and list(tags[0]["slot"]) == [int(s) for s in src[0]]      # ids kept, by their own slots
        assert live1 > 0 and int((ref[1].table["id"] != 0).sum()) == live1 and (ref[1].table["missed"][ref[1].table["id"] != 0] == 1).all()
        # the second call: vote on, a pitched small frame at an odd pointer; the NULL frame's tracks end
        keep, rptr, rstep = odd_view(small)
        p2 = [ptrs[0], rptr, 0, ptrs[3]]
        check_call(det, trk, ref, frames, streams, vote=True,
                   call=lambda **k: trk.detect_tracked_rois_device(p2, rows, cols, streams, steps=[3 * 1280, rstep, 0, 3 * 1280], **k))
        assert trk.last_ended_counts[2] == live1 and not (ref[1].table["id"] != 0).any()
        # host frames (one with a row pitch), another margin, grid and zoom
        wide = np.zeros((200, 260, 3), np.uint8)
        wide[:, :240] = small
        hframes = [big, wide[:, :240], None, big]
        check_call(det, trk, ref, frames, streams, margin=0.5, grid=2, max_zoom=4, call=lambda **k: trk.detect_tracked_rois(hframes, streams, **k))
        # a cap that cuts: RF_ERR_TRUNCATED, the step sees the first two faces
        full = len(got[0])
        check_call(det, trk, ref, frames, streams, max_faces=2, call=lambda **k: trk.detect_tracked_rois_device(ptrs, rows, cols, streams, **k))
        assert det.truncated and det.roi_counts[0] > 2 and full > 2
        # n = 0, and a call whose frames are all NULL or untracked: no pass, the stream still steps
        assert trk.detect_tracked_rois_device([], [], [], []) == ([], [], [])
        check_call(det, trk, ref, [None, None], [0, -1], call=lambda **k: trk.detect_tracked_rois_device([0, 0], [0, 0], [0, 0], [0, -1], **k))
    finally:
        trk.close()


# ---------------------------------------------------------------------------------------------- 4. the prefix identity
@pytest.mark.parametrize("max_tracks", (16, 64))
def test_live_prefix_equals_the_plain_region_call(rfa, scene, max_tracks):
    """on a table whose live slots are exactly 0 .. L - 1 the call's out, counts and src_roi are the bytes rf_detect_roi_batch_device
    returns for rf_roi_from_faces of the `last` boxes at coord scale 1, the same margin and spec"""
    det = engine(rfa)
    big, small, own = scene
    dev = to_device([big])[0]
    for margin, grid in ((None, 4), (0.5, 2)):
        trk = det.tracker(1, max_tracks=max_tracks)
        try:
            det.detect_tracked_device([dev.data_ptr()], [896], [1280], trk, [0], 0.5)
            table = trk.read(0)[0]
            L = int((table["id"] != 0).sum())
            assert L >= 4 and (table["id"][:L] != 0).all()
            lasts = [np.frombuffer(t["last"].tobytes(), np.float32) for t in table[:L]]
            rois = rfa.rois_from_faces(lasts, 1.0, margin)
            assert len(rois) == L
            want, wv, ws = det.detect_rois_device([dev.data_ptr()], [896], [1280], [rois], 0.5, grid=grid, return_src_roi=True)
            wc = list(det.roi_counts)
            got, tags, ended, gv, gs = trk.detect_tracked_rois_device([dev.data_ptr()], [896], [1280], [0], 0.5, margin=margin, grid=grid,
                                                                      return_src_roi=True)
            assert got == want and det.roi_counts == wc and len(got[0]) >= 4
            assert np.array_equal(gs[0], ws[0]) and np.array_equal(gv[0], wv[0])
            assert np.array_equal(trk.last_cells[0][:L], rfa.roi_plan(rois, NET, NET, grid)[0]) and (trk.last_cells[0][L:, 7] == rtr.VOID).all()
        finally:
            trk.close()


# ---------------------------------------------------------------------------------------------- 5. neighbouring calls, shared blocks
def same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def test_tracked_region_call_between_tiled_and_region_calls(rfa, scene, base_frame):
    """one SPLIT3 handle (launches of eight over three lanes): a tracked region call of 32 passes (max_tracks 64 at grid 2, two frames)
    between a tiled call and a plain region call of 30 passes; each returns the bytes a fresh handle returns for it"""
    big, small, own = scene
    lists = [regions(small, [], 30)]
    dev = to_device([small, np.ascontiguousarray(base_frame[:600, :700]), big])

    def tracked(d):
        trk = d.tracker(2, max_tracks=64, max_missed=1)
        try:
            d.detect_tracked_device([dev[2].data_ptr(), dev[0].data_ptr()], [896, 200], [1280, 240], trk, [1, 0], 0.5)
            res = trk.detect_tracked_rois_device([dev[2].data_ptr(), dev[0].data_ptr()], [896, 200], [1280, 240], [1, 0], 0.5, grid=2, return_src_roi=True)
            return res + (trk.last_cells, trk.read(0)[0], trk.read(1)[0])
        finally:
            trk.close()
    calls = (lambda d: d.detect_tiled_device([dev[1].data_ptr()], [600], [700], 0.5, return_tiles=True),
             tracked,
             lambda d: d.detect_rois_device([dev[0].data_ptr()], [200], [240], lists, 0.5, grid=1, return_src_roi=True))
    fresh = []
    for call in calls:
        det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", **SPLIT3)
        try:
            fresh.append(call(det))
        finally:
            det.close()
    assert rr.passes_of(64, 2) * 2 == 32 and len(fresh[1][0][0]) >= 4
    det = engine(rfa, **SPLIT3)
    assert det.max_batch == 8 and det.num_slots() == 3
    for _ in range(2):
        for call, want in zip(calls, fresh):
            assert same(call(det), want)


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_change_nothing(rfa, scene):
    det = engine(rfa)
    big, small, own = scene
    dev = to_device([small])[0]
    trk = det.tracker(2, max_tracks=16, max_missed=1)
    shots, follow = det.tracker(1, max_tracks=4), det.tracker(1, max_tracks=4, follow=True)
    try:
        shots.enable_shots()
        det.detect_tracked_device([dev.data_ptr()], [200], [240], trk, [0], 0.5)
        before = [trk.read(s) for s in range(2)]
        assert (before[0][0]["id"] != 0).any()

        def unchanged():
            for s in range(2):
                t, f, nid = trk.read(s)
                assert t.tobytes() == before[s][0].tobytes() and (f, nid) == before[s][1:]
        one = ([dev.data_ptr()], [200], [240])
        two = ([dev.data_ptr()] * 2, [200] * 2, [240] * 2)
        bad_calls = [lambda kw=kw: trk.detect_tracked_rois_device(*one, [0], 0.5, **kw)
                     for kw in (dict(grid=3), dict(grid=-1), dict(max_zoom=3), dict(max_faces=4097), dict(max_faces=-1), dict(margin=-1 / 256),
                                dict(margin=256.0))]
        bad_calls += [lambda kw=kw: trk.detect_tracked_rois([small], [0], 0.5, **kw) for kw in (dict(grid=3), dict(margin=256.0))]
        bad_calls += [lambda kw=kw: trk.roi_cells([0], **kw) for kw in (dict(grid=3), dict(margin=256.0), dict(margin=-1 / 256))]
        bad_calls += [lambda: trk.detect_tracked_rois_device(*two, [0, 0], 0.5),                 # a stream twice
                      lambda: trk.roi_cells([1, 0, 1]),
                      lambda: trk.detect_tracked_rois_device(*one, [2], 0.5),                    # a stream out of range
                      lambda: trk.roi_cells([-2]),
                      lambda: trk.detect_tracked_rois_device(*one, [0], 0.5, steps=[719]),       # a short step
                      lambda: shots.detect_tracked_rois_device(*one, [0], 0.5),                  # a gallery, follow: they do not compose yet
                      lambda: shots.roi_cells([0]),
                      lambda: follow.detect_tracked_rois_device(*one, [0], 0.5),
                      lambda: follow.roi_cells([0])]
        for call in bad_calls:
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1
            unchanged()
        # a tracker of another handle, NULL arguments
        lib = det._lib
        other = engine(rfa, stem="mnet-deconv-0517")
        foreign = other.tracker(1, max_tracks=16)
        cnt, out, cells = (C.c_int * 1)(), (rfa._lib.rf_face * det.max_detections)(), (rfa._lib.rf_roi_cell * 16)()
        frames = (det._h, (C.c_void_p * 1)(dev.data_ptr()), (C.c_int * 1)(200), (C.c_int * 1)(240), None, 1, 0.5, None, 0)
        st0 = (C.c_int * 1)(0)
        try:
            assert lib.rf_detect_track_roi_batch_device(*frames, out, det.max_detections, cnt, None, None, None, None, foreign._t, st0, None, None, 0, None) == -1
            assert lib.rf_roi_track_cells_device(det._h, foreign._t, st0, 1, 0, None, cells) == -1
        finally:
            foreign.close()
        assert lib.rf_detect_track_roi_batch_device(*frames, out, det.max_detections, cnt, None, None, None, None, None, st0, None, None, 0, None) == -1
        assert lib.rf_detect_track_roi_batch_device(*frames, out, det.max_detections, cnt, None, None, None, None, trk._t, None, None, None, 0, None) == -1
        assert lib.rf_detect_track_roi_batch_device(*frames, None, det.max_detections, cnt, None, None, None, None, trk._t, st0, None, None, 0, None) == -1
        assert lib.rf_roi_track_cells_device(det._h, trk._t, st0, 1, 0, None, None) == -1
        unchanged()
        # a NULL spec, NULL steps and every optional output NULL: the defaults, and the call works
        assert lib.rf_detect_track_roi_batch_device(*frames, out, det.max_detections, cnt, None, None, None, None, trk._t, st0, None, None, 0, None) == 0
        assert cnt[0] >= 1 and trk.read(0)[1] == before[0][1] + 1
    finally:
        for t in (trk, shots, follow):
            t.close()


def test_multi_device_handles_refuse_tracked_region_detection(rfa, crop448):
    det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", devices=[0, 0])
    try:
        dev = to_device([crop448])[0]
        lib = det._lib
        cnt, out, cells = (C.c_int * 1)(), (rfa._lib.rf_face * 8)(), (rfa._lib.rf_roi_cell * 256)()
        st0 = (C.c_int * 1)(0)
        frames = (det._h, (C.c_void_p * 1)(dev.data_ptr()), (C.c_int * 1)(448), (C.c_int * 1)(448), None, 1, 0.5, None, 0)
        assert lib.rf_detect_track_roi_batch_device(*frames, out, 8, cnt, None, None, None, None, None, st0, None, None, 0, None) == -5
        host = (det._h, (C.c_void_p * 1)(crop448.ctypes.data), (C.c_int * 1)(448), (C.c_int * 1)(448), None, 1, 0.5, None, 0)
        assert lib.rf_detect_track_roi_batch(*host, out, 8, cnt, None, None, None, None, None, st0, None, None, 0, None) == -5
        assert lib.rf_roi_track_cells_device(det._h, None, st0, 1, 0, None, cells) == -5
        assert len(det.detect_device([dev.data_ptr()], [448], [448], 0.5)[0]) >= 1
    finally:
        det.close()


# ---------------------------------------------------------------------------------------------- 7. the C++ class
def test_cpp_class_detect_tracked_rois(rfa, scene, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_roi_track.cpp")
    exe = str(tmp_path / "test_roi_track")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    big, small, own = scene
    raw, out = str(tmp_path / "frame.raw"), str(tmp_path / "out.bin")
    big.tofile(raw)
    det = engine(rfa)
    for T, grid, vote, mq in ((16, 0, 0, 0), (17, 2, 1, 128)):
        r = subprocess.run([exe, ASSETS, "mnet25", "448", "448", raw, "896", "1280", "0.5", str(T), str(grid), str(vote), str(mq), out],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        blob = open(out, "rb").read()
        trk = det.tracker(2, max_tracks=T, max_missed=1)
        try:
            det.detect_tracked([big, big], trk, [0, 1], 0.5)
            pos = 0
            for call in range(2):
                want, wt, we, wv, ws = trk.detect_tracked_rois([big, None], [0, 1], 0.5, margin=mq / 256 if mq else None, grid=grid, vote=vote == 1,
                                                               return_src_roi=True)
                assert int(np.frombuffer(blob, np.int32, 1, pos)[0]) == 2
                pos += 4
                for i in range(2):
                    k = int(np.frombuffer(blob, np.int32, 1, pos)[0])
                    pos += 4
                    assert k == len(want[i]) and (i == 1 or k >= 4)
                    assert blob[pos:pos + 60 * k] == rows_of(want[i]).tobytes()
                    pos += 60 * k
                    assert list(np.frombuffer(blob, np.int32, k, pos)) == list(wv[i]) and list(np.frombuffer(blob, np.int32, k, pos + 4 * k)) == list(ws[i])
                    pos += 8 * k
                    assert blob[pos:pos + 24 * k] == wt[i].tobytes()
                    pos += 24 * k
                    e = int(np.frombuffer(blob, np.int32, 1, pos)[0])
                    pos += 4
                    assert e == len(we[i]) and blob[pos:pos + 176 * e] == we[i].tobytes() and (i == 0 or (e > 0) == (call == 1))
                    pos += 176 * e
                    assert int(np.frombuffer(blob, np.int32, 1, pos)[0]) == T
                    pos += 4
                    assert blob[pos:pos + 32 * T] == trk.last_cells[i].tobytes()
                    pos += 32 * T
            assert pos == len(blob)
        finally:
            trk.close()
