"""Zoom-pyramid detection on the GPU: the zoom kernel against tests/pyramid_ref.zoom, the gather and voting merge kernels against
tests/pyramid_ref.py byte for byte on constructed faces (no forward pass), the fused call against its own parts (ONE
rf_detect_batch_device call over the 1x views and host-made zoom tiles of all frames + the reference merge), the levels = 1 invariant
against the tiled call, the refusals, the mosaic end to end against the oracle's golden, and the C++ class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyramid_ref as pr
import tile_ref
from conftest import ASSETS, ROOT, golden
from test_face_aa_gpu import roi_view
from test_gpu_align import FP16, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_pyramid_host import ZOOM_SHAPES, in_zoom, noise, windows
from test_tta_gpu import BIG, INT8, MD, NMS, SPLIT2, SPLIT3, big_engine, odd_view, score31
from test_tta_host import face, quarter

pytestmark = pytest.mark.gpu

NET = 448


# ---------------------------------------------------------------------------------------------- 1. the zoom kernel
def check_zoom(det, frame, z, wins, sources):
    import torch
    rows, cols = frame.shape[:2]
    for x0, y0, tw, th in wins:
        want = pr.zoom(frame, z, x0, y0, tw, th)
        for sptr, sstep in sources:
            for pad, shift in ((0, 0), (5, 0), (7, 1), (2, 3)):          # dense; pitched destinations, some at odd pointers
                dstep = 3 * tw + pad
                dst = torch.full((th * dstep + 8,), 0xAB, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                det.zoom_device(sptr, rows, cols, z, x0, y0, tw, th, dst.data_ptr() + shift, step=sstep, dst_step=dstep)
                got = dst.cpu().numpy()
                body = got[shift:shift + th * dstep].reshape(th, dstep)
                assert np.array_equal(body[:, :3 * tw].reshape(th, tw, 3), want), (frame.shape, z, x0, y0, tw, th, pad, shift)
                assert (body[:, 3 * tw:] == 0xAB).all() and (got[:shift] == 0xAB).all() and (got[shift + th * dstep:] == 0xAB).all()


@pytest.mark.parametrize("z", (2, 4))
def test_zoom_device_equals_the_reference(rfa, z):
    det = engine(rfa)
    for rows, cols in ZOOM_SHAPES:
        frame = noise(rows, cols)
        dense = to_device([frame])[0]
        keep, rptr, rstep = odd_view(frame)
        sources = ((dense.data_ptr(), 3 * cols), (rptr, rstep))
        wins = windows(rows, cols, z)
        check_zoom(det, frame, z, wins if rows < 100 else wins[:3] + wins[-3:], sources)
        if (rows, cols) == (113, 161) and z == 4:                        # widths around the four-pixel groups and the net's
            check_zoom(det, frame, z, [(x0, 5, tw, 3) for tw in (1, 2, 3, 4, 5, 447, 448) for x0 in (0, 3, 644 - tw)], sources)
        if (rows, cols) == (113, 161) and z == 2:
            check_zoom(det, frame, z, [(x0, 220, tw, 6) for tw in (1, 2, 3, 4, 5) for x0 in (0, 2, 322 - tw)], sources)


def test_zoom_device_of_a_frame_of_many_workgroups_and_refusals(rfa, base_frame):
    import torch
    det = engine(rfa)
    frame = np.ascontiguousarray(base_frame[30:478, 440:888])
    dev = to_device([base_frame])[0]
    dst = torch.zeros((448 * 448 * 3,), dtype=torch.uint8, device="cuda")
    for z, x0, y0 in ((2, 0, 0), (2, 448, 448), (4, 1344, 671)):        # tiles of the enlarged crop, read through a pitched view
        det.zoom_device(dev.data_ptr() + 30 * 3840 + 3 * 440, 448, 448, z, x0, y0, 448, 448, dst.data_ptr(), step=3840)
        assert np.array_equal(dst.cpu().numpy().reshape(448, 448, 3), pr.zoom(frame, z, x0, y0, 448, 448)), (z, x0, y0)
    ok = dict(src_ptr=dev.data_ptr(), rows=896, cols=1280, z=2, x0=0, y0=0, tw=448, th=448, dst_ptr=dst.data_ptr())
    for bad in (dict(z=1), dict(z=3), dict(z=8), dict(x0=-1), dict(y0=-1), dict(x0=2560 - 447), dict(y0=1792 - 447), dict(dst_step=3 * 448 - 1),
                dict(step=3 * 1280 - 1), dict(dst_ptr=0), dict(src_ptr=0), dict(tw=-1)):
        with pytest.raises(rfa.RFError) as e:
            det.zoom_device(**dict(ok, **bad))
        assert e.value.status == -1, bad
    det.zoom_device(**dict(ok, x0=2560 - 448, y0=1792 - 448))           # the last window of the enlarged frame is legal
    assert np.array_equal(dst.cpu().numpy().reshape(448, 448, 3), pr.zoom(base_frame, 2, 2560 - 448, 1792 - 448, 448, 448))


# ---------------------------------------------------------------------------------------------- 2. merge with constructed faces
SMALL = (100, 112)            # every level of `levels = 7` is one tile: nothing is dropped, the candidates are the faces
MOSAIC = (336, 480)


def to_pass(f, p):
    """the face of pass p (z, x0, y0, ...) that maps to the frame-space face f (quarter-pixel coordinates: exact)"""
    z, x0, y0 = int(p[0]), int(p[1]), int(p[2])
    g = in_zoom(f, z) if z > 1 else f.copy()
    g[[1, 3, 5, 6, 7, 8, 9]] -= np.float32(x0)
    g[[2, 4, 10, 11, 12, 13, 14]] -= np.float32(y0)
    return g


def deal(faces, shape=SMALL, levels=7, md=BIG):
    """frame-space faces dealt in turn over the passes of the plan (through the inverse mapping), each pass in score order"""
    plan = pr.plan(*shape, NET, NET, levels)
    if shape == SMALL:
        assert len(plan) == bin(levels).count("1")
    passes = [[] for _ in plan]
    full = [pr.is_full(p, *shape, NET, NET) for p in plan]
    for j, f in enumerate(faces):
        k = j % len(plan)
        if full[k]:
            k = (k + 1) % len(plan)
        passes[k].append(to_pass(f, plan[k]))
    out = []
    for ps in passes:
        ps = sorted(ps, key=lambda f: -f[0])
        assert len(ps) <= md
        out.append(np.stack(ps).astype(np.float32) if ps else np.zeros((0, 15), np.float32))
    return out


def mixed_faces(seed, want, span=40):
    """`want` faces: places that hold one to six faces around one spot, every fifth place a chain, scores from 31 values"""
    rng = np.random.default_rng(seed)
    faces, j = [], 0
    while len(faces) < want:
        x, y = 10.0 + 70 * (j % span), 10.0 + 60 * (j // span)
        if j % 5 == 4:
            group = [quarter(face(x + 15 * k, y, 40, 40, score31(rng))) for k in range(3)]
        else:
            group = [quarter(face(x + float(rng.uniform(-4, 4)), y + float(rng.uniform(-4, 4)), 40, 44, score31(rng))) for _ in range(int(rng.integers(1, 7)))]
        faces += group[:want - len(faces)]
        j += 1
    return faces


def check_merge_call(det, frames, md=BIG, levels=7, **kw):
    """frames: (rows, cols, passes); one rf_pyramid_merge_device call against pyramid_ref per frame, byte for byte"""
    rows, cols = [f[0] for f in frames], [f[1] for f in frames]
    dets, votes, src = det.pyramid_merge(rows, cols, [f[2] for f in frames], levels=levels, return_votes=True, **kw)
    counts = list(det.pyramid_counts)
    limit = min(kw.get("max_faces", 0) or md, kw.get("cap_per_image", md))
    assert det.truncated == any(c > limit for c in counts)
    ncand = []
    for i, (r, c, passes) in enumerate(frames):
        want = pr.merge(r, c, passes, NET, NET, NMS, md, levels, kw.get("overlap", 0), kw.get("edge", 0), True, kw.get("max_faces", 0),
                        kw.get("vote", True))
        assert counts[i] == want[1], (i, counts[i], want[1], want[4])
        assert rows_of(dets[i]).tobytes() == want[0][:limit].tobytes(), (i, want[4])
        assert list(votes[i]) == list(want[2][:limit]) and list(src[i]) == list(want[3][:limit]), i
        ncand.append(want[4])
    return dets, votes, src, counts, ncand


def test_merge_of_constructed_faces_equals_the_reference(rfa):
    det = big_engine(rfa)
    assert det.max_detections == BIG
    made = {}

    def frame(want, seed, shape=SMALL, levels=7):
        if (want, seed) not in made:
            made[(want, seed)] = shape + (deal(mixed_faces(seed, want), shape, levels),)
        return made[(want, seed)]
    # the three sort regimes and their boundaries, three frames per call
    calls = ([frame(0, 1), frame(1, 2), frame(65, 3)], [frame(257, 4), frame(1000, 5), frame(64, 6)])
    for frames in calls:
        dets, votes, src, counts, ncand = check_merge_call(det, frames)
        assert ncand == [sum(len(p) for p in f[2]) for f in frames]                    # single-tile levels drop nothing
        again = det.pyramid_merge([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], levels=7, return_votes=True)
        assert again[0] == dets and all(np.array_equal(a, b) for a, b in zip(again[1], votes))      # the counters re-armed, no order leaks
    r, c, passes = frame(1000, 5)
    want = pr.merge(r, c, passes, NET, NET, NMS, BIG, 7)
    assert want[2].max() >= 5 and (want[2] == 1).any() and set(want[3].tolist()) == {0, 1, 2}          # clusters across all three levels
    # vote off: the detector's greedy NMS on the same candidates
    dets, votes, src, counts, _ = check_merge_call(det, [frame(1000, 5), frame(257, 4)], vote=False)
    cand, g = pr.candidates(r, c, passes, NET, NET, BIG, 7)
    assert rows_of(dets[0]).tobytes() == cand[tile_ref.nms(cand, g, NMS)].tobytes()
    # a smaller max_faces and a smaller cap_per_image: counts stay true
    check_merge_call(det, [frame(257, 4), frame(1000, 5)], max_faces=7)
    assert det.truncated
    check_merge_call(det, [frame(65, 3)], cap_per_image=5)
    assert det.truncated and det.pyramid_counts[0] > 5
    # the mosaic's plan (two 1x tiles, a full-frame pass that gets nothing here, six 2x tiles): the edge rule drops faces on the device
    # as in the reference, at several band widths; an empty frame in the call
    spread = [quarter(face(float(x), float(y), 14, 16, score31(np.random.default_rng(x * 7 + y)))) for x in range(2, 470, 13) for y in range(2, 320, 29)]
    tiled = MOSAIC + (deal(spread, MOSAIC, 3),)
    for edge in (0, -1, 30):
        _, _, _, counts, ncand = check_merge_call(det, [tiled, (0, 0, [np.zeros((0, 15), np.float32)])], levels=3, edge=edge)
        assert 0 < ncand[0] < len(spread) and counts[1] == 0


def test_merge_overflow_is_reported_and_leaves_the_other_frame_exact(rfa):
    det = big_engine(rfa)
    rng = np.random.default_rng(9)
    grid = [quarter(face(3.0 + 10 * (j % 64), 3.0 + 10 * (j // 64), 5.5, 6.25, score31(rng))) for j in range(4500)]
    big = SMALL + (deal(grid),)
    assert sum(len(p) for p in big[2]) == 4500 > pr.MERGE_CAP
    other = SMALL + (deal(mixed_faces(11, 300)),)
    want = pr.merge(*SMALL, other[2], NET, NET, NMS, BIG, 7)
    for order in ((0, 1), (1, 0)):
        frames = [[big, other][k] for k in order]
        dets, votes, src = det.pyramid_merge([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], levels=7, return_votes=True)
        assert det.truncated
        i = order.index(1)
        assert det.pyramid_counts[i] == want[1] and rows_of(dets[i]).tobytes() == want[0].tobytes()
        assert list(votes[i]) == list(want[2]) and list(src[i]) == list(want[3])
    check_merge_call(det, [other])                         # the counters were re-armed: the next call is exact


# ---------------------------------------------------------------------------------------------- 3. fused call against its own parts
@pytest.fixture(scope="module")
def scenes(base_frame):
    """(name, pixels): the mosaic, a 50 x 70 piece of it (single-tile levels), a 500 x 700 window of the base frame (oversize)"""
    mosaic = pr.mosaic(base_frame)
    return {"mosaic": mosaic, "small": np.ascontiguousarray(mosaic[20:70, 10:80]), "big": np.ascontiguousarray(base_frame[0:500, 400:1100])}


def parts_of_call(det, frames, thr=0.5, md=MD, levels=0, **kw):
    """frames: (ptr, rows, cols, step, pixels) of one pyramid call (ptr 0: an empty frame).  pyramid_ref.merge, per frame, over what
    ONE rf_detect_batch_device call returns for the passes of all frames in plan order -- the call the engine itself makes: 1x passes
    as ROI views of the caller's frame, zoom tiles made on the host and uploaded densely."""
    plans = [pr.plan(r if ptr else 0, c if ptr else 0, det.net_h, det.net_w, levels, kw.get("overlap", 0), kw.get("full_frame", True))
             for ptr, r, c, _, _ in frames]
    tiles = to_device([pr.zoom(f[4], int(p[0]), *(int(v) for v in p[1:])) for f, plan in zip(frames, plans) if f[0] for p in plan if p[0] > 1])
    ptrs, rows, cols, steps, at = [], [], [], [], 0
    for (ptr, r, c, st, _), plan in zip(frames, plans):
        for z, x0, y0, tw, th in (tuple(int(v) for v in p) for p in plan):
            if not ptr:
                ptrs.append(0); rows.append(0); cols.append(0); steps.append(0)
            elif z == 1:
                ptrs.append(ptr + y0 * st + 3 * x0); rows.append(th); cols.append(tw); steps.append(st)
            else:
                ptrs.append(tiles[at].data_ptr()); rows.append(th); cols.append(tw); steps.append(3 * tw)
                at += 1
    res = det.detect_device(ptrs, rows, cols, thr, steps=steps)
    assert not det.truncated
    out, q = [], 0
    for (ptr, r, c, _, _), plan in zip(frames, plans):
        passes = [rows_of(x) for x in res[q:q + len(plan)]]
        q += len(plan)
        out.append((pr.merge(r, c, passes, det.net_h, det.net_w, NMS, md, levels, kw.get("overlap", 0), kw.get("edge", 0),
                             kw.get("full_frame", True), kw.get("max_faces", 0), kw.get("vote", True)) if ptr else None, passes))
    return out


def check_pyr(got, votes, src, counts, i, want):
    if want is None:
        assert got[i] == [] and counts[i] == 0
        return
    assert counts[i] == want[1] and rows_of(got[i]).tobytes() == want[0].tobytes(), (i, counts[i], want[1])
    assert list(votes[i]) == list(want[2]) and list(src[i]) == list(want[3]), i


def run_and_check(det, frames, **kw):
    want = parts_of_call(det, frames, **kw)
    got, votes, src = det.detect_pyramid_device([f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], 0.5,
                                                steps=[f[3] for f in frames], return_votes=True, **kw)
    assert not det.truncated
    for i in range(len(frames)):
        check_pyr(got, votes, src, det.pyramid_counts, i, want[i][0])
    return got, votes, src, want


@pytest.mark.parametrize("prec,kw", ((FP16, {}), (FP16, SPLIT2), (FP16, SPLIT3), (INT8, {})))
def test_fused_call_equals_the_merge_of_its_own_passes(rfa, scenes, prec, kw):
    """kw = {}: the whole call is one coalesced launch.  SPLIT2 / SPLIT3: the passes cross launches and lanes -- the merge waits for
    the other lanes' gathers on the device, and every lane waits for the zoom kernels."""
    det = engine(rfa, prec=prec, **kw)
    if kw:
        assert det.max_batch == 8 and det.num_slots() == kw["lanes"]
    dev = {k: to_device([v])[0] for k, v in scenes.items()}
    fr = {k: (dev[k].data_ptr(), v.shape[0], v.shape[1], 3 * v.shape[1], v) for k, v in scenes.items()}
    plain = det.detect_device([fr["mosaic"][0]], [336], [480], 0.5)
    # the mosaic: 9 passes; with the small and the oversize frame: 9 + 2 + 17 passes in one call
    got, votes, src, want = run_and_check(det, [fr["mosaic"]])
    assert len(got[0]) > len(plain[0]) and int(votes[0].max()) >= 2 and 2 in set(pr.plan(336, 480, NET, NET)[src[0], 0].tolist())
    allg, allv, alls, _ = run_and_check(det, [fr["mosaic"], fr["small"], fr["big"]])
    assert len(pr.plan(50, 70, NET, NET)) == 2 and len(pr.plan(500, 700, NET, NET)) == 4 + 1 + 12
    assert len(allg[2]) >= 2
    # repeats give identical bytes
    for _ in range(2):
        again = det.detect_pyramid_device([fr["mosaic"][0]], [336], [480], 0.5, return_votes=True)
        assert again[0] == got and all(np.array_equal(a, b) for a, b in zip(again[1], votes))
    # 1x and 4x only; vote off; a smaller max_faces; an empty frame in the batch
    run_and_check(det, [fr["small"], fr["mosaic"]], levels=5)
    off = run_and_check(det, [fr["mosaic"]], vote=False)[0]
    assert [d.score for d in off[0]] == [d.score for d in got[0]] and off != got                        # voting moved boxes, not heads
    run_and_check(det, [fr["small"], (0, 0, 0, 0, None), fr["mosaic"]])
    cut = det.detect_pyramid_device([fr["mosaic"][0]], [336], [480], 0.5, max_faces=3)
    assert det.truncated and det.pyramid_counts == [len(got[0])] and cut[0] == got[0][:3]
    assert det.detect_device([fr["mosaic"][0]], [336], [480], 0.5) == plain                             # the ordinary call is what it was
    if prec != FP16:
        return
    # a pitched ROI view at an odd pointer with an odd step
    keep, rptr, rstep = roi_view(scenes["mosaic"])
    run_and_check(det, [(rptr, 336, 480, rstep, scenes["mosaic"]), fr["small"]])
    # host frames: uploaded once, densely; an empty frame in between
    hgot, hvotes, hsrc = det.detect_pyramid([scenes["mosaic"], None, scenes["small"]], 0.5, return_votes=True)
    hwant = parts_of_call(det, [fr["mosaic"], (0, 0, 0, 0, None), fr["small"]])
    for i in range(3):
        check_pyr(hgot, hvotes, hsrc, det.pyramid_counts, i, hwant[i][0])
    assert det.detect_device([fr["mosaic"][0]], [336], [480], 0.5) == plain


@pytest.mark.parametrize("kw", ({}, SPLIT2))
def test_levels_1_without_vote_is_the_tiled_call(rfa, scenes, base_frame, kw):
    det = engine(rfa, **kw)
    frames = [base_frame, scenes["big"], scenes["mosaic"], scenes["small"]]
    dev = to_device(frames)
    args = ([d.data_ptr() for d in dev], [f.shape[0] for f in frames], [f.shape[1] for f in frames], 0.5)
    for spec in (dict(), dict(overlap=128, edge=-1, full_frame=False, max_faces=5)):
        tiled, tsrc = det.detect_tiled_device(*args, return_tiles=True, **spec)
        tcounts, ttr = list(det.tiled_counts), det.truncated
        got, votes, src = det.detect_pyramid_device(*args, levels=1, vote=False, return_votes=True, **spec)
        assert got == tiled and [rows_of(g).tobytes() for g in got] == [rows_of(t).tobytes() for t in tiled]
        assert det.pyramid_counts == tcounts and det.truncated == ttr and all(list(a) == list(b) for a, b in zip(src, tsrc))
    assert 0 < len(tiled[0]) <= 5


# ---------------------------------------------------------------------------------------------- 4. refusals
def pyr_calls(det, ptr, spec_kw):
    return (lambda: det.detect_pyramid_device([ptr], [448], [448], 0.5, **spec_kw),
            lambda: det.detect_pyramid([np.zeros((448, 448, 3), np.uint8)], 0.5, **spec_kw),
            lambda: det.pyramid_merge([100], [112], [[np.zeros((0, 15), np.float32)] * 2], **spec_kw))


def test_bad_specs_are_refused_and_leave_the_handle_usable(rfa, crop448):
    det = engine(rfa)
    dev = to_device([crop448])[0]
    before = det.detect_pyramid_device([dev.data_ptr()], [448], [448], 0.5)
    plain = det.detect_device([dev.data_ptr()], [448], [448], 0.5)
    for bad in (dict(max_faces=4097), dict(max_faces=-1), dict(levels=8), dict(levels=-1), dict(overlap=448), dict(edge=224)):
        for call in pyr_calls(det, dev.data_ptr(), bad):
            with pytest.raises((rfa.RFError, ValueError)) as e:
                call()
            assert getattr(e.value, "status", -1) == -1, bad
    cnt, out = (C.c_int * 1)(), (rfa._lib.rf_face * MD)()
    args = (det._h, (C.c_void_p * 1)(dev.data_ptr()), (C.c_int * 1)(448), (C.c_int * 1)(448), (C.c_int * 1)(1344), 1, 0.5)
    for field, value in (("struct_size", 24), ("struct_size", 20), ("vote", 3), ("vote", -1), ("full_frame", 3)):
        sp = rfa.pyramid_spec()
        setattr(sp, field, value)
        assert det._lib.rf_detect_pyramid_batch_device(*args, C.byref(sp), out, MD, cnt, None, None) == -1, field
    assert det._lib.rf_detect_pyramid_batch_device(*args, None, None, MD, cnt, None, None) == -1          # out is null
    assert det._lib.rf_detect_pyramid_batch_device(*args, None, out, MD, cnt, None, None) == 0 and cnt[0] == len(before[0])   # a NULL spec
    # a frame whose plan has more than 1024 passes is refused before anything runs: 4x of 3000 x 4000 is 48 x 36 tiles.  (At this net
    # 1024 tiles of 448 x 448 x 3 bytes stay below the 1 GiB cap on the zoom tiles, so only this refusal can be reached here;
    # tests/test_pyramid_host.py reaches the other at a 1024 x 1024 net.)
    big = (C.c_int * 1)(3000), (C.c_int * 1)(4000), (C.c_int * 1)(12000)
    sp = rfa.pyramid_spec(levels=4)
    assert det._lib.rf_detect_pyramid_batch_device(det._h, args[1], big[0], big[1], big[2], 1, 0.5, C.byref(sp), out, MD, cnt, None, None) == -1
    assert det.detect_pyramid_device([dev.data_ptr()], [448], [448], 0.5) == before and len(before[0]) >= 2
    assert det.detect_device([dev.data_ptr()], [448], [448], 0.5) == plain


def test_multi_device_handles_refuse_the_pyramid(rfa, crop448):
    det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", devices=[0, 0])
    try:
        dev = to_device([crop448])[0]
        for call in pyr_calls(det, dev.data_ptr(), {}) + (lambda: det.zoom_device(dev.data_ptr(), 448, 448, 2, 0, 0, 448, 448, dev.data_ptr()),):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -5
        assert len(det.detect_device([dev.data_ptr()], [448], [448], 0.5)[0]) >= 1
    finally:
        det.close()


# ---------------------------------------------------------------------------------------------- 5. the mosaic against the oracle
@pytest.mark.parametrize("stem", ("mnet25", "mnet-deconv-0517"))
def test_mosaic_finds_the_oracles_faces(rfa, scenes, stem):
    """tools/make_pyramid_golden.py chose the threshold (0.5 for both stems: the oracle's merge gives 54 faces and no anchor of any of
    the nine passes lies inside the fp16 score-noise band around it), so every oracle face is asserted, none is set aside."""
    g = golden("pyramid_mosaic.npz")
    thr, want = float(g[stem + "/threshold"]), g[stem + "/faces"]
    assert int(g[stem + "/in_band"]) == 0 and len(want) == 54 and int(g[stem + "/pass_counts"].sum()) == len(g[stem + "/scores"])
    det = engine(rfa, stem=stem)
    got = rows_of(det.detect_pyramid([scenes["mosaic"]], thr)[0])
    plain = det.detect(scenes["mosaic"], thr)
    print(stem, "pyramid faces", len(got), "plain faces", len(plain), "threshold", thr)
    iou = np.array([[tile_ref.iou_plus1(w[1:5], f[1:5]) for f in got] for w in want])
    print(stem, "worst best-IoU of an oracle face", float(iou.max(axis=1).min()) if len(got) else None)
    assert len(got) == 54 and len(plain) < 54
    best = iou.argmax(axis=1)
    assert (iou.max(axis=1) >= 0.5).all() and len(set(best.tolist())) == 54             # one to one, no extra face


# ---------------------------------------------------------------------------------------------- 6. the C++ class
def test_cpp_class_detect_pyramid(rfa, scenes, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_pyramid.cpp")
    exe = str(tmp_path / "test_pyramid")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    raw, out = str(tmp_path / "frame.raw"), str(tmp_path / "out.bin")
    frame = scenes["mosaic"]
    frame.tofile(raw)
    det = engine(rfa)
    for levels, vote, mf in ((0, 1, 0), (5, 2, 7), (1, 0, 0)):
        r = subprocess.run([exe, ASSETS, "mnet25", "448", "448", raw, "336", "480", "0.5", str(levels), str(vote), str(mf), out],
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
        want, wv, ws = det.detect_pyramid([frame, None, frame], 0.5, levels=levels, vote=vote != 2, max_faces=mf, return_votes=True)
        assert len(faces[0]) > 0 and len(faces[1]) == 0 and (not mf or len(faces[0]) == mf)
        for i in range(n):
            assert faces[i].tobytes() == rows_of(want[i]).tobytes() and list(votes[i]) == list(wv[i]) and list(srcs[i]) == list(ws[i]), i
