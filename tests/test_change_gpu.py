"""Change regions on the GPU: the two kernels against rf_change_step_host and tests/change_ref.py byte for byte on every case of
tests/test_change_host.py, pitched sources at odd addresses, streams side by side with a stream -1 image and a NULL frame between them;
the fused call against its own parts (ONE rf_detect_batch_device call over the reference's views + the reference's face rule, merge and
frame step), without a tracker and with a plain and a motion tracker; the identity with tracked region detection on a seeding step; and
the refusals, which change nothing."""
import numpy as np
import pytest

import change_ref as cr
import motion_ref as mr
import roi_ref as rr
import roi_track_ref as rtr
import track_ref as tr
from test_change_host import comb, paint_out, snake, spec_kw, spiral
from test_gpu_align import FP16, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_roi_track_gpu import check_state, key_call, ref_streams, void_cells
from test_tta_gpu import NET, NMS, odd_view

pytestmark = pytest.mark.gpu
ROWS, COLS = 896, 1280


def guarded(n_bytes):
    """a device buffer of n_bytes with 64 bytes of 0xAB on either side: (tensor, pointer of the body)"""
    import torch
    t = torch.full((n_bytes + 128,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t, t.data_ptr() + 64


def regions_guarded(det, chg, ptrs, rows, cols, streams, steps=None, margin=None, grid=0):
    """Changer.regions_device through the C entry point with 0xAB around both outputs: two records and two info records of sentinel
    in front of and behind the n * R cells and the n infos, all of which must come back untouched"""
    import ctypes as C
    from retinaface_amd import _lib
    from retinaface_amd.detector import _device_frames, _margin_q8, roi_spec
    n, R = len(ptrs), chg.max_regions
    cells, info = np.full((n * R + 4) * 32, 0xAB, np.uint8), np.full((n + 4) * 16, 0xAB, np.uint8)
    st = det._lib.rf_change_regions_device(det._h, chg._c, *_device_frames(ptrs, rows, cols, steps), (C.c_int * max(n, 1))(*streams), n,
                                           _margin_q8(margin), C.byref(roi_spec(grid)), C.cast(cells[64:].ctypes.data, C.POINTER(_lib.rf_roi_cell)),
                                           C.cast(info[32:].ctypes.data, C.POINTER(_lib.rf_change_info)))
    _lib.check(st, det._h)
    for a, lo, size in ((cells, 64, n * R * 32), (info, 32, n * 16)):
        assert (a[:lo] == 0xAB).all() and (a[lo + size:] == 0xAB).all()
    return cells[64:64 + n * R * 32].view(np.int32).reshape(n, R, 8).copy(), info[32:32 + n * 16].view(np.int32).reshape(n, 4).copy()


def read_guarded(det, chg, s):
    """Changer.read through the C entry point with 0xAB around the reference and the mask"""
    import ctypes as C
    nb = chg.bw * chg.bh
    ref, mask, frames = np.full(nb * 4 + 128, 0xAB, np.uint8), np.full(nb + 128, 0xAB, np.uint8), C.c_int64(-1)
    from retinaface_amd import _lib
    assert _lib.check(det._lib.rf_changer_read(chg._c, s, ref[64:].ctypes.data, C.byref(frames), mask[64:].ctypes.data), det._h) == nb
    for a, size in ((ref, nb * 4), (mask, nb)):
        assert (a[:64] == 0xAB).all() and (a[64 + size:] == 0xAB).all()
    return ref[64:64 + nb * 4].view(np.int32).reshape(chg.bh, chg.bw).copy(), int(frames.value), mask[64:64 + nb].reshape(chg.bh, chg.bw).copy()


def check_stream(rfa, chg, ref, s, host=None):
    """rf_changer_read of stream s against the reference stream (and the host state (ref, counter) stepped alongside)"""
    r, frames, mask = read_guarded(chg._det, chg, s)
    got = chg.read(s)
    assert np.array_equal(got[0], r) and got[1] == frames and np.array_equal(got[2], mask)
    assert frames == ref.frames and np.array_equal(r, ref.ref) and np.array_equal(mask, ref.mask), s
    if host is not None:
        assert np.array_equal(r, host[0]) and frames == host[1]


# ---------------------------------------------------------------------------------------------- 1. the kernels alone
def host_cases():
    iso = np.zeros((32, 32), np.uint8)
    iso[0::2, 0::2] = 1
    diag = np.zeros((6, 8), np.uint8)
    diag[1, 1] = diag[2, 2] = diag[4, 6] = diag[3, 7] = 1
    join = np.zeros((6, 8), np.uint8)
    join[0, 0] = join[0, 3] = join[5, 7] = 1
    ties = np.zeros((12, 16), np.uint8)
    ties[1, 1:4] = ties[5, 10:13] = ties[8, 2:7] = ties[3, 8:10] = 1
    ties[10, 14] = 1
    return {
        "diagonal": (diag, dict(block=8, dilate=2, min_blocks=1)),
        "spiral": (spiral(17), dict(block=8, dilate=2, min_blocks=1)),
        "snake": (snake(17), dict(block=8, dilate=2, min_blocks=1)),
        "comb": (comb(17), dict(block=8, dilate=2, min_blocks=1)),
        "spiral dilated": (spiral(17), dict(block=8)),
        "join off": (join, dict(block=8, dilate=2, min_blocks=1)),
        "join on": (join, dict(block=8, dilate=1, min_blocks=1)),
        "isolated": (iso, dict(block=8, dilate=2, min_blocks=1, max_regions=16)),
        "ties": (ties, dict(block=8, dilate=2, min_blocks=1)),
        "ties min 2": (ties, dict(block=8, dilate=2)),
        "ties min 3": (ties, dict(block=8, dilate=2, min_blocks=3)),
        "ties one": (ties, dict(block=8, dilate=2, min_blocks=1, max_regions=1)),
        "ties 64": (ties, dict(block=8, dilate=2, min_blocks=1, max_regions=64)),
        "whole frame": (np.ones((29, 37), np.uint8), dict()),
        "partial 16": (np.ones((3, 4), np.uint8), dict(block=16, min_blocks=1)),
    }


@pytest.mark.parametrize("name", sorted(host_cases()))
def test_masks_equal_the_host_code_and_the_reference(rfa, name):
    """seed on zeros, then the frame with 255 in the wanted blocks: cells, info and the changer's state against host and reference"""
    det = engine(rfa)
    mask, spec = host_cases()[name]
    B = spec.get("block", 16)
    rows, cols = mask.shape[0] * B - (5 if name == "partial 16" else 0), mask.shape[1] * B - (7 if name == "partial 16" else 0)
    ref = cr.Stream(rows, cols, **spec)
    chg = det.changer(rows, cols, 1, **spec)
    try:
        host = (np.zeros((ref.bh, ref.bw), np.int32), 0)
        check_stream(rfa, chg, ref, 0, host)
        for frame in cr.mask_frames(rows, cols, B, mask):
            dev = to_device([frame])[0]
            cells, info = regions_guarded(det, chg, [dev.data_ptr()], [rows], [cols], [0], grid=4)
            want = ref.step(frame, 0, NET, NET, 4)
            h = rfa.change_step_host(frame, host[0], host[1], NET, NET, spec_kw(ref), grid=4)
            host = (h[0], h[1])
            assert np.array_equal(cells[0], want[2]) and np.array_equal(cells[0], h[4]), (name, cells[0][:4], want[2][:4])
            assert np.array_equal(info[0], want[3]) and np.array_equal(info[0], h[5]), (name, info[0], want[3])
            check_stream(rfa, chg, ref, 0, host)
    finally:
        chg.close()


@pytest.mark.parametrize("shape", ((24, 40, 8), (29, 45, 8), (33, 33, 32), (33, 50, 16), (1024, 1024, 8), (70, 1100, 16)))
def test_random_frames_pitched_at_odd_addresses(rfa, shape):
    """random bytes, dense and as a pitched view at an odd address (every 16-byte chunk of a row is then cut differently); three
    streams in one call with a stream -1 image and a NULL frame between them; adapt_shift 0, 1 and 8; 0xAB around every output (the
    cells, the infos, the reference and the mask of rf_changer_read)"""
    det = engine(rfa)
    rows, cols, B = shape
    rng = np.random.default_rng(rows + cols)
    for a in ((0, 1, 8) if rows < 100 else (1,)):
        spec = dict(block=B, thr_q4=40, adapt_shift=a, min_blocks=1, max_regions=5)
        ref = [cr.Stream(rows, cols, **spec) for _ in range(3)]
        chg = det.changer(rows, cols, 3, **spec)
        try:
            for k in range(3):
                frames = [rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8) for _ in range(3)]
                if k == 2:
                    frames[0][: rows // 2] //= 4
                dense = to_device(frames)
                keep, optr, ostep = odd_view(frames[1])
                ptrs = [dense[0].data_ptr(), 0, optr, dense[2].data_ptr(), dense[2].data_ptr()]
                steps = [3 * cols, 0, ostep, 3 * cols, 3 * cols]
                streams = [2, -1, 0, -1, 1] if k else [2, 1, 0, -1, -1]               # stream 1: a NULL frame first, so it seeds one call later
                cells, info = regions_guarded(det, chg, ptrs, [rows, 0, rows, rows, rows], [cols, 0, cols, cols, cols], streams, steps=steps, margin=0.5, grid=2)
                for i, (s, f) in enumerate(zip(streams, (frames[0], None, frames[1], frames[2], frames[2]))):
                    if s < 0 or f is None:
                        assert np.array_equal(cells[i], void_cells(5)) and not info[i].any()
                        continue
                    want = ref[s].step(f, 128, NET, NET, 2)
                    assert np.array_equal(cells[i], want[2]) and np.array_equal(info[i], want[3]), (shape, a, k, i, info[i], want[3])
                for s in range(3):
                    check_stream(rfa, chg, ref[s], s)
            chg.reset(1)
            ref[1].reset()
            for s in range(3):
                check_stream(rfa, chg, ref[s], s)
        finally:
            chg.close()


def step_all(det, chg, ref, host, frame):
    """one step of the device, the reference and the host code on a dense frame; returns the device's (cells, info) and the host state"""
    rows, cols = frame.shape[:2]
    dev = to_device([frame])[0]
    cells, info = regions_guarded(det, chg, [dev.data_ptr()], [rows], [cols], [0])
    want = ref.step(frame, 0, NET, NET, 0)
    import retinaface_amd as rfa_mod
    h = rfa_mod.change_step_host(frame, host[0], host[1], NET, NET, spec_kw(ref))
    assert np.array_equal(cells[0], want[2]) and np.array_equal(cells[0], h[4]) and np.array_equal(info[0], want[3]) and np.array_equal(info[0], h[5])
    check_stream(None, chg, ref, 0, (h[0], h[1]))
    return info[0], (h[0], h[1]), chg.read(0)[2]


@pytest.mark.parametrize("shape", ((16, 16, 8, 0, 0), (17, 17, 8, 2, 2), (33, 33, 32, 1, 1)))
def test_threshold_exactly_and_one_unit_over_on_the_device(rfa, shape):
    """test_change_host.py's threshold cases: a full and a one-pixel block exactly at 16 * thr_q4 * npix (not marked) and one unit over
    (marked), with a positive and a negative difference; the kernel works npix out on its own"""
    det = engine(rfa)
    rows, cols, B, bx, by = shape
    spec = dict(block=B, thr_q4=16, dilate=2, min_blocks=1)
    base = np.full((rows, cols, 3), 100, np.uint8)
    at = base.copy()
    at[by * B:(by + 1) * B, bx * B:(bx + 1) * B] += 1
    over = at.copy()
    over[by * B, bx * B, 0] += 1
    under = base.copy()
    under[by * B:(by + 1) * B, bx * B:(bx + 1) * B] -= 1
    under[by * B, bx * B, 0] -= 1
    for second, marked in ((at, 0), (over, 1), (under, 1)):
        ref, chg = cr.Stream(rows, cols, **spec), det.changer(rows, cols, 1, **spec)
        try:
            host = (np.zeros((ref.bh, ref.bw), np.int32), 0)
            _, host, _ = step_all(det, chg, ref, host, base)
            info, host, mask = step_all(det, chg, ref, host, second)
            assert info[0] == marked and int(mask.sum()) == marked and (not marked or mask[by, bx] == 1)
        finally:
            chg.close()


def test_noise_marks_no_block_on_the_device(rfa):
    """+-2 of noise on both frames marks no block at the default threshold (|dS| <= 4 * 256 * npix < 8 * 256 * npix)"""
    det = engine(rfa)
    rng = np.random.default_rng(11)
    clean = rng.integers(2, 254, (45, 61, 3), dtype=np.uint8)
    ref, chg = cr.Stream(45, 61), det.changer(45, 61, 1)
    try:
        host = (np.zeros((ref.bh, ref.bw), np.int32), 0)
        for _ in range(3):
            noisy = (clean.astype(np.int16) + rng.integers(-2, 3, clean.shape)).astype(np.uint8)
            info, host, mask = step_all(det, chg, ref, host, noisy)
            assert info[0] == 0 and not mask.any()
    finally:
        chg.close()


# ---------------------------------------------------------------------------------------------- 2. the fused call against its own parts
def parts_of_call(det, trk_ref, chg_ref, frames, streams, thr, margin, grid, vote, max_faces):
    """The comparison target.  Per image with pixels: the track cells the reference plans from the tracker's reference stream (none
    without a tracker), then the change cells of the changer's reference stream, which steps; ONE plain call over the reference's
    views of all images in call order; roi_track_ref's face rule and merge; with a tracker the reference step."""
    md, R = det.max_detections, chg_ref[0].R
    T = trk_ref[0].spec.max_tracks if trk_ref else 0
    mq = 0 if margin is None else int(round(margin * 256))
    plans, infos, views = [], [], []
    for f, s in zip(frames, streams):
        cells, info = None, np.zeros(4, np.int32)
        if f is not None and s >= 0:
            tc = rtr.stream_cells(trk_ref[s], mq, NET, NET, grid, 0) if trk_ref else np.zeros((0, 8), np.int32)
            _, _, cc, info = chg_ref[s].step(f, mq, NET, NET, grid)
            cells = np.concatenate([tc, cc])
            views += list(rtr.atlas(f, cells, NET, NET, grid))
        plans.append(cells)
        infos.append(info)
    dev = to_device(views)
    res = det.detect_device([d.data_ptr() for d in dev], [NET] * len(dev), [NET] * len(dev), thr) if views else []
    assert not det.truncated
    out, q = [], 0
    PP = rr.passes_of(T + R, grid)
    none = (np.zeros((0, 15), np.float32), 0, np.zeros(0, np.int32), np.zeros(0, np.int32))
    for f, s, cells in zip(frames, streams, plans):
        merged, tags, ended = none, np.zeros(0, tr.TAG), np.zeros(0, tr.TRACK)
        if cells is not None:
            merged = rtr.merge(cells, [rows_of(x) for x in res[q:q + PP]], NET, NET, NMS, md, grid, vote, max_faces)[:4]
            q += PP
        if trk_ref and s >= 0:
            tags, ended, _ = rtr.step(trk_ref[s], merged[0], max_faces or md)
        out.append(tuple(merged) + (tags, ended, cells if cells is not None else void_cells(T + R)))
    assert q == len(res)
    return out, infos, views


def check_call(rfa, det, chg, chg_ref, trk, trk_ref, frames, streams, call, thr=0.5, margin=None, grid=4, vote=False, max_faces=0, views=None):
    want, infos, ref_views = parts_of_call(det, trk_ref, chg_ref, frames, streams, thr, margin, grid, vote, max_faces)
    res = call(tracker=trk, threshold=thr, margin=margin, grid=grid, vote=vote, max_faces=max_faces, return_src_roi=True)
    got, votes, src = res[0], res[-2], res[-1]
    for i, w in enumerate(want):
        faces, count, wv, ws, wt, we, wc = w
        assert det.roi_counts[i] == count and rows_of(got[i]).tobytes() == faces.tobytes(), (i, det.roi_counts[i], count)
        assert list(votes[i]) == list(wv) and list(src[i]) == list(ws), i
        assert np.array_equal(chg.last_cells[i], wc), (i, chg.last_cells[i], wc)
        assert np.array_equal(chg.last_info[i], infos[i]), (i, chg.last_info[i], infos[i])
        if trk is not None:
            assert res[1][i].tobytes() == wt.tobytes() and res[2][i].tobytes() == we.tobytes(), i
            assert trk.last_ended_counts[i] == len(we)
    assert not det.truncated
    if trk is not None:
        check_state(trk, trk_ref)
    for s in range(len(chg_ref)):
        check_stream(rfa, chg, chg_ref[s], s)
    if views is not None:
        have = views.cpu().numpy()
        body = have[64:64 + len(ref_views) * NET * NET * 3].reshape(len(ref_views), NET, NET, 3)
        assert all(np.array_equal(h, v) for h, v in zip(body, ref_views)) and (have[:64] == 0xAB).all() and (have[64 + body.size:] == 0xAB).all()
    return got, src, res


@pytest.fixture(scope="module")
def newcomer_frames(rfa, base_frame):
    """the base frame, and the base frame with its best-scoring face (of the plain call) painted out by its surroundings"""
    det = engine(rfa)
    faces = rows_of(det.detect(base_frame, 0.5))
    from tile_ref import frame_scale
    scale = float(frame_scale(ROWS, COLS, NET, NET))
    box = faces[0][1:5] * scale
    return base_frame, paint_out(base_frame, box)[0], box


@pytest.mark.parametrize("tracker", (None, "plain", "motion", "two passes"))
@pytest.mark.parametrize("stem", ("mnet25", "mnet-deconv-0517"))
def test_fused_call_equals_its_own_parts(rfa, newcomer_frames, stem, tracker):
    """a key call on the frame without the newcomer, a seeding call, then the frame with it: device frames with d_views, a NULL frame
    whose stream ages, a stream -1 image; vote on with host frames and a pitched frame.  max_tracks 10 with R = 6 at grid 4 is one
    pass, max_tracks 15 with R = 2 two."""
    det = engine(rfa, stem=stem)
    base, without, box = newcomer_frames
    T, R = (15, 2) if tracker == "two passes" else (10, 6)
    motion = (0.5, 8) if tracker == "motion" else None
    chg = det.changer(ROWS, COLS, 3, max_regions=R)
    chg_ref = [cr.Stream(ROWS, COLS, max_regions=R) for _ in range(3)]
    trk, trk_ref = None, None
    if tracker:
        kw = dict(max_tracks=T, max_missed=2, min_hits=1)
        trk = det.tracker(3, motion=dict(alpha=motion[0], horizon=motion[1]) if motion else None, **kw)
        trk_ref = ref_streams(3, motion, **kw)
    try:
        dev = to_device([base, without])
        if trk:
            key_call(det, trk, trk_ref, [dev[1], dev[1], dev[1]], [without] * 3, [0, 1, 2])
        PP = rr.passes_of((T if trk else 0) + R, 4)
        assert PP == (2 if tracker == "two passes" else 1)
        frames, streams = [without, None, without, without], [0, 1, -1, 2]
        ptrs, rows, cols = [dev[1].data_ptr(), 0, dev[1].data_ptr(), dev[1].data_ptr()], [ROWS, 0, ROWS, ROWS], [COLS, 0, COLS, COLS]
        got, src, res = check_call(rfa, det, chg, chg_ref, trk, trk_ref, frames, streams,
                                   call=lambda **k: chg.detect_changed_device(ptrs, rows, cols, streams, **k))
        assert (chg.last_info[[0, 3], 3] == 1).all() and not chg.last_info[[1, 2]].any()      # streams 0 and 2 seeded
        assert (chg.last_cells[:, -R:, 7] == cr.VOID).all()
        # the newcomer enters stream 0; stream 2 sees the same frame again; stream 1 seeds now
        frames, streams = [base, without, None, without], [0, 1, 2, -1]
        views, vptr = guarded(3 * PP * NET * NET * 3)
        ptrs = [dev[0].data_ptr(), dev[1].data_ptr(), 0, dev[1].data_ptr()]
        rows, cols = [ROWS, ROWS, 0, ROWS], [COLS, COLS, 0, COLS]
        got, src, res = check_call(rfa, det, chg, chg_ref, trk, trk_ref, frames, streams, views=views,      # two frames with pixels: 2 PP views
                                   call=lambda **k: chg.detect_changed_device(ptrs, rows, cols, streams, views_ptr=vptr, **k))
        info = chg.last_info
        assert info[0, 0] > 0 and info[0, 2] >= 1 and info[1, 3] == 1 and not info[2].any() and not info[3].any()
        Tn = T if trk else 0
        hit = [k for k, d in enumerate(got[0]) if tr.iou(rows_of([d])[0][1:5], box.astype(np.float32)) >= 0.5]
        assert len(hit) == 1 and int(src[0][hit[0]]) >= Tn                      # the newcomer: found by a change region
        if trk:
            tags = res[1][0]
            assert (tags["flags"][hit[0]] & tr.NEW) and int((tags["flags"] & tr.NEW != 0).sum()) == 1      # it opens the only new track
        # vote on, host frames, one of them pitched; stream 0 is quiet again, stream 1 gets the newcomer
        wide = np.zeros((ROWS, COLS * 3 + 7), np.uint8)
        pitched = wide[:, :COLS * 3].reshape(ROWS, COLS, 3)
        pitched[:] = base
        frames, streams = [base, pitched, None], [0, 1, 2]
        got, src, res = check_call(rfa, det, chg, chg_ref, trk, trk_ref, frames, streams, vote=True, margin=0.5,
                                   call=lambda **k: chg.detect_changed(frames, streams, **k))
        assert chg.last_info[0, 0] == 0 and chg.last_info[1, 0] > 0
    finally:
        chg.close()
        if trk:
            trk.close()


# ---------------------------------------------------------------------------------------------- 3. identity with tracked region detection
@pytest.mark.parametrize("motion", (None, (0.5, 8)))
def test_seeding_call_equals_the_tracked_region_call_on_a_twin(rfa, newcomer_frames, motion):
    """T + R <= grid^2: on a seeding step the change cells are void, so out, counts, src_roi, votes, tags and ended lists are those of
    rf_detect_track_roi_batch_device on a twin tracker, and the first T cell records are its records"""
    det = engine(rfa)
    base, without, _ = newcomer_frames
    kw = dict(max_tracks=10, max_missed=1, min_hits=1)
    mk = dict(alpha=motion[0], horizon=motion[1]) if motion else None
    a, b = det.tracker(2, motion=mk, **kw), det.tracker(2, motion=mk, **kw)
    chg = det.changer(ROWS, COLS, 2, max_regions=6)
    try:
        dev = to_device([base])
        for t in (a, b):
            det.detect_tracked_device([dev[0].data_ptr()], [ROWS], [COLS], t, [0], 0.5)
        ptrs, rows, cols, streams = [dev[0].data_ptr(), 0], [ROWS, 0], [COLS, 0], [0, 1]
        g1, t1, e1, v1, s1 = a.detect_tracked_rois_device(ptrs, rows, cols, streams, return_src_roi=True)
        c1 = list(det.roi_counts)
        g2, t2, e2, v2, s2 = chg.detect_changed_device(ptrs, rows, cols, streams, tracker=b, return_src_roi=True)
        assert list(det.roi_counts) == c1 and len(g1[0]) >= 4
        for i in range(2):
            assert rows_of(g1[i]).tobytes() == rows_of(g2[i]).tobytes() and list(v1[i]) == list(v2[i]) and list(s1[i]) == list(s2[i])
            assert t1[i].tobytes() == t2[i].tobytes() and e1[i].tobytes() == e2[i].tobytes()
            assert np.array_equal(chg.last_cells[i][:10], a.last_cells[i]) and (chg.last_cells[i][10:, 7] == cr.VOID).all()
        for s in range(2):
            assert a.read(s)[0].tobytes() == b.read(s)[0].tobytes()
        assert chg.read(0)[1] == 1 and chg.read(1)[1] == 0                         # the NULL frame did not touch its reference
    finally:
        chg.close()
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_change_nothing(rfa, newcomer_frames):
    det = engine(rfa)
    base, without, _ = newcomer_frames
    with pytest.raises(rfa.RFError):
        det.changer(1024, 1025, 1, block=8)                                          # 128 x 129 blocks
    for bad in (dict(block=4), dict(thr_q4=65536), dict(adapt_shift=9), dict(dilate=3), dict(max_regions=65)):
        with pytest.raises(rfa.RFError):
            det.changer(ROWS, COLS, 1, **bad)
    with pytest.raises(rfa.RFError):
        det.changer(ROWS, COLS, 0)
    chg = det.changer(ROWS, COLS, 2, max_regions=6)
    trk = det.tracker(2, max_tracks=10)
    three, big = det.tracker(3, max_tracks=10), det.tracker(2, max_tracks=251)
    shots, follow = det.tracker(2, max_tracks=10), det.tracker(2, max_tracks=10, follow=True)
    shots.enable_shots()
    ref = cr.Stream(ROWS, COLS, max_regions=6)
    try:
        dev = to_device([base, without, base[:448, :448]])
        p, small = dev[0].data_ptr(), dev[2].data_ptr()
        chg.detect_changed_device([dev[1].data_ptr()], [ROWS], [COLS], [0], tracker=trk)
        ref.step(without, 0, NET, NET, 4)
        state = [x.copy() if hasattr(x, "copy") else x for x in chg.read(0)]
        table = trk.read(0)[0].tobytes()

        def unchanged():
            now = chg.read(0)
            assert np.array_equal(now[0], state[0]) and now[1] == state[1] and np.array_equal(now[2], state[2]) and trk.read(0)[0].tobytes() == table
        calls = [dict(streams=[0, 0], n=2), dict(streams=[2]), dict(streams=[-2]), dict(margin=300.0), dict(grid=3), dict(tracker=three),
                 dict(tracker=big), dict(tracker=shots), dict(tracker=follow), dict(ptr=small, rows=448, cols=448)]
        for kw in calls:
            n = kw.get("n", 1)
            with pytest.raises(rfa.RFError):
                chg.detect_changed_device([kw.get("ptr", p)] * n, [kw.get("rows", ROWS)] * n, [kw.get("cols", COLS)] * n, kw.get("streams", [0]),
                                          tracker=kw.get("tracker", trk), margin=kw.get("margin"), grid=kw.get("grid", 0))
            unchanged()
        for kw in calls[:5] + calls[-1:]:
            n = kw.get("n", 1)
            with pytest.raises(rfa.RFError):
                chg.regions_device([kw.get("ptr", p)] * n, [kw.get("rows", ROWS)] * n, [kw.get("cols", COLS)] * n, kw.get("streams", [0]),
                                   margin=kw.get("margin"), grid=kw.get("grid", 0))
            unchanged()
        alien = engine(rfa, stem="mnet-deconv-0517").changer(ROWS, COLS, 2, max_regions=6)
        mine, chg._c = chg._c, alien._c                                              # a changer of another handle
        try:
            with pytest.raises(rfa.RFError):
                chg.regions_device([p], [ROWS], [COLS], [0])
        finally:
            chg._c = mine
            alien.close()
        unchanged()
        # and the changer still works
        cells, info = chg.regions_device([p], [ROWS], [COLS], [0])
        want = ref.step(base, 0, NET, NET, 4)
        assert np.array_equal(cells[0], want[2]) and np.array_equal(info[0], want[3]) and info[0, 0] > 0
    finally:
        for o in (chg, trk, three, big, shots, follow):
            o.close()


# ---------------------------------------------------------------------------------------------- 5. the C++ class
def test_cpp_class_detect_changed(rfa, newcomer_frames, tmp_path):
    """createChanger, detectChanged and changeRegions (tests/csrc/test_change.cpp) against the Python calls' bytes: a key call, a seeding call, the
    newcomer's call"""
    import os
    import subprocess
    from conftest import ASSETS, ROOT
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")                        # changeRegions takes device frames: the program calls hipMalloc
    src = os.path.join(ROOT, "tests", "csrc", "test_change.cpp")
    exe = str(tmp_path / "test_change")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir, "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib")])
    base, without, _ = newcomer_frames
    first, second, out = str(tmp_path / "first.raw"), str(tmp_path / "second.raw"), str(tmp_path / "out.bin")
    without.tofile(first)
    base.tofile(second)
    T, R = 10, 6
    r = subprocess.run([exe, ASSETS, "mnet25", "448", "448", first, second, str(ROWS), str(COLS), "0.5", str(T), str(R), out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    blob = open(out, "rb").read()
    det = engine(rfa)
    trk, chg = det.tracker(1, max_tracks=T), det.changer(ROWS, COLS, 1, max_regions=R)
    try:
        det.detect_tracked([without], trk, [0], 0.5)
        pos = 0
        for call, frame in enumerate((without, base)):
            want, wt, we, wv, ws = chg.detect_changed([frame], [0], tracker=trk, return_src_roi=True)
            k = int(np.frombuffer(blob, np.int32, 1, pos)[0])
            pos += 4
            assert k == len(want[0]) and k >= 4 + call
            assert blob[pos:pos + 60 * k] == rows_of(want[0]).tobytes()
            pos += 60 * k
            assert list(np.frombuffer(blob, np.int32, k, pos)) == list(wv[0]) and list(np.frombuffer(blob, np.int32, k, pos + 4 * k)) == list(ws[0])
            pos += 8 * k
            assert blob[pos:pos + 24 * k] == wt[0].tobytes()
            pos += 24 * k
            assert int(np.frombuffer(blob, np.int32, 1, pos)[0]) == T + R
            pos += 4
            assert blob[pos:pos + 32 * (T + R)] == chg.last_cells[0].tobytes()
            pos += 32 * (T + R)
            assert blob[pos:pos + 16] == chg.last_info[0].tobytes() and chg.last_info[0][3] == 1 - call
            pos += 16
        alone = det.changer(ROWS, COLS, 1, max_regions=R)
        try:
            for call, frame in enumerate((without, base)):
                dev = to_device([frame])[0]
                cells, info = alone.regions_device([dev.data_ptr()], [ROWS], [COLS], [0])
                assert int(np.frombuffer(blob, np.int32, 1, pos)[0]) == R
                pos += 4
                assert blob[pos:pos + 32 * R] == cells[0].tobytes() and blob[pos + 32 * R:pos + 32 * R + 16] == info[0].tobytes()
                pos += 32 * R + 16
                assert info[0][3] == 1 - call and (call == 0 or info[0][0] > 0)
        finally:
            alone.close()
        assert pos == len(blob)
    finally:
        trk.close()
        chg.close()
