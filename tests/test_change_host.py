"""Change regions on the host: rf_change_step_host (change.h, the code the two kernels run) against tests/change_ref.py byte for
byte -- block sums, the threshold, the reference update, the components and their selection, the refusals -- the claim (a face that
appears between two key frames is found from the change regions, and gets its id in the frame it appears in) end to end through the
CPU oracle, and change.h with roi.h on their own under the address and UB sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import change_ref as cr
import roi_ref as rr
import roi_track_ref as rtr
import track_ref as tr
from conftest import ROOT
from retinaface_amd import ROI_CROPPED, TRACK_DTYPE, _lib, change_spec, change_step_host, roi_atlas_host, roi_cells_from_tracks, track_step

NET, NMS = 448, 0.4


def spec_kw(s):
    return dict(block=s.B, thr_q4=s.thr, adapt_shift=s.a, dilate=1 if s.dilate else 2, min_blocks=s.min_blocks, max_regions=s.R)


def pitched(frame, extra=7, lead=1):
    """the frame at an odd address with a row pitch of cols * 3 + extra, 0xAB around its rows"""
    rows, cols = frame.shape[:2]
    step = cols * 3 + extra
    buf = np.full(lead + rows * step, 0xAB, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[lead:], (rows, cols, 3), (step, 3, 1))
    view[:] = frame
    return buf, view


def both(s, ref, counter, frame, margin_q8=0, grid=0, max_zoom=0, src=None):
    """one step of the reference stream `s` and of rf_change_step_host from (ref, counter): every output compared; the new (ref, counter)"""
    want = s.step(frame, margin_q8, NET, NET, grid, max_zoom)
    got = change_step_host(frame if src is None else src, ref, counter, NET, NET, spec_kw(s), None if not margin_q8 else margin_q8 / 256, grid,
                           max_zoom)
    assert got[1] == s.frames and np.array_equal(got[0], s.ref) and got[0].dtype == np.int32
    for g, w, name in zip(got[2:], want, ("mask", "regions", "cells", "info")):
        assert g.shape == w.shape and np.array_equal(g, w), (name, g, w)
    return got[0], got[1], got


def run_mask(rows, cols, mask, margin_q8=0, grid=0, **spec):
    """seed on zeros, then the frame with 255 in the blocks of `mask`; returns the second step's outputs"""
    s = cr.Stream(rows, cols, **spec)
    seed, frame = cr.mask_frames(rows, cols, s.B, mask)
    ref, cnt, out = both(s, np.zeros((s.bh, s.bw), np.int32), 0, seed, margin_q8, grid)
    assert list(out[5]) == [0, 0, 0, 1] and not out[2].any() and (out[4][:, 7] == cr.VOID).all()
    _, _, out = both(s, ref, cnt, frame, margin_q8, grid)
    assert np.array_equal(out[2], np.asarray(mask, np.uint8))
    return out


def test_struct_sizes():
    assert C.sizeof(_lib.rf_change_spec) == 32 and C.sizeof(_lib.rf_change_info) == 16


# ---------------------------------------------------------------------------------------------- 1. shapes and sums
@pytest.mark.parametrize("shape", ((24, 40, 8), (29, 45, 8), (33, 33, 32), (33, 50, 16)))
def test_random_frames_at_full_and_partial_blocks(shape):
    rows, cols, B = shape
    rng = np.random.default_rng(rows * cols)
    for a in (0, 1):
        s = cr.Stream(rows, cols, block=B, thr_q4=16, adapt_shift=a, min_blocks=1, max_regions=4)
        ref, cnt = np.zeros((s.bh, s.bw), np.int32), 0
        for k in range(4):
            frame = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
            if k == 2:
                frame[:, : cols // 2] = 255 - frame[:, : cols // 2] // 8
            ref, cnt, _ = both(s, ref, cnt, frame)


def test_sum_against_a_per_pixel_loop():
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (29, 45, 3), dtype=np.uint8)
    ref, cnt, mask, *_ = change_step_host(frame, np.zeros((4, 6), np.int32), 0, NET, NET, dict(block=8))
    for by in range(4):
        for bx in range(6):
            acc = 0
            for y in range(by * 8, min(29, by * 8 + 8)):
                for x in range(bx * 8, min(45, bx * 8 + 8)):
                    b, g, r = (int(v) for v in frame[y, x])
                    acc += 29 * b + 150 * g + 77 * r
            assert ref[by, bx] == acc


def test_pitched_source():
    rng = np.random.default_rng(9)
    s = cr.Stream(29, 45, block=8, min_blocks=1)
    ref, cnt = np.zeros((s.bh, s.bw), np.int32), 0
    for k in range(3):
        frame = rng.integers(0, 256, (29, 45, 3), dtype=np.uint8)
        buf, view = pitched(frame, 7 + k, 1 + k)
        ref, cnt, _ = both(s, ref, cnt, frame, src=view)


def test_grid_limit():
    """128 x 128 blocks of 8 pixels: 16384 blocks is the limit, one block column more is refused"""
    frame = np.zeros((1024, 1024, 3), np.uint8)
    frame[8:16, 8:24] = 200
    s = cr.Stream(1024, 1024, block=8)
    ref, cnt, _ = both(s, np.zeros((128, 128), np.int32), 0, np.zeros_like(frame))
    _, _, out = both(s, ref, cnt, frame)
    assert list(out[5]) == [2, 1, 1, 0]
    with pytest.raises(_lib.RFError):
        change_step_host(np.zeros((1024, 1025, 3), np.uint8), np.zeros((128, 129), np.int32), 0, NET, NET, dict(block=8))


# ---------------------------------------------------------------------------------------------- 2. the threshold
@pytest.mark.parametrize("shape", ((16, 16, 8, 0, 0), (17, 17, 8, 2, 2), (33, 33, 32, 1, 1)))
def test_block_exactly_at_the_threshold_and_one_unit_over(shape):
    """a full and a one-pixel (partial) block: |S - ref| == 16 thr npix does not mark it, one unit more does.  thr_q4 = 16 (one grey
    level): 256 per pixel, reached with one grey level on every channel of every pixel; one unit over: 29 more on one blue byte."""
    rows, cols, B, bx, by = shape
    s = cr.Stream(rows, cols, block=B, thr_q4=16, dilate=2, min_blocks=1)
    base = np.full((rows, cols, 3), 100, np.uint8)
    ref, cnt, _ = both(s, np.zeros((s.bh, s.bw), np.int32), 0, base)
    at = base.copy()
    at[by * B:(by + 1) * B, bx * B:(bx + 1) * B] += 1
    _, _, out = both(s, ref, cnt, at)
    assert not out[2].any()
    s.ref, s.frames = ref.copy(), cnt                                       # the reference stream back before that step
    over = at.copy()
    over[by * B, bx * B, 0] += 1
    _, _, out = both(s, ref, cnt, over)
    assert out[2][by, bx] == 1 and out[2].sum() == 1
    s.ref, s.frames = ref.copy(), cnt
    under = base.copy()
    under[by * B:(by + 1) * B, bx * B:(bx + 1) * B] -= 1
    under[by * B, bx * B, 0] -= 1                                           # negative difference, one unit over
    _, _, out = both(s, ref, cnt, under)
    assert out[2][by, bx] == 1 and out[2].sum() == 1


def test_noise_marks_no_block_at_the_default_threshold():
    """+-2 of noise on both frames: a pixel differs by at most 4 grey levels, so |dS| <= 4 * 256 * npix < 8 * 256 * npix = 16 * 128 * npix"""
    rng = np.random.default_rng(11)
    clean = rng.integers(2, 254, (45, 61, 3), dtype=np.uint8)
    s = cr.Stream(45, 61)
    ref, cnt = np.zeros((s.bh, s.bw), np.int32), 0
    for _ in range(3):
        noisy = (clean.astype(np.int16) + rng.integers(-2, 3, clean.shape)).astype(np.uint8)
        ref, cnt, out = both(s, ref, cnt, noisy)
        assert not out[2].any() and out[5][0] == 0


# ---------------------------------------------------------------------------------------------- 3. the reference update
@pytest.mark.parametrize("a", (0, 1, 8))
def test_reference_update_floors_negative_differences(a):
    s = cr.Stream(17, 23, block=8, adapt_shift=a)
    rng = np.random.default_rng(a)
    bright = rng.integers(128, 256, (17, 23, 3), dtype=np.uint8)
    ref, cnt, _ = both(s, np.zeros((s.bh, s.bw), np.int32), 0, bright)
    for k in range(3):
        dark = bright - (30 * (k + 1) + rng.integers(0, 10, bright.shape)).astype(np.uint8)     # darker every step: every difference negative
        before = ref.copy()
        ref, cnt, _ = both(s, ref, cnt, dark)
        S = cr.block_sums(dark, 8)[0]
        assert ((S - before) < 0).all() and np.array_equal(ref, before + ((S - before) >> a))
        if a == 0:
            assert np.array_equal(ref, S)


def test_seeding_and_reset():
    s = cr.Stream(24, 40, block=8)
    frame = np.random.default_rng(2).integers(0, 256, (24, 40, 3), dtype=np.uint8)
    ref, cnt, out = both(s, np.zeros((3, 5), np.int32), 0, frame)
    assert cnt == 1 and out[5][3] == 1 and np.array_equal(ref, cr.block_sums(frame, 8)[0])
    ref, cnt, out = both(s, ref, cnt, 255 - frame)
    assert cnt == 2 and out[5][3] == 0 and out[5][0] > 0
    s.reset()                                                               # counter 0 seeds again, whatever the reference holds
    ref, cnt, out = both(s, ref, 0, frame)
    assert cnt == 1 and list(out[5]) == [0, 0, 0, 1]


# ---------------------------------------------------------------------------------------------- 4. components
def spiral(n):
    """a one-block-wide path that winds inwards from (0, 0) with one free block between its turns"""
    m = np.zeros((n, n), np.uint8)
    x = y = turns = 0
    dx, dy = 1, 0
    m[0, 0] = 1
    while turns < 2:
        nx, ny, fx, fy = x + dx, y + dy, x + 2 * dx, y + 2 * dy
        if 0 <= nx < n and 0 <= ny < n and not m[ny, nx] and not (0 <= fx < n and 0 <= fy < n and m[fy, fx]):
            x, y, turns = nx, ny, 0
            m[y, x] = 1
        else:
            dx, dy, turns = -dy, dx, turns + 1
    return m


def snake(n):
    """a one-block-wide path that winds through an n x n grid: rows 0, 2, 4, .. joined alternately at the right and the left end"""
    m = np.zeros((n, n), np.uint8)
    m[0::2] = 1
    for k, y in enumerate(range(1, n, 2)):
        m[y, n - 1 if k % 2 == 0 else 0] = 1
    return m


def comb(n):
    m = np.zeros((n, n), np.uint8)
    m[n - 1] = 1
    m[:, 0::2] = 1
    return m


def test_diagonal_neighbours_are_one_component():
    m = np.zeros((6, 8), np.uint8)
    m[1, 1] = m[2, 2] = 1
    m[4, 6] = m[3, 7] = 1                                                   # the other diagonal
    out = run_mask(48, 64, m, block=8, dilate=2, min_blocks=1)
    assert list(out[5]) == [4, 2, 2, 0]
    assert list(out[3][0]) == [8 - 4, 8 - 4, 16 + 8, 16 + 8] and list(out[3][1]) == [48 - 4, 24 - 4, 16 + 8, 16 + 8]      # (a region is not clipped)


@pytest.mark.parametrize("shape", ("spiral", "snake", "comb"))
def test_winding_components_are_one(shape):
    m = {"spiral": spiral, "snake": snake, "comb": comb}[shape](17)
    out = run_mask(17 * 8, 17 * 8, m, block=8, dilate=2, min_blocks=1)
    assert out[5][1] == 1 and out[5][2] == 1 and out[5][0] == int(m.sum())
    assert list(out[4][0][:4]) == [-34, -34, 136 + 68, 136 + 68]


def test_dilation_joins_components_and_touches_the_border():
    m = np.zeros((6, 8), np.uint8)
    m[0, 0] = m[0, 3] = 1                                                   # two blocks apart: joined by the dilation, at the border
    m[5, 7] = 1
    off = run_mask(48, 64, m, block=8, dilate=2, min_blocks=1)
    assert list(off[5]) == [3, 3, 3, 0]
    on = run_mask(48, 64, m, block=8, dilate=1, min_blocks=1)
    assert list(on[5]) == [3, 2, 2, 0]
    assert list(on[3][0]) == [-10, -10, 40 + 20, 16 + 20]                   # blocks (0..4, 0..1): 40 x 16 pixels, margin a quarter of 40
    assert list(on[3][1]) == [48 - 4, 32 - 4, 16 + 8, 16 + 8]               # blocks (6..7, 4..5), clipped by the grid


def test_256_isolated_blocks_keep_the_sixteen_lowest_labels():
    m = np.zeros((32, 32), np.uint8)
    m[0::2, 0::2] = 1
    out = run_mask(256, 256, m, block=8, dilate=2, min_blocks=1, max_regions=16)
    assert list(out[5]) == [256, 256, 16, 0]
    assert [tuple(r[:2]) for r in out[3]] == [(16 * k - 2, -2) for k in range(16)]      # row 0, left to right: labels 0, 2, .. 30


def test_ties_min_blocks_and_region_counts():
    m = np.zeros((12, 16), np.uint8)
    m[1, 1:4] = 1                    # 3 blocks, label 17
    m[5, 10:13] = 1                  # 3 blocks, label 90: the tie goes to the lower label
    m[8, 2:7] = 1                    # 5 blocks
    m[10, 14] = 1                    # 1 block
    m[3, 8:10] = 1                   # 2 blocks
    kw = dict(block=8, dilate=2)
    out = run_mask(96, 128, m, min_blocks=1, **kw)
    assert list(out[5]) == [14, 5, 5, 0]
    assert [int(r[1]) + (int(r[3]) - 8) // 2 for r in out[3][:5]] == [64, 8, 40, 24, 80]      # by rows: 8, 1, 5, 3, 10
    out = run_mask(96, 128, m, **kw)                                        # min_blocks 2 by default: the single block is dropped
    assert list(out[5]) == [14, 5, 4, 0]
    out = run_mask(96, 128, m, min_blocks=3, **kw)
    assert list(out[5]) == [14, 5, 3, 0]
    out = run_mask(96, 128, m, min_blocks=1, max_regions=1, **kw)
    assert list(out[5]) == [14, 5, 1, 0] and out[3].shape == (1, 4)
    out = run_mask(96, 128, m, min_blocks=1, max_regions=64, **kw)
    assert list(out[5]) == [14, 5, 5, 0] and out[4].shape == (64, 8) and (out[4][5:, 7] == cr.VOID).all()


def test_whole_frame_change_is_one_cropped_region():
    out = run_mask(29 * 16, 37 * 16, np.ones((29, 37), np.uint8))
    assert list(out[5]) == [29 * 37, 1, 1, 0]
    assert out[4][0][4] == -2 and out[4][0][7] == ROI_CROPPED              # wider than four cells of 112 pixels


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals():
    lib = _lib.load_library()
    frame = np.zeros((24, 40, 3), np.uint8)
    ref = np.zeros(15, np.int32)
    mask = np.zeros(15, np.uint8)
    regions, cells, info = (_lib.rf_roi * 64)(), (_lib.rf_roi_cell * 64)(), _lib.rf_change_info()

    def call(spec=None, src=frame.ctypes.data, rows=24, cols=40, step=120, r=ref.ctypes.data, counter=0, mq=0, w=448, h=448, rs=None,
             m=mask.ctypes.data, rg=regions, cl=cells, inf=C.byref(info), no_counter=False):
        sp = change_spec(block=8) if spec is None else spec
        cnt = C.c_int64(counter)
        ref[:] = 77
        st = lib.rf_change_step_host(C.byref(sp), src, rows, cols, step, r, None if no_counter else C.byref(cnt), mq, w, h, rs, m, rg, cl, inf)
        return st, cnt.value
    assert call() == (0, 1) and (ref == 0).all()
    bad_roi = _lib.rf_roi_spec(C.sizeof(_lib.rf_roi_spec), 3, 0, 0, 0, 0)
    short = change_spec(block=8)
    short.struct_size = 28
    reserved = change_spec(block=8)
    reserved.reserved = 1
    bad_specs = [short, reserved, change_spec(block=4), change_spec(block=64), change_spec(thr_q4=65536), change_spec(thr_q4=-1),
                 change_spec(adapt_shift=9), change_spec(adapt_shift=-1), change_spec(dilate=3), change_spec(min_blocks=65536),
                 change_spec(max_regions=65), change_spec(max_regions=-1)]
    for kw in [dict(spec=s) for s in bad_specs] + [dict(src=None), dict(rows=0), dict(cols=0), dict(step=119), dict(r=None), dict(counter=-1),
                                                    dict(no_counter=True), dict(mq=-1), dict(mq=65536), dict(w=450), dict(w=56), dict(h=450),
                                                    dict(rs=C.byref(bad_roi)), dict(m=None), dict(rg=None), dict(cl=None), dict(inf=None),
                                                    dict(rows=8 * 129, cols=8 * 128)]:
        st, cnt = call(**kw)
        assert st == -1 and (ref == 77).all() and cnt == kw.get("counter", 0), kw
    with pytest.raises(_lib.RFError):
        change_step_host(frame, ref, 0, 448, 448, dict(block=8), margin=0.001)      # 0 / 256 would silently mean the default
    with pytest.raises(ValueError):
        change_step_host(frame, np.zeros(14, np.int32), 0, 448, 448, dict(block=8))


# ---------------------------------------------------------------------------------------------- 6. the claim, through the CPU oracle
CLAIM_THR = 0.6
NEWCOMER = 0                                                    # the face painted out of the seed frame: the key frame's best-scoring one


def paint_out(frame, box, grow=0.35):
    """the frame with the box (grown on every side) replaced by the mean colour of the ring of 8 pixels around it"""
    x1, y1, x2, y2 = (float(v) for v in box)
    m = grow * max(x2 - x1, y2 - y1)
    rows, cols = frame.shape[:2]
    X1, Y1, X2, Y2 = max(int(x1 - m), 0), max(int(y1 - m), 0), min(int(x2 + m) + 1, cols), min(int(y2 + m) + 1, rows)
    out = frame.copy()
    ring = frame[max(Y1 - 8, 0):min(Y2 + 8, rows), max(X1 - 8, 0):min(X2 + 8, cols)].astype(np.float64)
    total = ring.sum((0, 1)) - frame[Y1:Y2, X1:X2].astype(np.float64).sum((0, 1))
    n = ring.shape[0] * ring.shape[1] - (Y2 - Y1) * (X2 - X1)
    out[Y1:Y2, X1:X2] = np.round(total / n).astype(np.uint8)
    return out, (X1, Y1, X2, Y2)


def test_a_newcomer_is_found_from_the_change_regions_and_gets_its_id(oracles, base_frame):
    """The claim: mnet25, net 448, threshold 0.6, the 896 x 1280 base frame with its six faces.  The key frame is the base frame with
    its best-scoring face painted out by the mean of its surroundings: a full-resolution detection finds five faces, which open five
    tracks, and the changer seeds on it.  The next frame is the base frame itself: the sixth face has entered.  The changer's step at
    its defaults (B = 16, 8 grey levels, dilation, margin a quarter) gives change regions of which one contains the face; ONE
    448 x 448 view of the five track cells and the change cells, the oracle on it, the face rule, the merge and the frame step keep the
    five ids and open track 6 for the newcomer.  Tracked region detection alone on the same frame -- the track cells only -- does not
    find it.  Measured: see the prints; DESIGN.md section 34 quotes them."""
    oracle = oracles["mnet25"]
    full = oracle.detect(base_frame, CLAIM_THR, NMS, net_hw=base_frame.shape[:2]).rows()
    assert len(full) == 6
    box = full[NEWCOMER][1:5]
    key_frame, painted = paint_out(base_frame, box)
    key = oracle.detect(key_frame, CLAIM_THR, NMS, net_hw=base_frame.shape[:2]).rows()
    assert len(key) == 5 and all(tr.iou(f[1:5], box) < 0.1 for f in key)
    table = np.zeros(10, TRACK_DTYPE)                            # T = 10, R = 6: one pass at grid 4
    tags, ended, frames, next_id, trunc = track_step(table, 0, 1, key, max_tracks=10)
    assert sorted(tags["id"]) == [1, 2, 3, 4, 5] and next_id == 6
    ids = table["id"].copy()
    s = cr.Stream(896, 1280, max_regions=6)
    ref, cnt, _ = both(s, np.zeros((s.bh, s.bw), np.int32), 0, key_frame)
    ref, cnt, out = both(s, ref, cnt, base_frame, grid=4)
    mask, regions, cells, info = out[2:]
    print("changed blocks %d, components %d, kept %d; regions %s" % (info[0], info[1], info[2], [tuple(int(v) for v in r) for r in regions[:info[2]]]))
    # the changed blocks lie inside the painted rectangle, and a kept region contains the face's own region (its box grown by a quarter)
    ys, xs = np.nonzero(mask)
    assert info[2] >= 1 and xs.min() * 16 >= painted[0] - 15 and ys.min() * 16 >= painted[1] - 15 and xs.max() * 16 < painted[2] and ys.max() * 16 < painted[3]
    face_roi = rr.from_faces(full[NEWCOMER].reshape(1, 15), 1.0, 0)[0]
    holds = [k for k in range(info[2]) if regions[k][0] <= face_roi[0] and regions[k][1] <= face_roi[1] and
             regions[k][0] + regions[k][2] >= face_roi[0] + face_roi[2] and regions[k][1] + regions[k][3] >= face_roi[1] + face_roi[3]]
    assert holds, (face_roi, regions)
    track_cells = roi_cells_from_tracks(table, NET, NET, grid=4)
    found = {}
    for name, all_cells in (("tracks alone", track_cells), ("tracks and change regions", np.concatenate([track_cells, cells]))):
        rois = [tuple(int(v) for v in c[:4]) for c in all_cells]
        view = roi_atlas_host(base_frame, rois, NET, NET, 4)
        assert view.shape == (1, NET, NET, 3) and np.array_equal(view, rtr.atlas(base_frame, all_cells, NET, NET, 4))
        faces = oracle.detect(view[0], CLAIM_THR, NMS, net_hw=(NET, NET)).rows()
        merged, count, votes, src, _ = rtr.merge(all_cells, [faces], NET, NET, NMS, 64, 4)
        t2 = table.copy()
        tg, _, _, nid, _ = track_step(t2, frames, next_id, merged, max_tracks=10)
        hit = [k for k, f in enumerate(merged) if tr.iou(f[1:5], box) >= 0.5]
        print("%s: %d faces, regions %s, ids %s, level of the change cell %s" % (name, len(merged), [int(v) for v in src], [int(v) for v in tg["id"]],
                                                                                  int(cells[holds[0]][4])))
        found[name] = (merged, src, tg, nid, t2, hit)
    merged, src, tg, nid, t2, hit = found["tracks alone"]
    assert not hit and nid == next_id and sorted(tg["id"]) == [1, 2, 3, 4, 5]                   # section 33 alone does not see the newcomer
    merged, src, tg, nid, t2, hit = found["tracks and change regions"]
    assert len(hit) == 1 and int(src[hit[0]]) == 10 + holds[0]                                  # found by the change region that holds it
    assert sorted(tg["id"]) == [1, 2, 3, 4, 5, 6] and nid == 7 and int(tg["id"][hit[0]]) == 6   # five ids kept, the sixth opened
    assert (tg["flags"][hit[0]] & tr.NEW) and np.array_equal(t2["id"][:5], ids[:5])


# ---------------------------------------------------------------------------------------------- 7. the sanitizer program
def test_steps_under_address_and_ub_sanitizers(tmp_path):
    """tests/csrc/test_change_host.cpp: random frames and masks at this file's shapes stepped into exactly-sized heap buffers, every
    record checked against its definition; host code only, built with -fsanitize=address,undefined.  No GPU and no library: change.h
    and roi.h are compiled into the program."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")                        # for <hip/hip_runtime.h>, which roi.h includes
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "test_change_host")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "test_change_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), (r.stdout[-2000:], r.stderr[-4000:])
