"""Tracked region detection on the host: rf_roi_cells_from_tracks (roi.h roi_track_cell, the code the plan kernel runs) against
tests/roi_track_ref.py byte for byte, void cells through rf_roi_atlas_host and rf_roi_map_face, the refusals, the claim (a key frame's
six tracks found again, ids kept, from ONE 448 x 448 view of the regions planned from their table) end to end through the CPU oracle,
and roi.h with track.h and motion.h on their own under the address and UB sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import motion_ref as mr
import roi_ref as rr
import roi_track_ref as rtr
import track_ref as tr
from conftest import ROOT
from retinaface_amd import ROI_CROPPED, ROI_VOID, _lib, roi_atlas_host, roi_cells_from_tracks, roi_map_face, roi_plan, track_step
from retinaface_amd import MOTION_DTYPE, TRACK_DTYPE
from test_roi_host import LEVELS, fit, pitched
from test_track_host import by_score, face

f32 = np.float32
NET, NMS = 448, 0.4
VOID_ROI = (0, 0, 0, 0)


def check_cells(stream, margin=None, grid=0, max_zoom=0, net=(NET, NET)):
    """rf_roi_cells_from_tracks on the stream's table (and motion records) against the reference"""
    has_motion = isinstance(stream, mr.Stream)
    got = roi_cells_from_tracks(stream.table, net[0], net[1], motion=stream.motion if has_motion else None,
                                mspec=dict(alpha=float(stream.mspec.alpha), horizon=stream.mspec.horizon if stream.mspec.horizon else -1) if has_motion else None,
                                margin=margin, grid=grid, max_zoom=max_zoom)
    want = rtr.stream_cells(stream, 0 if margin is None else int(round(margin * 256)), net[0], net[1], grid, max_zoom)
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (got, want)
    return got


def is_void(cell):
    return tuple(int(v) for v in cell) == rtr.VOID_CELL


def stream_of(max_tracks, rows, motion=None, **kw):
    """a reference stream whose live slots are exactly 0 .. len(rows) - 1: one step over the rows in score order"""
    spec = tr.Spec(max_tracks, **kw)
    s = mr.Stream(spec, mr.Spec(*motion)) if motion is not None else tr.Stream(spec)
    (mr.step if motion is not None else tr.step)(s, by_score(rows) if len(rows) else np.zeros(0, tr.FACE))
    return s


def spread(n, size=40.0):
    """n faces that do not overlap, scores descending"""
    return [face(0.99 - 0.001 * k, 30.0 + 97.0 * (k % 12) + 0.25 * k, 20.0 + 83.0 * (k // 12), size + (k % 7) * 9.5) for k in range(n)]


def test_struct_and_flag():
    assert C.sizeof(_lib.rf_roi_cell) == 32 and ROI_VOID == 2 and ROI_CROPPED == 1
    assert TRACK_DTYPE.itemsize == tr.TRACK.itemsize == 176 and MOTION_DTYPE.itemsize == mr.MOTION.itemsize == 16


# ---------------------------------------------------------------------------------------------- 1. the cells of a table
@pytest.mark.parametrize("max_tracks", (1, 16, 17, 64))
def test_cells_of_live_prefix_holes_and_free_tables(max_tracks):
    """live slots 0 .. L - 1, holes made by max_missed = 1 and steps that omit faces, all free; every grid and every max_zoom"""
    for grid in (1, 2, 4):
        for mz in (0, 1, 2, 4):
            free = tr.Stream(tr.Spec(max_tracks))
            assert all(is_void(c) for c in check_cells(free, None, grid, mz))
    L = max(max_tracks - 3, 1)
    rows = spread(L)
    s = stream_of(max_tracks, rows, max_missed=1)
    for grid in (1, 2, 4):
        for mz in (0, 1, 2, 4):
            got = check_cells(s, None, grid, mz)
            assert [is_void(c) for c in got] == [k >= L for k in range(max_tracks)]
            assert rr.passes_of(max_tracks, grid) == -(-max_tracks // (grid * grid))
    # holes: two steps that omit every third face end those tracks; the others stay where they are
    keep = [r for k, r in enumerate(rows) if k % 3 != 1]
    for _ in range(2):
        tr.step(s, by_score(keep) if keep else np.zeros(0, tr.FACE))
    live = s.table["id"] != 0
    assert max_tracks == 1 or (not live[1] and live[0] and (L < 3 or live[2]))
    got = check_cells(s, 0.5, 4, 2)
    assert [is_void(c) for c in got] == [not v for v in live]
    # the cell of a live slot is the plan of the region of its last box: rf_roi_plan / rf_roi_from_faces give the same record
    from retinaface_amd import rois_from_faces
    for k in np.nonzero(live)[0]:
        last = np.frombuffer(s.table[k]["last"].tobytes(), np.float32)
        roi = rois_from_faces([last], 1.0, 0.5)
        assert np.array_equal(roi_plan(roi, NET, NET, 4, 2)[0][0], got[k])


@pytest.mark.parametrize("grid", (1, 2, 4))
def test_cell_levels_at_exact_fit_and_one_pixel_more(grid):
    """margin 1 / 256 (margin_q8 = 1): a box whose region fits its cell exactly, and one pixel more, at each of the five levels"""
    cw = NET // grid
    rows, want_levels = [], []
    for level in LEVELS:
        s = fit(level, cw)
        for target, lv in ((s, level), (s + 1, level - 1)):
            dx, side = next((dx, a) for dx in (0.0, 0.5) for a in range(1, target + 1)
                            if rr.from_faces(face(0.9, 10.0 + dx, 20.0, float(a)).reshape(1, 15), 1.0, 1)[0][2:] == (target, target))
            rows.append(face(0.99 - 0.001 * len(rows), 3000.0 * len(rows) + 10.0 + dx, 20.0 + dx, float(side)))
            want_levels.append(lv)
    s = stream_of(16, rows)
    got = check_cells(s, 1 / 256, grid, 4)
    assert list(got[:10, 4]) == [max(l, -2) for l in want_levels]
    assert list(got[:10, 7]) == [0] * 9 + [ROI_CROPPED] and all(is_void(c) for c in got[10:])


def test_cropped_void_and_margins():
    wide = face(0.99, -100.0, 50.0, 4 * 112 + 40.0, 60.0)                     # wider than four cells at margin 1 / 256
    nan, inf, inverted, far = (face(0.98 - 0.01 * k, 100.0 + 400 * k, 300.0, 50.0) for k in range(4))
    nan[1] = np.nan
    inf[3] = np.inf
    inverted[3] = inverted[1] - 1
    far[1:5] = (4e6, 0, 4e6 + 5, 5)
    edge = face(0.5, float(1 << 20) - 30, 10.0 - float(1 << 20), 30.0)      # a box that ends at +2^20
    rows = [wide, nan, inf, inverted, far, edge, face(0.4, 10.5, 20.25, 40.0, 50.0)]
    s = stream_of(16, rows)
    assert (s.table["id"][:7] != 0).all()                                      # every one of them opened a track
    got = check_cells(s, 1 / 256, 4, 2)
    assert got[0, 4] == -2 and got[0, 7] == ROI_CROPPED
    assert [is_void(c) for c in got[:7]] == [False, True, True, True, True, False, False]
    dflt = check_cells(s, None, 4, 2)                                           # margin_q8 0: the default, a quarter
    assert list(dflt[6, :4]) == [-2, 7, 65, 76] and np.array_equal(dflt, check_cells(s, 0.25, 4, 2))
    assert list(got[6, :4]) == [10, 20, 41, 51]                                # 50 / 256 px on every side, floored and ceiled
    check_cells(s, 65535 / 256, 4, 2)                                           # margin_q8 65535
    for net, grid in (((448, 448), 2), ((1280, 896), 4), ((64, 48), 4), ((32, 16), 2)):
        check_cells(s, None, grid, 4, net)


def test_cells_with_motion():
    """two steps with a displaced face give a velocity; samples == 0, missed 0 and 3, the horizon reached, a negative horizon"""
    moves = [face(0.99, 100.0, 100.0, 60.0), face(0.98, 400.0, 300.0, 80.0), face(0.97, 700.0, 120.0, 50.0)]
    for horizon in (8, 2, -1):
        s = stream_of(16, moves, motion=(0.5, horizon), max_missed=5)
        assert (s.motion["samples"][:3] == 0).all()
        first = check_cells(s, None, 4, 2)                                      # samples == 0: the last box itself
        plain = tr.Stream(s.spec)
        plain.table = s.table.copy()
        assert np.array_equal(first, check_cells(plain, None, 4, 2))
        for t in (1, 2):                                                        # the first two move, the third stands
            mr.step(s, by_score([face(0.99, 100.0 + 12 * t, 100.0 + 5 * t, 60.0), face(0.98, 400.0 - 9 * t, 300.0, 80.0), moves[2]]))
        assert (s.motion["samples"][:3] == 2).all() and s.motion["vx"][0] == 12 and s.motion["vx"][1] == -9
        plain.table = s.table.copy()
        for missed in range(4):                                                 # missed 0 .. 3: h = min(missed + 1, horizon)
            assert (s.table["missed"][:3] == missed).all()
            got = check_cells(s, None, 4, 2)
            base = check_cells(plain, None, 4, 2)
            h = min(missed + 1, max(horizon, 0))
            assert got[0, 0] - base[0, 0] == 12 * h and got[0, 1] - base[0, 1] == 5 * h and got[1, 0] - base[1, 0] == -9 * h
            assert np.array_equal(got[2], base[2])                              # the standing face: velocity 0
            if horizon < 0:
                assert np.array_equal(got, base)                                # never extrapolates: the plain tracker's bytes
            mr.step(s, np.zeros(0, tr.FACE))
            plain.table = s.table.copy()
    # a velocity that carries the box beyond +-2^20: void
    s = stream_of(4, [face(0.9, 1000.0, 10.0, 40.0)], motion=(1.0, 8))
    mr.step(s, by_score([face(0.9, 1010.0, 10.0, 40.0)]))
    assert s.motion["samples"][0] == 1
    s.motion["vx"][0] = 3e5
    s.table["missed"][0] = 5
    assert is_void(check_cells(s, None, 4, 2)[0])


def test_refusals():
    lib = _lib.load_library()
    table = np.zeros(4, TRACK_DTYPE)
    cells = (_lib.rf_roi_cell * 4)()
    tp = table.ctypes.data_as(C.POINTER(_lib.rf_track))

    def call(spec=None, mspec=None, t=tp, motion=None, T=4, mq=0, w=448, h=448, rs=None, out=cells):
        cells[0].level = 77
        return lib.rf_roi_cells_from_tracks(spec, mspec, t, motion, T, mq, w, h, rs, out)
    assert call() == 0 and cells[0].level == 0 and cells[0].flags == ROI_VOID
    bad_roi, bad_track, bad_motion = _lib.rf_roi_spec(), _lib.rf_track_spec(), _lib.rf_motion_spec()
    bad_roi.struct_size, bad_roi.grid = C.sizeof(_lib.rf_roi_spec), 3
    bad_track.struct_size = 20
    bad_motion.struct_size = 12
    for kw in (dict(T=0), dict(T=257), dict(mq=-1), dict(mq=65536), dict(t=None), dict(out=None), dict(w=450), dict(w=56), dict(h=450),
               dict(rs=C.byref(bad_roi)), dict(spec=C.byref(bad_track)), dict(mspec=C.byref(bad_motion))):
        assert call(**kw) == -1 and cells[0].level == 77, kw
    with pytest.raises(_lib.RFError):
        roi_cells_from_tracks(table, 448, 448, margin=0.001)                    # 0 / 256 would silently mean the default
    with pytest.raises(ValueError):
        roi_cells_from_tracks(table, 448, 448, motion=np.zeros(3, MOTION_DTYPE))
    # rf_roi_plan refuses the void region as before and never produces a void record
    with pytest.raises(_lib.RFError):
        roi_plan([VOID_ROI], 448, 448)


# ---------------------------------------------------------------------------------------------- 2. void cells
@pytest.mark.parametrize("view", ((32, 16, 2), (64, 48, 4)))
def test_atlas_host_with_void_cells_among_real_ones(view):
    """zeros in the void cells, the reference's bytes in the others, untouched sentinels around a pitched destination"""
    vw, vh, grid = view
    frame = np.random.default_rng(vw).integers(1, 256, (97, 131, 3), dtype=np.uint8)
    keep, src = pitched(frame)
    real = [(5, 7, 20, 12), (-6, 60, 40, 44), (100, 80, 60, 30), (40, 40, 9, 5), (0, 0, 131, 97), (128, 94, 8, 8)]
    rois = []
    for k in range(grid * grid + 2):                                           # two passes; voids first, last and between
        rois.append(VOID_ROI if k % 3 == 0 or k == grid * grid + 1 else real[k % len(real)])
    cells = np.array([rtr.VOID_CELL if r == VOID_ROI else tuple(r) + rr.plan_one(r, vw // grid, vh // grid, 2) for r in rois], np.int32)
    want = rtr.atlas(frame, cells, vw, vh, grid)
    got = roi_atlas_host(src, rois, vw, vh, grid, 2)
    assert got.shape == want.shape == (2, vh, vw, 3) and np.array_equal(got, want)
    cw, ch = vw // grid, vh // grid
    assert not got[0, :ch, :cw].any() and got[0, :ch, cw:2 * cw].any()         # cell 0 is void, cell 1 is not
    lib = _lib.load_library()
    arr = (_lib.rf_roi * len(rois))(*[_lib.rf_roi(*r) for r in rois])
    dstep = 3 * vw + 5
    dst = np.full(2 * vh * dstep + 3, 0xAB, np.uint8)
    st = lib.rf_roi_atlas_host(C.byref(_lib.rf_roi_spec(C.sizeof(_lib.rf_roi_spec), grid, 2, 0, 0, 0)), vw, vh, src.ctypes.data, 97, 131, src.strides[0],
                               arr, len(rois), dst[1:].ctypes.data, dstep)
    assert st == 0
    body = dst[1:1 + 2 * vh * dstep].reshape(2 * vh, dstep)
    assert np.array_equal(body[:, :3 * vw].reshape(2, vh, vw, 3), want)
    assert (body[:, 3 * vw:] == 0xAB).all() and dst[0] == 0xAB and (dst[1 + 2 * vh * dstep:] == 0xAB).all()


def test_map_face_drops_the_faces_of_void_cells():
    rois = [(100, 100, 112, 112), VOID_ROI, (300, 50, 112, 112), VOID_ROI, VOID_ROI, (10, 10, 112, 112)]      # the real ones fill their cells at x1
    cells = np.array([rtr.VOID_CELL if r == VOID_ROI else tuple(r) + rr.plan_one(r, 112, 112, 2) for r in rois], np.int32)

    def both(f):
        got = roi_map_face(f, rois, 0, NET, NET, 4, 2)
        want = rtr.map_face(f, cells, 0, NET, NET, 4)
        assert (got is None) == (want is None)
        if got is not None:
            assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
        return got
    # a centre in a void cell: its middle, its first pixel, the last float in front of its right border
    for cx in (112 + 56.0, 112.0, float(np.nextafter(f32(224), f32(0)))):
        f = face(0.9, cx - 10, 40.0, 20.0)
        assert both(f) is None
    # a border next to one: a quarter pixel in front of cell 0's right border and the first pixel of cell 2 keep their faces
    left = face(0.9, 111.75 - 10, 46.0, 20.0)
    right = face(0.9, 224.0 - 10 + 0.0, 46.0, 20.0)
    assert both(left) is not None and both(left)[1] == 0
    assert both(right) is not None and both(right)[1] == 2
    # the second row: cells 4 (void) and 5 (real)
    assert both(face(0.9, 40.0, 112.0 + 40, 20.0)) is None and both(face(0.9, 112.0 + 40, 112.0 + 40, 20.0))[1] == 5
    with pytest.raises(_lib.RFError):
        roi_map_face(left, [(0, 0, 0, 5)], 0, NET, NET)                         # an empty region that is not the void region stays refused


# ---------------------------------------------------------------------------------------------- 3. the claim, through the CPU oracle
CLAIM_THR, CLAIM_SHIFT = 0.6, 6
CLAIM_MIN_IOU = 0.3                                             # the tracker's default: what an id needs to survive


def claim_case(oracle, frame, table, frames, next_id):
    """one tracked region frame on the host: cells from the table, ONE view, the oracle, the face rule and merge, the step.  Returns
    (tags, the worst IoU of a merged face with the `last` box of the slot whose region found it, the table after)"""
    table = table.copy()
    cells = roi_cells_from_tracks(table, NET, NET, grid=4)
    assert np.array_equal(cells, rtr.cells_of(table.view(tr.TRACK), None, None, 0, NET, NET, 4))
    rois = [tuple(int(v) for v in c[:4]) for c in cells]
    view = roi_atlas_host(frame, rois, NET, NET, 4)
    assert view.shape == (1, NET, NET, 3) and np.array_equal(view, rtr.atlas(frame, cells, NET, NET, 4))
    faces = oracle.detect(view[0], CLAIM_THR, NMS, net_hw=(NET, NET)).rows()
    merged, count, votes, src, _ = rtr.merge(cells, [faces], NET, NET, NMS, 64, 4)
    for f in faces:                                               # rf_roi_map_face agrees with the reference on every face of the view
        got, want = roi_map_face(f, rois, 0, NET, NET, 4), rtr.map_face(f, cells, 0, NET, NET, 4)
        assert (got is None) == (want is None) and (got is None or (got[0].tobytes() == want[0].tobytes() and got[1] == want[1]))
    worst = 1.0
    for f, s in zip(merged, src):
        last = table[int(s)]["last"]
        worst = min(worst, float(tr.iou(f[1:5], np.array([last["x1"], last["y1"], last["x2"], last["y2"]], np.float32))))
    tags, ended, frames, next_id, trunc = track_step(table, frames, next_id, merged, max_tracks=16)
    return tags, src, worst, table, next_id


def test_six_tracks_keep_their_ids_through_one_view(oracles, base_frame):
    """The claim: mnet25, net 448, threshold 0.6.  A full-resolution key detection of the 896 x 1280 base frame opens six tracks
    (max_tracks 16: one pass at grid 4).  Their cells at the default margin of a quarter go into ONE 448 x 448 view; the oracle on that
    view, the face rule and the frame step keep six ids and open none -- on the same frame, and on the frame's content displaced by
    (6, 6) (a crop), as after a small pan.  An id survives at min_iou = 0.3.  Measured worst IoU of a merged face with the `last` box
    of its slot: 0.828 on the same frame, 0.699 displaced."""
    oracle = oracles["mnet25"]
    full = oracle.detect(base_frame, CLAIM_THR, NMS, net_hw=base_frame.shape[:2]).rows()
    assert len(full) == 6
    table = np.zeros(16, TRACK_DTYPE)
    tags, ended, frames, next_id, trunc = track_step(table, 0, 1, full, max_tracks=16)
    assert sorted(tags["id"]) == [1, 2, 3, 4, 5, 6] and next_id == 7
    ids = table["id"].copy()
    for name, frame in (("same frame", base_frame), ("displaced by (6, 6)", np.ascontiguousarray(base_frame[CLAIM_SHIFT:, CLAIM_SHIFT:]))):
        tags, src, worst, after, nid = claim_case(oracle, frame, table, frames, next_id)
        print("%s: %d faces, slots %s, worst IoU to `last` %.3f" % (name, len(tags), [int(v) for v in src], worst))
        assert len(tags) == 6 and nid == next_id and not (tags["flags"] & tr.NEW).any()          # six faces, none opened
        assert sorted(tags["id"]) == [1, 2, 3, 4, 5, 6] and np.array_equal(after["id"], ids)     # six ids kept, in their slots
        assert list(tags["slot"]) == [int(s) for s in src]                                        # each claimed by the slot whose region found it
        assert worst >= CLAIM_MIN_IOU


# ---------------------------------------------------------------------------------------------- 4. the sanitizer program
def test_cells_and_void_atlases_under_address_and_ub_sanitizers(tmp_path):
    """tests/csrc/test_roi_track_host.cpp: random tables with free slots and extreme floats planned into exactly-sized buffers, every
    cell checked against its definition, atlases with void cells into exactly-sized heap buffers; host code only, built with
    -fsanitize=address,undefined.  No GPU and no library: roi.h, track.h and motion.h are compiled into the program."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")                        # for <hip/hip_runtime.h>, which roi.h includes
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "test_roi_track_host")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "test_roi_track_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), (r.stdout[-2000:], r.stderr[-4000:])
