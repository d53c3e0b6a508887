"""Region detection on the host: rf_roi_plan, rf_roi_atlas_host, rf_roi_map_face, rf_roi_from_faces and rf_roi_merge_host against
tests/roi_ref.py byte for byte, the refusals, the claim (the base frame's six faces found again from one 448 x 448 atlas of their own
regions) end to end through the CPU oracle, and roi.h on its own under the address and UB sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import roi_ref as rr
from conftest import ROOT
from retinaface_amd import ROI_CROPPED, _lib, roi_atlas_host, roi_map_face, roi_merge_host, roi_plan, roi_spec, rois_from_faces
from test_tta_host import face

NET, NMS = (448, 448), 0.4
LEVELS = (2, 1, 0, -1, -2)


def fit(level, cell):
    """the largest side that fits a cell of `cell` pixels at `level`"""
    return cell >> level if level >= 0 else cell << -level


# ---------------------------------------------------------------------------------------------- 1. the plan
def check_plan(rois, view_w, view_h, grid=0, max_zoom=0):
    got, passes = roi_plan(rois, view_w, view_h, grid, max_zoom)
    want = rr.plan(rois, view_w, view_h, grid, max_zoom)
    assert np.array_equal(got, want), (got, want)
    assert passes == rr.passes_of(len(rois), grid)
    return got


@pytest.mark.parametrize("grid", (1, 2, 4))
def test_plan_levels_at_exact_fit_and_one_pixel_more(grid):
    cw = ch = 448 // grid
    for level in LEVELS:
        s = fit(level, cw)
        # exact in both axes, exact in one, one pixel more in x, in y; odd and even c2 = 2 x + w; w or h of 1
        rois = [(10, 20, s, s), (11, -7, s, 1), (-5, 3, 1, s), (0, 0, s + 1, s), (0, 0, s, s + 1), (7, 7, s - 1, s), (8, 8, s - 1, s - 1)]
        got = check_plan(rois, 448, 448, grid, 4)
        assert list(got[:3, 4]) == [level] * 3 and list(got[5:, 4]) == [level] * 2 and not got[:3, 7].any()
        if level > -2:
            assert got[3, 4] == level - 1 and got[4, 4] == level - 1 and not got[3, 7]
        else:
            assert got[3, 4] == -2 and got[3, 7] == ROI_CROPPED and got[4, 7] == ROI_CROPPED
    # the centre: a region of exactly the cell at x1 starts the cell at its own origin; odd c2 floors
    got = check_plan([(30, 40, cw, ch), (31, 41, cw - 1, ch - 1), (-31, -41, cw - 1, ch - 1)], 448, 448, grid, 1)
    assert list(got[0, 4:8]) == [0, 30, 40, 0] and list(got[1, 4:8]) == [0, 30, 40, 0] and list(got[2, 4:8]) == [0, -32, -42, 0]


def test_plan_max_zoom_and_cropped_regions():
    small = [(100, 100, 20, 24), (5, 5, 1, 1), (300, 200, 56, 56), (0, 0, 57, 20)]
    for mz, want in ((1, [0, 0, 0, 0]), (2, [1, 1, 1, 0]), (4, [2, 2, 1, 0]), (0, [1, 1, 1, 0])):
        got = check_plan(small, 448, 448, 4, mz)
        assert list(got[:, 4]) == want, mz
    # larger than four cells in either axis: x1/4, the centre of the region, flagged
    big = [(0, 0, 449, 10), (-200, 50, 10, 4 * 112 + 1), (-(1 << 20), 1 << 20, 16384, 16384), (1 << 20, -(1 << 20), 16384, 1)]
    got = check_plan(big, 448, 448, 4, 2)
    assert list(got[:, 4]) == [-2] * 4 and list(got[:, 7]) == [ROI_CROPPED] * 4
    assert got[0, 5] == (449 - 4 * 112) // 8 and got[0, 6] == (10 - 4 * 112) // 8
    for net in ((448, 448), (896, 896), (1280, 1280), (1280, 896)):
        for grid in (1, 2, 4):
            check_plan(small + big, net[0], net[1], grid, 4)


def test_plan_16_and_17_regions_are_one_and_two_passes():
    rois = [(10 * i, 7 * i, 30 + i, 40) for i in range(17)]
    assert roi_plan(rois[:16], 448, 448, 4)[1] == 1 and roi_plan(rois, 448, 448, 4)[1] == 2
    assert roi_plan(rois, 448, 448, 2)[1] == 5 and roi_plan(rois, 448, 448, 1)[1] == 17 and roi_plan([], 448, 448)[1] == 0


# ---------------------------------------------------------------------------------------------- 2. the atlas
def pitched(frame, slack=13):
    """the frame as a view with slack bytes behind every row, at an odd base address"""
    rows, cols = frame.shape[:2]
    buf = np.zeros(rows * (cols * 3 + slack) + 1, np.uint8)
    buf[:] = 0x5A
    view = np.lib.stride_tricks.as_strided(buf[1:], (rows, cols, 3), (cols * 3 + slack, 3, 1))
    view[:] = frame
    assert view.ctypes.data % 2 == 1
    return buf, view


def edge_rois(rows, cols, cell):
    """regions over every edge and a corner, wholly outside, inside, at each level for cells of `cell` pixels"""
    out = [(-10, 5, 30, 20), (cols - 15, 8, 30, 22), (20, -9, 25, 30), (30, rows - 11, 26, 28), (-7, -6, 20, 20), (cols - 9, rows - 8, 21, 19),
           (cols + 5, 10, 20, 20), (-500, -500, 30, 30), (10, rows + 1, 8, 8)]
    for level in LEVELS:
        s = fit(level, cell)
        out += [(cols // 3 - s // 2, rows // 2 - s // 2, s, max(s - 3, 1)), (-s // 2, rows - s // 3, max(s - 1, 1), s)]
    out.append((0, 0, 4 * cell + 40, 4 * cell + 9))         # cropped
    return out


@pytest.mark.parametrize("shape", ((96, 128), (200, 240), (97, 131)))
def test_atlas_equals_the_reference_byte_for_byte(shape):
    """97 x 131 is no multiple of 4: the last blocks of the x1/2 and x1/4 levels are clamped box means"""
    rows, cols = shape
    rng = np.random.default_rng(rows * 1000 + cols)
    frame = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    keep, view = pitched(frame)
    for vw, vh, grid in ((64, 48, 4), (32, 16, 2), (448, 448, 4), (448, 448, 2), (448, 448, 1)):
        rois = edge_rois(rows, cols, vw // grid)
        for mz in (1, 4):
            want = rr.atlas(frame, rois, vw, vh, grid, mz)
            for src in (frame, view):
                got = roi_atlas_host(src, rois, vw, vh, grid, mz)
                assert got.shape == want.shape and np.array_equal(got, want), (shape, vw, vh, grid, mz)
            cells = rr.plan(rois, vw, vh, grid, mz)
            assert set(cells[:, 4].tolist()) >= ({-2, -1, 0} if mz == 1 else set(LEVELS)), (vw, grid)
    # a region wholly outside the frame, its cell's context included, is all zero; unused cells of the last pass are zero
    got = roi_atlas_host(frame, [(cols + 60, 10, 20, 20), (-500, -500, 30, 30), (10, rows + 70, 8, 8)], 64, 48, 4)
    assert got.shape == (1, 48, 64, 3) and not got.any()
    got = roi_atlas_host(frame, [(10, 10, 16, 12)], 64, 48, 4, 1)
    assert got[0, :12, :16].any() and not got[0, 12:].any() and not got[0, :, 16:].any()
    assert np.array_equal(got[0, :12, :16], frame[10:22, 10:26])
    assert roi_atlas_host(frame, [], 64, 48).shape == (0, 48, 64, 3)


def test_atlas_leaves_the_bytes_behind_a_row_untouched():
    lib = _lib.load_library()
    frame = np.random.default_rng(3).integers(0, 256, (96, 128, 3), dtype=np.uint8)
    rois = edge_rois(96, 128, 16)[:20]
    arr = (_lib.rf_roi * len(rois))(*[_lib.rf_roi(*r) for r in rois])
    dstep = 3 * 64 + 5
    dst = np.full(2 * 48 * dstep, 0xAB, np.uint8)
    assert lib.rf_roi_atlas_host(C.byref(roi_spec(4, 4)), 64, 48, frame.ctypes.data, 96, 128, 384, arr, len(rois), dst.ctypes.data, dstep) == 0
    body = dst.reshape(2 * 48, dstep)
    assert np.array_equal(body[:, :192].reshape(2, 48, 64, 3), rr.atlas(frame, rois, 64, 48, 4, 4)) and (body[:, 192:] == 0xAB).all()


# ---------------------------------------------------------------------------------------------- 3. the face rule
def check_map(f, rois, p, grid=0, max_zoom=0, view=(448, 448)):
    got = roi_map_face(f, rois, p, view[0], view[1], grid, max_zoom)
    want = rr.map_face(f, rr.plan(rois, view[0], view[1], grid, max_zoom), p, view[0], view[1], grid)
    assert (got is None) == (want is None), (f[:5], got, want)
    if got is not None:
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1], (f[:5], got, want)
    return got


def test_map_face_every_level_and_the_borders():
    # one region per level in cells of 112 (grid 4, max_zoom 4): 28, 56, 112, 224 and 448 px wide, and one cropped
    rois = [(100, 50, 28, 25), (301, 77, 56, 51), (-20, 500, 112, 100), (1000, 1001, 223, 224), (33, 35, 447, 300), (5, 5, 600, 900)]
    cells = rr.plan(rois, 448, 448, 4, 4)
    assert list(cells[:, 4]) == [2, 1, 0, -1, -2, -2] and cells[5, 7] == ROI_CROPPED
    rng = np.random.default_rng(7)
    kept = 0
    for r in range(6):
        cx, cy = 112 * (r % 4), 112 * (r // 4)
        for _ in range(40):
            x, y, s = cx + rng.uniform(-5, 117), cy + rng.uniform(-5, 117), rng.uniform(4, 60)
            f = face(np.float32(x - s / 2), np.float32(y - s / 2), np.float32(s), np.float32(s * 1.25), np.float32(0.9))
            kept += check_map(f, rois, 0, 4, 4) is not None
    assert 60 < kept < 240
    # a centre exactly on a cell border belongs to the cell that starts there; exactly on a region's lower border it is kept, on its
    # upper border it is dropped
    lvl0 = [(200, 300, 112, 112), (0, 0, 112, 112)]
    on_border = face(np.float32(112 - 10), np.float32(40), np.float32(20), np.float32(20), np.float32(0.8))
    got = check_map(on_border, lvl0, 0, 4, 1)
    assert got is not None and got[1] == 1
    lower = face(np.float32(-10), np.float32(-10), np.float32(20), np.float32(20), np.float32(0.8))          # centre (0, 0) of cell 0
    got = check_map(lower, lvl0, 0, 4, 1)
    assert got is not None and got[1] == 0 and got[0][1] == np.float32(190)
    small = [(200, 300, 100, 100)]                         # the cell shows [194, 306) x [294, 406): the region's upper border is at cell pixel 106
    upper = face(np.float32(106 - 10), np.float32(50), np.float32(20), np.float32(20), np.float32(0.8))
    inside = face(np.float32(105.5 - 10), np.float32(50), np.float32(20), np.float32(20), np.float32(0.8))
    assert check_map(upper, small, 0, 4, 1) is None and check_map(inside, small, 0, 4, 1) is not None
    # a NaN coordinate drops the face (a comparison with a NaN is false); a face in an unused cell is dropped
    for i in (1, 2, 3, 4):
        bad = on_border.copy()
        bad[i] = np.nan
        assert check_map(bad, lvl0, 0, 4, 1) is None
    unused = face(np.float32(250), np.float32(250), np.float32(20), np.float32(20), np.float32(0.8))
    assert check_map(unused, lvl0, 0, 4, 1) is None
    # the second pass of 17 regions holds region 16 in cell 0
    many = [(10 * i, 5 * i, 100, 100) for i in range(17)]
    got = check_map(face(np.float32(40), np.float32(40), np.float32(30), np.float32(30), np.float32(0.7)), many, 1, 4, 1)
    assert got is not None and got[1] == 16
    # huge and infinite coordinates
    for v in (1e9, -1e9, 3e38, np.inf, -np.inf):
        bad = on_border.copy()
        bad[3] = np.float32(v)
        check_map(bad, lvl0, 0, 4, 1)


# ---------------------------------------------------------------------------------------------- 4. regions from faces, the merge
def scattered_faces(seed, n, span=1100):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        s = rng.uniform(8, 180)
        out.append(face(np.float32(rng.uniform(-20, span)), np.float32(rng.uniform(-20, span)), np.float32(s), np.float32(s * rng.uniform(0.8, 1.4)),
                        np.float32(rng.uniform(0.5, 1))))
    return out


def test_regions_from_faces_equal_the_reference():
    faces = scattered_faces(1, 60)
    odd = faces[0].copy(); odd[1] = np.nan
    empty = faces[1].copy(); empty[3] = empty[1] - 1
    far = faces[2].copy(); far[1:5] = (4e6, 0, 4e6 + 5, 5)
    faces = faces + [odd, empty, far]
    for scale, margin in ((1.0, 0.25), (2.857, 0.5), (0.35, None), (1.0, 1.0), (1.0, 1 / 256)):       # None: the C default, a quarter
        got = rois_from_faces(faces, scale, margin)
        want = rr.from_faces(np.stack(faces), scale, int(round((margin or 0) * 256)))
        assert got == want and len(got) == 60, (scale, margin)
    x, y, w, h = rois_from_faces([face(np.float32(10.5), np.float32(20.25), np.float32(40), np.float32(50), np.float32(0.9))])[0]
    assert (x, y, w, h) == (-2, 7, 65, 76)                  # the longer side is 50: 12.5 px on every side, floored and ceiled
    assert rois_from_faces([]) == []


def pass_faces(rois, seed, per_region=3, grid=4, max_zoom=2):
    """constructed faces of the views of `rois`: per region a few that sit inside it (as the view shows them), plus strays"""
    cells = rr.plan(rois, 448, 448, grid, max_zoom)
    g = grid or 4
    cw = 448 // g
    rng = np.random.default_rng(seed)
    passes = [[] for _ in range(rr.passes_of(len(rois), grid))]
    for r, c in enumerate(cells):
        p, cell = divmod(r, g * g)
        cj, ci = divmod(cell, g)
        for k in range(per_region):
            # the first face of a region sits on its cell's centre: two equal regions see it at the same place, and the merge joins them
            s = rng.uniform(6, cw / 2) if k else cw / 4
            x, y = (ci * cw + rng.uniform(0, cw), cj * cw + rng.uniform(0, cw)) if k else (ci * cw + cw / 2, cj * cw + cw / 2)
            passes[p].append(face(np.float32(x - s / 2), np.float32(y - s / 2), np.float32(s), np.float32(s), np.float32(rng.uniform(0.5, 1))))
    return [sorted(p, key=lambda f: -f[0]) for p in passes]


@pytest.mark.parametrize("grid,vote", ((4, False), (4, True), (2, False), (1, True)))
def test_merge_equals_the_reference(grid, vote):
    base = scattered_faces(5, 21, 900)
    rois = rois_from_faces(base)[:21 if grid > 1 else 5]
    rois += [rois[0], (rois[1][0] + 3, rois[1][1] - 2, rois[1][2], rois[1][3])]           # two regions that see the same faces
    passes = pass_faces(rois, 11 + grid, 4, grid)
    for md, mf, cap in ((64, 0, None), (64, 5, None), (3, 0, None), (64, 0, 4)):
        got = roi_merge_host(passes, rois, 448, 448, NMS, md, grid, 0, vote, mf, cap)
        want = rr.merge(rois, passes, 448, 448, NMS, md, grid, 0, vote, mf)
        limit = min(mf or md, cap if cap is not None else md)
        assert got[1] == want[1] and got[0].tobytes() == want[0][:limit].tobytes(), (md, mf, cap)
        assert list(got[2]) == list(want[2][:limit]) and list(got[3]) == list(want[3][:limit])
        assert got[4] == (want[1] > limit or any(len(p) > md for p in passes))
    assert want[4] > want[1] > 0                                # candidates were merged away
    none = roi_merge_host([], [], 448, 448, NMS, 64, grid)
    assert none[1] == 0 and len(none[0]) == 0 and not none[4]


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals():
    lib = _lib.load_library()
    frame = np.zeros((20, 30, 3), np.uint8)
    ok = [(1, 2, 3, 4)]
    for bad in ([(0, 0, 0, 5)], [(0, 0, 5, 0)], [(0, 0, 16385, 5)], [(0, 0, 5, 16385)], [((1 << 20) + 1, 0, 5, 5)], [(0, -(1 << 20) - 1, 5, 5)],
                [(0, 0, 8, 8)] * 257):
        for call in (lambda: roi_plan(bad, 448, 448), lambda: roi_atlas_host(frame, bad, 64, 48),
                     lambda: roi_map_face(np.zeros(15, np.float32), bad, 0, 448, 448),
                     lambda: roi_merge_host([[]] * rr.passes_of(len(bad)), bad, 448, 448, NMS, 8)):
            with pytest.raises(_lib.RFError) as e:
                call()
            assert e.value.status == -1
    for kw in (dict(grid=3), dict(grid=8), dict(grid=-1), dict(max_zoom=3), dict(max_zoom=8)):
        with pytest.raises(_lib.RFError):
            roi_plan(ok, 448, 448, **kw)
    for vw, vh, grid in ((450, 448, 4), (448, 450, 4), (56, 448, 4), (30, 16, 2), (0, 16, 1), (4100, 16, 1)):      # cells of 112.5, 14, 15 px ...
        with pytest.raises(_lib.RFError):
            roi_plan(ok, vw, vh, grid)
    with pytest.raises(_lib.RFError):
        roi_map_face(np.zeros(15, np.float32), ok, 1, 448, 448)          # pass outside the plan
    arr = (_lib.rf_roi * 1)(_lib.rf_roi(1, 2, 3, 4))
    cells = (_lib.rf_roi_cell * 1)()
    for field, value in (("struct_size", 20), ("vote", 3), ("vote", -1), ("max_faces", 4097), ("max_faces", -1), ("reserved", 1)):
        sp = roi_spec()
        setattr(sp, field, value)
        cells[0].level = 77
        assert lib.rf_roi_plan(C.byref(sp), 448, 448, arr, 1, cells, None) == -1 and cells[0].level == 77, field
    assert lib.rf_roi_plan(None, 448, 448, arr, 1, cells, None) == 0 and cells[0].level == 1          # a NULL spec: the defaults
    dst = np.full(64 * 48 * 3, 0xAB, np.uint8)
    for args in ((frame.ctypes.data, 20, 30, 89, dst.ctypes.data, 192), (frame.ctypes.data, 20, 30, 90, dst.ctypes.data, 191),
                 (None, 20, 30, 90, dst.ctypes.data, 192), (frame.ctypes.data, 20, 30, 90, None, 192), (frame.ctypes.data, 0, 30, 90, dst.ctypes.data, 192)):
        s, r, c, st, d, ds = args
        assert lib.rf_roi_atlas_host(None, 64, 48, s, r, c, st, arr, 1, d, ds) == -1
    assert (dst == 0xAB).all()
    with pytest.raises(_lib.RFError):
        rois_from_faces([np.zeros(15, np.float32)], coord_scale=0.0)
    for margin in (-0.5, 0.0, 0.001):                     # 0 / 256 would silently mean the default
        with pytest.raises(_lib.RFError):
            rois_from_faces([np.zeros(15, np.float32)], margin=margin)


# ---------------------------------------------------------------------------------------------- 6. the claim, through the CPU oracle
CLAIM_THR, CLAIM_MARGIN, CLAIM_SHIFT = 0.6, 0.25, 6
CLAIM_WORST_IOU = 0.864                                        # measured with roi_ref's views through the fp32 oracle; the assertion is this less 0.05


def claim_regions(full):
    """the regions of the claim: the full-resolution faces grown by a quarter and moved by (6, 6), as after a small pan"""
    return [(x + CLAIM_SHIFT, y + CLAIM_SHIFT, w, h) for x, y, w, h in rois_from_faces(full, 1.0, CLAIM_MARGIN)]


def check_claim(full, kept, src, floor):
    """one face per region, none lost and none extra, each at the full-resolution box of its region's face"""
    assert sorted(src) == list(range(len(full))), (sorted(src), len(full))
    worst = 1.0
    for f, r in zip(kept, src):
        iou = rr.tta_ref.iou_plus1(f[1:5], full[r][1:5])
        worst = min(worst, iou)
        assert iou >= floor, (r, iou)
    return worst


def test_six_faces_from_one_atlas_through_the_oracle(oracles, base_frame):
    """The claim: mnet25, net 448, threshold 0.6.  The 896 x 1280 base frame holds six faces of 115 to 149 px; the oracle finds them
    at full resolution (net 896 x 1280).  Their regions (rois_from_faces, margin 0.25, moved by (6, 6)) are packed into ONE 448 x 448
    view at grid 4 (five at x1/2, one at x1/4); the oracle detects that view, the face rule maps the faces back: one face per region,
    none lost, none extra.  Measured: scores 0.962 to 0.998, worst IoU to the full-resolution box 0.864; asserted: 0.814."""
    oracle = oracles["mnet25"]
    full = oracle.detect(base_frame, CLAIM_THR, NMS, net_hw=base_frame.shape[:2]).rows()
    assert len(full) == 6
    rois = claim_regions(full)
    cells = roi_plan(rois, 448, 448, 4)[0]
    view = roi_atlas_host(base_frame, rois, 448, 448, 4)
    assert view.shape == (1, 448, 448, 3) and np.array_equal(view, rr.atlas(base_frame, rois, 448, 448, 4))
    faces = oracle.detect(view[0], CLAIM_THR, NMS, net_hw=NET).rows()
    got = roi_merge_host([faces], rois, 448, 448, NMS, 64, 4)
    want = rr.merge(rois, [faces], 448, 448, NMS, 64, 4)
    assert got[0].tobytes() == want[0].tobytes() and list(got[3]) == list(want[3])
    print("levels:", list(cells[:, 4]), "view faces:", len(faces), "scores:", np.round(np.sort(got[0][:, 0]), 3), "src:", list(got[3]))
    worst = check_claim(full, got[0], [int(s) for s in got[3]], CLAIM_WORST_IOU - 0.05)
    print("worst IoU to the full-resolution box: %.3f, lowest score %.3f" % (worst, got[0][:, 0].min()))


# ---------------------------------------------------------------------------------------------- 7. the sanitizer program
def test_plan_atlas_and_map_under_address_and_ub_sanitizers(tmp_path):
    """tests/csrc/test_roi_host.cpp: a few hundred random plans, atlases into exactly-sized heap buffers and mappings over roi.h alone;
    host code only, built with -fsanitize=address,undefined.  No GPU and no library: roi.h is compiled into the program."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")                        # for <hip/hip_runtime.h>, which roi.h includes
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "test_roi_host")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "test_roi_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
