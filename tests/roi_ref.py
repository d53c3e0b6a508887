"""numpy restatement of region detection ("Region detection"): a helper, not a test.

A caller names up to 256 regions (x, y, w, h; int source pixels) of a frame.  A view of view_w x view_h pixels is cut into grid x grid
cells; region r goes to cell r mod grid^2 (row-major) of pass r // grid^2 and is shown there at the largest of the five steps x4, x2,
x1, x1/2, x1/4 (level 2 .. -2) not above max_zoom at which it fits the cell, centred, with the real pixels around it.  A face of a view
belongs to the cell its box centre lies in, is moved into the frame with one float32 add and, off level 0, one exact multiply and one
add per coordinate, and is kept only when its mapped centre lies inside its region.  The faces of all passes are merged by the flip-TTA
merge (tests/tta_ref.py) with g = region * max_det + j.  The kernels (retinaface_amd/csrc/kernels.hip roi_atlas_kernel,
pass_gather_kernel<RoiMap>, vote_merge_kernel), retinaface_amd/csrc/roi.h and the host entry points rf_roi_plan / rf_roi_atlas_host /
rf_roi_map_face / rf_roi_from_faces / rf_roi_merge_host are checked byte for byte against this file.
"""
import math

import numpy as np

import pyramid_ref
import tta_ref

f32 = np.float32
CROPPED = 1
MAX_REGIONS, MAX_SIDE, MAX_ORIGIN = 256, 16384, 1 << 20


def resolve(grid=0, max_zoom=0):
    return grid or 4, max_zoom or 2


def passes_of(n, grid=0):
    g = resolve(grid)[0]
    return -(-n // (g * g))


# ------------------------------------------------------------------------------------------------ the plan
def plan_one(roi, cw, ch, max_zoom=0):
    """(level, x0, y0, flags) of one region in a cell of cw x ch pixels"""
    x, y, w, h = (int(v) for v in roi)
    mz = resolve(0, max_zoom)[1]
    level, flags = None, 0
    for l in (2, 1, 0, -1, -2):
        if l > 0 and (1 << l) > mz:
            continue
        fits = (w << l <= cw and h << l <= ch) if l >= 0 else (w <= cw << -l and h <= ch << -l)
        if fits:
            level = l
            break
    if level is None:
        level, flags = -2, CROPPED
    cx2, cy2 = 2 * x + w, 2 * y + h
    if level >= 0:
        z = 1 << level
        return level, (cx2 * z - cw) // 2, (cy2 * z - ch) // 2, flags             # // floors, also below zero
    k = 1 << -level
    return level, (cx2 - k * cw) // (2 * k), (cy2 - k * ch) // (2 * k), flags


def plan(rois, view_w, view_h, grid=0, max_zoom=0):
    """(n, 8) int32 rows of x, y, w, h, level, x0, y0, flags"""
    g = resolve(grid)[0]
    assert view_w % g == 0 and view_h % g == 0 and (view_w // g) % 4 == 0
    out = [tuple(int(v) for v in r) + plan_one(r, view_w // g, view_h // g, max_zoom) for r in rois]
    return np.array(out, np.int32).reshape(len(out), 8)


# ------------------------------------------------------------------------------------------------ the pixel rule
def shrink(frame, k):
    """the frame at x1/k: the rounded mean of every k x k block, source coordinates clamped into the frame"""
    rows, cols = frame.shape[:2]
    lr, lc = -(-rows // k), -(-cols // k)
    ys = np.minimum(np.arange(lr * k), rows - 1)
    xs = np.minimum(np.arange(lc * k), cols - 1)
    big = frame.astype(np.int64)[ys][:, xs]
    acc = big.reshape(lr, k, lc, k, 3).sum(axis=(1, 3))
    return ((acc + k * k // 2) // (k * k)).astype(np.uint8)


def level_window(frame, level, X0, Y0, w, h):
    """pixels [Y0, Y0 + h) x [X0, X0 + w) of the frame's level image; outside the image: 0"""
    rows, cols = frame.shape[:2]
    if level > 0:
        lr, lc = rows << level, cols << level
    elif level == 0:
        lr, lc = rows, cols
    else:
        lr, lc = -(-rows >> -level), -(-cols >> -level)
    out = np.zeros((h, w, 3), np.uint8)
    xa, xb, ya, yb = max(X0, 0), min(X0 + w, lc), max(Y0, 0), min(Y0 + h, lr)
    if xa >= xb or ya >= yb:
        return out
    if level > 0:
        part = pyramid_ref.zoom(frame, 1 << level, xa, ya, xb - xa, yb - ya)
    elif level == 0:
        part = frame[ya:yb, xa:xb]
    else:
        part = shrink(frame, 1 << -level)[ya:yb, xa:xb]
    out[ya - Y0:yb - Y0, xa - X0:xb - X0] = part
    return out


def atlas(frame, rois, view_w, view_h, grid=0, max_zoom=0):
    """(passes, view_h, view_w, 3) uint8: the views of one frame's regions"""
    g = resolve(grid)[0]
    cw, ch = view_w // g, view_h // g
    cells = plan(rois, view_w, view_h, grid, max_zoom)
    out = np.zeros((passes_of(len(cells), g), view_h, view_w, 3), np.uint8)
    for r, c in enumerate(cells):
        p, cell = divmod(r, g * g)
        cj, ci = divmod(cell, g)
        out[p, cj * ch:(cj + 1) * ch, ci * cw:(ci + 1) * cw] = level_window(frame, int(c[4]), int(c[5]), int(c[6]), cw, ch)
    return out


# ------------------------------------------------------------------------------------------------ the face rule
MUL_ADD = {2: (f32(0.25), f32(-0.375)), 1: (f32(0.5), f32(-0.25)), -1: (f32(2), f32(0.5)), -2: (f32(4), f32(1.5))}
IS_X = np.array([False, True, False, True, False] + [True] * 5 + [False] * 5)


def map_face(face, cells, p, view_w, view_h, grid=0):
    """the face rule for one face (15 float32) of pass p of the frame whose cell records are `cells` (plan()): (the mapped face, its
    region), or None when it is dropped"""
    g = resolve(grid)[0]
    cw, ch = view_w // g, view_h // g
    f = np.asarray(face, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        cx, cy = (f[1] + f[3]) * f32(0.5), (f[2] + f[4]) * f32(0.5)
        ci = sum(1 for k in range(1, g) if cx >= f32(k * cw))
        cj = sum(1 for k in range(1, g) if cy >= f32(k * ch))
        cell = cj * g + ci
        r = p * g * g + cell
        if r >= len(cells):
            return None
        x, y, w, h, level, x0, y0, _ = (int(v) for v in cells[r])
        out = f.copy()
        out[1:] = f[1:] + np.where(IS_X[1:], f32(x0 - ci * cw), f32(y0 - cj * ch)).astype(np.float32)
        if level != 0:
            mul, add = MUL_ADD[level]
            out[1:] = out[1:] * mul
            out[1:] = out[1:] + add
        mx, my = (out[1] + out[3]) * f32(0.5), (out[2] + out[4]) * f32(0.5)
        if not (mx >= f32(x) and mx < f32(x + w) and my >= f32(y) and my < f32(y + h)):
            return None
    return out, r


def from_faces(faces, coord_scale=1.0, margin_q8=0):
    """the regions of faces ((k, 15) float32): the box times coord_scale (float32), grown by margin_q8 / 256 of its longer side
    (float64), floored / ceiled; faces whose box is not finite, is empty or lies beyond +-2^20 are skipped"""
    mq = margin_q8 or 64
    out = []
    for f in np.asarray(faces, np.float32).reshape(-1, 15):
        with np.errstate(invalid="ignore", over="ignore"):
            b = f[1:5] * f32(coord_scale)
        if not all(-MAX_ORIGIN <= v <= MAX_ORIGIN for v in b):
            continue
        b = [float(v) for v in b]
        if not (b[2] >= b[0] and b[3] >= b[1]):
            continue
        m = max(b[2] - b[0], b[3] - b[1]) * float(mq) / 256.0
        x1, y1, x2, y2 = math.floor(b[0] - m), math.floor(b[1] - m), math.ceil(b[2] + m), math.ceil(b[3] + m)
        if x1 < -MAX_ORIGIN or y1 < -MAX_ORIGIN:
            continue
        out.append((x1, y1, min(max(x2 - x1, 1), MAX_SIDE), min(max(y2 - y1, 1), MAX_SIDE)))
    return out


# ------------------------------------------------------------------------------------------------ the merge
def candidates(rois, passes, view_w, view_h, max_det, grid=0, max_zoom=0):
    """the kept faces of all passes of one frame, mapped: (rows (c, 15) float32, g (c,) int64) with g = region * max_det + j"""
    cells = plan(rois, view_w, view_h, grid, max_zoom)
    assert len(passes) == passes_of(len(cells), grid)
    out, gs = [], []
    for p, faces in enumerate(passes):
        faces = np.asarray(faces, np.float32).reshape(-1, 15)[:max_det]
        for j, f in enumerate(faces):
            m = map_face(f, cells, p, view_w, view_h, grid)
            if m is not None:
                out.append(m[0])
                gs.append(m[1] * max_det + j)
    return (np.stack(out) if out else np.zeros((0, 15), np.float32)), np.array(gs, np.int64)


def merge(rois, passes, view_w, view_h, nms_threshold, max_det, grid=0, max_zoom=0, vote_on=False, max_faces=0):
    """one frame: (faces (k, 15) float32 in merge order, k = min(count, max_faces); count: the true number of heads; votes (k,) int32;
    src_roi (k,) int32; the number of candidates).  passes[p]: the result of pass p, at most max_det faces in score order."""
    cand, g = candidates(rois, passes, view_w, view_h, max_det, grid, max_zoom)
    return tta_ref.merge_candidates(cand, g, nms_threshold, max_det, vote_on, max_faces) + (len(cand),)
