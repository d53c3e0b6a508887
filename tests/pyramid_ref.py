"""numpy restatement of zoom-pyramid detection ("Zoom-pyramid detection"): a helper, not a test.

A frame is detected at 1x (the passes of its tile plan) and as net-sized tiles of the frame enlarged 2x and / or 4x by an integer
bilinear zoom with half-pixel centres, so that faces below the smallest anchor reach the net at a size it knows.  A face of a zoom
tile passes the tile edge rule against the virtual (enlarged) frame, is moved into the virtual frame with one fp32 add and into the
source frame with one exact fp32 multiply and one fp32 subtract per coordinate; the faces of all passes are merged by the voting
merge of flip TTA on the total order (score, g = p * max_det + k).  The kernels (retinaface_amd/csrc/kernels.hip zoom_tile_kernel,
pass_gather_kernel<PyrMap>, vote_merge_kernel), retinaface_amd/csrc/pyramid.h and the host entry points rf_pyramid_plan / rf_pyramid_map_face /
rf_pyramid_merge_host / rf_zoom_host are checked byte for byte against this file.
"""
import numpy as np

import tile_ref
import tta_ref

f32 = np.float32
MERGE_CAP = 4096          # candidates per frame the device merge holds
MAX_PASSES = 1024
MAX_ZOOM_BYTES = 1 << 30  # zoom tiles of one call, each rounded up to 256 bytes
ZOOMS = (1, 2, 4)         # bit b of `levels` selects ZOOMS[b]


def plan(rows, cols, net_h, net_w, levels=0, overlap=0, full_frame=True):
    """(passes, 5) int32 of z, x0, y0, tw, th in the level's virtual pixels: the 1x passes of tile_ref.plan (its full-frame pass
    included), then the tiles of the 2x virtual frame, then those of the 4x one, without full-frame passes"""
    levels = levels or 3
    if not 1 <= levels <= 7:
        raise ValueError("levels must be in [1, 7]")
    if rows <= 0 or cols <= 0:
        return np.array([[1, 0, 0, 0, 0]], np.int32)
    out = []
    for b, z in enumerate(ZOOMS):
        if levels >> b & 1:
            ov, _ = tile_ref.resolve(net_h, net_w, overlap)
            xs, ys = tile_ref.axis(z * cols, net_w, ov), tile_ref.axis(z * rows, net_h, ov)
            if len(out) + len(xs) * len(ys) > MAX_PASSES:
                raise ValueError("more than 1024 passes")
            out += [(z,) + tuple(int(v) for v in t) for t in tile_ref.plan(z * rows, z * cols, net_h, net_w, overlap, full_frame and z == 1)]
    if len(out) > MAX_PASSES:
        raise ValueError("more than 1024 passes")
    if zoom_bytes(out) > MAX_ZOOM_BYTES:
        raise ValueError("zoom tiles above 1 GiB")
    return np.array(out, np.int32).reshape(-1, 5)


def zoom_bytes(passes):
    return sum((int(tw) * int(th) * 3 + 255) // 256 * 256 for z, _, _, tw, th in passes if z > 1)


def is_full(p, rows, cols, net_h, net_w):
    """a 1x pass that is the whole of a frame larger than the net: the full-frame pass"""
    z, x0, y0, tw, th = (int(v) for v in p)
    return z == 1 and (tw > net_w or th > net_h)


def zoom_axis(n, z, X0, count):
    """per output index X0 .. X0 + count - 1 of an axis of source length n enlarged z times: (i0, i1, w), w in units of 1 / 2z"""
    X = np.arange(X0, X0 + count, dtype=np.int64)
    D = 2 * z
    num = 2 * X + 1 - z
    i0 = num // D                      # floor, also below zero
    w = num - i0 * D
    return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), w


def zoom(frame, z, x0=0, y0=0, tw=None, th=None):
    """Z[y0 : y0 + th, x0 : x0 + tw] of Z = the frame enlarged z (2 or 4) times: bilinear with half-pixel centres in integers,
    clamped at the FRAME border"""
    rows, cols = frame.shape[:2]
    tw = z * cols - x0 if tw is None else tw
    th = z * rows - y0 if th is None else th
    D = 2 * z
    shift = 2 * (D.bit_length() - 1)
    xa, xb, wx = zoom_axis(cols, z, x0, tw)
    ya, yb, wy = zoom_axis(rows, z, y0, th)
    F = frame.astype(np.int64)
    wx = wx[None, :, None]
    wy = wy[:, None, None]
    a, b = F[ya][:, xa], F[ya][:, xb]
    c, d = F[yb][:, xa], F[yb][:, xb]
    acc = ((D - wx) * a + wx * b) * (D - wy) + ((D - wx) * c + wx * d) * wy
    return np.ascontiguousarray(((acc + D * D // 2) >> shift).astype(np.uint8))


def images(frame, passes):
    """the image of every pass: 1x passes as ROI views of the frame, zoom tiles as dense frames of their own"""
    out = []
    for z, x0, y0, tw, th in (tuple(int(v) for v in p) for p in passes):
        out.append(frame[y0:y0 + th, x0:x0 + tw] if z == 1 else zoom(frame, z, x0, y0, tw, th))
    return out


def map_face(face, p, rows, cols, net_h, net_w, levels=0, overlap=0, edge=0, full_frame=True):
    """edge rule and mapping of one face (15 float32) of pass p of the plan: the mapped row, or None when dropped"""
    _, ed = tile_ref.resolve(net_h, net_w, overlap, edge)
    z, x0, y0, tw, th = (int(v) for v in plan(rows, cols, net_h, net_w, levels, overlap, full_frame)[p])
    f = np.asarray(face, np.float32).copy()
    if is_full((z, x0, y0, tw, th), rows, cols, net_h, net_w):
        f[1:] = f[1:] * tile_ref.frame_scale(rows, cols, net_h, net_w)
        return f
    x1, y1, x2, y2 = f[1:5]
    if x0 > 0 and x1 < f32(ed):
        return None
    if y0 > 0 and y1 < f32(ed):
        return None
    if x0 + tw < z * cols and x2 > f32(tw - 1 - ed):
        return None
    if y0 + th < z * rows and y2 > f32(th - 1 - ed):
        return None
    fx, fy = f32(x0), f32(y0)
    xs, ys = [1, 3, 5, 6, 7, 8, 9], [2, 4, 10, 11, 12, 13, 14]
    f[xs] = f[xs] + fx
    f[ys] = f[ys] + fy
    if z > 1:
        inv, off = f32(1) / f32(z), f32(z - 1) / f32(2 * z)
        f[1:] = f[1:] * inv - off
    return f


def candidates(rows, cols, passes, net_h, net_w, max_det, levels=0, overlap=0, edge=0, full_frame=True):
    """the surviving faces of all passes of one frame, mapped: (rows (c, 15) float32, g (c,) int64) with g = p * max_det + k"""
    out, gs = [], []
    if rows > 0 and cols > 0:
        for p, faces in enumerate(passes):
            faces = np.asarray(faces, np.float32).reshape(-1, 15)[:max_det]
            for k, f in enumerate(faces):
                m = map_face(f, p, rows, cols, net_h, net_w, levels, overlap, edge, full_frame)
                if m is not None:
                    out.append(m)
                    gs.append(p * max_det + k)
    return (np.stack(out) if out else np.zeros((0, 15), np.float32)), np.array(gs, np.int64)


def merge(rows, cols, passes, net_h, net_w, nms_threshold, max_det, levels=0, overlap=0, edge=0, full_frame=True, max_faces=0,
          vote_on=True):
    """one frame: (faces (k, 15) float32 in merge order, k = min(count, max_faces); count: the true number of heads; votes (k,) int32;
    src_pass (k,) int32; the number of surviving candidates).  passes[p]: the result of pass p of the plan."""
    cand, g = candidates(rows, cols, passes, net_h, net_w, max_det, levels, overlap, edge, full_frame)
    return tta_ref.merge_candidates(cand, g, nms_threshold, max_det, vote_on, max_faces) + (len(cand),)


def mosaic(base):
    """the test frame: the padded base frame averaged over 8 x 8 blocks, (sum + 32) >> 6, placed 3 x 3: 336 x 480, 54 faces of 11 to
    14 px"""
    b = base.astype(np.uint32)
    h, w = b.shape[0] // 8, b.shape[1] // 8
    small = ((b[:h * 8, :w * 8].reshape(h, 8, w, 8, 3).sum(axis=(1, 3)) + 32) >> 6).astype(np.uint8)
    return np.ascontiguousarray(np.tile(small, (3, 3, 1)))
