"""numpy restatement of fisheye detection ("Fisheye detection"): a helper, not a test.

A dewarper holds V views of view_w x view_h pixels (multiples of 16).  Each view has a mesh of (view_h / 16 + 1) x (view_w / 16 + 1)
nodes: the source x and y, in 1/256 px, of view pixel (16 i, 16 j).  Between the nodes everything is integer arithmetic: a pixel's
source position is the bilinear blend of its cell's nodes (4-bit weights), the pixel the blend of four source taps (5-bit weights), a
face is moved back through the same mesh with 12-bit weights.  The plan (lens model -> mesh) is float64.  The faces of all views are
merged by the flip-TTA merge (tests/tta_ref.py) with g = view * max_det + j.  The kernels (retinaface_amd/csrc/kernels.hip
dewarp_views_kernel, pass_gather_kernel<DewarpMap>, vote_merge_kernel), retinaface_amd/csrc/dewarp.h and the host entry points
rf_dewarp_host / rf_dewarp_map_face / rf_dewarp_merge_host are checked byte for byte against this file, rf_dewarp_plan to one unit.
"""
import numpy as np

import tta_ref
from tile_ref import frame_scale

f32 = np.float32
f64 = np.float64
NODE_MAX = 1 << 22
EQUIDISTANT, EQUISOLID, STEREOGRAPHIC, ORTHOGRAPHIC = 0, 1, 2, 3


class Refused(ValueError):
    pass


# ------------------------------------------------------------------------------------------------ the plan (float64)
def radius(model, f, theta):
    if model == EQUISOLID:
        return 2.0 * f * np.sin(theta / 2.0)
    if model == STEREOGRAPHIC:
        return 2.0 * f * np.tan(theta / 2.0)
    if model == ORTHOGRAPHIC:
        return f * np.sin(theta)
    return f * theta


def rotation(yaw, pitch, roll):
    """R = Rz(yaw) Rx(pitch) Rz(roll), degrees"""
    def rz(a):
        c, s = np.cos(np.radians(a)), np.sin(np.radians(a))
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], f64)

    def rx(a):
        c, s = np.cos(np.radians(a)), np.sin(np.radians(a))
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], f64)
    return rz(yaw) @ rx(pitch) @ rz(roll)


def source_of(model, f, cx, cy, view, view_w, view_h, X, Y):
    """the exact source position (float64 x, y) of view pixels (X, Y) (arrays) of the view (yaw, pitch, roll, hfov); raises Refused for
    an angle the model cannot image"""
    yaw, pitch, roll, hfov = view
    fv = (view_w / 2.0) / np.tan(np.radians(hfov) / 2.0)
    a = (np.asarray(X, f64) - (view_w - 1) / 2.0) / fv
    b = (np.asarray(Y, f64) - (view_h - 1) / 2.0) / fv
    d = np.tensordot(rotation(yaw, pitch, roll), np.stack([a, b, np.ones_like(a)]), axes=1)
    theta = np.arctan2(np.hypot(d[0], d[1]), d[2])
    psi = np.arctan2(d[1], d[0])
    if (theta >= (np.pi / 2 if model == ORTHOGRAPHIC else np.pi)).any():
        raise Refused("a view reaches an angle the lens model cannot image")
    r = radius(model, f, theta)
    return cx + r * np.cos(psi), cy + r * np.sin(psi)


def ring(n, pitch, hfov):
    return [(360.0 * j / n, pitch, 0.0, hfov) for j in range(n)]


def plan(model, f, cx, cy, views, view_w, view_h):
    """(V, ny, nx, 2) int64 meshes; raises Refused as the C plan does"""
    ys, xs = np.meshgrid(np.arange(view_h // 16 + 1) * 16.0, np.arange(view_w // 16 + 1) * 16.0, indexing="ij")
    out = []
    for v in views:
        sx, sy = source_of(model, f, cx, cy, v, view_w, view_h, xs, ys)
        m = np.stack([np.rint(256.0 * sx), np.rint(256.0 * sy)], -1)
        if (np.abs(m) > NODE_MAX).any():
            raise Refused("a node lies beyond +-2^22")
        out.append(m.astype(np.int64))
    return np.stack(out)


def view_of(model, f, cx, cy, view, view_w, view_h, x, y):
    """the inverse of source_of for the equidistant model: the view position (float64 X, Y) of frame positions (x, y) and whether the
    view's camera sees them (in front of it)"""
    assert model == EQUIDISTANT
    yaw, pitch, roll, hfov = view
    fv = (view_w / 2.0) / np.tan(np.radians(hfov) / 2.0)
    dx, dy = np.asarray(x, f64) - cx, np.asarray(y, f64) - cy
    theta, psi = np.hypot(dx, dy) / f, np.arctan2(dy, dx)
    d = np.stack([np.sin(theta) * np.cos(psi), np.sin(theta) * np.sin(psi), np.cos(theta)])
    a, b, z = np.tensordot(rotation(yaw, pitch, roll).T, d, axes=1)
    front = (z > 1e-9) & (theta < np.pi)
    z = np.where(front, z, 1.0)
    return a / z * fv + (view_w - 1) / 2.0, b / z * fv + (view_h - 1) / 2.0, front


def poster_scene(posters, size, f, views, view_w, view_h):
    """A synthetic size x size equidistant fisheye frame (centre ((size - 1) / 2,) * 2): view j of `views` looks straight at poster j, a
    (view_h, view_w, 3) uint8 picture sampled bilinearly in float64; everything else is black."""
    c = (size - 1) / 2.0
    ys, xs = np.meshgrid(np.arange(size, dtype=f64), np.arange(size, dtype=f64), indexing="ij")
    out = np.zeros((size, size, 3), f64)
    for view, pic in zip(views, posters):
        X, Y, front = view_of(EQUIDISTANT, f, c, c, view, view_w, view_h, xs, ys)
        inside = front & (X >= 0) & (X <= view_w - 1) & (Y >= 0) & (Y <= view_h - 1)
        x0, y0 = np.clip(np.floor(X).astype(int), 0, view_w - 2), np.clip(np.floor(Y).astype(int), 0, view_h - 2)
        wx, wy = (X - x0)[..., None], (Y - y0)[..., None]
        p = pic.astype(f64)
        val = (p[y0, x0] * (1 - wx) + p[y0, x0 + 1] * wx) * (1 - wy) + (p[y0 + 1, x0] * (1 - wx) + p[y0 + 1, x0 + 1] * wx) * wy
        out = np.where(inside[..., None], val, out)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the pixel rule
def pixel_sources(mesh_view, view_w, view_h):
    """(qx, qy), each (view_h, view_w) int64: the source position of every view pixel in 1/32 px"""
    m = np.asarray(mesh_view, np.int64).reshape(view_h // 16 + 1, view_w // 16 + 1, 2)
    Y, X = np.meshgrid(np.arange(view_h), np.arange(view_w), indexing="ij")
    cx, cy, u, v = X >> 4, Y >> 4, X & 15, Y & 15
    out = []
    for k in range(2):
        n = m[..., k]
        s = n[cy, cx] * (16 - u) * (16 - v) + n[cy, cx + 1] * u * (16 - v) + n[cy + 1, cx] * (16 - u) * v + n[cy + 1, cx + 1] * u * v
        assert (np.abs(s) < 2 ** 31).all()
        out.append((s + 1024) >> 11)
    return out


def warp(frame, mesh_view, view_w, view_h):
    """one view of a (rows, cols, 3) uint8 frame"""
    rows, cols = frame.shape[:2]
    qx, qy = pixel_sources(mesh_view, view_w, view_h)
    x0, y0, wx, wy = qx >> 5, qy >> 5, qx & 31, qy & 31
    src = frame.astype(np.int64)
    acc = np.zeros((view_h, view_w, 3), np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = x0 + dx, y0 + dy
            inside = (x >= 0) & (x < cols) & (y >= 0) & (y < rows)
            tap = np.where(inside[..., None], src[np.clip(y, 0, rows - 1), np.clip(x, 0, cols - 1)], 0)
            w = (wx if dx else 32 - wx) * (wy if dy else 32 - wy)
            acc += tap * w[..., None]
    return ((acc + 512) >> 10).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the face rule
def quant(p, dim):
    """a scaled float32 view coordinate as an integer in 1/256 px, clamped to one cell beyond the view; a NaN becomes the lower bound"""
    lo, hi = f32(-4096), f32(256 * dim + 4096)
    with np.errstate(invalid="ignore"):
        pq = f32(p) * f32(256)
        c = pq if pq > lo else lo
        c = c if c < hi else hi
    return int(np.rint(f32(c)))


def map_point(mesh_view, view_w, view_h, qx, qy):
    """the source position (ints, 1/256 px) of the view point (qx, qy), 1/256 px"""
    m = np.asarray(mesh_view, np.int64).reshape(view_h // 16 + 1, view_w // 16 + 1, 2)
    cx = min(max(qx >> 12, 0), view_w // 16 - 1)
    cy = min(max(qy >> 12, 0), view_h // 16 - 1)
    u, v = qx - 4096 * cx, qy - 4096 * cy
    out = []
    for k in range(2):
        s = (int(m[cy, cx, k]) * (4096 - u) * (4096 - v) + int(m[cy, cx + 1, k]) * u * (4096 - v) + int(m[cy + 1, cx, k]) * (4096 - u) * v
             + int(m[cy + 1, cx + 1, k]) * u * v)
        out.append((s + (1 << 23)) >> 24)
    return out


def map_face(face, mesh_view, view_w, view_h, net_h, net_w, edge=0):
    """edge rule and mapping of one face (15 float32) of a view: the mapped face, or None when the edge rule drops it"""
    f = np.asarray(face, np.float32).copy()
    with np.errstate(invalid="ignore"):
        f[1:] = f[1:] * frame_scale(view_h, view_w, net_h, net_w)
        if edge > 0 and (f[1] < f32(edge) or f[2] < f32(edge) or f[3] > f32(view_w - 1 - edge) or f[4] > f32(view_h - 1 - edge)):
            return None
    inv = f32(1) / f32(256)
    x1, y1, x2, y2 = quant(f[1], view_w), quant(f[2], view_h), quant(f[3], view_w), quant(f[4], view_h)
    xm, ym = (x1 + x2) >> 1, (y1 + y2) >> 1
    pts = [map_point(mesh_view, view_w, view_h, x, y) for x, y in ((x1, y1), (xm, y1), (x2, y1), (x1, ym), (x2, ym), (x1, y2), (xm, y2), (x2, y2))]
    out = f.copy()
    out[1], out[2] = f32(min(p[0] for p in pts)) * inv, f32(min(p[1] for p in pts)) * inv
    out[3], out[4] = f32(max(p[0] for p in pts)) * inv, f32(max(p[1] for p in pts)) * inv
    for i in range(5):
        rx, ry = map_point(mesh_view, view_w, view_h, quant(f[5 + i], view_w), quant(f[10 + i], view_h))
        out[5 + i], out[10 + i] = f32(rx) * inv, f32(ry) * inv
    return out


# ------------------------------------------------------------------------------------------------ the merge
def candidates(mesh, view_w, view_h, passes, net_h, net_w, max_det, edge=0):
    """the mapped faces of all views of one frame: (rows (c, 15) float32, g (c,) int64) with g = view * max_det + j"""
    out, gs = [], []
    assert len(passes) == len(mesh)
    for v, faces in enumerate(passes):
        faces = np.asarray(faces, np.float32).reshape(-1, 15)[:max_det]
        for j, f in enumerate(faces):
            m = map_face(f, mesh[v], view_w, view_h, net_h, net_w, edge)
            if m is not None:
                out.append(m)
                gs.append(v * max_det + j)
    return (np.stack(out) if out else np.zeros((0, 15), np.float32)), np.array(gs, np.int64)


def merge(mesh, view_w, view_h, passes, net_h, net_w, nms_threshold, max_det, vote_on=False, max_faces=0, edge=0):
    """one frame: (faces (k, 15) float32 in merge order, k = min(count, max_faces); count: the true number of heads; votes (k,) int32;
    src_view (k,) int32; the number of candidates).  passes[v]: the result of view v, at most max_det faces in score order."""
    cand, g = candidates(mesh, view_w, view_h, passes, net_h, net_w, max_det, edge)
    return tta_ref.merge_candidates(cand, g, nms_threshold, max_det, vote_on, max_faces) + (len(cand),)
