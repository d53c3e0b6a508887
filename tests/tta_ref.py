"""numpy restatement of flip test-time augmentation ("Flip test-time augmentation"): a helper, not a test.

A frame is detected as it is (pass 0) and mirrored left-right (pass 1).  Every face is moved into source-frame pixels with one fp32
multiply per coordinate; a face of the mirrored pass is moved back with one fp32 subtract per x coordinate and a swap of the left /
right landmark pairs.  The faces of both passes are merged by the detector's greedy NMS on a total order, and with voting each kept
head becomes the score-weighted mean of the candidates it suppressed, accumulated in float64 in the total order.  The kernels
(retinaface_amd/csrc/kernels.hip mirror_rows_kernel, pass_gather_kernel<TtaMap>, vote_merge_kernel), retinaface_amd/csrc/tta.h and the host
entry points rf_tta_map_face / rf_tta_merge_host are checked byte for byte against this file.
"""
import numpy as np

from tile_ref import frame_scale, iou_plus1  # noqa: F401  (the same float; re-exported)

f32 = np.float32
f64 = np.float64
MERGE_CAP = 4096          # candidates per frame the device merge holds
PERM = (1, 0, 2, 4, 3)    # left eye <-> right eye, left mouth corner <-> right mouth corner


def mirror(frame):
    """pass 1 of a frame: M[y][x] = F[y][cols - 1 - x]"""
    return np.ascontiguousarray(frame[:, ::-1])


def map_face(face, p, rows, cols, net_h, net_w):
    """the mapping of one face (15 float32: score, box, 5 x, 5 y) of pass p"""
    f = np.asarray(face, np.float32).copy()
    f[1:] = f[1:] * frame_scale(rows, cols, net_h, net_w)
    if p == 0:
        return f
    c = f32(cols - 1)
    out = f.copy()
    out[1] = c - f[3]
    out[3] = c - f[1]
    for i in range(5):
        out[5 + i] = c - f[5 + PERM[i]]
        out[10 + i] = f[10 + PERM[i]]
    return out


def candidates(rows, cols, passes, net_h, net_w, max_det):
    """the mapped faces of all passes of one frame: (rows (c, 15) float32, g (c,) int64) with g = p * max_det + k"""
    out, gs = [], []
    for p, faces in enumerate(passes):
        faces = np.asarray(faces, np.float32).reshape(-1, 15)[:max_det]
        for k, f in enumerate(faces):
            out.append(map_face(f, p, rows, cols, net_h, net_w))
            gs.append(p * max_det + k)
    return (np.stack(out) if out else np.zeros((0, 15), np.float32)), np.array(gs, np.int64)


def clusters(cand, g, nms_threshold):
    """greedy NMS on the total order (score descending by bit order, g ascending) with the reference's rule (+1-pixel areas and
    intersections, skipped when w <= 0 or h <= 0, strict > threshold; float32, one rounding per operation).  Returns a list of
    clusters in merge order, each the indices into cand of its members in the total order, head first."""
    thr = f32(nms_threshold)
    bits = cand[:, 0].view(np.uint32).astype(np.int64)
    order = np.lexsort((g, -bits))
    b = cand[order, 1:5]
    n = len(order)
    alive = np.ones(n, bool)
    one = f32(1)
    area = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    out = []
    for i in range(n):
        if not alive[i]:
            continue
        members = [order[i]]
        rest = np.nonzero(alive[i + 1:])[0] + i + 1
        if len(rest):
            r = b[rest]
            x = np.maximum(b[i, 0], r[:, 0])
            y = np.maximum(b[i, 1], r[:, 1])
            w = np.minimum(b[i, 2], r[:, 2]) - x + one
            h = np.minimum(b[i, 3], r[:, 3]) - y + one
            ok = ~((w <= 0) | (h <= 0))
            inter = w * h
            with np.errstate(all="ignore"):
                iou = inter / (area[i] + area[rest] - inter)
            gone = rest[ok & (iou > thr)]
            alive[gone] = False
            members += [order[j] for j in gone]
        out.append(members)
    return out


def vote(cand, members):
    """the score-weighted mean of a cluster: the head's score, every coordinate (float32)(acc / sw) with both sums in float64 over the
    members in the total order, head first, one rounding per add (the product of two float32 is exact in float64)"""
    s = cand[members, 0].astype(f64)
    v = cand[members, 1:].astype(f64)
    out = cand[members[0]].copy()
    sw, acc = s[0], s[0] * v[0]
    for m in range(1, len(members)):
        sw = sw + s[m]
        acc = acc + s[m] * v[m]
    out[1:] = (acc / sw).astype(f32)
    return out


def merge_candidates(cand, g, nms_threshold, max_det, vote_on=True, max_faces=0):
    """(faces (k, 15) float32 in merge order, k = min(count, max_faces); count: the true number of heads; votes (k,) int32;
    src_pass (k,) int32)"""
    mf = max_faces or max_det
    cl = clusters(cand, g, nms_threshold) if len(cand) else []
    faces = [vote(cand, m) if vote_on else cand[m[0]] for m in cl[:mf]]
    return ((np.stack(faces) if faces else np.zeros((0, 15), np.float32)), len(cl), np.array([len(m) for m in cl[:mf]], np.int32),
            np.array([g[m[0]] // max_det for m in cl[:mf]], np.int32))


def merge(rows, cols, passes, net_h, net_w, nms_threshold, max_det, vote_on=True, max_faces=0):
    """one frame: merge_candidates' tuple plus the number of candidates.  passes[p]: the result of pass p, at most max_det faces in
    score order; two passes, or one with flip off."""
    cand, g = candidates(rows, cols, passes, net_h, net_w, max_det)
    return merge_candidates(cand, g, nms_threshold, max_det, vote_on, max_faces) + (len(cand),)
