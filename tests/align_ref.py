"""numpy restatement of the 5-point face alignment the engine computes ("Face alignment"): a helper, not a test.

Everything real is IEEE double with + - * / only, in the order written below (numpy never contracts into FMA); everything
after the sample coordinates is integer.  The kernel (retinaface_amd/csrc/kernels.hip, align_kernel) and rf_align_matrix are
checked byte for byte against this file.
"""
import numpy as np

TEMPLATE_X = (38.2946, 73.5318, 56.0252, 41.5493, 70.7299)      # left eye, right eye, nose, mouth left, mouth right @ 112 px
TEMPLATE_Y = (51.6963, 51.5014, 71.7366, 92.3655, 92.2041)


def estimate(face, cs=1.0, size=112):
    """face: 15 floats (score, box, px[5], py[5]) as float32.  cs: the float32 coordinate scale.
    Returns (valid, fwd[6] float64, (ia, ib, mp_x, mp_y, mq_x, mq_y))."""
    f = np.asarray(face, np.float32)
    c = np.float64(np.float32(cs))
    px = [np.float64(f[5 + i]) * c for i in range(5)]
    py = [np.float64(f[10 + i]) * c for i in range(5)]
    return estimate_points(px, py, size)


def estimate_points(px, py, size=112):
    """The same from five source points already in float64 (P_i of the definition)."""
    px = [np.float64(v) for v in px]
    py = [np.float64(v) for v in py]
    k = np.float64(size) / np.float64(112.0)
    qx = [np.float64(t) * k for t in TEMPLATE_X]
    qy = [np.float64(t) * k for t in TEMPLATE_Y]
    zero = np.float64(0.0)
    with np.errstate(all="ignore"):
        mpx = mpy = mqx = mqy = zero
        for i in range(5):
            mpx = mpx + px[i]; mpy = mpy + py[i]; mqx = mqx + qx[i]; mqy = mqy + qy[i]
        five = np.float64(5.0)
        mpx = mpx / five; mpy = mpy / five; mqx = mqx / five; mqy = mqy / five
        sxx = sxy = n2 = zero
        for i in range(5):
            a = px[i] - mpx; b = py[i] - mpy; cc = qx[i] - mqx; d = qy[i] - mqy
            sxx = sxx + (a * cc + b * d)
            sxy = sxy + (a * d - b * cc)
            n2 = n2 + (a * a + b * b)
        A = sxx / n2
        B = sxy / n2
        D = A * A + B * B
        if not (np.isfinite(n2) and n2 > 0 and np.isfinite(D) and D > 0):
            return False, np.zeros(6, np.float64), None
        fwd = np.array([A, -B, mqx - (A * mpx - B * mpy), B, A, mqy - (B * mpx + A * mpy)], np.float64)
        ia = A / D
        ib = -B / D
    return True, fwd, (ia, ib, mpx, mpy, mqx, mqy)


def align_matrix(face, cs=1.0, size=112):
    ok, fwd, _ = estimate(face, cs, size)
    return ok, fwd


def crop(frame, face, cs=1.0, size=112):
    """frame: H x W x 3 uint8 (any strides).  Returns (size x size x 3 uint8 crop, fwd[6] float64)."""
    S = int(size)
    out = np.zeros((S, S, 3), np.uint8)
    ok, fwd, inv = estimate(face, cs, S)
    if not ok:
        return out, fwd
    ia, ib, mpx, mpy, mqx, mqy = inv
    rows, cols = frame.shape[:2]
    with np.errstate(all="ignore"):
        du = np.arange(S, dtype=np.float64)[None, :] - mqx
        dv = np.arange(S, dtype=np.float64)[:, None] - mqy
        x = (ia * du - ib * dv) + mpx
        y = (ib * du + ia * dv) + mpy
        inside = (x > -2) & (x < np.float64(cols + 1)) & (y > -2) & (y < np.float64(rows + 1))
        xs = np.where(inside, x, 0.0)
        ys = np.where(inside, y, 0.0)
        X = np.floor(xs * 1024.0 + 0.5).astype(np.int64)
        Y = np.floor(ys * 1024.0 + 0.5).astype(np.int64)
    x0, fx = X >> 10, X & 1023
    y0, fy = Y >> 10, Y & 1023
    acc = np.zeros((S, S, 3), np.int64)
    for dy, wy in ((0, 1024 - fy), (1, fy)):
        for dx, wx in ((0, 1024 - fx), (1, fx)):
            xx, yy = x0 + dx, y0 + dy
            tap = inside & (xx >= 0) & (xx < cols) & (yy >= 0) & (yy < rows)
            pix = frame[np.where(tap, yy, 0), np.where(tap, xx, 0)].astype(np.int64)
            acc += np.where(tap, wx * wy, 0)[:, :, None] * pix
    out[:] = ((acc + (1 << 19)) >> 20).astype(np.uint8)
    out[~inside] = 0
    return out, fwd


def crops(frame, faces, cs=1.0, size=112):
    """(k, size, size, 3) crops and (k, 6) matrices of the rows of `faces`."""
    faces = np.asarray(faces, np.float32).reshape(-1, 15)
    cr = np.zeros((len(faces), size, size, 3), np.uint8)
    ms = np.zeros((len(faces), 6), np.float64)
    for i, f in enumerate(faces):
        cr[i], ms[i] = crop(frame, f, cs, size)
    return cr, ms
