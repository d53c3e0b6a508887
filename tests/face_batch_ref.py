"""numpy restatement of the face batches the engine computes ("Face batches"): a helper, not a test.

A face batch is the aligned faces of one call as one dense tensor.  The crop values come from align_ref (untouched); this file
adds the packed order and the map from a u8 crop value to an output element: one float32 subtract, one float32 multiply (numpy
never contracts them), then round-to-nearest-even to float16.  The kernel (retinaface_amd/csrc/kernels.hip, face_batch_kernel)
and rf_face_value_table are checked byte for byte against this file.
"""
import numpy as np

import align_ref

U8_HWC, F16_CHW, F32_CHW = 0, 1, 2
DTYPES = {U8_HWC: np.uint8, F16_CHW: np.float16, F32_CHW: np.float32}
FORMAT_OF = {"u8": U8_HWC, "f16": F16_CHW, "f32": F32_CHW}


def resolve(mean=None, scale=None):
    """(mean[3], scale[3]) float32 per output channel; all three scale entries 0 (or None) = (v - 127.5) / 128"""
    k = np.broadcast_to(np.asarray(0.0 if scale is None else scale, np.float32), (3,)).copy()
    m = np.broadcast_to(np.asarray(0.0 if mean is None else mean, np.float32), (3,)).copy()
    if not k.any():
        m[:], k[:] = np.float32(127.5), np.float32(1.0) / np.float32(128.0)
    return m, k


def value_table(fmt, channel, mean=None, scale=None):
    """the 256 output values of output channel `channel`, in the format's element type"""
    q = np.arange(256, dtype=np.uint8)
    if fmt == U8_HWC:
        return q
    m, k = resolve(mean, scale)
    f = (q.astype(np.float32) - np.float32(m[channel])) * np.float32(k[channel])
    return f.astype(np.float16) if fmt == F16_CHW else f


def offsets(counts, max_faces):
    off = np.zeros(len(counts) + 1, np.int64)
    for i, c in enumerate(counts):
        off[i + 1] = off[i] + min(int(c), int(max_faces))
    return off


def convert(crops, fmt, rgb=0, mean=None, scale=None):
    """(k, S, S, 3) u8 BGR crops -> the (k, S, S, 3) / (k, 3, S, S) block of the tensor"""
    crops = np.asarray(crops, np.uint8)
    src = crops[..., ::-1] if rgb else crops                    # output channel c = source channel 2 - c / c
    if fmt == U8_HWC:
        return np.ascontiguousarray(src)
    out = np.zeros((len(crops), 3) + crops.shape[1:3], DTYPES[fmt])
    for c in range(3):
        out[:, c] = value_table(fmt, c, mean, scale)[src[..., c]]
    return out


def batch(frames, faces, fmt, *, size=112, rgb=0, mean=None, scale=None, max_faces=4096, capacity=None, scales=None):
    """frames[i]: H x W x 3 u8 (None = an empty frame), faces[i]: (k_i, 15) float32.  Returns (tensor [min(total, capacity), ...],
    matrices [.., 6] float64, offsets [n + 1] -- the true numbers, not clamped)."""
    per_c, per_m = [], []
    counts = []
    for i, f in enumerate(frames):
        rows = np.asarray(faces[i], np.float32).reshape(-1, 15)[:max_faces]
        if f is None:
            rows = rows[:0]
        counts.append(len(rows))
        cr, ms = (align_ref.crops(f, rows, 1.0 if scales is None else scales[i], size) if len(rows)
                  else (np.zeros((0, size, size, 3), np.uint8), np.zeros((0, 6), np.float64)))
        per_c.append(cr)
        per_m.append(ms)
    off = offsets(counts, max_faces)
    cr = np.concatenate(per_c) if per_c else np.zeros((0, size, size, 3), np.uint8)
    ms = np.concatenate(per_m) if per_m else np.zeros((0, 6), np.float64)
    keep = int(off[-1]) if capacity is None else min(int(off[-1]), int(capacity))
    return convert(cr[:keep], fmt, rgb, mean, scale), ms[:keep], off
