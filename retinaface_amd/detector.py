"""Host-side mirror of the reference's ``RetinaFace`` class (retinaface/RetinaFace.h:63-78) over the C ABI.

Same constructor arguments (model directory, network preset, NMS threshold), same two entry points --
``detect(img, threshold)`` and ``detectBatchImages(imgs, threshold)`` -- taking OpenCV-style ``uint8``
H x W x 3 BGR arrays.  Unlike the reference, which returns ``void`` and drops its result
(RetinaFace.cpp:726-747), the detections are returned.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple as _namedtuple
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import (rf_face, rf_face_batch_spec, rf_face_gate, rf_face_quality, rf_options, rf_overlay_spec, rf_redact_spec, rf_tile_spec, rf_track,
                   rf_change_spec, rf_dewarp_spec, rf_enhance_spec, rf_roi, rf_roi_cell, rf_roi_spec, rf_motion_spec, rf_pyramid_spec, rf_rot_spec, rf_shot, rf_track_motion, rf_track_spec, rf_track_tag, rf_tta_spec,
                   rf_follow_spec, rf_track_follow)

PRECISION_FP32, PRECISION_FP16, PRECISION_INT8 = 0, 1, 2


@dataclass
class Detection:
    """FaceDetectInfo (RetinaFace.h:37-42) + the global anchor index that produced it."""
    score: float
    rect: tuple            # x1, y1, x2, y2 in network-input pixels
    xs: tuple              # 5 landmark x
    ys: tuple              # 5 landmark y
    anchor_index: int

    def as_row(self) -> np.ndarray:
        return np.array([self.score, *self.rect, *self.xs, *self.ys], dtype=np.float32)


def _face_rows(faces) -> np.ndarray:
    """(k, 15) float32 rows from an array, a list of rows or a list of Detection."""
    if isinstance(faces, np.ndarray):
        if faces.dtype.names:                          # rf_face records (FACE_DTYPE)
            return np.ascontiguousarray(faces).view(np.float32).reshape(-1, 15)
        return np.ascontiguousarray(faces, np.float32).reshape(-1, 15)
    rows = [f.as_row() if isinstance(f, Detection) else np.asarray(f, np.float32) for f in faces]
    return np.stack(rows).astype(np.float32).reshape(-1, 15) if rows else np.zeros((0, 15), np.float32)


def align_matrix(face, coord_scale: float = 1.0, crop_size: int = 112):
    """rf_align_matrix (host only, no GPU): (valid, forward matrix) of one face -- a Detection or 15 floats (score, box,
    5 landmark x, 5 landmark y).  The matrix maps source-frame pixels to crop pixels, row-major 2 x 3 float64; it is all zero
    for an invalid face (landmarks that do not span a plane)."""
    lib = _lib.load_library()
    row = _face_rows([face])[0]
    f = rf_face.from_buffer_copy(row.tobytes())
    m = (C.c_double * 6)()
    st = lib.rf_align_matrix(C.byref(f), float(coord_scale), int(crop_size), m)
    if st < 0:
        raise _lib.RFError(st, "rf_align_matrix: bad argument (crop_size must be in [16, 512])")
    return bool(st), np.array(m, np.float64).reshape(2, 3)


_FACE_FORMATS = {"u8": (_lib.RF_FACES_U8_HWC, np.uint8), "f16": (_lib.RF_FACES_F16_CHW, np.float16),
                 "f32": (_lib.RF_FACES_F32_CHW, np.float32)}


def face_batch_spec(crop_size: int = 112, dtype: str = "f16", rgb: bool = True, mean=None, scale=None, max_faces: int = 0,
                    capacity: int = 1, antialias: bool = False, aa_max: int = 0) -> rf_face_batch_spec:
    """An rf_face_batch_spec: dtype "u8" (HWC), "f16" or "f32" (CHW); mean / scale: one number or three, per OUTPUT channel
    (both None = (v - 127.5) / 128); max_faces 0 = the engine's max_detections; antialias: supersample faces larger than their crop
    with up to aa_max (1, 2, 4, 8; 0 = 4) sub-samples per axis (face_aa_factor gives a face's factor)."""
    if dtype not in _FACE_FORMATS:
        raise ValueError('dtype must be "u8", "f16" or "f32"')
    sp = rf_face_batch_spec()
    sp.struct_size = C.sizeof(rf_face_batch_spec)
    sp.crop_size, sp.format, sp.rgb = int(crop_size), _FACE_FORMATS[dtype][0], 1 if rgb else 0
    if scale is not None:
        m = np.broadcast_to(np.asarray(0.0 if mean is None else mean, np.float32), (3,))
        k = np.broadcast_to(np.asarray(scale, np.float32), (3,))
        sp.mean, sp.scale = (C.c_float * 3)(*m), (C.c_float * 3)(*k)
    elif mean is not None:
        raise ValueError("mean without scale")
    sp.max_faces, sp.capacity = int(max_faces), int(capacity)
    sp.antialias, sp.aa_max = 1 if antialias else 0, int(aa_max)
    return sp


def face_aa_factor(face, coord_scale: float = 1.0, crop_size: int = 112, aa_max: int = 0) -> int:
    """rf_face_aa_factor (host only, no GPU): the supersampling factor per axis (1, 2, 4 or 8; 1 for an invalid face) an antialiased
    face batch gives this face -- a Detection or 15 floats -- with this aa_max (0 = 4)."""
    lib = _lib.load_library()
    f = rf_face.from_buffer_copy(_face_rows([face])[0].tobytes())
    k = lib.rf_face_aa_factor(C.byref(f), float(coord_scale), int(crop_size), int(aa_max))
    if k < 0:
        raise _lib.RFError(k, "rf_face_aa_factor: bad argument (crop_size must be 0 or in [16, 512], aa_max 0, 1, 2, 4 or 8)")
    return int(k)


def face_batch_plan(counts: Sequence[int], *, crop_size: int = 112, dtype: str = "f16", max_faces: int = 0, capacity: int = 1):
    """rf_face_batch_plan (host only, no GPU): (total, offsets[n + 1], bytes_per_face) of a call that finds counts[i] faces in
    image i; total is not clamped to the capacity."""
    lib = _lib.load_library()
    sp = face_batch_spec(crop_size, dtype, max_faces=max_faces, capacity=capacity)
    n = len(counts)
    cnt = (C.c_int * max(n, 1))(*[int(c) for c in counts])
    off = (C.c_int * (n + 1))()
    bpf = C.c_size_t()
    total = lib.rf_face_batch_plan(C.byref(sp), cnt, n, off, C.byref(bpf))
    if total < 0:
        raise _lib.RFError(int(total), "rf_face_batch_plan: bad spec or a negative count")
    return int(total), np.array(off[:n + 1], np.int32), int(bpf.value)


def face_value_table(channel: int, *, dtype: str = "f16", rgb: bool = True, mean=None, scale=None) -> np.ndarray:
    """rf_face_value_table (host only, no GPU): the 256 output values of one output channel, as the kernel computes them."""
    lib = _lib.load_library()
    sp = face_batch_spec(112, dtype, rgb, mean, scale)
    out = np.zeros(256, _FACE_FORMATS[dtype][1])
    st = lib.rf_face_value_table(C.byref(sp), int(channel), out.ctypes.data)
    if st < 0:
        raise _lib.RFError(st, "rf_face_value_table: bad spec or channel")
    return out


# one rf_face_quality record (64 bytes)
QUALITY_DTYPE = np.dtype([("flags", "<i4"), ("covered", "<i4"), ("sum_luma", "<i8"), ("sum_lap", "<i8"), ("sum_lap2", "<i8"),
                          ("sharpness", "<f8"), ("iod2", "<f8"), ("yaw", "<f8"), ("sin2_roll", "<f8")])
_GATE_FIELDS = ("min_sharpness", "min_iod", "max_abs_yaw", "max_sin2_roll", "min_covered", "min_luma", "max_luma")


def face_gate(**kw) -> rf_face_gate:
    """An rf_face_gate.  Keywords (each 0 / absent = that gate is off): min_sharpness (variance of the luma Laplacian of the crop),
    min_iod (eye distance in source pixels), max_abs_yaw (nose offset along the eye axis, in eye distances), max_sin2_roll,
    min_covered (fraction of the crop sampled inside the frame), min_luma / max_luma (mean luma of the crop)."""
    g = rf_face_gate()
    g.struct_size = C.sizeof(rf_face_gate)
    for k, v in kw.items():
        if k not in _GATE_FIELDS:
            raise TypeError(f"face_gate: unknown field {k!r}")
        setattr(g, k, float(v))
    return g


def _as_gate(gate):
    if gate is None or isinstance(gate, rf_face_gate):
        return gate
    return face_gate(**gate)


def face_pose(face, coord_scale: float = 1.0, crop_size: int = 112) -> np.ndarray:
    """rf_face_pose (host only, no GPU): a QUALITY_DTYPE record with the landmark numbers of one face (iod2, yaw, sin2_roll) and
    flags = RF_GATE_INVALID for an invalid face; the image numbers are 0."""
    lib = _lib.load_library()
    f = rf_face.from_buffer_copy(_face_rows([face])[0].tobytes())
    q = np.zeros(1, QUALITY_DTYPE)
    st = lib.rf_face_pose(C.byref(f), float(coord_scale), int(crop_size), q.ctypes.data_as(C.POINTER(rf_face_quality)))
    if st < 0:
        raise _lib.RFError(st, "rf_face_pose: bad argument (crop_size must be 0 or in [16, 512])")
    return q[0]


def face_gate_eval(gate, q, crop_size: int = 112) -> int:
    """rf_face_gate_eval (host only, no GPU): the RF_GATE_* flags the gate (an rf_face_gate, a dict of face_gate() keywords or None)
    gives a QUALITY_DTYPE record."""
    lib = _lib.load_library()
    rec = np.array([q], QUALITY_DTYPE) if not (isinstance(q, np.ndarray) and q.dtype == QUALITY_DTYPE) else np.ascontiguousarray(q).reshape(-1)[:1].copy()
    g = _as_gate(gate)
    st = lib.rf_face_gate_eval(C.byref(g) if g is not None else None, rec.ctypes.data_as(C.POINTER(rf_face_quality)), int(crop_size))
    if st < 0:
        raise _lib.RFError(st, "rf_face_gate_eval: bad gate or crop_size")
    return int(st)


def tile_spec(overlap: int = 0, edge: int = 0, full_frame: bool = True, max_faces: int = 0) -> rf_tile_spec:
    """An rf_tile_spec: overlap (minimum overlap of neighbouring tiles in pixels; 0 = a quarter of the net's smaller side, negative =
    none), edge (width of the border band of the edge rule; 0 = 8, negative = 0), full_frame (also run the whole frame shrunk as one
    more pass), max_faces (merged faces kept per frame; 0 = the engine's max_detections)."""
    sp = rf_tile_spec()
    sp.struct_size = C.sizeof(rf_tile_spec)
    sp.overlap, sp.edge, sp.full_frame, sp.max_faces = int(overlap), int(edge), 1 if full_frame else 2, int(max_faces)
    return sp


def tile_plan(rows: int, cols: int, net_h: int, net_w: int, overlap: int = 0, full_frame: bool = True) -> np.ndarray:
    """rf_tile_plan (host only, no GPU): the passes of a rows x cols frame at a net_h x net_w net as a (passes, 4) int32 array of
    x0, y0, tw, th -- the tiles row-major, then the full-frame pass (0, 0, cols, rows) when the plan has one."""
    lib = _lib.load_library()
    sp = tile_spec(overlap, 0, full_frame)
    n = lib.rf_tile_plan(C.byref(sp), int(rows), int(cols), int(net_h), int(net_w), None, 0)
    if n < 0:
        raise _lib.RFError(n, "rf_tile_plan: bad spec, frame or net size, or more than 1024 passes")
    out = np.zeros((n, 4), np.int32)
    lib.rf_tile_plan(C.byref(sp), int(rows), int(cols), int(net_h), int(net_w), out.ctypes.data_as(C.POINTER(C.c_int)), n)
    return out


def tile_map_face(face, t: int, rows: int, cols: int, net_h: int, net_w: int, overlap: int = 0, edge: int = 0, full_frame: bool = True):
    """rf_tile_map_face (host only, no GPU): the face (a Detection or 15 floats) of pass t moved into source-frame pixels as 15
    float32, or None when the edge rule drops it."""
    lib = _lib.load_library()
    sp = tile_spec(overlap, edge, full_frame)
    f = rf_face.from_buffer_copy(_face_rows([face])[0].tobytes())
    g = rf_face()
    st = lib.rf_tile_map_face(C.byref(sp), int(rows), int(cols), int(net_h), int(net_w), int(t), C.byref(f), C.byref(g))
    if st < 0:
        raise _lib.RFError(st, "rf_tile_map_face: bad spec, frame, net size or pass index")
    return _faces_to_array(C.pointer(g), 1)[0] if st else None


FACE_DTYPE = np.dtype([("score", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("px", "<f4", 5), ("py", "<f4", 5)])
TRACK_DTYPE = np.dtype([("id", "<i8"), ("first_frame", "<i8"), ("last_frame", "<i8"), ("best_frame", "<i8"), ("best_value", "<f8"),
                        ("hits", "<i4"), ("missed", "<i4"), ("flags", "<i4"), ("reserved", "<i4"), ("last", FACE_DTYPE), ("best", FACE_DTYPE)])
TRACK_TAG_DTYPE = np.dtype([("id", "<i8"), ("slot", "<i4"), ("hits", "<i4"), ("age", "<i4"), ("flags", "<i4")])
# one rf_shot record (64 bytes)
SHOT_DTYPE = np.dtype([("id", "<i8"), ("frame", "<i8"), ("matrix", "<f8", 6)])


def shot_resolve(max_tracks: int, tags, counts, ended, ended_counts, first_frame: int, records, faces=None, coord_scale=None,
                 crop_size: int = 112):
    """rf_shot_resolve (host only, no GPU): the decisions of the two shot kernels for one stream's n images of one launch.  tags:
    (n, cap_per_image) TRACK_TAG_DTYPE, ended: (n, cap_ended) TRACK_DTYPE, records: (max_tracks,) SHOT_DTYPE before the launch, faces:
    None or (n, cap_per_image, 15) float32.  Returns (delivered, source (n, cap_ended, 3), owner (max_tracks, 2), records after)."""
    lib = _lib.load_library()
    tags = np.ascontiguousarray(tags, TRACK_TAG_DTYPE)
    ended = np.ascontiguousarray(ended, TRACK_DTYPE)
    n, cap = tags.shape
    cap_ended = ended.shape[1]
    rec = np.ascontiguousarray(records, SHOT_DTYPE).copy()
    cnt = (C.c_int * max(n, 1))(*[int(c) for c in counts])
    ec = (C.c_int * max(n, 1))(*[int(c) for c in ended_counts])
    source = np.zeros((max(n, 1), max(cap_ended, 1), 3), np.int32)
    owner = np.zeros((max_tracks, 2), np.int32)
    fr = np.ascontiguousarray(faces, np.float32) if faces is not None else None
    cs = (C.c_float * max(n, 1))(*coord_scale) if coord_scale is not None else None
    st = lib.rf_shot_resolve(int(max_tracks), n, tags.ctypes.data_as(C.POINTER(rf_track_tag)), cap, cnt, ended.ctypes.data_as(C.POINTER(rf_track)),
                             cap_ended, ec, int(first_frame), fr.ctypes.data_as(C.POINTER(rf_face)) if fr is not None else None, cs,
                             int(crop_size), rec.ctypes.data_as(C.POINTER(rf_shot)), source.ctypes.data_as(C.POINTER(C.c_int32)),
                             owner.ctypes.data_as(C.POINTER(C.c_int32)))
    if st < 0:
        raise _lib.RFError(st, "rf_shot_resolve: bad argument")
    return int(st), source[:n, :cap_ended], owner, rec
TRACK_NEW, TRACK_CONFIRMED, TRACK_BEST, TRACK_UNTRACKED, TRACK_OVERFLOW = 1, 2, 4, 8, 16


def track_spec(max_tracks: int = 0, min_iou: float = 0.0, max_missed: int = 0, min_hits: int = 0, new_score: float = 0.0) -> rf_track_spec:
    """rf_track_spec; 0 = the default (64 slots, IoU 0.3, 10 missed frames, 3 hits, every face opens a track)"""
    s = rf_track_spec()
    s.struct_size = C.sizeof(rf_track_spec)
    s.max_tracks, s.min_iou, s.max_missed, s.min_hits, s.new_score = int(max_tracks), float(min_iou), int(max_missed), int(min_hits), float(new_score)
    return s


# one rf_track_motion record (16 bytes)
MOTION_DTYPE = np.dtype([("vx", "<f4"), ("vy", "<f4"), ("samples", "<i4"), ("reserved", "<i4")])


def motion_spec(alpha: float = 0.0, horizon: int = 0) -> rf_motion_spec:
    """rf_motion_spec; 0 = the default (alpha 0.5, horizon 8 frames; a negative horizon never extrapolates)"""
    s = rf_motion_spec()
    s.struct_size = C.sizeof(rf_motion_spec)
    s.alpha, s.horizon, s.reserved = float(alpha), int(horizon), 0
    return s


def _as_motion_spec(spec):
    if spec is None or isinstance(spec, rf_motion_spec):
        return spec
    return motion_spec(**spec)


def track_predict(track, motion, ahead: int = 1, spec=None) -> np.ndarray:
    """rf_track_predict (host only, no GPU): the predicted face (15 float32) of one live track (a TRACK_DTYPE record) with its
    MOTION_DTYPE record, ahead = 0 (where redaction coasts) or 1 (where the next frame step matches); spec: motion_spec() or its
    keywords as a dict."""
    lib = _lib.load_library()
    sp = _as_motion_spec(spec)
    t = rf_track.from_buffer_copy(np.asarray(track, TRACK_DTYPE).tobytes())
    m = rf_track_motion.from_buffer_copy(np.asarray(motion, MOTION_DTYPE).tobytes())
    out = rf_face()
    st = lib.rf_track_predict(C.byref(sp) if sp is not None else None, C.byref(t), C.byref(m), int(ahead), C.byref(out))
    if st < 0:
        raise _lib.RFError(st, "rf_track_predict: free slot, bad spec or argument")
    return np.frombuffer(bytes(out), np.float32).copy()


def track_step(table: np.ndarray, frames: int, next_id: int, faces, coord_scale: float = 1.0, quality=None, max_faces: int = 256,
               cap_ended: Optional[int] = None, motion: Optional[np.ndarray] = None, mspec=None, **spec):
    """rf_track_step (host only, no GPU): one frame step on a caller-held table (TRACK_DTYPE records, updated in place).  Returns
    (tags, ended, frames, next_id, truncated); keywords as track_spec().  motion: a MOTION_DTYPE array of len(table) records (updated
    in place) makes it rf_track_step_motion; mspec: motion_spec() or its keywords as a dict."""
    lib = _lib.load_library()
    sp = track_spec(**spec)
    if motion is not None and (motion.dtype != MOTION_DTYPE or len(motion) != len(table) or not motion.flags.c_contiguous):
        raise ValueError("motion must be a contiguous MOTION_DTYPE array with one record per slot")
    rows = _face_rows(faces)
    count = len(rows)
    cap_ended = len(table) if cap_ended is None else int(cap_ended)
    tags = np.zeros(max(count, 1), TRACK_TAG_DTYPE)
    ended = np.zeros(max(cap_ended, 1), TRACK_DTYPE)
    f, nid, ne = C.c_int64(frames), C.c_int64(next_id), C.c_int(0)
    q = np.ascontiguousarray(quality, QUALITY_DTYPE) if quality is not None else None
    head = (C.byref(sp), table.ctypes.data_as(C.POINTER(rf_track)))
    tail = (C.byref(f), C.byref(nid), rows.ctypes.data_as(C.POINTER(rf_face)), count, float(coord_scale),
            q.ctypes.data_as(C.POINTER(rf_face_quality)) if q is not None else None, int(max_faces),
            tags.ctypes.data_as(C.POINTER(rf_track_tag)), ended.ctypes.data_as(C.POINTER(rf_track)), cap_ended, C.byref(ne))
    if motion is None:
        name, st = "rf_track_step", lib.rf_track_step(*head, *tail)
    else:
        msp = _as_motion_spec(mspec)
        name, st = "rf_track_step_motion", lib.rf_track_step_motion(head[0], C.byref(msp) if msp is not None else None, head[1],
                                                                    motion.ctypes.data_as(C.POINTER(rf_track_motion)), *tail)
    if st < 0 and st != _lib.RF_ERR_TRUNCATED:
        raise _lib.RFError(st, name + ": bad spec or argument")
    return tags[:count], ended[:min(ne.value, cap_ended)], f.value, nid.value, st == _lib.RF_ERR_TRUNCATED


# ---- followed tracks (follow.h): one rf_track_follow record (32 bytes); a template is 32 x 32 bytes
FOLLOW_DTYPE = np.dtype([(k, "<i4") for k in ("valid", "run", "q", "ox", "oy", "sad", "dx", "dy")])
FOLLOW_G = 32
TRACK_FOLLOWED = _lib.RF_TRACK_FOLLOWED


def follow_spec(radius: int = 0, max_mad: int = 0, max_run: int = 0) -> rf_follow_spec:
    """rf_follow_spec; 0 = the default (radius 8 cells, mean absolute difference 16, 8 follow steps between key steps)"""
    s = rf_follow_spec()
    s.struct_size = C.sizeof(rf_follow_spec)
    s.radius, s.max_mad, s.max_run, s.reserved = int(radius), int(max_mad), int(max_run), 0
    return s


def _as_follow_spec(spec):
    if spec is None or isinstance(spec, rf_follow_spec):
        return spec
    return follow_spec(**spec)


def _frame_view(frame):
    """(address, rows, cols, step) of a (rows, cols, 3) u8 view whose pixels are contiguous (rows may be strided); None: no pixels"""
    if frame is None or frame.size == 0:
        return None, 0, 0, 0
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3 or frame.strides[2] != 1 or frame.strides[1] != 3:
        raise ValueError("frame must be a (rows, cols, 3) uint8 view with contiguous pixels")
    return frame.ctypes.data, frame.shape[0], frame.shape[1], frame.strides[0]


def _dense_frame(frame: np.ndarray) -> np.ndarray:
    """The rule of every call that reads a host frame: uint8 H x W x 3; pixels that are not dense (strides[1] != 3) are copied, a row
    pitch is kept.  The caller owns the copy for as long as C reads it."""
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError("frames must be uint8 H x W x 3 (CV_8UC3, BGR)")
    if frame.strides[2] != 1 or frame.strides[1] != 3:
        frame = np.ascontiguousarray(frame)
    return frame


_HostFrames = _namedtuple("_HostFrames", "args keep")


def _host_frames(imgs, in_place: Optional[str] = None) -> _HostFrames:
    """The C arguments of a batch of host frames: args = (ptrs, rows, cols, steps, n), the first four ctypes arrays of max(n, 1)
    entries, and keep = the arrays ptrs points into.  None and zero-size frames become (NULL, 0, 0, 0).

    LIFETIME: ptrs holds raw addresses.  A frame whose pixels are not dense is copied (_dense_frame), and that copy is referenced by
    `keep` ALONE -- so the caller must hold the returned tuple until the C call that was given ptrs has returned.  Passing args on and
    dropping the tuple frees the copy under a host upload that is still reading it.

    in_place ("redacted", "drawn into"): the call writes into the caller's frames, so nothing may be copied -- pixels that are not
    dense and read-only frames are refused."""
    n = len(imgs)
    ptrs = (C.c_void_p * max(n, 1))()
    rows, cols, steps = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))()
    keep = []
    for i, im in enumerate(imgs):
        if im is None or im.size == 0:
            continue                                   # the arrays are zero-initialised
        if in_place is None:
            im = _dense_frame(im)
        elif im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.strides[2] != 1 or im.strides[1] != 3:
            raise ValueError("frames must be uint8 H x W x 3 with dense pixels (CV_8UC3, BGR)")
        elif not im.flags.writeable:
            raise ValueError("frames are %s in place: they must be writeable" % in_place)
        keep.append(im)
        ptrs[i], rows[i], cols[i], steps[i] = im.ctypes.data, im.shape[0], im.shape[1], im.strides[0]
    return _HostFrames((ptrs, rows, cols, steps, n), keep)


def _device_frames(ptrs, rows, cols, steps=None):
    """The C arguments (ptrs, rows, cols, steps; ctypes arrays of max(n, 1) entries) of a batch of frames resident in device memory;
    a pointer may be 0 or None (an empty frame), steps defaults to dense rows (3 * cols)."""
    n = len(ptrs)
    return ((C.c_void_p * max(n, 1))(*ptrs), (C.c_int * max(n, 1))(*rows), (C.c_int * max(n, 1))(*cols),
            (C.c_int * max(n, 1))(*(steps if steps is not None else [3 * x for x in cols])))


def _pack_passes(per_pass_faces, md: int):
    """(flat, pass_counts) of a list of face lists: a (passes, md, 15) float32 block and a ctypes int array.  A list longer than md is
    cut in the block, but its count stays the true length -- the C side reports the truncation from that."""
    rows = [_face_rows(f) for f in per_pass_faces]
    flat = np.zeros((max(len(rows), 1), md, 15), np.float32)
    pass_counts = (C.c_int * max(len(rows), 4))()      # (at least four: the host merges read one count per pass of their spec)
    for p, r in enumerate(rows):
        flat[p, :min(len(r), md)] = r[:md]
        pass_counts[p] = len(r)
    return flat, pass_counts


def _detection(row, anchor_index: int = -1) -> Detection:
    v = row.tolist()
    return Detection(v[0], tuple(v[1:5]), tuple(v[5:10]), tuple(v[10:15]), anchor_index)


def follow_geometry(box):
    """rf_follow_geometry (host only): (q, ox, oy) of a box (x1, y1, x2, y2), or None for an invalid geometry"""
    b = (C.c_float * 4)(*[float(v) for v in box])
    out = (C.c_int32 * 3)()
    st = _lib.load_library().rf_follow_geometry(b, out)
    if st < 0:
        raise _lib.RFError(st, "rf_follow_geometry: bad argument")
    return (out[0], out[1], out[2]) if st else None


def follow_template(frame: np.ndarray, q: int, ox: int, oy: int) -> np.ndarray:
    """rf_follow_template (host only): the (32, 32) u8 template of the lattice (q, ox, oy) in a frame"""
    ptr, rows, cols, step = _frame_view(frame)
    tpl = np.zeros((FOLLOW_G, FOLLOW_G), np.uint8)
    st = _lib.load_library().rf_follow_template(ptr, rows, cols, step, int(q), int(ox), int(oy), tpl.ctypes.data)
    if st < 0:
        raise _lib.RFError(st, "rf_follow_template: bad argument")
    return tpl


def follow_search(frame: np.ndarray, tpl: np.ndarray, q: int, ox: int, oy: int, radius: int = 8):
    """rf_follow_search (host only): (state, sad, du, dv); state 1 = no eligible candidate, 2 = the winner"""
    ptr, rows, cols, step = _frame_view(frame)
    t = np.ascontiguousarray(tpl, np.uint8)
    if t.size != FOLLOW_G * FOLLOW_G:
        raise ValueError("a template is 32 x 32 bytes")
    out = (C.c_int32 * 4)()
    st = _lib.load_library().rf_follow_search(ptr, rows, cols, step, t.ctypes.data, int(q), int(ox), int(oy), int(radius), out)
    if st < 0:
        raise _lib.RFError(st, "rf_follow_search: bad argument")
    return tuple(int(v) for v in out)


def _follow_state(table, records, templates):
    T = len(table)
    if records.dtype != FOLLOW_DTYPE or len(records) != T or not records.flags.c_contiguous:
        raise ValueError("records must be a contiguous FOLLOW_DTYPE array with one record per slot")
    if templates.dtype != np.uint8 or templates.size != T * FOLLOW_G * FOLLOW_G or not templates.flags.c_contiguous:
        raise ValueError("templates must be a contiguous (max_tracks, 32, 32) uint8 array")


def track_step_follow_key(table: np.ndarray, records: np.ndarray, templates: np.ndarray, frames: int, next_id: int, frame, faces,
                          coord_scale: float = 1.0, quality=None, max_faces: int = 256, cap_ended: Optional[int] = None, **spec):
    """rf_track_step_follow_key (host only): track_step() plus the keep rule on caller-held records (FOLLOW_DTYPE) and templates
    ((max_tracks, 32, 32) u8), all updated in place.  Returns (tags, ended, frames, next_id, truncated)."""
    lib = _lib.load_library()
    sp = track_spec(**spec)
    _follow_state(table, records, templates)
    ptr, rows, cols, step = _frame_view(frame)
    fr = _face_rows(faces)
    count = len(fr)
    cap_ended = len(table) if cap_ended is None else int(cap_ended)
    tags = np.zeros(max(count, 1), TRACK_TAG_DTYPE)
    ended = np.zeros(max(cap_ended, 1), TRACK_DTYPE)
    f, nid, ne = C.c_int64(frames), C.c_int64(next_id), C.c_int(0)
    q = np.ascontiguousarray(quality, QUALITY_DTYPE) if quality is not None else None
    st = lib.rf_track_step_follow_key(C.byref(sp), table.ctypes.data_as(C.POINTER(rf_track)), records.ctypes.data_as(C.POINTER(rf_track_follow)),
                                      templates.ctypes.data, C.byref(f), C.byref(nid), ptr, rows, cols, step,
                                      fr.ctypes.data_as(C.POINTER(rf_face)), count, float(coord_scale),
                                      q.ctypes.data_as(C.POINTER(rf_face_quality)) if q is not None else None, int(max_faces),
                                      tags.ctypes.data_as(C.POINTER(rf_track_tag)), ended.ctypes.data_as(C.POINTER(rf_track)), cap_ended, C.byref(ne))
    if st < 0 and st != _lib.RF_ERR_TRUNCATED:
        raise _lib.RFError(st, "rf_track_step_follow_key: bad spec or argument")
    return tags[:count if ptr else 0], ended[:min(ne.value, cap_ended)], f.value, nid.value, st == _lib.RF_ERR_TRUNCATED


def track_step_follow(table: np.ndarray, records: np.ndarray, templates: np.ndarray, frames: int, frame, cap: Optional[int] = None,
                      cap_ended: Optional[int] = None, fspec=None, **spec):
    """rf_track_step_follow (host only): one follow step on caller-held state.  Returns (followed faces (k, 15) float32, tags, count,
    ended, ended_count, frames, truncated); fspec: follow_spec() or its keywords as a dict."""
    lib = _lib.load_library()
    sp = track_spec(**spec)
    fs = _as_follow_spec(fspec)
    _follow_state(table, records, templates)
    ptr, rows, cols, step = _frame_view(frame)
    cap = len(table) if cap is None else int(cap)
    cap_ended = len(table) if cap_ended is None else int(cap_ended)
    out = np.zeros((max(cap, 1), 15), np.float32)
    tags = np.zeros(max(cap, 1), TRACK_TAG_DTYPE)
    ended = np.zeros(max(cap_ended, 1), TRACK_DTYPE)
    f, cnt, ne = C.c_int64(frames), C.c_int(0), C.c_int(0)
    st = lib.rf_track_step_follow(C.byref(sp), C.byref(fs) if fs is not None else None, table.ctypes.data_as(C.POINTER(rf_track)),
                                  records.ctypes.data_as(C.POINTER(rf_track_follow)), templates.ctypes.data, C.byref(f), ptr, rows, cols, step,
                                  out.ctypes.data_as(C.POINTER(rf_face)), tags.ctypes.data_as(C.POINTER(rf_track_tag)), cap, C.byref(cnt),
                                  ended.ctypes.data_as(C.POINTER(rf_track)), cap_ended, C.byref(ne))
    if st < 0 and st != _lib.RF_ERR_TRUNCATED:
        raise _lib.RFError(st, "rf_track_step_follow: bad spec or argument")
    k = min(cnt.value, cap)
    return out[:k], tags[:k], cnt.value, ended[:min(ne.value, cap_ended)], ne.value, f.value, st == _lib.RF_ERR_TRUNCATED


REDACT_PIXELATE, REDACT_FILL = _lib.RF_REDACT_PIXELATE, _lib.RF_REDACT_FILL
REDACT_RECT, REDACT_ELLIPSE = _lib.RF_REDACT_RECT, _lib.RF_REDACT_ELLIPSE


def redact_spec(mode: int = 0, shape: int = 0, cells: int = 0, margin: float = 0.0, fill=(0, 0, 0), max_regions: int = 0,
                coast: int = 0, blur: int = 0) -> rf_redact_spec:
    """rf_redact_spec; 0 = the default (pixelate, rectangle, 8 cells, margin 0.2 -- negative = none, max_detections regions, coast = the
    tracker's max_missed -- negative = no coasting regions).  blur = 1, 2, 3 (pixelate only): the faces are box-blurred with that many
    passes per axis, radius min(cell edge, 64) per region, instead of pixelated."""
    s = rf_redact_spec()
    s.struct_size = C.sizeof(rf_redact_spec)
    s.mode, s.shape, s.cells, s.margin, s.max_regions, s.coast = int(mode), int(shape), int(cells), float(margin), int(max_regions), int(coast)
    s.fill[0], s.fill[1], s.fill[2] = (int(v) for v in fill)
    if not 0 <= int(blur) <= 255:
        raise ValueError("blur must fit a byte (0 = none; 1, 2, 3 = box passes per axis)")
    s.blur = int(blur)
    return s


def _as_redact_spec(spec):
    if spec is None or isinstance(spec, rf_redact_spec):
        return spec
    return redact_spec(**spec)


def redact_region(face, rows: int, cols: int, coord_scale: float = 1.0, **spec):
    """rf_redact_region (host only, no GPU): (valid, [ux0, uy0, ux1, uy1, cx0, cy0, cx1, cy1, c]) of one face; keywords as redact_spec()"""
    lib = _lib.load_library()
    f = rf_face.from_buffer_copy(_face_rows([face])[0].tobytes())
    out = (C.c_int * 9)()
    st = lib.rf_redact_region(C.byref(redact_spec(**spec)), C.byref(f), float(coord_scale), int(rows), int(cols), out)
    if st < 0:
        raise _lib.RFError(st, "rf_redact_region: bad spec or argument")
    return bool(st), np.array(out, np.int32)


def redact_host(img: np.ndarray, faces, coord_scale: float = 1.0, **spec):
    """rf_redact_host (host only, no GPU): redacts a uint8 H x W x 3 array (any row stride) in place at the given faces.  Returns
    (pixels per region, truncated); keywords as redact_spec()."""
    lib = _lib.load_library()
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or (img.size and (img.strides[2] != 1 or img.strides[1] != 3)):
        raise ValueError("the frame must be uint8 H x W x 3 with dense pixels (CV_8UC3, BGR)")
    if not img.flags.writeable:
        raise ValueError("the frame is redacted in place: it must be writeable")
    rows_f = _face_rows(faces)
    k = len(rows_f)
    pixels = np.zeros(max(k, 1), np.int32)
    flat = np.ascontiguousarray(rows_f) if k else np.zeros((1, 15), np.float32)
    st = lib.rf_redact_host(C.byref(redact_spec(**spec)), C.c_void_p(img.ctypes.data if img.size else None), img.shape[0], img.shape[1],
                            img.strides[0] if img.size else 0, flat.ctypes.data_as(C.POINTER(rf_face)), k, float(coord_scale),
                            pixels.ctypes.data_as(C.POINTER(C.c_int32)))
    if st < 0 and st != _lib.RF_ERR_TRUNCATED:
        raise _lib.RFError(st, "rf_redact_host: bad spec or argument")
    return pixels[:k], st == _lib.RF_ERR_TRUNCATED


OVERLAY_LABEL_NONE, OVERLAY_LABEL_SCORE, OVERLAY_LABEL_ID = 0, 1, 2


def overlay_spec(thickness: int = 0, radius: int = 0, box=(0, 0, 0), point=(0, 0, 0), text=(0, 0, 0), colors_set: bool = False,
                 alpha: int = 0, label: int = 0, font_scale: int = 0, color_by_id: bool = False, max_regions: int = 0,
                 coast: int = 0) -> rf_overlay_spec:
    """rf_overlay_spec; 0 = the default (thickness 2, disc radius 2 -- negative = no landmarks, red boxes, green points, white digits,
    opaque, no label, font scale 2, max_detections regions, coast = the tracker's max_missed -- negative = no coasting tracks).  Colours
    are (B, G, R); colors_set makes all-zero colours mean black."""
    s = rf_overlay_spec()
    s.struct_size = C.sizeof(rf_overlay_spec)
    s.thickness, s.radius, s.label, s.font_scale, s.max_regions, s.coast = (int(thickness), int(radius), int(label), int(font_scale),
                                                                            int(max_regions), int(coast))
    if not 0 <= int(alpha) <= 255:
        raise ValueError("alpha must fit a byte (0 = opaque)")
    s.alpha, s.colors_set, s.color_by_id = int(alpha), int(bool(colors_set)), int(bool(color_by_id))
    for dst, src in ((s.box, box), (s.point, point), (s.text, text)):
        dst[0], dst[1], dst[2] = (int(v) for v in src)
    return s


def _as_overlay_spec(spec):
    if spec is None or isinstance(spec, rf_overlay_spec):
        return spec
    return overlay_spec(**spec)


def overlay_region(face, rows: int, cols: int, coord_scale: float = 1.0, track_id: int = 0, **spec):
    """rf_overlay_region (host only, no GPU): (valid, 24 int32: x0, y0, x1, y1, bounding rectangle bx0, by0, bx1, by1, digit count,
    digits (4 bits each), plate left, plate top, colour B | G << 8 | R << 16, disc mask, cx[5], cy[5]) of one face; keywords as
    overlay_spec()"""
    lib = _lib.load_library()
    f = rf_face.from_buffer_copy(_face_rows([face])[0].tobytes())
    out = (C.c_int32 * 24)()
    st = lib.rf_overlay_region(C.byref(overlay_spec(**spec)), C.byref(f), int(track_id), float(coord_scale), int(rows), int(cols), out)
    if st < 0:
        raise _lib.RFError(st, "rf_overlay_region: bad spec or argument")
    return bool(st), np.array(out, np.int32)


def _id_block(ids, n: int, cap: int):
    """per-image track ids as one (n, cap) int64 block, or None"""
    if ids is None:
        return None
    flat = np.zeros((max(n, 1), cap), np.int64)
    for i, v in enumerate(ids):
        v = np.asarray(v, np.int64).reshape(-1)
        flat[i, :min(len(v), cap)] = v[:cap]
    return flat


def overlay_host(img: np.ndarray, faces, coord_scale: float = 1.0, ids=None, **spec):
    """rf_overlay_host (host only, no GPU): draws boxes, landmark discs and labels into a uint8 H x W x 3 array (any row stride) in
    place at the given faces (ids: one track id per face, or None).  Returns (pixels per region, truncated); keywords as
    overlay_spec()."""
    lib = _lib.load_library()
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or (img.size and (img.strides[2] != 1 or img.strides[1] != 3)):
        raise ValueError("the frame must be uint8 H x W x 3 with dense pixels (CV_8UC3, BGR)")
    if not img.flags.writeable:
        raise ValueError("the frame is drawn into in place: it must be writeable")
    rows_f = _face_rows(faces)
    k = len(rows_f)
    pixels = np.zeros(max(k, 1), np.int32)
    flat = np.ascontiguousarray(rows_f) if k else np.zeros((1, 15), np.float32)
    idb = _id_block([ids], 1, max(k, 1)) if ids is not None else None
    st = lib.rf_overlay_host(C.byref(overlay_spec(**spec)), C.c_void_p(img.ctypes.data if img.size else None), img.shape[0], img.shape[1],
                             img.strides[0] if img.size else 0, flat.ctypes.data_as(C.POINTER(rf_face)),
                             idb.ctypes.data_as(C.POINTER(C.c_int64)) if idb is not None else None, k, float(coord_scale),
                             pixels.ctypes.data_as(C.POINTER(C.c_int32)))
    if st < 0 and st != _lib.RF_ERR_TRUNCATED:
        raise _lib.RFError(st, "rf_overlay_host: bad spec or argument")
    return pixels[:k], st == _lib.RF_ERR_TRUNCATED


class Tracker:
    """rf_tracker: per-stream track tables that live in device memory between calls (RetinaFace.tracker() creates one).  After every
    tracked call last_tags ((n, cap) TRACK_TAG_DTYPE), last_ended ((n, cap_ended) TRACK_DTYPE) and last_ended_counts hold the call's
    whole buffers and truncated says whether a table was full or an ended list was cut."""

    def __init__(self, det: "RetinaFace", n_streams: int, motion=None, follow=None, **spec):
        self._det, self._lib = det, det._lib
        self.motion_spec = None
        self.follow_spec = None
        self.spec = track_spec(**spec)
        self.max_tracks = self.spec.max_tracks or 64
        self.n_streams = int(n_streams)
        t = C.c_void_p()
        _lib.check(self._lib.rf_tracker_create(det._h, C.byref(self.spec), self.n_streams, C.byref(t)), det._h)
        self._t = t
        self.truncated = False
        self.last_tags = self.last_ended = self.last_ended_counts = None
        if motion is not None:
            try:
                self.enable_motion(**({} if motion is True else motion))
            except Exception:
                self.close()
                raise
        if follow is not None:
            try:
                self.enable_follow(**({} if follow is True else follow))
            except Exception:
                self.close()
                raise

    def close(self):
        if getattr(self, "_t", None) and getattr(self._det, "_h", None):
            self._lib.rf_tracker_destroy(self._t)
        self._t = None

    def _buffers(self, n, cap, cap_ended):
        cap_ended = self.max_tracks if cap_ended is None else int(cap_ended)
        self.last_tags = np.full((max(n, 1), max(cap, 1)), 0x55, np.uint8).repeat(24, 1).view(TRACK_TAG_DTYPE)
        self.last_ended = np.zeros((max(n, 1), max(cap_ended, 1)), TRACK_DTYPE)
        self.last_ended_counts = np.zeros(max(n, 1), np.int32)
        return (self._t, None, self.last_tags.ctypes.data_as(C.POINTER(rf_track_tag)), self.last_ended.ctypes.data_as(C.POINTER(rf_track)),
                cap_ended, self.last_ended_counts.ctypes.data_as(C.POINTER(C.c_int)))

    def _results(self, n, counts, cap):
        tags = [self.last_tags[i, :min(int(counts[i]), cap)].copy() for i in range(n)]
        ended = [self.last_ended[i, :min(int(self.last_ended_counts[i]), self.last_ended.shape[1])].copy() for i in range(n)]
        return tags, ended

    def update(self, streams: Sequence[int], faces, *, coord_scale: Optional[Sequence[float]] = None, quality=None,
               max_faces: Optional[int] = None, cap_per_image: Optional[int] = None, cap_ended: Optional[int] = None):
        """rf_track_update_device: frame steps over faces the caller supplies -- faces[i]: the faces of image i in score order (a
        (k, 15) array, rows or Detections), streams[i]: its stream or -1; quality[i]: None or its QUALITY_DTYPE records.  Returns
        (tags per image, ended tracks per image)."""
        n = len(streams)
        per = [_face_rows(f) for f in faces]
        mf = int(max_faces) if max_faces else self._det.max_detections
        cap = int(cap_per_image) if cap_per_image is not None else max([len(r) for r in per] + [1])
        flat = np.zeros((max(n, 1), cap, 15), np.float32)
        counts = (C.c_int * max(n, 1))()
        for i, r in enumerate(per):
            flat[i, :min(len(r), cap)] = r[:cap]
            counts[i] = len(r)
        q = None
        if quality is not None:
            q = np.zeros((max(n, 1), mf), QUALITY_DTYPE)
            for i, rec in enumerate(quality):
                if rec is not None and len(rec):
                    q[i, :min(len(rec), mf)] = np.asarray(rec, QUALITY_DTYPE)[:mf]
        cs = (C.c_float * max(n, 1))(*coord_scale) if coord_scale is not None else None
        t, _, tags, ended, ce, ec = self._buffers(n, cap, cap_ended)
        st = _lib.check(self._lib.rf_track_update_device(self._det._h, t, (C.c_int * max(n, 1))(*streams), n, flat.ctypes.data_as(C.POINTER(rf_face)),
                                                         cap, counts, cs, q.ctypes.data_as(C.POINTER(rf_face_quality)) if q is not None else None,
                                                         mf, tags, ended, ce, ec), self._det._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        return self._results(n, counts, cap)

    # ------------------------------------------------------------------ motion-predicted tracks
    def enable_motion(self, **spec):
        """rf_tracker_enable_motion: every tracked call then matches and coasts at the predicted boxes; keywords as motion_spec()"""
        sp = motion_spec(**spec)
        _lib.check(self._lib.rf_tracker_enable_motion(self._t, C.byref(sp)), self._det._h)
        self.motion_spec = sp
        return self

    def read_motion(self, stream: int) -> np.ndarray:
        """rf_tracker_read_motion: the (max_tracks,) MOTION_DTYPE records of a stream"""
        rec = np.zeros(self.max_tracks, MOTION_DTYPE)
        _lib.check(self._lib.rf_tracker_read_motion(self._t, int(stream), rec.ctypes.data_as(C.POINTER(rf_track_motion)), self.max_tracks),
                   self._det._h)
        return rec

    # ------------------------------------------------------------------ followed tracks
    def enable_follow(self, **spec):
        """rf_tracker_enable_follow: give the tracker templates; keywords as follow_spec().  From then on only the follow calls take it."""
        sp = follow_spec(**spec)
        _lib.check(self._lib.rf_tracker_enable_follow(self._t, C.byref(sp)), self._det._h)
        self.follow_spec = sp
        return self

    def read_follow(self, stream: int):
        """rf_tracker_read_follow: (records (max_tracks,) FOLLOW_DTYPE, templates (max_tracks, 32, 32) u8) of a stream"""
        rec = np.zeros(self.max_tracks, FOLLOW_DTYPE)
        tpl = np.zeros((self.max_tracks, FOLLOW_G, FOLLOW_G), np.uint8)
        _lib.check(self._lib.rf_tracker_read_follow(self._t, int(stream), rec.ctypes.data_as(C.POINTER(rf_track_follow)), tpl.ctypes.data,
                                                    self.max_tracks), self._det._h)
        return rec, tpl

    def update_follow(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], streams: Sequence[int], faces, *,
                      steps: Optional[Sequence[int]] = None, coord_scale: Optional[Sequence[float]] = None, quality=None,
                      cap_per_image: Optional[int] = None, cap_ended: Optional[int] = None):
        """rf_track_follow_update_device: a key step -- update() against frames resident in device memory + the keep rule.  Returns
        (tags per image, ended tracks per image)."""
        n = len(streams)
        per = [_face_rows(f) for f in faces]
        mf = self._det.max_detections
        cap = int(cap_per_image) if cap_per_image is not None else max([len(r) for r in per] + [1])
        flat = np.zeros((max(n, 1), cap, 15), np.float32)
        counts = (C.c_int * max(n, 1))()
        for i, r in enumerate(per):
            flat[i, :min(len(r), cap)] = r[:cap]
            counts[i] = len(r)
        q = None
        if quality is not None:
            q = np.zeros((max(n, 1), mf), QUALITY_DTYPE)
            for i, rec in enumerate(quality):
                if rec is not None and len(rec):
                    q[i, :min(len(rec), mf)] = np.asarray(rec, QUALITY_DTYPE)[:mf]
        cs = (C.c_float * max(n, 1))(*coord_scale) if coord_scale is not None else None
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        t, _, tags, ended, ce, ec = self._buffers(n, cap, cap_ended)
        st = _lib.check(self._lib.rf_track_follow_update_device(self._det._h, t, p, r, c, s, n, (C.c_int * max(n, 1))(*streams),
                                                                flat.ctypes.data_as(C.POINTER(rf_face)), cap, counts, cs,
                                                                q.ctypes.data_as(C.POINTER(rf_face_quality)) if q is not None else None, tags, ended,
                                                                ce, ec), self._det._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        self.last_counts = [0 if not ptrs[i] or rows[i] <= 0 or cols[i] <= 0 else int(counts[i]) for i in range(n)]
        return self._results(n, self.last_counts, cap)

    def _follow_call(self, fn, ptrs, rows, cols, streams, steps, cap_per_image, cap_ended):
        n = len(streams)
        cap = self.max_tracks if cap_per_image is None else int(cap_per_image)
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        self.last_out = np.zeros((max(n, 1), max(cap, 1), 15), np.float32)
        counts = (C.c_int * max(n, 1))()
        t, _, tags, ended, ce, ec = self._buffers(n, cap, cap_ended)
        st = _lib.check(fn(self._det._h, t, p, r, c, s, n, (C.c_int * max(n, 1))(*streams), self.last_out.ctypes.data_as(C.POINTER(rf_face)), cap,
                           counts, tags, ended, ce, ec), self._det._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        self.last_counts = [int(counts[i]) for i in range(n)]
        faces = [self.last_out[i, :min(self.last_counts[i], cap)].copy() for i in range(n)]
        return (faces,) + self._results(n, self.last_counts, cap)

    def follow_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], streams: Sequence[int], *,
                      steps: Optional[Sequence[int]] = None, cap_per_image: Optional[int] = None, cap_ended: Optional[int] = None):
        """rf_track_follow_device: a follow step over frames resident in device memory -- no forward pass.  Returns (followed faces
        per image ((k, 15) float32, slot-ascending), their tags, ended tracks per image); last_counts holds the true numbers."""
        return self._follow_call(self._lib.rf_track_follow_device, ptrs, rows, cols, streams, steps, cap_per_image, cap_ended)

    def follow(self, imgs: Sequence[np.ndarray], streams: Sequence[int], *, cap_per_image: Optional[int] = None,
               cap_ended: Optional[int] = None):
        """rf_track_follow_batch: follow_device() over host frames ((rows, cols, 3) u8 views; None or empty = no pixels)"""
        views = [_frame_view(im) for im in imgs]
        return self._follow_call(self._lib.rf_track_follow_batch, [v[0] for v in views], [v[1] for v in views], [v[2] for v in views], streams,
                                 [v[3] for v in views], cap_per_image, cap_ended)

    def follow_last_launch_ms(self) -> float:
        """rf_follow_last_launch_ms: HIP-event time of the search and step launches of the most recent follow_device()"""
        ms = C.c_float()
        _lib.check(self._lib.rf_follow_last_launch_ms(self._det._h, C.byref(ms)), self._det._h)
        return float(ms.value)

    # ------------------------------------------------------------------ best-shot gallery
    def enable_shots(self, **spec):
        """rf_tracker_enable_shots: give the tracker a gallery; keywords as face_batch_spec().  From then on only the shot calls take it."""
        sp = face_batch_spec(**spec)
        _lib.check(self._lib.rf_tracker_enable_shots(self._t, C.byref(sp)), self._det._h)
        self.shot_spec = sp
        self.shot_dtype = np.dtype(_FACE_FORMATS[spec.get("dtype", "f16")][1])
        self.bytes_per_face = 3 * (sp.crop_size or 112) ** 2 * self.shot_dtype.itemsize
        self.shot_max_faces = sp.max_faces or self._det.max_detections
        self.last_shots = self.last_shot_info = None
        return self

    def _shot_buffers(self, n, cap_ended, host=True):
        cap_ended = self.max_tracks if cap_ended is None else int(cap_ended)
        self.last_shots = np.full((max(n, 1), max(cap_ended, 1), self.bytes_per_face), 0xA5, np.uint8) if host else None
        self.last_shot_info = np.full((max(n, 1), max(cap_ended, 1)), 0xA5, np.uint8).repeat(64, 1).view(SHOT_DTYPE)
        return (self.last_shots.ctypes.data if host else None), self.last_shot_info.ctypes.data_as(C.POINTER(rf_shot))

    def _shot_results(self, n):
        ce = self.last_ended.shape[1]
        k = [min(int(self.last_ended_counts[i]), ce) for i in range(n)]
        shots = [self.last_shots[i, :k[i]].copy() for i in range(n)] if self.last_shots is not None else None
        return shots, [self.last_shot_info[i, :k[i]].copy() for i in range(n)]

    def read_shots(self, stream: int):
        """rf_tracker_read_shots: (entries (max_tracks, bytes_per_face) u8, records (max_tracks,) SHOT_DTYPE) of a stream"""
        ent = np.zeros((self.max_tracks, self.bytes_per_face), np.uint8)
        rec = np.zeros(self.max_tracks, SHOT_DTYPE)
        _lib.check(self._lib.rf_tracker_read_shots(self._t, int(stream), ent.ctypes.data, rec.ctypes.data_as(C.POINTER(rf_shot)), self.max_tracks),
                   self._det._h)
        return ent, rec

    def flush_shots(self, stream: int):
        """rf_tracker_flush_shots: (ended tracks, their shots (k, bytes_per_face) u8, their records), slot-ascending"""
        ended = np.zeros(self.max_tracks, TRACK_DTYPE)
        ent = np.zeros((self.max_tracks, self.bytes_per_face), np.uint8)
        rec = np.zeros(self.max_tracks, SHOT_DTYPE)
        k = _lib.check(self._lib.rf_tracker_flush_shots(self._t, int(stream), ended.ctypes.data_as(C.POINTER(rf_track)), self.max_tracks, None, None,
                                                        ent.ctypes.data, rec.ctypes.data_as(C.POINTER(rf_shot))), self._det._h)
        return ended[:k], ent[:k], rec[:k]

    def update_shots(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], streams: Sequence[int], faces, *,
                     steps: Optional[Sequence[int]] = None, coord_scale: Optional[Sequence[float]] = None, quality=None,
                     cap_per_image: Optional[int] = None, cap_ended: Optional[int] = None, d_shots: int = 0, host_shots: bool = True):
        """rf_track_shots_device: update() against frames resident in device memory + the gallery rules.  Returns (tags per image,
        ended tracks per image, shots per image (None without host_shots), shot records per image)."""
        n = len(streams)
        per = [_face_rows(f) for f in faces]
        mf = self.shot_max_faces
        cap = int(cap_per_image) if cap_per_image is not None else max([len(r) for r in per] + [1])
        flat = np.zeros((max(n, 1), cap, 15), np.float32)
        counts = (C.c_int * max(n, 1))()
        for i, r in enumerate(per):
            flat[i, :min(len(r), cap)] = r[:cap]
            counts[i] = len(r)
        q = None
        if quality is not None:
            q = np.zeros((max(n, 1), mf), QUALITY_DTYPE)
            for i, rec in enumerate(quality):
                if rec is not None and len(rec):
                    q[i, :min(len(rec), mf)] = np.asarray(rec, QUALITY_DTYPE)[:mf]
        cs = (C.c_float * max(n, 1))(*coord_scale) if coord_scale is not None else None
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        t, _, tags, ended, ce, ec = self._buffers(n, cap, cap_ended)
        shots, info = self._shot_buffers(n, cap_ended, host_shots)
        st = _lib.check(self._lib.rf_track_shots_device(self._det._h, t, p, r, c, s, n, (C.c_int * max(n, 1))(*streams),
                                                        flat.ctypes.data_as(C.POINTER(rf_face)), cap, counts, cs,
                                                        q.ctypes.data_as(C.POINTER(rf_face_quality)) if q is not None else None, tags, ended, ce,
                                                        ec, d_shots or None, shots, info), self._det._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        self.last_counts = [0 if not ptrs[i] else int(counts[i]) for i in range(n)]
        return self._results(n, self.last_counts, cap) + self._shot_results(n)

    def shot_last_launch_ms(self) -> float:
        """rf_shot_last_launch_ms: HIP-event time of the two shot launches of the most recent update_shots()"""
        ms = C.c_float()
        _lib.check(self._lib.rf_shot_last_launch_ms(self._det._h, C.byref(ms)), self._det._h)
        return float(ms.value)

    def detect_redacted_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], streams: Sequence[int],
                               threshold: float = 0.5, steps: Optional[Sequence[int]] = None, cap_ended: Optional[int] = None, spec=None):
        """rf_detect_track_redact_batch_device: RetinaFace.detect_tracked_device + redaction in place, the coasting tracks of each
        stream included (each stream at most once per call).  Returns (detections, tags, ended); last_pixels / last_region_counts
        hold the redaction's results."""
        det = self._det
        n = len(ptrs)
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        sp = _as_redact_spec(spec)
        mr = det._redact_regions(sp)
        self.last_pixels = np.zeros((max(n, 1), mr), np.int32)
        self.last_region_counts = np.zeros(max(n, 1), np.int32)
        cap = det.max_detections
        out = (rf_face * max(n * cap, 1))()
        counts = (C.c_int * max(n, 1))()
        t, _, tags, ended, ce, ec = self._buffers(n, cap, cap_ended)
        st = _lib.check(self._lib.rf_detect_track_redact_batch_device(
            det._h, p, r, c, s, n, float(threshold), out, cap, counts, t, (C.c_int * max(n, 1))(*streams), tags, ended, ce, ec,
            C.byref(sp) if sp is not None else None, self.last_pixels.ctypes.data_as(C.POINTER(C.c_int32)),
            self.last_region_counts.ctypes.data_as(C.POINTER(C.c_int))), det._h)
        det.truncated = self.truncated = st == _lib.RF_ERR_TRUNCATED
        det.last_out = _faces_to_array(out, max(n * cap, 1)).reshape(max(n, 1), cap, 15)
        det.last_counts = [int(counts[i]) for i in range(n)]
        return (det._collect(out, counts, n, cap),) + self._results(n, counts, cap)

    def detect_tracked_overlay(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], streams: Sequence[int],
                               threshold: float = 0.5, steps: Optional[Sequence[int]] = None, cap_ended: Optional[int] = None, spec=None):
        """rf_detect_track_overlay_batch_device: RetinaFace.detect_tracked_device + boxes, landmarks and labels drawn in place, ids
        from the tags of this frame's step, the coasting tracks of each stream dashed (each stream at most once per call).  Returns
        (detections, tags, ended); last_pixels / last_region_counts hold the overlay's results."""
        det = self._det
        n = len(ptrs)
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        sp = _as_overlay_spec(spec)
        mr = det._redact_regions(sp)
        self.last_pixels = np.zeros((max(n, 1), mr), np.int32)
        self.last_region_counts = np.zeros(max(n, 1), np.int32)
        cap = det.max_detections
        out = (rf_face * max(n * cap, 1))()
        counts = (C.c_int * max(n, 1))()
        t, _, tags, ended, ce, ec = self._buffers(n, cap, cap_ended)
        st = _lib.check(self._lib.rf_detect_track_overlay_batch_device(
            det._h, p, r, c, s, n, float(threshold), out, cap, counts, t, (C.c_int * max(n, 1))(*streams), tags, ended, ce, ec,
            C.byref(sp) if sp is not None else None, self.last_pixels.ctypes.data_as(C.POINTER(C.c_int32)),
            self.last_region_counts.ctypes.data_as(C.POINTER(C.c_int))), det._h)
        det.truncated = self.truncated = st == _lib.RF_ERR_TRUNCATED
        det.last_out = _faces_to_array(out, max(n * cap, 1)).reshape(max(n, 1), cap, 15)
        det.last_counts = [int(counts[i]) for i in range(n)]
        return (det._collect(out, counts, n, cap),) + self._results(n, counts, cap)

    # ------------------------------------------------------------------ tracked region detection
    def roi_cells(self, streams: Sequence[int], margin: Optional[float] = None, grid: int = 0, max_zoom: int = 0) -> np.ndarray:
        """rf_roi_track_cells_device: the plan kernel alone -- the (n, max_tracks, 8) int32 cell records (roi_plan()'s columns) the
        device plans from the tables of streams[i] (-1: void records).  Changes nothing."""
        n = len(streams)
        cells = (rf_roi_cell * max(n * self.max_tracks, 1))()
        _lib.check(self._lib.rf_roi_track_cells_device(self._det._h, self._t, (C.c_int * max(n, 1))(*streams), n, _margin_q8(margin),
                                                       C.byref(roi_spec(grid, max_zoom)), cells), self._det._h)
        return _cell_rows(cells, n * self.max_tracks).reshape(n, self.max_tracks, 8)

    def _tracked_rois(self, fn, frames, streams, threshold, margin, grid, max_zoom, vote, max_faces, views_ptr, cap_ended, return_src_roi):
        det = self._det
        n = frames[4]
        sp = roi_spec(grid, max_zoom, vote, max_faces)
        cap = sp.max_faces or det.max_detections
        cells = (rf_roi_cell * max(n * self.max_tracks, 1))()
        t, _, tags, ended, ce, ec = self._buffers(n, cap, cap_ended)
        head = (det._h,) + tuple(frames) + (float(threshold), C.byref(sp), _margin_q8(margin))
        tail = (cells, views_ptr, t, (C.c_int * max(n, 1))(*streams), tags, ended, ce, ec)
        dets, src, votes = det._merged_call(fn, head, n, cap, "roi_counts", True, tail=tail)      # the C call takes src_roi, then votes
        self.truncated = det.truncated
        self.last_cells = _cell_rows(cells, n * self.max_tracks).reshape(n, self.max_tracks, 8)
        res = (dets,) + self._results(n, det.roi_counts, cap)
        return res + (votes, src) if return_src_roi else res

    def detect_tracked_rois(self, imgs: Sequence[np.ndarray], streams: Sequence[int], threshold: float = 0.5, margin: Optional[float] = None,
                            grid: int = 0, max_zoom: int = 0, vote: bool = False, max_faces: int = 0, cap_ended: Optional[int] = None,
                            return_src_roi: bool = False):
        """rf_detect_track_roi_batch: every frame (None: an empty frame, whose stream ages) is detected only in the regions the device
        plans from the table of its stream (streams[i]; -1: no regions, no faces, no step) -- slot r is region r, a free slot a void
        cell; a live slot's region is its last (with motion: its predicted) box grown by `margin` of its longer side (None: a quarter)
        -- and the merged faces go straight into the frame step.  Returns (detections in SOURCE-FRAME pixels, tags per image, ended
        tracks per image); with return_src_roi also, per frame, how many candidates each face merged and the slot whose region found
        it.  self.last_cells holds the (n, max_tracks, 8) cell records the device planned; the detector's roi_counts the true counts."""
        f = _host_frames(imgs)
        return self._tracked_rois(self._lib.rf_detect_track_roi_batch, f.args, streams, threshold, margin, grid, max_zoom, vote, max_faces, None,
                                  cap_ended, return_src_roi)

    def detect_tracked_rois_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], streams: Sequence[int],
                                   threshold: float = 0.5, steps: Optional[Sequence[int]] = None, margin: Optional[float] = None, grid: int = 0,
                                   max_zoom: int = 0, vote: bool = False, max_faces: int = 0, views_ptr: Optional[int] = None,
                                   cap_ended: Optional[int] = None, return_src_roi: bool = False):
        """rf_detect_track_roi_batch_device: detect_tracked_rois for frames resident in device memory (0 / None: an empty frame).
        views_ptr: device memory of passes * net_h * net_w * 3 bytes that receives the views as dense frames."""
        frames = _device_frames(ptrs, rows, cols, steps) + (len(ptrs),)
        return self._tracked_rois(self._lib.rf_detect_track_roi_batch_device, frames, streams, threshold, margin, grid, max_zoom, vote, max_faces,
                                  views_ptr, cap_ended, return_src_roi)

    def read(self, stream: int):
        """rf_tracker_read: (table, frames, next_id) of a stream"""
        table = np.zeros(self.max_tracks, TRACK_DTYPE)
        f, nid = C.c_int64(), C.c_int64()
        _lib.check(self._lib.rf_tracker_read(self._t, int(stream), table.ctypes.data_as(C.POINTER(rf_track)), len(table), C.byref(f), C.byref(nid)),
                   self._det._h)
        return table, f.value, nid.value

    def flush(self, stream: int) -> np.ndarray:
        """rf_tracker_flush: ends every live track of the stream and returns them slot-ascending"""
        ended = np.zeros(self.max_tracks, TRACK_DTYPE)
        k = _lib.check(self._lib.rf_tracker_flush(self._t, int(stream), ended.ctypes.data_as(C.POINTER(rf_track)), len(ended), None, None), self._det._h)
        return ended[:k]

    def reset(self, stream: int = -1) -> None:
        _lib.check(self._lib.rf_tracker_reset(self._t, int(stream)), self._det._h)


def tta_spec(flip: bool = True, vote: bool = True, max_faces: int = 0) -> rf_tta_spec:
    """An rf_tta_spec: flip (also detect every frame mirrored left-right), vote (a kept box becomes the score-weighted mean of the
    candidates it suppressed; off: the plain greedy NMS), max_faces (merged faces kept per frame; 0 = the engine's max_detections)."""
    sp = rf_tta_spec()
    sp.struct_size = C.sizeof(rf_tta_spec)
    sp.flip, sp.vote, sp.max_faces = 1 if flip else 2, 1 if vote else 2, int(max_faces)
    return sp


def tta_map_face(face, pass_index: int, rows: int, cols: int, net_h: int, net_w: int) -> np.ndarray:
    """rf_tta_map_face (host only, no GPU): the face (a Detection or 15 floats) of pass 0 (the frame) or 1 (the frame mirrored) in
    source-frame pixels, as 15 float32."""
    lib = _lib.load_library()
    f = rf_face.from_buffer_copy(_face_rows([face])[0].tobytes())
    g = rf_face()
    st = lib.rf_tta_map_face(int(rows), int(cols), int(net_h), int(net_w), int(pass_index), C.byref(f), C.byref(g))
    if st < 0:
        raise _lib.RFError(st, "rf_tta_map_face: bad frame, net size or pass index")
    return _faces_to_array(C.pointer(g), 1)[0]


def tta_merge_host(passes, rows: int, cols: int, net_h: int, net_w: int, nms_threshold: float, max_detections: int, flip: bool = True,
                   vote: bool = True, max_faces: int = 0, cap: Optional[int] = None, spec=None):
    """rf_tta_merge_host (host only, no GPU): mapping and merge of ONE frame -- passes[p]: the faces of pass p (a (k, 15) array, rows of
    15 floats or Detections), two passes, one with flip off.  Returns (faces (k, 15) float32 in merge order, count: the true number of
    heads, votes (k,) int32, src_pass (k,) int32, truncated)."""
    lib = _lib.load_library()
    sp = spec if spec is not None else tta_spec(flip, vote, max_faces)
    md = int(max_detections)
    if md < 1:
        raise _lib.RFError(_lib.RF_ERR_INVALID_ARG, "rf_tta_merge_host: max_detections must be positive")
    passes = list(passes)
    flat, pc = _pack_passes(passes, md)
    cap = int(cap) if cap is not None else (sp.max_faces or md)
    out = (rf_face * max(cap, 1))()
    votes, src = (C.c_int * max(cap, 1))(), (C.c_int * max(cap, 1))()
    count = C.c_int(0)
    if len(passes) != (1 if sp.flip == 2 else 2):
        raise _lib.RFError(_lib.RF_ERR_INVALID_ARG, "rf_tta_merge_host: one pass per frame with flip off, two otherwise")
    st = lib.rf_tta_merge_host(C.byref(sp), int(rows), int(cols), int(net_h), int(net_w), float(nms_threshold), md,
                               flat.ctypes.data_as(C.POINTER(rf_face)), pc, out, cap, C.byref(count), votes, src)
    if st < 0 and st != _lib.RF_ERR_TRUNCATED:
        raise _lib.RFError(st, "rf_tta_merge_host: bad spec, frame, net size or counts")
    k = max(0, min(count.value, cap, sp.max_faces or md))
    return (_faces_to_array(out, max(cap, 1))[:k], int(count.value), np.array(votes[:k], np.int32), np.array(src[:k], np.int32),
            st == _lib.RF_ERR_TRUNCATED)


def rot_spec(rots: int = 0, vote: bool = False, max_faces: int = 0) -> rf_rot_spec:
    """An rf_rot_spec: rots (bit k: also detect every frame turned by k quarter turns counter-clockwise; 0 = all four), vote (a kept
    box becomes the score-weighted mean of the candidates it suppressed; off, the default: the plain greedy NMS over all passes),
    max_faces (merged faces kept per frame; 0 = the engine's max_detections)."""
    sp = rf_rot_spec()
    sp.struct_size = C.sizeof(rf_rot_spec)
    sp.rots, sp.vote, sp.max_faces = int(rots), 1 if vote else 2, int(max_faces)
    return sp


def _rot_list(rots: int):
    return [k for k in range(4) if (int(rots) or 15) >> k & 1]


def rot_map_face(face, k: int, rows: int, cols: int, net_h: int, net_w: int) -> np.ndarray:
    """rf_rot_map_face (host only, no GPU): the face (a Detection or 15 floats) of pass k (the rows x cols frame turned by k quarter
    turns counter-clockwise) in source-frame pixels, as 15 float32."""
    lib = _lib.load_library()
    f = rf_face.from_buffer_copy(_face_rows([face])[0].tobytes())
    g = rf_face()
    st = lib.rf_rot_map_face(int(rows), int(cols), int(net_h), int(net_w), int(k), C.byref(f), C.byref(g))
    if st < 0:
        raise _lib.RFError(st, "rf_rot_map_face: bad frame, net size or rotation")
    return _faces_to_array(C.pointer(g), 1)[0]


def rot_merge_host(passes, rows: int, cols: int, net_h: int, net_w: int, nms_threshold: float, max_detections: int, rots: int = 0,
                   vote: bool = False, max_faces: int = 0, cap: Optional[int] = None, spec=None):
    """rf_rot_merge_host (host only, no GPU): mapping and merge of ONE frame -- passes[p]: the faces of the p-th rotation of `rots` in
    ascending k (a (j, 15) array, rows of 15 floats or Detections).  Returns (faces (j, 15) float32 in merge order, count: the true
    number of heads, votes (j,) int32, src_rot (j,) int32, truncated, frame_rot, rot_score (4,) float32)."""
    lib = _lib.load_library()
    sp = spec if spec is not None else rot_spec(rots, vote, max_faces)
    md = int(max_detections)
    if md < 1:
        raise _lib.RFError(_lib.RF_ERR_INVALID_ARG, "rf_rot_merge_host: max_detections must be positive")
    passes = list(passes)
    flat, pc = _pack_passes(passes, md)
    cap = int(cap) if cap is not None else (sp.max_faces or md)
    out = (rf_face * max(cap, 1))()
    votes, src = (C.c_int * max(cap, 1))(), (C.c_int * max(cap, 1))()
    count, frame_rot = C.c_int(0), C.c_int(-1)
    score = (C.c_float * 4)()
    if 0 <= sp.rots <= 15 and len(passes) != len(_rot_list(sp.rots)):
        raise _lib.RFError(_lib.RF_ERR_INVALID_ARG, "rf_rot_merge_host: one pass per rotation of rots")
    st = lib.rf_rot_merge_host(C.byref(sp), int(rows), int(cols), int(net_h), int(net_w), float(nms_threshold), md,
                               flat.ctypes.data_as(C.POINTER(rf_face)), pc, out, cap, C.byref(count), votes, src, C.byref(frame_rot), score)
    if st < 0 and st != _lib.RF_ERR_TRUNCATED:
        raise _lib.RFError(st, "rf_rot_merge_host: bad spec, frame, net size or counts")
    k = max(0, min(count.value, cap, sp.max_faces or md))
    return (_faces_to_array(out, max(cap, 1))[:k], int(count.value), np.array(votes[:k], np.int32), np.array(src[:k], np.int32),
            st == _lib.RF_ERR_TRUNCATED, int(frame_rot.value), np.array(score[:], np.float32))


def rotate_host(frame: np.ndarray, k: int, out: Optional[np.ndarray] = None) -> np.ndarray:
    """rf_rotate_host (host only, no GPU): the BGR frame turned by k (0..3) quarter turns counter-clockwise, np.rot90(frame, k).
    `out`: a uint8 (rows_k, >= cols_k, 3) view to write into (its row pitch is kept); returned either way."""
    lib = _lib.load_library()
    frame = _dense_frame(frame)
    rows, cols = frame.shape[:2]
    dr, dc = (cols, rows) if int(k) & 1 else (rows, cols)
    if out is None:
        out = np.zeros((dr, dc, 3), np.uint8)
    if out.dtype != np.uint8 or out.ndim != 3 or out.shape[2] != 3 or out.strides[2] != 1 or out.strides[1] != 3 or out.shape[0] < dr:
        raise ValueError("out must be a uint8 (rows_k, cols_k, 3) array or row-pitched view")
    st = lib.rf_rotate_host(frame.ctypes.data, rows, cols, frame.strides[0] if rows else 3 * cols, int(k), out.ctypes.data,
                            out.strides[0] if out.shape[0] else 3 * dc)
    if st < 0:
        raise _lib.RFError(st, "rf_rotate_host: k must be in 0..3 and the destination pitch at least cols_k * 3")
    return out


LENS_EQUIDISTANT, LENS_EQUISOLID, LENS_STEREOGRAPHIC, LENS_ORTHOGRAPHIC = 0, 1, 2, 3


def dewarp_spec(model: int = LENS_EQUIDISTANT, f: float = 0.0, cx: float = 0.0, cy: float = 0.0, views=None, ring: int = 0,
                pitch: float = 0.0, hfov: float = 0.0, vote: bool = False, max_faces: int = 0, edge: int = 0) -> rf_dewarp_spec:
    """An rf_dewarp_spec: the lens (model, f in pixels, the centre cx, cy), the views -- `views`: up to 16 (yaw, pitch, roll, hfov)
    tuples in degrees, or `ring` = N views at equal yaw steps with one pitch and hfov -- and the call-level fields vote (a kept box
    becomes the score-weighted mean of its cluster; off by default), max_faces (0 = the engine's max_detections) and edge (a face
    within this many view pixels of its view's border is dropped; 0 = off)."""
    sp = rf_dewarp_spec()
    sp.struct_size = C.sizeof(rf_dewarp_spec)
    sp.model, sp.f, sp.cx, sp.cy = int(model), float(f), float(cx), float(cy)
    views = list(views or [])
    if len(views) > 16:
        raise _lib.RFError(_lib.RF_ERR_INVALID_ARG, "rf_dewarp_spec: at most 16 views")
    sp.views, sp.ring, sp.ring_pitch, sp.ring_hfov = len(views), int(ring), float(pitch), float(hfov)
    for j, v in enumerate(views):
        sp.view[j].yaw, sp.view[j].pitch, sp.view[j].roll, sp.view[j].hfov = (float(x) for x in v)
    sp.vote, sp.max_faces, sp.edge = 1 if vote else 2, int(max_faces), int(edge)
    return sp


def _mesh_array(mesh, view_w: int, view_h: int, views: Optional[int] = None) -> np.ndarray:
    m = np.ascontiguousarray(mesh, dtype=np.int32)
    per = (view_h // 16 + 1) * (view_w // 16 + 1) * 2
    if view_w < 16 or view_h < 16 or view_w % 16 or view_h % 16 or m.size % per or (views is not None and m.size != per * views):
        raise _lib.RFError(_lib.RF_ERR_INVALID_ARG, "a mesh holds (view_h / 16 + 1) x (view_w / 16 + 1) x 2 int32 per view")
    return m


def dewarp_plan(spec: rf_dewarp_spec, view_w: int, view_h: int) -> np.ndarray:
    """rf_dewarp_plan (host only, no GPU): the meshes of the spec's views, (V, view_h / 16 + 1, view_w / 16 + 1, 2) int32 -- per node
    the source x and y of view pixel (16 i, 16 j) in 1/256 px.  Raises for a spec the plan refuses."""
    lib = _lib.load_library()
    if view_w < 16 or view_h < 16 or view_w % 16 or view_h % 16:
        raise _lib.RFError(_lib.RF_ERR_INVALID_ARG, "rf_dewarp_plan: view_w / view_h must be multiples of 16")
    ny, nx = view_h // 16 + 1, view_w // 16 + 1
    mesh = np.zeros((16, ny, nx, 2), np.int32)
    views = C.c_int(0)
    st = lib.rf_dewarp_plan(C.byref(spec), int(view_w), int(view_h), mesh.ctypes.data_as(C.POINTER(C.c_int32)), mesh.size, C.byref(views))
    if st < 0:
        raise _lib.RFError(st, "rf_dewarp_plan: a bad spec, a view beyond what the lens images, or a node beyond +-2^22")
    return np.ascontiguousarray(mesh[:views.value])


def dewarp_host(frame: np.ndarray, view_mesh, view_w: int, view_h: int, out: Optional[np.ndarray] = None) -> np.ndarray:
    """rf_dewarp_host (host only, no GPU): one view (its nodes: view_mesh) of the BGR frame.  `out`: a (view_h, view_w, 3) uint8
    array or view whose pixels are contiguous (any row pitch)."""
    lib = _lib.load_library()
    m = _mesh_array(view_mesh, view_w, view_h, 1)
    frame = _dense_frame(frame)
    if out is None:
        out = np.empty((view_h, view_w, 3), np.uint8)
    if out.dtype != np.uint8 or out.shape != (view_h, view_w, 3) or out.strides[2] != 1 or out.strides[1] != 3:
        raise ValueError("out must be a (view_h, view_w, 3) uint8 array with contiguous pixels")
    st = lib.rf_dewarp_host(m.ctypes.data, int(view_w), int(view_h), frame.ctypes.data, frame.shape[0], frame.shape[1], frame.strides[0],
                            out.ctypes.data, out.strides[0])
    if st < 0:
        raise _lib.RFError(st, "rf_dewarp_host: bad mesh, frame or destination pitch")
    return out


def dewarp_map_face(face, view_mesh, view_w: int, view_h: int, net_h: int, net_w: int, edge: int = 0):
    """rf_dewarp_map_face (host only, no GPU): the face (a Detection or 15 floats) of the view whose nodes are view_mesh moved into the
    frame, 15 float32 -- or None when the edge rule drops it."""
    lib = _lib.load_library()
    m = _mesh_array(view_mesh, view_w, view_h, 1)
    f, g = rf_face(), rf_face()
    C.memmove(C.byref(f), _face_rows([face]).ctypes.data, 60)
    st = lib.rf_dewarp_map_face(m.ctypes.data, int(view_w), int(view_h), int(net_h), int(net_w), int(edge), C.byref(f), C.byref(g))
    if st < 0:
        raise _lib.RFError(st, "rf_dewarp_map_face: bad mesh, net size or edge")
    return np.frombuffer(bytes(g)[:60], np.float32).copy() if st else None


def dewarp_merge_host(passes, mesh, view_w: int, view_h: int, net_h: int, net_w: int, nms_threshold: float, max_detections: int,
                      vote: bool = False, max_faces: int = 0, edge: int = 0, cap: Optional[int] = None, spec=None):
    """rf_dewarp_merge_host (host only, no GPU): mapping and merge of ONE frame -- passes[v]: the faces of view v in score order.
    Returns (faces (j, 15) float32, the true number of heads, votes (j,) int32, src_view (j,) int32, truncated)."""
    lib = _lib.load_library()
    sp = spec if spec is not None else dewarp_spec(vote=vote, max_faces=max_faces, edge=edge)
    md = int(max_detections)
    if md < 1:
        raise _lib.RFError(_lib.RF_ERR_INVALID_ARG, "rf_dewarp_merge_host: max_detections must be positive")
    passes = list(passes)
    flat, pc = _pack_passes(passes, md)
    m = _mesh_array(mesh, view_w, view_h, len(passes))
    cap = int(cap) if cap is not None else (sp.max_faces or md)
    out = (rf_face * max(cap, 1))()
    votes, src = (C.c_int * max(cap, 1))(), (C.c_int * max(cap, 1))()
    count = C.c_int(0)
    st = lib.rf_dewarp_merge_host(C.byref(sp), m.ctypes.data, int(view_w), int(view_h), len(passes), int(net_h), int(net_w),
                                  float(nms_threshold), md, flat.ctypes.data_as(C.POINTER(rf_face)), pc, out, cap, C.byref(count), votes, src)
    if st < 0 and st != _lib.RF_ERR_TRUNCATED:
        raise _lib.RFError(st, "rf_dewarp_merge_host: bad spec, mesh, net size or counts")
    k = min(count.value, cap, sp.max_faces or md)
    return (_faces_to_array(out, max(cap, 1))[:k].copy(), int(count.value), np.array(votes[:k], np.int32), np.array(src[:k], np.int32),
            st == _lib.RF_ERR_TRUNCATED)


class Dewarper:
    """One camera's dewarped views on a detector (rf_dewarper_create): the shape of its frames, view_w x view_h (0 = the net size) and the
    meshes of its views -- an rf_dewarp_spec to plan them from, or a ready (V, ny, nx, 2) int32 mesh -- uploaded once."""

    def __init__(self, det: "RetinaFace", rows: int, cols: int, spec=None, mesh=None, view_w: int = 0, view_h: int = 0):
        self._det, self._d = det, None
        self.rows, self.cols = int(rows), int(cols)
        self.view_w, self.view_h = int(view_w) or det.net_w, int(view_h) or det.net_h
        self.spec = spec
        if mesh is None:
            if spec is None:
                raise ValueError("a dewarper needs a spec or a mesh")
            mesh = dewarp_plan(spec, self.view_w, self.view_h)
        self.mesh = _mesh_array(mesh, self.view_w, self.view_h).reshape(-1, self.view_h // 16 + 1, self.view_w // 16 + 1, 2)
        self.views = len(self.mesh)
        d = C.c_void_p()
        _lib.check(det._lib.rf_dewarper_create(det._h, self.rows, self.cols, int(view_w), int(view_h), self.views, self.mesh.ctypes.data,
                                               C.byref(d)), det._h)
        self._d = d

    def close(self):
        if self._d is not None and self._det._h:
            self._det._lib.rf_dewarper_destroy(self._d)
        self._d = None


def change_spec(block: int = 0, thr_q4: int = 0, adapt_shift: int = 0, dilate: int = 0, min_blocks: int = 0, max_regions: int = 0) -> rf_change_spec:
    """An rf_change_spec; a zero means the default: block 8, 16 or 32 (16); thr_q4, the mean luma difference of a block in 1/16 grey
    levels (128); adapt_shift 0..8 (0: the reference becomes the frame); dilate 0 / 1 = grow the mask by one block, 2 = off;
    min_blocks (2); max_regions 1..64 (16)."""
    return rf_change_spec(C.sizeof(rf_change_spec), int(block), int(thr_q4), int(adapt_shift), int(dilate), int(min_blocks), int(max_regions), 0)


def _as_change_spec(spec) -> rf_change_spec:
    return spec if isinstance(spec, rf_change_spec) else change_spec(**(spec or {}))


def _change_grid(sp: rf_change_spec, rows: int, cols: int):
    b = sp.block or 16
    return -(-int(cols) // b), -(-int(rows) // b)


def change_step_host(frame: np.ndarray, ref: np.ndarray, counter: int, view_w: int, view_h: int, spec=None, margin: Optional[float] = None,
                     grid: int = 0, max_zoom: int = 0):
    """rf_change_step_host (host only, no GPU): one step of one stream -- the code the kernels run.  ref: the (bh, bw) int32 reference
    (not written), counter: the stream's frame counter (0: this step seeds).  Returns (ref, counter, mask, regions, cells, info): the
    new reference and counter, the (bh, bw) uint8 mask of changed blocks BEFORE dilation, the (R, 4) int32 regions, the (R, 8) int32
    cell records (roi_plan()'s columns; void behind info[2]) and info = (changed_blocks, components, kept, flags)."""
    lib = _lib.load_library()
    sp = _as_change_spec(spec)
    frame = _dense_frame(frame)
    bw, bh = _change_grid(sp, frame.shape[0], frame.shape[1])
    ref = np.array(ref, np.int32).reshape(-1)
    if ref.size != bw * bh:
        raise ValueError("ref: one int32 per block (%d x %d)" % (bh, bw))
    R = sp.max_regions or 16
    cnt = C.c_int64(int(counter))
    mask = np.full(max(bw * bh, 1), 0xAB, np.uint8)
    regions, cells, info = (rf_roi * max(R, 1))(), (rf_roi_cell * max(R, 1))(), _lib.rf_change_info()
    st = lib.rf_change_step_host(C.byref(sp), frame.ctypes.data, frame.shape[0], frame.shape[1], frame.strides[0], ref.ctypes.data, C.byref(cnt),
                                 _margin_q8(margin), int(view_w), int(view_h), C.byref(roi_spec(grid, max_zoom)), mask.ctypes.data, regions,
                                 cells, C.byref(info))
    if st < 0:
        raise _lib.RFError(st, "rf_change_step_host: bad spec, frame shape, view size, margin or counter")
    return (ref.reshape(bh, bw), int(cnt.value), mask.reshape(bh, bw), np.frombuffer(regions, np.int32, 4 * R).reshape(R, 4).copy(),
            _cell_rows(cells, R), np.array([info.changed_blocks, info.components, info.kept, info.flags], np.int32))


class Changer:
    """Change regions on a detector (rf_changer_create): a per-stream reference image of one frame shape -- one luma sum per block --
    in device memory.  Every step marks the blocks of a frame that differ from it, updates it and turns the marked blocks into at most
    max_regions regions on the device; detect_changed() detects inside them, next to a tracker's regions when one is given."""

    def __init__(self, det: "RetinaFace", rows: int, cols: int, n_streams: int = 1, **spec):
        self._det, self._c = det, None
        self.rows, self.cols, self.n_streams = int(rows), int(cols), int(n_streams)
        self.spec = change_spec(**spec)
        self.max_regions = self.spec.max_regions or 16
        self.bw, self.bh = _change_grid(self.spec, rows, cols)
        c = C.c_void_p()
        _lib.check(det._lib.rf_changer_create(det._h, C.byref(self.spec), self.rows, self.cols, self.n_streams, C.byref(c)), det._h)
        self._c = c
        self.truncated = False
        self.last_cells = self.last_info = None

    def close(self):
        if self._c is not None and getattr(self._det, "_h", None):
            self._det._lib.rf_changer_destroy(self._c)
        self._c = None

    def reset(self, stream: int = -1):
        """rf_changer_reset: the stream (-1: every stream, which also clears the error state) seeds again on its next step"""
        _lib.check(self._det._lib.rf_changer_reset(self._c, int(stream)), self._det._h)

    def read(self, stream: int):
        """rf_changer_read: (ref, frames, mask) of a stream -- the (bh, bw) int32 reference, the frame counter and the (bh, bw) uint8
        mask of the blocks the last step found changed (before dilation)"""
        ref = np.zeros((self.bh, self.bw), np.int32)
        mask = np.zeros((self.bh, self.bw), np.uint8)
        frames = C.c_int64()
        _lib.check(self._det._lib.rf_changer_read(self._c, int(stream), ref.ctypes.data, C.byref(frames), mask.ctypes.data), self._det._h)
        return ref, int(frames.value), mask

    def _info_rows(self, info, n):
        return np.frombuffer(info, np.int32, 4 * n).reshape(n, 4).copy() if n else np.zeros((0, 4), np.int32)

    def regions_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], streams: Sequence[int],
                       steps: Optional[Sequence[int]] = None, margin: Optional[float] = None, grid: int = 0, max_zoom: int = 0):
        """rf_change_regions_device: the two kernels alone over frames in device memory; they STEP the reference of streams[i] (-1, or
        a 0 / None pointer: nothing happens for the image).  Returns (cells, info): the (n, max_regions, 8) int32 cell records and the
        (n, 4) int32 info records (changed_blocks, components, kept, flags)."""
        n, R = len(ptrs), self.max_regions
        cells, info = (rf_roi_cell * max(n * R, 1))(), (_lib.rf_change_info * max(n, 1))()
        det = self._det
        _lib.check(det._lib.rf_change_regions_device(det._h, self._c, *_device_frames(ptrs, rows, cols, steps), (C.c_int * max(n, 1))(*streams), n,
                                                     _margin_q8(margin), C.byref(roi_spec(grid, max_zoom)), cells, info), det._h)
        return _cell_rows(cells, n * R).reshape(n, R, 8), self._info_rows(info, n)

    def _changed(self, fn, frames, streams, tracker, threshold, margin, grid, max_zoom, vote, max_faces, views_ptr, cap_ended, return_src_roi):
        det = self._det
        n = frames[4]
        sp = roi_spec(grid, max_zoom, vote, max_faces)
        cap = sp.max_faces or det.max_detections
        S = (tracker.max_tracks if tracker is not None else 0) + self.max_regions
        cells, info = (rf_roi_cell * max(n * S, 1))(), (_lib.rf_change_info * max(n, 1))()
        sarr = (C.c_int * max(n, 1))(*streams)
        if tracker is not None:
            t, _, tags, ended, ce, ec = tracker._buffers(n, cap, cap_ended)
        else:
            t, tags, ended, ce, ec = None, None, None, 0, None
        head = (det._h,) + tuple(frames) + (float(threshold), C.byref(sp), _margin_q8(margin))
        tail = (cells, views_ptr, self._c, info, t, sarr, tags, ended, ce, ec)
        dets, src, votes = det._merged_call(fn, head, n, cap, "roi_counts", True, tail=tail)      # the C call takes src_roi, then votes
        self.truncated = det.truncated
        self.last_cells = _cell_rows(cells, n * S).reshape(n, S, 8)
        self.last_info = self._info_rows(info, n)
        res = (dets,)
        if tracker is not None:
            tracker.truncated = det.truncated
            res += tracker._results(n, det.roi_counts, cap)
        return res + (votes, src) if return_src_roi else (res if tracker is not None else dets)

    def detect_changed(self, imgs: Sequence[np.ndarray], streams: Sequence[int], tracker: Optional["Tracker"] = None, threshold: float = 0.5,
                       margin: Optional[float] = None, grid: int = 0, max_zoom: int = 0, vote: bool = False, max_faces: int = 0,
                       cap_ended: Optional[int] = None, return_src_roi: bool = False):
        """rf_detect_change_roi_batch: every frame (of the changer's shape; None: an empty frame) steps the reference of streams[i]
        (-1: nothing happens) and is detected inside the change regions -- with `tracker` also inside the regions of its stream's track
        slots, exactly as Tracker.detect_tracked_rois(), region r < max_tracks being slot r and region max_tracks + k change slot k; the
        merged faces then go into the frame step, so a newcomer gets its id on the frame it appears in.  Returns the detections per
        frame in SOURCE-FRAME pixels; with a tracker (detections, tags per image, ended tracks per image); with return_src_roi also
        the member counts and the region of each face.  self.last_cells: the (n, T + R, 8) cell records, self.last_info: the (n, 4)
        info records."""
        f = _host_frames(imgs)
        return self._changed(self._det._lib.rf_detect_change_roi_batch, f.args, streams, tracker, threshold, margin, grid, max_zoom, vote,
                             max_faces, None, cap_ended, return_src_roi)

    def detect_changed_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], streams: Sequence[int],
                              tracker: Optional["Tracker"] = None, threshold: float = 0.5, steps: Optional[Sequence[int]] = None,
                              margin: Optional[float] = None, grid: int = 0, max_zoom: int = 0, vote: bool = False, max_faces: int = 0,
                              views_ptr: Optional[int] = None, cap_ended: Optional[int] = None, return_src_roi: bool = False):
        """rf_detect_change_roi_batch_device: detect_changed for frames resident in device memory (0 / None: an empty frame).
        views_ptr: device memory of passes * net_h * net_w * 3 bytes that receives the views as dense frames."""
        frames = _device_frames(ptrs, rows, cols, steps) + (len(ptrs),)
        return self._changed(self._det._lib.rf_detect_change_roi_batch_device, frames, streams, tracker, threshold, margin, grid, max_zoom, vote,
                             max_faces, views_ptr, cap_ended, return_src_roi)


ROI_CROPPED = _lib.RF_ROI_CROPPED
ROI_VOID = _lib.RF_ROI_VOID


def roi_spec(grid: int = 0, max_zoom: int = 0, vote: bool = False, max_faces: int = 0) -> rf_roi_spec:
    """An rf_roi_spec: grid (cells per axis of a view: 1, 2 or 4; 0 = 4), max_zoom (the largest enlargement of a region: 1, 2 or 4;
    0 = 2), vote (a kept box becomes the score-weighted mean of its cluster; off by default) and max_faces (0 = the engine's
    max_detections)."""
    sp = rf_roi_spec()
    sp.struct_size = C.sizeof(rf_roi_spec)
    sp.grid, sp.max_zoom, sp.vote, sp.max_faces, sp.reserved = int(grid), int(max_zoom), 1 if vote else 2, int(max_faces), 0
    return sp


def _roi_array(rois):
    """a ctypes rf_roi array (at least one entry) of (x, y, w, h) rows, and their number"""
    rows = [tuple(int(v) for v in r) for r in rois]
    arr = (rf_roi * max(len(rows), 1))()
    for i, (x, y, w, h) in enumerate(rows):
        arr[i].x, arr[i].y, arr[i].w, arr[i].h = x, y, w, h
    return arr, len(rows)


def _roi_lists(rois_per_frame):
    """the regions of a call's frames as (rf_roi array, frame-major; per-frame counts as a ctypes int array; the counts as a list)"""
    counts = [len(r) for r in rois_per_frame]
    arr, _ = _roi_array([r for frame in rois_per_frame for r in frame])
    return arr, (C.c_int * max(len(counts), 1))(*counts), counts


def _cell_rows(cells, n: int) -> np.ndarray:
    """(n, 8) int32 rows of x, y, w, h, level, x0, y0, flags of a ctypes rf_roi_cell array"""
    return np.frombuffer(cells, np.int32, 8 * n).reshape(n, 8).copy() if n else np.zeros((0, 8), np.int32)


def _margin_q8(margin: Optional[float]) -> int:
    """a margin in 1/256ths for the C ABI, which reads 0 as its default (a quarter): None is that default, a margin that rounds to 0 is
    refused here rather than silently becoming a quarter"""
    if margin is None:
        return 0
    q8 = int(round(margin * 256))
    if q8 == 0:
        raise _lib.RFError(_lib.RF_ERR_INVALID_ARG, "a margin below 1 / 512 cannot be expressed (0 means the default); pass None for the default")
    return q8


def roi_cells_from_tracks(table, view_w: int, view_h: int, motion=None, mspec=None, margin: Optional[float] = None, grid: int = 0,
                          max_zoom: int = 0) -> np.ndarray:
    """rf_roi_cells_from_tracks (host only, no GPU): the (max_tracks, 8) int32 cell records (roi_plan()'s columns) of one stream's
    table (TRACK_DTYPE) -- slot r is region r; a free slot, or a box rois_from_faces() would skip, is the void record (zeros, flags
    ROI_VOID).  motion: None (a plain tracker) or the stream's MOTION_DTYPE records, read with mspec (an rf_motion_spec or motion_spec()'s keywords; None: the defaults)."""
    lib = _lib.load_library()
    table = np.ascontiguousarray(table)
    T = len(table)
    m = np.ascontiguousarray(motion) if motion is not None else None
    if table.ndim != 1 or table.dtype.itemsize != TRACK_DTYPE.itemsize or (m is not None and (m.shape != (T,) or m.dtype.itemsize != MOTION_DTYPE.itemsize)):
        raise ValueError("table: a 1-d array of TRACK_DTYPE records; motion: one MOTION_DTYPE record per slot")
    cells = (rf_roi_cell * max(T, 1))()
    ms = _as_motion_spec(mspec)
    st = lib.rf_roi_cells_from_tracks(None, C.byref(ms) if ms is not None else None, table.ctypes.data_as(C.POINTER(rf_track)),
                                      m.ctypes.data_as(C.POINTER(rf_track_motion)) if m is not None else None, T, _margin_q8(margin),
                                      int(view_w), int(view_h), C.byref(roi_spec(grid, max_zoom)), cells)
    if st < 0:
        raise _lib.RFError(st, "rf_roi_cells_from_tracks: bad spec, view size, margin or table")
    return _cell_rows(cells, T)


def roi_plan(rois, view_w: int, view_h: int, grid: int = 0, max_zoom: int = 0):
    """rf_roi_plan (host only, no GPU): (cells, passes) of one frame's regions in views of view_w x view_h -- cells: an (n, 8) int32 array
    of x, y, w, h, level (log2 of the step), x0, y0 (the cell's origin in level pixels) and flags (ROI_CROPPED)."""
    lib = _lib.load_library()
    arr, n = _roi_array(rois)
    cells = (_lib.rf_roi_cell * max(n, 1))()
    passes = C.c_int(0)
    st = lib.rf_roi_plan(C.byref(roi_spec(grid, max_zoom)), int(view_w), int(view_h), arr, n, cells, C.byref(passes))
    if st < 0:
        raise _lib.RFError(st, "rf_roi_plan: bad spec, view size or region")
    out = np.array([[c.roi.x, c.roi.y, c.roi.w, c.roi.h, c.level, c.x0, c.y0, c.flags] for c in cells[:n]], np.int32).reshape(n, 8)
    return out, int(passes.value)


def rois_from_faces(faces, coord_scale: float = 1.0, margin: Optional[float] = None):
    """rf_roi_from_faces (host only, no GPU): the regions (x, y, w, h) of faces (Detections or rows of 15 floats) -- each box times
    coord_scale, grown on every side by `margin` of its longer side (passed on in 1/256ths; None: the C default, a quarter), lower
    edges floored, upper edges ceiled.  The C ABI reads a margin of 0 as its default, so a margin that rounds to 0 / 256 is refused
    here rather than silently becoming a quarter.  A call's detections can so be handed to the next call as its regions."""
    lib = _lib.load_library()
    rows = _face_rows(faces)
    n = len(rows)
    q8 = 0 if margin is None else int(round(margin * 256))
    if margin is not None and q8 == 0:
        raise _lib.RFError(_lib.RF_ERR_INVALID_ARG, "rois_from_faces: a margin below 1 / 512 cannot be expressed (0 means the default); pass None for the default")
    out = (rf_roi * max(n, 1))()
    k = lib.rf_roi_from_faces(rows.ctypes.data_as(C.POINTER(rf_face)), n, float(coord_scale), q8, out)
    if k < 0:
        raise _lib.RFError(k, "rf_roi_from_faces: bad coord_scale or margin")
    return [(out[i].x, out[i].y, out[i].w, out[i].h) for i in range(k)]


def roi_atlas_host(frame: np.ndarray, rois, view_w: int, view_h: int, grid: int = 0, max_zoom: int = 0) -> np.ndarray:
    """rf_roi_atlas_host (host only, no GPU): the views of one frame's regions, a (passes, view_h, view_w, 3) uint8 array."""
    lib = _lib.load_library()
    frame = _dense_frame(frame)
    arr, n = _roi_array(rois)
    g = int(grid) or 4
    out = np.zeros((-(-n // (g * g)), int(view_h), int(view_w), 3), np.uint8)
    st = lib.rf_roi_atlas_host(C.byref(roi_spec(grid, max_zoom)), int(view_w), int(view_h), frame.ctypes.data, frame.shape[0], frame.shape[1],
                               frame.strides[0], arr, n, out.ctypes.data, 3 * int(view_w))
    if st < 0:
        raise _lib.RFError(st, "rf_roi_atlas_host: bad spec, view size, region or frame")
    return out


def roi_map_face(face, rois, pass_index: int, view_w: int, view_h: int, grid: int = 0, max_zoom: int = 0):
    """rf_roi_map_face (host only, no GPU): the face (a Detection or 15 floats) of pass `pass_index` of one frame's regions moved into
    the frame, (15 float32, its region) -- or None when the face rule drops it."""
    lib = _lib.load_library()
    arr, n = _roi_array(rois)
    f, g = rf_face(), rf_face()
    C.memmove(C.byref(f), _face_rows([face]).ctypes.data, 60)
    region = C.c_int(0)
    st = lib.rf_roi_map_face(C.byref(roi_spec(grid, max_zoom)), int(view_w), int(view_h), arr, n, int(pass_index), C.byref(f), C.byref(g),
                             C.byref(region))
    if st < 0:
        raise _lib.RFError(st, "rf_roi_map_face: bad spec, view size, region or pass")
    return (np.frombuffer(bytes(g)[:60], np.float32).copy(), int(region.value)) if st else None


def roi_merge_host(passes, rois, view_w: int, view_h: int, nms_threshold: float, max_detections: int, grid: int = 0, max_zoom: int = 0,
                   vote: bool = False, max_faces: int = 0, cap: Optional[int] = None):
    """rf_roi_merge_host (host only, no GPU): face rule and merge of ONE frame -- passes[p]: the faces of pass p in score order.
    Returns (faces (j, 15) float32, the true number of heads, votes (j,) int32, src_roi (j,) int32, truncated)."""
    lib = _lib.load_library()
    sp = roi_spec(grid, max_zoom, vote, max_faces)
    md = int(max_detections)
    if md < 1:
        raise _lib.RFError(_lib.RF_ERR_INVALID_ARG, "rf_roi_merge_host: max_detections must be positive")
    arr, n = _roi_array(rois)
    flat, pc = _pack_passes(passes, md)
    cap = int(cap) if cap is not None else (sp.max_faces or md)
    out = (rf_face * max(cap, 1))()
    votes, src = (C.c_int * max(cap, 1))(), (C.c_int * max(cap, 1))()
    count = C.c_int(0)
    st = lib.rf_roi_merge_host(C.byref(sp), int(view_w), int(view_h), arr, n, float(nms_threshold), md, flat.ctypes.data_as(C.POINTER(rf_face)),
                               pc, out, cap, C.byref(count), votes, src)
    if st < 0 and st != _lib.RF_ERR_TRUNCATED:
        raise _lib.RFError(st, "rf_roi_merge_host: bad spec, view size, regions or counts")
    k = min(count.value, cap, sp.max_faces or md)
    return (_faces_to_array(out, max(cap, 1))[:k].copy(), int(count.value), np.array(votes[:k], np.int32), np.array(src[:k], np.int32),
            st == _lib.RF_ERR_TRUNCATED)


def enhance_spec(tile: int = 0, clip: int = 0, dark_below: int = 0) -> rf_enhance_spec:
    """An rf_enhance_spec: tile (the tile edge in pixels: 16, 32, 64 or 128; 0 = 64), clip (the contrast limit in 1/256ths of a tile's
    mean bin count, 256..65535; 0 = 2048), dark_below (a tile is enhanced only when its p99 luma is below this, 1..256; 0 = 64)."""
    sp = rf_enhance_spec()
    sp.struct_size = C.sizeof(rf_enhance_spec)
    sp.tile, sp.clip, sp.dark_below = int(tile), int(clip), int(dark_below)
    return sp


def enhance_host(frame: np.ndarray, tile: int = 0, clip: int = 0, dark_below: int = 0, out: Optional[np.ndarray] = None, spec=None):
    """rf_enhance_host (host only, no GPU): the low-light enhancement of a BGR frame -- contrast-limited adaptive histogram
    equalisation of luma over tile x tile tiles, applied to the dark tiles as a hue-preserving gain.  `out`: a uint8 (rows, >= cols, 3)
    view to write into (its row pitch is kept; it may be `frame` itself).  Returns (enhanced frame, number of tiles enhanced)."""
    lib = _lib.load_library()
    frame = _dense_frame(frame)
    rows, cols = frame.shape[:2]
    if out is None:
        out = np.zeros((rows, cols, 3), np.uint8)
    if out.dtype != np.uint8 or out.ndim != 3 or out.shape[2] != 3 or out.strides[2] != 1 or out.strides[1] != 3 or out.shape[0] < rows:
        raise ValueError("out must be a uint8 (rows, cols, 3) array or row-pitched view")
    sp = spec if spec is not None else enhance_spec(tile, clip, dark_below)
    tiles = C.c_int(0)
    st = lib.rf_enhance_host(C.byref(sp), frame.ctypes.data, rows, cols, frame.strides[0] if rows else 3 * cols, out.ctypes.data,
                             out.strides[0] if out.shape[0] else 3 * cols, C.byref(tiles))
    if st < 0:
        raise _lib.RFError(st, "rf_enhance_host: bad spec, a destination pitch below cols * 3, or a destination that overlaps the frame")
    return out, int(tiles.value)


def pyramid_spec(levels: int = 0, overlap: int = 0, edge: int = 0, full_frame: bool = True, max_faces: int = 0,
                 vote: bool = True) -> rf_pyramid_spec:
    """An rf_pyramid_spec: levels (bit 0: the 1x passes, bit 1: 2x zoom tiles, bit 2: 4x zoom tiles; 0 = 3), overlap / edge /
    full_frame / max_faces as tile_spec (overlap and edge in net pixels at every level), vote as tta_spec."""
    sp = rf_pyramid_spec()
    sp.struct_size = C.sizeof(rf_pyramid_spec)
    sp.levels, sp.overlap, sp.edge, sp.full_frame, sp.max_faces, sp.vote = (int(levels), int(overlap), int(edge), 1 if full_frame else 2,
                                                                            int(max_faces), 1 if vote else 2)
    return sp


def pyramid_plan(rows: int, cols: int, net_h: int, net_w: int, levels: int = 0, overlap: int = 0, full_frame: bool = True,
                 spec=None) -> np.ndarray:
    """rf_pyramid_plan (host only, no GPU): the passes of a rows x cols frame at a net_h x net_w net as a (passes, 5) int32 array of
    z, x0, y0, tw, th in the level's virtual pixels -- the 1x passes of tile_plan, then the 2x tiles, then the 4x tiles."""
    lib = _lib.load_library()
    sp = spec if spec is not None else pyramid_spec(levels, overlap, 0, full_frame)
    n = lib.rf_pyramid_plan(C.byref(sp), int(rows), int(cols), int(net_h), int(net_w), None, 0)
    if n < 0:
        raise _lib.RFError(n, "rf_pyramid_plan: bad spec, frame or net size, more than 1024 passes or zoom tiles above 1 GiB")
    out = np.zeros((n, 5), np.int32)
    lib.rf_pyramid_plan(C.byref(sp), int(rows), int(cols), int(net_h), int(net_w), out.ctypes.data_as(C.POINTER(C.c_int)), n)
    return out


def pyramid_map_face(face, p: int, rows: int, cols: int, net_h: int, net_w: int, levels: int = 0, overlap: int = 0, edge: int = 0,
                     full_frame: bool = True):
    """rf_pyramid_map_face (host only, no GPU): the face (a Detection or 15 floats) of pass p of the pyramid plan moved into
    source-frame pixels as 15 float32, or None when the edge rule drops it."""
    lib = _lib.load_library()
    sp = pyramid_spec(levels, overlap, edge, full_frame)
    f = rf_face.from_buffer_copy(_face_rows([face])[0].tobytes())
    g = rf_face()
    st = lib.rf_pyramid_map_face(C.byref(sp), int(rows), int(cols), int(net_h), int(net_w), int(p), C.byref(f), C.byref(g))
    if st < 0:
        raise _lib.RFError(st, "rf_pyramid_map_face: bad spec, frame, net size or pass index")
    return _faces_to_array(C.pointer(g), 1)[0] if st else None


def pyramid_merge_host(passes, rows: int, cols: int, net_h: int, net_w: int, nms_threshold: float, max_detections: int, levels: int = 0,
                       overlap: int = 0, edge: int = 0, full_frame: bool = True, max_faces: int = 0, vote: bool = True,
                       cap: Optional[int] = None, spec=None):
    """rf_pyramid_merge_host (host only, no GPU): edge rule, mapping and merge of ONE frame -- passes[p]: the faces of pass p of the
    pyramid plan (a (k, 15) array, rows of 15 floats or Detections).  Returns (faces (k, 15) float32 in merge order, count: the true
    number of heads, votes (k,) int32, src_pass (k,) int32, truncated)."""
    lib = _lib.load_library()
    sp = spec if spec is not None else pyramid_spec(levels, overlap, edge, full_frame, max_faces, vote)
    md = int(max_detections)
    if md < 1:
        raise _lib.RFError(_lib.RF_ERR_INVALID_ARG, "rf_pyramid_merge_host: max_detections must be positive")
    want = lib.rf_pyramid_plan(C.byref(sp), int(rows), int(cols), int(net_h), int(net_w), None, 0)
    if want < 0 or len(passes) != want:
        raise _lib.RFError(_lib.RF_ERR_INVALID_ARG, "rf_pyramid_merge_host: bad spec or frame, or not one list of faces per pass of the plan")
    flat, pc = _pack_passes(passes, md)
    cap = int(cap) if cap is not None else (sp.max_faces or md)
    out = (rf_face * max(cap, 1))()
    votes, src = (C.c_int * max(cap, 1))(), (C.c_int * max(cap, 1))()
    count = C.c_int(0)
    st = lib.rf_pyramid_merge_host(C.byref(sp), int(rows), int(cols), int(net_h), int(net_w), float(nms_threshold), md,
                                   flat.ctypes.data_as(C.POINTER(rf_face)), pc, out, cap, C.byref(count), votes, src)
    if st < 0 and st != _lib.RF_ERR_TRUNCATED:
        raise _lib.RFError(st, "rf_pyramid_merge_host: bad spec, frame, net size or counts")
    k = max(0, min(count.value, cap, sp.max_faces or md))
    return (_faces_to_array(out, max(cap, 1))[:k], int(count.value), np.array(votes[:k], np.int32), np.array(src[:k], np.int32),
            st == _lib.RF_ERR_TRUNCATED)


def zoom_host(frame: np.ndarray, z: int, x0: int = 0, y0: int = 0, tw: Optional[int] = None, th: Optional[int] = None,
              out: Optional[np.ndarray] = None) -> np.ndarray:
    """rf_zoom_host (host only, no GPU): the window [x0, x0 + tw) x [y0, y0 + th) of the BGR frame enlarged z (2 or 4) times (integer
    bilinear, half-pixel centres; default: the whole enlarged frame).  `out`: a uint8 (th, >= tw, 3) view to write into (its row
    pitch is kept); returned either way."""
    lib = _lib.load_library()
    frame = _dense_frame(frame)
    rows, cols = frame.shape[:2]
    tw = int(z) * cols - int(x0) if tw is None else int(tw)
    th = int(z) * rows - int(y0) if th is None else int(th)
    if out is None:
        out = np.zeros((max(th, 0), max(tw, 0), 3), np.uint8)
    if out.dtype != np.uint8 or out.ndim != 3 or out.shape[2] != 3 or out.strides[2] != 1 or out.strides[1] != 3 or out.shape[0] < th:
        raise ValueError("out must be a uint8 (th, tw, 3) array or row-pitched view")
    st = lib.rf_zoom_host(frame.ctypes.data, rows, cols, frame.strides[0] if rows else 3 * cols, int(z), int(x0), int(y0), tw, th,
                          out.ctypes.data, out.strides[0] if out.shape[0] else 3 * max(tw, 0))
    if st < 0:
        raise _lib.RFError(st, "rf_zoom_host: z must be 2 or 4 and the window must lie inside the enlarged frame")
    return out


def debug_resident_cap(workgroups: int = 0) -> None:
    """rf_debug_resident_cap: process-wide test hook.  A positive value replaces the chip's resident workgroup count in the persistent
    launches' grid rule, so small inputs walk several tiles per workgroup; 0 = the production grids.  Clears the grid log."""
    _lib.load_library().rf_debug_resident_cap(int(workgroups))


def debug_grid_log() -> List[tuple]:
    """rf_debug_grid_log: the (tiles, grid) pairs the persistent launches were given since the last debug_resident_cap(), in call order."""
    cap = 256
    tiles, grid = (C.c_int * cap)(), (C.c_int * cap)()
    n = _lib.check(_lib.load_library().rf_debug_grid_log(cap, tiles, grid))
    return [(tiles[i], grid[i]) for i in range(min(n, cap))]


def debug_face_bands(crop_size: int, format: int) -> tuple:
    """rf_debug_face_bands: host-only test hook.  (band_rows, ring_rows): the crop rows one workgroup of the face-crop kernels covers for
    this crop size and format (RF_FACES_*: 0 u8 HWC, 1 f16 CHW, 2 f32 CHW), and the luma rows the quality kernel keeps in LDS."""
    band, ring = C.c_int(), C.c_int()
    _lib.check(_lib.load_library().rf_debug_face_bands(int(crop_size), int(format), C.byref(band), C.byref(ring)))
    return band.value, ring.value


def _faces_to_array(buf, n: int) -> np.ndarray:
    return np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_float)), shape=(n, 15)).copy()


class RetinaFace:
    def __init__(self, model: str, network: str = "net3", nms: float = 0.4, *, precision: int = PRECISION_FP16,
                 net_hw: Optional[tuple] = None, max_batch: int = 8, model_stem: Optional[str] = None,
                 max_candidates: int = 0, max_detections: int = 0, use_graph: bool = True,
                 keep_outputs: bool = False, device: Optional[int] = None, lanes: int = 0, coalesce: int = 0,
                 devices: Optional[Sequence[int]] = None, copy_threads: int = 0, plan_cache: bool = True,
                 oversize_resize: str = "area"):
        self._lib = _lib.load_library()
        o = rf_options()
        o.struct_size = C.sizeof(rf_options)
        o.precision = precision
        if net_hw:
            o.net_h, o.net_w = int(net_hw[0]), int(net_hw[1])
        o.max_batch = max_batch
        o.device = 0 if device is None else device + 1
        o.max_candidates = max_candidates
        o.max_detections = max_detections
        o.use_graph = 1 if use_graph else 2
        o.keep_outputs = 1 if keep_outputs else 0
        o.lanes = lanes
        o.coalesce = coalesce
        o.copy_threads = copy_threads
        o.plan_cache = 1 if plan_cache else 2
        o.oversize_resize = {"area": 1, "bilinear": 2}[oversize_resize]
        if devices:       # more than one entry: one engine per entry, detectBatchImages sharded by image over them
            self._devices = (C.c_int32 * len(devices))(*devices)
            o.devices, o.n_devices = self._devices, len(devices)
        self._stem = model_stem.encode() if model_stem else None
        o.model_stem = self._stem
        h = C.c_void_p()
        _lib.check(self._lib.rf_create(model.encode(), network.encode(), float(nms), C.byref(o), C.byref(h)))
        self._h = h
        nh, nw, mb = C.c_int(), C.c_int(), C.c_int()
        self._lib.rf_get_net_size(self._h, C.byref(nh), C.byref(nw), C.byref(mb))
        self.net_h, self.net_w, self.max_batch = nh.value, nw.value, mb.value
        self.max_detections = max_detections or 256
        self.truncated = False

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ reference entry points
    def detect(self, img: np.ndarray, threshold: float = 0.5, scales: float = 1.0) -> List[Detection]:
        """RetinaFace::detect(const Mat&, float threshold = 0.5, float scales = 1.0); `scales` is unused there too."""
        if img is None or img.size == 0:
            return []
        return self.detectBatchImages([img], threshold)[0]

    def detectBatchImages(self, imgs: Sequence[np.ndarray], threshold: float = 0.5) -> List[List[Detection]]:
        n = len(imgs)
        if n == 0:
            return []
        f = _host_frames(imgs)
        return self._run(self._lib.rf_detect_batch, *f.args, threshold)

    def frame_scale(self, rows: int, cols: int) -> float:
        """Multiply returned coordinates by this to get source-frame pixels (1.0 unless the frame is larger than the net)."""
        return float(self._lib.rf_frame_scale(self._h, int(rows), int(cols)))

    def detect_pad32(self, imgs: Sequence[np.ndarray], threshold: float = 0.5) -> List[List[Detection]]:
        """The reference's Caffe-build detect (RetinaFace.cpp:943-1075): no resize, each frame zero-padded to the next
        multiple of 32 and run at that size, boxes clipped to the padded size, coordinates in source-frame pixels.
        anchor_index of the returned detections is -1 (anchor tables differ per size)."""
        n = len(imgs)
        if n == 0:
            return []
        f = _host_frames(imgs)
        cap = self.max_detections
        out = (rf_face * (n * cap))()
        counts = (C.c_int * n)()
        st = _lib.check(self._lib.rf_detect_batch_pad32(self._h, *f.args, 0, float(threshold), out, cap, counts), self._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        return self._collect(out, counts, n, cap, anchors=False)

    # ------------------------------------------------------------------ device-resident frames
    def detect_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], threshold: float = 0.5,
                      steps: Optional[Sequence[int]] = None) -> List[List[Detection]]:
        n = len(ptrs)
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        return self._run(self._lib.rf_detect_batch_device, p, r, c, s, n, threshold)

    # ------------------------------------------------------------------ face alignment
    def align(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], faces, *, steps: Optional[Sequence[int]] = None,
              coord_scale: Optional[Sequence[float]] = None, crop_size: int = 112, max_faces: Optional[int] = None,
              d_crops: Optional[int] = None, host: bool = True):
        """rf_align_batch_device: aligned crops of faces the caller supplies, from device-resident frames.  faces[i]: the faces of
        image i (a (k, 15) array, rows of 15 floats or Detections).  coord_scale[i] multiplies image i's landmarks into source
        pixels (frame_scale() for detect results of an oversize frame; default 1).  Returns (crops, matrices): per image a
        (k, S, S, 3) uint8 array (None with host=False) and a (k, 2, 3) float64 array, k = min(len(faces[i]), max_faces).
        d_crops: a device buffer of n * max_faces * 3 * S * S bytes that receives the crops as well (slot i * max_faces + k)."""
        n = len(ptrs)
        rows_f = [_face_rows(f) for f in faces]
        if len(rows_f) != n:
            raise ValueError("faces must hold one entry per frame")
        cap = max(1, max((len(r) for r in rows_f), default=1))
        mf = int(max_faces) if max_faces else cap
        flat = np.zeros((n, cap, 15), np.float32)
        counts = (C.c_int * max(n, 1))()
        for i, r in enumerate(rows_f):
            flat[i, :len(r)] = r
            counts[i] = len(r)
        p, r_, c_, s_ = _device_frames(ptrs, rows, cols, steps)
        cs = None
        if coord_scale is not None:
            cs = (C.c_float * max(n, 1))(*[float(v) for v in coord_scale])
        S = int(crop_size)
        crops = np.zeros((n, mf, S, S, 3), np.uint8) if host else None
        mats = np.zeros((n, mf, 2, 3), np.float64)
        _lib.check(self._lib.rf_align_batch_device(
            self._h, p, r_, c_, s_, n, flat.ctypes.data_as(C.POINTER(rf_face)), cap, counts, cs, S, mf,
            C.c_void_p(d_crops) if d_crops else None, crops.ctypes.data if host else None,
            mats.ctypes.data_as(C.POINTER(C.c_double))), self._h)
        ks = [min(counts[i], mf) for i in range(n)]
        return ([crops[i, :ks[i]] for i in range(n)] if host else None), [mats[i, :ks[i]] for i in range(n)]

    def detect_aligned(self, imgs: Sequence[np.ndarray], threshold: float = 0.5, crop_size: int = 112,
                       max_faces: Optional[int] = None):
        """rf_detect_align_batch: detectBatchImages + the aligned crop of every face, in one call.  Returns (detections, crops,
        matrices): crops[i] is (k, S, S, 3) uint8 and matrices[i] (k, 2, 3) float64 for the first k = min(faces, max_faces)
        detections of image i (score order); frames larger than the net are sampled at their full resolution."""
        n = len(imgs)
        if n == 0:
            return [], [], []
        f = _host_frames(imgs)
        return self._run_aligned(self._lib.rf_detect_align_batch, *f.args, threshold, crop_size, max_faces, None, True)

    def detect_aligned_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], threshold: float = 0.5,
                              steps: Optional[Sequence[int]] = None, crop_size: int = 112, max_faces: Optional[int] = None,
                              d_crops: Optional[int] = None, host: bool = True):
        """rf_detect_align_batch_device: detect_aligned for frames resident in device memory.  d_crops: a device buffer of
        n * max_faces * 3 * S * S bytes that receives the crops (slot i * max_faces + k); host=False skips the host copy of
        the crops (crops is then None)."""
        n = len(ptrs)
        if n == 0:
            return [], [], []
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        return self._run_aligned(self._lib.rf_detect_align_batch_device, p, r, c, s, n, threshold, crop_size, max_faces, d_crops, host)

    def _run_aligned(self, fn, ptrs, rows, cols, steps, n, threshold, crop_size, max_faces, d_crops, host):
        cap = self.max_detections
        mf = int(max_faces) if max_faces else cap
        S = int(crop_size)
        out = (rf_face * (n * cap))()
        counts = (C.c_int * n)()
        crops = np.zeros((n, mf, S, S, 3), np.uint8) if host else None
        mats = np.zeros((n, mf, 2, 3), np.float64)
        st = _lib.check(fn(self._h, ptrs, rows, cols, steps, n, float(threshold), out, cap, counts, S, mf,
                           C.c_void_p(d_crops) if d_crops else None, crops.ctypes.data if host else None,
                           mats.ctypes.data_as(C.POINTER(C.c_double))), self._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        dets = self._collect(out, counts, n, cap)
        ks = [min(len(d), mf) for d in dets]
        return dets, ([crops[i, :ks[i]] for i in range(n)] if host else None), [mats[i, :ks[i]] for i in range(n)]

    # ------------------------------------------------------------------ face batches
    def detect_face_batch(self, imgs: Sequence[np.ndarray], threshold: float = 0.5, **kw):
        """rf_detect_face_batch: detectBatchImages + the faces it finds as ONE dense recogniser-ready tensor.  Keywords:
        crop_size (112), dtype ("u8" HWC | "f16" | "f32" CHW; default "f16"), rgb (True), mean / scale (per output channel; default
        (v - 127.5) / 128), max_faces (per image; default max_detections), capacity (packed faces the tensor holds; default
        n * max_faces), d_out (a device buffer of capacity faces that receives the tensor as well), host (False skips the host
        copy).  Returns (detections, tensor, matrices, offsets): tensor is [min(total, capacity), 3, S, S] (u8: [.., S, S, 3]),
        matrices [.., 2, 3] float64, offsets [n + 1]: face k of image i is tensor[offsets[i] + k].  self.faces_truncated tells
        whether total exceeded the capacity.
        gate= (an rf_face_gate from face_gate(), or a dict of its keywords) packs only the faces that pass it;
        return_quality=True appends a fifth result: per image a QUALITY_DTYPE array with the record of every considered face
        (k < min(faces, max_faces)), kept or dropped.  With neither, the ungated C entry point is called.
        antialias=True supersamples faces that are larger in the frame than their crop, with up to aa_max (1, 2, 4, 8; 0 = 4)
        sub-samples per axis (face_aa_factor gives a face's factor); the records' luma numbers are then the antialiased crop's."""
        f = _host_frames(imgs)
        return self._run_face_batch(self._lib.rf_detect_face_batch, self._lib.rf_detect_face_batch_gated, *f.args, threshold, **kw)

    def detect_face_batch_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], threshold: float = 0.5,
                                 steps: Optional[Sequence[int]] = None, **kw):
        """rf_detect_face_batch_device: detect_face_batch for frames resident in device memory."""
        n = len(ptrs)
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        return self._run_face_batch(self._lib.rf_detect_face_batch_device, self._lib.rf_detect_face_batch_gated_device, p, r, c, s, n,
                                    threshold, **kw)

    def face_batch(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], faces, *, steps: Optional[Sequence[int]] = None,
                   coord_scale: Optional[Sequence[float]] = None, **kw):
        """rf_face_batch_device: the face batch of faces the caller supplies (faces / coord_scale as align()).  Returns
        (None, tensor, matrices, offsets)."""
        n = len(ptrs)
        rows_f = [_face_rows(f) for f in faces]
        if len(rows_f) != n:
            raise ValueError("faces must hold one entry per frame")
        cap = max(1, max((len(r) for r in rows_f), default=1))
        flat = np.zeros((max(n, 1), cap, 15), np.float32)
        counts = (C.c_int * max(n, 1))()
        for i, r in enumerate(rows_f):
            flat[i, :len(r)] = r
            counts[i] = len(r)
        p, r_, c_, s_ = _device_frames(ptrs, rows, cols, steps)
        cs = (C.c_float * max(n, 1))(*[float(v) for v in coord_scale]) if coord_scale is not None else None

        def fn(h, spec, d_out, tensor, mats, offsets, gate=None, quality=None):
            if gate is None and quality is None:
                return self._lib.rf_face_batch_device(h, p, r_, c_, s_, n, flat.ctypes.data_as(C.POINTER(rf_face)), cap, counts, cs,
                                                      spec, d_out, tensor, mats, offsets)
            return self._lib.rf_face_batch_gated_device(h, p, r_, c_, s_, n, flat.ctypes.data_as(C.POINTER(rf_face)), cap, counts, cs,
                                                        spec, d_out, tensor, mats, offsets, gate, quality)
        kw.setdefault("max_faces", cap)
        res = self._face_batch_call(fn, n, **kw)
        if len(res) == 4:
            res = res[:3] + ([res[3][i, :min(counts[i], res[3].shape[1])] for i in range(n)],)
        return (None,) + res

    def face_quality(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], faces, *, steps: Optional[Sequence[int]] = None,
                     coord_scale: Optional[Sequence[float]] = None, crop_size: int = 112, max_faces: Optional[int] = None, gate=None):
        """rf_face_quality_device: the quality records of faces the caller supplies (faces / coord_scale as align()); no tensor is
        written.  Returns per image a QUALITY_DTYPE array of k = min(len(faces[i]), max_faces) records; flags are those of `gate`."""
        n = len(ptrs)
        rows_f = [_face_rows(f) for f in faces]
        if len(rows_f) != n:
            raise ValueError("faces must hold one entry per frame")
        cap = max(1, max((len(r) for r in rows_f), default=1))
        mf = int(max_faces) if max_faces else cap
        flat = np.zeros((max(n, 1), cap, 15), np.float32)
        counts = (C.c_int * max(n, 1))()
        for i, r in enumerate(rows_f):
            flat[i, :len(r)] = r
            counts[i] = len(r)
        p, r_, c_, s_ = _device_frames(ptrs, rows, cols, steps)
        cs = (C.c_float * max(n, 1))(*[float(v) for v in coord_scale]) if coord_scale is not None else None
        g = _as_gate(gate)
        q = np.zeros((max(n, 1), max(mf, 1)), QUALITY_DTYPE)
        _lib.check(self._lib.rf_face_quality_device(self._h, p, r_, c_, s_, n, flat.ctypes.data_as(C.POINTER(rf_face)), cap, counts, cs,
                                                    int(crop_size), mf, C.byref(g) if g is not None else None,
                                                    q.ctypes.data_as(C.POINTER(rf_face_quality))), self._h)
        return [q[i, :min(counts[i], mf)].copy() for i in range(n)]

    def _run_face_batch(self, fn, gated_fn, ptrs, rows, cols, steps, n, threshold, **kw):
        cap = self.max_detections
        out = (rf_face * max(n * cap, 1))()
        counts = (C.c_int * max(n, 1))()

        def call(h, spec, d_out, tensor, mats, offsets, gate=None, quality=None):
            if gate is None and quality is None:
                return fn(h, ptrs, rows, cols, steps, n, float(threshold), out, cap, counts, spec, d_out, tensor, mats, offsets)
            return gated_fn(h, ptrs, rows, cols, steps, n, float(threshold), out, cap, counts, spec, d_out, tensor, mats, offsets,
                            gate, quality)
        res = self._face_batch_call(call, n, **kw)
        if len(res) == 4:
            res = res[:3] + ([res[3][i, :min(counts[i], res[3].shape[1], cap)] for i in range(n)],)
        return (self._collect(out, counts, n, cap),) + res

    def _face_batch_call(self, call, n, crop_size: int = 112, dtype: str = "f16", rgb: bool = True, mean=None, scale=None,
                         max_faces: Optional[int] = None, capacity: Optional[int] = None, d_out: Optional[int] = None, host: bool = True,
                         gate=None, return_quality: bool = False, antialias: bool = False, aa_max: int = 0):
        mf = int(max_faces) if max_faces else self.max_detections
        capacity = int(capacity) if capacity is not None else max(1, n * mf)
        sp = face_batch_spec(crop_size, dtype, rgb, mean, scale, mf, capacity, antialias, aa_max)
        S = int(crop_size) if crop_size else 112
        shape = (S, S, 3) if dtype == "u8" else (3, S, S)
        tensor = np.zeros((max(capacity, 0),) + shape, _FACE_FORMATS[dtype][1]) if host else None
        mats = np.zeros((max(capacity, 0), 2, 3), np.float64)
        offsets = (C.c_int * (n + 1))()
        args = (self._h, C.byref(sp), C.c_void_p(d_out) if d_out else None, tensor.ctypes.data if host else None,
                mats.ctypes.data_as(C.POINTER(C.c_double)), offsets)
        quality = None
        if gate is not None or return_quality:
            g = _as_gate(gate)
            quality = np.zeros((max(n, 1), max(mf, 1)), QUALITY_DTYPE)
            # (the records are always fetched: they are what makes this the gated entry point when the gate is None)
            args += (C.byref(g) if g is not None else None, quality.ctypes.data_as(C.POINTER(rf_face_quality)))
        st = _lib.check(call(*args), self._h)
        offsets = np.array(offsets[:n + 1], np.int32)
        got = min(int(offsets[n]), capacity)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        self.faces_truncated = int(offsets[n]) > capacity
        res = (tensor[:got] if host else None), mats[:got], offsets
        return res + (quality,) if return_quality else res

    # ------------------------------------------------------------------ merged calls: tiled, TTA, rotation, dewarp, pyramid
    # Every C call of these five families ends (..., out, cap_per_image, counts, [votes,] src, extra outputs): per frame up to cap merged
    # faces in source-frame pixels and the true count, per face the pass it came from and -- all but tiled -- how many candidates it merged.
    def _merged_buffers(self, n, cap, votes=True):
        """(out, counts, per_face): per_face = ([votes,] src), one int per face slot each"""
        m = max(n * cap, 1)
        return (rf_face * m)(), (C.c_int * max(n, 1))(), tuple((C.c_int * m)() for _ in range(2 if votes else 1))

    def _merged_results(self, out, counts, per_face, n, cap, counts_attr, with_per_face):
        """Per frame the Detections of a merged call (anchor_index -1); with_per_face also each per-face array cut the same way.  The true
        counts go to self.<counts_attr> -- that attribute alone: one family's call leaves the counts of the others as they are."""
        rows = _faces_to_array(out, max(n * cap, 1))
        cut = [slice(i * cap, i * cap + min(counts[i], cap)) for i in range(n)]
        dets = [[_detection(r) for r in rows[s]] for s in cut]
        setattr(self, counts_attr, [int(counts[i]) for i in range(n)])
        return (dets,) + tuple([np.array(a[s], np.int32) for s in cut] for a in per_face) if with_per_face else dets

    def _merged_call(self, fn, head, n, cap, counts_attr, with_per_face, votes=True, tail=()):
        """fn(*head, out, cap, counts, [votes,] src, *tail) with fresh buffers; sets self.truncated.  tail: the extra outputs of the call."""
        out, counts, per_face = self._merged_buffers(n, cap, votes)
        st = _lib.check(fn(*head, out, cap, counts, *per_face, *tail), self._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        return self._merged_results(out, counts, per_face, n, cap, counts_attr, with_per_face)

    def _detect_merged(self, fn, handle, frames, threshold, sp, counts_attr, with_per_face, votes=True, tail=()):
        """The detect call of a merged family: fn(handle, ptrs, rows, cols, steps, n, threshold, spec, ...), frames = those five."""
        head = (handle,) + tuple(frames) + (float(threshold), C.byref(sp))
        return self._merged_call(fn, head, frames[4], sp.max_faces or self.max_detections, counts_attr, with_per_face, votes, tail)

    def _merge_call(self, fn, rows, cols, sp, per_pass_faces, cap_per_image, counts_attr, with_per_face, votes=True, tail=()):
        """The stand-alone merge of a family, over per-pass faces the caller supplies: fn(handle, rows, cols, n, spec, faces, pass_counts,
        ...)"""
        n = len(rows)
        flat, pc = _pack_passes([f for frame in per_pass_faces for f in frame], self.max_detections)
        cap = int(cap_per_image) if cap_per_image is not None else (sp.max_faces or self.max_detections)
        head = (self._h, (C.c_int * max(n, 1))(*rows), (C.c_int * max(n, 1))(*cols), n, C.byref(sp), flat.ctypes.data_as(C.POINTER(rf_face)), pc)
        return self._merged_call(fn, head, n, cap, counts_attr, with_per_face, votes, tail)

    # ------------------------------------------------------------------ tiled detection
    def detect_tiled(self, imgs: Sequence[np.ndarray], threshold: float = 0.5, overlap: int = 0, edge: int = 0, full_frame: bool = True,
                     max_faces: int = 0, return_tiles: bool = False):
        """rf_detect_tiled_batch: frames larger than the net are cut into overlapping net-sized tiles, every tile is detected at 1:1
        (plus the whole frame shrunk, with full_frame), and the faces are merged on the device.  Returns per frame the merged
        detections in SOURCE-FRAME pixels (anchor_index is -1); with return_tiles also, per frame, the pass each came from (tile_plan
        gives the passes).  Keywords as tile_spec()."""
        f = _host_frames(imgs)
        return self._detect_merged(self._lib.rf_detect_tiled_batch, self._h, f.args, threshold, tile_spec(overlap, edge, full_frame, max_faces),
                                   "tiled_counts", return_tiles, votes=False)

    def detect_tiled_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], threshold: float = 0.5,
                            steps: Optional[Sequence[int]] = None, overlap: int = 0, edge: int = 0, full_frame: bool = True,
                            max_faces: int = 0, return_tiles: bool = False):
        """rf_detect_tiled_batch_device: detect_tiled for frames resident in device memory."""
        frames = _device_frames(ptrs, rows, cols, steps) + (len(ptrs),)
        return self._detect_merged(self._lib.rf_detect_tiled_batch_device, self._h, frames, threshold,
                                   tile_spec(overlap, edge, full_frame, max_faces), "tiled_counts", return_tiles, votes=False)

    def tile_merge(self, rows: Sequence[int], cols: Sequence[int], per_pass_faces, overlap: int = 0, edge: int = 0, full_frame: bool = True,
                   max_faces: int = 0, cap_per_image: Optional[int] = None, return_tiles: bool = False):
        """rf_tile_merge_device: edge rule, mapping and merge of per-pass faces the caller supplies -- per_pass_faces[i][t]: the faces
        of pass t of frame i (a (k, 15) array, rows of 15 floats or Detections, at most max_detections), passes as tile_plan gives
        them.  No forward pass runs.  Returns as detect_tiled; self.tiled_counts holds the true merged counts."""
        sp = tile_spec(overlap, edge, full_frame, max_faces)
        return self._merge_call(self._lib.rf_tile_merge_device, rows, cols, sp, per_pass_faces, cap_per_image, "tiled_counts", return_tiles,
                                votes=False)

    def detect_tiled_face_batch_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], threshold: float = 0.5,
                                       steps: Optional[Sequence[int]] = None, overlap: int = 0, edge: int = 0, full_frame: bool = True,
                                       tile_max_faces: int = 0, **kw):
        """rf_detect_tiled_face_batch_device: detect_tiled_device followed on the device by the face batch of the merged faces.
        Keywords as detect_face_batch_device (gate= / return_quality= select the gated launches); returns (detections, tensor,
        matrices, offsets[, quality]) with the detections in source-frame pixels."""
        n = len(ptrs)
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        tsp = tile_spec(overlap, edge, full_frame, tile_max_faces)
        cap = tsp.max_faces or self.max_detections
        out, counts, (src,) = self._merged_buffers(n, cap, votes=False)

        def call(h, spec, d_out, tensor, mats, offsets, gate=None, quality=None):
            return self._lib.rf_detect_tiled_face_batch_device(h, p, r, c, s, n, float(threshold), C.byref(tsp), out, cap, counts, src,
                                                               spec, d_out, tensor, mats, offsets, gate, quality)
        res = self._face_batch_call(call, n, **kw)
        if len(res) == 4:
            res = res[:3] + ([res[3][i, :min(counts[i], res[3].shape[1], cap)] for i in range(n)],)
        return (self._merged_results(out, counts, (src,), n, cap, "tiled_counts", False),) + res

    # ------------------------------------------------------------------ face tracks
    def tracker(self, n_streams: int = 1, motion=None, follow=None, **spec) -> Tracker:
        """rf_tracker_create: a tracker on this handle; keywords as track_spec().  motion: True or motion_spec()'s keywords as a dict
        also gives it motion (Tracker.enable_motion); follow: True or follow_spec()'s keywords as a dict gives it follow
        (Tracker.enable_follow)."""
        return Tracker(self, n_streams, motion=motion, follow=follow, **spec)

    def _run_tracked(self, fn, ptrs, rows, cols, steps, n, threshold, tracker, streams, cap_ended):
        cap = self.max_detections
        out = (rf_face * max(n * cap, 1))()
        counts = (C.c_int * max(n, 1))()
        t, _, tags, ended, ce, ec = tracker._buffers(n, cap, cap_ended)
        st = _lib.check(fn(self._h, ptrs, rows, cols, steps, n, float(threshold), out, cap, counts, t, (C.c_int * max(n, 1))(*streams),
                           tags, ended, ce, ec), self._h)
        self.truncated = tracker.truncated = st == _lib.RF_ERR_TRUNCATED
        self.last_out = _faces_to_array(out, max(n * cap, 1)).reshape(max(n, 1), cap, 15)
        self.last_counts = [int(counts[i]) for i in range(n)]
        return (self._collect(out, counts, n, cap),) + tracker._results(n, counts, cap)

    def detect_tracked(self, imgs: Sequence[np.ndarray], tracker: Tracker, streams: Sequence[int], threshold: float = 0.5,
                       cap_ended: Optional[int] = None):
        """rf_detect_track_batch: detectBatchImages + the frame step of every image (streams[i]: its stream, -1 = not tracked).
        Returns (detections, tags per image, ended tracks per image); tracks live in source-frame pixels."""
        f = _host_frames(imgs)
        return self._run_tracked(self._lib.rf_detect_track_batch, *f.args, threshold, tracker, streams, cap_ended)

    def detect_tracked_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], tracker: Tracker, streams: Sequence[int],
                              threshold: float = 0.5, steps: Optional[Sequence[int]] = None, cap_ended: Optional[int] = None):
        """rf_detect_track_batch_device: detect_tracked for frames resident in device memory (a 0 pointer is a frame with no faces)."""
        n = len(ptrs)
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        return self._run_tracked(self._lib.rf_detect_track_batch_device, p, r, c, s, n, threshold, tracker, streams, cap_ended)

    def detect_track_follow_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], tracker: Tracker, streams: Sequence[int],
                                   threshold: float = 0.5, steps: Optional[Sequence[int]] = None, cap_ended: Optional[int] = None):
        """rf_detect_track_follow_batch_device: a key step -- detect_tracked_device on a tracker with follow, the templates of the matched
        and opened tracks retaken behind the track launch (each stream at most once per call)."""
        n = len(ptrs)
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        return self._run_tracked(self._lib.rf_detect_track_follow_batch_device, p, r, c, s, n, threshold, tracker, streams, cap_ended)

    def detect_followed(self, imgs: Sequence[np.ndarray], tracker: Tracker, streams: Sequence[int], key: bool, threshold: float = 0.5,
                        cap_ended: Optional[int] = None):
        """The key / follow schedule over host frames on a tracker with follow: key=True runs rf_detect_track_follow_batch (detection +
        frame step + templates) and returns (detections, tags, ended); key=False runs rf_track_follow_batch (no forward pass) and
        returns (followed faces per image as (k, 15) float32, tags, ended)."""
        if not key:
            return tracker.follow(imgs, streams, cap_ended=cap_ended)
        n = len(imgs)
        keep = [im if im is None or im.size == 0 or (im.strides[2] == 1 and im.strides[1] == 3) else np.ascontiguousarray(im) for im in imgs]
        views = [_frame_view(im) for im in keep]
        ptrs = (C.c_void_p * max(n, 1))(*[v[0] for v in views])
        rows, cols, steps = ((C.c_int * max(n, 1))(*[v[k] for v in views]) for k in (1, 2, 3))
        res = self._run_tracked(self._lib.rf_detect_track_follow_batch, ptrs, rows, cols, steps, n, threshold, tracker, streams, cap_ended)
        del keep
        return res

    def detect_track_face_batch_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], tracker: Tracker,
                                       streams: Sequence[int], threshold: float = 0.5, steps: Optional[Sequence[int]] = None,
                                       cap_ended: Optional[int] = None, **kw):
        """rf_detect_track_face_batch_device: detect_face_batch_device + the frame steps; with gate= / return_quality= the best shots go
        by sharpness.  Returns (detections, tensor, matrices, offsets[, quality], tags, ended)."""
        n = len(ptrs)
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        cap = self.max_detections
        out = (rf_face * max(n * cap, 1))()
        counts = (C.c_int * max(n, 1))()
        t, _, tags, ended, ce, ec = tracker._buffers(n, cap, cap_ended)
        sv = (C.c_int * max(n, 1))(*streams)

        def call(h, spec, d_out, tensor, mats, offsets, gate=None, quality=None):
            return self._lib.rf_detect_track_face_batch_device(h, p, r, c, s, n, float(threshold), out, cap, counts, spec, d_out, tensor, mats,
                                                               offsets, gate, quality, t, sv, tags, ended, ce, ec)
        res = self._face_batch_call(call, n, **kw)
        tracker.truncated = self.truncated
        if len(res) == 4:
            res = res[:3] + ([res[3][i, :min(counts[i], res[3].shape[1], cap)] for i in range(n)],)
        return (self._collect(out, counts, n, cap),) + res + tracker._results(n, counts, cap)

    # ------------------------------------------------------------------ best-shot gallery
    def _run_shots(self, fn, ptrs, rows, cols, steps, n, threshold, tracker, streams, cap_ended, gate, return_quality, d_shots, host_shots):
        cap = self.max_detections
        out = (rf_face * max(n * cap, 1))()
        counts = (C.c_int * max(n, 1))()
        t, _, tags, ended, ce, ec = tracker._buffers(n, cap, cap_ended)
        shots, info = tracker._shot_buffers(n, cap_ended, host_shots)
        g = _as_gate(gate)
        q = np.zeros((max(n, 1), tracker.shot_max_faces), QUALITY_DTYPE) if return_quality else None
        st = _lib.check(fn(self._h, ptrs, rows, cols, steps, n, float(threshold), out, cap, counts, t, (C.c_int * max(n, 1))(*streams), tags,
                           ended, ce, ec, C.byref(g) if g is not None else None,
                           q.ctypes.data_as(C.POINTER(rf_face_quality)) if q is not None else None, d_shots or None, shots, info), self._h)
        self.truncated = tracker.truncated = st == _lib.RF_ERR_TRUNCATED
        self.last_out = _faces_to_array(out, max(n * cap, 1)).reshape(max(n, 1), cap, 15)
        self.last_counts = [int(counts[i]) for i in range(n)]
        res = (self._collect(out, counts, n, cap),) + tracker._results(n, counts, cap) + tracker._shot_results(n)
        if q is not None:
            res += ([q[i, :min(counts[i], q.shape[1], cap)] for i in range(n)],)
        return res

    def detect_track_shots_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], tracker: Tracker, streams: Sequence[int],
                                  threshold: float = 0.5, steps: Optional[Sequence[int]] = None, cap_ended: Optional[int] = None, gate=None,
                                  return_quality: bool = False, d_shots: int = 0, host_shots: bool = True):
        """rf_detect_track_shots_batch_device: detect_tracked_device on a tracker with a gallery (Tracker.enable_shots); the tracks that
        end hand over their best shots.  Returns (detections, tags, ended, shots, shot records[, quality])."""
        n = len(ptrs)
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        return self._run_shots(self._lib.rf_detect_track_shots_batch_device, p, r, c, s, n, threshold, tracker, streams, cap_ended, gate,
                               return_quality, d_shots, host_shots)

    def detect_track_shots(self, imgs: Sequence[np.ndarray], tracker: Tracker, streams: Sequence[int], threshold: float = 0.5,
                           cap_ended: Optional[int] = None, gate=None, return_quality: bool = False):
        """rf_detect_track_shots_batch: detect_track_shots_device for frames in host memory"""
        f = _host_frames(imgs)
        return self._run_shots(self._lib.rf_detect_track_shots_batch, *f.args, threshold, tracker, streams, cap_ended, gate, return_quality, 0,
                               True)

    # ------------------------------------------------------------------ face redaction
    def _redact_regions(self, sp) -> int:
        return int(sp.max_regions) if sp is not None and sp.max_regions else min(self.max_detections, 1024)

    def redact_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], faces, *, steps: Optional[Sequence[int]] = None,
                      coord_scale: Optional[Sequence[float]] = None, spec=None, tracker: Optional[Tracker] = None,
                      streams: Optional[Sequence[int]] = None, cap_per_image: Optional[int] = None):
        """rf_redact_device: redacts faces the caller supplies in place in device-resident frames; faces[i]: the faces of image i (a
        (k, 15) array, rows or Detections).  spec: redact_spec() or its keywords as a dict.  With a tracker, streams[i] names the stream
        whose coasting tracks are redacted too (-1 = faces only).  Returns (pixels (n, max_regions) int32, region_counts (n,) int32);
        truncated says whether a region list was cut."""
        n = len(ptrs)
        per = [_face_rows(f) for f in faces]
        if len(per) != n:
            raise ValueError("faces must hold one entry per frame")
        cap = int(cap_per_image) if cap_per_image is not None else max([len(r) for r in per] + [1])
        flat = np.zeros((max(n, 1), cap, 15), np.float32)
        counts = (C.c_int * max(n, 1))()
        for i, r in enumerate(per):
            flat[i, :min(len(r), cap)] = r[:cap]
            counts[i] = len(r)
        p, r_, c_, s_ = _device_frames(ptrs, rows, cols, steps)
        cs = (C.c_float * max(n, 1))(*[float(v) for v in coord_scale]) if coord_scale is not None else None
        sp = _as_redact_spec(spec)
        pixels = np.zeros((max(n, 1), self._redact_regions(sp)), np.int32)
        rc = np.zeros(max(n, 1), np.int32)
        sv = (C.c_int * max(n, 1))(*streams) if streams is not None else None
        st = _lib.check(self._lib.rf_redact_device(
            self._h, p, r_, c_, s_, n, flat.ctypes.data_as(C.POINTER(rf_face)), cap, counts, cs, C.byref(sp) if sp is not None else None,
            tracker._t if tracker is not None else None, sv, pixels.ctypes.data_as(C.POINTER(C.c_int32)),
            rc.ctypes.data_as(C.POINTER(C.c_int))), self._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        return pixels[:n], rc[:n]

    def redact_last_launch_ms(self) -> float:
        """rf_redact_last_launch_ms: HIP-event time of the redaction launches of the last redact_device call"""
        ms = C.c_float()
        _lib.check(self._lib.rf_redact_last_launch_ms(self._h, C.byref(ms)), self._h)
        return float(ms.value)

    def detect_redacted_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], threshold: float = 0.5,
                               steps: Optional[Sequence[int]] = None, spec=None) -> List[List[Detection]]:
        """rf_detect_redact_batch_device: detect_device + redaction of what it finds, in place in the device frames.  last_pixels holds
        the pixels every region owns ((n, max_regions) int32)."""
        n = len(ptrs)
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        sp = _as_redact_spec(spec)
        self.last_pixels = np.zeros((max(n, 1), self._redact_regions(sp)), np.int32)
        cap = self.max_detections
        out = (rf_face * max(n * cap, 1))()
        counts = (C.c_int * max(n, 1))()
        st = _lib.check(self._lib.rf_detect_redact_batch_device(self._h, p, r, c, s, n, float(threshold), out, cap, counts,
                                                                C.byref(sp) if sp is not None else None,
                                                                self.last_pixels.ctypes.data_as(C.POINTER(C.c_int32))), self._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        self.last_out = _faces_to_array(out, max(n * cap, 1)).reshape(max(n, 1), cap, 15)
        self.last_counts = [int(counts[i]) for i in range(n)]
        return self._collect(out, counts, n, cap)

    def detect_redacted(self, imgs: Sequence[np.ndarray], threshold: float = 0.5, spec=None) -> List[List[Detection]]:
        """rf_detect_redact_batch: detectBatchImages + redaction; the frames (uint8 H x W x 3, dense pixels, any row stride, writeable)
        are redacted in place."""
        f = _host_frames(imgs, in_place="redacted")
        ptrs, rows, cols, steps, n = f.args
        sp = _as_redact_spec(spec)
        self.last_pixels = np.zeros((max(n, 1), self._redact_regions(sp)), np.int32)
        cap = self.max_detections
        out = (rf_face * max(n * cap, 1))()
        counts = (C.c_int * max(n, 1))()
        st = _lib.check(self._lib.rf_detect_redact_batch(self._h, ptrs, rows, cols, steps, n, float(threshold), out, cap, counts,
                                                         C.byref(sp) if sp is not None else None, ptrs, steps,
                                                         self.last_pixels.ctypes.data_as(C.POINTER(C.c_int32))), self._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        return self._collect(out, counts, n, cap)

    # ------------------------------------------------------------------ overlays
    def overlay_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], faces, *, ids=None,
                       steps: Optional[Sequence[int]] = None, coord_scale: Optional[Sequence[float]] = None, spec=None,
                       tracker: Optional[Tracker] = None, streams: Optional[Sequence[int]] = None, cap_per_image: Optional[int] = None):
        """rf_overlay_device: draws the boxes, landmark discs and labels of faces the caller supplies in place into device-resident
        frames; faces[i]: the faces of image i (a (k, 15) array, rows or Detections), ids[i]: their track ids (or ids = None).  spec:
        overlay_spec() or its keywords as a dict.  With a tracker, streams[i] names the stream whose coasting tracks are drawn dashed
        (-1 = faces only).  Returns (pixels (n, max_regions) int32, region_counts (n,) int32); truncated says whether a list was cut."""
        n = len(ptrs)
        per = [_face_rows(f) for f in faces]
        if len(per) != n or (ids is not None and len(ids) != n):
            raise ValueError("faces (and ids) must hold one entry per frame")
        cap = int(cap_per_image) if cap_per_image is not None else max([len(r) for r in per] + [1])
        flat = np.zeros((max(n, 1), cap, 15), np.float32)
        counts = (C.c_int * max(n, 1))()
        for i, r in enumerate(per):
            flat[i, :min(len(r), cap)] = r[:cap]
            counts[i] = len(r)
        idb = _id_block(ids, n, cap)
        p, r_, c_, s_ = _device_frames(ptrs, rows, cols, steps)
        cs = (C.c_float * max(n, 1))(*[float(v) for v in coord_scale]) if coord_scale is not None else None
        sp = _as_overlay_spec(spec)
        pixels = np.zeros((max(n, 1), self._redact_regions(sp)), np.int32)
        rc = np.zeros(max(n, 1), np.int32)
        sv = (C.c_int * max(n, 1))(*streams) if streams is not None else None
        st = _lib.check(self._lib.rf_overlay_device(
            self._h, p, r_, c_, s_, n, flat.ctypes.data_as(C.POINTER(rf_face)),
            idb.ctypes.data_as(C.POINTER(C.c_int64)) if idb is not None else None, cap, counts, cs, C.byref(sp) if sp is not None else None,
            tracker._t if tracker is not None else None, sv, pixels.ctypes.data_as(C.POINTER(C.c_int32)),
            rc.ctypes.data_as(C.POINTER(C.c_int))), self._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        return pixels[:n], rc[:n]

    def overlay_last_launch_ms(self) -> float:
        """rf_overlay_last_launch_ms: HIP-event time of the two overlay launches of the last overlay_device call"""
        ms = C.c_float()
        _lib.check(self._lib.rf_overlay_last_launch_ms(self._h, C.byref(ms)), self._h)
        return float(ms.value)

    def detect_overlay_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], threshold: float = 0.5,
                              steps: Optional[Sequence[int]] = None, spec=None) -> List[List[Detection]]:
        """rf_detect_overlay_batch_device: detect_device + the overlay of what it finds, in place in the device frames.  last_pixels
        holds the pixels every region painted ((n, max_regions) int32)."""
        n = len(ptrs)
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        sp = _as_overlay_spec(spec)
        self.last_pixels = np.zeros((max(n, 1), self._redact_regions(sp)), np.int32)
        cap = self.max_detections
        out = (rf_face * max(n * cap, 1))()
        counts = (C.c_int * max(n, 1))()
        st = _lib.check(self._lib.rf_detect_overlay_batch_device(self._h, p, r, c, s, n, float(threshold), out, cap, counts,
                                                                 C.byref(sp) if sp is not None else None,
                                                                 self.last_pixels.ctypes.data_as(C.POINTER(C.c_int32))), self._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        self.last_out = _faces_to_array(out, max(n * cap, 1)).reshape(max(n, 1), cap, 15)
        self.last_counts = [int(counts[i]) for i in range(n)]
        return self._collect(out, counts, n, cap)

    def detect_overlay(self, imgs: Sequence[np.ndarray], threshold: float = 0.5, spec=None) -> List[List[Detection]]:
        """rf_detect_overlay_batch: detectBatchImages + the overlay; the frames (uint8 H x W x 3, dense pixels, any row stride,
        writeable) are drawn into in place."""
        f = _host_frames(imgs, in_place="drawn into")
        ptrs, rows, cols, steps, n = f.args
        sp = _as_overlay_spec(spec)
        self.last_pixels = np.zeros((max(n, 1), self._redact_regions(sp)), np.int32)
        cap = self.max_detections
        out = (rf_face * max(n * cap, 1))()
        counts = (C.c_int * max(n, 1))()
        st = _lib.check(self._lib.rf_detect_overlay_batch(self._h, ptrs, rows, cols, steps, n, float(threshold), out, cap, counts,
                                                          C.byref(sp) if sp is not None else None, ptrs, steps,
                                                          self.last_pixels.ctypes.data_as(C.POINTER(C.c_int32))), self._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        self.last_out = _faces_to_array(out, max(n * cap, 1)).reshape(max(n, 1), cap, 15)
        self.last_counts = [int(counts[i]) for i in range(n)]
        return self._collect(out, counts, n, cap)

    # ------------------------------------------------------------------ flip test-time augmentation
    def detect_tta(self, imgs: Sequence[np.ndarray], threshold: float = 0.5, flip: bool = True, vote: bool = True, max_faces: int = 0,
                   return_votes: bool = False):
        """rf_detect_tta_batch: every frame is detected as it is and mirrored left-right; the mirrored faces are moved back and
        overlapping boxes of both passes are merged on the device into a score-weighted mean.  Returns per frame the merged
        detections in SOURCE-FRAME pixels (anchor_index is -1); with return_votes also, per frame, how many candidates each face
        merged and the pass (0: the frame, 1: mirrored) its head came from.  self.tta_counts holds the true merged counts."""
        f = _host_frames(imgs)
        return self._detect_merged(self._lib.rf_detect_tta_batch, self._h, f.args, threshold, tta_spec(flip, vote, max_faces), "tta_counts",
                                   return_votes)

    def detect_tta_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], threshold: float = 0.5,
                          steps: Optional[Sequence[int]] = None, flip: bool = True, vote: bool = True, max_faces: int = 0,
                          return_votes: bool = False):
        """rf_detect_tta_batch_device: detect_tta for frames resident in device memory (0 / None: an empty frame)."""
        frames = _device_frames(ptrs, rows, cols, steps) + (len(ptrs),)
        return self._detect_merged(self._lib.rf_detect_tta_batch_device, self._h, frames, threshold, tta_spec(flip, vote, max_faces),
                                   "tta_counts", return_votes)

    def tta_merge(self, rows: Sequence[int], cols: Sequence[int], per_pass_faces, flip: bool = True, vote: bool = True, max_faces: int = 0,
                  cap_per_image: Optional[int] = None, return_votes: bool = False):
        """rf_tta_merge_device: mapping and merge of per-pass faces the caller supplies -- per_pass_faces[i][p]: the faces of pass p
        of frame i (a (k, 15) array, rows of 15 floats or Detections, at most max_detections); two passes per frame, one with flip
        off.  No forward pass runs.  Returns as detect_tta; self.tta_counts holds the true merged counts."""
        n = len(rows)
        sp = tta_spec(flip, vote, max_faces)
        per = 2 if flip else 1
        if any(len(frame) != per for frame in per_pass_faces) or len(per_pass_faces) != n:
            raise ValueError("per_pass_faces: one list of %d passes per frame" % per)
        return self._merge_call(self._lib.rf_tta_merge_device, rows, cols, sp, per_pass_faces, cap_per_image, "tta_counts", return_votes)

    def mirror_device(self, src_ptr: int, rows: int, cols: int, dst_ptr: int, step: Optional[int] = None, dst_step: Optional[int] = None):
        """rf_mirror_device: the mirror kernel on its own -- row y of the destination (dst_step bytes apart, cols * 3 bytes written)
        is row y of the BGR frame at src_ptr (row pitch `step`, any alignment) mirrored left-right.  Both in device memory."""
        _lib.check(self._lib.rf_mirror_device(self._h, src_ptr, int(rows), int(cols), int(step if step is not None else 3 * cols), dst_ptr,
                                              int(dst_step if dst_step is not None else 3 * cols)), self._h)

    # ------------------------------------------------------------------ rotation-robust detection
    def detect_rotated(self, imgs: Sequence[np.ndarray], threshold: float = 0.5, rots: int = 0, vote: bool = False, max_faces: int = 0,
                       return_votes: bool = False):
        """rf_detect_rot_batch: every frame is detected as it is and turned by one, two and three quarter turns counter-clockwise
        (rots: a bit mask of the turns to run, 0 = all four; the copies are made on the device); the faces of all passes are moved
        back and merged on the device.  Returns per frame the merged detections in SOURCE-FRAME pixels (anchor_index is -1); with
        return_votes also, per frame, how many candidates each face merged and the rotation (0..3) its head came from.
        self.rot_counts holds the true merged counts, self.frame_rot per frame the quarter turns counter-clockwise that make it
        upright (-1: no face), self.rot_score the (n, 4) score sums behind that."""
        f = _host_frames(imgs)
        return self._rot_call(len(imgs), lambda tail: self._detect_merged(self._lib.rf_detect_rot_batch, self._h, f.args, threshold,
                                                                          rot_spec(rots, vote, max_faces), "rot_counts", return_votes, tail=tail))

    def detect_rotated_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], threshold: float = 0.5,
                              steps: Optional[Sequence[int]] = None, rots: int = 0, vote: bool = False, max_faces: int = 0,
                              return_votes: bool = False):
        """rf_detect_rot_batch_device: detect_rotated for frames resident in device memory (0 / None: an empty frame)."""
        frames = _device_frames(ptrs, rows, cols, steps) + (len(ptrs),)
        return self._rot_call(len(ptrs), lambda tail: self._detect_merged(self._lib.rf_detect_rot_batch_device, self._h, frames, threshold,
                                                                          rot_spec(rots, vote, max_faces), "rot_counts", return_votes, tail=tail))

    def _rot_call(self, n, call):
        """A rotation call with its two extra outputs: call((frame_rot, rot_score)) makes the C call; sets self.frame_rot / self.rot_score."""
        frame_rot, score = (C.c_int * max(n, 1))(), (C.c_float * max(4 * n, 1))()
        res = call((frame_rot, score))
        self.frame_rot = [int(frame_rot[i]) for i in range(n)]
        self.rot_score = np.array(score[:4 * n], np.float32).reshape(n, 4)
        return res

    def rot_merge(self, rows: Sequence[int], cols: Sequence[int], per_pass_faces, rots: int = 0, vote: bool = False, max_faces: int = 0,
                  cap_per_image: Optional[int] = None, return_votes: bool = False):
        """rf_rot_merge_device: mapping and merge of per-pass faces the caller supplies -- per_pass_faces[i][p]: the faces of the p-th
        rotation of `rots` (ascending k) of frame i (a (j, 15) array, rows of 15 floats or Detections, at most max_detections).  No
        forward pass runs.  Returns as detect_rotated; self.rot_counts, self.frame_rot and self.rot_score as there."""
        n = len(rows)
        sp = rot_spec(rots, vote, max_faces)
        per = len(_rot_list(rots)) if 0 <= int(rots) <= 15 else 4
        if any(len(frame) != per for frame in per_pass_faces) or len(per_pass_faces) != n:
            raise ValueError("per_pass_faces: one list of %d passes per frame" % per)
        return self._rot_call(n, lambda tail: self._merge_call(self._lib.rf_rot_merge_device, rows, cols, sp, per_pass_faces, cap_per_image,
                                                               "rot_counts", return_votes, tail=tail))

    def rotate_device(self, src_ptr: int, rows: int, cols: int, k: int, dst_ptr: int, step: Optional[int] = None,
                      dst_step: Optional[int] = None):
        """rf_rotate_device: the rotate kernel on its own -- the destination (rows dst_step bytes apart, cols_k * 3 bytes written) is
        the BGR frame at src_ptr (row pitch `step`, any alignment) turned by k quarter turns counter-clockwise.  Both in device memory."""
        dc = rows if int(k) & 1 else cols
        _lib.check(self._lib.rf_rotate_device(self._h, src_ptr, int(rows), int(cols), int(step if step is not None else 3 * cols), int(k),
                                              dst_ptr, int(dst_step if dst_step is not None else 3 * dc)), self._h)

    # ------------------------------------------------------------------ change regions
    def changer(self, rows: int, cols: int, n_streams: int = 1, **spec) -> Changer:
        """rf_changer_create: change regions for frames of rows x cols on this detector (see Changer; keywords as change_spec())."""
        return Changer(self, rows, cols, n_streams, **spec)

    # ------------------------------------------------------------------ fisheye detection
    def dewarper(self, rows: int, cols: int, spec=None, mesh=None, view_w: int = 0, view_h: int = 0) -> Dewarper:
        """rf_dewarper_create: a camera's views on this detector (see Dewarper)."""
        return Dewarper(self, rows, cols, spec, mesh, view_w, view_h)

    def detect_dewarped(self, imgs: Sequence[np.ndarray], dewarper: Dewarper, threshold: float = 0.5, vote: bool = False,
                        max_faces: int = 0, edge: int = 0, return_votes: bool = False):
        """rf_detect_dewarp_batch: every frame (of the dewarper's shape; None: an empty frame) is detected in the dewarper's views, made
        on the device; the faces of all views are moved back through the meshes and merged on the device.  Returns per frame the
        merged detections in SOURCE-FRAME pixels (anchor_index is -1); with return_votes also, per frame, how many candidates each
        face merged and the view its head came from.  self.dewarp_counts holds the true merged counts."""
        f = _host_frames(imgs)
        return self._detect_merged(self._lib.rf_detect_dewarp_batch, dewarper._d, f.args, threshold,
                                   dewarp_spec(vote=vote, max_faces=max_faces, edge=edge), "dewarp_counts", return_votes)

    def detect_dewarped_device(self, ptrs: Sequence[int], dewarper: Dewarper, threshold: float = 0.5, steps: Optional[Sequence[int]] = None,
                               rows: Optional[Sequence[int]] = None, cols: Optional[Sequence[int]] = None, vote: bool = False,
                               max_faces: int = 0, edge: int = 0, views_ptr: Optional[int] = None, return_votes: bool = False):
        """rf_detect_dewarp_batch_device: detect_dewarped for frames resident in device memory (0 / None: an empty frame).  views_ptr:
        device memory of n * V * view_h * view_w * 3 bytes that receives the views as dense frames."""
        rows = rows if rows is not None else [dewarper.rows if q else 0 for q in ptrs]
        cols = cols if cols is not None else [dewarper.cols if q else 0 for q in ptrs]
        frames = _device_frames(ptrs, rows, cols, steps) + (len(ptrs),)
        return self._detect_merged(self._lib.rf_detect_dewarp_batch_device, dewarper._d, frames, threshold,
                                   dewarp_spec(vote=vote, max_faces=max_faces, edge=edge), "dewarp_counts", return_votes, tail=(views_ptr,))

    def dewarp_merge(self, dewarper: Dewarper, per_view_faces, vote: bool = False, max_faces: int = 0, edge: int = 0,
                     cap_per_image: Optional[int] = None, return_votes: bool = False):
        """rf_dewarp_merge_device: edge rule, mapping and merge of per-view faces the caller supplies -- per_view_faces[i][v]: the faces
        of view v of frame i (a (j, 15) array, rows of 15 floats or Detections, at most max_detections).  No forward pass runs.
        Returns as detect_dewarped; self.dewarp_counts as there."""
        n = len(per_view_faces)
        sp = dewarp_spec(vote=vote, max_faces=max_faces, edge=edge)
        if any(len(frame) != dewarper.views for frame in per_view_faces):
            raise ValueError("per_view_faces: one list of %d views per frame" % dewarper.views)
        flat, pc = _pack_passes([f for frame in per_view_faces for f in frame], self.max_detections)
        cap = int(cap_per_image) if cap_per_image is not None else (sp.max_faces or self.max_detections)
        head = (dewarper._d, n, C.byref(sp), flat.ctypes.data_as(C.POINTER(rf_face)), pc)        # (a dewarper knows its frames' shape)
        return self._merged_call(self._lib.rf_dewarp_merge_device, head, n, cap, "dewarp_counts", return_votes)

    def dewarp_device(self, dewarper: Dewarper, view: int, src_ptr: int, dst_ptr: int, step: Optional[int] = None,
                      dst_step: Optional[int] = None):
        """rf_dewarp_device: the dewarp kernel on its own -- view `view` of the BGR frame at src_ptr (the dewarper's shape, row pitch
        `step`, any alignment) into the destination (rows dst_step bytes apart, view_w * 3 bytes written).  Both in device memory."""
        _lib.check(self._lib.rf_dewarp_device(dewarper._d, int(view), src_ptr, int(step if step is not None else 3 * dewarper.cols), dst_ptr,
                                              int(dst_step if dst_step is not None else 3 * dewarper.view_w)), self._h)

    # ------------------------------------------------------------------ region detection
    def detect_rois(self, imgs: Sequence[np.ndarray], rois, threshold: float = 0.5, grid: int = 0, max_zoom: int = 0, vote: bool = False,
                    max_faces: int = 0, return_src_roi: bool = False):
        """rf_detect_roi_batch: every frame (None: an empty frame) is detected only in its regions -- rois[i]: frame i's (x, y, w, h)
        list, at most 256 -- which are packed grid x grid to a net-sized view on the device, each at the largest power-of-two step
        (x max_zoom .. x1/4) at which it fits its cell; the faces are moved back and merged on the device.  Returns per frame the
        merged detections in SOURCE-FRAME pixels (anchor_index is -1); with return_src_roi also, per frame, how many candidates each
        face merged and the region it came from.  self.roi_counts holds the true merged counts."""
        f = _host_frames(imgs)
        arr, rc, _ = _roi_lists(rois)
        if len(rois) != len(imgs):
            raise ValueError("rois: one list of regions per frame")
        sp = roi_spec(grid, max_zoom, vote, max_faces)
        head = (self._h,) + tuple(f.args) + (arr, rc, float(threshold), C.byref(sp))
        return self._merged_call(self._lib.rf_detect_roi_batch, head, f.args[4], sp.max_faces or self.max_detections, "roi_counts", return_src_roi)

    def detect_rois_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], rois, threshold: float = 0.5,
                           steps: Optional[Sequence[int]] = None, grid: int = 0, max_zoom: int = 0, vote: bool = False, max_faces: int = 0,
                           views_ptr: Optional[int] = None, return_src_roi: bool = False):
        """rf_detect_roi_batch_device: detect_rois for frames resident in device memory (0 / None: an empty frame).  views_ptr: device
        memory of passes * net_h * net_w * 3 bytes that receives the views as dense frames."""
        if len(rois) != len(ptrs):
            raise ValueError("rois: one list of regions per frame")
        arr, rc, _ = _roi_lists(rois)
        sp = roi_spec(grid, max_zoom, vote, max_faces)
        head = (self._h,) + _device_frames(ptrs, rows, cols, steps) + (len(ptrs), arr, rc, float(threshold), C.byref(sp))
        return self._merged_call(self._lib.rf_detect_roi_batch_device, head, len(ptrs), sp.max_faces or self.max_detections, "roi_counts",
                                 return_src_roi, tail=(views_ptr,))

    def roi_merge(self, rows: Sequence[int], cols: Sequence[int], rois, per_pass_faces, grid: int = 0, max_zoom: int = 0, vote: bool = False,
                  max_faces: int = 0, cap_per_image: Optional[int] = None, return_src_roi: bool = False):
        """rf_roi_merge_device: face rule and merge of per-pass faces the caller supplies -- per_pass_faces[i][p]: the faces of pass p
        of frame i (a (j, 15) array, rows of 15 floats or Detections, at most max_detections), ceil(len(rois[i]) / grid^2) passes.
        No forward pass runs.  Returns as detect_rois; self.roi_counts as there."""
        n = len(rows)
        sp = roi_spec(grid, max_zoom, vote, max_faces)
        arr, rc, counts = _roi_lists(rois)
        gg = (sp.grid or 4) ** 2
        if len(rois) != n or len(per_pass_faces) != n or any(len(f) != -(-c // gg) for f, c in zip(per_pass_faces, counts)):
            raise ValueError("per_pass_faces: one list of ceil(regions / grid^2) passes per frame")
        flat, pc = _pack_passes([f for frame in per_pass_faces for f in frame], self.max_detections)
        cap = int(cap_per_image) if cap_per_image is not None else (sp.max_faces or self.max_detections)
        head = (self._h, (C.c_int * max(n, 1))(*rows), (C.c_int * max(n, 1))(*cols), n, arr, rc, C.byref(sp), flat.ctypes.data_as(C.POINTER(rf_face)), pc)
        return self._merged_call(self._lib.rf_roi_merge_device, head, n, cap, "roi_counts", return_src_roi)

    def roi_atlas_device(self, src_ptr: int, rows: int, cols: int, rois, dst_ptr: int, view_w: int, view_h: int, step: Optional[int] = None,
                         dst_step: Optional[int] = None, grid: int = 0, max_zoom: int = 0):
        """rf_roi_atlas_device: the atlas kernel on its own -- all passes of the regions of the BGR frame at src_ptr (row pitch `step`,
        any alignment) into the destination: pass p's row y at dst_ptr + (p * view_h + y) * dst_step, view_w * 3 bytes written.  Both
        in device memory."""
        arr, n = _roi_array(rois)
        _lib.check(self._lib.rf_roi_atlas_device(self._h, src_ptr, int(rows), int(cols), int(step if step is not None else 3 * cols), arr, n,
                                                 C.byref(roi_spec(grid, max_zoom)), int(view_w), int(view_h), dst_ptr,
                                                 int(dst_step if dst_step is not None else 3 * view_w)), self._h)

    # ------------------------------------------------------------------ low-light detection
    def detect_enhanced(self, imgs: Sequence[np.ndarray], threshold: float = 0.5, tile: int = 0, clip: int = 0, dark_below: int = 0,
                        enhanced_ptrs: Optional[Sequence[int]] = None, enhanced_steps: Optional[Sequence[int]] = None):
        """rf_detect_enhanced_batch: every frame is uploaded, enhanced on the device (enhance_host's arithmetic: the dark tiles get a
        contrast boost, lit tiles stay as they are) and detected, with no host wait in between.  Returns what detect() returns for the
        enhanced frames.  enhanced_ptrs: device buffers that receive the enhanced copies (row pitch enhanced_steps, default cols * 3).
        self.tiles_enhanced holds, per frame, the number of tiles the enhancement touched."""
        f = _host_frames(imgs)
        return self._run_enhanced(self._lib.rf_detect_enhanced_batch, *f.args, threshold, enhance_spec(tile, clip, dark_below), enhanced_ptrs,
                                  enhanced_steps)

    def detect_enhanced_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], threshold: float = 0.5,
                               steps: Optional[Sequence[int]] = None, tile: int = 0, clip: int = 0, dark_below: int = 0,
                               enhanced_ptrs: Optional[Sequence[int]] = None, enhanced_steps: Optional[Sequence[int]] = None):
        """rf_detect_enhanced_batch_device: detect_enhanced for frames resident in device memory (0 / None: an empty frame).  The
        frames are not written."""
        n = len(ptrs)
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        return self._run_enhanced(self._lib.rf_detect_enhanced_batch_device, p, r, c, s, n, threshold, enhance_spec(tile, clip, dark_below),
                                  enhanced_ptrs, enhanced_steps)

    def _run_enhanced(self, fn, ptrs, rows, cols, steps, n, threshold, sp, enhanced_ptrs, enhanced_steps):
        cap = self.max_detections
        out = (rf_face * max(n * cap, 1))()
        counts, tiles = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))()
        d_enh = (C.c_void_p * max(n, 1))(*enhanced_ptrs) if enhanced_ptrs is not None else None
        e_steps = (C.c_int * max(n, 1))(*enhanced_steps) if enhanced_steps is not None else None
        st = _lib.check(fn(self._h, ptrs, rows, cols, steps, n, float(threshold), C.byref(sp), out, cap, counts, d_enh, e_steps, tiles),
                        self._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        self.tiles_enhanced = [int(tiles[i]) for i in range(n)]
        return self._collect(out, counts, n, cap)

    def enhance_device(self, src_ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], dst_ptrs: Sequence[int],
                       steps: Optional[Sequence[int]] = None, dst_steps: Optional[Sequence[int]] = None, tile: int = 0, clip: int = 0,
                       dark_below: int = 0, spec=None) -> List[int]:
        """rf_enhance_device: the two enhance kernels on their own -- destination i (rows dst_steps[i] bytes apart, cols * 3 bytes
        written) is the enhancement of the BGR frame at src_ptrs[i] (row pitch steps[i], any alignment).  Both in device memory; a
        destination may be its source exactly (same pointer and pitch).  Returns the number of tiles enhanced per frame."""
        n = len(src_ptrs)
        sp = spec if spec is not None else enhance_spec(tile, clip, dark_below)
        p, r, c, s = _device_frames(src_ptrs, rows, cols, steps)
        d, _, _, ds = _device_frames(dst_ptrs, rows, cols, dst_steps)
        tiles = (C.c_int * max(n, 1))()
        _lib.check(self._lib.rf_enhance_device(self._h, C.byref(sp), p, r, c, s, n, d, ds, tiles), self._h)
        return [int(tiles[i]) for i in range(n)]

    # ------------------------------------------------------------------ zoom-pyramid detection
    def detect_pyramid(self, imgs: Sequence[np.ndarray], threshold: float = 0.5, levels: int = 0, overlap: int = 0, edge: int = 0,
                       full_frame: bool = True, max_faces: int = 0, vote: bool = True, return_votes: bool = False):
        """rf_detect_pyramid_batch: every frame is detected at 1x (its tile plan) and as net-sized tiles of the frame enlarged 2x / 4x
        on the device (levels: bit 0 1x, bit 1 2x, bit 2 4x; 0 = 1x and 2x), so that faces below the smallest anchor are found; the
        faces of all passes are moved back and merged as in detect_tta.  Returns per frame the merged detections in SOURCE-FRAME
        pixels (anchor_index is -1); with return_votes also, per frame, how many candidates each face merged and the pass of the
        plan (pyramid_plan) its head came from.  self.pyramid_counts holds the true merged counts."""
        f = _host_frames(imgs)
        return self._detect_merged(self._lib.rf_detect_pyramid_batch, self._h, f.args, threshold,
                                   pyramid_spec(levels, overlap, edge, full_frame, max_faces, vote), "pyramid_counts", return_votes)

    def detect_pyramid_device(self, ptrs: Sequence[int], rows: Sequence[int], cols: Sequence[int], threshold: float = 0.5,
                              steps: Optional[Sequence[int]] = None, levels: int = 0, overlap: int = 0, edge: int = 0,
                              full_frame: bool = True, max_faces: int = 0, vote: bool = True, return_votes: bool = False):
        """rf_detect_pyramid_batch_device: detect_pyramid for frames resident in device memory (0 / None: an empty frame)."""
        frames = _device_frames(ptrs, rows, cols, steps) + (len(ptrs),)
        return self._detect_merged(self._lib.rf_detect_pyramid_batch_device, self._h, frames, threshold,
                                   pyramid_spec(levels, overlap, edge, full_frame, max_faces, vote), "pyramid_counts", return_votes)

    def pyramid_merge(self, rows: Sequence[int], cols: Sequence[int], per_pass_faces, levels: int = 0, overlap: int = 0, edge: int = 0,
                      full_frame: bool = True, max_faces: int = 0, vote: bool = True, cap_per_image: Optional[int] = None,
                      return_votes: bool = False):
        """rf_pyramid_merge_device: edge rule, mapping and merge of per-pass faces the caller supplies -- per_pass_faces[i][p]: the
        faces of pass p of frame i's pyramid plan (a (k, 15) array, rows of 15 floats or Detections, at most max_detections).  No
        forward pass runs.  Returns as detect_pyramid; self.pyramid_counts holds the true merged counts."""
        n = len(rows)
        sp = pyramid_spec(levels, overlap, edge, full_frame, max_faces, vote)
        if len(per_pass_faces) != n:
            raise ValueError("per_pass_faces: one list of passes per frame")
        for i in range(n):
            want = 1 if rows[i] <= 0 or cols[i] <= 0 else self._lib.rf_pyramid_plan(C.byref(sp), int(rows[i]), int(cols[i]), self.net_h,
                                                                                    self.net_w, None, 0)
            if want >= 0 and len(per_pass_faces[i]) != want:
                raise ValueError("per_pass_faces[%d]: %d passes, the plan has %d" % (i, len(per_pass_faces[i]), want))
        return self._merge_call(self._lib.rf_pyramid_merge_device, rows, cols, sp, per_pass_faces, cap_per_image, "pyramid_counts",
                                return_votes)

    def zoom_device(self, src_ptr: int, rows: int, cols: int, z: int, x0: int, y0: int, tw: int, th: int, dst_ptr: int,
                    step: Optional[int] = None, dst_step: Optional[int] = None):
        """rf_zoom_device: the zoom kernel on its own -- the window [x0, x0 + tw) x [y0, y0 + th) of the BGR frame at src_ptr (row
        pitch `step`, any alignment) enlarged z (2 or 4) times, written as tw * 3 bytes per row, dst_step bytes apart.  Both in
        device memory."""
        _lib.check(self._lib.rf_zoom_device(self._h, src_ptr, int(rows), int(cols), int(step if step is not None else 3 * cols), int(z),
                                            int(x0), int(y0), int(tw), int(th), dst_ptr,
                                            int(dst_step if dst_step is not None else 3 * tw)), self._h)

    def enqueue_device(self, ptrs, rows, cols, threshold: float = 0.5, steps: Optional[Sequence[int]] = None) -> int:
        n = len(ptrs)
        p, r, c, s = _device_frames(ptrs, rows, cols, steps)
        t = C.c_int()
        _lib.check(self._lib.rf_enqueue_batch_device(self._h, p, r, c, s, n, float(threshold), C.byref(t)), self._h)
        return t.value

    def enqueue_host(self, imgs: Sequence[np.ndarray], threshold: float = 0.5) -> int:
        """rf_enqueue_batch: frames in host memory (numpy, OpenCV layout); they are staged before this returns."""
        return self.enqueue_prepared_host(self.prepare_host_batch(imgs), threshold)

    def prepare_host_batch(self, imgs: Sequence[np.ndarray]):
        """C argument arrays of rf_enqueue_batch for host frames that are submitted repeatedly (what a C caller keeps)."""
        n = len(imgs)
        keep = [np.ascontiguousarray(im) if (im.strides[2] != 1 or im.strides[1] != 3) else im for im in imgs]
        return ((C.c_void_p * n)(*[im.ctypes.data for im in keep]), (C.c_int * n)(*[im.shape[0] for im in keep]),
                (C.c_int * n)(*[im.shape[1] for im in keep]), (C.c_int * n)(*[im.strides[0] for im in keep]), n, C.c_int(), keep)

    def enqueue_prepared_host(self, batch, threshold: float = 0.5) -> int:
        p, r, c, s, n, t, _keep = batch
        _lib.check(self._lib.rf_enqueue_batch(self._h, p, r, c, s, n, threshold, C.byref(t)), self._h)
        return t.value

    def host_register(self, arr: np.ndarray) -> None:
        """Pin a caller-owned buffer (rf_host_register): frames inside it are DMA'd in place, without the staging copy."""
        _lib.check(self._lib.rf_host_register(self._h, arr.ctypes.data, arr.nbytes), self._h)

    def host_unregister(self, arr: np.ndarray) -> None:
        _lib.check(self._lib.rf_host_unregister(self._h, arr.ctypes.data), self._h)

    def invalidate_residency(self) -> None:
        """Forget where device frame pointers live (call after freeing / re-allocating frame buffers; rf_invalidate_residency)."""
        _lib.check(self._lib.rf_invalidate_residency(self._h), self._h)

    def num_devices(self) -> int:
        return self._lib.rf_num_devices(self._h)

    def scatter_stats(self) -> dict:
        """rf_scatter_stats: device frames pulled from other GPUs since the handle was built, and the peer copies that carried them."""
        f, c = C.c_longlong(), C.c_longlong()
        _lib.check(self._lib.rf_scatter_stats(self._h, C.byref(f), C.byref(c)), self._h)
        return {"frames": f.value, "peer_copies": c.value}

    def launch_stats(self) -> dict:
        """rf_launch_stats: super-batches launched since the handle was built, and the images in them."""
        l, i = C.c_longlong(), C.c_longlong()
        _lib.check(self._lib.rf_launch_stats(self._h, C.byref(l), C.byref(i)), self._h)
        return {"launches": l.value, "images": i.value}

    def prepare_device_batch(self, ptrs, rows, cols, steps=None):
        """Build the C argument arrays of rf_enqueue_batch_device once for a batch of device frames that is submitted
        repeatedly (a ring of camera buffers): what a C/C++ caller keeps on its side anyway.  Returns an opaque batch."""
        return _device_frames(ptrs, rows, cols, steps) + (len(ptrs), C.c_int())

    def enqueue_prepared(self, batch, threshold: float = 0.5) -> int:
        p, r, c, s, n, t = batch
        _lib.check(self._lib.rf_enqueue_batch_device(self._h, p, r, c, s, n, threshold, C.byref(t)), self._h)
        return t.value

    def wait(self, ticket: int, n: int) -> List[List[Detection]]:
        cap = self.max_detections
        out = (rf_face * (n * cap))()
        counts = (C.c_int * n)()
        st = _lib.check(self._lib.rf_wait(self._h, ticket, out, cap, counts), self._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        return self._collect(out, counts, n, cap)

    def wait_counts(self, ticket: int, n: int) -> List[int]:
        """rf_wait without materialising Python objects (benchmark loop)."""
        if not hasattr(self, "_wc_buf") or len(self._wc_buf[1]) < n:
            self._wc_buf = ((rf_face * (self.max_batch * self.max_detections))(), (C.c_int * self.max_batch)())
        out, counts = self._wc_buf
        st = _lib.check(self._lib.rf_wait(self._h, ticket, out, self.max_detections, counts), self._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        return list(counts[:n])

    def last_wait_faces(self) -> np.ndarray:
        """The result block the most recent wait_counts() filled, as a (max_batch, max_detections, 15) float view (no copy)."""
        return np.ctypeslib.as_array(C.cast(self._wc_buf[0], C.POINTER(C.c_float)),
                                     shape=(self.max_batch, self.max_detections, 15))

    def num_slots(self) -> int:
        return self._lib.rf_num_slots(self._h)

    # ------------------------------------------------------------------ inspection
    def last_timings(self):
        a, b, c, d = C.c_float(), C.c_float(), C.c_float(), C.c_float()
        self._lib.rf_last_timings(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        return {"pre_ms": a.value, "infer_ms": b.value, "post_ms": c.value, "total_ms": d.value}

    def last_candidate_counts(self, n: int) -> List[int]:
        buf = (C.c_int * n)()
        _lib.check(self._lib.rf_last_candidate_counts(self._h, buf, n), self._h)
        return list(buf)

    def get_output(self, blob: str, image: int = 0) -> np.ndarray:
        """blob_by_name(name)->result[image] (trtretinafacenet.cpp:104-114) as a (C, H, W) fp32 array."""
        need = self._lib.rf_get_output(self._h, blob.encode(), image, None, 0)
        if need < 0:
            _lib.check(int(need), self._h)
        arr = np.empty(need, dtype=np.float32)
        got = self._lib.rf_get_output(self._h, blob.encode(), image, arr.ctypes.data_as(C.POINTER(C.c_float)), need)
        if got < 0:
            _lib.check(int(got), self._h)
        stride = int(blob.rsplit("stride", 1)[1])
        return arr.reshape(-1, self.net_h // stride, self.net_w // stride)

    def debug_activation(self, blob: str, image: int = 0) -> np.ndarray:
        """Internal NHWC activation named after the reference blob it equals, as a (H, W, C) fp32 array."""
        dims = (C.c_int * 3)()
        need = self._lib.rf_debug_activation(self._h, blob.encode(), image, None, 0, dims)
        if need < 0:
            _lib.check(int(need), self._h)
        arr = np.empty(need, dtype=np.float32)
        got = self._lib.rf_debug_activation(self._h, blob.encode(), image, arr.ctypes.data_as(C.POINTER(C.c_float)),
                                            need, dims)
        if got < 0:
            _lib.check(int(got), self._h)
        return arr.reshape(dims[0], dims[1], dims[2])

    def profile(self, ptrs: Sequence[int], iters: int = 20):
        """Per-kernel HIP-event timing: list of dicts {name, kernel, ms, alg_bytes, macs, compulsory_bytes} in launch order
        (alg_bytes: layer-wise; compulsory_bytes: what the fused launch must move through HBM at least)."""
        n = len(ptrs)
        p = (C.c_void_p * n)(*ptrs)
        cap = 128
        names = (C.c_char_p * cap)()
        kernels = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        ab = (C.c_double * cap)()
        mc = (C.c_double * cap)()
        k = _lib.check(self._lib.rf_profile(self._h, p, n, iters, cap, names, kernels, ms, ab, mc), self._h)
        cb = (C.c_double * cap)()
        _lib.check(self._lib.rf_profile_compulsory_bytes(self._h, n, cap, cb), self._h)
        return [{"name": names[i].decode(), "kernel": kernels[i].decode(), "ms": ms[i], "alg_bytes": ab[i], "macs": mc[i],
                 "compulsory_bytes": cb[i]} for i in range(k)]

    # ------------------------------------------------------------------ internals
    def _run(self, fn, ptrs, rows, cols, steps, n, threshold):
        cap = self.max_detections
        out = (rf_face * (n * cap))()
        counts = (C.c_int * n)()
        st = _lib.check(fn(self._h, ptrs, rows, cols, steps, n, float(threshold), out, cap, counts), self._h)
        self.truncated = st == _lib.RF_ERR_TRUNCATED
        return self._collect(out, counts, n, cap)

    def _collect(self, out, counts, n, cap, anchors=True):
        rows = _faces_to_array(out, n * cap)
        res: List[List[Detection]] = []
        for i in range(n):
            k = min(counts[i], cap)
            idx = (C.c_int32 * max(k, 1))()
            got = self._lib.rf_last_anchor_indices(self._h, i, idx, k) if anchors else -1
            res.append([_detection(rows[i * cap + j], int(idx[j]) if got >= 0 else -1) for j in range(k)])
        return res
