"""ctypes binding of include/retinaface_amd.h (one declaration per exported symbol)."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path() -> str:
    return os.environ.get("RETINAFACE_AMD_LIB", os.path.join(_HERE, "lib", "libretinaface_amd.so"))


class RFError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"retinaface_amd error {status}: {message}")
        self.status = status


RF_OK, RF_ERR_INVALID_ARG, RF_ERR_IO, RF_ERR_MODEL, RF_ERR_HIP, RF_ERR_UNSUPPORTED, RF_ERR_TRUNCATED = 0, -1, -2, -3, -4, -5, -6


class rf_face(C.Structure):
    _fields_ = [("score", C.c_float), ("x1", C.c_float), ("y1", C.c_float), ("x2", C.c_float), ("y2", C.c_float),
                ("px", C.c_float * 5), ("py", C.c_float * 5)]


class rf_options(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("precision", C.c_int32), ("net_h", C.c_int32), ("net_w", C.c_int32),
                ("max_batch", C.c_int32), ("device", C.c_int32), ("max_candidates", C.c_int32),
                ("max_detections", C.c_int32), ("use_graph", C.c_int32), ("keep_outputs", C.c_int32),
                ("model_stem", C.c_char_p), ("lanes", C.c_int32), ("coalesce", C.c_int32),
                ("copy_threads", C.c_int32), ("n_devices", C.c_int32), ("devices", C.POINTER(C.c_int32)),
                ("plan_cache", C.c_int32), ("oversize_resize", C.c_int32)]


class rf_face_batch_spec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("crop_size", C.c_int32), ("format", C.c_int32), ("rgb", C.c_int32),
                ("mean", C.c_float * 3), ("scale", C.c_float * 3), ("max_faces", C.c_int32), ("capacity", C.c_int32),
                ("antialias", C.c_int32), ("aa_max", C.c_int32)]


RF_FACES_U8_HWC, RF_FACES_F16_CHW, RF_FACES_F32_CHW = 0, 1, 2


class rf_face_quality(C.Structure):
    _fields_ = [("flags", C.c_int32), ("covered", C.c_int32), ("sum_luma", C.c_int64), ("sum_lap", C.c_int64), ("sum_lap2", C.c_int64),
                ("sharpness", C.c_double), ("iod2", C.c_double), ("yaw", C.c_double), ("sin2_roll", C.c_double)]


class rf_face_gate(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_sharpness", C.c_float), ("min_iod", C.c_float), ("max_abs_yaw", C.c_float),
                ("max_sin2_roll", C.c_float), ("min_covered", C.c_float), ("min_luma", C.c_float), ("max_luma", C.c_float)]


class rf_tile_spec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("overlap", C.c_int32), ("edge", C.c_int32), ("full_frame", C.c_int32),
                ("max_faces", C.c_int32)]


class rf_track_spec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_tracks", C.c_int32), ("min_iou", C.c_float), ("max_missed", C.c_int32),
                ("min_hits", C.c_int32), ("new_score", C.c_float)]


class rf_track(C.Structure):
    _fields_ = [("id", C.c_int64), ("first_frame", C.c_int64), ("last_frame", C.c_int64), ("best_frame", C.c_int64),
                ("best_value", C.c_double), ("hits", C.c_int32), ("missed", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
                ("last", rf_face), ("best", rf_face)]


class rf_track_tag(C.Structure):
    _fields_ = [("id", C.c_int64), ("slot", C.c_int32), ("hits", C.c_int32), ("age", C.c_int32), ("flags", C.c_int32)]


class rf_shot(C.Structure):
    _fields_ = [("id", C.c_int64), ("frame", C.c_int64), ("matrix", C.c_double * 6)]


class rf_motion_spec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("alpha", C.c_float), ("horizon", C.c_int32), ("reserved", C.c_int32)]


class rf_track_motion(C.Structure):
    _fields_ = [("vx", C.c_float), ("vy", C.c_float), ("samples", C.c_int32), ("reserved", C.c_int32)]


class rf_follow_spec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("radius", C.c_int32), ("max_mad", C.c_int32), ("max_run", C.c_int32), ("reserved", C.c_int32)]


class rf_track_follow(C.Structure):
    _fields_ = [("valid", C.c_int32), ("run", C.c_int32), ("q", C.c_int32), ("ox", C.c_int32), ("oy", C.c_int32), ("sad", C.c_int32),
                ("dx", C.c_int32), ("dy", C.c_int32)]


RF_TRACK_FOLLOWED = 32
RF_SHOT_NONE, RF_SHOT_STORED, RF_SHOT_LAUNCH = 0, 1, 2
RF_SHOT_MAX_BYTES = 1 << 30


class rf_redact_spec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("shape", C.c_int32), ("cells", C.c_int32), ("margin", C.c_float),
                ("fill", C.c_uint8 * 3), ("blur", C.c_uint8), ("max_regions", C.c_int32), ("coast", C.c_int32)]


class rf_overlay_spec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("thickness", C.c_int32), ("radius", C.c_int32), ("box", C.c_uint8 * 3),
                ("colors_set", C.c_uint8), ("point", C.c_uint8 * 3), ("alpha", C.c_uint8), ("text", C.c_uint8 * 3),
                ("color_by_id", C.c_uint8), ("label", C.c_int32), ("font_scale", C.c_int32), ("max_regions", C.c_int32),
                ("coast", C.c_int32)]


RF_OVERLAY_LABEL_NONE, RF_OVERLAY_LABEL_SCORE, RF_OVERLAY_LABEL_ID = 0, 1, 2
RF_REDACT_PIXELATE, RF_REDACT_FILL = 0, 1
RF_REDACT_RECT, RF_REDACT_ELLIPSE = 0, 1

RF_TRACK_NEW, RF_TRACK_CONFIRMED, RF_TRACK_BEST, RF_TRACK_UNTRACKED, RF_TRACK_OVERFLOW = 1, 2, 4, 8, 16

class rf_tta_spec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flip", C.c_int32), ("vote", C.c_int32), ("max_faces", C.c_int32)]


class rf_rot_spec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("rots", C.c_int32), ("vote", C.c_int32), ("max_faces", C.c_int32)]


class rf_dewarp_view(C.Structure):
    _fields_ = [("yaw", C.c_double), ("pitch", C.c_double), ("roll", C.c_double), ("hfov", C.c_double)]


class rf_dewarp_spec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("model", C.c_int32), ("f", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("views", C.c_int32), ("ring", C.c_int32), ("ring_pitch", C.c_double), ("ring_hfov", C.c_double),
                ("view", rf_dewarp_view * 16), ("vote", C.c_int32), ("max_faces", C.c_int32), ("edge", C.c_int32),
                ("reserved_", C.c_int32)]


RF_LENS_EQUIDISTANT, RF_LENS_EQUISOLID, RF_LENS_STEREOGRAPHIC, RF_LENS_ORTHOGRAPHIC = 0, 1, 2, 3


class rf_roi(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]


class rf_roi_cell(C.Structure):
    _fields_ = [("roi", rf_roi), ("level", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("flags", C.c_int32)]


class rf_roi_spec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("grid", C.c_int32), ("max_zoom", C.c_int32), ("vote", C.c_int32), ("max_faces", C.c_int32),
                ("reserved", C.c_int32)]


RF_ROI_MAX_REGIONS, RF_ROI_CROPPED, RF_ROI_VOID = 256, 1, 2


class rf_change_spec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("block", C.c_int32), ("thr_q4", C.c_int32), ("adapt_shift", C.c_int32), ("dilate", C.c_int32),
                ("min_blocks", C.c_int32), ("max_regions", C.c_int32), ("reserved", C.c_int32)]


class rf_change_info(C.Structure):
    _fields_ = [("changed_blocks", C.c_int32), ("components", C.c_int32), ("kept", C.c_int32), ("flags", C.c_int32)]


class rf_enhance_spec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("tile", C.c_int32), ("clip", C.c_int32), ("dark_below", C.c_int32)]


class rf_pyramid_spec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("levels", C.c_int32), ("overlap", C.c_int32), ("edge", C.c_int32),
                ("full_frame", C.c_int32), ("max_faces", C.c_int32), ("vote", C.c_int32)]


RF_GATE_INVALID, RF_GATE_SHARPNESS, RF_GATE_IOD, RF_GATE_YAW, RF_GATE_ROLL, RF_GATE_COVERED, RF_GATE_DARK, RF_GATE_BRIGHT = (
    1, 2, 4, 8, 16, 32, 64, 128)

# every symbol include/retinaface_amd.h declares: name -> (restype, argtypes)
_PP = C.POINTER
SYMBOLS = {
    "rf_abi_version": (C.c_int, []),
    "rf_create": (C.c_int, [C.c_char_p, C.c_char_p, C.c_float, _PP(rf_options), _PP(C.c_void_p)]),
    "rf_preset_anchors": (C.c_int, [C.c_char_p, C.c_int, _PP(C.c_float), C.c_int]),
    "rf_destroy": (None, [C.c_void_p]),
    "rf_last_error": (C.c_char_p, [C.c_void_p]),
    "rf_get_net_size": (C.c_int, [C.c_void_p, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int)]),
    "rf_detect_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                  C.c_float, _PP(rf_face), C.c_int, _PP(C.c_int)]),
    "rf_detect_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int),
                                         C.c_int, C.c_float, _PP(rf_face), C.c_int, _PP(C.c_int)]),
    "rf_detect_batch_pad32": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                        C.c_int, C.c_float, _PP(rf_face), C.c_int, _PP(C.c_int)]),
    "rf_frame_scale": (C.c_float, [C.c_void_p, C.c_int, C.c_int]),
    "rf_align_matrix": (C.c_int, [_PP(rf_face), C.c_float, C.c_int, _PP(C.c_double)]),
    "rf_align_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                        _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_float), C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p, _PP(C.c_double)]),
    "rf_detect_align_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                               C.c_float, _PP(rf_face), C.c_int, _PP(C.c_int), C.c_int, C.c_int,
                                               C.c_void_p, C.c_void_p, _PP(C.c_double)]),
    "rf_detect_align_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                        C.c_float, _PP(rf_face), C.c_int, _PP(C.c_int), C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p, _PP(C.c_double)]),
    "rf_face_batch_plan": (C.c_long, [_PP(rf_face_batch_spec), _PP(C.c_int), C.c_int, _PP(C.c_int), _PP(C.c_size_t)]),
    "rf_face_value_table": (C.c_int, [_PP(rf_face_batch_spec), C.c_int, C.c_void_p]),
    "rf_face_aa_factor": (C.c_int, [_PP(rf_face), C.c_float, C.c_int, C.c_int]),
    "rf_detect_face_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                              C.c_float, _PP(rf_face), C.c_int, _PP(C.c_int), _PP(rf_face_batch_spec),
                                              C.c_void_p, C.c_void_p, _PP(C.c_double), _PP(C.c_int)]),
    "rf_detect_face_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                       C.c_float, _PP(rf_face), C.c_int, _PP(C.c_int), _PP(rf_face_batch_spec),
                                       C.c_void_p, C.c_void_p, _PP(C.c_double), _PP(C.c_int)]),
    "rf_face_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                       _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_float), _PP(rf_face_batch_spec),
                                       C.c_void_p, C.c_void_p, _PP(C.c_double), _PP(C.c_int)]),
    "rf_face_pose": (C.c_int, [_PP(rf_face), C.c_float, C.c_int, _PP(rf_face_quality)]),
    "rf_face_gate_eval": (C.c_int, [_PP(rf_face_gate), _PP(rf_face_quality), C.c_int]),
    "rf_face_quality_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                         _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_float), C.c_int, C.c_int,
                                         _PP(rf_face_gate), _PP(rf_face_quality)]),
    "rf_face_batch_gated_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                             _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_float), _PP(rf_face_batch_spec),
                                             C.c_void_p, C.c_void_p, _PP(C.c_double), _PP(C.c_int), _PP(rf_face_gate),
                                             _PP(rf_face_quality)]),
    "rf_detect_face_batch_gated_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                                    C.c_float, _PP(rf_face), C.c_int, _PP(C.c_int), _PP(rf_face_batch_spec),
                                                    C.c_void_p, C.c_void_p, _PP(C.c_double), _PP(C.c_int), _PP(rf_face_gate),
                                                    _PP(rf_face_quality)]),
    "rf_detect_face_batch_gated": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                             C.c_float, _PP(rf_face), C.c_int, _PP(C.c_int), _PP(rf_face_batch_spec),
                                             C.c_void_p, C.c_void_p, _PP(C.c_double), _PP(C.c_int), _PP(rf_face_gate),
                                             _PP(rf_face_quality)]),
    "rf_tile_plan": (C.c_int, [_PP(rf_tile_spec), C.c_int, C.c_int, C.c_int, C.c_int, _PP(C.c_int), C.c_int]),
    "rf_tile_map_face": (C.c_int, [_PP(rf_tile_spec), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _PP(rf_face), _PP(rf_face)]),
    "rf_detect_tiled_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                               C.c_float, _PP(rf_tile_spec), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int)]),
    "rf_detect_tiled_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                        C.c_float, _PP(rf_tile_spec), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int)]),
    "rf_tile_merge_device": (C.c_int, [C.c_void_p, _PP(C.c_int), _PP(C.c_int), C.c_int, _PP(rf_tile_spec), _PP(rf_face), _PP(C.c_int),
                                       _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int)]),
    "rf_detect_tiled_face_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                                    C.c_float, _PP(rf_tile_spec), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int),
                                                    _PP(rf_face_batch_spec), C.c_void_p, C.c_void_p, _PP(C.c_double), _PP(C.c_int),
                                                    _PP(rf_face_gate), _PP(rf_face_quality)]),
    "rf_track_step": (C.c_int, [_PP(rf_track_spec), _PP(rf_track), _PP(C.c_int64), _PP(C.c_int64), _PP(rf_face), C.c_int, C.c_float,
                                _PP(rf_face_quality), C.c_int, _PP(rf_track_tag), _PP(rf_track), C.c_int, _PP(C.c_int)]),
    "rf_tracker_create": (C.c_int, [C.c_void_p, _PP(rf_track_spec), C.c_int, _PP(C.c_void_p)]),
    "rf_tracker_destroy": (None, [C.c_void_p]),
    "rf_tracker_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "rf_tracker_read": (C.c_int, [C.c_void_p, C.c_int, _PP(rf_track), C.c_int, _PP(C.c_int64), _PP(C.c_int64)]),
    "rf_tracker_flush": (C.c_int, [C.c_void_p, C.c_int, _PP(rf_track), C.c_int, _PP(C.c_int64), _PP(C.c_int64)]),
    "rf_track_update_device": (C.c_int, [C.c_void_p, C.c_void_p, _PP(C.c_int), C.c_int, _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_float),
                                         _PP(rf_face_quality), C.c_int, _PP(rf_track_tag), _PP(rf_track), C.c_int, _PP(C.c_int)]),
    "rf_track_last_launch_ms": (C.c_int, [C.c_void_p, _PP(C.c_float)]),
    "rf_detect_track_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, C.c_float,
                                               _PP(rf_face), C.c_int, _PP(C.c_int), C.c_void_p, _PP(C.c_int), _PP(rf_track_tag),
                                               _PP(rf_track), C.c_int, _PP(C.c_int)]),
    "rf_detect_track_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, C.c_float,
                                        _PP(rf_face), C.c_int, _PP(C.c_int), C.c_void_p, _PP(C.c_int), _PP(rf_track_tag),
                                        _PP(rf_track), C.c_int, _PP(C.c_int)]),
    "rf_detect_track_face_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                                    C.c_float, _PP(rf_face), C.c_int, _PP(C.c_int), _PP(rf_face_batch_spec),
                                                    C.c_void_p, C.c_void_p, _PP(C.c_double), _PP(C.c_int), _PP(rf_face_gate),
                                                    _PP(rf_face_quality), C.c_void_p, _PP(C.c_int), _PP(rf_track_tag), _PP(rf_track),
                                                    C.c_int, _PP(C.c_int)]),
    "rf_shot_resolve": (C.c_int, [C.c_int, C.c_int, _PP(rf_track_tag), C.c_int, _PP(C.c_int), _PP(rf_track), C.c_int, _PP(C.c_int), C.c_int64,
                                  _PP(rf_face), _PP(C.c_float), C.c_int, _PP(rf_shot), _PP(C.c_int32), _PP(C.c_int32)]),
    "rf_tracker_enable_shots": (C.c_int, [C.c_void_p, _PP(rf_face_batch_spec)]),
    "rf_tracker_read_shots": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, _PP(rf_shot), C.c_int]),
    "rf_tracker_flush_shots": (C.c_int, [C.c_void_p, C.c_int, _PP(rf_track), C.c_int, _PP(C.c_int64), _PP(C.c_int64), C.c_void_p,
                                         _PP(rf_shot)]),
    "rf_track_shots_device": (C.c_int, [C.c_void_p, C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                        _PP(C.c_int), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_float), _PP(rf_face_quality),
                                        _PP(rf_track_tag), _PP(rf_track), C.c_int, _PP(C.c_int), C.c_void_p, C.c_void_p, _PP(rf_shot)]),
    "rf_shot_last_launch_ms": (C.c_int, [C.c_void_p, _PP(C.c_float)]),
    "rf_track_step_motion": (C.c_int, [_PP(rf_track_spec), _PP(rf_motion_spec), _PP(rf_track), _PP(rf_track_motion), _PP(C.c_int64),
                                       _PP(C.c_int64), _PP(rf_face), C.c_int, C.c_float, _PP(rf_face_quality), C.c_int, _PP(rf_track_tag),
                                       _PP(rf_track), C.c_int, _PP(C.c_int)]),
    "rf_track_predict": (C.c_int, [_PP(rf_motion_spec), _PP(rf_track), _PP(rf_track_motion), C.c_int, _PP(rf_face)]),
    "rf_tracker_enable_motion": (C.c_int, [C.c_void_p, _PP(rf_motion_spec)]),
    "rf_tracker_read_motion": (C.c_int, [C.c_void_p, C.c_int, _PP(rf_track_motion), C.c_int]),
    "rf_follow_geometry": (C.c_int, [_PP(C.c_float), _PP(C.c_int32)]),
    "rf_follow_template": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rf_follow_search": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _PP(C.c_int32)]),
    "rf_track_step_follow_key": (C.c_int, [_PP(rf_track_spec), _PP(rf_track), _PP(rf_track_follow), C.c_void_p, _PP(C.c_int64), _PP(C.c_int64),
                                           C.c_void_p, C.c_int, C.c_int, C.c_int, _PP(rf_face), C.c_int, C.c_float, _PP(rf_face_quality),
                                           C.c_int, _PP(rf_track_tag), _PP(rf_track), C.c_int, _PP(C.c_int)]),
    "rf_track_step_follow": (C.c_int, [_PP(rf_track_spec), _PP(rf_follow_spec), _PP(rf_track), _PP(rf_track_follow), C.c_void_p,
                                       _PP(C.c_int64), C.c_void_p, C.c_int, C.c_int, C.c_int, _PP(rf_face), _PP(rf_track_tag), C.c_int,
                                       _PP(C.c_int), _PP(rf_track), C.c_int, _PP(C.c_int)]),
    "rf_tracker_enable_follow": (C.c_int, [C.c_void_p, _PP(rf_follow_spec)]),
    "rf_tracker_read_follow": (C.c_int, [C.c_void_p, C.c_int, _PP(rf_track_follow), C.c_void_p, C.c_int]),
    "rf_track_follow_update_device": (C.c_int, [C.c_void_p, C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                                _PP(C.c_int), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_float), _PP(rf_face_quality),
                                                _PP(rf_track_tag), _PP(rf_track), C.c_int, _PP(C.c_int)]),
    "rf_detect_track_follow_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                                      C.c_float, _PP(rf_face), C.c_int, _PP(C.c_int), C.c_void_p, _PP(C.c_int),
                                                      _PP(rf_track_tag), _PP(rf_track), C.c_int, _PP(C.c_int)]),
    "rf_detect_track_follow_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                               C.c_float, _PP(rf_face), C.c_int, _PP(C.c_int), C.c_void_p, _PP(C.c_int),
                                               _PP(rf_track_tag), _PP(rf_track), C.c_int, _PP(C.c_int)]),
    "rf_track_follow_device": (C.c_int, [C.c_void_p, C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                         _PP(C.c_int), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(rf_track_tag), _PP(rf_track), C.c_int,
                                         _PP(C.c_int)]),
    "rf_track_follow_batch": (C.c_int, [C.c_void_p, C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                        _PP(C.c_int), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(rf_track_tag), _PP(rf_track), C.c_int,
                                        _PP(C.c_int)]),
    "rf_follow_last_launch_ms": (C.c_int, [C.c_void_p, _PP(C.c_float)]),
    "rf_detect_track_shots_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                                     C.c_float, _PP(rf_face), C.c_int, _PP(C.c_int), C.c_void_p, _PP(C.c_int),
                                                     _PP(rf_track_tag), _PP(rf_track), C.c_int, _PP(C.c_int), _PP(rf_face_gate),
                                                     _PP(rf_face_quality), C.c_void_p, C.c_void_p, _PP(rf_shot)]),
    "rf_detect_track_shots_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                              C.c_float, _PP(rf_face), C.c_int, _PP(C.c_int), C.c_void_p, _PP(C.c_int),
                                              _PP(rf_track_tag), _PP(rf_track), C.c_int, _PP(C.c_int), _PP(rf_face_gate),
                                              _PP(rf_face_quality), C.c_void_p, C.c_void_p, _PP(rf_shot)]),
    "rf_redact_region": (C.c_int, [_PP(rf_redact_spec), _PP(rf_face), C.c_float, C.c_int, C.c_int, _PP(C.c_int)]),
    "rf_redact_host": (C.c_int, [_PP(rf_redact_spec), C.c_void_p, C.c_int, C.c_int, C.c_int, _PP(rf_face), C.c_int, C.c_float,
                                 _PP(C.c_int32)]),
    "rf_redact_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, _PP(rf_face), C.c_int,
                                   _PP(C.c_int), _PP(C.c_float), _PP(rf_redact_spec), C.c_void_p, _PP(C.c_int), _PP(C.c_int32),
                                   _PP(C.c_int)]),
    "rf_redact_last_launch_ms": (C.c_int, [C.c_void_p, _PP(C.c_float)]),
    "rf_detect_redact_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, C.c_float,
                                                _PP(rf_face), C.c_int, _PP(C.c_int), _PP(rf_redact_spec), _PP(C.c_int32)]),
    "rf_detect_redact_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, C.c_float,
                                         _PP(rf_face), C.c_int, _PP(C.c_int), _PP(rf_redact_spec), _PP(C.c_void_p), _PP(C.c_int),
                                         _PP(C.c_int32)]),
    "rf_detect_track_redact_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                                      C.c_float, _PP(rf_face), C.c_int, _PP(C.c_int), C.c_void_p, _PP(C.c_int),
                                                      _PP(rf_track_tag), _PP(rf_track), C.c_int, _PP(C.c_int), _PP(rf_redact_spec),
                                                      _PP(C.c_int32), _PP(C.c_int)]),
    "rf_overlay_region": (C.c_int, [_PP(rf_overlay_spec), _PP(rf_face), C.c_int64, C.c_float, C.c_int, C.c_int, _PP(C.c_int32)]),
    "rf_overlay_host": (C.c_int, [_PP(rf_overlay_spec), C.c_void_p, C.c_int, C.c_int, C.c_int, _PP(rf_face), _PP(C.c_int64), C.c_int,
                                  C.c_float, _PP(C.c_int32)]),
    "rf_overlay_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, _PP(rf_face),
                                    _PP(C.c_int64), C.c_int, _PP(C.c_int), _PP(C.c_float), _PP(rf_overlay_spec), C.c_void_p, _PP(C.c_int),
                                    _PP(C.c_int32), _PP(C.c_int)]),
    "rf_overlay_last_launch_ms": (C.c_int, [C.c_void_p, _PP(C.c_float)]),
    "rf_detect_overlay_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, C.c_float,
                                                 _PP(rf_face), C.c_int, _PP(C.c_int), _PP(rf_overlay_spec), _PP(C.c_int32)]),
    "rf_detect_overlay_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, C.c_float,
                                          _PP(rf_face), C.c_int, _PP(C.c_int), _PP(rf_overlay_spec), _PP(C.c_void_p), _PP(C.c_int),
                                          _PP(C.c_int32)]),
    "rf_detect_track_overlay_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                                       C.c_float, _PP(rf_face), C.c_int, _PP(C.c_int), C.c_void_p, _PP(C.c_int),
                                                       _PP(rf_track_tag), _PP(rf_track), C.c_int, _PP(C.c_int), _PP(rf_overlay_spec),
                                                       _PP(C.c_int32), _PP(C.c_int)]),
    "rf_tta_map_face": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _PP(rf_face), _PP(rf_face)]),
    "rf_tta_merge_host": (C.c_int, [_PP(rf_tta_spec), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _PP(rf_face), _PP(C.c_int),
                                    _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int)]),
    "rf_mirror_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "rf_detect_tta_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                             C.c_float, _PP(rf_tta_spec), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int)]),
    "rf_detect_tta_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                      C.c_float, _PP(rf_tta_spec), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int)]),
    "rf_tta_merge_device": (C.c_int, [C.c_void_p, _PP(C.c_int), _PP(C.c_int), C.c_int, _PP(rf_tta_spec), _PP(rf_face), _PP(C.c_int),
                                      _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int)]),
    "rf_rot_map_face": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _PP(rf_face), _PP(rf_face)]),
    "rf_rot_merge_host": (C.c_int, [_PP(rf_rot_spec), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _PP(rf_face), _PP(C.c_int),
                                    _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), _PP(C.c_float)]),
    "rf_rotate_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "rf_rotate_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "rf_detect_rot_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                             C.c_float, _PP(rf_rot_spec), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int),
                                             _PP(C.c_int), _PP(C.c_float)]),
    "rf_detect_rot_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                      C.c_float, _PP(rf_rot_spec), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int),
                                      _PP(C.c_int), _PP(C.c_float)]),
    "rf_rot_merge_device": (C.c_int, [C.c_void_p, _PP(C.c_int), _PP(C.c_int), C.c_int, _PP(rf_rot_spec), _PP(rf_face), _PP(C.c_int),
                                      _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), _PP(C.c_float)]),
    "rf_dewarp_plan": (C.c_int, [_PP(rf_dewarp_spec), C.c_int, C.c_int, _PP(C.c_int32), C.c_int, _PP(C.c_int)]),
    "rf_dewarp_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "rf_dewarp_map_face": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _PP(rf_face), _PP(rf_face)]),
    "rf_dewarp_merge_host": (C.c_int, [_PP(rf_dewarp_spec), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                       _PP(rf_face), _PP(C.c_int), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int)]),
    "rf_dewarper_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, _PP(C.c_void_p)]),
    "rf_dewarper_destroy": (None, [C.c_void_p]),
    "rf_dewarp_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "rf_detect_dewarp_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, C.c_float,
                                                _PP(rf_dewarp_spec), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int),
                                                C.c_void_p]),
    "rf_detect_dewarp_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, C.c_float,
                                         _PP(rf_dewarp_spec), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int)]),
    "rf_dewarp_merge_device": (C.c_int, [C.c_void_p, C.c_int, _PP(rf_dewarp_spec), _PP(rf_face), _PP(C.c_int), _PP(rf_face), C.c_int,
                                         _PP(C.c_int), _PP(C.c_int), _PP(C.c_int)]),
    "rf_roi_plan": (C.c_int, [_PP(rf_roi_spec), C.c_int, C.c_int, _PP(rf_roi), C.c_int, _PP(rf_roi_cell), _PP(C.c_int)]),
    "rf_roi_from_faces": (C.c_int, [_PP(rf_face), C.c_int, C.c_float, C.c_int, _PP(rf_roi)]),
    "rf_roi_atlas_host": (C.c_int, [_PP(rf_roi_spec), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, _PP(rf_roi), C.c_int, C.c_void_p,
                                    C.c_int]),
    "rf_roi_map_face": (C.c_int, [_PP(rf_roi_spec), C.c_int, C.c_int, _PP(rf_roi), C.c_int, C.c_int, _PP(rf_face), _PP(rf_face), _PP(C.c_int)]),
    "rf_roi_merge_host": (C.c_int, [_PP(rf_roi_spec), C.c_int, C.c_int, _PP(rf_roi), C.c_int, C.c_float, C.c_int, _PP(rf_face), _PP(C.c_int),
                                    _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int)]),
    "rf_roi_atlas_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _PP(rf_roi), C.c_int, _PP(rf_roi_spec), C.c_int, C.c_int,
                                      C.c_void_p, C.c_int]),
    "rf_detect_roi_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, _PP(rf_roi),
                                             _PP(C.c_int), C.c_float, _PP(rf_roi_spec), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int),
                                             _PP(C.c_int), C.c_void_p]),
    "rf_detect_roi_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, _PP(rf_roi), _PP(C.c_int),
                                      C.c_float, _PP(rf_roi_spec), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int)]),
    "rf_roi_merge_device": (C.c_int, [C.c_void_p, _PP(C.c_int), _PP(C.c_int), C.c_int, _PP(rf_roi), _PP(C.c_int), _PP(rf_roi_spec), _PP(rf_face),
                                      _PP(C.c_int), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int)]),
    "rf_roi_cells_from_tracks": (C.c_int, [_PP(rf_track_spec), _PP(rf_motion_spec), _PP(rf_track), _PP(rf_track_motion), C.c_int, C.c_int, C.c_int,
                                           C.c_int, _PP(rf_roi_spec), _PP(rf_roi_cell)]),
    "rf_roi_track_cells_device": (C.c_int, [C.c_void_p, C.c_void_p, _PP(C.c_int), C.c_int, C.c_int, _PP(rf_roi_spec), _PP(rf_roi_cell)]),
    "rf_detect_track_roi_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, C.c_float,
                                                   _PP(rf_roi_spec), C.c_int, _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int),
                                                   _PP(rf_roi_cell), C.c_void_p, C.c_void_p, _PP(C.c_int), _PP(rf_track_tag), _PP(rf_track), C.c_int,
                                                   _PP(C.c_int)]),
    "rf_detect_track_roi_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, C.c_float,
                                            _PP(rf_roi_spec), C.c_int, _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int),
                                            _PP(rf_roi_cell), C.c_void_p, C.c_void_p, _PP(C.c_int), _PP(rf_track_tag), _PP(rf_track), C.c_int,
                                            _PP(C.c_int)]),
    "rf_changer_create": (C.c_int, [C.c_void_p, _PP(rf_change_spec), C.c_int, C.c_int, C.c_int, _PP(C.c_void_p)]),
    "rf_changer_destroy": (None, [C.c_void_p]),
    "rf_changer_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "rf_changer_read": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, _PP(C.c_int64), C.c_void_p]),
    "rf_change_step_host": (C.c_int, [_PP(rf_change_spec), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, _PP(C.c_int64), C.c_int, C.c_int,
                                      C.c_int, _PP(rf_roi_spec), C.c_void_p, _PP(rf_roi), _PP(rf_roi_cell), _PP(rf_change_info)]),
    "rf_change_regions_device": (C.c_int, [C.c_void_p, C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                           C.c_int, _PP(rf_roi_spec), _PP(rf_roi_cell), _PP(rf_change_info)]),
    "rf_detect_change_roi_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, C.c_float,
                                                    _PP(rf_roi_spec), C.c_int, _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int),
                                                    _PP(rf_roi_cell), C.c_void_p, C.c_void_p, _PP(rf_change_info), C.c_void_p, _PP(C.c_int),
                                                    _PP(rf_track_tag), _PP(rf_track), C.c_int, _PP(C.c_int)]),
    "rf_detect_change_roi_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, C.c_float,
                                             _PP(rf_roi_spec), C.c_int, _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int),
                                             _PP(rf_roi_cell), C.c_void_p, C.c_void_p, _PP(rf_change_info), C.c_void_p, _PP(C.c_int),
                                             _PP(rf_track_tag), _PP(rf_track), C.c_int, _PP(C.c_int)]),
    "rf_enhance_host": (C.c_int, [_PP(rf_enhance_spec), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, _PP(C.c_int)]),
    "rf_enhance_device": (C.c_int, [C.c_void_p, _PP(rf_enhance_spec), _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                    _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int)]),
    "rf_detect_enhanced_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, C.c_float,
                                                  _PP(rf_enhance_spec), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_void_p), _PP(C.c_int),
                                                  _PP(C.c_int)]),
    "rf_detect_enhanced_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int, C.c_float,
                                           _PP(rf_enhance_spec), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_void_p), _PP(C.c_int),
                                           _PP(C.c_int)]),
    "rf_pyramid_plan": (C.c_int, [_PP(rf_pyramid_spec), C.c_int, C.c_int, C.c_int, C.c_int, _PP(C.c_int), C.c_int]),
    "rf_pyramid_map_face": (C.c_int, [_PP(rf_pyramid_spec), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _PP(rf_face), _PP(rf_face)]),
    "rf_pyramid_merge_host": (C.c_int, [_PP(rf_pyramid_spec), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _PP(rf_face),
                                        _PP(C.c_int), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int)]),
    "rf_zoom_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "rf_zoom_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_int]),
    "rf_detect_pyramid_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                                 C.c_float, _PP(rf_pyramid_spec), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int),
                                                 _PP(C.c_int)]),
    "rf_detect_pyramid_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int), C.c_int,
                                          C.c_float, _PP(rf_pyramid_spec), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int)]),
    "rf_pyramid_merge_device": (C.c_int, [C.c_void_p, _PP(C.c_int), _PP(C.c_int), C.c_int, _PP(rf_pyramid_spec), _PP(rf_face),
                                          _PP(C.c_int), _PP(rf_face), C.c_int, _PP(C.c_int), _PP(C.c_int), _PP(C.c_int)]),
    "rf_num_slots": (C.c_int, [C.c_void_p]),
    "rf_enqueue_batch_device": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int),
                                          C.c_int, C.c_float, _PP(C.c_int)]),
    "rf_wait": (C.c_int, [C.c_void_p, C.c_int, _PP(rf_face), C.c_int, _PP(C.c_int)]),
    "rf_enqueue_batch": (C.c_int, [C.c_void_p, _PP(C.c_void_p), _PP(C.c_int), _PP(C.c_int), _PP(C.c_int),
                                   C.c_int, C.c_float, _PP(C.c_int)]),
    "rf_host_register": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "rf_host_unregister": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rf_invalidate_residency": (C.c_int, [C.c_void_p]),
    "rf_num_devices": (C.c_int, [C.c_void_p]),
    "rf_scatter_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "rf_launch_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "rf_last_anchor_indices": (C.c_int, [C.c_void_p, C.c_int, _PP(C.c_int32), C.c_int]),
    "rf_last_candidate_counts": (C.c_int, [C.c_void_p, _PP(C.c_int), C.c_int]),
    "rf_last_timings": (C.c_int, [C.c_void_p, _PP(C.c_float), _PP(C.c_float), _PP(C.c_float), _PP(C.c_float)]),
    "rf_get_output": (C.c_long, [C.c_void_p, C.c_char_p, C.c_int, _PP(C.c_float), C.c_size_t]),
    "rf_debug_activation": (C.c_long, [C.c_void_p, C.c_char_p, C.c_int, _PP(C.c_float), C.c_size_t, _PP(C.c_int)]),
    "rf_profile": (C.c_int, [C.c_void_p, _PP(C.c_void_p), C.c_int, C.c_int, C.c_int, _PP(C.c_char_p), _PP(C.c_char_p),
                             _PP(C.c_float), _PP(C.c_double), _PP(C.c_double)]),
    "rf_profile_compulsory_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _PP(C.c_double)]),
    "rf_debug_resident_cap": (None, [C.c_int]),
    "rf_debug_grid_log": (C.c_int, [C.c_int, _PP(C.c_int), _PP(C.c_int)]),
    "rf_debug_face_bands": (C.c_int, [C.c_int, C.c_int, _PP(C.c_int), _PP(C.c_int)]),
    "rf_convert_model": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]),
    "rf_plan_cache_probe": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, _PP(C.c_size_t)]),
    "rf_plan_folded": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, _PP(C.c_float), C.c_size_t, _PP(C.c_float),
                                 C.c_size_t, _PP(C.c_int)]),
    "rf_plan_int8_gemm": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, _PP(C.c_float), C.c_size_t, _PP(C.c_float), C.c_size_t,
                                    _PP(C.c_float), _PP(C.c_float), C.c_size_t, _PP(C.c_int)]),
    "rf_attach_calibration": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]),
}

ABI_VERSION = 2      # include/retinaface_amd.h RF_ABI_VERSION
_lib = None


def load_library() -> C.CDLL:
    """Load the HIP library; there is no fallback -- a missing build is a hard error."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm wheels bundle their own libamdhip64.so / libhsa-runtime64.so (same SONAME as /opt/rocm's).  If this
    # library were loaded first it would pull in /opt/rocm's copy and a later `import torch` would bring a SECOND HIP
    # runtime into the process (the second one then finds no device).  Importing torch first makes both share one.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           f"or `make -C retinaface_amd/csrc` (there is no CPU fallback)")
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.rf_abi_version() != ABI_VERSION:
        raise RuntimeError("libretinaface_amd.so ABI version mismatch")
    _lib = lib
    return lib


def abi_version() -> int:
    return load_library().rf_abi_version()


def check(status: int, handle=None) -> int:
    if status >= 0 or status == RF_ERR_TRUNCATED:
        return status
    msg = load_library().rf_last_error(handle)
    raise RFError(status, msg.decode("utf-8", "replace") if msg else "")
