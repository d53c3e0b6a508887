"""retinaface_amd -- MI355X-native drop-in for the RetinaFace::detect() hot path of clancylian/retinaface.

The product is the C-ABI shared library ``retinaface_amd/lib/libretinaface_amd.so`` (hand-written gfx950 HIP
kernels + C++ host runtime, sources in ``retinaface_amd/csrc``, boundary in ``include/retinaface_amd.h``).
This package is a thin ctypes binding over that boundary plus the host-side helpers the benchmark and the
tests need (synthetic face-bearing frames, batch sharding for one-process-per-GPU runs).
There is no CPU fallback: importing works anywhere, but creating a detector without the built library or
without a HIP device raises.
"""
from ._lib import RFError, abi_version, lib_path, load_library  # noqa: F401
from .detector import (PRECISION_FP16, PRECISION_FP32, PRECISION_INT8, QUALITY_DTYPE, Detection, RetinaFace, align_matrix,  # noqa: F401
                       face_aa_factor, face_batch_plan, face_batch_spec, face_gate, face_gate_eval, face_pose, face_value_table, tile_map_face,
                       tile_plan, tile_spec)
from .detector import (FACE_DTYPE, TRACK_BEST, TRACK_CONFIRMED, TRACK_DTYPE, TRACK_NEW, TRACK_OVERFLOW, TRACK_TAG_DTYPE, TRACK_UNTRACKED,  # noqa: F401
                       Tracker, track_spec, track_step)
from .detector import SHOT_DTYPE, shot_resolve  # noqa: F401
from .detector import debug_face_bands, debug_grid_log, debug_resident_cap  # noqa: F401
from .detector import MOTION_DTYPE, motion_spec, track_predict  # noqa: F401
from .detector import tta_map_face, tta_merge_host, tta_spec  # noqa: F401
from .detector import rot_map_face, rot_merge_host, rot_spec, rotate_host  # noqa: F401
from .detector import (LENS_EQUIDISTANT, LENS_EQUISOLID, LENS_ORTHOGRAPHIC, LENS_STEREOGRAPHIC, Dewarper, dewarp_host,  # noqa: F401
                       dewarp_map_face, dewarp_merge_host, dewarp_plan, dewarp_spec)
from .detector import ROI_VOID, roi_cells_from_tracks  # noqa: F401
from .detector import Changer, change_spec, change_step_host  # noqa: F401
from .detector import ROI_CROPPED, roi_atlas_host, roi_map_face, roi_merge_host, roi_plan, roi_spec, rois_from_faces  # noqa: F401
from .detector import enhance_host, enhance_spec  # noqa: F401
from .detector import pyramid_map_face, pyramid_merge_host, pyramid_plan, pyramid_spec, zoom_host  # noqa: F401
from .detector import (OVERLAY_LABEL_ID, OVERLAY_LABEL_NONE, OVERLAY_LABEL_SCORE, overlay_host, overlay_region,  # noqa: F401
                       overlay_spec)
from .detector import REDACT_ELLIPSE, REDACT_FILL, REDACT_PIXELATE, REDACT_RECT, redact_host, redact_region, redact_spec  # noqa: F401
