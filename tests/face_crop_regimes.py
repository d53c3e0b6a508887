"""The face-crop kernels' band regimes ("Face batches", "Face quality", "Best-shot gallery"): a helper, not a test.

align_kernel, face_batch_kernel, shot_keep_kernel and shot_deliver_kernel write a crop in bands of rows whose height depends on the crop
size and the element type (face_batch_band_rows in kernels.hip); face_quality_kernel walks it in bands of ring_rows - 2 new luma rows
(face_quality_ring_rows).  This file holds the one table of (format, crop) cases that runs every band height, and the one recipe for
the frame and the faces of a case.  tests/test_face_crop_regimes_host.py proves, from the library's own answer (rf_debug_face_bands),
that the table covers every regime and that the recipe's faces are what the GPU sweep needs; tests/test_face_crop_regimes_gpu.py runs
the sweep.  Both import everything from here, so the sweep and its preconditions cannot drift apart.

The sizes are the combinations the other GPU tests do not run (those stay within 16..128, all of them 8-row bands): per format the
smallest crop of every band height (16 for the 8-row bands, the one size here that the other tests run too), the crop just below every
transition (the fullest LDS run of its height), 511 and 512.
"""
import functools

import numpy as np

import align_ref
import face_aa_ref as far
import face_batch_ref as fbr
import face_quality_ref as fqr
from test_gpu_align import _template_face

FORMATS = ("u8", "f16", "f32")
ES = {"u8": 1, "f16": 2, "f32": 4}
CROPS = range(16, 513)                                                   # what the entry points accept

SIZES = {
    "f32": (16, 128, 129, 146, 147, 170, 171, 204, 205, 256, 257, 341, 342, 511, 512),
    "f16": (16, 256, 257, 292, 293, 341, 342, 409, 410, 511, 512),
    "u8": (16, 17, 511, 512),                                            # also align_kernel's
}
CASES = tuple((fmt, crop) for fmt in ("f32", "f16", "u8") for crop in SIZES[fmt])
RING_SIZES = (89, 90, 91, 257, 511, 512)                                 # 89: the last single band; 90: a second band of one row

IMAGENET = dict(mean=(103.53, 116.28, 123.675), scale=(1 / 57.375, 1 / 57.12, 1 / 58.395))
H, W = 211, 317
INSIDE, EDGE, CORNER, OUTSIDE, INVALID = range(5)

# antialiased cases: (format, crop, aa_max, the factor the case's face must reach), on the AA_HW frame
AA_CASES = (("f32", 171, 8, 8), ("f32", 342, 2, 2), ("f16", 293, 4, 4), ("u8", 511, 8, 2))
AA_HW = (1200, 1200)
AA_SOURCE_PER_CROP = {1: 1.0, 2: 2.0, 4: 3.5, 8: 6.0}                    # source pixels per crop pixel that give the factor: k^2 / 2 < s^2 < 2 k^2
QUALITY_AA_SIZES = (257, 512)                                            # records with aa_max = 2
GATED = ("f32", 257, dict(min_covered=0.5))                              # the gated batch: the packed index meets a 3-row band

# the gallery: (format, crop).  f32 342 and u8 512 have runs of whole 16-byte vectors (a stored shot leaves by copy_vectors), the rest go through LDS
GALLERY = (("f32", 129), ("f32", 342), ("f32", 511), ("f16", 257), ("u8", 512))
FUSED = (("f32", 224), ("f16", 299))                                     # 4 and 6 rows


# ---------------------------------------------------------------------------------------------- the regimes, from the library
def band_rows(rfa, fmt, crop):
    return rfa.debug_face_bands(crop, fbr.FORMAT_OF[fmt])[0]


def ring_rows(rfa, crop):
    return rfa.debug_face_bands(crop, fbr.U8_HWC)[1]


def bands_of(crop, rows):
    """(number of bands, rows of the last band) of a crop walked `rows` at a time"""
    n = (crop + rows - 1) // rows
    return n, crop - (n - 1) * rows


def table_gaps(rfa, sizes, ring_sizes):
    """what a table of sizes lacks, as a list of sentences (empty = the table covers every regime the library reports for CROPS)"""
    gaps = []
    for fmt in FORMATS:
        have = set(sizes.get(fmt, ()))
        rows = {c: band_rows(rfa, fmt, c) for c in CROPS}
        for v in sorted(set(rows.values())):
            first = min(c for c in CROPS if rows[c] == v)
            if first not in have:
                gaps.append(f"{fmt}: band_rows {v} starts at crop {first}, which is not in the table")
        for c in CROPS[1:]:
            if rows[c] != rows[c - 1] and c - 1 not in have:
                gaps.append(f"{fmt}: crop {c - 1}, the last one of band_rows {rows[c - 1]}, is not in the table")
        if CROPS[-1] not in have:
            gaps.append(f"{fmt}: crop {CROPS[-1]} is not in the table")
        if fmt != "u8":
            full = max(rows[c] * c * ES[fmt] for c in CROPS)
            if not any(rows[c] * c * ES[fmt] == full for c in have):
                gaps.append(f"{fmt}: no case fills an LDS run ({full} bytes)")
    short = [(fmt, c) for fmt in FORMATS for c in sizes.get(fmt, ()) if band_rows(rfa, fmt, c) < 8 and c % band_rows(rfa, fmt, c)]
    if not short:
        gaps.append("no case below 8 rows has a last band shorter than the others")
    if not any(c % band_rows(rfa, fmt, c) == 1 for fmt, c in short):
        gaps.append("no case below 8 rows has a last band of a single row")
    ring = {c: ring_rows(rfa, c) for c in CROPS}
    have = set(ring_sizes)
    first = min(c for c in CROPS if ring[c] != c + 2)                    # below it the ring holds the whole crop: one band
    for c, what in ((first - 1, "the last single-band crop"), (first, "the first crop walked in bands"), (CROPS[-1], "the largest crop")):
        if c not in have:
            gaps.append(f"quality: crop {c} ({what}, ring_rows {ring[c]}) is not in the table")
    if not any(bands_of(c, ring[c] - 2)[0] > 1 and bands_of(c, ring[c] - 2)[1] == 1 for c in have):
        gaps.append("quality: no case has a last band of a single row")
    return gaps


def describe(rfa, kernel, fmt, crop, faces):
    """the line every case of the sweep prints"""
    rows = ring_rows(rfa, crop) - 2 if kernel == "quality" else band_rows(rfa, fmt, crop)
    n, last = bands_of(crop, rows)
    return f"{kernel:8s} {fmt:3s} crop {crop:3d}: {rows} rows per band, {n} bands, last band {last} rows, {faces} faces"


# ---------------------------------------------------------------------------------------------- the frame and the faces of a case
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def frame():
    """no zero byte: an uncovered crop pixel is recognisable"""
    return _frozen(np.random.default_rng(11).integers(1, 256, size=(H, W, 3), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def faces(size):
    """five faces whose footprints are 100 to 200 source pixels whatever the crop size: upright inside the frame, turned by 0.6 rad across
    the left edge, across the bottom-right corner, entirely outside, invalid (a NaN landmark)"""
    f = 112.0 / size
    rows = [_template_face(size, 1.25 * f, 0.0, 90.5, 35.25),
            _template_face(size, 1.0 * f, 0.6, 20.0, 30.0),
            _template_face(size, 1.25 * f, 0.0, W - 70.0, H - 80.0),
            _template_face(size, 1.25 * f, 0.0, -5000.0, 40.0)]
    nan = rows[INSIDE].copy()
    nan[8] = np.nan
    return _frozen(np.array(rows + [nan], np.float32))


@functools.lru_cache(maxsize=None)
def aa_frame():
    return _frozen(np.random.default_rng(12).integers(1, 256, size=AA_HW + (3,), dtype=np.uint8))


def aa_face(size, factor):
    """a face inside aa_frame() whose footprint gives supersampling factor `factor` (given aa_max >= factor)"""
    if factor == 1:
        return _template_face(size, AA_SOURCE_PER_CROP[1], -0.3, 500.5, 300.25)
    return _template_face(size, AA_SOURCE_PER_CROP[factor], 0.05, 100.0, 40.0)


def aa_faces(size, factor):
    """the faces of an antialiased case; at factor 8 one more face of factor 1, so that two factors share a launch"""
    rows = [aa_face(size, factor)] + ([aa_face(size, 1)] if factor == 8 else [])
    return np.array(rows, np.float32)


# ---------------------------------------------------------------------------------------------- references, computed once and left unchanged
@functools.lru_cache(maxsize=None)
def ref_crops(size):
    """align_ref.crops of the five faces: ((5, S, S, 3) u8 BGR, (5, 6) matrices)"""
    return tuple(_frozen(a) for a in align_ref.crops(frame(), faces(size), 1.0, size))


@functools.lru_cache(maxsize=None)
def ref_batch(fmt, size):
    """face_batch_ref.batch of the five faces, rgb on, ImageNet mean / scale for the float formats: (tensor, matrices, offsets)"""
    kw = IMAGENET if fmt != "u8" else {}
    return tuple(_frozen(a) for a in fbr.batch([frame()], [faces(size)], fbr.FORMAT_OF[fmt], size=size, rgb=1, **kw))


def batch_kw(fmt):
    return dict(rgb=True, **(IMAGENET if fmt != "u8" else {}))


@functools.lru_cache(maxsize=None)
def ref_aa_batch(fmt, size, aa_max, factor):
    return tuple(_frozen(a) for a in far.batch([aa_frame()], [aa_faces(size, factor)], fbr.FORMAT_OF[fmt], size=size, rgb=1, aa_max=aa_max))


@functools.lru_cache(maxsize=None)
def ref_covered(size):
    """face_quality_ref.covered of the five faces"""
    return tuple(fqr.covered(frame(), f, 1.0, size) for f in faces(size))
