"""The band regimes of the face-crop kernels, host side (no GPU): rf_debug_face_bands is the library's own answer for the band height
of a (format, crop) and for the quality kernel's ring.  The table of tests/face_crop_regimes.py must cover every answer it gives over
crop 16..512 -- so a change to kFaceRunBytes, kAlignBandRows or kQualityRingBytes fails here until the table follows -- and the faces
of the recipe must be what tests/test_face_crop_regimes_gpu.py needs them to be, judged on the references alone: a comparison of
zeros with zeros proves nothing."""
import numpy as np
import pytest

import align_ref
import face_aa_ref as far
import face_batch_ref as fbr
import face_crop_regimes as reg
import face_quality_ref as fqr
import retinaface_amd as rfa


# ---------------------------------------------------------------------------------------------- the hook
def test_the_hook_answers_on_the_host_and_refuses_what_the_entry_points_refuse():
    assert rfa.debug_face_bands(112, fbr.F16_CHW) == (8, 73) and rfa.debug_face_bands(512, fbr.F32_CHW) == (2, 16)
    lib = rfa.load_library()
    assert lib.rf_debug_face_bands(112, fbr.U8_HWC, None, None) == 0                         # either pointer may be NULL
    for crop, fmt in ((15, fbr.U8_HWC), (513, fbr.F32_CHW), (0, fbr.F16_CHW), (-1, fbr.F16_CHW), (112, 3), (112, -1)):
        with pytest.raises(rfa.RFError) as e:
            rfa.debug_face_bands(crop, fmt)
        assert e.value.status == -1
    for crop in reg.CROPS:
        rows = [rfa.debug_face_bands(crop, fbr.FORMAT_OF[f]) for f in reg.FORMATS]
        assert len({r[1] for r in rows}) == 1                                                # the ring does not depend on the format
        assert all(1 <= r[0] <= crop and 3 <= r[1] <= crop + 2 for r in rows)
        # a band fits what the kernels reserve for it: 4096 bytes per CHW run, 8 x 512 x 3 for the u8 band, 8192 for the ring
        assert rows[0][0] * crop * 3 <= 8 * 512 * 3 and rows[1][0] * crop * 2 <= 4096 and rows[2][0] * crop * 4 <= 4096
        assert rows[0][1] * crop <= 8192


# ---------------------------------------------------------------------------------------------- the table covers the regimes
def test_the_table_covers_every_regime_the_library_reports():
    gaps = reg.table_gaps(rfa, reg.SIZES, reg.RING_SIZES)
    assert not gaps, gaps
    # the heights the sweep exists for are all there
    for fmt, want in (("f32", {2, 3, 4, 5, 6, 7, 8}), ("f16", {4, 5, 6, 7, 8}), ("u8", {8})):
        assert {reg.band_rows(rfa, fmt, c) for c in reg.SIZES[fmt]} == want, fmt
    assert reg.bands_of(90, reg.ring_rows(rfa, 90) - 2) == (2, 1) and reg.bands_of(89, reg.ring_rows(rfa, 89) - 2) == (1, 89)
    assert reg.bands_of(512, reg.ring_rows(rfa, 512) - 2) == (37, 8) and reg.ring_rows(rfa, 512) - 2 == 14
    # every case the other files take from the table is a size of the entry points
    for fmt, crop in reg.CASES + reg.GALLERY + reg.FUSED + tuple(c[:2] for c in reg.AA_CASES) + (reg.GATED[:2],):
        assert fmt in reg.FORMATS and crop in reg.CROPS
    assert {reg.band_rows(rfa, f, c) for f, c in reg.FUSED} == {4, 6} and reg.band_rows(rfa, *reg.GATED[:2]) == 3
    assert all(reg.band_rows(rfa, f, c) < 8 or f == "u8" for f, c in reg.GALLERY)


def test_a_table_without_one_regime_is_caught_and_the_missing_value_is_named():
    for fmt in ("f32", "f16"):
        heights = {reg.band_rows(rfa, fmt, c) for c in reg.CROPS}
        for v in sorted(heights):
            sizes = dict(reg.SIZES)
            sizes[fmt] = tuple(c for c in reg.SIZES[fmt] if reg.band_rows(rfa, fmt, c) != v)
            gaps = reg.table_gaps(rfa, sizes, reg.RING_SIZES)
            assert any(g.startswith(f"{fmt}: band_rows {v} ") for g in gaps), (fmt, v, gaps)
    for fmt in reg.FORMATS:                                                                   # and without any single size
        for drop in reg.SIZES[fmt]:
            sizes = dict(reg.SIZES)
            sizes[fmt] = tuple(c for c in reg.SIZES[fmt] if c != drop)
            gaps = reg.table_gaps(rfa, sizes, reg.RING_SIZES)
            if (fmt, drop) in (("u8", 17), ("u8", 511), ("f16", 511), ("f32", 511)):       # not a regime boundary: odd sizes next to the limit
                continue
            assert any(f"crop {drop}," in g or f"crop {drop} " in g for g in gaps), (fmt, drop, gaps)
    for drop in (89, 90, 512):
        gaps = reg.table_gaps(rfa, reg.SIZES, tuple(c for c in reg.RING_SIZES if c != drop))
        assert any(f"crop {drop} " in g for g in gaps), (drop, gaps)


# ---------------------------------------------------------------------------------------------- the faces are what the sweep needs
ALL_SIZES = sorted({c for _, c in reg.CASES} | set(reg.RING_SIZES))


@pytest.mark.parametrize("size", ALL_SIZES)
def test_the_five_faces_of_a_case(size):
    frame, faces = reg.frame(), reg.faces(size)
    assert frame.shape == (reg.H, reg.W, 3) and frame.min() >= 1 and len(faces) == 5
    area = size * size
    cov = reg.ref_covered(size)
    assert cov[reg.INSIDE] >= 0.9 * area, (size, cov)
    for k in (reg.EDGE, reg.CORNER):
        assert 0.1 * area <= cov[k] <= 0.9 * area, (size, k, cov)
    assert cov[reg.OUTSIDE] == 0 and cov[reg.INVALID] == 0
    for k in range(4):
        ok, fwd, inv = align_ref.estimate(faces[k], 1.0, size)
        assert ok and fwd.any()                                                               # the outside face too: a valid matrix
        assert 100 <= size / np.hypot(fwd[0], fwd[3]) <= 200                                  # the footprint, in source pixels
    ok, fwd, _ = align_ref.estimate(faces[reg.INVALID], 1.0, size)
    assert not ok and not fwd.any()
    fwd = align_ref.estimate(faces[reg.EDGE], 1.0, size)[1]
    assert abs(np.arctan2(fwd[3], fwd[0]) + 0.6) < 1e-3                                       # the edge face is the turned one


@pytest.mark.parametrize("fmt,size,aa_max,factor", reg.AA_CASES)
def test_the_antialiased_cases_reach_their_factors(fmt, size, aa_max, factor):
    faces = reg.aa_faces(size, factor)
    want = [factor] + ([1] if factor == 8 else [])
    assert [far.aa_factor(f, 1.0, size, aa_max) for f in faces] == want == [rfa.face_aa_factor(f, 1.0, size, aa_max) for f in faces]
    h, w = reg.AA_HW
    assert reg.aa_frame().shape == (h, w, 3) and reg.aa_frame().min() >= 1
    for f in faces:                                                                           # every crop pixel is sampled inside the frame
        assert fqr.covered(np.broadcast_to(np.uint8(1), (h, w, 3)), f, 1.0, size) == size * size


def test_the_quality_cases_under_aa_and_the_gated_batch():
    for size in reg.QUALITY_AA_SIZES:
        assert far.aa_factor(reg.aa_face(size, 2), 1.0, size, 2) == 2
        assert fqr.covered(np.broadcast_to(np.uint8(1), reg.AA_HW + (3,)), reg.aa_face(size, 2), 1.0, size) == size * size
    fmt, size, gate = reg.GATED
    cov = np.array(reg.ref_covered(size)) / (size * size)
    kept = cov >= gate["min_covered"]
    assert kept[reg.INSIDE] and not kept[reg.CORNER] and 1 <= kept.sum() < 5                  # the gate keeps some faces and drops some
    assert np.abs(cov - gate["min_covered"]).min() > 0.01                                     # and no face sits on the threshold
