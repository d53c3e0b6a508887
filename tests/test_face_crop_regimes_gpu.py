"""The face-crop kernels at every band height: align_kernel, face_batch_kernel (plain and antialiased), face_quality_kernel,
shot_keep_kernel and shot_deliver_kernel, byte for byte against the numpy references, at the (format, crop) cases of
tests/face_crop_regimes.py -- bands of 2 to 7 rows, last bands shorter than the others and of a single row, LDS runs that are exactly
full at a non-zero 16-byte phase, the u8 band at its limit, the quality ring on both sides of its transition and at 37 bands, the
gallery in fp32.  The other GPU tests run these kernels at crop 16..128 only, where every band has 8 rows.
tests/test_face_crop_regimes_host.py holds the table and the faces to what this file needs.  Every case prints one line: kernel,
format, crop, rows per band, number of bands, rows of the last band, faces (pytest -s shows them)."""
import numpy as np
import pytest

import face_aa_ref as far
import face_batch_ref as fbr
import face_crop_regimes as reg
import face_quality_ref as fqr
import track_ref as tr
from test_face_batch_gpu import same, want_batch
from test_face_quality_gpu import same_records
from test_gpu_align import engine, rfa, to_device  # noqa: F401  (rfa: fixture)
from test_shot_gpu import NOBODY, Rig, noise
from test_track_host import by_score, face
from test_tta_gpu import odd_view

pytestmark = pytest.mark.gpu

H, W = reg.H, reg.W


def canary(nbytes, phase):
    """a device buffer of 77s and the address `phase` bytes into it: [phase, phase + nbytes) is the destination, the rest must stay 77"""
    import torch
    buf = torch.full((nbytes + 64,), 77, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + phase


def check_canary(buf, phase, want_bytes, what):
    import torch
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    nb = len(want_bytes)
    assert got[phase:phase + nb].tobytes() == want_bytes, what
    assert (got[:phase] == 77).all() and (got[phase + nb:] == 77).all(), what                # nothing before the first face or after the last


# ---------------------------------------------------------------------------------------------- 1. face batches
@pytest.mark.parametrize("fmt,crop", reg.CASES)
def test_face_batch_at_every_band_height(rfa, fmt, crop):
    det = engine(rfa)
    frame, faces = np.array(reg.frame()), reg.faces(crop)                                    # (a writable copy for torch)
    n, es = len(faces), reg.ES[fmt]
    print("\n" + reg.describe(rfa, "batch", fmt, crop, n))
    want_t, want_m, want_o = reg.ref_batch(fmt, crop)
    assert list(want_o) == [0, n] and len(want_t) == n
    kw = reg.batch_kw(fmt)
    dev = to_device([frame])[0]
    # into the host
    _, t, m, off = det.face_batch([dev.data_ptr()], [H], [W], [faces], crop_size=crop, dtype=fmt, capacity=n, **kw)
    assert same(t, want_t), (fmt, crop, int((t != want_t).sum()))
    assert np.array_equal(m.reshape(-1, 6), want_m) and list(off) == [0, n] and not det.faces_truncated
    assert m[reg.OUTSIDE].any() and not m[reg.INVALID].any()
    # into a device buffer one element past a 16-byte boundary: no band starts aligned and the full 4096-byte runs sit at a non-zero
    # phase; the frame as a view at an odd pointer with an odd step
    keep, ptr, step = odd_view(frame)
    buf, d_out = canary(want_t.nbytes, es)
    _, t, m, off = det.face_batch([ptr], [H], [W], [faces], steps=[step], crop_size=crop, dtype=fmt, capacity=n, d_out=d_out, **kw)
    check_canary(buf, es, want_t.tobytes(), (fmt, crop))
    assert same(t, want_t) and np.array_equal(m.reshape(-1, 6), want_m) and list(off) == [0, n]


# ---------------------------------------------------------------------------------------------- 2. alignment
@pytest.mark.parametrize("crop", reg.SIZES["u8"])
def test_align_at_the_band_limits(rfa, crop):
    """512 at phase 3 is the band of exactly kAlignBandBytes next to the end of its LDS block"""
    det = engine(rfa)
    frame, faces = np.array(reg.frame()), reg.faces(crop)                                    # (a writable copy for torch)
    n = len(faces)
    print("\n" + reg.describe(rfa, "align", "u8", crop, n))
    want_c, want_m = reg.ref_crops(crop)
    dev = to_device([frame])[0]
    buf, d_crops = canary(want_c.nbytes, 3)
    crops, mats = det.align([dev.data_ptr()], [H], [W], [faces], crop_size=crop, d_crops=d_crops)
    check_canary(buf, 3, want_c.tobytes(), crop)
    assert np.array_equal(crops[0], want_c) and np.array_equal(mats[0].reshape(-1, 6), want_m)
    assert want_c[reg.INSIDE].all() and not want_c[reg.OUTSIDE].any() and (want_c[reg.CORNER] == 0).any() and want_c[reg.CORNER].any()


# ---------------------------------------------------------------------------------------------- 3. antialiased
@pytest.mark.parametrize("fmt,crop,aa_max,factor", reg.AA_CASES)
def test_antialiased_batch_below_eight_rows(rfa, fmt, crop, aa_max, factor):
    det = engine(rfa)
    frame, faces = np.array(reg.aa_frame()), reg.aa_faces(crop, factor)
    n, es = len(faces), reg.ES[fmt]
    print("\n" + reg.describe(rfa, "batch-aa", fmt, crop, n) + f", factors {[rfa.face_aa_factor(f, 1.0, crop, aa_max) for f in faces]}")
    want_t, want_m, want_o = reg.ref_aa_batch(fmt, crop, aa_max, factor)
    dev = to_device([frame])[0]
    buf, d_out = canary(want_t.nbytes, es)
    _, t, m, off = det.face_batch([dev.data_ptr()], [reg.AA_HW[0]], [reg.AA_HW[1]], [faces], crop_size=crop, dtype=fmt, rgb=True, capacity=n,
                                  d_out=d_out, antialias=True, aa_max=aa_max)
    check_canary(buf, es, want_t.tobytes(), (fmt, crop))
    assert same(t, want_t), (fmt, crop, int((t != want_t).sum()))
    assert np.array_equal(m.reshape(-1, 6), want_m) and list(off) == list(want_o) == [0, n]


# ---------------------------------------------------------------------------------------------- 4. quality
@pytest.mark.parametrize("crop", reg.RING_SIZES)
def test_quality_on_both_sides_of_the_ring_transition(rfa, crop):
    det = engine(rfa)
    frame, faces = np.array(reg.frame()), reg.faces(crop)                                    # (a writable copy for torch)
    print("\n" + reg.describe(rfa, "quality", "u8", crop, len(faces)))
    dev = to_device([frame])[0]
    want = fqr.records([frame], [faces], None, size=crop)
    assert tuple(int(c) for c in want[0]["covered"]) == reg.ref_covered(crop) and want[0]["sum_lap2"][reg.EDGE] > 0
    assert same_records(det.face_quality([dev.data_ptr()], [H], [W], [faces], crop_size=crop), want), crop
    gate = dict(min_covered=0.5, min_sharpness=1.0)
    want = fqr.records([frame], [faces], gate, size=crop)
    assert want[0]["flags"][reg.INSIDE] == 0 and want[0]["flags"][reg.CORNER] & fqr.COVERED and want[0]["flags"][reg.INVALID] & fqr.INVALID
    assert same_records(det.face_quality([dev.data_ptr()], [H], [W], [faces], crop_size=crop, gate=gate), want), crop


@pytest.mark.parametrize("crop", reg.QUALITY_AA_SIZES)
def test_antialiased_quality_in_the_ring_regime(rfa, crop):
    det = engine(rfa)
    frame, faces = np.array(reg.frame()), reg.faces(crop)                                    # (a writable copy for torch)
    print("\n" + reg.describe(rfa, "quality", "u8", crop, len(faces) + 1) + ", aa_max 2")
    dev, big = to_device([frame, np.array(reg.aa_frame())])

    def records_aa(ptr, hw, f):
        """rf_face_quality_device takes no spec: the antialiased records are those of the gated batch call with a NULL gate"""
        return det.face_batch([ptr], [hw[0]], [hw[1]], [f], crop_size=crop, dtype="u8", capacity=len(f), return_quality=True, antialias=True,
                              aa_max=2)[4]

    assert same_records(records_aa(dev.data_ptr(), (H, W), faces), far.records([frame], [faces], None, size=crop, aa_max=2)), crop
    two = np.array([reg.aa_face(crop, 2)], np.float32)                                        # and a face that is supersampled 2 x 2
    want = far.records([reg.aa_frame()], [two], None, size=crop, aa_max=2)
    assert want[0]["covered"][0] == crop * crop
    assert same_records(records_aa(big.data_ptr(), reg.AA_HW, two), want), crop


def test_gated_batch_where_the_packed_index_meets_a_three_row_band(rfa):
    fmt, crop, gate = reg.GATED
    det = engine(rfa)
    frame, faces = np.array(reg.frame()), reg.faces(crop)                                    # (a writable copy for torch)
    n, es = len(faces), reg.ES[fmt]
    print("\n" + reg.describe(rfa, "gated", fmt, crop, n))
    want_t, want_m, want_o, want_q = fqr.gated_batch([frame], [faces], fbr.FORMAT_OF[fmt], gate, size=crop, rgb=1)
    kept = int(want_o[1])
    assert 1 <= kept < n and len(want_t) == kept
    dev = to_device([frame])[0]
    buf, d_out = canary(n * 3 * crop * crop * es, es)
    _, t, m, off, q = det.face_batch([dev.data_ptr()], [H], [W], [faces], crop_size=crop, dtype=fmt, rgb=True, capacity=n, d_out=d_out,
                                     gate=gate, return_quality=True)
    check_canary(buf, es, want_t.tobytes(), (fmt, crop))                                      # nothing beyond the kept faces
    assert list(off) == list(want_o) and same_records(q, want_q)
    assert same(t, want_t) and np.array_equal(m.reshape(-1, 6), want_m)


# ---------------------------------------------------------------------------------------------- 5. the gallery
@pytest.mark.parametrize("fmt,crop", reg.GALLERY)
def test_gallery_below_eight_rows_and_in_fp32(rfa, fmt, crop):
    """Rig.call compares every buffer, the gallery and the twin tracker with shot_ref.  f32 342 and u8 512: runs of whole 16-byte vectors,
    the stored shot leaves by copy_vectors; the others go through LDS."""
    det = engine(rfa)
    print("\n" + reg.describe(rfa, "gallery", fmt, crop, 1))
    frames = [noise(70 + t, 200, 200) for t in range(3)]
    one = lambda score, x: by_score([face(score, x, 20.0, 140.0)])
    spec = dict(max_tracks=4, max_missed=-1)
    rig = Rig(det, 1, spec, fmt, crop)
    try:
        rig.call(frames[0:1], [0], [one(0.5, 30.0)])                                         # born: shot_keep_kernel writes the entry
        rig.call(frames[1:2], [0], [one(0.75, 32.0)])                                        # improves: the entry is rewritten
        shots, info, delivered = rig.call(frames[2:3], [0], [NOBODY])                        # ends: delivered from the stored entry
        want, mat = rig.gal.face_bytes(frames[1], tr.rows_of(one(0.75, 32.0))[0])
        assert delivered.tolist() == [1] and info[0, 0]["frame"] == 1 and info[0, 0]["matrix"].tobytes() == mat.tobytes()
        assert shots[0, 0].tobytes() == want.tobytes() and shots[0, 0].any()
    finally:
        rig.close()
    rig = Rig(det, 1, spec, fmt, crop)
    try:
        shots, info, delivered = rig.call(frames[:2], [0, 0], [one(0.5, 30.0), NOBODY])      # born and ended inside one call: delivered by sampling
        want, mat = rig.gal.face_bytes(frames[0], tr.rows_of(one(0.5, 30.0))[0])
        assert delivered.tolist() == [0, 1] and info[1, 0]["frame"] == 0 and shots[1, 0].tobytes() == want.tobytes() and shots[1, 0].any()
    finally:
        rig.close()


# ---------------------------------------------------------------------------------------------- 6. the fused call (the one forward pass)
@pytest.mark.parametrize("fmt,crop", reg.FUSED)
def test_fused_call_at_four_and_six_rows(rfa, fmt, crop):
    from retinaface_amd.frames import synth_frames
    frames = synth_frames(448, 448, 8, config=1)
    det = engine(rfa)
    dev = to_device(frames)
    dets, t, m, off = det.detect_face_batch_device([d.data_ptr() for d in dev], [448] * 8, [448] * 8, 0.5, dtype=fmt, crop_size=crop, rgb=True,
                                                   capacity=128)
    print("\n" + reg.describe(rfa, "fused", fmt, crop, len(t)))
    assert not det.faces_truncated
    want_t, want_m, want_o = want_batch(frames, dets, fmt, size=crop, rgb=1)
    assert len(t) >= 8 and same(t, want_t) and np.array_equal(m.reshape(-1, 6), want_m) and list(off) == list(want_o)
