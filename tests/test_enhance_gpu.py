"""Low-light detection on the GPU: the two enhance kernels against tests/enhance_ref.py byte for byte (edge shapes, ROI views, tile sizes,
clip limits, contents, in place, batches), the refusals, the fused call against its own parts (rf_enhance_device + rf_detect_batch_device),
the claim (dark frames lose their faces to the plain call and keep them in the enhanced call, as the fp32 oracle says), the multi-device
refusal and the C++ class."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import enhance_ref as er
from conftest import ASSETS, ROOT, STEMS
from test_gpu_align import FP16, FP32, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_tta_gpu import INT8, MD, SPLIT2, SPLIT3, odd_view

pytestmark = pytest.mark.gpu

# 1 x 1, one row, smaller than a tile, exactly one tile, edge tiles one pixel wide, more than one tile per axis
SHAPES = ((1, 1), (1, 200), (7, 5), (64, 64), (65, 129), (100, 150))


@functools.lru_cache(maxsize=None)
def ref(shape, name, tile=0, clip=0, dark_below=0):
    """(frame, enhanced frame, tiles enhanced): computed once and shared: nobody writes to them"""
    frame = er.contents(*shape, tile=tile or 64)[name]
    want, tiles = er.enhance(frame, tile, clip, dark_below)
    return frame, want, tiles


@functools.lru_cache(maxsize=None)
def synth():
    from retinaface_amd.frames import synth_frames
    frames = synth_frames(448, 448, 6, config=700, faces=[1, 3, 5], background="photo")
    for f in frames:
        f.setflags(write=False)
    return tuple(frames)


def canvas(rows, step, shift=0):
    """a destination of rows x step bytes at `shift` bytes into a block of 0xAB"""
    import torch
    buf = torch.full((rows * step + shift + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + shift


def body_of(buf, rows, cols, step, shift=0):
    """(the rows x cols x 3 pixels of a canvas, True when every byte outside them still is 0xAB)"""
    got = buf.cpu().numpy()
    body = got[shift:shift + rows * step].reshape(rows, step)
    clean = (body[:, 3 * cols:] == 0xAB).all() and (got[:shift] == 0xAB).all() and (got[shift + rows * step:] == 0xAB).all()
    return body[:, :3 * cols].reshape(rows, cols, 3), bool(clean)


def check_one(det, frame, want, tiles, **kw):
    """dense -> dense, and an ROI view at an odd pointer with an odd pitch -> a pitched destination at an odd pointer"""
    rows, cols = frame.shape[:2]
    dense = to_device([frame])[0]
    keep, rptr, rstep = odd_view(frame)
    for sptr, sstep, pad, shift in ((dense.data_ptr(), 3 * cols, 0, 0), (rptr, rstep, 7, 1)):
        dstep = 3 * cols + pad
        buf, dptr = canvas(rows, dstep, shift)
        got_tiles = det.enhance_device([sptr], [rows], [cols], [dptr], steps=[sstep], dst_steps=[dstep], **kw)
        got, clean = body_of(buf, rows, cols, dstep, shift)
        assert got_tiles == [tiles], (frame.shape, kw, got_tiles, tiles)
        assert np.array_equal(got, want) and clean, (frame.shape, kw, pad, int((got != want).sum()))
    assert np.array_equal(dense.cpu().numpy(), frame)


# ---------------------------------------------------------------------------------------------- 1. the two kernels on their own
@pytest.mark.parametrize("shape", SHAPES)
def test_enhance_device_equals_the_reference(rfa, shape):
    det = engine(rfa)
    for name in ("black", "white", "per_tile", "ramp", "noise006", "y0", "half"):
        for kw in (dict(), dict(dark_below=256)):
            frame, want, tiles = ref(shape, name, **kw)
            check_one(det, frame, want, tiles, **kw)
    assert ref(shape, "white")[2] == 0 and ref(shape, "black")[2] > 0 and ref(shape, "y0")[0].any()


@pytest.mark.parametrize("kw", (dict(tile=16), dict(tile=128), dict(clip=256), dict(clip=65535), dict(tile=32, dark_below=20),
                                dict(tile=128, dark_below=256, clip=65535)))
def test_tile_sizes_and_clip_limits(rfa, kw):
    det = engine(rfa)
    for name in ("per_tile", "ramp", "noise006", "half", "black"):
        frame, want, tiles = ref((130, 70), name, **kw)
        check_one(det, frame, want, tiles, **kw)


@pytest.mark.parametrize("tile", (16, 64, 128))
def test_a_whole_half_dark_frame_in_place_and_out_of_place(rfa, tile):
    """448 x 448: interior cells (for tile 128, four blocks per cell), lit cells that are plain copies or, in place, nothing at all"""
    det = engine(rfa)
    half = er.half_dark(synth()[1])
    want, tiles = er.enhance(half, tile)
    assert 0 < tiles < (-(-448 // tile)) ** 2
    dev = to_device([half, half])
    buf, dptr = canvas(448, 3 * 448)
    assert det.enhance_device([dev[0].data_ptr()], [448], [448], [dptr], tile=tile) == [tiles]
    got, clean = body_of(buf, 448, 448, 3 * 448)
    assert np.array_equal(got, want) and clean
    assert det.enhance_device([dev[1].data_ptr()], [448], [448], [dev[1].data_ptr()], tile=tile) == [tiles]          # dst == src
    assert np.array_equal(dev[1].cpu().numpy(), want) and np.array_equal(dev[0].cpu().numpy(), half)


def test_batches_of_different_shapes_in_place_and_past_one_launch(rfa):
    det = engine(rfa)
    trio = [ref((65, 129), "noise006"), ref((100, 150), "half"), ref((7, 5), "ramp")]
    dev = to_device([t[0] for t in trio])
    bufs = [canvas(t[0].shape[0], 3 * t[0].shape[1] + 5, 3) for t in trio[:2]]
    rows, cols = [t[0].shape[0] for t in trio], [t[0].shape[1] for t in trio]
    # two frames into pitched destinations, the third in place, an empty frame in between
    tiles = det.enhance_device([dev[0].data_ptr(), 0, dev[1].data_ptr(), dev[2].data_ptr()], [rows[0], 0, rows[1], rows[2]],
                               [cols[0], 0, cols[1], cols[2]], [bufs[0][1], 0, bufs[1][1], dev[2].data_ptr()],
                               dst_steps=[3 * cols[0] + 5, 0, 3 * cols[1] + 5, 3 * cols[2]])
    assert tiles == [trio[0][2], 0, trio[1][2], trio[2][2]]
    for i in range(2):
        got, clean = body_of(bufs[i][0], rows[i], cols[i], 3 * cols[i] + 5, 3)
        assert np.array_equal(got, trio[i][1]) and clean, i
    assert np.array_equal(dev[2].cpu().numpy(), trio[2][1])
    # more frames than one launch carries (sixteen): nineteen frames of three shapes, all in place
    many = [ref(s, n) for s, n in (((64, 64), "noise006"), ((65, 129), "per_tile"), ((1, 200), "ramp"))] * 7
    many = many[:19]
    mdev = to_device([m[0] for m in many])
    ptrs = [d.data_ptr() for d in mdev]
    tiles = det.enhance_device(ptrs, [m[0].shape[0] for m in many], [m[0].shape[1] for m in many], ptrs)
    assert tiles == [m[2] for m in many]
    for d, m in zip(mdev, many):
        assert np.array_equal(d.cpu().numpy(), m[1])


def test_refusals_leave_the_handle_usable(rfa):
    import torch
    det = engine(rfa)
    frame, want, tiles = ref((100, 150), "noise006")
    dev = to_device([frame])[0]
    buf, dptr = canvas(101, 450)

    def good():
        assert det.enhance_device([dev.data_ptr()], [100], [150], [dptr]) == [tiles]
        assert np.array_equal(body_of(buf, 100, 150, 450)[0], want)
    good()
    # bad specs
    cnt = (C.c_int * 1)(-7)
    args = ((C.c_void_p * 1)(dev.data_ptr()), (C.c_int * 1)(100), (C.c_int * 1)(150), (C.c_int * 1)(450), 1, (C.c_void_p * 1)(dptr), (C.c_int * 1)(450), cnt)
    for field, value in (("struct_size", 12), ("tile", 48), ("tile", 256), ("clip", 255), ("clip", 65536), ("dark_below", 257), ("dark_below", -1)):
        sp = rfa.enhance_spec()
        setattr(sp, field, value)
        assert det._lib.rf_enhance_device(det._h, C.byref(sp), *args) == -1 and cnt[0] == -7, field
        good()
    assert det._lib.rf_enhance_device(det._h, None, *args) == 0 and cnt[0] == tiles                # a NULL spec: the defaults
    # a destination that overlaps its source partially (one row down; another pitch), another frame's source, another destination
    two = torch.zeros((202 * 450,), dtype=torch.uint8, device="cuda")
    two[:100 * 450] = dev.view(-1)
    torch.cuda.synchronize()
    p = two.data_ptr()
    for call in (lambda: det.enhance_device([p], [100], [150], [p + 450]),
                 lambda: det.enhance_device([p], [100], [150], [p], dst_steps=[453]),
                 lambda: det.enhance_device([p], [100], [150], [p + 3]),
                 lambda: det.enhance_device([p, dev.data_ptr()], [100, 100], [150, 150], [p + 101 * 450, p + 50 * 450]),
                 lambda: det.enhance_device([p, dev.data_ptr()], [100, 100], [150, 150], [p + 101 * 450, p + 102 * 450]),
                 lambda: det.enhance_device([p], [100], [150], [p + 101 * 450], dst_steps=[449]),
                 lambda: det.enhance_device([p], [100], [150], [p + 101 * 450], steps=[449]),
                 lambda: det.enhance_device([p], [100], [150], [0])):
        with pytest.raises(rfa.RFError) as e:
            call()
        assert e.value.status == -1
        good()
    assert np.array_equal(two[:100 * 450].cpu().numpy(), frame.reshape(-1)) and not two[100 * 450:].any()
    # too many tiles: 192 x 256 = 49152 tiles of 16 pixels per 3072 x 4096 frame, six of them are 294912 > 262144; five are legal
    # (refused before a byte is touched, so one small block stands for the frames)
    with pytest.raises(rfa.RFError) as e:
        det.enhance_device([p] * 6, [3072] * 6, [4096] * 6, [p] * 6, tile=16)
    assert e.value.status == -1 and "262144" in str(e.value)
    good()
    # the fused call refuses the same: a bad spec, copies that would land on the frames
    with pytest.raises(rfa.RFError):
        det.detect_enhanced_device([p], [100], [150], 0.5, tile=48)
    for where in (p, p + 450):
        with pytest.raises(rfa.RFError) as e:
            det.detect_enhanced_device([p], [100], [150], 0.5, enhanced_ptrs=[where])
        assert e.value.status == -1
    good()
    assert np.array_equal(two[:100 * 450].cpu().numpy(), frame.reshape(-1))


# ---------------------------------------------------------------------------------------------- 2. the fused call against its own parts
@pytest.fixture(scope="module")
def three():
    """gain 0.06, half-dark, lit (a frame none of whose tiles is dark), with their reference enhancements"""
    f = synth()
    frames = [er.apply_gain(f[0], 0.06), er.half_dark(f[1]), np.array(f[3])]
    wants = [er.enhance(x) for x in frames]
    assert wants[0][1] == 49 and 21 <= wants[1][1] <= 28 and wants[2][1] == 0 and np.array_equal(wants[2][0], frames[2])
    return frames, [w[0] for w in wants], [w[1] for w in wants]


def as_bytes(res):
    return [rows_of(r).tobytes() for r in res]


@pytest.mark.parametrize("prec,kw", ((FP16, {}), (FP16, SPLIT2), (FP16, SPLIT3), (INT8, {})))
def test_fused_call_equals_detection_of_the_enhanced_frames(rfa, three, prec, kw):
    import torch
    det = engine(rfa, prec=prec, **kw)
    frames, wants, tiles = three
    n, hw = 3, [448] * 3
    dev = to_device(frames)
    ptrs = [d.data_ptr() for d in dev]
    # the parts: rf_enhance_device into dense buffers, rf_detect_batch_device over them
    enh = [torch.zeros_like(d) for d in dev]
    torch.cuda.synchronize()
    eptrs = [e.data_ptr() for e in enh]
    assert det.enhance_device(ptrs, hw, hw, eptrs) == tiles
    for e, w in zip(enh, wants):
        assert np.array_equal(e.cpu().numpy(), w)
    want = det.detect_device(eptrs, hw, hw, 0.5)
    assert not det.truncated and sum(len(w) for w in want) >= 3
    # the fused call: into the caller's buffers, then into the engine's block
    mine = [torch.zeros_like(d) for d in dev]
    torch.cuda.synchronize()
    got = det.detect_enhanced_device(ptrs, hw, hw, 0.5, enhanced_ptrs=[m.data_ptr() for m in mine])
    assert got == want and as_bytes(got) == as_bytes(want) and det.tiles_enhanced == tiles and not det.truncated
    for m, w, d, f in zip(mine, wants, dev, frames):
        assert np.array_equal(m.cpu().numpy(), w) and np.array_equal(d.cpu().numpy(), f)         # the copies; the frames are unchanged
    for _ in range(2):
        again = det.detect_enhanced_device(ptrs, hw, hw, 0.5)
        assert again == want and det.tiles_enhanced == tiles
    # the lit frame: no tile touched, so its result is the plain call's on the frame itself
    if det.tiles_enhanced[2] == 0:
        assert det.detect_device(eptrs[:2] + ptrs[2:], hw, hw, 0.5)[2] == got[2]
    plain = det.detect_device(ptrs, hw, hw, 0.5)
    print("faces, plain call:", [len(p) for p in plain], "enhanced call:", [len(g) for g in got], "tiles:", tiles)
    # the host twin: uploaded once, densely; with and without a place for the copies; an empty frame in between
    host = det.detect_enhanced(frames, 0.5)
    assert host == want and det.tiles_enhanced == tiles
    for m in mine:
        m.zero_()
    torch.cuda.synchronize()
    host = det.detect_enhanced([frames[0], None, frames[1]], 0.5, enhanced_ptrs=[mine[0].data_ptr(), 0, mine[1].data_ptr()])
    assert det.tiles_enhanced == [tiles[0], 0, tiles[1]] and host[1] == []
    assert np.array_equal(mine[0].cpu().numpy(), wants[0]) and np.array_equal(mine[1].cpu().numpy(), wants[1])
    parts = det.detect_device([eptrs[0], 0, eptrs[1]], [448, 0, 448], [448, 0, 448], 0.5)
    assert host == parts
    # nine frames: with SPLIT2 / SPLIT3 the call crosses launches and lanes, and every launch waits for the enhance kernels
    nine = det.detect_enhanced_device(ptrs * 3, hw * 3, hw * 3, 0.5)
    assert nine == det.detect_device(eptrs * 3, hw * 3, hw * 3, 0.5) and det.tiles_enhanced == tiles * 3
    # another spec; a pitched ROI source
    alt = dict(tile=32, clip=4096, dark_below=100)
    assert det.enhance_device(ptrs, hw, hw, eptrs, **alt) == [er.enhance(f, **alt)[1] for f in frames]
    keep, rptr, rstep = odd_view(frames[0])
    got = det.detect_enhanced_device([rptr] + ptrs[1:], hw, hw, 0.5, steps=[rstep, 1344, 1344], **alt)
    assert got == det.detect_device(eptrs, hw, hw, 0.5)
    # the ordinary call is what it was
    assert det.detect_device(ptrs, hw, hw, 0.5) == plain


# ---------------------------------------------------------------------------------------------- 3. the claim
@pytest.mark.parametrize("stem", STEMS)
def test_dark_frames_keep_their_faces(rfa, oracles, stem):
    """fp32 engine, the six frames at gain 0.03 and half-dark, default spec: the enhanced call finds as many faces as the fp32 oracle
    finds in the reference's enhanced frames (the CPU measurement: 13 for both models and both transforms), and strictly more than the
    plain call finds in the dark frames (there: 0 and 8)."""
    det = engine(rfa, stem=stem, prec=FP32)
    for name, dark in (("gain 0.03", [er.apply_gain(f, 0.03) for f in synth()]), ("half-dark", [er.half_dark(f) for f in synth()])):
        enhanced = [er.enhance(f) for f in dark]
        oracle = sum(len(oracles[stem].detect(e[0], 0.5, 0.4, net_hw=(448, 448)).detections) for e in enhanced)
        got = det.detect_enhanced(dark, 0.5)
        plain = det.detectBatchImages(dark, 0.5)
        total, before = sum(len(g) for g in got), sum(len(p) for p in plain)
        print(stem, name, "oracle on enhanced:", oracle, "enhanced call:", total, "plain call:", before, "tiles:", det.tiles_enhanced)
        assert det.tiles_enhanced == [e[1] for e in enhanced]
        assert total == oracle, (stem, name)
        assert total > before, (stem, name)


# ---------------------------------------------------------------------------------------------- 4. multi-device, the C++ class
def test_multi_device_handles_refuse_enhancement(rfa, crop448):
    det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", devices=[0, 0])
    try:
        dev = to_device([crop448, crop448])
        a, b = dev[0].data_ptr(), dev[1].data_ptr()
        for call in (lambda: det.enhance_device([a], [448], [448], [b]), lambda: det.detect_enhanced_device([a], [448], [448], 0.5),
                     lambda: det.detect_enhanced([crop448], 0.5)):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -5
        assert len(det.detect_device([a], [448], [448], 0.5)[0]) >= 1
    finally:
        det.close()


def test_cpp_class_detect_enhanced(rfa, three, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_enhance.cpp")
    exe = str(tmp_path / "test_enhance")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    raw, out = str(tmp_path / "frame.raw"), str(tmp_path / "out.bin")
    frame = three[0][1]
    frame.tofile(raw)
    det = engine(rfa)
    for tile, clip, dark in ((0, 0, 0), (32, 4096, 100)):
        r = subprocess.run([exe, ASSETS, "mnet25", "448", "448", raw, "448", "448", "0.5", str(tile), str(clip), str(dark), out],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        blob = open(out, "rb").read()
        assert int(np.frombuffer(blob, np.int32, 1)[0]) == 3
        want = det.detect_enhanced([frame, None, frame], 0.5, tile=tile, clip=clip, dark_below=dark)
        pos = 4
        for i in range(3):
            k = int(np.frombuffer(blob, np.int32, 1, pos)[0])
            faces = np.frombuffer(blob, np.float32, k * 15, pos + 4).reshape(k, 15)
            tiles = int(np.frombuffer(blob, np.int32, 1, pos + 4 + 60 * k)[0])
            pos += 8 + 60 * k
            assert faces.tobytes() == rows_of(want[i]).tobytes() and tiles == det.tiles_enhanced[i], i
            assert k == (0 if i == 1 else len(want[0]))
        assert pos == len(blob) and det.tiles_enhanced[0] == er.enhance(frame, tile, clip, dark)[1] > 0
