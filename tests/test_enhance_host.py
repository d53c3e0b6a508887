"""Low-light enhancement on the host (no GPU): rf_enhance_host -- the code the kernels run, compiled for the host -- against
tests/enhance_ref.py byte for byte over the edge shapes, tile sizes, clip limits and contents the GPU test uses, the refusals, lit frames
that must come back untouched, the tile count of the half-dark frame, and enhance.h on its own under the address and UB sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import enhance_ref as er
from conftest import ROOT
from retinaface_amd import _lib, enhance_host, enhance_spec

# smaller than a tile, exactly one tile, edge tiles one pixel wide, more than one tile per axis
SHAPES = ((1, 1), (1, 200), (7, 5), (64, 64), (65, 129), (100, 150))
SPECS = (dict(), dict(dark_below=256))


def pitched(frame, pad=13, shift=1):
    """the frame as a view with a row pitch above cols * 3 at an odd base address"""
    rows, cols = frame.shape[:2]
    step = (cols * 3 + pad) | 1
    buf = np.full(rows * step + shift + 8, 0xAB, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[shift:], (rows, cols, 3), (step, 3, 1))
    view[...] = frame
    assert view.ctypes.data % 2 == 1 and step % 2 == 1
    return buf, view


@pytest.mark.parametrize("shape", SHAPES)
def test_enhance_host_equals_the_reference_byte_for_byte(shape):
    for name, frame in er.contents(*shape).items():
        for kw in SPECS:
            want, tiles = er.enhance(frame, **kw)
            got, n = enhance_host(frame, **kw)
            assert n == tiles and np.array_equal(got, want), (shape, name, kw)
            assert (got.astype(int) >= frame).all()                                   # never darker
            if kw:
                assert n == -(-shape[0] // 64) * -(-shape[1] // 64)
    # the 100 x 150 frame as an ROI view: pitch above cols * 3, odd base pointers on both sides; bytes outside the rows stay
    frame = er.contents(*shape)["noise006"]
    sbuf, sview = pitched(frame)
    dbuf, dview = pitched(np.zeros_like(frame), pad=7, shift=3)
    before = dbuf.copy()
    got, n = enhance_host(sview, out=dview)
    want, tiles = er.enhance(frame)
    assert n == tiles and np.array_equal(dview, want) and np.array_equal(sview, frame)
    mask = np.ones(dbuf.shape, bool)
    step = dview.strides[0]
    for y in range(shape[0]):
        mask[3 + y * step:3 + y * step + 3 * shape[1]] = False
    assert np.array_equal(dbuf[mask], before[mask])
    # in place
    same, n2 = enhance_host(sview, out=sview)
    assert n2 == tiles and np.array_equal(sview, want)


@pytest.mark.parametrize("kw", (dict(tile=16), dict(tile=128), dict(tile=32), dict(clip=256), dict(clip=65535), dict(tile=16, dark_below=256),
                                dict(tile=128, dark_below=256, clip=65535), dict(dark_below=1), dict(dark_below=20)))
def test_tile_sizes_clip_limits_and_thresholds(kw):
    for name, frame in er.contents(130, 70, tile=kw.get("tile", 64)).items():
        want, tiles = er.enhance(frame, **kw)
        got, n = enhance_host(frame, **kw)
        assert n == tiles and np.array_equal(got, want), (name, kw)


def test_contents_do_what_they_are_there_for():
    c = er.contents(130, 70)
    assert (er.luma(c["y0"]) == 0).all() and c["y0"].any()
    got, n = enhance_host(c["y0"])
    assert n == 6 and np.array_equal(got, er.enhance(c["y0"])[0])
    # one value per tile: the whole histogram sits in one bin, the clip step redistributes nearly everything
    T, frame = 64, c["per_tile"]
    L, F = er.luts(frame)
    assert F.all() and all(len(np.unique(er.luma(frame)[j * T:(j + 1) * T, i * T:(i + 1) * T])) == 1 for j in range(3) for i in range(2))
    # white and black: p99 decides -- black is dark and is lifted by the redistributed histogram, white is lit
    assert enhance_host(c["white"])[1] == 0 and enhance_host(c["black"])[1] == 6
    # the dark ramp and the dark noise gain contrast: a wider luma range than they came with
    for name in ("ramp", "noise006"):
        got, n = enhance_host(c[name])
        assert n == 6 and np.ptp(er.luma(got)) > 2 * np.ptp(er.luma(c[name])), name


def test_a_lit_frame_comes_back_byte_identical(base_frame):
    frame = np.ascontiguousarray(base_frame[30:478, 440:888])
    L, F = er.luts(frame)
    assert not F.any()
    for kw in (dict(), dict(tile=16, dark_below=8), dict(tile=128)):
        got, n = enhance_host(frame, **kw)
        assert n == er.enhance(frame, **kw)[1]
        if n == 0:
            assert np.array_equal(got, frame)
    got, n = enhance_host(frame)
    assert n == 0 and np.array_equal(got, frame)
    white = np.full((70, 130, 3), 255, np.uint8)
    assert enhance_host(white)[1] == 0 and np.array_equal(enhance_host(white)[0], white)


def test_the_half_dark_frame_counts_its_dark_tiles():
    from retinaface_amd.frames import synth_frames
    frame = synth_frames(448, 448, 1, config=700, faces=[1, 3, 5], background="photo")[0]
    half = er.half_dark(frame)
    want, tiles = er.enhance(half)
    got, n = enhance_host(half)
    L, F = er.luts(half)
    assert n == tiles == int(F.sum()) and np.array_equal(got, want)
    assert F[:, :3].all() and 21 <= n <= 28                      # 7 x 7 tiles: the three dark columns, the straddling one maybe
    assert np.array_equal(got[:, 320:], half[:, 320:]) or F[:, 4:].any()         # beyond the last dark tile's centre nothing changes
    assert er.luma(got[:, :192]).mean() > 4 * er.luma(half[:, :192]).mean()


def test_bad_specs_pitches_and_overlaps_are_refused():
    lib = _lib.load_library()
    frame = er.contents(70, 130)["noise006"]
    out = np.zeros_like(frame)
    tiles = C.c_int(-7)

    def call(sp, src=frame, dst=out, rows=70, cols=130, step=390, dst_step=390):
        return lib.rf_enhance_host(C.byref(sp) if sp is not None else None, src.ctypes.data if src is not None else None, rows, cols, step,
                                   dst.ctypes.data if dst is not None else None, dst_step, C.byref(tiles))
    assert call(None) == 0 and tiles.value == 6 and np.array_equal(out, er.enhance(frame)[0])           # a NULL spec: the defaults
    assert call(enhance_spec()) == 0 and tiles.value == 6
    for field, value in (("struct_size", 12), ("tile", 48), ("tile", 8), ("tile", 256), ("tile", -64), ("clip", 255), ("clip", 65536), ("clip", -1),
                         ("dark_below", 257), ("dark_below", -1)):
        sp = enhance_spec()
        setattr(sp, field, value)
        tiles.value = -7
        assert call(sp) == -1 and tiles.value == -7, (field, value)
    for field, value in (("tile", 16), ("tile", 32), ("tile", 128), ("clip", 256), ("clip", 65535), ("dark_below", 1), ("dark_below", 256)):
        sp = enhance_spec()
        setattr(sp, field, value)
        assert call(sp) == 0, (field, value)
    sp = enhance_spec()
    assert call(sp, step=389) == -1 and call(sp, dst_step=389) == -1 and call(sp, src=None) == -1 and call(sp, dst=None) == -1
    assert call(sp, rows=-1) == -1 and call(sp, rows=0) == 0 and tiles.value == 0
    # the frame itself is the one legal overlap
    buf = np.zeros(70 * 390 + 390, np.uint8)
    a, b = buf[:70 * 390].reshape(70, 130, 3), buf[390:].reshape(70, 130, 3)
    a[...] = frame
    assert call(sp, src=a, dst=b) == -1 and call(sp, src=b, dst=a) == -1 and call(sp, src=a, dst=a, dst_step=393) == -1
    assert call(sp, src=a, dst=a) == 0 and np.array_equal(a, er.enhance(frame)[0])
    with pytest.raises(_lib.RFError):
        enhance_host(frame, tile=48)


def test_enhance_under_address_and_ub_sanitizers(tmp_path):
    """tests/csrc/test_enhance_host.cpp: enhance_host on the edge shapes in exactly-sized heap buffers and the whole domain of the gain's
    division against the plain one, host code only, built with -fsanitize=address,undefined.  No GPU and no library: enhance.h is compiled
    into the program."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")                        # for <hip/hip_runtime.h>, which enhance.h includes
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "test_enhance_host")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "test_enhance_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
