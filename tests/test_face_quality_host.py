"""Face quality, host side (no GPU): rf_face_pose and rf_face_gate_eval -- the code the kernel runs, compiled for the host -- must
equal tests/face_quality_ref.py bit for bit; the restatement itself is pinned on the golden detections of the base frame."""
import ctypes as C

import numpy as np
import pytest

import face_quality_ref as fqr
from conftest import golden
from retinaface_amd import _lib, face_gate, face_gate_eval, face_pose
from test_align_host import _golden_rows

CS = (1.0, 2.5, float(np.float32(1280) / np.float32(448)))


def _bits(v):
    return np.float64(v).tobytes()


def _native_pose(lib, row, cs, size):
    f = _lib.rf_face.from_buffer_copy(np.asarray(row, np.float32).tobytes())
    q = np.full(1, 7, fqr.DTYPE)                                           # whatever was there is overwritten
    st = lib.rf_face_pose(C.byref(f), C.c_float(cs), size, q.ctypes.data_as(C.POINTER(_lib.rf_face_quality)))
    return st, q[0]


def _check_pose(lib, row, cs, size):
    st, q = _native_pose(lib, row, cs, size)
    ok, iod2, yaw, s2 = fqr.pose(row, cs, size)
    assert st == 0 and int(q["flags"]) == (0 if ok else fqr.INVALID)
    for name, want in (("iod2", iod2), ("yaw", yaw), ("sin2_roll", s2)):
        assert _bits(q[name]) == _bits(want), (name, size, cs, q[name], want)
    assert q["covered"] == 0 and q["sum_luma"] == 0 and q["sum_lap"] == 0 and q["sum_lap2"] == 0 and _bits(q["sharpness"]) == _bits(0.0)
    return ok, q


def test_face_pose_equals_the_ref_on_every_golden_detection(built_lib):
    rows = _golden_rows()
    assert len(rows) >= 40
    for size in (16, 112, 512):
        for cs in CS:
            for r in rows:
                ok, q = _check_pose(built_lib, r, cs, size)
                assert ok and q["iod2"] > 0 and abs(q["yaw"]) < 2 and 0 <= q["sin2_roll"] <= 1
    assert _native_pose(built_lib, rows[0], 1.0, 0)[1].tobytes() == _native_pose(built_lib, rows[0], 1.0, 112)[1].tobytes()     # 0 = 112


def test_degenerate_faces(built_lib):
    same = np.zeros(15, np.float32)
    same[5:10], same[10:15] = 100.0, 50.0
    nan = golden("fixture_mnet25.npz")["det"][0].copy()
    nan[7] = np.nan
    for row in (same, nan):
        ok, q = _check_pose(built_lib, row, 1.0, 112)
        assert not ok and q["iod2"] == 0 and q["yaw"] == 0 and q["sin2_roll"] == 0
        # with a gate an invalid face always fails, and its zeros fail what they fail
        assert face_gate_eval(face_gate(max_abs_yaw=0.5), q) == fqr.INVALID
        assert face_gate_eval(face_gate(min_iod=1.0, min_sharpness=1.0), q) == fqr.INVALID | fqr.IOD | fqr.SHARPNESS
        assert face_gate_eval(None, q) == 0
    # coincident eyes, the other points spread: a valid similarity, but iod2 == 0 and yaw is NaN or infinite
    eyes = golden("fixture_mnet25.npz")["det"][0].copy()
    eyes[6], eyes[11] = eyes[5], eyes[10]
    ok, q = _check_pose(built_lib, eyes, 1.0, 112)
    assert ok and q["iod2"] == 0 and not np.isfinite(q["yaw"])
    for gate, want in ((dict(max_abs_yaw=0.5), fqr.YAW), (dict(min_iod=1e-3), fqr.IOD), (dict(max_abs_yaw=100.0, min_iod=1.0), fqr.YAW | fqr.IOD),
                       (dict(max_sin2_roll=0.9), 0)):
        assert fqr.gate_flags(q, gate) == want
        assert face_gate_eval(face_gate(**gate), q) == want


def _rec(**kw):
    q = np.zeros((), fqr.DTYPE)
    q["covered"], q["sum_luma"], q["sharpness"], q["iod2"], q["yaw"], q["sin2_roll"] = 10000, 1500000, 200.0, 1600.0, -0.1, 0.02
    for k, v in kw.items():
        q[k] = v
    return q


def test_gate_eval_equals_the_ref_at_and_around_every_threshold(built_lib):
    f32 = np.float32
    up = lambda v: np.nextafter(np.float64(v), np.inf)       # noqa: E731
    dn = lambda v: np.nextafter(np.float64(v), -np.inf)      # noqa: E731
    size = 112
    area = size * size
    t_sh, t_iod, t_yaw, t_roll, t_cov, t_lo, t_hi = f32(123.456), f32(37.3), f32(0.3), f32(0.11), f32(0.75), f32(90.5), f32(160.25)
    iod_edge = np.float64(t_iod) * np.float64(t_iod)
    cov_edge = int(np.float64(t_cov) * np.float64(area))                   # 0.75 * 12544 = 9408 exactly
    lo_edge, hi_edge = int(np.float64(t_lo) * area), int(np.float64(t_hi) * area)
    assert cov_edge == 9408 and np.float64(lo_edge) == np.float64(t_lo) * area and np.float64(hi_edge) == np.float64(t_hi) * area
    cases = []          # (gate, record, flag, fails)
    for v, fails in ((np.float64(t_sh), False), (dn(t_sh), True), (up(t_sh), False), (np.nan, True)):
        cases.append((dict(min_sharpness=t_sh), _rec(sharpness=v), fqr.SHARPNESS, fails))
    for v, fails in ((iod_edge, False), (dn(iod_edge), True), (up(iod_edge), False)):
        cases.append((dict(min_iod=t_iod), _rec(iod2=v), fqr.IOD, fails))
    for sign in (1.0, -1.0):
        for v, fails in ((np.float64(t_yaw), False), (dn(t_yaw), False), (up(t_yaw), True), (np.inf, True), (np.nan, True)):
            cases.append((dict(max_abs_yaw=t_yaw), _rec(yaw=sign * v), fqr.YAW, fails))
    for v, fails in ((np.float64(t_roll), False), (dn(t_roll), False), (up(t_roll), True), (np.nan, True)):
        cases.append((dict(max_sin2_roll=t_roll), _rec(sin2_roll=v), fqr.ROLL, fails))
    for v, fails in ((cov_edge, False), (cov_edge - 1, True), (cov_edge + 1, False)):     # integers: the neighbours are one count away
        cases.append((dict(min_covered=t_cov), _rec(covered=v), fqr.COVERED, fails))
    for v, fails in ((lo_edge, False), (lo_edge - 1, True), (lo_edge + 1, False)):
        cases.append((dict(min_luma=t_lo), _rec(sum_luma=v), fqr.DARK, fails))
    for v, fails in ((hi_edge, False), (hi_edge - 1, False), (hi_edge + 1, True)):
        cases.append((dict(max_luma=t_hi), _rec(sum_luma=v), fqr.BRIGHT, fails))
    for gate, q, flag, fails in cases:
        want = fqr.gate_flags(q, gate, size)
        assert want == (flag if fails else 0), (gate, q)
        assert face_gate_eval(face_gate(**gate), q, size) == want, (gate, q)
    # all failing bits are set, not only the first
    everything = dict(min_sharpness=t_sh, min_iod=t_iod, max_abs_yaw=t_yaw, max_sin2_roll=t_roll, min_covered=t_cov, min_luma=t_lo,
                      max_luma=t_hi)
    bad = _rec(sharpness=1.0, iod2=4.0, yaw=0.9, sin2_roll=0.5, covered=10, sum_luma=255 * area)
    want = fqr.SHARPNESS | fqr.IOD | fqr.YAW | fqr.ROLL | fqr.COVERED | fqr.BRIGHT
    assert fqr.gate_flags(bad, everything, size) == want == face_gate_eval(everything, bad, size)
    dark = _rec(sum_luma=0)
    assert fqr.gate_flags(dark, everything, size) == fqr.DARK == face_gate_eval(everything, dark, size)
    assert fqr.gate_flags(_rec(), everything, size) == 0 == face_gate_eval(everything, _rec(), size)
    # the area is the crop's: the same record at another crop size
    assert face_gate_eval(dict(min_covered=t_cov), _rec(covered=9000), 96) == 0 == fqr.gate_flags(_rec(covered=9000), dict(min_covered=t_cov), 96)
    assert face_gate_eval(dict(min_covered=t_cov), _rec(covered=9000), 112) == fqr.COVERED


def test_invalid_gates_and_arguments_are_refused(built_lib):
    q = _rec()
    qp = np.array([q]).ctypes.data_as(C.POINTER(_lib.rf_face_quality))
    for field in fqr.GATE_FIELDS:
        for v in (-1.0, -1e-30, float("nan"), float("inf"), -float("inf")):
            g = face_gate(**{field: v})
            assert built_lib.rf_face_gate_eval(C.byref(g), qp, 112) == _lib.RF_ERR_INVALID_ARG, (field, v)
            with pytest.raises(_lib.RFError):
                face_gate_eval(g, q)
    g = face_gate(min_covered=float(np.nextafter(np.float32(1), np.float32(2))))
    assert built_lib.rf_face_gate_eval(C.byref(g), qp, 112) == _lib.RF_ERR_INVALID_ARG
    assert built_lib.rf_face_gate_eval(C.byref(face_gate(min_covered=1.0)), qp, 112) == fqr.COVERED
    for size in (0, -1, 12, 100):
        g = face_gate(min_sharpness=1.0)
        g.struct_size = size
        assert built_lib.rf_face_gate_eval(C.byref(g), qp, 112) == _lib.RF_ERR_INVALID_ARG
    g = face_gate(min_sharpness=1.0)
    for size in (8, 15, 513, -112):
        assert built_lib.rf_face_gate_eval(C.byref(g), qp, size) == _lib.RF_ERR_INVALID_ARG
        assert _native_pose(built_lib, golden("fixture_mnet25.npz")["det"][0], 1.0, size)[0] == _lib.RF_ERR_INVALID_ARG
    assert built_lib.rf_face_gate_eval(C.byref(g), None, 112) == _lib.RF_ERR_INVALID_ARG
    assert built_lib.rf_face_pose(None, 1.0, 112, qp) == _lib.RF_ERR_INVALID_ARG
    assert built_lib.rf_face_gate_eval(None, qp, 112) == 0                 # no gate: every face is kept
    with pytest.raises(TypeError):
        face_gate(min_sharpnes=1.0)
    assert C.sizeof(_lib.rf_face_quality) == 64 == fqr.DTYPE.itemsize and C.sizeof(_lib.rf_face_gate) == 32


# ---------------------------------------------------------------------------------------------- the restatement, pinned
SUMS = {0: (2028871, 880, 2592908), 5: (1969923, 1076, 1001258)}          # (sum_luma, sum_lap, sum_lap2) at S = 112


def test_ref_pins_on_the_base_frame(base_frame):
    det = golden("fixture_mnet25.npz")["det"]
    assert len(det) == 6
    recs = [fqr.quality(base_frame, d, 1.0, 112) for d in det]
    sh = [float(r["sharpness"]) for r in recs]
    yaw = [float(r["yaw"]) for r in recs]
    assert 82.5 < min(sh) < 83.0 and 345.0 < max(sh) < 345.5, sh
    assert -0.355 < min(yaw) < -0.354 and 0.029 < max(yaw) < 0.0291, yaw
    for r in recs:
        assert r["covered"] == 112 * 112 and r["flags"] == 0 and 900 < r["iod2"] < 3000 and 0 <= r["sin2_roll"] < 0.2
    for k, want in SUMS.items():
        assert (int(recs[k]["sum_luma"]), int(recs[k]["sum_lap"]), int(recs[k]["sum_lap2"])) == want
    assert _bits(recs[0]["sharpness"]) == _bits(((110 * 110) * 2592908 - 880 * 880) / (12100.0 * 12100.0))
    # a 5 x 5 box blur of the frame lowers every face's sharpness
    pad = np.pad(base_frame.astype(np.int64), ((2, 2), (2, 2), (0, 0)), mode="edge")
    H, W = base_frame.shape[:2]
    blur = sum(pad[dy:dy + H, dx:dx + W] for dy in range(5) for dx in range(5))
    blur = ((blur + 12) // 25).astype(np.uint8)
    for d, r in zip(det, recs):
        b = fqr.quality(blur, d, 1.0, 112)
        assert b["sharpness"] < r["sharpness"] and b["iod2"] == r["iod2"] and b["yaw"] == r["yaw"]


def test_ref_checkerboard_and_constant_crops():
    board = (((np.arange(64)[:, None] + np.arange(64)[None, :]) & 1) * 255).astype(np.uint8)
    crop = np.repeat(board[:, :, None], 3, axis=2)
    for size, lap, lap2 in ((16, 0, 203918400), (17, -1020, 234090000)):
        sl, sa, sb = fqr.sums(crop[:size, :size])
        assert (sa, sb) == (lap, lap2)
    assert fqr.sums(np.full((20, 20, 3), 255, np.uint8)) == (255 * 400, 0, 0)
    assert fqr.luma(np.array([[[255, 255, 255]], [[0, 0, 255]], [[255, 0, 0]]], np.uint8)).ravel().tolist() == [255, 77, 29]
    assert fqr.sharpness(0, 270608040000, 512) == 1040400.0 and fqr.sharpness(0, 0, 16) == 0.0


def test_python_wrappers(built_lib):
    from retinaface_amd import Detection
    r = golden("fixture_mnet25.npz")["det"][1]
    q = face_pose(r, 2.5, 96)
    ok, iod2, yaw, s2 = fqr.pose(r, 2.5, 96)
    assert ok and _bits(q["iod2"]) == _bits(iod2) and _bits(q["yaw"]) == _bits(yaw) and _bits(q["sin2_roll"]) == _bits(s2)
    d = Detection(float(r[0]), tuple(r[1:5]), tuple(r[5:10]), tuple(r[10:15]), -1)
    assert face_pose(d, 2.5, 96).tobytes() == q.tobytes()
    assert face_gate_eval(dict(max_abs_yaw=0.05), q, 96) == fqr.YAW and face_gate_eval(None, q, 96) == 0


def test_cpp_host_checks_under_sanitizers(built_lib, tmp_path):
    """tests/csrc/test_face_quality.cpp `host`: a stand-alone program with face_quality.h compiled in, under ASan / UBSan -- the
    header's functions against the library's entry points on random faces, gates and sums; every bad gate refused"""
    import os
    import shutil
    import subprocess
    from conftest import ROOT
    from retinaface_amd import lib_path
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    clang = os.path.join(rocm, "llvm", "bin", "clang++")                   # the compiler the library is built with (g++ has no _Float16)
    assert os.path.exists(clang) or shutil.which("clang++"), "no clang++ next to hipcc"
    clang = clang if os.path.exists(clang) else shutil.which("clang++")
    exe, lib_dir = str(tmp_path / "test_face_quality"), os.path.dirname(lib_path())
    subprocess.check_call([clang, "-O1", "-g", "-std=c++17", "-DRF_NO_OPENCV", "-DRF_FACE_QUALITY_HEADER", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"), "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "csrc", "test_face_quality.cpp"),
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert out.returncode == 0 and "ok" in out.stdout, (out.returncode, out.stdout, out.stderr[-2000:])
