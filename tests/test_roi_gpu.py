"""Region detection on the GPU: the atlas kernel against tests/roi_ref.py byte for byte, the fused call against its own parts (ONE
rf_detect_batch_device call over the reference's atlas views + the reference's face rule and merge), the stand-alone merge against
rf_roi_merge_host, calls of more than 24 passes between tiled and fisheye calls on a handle that splits its launches, the refusals, and
the C++ class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import roi_ref as rr
from conftest import ASSETS, ROOT
from test_dewarp_host import RING
from test_gpu_align import FP16, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_roi_host import LEVELS, edge_rois, pass_faces, scattered_faces
from test_tta_gpu import MD, NET, NMS, SPLIT3, odd_view
from tile_ref import frame_scale

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- 1. the atlas kernel
@pytest.mark.parametrize("view", ((32, 16, 2), (64, 48, 4), (448, 448, 1), (448, 448, 2), (448, 448, 4)))
def test_atlas_device_equals_the_reference(rfa, view):
    """every level, regions over the edges and wholly outside, a pitched source at an odd address, a dense and a pitched destination at
    an odd address, guard bytes around the destination; 97 x 131 is no multiple of 4 (the clamped box mean)"""
    import torch
    det = engine(rfa)
    vw, vh, grid = view
    for rows, cols in ((96, 128), (97, 131)):
        rng = np.random.default_rng(rows * 1000 + cols)
        frame = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        rois = edge_rois(rows, cols, vw // grid)
        if vw == 448:
            rois = rois[:9] + rois[9::2] + rois[-1:]           # fewer passes of the large views: every level still, and the cropped one
        want = rr.atlas(frame, rois, vw, vh, grid, 4)
        assert set(rr.plan(rois, vw, vh, grid, 4)[:, 4].tolist()) == set(LEVELS)
        P = len(want)
        dense = to_device([frame])[0]
        keep, rptr, rstep = odd_view(frame)
        for sptr, sstep, pad, shift in ((dense.data_ptr(), 3 * cols, 0, 0), (rptr, rstep, 7, 1)):
            dstep = 3 * vw + pad
            dst = torch.full((P * vh * dstep + 8,), 0xAB, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            det.roi_atlas_device(sptr, rows, cols, rois, dst.data_ptr() + shift, vw, vh, step=sstep, dst_step=dstep, grid=grid, max_zoom=4)
            got = dst.cpu().numpy()
            body = got[shift:shift + P * vh * dstep].reshape(P * vh, dstep)
            assert np.array_equal(body[:, :3 * vw].reshape(P, vh, vw, 3), want), (view, rows, cols, pad, shift)
            assert (body[:, 3 * vw:] == 0xAB).all() and (got[:shift] == 0xAB).all() and (got[shift + P * vh * dstep:] == 0xAB).all()
        assert np.array_equal(rfa.roi_atlas_host(frame, rois, vw, vh, grid, 4), want)


def test_atlas_device_stages_whole_tiles_of_the_shrunk_levels(rfa):
    """x1/2 and x1/4 cells of 224 and 448 px: whole 64 x 16 tiles whose source box (128 x 32, 256 x 64 px) lies inside the 300 x 640 frame
    go through the staged path, those that touch its border (the first and last column and row included: boxes that start at pixel 0
    or end at the last) through the gather path with its clamp -- side by side in one cell; a dense source and a pitched one at an odd
    address, where every source row has another alignment"""
    import torch
    det = engine(rfa)
    rows, cols = 300, 640
    frame = np.random.default_rng(300640).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    dense = to_device([frame])[0]
    keep, rptr, rstep = odd_view(frame)
    for grid, rois in ((2, [(20, 10, 600, 280), (100, 40, 400, 200), (0, 0, 448, 224), (192, 76, 448, 224)]),
                       (1, [(-64, -30, 896, 360), (1, 22, 638, 256), (0, 0, 1792, 300), (100, 40, 1000, 200)])):
        want = rr.atlas(frame, rois, NET, NET, grid, 1)
        assert set(rr.plan(rois, NET, NET, grid, 1)[:, 4].tolist()) == {-1, -2}
        P = len(want)
        for sptr, sstep in ((dense.data_ptr(), 3 * cols), (rptr, rstep)):
            dst = torch.full((P * NET * NET * 3 + 8,), 0xAB, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            det.roi_atlas_device(sptr, rows, cols, rois, dst.data_ptr(), NET, NET, step=sstep, grid=grid, max_zoom=1)
            got = dst.cpu().numpy()
            assert np.array_equal(got[:P * NET * NET * 3].reshape(P, NET, NET, 3), want), (grid, sstep)
            assert (got[P * NET * NET * 3:] == 0xAB).all()


# ---------------------------------------------------------------------------------------------- 2. the stand-alone merge
def test_merge_device_equals_the_host_merge(rfa):
    det = engine(rfa)
    assert det.max_detections == MD
    lists = []
    for seed, want in ((1, 0), (2, 1), (3, 16), (4, 17), (5, 40)):
        rois = rfa.rois_from_faces(scattered_faces(seed, want, 900))
        lists.append(rois + rois[:1] if rois else rois)             # two equal regions: their centre faces merge
    for grid, vote, mf, cap in ((4, False, 0, None), (4, True, 0, None), (2, False, 7, None), (1, True, 0, 5)):
        frames = [pass_faces(r, 20 + i, 4, grid) for i, r in enumerate(lists)]
        got, votes, src = det.roi_merge([600] * 5, [700] * 5, lists, frames, grid=grid, vote=vote, max_faces=mf, cap_per_image=cap,
                                        return_src_roi=True)
        limit = min(mf or MD, cap if cap is not None else MD)
        for i, (rois, passes) in enumerate(zip(lists, frames)):
            want = rfa.roi_merge_host(passes, rois, NET, NET, NMS, MD, grid, 0, vote, mf, cap)
            ref = rr.merge(rois, passes, NET, NET, NMS, MD, grid, 0, vote, mf)
            assert det.roi_counts[i] == want[1] == ref[1], (grid, i)
            assert rows_of(got[i]).tobytes() == want[0].tobytes() == ref[0][:limit].tobytes(), (grid, i)
            assert list(votes[i]) == list(want[2]) and list(src[i]) == list(want[3]), (grid, i)
        assert det.truncated == any(c > limit for c in det.roi_counts)
        assert det.roi_counts[0] == 0 and det.roi_counts[4] > 30
    again = det.roi_merge([600] * 5, [700] * 5, lists, frames, grid=1, vote=True, cap_per_image=5, return_src_roi=True)
    assert again[0] == got and all(np.array_equal(a, b) for a, b in zip(again[2], src))      # the counters re-armed, no order leaks


# ---------------------------------------------------------------------------------------------- 3. fused call against its own parts
@pytest.fixture(scope="module")
def scene(rfa, base_frame):
    """the 896 x 1280 base frame, a 200 x 240 window of it around its first face, and the regions of the base frame's own faces"""
    det = engine(rfa)
    faces = rows_of(det.detect(base_frame, 0.5))                     # the plain call: net pixels, the frame shrunk by frame_scale
    assert len(faces) >= 4
    scale = float(frame_scale(896, 1280, NET, NET))
    x, y = int(faces[0][1] * scale), int(faces[0][2] * scale)
    x, y = min(max(x - 40, 0), 1280 - 240), min(max(y - 20, 0), 896 - 200)
    small = np.ascontiguousarray(base_frame[y:y + 200, x:x + 240])
    return base_frame, small, rfa.rois_from_faces(faces, scale)


def regions(frame, own, count):
    """`count` regions of a frame: its own faces' first, then windows of many sizes walking over it and over its edges"""
    rows, cols = frame.shape[:2]
    out = list(own)[:count]
    sizes = ((90, 110), (200, 220), (56, 56), (20, 28), (300, 260), (112, 112), (440, 400), (130, 170))
    k = 0
    while len(out) < count:
        w, h = sizes[k % len(sizes)]
        out.append(((k * 173) % (cols + 60) - 50, (k * 97) % (rows + 40) - 30, w, h))
        k += 1
    return out


_views = {}


def ref_views(frame, rois, grid, max_zoom):
    key = (frame.shape, tuple(rois), grid, max_zoom)
    if key not in _views:
        _views[key] = rr.atlas(frame, rois, NET, NET, grid, max_zoom)
    return _views[key]


def parts_of_call(det, frames, lists, thr=0.5, grid=0, max_zoom=0, vote=False, max_faces=0):
    """rr.merge, per frame, over what ONE rf_detect_batch_device call returns for the reference's atlas views of all frames in call
    order -- the call the engine itself makes (a None frame keeps its passes, empty)"""
    views, per_frame = [], []
    for f, rois in zip(frames, lists):
        P = rr.passes_of(len(rois), grid)
        per_frame.append(P)
        views += [None] * P if f is None else list(ref_views(f, rois, grid, max_zoom))
    live = to_device([v for v in views if v is not None])
    ptrs, at = [], 0
    for v in views:
        ptrs.append(0 if v is None else live[at].data_ptr())
        at += v is not None
    res = det.detect_device(ptrs, [NET if p else 0 for p in ptrs], [NET if p else 0 for p in ptrs], thr) if ptrs else []
    assert not det.truncated
    out, q = [], 0
    for f, rois, P in zip(frames, lists, per_frame):
        passes = [rows_of(x) for x in res[q:q + P]]
        q += P
        out.append(rr.merge(rois, passes, NET, NET, NMS, det.max_detections, grid, max_zoom, vote, max_faces) if f is not None else None)
    return out, views


def check_frame(det, got, votes, src, i, want):
    if want is None:
        assert got[i] == [] and det.roi_counts[i] == 0
        return
    assert det.roi_counts[i] == want[1] and rows_of(got[i]).tobytes() == want[0].tobytes(), (i, det.roi_counts[i], want[1])
    assert list(votes[i]) == list(want[2]) and list(src[i]) == list(want[3]), i


def run_and_check(det, frames, dev, lists, thr=0.5, views_ptr=None, **kw):
    want, views = parts_of_call(det, frames, lists, thr, **kw)
    ptrs = [d.data_ptr() if d is not None else 0 for d in dev]
    shapes = [f.shape if f is not None else (0, 0) for f in frames]
    got, votes, src = det.detect_rois_device(ptrs, [s[0] for s in shapes], [s[1] for s in shapes], lists, thr, views_ptr=views_ptr,
                                             return_src_roi=True, **kw)
    assert not det.truncated
    for i in range(len(frames)):
        check_frame(det, got, votes, src, i, want[i])
    return got, votes, src, views


@pytest.mark.parametrize("stem", ("mnet25", "mnet-deconv-0517"))
def test_fused_call_equals_the_merge_of_its_own_views(rfa, scene, stem):
    import torch
    det = engine(rfa, stem=stem)
    big, small, own = scene
    crop = to_device([np.ascontiguousarray(big[30:478, 440:888])])[0]
    plain = det.detect_device([crop.data_ptr()], [448], [448], 0.5)
    # eight frames with different region counts: 0, 1, 16 and 17 on either frame size, a NULL frame that has regions
    frames = [small, big, None, big, small, big, small, big]
    counts = [0, 1, 16, 17, 16, 16, 17, 3]
    lists = [regions(f if f is not None else big, own if f is big else [], c) for f, c in zip(frames, counts)]
    dev = [to_device([f])[0] if f is not None else None for f in frames]
    P = sum(rr.passes_of(c) for c in counts)
    views = torch.full((P * NET * NET * 3,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    got, votes, src, ref = run_and_check(det, frames, dev, lists, views_ptr=views.data_ptr())
    assert sum(len(g) for g in got) >= 6 and got[0] == [] and got[2] == []
    assert len(got[3]) >= 4 and len({int(s) for s in src[3]}) >= 4  # the base frame's own faces, from regions of their own
    have = views.cpu().numpy().reshape(P, NET, NET, 3)
    for q, v in enumerate(ref):                                     # d_views: the reference's views; a NULL frame's are untouched
        assert np.array_equal(have[q], v) if v is not None else (have[q] == 0xAB).all(), q
    # repeats give identical bytes, with the engine's own view block too
    again = run_and_check(det, frames, dev, lists)
    assert again[0] == got and all(np.array_equal(a, b) for a, b in zip(again[2], src))
    # vote on, other grids and zooms
    run_and_check(det, frames[:4], dev[:4], lists[:4], vote=True)
    run_and_check(det, [big, small], [dev[1], dev[0]], [lists[3], lists[4][:5]], grid=2, max_zoom=4)
    run_and_check(det, [small], [dev[0]], [lists[4][:3]], grid=1, max_zoom=1)
    # no frame has a region: no pass, no faces
    none = det.detect_rois_device([dev[0].data_ptr(), dev[1].data_ptr()], [200, 896], [240, 1280], [[], []], 0.5)
    assert none == [[], []] and det.roi_counts == [0, 0] and not det.truncated
    # a cap that cuts
    full = got[3]
    cut = det.detect_rois_device([dev[3].data_ptr()], [896], [1280], [lists[3]], 0.5, max_faces=2)
    assert det.truncated and det.roi_counts == [len(full)] and cut[0] == full[:2] and len(full) > 2
    cnt, out = (C.c_int * 1)(), (rfa._lib.rf_face * 2)()
    arr = (rfa._lib.rf_roi * 17)(*[rfa._lib.rf_roi(*r) for r in lists[3]])
    st = det._lib.rf_detect_roi_batch_device(det._h, (C.c_void_p * 1)(dev[3].data_ptr()), (C.c_int * 1)(896), (C.c_int * 1)(1280), None, 1, arr,
                                             (C.c_int * 1)(17), 0.5, None, out, 2, cnt, None, None, None)
    assert st == -6 and cnt[0] == len(full)                         # RF_ERR_TRUNCATED by cap_per_image, a NULL spec and NULL steps
    # a pitched device frame at an odd pointer; pinned host memory as a device frame
    keep, rptr, rstep = odd_view(small)
    pinned = torch.from_numpy(big).pin_memory()
    pgot = det.detect_rois_device([rptr, pinned.data_ptr()], [200, 896], [240, 1280], [lists[4], lists[3]], 0.5, steps=[rstep, 3 * 1280],
                                  return_src_roi=True)
    pwant = parts_of_call(det, [small, big], [lists[4], lists[3]])[0]
    for i in range(2):
        check_frame(det, pgot[0], pgot[1], pgot[2], i, pwant[i])
    # host frames: uploaded once, densely; an empty frame in between; a frame with a row pitch
    wide = np.zeros((200, 260, 3), np.uint8)
    wide[:, :240] = small
    hframes = [big, None, wide[:, :240]]
    hgot, hvotes, hsrc = det.detect_rois(hframes, [lists[3], lists[2], lists[4]], 0.5, return_src_roi=True)
    hwant = parts_of_call(det, [big, None, small], [lists[3], lists[2], lists[4]])[0]
    for i in range(3):
        check_frame(det, hgot, hvotes, hsrc, i, hwant[i])
    assert det.detect_device([crop.data_ptr()], [448], [448], 0.5) == plain


# ---------------------------------------------------------------------------------------------- 4. more than 24 passes, shared blocks
def test_thirty_passes_between_tiled_and_fisheye_calls(rfa, scene, base_frame):
    """one SPLIT3 handle (launches of eight over three lanes): a region call of 30 passes (grid 1) between a tiled and a fisheye call;
    each returns the bytes a fresh handle returns for it, and the region call those of its own parts"""
    big, small, own = scene
    lists = [regions(small, [], 30)]
    dev = to_device([small, np.ascontiguousarray(base_frame[:600, :700]), np.ascontiguousarray(np.pad(base_frame, ((0, 128), (0, 0), (0, 0)))[:1024, :1024])])
    mesh = rfa.dewarp_plan(rfa.dewarp_spec(**RING), 448, 448)
    calls = (lambda d, dw: d.detect_tiled_device([dev[1].data_ptr()], [600], [700], 0.5, return_tiles=True),
             lambda d, dw: d.detect_rois_device([dev[0].data_ptr()], [200], [240], lists, 0.5, grid=1, return_src_roi=True),
             lambda d, dw: d.detect_dewarped_device([dev[2].data_ptr()], dw, 0.5, return_votes=True))
    fresh = []
    for call in calls:
        det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", **SPLIT3)
        try:
            fresh.append(call(det, det.dewarper(1024, 1024, mesh=mesh)))
        finally:
            det.close()
    det = engine(rfa, **SPLIT3)
    assert det.max_batch == 8 and det.num_slots() == 3
    dw = det.dewarper(1024, 1024, mesh=mesh)
    for _ in range(2):
        for call, want in zip(calls, fresh):
            got = call(det, dw)
            assert got[0] == want[0] and all(np.array_equal(a, b) for x, y in zip(got[1:], want[1:]) for a, b in zip(x, y))
    dw.close()
    assert rr.passes_of(30, 1) == 30
    run_and_check(det, [small], dev[:1], lists, grid=1)


# ---------------------------------------------------------------------------------------------- 5. refusals, multi-device
def test_refusals_leave_the_handle_usable(rfa, scene):
    det = engine(rfa)
    big, small, own = scene
    dev = to_device([small])[0]
    lists = [regions(small, [], 5)]
    before = det.detect_rois_device([dev.data_ptr()], [200], [240], lists, 0.5, return_src_roi=True)
    crop = to_device([np.ascontiguousarray(big[30:478, 440:888])])[0]
    plain = det.detect_device([crop.data_ptr()], [448], [448], 0.5)

    def usable():
        got = det.detect_rois_device([dev.data_ptr()], [200], [240], lists, 0.5, return_src_roi=True)
        assert got[0] == before[0] and all(np.array_equal(a, b) for a, b in zip(got[2], before[2]))
        assert det.detect_device([crop.data_ptr()], [448], [448], 0.5) == plain
    for bad in (dict(max_faces=4097), dict(max_faces=-1), dict(grid=3), dict(grid=-1), dict(max_zoom=3), dict(max_zoom=8)):
        for call in (lambda: det.detect_rois_device([dev.data_ptr()], [200], [240], lists, 0.5, **bad), lambda: det.detect_rois([small], lists, 0.5, **bad)):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1, bad
    for rois in ([(0, 0, 0, 5)], [(0, 0, 5, 16385)], [((1 << 20) + 1, 0, 5, 5)], [(0, 0, 8, 8)] * 257):
        for call in (lambda: det.detect_rois_device([dev.data_ptr()], [200], [240], [rois], 0.5), lambda: det.detect_rois([small], [rois], 0.5),
                     lambda: det.roi_merge([200], [240], [rois], [[[]] * rr.passes_of(len(rois))]),
                     lambda: det.roi_atlas_device(dev.data_ptr(), 200, 240, rois, crop.data_ptr(), 448, 448)):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1
    usable()
    lib = det._lib
    arr = (rfa._lib.rf_roi * 5)(*[rfa._lib.rf_roi(*r) for r in lists[0]])
    cnt, out = (C.c_int * 1)(), (rfa._lib.rf_face * MD)()
    args = (det._h, (C.c_void_p * 1)(dev.data_ptr()), (C.c_int * 1)(200), (C.c_int * 1)(240), (C.c_int * 1)(720), 1, arr, (C.c_int * 1)(5), 0.5)
    tail = (out, MD, cnt, None, None, None)
    for field, value in (("struct_size", 20), ("vote", 3), ("vote", -1), ("reserved", 1)):
        sp = rfa.roi_spec()
        setattr(sp, field, value)
        assert lib.rf_detect_roi_batch_device(*args, C.byref(sp), *tail) == -1, field
    assert lib.rf_detect_roi_batch_device(*args, None, None, MD, cnt, None, None, None) == -1                       # out is null
    assert lib.rf_detect_roi_batch_device(*args[:7], None, 0.5, None, *tail) == -1                                  # roi_counts is null
    assert lib.rf_detect_roi_batch_device(*args[:6], None, (C.c_int * 1)(5), 0.5, None, *tail) == -1                # rois is null
    assert lib.rf_detect_roi_batch_device(*args[:4], (C.c_int * 1)(719), *args[5:], None, *tail) == -1               # a short step
    assert lib.rf_detect_roi_batch_device(*args, None, *tail) == 0 and cnt[0] == len(before[0][0])                  # a NULL spec: the defaults
    usable()
    # the kernel's own refusals
    for kw in (dict(view_w=450), dict(view_w=56), dict(step=719), dict(dst_step=3 * 448 - 1), dict(grid=3), dict(rows=0)):
        a = dict(rows=200, view_w=448)
        a.update(kw)
        with pytest.raises(rfa.RFError) as e:
            det.roi_atlas_device(dev.data_ptr(), a["rows"], 240, lists[0], crop.data_ptr(), a["view_w"], 448, step=a.get("step"),
                                 dst_step=a.get("dst_step"), grid=a.get("grid", 0))
        assert e.value.status == -1, kw
    with pytest.raises(rfa.RFError):
        det.roi_atlas_device(dev.data_ptr(), 200, 240, lists[0], 0, 448, 448)
    with pytest.raises(rfa.RFError):
        det.roi_atlas_device(0, 200, 240, lists[0], crop.data_ptr(), 448, 448)
    usable()


def test_multi_device_handles_refuse_region_detection(rfa, crop448):
    det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", devices=[0, 0])
    try:
        dev = to_device([crop448])[0]
        for call in (lambda: det.detect_rois([crop448], [[(0, 0, 100, 100)]], 0.5),
                     lambda: det.detect_rois_device([dev.data_ptr()], [448], [448], [[(0, 0, 100, 100)]], 0.5),
                     lambda: det.roi_merge([448], [448], [[(0, 0, 100, 100)]], [[[]]]),
                     lambda: det.roi_atlas_device(dev.data_ptr(), 448, 448, [(0, 0, 100, 100)], dev.data_ptr(), 448, 448)):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -5
        assert len(det.detect_device([dev.data_ptr()], [448], [448], 0.5)[0]) >= 1
    finally:
        det.close()


# ---------------------------------------------------------------------------------------------- 6. the C++ class
def test_cpp_class_detect_rois(rfa, scene, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_roi.cpp")
    exe = str(tmp_path / "test_roi")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    big, small, own = scene
    rois = regions(big, own, 17)
    raw, rbin, out = str(tmp_path / "frame.raw"), str(tmp_path / "rois.bin"), str(tmp_path / "out.bin")
    big.tofile(raw)
    np.array(rois, np.int32).tofile(rbin)
    det = engine(rfa)
    for grid, mz, vote, mf in ((0, 0, 0, 0), (2, 4, 1, 3)):
        r = subprocess.run([exe, ASSETS, "mnet25", "448", "448", raw, "896", "1280", rbin, "0.5", str(grid), str(mz), str(vote), str(mf), out],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        blob = open(out, "rb").read()
        n = int(np.frombuffer(blob, np.int32, 1)[0])
        assert n == 3
        want, wv, ws = det.detect_rois([big, None, big], [rois, rois, rois[:8]], 0.5, grid=grid, max_zoom=mz, vote=vote == 1, max_faces=mf,
                                       return_src_roi=True)
        pos = 4
        for i in range(n):
            k = int(np.frombuffer(blob, np.int32, 1, pos)[0])
            faces = np.frombuffer(blob, np.float32, k * 15, pos + 4).reshape(k, 15)
            votes = np.frombuffer(blob, np.int32, k, pos + 4 + 60 * k)
            srcs = np.frombuffer(blob, np.int32, k, pos + 4 + 64 * k)
            pos += 4 + 68 * k
            assert faces.tobytes() == rows_of(want[i]).tobytes() and list(votes) == list(wv[i]) and list(srcs) == list(ws[i]), i
            assert k == (0 if i == 1 else len(want[i])) and (mf == 0 or i == 1 or k == mf)
        m = int(np.frombuffer(blob, np.int32, 1, pos)[0])
        nxt = np.frombuffer(blob, np.int32, 4 * m, pos + 4).reshape(m, 4)
        assert [tuple(int(v) for v in r) for r in nxt] == rfa.rois_from_faces(want[0]) and m == len(want[0]) > 0
        assert pos + 4 + 16 * m == len(blob)
