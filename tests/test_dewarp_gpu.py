"""Fisheye detection on the GPU: the dewarp kernel against tests/dewarp_ref.py byte for byte, the gather and merge kernels on constructed
faces (no forward pass), the fused call against its own parts (ONE rf_detect_batch_device call over the reference's views + the reference
merge), the claim (four posters around the axis of a synthetic fisheye frame), the refusals, and the C++ class."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import dewarp_ref as dr
from conftest import ASSETS, ROOT
from test_dewarp_host import (F1024, MESHES, RING, SCENE_THR, SOURCES, VIEWS, check_claim, deal_views, make_mesh, overlapping_views,
                              poster_scene)
from test_gpu_align import FP16, engine, rfa, rows_of, to_device  # noqa: F401  (rfa: fixture)
from test_rot_host import mixed_faces
from test_tta_gpu import BIG, INT8, MD, NET, NMS, SPLIT2, SPLIT3, big_engine, odd_view
from test_tta_host import face, quarter

pytestmark = pytest.mark.gpu

# the workgroup tile is 64 x 16 view pixels and a view is whole cells of 16: one cell less than a tile, a tile, one cell more, and two
# tiles and a cell, with one and two tile rows
TILE_EDGES = ((48, 16), (64, 32), (80, 16), (144, 32))


# ---------------------------------------------------------------------------------------------- 1. the dewarp kernel
@pytest.mark.parametrize("view", VIEWS + TILE_EDGES)
def test_dewarp_device_equals_the_reference(rfa, view):
    import torch
    det = engine(rfa)
    view_w, view_h = view
    for rows, cols in SOURCES:
        rng = np.random.default_rng(rows * 1000 + cols)
        frame = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        mesh = np.stack([make_mesh(kind, view_w, view_h, rows, cols) for kind in MESHES])
        dw = det.dewarper(rows, cols, mesh=mesh, view_w=view_w, view_h=view_h)
        dense = to_device([frame])[0]
        keep, rptr, rstep = odd_view(frame)
        for v, kind in enumerate(MESHES):
            want = dr.warp(frame, mesh[v], view_w, view_h)
            for sptr, sstep in ((dense.data_ptr(), 3 * cols), (rptr, rstep)):
                for pad, shift in ((0, 0), (7, 1)):                  # a dense destination; a pitched one at an odd pointer
                    dstep = 3 * view_w + pad
                    dst = torch.full((view_h * dstep + 8,), 0xAB, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    det.dewarp_device(dw, v, sptr, dst.data_ptr() + shift, step=sstep, dst_step=dstep)
                    got = dst.cpu().numpy()
                    body = got[shift:shift + view_h * dstep].reshape(view_h, dstep)
                    assert np.array_equal(body[:, :3 * view_w].reshape(view_h, view_w, 3), want), (view, rows, cols, kind, pad, shift)
                    assert (body[:, 3 * view_w:] == 0xAB).all() and (got[:shift] == 0xAB).all() and (got[shift + view_h * dstep:] == 0xAB).all()
        dw.close()


# ---------------------------------------------------------------------------------------------- 2. merge with constructed faces
def view_faces(seed, want):
    """`want` faces of test_rot_host.mixed_faces laid out on a 1300-wide sheet and shrunk by 0.34: all of them inside a 448 x 448 view"""
    out = []
    for f in mixed_faces(seed, want, cols=1300):
        g = f.copy()
        g[1:] = g[1:] * np.float32(0.34)
        out.append(g)
    assert not out or max(f[1:].max() for f in out) < 448
    return out


def check_merge_call(det, dw, frames, md=BIG, **kw):
    """frames: per frame the faces of the dewarper's views; one rf_dewarp_merge_device call against dewarp_ref per frame, byte for byte,
    votes and views included"""
    dets, votes, src = det.dewarp_merge(dw, frames, return_votes=True, **kw)
    counts = list(det.dewarp_counts)
    limit = min(kw.get("max_faces", 0) or md, kw.get("cap_per_image", md))
    assert det.truncated == any(c > limit for c in counts)
    for i, passes in enumerate(frames):
        want = dr.merge(dw.mesh, dw.view_w, dw.view_h, passes, NET, NET, NMS, md, kw.get("vote", False), kw.get("max_faces", 0), kw.get("edge", 0))
        faces = want[0][:limit]
        assert counts[i] == want[1], (i, counts[i], want[1], want[4])
        assert rows_of(dets[i]).tobytes() == faces.tobytes(), (i, want[4])
        assert list(votes[i]) == list(want[2][:limit]) and list(src[i]) == list(want[3][:limit]), i
    return dets, votes, src, counts


def test_merge_of_constructed_faces_equals_the_reference(rfa):
    det = big_engine(rfa)
    assert det.max_detections == BIG
    dw = det.dewarper(600, 700, mesh=overlapping_views(4))
    made = {}

    def frame(want, seed):
        if (want, seed) not in made:
            made[want, seed] = deal_views(view_faces(seed, want), 4, md=BIG)
        return made[want, seed]
    # the three sort regimes and their boundaries, several frames per call
    calls = ([frame(0, 1), frame(1, 2), frame(64, 3), frame(257, 5)], [frame(65, 4), frame(1000, 6)])
    heads = []
    for frames in calls:
        for vote in (False, True):
            for edge in (0, 8):
                dets, votes, src, counts = check_merge_call(det, dw, frames, vote=vote, edge=edge)
        heads += check_merge_call(det, dw, frames)[3]
        again = det.dewarp_merge(dw, frames, vote=True, edge=8, return_votes=True)
        assert again[0] == dets and all(np.array_equal(a, b) for a, b in zip(again[1], votes))      # the counters re-armed, no order leaks
    assert heads[0] == 0 and heads[1] == 1 and all(0 < k < w for k, w in zip(heads[2:], (64, 257, 65, 1000)))
    want = dr.merge(dw.mesh, 448, 448, frame(1000, 6), NET, NET, NMS, BIG, True)
    assert want[2].max() >= 4 and (want[2] == 1).any() and set(want[3].tolist()) == {0, 1, 2, 3}
    assert dr.merge(dw.mesh, 448, 448, frame(1000, 6), NET, NET, NMS, BIG, True, 0, 8)[4] < want[4]       # the edge rule dropped faces
    # a smaller max_faces and a smaller cap_per_image: counts stay true
    check_merge_call(det, dw, [frame(257, 5), frame(1000, 6)], max_faces=7)
    assert det.truncated
    check_merge_call(det, dw, [frame(65, 4)], cap_per_image=5)
    assert det.truncated and det.dewarp_counts[0] > 5
    dw.close()


def test_merge_overflow_is_reported_and_leaves_the_other_frame_exact(rfa):
    det = big_engine(rfa)
    dw = det.dewarper(600, 700, mesh=overlapping_views(4))
    rng = np.random.default_rng(9)
    grid = [quarter(face(2.0 + 6 * (j % 74), 2.0 + 6 * (j // 74), 3.5, 4.25, np.float32(0.5) + np.float32(rng.integers(1, 32)) / np.float32(64)))
            for j in range(4500)]
    big = deal_views(grid, 4, md=BIG)
    assert sum(len(p) for p in big) == 4500 > dr.tta_ref.MERGE_CAP
    other = deal_views(view_faces(11, 300), 4, md=BIG)
    want = dr.merge(dw.mesh, 448, 448, other, NET, NET, NMS, BIG)
    for order in ((0, 1), (1, 0)):
        frames = [[big, other][k] for k in order]
        dets, votes, src = det.dewarp_merge(dw, frames, return_votes=True)
        assert det.truncated
        i = order.index(1)
        assert det.dewarp_counts[i] == want[1] and rows_of(dets[i]).tobytes() == want[0].tobytes()
        assert list(votes[i]) == list(want[2]) and list(src[i]) == list(want[3])
    check_merge_call(det, dw, [other])                     # the counters were re-armed: the next call is exact
    dw.close()


# ---------------------------------------------------------------------------------------------- 3. fused call against its own parts
@pytest.fixture(scope="module")
def scenes(base_frame):
    """the fisheye frame of the claim and five more made from it without another ray cast: turned and mirrored, it is still a fisheye
    frame around the same centre, whose posters the ring's views see turned or mirrored"""
    scene, posters, views = poster_scene(base_frame)
    frames = [scene, np.rot90(scene, 1), scene[:, ::-1], np.rot90(scene, 2), scene[::-1], np.rot90(scene, 3)]
    return [np.ascontiguousarray(f) for f in frames], posters, views


@pytest.fixture(scope="module")
def ring_mesh(rfa):
    return rfa.dewarp_plan(rfa.dewarp_spec(**RING), 448, 448)


_warped = {}


def ref_views(frame, mesh):
    """the reference's views of a frame, made once"""
    key = (hashlib.sha1(frame.tobytes()).hexdigest(), hashlib.sha1(mesh.tobytes()).hexdigest())
    if key not in _warped:
        _warped[key] = [dr.warp(frame, m, 448, 448) for m in mesh]
    return _warped[key]


def parts_of_call(det, mesh, frames, thr=0.5, md=MD, **kw):
    """frames: the pixels of one fisheye call (None: an empty frame).  dewarp_ref.merge, per frame, over what ONE rf_detect_batch_device
    call returns for [f0 v0, f0 v1, ..., f1 v0, ...] -- the call the engine itself makes; the views are made with numpy and uploaded
    densely.  One call, because the last bits of an image's result can depend on what shares its launch."""
    V = len(mesh)
    copies = to_device([v for f in frames if f is not None for v in ref_views(f, mesh)])
    ptrs, rows, cols, at = [], [], [], 0
    for f in frames:
        for v in range(V):
            if f is None:
                ptrs.append(0); rows.append(0); cols.append(0)
            else:
                ptrs.append(copies[at].data_ptr()); rows.append(448); cols.append(448)
                at += 1
    res = det.detect_device(ptrs, rows, cols, thr)
    assert not det.truncated
    out = []
    for i, f in enumerate(frames):
        passes = [rows_of(x) for x in res[V * i:V * (i + 1)]]
        out.append(dr.merge(mesh, 448, 448, passes, det.net_h, det.net_w, NMS, md, kw.get("vote", False), kw.get("max_faces", 0), kw.get("edge", 0))
                   if f is not None else None)
    return out


def check_frame(det, got, votes, src, i, want):
    if want is None:
        assert got[i] == [] and det.dewarp_counts[i] == 0
        return
    assert det.dewarp_counts[i] == want[1] and rows_of(got[i]).tobytes() == want[0].tobytes(), (i, det.dewarp_counts[i], want[1])
    assert list(votes[i]) == list(want[2]) and list(src[i]) == list(want[3]), i


def run_and_check(det, dw, frames, dev, thr=0.5, **kw):
    """frames: pixels (None: empty); dev: their device tensors (None likewise)"""
    want = parts_of_call(det, dw.mesh, frames, thr, **kw)
    got, votes, src = det.detect_dewarped_device([d.data_ptr() if d is not None else 0 for d in dev], dw, thr, return_votes=True, **kw)
    assert not det.truncated
    for i in range(len(frames)):
        check_frame(det, got, votes, src, i, want[i])
    return got, votes, src, want


@pytest.mark.parametrize("prec,kw", ((FP16, {}), (FP16, SPLIT2), (FP16, SPLIT3), (INT8, {})))
def test_fused_call_equals_the_merge_of_its_own_views(rfa, scenes, ring_mesh, prec, kw):
    """kw = {}: the whole call is one coalesced launch.  SPLIT2 / SPLIT3: the 24 views of six frames cross launches and lanes -- the merge
    waits for the other lanes' gathers on the device, and every lane waits for the dewarp kernel."""
    import torch
    det = engine(rfa, prec=prec, **kw)
    if kw:
        assert det.max_batch == 8 and det.num_slots() == kw["lanes"]
    frames = scenes[0]
    dev = to_device(frames)
    dw = det.dewarper(1024, 1024, mesh=ring_mesh)
    crop = to_device([np.ascontiguousarray(frames[0][100:548, 300:748])])[0]
    plain = det.detect_device([crop.data_ptr()], [448], [448], 0.5)
    got, votes, src, want = run_and_check(det, dw, frames, dev)
    assert sum(len(g) for g in got) >= 6 and len({int(s) for v in src for s in v}) >= 3          # heads came from several views
    # the first frame alone: four views, one launch
    first = run_and_check(det, dw, frames[:1], dev[:1])[0]
    # repeats give identical bytes; d_views receives the reference's views
    ptrs = [d.data_ptr() for d in dev]
    views = torch.full((6 * 4 * 448 * 448 * 3,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for views_ptr in (None, views.data_ptr()):
        again = det.detect_dewarped_device(ptrs, dw, 0.5, views_ptr=views_ptr, return_votes=True)
        assert again[0] == got and all(np.array_equal(a, b) for a, b in zip(again[2], src))
    have = views.cpu().numpy().reshape(6, 4, 448, 448, 3)
    for i, f in enumerate(frames):
        for v, w in enumerate(ref_views(f, dw.mesh)):
            assert np.array_equal(have[i, v], w), (i, v)
    # vote on, the edge rule, a smaller max_faces, an empty frame in the middle of the batch (whose views stay untouched)
    run_and_check(det, dw, frames[:3], dev[:3], vote=True)
    run_and_check(det, dw, frames[:2], dev[:2], edge=8)
    views.fill_(0xAB)
    torch.cuda.synchronize()
    mixed, mdev = frames[:2] + [None] + frames[2:4], dev[:2] + [None] + dev[2:4]
    run_and_check(det, dw, mixed, mdev)
    det.detect_dewarped_device([d.data_ptr() if d is not None else 0 for d in mdev], dw, 0.5, views_ptr=views.data_ptr())
    have = views.cpu().numpy().reshape(6, 4, 448, 448, 3)
    assert (have[2] == 0xAB).all() and np.array_equal(have[3, 1], ref_views(frames[2], dw.mesh)[1]) and (have[5] == 0xAB).all()
    cut = det.detect_dewarped_device(ptrs[:1], dw, 0.5, max_faces=1)
    assert det.truncated and det.dewarp_counts == [len(first[0])] and cut[0] == first[0][:1] and len(first[0]) > 1
    assert det.detect_device([crop.data_ptr()], [448], [448], 0.5) == plain
    if prec != FP16:
        dw.close()
        return
    # a pitched device frame at an odd pointer
    keep, rptr, rstep = odd_view(frames[1])
    pgot = det.detect_dewarped_device([rptr, ptrs[0]], dw, 0.5, steps=[rstep, 3 * 1024], return_votes=True)
    pwant = parts_of_call(det, dw.mesh, [frames[1], frames[0]])
    for i in range(2):
        check_frame(det, pgot[0], pgot[1], pgot[2], i, pwant[i])
    # host frames: uploaded once, densely; an empty frame in between
    hgot, hvotes, hsrc = det.detect_dewarped([frames[0], None, frames[1]], dw, 0.5, return_votes=True)
    hwant = parts_of_call(det, dw.mesh, [frames[0], None, frames[1]])
    for i in range(3):
        check_frame(det, hgot, hvotes, hsrc, i, hwant[i])
    assert det.detect_device([crop.data_ptr()], [448], [448], 0.5) == plain
    dw.close()


def test_fisheye_tta_and_rotation_calls_share_their_blocks(rfa, scenes, ring_mesh, base_frame):
    """one SPLIT3 handle: a fisheye call between a TTA and a rotation call; each returns the bytes a fresh handle returns for it"""
    frames = scenes[0][:3]
    dev = to_device(frames)
    ptrs = [d.data_ptr() for d in dev]
    wins = to_device([np.ascontiguousarray(base_frame[y:y + 448, x:x + 448]) for y, x in ((30, 440), (30, 0), (200, 300))])
    wptrs = [d.data_ptr() for d in wins]
    calls = (lambda d, dw: d.detect_tta_device(wptrs, [448] * 3, [448] * 3, 0.5, return_votes=True),
             lambda d, dw: d.detect_dewarped_device(ptrs, dw, 0.5, return_votes=True),
             lambda d, dw: d.detect_rotated_device(wptrs, [448] * 3, [448] * 3, 0.5, return_votes=True))
    fresh = []
    for call in calls:
        det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", **SPLIT3)
        try:
            fresh.append(call(det, det.dewarper(1024, 1024, mesh=ring_mesh)))
        finally:
            det.close()
    det = engine(rfa, **SPLIT3)
    dw = det.dewarper(1024, 1024, mesh=ring_mesh)
    for _ in range(2):
        for call, want in zip(calls, fresh):
            got = call(det, dw)
            assert got[0] == want[0] and all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))
            assert all(np.array_equal(a, b) for a, b in zip(got[2], want[2]))
    dw.close()


# ---------------------------------------------------------------------------------------------- 4. the claim
def test_four_posters_around_the_axis_are_found(rfa, scenes, ring_mesh):
    """fp16 mnet25, threshold 0.6, the scene of tests/test_dewarp_host.py: the fisheye call finds the two faces of each of the four
    posters, every head from the view that looks at its poster; the plain call on the frame, shrunk to the net, finds fewer.  The
    oracle's nearest score to 0.6 is 0.757: a margin of 0.157, 78 x the suite's SCORE_NOISE of 2e-3."""
    det = engine(rfa)
    (scene, *_), posters, views = scenes
    dw = det.dewarper(1024, 1024, mesh=ring_mesh)
    dev = to_device([scene] + posters)
    got, votes, src = det.detect_dewarped_device([dev[0].data_ptr()], dw, SCENE_THR, return_votes=True)
    plain = det.detect_device([dev[0].data_ptr()], [1024], [1024], SCENE_THR)[0]
    on_posters = [rows_of(p) for p in det.detect_device([d.data_ptr() for d in dev[1:]], [448] * 4, [448] * 4, SCENE_THR)]
    print("fisheye call:", len(got[0]), "src_view:", list(src[0]), "posters:", [len(p) for p in on_posters], "plain call:", len(plain))
    assert sorted(src[0].tolist()) == [0, 0, 1, 1, 2, 2, 3, 3]
    check_claim(rows_of(got[0]), on_posters, plain, views)
    dw.close()


# ---------------------------------------------------------------------------------------------- 5. refusals, multi-device
def test_refusals_leave_the_handle_usable(rfa, scenes, ring_mesh):
    det = engine(rfa)
    lib = det._lib
    scene = scenes[0][0]
    dev = to_device([scene])[0]
    dw = det.dewarper(1024, 1024, mesh=ring_mesh)
    before = det.detect_dewarped_device([dev.data_ptr()], dw, 0.5)
    crop = to_device([np.ascontiguousarray(scene[100:548, 300:748])])[0]
    plain = det.detect_device([crop.data_ptr()], [448], [448], 0.5)

    def usable():
        assert det.detect_dewarped_device([dev.data_ptr()], dw, 0.5) == before
        assert det.detect_device([crop.data_ptr()], [448], [448], 0.5) == plain
    for bad in (dict(max_faces=4097), dict(max_faces=-1), dict(edge=-1), dict(edge=1025)):
        for call in (lambda: det.detect_dewarped_device([dev.data_ptr()], dw, 0.5, **bad), lambda: det.detect_dewarped([scene], dw, 0.5, **bad),
                     lambda: det.dewarp_merge(dw, [[np.zeros((0, 15), np.float32)] * 4], **bad)):
            with pytest.raises(rfa.RFError) as e:
                call()
            assert e.value.status == -1, bad
    usable()
    cnt, out = (C.c_int * 1)(), (rfa._lib.rf_face * MD)()
    args = (dw._d, (C.c_void_p * 1)(dev.data_ptr()), (C.c_int * 1)(1024), (C.c_int * 1)(1024), (C.c_int * 1)(3072), 1, 0.5)
    tail = (out, MD, cnt, None, None, None)
    for field, value in (("struct_size", 580), ("vote", 3), ("vote", -1)):
        sp = rfa.dewarp_spec()
        setattr(sp, field, value)
        assert lib.rf_detect_dewarp_batch_device(*args, C.byref(sp), *tail) == -1, field
    assert lib.rf_detect_dewarp_batch_device(*args, None, None, MD, cnt, None, None, None) == -1                  # out is null
    assert lib.rf_detect_dewarp_batch_device(*args, None, *tail) == 0 and cnt[0] == len(before[0])                  # a NULL spec: the defaults
    usable()
    # a frame of another shape, a short step
    for r, c, st in ((1024, 1023, 3072), (512, 1024, 3072), (1024, 1024, 3071)):
        bad_args = (dw._d, (C.c_void_p * 1)(dev.data_ptr()), (C.c_int * 1)(r), (C.c_int * 1)(c), (C.c_int * 1)(st), 1, 0.5)
        assert lib.rf_detect_dewarp_batch_device(*bad_args, None, *tail) == -1, (r, c, st)
    with pytest.raises(rfa.RFError):
        det.detect_dewarped([scene[:1000]], dw, 0.5)
    usable()
    # dewarpers that cannot be: more than 16 views, a bad view size, a node beyond 2^22, a bad frame shape, a null mesh
    d = C.c_void_p()
    many = np.zeros((17, 29, 29, 2), np.int32)
    far = ring_mesh.copy()
    far[3, 28, 28, 1] = dr.NODE_MAX + 1
    for r, c, vw, vh, n, m in ((1024, 1024, 448, 448, 17, many.ctypes.data), (1024, 1024, 440, 448, 4, ring_mesh.ctypes.data),
                               (1024, 1024, 448, 448, 0, ring_mesh.ctypes.data), (1024, 1024, 448, 448, 4, far.ctypes.data),
                               (0, 1024, 448, 448, 4, ring_mesh.ctypes.data), (4097, 3072, 448, 448, 4, ring_mesh.ctypes.data),
                               (1024, 1024, 448, 448, 4, None), (1024, 1024, -16, 448, 4, ring_mesh.ctypes.data)):
        assert lib.rf_dewarper_create(det._h, r, c, vw, vh, n, m, C.byref(d)) == -1 and not d.value, (r, c, vw, vh, n)
    assert lib.rf_dewarper_create(det._h, 1024, 1024, 0, 0, 4, ring_mesh.ctypes.data, C.byref(d)) == 0      # 0: the net size
    lib.rf_dewarper_destroy(d)
    # a destroyed dewarper is refused by every call, again and again, and destroying it twice is harmless
    for _ in range(2):
        assert lib.rf_detect_dewarp_batch_device(d, *args[1:], None, *tail) == -1
        assert lib.rf_dewarp_device(d, 0, dev.data_ptr(), 3072, crop.data_ptr(), 3 * 448) == -1
        assert lib.rf_dewarp_merge_device(d, 0, None, None, None, None, 0, None, None, None) == -1
        lib.rf_dewarper_destroy(d)
    # the kernel's own refusals
    for kw in (dict(view=4), dict(view=-1), dict(step=3071), dict(dst_step=3 * 448 - 1)):
        with pytest.raises(rfa.RFError) as e:
            det.dewarp_device(dw, kw.pop("view", 0), dev.data_ptr(), crop.data_ptr(), **kw)
        assert e.value.status == -1
    with pytest.raises(rfa.RFError):
        det.dewarp_device(dw, 0, dev.data_ptr(), 0)
    usable()
    dw.close()


def test_multi_device_handles_refuse_fisheye_detection(rfa, crop448, ring_mesh):
    det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=(448, 448), model_stem="mnet25", devices=[0, 0])
    try:
        with pytest.raises(rfa.RFError) as e:
            det.dewarper(1024, 1024, mesh=ring_mesh)
        assert e.value.status == -5
        dev = to_device([crop448])[0]
        assert len(det.detect_device([dev.data_ptr()], [448], [448], 0.5)[0]) >= 1
    finally:
        det.close()


# ---------------------------------------------------------------------------------------------- 6. the C++ class
def test_cpp_class_detect_dewarped(rfa, scenes, tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "test_dewarp.cpp")
    exe = str(tmp_path / "test_dewarp")
    lib_dir = os.path.dirname(rfa.lib_path())
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DRF_NO_OPENCV", "-I" + os.path.join(ROOT, "include"), "-o", exe, src,
                           "-L" + lib_dir, "-lretinaface_amd", "-Wl,-rpath," + lib_dir])
    raw, out = str(tmp_path / "frame.raw"), str(tmp_path / "out.bin")
    scene = scenes[0][0]
    scene.tofile(raw)
    det = engine(rfa)
    dw = det.dewarper(1024, 1024, spec=rfa.dewarp_spec(**RING))
    for vote, mf, edge in ((0, 0, 0), (1, 3, 0), (2, 0, 8)):
        r = subprocess.run([exe, ASSETS, "mnet25", "448", "448", raw, "1024", "0.5", "%.17g" % F1024, "4", "55", "60", str(vote), str(mf), str(edge), out],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        blob = open(out, "rb").read()
        n = int(np.frombuffer(blob, np.int32, 1)[0])
        assert n == 3
        want, wv, ws = det.detect_dewarped([scene, None, scene], dw, 0.5, vote=vote == 1, max_faces=mf, edge=edge, return_votes=True)
        pos = 4
        for i in range(n):
            k = int(np.frombuffer(blob, np.int32, 1, pos)[0])
            faces = np.frombuffer(blob, np.float32, k * 15, pos + 4).reshape(k, 15)
            votes = np.frombuffer(blob, np.int32, k, pos + 4 + 60 * k)
            srcs = np.frombuffer(blob, np.int32, k, pos + 4 + 64 * k)
            pos += 4 + 68 * k
            assert faces.tobytes() == rows_of(want[i]).tobytes() and list(votes) == list(wv[i]) and list(srcs) == list(ws[i]), i
            assert k == (0 if i == 1 else len(want[0])) and (mf == 0 or i == 1 or k == mf)
        assert pos == len(blob)
    dw.close()
