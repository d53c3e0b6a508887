"""Fisheye detection on the host (no GPU): rf_dewarp_host, rf_dewarp_map_face and rf_dewarp_merge_host -- the code the kernels run,
compiled for the host -- against tests/dewarp_ref.py byte for byte, rf_dewarp_plan against the float64 plan to one unit, the refusals,
a synthetic fisheye scene of four posters end to end through the CPU oracle, and dewarp.h on its own under the address and UB
sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import dewarp_ref as dr
from conftest import ROOT
from retinaface_amd import _lib, dewarp_host, dewarp_map_face, dewarp_merge_host, dewarp_plan, dewarp_spec
from test_rot_host import mixed_faces
from test_tta_host import face

MD = 256
NMS = 0.4
NET = (448, 448)
VIEWS = ((16, 16), (16, 48), (80, 48), (448, 448))            # (view_w, view_h)
SOURCES = ((1, 1), (2, 3), (63, 65), (129, 131))              # (rows, cols)
MESHES = ("random", "smooth", "last", "mirrored", "constant", "extreme", "negative")


def make_mesh(kind, view_w, view_h, rows, cols, seed=0):
    """one view's nodes, (ny, nx, 2) int32: nodes that are negative, beyond the frame, exactly on the last pixel, decreasing (a
    mirrored view), constant, and at +-2^22"""
    rng = np.random.default_rng(seed * 1000 + view_w * 7 + view_h + rows * 31 + cols)
    ny, nx = view_h // 16 + 1, view_w // 16 + 1
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    m = np.zeros((ny, nx, 2), np.int64)
    if kind == "random":                     # anywhere from 20 px outside to 20 px beyond the frame, cell by cell
        m[..., 0] = rng.integers(-20 * 256, (cols + 20) * 256, (ny, nx))
        m[..., 1] = rng.integers(-20 * 256, (rows + 20) * 256, (ny, nx))
    elif kind == "smooth":                   # the frame stretched over the view with a margin outside, and a wobble
        m[..., 0] = np.rint((ii / (nx - 1) * (cols + 3) - 2) * 256 + rng.integers(-200, 200, (ny, nx)))
        m[..., 1] = np.rint((jj / (ny - 1) * (rows + 3) - 2) * 256 + rng.integers(-200, 200, (ny, nx)))
    elif kind == "last":                     # the last pixel exactly in one corner, the first in the other: taps x0 + 1 = cols are outside
        m[..., 0] = np.rint(ii / (nx - 1) * (cols - 1) * 256)
        m[..., 1] = np.rint(jj / (ny - 1) * (rows - 1) * 256)
    elif kind == "mirrored":                 # decreasing in x and y
        m[..., 0] = np.rint((1 - ii / (nx - 1)) * (cols - 1) * 256 + 77)
        m[..., 1] = np.rint((1 - jj / (ny - 1)) * (rows - 1) * 256 - 33)
    elif kind == "constant":
        m[..., 0], m[..., 1] = (cols - 1) * 256, (rows - 1) * 128
    elif kind == "extreme":                  # +-2^22 with random signs, one node row inside so that something is drawn
        m[...] = np.where(rng.integers(0, 2, (ny, nx, 2)) > 0, dr.NODE_MAX, -dr.NODE_MAX)
        m[0] = 0
    elif kind == "negative":
        m[..., 0] = -rng.integers(1, 3 * 256, (ny, nx))
        m[..., 1] = -rng.integers(1, 3 * 256, (ny, nx))
    return m.astype(np.int32)


def pitched(frame):
    """the frame as a view, at an odd address, of a buffer whose row pitch is odd"""
    rows, cols = frame.shape[:2]
    extra = 4 if cols & 1 else 5
    buf = np.zeros(rows * (3 * cols + extra) + 1, np.uint8)
    v = np.lib.stride_tricks.as_strided(buf[1:], (rows, cols, 3), (3 * cols + extra, 3, 1))
    v[...] = frame
    return v


# ---------------------------------------------------------------------------------------------- the warp
@pytest.mark.parametrize("view", VIEWS)
def test_warp_equals_the_reference_byte_for_byte(view):
    view_w, view_h = view
    for rows, cols in SOURCES:
        rng = np.random.default_rng(rows * 1000 + cols)
        frame = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        odd = pitched(frame)
        assert odd.strides[0] & 1
        for kind in MESHES:
            mesh = make_mesh(kind, view_w, view_h, rows, cols)
            want = dr.warp(frame, mesh, view_w, view_h)
            assert np.array_equal(dewarp_host(frame, mesh, view_w, view_h), want), (view, rows, cols, kind)
            buf = np.full((view_h, view_w + 3, 3), 0xAB, np.uint8)                     # a pitched destination
            dewarp_host(odd, mesh, view_w, view_h, out=buf[:, :view_w])
            assert np.array_equal(buf[:, :view_w], want) and (buf[:, view_w:] == 0xAB).all(), (view, rows, cols, kind)
            if kind in ("last", "smooth"):
                assert want.any()                                                         # the case draws something


def test_warp_of_an_identity_mesh_is_the_frame_and_half_pixels_blend():
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (48, 80, 3), dtype=np.uint8)
    jj, ii = np.meshgrid(np.arange(4), np.arange(6), indexing="ij")
    ident = np.stack([ii * 16 * 256, jj * 16 * 256], -1).astype(np.int32)
    assert np.array_equal(dewarp_host(frame, ident, 80, 48), frame)
    half = ident.copy()
    half[..., 0] += 128                                                                   # half a pixel to the right
    want = (frame[:, :-1].astype(int) * 16 * 32 + frame[:, 1:].astype(int) * 16 * 32 + 512) >> 10
    got = dewarp_host(frame, half, 80, 48)
    assert np.array_equal(got[:, :-1], want) and np.array_equal(got[:, -1], (frame[:, -1].astype(int) * 512 + 512) >> 10)


def test_warp_refusals():
    lib = _lib.load_library()
    src, dst = np.zeros((4, 6, 3), np.uint8), np.zeros((16, 16, 3), np.uint8)
    mesh = np.zeros((2, 2, 2), np.int32)
    call = lambda m=mesh.ctypes.data, vw=16, vh=16, s=src.ctypes.data, rows=4, cols=6, step=18, d=dst.ctypes.data, dstep=48: lib.rf_dewarp_host(  # noqa: E731
        m, vw, vh, s, rows, cols, step, d, dstep)
    assert call() == 0
    far = mesh.copy()
    far[0, 0, 0] = dr.NODE_MAX + 1
    for kw in (dict(m=None), dict(vw=17), dict(vw=0), dict(vh=8), dict(vw=4112), dict(s=None), dict(d=None), dict(rows=0), dict(cols=-1), dict(step=17),
               dict(dstep=47), dict(m=far.ctypes.data)):
        assert call(**kw) == _lib.RF_ERR_INVALID_ARG, kw


# ---------------------------------------------------------------------------------------------- the face mapping
def border_faces(view_w, view_h, rng):
    """faces at and beyond the view borders, a NaN coordinate, and random ones"""
    w, h = float(view_w - 1), float(view_h - 1)
    faces = [face(0.0, 0.0, w, h, 0.99), face(-30.0, -40.0, w + 60, h + 80, 0.9), face(w - 3, h - 3, 3.0, 3.0, 0.8), face(-100.0, 5.0, 20.0, 8.0, 0.7),
             face(w + 16.0, h + 16.0, 40.0, 40.0, 0.6), face(w + 15.99, -16.01, 1.0, 1.0, 0.6), face(1e9, -1e9, 1.0, 1.0, 0.55)]
    nan = face(3.0, 4.0, 7.0, 6.0, 0.75)
    nan[2] = nan[7] = np.float32("nan")
    faces.append(nan)
    for _ in range(20):
        f = rng.uniform(-24, max(view_w, view_h) + 24, 15).astype(np.float32)
        f[0] = np.float32(rng.uniform(0.5, 1))
        f[3], f[4] = max(f[1], f[3]), max(f[2], f[4])
        faces.append(f)
    return faces


@pytest.mark.parametrize("view", VIEWS)
def test_map_face_equals_the_reference_bit_for_bit(view):
    view_w, view_h = view
    rng = np.random.default_rng(view_w * 100 + view_h)
    nets = (NET, (8, 8)) if view != (448, 448) else (NET, (224, 256))          # scales of 1 and above 1
    assert dr.frame_scale(view_h, view_w, *nets[0]) == 1 and dr.frame_scale(view_h, view_w, *nets[1]) > 1
    for kind in MESHES:
        mesh = make_mesh(kind, view_w, view_h, 129, 131)
        for net in nets:
            for f in border_faces(view_w, view_h, rng):
                for edge in (0, 3):
                    want = dr.map_face(f, mesh, view_w, view_h, *net, edge)
                    got = dewarp_map_face(f, mesh, view_w, view_h, *net, edge)
                    assert (got is None) == (want is None), (view, kind, net, edge, f)
                    if want is not None:
                        assert got.tobytes() == want.tobytes(), (view, kind, net, edge, f)
                        assert got[1] <= got[3] and got[2] <= got[4] and got[0] == f[0]


def test_map_face_on_an_identity_mesh_and_the_edge_rule():
    jj, ii = np.meshgrid(np.arange(4), np.arange(6), indexing="ij")
    ident = np.stack([ii * 16 * 256 + 5 * 256, jj * 16 * 256 - 3 * 256], -1).astype(np.int32)      # a shift by (5, -3)
    f = face(10.25, 7.5, 30.0, 20.5, 0.875)
    got = dewarp_map_face(f, ident, 80, 48, *NET)
    want = f.copy()
    want[[1, 3, 5, 6, 7, 8, 9]] += 5
    want[[2, 4, 10, 11, 12, 13, 14]] -= 3
    assert np.allclose(got, want, atol=1 / 256) and got[0] == f[0]
    assert got[1:5].tobytes() == want[1:5].tobytes()                       # quarter pixels are exact
    # a point one cell beyond the view is extrapolated, further out it is clamped
    p = np.zeros(15, np.float32)
    p[5], p[10] = 80 + 16, -16
    m = dewarp_map_face(p, ident, 80, 48, *NET)
    assert (m[5], m[10]) == (101.0, -19.0)
    p[5], p[10] = 500, -500
    assert tuple(dewarp_map_face(p, ident, 80, 48, *NET)[[5, 10]]) == (101.0, -19.0)
    # the edge rule reads the scaled box, in view pixels
    for box, kept in (((8, 8, 71, 39), True), ((7.99, 8, 71, 39), False), ((8, 7.99, 71, 39), False), ((8, 8, 71.01, 39), False), ((8, 8, 71, 39.01), False)):
        g = face(box[0], box[1], box[2] - box[0], box[3] - box[1], 0.9)
        g[1:5] = box
        assert (dewarp_map_face(g, ident, 80, 48, *NET, edge=8) is not None) == kept, box
        assert dewarp_map_face(g, ident, 80, 48, *NET, edge=0) is not None


def test_map_face_refusals():
    lib = _lib.load_library()
    f, g = _lib.rf_face(), _lib.rf_face()
    mesh = np.zeros((2, 2, 2), np.int32)
    call = lambda m=mesh.ctypes.data, vw=16, vh=16, nh=448, nw=448, edge=0, a=C.byref(f), b=C.byref(g): lib.rf_dewarp_map_face(m, vw, vh, nh, nw, edge, a, b)  # noqa: E731
    assert call() == 1
    for kw in (dict(m=None), dict(vw=24), dict(vh=0), dict(nh=0), dict(nw=-1), dict(edge=-1), dict(edge=1025), dict(a=None), dict(b=None)):
        assert call(**kw) == _lib.RF_ERR_INVALID_ARG, kw


# ---------------------------------------------------------------------------------------------- the plan
F1024 = 0.98 * 1024 / np.pi
RING = dict(f=F1024, cx=511.5, cy=511.5, ring=4, pitch=55.0, hfov=60.0)


@pytest.mark.parametrize("model", (dr.EQUIDISTANT, dr.EQUISOLID, dr.STEREOGRAPHIC, dr.ORTHOGRAPHIC))
def test_plan_equals_the_float64_plan_to_one_unit(model):
    """libm and numpy are not correctly rounded: a node may differ by one unit of 1/256 px, no more"""
    pitch = 30.0 if model == dr.ORTHOGRAPHIC else 55.0
    for view_w, view_h, views in ((448, 448, dr.ring(4, pitch, 60.0)), (80, 48, [(10.0, 20.0, 30.0, 40.0), (-200.0, pitch, -45.0, 75.0), (0.0, 0.0, 0.0, 90.0)])):
        got = dewarp_plan(dewarp_spec(model, F1024, 511.5, 300.25, views=views), view_w, view_h)
        want = dr.plan(model, F1024, 511.5, 300.25, views, view_w, view_h)
        assert got.shape == want.shape and np.abs(got.astype(np.int64) - want).max() <= 1, (model, view_w)
    # the ring preset is the explicit list
    ring = dewarp_plan(dewarp_spec(model, F1024, 511.5, 511.5, ring=4, pitch=pitch, hfov=60.0), 448, 448)
    assert np.array_equal(ring, dewarp_plan(dewarp_spec(model, F1024, 511.5, 511.5, views=dr.ring(4, pitch, 60.0)), 448, 448))
    # The centre of an on-axis view lands on (cx, cy).  The centre, (w - 1) / 2, is no node; at hfov 20 the lens map is linear over the
    # 16 px cell around it to 2e-4 px (its cubic term, (15.5 / fv)^3 / 3 f with fv = 1270), so the mesh's blend there shows the plan.
    for yaw, roll in ((0.0, 0.0), (77.0, 0.0), (0.0, 123.0)):
        axis = dewarp_plan(dewarp_spec(model, F1024, 511.5, 300.25, views=[(yaw, 0.0, roll, 20.0)]), 448, 448)[0]
        cx, cy = dr.map_point(axis, 448, 448, 447 * 128, 447 * 128)
        assert abs(cx - 511.5 * 256) <= 1 and abs(cy - 300.25 * 256) <= 1, (model, yaw, roll, cx, cy)
    # pitch > 0 at yaw 0: the view's centre lies above the lens centre, and the view's up points away from it
    up = dewarp_plan(dewarp_spec(model, F1024, 511.5, 511.5, views=[(0.0, pitch, 0.0, 60.0)]), 448, 448)[0]
    assert abs(up[14, 14, 0] - 511.5 * 256) < 16 * 256 and up[14, 14, 1] < 400 * 256 and up[0, 14, 1] < up[14, 14, 1] < up[28, 14, 1]


def test_plan_refusals():
    lib = _lib.load_library()
    mesh = np.zeros(16 * 29 * 29 * 2, np.int32)
    views = C.c_int(-7)

    def call(sp, vw=448, vh=448, m=mesh.ctypes.data_as(C.POINTER(C.c_int32)), cap=mesh.size):
        return lib.rf_dewarp_plan(C.byref(sp) if sp is not None else None, vw, vh, m, cap, C.byref(views))
    assert call(dewarp_spec(**RING)) == 0 and views.value == 4
    assert C.sizeof(_lib.rf_dewarp_spec) == 584
    bad = [dewarp_spec(dr.ORTHOGRAPHIC, F1024, 511.5, 511.5, ring=4, pitch=65.0, hfov=60.0),      # theta reaches pi / 2 in the top corners
           dewarp_spec(dr.ORTHOGRAPHIC, F1024, 511.5, 511.5, views=[(0.0, 61.0, 0.0, 60.0)]),
           dewarp_spec(dr.STEREOGRAPHIC, F1024, 511.5, 511.5, views=[(0.0, 179.0, 0.0, 60.0)]),   # 2 f tan(theta / 2) beyond 2^22
           dewarp_spec(f=1e5, cx=511.5, cy=511.5, ring=4, pitch=55.0, hfov=60.0),                 # f theta beyond 2^22
           dewarp_spec(f=0.0, cx=511.5, cy=511.5, ring=4, pitch=55.0, hfov=60.0),
           dewarp_spec(f=F1024, ring=4, pitch=55.0, hfov=180.0), dewarp_spec(f=F1024, ring=4, pitch=55.0, hfov=0.0),
           dewarp_spec(f=F1024, ring=17, pitch=55.0, hfov=60.0), dewarp_spec(f=F1024, ring=0, pitch=55.0, hfov=60.0),
           dewarp_spec(f=F1024, ring=2, pitch=55.0, hfov=60.0, views=[(0.0, 0.0, 0.0, 60.0)]),    # a ring and a list
           dewarp_spec(4, **RING), dewarp_spec(-1, **RING), dewarp_spec(f=float("nan"), ring=4, pitch=55.0, hfov=60.0)]
    size = dewarp_spec(**RING)
    size.struct_size = 580
    many = dewarp_spec(**RING)
    many.ring, many.views = 0, 17
    for sp in bad + [size, many]:
        views.value = -7
        assert call(sp) == _lib.RF_ERR_INVALID_ARG and views.value == -7
    ok = dewarp_spec(**RING)
    for kw in (dict(vw=440), dict(vh=0), dict(vw=4112), dict(m=None), dict(cap=4 * 29 * 29 * 2 - 1), dict(cap=-1)):
        assert call(ok, **kw) == _lib.RF_ERR_INVALID_ARG, kw
    assert call(None) == _lib.RF_ERR_INVALID_ARG
    assert call(ok, cap=4 * 29 * 29 * 2) == 0
    with pytest.raises(_lib.RFError):
        dewarp_spec(views=[(0.0, 0.0, 0.0, 60.0)] * 17)
    with pytest.raises(dr.Refused):
        dr.plan(dr.ORTHOGRAPHIC, F1024, 511.5, 511.5, dr.ring(4, 65.0, 60.0), 448, 448)
    with pytest.raises(dr.Refused):
        dr.plan(dr.EQUIDISTANT, 1e5, 511.5, 511.5, dr.ring(4, 55.0, 60.0), 448, 448)


# ---------------------------------------------------------------------------------------------- merge
def overlapping_views(views, view_w=448, view_h=448, seed=3):
    """meshes of views that look at nearly the same part of a frame, shifted and wobbled: faces at the same view coordinates of
    different views land on overlapping boxes, so the merge has clusters across views"""
    rng = np.random.default_rng(seed)
    ny, nx = view_h // 16 + 1, view_w // 16 + 1
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    out = []
    for v in range(views):
        m = np.stack([ii * 16 * 256 * 1.25 + 700 * v + 40 * 256, jj * 16 * 256 * 1.125 - 500 * v + 9 * 256], -1) + rng.integers(-300, 300, (ny, nx, 2))
        out.append(np.rint(m).astype(np.int32))
    return np.stack(out)


def deal_views(faces, views, md=MD):
    """view-space faces dealt in turn over the views, each view in score order"""
    passes = [[] for _ in range(views)]
    for j, f in enumerate(faces):
        passes[j % views].append(f)
    out = []
    for p in passes:
        p = sorted(p, key=lambda f: -f[0])
        assert len(p) <= md
        out.append(np.stack(p).astype(np.float32) if p else np.zeros((0, 15), np.float32))
    return out


def check_host(passes, mesh, view=(448, 448), thr=NMS, md=MD, net=NET, **kw):
    """rf_dewarp_merge_host against dewarp_ref.merge, byte for byte; returns the reference tuple"""
    vote, mf, edge = kw.get("vote", False), kw.get("max_faces", 0), kw.get("edge", 0)
    limit = min(mf or md, kw["cap"] if kw.get("cap") is not None else md)
    want = dr.merge(mesh, *view, passes, *net, thr, md, vote, mf, edge)
    faces, count, votes, src, truncated = dewarp_merge_host(passes, mesh, *view, *net, thr, md, **kw)
    assert count == want[1]
    assert faces.tobytes() == want[0][:limit].tobytes()
    assert list(votes) == list(want[2][:limit]) and list(src) == list(want[3][:limit])
    assert truncated == (count > limit or any(len(p) > md for p in passes))
    return want


def test_merge_of_zero_one_and_two_candidates():
    mesh = overlapping_views(3)
    none = np.zeros((0, 15), np.float32)
    assert check_host([none] * 3, mesh)[1] == 0
    a, b = face(100, 100, 40, 40, 0.9), face(101, 102, 40, 40, 0.8)
    for v in range(3):
        passes = [none] * 3
        passes[v] = a[None]
        want = check_host(passes, mesh)
        assert want[1] == 1 and list(want[3]) == [v] and want[0][0].tobytes() == dr.map_face(a, mesh[v], 448, 448, *NET).tobytes()
    want = check_host([a[None], none, b[None]], mesh)                          # vote off, the default: the head keeps its bytes
    assert want[1] == 1 and list(want[2]) == [2] and list(want[3]) == [0]
    voted = check_host([a[None], none, b[None]], mesh, vote=True)
    assert voted[1] == 1 and voted[0][0].tobytes() != want[0][0].tobytes()
    # equal scores: g decides, the lower view heads the cluster
    b[0] = a[0]
    assert list(check_host([none, b[None], a[None]], mesh)[3]) == [1]
    # the edge rule drops a face before the merge sees it
    near = face(2, 100, 40, 40, 0.95)
    want = check_host([near[None], a[None], none], mesh, edge=8)
    assert want[1] == 1 and want[4] == 1 and list(want[3]) == [1]
    # a NULL spec is vote off, edge 0
    lib = _lib.load_library()
    flat = np.zeros((3, MD, 15), np.float32)
    flat[0, 0], flat[2, 0] = a, b
    out, count = (_lib.rf_face * MD)(), C.c_int()
    assert lib.rf_dewarp_merge_host(None, mesh.ctypes.data, 448, 448, 3, 448, 448, NMS, MD, flat.ctypes.data_as(C.POINTER(_lib.rf_face)), (C.c_int * 3)(1, 0, 1),
                                    out, MD, C.byref(count), None, None) == 0
    assert count.value == 1


@pytest.mark.parametrize("views", (1, 4, 16))
@pytest.mark.parametrize("vote", (False, True))
def test_merge_equals_the_reference_on_dealt_faces(views, vote):
    mesh = overlapping_views(views)
    passes = deal_views(mixed_faces(11 + views, 180), views)
    want = check_host(passes, mesh, vote=vote)
    assert 0 < want[1] < 180 and (want[2] == 1).any() and set(want[3].tolist()) <= set(range(views))
    if views > 1:
        assert want[2].max() >= 3 and len(set(want[3].tolist())) >= min(views, 3)
    assert check_host(passes, mesh, vote=vote, edge=8)[4] < want[4]            # the edge rule dropped some
    # max_faces and cap cut the list; the count stays true and the call says so
    check_host(passes, mesh, vote=vote, max_faces=7)
    check_host(passes, mesh, vote=vote, cap=5)
    check_host(passes, mesh, vote=vote, max_faces=9, cap=3)
    check_host(passes, mesh, vote=vote, cap=0)
    # a pass count above max_detections is clamped and reported
    if views <= 4:
        check_host(passes, mesh, vote=vote, md=16)
        assert dewarp_merge_host(passes, mesh, 448, 448, *NET, NMS, 16)[4]
    # views larger than the net: every face is scaled first
    small = overlapping_views(views, 80, 48)
    check_host(deal_views(mixed_faces(5, 40, cols=60, rows=60), views), small, view=(80, 48), net=(32, 32), vote=vote)


def test_merge_refusals():
    lib = _lib.load_library()
    mesh = overlapping_views(2)
    faces = (_lib.rf_face * (2 * MD))()
    pc = (C.c_int * 2)(0, 0)
    out = (_lib.rf_face * MD)()
    count = C.c_int(-7)

    def call(sp, m=mesh.ctypes.data, vw=448, vh=448, views=2, nh=448, nw=448, md=MD, faces=faces, pc=pc, out=out, cap=MD, count=C.byref(count)):
        return lib.rf_dewarp_merge_host(sp, m, vw, vh, views, nh, nw, 0.4, md, faces, pc, out, cap, count, None, None)
    assert call(None) == 0 and count.value == 0
    assert call(C.byref(dewarp_spec())) == 0 and call(C.byref(dewarp_spec(vote=True, max_faces=4096, edge=1024))) == 0
    for field, value in (("struct_size", 580), ("struct_size", 588), ("vote", 3), ("vote", -1), ("max_faces", 4097), ("max_faces", -1), ("edge", -1),
                         ("edge", 1025)):
        sp = dewarp_spec()
        setattr(sp, field, value)
        count.value = -7
        assert call(C.byref(sp)) == _lib.RF_ERR_INVALID_ARG and count.value == -7, (field, value)
    for kw in (dict(md=0), dict(md=4097), dict(nh=0), dict(m=None), dict(vw=440), dict(views=0), dict(views=17), dict(faces=None), dict(pc=None),
               dict(count=None), dict(cap=-1), dict(out=None), dict(pc=(C.c_int * 2)(0, -1))):
        assert call(None, **kw) == _lib.RF_ERR_INVALID_ARG, kw
    assert call(None, out=None, cap=0) == 0
    with pytest.raises(_lib.RFError):
        dewarp_merge_host([np.zeros((0, 15), np.float32)] * 3, mesh, 448, 448, *NET, NMS, MD)        # two views want two passes


# ---------------------------------------------------------------------------------------------- end to end through the CPU oracle
POSTERS = ((30, 440), (30, 0), (200, 300), (0, 832))          # windows of the base frame, (y, x)
SCENE_THR = 0.6


def poster_scene(base_frame):
    """the 1024 x 1024 equidistant fisheye frame of the claim, its ring of four views and their exact meshes"""
    views = dr.ring(4, 55.0, 60.0)
    posters = [np.ascontiguousarray(base_frame[y:y + 448, x:x + 448]) for y, x in POSTERS]
    return dr.poster_scene(posters, 1024, F1024, views, 448, 448), posters, views


def exact_box(box, view):
    """a view box pushed through the exact float map: the bounds of its outline in the frame"""
    t = np.linspace(0, 1, 33)
    xs = np.concatenate([box[0] + t * (box[2] - box[0]), np.full(33, box[2]), box[0] + t * (box[2] - box[0]), np.full(33, box[0])])
    ys = np.concatenate([np.full(33, box[1]), box[1] + t * (box[3] - box[1]), np.full(33, box[3]), box[1] + t * (box[3] - box[1])])
    sx, sy = dr.source_of(dr.EQUIDISTANT, F1024, 511.5, 511.5, view, 448, 448, xs, ys)
    return sx.min(), sy.min(), sx.max(), sy.max()


def check_claim(merged, on_posters, plain, views):
    """every face the detector finds on the posters themselves is in the merge, its box where the exact map puts the poster's box; the
    plain pass finds fewer"""
    assert [len(p) for p in on_posters] == [2, 2, 2, 2] and len(merged) == 8 > len(plain)
    for v, faces in enumerate(on_posters):
        for f in faces:
            want = exact_box(f[1:5], views[v])
            assert max(dr.tta_ref.iou_plus1(m[1:5], want) for m in merged) >= 0.5, (v, f[:5], want)


def test_four_posters_around_the_axis_through_the_oracle(oracles, base_frame):
    """The claim: mnet25, 448 net, threshold 0.6.  A synthetic 1024 x 1024 equidistant fisheye frame (f = 0.98 * 1024 / pi, centre
    (511.5, 511.5)) shows the windows (30, 440), (30, 0), (200, 300), (0, 832) of the base frame as posters around the axis; a ring of
    four views (pitch 55, hfov 60) looks straight at them.  The four dewarped views give back the posters' own faces, 2 each (scores
    0.995 0.994 | 0.991 0.984 | 0.994 0.757 | 0.996 0.988; nothing else above 0.3, so the nearest score is 0.157 from the threshold);
    the plain pass on the frame shrunk to the net finds 2.  The mesh deviates from the exact per-pixel map by at most 0.131 px."""
    oracle = oracles["mnet25"]
    scene, posters, views = poster_scene(base_frame)
    mesh = dewarp_plan(dewarp_spec(**RING), 448, 448)
    Y, X = np.meshgrid(np.arange(448), np.arange(448), indexing="ij")
    for v in range(4):
        qx, qy = dr.pixel_sources(mesh[v], 448, 448)
        sx, sy = dr.source_of(dr.EQUIDISTANT, F1024, 511.5, 511.5, views[v], 448, 448, X, Y)
        dev = np.hypot(qx / 32 - sx, qy / 32 - sy).max()
        print("view", v, "mesh deviation %.4f px" % dev)
        assert dev < 0.2
    passes = []
    for v in range(4):
        warped = dewarp_host(scene, mesh[v], 448, 448)
        assert np.array_equal(warped, dr.warp(scene, mesh[v], 448, 448))
        passes.append(oracle.detect(warped, SCENE_THR, NMS, net_hw=NET).rows())
        near = oracle.detect(warped, SCENE_THR - 0.02, NMS, net_hw=NET).rows()
        assert len(near) == len(passes[-1]) and (passes[-1][:, 0] > SCENE_THR + 0.02).all()      # no score within 0.02 of the threshold
    on_posters = [oracle.detect(p, SCENE_THR, NMS, net_hw=NET).rows() for p in posters]
    plain = oracle.detect(scene, SCENE_THR, NMS, net_hw=NET).rows()
    want = check_host(passes, mesh)
    print("views:", [len(p) for p in passes], "posters:", [len(p) for p in on_posters], "merged:", want[1], "plain:", len(plain))
    assert sorted(want[3].tolist()) == [0, 0, 1, 1, 2, 2, 3, 3]
    check_claim(want[0], on_posters, plain, views)


# ---------------------------------------------------------------------------------------------- the sanitizer program
def test_warp_and_map_under_address_and_ub_sanitizers(tmp_path):
    """tests/csrc/test_dewarp_host.cpp: dewarp_view_host into exactly-sized heap buffers over meshes that leave the frame on every side
    and sit at +-2^22, dewarp_map_face at the extremes, the plan; host code only, built with -fsanitize=address,undefined.  No GPU and
    no library: dewarp.h is compiled into the program."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")                        # for <hip/hip_runtime.h>, which dewarp.h includes
    gxx = shutil.which("g++")
    assert gxx, "no g++"
    exe = str(tmp_path / "test_dewarp_host")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "test_dewarp_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
