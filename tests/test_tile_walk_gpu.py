"""Tile walks of the persistent kernels (`-m gpu`): a launch whose grid is forced small must store the bytes of the same launch with one
workgroup per tile.

A persistent kernel's workgroup loads its weights once and walks tiles first, first + G, ... (pack.h TileCoord / TileStep), prefetching the
next tile's halo and re-using its LDS regions and LDS-DMA ring slots from tile to tile, across image boundaries.  That only happens where
a launch has more tiles than the chip keeps workgroups resident (256 CUs x 1..8), which no launch of the per-launch tests reaches: the
largest persistent launch at 352 x 608 has 330 tiles for three images.  A tile's arithmetic does not depend on which workgroup computes it or on what that workgroup
computed before, so the property needs no tolerance: with rf_debug_resident_cap(c) standing in for the resident count, every stored
tensor of every launch and every detection is bit-equal to the uncapped run -- which tests/test_launch_interval_gpu.py holds to the
float64 interval model (fp32, fp16) and tests/test_gpu_parity.py to the integer oracle (int8).

Engines: mnet25 and mnet-deconv-0517, fp32 / fp16 / int8, at 64 x 96 (every tile of every kernel partial), 96 x 160 (odd tile counts) and
352 x 608 (full, right-edge and bottom-edge tiles in one walk), three distinct frames per call.  Caps: 1 (one workgroup walks every tile
of all three images), 2 and 3 (on maps of one to six tiles per image the step G is below, at or just over a whole image: TileStep::si and
the image carry), 11 (above 8 and no multiple of 8: xcd_remap's remainder branch orders the walk).

rf_debug_grid_log proves that the caps took effect.  WALK_TILES below restates each persistent launch's tile shape from kernels.hip
(dwpw_select, conv3_select, dwpw2_kernel, SshTailCfg); the tile counts the library logs must equal the counts that table gives, so the table
that names the tile of a differing element is itself checked on every run.  The fp32 engine has NO persistent launch: its depthwise /
pointwise blocks and 3 x 3 convs launch one workgroup per tile (`sizeof(T) <= 2 ? persistent_grid(..) : nblk`), the stems and the head of
every precision as well.  Its log must therefore be EMPTY under every cap (asserted), and its equalities show that the cap touches nothing
that is not persistent.  fp16: 14 persistent launches per call, int8: 16.
"""
import json
import os
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import pytest

import launch_ref as lr
from conftest import ASSETS

pytestmark = pytest.mark.gpu

FP32, FP16, INT8 = lr.FP32, lr.FP16, 2
PNAME = {FP32: "fp32", FP16: "fp16", INT8: "int8"}
MODELS = ("mnet25", "mnet-deconv-0517")
SIZES = lr.SMALL_SIZES + (lr.BIG_SIZE,)
CAPS = (1, 2, 3, 11)
N_FRAMES = 3
RECORDS = []         # the grid log of every engine of the session, written out by test_report_tile_walk_log


@pytest.fixture(scope="module")
def rfa(built_lib):
    import retinaface_amd
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need the GPU box"
    return retinaface_amd


@pytest.fixture(scope="module", autouse=True)
def _cap_off_when_the_module_ends(built_lib):
    yield
    built_lib.rf_debug_resident_cap(0)


# ------------------------------------------------------------------------------------------------ the launches and their tiles
@dataclass
class WalkLaunch:
    name: str
    outs: List[Tuple[str, Optional[Tuple[int, int]]]]     # (blob, channel slice or None), as launch_ref.Launch.outs
    tile: Optional[Tuple[int, int]]                       # (TH, TW) of the output tile, None: not a persistent launch
    grid_of: str = ""                                     # the device launch (one grid, one log pair) this level belongs to
    head: bool = False


def _aggr1_tile(prec, hw):
    """kernels.hip conv3_select: fp16 maps of >= 48 x 48 pixels with even sides run conv3x3_up_dma_kernel (8 x 8 tiles), else 4 x 8"""
    h, w = hw[0] // 8, hw[1] // 8
    return (8, 8) if prec == FP16 and h * w >= 48 * 48 and h % 2 == 0 and w % 2 == 0 else (4, 8)


# (TH, TW) of every persistent launch, by name; dwpw<i> of the int8 engine where it differs (kernels.hip dwpw_select)
WALK_TILES = {"dwpw2(2,3)": (4, 8), "aggr0": (4, 8), "ssh.a": (8, 8), "ssh.tail": (8, 8), **{f"dwpw{i}": (4, 8) for i in range(4, 13)}}
WALK_TILES_INT8 = {"dwpw1": (8, 16), "dwpw2": (8, 16), "dwpw3": (8, 8), "dwpw12": (8, 8), **{f"dwpw{i}": (4, 16) for i in range(6, 11)}}


def walk_launches(prec: int, hw) -> List[WalkLaunch]:
    """net.cpp build_net in launch order (launch_ref.launches for fp32 / fp16; the int8 engine = the fp16 list with its own front end:
    stem -> relu2, then blocks 1 .. 3 as depthwise / pointwise launches of their own), each with the tile it walks."""
    out = []
    src = lr.launches(FP16 if prec == INT8 else prec)
    if prec == INT8:
        out.append(WalkLaunch("stem", [(lr.relu_blob(2), None)], None))
        out += [WalkLaunch(f"dwpw{i}", [(lr.relu_blob(2 * i + 2), None)], None) for i in (1, 2, 3)]
        src = [L for L in src if L.name not in ("stem2", "dwpw2(2,3)")]
    for L in src:
        out.append(WalkLaunch(L.name, list(L.outs), None, head=bool(L.head_stride)))
    for wl in out:
        if prec == FP32 or wl.head or wl.name in ("stem", "stem2"):
            continue
        if wl.name.startswith("ssh"):
            wl.grid_of = "ssh." + wl.name.split(".")[1]
            wl.tile = WALK_TILES[wl.grid_of]
        else:
            wl.grid_of = wl.name
            wl.tile = _aggr1_tile(prec, hw) if wl.name == "aggr1" else (prec == INT8 and WALK_TILES_INT8.get(wl.name)) or WALK_TILES[wl.name]
    return out


def expected_log(launches: List[WalkLaunch], blobs) -> List[Tuple[str, int, int]]:
    """(device launch, levels, tiles) of every persistent launch in launch order: tiles = images x ceil(H / TH) x ceil(W / TW) of the output
    map, summed over the levels of a multi-level launch"""
    order, tiles, levels = [], {}, {}
    for wl in launches:
        if wl.tile is None:
            continue
        n, h, w, _ = blobs[wl.outs[0][0]].shape
        if wl.grid_of not in tiles:
            order.append(wl.grid_of)
        tiles[wl.grid_of] = tiles.get(wl.grid_of, 0) + n * -(-h // wl.tile[0]) * -(-w // wl.tile[1])
        levels[wl.grid_of] = levels.get(wl.grid_of, 0) + 1
    return [(g, levels[g], tiles[g]) for g in order]


# ------------------------------------------------------------------------------------------------ running and reading an engine
def _key(res):
    return [[(d.anchor_index, d.as_row().tobytes()) for d in r] for r in res]


def _eager(rfa, stem, prec, hw):
    return rfa.RetinaFace(ASSETS, "net3", 0.4, precision=prec, net_hw=hw, model_stem=stem, keep_outputs=True, use_graph=False,
                          plan_cache=False, max_batch=8)


def _scrub_frames(frames):
    """other pictures of the same size (the frames turned by 180 degrees)"""
    return [np.ascontiguousarray(f[::-1, ::-1]) for f in frames]


def _run(rfa, det, launches, frames, prec, cap):
    """one call under `cap`: (detection keys, blob -> stored tensor of all images, grid log).  The engine's buffers keep the previous call's
    tensors, and a walk that SKIPS a tile leaves them in place: an uncapped call on other pictures comes first, so that what a skipped
    tile leaves behind is not the right answer."""
    raw = "#raw" if prec == INT8 else ""
    rfa.debug_resident_cap(0)
    det.detectBatchImages(_scrub_frames(frames), 0.5)
    rfa.debug_resident_cap(cap)
    res = det.detectBatchImages(frames, 0.5)
    log = rfa.debug_grid_log()
    blobs = {}
    for wl in launches:
        for blob, _ in wl.outs:
            if blob not in blobs:
                read = (lambda i: det.get_output(blob, i)) if wl.head else (lambda i: det.debug_activation(blob + raw, i))
                blobs[blob] = np.stack([read(i) for i in range(len(frames))])
    return _key(res), blobs, log


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _difference(wl: WalkLaunch, blob, sl, walked, plain, grid) -> Optional[str]:
    """None if the launch's share of `blob` is bit-equal, else: the first differing (image, y, x, c), both values, and the tile and edge it lies in"""
    a, b = (walked, plain) if sl is None else (walked[..., sl[0]:sl[1]], plain[..., sl[0]:sl[1]])
    bad = _bits(a) != _bits(b)
    if not bad.any():
        return None
    i0 = tuple(int(i) for i in np.argwhere(bad)[0])
    img, y, x, c = (i0[0], i0[2], i0[3], i0[1]) if wl.head else i0[:3] + (i0[3] + (sl[0] if sl else 0),)
    hh, ww = (a.shape[2], a.shape[3]) if wl.head else (a.shape[1], a.shape[2])
    where = "not a persistent launch"
    if wl.tile is not None:
        th, tw = wl.tile
        tx_n, ty_n = -(-ww // tw), -(-hh // th)
        t = (img * ty_n + y // th) * tx_n + x // tw
        edge = [e for e, on in (("right-edge partial tile", ww % tw and x // tw == tx_n - 1), ("bottom-edge partial tile", hh % th and y // th == ty_n - 1)) if on]
        where = (f"tile (ty {y // th}, tx {x // tw}) of {ty_n} x {tx_n} tiles of {th} x {tw}, tile {t} of this map's walk ({' and '.join(edge) or 'full tile'}); "
                 f"grid {grid}: a single-level launch walks it as workgroup {t % grid if grid else '?'}'s round {t // grid if grid else '?'}")
    name = blob if sl is None else f"{blob}[{sl[0]}:{sl[1]}]"
    return (f"{wl.name} -> {name}: {int(bad.sum())} of {bad.size} elements differ; first (image {img}, y {y}, x {x}, c {c}) walked {a[i0]!r} "
            f"one-tile-per-workgroup {b[i0]!r}; {where}")


def _check_log(prec, cap, log, want):
    """the cap took effect: the logged launches are the persistent ones, and none with more tiles than the cap kept one workgroup per tile"""
    assert [t for t, _ in log] == [t for _, _, t in want], (PNAME[prec], cap, log, want)
    if prec != FP32:
        assert len(log) >= 1
    for (name, levels, tiles), (_, grid) in zip(want, log):
        assert 1 <= grid <= tiles, (name, tiles, grid)
        if cap == 1:
            assert grid == 1 or (levels > 1 and grid == levels), (name, tiles, grid)
        if cap > 0:
            assert grid <= cap, (name, cap, grid)
            if tiles > cap:
                assert grid < tiles, (name, cap, tiles, grid)


def _record(stem, prec, hw, cap, want, log):
    RECORDS.append(dict(model=stem, precision=PNAME[prec], size=f"{hw[0]}x{hw[1]}", cap=cap,
                        launches=[dict(launch=n, levels=lv, tiles=t, grid=g, rounds=-(-t // g)) for (n, lv, t), (_, g) in zip(want, log)]))


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("prec", [FP32, FP16, INT8], ids=["fp32", "fp16", "int8"])
@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
@pytest.mark.parametrize("stem", MODELS)
def test_capped_walk_stores_the_bytes_of_one_tile_per_workgroup(rfa, base_frame, stem, hw, prec):
    frames = lr.case_frames(base_frame, hw)
    launches = walk_launches(prec, hw)
    tag = f"{stem} {PNAME[prec]} {hw[0]}x{hw[1]}"
    det = _eager(rfa, stem, prec, hw)
    try:
        key0, plain, log0 = _run(rfa, det, launches, frames, prec, 0)
        want = expected_log(launches, plain)
        # every tensor a launch stores and the nine head blobs; persistent launches: none (fp32), 14 (fp16), 16 (int8)
        assert len(plain) == {FP32: 37, FP16: 31, INT8: 33}[prec] and len(want) == {FP32: 0, FP16: 14, INT8: 16}[prec], (want, sorted(plain))
        _check_log(prec, 0, log0, want)
        _record(stem, prec, hw, 0, want, log0)
        print(f"{tag} production: " + ", ".join(f"{n} {t}/{g}" for (n, _, t), (_, g) in zip(want, log0)))
        failures = []
        for cap in CAPS:
            key, walked, log = _run(rfa, det, launches, frames, prec, cap)
            _check_log(prec, cap, log, want)
            _record(stem, prec, hw, cap, want, log)
            print(f"{tag} cap {cap}: " + ", ".join(f"{n} {t}/{g}" for (n, _, t), (_, g) in zip(want, log)))
            grid = {n: g for (n, _, _), (_, g) in zip(want, log)}
            for wl in launches:
                for blob, sl in wl.outs:
                    assert walked[blob].shape == plain[blob].shape
                    msg = _difference(wl, blob, sl, walked[blob], plain[blob], grid.get(wl.grid_of, 0))
                    if msg:
                        failures.append(f"{tag} cap {cap}: {msg}")
            if key != key0:
                failures.append(f"{tag} cap {cap}: detections differ from the uncapped call's")
        assert not failures, f"{len(failures)} differences\n" + "\n".join(failures[:12])
    finally:
        rfa.debug_resident_cap(0)
        det.close()


@pytest.mark.parametrize("prec", [FP32, FP16], ids=["fp32", "fp16"])
def test_cap1_walk_lies_inside_the_float64_intervals(rfa, built_lib, base_frame, prec):
    """The walked result tied to the reference directly, not only through the uncapped run: one workgroup per launch (per level), every
    stored element judged as tests/test_launch_interval_gpu.py judges the production launch."""
    from test_launch_interval_gpu import _device_blobs, consts
    stem, hw = "mnet25", lr.SMALL_SIZES[0]
    frames = lr.case_frames(base_frame, hw)
    k = consts(built_lib, ASSETS, stem, prec)
    launches = lr.launches(prec)
    det = _eager(rfa, stem, prec, hw)
    try:
        det.detectBatchImages(_scrub_frames(frames), 0.5)        # (see _run: a skipped tile must not find the right answer in place)
        rfa.debug_resident_cap(1)
        det.detectBatchImages(frames, 0.5)
        log = rfa.debug_grid_log()
        assert len(log) == (0 if prec == FP32 else 14) and all(g == 1 for _, g in log), log
        blobs = _device_blobs(det, launches, frames)
    finally:
        rfa.debug_resident_cap(0)
        det.close()
    failures = [v.message() for L in launches for v in lr.judge_launch(k, L, blobs) if not v.ok]
    assert not failures, "\n".join(failures[:8])


def test_cap1_walk_equals_the_integer_oracle(rfa, nets, base_frame):
    """int8: every activation, the raw heads, candidates and detections of the cap-1 call against oracle/int8_forward.py, as
    test_int8_engine_is_bit_exact_against_the_integer_oracle holds the production launches."""
    from oracle.int8_forward import Int8Net
    from test_gpu_parity import _assert_int8_image_bit_exact
    stem, hw = "mnet25", lr.SMALL_SIZES[0]
    frames = lr.case_frames(base_frame, hw)
    q = Int8Net(nets[stem])
    det = _eager(rfa, stem, INT8, hw)
    try:
        det.detectBatchImages(_scrub_frames(frames), 0.5)
        rfa.debug_resident_cap(1)
        res = det.detectBatchImages(frames, 0.5)
        log = rfa.debug_grid_log()
        assert len(log) == 16 and all(g == 1 for _, g in log), log
        for i in range(N_FRAMES):
            _assert_int8_image_bit_exact(det, q, i, hw, 0.5, res[i])
    finally:
        rfa.debug_resident_cap(0)
        det.close()


@pytest.mark.parametrize("prec", [FP16, INT8], ids=["fp16", "int8"])
@pytest.mark.parametrize("stem", MODELS)
def test_graph_replay_under_a_cap_equals_eager(rfa, base_frame, stem, prec):
    """A default engine created under cap 3 captures the small grids into its graph; replaying it (two calls) must return the eager
    capped engine's detections byte for byte -- which are the uncapped eager call's."""
    hw, cap = lr.SMALL_SIZES[1], 3
    frames = lr.case_frames(base_frame, hw)
    try:
        det = _eager(rfa, stem, prec, hw)
        try:
            plain = _key(det.detectBatchImages(frames, 0.5))
            det.detectBatchImages(_scrub_frames(frames), 0.5)
            rfa.debug_resident_cap(cap)
            eager = _key(det.detectBatchImages(frames, 0.5))
            log = rfa.debug_grid_log()
            assert len(log) >= 1 and all(g <= cap for _, g in log) and any(g < t for t, g in log), log
            assert eager == plain
        finally:
            det.close()
        rfa.debug_resident_cap(cap)                      # (clears the log: what follows is the graph engine's own)
        det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=prec, net_hw=hw, model_stem=stem, plan_cache=False, max_batch=8)
        try:
            first = _key(det.detectBatchImages(frames, 0.5))
            log = rfa.debug_grid_log()
            second = _key(det.detectBatchImages(frames, 0.5))
            assert len(log) >= 1 and all(g <= cap for _, g in log) and any(g < t for t, g in log), log
            assert first == eager and second == eager
        finally:
            det.close()
    finally:
        rfa.debug_resident_cap(0)


def test_report_tile_walk_log():
    """Not an assertion on the device: writes the session's grid logs (per engine and cap: launch, tiles, grid, rounds) where a run can
    collect them."""
    out = os.environ.get("RF_TILE_WALK_JSON")
    if out and RECORDS:
        with open(out, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(r) for r in RECORDS) + "\n]\n")          # one engine call per line
    walking = sum(1 for r in RECORDS if r["cap"] for L in r["launches"] if L["rounds"] > 1)
    print(f"{len(RECORDS)} engine calls logged, {walking} capped launches walked more than one round")


def test_cap_is_off_and_a_default_engine_gets_production_grids(rfa, base_frame):
    """Last test of the module: after every test's reset the cap is off; a default engine created now logs production grids -- at
    96 x 160 every launch has fewer tiles than the chip has compute units (9 per image, 72 for a full batch of 8), so one workgroup per
    tile."""
    hw = lr.SMALL_SIZES[1]
    frames = lr.case_frames(base_frame, hw)
    before = len(rfa.debug_grid_log())
    det = rfa.RetinaFace(ASSETS, "net3", 0.4, precision=FP16, net_hw=hw, model_stem="mnet25", plan_cache=False, max_batch=8)
    try:
        det.detectBatchImages(frames, 0.5)
        log = rfa.debug_grid_log()[before:]
    finally:
        det.close()
    assert len(log) >= 14 and all(g == t for t, g in log), log
