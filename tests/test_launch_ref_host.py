"""The per-launch interval judge of tests/launch_ref.py, checked on the CPU (no GPU):

  * the constants the float64 model uses are the ones the host packer exports (rf_plan_folded, the `.eq` and `stem2.*` ops), on both
    shipped models and on the derived weight sets, and the `stem2.*` ops equal an independent numpy restatement of the packer's arithmetic;
  * the judge ACCEPTS the reference: an emulation of every launch with float32 accumulation in three summation orders (natural,
    reversed, pairwise inside blocks of the MFMA K step) and the storage roundings at the model's points lies inside every interval, on
    every frame, model and weight set the GPU test runs -- the inputs chosen keep the reference itself inside the bar;
  * the judge REJECTS mutants of that emulation, each on the launch it is named for;
  * the derived weight sets meet their conditions;
  * the four-anchor heads ("net3a", the widened models of tests/net3a_models.py) are judged by the same function: their emulation is
    accepted, and rejected with two channels of anchor 2 exchanged.
"""
import numpy as np
import pytest

import launch_ref as lr
import net3a_models as nm
from conftest import ASSETS, STEMS

FP32, FP16 = lr.FP32, lr.FP16
F32, F64 = np.float32, np.float64
ORDERS = ("natural", "reversed", "blocked")


@pytest.fixture(scope="module")
def model_dirs(nets, tmp_path_factory):
    dirs = lr.weight_set_dirs(nets, ASSETS, lambda name: str(tmp_path_factory.mktemp(name)))
    dirs["net3a"] = nm.write_model_dir(nets, str(tmp_path_factory.mktemp("net3a")))
    return dirs


_consts = {}


def consts(lib, model_dir, stem, prec):
    key = (model_dir, stem, prec)
    if key not in _consts:
        _consts[key] = lr.Consts(lib, model_dir, stem, prec)
    return _consts[key]


def _judge_all(k, blobs, only=None):
    """verdicts of every launch (or of the launches named) on stored tensors"""
    return [v for L in lr.launches(k.prec) if only is None or L.name in only for v in lr.judge_launch(k, L, blobs)]


# ------------------------------------------------------------------------------------------------ packed constants
def _h(x):
    return np.asarray(x, F32).astype(np.float16)


def _np_stem2(f):
    """weights.h WeightPack<half_t>::pack, the stem2 part, restated: f(op) -> (w, b) of rf_plan_folded.  Plain Python floats are IEEE
    doubles and the sums run in the packer's order."""
    w0, b0 = f("conv0")
    dw0, dwb0 = f("dw0")
    pw0, pwb0 = f("pw0")
    dwq, dwqb = f("dw1.eq")
    pwq, pwqb = f("pw1.eq")
    w0, dw0, pw0, dwq, pwq = w0.reshape(8, 27), dw0.reshape(8, 9), pw0.reshape(16, 8), dwq.reshape(16, 9), pwq.reshape(32, 16)
    out = {}
    hi = _h(w0)
    lo = _h(w0 - hi.astype(F32))
    bm = []
    for r in range(8):
        sw = 0.0
        for k in range(27):
            sw += float(hi[r, k]) + float(lo[r, k])
        bm.append(float(b0[r]) - 1024.0 * sw)
    out["c0"] = np.array(bm).astype(F32)
    y1 = []
    for c in range(8):
        sw = 0.0
        for k in range(27):
            sw += float(w0[c, k])
        y0 = max(0.0, float(b0[c]) + 128.0 * sw)
        st = 0.0
        for t in range(9):
            st += float(dw0[c, t])
        y1.append(max(0.0, float(dwb0[c]) + y0 * st))
    mu2, mu3 = [], []
    for o in range(16):
        y2 = float(pwb0[o])
        for c in range(8):
            y2 += float(pw0[o, c]) * y1[c]
        mu2.append(float(_h(F32(min(30000.0, max(0.0, y2))))))
        st = 0.0
        for t in range(9):
            st += float(dwq[o, t])
        mu3.append(float(_h(F32(min(30000.0, max(0.0, float(dwqb[o]) + mu2[o] * st))))))
    floor = lambda mu: np.array([0.0 if m == 0.0 else -m for m in mu]).astype(np.float16).astype(F32)
    out["floor2"], out["floor3"] = floor(mu2), floor(mu3)
    out["c2"] = pwb0 - np.array(mu2, F32)                                           # float32 arithmetic, as the packer
    taps16 = _h(dwq)
    b3 = []
    for c in range(16):
        st = 0.0
        for t in range(9):
            st += float(taps16[c, t])
        b3.append(float(dwqb[c]) + mu2[c] * st - mu3[c])
    out["c3"], out["c3.w"] = np.array(b3).astype(F32), taps16.astype(F32).reshape(16, 3, 3, 1)
    ph = _h(pwq)
    pl = _h(pwq - ph.astype(F32))
    b4 = []
    for o in range(32):
        corr = 0.0
        for k in range(16):
            corr += (float(ph[o, k]) + float(pl[o, k])) * mu3[k]
        b4.append(float(pwqb[o]) + corr)
    out["c4"] = np.array(b4).astype(F32)
    return out


@pytest.mark.parametrize("ws", lr.WEIGHT_SETS)
@pytest.mark.parametrize("stem", STEMS)
def test_packed_constants_are_the_packer_exports(built_lib, model_dirs, stem, ws):
    """(1) Every `dw<i>.eq` / `pw<i>.eq` pair is a pure re-scaling of the folded block (test_host.py's equalisation check, here on every
    block of every weight set): taps and bias / t, pointwise column * t, 1 <= t < 2, pointwise bias untouched.  (2) The fp16 model holds
    exactly their nearest-even halves, and the fp16 hi + lo pairs where the packer makes them.  (3) The `stem2.*` ops -- constants that exist
    only inside the packed image -- equal the numpy restatement of the packer bit for bit, and their weights are the folded ones."""
    d = model_dirs[ws]
    f = lambda op: lr.folded(built_lib, d, stem, op)
    k16, k32 = consts(built_lib, d, stem, FP16), consts(built_lib, d, stem, FP32)
    for i in range(1, 13):
        (dw, db), (pw, pb), (dwe, dbe), (pwe, pbe) = f(f"dw{i}"), f(f"pw{i}"), f(f"dw{i}.eq"), f(f"pw{i}.eq")
        c = dw.shape[0]
        d9, e9 = dw.reshape(c, 9).astype(F64), dwe.reshape(c, 9).astype(F64)
        live = np.abs(d9).max(1) > 1e-20
        j = np.abs(d9).argmax(1)
        t = np.where(live, d9[np.arange(c), j] / np.where(live, e9[np.arange(c), j], 1.0), 1.0)
        assert (t >= 1.0 - 1e-6).all() and (t < 2.0).all(), (ws, stem, i)
        assert np.allclose(e9 * t[:, None], d9, rtol=2e-7, atol=1e-30)
        assert np.allclose(dbe.astype(F64) * t, db, rtol=2e-7, atol=1e-30)
        assert np.allclose(pwe.reshape(-1, c), pw.reshape(-1, c).astype(F64) * t[None, :], rtol=2e-7, atol=1e-30) and np.array_equal(pbe, pb)
        if i >= 2:
            assert np.array_equal(k16.ops[f"dw{i}"].w, _h(dwe).astype(F64)) and np.array_equal(k16.ops[f"dw{i}"].b, dbe.astype(F64))
            assert np.array_equal(k16.ops[f"pw{i}"].w, _h(pwe).astype(F64)) and np.array_equal(k16.ops[f"pw{i}"].b, pbe.astype(F64))
        assert np.array_equal(k32.ops[f"dw{i}"].w, dw.astype(F64)) and np.array_equal(k32.ops[f"pw{i}"].w, pw.astype(F64))
    for i in range(3):
        w, b = f(f"ssh{i}.head")
        hi = _h(w)
        lo = _h(w - hi.astype(F32))
        assert np.array_equal(k16.ops[f"ssh{i}.head"].w, hi.astype(F64) + lo.astype(F64)) and k16.ops[f"ssh{i}.head"].K == 129
        assert np.abs(k16.ops[f"ssh{i}.head"].w - w).max() <= 2.0 ** -21 * max(np.abs(w).max(), 2.0 ** -14)
    ref = _np_stem2(f)
    for op, wsrc in (("c0", "conv0"), ("c2", "pw0"), ("c4", "pw1.eq")):
        w, b = f("stem2." + op)
        assert np.array_equal(w, f(wsrc)[0]), op
        assert np.array_equal(b, ref[op]), (ws, stem, op, b, ref[op])
    w, b = f("stem2.c3")
    assert np.array_equal(w, ref["c3.w"]) and np.array_equal(b, ref["c3"]), (ws, stem, "c3")
    for op in ("floor2", "floor3"):
        w, b = f("stem2." + op)
        assert w.shape == (16, 1, 1, 1) and np.array_equal(w.reshape(-1), ref[op]) and np.array_equal(b, ref[op]), (ws, stem, op)
        assert (b <= 0).all()
    # and the model holds them: the centred tiles' floors, the -mu2 padding of conv3's input, the hi / lo pairs
    s2 = k16.ops
    assert np.array_equal(s2["s2.c2"].floor, ref["floor2"]) and np.array_equal(s2["s2.c3"].pad, ref["floor2"]) and np.array_equal(s2["s2.c3"].floor, ref["floor3"])
    w0 = f("conv0")[0]
    assert np.array_equal(s2["s2.c0"].w[..., :3], _h(w0).astype(F64)) and np.array_equal(s2["s2.c0"].w[..., 3:], _h(w0 - _h(w0).astype(F32)).astype(F64))
    assert s2["s2.c0"].K == 55 and s2["s2.c2"].K == 25 and s2["s2.c4"].K == 33 and s2["s2.c1"].K == 10
    with pytest.raises(AssertionError):
        f("stem2.nothing")


# ------------------------------------------------------------------------------------------------ the judge accepts the reference
CASES = [("shipped", s, hw) for s, hw in lr.SHIPPED_CASES] + [(ws, s, hw) for ws in ("degenerate", "ragged") for s, hw in lr.DERIVED_CASES]


@pytest.mark.parametrize("prec", [FP32, FP16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("ws,stem,hw", CASES, ids=[f"{ws}-{s}-{h}x{w}" for ws, s, (h, w) in CASES])
def test_the_judge_accepts_the_float32_emulation_in_three_summation_orders(built_lib, model_dirs, base_frame, ws, stem, hw, prec):
    k = consts(built_lib, model_dirs[ws], stem, prec)
    frames = lr.case_frames(base_frame, hw)
    for order in ORDERS:
        blobs = lr.emulate(k, frames, order)
        bad = [v.message() for v in _judge_all(k, blobs) if not v.ok]
        assert not bad, (order, bad[:4])


# ------------------------------------------------------------------------------------------------ the judge rejects mutants
MUTANTS = [
    # (label, precision, mutant, launch that must reject it)
    ("stores rounded toward zero, dw of block 7", FP16, lr.Mutant("rtz", "dw7"), "dwpw7"),
    ("stores rounded toward zero, pw of block 7", FP16, lr.Mutant("rtz", "pw7"), "dwpw7"),
    ("one tap of a border pixel dropped, rf_c1_aggr", FP16, lr.Mutant("drop_tap", "aggr1", (1, 0, 5, 7)), "aggr1"),
    ("one tap of a border pixel dropped, rf_c1_aggr", FP32, lr.Mutant("drop_tap", "aggr1", (1, 0, 5, 7)), "aggr1"),
    ("conv0's lo half dropped", FP16, lr.Mutant("drop_lo", "s2.c0"), "stem2"),
    ("one depthwise channel of block 6 left unequalised", FP16, lr.Mutant("raw_dw_channel", "dw6", (37,)), "dwpw6"),
    ("two adjacent output channels of a lateral swapped", FP16, lr.Mutant("swap_channels", "lateral1", (20,)), "dwpw10"),
    ("two adjacent output channels of a lateral swapped", FP32, lr.Mutant("swap_channels", "lateral1", (20,)), "dwpw10"),
    ("upsample taps 0.25 / 0.75 swapped on the y axis, rf_c2_aggr", FP16, lr.Mutant("swap_up_taps", "plus0", (0,)), "aggr0"),
    ("upsample taps 0.25 / 0.75 swapped on the x axis, rf_c2_aggr", FP32, lr.Mutant("swap_up_taps", "plus0", (1,)), "aggr0"),
    ("ReLU before the centred floor instead of the floor", FP16, lr.Mutant("relu_before_floor", "s2.c2"), "stem2"),
    ("last image of the batch taken from image 0", FP16, lr.Mutant("last_image", "ssh1.tail"), "ssh1.tail"),
    ("last image of the batch taken from image 0", FP32, lr.Mutant("last_image", "dwpw3"), "dwpw3"),
]


@pytest.mark.parametrize("label,prec,mutant,launch", MUTANTS, ids=[f"{'fp32' if p == FP32 else 'fp16'}-{m.kind}-{m.tag}" for _, p, m, _ in MUTANTS])
def test_the_judge_rejects_the_mutant_on_its_launch(built_lib, base_frame, label, prec, mutant, launch):
    """Each mutant is applied to the emulation (blocked order) of mnet25 at 64 x 96; the launch named must have at least one element
    outside its interval, and the launches BEFORE it -- which the mutant does not touch -- must stay inside."""
    k = consts(built_lib, ASSETS, "mnet25", prec)
    raw = None
    if mutant.kind == "raw_dw_channel":
        # the folded (unequalised) depthwise stage, its taps rounded to half as the packer would
        w, b = lr.folded(built_lib, ASSETS, "mnet25", mutant.tag)
        assert not np.array_equal(_h(w).astype(F64)[mutant.arg[0]], k.ops[mutant.tag].w[mutant.arg[0]]), "the channel chosen is equalised with t = 1"

        class Raw:
            ops = {mutant.tag: lr.Op(_h(w).astype(F64), b.astype(F64), "dw", 1, 10)}
        raw = Raw
    frames = lr.case_frames(base_frame, (64, 96))
    blobs = lr.emulate(k, frames, "blocked", mutant, raw)
    names = [L.name for L in lr.launches(prec)]
    before = names[:names.index(launch)]
    assert all(v.ok for v in _judge_all(k, blobs, only=before)), label
    verdicts = _judge_all(k, blobs, only=(launch,))
    failed = [v for v in verdicts if not v.ok]
    assert failed, label
    msg = failed[0].message()
    assert launch in msg and "first (image" in msg and "interior" in msg
    if mutant.kind == "drop_tap":
        img, y, x, _ = mutant.arg
        assert failed[0].first[0][:3] == (img, y, x) and failed[0].where["border row or column"] == failed[0].n_fail
    if mutant.kind == "last_image":
        assert failed[0].where["images"] == [2]


# ------------------------------------------------------------------------------------------------ the derived sets
@pytest.mark.parametrize("stem,hw", lr.DERIVED_CASES, ids=[f"{s}-{h}x{w}" for s, (h, w) in lr.DERIVED_CASES])
def test_ragged_meets_its_conditions(built_lib, nets, model_dirs, base_frame, stem, hw):
    """Output rows of every convolution scaled by a seeded power of two; on the GPU test's frames, in the float64 model of either
    precision: every activation finite and below 2^14, at most 90 % of any launch's outputs exactly 0."""
    net, rag = nets[stem], lr.derive_ragged(nets[stem])
    n_scaled = 0
    for a, b in zip(net.layers, rag.layers):
        if a.type == "Convolution":
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(a.blobs[0] != 0, b.blobs[0] / np.where(a.blobs[0] != 0, a.blobs[0], 1), np.nan)
            rows = ratio.reshape(ratio.shape[0], -1)
            first = np.nanmax(rows, axis=1)
            assert np.all((rows == first[:, None]) | np.isnan(rows)) and set(np.unique(first[~np.isnan(first)])) <= set(lr.RAGGED_EXPONENTS), a.name
            n_scaled += int((first != 1).sum())
            assert all(np.array_equal(x, y) for x, y in zip(a.blobs[1:], b.blobs[1:]))
        else:
            assert all(np.array_equal(x, y) for x, y in zip(a.blobs, b.blobs)), a.name
    assert n_scaled > 100
    frames = lr.case_frames(base_frame, hw)
    for prec in (FP32, FP16):
        k = consts(built_lib, model_dirs["ragged"], stem, prec)
        blobs = lr.model_forward(k, frames)
        for L in lr.launches(prec):
            outs = [blobs[b] if sl is None else blobs[b][..., sl[0]:sl[1]] for b, sl in L.outs]
            assert all(np.isfinite(o).all() for o in outs), L.name
            assert max(float(np.abs(o).max()) for o in outs) < 2.0 ** 14, L.name
            if not L.head_stride:
                zeros = sum(int((o == 0).sum()) for o in outs) / sum(o.size for o in outs)
                assert zeros <= 0.9, (L.name, zeros)


@pytest.mark.parametrize("stem", STEMS)
def test_degenerate_reaches_the_float_models_cold_branches(built_lib, nets, model_dirs, base_frame, stem):
    """tests/int8_derived.py `degenerate` as the float engines see it: all-zero weight rows and depthwise taps survive the fold (and the
    equalisation leaves an all-zero channel alone), the beta = 1e4 channels sit at ~1e4 everywhere, and every activation stays finite in fp16."""
    from int8_derived import degenerate_edits
    ed = degenerate_edits(nets[stem])
    k = consts(built_lib, model_dirs["degenerate"], stem, FP16)
    ch = ed["mobilenet0_conv9_fwd:zero"]                       # depthwise of block 4
    assert not k.ops["dw4"].w[ch].any()
    assert not k.ops["lateral1"].w[ed["rf_c2_lateral:zero"]].any() and not k.ops["aggr1"].w[ed["rf_c1_aggr:zero"]].any()
    blobs = lr.model_forward(k, lr.case_frames(base_frame, (64, 96)))
    assert all(np.isfinite(v).all() for v in blobs.values())
    hot = blobs[lr.relu_blob(12)][..., ed["mobilenet0_conv12_fwd:beta"]]
    assert hot.min() > 5e3 and hot.max() < 6e4


# ------------------------------------------------------------------------------------------------ four anchors per cell
HEADS = ("head0", "head1", "head2")
NET3A_CASES = [(s, hw) for s in STEMS for hw in lr.SMALL_SIZES]


@pytest.mark.parametrize("prec", [FP32, FP16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("stem,hw", NET3A_CASES, ids=[f"{s}-{h}x{w}" for s, (h, w) in NET3A_CASES])
def test_the_judge_accepts_the_emulated_four_anchor_heads(built_lib, model_dirs, base_frame, stem, hw, prec):
    """The widened models: 64 head channels per stride (K = 65, fp16: the hi + lo pair, K = 129), softmax over (a, A + a) with A = 4.  The
    emulation's head launches lie inside their intervals in all three summation orders, on the frames and sizes the GPU test judges;
    every anchor number has a probability above 0.5 and above 0.02 somewhere, so the intervals of all four softmax pairs are judged on
    both sides of the thresholds."""
    k = consts(built_lib, model_dirs["net3a"], stem, prec)
    assert k.anchors == 4 and k.ops["ssh0.head"].w.shape[0] == 64 and k.ops["ssh0.head"].K == (129 if prec == FP16 else 65)
    frames = lr.case_frames(base_frame, hw)
    for order in ORDERS:
        blobs = lr.emulate(k, frames, order)
        verdicts = _judge_all(k, blobs, only=HEADS)
        assert len(verdicts) == 9 and all(v.ok for v in verdicts), (order, [v.message() for v in verdicts if not v.ok][:4])
        probs = [blobs[lr.head_names(s)[0]] for s in lr.STRIDES]
        assert probs[0].shape[1] == 8
        for thr in (0.5, 0.02):
            assert nm.anchors_with_candidates(probs, thr) == {0, 1, 2, 3}, (order, thr)


@pytest.mark.parametrize("prec", [FP32, FP16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("c,blob", [(8 + 2 * 4, "bbox_pred"), (24 + 2 * 10 + 1, "landmark_pred"), (4 + 2, "cls_prob")])
def test_the_judge_rejects_exchanged_channels_of_anchor_2(built_lib, model_dirs, base_frame, prec, c, blob):
    """Head channels c and c + 1 of the stride-8 head exchanged in the emulation (dx / dy of anchor 2; y0 / x1 of its landmarks; the
    foreground logits of anchors 2 and 3): head2 rejects it on the blob named, head0 and head1 stay inside."""
    k = consts(built_lib, model_dirs["net3a"], "mnet25", prec)
    blobs = lr.emulate(k, lr.case_frames(base_frame, (64, 96)), "blocked", lr.Mutant("swap_channels", "ssh2.head", (c,)))
    assert all(v.ok for v in _judge_all(k, blobs, only=("head0", "head1")))
    failed = [v for v in _judge_all(k, blobs, only=("head2",)) if not v.ok]
    assert failed and all(blob in v.blob for v in failed), [v.message() for v in failed]
