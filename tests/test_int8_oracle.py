"""Pin the integer-exact int8 oracle (oracle/int8_forward.py) on the CPU: known answers for its float epilogue, its two conv
back-ends against each other, its upsample + add against the Caffe-semantics deconvolution of the fp32 oracle, and the whole
int8 network against the fp32 oracle (quantisation noise only).  The GPU engine is then held BIT-exact to it (-m gpu)."""
import os

import numpy as np
import pytest

from conftest import STEMS
from oracle import int8_forward as i8
from oracle.caffe_forward import _deconv2d_numpy
from oracle.retinaface_post import decode, iou_plus1, nms, preprocess_trt_identity


def _requant(acc, mult, bias, relu=True):
    acc = np.asarray(acc, np.int32).reshape(1, -1, 1)
    n = acc.shape[1]
    out = np.empty((1, n, 1), np.int8)
    for k in range(n):      # one channel per call so every entry can have its own (mult, bias)
        a = np.ascontiguousarray(acc[:, k:k + 1])
        o = i8.Int8Net._requant(a, np.array([mult[k]], np.float32), np.array([bias[k]], np.float32), relu)
        out[0, k, 0] = o[0, 0, 0]
    return out.reshape(-1).tolist()


def test_requantisation_known_answers():
    """y = fmaf(acc, mult, bias) with ONE rounding, then round-half-even of the clamped value."""
    f = float.fromhex
    # ties go to the even integer; negative -> 0 (ReLU); saturation at 127; -127 floor without ReLU
    assert _requant([5, 7, 9, -3, 1000, 254], [0.5] * 6, [0.0] * 6) == [2, 4, 4, 0, 127, 127]
    assert _requant([-5, -7, -1000, 5], [0.5] * 4, [0.0] * 4, relu=False) == [-2, -4, -127, 2]
    # vectors where fl(fl(acc * mult) + bias) and fmaf(acc, mult, bias) land on different sides of k + 0.5 (found by search):
    # the oracle and the kernels (v_fma_f32) take the fused value
    cases = [(95164, f("0x1.391236p-7"), f("-0x1.a7db4ep+9"), 61, 62), (129121, f("0x1.472a02p-10"), f("-0x1.7a96aap+6"), 66, 67),
             (180870, f("0x1.b88268p-9"), f("-0x1.232f8ep+9"), 25, 26), (150071, f("0x1.ed08d6p-8"), f("-0x1.fac014p+9"), 115, 116)]
    for acc, m, b, fused, unfused in cases:
        assert _requant([acc], [m], [b]) == [fused]
        two_step = np.float32(np.float32(np.float32(acc) * np.float32(m)) + np.float32(b))
        assert int(np.rint(two_step)) == unfused
    # depthwise outputs (round 6): ReLU'd quanta 0..255 stored minus 128 (relu = 2): ties to even, saturation at 255, negatives -> 0
    assert _requant([5, 7, -3, 1000, 509, 511, 256], [0.5] * 7, [0.0] * 7, relu=2) == [2 - 128, 4 - 128, -128, 127, 254 - 128, 127, 0]
    # int32 -> float conversion of the accumulator rounds to nearest even above 2**24 (15-bit depthwise taps reach 1.9e7)
    assert _requant([2 ** 24 + 1, 2 ** 24 + 3], [2.0 ** -18] * 2, [0.0] * 2) == [64, 64]


def test_integer_blend_equals_caffe_deconv_plus_eltwise(nets):
    """rfi8_upadd mode 1 (integers, round half to even on the total) == rint(Deconvolution(k4 s2 p1 g, bilinear weights) + Crop +
    Eltwise SUM) computed with the fp32 oracle's own transposed convolution on the same quanta; mode 0 (fp32 form) with unit
    scale ratios agrees with it bit for bit, and with non-unit ratios follows fmaf(lat, a_lat, blend * a_up)."""
    rng = np.random.default_rng(5)
    net = i8.Int8Net(nets["mnet25"])
    h, w, c = 10, 14, 64
    lat = rng.integers(0, 128, (h, w, c)).astype(np.int8)
    up = rng.integers(0, 128, (h // 2, w // 2, c)).astype(np.int8)
    k1 = np.array([0.25, 0.75, 0.75, 0.25], np.float32)
    wdec = np.tile(np.outer(k1, k1)[None, None], (c, 1, 1, 1)).astype(np.float32)          # [cin][cout/g = 1][4][4]
    dec = _deconv2d_numpy(up.transpose(2, 0, 1)[None].astype(np.float32), wdec, None, 2, 1, c)[0].transpose(1, 2, 0)
    want = np.minimum(np.rint(dec.astype(np.float64) + lat), 127).astype(np.int8)         # multiples of 1/16: exact, half to even
    out = np.empty_like(lat)
    i8.lib().rfi8_upadd(lat.ctypes.data, up.ctypes.data, h, w, c, 1.0, 1.0, 1, out.ctypes.data)
    assert np.array_equal(out, want)
    out0 = np.empty_like(lat)
    i8.lib().rfi8_upadd(lat.ctypes.data, up.ctypes.data, h, w, c, 1.0, 1.0, 0, out0.ctypes.data)
    assert np.array_equal(out0, want)
    a_lat, a_up = np.float32(0.7312), np.float32(1.318)
    i8.lib().rfi8_upadd(lat.ctypes.data, up.ctypes.data, h, w, c, float(a_lat), float(a_up), 0, out0.ctypes.data)
    real = lat.astype(np.float64) * float(a_lat) + dec.astype(np.float64) * float(a_up)
    assert np.abs(out0 - np.clip(real, -127, 127)).max() <= 0.5 + 1e-4
    assert net.per_channel and net.a_lat == [1.0, 1.0]


@pytest.mark.parametrize("stem", STEMS)
def test_int8_conv_backends_agree_exactly(nets, stem):
    """float64 BLAS convolution (exact: every partial sum is an integer below 2**53) vs the plain C loops, every activation of
    the network, on random quanta at a 64 x 96 net size."""
    rng = np.random.default_rng(11)
    x = rng.integers(0, 128, (32, 48, 16)).astype(np.int8)
    a = i8.Int8Net(nets[stem], backend="blas").forward_from("mobilenet0_relu2_fwd", x)
    b = i8.Int8Net(nets[stem], backend="c").forward_from("mobilenet0_relu2_fwd", x)
    assert set(a) == set(b) and len(a) > 40
    for k in a:
        if k == "__heads__":
            for hk in a[k]:
                assert np.array_equal(a[k][hk], b[k][hk]), hk
        else:
            assert a[k].dtype == np.int8 and np.array_equal(a[k], b[k]), k
    # later starting points continue identically (the engine's fused front end hands over at relu4)
    c = i8.Int8Net(nets[stem]).forward_from("mobilenet0_relu4_fwd", a["mobilenet0_relu4_fwd"])
    assert all(np.array_equal(c[k], a[k]) for k in c if k != "__heads__")


@pytest.mark.parametrize("stem", STEMS)
def test_int8_oracle_tracks_the_fp32_oracle(nets, oracles, stem):
    """The int8 definition is sane: fed the fp32 oracle's own first block output, it finds the same faces (IoU / anchor
    agreement at the level the engine's INT8_BAR documents) and every layer stays within a few percent of the range."""
    from retinaface_amd.frames import synth_frames
    q = i8.Int8Net(nets[stem])
    ious, same_anchor, faces = [], 0, 0
    for f in synth_frames(448, 448, 4, config=300, faces=[1, 3, 5]):
        blobs = oracles[stem].forward(preprocess_trt_identity(f, 448, 448), keep_all=True)
        x = q.quantise_blob("mobilenet0_relu2_fwd", blobs["mobilenet0_relu2_fwd"][0].transpose(1, 2, 0))
        acts = q.forward_from("mobilenet0_relu2_fwd", x)
        for n in ("mobilenet0_relu10_fwd", "mobilenet0_relu26_fwd", "rf_c1_aggr_relu", "rf_c2_det_concat_relu"):
            r = blobs[n][0].transpose(1, 2, 0)
            a = acts[n].astype(np.float32) * q.scale_of_blob[n]
            assert np.abs(a - np.minimum(r, a.max())).mean() <= 0.035 * max(1.0, float(np.abs(r).max())), n
        heads = {k: v[None] for k, v in acts["__heads__"].items()}
        got = nms(list(decode(heads, 448, 448, 0.5)), 0.4)
        ref = oracles[stem].detect(f, 0.5, 0.4, net_hw=(448, 448)).detections
        assert len(got) == len(ref)
        for r in ref:
            best = max(got, key=lambda g: iou_plus1(g.rect, r.rect))
            ious.append(iou_plus1(best.rect, r.rect))
            same_anchor += best.anchor_index == r.anchor_index
            faces += 1
    assert faces >= 4 and min(ious) >= 0.85 and same_anchor / faces >= 0.5, (min(ious), same_anchor, faces)


def test_per_channel_table_with_equal_channels_equals_the_per_tensor_table(nets):
    """The per-channel extension of the table format (`blob#c` lines) must reduce to the TensorRT per-tensor semantics when every
    channel carries the tensor's scale -- except for the FPN adds, where per-channel tables give the three tensors of an add one
    common scale (the largest) and blend in integers: with equal scales for all three the two blends are the same function, so the
    whole network must agree activation for activation."""
    import copy
    from conftest import ASSETS
    from oracle.caffe_io import read_int8_table
    net = copy.deepcopy(nets["mnet-deconv-0517"])
    net.int8_qweights = {}            # the per-tensor table is the reference's TensorRT cache (assets/mnet-deconv-0517.table.int8), rounded to nearest
    net.int8_scales = read_int8_table(os.path.join(ASSETS, "mnet-deconv-0517.table.int8"))
    base = dict(net.int8_scales)
    # force the three tensors of each add to one per-tensor scale, so that the per-tensor engine's ratios are exactly 1
    for group in (("rf_c3_lateral_relu", "rf_c2_lateral_relu", "_plus0"), ("rf_c2_aggr_relu", "rf_c1_red_conv_relu", "_plus1")):
        m = max(base[g] for g in group)
        for g in group:
            base[g] = m
    net.int8_scales = dict(base)
    per_tensor = i8.Int8Net(net)
    assert not per_tensor.per_channel and per_tensor.a_lat == [1.0, 1.0] and per_tensor.a_up == [1.0, 1.0]
    chans = {"_plus0": 64, "_plus1": 64}
    for i in range(13):
        c = i8.Int8Net.BLOCK_COUT[i]
        chans[f"mobilenet0_relu{2 * i + 2}_fwd"] = c
        chans[f"mobilenet0_relu{2 * i + 1}_fwd"] = 8 if i == 0 else i8.Int8Net.BLOCK_COUT[i - 1]
    for n in ("rf_c3_lateral_relu", "rf_c2_lateral_relu", "rf_c1_red_conv_relu", "rf_c2_aggr_relu", "rf_c1_aggr_relu"):
        chans[n] = 64
    for c in (3, 2, 1):
        chans[f"rf_c{c}_det_concat_relu"] = 64
        chans[f"rf_c{c}_det_context_conv1_relu"] = 16
        chans[f"rf_c{c}_det_context_conv3_1_relu"] = 16
    wide = dict(base)
    for n, c in chans.items():
        for k in range(c):
            wide[f"{n}#{k}"] = base[n]
    net2 = copy.deepcopy(net)
    net2.int8_scales = wide
    per_channel = i8.Int8Net(net2)
    assert per_channel.per_channel
    rng = np.random.default_rng(23)
    x = rng.integers(0, 128, (32, 48, 16)).astype(np.int8)
    a = per_tensor.forward_from("mobilenet0_relu2_fwd", x)
    b = per_channel.forward_from("mobilenet0_relu2_fwd", x)
    for k in a:
        if k == "__heads__":
            assert all(np.array_equal(a[k][h], b[k][h]) for h in a[k])
        else:
            assert np.array_equal(a[k], b[k]), k


def test_u8_mid_algebra_and_calibrated_weights(nets):
    """A pointwise conv whose input is a depthwise mid stored as q - 128: sum_k w_q (q - 128) with the bias fmaf(mult, 128 * sum_k w_q, bias)
    is the conv over the unsigned quanta (exact integers; one extra fp32 rounding in the bias), the mid's scale is the table's x fp32(127/255),
    and calibrated weights replace the rounding but not the grid."""
    rng = np.random.default_rng(3)
    w = rng.standard_normal((32, 1, 1, 16)).astype(np.float32) * 0.1
    b = rng.standard_normal(32).astype(np.float32)
    s_in = rng.uniform(0.01, 0.05, 16).astype(np.float32)
    s_out = rng.uniform(0.02, 0.06, 32).astype(np.float32)
    g = i8.QGemm(w, b, s_in, s_out, in_u8=True)
    plain = i8.QGemm(w, b, (s_in * i8.MID_U8).astype(np.float32), s_out)
    assert np.array_equal(g.wq, plain.wq) and np.array_equal(g.mult, plain.mult)
    q = rng.integers(0, 256, (5, 7, 16))
    acc_u = np.einsum("hwk,ok->hwo", q, plain.wq.reshape(32, 16))
    acc_s = np.einsum("hwk,ok->hwo", q - 128, g.wq.reshape(32, 16))
    y_u = acc_u * plain.mult.astype(np.float64) + plain.bias.astype(np.float64)
    y_s = acc_s * g.mult.astype(np.float64) + g.bias.astype(np.float64)
    assert np.abs(y_u - y_s).max() <= 4e-6 * max(1.0, float(np.abs(y_u).max()))          # the only difference: fp32 rounding of the folded bias
    # calibrated integers: taken as they are, same multipliers, bias shifted by bias_delta / s_out
    cq = np.clip(plain.wq.reshape(32, 16) + rng.integers(-1, 2, (32, 16)), -127, 127).astype(np.int8)
    db = rng.standard_normal(32).astype(np.float32) * 0.01
    c = i8.QGemm(w, b, s_in, s_out, calibrated=(cq, db))
    n = i8.QGemm(w, b, s_in, s_out)
    assert np.array_equal(c.wq.reshape(32, 16), cq) and np.array_equal(c.mult, n.mult)
    assert np.array_equal(c.bias, ((b + db).astype(np.float32) / s_out).astype(np.float32))
    # the shipped models carry calibrated weights for every fused dense conv, all inside the int8 grid, and they differ from plain rounding
    for stem in STEMS:
        net = nets[stem]
        assert len(net.int8_qweights) == 29
        q8 = i8.Int8Net(net)
        import copy
        rtn = copy.copy(net)
        rtn.int8_qweights = {}
        q0 = i8.Int8Net(rtn)
        moved = np.mean([np.mean(a.wq != b.wq) for a, b in zip(q8.pw[1:], q0.pw[1:])])
        assert 0.03 < moved < 0.4, moved
        assert all(np.abs(a.wq - b.wq).max() <= 3 for a, b in zip(q8.pw[1:], q0.pw[1:]))


def test_variant_frames_drive_the_int8_epilogues_into_their_top_clamp(nets, oracles):
    """Every requantising epilogue of the int8 engine clamps at the top code: fmed3(v, 0, 127) + v_cvt_pk_u8_f32 for block outputs, FPN
    and SSH tensors, and the 0..255 depthwise mid store (q - 128), which relies on the conversion's own clamp.  On the plain contract
    frames those clamps are almost never reached, so the GPU's bit-exactness against this oracle says little about them.  The frames of
    tests/frame_variants.py (fed to the GPU's int8 bit-exact test) must reach them: on the first frame of every variant, continued from
    the quantised fp32 front end as the engine is, at least one variant puts >= 0.1 % of some block output's quanta at 127, and at least
    one does so for a depthwise intermediate."""
    import frame_variants as fv
    start = "mobilenet0_relu2_fwd"            # the int8 engine's first int8 activation
    best_block, best_dw = (0.0, ""), (0.0, "")
    for stem in STEMS:
        q = i8.Int8Net(nets[stem])
        for name in fv.ALL:
            f = fv.variant_frames(name, 1)[0]
            blobs = oracles[stem].forward(preprocess_trt_identity(f, *fv.HW), keep_all=True)
            acts = q.forward_from(start, q.quantise_blob(start, blobs[start][0].transpose(1, 2, 0)))
            top_b, top_d = (0.0, ""), (0.0, "")
            for n, a in acts.items():
                if n in ("__heads__", start) or n.startswith("_plus"):
                    continue
                frac = (float((a == 127).mean()), f"{stem} {name} {n}")
                dw = n.startswith("mobilenet0_relu") and int(n[len("mobilenet0_relu"):].split("_")[0]) % 2 == 1
                if dw:
                    top_d = max(top_d, frac)
                else:
                    top_b = max(top_b, frac)
            print(f"int8 top code {stem} {name:8s}: block / FPN / SSH {top_b[0]:.5f} ({top_b[1].split()[-1]}), depthwise {top_d[0]:.5f} ({top_d[1].split()[-1]})")
            best_block, best_dw = max(best_block, top_b), max(best_dw, top_d)
    assert best_block[0] >= 1e-3, best_block
    assert best_dw[0] >= 1e-3, best_dw


# ------------------------------------------------------------------------------------------------ derived tables and weight sets
# tests/int8_derived.py: the branches of the int8 path that the shipped tables (25 % head-room) and the trained weights leave cold.
# Here: the conditions on the INPUTS of tests/test_int8_derived_gpu.py (checked on the reference alone), the C++ packer against the
# oracle on every derived set, and the refusal of unusable scales.

import ctypes as C  # noqa: E402

import int8_derived as drv  # noqa: E402
from conftest import ASSETS  # noqa: E402
from test_gpu_parity import _edge_frame  # noqa: E402  (the GPU tests' own frame; importing that module needs no GPU)

COVERAGE_HW = (352, 608)          # at 64 x 96 one or two tensors stay unsaturated under the same tables
START = "mobilenet0_relu2_fwd"


def _is_mid(name):
    return name.startswith("mobilenet0_relu") and int(name[len("mobilenet0_relu"):].split("_")[0]) % 2 == 1


@pytest.fixture(scope="module")
def coverage_blobs(oracles, base_frame):
    """the fp32 oracle's activations on the coverage frame, once per model"""
    f = _edge_frame(base_frame, COVERAGE_HW)
    return {stem: oracles[stem].forward(preprocess_trt_identity(f, *COVERAGE_HW), keep_all=True) for stem in STEMS}


def _continue_from_fp32(q, blobs):
    return q.forward_from(START, q.quantise_blob(START, blobs[START][0].transpose(1, 2, 0)))


def _top_code_report(stem, name, acts):
    """(share of top codes per tensor, printed summary): 127 is the top code of every tensor -- a depthwise mid's 255 is stored as 127"""
    share = {n: float((a == 127).mean()) for n, a in acts.items() if n != "__heads__"}
    relu = [v for n, v in share.items() if not _is_mid(n)]
    mids = [v for n, v in share.items() if _is_mid(n)]
    quanta = sum(a.size for n, a in acts.items() if n != "__heads__")
    total = sum(int((a == 127).sum()) for n, a in acts.items() if n != "__heads__") / quanta
    low = min(share, key=share.get)
    print(f"int8 derived {stem} {name}: {total:.4f} of all quanta at the top code; ReLU tensors mean {np.mean(relu):.4f}, depthwise mids mean "
          f"{np.mean(mids):.4f}; lowest {share[low]:.5f} ({low})")
    return share


@pytest.mark.parametrize("name", ["pc_half", "pt_quarter"])
@pytest.mark.parametrize("stem", STEMS)
def test_derived_tables_put_every_int8_tensor_at_its_top_code(nets, coverage_blobs, stem, name):
    """Under `pc_half` (per-channel path) and `pt_quarter` (per-tensor path), on the GPU test's own 352 x 608 frame continued from the
    quantised fp32 front end, EVERY int8 tensor of the network -- the 28 ReLU tensors behind the start blob, `_plus0` / `_plus1` included,
    and all 12 depthwise mids -- has quanta at its top code, so a bit-exact pass of the engine on these tables exercises the top clamp of
    every requantising epilogue.  A condition on the inputs, checked on the reference alone."""
    q = i8.Int8Net(drv.derive(nets[stem], name))
    assert q.per_channel == name.startswith("pc_")
    acts = _continue_from_fp32(q, coverage_blobs[stem])
    share = _top_code_report(stem, name, acts)
    cand = list(decode({k: v[None] for k, v in acts["__heads__"].items()}, *COVERAGE_HW, 0.02))
    print(f"int8 derived {stem} {name}: {len(cand)} candidates at 0.02, {len(nms(cand, 0.4))} kept")
    relu = [n for n in share if not _is_mid(n) and n != START]
    mids = [n for n in share if _is_mid(n)]
    assert len(relu) == 28 and {"_plus0", "_plus1"} <= set(relu) and len(mids) == 12
    unsaturated = [n for n, v in share.items() if v == 0.0]
    assert not unsaturated, unsaturated


@pytest.mark.parametrize("stem", STEMS)
def test_derived_tables_reach_the_front_end_clamp_and_the_bitonic_nms(nets, coverage_blobs, stem):
    """`pc_quarter`: at least 1000 positions of relu2 and of relu4 (the two blobs at which the engine's float front end may hand over) lie
    at or above 135 quanta of the fp32 oracle -- 127 + 8, twice what a 1 LSB error at the shipped scale can move a value at a quarter of
    that scale -- so the front end's own top clamp is pinned there whatever its rounding.  `pt_eighth`: more than 256 candidates at
    threshold 0.02, the NMS kernel's bitonic path, with the tied scores int8 heads give."""
    q = i8.Int8Net(drv.derive(nets[stem], "pc_quarter"))
    for blob in ("mobilenet0_relu2_fwd", "mobilenet0_relu4_fwd"):
        r = coverage_blobs[stem][blob][0].transpose(1, 2, 0).astype(np.float32)
        over = int(((r * (np.float32(1) / q.scale_of_blob[blob]).reshape(1, 1, -1)).astype(np.float32) >= 135).sum())
        print(f"int8 derived {stem} pc_quarter: {over} of {r.size} positions of {blob} at or above 135 quanta")
        assert over >= 1000, (blob, over)
    q = i8.Int8Net(drv.derive(nets[stem], "pt_eighth"))
    acts = _continue_from_fp32(q, coverage_blobs[stem])
    _top_code_report(stem, "pt_eighth", acts)
    heads = {k: v[None] for k, v in acts["__heads__"].items()}
    cand = list(decode(heads, *COVERAGE_HW, 0.02))
    kept = nms(cand, 0.4)
    scores = np.array([c.score for c in cand], np.float32)
    print(f"int8 derived {stem} pt_eighth: {len(cand)} candidates at 0.02 ({len(np.unique(scores))} distinct scores), {len(kept)} kept")
    assert len(cand) > 256


@pytest.mark.parametrize("stem", STEMS)
def test_remaining_derived_sets_are_what_they_say(nets, coverage_blobs, stem):
    """The other sets on the same frame (their shares of top codes are printed for DESIGN.md section 5).  `pc_coarse` is the low end:
    nothing saturates and no ReLU tensor uses even half of its codes (the shipped table's ~100 quanta of range become ~25).  `pc_ragged`: in each FPN add the three calibrated scales of a
    channel really differ, in most channels, so the max-merge picks different tensors in neighbouring channels.  `pc_quarter` saturates
    more than `pc_half` does; `degenerate` runs on the shipped table."""
    shares = {}
    for name in ("pc_quarter", "pc_coarse", "pc_ragged", "degenerate"):
        net = drv.derive(nets[stem], name)
        acts = _continue_from_fp32(i8.Int8Net(net), coverage_blobs[stem])
        shares[name] = _top_code_report(stem, name, acts)
        heads = {k: v[None] for k, v in acts["__heads__"].items()}
        cand = list(decode(heads, *COVERAGE_HW, 0.02))
        print(f"int8 derived {stem} {name}: {len(cand)} candidates at 0.02, {len(nms(cand, 0.4))} kept")
        if name == "pc_coarse":
            assert max(shares[name].values()) == 0.0
            assert max(int(a.max()) for n, a in acts.items() if n != "__heads__" and not _is_mid(n)) < 64
        if name == "pc_ragged":
            t = net.int8_scales
            for group in (("rf_c3_lateral_relu", "rf_c2_lateral_relu", "_plus0"), ("rf_c2_aggr_relu", "rf_c1_red_conv_relu", "_plus1")):
                s = np.array([[t[f"{g}#{c}"] for c in range(64)] for g in group], np.float32)
                winners = s.argmax(axis=0)
                assert len(set(winners.tolist())) == 3 and np.mean(s.max(axis=0) > s.min(axis=0)) > 0.5, group
    assert np.mean(list(shares["pc_quarter"].values())) > 0.05


def _oracle_gemms(q):
    """fused-op name (as plan.h names it: reference layer names, '+'-joined for merged siblings) -> the oracle's QGemm"""
    ops = {f"mobilenet0_conv{2 * i + 2}_fwd": q.pw[i] for i in range(1, 13)}
    ops.update(zip(("rf_c3_lateral", "rf_c2_lateral", "rf_c1_red_conv"), q.lat))
    ops.update(zip(("rf_c2_aggr", "rf_c1_aggr"), q.aggr))
    for m in q.ssh:
        pre, st = m["pre"], f"stride{m['stride']}"
        ops[pre + "conv1+" + pre + "context_conv1"] = m["a"]
        ops[pre + "context_conv2+" + pre + "context_conv3_1"] = m["b"]
        ops[pre + "context_conv3_2"] = m["c"]
        ops[f"face_rpn_cls_score_{st}+face_rpn_bbox_pred_{st}+face_rpn_landmark_pred_{st}"] = m["head"]
    return ops


def _packer_gemms(lib, model_dir, stem, shapes):
    """every fused dense conv `rf_plan_int8_gemm` enumerates ("?i") for <model_dir>/<stem>.rfw: name -> (unrounded quanta, row scales);
    `shapes` (name -> (cout, ktot), the oracle's) sizes the buffers and is checked against the packer's own dims"""
    F = C.POINTER(C.c_float)
    d, s = str(model_dir).encode(), stem.encode()
    out = {}
    for i in range(64):
        dims = (C.c_int * 4)()
        buf = np.zeros(64, np.float32)
        st = lib.rf_plan_int8_gemm(d, s, None, f"?{i}".encode(), buf.ctypes.data_as(F), buf.size, None, 0, None, None, 0, dims)
        if st != 0:
            break
        op = buf.tobytes()[:dims[0]]
        assert op.decode() in shapes, op
        quanta, row = np.zeros(shapes[op.decode()], np.float32), np.zeros(shapes[op.decode()][0], np.float32)
        st = lib.rf_plan_int8_gemm(d, s, None, op, quanta.ctypes.data_as(F), quanta.size, None, 0, row.ctypes.data_as(F), None, row.size, dims)
        assert st == 0 and (dims[0], dims[1]) == quanta.shape, (op, lib.rf_last_error(None), list(dims))
        out[op.decode()] = (quanta, row)
    return out


@pytest.mark.parametrize("name", drv.ALL)
@pytest.mark.parametrize("stem", STEMS)
def test_host_packer_equals_the_oracle_on_derived_sets(built_lib, nets, tmp_path, stem, name):
    """Every derived set, packed as the GPU test packs it (write_rfw; tables also through rf_attach_calibration from their text form): the
    container reads back with the same scales and no calibrated weights, and for every fused dense conv the C++ packer (weights.h put_gemm)
    has the oracle's weight grid `s_w` BIT for bit and the oracle's integers `wq` -- the zero rows of `degenerate` included, where the row
    scale must be 1 and the integers all 0 (the `amax > 0 ? amax / 127 : 1` branch no shipped model reaches)."""
    from oracle.caffe_io import read_int8_table, read_rfw, write_rfw
    net = drv.derive(nets[stem], name)
    assert net.int8_qweights == {}
    dirs = [tmp_path / "py"]
    dirs[0].mkdir()
    write_rfw(net, str(dirs[0] / (stem + ".rfw")))
    if name in drv.TABLES:
        table = str(tmp_path / "derived.table.int8")
        drv.write_table(net.int8_scales, table)
        assert read_int8_table(table) == net.int8_scales
        dirs.append(tmp_path / "capi")
        dirs[1].mkdir()
        st = built_lib.rf_attach_calibration(ASSETS.encode(), stem.encode(), table.encode(), None, str(dirs[1] / (stem + ".rfw")).encode())
        assert st == 0, built_lib.rf_last_error(None)
        shipped = nets[stem].int8_scales
        if name.startswith("pt_"):
            assert set(net.int8_scales) == {k for k in shipped if "#" not in k}
        else:
            assert list(net.int8_scales) == list(shipped)
        ratios = {net.int8_scales[k] / shipped[k] for k in net.int8_scales}
        assert ratios == (set(drv.RAGGED_FACTORS) if name == "pc_ragged" else {drv._FACTOR[name]}), ratios
    for d in dirs:
        back = read_rfw(str(d / (stem + ".rfw")))
        assert back.int8_qweights == {} and back.int8_scales == net.int8_scales and list(back.int8_scales) == list(net.int8_scales)
    q = i8.Int8Net(net)
    want = _oracle_gemms(q)
    got = _packer_gemms(built_lib, dirs[-1], stem, {op: (g.cout, g.k * g.k * g.cin) for op, g in want.items()})
    assert set(got) == set(want) and len(got) == 29, sorted(set(got) ^ set(want))
    zero_rows = 0
    for op, g in want.items():
        quanta, row = got[op]
        assert np.array_equal(row.view(np.uint32), g.s_w.view(np.uint32)), op
        wq = np.clip(np.rint(quanta), -127, 127).astype(np.int32)               # put_gemm's own rounding of what it records: nearbyintf, then the clamp
        assert np.array_equal(wq, g.wq.reshape(g.cout, -1)), op
        dead = ~wq.any(axis=1)
        assert np.all(row[dead] == 1.0) and not quanta[dead].any(), op       # a live row has a +-127 somewhere: all-zero integers = a zero row
        zero_rows += int(dead.sum())
    if name == "degenerate":
        ed = drv.degenerate_edits(nets[stem])
        for layer, _ in drv.ZERO_ROWS:
            op = next(o for o in want if layer in o.split("+"))
            off = 0
            for part in op.split("+"):                       # merged siblings: the layer's rows sit behind those of the layers named before it
                if part == layer:
                    break
                off += nets[stem].layer(part).blobs[0].shape[0]
            rows = ed[layer + ":zero"] + off
            assert np.all(got[op][1][rows] == 1.0) and not got[op][0][rows].any(), (op, rows)
            assert np.all(want[op].s_w[rows] == 1.0) and not want[op].wq[rows].any(), (op, rows)
        assert zero_rows == sum(n for _, n in drv.ZERO_ROWS)
        # the depthwise counterpart (weights.h put_dw / the oracle's QDw): zero taps -> tap scale 1, integers 0
        dw = q.dw[(int(drv.ZERO_TAPS[0][len("mobilenet0_conv"):].split("_")[0]) - 1) // 2]
        ch = ed[drv.ZERO_TAPS[0] + ":zero"]
        assert np.all(dw.mult[ch] == 1.0) and not dw.wq[ch].any()
    else:
        assert zero_rows == 0


def test_degenerate_weight_set_is_what_it_says(nets):
    """`degenerate` leaves everything before mobilenet0_conv5_fwd alone (the engine's float front end may run through relu4), and its dead
    and saturated channels behave as intended in the oracle: a zero-row pointwise channel is one constant code, a zero-tap depthwise channel
    is one constant code, a beta = 1e4 channel is 127 everywhere."""
    rng = np.random.default_rng(31)
    x = rng.integers(0, 128, (32, 48, 16)).astype(np.int8)
    for stem in STEMS:
        net = drv.derive(nets[stem], "degenerate")
        names = [l.name for l in net.layers]
        cut = names.index("mobilenet0_conv5_fwd")
        for a, b in zip(net.layers[:cut], nets[stem].layers[:cut]):
            assert len(a.blobs) == len(b.blobs) and all(np.array_equal(u, v) for u, v in zip(a.blobs, b.blobs)), a.name
        assert net.int8_scales == nets[stem].int8_scales
        ed = drv.degenerate_edits(nets[stem])
        acts = i8.Int8Net(net).forward_from(START, x)
        for blob, key in (("mobilenet0_relu8_fwd", "mobilenet0_conv8_fwd:zero"), ("mobilenet0_relu9_fwd", "mobilenet0_conv9_fwd:zero"),
                          ("rf_c2_lateral_relu", "rf_c2_lateral:zero"), ("rf_c1_aggr_relu", "rf_c1_aggr:zero")):
            for c in ed[key]:
                assert len(np.unique(acts[blob][:, :, c])) == 1, (stem, blob, c)
        for c in ed["mobilenet0_conv12_fwd:beta"]:
            assert np.all(acts["mobilenet0_relu12_fwd"][:, :, c] == 127), (stem, c)
        live = np.setdiff1d(np.arange(64), ed["mobilenet0_conv8_fwd:zero"])
        assert all(len(np.unique(acts["mobilenet0_relu8_fwd"][:, :, c])) > 1 for c in live[:8])


BAD_SCALES = (0.0, -0.03125, float("nan"), float("inf"))


@pytest.mark.parametrize("bad", BAD_SCALES)
def test_unusable_calibration_scales_are_refused(built_lib, nets, tmp_path, bad):
    """A calibration scale is a quantum size the int8 packer divides by: zero, negative, NaN and inf are refused with RF_ERR_MODEL and a
    message naming the blob -- by rf_attach_calibration for a line of a text table, by rf_create (int8) for a scale entry of an RFW1
    container.  The same container still gives an fp16 engine, which never reads the scales."""
    import copy
    from oracle.caffe_io import write_rfw
    from retinaface_amd import _lib
    stem, blob = "mnet25", "rf_c2_aggr_relu#17"
    scales = dict(nets[stem].int8_scales)
    assert blob in scales
    scales[blob] = bad
    table = str(tmp_path / "bad.table.int8")
    drv.write_table(scales, table)
    st = built_lib.rf_attach_calibration(ASSETS.encode(), stem.encode(), table.encode(), None, str(tmp_path / "out.rfw").encode())
    msg = built_lib.rf_last_error(None).decode()
    assert st == _lib.RF_ERR_MODEL and blob in msg, (st, msg)
    assert not os.path.exists(tmp_path / "out.rfw")
    net = copy.copy(nets[stem])
    net.int8_scales, net.int8_qweights = scales, {}
    write_rfw(net, str(tmp_path / (stem + ".rfw")))

    def create(precision):
        o = _lib.rf_options()
        o.struct_size = C.sizeof(_lib.rf_options)
        o.model_stem, o.precision, o.plan_cache = stem.encode(), precision, 2      # 2: no plan cache
        h = C.c_void_p()
        st = built_lib.rf_create(str(tmp_path).encode(), b"net3", 0.4, C.byref(o), C.byref(h))
        msg = built_lib.rf_last_error(None).decode()
        if h.value:
            built_lib.rf_destroy(h)
        return st, msg
    st, msg = create(2)
    assert st == _lib.RF_ERR_MODEL and blob in msg, (st, msg)
    st, msg = create(1)
    assert st in (0, _lib.RF_ERR_HIP), (st, msg)                  # parsed and packed; fails only for want of a GPU
    # ... and re-packing that container without a new table is refused as well
    st = built_lib.rf_attach_calibration(str(tmp_path).encode(), stem.encode(), None, None, str(tmp_path / "out2.rfw").encode())
    assert st == _lib.RF_ERR_MODEL and blob in built_lib.rf_last_error(None).decode()
