"""Float64 models of the fp32 / fp16 engines' launches, one launch at a time, and the interval judge (numpy only, no GPU).

The float engines keep fp32 accumulators and round to nearest-even exactly where an activation is stored (LDS tile or HBM) and where
a weight is packed.  Rounding is monotone, so ONE launch -- given the device's own stored inputs and the constants the packer really
emitted -- can be bracketed element by element, with no tolerance that depends on the tensor's range or on earlier layers.

A launch is a chain of stages.  A stage is a linear operation (dense 1x1 / 3x3 pad 1, depthwise 3x3 stride 1 / 2, the fixed bilinear
x2 upsample + add, concat), an optional ReLU, and the storage rounding rn_T (fp16 nearest-even for the fp16 engine, the identity for
fp32 and for the head outputs, which are never stored narrow).  For a stage input inside [lo, hi] (lo == hi for the launch's own
inputs, which are exact):

    z_lo = W+ . lo + W- . hi + b          z_hi = W+ . hi + W- . lo + b                       (float64)
    gamma = (K + 2) * 2^-23 * (|W| . max(|lo|, |hi|) + |b|)                                   K = contraction length, bias included
    stored value  in  [ rn_T(act(z_lo - gamma)),  rn_T(act(z_hi + gamma)) ]

gamma is the standard bound of an fp32 sum of K terms in ANY order of accumulation, taken with unit roundoff 2^-23 (twice the
nearest-even value), so it does not depend on how the matrix unit rounds inside an accumulate chain.  Nothing in it is fitted.

Two places where the kernels compute something other than one fp32 sum are modelled as what they are:
  * the fp16 engine's upsample + add (kernels.hip upadd_blend) runs in packed fp16 and rounds after EVERY step:
    a = rn(9/16 t0); a = rn(3/16 t1 + a); a = rn(3/16 t2 + a); a = rn(1/16 t3 + a); plus = rn(a + lat), each an exact product-sum
    rounded once (fma).  All weights are positive, so the chain is monotone and is evaluated on lo and on hi; on the launch's own
    inputs it is bit-exact.
  * the fp16 engine's head weights are an fp16 hi + lo pair along K (weights.h): W = rn(w) + rn(w - rn(w)), K = 2 * 64 + 1.

Constants come from rf_plan_folded (any model directory): folded fp32 weights for the fp32 engine; for the fp16 engine `dw<i>.eq` /
`pw<i>.eq` (the equalised block) rounded to half, every other GEMM rounded to half, biases fp32.

The fp16 engine's first launch (stem2: conv0 .. conv4) computes algebraically rearranged forms, modelled from the packed constants (the
`stem2.*` ops of rf_plan_folded): conv0 on 1024 + pixel with fp16 hi + lo weights and the offset folded into the bias, result kept in
fp32; conv1 stored as an fp16 hi + lo pair (bracketed, see IntervalBackend.stage); conv2 on that pair with hi / lo weights, without
the lo x lo products (bracketed), its tile stored centred by mu2 with the floor -mu2 in place of ReLU's 0 and -mu2 outside the map; conv3
on the centred tile, stored centred by mu3; conv4 with hi | lo weights along K.

Weight set `ragged` (derive_ragged): every Convolution's output rows scaled by a seeded power of two from RAGGED_EXPONENTS.  The full
exponent set {1/4, 1/2, 1, 2, 4} misses the |a| < 2^14 condition under every seed tried (the BN means are not rescaled, so the factors
compound: relu26 reaches 1e6 .. inf); the final choice is the narrowed set {1/2, 1, 2} with SEED 20240517 (max |a| 233, at most 82 %
zeros in any stored tensor, on the GPU test's frames).
"""
from __future__ import annotations

import copy
import ctypes as C
import zlib
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

FP32, FP16 = 0, 1
F32, F64 = np.float32, np.float64
U = 2.0 ** -23                      # the unit roundoff gamma is taken with (twice fp32 nearest-even)
SCORE_EPS = 1e-5                    # = TOL[FP32]["score"] of test_gpu_parity.py: the bar that blob already carries for the exp and the divide
STRIDES = (32, 16, 8)
DW_STRIDES = (1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1)
LATERAL_OF_BLOCK = {4: 2, 10: 1, 12: 0}
LATERAL_BLOBS = ("rf_c3_lateral_relu", "rf_c2_lateral_relu", "rf_c1_red_conv_relu")
AGGR_BLOBS = ("rf_c2_aggr_relu", "rf_c1_aggr_relu")

SEED = 20240517
RAGGED_EXPONENTS = (0.5, 1.0, 2.0)


def relu_blob(n: int) -> str:
    return f"mobilenet0_relu{n}_fwd"


def rn16(x: np.ndarray) -> np.ndarray:
    """fp16 nearest-even of float64 values (numpy converts double -> half with one rounding)"""
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(np.float16).astype(F64)


def rz16(x: np.ndarray) -> np.ndarray:
    """fp16 toward zero (the `stores rounded toward zero` mutant)"""
    r = rn16(x)
    over = np.abs(r) > np.abs(x)
    return np.where(over, np.nextafter(r.astype(np.float16), np.float16(0)).astype(F64), r)


def ident(x):
    return x


def store_rounding(prec: int):
    return rn16 if prec == FP16 else ident


# ------------------------------------------------------------------------------------------------ constants
_folded_cache: Dict[Tuple[str, str, str], Tuple[np.ndarray, np.ndarray]] = {}


def folded(lib, model_dir: str, stem: str, op: str) -> Tuple[np.ndarray, np.ndarray]:
    """rf_plan_folded: ([cout][k][k][cin / group] fp32, [cout] fp32).  Every call parses the model and compiles the plan, so results are
    kept per (directory, stem, op); callers get copies."""
    key = (model_dir, stem, op)
    if key not in _folded_cache:
        _folded_cache[key] = _folded(lib, model_dir, stem, op)
    w, b = _folded_cache[key]
    return w.copy(), b.copy()


def _folded(lib, model_dir: str, stem: str, op: str) -> Tuple[np.ndarray, np.ndarray]:
    dims = (C.c_int * 4)()
    st = lib.rf_plan_folded(model_dir.encode(), stem.encode(), op.encode(), None, 0, None, 0, dims)
    assert st == 0, (op, lib.rf_last_error(None))
    n = dims[0] * dims[1] * dims[2] * dims[3]
    w, b = np.empty(n, F32), np.empty(dims[0], F32)
    st = lib.rf_plan_folded(model_dir.encode(), stem.encode(), op.encode(), w.ctypes.data_as(C.POINTER(C.c_float)), n,
                            b.ctypes.data_as(C.POINTER(C.c_float)), dims[0], dims)
    assert st == 0, (op, lib.rf_last_error(None))
    return w.reshape(dims[0], dims[1], dims[2], dims[3]), b


def half_of(w: np.ndarray) -> np.ndarray:
    """a float32 constant as the packer stores it in half: one nearest-even rounding"""
    return np.asarray(w, F32).astype(np.float16)


def head_hi_lo(w: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """weights.h: hi = rn16(w), lo = rn16(w - hi) (the difference is exact in fp32)"""
    w = np.asarray(w, F32)
    hi = w.astype(np.float16)
    lo = (w - hi.astype(F32)).astype(np.float16)
    return hi, lo


@dataclass
class Op:
    w: np.ndarray          # float64, [cout][k][k][cin / group], as the kernel sees it
    b: np.ndarray          # float64 [cout]
    kind: str              # "dense" | "dw"
    stride: int
    K: int                 # contraction length, the bias counted as a term
    pad: Optional[np.ndarray] = None       # what the input tile holds outside the map, per input channel (default 0)
    floor: Optional[np.ndarray] = None     # per-channel floor that stands in for ReLU's 0 (DC-centred tiles)
    w_lo: Optional[np.ndarray] = None      # the input is an fp16 hi + lo pair, multiplied as w x_hi + w x_lo + w_lo x_hi
    store: str = "T"                       # "T" = rn_T | "f32" = kept in fp32 | "pair" = fp16 hi + lo pair


class Consts:
    """Every constant of one engine (model directory, stem, precision) as its kernels see it."""

    def __init__(self, lib, model_dir: str, stem: str, prec: int):
        self.prec, self.stem = prec, stem
        self.ops: Dict[str, Op] = {}
        f = lambda op: folded(lib, model_dir, stem, op)
        h = (lambda w: half_of(w).astype(F64)) if prec == FP16 else (lambda w: w.astype(F64))

        def put(tag, w, b, kind="dense", stride=1, kmul=1, **kw):
            k = (w.shape[1] * w.shape[2] * w.shape[3]) * kmul + 1
            self.ops[tag] = Op(np.asarray(w, F64), b.astype(F64), kind, stride, k, **kw)

        if prec == FP32:
            w, b = f("conv0")
            put("conv0", w, b, stride=2)
        else:
            # stem2 (weights.h pack(), kernels.hip stem2_kernel).  conv0: fp16 hi + lo weights against 1024 + pixel (exact in fp16), the
            # bias with -1024 * sum(hi + lo) folded in, result kept in fp32; conv1: fp32 taps, result an fp16 hi + lo pair; conv2: hi / lo
            # weights, bias - mu2, tile centred with floor -mu2 (and -mu2 outside the map); conv3: equalised fp16 taps, bias + mu2 *
            # sum(taps) - mu3, floor -mu3; conv4: equalised weights as hi | lo along K, bias + W mu3.
            pair = lambda w: [v.astype(F64) for v in head_hi_lo(w)]
            w, b = f("stem2.c0")
            hi, lo = pair(w)
            put("s2.c0", np.concatenate([hi, lo], -1), b, stride=2, pad=np.full(6, 1024.0), store="f32")
            w, b = f("dw0")
            put("s2.c1", w.astype(F64), b, "dw", 1, store="pair")
            floor2, floor3 = f("stem2.floor2")[1].astype(F64), f("stem2.floor3")[1].astype(F64)
            w, b = f("stem2.c2")
            hi, lo = pair(w)
            put("s2.c2", hi, b, kmul=3, floor=floor2, w_lo=lo)
            w, b = f("stem2.c3")
            put("s2.c3", w.astype(F64), b, "dw", 2, pad=floor2, floor=floor3)
            w, b = f("stem2.c4")
            hi, lo = pair(w)
            put("s2.c4", hi + lo, b, kmul=2)
        for i in range(0 if prec == FP32 else 2, 13):
            sfx = ".eq" if prec == FP16 else ""
            w, b = f(f"dw{i}{sfx}")
            put(f"dw{i}", h(w), b, "dw", DW_STRIDES[i])
            w, b = f(f"pw{i}{sfx}")
            put(f"pw{i}", h(w), b)
        for i in range(3):
            w, b = f(f"lateral{i}")
            put(f"lateral{i}", h(w), b)
        for i in range(2):
            w, b = f(f"aggr{i}")
            put(f"aggr{i}", h(w), b)
        for i in range(3):
            for t in "abc":
                w, b = f(f"ssh{i}.{t}")
                put(f"ssh{i}.{t}", h(w), b)
            w, b = f(f"ssh{i}.head")
            if prec == FP16:
                hi, lo = head_hi_lo(w)
                put(f"ssh{i}.head", hi.astype(F64) + lo.astype(F64), b, kmul=2)
            else:
                put(f"ssh{i}.head", w, b)
        self.anchors = self.ops["ssh0.head"].w.shape[0] // 16


# ------------------------------------------------------------------------------------------------ linear operations (float64)
def _patches(x: np.ndarray, k: int, stride: int, pad: Optional[np.ndarray] = None):
    """the k*k shifted views of x (N, H, W, C) a pad-(k//2) convolution reads, in (ky, kx) order, each (N, H/stride, W/stride, C); outside
    the map the input is `pad` (per channel), 0 by default"""
    p = k // 2
    n, hh, ww, c = x.shape
    ho, wo = hh // stride, ww // stride
    if p and pad is not None:
        xp = np.empty((n, hh + 2 * p, ww + 2 * p, c), x.dtype)
        xp[...] = np.asarray(pad, x.dtype)
        xp[:, p:-p, p:-p, :] = x
    else:
        xp = np.pad(x, ((0, 0), (p, p), (p, p), (0, 0))) if p else x
    return [xp[:, ky:ky + stride * ho:stride, kx:kx + stride * wo:stride, :] for ky in range(k) for kx in range(k)]


def lin(x: np.ndarray, op: Op, w: Optional[np.ndarray] = None, pad: Optional[np.ndarray] = None) -> np.ndarray:
    """the stage's linear operation without its bias, with weights `w` (default: the op's own) and outside-map value `pad` (default: the op's)"""
    w = op.w if w is None else w
    k = w.shape[1]
    ps = _patches(x, k, op.stride, op.pad if pad is None else pad)
    out = None
    for t, p in enumerate(ps):
        wt = w[:, t // k, t % k, :]
        y = p * wt[:, 0] if op.kind == "dw" else p @ wt.T
        out = y if out is None else out + y
    return out


def up_taps(x: np.ndarray, swap_axis: Optional[int] = None) -> List[np.ndarray]:
    """The four coarse-map taps of the bilinear x2 upsample at every fine pixel, in the kernel's order (weights 9/16, 3/16, 3/16, 1/16):
    (my, mx), (my, mx2), (my2, mx), (my2, mx2) with m = i >> 1, m2 = m + 1 for odd i, m - 1 for even i; taps outside the map are 0.
    swap_axis (0 = y, 1 = x): the mutant that swaps the near (0.75) and far (0.25) tap on that axis."""
    n, hh, ww, c = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))

    def idx(size):
        i = np.arange(2 * size)
        m = i >> 1
        m2 = np.where(i & 1, m + 1, m - 1)
        return m + 1, m2 + 1               # +1: the zero ring

    (ya, yb), (xa, xb) = idx(hh), idx(ww)
    if swap_axis == 0:
        ya, yb = yb, ya
    if swap_axis == 1:
        xa, xb = xb, xa
    g = lambda yi, xi: xp[:, yi][:, :, xi]
    return [g(ya, xa), g(ya, xb), g(yb, xa), g(yb, xb)]


UP_W = (0.5625, 0.1875, 0.1875, 0.0625)


# ------------------------------------------------------------------------------------------------ interval backend
@dataclass
class IV:
    lo: np.ndarray
    hi: np.ndarray
    zmid: Optional[np.ndarray] = None      # of the last stage: the exact value at the interval's middle, before act and rounding
    gtot: Optional[np.ndarray] = None      # gamma + half the propagated width, before act and rounding
    narrow: bool = False                   # the last stage stored through rn16


class IntervalBackend:
    def __init__(self, prec: int):
        self.prec = prec
        self.rn = store_rounding(prec)

    def input(self, a: np.ndarray) -> IV:
        a = np.asarray(a, F64)
        return IV(a, a)

    def stage(self, x: IV, op: Op, tag: str, relu: bool = True, store: bool = True) -> IV:
        w = op.w if op.w_lo is None else op.w + op.w_lo
        wp, wn = np.maximum(w, 0.0), np.minimum(w, 0.0)
        wa = np.abs(op.w) if op.w_lo is None else np.abs(op.w) + np.abs(op.w_lo)
        apad = None if op.pad is None else np.abs(op.pad)
        xa = np.maximum(np.abs(x.lo), np.abs(x.hi))
        if x.lo is x.hi:
            z_lo = z_hi = lin(x.lo, op, w) + op.b
        else:
            z_lo = lin(x.lo, op, wp) + lin(x.hi, op, wn) + op.b
            z_hi = lin(x.hi, op, wp) + lin(x.lo, op, wn) + op.b
        mag = lin(xa, op, wa, apad) + np.abs(op.b)
        g = (op.K + 2) * U * mag
        if op.w_lo is not None:
            # Input pair x_hi + x_lo = s (the interval is on s): the kernel multiplies w x_hi + w x_lo + w_lo x_hi and leaves w_lo x_lo out.
            # |x_lo| <= half an fp16 ulp at x_hi <= 2^-11 (s + |x_lo|) <= 2^-11 (1 + 2^-10) s (+ 2^-25 in the subnormal range);
            # |x_hi| + |x_lo| <= (1 + 2^-10) s.
            g = g * (1.0 + 2.0 ** -10) + lin(2.0 ** -11 * (1.0 + 2.0 ** -10) * xa + 2.0 ** -25, op, np.abs(op.w_lo))
        if op.floor is not None:
            act = lambda v: np.maximum(v, op.floor)
        else:
            act = (lambda v: np.maximum(v, 0.0)) if relu else ident
        lo, hi = act(z_lo - g), act(z_hi + g)
        zmid, gtot = 0.5 * (z_lo + z_hi), g + 0.5 * (z_hi - z_lo)
        if not store or op.store == "f32":
            return IV(lo, hi, zmid, gtot)
        if op.store == "pair":
            # hi = rn16(v), lo = rn16(v - hi) (the difference is exact in fp32): the pair's sum is v up to the rounding of lo,
            # <= 2^-11 |v - hi| <= 2^-22 |v|, or 2^-25 where lo is subnormal; v = 0 is stored exactly.  v >= 0 (after ReLU), so v - eps(v) is increasing.
            eps = lambda v: np.where(v == 0, 0.0, np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25))
            return IV(lo - eps(lo), hi + eps(hi), zmid, gtot)
        return IV(self.rn(lo), self.rn(hi), zmid, gtot, self.prec == FP16)

    def plus(self, lat: IV, coarse: IV, tag: str) -> IV:
        if self.prec == FP16:
            def chain(l, c):
                t = up_taps(c)
                a = rn16(t[0] * UP_W[0])
                for q in (1, 2, 3):
                    a = rn16(t[q] * UP_W[q] + a)
                return rn16(a + l)
            lo = chain(lat.lo, coarse.lo)
            hi = lo if (lat.lo is lat.hi and coarse.lo is coarse.hi) else chain(lat.hi, coarse.hi)
            return IV(lo, hi, 0.5 * (lo + hi), 0.5 * (hi - lo), True)
        up = lambda c: sum(wq * t for wq, t in zip(UP_W, up_taps(c)))
        z_lo, z_hi = lat.lo + up(coarse.lo), lat.hi + up(coarse.hi)
        mag = np.maximum(np.abs(lat.lo), np.abs(lat.hi)) + up(np.maximum(np.abs(coarse.lo), np.abs(coarse.hi)))
        g = (5 + 2) * U * mag                  # five terms (four taps and the lateral), no bias
        return IV(z_lo - g, z_hi + g, 0.5 * (z_lo + z_hi), g + 0.5 * (z_hi - z_lo))

    def ch(self, x: IV, a: int, b: int) -> IV:
        s = lambda v: None if v is None else v[..., a:b]
        return IV(s(x.lo), s(x.hi), s(x.zmid), s(x.gtot), x.narrow)

    def cat(self, xs: Sequence[IV]) -> IV:
        c = lambda f: np.concatenate([f(x) for x in xs], axis=-1)
        return IV(c(lambda x: x.lo), c(lambda x: x.hi), c(lambda x: x.zmid), c(lambda x: x.gtot), xs[0].narrow)


# ------------------------------------------------------------------------------------------------ emulation backend
MUTANT_KINDS = ("rtz", "drop_tap", "drop_lo", "raw_dw_channel", "swap_channels", "swap_up_taps", "relu_before_floor", "last_image")


@dataclass
class Mutant:
    kind: str = ""             # "" = the faithful emulation, or one of MUTANT_KINDS
    tag: str = ""              # the stage it applies to (last_image: the launch; "" = every launch)
    arg: Tuple = ()

    def __post_init__(self):
        assert self.kind == "" or self.kind in MUTANT_KINDS, self.kind


def _tree_sum(a: np.ndarray) -> np.ndarray:
    """pairwise (tree) float32 sum over axis 1"""
    while a.shape[1] > 1:
        if a.shape[1] & 1:
            a = np.concatenate([a, np.zeros_like(a[:, :1])], axis=1)
        a = a[:, 0::2] + a[:, 1::2]
    return a[:, 0]


class EmuBackend:
    """The launches in float32 arithmetic with a chosen summation order (natural | reversed | blocked), storage roundings at the
    model's points, optionally with one mutant."""

    def __init__(self, prec: int, order: str, mutant: Optional[Mutant] = None, raw=None):
        self.prec, self.order, self.m = prec, order, mutant or Mutant()
        self.block = 4 if prec == FP32 else 32          # the MFMA K step of the precision
        self.raw = raw                                  # unequalised constants (raw_dw_channel)

    def input(self, a):
        return np.asarray(a, F32)

    def _store(self, v, tag, store):
        if not store or self.prec != FP16:
            return v
        if self.m.kind == "rtz" and self.m.tag == tag:
            return rz16(v.astype(F64)).astype(F32)
        return rn16(v.astype(F64)).astype(F32)

    def stage(self, x, op: Op, tag: str, relu: bool = True, store: bool = True):
        w, b = op.w.astype(F32), op.b.astype(F32)
        hit = self.m.tag == tag
        if op.w_lo is not None:                       # x = (hi, lo): w x_hi + w x_lo + w_lo x_hi, as three K groups
            x = np.concatenate([x[0], x[1], x[0]], -1)
            w = np.concatenate([w, w, op.w_lo.astype(F32)], -1)
        if hit and self.m.kind == "drop_lo":
            w = w.copy()
            w[..., w.shape[-1] // 2:] = 0
        if hit and self.m.kind == "raw_dw_channel":
            c = self.m.arg[0]
            w, b = w.copy(), b.copy()
            w[c], b[c] = self.raw.ops[tag].w[c].astype(F32), self.raw.ops[tag].b[c].astype(F32)
        k = w.shape[1]
        ps = _patches(x, k, op.stride, op.pad)
        n, ho, wo, _ = ps[0].shape
        cout = w.shape[0]
        if op.kind == "dw":
            X = np.stack([p.reshape(-1, cout) for p in ps], axis=1)                      # (P, 9, C)
            Wt = np.stack([w[:, t // k, t % k, 0] for t in range(k * k)], axis=0)        # (9, C)
            term = lambda j: X[:, j, :] * Wt[j]
            terms = lambda j0, j1: X[:, j0:j1, :] * Wt[None, j0:j1, :]
        else:
            X = np.concatenate([p.reshape(n * ho * wo, -1) for p in ps], axis=1)         # (P, K), k = tap * cin + c
            Wt = np.concatenate([w[:, t // k, t % k, :].T for t in range(k * k)], axis=0)  # (K, cout)
            if hit and self.m.kind == "drop_tap":
                img, y, xx, tap = self.m.arg
                cin = w.shape[3]
                X = X.copy()
                X[(img * ho + y) * wo + xx, tap * cin:(tap + 1) * cin] = 0
            term = lambda j: X[:, j, None] * Wt[j]
            terms = lambda j0, j1: X[:, j0:j1, None] * Wt[None, j0:j1, :]
        kk = Wt.shape[0]
        if self.order == "natural":
            acc = np.broadcast_to(b, (X.shape[0], cout)).astype(F32)
            for j in range(kk):
                acc = acc + term(j)
        elif self.order == "reversed":
            acc = np.zeros((X.shape[0], cout), F32)
            for j in reversed(range(kk)):
                acc = acc + term(j)
            acc = acc + b
        else:
            acc = np.broadcast_to(b, (X.shape[0], cout)).astype(F32)
            for j0 in range(0, kk, self.block):
                acc = acc + _tree_sum(terms(j0, min(kk, j0 + self.block)))
        assert acc.dtype == F32
        v = acc.reshape(n, ho, wo, cout)
        if op.floor is not None:
            if hit and self.m.kind == "relu_before_floor":
                v = np.maximum(v, F32(0))
            v = np.maximum(v, op.floor.astype(F32))
        elif relu:
            v = np.maximum(v, F32(0))
        if op.store == "pair":
            hi = rn16(v.astype(F64)).astype(F32)
            return hi, rn16((v - hi).astype(F64)).astype(F32)
        if op.store == "f32":
            return v
        if hit and self.m.kind == "swap_channels":
            c = self.m.arg[0]
            v = v.copy()
            v[..., [c, c + 1]] = v[..., [c + 1, c]]
        return self._store(v, tag, store)

    def plus(self, lat, coarse, tag):
        t = up_taps(coarse, self.m.arg[0] if (self.m.kind == "swap_up_taps" and self.m.tag == tag) else None)
        if self.prec == FP16:
            a = rn16(t[0].astype(F64) * UP_W[0])
            for q in (1, 2, 3):
                a = rn16(t[q].astype(F64) * UP_W[q] + a)
            return rn16(a + lat).astype(F32)
        a = F32(UP_W[0]) * t[0]
        for q in (1, 2, 3):
            a = a + F32(UP_W[q]) * t[q]
        return lat + a

    def ch(self, x, a, b):
        return x[..., a:b]

    def cat(self, xs):
        return np.concatenate(xs, axis=-1)


# ------------------------------------------------------------------------------------------------ the launches
@dataclass
class Launch:
    name: str
    ins: List[str]                               # blobs (or "frame") read from the device
    outs: List[Tuple[str, Optional[Tuple[int, int]]]]     # (blob, channel slice of it or None)
    run: Callable                                 # (backend, Consts, inputs) -> outputs, in `outs` order
    head_stride: int = 0                          # heads: outs are the three head blobs of this stride


def head_names(stride: int) -> Tuple[str, str, str]:
    s = f"stride{stride}"
    return f"face_rpn_cls_prob_reshape_{s}", f"face_rpn_bbox_pred_{s}", f"face_rpn_landmark_pred_{s}"


def launches(prec: int) -> List[Launch]:
    """The launches of net.cpp build_net for this precision, in launch order, at the storage points the precision really has.  Levels of
    the SSH / head launches are listed one by one (one grid on the device, independent maps)."""
    L: List[Launch] = []

    def block_fn(i):
        def run(be, k, x):
            y = be.stage(be.input(x[0]), k.ops[f"dw{i}"], f"dw{i}")
            y = be.stage(y, k.ops[f"pw{i}"], f"pw{i}")
            if i in LATERAL_OF_BLOCK:
                li = LATERAL_OF_BLOCK[i]
                return [y, be.stage(y, k.ops[f"lateral{li}"], f"lateral{li}")]
            return [y]
        return run

    first = 0
    if prec == FP32:
        L.append(Launch("conv0", ["frame"], [(relu_blob(0), None)],
                        lambda be, k, x: [be.stage(be.input(x[0]), k.ops["conv0"], "conv0")]))
    else:
        def stem2(be, k, x):
            y = be.input(np.concatenate([x[0] + 1024.0, x[0] + 1024.0], -1))
            for t in ("c0", "c1", "c2", "c3", "c4"):
                y = be.stage(y, k.ops["s2." + t], "s2." + t)
            return [y]
        L.append(Launch("stem2", ["frame"], [(relu_blob(4), None)], stem2))

        def dwpw2(be, k, x):
            y = be.input(x[0])
            for i in (2, 3):
                y = be.stage(be.stage(y, k.ops[f"dw{i}"], f"dw{i}"), k.ops[f"pw{i}"], f"pw{i}")
            return [y]
        L.append(Launch("dwpw2(2,3)", [relu_blob(4)], [(relu_blob(8), None)], dwpw2))
        first = 4
    for i in range(first, 13):
        outs = [(relu_blob(2 * i + 2), None)]
        if i in LATERAL_OF_BLOCK:
            outs.append((LATERAL_BLOBS[LATERAL_OF_BLOCK[i]], None))
        L.append(Launch(f"dwpw{i}", [relu_blob(2 * i)], outs, block_fn(i)))
    feat = [LATERAL_BLOBS[0], AGGR_BLOBS[0], AGGR_BLOBS[1]]
    for i in range(2):
        def aggr(be, k, x, i=i):
            p = be.plus(be.input(x[0]), be.input(x[1]), f"plus{i}")
            return [be.stage(p, k.ops[f"aggr{i}"], f"aggr{i}")]
        L.append(Launch(f"aggr{i}", [LATERAL_BLOBS[i + 1], feat[i]], [(AGGR_BLOBS[i], None)], aggr))
    for i in range(3):
        pre = f"rf_c{3 - i}_det_"
        cat, c1, c31 = pre + "concat_relu", pre + "context_conv1_relu", pre + "context_conv3_1_relu"

        def ssh_a(be, k, x, i=i):
            y = be.stage(be.input(x[0]), k.ops[f"ssh{i}.a"], f"ssh{i}.a")
            return [be.ch(y, 0, 32), be.ch(y, 32, 48)]
        L.append(Launch(f"ssh{i}.a", [feat[i]], [(cat, (0, 32)), (c1, None)], ssh_a))
        if prec == FP16:
            def tail(be, k, x, i=i):
                yb = be.stage(be.input(x[0]), k.ops[f"ssh{i}.b"], f"ssh{i}.b")
                yc = be.stage(be.ch(yb, 16, 32), k.ops[f"ssh{i}.c"], f"ssh{i}.c")
                return [be.cat([be.ch(yb, 0, 16), yc])]
            L.append(Launch(f"ssh{i}.tail", [c1], [(cat, (32, 64))], tail))
        else:
            def ssh_b(be, k, x, i=i):
                y = be.stage(be.input(x[0]), k.ops[f"ssh{i}.b"], f"ssh{i}.b")
                return [be.ch(y, 0, 16), be.ch(y, 16, 32)]
            L.append(Launch(f"ssh{i}.b", [c1], [(cat, (32, 48)), (c31, None)], ssh_b))
            L.append(Launch(f"ssh{i}.c", [c31], [(cat, (48, 64))],
                            lambda be, k, x, i=i: [be.stage(be.input(x[0]), k.ops[f"ssh{i}.c"], f"ssh{i}.c")]))

        def head(be, k, x, i=i):
            return [be.stage(be.input(x[0]), k.ops[f"ssh{i}.head"], f"ssh{i}.head", relu=False, store=False)]
        L.append(Launch(f"head{i}", [cat], [(n, None) for n in head_names(STRIDES[i])], head, head_stride=STRIDES[i]))
    return L


def frame_input(frames: Sequence[np.ndarray]) -> np.ndarray:
    """conv0's input: the BGR u8 frames as the net's RGB channels, raw 0..255 (N, H, W, 3)"""
    return np.stack([np.asarray(f)[:, :, ::-1] for f in frames]).astype(F64)


# ------------------------------------------------------------------------------------------------ heads
def sigmoid(d):
    d = np.asarray(d, F64)
    with np.errstate(over="ignore"):
        return np.where(d >= 0, 1.0 / (1.0 + np.exp(-np.abs(d))), np.exp(-np.abs(d)) / (1.0 + np.exp(-np.abs(d))))


def head_intervals(iv: IV, anchors: int) -> List[IV]:
    """(N, H, W, 16A) head outputs -> the three blobs as (N, C, H, W): cls_prob = softmax over (background a, foreground a) = a monotone
    function of d = z_fg - z_bg, interval [sigma(d_lo) - eps, sigma(d_hi) + eps]; bbox / landmark are linear."""
    a = anchors
    t = lambda v: np.transpose(v, (0, 3, 1, 2))
    bg_lo, bg_hi, fg_lo, fg_hi = iv.lo[..., 0:a], iv.hi[..., 0:a], iv.lo[..., a:2 * a], iv.hi[..., a:2 * a]
    d_lo, d_hi = fg_lo - bg_hi, fg_hi - bg_lo
    p_lo = np.concatenate([sigmoid(-d_hi), sigmoid(d_lo)], -1) - SCORE_EPS
    p_hi = np.concatenate([sigmoid(-d_lo), sigmoid(d_hi)], -1) + SCORE_EPS
    d_mid = iv.zmid[..., a:2 * a] - iv.zmid[..., 0:a]
    prob = IV(t(p_lo), t(p_hi), t(np.concatenate([sigmoid(-d_mid), sigmoid(d_mid)], -1)),
              t(np.concatenate([0.5 * (p_hi[..., :a] - p_lo[..., :a]), 0.5 * (p_hi[..., a:] - p_lo[..., a:])], -1)))
    s = lambda lo, hi: IV(t(iv.lo[..., lo:hi]), t(iv.hi[..., lo:hi]), t(iv.zmid[..., lo:hi]), t(iv.gtot[..., lo:hi]))
    return [prob, s(2 * a, 6 * a), s(6 * a, 16 * a)]


def head_values(v: np.ndarray, anchors: int) -> List[np.ndarray]:
    """the emulation's head outputs -> the three blobs, softmax in float32 as the kernel writes it"""
    a = anchors
    v = np.asarray(v, F32)
    s0, s1 = v[..., 0:a], v[..., a:2 * a]
    m = np.maximum(s0, s1)
    e0, e1 = np.exp(s0 - m), np.exp(s1 - m)
    prob = np.concatenate([e0 / (e0 + e1), e1 / (e0 + e1)], -1).astype(F32)
    t = lambda x: np.transpose(x, (0, 3, 1, 2))
    return [t(prob), t(v[..., 2 * a:6 * a]), t(v[..., 6 * a:16 * a])]


# ------------------------------------------------------------------------------------------------ the judge
@dataclass
class Verdict:
    launch: str
    blob: str
    ok: bool
    n: int
    n_fail: int = 0
    first: Optional[Tuple] = None          # (image, y, x, c), value, lo, hi
    where: Dict[str, int] = field(default_factory=dict)
    share_exact: float = 0.0
    median_width_ulps: float = 0.0
    max_dev_over_gamma: float = 0.0

    def message(self) -> str:
        if self.ok:
            return f"{self.launch} {self.blob}: inside"
        (img, y, x, c), v, lo, hi = self.first
        return (f"{self.launch} -> {self.blob}: {self.n_fail} of {self.n} elements outside their interval; first (image {img}, y {y}, x {x}, "
                f"c {c}) value {v!r} not in [{lo!r}, {hi!r}]; failing elements lie: {self.where}")


def judge(launch: str, blob: str, value: np.ndarray, iv: IV, layout: str = "NHWC", tile: Tuple[int, int] = (8, 8)) -> Verdict:
    """Every element must satisfy lo <= value <= hi: none excluded, nothing relative to the tensor's range.  `value`, `iv` share a
    layout: NHWC (activations) or NCHW (head blobs)."""
    v = np.asarray(value, F64)
    assert v.shape == iv.lo.shape, (launch, blob, v.shape, iv.lo.shape)
    bad = ~((iv.lo <= v) & (v <= iv.hi))              # NaN fails
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # (the ulp of the stored type at the interval's larger end: a probability of ~0 inside [0, eps] is measured in ulps of eps)
        ulp = np.spacing(np.maximum(np.abs(iv.lo), np.abs(iv.hi)).astype(np.float16 if iv.narrow else F32)).astype(F64)
        width = (iv.hi - iv.lo) / ulp
        denom = iv.gtot + (0.5 * np.spacing(np.abs(iv.zmid).astype(np.float16)).astype(F64) if iv.narrow else 0.0)
        dev = np.where(denom > 0, np.abs(v - iv.zmid) / np.where(denom > 0, denom, 1.0), 0.0)
    # (a ReLU'd element's z_mid may be negative while the stored value is 0: those are left out of the deviation statistic)
    dev = np.where((v == 0) & (iv.zmid < 0), 0.0, dev)
    r = Verdict(launch, blob, not bad.any(), v.size, share_exact=float((iv.lo == iv.hi).mean()),
                median_width_ulps=float(np.median(width[np.isfinite(width)])) if np.isfinite(width).any() else 0.0,
                max_dev_over_gamma=float(dev.max()) if dev.size else 0.0)
    if not r.ok:
        idx = np.argwhere(bad)
        yx = (1, 2) if layout == "NHWC" else (2, 3)
        cax = 3 if layout == "NHWC" else 1
        hh, ww = v.shape[yx[0]], v.shape[yx[1]]
        i0 = tuple(int(i) for i in idx[0])
        r.n_fail = int(bad.sum())
        r.first = ((i0[0], i0[yx[0]], i0[yx[1]], i0[cax]), float(v[i0]), float(iv.lo[i0]), float(iv.hi[i0]))
        y, x = idx[:, yx[0]], idx[:, yx[1]]
        border = (y == 0) | (y == hh - 1) | (x == 0) | (x == ww - 1)
        partial = (y >= hh - hh % tile[0]) & (hh % tile[0] != 0) | (x >= ww - ww % tile[1]) & (ww % tile[1] != 0)
        r.where = {"interior": int((~border).sum()), "border row or column": int(border.sum()), "last partial tile": int(partial.sum()),
                   "images": sorted(set(int(i) for i in idx[:, 0]))}
    return r


def run_launch(be, k: Consts, launch: Launch, inputs: Sequence[np.ndarray]):
    outs = launch.run(be, k, list(inputs))
    if launch.head_stride:
        return head_intervals(outs[0], k.anchors) if isinstance(be, IntervalBackend) else head_values(outs[0], k.anchors)
    return outs


def judge_launch(k: Consts, launch: Launch, blobs: Dict[str, np.ndarray]) -> List[Verdict]:
    """One launch against stored tensors: `blobs` maps every blob the launch reads or writes ("frame" included, as frame_input gives it)
    to the device's (or an emulation's) stored tensor, activations (N, H, W, C), head blobs (N, C, H, W)."""
    ivs = run_launch(IntervalBackend(k.prec), k, launch, [blobs[n] for n in launch.ins])
    res = []
    for (blob, sl), iv in zip(launch.outs, ivs):
        v = blobs[blob]
        if sl is not None:
            v = v[..., sl[0]:sl[1]]
        res.append(judge(launch.name, blob if sl is None else f"{blob}[{sl[0]}:{sl[1]}]", v, iv, "NCHW" if launch.head_stride else "NHWC"))
    return res


def emulate(k: Consts, frames: Sequence[np.ndarray], order: str, mutant: Optional[Mutant] = None, raw=None) -> Dict[str, np.ndarray]:
    """The whole engine as a chain of emulated launches, each reading the emulation's own stored tensors: blob -> tensor."""
    be = EmuBackend(k.prec, order, mutant, raw)
    blobs: Dict[str, np.ndarray] = {"frame": frame_input(frames)}
    for L in launches(k.prec):
        outs = run_launch(be, k, L, [blobs[n] for n in L.ins])
        for (blob, sl), v in zip(L.outs, outs):
            v = np.asarray(v, F64)
            if mutant is not None and mutant.kind == "last_image" and mutant.tag in ("", L.name):
                v = v.copy()
                v[-1] = v[0]
            if sl is None:
                blobs[blob] = v
            else:
                if blob not in blobs:
                    blobs[blob] = np.zeros(v.shape[:-1] + (64,), F64)
                blobs[blob][..., sl[0]:sl[1]] = v
    return blobs


def model_forward(k: Consts, frames: Sequence[np.ndarray]) -> Dict[str, np.ndarray]:
    """The float64 model run as a chain, every launch reading the stored middles of the intervals before it: what a weight set's
    conditions are checked on, on the CPU.  blob -> tensor."""
    be = IntervalBackend(k.prec)
    blobs: Dict[str, np.ndarray] = {"frame": frame_input(frames)}
    for L in launches(k.prec):
        outs = run_launch(be, k, L, [blobs[n] for n in L.ins])
        for (blob, sl), iv in zip(L.outs, outs):
            v = 0.5 * (iv.lo + iv.hi)
            if iv.narrow:
                v = rn16(v)
            if sl is None:
                blobs[blob] = v
            else:
                if blob not in blobs:
                    blobs[blob] = np.zeros(v.shape[:-1] + (64,), F64)
                blobs[blob][..., sl[0]:sl[1]] = v
    return blobs


# ------------------------------------------------------------------------------------------------ weight sets
def derive_ragged(net, exponents: Sequence[float] = RAGGED_EXPONENTS, seed: int = SEED):
    """A copy of `net` (a NetSpec) whose every Convolution has its output rows scaled by a seeded power of two.  Not function-preserving:
    it moves the grid the fp16 tap equalisation searches on and the channel magnitudes inside one MFMA tile apart."""
    out = copy.deepcopy(net)
    out.int8_qweights = {}
    for l in out.layers:
        if l.type != "Convolution":
            continue
        rng = np.random.default_rng([seed, zlib.crc32(l.name.encode())])
        f = np.asarray(exponents, F32)[rng.integers(0, len(exponents), l.blobs[0].shape[0])]
        l.blobs[0] *= f.reshape(-1, *([1] * (l.blobs[0].ndim - 1)))
    return out


# ------------------------------------------------------------------------------------------------ what the GPU test runs (shared with the host tests)
SMALL_SIZES = ((64, 96), (96, 160))
BIG_SIZE = (352, 608)
SHIPPED_CASES = [(stem, hw) for stem in ("mnet25", "mnet-deconv-0517") for hw in SMALL_SIZES] + [("mnet25", BIG_SIZE)]
DERIVED_CASES = [("mnet25", (64, 96)), ("mnet-deconv-0517", (64, 96)), ("mnet25", (96, 160))]
WEIGHT_SETS = ("shipped", "degenerate", "ragged")


def case_frames(base_frame, hw):
    """the three distinct frames of one call, cut from the fixture photo"""
    from schedule_ref import edge_frame
    frames = [edge_frame(base_frame, hw, k) for k in range(3)]
    assert len({f.tobytes() for f in frames}) == 3
    return frames


def weight_set_dirs(nets, assets: str, mkdir: Callable[[str], str]) -> Dict[str, str]:
    """weight set -> model directory.  Shipped: the assets; derived: written at run time into mkdir(name), nothing is stored."""
    import os
    from int8_derived import derive
    from oracle.caffe_io import write_rfw
    dirs = {"shipped": assets}
    for ws, make in (("degenerate", lambda n: derive(n, "degenerate")), ("ragged", derive_ragged)):
        d = mkdir(ws)
        for stem, net in nets.items():
            write_rfw(make(net), os.path.join(d, stem + ".rfw"))
        dirs[ws] = d
    return dirs
