"""The GEMM family (csrc/k_gemm.hip, k_gemm16.hip, k_gemm256.hip), its implicit-GEMM convolution loaders and the fused QK-norm +
RoPE + KV-append epilogue: float64 references, per-element error bounds, the case list and the CPU restatements of the kernels'
plausible mistakes.  Same method as tests/ops_ref.py, whose helpers it reuses.  Shared by tests/test_gemm_ref_host.py (CPU: an honest
float32 evaluation lies inside every bound, every listed mutant outside) and tests/test_gpu_gemm_epilogues.py (GPU: one launch per case
through q3a_selftest_gemm_launch / q3a_selftest_qkrope_launch, every element of every output buffer compared).

A result is a whole output buffer: float64 values where the launch must write, and the buffer's initial content (a NaN sentinel, or
the residual where the output aliases it) everywhere else -- rows a row map drops, columns N..ldo, rows past M, cache rows no token
names.  Written elements are compared against the bound, the others for equality with the initial content.

Bounds (u = 2^-24; each derivation stands next to its function):
    fp32 dot product of exactly representable operands     (K + 2) u sum|x||w|                          ops_ref.matmul_bound
    an epilogue addition                                    + u |result|
    fp32 x rounded to bf16 once (launch_gemm, split = 0)    + sum half_ulp_bf16(x) |w|                   (<= 2^-8 sum|x||w|)
    hi + lo split (launch_gemm, split = 1)                  + 2^-8 sum half_ulp_bf16(x) |w|, 2 K terms   (<= 2^-16 sum|x||w|)
    bf16 output                                             half_ulp_bf16(|ref| + e) + e
    gelu_erf, silu_f (precise kernels)                      ops_ref.unary_bound("gelu" / "silu"): k_ops.hip evaluates the same expressions
    gelu_fast                                               2 x 3.85e-7 max(1, |x|) + 1.13 e
    silu_fast                                               ((1 - sigmoid x)(2 |x| + 2) + 4) u |silu x| + 1.1 e
    RMS-norm + rotation                                     qk_bound
A bf16 rounding is bounded by half a bf16 ulp of the value, which is 2^-8 |v| at the bottom of a binade and 2^-9 |v| only at its top
(bf16 keeps 8 significant bits): torch's own conversion of 1 + 2^-8 + 2^-20 is off by 0.0039 = 2^-8.0.

Worst excess (|got - ref| / bound, <= 1 passes) on an MI355X, printed by tests/test_gpu_gemm_epilogues.py:
    family                                          fp32 out    bf16 out (half-ulp bounds: near 1 by construction)
    launch_gemm, split 0 / 1, every tile            0.401       -
    launch_gemm16_small, every tile form            0.043       0.997
    launch_gemm256, persist 0 / 1 / 2               0.018       0.993
    launch_gemm256 + split tail                     0.022       0.996
    ConvA (launch_conv3x3s2_gemm)                   0.243       -
    ConvA16 / ConvA256                              0.004       0.976
    launch_gemm256_qkrope (and its split)           0.010       0.995
    launch_qknorm_rope_kv                           0.216       1.000  (ties of exact fp32 inputs sit exactly on half an ulp)
    gelu_fast alone, exact inputs                   0.477       (3.67e-7 max(1, |x|) at x = 0.80; gate 7.70e-7)
    silu_fast alone, exact inputs                   0.592       (14.9 u relative at x = -11.8; 1 ulp assumed for v_exp_f32 and v_rcp_f32)
"""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import ops_ref as R
from ops_ref import U, bf16_round, conv2d_ref, excess, f32, im2col, inside, matmul_bound

SENT32 = np.uint32(0x7FC5A5A5)   # what an untouched fp32 output element holds (a NaN no kernel produces)
SENT16 = np.uint16(0x7FC5)       # the same for bf16 outputs
HUGE_TILES = 1 << 30             # gemm256_min_tiles: never dispatch to gemm256
PAST_M = 3                       # output rows behind the last GEMM row: must come back untouched
GELU_FAST_WORST = 3.85e-7        # float32 restatement of dev.h gelu_fast vs float64 erf-GELU, per max(1, |x|) (test_gemm_ref_host.py sweeps it)
GELU_SLOPE, SILU_SLOPE = 1.13, 1.1   # max |gelu'| = 1.129 (x = 1.41), max |silu'| = 1.0998 (x = 2.40)


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def bf16_bits(x):
    """uint16 bit patterns of bf16-representable fp32 values."""
    b = f32(x).view(np.uint32)
    assert not (b & np.uint32(0xFFFF)).any(), "not bf16-representable"
    return (b >> np.uint32(16)).astype(np.uint16)


def bf16_from_bits(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_truncate(x):
    return (f32(x).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


# bf16 has 8 significant bits: the spacing at v = m 2^e (0.5 <= m < 1) is 2^(e - 8), round to nearest moves a value by at most half of it.
def half_ulp_bf16(v):
    v = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(v)
    return np.where(v > 0, np.ldexp(1.0, e - 9), 0.0)


def _t64(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float64))


def gelu64(x):
    return 0.5 * x * (1.0 + torch.special.erf(_t64(x) / math.sqrt(2.0)).numpy())


def silu64(x):
    return x / (1.0 + np.exp(-x))


def gelu_fast_f32(x):
    """dev.h gelu_fast in float32 numpy: erfc by Abramowitz & Stegun 7.1.28, six multiply-adds, four squarings, one reciprocal."""
    x = f32(x)
    z = np.abs(x) * np.float32(0.70710678118654752440)
    p = np.float32(0.0000430638)
    for c in (0.0002765672, 0.0001520143, 0.0092705272, 0.0422820123, 0.0705230784, 1.0):
        p = p * z + np.float32(c)
    with np.errstate(over="ignore"):
        for _ in range(4):
            p = p * p
    pe = np.float32(1.0) / p
    return np.float32(0.5) * x * np.where(x >= 0, np.float32(2.0) - pe, pe)


def silu_fast_f32(x):
    """dev.h silu_fast in float32 numpy: x * rcp(1 + exp(-x))."""
    x = f32(x)
    with np.errstate(over="ignore"):
        return x * (np.float32(1.0) / (np.float32(1.0) + np.exp(-x)))


# ---------------------------------------------------------------------------------------------------------------------
# bounds of the epilogue steps.  v: float64 reference value so far, e: bound of the device's fp32 value against it.
# ---------------------------------------------------------------------------------------------------------------------
# fl(a^ + t) = (a^ + t)(1 + d), |d| <= u, t exact: the error e of a^ passes through, the rounding adds u |a^ + t| <= u (|v + t| + e).
def add_step(v, e, t):
    v2 = v + t
    return v2, e + U * (np.abs(v2) + e)


# GELU of a value known to e: |gelu'| <= 1.13 carries e through; the function's own error is
#   precise kernels (gelu_erf, the expression k_ops.hip evaluates): ops_ref.unary_bound("gelu") -- its ULP gate where x >= -1, the
#     legacy atol / rtol below (gate_domain);
#   default kernels (gelu_fast): twice the float32 restatement's worst error, 2 x 3.85e-7 max(1, |x|) -- the margin is for the
#     hardware reciprocal (not correctly rounded) and its error through p^16, of the order of 16 u relative on erfc.
def gelu_step(v, e, fast):
    g = gelu64(v)
    fn = 2.0 * GELU_FAST_WORST * np.maximum(1.0, np.abs(v)) if fast else R.unary_bound("gelu", v, g)
    return g, GELU_SLOPE * e + fn


# silu_fast = x * rcp(1 + exp(-x)), exp(-x) = v_exp_f32(-x log2 e).  The argument t = fl(-x fl(log2 e)) carries two roundings, 2 u |t|,
# which 2^t turns into the relative error 2 u |t| ln 2 = 2 u |x|; the guides state no accuracy for v_exp_f32 and v_rcp_f32, so 1 ulp
# (<= 2 u relative) each is ASSUMED.  E = exp(-x) is thus known to (2 |x| + 2) u relative; in 1 + E that weighs E / (1 + E) =
# 1 - sigmoid(x), plus u for the addition; the reciprocal adds 2 u, the product with x one more:
#     relative error of silu_fast(x) <= ((1 - sigmoid x)(2 |x| + 2) + 4) u,
# plus 2^-126 absolute where exp overflows or the result leaves the normal range.  The precise kernels evaluate silu_f = x / (1 + expf(-x)),
# the expression behind ops_ref's "silu" gate.  An input known to e moves the result by at most 1.1 e (|silu'| <= 1.1).
def silu_step(v, e, fast):
    s = silu64(v)
    if fast:
        with np.errstate(over="ignore"):
            q = 1.0 / (1.0 + np.exp(v))
        fn = (q * (2.0 * np.abs(v) + 2.0) + 4.0) * U * np.abs(s) + 2.0 ** -126
    else:
        fn = R.unary_bound("silu", v, s)
    return s, SILU_SLOPE * e + fn


# silu(g) * up: (s + ds)(p + dp) - s p = p ds + s dp + ds dp, and the product is rounded once.
def glu_step(g, eg, up, eu, fast):
    s, es = silu_step(g, eg, fast)
    v = s * up
    e = np.abs(up) * es + np.abs(s) * eu + es * eu
    return v, e + U * (np.abs(v) + e)


# round to nearest even of a value known to e: the rounded value is within half a bf16 ulp of the device's fp32 value, which is within e of
# the reference (and at most |ref| + e large, so the spacing is taken there: a value pushed into the next binade is covered)
def bf16_out_bound(v, e):
    return half_ulp_bf16(np.abs(v) + e) + e


# ---------------------------------------------------------------------------------------------------------------------
# dense and convolution cases
# ---------------------------------------------------------------------------------------------------------------------
def conv_dims(c):
    return (c["H"] - 1) // 2 + 1, (c["W"] - 1) // 2 + 1


def im2col_nhwc(x, right_zero=True, bottom_zero=True, img_lost=False):
    """[imgs OH OW, 9 C] matrix of a 3x3 / stride 2 / pad 1 convolution over NHWC x, k = (kh, kw, c) as the loaders state.  Pixels are
    fetched by linear address, as a kernel does: with right_zero / bottom_zero off (the mutants) a tap right of the image reads the next
    row's first pixel, a tap below it the next image's first row (zeros past the end of the array)."""
    imgs, H, W, C = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    flat = np.concatenate([x.reshape(-1, C), np.zeros((1, C), x.dtype)])
    img, oh, ow = np.meshgrid(np.arange(imgs), np.arange(OH), np.arange(OW), indexing="ij")
    img, oh, ow = img.reshape(-1), oh.reshape(-1), ow.reshape(-1)
    if img_lost: img = np.zeros_like(img)
    cols = np.zeros((img.size, 9, C), x.dtype)
    for kh in range(3):
        for kw in range(3):
            ih, iw = oh * 2 - 1 + kh, ow * 2 - 1 + kw
            ok = (ih >= 0) & (iw >= 0)
            if bottom_zero: ok &= ih < H
            if right_zero: ok &= iw < W
            lin = (img * H + ih) * W + iw
            ok &= (lin >= 0) & (lin < imgs * H * W)
            cols[:, kh * 3 + kw] = flat[np.where(ok, lin, imgs * H * W)]
    return cols.reshape(img.size, 9 * C)


def _rowmap(kind, M, g):
    if kind == "none": return None
    rm = g.permutation(M).astype(np.int32)           # into rows [0, M): the PAST_M rows behind stay untouched
    if kind == "perm_drop": rm[np.arange(M) % 11 == 5] = -1
    return rm


_operands = {}


def materialize(c):
    """The arrays of a case.  X, W and the epilogue operands depend on the shape alone, so that the cases of one shape share the float64
    product (product64)."""
    conv = c["family"] == "conv"
    M, N, K = c["M"], c["N"], c["K"]
    fp32x = c["launcher"] in ("gemm", "conv")
    key = (c["family"], M, N, K, fp32x) + ((c["imgs"], c["H"], c["W"], c["C"]) if conv else ())
    if key not in _operands:
        if len(_operands) > 6: _operands.clear()
        g = rng_of("ops", key)
        if conv:
            # every pixel its own value: image, row, column and channel all show in it (plus noise), so an index slip changes the sums
            imgs, H, W, C = c["imgs"], c["H"], c["W"], c["C"]
            i, h, w_, ch = np.meshgrid(np.arange(imgs), np.arange(H), np.arange(W), np.arange(C), indexing="ij")
            x = 0.5 * g.standard_normal((imgs, H, W, C)) + 0.37 * np.sin(1.0 + 1.3 * i + 0.7 * h + 0.45 * w_ + 0.11 * ch)
        else:
            x = g.standard_normal((M, K))
        x = f32(x) if fp32x else bf16_round(x)
        w = bf16_round(g.standard_normal((N, K)) / math.sqrt(K))
        _operands[key] = dict(x=x, w=w, bias=f32(0.5 * g.standard_normal(N)), g_seed=key)
    d = dict(_operands[key])
    g = rng_of("epi", c["name"])
    ldo, rows = c["ldo"], M + PAST_M
    d["rows"] = rows
    d["bias"] = d["bias"] if c["bias"] else None
    d["addend"] = f32(0.5 * g.standard_normal((c["addend"], ldo))) if c["addend"] else None
    d["rowmap"] = _rowmap(c["rowmap"], M, g)
    d["resid"] = f32(g.standard_normal((rows, ldo))) if c["resid"] != "none" else None
    if not conv:   # the row stride: columns K..lda hold values that would show in any sum
        xs = np.full((M, c["lda"]), 1000.0, np.float32)
        xs[:, :K] = d["x"]
        d["x_strided"] = xs
    if c["resid"] == "inplace": d["init"] = d["resid"].view(np.uint32).copy()
    elif c["out16"]: d["init"] = np.full((rows, ldo), SENT16, np.uint16)
    else: d["init"] = np.full((rows, ldo), SENT32, np.uint32)
    return d


def decode(raw, out16):
    """A raw output buffer as float64: the sentinel reads NaN, any other non-finite value +inf (never equal to a reference)."""
    raw = np.asarray(raw)
    v = (bf16_from_bits(raw) if out16 else raw.view(np.float32)).astype(np.float64)
    sent = raw == (SENT16 if out16 else SENT32)
    return np.where(sent, np.nan, np.where(np.isfinite(v), v, np.inf))


_products = {}


def product64(c, d, A):
    """float64 X . W^T and sum |x||w| of the case's shape (cached: the epilogue kinds of a shape share them)."""
    key = d["g_seed"]
    if key not in _products:
        if len(_products) > 3: _products.clear()
        W = d["w"].astype(np.float64)
        hu = half_ulp_bf16(A) @ np.abs(W).T if c["launcher"] in ("gemm", "conv") else None
        _products[key] = (A @ W.T, np.abs(A) @ np.abs(W).T, hu)
    return _products[key]


def a_matrix(c, d, mut=None, dt=np.float64):
    """The logical A operand [M][K] (the im2col matrix for a convolution), with the loader mutants."""
    if c["family"] == "conv":
        x = d["x"].astype(dt)
        if mut == "k_order_c_kh_kw":   # ops_ref.im2col orders k = (c, kh, kw): the loader reading the weight's k in that order
            return im2col(np.ascontiguousarray(x.transpose(0, 3, 1, 2)), (c["N"], c["C"], 3, 3), (2, 2), (1, 1), (1, 1)).astype(dt)
        return im2col_nhwc(x, right_zero=mut != "right_pad_neighbour", bottom_zero=mut != "bottom_pad_neighbour", img_lost=mut == "image_lost")
    return d["x"].astype(dt)


def fp32_product_bound(c, cond, hu):
    """Bound of the accumulator against the float64 product of the operands AS GIVEN.
    bf16 launchers: both operands exact, (K + 2) u sum|x||w| (ops_ref.matmul_bound).
    launch_gemm, split = 0: the kernel multiplies x^ = bf16(x), |x - x^| <= half_ulp_bf16(x) (<= 2^-8 |x|): sum half_ulp_bf16(x) |w| for
      the operand, and the dot product of x^ (|x^| <= (1 + 2^-8) |x|) on top.
    split = 1: hi = bf16(x); r = x - hi is exact in fp32 (it has at most 16 significant bits) and |r| <= half_ulp_bf16(x); lo = bf16(r),
      |r - lo| <= 2^-8 |r|.  So |x - hi - lo| <= 2^-8 half_ulp_bf16(x) (<= 2^-16 |x|), and the dot product has 2 K terms of total
      magnitude <= (1 + 2^-7) sum|x||w|."""
    K = c["K"]
    if c["launcher"] not in ("gemm", "conv"):
        assert K * K * U <= 2.0
        return (K + 2) * U * cond
    if not c["split"]:
        return hu + (K + 2) * U * (1.0 + 2.0 ** -8) * cond
    assert 4 * K * K * U <= 2.0
    return 2.0 ** -8 * hu + (2 * K + 2) * U * (1.0 + 2.0 ** -7) * cond


def _fast(c):
    return c["launcher"] not in ("gemm", "conv")   # the bf16-activation kernels use gelu_fast / silu_fast, k_gemm.hip gelu_erf / silu_f


def _glu_cols(N, mut):
    c2 = np.arange(N // 2)
    blk = 32 if mut == "interleave_32" else 16        # [blk gate | blk up] row blocks of W
    gi = ((c2 // blk) * 2 * blk + c2 % blk) % N
    ui = ((c2 // blk) * 2 * blk + blk + c2 % blk) % N
    return (ui, gi) if mut == "gate_up_swapped" else (gi, ui)


def evaluate(c, d, mut=None, honest=False):
    """(full, written, bound): the whole output buffer as float64 (initial content where nothing is written), the mask of the written
    elements and, for the reference (no mutant, not honest), the per-element bound.  honest: an fp32 evaluation with torch's matmul on the
    operands the kernel multiplies and the numpy restatements of the fast activations.  mut: one plausible mistake."""
    M, N, K, ldo = c["M"], c["N"], c["K"], c["ldo"]
    fast, glu = _fast(c), c["glu"]
    dt = np.float32 if honest else np.float64
    A = a_matrix(c, d, mut, dt)
    W = d["w"].astype(dt)
    e = None
    if honest:
        if not fast:   # what k_gemm.hip multiplies: bf16(x), or the hi + lo pair
            hi = bf16_round(A)
            A = np.concatenate([hi, bf16_round(A - hi)], 1) if c["split"] else hi
            if c["split"]: W = np.concatenate([W, W], 1)
        S = torch.matmul(torch.from_numpy(np.ascontiguousarray(A)), torch.from_numpy(np.ascontiguousarray(W)).T).numpy()
    elif mut in ("half_k_dropped", "k_order_c_kh_kw", "right_pad_neighbour", "bottom_pad_neighbour", "image_lost"):
        kk = K - 32 if mut == "half_k_dropped" else K
        S = A[:, :kk] @ W[:, :kk].T
    else:
        S, cond, hu = product64(c, d, A)
        if mut is None: e = fp32_product_bound(c, cond, hu)
    track = e is not None
    if not track: e = np.zeros((), dt)
    add = (lambda v, e, t: add_step(v, e, t)) if track else (lambda v, e, t: ((v + t.astype(dt)).astype(dt), e))
    m = np.arange(M)
    M1 = c.get("split_rows", 0)
    tail = m >= M1 if M1 else np.zeros(M, bool)
    rm = d["rowmap"]
    if rm is None: orow = m.copy()
    elif mut == "tail_rowmap_unshifted": orow = np.where(tail, rm[np.where(tail, m - M1, 0)], rm)
    else: orow = rm.copy()
    keep = orow >= 0
    oc = np.where(keep, orow, 0)
    bias = None if (d["bias"] is None or mut == "bias_dropped") else d["bias"]

    def act_of(v, e):
        if not c["act"]: return v, e
        if track: return gelu_step(v, e, fast)
        if honest: return (gelu_fast_f32(v) if fast else F.gelu(torch.from_numpy(v)).numpy()), e
        return gelu64(v), e

    if glu:
        gi, ui = _glu_cols(N, mut)
        g_, eg = S[:, gi], (e[:, gi] if track else e)
        u_, eu = S[:, ui], (e[:, ui] if track else e)
        if bias is not None:
            g_, eg = add(g_, eg, bias[gi][None, :])
            u_, eu = add(u_, eu, bias[ui][None, :])
        if track: v, e = glu_step(g_, eg, u_, eu, fast)
        elif honest: v = ((silu_fast_f32(g_) if fast else F.silu(torch.from_numpy(g_)).numpy()) * u_).astype(dt)
        else: v = silu64(g_) * u_
        ncols = N // 2
    else:
        v, ncols = S, N
        if bias is not None: v, e = add(v, e, bias[None, :])
        if d["addend"] is not None:
            arow = (oc if mut == "addend_by_out_row" else m) % c["addend"]
            v, e = add(v, e, d["addend"][arow][:, :N])
        rrow = None
        if d["resid"] is not None:
            rrow = m if mut == "resid_at_gemm_row" else np.where(tail, oc - M1, oc) if mut == "tail_resid_unshifted" else oc
        if mut == "act_after_resid" and rrow is not None:
            v, e = add(v, e, d["resid"][rrow][:, :N])
            v, e = act_of(v, e)
        else:
            v, e = act_of(v, e)
            if rrow is not None: v, e = add(v, e, d["resid"][rrow][:, :N])
    if c["out16"]:
        if track: e = bf16_out_bound(v, e)
        elif mut == "bf16_truncate": v = bf16_truncate(v).astype(np.float64)
        elif honest: v = bf16_round(v)
    # ---- placement ----
    full = decode(d["init"], c["out16"])
    written = np.zeros(full.shape, bool)
    bound = np.zeros(full.shape) if track else None
    dst = np.where(tail, oc - M1, oc) if mut == "tail_out_unshifted" else oc
    order = np.argsort(tail, kind="stable")   # the head launch first, the tail launch behind it
    rows = order[keep[order]]
    full[dst[rows], :ncols] = v[rows]
    written[dst[rows], :ncols] = True
    if track: bound[dst[rows], :ncols] = e[rows]
    if mut == "dropped_row_written" and not keep.all():   # the `orow < 0` test missing: the row lands on the row its index clamps to
        full[0, :ncols] = v[~keep][-1]
        written[0, :ncols] = True
    if mut == "tail_row_clamped_stored":   # rows past M of the last tile computed from row M - 1 (the loaders clamp) AND stored
        full[M:, :ncols] = v[M - 1]
        written[M:, :ncols] = True
    return full, written, bound


def accepts(full, exp):
    """full: a whole output buffer as float64 (decode() of a device buffer, or a CPU evaluation).  Inside the bound where the reference is
    written, equal to the initial content everywhere else."""
    ref, written, bound = exp
    full = np.asarray(full, np.float64)
    if full.shape != ref.shape: return False
    if not np.array_equal(full[~written], ref[~written], equal_nan=True): return False
    return inside(full[written], ref[written], bound[written])


def worst_excess(full, exp):
    ref, written, bound = exp
    e = excess(np.asarray(full, np.float64)[written], ref[written], bound[written])
    return float(e.max()) if e.size else 0.0


# ---- epilogue kinds: the engine's own combinations (csrc/engine.cpp), one dict each ----
def _kind(**kw):
    k = dict(bias=True, addend=0, rowmap="none", act=0, resid="none", out16=False, glu=False, pad_ldo=0, pad_lda=0)
    k.update(kw)
    return k


KINDS = {
    "conv_out": _kind(rowmap="perm_drop", addend=13),                  # fp32 + bias + positional addend through a row map with drops
    "conv_out_nobias": _kind(bias=False, rowmap="perm_drop", addend=13),
    "qkv_bf16": _kind(out16=True),                                     # encoder qkv
    "proj_f32": _kind(),                                               # encoder qkv in precise mode, proj2
    "resid_inplace": _kind(resid="inplace"),                           # out / fc2 / o / down: x += X W^T + b
    "fc1_bf16_gelu": _kind(out16=True, act=1),                         # fc1 / proj1
    "f32_gelu": _kind(act=1),                                          # the same at fp32 resolution
    "conv3_bf16_gelu_perm": _kind(out16=True, act=1, rowmap="perm"),   # conv3: permuting row map
    "all_at_once": _kind(addend=13, rowmap="perm_drop", act=1, resid="sep"),
    "ldo_plus_8": _kind(out16=True, pad_ldo=8),
    "lda_plus_8": _kind(pad_lda=8),
    "glu_bf16": _kind(glu=True, out16=True),                           # gate / up
    "glu_bf16_nobias": _kind(glu=True, out16=True, bias=False),
    "glu_bf16_ldo4": _kind(glu=True, out16=True, pad_ldo=4),           # ldo % 8 != 0: the 4-column store path
    "glu_f32": _kind(glu=True),
    "glu_f32_nobias": _kind(glu=True, bias=False),
}
KIND_MUTANTS = {
    "conv_out": ["bias_dropped", "addend_by_out_row", "dropped_row_written"], "conv_out_nobias": ["addend_by_out_row"],
    "qkv_bf16": ["bias_dropped", "bf16_truncate", "half_k_dropped"], "proj_f32": ["bias_dropped", "half_k_dropped", "tail_row_clamped_stored"],
    "resid_inplace": ["bias_dropped"], "fc1_bf16_gelu": ["bias_dropped", "bf16_truncate"], "f32_gelu": ["bias_dropped"],
    "conv3_bf16_gelu_perm": ["bias_dropped"], "all_at_once": ["resid_at_gemm_row", "act_after_resid", "addend_by_out_row", "dropped_row_written"],
    "ldo_plus_8": ["bias_dropped"], "lda_plus_8": ["bias_dropped"], "glu_bf16": ["gate_up_swapped", "interleave_32", "bias_dropped", "bf16_truncate"],
    "glu_bf16_nobias": ["gate_up_swapped", "interleave_32"], "glu_bf16_ldo4": ["gate_up_swapped"], "glu_f32": ["gate_up_swapped", "interleave_32"],
    "glu_f32_nobias": ["gate_up_swapped"],
}
F32_KINDS = ["conv_out", "conv_out_nobias", "proj_f32", "resid_inplace", "f32_gelu", "all_at_once", "lda_plus_8", "glu_f32", "glu_f32_nobias"]
BF16_KINDS = ["conv_out", "conv_out_nobias", "qkv_bf16", "proj_f32", "resid_inplace", "fc1_bf16_gelu", "f32_gelu", "conv3_bf16_gelu_perm", "all_at_once",
              "ldo_plus_8", "lda_plus_8", "glu_bf16", "glu_bf16_nobias", "glu_bf16_ldo4"]


def _dense(group, launcher, form, M, N, K, kind, split=0, knobs=None, n_glu=None, mutants=None, split_rows=0):
    k = KINDS[kind]
    if k["glu"]: N = n_glu
    ncols = N // 2 if k["glu"] else N
    c = dict(family="dense", group=group, launcher=launcher, form=form, split=split, M=M, N=N, K=K, lda=K + k["pad_lda"], ldo=ncols + k["pad_ldo"],
             kind=kind, knobs=dict(knobs or {}), split_rows=split_rows, mutants=list(KIND_MUTANTS[kind] if mutants is None else mutants))
    c.update({f: k[f] for f in ("bias", "addend", "rowmap", "act", "resid", "out16", "glu")})
    if K < 64: c["mutants"] = [m for m in c["mutants"] if m != "half_k_dropped"]
    c["name"] = f"{group}-{kind}"
    return c


# (M, N, K, N for GLU) per tile form of launch_gemm16_small (csrc/k_gemm16.hip): the K-split 32 x 32 tiles (K % 256 == 0, K % 128 == 0
# only), the 32 x 64 ring, BK = 32, the element-wise epilogue (N % 4 != 0), and the smallest ragged M x N that reaches 384 tiles of
# 64 x 64 (24 x 16 tiles) and of 128 x 128
GEMM16_FORMS = [
    ("ksplit256", 33, 36, 512, None), ("ksplit128", 70, 40, 640, None), ("ring32x64", 70, 96, 64, 96), ("bk32", 130, 200, 96, 224),
    ("elementwise", 70, 98, 64, None), ("tile64", 1473, 964, 192, 992), ("tile128", 2945, 1924, 128, 1952),
]
BIG_FORMS = ("tile64", "tile128")                  # millions of elements: every kind runs, one mutant each is restated
# launch_gemm (csrc/k_gemm.hip) picks its tile by workgroup count and K: 32 x 32 (64 for GLU) x 128, 64 x 64 x 32, 64 x 64 x 128, 128 x 128 x 64
GEMM_FORMS = [("t32k128", 70, 40, 128, 96), ("t64k32", 130, 200, 96, 224), ("t64k128", 1473, 964, 128, 992), ("t128k64", 2945, 1924, 192, 1952)]
# gemm256, dense: two tile rows and two tile columns, both ragged; M % 4 zero (residual prefetch) and not; N % 8 zero (8-column bf16
# stores) and not; two K tiles (only seams) and five; walked by one workgroup per tile, one per CU, and exactly two
GEMM256_SHAPES = [(300, 328, 128), (301, 324, 320), (300, 324, 320), (301, 328, 128)]
GEMM256_N_GLU = 352
SPLIT_TAIL = (65536 + 37, 72, 128, 96)             # 257 tiles of 256 x 256, remainder 1: rows 65536.. go to the small tiles
SPLIT_TAIL_ROWS = 65536


def dense_cases():
    out = []
    for form, M, N, K, ng in GEMM16_FORMS:
        for kind in BF16_KINDS:
            k = KINDS[kind]
            if k["glu"] and ng is None: continue
            if form == "elementwise" and (k["glu"] or k["pad_ldo"]): continue
            muts = KIND_MUTANTS[kind][:1] if form in BIG_FORMS else None
            launcher = "gemm16" if form in ("ring32x64", "ksplit256") else "gemm16_small"   # both doors: with the dispatch forbidden, and behind it
            out.append(_dense(f"gemm16-{form}", launcher, form, M, N, K, kind, knobs=dict(gemm256_min_tiles=HUGE_TILES), n_glu=ng, mutants=muts))
    for form, M, N, K, ng in GEMM_FORMS:
        for split in (0, 1):
            for kind in F32_KINDS:
                muts = KIND_MUTANTS[kind][:1] if form in ("t64k128", "t128k64") else None
                out.append(_dense(f"gemm-{form}-split{split}", "gemm", form, M, N, K, kind, split=split, n_glu=ng, mutants=muts))
    for M, N, K in GEMM256_SHAPES:
        for persist in (0, 1, 2):
            for kind in BF16_KINDS:
                muts = None if persist == 1 else KIND_MUTANTS[kind][:1]
                out.append(_dense(f"gemm256-{M}x{N}x{K}-persist{persist}", "gemm16", "gemm256", M, N, K, kind,
                                  knobs=dict(gemm256_min_tiles=0, gemm256_persist=persist), n_glu=GEMM256_N_GLU, mutants=muts))
    M, N, K, ng = SPLIT_TAIL
    kn = dict(gemm256_min_tiles=0)
    T = SPLIT_TAIL_ROWS
    out += [
        _dense("gemm256-split_tail", "gemm16", "gemm256+tail", M, N, K, "resid_inplace", knobs=kn, split_rows=T, mutants=["tail_resid_unshifted", "tail_out_unshifted"]),
        _dense("gemm256-split_tail", "gemm16", "gemm256+tail", M, N, K, "qkv_bf16", knobs=kn, split_rows=T, mutants=["tail_out_unshifted"]),
        _dense("gemm256-split_tail", "gemm16", "gemm256+tail", M, N, K, "conv3_bf16_gelu_perm", knobs=kn, split_rows=T, mutants=["tail_rowmap_unshifted"]),
        _dense("gemm256-split_tail", "gemm16", "gemm256+tail", M, N, K, "glu_bf16", knobs=kn, n_glu=ng, split_rows=T, mutants=["tail_out_unshifted"]),
    ]
    return out


# convolutions: (H, W) even and odd both ways -- (16, 25) -> (8, 13) is conv3's geometry, the only one of the engine's in which the right
# padding column is read; C = 64 is the BK = 64 loader no preset reaches, C = 96 gives K % 64 == 32 (gemm256's half tile past K);
# gemm256 needs M >= 128: (16, 25) x 2 images = 208 rows, (16, 13) x 6 = 336 and (16, 25) x 3 = 312 (a second 256-row tile)
CONV_GEOMS = [  # name, imgs, H, W, C, Cout
    ("8x10_i1_c32", 1, 8, 10, 32, 32), ("7x9_i3_c64", 3, 7, 9, 64, 36), ("5x4_i3_c96", 3, 5, 4, 96, 40), ("16x25_i1_c32", 1, 16, 25, 32, 40),
    ("7x9_i1_c96", 1, 7, 9, 96, 32), ("8x10_i3_c64", 3, 8, 10, 64, 40), ("5x4_i1_c32", 1, 5, 4, 32, 36),
    ("16x25_i2_c96", 2, 16, 25, 96, 36), ("16x13_i6_c64", 6, 16, 13, 64, 32), ("16x25_i3_c64", 3, 16, 25, 64, 40), ("16x25_i2_c32", 2, 16, 25, 32, 32),
]


def _conv(group, launcher, geom, kind, split=0, knobs=None):
    name, imgs, H, W, C, Cout = geom
    k = KINDS[kind]
    c = dict(family="conv", group=group, launcher=launcher, form=group, split=split, imgs=imgs, H=H, W=W, C=C, N=Cout, K=9 * C, ldo=Cout + k["pad_ldo"],
             kind=kind, knobs=dict(knobs or {}), split_rows=0)
    OH, OW = conv_dims(c)
    c["M"] = imgs * OH * OW
    c["lda"] = c["K"]
    c.update({f: k[f] for f in ("bias", "addend", "rowmap", "act", "resid", "out16", "glu")})
    muts = ["k_order_c_kh_kw", "tail_row_clamped_stored"]
    if W % 2: muts.append("right_pad_neighbour")
    if H % 2 and imgs > 1: muts.append("bottom_pad_neighbour")   # (below the last image there is nothing to read)
    if imgs > 1: muts.append("image_lost")
    if c["K"] % 64 == 32: muts.append("half_k_dropped")
    if k["bias"]: muts.append("bias_dropped")
    c["mutants"] = muts
    c["name"] = f"{group}-{name}-{kind}"
    return c


def conv_cases():
    out = []
    for geom in CONV_GEOMS:
        M = geom[1] * ((geom[2] - 1) // 2 + 1) * ((geom[3] - 1) // 2 + 1)
        for split in (0, 1):
            for kind in ("f32_gelu", "proj_f32"):
                out.append(_conv(f"conv-split{split}", "conv", geom, kind, split=split))
        for kind in ("fc1_bf16_gelu", "proj_f32", "conv3_bf16_gelu_perm"):
            out.append(_conv("conv16-tiles", "conv16", geom, kind, knobs=dict(gemm256_min_tiles=HUGE_TILES)))
        if M >= 128:
            for persist in (0, 1, 2):
                for kind in ("fc1_bf16_gelu", "proj_f32", "conv3_bf16_gelu_perm"):
                    out.append(_conv(f"conv256-persist{persist}", "conv16", geom, kind, knobs=dict(gemm256_min_tiles=0, gemm256_persist=persist)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# per-head RMS-norm + RoPE + KV-cache append (RopeKvArgs, csrc/kernels.h)
# ---------------------------------------------------------------------------------------------------------------------
QK_EPS = 1e-6


def _qk(group, n_q, n_kv, fused, bias=False, kv_f32=0, q16=True, M=300, n_seq=3, knobs=None, split_rows=0, scratch=False, mutants=None):
    c = dict(family="qk", group=group, n_q=n_q, n_kv=n_kv, fused=fused, bias=bias, kv_f32=kv_f32, q16=q16, M=M, K=128, n_seq=n_seq, knobs=dict(knobs or {}),
             split_rows=split_rows, scratch=scratch, N=(n_q + 2 * n_kv) * 128)
    muts = ["rot_sign_flipped", "q_given_k_norm", "pos_from_row_index", "wrong_sequence", "v_normalised"] + (["partner_bias_dropped"] if bias else [])
    c["mutants"] = muts if mutants is None else mutants
    c["name"] = f"{group}-q{n_q}kv{n_kv}" + ("-bias" if bias else "") + ("-kvf32" if kv_f32 else "") + ("" if q16 else "-q_in_place") + (f"-M{M}" if M != 300 else "")
    return c


QK_SPLIT = (32768 + 45, 8, 32768)   # M, sequences, gemm256_split_rows: N = 512 -> 129 x 2 = 258 tiles, remainder 2


def qk_cases():
    out = []
    for n_q, n_kv in [(2, 1), (4, 2), (4, 1)]:
        for bias in (False, True):
            out.append(_qk("qkrope-fused", n_q, n_kv, 1, bias=bias, knobs=dict(gemm256_persist=1)))
        out.append(_qk("qkrope-fused-persist2", n_q, n_kv, 1, bias=True, knobs=dict(gemm256_persist=2), mutants=["partner_bias_dropped"]))
        for kv_f32 in (0, 1):
            for q16 in (True, False):
                out.append(_qk("qkrope-separate", n_q, n_kv, 0, kv_f32=kv_f32, q16=q16))
    M, S, T = QK_SPLIT
    out.append(_qk("qkrope-fused-split", 2, 1, 1, bias=True, M=M, n_seq=S, split_rows=T, scratch=True, mutants=["pos_from_row_index", "wrong_sequence"]))
    return out


def qk_materialize(c):
    g = rng_of("qk", c["name"])
    M, S, N, K = c["M"], c["n_seq"], c["N"], c["K"]
    # unequal lengths, positions that do not start at 0, sequence ids not in row order
    w = g.uniform(0.6, 1.4, S)
    lens = np.floor(w / w.sum() * (M - S)).astype(int) + 1
    lens[0] += M - lens.sum()
    starts = g.integers(3, 20, S)
    ids = g.permutation(S)
    row_seq = np.concatenate([np.full(n, i) for n, i in zip(lens, ids)]).astype(np.int32)
    row_pos = np.concatenate([st + np.arange(n) for n, st in zip(lens, starts)]).astype(np.int32)
    max_ctx = int((lens + starts).max()) + 7
    pos = np.arange(max_ctx)[:, None] * (10000.0 ** (-np.arange(64) / 64.0))[None, :]
    d = dict(row_seq=row_seq, row_pos=row_pos, max_ctx=max_ctx, cos=f32(np.cos(pos)), sin=f32(np.sin(pos)),
             q_norm=f32(1.0 + 0.3 * g.standard_normal(128)), k_norm=f32(1.0 + 0.3 * g.standard_normal(128)))
    if c["fused"]:
        d["x"] = bf16_round(g.standard_normal((M, K)))
        d["w"] = bf16_round(g.standard_normal((N, K)) / math.sqrt(K))
        d["bias"] = f32(0.5 * g.standard_normal(N)) if c["bias"] else None
        d["qkv"] = None
    else:
        d["qkv"] = f32(g.standard_normal((M, N)) * (1.0 + 0.5 * g.random((1, N))))
    return d


# y: the head's 128 projected values, each known to ey (0 for the separate kernel: its fp32 input is exact).  The kernel computes
#   ss^ = fl(sum y^2): each square rounded (u), chains of at most 20 additions (fused: 16 per lane + 3 DPP steps; separate: 1 + 6) --
#       |ss^ - ss| <= 22 u ss + sum (2 |y| ey + ey^2);
#   r^ = fl(1 / sqrt(fl(ss^ / 128 + eps))): the radicand's relative error halves, + u for adding eps (/ 128 is exact), and 1 / sqrtf is
#       granted ops_ref's "rsqrt" gate in ULPs (2 u relative per ULP): rho = dss / (2 (ss + 128 eps)) + (1 + 2 gate) u;
#   n^ = fl(fl(y^ r^) w): |n^ - n| <= r |w| ey + |n| (rho + 2 u) =: En;
#   out = fl(n_own c + n_partner' s), two products and one addition, or a product and a fused multiply-add:
#       |out^ - out| <= |c| En_own + |s| En_partner + 2 u (|n_own c| + |n_partner s|).
# v is copied: ey alone.  A bf16 destination adds bf16_out_bound.
def qk_bound(y, ey, wn, cosr, sinr, eps):
    ss = (y ** 2).sum(-1, keepdims=True)
    dss = 22.0 * U * ss + (2.0 * np.abs(y) * ey + ey ** 2).sum(-1, keepdims=True)
    rho = dss / (2.0 * (ss + 128.0 * eps)) + (1.0 + 2.0 * R.ULP_GATE["rsqrt"]) * U
    r = 1.0 / np.sqrt(ss / 128.0 + eps)
    n = y * r * wn
    En = r * np.abs(wn) * ey + np.abs(n) * (rho + 2.0 * U)
    c2, s2 = np.concatenate([cosr, cosr], -1), np.concatenate([sinr, sinr], -1)
    npar, Enpar = np.roll(n, 64, -1), np.roll(En, 64, -1)
    return np.abs(c2) * En + np.abs(s2) * Enpar + 2.0 * U * (np.abs(n * c2) + np.abs(npar * s2))


def _norm_rope(y, wn, cosr, sinr, eps, dt, sign=1.0, y_partner=None):
    """RMS-norm over 128 dims, weight, rotate_half with the rows' cos / sin ([rows][64]).  y_partner: the values the partner half
    contributes (the mutant that drops the partner's bias); sign -1: the rotation's sign flipped."""
    yp = y if y_partner is None else y_partner
    half = np.arange(128) < 64
    def one(own_first):   # the output half whose own dims are exact and whose partner dims come from yp
        mix = np.where(half == own_first, y, yp)
        ss = (mix * mix).sum(-1, keepdims=True, dtype=dt)
        r = (dt(1.0) / np.sqrt(ss / dt(128.0) + dt(eps))).astype(dt)
        return (mix * r * wn).astype(dt)
    n_a, n_b = one(True), one(False)
    c2, s2 = np.concatenate([cosr, cosr], -1).astype(dt), np.concatenate([sinr, sinr], -1).astype(dt)
    rot_a = np.concatenate([-n_a[..., 64:], n_a[..., :64]], -1) * dt(sign)
    rot_b = np.concatenate([-n_b[..., 64:], n_b[..., :64]], -1) * dt(sign)
    out_a, out_b = n_a * c2 + rot_a * s2, n_b * c2 + rot_b * s2
    return np.where(half, out_a, out_b).astype(dt)


def qk_evaluate(c, d, mut=None, honest=False):
    """{buffer name: (full, written, bound)} for q (q16, or the q columns of qkv in place), kcache, vcache and, when the case hands one
    in, the untouched remainder of qkv."""
    M, N, n_q, n_kv, S, max_ctx = c["M"], c["N"], c["n_q"], c["n_kv"], c["n_seq"], d["max_ctx"]
    dt = np.float32 if honest else np.float64
    track = mut is None and not honest
    if c["fused"]:
        X, W = d["x"].astype(dt), d["w"].astype(dt)
        if honest: Y = torch.matmul(torch.from_numpy(X), torch.from_numpy(W).T).numpy()
        else: Y = X @ W.T
        ey = matmul_bound(X, W.T) if track else 0.0
        Yb = Y
        if d["bias"] is not None:
            if track: Yb, ey = add_step(Y, ey, d["bias"][None, :])
            else: Yb = (Y + d["bias"][None, :].astype(dt)).astype(dt)
    else:
        Y = Yb = d["qkv"].astype(dt)
        ey = np.zeros((M, N)) if track else 0.0
    Ypart = Y if mut == "partner_bias_dropped" else None
    pos, seq = d["row_pos"].astype(np.int64), d["row_seq"].astype(np.int64)
    if mut == "pos_from_row_index": pos = np.minimum(np.arange(M), max_ctx - 1)
    if mut == "wrong_sequence": seq = (seq + 1) % S
    cosr, sinr = d["cos"][pos], d["sin"][pos]
    sign = -1.0 if mut == "rot_sign_flipped" else 1.0
    bf_kv, bf_q = not c["kv_f32"], c["q16"]

    def finish(v, e, to_bf16):
        if to_bf16:
            if track: e = bf16_out_bound(v, e)
            elif honest: v = bf16_round(v)
        return v.astype(np.float64), e

    res = {}
    sent = lambda shape, b16: np.full(shape, np.nan)
    # ---- q ----
    qw = d["k_norm"] if mut == "q_given_k_norm" else d["q_norm"]
    qv, qe = [], []
    for h in range(n_q):
        sl = slice(h * 128, (h + 1) * 128)
        v = _norm_rope(Yb[:, sl], qw.astype(dt), cosr, sinr, QK_EPS, dt, sign, None if Ypart is None else Ypart[:, sl])
        e = qk_bound(Yb[:, sl], ey[:, sl], qw.astype(np.float64), cosr.astype(np.float64), sinr.astype(np.float64), QK_EPS) if track else None
        v, e = finish(v, e, bf_q)
        qv.append(v); qe.append(e)
    qfull = np.concatenate(qv, 1)
    qb = np.concatenate(qe, 1) if track else None
    if c["q16"]:
        res["q16"] = (qfull, np.ones(qfull.shape, bool), qb)
        if d["qkv"] is not None:   # the fp32 matrix is then read only
            res["qkv"] = (d["qkv"].astype(np.float64), np.zeros((M, N), bool), np.zeros((M, N)) if track else None)
        elif c["scratch"]:         # the split's trailing rows leave their fp32 projection (+ bias) in the first rows of the scratch matrix
            M1 = c["split_rows"]
            full, wr = np.full((M, N), np.nan), np.zeros((M, N), bool)
            full[:M - M1], wr[:M - M1] = Yb[M1:], True
            b = np.zeros((M, N)) if track else None
            if track: b[:M - M1] = ey[M1:]
            res["qkv"] = (full, wr, b)
    else:
        full = d["qkv"].astype(np.float64).copy()
        wr = np.zeros((M, N), bool)
        full[:, :n_q * 128] = qfull
        wr[:, :n_q * 128] = True
        b = np.zeros((M, N)) if track else None
        if track: b[:, :n_q * 128] = qb
        res["qkv"] = (full, wr, b)
    # ---- k, v ----
    for name, base, normed in (("kcache", n_q, True), ("vcache", n_q + n_kv, mut == "v_normalised")):
        full = np.full((S, n_kv, max_ctx, 128), np.nan)
        wr = np.zeros(full.shape, bool)
        b = np.zeros(full.shape) if track else None
        for h in range(n_kv):
            sl = slice((base + h) * 128, (base + h + 1) * 128)
            if normed and name == "kcache":
                v = _norm_rope(Yb[:, sl], d["k_norm"].astype(dt), cosr, sinr, QK_EPS, dt, sign, None if Ypart is None else Ypart[:, sl])
                e = qk_bound(Yb[:, sl], ey[:, sl], d["k_norm"].astype(np.float64), cosr.astype(np.float64), sinr.astype(np.float64), QK_EPS) if track else None
            elif normed:   # the mutant: v normalised like k (no rotation)
                y = Yb[:, sl]
                v, e = y / np.sqrt((y * y).mean(-1, keepdims=True) + QK_EPS) * d["k_norm"].astype(dt), None
            else:
                v, e = Yb[:, sl], (ey[:, sl] if track else None)
            v, e = finish(v, e, bf_kv)
            full[seq, h, pos] = v
            wr[seq, h, pos] = True
            if track: b[seq, h, pos] = e
        res[name] = (full, wr, b)
    return res


def qk_accepts(got, exp):
    return all(accepts(got[k][0] if isinstance(got[k], tuple) else got[k], exp[k]) for k in exp)


# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = {"dense": dense_cases, "conv": conv_cases, "qk": qk_cases}
FAMILY_MUTANTS = {
    "dense": ["bias_dropped", "addend_by_out_row", "resid_at_gemm_row", "act_after_resid", "dropped_row_written", "tail_resid_unshifted",
              "tail_out_unshifted", "tail_rowmap_unshifted", "gate_up_swapped", "interleave_32", "bf16_truncate", "half_k_dropped", "tail_row_clamped_stored"],
    "conv": ["right_pad_neighbour", "bottom_pad_neighbour", "image_lost", "k_order_c_kh_kw", "tail_row_clamped_stored", "half_k_dropped", "bias_dropped"],
    "qk": ["rot_sign_flipped", "partner_bias_dropped", "q_given_k_norm", "pos_from_row_index", "wrong_sequence", "v_normalised"],
}


def groups(family):
    """Cases of a family by group (one launcher, tile form and shape): the unit of a parametrised test."""
    out = {}
    for c in FAMILIES[family]():
        out.setdefault(c["group"], []).append(c)
    return out
