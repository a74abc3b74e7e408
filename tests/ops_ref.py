"""Op-level veneer (include/q3asr_ops.h, csrc/k_ops.hip): float64 references, per-element error bounds, the case list and
the CPU restatements of the kernels' plausible mistakes.  Shared by tests/test_ops_ref_host.py (CPU: torch's own float32 op
lies inside every bound, every listed mutant outside) and tests/test_gpu_ops_shapes.py (GPU: the kernels at the same cases).

Every expected value is a plain float64 restatement (numpy, or torch in float64) of the op on the float32 inputs.  Every
tolerance is a per-element bound from first-order rounding analysis with u = 2^-24 (round to nearest, fp32), derived next to
the function that computes it; nothing is a hand-picked atol.  Ops that do no arithmetic are compared for equality.

Library functions (exp, sin, cos, log10, erf-GELU, SiLU, pow, sqrt, rsqrt) cannot be bounded from first principles here: they
are compared in ULPs of the fp32 result against float64, gated at twice the worst value measured on an MI355X over the
sweeps of `unary_sweep`, and never looser than the atol / rtol tests/test_ops_veneer.py uses for the function at |x| <= 4.

    function        worst ULP measured (at x)       gate (2 x)
    exp             0.776  (0.4326)                 1.552
    sin             1.413  (-22.24)                 2.826
    cos             1.480  (-1.3192)                2.960
    log10           2.126  (0.24115)                4.252
    gelu, x >= -1   2.528  (-0.7983)                5.056      (below -1: the existing atol / rtol only, see gate_domain)
    silu            1.837  (-1.9902)                3.674
    pow(x, 1.5)     1.213  (3.4037)                 2.426
    sqrt            0.500  (1.2986)                 1.000
    rsqrt           1.395  (1.28e-32)               2.790
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
SUB = 2.0 ** -149   # spacing of fp32 subnormals
F32, F16, BF16, I64, I32, BOOL = range(6)   # qwen3_asr_rs_amd.tensor dtype codes

# worst |got - ref| / ulp(ref) on an MI355X over unary_sweep(name) (tests/test_gpu_ops_shapes.py prints them), and the gate
ULP_MEASURED = {"exp": 0.776, "sin": 1.413, "cos": 1.480, "log10": 2.126, "gelu": 2.528, "silu": 1.837, "pow": 1.213, "sqrt": 0.500, "rsqrt": 1.395}
ULP_GATE = {k: 2.0 * v for k, v in ULP_MEASURED.items()}
# (atol, rtol) of tests/test_ops_veneer.py::test_ops_against_torch per function: the ceiling of the gate at |x| <= 4
LEGACY_TOL = {"exp": (1e-6, 2e-6), "sin": (2e-6, 1e-5), "cos": (2e-6, 1e-5), "log10": (2e-6, 1e-5), "gelu": (2e-6, 1e-5),
              "silu": (2e-6, 1e-5), "pow": (1e-6, 1e-5), "sqrt": (1e-6, 1e-5), "rsqrt": (1e-6, 2e-6)}
EXP_ULP = 2.0   # what the softmax bound grants expf (its measured worst is below 1 ULP; see ULP_MEASURED)


def rng(seed):
    return np.random.default_rng(seed)


def f32(x):
    return np.asarray(x, dtype=np.float32)


def bf16_round(x):
    """fp32 -> bf16 -> fp32, round to nearest even (torch's conversion)."""
    return torch.from_numpy(f32(x)).to(torch.bfloat16).float().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# view programs: how a test operand is derived from its base array -- the same list runs on numpy here and on the device
# ---------------------------------------------------------------------------------------------------------------------
def apply_np(x, prog):
    x = np.asarray(x)
    for op in prog:
        k = op[0]
        if k == "tr": x = x.T
        elif k == "transpose": x = np.swapaxes(x, op[1], op[2])
        elif k == "permute": x = np.transpose(x, op[1])
        elif k == "narrow": x = np.take(x, range(op[2], op[2] + op[3]), axis=op[1])
        elif k == "unsqueeze": x = np.expand_dims(x, op[1])
        elif k == "expand": x = np.broadcast_to(x, op[1])
        elif k == "select": x = np.take(x, op[2], axis=op[1])
        elif k == "bf16": x = bf16_round(x)
        else: raise KeyError(k)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------
def same_specials(got, ref):
    """NaN in the same places, +-inf equal."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool(got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)) and
                np.array_equal(np.where(np.isinf(ref), ref, 0.0), np.where(np.isinf(got), got, 0.0)))


def excess(got, ref, bound):
    """|got - ref| / bound per finite element (0 / 0 = 0): inside the bound iff the maximum is <= 1."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    fin = np.isfinite(ref) & np.isfinite(got)
    err = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0)), 0.0)
    b = np.broadcast_to(bound, err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0.0, 0.0, np.where(b > 0, err / np.where(b > 0, b, 1.0), np.inf))


def inside(got, ref, bound):
    got = np.asarray(got, np.float64)
    if got.shape != np.asarray(ref).shape or not same_specials(got, ref):
        return False
    e = excess(got, ref, bound)
    return bool(e.size == 0 or e.max() <= 1.0)


def broken_fraction(got, ref, bound):
    """Share of the elements a wrong result puts outside the bound (1.0 when the special values already differ)."""
    got = np.asarray(got, np.float64)
    if got.shape != np.asarray(ref).shape or not same_specials(got, ref):
        return 1.0
    e = excess(got, ref, bound)
    return float((e > 1.0).mean()) if e.size else 0.0


def bits_equal(got, ref):
    """Equality for ops that do no arithmetic: same shape, same fp32 bit patterns (so -0 != +0), NaN where NaN."""
    got, ref = f32(got), f32(ref)
    if got.shape != ref.shape:
        return False
    nan = np.isnan(ref)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan]))


def ulp_of(ref):
    """Spacing of fp32 at the float64 reference value (2^-149 in the subnormal range)."""
    a = np.abs(np.asarray(ref, np.float64)).astype(np.float32)
    a = np.where(np.isfinite(a), a, np.float32(0))
    return np.spacing(a).astype(np.float64)


def ulp_error(got, ref):
    """|got - ref| in ULPs of the reference, over the elements whose reference is finite."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref) & np.isfinite(got)
    return np.where(fin, np.abs(np.where(fin, got - ref, 0.0)) / ulp_of(ref), 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# matmul / conv2d
# ---------------------------------------------------------------------------------------------------------------------
# A dot product of K exactly representable pairs, evaluated in fp32 in ANY order with or without fused multiply-adds: every
# product and every addition is rounded once, so (Higham, Accuracy and Stability, 3.1) |fl(s) - s| <= gamma_K sum|a_k b_k| with
# gamma_K = K u / (1 - K u).  (K + 2) u >= gamma_K while K^2 u <= 2, i.e. K <= 5792 -- every K used here -- and K = 0 gives an
# exact zero.  The bound does not depend on tile shape, K step or the order of the chain, so it holds for the MFMA tile
# kernel, for torch's blocked CPU GEMM and for any honest fp32 implementation; it is loose at long K (a worst case over K
# roundings of one sign), where the bit-identity checks of the GPU file are the sharp ones.
def matmul_ref(a, b):
    return np.matmul(np.asarray(a, np.float64), np.asarray(b, np.float64))


def matmul_bound(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    K = a.shape[-1]
    assert K * K * U <= 2.0
    return (K + 2) * U * np.matmul(np.abs(a), np.abs(b))


# conv2d = the same dot product over k = (ci, kh, kw), K = Ci KH KW (padded taps are exact zeros), then ONE addition of the
# bias to the finished sum: fl(s^ + b) = (s^ + b)(1 + d), |d| <= u, so the bias costs u |b| and u |s^| -- the latter is the
# "+ 1" that (K + 2) already holds over gamma_K's first-order K.  (A bias carried as the accumulator's start value would be
# rounded K times at its own size and is NOT covered: the kernel adds it in the epilogue, like ATen.)
def conv2d_ref(x, w, bias, stride, padding, dilation):
    y = F.conv2d(torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(w, np.float64)),
                 None if bias is None else torch.from_numpy(np.asarray(bias, np.float64)), stride, padding, dilation)
    return y.numpy()


def conv2d_bound(x, w, bias, stride, padding, dilation):
    K = int(np.prod(w.shape[1:]))
    cond = conv2d_ref(np.abs(x), np.abs(w), None, stride, padding, dilation)
    b = (K + 2) * U * cond
    return b if bias is None else b + U * np.abs(np.asarray(bias, np.float64))[None, :, None, None]


def im2col(x, w_shape, stride, padding, dilation):
    """[N OH OW, Ci KH KW] fp32 matrix whose product with weight.reshape(Co, -1).T is the convolution (rows (n, oh, ow), k =
    (ci, kh, kw) ascending: the kernel's implicit GEMM, built on the host)."""
    cols = F.unfold(torch.from_numpy(f32(x)), w_shape[2:], dilation, padding, stride)   # [N, Ci KH KW, OH OW]
    return np.ascontiguousarray(cols.permute(0, 2, 1).reshape(-1, cols.shape[1]).numpy())


# ---------------------------------------------------------------------------------------------------------------------
# row reductions
# ---------------------------------------------------------------------------------------------------------------------
def chain(D, per_lane=256):
    """Longest addition chain of a row sum: ceil(D / 256) per thread, 6 shuffle steps, 2 cross-wave additions."""
    return -(-D // per_lane) + 8


# mean: the sum of D values along chains of at most L additions has |error| <= L u sum|x| (each element passes through at most
# L roundings); the division by D adds one more: (L + 1) u mean|x|.
def mean_ref(x, dims, keepdim):
    return np.asarray(x, np.float64).mean(axis=tuple(dims), keepdims=keepdim)


def mean_bound(x, dims, keepdim):
    D = int(np.prod([np.asarray(x).shape[d] for d in dims]))
    return (chain(D) + 1) * U * np.abs(np.asarray(x, np.float64)).mean(axis=tuple(dims), keepdims=keepdim)


# softmax along `dim`: y_i = e_i / s, e_i = exp(x_i - m), m = max (exact: it is one of the x).  t_i = fl(x_i - m) has absolute
# error u |x_i - m|, which exp turns into the same RELATIVE error of e_i; expf adds 2 EXP_ULP u (one ULP is at most 2 u
# relative).  All e_j >= 0, so the relative error of s is the p-weighted mean of the terms' errors, sum_j p_j |x_j - m| u +
# 2 EXP_ULP u, plus L u for its L-long addition chain; the division adds u.  Relative bound of y_i:
#     u ( |x_i - m| + sum_j p_j |x_j - m| + 4 EXP_ULP + L + 1 ),
# plus (2 EXP_ULP + 1) subnormal spacings absolute for results below the normal range.  -inf entries are exact zeros.  A row of
# -inf only is NaN in the reference (x - m = -inf + inf) and must be NaN in the same places.
def softmax_ref(x, dim):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(x - x.max(axis=dim, keepdims=True))
        return e / e.sum(axis=dim, keepdims=True)


def softmax_bound(x, dim):
    x = np.asarray(x, np.float64)
    p = softmax_ref(x, dim)
    with np.errstate(invalid="ignore"):
        t = np.abs(x - x.max(axis=dim, keepdims=True))
    t = np.where(np.isfinite(t), t, 0.0)
    pt = np.where(np.isfinite(p), p, 0.0) * t
    rel = U * (t + pt.sum(axis=dim, keepdims=True) + 4 * EXP_ULP + chain(x.shape[dim]) + 1)
    return rel * np.where(np.isfinite(p), p, 0.0) + (2 * EXP_ULP + 1) * SUB


# layer_norm over the last dimension, two passes: mu^ = fl(mean x), d^_i = fl(x_i - mu^), v^ = fl(mean d^_i^2), r^ = fl(1 /
# sqrt(v^ + eps)), y^_i = fl(fl(fl(d^_i r^) w_i) + b_i).  With L the longest addition chain (one wave per row in the engine's
# kernel: D / 64 per lane; 256 threads per row in the generic one; L = ceil(D / 64) + 8 covers both):
#   dmu = |mu^ - mu| <= (L + 1) u mean|x|                       -- this is the term that grows with the row's offset;
#   |d^_i - d_i| <= dmu + u |d_i|;
#   v^: the common shift of all d^_i enters only as shift^2 (sum d_i = 0), the u |d_i| part as 2 u relative, each square is
#       rounded (u) and the sum has an L-long chain:  |v^ - v| <= (L + 4) u v + dmu^2;  + eps and its rounding: one more u;
#   r^ = r (1 + rho), |rho| <= ((L + 4) u v + dmu^2) / (2 (v + eps)) + 3 u        (half the radicand's error; sqrt, divide);
#   y^_i: |y^_i - y_i| <= r |w_i| (dmu + u |d_i|) + |d_i| r |w_i| (rho + 2 u) + u |y_i|.
# The r |w_i| dmu term is the one that "carries |mean| rstd": rows offset by +100 have mean|x| = 100 and a bound 100x wider
# than centred rows of the same spread, which the +100 cases exercise (a one-pass E[x^2] - mu^2 variance would not fit it).
def layer_norm_ref(x, w, b, eps):
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    y = (x - mu) / np.sqrt(var + eps)
    if w is not None: y = y * np.asarray(w, np.float64)
    if b is not None: y = y + np.asarray(b, np.float64)
    return y


def layer_norm_bound(x, w, b, eps):
    x = np.asarray(x, np.float64)
    D = x.shape[-1]
    L = -(-D // 64) + 8
    mu = x.mean(-1, keepdims=True)
    d = x - mu
    v = (d ** 2).mean(-1, keepdims=True)
    r = 1.0 / np.sqrt(v + eps)
    aw = np.abs(np.asarray(w, np.float64)) if w is not None else 1.0
    dmu = (L + 1) * U * np.abs(x).mean(-1, keepdims=True)
    rho = ((L + 4) * U * v + dmu ** 2) / (2 * (v + eps)) + 3 * U
    y = layer_norm_ref(x, w, b, eps)
    return r * aw * (dmu + U * np.abs(d)) + np.abs(d) * r * aw * (rho + 2 * U) + U * np.abs(y)


def argmax_ref(x, dim):
    """torch's rule: the first NaN if there is one, else the first index of the maximum."""
    x = np.asarray(x, np.float64)
    nan = np.isnan(x)
    return np.where(nan.any(axis=dim), nan.argmax(axis=dim), np.where(nan, -np.inf, x).argmax(axis=dim)).astype(np.int64)


def max_ref(x):
    x = np.asarray(x, np.float32)
    return np.float32(np.nan) if np.isnan(x).any() else x.max()


# ---------------------------------------------------------------------------------------------------------------------
# stft (center = False), reflection pad
# ---------------------------------------------------------------------------------------------------------------------
# X[k, f] = scale sum_t x[f hop + t] w[t] exp(-2 pi i k t / n): per component a dot product of K = n_fft terms, so the matmul
# bound, plus two more roundings per term that the operands bring with them -- the window product fl(x w) (u) and the fp32
# rounding of the cos / sin table entry (u relative; the tables are made in float64 with the angle reduced exactly) -- i.e.
# (n_fft + 4) u sum_t |x w| |cos|.  normalized: scale = fl(1 / fl(sqrt n)) (2 u) and its product (u): + 3.  The float64 table
# itself (here and on the host side of the op) is only good to an ABSOLUTE 2^-50 or so -- the angle 2 pi k t / n is rounded, so
# sin(pi t) comes out as 1e-16 where it is 0 -- hence one more term, 2^-50 sum_t |x w|, that matters only at those zeros.
def stft_ref(x, win, n_fft, hop, normalized, onesided):
    x, win = np.asarray(x, np.float64), np.asarray(win, np.float64)
    n_frames = 1 + (len(x) - n_fft) // hop
    n_freq = n_fft // 2 + 1 if onesided else n_fft
    fr = np.stack([x[f * hop:f * hop + n_fft] * win for f in range(n_frames)], 1)                  # [n_fft, n_frames]
    ang = 2.0 * np.pi * ((np.arange(n_freq)[:, None] * np.arange(n_fft)[None, :]) % n_fft) / n_fft
    sc = 1.0 / math.sqrt(n_fft) if normalized else 1.0
    re, im = np.cos(ang) @ fr * sc, -(np.sin(ang) @ fr) * sc
    bre, bim = np.abs(np.cos(ang)) @ np.abs(fr) * sc, np.abs(np.sin(ang)) @ np.abs(fr) * sc
    k = (n_fft + 4 + (3 if normalized else 0)) * U
    tab = 2.0 ** -50 * np.abs(fr).sum(0, keepdims=True) * sc
    return np.stack([re, im], -1), k * np.stack([bre, bim], -1) + tab[..., None]                                      # [n_freq, n_frames, 2] each


def reflect_pad_ref(x, pl, pr):
    return np.pad(np.asarray(x), [(0, 0)] * (np.ndim(x) - 1) + [(pl, pr)], mode="reflect")


# ---------------------------------------------------------------------------------------------------------------------
# library functions
# ---------------------------------------------------------------------------------------------------------------------
_ERF = np.vectorize(math.erf, otypes=[np.float64])
UNARY_REF = {
    "exp": lambda x: np.exp(x), "sin": lambda x: np.sin(x), "cos": lambda x: np.cos(x), "log10": lambda x: np.log10(x),
    "sqrt": lambda x: np.sqrt(x), "rsqrt": lambda x: 1.0 / np.sqrt(x), "gelu": lambda x: 0.5 * x * (1.0 + _ERF(x / math.sqrt(2.0))),
    "silu": lambda x: x / (1.0 + np.exp(-x)), "pow": lambda x: np.power(x, POW_E),
}
POW_E = 1.5
UNARY_TORCH = {
    "exp": torch.exp, "sin": torch.sin, "cos": torch.cos, "log10": torch.log10, "sqrt": torch.sqrt, "rsqrt": lambda t: t.sqrt().reciprocal(),
    "gelu": F.gelu, "silu": F.silu, "pow": lambda t: t.pow(POW_E),
}


def unary_ref(name, x):
    with np.errstate(all="ignore"):
        return UNARY_REF[name](np.asarray(x, np.float64))


def unary_sweep(name):
    """fp32 inputs of the ULP sweep: a dense grid of |x| <= 4 (where the legacy atol / rtol caps the gate) and a coarse one
    over the range in which the fp32 result stays normal.  GELU and SiLU leave the negative tail beyond -4 out: 1 + erf(x)
    and 1 + exp(-x) cancel there, the fp32 formula of the reference's own arm has no significant bits left, and a ULP count
    of it measures the formula, not the kernel (the special-value test pins those results to torch's)."""
    g = rng(11)
    dense = np.concatenate([np.linspace(-4.0, 4.0, 16385), g.uniform(-4.0, 4.0, 16384)])
    pos = np.concatenate([np.linspace(2.0 ** -10, 4.0, 16385), g.uniform(0.0, 4.0, 16384) + 1e-6])
    wide = {
        "exp": np.linspace(-87.0, 88.0, 4097), "sin": np.linspace(-100.0, 100.0, 8193), "cos": np.linspace(-100.0, 100.0, 8193),
        "log10": np.logspace(-37, 38, 4097), "sqrt": np.logspace(-37, 38, 4097), "rsqrt": np.logspace(-37, 38, 4097),
        "pow": np.logspace(-20, 20, 4097), "gelu": np.linspace(4.0, 30.0, 2049), "silu": np.linspace(4.0, 60.0, 2049),
    }[name]
    base = pos if name in ("log10", "sqrt", "rsqrt", "pow") else dense
    return f32(np.concatenate([base, wide]))


def gate_domain(name, x):
    """Where the ULP count of a function is measured and gated.  Everything, except GELU below -1: 1 + erf(x / sqrt 2) cancels
    there, the absolute error of erf (a few u in any fp32 erf) is all that is left of the result, and the ULP count measures
    the formula of the reference's own arm, not the kernel -- 4 084 ULP on the MI355X and 58 715 ULP in torch's CPU kernel at
    x = -3.9, both inside the 2e-6 the existing test allows.  That stretch keeps the existing atol / rtol alone."""
    x = np.asarray(x, np.float64)
    return x >= -1.0 if name == "gelu" else np.ones(x.shape, bool)


def unary_bound(name, x, ref, gate=None):
    """gate ULPs of the reference; where |x| <= 4 never more than the legacy atol + rtol |ref| (and only that outside
    gate_domain)."""
    gate = ULP_GATE[name] if gate is None else gate
    x = np.asarray(x, np.float64)
    atol, rtol = LEGACY_TOL[name]
    legacy = atol + rtol * np.abs(ref)
    b = np.where(gate_domain(name, x), gate * ulp_of(ref), legacy)
    return np.where(np.abs(x) <= 4.0, np.minimum(b, legacy), b)


def special_pattern_equal(got, want):
    """The NaN / +-inf / signed-zero pattern of two fp32 results is the same."""
    got, want = f32(got), f32(want)
    sp = lambda a: (np.isnan(a), np.where(np.isinf(a), a, 0), (a == 0) & np.signbit(a), (a == 0) & ~np.signbit(a))
    return got.shape == want.shape and all(np.array_equal(p, q) for p, q in zip(sp(got), sp(want)))


# ---------------------------------------------------------------------------------------------------------------------
# the cases.  Each is a dict: family, name, the inputs, and `mutants`: the names (keys of MUTANTS) of the mistakes this case
# must catch.  expected(case) -> (ref, bound); bound None = equality.  honest(case) -> torch's float32 CPU result.
# ---------------------------------------------------------------------------------------------------------------------
MATMUL_MNK = [(1, 1, 1), (63, 65, 31), (64, 64, 32), (65, 63, 33), (129, 130, 70), (130, 70, 4321), (5, 3, 0)]


def matmul_cases():
    out = []
    g = rng(1)
    r = lambda *s: f32(g.standard_normal(s))
    for M, N, K in MATMUL_MNK:
        muts = (["k0_unwritten"] if K == 0 else ["drop_last_k"]) + (["skip_k_tail"] if K % 32 and K > 32 else [])
        out.append(dict(family="matmul", name=f"{M}x{N}x{K}", a=r(M, K), pa=[], b=r(K, N), pb=[], mutants=muts))
    for M, N, K in [(65, 63, 33), (129, 130, 70)]:   # b = weight.tr(): the in-place [N][K] reader
        out.append(dict(family="matmul", name=f"tr_{M}x{N}x{K}", a=r(M, K), pa=[], b=r(N, K), pb=[("tr",)],
                        mutants=["drop_last_k", "skip_k_tail", "tb_transposed"]))
    K, N, M = 70, 45, 37
    T = ["drop_last_k", "skip_k_tail"]
    out += [
        dict(family="matmul", name="vec_mat", a=r(K), pa=[], b=r(K, N), pb=[], mutants=T),
        dict(family="matmul", name="mat_vec", a=r(M, K), pa=[], b=r(K), pb=[], mutants=T),
        dict(family="matmul", name="vec_vec", a=r(K), pa=[], b=r(K), pb=[], mutants=T),
        dict(family="matmul", name="a2d_b_batched", a=r(M, K), pa=[], b=r(3, K, N), pb=[], mutants=T + ["batch_zero_only"]),
        dict(family="matmul", name="partial_broadcast", a=r(2, 1, M, K), pa=[], b=r(1, 3, K, N), pb=[], mutants=T + ["batch_zero_only"]),
        dict(family="matmul", name="a_bf16", a=r(M, K), pa=[("bf16",)], b=r(K, N), pb=[], mutants=T + ["bf16_truncate_a"]),
        dict(family="matmul", name="a_permuted", a=r(K, 2, M), pa=[("permute", (1, 2, 0))], b=r(2, N, K), pb=[("transpose", 1, 2)],
             mutants=T + ["batch_zero_only"]),
        dict(family="matmul", name="batch_70000", a=r(70000, 1, 2), pa=[], b=r(70000, 2, 3), pb=[], mutants=["drop_last_k", "batch_beyond_grid"]),
    ]
    return out


def conv_cases():
    g = rng(2)
    r = lambda *s: f32(g.standard_normal(s))
    spec = [  # name, x shape, w shape, stride, padding, dilation, bias
        ("stem_480", (1, 480, 8, 8), (480, 480, 3, 3), (2, 2), (1, 1), (1, 1), True),      # K = 4320, 8 column tiles
        ("co1_k27", (3, 3, 9, 9), (1, 3, 3, 3), (1, 1), (1, 1), (1, 1), True),             # 3 images of 81 rows: a tile crosses images
        ("co65_k32", (3, 8, 9, 10), (65, 8, 2, 2), (1, 1), (0, 0), (1, 1), False),         # 72 rows per image
        ("co130_k63", (3, 7, 9, 9), (130, 7, 3, 3), (1, 1), (1, 1), (1, 1), True),
        ("k1x3_s1x2", (2, 5, 7, 11), (6, 5, 1, 3), (1, 2), (0, 0), (1, 1), False),
        ("k3x1_p0x2", (2, 5, 7, 11), (6, 5, 3, 1), (1, 1), (0, 2), (1, 1), True),
        ("k2x4_d2x1", (2, 5, 9, 11), (6, 5, 2, 4), (1, 1), (0, 0), (2, 1), False),
    ]
    out = []
    for name, xs, ws, st, pd, dl, bias in spec:
        K = ws[1] * ws[2] * ws[3]
        muts = ["drop_last_k"] + (["skip_k_tail"] if K % 32 and K > 32 else []) + (["bias_dropped"] if bias else [])
        if xs[0] > 1: muts.append("image_zero_only")
        out.append(dict(family="conv2d", name=name, x=r(*xs), w=r(*ws) / math.sqrt(K), bias=r(ws[0]) if bias else None, stride=st, padding=pd,
                        dilation=dl, mutants=muts))
    return out


ROW_D = [1, 63, 64, 65, 255, 256, 257, 1000, 4097]
ROW_R = [1, 3]


def _row_mutants(D, rows, softmax=False):
    m = []
    if D > 256 and D % 256: m.append("drop_row_tail")
    if D > 64: m.append("drop_wave")
    if D >= 2: m.append("drop_last_element")
    if rows > 1 and not (softmax and D == 1): m.append("row_zero_only")   # (softmax of one element is 1 in every row)
    return m or ["unwritten"]


def softmax_cases():
    g = rng(3)
    out = []
    for D in ROW_D:
        for rows in ROW_R:
            out.append(dict(family="softmax", name=f"{rows}x{D}", x=f32(3.0 * g.standard_normal((rows, D))), px=[], dim=-1, mutants=_row_mutants(D, rows, True)))
    base = f32(2.0 * g.standard_normal((70, 300)))
    view = [("tr",), ("narrow", 0, 3, 257), ("narrow", 1, 1, 65)]          # [257, 65] view of a [70, 300] array
    out.append(dict(family="softmax", name="dim0_of_view", x=base, px=view, dim=0, mutants=["drop_row_tail", "drop_wave", "wrong_dim"]))
    out.append(dict(family="softmax", name="dim1_of_view", x=base, px=view, dim=1, mutants=["drop_wave", "drop_last_element", "wrong_dim"]))
    m = f32(g.standard_normal((3, 300)))
    m[0, 100:] = -np.inf; m[1, ::2] = -np.inf; m[2, :299] = -np.inf        # masked attention rows (row 2: one key left)
    out.append(dict(family="softmax", name="masked", x=m, px=[], dim=-1, mutants=["drop_wave", "row_zero_only"]))
    a = f32(g.standard_normal((3, 300)))
    a[1, :] = -np.inf                                                       # NaN row in the reference
    out.append(dict(family="softmax", name="all_masked_row", x=a, px=[], dim=-1, mutants=["nan_row_as_zero", "row_zero_only"]))
    big = f32(np.where(g.random((3, 300)) < 0.5, 1e4, -1e4) + g.standard_normal((3, 300)))
    out.append(dict(family="softmax", name="pm1e4", x=big, px=[], dim=-1, mutants=["drop_wave", "no_max_subtraction"]))
    return out


def mean_cases():
    g = rng(4)
    out = []
    for D in ROW_D:
        for rows in ROW_R:
            out.append(dict(family="mean", name=f"{rows}x{D}", x=f32(g.standard_normal((rows, D)) + 0.5), px=[], dims=(-1,), keepdim=False,
                            mutants=_row_mutants(D, rows)))
    x3 = f32(g.standard_normal((4, 70, 33)) + 0.5)
    for name, px, dims, keep, muts in [
        ("dim1_3d", [], (1,), False, ["drop_wave", "drop_last_element", "wrong_dim"]),
        ("dim1_3d_keep", [], (1,), True, ["drop_wave", "drop_last_element", "wrong_dim"]),
        ("dims02", [], (0, 2), False, ["drop_wave", "drop_last_element", "wrong_dim"]),
        ("dims02_keep", [], (0, 2), True, ["drop_wave", "drop_last_element", "wrong_dim"]),
        ("all_dims", [], (0, 1, 2), False, ["drop_row_tail", "drop_wave", "drop_last_element"]),
        ("all_dims_keep", [], (0, 1, 2), True, ["drop_row_tail", "drop_wave", "drop_last_element"]),
        ("noncontig", [("transpose", 0, 2), ("narrow", 1, 2, 65)], (-2,), False, ["drop_wave", "drop_last_element", "wrong_dim"]),
    ]:
        out.append(dict(family="mean", name=name, x=x3, px=px, dims=dims, keepdim=keep, mutants=muts))
    return out


LN_D = [4, 252, 256, 260, 2044, 2048, 2050, 2052, 4096]
LN_R = [1, 5, 9]
LN_EPS = 1e-5


def layer_norm_cases():
    g = rng(5)
    out = []
    for D in LN_D:
        w, b = f32(1.0 + 0.3 * g.standard_normal(D)), f32(0.5 * g.standard_normal(D))
        for rows in LN_R:
            x = f32(g.standard_normal((rows, D)) * 1.5 + 0.3)
            for mode in ("both", "weight", "bias", "neither"):
                muts = ["var_unbiased", "drop_last_element"] + (["row_zero_only"] if rows > 1 else []) + (["drop_wave"] if D > 64 else [])
                if mode in ("both", "weight"): muts.append("weight_dropped")
                if mode in ("both", "bias"): muts.append("bias_dropped")
                out.append(dict(family="layer_norm", name=f"{rows}x{D}_{mode}", x=x, w=w if mode in ("both", "weight") else None,
                                b=b if mode in ("both", "bias") else None, mutants=muts))
    for D in (256, 2048, 2052):   # rows offset by +100: the bound's |mean| rstd term
        w, b = f32(1.0 + 0.3 * g.standard_normal(D)), f32(0.5 * g.standard_normal(D))
        x = f32(g.standard_normal((5, D)) + 100.0)
        for mode in ("both", "neither"):
            out.append(dict(family="layer_norm", name=f"5x{D}_{mode}_offset100", x=x, w=w if mode == "both" else None, b=b if mode == "both" else None,
                            mutants=["var_unbiased", "drop_wave", "one_pass_variance"]))
    return out


ARG_D = [1, 63, 64, 65, 255, 256, 257, 1000, 4097]


def argmax_cases():
    """Rows of small distinct integers-plus-noise values with the structure under test planted; every row of a case is its own
    sub-case, so one launch covers them.  Exact: the index (and the value for `max`) must be equal."""
    g = rng(6)
    out = []
    for D in ARG_D:
        rows, tags = [], []

        def base():
            return f32(g.uniform(-1.0, 1.0, D))

        for pos in sorted({p for p in (0, 63, 64, 255, 256, D - 1) if p < D}):
            x = base(); x[pos] = 5.0
            rows.append(x); tags.append(f"max@{pos}")
        for d in (1, 64, 256):
            for i in sorted({0, 3, D - 1 - d}):
                if 0 <= i and i + d < D:
                    x = base(); x[i] = 5.0; x[i + d] = 5.0
                    rows.append(x); tags.append(f"tie@{i},{i + d}")
        rows.append(np.full(D, 0.25, np.float32)); tags.append("all_equal")
        rows.append(np.full(D, -np.inf, np.float32)); tags.append("all_-inf")
        for pos in sorted({p for p in (0, 1, 64, 300, D - 1) if p < D}):
            x = base(); x[pos] = np.nan
            if pos + 70 < D: x[pos + 70] = np.nan          # a later NaN, in another wave: the FIRST one is the answer
            if pos > 0: x[0] = 9.0                          # and an ordinary maximum before it that must not win
            rows.append(x); tags.append(f"nan@{pos}")
        muts = ["unwritten"] if D == 1 else ["last_on_ties", "nan_ignored"]
        if D > 64: muts += ["merge_ge", "drop_wave"]
        out.append(dict(family="argmax", name=f"D{D}", x=np.stack(rows), tags=tags, dim=-1, keepdim=False, mutants=muts))
    lg = f32(g.standard_normal((2, 151936)))
    lg[0, 151935] = 9.0; lg[1, 77777] = 9.0; lg[1, 151000] = 9.0
    out.append(dict(family="argmax", name="logits_151936", x=lg, tags=["last", "tie"], dim=-1, keepdim=False, mutants=["last_on_ties", "drop_row_tail"]))
    x3 = f32(g.integers(0, 4, (5, 300, 7)))                 # many ties along a non-last dim
    out.append(dict(family="argmax", name="dim1_keepdim", x=x3, tags=[], dim=1, keepdim=True, mutants=["last_on_ties", "wrong_dim"]))
    out.append(dict(family="argmax", name="dim0", x=x3, tags=[], dim=0, keepdim=False, mutants=["last_on_ties", "wrong_dim"]))
    return out


def stft_cases():
    g = rng(7)
    out = []
    for n_fft, hop, L, norm, onesided in [
        (16, 1, 16 + 37, False, True), (16, 16, 16, True, False), (16, 160, 16 + 400, False, False),
        (400, 160, 400 + 3 * 160 + 77, False, True), (400, 1, 400 + 5, True, True), (400, 400, 400, False, False), (400, 400, 3 * 400 + 123, True, True),
        (512, 160, 512 + 2 * 160 + 5, False, True), (512, 512, 512, True, True), (512, 1, 512 + 3, False, False),
    ]:
        # Hamming, not Hann: a window that vanishes at its ends hides the first and last tap of the frame from any bound
        win = f32(0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft))
        muts = ["drop_last_k", "conjugate"] + (["scale_dropped"] if norm else []) + (["freq_wrap_dropped"] if (n_fft // 2 + 1 if onesided else n_fft) > 256 else [])
        if (L - n_fft) // hop >= 1: muts.append("hop_as_n_fft" if hop != n_fft else "hop_off_by_one")
        out.append(dict(family="stft", name=f"n{n_fft}_h{hop}_L{L}_{'norm' if norm else 'raw'}_{'one' if onesided else 'two'}", x=f32(g.standard_normal(L)),
                        win=win, n_fft=n_fft, hop=hop, normalized=norm, onesided=onesided, mutants=muts))
    return out


def reflect_pad_cases():
    g = rng(8)
    n = 37
    out = []
    for name, shape, pad in [("full", (n,), (n - 1, n - 1)), ("none", (n,), (0, 0)), ("right5", (n,), (0, 5)), ("rows_2x3", (2, 3, n), (4, 7)),
                             ("mel_pad", (1, 1, 1000), (200, 200))]:
        muts = ["unwritten"] if pad == (0, 0) else ["mirror_right_off_by_one"] + (["mirror_left_repeats_edge"] if pad[0] else [])
        out.append(dict(family="reflect_pad", name=name, x=f32(g.standard_normal(shape)), pad=pad, mutants=muts))
    return out


FAMILIES = {"matmul": matmul_cases, "conv2d": conv_cases, "softmax": softmax_cases, "mean": mean_cases, "layer_norm": layer_norm_cases,
            "argmax": argmax_cases, "stft": stft_cases, "reflect_pad": reflect_pad_cases}


def operands(c):
    """The logical (viewed / converted) operands of a case, as numpy arrays."""
    f = c["family"]
    if f == "matmul": return apply_np(c["a"], c["pa"]), apply_np(c["b"], c["pb"])
    if f in ("softmax", "mean"): return (apply_np(c["x"], c["px"]),)
    return (c["x"],)


def expected(c):
    """(float64 reference, per-element bound or None for equality)."""
    f = c["family"]
    if f == "matmul":
        a, b = operands(c)
        return matmul_ref(a, b), matmul_bound(a, b)
    if f == "conv2d":
        args = (c["x"], c["w"], c["bias"], c["stride"], c["padding"], c["dilation"])
        return conv2d_ref(*args), conv2d_bound(*args)
    if f == "softmax":
        (x,) = operands(c)
        return softmax_ref(x, c["dim"]), softmax_bound(x, c["dim"])
    if f == "mean":
        (x,) = operands(c)
        dims = tuple(d % x.ndim for d in c["dims"])
        return mean_ref(x, dims, c["keepdim"]), mean_bound(x, dims, c["keepdim"])
    if f == "layer_norm":
        return layer_norm_ref(c["x"], c["w"], c["b"], LN_EPS), layer_norm_bound(c["x"], c["w"], c["b"], LN_EPS)
    if f == "argmax":
        r = argmax_ref(c["x"], c["dim"])
        return (np.expand_dims(r, c["dim"]) if c["keepdim"] else r), None
    if f == "stft":
        return stft_ref(c["x"], c["win"], c["n_fft"], c["hop"], c["normalized"], c["onesided"])
    if f == "reflect_pad":
        return reflect_pad_ref(c["x"], *c["pad"]), None
    raise KeyError(f)


def honest(c):
    """torch's own float32 CPU op on the same operands."""
    f = c["family"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(f32(a)))
    if f == "matmul":
        a, b = operands(c)
        return torch.matmul(t(a), t(b)).numpy()
    if f == "conv2d":
        return F.conv2d(t(c["x"]), t(c["w"]), None if c["bias"] is None else t(c["bias"]), c["stride"], c["padding"], c["dilation"]).numpy()
    if f == "softmax":
        return torch.softmax(t(operands(c)[0]), c["dim"]).numpy()
    if f == "mean":
        return t(operands(c)[0]).mean(c["dims"], keepdim=c["keepdim"]).numpy()
    if f == "layer_norm":
        D = c["x"].shape[-1]
        return F.layer_norm(t(c["x"]), (D,), None if c["w"] is None else t(c["w"]), None if c["b"] is None else t(c["b"]), LN_EPS).numpy()
    if f == "argmax":
        return t(c["x"]).argmax(c["dim"], keepdim=c["keepdim"]).numpy()
    if f == "stft":
        s = torch.stft(t(c["x"]), c["n_fft"], c["hop"], c["n_fft"], t(c["win"]), center=False, normalized=c["normalized"], onesided=c["onesided"],
                       return_complex=True)
        return torch.view_as_real(s).numpy()
    if f == "reflect_pad":
        x = t(c["x"])
        return F.pad(x.reshape(1, -1, x.shape[-1]), c["pad"], mode="reflect").reshape(*x.shape[:-1], -1).numpy()
    raise KeyError(f)


def accepts(c, got, exp=None):
    ref, bound = exp if exp is not None else expected(c)
    if bound is None:
        got = np.asarray(got)
        return bool(got.shape == ref.shape and np.array_equal(got, ref)) if ref.dtype == np.int64 else bits_equal(got, ref)
    return inside(got, ref, bound)


# ---------------------------------------------------------------------------------------------------------------------
# mutants: what a kernel with one plausible mistake computes (float64 on the case's operands; name -> function(case))
# ---------------------------------------------------------------------------------------------------------------------
def _row_view(c):
    """The case's operand with the reduced dimension(s) last, flattened to [rows, D], and a function that puts a [rows] or
    [rows, D] result back into the op's output shape."""
    f = c["family"]
    (x,) = operands(c)
    x = np.asarray(x, np.float64)
    if f == "mean":
        dims = tuple(d % x.ndim for d in c["dims"])
        keep = [d for d in range(x.ndim) if d not in dims]
        xr = np.transpose(x, keep + list(dims))
        oshape = [1 if d in dims else x.shape[d] for d in range(x.ndim)] if c["keepdim"] else [x.shape[d] for d in keep]
        return xr.reshape(int(np.prod([x.shape[d] for d in keep], dtype=np.int64)), -1), lambda y: y.reshape(oshape)
    if f == "layer_norm":
        return x.reshape(-1, x.shape[-1]), lambda y: y.reshape(x.shape)
    d = c["dim"] % x.ndim
    xr = np.moveaxis(x, d, -1)
    if f == "softmax":
        return xr.reshape(-1, x.shape[d]), lambda y: np.moveaxis(y.reshape(xr.shape), -1, d)
    oshape = expected(c)[0].shape                                                   # argmax
    return xr.reshape(-1, x.shape[d]), lambda y: y.reshape(oshape)


def _row_op(c, xr, keepmask=None):
    """The family's row op in float64 over [rows, D]; keepmask [D] marks the elements the (mutated) kernel visits."""
    f = c["family"]
    D = xr.shape[1]
    km = np.ones(D, bool) if keepmask is None else keepmask
    if f == "mean":
        return np.where(km, xr, 0.0).sum(1) / D
    if f == "softmax":
        with np.errstate(invalid="ignore"):
            m = np.where(km, xr, -np.inf).max(1, keepdims=True)
            e = np.exp(xr - m)
            return np.where(km, e / np.where(km, e, 0.0).sum(1, keepdims=True), 0.0)
    if f == "layer_norm":
        mu = np.where(km, xr, 0.0).sum(1, keepdims=True) / D
        var = np.where(km, (xr - mu) ** 2, 0.0).sum(1, keepdims=True) / D
        y = np.where(km, (xr - mu) / np.sqrt(var + LN_EPS), 0.0)
        if c["w"] is not None: y = y * c["w"]
        if c["b"] is not None: y = np.where(km, y + c["b"], 0.0)
        return y
    if f == "argmax":
        return argmax_ref(np.where(km, xr, -np.inf), 1)
    raise KeyError(f)


def _masked(mask_of_D):
    def mut(c):
        xr, back = _row_view(c)
        return back(_row_op(c, xr, mask_of_D(xr.shape[1])))
    return mut


def _last_wave(D):
    idx = np.arange(D)
    return (idx % 256) // 64 != min(3, (D - 1) // 64)


def _row_zero_only(c):
    xr, back = _row_view(c)
    y = _row_op(c, xr)
    return back(np.broadcast_to(y[:1], y.shape).copy())


def _wrong_dim(c):
    c2 = dict(c)
    if c["family"] == "mean":
        x = operands(c)[0]
        c2["dims"] = tuple((d % x.ndim + 1) % x.ndim for d in c["dims"])
        r = expected(c2)[0]
        want = expected(c)[0].shape
        return r.reshape(want) if r.size == int(np.prod(want)) else np.zeros(want)
    nd = operands(c)[0].ndim
    c2["dim"] = (c["dim"] % nd + 1) % nd
    r = expected(c2)[0]
    want = expected(c)[0].shape
    return r if r.shape == want else (np.resize(r, want))


def _mm(c):
    a, b = operands(c)
    return np.asarray(a, np.float64), np.asarray(b, np.float64)


def _mm_drop_last_k(c):
    if c["family"] == "stft":
        x = c["x"].copy()
        ref = stft_ref(x, np.where(np.arange(c["n_fft"]) == c["n_fft"] - 1, 0.0, 1.0) * c["win"].astype(np.float64) +
                       0.0, c["n_fft"], c["hop"], c["normalized"], c["onesided"])[0]
        return ref
    if c["family"] == "conv2d":
        w = np.asarray(c["w"], np.float64).copy()
        w[:, -1, -1, -1] = 0.0
        return conv2d_ref(c["x"], w, c["bias"], c["stride"], c["padding"], c["dilation"])
    a, b = _mm(c)
    return matmul_ref(a[..., :-1], b[..., :-1, :] if b.ndim > 1 else b[:-1])


def _mm_skip_k_tail(c):
    if c["family"] == "conv2d":
        w = np.asarray(c["w"], np.float64).copy()
        K = int(np.prod(w.shape[1:]))
        w.reshape(w.shape[0], -1)[:, K // 32 * 32:] = 0.0
        return conv2d_ref(c["x"], w, c["bias"], c["stride"], c["padding"], c["dilation"])
    a, b = _mm(c)
    K = a.shape[-1] // 32 * 32
    return matmul_ref(a[..., :K], b[..., :K, :] if b.ndim > 1 else b[:K])


def _mm_tb_transposed(c):     # the [N][K] weight read as if it were [K][N]
    a, _ = _mm(c)
    return matmul_ref(a, np.asarray(c["b"], np.float64).reshape(c["b"].shape[1], c["b"].shape[0]))


def _mm_batch_zero_only(c):   # every batch computes batch 0's product (a batch stride of 0 where one is due)
    r = matmul_ref(*_mm(c))
    flat = r.reshape(-1, *r.shape[-2:])
    return np.broadcast_to(flat[:1], flat.shape).reshape(r.shape).copy()


def _mm_batch_beyond_grid(c):  # the launch covers gridDim.z <= 65535 batches; the rest of the output stays unwritten
    r = matmul_ref(*_mm(c))
    r[65535:] = 0.0
    return r


def _bf16_truncate(x):
    return (f32(x).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _mm_bf16_truncate_a(c):
    return matmul_ref(_bf16_truncate(c["a"]), apply_np(c["b"], c["pb"]))


def _conv_bias_dropped(c):
    if c["family"] == "layer_norm":
        return layer_norm_ref(c["x"], c["w"], None, LN_EPS)
    return conv2d_ref(c["x"], c["w"], None, c["stride"], c["padding"], c["dilation"])


def _conv_image_zero_only(c):  # n = m / (OH OW) lost: every image convolves image 0
    x = np.broadcast_to(c["x"][:1], c["x"].shape)
    return conv2d_ref(x, c["w"], c["bias"], c["stride"], c["padding"], c["dilation"])


def _ln_var_unbiased(c):
    x = np.asarray(c["x"], np.float64)
    D = x.shape[-1]
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).sum(-1, keepdims=True) / max(D - 1, 1) * (1.0 if D > 1 else 0.0)
    y = (x - mu) / np.sqrt(var + LN_EPS)
    if D == 1: y = y + 1.0     # (nothing to normalise: make the D - 1 = 0 division visible)
    if c["w"] is not None: y = y * c["w"]
    if c["b"] is not None: y = y + c["b"]
    return y


def _ln_one_pass(c):           # var = E[x^2] - mean^2 evaluated in fp32: cancels at an offset of 100
    x = torch.from_numpy(f32(c["x"]))
    mu = x.mean(-1, keepdim=True)
    var = ((x * x).mean(-1, keepdim=True) - mu * mu).clamp_min(0.0)
    y = ((x - mu) / torch.sqrt(var + LN_EPS)).double().numpy()
    if c["w"] is not None: y = y * c["w"]
    if c["b"] is not None: y = y + c["b"]
    return y


def _argmax_last_on_ties(c):
    xr, back = _row_view(c)
    nan = np.isnan(xr)
    D = xr.shape[1]
    last = lambda m: D - 1 - m[:, ::-1].argmax(1)
    return back(np.where(nan.any(1), last(nan), last(np.where(nan, -np.inf, xr) == np.where(nan, -np.inf, xr).max(1, keepdims=True))).astype(np.int64))


def _argmax_partials(xr):
    """Per-wave (value, index) partials of the 256-thread row scan under the correct rule: [rows, 4] each."""
    rows, D = xr.shape
    vals, idxs = np.full((rows, 4), -np.inf), np.full((rows, 4), 2 ** 31 - 1, np.int64)
    for w in range(4):
        km = (np.arange(D) % 256) // 64 == w
        if km.any():
            sub = np.where(km, xr, -np.inf)
            i = argmax_ref(sub, 1)
            vals[:, w], idxs[:, w] = xr[np.arange(rows), i], i
    return vals, idxs


def _argmax_merge_ge(c):       # cross-wave merge with >= : a later wave's equal value replaces the earlier one
    xr, back = _row_view(c)
    vals, idxs = _argmax_partials(xr)
    best, bi = vals[:, 0].copy(), idxs[:, 0].copy()
    for w in range(1, 4):
        nb, nv = np.isnan(best), np.isnan(vals[:, w])
        take = np.where(nb | nv, nv, vals[:, w] >= best) & (idxs[:, w] < 2 ** 31 - 1)
        best, bi = np.where(take, vals[:, w], best), np.where(take, idxs[:, w], bi)
    return back(bi.astype(np.int64))


def _argmax_nan_ignored(c):    # `v > best` alone: a NaN never wins unless it is the first element a thread visits
    xr, back = _row_view(c)
    return back(np.where(np.isnan(xr), -np.inf, xr).argmax(1).astype(np.int64))


def _softmax_nan_row_as_zero(c):
    r = expected(c)[0]
    return np.where(np.isnan(r), 0.0, r)


def _softmax_no_max(c):        # exp(x) / sum exp(x) in fp32: overflows at 1e4
    (x,) = operands(c)
    with np.errstate(all="ignore"):
        e = np.exp(f32(x)).astype(np.float32)
        return (e / e.sum(c["dim"], keepdims=True)).astype(np.float64)


def _stft_variant(**kw):
    def mut(c):
        a = dict(x=c["x"], win=c["win"], n_fft=c["n_fft"], hop=c["hop"], normalized=c["normalized"], onesided=c["onesided"])
        want = stft_ref(**a)[0]
        if "hop" in kw:
            a["hop"] = kw["hop"](c)
        if "normalized" in kw:
            a["normalized"] = kw["normalized"]
        r = stft_ref(**a)[0]
        if kw.get("conj"):
            r = r * np.array([1.0, -1.0])
        if kw.get("wrap"):
            r[256:] = 0.0
        if r.shape != want.shape:   # the same frames count, read from the wrong offsets
            n = want.shape[1]
            r = np.concatenate([r, np.zeros_like(want)], 1)[:, :n]
        return r
    return mut


def _pad_mirror_right(c):      # src = 2 n - 1 - src at the right edge: repeats the last sample
    x, (pl, pr) = np.asarray(c["x"]), c["pad"]
    n = x.shape[-1]
    j = np.arange(n + pl + pr) - pl
    j = np.where(j < 0, -j, j)
    j = np.where(j >= n, 2 * n - 1 - j, j)
    return x[..., j]


def _pad_mirror_left(c):       # src = -src - 1 at the left edge
    x, (pl, pr) = np.asarray(c["x"]), c["pad"]
    n = x.shape[-1]
    j = np.arange(n + pl + pr) - pl
    j = np.where(j < 0, -j - 1, j)
    j = np.where(j >= n, 2 * (n - 1) - j, j)
    return x[..., j]


def _unwritten(c):
    r = expected(c)[0]
    return np.full(r.shape, 1 if r.dtype == np.int64 else 0.5, r.dtype)


def _weight_dropped(c):
    return layer_norm_ref(c["x"], None, c["b"], LN_EPS)


MUTANTS = {
    "drop_last_k": _mm_drop_last_k, "skip_k_tail": _mm_skip_k_tail, "tb_transposed": _mm_tb_transposed, "k0_unwritten": _unwritten,
    "batch_zero_only": _mm_batch_zero_only, "batch_beyond_grid": _mm_batch_beyond_grid, "bf16_truncate_a": _mm_bf16_truncate_a,
    "bias_dropped": _conv_bias_dropped, "image_zero_only": _conv_image_zero_only, "weight_dropped": _weight_dropped,
    "drop_row_tail": _masked(lambda D: np.arange(D) < D // 256 * 256), "drop_wave": _masked(_last_wave),
    "drop_last_element": _masked(lambda D: np.arange(D) < D - 1), "row_zero_only": _row_zero_only, "wrong_dim": _wrong_dim,
    "unwritten": _unwritten, "var_unbiased": _ln_var_unbiased, "one_pass_variance": _ln_one_pass,
    "last_on_ties": _argmax_last_on_ties, "merge_ge": _argmax_merge_ge, "nan_ignored": _argmax_nan_ignored,
    "nan_row_as_zero": _softmax_nan_row_as_zero, "no_max_subtraction": _softmax_no_max,
    "scale_dropped": _stft_variant(normalized=False), "conjugate": _stft_variant(conj=True), "freq_wrap_dropped": _stft_variant(wrap=True),
    "hop_as_n_fft": _stft_variant(hop=lambda c: c["n_fft"]), "hop_off_by_one": _stft_variant(hop=lambda c: c["hop"] - 1),
    "mirror_right_off_by_one": _pad_mirror_right, "mirror_left_repeats_edge": _pad_mirror_left,
}


# ---------------------------------------------------------------------------------------------------------------------
# conversions at special values (equal to torch's) and their mutant: truncation instead of round-to-nearest-even
# ---------------------------------------------------------------------------------------------------------------------
def conversion_inputs():
    """fp32 values around the rounding ties and limits of bf16 / f16, signed zeros, infinities, NaN and subnormals."""
    bits = np.array([0x3F800000, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F80FFFF, 0x7F7FFFFF, 0x7F7F8000, 0x00000001, 0x00008000,
                     0x00018000, 0x007FFFFF, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x7FC00000], np.uint32).view(np.float32)
    vals = np.array([65504.0, 65519.996, 65520.0, 65536.0, -65520.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 2.0 ** -24,
                     2.0 ** -25, 1.5 * 2.0 ** -24, 2.0 ** -25 * 1.0001, 6.0e-8, -0.75, -1.5, -2.5, 2.5, 0.999, -0.999, 1e-30, 3.0e9, -3.0e9, 1.0e18],
                    np.float32)
    return np.concatenate([bits, vals])


def convert_ref(x, dtype):
    """torch's conversion of fp32 `x` to the dtype code, read back as the array the device test can fetch (fp32 for the float
    types and bool, int64 for the integers).  Integer conversion of non-finite or out-of-range values is undefined in C++ and
    in torch: those inputs are left out by `convertible`."""
    t = torch.from_numpy(f32(x))
    if dtype == BF16: return t.to(torch.bfloat16).float().numpy()
    if dtype == F16: return t.to(torch.float16).float().numpy()
    if dtype == I64: return t.to(torch.int64).numpy()
    if dtype == I32: return t.to(torch.int32).to(torch.int64).numpy()
    if dtype == BOOL: return t.to(torch.bool).float().numpy()
    raise KeyError(dtype)


def convertible(x, dtype):
    x = f32(x)
    lim = {I64: 9.0e18, I32: 2.0e9}.get(dtype)
    return np.ones(x.shape, bool) if lim is None else (np.isfinite(x) & (np.abs(x) < lim))


def convert_truncating(x, dtype):
    """The mutant: bf16 by dropping the low 16 bits, f16 by rounding toward zero."""
    if dtype == BF16:
        return _bf16_truncate(x)
    x = f32(x)
    with np.errstate(over="ignore", invalid="ignore"):
        h = x.astype(np.float16)
        over = np.abs(h.astype(np.float32)) > np.abs(x)
        return np.where(over & np.isfinite(x), np.nextafter(h, np.float16(0)), h).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# grid-stride kernels: one array with more elements than the 16384 x 256 threads a launch starts
# ---------------------------------------------------------------------------------------------------------------------
BIG_SHAPE = (2049, 2051)
GRID_THREADS = 16384 * 256
assert BIG_SHAPE[0] * BIG_SHAPE[1] > GRID_THREADS


def big_array():
    return f32(rng(9).standard_normal(BIG_SHAPE))


def big_refs(x):
    """name -> expected fp32 array of each op the big array goes through (all exact: one rounding or none)."""
    row, col = f32(rng(10).standard_normal(BIG_SHAPE[1])), f32(rng(12).standard_normal((BIG_SHAPE[0], 1)))
    return {"neg": -x, "add_row": x + row, "add_col": x + col, "transpose_contiguous": np.ascontiguousarray(x.T), "fill": np.full(BIG_SHAPE, 1.25, np.float32),
            "triu1": np.triu(x, 1), "bf16_round_trip": bf16_round(x), "cat_self": np.concatenate([x, x], 0)}, row, col


def grid_stride_dropped(ref):
    """The mutant: `if (i < n)` where the `for (; i < n; i += grid)` loop belongs -- elements past the grid stay unwritten."""
    r = np.array(ref, copy=True)
    r.reshape(-1)[GRID_THREADS:] = 0
    return r


UNARY_MUTANTS = {
    "f16_math": lambda name, x: UNARY_TORCH[name](torch.from_numpy(f32(x)).half().float()).half().double().numpy(),   # evaluated through __half
    "gelu_tanh": lambda name, x: F.gelu(torch.from_numpy(f32(x)).double(), approximate="tanh").numpy(),
}
