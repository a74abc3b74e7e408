"""The batched decode step's kernels (5 to 32 sequences per group): launch_skinny (csrc/k_skinny.hip) in every form its launcher can
pick, launch_decode_attn_batched, and launch_decode_attn at S > 1 with launch_attn_combine behind it (csrc/k_dattn.hip) -- cases,
float64 references, derived per-element bounds and the numpy restatements of the kernels' plausible mistakes.  Same method and helpers
as tests/gemm_ref.py and tests/decode_kernels_ref.py.  Shared by tests/test_batched_decode_ref_host.py (CPU: an honest float32
evaluation in another summation order lies inside every bound, every applicable mutant outside by a stated factor, the case table
reaches every family of FAMILIES) and tests/test_gpu_batched_decode_kernels.py (GPU: one launch per case through
q3a_selftest_skinny_launch / q3a_selftest_batched_attn_launch, every element of every output buffer compared, the reported
instantiation compared with the case's `form`).

A result is a whole output buffer: float64 values where the launch must write, NaN (the sentinel) everywhere else -- rows >= S, columns
N..ldo, fragment slots and next_ss entries of sequences >= S.  Every input slot of a sequence >= S (fragment buffers, ss_parts columns)
holds NaN, so a read from the wrong slot shows.

Bounds (u = 2^-24).  The operands that enter the MFMA are known exactly: W is bf16, the x operand is bf16(fl32(x g)) (bf16(x) without a
norm; the bf16 sources as given) -- one IEEE multiply and one rounding, both reproduced in numpy.  So:
    dot product             gamma_(K + 16) sum|a||w|, gamma_n = n u / (1 - n u): any order, the cross-wave sum included (ops_ref.matmul_bound
                            is the first-order form (K + 2) u, which it asserts for K <= 5792 only; K = 6144 is a case here)
    split = 1               the operand is fl32(x g) itself; + 2^-8 sum half_ulp_bf16(a)|w| for hi + lo, 2 K terms of (1 + 2^-7) the size
    rstd                    relative (K + 16) u from the sum of squares in any order, + 2 u (1 ulp of v_rsq_f32) with fast_math
    v = dot rstd            e = rstd e_dot + |v| (r_rstd + u);  bias, residual: gemm_ref.add_step
    GLU                     gemm_ref.glu_step (silu_fast's bound with fast_math, the precise silu gate without)
    bf16 output             gemm_ref.bf16_out_bound = half_ulp_bf16(|ref| + e) + e
    next_xw16f, next_ss     from the `out` the launch wrote: bf16_out_bound(out w, u |out w|); (16 + 2) u sum out^2 (8 + 2 under quarter
                            workgroups)
    attention               decode_kernels_ref's: new rows within new_row_bound, every other cache row bit-unchanged, the context against
                            float64 on the rows the launch appended.  The batched bf16 kernel forms its scores from bf16(q): the score
                            bound gains sum_d |k_jd| (half_ulp_bf16(|q_d| + e_q) + e_q) / scale, e_q = GAMMA_Q |q_d|.  That is wide, so
                            every case also runs the fp32-cache instantiation (no q rounding, expf), where the tight bound applies.

Worst excess (|got - ref| / bound, <= 1 passes) on an MI355X, printed by tests/test_gpu_batched_decode_kernels.py:
    family (kind, TILES, activations)                   fp32 out    bf16 out    next_xw16f  next_ss     (bf16: half-ulp bounds, near 1 by construction)
    direct, 1 tile, fp32 x (K = 32: 0.015) / split      0.015       -           -           -           split = 1: 0.0057
    direct, 1 tile, bf16 x                              0.0018      -           -           -
    direct, 2 tiles, fp32 x split / bf16 x              0.0011      0.809       -           -
    LDS-staged, 1 tile, fp32 x / bf16 x                 0.0018      -           0.9999      0.128       (0.0046 with bf16 x)
    LDS-staged, 2 tiles (pair), fp32 x / bf16 x         0.0011      0.881       -           -
    two-pass pair, aliased partial tile                 -           0.809       -           -
    half-pair tiles                                     0.0010      0.881       -           -
    quarter workgroups                                  0.0046      -           0.9999      0.208
    hand-over chain: consumer on the producer's buffers 0.0010; against the fused-norm launch 0.0003 of the joint bound
    quarter / full workgroups: sums of next_ss          0.027 of the joint bound apart
    batched attention, bf16 cache (scores from bf16 q)  context 0.016 (fp32 out), 0.019 (bf16 out); new rows 0.997
    batched attention, fp32 cache                       context 0.0006 (fp32 out), 0.92 (bf16 out); new rows 0.018
    split path + attn_combine                           0.034 of the merge bound (fp32), 0.9998 of half a bf16 ulp; context 0.0004 / 0.79 of the attention bound
Every case reported the form its table entry states, and every bit-identity held.
"""
import numpy as np

import decode_kernels_ref as D
from decode_kernels_ref import U, _norm_rope, bf16_bits, bf16_round, bf16_value, merge_partials, new_row_bound
from gemm_ref import SENT16, SENT32, add_step, bf16_out_bound, decode, glu_step, half_ulp_bf16

EPS = 0.5
NAN16 = np.uint16(0x7FC0)   # what the slots of sequences >= S hold in a bf16 input buffer
WAVES = 8                   # k_skinny.hip SK_WAVES: K is split eight ways


# ---------------------------------------------------------------------------------------------------------------------
# skinny GEMM: the case table
# ---------------------------------------------------------------------------------------------------------------------
# x: "f32" fp32 x, "f32norm" fp32 x + rms_w, "x16" bf16 row-major, "x16frag" bf16 fragment order, "pre" pre-normalised (xw16f + ss_parts)
# out: "f32", "bf16" (row-major), "bf16frag".   form: what launch_skinny must report -- kind (direct / wlds / qs / palias / hp), TILES, SH,
# XMODE, UNR, dynamic LDS bytes; `passes` = LDS passes over a wave's K slice (k-steps per wave / UNR), stated for the record.
def _form(kind, tiles, sh, xmode, unr, dyn_lds, split=0):
    return dict(kind=kind, split=split, tiles=tiles, sh=sh, xmode=xmode, unr=unr, wlds=int(kind != "direct"), qs=int(kind == "qs"),
                palias=int(kind in ("palias", "hp")), hp=int(kind == "hp"), dyn_lds=dyn_lds)


def _c(name, K, N, S, mode, x, form, out="f32", **kw):
    c = dict(name=name, K=K, N=N, S=S, mode=mode, x=x, form=form, out=out, bias=False, split=False, qsplit=False, inplace=False, next=False,
             glu_hp3=1, n_cu=0, ss_nparts=64, fast=x not in ("f32", "f32norm"))
    c.update(kw)
    return c


SKINNY_CASES = (
    # 1: LDS-staged weights, one pass of 4 steps; S at both sides of the sequence-half threshold; the last block has 6 live rows
    [_c(f"01-wlds-norm-bias-s{S}", 1024, 70, S, 0, "f32norm", _form("wlds", 1, 1 if S <= 16 else 2, 1, 4, 32768), bias=True) for S in (5, 16, 17, 32)] + [
    _c("02-split-direct", 1024, 70, 21, 0, "f32norm", _form("direct", 1, 2, 1, 4, 0, split=1), split=True),
    # 3: 8 steps per wave in passes of 6: a pass of 6, then 2 live + 4 dead
    _c("03-direct-unr6-dead-tail", 2048, 70, 21, 0, "f32norm", _form("direct", 1, 2, 1, 6, 0)),
    _c("04-wlds-unr6-two-passes-inplace", 3072, 70, 21, 1, "f32", _form("wlds", 1, 2, 0, 6, 49152), inplace=True),
    # 5: 9 steps, 2 per wave: waves hold 2, 2, 2, 2, 1, 0, 0, 0
    _c("05-direct-ragged-k288", 288, 70, 21, 0, "f32", _form("direct", 1, 2, 0, 4, 0)),
    _c("06-direct-one-step-k32", 32, 20, 5, 0, "f32", _form("direct", 1, 1, 0, 4, 0)),
    # 7: 36 steps, 5 per wave, wave 7 holds one
    _c("07-direct-unr8-x16-rowmajor", 1152, 70, 21, 1, "x16", _form("direct", 1, 2, 2, 8, 0)),
    _c("07-direct-unr8-x16-frag", 1152, 70, 21, 1, "x16frag", _form("direct", 1, 2, 2, 8, 0)),
    _c("08-wlds-unr12-next", 3072, 70, 21, 1, "x16frag", _form("wlds", 1, 2, 2, 12, 98304), next=True),
    _c("08-wlds-unr12-two-passes-next", 6144, 70, 21, 1, "x16frag", _form("wlds", 1, 2, 2, 12, 98304), next=True)] + [
    # 9: quarter workgroups; two sequence halves except at S = 9
    _c(f"09-qs-k{K}-s{S}", K, N, S, 1, "x16frag", _form("qs", 1, 1, 2, unr, WAVES * (unr // 2) * 1024), qsplit=True, bias=True, next=True, inplace=True)
    for K, N, S, unr in ((512, 64, 32, 2), (1024, 64, 17, 4), (2048, 128, 21, 8), (3072, 64, 9, 12), (6144, 64, 17, 12))] + [
    _c("10-pair-wlds-norm-bias", 1024, 96, 21, 2, "f32norm", _form("wlds", 2, 2, 1, 4, 65536), bias=True),
    _c("10-pair-wlds-norm-bias-s9", 1024, 96, 9, 2, "f32norm", _form("wlds", 2, 1, 1, 4, 65536), bias=True),
    _c("11-pair-split-direct", 2048, 64, 21, 2, "f32norm", _form("direct", 2, 2, 1, 6, 0, split=1), split=True),
    _c("12-pair-wlds-s21", 1024, 96, 21, 2, "pre", _form("wlds", 2, 2, 3, 4, 65536), out="bf16frag", glu_hp3=0),
    _c("12-hp3-one-pass-s21", 1024, 96, 21, 2, "pre", _form("hp", 3, 2, 3, 4, 98304), out="bf16frag", glu_hp3=2),
    _c("12-pair-wlds-s9", 1024, 96, 9, 2, "pre", _form("wlds", 2, 1, 3, 4, 65536), out="bf16frag", glu_hp3=0),
    _c("12-hp3-one-pass-s9", 1024, 96, 9, 2, "pre", _form("hp", 3, 1, 3, 4, 98304), out="bf16frag", glu_hp3=2),
    _c("12-hp3-bias-f32-out", 1024, 96, 21, 2, "pre", _form("hp", 3, 2, 3, 4, 98304), glu_hp3=2, bias=True),
    _c("13-hp3-two-passes-s9", 2048, 96, 9, 2, "pre", _form("hp", 3, 1, 3, 4, 98304), out="bf16", glu_hp3=2),
    _c("13-hp3-two-passes-s21", 2048, 96, 21, 2, "pre", _form("hp", 3, 2, 3, 4, 98304), out="bf16", glu_hp3=2),
    # 14: glu_hp3 = 1 takes the half-pair form only where it balances: 6 pair tiles > 5 CUs and 4 workgroups <= 5
    _c("14-hp3-balances-ncu5", 1024, 192, 21, 2, "pre", _form("hp", 3, 2, 3, 4, 98304), out="bf16", glu_hp3=1, n_cu=5),
    _c("14-pair-wlds-ncu256", 1024, 192, 21, 2, "pre", _form("wlds", 2, 2, 3, 4, 65536), out="bf16", glu_hp3=1, n_cu=256),
    # 15: the pair form at hidden 2048: two passes with the aliased partial tile when the grid exceeds the CUs; otherwise the 128 KiB
    # image fits next to the static partial tile of ONE sequence half only (sk_dyn_lds_max(2, 2) = 125952): direct loads at S > 16
    _c("15-pair-two-pass-palias", 2048, 64, 21, 2, "pre", _form("palias", 2, 2, 3, 4, 65536), out="bf16", glu_hp3=0, n_cu=1),
    _c("15-pair-two-pass-palias-s9", 2048, 64, 9, 2, "pre", _form("palias", 2, 1, 3, 4, 65536), out="bf16", glu_hp3=0, n_cu=1),
    _c("15-pair-direct-unr8", 2048, 64, 21, 2, "pre", _form("direct", 2, 2, 3, 8, 0), out="bf16", glu_hp3=0, n_cu=256),
    _c("15-pair-wlds-unr8-128k-s9", 2048, 64, 9, 2, "pre", _form("wlds", 2, 1, 3, 8, 131072), out="bf16", glu_hp3=0, n_cu=256),
    _c("16-pair-two-pass-unr6-x16", 3072, 64, 21, 2, "x16frag", _form("palias", 2, 2, 2, 6, 98304), out="bf16", n_cu=1),
    _c("16-pair-direct-unr12-x16", 3072, 64, 21, 2, "x16frag", _form("direct", 2, 2, 2, 12, 0), out="bf16", n_cu=256)] + [
    # 17: the producer's partial rows; 300 runs the loop behind the SS_PRE prefetch (256 rows)
    _c(f"17-pre-nparts{p}", 1024, 70, 21, 0, "pre", _form("wlds", 1, 2, 3, 4, 32768), ss_nparts=p) for p in (64, 128, 256, 300)] + [
    _c("17-pre-nparts64-s9", 1024, 70, 9, 0, "pre", _form("wlds", 1, 1, 3, 4, 32768), ss_nparts=64)])
SKINNY_BY_NAME = {c["name"]: c for c in SKINNY_CASES}

# (kind, TILES, SH, XMODE class) of every skinny_kernel family: the twelve whose large dynamic LDS skinny_init() registers
# (allow_big_lds_shapes: LDS-staged x 1 / 2 tiles x 1 / 2 sequence halves x fp32 / bf16 activations; allow_glu_hp3; allow_glu_2pass),
# the quarter workgroups (48 KiB at most: no attribute) and the direct-load families a legal call reaches
FAMILIES = [("wlds", 1, 1, "fp32"), ("wlds", 1, 2, "fp32"), ("wlds", 2, 1, "fp32"), ("wlds", 2, 2, "fp32"),
            ("wlds", 1, 1, "bf16"), ("wlds", 1, 2, "bf16"), ("wlds", 2, 1, "bf16"), ("wlds", 2, 2, "bf16"),
            ("hp", 3, 1, "bf16"), ("hp", 3, 2, "bf16"), ("palias", 2, 1, "bf16"), ("palias", 2, 2, "bf16"),
            ("qs", 1, 1, "bf16"),
            ("direct", 1, 1, "fp32"), ("direct", 1, 2, "fp32"), ("direct", 1, 2, "bf16"), ("direct", 2, 2, "fp32"), ("direct", 2, 2, "bf16")]


def family(c):
    f = c["form"]
    return (f["kind"], f["tiles"], f["sh"], "fp32" if f["xmode"] < 2 else "bf16")


def cols_of(c):
    return c["N"] // 2 if c["mode"] == 2 else c["N"]


def ldo_of(c):
    return cols_of(c) + 3       # columns N..ldo must come back untouched


def ldx_of(c):
    return c["K"] + 8           # columns K..ldx hold 1000: a read past K shows in any sum


def frag_len(cols):
    return 32 * ((cols + 31) // 32 * 32)


def ss_rows_of(c):
    return c["N"] // 8 if c["qsplit"] else (c["N"] + 15) // 16


def frag_index(s, k, mut=None):
    """kernels.h skinny_frag_index, with the two index mutants."""
    ks, h, kc, l, e = k >> 5, s >> 4, (k >> 3) & 3, s & 15, k & 7
    if mut == "frag-halves-swapped":
        h = h ^ 1
    if mut == "frag-kchunk-seq-swapped":
        return (((ks * 2 + h) * 16 + l) * 4 + kc) * 8 + e
    return (((ks * 2 + h) * 4 + kc) * 16 + l) * 8 + e


_data = {}


def skinny_inputs(c):
    """The logical operands of a case, always for 32 sequences (a case uses rows 0 .. S - 1).  They depend on (K, N, mode) alone, so the
    forms that must agree bit for bit (pair / half pair, full / quarter workgroups, row-major / fragment order, S = 5 / 21) run on the
    same data.  Every sequence has its own random row; the rows share a sign pattern p_k that the weight rows carry too, so a dot product
    is a fixed share of sum |terms| (not a random walk) and bias / residual of order 1 stay visible next to it.  The last four columns are
    loud, sqrt(3 K / 8) times the others: they carry half of sum x^2, so the last partial row weighs whichever way the sum is cut (one
    row of 300 dropped must show through a bf16 output's half ulp)."""
    key = (c["K"], c["N"], c["mode"])
    if key not in _data:
        if len(_data) > 8: _data.clear()
        K, N = c["K"], c["N"]
        r = D._rng("skinny-%d-%d-%d" % key)
        p = np.where(r.uniform(size=K) < 0.5, -1.0, 1.0)
        x = r.normal(0, 1, (32, K)) + 0.7 * p * r.uniform(0.5, 1.5, (32, 1))
        x[:, K - 4:] *= np.sqrt(3 * K / 8)
        a = r.uniform(-1, 1, (N, 1))
        W = bf16_round(((r.normal(0, 1, (N, K)) + a * p) * (4.0 / K)).astype(np.float32))
        sgn = lambda *n: np.where(r.uniform(size=n) < 0.5, -1.0, 1.0)
        cols = N // 2 if c["mode"] == 2 else N
        _data[key] = dict(x=x.astype(np.float32), g=(1.5 + 0.5 * r.uniform(-1, 1, K)).astype(np.float32), W=W,
                          bias=(sgn(N) * r.uniform(1, 2, N)).astype(np.float32), resid=(sgn(32, cols) * r.uniform(1, 2, (32, cols))).astype(np.float32),
                          next_w=(1.5 + 0.5 * r.uniform(-1, 1, N)).astype(np.float32))
    return dict(_data[key])


def gamma(n):
    return n * U / (1.0 - n * U)


def part_of_column(K, nparts):
    """The partial row of sum x^2 that column k belongs to (contiguous runs, as the producers write them)."""
    return np.arange(K) * nparts // K


def pack(c, d):
    """The arrays of one q3a_selftest_skinny_launch call.  Slots of sequences >= S hold NaN; output buffers the sentinel."""
    K, N, S, cols, ldo, ldx = c["K"], c["N"], c["S"], cols_of(c), ldo_of(c), ldx_of(c)
    x = d["x"][:S]
    pk = {}
    s_idx, k_idx = np.arange(S)[:, None], np.arange(K)[None, :]
    def to_frag(v):   # [S][K] bf16-representable values -> fragment order, 32 sequences' room
        buf = np.full(32 * K, NAN16, np.uint16)
        buf[frag_index(s_idx, k_idx)] = bf16_bits(v)
        return buf
    if c["x"] in ("f32", "f32norm"):
        xs = np.full((S, ldx), 1000.0, np.float32)
        xs[:, :K] = x
        pk["x"] = xs
    elif c["x"] == "x16":
        xs = np.full((S, ldx), bf16_bits(np.float32(1000.0)), np.uint16)
        xs[:, :K] = bf16_bits(bf16_round(x))
        pk["x16"] = xs
    elif c["x"] == "x16frag":
        pk["x16"] = to_frag(bf16_round(x))
    else:
        pk["xw16f"] = to_frag(bf16_round((x * d["g"]).astype(np.float32)))
        parts = np.full((c["ss_nparts"], 32), np.nan, np.float32)
        sq = x.astype(np.float64) ** 2
        part = part_of_column(K, c["ss_nparts"])
        for p in range(c["ss_nparts"]):
            parts[p, :S] = sq[:, part == p].sum(axis=1)
        pk["ss_parts"] = parts
    if c["x"] == "f32norm": pk["rms_w"] = d["g"]
    if c["bias"]: pk["bias"] = d["bias"]
    out = np.full((32, ldo), SENT32, np.uint32)
    if c["mode"] == 1:
        if c["inplace"]:
            out[:S, :N] = d["resid"][:S].view(np.uint32)
        else:
            rs = np.full((S, ldo), 1000.0, np.float32)
            rs[:, :N] = d["resid"][:S]
            pk["resid"] = rs
    if c["out"] == "f32": pk["out"] = out
    elif c["out"] == "bf16": pk["out16"] = np.full((32, ldo), SENT16, np.uint16)
    else: pk["out16"] = np.full(frag_len(cols), SENT16, np.uint16)
    if c["next"]:
        pk["next_w"] = d["next_w"]
        pk["next_xw16f"] = np.full(frag_len(N), SENT16, np.uint16)
        pk["next_ss"] = np.full((ss_rows_of(c), 32), SENT32, np.uint32)
    return pk


def decode_outputs(c, pk):
    """The output buffers of a launch as float64 (the sentinel reads NaN, any other non-finite value inf)."""
    o = {}
    if "out" in pk: o["out"] = decode(pk["out"], False)
    if "out16" in pk: o["out16"] = decode(pk["out16"], True)
    if c["next"]:
        o["next_x"], o["next_ss"] = decode(pk["next_xw16f"], True), decode(pk["next_ss"], False)
    return o


def _main_key(c):
    return "out" if c["out"] == "f32" else "out16"


def _place(c, v, mut=None):
    """v [S][cols] -> the main output buffer's layout, NaN where nothing is written."""
    S, cols, ldo = c["S"], cols_of(c), ldo_of(c)
    if c["out"] == "bf16frag":
        buf = np.full(frag_len(cols), np.nan)
        s_idx, c_idx = np.arange(S)[:, None], np.arange(cols)[None, :]
        buf[s_idx * cols + c_idx if mut == "frag-out-row-major" else frag_index(s_idx, c_idx)] = v
        return buf
    buf = np.full((32, ldo), np.nan)
    buf[:S, :cols] = v
    return buf


def next_reference(c, d, out_written):
    """(ref, bound) of next_xw16f and next_ss from the fp32 `out` [32][ldo] the launch wrote (decoded)."""
    N, S = c["N"], c["S"]
    y = out_written[:S, :N]
    nx = y * d["next_w"].astype(np.float64)
    s_idx, n_idx = np.arange(S)[:, None], np.arange(N)[None, :]
    rx, bx = np.full(frag_len(N), np.nan), np.ones(frag_len(N))
    rx[frag_index(s_idx, n_idx)] = nx
    bx[frag_index(s_idx, n_idx)] = bf16_out_bound(nx, U * np.abs(nx))
    blk, rows = (8 if c["qsplit"] else 16), ss_rows_of(c)
    rs, bs = np.full((rows, 32), np.nan), np.ones((rows, 32))
    for r in range(rows):
        q = (y[:, r * blk:min((r + 1) * blk, N)] ** 2).sum(axis=1)
        rs[r, :S], bs[r, :S] = q, (blk + 2) * U * q + 2.0 ** -140
    return dict(next_x=(rx, bx), next_ss=(rs, bs))


def skinny_reference(c, d, out_written=None):
    """name -> (ref, bound), whole buffers in float64.  out_written: the decoded `out` of the launch under test, for the next_* outputs."""
    K, N, S, fast = c["K"], c["N"], c["S"], c["fast"]
    W = d["W"].astype(np.float64)
    x = d["x"][:S]
    p = (x * d["g"]).astype(np.float32) if c["x"] in ("f32norm", "pre") else x
    if c["split"]:
        A = p.astype(np.float64)
        e = gamma(2 * K + 16) * (1 + 2.0 ** -7) * (np.abs(A) @ np.abs(W).T) + 2.0 ** -8 * (half_ulp_bf16(A) @ np.abs(W).T)
    else:
        A = bf16_round(p).astype(np.float64)
        e = gamma(K + 16) * (np.abs(A) @ np.abs(W).T)
    v = A @ W.T
    if c["x"] in ("f32norm", "pre"):
        if c["x"] == "pre":
            q = pack(c, d)["ss_parts"][:, :S].astype(np.float64).sum(axis=0)   # the fp32 partial rows as the launch is given them
        else:
            q = (x.astype(np.float64) ** 2).sum(axis=1)
        rstd = (1.0 / np.sqrt(q / K + EPS))[:, None]
        v = v * rstd
        e = rstd * e + np.abs(v) * (gamma(K + 16) + (2 * U if fast else 0.0) + U)
    if c["bias"]:
        v, e = add_step(v, e, d["bias"].astype(np.float64))
    if c["mode"] == 1:
        v, e = add_step(v, e, d["resid"][:S].astype(np.float64))
    if c["mode"] == 2:
        gi, ui = D.glu_rows(N)
        v, e = glu_step(v[:, gi], e[:, gi], v[:, ui], e[:, ui], fast)
    if c["out"] != "f32":
        e = bf16_out_bound(v, e)
    ref = {_main_key(c): (_place(c, v), np.nan_to_num(_place(c, e), nan=1.0))}
    if c["next"] and out_written is not None:
        ref.update(next_reference(c, d, out_written))
    return ref


def buffer_excess(got, ref, bound):
    """Worst |got - ref| / bound over the elements a launch must write (inf: one of them is not finite, or an element that must keep the
    sentinel does not)."""
    got = np.asarray(got, np.float64)
    keep = np.isnan(ref)
    if got.shape != ref.shape or not np.all(np.isnan(got[keep])) or not np.all(np.isfinite(got[~keep])):
        return np.inf
    err = np.abs(got[~keep] - ref[~keep])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound[~keep])
    return float(r.max()) if r.size else 0.0


def skinny_excess_by_buffer(c, d, outs):
    """Worst excess of each output buffer of a launch (outs: decode_outputs or skinny_sim)."""
    ref = skinny_reference(c, d, outs.get("out"))
    return {k: buffer_excess(outs[k], *ref[k]) for k in ref}


def skinny_excess(c, d, outs):
    return max(skinny_excess_by_buffer(c, d, outs).values())


# ---------------------------------------------------------------------------------------------------------------------
# skinny GEMM: the kernel's plausible mistakes, restated in numpy on the buffers the launch is given
# ---------------------------------------------------------------------------------------------------------------------
SKINNY_MUTANTS = ["frag-halves-swapped", "frag-kchunk-seq-swapped", "ss_nparts-1", "parts-beyond-256-dropped", "ss-other-half", "hp-up-row+8",
                  "glu-bias-by-column", "dead-step-counted", "last-live-step-dropped", "row-clamp-n-against-k", "qs-halves-ignored",
                  "next-ss-16-row-index", "resid-after-store", "frag-out-row-major"]


def wave_steps(c):
    """[(ks0, ks1)] of the eight waves: k-steps of 32 columns."""
    steps = c["K"] // 32
    per = (steps + WAVES - 1) // WAVES
    return [(w * per, max(w * per, min(steps, w * per + per))) for w in range(WAVES)]


def step_weights(c, mut=None):
    """How often each k-step enters the sum (1 everywhere in the kernel as written)."""
    m = np.ones(c["K"] // 32)
    for ks0, ks1 in wave_steps(c):
        if ks1 == ks0: continue
        if mut == "dead-step-counted" and not c["form"]["wlds"]:   # the tail's address is clamped to the last live step: its weight not zeroed
            m[ks1 - 1] += (-(ks1 - ks0)) % c["form"]["unr"]
        if mut == "last-live-step-dropped":
            m[ks1 - 1] -= 1
    return m


def skinny_applies(c, m):
    f = c["form"]
    return {"frag-halves-swapped": c["x"] in ("x16frag", "pre"), "frag-kchunk-seq-swapped": c["x"] in ("x16frag", "pre"),
            "ss_nparts-1": c["x"] == "pre", "parts-beyond-256-dropped": c["x"] == "pre" and c["ss_nparts"] > 256,
            "ss-other-half": c["x"] == "pre", "hp-up-row+8": bool(f["hp"]), "glu-bias-by-column": c["mode"] == 2 and c["bias"],
            "dead-step-counted": bool((step_weights(c, "dead-step-counted") != 1).any()), "last-live-step-dropped": True,
            "row-clamp-n-against-k": c["mode"] != 2 and c["N"] % 16 != 0 and c["K"] > c["N"],
            "qs-halves-ignored": c["qsplit"] and c["S"] > 16, "next-ss-16-row-index": c["qsplit"] and c["next"],
            "resid-after-store": c["inplace"], "frag-out-row-major": c["out"] == "bf16frag"}[m]


def skinny_sim(c, d, mut=None, honest=False):
    """The launch in numpy on the packed buffers: float32 in another summation order (honest), or float64 with one mistake (mut).
    Returns the decoded output buffers."""
    dt = np.float32 if honest else np.float64
    K, N, S, cols, ldo = c["K"], c["N"], c["S"], cols_of(c), ldo_of(c)
    pk = pack(c, d)
    W = d["W"].astype(dt)
    s_idx, k_idx = np.arange(S)[:, None], np.arange(K)[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        # the MFMA operand, as the kernel fetches it
        x = None
        if c["x"] in ("x16frag", "pre"):
            A = bf16_value(pk["xw16f" if c["x"] == "pre" else "x16"])[frag_index(s_idx, k_idx, mut)].astype(dt)
        elif c["x"] == "x16":
            A = bf16_value(pk["x16"])[:, :K].astype(dt)
        else:
            x = pk["x"][:, :K]
            p = (x * d["g"]).astype(np.float32) if c["x"] == "f32norm" else x
            hi = bf16_round(p)
            if c["split"] and honest:
                A, W = np.concatenate([hi, bf16_round(p - hi)], 1), np.concatenate([W, W], 1)
            else:
                A = (p if c["split"] else hi).astype(dt)
        wt = np.repeat(step_weights(c, mut), 32).astype(dt)
        if A.shape[1] == 2 * K: wt = np.concatenate([wt, wt])
        v = np.matmul((A * wt)[:, ::-1], W[:, ::-1].T).astype(dt)
        if c["x"] in ("f32norm", "pre"):
            if c["x"] == "pre":
                n = c["ss_nparts"] - (mut == "ss_nparts-1")
                if mut == "parts-beyond-256-dropped": n = min(n, 256)
                col = np.arange(S) ^ (16 if mut == "ss-other-half" else 0)
                q = pk["ss_parts"][:n][::-1, col].sum(axis=0, dtype=dt)
            else:
                q = (x[:, ::-1].astype(dt) ** 2).sum(axis=1, dtype=dt)
            v = (v * (dt(1) / np.sqrt(q / dt(K) + dt(EPS)))[:, None]).astype(dt)
        bias = d["bias"].astype(dt) if c["bias"] else np.zeros(N, dt)
        outs = {}
        if c["mode"] == 2:
            j = np.arange(cols)
            gi = (j // 16) * 32 + j % 16
            ui = gi + (8 if mut == "hp-up-row+8" else 16)
            bg, bu = (bias[j], bias[j + cols]) if mut == "glu-bias-by-column" else (bias[gi], bias[ui])
            G, Uv = v[:, gi] + bg, v[:, ui] + bu
            y = (G / (dt(1) + np.exp(-G)) * Uv).astype(dt)
        else:
            y = v + bias
            if c["mode"] == 1:
                rs = d["resid"][:S].astype(dt)
                y = y + (np.roll(y + rs, 1, axis=0) if mut == "resid-after-store" else rs)
            y = y.astype(dt)
        if c["out"] != "f32":
            y = bf16_round(y.astype(np.float32))
        full = _place(c, y.astype(np.float64), mut)
        if mut == "row-clamp-n-against-k":   # stores gated by n < K: the last block's void rows are written
            full[:S, N:min((N + 15) // 16 * 16, K, ldo)] = 0.0
        if mut == "qs-halves-ignored":       # both halves of a row tile work on sequences 0 .. 15
            full[16:] = np.nan
        outs[_main_key(c)] = full
        if c["next"]:
            y32 = y.astype(np.float32)
            nx = np.full(frag_len(N), np.nan)
            nx[frag_index(s_idx, np.arange(N)[None, :])] = bf16_round(y32 * d["next_w"])
            blk, rows = (8 if c["qsplit"] else 16), ss_rows_of(c)
            ss = np.full((rows, 32), np.nan)
            for r in range(rows):
                row = r // 2 if mut == "next-ss-16-row-index" else r
                ss[row, :S] = (y32[:, r * blk:min((r + 1) * blk, N)][:, ::-1].astype(dt) ** 2).sum(axis=1, dtype=dt)
            if mut == "qs-halves-ignored": nx[frag_index(np.arange(16, 32)[:, None], np.arange(N)[None, :])] = np.nan; ss[:, 16:] = np.nan
            outs["next_x"], outs["next_ss"] = nx, ss
    return outs


# ---------------------------------------------------------------------------------------------------------------------
# batched decode attention and the split path at S > 1
# ---------------------------------------------------------------------------------------------------------------------
SCALE, GAMMA_Q, ATTN_EPS = D.SCALE, D.GAMMA_Q, D.DATTN_EPS
POS6 = (0, 127, 128, 255, 300, 639)   # tile edges: 300 uses three tiles (ring slot 0 refilled once), 639 five, the cache's last row
ATTN_CASES = [
    dict(name="edges-trim0", n_q=4, n_kv=2, pos=POS6, max_ctx=640, trim=0),
    dict(name="edges-trim1", n_q=4, n_kv=2, pos=POS6, max_ctx=640, trim=1),
    dict(name="ctx128-prologue-clamp", n_q=4, n_kv=2, pos=(0, 127), max_ctx=128, trim=0),   # the prologue's second tile clamps onto tile 0
    dict(name="ctx128-prologue-clamp-trim1", n_q=4, n_kv=2, pos=(0, 127), max_ctx=128, trim=1),
    dict(name="group1", n_q=2, n_kv=2, pos=(130,), max_ctx=256, trim=0),
    dict(name="group4", n_q=8, n_kv=2, pos=(130,), max_ctx=256, trim=0),
]
SPLIT_CASE = dict(name="split-5x128", n_q=4, n_kv=2, pos=POS6, max_ctx=640, nsplit=5, keys=128)
OUT_FORMS = ("f32", "bf16", "bf16frag")


def attn_inputs(c, kv_f32, stale_nan=True):
    """qkv [S][n_q + 2 n_kv][128], norm weights, rope [S][128], caches [S][n_kv][max_ctx][128] (fp32 values, bf16-representable unless
    kv_f32).  Rows >= pos hold NaN (stale_nan: the batched cases) or data four times as loud (the split path, as decode_kernels_ref)."""
    r = D._rng("attn-" + c["name"].split("-trim")[0] + ("-f32" if kv_f32 else ""))
    S, n_q, n_kv, ctx = len(c["pos"]), c["n_q"], c["n_kv"], c["max_ctx"]
    qkv = r.normal(0, 1, (S, n_q + 2 * n_kv, 128)).astype(np.float32)
    q_norm = (1.5 + 0.5 * r.uniform(-1, 1, 128)).astype(np.float32)
    k_norm = (0.75 + 0.25 * r.uniform(-1, 1, 128)).astype(np.float32)
    ang = r.uniform(0, 2 * np.pi, (S, 64))
    rope = np.concatenate([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)
    kc = r.normal(0, 1, (S, n_kv, ctx, 128)).astype(np.float32)
    vc = r.normal(0, 1, (S, n_kv, ctx, 128)).astype(np.float32)
    if not kv_f32: kc, vc = bf16_round(kc), bf16_round(vc)
    for s, p in enumerate(c["pos"]):
        if stale_nan: kc[s, :, p:] = np.nan; vc[s, :, p:] = np.nan
        else: kc[s, :, p:] *= 4; vc[s, :, p:] *= 4
    return dict(qkv=qkv, q_norm=q_norm, k_norm=k_norm, rope=rope, kc=kc, vc=vc, pos=np.asarray(c["pos"], np.int32), kv_f32=kv_f32)


def attn_new_rows(c, d, dt=np.float64):
    """q [S][n_q][128], the new k and v rows [S][n_kv][128] before they are stored."""
    n_q, n_kv = c["n_q"], c["n_kv"]
    rope = d["rope"][:, None, :]
    q = np.stack([_norm_rope(d["qkv"][s, :n_q], d["q_norm"], ATTN_EPS, d["rope"][s], dt) for s in range(len(c["pos"]))])
    k = np.stack([_norm_rope(d["qkv"][s, n_q:n_q + n_kv], d["k_norm"], ATTN_EPS, d["rope"][s], dt) for s in range(len(c["pos"]))])
    return q, k, d["qkv"][:, n_q + n_kv:].astype(dt)


def row_bound(exact, kv_f32):
    """bf16 cache: decode_kernels_ref.new_row_bound (the rounding dominates).  fp32 cache: the stored value is the rotation c n1 -+ s n2
    itself, whose rounding is relative to |c n1| + |s n2| <= hypot(n1, n2) = hypot of the element and its partner 64 further on (a
    rotation keeps it) -- not to the difference, which may cancel."""
    if not kv_f32: return new_row_bound(exact)
    return GAMMA_Q * np.hypot(exact, np.roll(exact, 64, axis=-1)) + 2.0 ** -133


ATTN_MUTANTS = ["pos-1", "pos+1", "caches-swapped", "edge-tile-inner", "new-row-not-patched", "group4-as-group2", "frag-out-row-major"]


def attn_applies(c, m, form="f32"):
    return {"group4-as-group2": c["n_q"] // c["n_kv"] == 4, "frag-out-row-major": form == "bf16frag", "pos-1": max(c["pos"]) > 0}.get(m, True)


def attn_context(c, d, k_rows, v_rows, dt=np.float64, bf16_q=False, mut=None):
    """Context [S][n_q][128] over cache rows 0 .. pos - 1 and the appended rows at pos, with decode_kernels_ref's bound (float64 only);
    bf16_q: the scores come from bf16(q) (honest float32) / the bound carries that rounding (float64)."""
    S, n_q, n_kv, ctx = len(c["pos"]), c["n_q"], c["n_kv"], c["max_ctx"]
    q, _, _ = attn_new_rows(c, d, dt)
    out, bound = np.zeros((S, n_q, 128)), np.zeros((S, n_q, 128))
    kc, vc = (d["vc"], d["kc"]) if mut == "caches-swapped" else (d["kc"], d["vc"])
    group = 2 if mut == "group4-as-group2" else n_q // n_kv
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            pos = int(np.clip(d["pos"][s] + {"pos-1": -1, "pos+1": 1}.get(mut, 0), 0, ctx - 1))
            for h in range(n_q):
                kv = (h // group) % n_kv
                K, V = np.concatenate([kc[s, kv, :pos], k_rows[s, kv][None]]), np.concatenate([vc[s, kv, :pos], v_rows[s, kv][None]])
                if mut == "new-row-not-patched":     # the cache's own row `pos`, as it was before the launch
                    K, V = kc[s, kv, :pos + 1], vc[s, kv, :pos + 1]
                if mut == "edge-tile-inner":         # every key of the tile that holds pos is live
                    end = min((pos // 128 + 1) * 128, ctx)
                    K, V = np.concatenate([K, kc[s, kv, pos + 1:end]]), np.concatenate([V, vc[s, kv, pos + 1:end]])
                K, V = K.astype(dt), V.astype(dt)
                qh = q[s, h]
                if dt is np.float32:
                    K, V = K[::-1], V[::-1]
                    if bf16_q: qh = bf16_round(qh)
                sc = (K * qh).sum(axis=1, dtype=dt) / dt(SCALE)
                p = np.exp(sc - sc.max())
                out[s, h] = (p[:, None] * V).sum(axis=0, dtype=dt) / p.sum(dtype=dt)
                if dt is np.float64 and mut is None:
                    ds = GAMMA_Q * (np.abs(K) * np.abs(qh)).sum(axis=1)
                    if bf16_q:
                        eq = GAMMA_Q * np.abs(qh)
                        ds = ds + (np.abs(K) * (half_ulp_bf16(np.abs(qh) + eq) + eq)).sum(axis=1)
                    e = 2 * ds.max() / SCALE + 8 * U * (np.abs(sc - sc.max()).max() + 2)
                    bound[s, h] = (2 * e + 2 * (len(sc) + 64) * U) * (p[:, None] * np.abs(V)).sum(axis=0) / p.sum() + 2.0 ** -133
    return out, bound


def attn_place(c, ctx, form, mut=None):
    """Context [S][n_q][128] -> the output buffer's layout (NaN where nothing is written)."""
    S, hd = len(c["pos"]), c["n_q"] * 128
    v = ctx.reshape(S, hd)
    if form != "bf16frag":
        return v.copy()
    buf = np.full(32 * hd, np.nan)
    s_idx, k_idx = np.arange(S)[:, None], np.arange(hd)[None, :]
    buf[s_idx * hd + k_idx if mut == "frag-out-row-major" else frag_index(s_idx, k_idx)] = v
    return buf


def attn_out_init(c, form):
    S, hd = len(c["pos"]), c["n_q"] * 128
    if form == "f32": return np.full((S, hd), SENT32, np.uint32)
    return np.full((S, hd) if form == "bf16" else 32 * hd, SENT16, np.uint16)


def attn_excess(c, d, kc_out, vc_out, out, form, bf16_q):
    return max(attn_excess_parts(c, d, kc_out, vc_out, out, form, bf16_q))


def attn_excess_parts(c, d, kc_out, vc_out, out, form, bf16_q):
    """Worst excess of one launch, (appended rows, context in its output form `out` (decoded)); inf when a cache row other than pos
    changed (compared as bits: the stale rows are NaN).  The context reference uses the rows the launch appended."""
    S = len(c["pos"])
    _, k64, v64 = attn_new_rows(c, d)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    worst = 0.0
    k_new, v_new = np.zeros_like(k64), np.zeros_like(v64)
    for s, p in enumerate(d["pos"]):
        kept = np.ones(c["max_ctx"], bool); kept[p] = False
        if not (np.array_equal(bits(kc_out[s][:, kept]), bits(d["kc"][s][:, kept])) and np.array_equal(bits(vc_out[s][:, kept]), bits(d["vc"][s][:, kept]))):
            return np.inf, np.inf
        k_new[s], v_new[s] = kc_out[s, :, p], vc_out[s, :, p]
    if not (np.all(np.isfinite(k_new)) and np.all(np.isfinite(v_new))):
        return np.inf, np.inf
    worst = max(worst, float((np.abs(k_new - k64) / row_bound(k64, d["kv_f32"])).max()), float((np.abs(v_new - v64) / row_bound(v64, d["kv_f32"])).max()))
    ref, bound = attn_context(c, d, k_new, v_new, bf16_q=bf16_q)
    if form != "f32": bound = bf16_out_bound(ref, bound)
    return worst, buffer_excess(out, attn_place(c, ref, form), np.nan_to_num(attn_place(c, bound, form), nan=1.0))


def attn_sim(c, d, form="f32", bf16_q=False, mut=None):
    """The batched launch in numpy float32, keys in descending order: (kc_out, vc_out, output buffer decoded); optionally one mistake."""
    _, k, v = attn_new_rows(c, d, np.float32)
    if not d["kv_f32"]: k, v = bf16_round(k), bf16_round(v)
    kc_out, vc_out = d["kc"].copy(), d["vc"].copy()
    for s, p in enumerate(d["pos"]):
        p = int(np.clip(p + {"pos-1": -1, "pos+1": 1}.get(mut, 0), 0, c["max_ctx"] - 1))
        (vc_out if mut == "caches-swapped" else kc_out)[s, :, p] = k[s]
        (kc_out if mut == "caches-swapped" else vc_out)[s, :, p] = v[s]
    ctx, _ = attn_context(c, d, k, v, np.float32, bf16_q=bf16_q, mut=mut)
    if form != "f32": ctx = bf16_round(ctx.astype(np.float32)).astype(np.float64)
    return kc_out, vc_out, attn_place(c, ctx, form, mut)


# ---- the split path: launch_decode_attn's partials, then launch_attn_combine -------------------------------------------------------
def split_partials_f32(c, d):
    """Honest float32 partials [S][n_q][nsplit] (, [128]) of the split kernel: keys of split sp are sp * keys .. min(pos, (sp + 1) * keys - 1)."""
    S, n_q, n_kv, ns, keys = len(c["pos"]), c["n_q"], c["n_kv"], c["nsplit"], c["keys"]
    f = np.float32
    q, k, v = attn_new_rows(c, d, f)
    k, v = bf16_round(k), bf16_round(v)
    pm, pl, po = np.full((S, n_q, ns), -np.inf, f), np.zeros((S, n_q, ns), f), np.zeros((S, n_q, ns, 128), f)
    for s, pos in enumerate(d["pos"]):
        for h in range(n_q):
            kv = h // (n_q // n_kv)
            K, V = np.concatenate([d["kc"][s, kv, :pos], k[s, kv][None]]), np.concatenate([d["vc"][s, kv, :pos], v[s, kv][None]])
            for sp in range(pos // keys + 1):
                Ks, Vs = K[sp * keys:(sp + 1) * keys][::-1], V[sp * keys:(sp + 1) * keys][::-1]
                sc = (Ks * q[s, h]).sum(axis=1, dtype=f) / f(SCALE)
                p = np.exp(sc - sc.max())
                pm[s, h, sp], pl[s, h, sp], po[s, h, sp] = sc.max(), p.sum(dtype=f), (p[:, None] * Vs).sum(axis=0, dtype=f)
    return pm, pl, po


def combine_f32(pm, pl, po, mut=None):
    """launch_attn_combine in numpy float32 (splits in descending order): context [S][n_q][128]."""
    f = np.float32
    if mut == "combine-drops-last-split": pm, pl, po = pm[..., :-1], pl[..., :-1], po[..., :-1, :]
    M = pm.max(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        w = np.where(np.isneginf(pm), f(0), np.exp(pm - M, dtype=f)).astype(f)
    L = (pl[..., ::-1] * w[..., ::-1]).sum(axis=-1, dtype=f)
    return ((po[..., ::-1, :] * w[..., ::-1, None]).sum(axis=-2, dtype=f) / L[..., None]).astype(f)


def combine_reference(pm, pl, po):
    """float64 merge of the partials [S][n_q][ns] a launch wrote, and its bound (decode_kernels_ref.merge_partials)."""
    S, n_q, ns = pm.shape
    x, dx = merge_partials(pm.reshape(S * n_q, ns), pl.reshape(S * n_q, ns), po.reshape(S * n_q, ns, 128))
    return x.reshape(S, n_q, 128), dx.reshape(S, n_q, 128) + 2.0 ** -133


def check_empty_splits(c, d, pm, pl, po):
    """Splits that hold no key of a sequence are (-inf, 0, 0); every live one was written with finite values."""
    for s, pos in enumerate(d["pos"]):
        live = pos // c["keys"] + 1
        assert np.all(np.isneginf(pm[s, :, live:])) and np.all(pl[s, :, live:] == 0) and np.all(po[s, :, live:] == 0), f"sequence {s}: an empty split is not (-inf, 0, 0)"
        assert np.all(np.isfinite(pm[s, :, :live])) and np.all(np.isfinite(pl[s, :, :live])) and np.all(np.isfinite(po[s, :, :live])), f"sequence {s}: a live split was not written"
