"""Segment attention (encoder windows, causal prefill): csrc/k_attn.hip (fp32 VALU) and csrc/k_fattn.hip (the MFMA register-staged
kernel, its KSPLIT = 2 form and the LDS-DMA ring kernel) -- cases, float64 reference, derived per-element bounds and the numpy
restatements of the kernels' plausible mistakes.  Same method and helpers as tests/gemm_ref.py and tests/batched_decode_ref.py.  Shared by
tests/test_seg_attn_ref_host.py (CPU: an honest float32 evaluation, tile by tile in the kernel's order with P rounded to bf16 for the
MFMA forms, lies inside every bound; every applicable mutant outside by a factor of 10; the fattn_block remap is a bijection) and
tests/test_gpu_seg_attn.py (GPU: one launch per case through q3a_selftest_seg_attn_launch, every element of the output buffer compared,
the reported instantiation compared with the case's `form`).

Layouts are the engine's.  Encoder: one [rows][3 D] buffer holds q, k and v interleaved (D = 3 heads x 64), kv_hs = 64, kv_rs = q_rs =
3 D, kv_off = q_row0 3 D, o_rs = D; rows past the last segment hold NaN.  Prefill: q [rows][n_q 128], caches [S][n_kv][max_ctx][128],
kv_hs = max_ctx 128, kv_rs = 128, kv_off = s n_kv max_ctx 128, q_row0 the prefix sum of the lengths; every cache row >= len holds NaN.
PAD q / output rows behind the last segment belong to no segment: q holds NaN there and the output must keep its sentinel.

Loud edge keys.  q = noise + 0.5 w with a sign vector w per K/V head; the keys at 31, 32, 63, 64, len - 1 and the first key of the last
32-key tile are K = BETA w + 0.25 noise -- a score about 4.5 above a typical one for every query of the group -- with V four times as
loud, so one lost, extra or misplaced key moves the output by far more than the rounding of P.

Bounds (u = 2^-24), the rule of DESIGN section 5.  K, V and q16 are exact bf16 values, so no operand rounding enters.
    score error     e_s = (HD + 2) u max_j sum_d |k_jd||q_d| / scale + 8 u (max_j |s_j - m| + 2)   (batched_decode_ref.attn_context's form)
    fp32 q -> bf16  + max_j sum_d |k_jd| half_ulp_bf16(q_d) / scale inside e_s (the MFMA kernels round an fp32 q once)
    v_exp_f32       + 2 u inside e_s: 1 ulp ASSUMED for the hardware exponential, as gemm_ref.silu_step assumes
    output          (2 e_s + 2 (n + 64) u) sum_j p_j |v_jd| / sum_j p_j
    P as bf16       + 2^-8 sum_j p_j |v_jd| / sum_j p_j (MFMA): the row sum l is taken from the unrounded p, so the rounding does not cancel
    bf16 output     gemm_ref.bf16_out_bound
Three mistakes the issue lists cannot leave this bound by a factor of 10 on any data, by arithmetic, and are not in MUTANTS: P not
rounded (closer to the reference than the kernel) and P truncated (at most one bf16 ulp = twice the P term); an empty KSPLIT half taken
as m = 0 (its l and O are 0, so the factor it changes multiplies numerator and denominator alike); the first tile past wave_qmax consumed
(it goes through the masked path: every score -inf, every p 0, alpha 1).

Worst excess (|got - ref| / bound, <= 1 passes) on an MI355X, printed by tests/test_gpu_seg_attn.py:
    family                                               fp32 out                bf16 out
    fattn_dma_kernel HD 64 (encoder), NS 3 and 4         0.733                   0.757
    fattn_dma_kernel HD 128, GROUP 1 / 2 / 4             0.804 / 0.906 / 0.822   0.746 / 0.792 / 0.856
    fattn_dma_kernel GROUP 4, grids of 1 .. 27           0.496 .. 0.834          -
    fattn_kernel with q16 (Q3A_FATTN_DMA=0)              0.733; 0.804 / 0.906 / 0.822 (the DMA kernel's cases)
    fattn_kernel KSPLIT 2, q16 / fp32 q                  0.705 / 0.109           0.824 / -
    fattn_kernel behind fp32 q, GROUP 1 / 2 / 4          0.100 / 0.133 / 0.150   0.111 / 0.150 / 0.161   (the bound carries the rounding of q)
    fattn_kernel fp32 K/V, fp32 q (encoder)              0.065                   0.109
    attn_kernel HD 64                                    0.018                   -
    attn_kernel HD 128, GROUP 1 / 2 / 4, either cache    0.012 / 0.017 / 0.015   -
The P term is a half-ulp bound: the MFMA kernels with exact operands sit near it by construction (the honest float32 restatement reaches
0.906 on the same case).  Every case reported the form its table entry states, NS = 4 reproduced the NS = 3 bits, every bit-identity held.
"""
import numpy as np

from batched_decode_ref import buffer_excess
from decode_kernels_ref import U, _rng, bf16_round
from gemm_ref import SENT16, SENT32, bf16_out_bound, decode, half_ulp_bf16

PAD = 32            # q / output rows behind the last segment: a store for a query >= len of the last 32-query tile lands there
MAX_CTX = 256
ENC_LENS = (1, 31, 32, 33, 64, 65, 104, 128, 129, 200)
FORM_FIELDS = ("mfma", "dma", "hd", "group", "causal", "kv_f32", "ksplit", "ns", "qpw", "grid_x", "grid_y", "grid_z")


def _form(kind, hd, group, kv_f32=0, ksplit=1, qpw=0):
    """What the launcher must report: kind "dma" (fattn_dma_kernel, NS 3 unless the knob says 4), "staged" (fattn_kernel), "valu"."""
    return dict(mfma=int(kind != "valu"), dma=int(kind == "dma"), hd=hd, group=group, causal=int(hd == 128), kv_f32=kv_f32, ksplit=ksplit,
                ns=3 if kind == "dma" else 0, qpw=qpw)


def _enc(name, launcher, q, kv, form):
    return dict(name=name, launcher=launcher, layout="enc", hd=64, n_kv=3, group=1, lens=ENC_LENS, q=q, kv=kv, form=form, data="enc")


def _pre(name, launcher, group, n_kv, lens, q, kv, form, data=None):
    return dict(name=name, launcher=launcher, layout="pre", hd=128, n_kv=n_kv, group=group, lens=tuple(lens), q=q, kv=kv, form=form,
                data=data or f"pre-{group}-{n_kv}-" + "-".join(map(str, lens)))


DMA_LENS, STAGED_LENS, VALU_LENS, KSPLIT_LENS = (1, 32, 33, 97, 128, 129, 230), (1, 33, 97, 129), (1, 33, 64, 65, 129), (1, 32, 33, 64, 65, 97)
# q: "q16" bf16 q, "f32" fp32 q (not bf16-representable: the MFMA kernels round it), "f32x" fp32 q holding bf16 values;
# kv: "bf16" / "f32" (fp32 buffers hold bf16 values: the relations between the two forms are bit for bit)
CASES = [
    # 60 workgroups (60 % 8 = 4): n_tiles 1 .. 7, stage 0 of the three refilled twice; the HD 64 swizzles; a second 128-query block
    _enc("enc-dma", 2, "q16", "bf16", _form("dma", 64, 1)),
    _enc("enc-staged-f32", 2, "f32", "f32", _form("staged", 64, 1, kv_f32=1)),
    _enc("enc-valu", 0, "f32", "f32", _form("valu", 64, 1, kv_f32=1, qpw=8)),
    # per-block n_tiles 1 .. 8, full against masked tiles, the diagonal in the last tile, QT = 128 / 64 / 32
    _pre("pre-dma-g1", 3, 1, 2, DMA_LENS, "q16", "bf16", _form("dma", 128, 1)),
    _pre("pre-dma-g2", 3, 2, 8, DMA_LENS, "q16", "bf16", _form("dma", 128, 2)),       # ceil(230 / 64) 8 7 = 224 >= 128: not KSPLIT
    _pre("pre-dma-g4", 3, 4, 2, DMA_LENS, "q16", "bf16", _form("dma", 128, 4)),
    # ceil(97 / 64) 2 6 = 24 < 128: half 1 empty for every query (1, 32), for all but one (33), for some (64 .. 97)
    _pre("pre-ksplit", 3, 2, 2, KSPLIT_LENS, "q16", "bf16", _form("staged", 128, 2, ksplit=2)),
    _pre("pre-ksplit-f32q", 3, 2, 2, KSPLIT_LENS, "f32", "bf16", _form("staged", 128, 2, ksplit=2)),
    # fp32 q: the register-staged kernels as the launcher's fallback (group 2: ceil(129 / 64) 11 4 = 132 >= 128)
    _pre("pre-staged-g1", 3, 1, 2, STAGED_LENS, "f32", "bf16", _form("staged", 128, 1)),
    _pre("pre-staged-g2", 3, 2, 11, STAGED_LENS, "f32", "bf16", _form("staged", 128, 2)),
    _pre("pre-staged-g4", 3, 4, 2, STAGED_LENS, "f32", "bf16", _form("staged", 128, 4)),
] + [
    _pre(f"pre-valu-g{g}-{kv}", 1, g, 2, VALU_LENS, "f32", kv, _form("valu", 128, g, kv_f32=int(kv == "f32"), qpw=2 if g == 4 else 4), data=f"pre-valu-{g}")
    for g in (1, 2, 4) for kv in ("f32", "bf16")
] + [
    # max_len 64 above the longest segment: a column of workgroups that return at once
    dict(_pre("pre-dma-g1-max_len+64", 3, 1, 2, DMA_LENS, "q16", "bf16", _form("dma", 128, 1)), max_len=230 + 64),
]
BY_NAME = {c["name"]: c for c in CASES}

# The fattn_block bijection on the device: sub-launches of one data set (group 4: 32-query tiles) with n_segs x n_kv x tiles =
# 1, 7, 8, 9, 27 workgroups, every one of them with work.  (segments of GRID_LENS, K/V heads, expected grid)
GRID_LENS = (20, 96, 70, 224, 230)
GRIDS = [((0,), 1, (1, 1, 1)), ((3,), 1, (7, 1, 1)), ((4,), 1, (8, 1, 1)), ((1,), 3, (3, 3, 1)), ((1, 2, 0), 3, (3, 3, 3))]
GRID_BASE = _pre("grids", 3, 4, 3, GRID_LENS, "q16", "bf16", _form("dma", 128, 4))


def sub_case(c, segs, n_kv=None, **kw):
    """The same data, only the segments `segs` (in that order) and the first n_kv K/V heads: another q_row0 / kv_off for each."""
    return dict(c, name=c["name"] + "/" + ",".join(map(str, segs)) + (f"/kv{n_kv}" if n_kv else ""), segs=tuple(segs), sub_kv=n_kv, **kw)


def grid_cases():
    return [sub_case(GRID_BASE, segs, n_kv) for segs, n_kv, _ in GRIDS]


def variant(c, **kw):
    return dict(c, name=c["name"] + "/" + ",".join(f"{k}={v}" for k, v in kw.items()), **kw)


def n_kv_of(c):
    return c.get("sub_kv") or c["n_kv"]


def seg_ids(c):
    return c.get("segs") or tuple(range(len(c["lens"])))


def lens_of(c):
    return [c["lens"][s] for s in seg_ids(c)]


def mfma(c):
    return c["launcher"] >= 2


def causal(c):
    return c["layout"] == "pre"


def scale_of(c):
    return float(np.sqrt(c["hd"]))


def kt_of(c):
    return 32 if mfma(c) else 64


def q_rounded(c):
    """The MFMA kernels round an fp32 q that is not bf16-representable."""
    return mfma(c) and c["q"] == "f32"


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
ALPHA, LOUD_SCORE = 0.5, 4.5
_data = {}


def loud_keys(L):
    return sorted({j for j in (31, 32, 63, 64, L - 1, 32 * ((L - 1) // 32)) if 0 <= j < L})


def inputs(c):
    """Per segment of c["lens"]: q [L][n_q][hd] fp32, k / v [n_kv][L][hd] fp32 holding bf16 values.  Keyed by c["data"]: the forms that
    must agree bit for bit run on the same numbers ("f32x" / "q16" cases read bf16(q))."""
    key = c["data"]
    if key not in _data:
        r = _rng("seg-attn-" + key)
        hd, n_kv, G = c["hd"], c["n_kv"], c["group"]
        beta = LOUD_SCORE / (ALPHA * np.sqrt(hd))
        q, k, v = [], [], []
        for L in c["lens"]:
            w = np.where(r.uniform(size=(n_kv, hd)) < 0.5, -1.0, 1.0)
            qs = r.normal(0, 1, (L, n_kv * G, hd)) + ALPHA * np.repeat(w, G, axis=0)[None]
            ks, vs = r.normal(0, 1, (n_kv, L, hd)), r.normal(0, 1, (n_kv, L, hd))
            for j in loud_keys(L):   # (a segment of one key: against w, a score of -4.5 -- next to it a zero row admitted at `len` owns the softmax)
                ks[:, j] = (beta if L > 1 else -beta) * w + 0.25 * r.normal(0, 1, (n_kv, hd))
                vs[:, j] *= 4
            q.append(qs.astype(np.float32)); k.append(bf16_round(ks.astype(np.float32))); v.append(bf16_round(vs.astype(np.float32)))
        _data[key] = dict(q=q, k=k, v=v)
    d = _data[key]
    if c["q"] != "f32":
        return dict(d, q=[bf16_round(x) for x in d["q"]])
    return dict(d)


def bits16(a):
    """fp32 holding bf16 values (or NaN) -> bf16 bit patterns."""
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def pack(c, d, out16=False):
    """The arrays and scalars of one q3a_selftest_seg_attn_launch call (fp32 values; the caller converts q16 / bf16 K/V with bits16)."""
    hd, G, n_kv, ids = c["hd"], c["group"], n_kv_of(c), seg_ids(c)
    lens = lens_of(c)
    n_q, rows = n_kv * G, sum(lens) + PAD
    row0 = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    pk = dict(row0=row0, lens=np.asarray(lens, np.int32), rows=rows, n_kv=n_kv, max_len=c.get("max_len", max(lens)))
    if c["layout"] == "enc":
        D = n_q * hd
        buf = np.full((rows, 3 * D), np.nan, np.float32)
        for i, s in enumerate(ids):
            sl = slice(row0[i], row0[i] + lens[i])
            buf[sl, :D] = d["q"][s][:, :n_q].reshape(lens[i], D)
            buf[sl, D:2 * D] = d["k"][s][:n_kv].transpose(1, 0, 2).reshape(lens[i], D)
            buf[sl, 2 * D:] = d["v"][s][:n_kv].transpose(1, 0, 2).reshape(lens[i], D)
        pk.update(q=buf, k=buf, v=buf, q_rs=3 * D, kv_off=row0.astype(np.int64) * 3 * D, k_base=D, v_base=2 * D, kv_hs=hd, kv_rs=3 * D, o_rs=D)
    else:
        qb = np.full((rows, n_q * hd), np.nan, np.float32)
        kc = np.full((len(ids), n_kv, MAX_CTX, hd), np.nan, np.float32)
        vc = kc.copy()
        for i, s in enumerate(ids):
            qb[row0[i]:row0[i] + lens[i]] = d["q"][s][:, :n_q].reshape(lens[i], n_q * hd)
            kc[i, :, :lens[i]], vc[i, :, :lens[i]] = d["k"][s][:n_kv], d["v"][s][:n_kv]
        pk.update(q=qb, k=kc, v=vc, q_rs=n_q * hd, kv_off=np.arange(len(ids), dtype=np.int64) * n_kv * MAX_CTX * hd, k_base=0, v_base=0,
                  kv_hs=MAX_CTX * hd, kv_rs=hd, o_rs=n_q * hd)
    pk["out"] = np.full((rows, pk["o_rs"]), SENT16 if out16 else SENT32, np.uint16 if out16 else np.uint32)
    return pk


def launch(lib, c, d, out16=False, pk=None):
    """One q3a_selftest_seg_attn_launch of the case (pk: buffers other than pack()'s).  (raw output buffer, reported form as a dict), or
    (None, the error message) when the call was refused."""
    import ctypes as C
    pk = pk or pack(c, d, out16)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    kv_f32 = c["kv"] == "f32"
    if c["layout"] == "enc":      # one buffer, bf16 or fp32 as a whole
        buf = f32(pk["q"]) if kv_f32 else np.ascontiguousarray(bits16(pk["q"]))
        q, q16, k, v = (buf, None, buf, buf) if kv_f32 else (None, buf, buf, buf)
    else:
        q, q16 = (None, np.ascontiguousarray(bits16(pk["q"]))) if c["q"] == "q16" else (f32(pk["q"]), None)
        k, v = (f32(pk["k"]), f32(pk["v"])) if kv_f32 else (np.ascontiguousarray(bits16(pk["k"])), np.ascontiguousarray(bits16(pk["v"])))
    out = np.ascontiguousarray(pk["out"]).copy()
    form = np.full(len(FORM_FIELDS), -1, np.int32)
    row0, lens, off = (np.ascontiguousarray(pk[x]) for x in ("row0", "lens", "kv_off"))
    rc = lib.q3a_selftest_seg_attn_launch(0, c["launcher"], int(kv_f32), c["group"], ptr(row0), ptr(lens), ptr(off), len(lens), int(pk["max_len"]),
                                          ptr(q), ptr(q16), pk["rows"], pk["q_rs"], ptr(k), ptr(v), k.size, pk["k_base"], pk["v_base"], pk["kv_hs"],
                                          pk["kv_rs"], pk["n_kv"], scale_of(c), None if out16 else ptr(out), ptr(out) if out16 else None,
                                          out.shape[0], pk["o_rs"], ptr(form))
    if rc != 0:
        return None, (lib.q3a_last_error(None) or b"").decode()
    return out, dict(zip(FORM_FIELDS, form.tolist()))


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference and bound
# ---------------------------------------------------------------------------------------------------------------------
def _mask(c, L, n_keys=None):
    qi, kj = np.arange(L)[:, None], np.arange(n_keys or L)[None, :]
    return (kj < L) & ((kj <= qi) if causal(c) else True)


def reference(c, d, out16=False):
    """(ref, bound): the whole output buffer [rows][o_rs] in float64, NaN where nothing may be written (bound 1 there)."""
    hd, G, n_kv, scale = c["hd"], c["group"], n_kv_of(c), scale_of(c)
    lens = lens_of(c)
    n_q, rows = n_kv * G, sum(lens) + PAD
    ref, bound = np.full((rows, n_q * hd), np.nan), np.ones((rows, n_q * hd))
    r0 = 0
    for s, L in zip(seg_ids(c), lens):
        q = d["q"][s][:, :n_q].astype(np.float64).transpose(1, 0, 2)                     # [n_q][L][hd]
        K, V = (np.repeat(d[x][s][:n_kv].astype(np.float64), G, axis=0) for x in ("k", "v"))   # [n_q][L][hd]
        valid = _mask(c, L)[None]
        sc = np.where(valid, q @ K.transpose(0, 2, 1) / scale, -np.inf)
        m = sc.max(axis=2, keepdims=True)
        p = np.exp(sc - m)
        den = p.sum(axis=2, keepdims=True)
        out, absv = p @ V / den, p @ np.abs(V) / den
        ds = (hd + 2) * U * (np.abs(q) @ np.abs(K).transpose(0, 2, 1))
        if q_rounded(c):
            ds = ds + half_ulp_bf16(q) @ np.abs(K).transpose(0, 2, 1)
        ds = np.where(valid, ds, 0.0).max(axis=2, keepdims=True) / scale
        spread = np.where(valid, m - sc, 0.0).max(axis=2, keepdims=True)
        e_s = ds + 8 * U * (spread + 2) + (2 * U if mfma(c) else 0.0)
        b = (2 * e_s + 2 * (L + 64) * U + (2.0 ** -8 if mfma(c) else 0.0)) * absv + 2.0 ** -133
        ref[r0:r0 + L] = out.transpose(1, 0, 2).reshape(L, n_q * hd)
        bound[r0:r0 + L] = b.transpose(1, 0, 2).reshape(L, n_q * hd)
        r0 += L
    if out16:
        bound = np.where(np.isnan(ref), 1.0, bf16_out_bound(np.nan_to_num(ref), bound))
    return ref, bound


def excess(c, d, got, out16=False):
    """Worst |got - ref| / bound of a decoded output buffer (inf: a written element is not finite, or a sentinel is gone)."""
    return buffer_excess(got, *reference(c, d, out16))


def excess_by_segment(c, d, got, out16=False):
    ref, bound = reference(c, d, out16)
    ends = np.cumsum(lens_of(c))
    return [buffer_excess(got[e - L:e], ref[e - L:e], bound[e - L:e]) for e, L in zip(ends, lens_of(c))]


# ---------------------------------------------------------------------------------------------------------------------
# the launch in numpy: honest float32 in the kernel's order, or float64 with one mistake
# ---------------------------------------------------------------------------------------------------------------------
MUTANTS = ["causal-lt", "causal-le+1", "tail-key-dropped", "len-key-clamped", "len-key-zero-row", "full-on-diagonal-tile",
           "v-keys-permuted-in-tile", "k-dims-chunk-rotated", "gqa-other-head-q", "wrong-kv-head", "kv-off-neighbour", "q-row0-neighbour",
           "scale-squared", "ksplit-half1-dropped", "ksplit-merge-swapped", "rescale-skipped-single", "rows-past-len-written",
           "bf16-out-at-fp32-offsets"]


def applies(c, m, out16=False):
    f = c["form"]
    return {"causal-lt": causal(c), "causal-le+1": causal(c), "len-key-clamped": not causal(c), "len-key-zero-row": not causal(c),
            "full-on-diagonal-tile": causal(c) and mfma(c), "v-keys-permuted-in-tile": mfma(c), "k-dims-chunk-rotated": mfma(c),
            "gqa-other-head-q": c["group"] > 1, "wrong-kv-head": n_kv_of(c) > 1, "kv-off-neighbour": len(seg_ids(c)) > 1,
            "q-row0-neighbour": len(seg_ids(c)) > 1, "ksplit-half1-dropped": f["ksplit"] == 2, "ksplit-merge-swapped": f["ksplit"] == 2,
            # a wave that holds one query alone, behind at least one tile; a last 32-query tile with room behind the segment
            "rescale-skipped-single": causal(c) and mfma(c) and any(L > 32 and L % 32 == 1 for L in lens_of(c)),
            "rows-past-len-written": any(L % 32 for L in lens_of(c)), "bf16-out-at-fp32-offsets": out16}.get(m, True)


def _fit(a, L):
    """Rows 0 .. L - 1 of a [..][rows][hd] array; NaN where it has fewer (what a cache holds behind another segment's last row)."""
    if a.shape[-2] >= L:
        return a[..., :L, :]
    return np.concatenate([a, np.full(a.shape[:-2] + (L - a.shape[-2], a.shape[-1]), np.nan, a.dtype)], axis=-2)


def _flash(c, q, K, V, valid, dt, mut, keys=None):
    """Online softmax over key tiles of kt_of(c): (m [H][L], l [H][L], O [H][L][hd]) in dt.  keys: the key indices this pass sees."""
    H, L, hd = q.shape
    KT, scale = kt_of(c), dt(scale_of(c) ** (2 if mut == "scale-squared" else 1))
    m, l, O = np.full((H, L), -np.inf, dt), np.zeros((H, L), dt), np.zeros((H, L, hd), dt)
    n = K.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, n, KT):
            sel = np.arange(k0, min(k0 + KT, n))
            if keys is not None:
                sel = sel[np.isin(sel, keys)]
            if sel.size == 0 or not valid[:, sel].any():
                continue
            sc = np.where(valid[None, :, sel], (q @ K[:, sel].transpose(0, 2, 1)).astype(dt) / scale, dt(-np.inf))
            m_new = np.maximum(m, sc.max(axis=2))
            dead = np.isneginf(m_new)             # nothing visible yet for this query
            alpha = np.where(dead, 1, np.exp(m - m_new)).astype(dt)
            p = np.where(dead[..., None], 0, np.exp(sc - m_new[..., None])).astype(dt)
            l = (l * alpha + p.sum(axis=2, dtype=dt)).astype(dt)
            o_scale = alpha
            if mut == "rescale-skipped-single":   # per wave of 32 queries: the running output keeps its scale when one query alone saw a new maximum
                saw = (m_new > m)
                pad = (-L) % 32
                cnt = np.pad(saw, ((0, 0), (0, pad))).reshape(H, -1, 32).sum(axis=2)
                one = np.repeat(cnt == 1, 32, axis=1)[:, :L]
                o_scale = np.where(one, dt(1), alpha)
            if mfma(c):
                p = bf16_round(p.astype(np.float32)).astype(dt)
            O = (O * o_scale[..., None] + p @ V[:, sel]).astype(dt)
            m = m_new
    return m, l, O


def sim(c, d, mut=None, honest=False, out16=False):
    """The launch on the data: the decoded output buffer (NaN where nothing is written)."""
    dt = np.float32 if honest else np.float64
    hd, G, n_kv = c["hd"], c["group"], n_kv_of(c)
    ids, lens = seg_ids(c), lens_of(c)
    n_q, rows = n_kv * G, sum(lens) + PAD
    out = np.full((rows, n_q * hd), np.nan)
    staged_zero = not (c["form"]["dma"])     # rows past the segment: zero-filled (register-staged, VALU) or the last row again (DMA)
    r0 = 0
    for i, (s, L) in enumerate(zip(ids, lens)):
        nb = ids[(i + 1) % len(ids)]
        qsrc = d["q"][nb if mut == "q-row0-neighbour" else s][:, :n_q]
        q = _fit(qsrc.transpose(1, 0, 2), L)                                   # [n_q][L][hd]
        if q_rounded(c): q = bf16_round(q)
        if mut == "gqa-other-head-q": q = q[np.arange(n_q) ^ 1]
        ksrc, vsrc = (d[x][nb if mut == "kv-off-neighbour" else s][:n_kv] for x in ("k", "v"))
        kvh = np.arange(n_q) // G
        if mut == "wrong-kv-head": kvh = (kvh + 1) % n_kv
        Lp = (L + 63) // 64 * 64
        K, V = _fit(ksrc, L)[kvh], _fit(vsrc, L)[kvh]
        tail = np.zeros((n_q, Lp - L, hd), np.float32) if staged_zero else np.repeat(K[:, L - 1:L], Lp - L, axis=1)
        tailv = np.zeros((n_q, Lp - L, hd), np.float32) if staged_zero else np.repeat(V[:, L - 1:L], Lp - L, axis=1)
        if mut == "len-key-clamped": tail, tailv = np.repeat(K[:, L - 1:L], Lp - L, axis=1), np.repeat(V[:, L - 1:L], Lp - L, axis=1)
        if mut == "len-key-zero-row": tail, tailv = np.zeros((n_q, Lp - L, hd), np.float32), np.zeros((n_q, Lp - L, hd), np.float32)
        K, V = np.concatenate([K, tail], axis=1), np.concatenate([V, tailv], axis=1)
        if mut == "v-keys-permuted-in-tile":     # the transpose-read map: key r of a tile from row r ^ 5
            V = V[:, np.arange(Lp) ^ 5]
        if mut == "k-dims-chunk-rotated":        # the swizzle: 16-byte chunk c from chunk c + 1
            K = np.roll(K, -8, axis=2)
        qi, kj = np.arange(L)[:, None], np.arange(Lp)[None, :]
        valid = _mask(c, L, Lp)
        if mut == "causal-lt": valid = (kj < L) & (kj < qi)
        if mut == "causal-le+1": valid = (kj < L) & (kj <= qi + 1)
        if mut == "tail-key-dropped": valid = valid & (kj < L - 1)
        if mut in ("len-key-clamped", "len-key-zero-row"): valid = kj <= L
        if mut == "full-on-diagonal-tile":       # no mask on the tile that holds the wave's first query
            valid = valid | (kj // 32 == qi // 32)
        valid = np.broadcast_to(valid, (L, Lp)) & (kj < Lp)
        q, K, V = q.astype(dt), K.astype(dt), V.astype(dt)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if c["form"]["ksplit"] == 2:
                h0, h1 = (np.arange(Lp)[(np.arange(Lp) // 32) % 2 == h] for h in (0, 1))
                m1, l1, O1 = _flash(c, q, K, V, valid, dt, mut, h0)
                m2, l2, O2 = _flash(c, q, K, V, valid, dt, mut, h1)
                if mut == "ksplit-half1-dropped": m2, l2, O2 = np.full_like(m2, -np.inf), np.zeros_like(l2), np.zeros_like(O2)
                mn = np.maximum(m1, m2)
                f1 = np.where(np.isfinite(m1), np.exp(m1 - mn), 0).astype(dt)
                f2 = np.where(np.isfinite(m2), np.exp(m2 - mn), 0).astype(dt)
                if mut == "ksplit-merge-swapped": f1, f2 = f2, f1
                l, O = (l1 * f1 + l2 * f2).astype(dt), (O1 * f1[..., None] + O2 * f2[..., None]).astype(dt)
            else:
                _, l, O = _flash(c, q, K, V, valid, dt, mut)
            res = (O * (dt(1) / l)[..., None]).astype(dt)
        out[r0:r0 + L] = res.transpose(1, 0, 2).reshape(L, n_q * hd)
        if mut == "rows-past-len-written":
            out[r0 + L:min(r0 + (L + 31) // 32 * 32, rows)] = 0.0
        r0 += L
    if out16:
        out = np.where(np.isnan(out), np.nan, bf16_round(np.nan_to_num(out).astype(np.float32)).astype(np.float64))
        if mut == "bf16-out-at-fp32-offsets":
            flat = np.full(out.size, np.nan)
            flat[::2] = out.ravel()[:(out.size + 1) // 2]
            out = flat.reshape(out.shape)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# fattn_block (k_fattn.hip), restated: workgroup -> (query tile, K/V head, segment)
# ---------------------------------------------------------------------------------------------------------------------
def fattn_block(gx, gy, gz):
    """The triple each workgroup of a gx x gy x gz grid takes: [total][3]."""
    total = gx * gy * gz
    lin = np.arange(total)
    xcd, loc, q, r = lin & 7, lin >> 3, total >> 3, total & 7
    idx = np.where(xcd < r, xcd * (q + 1), r * (q + 1) + (xcd - r) * q) + loc
    return np.stack([idx % gx, (idx // gx) % gy, idx // gx // gy], axis=1)
