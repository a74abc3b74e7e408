"""float64 references, derived per-element bounds and the cases of the one-sequence decode kernels (csrc/k_gemv.hip, k_dattn.hip,
k_decode.hip argmax_finalize), as q3a_selftest_gemv_launch / q3a_selftest_decode_attn_launch run them.

What these tests guard is the marshalling of kernel arguments (a flat, preloaded head and a tail struct per kernel): a swapped pointer
pair, a field read from the wrong place, an offset off by one.  Such an error is not small, so the inputs are built to make every
argument matter -- bias and residual of order 1, a norm weight away from 1, an eps that moves rstd, weight rows correlated with the
activations so that a dot product is far from a random walk -- and tests/test_decode_kernels_ref_host.py shows on the CPU that an
honest fp32 evaluation in another summation order stays inside each bound while every listed single-argument mutant leaves it by a
factor of at least 100.

Bounds (u = 2^-24; Higham, Accuracy and Stability of Numerical Algorithms, 3.1: a length-n fp32 sum of products, any order, any fusing,
errs by at most gamma_n sum |terms|, gamma_n ~ n u):
  GEMV       gamma = (K + 16) u;  bound_n = 4 gamma (|rstd| sum_k |W_nk x_k g_k| + |bias_n| + |resid_n|).  The 16 covers the wave tree and
             the epilogue; the factor 4 covers the second length-K sum inside the norm scale (rstd's relative error <= gamma, it
             multiplies the dot product) and the final adds.
  GLU        gate G and up U with bounds bG, bU: out = silu(G) U, |silu'| <= 1.1, so
             bound = 1.1 bG |U| + |silu(G)| bU + 1.1 bG bU + 16 u |silu(G) U| (the last term: expf, the division and the product).
  merged x   x_k = sum_s f_s o_sk / L, f_s = exp(m_s - M), L = sum_s l_s f_s: each f_s has relative error <= e = 4 u (|m_s - M| + 2)
             (expf and the subtraction), numerator and denominator sums add (ns + 4) u: dx_k = (2 e_max + 2 (ns + 4) u) sum_s f_s |o_sk| / L,
             and the GEMV bound gains sum_k |W_nk| dx_k.
  attention  scores s_j = q . k_j / scale: ds_j = gamma_q sum_d |q_d k_jd| / scale with gamma_q = (128 + 32) u (the 128-term dot and the
             roundings of the per-head norm and RoPE that made q; the bf16 cache runs the default arithmetic: hardware rsq, 1 ulp);
             p_j = exp(s_j - m) has relative error e_j = 2 ds_max + 8 u (|s_j - m| + 2) (the hardware exponential of the bf16-cache
             form: 2 ulp after an argument scaled by log2 e); the context c_d = sum_j p_j v_jd / sum_j p_j over at most max_ctx keys,
             summed per lane, per wave, per split and merged: bound_d = (2 e_max + 2 (keys + 64) u) sum_j p_j |v_jd| / sum_j p_j.
             The merged, normalised context is compared, so the check does not depend on which maximum a split chose.
  new k / v  the appended cache rows are bf16 roundings of fp32 values: |row - exact| <= bf16 half-ulp(exact) + gamma_q |exact| (a value
             next to a rounding boundary may round either way); the context reference then uses the row the launch appended.
"""
import numpy as np

U = 2.0 ** -24
SENTINEL = np.float32(-7777.25)


def bf16_round(a):
    """fp32 -> nearest-even bf16, returned as fp32."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def bf16_bits(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_half_ulp(a):
    a = np.abs(np.asarray(a, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (e - 8)


def silu(x):
    return x / (1.0 + np.exp(-x))


# ---- one-sequence GEMV -------------------------------------------------------------------------------------------------------
# K, N, mode (0 store, 1 + resid, 2 GLU, 3 lm_head), rms (fused norm), bias; form = what launch_gemv picks (k_gemv.hip launch1k)
GEMV_CASES = [
    dict(name="a-xl-bias-void-last-block", K=1024, N=4098, mode=0, rms=True, bias=True),   # XL form; 2 rows per wave, the last block partly void
    dict(name="b-xl-kin-false", K=1016, N=36, mode=0, rms=True, bias=False),                # columns 1016..1023 clamped on the last lanes; 1 row per wave
    dict(name="c-norm-k2048", K=2048, N=4096, mode=0, rms=True, bias=False),                # the non-XL norm form
    dict(name="d-glu-bias", K=1024, N=2 * 96, mode=2, rms=True, bias=True),                 # row interleave [16 gate | 16 up]
    dict(name="e-resid-ki6", K=3072, N=70, mode=1, rms=False, bias=False),                  # KI 6
    dict(name="f-plain-ki12", K=6144, N=40, mode=0, rms=False, bias=False),                 # KI 12
]
# attention partials as x (o_proj: K = 16 heads x 128, mode 1): splits -> MF 4 with a clamped empty slot, MF 8, the chunked form
ATTN_GEMV_CASES = [
    dict(name="attn-3-splits-mf4", K=2048, N=70, heads=16, nsplit=3, empty=None),
    dict(name="attn-5-splits-mf8", K=2048, N=70, heads=16, nsplit=5, empty=None),
    dict(name="attn-9-splits-chunked", K=2048, N=70, heads=16, nsplit=9, empty=None),
    dict(name="attn-3-splits-last-empty", K=2048, N=70, heads=16, nsplit=3, empty=2),     # m = -inf, l = 0, o = 0 in the last split
]
EPS = 0.5  # moves rstd by tens of per cent against eps = 0


def _rng(name):
    return np.random.default_rng(sum(map(ord, name)) * 7919 + 13)  # (a seed from the case's name, the same in every process)


def gemv_inputs(c):
    r = _rng(c["name"])
    K, N = c["K"], c["N"]
    x = r.normal(0, 1, K).astype(np.float32)
    g = (1.5 + 0.5 * r.uniform(-1, 1, K)).astype(np.float32) if c["rms"] else None
    # rows correlated with the activations: W_nk = (noise + a_n sign(x_k)) 4 / K, so |y_n| is a fixed share of sum |terms| and both are
    # of order 1 at every K (bias and residual stay visible next to them)
    a = r.uniform(-1, 1, (N, 1))
    W = bf16_round(((r.normal(0, 1, (N, K)) + a * np.sign(x)) * (4.0 / K)).astype(np.float32))
    sgn = lambda n: np.where(r.uniform(size=n) < 0.5, -1.0, 1.0)
    bias = (sgn(N) * r.uniform(1, 2, N)).astype(np.float32) if c["bias"] else None
    resid = (sgn(N) * r.uniform(1, 2, N)).astype(np.float32) if c["mode"] == 1 else None
    return dict(W=W, x=x, g=g, bias=bias, resid=resid, eps=EPS if c["rms"] else 0.0)


def attn_gemv_inputs(c):
    r = _rng(c["name"])
    K, N, H, ns = c["K"], c["N"], c["heads"], c["nsplit"]
    pm = r.normal(0, 2, (H, ns)).astype(np.float32)
    pl = r.uniform(1, 50, (H, ns)).astype(np.float32)
    po = (r.normal(0, 1, (H, ns, 128)) * pl[:, :, None]).astype(np.float32)
    if c["empty"] is not None:
        pm[:, c["empty"]] = -np.inf; pl[:, c["empty"]] = 0; po[:, c["empty"]] = 0
    else:  # the last split carries weight in every head (a merge that stops one split short must show)
        pm[:, -1] = pm.max(axis=1) + 0.5
    x64, _ = merge_partials(pm, pl, po)
    a = r.uniform(-1, 1, (N, 1))
    W = bf16_round(((r.normal(0, 1, (N, K)) + a * np.sign(x64.ravel())) * (4.0 / K)).astype(np.float32))
    resid = (np.where(r.uniform(size=N) < 0.5, -1.0, 1.0) * r.uniform(1, 2, N)).astype(np.float32)
    return dict(W=W, pm=pm, pl=pl, po=po, resid=resid)


def merge_partials(pm, pl, po):
    """fp64 merge of flash-decoding partials [H][ns], [H][ns], [H][ns][128] -> context [H][128] and its bound."""
    pm, pl, po = (np.asarray(v, np.float64) for v in (pm, pl, po))
    ns = pm.shape[1]
    M = pm.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        f = np.where(np.isneginf(pm), 0.0, np.exp(pm - M))
        e = np.where(np.isneginf(pm), 0.0, 4 * U * (np.abs(pm - M) + 2)).max()
    L = (pl * f).sum(axis=1, keepdims=True)
    x = (po * f[:, :, None]).sum(axis=1) / L
    dx = (2 * e + 2 * (ns + 4) * U) * (np.abs(po) * f[:, :, None]).sum(axis=1) / L
    return x, dx


def gemv_reference(c, d):
    """(ref, bound) in float64 of a GEMV_CASES / ATTN_GEMV_CASES entry on inputs d; GLU: [N / 2] outputs."""
    W = d["W"].astype(np.float64)
    K, N = W.shape[1], W.shape[0]
    gam = (K + 16) * U
    if "po" in d:
        x, dx = merge_partials(d["pm"], d["pl"], d["po"])
        x, dx = x.ravel(), dx.ravel()
        y = W @ x + d["resid"]
        return y, 4 * gam * (np.abs(W) @ np.abs(x) + np.abs(d["resid"])) + np.abs(W) @ dx
    x = d["x"].astype(np.float64)
    rstd, xg = 1.0, x
    if d["g"] is not None:
        rstd = 1.0 / np.sqrt((x * x).mean() + d["eps"])
        xg = x * d["g"]
    b = d["bias"].astype(np.float64) if d["bias"] is not None else np.zeros(N)
    rs = d["resid"].astype(np.float64) if d["resid"] is not None else np.zeros(N)
    y = rstd * (W @ xg) + b + rs
    bound = 4 * gam * (rstd * (np.abs(W) @ np.abs(xg)) + np.abs(b) + np.abs(rs))
    if c.get("mode") == 2:
        gi, ui = glu_rows(N)
        G, Uv, bG, bU = y[gi], y[ui], bound[gi], bound[ui]
        out = silu(G) * Uv
        return out, 1.1 * bG * np.abs(Uv) + np.abs(silu(G)) * bU + 1.1 * bG * bU + 16 * U * np.abs(out)
    return y, bound


def glu_rows(N):
    """weight rows of gate_j and up_j, j < N / 2: rows come in [16 gate | 16 up] blocks."""
    j = np.arange(N // 2)
    g = (j // 16) * 32 + j % 16
    return g, g + 16


GEMV_MUTATIONS = ["bias<->resid", "x<->rms_w", "N<->K clamps", "eps=0", "dropped residual"]


def gemv_mutation_applies(c, m):
    """A mutation applies where it changes what the kernel is given.  bias <-> resid is invisible in mode 1 (the two are added to the
    same sum), so it applies to the cases with a bias and no residual: there the bias lands in a slot the mode ignores."""
    return {"bias<->resid": c["bias"] and c["mode"] != 1, "x<->rms_w": c["rms"], "N<->K clamps": True, "eps=0": c["rms"],
            "dropped residual": c["mode"] == 1}[m]


def gemv_f32(c, d, mutation=None):
    """The kernel's computation in numpy float32 with ANOTHER summation order (columns descending, numpy's pairwise sums), optionally
    with one argument mutated."""
    f = np.float32
    W, x, g, bias, resid, eps = d["W"], d["x"], d["g"], d["bias"], d["resid"], f(d["eps"])
    N, K = W.shape
    n_rows, n_cols = N, K
    if mutation == "bias<->resid":
        bias, resid = resid, bias
    elif mutation == "x<->rms_w":
        x, g = g, x
    elif mutation == "eps=0":
        eps = f(0)
    elif mutation == "dropped residual":
        resid = None
    elif mutation == "N<->K clamps":  # columns clamped against N, rows against K
        n_rows, n_cols = min(N, K), min(K, N)
    xg = (x * g).astype(f) if g is not None else x
    acc = (W[:, :n_cols][:, ::-1] * xg[:n_cols][::-1]).astype(f).sum(axis=1, dtype=f)
    if g is not None:
        ss = (x[:n_cols][::-1] * x[:n_cols][::-1]).astype(f).sum(dtype=f)
        acc = acc * (f(1) / np.sqrt(ss / f(K) + eps, dtype=f))
    if bias is not None:
        acc = acc + bias
    if c["mode"] == 1 and resid is not None:
        acc = acc + resid
    acc = acc.astype(f)
    acc[n_rows:] = SENTINEL  # rows the mutant's clamp voids are never stored
    if c["mode"] == 2:
        gi, ui = glu_rows(N)
        G, Uv = acc[gi], acc[ui]
        return (G / (f(1) + np.exp(-G, dtype=f)) * Uv).astype(f)
    return acc


ATTN_GEMV_MUTATIONS = ["attn_pm<->attn_pl", "nsplit-1", "dropped residual"]


def attn_gemv_mutation_applies(c, m):
    return not (m == "nsplit-1" and c["empty"] is not None)  # (dropping an EMPTY last split changes nothing, rightly)


def attn_gemv_f32(c, d, mutation=None):
    f = np.float32
    pm, pl, po, resid = d["pm"], d["pl"], d["po"], d["resid"]
    if mutation == "attn_pm<->attn_pl":
        pm, pl = pl, pm
    elif mutation == "nsplit-1":
        pm, pl, po = pm[:, :-1], pl[:, :-1], po[:, :-1]
    elif mutation == "dropped residual":
        resid = np.zeros_like(resid)
    M = pm.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        w = np.where(np.isneginf(pm), f(0), np.exp(pm - M, dtype=f)).astype(f)
    L = (pl[:, ::-1] * w[:, ::-1]).sum(axis=1, dtype=f, keepdims=True)
    x = ((po[:, ::-1] * w[:, ::-1, None]).sum(axis=1, dtype=f) / L).astype(f).ravel()
    return ((d["W"][:, ::-1] * x[::-1]).astype(f).sum(axis=1, dtype=f) + resid).astype(f)


def excess(got, ref, bound):
    """max |got - ref| / bound over the elements (NaN or inf anywhere: inf)."""
    got = np.asarray(got, np.float64)
    if not np.all(np.isfinite(got)):
        return np.inf
    return float((np.abs(got - ref) / bound).max())


# ---- lm_head (mode 3) ----------------------------------------------------------------------------------------------------------
# N = 16 * 37 + 5 is the smallest shape with a partly filled last 16-row block; launch_gemv runs it one row per wave.  The pruned pair
# (int8 pre-pass + rescore) only exists where the unpruned launch runs 16-row blocks -- 4 rows per wave, from 32768 rows on
# (k_gemv.hip lm_head_prune_check refuses anything else) -- so the pair is checked at 32768 + 16 * 37 + 5 rows, against the unpruned
# launch on the same data.  K = 2048 (the 1.7B model's hidden size) runs the other instantiation of each kernel: gemv1_head_kernel<*, 4>,
# lm_head_approx_kernel<4>, lm_head_rescore_kernel<4, 4>.
LM_HEAD_CASES = [dict(name="lm-head-597", K=1024, N=16 * 37 + 5, pruned=False),
                 dict(name="lm-head-33365", K=1024, N=32768 + 16 * 37 + 5, pruned=True),
                 dict(name="lm-head-597-k2048", K=2048, N=16 * 37 + 5, pruned=False),
                 dict(name="lm-head-33365-k2048", K=2048, N=32768 + 16 * 37 + 5, pruned=True)]


def lm_head_inputs(c):
    r = _rng(c["name"])
    K, N = c["K"], c["N"]
    x = r.normal(0, 1, K).astype(np.float32)
    g = (1.5 + 0.5 * r.uniform(-1, 1, K)).astype(np.float32)
    a = r.uniform(-0.5, 0.5, (N, 1)).astype(np.float32)
    winner = N - 3  # in the partly filled last block
    a[winner] = 1.0
    W = bf16_round((r.normal(0, 1, (N, K)).astype(np.float32) + a * np.sign(x)) * np.float32(4.0 / K))
    return dict(W=W, x=x, g=g, bias=None, resid=None, eps=EPS), winner


# ---- one-sequence decode attention -----------------------------------------------------------------------------------------------
# GROUP 2 (n_q 4, n_kv 2), bf16 cache, 128-key splits.  pos = 0: only the new token; 127 / 128: the new row is the last of split 0, then
# the first of split 1; 300 at max_ctx 384: a trailing split that is partly empty.  nsplit covers the context held (pos // 128 + 1),
# plus one whole empty split in the first case.
DATTN_CASES = [
    dict(name="pos-0", pos=0, max_ctx=256, nsplit=2),
    dict(name="pos-127", pos=127, max_ctx=256, nsplit=1),
    dict(name="pos-128", pos=128, max_ctx=256, nsplit=2),
    dict(name="pos-300-ctx-384", pos=300, max_ctx=384, nsplit=3),
]
N_Q, N_KV, SCALE = 4, 2, float(np.sqrt(128.0))
DATTN_EPS = 1e-6


def dattn_inputs(c):
    r = _rng(c["name"])
    pos, ctx = c["pos"], c["max_ctx"]
    qkv = r.normal(0, 1, (N_Q + 2 * N_KV, 128)).astype(np.float32)
    q_norm = (1.5 + 0.5 * r.uniform(-1, 1, 128)).astype(np.float32)
    k_norm = (0.75 + 0.25 * r.uniform(-1, 1, 128)).astype(np.float32)
    ang = r.uniform(0, 2 * np.pi, 64)
    rope = np.concatenate([np.cos(ang), np.sin(ang)]).astype(np.float32)
    # every cache row holds data: rows >= pos are stale and LOUD (a reader that looks one row too far sees it)
    kc = bf16_round(r.normal(0, 1, (N_KV, ctx, 128)).astype(np.float32))
    vc = bf16_round(r.normal(0, 1, (N_KV, ctx, 128)).astype(np.float32))
    kc[:, pos:] *= 4; vc[:, pos:] *= 4
    return dict(qkv=qkv, q_norm=q_norm, k_norm=k_norm, rope=rope, kc=kc, vc=vc, pos=pos, eps=DATTN_EPS)


def _norm_rope(v, w, eps, rope, dt):
    v = v.astype(dt)
    n = v / np.sqrt((v * v).mean(axis=-1, keepdims=True) + dt(eps)) * w.astype(dt)
    c, s = rope[:64].astype(dt), rope[64:].astype(dt)
    n1, n2 = n[..., :64], n[..., 64:]
    return np.concatenate([c * n1 - s * n2, c * n2 + s * n1], axis=-1)


def dattn_new_rows(d, dt=np.float64):
    """q [n_q][128], the new k and v rows [n_kv][128] before their rounding to the cache format."""
    qkv = d["qkv"]
    q = _norm_rope(qkv[:N_Q], d["q_norm"], d["eps"], d["rope"], dt)
    k = _norm_rope(qkv[N_Q:N_Q + N_KV], d["k_norm"], d["eps"], d["rope"], dt)
    return q, k, qkv[N_Q + N_KV:].astype(dt)


GAMMA_Q = (128 + 32) * U


def new_row_bound(exact):
    return bf16_half_ulp(exact) + GAMMA_Q * np.abs(exact) + 2.0 ** -133


def dattn_context(d, k_rows, v_rows, dt=np.float64, pos=None, swap=False):
    """Context [n_q][128] over cache rows 0 .. pos - 1 and the appended rows k_rows / v_rows [n_kv][128] at pos, with its bound."""
    pos = d["pos"] if pos is None else pos
    q, _, _ = dattn_new_rows(d, dt)
    kc, vc = (d["vc"], d["kc"]) if swap else (d["kc"], d["vc"])
    ctx, bound = np.zeros((N_Q, 128)), np.zeros((N_Q, 128))
    for h in range(N_Q):
        kv = h // (N_Q // N_KV)
        K = np.concatenate([kc[kv, :pos], k_rows[kv][None]]).astype(dt)
        V = np.concatenate([vc[kv, :pos], v_rows[kv][None]]).astype(dt)
        if dt is np.float32:
            K, V = K[::-1], V[::-1]
        s = (K * q[h]).sum(axis=1, dtype=dt) / dt(SCALE)
        p = np.exp(s - s.max())
        ctx[h] = (p[:, None] * V).sum(axis=0, dtype=dt) / p.sum(dtype=dt)
        ds = GAMMA_Q * (np.abs(K) * np.abs(q[h])).sum(axis=1).max() / SCALE
        e = 2 * ds + 8 * U * (np.abs(s - s.max()).max() + 2)
        bound[h] = (2 * e + 2 * (len(s) + 64) * U) * (p[:, None] * np.abs(V)).sum(axis=0) / p.sum() + 2.0 ** -133
    return ctx, bound


def dattn_excess(c, d, kc_out, vc_out, ctx):
    """Worst excess of the appended rows and of the merged context [n_q][128] over the reference (inf: a cache row other than pos
    changed).  The context reference uses the rows the launch appended (see the module docstring)."""
    pos = d["pos"]
    _, k64, v64 = dattn_new_rows(d)
    kept = np.ones(c["max_ctx"], bool); kept[pos] = False
    if not (np.array_equal(kc_out[:, kept], d["kc"][:, kept]) and np.array_equal(vc_out[:, kept], d["vc"][:, kept])):
        return np.inf
    w_rows = max(excess(kc_out[:, pos], k64, new_row_bound(k64)), excess(vc_out[:, pos], v64, new_row_bound(v64)))
    ref, bound = dattn_context(d, kc_out[:, pos], vc_out[:, pos])
    return max(w_rows, excess(ctx, ref, bound))


def dattn_check(c, d, kc_out, vc_out, pm, pl, po):
    """Worst excess of one launch's outputs (cache images as fp32 values, partials [n_q][nsplit](, [128])); asserts the exact parts."""
    live = d["pos"] // 128 + 1
    assert np.all(np.isneginf(pm[:, live:])) and np.all(pl[:, live:] == 0) and np.all(po[:, live:] == 0), "an empty split is not (-inf, 0, 0)"
    assert np.all(np.isfinite(pm[:, :live])) and not np.any(po == SENTINEL) and not np.any(pl == SENTINEL), "a partial was not written"
    return dattn_excess(c, d, kc_out, vc_out, merge_partials(pm, pl, po)[0])


DATTN_MUTATIONS = ["kcache<->vcache", "pos-1", "pos+1"]


def dattn_f32(c, d, mutation=None):
    """The launch in numpy float32, keys in descending order: (kc_out, vc_out, context [n_q][128]); a mutant reads pos off by one or the
    caches swapped (and appends to the swapped caches)."""
    pos = d["pos"] + {"pos-1": -1, "pos+1": 1}.get(mutation, 0)
    swap = mutation == "kcache<->vcache"
    _, k, v = dattn_new_rows(d, np.float32)
    k, v = bf16_round(k), bf16_round(v)
    kc_out, vc_out = d["kc"].copy(), d["vc"].copy()
    (vc_out if swap else kc_out)[:, pos] = k
    (kc_out if swap else vc_out)[:, pos] = v
    ctx, _ = dattn_context(d, k, v, np.float32, pos=pos, swap=swap)
    return kc_out, vc_out, ctx
