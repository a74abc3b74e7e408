"""float64 references, derived per-element bounds and the cases of the one-sequence chain with o_proj per pair of kv heads (csrc/k_gemv.hip
oproj_head_kernel and the gate / up form that adds its partial vectors, k_dattn.hip at 32 and 64 keys per split), as
q3a_selftest_oproj_head_launch / q3a_selftest_gemv_parts_launch / q3a_selftest_decode_attn_split_launch run them.

The chain computes  x' = resid + sum_p y_p,  y_p[n] = sum_{k in slice p} W[n][k] c[k] (+ bias[n] in slice 0),  c = the merged attention
context, then the norm-fused GLU of x'.  Bounds, from the order-free formulas of tests/decode_kernels_ref.py (u = 2^-24; nothing here is
measured):
  y_p        gamma = (K + 16) u as for every GEMV there (K, the whole row, bounds the 512 terms of a slice and the wave tree from above),
             and the merged-context term with up to 16 splits:  bound_p[n] = 4 gamma (sum_{k in p} |W_nk c_k| + |bias_n|) + sum_{k in p} |W_nk| dc_k.
             dc is merge_partials' bound, whose per-weight error e = 4 u (|m - M| + 2) also covers the hardware exponential this kernel
             always uses: exp2(d log2 e) with the product rounded once (relative error of the result <= |d| u) and the instruction's
             1 ulp (2 u).
  x'         a sum of n_parts + 1 fp32 terms in a fixed order:  (n_parts + 2) u (|resid| + sum_p |y_p|)  on top of the terms' own bounds.
  GLU        the launch returns x' as it stored it and the kernel normalises exactly those bits, so the GLU reference is formed from the
             returned vector with decode_kernels_ref.gemv_reference: no perturbation analysis is needed.
  attention  decode_kernels_ref.dattn_excess, with the number of live splits taken at the launch's split size.

tests/test_oproj_by_head_host.py shows on the CPU that an honest fp32 evaluation in the chain's order stays inside these bounds and
that each single-argument mutant leaves them by a factor of at least 100.
"""
import numpy as np

import decode_kernels_ref as R

U = R.U
MAX_SPLITS = 16  # OPROJ_HEAD_MAX_SPLITS

# q heads (a slice is two kv heads of two q heads each: 512 columns; 4 / 2 heads: one slice), N = 70: 16-row blocks, the last one partly void.
# nsplit 1, 3 with the last split empty, 16 (every slot of the kernel's table live); a bias in two of them (it rides in slice 0).
OPROJ_CASES = [dict(name=f"oproj-{nq}q-{ns}-splits" + ("-last-empty" if em is not None else "") + ("-bias" if b else ""),
                    heads=nq, n_parts=nq // 4, K=nq * 128, N=70, nsplit=ns, empty=em, bias=b)
               for nq in (4, 16) for ns, em, b in ((1, None, False), (3, 2, True), (16, None, False))]
# gate / up with partial vectors: K = 1024 and 1016 (the last lanes' columns clamped), N = 2 x 96 with bias, 4 vectors; and the tiny
# preset's shape (K = 256, 1 vector: three of the kernel's four requests clamped to it and not added)
PARTS_CASES = [dict(name="parts-k1024", K=1024, N=2 * 96, n_parts=4, mode=2, rms=True, bias=True),
               dict(name="parts-k1016", K=1016, N=2 * 96, n_parts=4, mode=2, rms=True, bias=True),
               dict(name="parts-k256-1-vector", K=256, N=2 * 96, n_parts=1, mode=2, rms=True, bias=True)]
# decode attention at 32 and 64 keys per split (GROUP 2, bf16 cache): around the first three boundaries of either size under max_ctx
# 96, and at the regime change of the engine's table (511: the last position of sixteen 32-key splits; 512) under max_ctx 640
DATTN_SPLIT_CASES = ([dict(name=f"kps{k}-pos-{p}", kps=k, pos=p, max_ctx=96) for k in (32, 64) for p in (0, 31, 32, 33, 63, 64, 65)] +
                     [dict(name=f"kps{k}-pos-{p}-ctx-640", kps=k, pos=p, max_ctx=640) for k in (32, 64) for p in (511, 512)])


# End to end on the tiny preset (tests/conftest.py tiny_dir): synthetic_clip(seed, seconds), fixed_new_tokens = steps.  A 275-token
# prompt and 260 steps take the context from 276 to 535 keys: 32-key splits up to 512 keys, then 64-key splits.  The seed is the one
# of 0 .. 59 with the largest smallest top-1 / top-2 margin of the fp32 oracle over the run (1.7e-3; the host test asserts > 1e-3).
# A one-second clip would start at 29 keys, but over the ~500 steps it then needs none of 120 seeds keeps the margin above 1e-3.
E2E_CLIP_SEED, E2E_CLIP_SECONDS, E2E_STEPS, E2E_MIN_MARGIN = 34, 20.0, 260, 1e-3


def dattn_nsplit(c):
    """Splits launched: those that hold a key, plus one whole empty split where the cache has room for it."""
    return min((c["max_ctx"] + c["kps"] - 1) // c["kps"], c["pos"] // c["kps"] + 2)


def dattn_check(c, d, kc_out, vc_out, pm, pl, po):
    """decode_kernels_ref.dattn_check at the case's split size."""
    live = d["pos"] // c["kps"] + 1
    assert np.all(np.isneginf(pm[:, live:])) and np.all(pl[:, live:] == 0) and np.all(po[:, live:] == 0), "an empty split is not (-inf, 0, 0)"
    assert np.all(np.isfinite(pm[:, :live])) and not np.any(po == R.SENTINEL) and not np.any(pl == R.SENTINEL), "a partial was not written"
    return R.dattn_excess(c, d, kc_out, vc_out, R.merge_partials(pm, pl, po)[0])


def oproj_inputs(c):
    r = R._rng(c["name"])
    K, N, H, ns = c["K"], c["N"], c["heads"], c["nsplit"]
    pm = r.normal(0, 2, (H, ns)).astype(np.float32)
    pl = r.uniform(1, 50, (H, ns)).astype(np.float32)
    # heads that differ loudly: a slice merged from its neighbour's partials must show
    po = ((r.normal(0, 1, (H, ns, 128)) + 0.5 * r.normal(0, 1, (H, 1, 128))) * pl[:, :, None]).astype(np.float32)
    if c["empty"] is not None:
        pm[:, c["empty"]] = -np.inf; pl[:, c["empty"]] = 0; po[:, c["empty"]] = 0
    elif ns > 1:  # the last split carries weight in every head (a merge that stops one split short must show)
        pm[:, -1] = pm.max(axis=1) + 0.5
    x64, _ = R.merge_partials(pm, pl, po)
    a = r.uniform(0.25, 1, (N, 1)) * np.where(r.uniform(size=(N, 1)) < 0.5, -1.0, 1.0)
    # rows correlated with the context inside EVERY slice (|y_p| a fixed share of the slice's sum |terms|), 512 columns per slice
    W = R.bf16_round(((r.normal(0, 1, (N, K)) + a * np.sign(x64.ravel())) * (4.0 / 512)).astype(np.float32))
    sgn = lambda n: np.where(r.uniform(size=n) < 0.5, -1.0, 1.0)
    resid = (sgn(N) * r.uniform(1, 2, N)).astype(np.float32)
    bias = (sgn(N) * r.uniform(1, 2, N)).astype(np.float32) if c["bias"] else None
    return dict(W=W, pm=pm, pl=pl, po=po, resid=resid, bias=bias)


def oproj_reference(c, d):
    """y_part [n_parts][N] and its bound; the chain's x' = resid + sum_p y_p [N] and its bound."""
    W = d["W"].astype(np.float64)
    N, K = W.shape
    P = c["n_parts"]
    gam = (K + 16) * U
    x, dx = R.merge_partials(d["pm"], d["pl"], d["po"])
    x, dx = x.ravel(), dx.ravel()
    y, b = np.zeros((P, N)), np.zeros((P, N))
    for p in range(P):
        s = slice(p * 512, (p + 1) * 512)
        bias = d["bias"].astype(np.float64) if (d["bias"] is not None and p == 0) else np.zeros(N)
        y[p] = W[:, s] @ x[s] + bias
        b[p] = 4 * gam * (np.abs(W[:, s]) @ np.abs(x[s]) + np.abs(bias)) + np.abs(W[:, s]) @ dx[s] + 2.0 ** -133
    xs = d["resid"].astype(np.float64) + y.sum(axis=0)
    bs = b.sum(axis=0) + (P + 2) * U * (np.abs(d["resid"]) + np.abs(y).sum(axis=0) + b.sum(axis=0))
    return y, b, xs, bs


OPROJ_MUTATIONS = ["head+1", "head-1", "pm<->pl", "nsplit-1", "vector dropped", "vector twice", "residual dropped"]


def oproj_mutation_applies(c, m):
    """nsplit - 1 needs a last split that carries weight (and another one to fall back to)."""
    return not (m == "nsplit-1" and (c["empty"] is not None or c["nsplit"] == 1))


def oproj_f32(c, d, mutation=None):
    """The chain in numpy float32 in its own order -- each slice's context merged from its four heads' partials, one dot product per
    slice, then resid + y_0 + y_1 + ... ascending -- with ANOTHER order inside every sum (splits and columns descending, numpy's
    pairwise sums), optionally with one argument mutated: (y_part [n_parts][N], x' [N])."""
    f = np.float32
    pm, pl, po, W = d["pm"], d["pl"], d["po"], d["W"]
    P, N, H = c["n_parts"], W.shape[0], c["heads"]
    if mutation == "pm<->pl":
        pm, pl = pl, pm
    elif mutation == "nsplit-1":
        pm, pl, po = pm[:, :-1], pl[:, :-1], po[:, :-1]
    shift = {"head+1": 1, "head-1": -1}.get(mutation, 0)
    y = np.zeros((P, N), f)
    for p in range(P):
        hs = [(4 * p + g + shift) % H for g in range(4)]  # the q heads whose partials slice p merges
        M = pm[hs].max(axis=1, keepdims=True)
        with np.errstate(invalid="ignore"):
            w = np.where(np.isneginf(pm[hs]), f(0), np.exp(pm[hs] - M, dtype=f)).astype(f)
        L = (pl[hs][:, ::-1] * w[:, ::-1]).sum(axis=1, dtype=f, keepdims=True)
        x = ((po[hs][:, ::-1] * w[:, ::-1, None]).sum(axis=1, dtype=f) / L).astype(f).ravel()
        y[p] = (W[:, p * 512:(p + 1) * 512][:, ::-1] * x[::-1]).astype(f).sum(axis=1, dtype=f)
        if d["bias"] is not None and p == 0:
            y[p] = y[p] + d["bias"]
    xs = np.zeros(N, f) if mutation == "residual dropped" else d["resid"].copy()
    for p in range(P):
        if mutation == "vector dropped" and p == P - 1:
            continue
        xs = (xs + y[p]).astype(f)
        if mutation == "vector twice" and p == 0:
            xs = (xs + y[p]).astype(f)
    return y, xs


def oproj_excess(c, d, y_part, xs=None):
    """Worst excess of the partial vectors (and, when given, of the summed residual) over their bounds."""
    y, b, x_ref, x_b = oproj_reference(c, d)
    w = R.excess(y_part, y, b)
    return w if xs is None else max(w, R.excess(xs, x_ref, x_b))


# ---- gate / up with partial vectors --------------------------------------------------------------------------------------------
def parts_inputs(c):
    r = R._rng(c["name"])
    K, P = c["K"], c["n_parts"]
    d = R.gemv_inputs(c)  # W correlated with d["x"]: the vector the GLU must see is the SUM, so x is split into resid + parts below
    total = d["x"]
    sgn = lambda n: np.where(r.uniform(size=n) < 0.5, -1.0, 1.0)
    parts = (sgn((P, K)) * r.uniform(0.5, 1.5, (P, K))).astype(np.float32)  # every vector of order 1: none can go missing unseen
    resid = (total.astype(np.float64) - parts.astype(np.float64).sum(axis=0)).astype(np.float32)
    d.update(resid_x=resid, parts=parts)
    del d["x"]
    return d


def parts_sum_reference(d):
    """x' = resid + sum of the vectors in float64, and its bound."""
    t = np.concatenate([d["resid_x"][None], d["parts"]]).astype(np.float64)
    return t.sum(axis=0), (len(t) + 1) * U * np.abs(t).sum(axis=0) + 2.0 ** -133


def parts_glu_reference(c, d, x_sum):
    """The GLU reference and bound on the summed vector as the launch stored it (fp32 bits)."""
    return R.gemv_reference(c, dict(d, x=np.asarray(x_sum, np.float32)))


PARTS_MUTATIONS = ["vector dropped", "vector twice", "residual dropped", "stride K+8"]


def parts_mutation_applies(c, m):
    return not (m == "stride K+8" and c["n_parts"] == 1)  # (a single vector starts where the buffer does, whatever the stride)


def parts_f32(c, d, mutation=None):
    """(x' [K], GLU out [N / 2]) in numpy float32: the sum ascending, the GEMV in decode_kernels_ref.gemv_f32's other order."""
    f = np.float32
    parts, P, K = d["parts"], c["n_parts"], c["K"]
    if mutation == "stride K+8":  # vector h read 8 h floats further on (the flat buffer, wrapped at its end)
        flat = parts.ravel()
        parts = np.stack([np.roll(flat, -8 * h)[h * K:(h + 1) * K] for h in range(P)])
    xs = np.zeros(K, f) if mutation == "residual dropped" else d["resid_x"].copy()
    for h in range(P):
        if mutation == "vector dropped" and h == P - 1:
            continue
        xs = (xs + parts[h]).astype(f)
        if mutation == "vector twice" and h == 0:
            xs = (xs + parts[h]).astype(f)
    return xs, R.gemv_f32(c, dict(d, x=xs))
