"""Reference arithmetic for the sampling-filter tests (numpy only; include/q3asr.h "sampling filter"): the value threshold of top-k and
top-p in float64 by the contract's definition, the sandwich thresholds at top_p +- DELTA, the draw over a given threshold, and the
seeded inputs the kernel tests run on, so a CPU test can hold what the GPU test relies on."""
from __future__ import annotations

import numpy as np

import sampling_ref as R

DELTA = 1e-5        # the header's bound on |G_device - G_exact|, derived there from the arithmetic (fixed-point weights at 2^-40, expf)
NEG_INF = np.float32(-np.inf)


def _f32(v) -> np.float32:
    """A threshold as the device reports it: fp32, a zero as +0.0."""
    return np.float32(v) + np.float32(0.0)


def tau_k(row, top_k: int) -> np.float32:
    """The top_k-th largest entry counted with multiplicity; -inf when top-k is off (0 or >= V) or fewer than top_k entries are finite."""
    l = np.asarray(row, dtype=np.float32)
    V = l.shape[0]
    if top_k <= 0 or top_k >= V:
        return NEG_INF
    return _f32(np.sort(l)[::-1][top_k - 1])    # (-inf when the row runs out of finite entries first: every finite entry stays)


def mass_above(row, T: float, top_k: int):
    """(distinct finite values of K_k in descending order, G of each): G(v) = sum of w_j over { j in K_k : l_j > v } / Z, float64."""
    l = np.asarray(row, dtype=np.float32).astype(np.float64)
    l = l + 0.0                                  # -0.0 and +0.0 are one value
    keep = np.isfinite(l) & (l >= float(tau_k(row, top_k)))
    vals = np.sort(l[keep])[::-1]
    w = np.exp((vals - vals[0]) / float(np.float32(T)))
    Z = w.sum()
    excl = np.concatenate([[0.0], np.cumsum(w)[:-1]])          # mass in front of each entry, in descending order
    first = np.concatenate([[True], vals[1:] != vals[:-1]])    # the first entry of each run of equal values: the mass strictly above the run
    return vals[first], excl[first] / Z


def tau_p(row, T: float, top_k: int, top_p: float) -> np.float32:
    """The smallest row value v with G(v) < top_p; -inf when top-p is off (>= 1); the row maximum when nothing else qualifies."""
    if top_p >= 1.0:
        return NEG_INF
    vals, G = mass_above(row, T, top_k)
    ok = np.nonzero(G < top_p)[0]                # G grows downwards: the qualifying values are a leading run
    return _f32(vals[ok[-1]] if len(ok) else vals[0])


def threshold(row, T: float, top_k: int, top_p: float):
    """(max(tau_k, tau_p) as fp32, the number of entries >= it that are not -inf)."""
    top_p = float(np.float32(top_p))
    t = max(tau_k(row, top_k), tau_p(row, T, top_k, top_p))
    l = np.asarray(row, dtype=np.float32)
    return _f32(t), int((np.isfinite(l) & (l >= t)).sum())


def sandwich(row, T: float, top_k: int, top_p: float, delta: float = DELTA):
    """((tau, kept) at top_p + delta, (tau, kept) at top_p - delta): the device's threshold lies between the two taus, its count
    between the two counts.  top_p = 1 is exact: both are the top-k threshold.  top_p - delta <= 0 leaves the row maximum."""
    top_p = float(np.float32(top_p))
    if top_p >= 1.0:
        lo = hi = threshold(row, T, top_k, 1.0)
        return lo, hi
    lo_t = max(tau_k(row, top_k), tau_p(row, T, top_k, min(top_p + delta, 1.0)))
    hi_t = max(tau_k(row, top_k), tau_p(row, T, top_k, max(top_p - delta, 0.0)))
    l = np.asarray(row, dtype=np.float32)
    count = lambda t: int((np.isfinite(l) & (l >= t)).sum())
    return (_f32(lo_t), count(lo_t)), (_f32(hi_t), count(hi_t))


def minp_threshold(row, T: float, min_p: float) -> float:
    """m + T ln(min_p) as sampling_ref.kept_set evaluates it (float64 of the fp32 setting)."""
    l = np.asarray(row, dtype=np.float32).astype(np.float64)
    with np.errstate(divide="ignore"):
        return float(l.max() + float(np.float32(T)) * np.log(float(np.float32(min_p))))


def sample_over(row, T: float, thr: float, seed: int, s: int, t: int) -> R.Draw:
    """sampling_ref.sample over K = { j : l_j >= thr, l_j > -inf } for a threshold given as a number."""
    l32 = np.asarray(row, dtype=np.float32)
    keep = np.isfinite(l32) & (l32.astype(np.float64) >= thr)
    assert keep.any()
    ids = np.nonzero(keep)[0]
    z = l32[ids].astype(np.float64) + float(np.float32(T)) * R.gumbel(R.uniform(R.sample_word(seed, s, t, ids)))
    top = int(np.argmax(z))
    d = R.Draw()
    d.id, d.z, d.kept, d.thr_gap = int(ids[top]), float(z[top]), keep, np.inf
    if len(ids) > 1:
        rest = z.copy()
        rest[top] = -np.inf
        nxt = int(np.argmax(rest))
        d.second, d.margin = int(ids[nxt]), float(z[top] - z[nxt])
    else:
        d.second, d.margin = -1, np.inf
    d.lp = float(R.log_softmax64(l32)[d.id])
    return d


def sample(row, T: float, min_p: float, top_k: int, top_p: float, seed: int, s: int, t: int) -> R.Draw:
    """One draw by the contract: over { l >= max(tau_k, tau_p, tau_minp) }."""
    return sample_over(row, T, max(float(threshold(row, T, top_k, top_p)[0]), minp_threshold(row, T, min_p)), seed, s, t)


def filtered_softmax(row, T: float, min_p: float, top_k: int, top_p: float) -> np.ndarray:
    """softmax(l / T) restricted to the contract's K, float64: the distribution a draw follows."""
    l = np.asarray(row, dtype=np.float32).astype(np.float64)
    keep = np.isfinite(l) & (l >= max(float(threshold(row, T, top_k, top_p)[0]), minp_threshold(row, T, min_p)))
    p = np.where(keep, np.exp((l - l[keep].max()) / float(np.float32(T))), 0.0)
    return p / p.sum()


# ---- the kernel tests' inputs ------------------------------------------------------------------------------------------------
KERNEL_V = R.KERNEL_V
BIG_V = R.BIG_V
N_ROWS = 12
# per vocabulary size: the seed of the six rows added here and the sampling seed, chosen on the CPU so that no reference draw of
# kernel_draws(V) has a margin under 1e-3 T, none changes between the two ends of the sandwich and no logit lies within 1e-4 of a
# min-p threshold (tests/test_sampling_filter_host.py holds all three)
DATA_SEED = {1: 0, 63: 0, 2048: 0, 2049: 0, 4100: 0, 6150: 2, BIG_V: 0}
SAMPLE_SEED = {V: (1 << 41) + 777 + 1000 * n + V for V, n in {1: 0, 63: 0, 2048: 0, 2049: 0, 4100: 0, 6150: 1, BIG_V: 0}.items()}   # above 2^32
N_ZERO = 60         # zeros of both signs in row 7: the 2nd and the 50th place fall among them
N_TIED = 60         # entries of the tied value in row 9, likewise
N_FINITE = 30       # finite entries of row 10: fewer than top_k = 50


def kernel_rows(V: int) -> np.ndarray:
    """Twelve rows [12][V] fp32: the six of sampling_ref.kernel_rows, then (6) all entries equal, (7) both signs with +0.0 and -0.0
    straddling the k-th place, (8) one logit with more than 0.9 of the mass at every temperature, (9) the k-th value tied across two
    2048-chunks, (10) fewer finite entries than top_k = 50, (11) a steep row (scale 30) whose tail weights underflow.  Where V is too
    small for a case the row stays as close to it as V allows."""
    rng = np.random.default_rng(5000 + DATA_SEED[V] * 7919 + V)
    rows = (rng.standard_normal((N_ROWS, V)) * 3.0).astype(np.float32)
    rows[:6] = R.kernel_rows(V)
    rows[6, :] = np.float32(rng.standard_normal() * 3.0)
    if V >= 3:                                   # one positive entry, zeros of both signs, the rest negative
        r = -np.abs(rows[7]) - np.float32(0.5)
        pos = rng.permutation(V)
        nz = min(N_ZERO, V - 2)
        r[pos[0]] = np.float32(2.5)
        r[pos[1:1 + nz:2]] = np.float32(0.0)
        r[pos[2:1 + nz:2]] = np.float32(-0.0)
        rows[7] = r
    rows[8, int(rng.integers(0, V))] = np.float32(rows[8].max() + 25.0)
    if V >= 4:                                   # one entry above, then a run of equal values: in the first and in the last chunk
        nt = min(N_TIED, V - 2)
        top = np.float32(rows[9].max())
        last = ((V - 1) // R.CHUNK) * R.CHUNK
        a = rng.choice(min(V, R.CHUNK), nt // 2 + 1, replace=False)
        b = np.setdiff1d(last + rng.choice(V - last, min(nt - nt // 2, V - last), replace=False), a)
        rows[9, a[1:]] = rows[9, b] = top + np.float32(1.0)
        rows[9, a[0]] = top + np.float32(2.0)
    if V > N_FINITE:
        keep = rng.choice(V, N_FINITE, replace=False)
        r = np.full(V, -np.inf, dtype=np.float32)
        r[keep] = rows[10, keep]
        rows[10] = r
    rows[11] = (rng.standard_normal(V) * 30.0).astype(np.float32)
    return rows


def kernel_combos(V: int):
    """(T, min_p, top_k, top_p, step): a chosen subset of the grid in which every value of every axis appears, top-k and top-p alone
    and together."""
    if V == BIG_V:
        return [(1.0, 0.05, 50, 0.9, 7)]
    return [(1.0, 0.0, 0, 1.0, 0),               # off: q3a_selftest_sample's ids and z
            (1.0, 0.0, 1, 1.0, 7),               # the argmax
            (0.2, 0.05, 2, 1.0, 1023),
            (2.0, 0.0, 50, 1.0, 0),
            (1.0, 0.0, V, 1.0, 7),               # top_k >= V: off
            (1.0, 0.05, V + 7, 0.9, 1023),
            (1.0, 0.0, 0, 0.9, 0),
            (0.2, 0.0, 0, 0.5, 7),
            (2.0, 0.05, 0, 0.05, 1023),
            (1.0, 0.05, 50, 0.9, 0),
            (2.0, 0.0, 2, 0.5, 7),
            (0.2, 0.0, 50, 0.05, 1023)]


def kernel_calls(V: int):
    """Every (rows of the call, T, min_p, top_k, top_p, step): S = 3 four times (all twelve rows) and S = 1 for each of the six rows
    added here; at the full vocabulary the four S = 3 calls alone."""
    groups = [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]]
    if V != BIG_V:
        groups += [[r] for r in range(6, N_ROWS)]
    return [(g,) + c for c in kernel_combos(V) for g in groups]


class Case:
    __slots__ = ("call", "s", "row", "lo", "hi", "draw", "draw_lo", "draw_hi", "minp_gap")


def kernel_draws(V: int):
    """Per sequence of every call: the sandwich (lo = at top_p + DELTA, hi = at top_p - DELTA, each (tau, kept)), the reference draw
    over the contract's kept set and over the two ends of the sandwich, and the distance of the nearest logit to the min-p threshold."""
    rows = kernel_rows(V)
    out = []
    for ci, (g, T, min_p, k, p, st) in enumerate(kernel_calls(V)):
        for s, r in enumerate(g):
            c = Case()
            c.call, c.s, c.row = ci, s, r
            c.lo, c.hi = sandwich(rows[r], T, k, p)
            tm = minp_threshold(rows[r], T, min_p)
            fin = rows[r][np.isfinite(rows[r])].astype(np.float64)
            c.minp_gap = float(np.abs(fin - tm).min()) if np.isfinite(tm) else np.inf
            c.draw = sample(rows[r], T, min_p, k, p, SAMPLE_SEED[V], s, st)
            c.draw_lo = sample_over(rows[r], T, max(float(c.lo[0]), tm), SAMPLE_SEED[V], s, st)
            c.draw_hi = sample_over(rows[r], T, max(float(c.hi[0]), tm), SAMPLE_SEED[V], s, st)
            out.append(c)
    return out


def draw_is_safe(c: Case, T: float) -> bool:
    """What the GPU test needs of a reference draw: a margin over 1e-3 T at both ends of the sandwich, the same winner at both, and
    no logit within 1e-4 of the min-p threshold."""
    return (c.draw_lo.id == c.draw_hi.id == c.draw.id and min(c.draw_lo.margin, c.draw_hi.margin, c.draw.margin) > 1e-3 * T
            and c.minp_gap > 1e-4)
