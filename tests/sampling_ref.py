"""Reference arithmetic for the sampling tests (numpy only; include/q3asr.h "sampling"): Philox4x32-10 in uint64 arithmetic, the
uniform and the Gumbel noise in float64, the min-p kept set, the noisy argmax under the engine's tie rule and float64 log_softmax.
Also the seeded inputs the kernel tests run on, so a CPU test can hold what the GPU test relies on (no reference margin under
1e-3 T)."""
from __future__ import annotations

import itertools

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57     # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85     # key increments (Weyl sequence)
MASK = np.uint64(0xFFFFFFFF)
CHUNK = 2048                        # logits per workgroup of the sampler (kernels.h SAMPLE_CHUNK)


def philox4x32(counter, key, rounds: int = 10):
    """The four output words (uint64 arrays holding 32-bit values) of Philox4x32-`rounds`; counter: 4 words, key: 2 words, each a
    scalar or an array (broadcast)."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in counter]
    k0, k1 = (np.asarray(x, dtype=np.uint64) & MASK for x in key)
    s32 = np.uint64(32)
    for _ in range(rounds):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]         # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & MASK, (p0 >> s32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c


def sample_word(seed: int, s, t, j) -> np.ndarray:
    """x = word 0 with counter (j, t, s, 0) and key (seed low word, seed high word), as uint32."""
    seed = int(seed)
    return philox4x32((j, t, s, 0), (seed & 0xFFFFFFFF, seed >> 32))[0].astype(np.uint32)


def uniform(x) -> np.ndarray:
    """u = ((x >> 8) + 0.5) 2^-24 in float64 (exact): strictly between 0 and 1."""
    return ((np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def gumbel(u) -> np.ndarray:
    return -np.log(-np.log(np.asarray(u, dtype=np.float64)))


def log_softmax64(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def kept_set(row, T: float, min_p: float):
    """(mask of K, distance of the nearest finite logit to the threshold): K = { j : l_j >= m + T ln(min_p), l_j > -inf }."""
    l = np.asarray(row, dtype=np.float32).astype(np.float64)
    m = l.max()
    with np.errstate(divide="ignore"):
        thr = m + float(np.float32(T)) * np.log(float(np.float32(min_p)))
    fin = np.isfinite(l)
    keep = fin & (l >= thr)
    gap = float(np.abs(l[fin] - thr).min()) if np.isfinite(thr) and min_p < 1.0 else np.inf
    return keep, gap


class Draw:
    __slots__ = ("id", "second", "margin", "z", "lp", "kept", "thr_gap")


def sample(row, T: float, min_p: float, seed: int, s: int, t: int) -> Draw:
    """One draw: id = argmax over K of z_j = l_j + T g_j (larger value, then smaller id), the runner-up and the margin between the two
    (inf / -1 when K has one entry), z of the winner, lp = float64 log_softmax(l)[id]."""
    l32 = np.asarray(row, dtype=np.float32)
    assert l32.ndim == 1 and not np.isnan(l32).any() and np.isfinite(l32).any()
    keep, gap = kept_set(l32, T, min_p)
    ids = np.nonzero(keep)[0]
    z = l32[ids].astype(np.float64) + float(np.float32(T)) * gumbel(uniform(sample_word(seed, s, t, ids)))
    top = int(np.argmax(z))                # larger z, then smaller id (ids ascend; argmax returns the first maximum)
    d = Draw()
    d.id, d.z, d.kept, d.thr_gap = int(ids[top]), float(z[top]), keep, gap
    if len(ids) > 1:
        rest = z.copy()
        rest[top] = -np.inf
        nxt = int(np.argmax(rest))
        d.second, d.margin = int(ids[nxt]), float(z[top] - z[nxt])
    else:
        d.second, d.margin = -1, np.inf
    d.lp = float(log_softmax64(l32)[d.id])
    return d


def sample_many(jobs, threads: int = 8):
    """[sample(*job) for job in jobs] on a few threads (numpy releases the interpreter lock inside its loops)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=threads) as ex:
        return list(ex.map(lambda j: sample(*j), jobs))


def restricted_softmax(row, T: float, min_p: float) -> np.ndarray:
    """softmax(l / T) restricted to K, float64: the distribution a draw follows."""
    keep, _ = kept_set(row, T, min_p)
    l = np.asarray(row, dtype=np.float32).astype(np.float64) / float(np.float32(T))
    p = np.where(keep, np.exp(l - l[keep].max()), 0.0)
    return p / p.sum()


# ---- the kernel tests' inputs ------------------------------------------------------------------------------------------------
KERNEL_V = (1, 63, 2048, 2049, 4100, 6150)
KERNEL_T = (0.2, 1.0, 2.0)
KERNEL_MIN_P = (0.0, 0.05, 1.0)
KERNEL_STEP = (0, 7, 1023)
BIG_V = 151936
# data seed per vocabulary size: chosen on the CPU so that no reference draw of kernel_draws(V) has a margin under 1e-3 T and no logit
# lies within 1e-4 of a kept-set threshold (tests/test_sampling_host.py holds both)
DATA_SEED = {1: 0, 63: 0, 2048: 0, 2049: 0, 4100: 0, 6150: 0, BIG_V: 0}
SAMPLE_SEED = (1 << 40) + 12345     # above 2^32: both key words are live


def kernel_rows(V: int) -> np.ndarray:
    """Six rows [6][V] fp32: (0) a whole 2048-chunk of -inf, (1) the maximum in the last (partial) chunk, (2) twin maxima, (3) one finite
    entry, (4, 5) plain random rows.  Where V is too small for a case the row stays as random as V allows."""
    rng = np.random.default_rng(1000 + DATA_SEED[V] * 7919 + V)
    rows = (rng.standard_normal((6, V)) * 3.0).astype(np.float32)
    if V > CHUNK:
        c = int(rng.integers(0, V // CHUNK))
        rows[0, c * CHUNK:(c + 1) * CHUNK] = -np.inf
    last = ((V - 1) // CHUNK) * CHUNK
    rows[1, int(rng.integers(last, V))] = np.float32(rows[1].max() + 1.5)
    if V >= 2:
        a, b = sorted(rng.choice(V, 2, replace=False).tolist())
        if V > CHUNK:
            b = V - 1 - (a % 7)             # the twins in different chunks
            a = a % CHUNK
        rows[2, a] = rows[2, b] = np.float32(rows[2].max() + 0.75)
    one = int(rng.integers(0, V))
    keep = rows[3, one]
    rows[3, :] = -np.inf
    rows[3, one] = keep
    return rows


def kernel_combos(V: int):
    if V == BIG_V:
        return [(1.0, 0.05, 7)]
    return list(itertools.product(KERNEL_T, KERNEL_MIN_P, KERNEL_STEP))


def kernel_calls(V: int):
    """Every (rows of the call, T, min_p, step): S = 3 twice (rows 0-2, 3-5) and S = 1 for each of the six rows."""
    groups = [[0, 1, 2], [3, 4, 5]] + [[r] for r in range(6)]
    return [(g, T, p, st) for (T, p, st) in kernel_combos(V) for g in groups]


def kernel_draws(V: int):
    """The reference draw of every sequence of every call: [(call index, position in the call, Draw)]."""
    rows = kernel_rows(V)
    out = []
    for ci, (g, T, p, st) in enumerate(kernel_calls(V)):
        for s, r in enumerate(g):
            out.append((ci, s, sample(rows[r], T, p, SAMPLE_SEED, s, st)))
    return out
