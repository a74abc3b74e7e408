"""Reference arithmetic for the repetition tests (numpy only; include/q3asr.h "repetition"): the repetition penalty over the distinct
ids of a history and the no-repeat n-gram ban, in fp32 with one rounding per entry, written from the contract; a naive triple loop
that restates the same rule without sets or slices; float64 log_softmax; and the seeded rows and histories the GPU kernel test
runs on."""
from __future__ import annotations

import numpy as np

NEG_INF = np.float32(-np.inf)


def apply(row, hist, p: float, n: int) -> np.ndarray:
    """l'' of one row: every distinct id j of hist gets l_j / p where l_j > 0 and l_j * p elsewhere (fp32, once); then, with
    t = len(hist) and only when n >= 1 and t >= n - 1, every i in [0, t - n + 1) whose n - 1 ids equal the last n - 1 ids of hist bans
    hist[i + n - 1]."""
    l = np.array(row, dtype=np.float32, copy=True)
    hist = [int(x) for x in hist]
    p32 = np.float32(p)
    if p32 != np.float32(1.0):
        for j in sorted(set(hist)):
            l[j] = l[j] / p32 if l[j] > 0 else l[j] * p32
    t = len(hist)
    if n >= 1 and t >= n - 1:
        tail = hist[t - n + 1:] if n > 1 else []
        for i in range(0, t - n + 1):
            if hist[i:i + n - 1] == tail:
                l[hist[i + n - 1]] = NEG_INF
    return l


def apply_naive(row, hist, p: float, n: int) -> np.ndarray:
    """The same rule as three plain loops: over the vocabulary for the penalty (is j anywhere in the history?), over (i, k) for the
    ban."""
    l = np.array(row, dtype=np.float32, copy=True)
    p32 = np.float32(p)
    t = len(hist)
    for j in range(len(l)):
        seen = False
        for i in range(t):
            if int(hist[i]) == j:
                seen = True
        if seen:
            l[j] = l[j] / p32 if l[j] > 0 else l[j] * p32
    if n >= 1 and t >= n - 1:
        for i in range(0, t - n + 1):
            match = True
            for k in range(n - 1):
                if int(hist[i + k]) != int(hist[t - n + 1 + k]):
                    match = False
            if match:
                l[int(hist[i + n - 1])] = NEG_INF
    return l


def apply_rows(rows, hists, p: float, n: int) -> np.ndarray:
    return np.stack([apply(r, h, p, n) for r, h in zip(rows, hists)])


def argmax(x) -> int:
    """The engine's tie rule: the larger value, then the smaller id (numpy's argmax returns the first maximum)."""
    return int(np.argmax(np.asarray(x)))


def log_softmax64(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---- the kernel test's inputs ------------------------------------------------------------------------------------------------
KERNEL_V = (1, 31, 32, 33, 2049, 6150, 8225)   # 8225: 258 bitmap words, more than one per thread, the last ragged
BIG_V = 151936
KERNEL_N = (0, 1, 2, 3, 5)
KERNEL_P = (1.0, 1.3, 0.8)
LONG_T = 4200


def kernel_lengths(n: int):
    """t of the contract's list: 0, 1, n - 1, n, and the lengths that make the history walk and the n-gram scan cross the 256-thread
    stride."""
    return sorted({0, 1, max(n - 1, 0), n, 255, 256, 257, 1023})


def kernel_row(V: int, seed: int) -> np.ndarray:
    """One row [V] fp32 in the normal range: random values of both signs, and -- where V has room -- a zero, a -inf, a large positive
    and a large negative entry at low ids (the ids the histories draw from most often)."""
    rng = np.random.default_rng(7000 + 31 * V + seed)
    row = (rng.standard_normal(V) * 4.0).astype(np.float32)
    row[np.abs(row) < 1e-3] = np.float32(0.5)       # normal range, away from the subnormals
    if V > 8:
        row[1] = NEG_INF
        row[2] = np.float32(0.0)
        row[3] = np.float32(11.5)                   # the row maximum unless it is penalised or banned
        row[4] = np.float32(-9.25)
        row[V - 1] = np.float32(10.75)              # the runner-up, at the last id
    return row


def kernel_history(V: int, t: int, n: int, kind: int, seed: int) -> list:
    """A history of t ids.  kind 0: ids from a small alphabet that includes 0 and V - 1 (many overlapping n-gram matches), ending in a
    repeat of its own start so that a match is certain where t allows one; kind 1: one id 200 times, then ids from the whole
    vocabulary; kind 2: a period-2 pattern 'abab...' (overlapping matches, the banned id is also a penalised one)."""
    rng = np.random.default_rng(9000 + 131 * V + 17 * t + 5 * n + kind + 1000 * seed)
    if t == 0:
        return []
    small = sorted({0, V - 1, min(3, V - 1), min(2, V - 1), min(1, V - 1), min(4, V - 1), V // 2})
    if kind == 0:
        h = [small[int(x)] for x in rng.integers(0, len(small), t)]
        k = max(n - 1, 1)
        if t >= 2 * k + 1:
            h[t - k:] = h[:k]                        # the tail repeats the head: h[k] is banned for n >= 2
        return h
    if kind == 1:
        rep = int(small[int(rng.integers(0, len(small)))])
        h = [rep] * min(t, 200) + [int(x) for x in rng.integers(0, V, max(t - 200, 0))]
        return h
    a, b = small[-1], small[0]
    return [a if i % 2 == 0 else b for i in range(t)]


def kernel_cases(V: int):
    """[(S, rows [S][V], hists (S lists), p, n)]: for every (n, p) one S = 3 call with per-sequence lengths that differ and an S = 1
    call for each remaining length, the three kinds of history rotating.  V = BIG_V: one call."""
    if V == BIG_V:
        rows = np.stack([kernel_row(V, s) for s in range(3)])
        hists = [kernel_history(V, t, 3, k, 0) for k, t in enumerate((1023, 257, 2))]
        return [(3, rows, hists, 1.3, 3)]
    cases = []
    for ni, n in enumerate(KERNEL_N):
        for pi, p in enumerate(KERNEL_P):
            ts = kernel_lengths(n)
            trio, rest = [ts[-1], ts[len(ts) // 2], ts[0]], [t for i, t in enumerate(ts) if i not in (0, len(ts) // 2, len(ts) - 1)]
            rows = np.stack([kernel_row(V, 10 * ni + pi + s) for s in range(3)])
            cases.append((3, rows, [kernel_history(V, t, n, (k + pi) % 3, ni) for k, t in enumerate(trio)], p, n))
            for k, t in enumerate(rest):
                cases.append((1, kernel_row(V, 100 + k)[None], [kernel_history(V, t, n, (k + ni + pi) % 3, pi)], p, n))
    if V == 6150:   # a history longer than the 4096 ids the kernel keeps in LDS: the ids beyond them are read in place
        cases.append((1, kernel_row(V, 999)[None], [kernel_history(V, LONG_T, 3, 0, 7)], 1.3, 3))
    return cases
