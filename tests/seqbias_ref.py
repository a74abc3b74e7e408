"""Reference arithmetic for the sequence-bias tests (numpy only; include/q3asr.h "sequence bias"): the processor written from the
contract, a naive restatement as plain loops over vocabulary x entries, float64 log_softmax, and the seeded rows, histories and
lists the GPU kernel test runs on.  An entry is (ids, bias): a tuple of 1 to 32 token ids and a bias that is finite or -inf; a list
of entries is in the caller's order, which is the order the biases of one target are added in."""
from __future__ import annotations

import numpy as np

NEG_INF = np.float32(-np.inf)
MAX_LEN, MAX_ENTRIES, MAX_IDS = 32, 4096, 65536


def fires(seq, hist) -> bool:
    """t >= L - 1 and h[t - L + 1 .. t) == q_0 .. q_{L-2}; a one-token entry always fires."""
    L, t = len(seq), len(hist)
    return t >= L - 1 and [int(x) for x in hist[t - L + 1:t]] == [int(x) for x in seq[:-1]]


def apply(row, hist, entries) -> np.ndarray:
    """l'' of one row.  Per target id: acc = 0.0f, + the bias of its one-token entry (it always fires), + the bias of each longer
    firing entry in the caller's order, one fp32 add each; then l_target + acc, one more, if anything fired."""
    l = np.array(row, dtype=np.float32, copy=True)
    hist = [int(x) for x in hist]
    acc, order = {}, []
    for single in (True, False):                      # the one-token entries first, then the others: both in the caller's order
        for seq, b in entries:
            if (len(seq) == 1) != single or not fires(seq, hist):
                continue
            v = int(seq[-1])
            if v not in acc:
                acc[v] = np.float32(0.0)
                order.append(v)
            with np.errstate(over="ignore", invalid="ignore"):
                acc[v] = np.float32(acc[v] + np.float32(b))
    with np.errstate(over="ignore", invalid="ignore"):
        for v in order:
            l[v] = np.float32(l[v] + acc[v])
    return l


def apply_naive(row, hist, entries) -> np.ndarray:
    """The same rule as plain loops: for every id of the vocabulary, every entry, every position of its prefix."""
    l = np.array(row, dtype=np.float32, copy=True)
    t = len(hist)
    for v in range(len(l)):
        acc, fired = np.float32(0.0), False
        for want_single in (True, False):
            for seq, b in entries:
                L = len(seq)
                if int(seq[L - 1]) != v or (L == 1) != want_single or t < L - 1:
                    continue
                match = True
                for k in range(L - 1):
                    if int(hist[t - L + 1 + k]) != int(seq[k]):
                        match = False
                if match:
                    with np.errstate(over="ignore", invalid="ignore"):
                        acc = np.float32(acc + np.float32(b))
                    fired = True
        if fired:
            with np.errstate(over="ignore", invalid="ignore"):
                l[v] = np.float32(l[v] + acc)
    return l


def apply_rows(rows, hists, entries) -> np.ndarray:
    return np.stack([apply(r, h, entries) for r, h in zip(rows, hists)])


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


def flatten(entries):
    """(ids int32, lens int32, bias float32) as q3a_set_sequence_bias / q3a_selftest_seqbias take a list."""
    ids = np.asarray([int(t) for seq, _ in entries for t in seq], dtype=np.int32)
    lens = np.asarray([len(seq) for seq, _ in entries], dtype=np.int32)
    bias = np.asarray([b for _, b in entries], dtype=np.float32)
    return ids, lens, bias


# ---- the kernel test's inputs ------------------------------------------------------------------------------------------------
KERNEL_V = (1, 33, 2049, 8225)
BIG_V = 151936
KERNEL_L = (1, 2, 31, 32)
KERNEL_T = (0, 1, 2, 29, 30, 31, 32, 257, 1023)     # t = 0, 1, L - 2, L - 1, L for L in KERNEL_L, 31, 32, 257, 1023
# (entries E of a list, every entry on a target of its own) per vocabulary.  With targets of their own E is also the number of
# groups G: 255 / 256 / 257 groups around the 256-thread stride, 4096 the capacity (16 groups per thread); the other lists put
# several entries on one target (at V = 33 up to 4096 entries on 33 targets: long group walks).
KERNEL_E = {1: ((1, False), (32, False)), 33: ((1, False), (255, False), (4096, False)),
            2049: ((255, True), (256, True), (257, True), (4096, False)), 8225: ((1, False), (300, False), (4096, True))}
ORDER_BIASES = (1e8, 1.0, -1e8)                     # (0 + 1e8 + 1) - 1e8 = 0 in fp32, any other order gives 1


def kernel_row(V: int, seed: int) -> np.ndarray:
    """One row [V] fp32 in the normal range, both signs; where V has room a -inf, a zero, the row maximum and a runner-up."""
    rng = np.random.default_rng(7100 + 31 * V + seed)
    row = (rng.standard_normal(V) * 4.0).astype(np.float32)
    row[np.abs(row) < 1e-3] = np.float32(0.5)
    if V > 8:
        row[1] = NEG_INF
        row[2] = np.float32(0.0)
        row[3] = np.float32(21.5)
        row[V - 1] = np.float32(20.75)
    return row


def kernel_history(V: int, t: int, seed: int) -> list:
    """t ids: from a small alphabet that includes 0 and V - 1 (prefixes recur, so entries made for one history also meet others)."""
    rng = np.random.default_rng(9100 + 131 * V + 17 * t + seed)
    small = sorted({0, V - 1, min(3, V - 1), min(2, V - 1), min(1, V - 1), V // 2})
    return [small[int(x)] for x in rng.integers(0, len(small), t)]


def kernel_entries(V: int, E: int, hists, seed: int, own_targets: bool = False):
    """E distinct entries in a shuffled caller's order.  Built from the histories so that entries of every length the history allows
    fire (their leading ids are the history's tail), next to entries that cannot (a tail with its last id changed, or longer than
    the history); one target carries a one-token entry and two longer ones with ORDER_BIASES, so the order of the additions shows;
    some biases are -inf.  own_targets: that triple is left out and every entry gets a target of its own (E entries, E groups)."""
    rng = np.random.default_rng(5100 + 7 * V + 13 * E + seed)
    if E == 1:                                        # one two-token entry: fires on the rows whose history ends in id 0, not on the others
        return [((0, 7 % V), float(np.float32(9.5)))]
    if V == 1:                                        # a one-id vocabulary has one entry per length, all on target 0
        lens = rng.permutation(np.arange(1, E + 1))
        return [((0,) * int(L), float(np.float32(rng.standard_normal() * 3.0))) for L in lens]
    seen, out = set(), []

    def add(seq, b):
        seq = tuple(int(x) for x in seq)
        if len(out) < E and seq not in seen and 1 <= len(seq) <= MAX_LEN:
            seen.add(seq)
            out.append((seq, float(np.float32(b))))

    def tail(h, L):                                   # the L - 1 leading ids an L-token entry needs to fire on h
        return list(h[len(h) - (L - 1):]) if L > 1 else []

    def free_target():
        v = int(rng.integers(0, V))
        for _ in range(64):
            if v not in used:
                break
            v = int(rng.integers(0, V))
        used.add(v)
        return v

    used = {1, 3, 5} if V > 8 else set()
    longest = max(hists, key=len)
    # the order-sensitive triple on one target: its one-token entry and two longer firing entries
    if E >= 3 and len(longest) >= 2 and V > 8 and not own_targets:
        tgt = 5
        add(tail(longest, 3) + [tgt], ORDER_BIASES[1])
        add(tail(longest, 2) + [tgt], ORDER_BIASES[2])
        add([tgt], ORDER_BIASES[0])
    for h in hists:
        t = len(h)
        for L in KERNEL_L + (3, 5):
            tgt = free_target()
            b = NEG_INF if rng.random() < 0.25 else rng.standard_normal() * 6.0
            if t >= L - 1:
                add(tail(h, L) + [tgt], b)            # fires on h
                if L > 1 and V > 1:                   # the same with the id next to the target changed: does not fire on h
                    miss = tail(h, L)
                    miss[-1] = (miss[-1] + 1) % V
                    add(miss + [free_target()], rng.standard_normal() * 6.0)
            else:
                add([int(x) for x in rng.integers(0, V, L - 1)] + [tgt], b)   # longer than the history: cannot fire yet
    if V > 8:
        add([3], -7.25)                               # a one-token entry on the row maximum: the argmax moves
        add([1], 2.0)                                 # ... and one on the -inf logit: -inf stays -inf
    while len(out) < E:                               # fill: random entries, each on a target of its own while V has room
        L = int(KERNEL_L[int(rng.integers(0, 4))]) if rng.random() < 0.3 else int(rng.integers(1, 5))
        add([int(x) for x in rng.integers(0, V, L - 1)] + [free_target()], NEG_INF if rng.random() < 0.1 else rng.standard_normal() * 6.0)
    order = rng.permutation(len(out))
    return [out[int(i)] for i in order]


def kernel_cases(V: int):
    """[(S, rows [S][V], hists (S lists), entries)].  For every E of KERNEL_E[V]: one S = 3 call with three lengths that differ and
    an S = 1 call for every other length of KERNEL_T.  V = BIG_V: one S = 3 call with 4096 entries."""
    if V == BIG_V:
        hists = [kernel_history(V, t, 3) for t in (1023, 32, 0)]
        return [(3, np.stack([kernel_row(V, s) for s in range(3)]), hists, kernel_entries(V, MAX_ENTRIES, hists, 0, True))]
    cases = []
    for ei, (E, own) in enumerate(KERNEL_E[V]):
        ts = list(KERNEL_T)
        trio = [ts[(ei + 8) % 9], ts[(ei + 4) % 9], ts[ei % 9]]
        hists = [kernel_history(V, t, ei) for t in trio]
        cases.append((3, np.stack([kernel_row(V, 10 * ei + s) for s in range(3)]), hists, kernel_entries(V, E, hists, ei, own)))
        for k, t in enumerate(t for t in ts if t not in trio):
            h = [kernel_history(V, t, 50 + ei)]
            cases.append((1, kernel_row(V, 100 + k)[None], h, kernel_entries(V, E, h, 20 + k, own)))
    return cases
