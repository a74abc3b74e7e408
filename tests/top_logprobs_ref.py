"""Float64 reference of the top log-probabilities (include/q3asr.h "top log-probabilities"), and the rows the
kernel tests run.  The ordering and the log-probabilities are beam_ref.topk_ref's -- larger logit first, then smaller id; -0.0 and
+0.0 one value; -inf last with lp = -inf; log_softmax in float64 --, to which this adds the slot rule: row s writes its n entries to
slot step_count[s] of a history [S][stride][20] unless it is done or the slot is not below the stride."""
import numpy as np

from beam_ref import topk_ref

INNER = 20                                   # the history's fixed inner stride, and the largest n
CHUNK = 2048                                 # logits per workgroup of the chunk kernel
KERNEL_V = (20, 63, 2048, 2049, 4100, 6150)  # n itself, an odd size, one chunk, one entry more, three chunks (16-byte loads), four (scalar loads)
BIG_V = 151936
KERNEL_N = (1, 2, 8, 20)
UNWRITTEN = (-1, 0.0)                        # what the selftest's history holds where nothing was written


def top_ref(rows, n):
    """(ids int32 [S][n], lp float64 [S][n]) of fp32 rows [S][V]."""
    return topk_ref(np.asarray(rows, np.float32), n)


def history_ref(rows, n, step_count, done, stride):
    """The selftest's history: ids int32 [S][stride][20] (-1 where nothing was written), lp float64 likewise (0), and the mask of the
    written entries."""
    rows = np.asarray(rows, np.float32)
    S = rows.shape[0]
    ids = np.full((S, stride, INNER), UNWRITTEN[0], np.int32)
    lp = np.full((S, stride, INNER), UNWRITTEN[1], np.float64)
    written = np.zeros((S, stride, INNER), bool)
    ti, tl = top_ref(rows, n)
    for s in range(S):
        t = int(step_count[s])
        if done[s] or not (0 <= t < stride):
            continue
        ids[s, t, :n], lp[s, t, :n], written[s, t, :n] = ti[s], tl[s], True
    return ids, lp, written


def random_rows(V, S, seed):
    """S rows of N(0, 4^2) logits; every second row is rounded to halves, which ties hundreds of entries at every level."""
    rng = np.random.default_rng(seed)
    rows = (rng.standard_normal((S, V)) * 4.0).astype(np.float32)
    rows[1::2] = np.round(rows[1::2] * 2.0) / 2.0
    return rows


HAND_V = 6150      # four chunks: 2048 + 2048 + 2048 + 6


def hand_rows():
    """name -> (row [HAND_V] fp32, n, what the row claims: the ids its n best must be).  tests/test_top_logprobs_host.py holds that the
    rows contain what their names say."""
    V = HAND_V
    rng = np.random.default_rng(77)
    base = (rng.standard_normal(V) * 0.5 - 20.0).astype(np.float32)      # a floor nothing below reaches: every planted value is > -10
    out = {}
    r = base.copy()                                                       # the 20 best inside chunk 1, descending by position
    at = 2048 + 37 + 97 * np.arange(20)
    r[at] = 10.0 - 0.25 * np.arange(20, dtype=np.float32)
    out["one_chunk"] = (r, 20, at.tolist())
    r = base.copy()                                                       # the 4 best in 4 different chunks (the last one has 6 entries)
    at = np.array([6147, 11, 4097, 2050])
    r[at] = np.array([9.0, 8.0, 7.0, 6.0], np.float32)
    out["spread"] = (r, 4, at.tolist())
    r = base.copy()                                                       # the largest value twice, across the first chunk boundary
    r[[2047, 2048]] = 5.0
    r[100] = 4.0
    out["tie_2047_2048"] = (r, 2, [2047, 2048])
    out["tie_2047_2048_n1"] = (r, 1, [2047])
    out["tie_2047_2048_n3"] = (r, 3, [2047, 2048, 100])
    out["all_equal"] = (np.full(V, -1.5, np.float32), 20, list(range(20)))
    r = base.copy()                                                       # zeros of both signs around the boundary: one value, by id
    r[[2046, 2047, 2048, 2049]] = np.array([0.0, -0.0, 0.0, -0.0], np.float32)
    r[5000] = -0.0
    out["zeros_boundary"] = (r, 5, [2046, 2047, 2048, 2049, 5000])
    r = np.full(V, -np.inf, np.float32)                                   # three finite entries, n = 8: then -inf by id
    r[[4100, 7, 2048]] = np.array([1.0, 3.0, 2.0], np.float32)
    out["few_finite"] = (r, 8, [7, 2048, 4100, 0, 1, 2, 3, 4])
    r = (-1000.0 * np.arange(V)).astype(np.float32)                        # steep: every weight but the first underflows
    out["steep"] = (r, 20, list(range(20)))
    return out


def big_rows():
    """Two rows at the real vocabulary: a random one, and one whose 20 best stand in 20 different chunks."""
    rows = random_rows(BIG_V, 2, 5)
    at = (np.arange(20) * 3 + 2) * CHUNK + 5 + 101 * np.arange(20)
    rows[1] = np.minimum(rows[1], 20.0)
    rows[1, at] = 40.0 - np.arange(20, dtype=np.float32)
    return rows, at
