"""Reference for row options (include/q3asr.h "row options"): the existing references composed row by row, each row with its own
record and its own list -- seqbias_ref.apply, repetition_ref.apply, then sampling_filter_ref / sampling_ref -- plus the one rule
this section adds: a row with temperature 0 takes the argmax (larger value, then smaller id), its threshold reads -inf and its kept
count the finite entries.  Also the inputs of the kernel test (tests/test_gpu_row_options.py), whose near-tie freedom
tests/test_row_options_host.py asserts on the CPU."""
from dataclasses import dataclass, field, replace

import numpy as np

import repetition_ref as P
import sampling_filter_ref as F
import sampling_ref as R
import seqbias_ref as Q

NEG_INF = np.float32(-np.inf)


@dataclass(frozen=True)
class Record:
    """q3a_row_options."""
    temperature: float = 0.0
    min_p: float = 0.0
    seed: int = 0
    top_k: int = 0
    top_p: float = 1.0
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    sequence_list: int = -1

    @property
    def sampled(self):
        return self.temperature > 0.0

    @property
    def filtered(self):
        return self.sampled and (self.top_k, float(np.float32(self.top_p))) != (0, 1.0)

    @property
    def p_on(self):
        return self.sampled and float(np.float32(self.top_p)) < 1.0


@dataclass
class RowResult:
    logits: np.ndarray            # l'' fp32
    id: int
    lp: float                     # float64 log_softmax(l'')[id]
    z: float                      # the winning noisy score (l''_id on a greedy row)
    thr: np.float32               # max(tau_k, tau_p) by the contract (-inf: greedy or unfiltered)
    kept: int                     # entries >= thr that are not -inf
    lo: tuple = None              # sandwich ends (tau, kept) at top_p + DELTA / - DELTA (top-p rows only)
    hi: tuple = None
    case: object = field(default=None, repr=False)   # sampling_filter_ref.Case of a sampled row (draw_is_safe)


def processed(row, hist, rec: Record, lists) -> np.ndarray:
    """l'' of one row: the row's own list, then the row's own penalty and n-gram ban."""
    l = np.array(row, dtype=np.float32, copy=True)
    if rec.sequence_list >= 0:
        l = Q.apply(l, hist, lists[rec.sequence_list])
    return P.apply(l, hist, rec.repetition_penalty, rec.no_repeat_ngram_size)


def run_row(row, hist, rec: Record, lists, s: int) -> RowResult:
    """Row s at step t = len(hist)."""
    l, t = processed(row, hist, rec, lists), len(hist)
    finite = int(np.isfinite(l).sum())
    if not rec.sampled:                                   # the rule of this section
        i = Q.argmax(l)
        return RowResult(l, i, float(R.log_softmax64(l)[i]), float(l[i]), NEG_INF, finite)
    T, mp, k, p = rec.temperature, rec.min_p, rec.top_k, rec.top_p
    c = F.Case()
    c.call, c.s, c.row = 0, s, s
    c.lo, c.hi = F.sandwich(l, T, k, p)
    tm = F.minp_threshold(l, T, mp)
    fin = l[np.isfinite(l)].astype(np.float64)
    c.minp_gap = float(np.abs(fin - tm).min()) if np.isfinite(tm) else np.inf
    c.draw = F.sample(l, T, mp, k, p, rec.seed, s, t) if rec.filtered else R.sample(l, T, mp, rec.seed, s, t)
    c.draw_lo = F.sample_over(l, T, max(float(c.lo[0]), tm), rec.seed, s, t)
    c.draw_hi = F.sample_over(l, T, max(float(c.hi[0]), tm), rec.seed, s, t)
    thr, kept = F.threshold(l, T, k, p) if rec.filtered else (NEG_INF, finite)
    return RowResult(l, c.draw.id, c.draw.lp, c.draw.z, thr, kept, c.lo, c.hi, c)


def run(rows, hists, recs, lists):
    return [run_row(rows[s], hists[s], recs[s], lists, s) for s in range(len(recs))]


def is_safe(r: RowResult, rec: Record) -> bool:
    """A sampled row whose id the device must reproduce exactly (sampling_filter_ref.draw_is_safe); a greedy row: no exact tie at the top
    is needed (the tie rule is the contract), so always."""
    return True if r.case is None else F.draw_is_safe(r.case, rec.temperature)


def flatten_lists(lists):
    """(ids, lens, bias, list_lens) as q3a_set_sequence_bias_lists / q3a_selftest_row_options take them."""
    flat = [e for l in lists for e in l]
    ids, lens, bias = Q.flatten(flat)
    return ids, lens, bias, np.asarray([len(l) for l in lists], dtype=np.int32)


# ---- the kernel test's inputs ------------------------------------------------------------------------------------------------
KERNEL_V = (2049, 4100, 8225)     # scalar loads + one logit in the second chunk; 16-byte loads, three chunks; > 1 bitmap word per thread
BIG_V = 151936
LENS = (0, 1, 31, 32, 257, 40)    # history length of row s; the last becomes LONG_T at V = 8225
LONG_T = 4200                     # beyond REPEAT_HIST_LDS (4096)
SHARED, FIRED, BANNED = 7, 11, 12  # target ids: in both lists with different biases; of list 1's firing entry; of its -inf entry
SEED0 = (5 << 32) + 2024          # above 2^32: both key words are live; row s draws with SEED0 + SEEDS[..] + s
# first seed offsets at which the reference alone shows no unsafe draw (tests/test_row_options_host.py asserts it)
SEEDS = {(2049, False): 0, (2049, True): 0, (4100, False): 0, (4100, True): 0, (8225, False): 0, (8225, True): 0, (BIG_V, False): 0}


def records(seed: int, reverse: bool = False):
    """The six records of the kernel test in the issue's order (reverse: the last first); row s draws with seed + s."""
    recs = [Record(),
            Record(temperature=1.0),
            Record(temperature=0.7, top_k=5),
            Record(temperature=1.3, top_p=0.8, min_p=0.05),
            Record(repetition_penalty=1.3, no_repeat_ngram_size=2, sequence_list=0),
            Record(temperature=1.0, top_k=50, top_p=0.9, repetition_penalty=0.8, no_repeat_ngram_size=3, sequence_list=1)]
    if reverse:
        recs = recs[::-1]
    return [replace(r, seed=seed + s) for s, r in enumerate(recs)]


def kernel_case(V: int, reverse: bool = False, seed_offset=None):
    """(rows [6][V], hists, records, lists) of one call."""
    rng = np.random.default_rng(4242 + 7 * V + (1 if reverse else 0))
    rows = (rng.standard_normal((6, V)) * 3.0).astype(np.float32)
    rows[np.abs(rows) < 1e-3] = np.float32(0.5)
    rows[:, 1] = NEG_INF
    rows[:, 2] = np.float32(0.0)
    lens = list(LENS)
    if V == 8225:
        lens[5] = LONG_T
    hists = [P.kernel_history(V, t, 3, 0, s) for s, t in enumerate(lens)]
    off = SEEDS[(V, reverse)] if seed_offset is None else seed_offset
    recs = records(SEED0 + 1000 * off, reverse)
    h5 = hists[[r.sequence_list for r in recs].index(0)]
    h6 = hists[[r.sequence_list for r in recs].index(1)]
    list0 = [((SHARED,), 1.5), ((5, 9), -2.0)] + ([((h5[-1], 20), 3.0)] if h5 else [])
    list1 = [((SHARED,), -0.75), (tuple(h6[-2:]) + (FIRED,), 4.0), ((BANNED,), float("-inf")), ((5, 9), 0.5)]
    return rows, hists, recs, [list0, list1]


def all_cases():
    """Every small vocabulary with the table both ways round, the real one once."""
    return [(V, rev) for V in KERNEL_V for rev in (False, True)] + [(BIG_V, False)]
