"""Reference arithmetic for the logit bias tests (numpy only): the dense vector q3a_set_logit_bias composes, the argmax under
the engine's tie rule, float64 log_softmax with -inf entries, and the three bias kinds the GPU tests use."""
from __future__ import annotations

import numpy as np

EOS_IDS = (151643, 151645)
TOL_SUM = 2.0 ** -22  # |l' - (l + b)| <= TOL_SUM * (|l| + |b|): one rounding of l, one of the sum (include/q3asr.h)


def dense(vocab: int, ids, bias, default: float = 0.0) -> np.ndarray:
    """b = default everywhere, then b[ids[i]] = bias[i] (fp32)."""
    b = np.full(vocab, default, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.int64)
    assert len(set(ids.tolist())) == len(ids), "duplicate id"
    if len(ids):
        assert ids.min() >= 0 and ids.max() < vocab
        b[ids] = np.asarray(bias, dtype=np.float32)
    assert not np.isnan(b).any() and not (b == np.inf).any() and np.isfinite(b).any()
    return b


def argmax(x) -> int:
    """Larger value, then smaller id (np.argmax returns the first maximum); -inf is a legal value, NaN is not."""
    x = np.asarray(x)
    assert not np.isnan(x).any()
    return int(np.argmax(x))


def log_softmax64(x) -> np.ndarray:
    """float64 log_softmax along the last axis; -inf entries contribute 0 to the sum and stay -inf."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    assert np.isfinite(m).all()
    with np.errstate(divide="ignore"):
        return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def sum_tolerance(l, b) -> np.ndarray:
    return TOL_SUM * (np.abs(np.asarray(l, dtype=np.float64)) + np.abs(np.asarray(b, dtype=np.float64)))


def kind_suppress(vocab: int, emitted, top: int) -> dict:
    """(a) every id an unbiased run emitted plus the 6144-id range that starts 2048 below the 2048-aligned chunk of `top` (clipped):
    at least one whole partial of every producer -- 16-row blocks, 64-column tiles, V/128 slices, 2048-logit chunks -- is all -inf."""
    lo = max(0, (int(top) // 2048) * 2048 - 2048)
    ids = set(int(t) for t in emitted) | set(range(lo, min(vocab, lo + 6144)))
    return {t: -np.inf for t in sorted(ids)}


def kind_small(vocab: int, emitted, top: int, seed: int = 7) -> dict:
    """(b) = (a) plus finite biases in +-[0.05, 2] on 64 seeded ids that include id 0 and id V - 1 (suppression wins on a clash)."""
    out = kind_suppress(vocab, emitted, top)
    rng = np.random.default_rng(seed)
    ids = sorted(set(rng.choice(vocab, 62, replace=False).tolist()) | {0, vocab - 1})
    mag = rng.uniform(0.05, 2.0, len(ids)) * rng.choice([-1.0, 1.0], len(ids))
    for t, v in zip(ids, mag):
        out.setdefault(int(t), float(np.float32(v)))
    return out


def kind_allow(vocab: int, seed: int = 11):
    """(c) an allow-list: 1000 seeded ids plus both EOS ids at 0, everything else -inf.  Returns (bias dict, default)."""
    rng = np.random.default_rng(seed)
    ids = sorted(set(rng.choice(vocab, 1000, replace=False).tolist()) | set(EOS_IDS))
    return {int(t): 0.0 for t in ids}, -np.inf


def as_dense(vocab: int, bias: dict, default: float = 0.0) -> np.ndarray:
    ids = sorted(bias)
    return dense(vocab, ids, [bias[t] for t in ids], default)
