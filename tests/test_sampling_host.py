"""Sampling without a GPU: the host's q3a_sample_word against the numpy Philox bit for bit, the published known-answer vector, the
distribution of the reference's draws, the inputs the GPU kernel test relies on, the fallback decision and the refusals."""
import math

import numpy as np
import pytest

import sampling_ref as R
from qwen3_asr_rs_amd.engine import (Q3aError, attempt_acceptable, check_sampling_args, compression_ratio, temperature_fallback)


def test_known_answer_vector():
    """Random123's kat_vectors entry for Philox4x32-10 with an all-zero counter and key; and the all-ones entry."""
    assert [int(x) for x in R.philox4x32((0, 0, 0, 0), (0, 0))] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert [int(x) for x in R.philox4x32((f, f, f, f), (f, f))] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_host_word_equals_the_reference_bit_for_bit(lib):
    rng = np.random.default_rng(5)
    edge = [0, 1, 2 ** 32 - 1, 2 ** 31, 151935]
    seeds = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 12345, 2 ** 64 - 1] + [int(x) for x in rng.integers(0, 2 ** 63, 6)]
    cases = [(sd, s, t, j) for sd in seeds[:6] for s in edge[:3] for t in edge[:3] for j in edge]
    n = 4000 - len(cases)
    cases += [(seeds[int(i) % len(seeds)], int(a), int(b), int(c)) for i, a, b, c in
              zip(rng.integers(0, 1000, n), rng.integers(0, 2 ** 32, n), rng.integers(0, 2 ** 32, n), rng.integers(0, 2 ** 32, n))]
    for sd in set(c[0] for c in cases):
        sub = [c for c in cases if c[0] == sd]
        want = R.sample_word(sd, [c[1] for c in sub], [c[2] for c in sub], [c[3] for c in sub])
        got = np.array([lib.q3a_sample_word(sd, s, t, j) for _, s, t, j in sub], dtype=np.uint32)
        assert np.array_equal(got, want), sd
    assert lib.q3a_sample_word(0, 0, 0, 0) == 0x6627E8D5


def test_uniform_is_strictly_inside_the_unit_interval():
    u = R.uniform(np.array([0, 255, 256, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32))
    assert u[0] == 2.0 ** -25 and u[1] == u[0] and u[-1] == 1.0 - 2.0 ** -25 and (u > 0).all() and (u < 1).all()
    assert np.isfinite(R.gumbel(u)).all()


def _chi2_sf(x: float, k: int) -> float:
    """P(chi-square with k degrees of freedom > x) = Q(k / 2, x / 2): series below a + 1, continued fraction above (Lentz)."""
    a, x = k / 2.0, x / 2.0
    if x <= 0:
        return 1.0
    lg = math.lgamma(a)
    if x < a + 1.0:
        term = total = 1.0 / a
        n = a
        for _ in range(10000):
            n += 1.0
            term *= x / n
            total += term
            if abs(term) < abs(total) * 1e-15:
                break
        return 1.0 - total * math.exp(-x + a * math.log(x) - lg)
    tiny = 1e-300
    b = x + 1.0 - a
    c, d = 1.0 / tiny, 1.0 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-15:
            break
    return math.exp(-x + a * math.log(x) - lg) * h


def test_chi2_helper():
    assert abs(_chi2_sf(3.841458820694124, 1) - 0.05) < 1e-9 and abs(_chi2_sf(18.307038053275146, 10) - 0.05) < 1e-9
    assert abs(_chi2_sf(2.0, 10) - 0.996340153172656) < 1e-9


def test_reference_draws_follow_the_restricted_softmax():
    """One row of 100 logits, T = 0.7, min_p = 0.05, 8192 draws over (s, t): nothing outside K is drawn, and a chi-square test
    against the analytic restricted softmax passes at p > 0.01 (cells with an expectation under 5 pooled)."""
    T, min_p, seed, n_s, n_t = 0.7, 0.05, 2024, 64, 128
    row = (np.random.default_rng(9).standard_normal(100) * 1.5).astype(np.float32)
    p = R.restricted_softmax(row, T, min_p)
    keep, _ = R.kept_set(row, T, min_p)
    assert 3 <= keep.sum() < 100 and keep[np.argmax(row)] and abs(p.sum() - 1.0) < 1e-12 and (p[~keep] == 0).all()
    # the rule on probabilities: p_j >= min_p * p_max at temperature T
    full = np.exp(R.log_softmax64(row.astype(np.float64) / np.float32(T)))
    assert np.array_equal(keep, full >= np.float32(min_p) * full.max() * (1 - 1e-12))
    counts = np.zeros(100, dtype=np.int64)
    for s in range(n_s):
        for t in range(n_t):
            counts[R.sample(row, T, min_p, seed, s, t).id] += 1
    n = n_s * n_t
    assert counts.sum() == n == 8192 and (counts[~keep] == 0).all()
    exp = p * n
    big = keep & (exp >= 5.0)
    obs_cells, exp_cells = list(counts[big]), list(exp[big])
    if (keep & ~big).any():
        obs_cells.append(counts[keep & ~big].sum())
        exp_cells.append(exp[keep & ~big].sum())
    chi2 = float(sum((o - e) ** 2 / e for o, e in zip(obs_cells, exp_cells)))
    pv = _chi2_sf(chi2, len(obs_cells) - 1)
    print(f"[sampling] chi-square {chi2:.2f} on {len(obs_cells) - 1} degrees of freedom, p = {pv:.3f}; |K| = {int(keep.sum())}")
    assert pv > 0.01


def test_reference_edge_rules():
    row = np.array([1.0, -np.inf, 3.0, 3.0, 2.9], dtype=np.float32)
    for t in range(50):
        d = R.sample(row, 1.0, 0.0, 3, 0, t)
        assert d.id != 1 and not d.kept[1] and d.kept.sum() == 4          # -inf is never kept, every finite logit is
        d = R.sample(row, 1.0, 1.0, 3, 0, t)
        assert d.id in (2, 3) and d.kept.tolist() == [False, False, True, True, False]   # min_p = 1: the maxima alone
        assert R.sample(row, 1e-6, 0.0, 3, 0, t).id in (2, 3)            # T -> 0 runs into the greedy id (a twin here)
    one = np.full(5000, -np.inf, dtype=np.float32)
    one[4321] = -7.0
    d = R.sample(one, 2.0, 0.0, 3, 1, 2)
    assert d.id == 4321 and d.margin == np.inf and d.second == -1 and d.lp == 0.0
    # the noise of a token depends on (seed, s, t, j) alone
    a, b = R.sample(row, 1.0, 0.0, 3, 0, 0), R.sample(np.concatenate([row, [0.5]]).astype(np.float32), 1.0, 0.0, 3, 0, 0)
    assert a.z == b.z or b.id == 5


@pytest.mark.parametrize("V", list(R.KERNEL_V) + [R.BIG_V])
def test_kernel_inputs_have_no_close_calls(V):
    """What tests/test_gpu_sampling.py relies on: over every draw of the kernel test the reference's margin stays above 1e-3 T and no
    logit lies within 1e-4 of a kept-set threshold, so the device's fp32 arithmetic cannot flip a draw or the kept set."""
    rows, calls = R.kernel_rows(V), R.kernel_calls(V)
    if V > R.CHUNK:
        assert any((rows[0, c * R.CHUNK:(c + 1) * R.CHUNK] == -np.inf).all() for c in range(V // R.CHUNK))
    assert int(np.argmax(rows[1])) >= ((V - 1) // R.CHUNK) * R.CHUNK
    if V >= 2:
        assert (rows[2] == rows[2].max()).sum() == 2
    assert np.isfinite(rows[3]).sum() == 1
    draws = R.kernel_draws(V)
    assert len(draws) == 12 * len(R.kernel_combos(V))
    for ci, s, d in draws:
        T = calls[ci][1]
        assert d.margin > 1e-3 * T and d.thr_gap > 1e-4, (V, calls[ci], s, d.margin, d.thr_gap)


class _Res:
    def __init__(self, text, avg_logprob):
        self.text, self.avg_logprob = text, avg_logprob


def _scripted(script):
    calls = []

    def attempt(t, seed):
        calls.append((t, seed))
        return _Res(*script[len(calls) - 1])
    return attempt, calls


TEMPS = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)


def test_fallback_decision():
    loop = "ha " * 200
    assert compression_ratio(loop) > 2.4 and compression_ratio("the quick brown fox jumps over the lazy dog") < 2.4
    assert attempt_acceptable("a fine sentence", -0.3) and not attempt_acceptable("a fine sentence", -1.5)
    assert not attempt_acceptable(loop, -0.1) and attempt_acceptable("", None)
    assert attempt_acceptable("a fine sentence", -1.0) and not attempt_acceptable("a fine sentence", float("nan"))
    # the first acceptable attempt wins; attempt k runs at temperatures[k] with seed + k
    attempt, calls = _scripted([(loop, -0.1), ("guess", -2.0), ("good text", -0.4), ("never reached", 0.0)])
    res, t, n = temperature_fallback(attempt, TEMPS, seed=100)
    assert (res.text, t, n) == ("good text", 0.4, 3) and calls == [(0.0, 100), (0.2, 101), (0.4, 102)]
    # greedy passes: one attempt
    attempt, calls = _scripted([("good text", -0.2)])
    assert temperature_fallback(attempt, TEMPS, seed=7)[1:] == (0.0, 1) and calls == [(0.0, 7)]
    # the last attempt is kept when all fail
    attempt, calls = _scripted([(loop, -0.1)] * 5 + [("last " + loop, -3.0)])
    res, t, n = temperature_fallback(attempt, TEMPS, seed=2 ** 40)
    assert res.text.startswith("last ") and (t, n) == (1.0, 6) and calls == [(x, 2 ** 40 + k) for k, x in enumerate(TEMPS)]
    # the thresholds are the caller's
    attempt, calls = _scripted([(loop, -1.5)])
    assert temperature_fallback(attempt, TEMPS, logprob_threshold=-2.0, compression_ratio_threshold=1e9)[2] == 1
    with pytest.raises(Q3aError, match="no temperature"):
        temperature_fallback(attempt, ())


def test_refusals_that_need_no_device(lib):
    assert check_sampling_args(0, 0, 0) == (0.0, 0.0, 0) and check_sampling_args(0.7, 1.0, 2 ** 64 - 1) == (0.7, 1.0, 2 ** 64 - 1)
    for args, msg in [((-0.1,), "temperature"), ((float("nan"),), "temperature"), ((float("inf"),), "temperature"), (("hot",), "numbers"),
                      ((1.0, -0.01), "min_p"), ((1.0, 1.01), "min_p"), ((1.0, float("nan")), "min_p"),
                      ((1.0, 0.0, -1), "seed"), ((1.0, 0.0, 2 ** 64), "seed"), ((1.0, 0.0, 1.5), "seed")]:
        with pytest.raises(Q3aError, match=msg):
            check_sampling_args(*args)
    # the C entry points: a null engine, and the selftest's arguments before it looks for a device
    C = __import__("ctypes")
    assert lib.q3a_set_sampling(None, C.c_float(1.0), C.c_float(0.0), 0) != 0
    x = np.zeros(4, dtype=np.float32)
    xp = x.ctypes.data_as(C.POINTER(C.c_float))
    for T, p, V, msg in [(0.0, 0.0, 4, b"temperature"), (-1.0, 0.0, 4, b"temperature"), (float("nan"), 0.0, 4, b"temperature"),
                         (1.0, 1.5, 4, b"min_p"), (1.0, -0.5, 4, b"min_p"), (1.0, 0.0, 0, b"bad argument")]:
        assert lib.q3a_selftest_sample(0, xp, 1, V, C.c_float(T), C.c_float(p), 0, 0, None, None, None) != 0
        assert msg in lib.q3a_last_error(None), (T, p, V, lib.q3a_last_error(None))
