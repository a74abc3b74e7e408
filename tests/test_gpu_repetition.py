"""Repetition penalty and no-repeat n-grams on the GPU (q3a_set_repetition; k_repeat.hip): the kernel against the numpy reference
through q3a_selftest_repeat, every lm_head form feeding it, graph replay against the eager stage API, the way back to the plain
engine, the composition with sampling, the logit bias, scoring and beam search, the refusals, the CLI, AsrInference and the device
memory across cycles.

Nothing about the rewritten logits is measured: the device and the reference do the same single fp32 rounding per entry, so l'' is
compared bit for bit (uint32 view) and the id exactly (ties resolve by the smaller id).  Log-probabilities lie within 1e-4 of float64
log_softmax(l'')[id], the project's existing bound."""
import json
import os
import subprocess

import numpy as np
import pytest

import logit_bias_ref as B_
import repetition_ref as R
import sampling_ref as S_
from align_ref import tiny_aligner_dir
from qwen3_asr_rs_amd import _lib, synthetic
from qwen3_asr_rs_amd.engine import AsrInference, HipEngine, Q3aError

pytestmark = pytest.mark.gpu

V = 151936
C = _lib.C
LP_TOL = 1e-4
SAMPLE_EPS = 7.1e-6     # the sampler's id rule (tests/test_gpu_sampling.py EPS)
SEED = (5 << 32) + 77


def _selftest(rows, hists, p, n):
    lib = _lib.load()
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    S, Vr = rows.shape
    stride = max(1, max(len(h) for h in hists))
    hist = np.zeros((S, stride), np.int32)
    for s, h in enumerate(hists):
        hist[s, :len(h)] = h
    lens = np.array([len(h) for h in hists], np.int32)
    out, ids, lp = np.zeros_like(rows), np.full(S, -7, np.int32), np.zeros(S, np.float32)
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    rc = lib.q3a_selftest_repeat(0, rows.ctypes.data_as(f32p), S, Vr, hist.ctypes.data_as(i32p), stride, lens.ctypes.data_as(i32p),
                                 C.c_float(p), n, out.ctypes.data_as(f32p), ids.ctypes.data_as(i32p), lp.ctypes.data_as(f32p))
    assert rc == 0, lib.q3a_last_error(None)
    return out, ids, lp


# ---- 1. the kernel against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("Vk", list(R.KERNEL_V) + [R.BIG_V])
def test_kernel_against_the_reference(Vk):
    """V = 1, 31, 32, 33 (the bitmap's word edge), 2049 (a ragged last word), 6150, 8225 (258 words: more than one per thread),
    151936 once; S = 1 and 3 with lengths that differ; t = 0, 1, n - 1, n, 255, 256, 257, 1023; n = 0, 1, 2,
    3, 5; p = 1, 1.3, 0.8; at V = 6150 also one history of 4200 ids, longer than the kernel's LDS copy (4096), whose tail is read in
    place; histories as tests/test_repetition_host.py holds them."""
    worst_lp, rows_seen = 0.0, 0
    for S, rows, hists, p, n in R.kernel_cases(Vk):
        want = R.apply_rows(rows, hists, p, n)
        out, ids, lp = _selftest(rows, hists, p, n)
        where = (Vk, S, [len(h) for h in hists], p, n)
        assert np.array_equal(R.bits(out), R.bits(want)), (where, np.nonzero(R.bits(out) != R.bits(want)))
        for s in range(S):
            rows_seen += 1
            if not np.isfinite(want[s]).any():
                continue                                                 # (V = 1 with its only id banned: no id is specified)
            assert int(ids[s]) == R.argmax(want[s]), (where, s, int(ids[s]), R.argmax(want[s]))
            ref = float(R.log_softmax64(want[s])[int(ids[s])])
            worst_lp = max(worst_lp, abs(float(lp[s]) - ref))
            assert abs(float(lp[s]) - ref) <= LP_TOL, (where, s, float(lp[s]), ref)
    print(f"[repetition] V={Vk}: {rows_seen} rows bit-equal, largest |lp - log_softmax64| {worst_lp:.2e}")


# ---- 2. every head form ------------------------------------------------------------------------------------------------------
def _clips(n, seed0=40, base=1.0):
    return [synthetic.synthetic_clip(seed0 + i, base + 0.25 * (i % 4)) for i in range(n)]


def _prompts(eng):
    return [HipEngine.build_prompt(t) for t in eng._T]


def _forced_pair(a, b, clips, steps):
    """Engine b (with its setting) runs `steps` steps through the stage API; engine a (never had the setting) is teacher-forced with b's
    ids, so it runs the same head kernels on the same inputs and its logits_out is b's l'.  Returns (l' [steps][B][V], b's logits_out,
    b's ids [steps][B])."""
    for e in (a, b):
        e.mel(clips)
        e.encode()
    la, _ = a.prefill(_prompts(a))
    lb, nb = b.prefill(_prompts(b))
    LA, LB, TB = [la.copy()], [lb.copy()], [nb.copy()]
    for _ in range(steps - 1):
        a.set_next_tokens(TB[-1])
        la, _, _ = a.decode_step()
        lb, nb, _ = b.decode_step()
        LA.append(la.copy())
        LB.append(lb.copy())
        TB.append(nb.copy())
    return np.stack(LA), np.stack(LB), np.stack(TB)


@pytest.mark.parametrize("precise,B", [(False, 1), (False, 2), (False, 5), (False, 32), (False, 40), (True, 5)])
def test_every_head_form_feeds_the_kernel(tiny_dir, precise, B):
    """B = 1 the fused-norm GEMV head (the pruned pair must not be taken), 2 the two-sequence GEMV, 5 / 32 the gemm16 form, 40 and the
    precise mode the stored-logits forms: 12 steps at p = 1.3, n = 2.  At every step reference(l' of the engine without the setting,
    the history) is the engine's logits_out bit for bit, the id is its argmax and the log-probability is log_softmax(l'')[id].
    The case bites: the fp32 oracle's unconstrained greedy ids of clips 40..43 on this checkpoint open with 4481, 4481 (clip 42: eight
    times), so the unconstrained run repeats inside the 12 steps, the constrained ids differ, and with n = 1 all ids are distinct."""
    steps, p, n = 12, 1.3, 2
    clips = _clips(B)
    a = HipEngine(tiny_dir, 0, precise=precise, max_new_tokens=16, token_logprobs=True)
    b = HipEngine(tiny_dir, 0, precise=precise, max_new_tokens=16, token_logprobs=True)
    try:
        free = a.transcribe_batch(clips, None, max_new=steps, fixed_new_tokens=steps)
        b.set_repetition(p, n)
        assert b.repetition_stats() == {"active": True, "repetition_penalty": float(np.float32(p)), "no_repeat_ngram_size": n}
        LA, LB, TB = _forced_pair(a, b, clips, steps)
        lps = b.fetch_logprobs()
        ids = b.fetch_ids(16)
        b.set_repetition(1.0, 1)
        distinct = b.transcribe_batch(clips, None, max_new=steps, fixed_new_tokens=steps)
    finally:
        a.close()
        b.close()
    assert not np.isnan(LA).any()
    worst_lp, changed = 0.0, 0
    for q in range(B):
        col = [int(x) for x in TB[:, q]]
        for t in range(steps):
            want = R.apply(LA[t][q], col[:t], p, n)
            assert np.array_equal(R.bits(want), R.bits(LB[t][q])), (precise, B, q, t, np.nonzero(R.bits(want) != R.bits(LB[t][q])))
            assert col[t] == R.argmax(want), (precise, B, q, t)
            changed += int(not np.array_equal(R.bits(want), R.bits(LA[t][q])))
        stop = next((i for i, x in enumerate(col) if x in B_.EOS_IDS), steps)
        assert ids[q] == col[:stop] and len(lps[q]) == stop
        for t in range(stop):
            ref = float(R.log_softmax64(LB[t][q])[col[t]])
            worst_lp = max(worst_lp, abs(float(lps[q][t]) - ref))
            assert abs(float(lps[q][t]) - ref) <= LP_TOL, (q, t, float(lps[q][t]), ref)
        assert all(col[i:i + 2] != col[j:j + 2] for i in range(steps - 1) for j in range(i + 1, steps - 1))   # no 2-gram twice
    assert all(len(set(u)) < len(u) for u in free[:4])                     # the unconstrained ids repeat a token ...
    assert [list(TB[:, q]) for q in range(B)] != free                      # ... and the constrained ones are others
    assert all(len(x) == steps and len(set(x)) == steps for x in distinct)   # n = 1: every id once
    assert changed >= B * (steps - 1)                                      # every step past the prefill's rewrote its row
    print(f"[repetition] precise={precise} B={B}: {B * steps} rows bit-equal to the reference, worst |lp - log_softmax64| {worst_lp:.2e}")


# ---- 3. graph and eager, another setting on the same graph, and the way back -------------------------------------------------
def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _stats(eng):
    return eng.debug_read_raw("lm_head_prune_stats").view(np.int32).copy()


def _captures(eng):
    return int(eng.debug_read_raw("graph_captures").view(np.int32)[0])


def _stage_ids(eng, clips, kmax):
    eng.mel(clips)
    eng.encode()
    _, nxt = eng.prefill(_prompts(eng))
    T = [nxt.copy()]
    for _ in range(kmax - 1):
        T.append(eng.decode_step()[1].copy())
    return np.stack(T)


def _eos_bias(model_dir, clips, gap=0.1):
    """A bias on <|im_end|> that puts it `gap` under clip 0's best prefill logit: once the penalty and the ban have pushed a few
    favourites down, EOS wins -- natural EOS at ragged lengths."""
    eng = HipEngine(model_dir, 0, max_new_tokens=4)
    try:
        eng.mel(clips[:1])
        eng.encode()
        l, _ = eng.prefill([HipEngine.build_prompt(eng._T[0])])
    finally:
        eng.close()
    return {151645: float(np.float32(l[0].max() - gap - l[0][151645]))}


@pytest.mark.parametrize("B", [1, 5])
def test_graph_eager_other_setting_and_back(tiny_dir, B):
    clips, kmax = _clips(B, 80, 1.5), 12
    bias = _eos_bias(tiny_dir, clips)
    fresh = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True)       # never has the setting
    plain = fresh.transcribe_batch(clips, None, max_new=kmax), fresh.fetch_logprobs(), _stats(fresh)
    fresh.close()
    eager = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True, use_graph=False)
    try:
        eager.set_logit_bias(bias)
        eager.set_repetition(1.3, 2)
        T = _stage_ids(eager, clips, kmax)
        want, want_lp = eager.fetch_ids(kmax), eager.fetch_logprobs()
    finally:
        eager.close()
    for q in range(B):
        col = [int(x) for x in T[:, q]]
        assert want[q] == col[:next((i for i, x in enumerate(col) if x in B_.EOS_IDS), kmax)]
    eng = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True)
    try:
        eng.set_logit_bias(bias)
        eng.set_repetition(1.3, 2)
        r1 = eng.transcribe_batch(clips, None, max_new=kmax), eng.fetch_logprobs()
        r2 = eng.transcribe_batch(clips, None, max_new=kmax), eng.fetch_logprobs()
        assert r1[0] == want, (r1[0], want)                                        # graph replay, natural EOS == the eager stage API
        assert all(0 < len(x) < kmax for x in r1[0])                               # every sequence stopped at its own EOS
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(r1[1], want_lp))
        assert r2[0] == r1[0] and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(r1[1], r2[1]))   # bit-identical twice
        g0 = _captures(eng)
        assert g0 >= 1
        eng.set_repetition(0.5, 0)                                                 # another (p, n) -- a reward: the same graph, other ids
        assert eng.repetition_stats() == {"active": True, "repetition_penalty": 0.5, "no_repeat_ngram_size": 0}
        r3 = eng.transcribe_batch(clips, None, max_new=kmax)
        print(f"[repetition] B={B}: natural-EOS lengths {[len(x) for x in r1[0]]} / other setting {[len(x) for x in r3]}")
        assert _captures(eng) == g0 and r3 != r1[0]
        # back: the ids, log-probabilities and pruned-argmax passes of an engine that never had the setting
        eng.set_logit_bias(None)
        eng.set_repetition(1.0, 0)
        with pytest.raises(Q3aError, match="nothing generated"):                   # the decode state is dropped
            eng.fetch_ids(kmax)
        assert eng.repetition_stats() == {"active": False, "repetition_penalty": 1.0, "no_repeat_ngram_size": 0}
        s0 = _stats(eng)
        back = eng.transcribe_batch(clips, None, max_new=kmax), eng.fetch_logprobs()
        s1 = _stats(eng)
    finally:
        eng.close()
    assert back[0] == plain[0] and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(back[1], plain[1]))
    assert (s0 == 0).all(), s0                                                     # no pruned pass ran while the setting was on ...
    assert (s1 - s0 == plain[2]).all(), (s0, s1, plain[2])                          # ... and afterwards as on the fresh engine
    print(f"[repetition] B={B}: plain lengths {[len(x) for x in plain[0]]}")


def test_pruned_argmax_returns_after_the_setting(tiny_dir):
    """One sequence without token log-probabilities: the greedy step is the pruned pair.  While the setting is on it is not taken;
    after set_repetition(1, 0) the passes advance exactly as on a fresh engine and the ids are its ids."""
    clip, steps = synthetic.synthetic_clip(0, 9.3), 16
    never = HipEngine(tiny_dir, 0, max_new_tokens=steps)
    want = never.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)
    s_never = _stats(never)
    never.close()
    assert s_never[1] >= steps - 1
    eng = HipEngine(tiny_dir, 0, max_new_tokens=steps)
    try:
        eng.set_repetition(1.3, 3)
        a = eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)
        assert a != want and len(a[0]) == steps and (_stats(eng) == 0).all()
        assert eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps) == a
        eng.set_repetition(1.0, 0)
        assert eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps) == want
        assert (_stats(eng) == s_never).all(), (_stats(eng), s_never)
    finally:
        eng.close()


# ---- 4. composition ----------------------------------------------------------------------------------------------------------
def test_sampling_draws_from_the_rewritten_row(tiny_dir):
    """set_sampling(T = 1) over set_repetition(1.3, 2): at every step the engine's logits_out is the reference's l'' of the plain
    engine's l', and the drawn id is sampling_ref's draw from that l'' with the same (seed, s, t)."""
    steps, B, p, n = 10, 3, 1.3, 2
    clips = _clips(B, 60, 1.25)
    a = HipEngine(tiny_dir, 0, max_new_tokens=16, token_logprobs=True)
    b = HipEngine(tiny_dir, 0, max_new_tokens=16, token_logprobs=True)
    try:
        b.set_repetition(p, n)
        b.set_sampling(1.0, 0.0, SEED)
        LA, LB, TB = _forced_pair(a, b, clips, steps)
        lps = b.fetch_logprobs()
    finally:
        a.close()
        b.close()
    under = 0
    for q in range(B):
        col = [int(x) for x in TB[:, q]]
        stop = next((i for i, x in enumerate(col) if x in B_.EOS_IDS), steps)
        for t in range(steps):
            want = R.apply(LA[t][q], col[:t], p, n)
            assert np.array_equal(R.bits(want), R.bits(LB[t][q])), (q, t)
            d = S_.sample(want, 1.0, 0.0, SEED, q, t)
            if d.margin > SAMPLE_EPS:
                assert col[t] == d.id, (q, t, col[t], d.id, d.second, d.margin)
            else:
                assert col[t] in (d.id, d.second), (q, t)
                under += 1
            assert np.isfinite(want[col[t]])                              # a banned id is never drawn
            if t < stop:
                assert abs(float(lps[q][t]) - float(R.log_softmax64(want)[col[t]])) <= LP_TOL, (q, t)
        assert all(col[i:i + 2] != col[j:j + 2] for i in range(steps - 1) for j in range(i + 1, steps - 1))
    assert under <= 0.01 * steps * B + 1


def test_composition_with_the_logit_bias_score_and_beam(tiny_dir):
    clips, kmax = _clips(3, 70, 1.5), 12
    eng = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True)
    try:
        plain = eng.transcribe_batch(clips, None, max_new=kmax, fixed_new_tokens=kmax)
        targets = [x[:6] + [151645] for x in plain]
        score_off = eng.score_batch(clips, targets)
        eng.set_repetition(1.3, 2)
        rep_only = eng.transcribe_batch(clips, None, max_new=kmax, fixed_new_tokens=kmax)
        sup = B_.kind_suppress(V, set(t for x in plain + rep_only for t in x), rep_only[0][0])
        dense = B_.as_dense(V, sup)
        eng.set_logit_bias(sup)
        got = eng.transcribe_batch(clips, None, max_new=kmax, fixed_new_tokens=kmax)
        assert all(len(x) == kmax for x in got) and all(np.isfinite(dense[t]) for x in got for t in x)   # no suppressed id, ever
        assert got != rep_only and got != plain
        assert all(x[i:i + 2] != x[j:j + 2] for x in got for i in range(kmax - 1) for j in range(i + 1, kmax - 1))
        score_on = eng.score_batch(clips, targets)                       # q3a_score* never sees the setting (or the bias)
        for x, y in zip(score_off, score_on):
            assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(x[1], y[1]) and np.array_equal(_bits(x[2]), _bits(y[2]))
        eng.set_logit_bias(None)
        # beam search while the setting is on is refused, in both forms
        with pytest.raises(Q3aError, match="repetition control is on"):
            eng.beam_search_batch(clips[:1], 2, max_new=4)
        rep = [clips[0]] * 2
        eng.mel(rep)
        eng.encode()
        eng.prefill(_prompts(eng))
        with pytest.raises(Q3aError, match="repetition control is on"):
            eng.beam_begin(2)
        eng.set_repetition(1.0, 0)
        assert len(eng.beam_search_batch(clips[:1], 2, max_new=4)[0]) == 2
    finally:
        eng.close()


# ---- 5. refusals and state ---------------------------------------------------------------------------------------------------
def test_refusals_and_state(tiny_dir):
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8)
    lib = eng._lib
    try:
        eng.set_repetition(1.3, 3)
        for p, n, msg in [(0.0, 0, "repetition_penalty"), (-1.0, 0, "repetition_penalty"), (float("nan"), 0, "repetition_penalty"),
                          (float("inf"), 0, "repetition_penalty"), (1.0, -1, "no_repeat_ngram_size"), (1.0, 33, "no_repeat_ngram_size")]:
            with pytest.raises(Q3aError, match=msg):
                eng._chk(lib.q3a_set_repetition(eng._h, C.c_float(p), n))
            st = eng.repetition_stats()                                  # a refused call changes nothing
            assert st == {"active": True, "repetition_penalty": float(np.float32(1.3)), "no_repeat_ngram_size": 3}
        eng.set_repetition(1.0, 32)                                      # the largest n; the penalty alone off is still on
        assert eng.repetition_stats()["active"] is True
        eng.set_repetition(0.8, 0)
        assert eng.repetition_stats() == {"active": True, "repetition_penalty": float(np.float32(0.8)), "no_repeat_ngram_size": 0}
        clip = synthetic.synthetic_clip(3, 1.0)
        eng.mel([clip])
        eng.encode()
        eng.prefill([HipEngine.build_prompt(eng._T[0])])
        eng.decode_step()
        eng.set_repetition(1.3, 2)                                       # a successful call drops the decode state
        with pytest.raises(Q3aError):
            eng.decode_step()
        with pytest.raises(Q3aError, match="no decode state"):
            eng.set_next_tokens([5])
        # an n-gram ban over a bias that forbids both EOS ids and leaves no more tokens finite than max_new_tokens (8): refused by
        # whichever setter comes second, and the refused call changes nothing
        allow8 = {t: 0.0 for t in range(100, 108)}
        with pytest.raises(Q3aError, match="run out of finite logits"):
            eng.set_logit_bias(allow8, -np.inf)
        assert eng.logit_bias_stats() == {"active": False, "finite": V}
        eng.set_logit_bias({t: 0.0 for t in range(100, 109)}, -np.inf)   # nine finite tokens: more than max_new_tokens
        eng.set_logit_bias({**allow8, 151645: 0.0}, -np.inf)       # an EOS id stays open
        eng.set_repetition(1.3, 0)                                       # the penalty alone never empties a row
        eng.set_logit_bias(allow8, -np.inf)
        with pytest.raises(Q3aError, match="run out of finite logits"):
            eng.set_repetition(1.3, 1)
        assert eng.repetition_stats()["no_repeat_ngram_size"] == 0
        eng.set_logit_bias(None)
        eng.set_repetition(1.3, 1)
    finally:
        eng.close()
    al = HipEngine(tiny_aligner_dir(), 0, max_new_tokens=1)
    try:
        with pytest.raises(Q3aError, match="forced aligner"):            # an aligner engine generates nothing
            al.set_repetition(1.3, 2)
        with pytest.raises(Q3aError, match="forced aligner"):
            al.repetition_stats()
    finally:
        al.close()


# ---- 6. AsrInference and the CLI ---------------------------------------------------------------------------------------------
class _Tok:
    def decode(self, ids, skip):
        return "language English<asr_text>" + " ".join(f"t{i}" for i in ids)

    def encode(self, text):
        return []


def test_asr_inference_arguments(tiny_dir):
    clip = synthetic.synthetic_clip(12, 1.5)
    asr = AsrInference.load(tiny_dir, 0, token_logprobs=True, max_new_tokens=16)
    try:
        asr.tokenizer = _Tok()
        eng = asr.engine
        plain = asr.transcribe(clip, max_new_tokens=8)
        assert len(plain.ids) == 8 and len(set(plain.ids)) < 8            # the plain transcript repeats a token
        a = asr.transcribe(clip, max_new_tokens=8, repetition_penalty=1.3, no_repeat_ngram_size=1)
        assert a.ids != plain.ids and len(set(a.ids)) == len(a.ids) == 8
        assert eng.repetition_stats()["active"] is False and eng.repetition_state == (1.0, 0)   # restored
        eng.set_repetition(1.3, 1)
        assert eng.transcribe_batch([clip], None, 8) == [a.ids]
        # the engine's own setting is the default of a call without the arguments, and is restored after one with them
        b = asr.transcribe(clip, max_new_tokens=8, repetition_penalty=2.0)
        assert eng.repetition_state == (1.3, 1) and eng.repetition_stats()["no_repeat_ngram_size"] == 1
        eng.set_repetition(2.0, 0)
        assert eng.transcribe_batch([clip], None, 8) == [b.ids]
        eng.set_repetition(1.0, 0)
        # a temperature tuple: every attempt of the fallback runs under the same setting (a random checkpoint fails every attempt, the
        # last one, T = 1 with seed + 1, is kept)
        res = asr.transcribe(clip, max_new_tokens=8, temperature=(0.0, 1.0), seed=4, no_repeat_ngram_size=1)
        eng.set_repetition(1.0, 1)
        eng.set_sampling(1.0, 0.0, 5)
        want = eng.transcribe_batch([clip], None, 8)[0]
        eng.set_sampling(0.0)
        eng.set_repetition(1.0, 0)
        assert res.temperature == 1.0 and res.ids == want and len(set(res.ids)) == len(res.ids)
        assert asr.transcribe(clip, max_new_tokens=8).ids == plain.ids
        with pytest.raises(Q3aError, match="beam"):
            asr.transcribe(clip, max_new_tokens=4, beam_size=2, no_repeat_ngram_size=2)
        with pytest.raises(Q3aError, match="repetition_penalty"):
            asr.transcribe(clip, max_new_tokens=4, repetition_penalty=0.0)
    finally:
        asr.engine.close()


def test_cli_environment_variables(tiny_dir, tmp_path):
    """Q3A_REPETITION_PENALTY / Q3A_NO_REPEAT_NGRAM through the CLI give the text of the Python call (token t<i> decodes to "t<i>")."""
    from qwen3_asr_rs_amd.build import CLI_PATH
    mdir = tmp_path / "model"
    mdir.mkdir()
    for f in os.listdir(tiny_dir):
        if f.endswith((".json", ".safetensors")):
            os.symlink(os.path.join(tiny_dir, f), mdir / f)
    vocab = {f"t{i}": i for i in range(V) if i not in B_.EOS_IDS}
    tok = {"version": "1.0", "added_tokens": [{"id": 151643, "content": "<|endoftext|>", "special": True},
                                              {"id": 151645, "content": "<|im_end|>", "special": True}],
           "model": {"type": "BPE", "vocab": vocab, "merges": []}}
    (mdir / "tokenizer.json").write_text(json.dumps(tok))
    wav = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_audio", "sample1.wav")
    asr = AsrInference.load(str(mdir), 0)
    plain = asr.transcribe(wav)
    want = asr.transcribe(wav, repetition_penalty=1.3, no_repeat_ngram_size=2)
    asr.engine.close()
    assert want.ids != plain.ids
    env = {k: v for k, v in os.environ.items() if not k.startswith("Q3A_")}
    env.update(RUST_LOG="warn", Q3A_REPETITION_PENALTY="1.3", Q3A_NO_REPEAT_NGRAM="2")
    out = subprocess.run([CLI_PATH, str(mdir), wav], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    assert lines[0] == f"Language: {want.language}" and lines[1] == f"Text: {want.text}" and want.text != plain.text
    bad = subprocess.run([CLI_PATH, str(mdir), wav], capture_output=True, text=True, timeout=300, env=dict(env, Q3A_NO_REPEAT_NGRAM="40"))
    assert bad.returncode == 1 and "Repetition control failed" in bad.stderr and "no_repeat_ngram_size" in bad.stderr
    bad = subprocess.run([CLI_PATH, str(mdir), wav], capture_output=True, text=True, timeout=300, env=dict(env, Q3A_REPETITION_PENALTY="strong"))
    assert bad.returncode == 1 and "Q3A_REPETITION_PENALTY is not a number" in bad.stderr


# ---- 7. no leak --------------------------------------------------------------------------------------------------------------
def test_device_memory_is_level_across_cycles(tiny_dir):
    clips = _clips(2, 90, 1.0)

    def cycle():
        eng = HipEngine(tiny_dir, 0, max_new_tokens=8, token_logprobs=True)
        eng.set_repetition(1.3, 2)
        eng.transcribe_batch(clips, None, max_new=6, fixed_new_tokens=6)
        inside = int(eng.debug_read_raw("device_bytes").view(np.uint64)[0])
        eng.set_repetition(1.0, 0)
        eng.transcribe_batch(clips, None, max_new=6, fixed_new_tokens=6)
        eng.close()
        return inside

    probe = HipEngine(tiny_dir, 0, max_new_tokens=8)
    try:
        base = int(probe.debug_read_raw("device_bytes").view(np.uint64)[0])
        first = cycle()
        level = int(probe.debug_read_raw("device_bytes").view(np.uint64)[0])
        for _ in range(3):
            assert cycle() == first
            assert int(probe.debug_read_raw("device_bytes").view(np.uint64)[0]) == level
        assert level == base
    finally:
        probe.close()
