"""Sequence bias on the GPU (q3a_set_sequence_bias; k_repeat.hip): the kernel against the numpy reference through
q3a_selftest_seqbias, every lm_head form feeding it, graph replay against the eager stage API, another list on the same graph, the
way back to the plain engine, the composition with sampling, the logit bias, repetition control and scoring, the refusals,
AsrInference, the CLI and the device memory across set / clear cycles.

Nothing about the rewritten logits is measured: the device and the reference do the same fp32 additions in the same order, so l'' is
compared bit for bit (uint32 view) and the id exactly (ties resolve by the smaller id).  Log-probabilities lie within 1e-4 of float64
log_softmax(l'')[id], the bound tests/test_gpu_repetition.py uses for the same quantity."""
import json
import os
import subprocess

import numpy as np
import pytest

import logit_bias_ref as B_
import repetition_ref as Rep
import sampling_ref as S_
import seqbias_ref as R
from align_ref import tiny_aligner_dir
from qwen3_asr_rs_amd import _lib, synthetic
from qwen3_asr_rs_amd.engine import AsrInference, HipEngine, Q3aError, banned_sequences, hotword_sequences

pytestmark = pytest.mark.gpu

V = 151936
C = _lib.C
LP_TOL = 1e-4
SAMPLE_EPS = 7.1e-6     # the sampler's id rule (tests/test_gpu_sampling.py EPS)
SEED = (5 << 32) + 77
NINF = float("-inf")


def _selftest(rows, hists, entries):
    lib = _lib.load()
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    S, Vr = rows.shape
    stride = max(1, max(len(h) for h in hists))
    hist = np.zeros((S, stride), np.int32)
    for s, h in enumerate(hists):
        hist[s, :len(h)] = h
    lens = np.array([len(h) for h in hists], np.int32)
    ids, sl, sb = R.flatten(entries)
    out, tok, lp = np.zeros_like(rows), np.full(S, -7, np.int32), np.zeros(S, np.float32)
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    rc = lib.q3a_selftest_seqbias(0, rows.ctypes.data_as(f32p), S, Vr, hist.ctypes.data_as(i32p), stride, lens.ctypes.data_as(i32p),
                                  ids.ctypes.data_as(i32p), sl.ctypes.data_as(i32p), sb.ctypes.data_as(f32p), len(sl),
                                  out.ctypes.data_as(f32p), tok.ctypes.data_as(i32p), lp.ctypes.data_as(f32p))
    assert rc == 0, lib.q3a_last_error(None)
    return out, tok, lp


# ---- 1. the kernel against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("Vk", list(R.KERNEL_V) + [R.BIG_V])
def test_kernel_against_the_reference(Vk):
    """V = 1, 33, 2049, 8225 and 151936 once; lists of 1, 32, 255, 256, 257, 300 and 4096 entries, with 255 / 256 / 257 / 4096 target
    groups where every entry has a target of its own (the 256-thread stride wraps, 16 groups per thread at the capacity) and up to
    4096 entries on 33 targets (long group walks); entries of 1, 2, 31 and 32 ids; t = 0, 1, 2, 29, 30, 31, 32, 257, 1023 (the LDS
    tail holds min(t, 31) ids; the kernel has no LDS share of max_new, so no history outgrows one); S = 1, and S = 3 with lengths that
    differ; inputs as tests/test_seqbias_host.py holds them."""
    worst_lp, rows_seen = 0.0, 0
    for S, rows, hists, entries in R.kernel_cases(Vk):
        want = R.apply_rows(rows, hists, entries)
        out, ids, lp = _selftest(rows, hists, entries)
        where = (Vk, S, [len(h) for h in hists], len(entries))
        assert np.array_equal(R.bits(out), R.bits(want)), (where, np.nonzero(R.bits(out) != R.bits(want)))
        for s in range(S):
            rows_seen += 1
            if not np.isfinite(want[s]).any():
                continue                                                 # (no finite logit left: no id is specified)
            assert int(ids[s]) == R.argmax(want[s]), (where, s, int(ids[s]), R.argmax(want[s]))
            ref = float(R.log_softmax64(want[s])[int(ids[s])])
            worst_lp = max(worst_lp, abs(float(lp[s]) - ref))
            assert abs(float(lp[s]) - ref) <= LP_TOL, (where, s, float(lp[s]), ref)
    print(f"[sequence bias] V={Vk}: {rows_seen} rows bit-equal, largest |lp - log_softmax64| {worst_lp:.2e}")


# ---- 2. every head form ------------------------------------------------------------------------------------------------------
def _clips(n, seed0=40, base=1.0):
    return [synthetic.synthetic_clip(seed0 + i, base + 0.25 * (i % 4)) for i in range(n)]


def _prompts(eng):
    return [HipEngine.build_prompt(t) for t in eng._T]


def _forced_pair(a, b, clips, steps):
    """Engine b (with its setting) runs `steps` steps through the stage API; engine a (without it) is teacher-forced with b's ids, so
    it runs the same head kernels on the same inputs and its logits_out is b's l'.  Returns (l' [steps][B][V], b's logits_out, b's ids
    [steps][B])."""
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


def _list_from(free, boost=2.0):
    """A list built from the plain greedy ids g of every sequence: a one-token entry on an id nobody writes (fires at every step, t = 0
    included), (g0, g1) with a boost (fires at t = 1 and keeps g1 on top), (g0, g1, g2) at -inf (fires at t = 2 on the id greedy
    would write: the sequence must leave its greedy path there at the latest), and a five-token entry at -inf."""
    entries = {(7,): -2.5}
    for g in free:
        entries.setdefault(tuple(g[:2]), boost)
        entries.setdefault(tuple(g[:3]), NINF)
        entries.setdefault(tuple(g[:5]), NINF)
    return list(entries.items())


@pytest.mark.parametrize("precise,B", [(False, 1), (False, 2), (False, 5), (False, 32), (False, 40), (True, 5)])
def test_every_head_form_feeds_the_kernel(tiny_dir, precise, B):
    """B = 1 the fused-norm GEMV head (the pruned pair must not be taken), 2 the two-sequence GEMV, 5 / 32 the gemm16 form, 40 and the
    precise mode the stored-logits forms: 12 free-running steps under a list built from the plain greedy ids.  At every step
    reference(l' of the engine without the setting, the history) is the engine's logits_out bit for bit, the id is its argmax and the
    log-probability is log_softmax(l'')[id]; multi-token entries fired, and the ids are not the plain greedy ids."""
    steps = 12
    clips = _clips(B)
    a = HipEngine(tiny_dir, 0, precise=precise, max_new_tokens=16, token_logprobs=True)
    b = HipEngine(tiny_dir, 0, precise=precise, max_new_tokens=16, token_logprobs=True)
    try:
        free = a.transcribe_batch(clips, None, max_new=steps, fixed_new_tokens=steps)
        entries = _list_from(free)
        b.set_sequence_bias(entries)
        st = b.sequence_bias_stats()
        assert st == {"active": True, "entries": len(entries), "ids": sum(len(s) for s, _ in entries), "targets": len({s[-1] for s, _ in entries})}
        LA, LB, TB = _forced_pair(a, b, clips, steps)
        lps = b.fetch_logprobs()
        ids = b.fetch_ids(16)
    finally:
        a.close()
        b.close()
    assert not np.isnan(LA).any()
    worst_lp, fired_multi, banned = 0.0, 0, 0
    for q in range(B):
        col = [int(x) for x in TB[:, q]]
        for t in range(steps):
            want = R.apply(LA[t][q], col[:t], entries)
            assert np.array_equal(R.bits(want), R.bits(LB[t][q])), (precise, B, q, t, np.nonzero(R.bits(want) != R.bits(LB[t][q])))
            assert col[t] == R.argmax(want), (precise, B, q, t)
            assert not np.array_equal(R.bits(want), R.bits(LA[t][q]))    # the one-token entry fires at every step, the prefill's too
            fired_multi += sum(1 for s, _ in entries if len(s) > 1 and R.fires(s, col[:t]))
            banned += int((np.isneginf(want) & ~np.isneginf(LA[t][q])).any())
        stop = next((i for i, x in enumerate(col) if x in B_.EOS_IDS), steps)
        assert ids[q] == col[:stop] and len(lps[q]) == stop
        for t in range(stop):
            ref = float(R.log_softmax64(LB[t][q])[col[t]])
            worst_lp = max(worst_lp, abs(float(lps[q][t]) - ref))
            assert abs(float(lps[q][t]) - ref) <= LP_TOL, (q, t, float(lps[q][t]), ref)
        assert col != free[q]                                            # the feature did something: greedy's third id is banned
        assert all(tuple(col[i:i + 3]) != tuple(g[:3]) for g in free for i in range(steps - 2))   # no banned phrase was written
    assert fired_multi >= 2 * B and banned >= B
    print(f"[sequence bias] precise={precise} B={B}: {B * steps} rows bit-equal to the reference, {fired_multi} multi-token firings, "
          f"worst |lp - log_softmax64| {worst_lp:.2e}")


# ---- 3. graph and eager, another list on the same graph, and the way back ----------------------------------------------------
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


@pytest.mark.parametrize("B", [1, 5])
def test_graph_eager_other_list_and_back(tiny_dir, B):
    clips, kmax = _clips(B, 80, 1.5), 12
    fresh = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True)       # never has the setting
    plain = fresh.transcribe_batch(clips, None, max_new=kmax), fresh.fetch_logprobs(), _stats(fresh)
    fresh.close()
    assert all(len(x) >= 5 for x in plain[0])
    entries = _list_from(plain[0])
    eager = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True, use_graph=False)
    try:
        eager.set_sequence_bias(entries)
        T = _stage_ids(eager, clips, kmax)
        want, want_lp = eager.fetch_ids(kmax), eager.fetch_logprobs()
    finally:
        eager.close()
    for q in range(B):
        col = [int(x) for x in T[:, q]]
        assert want[q] == col[:next((i for i, x in enumerate(col) if x in B_.EOS_IDS), kmax)]
    eng = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True)
    try:
        eng.set_sequence_bias(entries)
        r1 = eng.transcribe_batch(clips, None, max_new=kmax), eng.fetch_logprobs()
        r2 = eng.transcribe_batch(clips, None, max_new=kmax), eng.fetch_logprobs()
        assert r1[0] == want and r1[0] != plain[0], (r1[0], want)                  # graph replay == the eager stage API
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(want_lp, r1[1]))
        assert r2[0] == r1[0] and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(r1[1], r2[1]))   # bit-identical twice
        g0 = _captures(eng)
        assert g0 >= 1
        other = [((7,), 1.5)] + [(tuple(x[:2]), NINF) for x in r1[0]] + [((9, 9, 9), 4.0)]   # another list, 4096 entries the next
        eng.set_sequence_bias(dict(other))
        r3 = eng.transcribe_batch(clips, None, max_new=kmax)
        big = [((i, 7), -0.5) for i in range(R.MAX_ENTRIES)]
        eng.set_sequence_bias(big)
        assert eng.sequence_bias_stats() == {"active": True, "entries": 4096, "ids": 8192, "targets": 1}
        r4 = eng.transcribe_batch(clips, None, max_new=kmax)
        assert _captures(eng) == g0 and r3 != r1[0] and len(r4) == B                # the same graph, other ids
        assert all(tuple(x[:2]) != tuple(y[:2]) for x, y in zip(r3, r1[0]))
        # back: the ids, log-probabilities and pruned-argmax passes of an engine that never had the setting
        eng.set_sequence_bias(None)
        with pytest.raises(Q3aError, match="nothing generated"):                   # the decode state is dropped
            eng.fetch_ids(kmax)
        assert eng.sequence_bias_stats() == {"active": False, "entries": 0, "ids": 0, "targets": 0}
        s0 = _stats(eng)
        back = eng.transcribe_batch(clips, None, max_new=kmax), eng.fetch_logprobs()
        s1 = _stats(eng)
    finally:
        eng.close()
    assert back[0] == plain[0] and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(back[1], plain[1]))
    assert (s0 == 0).all(), s0                                                     # no pruned pass ran while the setting was on ...
    assert (s1 - s0 == plain[2]).all(), (s0, s1, plain[2])                          # ... and afterwards as on the fresh engine


def test_pruned_argmax_returns_after_the_setting(tiny_dir):
    """One sequence without token log-probabilities: the greedy step is the pruned pair.  While a list is set it is not taken;
    after set_sequence_bias(None) the passes advance exactly as on a fresh engine and the ids are its ids."""
    clip, steps = synthetic.synthetic_clip(0, 9.3), 16
    never = HipEngine(tiny_dir, 0, max_new_tokens=steps)
    want = never.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)
    s_never = _stats(never)
    never.close()
    assert s_never[1] >= steps - 1
    eng = HipEngine(tiny_dir, 0, max_new_tokens=steps)
    try:
        eng.set_sequence_bias(_list_from(want))
        a = eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)
        assert a != want and len(a[0]) == steps and (_stats(eng) == 0).all()
        assert eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps) == a
        eng.set_sequence_bias([])
        assert eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps) == want
        assert (_stats(eng) == s_never).all(), (_stats(eng), s_never)
    finally:
        eng.close()


# ---- 4. composition ----------------------------------------------------------------------------------------------------------
def test_sampling_draws_from_the_rewritten_row(tiny_dir):
    """set_sampling(T = 1) over a list: at every step the engine's logits_out is the reference's l'' of the plain engine's l', and
    the drawn id is sampling_ref's draw from that l'' with the same (seed, s, t); a banned id is never drawn."""
    steps, B = 10, 3
    clips = _clips(B, 60, 1.25)
    a = HipEngine(tiny_dir, 0, max_new_tokens=16, token_logprobs=True)
    b = HipEngine(tiny_dir, 0, max_new_tokens=16, token_logprobs=True)
    try:
        free = a.transcribe_batch(clips, None, max_new=steps, fixed_new_tokens=steps)
        top = sorted({g[0] for g in free})
        entries = [((t,), NINF) for t in top] + [((7,), 1.0)] + _list_from(free)[1:]   # the greedy opening ids are banned outright
        b.set_sequence_bias(entries)
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
            want = R.apply(LA[t][q], col[:t], entries)
            assert np.array_equal(R.bits(want), R.bits(LB[t][q])), (q, t)
            d = S_.sample(want, 1.0, 0.0, SEED, q, t)
            if d.margin > SAMPLE_EPS:
                assert col[t] == d.id, (q, t, col[t], d.id, d.second, d.margin)
            else:
                assert col[t] in (d.id, d.second), (q, t)
                under += 1
            assert np.isfinite(want[col[t]]) and col[t] not in top       # a banned id is never drawn
            if t < stop:
                assert abs(float(lps[q][t]) - float(R.log_softmax64(want)[col[t]])) <= LP_TOL, (q, t)
    assert under <= 0.01 * steps * B + 1


def test_composition_with_the_logit_bias_and_repetition_control(tiny_dir):
    """The stated order, bit for bit against the reference chain: the logit bias inside the head (both engines carry it, so l' includes
    it), the sequence bias, then the repetition penalty and the n-gram ban on its result."""
    steps, B, p, n = 12, 3, 1.3, 2
    clips = _clips(B, 70, 1.5)
    a = HipEngine(tiny_dir, 0, max_new_tokens=16, token_logprobs=True)
    b = HipEngine(tiny_dir, 0, max_new_tokens=16, token_logprobs=True)
    try:
        free0 = a.transcribe_batch(clips, None, max_new=steps, fixed_new_tokens=steps)
        sup = {free0[1][0]: -0.5, 12: 0.75, 11: -np.inf, free0[0][1]: -np.inf}   # an id greedy wrote is suppressed, finite entries too
        for e in (a, b):
            e.set_logit_bias(sup)
        free = a.transcribe_batch(clips, None, max_new=steps, fixed_new_tokens=steps)   # greedy under the logit bias
        assert free != free0
        # finite boosts on ids the history holds: the penalty then divides the BOOSTED logit (the order is visible)
        entries = [((g[0],), 3.0) for g in {tuple(x[:1]): x for x in free}.values()] + _list_from(free)
        entries = list(dict(entries).items())
        b.set_sequence_bias(entries)
        b.set_repetition(p, n)
        LA, LB, TB = _forced_pair(a, b, clips, steps)
        lps = b.fetch_logprobs()
    finally:
        a.close()
        b.close()
    dense = B_.as_dense(V, sup)
    order_visible = 0
    for q in range(B):
        col = [int(x) for x in TB[:, q]]
        stop = next((i for i, x in enumerate(col) if x in B_.EOS_IDS), steps)
        for t in range(steps):
            assert np.isneginf(LA[t][q][np.isneginf(dense)]).all()         # l' carries the logit bias
            mid = R.apply(LA[t][q], col[:t], entries)
            want = Rep.apply(mid, col[:t], p, n)
            assert np.array_equal(R.bits(want), R.bits(LB[t][q])), (q, t, np.nonzero(R.bits(want) != R.bits(LB[t][q])))
            assert col[t] == R.argmax(want) and np.isfinite(dense[col[t]])
            other = R.apply(Rep.apply(LA[t][q], col[:t], p, n), col[:t], entries)   # the other order gives another row
            order_visible += int(not np.array_equal(R.bits(other), R.bits(want)))
            if t < stop:
                assert abs(float(lps[q][t]) - float(R.log_softmax64(want)[col[t]])) <= LP_TOL, (q, t)
        assert all(col[i:i + 2] != col[j:j + 2] for i in range(steps - 1) for j in range(i + 1, steps - 1))   # no 2-gram twice
    assert order_visible >= B


def test_score_never_sees_it(tiny_dir):
    clips, kmax = _clips(3, 70, 1.5), 8
    eng = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True)
    try:
        plain = eng.transcribe_batch(clips, None, max_new=kmax, fixed_new_tokens=kmax)
        targets = [x[:6] + [151645] for x in plain]
        off = eng.score_batch(clips, targets)
        eng.set_sequence_bias(_list_from(plain) + [((151645,), NINF)])
        assert eng.transcribe_batch(clips, None, max_new=kmax, fixed_new_tokens=kmax) != plain
        on = eng.score_batch(clips, targets)
        for x, y in zip(off, on):
            assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(x[1], y[1]) and np.array_equal(_bits(x[2]), _bits(y[2]))
    finally:
        eng.close()


# ---- 5. refusals and state ---------------------------------------------------------------------------------------------------
def test_refusals_and_state(tiny_dir):
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8)
    lib = eng._lib
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)

    def raw(ids, lens, bias):
        ids, lens, bias = np.asarray(ids, np.int32), np.asarray(lens, np.int32), np.asarray(bias, np.float32)
        eng._chk(lib.q3a_set_sequence_bias(eng._h, ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), bias.ctypes.data_as(f32p), len(lens)))

    try:
        keep = [((5, 6), 1.0), ((9,), NINF)]
        eng.set_sequence_bias(keep)
        on = {"active": True, "entries": 2, "ids": 3, "targets": 2}
        assert eng.sequence_bias_stats() == on
        for args, msg in [(([V], [1], [1.0]), "outside the vocabulary"), (([-1], [1], [1.0]), "outside the vocabulary"),
                          (([1], [0], [1.0]), "empty sequence"), (([1] * 33, [33], [1.0]), "more than 32"),
                          (([1, 2, 1, 2], [2, 2], [1.0, 2.0]), "repeats the sequence"), (([1], [1], [float("nan")]), "NaN or \\+inf"),
                          (([1], [1], [float("inf")]), "NaN or \\+inf"),
                          (([i % 3 for i in range(4097 * 2)], [2] * 4097, [1.0] * 4097), "4097 entries"),
                          (([(i >> (2 * k)) & 3 for i in range(2049) for k in range(32)], [32] * 2049, [1.0] * 2049), "65536 ids")]:
            with pytest.raises(Q3aError, match=msg):
                raw(*args)
            assert eng.sequence_bias_stats() == on                      # a refused call changes nothing
        # beam search and drafts while it is on, in both forms each; the engine stays usable
        clip = synthetic.synthetic_clip(3, 1.0)
        with pytest.raises(Q3aError, match="a sequence bias is on"):
            eng.beam_search_batch([clip], 2, max_new=4)
        with pytest.raises(Q3aError, match="a sequence bias is on"):
            eng.transcribe_draft_batch([clip], [[11, 12]], None, 6)
        eng.mel([clip, clip])
        eng.encode()
        eng.prefill(_prompts(eng))
        with pytest.raises(Q3aError, match="a sequence bias is on"):
            eng.beam_begin(2)
        with pytest.raises(Q3aError, match="a sequence bias is on"):
            eng.prefill_draft(_prompts(eng), [[11, 12], [13]])
        eng.mel([clip])
        eng.encode()
        eng.prefill(_prompts(eng))
        eng.decode_step()
        eng.set_sequence_bias(keep)                                      # a successful call drops the decode state
        with pytest.raises(Q3aError):
            eng.decode_step()
        with pytest.raises(Q3aError, match="no decode state"):
            eng.set_next_tokens([5])
        assert len(eng.transcribe_batch([clip], None, 6, fixed_new_tokens=6)[0]) == 6
        # a -inf entry over an allow-list that leaves no more tokens finite than the -inf targets (+ max_new_tokens = 8 under an
        # n-gram ban): refused by whichever setter comes second, and the refused call changes nothing
        allow2, allow3 = {100: 0.0, 101: 0.0}, {100: 0.0, 101: 0.0, 102: 0.0}
        two_inf = [((100,), NINF), ((5, 101), NINF), ((6, 101), NINF), ((7,), 1.0)]       # two distinct -inf targets
        eng.set_sequence_bias(two_inf)
        with pytest.raises(Q3aError, match="run out of finite logits"):
            eng.set_logit_bias(allow2, -np.inf)
        assert eng.logit_bias_stats() == {"active": False, "finite": V}
        eng.set_logit_bias(allow3, -np.inf)                              # three finite tokens: one more than the -inf targets
        with pytest.raises(Q3aError, match="run out of finite logits"):
            eng.set_repetition(1.0, 2)                                   # ... but not 2 + max_new_tokens
        assert eng.repetition_stats()["no_repeat_ngram_size"] == 0
        eng.set_repetition(1.3, 0)                                       # the penalty alone never empties a row
        with pytest.raises(Q3aError, match="run out of finite logits"):
            eng.set_sequence_bias(two_inf + [((102,), NINF)])
        assert eng.sequence_bias_stats()["entries"] == 4
        eng.set_sequence_bias([((7,), 1.0)])                             # no -inf entry: any allow-list goes
        eng.set_logit_bias(allow2, -np.inf)
        eng.set_logit_bias({t: 0.0 for t in range(100, 111)}, -np.inf)   # 11 finite tokens
        eng.set_repetition(1.0, 2)
        with pytest.raises(Q3aError, match="run out of finite logits"):
            eng.set_sequence_bias(two_inf + [((102,), NINF)])            # 3 + 8 >= 11
        eng.set_sequence_bias(two_inf)                                   # 2 + 8 < 11
        eng.set_logit_bias(None)
        eng.set_repetition(1.0, 0)
        eng.set_sequence_bias(None)
        assert eng.sequence_bias_stats()["active"] is False
    finally:
        eng.close()
    al = HipEngine(tiny_aligner_dir(), 0, max_new_tokens=1)
    try:
        with pytest.raises(Q3aError, match="forced aligner"):            # an aligner engine generates nothing
            al.set_sequence_bias([((5,), 1.0)])
        with pytest.raises(Q3aError, match="forced aligner"):
            al.sequence_bias_stats()
    finally:
        al.close()


# ---- 6. AsrInference and the CLI ---------------------------------------------------------------------------------------------
class _Tok:
    """id i <-> "t<i>"; a leading space makes the first id one larger (a second tokenisation of every phrase)."""
    def decode(self, ids, skip):
        return "language English<asr_text>" + " ".join(f"t{i}" for i in ids)

    def encode(self, text):
        ids = [int(w[1:]) for w in text.split()]
        if text.startswith(" "):
            ids[0] += 1
        return ids


def test_asr_inference_arguments(tiny_dir):
    clip = synthetic.synthetic_clip(12, 1.5)
    asr = AsrInference.load(tiny_dir, 0, token_logprobs=True, max_new_tokens=16)
    try:
        asr.tokenizer = tok = _Tok()
        eng = asr.engine
        plain = asr.transcribe(clip, max_new_tokens=8)
        g = plain.ids
        phrase = " ".join(f"t{i}" for i in g[:3])
        a = asr.transcribe(clip, max_new_tokens=8, banned_phrases=[phrase])
        assert a.ids != plain.ids and a.ids[:2] == g[:2] and a.ids[2] != g[2]
        assert eng.sequence_bias_stats()["active"] is False and eng.sequence_bias_state == []     # restored
        eng.set_sequence_bias(banned_sequences(tok, [phrase]))
        assert eng.transcribe_batch([clip], None, 8) == [a.ids]
        # hotwords (here pushed DOWN, so that the effect does not hang on this checkpoint's logit gaps: the greedy opening id
        # cannot be written) together with entries given as ids; the engine's own list is restored after the call
        own = [((7,), -1.0)]
        eng.set_sequence_bias(own)
        b = asr.transcribe(clip, max_new_tokens=8, hotwords=[phrase], hotword_boost=-1000.0, hotword_start_boost=-1000.0, sequence_bias={(9,): -0.25})
        assert b.ids[0] != g[0] and b.ids != a.ids
        assert eng.sequence_bias_state == own and eng.sequence_bias_stats() == {"active": True, "entries": 1, "ids": 1, "targets": 1}
        eng.set_sequence_bias(hotword_sequences(tok, [phrase], -1000.0, -1000.0) + [((9,), -0.25)])
        assert eng.transcribe_batch([clip], None, 8) == [b.ids]
        eng.set_sequence_bias(own)
        with pytest.raises(Exception):                                   # an exception inside the call: the list is restored too
            asr.transcribe("/nonexistent/clip.wav", banned_phrases=[phrase])
        assert eng.sequence_bias_state == own and eng.sequence_bias_stats()["entries"] == 1
        eng.set_sequence_bias(None)
        # composes with temperature, repetition control and the logit-bias arguments
        c = asr.transcribe(clip, max_new_tokens=8, banned_phrases=[phrase], temperature=1.0, seed=4, no_repeat_ngram_size=1, suppress_tokens=[a.ids[2]])
        eng.set_sequence_bias(banned_sequences(tok, [phrase]))
        eng.set_repetition(1.0, 1)
        eng.set_sampling(1.0, 0.0, 4)
        eng.set_logit_bias({a.ids[2]: -np.inf})
        want = eng.transcribe_batch([clip], None, 8)[0]
        eng.set_logit_bias(None)
        eng.set_sampling(0.0)
        eng.set_repetition(1.0, 0)
        eng.set_sequence_bias(None)
        assert c.ids == want and len(set(c.ids)) == len(c.ids) and a.ids[2] not in c.ids
        assert asr.transcribe(clip, max_new_tokens=8).ids == plain.ids
        for kw, msg in [(dict(hotwords=[phrase]), "hotword_boost"), (dict(hotword_boost=2.0), "without hotwords"),
                        (dict(banned_phrases=[phrase], beam_size=2), "beam"), (dict(banned_phrases=[phrase], draft=[5, 6]), "draft"),
                        (dict(sequence_bias=[((V,), 1.0)]), "outside the vocabulary"),
                        (dict(hotwords=[" ".join(["t5"] * 33)], hotword_boost=1.0), "33 ids")]:
            with pytest.raises(Q3aError, match=msg):
                asr.transcribe(clip, max_new_tokens=4, **kw)
        assert eng.sequence_bias_stats()["active"] is False
    finally:
        asr.engine.close()


def test_cli_environment_variables(tiny_dir, tmp_path):
    """Q3A_SEQUENCE_BIAS, Q3A_HOTWORDS (+ Q3A_HOTWORD_BOOST, Q3A_HOTWORD_START_BOOST) and Q3A_BANNED_PHRASES through the CLI give the text
    of the Python call.  The tokenizer names the plain run's first ids "a", "b", ... (byte-level BPE without merges), every other id
    "t<i>", so a phrase of those letters encodes to those ids."""
    from qwen3_asr_rs_amd.build import CLI_PATH
    wav = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_audio", "sample1.wav")
    eng = HipEngine(tiny_dir, 0, max_new_tokens=16)
    from qwen3_asr_rs_amd.audio import load_audio
    g = eng.transcribe_batch([load_audio(wav, 16000)], None, 8, fixed_new_tokens=8)[0]
    eng.close()
    letters = {}
    for t in g[:4]:
        letters.setdefault(t, "abcd"[len(letters)])
    space = next(i for i in range(300, 400) if i not in letters)
    mdir = tmp_path / "model"
    mdir.mkdir()
    for f in os.listdir(tiny_dir):
        if f.endswith((".json", ".safetensors")):
            os.symlink(os.path.join(tiny_dir, f), mdir / f)
    vocab = {f"t{i}": i for i in range(V) if i not in B_.EOS_IDS and i not in letters and i != space}
    vocab.update({ch: t for t, ch in letters.items()})
    vocab["Ġ"] = space
    tok = {"version": "1.0", "added_tokens": [{"id": 151643, "content": "<|endoftext|>", "special": True},
                                              {"id": 151645, "content": "<|im_end|>", "special": True}],
           "model": {"type": "BPE", "vocab": vocab, "merges": []}}
    (mdir / "tokenizer.json").write_text(json.dumps(tok))
    phrase = "".join(letters[t] for t in g[:3])
    asr = AsrInference.load(str(mdir), 0)
    assert asr.tokenizer.encode(phrase) == g[:3] and asr.tokenizer.encode(" " + phrase) == [space] + g[:3]
    plain = asr.transcribe(wav)
    ban = asr.transcribe(wav, banned_phrases=[phrase])
    assert ban.ids[:2] == g[:2] and ban.ids[2] != g[2]
    seq = [((g[0], g[1]), NINF), ((7,), -1.0)]
    hot = asr.transcribe(wav, hotwords=[phrase], hotword_boost=-30.0, hotword_start_boost=-40.0, banned_phrases=[phrase], sequence_bias=seq)
    asr.engine.close()
    assert all(x.ids != plain.ids for x in (ban, hot))
    (tmp_path / "ban.txt").write_text(f"# never write this\n{phrase}\n\n")
    (tmp_path / "hot.txt").write_text(f"{phrase}   # one phrase per line\n")
    (tmp_path / "seq.txt").write_text(f"-inf {g[0]} {g[1]}\n-1.0 7  # a one-token entry\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("Q3A_")}
    env.update(RUST_LOG="warn")

    def cli(**kw):
        return subprocess.run([CLI_PATH, str(mdir), wav], capture_output=True, text=True, timeout=300, env=dict(env, **kw))

    for want, kw in [(ban, dict(Q3A_BANNED_PHRASES=str(tmp_path / "ban.txt"))),
                     (hot, dict(Q3A_HOTWORDS=str(tmp_path / "hot.txt"), Q3A_HOTWORD_BOOST="-30", Q3A_HOTWORD_START_BOOST="-40",
                                Q3A_BANNED_PHRASES=str(tmp_path / "ban.txt"), Q3A_SEQUENCE_BIAS=str(tmp_path / "seq.txt")))]:
        out = cli(**kw)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.split("\n")
        assert lines[0] == f"Language: {want.language}" and lines[1] == f"Text: {want.text}" and want.text != plain.text, kw
    bad = cli(Q3A_HOTWORDS=str(tmp_path / "hot.txt"))
    assert bad.returncode == 1 and "Sequence bias failed" in bad.stderr and "Q3A_HOTWORD_BOOST" in bad.stderr
    (tmp_path / "bad.txt").write_text("2.5 oops\n")
    bad = cli(Q3A_SEQUENCE_BIAS=str(tmp_path / "bad.txt"))
    assert bad.returncode == 1 and "Sequence bias failed" in bad.stderr and "not an id" in bad.stderr


# ---- 7. no leak --------------------------------------------------------------------------------------------------------------
def test_device_memory_is_level_across_set_clear_cycles(tiny_dir):
    clip = synthetic.synthetic_clip(5, 1.0)
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8)

    def dev_bytes():
        return int(eng.debug_read_raw("device_bytes").view(np.uint64)[0])

    try:
        eng.transcribe_batch([clip], None, 4, fixed_new_tokens=4)
        base = dev_bytes()
        eng.set_sequence_bias(None)                                      # clearing an engine that never had a list allocates nothing
        assert dev_bytes() == base
        eng.set_sequence_bias([((5, 6), 1.0)])
        eng.transcribe_batch([clip], None, 4, fixed_new_tokens=4)
        eng.set_sequence_bias(None)
        eng.transcribe_batch([clip], None, 4, fixed_new_tokens=4)
        level = dev_bytes()
        assert level - base >= 81926 * 4                                # the tables: one buffer of fixed size (and whatever a storing head adds)
        for k in range(20):
            eng.set_sequence_bias([((i, 6), 1.0) for i in range(1 + 200 * k)])
            assert dev_bytes() == level
            if k % 5 == 0:
                eng.transcribe_batch([clip], None, 4, fixed_new_tokens=4)
            eng.set_sequence_bias(None)
            assert dev_bytes() == level
    finally:
        eng.close()
