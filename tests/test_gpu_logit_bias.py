"""Constrained decoding on the GPU: the per-token logit bias (q3a_set_logit_bias) inside every lm_head form.

Every head of the generation paths works on l' = l + b.  Checked here, per head form (the list of tests/test_gpu_logprobs.py): the
ids are the argmax of the engine's own l', the log-probabilities are the float64 log_softmax of l', l' is -inf exactly on suppressed
ids, l' against the unbiased l of the same history, the tie rule, the pruned one-sequence argmax under a bias (ids, that it runs, its
extended bound), the whole path and the engine's state across set / clear, beam search, the paths a bias must not touch, the fp32
oracle, the refusals and the CLI."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import logit_bias_ref as R
from align_ref import tiny_aligner_dir, word_ids
from eos_plan import peaked_checkpoint, plan_class_stops
from qwen3_asr_rs_amd import _lib, synthetic
from qwen3_asr_rs_amd.engine import AsrInference, HipEngine, Q3aError

pytestmark = pytest.mark.gpu

V = 151936
STEPS = 6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_audio")
_FORMS = [(False, 1, 1), (False, 1, 0), (False, 2, 1), (False, 5, 1), (False, 32, 1), (False, 40, 1), (True, 1, 1), (True, 5, 1)]
_FORM_PARAMS = [pytest.param(p, b, k, id=f"{p}-{b}" + ("" if k else "-prune0")) for p, b, k in _FORMS]
TOL = {True: 2e-4, False: 6e-2}  # the project's logit tolerance against the fp32 oracle (tests/test_gpu_parity.py TOL[..]["logit"])


def _set_prune(v: int):
    assert _lib.load().q3a_debug_set(b"lm_head_prune", v) == 0


@pytest.fixture(autouse=True)
def _restore_knob():
    yield
    _set_prune(1)


def _clips(n, seed0=40, base=1.0):
    return [synthetic.synthetic_clip(seed0 + i, base + 0.25 * (i % 4)) for i in range(n)]


def _stage_run(eng, clips, steps, forced=None):
    """Prefill + decode through the graph-replayed stage API: logits [steps][B][V], ids [steps][B], fetch_logprobs().
    forced: ids [steps][B] fed instead of the engine's own (teacher forcing on another run's history)."""
    eng.mel(clips)
    eng.encode()
    logits, nxt = eng.prefill([HipEngine.build_prompt(t) for t in eng._T])
    L, T = [logits.copy()], [nxt.copy()]
    for s in range(steps - 1):
        if forced is not None:
            eng.set_next_tokens(forced[s])
        lg, nx, _ = eng.decode_step()
        L.append(lg.copy())
        T.append(nx.copy())
    return np.stack(L), np.stack(T), (eng.fetch_logprobs() if eng.token_logprobs and forced is None else None)


def _kinds(emitted, top):
    c, c_default = R.kind_allow(V)
    return [("a", R.kind_suppress(V, emitted, top), 0.0), ("b", R.kind_small(V, emitted, top), 0.0), ("c", c, c_default)]


def _stats(eng) -> np.ndarray:
    return eng.debug_read_raw("lm_head_prune_stats").view(np.int32).copy()


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ---- 1. / 2. every head form, three bias kinds ---------------------------------------------------------------------------
@pytest.mark.parametrize("precise,B,prune", _FORM_PARAMS)
def test_bias_kinds_in_every_head_form(tiny_dir, precise, B, prune):
    """B = 1 the fused-norm GEMV head, 2 the two-sequence GEMV, 5 / 32 the gemm16 argmax epilogue, 40 and the precise mode
    argmax_partial_kernel.  Unbiased first; then suppress (a), suppress + small finite biases (b), an allow-list (c)."""
    _set_prune(prune)
    clips = _clips(B)
    plain = HipEngine(tiny_dir, 0, precise=precise, max_new_tokens=16, token_logprobs=True)
    eng = HipEngine(tiny_dir, 0, precise=precise, max_new_tokens=16, token_logprobs=True)
    try:
        _, T0, _ = _stage_run(plain, clips, STEPS)
        emitted, top = set(int(t) for t in T0.reshape(-1)), int(T0[0][0])
        worst_lp = worst_sum = 0.0
        for name, bias, default in _kinds(emitted, top):
            b = R.as_dense(V, bias, default)
            eng.set_logit_bias(bias, default)
            assert np.array_equal(_bits(eng.logit_bias_vector()), _bits(b))
            assert eng.logit_bias_stats() == {"active": True, "finite": int(np.isfinite(b).sum())}
            L, T, lp = _stage_run(eng, clips, STEPS)
            assert not np.isnan(L).any(), name
            assert np.array_equal(L == -np.inf, np.broadcast_to(b == -np.inf, L.shape)), name  # -inf exactly on suppressed ids
            for s in range(STEPS):
                ls = R.log_softmax64(L[s])
                for q in range(B):
                    t = int(T[s][q])
                    assert t == R.argmax(L[s][q]), (name, s, q)
                    assert np.isfinite(b[t]), (name, s, q, t)                              # every emitted id has a finite bias
                    if name != "c":
                        assert t not in emitted, (name, s, q, t)
                    err = abs(float(lp[q][s]) - float(ls[q][t]))
                    worst_lp = max(worst_lp, err)
                    assert err <= 1e-4, (name, s, q, float(lp[q][s]), float(ls[q][t]))
            assert all(len(x) == STEPS and np.all(x <= 0.0) for x in lp), name
            # l' against l: the unbiased engine teacher-forced on this run's ids sees the same history
            L0, _, _ = _stage_run(plain, clips, STEPS, forced=T)
            fin, zero = np.isfinite(b), b == 0.0
            b64 = b[fin].astype(np.float64)
            for s in range(STEPS):
                l0 = L0[s][:, fin].astype(np.float64)
                d = np.abs(L[s][:, fin].astype(np.float64) - (l0 + b64))
                tol = R.sum_tolerance(l0, b64)
                assert (d <= tol).all(), (name, s, float((d - tol).max()))
                worst_sum = max(worst_sum, float((d[tol > 0] / tol[tol > 0]).max()))   # (a zero row of the head: l = b = 0, d = 0)
                assert np.array_equal(_bits(L[s][:, zero]), _bits(L0[s][:, zero])), (name, s)        # exact for b = 0
        print(f"[logit_bias] precise={precise} B={B} prune={prune}: worst |lp - log_softmax64| {worst_lp:.2e}, "
              f"worst |l' - (l + b)| / tolerance {worst_sum:.3f}")
    finally:
        plain.close()
        eng.close()


# ---- 3. tie rule ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin_rows_dir(tiny_untied_dir):
    """lm_head rows V/2 .. V-1 replaced by rows 0 .. V/2-1 (as tests/test_gpu_logprobs.py): every logit has an exact twin in another
    block, wave, workgroup and partial."""
    d = "/tmp/q3a_ckpt_tiny_untied_twin_rows_logit_bias"
    if os.path.exists(d):
        shutil.rmtree(d)
    shutil.copytree(tiny_untied_dir, d)
    key = synthetic.output_embedding_key(d)
    head = synthetic.read_tensor(d, key).astype(np.float32)
    h = head.shape[0] // 2
    head[h:] = head[:h]
    synthetic.overwrite_tensor(d, key, head)
    return d


@pytest.mark.parametrize("precise,B,prune", _FORM_PARAMS)
def test_tie_rule_under_a_bias(twin_rows_dir, precise, B, prune):
    _set_prune(prune)
    clips, h = _clips(B), V // 2
    eng = HipEngine(twin_rows_dir, 0, precise=precise, max_new_tokens=16, token_logprobs=True)
    try:
        _, T0, _ = _stage_run(eng, clips, STEPS)
        assert (T0 < h).all()
        w = int(T0[0][0])
        eng.set_logit_bias({w: 0.5, w + h: 0.5})      # equal bias on a twin pair: the lower id wins
        L, T, _ = _stage_run(eng, clips, STEPS)
        assert int(T[0][0]) == w and (T < h).all()
        assert np.array_equal(_bits(L[:, :, :h]), _bits(L[:, :, h:]))
        eng.set_logit_bias({w + h: 2.0 ** -10})       # the upper twin of the unbiased winner a hair above it: it wins on that step
        L, T, _ = _stage_run(eng, clips, STEPS)
        assert int(T[0][0]) == w + h
        for s in range(STEPS):
            for q in range(B):
                assert int(T[s][q]) == R.argmax(L[s][q]), (s, q)
    finally:
        eng.close()


# ---- 4. the pruned one-sequence argmax -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_clip_plain(tiny_dir):
    """48 unbiased steps at one clip: the ids that define bias kinds (a) and (b) for the pruned-path tests."""
    clip = synthetic.synthetic_clip(0, 9.3)
    eng = HipEngine(tiny_dir, 0, max_new_tokens=56)
    ids = eng.transcribe_batch([clip], None, max_new=48, fixed_new_tokens=48)[0]
    eng.close()
    return clip, ids


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_pruned_argmax_under_a_bias(tiny_dir, one_clip_plain, kind):
    clip, ids0 = one_clip_plain
    name, bias, default = next(k for k in _kinds(set(ids0), ids0[0]) if k[0] == kind)
    b = R.as_dense(V, bias, default)
    steps = 48
    eng = HipEngine(tiny_dir, 0, max_new_tokens=steps + 8)
    try:
        eng.set_logit_bias(bias, default)
        _set_prune(0)
        off = eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)
        s0 = _stats(eng)
        _set_prune(1)
        on = eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)
        s1 = _stats(eng)
    finally:
        eng.close()
    assert (s0 == 0).all(), s0
    assert on == off and len(on[0]) == steps
    assert all(np.isfinite(b[t]) for t in on[0])
    blocks, passes = int(s1[0]), int(s1[1])
    assert steps - 1 <= passes <= steps + 1, s1          # the pruned passes ran: prefill + the decode steps
    per = blocks / passes
    print(f"[logit_bias] pruned, kind {kind}: {per:.2f} candidate blocks per pass")
    assert per >= 1.0
    if kind == "c":  # a block with every row suppressed is never rescored
        allowed_blocks = len({t // 16 for t in bias})
        assert per <= allowed_blocks, (per, allowed_blocks)


def test_pruned_tie_rule_under_a_bias(twin_rows_dir):
    """The tie rule through lm_head_approx_bias_kernel + the rescore pass.  The stage API of test_tie_rule_under_a_bias keeps the
    logits and so never takes the pruned pair; transcribe_batch at one clip does.  Twin rows sit in blocks V/32 apart, so both
    twins are candidates of one pass: equal bias -> the lower id, +2^-10 on the upper twin -> the upper id, as the full GEMV."""
    clip, h, steps = _clips(1)[0], V // 2, 12
    eng = HipEngine(twin_rows_dir, 0, max_new_tokens=steps + 8)
    try:
        plain = eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)[0]
        assert all(t < h for t in plain)
        w = plain[0]
        for bias, first in (({w: 0.5, w + h: 0.5}, w), ({w + h: 2.0 ** -10}, w + h)):
            eng.set_logit_bias(bias)
            _set_prune(0)
            s0 = _stats(eng)
            off = eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)[0]
            s1 = _stats(eng)
            _set_prune(1)
            on = eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)[0]
            s2 = _stats(eng)
            assert (s1 == s0).all(), (s0, s1)
            assert steps - 1 <= int(s2[1] - s1[1]) <= steps + 1, (s1, s2)   # the pruned passes ran
            assert on == off and len(on) == steps, (bias, on, off)
            assert on[0] == first, (bias, on[0])
            if first == w:
                assert all(t < h for t in on), on                           # every tie still goes to the lower twin
    finally:
        eng.close()


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_pruned_bound_under_a_bias(tiny_dir, one_clip_plain, kind):
    """|a' - l'| <= e' for every row of 9 decoder states (random histories); suppressed rows are (-inf, 0) next to l' = -inf."""
    clip, ids0 = one_clip_plain
    name, bias, default = next(k for k in _kinds(set(ids0), ids0[0]) if k[0] == kind)
    b = R.as_dense(V, bias, default)
    sup = b == -np.inf
    rng = np.random.default_rng(3)
    eng = HipEngine(tiny_dir, 0, debug_taps=True, max_new_tokens=24)
    worst = 0.0
    try:
        eng.set_logit_bias(bias, default)
        eng.mel([clip])
        eng.encode()
        logits, _ = eng.prefill([HipEngine.build_prompt(eng.num_audio_tokens(len(clip)))])
        for s in range(9):
            if s > 0:
                eng.set_next_tokens([int(rng.integers(V))])
                logits, _, _ = eng.decode_step(True)
            ab = eng.debug_read("lm_head_bound").reshape(V, 2).astype(np.float64)
            l = logits[0].astype(np.float64)   # l' as the head stored it (the "logits" tap is the prefill's copy of the same buffer)
            if s == 0:
                assert np.array_equal(_bits(eng.debug_read("logits").reshape(-1, V)[0]), _bits(logits[0]))
            assert (ab[sup, 0] == -np.inf).all() and (l[sup] == -np.inf).all() and (ab[sup, 1] == 0.0).all()
            assert np.isfinite(ab[~sup]).all() and np.isfinite(l[~sup]).all()
            err = np.abs(ab[~sup, 0] - l[~sup])
            bad = np.nonzero(err > ab[~sup, 1])[0]
            assert len(bad) == 0, (s, bad[:8], err[bad[:8]])
            worst = max(worst, float((err / ab[~sup, 1]).max()))
    finally:
        eng.close()
    print(f"[logit_bias] bound, kind {kind}: largest |a' - l'| / e' over 9 states {worst:.4f}")


# ---- 5. whole path and state ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged():
    """3 clips in 3 length classes on a peaked checkpoint with planted stops (as tests/test_gpu_eos.py): EOS at step 1, at step 3, never."""
    d = peaked_checkpoint("/tmp/q3a_ckpt_tinyu_logit_bias_eos", "tiny_untied", seed=5)
    kmax = 6
    clips = [synthetic.synthetic_clip(200 + i, 1.0 + 0.35 * i) for i in range(3)]
    plan_class_stops(d, clips, [0, 1, 2], [1, 3, None], kmax)
    return d, clips, kmax


@pytest.mark.parametrize("precise", [True, False])
def test_eos_forbidden_and_eos_favoured(ragged, precise):
    d, clips, kmax = ragged
    for sel in (clips, clips[:1]):
        eng = HipEngine(d, 0, precise=precise, max_new_tokens=kmax)
        try:
            want = eng.transcribe_batch(sel, None, max_new=kmax)
            if precise:
                assert len(want[0]) == 1, [len(x) for x in want]                   # the planted stop is there without a bias
            assert min(len(x) for x in want) < kmax
            eng.set_logit_bias({t: -np.inf for t in R.EOS_IDS})
            got = eng.transcribe_batch(sel, None, max_new=kmax)
            assert [len(x) for x in got] == [kmax] * len(sel)                      # exactly max_new ids for every utterance
            assert all(g[:len(w)] == w for g, w in zip(got, want))                 # same ids up to the stop that is now forbidden
            eng.set_logit_bias({151645: 1e4})
            assert eng.transcribe_batch(sel, None, max_new=kmax) == [[]] * len(sel)  # length 0 everywhere
        finally:
            eng.close()


def _whole(model_dir, clips, steps, bias, default, use_graph=True, fixed=True):
    eng = HipEngine(model_dir, 0, max_new_tokens=steps, use_graph=use_graph, token_logprobs=True)
    try:
        eng.set_logit_bias(bias, default)
        ids = eng.transcribe_batch(clips, None, max_new=steps, fixed_new_tokens=steps if fixed else 0)
        return ids, eng.fetch_logprobs()
    finally:
        eng.close()


def _same(x, y):
    return x[0] == y[0] and len(x[1]) == len(y[1]) and all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(x[1], y[1]))


@pytest.mark.parametrize("B", [1, 3])
def test_state_across_set_and_clear(tiny_dir, B):
    """ONE engine and batch shape: unbiased -> bias A -> bias B -> cleared.  The first and the fourth result are bit-identical, A and
    B each match a fresh engine given that bias (graph and eager): a stale graph or a stale vector shows here."""
    clips, steps = _clips(B, 80, 2.0), 12
    plain = _whole(tiny_dir, clips, steps, None, 0.0)
    emitted, top = set(t for x in plain[0] for t in x), plain[0][0][0]
    kinds = _kinds(emitted, top)
    (_, A, dA), (_, Bb, dB) = kinds[0], kinds[2]
    wantA, wantB = _whole(tiny_dir, clips, steps, A, dA), _whole(tiny_dir, clips, steps, Bb, dB)
    assert wantA[0] != plain[0] and wantB[0] != plain[0] and wantA[0] != wantB[0]
    assert _same(wantA, _whole(tiny_dir, clips, steps, A, dA, use_graph=False))          # graph replay equals eager
    assert _same(wantB, _whole(tiny_dir, clips, steps, Bb, dB, use_graph=False))
    assert _same(plain, _whole(tiny_dir, clips, steps, None, 0.0, use_graph=False))
    eng = HipEngine(tiny_dir, 0, max_new_tokens=steps, token_logprobs=True)
    try:
        def run():
            return eng.transcribe_batch(clips, None, max_new=steps, fixed_new_tokens=steps), eng.fetch_logprobs()
        r1 = run()
        eng.set_logit_bias(A, dA)
        with pytest.raises(Q3aError, match="nothing generated"):   # the decode state is dropped, as after q3a_score
            eng.fetch_ids(steps)
        r2 = run()
        eng.set_logit_bias(Bb, dB)
        r3 = run()
        eng.set_logit_bias(None)
        assert eng.logit_bias_stats() == {"active": False, "finite": V} and not eng.logit_bias_vector().any()
        r4 = run()
    finally:
        eng.close()
    assert _same(r1, plain) and _same(r4, r1) and _same(r2, wantA) and _same(r3, wantB)


def test_prune_stats_after_a_clear(tiny_dir):
    """After the clear the pruned passes advance as on an engine that never had a bias."""
    clip, steps = synthetic.synthetic_clip(0, 9.3), 16
    never = HipEngine(tiny_dir, 0, max_new_tokens=steps)
    want = never.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)
    s_never = _stats(never)
    never.close()
    eng = HipEngine(tiny_dir, 0, max_new_tokens=steps)
    try:
        eng.set_logit_bias({t: -np.inf for t in want[0]})
        assert eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps) != want
        s_a = _stats(eng)
        eng.set_logit_bias({})
        assert eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps) == want
        s_b = _stats(eng)
    finally:
        eng.close()
    assert s_a[1] == s_never[1] and (s_b - s_a == s_never).all(), (s_never, s_a, s_b)


def test_asr_inference_arguments_restore_the_previous_state(tiny_dir):
    clip = synthetic.synthetic_clip(12, 1.5)
    asr = AsrInference.load(tiny_dir, 0, token_logprobs=True)
    plain = asr.transcribe(clip, max_new_tokens=10)
    res = asr.transcribe(clip, max_new_tokens=10, suppress_tokens=plain.ids)
    assert len(res.ids) == 10 and not set(res.ids) & set(plain.ids) and len(res.token_logprobs) == 10
    assert asr.engine.logit_bias_stats()["active"] is False
    assert asr.transcribe(clip, max_new_tokens=10).ids == plain.ids
    allowed = sorted(set(res.ids[:3]) | {5, 6})
    only = asr.transcribe(clip, max_new_tokens=10, allowed_tokens=allowed)
    assert set(only.ids) <= set(allowed) | set(R.EOS_IDS)
    asr.engine.set_logit_bias({7: 1.0})                       # a bias of the caller's own survives a constrained call
    beam = asr.transcribe(clip, max_new_tokens=6, beam_size=3, suppress_tokens=plain.ids)
    assert not set(beam.ids) & set(plain.ids) and all(not set(a.ids) & set(plain.ids) for a in beam.alternatives)
    assert asr.engine.logit_bias_state == ({7: 1.0}, 0.0) and asr.engine.logit_bias_stats() == {"active": True, "finite": V}
    asr.engine.close()


# ---- 6. beam search ------------------------------------------------------------------------------------------------------
def test_beam_search_under_a_bias(tiny_dir):
    U, W, rounds = 2, 4, 6
    clips = [synthetic.synthetic_clip(300 + u, 1.0 + 0.25 * u) for u in range(U)]
    plain = HipEngine(tiny_dir, 0, max_new_tokens=8)
    ids0 = plain.transcribe_batch(clips, None, max_new=8, fixed_new_tokens=8)
    plain.close()
    bias = R.kind_suppress(V, set(t for x in ids0 for t in x), ids0[0][0])
    b = R.as_dense(V, bias)
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8)
    try:
        eng.set_logit_bias(bias)
        hyps = eng.beam_search_batch(clips, W, max_new=rounds)
        assert all(len(h) == W for h in hyps)
        for h in (x for hs in hyps for x in hs):
            assert np.isfinite(b[h.ids]).all() and np.isfinite(h.token_logprobs).all() and np.isfinite(h.score)
        # stage form: every candidate's lp is the float64 log_softmax of that round's l'
        rep = [c for c in clips for _ in range(W)]
        eng.mel(rep)
        eng.encode()
        logits, _ = eng.prefill([HipEngine.build_prompt(t) for t in eng._T])
        worst = 0.0
        for rnd in range(rounds):
            if rnd == 0:
                eng.beam_begin(W)
            else:
                _, logits = eng.beam_step(want_logits=True)
            assert np.array_equal(logits == -np.inf, np.broadcast_to(b == -np.inf, logits.shape)) and not np.isnan(logits).any()
            dbg = eng.beam_debug()
            ls = R.log_softmax64(logits)
            for s in range(U * W):
                order = np.lexsort((np.arange(V), -logits[s].astype(np.float64)))[:W]   # larger value, then smaller id
                assert dbg["topk_ids"][s].tolist() == order.tolist(), (rnd, s)
                assert np.isfinite(b[dbg["topk_ids"][s]]).all()
                err = np.abs(dbg["topk_lp"][s].astype(np.float64) - ls[s][dbg["topk_ids"][s]])
                worst = max(worst, float(err.max()))
                assert (err <= 1e-4).all(), (rnd, s, err)
        for h in (x for hs in eng.beam_fetch(rounds) for x in hs):
            assert np.isfinite(b[h.ids]).all() and np.isfinite(h.token_logprobs).all()
        print(f"[logit_bias] beam: worst |lp - log_softmax64(l')| {worst:.2e}")
    finally:
        eng.close()


def test_beam_width_one_is_the_biased_greedy_loop_and_width_check(ragged):
    d, clips, kmax = ragged
    eng = HipEngine(d, 0, max_new_tokens=kmax)
    try:
        plain = eng.transcribe_batch(clips, None, max_new=kmax)
        eng.set_logit_bias({plain[2][1]: -np.inf, plain[1][0]: -0.25})
        want = eng.transcribe_batch(clips, None, max_new=kmax)
        assert want != plain
        got = eng.beam_search_batch(clips, 1, max_new=kmax)
        assert [h[0].ids for h in got] == want
        assert [h[0].finished for h in got] == [len(w) < kmax for w in want]
        # a width larger than the number of finite entries is refused, in both forms
        eng.set_logit_bias({5: 0.0, 6: 0.5, 151645: 0.0}, -np.inf)
        with pytest.raises(Q3aError, match="exceeds the 3 tokens"):
            eng.beam_search_batch(clips[:1], 4, max_new=kmax)
        rep = [clips[0]] * 4
        eng.mel(rep)
        eng.encode()
        eng.prefill([HipEngine.build_prompt(t) for t in eng._T])
        with pytest.raises(Q3aError, match="exceeds the 3 tokens"):
            eng.beam_begin(4)
        hy = eng.beam_search_batch(clips[:1], 3, max_new=kmax)                # width == finite entries is served
        assert all(set(h.ids) <= {5, 6} for h in hy[0])
    finally:
        eng.close()


# ---- 7. paths a bias must not touch --------------------------------------------------------------------------------------
def test_score_and_align_ignore_the_bias(tiny_dir):
    clips = _clips(3, 70, 1.5)
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8)
    try:
        ids = eng.transcribe_batch(clips, None, max_new=6, fixed_new_tokens=6)
        targets = [x + [151645] for x in ids]
        before = eng.score_batch(clips, targets)
        eng.set_logit_bias(R.kind_small(V, set(t for x in ids for t in x), ids[0][0]))
        after = eng.score_batch(clips, targets)
        assert eng.transcribe_batch(clips, None, max_new=6, fixed_new_tokens=6) != ids   # the bias is live for generation
    finally:
        eng.close()
    for x, y in zip(before, after):
        assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(x[1], y[1]) and np.array_equal(_bits(x[2]), _bits(y[2]))
    al = HipEngine(tiny_aligner_dir(), 0, max_new_tokens=1)
    try:
        text = [word_ids(4 + i, 10 + i) for i in range(2)]
        a0 = al.align_batch(clips[:2], text)
        with pytest.raises(Q3aError, match="forced aligner"):                            # an aligner engine has no logit bias
            al.set_logit_bias({5: 1.0})
        with pytest.raises(Q3aError, match="forced aligner"):
            al.logit_bias_stats()
        assert al.align_batch(clips[:2], text) == a0
    finally:
        al.close()


# ---- 8. the fp32 oracle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precise", [True, False])
def test_biased_logits_against_the_oracle(tiny_dir, tiny_oracle, precise):
    """3 clips, 12 steps, bias (b): the oracle teacher-forced on the engine's ids; |l' - (l_oracle + b)| <= TOL + 2^-22 (|l| + |b|) on
    finite entries, -inf exactly where b is -inf; no step is exempt."""
    steps = 12
    clips = [synthetic.synthetic_clip(40 + i, 1.0 + 0.25 * i) for i in range(3)]
    plain = HipEngine(tiny_dir, 0, precise=precise, max_new_tokens=16)
    ids0 = plain.transcribe_batch(clips, None, max_new=steps, fixed_new_tokens=steps)
    plain.close()
    bias = R.kind_small(V, set(t for x in ids0 for t in x), ids0[0][0])
    b = R.as_dense(V, bias)
    fin = np.isfinite(b)
    b64 = np.where(fin, b, 0.0).astype(np.float64)
    eng = HipEngine(tiny_dir, 0, precise=precise, max_new_tokens=16)
    try:
        eng.set_logit_bias(bias)
        L, T, _ = _stage_run(eng, clips, steps)
    finally:
        eng.close()
    worst = 0.0
    for q, clip in enumerate(clips):
        ids = [int(t) for t in T[:, q]]
        ref = tiny_oracle.transcribe_ids(clip, forced_ids=ids[:steps - 1], last_only=True)
        for s in range(steps):
            lo = ref.step_logits[s].numpy().astype(np.float64)
            assert (L[s][q][~fin] == -np.inf).all() and np.isfinite(L[s][q][fin]).all()
            d = np.abs(L[s][q][fin].astype(np.float64) - (lo[fin] + b64[fin]))
            tol = TOL[precise] + R.sum_tolerance(lo[fin], b64[fin])
            worst = max(worst, float(d.max()))
            assert (d <= tol).all(), (precise, q, s, float(d.max()))
    print(f"[logit_bias] oracle precise={precise}: worst |l' - (l_oracle + b)| {worst:.2e} (TOL {TOL[precise]})")


# ---- 9. refusals and the CLI ---------------------------------------------------------------------------------------------
def test_refusals(tiny_dir):
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8)
    lib, i32p, f32p = eng._lib, _lib.C.POINTER(_lib.C.c_int32), _lib.C.POINTER(_lib.C.c_float)

    def raw(ids, bias, default=0.0):
        a, v = np.asarray(ids, np.int32), np.asarray(bias, np.float32)
        eng._chk(lib.q3a_set_logit_bias(eng._h, a.ctypes.data_as(i32p), v.ctypes.data_as(f32p), len(a), _lib.C.c_float(default)))
    try:
        eng.set_logit_bias({3: 1.0})
        for args, msg in [(([-1], [1.0]), "id -1 is outside the vocabulary"), (([V], [1.0]), f"id {V} is outside the vocabulary"),
                          (([4, 9, 4], [1.0, 2.0, 3.0]), "duplicate id 4"), (([4], [np.nan]), "NaN or \\+inf"), (([4], [np.inf]), "NaN or \\+inf"),
                          (([4], [1.0], 1.0), "default_bias must be 0 or -inf"), (([4], [1.0], np.inf), "default_bias must be 0 or -inf"),
                          (([4], [1.0], np.nan), "default_bias must be 0 or -inf"),
                          (([], [], -np.inf), "no finite entry"), (([4], [-np.inf], -np.inf), "no finite entry")]:
            with pytest.raises(Q3aError, match=msg):
                raw(*args)
            assert eng.logit_bias_state == ({3: 1.0}, 0.0) and eng.logit_bias_stats() == {"active": True, "finite": V}  # a refused call changes nothing
        assert float(eng.logit_bias_vector()[3]) == 1.0
        # the decode state is dropped by a successful call
        clip = synthetic.synthetic_clip(3, 1.0)
        eng.mel([clip])
        eng.encode()
        eng.prefill([HipEngine.build_prompt(eng._T[0])])
        eng.decode_step()
        eng.set_logit_bias({3: 2.0})
        with pytest.raises(Q3aError):
            eng.decode_step()
        with pytest.raises(Q3aError, match="no decode state"):
            eng.set_next_tokens([5])
        with pytest.raises(Q3aError, match="nothing generated"):
            eng.fetch_ids(4)
    finally:
        eng.close()


def test_cli_environment_variables(tiny_dir, tmp_path):
    """Q3A_SUPPRESS_TOKENS / Q3A_LOGIT_BIAS through the CLI give the ids of the Python call (token t<i> decodes to "t<i>")."""
    from qwen3_asr_rs_amd.build import CLI_PATH
    mdir = tmp_path / "model"
    mdir.mkdir()
    for f in os.listdir(tiny_dir):
        if f.endswith((".json", ".safetensors")):
            os.symlink(os.path.join(tiny_dir, f), mdir / f)
    vocab = {f"t{i}": i for i in range(V) if i not in R.EOS_IDS}
    tok = {"version": "1.0", "added_tokens": [{"id": 151643, "content": "<|endoftext|>", "special": True},
                                              {"id": 151645, "content": "<|im_end|>", "special": True}],
           "model": {"type": "BPE", "vocab": vocab, "merges": []}}
    (mdir / "tokenizer.json").write_text(json.dumps(tok))
    wav = os.path.join(GOLDEN, "sample1.wav")
    asr = AsrInference.load(str(mdir), 0)
    plain = asr.transcribe(wav)
    sup = sorted(set(plain.ids))[:8]
    lo = (plain.ids[0] // 2048) * 2048
    nudges = {1234: 1.5, 77: -0.5}
    want = asr.transcribe(wav, suppress_tokens=sup + list(range(lo, lo + 2048)), logit_bias=nudges)
    asr.engine.close()
    assert want.ids != plain.ids and not set(want.ids) & set(sup)
    (tmp_path / "bias.txt").write_text(f"# nudges\n1234 1.5\n77 -0.5\n{lo}-{lo + 2047} -inf\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("Q3A_")}
    env.update(RUST_LOG="warn", Q3A_SUPPRESS_TOKENS=",".join(str(t) for t in sup if not lo <= t < lo + 2048),
               Q3A_LOGIT_BIAS=str(tmp_path / "bias.txt"))
    out = subprocess.run([CLI_PATH, str(mdir), wav], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    assert lines[0] == f"Language: {want.language}" and lines[1] == f"Text: {want.text}" and want.text != plain.text
    bad = subprocess.run([CLI_PATH, str(mdir), wav], capture_output=True, text=True, timeout=300, env=dict(env, Q3A_SUPPRESS_TOKENS="1,1"))
    assert bad.returncode == 1 and "Logit bias failed" in bad.stderr and "duplicate id 1" in bad.stderr
