"""Top-k / top-p on the GPU (q3a_set_sampling_filter; k_sample.hip): the threshold stage against the float64 reference through
q3a_selftest_sample_filter, every lm_head form feeding it, graph replay against the eager stage API, another setting on the same
graph, the way back to the unfiltered sampler and to the greedy engine, the composition with the logit bias, repetition control and
scoring, the refusals and the device memory across cycles.

The rules (include/q3asr.h "sampling filter").  With top_p = 1 the threshold and the kept count are the reference's, bit for bit.
With top_p < 1 the threshold lies between the reference's at top_p + DELTA and at top_p - DELTA and the count between theirs; DELTA
(1e-5) is derived in the header from the arithmetic, and the largest deviation the thresholds imply is printed.  The id is the
reference's draw over { l >= max(threshold the device reported, the min-p threshold) } under the sampler's own rule: beyond a margin
of EPS the reference's id, within it one of its best two, and at most 1 % of a test's draws that close."""
import numpy as np
import pytest

import logit_bias_ref as B_
import sampling_filter_ref as F
import sampling_ref as R
from align_ref import tiny_aligner_dir
from qwen3_asr_rs_amd import _lib, synthetic
from qwen3_asr_rs_amd.engine import AsrInference, HipEngine, Q3aError

pytestmark = pytest.mark.gpu

V = 151936
EPS = 7.1e-6
SEED = (9 << 32) + 4242
C = _lib.C


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _selftest(rows, T, min_p, top_k, top_p, seed, step):
    lib = _lib.load()
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    S, Vr = rows.shape
    ids, lp, z = np.full(S, -7, np.int32), np.zeros(S, np.float32), np.zeros(S, np.float32)
    thr, kept = np.zeros(S, np.float32), np.full(S, -7, np.int32)
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    rc = lib.q3a_selftest_sample_filter(0, rows.ctypes.data_as(f32p), S, Vr, C.c_float(T), C.c_float(min_p), top_k, C.c_float(top_p),
                                        C.c_uint64(seed), step, ids.ctypes.data_as(i32p), lp.ctypes.data_as(f32p), z.ctypes.data_as(f32p),
                                        thr.ctypes.data_as(f32p), kept.ctypes.data_as(i32p))
    assert rc == 0, lib.q3a_last_error(None)
    return ids, lp, z, thr, kept


def _selftest_plain(rows, T, min_p, seed, step):
    lib = _lib.load()
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    S, Vr = rows.shape
    ids, z = np.full(S, -7, np.int32), np.zeros(S, np.float32)
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    rc = lib.q3a_selftest_sample(0, rows.ctypes.data_as(f32p), S, Vr, C.c_float(T), C.c_float(min_p), C.c_uint64(seed), step,
                                 ids.ctypes.data_as(i32p), None, z.ctypes.data_as(f32p))
    assert rc == 0, lib.q3a_last_error(None)
    return ids, z


def _judge(got_id: int, d, where):
    """The sampler's id rule; returns 1 when the draw was under EPS (counted against the 1 % cap)."""
    if d.margin > EPS:
        assert got_id == d.id, (where, got_id, d.id, d.second, d.margin)
        return 0
    assert got_id in (d.id, d.second), (where, got_id, d.id, d.second, d.margin)
    return 1


def _check_threshold(row, T, k, p, thr, kept, where):
    """The sandwich; returns the deviation |G_device - G_ref| the threshold implies (0 where the reference's own threshold came out)."""
    lo, hi = F.sandwich(row, T, k, p)
    if float(np.float32(p)) >= 1.0:
        assert _bits(thr) == _bits(lo[0]) and int(kept) == lo[1], (where, thr, kept, lo)
        return 0.0
    assert lo[0] <= thr <= hi[0] and hi[1] <= int(kept) <= lo[1], (where, thr, kept, lo, hi)
    vals, G = F.mass_above(row, T, k)
    at = np.nonzero(vals == np.float64(thr))[0]
    assert len(at) == 1, (where, thr)                                                  # a row value
    i, pf = int(at[0]), float(np.float32(p))
    dev = max(0.0, G[i] - pf)                                                          # it kept a value whose exact G is not under top_p
    if i + 1 < len(vals):
        dev = max(dev, pf - G[i + 1])                                                  # it dropped a value whose exact G is under top_p
    return max(dev, 0.0)


# ---- 1. the kernels against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("Vk", list(F.KERNEL_V) + [F.BIG_V])
def test_kernels_against_the_reference(Vk):
    """V = 1, 63, 2048, 2049, 4100 (scalar loads), 6150, 151936 once; S = 1 and 3; the settings of sampling_filter_ref.kernel_combos;
    the six rows of the sampler's test and six more: all equal, zeros of both signs at the k-th place, one dominant logit, the k-th
    value tied across chunks, fewer finite entries than top_k, a steep row.  Every call runs the stage twice on one table."""
    rows, calls, cases = F.kernel_rows(Vk), F.kernel_calls(Vk), F.kernel_draws(Vk)
    by_call = {}
    for c in cases:
        by_call.setdefault(c.call, []).append(c)
    under = n = 0
    worst_dev = worst_lp = worst_z = 0.0
    for ci, (g, T, mp, k, p, st) in enumerate(calls):
        ids, lp, z, thr, kept = _selftest(rows[g], T, mp, k, p, F.SAMPLE_SEED[Vk], st)
        if (k, p) == (0, 1.0):                                                         # off: the sampler without the stage, bit for bit
            ids0, z0 = _selftest_plain(rows[g], T, mp, F.SAMPLE_SEED[Vk], st)
            assert np.array_equal(ids, ids0) and np.array_equal(_bits(z), _bits(z0)), (Vk, g)
        if (k, p) == (50, 0.9):                                                        # two runs are bit-identical
            again = _selftest(rows[g], T, mp, k, p, F.SAMPLE_SEED[Vk], st)
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip((ids, lp, z, thr, kept), again)), (Vk, g)
        for s, c in enumerate(by_call[ci]):
            where = (Vk, g, T, mp, k, p, st, s)
            row = rows[g[s]]
            assert F.draw_is_safe(c, T), where                                         # (held on the CPU by tests/test_sampling_filter_host.py)
            worst_dev = max(worst_dev, _check_threshold(row, T, k, p, thr[s], kept[s], where))
            d = F.sample_over(row, T, max(float(thr[s]), F.minp_threshold(row, T, mp)), F.SAMPLE_SEED[Vk], s, st)
            under += _judge(int(ids[s]), d, where)
            n += 1
            if int(ids[s]) == d.id:
                worst_z = max(worst_z, abs(float(z[s]) - d.z))
            ref_lp = float(R.log_softmax64(row)[int(ids[s])])
            worst_lp = max(worst_lp, abs(float(lp[s]) - ref_lp))
            assert abs(float(lp[s]) - ref_lp) <= 1e-4, (where, float(lp[s]), ref_lp)
            if k == 1 and (row == row.max()).sum() == 1:                               # top_k = 1 without ties: the argmax, whatever the seed
                assert int(ids[s]) == int(np.argmax(row)) and int(kept[s]) == 1, where
    print(f"[sampling filter] V={Vk}: {n} draws, largest |G_device - G_ref| implied by a threshold {worst_dev:.3e} (DELTA {F.DELTA:.0e}), "
          f"largest |z - z_ref| {worst_z:.3e}, largest |lp - log_softmax64| {worst_lp:.2e}, {under} under EPS")
    assert worst_dev <= F.DELTA
    assert under <= 0.01 * n


# ---- 2. every head form stores what the stage reads ------------------------------------------------------------------------
def _clips(n, seed0=40, base=1.0):
    return [synthetic.synthetic_clip(seed0 + i, base + 0.25 * (i % 4)) for i in range(n)]


def _sel(eng):
    return eng.debug_read_raw("sample_threshold").view(np.float32).copy(), eng.debug_read_raw("sample_kept").view(np.int32).copy()


def _stage_run(eng, clips, steps, read_sel=True):
    """Prefill + decode through the stage API: logits [steps][B][V], ids [steps][B], and per step the stage's (threshold, kept)."""
    eng.mel(clips)
    eng.encode()
    logits, nxt = eng.prefill([HipEngine.build_prompt(t) for t in eng._T])
    L, T, S = [logits.copy()], [nxt.copy()], [_sel(eng) if read_sel else None]
    for _ in range(steps - 1):
        lg, nx, _ = eng.decode_step()
        L.append(lg.copy())
        T.append(nx.copy())
        S.append(_sel(eng) if read_sel else None)
    return np.stack(L), np.stack(T), S


@pytest.mark.parametrize("precise,B,k,p", [(False, 1, 50, 0.9), (False, 2, 0, 0.9), (False, 5, 50, 0.5), (True, 5, 7, 1.0)])
def test_every_head_form_feeds_the_stage(tiny_dir, precise, B, k, p):
    """B = 1 and 2 the GEMV heads, 5 the gemm16 argmax epilogue, and the precise mode: 8 steps at T = 1, at every step the threshold
    and the kept count against that step's own logits, and the id against the reference draw with (s, t)."""
    steps = 8
    eng = HipEngine(tiny_dir, 0, precise=precise, max_new_tokens=16, token_logprobs=True)
    try:
        eng.set_sampling(1.0, 0.0, SEED)
        eng.set_sampling_filter(k, p)
        assert eng.sampling_filter_stats() == {"active": True, "top_k": k, "top_p": float(np.float32(p))}
        assert eng.sampling_stats() == {"active": True, "temperature": 1.0, "min_p": 0.0, "seed": SEED}
        L, T, S = _stage_run(eng, _clips(B), steps)
    finally:
        eng.close()
    assert not np.isnan(L).any()
    under = 0
    worst = 0.0
    for t in range(steps):
        thr, kept = S[t]
        assert thr.shape == kept.shape == (B,)
        for q in range(B):
            worst = max(worst, _check_threshold(L[t][q], 1.0, k, p, thr[q], kept[q], (precise, B, t, q)))
            under += _judge(int(T[t][q]), F.sample_over(L[t][q], 1.0, float(thr[q]), SEED, q, t), (precise, B, t, q))
            assert L[t][q][int(T[t][q])] >= thr[q]
    assert worst <= F.DELTA and under <= 0.01 * steps * B
    print(f"[sampling filter] precise={precise} B={B} ({k}, {p}): kept {S[0][1].tolist()} at the prefill, implied deviation {worst:.2e}")


def test_batch_grows_and_shrinks_on_one_engine(tiny_dir):
    """One engine with the filter on at 1, then 5, then 1 sequences (the stage's table grows with the batch and must be zero for every
    row whatever ran before): 4 steps each, threshold, kept count and id against each step's own logits."""
    eng = HipEngine(tiny_dir, 0, max_new_tokens=16)
    k, p, steps = 50, 0.9, 4
    try:
        eng.set_sampling(1.0, 0.0, SEED)
        eng.set_sampling_filter(k, p)
        runs = [(B, _stage_run(eng, _clips(B, 50 + B), steps)) for B in (1, 5, 1)]
    finally:
        eng.close()
    for n, (B, (L, T, S)) in enumerate(runs):
        for t in range(steps):
            thr, kept = S[t]
            assert thr.shape == (B,)
            for q in range(B):
                assert _check_threshold(L[t][q], 1.0, k, p, thr[q], kept[q], (n, B, t, q)) <= F.DELTA
                _judge(int(T[t][q]), F.sample_over(L[t][q], 1.0, float(thr[q]), SEED, q, t), (n, B, t, q))
    assert np.array_equal(runs[0][1][1], runs[2][1][1])                               # the same clip, the same seed: the same ids again


# ---- 3. graph, eager, another setting on the same graph, and the ways back ---------------------------------------------------
def _stats(eng):
    return eng.debug_read_raw("lm_head_prune_stats").view(np.int32).copy()


def _captures(eng):
    return int(eng.debug_read_raw("graph_captures").view(np.int32)[0])


@pytest.mark.parametrize("B", [1, 5])
def test_graph_eager_settings_and_the_ways_back(tiny_dir, B):
    clips, kmax = _clips(B, 80, 1.5), 10
    fix = dict(max_new=kmax, fixed_new_tokens=kmax)
    fresh = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True)           # never samples, never filters
    greedy = fresh.transcribe_batch(clips, None, **fix), fresh.fetch_logprobs(), _stats(fresh)
    fresh.set_sampling(1.0, 0.0, SEED)
    unfiltered = fresh.transcribe_batch(clips, None, **fix), fresh.fetch_logprobs()
    fresh.close()
    eager = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True, use_graph=False)
    try:
        eager.set_sampling(1.0, 0.0, SEED)
        eager.set_sampling_filter(20, 0.8)
        _, T, _ = _stage_run(eager, clips, kmax, read_sel=False)
        want, want_lp = [[int(x) for x in T[:, q]] for q in range(B)], eager.fetch_logprobs()
    finally:
        eager.close()
    eng = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True)
    try:
        eng.set_sampling(1.0, 0.0, SEED)
        eng.set_sampling_filter(20, 0.8)
        r1 = eng.transcribe_batch(clips, None, **fix), eng.fetch_logprobs()
        n_graphs = _captures(eng)
        r2 = eng.transcribe_batch(clips, None, **fix), eng.fetch_logprobs()
        assert r1[0] == want and r1[0] != unfiltered[0]                                # graph replay == the eager stage API
        assert all(np.array_equal(_bits(a)[:kmax], _bits(b)[:kmax]) for a, b in zip(r1[1], want_lp))
        assert r2[0] == r1[0] and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(r1[1], r2[1]))   # bit-identical twice
        thr, kept = _sel(eng)
        assert (kept >= 1).all() and (kept <= 20).all() and np.isfinite(thr).all()
        # another setting replays the same graph; top_k = 1 is the argmax, so the ids are the greedy engine's
        eng.set_sampling_filter(1, 1.0)
        r3 = eng.transcribe_batch(clips, None, **fix)
        assert r3 == greedy[0] and _captures(eng) == n_graphs
        assert (_sel(eng)[1] == 1).all()
        # filter off: the sampler of an engine that never had one
        eng.set_sampling_filter(0, 1.0)
        assert eng.sampling_filter_stats() == {"active": False, "top_k": 0, "top_p": 1.0}
        with pytest.raises(Q3aError, match="nothing generated"):                       # the decode state is dropped
            eng.fetch_ids(kmax)
        r4 = eng.transcribe_batch(clips, None, **fix), eng.fetch_logprobs()
        assert r4[0] == unfiltered[0] and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(r4[1], unfiltered[1]))
        with pytest.raises(Q3aError, match="sample_threshold"):
            _sel(eng)
        # sampling off with a filter still set: the greedy launches, ids, log-probabilities and pruned passes of a fresh engine
        eng.set_sampling_filter(20, 0.8)
        eng.set_sampling(0.0)
        s0 = _stats(eng)
        back = eng.transcribe_batch(clips, None, **fix), eng.fetch_logprobs()
        s1 = _stats(eng)
    finally:
        eng.close()
    assert back[0] == greedy[0] and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(back[1], greedy[1]))
    assert (s0 == 0).all(), s0
    assert (s1 - s0 == greedy[2]).all(), (s0, s1, greedy[2])


# ---- 4. composition ----------------------------------------------------------------------------------------------------------
def test_composition_with_the_logit_bias_repetition_and_score(tiny_dir):
    clips, kmax = _clips(3, 70, 1.5), 12
    fix = dict(max_new=kmax, fixed_new_tokens=kmax)
    eng = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True)
    try:
        plain = eng.transcribe_batch(clips, None, **fix)
        targets = [x[:6] + [151645] for x in plain]
        score_off = eng.score_batch(clips, targets)
        eng.set_repetition(1.3, 2)
        rep_greedy = eng.transcribe_batch(clips, None, **fix)
        assert rep_greedy != plain
        # repetition control under top_k = 1 is the greedy run under the same repetition setting
        eng.set_sampling(1.0, 0.0, SEED)
        eng.set_sampling_filter(1, 1.0)
        assert eng.transcribe_batch(clips, None, **fix) == rep_greedy
        eng.set_repetition(1.0, 0)
        # under a suppress bias no suppressed id is drawn
        sup = B_.kind_suppress(V, set(t for x in plain for t in x), plain[0][0])
        dense = B_.as_dense(V, sup)
        eng.set_logit_bias(sup)
        eng.set_sampling(2.0, 0.0, SEED)
        eng.set_sampling_filter(50, 0.95)
        got = eng.transcribe_batch(clips, None, **fix)
        assert all(len(x) == kmax for x in got) and all(np.isfinite(dense[t]) for x in got for t in x) and got != plain
        score_on = eng.score_batch(clips, targets)                                     # q3a_score* never sees the filter
        for x, y in zip(score_off, score_on):
            assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(x[1], y[1]) and np.array_equal(_bits(x[2]), _bits(y[2]))
        with pytest.raises(Q3aError, match="sampling is on"):                          # beam search keeps its refusal of sampling
            eng.beam_search_batch(clips[:1], 2, max_new=4)
    finally:
        eng.close()


# ---- 5. refusals, state, memory ------------------------------------------------------------------------------------------------
def test_refusals_and_state(tiny_dir):
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8)
    lib = eng._lib
    try:
        eng.set_sampling(0.7, 0.05, 11)
        eng.set_sampling_filter(40, 0.9)
        want = {"active": True, "top_k": 40, "top_p": float(np.float32(0.9))}
        for k, p, msg in [(-1, 1.0, "top_k"), (0, 0.0, "top_p"), (0, -0.5, "top_p"), (0, 1.5, "top_p"), (0, float("nan"), "top_p")]:
            with pytest.raises(Q3aError, match=msg):
                eng._chk(lib.q3a_set_sampling_filter(eng._h, k, C.c_float(p)))
            assert eng.sampling_filter_stats() == want                                 # a refused call changes nothing
        clip = synthetic.synthetic_clip(3, 1.0)
        assert len(eng.transcribe_batch([clip], None, max_new=6, fixed_new_tokens=6)[0]) == 6   # the engine is usable afterwards
        eng.mel([clip])
        eng.encode()
        eng.prefill([HipEngine.build_prompt(eng._T[0])])
        eng.decode_step()
        eng.set_sampling_filter(V + 7, 0.9)                                            # a successful call drops the decode state
        with pytest.raises(Q3aError):
            eng.decode_step()
        assert eng.sampling_stats()["seed"] == 11                                      # "sampling" reads as before
        with pytest.raises(Q3aError, match="sample_kept"):                             # ... and the last run's values with it
            eng.debug_read_raw("sample_kept")
    finally:
        eng.close()
    al = HipEngine(tiny_aligner_dir(), 0, max_new_tokens=1)
    try:
        with pytest.raises(Q3aError, match="forced aligner"):                          # an aligner engine generates nothing
            al.set_sampling_filter(40, 0.9)
        with pytest.raises(Q3aError, match="forced aligner"):
            al.sampling_filter_stats()
    finally:
        al.close()


def test_device_memory_is_level_across_cycles(tiny_dir):
    clips = _clips(2, 90, 1.0)
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8, token_logprobs=True)
    try:
        def cycle():
            eng.set_sampling(1.0, 0.05, 3)
            eng.set_sampling_filter(50, 0.9)
            eng.transcribe_batch(clips, None, max_new=6, fixed_new_tokens=6)
            inside = int(eng.debug_read_raw("device_bytes").view(np.uint64)[0])
            eng.set_sampling_filter(0, 1.0)
            eng.transcribe_batch(clips, None, max_new=6, fixed_new_tokens=6)
            eng.set_sampling(0.0)
            eng.transcribe_batch(clips, None, max_new=6, fixed_new_tokens=6)
            return inside, int(eng.debug_read_raw("device_bytes").view(np.uint64)[0])
        first = cycle()
        assert first[0] == first[1]                                                    # clearing frees nothing: freed with the engine
        for _ in range(3):
            assert cycle() == first
    finally:
        eng.close()


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
        sampled = asr.transcribe(clip, max_new_tokens=8, temperature=1.0, seed=4)
        a = asr.transcribe(clip, max_new_tokens=8, temperature=1.0, seed=4, top_k=30, top_p=0.9)
        b = asr.transcribe(clip, max_new_tokens=8, temperature=1.0, seed=4, top_p=0.9, top_k=30)
        assert a.ids == b.ids and a.ids != sampled.ids and a.token_logprobs == b.token_logprobs
        assert eng.sampling_filter_stats()["active"] is False and eng.sampling_filter_state == (0, 1.0)     # restored
        assert asr.transcribe(clip, max_new_tokens=8, temperature=1.0, seed=4, top_k=1).ids == plain.ids
        eng.set_sampling_filter(7, 0.5)                                                # the engine's own setting comes back
        asr.transcribe(clip, max_new_tokens=8, temperature=1.0, seed=4, top_p=0.9)
        assert eng.sampling_filter_state == (7, 0.5) and eng.sampling_filter_stats() == {"active": True, "top_k": 7, "top_p": 0.5}
        eng.set_sampling_filter(0, 1.0)
        # with the fallback tuple: every attempt fails on a random checkpoint, the last (T = 1, seed + 1) is kept, drawn under the filter
        res = asr.transcribe(clip, max_new_tokens=8, temperature=(0.0, 1.0), seed=4, top_k=30)
        eng.set_sampling(1.0, 0.0, 5)
        eng.set_sampling_filter(30, 1.0)
        want = eng.transcribe_batch([clip], None, 8)[0]
        eng.set_sampling_filter(0, 1.0)
        eng.set_sampling(0.0)
        assert res.temperature == 1.0 and res.ids == want
        with pytest.raises(Q3aError, match="temperature > 0"):
            asr.transcribe(clip, max_new_tokens=4, top_k=5)
        assert asr.transcribe(clip, max_new_tokens=8).ids == plain.ids
    finally:
        asr.engine.close()
