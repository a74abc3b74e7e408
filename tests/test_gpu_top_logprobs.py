"""Top log-probabilities on the GPU (q3a_set_top_logprobs; k_toplp.hip): the two launches
against the float64 reference through q3a_selftest_top_logprobs, every lm_head form feeding them, graph replay against the eager stage
API, another n on the same graph, the way back to an engine that never had the setting, the composition with the other logits
processors, ragged stops, a batch that grows and shrinks, the refusals and the device memory across cycles.

The rules (include/q3asr.h "top log-probabilities").  The ids are the reference's exactly, ties included: kernel and reference read
the same fp32 values.  lp is within 1e-4 of the float64 log_softmax, -inf exactly where the logit is -inf, and a second run on the
same scratch is bit-equal to the first (the selftest runs twice and fails otherwise)."""
import numpy as np
import pytest

import logit_bias_ref as B_
import top_logprobs_ref as T
from align_ref import tiny_aligner_dir
from qwen3_asr_rs_amd import _lib, synthetic
from qwen3_asr_rs_amd.engine import AsrInference, HipEngine, Q3aError

pytestmark = pytest.mark.gpu

V = 151936
LP_TOL = 1e-4
C = _lib.C


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _selftest(rows, n, step_count, done, stride):
    lib = _lib.load()
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    S, Vr = rows.shape
    sc, dn = np.ascontiguousarray(step_count, dtype=np.int32), np.ascontiguousarray(done, dtype=np.uint8)
    ids, lp = np.full((S, stride, T.INNER), -7, np.int32), np.full((S, stride, T.INNER), 7.0, np.float32)
    f32p, i32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    rc = lib.q3a_selftest_top_logprobs(0, rows.ctypes.data_as(f32p), S, Vr, n, sc.ctypes.data_as(i32p), dn.ctypes.data_as(u8p), stride,
                                       ids.ctypes.data_as(i32p), lp.ctypes.data_as(f32p))
    assert rc == 0, lib.q3a_last_error(None)
    return ids, lp


def _compare(got_ids, got_lp, want_ids, want_lp, where):
    """ids exactly; lp within LP_TOL, -inf exactly where the reference has -inf.  Returns the largest |lp - lp64| over finite entries."""
    assert np.array_equal(got_ids, want_ids), (where, got_ids.tolist(), np.asarray(want_ids).tolist())
    inf = np.isneginf(want_lp)
    assert np.array_equal(np.isneginf(got_lp), inf) and not np.isnan(got_lp).any(), (where, got_lp, want_lp)
    err = np.abs(got_lp.astype(np.float64)[~inf] - want_lp[~inf])
    worst = float(err.max()) if err.size else 0.0
    assert worst <= LP_TOL, (where, worst)
    return worst


def _check_history(rows, n, step_count, done, stride, where):
    ids, lp = _selftest(rows, n, step_count, done, stride)
    want_ids, want_lp, written = T.history_ref(rows, n, step_count, done, stride)
    assert (ids[~written] == T.UNWRITTEN[0]).all() and (lp[~written] == T.UNWRITTEN[1]).all(), where   # nothing else was touched
    assert (ids[written] >= 0).all()
    return _compare(ids[written], lp[written], want_ids[written], want_lp[written], where)


# ---- 1. the kernels against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("Vk", T.KERNEL_V)
def test_kernels_against_the_reference(Vk):
    """V = 20, 63, 2048, 2049, 4100, 6150; S = 1 and 3; n = 1, 2, 8, 20 (n <= V); random rows, every second one quantised so that
    hundreds of entries tie; every row at a slot of its own."""
    worst = 0.0
    for S in (1, 3):
        rows = T.random_rows(Vk, S, 100 + Vk + S)
        for n in T.KERNEL_N:
            if n > Vk:
                continue
            sc = [(2 * s + n) % 5 for s in range(S)]
            worst = max(worst, _check_history(rows, n, sc, [0] * S, 5, (Vk, S, n)))
    print(f"[top logprobs] V={Vk}: largest |lp - log_softmax64| {worst:.2e}")


def test_kernels_at_the_real_vocabulary():
    """V = 151936 once (75 chunks, 1500 candidates in the row kernel): a random row, and a row whose 20 best stand in 20 chunks."""
    rows, at = T.big_rows()
    ids, lp = _selftest(rows, 20, [0, 1], [0, 0], 2)
    assert ids[1, 1].tolist() == at.tolist()
    want_ids, want_lp, written = T.history_ref(rows, 20, [0, 1], [0, 0], 2)
    worst = _compare(ids[written], lp[written], want_ids[written], want_lp[written], "big")
    assert (ids[~written] == -1).all()
    print(f"[top logprobs] V={V}: largest |lp - log_softmax64| {worst:.2e}")


def test_hand_made_rows():
    """The rows of top_logprobs_ref.hand_rows (tests/test_top_logprobs_host.py holds what they contain), each alone and all with the same
    n in one call; then a done row and a row without a slot next to a live one."""
    hand = T.hand_rows()
    worst = 0.0
    for name, (row, n, claim) in hand.items():
        ids, lp = _selftest(row[None], n, [1], [0], 3)
        assert ids[0, 1, :n].tolist() == claim, name
        worst = max(worst, _check_history(row[None], n, [1], [0], 3, name))
    ids, lp = _selftest(hand["few_finite"][0][None], 8, [0], [0], 1)
    assert np.isfinite(lp[0, 0, :3]).all() and np.isneginf(lp[0, 0, 3:8]).all()
    ids, lp = _selftest(hand["steep"][0][None], 20, [0], [0], 1)
    assert lp[0, 0, 0] == 0.0 and lp[0, 0, 1] == -1000.0 and lp[0, 0, 19] == -19000.0   # the sum is exactly 1: the tail underflows
    names = ("one_chunk", "all_equal", "steep", "few_finite", "zeros_boundary")
    rows = np.stack([hand[k][0] for k in names])
    worst = max(worst, _check_history(rows, 20, [0, 1, 2, 3, 4], [0] * 5, 5, "together"))
    # done = 1, and step_count >= stride: both write nothing; the live row between them is not disturbed
    rows3 = np.stack([hand["one_chunk"][0], hand["spread"][0], hand["tie_2047_2048"][0]])
    for sc, dn in (([1, 1, 1], [1, 0, 0]), ([1, 4, 0], [0, 0, 1]), ([4, 9, 1 << 30], [0, 0, 0]), ([-1, 2, -5], [0, 0, 0])):
        _check_history(rows3, 4, sc, dn, 4, (sc, dn))
    ids, _ = _selftest(rows3, 4, [4, 9, 1 << 30], [0, 0, 0], 4)
    assert (ids == -1).all()
    print(f"[top logprobs] hand-made rows: largest |lp - log_softmax64| {worst:.2e}")


# ---- 2. every head form stores what the two kernels read -------------------------------------------------------------------
def _clips(n, seed0=40, base=1.0):
    return [synthetic.synthetic_clip(seed0 + i, base + 0.25 * (i % 4)) for i in range(n)]


def _stage_run(eng, clips, steps, forced=None):
    """Prefill + decode through the stage API: logits [steps][B][V] and ids [steps][B].  forced[t]: ids fed after step t instead."""
    eng.mel(clips)
    eng.encode()
    logits, nxt = eng.prefill([HipEngine.build_prompt(t) for t in eng._T])
    L, Tk = [logits.copy()], [nxt.copy()]
    for t in range(steps - 1):
        if forced is not None:
            eng.set_next_tokens(forced[t])
        lg, nx, _ = eng.decode_step()
        L.append(lg.copy())
        Tk.append(nx.copy())
    return np.stack(L), np.stack(Tk)


def _check_against_logits(L, top, n, where, steps=None):
    """Every step's entries against that step's own logits."""
    worst = 0.0
    for q, (ids, lp) in enumerate(top):
        k = len(ids) if steps is None else steps
        assert ids.shape == lp.shape == (len(ids), n) and len(ids) >= k, (where, q, ids.shape)
        for t in range(k):
            wi, wl = T.top_ref(L[t][q][None], n)
            worst = max(worst, _compare(ids[t], lp[t], wi[0], wl[0], (where, q, t)))
    return worst


@pytest.mark.parametrize("precise,B,n", [(False, 1, 5), (False, 2, 20), (False, 5, 8), (True, 5, 3)])
def test_every_head_form_feeds_the_phases(tiny_dir, precise, B, n):
    """B = 1 and 2 the GEMV heads, 5 the gemm16 argmax epilogue, and the precise mode: 8 steps through the stage API, every step's
    entries against that step's own logits_out; greedy, so entry 0 is the id that was written."""
    steps = 8
    eng = HipEngine(tiny_dir, 0, precise=precise, max_new_tokens=16)
    try:
        eng.set_top_logprobs(n)
        assert eng.top_logprobs_stats() == {"active": True, "n": n}
        L, Tk = _stage_run(eng, _clips(B), steps)
        top = eng.fetch_top_logprobs()
        ids = eng.fetch_ids(16)
    finally:
        eng.close()
    assert not np.isnan(L).any() and len(top) == B
    worst = _check_against_logits(L, top, n, (precise, B), steps)
    for q in range(B):
        assert len(top[q][0]) == len(ids[q]) == steps
        assert top[q][0][:, 0].tolist() == ids[q] == Tk[:, q].tolist()
    print(f"[top logprobs] precise={precise} B={B} n={n}: largest |lp - log_softmax64| {worst:.2e}")


def test_teacher_forcing_keeps_each_steps_own_row(tiny_dir):
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8)
    try:
        eng.set_top_logprobs(4)
        forced = [[1000 + 7 * t, 2000 + 3 * t] for t in range(5)]
        L, Tk = _stage_run(eng, _clips(2, 44), 6, forced)
        top = eng.fetch_top_logprobs()
    finally:
        eng.close()
    _check_against_logits(L, top, 4, "forced", 6)


# ---- 3. graph, eager, another n on the same graph, and the way back -------------------------------------------------------------
def _stats(eng):
    return eng.debug_read_raw("lm_head_prune_stats").view(np.int32).copy()


def _captures(eng):
    return int(eng.debug_read_raw("graph_captures").view(np.int32)[0])


def _same_top(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(_bits(x[1]), _bits(y[1])) for x, y in zip(a, b))


@pytest.mark.parametrize("B", [1, 5])
def test_graph_eager_another_n_and_the_way_back(tiny_dir, B):
    clips, kmax = _clips(B, 80, 1.5), 10
    fix = dict(max_new=kmax, fixed_new_tokens=kmax)
    fresh = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True)           # never had the setting
    greedy = fresh.transcribe_batch(clips, None, **fix), fresh.fetch_logprobs(), _stats(fresh)
    with pytest.raises(Q3aError, match="top log-probabilities off"):
        fresh.fetch_top_logprobs()
    fresh.close()
    eager = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True, use_graph=False)
    try:
        eager.set_top_logprobs(5)
        L, Tk = _stage_run(eager, clips, kmax)
        want, want_lp = eager.fetch_top_logprobs(), eager.fetch_logprobs()
    finally:
        eager.close()
    _check_against_logits(L, want, 5, ("eager", B), kmax)
    eng = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True)
    try:
        eng.set_top_logprobs(5)
        r1 = eng.transcribe_batch(clips, None, **fix), eng.fetch_top_logprobs(), eng.fetch_logprobs()
        n_graphs = _captures(eng)
        r2 = eng.transcribe_batch(clips, None, **fix), eng.fetch_top_logprobs()
        assert r1[0] == greedy[0] == r2[0]                                             # the setting only reads the row
        assert _same_top(r1[1], want)                                                  # graph replay == the eager stage API
        assert _same_top(r1[1], r2[1])                                                 # bit-identical twice
        for q in range(B):
            assert r1[1][q][0][:, 0].tolist() == r1[0][q]                              # greedy: entry 0 is the written id
            assert np.abs(r1[1][q][1][:, 0].astype(np.float64) - r1[2][q].astype(np.float64)).max() <= 2e-4   # two fp32 sums
            assert np.array_equal(_bits(r1[2][q]), _bits(greedy[1][q])) and np.array_equal(_bits(r1[2][q]), _bits(want_lp[q][:kmax]))
        # another n > 0 replays the same graph
        eng.set_top_logprobs(20)
        with pytest.raises(Q3aError, match="nothing generated"):                       # the decode state is dropped
            eng.fetch_top_logprobs()
        r3 = eng.transcribe_batch(clips, None, **fix), eng.fetch_top_logprobs()
        assert _captures(eng) == n_graphs and r3[0] == greedy[0]
        for q in range(B):
            assert r3[1][q][0].shape == (kmax, 20)
            assert np.array_equal(r3[1][q][0][:, :5], r1[1][q][0]) and np.array_equal(_bits(r3[1][q][1][:, :5]), _bits(r1[1][q][1]))
        # off again: the ids, log-probability bits and pruned-pass counts of an engine that never had the setting
        eng.set_top_logprobs(0)
        assert eng.top_logprobs_stats() == {"active": False, "n": 0}
        s0 = _stats(eng)
        back = eng.transcribe_batch(clips, None, **fix), eng.fetch_logprobs()
        s1 = _stats(eng)
        with pytest.raises(Q3aError, match="top log-probabilities off"):
            eng.fetch_top_logprobs()
    finally:
        eng.close()
    assert back[0] == greedy[0] and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(back[1], greedy[1]))
    assert (s0 == 0).all(), s0                                                         # no pruned pass ran while it was on
    assert (s1 - s0 == greedy[2]).all(), (s0, s1, greedy[2])


def test_off_again_keeps_the_pruned_head_without_token_logprobs(tiny_dir):
    """One sequence without token_logprobs: the pruned lm_head runs when the setting is off, does not while it is on, and runs again,
    with the same counts, after n = 0."""
    clips, kmax = _clips(1, 83, 1.5), 8
    fix = dict(max_new=kmax, fixed_new_tokens=kmax)
    fresh = HipEngine(tiny_dir, 0, max_new_tokens=kmax)
    ids0, st0 = fresh.transcribe_batch(clips, None, **fix), _stats(fresh)
    fresh.close()
    eng = HipEngine(tiny_dir, 0, max_new_tokens=kmax)
    try:
        eng.set_top_logprobs(3)
        assert eng.transcribe_batch(clips, None, **fix) == ids0
        assert (_stats(eng) == 0).all()
        eng.set_top_logprobs(0)
        assert eng.transcribe_batch(clips, None, **fix) == ids0
        assert (_stats(eng) == st0).all(), (_stats(eng), st0)
    finally:
        eng.close()


# ---- 4. composition ----------------------------------------------------------------------------------------------------------
def test_composition_with_bias_repetition_sequence_bias_and_sampling(tiny_dir):
    clips, kmax, n = _clips(3, 70, 1.5), 8, 6
    eng = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True)
    try:
        eng.set_top_logprobs(n)
        L0, T0 = _stage_run(eng, clips, kmax)
        plain = [T0[:, q].tolist() for q in range(3)]
        # a suppress bias: the suppressed ids come last, with -inf (n = 20 at a vocabulary whose finite entries are few)
        allow = sorted(set(t for x in plain for t in x) | {777, 12345, 100000})[:4]   # (a flat checkpoint may repeat one id: four for sure)
        assert len(allow) == 4
        eng.set_logit_bias({i: 0.0 for i in allow}, default=-np.inf)
        eng.set_top_logprobs(20)
        L, Tk = _stage_run(eng, clips, 3)
        top = eng.fetch_top_logprobs()
        _check_against_logits(L, top, 20, "allow-list", 3)
        for q in range(3):
            for t in range(3):
                assert sorted(top[q][0][t, :4].tolist()) == allow and np.isfinite(top[q][1][t, :4]).all()
                assert np.isneginf(top[q][1][t, 4:]).all()
                rest = [i for i in range(40) if i not in allow][:16]
                assert top[q][0][t, 4:].tolist() == rest                                # -inf entries by id
        eng.set_logit_bias(None)
        eng.set_top_logprobs(n)
        # repetition control and a sequence bias: the entries are those of the rewritten row (logits_out holds l'')
        eng.set_repetition(1.5, 2)
        eng.set_sequence_bias([((plain[0][1],), 4.0), ((plain[0][0], plain[0][1]), -np.inf)])
        L, Tk = _stage_run(eng, clips, kmax)
        top = eng.fetch_top_logprobs()
        assert not np.array_equal(L, L0)
        _check_against_logits(L, top, n, "rewritten", kmax)
        for q in range(3):
            assert top[q][0][:, 0].tolist() == Tk[:, q].tolist()
        eng.set_repetition(1.0, 0)
        eng.set_sequence_bias(None)
        # temperature 1 with a seed: the entries are still the untempered row's; the drawn id need not be entry 0
        eng.set_sampling(1.0, 0.0, 77)
        eng.set_sampling_filter(50, 0.9)
        L, Tk = _stage_run(eng, clips, kmax)
        top, lps = eng.fetch_top_logprobs(), eng.fetch_logprobs()
        _check_against_logits(L, top, n, "sampled", kmax)
        drawn_elsewhere = 0
        for q in range(3):
            for t in range(kmax):
                hit = np.flatnonzero(top[q][0][t] == Tk[t, q])
                drawn_elsewhere += len(hit) == 0 or hit[0] != 0
                if len(hit):                                                           # the same distribution as q3a_fetch_logprobs
                    assert abs(float(top[q][1][t, hit[0]]) - float(lps[q][t])) <= 2e-4
        assert drawn_elsewhere > 0
    finally:
        eng.close()


def test_composes_with_a_row_table(tiny_dir):
    from qwen3_asr_rs_amd.engine import RowOptions
    clips, kmax = _clips(3, 75, 1.25), 6
    eng = HipEngine(tiny_dir, 0, max_new_tokens=kmax)
    try:
        eng.set_top_logprobs(4)
        eng.set_row_options([RowOptions(), RowOptions(1.0, 0.0, 5, 20, 0.9), RowOptions(repetition_penalty=1.4, no_repeat_ngram_size=2)])
        L, Tk = _stage_run(eng, clips, kmax)
        top = eng.fetch_top_logprobs()
    finally:
        eng.close()
    _check_against_logits(L, top, 4, "row table", kmax)
    assert top[0][0][:, 0].tolist() == Tk[:, 0].tolist() and top[2][0][:, 0].tolist() == Tk[:, 2].tolist()


# ---- 5. ragged stops -----------------------------------------------------------------------------------------------------------
def test_ragged_stops(tmp_path):
    """Stops planted with eos_plan.plan_ragged_eos (precise mode: the engine follows the oracle the plan was made with): the lengths
    are fetch_ids', and in a run that goes on past the stops (fixed_new_tokens) a stopped row's slots behind its EOS stay as the
    prefill cleared them while its neighbours' fill up."""
    from eos_plan import fresh_eos_checkpoint, plan_ragged_eos
    d = fresh_eos_checkpoint(str(tmp_path / "ckpt"), "tiny_untied", seed=5)
    clips = [synthetic.synthetic_clip(200 + i, 1.0 + 0.17 * (i % 7)) for i in range(5)]
    kmax, n = 7, 3
    stops, _, _ = plan_ragged_eos(d, clips, kmax, [None, 5, 3, 2, 4], margin_min=1e-3)
    eng = HipEngine(d, 0, precise=True, max_new_tokens=kmax)
    try:
        eng.set_top_logprobs(n)
        ids = eng.transcribe_batch(clips, None, max_new=kmax)
        top = eng.fetch_top_logprobs()
        ids_fixed = eng.transcribe_batch(clips, None, max_new=kmax, fixed_new_tokens=kmax)
        top_fixed = eng.fetch_top_logprobs()
    finally:
        eng.close()
    lens = [len(x) for x in ids]
    print(f"[top logprobs] ragged: planned stops {stops}, lengths {lens}")
    assert min(lens) < max(lens) and len(set(lens)) >= 3, (lens, stops)                  # really ragged
    for q in range(5):
        assert top[q][0].shape == (lens[q], n) and top[q][0][:, 0].tolist() == ids[q]
        assert top_fixed[q][0].shape == (kmax, n) and ids_fixed[q][:lens[q]] == ids[q]
        assert np.array_equal(top_fixed[q][0][:lens[q]], top[q][0]) and np.array_equal(_bits(top_fixed[q][1][:lens[q]]), _bits(top[q][1]))
        if lens[q] < kmax:
            assert top_fixed[q][0][lens[q], 0] == synthetic.ENDOFTEXT_ID                 # the EOS step itself is recorded ...
            assert (top_fixed[q][0][lens[q] + 1:] == 0).all() and (_bits(top_fixed[q][1][lens[q] + 1:]) == 0).all()   # ... nothing behind it
        else:
            assert (top_fixed[q][1][:, 0] < 0).all()                                    # a row that goes on is written at every step


# ---- 6. a batch that grows and shrinks ---------------------------------------------------------------------------------------------
def test_batch_grows_and_shrinks_on_one_engine(tiny_dir):
    """1, then 5, then 1 sequences on one engine (the scratch and the history grow with the batch): every run against its own logits,
    and the third run's entries are the first's."""
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8)
    n, steps = 8, 4
    try:
        eng.set_top_logprobs(n)
        runs = []
        for B in (1, 5, 1):
            L, Tk = _stage_run(eng, _clips(B, 50 + B), steps)
            runs.append((B, L, eng.fetch_top_logprobs()))
    finally:
        eng.close()
    for B, L, top in runs:
        assert len(top) == B
        _check_against_logits(L, top, n, ("grow", B), steps)
    assert _same_top(runs[0][2], runs[2][2])


# ---- 7. state, refusals, memory ---------------------------------------------------------------------------------------------------
def test_refusals_and_state(tiny_dir):
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8)
    lib = eng._lib
    clip = synthetic.synthetic_clip(3, 1.0)
    try:
        with pytest.raises(Q3aError, match="nothing generated"):                       # before anything was generated
            eng.batch = 1
            eng.fetch_top_logprobs()
        eng.set_top_logprobs(7)
        for bad in (-1, 21, 1 << 20):
            assert lib.q3a_set_top_logprobs(eng._h, bad) != 0
            assert "n must lie" in lib.q3a_last_error(eng._h).decode()
            assert eng.top_logprobs_stats() == {"active": True, "n": 7}                 # a refused call changes nothing
        got = eng.transcribe_batch([clip], None, max_new=6, fixed_new_tokens=6)
        top = eng.fetch_top_logprobs()
        assert top[0][0].shape == (6, 7) and top[0][0][:, 0].tolist() == got[0]
        # a refused call leaves the decode state too
        assert lib.q3a_set_top_logprobs(eng._h, 21) != 0
        assert _same_top(eng.fetch_top_logprobs(), top)
        # beam search and draft verification are refused while it is on, and leave the setting
        with pytest.raises(Q3aError, match="top log-probabilities are on"):
            eng.beam_search_batch([clip], 2, max_new=4)
        with pytest.raises(Q3aError, match="top log-probabilities are on"):
            eng.transcribe_draft_batch([clip], [got[0][:3]], None, 6)
        eng.mel([clip])
        eng.encode()
        prompt = HipEngine.build_prompt(eng._T[0])
        with pytest.raises(Q3aError, match="top log-probabilities are on"):
            eng.prefill_draft([prompt], [got[0][:3]])
        eng.prefill([prompt])
        with pytest.raises(Q3aError, match="top log-probabilities are on"):
            eng.beam_begin(1)
        eng.decode_step()
        assert eng.top_logprobs_stats() == {"active": True, "n": 7}
        assert eng.fetch_top_logprobs()[0][0].shape == (2, 7)                           # the stage API's two steps
        # a setter drops the decode state: the fetch refuses, as the "sample_threshold" reads do
        eng.set_repetition(1.2, 0)
        with pytest.raises(Q3aError, match="nothing generated"):
            eng.fetch_top_logprobs()
        eng.set_repetition(1.0, 0)
        # the partial fetch: entries past n_stride and rows past out_lens are untouched
        eng.transcribe_batch([clip], None, max_new=6, fixed_new_tokens=6)
        oi, ol, lens = np.full((1, 4, 9), -7, np.int32), np.full((1, 4, 9), 7.0, np.float32), np.zeros(1, np.int32)
        f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        eng._chk(lib.q3a_fetch_top_logprobs(eng._h, oi.ctypes.data_as(i32p), ol.ctypes.data_as(f32p), 4, 9, lens.ctypes.data_as(i32p)))
        assert lens[0] == 6 and np.array_equal(oi[0, :, :7], top[0][0][:4]) and (oi[0, :, 7:] == -7).all() and (ol[0, :, 7:] == 7.0).all()
    finally:
        eng.close()
    al = HipEngine(tiny_aligner_dir(), 0, max_new_tokens=1)
    try:
        with pytest.raises(Q3aError, match="forced aligner"):                          # an aligner engine generates nothing
            al.set_top_logprobs(5)
    finally:
        al.close()


def test_score_is_blind_to_the_setting_and_memory_is_level(tiny_dir):
    clips = _clips(2, 90, 1.0)
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8, token_logprobs=True)
    try:
        plain = eng.transcribe_batch(clips, None, max_new=6, fixed_new_tokens=6)
        targets = [x[:4] + [151645] for x in plain]
        score_off = eng.score_batch(clips, targets)
        eng.set_top_logprobs(5)
        score_on = eng.score_batch(clips, targets)
        for x, y in zip(score_off, score_on):
            assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(x[1], y[1]) and np.array_equal(_bits(x[2]), _bits(y[2]))
        eng.set_top_logprobs(0)

        def cycle():
            eng.set_top_logprobs(5)
            eng.transcribe_batch(clips, None, max_new=6, fixed_new_tokens=6)
            inside = int(eng.debug_read_raw("device_bytes").view(np.uint64)[0])
            eng.set_top_logprobs(20)
            eng.transcribe_batch(clips, None, max_new=6, fixed_new_tokens=6)
            eng.set_top_logprobs(0)
            eng.transcribe_batch(clips, None, max_new=6, fixed_new_tokens=6)
            return inside, int(eng.debug_read_raw("device_bytes").view(np.uint64)[0])
        first = cycle()
        assert first[0] == first[1]                                                    # clearing frees nothing: freed with the engine
        for _ in range(3):
            assert cycle() == first
    finally:
        eng.close()


# ---- 8. AsrInference ---------------------------------------------------------------------------------------------------------------
class _Tok:
    def decode(self, ids, skip):
        return "language English<asr_text>" + " ".join(f"t{i}" for i in ids) if skip else "".join(f"<{i}>" for i in ids)

    def encode(self, text):
        return []


def test_asr_inference_fills_top_logprobs(tiny_dir):
    clip, clip2 = synthetic.synthetic_clip(12, 1.5), synthetic.synthetic_clip(13, 1.25)
    asr = AsrInference.load(tiny_dir, 0, token_logprobs=True, max_new_tokens=16)
    try:
        asr.tokenizer = _Tok()
        eng = asr.engine
        plain = asr.transcribe(clip, max_new_tokens=8)
        assert plain.top_logprobs is None
        res = asr.transcribe(clip, max_new_tokens=8, top_logprobs=5)
        assert res.ids == plain.ids and res.token_logprobs == plain.token_logprobs
        assert len(res.top_logprobs) == len(res.ids) and all(len(c) == 5 for c in res.top_logprobs)
        for i, cands in zip(res.ids, res.top_logprobs):
            assert cands[0].id == i and cands[0].token == f"<{i}>"
            assert all(a.logprob >= b.logprob for a, b in zip(cands, cands[1:]))
        assert eng.top_logprobs_state == 0 and eng.top_logprobs_stats()["active"] is False   # restored
        eng.set_top_logprobs(2)                                                        # the engine's own setting comes back
        both = asr.transcribe(clip, max_new_tokens=8, top_logprobs=5, repetition_penalty=1.3, temperature=(0.0, 1.0), seed=4,
                              suppress_tokens=[plain.ids[0]])
        assert eng.top_logprobs_state == 2 and len(both.top_logprobs) == len(both.ids) and both.temperature == 1.0
        assert all(c.id != plain.ids[0] for cands in both.top_logprobs for c in cands)
        eng.set_top_logprobs(0)
        out = asr.transcribe_batch([clip, clip2], max_new_tokens=6, options=[{"top_logprobs": 3}, {"top_logprobs": 3, "temperature": 1.0}])
        assert all(len(r.top_logprobs) == len(r.ids) and len(r.top_logprobs[0]) == 3 for r in out)
        assert [c[0].id for c in out[0].top_logprobs] == out[0].ids
        assert eng.top_logprobs_state == 0
        with pytest.raises(ValueError, match="equal for all rows"):
            asr.transcribe_batch([clip, clip2], options=[{"top_logprobs": 3}, None])
        assert asr.transcribe(clip, max_new_tokens=8).top_logprobs is None
    finally:
        asr.engine.close()
