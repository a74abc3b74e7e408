"""Row options on the GPU (q3a_set_row_options / q3a_set_sequence_bias_lists; include/q3asr.h "row options"): the kernels alone
against tests/row_options_ref.py through q3a_selftest_row_options, rows independent of their neighbours' settings through the stage
API, graph replay against the eager stage API and the ways back, the refusals, device memory across cycles, and
AsrInference.transcribe_batch.  The ids of the kernel test are exact: tests/test_row_options_host.py holds every sampled draw of its
cases clear of a near tie.  Bounds are the existing tests': EPS / 2 on a noisy score and 1e-4 on a log-probability
(tests/test_gpu_sampling.py), DELTA on a top-p threshold (tests/sampling_filter_ref.py, derived in the header)."""
import numpy as np
import pytest

import logit_bias_ref as B_
import row_options_ref as W
import sampling_filter_ref as F
import sampling_ref as R
import seqbias_ref as Q
from align_ref import tiny_aligner_dir
from qwen3_asr_rs_amd import _lib, synthetic
from qwen3_asr_rs_amd.engine import AsrInference, HipEngine, Q3aError, RowOptions
from test_gpu_sampling import EPS
from test_gpu_seqbias import LP_TOL

pytestmark = pytest.mark.gpu

C = _lib.C
f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
NINF = float("-inf")
SEED = (3 << 32) + 515


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _table(recs):
    table = (_lib.RowOptionsC * len(recs))()
    for c, r in zip(table, recs):
        (c.temperature, c.min_p, c.seed, c.top_k, c.top_p, c.repetition_penalty, c.no_repeat_ngram_size,
         c.sequence_list) = (r.temperature, r.min_p, r.seed, r.top_k, r.top_p, r.repetition_penalty, r.no_repeat_ngram_size, r.sequence_list)
    return table


def _selftest(rows, hists, recs, lists):
    lib = _lib.load()
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    S, V = rows.shape
    stride = max(1, max(len(h) for h in hists))
    hist = np.zeros((S, stride), np.int32)
    for s, h in enumerate(hists):
        hist[s, :len(h)] = h
    lens = np.array([len(h) for h in hists], np.int32)
    ids, sl, sb, ll = W.flatten_lists(lists)
    out, tok, lp = np.zeros_like(rows), np.full(S, -7, np.int32), np.zeros(S, np.float32)
    z, thr, kept = np.zeros(S, np.float32), np.zeros(S, np.float32), np.full(S, -7, np.int32)
    n = len(sl)
    rc = lib.q3a_selftest_row_options(0, rows.ctypes.data_as(f32p), S, V, hist.ctypes.data_as(i32p), stride, lens.ctypes.data_as(i32p), _table(recs),
                                      ids.ctypes.data_as(i32p) if n else None, sl.ctypes.data_as(i32p) if n else None,
                                      sb.ctypes.data_as(f32p) if n else None, ll.ctypes.data_as(i32p) if len(lists) else None, len(lists),
                                      out.ctypes.data_as(f32p), tok.ctypes.data_as(i32p), lp.ctypes.data_as(f32p), z.ctypes.data_as(f32p),
                                      thr.ctypes.data_as(f32p), kept.ctypes.data_as(i32p))
    assert rc == 0, lib.q3a_last_error(None)
    return out, tok, lp, z, thr, kept


# ---- 1. the kernels alone, against the reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("V,rev", W.all_cases())
def test_kernels_against_the_reference(V, rev):
    """Six rows with six different records (tests/row_options_ref.py), histories of 0, 1, 31, 32, 257 and 40 / 4200 ids, two lists that
    share a target: l'' bit for bit, ids exact, the kept count exact where top-p is off, the threshold inside the sandwich where it
    is on, greedy rows at -inf with their finite count, and the unfiltered sampled row with the bits of q3a_selftest_sample."""
    rows, hists, recs, lists = W.kernel_case(V, rev)
    want = W.run(rows, hists, recs, lists)
    out, tok, lp, z, thr, kept = _selftest(rows, hists, recs, lists)
    worst_z = worst_lp = 0.0
    for s, (c, w) in enumerate(zip(recs, want)):
        where = (V, rev, s, c)
        assert np.array_equal(_bits(out[s]), _bits(w.logits)), (where, np.nonzero(_bits(out[s]) != _bits(w.logits)))
        assert W.is_safe(w, c), where                                   # (held on the CPU by tests/test_row_options_host.py)
        print(f"[row options] V={V} rev={rev} row {s}: id {int(tok[s])} (ref {w.id}) z {float(z[s])!r} (ref {w.z!r}) lp {float(lp[s])!r} "
              f"(ref {w.lp!r}) thr {float(thr[s])!r} kept {int(kept[s])} (ref {w.thr!r}, {w.kept})")
        assert int(tok[s]) == w.id, where
        if not c.p_on:
            assert _bits(thr[s]) == _bits(w.thr) and int(kept[s]) == w.kept, (where, thr[s], kept[s], w.thr, w.kept)
        else:
            (lo_t, lo_n), (hi_t, hi_n) = F.sandwich(w.logits, c.temperature, c.top_k, c.top_p, F.DELTA)
            assert lo_t <= thr[s] <= hi_t and hi_n <= int(kept[s]) <= lo_n, (where, thr[s], kept[s], (lo_t, lo_n), (hi_t, hi_n))
        if not c.sampled:
            assert np.isneginf(thr[s]) and int(kept[s]) == int(np.isfinite(w.logits).sum()), where
            assert _bits(z[s]) == _bits(w.logits[w.id]), where          # z = l itself, no noise and no fma
        worst_z = max(worst_z, abs(float(z[s]) - w.z))
        worst_lp = max(worst_lp, abs(float(lp[s]) - w.lp))
        assert abs(float(z[s]) - w.z) <= EPS / 2, (where, float(z[s]), w.z)
        assert abs(float(lp[s]) - w.lp) <= LP_TOL, (where, float(lp[s]), w.lp)
    # the unfiltered sampled row (T = 1, nothing else) next to filtering rows: the bits of the sampler alone at the same s and step
    s2 = [i for i, c in enumerate(recs) if c.sampled and not c.filtered][0]
    lib = _lib.load()
    alone = np.ascontiguousarray(np.repeat(rows[s2][None], s2 + 1, axis=0))
    ids1, lp1, z1 = np.full(s2 + 1, -7, np.int32), np.zeros(s2 + 1, np.float32), np.zeros(s2 + 1, np.float32)
    rc = lib.q3a_selftest_sample(0, alone.ctypes.data_as(f32p), s2 + 1, V, C.c_float(1.0), C.c_float(0.0), C.c_uint64(recs[s2].seed),
                                 len(hists[s2]), ids1.ctypes.data_as(i32p), lp1.ctypes.data_as(f32p), z1.ctypes.data_as(f32p))
    assert rc == 0, lib.q3a_last_error(None)
    assert int(ids1[s2]) == int(tok[s2]) and _bits(z1[s2]) == _bits(z[s2]) and _bits(lp1[s2]) == _bits(lp[s2]), (V, rev, s2)
    assert np.isneginf(thr[s2])
    print(f"[row options] V={V} rev={rev}: largest |z - z_ref| {worst_z:.3e} (EPS / 2 {EPS / 2:.2e}), largest |lp - log_softmax64| {worst_lp:.2e}")


def test_a_single_list_is_the_uniform_sequence_bias():
    """The layout of one list is what q3a_set_sequence_bias lays out (there is no host entry point to the words: compared through the
    two selftests): greedy rows that all read list 0 give q3a_selftest_seqbias's logits, ids and log-probability bits; and a table
    without anything on leaves the rows alone."""
    from test_gpu_seqbias import _selftest as seqbias_selftest
    for S, rows, hists, entries in Q.kernel_cases(2049)[:6]:
        want = seqbias_selftest(rows, hists, entries)
        got = _selftest(rows, hists, [W.Record(sequence_list=0)] * S, [entries])
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(want, got[:3])), (S, len(entries))
        off = _selftest(rows, hists, [W.Record()] * S, [entries])
        assert np.array_equal(_bits(off[0]), _bits(rows))


# ---- 2. rows are independent of their neighbours' settings -------------------------------------------------------------------
def _clips(n, seed0=40, base=1.0):
    return [synthetic.synthetic_clip(seed0 + i, base + 0.25 * (i % 4)) for i in range(n)]


def _stage_run(eng, clips, steps):
    """Prefill + decode through the stage API: logits_out [steps][B][V], ids [steps][B], log-probabilities [B][<= steps]."""
    eng.mel(clips)
    eng.encode()
    logits, nxt = eng.prefill([HipEngine.build_prompt(t) for t in eng._T])
    L, T = [logits.copy()], [nxt.copy()]
    for _ in range(steps - 1):
        lg, nx, _ = eng.decode_step()
        L.append(lg.copy())
        T.append(nx.copy())
    return np.stack(L), np.stack(T), eng.fetch_logprobs()


LIST_A = [((7,), -2.5), ((11, 12), 3.0), ((13,), NINF)]
LIST_B = [((7,), 1.25), ((9,), NINF), ((11, 12), -1.0)]


def _mixed_rows(B):
    rows = [RowOptions(),
            RowOptions(temperature=1.0, seed=SEED + 1),
            RowOptions(temperature=0.7, top_k=5, seed=SEED + 2, sequence_bias=LIST_B),
            RowOptions(repetition_penalty=1.3, no_repeat_ngram_size=2, sequence_bias=LIST_A),
            RowOptions(temperature=1.0, top_k=50, top_p=0.9, min_p=0.01, repetition_penalty=0.8, no_repeat_ngram_size=3, seed=SEED + 4,
                       sequence_bias=LIST_B)]
    return [rows[2], rows[0]] if B == 2 else rows[:B]


def _set_uniform(eng, r):
    eng.set_row_options(None)
    eng.set_sampling(r.temperature, r.min_p, r.seed)
    eng.set_sampling_filter(r.top_k, r.top_p)
    eng.set_repetition(r.repetition_penalty, r.no_repeat_ngram_size)
    eng.set_sequence_bias(r.sequence_bias)


@pytest.mark.parametrize("precise,B", [(False, 2), (False, 5), (True, 5)])
def test_rows_do_not_depend_on_their_neighbours_settings(tiny_dir, precise, B):
    """B = 2 the GEMV heads, 5 the gemm16 epilogue, once in the precise mode; 8 steps.  A batch under a mixed table, then the same
    batch on the same engine with each record as the engine's uniform setting: row s of the mixed run has the ids (and, sampled, the
    log-probability bits) of the uniform run of its record, on the same stored logits; a greedy row with nothing on has the ids of an
    engine that never had a setting, and every greedy row's log-probability is log_softmax64 of its own stored logits."""
    steps, clips, table = 8, _clips(B), _mixed_rows(B)
    fresh = HipEngine(tiny_dir, 0, precise=precise, max_new_tokens=16, token_logprobs=True)
    try:
        _, T0, _ = _stage_run(fresh, clips, steps)
    finally:
        fresh.close()
    eng = HipEngine(tiny_dir, 0, precise=precise, max_new_tokens=16, token_logprobs=True)
    try:
        eng.set_row_options(table)
        st = eng.row_options_stats()
        assert st["active"] and len(st["rows"]) == B and [r["temperature"] for r in st["rows"]] == [float(np.float32(r.temperature)) for r in table]
        L, T, lps = _stage_run(eng, clips, steps)
        assert not np.isnan(L).any()
        for s, r in enumerate(table):
            _set_uniform(eng, r)
            Lu, Tu, lpu = _stage_run(eng, clips, steps)
            where = (precise, B, s)
            assert np.array_equal(T[:, s], Tu[:, s]), (where, T[:, s], Tu[:, s])
            assert np.array_equal(_bits(L[:, s]), _bits(Lu[:, s])), where          # the same stored logits: the comparison stands
            n = min(len(lps[s]), len(lpu[s]))
            assert len(lps[s]) == len(lpu[s]) and n >= 1
            if r.temperature > 0:
                assert np.array_equal(_bits(lps[s]), _bits(lpu[s])), where
            else:
                if r.sequence_bias is None and r.repetition_penalty == 1.0:
                    assert np.array_equal(T[:, s], T0[:, s]), (where, T[:, s], T0[:, s])
                for t in range(n):
                    ref = float(R.log_softmax64(L[t][s])[int(T[t][s])])
                    assert abs(float(lps[s][t]) - ref) <= LP_TOL, (where, t, float(lps[s][t]), ref)
                    assert int(T[t][s]) == Q.argmax(L[t][s]), (where, t)
    finally:
        eng.close()


# ---- 3. graph, eager, and the ways back --------------------------------------------------------------------------------------
def _stats(eng):
    return eng.debug_read_raw("lm_head_prune_stats").view(np.int32).copy()


def _captures(eng):
    return int(eng.debug_read_raw("graph_captures").view(np.int32)[0])


def test_graph_eager_other_table_and_back(tiny_dir):
    B, kmax = 5, 10
    clips, table = _clips(B, 80, 1.5), _mixed_rows(5)
    eager = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True, use_graph=False)
    try:
        eager.set_row_options(table)
        _stage_run(eager, clips, kmax)
        want, want_lp = eager.fetch_ids(kmax), eager.fetch_logprobs()
    finally:
        eager.close()
    eng = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True)
    try:
        plain = eng.transcribe_batch(clips, None, max_new=kmax), eng.fetch_logprobs()    # before a table was ever set
        eng.set_row_options(table)
        with pytest.raises(Q3aError, match="nothing generated"):                          # the decode state is dropped
            eng.fetch_ids(kmax)
        r1 = eng.transcribe_batch(clips, None, max_new=kmax), eng.fetch_logprobs()
        r2 = eng.transcribe_batch(clips, None, max_new=kmax), eng.fetch_logprobs()
        assert r1[0] == want and r1[0] != plain[0], (r1[0], want)                         # graph replay == the eager stage API
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(want_lp, r1[1]))
        assert r2[0] == r1[0] and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(r1[1], r2[1]))
        g0 = _captures(eng)
        other = [RowOptions(temperature=0.9, top_p=0.7, seed=5), RowOptions(no_repeat_ngram_size=1), RowOptions(sequence_bias=LIST_A),
                 RowOptions(temperature=1.1, top_k=3, seed=9), RowOptions(repetition_penalty=1.1, sequence_bias=LIST_B)]
        eng.set_row_options(other)                                                        # the same switches, other values and rows
        r3 = eng.transcribe_batch(clips, None, max_new=kmax)
        assert _captures(eng) == g0 and r3 != r1[0]
        eng.set_row_options(None)
        assert eng.row_options_stats() == {"active": False, "rows": []}
        back = eng.transcribe_batch(clips, None, max_new=kmax), eng.fetch_logprobs()
        assert back[0] == plain[0] and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(back[1], plain[1]))
    finally:
        eng.close()


def test_the_pruned_argmax_returns_after_the_table(tiny_dir):
    """B = 1 without log-probabilities: the greedy step is the pruned pair; after a table was set and cleared its pass counts advance as
    on an engine that never had one, and the ids are its ids."""
    clip, steps = synthetic.synthetic_clip(0, 9.3), 10
    never = HipEngine(tiny_dir, 0, max_new_tokens=steps)
    want = never.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)
    s_never = _stats(never)
    never.close()
    eng = HipEngine(tiny_dir, 0, max_new_tokens=steps)
    try:
        eng.set_row_options([RowOptions(temperature=1.0, top_k=20, seed=3, sequence_bias=LIST_A)])
        a = eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)
        assert a != want and (_stats(eng) == 0).all()
        eng.set_row_options(None)
        assert eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps) == want
        assert (_stats(eng) == s_never).all(), (_stats(eng), s_never)
    finally:
        eng.close()


# ---- 4. refusals and state ---------------------------------------------------------------------------------------------------
def test_refusals_and_state(tiny_dir):
    clips = _clips(5, 20)
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8, token_logprobs=True)
    try:
        targets = [[5, 6, 7]] * 3
        score0 = eng.score_batch(clips[:3], targets)
        eng.set_row_options(_mixed_rows(5))
        with pytest.raises(Q3aError, match="a batch of 3 sequences under a row table of 5 rows"):
            eng.transcribe_batch(clips[:3], None, max_new=4)
        score1 = eng.score_batch(clips[:3], targets)                                      # scoring never sees the table
        assert all(np.array_equal(_bits(x), _bits(y)) for a, b in zip(score0, score1) for x, y in ((a[0], b[0]), (a[2], b[2])))
        # beam search (1 clip x width 2 = 2 rows) and a draft (1 row) while any row has something on
        eng.set_row_options([RowOptions(), RowOptions(temperature=0.5)])
        with pytest.raises(Q3aError, match="sampling is on"):
            eng.beam_search_batch(clips[:1], 2, None, 4)
        eng.set_row_options([RowOptions(temperature=0.5)])
        with pytest.raises(Q3aError, match="sampling is on"):
            eng.transcribe_draft_batch(clips[:1], [[5, 6]], None, 4)
        eng.set_row_options([RowOptions(no_repeat_ngram_size=2), RowOptions()])
        with pytest.raises(Q3aError, match="repetition control is on"):
            eng.beam_search_batch(clips[:1], 2, None, 4)
        eng.set_row_options([RowOptions(sequence_bias=LIST_A)])
        with pytest.raises(Q3aError, match="a sequence bias is on"):
            eng.transcribe_draft_batch(clips[:1], [[5, 6]], None, 4)
        eng.set_row_options([RowOptions(), RowOptions()])                                 # an all-off table: both are accepted
        assert len(eng.beam_search_batch(clips[:1], 2, None, 4)) == 1
        eng.set_row_options([RowOptions()])
        assert len(eng.transcribe_draft_batch(clips[:1], [[5, 6]], None, 4)[0]) == 1
        # the two finite-logit rules, tripped by one row only
        eng.set_row_options(None)
        eng.set_logit_bias({5: 0.0, 6: 0.0, 7: 0.0}, default=NINF)                        # an allow-list of 3, both EOS ids closed
        ok = RowOptions()
        with pytest.raises(Q3aError, match="row 1.*no_repeat_ngram_size 2"):
            eng.set_row_options([ok, RowOptions(no_repeat_ngram_size=2)])
        with pytest.raises(Q3aError, match="row 2.*-inf sequence-bias entries"):
            eng.set_row_options([ok, ok, RowOptions(sequence_bias=[((5,), NINF), ((6,), NINF), ((7,), NINF)])])
        assert eng.row_options_state is None and eng.row_options_stats()["active"] is False
        eng.set_row_options([ok, ok])                                                     # the engine stays usable
        eng.set_logit_bias(None)
    finally:
        eng.close()
    al = HipEngine(tiny_aligner_dir(), 0)
    try:
        with pytest.raises(Q3aError, match="forced aligner"):
            al.set_row_options([RowOptions()])
    finally:
        al.close()


# ---- 5. device memory --------------------------------------------------------------------------------------------------------
def test_device_memory_is_level_across_cycles(tiny_dir):
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8)
    try:
        size = lambda: int(eng.debug_read_raw("device_bytes").view(np.uint64)[0])
        clips, table = _clips(5, 30), _mixed_rows(5)
        seen = []
        for _ in range(11):
            eng.set_row_options(table)
            eng.transcribe_batch(clips, None, max_new=3)
            eng.set_row_options(None)
            seen.append(size())
        assert len(set(seen[1:])) == 1 and seen[0] == seen[1], seen
    finally:
        eng.close()


# ---- 6. AsrInference.transcribe_batch ----------------------------------------------------------------------------------------
def test_transcribe_batch_with_options(tiny_dir):
    clips = _clips(3, 80, 1.5)
    table = [RowOptions(temperature=0.7, top_k=5, seed=SEED + 2, sequence_bias=LIST_B), RowOptions(),
             RowOptions(repetition_penalty=1.3, no_repeat_ngram_size=2, sequence_bias=LIST_A)]
    eng = HipEngine(tiny_dir, 0, max_new_tokens=10, token_logprobs=True)
    try:
        eng.set_row_options(table)
        want = eng.transcribe_batch(clips, None, max_new=10), eng.fetch_logprobs()
        eng.set_row_options(None)
        eng.set_sequence_bias(LIST_A)                                                     # the engine's own state, to be found again
        asr = AsrInference(eng)
        opts = [dict(temperature=0.7, top_k=5, seed=SEED + 2, sequence_bias=LIST_B), None,
                dict(repetition_penalty=1.3, no_repeat_ngram_size=2, sequence_bias=dict(LIST_A))]
        got = asr.transcribe_batch(clips, max_new_tokens=10, options=opts)
        assert [r.ids for r in got] == want[0] and [r.temperature for r in got] == [0.7, 0.0, 0.0]
        assert all(np.array_equal(_bits(r.token_logprobs), _bits(w)) for r, w in zip(got, want[1]))
        assert eng.row_options_state is None and eng.sequence_bias_stats()["entries"] == len(LIST_A)
        for bad, word in (([dict(temperature=(0.0, 0.5)), None, None], "tuple of temperatures"), ([dict(beam_size=2), None, None], "beam_size"),
                          ([None, dict(draft=[1, 2]), None], "draft"), ([None, None, dict(logit_bias={1: 1.0})], "logit_bias"),
                          ([dict(top_k=5), None, None], "temperature > 0"), ([None, None], "2 option dict")):
            with pytest.raises(Q3aError, match=word):
                asr.transcribe_batch(clips, options=bad)
        # an exception inside the call: the engine's previous state is back
        with pytest.raises(Q3aError, match="a batch of 2"):
            orig = eng.transcribe_batch
            eng.transcribe_batch = lambda c, *a, **k: orig(c[:2], *a, **k)
            try:
                asr.transcribe_batch(clips, options=opts)
            finally:
                del eng.transcribe_batch
        assert eng.row_options_state is None and eng.sequence_bias_stats()["entries"] == len(LIST_A)
        assert eng.row_options_stats()["active"] is False
    finally:
        eng.close()
