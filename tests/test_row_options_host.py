"""Row options without a GPU (include/q3asr.h "row options"): the reference composes the existing references and reproduces them when
every row holds the same record; the kernel test's draws are free of near ties, so tests/test_gpu_row_options.py may demand exact
ids; the Python checks and the collection of the rows' lists; the refusals of q3a_selftest_row_options that are decided before a
device is looked for.  The layout of a single list has no host entry point of its own (the existing sequence-bias host test has none
either): tests/test_gpu_row_options.py compares it through q3a_selftest_row_options against q3a_selftest_seqbias on the GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import repetition_ref as P
import row_options_ref as W
import sampling_filter_ref as F
import sampling_ref as R
import seqbias_ref as Q
from qwen3_asr_rs_amd import _lib, engine
from qwen3_asr_rs_amd.engine import Q3aError, RowOptions, check_row_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- the surfaces exist ------------------------------------------------------------------------------------------------------
def test_symbols_in_header_binding_and_python(lib):
    header = open(os.path.join(ROOT, "include", "q3asr.h")).read()
    for sym in ("q3a_set_row_options", "q3a_set_sequence_bias_lists", "q3a_selftest_row_options"):
        assert re.search(r"^int32_t %s\(" % sym, header, flags=re.M), sym
        assert sym in _lib.SYMBOLS and hasattr(lib, sym), sym
    assert "typedef struct q3a_row_options {" in header and C.sizeof(_lib.RowOptionsC) == 40
    for name in ("set_row_options", "row_options_stats"):
        assert callable(getattr(engine.HipEngine, name))
    assert callable(engine.AsrInference.transcribe_batch)
    flat = " ".join(header.replace(" * ", " ").split())
    sec = flat[flat.index("---- row options:"):flat.index("int32_t q3a_selftest_row_options(")]
    for phrase in ("params becomes params[s]", '"sample_threshold" reads -inf', "without a row table every row uses list 0",
                   "allowed across lists", "another table of the same switches replays the same graph", "n_rows = 0 clears",
                   "whichever of the two setters comes second", "a prefill whose batch differs from n_rows",
                   "Out of scope: logit-bias vectors per row", "per-row max_new_tokens", "a Philox row index other than s"):
        assert phrase in sec, phrase


# ---- the reference -----------------------------------------------------------------------------------------------------------
def test_equal_rows_reproduce_the_existing_references():
    """With one record on every row the composition IS the existing reference, on cases of theirs: the sampler's, the filter's,
    repetition control's and the sequence bias's."""
    V = 2049
    rows = R.kernel_rows(V)
    for g, T, mp, st in R.kernel_calls(V)[:12]:
        rec = W.Record(temperature=T, min_p=mp, seed=R.SAMPLE_SEED)
        for s, r in enumerate(g):
            want, got = R.sample(rows[r], T, mp, R.SAMPLE_SEED, s, st), W.run_row(rows[r], [0] * st, rec, [], s)
            assert (got.id, got.z, got.lp) == (want.id, want.z, want.lp) and got.thr == -np.inf
    frows = F.kernel_rows(V)
    for g, T, mp, k, p, st in F.kernel_calls(V)[:24]:
        rec = W.Record(temperature=T, min_p=mp, seed=F.SAMPLE_SEED[V], top_k=k, top_p=p)
        for s, r in enumerate(g):
            want, got = F.sample(frows[r], T, mp, k, p, F.SAMPLE_SEED[V], s, st), W.run_row(frows[r], [0] * st, rec, [], s)
            assert (got.id, got.z) == (want.id, want.z)
            if rec.filtered:
                assert (got.thr, got.kept) == F.threshold(frows[r], T, k, p)
    for S, prow, hists, p, n in P.kernel_cases(33)[:20]:
        rec = W.Record(repetition_penalty=p, no_repeat_ngram_size=n)
        for s in range(S):
            got = W.run_row(prow[s], hists[s], rec, [], s)
            want = P.apply(prow[s], hists[s], p, n)
            assert np.array_equal(P.bits(got.logits), P.bits(want)) and got.id == P.argmax(want)
            assert got.thr == -np.inf and got.kept == int(np.isfinite(want).sum())
    row, hist = Q.kernel_row(2049, 0), Q.kernel_history(2049, 31, 0)
    entries = Q.kernel_entries(2049, 255, [hist], 0)
    got = W.run_row(row, hist, W.Record(sequence_list=0), [entries], 0)
    assert np.array_equal(Q.bits(got.logits), Q.bits(Q.apply(row, hist, entries)))
    # and the order: the list first, the penalty on its result
    both = W.run_row(row, hist, W.Record(sequence_list=0, repetition_penalty=1.3, no_repeat_ngram_size=2), [entries], 0)
    assert np.array_equal(Q.bits(both.logits), Q.bits(P.apply(Q.apply(row, hist, entries), hist, 1.3, 2)))


def test_a_greedy_row_is_the_argmax_with_the_smaller_id():
    row = np.asarray([1.0, 5.0, -np.inf, 5.0, 0.0], np.float32)
    r = W.run_row(row, [], W.Record(), [], 3)
    assert (r.id, r.z, r.kept) == (1, 5.0, 4) and r.thr == -np.inf and np.isneginf(r.thr)
    assert abs(r.lp - float(R.log_softmax64(row)[1])) == 0.0


@pytest.mark.parametrize("V,rev", W.all_cases())
def test_kernel_cases_have_no_near_ties(V, rev):
    """Every sampled row of every kernel case is safe (sampling_filter_ref.draw_is_safe), so the GPU test demands exact ids; and the
    cases hold what they promise: the lists share a target with different biases, list 1 fires on its row's history and bans an id."""
    rows, hists, recs, lists = W.kernel_case(V, rev)
    res = W.run(rows, hists, recs, lists)
    assert [W.is_safe(r, c) for r, c in zip(res, recs)] == [True] * 6
    assert [len(h) for h in hists][:5] == [0, 1, 31, 32, 257] and len(hists[5]) == (W.LONG_T if V == 8225 else 40)
    assert sum(c.sampled for c in recs) == 4 and sum(c.filtered for c in recs) == 3 and sum(c.p_on for c in recs) == 2
    b0, b1 = dict(lists[0])[(W.SHARED,)], dict(lists[1])[(W.SHARED,)]
    assert b0 != b1
    s5, s6 = [c.sequence_list for c in recs].index(0), [c.sequence_list for c in recs].index(1)
    fired = [seq for seq, _ in lists[1] if seq[-1] == W.FIRED][0]
    assert Q.fires(fired, hists[s6]) and np.isneginf(res[s6].logits[W.BANNED]) and np.isfinite(res[s5].logits[W.BANNED])
    assert res[s6].logits[W.FIRED] != rows[s6][W.FIRED]
    for s, c in enumerate(recs):                                   # rows with nothing on keep their logits
        if c.sequence_list < 0 and c.repetition_penalty == 1.0:
            assert np.array_equal(Q.bits(res[s].logits), Q.bits(rows[s]))


# ---- Python ------------------------------------------------------------------------------------------------------------------
def test_check_row_options_refusals_name_the_row():
    ok = RowOptions()
    for bad, word in ((RowOptions(temperature=-1.0), "temperature"), (RowOptions(temperature=float("nan")), "temperature"),
                      (RowOptions(min_p=1.5), "min_p"), (RowOptions(seed=-1), "seed"), (RowOptions(top_k=-1), "top_k"),
                      (RowOptions(top_p=0.0), "top_p"), (RowOptions(repetition_penalty=0.0), "repetition_penalty"),
                      (RowOptions(no_repeat_ngram_size=33), "no_repeat_ngram_size"),
                      (RowOptions(sequence_bias=[((1, 2), 1.0), ((1, 2), 2.0)]), "repeats the sequence"),
                      (RowOptions(sequence_bias=[((999,), 1.0)]), "outside the vocabulary")):
        with pytest.raises(Q3aError, match="row 2") as e:
            check_row_options([ok, ok, bad], 100)
        assert word in str(e.value), (word, str(e.value))
    with pytest.raises(Q3aError, match="row 0 is not a RowOptions"):
        check_row_options([{"temperature": 1.0}], 100)


def test_equal_lists_share_an_index_and_indices_are_stable():
    a, b = [((1, 2), 1.0), ((3,), -np.inf)], {(4, 5): 2.0}
    rows = [RowOptions(sequence_bias=b), RowOptions(), RowOptions(sequence_bias=a), RowOptions(sequence_bias=list(b.items())),
            RowOptions(sequence_bias=[]), RowOptions(sequence_bias=a, temperature=0.5)]
    recs, lists = check_row_options(rows, 100)
    assert [r[7] for r in recs] == [0, -1, 1, 0, -1, 1]
    assert lists == [[((4, 5), 2.0)], [((1, 2), 1.0), ((3,), -np.inf)]]
    assert recs[5][:3] == (0.5, 0.0, 0) and recs[1] == (0.0, 0.0, 0, 0, 1.0, 1.0, 0, -1)
    # the same sequence in two lists is fine; more than 256 distinct lists is not
    check_row_options([RowOptions(sequence_bias=[((1,), 1.0)]), RowOptions(sequence_bias=[((1,), 2.0)])], 100)
    with pytest.raises(Q3aError, match="257 distinct"):
        check_row_options([RowOptions(sequence_bias=[((i % 90, i // 90), 1.0)]) for i in range(257)], 100)


# ---- the ABI's refusals, before a device is looked for -----------------------------------------------------------------------
def _call(lib, recs, lists, S=None, V=64, lens=None):
    S = len(recs) if S is None else S
    rows = np.zeros((S, V), np.float32)
    hl = np.zeros(S, np.int32) if lens is None else np.asarray(lens, np.int32)
    hist = np.zeros((S, 4), np.int32)
    table = (_lib.RowOptionsC * len(recs))()
    for c, r in zip(table, recs):
        (c.temperature, c.min_p, c.seed, c.top_k, c.top_p, c.repetition_penalty, c.no_repeat_ngram_size,
         c.sequence_list) = (r.temperature, r.min_p, r.seed, r.top_k, r.top_p, r.repetition_penalty, r.no_repeat_ngram_size, r.sequence_list)
    ids, ln, bias, ll = W.flatten_lists(lists)
    n = len(ln)
    rc = lib.q3a_selftest_row_options(0, rows.ctypes.data_as(f32p), S, V, hist.ctypes.data_as(i32p), 4, hl.ctypes.data_as(i32p), table,
                                      ids.ctypes.data_as(i32p) if n else None, ln.ctypes.data_as(i32p) if n else None,
                                      bias.ctypes.data_as(f32p) if n else None, ll.ctypes.data_as(i32p) if len(lists) else None, len(lists),
                                      None, None, None, None, None, None)
    return rc, (lib.q3a_last_error(None) or b"").decode()


def test_abi_refusals_name_the_row(lib):
    ok = W.Record()
    for bad, word in ((W.Record(temperature=-1.0), "temperature"), (W.Record(temperature=float("inf")), "temperature"),
                      (W.Record(min_p=-0.1), "min_p"), (W.Record(top_k=-3), "top_k"), (W.Record(top_p=1.5), "top_p"),
                      (W.Record(top_p=float("nan")), "top_p"), (W.Record(repetition_penalty=-2.0), "repetition_penalty"),
                      (W.Record(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (W.Record(no_repeat_ngram_size=33), "no_repeat_ngram_size"),
                      (W.Record(sequence_list=-2), "sequence_list"), (W.Record(sequence_list=1), "sequence_list")):
        rc, msg = _call(lib, [ok, bad, ok], [[((1,), 1.0)]])
        assert rc != 0 and "q3a_selftest_row_options: row 1: " in msg and word in msg, (bad, msg)
    rc, msg = _call(lib, [W.Record(sequence_list=0)], [])
    assert rc != 0 and "row 0" in msg and "outside [-1, 0)" in msg, msg


def test_abi_list_refusals(lib):
    one = [W.Record()]
    rc, msg = _call(lib, one, [[((1, 2), 1.0)], [((3,), 1.0), ((1, 2), 0.5), ((1, 2), 2.0)]])
    assert rc != 0 and "entry 3 repeats the sequence of an earlier entry" in msg, msg
    rc, msg = _call(lib, one, [[((1, 2), 1.0)], [((1, 2), 2.0)]])       # the same sequence in two lists: past the validation
    assert "repeats" not in msg and "sequence_list" not in msg and "more than" not in msg, msg
    rc, msg = _call(lib, one, [[((i % 60, i // 60), 1.0)] for i in range(257)], V=64)
    assert rc != 0 and "257 lists, more than 256" in msg, msg
    many = [[((i % 60, i // 60 % 60, i // 3600), 1.0) for i in range(k * 2049, (k + 1) * 2049)] for k in range(2)]
    rc, msg = _call(lib, one, many)
    assert rc != 0 and "4098 entries, more than 4096" in msg, msg
    long_ = [[(tuple((i + j) % 60 for j in range(31)) + (i // 60,), 1.0) for i in range(k * 1100, (k + 1) * 1100)] for k in range(2)]
    rc, msg = _call(lib, one, long_)
    assert rc != 0 and "more than 65536 ids over all entries" in msg, msg
    rc, msg = _call(lib, one, [[((1,), float("nan"))]])
    assert rc != 0 and "NaN or +inf" in msg, msg
    rc, msg = _call(lib, one, [], lens=[5])
    assert rc != 0 and "a history length outside [0, stride]" in msg, msg
