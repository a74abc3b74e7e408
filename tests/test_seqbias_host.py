"""Sequence bias without a GPU: the surfaces exist, the header states the contract, the refusals that need no device, the numpy
reference against HuggingFace's SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor bit for bit and against a naive loop, the
hotword and banned-phrase helpers on a small tokenizer, and the inputs the GPU kernel test relies on."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import seqbias_ref as R
from qwen3_asr_rs_amd.engine import Q3aError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUST = os.path.join(ROOT, "integration", "rust", "src", "backend", "hip")
INF = float("inf")


# ---- the surfaces exist ---------------------------------------------------------------------------------------------------
def test_symbols_in_header_binding_and_rust(lib):
    from qwen3_asr_rs_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "q3asr.h")).read()
    rust = open(os.path.join(RUST, "engine.rs")).read()
    cli = open(os.path.join(ROOT, "qwen3_asr_rs_amd", "csrc", "asr_main.cpp")).read()
    for sym in ("q3a_set_sequence_bias", "q3a_selftest_seqbias", "q3a_parse_sequence_bias", "q3a_hotword_sequences", "q3a_banned_sequences"):
        assert re.search(r"^int32_t %s\(" % sym, header, flags=re.M), sym
        assert sym in _lib.SYMBOLS, sym
        assert hasattr(lib, sym), f"libq3asr_hip.so does not export {sym}"
    for sym in ("q3a_set_sequence_bias", "q3a_selftest_seqbias"):
        assert re.search(r"pub fn %s\(" % sym, rust), sym
    assert re.search(r"pub fn set_sequence_bias\(&self, ", rust)
    for name in ("set_sequence_bias", "sequence_bias_stats"):
        assert callable(getattr(engine.HipEngine, name))
    for name in ("check_sequence_bias", "hotword_sequences", "banned_sequences", "parse_sequence_bias"):
        assert callable(getattr(engine, name))
    params = inspect.signature(engine.AsrInference.transcribe).parameters
    assert {"hotwords", "hotword_boost", "hotword_start_boost", "banned_phrases", "sequence_bias"} <= set(params)
    assert params["hotword_boost"].default is None and params["hotword_start_boost"].default == 0.0   # no tuned boost to default to
    assert "tuned on real weights" in engine.AsrInference.transcribe.__doc__
    for var in ("Q3A_SEQUENCE_BIAS", "Q3A_HOTWORDS", "Q3A_HOTWORD_BOOST", "Q3A_HOTWORD_START_BOOST", "Q3A_BANNED_PHRASES"):
        assert var in cli, var
    kernels = open(os.path.join(ROOT, "qwen3_asr_rs_amd", "csrc", "kernels.h")).read()
    assert "struct SeqBiasArgs" in kernels and "launch_seqbias_apply(" in kernels


def test_rust_ffi_is_what_the_generator_writes():
    """tools/gen_rust_ffi.py regenerates ffi.rs from include/q3asr_ops.h; the committed file is its output and binds no engine call."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_rust_ffi", os.path.join(ROOT, "tools", "gen_rust_ffi.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ops = re.sub(r"/\*.*?\*/", "", open(gen.HDR).read(), flags=re.S)
    want = set(re.findall(r"^\s*(?:const char\*|int32_t|int64_t|void)\s+(q3a_[a-z0-9_]+)\s*\(", ops, flags=re.M))
    bound = set(re.findall(r"pub fn (q3a_[a-z0-9_]+)\s*\(", open(os.path.join(RUST, "ffi.rs")).read()))
    assert bound == want and "q3a_set_sequence_bias" not in bound


def test_header_states_the_contract():
    header = " ".join(open(os.path.join(ROOT, "include", "q3asr.h")).read().replace(" * ", " ").split())
    sec = header[header.index("---- sequence bias:"):header.index("int32_t q3a_selftest_seqbias(")]
    for phrase in (  # history, firing rule, sum
                   "The prompt is not history", "q3a_set_next_tokens is not history",
                   "fires on a row iff t >= L - 1 and h[t - L + 1 .. t) equals q_0 .. q_{L-2}", "A one-token entry always fires, also at t = 0",
                   "acc = 0.0f", "in the order the caller gave them", "one more fp32 add", "Ids that no entry fired on are not touched",
                   "-inf stays -inf and never yields NaN",
                   # the pin
                   "SequenceBiasLogitsProcessor", "input_ids = [x] ++ h", "len(sequence) > context quirk", "NoBadWordsLogitsProcessor",
                   "a logit of -0.0 that nothing fired on stays -0.0",
                   # the order of the processors
                   "logit bias (inside the head), sequence bias, repetition penalty, n-gram ban, then argmax or sampler",
                   "a -inf is invariant under the penalty and the ban",
                   # downstream, on / off, state
                   "q3a_fetch_logprobs = log_softmax(l'')[id]", 'the "logits" tap hold l\'\'', "An empty list (n = 0) is off",
                   "the one-sequence pruned argmax is not taken", "another list replays the same graph",
                   "allocated at the first non-empty set and freed with the engine",
                   "q3a_score* and q3a_align* never see it",
                   # limits and every refusal
                   "E <= 4096; L <= 32; at most 65536 ids over all entries",
                   "an id < 0 or >= vocab", "an empty sequence, or L > 32", "more entries or ids than the limits", "the same sequence twice",
                   "a NaN or +inf bias", "an aligner engine", "q3a_beam_begin / q3a_beam_search_batch_ptrs while it is on",
                   "q3a_prefill_draft / q3a_transcribe_draft_batch_ptrs while it is on",
                   "a -inf entry together with an allow-list logit bias", "the distinct targets of -inf entries plus, with an n-gram ban on, max_new_tokens",
                   "comes second",
                   'q3a_debug_read(e, "sequence_bias", ..) (int32 [4]',
                   # out of scope
                   "per-utterance lists inside one batch", "subtracting a partial boost when a phrase is abandoned",
                   "sequence bias inside beam search or under a draft (so not in StreamingTranscriber)", "matching over the prompt",
                   "boost values tuned on real weights"):
        assert phrase in sec, phrase
    # the logit-bias section points here and keeps its own sentence
    bias = header[header.index("Out of scope: per-utterance biases"):header.index("int32_t q3a_set_logit_bias(")]
    assert "multi-token phrase constraints" in bias and "multi-token sequences: their own section below" in bias


# ---- refusals that need no device -----------------------------------------------------------------------------------------
def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))


def test_check_sequence_bias():
    from qwen3_asr_rs_amd.engine import check_sequence_bias
    ids, lens, bias = check_sequence_bias([((5, 6, 7), 2.5), ([9], -INF), ((np.int32(5), 6), 0.0)], 10)
    assert ids.tolist() == [5, 6, 7, 9, 5, 6] and lens.tolist() == [3, 1, 2] and bias.tolist() == [2.5, -INF, 0.0]
    assert ids.dtype == np.int32 and lens.dtype == np.int32 and bias.dtype == np.float32
    ids, lens, bias = check_sequence_bias({(1, 2): 1.0, (3,): -1.0}, 10)            # a mapping, in its own order
    assert ids.tolist() == [1, 2, 3] and lens.tolist() == [2, 1]
    for empty in (None, [], {}):
        assert [len(x) for x in check_sequence_bias(empty, 10)] == [0, 0, 0]
    assert len(check_sequence_bias([(tuple(range(32)), 1.0)], 100)[0]) == 32
    for entries, msg in [([((10,), 1.0)], "outside the vocabulary"), ([((-1,), 1.0)], "outside the vocabulary"),
                         ([((), 1.0)], "0 ids"), ([(tuple(range(33)), 1.0)], "33 ids"),
                         ([((1, 2), 1.0), ((1, 2), 2.0)], "repeats the sequence"), ([((1,), float("nan"))], "NaN or \\+inf"),
                         ([((1,), INF)], "NaN or \\+inf"), ([((1.5,), 1.0)], "not an integer"), ([((True,), 1.0)], "not an integer"),
                         ([((1,), "big")], "must be a number"), ([5], "must be \\(ids, bias\\)"),
                         ([((i // 9, i % 9), 1.0) for i in range(4097)], "4097 entries"),
                         ([(tuple([i % 7] + [i // 7 % 7] + [i // 49] + [0] * 29), 1.0) for i in range(2049)], "65568 ids")]:
        with pytest.raises(Q3aError, match=msg):
            check_sequence_bias(entries, 4097 if len(entries) > 100 else 10)


def test_c_entry_points_refuse_before_a_device(lib):
    assert lib.q3a_set_sequence_bias(None, None, None, None, 0) != 0                # a null engine
    x, h, one = np.zeros(4, np.float32), np.zeros(4, np.int32), np.array([1], np.int32)

    def selftest(seq_ids, seq_lens, seq_bias, V=4, lens=one, S=1):
        n = len(seq_lens)
        return lib.q3a_selftest_seqbias(0, _f32(x), S, V, _i32(h), 4, _i32(lens), _i32(seq_ids) if n else None, _i32(seq_lens) if n else None,
                                        _f32(seq_bias) if n else None, n, None, None, None)

    for args, kw, msg in [(([4], [1], [1.0]), {}, b"outside the vocabulary"), (([-1], [1], [1.0]), {}, b"outside the vocabulary"),
                          (([1], [0], [1.0]), {}, b"empty sequence"), (([1] * 33, [33], [1.0]), {}, b"more than 32"),
                          (([1, 2, 1, 2], [2, 2], [1.0, 2.0]), {}, b"repeats the sequence"), (([1], [1], [float("nan")]), {}, b"NaN or +inf"),
                          (([1], [1], [INF]), {}, b"NaN or +inf"), (([1], [1], [1.0]), {"V": 0}, b"bad argument"),
                          (([1], [1], [1.0]), {"S": 0}, b"bad argument"), (([1], [1], [1.0]), {"lens": np.array([5], np.int32)}, b"history length"),
                          (([1], [1], [1.0]), {"lens": np.array([-1], np.int32)}, b"history length"),
                          (([i % 3 for i in range(4097 * 2)], [2] * 4097, [1.0] * 4097), {}, b"4097 entries"),
                          (([(i >> (2 * k)) & 3 for i in range(2049) for k in range(32)], [32] * 2049, [1.0] * 2049), {}, b"65536 ids")]:
        assert selftest(*args, **kw) != 0
        assert msg in lib.q3a_last_error(None), (msg, lib.q3a_last_error(None))
    h[0] = 4                                                                         # a history id outside the vocabulary
    assert selftest([1], [1], [1.0]) != 0 and b"history id outside the vocabulary" in lib.q3a_last_error(None)


def test_parse_sequence_bias(lib):
    from qwen3_asr_rs_amd.engine import parse_sequence_bias
    text = "# names\n2.5 10 11 12   # a three-token phrase\n\n-inf 7\n  -INF 8 9\n0 1 2\n1e-3\t3\t4\n"
    assert parse_sequence_bias(text) == [((10, 11, 12), 2.5), ((7,), -INF), ((8, 9), -INF), ((1, 2), 0.0), ((3, 4), float(np.float32(1e-3)))]
    assert parse_sequence_bias("") == [] and parse_sequence_bias("# nothing\n\n") == []
    assert len(parse_sequence_bias("1.0 " + " ".join(str(i) for i in range(32)))[0][0]) == 32
    for bad, msg in [("2.5", "expected"), ("2.5 x", "not an id"), ("2.5 -3", "not an id"), ("2.5 1.5", "not an id"), ("inf 3", "not a finite bias"),
                     ("nan 3", "not a finite bias"), ("+inf 3", "not a finite bias"), ("abc 3", "not a finite bias"),
                     ("1.0 1 2\n2.0 1 2", "earlier line"), ("1.0 " + " ".join(["1"] * 33), "more than 32"), ("1.0 99999999999", "not an id")]:
        with pytest.raises(Q3aError, match=msg):
            parse_sequence_bias(bad)
    with pytest.raises(Q3aError, match="line 3"):
        parse_sequence_bias("1.0 1\n# fine\n2.0 oops\n")
    n_ids, n = C.c_int32(), C.c_int32()
    assert lib.q3a_parse_sequence_bias(b"1 2 3", None, 0, None, None, 0, None, None) != 0 and b"bad argument" in lib.q3a_last_error(None)
    assert lib.q3a_parse_sequence_bias(b"1 2 3\n-inf 4", None, 0, None, None, 0, C.byref(n_ids), C.byref(n)) == 0
    assert (n_ids.value, n.value) == (3, 2)


# ---- the reference --------------------------------------------------------------------------------------------------------
GRID = [(V, t) for V in (1, 31, 33, 100) for t in (0, 1, 2, 3, 7, 40)]


def _grid_case(rng, V, t, all_inf=False):
    """A row with a -inf and a 0.0, a history over a small alphabet, and entries of L = 1, 2, 3 and 5: several on one target, with
    overlapping matches (prefixes cut from the history's own tail and from earlier stretches of it), finite and -inf biases."""
    hist = rng.integers(0, min(V, 3), t).tolist()
    l = (rng.standard_normal(V) * 5).astype(np.float32)
    if V > 2:
        l[1] = -np.inf
        l[2] = 0.0
    entries = {}
    for L in (1, 2, 3, 5, 2, 3, 1, 5, 3):
        for kind in range(3):
            if kind == 0 and t >= L - 1:
                pre = hist[t - L + 1:]                                   # fires
            elif kind == 1 and t >= L:
                pre = hist[t - L:t - 1]                                  # the stretch one step earlier: fires only if it recurs
            else:
                pre = rng.integers(0, min(V, 3), L - 1).tolist()
            seq = tuple(pre) + (int(rng.integers(0, min(V, 4))),)        # few targets: several entries share one
            b = -np.inf if (all_inf or rng.random() < 0.3) else float(np.float32(rng.standard_normal() * 4))
            entries.setdefault(seq, b)
    return l, hist, list(entries.items())


def _hf_input(hist, x=0):
    import torch
    return torch.tensor([[x] + list(hist)], dtype=torch.long)


def test_reference_equals_sequence_bias_logits_processor_bit_for_bit():
    """SequenceBiasLogitsProcessor(sequence_bias = the entries as a dict in the caller's order) on input_ids = [x] ++ h.  The rows
    hold no -0.0 (the contract's one exception)."""
    pytest.importorskip("transformers")
    import torch
    from transformers import SequenceBiasLogitsProcessor
    rng = np.random.default_rng(0)
    fired_some, missed_some, shared = 0, 0, 0
    for V, t in GRID:
        for rep in range(3):
            l, hist, entries = _grid_case(rng, V, t)
            mine = R.apply(l, hist, entries)
            proc = SequenceBiasLogitsProcessor(sequence_bias={tuple(s): float(b) for s, b in entries})
            want = proc(_hf_input(hist, x=rep % V), torch.tensor(l)[None].clone())[0].numpy()
            assert np.array_equal(R.bits(mine), R.bits(want)), (V, t, hist, entries)
            assert not np.isnan(mine).any()
            f = [R.fires(s, hist) for s, _ in entries]
            fired_some += any(f)
            missed_some += not all(f)
            tg = [s[-1] for (s, _), ok in zip(entries, f) if ok]
            shared += len(tg) != len(set(tg))
    assert fired_some == 3 * len(GRID) and missed_some >= len(GRID) and shared >= len(GRID)   # the grid bites
    assert len(GRID) == 24


def test_reference_with_minus_inf_equals_no_bad_words_logits_processor():
    pytest.importorskip("transformers")
    import torch
    from transformers import NoBadWordsLogitsProcessor
    rng = np.random.default_rng(2)
    for V, t in GRID:
        l, hist, entries = _grid_case(rng, V, t, all_inf=True)
        mine = R.apply(l, hist, entries)
        proc = NoBadWordsLogitsProcessor(bad_words_ids=[list(s) for s, _ in entries])
        want = proc(_hf_input(hist), torch.tensor(l)[None].clone())[0].numpy()
        assert np.array_equal(R.bits(mine), R.bits(want)), (V, t, hist, entries)
        banned = {s[-1] for s, _ in entries if R.fires(s, hist)}
        assert banned and all(np.isneginf(mine[v]) for v in banned) and not np.isnan(mine).any()


def test_reference_equals_the_naive_loops():
    rng = np.random.default_rng(1)
    for V, t in GRID:
        for _ in range(2):
            l, hist, entries = _grid_case(rng, V, t)
            assert np.array_equal(R.bits(R.apply(l, hist, entries)), R.bits(R.apply_naive(l, hist, entries))), (V, t, hist, entries)
    for S, rows, hists, entries in R.kernel_cases(33)[:4]:                          # and on kernel inputs (E = 1 and 255)
        for r, h in zip(rows, hists):
            assert np.array_equal(R.bits(R.apply(r, h, entries)), R.bits(R.apply_naive(r, h, entries)))


def test_reference_edge_rules():
    f = np.float32
    row = np.array([2.0, -3.0, 0.0, -np.inf, 1.5, 4.0], np.float32)
    # t = L - 1 fires (HuggingFace on input_ids = h alone would ignore it: the sequence is "longer than the context"); t = L - 2 does not
    e3 = [((0, 1, 4), 2.0)]
    assert R.apply(row, [0, 1], e3)[4] == f(3.5) and R.fires((0, 1, 4), [0, 1])
    assert np.array_equal(R.bits(R.apply(row, [1], e3)), R.bits(row)) and not R.fires((0, 1, 4), [1])
    assert np.array_equal(R.bits(R.apply(row, [], e3)), R.bits(row))
    assert R.apply(row, [5, 0, 1], e3)[4] == f(3.5) and np.array_equal(R.bits(R.apply(row, [0, 1, 5], e3)), R.bits(row))
    # a one-token entry always fires, at t = 0 too
    assert R.apply(row, [], [((5,), -1.0)])[5] == f(3.0) and R.apply(row, [1, 2, 3], [((5,), -1.0)])[5] == f(3.0)
    # the order of the additions is visible: the one-token entry first wherever the caller put it, then the caller's order
    a, b, c = ((4,), 1e8), ((1, 4), 1.0), ((0, 1, 4), -1e8)
    assert R.apply(row, [0, 1], [a, b, c])[4] == f(1.5)                    # ((0 + 1e8) + 1) - 1e8 = 0
    assert R.apply(row, [0, 1], [b, c, a])[4] == f(1.5)                    # the one-token entry still goes first
    assert R.apply(row, [0, 1], [a, c, b])[4] == f(2.5)                    # ((0 + 1e8) - 1e8) + 1 = 1
    assert R.apply(row, [0, 1], [c, b, a])[4] == f(2.5)
    # acc is summed first, then added once: (1.5 + 1e8) - 1e8 would be 0
    assert R.apply(row, [0, 1], [((1, 4), 1e8), ((0, 1, 4), -1e8)])[4] == f(1.5)
    # -inf stays -inf, with a finite and with a -inf bias, and a -inf bias wins over any finite one on the same target; never NaN
    assert np.isneginf(R.apply(row, [], [((3,), 5.0)])[3]) and np.isneginf(R.apply(row, [], [((3,), -np.inf)])[3])
    out = R.apply(row, [0], [((5,), 3.0), ((0, 5), -np.inf)])
    assert np.isneginf(out[5]) and not np.isnan(out).any()
    # untouched ids keep their bits, a -0.0 included
    z = np.array([-0.0, 1.0], np.float32)
    assert np.array_equal(R.bits(R.apply(z, [], [((1,), 1.0)])), R.bits(np.array([-0.0, 2.0], np.float32)))
    assert R.argmax(np.array([1.0, 3.0, 3.0], np.float32)) == 1


# ---- hotwords and banned phrases ------------------------------------------------------------------------------------------
@pytest.fixture()
def small_tokenizer(lib, tmp_path):
    """Byte-level BPE over a, b, c and the space: "abc" -> [ab, c], " abc" -> [G, ab, c] (G = the space's byte symbol)."""
    from qwen3_asr_rs_amd.audio import AsrTokenizer
    vocab = {"a": 0, "b": 1, "c": 2, "Ġ": 3, "ab": 4, "Ġc": 5}
    tok = {"version": "1.0", "added_tokens": [], "model": {"type": "BPE", "vocab": vocab, "merges": ["a b", "Ġ c"]}}
    p = tmp_path / "tokenizer.json"
    p.write_text(json.dumps(tok))
    return AsrTokenizer(str(p))


class _Duck:
    """Any object with encode(text): hotword_sequences then applies the rule in Python instead of calling the C helper."""
    def __init__(self, tok):
        self.tok = tok

    def encode(self, text):
        return self.tok.encode(text)


def test_hotword_sequences(small_tokenizer):
    from qwen3_asr_rs_amd.engine import banned_sequences, check_sequence_bias, hotword_sequences
    t = small_tokenizer
    assert t.encode("abc") == [4, 2] and t.encode(" abc") == [3, 4, 2] and t.encode("ab c") == [4, 5]
    got = hotword_sequences(t, ["abc"], 2.0)
    # both tokenisations, every prefix of two ids and more, no one-token entry without a start boost
    assert got == [((4, 2), 2.0), ((3, 4), 2.0), ((3, 4, 2), 2.0)]
    got = hotword_sequences(t, ["abc"], 2.0, 0.5)
    assert got == [((4,), 0.5), ((4, 2), 2.0), ((3,), 0.5), ((3, 4), 2.0), ((3, 4, 2), 2.0)]
    # equal sequences are merged and keep the larger bias: "ab" and "abc" share (3, 4); "ab" alone is one token, boosted by start_boost only
    got = dict(hotword_sequences(t, ["abc", "ab", "ab c"], 2.0, 3.0))
    assert got == {(4,): 3.0, (4, 2): 2.0, (3,): 3.0, (3, 4): 2.0, (3, 4, 2): 2.0, (4, 5): 2.0, (3, 4, 5): 2.0}
    assert dict(hotword_sequences(t, ["ab"], 2.0)) == {(3, 4): 2.0}
    assert dict(hotword_sequences(t, ["abc"], -1.0, -4.0))[(4,)] == -4.0
    got = hotword_sequences(t, ["cc", "c c"], 1.0, 2.0)                  # (2,) from both phrases once; (3, 2) / (3, 2, 5) prefixes
    assert len(got) == len(dict(got)) and dict(got)[(2,)] == 2.0
    check_sequence_bias(got, 6)
    for phrases, boosts in [(["abc", "ab c", "cab"], (2.0, 0.0)), (["abc", "ab"], (1.5, 0.25)), ("abc", (1.0, 0.0))]:
        assert hotword_sequences(_Duck(t), phrases, *boosts) == hotword_sequences(t, phrases, *boosts)   # the C helper and the Python rule
    assert banned_sequences(t, ["abc", "ab"]) == [((4, 2), -INF), ((3, 4, 2), -INF), ((4,), -INF), ((3, 4), -INF)]
    assert banned_sequences(_Duck(t), ["abc", "ab"]) == banned_sequences(t, ["abc", "ab"])
    long = "c" * 33
    for tok in (t, _Duck(t)):
        with pytest.raises(Q3aError, match="phrase '%s' encodes to 33 ids" % long):
            hotword_sequences(tok, ["abc", long], 1.0)
        assert len(hotword_sequences(tok, ["c" * 32], 1.0)) == 31 + 31     # 32 ids in both tokenisations: the limit itself fits
        with pytest.raises(Q3aError, match="empty phrase"):
            hotword_sequences(tok, ["  "], 1.0)
        with pytest.raises(Q3aError, match="finite"):
            hotword_sequences(tok, ["abc"], INF)
        with pytest.raises(Q3aError, match="33 ids"):
            banned_sequences(tok, [long])


# ---- the kernel test's inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", list(R.KERNEL_V) + [R.BIG_V])
def test_kernel_inputs_cover_what_the_gpu_test_claims(V):
    """What tests/test_gpu_seqbias.py relies on: S = 1 and 3 with lengths that differ, every history length of KERNEL_T under every
    list size, entries of 1, 2, 31 and 32 ids that fire, at least one firing and one non-firing entry per call (a list of ONE entry:
    over the calls of that list size), two entries on one target that both fire, the visible order of additions, -inf biases, more
    than 256 and exactly 4096 target groups, lists inside the limits, and a row whose argmax the bias moves."""
    from qwen3_asr_rs_amd.engine import check_sequence_bias
    cases = R.kernel_cases(V)
    assert {c[0] for c in cases} == ({3} if V == R.BIG_V else {1, 3})
    by_E, fired_L, groups_seen, shared, moved, inf_bias, order_seen = {}, set(), set(), False, False, False, False
    for S, rows, hists, entries in cases:
        assert rows.shape == (S, V) and rows.dtype == np.float32 and len(hists) == S and not np.isnan(rows).any()
        check_sequence_bias(entries, V)                                  # distinct, inside the vocabulary and the limits
        if S == 3:
            assert len({len(h) for h in hists}) == 3
        E = len(entries)
        groups_seen.add(len({s[-1] for s, _ in entries}))
        if V == R.BIG_V or (V != 1 and dict(R.KERNEL_E[V])[E]):
            assert len({s[-1] for s, _ in entries}) == E                 # every entry on a target of its own: E groups
        rec = by_E.setdefault(E, {"t": set(), "fire": False, "miss": False})
        call_fire = call_miss = False
        for r, h in zip(rows, hists):
            assert all(0 <= x < V for x in h)
            rec["t"].add(len(h))
            f = [R.fires(s, h) for s, _ in entries]
            call_fire, call_miss = call_fire or any(f), call_miss or not all(f)
            fired_L |= {len(s) for (s, _), ok in zip(entries, f) if ok}
            tg = [s[-1] for (s, _), ok in zip(entries, f) if ok]
            shared = shared or len(tg) != len(set(tg))
            inf_bias = inf_bias or any(ok and b == -np.inf for (_, b), ok in zip(entries, f))
            out = R.apply(r, h, entries)
            assert not np.isnan(out).any()
            moved = moved or R.argmax(out) != R.argmax(r)
            order = [b for (s, b), ok in zip(entries, f) if ok and s[-1] == 5 and b in R.ORDER_BIASES]
            order_seen = order_seen or sorted(order) == sorted(R.ORDER_BIASES)
        rec["fire"], rec["miss"] = rec["fire"] or call_fire, rec["miss"] or call_miss
        if E > 1:   # (a one-id vocabulary's entries are runs of id 0: once the history is as long as the longest, none can miss)
            assert call_fire and (call_miss or (V == 1 and min(len(h) for h in hists) >= E - 1)), (V, E, [len(h) for h in hists])
    if V == R.BIG_V:
        assert set(by_E) == {4096} and by_E[4096]["t"] == {1023, 32, 0}
    else:
        assert set(by_E) == {E for E, _ in R.KERNEL_E[V]}
        for E, rec in by_E.items():
            assert rec["t"] == set(R.KERNEL_T) and rec["fire"] and rec["miss"], (V, E)
    assert set(R.KERNEL_T) == {0, 1, 31, 32, 257, 1023} | {L - 2 for L in R.KERNEL_L if L >= 2} | {L - 1 for L in R.KERNEL_L} | set(R.KERNEL_L)
    if V == 1:
        assert fired_L == set(range(1, 33)) and shared
    else:
        assert set(R.KERNEL_L) <= fired_L
    if V > 8:
        assert moved and inf_bias and (V == R.BIG_V or (shared and order_seen))
    if V == 2049:
        assert {255, 256, 257} <= groups_seen and max(groups_seen) > 257   # E = G around the 256-thread stride, and several groups per thread
    if V in (8225, R.BIG_V):
        assert 4096 in groups_seen                                       # the capacity: 16 groups per thread
