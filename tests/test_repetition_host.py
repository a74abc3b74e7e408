"""Repetition control without a GPU: the surfaces exist, the refusals that need no device, the numpy reference against HuggingFace's
two processors bit for bit and against a naive triple loop, and the inputs the GPU kernel test relies on."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import repetition_ref as R
from qwen3_asr_rs_amd.engine import Q3aError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUST = os.path.join(ROOT, "integration", "rust", "src", "backend", "hip")


# ---- the surfaces exist ---------------------------------------------------------------------------------------------------
def test_symbols_in_header_binding_and_rust(lib):
    from qwen3_asr_rs_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "q3asr.h")).read()
    # the engine-level Rust declarations live in engine.rs; ffi.rs is generated from the op-level header q3asr_ops.h only
    # (tests/test_ops_veneer.py holds that it binds exactly those names), so it must come out of the generator unchanged
    rust = open(os.path.join(RUST, "engine.rs")).read()
    cli = open(os.path.join(ROOT, "qwen3_asr_rs_amd", "csrc", "asr_main.cpp")).read()
    for sym in ("q3a_set_repetition", "q3a_selftest_repeat"):
        assert re.search(r"^int32_t %s\(" % sym, header, flags=re.M), sym
        assert sym in _lib.SYMBOLS and re.search(r"pub fn %s\(" % sym, rust), sym
        assert hasattr(lib, sym), f"libq3asr_hip.so does not export {sym}"
    assert re.search(r"pub fn set_repetition\(&self, repetition_penalty: f32, no_repeat_ngram_size: usize\)", rust)
    for name in ("set_repetition", "repetition_stats"):
        assert callable(getattr(engine.HipEngine, name))
    assert callable(engine.check_repetition_args)
    assert {"repetition_penalty", "no_repeat_ngram_size"} <= set(inspect.signature(engine.AsrInference.transcribe).parameters)
    assert "Q3A_REPETITION_PENALTY" in cli and "Q3A_NO_REPEAT_NGRAM" in cli


def test_header_states_the_contract():
    header = " ".join(open(os.path.join(ROOT, "include", "q3asr.h")).read().replace(" * ", " ").split())
    sec = header[header.index("---- repetition:"):header.index("int32_t q3a_selftest_repeat(")]
    for phrase in ("The prompt (audio pads and a chat template) is not history", "q3a_set_next_tokens is not history",
                   "penalised once", "-inf stays -inf and 0 stays 0", "The ban is applied after the penalty and wins",
                   "RepetitionPenaltyLogitsProcessor followed by NoRepeatNGramLogitsProcessor",
                   "repetition_penalty == 1 and no_repeat_ngram_size == 0 is off",
                   # the refusals
                   "not finite or <= 0", "no_repeat_ngram_size < 0 or > 32", "an aligner engine",
                   "q3a_beam_begin / q3a_beam_search_batch_ptrs while it is on", "262144 ids", "151936 fits",
                   "leaves both EOS ids at -inf and no more finite entries than max_new_tokens", "comes second",
                   # bit-identical bystanders, the readable state
                   "q3a_score* and q3a_align* never see it", 'q3a_debug_read(e, "repetition", ..) (uint32 [3]',
                   # out of scope
                   "penalties over the prompt", "frequency / presence penalties", "a history window",
                   "repetition control inside beam search", "keeping the one-sequence pruned argmax under it"):
        assert phrase in sec, phrase
    # the logit-bias section no longer calls the two processors out of scope
    bias = header[header.index("Out of scope: per-utterance biases"):header.index("int32_t q3a_set_logit_bias(")]
    assert "their own sections below" in bias and "processors (no-repeat n-gram, repetition penalty);" not in bias


def test_rust_ffi_is_what_the_generator_writes():
    """tools/gen_rust_ffi.py regenerates ffi.rs from include/q3asr_ops.h; the committed file is its output."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_rust_ffi", os.path.join(ROOT, "tools", "gen_rust_ffi.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ops = re.sub(r"/\*.*?\*/", "", open(gen.HDR).read(), flags=re.S)
    want = set(re.findall(r"^\s*(?:const char\*|int32_t|int64_t|void)\s+(q3a_[a-z0-9_]+)\s*\(", ops, flags=re.M))
    bound = set(re.findall(r"pub fn (q3a_[a-z0-9_]+)\s*\(", open(os.path.join(RUST, "ffi.rs")).read()))
    assert bound == want and "q3a_set_repetition" not in bound


# ---- refusals that need no device -----------------------------------------------------------------------------------------
def test_refusals_that_need_no_device(lib):
    from qwen3_asr_rs_amd.engine import check_repetition_args
    assert check_repetition_args() == (1.0, 0) and check_repetition_args(1.3, 3) == (1.3, 3)
    assert check_repetition_args(0.8, np.int32(32)) == (0.8, 32)
    for args, msg in [((0.0,), "repetition_penalty"), ((-1.3,), "repetition_penalty"), ((float("nan"),), "repetition_penalty"),
                      ((float("inf"),), "repetition_penalty"), (("strong",), "number"),
                      ((1.0, -1), "no_repeat_ngram_size"), ((1.0, 33), "no_repeat_ngram_size"), ((1.0, 2.0), "no_repeat_ngram_size"),
                      ((1.0, True), "no_repeat_ngram_size")]:
        with pytest.raises(Q3aError, match=msg):
            check_repetition_args(*args)
    # the C entry points: a null engine, and the selftest's arguments before it looks for a device
    assert lib.q3a_set_repetition(None, C.c_float(1.3), 2) != 0
    x = np.zeros(4, dtype=np.float32)
    h = np.zeros(4, dtype=np.int32)
    xp, hp = x.ctypes.data_as(C.POINTER(C.c_float)), h.ctypes.data_as(C.POINTER(C.c_int32))
    one, five, neg = (np.array([v], np.int32) for v in (1, 5, -1))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    for p, n, V, lens, msg in [(0.0, 0, 4, one, b"repetition_penalty"), (float("nan"), 0, 4, one, b"repetition_penalty"),
                               (float("inf"), 0, 4, one, b"repetition_penalty"), (1.0, -1, 4, one, b"no_repeat_ngram_size"),
                               (1.0, 33, 4, one, b"no_repeat_ngram_size"), (1.0, 0, 0, one, b"bad argument"),
                               (1.0, 0, (1 << 18) + 1, one, b"bitmap"), (1.0, 0, 4, five, b"history length"),
                               (1.0, 0, 4, neg, b"history length")]:
        assert lib.q3a_selftest_repeat(0, xp, 1, V, hp, 4, ip(lens), C.c_float(p), n, None, None, None) != 0
        assert msg in lib.q3a_last_error(None), (p, n, V, lib.q3a_last_error(None))
    h[0] = 4                                                             # an id outside the vocabulary
    assert lib.q3a_selftest_repeat(0, xp, 1, 4, hp, 4, ip(one), C.c_float(1.0), 0, None, None, None) != 0
    assert b"outside the vocabulary" in lib.q3a_last_error(None)


# ---- the reference --------------------------------------------------------------------------------------------------------
GRID = [(V, t, n, p) for V in (1, 31, 33, 100) for t in (0, 1, 2, 3, 7, 40) for n in (0, 1, 2, 3, 5) for p in (1.0, 1.3, 0.8)]


def _grid_case(rng, V, t):
    hist = rng.integers(0, min(V, 4), t).tolist()
    l = (rng.standard_normal(V) * 5).astype(np.float32)
    if V > 2:
        l[1] = -np.inf
        l[2] = 0.0
    return l, hist


def test_reference_equals_the_transformers_processors_bit_for_bit():
    """RepetitionPenaltyLogitsProcessor followed by NoRepeatNGramLogitsProcessor on input_ids = h; t = 0 compares against the identity
    (the processors need at least one input id)."""
    pytest.importorskip("transformers")
    import torch
    from transformers import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor
    rng = np.random.default_rng(0)
    for V, t, n, p in GRID:
        l, hist = _grid_case(rng, V, t)
        mine = R.apply(l, hist, p, n)
        if t == 0:
            want = l.copy()
        else:
            ids, s = torch.tensor([hist], dtype=torch.long), torch.tensor(l)[None].clone()
            if p != 1.0:
                s = RepetitionPenaltyLogitsProcessor(p)(ids, s)
            if n > 0:
                s = NoRepeatNGramLogitsProcessor(n)(ids, s)
            want = s[0].numpy()
        assert np.array_equal(R.bits(mine), R.bits(want)), (V, t, n, p, hist)
    assert len(GRID) == 360


def test_reference_equals_a_naive_triple_loop():
    rng = np.random.default_rng(1)
    for V, t, n, p in GRID:
        l, hist = _grid_case(rng, V, t)
        assert np.array_equal(R.bits(R.apply(l, hist, p, n)), R.bits(R.apply_naive(l, hist, p, n))), (V, t, n, p, hist)
    a, b = 0, 1
    row = np.array([2.0, -3.0, 0.0, -np.inf, 1.5], np.float32)
    for hist in ([a] * 4, [a, b] * 2, [a, b, a], [a, a, b, a, a], [a, b, a, b, a]):        # overlapping histories: aaaa, abab, ...
        for n in (0, 1, 2, 3, 4, 5):
            for p in (1.0, 1.3, 0.8):
                assert np.array_equal(R.bits(R.apply(row, hist, p, n)), R.bits(R.apply_naive(row, hist, p, n))), (hist, n, p)


def test_reference_edge_rules():
    inf = np.inf
    row = np.array([2.0, -3.0, 0.0, -inf, 1.5, 4.0], np.float32)
    f = np.float32
    # penalised once however often an id occurred; positive divided, negative multiplied, 0 and -inf unchanged
    out = R.apply(row, [0, 0, 0, 1, 2, 3], 1.3, 0)
    assert out[0] == f(2.0) / f(1.3) and out[1] == f(-3.0) * f(1.3) and out[2] == 0 and out[3] == -inf and out[4] == f(1.5)
    assert R.apply(row, [0] * 7, 0.8, 0)[0] == f(2.0) / f(0.8)            # p < 1 rewards
    # aaaa with n = 2: a is banned; abab with n = 2: the tail is b, b was followed by a; with n = 3: tail ab was followed by a
    assert R.apply(row, [0, 0, 0, 0], 1.0, 2)[0] == -inf
    assert np.nonzero(np.isneginf(R.apply(row, [0, 1, 0, 1], 1.0, 2)))[0].tolist() == [0, 3]
    assert np.nonzero(np.isneginf(R.apply(row, [0, 1, 0, 1], 1.0, 3)))[0].tolist() == [0, 3]
    assert np.nonzero(np.isneginf(R.apply(row, [0, 1, 0, 4], 1.0, 3)))[0].tolist() == [3]   # tail (0, 4) never seen before
    # n = 1 bans every id already emitted; the ban wins over the penalty
    assert np.nonzero(np.isneginf(R.apply(row, [5, 0], 1.3, 1)))[0].tolist() == [0, 3, 5]
    # t < n - 1: no ban, the penalty alone; t = 0: the identity
    assert np.array_equal(R.bits(R.apply(row, [0, 1], 1.3, 5)), R.bits(R.apply(row, [0, 1], 1.3, 0)))
    assert np.array_equal(R.bits(R.apply(row, [], 1.3, 1)), R.bits(row))
    # t = n - 1: the tail is the whole history and nothing precedes it
    assert np.array_equal(R.bits(R.apply(row, [0, 1], 1.0, 3)), R.bits(row))
    assert R.argmax(np.array([1.0, 3.0, 3.0], np.float32)) == 1


@pytest.mark.parametrize("V", list(R.KERNEL_V) + [R.BIG_V])
def test_kernel_inputs_cover_what_the_gpu_test_claims(V):
    """What tests/test_gpu_repetition.py relies on: S = 1 and 3 with lengths that differ, every (n, p), every length of the contract's
    list, ids 0 and V - 1, an id repeated 200 times, a banned id, seen ids with positive, negative, zero and -inf logits, values in
    the normal fp32 range, and a unique maximum of l'' (so the id does not hang on the tie rule alone)."""
    cases = R.kernel_cases(V)
    if V == R.BIG_V:
        assert len(cases) == 1
    else:
        assert {c[0] for c in cases} == {1, 3}
        assert {(c[4], c[3]) for c in cases} == {(n, p) for n in R.KERNEL_N for p in R.KERNEL_P}
        for n in R.KERNEL_N:
            assert {len(h) for c in cases if c[4] == n for h in c[2]} - {R.LONG_T} == set(R.kernel_lengths(n))
        assert (V == 6150) == any(len(h) == R.LONG_T > 4096 for c in cases for h in c[2])
    seen_ids, rep200, banned, signs = set(), False, False, set()
    for S, rows, hists, p, n in cases:
        assert rows.shape == (S, V) and rows.dtype == np.float32 and len(hists) == S
        if S == 3:
            assert len({len(h) for h in hists}) == 3
        tiny = np.isfinite(rows) & (rows != 0) & (np.abs(rows) < 1e-30)
        assert not tiny.any() and not np.isnan(rows).any()
        out = R.apply_rows(rows, hists, p, n)
        for r, h, o in zip(rows, hists, out):
            assert all(0 <= x < V for x in h)
            seen_ids |= set(h)
            rep200 = rep200 or (len(h) >= 200 and len(set(h[:200])) == 1)
            banned = banned or bool((np.isneginf(o) & ~np.isneginf(r)).any())
            for x in set(h):
                signs.add("inf" if np.isneginf(r[x]) else "zero" if r[x] == 0 else "pos" if r[x] > 0 else "neg")
            if np.isfinite(o).any():
                assert (o == o.max()).sum() == 1
    assert {0, V - 1} <= seen_ids
    if V > 8:
        assert rep200 and banned and signs == {"inf", "zero", "pos", "neg"}
