"""Host side of the logit bias (no GPU): the list parser of the C ABI, compose_logit_bias, the numpy reference, and that the
symbols exist in the header, the Python binding and the Rust declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import logit_bias_ref as R
from qwen3_asr_rs_amd.engine import EOS_TOKEN_IDS, Q3aError, compose_logit_bias, parse_logit_bias

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 151936


# ---- q3a_parse_logit_bias -------------------------------------------------------------------------------------------------
def test_parser_lines_ranges_comments_and_inf(lib):
    text = "# domain nudges\n\n17 1.5\n  20-22\t-0.25   # three ids\n151645 -inf\n9 -Infinity\n3 - 4 2e-1\n"
    ids, bias = parse_logit_bias(text, None)
    assert ids.tolist() == [17, 20, 21, 22, 151645, 9, 3, 4]
    assert bias.dtype == np.float32 and ids.dtype == np.int32
    assert bias.tolist() == [1.5, -0.25, -0.25, -0.25, -np.inf, -np.inf, np.float32(0.2), np.float32(0.2)]


def test_parser_takes_a_bias_that_underflows(lib):
    """A value below fp32's range is a harmless 0 (or a denormal), not a refusal; one above it is refused (test_parser_refusals)."""
    ids, bias = parse_logit_bias("5 1e-50\n6 -1e-50\n7 1e-40\n", None)
    assert ids.tolist() == [5, 6, 7]
    assert bias[0] == 0.0 and bias[1] == 0.0 and 0.0 < float(bias[2]) < 2.0 ** -126


def test_parser_suppress_list_and_both_sources(lib):
    ids, bias = parse_logit_bias(None, "5, 10-12 ,151643")
    assert ids.tolist() == [5, 10, 11, 12, 151643] and np.all(bias == -np.inf)
    ids, bias = parse_logit_bias("1 0.5\n", "2-3")
    assert ids.tolist() == [1, 2, 3] and bias.tolist() == [0.5, -np.inf, -np.inf]
    for empty in ((None, None), ("", ""), ("# nothing\n\n", "  ")):
        ids, bias = parse_logit_bias(*empty)
        assert len(ids) == 0 and len(bias) == 0


@pytest.mark.parametrize("text,sup,msg", [
    ("7 1\n7 2\n", None, "duplicate id 7"),
    ("5-9 1\n8 -inf\n", None, "duplicate id 8"),
    ("4 1\n", "4", "duplicate id 4"),
    (None, "1,1", "duplicate id 1"),
    ("12\n", None, "line 1"),
    ("1 2\nabc 1\n", None, "line 2"),
    ("1 x\n", None, "not a finite bias"),
    ("1 nan\n", None, "not a finite bias"),
    ("1 inf\n", None, "not a finite bias"),
    ("1 +inf\n", None, "not a finite bias"),
    ("1 1e99\n", None, "not a finite bias"),
    ("-3 1\n", None, "not an id"),
    ("9-3 1\n", None, "runs backwards"),
    ("1.5 1\n", None, "not an id"),
    ("0-99999999 1\n", None, "too large"),
    (None, "1,,2", "empty item"),
    (None, "1;2", "not an id"),
    (None, "a-b", "not an id"),
])
def test_parser_refusals(lib, text, sup, msg):
    with pytest.raises(Q3aError, match=re.escape(msg)):
        parse_logit_bias(text, sup)


def test_parser_cap_smaller_than_needed(lib):
    """*n = entries needed, at most cap written: the rest of the caller's arrays is untouched."""
    n = C.c_int32()
    ids = np.full(8, -7, np.int32)
    bias = np.full(8, 99.0, np.float32)
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    rc = lib.q3a_parse_logit_bias(b"10-15 0.5\n", b"1,2", ids.ctypes.data_as(i32p), bias.ctypes.data_as(f32p), 3, C.byref(n))
    assert rc == 0 and n.value == 8
    assert ids.tolist() == [10, 11, 12, -7, -7, -7, -7, -7] and bias.tolist() == [0.5, 0.5, 0.5, 99.0, 99.0, 99.0, 99.0, 99.0]
    rc = lib.q3a_parse_logit_bias(b"10-15 0.5\n", b"1,2", None, None, 0, C.byref(n))
    assert rc == 0 and n.value == 8
    assert lib.q3a_parse_logit_bias(b"1 1\n", None, None, None, 4, C.byref(n)) != 0  # cap > 0 without arrays
    assert b"bad argument" in lib.q3a_last_error(None)


# ---- compose_logit_bias ---------------------------------------------------------------------------------------------------
def test_compose_suppress_and_bias():
    ids, bias, default = compose_logit_bias(V, suppress_tokens=[9, 3], logit_bias={5: 1.25, 3: 0.5, 7: -np.inf, 11: 0.0})
    assert default == 0.0 and ids.dtype == np.int32 and bias.dtype == np.float32
    assert ids.tolist() == [3, 5, 7, 9]                      # ascending, unique; 11 carries the default and is left out
    assert bias.tolist() == [-np.inf, 1.25, -np.inf, -np.inf]  # suppress wins over the finite bias on id 3
    assert compose_logit_bias(V)[0].size == 0 and compose_logit_bias(V)[2] == 0.0


def test_compose_allow_list_keeps_eos_unless_told_otherwise():
    ids, bias, default = compose_logit_bias(V, allowed_tokens=[10, 20, 30], logit_bias={20: -0.5, 40: 3.0}, suppress_tokens=[30])
    assert default == -np.inf
    assert ids.tolist() == [10, 20] + sorted(EOS_TOKEN_IDS)   # 30 suppressed, 40 is outside the allow-list
    assert bias.tolist() == [0.0, -0.5, 0.0, 0.0]
    ids, bias, default = compose_logit_bias(V, allowed_tokens=[10, 20], keep_eos=False)
    assert ids.tolist() == [10, 20] and default == -np.inf
    # the dense vector the engine would hold
    b = R.dense(V, ids, bias, default)
    assert np.isfinite(b).sum() == 2 and b[10] == 0.0 and b[0] == -np.inf


@pytest.mark.parametrize("kw", [dict(suppress_tokens=[-1]), dict(suppress_tokens=[V]), dict(logit_bias={V: 1.0}),
                                dict(logit_bias={1: float("nan")}), dict(logit_bias={1: float("inf")}), dict(allowed_tokens=[2.5])])
def test_compose_refusals(kw):
    with pytest.raises(ValueError):
        compose_logit_bias(V, **kw)


# ---- the reference itself -------------------------------------------------------------------------------------------------
def test_reference_arithmetic():
    x = np.array([1.0, 3.0, -np.inf, 3.0, 2.0], np.float32)
    assert R.argmax(x) == 1                                    # first of the equal maxima
    ls = R.log_softmax64(x)
    assert ls[2] == -np.inf and not np.isnan(ls).any()
    assert np.exp(ls[np.isfinite(ls)]).sum() == pytest.approx(1.0, abs=1e-15)
    a = R.kind_suppress(V, [5, 70000], 70000)
    lo = (70000 // 2048) * 2048 - 2048
    assert set(range(lo, lo + 6144)) <= set(a) and 5 in a and len(a) == 6145
    assert len(R.kind_suppress(V, [], 100)) == 6144 and min(R.kind_suppress(V, [], 100)) == 0   # clipped at 0
    assert max(R.kind_suppress(V, [], V - 1)) == V - 1                                          # clipped at V
    b = R.kind_small(V, [5], 70000)
    fin = {t: v for t, v in b.items() if np.isfinite(v)}
    assert 0 in b and V - 1 in b and 50 <= len(fin) <= 64 and all(0.05 <= abs(v) <= 2.0 for v in fin.values())
    c, default = R.kind_allow(V)
    assert default == -np.inf and 1000 <= len(c) <= 1002 and set(R.EOS_IDS) <= set(c)
    assert np.isfinite(R.as_dense(V, c, default)).sum() == len(c)


# ---- the surfaces exist ---------------------------------------------------------------------------------------------------
def test_symbols_in_header_binding_and_rust():
    from qwen3_asr_rs_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "q3asr.h")).read()
    rust = open(os.path.join(ROOT, "integration", "rust", "src", "backend", "hip", "engine.rs")).read()
    cli = open(os.path.join(ROOT, "qwen3_asr_rs_amd", "csrc", "asr_main.cpp")).read()
    for sym in ("q3a_set_logit_bias", "q3a_parse_logit_bias"):
        assert re.search(r"^int32_t %s\(" % sym, header, flags=re.M), sym
        assert sym in _lib.SYMBOLS and re.search(r"pub fn %s\(" % sym, rust), sym
    assert "q3a_score* and q3a_align*" in header and "Out of scope: per-utterance biases" in header
    for name in ("set_logit_bias", "logit_bias_vector", "logit_bias_stats"):
        assert callable(getattr(engine.HipEngine, name))
    assert callable(engine.compose_logit_bias) and callable(engine.parse_logit_bias)
    import inspect
    assert {"suppress_tokens", "logit_bias", "allowed_tokens"} <= set(inspect.signature(engine.AsrInference.transcribe).parameters)
    assert "Q3A_SUPPRESS_TOKENS" in cli and "Q3A_LOGIT_BIAS" in cli
