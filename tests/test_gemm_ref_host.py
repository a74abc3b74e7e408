"""CPU side of the GEMM family's fp64 checks (tests/gemm_ref.py): for every case tests/test_gpu_gemm_epilogues.py runs on the GPU, (a)
an honest float32 evaluation -- torch's matmul on the operands the kernel multiplies, the numpy restatements of gelu_fast / silu_fast,
torch's bf16 conversion -- lies inside the bound, so the bound is validated against the reference and not against the code under test,
and (b) every mutant the case lists lies outside it.  Every mutant of a family is listed by at least one case.  Plus: the new entry
points are declared, exported and bound, and the two wave-quantisation splits the cases rely on are the ones the library computes."""
import os
import re

import numpy as np
import pytest
import torch

import gemm_ref as G
import ops_ref as R
from qwen3_asr_rs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["q3a_selftest_gemm_launch", "q3a_selftest_qkrope_launch", "q3a_gemm256_split_rows"]
GROUPS = [(f, g) for f in ("dense", "conv") for g in G.groups(f)]
QK_CASES = [c["name"] for c in G.qk_cases()]


def test_new_symbols_in_header_bindings_and_rust(lib):
    with open(os.path.join(ROOT, "include", "q3asr.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "integration", "rust", "src", "backend", "hip", "engine.rs")) as f:
        rust = f.read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", hdr), s
        assert s in _lib.SYMBOLS, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
        assert re.search(r"pub fn " + s + r"\(", rust), s


def test_split_rows_the_cases_rely_on(lib):
    """257 tiles (remainder 1) and 258 tiles (remainder 2): the leading whole rounds stay with gemm256, the rest goes to the small tiles."""
    M, N, _, n_glu = G.SPLIT_TAIL
    assert lib.q3a_gemm256_split_rows(M, N) == G.SPLIT_TAIL_ROWS == 65536
    assert lib.q3a_gemm256_split_rows(M, n_glu) == 65536
    Mq, _, Tq = G.QK_SPLIT
    assert lib.q3a_gemm256_split_rows(Mq, 512) == Tq == 32768
    for M, N, _ in G.GEMM256_SHAPES:   # and the two-by-two shapes do not split
        assert lib.q3a_gemm256_split_rows(M, N) == 0
    for c in G.dense_cases() + G.qk_cases():
        if c["split_rows"]:
            assert lib.q3a_gemm256_split_rows(c["M"], c["N"]) == c["split_rows"], c["name"]


def test_every_mutant_is_listed_by_a_case():
    for fam, muts in G.FAMILY_MUTANTS.items():
        listed = {m for c in G.FAMILIES[fam]() for m in c["mutants"]}
        assert set(muts) <= listed, (fam, set(muts) - listed)
        assert listed <= set(muts), (fam, listed - set(muts))


def test_every_launcher_form_and_kind_has_a_case():
    d = G.dense_cases()
    assert {(c["launcher"], c["split"]) for c in d} >= {("gemm", 0), ("gemm", 1), ("gemm16", 0), ("gemm16_small", 0)}
    for form, *_ in G.GEMM16_FORMS:
        kinds = {c["kind"] for c in d if c["form"] == form}
        want = set(G.BF16_KINDS) if form in ("ring32x64", "bk32", "tile64", "tile128") else {k for k in G.BF16_KINDS if not G.KINDS[k]["glu"]}
        if form == "elementwise": want -= {"ldo_plus_8"}
        assert kinds == want, (form, want - kinds)
    for persist in (0, 1, 2):
        assert {c["kind"] for c in d if c["form"] == "gemm256" and c["knobs"]["gemm256_persist"] == persist} == set(G.BF16_KINDS)
    assert {c["kind"] for c in d if c["launcher"] == "gemm"} == set(G.F32_KINDS)
    cv = G.conv_cases()
    assert {c["C"] for c in cv if c["group"].startswith("conv256")} == {32, 64, 96}
    assert {(c["launcher"], c["split"]) for c in cv} == {("conv", 0), ("conv", 1), ("conv16", 0)}
    assert {(c["H"] % 2, c["W"] % 2) for c in cv} == {(0, 0), (1, 1), (1, 0), (0, 1)}
    q = G.qk_cases()
    assert {(c["fused"], c["kv_f32"], c["q16"]) for c in q} == {(1, 0, True), (0, 0, True), (0, 0, False), (0, 1, True), (0, 1, False)}


def test_conv_matrix_is_the_convolution():
    """The (kh, kw, c)-ordered im2col matrix times W^T is ops_ref.conv2d_ref of the same NHWC data."""
    for c in G.conv_cases()[::7]:
        d = G.materialize(c)
        A = G.a_matrix(c, d)
        x = d["x"].astype(np.float64).transpose(0, 3, 1, 2)
        w = d["w"].astype(np.float64).reshape(c["N"], 3, 3, c["C"]).transpose(0, 3, 1, 2)
        ref = R.conv2d_ref(x, w, None, (2, 2), (1, 1), (1, 1)).transpose(0, 2, 3, 1).reshape(c["M"], c["N"])
        assert np.abs(A @ d["w"].astype(np.float64).T - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), c["name"]


@pytest.mark.parametrize("family,group", GROUPS, ids=[g for _, g in GROUPS])
def test_bound_accepts_honest_fp32_and_rejects_every_mutant(family, group):
    worst = 0.0
    for c in G.groups(family)[group]:
        d = G.materialize(c)
        exp = G.evaluate(c, d)
        assert exp[1].any() and (exp[2][exp[1]] > 0).all(), c["name"]
        got = G.evaluate(c, d, honest=True)[0]
        w = G.worst_excess(got, exp)
        worst = max(worst, w)
        assert G.accepts(got, exp), f"{c['name']}: an honest float32 evaluation is at {w:.3f} of the bound"
        assert c["mutants"], c["name"]
        for m in c["mutants"]:
            wrong = G.evaluate(c, d, mut=m)[0]
            assert not G.accepts(wrong, exp), f"{c['name']}: mutant {m} passes"
    print(f"{group}: honest fp32 at {worst:.3f} of the bound")


@pytest.mark.parametrize("name", QK_CASES)
def test_qk_bound_accepts_honest_fp32_and_rejects_every_mutant(name):
    c = next(c for c in G.qk_cases() if c["name"] == name)
    d = G.qk_materialize(c)
    exp = G.qk_evaluate(c, d)
    got = G.qk_evaluate(c, d, honest=True)
    print(name, {k: round(G.worst_excess(got[k][0], exp[k]), 3) for k in exp})
    assert G.qk_accepts(got, exp), "an honest float32 evaluation is outside the bound"
    for k in ("kcache", "vcache"):   # cache rows no token names exist and stay untouched
        assert not exp[k][1].all() and exp[k][1].any()
    for m in c["mutants"]:
        assert not G.qk_accepts(G.qk_evaluate(c, d, mut=m), exp), f"mutant {m} passes"


def test_fast_activation_restatements_against_float64():
    """gelu_fast: the restatement's worst error per max(1, |x|) over [-12, 12) in steps of 1.2e-5 is the figure the device gate doubles
    (this sweep: 3.90e-7 at x = 0.895, 8.16e-7 absolute at x = 4.025; dev.h documents 4e-7).  silu_fast: inside its derived bound."""
    x = np.arange(-12.0, 12.0, 1.2e-5).astype(np.float32)
    x64 = x.astype(np.float64)
    err = np.abs(G.gelu_fast_f32(x).astype(np.float64) - G.gelu64(x64))
    rel = err / np.maximum(1.0, np.abs(x64))
    print(f"gelu_fast restatement: {rel.max():.3e} max(1, |x|) at x = {x[rel.argmax()]:.3f}; {err.max():.3e} absolute at x = {x[err.argmax()]:.3f}")
    assert rel.max() <= 1.02 * G.GELU_FAST_WORST and err.max() <= 8.2e-7
    _, b = G.gelu_step(x64, 0.0, True)
    assert (err <= b).all()
    xs = np.arange(-30.0, 30.0, 1e-4).astype(np.float32)
    s, bs = G.silu_step(xs.astype(np.float64), 0.0, True)
    es = np.abs(G.silu_fast_f32(xs).astype(np.float64) - s)
    print(f"silu_fast restatement at {(es / bs).max():.3f} of its bound")
    assert (es <= bs).all()


def test_bf16_rounding_bound_is_half_an_ulp():
    """Round to nearest is within half a bf16 ulp: 2^-8 |v| just above a power of two, 2^-9 |v| just below the next -- torch's own conversion
    needs the former -- and truncation leaves it wherever it differs from rounding."""
    v = np.float32([1.0 + 2.0 ** -8 + 2.0 ** -20, 1.9960938, 3.0e-3, 1234.5])
    err = np.abs(G.bf16_round(v).astype(np.float64) - v)
    assert (err <= G.half_ulp_bf16(v)).all()
    assert err[0] > 2.0 ** -9 * v[0] and abs(G.half_ulp_bf16(v[1]) / v[1] - 2.0 ** -9) < 2.0 ** -17
    x = R.f32(np.random.default_rng(5).standard_normal(4096))
    t = G.bf16_truncate(x)
    differs = t != G.bf16_round(x)
    assert differs.any() and (np.abs(t.astype(np.float64) - x)[differs] > G.half_ulp_bf16(x)[differs]).all()
