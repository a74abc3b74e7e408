"""Top-k / top-p without a GPU: the surfaces exist, the header states the contract, the refusals that need no device, the numpy
reference against HuggingFace's warper chain, the distribution of the reference's draws, and the conditions the GPU kernel test
rests on, held for every seeded input."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import sampling_filter_ref as F
import sampling_ref as R
from qwen3_asr_rs_amd.engine import Q3aError
from test_sampling_host import _chi2_sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUST = os.path.join(ROOT, "integration", "rust", "src", "backend", "hip")


# ---- the surfaces exist ---------------------------------------------------------------------------------------------------
def test_symbols_in_header_binding_rust_and_cli(lib):
    from qwen3_asr_rs_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "q3asr.h")).read()
    rust = open(os.path.join(RUST, "engine.rs")).read()
    cli = open(os.path.join(ROOT, "qwen3_asr_rs_amd", "csrc", "asr_main.cpp")).read()
    for sym in ("q3a_set_sampling_filter", "q3a_selftest_sample_filter"):
        assert re.search(r"^int32_t %s\(" % sym, header, flags=re.M), sym
        assert sym in _lib.SYMBOLS and re.search(r"pub fn %s\(" % sym, rust), sym
        assert hasattr(lib, sym), f"libq3asr_hip.so does not export {sym}"
    assert re.search(r"pub fn set_sampling_filter\(&self, top_k: usize, top_p: f32\)", rust)
    assert "q3a_set_sampling_filter" not in open(os.path.join(RUST, "ffi.rs")).read()      # ffi.rs stays the generator's output
    for name in ("set_sampling_filter", "sampling_filter_stats"):
        assert callable(getattr(engine.HipEngine, name))
    assert callable(engine.check_sampling_filter_args)
    sig = inspect.signature(engine.AsrInference.transcribe).parameters
    assert sig["top_k"].default == 0 and sig["top_p"].default == 1.0
    assert "Q3A_TOP_K" in cli and "Q3A_TOP_P" in cli and "q3a_set_sampling_filter(" in cli


def test_header_states_the_contract():
    header = " ".join(open(os.path.join(ROOT, "include", "q3asr.h")).read().replace(" * ", " ").split())
    sec = header[header.index("---- sampling filter:"):header.index("int32_t q3a_selftest_sample_filter(")]
    for phrase in ("tau = max(tau_k, tau_p, tau_minp)", "never a rank", "-0.0 and +0.0 are equal values",
                   # the tie rule
                   "every entry that ties the k-th value is kept", "equal values share their fate", "here the whole run is kept",
                   "fewer than top_k finite entries every finite entry is kept", "smallest row value v with G(v) < top_p",
                   "TemperatureLogitsWarper(T) -> TopKLogitsWarper(k) -> TopPLogitsWarper(p) -> MinPLogitsWarper(min_p)",
                   # delta and where it comes from
                   "delta = 1e-5", "tau_ref(top_p + delta) <= tau <= tau_ref(top_p - delta)", "28 2^-23", "2 ulp", "2^17.2 2^-40",
                   "bit-identical from run to run",
                   # the refusals
                   "top_k < 0", "top_p NaN or outside (0, 1]", "an aligner engine", "the engine stays usable",
                   # state, the readable state
                   "(0, 1.0f) = off", "only while sampling is on", "replays the same graph",
                   'q3a_debug_read(e, "sampling_filter", ..) (uint32 [3]', '"sample_threshold" (fp32 [S]', '"sample_kept" (int32 [S]',
                   # out of scope
                   "typical / eta / epsilon sampling", "min_tokens_to_keep > 1", "per-utterance settings inside one batch",
                   "a filter inside beam search"):
        assert phrase in sec, phrase
    assert f"{F.DELTA:g}" == "1e-05"
    # the sampling section no longer calls the two out of scope
    samp = header[header.index("---- sampling: the next id"):header.index("int32_t q3a_set_sampling(")]
    assert "Out of scope: top-k" not in samp and "their own section below" in samp


# ---- refusals that need no device -----------------------------------------------------------------------------------------
def test_refusals_that_need_no_device(lib):
    from qwen3_asr_rs_amd.engine import check_sampling_filter_args
    assert check_sampling_filter_args() == (0, 1.0) and check_sampling_filter_args(50, 0.9) == (50, 0.9)
    assert check_sampling_filter_args(np.int32(3), 1) == (3, 1.0)
    for args, msg in [((-1,), "top_k"), ((1.5,), "top_k"), ((True,), "top_k"), (("many",), "top_k"), ((1 << 31,), "top_k"),
                      ((0, 0.0), "top_p"), ((0, -0.1), "top_p"), ((0, 1.01), "top_p"), ((0, float("nan")), "top_p"),
                      ((0, 1e-60), "top_p"), ((0, "most"), "top_p")]:
        with pytest.raises(Q3aError, match=msg):
            check_sampling_filter_args(*args)
    # the C entry points: a null engine, and the selftest's arguments before it looks for a device
    assert lib.q3a_set_sampling_filter(None, 50, C.c_float(0.9)) != 0
    x = np.zeros(4, dtype=np.float32)
    xp = x.ctypes.data_as(C.POINTER(C.c_float))
    for T, mp, k, p, V, msg in [(0.0, 0.0, 0, 1.0, 4, b"temperature"), (1.0, 1.5, 0, 1.0, 4, b"min_p"), (1.0, 0.0, -1, 1.0, 4, b"top_k"),
                                (1.0, 0.0, 0, 0.0, 4, b"top_p"), (1.0, 0.0, 0, 1.5, 4, b"top_p"), (1.0, 0.0, 0, float("nan"), 4, b"top_p"),
                                (1.0, 0.0, 0, 1.0, 0, b"bad argument")]:
        rc = lib.q3a_selftest_sample_filter(0, xp, 1, V, C.c_float(T), C.c_float(mp), k, C.c_float(p), 0, 0, None, None, None, None, None)
        assert rc != 0 and msg in lib.q3a_last_error(None), (T, mp, k, p, V, lib.q3a_last_error(None))


def test_transcribe_refuses_a_filter_without_sampling():
    """The check runs before the engine is touched: an AsrInference without an engine is enough."""
    from qwen3_asr_rs_amd.engine import AsrInference
    asr = AsrInference.__new__(AsrInference)
    for kw in ({"top_k": 5}, {"top_p": 0.9}, {"top_k": 5, "temperature": (0.0,)}):
        with pytest.raises(Q3aError, match="temperature > 0"):
            asr.transcribe(np.zeros(16000, np.float32), **kw)
    with pytest.raises(Q3aError, match="top_p"):
        asr.transcribe(np.zeros(16000, np.float32), temperature=1.0, top_p=0.0)


def test_cost_tool_refuses_an_unknown_arm():
    """tools/sampling_cost.py: a misspelt arm is an error before anything is loaded, not a silent T = 1 run."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sampling_cost.py"), "--arms", "off,t1k5O"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "unknown arm" in out.stderr and "t1k5O" in out.stderr


# ---- the reference --------------------------------------------------------------------------------------------------------
GRID = [(V, T, k, p, mp) for V in (5, 63, 700) for T in (0.3, 1.0, 2.0) for k in (0, 1, 3, 50) for p in (0.1, 0.5, 0.9, 0.999, 1.0)
        for mp in (0.0, 0.05)]


def _hf_finite(row64, T, k, p, mp):
    """What HuggingFace's chain leaves finite, on a float64 row."""
    import torch
    from transformers import MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s, ids = torch.tensor(row64, dtype=torch.float64)[None], torch.zeros((1, 1), dtype=torch.long)
    if T != 1.0:
        s = TemperatureLogitsWarper(float(T))(ids, s)
    if k > 0:
        s = TopKLogitsWarper(k)(ids, s)
    if p < 1.0:
        s = TopPLogitsWarper(float(p))(ids, s)
    if mp > 0.0:
        s = MinPLogitsWarper(float(mp))(ids, s)
    return torch.isfinite(s[0]).numpy(), s[0]


def _ref_kept(row, T, k, p, mp):
    l = np.asarray(row, np.float32)
    return np.isfinite(l) & (l.astype(np.float64) >= max(float(F.threshold(row, T, k, p)[0]), F.minp_threshold(row, T, mp)))


def test_reference_equals_the_transformers_warper_chain():
    """TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> MinPLogitsWarper in float64 on tie-free rows (fp32 values, so
    the reference sees the same numbers), and top-k on a tied row."""
    pytest.importorskip("transformers")
    rng = np.random.default_rng(0)
    for V, T, k, p, mp in GRID:
        row = (rng.standard_normal(V) * 2.5).astype(np.float32)
        while len(np.unique(row)) != V:                                                      # tie-free rows
            row = (rng.standard_normal(V) * 2.5).astype(np.float32)
        Tf, pf, mpf = float(np.float32(T)), float(np.float32(p)), float(np.float32(mp))          # the settings as the engine holds them
        want, _ = _hf_finite(row.astype(np.float64), Tf, k, pf, mpf)
        assert np.array_equal(_ref_kept(row, T, k, p, mp), want), (V, T, k, p, mp)
    assert len(GRID) == 360
    tied = np.array([1.0, 3.0, 2.0, 2.0, -1.0, 2.0, 0.5], np.float32)                         # the 3rd place inside a run of three
    for k, n in ((1, 1), (2, 4), (3, 4), (4, 4), (5, 5), (7, 7), (9, 7)):
        want, _ = _hf_finite(tied.astype(np.float64), 1.0, min(k, 7), 1.0, 0.0)
        assert np.array_equal(_ref_kept(tied, 1.0, k, 1.0, 0.0), want) and F.threshold(tied, 1.0, k, 1.0)[1] == n, k


def test_reference_edge_rules():
    inf = np.inf
    row = np.array([1.0, -inf, 3.0, 3.0, 2.9, 0.0, -0.0, -2.0], np.float32)
    assert F.threshold(row, 1.0, 0, 1.0) == (-inf, 7) and F.threshold(row, 1.0, 8, 1.0) == (-inf, 7)     # off both ways
    assert F.threshold(row, 1.0, 1, 1.0) == (3.0, 2) and F.threshold(row, 1.0, 2, 1.0) == (3.0, 2)       # ties at the k-th place stay
    t, n = F.threshold(row, 1.0, 5, 1.0)                                                              # the 5th place is a zero: both stay
    assert t == 0.0 and not np.signbit(t) and n == 6
    assert F.threshold(row, 1.0, 7, 1.0)[0] == -2.0 and F.threshold(row, 1.0, 8, 1.0)[0] == -inf
    few = np.array([-inf, 2.0, -inf, 1.0], np.float32)
    assert F.threshold(few, 1.0, 3, 1.0) == (-inf, 2)                                                  # fewer finite entries than top_k
    # top-p: the twin maxima share their fate; a tiny top_p keeps the maximum alone (G = 0 qualifies)
    assert F.threshold(row, 1.0, 0, 1e-6) == (3.0, 2)
    p = np.exp(row.astype(np.float64) - 3.0)
    p /= p.sum()
    assert F.threshold(row, 1.0, 0, float(2 * p[2] + 1e-6)) == (np.float32(2.9), 3)
    assert F.threshold(row, 1.0, 0, float(2 * p[2] - 1e-6)) == (3.0, 2)
    # top-p is renormalised over the top-k set, at temperature T
    assert F.threshold(row, 1.0, 3, 0.999999) == (np.float32(2.9), 3)
    assert F.threshold(row, 0.01, 0, 0.99) == (3.0, 2)
    # the sandwich brackets the threshold, and top_p = 1 is exact
    lo, hi = F.sandwich(row, 1.0, 0, 0.9)
    assert lo[0] <= F.threshold(row, 1.0, 0, 0.9)[0] <= hi[0] and lo[1] >= hi[1]
    assert F.sandwich(row, 1.0, 2, 1.0) == ((3.0, 2), (3.0, 2))


def test_reference_draws_follow_the_huggingface_distribution():
    """One row of 100 logits, T = 0.7, top_k = 40, top_p = 0.9, min_p = 0.02, 8192 draws over (s, t): nothing outside K is drawn, and a
    chi-square test against softmax of what HuggingFace's chain leaves passes at p > 0.01 (cells with an expectation under 5 pooled)."""
    T, k, tp, mp, seed, n_s, n_t = 0.7, 40, 0.9, 0.02, 2025, 64, 128
    row = (np.random.default_rng(9).standard_normal(100) * 1.5).astype(np.float32)
    p = F.filtered_softmax(row, T, mp, k, tp)
    keep = p > 0
    try:
        import torch
        _, s = _hf_finite(row.astype(np.float64), float(np.float32(T)), k, float(np.float32(tp)), float(np.float32(mp)))
        p = torch.softmax(s, -1).numpy()                                                   # the renormalised HuggingFace distribution
        assert np.array_equal(p > 0, keep)
    except ImportError:
        pass
    assert 3 <= keep.sum() < 40 and keep[np.argmax(row)] and abs(p.sum() - 1.0) < 1e-12
    counts = np.zeros(100, dtype=np.int64)
    for s in range(n_s):
        for t in range(n_t):
            counts[F.sample(row, T, mp, k, tp, seed, s, t).id] += 1
    n = n_s * n_t
    assert counts.sum() == n == 8192 and (counts[~keep] == 0).all()
    exp = p * n
    big = keep & (exp >= 5.0)
    obs_cells, exp_cells = list(counts[big]), list(exp[big])
    if (keep & ~big).any():
        obs_cells.append(counts[keep & ~big].sum())
        exp_cells.append(exp[keep & ~big].sum())
    chi2 = float(sum((o - e) ** 2 / e for o, e in zip(obs_cells, exp_cells)))
    pv = _chi2_sf(chi2, len(obs_cells) - 1)
    print(f"[sampling filter] chi-square {chi2:.2f} on {len(obs_cells) - 1} degrees of freedom, p = {pv:.3f}; |K| = {int(keep.sum())}")
    assert pv > 0.01


# ---- what the GPU kernel test rests on --------------------------------------------------------------------------------------
def test_kernel_combos_cover_the_grid():
    for V in F.KERNEL_V:
        combos = F.kernel_combos(V)
        assert {c[0] for c in combos} == {0.2, 1.0, 2.0} and {c[1] for c in combos} == {0.0, 0.05}
        assert {c[2] for c in combos} == {0, 1, 2, 50, V, V + 7} and {c[3] for c in combos} == {1.0, 0.9, 0.5, 0.05}
        assert any(0 < c[2] < V and c[3] < 1.0 for c in combos) or V <= 2                 # top-k and top-p together
        assert {len(g) for g, *_ in F.kernel_calls(V)} == {1, 3}
        assert {r for g, *_ in F.kernel_calls(V) for r in g} == set(range(F.N_ROWS))
    assert F.kernel_combos(F.BIG_V) == [(1.0, 0.05, 50, 0.9, 7)]
    assert all(s > 1 << 32 for s in F.SAMPLE_SEED.values())


@pytest.mark.parametrize("V", list(F.KERNEL_V) + [F.BIG_V])
def test_kernel_inputs_are_what_the_gpu_test_claims(V):
    rows = F.kernel_rows(V)
    assert rows.shape == (F.N_ROWS, V) and rows.dtype == np.float32 and not np.isnan(rows).any()
    assert np.array_equal(rows[:6].view(np.uint32), R.kernel_rows(V).view(np.uint32))
    assert len(np.unique(rows[6])) == 1 and np.isfinite(rows[6, 0])                       # all entries equal
    if V >= 63:
        z = rows[7] == 0                                                                  # both zeros, at the 2nd and the 50th place
        assert np.signbit(rows[7][z]).any() and (~np.signbit(rows[7][z])).any() and (rows[7] > 0).sum() == 1
        assert 1 + z.sum() >= 50 or V == 63
        assert F.threshold(rows[7], 1.0, 2, 1.0) == (0.0, 1 + z.sum())
        assert np.isfinite(rows[10]).sum() == F.N_FINITE < 50 and F.threshold(rows[10], 1.0, 50, 1.0) == (-np.inf, F.N_FINITE)
    for T in (0.2, 1.0, 2.0):                                                             # one logit with more than top_p of the mass
        assert F.threshold(rows[8], T, 0, 0.9) == (rows[8].max(), 1) or V == 1
    if V >= 63:
        v, c = np.unique(rows[9], return_counts=True)
        tied = np.nonzero(rows[9] == v[-2])[0]                                            # the run under the single maximum
        assert c[-1] == 1 and c[-2] >= 25 and F.threshold(rows[9], 1.0, 2, 1.0) == (v[-2], 1 + c[-2])
        if V > R.CHUNK:
            assert tied.min() < R.CHUNK and tied.max() >= ((V - 1) // R.CHUNK) * R.CHUNK  # tied across two different chunks
    if V >= 2048:                                                                         # a steep row: the tail weighs nothing at 2^-40
        w = np.exp((rows[11].astype(np.float64) - rows[11].max()) / 0.2)
        assert (w * 2.0 ** 40 < 1).sum() > V // 2


@pytest.mark.parametrize("V", list(F.KERNEL_V) + [F.BIG_V])
def test_kernel_inputs_have_no_close_calls(V):
    """What tests/test_gpu_sampling_filter.py relies on, held by the reference alone: over every draw of the kernel test the margin
    between the best two z stays above 1e-3 T over the filtered kept sets, the winner over K(top_p + DELTA) lies inside
    K(top_p - DELTA) (it is the winner there too), and no logit lies within 1e-4 of a min-p threshold.  The seeds in
    sampling_filter_ref were chosen so that no draw is left out; the cap of DESIGN.md section 3.11 (1 %) is the most it may ever be."""
    calls, cases = F.kernel_calls(V), F.kernel_draws(V)
    assert len(cases) == sum(len(c[0]) for c in calls)
    unsafe = [(c.call, c.s) for c in cases if not F.draw_is_safe(c, calls[c.call][1])]
    assert len(unsafe) <= 0.01 * len(cases), unsafe
    assert not unsafe, unsafe
    for c in cases:
        assert c.lo[0] <= c.hi[0] and c.lo[1] >= c.hi[1] and c.draw_hi.kept[c.draw_lo.id]
        if calls[c.call][4] == 1.0:
            assert c.lo == c.hi                                                           # top-k alone is exact
