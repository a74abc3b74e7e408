"""Top log-probabilities without a GPU: the surfaces exist, the float64 reference against torch.topk + log_softmax and on hand-made
rows, the argument checks and the refusals that are decided on the host, and the inputs the GPU kernel test relies on."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import top_logprobs_ref as T
from qwen3_asr_rs_amd import engine
from qwen3_asr_rs_amd.engine import AsrInference, Q3aError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUST = os.path.join(ROOT, "integration", "rust", "src", "backend", "hip")
SYMS = ("q3a_set_top_logprobs", "q3a_fetch_top_logprobs", "q3a_selftest_top_logprobs")


# ---- the surfaces exist ---------------------------------------------------------------------------------------------------
def test_symbols_in_header_binding_rust_and_cli(lib):
    from qwen3_asr_rs_amd import _lib
    header = open(os.path.join(ROOT, "include", "q3asr.h")).read()
    rust = open(os.path.join(RUST, "engine.rs")).read()
    cli = open(os.path.join(ROOT, "qwen3_asr_rs_amd", "csrc", "asr_main.cpp")).read()
    for sym in SYMS:
        assert re.search(r"^int32_t %s\(" % sym, header, flags=re.M), sym
        assert sym in _lib.SYMBOLS and re.search(r"pub fn %s\(" % sym, rust), sym
        assert hasattr(lib, sym), f"libq3asr_hip.so does not export {sym}"
    assert re.search(r"pub fn set_top_logprobs\(&self, n: usize\)", rust) and re.search(r"pub fn fetch_top_logprobs\(&self,", rust)
    for name in ("set_top_logprobs", "fetch_top_logprobs", "top_logprobs_stats"):
        assert callable(getattr(engine.HipEngine, name))
    assert callable(engine.check_top_logprobs_args)
    assert "top_logprobs" in inspect.signature(AsrInference.transcribe).parameters
    assert "top_logprobs" in AsrInference._ROW_OPTION_KEYS
    assert [f.name for f in engine.dataclasses.fields(engine.TokenCandidate)] == ["id", "token", "logprob"]
    assert "top_logprobs" in [f.name for f in engine.dataclasses.fields(engine.TranscribeResult)]
    assert "Q3A_TOP_LOGPROBS" in cli


def test_header_states_the_contract():
    header = " ".join(open(os.path.join(ROOT, "include", "q3asr.h")).read().replace(" * ", " ").split())
    sec = header[header.index("---- top log-probabilities:"):header.index("int32_t q3a_selftest_top_logprobs(")]
    for phrase in ("0 <= n <= 20", "Larger logit first, then smaller id", "-0.0 and +0.0 are one value", "ranks last", "lp = -inf",
                   "fixed summation order", "bit-identical", "[s][t][0 .. n)", "writes nothing", "q3a_set_next_tokens",
                   "Independent of opts.token_logprobs", "pruned argmax is not taken", "fixed inner stride of 20", "device_bytes",
                   "an aligner engine", "q3a_prefill_draft", "q3a_beam_begin", "q3a_score* and q3a_align* never see it",
                   "q3a_group_engine"):
        assert phrase in sec, phrase


def test_every_logits_processor_has_a_kernel_of_its_own():
    """No kernel is a trampoline into another job's code: the kernel that once ran the sequence bias, the repetition penalty, the
    sampling filter and this selection as phases is gone with its argument struct and its launcher, k_repeat.hip holds the two
    history processors and k_toplp.hip the chunk kernel (a template) and the row kernel."""
    csrc = os.path.join(ROOT, "qwen3_asr_rs_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        text = open(os.path.join(csrc, name), errors="replace").read()
        # (the first name in two pieces: a search of the tree for it finds no file at all)
        for gone in ("history_" "apply_kernel", "SampleStageArgs", "launch_sample_stage", "_stage_phase"):
            assert gone not in text, (name, gone)
    assert not os.path.exists(os.path.join(csrc, "top_logprobs.h"))
    assert len(re.findall(r"__global__", open(os.path.join(csrc, "k_repeat.hip")).read())) == 2
    assert len(re.findall(r"__global__", open(os.path.join(csrc, "k_toplp.hip")).read())) == 2


# ---- the reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,n", [(20, 20), (63, 8), (2049, 20), (6150, 2)])
def test_reference_equals_torch_on_tie_free_rows(V, n):
    rng = np.random.default_rng(V)
    rows = (rng.permutation(V * 3).reshape(3, V) * 0.01 - 5.0).astype(np.float32)    # distinct values: no tie rule enters
    assert all(len(np.unique(r)) == V for r in rows)
    ids, lp = T.top_ref(rows, n)
    want = torch.topk(torch.from_numpy(rows).double(), n, dim=1)
    ls = torch.log_softmax(torch.from_numpy(rows).double(), dim=1)
    assert np.array_equal(ids, want.indices.numpy().astype(np.int32))
    assert np.abs(lp - torch.gather(ls, 1, want.indices).numpy()).max() < 1e-12


def test_reference_tie_zero_and_inf_rules():
    r = np.array([[1.0, 3.0, 3.0, -np.inf, 0.0, -0.0, 3.0, -np.inf]], np.float32)
    ids, lp = T.top_ref(r, 8)
    assert ids[0].tolist() == [1, 2, 6, 0, 4, 5, 3, 7]                                # ties by id; the zeros are one value; -inf last, by id
    assert np.isneginf(lp[0][6:]).all() and np.isfinite(lp[0][:6]).all()
    assert lp[0][4] == lp[0][5]
    assert abs(np.exp(lp[0][:6]).sum() - 1.0) < 1e-12
    r = np.array([[-0.0, 0.0, -0.0]], np.float32)
    assert T.top_ref(r, 2)[0][0].tolist() == [0, 1]


def test_reference_slot_rule():
    rows = T.random_rows(63, 4, 1)
    ids, lp, written = T.history_ref(rows, 3, [2, 0, 5, 4], [0, 1, 0, 0], 5)
    assert written[0, 2, :3].all() and written.sum() == 3 + 3                         # row 1 is done, row 2 has no slot
    assert written[3, 4, :3].all()
    assert (ids[~written] == -1).all() and (lp[~written] == 0.0).all()
    assert np.array_equal(ids[0, 2, :3], T.top_ref(rows[:1], 3)[0][0])


# ---- argument checks and refusals decided on the host ---------------------------------------------------------------------------
def test_python_argument_checks():
    assert engine.check_top_logprobs_args(0) == 0 and engine.check_top_logprobs_args(np.int32(20)) == 20
    for bad in (-1, 21, 2.0, "5", True, None):
        with pytest.raises(Q3aError, match="set_top_logprobs"):
            engine.check_top_logprobs_args(bad)
    engine.check_top_logprobs_compat(0, 4, [1, 2])                                      # off: nothing to refuse
    with pytest.raises(Q3aError, match="beam"):
        engine.check_top_logprobs_compat(5, 2, None)
    with pytest.raises(Q3aError, match="draft"):
        engine.check_top_logprobs_compat(5, 1, [1, 2])
    assert engine.uniform_top_logprobs([None, {}, {"temperature": 1.0}]) == 0
    assert engine.uniform_top_logprobs([{"top_logprobs": 5}, {"top_logprobs": 5}]) == 5
    with pytest.raises(ValueError, match="equal for all rows"):
        engine.uniform_top_logprobs([{"top_logprobs": 5}, None])
    with pytest.raises(ValueError, match="equal for all rows"):
        engine.uniform_top_logprobs([{"top_logprobs": 5}, {"top_logprobs": 6}])
    with pytest.raises(Q3aError):
        engine.uniform_top_logprobs([{"top_logprobs": 21}])


def test_asr_inference_refuses_before_the_engine_is_touched():
    asr = AsrInference(None, None)                                                      # no engine: whatever touches it raises AttributeError
    with pytest.raises(Q3aError, match="beam"):
        asr.transcribe(np.zeros(16000, np.float32), top_logprobs=5, beam_size=2)
    with pytest.raises(Q3aError, match="draft"):
        asr.transcribe(np.zeros(16000, np.float32), top_logprobs=5, draft=[1, 2, 3])
    with pytest.raises(Q3aError, match="set_top_logprobs"):
        asr.transcribe(np.zeros(16000, np.float32), top_logprobs=21)
    with pytest.raises(ValueError, match="equal for all rows"):
        asr.transcribe_batch([np.zeros(16000, np.float32)] * 2, options=[{"top_logprobs": 3}, {}])


def test_c_refusals_that_need_no_device(lib):
    f32p, i32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    rows = np.zeros((1, 8), np.float32)
    sc, done = np.zeros(1, np.int32), np.zeros(1, np.uint8)
    oi, ol = np.zeros(2 * 20, np.int32), np.zeros(2 * 20, np.float32)

    def call(n, V=8, stride=2, logits=rows):
        return lib.q3a_selftest_top_logprobs(0, logits.ctypes.data_as(f32p) if logits is not None else None, 1, V, n, sc.ctypes.data_as(i32p),
                                             done.ctypes.data_as(u8p), stride, oi.ctypes.data_as(i32p), ol.ctypes.data_as(f32p))
    for kw, msg in ((dict(n=0), "n must lie"), (dict(n=21), "n must lie"), (dict(n=9), "n must lie"), (dict(n=2, stride=0), "bad argument"),
                    (dict(n=2, logits=None), "bad argument")):
        assert call(**kw) != 0
        assert msg in lib.q3a_last_error(None).decode(), kw
    assert lib.q3a_set_top_logprobs(None, 5) != 0 and lib.q3a_fetch_top_logprobs(None, None, None, 0, 0, None) != 0


# ---- the rows of the GPU kernel test contain what they claim ---------------------------------------------------------------------
def test_hand_rows_contain_what_they_claim():
    rows = T.hand_rows()
    assert T.HAND_V == 3 * T.CHUNK + 6
    for name, (row, n, claim) in rows.items():
        assert row.shape == (T.HAND_V,) and row.dtype == np.float32 and not np.isnan(row).any(), name
        assert T.top_ref(row[None], n)[0][0].tolist() == claim, name
    row, n, claim = rows["one_chunk"]
    assert n == 20 and {i // T.CHUNK for i in claim} == {1}
    row, n, claim = rows["spread"]
    assert sorted(i // T.CHUNK for i in claim) == [0, 1, 2, 3]
    row = rows["tie_2047_2048"][0]
    assert row[2047] == row[2048] == row.max() and 2047 // T.CHUNK != 2048 // T.CHUNK and (row == row.max()).sum() == 2
    assert len(np.unique(rows["all_equal"][0])) == 1
    row = rows["zeros_boundary"][0]
    z = np.flatnonzero(row == 0.0)
    assert z.tolist() == [2046, 2047, 2048, 2049, 5000] and row.max() == 0.0
    assert np.signbit(row[z]).tolist() == [False, True, False, True, True]            # both signs on both sides of the boundary
    row, n, _ = rows["few_finite"]
    assert np.isfinite(row).sum() == 3 < n
    row = rows["steep"][0]
    with np.errstate(under="ignore"):
        assert (np.exp((row[1:] - row[0]).astype(np.float32)) == 0.0).all()           # every tail weight underflows in fp32
    big, at = T.big_rows()
    assert big.shape == (2, T.BIG_V) and len({int(i) // T.CHUNK for i in at}) == 20 and at.max() < T.BIG_V
    assert T.top_ref(big[1:], 20)[0][0].tolist() == at.tolist()
    quant = T.random_rows(6150, 2, 3)[1]
    assert (quant == np.sort(quant)[-20]).sum() > 1                                    # the quantised rows tie at the 20th place
