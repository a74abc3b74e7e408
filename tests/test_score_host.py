"""Scoring a given transcript (q3a_score, q3a_score_batch_ptrs) without a GPU: the symbols are declared, exported and bound, and the
reference the GPU tests use (tests/score_ref.py) agrees with an independent teacher-forced run of the oracle."""
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from oracle import q3asr_oracle as O
from qwen3_asr_rs_amd import _lib, synthetic
from score_ref import oracle_score, perturb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["q3a_score", "q3a_score_batch_ptrs"]


def test_new_symbols_in_header_bindings_and_rust(lib):
    with open(os.path.join(ROOT, "include", "q3asr.h")) as f:
        hdr = f.read()
    # the engine-level Rust declarations live in engine.rs (ffi.rs is generated from the op-level header q3asr_ops.h only)
    with open(os.path.join(ROOT, "integration", "rust", "src", "backend", "hip", "engine.rs")) as f:
        rust = f.read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", hdr), s
        assert s in _lib.SYMBOLS, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
        assert re.search(r"pub fn " + s + r"\(", rust), s


def test_header_states_the_refusals_and_what_is_out_of_scope():
    with open(os.path.join(ROOT, "include", "q3asr.h")) as f:
        hdr = f.read()
    sec = hdr[hdr.index("scoring a given transcript"):hdr.index("int32_t q3a_score(")]
    for word in ("audio_pad", "stride", "aligner", "q3a_encode", "q3a_group", "score_head_ms", "Out of scope"):
        assert word in sec, word


@torch.no_grad()
def _one_shot(orc, clip, targets, prefix=None):
    """Independent of transcribe_ids' step loop: ONE causal forward over prompt ++ targets[:-1] with every position's logits."""
    tc = orc.cfg.text
    audio = orc.encode(clip)
    T = audio.shape[0]
    ids, apos = O.build_prompt(T, prefix)
    p = len(ids)
    ids = ids + [int(t) for t in targets[:-1]]
    embed = O._w(orc.weights, "thinker.model", "embed_tokens.weight")
    hidden = F.embedding(torch.tensor(ids, dtype=torch.int64), embed)[None].clone()
    hidden[0, apos[0]:apos[0] + T] = audio
    cos, sin = O.compute_mrope_cos_sin(O.build_position_ids(ids), tc.head_dim, tc.rope_theta, tc.mrope_section, tc.mrope_interleaved)
    logits = O.text_decoder_forward(orc.weights, tc, hidden, cos, sin, O.KvCache(tc.num_hidden_layers), O.create_causal_mask(len(ids), 0))
    return logits[0, p - 1:p - 1 + len(targets)]


def test_oracle_score_agrees_with_a_one_shot_forward(tiny_oracle):
    clip = synthetic.synthetic_clip(300, 1.25)
    greedy = tiny_oracle.transcribe_ids(clip, fixed_new_tokens=9, keep_logits=False).ids
    targets = [perturb(t) if s % 3 == 2 else t for s, t in enumerate(greedy)]
    for prefix in (None, [100, 2000, 30000]):
        lp, top, top_lp, margin, logits = oracle_score(tiny_oracle, clip, targets, prefix)
        assert logits.shape == (9, 151936) and len(lp) == len(top) == len(top_lp) == len(margin) == 9
        ref = torch.log_softmax(_one_shot(tiny_oracle, clip, targets, prefix).double(), -1).numpy()
        want = ref[np.arange(9), targets]
        np.testing.assert_allclose(lp, want, atol=1e-4, rtol=0)
        np.testing.assert_allclose(top_lp, ref.max(axis=1), atol=1e-4, rtol=0)
        assert np.all(lp <= top_lp) and np.all(top_lp <= 0) and np.all(margin >= 0)
        for i in range(9):
            assert int(top[i]) == int(ref[i].argmax()) or margin[i] < 1e-4, i
            assert (lp[i] == top_lp[i]) == (targets[i] == int(top[i])) or margin[i] == 0, i
    with_prefix = oracle_score(tiny_oracle, clip, targets, [100, 2000, 30000])[0]
    assert abs(with_prefix - oracle_score(tiny_oracle, clip, targets)[0]).max() > 1e-3  # the prefix reaches the prompt


def test_oracle_score_lengths_zero_and_one(tiny_oracle):
    clip = synthetic.synthetic_clip(301, 1.0)
    lp, top, top_lp, margin, logits = oracle_score(tiny_oracle, clip, [])
    assert len(lp) == len(top) == len(top_lp) == len(margin) == 0 and logits.shape == (0, 151936)
    lp, top, top_lp, margin, logits = oracle_score(tiny_oracle, clip, [7])
    prefill = tiny_oracle.transcribe_ids(clip, fixed_new_tokens=1, last_only=True)
    assert int(top[0]) == prefill.all_step_ids[0]
    assert np.array_equal(logits[0], prefill.step_logits[0].numpy())
