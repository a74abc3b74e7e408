"""The forced aligner on the fp32 oracle: composed from oracle/q3asr_oracle.py's own functions (encode, the decoder forward with
an untied [classify_num, hidden] head applied to every row), plus the checkpoints and word ids the aligner tests share."""
import os

import numpy as np
import torch

from oracle import q3asr_oracle as O
from qwen3_asr_rs_amd import synthetic

TS = 151705
AUDIO_START, AUDIO_END = 151669, 151670


def tiny_aligner_dir():
    return synthetic.write_checkpoint("/tmp/q3a_ckpt_tiny_aligner", "tiny_aligner", seed=3)


def aligner_0p6b_dir():
    return synthetic.write_checkpoint("/tmp/q3a_ckpt_0p6b_aligner", "0.6b_aligner", seed=4,
                                      embed_scale=synthetic.PEAKED_EMBED_SCALE)


def align_prompt(T, text_ids):
    """The aligner prompt, restated (the engine's is q3a_build_align_prompt)."""
    return [AUDIO_START] + [O.AUDIO_PAD_TOKEN_ID] * T + [AUDIO_END] + list(text_ids)


def word_ids(n_words, seed):
    """Word and marker ids of n_words seeded words of 1-3 ordinary vocabulary ids each."""
    rng = np.random.default_rng(seed)
    ids = []
    for _ in range(n_words):
        ids += [int(x) for x in rng.integers(100, 150000, size=int(rng.integers(1, 4)))] + [TS, TS]
    return ids


@torch.no_grad()
def oracle_align(oracle: O.AsrOracle, clip, text_ids):
    """(prompt ids, fp32 logits of the marker rows [markers][classify_num])."""
    tc = oracle.cfg.text
    audio = oracle.encode(clip)
    T = audio.shape[0]
    ids = align_prompt(T, text_ids)
    embed = O._w(oracle.weights, "thinker.model", "embed_tokens.weight")
    hidden = F_embedding(ids, embed)
    hidden[0, 1:1 + T] = audio
    cos, sin = O.compute_mrope_cos_sin(O.build_position_ids(ids), tc.head_dim, tc.rope_theta, tc.mrope_section, tc.mrope_interleaved)
    logits = O.text_decoder_forward(oracle.weights, tc, hidden, cos, sin, O.KvCache(tc.num_hidden_layers), O.create_causal_mask(len(ids), 0))
    rows = [i for i, x in enumerate(ids) if x == TS]
    return ids, logits[0, rows].numpy()


def F_embedding(ids, embed):
    return torch.nn.functional.embedding(torch.tensor(ids, dtype=torch.int64), embed)[None].clone()


def top2_margin(logits):
    s = np.sort(np.asarray(logits, dtype=np.float64), axis=-1)
    return s[..., -1] - s[..., -2]
