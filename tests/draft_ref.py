"""numpy reference of draft-verified decoding (include/q3asr.h "draft-verified decoding"): the acceptance rule, the draft of the
next round, and every word of engine state the accept kernel leaves behind.  No device, no engine."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

EOS_IDS = (151643, 151645)
AUDIO_PAD = 151676


def accept(draft: Sequence[int], top_ids: Sequence[int]) -> Tuple[int, int]:
    """top_ids[i] = the argmax of the row that predicts position i (len(draft) + 1 of them).  Returns (k, tok): the FIRST i with
    top_ids[i] != draft[i] (len(draft) if there is none) and top_ids[k]."""
    n = len(draft)
    assert len(top_ids) >= n + 1
    k = next((i for i in range(n) if int(top_ids[i]) != int(draft[i])), n)
    return k, int(top_ids[k])


def accept_from_greedy(draft: Sequence[int], greedy: Sequence[int], max_new: int) -> int:
    """k for a draft against the ids a natural-EOS greedy run returned (EOS excluded): the rows up to the first mismatch are rows of
    that run, and behind its last id the run wrote an EOS (or hit max_new, where the draft cannot be longer)."""
    n = len(draft)
    assert n <= max_new
    for i in range(n):
        if i >= len(greedy) or int(draft[i]) != int(greedy[i]):
            return i
    return n


def next_round(draft: Sequence[int], k: int, tok: int) -> List[int]:
    """d[:k] + [tok] + d[k+1:], or d[:k] when tok is an EOS id."""
    d = [int(t) for t in draft]
    assert 0 <= k <= len(d)
    if int(tok) in EOS_IDS:
        return d[:k]
    return d[:k] + [int(tok)] + d[k + 1:]


def frag_index(s: int, k: int) -> int:
    """kernels.h skinny_frag_index."""
    return ((((k >> 5) * 2 + (s >> 4)) * 4 + ((k >> 3) & 3)) * 16 + (s & 15)) * 8 + (k & 7)


def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_rne(x: np.ndarray) -> np.ndarray:
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def expected_state(drafts: Sequence[Sequence[int]], top_ids: Sequence[Sequence[int]], top_lp: Optional[Sequence[Sequence[float]]],
                   prompt_lens: Sequence[int], out_stride: int, embed_bits: np.ndarray, norm_w: Optional[np.ndarray], group_size: int,
                   cos_t: np.ndarray, sin_t: np.ndarray, sentinel_i: int, sentinel_f: float, sentinel_h: int):
    """Everything q3a_selftest_draft_accept returns, for output buffers that arrived filled with the sentinels."""
    S = len(drafts)
    V, H = embed_bits.shape
    nparts = H // 16
    groups = (S + group_size - 1) // group_size
    out = {
        "accepted": np.zeros(2 * S, np.int32),
        "out_ids": np.full((S, out_stride), sentinel_i, np.int32),
        "out_lp": np.full((S, out_stride), sentinel_f, np.float32),
        "next_tok": np.zeros(S, np.int32), "step_count": np.zeros(S, np.int32), "pos": np.zeros(S, np.int32), "done": np.zeros(S, np.int32),
        "x_next": np.zeros((S, H), np.float32), "rope_cur": np.zeros((S, 128), np.float32),
        "nn_x": np.full(groups * 32 * H, sentinel_h, np.uint16), "nn_ss": np.full((groups, nparts, 32), sentinel_f, np.float64),
    }
    n_done = 0
    for s in range(S):
        k, tok = accept(drafts[s], top_ids[s])
        out["accepted"][s], out["accepted"][S + s] = k, tok
        out["next_tok"][s], out["step_count"][s], out["pos"][s] = tok, k + 1, prompt_lens[s] + k
        for i in range(min(k, out_stride)):
            out["out_ids"][s, i] = drafts[s][i]
            if top_lp is not None:
                out["out_lp"][s, i] = top_lp[s][i]
        if k < out_stride:
            out["out_ids"][s, k] = tok
            if top_lp is not None:
                out["out_lp"][s, k] = top_lp[s][k]
        if tok in EOS_IDS:
            out["done"][s] = 1
            n_done += 1
        x = bf16_to_f32(embed_bits[tok])
        out["x_next"][s] = x
        np_ = prompt_lens[s] + k
        out["rope_cur"][s, :64], out["rope_cur"][s, 64:] = cos_t[np_], sin_t[np_]
        if norm_w is not None:
            g, sl = s // group_size, s % group_size
            xw = f32_to_bf16_rne(x * norm_w.astype(np.float32))
            idx = np.array([frag_index(sl, c) for c in range(H)]) + g * 32 * H
            out["nn_x"][idx] = xw
            out["nn_ss"][g, 0, sl] = float(np.sum(x.astype(np.float64) ** 2))
            out["nn_ss"][g, 1:, sl] = 0.0
    out["n_done"] = n_done
    out["progress"] = (int(out["step_count"][0]), 1 if n_done == S else 0)
    return out
