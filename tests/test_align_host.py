"""Forced aligner (Qwen3-ForcedAligner word timestamps) without a GPU: the oracle composition against HuggingFace's own
Qwen3ASRForTokenClassification, the C++ host helpers against HF's word split and monotonicity fix-up, the prompt layout, the
checkpoint / config rules and the exported symbols."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from align_ref import TS, align_prompt, oracle_align, tiny_aligner_dir
from oracle import q3asr_oracle as O
from qwen3_asr_rs_amd import _lib, synthetic
from qwen3_asr_rs_amd.audio import build_align_prompt, fix_timestamps, split_words_for_alignment

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["q3a_aligner_info", "q3a_build_align_prompt", "q3a_align", "q3a_align_batch_ptrs", "q3a_split_words_for_alignment",
               "q3a_align_text_ids", "q3a_fix_timestamps"]


@pytest.fixture(scope="module")
def aligner_oracle():
    return O.AsrOracle(tiny_aligner_dir())


def test_oracle_matches_hf_token_classification(aligner_oracle):
    """tests/golden/hf_align_pin.npz (make_hf_align_pin.py): HF's Qwen3ASRForTokenClassification on the seeded tiny aligner."""
    import sys
    sys.path.insert(0, GOLDEN)
    from make_hf_align_pin import CASES
    g = np.load(os.path.join(GOLDEN, "hf_align_pin.npz"))
    for n, (ci, sec, words) in enumerate(CASES):
        text = [x for w in words for x in list(w) + [TS, TS]]
        ids, lg = oracle_align(aligner_oracle, synthetic.synthetic_clip(ci, sec), text)
        assert ids == g[f"c{n}_ids"].tolist()
        assert lg.shape == (2 * len(words), 5000)
        np.testing.assert_allclose(lg[:, ::13], g[f"c{n}_logits_q"], atol=1e-4, rtol=0)
        np.testing.assert_allclose(np.take_along_axis(lg, g[f"c{n}_top_idx"], -1), g[f"c{n}_top_val"], atol=1e-4, rtol=0)
        assert lg.argmax(-1).tolist() == g[f"c{n}_classes"].tolist()


@pytest.fixture(scope="module")
def host_pin():
    with open(os.path.join(GOLDEN, "hf_align_host_pin.json")) as f:
        return json.load(f)


def test_split_words_matches_hf(lib, host_pin):
    for text, words in host_pin["split"]:
        assert split_words_for_alignment(text) == words, text


def test_split_words_refuses_japanese_and_korean(lib):
    for lang in ("japanese", "Japanese", "ja", "korean", "ko"):
        with pytest.raises(RuntimeError, match="not supported"):
            split_words_for_alignment("テスト", lang)
    assert split_words_for_alignment("a b", "english") == ["a", "b"]


def test_fix_timestamps_matches_hf(lib, host_pin):
    for seq, fixed in host_pin["fix"]:
        assert fix_timestamps(seq) == fixed, seq
        out = fix_timestamps(seq)
        assert all(a <= b for a, b in zip(out, out[1:])), seq
    assert fix_timestamps([]) == []


def test_build_align_prompt_ids(lib):
    text = [9707, TS, TS, 1879, 13, TS, TS]
    assert build_align_prompt(3, text) == [151669, 151676, 151676, 151676, 151670] + text
    assert build_align_prompt(0, []) == [151669, 151670]
    assert build_align_prompt(5, text) == align_prompt(5, text)


def test_align_text_ids_from_words(lib, tmp_path):
    from qwen3_asr_rs_amd.audio import AsrTokenizer
    vocab = {"a": 0, "b": 1, "ab": 2, "c": 3}
    tok = {"version": "1.0", "added_tokens": [], "model": {"type": "BPE", "vocab": vocab, "merges": ["a b"]}}
    p = tmp_path / "tokenizer.json"
    p.write_text(json.dumps(tok))
    t = AsrTokenizer(str(p))
    assert t.align_text_ids(["ab", "c", "abc"], TS) == [2, TS, TS, 3, TS, TS, 2, 3, TS, TS]
    assert t.align_text_ids([], TS) == []


def _arena_bytes(lib, d):
    n = C.c_uint64()
    rc = lib.q3a_arena_bytes(os.fsencode(d), C.byref(n))
    return rc, n.value, (lib.q3a_last_error(None) or b"").decode()


def _write_cfg(d, **over):
    cfg = dict(synthetic.CONFIG_TINY_ALIGNER)
    cfg["text_config"] = dict(cfg["text_config"])
    for k, v in over.items():
        if k == "tie":
            cfg["text_config"]["tie_word_embeddings"] = v
        elif v is None:
            cfg.pop(k, None)
        else:
            cfg[k] = v
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump({"thinker_config": cfg}, f)


def test_aligner_arena_holds_the_classifier(lib, tmp_path):
    """The arena of an aligner holds a [classify_num][hidden] bf16 head where an untied ASR checkpoint holds [vocab][hidden]."""
    a, u = tmp_path / "a", tmp_path / "u"
    _write_cfg(str(a))
    _write_cfg(str(u), classify_num=None, timestamp_token_id=None, timestamp_segment_time=None)
    ra, na, _ = _arena_bytes(lib, str(a))
    ru, nu, _ = _arena_bytes(lib, str(u))
    assert ra == 0 and ru == 0
    H = synthetic.CONFIG_TINY["text_config"]["hidden_size"]
    assert abs((nu - na) - (151936 - 5000) * H * 2) <= 256


def test_aligner_config_refusals(lib, tmp_path):
    d = tmp_path / "tied"
    _write_cfg(str(d), tie=True)
    rc, _, msg = _arena_bytes(lib, str(d))
    assert rc != 0 and "tied" in msg
    d = tmp_path / "badid"
    _write_cfg(str(d), timestamp_token_id=200000)
    rc, _, msg = _arena_bytes(lib, str(d))
    assert rc != 0 and "timestamp_token_id" in msg


def _pack(lib, d):
    rc, n, msg = _arena_bytes(lib, d)
    assert rc == 0, msg
    buf = (C.c_uint8 * n)()
    rc = lib.q3a_arena_pack(os.fsencode(d), buf, n)
    return rc, (lib.q3a_last_error(None) or b"").decode()


def test_aligner_checkpoint_head_refusals(lib, tmp_path):
    """A missing classifier or one with the wrong number of rows fails with a message naming it."""
    src = tiny_aligner_dir()
    assert _pack(lib, src)[0] == 0
    for name, rows in (("missing", None), ("rows", 4000)):
        d = tmp_path / name
        os.makedirs(d)
        with open(os.path.join(src, "config.json")) as f:
            (d / "config.json").write_text(f.read())
        w = O.load_model_weights(src)
        tensors = [(k, v) for k, v in w.items() if not (rows is None and k == "thinker.lm_head.weight")]
        if rows is not None:
            tensors = [(k, v[:rows] if k == "thinker.lm_head.weight" else v) for k, v in tensors]
        synthetic._write_safetensors(str(d / "model.safetensors"), tensors)
        rc, msg = _pack(lib, str(d))
        assert rc != 0 and "thinker.lm_head.weight" in msg, msg


def test_new_symbols_in_header_and_bindings():
    with open(os.path.join(ROOT, "include", "q3asr.h")) as f:
        hdr = f.read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", hdr), s
        assert s in _lib.SYMBOLS, s


def test_presets_leave_the_existing_ones_alone():
    """The aligner presets are new entries; the existing presets' tensor lists are what they were."""
    assert "classify_num" not in synthetic.CONFIG_TINY and "classify_num" not in synthetic.CONFIG_0P6B
    specs = synthetic.tensor_specs(synthetic.CONFIG_TINY_ALIGNER)
    head = [s for s in specs if s[0] == "thinker.lm_head.weight"]
    assert len(head) == 1 and head[0][1] == (5000, 256)
    assert [s[0] for s in synthetic.tensor_specs(synthetic.CONFIG_TINY_UNTIED)][-1] == "thinker.lm_head.weight"
    assert synthetic.tensor_specs(synthetic.CONFIG_TINY_UNTIED)[-1][1] == (151936, 256)
