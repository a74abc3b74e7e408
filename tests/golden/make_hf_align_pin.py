"""Independent pin of the forced-aligner path (Qwen3-ForcedAligner) at tiny dimensions.

HuggingFace `transformers` (5.15 in the build container) ships `Qwen3ASRForTokenClassification` (the aligner network: the ASR
encoder and decoder with a `score` classifier over the time classes) and the processor's `split_words_for_alignment` /
`_fix_timestamps`.  This script loads the seeded synthetic aligner checkpoint (reference key layout; `thinker.lm_head.weight`
becomes `score.weight`) into that model, runs three clips with their aligner prompts and stores the marker-row logits (every
13th class, the top 4 and the argmax) in hf_align_pin.npz.  It also runs the two host functions on mixed scripts and on
adversarial timestamp sequences and stores their results in hf_align_host_pin.json.  tests/test_align_host.py holds the oracle
and the C++ host helpers to them.

The prompt layout is the engine's (csrc/host_align.cpp, the original aligner's: audio start, audio pads, audio end, then per
word its ids and two <timestamp> markers); HF builds it from a chat template that only a real checkpoint carries, so it is
restated here.  Nothing of `transformers` travels: only the numbers.  Run in the build container:
    python tests/golden/make_hf_align_pin.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import q3asr_oracle as O  # noqa: E402
from qwen3_asr_rs_amd import synthetic  # noqa: E402
from make_hf_pin import remap_key  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CKPT = "/tmp/q3a_ckpt_tiny_aligner"
SEED = 3
TS = 151705
# (clip index, seconds, word ids: one list per word -- arbitrary ordinary vocabulary ids, no tokenizer needed)
CASES = [(0, 3.1, [[9707], [1879, 13], [40, 2776, 264]]),
         (1, 1.3, [[2610]]),
         (2, 5.0, [[785], [11], [3974, 17], [9906], [21, 22, 23], [1000]])]
SPLIT_TEXTS = ["Hello, world!  It's 2024.", "你好，世界！ ok-go", "don't  stop\tbelievin'", "数字123和abc混合", "  ", "¡Hola! ¿Qué tal? Ça va.",
               "a'b ''  x", "Ελληνικά και русский 42", "tab\tsep\nnew line", "１２３ ｆｕｌｌ"]
FIX_SEQS = [[0, 80, 160, 240], [0, 160, 80, 240], [0, 400, 80, 160, 240], [0, 400, 480, 80, 160, 240, 320],
            [800, 0, 80, 160], [800, 720, 0, 80, 160, 240], [0, 80, 160, 40], [0, 80, 160, 240, 40, 40],
            [160, 160, 160, 160], [500, 400, 300, 200, 100], [0, 80, 960, 880, 800, 720, 400, 480],
            [240, 0, 80, 640, 560, 480, 400, 160, 320], [80], [0, 1000, 2000, 10, 20, 30, 40, 3000],
            [320, 240, 160, 80, 0, 400, 480, 560]]


def align_prompt(T, words):
    ids = [151669] + [O.AUDIO_PAD_TOKEN_ID] * T + [151670]
    for w in words:
        ids += list(w) + [TS, TS]
    return ids


def load_hf(model_dir):
    from transformers import Qwen3ASRConfig, Qwen3ASRForTokenClassification
    cfg = O.AsrConfig.from_file(os.path.join(model_dir, "config.json"))
    with open(os.path.join(model_dir, "config.json")) as f:
        classify_num = json.load(f)["thinker_config"]["classify_num"]
    a, t = cfg.audio, cfg.text
    hf_cfg = Qwen3ASRConfig(
        audio_config=dict(num_mel_bins=a.num_mel_bins, encoder_layers=a.encoder_layers,
                          encoder_attention_heads=a.encoder_attention_heads, encoder_ffn_dim=a.encoder_ffn_dim,
                          d_model=a.d_model, n_window=a.n_window, n_window_infer=a.n_window_infer,
                          output_dim=a.output_dim, downsample_hidden_size=a.downsample_hidden_size),
        text_config=dict(model_type="qwen3", vocab_size=t.vocab_size, hidden_size=t.hidden_size,
                         intermediate_size=t.intermediate_size, num_hidden_layers=t.num_hidden_layers,
                         num_attention_heads=t.num_attention_heads, num_key_value_heads=t.num_key_value_heads,
                         head_dim=t.head_dim, rms_norm_eps=t.rms_norm_eps, max_position_embeddings=65536,
                         rope_parameters={"rope_type": "default", "rope_theta": t.rope_theta},
                         tie_word_embeddings=False, attention_bias=False),
        tie_word_embeddings=False, timestamp_token_id=TS, num_labels=classify_num)
    hf_cfg._attn_implementation = "eager"
    model = Qwen3ASRForTokenClassification(hf_cfg).to(torch.float32).eval()
    assert tuple(model.score.weight.shape) == (classify_num, t.hidden_size) and model.score.bias is None
    weights = O.load_model_weights(model_dir)
    sd = {}
    for k, v in weights.items():
        hk = "score.weight" if k == "thinker.lm_head.weight" else remap_key(k)
        sd[hk] = v
    missing, unexpected = model.load_state_dict(sd, strict=False)
    missing = [m for m in missing if "positional_embedding" not in m]
    assert not missing and not unexpected, (missing, unexpected)
    return model, cfg


@torch.no_grad()
def hf_align(model, cfg, clip, words):
    mel = O.WhisperFeatureExtractor(400, 160, cfg.audio.num_mel_bins, 16000).extract(clip)
    F_ = mel.shape[1]
    chunk = cfg.audio.n_window * 2
    Fp = (F_ + chunk - 1) // chunk * chunk
    feats = torch.zeros(1, mel.shape[0], Fp)
    feats[0, :, :F_] = mel
    mask = torch.zeros(1, Fp, dtype=torch.long)
    mask[0, :F_] = 1
    T = model.model.get_audio_features(feats, mask, return_dict=True).pooler_output.shape[0]
    ids = align_prompt(T, words)
    out = model(input_ids=torch.tensor([ids]), input_features=feats, input_features_mask=mask)
    rows = [i for i, x in enumerate(ids) if x == TS]
    return np.array(ids, dtype=np.int64), out.logits[0, rows].numpy()


def main():
    synthetic.write_checkpoint(CKPT, preset="tiny_aligner", seed=SEED)
    model, cfg = load_hf(CKPT)
    out = {}
    for n, (ci, sec, words) in enumerate(CASES):
        ids, lg = hf_align(model, cfg, synthetic.synthetic_clip(ci, sec), words)
        top = torch.from_numpy(lg).topk(4, dim=-1)
        out[f"c{n}_ids"] = ids
        out[f"c{n}_logits_q"] = lg[:, ::13].astype(np.float32)
        out[f"c{n}_top_idx"] = top.indices.numpy().astype(np.int64)
        out[f"c{n}_top_val"] = top.values.numpy().astype(np.float32)
        out[f"c{n}_classes"] = lg.argmax(-1).astype(np.int64)
        print(f"case {n}: P {len(ids)} markers {lg.shape[0]} classes {out[f'c{n}_classes'].tolist()}")
    np.savez_compressed(os.path.join(HERE, "hf_align_pin.npz"), **out)

    from transformers.models.qwen3_asr import processing_qwen3_asr as P
    split = P.Qwen3ASRProcessor.split_words_for_alignment
    host = {"split": [[t, split(None, t)] for t in SPLIT_TEXTS],
            "fix": [[s, P._fix_timestamps(np.array(s, dtype=np.float32))] for s in FIX_SEQS]}
    with open(os.path.join(HERE, "hf_align_host_pin.json"), "w") as f:
        json.dump(host, f, ensure_ascii=False, indent=0)


if __name__ == "__main__":
    main()
