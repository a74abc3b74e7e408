"""Decoder projection biases (q/k/v/o, gate/up/down: optional in the reference's Linear::load): the checkpoints that carry
them, fp64 references of the prefill launches that add them, and the index mistakes those launches could make.
Shared by tests/test_bias_host.py (CPU) and tests/test_gpu_bias.py (GPU)."""
import math

import numpy as np
import torch

from oracle import q3asr_oracle as O
from qwen3_asr_rs_amd import synthetic

BIAS_STD = 0.1
# name -> (directory, write_checkpoint arguments): the conftest checkpoints of the same seeds, plus all seven decoder biases
CHECKPOINTS = {
    "tiny": ("/tmp/q3a_ckpt_tiny_bias", dict(preset="tiny", seed=1)),                                 # GQA 2
    "tiny_untied": ("/tmp/q3a_ckpt_tiny_untied_bias", dict(preset="tiny_untied", seed=2, shards=3)),  # GQA 4, untied lm_head
    "0.6b": ("/tmp/q3a_ckpt_0p6b_bias", dict(preset="0.6b", seed=0, embed_scale=synthetic.PEAKED_EMBED_SCALE)),
}

# The GPU checks and their tolerances (tests/test_gpu_bias.py).  STAGE: _stage_check's rel-L2 of the layer-0 output per mode
# (precise 1e-4, default 2e-2: tests/test_gpu_parity.py TOL).  LAUNCH: rel-L2 of one default-mode prefill launch's output
# against the fp64 reference on the launch's own bf16 input, per row -- bf16 outputs (q, K / V cache rows, SwiGLU) are rounded
# once (at most 2^-8 = 3.9e-3 relative per element, hence per row; 1.5-2.2e-3 measured), fp32 outputs (the o / down residual
# epilogues) only see fp32 summation.
STAGE_REL = {"precise": 1e-4, "default": 2e-2}
LAUNCH_REL = {"q": 4.5e-3, "k": 4.5e-3, "v": 4.5e-3, "act": 4.5e-3, "o": 1e-4, "x": 1e-4}
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def write(name: str) -> str:
    d, kw = CHECKPOINTS[name]
    return synthetic.write_checkpoint(d, dec_bias="all", dec_bias_std=BIAS_STD, **kw)


def _key(li: int, proj: str) -> str:
    return f"thinker.model.layers.{li}.{'mlp' if proj in ('gate_proj', 'up_proj', 'down_proj') else 'self_attn'}.{proj}.bias"


# ---- mutations: what a kernel that picks the wrong bias element computes ---------------------------------------------
def mutate(weights: dict, name: str, n_layers: int, head_dim: int = 128) -> dict:
    """A copy of the oracle's weight dict with one bias mistake in every decoder layer: "drop_<proj>" (bias ignored),
    "swap_gate_up", "roll_gate_16" (gate bias one 16-row block off: the gate/up interleave), "q_halves" / "k_halves" (the two
    RoPE halves of every head's q / k bias swapped: the partner index of the fused qkv epilogue)."""
    w = dict(weights)
    for li in range(n_layers):
        if name.startswith("drop_"):
            del w[_key(li, name[5:])]
        elif name == "swap_gate_up":
            w[_key(li, "gate_proj")], w[_key(li, "up_proj")] = weights[_key(li, "up_proj")], weights[_key(li, "gate_proj")]
        elif name == "roll_gate_16":
            w[_key(li, "gate_proj")] = torch.roll(weights[_key(li, "gate_proj")], 16)
        elif name in ("q_halves", "k_halves"):
            k = _key(li, name[0] + "_proj")
            w[k] = weights[k].reshape(-1, 2, head_dim // 2).flip(1).reshape(-1)
        else:
            raise KeyError(name)
    return w


MUTATIONS = tuple(f"drop_{p}" for p in PROJ) + ("swap_gate_up", "roll_gate_16", "q_halves", "k_halves")
# mutation -> the GPU checks that claim to catch it: "precise" / "default" (_stage_check), or a launch of LAUNCH_REL
CLAIMS = {
    "drop_q_proj": ("precise", "q"),
    "drop_k_proj": ("precise", "k"),
    "drop_v_proj": ("precise", "default", "v"),
    "drop_o_proj": ("precise", "default", "o"),
    "drop_gate_proj": ("precise", "act"),
    "drop_up_proj": ("precise", "act"),
    "drop_down_proj": ("precise", "default", "x"),
    "swap_gate_up": ("precise", "default", "act"),
    "roll_gate_16": ("precise", "act"),
    "q_halves": ("precise", "q"),
    "k_halves": ("precise", "k"),
}


# ---- fp64 references of the prefill launches -------------------------------------------------------------------------
def layer_weights(weights: dict, li: int) -> dict:
    p = f"thinker.model.layers.{li}"
    g = lambda k: weights[k].double().numpy() if k in weights else None
    w = {n: g(f"{p}.{'mlp' if n in ('gate_proj', 'up_proj', 'down_proj') else 'self_attn'}.{n}.weight") for n in PROJ}
    b = {n: g(_key(li, n)) for n in PROJ}
    return dict(w=w, b=b, k_norm=g(f"{p}.self_attn.k_norm.weight"), q_norm=g(f"{p}.self_attn.q_norm.weight"),
                ln1=g(f"{p}.input_layernorm.weight"), ln2=g(f"{p}.post_attention_layernorm.weight"))


def _lin(x, w, b):
    y = np.asarray(x, np.float64) @ w.T
    return y + b if b is not None else y


def rope_tables(cfg, n_pos: int):
    tc = cfg.text
    cos, sin = O.compute_mrope_cos_sin(O.build_position_ids(list(range(n_pos))), tc.head_dim, tc.rope_theta, tc.mrope_section,
                                       tc.mrope_interleaved)
    return cos.double().numpy(), sin.double().numpy()


def _norm_rope(x, norm_w, eps, cos, sin):  # x [rows, heads, hd]; cos / sin [rows, hd]
    x = x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * norm_w
    h = x.shape[-1] // 2
    rot = np.concatenate([-x[..., h:], x[..., :h]], -1)
    return x * cos[:, None] + rot * sin[:, None]


def ref_k(ln1, lw, cfg, cos, sin):
    """K cache rows [rows, n_kv, hd] = rope(k_norm(ln1 Wk^T + bk)) at the rows' positions (cos / sin per row)."""
    tc = cfg.text
    k = _lin(ln1, lw["w"]["k_proj"], lw["b"]["k_proj"]).reshape(len(ln1), tc.num_key_value_heads, tc.head_dim)
    return _norm_rope(k, lw["k_norm"], tc.rms_norm_eps, cos, sin)


def ref_q(ln1, lw, cfg, cos, sin):
    tc = cfg.text
    q = _lin(ln1, lw["w"]["q_proj"], lw["b"]["q_proj"]).reshape(len(ln1), tc.num_attention_heads, tc.head_dim)
    return _norm_rope(q, lw["q_norm"], tc.rms_norm_eps, cos, sin)


def ref_v(ln1, lw, cfg):
    tc = cfg.text
    return _lin(ln1, lw["w"]["v_proj"], lw["b"]["v_proj"]).reshape(len(ln1), tc.num_key_value_heads, tc.head_dim)


def ref_o(resid, attn, lw):
    return np.asarray(resid, np.float64) + _lin(attn, lw["w"]["o_proj"], lw["b"]["o_proj"])


def ref_act(ln2, lw):
    g = _lin(ln2, lw["w"]["gate_proj"], lw["b"]["gate_proj"])
    u = _lin(ln2, lw["w"]["up_proj"], lw["b"]["up_proj"])
    return g / (1.0 + np.exp(-g)) * u


def ref_x(o, act, lw):
    return np.asarray(o, np.float64) + _lin(act, lw["w"]["down_proj"], lw["b"]["down_proj"])


def rms_norm(x, w, eps):
    x = np.asarray(x, np.float64)
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * w


def layer_inputs(x, lw, cfg, cos, sin) -> dict:
    """One sequence through one decoder layer in fp64 (causal attention): the input of every launch the GPU checks take."""
    tc = cfg.text
    P = len(x)
    ln1 = rms_norm(x, lw["ln1"], tc.rms_norm_eps)
    q, k, v = ref_q(ln1, lw, cfg, cos, sin), ref_k(ln1, lw, cfg, cos, sin), ref_v(ln1, lw, cfg)
    rep = tc.num_attention_heads // tc.num_key_value_heads
    s = np.einsum("qhd,khd->hqk", q, np.repeat(k, rep, 1)) / math.sqrt(tc.head_dim)
    s = s + np.triu(np.full((P, P), -np.inf), 1)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    attn = np.einsum("hqk,khd->qhd", p, np.repeat(v, rep, 1)).reshape(P, -1)
    o = ref_o(x, attn, lw)
    ln2 = rms_norm(o, lw["ln2"], tc.rms_norm_eps)
    act = ref_act(ln2, lw)
    return dict(resid=np.asarray(x, np.float64), ln1=ln1, attn=attn, o=o, ln2=ln2, act=act, x=ref_x(o, act, lw))


def launch_outputs(inp: dict, lw, cfg, cos, sin) -> dict:
    """What each checked launch computes from its own input (inp: layer_inputs, or the engine's taps)."""
    return {"q": ref_q(inp["ln1"], lw, cfg, cos, sin), "k": ref_k(inp["ln1"], lw, cfg, cos, sin), "v": ref_v(inp["ln1"], lw, cfg),
            "o": ref_o(inp["resid"], inp["attn"], lw),
            "act": ref_act(inp["ln2"], lw), "x": ref_x(inp["o"], inp["act"], lw)}


def rel_l2(got, ref) -> float:
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    return float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30))
