"""Decoder projection biases on the CPU: the fixture option leaves every other checkpoint as it was, and each bias mistake a
kernel could make moves the quantity its GPU check compares by at least 5x that check's tolerance (tests/bias_ref.py CLAIMS),
so the GPU checks of tests/test_gpu_bias.py can fail -- at this bias scale, with these tolerances."""
import os

import numpy as np
import pytest
import torch

from oracle import q3asr_oracle as O
from qwen3_asr_rs_amd import synthetic

import bias_ref as BR


@pytest.fixture(scope="module")
def tiny_bias_dir():
    return BR.write("tiny")


def test_bias_option_adds_only_the_bias_tensors(tiny_dir, tiny_bias_dir):
    """The biases are drawn after every other tensor: the rest of the checkpoint is the conftest one of the same seed, byte
    for byte; with the option off the writer's output (and directory tag) is unchanged -- the committed goldens check that."""
    plain = synthetic.tensor_specs(synthetic.CONFIG_TINY)
    with_b = synthetic.tensor_specs(synthetic.CONFIG_TINY, dec_bias="all")
    assert with_b[:len(plain)] == plain and len(with_b) == len(plain) + 7 * 2
    assert {k for k, *_ in synthetic.tensor_specs(synthetic.CONFIG_TINY, dec_bias="attn")[len(plain):]} == \
        {f"thinker.model.layers.{i}.self_attn.{p}_proj.bias" for i in range(2) for p in "qkvo"}
    a, b = O.load_model_weights(tiny_dir), O.load_model_weights(tiny_bias_dir)
    assert set(b) - set(a) == {BR._key(i, p) for i in range(2) for p in BR.PROJ}
    for k in a:
        assert torch.equal(a[k], b[k]), k
    std = float(torch.cat([b[BR._key(i, p)] for i in range(2) for p in BR.PROJ]).std())
    assert 0.09 < std < 0.11, std
    assert os.listdir(tiny_dir) != os.listdir(tiny_bias_dir)   # a directory tag of its own


@torch.no_grad()
def test_bias_mutations_exceed_the_gpu_tolerances(tiny_bias_dir):
    """Each mutation of tests/bias_ref.py applied to the oracle's weights: (i) the layer-0 output of the prefill moves by at
    least 5x the stage check's rel-L2 in every mode that claims it; (ii) the output of the one launch that claims it, on the
    launch's correct input, moves by at least 5x the launch check's rel-L2.  Keeps the GPU checks honest if a bias scale or a
    tolerance changes."""
    orc = O.AsrOracle(tiny_bias_dir)
    cfg = orc.cfg
    clip = synthetic.synthetic_clip(2, 4.0)
    ref = orc.transcribe_ids(clip, fixed_new_tokens=1, want_taps=True)
    x0 = ref.taps["dec_embed"].double().numpy()
    cos, sin = BR.rope_tables(cfg, len(x0))
    lw = BR.layer_weights(orc.weights, 0)
    inp = BR.layer_inputs(x0, lw, cfg, cos, sin)
    # the fp64 layer is the oracle's layer (fp32): the references the launch checks use are the network's
    assert BR.rel_l2(inp["x"], ref.taps["dec_layer0"].numpy()) < 1e-5
    want = BR.launch_outputs(inp, lw, cfg, cos, sin)
    saved = orc.weights
    effects = {}
    try:
        for name in BR.MUTATIONS:
            orc.weights = BR.mutate(saved, name, cfg.text.num_hidden_layers)
            got = orc.transcribe_ids(clip, fixed_new_tokens=1, want_taps=True)
            mut = BR.launch_outputs(inp, BR.layer_weights(orc.weights, 0), cfg, cos, sin)
            effects[name] = dict(stage=BR.rel_l2(got.taps["dec_layer0"], ref.taps["dec_layer0"]),
                                 logit=float((got.step_logits[0] - ref.step_logits[0]).abs().max()),
                                 **{k: BR.rel_l2(mut[k], want[k]) for k in BR.LAUNCH_REL})
    finally:
        orc.weights = saved
    for name, claims in BR.CLAIMS.items():
        e = effects[name]
        for c in claims:
            if c in BR.STAGE_REL:
                assert e["stage"] >= 5 * BR.STAGE_REL[c], (name, c, e)
            else:
                assert e[c] >= 5 * BR.LAUNCH_REL[c], (name, c, e)


def test_fp64_launch_references_match_the_oracle_on_a_gqa4_bias_checkpoint():
    """tiny_untied with biases (GQA 4, contiguous mrope map): the fp64 layer of tests/bias_ref.py is the oracle's layer 0."""
    orc = O.AsrOracle(BR.write("tiny_untied"))
    r = orc.transcribe_ids(synthetic.synthetic_clip(3, 1.7), fixed_new_tokens=1, want_taps=True)
    x0 = r.taps["dec_embed"].double().numpy()
    cos, sin = BR.rope_tables(orc.cfg, len(x0))
    inp = BR.layer_inputs(x0, BR.layer_weights(orc.weights, 0), orc.cfg, cos, sin)
    assert BR.rel_l2(inp["x"], r.taps["dec_layer0"].numpy()) < 1e-5
