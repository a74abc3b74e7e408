"""GPU tests (pytest -m gpu) of the decoder projection biases (q/k/v/o, gate/up/down) and of the decode attention's split partials.

Biases: the checkpoints of tests/bias_ref.py carry all seven, std 0.1.  (i) The whole path against the fp32 oracle
(tests/test_gpu_parity.py _stage_check) in the precise mode on every decode form the dispatcher picks, and in the default mode;
(ii) each default-mode prefill launch that adds a bias -- q and the K / V cache rows of the qkv GEMM (fused QK-norm + RoPE + append
epilogue of gemm256, or the separate kernel after gemm16 / gemm256), the SwiGLU output, the o and down residual epilogues --
against its fp64 reference on the launch's own tapped input, at layer 0 and the last layer.  tests/test_bias_host.py shows every
bias mistake moves the compared quantity by at least 5x the tolerance used here.

Split partials: the o_proj GEMV of a one-sequence decode step merges the attention's key splits from 16-byte loads of each
head's statistics; with poison_attn_partials every entry no attention launch wrote is NaN, so a merge that reads one shows."""
import numpy as np
import pytest

from oracle import q3asr_oracle as O
from qwen3_asr_rs_amd import _lib, synthetic
from qwen3_asr_rs_amd.engine import HipEngine

import bias_ref as BR
from test_gpu_parity import _stage_check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny_bias_dir():
    return BR.write("tiny")


@pytest.fixture(scope="module")
def tiny_untied_bias_dir():
    return BR.write("tiny_untied")


@pytest.fixture(scope="module")
def bias_0p6b_dir():
    return BR.write("0.6b")


def _knobs(lib, **kv):
    for k, v in kv.items():
        assert lib.q3a_debug_set(k.encode(), int(v)) == 0, k


DEFAULT_KNOBS = dict(gemm256_min_tiles=128, fuse_qkrope=1, skinny_q=1, skinny_glu_hp3=1, dattn_batched_min_wgs=128, layer_taps=0,
                     poison_attn_partials=0)


def test_bias_stage_parity_precise_every_decode_form(tiny_bias_dir):
    """Precise mode, exact ids: 1 and 2 sequences (the GEMV path: norm-fused qkv GEMV, o_proj GEMV with the split merge in front,
    mode-2 gate/up), 3 and 5 (the skinny path with fp32 activations), 40 (a group of 32 and a group of 8).  (The quarter
    workgroups and the half-pair gate/up form read bf16 activations: they exist in the default mode only, test_bias_at_0p6b_dims.)"""
    clips = [synthetic.synthetic_clip(400 + i, 1.1 + 0.29 * (i % 7)) for i in range(40)]
    for B in (1, 2, 3, 5, 40):
        _stage_check(tiny_bias_dir, clips[:B], True, steps=3)


def test_bias_stage_parity_default_mode(tiny_bias_dir, tiny_untied_bias_dir):
    """Default mode (bf16 activations, fused qkv epilogue forced on): the stage tolerances catch the gross index mistakes
    (a dropped v / o / down bias, gate and up swapped: tests/bias_ref.py CLAIMS)."""
    lib = _lib.load()
    clips = [synthetic.synthetic_clip(0, 9.3), synthetic.synthetic_clip(1, 2.17), synthetic.synthetic_clip(2, 4.0)[:63999]]
    try:
        _stage_check(tiny_bias_dir, clips[:1], False)
        for fuse in (1, 0):
            _knobs(lib, gemm256_min_tiles=0, fuse_qkrope=fuse)
            _stage_check(tiny_bias_dir, clips, False)
        _stage_check(tiny_untied_bias_dir, clips, False)
    finally:
        _knobs(lib, **DEFAULT_KNOBS)


def _bf16(raw: np.ndarray) -> np.ndarray:
    return (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def _launch_check(model_dir, clips, layers=None):
    """Default mode, one prefill with the layer taps on: every biased launch of the checked layers against its fp64 reference
    (tests/bias_ref.py) on the engine's own input of that launch.  Worst per-row rel-L2 per launch kind."""
    orc_cfg = O.AsrConfig.from_file(model_dir + "/config.json")
    weights = O.load_model_weights(model_dir)
    tc = orc_cfg.text
    H, QD, I, nkv = tc.hidden_size, tc.num_attention_heads * tc.head_dim, tc.intermediate_size, tc.num_key_value_heads
    nq = tc.num_attention_heads
    eng = HipEngine(model_dir, 0, debug_taps=True, max_new_tokens=8)
    try:
        eng.mel(clips)
        eng.encode()
        prompts = [HipEngine.build_prompt(eng.num_audio_tokens(len(c))) for c in clips]
        eng.prefill(prompts)
        P = [len(p) for p in prompts]
        T = sum(P)
        pos = np.concatenate([np.arange(p) for p in P])
        cos, sin = BR.rope_tables(orc_cfg, max(P))
        cos, sin = cos[pos], sin[pos]
        L = tc.num_hidden_layers
        worst = {k: 0.0 for k in BR.LAUNCH_REL}
        for li in (layers if layers is not None else (0, L - 1)):
            tap = lambda w: eng.debug_read_raw(f"L{li:02d}_{w}")
            inp = dict(ln1=_bf16(tap("ln1")).reshape(T, H), attn=_bf16(tap("attn")).reshape(T, QD),
                       ln2=_bf16(tap("ln2")).reshape(T, H), act=_bf16(tap("act")).reshape(T, I),
                       o=tap("o").view(np.float32).reshape(T, H),
                       resid=(eng.debug_read("dec_embed") if li == 0 else eng.debug_read_raw(f"L{li - 1:02d}_x").view(np.float32)).reshape(T, H))
            got = {"q": _bf16(tap("q")).reshape(T, nq, tc.head_dim), "o": inp["o"], "act": inp["act"],
                   "x": tap("x").view(np.float32).reshape(T, H)}
            for kv in ("k", "v"):  # cache [sequence][kv head][max_ctx][128]: the prompt rows of every sequence
                c = _bf16(tap(kv)).reshape(len(P), nkv, -1, tc.head_dim)
                got[kv] = np.concatenate([c[s, :, :P[s]].transpose(1, 0, 2) for s in range(len(P))])
            want = BR.launch_outputs(inp, BR.layer_weights(weights, li), orc_cfg, cos, sin)
            for k in BR.LAUNCH_REL:
                g, w = got[k].reshape(T, -1).astype(np.float64), want[k].reshape(T, -1)
                assert np.isfinite(g).all(), (li, k)
                row = np.linalg.norm(g - w, axis=1) / (np.linalg.norm(w, axis=1) + 1e-30)
                worst[k] = max(worst[k], float(row.max()))
        for k, tol in BR.LAUNCH_REL.items():
            assert worst[k] <= tol, (k, worst)
        return worst
    finally:
        eng.close()


@pytest.mark.parametrize("qkv_form", ["gemm256_fused", "gemm256_rope_kernel", "gemm16_rope_kernel"])
def test_bias_prefill_launches_against_fp64(tiny_bias_dir, tiny_untied_bias_dir, qkv_form):
    """7 ragged prompts (the last 256-row tile partial), GQA 2 and 4: q, K / V cache rows, SwiGLU output, o and down residual
    epilogues of layer 0 and the last layer, with the qkv projection as the fused gemm256 epilogue, as gemm256 + the separate
    QK-norm / RoPE / append kernel, or as gemm16 + that kernel (gemm16 also takes the other projections then)."""
    lib = _lib.load()
    clips = [synthetic.synthetic_clip(60 + i, 2.0 + 0.53 * i) for i in range(7)]
    try:
        _knobs(lib, layer_taps=1, gemm256_min_tiles=(1 << 30) if qkv_form == "gemm16_rope_kernel" else 0,
               fuse_qkrope=int(qkv_form == "gemm256_fused"))
        for d in (tiny_bias_dir, tiny_untied_bias_dir):
            _launch_check(d, clips)
    finally:
        _knobs(lib, **DEFAULT_KNOBS)


def _teacher_forced(model_dir, clips, refs, precise, steps):
    """Prefill + teacher-forced decode steps through the stage API: [(logits, ids)] per step."""
    eng = HipEngine(model_dir, 0, precise=precise, max_new_tokens=8)
    try:
        eng.mel(clips)
        eng.encode()
        logits, nxt = eng.prefill([HipEngine.build_prompt(r.num_audio_tokens) for r in refs])
        out = [(logits.copy(), nxt.copy())]
        for s in range(steps - 1):
            eng.set_next_tokens([r.all_step_ids[s] for r in refs])
            lg, nx, _ = eng.decode_step()
            out.append((lg.copy(), nx.copy()))
        return out
    finally:
        eng.close()


def test_bias_at_0p6b_dims(bias_0p6b_dir):
    """0.6B dimensions with all seven biases.  (i) Prefill launches against fp64: 32 prompts with gemm256 forced on (the fused
    QK-norm + RoPE + append qkv epilogue, gate/up, o and down at their real widths and tile seams), and one 30 s prompt on the
    dispatcher's own choice (gemm16).  (ii) Teacher-forced logits against the oracle: precise mode, exact ids, one sequence (the
    XL norm-fused GEMV, the o_proj GEMV with the merge in front) and three (skinny path, fp32 activations); default mode, one
    sequence and five, the five with gate/up as pairs and as half pairs (skinny_glu_hp3 0 / 2) and o / down as full and quarter
    workgroups (skinny_q 0 / 1) -- forms that read bf16 activations and exist in the default mode only.  Default-mode logits
    within twice the stage tolerance (as test_parity_0p6b_dims_batch3_skinny_decode), ids exact wherever the oracle's top-1 /
    top-2 margin exceeds twice the error; the exact bits of these forms are held by the bit-identity tests of test_gpu_parity."""
    lib = _lib.load()
    try:
        _knobs(lib, layer_taps=1, gemm256_min_tiles=0, fuse_qkrope=1)
        _launch_check(bias_0p6b_dir, [synthetic.synthetic_clip(450 + i, 2.0 + 0.07 * i) for i in range(32)])
        _knobs(lib, gemm256_min_tiles=128)
        _launch_check(bias_0p6b_dir, [synthetic.synthetic_clip(0, 30.0)], layers=(0,))
        _knobs(lib, layer_taps=0)
        orc = O.AsrOracle(bias_0p6b_dir)
        clips = [synthetic.synthetic_clip(3 + i, 1.2 + 0.47 * i) for i in range(5)]
        steps = 3
        refs = [orc.transcribe_ids(c, fixed_new_tokens=steps, last_only=True) for c in clips]
        legs = [(True, 1, 1, 1), (True, 3, 1, 1), (False, 1, 1, 1), (False, 5, 0, 1), (False, 5, 2, 1), (False, 5, 0, 0)]
        for precise, B, hp3, q in legs:
            _knobs(lib, skinny_glu_hp3=hp3, skinny_q=q)
            tol = 2e-4 if precise else 2 * 6e-2
            out = _teacher_forced(bias_0p6b_dir, clips[:B], refs[:B], precise, steps)
            for s, (lg, nx) in enumerate(out):
                for b in range(B):
                    ref = refs[b].step_logits[s]
                    err = float(np.abs(lg[b] - ref.numpy()).max())
                    assert err <= tol, (precise, B, hp3, q, s, b, err)
                    top = ref.topk(2).values
                    if precise or float(top[0] - top[1]) > 2 * err:
                        assert int(nx[b]) == refs[b].all_step_ids[s], (precise, B, hp3, q, s, b)
    finally:
        _knobs(lib, **DEFAULT_KNOBS)


# ---- stale split partials ------------------------------------------------------------------------------------------------
def _poison_run(model_dir, clips, precise, forced, max_new):
    """Stage API: prefill, then len(forced) teacher-forced decode steps reading logits; ids of the whole (graph-replayed) path."""
    eng = HipEngine(model_dir, 0, precise=precise, max_new_tokens=max_new)
    try:
        eng.mel(clips)
        eng.encode()
        logits, nxt = eng.prefill([HipEngine.build_prompt(eng.num_audio_tokens(len(c))) for c in clips])
        out = [logits.copy(), nxt.copy()]
        for s in range(len(forced)):
            eng.set_next_tokens(forced[s])
            lg, nx, _ = eng.decode_step()
            out += [lg.copy(), nx.copy()]
        ids = eng.transcribe_batch(clips, None, max_new=len(forced) + 1, fixed_new_tokens=len(forced) + 1)
        return out, ids
    finally:
        eng.close()


def test_stale_split_partials_do_not_enter_the_merge(tiny_bias_dir):
    """max_new_tokens 1024 reserves up to 9 key splits per head; the live count follows the context.  Contexts of 1..8 live splits
    (the merge-first o_proj GEMV, 4 and 8 splits per load round) and one of 9 (its chunked merge), one sequence and two (the
    chunked merge of the GEMV path), five with key splits + the merge launch: with every unwritten partial NaN
    (poison_attn_partials), ids and logits are bit-identical to the run without poison, and in the precise mode the ids are
    the oracle's."""
    lib = _lib.load()
    orc = O.AsrOracle(tiny_bias_dir)
    eng = HipEngine(tiny_bias_dir, 0, max_new_tokens=8)
    secs = [3.0, 14.0, 24.0, 33.5, 43.0, 53.0, 63.0, 73.0, 83.0]
    P = [len(HipEngine.build_prompt(eng.num_audio_tokens(int(s * 16000)))) for s in secs]
    eng.close()
    assert sorted({(p + 3) // 128 + 1 for p in P}) == list(range(1, 10)), P   # live splits at the decode steps below
    steps = 3
    cases = [[synthetic.synthetic_clip(600 + i, s)] for i, s in enumerate(secs)]
    cases += [[synthetic.synthetic_clip(610, 8.5), synthetic.synthetic_clip(611, 30.0)]]
    cases += [[synthetic.synthetic_clip(620 + i, 3.0 + 9.0 * i) for i in range(5)]]   # 1..5 live splits
    try:
        _knobs(lib, dattn_batched_min_wgs=1 << 30)
        for clips in cases:
            refs = [orc.transcribe_ids(c, fixed_new_tokens=steps + 1, last_only=True) for c in clips]
            forced = [[r.all_step_ids[s] for r in refs] for s in range(steps)]
            for precise in (True, False):
                got = {}
                for poison in (0, 1):
                    _knobs(lib, poison_attn_partials=poison)
                    got[poison] = _poison_run(tiny_bias_dir, clips, precise, forced, 1024)
                for a, b in zip(got[0][0], got[1][0]):
                    assert np.isfinite(a).all() and np.array_equal(a, b), (len(clips), precise)
                assert got[0][1] == got[1][1], (len(clips), precise)
                if precise:
                    assert got[1][1] == [r.all_step_ids[:steps + 1] for r in refs], [len(c) for c in clips]
                    for s in range(steps + 1):
                        assert [int(t) for t in got[1][0][2 * s + 1]] == [r.all_step_ids[s] for r in refs], (len(clips), s)
    finally:
        _knobs(lib, **DEFAULT_KNOBS)
