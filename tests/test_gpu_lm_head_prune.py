"""GPU tests of the pruned one-sequence lm_head argmax (k_gemv.hip lm_head_approx_kernel / lm_head_rescore_kernel, knob
"lm_head_prune"): the ids must be bit-identical to the full bf16 GEMV (knob 0) over every generated step, on the benchmarked
checkpoint, on the tiny presets and on adversarial heads (exact ties, near-ties, thousands of equal rows), and the bound
|a_r - l_r| <= e_r of the int8 pre-pass must hold for every row of many decoder states."""
import os
import shutil

import numpy as np
import pytest

from qwen3_asr_rs_amd import _lib, synthetic
from qwen3_asr_rs_amd.engine import HipEngine

pytestmark = pytest.mark.gpu

STEPS = 48


def _set_prune(v: int):
    assert _lib.load().q3a_debug_set(b"lm_head_prune", v) == 0


@pytest.fixture(autouse=True)
def _restore_knob():
    yield
    _set_prune(1)


def _stats(eng) -> np.ndarray:
    return eng.debug_read_raw("lm_head_prune_stats").view(np.int32).copy()


def _ids_on_off(model_dir, clips, steps=STEPS):
    """ids with the knob on and off on ONE engine, and the candidate blocks per pruned pass seen with it on"""
    eng = HipEngine(model_dir, 0, max_new_tokens=steps + 8)
    try:
        _set_prune(0)
        off = eng.transcribe_batch(clips, None, max_new=steps, fixed_new_tokens=steps)
        s0 = _stats(eng)
        _set_prune(1)
        on = eng.transcribe_batch(clips, None, max_new=steps, fixed_new_tokens=steps)
        s1 = _stats(eng)
        _set_prune(0)
        off2 = eng.transcribe_batch(clips, None, max_new=steps, fixed_new_tokens=steps)
        s2 = _stats(eng)
    finally:
        eng.close()
    assert (s0 == 0).all() and (s2 == s1).all(), (s0, s1, s2)  # knob 0 never runs the pruned passes
    assert on == off == off2
    return on, s1


def _check_pruned(model_dir, clips, min_per_pass=None):
    ids, st = _ids_on_off(model_dir, clips)
    blocks, passes = int(st[0]), int(st[1])
    if len(clips) == 1:
        assert STEPS - 1 <= passes <= STEPS + 1, st  # prefill + the decode steps
        per = blocks / passes
        print(f"{os.path.basename(model_dir)}: {per:.2f} candidate blocks per step")
        assert per >= 1.0
        if min_per_pass is not None:
            assert per > min_per_pass, per
    else:
        assert passes == 0, st  # two sequences keep the full GEMV
    return ids


def test_prune_ids_0p6b_one_and_two_clips():
    d = synthetic.write_checkpoint("/tmp/q3a_ckpt_0p6b_peaked", "0.6b", seed=0, embed_scale=synthetic.PEAKED_EMBED_SCALE)
    clips = [synthetic.synthetic_clip(0, 30.0), synthetic.synthetic_clip(1, 30.0)]
    _check_pruned(d, clips[:1])
    _check_pruned(d, clips)


def test_prune_ids_tiny(tiny_dir):
    _check_pruned(tiny_dir, [synthetic.synthetic_clip(0, 9.3)])


def test_prune_ids_tiny_untied(tiny_untied_dir):
    _check_pruned(tiny_untied_dir, [synthetic.synthetic_clip(1, 9.3)])


def _adversarial_copy(src, dst):
    if os.path.exists(dst):
        shutil.rmtree(dst)
    shutil.copytree(src, dst)
    return dst


def _winner(model_dir, clip):
    """the token the unpruned head picks most often on this clip"""
    _set_prune(0)
    eng = HipEngine(model_dir, 0, max_new_tokens=STEPS + 8)
    try:
        ids = eng.transcribe_batch([clip], None, max_new=STEPS, fixed_new_tokens=STEPS)[0]
    finally:
        eng.close()
    _set_prune(1)
    vals, counts = np.unique(ids, return_counts=True)
    return int(vals[np.argmax(counts)])


@pytest.mark.parametrize("case", ["ties", "near_ties", "thousands"])
def test_prune_adversarial_heads(tiny_untied_dir, case):
    d = _adversarial_copy(tiny_untied_dir, f"/tmp/q3a_ckpt_prune_{case}")
    clip = synthetic.synthetic_clip(1, 9.3)
    key = synthetic.output_embedding_key(d)
    w = _winner(d, clip)
    head = synthetic.read_tensor(d, key).astype(np.float32)
    V = head.shape[0]
    row = head[w].copy()
    if case == "ties":  # the winning row again at lower and higher indices, in other blocks and inside its own
        targets = sorted({3, 17, max(0, w - 40), w ^ 1, min(V - 1, w + 40), V - 20, V - 1} - {w})
        for r in targets:
            head[r] = row
    elif case == "near_ties":  # the winning row with one element moved by one bf16 ulp, up and down, spread over the vocabulary
        rng = np.random.default_rng(5)
        targets = sorted(set(rng.choice(V, 64, replace=False).tolist()) - {w})
        for j, r in enumerate(targets):
            v = row.copy()
            k = int(rng.integers(len(v)))
            bits = int(np.float32(v[k]).view(np.uint32)) >> 16
            if bits & 0x7FFF:
                bits += 1 if j % 2 else -1
            v[k] = np.uint32(bits << 16).view(np.float32)
            head[r] = v
    else:  # 4000 equal rows, one per 16-row block: pass 2 must rescore thousands of blocks
        targets = [16 * j + (j % 16) for j in range(4000) if 16 * j + (j % 16) != w]
        head[targets] = row
    synthetic.overwrite_tensor(d, key, head)
    ids, st = _ids_on_off(d, [clip])
    per = st[0] / st[1]
    print(f"{case}: winner {w}, {per:.1f} candidate blocks per step, ids {ids[0][:8]}...")
    assert per > 1.0
    if case == "thousands":
        assert per > 1000


def _bound_check(model_dir, n_steps, seed, seconds):
    rng = np.random.default_rng(seed)
    eng = HipEngine(model_dir, 0, debug_taps=True, max_new_tokens=n_steps + 8)
    worst = 0.0
    try:
        clip = synthetic.synthetic_clip(seed, seconds)
        eng.mel([clip])
        eng.encode()
        logits, _ = eng.prefill([HipEngine.build_prompt(eng.num_audio_tokens(len(clip)))])
        V = eng.dims.vocab_size
        for s in range(n_steps + 1):
            if s > 0:
                eng.set_next_tokens([int(rng.integers(V))])  # random history: many decoder states
                logits, _, _ = eng.decode_step(True)
            ab = eng.debug_read("lm_head_bound").reshape(V, 2).astype(np.float64)
            l = logits[0].astype(np.float64)
            err = np.abs(ab[:, 0] - l)
            assert np.isfinite(ab).all()
            bad = np.nonzero(err > ab[:, 1])[0]
            assert len(bad) == 0, (s, bad[:8], err[bad[:8]], ab[bad[:8], 1])
            worst = max(worst, float((err / ab[:, 1]).max()))
    finally:
        eng.close()
    print(f"{os.path.basename(model_dir)}: largest |a - l| / e over {n_steps + 1} states: {worst:.4f}")
    return worst


def test_prune_bound_tiny(tiny_dir):
    assert _bound_check(tiny_dir, 40, 3, 9.3) <= 1.0


def test_prune_bound_0p6b():
    d = synthetic.write_checkpoint("/tmp/q3a_ckpt_0p6b_peaked", "0.6b", seed=0, embed_scale=synthetic.PEAKED_EMBED_SCALE)
    assert _bound_check(d, 24, 4, 30.0) <= 1.0
