"""Scoring a given transcript on the GPU (q3a_score, q3a_score_batch_ptrs): per-token log-probabilities in one prefill.

The lm_head at the rows that predict the transcript reduces in its epilogue (k_align.hip: one (max, first index, log-sum) partial per
row and 64-column strip, the target's accumulator through a single writer, one wave per row merging the partials).  Checked here:
the reduction against float64 log_softmax of the engine's own logits in both modes and on a head whose every logit has a twin, the
values against the fp32 oracle (tiny, 32 ragged clips; the 0.6B dimensions), agreement with the decode path's token
log-probabilities, the refusals and the engine's state afterwards, the CLI's Score line, and that one scoring call costs less than
the decode loop that was the only way to these numbers before."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import q3asr_oracle as O
from qwen3_asr_rs_amd import synthetic
from qwen3_asr_rs_amd.engine import AsrInference, HipEngine, Q3aError
from score_ref import AUDIO_PAD, EOS, V, oracle_score, perturb, ragged_lens, reduce_logits

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_audio")


def _clips32(n=32):
    return [synthetic.synthetic_clip(300 + i, 1.0 + 0.25 * (i % 7)) for i in range(n)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(x[k]), _bits(y[k])) for x, y in zip(a, b) for k in range(3))


def _stage_score(eng, clips, targets, want_logits=True, prefix=None):
    eng.mel(clips)
    eng.encode()
    return eng.score([HipEngine.build_prompt(t, prefix) for t in eng._T], targets, want_logits=want_logits)


def _arith_targets(B):
    """Ragged lengths 3, 8, 13, 4, ... with arbitrary ids; utterance 0 holds id 0 and an id of the last 64-column strip."""
    out = []
    for b, n in enumerate(ragged_lens(B)):
        t = [((b * 131 + i * 7919 + 17) * 48271 + 12345) % V for i in range(n)]
        out.append([x + 1 if x == AUDIO_PAD else x for x in t])
    out[0][0], out[0][1] = 0, V - 3
    return out


@pytest.fixture(scope="module")
def twin_rows_dir(tiny_untied_dir):
    """The untied tiny checkpoint with lm_head rows V/2 .. V-1 replaced by rows 0 .. V/2-1 (as test_gpu_logprobs.py builds it, in a
    directory of its own): every logit has an exact twin in another strip, tile and partial."""
    d = "/tmp/q3a_ckpt_score_twin_rows"
    if os.path.exists(d):
        shutil.rmtree(d)
    shutil.copytree(tiny_untied_dir, d)
    key = synthetic.output_embedding_key(d)
    head = synthetic.read_tensor(d, key).astype(np.float32)
    h = head.shape[0] // 2
    head[h:] = head[:h]
    synthetic.overwrite_tensor(d, key, head)
    return d


@pytest.mark.parametrize("head", ["tiny", "twin_rows"])
@pytest.mark.parametrize("B", [1, 5, 32])
@pytest.mark.parametrize("precise", [False, True])
def test_reduction_matches_log_softmax_of_the_engines_logits(request, precise, B, head):
    d = request.getfixturevalue("tiny_dir" if head == "tiny" else "twin_rows_dir")
    clips, targets = _clips32(B), _arith_targets(B)
    M = sum(len(t) for t in targets)
    assert M % 64 != 0 and (B < 32 or M == 210)
    eng = HipEngine(d, 0, precise=precise, max_new_tokens=16)
    res, logits = _stage_score(eng, clips, targets)
    again, logits2 = _stage_score(eng, clips, targets)
    plain = _stage_score(eng, clips, targets, want_logits=False)
    eng.close()
    assert logits.shape == (M, V)
    assert _same(res, again) and np.array_equal(_bits(logits), _bits(logits2)), "a second run differs"
    assert _same(res, plain), "results differ without logits_out"
    worst, k = 0.0, 0
    for b in range(B):
        lp, top, top_lp = res[b]
        n = len(targets[b])
        assert len(lp) == len(top) == len(top_lp) == n
        r_lp, r_top, r_top_lp, _ = reduce_logits(logits[k:k + n], targets[b])
        for i in range(n):
            assert int(top[i]) == int(r_top[i]), (b, i)
            if head == "twin_rows":
                assert int(top[i]) < V // 2, (b, i, int(top[i]))
            e1, e2 = abs(float(lp[i]) - r_lp[i]), abs(float(top_lp[i]) - r_top_lp[i])
            worst = max(worst, e1, e2)
            assert e1 <= 1e-4 and e2 <= 1e-4, (precise, B, b, i, float(lp[i]), r_lp[i], float(top_lp[i]), r_top_lp[i])
            assert float(lp[i]) <= 0.0 and float(top_lp[i]) <= 0.0
            if int(top[i]) == targets[b][i]:
                assert _bits(lp[i:i + 1])[0] == _bits(top_lp[i:i + 1])[0], (b, i)
        k += n
    print(f"[score] {head} precise={precise} B={B}: {M} rows, worst |lp - log_softmax| {worst:.2e}")


def test_target_equal_to_the_argmax_is_bit_equal(tiny_dir):
    """Scoring the model's own argmax ids (one utterance, prefix of its greedy path): lp is top_lp bit for bit on every row."""
    clip = synthetic.synthetic_clip(300, 1.0)
    eng = HipEngine(tiny_dir, 0, max_new_tokens=16)
    ids = eng.transcribe_batch([clip], None, max_new=8, fixed_new_tokens=8)[0]
    lp, top, top_lp = eng.score_batch([clip], [ids])[0]
    eng.close()
    hit = [i for i in range(8) if int(top[i]) == ids[i]]
    assert hit, "no row whose argmax is the target"
    assert np.array_equal(_bits(lp[hit]), _bits(top_lp[hit]))


@pytest.fixture(scope="module")
def tiny32(tiny_dir, tiny_oracle):
    """The 32 ragged clips, their targets (the oracle's greedy ids, every third replaced) and the oracle's scores."""
    clips, lens = _clips32(), ragged_lens(32)
    targets, ref = [], []
    for c, n in zip(clips, lens):
        g = tiny_oracle.transcribe_ids(c, fixed_new_tokens=n, keep_logits=False).ids if n else []
        t = [perturb(x) if s % 3 == 2 else int(x) for s, x in enumerate(g)]
        assert AUDIO_PAD not in t
        targets.append(t)
        ref.append(oracle_score(tiny_oracle, c, t))
    return clips, targets, ref


@pytest.mark.parametrize("precise", [True, False])
def test_against_the_oracle_tiny_32_ragged_clips(tiny_dir, tiny32, precise):
    clips, targets, ref = tiny32
    eng = HipEngine(tiny_dir, 0, precise=precise, max_new_tokens=16)
    res, logits = _stage_score(eng, clips, targets)
    whole = eng.score_batch(clips, targets)
    eng.close()
    assert _same(res, whole), "q3a_score_batch_ptrs differs from the stage form"
    k, left_out, worst, worst_err, off_argmax = 0, 0, 0.0, 0.0, 0
    for b in range(32):
        lp, top, _ = res[b]
        r_lp, r_top, _, margin, r_logits = ref[b]
        for i in range(len(targets[b])):
            err = float(np.abs(logits[k] - r_logits[i]).max())
            dlp = abs(float(lp[i]) - r_lp[i])
            worst, worst_err = max(worst, dlp), max(worst_err, err)
            off_argmax += int(r_top[i]) != targets[b][i]
            if precise:
                assert dlp <= 1e-4, (b, i, float(lp[i]), r_lp[i])
                if margin[i] > 2.0 * err:
                    assert int(top[i]) == int(r_top[i]), (b, i, margin[i], err)
                else:
                    left_out += 1
            else:
                assert dlp <= 2.0 * err + 1e-5, (b, i, float(lp[i]), r_lp[i], err)
            k += 1
    assert k == 210
    print(f"[score] tiny 32 clips precise={precise}: worst |dlp| {worst:.2e}, worst |dlogit| {worst_err:.2e}, "
          f"{off_argmax} of 210 targets off the oracle's argmax, {left_out} rows left out of the id comparison")
    assert left_out <= 2


def test_against_the_oracle_0p6b_dims():
    d = synthetic.write_checkpoint("/tmp/q3a_ckpt_0p6b_peaked", "0.6b", seed=0, embed_scale=synthetic.PEAKED_EMBED_SCALE)
    clip = synthetic.synthetic_clip(0, 30.0)
    N = 100
    orc = O.AsrOracle(d)
    t = [int(x) for x in orc.transcribe_ids(clip, fixed_new_tokens=N, keep_logits=False, last_only=True).ids]
    for s in range(3, N, 7):
        t[s] = perturb(t[s])
    r_lp, r_top, _, margin, r_logits = oracle_score(orc, clip, t)
    for precise in (True, False):
        eng = HipEngine(d, 0, precise=precise, max_new_tokens=8)
        lp, top, top_lp = eng.score_batch([clip], [t])[0]
        st, logits = _stage_score(eng, [clip], [t])
        eng.close()
        assert _same([(lp, top, top_lp)], st)
        errs = np.abs(logits - r_logits).max(axis=1)
        d_lp = np.abs(lp.astype(np.float64) - r_lp)
        left_out = int(np.sum(margin <= 2.0 * errs))
        print(f"[score] 0.6B precise={precise}: worst |dlp| {d_lp.max():.2e}, worst |dlogit| {errs.max():.2e}, {left_out} rows left out, "
              f"{int(np.sum(r_top != np.asarray(t)))} targets off the argmax, lp from {r_lp.max():.2f} to {r_lp.min():.2f}")
        for s in range(N):
            assert d_lp[s] <= (1e-4 if precise else 2.0 * errs[s] + 1e-5), (precise, s, float(lp[s]), r_lp[s], errs[s])
            if margin[s] > 2.0 * errs[s]:
                assert int(top[s]) == int(r_top[s]), (precise, s, margin[s], errs[s])
        assert left_out <= (0 if precise else 10)


@pytest.mark.parametrize("prefix", [None, [100, 2000, 30000]])
def test_agrees_with_the_decode_path(tiny_dir, tiny_oracle, prefix):
    clips = _clips32()
    eng = HipEngine(tiny_dir, 0, precise=True, max_new_tokens=16, token_logprobs=True)
    left_out, rows, worst = 0, 0, 0.0
    for batch in (clips[:1], clips):
        ids = eng.transcribe_batch(batch, prefix, max_new=12, fixed_new_tokens=12)
        glp = eng.fetch_logprobs()
        res = eng.score_batch(batch, ids, prefix)
        for b, clip in enumerate(batch):
            assert AUDIO_PAD not in ids[b]
            lp, top, _ = res[b]
            margin = oracle_score(tiny_oracle, clip, ids[b], prefix)[3]
            for i in range(12):
                worst = max(worst, abs(float(lp[i]) - float(glp[b][i])))
                assert abs(float(lp[i]) - float(glp[b][i])) <= 2e-4, (b, i, float(lp[i]), float(glp[b][i]))
                if len(batch) == 32:
                    rows += 1
                    if margin[i] > 1e-3:
                        assert int(top[i]) == ids[b][i], (b, i, margin[i])
                    else:
                        left_out += 1
                elif margin[i] > 1e-3:
                    assert int(top[i]) == ids[b][i], (b, i, margin[i])
        if prefix is not None and len(batch) == 1:
            other = eng.score_batch(batch, ids)[0][0]
            assert np.abs(other - res[0][0]).max() > 1e-3, "the language prefix did not reach the prompt"
    eng.close()
    print(f"[score] decode path, prefix={prefix}: worst |lp - generated lp| {worst:.2e}, {left_out} of {rows} rows left out")
    assert rows == 384 and left_out <= 4


def test_errors_and_state(tiny_dir):
    from align_ref import tiny_aligner_dir
    from qwen3_asr_rs_amd.audio import build_align_prompt
    clips = _clips32(3)
    fresh = HipEngine(tiny_dir, 0, max_new_tokens=16)
    want = fresh.transcribe_batch(clips, None, max_new=10, fixed_new_tokens=10)
    want1 = fresh.transcribe_batch(clips[:1], None, max_new=10, fixed_new_tokens=10)
    fresh.close()
    eng = HipEngine(tiny_dir, 0, max_new_tokens=16)
    with pytest.raises(Q3aError, match="q3a_encode"):
        eng.score([HipEngine.build_prompt(13)], [[1, 2]])
    assert eng.transcribe_batch(clips, None, max_new=10, fixed_new_tokens=10) == want  # (captures the decode graph)
    ok = [[5, 6, 7], [], [9]]
    for bad, msg in (([[5, -1, 7], [], [9]], "out of range"), ([[5, V, 7], [], [9]], "out of range"),
                     ([[5, AUDIO_PAD, 7], [], [9]], "audio_pad")):
        with pytest.raises(Q3aError, match=msg):
            eng.score_batch(clips, bad)
    with pytest.raises(Q3aError, match="stride"):
        eng.score_batch(clips, ok, stride=2)
    eng.mel(clips)
    eng.encode()
    prompts = [HipEngine.build_prompt(t) for t in eng._T]
    with pytest.raises(Q3aError, match="stride"):
        eng.score(prompts, ok, stride=2)
    with pytest.raises(Q3aError, match="audio_pad"):
        eng.score(prompts, [[AUDIO_PAD], [], []])
    # nothing to score is valid and returns nothing
    empty = eng.score_batch(clips, [[], [], []])
    assert [len(x[0]) for x in empty] == [0, 0, 0]
    res = eng.score_batch(clips, ok)
    assert [len(x[0]) for x in res] == [3, 0, 1]
    tm = eng.timings()
    p = [len(HipEngine.build_prompt(eng.num_audio_tokens(len(c)))) for c in clips]
    assert tm["decode_steps"] == 0 and tm["batch"] == 3
    assert tm["total_prompt_tokens"] == sum(pb + max(len(t) - 1, 0) for pb, t in zip(p, ok))
    assert tm["total_ms"] >= tm["prefill_ms"] > 0 and tm["mel_ms"] > 0 and tm["encoder_ms"] > 0
    head_ms = eng.debug_read("score_head_ms")
    assert head_ms.shape == (1,) and 0 < float(head_ms[0]) <= tm["prefill_ms"]
    # no decode state after a score call
    with pytest.raises(Q3aError, match="no prefill state"):
        eng.decode_step()
    with pytest.raises(Q3aError, match="no decode state"):
        eng.set_next_tokens([1, 2, 3])
    with pytest.raises(Q3aError, match="nothing generated"):
        eng.fetch_ids(4)
    # ... and the next transcription is what a fresh engine returns (graph replay included), for the same and another batch shape
    assert eng.transcribe_batch(clips, None, max_new=10, fixed_new_tokens=10) == want
    eng.score_batch(clips[:1], [[3] * 14])
    assert eng.transcribe_batch(clips[:1], None, max_new=10, fixed_new_tokens=10) == want1
    assert eng.transcribe_batch(clips, None, max_new=10, fixed_new_tokens=10) == want
    # an aligner engine refuses score; an ASR engine still refuses align
    al = HipEngine(tiny_aligner_dir(), 0, max_new_tokens=4)
    with pytest.raises(Q3aError, match="forced aligner"):
        al.score_batch(clips[:1], [[1, 2]])
    al.mel(clips[:1])
    al.encode()
    with pytest.raises(Q3aError, match="forced aligner"):
        al.score([build_align_prompt(al._T[0], [])], [[1, 2]])
    al.close()
    eng.mel(clips[:1])
    eng.encode()
    with pytest.raises(Q3aError, match="not a forced-aligner"):
        eng.align([build_align_prompt(eng._T[0], [])])
    eng.close()


def test_asr_inference_score_ids(tiny_dir):
    clip = synthetic.synthetic_clip(12, 1.5)
    asr = AsrInference.load(tiny_dir, 0)
    ids = asr.transcribe(clip, max_new_tokens=6).ids
    res = asr.score(clip, ids)
    assert res.target_ids == ids + [EOS] and len(res.token_logprobs) == len(res.greedy_ids) == len(res.greedy_logprobs) == len(ids) + 1
    assert res.avg_logprob == pytest.approx(float(np.mean(np.asarray(res.token_logprobs, np.float64))), abs=1e-12)
    assert all(a <= b <= 0.0 for a, b in zip(res.token_logprobs, res.greedy_logprobs))
    plain = asr.score(clip, ids, eos=False)
    assert plain.target_ids == ids and plain.token_logprobs == res.token_logprobs[:-1]
    assert asr.score(clip, [], eos=False).avg_logprob is None
    with pytest.raises(Q3aError, match="tokenizer"):
        asr.score(clip, "some text", language="english")


def test_cli_score_line(tiny_dir, tmp_path):
    """`asr` with a language argument: without Q3A_SCORE_TEXT the output is what it was; with it one more stdout line,
    `Score: avg_logprob <x> min_token_prob <p> tokens <n> disagree <k>`, whose values are those of the Python API."""
    from qwen3_asr_rs_amd.build import CLI_PATH
    mdir = tmp_path / "model"
    mdir.mkdir()
    for f in os.listdir(tiny_dir):
        if f.endswith((".json", ".safetensors")):
            os.symlink(os.path.join(tiny_dir, f), mdir / f)
    special = {151643: "<|endoftext|>", 151645: "<|im_end|>", 151704: "<asr_text>"}
    vocab = {f"t{i}": i for i in range(151936) if i not in special}
    # single letters make an arbitrary lower-case text encodable by this toy vocabulary
    for j, ch in enumerate("abcdefghijklmnopqrstuvwxyz"):
        del vocab[f"t{1000 + j}"]
        vocab[ch] = 1000 + j
    del vocab["t220"], vocab["t1100"]
    vocab["Ġ"], vocab["E"] = 220, 1100  # the byte-level space; the capital of the prefix "language English"
    tok = {"version": "1.0", "added_tokens": [{"id": i, "content": c, "special": True} for i, c in special.items()],
           "model": {"type": "BPE", "vocab": vocab, "merges": []}}
    (mdir / "tokenizer.json").write_text(json.dumps(tok))
    text = "hello world"
    (tmp_path / "ref.txt").write_text(text + "\n")
    wav = os.path.join(GOLDEN, "sample1.wav")
    env = {k: v for k, v in os.environ.items() if k not in ("Q3A_SCORE_TEXT", "Q3A_TOKEN_LOGPROBS", "Q3A_ALIGNER")}
    env["RUST_LOG"] = "warn"
    cmd = [CLI_PATH, str(mdir), wav, "english"]
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert plain.returncode == 0, plain.stderr
    scored = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(env, Q3A_SCORE_TEXT=str(tmp_path / "ref.txt")))
    assert scored.returncode == 0, scored.stderr
    a, b = plain.stdout.split("\n"), scored.stdout.split("\n")
    assert len(a) == 3 and a[2] == "" and a[0].startswith("Language: ") and a[1].startswith("Text: ")
    assert len(b) == 4 and b[:2] == a[:2] and b[3] == ""
    assert plain.stderr == scored.stderr
    # without a language argument the variable changes nothing
    nolang = subprocess.run(cmd[:3], capture_output=True, text=True, timeout=300, env=dict(env, Q3A_SCORE_TEXT=str(tmp_path / "ref.txt")))
    assert nolang.returncode == 0 and len(nolang.stdout.split("\n")) == 3
    m = re.fullmatch(r"Score: avg_logprob (-?\d+\.\d{6}) min_token_prob (\d+\.\d{6}) tokens (\d+) disagree (\d+)", b[2])
    assert m, b[2]
    asr = AsrInference.load(str(mdir), 0)
    res = asr.score(wav, text, language="english")
    assert res.target_ids == [151704] + [1000 + ord(c) - ord("a") if c != " " else 220 for c in text] + [EOS]
    assert int(m.group(3)) == len(res.target_ids)
    assert int(m.group(4)) == sum(int(x != y) for x, y in zip(res.greedy_ids, res.target_ids))
    assert float(m.group(1)) == pytest.approx(res.avg_logprob, abs=1e-6)
    assert float(m.group(2)) == pytest.approx(float(np.exp(min(res.token_logprobs))), abs=1e-6)


def test_one_score_call_costs_less_than_the_decode_loop():
    """0.6B dimensions, 32 x 30 s clips, 100 positions each: the only way to as many teacher-forced positions without q3a_score
    is a prefill plus 100 dependent decode steps; the scoring call (one longer prefill plus the head) must take less."""
    d = synthetic.write_checkpoint("/tmp/q3a_ckpt_0p6b_peaked", "0.6b", seed=0, embed_scale=synthetic.PEAKED_EMBED_SCALE)
    clips = [synthetic.synthetic_clip(500 + i, 30.0) for i in range(32)]
    N = 100
    eng = HipEngine(d, 0, max_new_tokens=N)
    ids = eng.transcribe_batch(clips, None, max_new=N, fixed_new_tokens=N)
    targets = [[x + 1 if x == AUDIO_PAD else x for x in t] for t in ids]
    eng.score_batch(clips, targets)  # warm-up of both done
    eng.transcribe_batch(clips, None, max_new=N, fixed_new_tokens=N)
    t_dec = eng.timings()
    eng.score_batch(clips, targets)
    t_sc = eng.timings()
    head_ms = float(eng.debug_read("score_head_ms")[0])
    eng.close()
    print(f"[score] 0.6B 32 x 30 s x {N}: score total {t_sc['total_ms']:.2f} ms (prefill {t_sc['prefill_ms']:.2f}, head {head_ms:.2f}); "
          f"transcribe total {t_dec['total_ms']:.2f} ms (prefill {t_dec['prefill_ms']:.2f}, decode {t_dec['decode_ms']:.2f})")
    assert t_sc["decode_steps"] == 0 and t_dec["decode_steps"] == N - 1
    assert t_sc["total_ms"] < t_dec["total_ms"]
