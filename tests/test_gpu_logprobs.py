"""Token log-probabilities (q3a_opts.token_logprobs, q3a_fetch_logprobs) on the GPU.

Every producer of argmax partials (the one-sequence GEMV head, the two-sequence GEMV, the gemm16 epilogue for up to 32 sequences,
argmax_partial_kernel for the precise mode and above 32 sequences) carries a log-sum channel that argmax_finalize merges into
lp = logit[id] - logsumexp(logits).  Checked here: the reduction arithmetic on every path against float64 log_softmax of the
engine's own logits, the values against the fp32 oracle at the 0.6B dimensions, that the option never changes an id or a length,
that a cached graph of another batch shape is never replayed for the channel, the error cases and the CLI's confidence line."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from eos_plan import peaked_checkpoint, plan_class_stops
from oracle import q3asr_oracle as O
from qwen3_asr_rs_amd import synthetic
from qwen3_asr_rs_amd.engine import AsrInference, HipEngine, Q3aError

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_audio")


def _log_softmax_at(logits, idx):
    x = np.asarray(logits, dtype=np.float64)
    m = x.max()
    return float(x[idx] - m - np.log(np.exp(x - m).sum()))


def _clips(n, seed0=40, base=1.0):
    return [synthetic.synthetic_clip(seed0 + i, base + 0.25 * (i % 4)) for i in range(n)]


def _stage_run(eng, clips, steps):
    """Prefill + free-running decode through the stage API: per-step [B][V] logits and [B] ids, then fetch_logprobs()."""
    eng.mel(clips)
    eng.encode()
    logits, nxt = eng.prefill([HipEngine.build_prompt(t) for t in eng._T])
    L, T = [logits.copy()], [nxt.copy()]
    for _ in range(steps - 1):
        lg, nx, _ = eng.decode_step()
        L.append(lg.copy())
        T.append(nx.copy())
    return L, T, eng.fetch_logprobs()


@pytest.fixture(scope="module")
def twin_rows_dir(tiny_untied_dir):
    """The untied tiny checkpoint with lm_head rows V/2 .. V-1 replaced by rows 0 .. V/2-1: every logit has an exact twin V/2 rows
    later, in another block, wave, workgroup and partial, so every path's argmax meets a tie at its maximum."""
    d = "/tmp/q3a_ckpt_tiny_untied_twin_rows"
    if os.path.exists(d):
        shutil.rmtree(d)
    shutil.copytree(tiny_untied_dir, d)
    key = synthetic.output_embedding_key(d)
    head = synthetic.read_tensor(d, key).astype(np.float32)
    h = head.shape[0] // 2
    assert head.shape[0] == 2 * h
    head[h:] = head[:h]
    synthetic.overwrite_tensor(d, key, head)
    return d


_PATHS = [(False, 1), (False, 2), (False, 5), (False, 32), (False, 40), (True, 1), (True, 5)]


@pytest.mark.parametrize("precise,B,head", [pytest.param(p, b, "tiny", id=f"{p}-{b}") for p, b in _PATHS] +
                         [pytest.param(p, b, "twin_rows", id=f"{p}-{b}-twin_rows") for p, b in _PATHS])
def test_logprobs_match_log_softmax_of_the_engines_logits(request, precise, B, head):
    """One path per case: B = 1 the fused-norm GEMV head, 2 the two-sequence GEMV, 5 / 32 the gemm16 argmax epilogue, 40 (two
    decode groups) and the precise mode argmax_partial_kernel.  Graph-replayed stage API, so the first step is the prefill's.
    twin_rows: the tie rule (the first index wins) on every path -- every id lies in the first half of the vocabulary."""
    steps = 6
    d = request.getfixturevalue("tiny_dir" if head == "tiny" else "twin_rows_dir")
    eng = HipEngine(d, 0, precise=precise, max_new_tokens=16, token_logprobs=True)
    L, T, lp = _stage_run(eng, _clips(B), steps)
    eng.close()
    assert len(lp) == B
    worst = 0.0
    for b in range(B):
        assert len(lp[b]) == steps, (b, len(lp[b]))   # random weights: no EOS within a few steps
        for s in range(steps):
            assert int(T[s][b]) == int(np.argmax(L[s][b])), (b, s)
            if head == "twin_rows":
                assert int(T[s][b]) < len(L[s][b]) // 2, (precise, B, b, s, int(T[s][b]))
            ref = _log_softmax_at(L[s][b], int(T[s][b]))
            err = abs(float(lp[b][s]) - ref)
            worst = max(worst, err)
            assert err <= 1e-4, (precise, B, b, s, float(lp[b][s]), ref)
    assert np.all(np.concatenate(lp) <= 0.0)
    print(f"[logprobs] {head} precise={precise} B={B}: {B * steps} values, worst |lp - log_softmax| {worst:.2e}")


def test_logprobs_against_the_oracle_0p6b_dims():
    """0.6B dims, peaked checkpoint, one 30 s clip, 100 tokens graph-replayed: the oracle teacher-forced on the engine's ids.
    Precise mode within 1e-4 per step; default mode within 2 max|logit err| of that step (+1e-5): |dlp| <= |dl_id| + |dLSE|."""
    d = synthetic.write_checkpoint("/tmp/q3a_ckpt_0p6b_peaked", "0.6b", seed=0, embed_scale=synthetic.PEAKED_EMBED_SCALE)
    clip = synthetic.synthetic_clip(0, 30.0)
    N = 100
    orc = O.AsrOracle(d)
    for precise in (True, False):
        eng = HipEngine(d, 0, precise=precise, max_new_tokens=N, token_logprobs=True)
        ids = eng.transcribe_batch([clip], None, max_new=N, fixed_new_tokens=N)[0]
        lp = eng.fetch_logprobs()[0]
        assert len(ids) == len(lp) == N
        ref = orc.transcribe_ids(clip, forced_ids=ids[:N - 1], last_only=True)
        ref_lp = [float(torch.log_softmax(ref.step_logits[s].double(), 0)[ids[s]]) for s in range(N)]
        # the engine's own logits on the same history (eager stage API) give the per-step logit error
        eng.mel([clip])
        eng.encode()
        logits, _ = eng.prefill([HipEngine.build_prompt(ref.num_audio_tokens)])
        errs = [float(np.abs(logits[0] - ref.step_logits[0].numpy()).max())]
        for s in range(N - 1):
            eng.set_next_tokens([ids[s]])
            lg, _, _ = eng.decode_step()
            errs.append(float(np.abs(lg[0] - ref.step_logits[s + 1].numpy()).max()))
        eng.close()
        d_lp = [abs(float(lp[s]) - ref_lp[s]) for s in range(N)]
        print(f"[logprobs] 0.6B precise={precise}: worst |dlp| {max(d_lp):.2e}, worst |dlogit| {max(errs):.2e}, "
              f"mean lp {np.mean(lp):.4f} (oracle {np.mean(ref_lp):.4f})")
        for s in range(N):
            bound = 1e-4 if precise else 2.0 * errs[s] + 1e-5
            assert d_lp[s] <= bound, (precise, s, float(lp[s]), ref_lp[s], errs[s])


def _whole(d, clips, kmax, fixed, use_graph, lp_on):
    eng = HipEngine(d, 0, max_new_tokens=kmax, use_graph=use_graph, token_logprobs=lp_on)
    ids = eng.transcribe_batch(clips, None, max_new=kmax, fixed_new_tokens=kmax if fixed else 0)
    lp = eng.fetch_logprobs() if lp_on else None
    steps = eng.timings()["decode_steps"]
    eng.close()
    return ids, lp, steps


def _compare_on_off(tag, d, clips, kmax):
    for fixed in (True, False):
        for use_graph in (True, False):
            off, _, steps_off = _whole(d, clips, kmax, fixed, use_graph, False)
            on, lp, steps_on = _whole(d, clips, kmax, fixed, use_graph, True)
            assert on == off, f"{tag}: ids differ with token_logprobs (fixed={fixed}, graph={use_graph})"
            assert steps_on == steps_off
            assert [len(x) for x in lp] == [len(x) for x in on]
            for x in lp:
                assert np.all(np.isfinite(x)) and np.all(x <= 0.0), (tag, x)
    return off


def test_option_changes_no_id_one_and_three_clips(tiny_dir):
    """One clip (pruned int8 argmax with the option off, the full GEMV with it on) and three clips (gemm16 epilogue), graph and
    eager, fixed-length and natural-EOS mode: identical ids and lengths."""
    _compare_on_off("tiny 1 clip", tiny_dir, _clips(1, 60, 2.0), 24)
    _compare_on_off("tiny 3 clips", tiny_dir, _clips(3, 70, 1.5), 24)


def test_option_changes_no_id_ragged_eos_batch_of_32():
    """32 utterances with planted EOS at steps 1 / 2 / 3 / 5 / 7 and two never-EOS classes (tests/eos_plan.py): the ragged
    natural-EOS lengths and every id are the same with the option on, and the log-probabilities cover exactly those ids."""
    d = peaked_checkpoint("/tmp/q3a_ckpt_tinyu_peaked_lp", "tiny_untied", seed=5)
    B, kmax = 32, 9
    classes = [i % 7 for i in range(B)]
    clips = [synthetic.synthetic_clip(200 + i, 1.0 + 0.35 * classes[i]) for i in range(B)]
    stops, _, _ = plan_class_stops(d, clips, classes, [1, None, 3, 5, 7, None, 2], kmax)
    ids = _compare_on_off("tiny ragged 32", d, clips, kmax)
    lens = sorted({len(x) for x in ids})
    print(f"[logprobs] ragged batch: natural-EOS lengths {lens}")
    assert len(lens) >= 3, lens   # really ragged


def test_no_stale_graph_across_batch_shapes(tiny_dir):
    """One engine runs batch A, then B, then A again; each run's log-probabilities equal an eager engine's, bit for bit."""
    A, Bb = _clips(1, 80, 2.0), _clips(3, 90, 1.25)
    kmax = 12
    eager = HipEngine(tiny_dir, 0, max_new_tokens=kmax, use_graph=False, token_logprobs=True)
    want = {}
    for name, clips in (("A", A), ("B", Bb)):
        want[name] = (eager.transcribe_batch(clips, None, max_new=kmax, fixed_new_tokens=kmax), eager.fetch_logprobs())
    eager.close()
    eng = HipEngine(tiny_dir, 0, max_new_tokens=kmax, use_graph=True, token_logprobs=True)
    for name, clips in (("A", A), ("B", Bb), ("A", A)):
        ids = eng.transcribe_batch(clips, None, max_new=kmax, fixed_new_tokens=kmax)
        lp = eng.fetch_logprobs()
        assert ids == want[name][0], name
        assert len(lp) == len(want[name][1])
        for x, y in zip(lp, want[name][1]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name
    eng.close()


def test_fetch_logprobs_errors(tiny_dir):
    clip = synthetic.synthetic_clip(3, 1.0)
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8)
    eng.transcribe_batch([clip], None, max_new=4, fixed_new_tokens=4)
    with pytest.raises(Q3aError, match="token_logprobs"):
        eng.fetch_logprobs()
    eng.close()
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8, token_logprobs=True)
    eng.batch = 1
    with pytest.raises(Q3aError, match="nothing generated"):
        eng.fetch_logprobs()
    eng.close()


def test_asr_inference_fills_the_confidence_fields(tiny_dir):
    clip = synthetic.synthetic_clip(12, 1.5)
    plain = AsrInference.load(tiny_dir, 0).transcribe(clip, max_new_tokens=20)
    assert plain.token_logprobs is None and plain.avg_logprob is None
    res = AsrInference.load(tiny_dir, 0, token_logprobs=True).transcribe(clip, max_new_tokens=20)
    assert res.ids == plain.ids and len(res.token_logprobs) == len(res.ids) == 20
    assert res.avg_logprob == pytest.approx(float(np.mean(np.asarray(res.token_logprobs, np.float64))), abs=1e-12)


def test_cli_confidence_line(tiny_dir, tmp_path):
    """`asr` on the tiny checkpoint and tests/golden/test_audio/sample1.wav: without Q3A_TOKEN_LOGPROBS two stdout lines as
    before; with it a third, `Confidence: avg_logprob <x> min_token_prob <p>`, whose values are those of the Python API."""
    import json
    from qwen3_asr_rs_amd.build import CLI_PATH
    mdir = tmp_path / "model"
    mdir.mkdir()
    for f in os.listdir(tiny_dir):
        if f.endswith((".json", ".safetensors")):
            os.symlink(os.path.join(tiny_dir, f), mdir / f)
    vocab = {f"t{i}": i for i in range(151936) if i not in (151643, 151645)}
    tok = {"version": "1.0", "added_tokens": [{"id": 151643, "content": "<|endoftext|>", "special": True},
                                              {"id": 151645, "content": "<|im_end|>", "special": True}],
           "model": {"type": "BPE", "vocab": vocab, "merges": []}}
    (mdir / "tokenizer.json").write_text(json.dumps(tok))
    wav = os.path.join(GOLDEN, "sample1.wav")
    env = {k: v for k, v in os.environ.items() if k != "Q3A_TOKEN_LOGPROBS"}
    env["RUST_LOG"] = "warn"
    plain = subprocess.run([CLI_PATH, str(mdir), wav], capture_output=True, text=True, timeout=300, env=env)
    assert plain.returncode == 0, plain.stderr
    withlp = subprocess.run([CLI_PATH, str(mdir), wav], capture_output=True, text=True, timeout=300, env=dict(env, Q3A_TOKEN_LOGPROBS="1"))
    assert withlp.returncode == 0, withlp.stderr
    a, b = plain.stdout.split("\n"), withlp.stdout.split("\n")
    assert len(a) == 3 and a[2] == "" and a[0].startswith("Language: ") and a[1].startswith("Text: ")
    assert len(b) == 4 and b[:2] == a[:2] and b[3] == ""
    assert plain.stderr == withlp.stderr
    m = re.fullmatch(r"Confidence: avg_logprob (-?\d+\.\d{6}) min_token_prob (\d+\.\d{6})", b[2])
    assert m, b[2]
    res = AsrInference.load(str(mdir), 0, token_logprobs=True).transcribe(wav)
    assert a[0] == f"Language: {res.language}" and a[1] == f"Text: {res.text}"
    assert len(res.token_logprobs) == len(res.ids) > 0
    assert float(m.group(1)) == pytest.approx(res.avg_logprob, abs=1e-6)
    assert float(m.group(2)) == pytest.approx(float(np.exp(min(res.token_logprobs))), abs=1e-6)
