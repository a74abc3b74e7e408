"""Temperature sampling on the GPU (q3a_set_sampling; k_sample.hip): the kernels against the numpy reference through
q3a_selftest_sample, every lm_head form feeding the sampler, graph replay against the eager stage API, repeatability, the return to
the greedy engine, the composition with the logit bias, log-probabilities, the refusals and the device memory across cycles.

The rule for an id (include/q3asr.h "sampling"): the device evaluates z = l' + T g in fp32, the reference in float64.  Where the
reference's margin between its best two z exceeds EPS the id must be the reference's; where it does not, it must be one of those two,
and at most 1 % of a test's draws may be that close.  EPS is twice the largest |z_device - z_reference| measured over the kernel test
(3.54e-6 on the first run on an MI355X, at V = 6150): it pays for fp32 log / log1p / fma against float64."""
import json
import os
import subprocess

import numpy as np
import pytest

import logit_bias_ref as B_
import sampling_ref as R
from qwen3_asr_rs_amd import _lib, synthetic
from qwen3_asr_rs_amd.engine import AsrInference, HipEngine, Q3aError

pytestmark = pytest.mark.gpu

V = 151936
EPS = 7.1e-6
SEED = (7 << 32) + 99
C = _lib.C


def _selftest(rows, T, min_p, seed, step):
    lib = _lib.load()
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    S, Vr = rows.shape
    ids, lp, z = np.full(S, -7, np.int32), np.zeros(S, np.float32), np.zeros(S, np.float32)
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    rc = lib.q3a_selftest_sample(0, rows.ctypes.data_as(f32p), S, Vr, C.c_float(T), C.c_float(min_p), C.c_uint64(seed), step,
                                 ids.ctypes.data_as(i32p), lp.ctypes.data_as(f32p), z.ctypes.data_as(f32p))
    assert rc == 0, lib.q3a_last_error(None)
    return ids, lp, z


def _judge(got_id: int, d, where):
    """The id rule; returns 1 when the draw was under EPS (counted against the 1 % cap)."""
    if d.margin > EPS:
        assert got_id == d.id, (where, got_id, d.id, d.second, d.margin)
        return 0
    assert got_id in (d.id, d.second), (where, got_id, d.id, d.second, d.margin)
    return 1


# ---- 1. the kernels against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("Vk", list(R.KERNEL_V) + [R.BIG_V])
def test_kernels_against_the_reference(Vk):
    """V = 1, 63 (one partial chunk), 2048 (exactly one), 2049 (one logit in the second), 4100 (scalar loads: not a multiple of 4),
    6150 (four chunks, the last partial), 151936 once; S = 1 and 3; T, min_p, step as sampling_ref lists them; rows with a whole
    chunk of -inf, the maximum in the last partial chunk, twin maxima and a single finite entry."""
    rows, calls, draws = R.kernel_rows(Vk), R.kernel_calls(Vk), R.kernel_draws(Vk)
    by_call = {}
    for ci, s, d in draws:
        by_call.setdefault(ci, []).append(d)
    under = n = 0
    worst_z = worst_lp = 0.0
    for ci, (g, T, p, st) in enumerate(calls):
        ids, lp, z = _selftest(rows[g], T, p, R.SAMPLE_SEED, st)
        for s, d in enumerate(by_call[ci]):
            assert d.margin > 1e-3 * T                                    # (held on the CPU by tests/test_sampling_host.py)
            under += _judge(int(ids[s]), d, (Vk, g, T, p, st, s))
            n += 1
            if int(ids[s]) == d.id:
                worst_z = max(worst_z, abs(float(z[s]) - d.z))
            ref_lp = float(R.log_softmax64(rows[g[s]])[int(ids[s])])
            worst_lp = max(worst_lp, abs(float(lp[s]) - ref_lp))
            assert abs(float(lp[s]) - ref_lp) <= 1e-4, (Vk, g, T, p, st, s, float(lp[s]), ref_lp)
            assert d.kept[int(ids[s])]
            if p == 1.0 and g[s] != 2:                                    # min_p = 1 without ties: the plain argmax
                assert int(ids[s]) == int(np.argmax(rows[g[s]]))
    print(f"[sampling] V={Vk}: {n} draws, largest |z - z_ref| {worst_z:.3e} (EPS {EPS:.1e}), largest |lp - log_softmax64| {worst_lp:.2e}, "
          f"{under} under EPS")
    assert worst_z <= EPS / 2, worst_z                                   # EPS is twice the measured figure: a build that computes z worse shows here
    assert under <= 0.01 * n


# ---- 2. every head form stores what the sampler reads ------------------------------------------------------------------------
def _clips(n, seed0=40, base=1.0):
    return [synthetic.synthetic_clip(seed0 + i, base + 0.25 * (i % 4)) for i in range(n)]


def _stage_run(eng, clips, steps):
    """Prefill + decode through the stage API: logits [steps][B][V], ids [steps][B], done [steps][B] (the prefill's row: zeros)."""
    eng.mel(clips)
    eng.encode()
    logits, nxt = eng.prefill([HipEngine.build_prompt(t) for t in eng._T])
    L, T, D = [logits.copy()], [nxt.copy()], [np.zeros(len(clips), np.uint8)]
    for _ in range(steps - 1):
        lg, nx, dn = eng.decode_step()
        L.append(lg.copy())
        T.append(nx.copy())
        D.append(dn.copy())
    return np.stack(L), np.stack(T), np.stack(D)


@pytest.mark.parametrize("precise,B", [(False, 1), (False, 2), (False, 5), (False, 32), (False, 40), (True, 5)])
def test_every_head_form_feeds_the_sampler(tiny_dir, precise, B):
    """B = 1 the fused-norm GEMV head (the pruned pair must not be taken), 2 the two-sequence GEMV, 5 / 32 the gemm16 argmax epilogue,
    40 and the precise mode argmax_partial_kernel: 12 steps at T = 1, every id against the reference on that step's own logits with
    (s, t) = (index in the call, step), the log-probabilities, done and the lengths."""
    steps = 12
    eng = HipEngine(tiny_dir, 0, precise=precise, max_new_tokens=16, token_logprobs=True)
    try:
        eng.set_sampling(1.0, 0.0, SEED)
        assert eng.sampling_stats() == {"active": True, "temperature": 1.0, "min_p": 0.0, "seed": SEED}
        L, T, D = _stage_run(eng, _clips(B), steps)
        lps = eng.fetch_logprobs()
        ids = eng.fetch_ids(16)
    finally:
        eng.close()
    assert not np.isnan(L).any()
    draws = R.sample_many([(L[t][q], 1.0, 0.0, SEED, q, t) for t in range(steps) for q in range(B)], threads=12)
    under = 0
    worst_lp = 0.0
    for t in range(steps):
        for q in range(B):
            under += _judge(int(T[t][q]), draws[t * B + q], (precise, B, t, q))
    assert under <= 0.01 * steps * B
    assert len({int(x) for x in T.reshape(-1)}) > steps * B // 2          # draws, not one id over and over
    for q in range(B):
        col = [int(x) for x in T[:, q]]
        stop = next((i for i, x in enumerate(col) if x in B_.EOS_IDS), steps)
        assert ids[q] == col[:stop] and len(lps[q]) == stop
        for t in range(1, steps):
            assert bool(D[t][q]) == (stop <= t), (q, t)
        for t in range(stop):
            ref = float(R.log_softmax64(L[t][q])[col[t]])
            worst_lp = max(worst_lp, abs(float(lps[q][t]) - ref))
            assert abs(float(lps[q][t]) - ref) <= 1e-4, (q, t, float(lps[q][t]), ref)
    print(f"[sampling] precise={precise} B={B}: {under} of {steps * B} draws under EPS, worst |lp - log_softmax64| {worst_lp:.2e}")


# ---- 3. graph, eager, repeatability, and the way back to greedy --------------------------------------------------------------
def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _eos_bias(model_dir, clips, p_stop=0.25):
    """A bias on <|im_end|> under which a draw at T = 1 stops with probability about p_stop: natural EOS at ragged lengths."""
    eng = HipEngine(model_dir, 0, max_new_tokens=4)
    try:
        eng.mel(clips[:1])
        eng.encode()
        l, _ = eng.prefill([HipEngine.build_prompt(eng._T[0])])
    finally:
        eng.close()
    l = l[0].astype(np.float64)
    lse = l.max() + np.log(np.exp(l - l.max()).sum())
    return {151645: float(np.float32(lse - l[151645] + np.log(p_stop / (1 - p_stop))))}


def _stats(eng):
    return eng.debug_read_raw("lm_head_prune_stats").view(np.int32).copy()


@pytest.mark.parametrize("B", [1, 5])
def test_graph_eager_repeatability_and_back_to_greedy(tiny_dir, B):
    clips, kmax = _clips(B, 80, 1.5), 12
    bias = _eos_bias(tiny_dir, clips)
    fresh = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True)       # never samples
    greedy = fresh.transcribe_batch(clips, None, max_new=kmax), fresh.fetch_logprobs(), _stats(fresh)
    fresh.close()
    eager = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True, use_graph=False)
    try:
        eager.set_logit_bias(bias)
        eager.set_sampling(1.0, 0.0, SEED)
        _, T, _ = _stage_run(eager, clips, kmax)
        want, want_lp = eager.fetch_ids(kmax), eager.fetch_logprobs()
    finally:
        eager.close()
    for q in range(B):
        col = [int(x) for x in T[:, q]]
        assert want[q] == col[:next((i for i, x in enumerate(col) if x in B_.EOS_IDS), kmax)]
    eng = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True)
    try:
        eng.set_logit_bias(bias)
        eng.set_sampling(1.0, 0.0, SEED)
        r1 = eng.transcribe_batch(clips, None, max_new=kmax), eng.fetch_logprobs()
        r2 = eng.transcribe_batch(clips, None, max_new=kmax), eng.fetch_logprobs()
        assert r1[0] == want, (r1[0], want)                                        # graph replay, natural EOS == the eager stage API
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(r1[1], want_lp))
        assert r2[0] == r1[0] and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(r1[1], r2[1]))   # bit-identical twice
        eng.set_sampling(1.0, 0.0, SEED + 1)                                       # another seed, the same graph
        r3 = eng.transcribe_batch(clips, None, max_new=kmax)
        assert r3 != r1[0]
        eng.set_sampling(0.5, 0.1, SEED)
        assert eng.sampling_stats() == {"active": True, "temperature": 0.5, "min_p": float(np.float32(0.1)), "seed": SEED}
        eng.transcribe_batch(clips, None, max_new=kmax)
        # back to greedy: the ids, log-probabilities and pruned-argmax passes of an engine that never sampled
        eng.set_logit_bias(None)
        eng.set_sampling(0.0)
        with pytest.raises(Q3aError, match="nothing generated"):                   # the decode state is dropped
            eng.fetch_ids(kmax)
        assert eng.sampling_stats()["active"] is False
        s0 = _stats(eng)
        back = eng.transcribe_batch(clips, None, max_new=kmax), eng.fetch_logprobs()
        s1 = _stats(eng)
    finally:
        eng.close()
    assert back[0] == greedy[0] and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(back[1], greedy[1]))
    assert (s0 == 0).all(), s0                                                     # no pruned pass ran while sampling ...
    assert (s1 - s0 == greedy[2]).all(), (s0, s1, greedy[2])                        # ... and afterwards as on the fresh engine
    print(f"[sampling] B={B}: natural-EOS lengths {[len(x) for x in r1[0]]} / other seed {[len(x) for x in r3]}")


def test_pruned_argmax_returns_after_sampling(tiny_dir):
    """One sequence without token log-probabilities: the greedy step is the pruned pair.  While sampling is on it is not taken; after
    set_sampling(0) the passes advance exactly as on a fresh engine and the ids are its ids."""
    clip, steps = synthetic.synthetic_clip(0, 9.3), 16
    never = HipEngine(tiny_dir, 0, max_new_tokens=steps)
    want = never.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)
    s_never = _stats(never)
    never.close()
    assert s_never[1] >= steps - 1
    eng = HipEngine(tiny_dir, 0, max_new_tokens=steps)
    try:
        eng.set_sampling(2.0, 0.0, 5)
        a = eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps)
        assert a != want and len(a[0]) == steps and (_stats(eng) == 0).all()
        assert eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps) == a
        eng.set_sampling(0.0)
        assert eng.transcribe_batch([clip], None, max_new=steps, fixed_new_tokens=steps) == want
        assert (_stats(eng) == s_never).all(), (_stats(eng), s_never)
    finally:
        eng.close()


# ---- 4. composition ----------------------------------------------------------------------------------------------------------
def test_composition_with_the_logit_bias_beam_and_score(tiny_dir):
    clips, kmax = _clips(3, 70, 1.5), 12
    eng = HipEngine(tiny_dir, 0, max_new_tokens=kmax, token_logprobs=True)
    try:
        plain = eng.transcribe_batch(clips, None, max_new=kmax, fixed_new_tokens=kmax)
        targets = [x[:6] + [151645] for x in plain]
        score_off = eng.score_batch(clips, targets)
        sup = B_.kind_suppress(V, set(t for x in plain for t in x), plain[0][0])
        dense = B_.as_dense(V, sup)
        eng.set_logit_bias(sup)
        eng.set_sampling(2.0, 0.0, SEED)
        got = eng.transcribe_batch(clips, None, max_new=kmax, fixed_new_tokens=kmax)
        assert all(len(x) == kmax for x in got) and all(np.isfinite(dense[t]) for x in got for t in x)   # no suppressed id, ever
        assert got != plain
        score_on = eng.score_batch(clips, targets)                       # q3a_score* never sees the sampler (or the bias)
        for x, y in zip(score_off, score_on):
            assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(x[1], y[1]) and np.array_equal(_bits(x[2]), _bits(y[2]))
        eng.set_logit_bias({151645: 1e4})                                # EOS at +1e4: length 0
        assert eng.transcribe_batch(clips, None, max_new=kmax) == [[]] * 3
        eng.set_logit_bias({t: -np.inf for t in B_.EOS_IDS})              # EOS forbidden: exactly max_new ids
        assert [len(x) for x in eng.transcribe_batch(clips, None, max_new=kmax)] == [kmax] * 3
        # beam search while sampling is refused, in both forms
        with pytest.raises(Q3aError, match="sampling is on"):
            eng.beam_search_batch(clips[:1], 2, max_new=4)
        rep = [clips[0]] * 2
        eng.mel(rep)
        eng.encode()
        eng.prefill([HipEngine.build_prompt(t) for t in eng._T])
        with pytest.raises(Q3aError, match="sampling is on"):
            eng.beam_begin(2)
        eng.set_sampling(0.0)
        assert len(eng.beam_search_batch(clips[:1], 2, max_new=4)[0]) == 2
    finally:
        eng.close()


def test_refusals_and_state(tiny_dir):
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8)
    lib = eng._lib
    try:
        eng.set_sampling(0.7, 0.05, 11)
        for T, p, msg in [(-1.0, 0.0, "temperature"), (float("nan"), 0.0, "temperature"), (float("inf"), 0.0, "temperature"),
                          (1.0, -0.1, "min_p"), (1.0, 1.5, "min_p"), (1.0, float("nan"), "min_p")]:
            with pytest.raises(Q3aError, match=msg):
                eng._chk(lib.q3a_set_sampling(eng._h, C.c_float(T), C.c_float(p), C.c_uint64(3)))
            st = eng.sampling_stats()                                    # a refused call changes nothing
            assert st["active"] and st["seed"] == 11 and st["temperature"] == float(np.float32(0.7))
        clip = synthetic.synthetic_clip(3, 1.0)
        eng.mel([clip])
        eng.encode()
        eng.prefill([HipEngine.build_prompt(eng._T[0])])
        eng.decode_step()
        eng.set_sampling(0.7, 0.05, 12)                                  # a successful call drops the decode state
        with pytest.raises(Q3aError):
            eng.decode_step()
        with pytest.raises(Q3aError, match="no decode state"):
            eng.set_next_tokens([5])
    finally:
        eng.close()


class _Tok:
    def decode(self, ids, skip):
        return "language English<asr_text>" + " ".join(f"t{i}" for i in ids)

    def encode(self, text):
        return []


def test_asr_inference_temperature_and_fallback(tiny_dir):
    clip = synthetic.synthetic_clip(12, 1.5)
    asr = AsrInference.load(tiny_dir, 0, token_logprobs=True, max_new_tokens=16)
    try:
        asr.tokenizer = _Tok()
        plain = asr.transcribe(clip, max_new_tokens=8)
        assert plain.temperature is None and len(plain.ids) == 8
        a = asr.transcribe(clip, max_new_tokens=8, temperature=1.0, seed=4)
        b = asr.transcribe(clip, max_new_tokens=8, temperature=1.0, seed=4)
        assert a.temperature == 1.0 and a.ids == b.ids and a.ids != plain.ids and a.token_logprobs == b.token_logprobs
        assert asr.engine.sampling_stats()["active"] is False and asr.engine.sampling_state == (0.0, 0.0, 0)
        assert asr.transcribe(clip, max_new_tokens=8).ids == plain.ids
        # fallback: a random checkpoint's avg_logprob is far below -1, so every attempt fails and the last (T = 1, seed + 5) is kept ...
        temps = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)
        res = asr.transcribe(clip, max_new_tokens=8, temperature=temps, seed=4)
        eng = asr.engine
        eng.set_sampling(1.0, 0.0, 9)
        want = eng.transcribe_batch([clip], None, 8)[0]
        eng.set_sampling(0.0)
        assert res.temperature == 1.0 and res.avg_logprob < -1.0 and res.ids == want
        # ... and with a threshold the greedy attempt passes, it is the greedy result
        ok = asr.transcribe(clip, max_new_tokens=8, temperature=temps, seed=4, logprob_threshold=-1e9)
        assert ok.temperature == 0.0 and ok.ids == plain.ids
        with pytest.raises(Q3aError, match="beam"):
            asr.transcribe(clip, max_new_tokens=4, beam_size=2, temperature=0.5)
    finally:
        asr.engine.close()
    bare = AsrInference.load(tiny_dir, 0, max_new_tokens=8)
    try:
        with pytest.raises(Q3aError, match="token_logprobs=True"):
            bare.transcribe(clip, max_new_tokens=4, temperature=(0.0, 0.5))
    finally:
        bare.engine.close()


def test_cli_environment_variables(tiny_dir, tmp_path):
    """Q3A_TEMPERATURE / Q3A_MIN_P / Q3A_SEED through the CLI give the text of the Python call (token t<i> decodes to "t<i>")."""
    from qwen3_asr_rs_amd.build import CLI_PATH
    mdir = tmp_path / "model"
    mdir.mkdir()
    for f in os.listdir(tiny_dir):
        if f.endswith((".json", ".safetensors")):
            os.symlink(os.path.join(tiny_dir, f), mdir / f)
    vocab = {f"t{i}": i for i in range(V) if i not in B_.EOS_IDS}
    tok = {"version": "1.0", "added_tokens": [{"id": 151643, "content": "<|endoftext|>", "special": True},
                                              {"id": 151645, "content": "<|im_end|>", "special": True}],
           "model": {"type": "BPE", "vocab": vocab, "merges": []}}
    (mdir / "tokenizer.json").write_text(json.dumps(tok))
    wav = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_audio", "sample1.wav")
    asr = AsrInference.load(str(mdir), 0)
    plain = asr.transcribe(wav)
    want = asr.transcribe(wav, temperature=1.0, min_p=0.02, seed=2 ** 33 + 5)
    asr.engine.close()
    assert want.ids != plain.ids and want.temperature == 1.0
    env = {k: v for k, v in os.environ.items() if not k.startswith("Q3A_")}
    env.update(RUST_LOG="warn", Q3A_TEMPERATURE="1.0", Q3A_MIN_P="0.02", Q3A_SEED=str(2 ** 33 + 5))
    out = subprocess.run([CLI_PATH, str(mdir), wav], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    assert lines[0] == f"Language: {want.language}" and lines[1] == f"Text: {want.text}" and want.text != plain.text
    bad = subprocess.run([CLI_PATH, str(mdir), wav], capture_output=True, text=True, timeout=300, env=dict(env, Q3A_MIN_P="1.5"))
    assert bad.returncode == 1 and "Sampling failed" in bad.stderr and "min_p" in bad.stderr
    bad = subprocess.run([CLI_PATH, str(mdir), wav], capture_output=True, text=True, timeout=300, env=dict(env, Q3A_TEMPERATURE="warm"))
    assert bad.returncode == 1 and "Q3A_TEMPERATURE is not a number" in bad.stderr


# ---- 5. no leak --------------------------------------------------------------------------------------------------------------
def test_device_memory_is_level_across_cycles(tiny_dir):
    clips = _clips(2, 90, 1.0)

    def cycle():
        eng = HipEngine(tiny_dir, 0, max_new_tokens=8, token_logprobs=True)
        eng.set_sampling(1.0, 0.05, 3)
        eng.transcribe_batch(clips, None, max_new=6, fixed_new_tokens=6)
        inside = int(eng.debug_read_raw("device_bytes").view(np.uint64)[0])
        eng.set_sampling(0.0)
        eng.transcribe_batch(clips, None, max_new=6, fixed_new_tokens=6)
        eng.close()
        return inside

    probe = HipEngine(tiny_dir, 0, max_new_tokens=8)
    try:
        base = int(probe.debug_read_raw("device_bytes").view(np.uint64)[0])
        first = cycle()
        level = int(probe.debug_read_raw("device_bytes").view(np.uint64)[0])
        for _ in range(3):
            assert cycle() == first
            assert int(probe.debug_read_raw("device_bytes").view(np.uint64)[0]) == level
        assert level == base
    finally:
        probe.close()
