"""GPU tests (pytest -m gpu) of draft-verified decoding (include/q3asr.h "draft-verified decoding").

The contract: q3a_transcribe_draft_batch_ptrs returns exactly the ids of the greedy natural-EOS loop, whatever the draft; the draft
only moves work from dependent decode steps into one prefill.  So the references are (a) tests/draft_ref.py for the accept kernel
alone, word by word, (b) the plain call on the same engine and the oracle's natural-EOS run for the whole path, on the peaked
fixtures of tests/eos_plan.py where both the precise and the default bf16 mode are decidable.
"""
import json
import os
import re
import subprocess
import time

import numpy as np
import pytest

import draft_ref
from oracle import q3asr_oracle as O
from qwen3_asr_rs_amd import _lib, synthetic
from qwen3_asr_rs_amd.engine import AsrInference, HipEngine, Q3aError, StreamingTranscriber

from eos_plan import free_run_margins, peaked_checkpoint, plan_class_stops, walk_next
from test_gpu_eos import BF16_MARGIN

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_audio")
EOS0, EOS1 = draft_ref.EOS_IDS
JUNK = [7, 8, 9, 10, 11, 12, 13, 14, 15]   # ids no walk of the fixtures visits


# ---- the accept kernel alone -----------------------------------------------------------------------------------------------
def _accept_cases(V):
    """(draft, top_ids) pairs: every shape of acceptance the header lists."""
    rng = np.random.default_rng(11)

    def ids(n):
        return [int(x) for x in rng.integers(20, V - 10, size=n)]

    cases = []
    d = ids(6)
    cases.append((d, d[:3] + [d[3] + 1] + d[4:] + [17]))                   # a wrong id at j = 3 followed by rows that match again: k = j
    cases.append(([], [42]))                                                # n = 0
    cases.append(([5], [5, EOS1]))                                          # n = 1, k = n, tok = EOS (151645)
    d = ids(1100)
    cases.append((d, d[:1030] + [d[1030] + 1] + d[1031:] + [3]))           # longer than a workgroup, first mismatch at 1030
    d = ids(5)
    cases.append((d, [d[0] + 1] + d[1:] + [9]))                            # k = 0
    cases.append((d, d[:4] + [EOS0] + [9]))                                 # k = n - 1, tok = EOS (151643)
    cases.append((d, d + [23]))                                             # k = n
    d = ids(12)
    cases.append((d, d + [29]))                                             # k + 1 > out_stride (the guard)
    cases.append((d[:7], d[:7] + [31]))                                     # k + 1 == out_stride
    cases.append(([6], [7, 8]))                                             # n = 1, k = 0
    return cases


@pytest.mark.parametrize("with_lp", [False, True])
@pytest.mark.parametrize("S", [1, 2, 3, 33])
def test_accept_kernel_alone(lib, S, with_lp):
    import ctypes as C
    V, H, stride, max_pos, gsz = 2048, 128, 8, 1400, 32
    rng = np.random.default_rng(100 + S)
    base = _accept_cases(V)
    cases = [base[(s + S) % len(base)] for s in range(S)] if S < 33 else [base[s % len(base)] for s in range(S)]
    if S == 2:   # every sequence stops: the all-done progress word
        cases = [base[2], base[5]]
    drafts, tops = [c[0] for c in cases], [c[1] for c in cases]
    plens = [int(x) for x in rng.integers(20, 200, size=S)]
    top_lp = [[-float(x) for x in rng.random(len(t))] for t in tops] if with_lp else None
    # the token table reaches up to the EOS ids (the kernel embeds tok, and an EOS is a legal tok): random rows where the cases' ids
    # live and at the two EOS ids, zeros between
    Vt = EOS1 + 1
    table = np.zeros((Vt, H), np.uint16)
    table[:V] = draft_ref.f32_to_bf16_rne(rng.standard_normal((V, H)).astype(np.float32))
    table[[EOS0, EOS1]] = draft_ref.f32_to_bf16_rne(rng.standard_normal((2, H)).astype(np.float32))
    norm_w = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32) if S > 2 else None   # (the engine pre-normalises from 3 sequences on)
    cos_t = np.cos(np.arange(max_pos * 64, dtype=np.float32) * 0.01).reshape(max_pos, 64)
    sin_t = np.sin(np.arange(max_pos * 64, dtype=np.float32) * 0.01).reshape(max_pos, 64)
    SI, SF, SH = -77, -123.5, 0xABCD
    off = np.zeros(S + 1, np.int32)
    off[1:] = np.cumsum([len(d) for d in drafts])
    flat_d = np.asarray([t for d in drafts for t in d] + [0], np.int32)
    flat_t = np.asarray([t for tt in tops for t in tt], np.int32)
    flat_lp = np.asarray([v for tt in top_lp for v in tt], np.float32) if with_lp else None
    groups, nparts = (S + gsz - 1) // gsz, H // 16
    acc = np.zeros(2 * S, np.int32)
    out_ids = np.full((S, stride), SI, np.int32)
    out_lp = np.full((S, stride), SF, np.float32)
    state = np.zeros(4 * S + 3, np.int32)
    x_next = np.full((S, H), SF, np.float32)
    rope = np.full((S, 128), SF, np.float32)
    nn_x = np.full(groups * 32 * H, SH, np.uint16)
    nn_ss = np.full((groups, nparts, 32), SF, np.float32)
    pl = np.asarray(plens, np.int32)
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    p = lambda a, t: a.ctypes.data_as(t) if a is not None else None
    rc = lib.q3a_selftest_draft_accept(0, S, p(flat_d, i32p), p(off, i32p), p(pl, i32p), p(flat_t, i32p), p(flat_lp, f32p), stride,
                                       table.ctypes.data_as(C.c_void_p), Vt, H, p(norm_w, f32p), gsz, p(cos_t, f32p), p(sin_t, f32p), max_pos,
                                       p(acc, i32p), p(out_ids, i32p), p(out_lp, f32p) if with_lp else None, p(state, i32p), p(x_next, f32p),
                                       p(rope, f32p), nn_x.ctypes.data_as(C.c_void_p) if norm_w is not None else None,
                                       p(nn_ss, f32p) if norm_w is not None else None)
    assert rc == 0, lib.q3a_last_error(None)
    want = draft_ref.expected_state(drafts, tops, top_lp, plens, stride, table, norm_w, gsz, cos_t, sin_t, SI, SF, SH)
    assert acc.tolist() == want["accepted"].tolist()
    assert np.array_equal(out_ids, want["out_ids"])
    if with_lp:
        assert np.array_equal(out_lp.view(np.uint32), want["out_lp"].view(np.uint32))
    assert state[:S].tolist() == want["next_tok"].tolist()
    assert state[S:2 * S].tolist() == want["step_count"].tolist()
    assert state[2 * S:3 * S].tolist() == want["pos"].tolist()
    assert state[3 * S:4 * S].tolist() == want["done"].tolist()
    assert int(state[4 * S]) == want["n_done"] and (int(state[4 * S + 1]), int(state[4 * S + 2])) == want["progress"]
    assert np.array_equal(x_next.view(np.uint32), want["x_next"].view(np.uint32))
    assert np.array_equal(rope.view(np.uint32), want["rope_cur"].view(np.uint32))
    if norm_w is not None:
        assert np.array_equal(nn_x, want["nn_x"])
        # row 0: the row's sum of squares (fp32, summed in the kernel's order: H = 128 terms of size ~1 -> 128 x 2^-24 relative);
        # rows 1 ..: zeros for the live sequences, the sentinel elsewhere
        assert np.allclose(nn_ss[:, 0, :], want["nn_ss"][:, 0, :], rtol=1e-5, atol=0)
        assert np.array_equal(nn_ss[:, 1:, :].astype(np.float64), want["nn_ss"][:, 1:, :])
    if S == 2:
        assert want["progress"][1] == 1


# ---- equality with the greedy loop, tiny dimensions -------------------------------------------------------------------------
KMAX = 9


@pytest.fixture(scope="module")
def peaked40():
    """The fixture of test_gpu_eos.py (40 ragged clips in 7 length classes, stops at 1 / never / 3 / 5 / 7 / never / 2) in a directory
    of its own; the oracle's natural-EOS ids and per-step margins are computed once and shared."""
    d = peaked_checkpoint("/tmp/q3a_ckpt_draft_tinyu_peaked", "tiny_untied", seed=5)
    B = 40
    classes = [i % 7 for i in range(B)]
    clips = [synthetic.synthetic_clip(200 + i, 1.0 + 0.35 * classes[i]) for i in range(B)]
    stops, routers, info = plan_class_stops(d, clips, classes, [1, None, 3, 5, 7, None, 2], KMAX)
    ref, margins = free_run_margins(d, clips, KMAX)
    assert [len(r) for r in ref] == [KMAX if k is None else k for k in stops]
    ok_bf16 = [min(m) >= BF16_MARGIN for m in margins]
    assert sum(ok_bf16) >= 36   # at least 90 % of the utterances decide both modes
    V = O.AsrOracle(d).cfg.text.vocab_size
    return {"dir": d, "clips": clips, "ref": ref, "ok_bf16": ok_bf16, "stops": stops, "V": V}


def _drafts(kind, ref, V):
    """One draft per utterance from the oracle's ids."""
    out = []
    for u, r in enumerate(ref):
        r = list(r)
        k = kind if kind != "mix" else ["empty", "exact", "junk", "wrong_first", "substitution", "longer"][u % 6]
        if k == "empty":
            dft = []
        elif k == "exact":
            dft = r
        elif k == "junk":
            dft = r + JUNK
        elif k == "wrong_first":
            dft = ([JUNK[0]] + r[1:]) if r else [JUNK[0]]
        elif k == "substitution":
            dft = (r[:len(r) // 2] + [JUNK[1]] + r[len(r) // 2 + 1:]) if r else []
        elif k == "longer":   # the walk goes on behind the natural stop
            dft = r[:]
            while len(dft) < len(r) + 3:
                dft.append(walk_next(dft[-1] if dft else 1000, V))
        out.append([t for t in dft[:KMAX] if t not in (EOS0, EOS1, draft_ref.AUDIO_PAD)])
    return out


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("precise", [True, False])
def test_equals_the_greedy_loop_tiny_dims(peaked40, precise, use_graph):
    f = peaked40
    eng = HipEngine(f["dir"], 0, max_new_tokens=KMAX, precise=precise, use_graph=use_graph)
    compared = 0
    for B in (1, 2, 5, 40):
        sel = list(range(B)) if B != 1 else [3]
        clips, ref = [f["clips"][u] for u in sel], [f["ref"][u] for u in sel]
        use = [precise or f["ok_bf16"][u] for u in sel]
        plain = eng.transcribe_batch(clips, None, max_new=KMAX)
        for kind in ("empty", "exact", "junk", "wrong_first", "substitution", "longer", "mix"):
            drafts = _drafts(kind, ref, f["V"])
            got, acc = eng.transcribe_draft_batch(clips, drafts, None, max_new=KMAX)
            for i in range(B):
                if not use[i]:
                    continue
                tag = (precise, use_graph, B, kind, i)
                assert got[i] == plain[i] == ref[i], tag
                assert acc[i] == draft_ref.accept_from_greedy(drafts[i], ref[i], KMAX), tag
                compared += 1
        if B == 40:
            assert sum(use) >= 36
    eng.close()
    print(f"[draft] tiny precise={precise} graph={use_graph}: {compared} (utterance, draft) pairs equal to the plain call and the oracle")


@pytest.mark.parametrize("S,precise", [(1, False), (1, True), (3, True), (33, True)])
def test_empty_draft_leaves_the_state_of_a_plain_prefill(peaked40, S, precise):
    """prefill_draft with empty drafts commits one token per sequence through the accept kernel, prefill through argmax_finalize:
    both must leave the same decode state, so the two decode steps behind either are bit-equal.  S = 1 is the GEMV path (no
    pre-normalised copy of the embedding row), S = 3 and 33 the skinny path with one and two sequence groups.  The default mode
    from 3 sequences on is left out: the row's sum of squares is folded over 16 waves in finalize and over 4 in the accept kernel."""
    f = peaked40
    sel = [u for u, ok in enumerate(f["ok_bf16"]) if ok][:S]
    assert len(sel) == S
    eng = HipEngine(f["dir"], 0, max_new_tokens=KMAX, precise=precise)
    eng.mel([f["clips"][u] for u in sel]); eng.encode()
    prompts = [HipEngine.build_prompt(t) for t in eng._T]

    def two_steps():
        steps = [eng.decode_step(want_logits=True) for _ in range(2)]
        return [lg.copy() for lg, _, _ in steps], [nx.tolist() for _, nx, _ in steps], eng.fetch_ids(KMAX)

    _, nxt_plain = eng.prefill(prompts)
    plain = two_steps()
    acc, nxt_draft = eng.prefill_draft(prompts, [[]] * S)
    draft = two_steps()
    eng.close()
    assert acc.tolist() == [0] * S
    assert nxt_draft.tolist() == nxt_plain.tolist()
    for a, b in zip(plain[0], draft[0]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert draft[1] == plain[1]
    assert draft[2] == plain[2]


def test_token_logprobs_agree_with_the_plain_call(peaked40):
    f = peaked40
    sel = [0, 1, 2, 3, 4]
    clips, ref = [f["clips"][u] for u in sel], [f["ref"][u] for u in sel]
    eng = HipEngine(f["dir"], 0, max_new_tokens=KMAX, precise=True, token_logprobs=True)
    assert eng.transcribe_batch(clips, None, max_new=KMAX) == ref
    plain = eng.fetch_logprobs()
    worst = 0.0
    for kind in ("exact", "substitution", "mix"):
        got, _ = eng.transcribe_draft_batch(clips, _drafts(kind, ref, f["V"]), None, max_new=KMAX)
        assert got == ref
        lp = eng.fetch_logprobs()
        for a, b in zip(lp, plain):
            assert a.shape == b.shape and (a <= 0).all()
            if len(a):
                worst = max(worst, float(np.abs(a - b).max()))
    eng.close()
    print(f"[draft] worst |lp(draft call) - lp(plain call)| precise mode: {worst:.2e}")
    assert worst <= 1e-4


def test_logit_bias_composes_and_scoring_stays_unbiased(peaked40):
    f = peaked40
    sel = [1, 5, 8]   # never-EOS classes and a late stop: long greedy paths
    clips, ref = [f["clips"][u] for u in sel], [f["ref"][u] for u in sel]
    eng = HipEngine(f["dir"], 0, max_new_tokens=KMAX, precise=True)
    targets = [r[:4] for r in ref]
    before = eng.score_batch(clips, targets)
    allow = sorted({t for r in ref for t in r} | set(range(3000, 3040)))
    for bias, default in (({ref[0][2]: -np.inf, ref[1][1]: -np.inf}, 0.0), ({t: 0.0 for t in allow + [EOS0, EOS1]}, -np.inf)):
        eng.set_logit_bias(bias, default)
        plain = eng.transcribe_batch(clips, None, max_new=KMAX)
        if default == 0.0:
            assert plain[0] != ref[0] and ref[0][2] not in plain[0]
        for drafts in (ref, plain, _drafts("substitution", plain, f["V"]), _drafts("junk", plain, f["V"])):
            drafts = [[t for t in d[:KMAX]] for d in drafts]
            got, acc = eng.transcribe_draft_batch(clips, drafts, None, max_new=KMAX)
            assert got == plain
            assert acc == [draft_ref.accept_from_greedy(d, p, KMAX) for d, p in zip(drafts, plain)]
        mid = eng.score_batch(clips, targets)
        for a, b in zip(before, mid):
            assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b)), "q3a_score changed under a logit bias"
    eng.set_logit_bias(None)
    assert eng.transcribe_batch(clips, None, max_new=KMAX) == ref
    eng.close()


def test_rounds(peaked40):
    f = peaked40
    u = 1   # a never-EOS class: KMAX ids
    clip, r = f["clips"][u], list(f["ref"][u])
    assert len(r) == KMAX
    draft = r[:2] + [JUNK[0]] + r[3:5] + [JUNK[1]] + r[6:]
    eng = HipEngine(f["dir"], 0, max_new_tokens=KMAX, precise=True)
    p = len(HipEngine.build_prompt(eng.num_audio_tokens(len(clip))))
    accs = []
    for rounds in (1, 2, 3):
        got, acc = eng.transcribe_draft_batch([clip], [draft], None, max_new=KMAX, max_rounds=rounds, min_tail=1)
        assert got == [r]
        st = eng.draft_stats()
        assert st == {"rounds": rounds, "rows": [p + KMAX] * rounds}
        tm = eng.timings()
        assert tm["decode_steps"] == max(KMAX - 1 - acc[0], 0) and tm["prefill_ms"] > 0
        accs.append(acc[0])
    assert accs == [2, 5, KMAX]
    # a tail shorter than min_tail ends the rounds early
    got, acc = eng.transcribe_draft_batch([clip], [draft], None, max_new=KMAX, max_rounds=3, min_tail=4)
    assert got == [r] and acc == [5] and eng.draft_stats()["rounds"] == 2
    eng.close()


def _device_bytes(eng):
    return int(eng.debug_read_raw("device_bytes").view(np.uint64)[0])


def test_stage_form_state_and_refusals(peaked40):
    from align_ref import tiny_aligner_dir
    f = peaked40
    sel = [1, 3, 8]
    clips, ref = [f["clips"][u] for u in sel], [f["ref"][u] for u in sel]
    drafts = _drafts("mix", ref, f["V"])
    base = None
    for cycle in range(2):
        eng = HipEngine(f["dir"], 0, max_new_tokens=KMAX, precise=True, token_logprobs=True)
        eng.mel(clips); eng.encode()
        prompts = [HipEngine.build_prompt(t) for t in eng._T]
        acc, nxt, logits = eng.prefill_draft(prompts, drafts, want_logits=True)
        assert logits.shape == (sum(len(d) + 1 for d in drafts), f["V"])
        assert acc.tolist() == [draft_ref.accept_from_greedy(d, r, KMAX) for d, r in zip(drafts, ref)]
        # the rows are the greedy loop's: their argmax reproduces (k, tok)
        row = 0
        for b, d in enumerate(drafts):
            tops = logits[row:row + len(d) + 1].argmax(axis=1)
            assert draft_ref.accept(d, tops) == (int(acc[b]), int(nxt[b]))
            row += len(d) + 1
        # a second identical call is bit-identical
        acc2, nxt2, logits2 = eng.prefill_draft(prompts, drafts, want_logits=True)
        assert np.array_equal(acc, acc2) and np.array_equal(nxt, nxt2) and np.array_equal(logits.view(np.uint32), logits2.view(np.uint32))
        # free-running decode steps from there reproduce the whole path
        for _ in range(KMAX - 1 - int(acc.min())):
            eng.decode_step(want_logits=False)
        assert eng.fetch_ids(KMAX) == ref
        assert [len(x) for x in eng.fetch_logprobs()] == [len(r) for r in ref]
        # teacher forcing still works after a draft prefill
        eng.prefill_draft(prompts, drafts)
        eng.set_next_tokens([5, 6, 7])
        eng.decode_step(want_logits=False)
        if cycle == 1:
            assert _device_bytes(eng) == base, "device memory is not level across engine cycles"
        base = _device_bytes(eng)
        if cycle == 0:
            ok = eng.transcribe_draft_batch(clips, drafts, None, max_new=KMAX)
            V = f["V"]
            for bad, msg in (([[V], [], []], "out of range"), ([[-1], [], []], "out of range"), ([[draft_ref.AUDIO_PAD], [], []], "audio_pad"),
                             ([[5, EOS0], [], []], "EOS"), ([[EOS1], [], []], "EOS"), ([list(range(20, 20 + KMAX + 1)), [], []], "more than max_new")):
                with pytest.raises(Q3aError, match=msg):
                    eng.transcribe_draft_batch(clips, bad, None, max_new=KMAX)
                eng.mel(clips); eng.encode()   # (a whole-path call, refused or not, begins a new batch)
                with pytest.raises(Q3aError, match=msg):
                    eng.prefill_draft(prompts, bad)
                assert eng.prefill_draft(prompts, drafts)[0].tolist() == acc.tolist()
                assert eng.transcribe_draft_batch(clips, drafts, None, max_new=KMAX) == ok   # the engine stays usable
            eng.set_sampling(0.7, 0.0, 1)
            with pytest.raises(Q3aError, match="sampling"):
                eng.transcribe_draft_batch(clips, drafts, None, max_new=KMAX)
            eng.set_sampling(0.0)
            eng.set_repetition(1.3, 0)
            with pytest.raises(Q3aError, match="repetition"):
                eng.transcribe_draft_batch(clips, drafts, None, max_new=KMAX)
            eng.set_repetition(1.0, 0)
            # a live beam search owns the decode state
            eng.mel(clips[:1] * 2); eng.encode()
            eng.prefill([HipEngine.build_prompt(eng._T[0])] * 2)
            eng.beam_begin(2)
            with pytest.raises(Q3aError, match="beam"):
                eng.prefill_draft([HipEngine.build_prompt(eng._T[0])] * 2, [[], []])
            with pytest.raises(Q3aError, match="beam"):
                eng.transcribe_draft_batch(clips, drafts, None, max_new=KMAX)
            eng.prefill([HipEngine.build_prompt(eng._T[0])] * 2)   # a new prefill returns to the greedy step
            assert eng.transcribe_draft_batch(clips, drafts, None, max_new=KMAX) == ok
            assert ok[0] == ref
        eng.close()
    al = HipEngine(tiny_aligner_dir(), 0, max_new_tokens=4)
    with pytest.raises(Q3aError, match="forced aligner"):
        al.transcribe_draft_batch(clips[:1], [[1, 2]])
    al.close()


# ---- real dimensions -------------------------------------------------------------------------------------------------------
def test_real_dims_margin_report():
    """0.6B dimensions, one 5 s clip, 16 tokens, default mode: the draft is the plain ids with id 9 replaced.  Per-position engine
    logits -- the verify head's rows for positions <= k, decode_step's behind them -- against the oracle teacher-forced on the
    returned ids, under test_gpu_configs.margin_report's own LOGIT_TOL / MAX_FLIPS / MAX_UNDER_MARGIN."""
    from test_gpu_configs import margin_report
    d = synthetic.write_checkpoint("/tmp/q3a_ckpt_0p6b_peaked", "0.6b", seed=0, embed_scale=synthetic.PEAKED_EMBED_SCALE)
    clip = synthetic.synthetic_clip(0, 5.0)
    N = 16
    eng = HipEngine(d, 0, max_new_tokens=N)
    plain = eng.transcribe_batch([clip], None, max_new=N)[0]
    assert len(plain) == N and draft_ref.AUDIO_PAD not in plain
    draft = list(plain)
    draft[9] = plain[9] + 1 if plain[9] + 1 not in (EOS0, EOS1, draft_ref.AUDIO_PAD) else plain[9] - 1
    got, acc = eng.transcribe_draft_batch([clip], [draft], None, max_new=N)
    assert got[0] == plain and acc == [9]
    eng.mel([clip]); eng.encode()
    a, nxt, logits = eng.prefill_draft([HipEngine.build_prompt(eng._T[0])], [draft], want_logits=True)
    k = int(a[0])
    assert k == 9 and int(nxt[0]) == plain[9]
    L = [logits[i] for i in range(k + 1)]
    T = [int(logits[i].argmax()) for i in range(k + 1)]
    for _ in range(N - 1 - k):
        lg, nx, _ = eng.decode_step()
        L.append(lg[0].copy()); T.append(int(nx[0]))
    ids = eng.fetch_ids(N)[0]
    assert ids == plain == T
    eng.close()
    ref = O.AsrOracle(d).transcribe_ids(clip, forced_ids=ids[:N - 1], last_only=True)
    margin_report("draft 0.6B B=1 16 tokens, verify rows 0..9 + decode steps", T, L, ref)


def test_cost_sign_fully_accepted_draft_is_cheaper():
    """0.6B dimensions, one 30 s clip, max_new = 100: a fully accepted draft call takes less wall time than the plain call on the same
    engine (DESIGN section 3.8 leads one to expect more than 10 x; the factor is printed, not gated).  On this random-init checkpoint
    some steps of a 100-token run sit inside the default mode's rounding noise (test_gpu_score.py leaves up to 10 of 100 rows out), and
    there the verify head (prefill kernels) and the decode step (GEMV kernels) may pick different ids: the draft that IS fully accepted
    is found by feeding a draft call's result back as the next draft until it comes back unchanged (every pass gets past one such
    step; the passes are printed)."""
    d = synthetic.write_checkpoint("/tmp/q3a_ckpt_0p6b_peaked", "0.6b", seed=0, embed_scale=synthetic.PEAKED_EMBED_SCALE)
    clip = synthetic.synthetic_clip(0, 30.0)
    N = 100
    eng = HipEngine(d, 0, max_new_tokens=N)
    plain = eng.transcribe_batch([clip], None, max_new=N)[0]
    draft, passes, first = [t for t in plain if t != draft_ref.AUDIO_PAD][:N], 0, None
    for passes in range(1, 41):
        got, acc = eng.transcribe_draft_batch([clip], [draft], None, max_new=N)
        first = acc[0] if first is None else first
        if got[0] == draft:
            break
        assert got[0][:acc[0]] == draft[:acc[0]]
        draft = got[0]
    assert got[0] == draft and acc[0] == len(draft), "no fully accepted draft after 40 passes"
    t0 = time.perf_counter()
    eng.transcribe_batch([clip], None, max_new=N)
    t1 = time.perf_counter()
    got, acc = eng.transcribe_draft_batch([clip], [draft], None, max_new=N)
    t2 = time.perf_counter()
    tm = eng.timings()
    eng.close()
    print(f"[draft] 0.6B 1 x 30 s x {N}: plain call {1e3 * (t1 - t0):.2f} ms, fully accepted draft call {1e3 * (t2 - t1):.2f} ms "
          f"({(t1 - t0) / (t2 - t1):.1f} x; accepted {acc[0]} / {len(draft)}, decode steps {tm['decode_steps']}; the plain ids were accepted "
          f"to {first}, the settled draft took {passes} passes)")
    assert got[0] == draft and acc[0] == len(draft) and tm["decode_steps"] == max(N - 1 - acc[0], 0)
    assert t2 - t1 < t1 - t0


# ---- streaming ---------------------------------------------------------------------------------------------------------------
def _plan_shared_walk(model_dir, clips, stops, kmax, hi=30.0, lo=-10.0):
    """plan_class_stops with ONE walk for all clips (a stream's "audio so far" keeps its transcript): one router row that wins step 0
    for every clip, and the <|endoftext|> row planted to win at clip u's stop step only -- the clips share their token history, so
    what tells them apart is the prompt length (other RoPE phases), as for the router rows of the class fixture."""
    orc = O.AsrOracle(model_dir)
    V = orc.cfg.text.vocab_size
    walk = [1000]
    while len(walk) < kmax:
        walk.append(walk_next(walk[-1], V))
    states, owner, peak = [], [], 0.0
    for u, clip in enumerate(clips):
        last = kmax - 1 if stops[u] is None else stops[u]
        r = orc.transcribe_ids(clip, forced_ids=walk[:last], want_hidden=True, last_only=True)
        for s in range(last + 1):
            states.append(r.step_hidden[s].numpy()); owner.append((u, s))
        peak = max(peak, max(float(l.max()) for l in r.step_logits[:last + 1]))
    Hm = np.stack(states).astype(np.float64)
    key = synthetic.output_embedding_key(model_dir)
    for tok, fire in ((walk[0], [s == 0 for _, s in owner]), (synthetic.ENDOFTEXT_ID, [stops[u] is not None and s == stops[u] for u, s in owner])):
        fire = np.asarray(fire, dtype=bool)
        w, *_ = np.linalg.lstsq(Hm, np.where(fire, hi, lo), rcond=1e-4)
        stored = synthetic.overwrite_row(model_dir, key, tok, w.astype(np.float32))
        got = Hm @ stored.astype(np.float64)
        assert got[fire].min() > peak + 10.0 and got[~fire].max() < -2.0, (tok, got[fire].min(), got[~fire].max(), peak)
    return walk


def test_streaming_updates_equal_the_plain_transcripts():
    """A clip pushed in three pieces whose "audio so far" stops at 3, then never, then 5: every update equals the plain transcript of
    the audio so far, and accepted is 0, 3 and 5."""
    d = peaked_checkpoint("/tmp/q3a_ckpt_draft_stream_peaked", "tiny_untied", seed=5, peak=18.0)   # (peak 14: step 1 of the walk has a margin of 0.9)
    kmax = 8
    whole = synthetic.synthetic_clip(77, 2.4)
    cuts = [int(16000 * 1.0), int(16000 * 1.7), len(whole)]
    sofar = [whole[:c] for c in cuts]
    stops = [3, None, 5]
    walk = _plan_shared_walk(d, sofar, stops, kmax)
    ref, margins = free_run_margins(d, sofar, kmax)
    assert ref == [walk[:3], walk[:kmax], walk[:5]]
    assert min(min(m) for m in margins) >= BF16_MARGIN
    asr = AsrInference(HipEngine(d, 0, max_new_tokens=kmax), None)
    st = StreamingTranscriber(asr, max_new_tokens=kmax)
    prev = 0
    for i, c in enumerate(cuts):
        up = st.push(whole[prev:c])
        prev = c
        assert up.result.ids == ref[i] == asr.transcribe(sofar[i], max_new_tokens=kmax).ids
        assert up.accepted == [0, 3, 5][i] and up.audio_seconds == pytest.approx(c / 16000.0)
    asr.engine.close()


# ---- CLI -------------------------------------------------------------------------------------------------------------------
def test_cli_accepted_line(tiny_dir, tmp_path):
    """`asr` with a language argument and Q3A_DRAFT_TEXT: the same Language / Text lines as without it, then `Accepted: k / n` with
    the Python API's k."""
    from qwen3_asr_rs_amd.build import CLI_PATH
    mdir = tmp_path / "model"
    mdir.mkdir()
    for fn in os.listdir(tiny_dir):
        if fn.endswith((".json", ".safetensors")):
            os.symlink(os.path.join(tiny_dir, fn), mdir / fn)
    special = {151643: "<|endoftext|>", 151645: "<|im_end|>", 151704: "<asr_text>"}
    vocab = {f"t{i}": i for i in range(151936) if i not in special}
    for j, ch in enumerate("abcdefghijklmnopqrstuvwxyz"):
        del vocab[f"t{1000 + j}"]
        vocab[ch] = 1000 + j
    del vocab["t220"], vocab["t1100"]
    vocab["Ġ"], vocab["E"] = 220, 1100
    tok = {"version": "1.0", "added_tokens": [{"id": i, "content": c, "special": True} for i, c in special.items()],
           "model": {"type": "BPE", "vocab": vocab, "merges": []}}
    (mdir / "tokenizer.json").write_text(json.dumps(tok))
    text = "hello world"
    (tmp_path / "draft.txt").write_text(text + "\n")
    wav = os.path.join(GOLDEN, "sample1.wav")
    env = {k: v for k, v in os.environ.items() if not k.startswith("Q3A_")}
    env["RUST_LOG"] = "warn"
    cmd = [CLI_PATH, str(mdir), wav, "english"]
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert plain.returncode == 0, plain.stderr
    drafted = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(env, Q3A_DRAFT_TEXT=str(tmp_path / "draft.txt")))
    assert drafted.returncode == 0, drafted.stderr
    a, b = plain.stdout.split("\n"), drafted.stdout.split("\n")
    assert len(a) == 3 and a[0].startswith("Language: ") and a[1].startswith("Text: ") and a[2] == ""
    assert len(b) == 4 and b[:2] == a[:2] and b[3] == ""
    assert plain.stderr == drafted.stderr
    m = re.fullmatch(r"Accepted: (\d+) / (\d+)", b[2])
    assert m, b[2]
    asr = AsrInference.load(str(mdir), 0)
    res = asr.transcribe(wav, language="english", draft=text)
    plain_res = asr.transcribe(wav, language="english")
    asr.engine.close()
    assert res.ids == plain_res.ids and res.text == plain_res.text
    assert (int(m.group(1)), int(m.group(2))) == (res.accepted_draft_tokens, 1 + len(text))
    nolang = subprocess.run(cmd[:3], capture_output=True, text=True, timeout=300, env=dict(env, Q3A_DRAFT_TEXT=str(tmp_path / "draft.txt")))
    assert nolang.returncode != 0 and "language" in nolang.stderr
