"""Beam search on the GPU (q3a_beam_*; csrc/k_beam.hip): the three kernels on their own, the rounds of the stage API replayed
against tests/beam_ref.py, the whole path against the greedy loop (W = 1), against q3a_score (the histories) and against a CPU
beam search over the fp32 oracle, graph replay against eager launches, the refusals, and the CLI / AsrInference front doors."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from qwen3_asr_rs_amd import synthetic
from qwen3_asr_rs_amd.engine import AsrInference, HipEngine, Q3aError

from beam_ref import EOS_IDS, beam_round, initial_state, oracle_beam_search, plant_beam_stops, topk_ref
from eos_plan import peaked_checkpoint, plan_class_stops

pytestmark = pytest.mark.gpu

V = 151936
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_audio")


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _err(lib):
    return (lib.q3a_last_error(None) or b"").decode()


# ---- 1. top-W of rows ------------------------------------------------------------------------------------------------
def _row(kind, Vn, W, rng):
    if kind == 1:
        return np.full(Vn, 0.5, np.float32)  # all equal: ids 0 .. W-1
    x = (rng.standard_normal(Vn) * 3).astype(np.float32)
    if kind == 2:
        x[0] = x[Vn - 1] = 50.0  # maxima at id 0 and id V-1
    elif kind == 3:
        x[Vn // 2:Vn // 2 * 2] = x[:Vn // 2]  # the upper half a copy of the lower
    elif kind == 4:
        keep = rng.choice(Vn, size=W, replace=False)  # -inf everywhere but W entries
        y = np.full(Vn, -np.inf, np.float32)
        y[keep] = x[keep]
        x = y
    elif kind == 5:
        # values spread over +-1e4: the log-sum must not overflow.  lp is an fp32 number: beyond |lp| ~ 1000 half an ulp of the RESULT
        # exceeds the 1e-4 bound whatever the kernel does, so the W entries that are selected lie within 8 of the maximum and the
        # spread is everything below them
        x = rng.uniform(-1e4, 1e4 - 16.0, Vn).astype(np.float32)
        top = rng.choice(Vn, size=W, replace=False)
        x[top] = (1e4 - rng.uniform(0.0, 8.0, W)).astype(np.float32)
    return x


def _check_topk(logits, W, ids, lp, tag):
    ref_ids, ref_lp = topk_ref(logits, W)
    assert np.array_equal(ids, ref_ids), tag
    assert np.all(np.isfinite(lp)), tag
    err = float(np.abs(lp.astype(np.float64) - ref_lp).max())
    assert err <= 1e-4, (tag, err)
    return err


@pytest.mark.parametrize("S,Vn,W", [(1, V, 1), (1, V, 8), (2, V, 4), (32, V, 4), (3, 1000, 3), (5, 65, 8), (1, 8, 8)])
def test_topk_kernel_alone(lib, S, Vn, W):
    rng = np.random.default_rng(S * 1000 + W)
    kinds = list(range(7))  # 0 and 6: plain random rows
    worst = 0.0
    for first in range(0, 7, S):  # every kind of row at least once, S rows per call
        x = np.stack([_row(kinds[(first + s) % 7], Vn, W, rng) for s in range(S)])
        ids = np.zeros((S, W), np.int32)
        lp = np.zeros((S, W), np.float32)
        assert lib.q3a_selftest_beam_topk(0, _p(x, C.c_float), S, Vn, W, _p(ids, C.c_int32), _p(lp, C.c_float)) == 0, _err(lib)
        worst = max(worst, _check_topk(x, W, ids, lp, (S, Vn, W, first)))
        for s in range(S):
            if kinds[(first + s) % 7] == 1:
                assert ids[s].tolist() == list(range(W))
    print(f"[beam] top-W S={S} V={Vn} W={W}: worst |lp - float64 log_softmax| {worst:.2e}")
    bad = np.zeros((1, 4), np.float32)
    assert lib.q3a_selftest_beam_topk(0, _p(bad, C.c_float), 1, 4, 8, _p(np.zeros(8, np.int32), C.c_int32), _p(np.zeros(8, np.float32), C.c_float)) != 0


# ---- 2. the advance kernel -------------------------------------------------------------------------------------------
def _advance(lib, U, W, ids, lp, score, finished):
    S = U * W
    ids, lp = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(lp, np.float32)
    score, finished = np.ascontiguousarray(score, np.float32), np.ascontiguousarray(finished, np.uint8)
    par, tok, sc, fin = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.float32), np.zeros(S, np.uint8)
    assert lib.q3a_selftest_beam_advance(0, U, W, _p(ids, C.c_int32), _p(lp, C.c_float), _p(score, C.c_float), _p(finished, C.c_uint8),
                                         _p(par, C.c_int32), _p(tok, C.c_int32), _p(sc, C.c_float), _p(fin, C.c_uint8)) == 0, _err(lib)
    return {"parent": par, "token": tok, "score": sc, "finished": fin}


def _bit_equal(got, want, tag):
    for k in ("parent", "token", "finished"):
        assert np.array_equal(got[k], want[k]), (tag, k, got[k].tolist(), want[k].tolist())
    assert np.array_equal(got["score"].view(np.uint32), want["score"].view(np.uint32)), (tag, got["score"].tolist(), want["score"].tolist())


def test_advance_kernel_alone(lib):
    rng = np.random.default_rng(11)
    cases = []
    W = 4
    base_ids = np.tile(np.array([10, 20, 30, 40], np.int32), (W, 1))
    base_lp = np.tile(np.array([-0.1, -0.7, -1.3, -2.9], np.float32), (W, 1))
    sc0, fin0 = initial_state(2, W)
    cases.append(("round 0", 2, W, np.tile(base_ids, (2, 1)), np.tile(base_lp, (2, 1)), sc0, fin0))
    cases.append(("all survivors from one parent", 1, W, base_ids, base_lp, [-50, 0, -50, -50], [0, 0, 0, 0]))
    for eos in EOS_IDS:
        ids = base_ids.copy()
        ids[2, 0] = eos
        cases.append((f"a finish by {eos}", 1, W, ids, base_lp, [-1, -2, -0.5, -3], [0, 0, 0, 0]))
    cases.append(("a finished slot survives", 1, W, base_ids, base_lp, [-1, -1.2, -3, -4], [0, 1, 0, 0]))
    cases.append(("a finished slot is displaced", 1, W, base_ids, base_lp, [-1, -30, -1.5, -2], [0, 1, 0, 0]))
    cases.append(("all finished", 2, W, np.tile(base_ids, (2, 1)), np.tile(base_lp, (2, 1)), [-1, -2, -3, -4, -4, -3, -2, -1], [1] * 8))
    tie_lp = np.tile(np.array([-0.5, -0.5, -1.0, -1.0], np.float32), (W, 1))
    cases.append(("equal scores across parents and tokens", 1, W, base_ids, tie_lp, [-1, -1, -1.5, -1], [0, 0, 0, 1]))
    cases.append(("an empty slot", 1, W, base_ids, base_lp, [-1, -np.inf, -2, -np.inf], [0, 0, 0, 0]))
    for U, Wr in ((32, 1), (4, 8), (3, 3), (16, 2), (5, 5), (1, 7)):  # (more utterances than the kernel has waves: 32, 16)
        for _ in range(4):
            S = U * Wr
            ids = np.stack([rng.choice(50, size=Wr, replace=False) for _ in range(S)]).astype(np.int32)
            for s in np.flatnonzero(rng.random(S) < 0.2):  # (ids of a row are distinct: at most one EOS)
                ids[s, rng.integers(Wr)] = EOS_IDS[int(rng.integers(2))]
            lp = -np.sort(rng.integers(0, 6, size=(S, Wr)) * 0.5, axis=1).astype(np.float32)
            score = (-rng.integers(0, 5, size=S) * 0.5).astype(np.float32)
            finished = (rng.random(S) < 0.3).astype(np.uint8)
            cases.append((f"random U={U} W={Wr}", U, Wr, ids, lp, score, finished))
    for tag, U, Wc, ids, lp, score, finished in cases:
        _bit_equal(_advance(lib, U, Wc, ids, lp, score, finished), beam_round(ids, lp, score, finished, Wc), tag)


# ---- 3. the KV reorder kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem", [2, 4])
def test_kv_reorder_kernel_alone(lib, elem):
    layers, U, W, n_kv, max_ctx = 2, 2, 4, 2, 128
    S = U * W
    lo = np.repeat(np.array([5, 17], np.int32), W)
    hi = np.repeat(np.array([9, 40], np.int32), W)
    # [K | V][layer][sequence][head][row][128 * elem bytes]: random bytes, so every (layer, K/V, sequence, head, row) is its own pattern
    shape = (2, layers, S, n_kv, max_ctx, 128 * elem)
    before = np.random.default_rng(elem).integers(0, 256, size=shape, dtype=np.uint8)
    assert len({before[w, l, s, h, r].tobytes() for w in range(2) for l in range(layers) for s in range(S) for h in range(n_kv) for r in (5, 9, 17, 40)}) == 2 * layers * S * n_kv * 4
    slots = {"identity": ([0, 1, 2, 3], [0, 1, 2, 3]), "a two-cycle": ([1, 0, 2, 3], [0, 3, 2, 1]), "a four-cycle": ([1, 2, 3, 0], [3, 0, 1, 2]),
             "all from slot 3": ([3, 3, 3, 3], [3, 3, 3, 3]), "a mix": ([0, 0, 3, 1], [2, 1, 1, 2])}
    for tag, (p0, p1) in slots.items():
        parent = np.array(p0 + [W + j for j in p1], np.int32)
        cache = before.copy()
        assert lib.q3a_selftest_kv_reorder(0, cache.ctypes.data_as(C.c_void_p), elem, layers, S, n_kv, max_ctx, _p(lo, C.c_int32), _p(hi, C.c_int32),
                                           _p(parent, C.c_int32)) == 0, _err(lib)
        want = before.copy()
        for s in range(S):
            if parent[s] != s:
                want[:, :, s, :, lo[s]:hi[s] + 1] = before[:, :, parent[s], :, lo[s]:hi[s] + 1]
        assert np.array_equal(cache, want), tag  # rows inside [lo, hi] are the parent's old rows, every other byte is unchanged
    bad = np.array([4, 1, 2, 3, 4, 5, 6, 7], np.int32)  # a parent in another utterance (other rows)
    assert lib.q3a_selftest_kv_reorder(0, before.copy().ctypes.data_as(C.c_void_p), elem, layers, S, n_kv, max_ctx, _p(lo, C.c_int32), _p(hi, C.c_int32),
                                       _p(bad, C.c_int32)) != 0


# ---- 4. rounds replayed ------------------------------------------------------------------------------------------------
def _clip(i):
    return synthetic.synthetic_clip(i, 1.0 + 0.25 * (i % 7))


@pytest.mark.parametrize("precise", [True, False])
@pytest.mark.parametrize("U,W", [(1, 2), (1, 3), (1, 5), (2, 8), (8, 4)])
def test_rounds_replayed(tiny_dir, U, W, precise):
    S = U * W
    clips = [_clip(300 + u) for u in range(U) for _ in range(W)]
    eng = HipEngine(tiny_dir, 0, precise=precise, max_new_tokens=8)
    eng.mel(clips)
    eng.encode()
    logits, _ = eng.prefill([HipEngine.build_prompt(t) for t in eng._T])
    score, finished = initial_state(U, W)
    worst = 0.0
    for rnd in range(6):
        if rnd == 0:
            eng.beam_begin(W)
        else:
            _, logits = eng.beam_step(want_logits=True)
        dbg = eng.beam_debug()
        assert dbg["topk_ids"].shape == (S, W) and dbg["stats"][0] == rnd + 1
        worst = max(worst, _check_topk(logits, W, dbg["topk_ids"], dbg["topk_lp"], (U, W, precise, rnd)))
        want = beam_round(dbg["topk_ids"], dbg["topk_lp"], score, finished, W)
        _bit_equal(dbg, want, (U, W, precise, rnd))
        score, finished = dbg["score"].copy(), dbg["finished"].copy()
    hyps = eng.beam_fetch()
    assert [len(h) for h in hyps] == [W] * U and all(len(x.ids) == 6 and not x.finished for h in hyps for x in h)
    for u in range(U):
        assert [x.score for x in hyps[u]] == sorted((float(v) for v in score[u * W:(u + 1) * W]), reverse=True)
        for x in hyps[u]:  # one fp32 add per round, in order
            acc = np.float32(0)
            for v in x.token_logprobs:
                acc = np.float32(acc + np.float32(v))
            assert float(acc) == x.score
    eng.close()
    print(f"[beam] rounds U={U} W={W} precise={precise}: worst |lp - float64 log_softmax| {worst:.2e}")


# ---- 5. W = 1 is the greedy loop -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged():
    """7 clips in 7 length classes on a peaked checkpoint with planted stops (as tests/test_gpu_eos.py)."""
    d = peaked_checkpoint("/tmp/q3a_ckpt_tinyu_beam_ragged", "tiny_untied", seed=5)
    kmax = 9
    classes = list(range(7))
    clips = [synthetic.synthetic_clip(200 + i, 1.0 + 0.35 * classes[i]) for i in range(7)]
    stops, _, _ = plan_class_stops(d, clips, classes, [1, None, 3, 5, 7, None, 2], kmax)
    return d, clips, kmax, stops


@pytest.mark.parametrize("use_graph", [True, False])
def test_width_one_is_the_greedy_loop(tiny_dir, ragged, use_graph):
    clips = [_clip(300 + i) for i in range(5)]
    for precise in (False, True):
        for sel in (clips, clips[:2], clips[:1]):  # skinny path, GEMV path with two sequences, one sequence
            eng = HipEngine(tiny_dir, 0, precise=precise, max_new_tokens=8, use_graph=use_graph)
            want = eng.transcribe_batch(sel, None, max_new=8)
            got = eng.beam_search_batch(sel, 1, max_new=8)
            assert [h[0].ids for h in got] == want and all(not h[0].finished for h in got)
            eng.close()
    d, rclips, kmax, stops = ragged
    for precise in (False, True):
        eng = HipEngine(d, 0, precise=precise, max_new_tokens=kmax, use_graph=use_graph)
        want = eng.transcribe_batch(rclips, None, max_new=kmax)
        got = eng.beam_search_batch(rclips, 1, max_new=kmax)
        assert [h[0].ids for h in got] == want
        assert [h[0].finished for h in got] == [len(w) < kmax for w in want]
        if precise:
            assert [len(w) for w in want] == [kmax if k is None else k for k in stops]
        assert eng.timings()["decode_steps"] == eng.beam_debug()["stats"][0] - 1
        eng.close()


# ---- 6. / 7. histories and the oracle ------------------------------------------------------------------------------------
_REF = {}


def _ref_search(orc, i, W):
    if (i, W) not in _REF:
        _REF[i, W] = oracle_beam_search(orc, _clip(i), W, 8)
    return _REF[i, W]


def _score_diffs(eng, clips, hyps):
    """Worst |lp of the search - q3a_score_batch_ptrs of the same ids on the same clip| over every token of every hypothesis."""
    worst = 0.0
    for clip, hs in zip(clips, hyps):
        res = eng.score_batch([clip] * len(hs), [h.ids + ([EOS_IDS[1]] if h.finished else []) for h in hs])
        for h, (lp, _, _) in zip(hs, res):
            n = len(h.ids)
            worst = max(worst, float(np.abs(lp[:n].astype(np.float64) - h.token_logprobs[:n].astype(np.float64)).max()))
    return worst


def test_histories_are_the_right_ones(tiny_dir, tiny_oracle):
    """A reorder bug leaves a hypothesis with another slot's KV rows: its later log-probabilities then differ from a fresh prefill of
    its own ids (q3a_score_batch_ptrs).

    Measured on the MI355X: precise mode worst difference 4.8e-6 (bound 2e-4) with 36 history copies; default
    mode d0 = 2.07e-3 on the greedy ids, 3.63e-3 on the beams' tokens (bound 2 d0 + 1e-5 = 4.15e-3)."""
    idx = [300, 302, 303]
    clips = [_clip(i) for i in idx]
    eng = HipEngine(tiny_dir, 0, precise=True, max_new_tokens=8)
    hyps = eng.beam_search_batch(clips, 4, max_new=8)
    stats = eng.beam_debug()["stats"]
    worst = _score_diffs(eng, clips, hyps)
    eng.close()
    ref_copies = sum(_ref_search(tiny_oracle, i, 4)[1] for i in idx)
    print(f"[beam] histories, precise: worst |beam lp - score lp| {worst:.2e}; copies {stats[1]} (reference {ref_copies}), KV rows copied {stats[2]}")
    assert worst <= 2e-4
    assert stats[1] == ref_copies and stats[1] > 0 and stats[2] > 0
    # default mode: the error of the same two paths on the greedy ids first, then the beams' (lower-probability) tokens
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8, token_logprobs=True)
    greedy = eng.transcribe_batch(clips, None, max_new=8, fixed_new_tokens=8)
    glp = eng.fetch_logprobs()
    res = eng.score_batch(clips, greedy)
    d0 = max(float(np.abs(res[b][0].astype(np.float64) - glp[b].astype(np.float64)).max()) for b in range(len(clips)))
    hyps = eng.beam_search_batch(clips, 4, max_new=8)
    assert eng.beam_debug()["stats"][1] > 0
    worst = _score_diffs(eng, clips, hyps)
    eng.close()
    print(f"[beam] histories, default mode: d0 (greedy ids) {d0:.2e}; worst over the beams' tokens {worst:.2e}; bound {2 * d0 + 1e-5:.2e}")
    assert worst <= 2 * d0 + 1e-5


@pytest.mark.parametrize("W,idx", [(4, [300, 302, 303, 307, 315, 321]), (3, [300, 301, 302, 303, 304, 305])])
def test_against_the_oracle(tiny_dir, tiny_oracle, W, idx):
    refs = [_ref_search(tiny_oracle, i, W) for i in idx]
    for i, (_, copies, gap) in zip(idx, refs):  # the clips were chosen for this: every candidate gap down to rank W + 1 exceeds 1e-3
        assert gap > 1e-3, (i, W, gap)
    eng = HipEngine(tiny_dir, 0, precise=True, max_new_tokens=8)
    hyps = eng.beam_search_batch([_clip(i) for i in idx], W, max_new=8)
    stats = eng.beam_debug()["stats"]
    eng.close()
    worst = 0.0
    for i, hs, (ref, _, _) in zip(idx, hyps, refs):
        assert len(hs) == len(ref) == W
        for k, (h, r) in enumerate(zip(hs, ref)):
            assert h.ids == r["ids"] and int(h.finished) == r["finished"], (i, W, k)
            worst = max(worst, abs(h.score - r["score"]))
            assert abs(h.score - r["score"]) <= 2e-4, (i, W, k, h.score, r["score"])
    assert stats[1] == sum(c for _, c, _ in refs)
    print(f"[beam] oracle W={W}: smallest gap {min(g for _, _, g in refs):.2e}; worst |score - reference| {worst:.2e}; copies {stats[1]}")


# ---- 8. graph replay equals eager ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def beam_planted():
    """U 3 x W 4 on a peaked checkpoint whose EOS row makes every hypothesis of utterance u stop in round (3, 5, 6)[u]."""
    d = peaked_checkpoint("/tmp/q3a_ckpt_tinyu_beam_stops", "tiny_untied", seed=5)
    clips = [synthetic.synthetic_clip(200 + i, 1.0 + 0.35 * i) for i in range(3)]
    fire, quiet = plant_beam_stops(d, clips, 4, [3, 5, 6], 8, hi=40.0)
    assert fire > 32.0 and quiet < -5.0, (fire, quiet)
    return d, clips


def _flat(hyps):
    return [(h.ids, np.float32(h.score).tobytes(), h.finished, h.token_logprobs.tobytes()) for hs in hyps for h in hs]


def test_graph_replay_equals_eager(beam_planted):
    d, clips = beam_planted
    runs = {}
    for use_graph in (True, False):
        eng = HipEngine(d, 0, precise=True, max_new_tokens=8, use_graph=use_graph)
        for max_new in (8, 5):
            hyps = eng.beam_search_batch(clips, 4, max_new=max_new)
            runs[use_graph, max_new] = (_flat(hyps), eng.beam_debug()["stats"].tolist(), eng.timings()["decode_steps"], hyps)
        eng.close()
    for max_new in (8, 5):
        assert runs[True, max_new][:3] == runs[False, max_new][:3], f"hipGraph replay and eager launches disagree (max_new {max_new})"
    _, stats, steps, hyps = runs[True, 8]
    # ended by "all finished": fewer rounds than the limit, every hypothesis finished, and the first utterance finished while others lived
    assert stats[0] == 7 and steps == 6 and stats[3] == 12 and all(h.finished for hs in hyps for h in hs)
    assert [max(len(h.ids) for h in hs) for hs in hyps] == [3, 5, 6]
    _, stats, steps, hyps = runs[True, 5]
    # ended by the round limit: utterance 0 is finished, the others live with max_new ids
    assert stats[0] == 5 and steps == 4 and stats[3] == 4
    assert all(h.finished for h in hyps[0]) and all(not h.finished and len(h.ids) == 5 for hs in hyps[1:] for h in hs)


def test_no_stale_beam_graph_across_shapes(tiny_dir):
    """One graph engine searches shape A (1 clip x width 2, 6 rounds), then B (2 clips x width 4, 12 rounds, longer clips), then A
    again; every search equals an eager engine's, bit for bit.  B regrows the beam tables (history, candidates) inside beam_begin,
    after setup_prompts has already swept for reallocations, so a graph captured for A must not replay on the freed addresses
    (the greedy twin: tests/test_gpu_logprobs.py::test_no_stale_graph_across_batch_shapes)."""
    shapes = {"A": ([synthetic.synthetic_clip(410, 1.25)], 2, 6), "B": ([synthetic.synthetic_clip(420 + i, 2.0) for i in range(2)], 4, 12)}
    eager = HipEngine(tiny_dir, 0, max_new_tokens=12, use_graph=False)
    want = {name: eager.beam_search_batch(clips, W, max_new=k) for name, (clips, W, k) in shapes.items()}
    eager.close()
    eng = HipEngine(tiny_dir, 0, max_new_tokens=12, use_graph=True)
    for name in ("A", "B", "A"):
        clips, W, k = shapes[name]
        got = eng.beam_search_batch(clips, W, max_new=k)
        assert [len(hs) for hs in got] == [W] * len(clips), name
        for hs, ws in zip(got, want[name]):
            for h, w in zip(hs, ws):
                assert h.ids == w.ids and len(h.ids) == len(w.ids) and h.finished == w.finished, name
                assert np.float32(h.score).view(np.uint32) == np.float32(w.score).view(np.uint32), name
                assert np.array_equal(np.asarray(h.token_logprobs, np.float32).view(np.uint32), np.asarray(w.token_logprobs, np.float32).view(np.uint32)), name
    eng.close()


# ---- 9. refusals and state ---------------------------------------------------------------------------------------------
def test_refusals_and_state(lib, tiny_dir):
    from align_ref import tiny_aligner_dir
    clips = [_clip(300 + i) for i in range(3)]
    probe = HipEngine(tiny_dir, 0, max_new_tokens=8)
    probe.transcribe_batch(clips, None, max_new=8)
    probe.beam_search_batch(clips, 4, max_new=8)
    level = int(probe.debug_read_raw("device_bytes").view(np.uint64)[0])
    extra = HipEngine(tiny_dir, 0, max_new_tokens=8)
    extra.beam_search_batch(clips, 4, max_new=8)
    assert int(probe.debug_read_raw("device_bytes").view(np.uint64)[0]) > level
    extra.close()
    assert int(probe.debug_read_raw("device_bytes").view(np.uint64)[0]) == level  # create / destroy leaves it level
    probe.close()
    eng = HipEngine(tiny_dir, 0, max_new_tokens=8)
    with pytest.raises(Q3aError, match="before any beam search"):
        eng.debug_read_raw("beam_stats")
    before = eng.transcribe_batch(clips, None, max_new=8)
    for w in (0, 9):
        with pytest.raises(Q3aError, match="width must be 1..8"):
            eng.beam_search_batch(clips, w, max_new=8)
    with pytest.raises(Q3aError, match="exceeds 32"):
        eng.beam_search_batch(clips * 3, 4, max_new=8)
    # stride < max_new (the Python layer sizes its buffers itself: straight through the C ABI)
    arrs, ptrs, ns = HipEngine._ptrs(clips)
    ids, lens = np.zeros((3, 2, 4), np.int32), np.zeros((3, 2), np.int32)
    assert lib.q3a_beam_search_batch_ptrs(eng._h, ptrs, ns.ctypes.data_as(C.POINTER(C.c_int64)), 3, None, 0, 2, 8, _p(ids, C.c_int32), 4, _p(lens, C.c_int32),
                                          None, None, None) != 0
    assert b"stride" in lib.q3a_last_error(eng._h)
    with pytest.raises(Q3aError, match="q3a_beam_begin"):
        eng.beam_step()
    with pytest.raises(Q3aError, match="q3a_beam_begin"):
        eng._beam_width = 2
        eng.beam_fetch()
    eng.mel(clips)
    eng.encode()
    prompts = [HipEngine.build_prompt(t) for t in eng._T]
    eng.prefill(prompts)
    with pytest.raises(Q3aError, match="not divisible"):
        eng.beam_begin(2)
    eng.mel([clips[0], clips[1]])
    eng.encode()
    eng.prefill([HipEngine.build_prompt(t) for t in eng._T])
    with pytest.raises(Q3aError, match="differ in length"):
        eng.beam_begin(2)
    # a search owns the decode state; afterwards there is none until the next prefill
    eng.mel([clips[0], clips[0]])
    eng.encode()
    eng.prefill([HipEngine.build_prompt(t) for t in eng._T])
    eng.beam_begin(2)
    with pytest.raises(Q3aError, match="beam search owns"):
        eng.decode_step()
    with pytest.raises(Q3aError, match="no decode state"):
        eng.set_next_tokens([1, 2])
    a = eng.beam_search_batch(clips, 4, max_new=8)
    tm = eng.timings()
    assert tm["decode_steps"] == 7 and tm["batch"] == 12 and tm["mel_ms"] > 0 and tm["encoder_ms"] > 0 and tm["prefill_ms"] > 0 and tm["decode_ms"] > 0
    with pytest.raises(Q3aError, match="no prefill state"):
        eng.decode_step()
    with pytest.raises(Q3aError, match="nothing generated"):
        eng.fetch_ids(4)
    assert eng.transcribe_batch(clips, None, max_new=8) == before  # the greedy path is what it was
    b = eng.beam_search_batch(clips, 4, max_new=8)
    assert _flat(a) == _flat(b)  # two beam calls: identical bits
    assert eng.transcribe_batch(clips[:1], None, max_new=8) == before[:1]
    eng.close()
    al = HipEngine(tiny_aligner_dir(), 0, max_new_tokens=4)
    with pytest.raises(Q3aError, match="forced aligner"):
        al.beam_search_batch(clips[:1], 2, max_new=4)
    with pytest.raises(Q3aError, match="forced aligner"):
        al.beam_begin(2)
    al.close()


# ---- 10. the front doors -----------------------------------------------------------------------------------------------
def test_cli_hyp_lines_and_asr_inference(tiny_dir, tmp_path):
    """`Q3A_BEAM=4 asr <model> <wav> english` prints one `Hyp k: <score> <text>` line per hypothesis after `Text:`; the values are
    those of AsrInference.transcribe(beam_size=4)."""
    from qwen3_asr_rs_amd.build import CLI_PATH
    mdir = tmp_path / "model"
    mdir.mkdir()
    cfg = json.load(open(os.path.join(tiny_dir, "config.json")))
    for f in os.listdir(tiny_dir):
        if f.endswith((".json", ".safetensors")):
            os.symlink(os.path.join(tiny_dir, f), mdir / f)
    special = {151643: "<|endoftext|>", 151645: "<|im_end|>", 151704: "<asr_text>"}
    vocab = {f"t{i}": i for i in range(151936) if i not in special}
    del vocab["t220"], vocab["t1100"]
    vocab["Ġ"], vocab["E"] = 220, 1100  # the byte-level space; the capital of the prefix "language English"
    for j, ch in enumerate("abcdefghijklmnopqrstuvwxyz"):
        del vocab[f"t{1000 + j}"]
        vocab[ch] = 1000 + j
    tok = {"version": "1.0", "added_tokens": [{"id": i, "content": c, "special": True} for i, c in special.items()],
           "model": {"type": "BPE", "vocab": vocab, "merges": []}}
    (mdir / "tokenizer.json").write_text(json.dumps(tok))
    wav = os.path.join(GOLDEN, "sample1.wav")
    env = {k: v for k, v in os.environ.items() if k not in ("Q3A_SCORE_TEXT", "Q3A_TOKEN_LOGPROBS", "Q3A_ALIGNER", "Q3A_BEAM")}
    env["RUST_LOG"] = "warn"
    cmd = [CLI_PATH, str(mdir), wav, "english"]
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert plain.returncode == 0, plain.stderr
    beam = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(env, Q3A_BEAM="4"))
    assert beam.returncode == 0, beam.stderr
    a, b = plain.stdout.split("\n"), beam.stdout.split("\n")
    assert len(a) == 3 and len(b) == 7 and b[:2] == a[:2] and b[6] == "" and plain.stderr == beam.stderr
    asr = AsrInference.load(str(mdir), 0)
    res = asr.transcribe(wav, language="english", beam_size=4)
    assert len(res.alternatives) == 4 and res.ids == res.alternatives[0].ids and res.text == res.alternatives[0].text
    assert [x.score for x in res.alternatives] == sorted((x.score for x in res.alternatives), reverse=True)
    for k, (line, alt) in enumerate(zip(b[2:6], res.alternatives)):
        m = re.fullmatch(r"Hyp (\d): (-?\d+\.\d{6}) (.*)", line)
        assert m and int(m.group(1)) == k, line
        assert float(m.group(2)) == pytest.approx(alt.score, abs=1e-6) and m.group(3) == alt.text
    assert asr.transcribe(wav, language="english", max_new_tokens=16).alternatives is None
    short = asr.transcribe(wav, language="english", max_new_tokens=16, beam_size=4)
    ranked = asr.transcribe(wav, language="english", max_new_tokens=16, beam_size=4, length_penalty=1.0)
    assert sorted(tuple(x.ids) for x in ranked.alternatives) == sorted(tuple(x.ids) for x in short.alternatives)
    assert all(len(x.ids) == 16 for x in short.alternatives)
    bad = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(env, Q3A_BEAM="9"))
    assert bad.returncode != 0 and "width must be 1..8" in bad.stderr
