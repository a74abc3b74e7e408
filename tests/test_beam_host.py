"""Beam search (q3a_beam_*) without a GPU: the symbols are declared, exported and bound, the header states the contract's refusals,
and the reference round the GPU tests replay (tests/beam_ref.py) agrees with a brute-force sort of every candidate."""
import os
import re

import numpy as np

from qwen3_asr_rs_amd import _lib
from beam_ref import EOS_IDS, NONE, assign_slots, beam_round, brute_round, initial_state, topk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["q3a_beam_search_batch_ptrs", "q3a_beam_begin", "q3a_beam_step", "q3a_beam_fetch", "q3a_selftest_beam_topk",
               "q3a_selftest_beam_advance", "q3a_selftest_kv_reorder"]


def test_new_symbols_in_header_bindings_and_rust(lib):
    with open(os.path.join(ROOT, "include", "q3asr.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "integration", "rust", "src", "backend", "hip", "engine.rs")) as f:
        rust = f.read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", hdr), s
        assert s in _lib.SYMBOLS, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
        assert re.search(r"pub fn " + s + r"\(", rust), s


def test_header_names_every_refusal_and_what_is_out_of_scope():
    with open(os.path.join(ROOT, "include", "q3asr.h")) as f:
        hdr = f.read()
    sec = hdr[hdr.index("beam search: n-best"):hdr.index("int32_t q3a_beam_search_batch_ptrs(")]
    for word in ("width < 1 or > 8", "U * width > 32", "not divisible by width", "differ in length", "stride < max_new", "aligner engine",
                 "without q3a_beam_begin", "Out of scope", "q3a_group", "beam_stats", "151643", "151645", "smaller parent slot"):
        assert word in sec, word


def test_beam_kernels_are_built_from_their_own_source():
    from qwen3_asr_rs_amd import build
    assert "k_beam.hip" in build.SOURCES
    with open(os.path.join(ROOT, "qwen3_asr_rs_amd", "csrc", "kernels.h")) as f:
        kh = f.read()
    for name in ("launch_beam_topk", "launch_beam_advance", "launch_kv_reorder"):
        assert name in kh, name


def _tables(lp_full, W):
    """Top-W tables of float32 log-probability rows under the tie rule (what the device's selection hands to the round)."""
    ids, _ = topk_ref(lp_full, W)
    return ids, np.take_along_axis(np.asarray(lp_full, np.float32), ids.astype(np.int64), axis=1)


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("parent", "token", "score", "finished")) and a["copies"] == b["copies"]


def test_round_agrees_with_a_brute_force_sort_of_all_candidates():
    rng = np.random.default_rng(7)
    seen = {"finished_survives": 0, "finished_displaced": 0, "empty": 0, "ties": 0}
    for trial in range(200):
        W = int(rng.integers(1, 9))
        U = int(rng.integers(1, 4))
        V = int(rng.integers(W, 14))
        S = U * W
        # coarse values: exact score ties across parents and across tokens are common
        lp_full = (-rng.integers(0, 6, size=(S, V)) * 0.5).astype(np.float32)
        score = (-rng.integers(0, 5, size=S) * 0.5).astype(np.float32)
        finished = (rng.random(S) < 0.3).astype(np.uint8)
        empty = (rng.random(S) < 0.15) & (finished == 0)
        for u in range(U):  # at least one slot of every utterance holds something
            empty[u * W] = False
        score[empty] = -np.inf
        if trial == 0:
            score, finished = initial_state(U, W)
            empty = score == -np.inf
        ids, lp = _tables(lp_full, W)
        got = beam_round(ids, lp, score, finished, W)
        want = brute_round(lp_full, score, finished, W)
        assert _same(got, want), trial
        was = {int(q) for q in np.flatnonzero(finished)}
        kept = {int(q) for q in np.flatnonzero(got["token"] == NONE) if got["finished"][q]}
        assert kept <= was
        seen["finished_survives"] += len(kept)
        seen["finished_displaced"] += len(was - kept)
        seen["empty"] += int(empty.sum())
        seen["ties"] += int(len(np.unique(got["score"][np.isfinite(got["score"])])) < np.isfinite(got["score"]).sum())
        for q in kept:  # a finished hypothesis never moves and keeps its score
            assert got["parent"][q] == q and got["score"][q] == score[q]
        for q in range(S):
            if got["token"][q] in EOS_IDS:
                assert got["finished"][q] == 1
    assert all(v > 0 for v in seen.values()), seen


def test_crafted_round_with_ties_a_surviving_and_a_displaced_finished_slot():
    W = 4
    # slot 0 live (score -1), slot 1 finished (score -1.5: survives), slot 2 finished (score -9: displaced), slot 3 empty
    score = np.array([-1.0, -1.5, -9.0, -np.inf], np.float32)
    finished = np.array([0, 1, 1, 0], np.uint8)
    ids = np.array([[7, 3, 151645, 9]] + [[0, 1, 2, 3]] * 3, np.int32)
    lp = np.array([[-0.25, -0.5, -0.5, -3.0]] + [[-1.0] * 4] * 3, np.float32)
    r = beam_round(ids, lp, score, finished, W)
    # candidates: (-1.25, 0, 7), (-1.5, 0, 3), (-1.5, 0, EOS), (-1.5, 1, none), (-4, 0, 9), (-9, 2, none): the tie at -1.5 goes to the
    # smaller parent slot, then the smaller token
    assert r["parent"].tolist() == [0, 1, 0, 0] and r["token"].tolist() == [7, NONE, 3, 151645]
    assert r["score"].tolist() == [-1.25, -1.5, -1.5, -1.5] and r["finished"].tolist() == [0, 1, 0, 1]
    assert r["copies"] == 2 and r["min_gap"] == 0.0


def test_a_sole_surviving_child_stays_in_its_parents_slot():
    assert assign_slots([2, 0, 1], 3) == [2, 0, 1]
    assert assign_slots([1, 1, 1, 3], 4) == [1, 0, 2, 3]  # first child keeps slot 1, its siblings fill the free slots in ascending order
    W = 3
    score = np.array([-5.0, -0.5, -4.0], np.float32)
    finished = np.zeros(3, np.uint8)
    ids = np.tile(np.arange(3, dtype=np.int32), (3, 1))
    lp = np.array([[-0.1, -9, -9], [-0.1, -0.2, -9], [-0.1, -9, -9]], np.float32)
    r = beam_round(ids, lp, score, finished, W)
    # ranks: (-0.6, parent 1), (-0.7, parent 1), (-4.1, parent 2): slot 2's only child stays in slot 2, slot 1's second child takes slot 0
    assert r["parent"].tolist() == [1, 1, 2] and r["token"].tolist() == [1, 0, 0] and r["copies"] == 1
