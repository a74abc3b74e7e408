"""Host-side mirror of the reference's pipeline interface over the C ABI (include/q3asr.h).

Names, argument meaning and error behaviour follow the reference (second-state/qwen3_asr_rs):
    AsrInference.load(model_dir, device)        src/inference.rs:30-86
    AsrInference.transcribe(audio, language)    src/inference.rs:89-213
    WhisperFeatureExtractor.extract(samples)    src/mel.rs:49-96
    AudioEncoder.forward(...)                   src/audio_encoder.rs:79-169
    TextDecoder prefill / greedy step           src/text_decoder.rs:94-113, src/inference.rs:140-200
    parse_asr_output / capitalize_first         src/inference.rs:276-313
This module holds no arithmetic: every number is produced by the HIP kernels behind libq3asr_hip.so.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os
import zlib
from dataclasses import dataclass
from typing import Any, Iterable, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from . import _lib

EOS_TOKEN_IDS = (151643, 151645)  # src/inference.rs:154, src/tokenizer.rs:54-55


AUDIO_PAD_ID = 151676  # <|audio_pad|>: the engine finds audio rows by this id
# transcribe_draft_batch: a further verification round runs while the longest rejected tail of a draft has at least this many ids.
# The break-even is (prefill + head + accept time) / (time of one decode step) at one clip, rounded up: measured 2.614 ms / 585.8 us =
# 4.46 (tools/draft_cost.py, 0.6b preset, one 30 s clip, 100 ids).  At 32 clips it is 16.7: pass min_tail there.
DRAFT_MIN_TAIL = 5


class Q3aError(RuntimeError):
    pass


def _f32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _i32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _i64p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def compose_logit_bias(vocab: int, suppress_tokens: Optional[Iterable[int]] = None, logit_bias: Optional[Mapping[int, float]] = None,
                       allowed_tokens: Optional[Iterable[int]] = None, keep_eos: bool = True):
    """The (ids, bias, default) q3a_set_logit_bias takes, from the three ways callers state a constraint (pure host function).

    suppress_tokens: ids that must never be written (bias -inf; Whisper's suppress_tokens, HF bad_words_ids of length 1).
    logit_bias: id -> finite bias or -inf (OpenAI-style logit_bias, HF sequence_bias of length 1).
    allowed_tokens: an allow-list -- default -inf, the listed ids at 0 (or at their logit_bias entry); with keep_eos both EOS ids
    (151643, 151645) are allowed as well, so that generation can stop.  A logit_bias entry for an id outside the allow-list is dropped.
    Suppression wins: an id in suppress_tokens is -inf whatever logit_bias or allowed_tokens say.
    Returns ids (int32, ascending, unique), bias (float32) and the default (0.0 or -inf); ids whose bias equals the default are left out."""
    def checked(ids, what):
        out = []
        for t in ids:
            if int(t) != t or not 0 <= int(t) < vocab:
                raise ValueError(f"{what}: id {t!r} is outside the vocabulary ({vocab})")
            out.append(int(t))
        return out
    table = {}
    for t, v in (logit_bias or {}).items():
        t = checked([t], "logit_bias")[0]
        v = float(v)
        if np.isnan(v) or v == np.inf:
            raise ValueError(f"logit_bias: the bias of id {t} is NaN or +inf (finite or -inf only)")
        table[t] = v
    default = 0.0
    if allowed_tokens is not None:
        default = -np.inf
        allowed = set(checked(allowed_tokens, "allowed_tokens"))
        if keep_eos:
            allowed |= {t for t in EOS_TOKEN_IDS if t < vocab}
        table = {t: table.get(t, 0.0) for t in allowed}
    for t in checked(suppress_tokens or [], "suppress_tokens"):
        table[t] = -np.inf
    ids = sorted(t for t, v in table.items() if v != default)
    return np.asarray(ids, dtype=np.int32), np.asarray([table[t] for t in ids], dtype=np.float32), float(default)


def check_sampling_args(temperature: float, min_p: float = 0.0, seed: int = 0) -> Tuple[float, float, int]:
    """The refusals of q3a_set_sampling that need no engine (pure host function): temperature finite and >= 0 (0 = off), min_p in
    [0, 1], seed an unsigned 64-bit integer.  Returns the three as the C call takes them."""
    try:
        t, p = float(temperature), float(min_p)
    except (TypeError, ValueError):
        raise Q3aError("set_sampling: temperature and min_p must be numbers")
    if not (math.isfinite(t) and t >= 0.0):
        raise Q3aError(f"set_sampling: temperature must be finite and >= 0 (0 turns sampling off), got {temperature!r}")
    if not (0.0 <= p <= 1.0):
        raise Q3aError(f"set_sampling: min_p must lie in [0, 1], got {min_p!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not (0 <= int(seed) < 1 << 64):
        raise Q3aError(f"set_sampling: seed must be an integer in [0, 2^64), got {seed!r}")
    return t, p, int(seed)


def check_sampling_filter_args(top_k: int = 0, top_p: float = 1.0) -> Tuple[int, float]:
    """The refusals of q3a_set_sampling_filter that need no engine (pure host function): top_k an integer >= 0 (0 = off) that fits an
    int32, top_p in (0, 1] (1 = off).  Returns the two as the C call takes them."""
    k = top_k
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not (0 <= int(k) < 1 << 31):
        raise Q3aError(f"set_sampling_filter: top_k must be an integer >= 0 (0 turns top-k off), got {top_k!r}")
    try:
        p = float(top_p)
    except (TypeError, ValueError):
        raise Q3aError("set_sampling_filter: top_p must be a number")
    if not (0.0 < p <= 1.0) or float(np.float32(p)) <= 0.0:
        raise Q3aError(f"set_sampling_filter: top_p must lie in (0, 1] (1 turns top-p off), got {top_p!r}")
    return int(k), p


def check_repetition_args(repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0) -> Tuple[float, int]:
    """The refusals of q3a_set_repetition that need no engine (pure host function): repetition_penalty finite and > 0 (1 = no
    penalty), no_repeat_ngram_size an integer in [0, 32] (0 = no ban).  Returns the two as the C call takes them."""
    try:
        p = float(repetition_penalty)
    except (TypeError, ValueError):
        raise Q3aError("set_repetition: repetition_penalty must be a number")
    if not (math.isfinite(p) and p > 0.0):
        raise Q3aError(f"set_repetition: repetition_penalty must be finite and > 0 (1 turns the penalty off), got {repetition_penalty!r}")
    n = no_repeat_ngram_size
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not (0 <= int(n) <= 32):
        raise Q3aError(f"set_repetition: no_repeat_ngram_size must be an integer in [0, 32] (0 turns the ban off), got {no_repeat_ngram_size!r}")
    return p, int(n)


TOP_LOGPROBS_MAX = 20


def check_top_logprobs_args(n: int = 0) -> int:
    """The refusals of q3a_set_top_logprobs that need no engine (pure host function): n an integer in [0, 20] (0 = off).  Returns n as
    the C call takes it.  (n above the vocabulary is the engine's refusal: it knows the vocabulary.)"""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not (0 <= int(n) <= TOP_LOGPROBS_MAX):
        raise Q3aError(f"set_top_logprobs: n must be an integer in [0, {TOP_LOGPROBS_MAX}] (0 turns it off), got {n!r}")
    return int(n)


def check_top_logprobs_compat(top_logprobs: int, beam_size: int = 1, draft=None):
    """What transcribe(top_logprobs=...) does not run with, decided on the host before the engine is touched."""
    if top_logprobs and beam_size > 1:
        raise Q3aError("transcribe: beam search reports no top log-probabilities (beam_size > 1 with top_logprobs): its slots re-order rows")
    if top_logprobs and draft is not None:
        raise Q3aError("transcribe: a draft cannot be verified with top log-probabilities (draft with top_logprobs): accepted tokens never pass the step's head")


def uniform_top_logprobs(options) -> int:
    """The one top_logprobs of a batch's option dicts (0 when none has the key).  The setting is uniform for a batch -- the history has
    one inner stride and the step one n --, so dicts that disagree are refused."""
    given = [check_top_logprobs_args((o or {}).get("top_logprobs", 0)) for o in options]
    if len(set(given)) > 1:
        raise ValueError(f"transcribe_batch: top_logprobs must be equal for all rows (the engine records one n per batch, not per row), got {given}")
    return given[0] if given else 0


SEQUENCE_BIAS_MAX_ENTRIES, SEQUENCE_BIAS_MAX_LEN, SEQUENCE_BIAS_MAX_IDS = 4096, 32, 65536


def _sequence_bias_pairs(entries) -> List[Tuple[tuple, float]]:
    """entries as a list of (ids, bias) pairs: from a mapping {tuple of ids: bias} or an iterable of (ids, bias); None: no entry."""
    if entries is None:
        return []
    items = entries.items() if isinstance(entries, Mapping) else entries
    out = []
    for item in items:
        try:
            seq, b = item
            out.append((tuple(seq), b))
        except (TypeError, ValueError):
            raise Q3aError(f"sequence_bias: an entry must be (ids, bias), got {item!r}")
    return out


def check_sequence_bias(entries, vocab: int):
    """The refusals of q3a_set_sequence_bias that need no engine (pure host function): every entry 1 to 32 integer ids inside the
    vocabulary with a bias that is finite or -inf, no sequence twice, at most 4096 entries and 65536 ids.  `entries` is a mapping
    {tuple of ids: bias} or an iterable of (ids, bias) pairs, in the order the biases are to be added.  Returns (ids int32, the
    entries' ids one after the other; lens int32; bias float32) as the C call takes them."""
    pairs = _sequence_bias_pairs(entries)
    if len(pairs) > SEQUENCE_BIAS_MAX_ENTRIES:
        raise Q3aError(f"sequence_bias: {len(pairs)} entries, more than {SEQUENCE_BIAS_MAX_ENTRIES}")
    ids, lens, bias, seen = [], [], [], set()
    for i, (seq, b) in enumerate(pairs):
        if not 1 <= len(seq) <= SEQUENCE_BIAS_MAX_LEN:
            raise Q3aError(f"sequence_bias: entry {i} has {len(seq)} ids (1 to {SEQUENCE_BIAS_MAX_LEN})")
        for t in seq:
            if isinstance(t, bool) or not isinstance(t, (int, np.integer)):
                raise Q3aError(f"sequence_bias: id {t!r} of entry {i} is not an integer")
            if not 0 <= int(t) < vocab:
                raise Q3aError(f"sequence_bias: id {int(t)} of entry {i} is outside the vocabulary ({vocab})")
        seq = tuple(int(t) for t in seq)
        if seq in seen:
            raise Q3aError(f"sequence_bias: entry {i} repeats the sequence of an earlier entry")
        seen.add(seq)
        try:
            b = float(b)
        except (TypeError, ValueError):
            raise Q3aError(f"sequence_bias: the bias of entry {i} must be a number")
        if math.isnan(b) or b == math.inf:
            raise Q3aError(f"sequence_bias: the bias of entry {i} is NaN or +inf (finite or -inf only)")
        ids += seq
        lens.append(len(seq))
        bias.append(b)
    if len(ids) > SEQUENCE_BIAS_MAX_IDS:
        raise Q3aError(f"sequence_bias: {len(ids)} ids over all entries, more than {SEQUENCE_BIAS_MAX_IDS}")
    return np.asarray(ids, dtype=np.int32), np.asarray(lens, dtype=np.int32), np.asarray(bias, dtype=np.float32)


SEQUENCE_BIAS_MAX_LISTS = 256


@dataclasses.dataclass
class RowOptions:
    """The decoding options of ONE sequence of a batch (q3a_row_options; include/q3asr.h "row options"): what set_sampling,
    set_sampling_filter, set_repetition and set_sequence_bias hold once per engine.  The defaults are a plain greedy row."""
    temperature: float = 0.0
    min_p: float = 0.0
    seed: int = 0
    top_k: int = 0
    top_p: float = 1.0
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    sequence_bias: Any = None  # entries as set_sequence_bias takes them, or None


def check_row_options(rows, vocab: int):
    """The refusals of HipEngine.set_row_options that need no engine, each with the row's index, and the rows' lists collected:
    returns (records, lists) -- records[s] = (temperature, min_p, seed, top_k, top_p, repetition_penalty, no_repeat_ngram_size,
    list index or -1), lists = the distinct non-empty entry lists in the order rows first name them (equal lists share an index)."""
    records, lists, index = [], [], {}
    for s, r in enumerate(rows):
        if not isinstance(r, RowOptions):
            raise Q3aError(f"set_row_options: row {s} is not a RowOptions")
        try:
            t, mp, sd = check_sampling_args(r.temperature, r.min_p, r.seed)
            k, tp = check_sampling_filter_args(r.top_k, r.top_p)
            p, n = check_repetition_args(r.repetition_penalty, r.no_repeat_ngram_size)
            pairs = _sequence_bias_pairs(r.sequence_bias)
            check_sequence_bias(pairs, vocab)
        except Q3aError as e:
            raise Q3aError(f"set_row_options: row {s}: {e}") from None
        li = -1
        if pairs:
            key = tuple(pairs)
            if key not in index:
                index[key] = len(lists)
                lists.append(pairs)
            li = index[key]
        records.append((t, mp, sd, k, tp, p, n, li))
    if len(lists) > SEQUENCE_BIAS_MAX_LISTS:
        raise Q3aError(f"set_row_options: {len(lists)} distinct sequence-bias lists, more than {SEQUENCE_BIAS_MAX_LISTS}")
    if sum(len(l) for l in lists) > SEQUENCE_BIAS_MAX_ENTRIES:
        raise Q3aError(f"set_row_options: {sum(len(l) for l in lists)} entries over all lists, more than {SEQUENCE_BIAS_MAX_ENTRIES}")
    if sum(len(q) for l in lists for q, _ in l) > SEQUENCE_BIAS_MAX_IDS:
        raise Q3aError(f"set_row_options: more than {SEQUENCE_BIAS_MAX_IDS} ids over all lists")
    return records, lists


def check_sequence_bias_lists(lists, vocab: int):
    """Several lists, one after the other, as q3a_set_sequence_bias_lists takes them: each checked as check_sequence_bias checks one
    (a sequence may recur in another list), the limits over all of them."""
    parts = [check_sequence_bias(l, vocab) for l in lists]
    if not parts:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def _sequence_list_call(fn, *front) -> List[Tuple[tuple, float]]:
    """One of the C helpers that return a sequence-bias list (sized by a first call with no room)."""
    lib = _lib.load()
    n_ids, n = C.c_int32(), C.c_int32()
    if fn(*front, None, 0, None, None, 0, C.byref(n_ids), C.byref(n)) != 0:
        raise Q3aError((lib.q3a_last_error(None) or b"").decode())
    ids, lens, bias = np.zeros(max(n_ids.value, 1), np.int32), np.zeros(max(n.value, 1), np.int32), np.zeros(max(n.value, 1), np.float32)
    if fn(*front, _i32p(ids), n_ids.value, _i32p(lens), _f32p(bias), n.value, C.byref(n_ids), C.byref(n)) != 0:
        raise Q3aError((lib.q3a_last_error(None) or b"").decode())
    out, o = [], 0
    for k in range(n.value):
        out.append((tuple(int(t) for t in ids[o:o + lens[k]]), float(bias[k])))
        o += int(lens[k])
    return out


def parse_sequence_bias(text: str) -> List[Tuple[tuple, float]]:
    """q3a_parse_sequence_bias: lines "bias id id ..." ('#' comments, "-inf") -> [(ids, bias)].  Host only."""
    return _sequence_list_call(_lib.load().q3a_parse_sequence_bias, text.encode())


def _phrase_array(phrases):
    ps = [phrases] if isinstance(phrases, str) else list(phrases)
    return (C.c_char_p * max(len(ps), 1))(*[p.encode("utf-8") for p in ps]), ps


def _phrase_tokenisations(tokenizer, phrase: str, what: str) -> List[List[int]]:
    p = phrase.strip()
    if not p:
        raise Q3aError(f"{what}: an empty phrase")
    out = []
    for text in (p, " " + p):
        ids = [int(t) for t in tokenizer.encode(text)]
        if not ids:
            raise Q3aError(f"{what}: phrase '{p}' encodes to no id")
        if len(ids) > SEQUENCE_BIAS_MAX_LEN:
            raise Q3aError(f"{what}: phrase '{p}' encodes to {len(ids)} ids, more than {SEQUENCE_BIAS_MAX_LEN}")
        out.append(ids)
    return out


def _merge_sequences(pairs) -> List[Tuple[tuple, float]]:
    table = {}
    for seq, b in pairs:
        table[seq] = max(table[seq], b) if seq in table else b
    return list(table.items())


def hotword_sequences(tokenizer, phrases, boost: float, start_boost: float = 0.0) -> List[Tuple[tuple, float]]:
    """q3a_hotword_sequences: the sequence-bias entries that boost `phrases`.  For each phrase both tokenisations, encode(phrase) and
    encode(" " + phrase); for each tokenisation p_0 .. p_{L-1} the entries (p_0 .. p_j), j = 1 .. L-1, with bias `boost`, and, when
    start_boost != 0, also (p_0) with start_boost.  Equal sequences are merged, keeping the larger bias; a phrase over 32 ids is
    refused by name.  No boost value has been tuned on real weights: `boost` has no default.  An AsrTokenizer goes through the C
    helper; any other object with encode(text) through the same rule in Python."""
    boost, start_boost = float(boost), float(start_boost)
    if not (math.isfinite(boost) and math.isfinite(start_boost)):
        raise Q3aError("hotword_sequences: boost and start_boost must be finite")
    if isinstance(tokenizer, AsrTokenizer):
        arr, ps = _phrase_array(phrases)
        return _sequence_list_call(_lib.load().q3a_hotword_sequences, tokenizer._h, arr, len(ps), C.c_float(boost), C.c_float(start_boost))
    pairs = []
    for phrase in ([phrases] if isinstance(phrases, str) else phrases):
        for p in _phrase_tokenisations(tokenizer, phrase, "hotword_sequences"):
            if start_boost != 0.0:
                pairs.append((tuple(p[:1]), start_boost))
            pairs += [(tuple(p[:j + 1]), boost) for j in range(1, len(p))]
    return _merge_sequences(pairs)


def banned_sequences(tokenizer, phrases) -> List[Tuple[tuple, float]]:
    """q3a_banned_sequences: both tokenisations of each phrase, whole, at -inf (equal sequences once)."""
    if isinstance(tokenizer, AsrTokenizer):
        arr, ps = _phrase_array(phrases)
        return _sequence_list_call(_lib.load().q3a_banned_sequences, tokenizer._h, arr, len(ps))
    pairs = []
    for phrase in ([phrases] if isinstance(phrases, str) else phrases):
        pairs += [(tuple(p), -math.inf) for p in _phrase_tokenisations(tokenizer, phrase, "banned_sequences")]
    return _merge_sequences(pairs)


def check_draft_ids(draft, vocab: int, max_new: int) -> List[int]:
    """The refusals of q3a_prefill_draft / q3a_transcribe_draft_batch_ptrs that need no engine (pure host function): every id an
    integer inside the vocabulary, none of them <|audio_pad|> or an EOS id, at most max_new of them.  Returns the ids as a list."""
    out = []
    for t in draft:
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)):
            raise Q3aError(f"draft: id {t!r} is not an integer")
        t = int(t)
        if not 0 <= t < vocab:
            raise Q3aError(f"draft: id {t} is outside the vocabulary ({vocab})")
        if t == AUDIO_PAD_ID:
            raise Q3aError(f"draft: <|audio_pad|> ({AUDIO_PAD_ID}) cannot be a draft id")
        if t in EOS_TOKEN_IDS:
            raise Q3aError(f"draft: an EOS id ({t}) cannot be a draft id: a draft ends where its ids end")
        out.append(t)
    if len(out) > max_new:
        raise Q3aError(f"draft: {len(out)} ids, more than max_new {max_new}")
    return out


def check_draft_compat(beam_size: int = 1, temperatures: Sequence[float] = (0.0,), repetition: Tuple[float, int] = (1.0, 0)):
    """What a draft does not combine with (pure host function): beam search, sampling, repetition control -- their choices are not the
    argmax of a row alone, so one prefill cannot verify them."""
    if beam_size > 1:
        raise Q3aError("transcribe: a draft verifies the greedy loop, not a beam search (draft with beam_size > 1)")
    if any(float(t) > 0.0 for t in temperatures):
        raise Q3aError("transcribe: a draft cannot be verified under sampling (draft with a temperature > 0)")
    if tuple(repetition) != (1.0, 0):
        raise Q3aError("transcribe: a draft cannot be verified under repetition control (draft with repetition_penalty / no_repeat_ngram_size)")


def draft_next_round(draft: Sequence[int], k: int, tok: int, cap: Optional[int] = None) -> Tuple[List[int], int]:
    """q3a_draft_next_round (host only): the draft of the next verification round, d[:k] + [tok] + d[k+1:], or d[:k] when tok is an EOS
    id.  Returns (the ids, at most cap of them; the number of ids the full answer has)."""
    lib = _lib.load()
    d = np.asarray(list(draft), dtype=np.int32)
    cap = len(d) + 1 if cap is None else int(cap)
    out = np.zeros(max(cap, 1), dtype=np.int32)
    n = C.c_int32()
    if lib.q3a_draft_next_round(_i32p(d) if len(d) else None, len(d), int(k), int(tok), _i32p(out) if cap > 0 else None, cap, C.byref(n)) != 0:
        raise Q3aError((lib.q3a_last_error(None) or b"").decode())
    return out[:min(n.value, cap)].tolist(), int(n.value)


def compression_ratio(text: str) -> float:
    """len(utf8) / len(zlib.compress(utf8)): Whisper's measure of a repetition loop (a looping transcript compresses well)."""
    raw = text.encode("utf-8")
    return len(raw) / len(zlib.compress(raw))


def attempt_acceptable(text: str, avg_logprob: Optional[float], logprob_threshold: float = -1.0,
                       compression_ratio_threshold: float = 2.4) -> bool:
    """The fallback's acceptance rule: avg_logprob >= logprob_threshold (an attempt without tokens has none and passes this half) and
    compression_ratio(text) <= compression_ratio_threshold."""
    if avg_logprob is not None and not (avg_logprob >= logprob_threshold):
        return False
    return compression_ratio(text) <= compression_ratio_threshold


def temperature_fallback(attempt, temperatures: Sequence[float], seed: int = 0, logprob_threshold: float = -1.0,
                         compression_ratio_threshold: float = 2.4):
    """Whisper's temperature fallback as a pure function: attempt(temperature, seed + k) for k = 0, 1, ... must return an object with
    .text and .avg_logprob; the first acceptable attempt (attempt_acceptable) is returned, the last one when none is.  Returns
    (result, temperature used, number of attempts made)."""
    temps = [float(t) for t in temperatures]
    if not temps:
        raise Q3aError("temperature_fallback: no temperature given")
    res = None
    for k, t in enumerate(temps):
        res = attempt(t, int(seed) + k)
        if attempt_acceptable(res.text, res.avg_logprob, logprob_threshold, compression_ratio_threshold):
            return res, t, k + 1
    return res, temps[-1], len(temps)


def parse_logit_bias(text: Optional[str] = None, suppress_list: Optional[str] = None):
    """q3a_parse_logit_bias: "id bias" / "lo-hi bias" lines ('#' comments, "-inf") and a comma list "id,lo-hi,..." of ids to
    suppress -> (ids int32, bias float32).  Host only."""
    lib = _lib.load()
    t = text.encode() if text is not None else None
    sl = suppress_list.encode() if suppress_list is not None else None
    n = C.c_int32()
    if lib.q3a_parse_logit_bias(t, sl, None, None, 0, C.byref(n)) != 0:
        raise Q3aError((lib.q3a_last_error(None) or b"").decode())
    ids, bias = np.zeros(max(n.value, 1), dtype=np.int32), np.zeros(max(n.value, 1), dtype=np.float32)
    if lib.q3a_parse_logit_bias(t, sl, _i32p(ids), _f32p(bias), n.value, C.byref(n)) != 0:
        raise Q3aError((lib.q3a_last_error(None) or b"").decode())
    return ids[:n.value], bias[:n.value]


class HipEngine:
    """Thin RAII wrapper of a q3a_engine handle (one per GPU, one host thread per handle)."""

    def __init__(self, model_dir: str, device: int = 0, precise: bool = False, max_new_tokens: int = 4096,
                 use_graph: bool = True, debug_taps: bool = False, device_arena: Optional[Tuple[int, int]] = None,
                 valu_attention: bool = False, token_logprobs: bool = False):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        opts = _lib.Opts()
        self._lib.q3a_opts_default(C.byref(opts))
        opts.precise = int(precise)
        opts.max_new_tokens = int(max_new_tokens)
        opts.use_graph = int(use_graph)
        opts.debug_taps = int(debug_taps)
        opts.valu_attention = int(valu_attention)
        opts.token_logprobs = int(token_logprobs)
        self.token_logprobs = bool(token_logprobs)
        self.max_new_tokens = int(max_new_tokens) if int(max_new_tokens) > 0 else 4096
        md = os.fsencode(model_dir)
        if device_arena is None:
            rc = self._lib.q3a_engine_create(md, device, C.byref(opts), C.byref(self._h))
        else:
            ptr, nbytes = device_arena
            rc = self._lib.q3a_engine_create_from_arena(md, device, C.c_void_p(ptr), nbytes, C.byref(opts), C.byref(self._h))
        if rc != 0:
            raise Q3aError((self._lib.q3a_last_error(None) or b"").decode())
        d = _lib.DimsC()
        self._lib.q3a_get_dims(self._h, C.byref(d))
        self.dims = d
        self.model_dir = model_dir
        self.batch = 0
        self._n_frames: List[int] = []
        self._T: List[int] = []
        self.logit_bias_state: Tuple[Optional[dict], float] = (None, 0.0)  # what set_logit_bias was last given
        self.sampling_state: Tuple[float, float, int] = (0.0, 0.0, 0)  # what set_sampling was last given
        self.sampling_filter_state: Tuple[int, float] = (0, 1.0)  # what set_sampling_filter was last given
        self.repetition_state: Tuple[float, int] = (1.0, 0)  # what set_repetition was last given
        self.sequence_bias_state: List[Tuple[tuple, float]] = []  # what set_sequence_bias was last given, as (ids, bias) pairs
        self.row_options_state: Optional[List[RowOptions]] = None  # what set_row_options was last given (None: no row table)
        self.top_logprobs_state: int = 0  # what set_top_logprobs was last given

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.q3a_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc != 0:
            raise Q3aError((self._lib.q3a_last_error(self._h) or b"").decode())

    # ---- helpers ------------------------------------------------------------------------------------
    @staticmethod
    def _concat(clips: Sequence[np.ndarray]):
        ns = np.array([len(c) for c in clips], dtype=np.int64)
        pcm = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.float32) for c in clips]))
        return pcm, ns

    def num_audio_tokens(self, n_samples: int) -> int:
        return int(self._lib.q3a_num_audio_tokens(self._h, self._lib.q3a_num_frames(int(n_samples))))

    @staticmethod
    def build_prompt(num_audio_tokens: int, lang_prefix_ids: Optional[Sequence[int]] = None) -> np.ndarray:
        lib = _lib.load()
        n = C.c_int32()
        pre = np.asarray(lang_prefix_ids if lang_prefix_ids is not None else [], dtype=np.int32)
        prep = _i32p(pre) if len(pre) else None
        lib.q3a_build_prompt(num_audio_tokens, prep, len(pre), None, C.byref(n))
        ids = np.zeros(n.value, dtype=np.int32)
        lib.q3a_build_prompt(num_audio_tokens, prep, len(pre), _i32p(ids), C.byref(n))
        return ids

    # ---- stage API ----------------------------------------------------------------------------------
    def mel(self, clips: Sequence[np.ndarray]) -> List[np.ndarray]:
        pcm, ns = self._concat(clips)
        B = len(clips)
        nf = np.zeros(B, dtype=np.int32)
        frames = [int(self._lib.q3a_num_frames(int(n))) for n in ns]
        out = np.zeros(int(sum(frames)) * self.dims.num_mel_bins, dtype=np.float32)
        self._chk(self._lib.q3a_mel(self._h, _f32p(pcm), _i64p(ns), B, _f32p(out), _i32p(nf)))
        self.batch, self._n_frames = B, [int(x) for x in nf]
        res, off = [], 0
        for f in self._n_frames:
            res.append(out[off:off + f * self.dims.num_mel_bins].reshape(self.dims.num_mel_bins, f).copy())
            off += f * self.dims.num_mel_bins
        return res

    def encode(self) -> List[np.ndarray]:
        B = self.batch
        T = np.zeros(B, dtype=np.int32)
        total = sum(int(self._lib.q3a_num_audio_tokens(self._h, f)) for f in self._n_frames)
        out = np.zeros((total, self.dims.enc_output_dim), dtype=np.float32)
        self._chk(self._lib.q3a_encode(self._h, _f32p(out), _i32p(T)))
        self._T = [int(t) for t in T]
        res, off = [], 0
        for t in self._T:
            res.append(out[off:off + t].copy())
            off += t
        return res

    def prefill(self, prompts: Sequence[Sequence[int]], want_logits: bool = True):
        B = len(prompts)
        lens = np.array([len(p) for p in prompts], dtype=np.int32)
        ids = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in prompts]))
        logits = np.zeros((B, self.dims.vocab_size), dtype=np.float32) if want_logits else None
        nxt = np.zeros(B, dtype=np.int32)
        self._chk(self._lib.q3a_prefill(self._h, _i32p(ids), _i32p(lens), B, _f32p(logits) if want_logits else None, _i32p(nxt)))
        return logits, nxt

    def decode_step(self, want_logits: bool = True):
        B = self.batch
        logits = np.zeros((B, self.dims.vocab_size), dtype=np.float32) if want_logits else None
        nxt = np.zeros(B, dtype=np.int32)
        done = np.zeros(B, dtype=np.uint8)
        self._chk(self._lib.q3a_decode_step(self._h, _i32p(nxt), done.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            _f32p(logits) if want_logits else None))
        return logits, nxt, done

    def set_next_tokens(self, ids: Sequence[int]):
        a = np.asarray(ids, dtype=np.int32)
        self._chk(self._lib.q3a_set_next_tokens(self._h, _i32p(a), len(a)))

    # ---- whole path ---------------------------------------------------------------------------------
    def upload_pcm(self, clips: Sequence[np.ndarray]):
        pcm, ns = self._concat(clips)
        self._chk(self._lib.q3a_upload_pcm(self._h, _f32p(pcm), _i64p(ns), len(clips)))
        self.batch = len(clips)

    def run_resident(self, lang_prefix_ids: Optional[Sequence[int]] = None, max_new: int = 0, fixed_new_tokens: int = 0):
        pre = np.asarray(lang_prefix_ids if lang_prefix_ids is not None else [], dtype=np.int32)
        self._chk(self._lib.q3a_run_resident(self._h, _i32p(pre) if len(pre) else None, len(pre), max_new, fixed_new_tokens))

    def fetch_ids(self, stride: int) -> List[List[int]]:
        out = np.zeros((self.batch, stride), dtype=np.int32)
        lens = np.zeros(self.batch, dtype=np.int32)
        self._chk(self._lib.q3a_fetch_ids(self._h, _i32p(out), stride, _i32p(lens)))
        return [out[b, :min(int(lens[b]), stride)].tolist() for b in range(self.batch)]

    def fetch_logprobs(self) -> List[np.ndarray]:
        """q3a_fetch_logprobs: per utterance, the natural-log probability (float32) of every id fetch_ids / transcribe_batch returned
        for the last run or stage-API step, same order and lengths.  Needs token_logprobs=True."""
        lens = np.zeros(self.batch, dtype=np.int32)
        self._chk(self._lib.q3a_fetch_logprobs(self._h, None, 0, _i32p(lens)))  # lengths first
        stride = max(1, int(lens.max()) if len(lens) else 1)
        out = np.zeros((self.batch, stride), dtype=np.float32)
        self._chk(self._lib.q3a_fetch_logprobs(self._h, _f32p(out), stride, _i32p(lens)))
        return [out[b, :int(lens[b])].copy() for b in range(self.batch)]

    def fetch_top_logprobs(self) -> List[Tuple[np.ndarray, np.ndarray]]:
        """q3a_fetch_top_logprobs: per utterance (ids int32 [len][n], lp float32 [len][n]) -- for every id fetch_ids / transcribe_batch
        returned for the last run or stage-API step, the n best entries of the row it was chosen from, best first, with their
        natural-log probabilities.  Needs set_top_logprobs(n > 0) before the run."""
        n = self.top_logprobs_state
        lens = np.zeros(self.batch, dtype=np.int32)
        self._chk(self._lib.q3a_fetch_top_logprobs(self._h, None, None, 0, 0, _i32p(lens)))  # lengths first (and the refusals)
        stride = max(1, int(lens.max()) if len(lens) else 1)
        ids = np.zeros((self.batch, stride, max(n, 1)), dtype=np.int32)
        lp = np.zeros((self.batch, stride, max(n, 1)), dtype=np.float32)
        self._chk(self._lib.q3a_fetch_top_logprobs(self._h, _i32p(ids), _f32p(lp), stride, max(n, 1), _i32p(lens)))
        return [(ids[b, :int(lens[b]), :n].copy(), lp[b, :int(lens[b]), :n].copy()) for b in range(self.batch)]

    @staticmethod
    def _ptrs(clips: Sequence[np.ndarray]):
        """One pointer per utterance (q3a_transcribe_batch_ptrs): float32 C-contiguous arrays are passed as they are -- no
        concatenation, no copy on the Python side.  Returns (kept-alive arrays, void* array, int64 lengths)."""
        arrs = [np.ascontiguousarray(c, dtype=np.float32) for c in clips]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        ns = np.array([a.size for a in arrs], dtype=np.int64)
        return arrs, ptrs, ns

    def transcribe_batch(self, clips: Sequence[np.ndarray], lang_prefix_ids: Optional[Sequence[int]] = None,
                         max_new: int = 4096, fixed_new_tokens: int = 0) -> List[List[int]]:
        """AsrInference::transcribe steps 2-8 for a batch, host PCM -> ids on the host, ONE call through the C ABI."""
        arrs, ptrs, ns = self._ptrs(clips)
        B = len(arrs)
        stride = fixed_new_tokens if fixed_new_tokens > 0 else max_new
        out = np.zeros((B, stride), dtype=np.int32)
        lens = np.zeros(B, dtype=np.int32)
        pre = np.asarray(lang_prefix_ids if lang_prefix_ids is not None else [], dtype=np.int32)
        self._chk(self._lib.q3a_transcribe_batch_ptrs(self._h, ptrs, _i64p(ns), B, _i32p(pre) if len(pre) else None, len(pre), max_new,
                                                      fixed_new_tokens, _i32p(out), stride, _i32p(lens)))
        self.batch = B
        return [out[b, :min(int(lens[b]), stride)].tolist() for b in range(B)]

    # ---- draft-verified decoding ----------------------------------------------------------------------
    @staticmethod
    def _flat_drafts(drafts: Sequence[Sequence[int]]):
        dl = np.array([len(t) for t in drafts], dtype=np.int32)
        flat = np.concatenate([np.asarray(t, dtype=np.int64).reshape(-1) for t in drafts] + [np.zeros(1, np.int64)])
        if flat.min() < -2**31 or flat.max() >= 2**31:
            raise Q3aError("draft: id does not fit 32 bits")
        return dl, np.ascontiguousarray(flat.astype(np.int32))

    def prefill_draft(self, prompts: Sequence[Sequence[int]], drafts: Sequence[Sequence[int]], want_logits: bool = False):
        """Stage form (q3a_prefill_draft) after mel() + encode(): ONE prefill of prompt + draft per utterance, the lm_head at the n + 1
        rows that predict the draft ids and the id behind them, and the engine stands where the greedy loop stands after the accepted
        ids: decode_step / set_next_tokens / fetch_ids / fetch_logprobs continue from there.  Returns (accepted k per utterance, the
        token at k per utterance[, the verified rows' logits [sum of (n + 1)][vocab]])."""
        B = len(prompts)
        if len(drafts) != B:
            raise Q3aError(f"prefill_draft: {len(drafts)} draft(s) for {B} prompt(s)")
        pl = np.array([len(p) for p in prompts], dtype=np.int32)
        pids = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in prompts]))
        dl, flat = self._flat_drafts(drafts)
        acc, nxt = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        logits = np.zeros((int(dl.sum()) + B, self.dims.vocab_size), dtype=np.float32) if want_logits else None
        self._chk(self._lib.q3a_prefill_draft(self._h, _i32p(pids), _i32p(pl), _i32p(flat), _i32p(dl), B, _i32p(acc), _i32p(nxt),
                                              _f32p(logits) if want_logits else None))
        self.batch = B
        return (acc, nxt, logits) if want_logits else (acc, nxt)

    def transcribe_draft_batch(self, clips: Sequence[np.ndarray], drafts: Sequence[Sequence[int]], lang_prefix_ids: Optional[Sequence[int]] = None,
                               max_new: int = 0, max_rounds: int = 1, min_tail: int = DRAFT_MIN_TAIL) -> Tuple[List[List[int]], List[int]]:
        """Whole path (q3a_transcribe_draft_batch_ptrs): the greedy natural-EOS transcript of every clip, exactly what transcribe_batch
        returns, with the longest prefix of each draft that the greedy loop would have written itself verified in one prefill instead
        of decoded step by step.  max_new <= 0: the engine's max_new_tokens.  max_rounds > 1: a rejected id is replaced by the model's
        and the rest of the draft verified again while its tail has at least min_tail ids.  Returns (ids per clip, accepted ids per
        clip in the last round)."""
        arrs, ptrs, ns = self._ptrs(clips)
        B = len(arrs)
        if len(drafts) != B:
            raise Q3aError(f"transcribe_draft_batch: {len(drafts)} draft(s) for {B} clip(s)")
        stride = max(1, min(int(max_new), self.max_new_tokens) if max_new > 0 else self.max_new_tokens)
        dl, flat = self._flat_drafts(drafts)
        out = np.zeros((B, stride), dtype=np.int32)
        lens, acc = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        pre = np.asarray(lang_prefix_ids if lang_prefix_ids is not None else [], dtype=np.int32)
        self._chk(self._lib.q3a_transcribe_draft_batch_ptrs(self._h, ptrs, _i64p(ns), B, _i32p(pre) if len(pre) else None, len(pre), _i32p(flat),
                                                            _i32p(dl), int(max_new), int(max_rounds), int(min_tail), _i32p(out), stride, _i32p(lens),
                                                            _i32p(acc)))
        self.batch = B
        return [out[b, :min(int(lens[b]), stride)].tolist() for b in range(B)], [int(k) for k in acc]

    def draft_stats(self) -> dict:
        """The last draft call (q3a_debug_read "draft_stats"): rounds run and the rows prefilled in each."""
        st = self.debug_read_raw("draft_stats").view(np.int32)
        return {"rounds": int(st[0]), "rows": [int(v) for v in st[1:]]}

    def io_timings(self) -> dict:
        """Input side of the last transcribe_batch (q3a_io_timings_last)."""
        t = _lib.IoTimings()
        self._chk(self._lib.q3a_io_timings_last(self._h, C.byref(t)))
        return {n: getattr(t, n) for n, _ in _lib.IoTimings._fields_}

    # ---- measurement / debug --------------------------------------------------------------------------
    def timings(self) -> dict:
        t = _lib.Timings()
        self._chk(self._lib.q3a_stage_timings(self._h, C.byref(t)))
        return {n: getattr(t, n) for n, _ in _lib.Timings._fields_}

    def profile_decode_step(self) -> dict:
        p = _lib.KernelProfile()
        self._chk(self._lib.q3a_profile_decode_step(self._h, C.byref(p)))
        return {name: {"total_us": float(p.total_us[i]), "launches": int(p.launches[i]), "weight_bytes": float(p.weight_bytes[i])}
                for i, name in enumerate(_lib.KC_NAMES)}

    def profile_weight_stream(self, reps: int = 4) -> dict:
        """Back-to-back qkv + gate/up GEMVs over all layers between one HIP event pair (see q3asr.h)."""
        avg, nbytes, n = C.c_float(), C.c_double(), C.c_int32()
        self._chk(self._lib.q3a_profile_weight_stream(self._h, reps, C.byref(avg), C.byref(nbytes), C.byref(n)))
        return {"avg_us": float(avg.value), "bytes_per_launch": float(nbytes.value), "launches": int(n.value)}

    def debug_read(self, name: str) -> np.ndarray:
        n = C.c_uint64()
        self._chk(self._lib.q3a_debug_read(self._h, name.encode(), None, 0, C.byref(n)))
        out = np.zeros(n.value // 4, dtype=np.float32)
        self._chk(self._lib.q3a_debug_read(self._h, name.encode(), out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return out

    # ---- forced aligner -----------------------------------------------------------------------------
    def aligner_info(self) -> dict:
        """classify_num (0: not an aligner), timestamp_token_id and ms per class (q3a_aligner_info)."""
        n, tid, seg = C.c_int32(), C.c_int32(), C.c_float()
        self._chk(self._lib.q3a_aligner_info(self._h, C.byref(n), C.byref(tid), C.byref(seg)))
        return {"classify_num": int(n.value), "timestamp_token_id": int(tid.value), "segment_ms": float(seg.value)}

    def align(self, prompts: Sequence[Sequence[int]], stride: Optional[int] = None, want_logits: bool = False):
        """Stage form after mel() + encode(): one prefill of the aligner prompts and the classifier head at every marker row.
        Returns (classes per utterance, logits [markers][classify_num] or None)."""
        B = len(prompts)
        lens = np.array([len(p) for p in prompts], dtype=np.int32)
        ids = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in prompts]))
        tid = self.aligner_info()["timestamp_token_id"]
        if stride is None:
            stride = max(1, max(int(np.sum(np.asarray(p) == tid)) for p in prompts))
        out = np.zeros((B, max(stride, 1)), dtype=np.int32)
        counts = np.zeros(B, dtype=np.int32)
        logits = None
        if want_logits:
            total = int(sum(int(np.sum(np.asarray(p) == tid)) for p in prompts))
            logits = np.zeros((max(total, 1), self.aligner_info()["classify_num"]), dtype=np.float32)
        self._chk(self._lib.q3a_align(self._h, _i32p(ids), _i32p(lens), B, _i32p(out), stride, _i32p(counts),
                                      _f32p(logits) if want_logits else None))
        cls = [out[b, :int(counts[b])].tolist() for b in range(B)]
        if want_logits:
            logits = logits[:int(counts.sum())]
        return cls, logits

    def align_batch(self, clips: Sequence[np.ndarray], text_ids: Sequence[Sequence[int]], stride: Optional[int] = None) -> List[List[int]]:
        """Whole path (q3a_align_batch_ptrs): host PCM + the word and marker ids of each utterance -> marker classes."""
        arrs, ptrs, ns = self._ptrs(clips)
        B = len(arrs)
        tl = np.array([len(t) for t in text_ids], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32) for t in text_ids] + [np.zeros(1, np.int32)]))
        if stride is None:
            tid = self.aligner_info()["timestamp_token_id"]
            stride = max(1, max(int(np.sum(np.asarray(t) == tid)) for t in text_ids))
        out = np.zeros((B, max(stride, 1)), dtype=np.int32)
        counts = np.zeros(B, dtype=np.int32)
        self._chk(self._lib.q3a_align_batch_ptrs(self._h, ptrs, _i64p(ns), B, _i32p(flat), _i32p(tl), _i32p(out), stride, _i32p(counts)))
        self.batch = B
        return [out[b, :int(counts[b])].tolist() for b in range(B)]

    # ---- scoring a given transcript ------------------------------------------------------------------
    @staticmethod
    def _score_targets(targets: Sequence[Sequence[int]], stride: Optional[int] = None):
        tl = np.array([len(t) for t in targets], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int64).reshape(-1) for t in targets] + [np.zeros(1, np.int64)]))
        if len(flat) and (flat.min() < -2**31 or flat.max() >= 2**31):
            raise Q3aError("score: target id does not fit 32 bits")
        if stride is None:
            stride = max(1, int(tl.max()) if len(tl) else 1)
        return tl, flat.astype(np.int32), int(stride)

    @staticmethod
    def _score_split(tl, lp, ti, tp):
        return [(lp[b, :int(n)].copy(), ti[b, :int(n)].copy(), tp[b, :int(n)].copy()) for b, n in enumerate(tl)]

    def score(self, prompts: Sequence[Sequence[int]], targets: Sequence[Sequence[int]], want_logits: bool = False,
              stride: Optional[int] = None):
        """Stage form (q3a_score) after mel() + encode(): ONE prefill of prompt + targets[:-1] per utterance and the lm_head at the rows
        that predict the targets.  Returns per utterance (lp, top_ids, top_lp): the log-probability of every target, the model's own
        argmax at that position and its log-probability; with want_logits also the fp32 logits [sum of lengths][vocab]."""
        B = len(prompts)
        if len(targets) != B:
            raise Q3aError(f"score: {len(targets)} target list(s) for {B} prompt(s)")
        pl = np.array([len(p) for p in prompts], dtype=np.int32)
        pids = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in prompts]))
        tl, flat, stride = self._score_targets(targets, stride)
        lp = np.zeros((B, max(stride, 1)), dtype=np.float32)
        ti = np.zeros((B, max(stride, 1)), dtype=np.int32)
        tp = np.zeros((B, max(stride, 1)), dtype=np.float32)
        logits = np.zeros((max(int(tl.sum()), 1), self.dims.vocab_size), dtype=np.float32) if want_logits else None
        self._chk(self._lib.q3a_score(self._h, _i32p(pids), _i32p(pl), _i32p(flat), _i32p(tl), B, _f32p(lp), _i32p(ti), _f32p(tp), stride,
                                      _f32p(logits) if want_logits else None))
        res = self._score_split(tl, lp, ti, tp)
        return (res, logits[:int(tl.sum())]) if want_logits else res

    def score_batch(self, clips: Sequence[np.ndarray], targets: Sequence[Sequence[int]], lang_prefix_ids: Optional[Sequence[int]] = None,
                    stride: Optional[int] = None):
        """Whole path (q3a_score_batch_ptrs): host PCM + the ids to score per utterance -> (lp, top_ids, top_lp) per utterance."""
        arrs, ptrs, ns = self._ptrs(clips)
        B = len(arrs)
        if len(targets) != B:
            raise Q3aError(f"score_batch: {len(targets)} target list(s) for {B} clip(s)")
        tl, flat, stride = self._score_targets(targets, stride)
        pre = np.asarray(lang_prefix_ids if lang_prefix_ids is not None else [], dtype=np.int32)
        lp = np.zeros((B, max(stride, 1)), dtype=np.float32)
        ti = np.zeros((B, max(stride, 1)), dtype=np.int32)
        tp = np.zeros((B, max(stride, 1)), dtype=np.float32)
        self._chk(self._lib.q3a_score_batch_ptrs(self._h, ptrs, _i64p(ns), B, _i32p(pre) if len(pre) else None, len(pre), _i32p(flat), _i32p(tl),
                                                 _f32p(lp), _i32p(ti), _f32p(tp), stride))
        self.batch = B
        return self._score_split(tl, lp, ti, tp)

    # ---- constrained decoding ----------------------------------------------------------------------------
    def set_logit_bias(self, bias: Optional[Mapping[int, float]] = None, default: float = 0.0):
        """q3a_set_logit_bias: b = `default` (0.0 or -inf) everywhere, then b[id] = bias[id]; every head of the generation paths works
        on logits + b until it is cleared (None / {} with default 0.0).  Drops the decode state: prefill again before a stage-API
        step.  compose_logit_bias() builds the arguments from suppress / bias / allow lists."""
        items = sorted((int(t), float(v)) for t, v in (bias or {}).items())
        ids = np.asarray([t for t, _ in items], dtype=np.int32)
        vals = np.asarray([v for _, v in items], dtype=np.float32)
        self._chk(self._lib.q3a_set_logit_bias(self._h, _i32p(ids) if len(ids) else None, _f32p(vals) if len(ids) else None, len(ids),
                                               C.c_float(default)))
        self.logit_bias_state = (dict(items) if items else None, float(default))

    def logit_bias_vector(self) -> np.ndarray:
        """The dense fp32 [vocab] bias as the device holds it (zeros when off)."""
        return self.debug_read("logit_bias")

    def logit_bias_stats(self) -> dict:
        st = self.debug_read_raw("logit_bias_stats").view(np.int32)
        return {"active": bool(st[0]), "finite": int(st[1])}

    # ---- sampling ---------------------------------------------------------------------------------------
    def set_sampling(self, temperature: float, min_p: float = 0.0, seed: int = 0):
        """q3a_set_sampling: with temperature > 0 every generation step draws its id from softmax(logits / temperature) restricted to
        the min-p kept set, on the device, reproducibly from `seed`; 0 turns it off.  Drops the decode state: prefill again before a
        stage-API step.  The noise depends on a sequence's index in the call, so a clip alone and inside a batch draw differently."""
        t, p, sd = check_sampling_args(temperature, min_p, seed)
        self._chk(self._lib.q3a_set_sampling(self._h, C.c_float(t), C.c_float(p), C.c_uint64(sd)))
        self.sampling_state = (t, p, sd)

    def sampling_stats(self) -> dict:
        st = self.debug_read_raw("sampling").view(np.uint32)
        return {"active": bool(st[0]), "temperature": float(st[1:2].view(np.float32)[0]), "min_p": float(st[2:3].view(np.float32)[0]),
                "seed": int(st[3]) | (int(st[4]) << 32)}

    def set_sampling_filter(self, top_k: int = 0, top_p: float = 1.0):
        """q3a_set_sampling_filter: while sampling is on, every step keeps only the entries >= the top_k-th largest logit (ties kept) and,
        of those, the smallest head whose probability at the temperature reaches top_p (equal values share their fate) -- HuggingFace's
        TopKLogitsWarper and TopPLogitsWarper as a value threshold, found on the device.  (0, 1.0) turns it off.  Drops the decode
        state: prefill again before a stage-API step."""
        k, p = check_sampling_filter_args(top_k, top_p)
        self._chk(self._lib.q3a_set_sampling_filter(self._h, k, C.c_float(p)))
        self.sampling_filter_state = (k, p)

    def sampling_filter_stats(self) -> dict:
        st = self.debug_read_raw("sampling_filter").view(np.uint32)
        return {"active": bool(st[0]), "top_k": int(st[1]), "top_p": float(st[2:3].view(np.float32)[0])}

    # ---- repetition penalty / no-repeat n-grams ------------------------------------------------------------
    def set_repetition(self, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0):
        """q3a_set_repetition: every generation step divides the positive (multiplies the other) logits of the ids the sequence has
        generated so far by repetition_penalty, once per distinct id, then bans (-inf) every id that would complete an n-gram of
        no_repeat_ngram_size ids already generated -- on the device, on the sequence's own out_ids, bit for bit HuggingFace's two
        processors.  (1.0, 0) turns it off.  Drops the decode state: prefill again before a stage-API step."""
        p, n = check_repetition_args(repetition_penalty, no_repeat_ngram_size)
        self._chk(self._lib.q3a_set_repetition(self._h, C.c_float(p), n))
        self.repetition_state = (p, n)

    def repetition_stats(self) -> dict:
        st = self.debug_read_raw("repetition").view(np.uint32)
        return {"active": bool(st[0]), "repetition_penalty": float(st[1:2].view(np.float32)[0]), "no_repeat_ngram_size": int(st[2])}

    # ---- top log-probabilities -------------------------------------------------------------------------------
    def set_top_logprobs(self, n: int = 0):
        """q3a_set_top_logprobs: while n > 0 (at most 20) every generation step also records the n best entries of its final row --
        larger logit first, then smaller id -- with their log-probabilities under the untempered, unfiltered distribution; read them
        with fetch_top_logprobs.  0 turns it off.  Drops the decode state: prefill again before a stage-API step."""
        n = check_top_logprobs_args(n)
        self._chk(self._lib.q3a_set_top_logprobs(self._h, n))
        self.top_logprobs_state = n

    def top_logprobs_stats(self) -> dict:
        n = int(self.debug_read_raw("top_logprobs").view(np.int32)[0])
        return {"active": n > 0, "n": n}

    # ---- sequence bias: hotword boosts and banned phrases ------------------------------------------------------
    def set_sequence_bias(self, entries=None):
        """q3a_set_sequence_bias: `entries` is a mapping {tuple of ids: bias} or an iterable of (ids, bias) pairs; at every generation
        step the bias of an entry is added to the logit of its last id whenever the ids the sequence has generated so far end in the
        rest of the entry -- on the device, on the sequence's own out_ids, bit for bit HuggingFace's SequenceBiasLogitsProcessor
        (NoBadWordsLogitsProcessor with a bias of -inf).  None / an empty list turns it off.  hotword_sequences() and
        banned_sequences() build entries from phrases.  Drops the decode state: prefill again before a stage-API step."""
        ids, lens, bias = check_sequence_bias(entries, self.dims.vocab_size)
        n = len(lens)
        self._chk(self._lib.q3a_set_sequence_bias(self._h, _i32p(ids) if n else None, _i32p(lens) if n else None, _f32p(bias) if n else None, n))
        self.sequence_bias_state = _sequence_bias_pairs(entries)

    # ---- row options: per-request settings inside one batch ------------------------------------------------------
    def _set_sequence_bias_lists(self, lists):
        flat = [e for l in lists for e in l]
        ids, lens, bias = check_sequence_bias_lists(lists, self.dims.vocab_size)
        ll = np.asarray([len(l) for l in lists], dtype=np.int32)
        n = len(flat)
        self._chk(self._lib.q3a_set_sequence_bias_lists(self._h, _i32p(ids) if n else None, _i32p(lens) if n else None, _f32p(bias) if n else None,
                                                        _i32p(ll) if len(lists) else None, len(lists)))

    def set_row_options(self, rows=None):
        """q3a_set_row_options: `rows` holds one RowOptions per sequence of the next batches -- sequence s samples, filters, penalises
        and biases by ITS record (a row with the defaults is a plain greedy row), on the device, in the same launches.  The rows'
        distinct sequence_bias lists go to the engine as its lists (q3a_set_sequence_bias_lists; equal lists share an index).  None
        or an empty list clears the table and puts back the list set_sequence_bias last gave: the uniform settings, remembered all
        along, are in force again.  The next prefill must have len(rows) sequences.  Drops the decode state.  A refused table
        leaves the engine without one."""
        rows = list(rows) if rows is not None else []
        if not rows:
            self._clear_row_options()
            return
        records, lists = check_row_options(rows, self.dims.vocab_size)

        def table(with_lists):
            t = (_lib.RowOptionsC * len(records))()
            for c, (tm, mp, sd, k, tp, p, n, li) in zip(t, records):
                (c.temperature, c.min_p, c.seed, c.top_k, c.top_p, c.repetition_penalty, c.no_repeat_ngram_size,
                 c.sequence_list) = (tm, mp, sd, k, tp, p, n, li if with_lists else -1)
            return t
        # neither setter may meet an index the other has not seen: the records without their lists, the lists, then the records
        try:
            self._chk(self._lib.q3a_set_row_options(self._h, table(False), len(records)))
            self.row_options_state = [dataclasses.replace(r, sequence_bias=None) for r in rows]
            self._set_sequence_bias_lists(lists)
            self._chk(self._lib.q3a_set_row_options(self._h, table(True), len(records)))
        except Q3aError:
            self._clear_row_options()
            raise
        self.row_options_state = [dataclasses.replace(r) for r in rows]

    def _clear_row_options(self):
        if self.row_options_state is not None:
            # the lists are the table's: rows that name none (so that no row names a list that goes), the engine's own list, no table
            n = len(self.row_options_state)
            off = (_lib.RowOptionsC * n)(*[_lib.RowOptionsC(0.0, 0.0, 0, 0, 1.0, 1.0, 0, -1)] * n)
            self._chk(self._lib.q3a_set_row_options(self._h, off, n))
            self.set_sequence_bias(self.sequence_bias_state)
        self._chk(self._lib.q3a_set_row_options(self._h, None, 0))
        self.row_options_state = None

    def row_options_stats(self) -> dict:
        raw = self.debug_read_raw("row_options")
        n = raw.size // C.sizeof(_lib.RowOptionsC)
        table = (_lib.RowOptionsC * n).from_buffer_copy(raw.tobytes()) if n else []
        return {"active": n > 0, "rows": [{f: getattr(c, f) for f, _ in _lib.RowOptionsC._fields_} for c in table]}

    def sequence_bias_stats(self) -> dict:
        st = self.debug_read_raw("sequence_bias").view(np.int32)
        return {"active": bool(st[0]), "entries": int(st[1]), "ids": int(st[2]), "targets": int(st[3])}

    # ---- beam search ----------------------------------------------------------------------------------
    def _beam_unpack(self, U, W, stride, ids, lens, scores, fin, lp) -> "List[List[BeamHypothesis]]":
        res = []
        for u in range(U):
            hyps = []
            for k in range(W):
                n, f = int(lens[u, k]), bool(fin[u, k])
                hyps.append(BeamHypothesis(ids[u, k, :n].tolist(), float(scores[u, k]), f, lp[u, k, :n + (1 if f else 0)].copy()))
            res.append(hyps)
        return res

    def beam_search_batch(self, clips: Sequence[np.ndarray], width: int, lang_prefix_ids: Optional[Sequence[int]] = None,
                          max_new: int = 0) -> "List[List[BeamHypothesis]]":
        """Whole path (q3a_beam_search_batch_ptrs): per clip its `width` hypotheses, best first (larger score, then smaller slot).
        max_new <= 0: the engine's max_new_tokens."""
        arrs, ptrs, ns = self._ptrs(clips)
        U, W = len(arrs), int(width)
        stride = max(1, min(int(max_new), self.max_new_tokens) if max_new > 0 else self.max_new_tokens)
        shape = (max(U, 1), max(W, 1))
        ids = np.zeros(shape + (stride,), dtype=np.int32)
        lens = np.zeros(shape, dtype=np.int32)
        scores = np.zeros(shape, dtype=np.float32)
        fin = np.zeros(shape, dtype=np.uint8)
        lp = np.zeros(shape + (stride + 1,), dtype=np.float32)
        pre = np.asarray(lang_prefix_ids if lang_prefix_ids is not None else [], dtype=np.int32)
        self._chk(self._lib.q3a_beam_search_batch_ptrs(self._h, ptrs, _i64p(ns), U, _i32p(pre) if len(pre) else None, len(pre), W, int(max_new),
                                                       _i32p(ids), stride, _i32p(lens), _f32p(scores), fin.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                       _f32p(lp)))
        self.batch = U * W
        return self._beam_unpack(U, W, stride, ids, lens, scores, fin, lp)

    def beam_begin(self, width: int):
        """Stage form (q3a_beam_begin), directly after prefill() of U * width sequences in which each utterance appears `width` times
        in a row: round 0 on the prefill's logits."""
        self._chk(self._lib.q3a_beam_begin(self._h, int(width)))
        self._beam_width = int(width)

    def beam_step(self, want_logits: bool = False):
        """One decode step and its round (q3a_beam_step).  Returns (all_finished, logits [S][vocab] the round selected from or None)."""
        done = C.c_uint8()
        logits = np.zeros((self.batch, self.dims.vocab_size), dtype=np.float32) if want_logits else None
        self._chk(self._lib.q3a_beam_step(self._h, C.byref(done), _f32p(logits) if want_logits else None))
        return bool(done.value), logits

    def beam_fetch(self, stride: Optional[int] = None) -> "List[List[BeamHypothesis]]":
        """The hypotheses after the rounds run so far (q3a_beam_fetch), per utterance best first."""
        W = int(getattr(self, "_beam_width", 0))
        if W <= 0:
            self._chk(self._lib.q3a_beam_fetch(self._h, None, 0, None, None, None, None))  # (the engine's own refusal)
        U = self.batch // W
        stride = int(stride) if stride is not None else self.max_new_tokens
        ids = np.zeros((U, W, stride), dtype=np.int32)
        lens = np.zeros((U, W), dtype=np.int32)
        scores = np.zeros((U, W), dtype=np.float32)
        fin = np.zeros((U, W), dtype=np.uint8)
        lp = np.zeros((U, W, stride + 1), dtype=np.float32)
        self._chk(self._lib.q3a_beam_fetch(self._h, _i32p(ids), stride, _i32p(lens), _f32p(scores), fin.ctypes.data_as(C.POINTER(C.c_uint8)), _f32p(lp)))
        return self._beam_unpack(U, W, stride, ids, lens, scores, fin, lp)

    def beam_debug(self) -> dict:
        """The last round of the last beam search (q3a_debug_read "beam_*"): topk_ids / topk_lp [S][W], parent / token / score /
        finished [S], stats int32 [4] (rounds run, survivors that needed a copy, KV rows copied, hypotheses finished)."""
        raw = {n: self.debug_read_raw("beam_" + n) for n in ("topk_ids", "topk_lp", "parent", "token", "score", "finished", "stats")}
        S = len(raw["finished"])
        return {"topk_ids": raw["topk_ids"].view(np.int32).reshape(S, -1), "topk_lp": raw["topk_lp"].view(np.float32).reshape(S, -1),
                "parent": raw["parent"].view(np.int32), "token": raw["token"].view(np.int32), "score": raw["score"].view(np.float32),
                "finished": raw["finished"].copy(), "stats": raw["stats"].view(np.int32)}

    def debug_read_raw(self, name: str) -> np.ndarray:
        """The same as bytes (records of mixed types: tools/soak_engines.py)."""
        n = C.c_uint64()
        self._chk(self._lib.q3a_debug_read(self._h, name.encode(), None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        if n.value:
            self._chk(self._lib.q3a_debug_read(self._h, name.encode(), out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return out


class HipGroup:
    """q3a_group: one process, one host thread per GPU; weights loaded once and replicated with one RCCL broadcast;
    utterances partitioned contiguously (include/q3asr.h, csrc/group.cpp)."""

    def __init__(self, model_dir: str, n_gpus: int = 1, devices: Optional[Sequence[int]] = None, precise: bool = False,
                 max_new_tokens: int = 4096):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        opts = _lib.Opts()
        self._lib.q3a_opts_default(C.byref(opts))
        opts.precise = int(precise)
        opts.max_new_tokens = int(max_new_tokens)
        dv = np.asarray(devices, dtype=np.int32) if devices is not None else None
        rc = self._lib.q3a_group_create(os.fsencode(model_dir), n_gpus, _i32p(dv) if dv is not None else None, C.byref(opts), C.byref(self._h))
        if rc != 0:
            raise Q3aError((self._lib.q3a_last_error(None) or b"").decode())

    @property
    def size(self) -> int:
        return int(self._lib.q3a_group_size(self._h))

    @property
    def used_rccl(self) -> bool:
        return bool(self._lib.q3a_group_used_rccl(self._h))

    def engine_timings(self, rank: int) -> dict:
        """Stage timings of rank's engine for its slice of the last batch (q3a_group_engine + q3a_stage_timings)."""
        h = self._lib.q3a_group_engine(self._h, rank)
        t = _lib.Timings()
        if not h or self._lib.q3a_stage_timings(C.c_void_p(h), C.byref(t)) != 0:
            return {}
        return {n: getattr(t, n) for n, _ in _lib.Timings._fields_}

    @property
    def startup_seconds(self) -> dict:
        """Stage times of q3a_group_create: checkpoint read + pack, H2D upload to the first GPU, RCCL broadcast, engine creation."""
        v = (C.c_double * 4)()
        self._lib.q3a_group_startup_seconds(self._h, v)
        return {"pack_s": v[0], "upload_s": v[1], "broadcast_s": v[2], "engines_s": v[3]}

    def transcribe_batch(self, clips: Sequence[np.ndarray], lang_prefix_ids: Optional[Sequence[int]] = None,
                         max_new: int = 4096, fixed_new_tokens: int = 0) -> List[List[int]]:
        arrs, ptrs, ns = HipEngine._ptrs(clips)
        B = len(arrs)
        stride = fixed_new_tokens if fixed_new_tokens > 0 else max_new
        out = np.zeros((B, stride), dtype=np.int32)
        lens = np.zeros(B, dtype=np.int32)
        pre = np.asarray(lang_prefix_ids if lang_prefix_ids is not None else [], dtype=np.int32)
        rc = self._lib.q3a_group_transcribe_ptrs(self._h, ptrs, _i64p(ns), B, _i32p(pre) if len(pre) else None, len(pre), max_new,
                                                 fixed_new_tokens, _i32p(out), stride, _i32p(lens))
        if rc != 0:
            raise Q3aError((self._lib.q3a_group_last_error(self._h) or b"").decode())
        return [out[b, :min(int(lens[b]), stride)].tolist() for b in range(B)]

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.q3a_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def measure_peaks(device: int = 0, reps: int = 5) -> dict:
    """q3a_measure_peaks (include/q3asr.h): HBM read / copy / triad GB/s and the 8192^3 bf16 GEMM TFLOP/s measured on this device."""
    lib = _lib.load()
    pk = _lib.Peaks()
    if lib.q3a_measure_peaks(device, reps, C.byref(pk)) != 0:
        raise RuntimeError("q3a_measure_peaks failed (no HIP device, or less than 2 GiB of free device memory)")
    return {"hbm_read_GBps": round(pk.hbm_read_gbps, 1), "hbm_copy_GBps": round(pk.hbm_copy_gbps, 1), "hbm_triad_GBps": round(pk.hbm_triad_gbps, 1),
            "mfma_bf16_TFLOPs": round(pk.mfma_bf16_tflops, 1), "mfma_bf16_TFLOPs_random_data": round(pk.mfma_bf16_tflops_random, 1), "gemm": [pk.gemm_m, pk.gemm_n, pk.gemm_k], "read_sweep_bytes": int(pk.hbm_read_bytes),
            "n_cu": pk.n_cu, "best_of": pk.reps}


def selftest_gemm16(M: int, N: int, K: int, reps: int = 0, device: int = 0) -> dict:
    """bf16-activation GEMM (global_load_lds path) vs the naive device reference; optional timing of both GEMMs."""
    lib = _lib.load()
    err, ref, t16, t32 = C.c_float(), C.c_float(), C.c_float(), C.c_float()
    rc = lib.q3a_selftest_gemm16(device, M, N, K, reps, C.byref(err), C.byref(ref), C.byref(t16), C.byref(t32))
    if rc != 0:
        raise Q3aError((lib.q3a_last_error(None) or b"").decode())
    flops = 2.0 * M * N * K
    out = {"err": err.value, "ref_max": ref.value}
    if reps > 0:
        out.update(us_bf16=t16.value, us_f32=t32.value, tflops_bf16=flops / t16.value / 1e6, tflops_f32=flops / t32.value / 1e6)
    return out


def selftest_gemm(M: int, N: int, K: int, split: bool = False, device: int = 0) -> Tuple[float, float]:
    lib = _lib.load()
    err, ref = C.c_float(), C.c_float()
    rc = lib.q3a_selftest_gemm(device, M, N, K, int(split), C.byref(err), C.byref(ref))
    if rc != 0:
        raise Q3aError((lib.q3a_last_error(None) or b"").decode())
    return err.value, ref.value


# ------------------------------------------------------------------------------------------------------
# Reference-shaped front door
# ------------------------------------------------------------------------------------------------------
from .audio import AsrTokenizer, capitalize_first, fix_timestamps, load_audio, parse_asr_output, split_words_for_alignment  # noqa: E402  (C++ host code behind the C ABI)


@dataclass
class BeamHypothesis:
    """One hypothesis of a beam search: ids (EOS excluded), score = the sum of its tokens' natural-log probabilities (the EOS's included
    when it finished), finished, and the log-probability of every id followed by the EOS's when finished (float32)."""
    ids: List[int]
    score: float
    finished: bool
    token_logprobs: np.ndarray


@dataclass
class Alternative:
    """An entry of TranscribeResult.alternatives: decoded text, the search's score (before any length penalty) and the ids."""
    text: str
    score: float
    ids: List[int]


@dataclass
class TokenCandidate:
    """An entry of TranscribeResult.top_logprobs: a token the step could have written, its text (empty without a tokenizer) and its
    natural-log probability under the step's final, untempered distribution."""
    id: int
    token: str
    logprob: float


@dataclass
class TranscribeResult:
    """src/inference.rs:269-274 (+ the raw ids, which is where parity is pinned).  With an engine created with token_logprobs=True
    also the log-probability of every id and their mean (Whisper's avg_logprob; None when no token was generated)."""
    text: str
    language: str
    raw_output: str
    ids: List[int]
    token_logprobs: Optional[List[float]] = None
    avg_logprob: Optional[float] = None
    alternatives: Optional[List[Alternative]] = None  # beam_size > 1: the n-best list, best first (this result is its first entry)
    temperature: Optional[float] = None  # transcribe(temperature=...): the temperature of the attempt that was kept (0.0 = greedy)
    accepted_draft_tokens: Optional[int] = None  # transcribe(draft=...): leading ids of the draft the greedy loop would have written itself
    top_logprobs: Optional[List[List[TokenCandidate]]] = None  # transcribe(top_logprobs=n): per id of `ids` the n best candidates of its step, best first


@dataclass
class ScoreResult:
    """AsrInference.score: the ids that were scored, the log-probability of each (natural log) and their mean (None when nothing was
    scored), and what the model would have written at each position given the same history, with its log-probability."""
    target_ids: List[int]
    token_logprobs: List[float]
    avg_logprob: Optional[float]
    greedy_ids: List[int]
    greedy_logprobs: List[float]


class AsrInference:
    """Drop-in for the reference's AsrInference (src/inference.rs:19-27) backed by the HIP engine."""

    def __init__(self, engine: HipEngine, tokenizer=None):
        self.engine = engine
        self.tokenizer = tokenizer

    @classmethod
    def load(cls, model_dir: str, device: int = 0, **engine_kwargs) -> "AsrInference":
        """src/inference.rs:30-86.  The tokenizer (tokenizer.json, src/tokenizer.rs:11-30) is optional here:
        synthetic checkpoints have none and parity is defined on token ids."""
        eng = HipEngine(model_dir, device, **engine_kwargs)
        tok = None
        tj = os.path.join(model_dir, "tokenizer.json")
        if os.path.exists(tj):
            tok = AsrTokenizer(tj)
        return cls(eng, tok)

    def transcribe(self, audio, language: Optional[str] = None, max_new_tokens: int = 4096, beam_size: int = 1,
                   length_penalty: float = 0.0, suppress_tokens: Optional[Iterable[int]] = None,
                   logit_bias: Optional[Mapping[int, float]] = None, allowed_tokens: Optional[Iterable[int]] = None,
                   temperature=0.0, min_p: float = 0.0, seed: int = 0, logprob_threshold: float = -1.0,
                   compression_ratio_threshold: float = 2.4, repetition_penalty: float = 1.0,
                   no_repeat_ngram_size: int = 0, draft=None, hotwords: Optional[Iterable[str]] = None,
                   hotword_boost: Optional[float] = None, hotword_start_boost: float = 0.0,
                   banned_phrases: Optional[Iterable[str]] = None, sequence_bias=None, top_k: int = 0,
                   top_p: float = 1.0, top_logprobs: int = 0) -> TranscribeResult:
        """src/inference.rs:89-213.  `audio`: path to a WAV file or a 16 kHz float32 array.  beam_size > 1: a beam search of that
        width instead of the greedy loop; `alternatives` holds its hypotheses ordered by score / max(len, 1) ** length_penalty
        (float64 on the host; 0: the search's own order) and the result is the first of them.
        suppress_tokens / logit_bias / allowed_tokens (compose_logit_bias): constrain this call -- the engine's logit bias is set for
        it and whatever was set before is restored afterwards; composes with beam_size.
        temperature: a number > 0 samples this call at that temperature (HipEngine.set_sampling with min_p and seed; the engine's
        own setting is restored afterwards); the default 0.0 leaves the engine as it is.  A tuple such as (0.0, 0.2, 0.4, 0.6, 0.8,
        1.0) is Whisper's fallback (temperature_fallback): attempt k runs at temperatures[k] with seed + k, the first attempt with
        avg_logprob >= logprob_threshold and compression ratio <= compression_ratio_threshold is kept, else the last; it needs an
        engine created with token_logprobs=True.  The result's `temperature` is the one that was used.  Not with beam_size > 1.
        top_k / top_p: anything but (0, 1.0) sets HipEngine.set_sampling_filter for this call and restores the engine's own setting
        afterwards; every attempt of a temperature fallback runs under it (the greedy attempt ignores it).  Raises Q3aError when no
        temperature of the call is > 0: a filter without sampling would do nothing.
        repetition_penalty / no_repeat_ngram_size: anything but (1.0, 0) sets HipEngine.set_repetition for this call and restores the
        engine's own setting afterwards; every attempt of a temperature fallback runs under the same setting.  Not with beam_size > 1.
        draft: a transcript that is probably mostly right -- a list of ids, an earlier TranscribeResult (its ids) or a string (score()'s
        text convention: it needs `language`, and the ids are encode("<asr_text>" + text)).  The result is the greedy result; the ids of
        the draft the greedy loop would have written itself are verified in one prefill instead of decoded one by one, and
        `accepted_draft_tokens` says how many that were.  Composes with suppress_tokens / logit_bias / allowed_tokens; raises Q3aError
        with beam_size > 1, a temperature > 0 or repetition control.
        hotwords / banned_phrases / sequence_bias: a sequence bias for this call (HipEngine.set_sequence_bias; the engine's own list is
        restored afterwards).  hotwords: phrases to boost -- hotword_sequences(tokenizer, hotwords, hotword_boost,
        hotword_start_boost); hotword_boost has NO default and is required with hotwords: no value has been tuned on real weights.
        banned_phrases: phrases never to write -- the two tokenisations of each at -inf.  sequence_bias: entries given as ids, a
        mapping {tuple of ids: bias} or (ids, bias) pairs.  The three are concatenated in that order; a sequence named twice keeps the
        larger bias.  Composes with temperature, repetition_penalty, no_repeat_ngram_size and the logit-bias arguments; raises
        Q3aError with beam_size > 1 or a draft.
        top_logprobs: n in [1, 20] sets HipEngine.set_top_logprobs for this call (the engine's own setting is restored afterwards) and
        fills the result's `top_logprobs`: for every id of `ids` the n best candidates of the step that wrote it -- the row after the
        logit bias, the sequence bias and repetition control, untempered and unfiltered --, best first.  In a greedy call the first
        candidate is the id itself.  Composes with temperature (every attempt of a fallback; the kept attempt's candidates are
        returned), repetition control, hotwords and the logit-bias arguments; raises Q3aError with beam_size > 1 or a draft."""
        top_n = check_top_logprobs_args(top_logprobs)
        check_top_logprobs_compat(top_n, beam_size, draft)
        seq_entries = self._sequence_bias_entries(hotwords, hotword_boost, hotword_start_boost, banned_phrases, sequence_bias)
        if seq_entries is not None and beam_size > 1:
            raise Q3aError("transcribe: beam search has no sequence bias (beam_size > 1 with hotwords / banned_phrases / sequence_bias)")
        if seq_entries is not None and draft is not None:
            raise Q3aError("transcribe: a draft cannot be verified under a sequence bias (draft with hotwords / banned_phrases / sequence_bias)")
        rep_args = check_repetition_args(repetition_penalty, no_repeat_ngram_size)
        if beam_size > 1 and rep_args != (1.0, 0):
            raise Q3aError("transcribe: beam search has no repetition control (beam_size > 1 with repetition_penalty / no_repeat_ngram_size)")
        fallback = isinstance(temperature, (tuple, list))
        temps = [float(t) for t in temperature] if fallback else [float(temperature)]
        for t in temps:
            check_sampling_args(t, min_p, seed)
        filt_args = check_sampling_filter_args(top_k, top_p)
        if filt_args != (0, 1.0) and not any(t > 0.0 for t in temps):
            raise Q3aError("transcribe: top_k / top_p filter a sampled step: give a temperature > 0 with them")
        if fallback and not self.engine.token_logprobs:
            raise Q3aError("transcribe: a tuple of temperatures (fallback) decides on avg_logprob: create the engine with token_logprobs=True")
        if beam_size > 1 and any(t > 0.0 for t in temps):
            raise Q3aError("transcribe: beam search does not sample (beam_size > 1 with a temperature > 0)")
        draft_ids = None
        if draft is not None:
            check_draft_compat(beam_size, temps, rep_args)
            draft_ids = self._draft_ids(draft, language, max_new_tokens)
        run = lambda: self._transcribe(audio, language, max_new_tokens, beam_size, length_penalty, draft_ids)
        if fallback or temps[0] > 0.0:
            plain, eng = run, self.engine

            def attempt(t, sd):
                eng.set_sampling(t, min_p, sd)
                res = plain()
                res.temperature = t
                return res

            def run():
                before = eng.sampling_state
                try:
                    return temperature_fallback(attempt, temps, seed, logprob_threshold, compression_ratio_threshold)[0]
                finally:
                    eng.set_sampling(*before)
        if filt_args != (0, 1.0):
            inner_f, feng = run, self.engine

            def run():
                before = feng.sampling_filter_state
                feng.set_sampling_filter(*filt_args)
                try:
                    return inner_f()
                finally:
                    feng.set_sampling_filter(*before)
        if rep_args != (1.0, 0):
            inner, reng = run, self.engine

            def run():
                before = reng.repetition_state
                reng.set_repetition(*rep_args)
                try:
                    return inner()
                finally:
                    reng.set_repetition(*before)
        if seq_entries is not None:
            inner_sb, seng = run, self.engine

            def run():
                before = seng.sequence_bias_state
                seng.set_sequence_bias(seq_entries)
                try:
                    return inner_sb()
                finally:
                    seng.set_sequence_bias(before)
        if top_n:
            inner_tl, teng = run, self.engine

            def run():
                before = teng.top_logprobs_state
                teng.set_top_logprobs(top_n)
                try:
                    return inner_tl()
                finally:
                    teng.set_top_logprobs(before)
        if suppress_tokens is None and logit_bias is None and allowed_tokens is None:
            return run()
        ids, bias, default = compose_logit_bias(self.engine.dims.vocab_size, suppress_tokens, logit_bias, allowed_tokens)
        before = self.engine.logit_bias_state
        self.engine.set_logit_bias(dict(zip(ids.tolist(), bias.tolist())), default)
        try:
            return run()
        finally:
            self.engine.set_logit_bias(*before)

    _ROW_OPTION_KEYS = ("temperature", "min_p", "seed", "top_k", "top_p", "repetition_penalty", "no_repeat_ngram_size", "hotwords", "hotword_boost",
                        "hotword_start_boost", "banned_phrases", "sequence_bias", "top_logprobs")

    def transcribe_batch(self, audios, language: Optional[str] = None, max_new_tokens: int = 4096, options=None) -> List[TranscribeResult]:
        """transcribe() for several audios in ONE batch, each with its own decoding options (HipEngine.set_row_options): `options` holds
        one dict or None per audio, with transcribe's keys temperature (a number), min_p, seed, top_k, top_p, repetition_penalty,
        no_repeat_ngram_size, hotwords, hotword_boost, hotword_start_boost, banned_phrases and sequence_bias.  None is a plain greedy
        request.  The noise of a sampled row depends on its index in the batch.  `language` is one per call.  The engine's row table
        and sequence-bias lists are restored afterwards.  Raises Q3aError for a tuple of temperatures (fallback decides per attempt,
        not per row), beam_size, draft, the logit-bias arguments (one vector per engine) and top_k / top_p without a temperature > 0.
        The key top_logprobs is the exception to "its own": the engine records one n per batch, so it may be given only if it is equal
        for all rows (ValueError otherwise); the results then carry `top_logprobs` as transcribe's do."""
        audios = list(audios)
        options = [None] * len(audios) if options is None else list(options)
        if len(options) != len(audios):
            raise Q3aError(f"transcribe_batch: {len(options)} option dict(s) for {len(audios)} audio(s)")
        top_n = uniform_top_logprobs(options)
        rows = []
        for i, o in enumerate(options):
            o = dict(o) if o is not None else {}
            for key in ("beam_size", "draft"):
                if key in o:
                    raise Q3aError(f"transcribe_batch: options[{i}] has {key}: beam search and drafts do not run under per-row options")
            for key in ("suppress_tokens", "logit_bias", "allowed_tokens"):
                if key in o:
                    raise Q3aError(f"transcribe_batch: options[{i}] has {key}: the logit bias is one vector per engine, not per row")
            unknown = sorted(set(o) - set(self._ROW_OPTION_KEYS))
            if unknown:
                raise Q3aError(f"transcribe_batch: options[{i}] has unknown key(s) {unknown}")
            t = o.get("temperature", 0.0)
            if isinstance(t, (tuple, list)):
                raise Q3aError(f"transcribe_batch: options[{i}] has a tuple of temperatures: the fallback is transcribe()'s, one audio at a time")
            filt = check_sampling_filter_args(o.get("top_k", 0), o.get("top_p", 1.0))
            t = check_sampling_args(t, o.get("min_p", 0.0), o.get("seed", 0))[0]
            if filt != (0, 1.0) and not t > 0.0:
                raise Q3aError(f"transcribe_batch: options[{i}]: top_k / top_p filter a sampled step: give a temperature > 0 with them")
            entries = self._sequence_bias_entries(o.get("hotwords"), o.get("hotword_boost"), o.get("hotword_start_boost", 0.0),
                                                  o.get("banned_phrases"), o.get("sequence_bias"))
            rows.append(RowOptions(t, o.get("min_p", 0.0), o.get("seed", 0), filt[0], filt[1], o.get("repetition_penalty", 1.0),
                                   o.get("no_repeat_ngram_size", 0), entries))
        samples = [load_audio(os.fspath(a), 16000) if isinstance(a, (str, os.PathLike)) else np.asarray(a, dtype=np.float32) for a in audios]
        prefix = None
        if language is not None:
            if self.tokenizer is None:
                raise Q3aError("forcing a language needs tokenizer.json (src/inference.rs:246-251)")
            prefix = self.tokenizer.encode("language " + capitalize_first(language))
        eng = self.engine
        before, before_top = eng.row_options_state, eng.top_logprobs_state
        tops = None
        try:
            eng.set_row_options(rows)
            if top_n:
                eng.set_top_logprobs(top_n)
            all_ids = eng.transcribe_batch(samples, prefix, max_new_tokens)
            lps = eng.fetch_logprobs() if eng.token_logprobs else None
            if top_n:
                tops = eng.fetch_top_logprobs()
        finally:
            eng.set_row_options(before)
            if top_n:
                eng.set_top_logprobs(before_top)
        results = []
        for i, ids in enumerate(all_ids):
            raw = self.tokenizer.decode(ids, True) if self.tokenizer is not None else ""
            lang, text = parse_asr_output(raw, language is not None)
            res = TranscribeResult(text, lang, raw, ids)
            res.temperature = rows[i].temperature
            if lps is not None:
                res.token_logprobs = [float(v) for v in lps[i]]
                res.avg_logprob = float(np.mean(lps[i], dtype=np.float64)) if len(lps[i]) else None
            if tops is not None:
                res.top_logprobs = self._candidates(*tops[i])
            results.append(res)
        return results

    def _candidates(self, ids: np.ndarray, lp: np.ndarray) -> List[List[TokenCandidate]]:
        """fetch_top_logprobs' arrays of one utterance as TokenCandidate lists, one list per generated id."""
        text = (lambda i: self.tokenizer.decode([i], False)) if self.tokenizer is not None else (lambda i: "")
        return [[TokenCandidate(int(i), text(int(i)), float(v)) for i, v in zip(row_i, row_l)] for row_i, row_l in zip(ids, lp)]

    def _sequence_bias_entries(self, hotwords, hotword_boost, hotword_start_boost, banned_phrases, sequence_bias):
        """The call's sequence-bias entries, checked; None when none of the arguments was given."""
        if hotwords is None and banned_phrases is None and sequence_bias is None:
            if hotword_boost is not None:
                raise Q3aError("transcribe: hotword_boost without hotwords")
            return None
        pairs = []
        if hotwords is not None:
            if hotword_boost is None:
                raise Q3aError("transcribe: hotwords need hotword_boost (it has no default: no value has been tuned on real weights)")
            if self.tokenizer is None:
                raise Q3aError("hotwords need tokenizer.json (src/inference.rs:246-251)")
            pairs += hotword_sequences(self.tokenizer, hotwords, hotword_boost, hotword_start_boost)
        elif hotword_boost is not None:
            raise Q3aError("transcribe: hotword_boost without hotwords")
        if banned_phrases is not None:
            if self.tokenizer is None:
                raise Q3aError("banned_phrases need tokenizer.json (src/inference.rs:246-251)")
            pairs += banned_sequences(self.tokenizer, banned_phrases)
        pairs += _sequence_bias_pairs(sequence_bias)
        pairs = _merge_sequences(pairs)
        check_sequence_bias(pairs, self.engine.dims.vocab_size)
        return pairs

    def _draft_ids(self, draft, language, max_new_tokens) -> List[int]:
        if isinstance(draft, TranscribeResult):
            draft = draft.ids
        if isinstance(draft, str):
            if self.tokenizer is None:
                raise Q3aError("a text draft needs tokenizer.json (src/inference.rs:246-251)")
            if language is None:
                raise Q3aError("transcribe: a text draft needs `language` (the ids after a free-running prompt start with the language the model detects)")
            draft = self.tokenizer.encode("<asr_text>" + draft)
        return check_draft_ids(draft, self.engine.dims.vocab_size, min(int(max_new_tokens), self.engine.max_new_tokens))

    def _transcribe(self, audio, language, max_new_tokens, beam_size, length_penalty, draft_ids=None) -> TranscribeResult:
        if isinstance(audio, (str, os.PathLike)):
            samples = load_audio(os.fspath(audio), 16000)
        else:
            samples = np.asarray(audio, dtype=np.float32)
        prefix = None
        if language is not None:
            if self.tokenizer is None:
                raise Q3aError("forcing a language needs tokenizer.json (src/inference.rs:246-251)")
            prefix = self.tokenizer.encode("language " + capitalize_first(language))
        if beam_size > 1:
            hyps = self.engine.beam_search_batch([samples], beam_size, prefix, min(max_new_tokens, self.engine.max_new_tokens))[0]
            hyps = [h for h in hyps if h.score > -np.inf]
            if length_penalty != 0.0:  # (stable: equal keys keep the search's order)
                hyps = sorted(hyps, key=lambda h: -(float(h.score) / float(max(len(h.ids) + int(h.finished), 1)) ** float(length_penalty)))
            alts = []
            for h in hyps:
                raw = self.tokenizer.decode(h.ids, True) if self.tokenizer is not None else ""
                alts.append((Alternative(parse_asr_output(raw, language is not None)[1], h.score, h.ids), raw, h))
            alt, raw, best = alts[0]
            lang = parse_asr_output(raw, language is not None)[0]
            lps = best.token_logprobs[:len(best.ids)]
            return TranscribeResult(alt.text, lang, raw, best.ids, [float(v) for v in lps],
                                    float(np.mean(lps, dtype=np.float64)) if len(lps) else None, [a for a, _, _ in alts])
        accepted = None
        if draft_ids is not None:
            got, acc = self.engine.transcribe_draft_batch([samples], [draft_ids], prefix, min(max_new_tokens, self.engine.max_new_tokens))
            ids, accepted = got[0], acc[0]
        else:
            ids = self.engine.transcribe_batch([samples], prefix, max_new_tokens)[0]
        raw = self.tokenizer.decode(ids, True) if self.tokenizer is not None else ""
        lang, text = parse_asr_output(raw, language is not None)
        res = TranscribeResult(text, lang, raw, ids, accepted_draft_tokens=accepted)
        if self.engine.token_logprobs:
            lp = self.engine.fetch_logprobs()[0]
            res.token_logprobs = [float(v) for v in lp]
            res.avg_logprob = float(np.mean(lp, dtype=np.float64)) if len(lp) else None
        if self.engine.top_logprobs_state and beam_size <= 1 and draft_ids is None:
            res.top_logprobs = self._candidates(*self.engine.fetch_top_logprobs()[0])
        return res


    def score(self, audio, text_or_ids, language: Optional[str] = None, eos: bool = True) -> ScoreResult:
        """How likely the model finds a given transcript of `audio`, token by token (one prefill, no decode loop).  A list of ids is
        scored as given (the pinned contract).  A string needs `language`: the prompt carries the prefix transcribe() builds and the
        targets are encode("<asr_text>" + text) -- what a published checkpoint writes after a forced-language prompt as
        parse_asr_output reads it.  eos: also score <|im_end|> (151645) after the last id, i.e. "the transcript stops here"."""
        if isinstance(audio, (str, os.PathLike)):
            samples = load_audio(os.fspath(audio), 16000)
        else:
            samples = np.asarray(audio, dtype=np.float32)
        prefix = None
        if language is not None or isinstance(text_or_ids, str):
            if self.tokenizer is None:
                raise Q3aError("scoring text or forcing a language needs tokenizer.json (src/inference.rs:246-251)")
            if language is None:
                raise Q3aError("score: a text transcript needs `language` (the ids after a free-running prompt start with the language the model detects)")
            prefix = self.tokenizer.encode("language " + capitalize_first(language))
        if isinstance(text_or_ids, str):
            ids = [int(t) for t in self.tokenizer.encode("<asr_text>" + text_or_ids)]
        else:
            ids = [int(t) for t in text_or_ids]
        if eos:
            ids = ids + [EOS_TOKEN_IDS[1]]
        lp, top, top_lp = self.engine.score_batch([samples], [ids], prefix)[0]
        return ScoreResult(ids, [float(v) for v in lp], float(np.mean(lp, dtype=np.float64)) if len(lp) else None,
                           [int(t) for t in top], [float(v) for v in top_lp])


@dataclass
class StreamingUpdate:
    """One push of a StreamingTranscriber: the transcript of all audio so far, how many leading ids of the previous transcript stayed
    (0 on the first push), and the seconds of audio it covers."""
    result: TranscribeResult
    accepted: int
    audio_seconds: float


class StreamingTranscriber:
    """Incremental transcription on top of AsrInference.transcribe(draft=...): every push() transcribes ALL audio received so far with
    the previous transcript's ids as the draft, so what the new audio did not change is verified in one prefill instead of decoded
    again, and `accepted` -- the ids that stayed -- is read off the result instead of guessed with a roll-back heuristic.
    Each push re-runs the log-mel, the encoder and the prefill over the whole audio: the cost per update grows with the stream, and
    a bounded window for endless streams is out of scope.  transcribe_kwargs go to every transcribe call (max_new_tokens,
    suppress_tokens, ...); anything a draft does not combine with raises Q3aError at the first push."""

    def __init__(self, asr, language: Optional[str] = None, **transcribe_kwargs):
        if "draft" in transcribe_kwargs or "audio" in transcribe_kwargs:
            raise Q3aError("StreamingTranscriber: the draft and the audio are its own")
        self.asr, self.language, self.kwargs = asr, language, dict(transcribe_kwargs)
        self.reset()

    def reset(self):
        """Forget the audio and the previous transcript: the next push starts a new stream."""
        self._audio = np.zeros(0, dtype=np.float32)
        self._ids: List[int] = []
        self.last: Optional[StreamingUpdate] = None

    def push(self, samples) -> StreamingUpdate:
        """Append 16 kHz float32 samples and transcribe the audio so far."""
        self._audio = np.concatenate([self._audio, np.asarray(samples, dtype=np.float32).reshape(-1)])
        draft = []
        for t in self._ids:  # (an id a draft may not hold -- a model that wrote <|audio_pad|> -- ends it)
            if t == AUDIO_PAD_ID or t in EOS_TOKEN_IDS:
                break
            draft.append(t)
        res = self.asr.transcribe(self._audio, language=self.language, draft=draft, **self.kwargs)
        self._ids = [int(t) for t in res.ids]
        self.last = StreamingUpdate(res, int(res.accepted_draft_tokens or 0), len(self._audio) / 16000.0)
        return self.last

    def finish(self) -> Optional[StreamingUpdate]:
        """The last update (None when nothing was pushed); the stream is reset."""
        last = self.last
        self.reset()
        return last


class ForcedAligner:
    """Word timestamps with a Qwen3-ForcedAligner checkpoint (HF Qwen3ASRProcessor.prepare_forced_aligner_inputs +
    Qwen3ASRForTokenClassification + decode_forced_alignment), every number from the HIP engine."""

    def __init__(self, engine: HipEngine, tokenizer: AsrTokenizer):
        info = engine.aligner_info()
        if info["classify_num"] <= 0:
            raise Q3aError("ForcedAligner: not a forced-aligner checkpoint (config.json has no thinker_config.classify_num)")
        self.engine, self.tokenizer = engine, tokenizer
        self.timestamp_token_id, self.segment_ms = info["timestamp_token_id"], info["segment_ms"]

    @classmethod
    def load(cls, model_dir: str, device: int = 0, precise: bool = False) -> "ForcedAligner":
        return cls(HipEngine(model_dir, device, precise=precise, max_new_tokens=1), AsrTokenizer.from_dir(model_dir))

    def _text_ids(self, words: Sequence[str]) -> List[int]:
        return self.tokenizer.align_text_ids(words, self.timestamp_token_id)

    def _decode(self, words: Sequence[str], classes: Sequence[int]) -> List[dict]:
        ms = fix_timestamps([float(c) * self.segment_ms for c in classes]) if len(classes) else []
        return [{"text": w, "start_time": round(ms[2 * i] / 1000.0, 3), "end_time": round(ms[2 * i + 1] / 1000.0, 3)}
                for i, w in enumerate(words)]

    def align_batch(self, clips: Sequence, transcripts: Sequence[str], language: Optional[str] = None) -> List[List[dict]]:
        """One list of {"text", "start_time", "end_time"} (seconds, rounded to ms) per clip."""
        if len(clips) != len(transcripts):
            raise Q3aError(f"ForcedAligner: {len(transcripts)} transcript(s) for {len(clips)} clip(s)")
        samples = [load_audio(os.fspath(a), 16000) if isinstance(a, (str, os.PathLike)) else np.asarray(a, dtype=np.float32)
                   for a in clips]
        words = [split_words_for_alignment(t, language) for t in transcripts]
        classes = self.engine.align_batch(samples, [self._text_ids(w) for w in words])
        return [self._decode(w, c) for w, c in zip(words, classes)]

    def align(self, audio, transcript: str, language: Optional[str] = None) -> List[dict]:
        return self.align_batch([audio], [transcript], language)[0]
