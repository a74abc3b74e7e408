"""WAV ingest and text glue of the pipeline shell -- thin ctypes wrappers over the C++ host code
(csrc/host_audio.cpp, csrc/host_text.cpp), so the Python tests, the `asr` CLI and a Rust shim all share ONE
implementation.  Reference: src/audio.rs:7 (load_audio), src/tokenizer.rs (AsrTokenizer), src/inference.rs:276-313."""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib


def _err() -> str:
    return (_lib.load().q3a_last_error(None) or b"").decode()


def _take(ptr, n) -> np.ndarray:
    lib = _lib.load()
    out = np.ctypeslib.as_array(ptr, shape=(max(int(n), 1),))[:int(n)].copy()
    lib.q3a_free(C.cast(ptr, C.c_void_p))
    return out


def load_audio(path: str, target_sr: int = 16000) -> np.ndarray:
    """src/audio.rs:7 load_audio(path, target_sample_rate) -> mono f32 at the target rate (WAV input)."""
    lib = _lib.load()
    p, n = C.POINTER(C.c_float)(), C.c_int64()
    if lib.q3a_load_audio(os.fsencode(path), target_sr, C.byref(p), C.byref(n)) != 0:
        raise RuntimeError(_err())
    return _take(p, n.value)


def resample(x: np.ndarray, sr_in: int, sr_out: int, method: str = "polyphase") -> np.ndarray:
    """method "polyphase": this backend's Kaiser polyphase filter; "rubato": the reference fallback's resampler
    (src/audio.rs:220-245) restated (see include/q3asr.h q3a_resample_rubato)."""
    lib = _lib.load()
    x = np.ascontiguousarray(x, dtype=np.float32)
    p, n = C.POINTER(C.c_float)(), C.c_int64()
    fn = lib.q3a_resample_rubato if method == "rubato" else lib.q3a_resample
    if fn(x.ctypes.data_as(C.POINTER(C.c_float)), len(x), sr_in, sr_out, C.byref(p), C.byref(n)) != 0:
        raise RuntimeError(_err())
    return _take(p, n.value)


class AsrTokenizer:
    """src/tokenizer.rs:4-50 over tokenizer.json (byte-level BPE): decode(ids) with special tokens skipped,
    encode(text) for the ASCII forced-language prompt."""

    def __init__(self, tokenizer_json: str):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        if self._lib.q3a_tokenizer_create(os.fsencode(tokenizer_json), C.byref(self._h)) != 0:
            raise RuntimeError(_err())

    @classmethod
    def from_dir(cls, model_dir: str) -> "AsrTokenizer":
        return cls(os.path.join(model_dir, "tokenizer.json"))

    def decode(self, ids: Sequence[int], skip_special_tokens: bool = True) -> str:
        a = np.asarray(list(ids), dtype=np.int32)
        n = C.c_int32()
        ap = a.ctypes.data_as(C.POINTER(C.c_int32))
        if self._lib.q3a_tokenizer_decode(self._h, ap, len(a), int(skip_special_tokens), None, 0, C.byref(n)) != 0:
            raise RuntimeError(_err())
        buf = C.create_string_buffer(n.value + 1)
        self._lib.q3a_tokenizer_decode(self._h, ap, len(a), int(skip_special_tokens), buf, n.value + 1, C.byref(n))
        return buf.raw[:n.value].decode("utf-8")

    def encode(self, text: str) -> List[int]:
        ids = np.zeros(max(4 * len(text), 16), dtype=np.int32)
        n = C.c_int32()
        if self._lib.q3a_tokenizer_encode(self._h, text.encode("utf-8"), ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), C.byref(n)) != 0:
            raise RuntimeError(_err())
        return ids[:n.value].tolist()

    def align_text_ids(self, words: Sequence[str], timestamp_token_id: int) -> List[int]:
        """The word and marker part of a forced-aligner prompt: encode(word) + two markers per word (q3a_align_text_ids)."""
        arr = (C.c_char_p * max(len(words), 1))(*[w.encode("utf-8") for w in words])
        n = C.c_int32()
        if self._lib.q3a_align_text_ids(self._h, arr, len(words), int(timestamp_token_id), None, 0, C.byref(n)) != 0:
            raise RuntimeError(_err())
        ids = np.zeros(max(n.value, 1), dtype=np.int32)
        if self._lib.q3a_align_text_ids(self._h, arr, len(words), int(timestamp_token_id), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                        len(ids), C.byref(n)) != 0:
            raise RuntimeError(_err())
        return ids[:n.value].tolist()

    def __del__(self):
        try:
            if self._h.value:
                self._lib.q3a_tokenizer_destroy(self._h)
        except Exception:
            pass


def parse_asr_output(raw: str, language_forced: bool) -> Tuple[str, str]:
    """src/inference.rs:276-305"""
    lib = _lib.load()
    lang = C.create_string_buffer(1024)
    text = C.create_string_buffer(4 * len(raw.encode("utf-8")) + 64)
    if lib.q3a_parse_asr_output(raw.encode("utf-8"), int(language_forced), lang, len(lang), text, len(text)) != 0:
        raise RuntimeError(_err())
    return lang.value.decode("utf-8"), text.value.decode("utf-8")


def capitalize_first(s: str) -> str:
    """src/inference.rs:307-313"""
    lib = _lib.load()
    out = C.create_string_buffer(len(s.encode("utf-8")) + 8)
    lib.q3a_capitalize_first(s.encode("utf-8"), out, len(out))
    return out.value.decode("utf-8")


def normalize_nfc(s: str) -> str:
    """The normaliser step of the tokenizer (Unicode NFC, csrc/host_text.cpp normalize_nfc)."""
    lib = _lib.load()
    raw = s.encode("utf-8")
    n = C.c_int32()
    out = C.create_string_buffer(3 * len(raw) + 16)
    if lib.q3a_normalize_nfc(raw, out, len(out), C.byref(n)) != 0:
        raise RuntimeError(_err())
    return out.raw[:n.value].decode("utf-8")


def split_words_for_alignment(text: str, language: Optional[str] = None) -> List[str]:
    """Words of a transcript as the forced aligner splits them (csrc/host_align.cpp; Japanese / Korean are refused)."""
    lib = _lib.load()
    raw = text.encode("utf-8")
    n_words, n = C.c_int32(), C.c_int32()
    lang = language.encode("utf-8") if language else None
    out = C.create_string_buffer(len(raw) * 2 + 16)
    if lib.q3a_split_words_for_alignment(raw, lang, out, len(out), C.byref(n_words), C.byref(n)) != 0:
        raise RuntimeError(_err())
    s = out.raw[:n.value].decode("utf-8")
    return s.split("\n") if n_words.value else []


def fix_timestamps(ms: Sequence[float]) -> List[int]:
    """Monotone marker times in ms (csrc/host_align.cpp q3a_fix_timestamps: LIS, snapping, interpolation)."""
    lib = _lib.load()
    a = np.ascontiguousarray(np.asarray(ms, dtype=np.float32))
    out = np.zeros(max(len(a), 1), dtype=np.float32)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    if lib.q3a_fix_timestamps(fp(a), len(a), fp(out)) != 0:
        raise RuntimeError(_err())
    return [int(v) for v in out[:len(a)]]


def build_align_prompt(num_audio_tokens: int, text_ids: Sequence[int]) -> List[int]:
    """The forced aligner's prompt (q3a_build_align_prompt): audio start, pads, audio end, then the word and marker ids."""
    lib = _lib.load()
    t = np.ascontiguousarray(np.asarray(list(text_ids), dtype=np.int32))
    tp = t.ctypes.data_as(C.POINTER(C.c_int32)) if len(t) else None
    n = C.c_int32()
    if lib.q3a_build_align_prompt(int(num_audio_tokens), tp, len(t), None, C.byref(n)) != 0:
        raise RuntimeError(_err())
    ids = np.zeros(n.value, dtype=np.int32)
    lib.q3a_build_align_prompt(int(num_audio_tokens), tp, len(t), ids.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n))
    return ids.tolist()
