"""Forced aligner (Qwen3-ForcedAligner word timestamps) on the GPU: the prefill of the aligner prompts and the classifier head
(k_align.hip) against the fp32 oracle, the tie rule, batch independence, the refusals of both engine kinds and the end-to-end
paths (ForcedAligner, the asr CLI with Q3A_ALIGNER)."""
import json
import os
import shutil
import subprocess
import wave

import numpy as np
import pytest

from align_ref import TS, aligner_0p6b_dir, oracle_align, tiny_aligner_dir, top2_margin, word_ids
from oracle import q3asr_oracle as O
from qwen3_asr_rs_amd import synthetic
from qwen3_asr_rs_amd.audio import build_align_prompt
from qwen3_asr_rs_amd.engine import ForcedAligner, HipEngine, HipGroup, Q3aError

pytestmark = pytest.mark.gpu

LOGIT_TOL = 0.01     # default-mode max |logit error| as a fraction of the largest |logit| (tests/test_gpu_configs.py: 1 % of the logit scale)
MAX_FLIPS = 0.02     # fraction of markers whose default-mode class may differ from the oracle's (under the margin rule)
TIE_MARGIN = 1e-3    # precise mode: oracle top-1/top-2 gaps below this are rounding ties


def _clips(n, seed0=60, base=1.0):
    return [synthetic.synthetic_clip(seed0 + i, base + 0.25 * (i % 4)) for i in range(n)]


def _texts(n, seed0=7):
    """Ragged word counts, one empty transcript when n > 1 (count 0 is not an error)."""
    return [word_ids(0 if (n > 1 and i == 3) else 1 + (5 * i + seed0) % 12, seed0 + i) for i in range(n)]


def _stage(eng, clips, texts, want_logits=False):
    eng.mel(clips)
    eng.encode()
    return eng.align([build_align_prompt(t, x) for t, x in zip(eng._T, texts)], want_logits=want_logits)


@pytest.fixture(scope="module")
def tiny_al():
    return tiny_aligner_dir()


@pytest.fixture(scope="module")
def al_0p6b():
    return aligner_0p6b_dir()


_ORACLES = {}


def _oracle_run(d, clips, texts):
    if d not in _ORACLES:
        _ORACLES[d] = O.AsrOracle(d)
    return [oracle_align(_ORACLES[d], c, t)[1] for c, t in zip(clips, texts)]


@pytest.mark.parametrize("which,B", [("tiny", 1), ("tiny", 32), ("0p6b", 1), ("0p6b", 32)])
def test_classes_match_oracle(request, which, B):
    d = request.getfixturevalue("tiny_al" if which == "tiny" else "al_0p6b")
    clips, texts = _clips(B), _texts(B)
    ref = _oracle_run(d, clips, texts)
    # precise mode: the oracle's classes wherever its own top-2 margin is not a rounding tie
    eng = HipEngine(d, 0, precise=True, max_new_tokens=1)
    cls_p, _ = _stage(eng, clips, texts)
    eng.close()
    n = skipped = 0
    for b in range(B):
        assert len(cls_p[b]) == len(ref[b]) == sum(1 for x in texts[b] if x == TS)
        for k, c in enumerate(cls_p[b]):
            n += 1
            if top2_margin(ref[b][k]) < TIE_MARGIN:
                skipped += 1
                continue
            assert c == int(ref[b][k].argmax()), (which, B, b, k)
    assert skipped <= 0.02 * n + 1, (skipped, n)
    # default mode: classes wherever the margin exceeds twice the measured logit error, at most MAX_FLIPS flips, logits in tolerance
    eng = HipEngine(d, 0, max_new_tokens=1)
    cls_d, lg = _stage(eng, clips, texts, want_logits=True)
    eng.close()
    flat_ref = np.concatenate([r for r in ref if len(r)])
    err = np.abs(lg - flat_ref).max(-1)
    assert float(err.max()) <= LOGIT_TOL * float(np.abs(flat_ref).max()), (float(err.max()), float(np.abs(flat_ref).max()))
    flips = 0
    k = 0
    for b in range(B):
        for c in cls_d[b]:
            assert c == int(lg[k].argmax())
            o = int(flat_ref[k].argmax())
            if top2_margin(flat_ref[k]) > 2 * err[k]:
                assert c == o, (which, B, b, k)
            flips += int(c != o)
            k += 1
    assert flips <= max(1, MAX_FLIPS * k), (flips, k)  # (every flip is under the margin, asserted above; one is allowed at 16 markers)
    print(f"[align] {which} B={B}: {k} markers, precise skipped {skipped}, default flips {flips}, max |logit err| {err.max():.4f}")


@pytest.fixture(scope="module")
def twin_head_dir(tiny_al):
    """The tiny aligner with classifier rows 2500 .. 4999 replaced by rows 0 .. 2499: every logit has an exact twin in another
    column tile, strip and partial, so the argmax meets a tie at its maximum."""
    d = "/tmp/q3a_ckpt_tiny_aligner_twin"
    if os.path.exists(d):
        shutil.rmtree(d)
    shutil.copytree(tiny_al, d)
    head = synthetic.read_tensor(d, "thinker.lm_head.weight").astype(np.float32)
    head[2500:] = head[:2500]
    synthetic.overwrite_tensor(d, "thinker.lm_head.weight", head)
    return d


@pytest.mark.parametrize("precise", [False, True])
def test_ties_take_the_first_class(twin_head_dir, precise):
    clips, texts = _clips(5, 80), _texts(5, 3)
    eng = HipEngine(twin_head_dir, 0, precise=precise, max_new_tokens=1)
    cls, lg = _stage(eng, clips, texts, want_logits=True)
    whole = eng.align_batch(clips, texts)
    eng.close()
    flat = [c for row in cls for c in row]
    assert flat and all(c < 2500 for c in flat), flat
    assert np.array_equal(lg[:, :2500], lg[:, 2500:])
    assert [int(x) for x in lg.argmax(-1)] == flat
    assert whole == cls


def test_alone_equals_inside_a_batch(tiny_al):
    clips, texts = _clips(32, 100), _texts(32, 11)
    eng = HipEngine(tiny_al, 0, max_new_tokens=1)
    batch = eng.align_batch(clips, texts)
    _, lg = _stage(eng, clips, texts, want_logits=True)
    alone = eng.align_batch([clips[5]], [texts[5]])[0]
    eng.close()
    off = sum(len(batch[b]) for b in range(5))
    for k, (a, c) in enumerate(zip(alone, batch[5])):
        if a != c:
            assert top2_margin(lg[off + k]) <= 2 * LOGIT_TOL * float(np.abs(lg).max()), (k, a, c)
    assert sum(int(a != c) for a, c in zip(alone, batch[5])) <= max(1, MAX_FLIPS * len(alone))
    assert len(alone) == len(batch[5]) == sum(1 for x in texts[5] if x == TS)


def test_whole_path_equals_stage_form_and_timings(tiny_al):
    clips, texts = _clips(4, 120), _texts(4, 5)
    eng = HipEngine(tiny_al, 0, max_new_tokens=1)
    whole = eng.align_batch(clips, texts)
    t = eng.timings()
    assert t["decode_steps"] == 0 and t["prefill_ms"] > 0 and t["encoder_ms"] > 0 and t["mel_ms"] > 0
    head_ms = float(eng.debug_read("align_head_ms")[0])
    assert 0 < head_ms < t["prefill_ms"]
    stage, _ = _stage(eng, clips, texts)
    assert whole == stage
    assert eng.aligner_info() == {"classify_num": 5000, "timestamp_token_id": TS, "segment_ms": 80.0}
    eng.close()


def test_refusals(tiny_al, tiny_dir):
    clip = _clips(1)[0]
    al = HipEngine(tiny_al, 0, max_new_tokens=4)
    asr = HipEngine(tiny_dir, 0, max_new_tokens=4)
    ref_ids = asr.transcribe_batch([clip], None, max_new=4, fixed_new_tokens=4)
    # an aligner engine refuses every transcription entry point
    with pytest.raises(Q3aError, match="forced aligner"):
        al.transcribe_batch([clip], None, max_new=4, fixed_new_tokens=4)
    al.mel([clip])
    al.encode()
    with pytest.raises(Q3aError, match="forced aligner"):
        al.prefill([HipEngine.build_prompt(al._T[0])])
    with pytest.raises(Q3aError, match="forced aligner"):
        al.decode_step()
    with pytest.raises(Q3aError, match="forced aligner"):
        al.run_resident(None, 4, 4)
    pcm = np.ascontiguousarray(clip, dtype=np.float32)
    ns = np.array([len(pcm)], dtype=np.int64)
    import ctypes as C
    out, lens = np.zeros(4, np.int32), np.zeros(1, np.int32)
    rc = al._lib.q3a_transcribe_batch(al._h, pcm.ctypes.data_as(C.POINTER(C.c_float)), ns.ctypes.data_as(C.POINTER(C.c_int64)), 1,
                                      None, 0, 4, 4, out.ctypes.data_as(C.POINTER(C.c_int32)), 4, lens.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc != 0 and b"forced aligner" in al._lib.q3a_last_error(al._h)
    with pytest.raises(Q3aError, match="forced-aligner checkpoint cannot serve"):
        HipGroup(tiny_al, 1)
    # a stride below an utterance's marker count; an empty transcript is not an error
    text = word_ids(3, 1)
    with pytest.raises(Q3aError, match="stride"):
        al.align_batch([clip], [text], stride=5)
    al.mel([clip])
    al.encode()
    with pytest.raises(Q3aError, match="stride"):
        al.align([build_align_prompt(al._T[0], text)], stride=2)
    assert al.align_batch([clip, clip], [[], text])[0] == []
    # an ASR engine refuses q3a_align*
    asr.mel([clip])
    asr.encode()
    with pytest.raises(Q3aError, match="not a forced-aligner"):
        asr.align([build_align_prompt(asr._T[0], text)])
    with pytest.raises(Q3aError, match="not a forced-aligner"):
        asr.align_batch([clip], [text])
    assert asr.aligner_info()["classify_num"] == 0
    # the ASR engine's ids are what they were before the aligner ran in this process
    assert asr.transcribe_batch([clip], None, max_new=4, fixed_new_tokens=4) == ref_ids
    al.close()
    asr.close()


def _tokenizer_dir(src, dst):
    """A model directory with a synthetic tokenizer.json: id i <-> "t{i}" as in test_gpu_parity.py, except that the last 36 ids
    are the single letters and digits the aligner's word ids are encoded from."""
    os.makedirs(dst, exist_ok=True)
    for f in os.listdir(src):
        if f.endswith((".json", ".safetensors")) and not os.path.exists(os.path.join(dst, f)):
            os.symlink(os.path.join(src, f), os.path.join(dst, f))
    chars = "abcdefghijklmnopqrstuvwxyz0123456789"
    vocab = {f"t{i}": i for i in range(151936 - len(chars)) if i not in (151643, 151645)}
    vocab.update({c: 151936 - len(chars) + k for k, c in enumerate(chars)})
    tok = {"version": "1.0", "added_tokens": [{"id": 151643, "content": "<|endoftext|>", "special": True},
                                              {"id": 151645, "content": "<|im_end|>", "special": True}],
           "model": {"type": "BPE", "vocab": vocab, "merges": []}}
    with open(os.path.join(dst, "tokenizer.json"), "w") as f:
        json.dump(tok, f)
    return dst


def test_forced_aligner_end_to_end(tiny_al, tmp_path):
    d = _tokenizer_dir(tiny_al, str(tmp_path / "aligner"))
    fa = ForcedAligner.load(d, 0)
    transcript = "the quick brown fox, jumps over 12 lazy dogs"
    res = fa.align(_clips(1, 140, 3.0)[0], transcript)
    assert [r["text"] for r in res] == ["the", "quick", "brown", "fox", "jumps", "over", "12", "lazy", "dogs"]
    times = [t for r in res for t in (r["start_time"], r["end_time"])]
    assert all(a <= b for a, b in zip(times, times[1:])), times
    assert all(t == round(t, 3) and 0 <= t < 400 for t in times)
    both = fa.align_batch(_clips(2, 140, 3.0), [transcript, "one two"])
    assert both[0] == res and [r["text"] for r in both[1]] == ["one", "two"]


def test_cli_word_lines(tiny_dir, tiny_al, tmp_path):
    from qwen3_asr_rs_amd.build import CLI_PATH
    mdir = _tokenizer_dir(tiny_dir, str(tmp_path / "asr"))
    adir = _tokenizer_dir(tiny_al, str(tmp_path / "aligner"))
    clip = synthetic.synthetic_clip(12, 2.0)
    wav = tmp_path / "clip.wav"
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes((np.clip(clip, -1, 1) * 32767).astype("<i2").tobytes())
    env = dict(os.environ, RUST_LOG="warn")
    env.pop("Q3A_ALIGNER", None)
    plain = subprocess.run([CLI_PATH, mdir, str(wav)], capture_output=True, text=True, timeout=600, env=env)
    assert plain.returncode == 0, plain.stderr
    assert not any(l.startswith("Word: ") for l in plain.stdout.split("\n"))
    withal = subprocess.run([CLI_PATH, mdir, str(wav)], capture_output=True, text=True, timeout=600, env=dict(env, Q3A_ALIGNER=adir))
    assert withal.returncode == 0, withal.stderr
    lines = withal.stdout.strip().split("\n")
    head = plain.stdout.strip().split("\n")
    assert lines[:len(head)] == head
    words = lines[len(head):]
    assert words and all(l.startswith("Word: ") for l in words)
    text = head[1][len("Text: "):]
    from qwen3_asr_rs_amd.audio import split_words_for_alignment
    assert [l.split(" ", 3)[3] for l in words] == split_words_for_alignment(text)
    times = [float(x) for l in words for x in l.split(" ")[1:3]]
    assert all(a <= b for a, b in zip(times, times[1:])), times
