"""CPU tests of draft-verified decoding's host side: the next-round helper of the C ABI against the numpy reference, the Python
argument refusals, and StreamingTranscriber's bookkeeping driven by a stub AsrInference (no GPU, no engine)."""
import numpy as np
import pytest

import draft_ref
from qwen3_asr_rs_amd import engine as E
from qwen3_asr_rs_amd.engine import Q3aError, StreamingTranscriber, StreamingUpdate, TranscribeResult

EOS0, EOS1 = draft_ref.EOS_IDS


@pytest.mark.parametrize("draft,k,tok", [
    ([5, 6, 7], 3, 9),          # an empty tail: everything accepted, the head's next id is appended
    ([5, 6, 7], 0, 9),          # k = 0
    ([5, 6, 7], 2, 9),          # k = n - 1
    ([5, 6, 7, 8, 10], 2, 9),   # a substitution in the middle: the tail stays
    ([5, 6, 7, 8], 1, EOS0),    # the model stops at k: the tail is dropped
    ([5, 6, 7, 8], 4, EOS1),
    ([], 0, 4),
    ([], 0, EOS1),
])
def test_next_round_matches_the_reference(lib, draft, k, tok):
    want = draft_ref.next_round(draft, k, tok)
    got, need = E.draft_next_round(draft, k, tok)
    assert got == want and need == len(want)
    # a short cap: the count is still the full answer's, and only cap ids are written
    for cap in (0, 1, max(len(want) - 1, 0)):
        got, need = E.draft_next_round(draft, k, tok, cap=cap)
        assert need == len(want) and got == want[:cap]


def test_next_round_refuses_bad_arguments(lib):
    for draft, k in (([1, 2], 3), ([1, 2], -1)):
        with pytest.raises(Q3aError, match="q3a_draft_next_round"):
            E.draft_next_round(draft, k, 7)


def test_python_argument_refusals():
    V = 151936
    assert E.check_draft_ids([1, np.int32(2), 3], V, 3) == [1, 2, 3]
    assert E.check_draft_ids([], V, 0) == []
    for bad, msg in (([1, -1], "outside the vocabulary"), ([V], "outside the vocabulary"), ([draft_ref.AUDIO_PAD], "audio_pad"),
                     ([3, EOS0], "EOS"), ([EOS1], "EOS"), ([1.5], "not an integer"), ([True], "not an integer"), ([1, 2, 3, 4], "more than max_new")):
        with pytest.raises(Q3aError, match=msg):
            E.check_draft_ids(bad, V, 3)
    E.check_draft_compat(1, [0.0], (1.0, 0))
    for args, msg in (((2, [0.0], (1.0, 0)), "beam"), ((1, [0.0, 0.4], (1.0, 0)), "sampling"), ((1, [0.0], (1.2, 0)), "repetition"),
                      ((1, [0.0], (1.0, 3)), "repetition")):
        with pytest.raises(Q3aError, match=msg):
            E.check_draft_compat(*args)

    class NoEngine:   # transcribe() must refuse before it touches the engine
        def __getattr__(self, name):
            raise AssertionError(f"the engine was touched ({name})")

    asr = E.AsrInference(NoEngine(), None)
    clip = np.zeros(16000, np.float32)
    for kw, msg in ((dict(beam_size=2), "beam"), (dict(temperature=0.5), "sampling"), (dict(repetition_penalty=1.3), "repetition"),
                    (dict(no_repeat_ngram_size=2), "repetition")):
        with pytest.raises(Q3aError, match=msg):
            asr.transcribe(clip, draft=[1, 2, 3], **kw)
    with pytest.raises(Q3aError, match="tokenizer"):
        asr.transcribe(clip, draft="some text", language="english")
    assert TranscribeResult("", "", "", []).accepted_draft_tokens is None
    assert E.DRAFT_MIN_TAIL >= 1


class StubAsr:
    """Stands in for AsrInference: records what transcribe() is given and answers from a script of (ids per push)."""

    def __init__(self, script):
        self.script, self.calls = list(script), []

    def transcribe(self, audio, language=None, draft=None, **kw):
        self.calls.append({"n": len(audio), "language": language, "draft": list(draft), "kw": kw})
        ids = self.script[len(self.calls) - 1]
        return TranscribeResult("", "", "", list(ids), accepted_draft_tokens=draft_ref.accept_from_greedy(draft, ids, 64))


def test_streaming_transcriber_bookkeeping():
    script = [[10, 11, 12], [10, 11, 12, 13, 14], [10, 11, 99, 13, 14, 15], [20, 21]]
    stub = StubAsr(script)
    st = StreamingTranscriber(stub, language="english", max_new_tokens=64)
    pieces = [np.full(8000, 0.1, np.float32), np.full(4000, 0.2, np.float32), np.full(12000, 0.3, np.float32)]
    ups = [st.push(p) for p in pieces]
    assert all(isinstance(u, StreamingUpdate) for u in ups)
    # every push transcribes ALL audio so far, with the previous push's ids as the draft (none on the first)
    assert [c["n"] for c in stub.calls] == [8000, 12000, 24000]
    assert [c["draft"] for c in stub.calls] == [[], script[0], script[1]]
    assert all(c["language"] == "english" and c["kw"] == {"max_new_tokens": 64} for c in stub.calls)
    assert [u.result.ids for u in ups] == script[:3]
    assert [u.accepted for u in ups] == [0, 3, 2]   # the ids that stayed
    assert [u.audio_seconds for u in ups] == [0.5, 0.75, 1.5]
    # finish() returns the last update and resets; reset() clears the draft and the audio
    assert st.finish() is ups[2] and st.last is None
    up = st.push(pieces[1])
    assert stub.calls[-1]["draft"] == [] and stub.calls[-1]["n"] == 4000 and up.accepted == 0 and up.result.ids == script[3]
    st.reset()
    assert st.finish() is None
    # an id a draft may not hold ends the draft of the next push
    stub2 = StubAsr([[1, 2, draft_ref.AUDIO_PAD, 4], [1, 2, 3]])
    st2 = StreamingTranscriber(stub2)
    st2.push(pieces[0]); st2.push(pieces[0])
    assert stub2.calls[1]["draft"] == [1, 2]
    with pytest.raises(Q3aError):
        StreamingTranscriber(stub, draft=[1])
