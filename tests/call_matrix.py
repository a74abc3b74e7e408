"""The engine's call order as a whole: every probe call issued at every state an engine can be driven to, and what came back.

One driver for the recorder (tools/record_call_matrix.py) and the test (tests/test_gpu_call_matrix.py), so the two cannot drift.
A row is (engine, state, probe) -> (return code, full q3a_last_error text; a success records an empty text).  Before every probe
the state is driven again from a reset -- every decoding setting off (which also ends whatever search or decode state the last
probe left), then a fresh upload -- so the engine's own state never carries over from the rows before.  The one state that cannot
be re-driven, "created", is probed first on the fresh engine: every probe is refused there and a refused probe leaves nothing behind.

Two things about the texts.  A HIP error names the source position of the failing call ("at <path>/engine.cpp:2368 (...)"): the
position is where the checkout lies and how long the file is, not behaviour, so it is recorded as "at <file>:<line> (...)"; the
rest of the text is compared as it is.  And HIP's last-error word belongs to the thread, not to the engine: q3a_decode_step on an
engine without a prompt fails in a copy from a buffer that does not exist yet, and q3a_run_resident, later in the same row of
probes, reports that stale error from its own check.  Both rows are part of the recording; the order of the probes is fixed.

The model is the tiny synthetic checkpoint (the smallest shape that reaches every state) and the tiny forced aligner; the two clips
are under a second and equally long, so a prompt built for one fits the other, and the same clip stands in both sequences wherever
a beam of width 2 may begin (its slots must hold equal prompts)."""
import re

from qwen3_asr_rs_amd import synthetic
from qwen3_asr_rs_amd.engine import HipEngine, Q3aError

from align_ref import align_prompt, tiny_aligner_dir, word_ids

MAX_NEW = 8
TARGETS = [[1000, 2000, 3000]] * 2
DRAFTS = [[1000, 2000]] * 2
BIAS = {1000: 1.5}

ASR_PROBES = ["encode", "prefill", "decode_step", "set_next_tokens", "fetch_ids", "fetch_logprobs", "beam_begin", "beam_step", "beam_fetch",
              "score", "prefill_draft", "run_resident", "align", "profile_decode_step", "set_logit_bias"]
ALIGNER_PROBES = ["prefill", "score", "align", "set_logit_bias", "beam_begin"]


class _Driver:
    def __init__(self, model_dir, **opts):
        self.eng = HipEngine(model_dir, 0, max_new_tokens=MAX_NEW, **opts)
        self.clip_a = synthetic.synthetic_clip(0, 0.6)
        self.clip_b = synthetic.synthetic_clip(1, 0.6)
        self.same, self.two = [self.clip_a, self.clip_a], [self.clip_a, self.clip_b]
        T = self.eng.num_audio_tokens(len(self.clip_a))
        self.prompts = [HipEngine.build_prompt(T)] * 2
        self.bad_prompts = [HipEngine.build_prompt(T + 1)] * 2  # one <|audio_pad|> too many
        self.align_prompts = [align_prompt(T, word_ids(2, 5))] * 2
        self.last = (0, "")
        self.eng._chk = self._chk  # (the wrapper's own check, so that a row holds the code the C ABI returned)

    def _chk(self, rc):
        if rc != 0:
            text = (self.eng._lib.q3a_last_error(self.eng._h) or b"").decode()
            text = re.sub(r"^(HIP error: .*? at )\S+:\d+ \(", r"\1<file>:<line> (", text)
            self.last = (int(rc), text)
            raise Q3aError(text)

    def call(self, name):
        """(rc, error text) of one probe; the arguments are the same at every state."""
        e = self.eng
        e.batch, e._beam_width = 2, 2  # (the wrapper sizes its buffers by these)
        e._n_frames = [(len(self.clip_a) + 159) // 160] * 2
        fn = {
            "encode": e.encode,
            "prefill": lambda: e.prefill(self.prompts, want_logits=False),
            "bad_prefill": lambda: e.prefill(self.bad_prompts, want_logits=False),
            "decode_step": lambda: e.decode_step(want_logits=False),
            "set_next_tokens": lambda: e.set_next_tokens([1000, 1000]),
            "fetch_ids": lambda: e.fetch_ids(MAX_NEW),
            "fetch_logprobs": e.fetch_logprobs,
            "beam_begin": lambda: e.beam_begin(2),
            "beam_step": e.beam_step,
            "beam_fetch": lambda: e.beam_fetch(MAX_NEW),
            "score": lambda: e.score(self.prompts, TARGETS),
            "prefill_draft": lambda: e.prefill_draft(self.prompts, DRAFTS),
            "run_resident": lambda: e.run_resident(max_new=4),
            "align": lambda: e.align(self.align_prompts, stride=4),
            "profile_decode_step": e.profile_decode_step,
            "set_logit_bias": lambda: e.set_logit_bias(BIAS),
            "set_sampling": lambda: e.set_sampling(0.7),
            "set_repetition": lambda: e.set_repetition(1.2, 2),
            "upload": lambda: e.upload_pcm(self.same),
            "mel": lambda: e.mel(self.same),
            "transcribe": lambda: e.transcribe_batch(self.two, max_new=4),
            "beam_search": lambda: e.beam_search_batch([self.clip_a], 2, max_new=4),
            "score_batch": lambda: e.score_batch(self.two, TARGETS),
            "transcribe_draft": lambda: e.transcribe_draft_batch(self.two, DRAFTS, max_new=4),
        }[name]
        self.last = (0, "")
        try:
            fn()
        except Q3aError:
            assert self.last[0] != 0, (name, "refused on the Python side")
        return self.last

    def drive(self, steps):
        """Reset, then the calls of a state; a name with a leading '!' must be refused, every other must succeed."""
        e = self.eng
        if not e.aligner_info()["classify_num"]:
            e.set_logit_bias(None)
            e.set_sampling(0.0)
            e.set_repetition(1.0, 0)
        for name in ["upload"] + steps:
            rc, text = self.call(name.lstrip("!"))
            assert (rc != 0) == name.startswith("!"), (steps, name, rc, text)


_ENCODED = ["mel", "encode"]
_PREFILLED = _ENCODED + ["prefill"]
# state -> the calls that lead there from a fresh upload (None: the engine as created, probed before anything else)
ASR_STATES = {
    "created": None,
    "pcm uploaded": [],
    "mel": ["mel"],
    "encoded": _ENCODED,
    "prefilled": _PREFILLED,
    "prefilled + decode_step": _PREFILLED + ["decode_step"],
    "prefilled + beam_begin(2)": _PREFILLED + ["beam_begin"],
    "after score": _ENCODED + ["score"],
    "after prefill_draft": _ENCODED + ["prefill_draft"],
    "prefilled + set_logit_bias": _PREFILLED + ["set_logit_bias"],
    "prefilled + set_sampling(0.7)": _PREFILLED + ["set_sampling"],
    "prefilled + set_repetition(1.2, 2)": _PREFILLED + ["set_repetition"],
    "after transcribe_batch": ["transcribe"],
    "after beam_search_batch": ["beam_search"],
    "after score_batch": ["score_batch"],
    "after transcribe_draft_batch": ["transcribe_draft"],
    "prefilled + refused prefill": _PREFILLED + ["!bad_prefill"],
}
ALIGNER_STATES = {"created": None, "encoded": _ENCODED}


def _rows(engine, drv, states, probes):
    rows = []
    for state, steps in states.items():
        for probe in probes:
            if steps is not None:
                drv.drive(steps)
            rc, text = drv.call(probe)
            rows.append({"engine": engine, "state": state, "probe": probe, "rc": rc, "error": text})
    return rows


def check_covers(rows):
    """An all-success or all-refusal recording must not pass: every state refuses something, every probe succeeds somewhere (`align`
    on the aligner engine; the aligner's own probe list is the ASR engine's cut to what bears on an aligner, refusals by design)."""
    for engine, states in (("asr", ASR_STATES), ("aligner", ALIGNER_STATES)):
        for state in states:
            assert any(r["rc"] != 0 for r in rows if r["engine"] == engine and r["state"] == state), (engine, state)
    for probe in ASR_PROBES:
        assert any(r["rc"] == 0 for r in rows if r["probe"] == probe), probe


def run_matrix(tiny_dir):
    rows = []
    for engine, model_dir, opts, states, probes in (("asr", tiny_dir, {"token_logprobs": True}, ASR_STATES, ASR_PROBES),
                                                    ("aligner", tiny_aligner_dir(), {}, ALIGNER_STATES, ALIGNER_PROBES)):
        drv = _Driver(model_dir, **opts)
        try:
            rows += _rows(engine, drv, states, probes)
        finally:
            drv.eng.close()
    check_covers(rows)
    return rows
