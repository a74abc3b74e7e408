"""Token log-probabilities (q3a_opts.token_logprobs, q3a_fetch_logprobs): the parts that need no GPU -- the option's place in
the three mirrors of q3a_opts (C header, ctypes, Rust), its default, the declaration of the entry point, the result type's
backwards compatibility and the option's route through the engine source."""
import ctypes as C
import os
import re

from qwen3_asr_rs_amd import _lib
from qwen3_asr_rs_amd.engine import TranscribeResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _c_struct_fields(src, name, open_pat):
    body = src[src.index(open_pat):]
    body = body[:body.index("}")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = re.sub(r"//[^\n]*", "", body)
    return body


def _header_opts_offsets():
    """(field, byte offset) of every int32 field of q3a_opts in include/q3asr.h, arrays expanded by their length."""
    body = _c_struct_fields(_read("include", "q3asr.h"), "q3a_opts", "typedef struct q3a_opts {")
    off, out = 0, []
    for m in re.finditer(r"int32_t\s+([a-z_]+)(?:\[(\d+)\])?\s*;", body):
        out.append((m.group(1), off))
        off += 4 * int(m.group(2) or 1)
    return out, off


def _rust_opts_offsets():
    body = _c_struct_fields(_read("integration", "rust", "src", "backend", "hip", "engine.rs"), "q3a_opts", "pub struct q3a_opts {")
    off, out = 0, []
    for m in re.finditer(r"pub\s+([a-z_]+)\s*:\s*(?:i32|\[i32;\s*(\d+)\])\s*,", body):
        out.append((m.group(1), off))
        off += 4 * int(m.group(2) or 1)
    return out, off


def test_opts_field_has_one_offset_in_header_ctypes_and_rust():
    hdr, hdr_size = _header_opts_offsets()
    rust, rust_size = _rust_opts_offsets()
    assert dict(hdr)["token_logprobs"] == 20                      # right after valu_attention, taken from `reserved`
    assert dict(hdr)["token_logprobs"] == _lib.Opts.token_logprobs.offset
    assert dict(rust)["token_logprobs"] == dict(hdr)["token_logprobs"]
    assert hdr == rust and [n for n, _ in hdr] == [f[0] for f in _lib.Opts._fields_]
    assert all(getattr(_lib.Opts, n).offset == o for n, o in hdr)
    # the struct keeps its size: 16 int32 words in every mirror
    assert hdr_size == rust_size == C.sizeof(_lib.Opts) == 64


def test_header_declares_fetch_logprobs():
    hdr = _read("include", "q3asr.h")
    m = re.search(r"int32_t\s+q3a_fetch_logprobs\s*\(\s*q3a_engine\s*\*\s*e\s*,\s*float\s*\*\s*out_lp\s*,\s*int32_t\s+stride\s*,"
                  r"\s*int32_t\s*\*\s*out_lens\s*\)\s*;", hdr)
    assert m, "q3a_fetch_logprobs is not declared with the documented signature"
    assert "q3a_fetch_logprobs" in _lib.SYMBOLS
    assert "fn q3a_fetch_logprobs(" in _read("integration", "rust", "src", "backend", "hip", "engine.rs")


def test_opts_default_leaves_token_logprobs_off(lib):
    o = _lib.Opts()
    C.memset(C.byref(o), 0x5A, C.sizeof(o))  # garbage in: the default must write the field
    lib.q3a_opts_default(C.byref(o))
    assert o.token_logprobs == 0
    assert (o.precise, o.max_new_tokens, o.use_graph, o.debug_taps, o.valu_attention) == (0, 4096, 1, 0, 0)
    assert list(o.reserved) == [0] * 10


def test_fetch_logprobs_is_exported_and_refuses_a_null_engine(lib):
    assert hasattr(lib, "q3a_fetch_logprobs")
    lens = (C.c_int32 * 1)()
    assert lib.q3a_fetch_logprobs(None, None, 0, lens) != 0


def test_transcribe_result_constructs_from_the_four_old_fields():
    r = TranscribeResult("text", "English", "language English<asr_text>text", [1, 2, 3])
    assert r.token_logprobs is None and r.avg_logprob is None
    r2 = TranscribeResult(text="t", language="l", raw_output="r", ids=[7], token_logprobs=[-0.5], avg_logprob=-0.5)
    assert r2.avg_logprob == -0.5


def test_engine_hands_one_argmax_descriptor_to_every_producer():
    """The engine passes the log-sum channel to each producer of argmax partials that run_head can launch, the finalize writes
    out_lp, the option is part of the graph signature, and the pruned one-sequence argmax is refused with it (the full GEMV runs)."""
    src = _read("qwen3_asr_rs_amd", "csrc", "engine.cpp")
    head = src[src.index("  void run_head(int advance) {"):]
    head = head[:head.index("\n  }\n")]
    # ONE descriptor, built once, that carries the sum exactly when token_lp() ...
    decl = re.findall(r"const ArgmaxPartials part\{([^;]*)\};", head)
    assert len(decl) == 1, decl
    assert re.search(r"token_lp\(\)\s*\?\s*part_sum\.as<float>\(\)\s*:\s*nullptr", decl[0]), decl[0]
    assert head.count("ArgmaxPartials") == 1 and "part_sum" not in head.replace(decl[0], "")
    # ... handed to every producer run_head can launch (the GEMV head, whose prune args copy g; the gemm16 epilogue; both
    # argmax_partial launches) and to the finalize, which writes out_lp with it
    assert "g.part = part;" in head and "pa = prune_args(g)" in head and "ep.part = part;" in head
    assert head.count("launch_argmax_partials(") == head.count("launch_argmax_partials(logits.as<float>(), V, S, part, n_part, stream)") == 2
    # (out_lp is part of what a token commits, DecodeStep::commit(), under the same condition as the descriptor's sum)
    assert "f.part = part;" in head and "f.c = commit();" in head
    commit = src[src.index("  StepCommit commit() const {"):]
    assert re.search(r"c\.out_lp = token_lp\(\) \? out_lp\.as<float>\(\) : nullptr;", commit[:commit.index("\n  }\n")])
    sig = src[src.index("std::string make_graph_sig() const"):]
    assert "token_lp()" in sig[:sig.index("return buf;")]
    gemv = _read("qwen3_asr_rs_amd", "csrc", "k_gemv.hip")
    check = gemv[gemv.index("const char* lm_head_prune_check("):]
    assert re.search(r"if \(g\.part\.sum\) return", check[:check.index("\n}\n")])
