// Engine: owns the weight arena, the workspace and the HIP stream of one GPU and sequences the
// kernels of the hot path.  Exposes the C ABI of include/q3asr.h.
//
// Pipeline per batch of B independent utterances (reference: AsrInference::transcribe,
// src/inference.rs:89-200, run B times):
//   pcm -> k_mel -> k_conv1 -> conv2/conv3 (implicit GEMM) -> conv_out GEMM (+pos-emb, valid-token gather)
//       -> encoder layers {LN, QKV GEMM, window attention, out GEMM+res, LN, fc1 GEMM+GELU, fc2 GEMM+res}
//       -> ln_post, proj1+GELU, proj2 -> audio embeds -> scattered into the prompt embeddings
//       -> decoder prefill layers {RMSNorm, QKV GEMM, qk-norm+RoPE+KV append, causal GQA attention,
//          o GEMM+res, RMSNorm, gate/up GEMM+SiLU*up, down GEMM+res} -> last-row lm_head -> argmax
//       -> decode steps (GEMV path for 1-2 sequences, skinny MFMA GEMM for 3-32, tiled GEMM above), replayed
//          from a hipGraph.
// Residual streams / projections fp32 in HBM, GEMM-input activations bf16 in the default mode (fp32 in precise mode);
// weights bf16; KV cache bf16 (fp32 in precise mode).
#include <hip/hip_runtime.h>

#include <sched.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <thread>

#include "engine_internal.h"

using namespace q3a;

namespace {

thread_local std::string g_last_error;

// Decode-step projections: fp32-x GEMV kernels up to this many sequences, the skinny MFMA GEMM above.  Measured
// (0.6B, 100 tokens): 2 sequences 96.6 ms on the GEMV path; 4 sequences 141 ms on it against 111 ms for FIVE
// sequences on the skinny path.
constexpr int kGemvMaxSeq = 2;

template <typename T>
void upload(DevBuf& b, const std::vector<T>& v, hipStream_t s) {
  b.ensure(std::max<size_t>(v.size() * sizeof(T), 16));
  if (!v.empty()) HIPCHK(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
}

struct ProfEvent {
  int kclass;
  double bytes;
  hipEvent_t a, b;
};

// Prompts of B utterances as setup_prompts takes them: (ids concatenated, lens[B]).  build(s, dst) returns the length of utterance
// s's prompt and, when dst is not null, writes it there (the shape of q3a_build_prompt / q3a_build_align_prompt).
template <class Build>
std::pair<std::vector<int32_t>, std::vector<int32_t>> concat_prompts(int B, Build&& build) {
  std::vector<int32_t> ids, lens(B);
  for (int s = 0; s < B; ++s) {
    lens[s] = build(s, nullptr);
    const size_t o = ids.size();
    ids.resize(o + lens[s]);
    build(s, ids.data() + o);
  }
  return {std::move(ids), std::move(lens)};
}

void require_utterance_ptrs(const char* what, const float* const* ptrs, int B) {
  for (int u = 0; u < B; ++u)
    if (!ptrs[u]) fail(std::string(what) + ": null utterance pointer");
}

}  // namespace

// A/B knobs (kernels.h Knobs: defaults and what each one does).  ONE table names them: q3a_debug_set looks its key up here, and
// knobs() reads the environment names exactly once (atomics afterwards: q3a_debug_set writes them while q3a_group_transcribe may
// have one host thread per GPU reading them).  include/q3asr.h documents the keys; tests/test_host.py compares the two.
namespace q3a {
struct KnobEntry { const char* key; const char* env; std::atomic<int> Knobs::*field; };  // env null: no environment name
static const KnobEntry kKnobTable[] = {
    {"gemm256_min_tiles", "Q3A_GEMM256_MIN_TILES", &Knobs::gemm256_min_tiles},
    {"gemm256_persist", "Q3A_GEMM256_PERSIST", &Knobs::gemm256_persist},
    {"gemm256_group_m", "Q3A_GEMM256_GROUP_M", &Knobs::gemm256_group_m},
    {"dattn_batched_min_wgs", "Q3A_DATTN_BATCHED_MIN_WGS", &Knobs::dattn_batched_min_wgs},
    {"decode_group_size", "Q3A_DECODE_GROUP", &Knobs::decode_group_size},
    {"decode_parallel_groups", "Q3A_DECODE_PARALLEL", &Knobs::decode_parallel_groups},
    {"fuse_qkrope", "Q3A_FUSE_QKROPE", &Knobs::fuse_qkrope},
    {"skinny_q", "Q3A_SKINNY_Q", &Knobs::skinny_q},
    {"eos_run_ahead", "Q3A_EOS_RUN_AHEAD", &Knobs::eos_run_ahead},
    {"skinny_glu_hp3", "Q3A_SKINNY_GLU_HP3", &Knobs::skinny_glu_hp3},
    {"lm_head_prune", "Q3A_LM_HEAD_PRUNE", &Knobs::lm_head_prune},
    {"oproj_by_head", "Q3A_OPROJ_BY_HEAD", &Knobs::oproj_by_head},
    {"layer_taps", "Q3A_DEBUG_LAYER_TAPS", &Knobs::layer_taps},
    {"poison_attn_partials", nullptr, &Knobs::poison_attn_partials},
};
Knobs& knobs() {
  static Knobs k;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const KnobEntry& t : kKnobTable)
      if (const char* e = t.env ? getenv(t.env) : nullptr) (k.*t.field).store(atoi(e));
  });
  return k;
}
}  // namespace q3a

namespace q3a {
// The lists of q3a_set_sequence_bias_lists (q3a_set_sequence_bias: one list) as seqbias_apply_kernel (k_repeat.hip) reads
// them (engine_internal.h; kernels.h SeqBiasArgs).  One list gives the words it always gave, plus the directory.
SeqBiasTable seqbias_layout(const char* what_c, const int32_t* ids, const int32_t* lens, const float* bias, int n, int V) {
  if (n < 0) fail(std::string(what_c) + ": bad argument");
  return seqbias_layout_lists(what_c, ids, lens, bias, &n, n > 0 ? 1 : 0, V);
}
SeqBiasTable seqbias_layout_lists(const char* what_c, const int32_t* ids, const int32_t* lens, const float* bias, const int32_t* list_lens, int n_lists, int V) {
  const std::string what = what_c;
  if (n_lists < 0 || (n_lists > 0 && !list_lens)) fail(what + ": bad argument");
  if (n_lists > SEQBIAS_MAX_LISTS) fail(what + ": " + std::to_string(n_lists) + " lists, more than " + std::to_string(SEQBIAS_MAX_LISTS));
  long n_l = 0;
  for (int k = 0; k < n_lists; ++k) {
    if (list_lens[k] < 0) fail(what + ": list " + std::to_string(k) + " has a negative length");
    n_l += list_lens[k];
  }
  if (n_l > 0 && (!ids || !lens || !bias)) fail(what + ": bad argument");
  if (n_l > SEQBIAS_MAX_ENTRIES) fail(what + ": " + std::to_string(n_l) + " entries, more than " + std::to_string(SEQBIAS_MAX_ENTRIES));
  const int n = (int)n_l;
  struct Ent { int off, len, order, list; float bias; };
  std::vector<Ent> ents;
  std::set<std::vector<int32_t>> seen;  // of the list being read: the same sequence in two lists is two entries
  long total = 0;
  int list = 0, list_end = n_lists > 0 ? list_lens[0] : 0;
  for (int i = 0; i < n; ++i) {
    while (i >= list_end) { list_end += list_lens[++list]; seen.clear(); }
    const int L = lens[i];
    if (L < 1) fail(what + ": entry " + std::to_string(i) + " is an empty sequence");
    if (L > SEQBIAS_MAX_LEN) fail(what + ": entry " + std::to_string(i) + " has " + std::to_string(L) + " ids, more than " + std::to_string(SEQBIAS_MAX_LEN));
    if (total + L > SEQBIAS_MAX_IDS) fail(what + ": more than " + std::to_string(SEQBIAS_MAX_IDS) + " ids over all entries");
    for (int k = 0; k < L; ++k) {
      const int id = ids[total + k];
      if (id < 0 || id >= V) fail(what + ": id " + std::to_string(id) + " of entry " + std::to_string(i) + " is outside the vocabulary (" + std::to_string(V) + ")");
    }
    if (!seen.insert(std::vector<int32_t>(ids + total, ids + total + L)).second) fail(what + ": entry " + std::to_string(i) + " repeats the sequence of an earlier entry");
    const float v = bias[i];
    if (std::isnan(v) || v == INFINITY) fail(what + ": the bias of entry " + std::to_string(i) + " is NaN or +inf (finite or -inf only)");
    ents.push_back({(int)total, L, i, list, v});
    total += L;
  }
  // list after list; inside a list stable by target id, the one-token entry of a target (there is at most one) first, the longer ones
  // in the caller's order
  std::stable_sort(ents.begin(), ents.end(), [&](const Ent& a, const Ent& b) {
    if (a.list != b.list) return a.list < b.list;
    const int ta = ids[a.off + a.len - 1], tb = ids[b.off + b.len - 1];
    return ta != tb ? ta < tb : (a.len == 1) > (b.len == 1);
  });
  SeqBiasTable t;
  t.words.assign(SEQBIAS_TABLE_WORDS, 0u);
  t.list_entries.assign((size_t)n_lists, 0);
  t.list_inf_targets.assign((size_t)n_lists, 0);
  uint32_t* const w = t.words.data();
  int pre = 0, last_inf_target = -1, cur_list = -1;
  for (size_t e = 0; e < ents.size(); ++e) {
    const Ent& x = ents[e];
    const int target = ids[x.off + x.len - 1];
    if (x.list != cur_list) {  // (a target's group belongs to one list: a new list starts a new group whatever its first target)
      for (int k = cur_list + 1; k <= x.list; ++k) w[SEQBIAS_OFF_LISTS + k] = (uint32_t)t.groups;
      last_inf_target = -1;
    }
    if (x.list != cur_list || (int)w[SEQBIAS_OFF_TARGET + t.groups - 1] != target) {
      w[SEQBIAS_OFF_TARGET + t.groups] = (uint32_t)target;
      w[SEQBIAS_OFF_BEGIN + t.groups] = (uint32_t)e;
      ++t.groups;
    }
    cur_list = x.list;
    ++t.list_entries[x.list];
    memcpy(&w[SEQBIAS_OFF_BIAS + e], &x.bias, 4);
    w[SEQBIAS_OFF_PRE_OFF + e] = (uint32_t)pre;
    for (int k = 0; k + 1 < x.len; ++k) w[SEQBIAS_OFF_PRE_IDS + pre++] = (uint32_t)ids[x.off + k];
    if (x.bias == -INFINITY && target != last_inf_target) { ++t.list_inf_targets[x.list]; last_inf_target = target; }
  }
  for (int k = cur_list + 1; k <= SEQBIAS_MAX_LISTS; ++k) w[SEQBIAS_OFF_LISTS + k] = (uint32_t)t.groups;  // (lists behind the last entry: empty)
  w[SEQBIAS_OFF_BEGIN + t.groups] = (uint32_t)ents.size();
  w[SEQBIAS_OFF_PRE_OFF + ents.size()] = (uint32_t)pre;
  t.entries = (int)ents.size(); t.ids = (int)total; t.lists = n_lists;
  t.inf_targets = n_lists > 0 ? t.list_inf_targets[0] : 0;
  w[0] = (uint32_t)t.groups; w[1] = (uint32_t)t.entries;
  return t;
}

// q3a_set_row_options' refusals that need no engine (engine_internal.h): every value a uniform setter refuses, with the row's index.
void row_options_check(const char* what_c, const q3a_row_options* rows, int n_rows, int n_lists, int V) {
  const std::string what = what_c;
  if (n_rows < 0 || (n_rows > 0 && !rows)) fail(what + ": bad argument");
  for (int r = 0; r < n_rows; ++r) {
    const q3a_row_options& o = rows[r];
    const std::string row = what + ": row " + std::to_string(r) + ": ";
    if (!(o.temperature >= 0.f) || !std::isfinite(o.temperature)) fail(row + "temperature must be finite and >= 0 (0: this row takes the argmax)");
    if (!(o.min_p >= 0.f && o.min_p <= 1.f)) fail(row + "min_p must lie in [0, 1]");
    if (o.top_k < 0) fail(row + "top_k must be >= 0 (0 turns top-k off)");
    if (!(o.top_p > 0.f && o.top_p <= 1.f)) fail(row + "top_p must lie in (0, 1] (1 turns top-p off)");
    if (!std::isfinite(o.repetition_penalty) || !(o.repetition_penalty > 0.f)) fail(row + "repetition_penalty must be finite and > 0 (1 turns the penalty off)");
    if (o.no_repeat_ngram_size < 0 || o.no_repeat_ngram_size > 32) fail(row + "no_repeat_ngram_size must lie in [0, 32] (0 turns the ban off)");
    if (!(o.repetition_penalty == 1.f && o.no_repeat_ngram_size == 0) && V > REPEAT_MAX_VOCAB)
      fail(row + "the vocabulary (" + std::to_string(V) + ") exceeds the " + std::to_string(REPEAT_MAX_VOCAB) + " ids the kernel's bitmap holds");
    if (o.sequence_list < -1 || o.sequence_list >= n_lists)
      fail(row + "sequence_list " + std::to_string(o.sequence_list) + " is outside [-1, " + std::to_string(n_lists) + ") (q3a_set_sequence_bias_lists sets the lists)");
  }
}
// The table as the device holds it: four regions of [n_rows][4] words in the words of the uniform buffers (DecodeStep::row_opts).
std::vector<uint32_t> row_options_words(const q3a_row_options* rows, int n_rows) {
  std::vector<uint32_t> w((size_t)16 * n_rows, 0u);
  for (int r = 0; r < n_rows; ++r) {
    const q3a_row_options& o = rows[r];
    uint32_t* const sp = &w[(size_t)(0 * n_rows + r) * 4];
    uint32_t* const fl = &w[(size_t)(1 * n_rows + r) * 4];
    uint32_t* const rp = &w[(size_t)(2 * n_rows + r) * 4];
    memcpy(&sp[0], &o.temperature, 4); memcpy(&sp[1], &o.min_p, 4);
    sp[2] = (uint32_t)o.seed; sp[3] = (uint32_t)(o.seed >> 32);
    fl[0] = (uint32_t)o.top_k; memcpy(&fl[1], &o.top_p, 4);
    memcpy(&rp[0], &o.repetition_penalty, 4); rp[1] = (uint32_t)o.no_repeat_ngram_size;
    w[(size_t)(3 * n_rows + r) * 4] = (uint32_t)o.sequence_list;
  }
  return w;
}
}  // namespace q3a

namespace {

// Debug taps, device copies by name for q3a_debug_read.  opts.debug_taps: 1 = every tap; 2 = only the small ones a soak run compares
struct Taps {
  std::map<std::string, DevBuf> bufs;  std::map<std::string, size_t> bytes;  // by name: the copy, and the bytes of it that are valid
  DevBuf& reserve(const char* name, size_t n) { DevBuf& t = bufs[name]; t.ensure(n); bytes[name] = n; return t; }
  static bool light(const char* name) { return strcmp(name, "dec_last_hidden") == 0 || strcmp(name, "head_in") == 0; }
  void copy(int level, hipStream_t s, const char* name, const void* ptr, size_t n) {
    if (!level || n == 0 || (level == 2 && !light(name))) return;
    HIPCHK(hipMemcpyAsync(reserve(name, n).p, ptr, n, hipMemcpyDeviceToDevice, s));
  }
};

// All the captured decode step sees of its owner: configuration, streams and the per-batch scalars, every one a read-only
// reference to the owner's own word (so nothing is copied and nothing can go stale), and the rules that follow from them alone.
struct StepView {
  const Dims& d; const ArenaLayout& L; const q3a_opts& opts;
  uint8_t* const& arena; const uint32_t& arena_flags; const hipStream_t& stream;
  const std::vector<hipStream_t>& chain_streams;  // one per sequence group after the first, made by the owner before a step forks
  const std::vector<hipEvent_t>& join_ev; const hipEvent_t& fork_ev; const int& n_cu; int* const& host_prog_dev;  // (pinned progress words, device view)
  std::vector<ProfEvent>* const& prof; Taps& taps;  // prof not null: every launch between a pair of events
  const int8_t* const& lm_q; const float* const& lm_qs; const int& lm_q_cols;  // int8 lm_head copy: set once at init, never moved
  const int &B, &max_ctx, &max_new, &gsize, &live_nsplit_, &live_kps_, &attn_nsplit, &min_P_, &part_stride, &beam_w_;
  const size_t& kv_layer_elems; const bool& head_logits_;
  const int &k_parallel_groups, &k_skinny_q, &k_dattn_batched_min_wgs, &k_skinny_glu_hp3, &k_lm_head_prune, &k_oproj_by_head;  // knobs as latched per batch
  const bool& logit_bias_on_;  // q3a_set_logit_bias: a bias is set (changes only while the engine holds no decode state)
  const bool& sampling_on_;    // q3a_set_sampling: temperature > 0 (likewise)
  const bool& sampling_filter_on_;  // q3a_set_sampling_filter: top_k != 0 or top_p != 1 (likewise; acts only while sampling is on)
  const bool& repetition_on_;  // q3a_set_repetition: a penalty != 1 or an n-gram size > 0 (likewise)
  const bool& sequence_bias_on_;  // q3a_set_sequence_bias: a list with at least one entry (likewise)
  // q3a_set_row_options: a row table is set (likewise).  The four switches above then say "on for ANY row", and the kernels read
  // row s's record from DecodeStep::row_opts instead of the uniform buffers
  const bool& row_table_on_;
  const bool& top_lp_on_;  // q3a_set_top_logprobs: n > 0 (likewise); n itself lives in DecodeStep::top_n, which the kernel reads

  bool precise() const { return opts.precise != 0; }
  bool token_lp() const { return opts.token_logprobs != 0; }
  bool kv_f32() const { return opts.precise != 0; }
  size_t kv_elem() const { return kv_f32() ? 4 : 2; }
  int fast_math() const { return precise() ? 0 : 1; }  // GemvArgs / SkinnyArgs::fast_math, the merge's fast exp
  template <typename T> const T* w(uint64_t off) const { return reinterpret_cast<const T*>(arena + off); }
  const float* wf(uint64_t off) const { return w<float>(off); }
  const uint16_t* wh(uint64_t off) const { return w<uint16_t>(off); }
};

// The captured decode step as one unit: every DevBuf a launch of the step reads or writes, and every function that enqueues
// such a launch or computes its arguments from buffers.  The rest of the engine is reachable through StepView only, so a step
// function cannot name a buffer that the two guards against a stale graph do not cover: the reallocation sweep of setup_prompts
// and the address hash of make_graph_sig both walk each_buf().  Sizing stays with the owner (setup_prompts, beam_begin, ensure_rope).
struct DecodeStep : StepView {
  DevBuf kcache, vcache, x_dec, d_pos, next_tok, out_ids, step_count, done, s_ln, s_qkv, s_ctx, s_act, logits, part_val, part_idx;
  DevBuf part_sum, out_lp;  // opts.token_logprobs: log-sum channel of the argmax partials, [B][max_new] log-probabilities next to out_ids
  DevBuf blk_lo, blk_hi;  // pruned lm_head argmax: per 16-row block bounds (pass 1 -> pass 2)
  DevBuf prune_stats;     // [2] candidate blocks rescored, pass-2 launches (q3a_debug_read "lm_head_prune_stats"; never read by the step)
  DevBuf o_part, x_mid;  // one-sequence chain with o_proj per pair of kv heads: its partial vectors [n_kv / 2][hidden], and the residual after o_proj [hidden] (gate / up writes it, down reads it)
  DevBuf attn_pm, attn_pl, attn_po, nn_x, nn_ss;  // nn_*: pre-normalised residual row for the next skinny GEMM: [32 * hidden] bf16 fragment order, [hidden/16][32] f32
  // rope_cur: [B][128] cos|sin row of each sequence's current position (kept by argmax_finalize for decode attention); the tables: ensure_rope
  DevBuf rope_cur, rope_cos, rope_sin;
  DevBuf n_done, forced_tok;  // n_done: device counter of sequences that have produced their EOS (argmax_finalize)
  DevBuf beam_cand_val, beam_cand_idx, beam_part_max, beam_part_sum, beam_topk_ids, beam_topk_lp, beam_score, beam_finished, beam_parent, beam_token;
  DevBuf beam_feed, beam_hist_parent, beam_hist_token, beam_hist_lp, beam_state, beam_lo;
  DevBuf logit_bias;  // [vocab] fp32, every entry finite or -inf (q3a_set_logit_bias; zeros while off): every head form adds it to its logits
  // q3a_set_sampling: {temperature, min_p, seed low, seed high} as the sampler's kernels read them (a new setting needs no new graph),
  // and the clean (max, sum exp) pair of every 2048-logit chunk of every row [B][sample_chunks(vocab)]
  DevBuf samp_params, samp_max, samp_sum;
  // q3a_set_sampling_filter: {top_k, top_p (fp32 bits), 0, 0} as the threshold stage reads them (a new setting needs no new graph); the
  // stage's first-digit table per row, [B][SAMPLE_BUCKETS] uint64 weights then [B][SAMPLE_BUCKETS] uint32 counts, zero between steps;
  // and what it leaves: [B] fp32 max(tau_k, tau_p), then [B] int32 entries kept by it
  DevBuf samp_filter, samp_hist, samp_sel;
  DevBuf rep_params;  // q3a_set_repetition: {penalty (fp32 bits), n-gram size, 0, 0} as repeat_apply_kernel reads them (a new setting needs no new graph)
  DevBuf seq_bias;  // q3a_set_sequence_bias: the list's tables and counts, SEQBIAS_TABLE_WORDS words whatever the list (a new list needs no new graph); allocated by the first non-empty set
  // q3a_set_row_options: four regions of [B][4] words, one record per row each, as the kernels read the uniform buffers: sampling
  // (samp_params), filter (samp_filter), repetition (rep_params), then {the row's sequence-bias list or -1, 0, 0, 0}.  Allocated by the
  // first table and kept; another table of the same switches needs no new graph
  DevBuf row_opts;
  // q3a_set_top_logprobs: {n, 0, 0, 0} as the kernel reads it (another n > 0 needs no new graph); the scratch of a step, the chunks'
  // candidates [B][sample_chunks(vocab)][TOP_LP_MAX] words and their (max, sum exp) pairs [B][sample_chunks(vocab)]; and the history
  // [B][max_new][TOP_LP_MAX] ids and log-probabilities next to out_ids.  Allocated by the first prefill under n > 0
  DevBuf top_n, top_cand, top_max, top_sum, top_ids, top_lp;
  DevBuf draft_accepted;  // draft verification (k_draft.hip): [2 B] first mismatch k per sequence, then its token -- one small D2H copy per prefill
  // f(buffer) for every DevBuf declared above, in declaration order (s: a DecodeStep, const or not).  The declarations of this
  // struct ARE the guarded set: tests/test_host.py::test_step_buffers_cover_the_captured_step compares this list with them.
  template <class Self, class F> static void each_buf(Self& s, F&& f) {
    for (auto* b : {&s.kcache, &s.vcache, &s.x_dec, &s.d_pos, &s.next_tok, &s.out_ids, &s.step_count, &s.done, &s.s_ln, &s.s_qkv, &s.s_ctx, &s.s_act, &s.logits,
                    &s.part_val, &s.part_idx, &s.part_sum, &s.out_lp, &s.blk_lo, &s.blk_hi, &s.prune_stats, &s.o_part, &s.x_mid, &s.attn_pm, &s.attn_pl, &s.attn_po, &s.nn_x, &s.nn_ss,
                    &s.rope_cur, &s.rope_cos, &s.rope_sin, &s.n_done, &s.forced_tok,
                    &s.beam_cand_val, &s.beam_cand_idx, &s.beam_part_max, &s.beam_part_sum, &s.beam_topk_ids, &s.beam_topk_lp, &s.beam_score, &s.beam_finished,
                    &s.beam_parent, &s.beam_token, &s.beam_feed, &s.beam_hist_parent, &s.beam_hist_token, &s.beam_hist_lp, &s.beam_state, &s.beam_lo,
                    &s.logit_bias, &s.samp_params, &s.samp_max, &s.samp_sum, &s.samp_filter, &s.samp_hist, &s.samp_sel, &s.rep_params, &s.seq_bias, &s.row_opts, &s.top_n, &s.top_cand, &s.top_max, &s.top_sum, &s.top_ids, &s.top_lp, &s.draft_accepted})
      f(*b);
  }

  // region r of row_opts (0 sampling, 1 filter, 2 repetition, 3 list) while a row table is set, else the uniform record; the words
  // between two rows' records go to `stride` (kernels.h row_stride)
  enum { kRowSampling = 0, kRowFilter = 1, kRowRepetition = 2, kRowList = 3, kRowRegions = 4 };
  const uint32_t* row_words(int region, const DevBuf& uniform, int& stride) const {
    stride = row_table_on_ ? 4 : 0;
    if (!row_table_on_) return uniform.as<uint32_t>();
    if (!row_opts.p || row_opts.cap < (size_t)kRowRegions * B * 16) fail("row options: a table without its buffer");
    return row_opts.as<uint32_t>() + (size_t)region * B * 4;
  }

  void tap(const char* name, const void* ptr, size_t bytes) { taps.copy(opts.debug_taps, stream, name, ptr, bytes); }
  // run fn() (which enqueues exactly one kernel class) optionally bracketed by events
  template <class F> void timed(int kclass, double bytes, F&& fn) {
    if (!prof) return fn();
    ProfEvent pe{kclass, bytes, nullptr, nullptr};
    HIPCHK(hipEventCreate(&pe.a));
    HIPCHK(hipEventCreate(&pe.b));
    HIPCHK(hipEventRecord(pe.a, stream));
    fn();
    HIPCHK(hipEventRecord(pe.b, stream));
    prof->push_back(pe);
  }

  void* kc_layer(int l) { return (uint8_t*)kcache.p + (size_t)l * kv_layer_elems * kv_elem(); }
  void* vc_layer(int l) { return (uint8_t*)vcache.p + (size_t)l * kv_layer_elems * kv_elem(); }

  LmHeadPruneArgs prune_args(const GemvArgs& g) {
    LmHeadPruneArgs pa{};
    pa.g = g; pa.Wq = lm_q; pa.qcols = lm_q_cols; pa.qs = lm_qs;
    pa.blk_lo = blk_lo.as<float>(); pa.blk_hi = blk_hi.as<float>(); pa.stats = prune_stats.as<int>();
    pa.logit_bias = g.bias != nullptr;  // (the one bias run_head puts there)
    return pa;
  }

  // the logit bias for whichever head form runs; null: none set, every launch is the one of an engine that never had one
  const float* head_bias() const { return logit_bias_on_ ? logit_bias.as<float>() : nullptr; }

  // final norm + lm_head on x_dec -> logits (+ block argmax partials), then argmax/finalize.  While sampling is on every form
  // stores its logits (as with head_logits_), the sampler (k_sample.hip) replaces the head's partials with its own noisy ones, and
  // finalize runs on those unchanged.  While q3a_set_repetition is on every form stores its logits too, repeat_apply_kernel
  // (k_repeat.hip) rewrites the stored rows in place (l' -> l''), and fresh partials over l'' (or the sampler) replace the head's.
  // q3a_set_sequence_bias is the same arrangement one place earlier: seqbias_apply_kernel (k_repeat.hip) rewrites the stored rows
  // first, repetition control then works on its result, and the fresh partials are computed once, after the last rewriting kernel.
  // With a logit bias every form below
  // works on l' = l + b: the GEMV heads and both passes of the pruned argmax through GemvArgs::bias, the gemm16 forms through
  // GemmEpilogue::bias (in front of the argmax epilogue and of the stored logits), the precise batched form through batched_proj.
  void run_head(int advance) {
    const int S = B, H = d.hidden, V = d.vocab;
    const float* const hb = head_bias();
    const bool sample = sampling_on_, repeat = repetition_on_, seqb = sequence_bias_on_, rewrite = repeat || seqb, store = head_logits_ || sample || rewrite || top_lp_on_;
    tap("head_in", x_dec.p, (size_t)S * H * 4);  // (debug taps) last-layer residual rows the final norm + lm_head read
    const double wbytes = 2.0 * V * H;
    int n_part = 0;
    // the argmax partials every producer below writes and argmax_finalize merges; with token log-probabilities also their log-sum
    // channel (null: off, the kernels without it)
    const ArgmaxPartials part{part_val.as<float>(), part_idx.as<int>(), token_lp() ? part_sum.as<float>() : nullptr, part_stride};
    if (S <= kGemvMaxSeq) {
      GemvArgs g{};
      g.fast_math = fast_math();
      g.x = x_dec.as<float>(); g.ldx = H; g.rms_w = wf(L.final_norm); g.eps = d.rms_eps;
      g.W = wh(L.lm_head); g.N = V; g.K = H; g.mode = 3; g.out = logits.as<float>(); g.ldo = V;
      g.part = part; g.bias = hb;
      // (with the log-sum channel lm_head_prune_check refuses: the pruned argmax never computes most logits, the full GEMV runs)
      LmHeadPruneArgs pa{};
      const bool prunable = S == 1 && !precise() && lm_q_cols > 0 && (pa = prune_args(g), !lm_head_prune_check(pa));
      if (prunable && opts.debug_taps == 1) {  // (debug taps) approximate logits and their bounds next to the stored logits
        // a debug buffer outside each_buf(): reached only with debug_taps == 1, and V * 8 bytes whatever the batch, so it is
        // allocated once per engine and no captured launch can outlive its address
        DevBuf& t = taps.reserve("lm_head_bound", (size_t)V * 8);
        LmHeadPruneArgs pd = pa;
        pd.dbg = t.as<float>(); pd.stats = nullptr;
        KCHK(launch_lm_head_approx(pd, stream));
      }
      if (prunable && k_lm_head_prune && !store) {
        // nobody reads the logits: the exact argmax from the int8 pre-pass + a bf16 rescore of the candidate blocks
        g.out = nullptr; pa.g.out = nullptr;
        n_part = lm_head_rescore_groups(g, n_cu);
        timed(Q3A_KC_GEMV_LM_HEAD, (double)V * lm_q_cols, [&] { KCHK(launch_lm_head_approx(pa, stream)); });
        timed(Q3A_KC_ARGMAX, 0, [&] { KCHK(launch_lm_head_rescore(pa, n_part, stream)); });
      } else {
        n_part = gemv_blocks(g);
        timed(Q3A_KC_GEMV_LM_HEAD, wbytes, [&] { KCHK(launch_gemv(g, S, stream)); });
      }
    } else if (!precise()) {
      // default mode: bf16 normed rows, then the LDS-DMA GEMM at M = S (32-row tiles) -- the vocabulary matrix is
      // streamed once through double-buffered LDS; the skinny kernel re-reads x per 16 vocabulary rows (3x slower here)
      timed(Q3A_KC_NORM, 0, [&] { KCHK(launch_rmsnorm(x_dec.as<float>(), wf(L.final_norm), s_ln.as<float>(), S, H, d.rms_eps, stream, s_ln.as<uint16_t>())); });
      GemmEpilogue ep; ep.out = logits.as<float>(); ep.ldo = V; ep.bias = hb;
      if (S <= 32 && V % 4 == 0 && H % 64 == 0 && part_stride >= (V + 63) / 64) {
        // the argmax partials are the GEMM's epilogue (one per 64-column tile and row), and inside q3a_transcribe_batch /
        // q3a_run_resident nobody reads the logits: they are not stored (19 MB per step at 32 sequences)
        ep.part = part;
        if (!store) ep.out = nullptr;
        n_part = (V + 63) / 64;
        timed(Q3A_KC_GEMM, wbytes, [&] { KCHK(launch_gemm16(s_ln.as<uint16_t>(), H, wh(L.lm_head), S, V, H, ep, false, stream)); });
      } else {
        timed(Q3A_KC_GEMM, wbytes, [&] { KCHK(launch_gemm16(s_ln.as<uint16_t>(), H, wh(L.lm_head), S, V, H, ep, false, stream)); });
        n_part = 128;
        if (!rewrite) timed(Q3A_KC_ARGMAX, 0, [&] { KCHK(launch_argmax_partials(logits.as<float>(), V, S, part, n_part, stream)); });
      }
    } else {
      timed(Q3A_KC_NORM, 0, [&] { KCHK(launch_rmsnorm(x_dec.as<float>(), wf(L.final_norm), s_ln.as<float>(), S, H, d.rms_eps, stream)); });
      timed(Q3A_KC_GEMM, wbytes, [&] { batched_proj(s_ln.as<float>(), H, wh(L.lm_head), V, H, hb, 0, logits.as<float>(), V, nullptr); });
      n_part = 128;
      if (!rewrite) timed(Q3A_KC_ARGMAX, 0, [&] { KCHK(launch_argmax_partials(logits.as<float>(), V, S, part, n_part, stream)); });
    }
    if (seqb) n_part = enqueue_sequence_bias(part, !sample && !repeat);
    if (repeat) n_part = enqueue_repetition(part, !sample);
    FinalizeArgs f{};
    f.part = part; f.n_part = n_part; f.V = V; f.advance = advance; f.c = commit();
    if (top_lp_on_) enqueue_top_logprobs(f.c);  // reads l'' only; step_count is still this id's slot, done still last step's
    if (sample) enqueue_sampler(f);
    timed(Q3A_KC_ARGMAX, 0, [&] { KCHK(launch_argmax_finalize(f, S, stream)); });
    if (sample && token_lp()) enqueue_sample_logprob();
  }
  // What a committed token leaves behind (kernels.h StepCommit), in the live buffers: the ONE place that names them for that purpose,
  // whichever launch commits (finalize, draft accept, a fed token).
  StepCommit commit() const {
    StepCommit c{};
    c.next_tok = next_tok.as<int>(); c.out_ids = out_ids.as<int>(); c.out_stride = max_new; c.out_lp = token_lp() ? out_lp.as<float>() : nullptr;
    c.step_count = step_count.as<int>(); c.pos = d_pos.as<int>();
    c.done = done.as<uint8_t>(); c.n_done = n_done.as<int>(); c.n_seq = B; c.host_progress = host_prog_dev;
    c.embed = wh(L.embed); c.H = d.hidden; c.x_next = x_dec.as<float>(); c.eos0 = kEos0; c.eos1 = kEos1;
    c.cos_t = rope_cos.as<float>(); c.sin_t = rope_sin.as<float>(); c.rope_cur = rope_cur.as<float>();
    c.nn = first_layer_norm_out();
    return c;
  }
  // Draft verification (k_draft.hip), in the place of the prefill's run_head(0): from the verify head's argmax per row to the state the
  // greedy loop has after the accepted tokens.  It writes the step's buffers, so it is enqueued here; `a` arrives with the call's own
  // inputs (draft, offsets, prompt lengths, the head's top_id / top_lp: buffers of one prefill that no captured launch ever sees).
  void enqueue_draft_accept(DraftAcceptArgs a) {
    a.n_seq = B; a.accepted = draft_accepted.as<int>(); a.c = commit();
    timed(Q3A_KC_ARGMAX, 0, [&] { KCHK(launch_draft_accept(a, stream)); });
  }
  // teacher forcing and the beam round: tok [B] (device) is what the next step feeds
  void enqueue_set_tokens(const int* tok) { KCHK(launch_set_tokens(tok, B, commit(), stream)); }
  // the same from host ids (q3a_set_next_tokens), through the step's own staging buffer
  void enqueue_forced_tokens(const int32_t* ids) {
    HIPCHK(hipMemcpy(forced_tok.p, ids, (size_t)B * 4, hipMemcpyHostToDevice));
    enqueue_set_tokens(forced_tok.as<int>());
  }
  // fresh argmax partials (log-sum channel included) over rows a kernel has rewritten in place; returns their number per row
  int enqueue_rewritten_partials(const ArgmaxPartials& part) {
    constexpr int kRewrittenParts = 128;
    timed(Q3A_KC_ARGMAX, 0, [&] { KCHK(launch_argmax_partials(logits.as<float>(), d.vocab, B, part, kRewrittenParts, stream)); });
    return kRewrittenParts;
  }
  // Sequence bias (k_repeat.hip): the stored rows, in place, from each sequence's own out_ids and the list's tables in seq_bias.
  // It runs in front of repetition control (HuggingFace's generate() order); `partials`: no rewriting kernel follows and the
  // sampler does not either, so the rewritten rows' own partials take the place of the head's here.
  int enqueue_sequence_bias(const ArgmaxPartials& part, bool partials) {
    SeqBiasArgs sa{};
    sa.logits = logits.as<float>(); sa.S = B; sa.V = d.vocab; seqbias_point(sa, seq_bias.p);
    sa.out_ids = out_ids.as<int>(); sa.out_stride = max_new; sa.step_count = step_count.as<int>();
    if (!seq_bias.p) fail("sequence bias: on without its tables");
    if (row_table_on_) sa.row_list = reinterpret_cast<const int*>(row_words(kRowList, seq_bias, sa.row_stride));  // (else list 0 for every row)
    timed(Q3A_KC_ARGMAX, 0, [&] { KCHK(launch_seqbias_apply(sa, stream)); });
    return partials ? enqueue_rewritten_partials(part) : 0;
  }
  // Repetition penalty and no-repeat n-grams (k_repeat.hip): the stored rows, in place, from each sequence's own out_ids
  // (l' -> l'').  The head's partials, where it wrote any, are those of l': with `partials` the rewritten rows' own, log-sum channel
  // included, take their place (the sampler writes its own instead).  Returns the partials per row finalize then merges.
  int enqueue_repetition(const ArgmaxPartials& part, bool partials) {
    RepeatArgs ra{};
    ra.logits = logits.as<float>(); ra.S = B; ra.V = d.vocab; ra.params = row_words(kRowRepetition, rep_params, ra.row_stride);
    ra.out_ids = out_ids.as<int>(); ra.out_stride = max_new; ra.step_count = step_count.as<int>();
    timed(Q3A_KC_ARGMAX, 0, [&] { KCHK(launch_repeat_apply(ra, stream)); });
    return partials ? enqueue_rewritten_partials(part) : 0;
  }
  // Top log-probabilities (k_toplp.hip): the n best entries of every live row of l'' into slot step_count[s] of the
  // history.  Behind the last rewriting kernel, in front of the finalize, which advances step_count and sets done.
  void enqueue_top_logprobs(const StepCommit& c) {  // c: what the finalize behind this launch commits into
    if (!top_n.p || !top_cand.p || !top_max.p || !top_sum.p || !top_ids.p || !top_lp.p) fail("top log-probabilities: on without its buffers");
    TopLpArgs a{};
    a.logits = logits.as<float>(); a.S = B; a.V = d.vocab; a.n_dev = top_n.as<int>(); a.step_count = c.step_count; a.done = c.done;
    a.cand = top_cand.as<unsigned long long>(); a.chunk_max = top_max.as<float>(); a.chunk_sum = top_sum.as<float>();
    a.out_ids = top_ids.as<int>(); a.out_lp = top_lp.as<float>(); a.out_stride = max_new;
    timed(Q3A_KC_ARGMAX, 0, [&] { KCHK(launch_top_logprobs(a, stream)); });
  }
  // Sampling (k_sample.hip), around the finalize of run_head.  The head's partials are done with: the sampler writes its own noisy
  // ones into the same buffers -- no log-sum channel, the drawn id is not the maximum -- and finalize merges those instead.
  void enqueue_sampler(FinalizeArgs& f) {
    SampleArgs sa{};
    sa.logits = logits.as<float>(); sa.S = B; sa.V = d.vocab; sa.params = row_words(kRowSampling, samp_params, sa.row_stride); sa.step_count = step_count.as<int>();
    sa.chunk_max = samp_max.as<float>(); sa.chunk_sum = samp_sum.as<float>();
    f.part.sum = nullptr; f.c.out_lp = nullptr; f.n_part = sample_chunks(d.vocab);
    sa.part = f.part;
    if (!sampling_filter_on_) { timed(Q3A_KC_ARGMAX, 0, [&] { KCHK(launch_sample(sa, stream)); }); return; }
    // top-k / top-p: the threshold stage between the sampler's two launches
    if ((!row_table_on_ && !samp_filter.p) || !samp_hist.p || !samp_sel.p) fail("sampling filter: on without its buffers");
    SampleFilterArgs sf{};
    sf.filter = row_words(kRowFilter, samp_filter, sf.row_stride); sf.hist_mass = samp_hist.as<unsigned long long>();
    sf.hist_cnt = reinterpret_cast<uint32_t*>(sf.hist_mass + (size_t)B * SAMPLE_BUCKETS);
    sf.tau_sel = samp_sel.as<float>(); sf.kept = samp_sel.as<int>() + B;
    timed(Q3A_KC_ARGMAX, 0, [&] { KCHK(launch_sample_filtered(sa, sf, stream)); });
  }
  // log_softmax(l')[id] of the drawn id, where the greedy step's log-probability would stand
  void enqueue_sample_logprob() {
    SampleLogprobArgs sl{};
    sl.logits = logits.as<float>(); sl.S = B; sl.V = d.vocab; sl.chunk_max = samp_max.as<float>(); sl.chunk_sum = samp_sum.as<float>();
    sl.next_tok = next_tok.as<int>(); sl.step_count = step_count.as<int>(); sl.out_lp = out_lp.as<float>(); sl.out_stride = max_new;
    timed(Q3A_KC_ARGMAX, 0, [&] { KCHK(launch_sample_logprob(sl, stream)); });
  }

  // Skinny decode path in the default mode: every kernel that writes a row of the residual stream (token embedding,
  // o / down projection) also leaves it pre-normalised for the GEMM that reads it next -- bf16(x * w_norm) in MFMA
  // fragment order in nn_x plus partial sums of x^2 in nn_ss (kernels.h NextNormOut / SkinnyArgs::xw16f).
  bool prenorm_path() const { return B > kGemvMaxSeq && !precise(); }
  // o / down projections of the batched decode step as 8-row x 16-sequence workgroups (k_skinny.hip QS; Q3A_SKINNY_Q=0: off)
  bool skinny_q() const {
    auto whole = [](int K) { const int st = K / 32, per = (st + 7) / 8, unr = per <= 2 ? 2 : per <= 4 ? 4 : per <= 8 ? 8 : 12; return K % 256 == 0 && per % unr == 0; };
    return k_skinny_q != 0 && !precise() && d.hidden % 64 == 0 && whole(d.q_dim()) && whole(d.inter);
  }
  int nn_parts() const { return d.hidden / (skinny_q() ? 8 : 16); }  // one partial per 16- (8-) column block of a hidden-wide GEMM output
  // Batched decode (more than kGemvMaxSeq sequences) runs in groups of <= 32 sequences: the skinny MFMA GEMM holds 32
  // sequences per weight sweep, and the second group's sweep of a 4-13 MB matrix is served by the L2 / Infinity Cache.
  int n_groups(int b) const { return b <= kGemvMaxSeq ? 1 : (b + gsize - 1) / gsize; }
  size_t nn_x_stride() const { return (size_t)32 * d.hidden; }         // elements per group
  size_t nn_ss_stride() const { return (size_t)nn_parts() * 32; }
  uint16_t* nn_x_g(int g) const { return nn_x.as<uint16_t>() + (size_t)g * nn_x_stride(); }
  float* nn_ss_g(int g) const { return nn_ss.as<float>() + (size_t)g * nn_ss_stride(); }
  float* s_ctx_g(int g) const { return s_ctx.as<float>() + (size_t)g * 32 * d.q_dim(); }   // fp32 [S][QD] or bf16 fragment order
  float* s_act_g(int g) const { return s_act.as<float>() + (size_t)g * 32 * d.inter; }
  NextNormOut first_layer_norm_out() const {
    NextNormOut nn{};
    if (prenorm_path()) {
      nn.next_w = wf(L.dec[0].in_ln); nn.next_xw16f = nn_x.as<uint16_t>(); nn.next_ss = nn_ss.as<float>(); nn.nparts = nn_parts();
      nn.group_stride_x = (long)nn_x_stride(); nn.group_stride_ss = (long)nn_ss_stride(); nn.group_size = gsize;
    }
    return nn;
  }

  // decode-step projection for more than 4 sequences: skinny MFMA GEMM up to 32, generic tiles above
  void batched_proj(const float* x, int ldx, const uint16_t* W, int N, int K, const float* bias, int mode, float* out,
                    int ldo, const float* resid) {
    const int S = B;  // (precise-mode lm_head only)
    if (S <= 32) {
      SkinnyArgs sk{};
      sk.fast_math = fast_math();
      sk.x = x; sk.ldx = ldx; sk.S = S; sk.W = W; sk.N = N; sk.K = K; sk.bias = bias; sk.mode = mode; sk.out = out; sk.ldo = ldo; sk.resid = resid;
      KCHK(launch_skinny(sk, precise(), stream));
    } else {
      GemmEpilogue ep; ep.out = out; ep.ldo = ldo; ep.bias = bias; ep.resid = (mode == 1) ? resid : nullptr;
      KCHK(launch_gemm(x, ldx, W, S, N, K, ep, mode == 2, precise(), stream));
    }
  }

  // The four projections of a decoder layer, stated ONCE for every path that launches them (decode_layer's GEMV and skinny forms,
  // q3a_profile_weight_stream).  A caller starts its kernel arguments from one with gemv_args / skinny_args and sets only what its
  // path adds: x and out pointers, the norm source, fragment flags, next-norm outputs.
  struct Proj {
    const uint16_t* W;  // [N][K] bf16
    int N, K;
    const float* bias;  // null: the checkpoint has none (arena flags)
    int mode;           // GemvArgs / SkinnyArgs::mode: 0 plain, 1 + residual, 2 SiLU(gate) * up of interleaved rows -> N / 2 columns
    int kclass;         // profile class of its GEMV (the skinny path books every projection as Q3A_KC_GEMM)
    double bytes;       // weight bytes one launch streams
  };
  struct LayerProjs { Proj qkv, o, gu, down; };
  LayerProjs layer_projs(int li) const {
    const DecLayerOff& l = L.dec[li];
    const int H = d.hidden, I = d.inter, QD = d.q_dim(), QKV = d.qkv_dim();
    auto proj = [&](uint64_t w_off, int N, int K, uint32_t bias_flag, uint64_t b_off, int mode, int kclass) {
      return Proj{wh(w_off), N, K, (arena_flags & bias_flag) ? wf(b_off) : nullptr, mode, kclass, 2.0 * N * K};
    };
    return {proj(l.qkv_w, QKV, H, kFlagDecQkvBias, l.qkv_b, 0, Q3A_KC_GEMV), proj(l.o_w, H, QD, kFlagDecOBias, l.o_b, 1, Q3A_KC_GEMV_O),
            proj(l.gu_w, 2 * I, H, kFlagDecMlpBias, l.gu_b, 2, Q3A_KC_GEMV), proj(l.down_w, H, I, kFlagDecMlpBias, l.down_b, 1, Q3A_KC_GEMV_DOWN)};
  }
  template <class Args> Args proj_args(const Proj& p) const {  // the fields GemvArgs and SkinnyArgs share
    Args a{};
    a.fast_math = fast_math(); a.eps = d.rms_eps;  // (eps: read only where a norm source is set)
    a.W = p.W; a.N = p.N; a.K = p.K; a.ldx = p.K; a.bias = p.bias; a.mode = p.mode; a.ldo = p.mode == 2 ? p.N / 2 : p.N;
    return a;
  }
  GemvArgs gemv_args(const Proj& p) const { return proj_args<GemvArgs>(p); }
  SkinnyArgs skinny_args(const Proj& p, int S) const { SkinnyArgs k = proj_args<SkinnyArgs>(p); k.S = S; return k; }

  // one decoder layer of the greedy-loop iteration (inference.rs:172-197) for sequences [s0, s0 + S) -- the whole batch on
  // the GEMV path, one group of <= 32 on the skinny MFMA path
  void decode_layer(int li, int grp, int s0, int S, hipStream_t ks) {
    const int H = d.hidden, QKV = d.qkv_dim();
    const bool gemv = B <= kGemvMaxSeq;
    const DecLayerOff& l = L.dec[li];
    const LayerProjs pj = layer_projs(li);
    float* const x = x_dec.as<float>() + (size_t)s0 * H;
    float* const qkv = s_qkv.as<float>() + (size_t)s0 * QKV;
    const size_t kv_seq = (size_t)d.n_kv * max_ctx * 128 * kv_elem();  // bytes per sequence and layer
    DecodeAttnArgs da{};
    da.qkv = qkv; da.pos = d_pos.as<int>() + s0; da.eps = d.rms_eps;
    da.rope_cur = rope_cur.as<float>() + (size_t)s0 * 128;
    da.pm = attn_pm.as<float>() + (size_t)s0 * d.n_q * attn_nsplit; da.pl = attn_pl.as<float>() + (size_t)s0 * d.n_q * attn_nsplit;
    da.po = attn_po.as<float>() + (size_t)s0 * d.n_q * attn_nsplit * 128; da.nsplit = live_nsplit_;  // (buffers sized for attn_nsplit)
    da.keys_per_split = live_kps_;  // (0 outside the chain with o_proj by column slice: 128)
    da.n_q = d.n_q; da.n_kv = d.n_kv; da.max_ctx = max_ctx; da.scale_div = sqrtf((float)d.head_dim);
    da.q_norm = wf(l.q_norm); da.k_norm = wf(l.k_norm);
    da.kcache = (uint8_t*)kc_layer(li) + (size_t)s0 * kv_seq; da.vcache = (uint8_t*)vc_layer(li) + (size_t)s0 * kv_seq;
    if (gemv) {
      auto run = [&](const Proj& p, const GemvArgs& a) { timed(p.kclass, p.bytes, [&] { KCHK(launch_gemv(a, S, ks)); }); };
      GemvArgs g = gemv_args(pj.qkv);
      g.x = x; g.rms_w = wf(l.in_ln); g.out = qkv;
      run(pj.qkv, g);
      timed(Q3A_KC_DECODE_ATTN, 0, [&] { KCHK(launch_decode_attn(da, S, kv_f32(), ks)); });
      if (live_kps_ > 0) {
        // o_proj per pair of kv heads: n_kv / 2 partial vectors, no residual add; gate / up forms x + their sum for itself and leaves it in x_mid
        // (x_dec is read by every workgroup of that launch: the sum cannot go back there), the down projection adds to x_mid and
        // writes x_dec, where the next layer and the head expect the residual stream
        OprojHeadArgs oh{};
        oh.pm = da.pm; oh.pl = da.pl; oh.po = da.po; oh.nsplit = live_nsplit_;
        oh.W = pj.o.W; oh.N = pj.o.N; oh.K = pj.o.K; oh.bias = pj.o.bias; oh.n_parts = d.n_kv / 2; oh.y_part = o_part.as<float>();
        timed(pj.o.kclass, pj.o.bytes, [&] { KCHK(launch_oproj_head(oh, ks)); });
        GemvArgs u = gemv_args(pj.gu);
        u.x = x; u.rms_w = wf(l.post_ln); u.out = s_act_g(grp);
        u.x_parts = oh.y_part; u.x_nparts = oh.n_parts; u.x_out = x_mid.as<float>();
        run(pj.gu, u);
        GemvArgs dn = gemv_args(pj.down);
        dn.x = s_act_g(grp); dn.out = x; dn.resid = u.x_out;
        run(pj.down, dn);
        return;
      }
      GemvArgs o = gemv_args(pj.o);
      if (std::min(S, 4) * d.n_q * live_nsplit_ <= GEMV_ATTN_MAX_TABLE) {  // merge the key splits inside the o_proj GEMV
        o.attn_pm = da.pm; o.attn_pl = da.pl; o.attn_po = da.po;
        o.attn_nsplit = live_nsplit_; o.attn_heads = d.n_q; o.attn_fast_exp = fast_math();
      } else {  // very long contexts: separate merge launch
        timed(Q3A_KC_DECODE_ATTN, 0, [&] { KCHK(launch_attn_combine(da.pm, da.pl, da.po, live_nsplit_, S, d.n_q, s_ctx_g(grp), ks)); });
        o.x = s_ctx_g(grp);
      }
      o.out = x; o.resid = x;
      run(pj.o, o);
      GemvArgs u = gemv_args(pj.gu);
      u.x = x; u.rms_w = wf(l.post_ln); u.out = s_act_g(grp);
      run(pj.gu, u);
      GemvArgs dn = gemv_args(pj.down);
      dn.x = s_act_g(grp); dn.out = x; dn.resid = x;
      run(pj.down, dn);
      return;
    }
    // skinny MFMA GEMMs: the norms are fused (no norm launches), and in the default mode the two K-heavy projections read
    // bf16 activations written by their producers (attention, SwiGLU epilogue) in fragment order
    const bool b16 = !precise(), pre = prenorm_path();
    uint16_t* const s_ctx16 = b16 ? reinterpret_cast<uint16_t*>(s_ctx_g(grp)) : nullptr;
    uint16_t* const s_act16 = b16 ? reinterpret_cast<uint16_t*>(s_act_g(grp)) : nullptr;
    auto run = [&](const Proj& p, const SkinnyArgs& a) { timed(Q3A_KC_GEMM, p.bytes, [&] { KCHK(launch_skinny(a, precise(), ks)); }); };
    // x of a projection that reads the residual stream: pre-normalised by its producer, or normalised in the GEMM by norm_w
    auto from_residual = [&](SkinnyArgs& a, const float* norm_w) {
      a.x = x;
      if (pre) { a.xw16f = nn_x_g(grp); a.ss_parts = nn_ss_g(grp); a.ss_nparts = nn_parts(); }
      else a.rms_w = norm_w;
    };
    // a projection that writes the residual stream: quarter workgroups where the shape allows, and the row pre-normalised by
    // next_w for the GEMM that reads it next (null: nobody does)
    auto to_residual = [&](SkinnyArgs& a, const float* next_w) {
      a.out = x; a.resid = x;
      a.qsplit = b16 && skinny_q();
      if (pre && next_w) { a.next_w = next_w; a.next_xw16f = nn_x_g(grp); a.next_ss = nn_ss_g(grp); }
    };
    SkinnyArgs q = skinny_args(pj.qkv, S);
    from_residual(q, wf(l.in_ln));
    q.out = qkv;
    run(pj.qkv, q);
    if (S * d.n_kv >= k_dattn_batched_min_wgs) {
      // the group alone fills the chip: one workgroup per (sequence, kv head) walks all keys and writes the context itself
      if (b16) { da.out16 = s_ctx16; da.out_frag = 1; } else da.out = s_ctx_g(grp);
      da.trim_prologue = min_P_ < 2 * 128;  // some sequence is shorter than the kernel's two prologue key tiles
      timed(Q3A_KC_DECODE_ATTN, 0, [&] { KCHK(launch_decode_attn_batched(da, S, kv_f32(), ks)); });
    } else {
      timed(Q3A_KC_DECODE_ATTN, 0, [&] { KCHK(launch_decode_attn(da, S, kv_f32(), ks)); });
      timed(Q3A_KC_DECODE_ATTN, 0, [&] { KCHK(launch_attn_combine(da.pm, da.pl, da.po, live_nsplit_, S, d.n_q, s_ctx_g(grp), ks, s_ctx16, b16)); });
    }
    SkinnyArgs o = skinny_args(pj.o, S);
    o.x = s_ctx_g(grp); o.x16 = s_ctx16; o.x16_frag = b16;
    to_residual(o, wf(l.post_ln));
    run(pj.o, o);
    SkinnyArgs u = skinny_args(pj.gu, S);
    from_residual(u, wf(l.post_ln));
    u.out = s_act_g(grp); u.out16 = s_act16; u.out16_frag = b16;
    u.n_cu = n_cu;
    u.glu_hp3 = k_skinny_glu_hp3;
    run(pj.gu, u);
    SkinnyArgs dn = skinny_args(pj.down, S);
    dn.x = s_act_g(grp); dn.x16 = s_act16; dn.x16_frag = b16;
    // (the last layer feeds the final norm + lm_head, which read x_dec)
    to_residual(dn, li + 1 < d.dec_layers ? wf(L.dec[li + 1].in_ln) : nullptr);
    run(pj.down, dn);
  }

  // one greedy-loop iteration for all sequences (inference.rs:160-200).  Batched path: the groups of `gsize` sequences are
  // independent chains of latency-bound kernels (5 per layer), so every group runs on its own stream -- forked from and
  // joined back into the engine's stream with events, which a hipGraph capture records as parallel branches: one group's
  // KV-streaming attention overlaps another group's weight-streaming GEMMs.  (Profiling runs keep everything on one stream.)
  bool forks() const { return n_groups(B) > 1 && !prof && k_parallel_groups != 0; }  // (the owner makes the group streams first)
  void enqueue_decode_step() {
    const int ng = n_groups(B);
    const bool chains = forks();
    if (chains) HIPCHK(hipEventRecord(fork_ev, stream));
    for (int g = 0; g < ng; ++g) {
      const int s0 = ng == 1 ? 0 : g * gsize;
      const int S = ng == 1 ? B : std::min(gsize, B - s0);
      hipStream_t ks = (chains && g > 0) ? chain_streams[g - 1] : stream;
      if (chains && g > 0) HIPCHK(hipStreamWaitEvent(ks, fork_ev, 0));
      for (int li = 0; li < d.dec_layers; ++li) decode_layer(li, g, s0, S, ks);
      if (chains && g > 0) {
        HIPCHK(hipEventRecord(join_ev[g - 1], ks));
        HIPCHK(hipStreamWaitEvent(stream, join_ev[g - 1], 0));
      }
    }
    run_head(1);
  }

  // does any group of the batch run the key-split attention (GEMV path, or a group too small for the batched kernel)?
  // The one-sequence chain of the default mode with o_proj per pair of kv heads (k_gemv.hip oproj_head_kernel, the XP gate / up form)
  // and the finer key splits it allows: where the shapes are the kernels' -- kv heads of two q heads, at most GEMV_X_PARTS_MAX pairs,
  // a hidden size in the gate / up hand-over form (K <= 1024).  The 1.7B model (hidden 2048) keeps the merging o_proj.
  bool oproj_by_head() const {
    return k_oproj_by_head != 0 && B == 1 && !precise() && d.n_q == 2 * d.n_kv && d.n_kv % 2 == 0 && d.n_kv / 2 <= GEMV_X_PARTS_MAX && d.hidden <= 1024;
  }
  // keys per split for a step whose context is `keys` keys; 0: the chain does not run (contexts beyond dattn_fine_keys_per_split)
  int fine_keys_per_split(int keys) const { return oproj_by_head() ? dattn_fine_keys_per_split(keys) : 0; }
  bool uses_key_splits() const {
    if (B <= kGemvMaxSeq) return true;
    const int ng = n_groups(B);
    const int smallest = ng == 1 ? B : std::min(gsize, B - (ng - 1) * gsize);
    return smallest * d.n_kv < k_dattn_batched_min_wgs;
  }

  void enqueue_step() {
    enqueue_decode_step();
    if (beam_w_ > 0) enqueue_beam_round();
  }
  void enqueue_beam_round() {
    const int W = beam_w_, S = B, U = B / W;
    BeamTopkArgs t{};
    t.logits = logits.as<float>(); t.S = S; t.V = d.vocab; t.W = W;
    t.cand_val = beam_cand_val.as<float>(); t.cand_idx = beam_cand_idx.as<int>();
    t.part_max = beam_part_max.as<float>(); t.part_sum = beam_part_sum.as<float>();
    t.out_ids = beam_topk_ids.as<int>(); t.out_lp = beam_topk_lp.as<float>();
    timed(Q3A_KC_ARGMAX, 0, [&] { KCHK(launch_beam_topk(t, stream)); });
    BeamAdvanceArgs a{};
    a.U = U; a.W = W; a.topk_ids = t.out_ids; a.topk_lp = t.out_lp;
    a.score = beam_score.as<float>(); a.finished = beam_finished.as<uint8_t>();
    a.parent = beam_parent.as<int>(); a.token = beam_token.as<int>(); a.feed = beam_feed.as<int>();
    a.hist_parent = beam_hist_parent.as<int>(); a.hist_token = beam_hist_token.as<int>(); a.hist_lp = beam_hist_lp.as<float>();
    a.hist_cap = max_new; a.state = beam_state.as<int>();
    // rows a copy moves: the generated suffix, first row = the prompt length, last = the row the step just appended (pos was advanced)
    a.pos = d_pos.as<int>(); a.lo = beam_lo.as<int>(); a.hi_bias = -1;
    a.host_progress = host_prog_dev + 2; a.eos0 = kEos0; a.eos1 = kEos1;
    timed(Q3A_KC_ARGMAX, 0, [&] { KCHK(launch_beam_advance(a, stream)); });
    KvReorderArgs r{};
    r.kcache = kcache.p; r.vcache = vcache.p; r.elem_bytes = (int)kv_elem(); r.layers = d.dec_layers; r.S = S; r.n_kv = d.n_kv; r.max_ctx = max_ctx;
    r.parent = a.parent; r.lo = a.lo; r.hi = a.pos; r.hi_bias = -1; r.all_done = a.state + BEAM_ST_ALL_DONE;
    timed(Q3A_KC_OTHER, 0, [&] { KCHK(launch_kv_reorder(r, stream)); });
    timed(Q3A_KC_OTHER, 0, [&] { enqueue_set_tokens(a.feed); });
  }
};

// How far the current batch has come.  Monotone: a stage implies every stage below it, and a call that overwrites what a stage
// stands for rewinds first.  Decoding: the engine holds decode state (KV cache, next token, out_ids of a prefill).
enum class Stage { None, Batch, Mel, Encoded, Decoding };

// What a call requires of the engine and what it leaves behind.  The functions below are the ONLY writers of the four words, for the
// engine and for the extern "C" layer alike (tests/test_host.py), so a new call type states its requirements and its effect in their
// terms and cannot forget half of a rule.  The captured step reads beam_w() and head_logits() through StepView's references.
class CallState {
  Stage stage_ = Stage::None;
  int beam_w_ = 0;           // > 0: a live beam search, slots per utterance (part of the graph signature); only while Decoding
  bool fixed_mode_ = false;  // the ids of the last generating call have a fixed length (no cut at EOS)
  bool head_logits_ = true;  // store the logits of a batched decode step (step API, debug taps); off inside the whole-path calls
 public:
  bool at(Stage s) const { return stage_ >= s; }
  const int& beam_w() const { return beam_w_; }
  bool fixed_mode() const { return fixed_mode_; }
  const bool& head_logits() const { return head_logits_; }
  void advance(Stage s) { if (stage_ < s) stage_ = s; }
  void rewind(Stage s) {  // to at most s; a search does not outlive its decode state
    if (stage_ > s) stage_ = s;
    if (stage_ < Stage::Decoding) end_search();
  }
  void drop_decode_state() { rewind(Stage::Encoded); }  // no decode state until the next prefill
  void require(Stage s, const char* text) const { if (stage_ < s) fail(text); }
  void require(Stage s, const std::string& text) const { require(s, text.c_str()); }
  void begin_search(int W) { beam_w_ = W; }
  void end_search() { beam_w_ = 0; }
  // the mode pair of a call that generates; a single step of the step API keeps the length rule of its prefill
  void begin_call(bool fixed, bool keep_logits) { fixed_mode_ = fixed; head_logits_ = keep_logits; }
  void begin_step_call() { head_logits_ = true; }
};

}  // namespace

struct q3a_engine : CallState {
  Dims d;
  ArenaLayout L;
  q3a_opts opts{};
  int device = 0;
  hipStream_t stream = nullptr;
  uint8_t* arena = nullptr;
  bool own_arena = false;
  uint32_t arena_flags = 0;
  std::string err;

  // constant tables
  DevBuf dft, filt_t, pos_emb;  // (the RoPE tables are the step's: step.rope_cos / rope_sin)
  int rope_positions = 0;

  // ---- batch description (host) ----
  int B = 0;
  std::vector<int64_t> n_samples, pcm_off, mel_off;
  std::vector<int> n_frames, n_chunks, T, tok_off;   // per utterance; tok_off = first encoder token
  int total_chunks = 0, total_T = 0, max_frames = 0;
  std::vector<int> P, seq_off;  // prompt lengths / first row
  int total_P = 0, max_ctx = 0, max_new = 0;
  std::vector<AttnSeg> enc_segs_h;
  int enc_max_seg = 0;

  // ---- device workspace ----
  DevBuf pcm, d_pcm_off, d_n_samples, d_mel_off, d_n_frames, mel, gmax, d_chunk_utt, d_chunk_frame0;
  DevBuf conv1, conv2, conv3, conv3_rowmap, convout_rowmap;
  DevBuf enc_x, enc_ln, enc_qkv, enc_ctx, enc_ffn, enc_segs, audio_embeds;
  DevBuf ids, audio_rowmap, row_seq, row_pos, dec_segs, last_rows;
  DevBuf dec_x, dec_ln, dec_qkv, dec_ctx, dec_act;
  DevBuf lm_q_buf, lm_qs_buf;  // int8 lm_head copy + per-row scale and norms (init_lm_head_q), never reallocated: the step gets ...
  const int8_t* lm_q = nullptr; const float* lm_qs = nullptr;  // ... these plain pointers
  int lm_q_cols = 0;      // 0: no copy
  DevBuf enc_ctx16, dec_ctx16;  // opts.valu_attention in the default mode: bf16 copy of the fp32 attention context
  DevBuf dec_q16;
  int n_cu = 256;
  int* host_prog = nullptr;      // pinned host words written by argmax_finalize (FinalizeArgs::host_progress), polled without a sync
  int* host_prog_dev = nullptr;  // the same words as the device sees them
  DevBuf zero_page;  // 256 B of zeros: padded filter taps of the bf16 implicit-GEMM convolutions read it
  int part_stride = 0, attn_nsplit = 0;
  size_t kv_layer_elems = 0;

  // ---- batched decode: sequence groups and their streams ----
  int gsize = 32;  // sequences per group of the batched decode step (<= 32: one skinny-GEMM weight sweep), fixed per batch
  // knobs that shape the decode step, latched per batch in setup_prompts: producers outside the captured graph (prefill
  // finalize, set_tokens) and the captured step must agree on them, and the graph signature names them
  int k_parallel_groups = 1, k_skinny_q = 1, k_dattn_batched_min_wgs = 128, k_skinny_glu_hp3 = 1, k_lm_head_prune = 1, k_oproj_by_head = 1;
  std::vector<hipStream_t> chain_streams;
  std::vector<hipEvent_t> join_ev;
  hipEvent_t fork_ev = nullptr;

  // ---- graph ----
  // instantiated decode-step graphs by signature (make_graph_sig): a batch shape met before -- or the same batch at a key-split
  // count met before -- replays without a new capture; oldest entry dropped beyond kGraphCacheMax
  static constexpr size_t kGraphCacheMax = 16;
  std::vector<std::pair<std::string, hipGraphExec_t>> graph_cache;
  // Key splits the one-sequence decode attention launches (k_dattn.hip decode_attn_kernel: one workgroup per kv head and
  // 128-key split).  Sized by what the caches HOLD, not by their capacity: pos_hi_ = longest prompt + decode steps enqueued
  // (host-side count, an upper bound of every sequence's position), so a generous max_new_tokens costs no empty splits.
  int pos_hi_ = 0, live_nsplit_ = 0;
  int live_kps_ = 0;  // keys per split of the step being enqueued where the chain with o_proj by column slice runs (32 / 64 / 128), else 0
  int min_P_ = 0;  // shortest prompt of the batch (decides DecodeAttnArgs::trim_prologue; part of the graph signature)

  // ---- input upload of q3a_transcribe_batch[_ptrs] (the window is host PCM -> ids on the host) ----
  // The caller's buffers are pageable: they are copied (several host threads for a batch-sized input) into a pinned
  // mirror of the device layout and shipped piece by piece on a copy stream of its own; the compute stream waits for a
  // piece's event and runs the log-mel kernel of exactly those utterances, so the front end runs under the rest of the
  // upload.  Q3A_UPLOAD_MODE=0 keeps the old form (one pageable hipMemcpyAsync per utterance on the compute stream).
  hipStream_t up_stream = nullptr;
  void* pin_p = nullptr;
  size_t pin_cap = 0;
  std::vector<hipEvent_t> up_ev;
  hipEvent_t up_t0 = nullptr, up_t1 = nullptr;
  q3a_io_timings io{};
  bool geom_valid = false;  // the device tables of set_batch describe n_samples (same lengths again: nothing to rebuild)

  // ---- measurement ----
  q3a_timings timings{};
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  std::vector<ProfEvent>* prof = nullptr;
  Taps taps;

  bool logit_bias_on_ = false;  // q3a_set_logit_bias: step.logit_bias is applied by every head of the generation paths (graph signature)
  int logit_bias_finite_ = 0;   // its finite entries (the vocabulary while off): what a beam width is checked against
  bool sampling_on_ = false;    // q3a_set_sampling: temperature > 0, the step draws its ids (k_sample.hip; graph signature)
  uint32_t samp_words_[4] = {0, 0, 0, 0};  // what step.samp_params holds: temperature and min_p (fp32 bits), seed low / high
  bool sampling_filter_on_ = false;  // q3a_set_sampling_filter: top_k != 0 or top_p != 1 (k_sample.hip; graph signature)
  uint32_t samp_filter_words_[2] = {0, 0x3f800000u};  // what step.samp_filter holds: top_k, top_p (fp32 bits)
  bool logit_bias_eos_open_ = true;  // the logit bias leaves an EOS id finite (true while off): a sequence can always stop
  bool repetition_on_ = false;       // q3a_set_repetition: penalty != 1 or n-gram size > 0 (k_repeat.hip; graph signature)
  float rep_penalty_ = 1.f;          // what step.rep_params holds
  int rep_ngram_ = 0;
  bool logit_bias_allow_list_ = false;  // the logit bias was set with default_bias = -inf (an allow-list)
  bool sequence_bias_on_ = false;       // q3a_set_sequence_bias: a list with at least one entry (k_repeat.hip; graph signature)
  int seq_bias_stats_[4] = {0, 0, 0, 0};  // of the list step.seq_bias holds: on, entries, ids over all entries, distinct targets
  int seq_bias_inf_targets_ = 0;        // distinct targets of its -inf entries (0 while off)
  std::vector<int> seq_list_entries_, seq_list_inf_;  // per list of q3a_set_sequence_bias_lists: entries, distinct -inf targets
  // q3a_set_row_options.  The four switches above are what the step runs under: the uniform setters' own while no table is set
  // (uni_on_, in the order sampling, filter, repetition, sequence bias), "on for any row" while one is.
  bool row_table_on_ = false;           // (graph signature)
  std::vector<q3a_row_options> rows_;   // the table as uploaded (q3a_debug_read "row_options")
  bool uni_on_[4] = {false, false, false, false};
  bool top_lp_on_ = false;              // q3a_set_top_logprobs: n > 0 (k_toplp.hip; graph signature)
  int top_lp_n_ = 0;                    // n as last set: what step.top_n holds while it is allocated
  int top_lp_run_n_ = 0;                // n the decode state was produced under (0: it has no history to fetch)

  // ---- the captured decode step: its buffers and launches, and all it sees of the members above ----
  DecodeStep step{StepView{d, L, opts, arena, arena_flags, stream, chain_streams, join_ev, fork_ev, n_cu, host_prog_dev, prof, taps, lm_q, lm_qs, lm_q_cols,
                           B, max_ctx, max_new, gsize, live_nsplit_, live_kps_, attn_nsplit, min_P_, part_stride, beam_w(), kv_layer_elems, head_logits(),
                           k_parallel_groups, k_skinny_q, k_dattn_batched_min_wgs, k_skinny_glu_hp3, k_lm_head_prune, k_oproj_by_head, logit_bias_on_, sampling_on_, sampling_filter_on_, repetition_on_, sequence_bias_on_, row_table_on_, top_lp_on_}};

  // (the mode rules are stated once, in StepView)
  bool precise() const { return step.precise(); }
  bool token_lp() const { return step.token_lp(); }
  bool kv_f32() const { return step.kv_f32(); }
  size_t kv_elem() const { return step.kv_elem(); }
  // GEMM-input activations (conv maps, norm outputs, attention context, FFN hidden) are stored as bf16 in the default
  // mode -- exactly the values the MFMA consumes -- and as fp32 in the precise mode (hi+lo split inside the GEMM)
  size_t act_elem() const { return precise() ? 4 : 2; }
  // the fp32 VALU attention (precise mode / opts.valu_attention) writes an fp32 context that is rounded afterwards
  bool valu_attn() const { return precise() || opts.valu_attention; }
  const float* wf(uint64_t off) const { return step.wf(off); }
  const uint16_t* wh(uint64_t off) const { return step.wh(off); }

  void tap(const char* name, const void* ptr, size_t bytes) { step.tap(name, ptr, bytes); }
  // tap of an activation buffer that is bf16 in the default mode and fp32 in the precise mode: always read back as fp32
  void tap_act(const char* name, const void* ptr, size_t elems) {
    if (!opts.debug_taps || elems == 0 || opts.debug_taps == 2) return;
    if (precise()) return tap(name, ptr, elems * 4);
    KCHK(launch_from_bf16((const uint16_t*)ptr, taps.reserve(name, elems * 4).as<float>(), elems, stream));
  }

  // GEMM over an activation buffer: LDS-DMA bf16 kernel (k_gemm16.hip) in the default mode, fp32 hi+lo split kernel
  // (k_gemm.hip) in the precise mode
  void act_gemm(const DevBuf& x, int lda, const uint16_t* W, int M, int N, int K, const GemmEpilogue& ep, bool glu) {
    if (precise()) KCHK(launch_gemm(x.as<float>(), lda, W, M, N, K, ep, glu, true, stream));
    else KCHK(launch_gemm16(x.as<uint16_t>(), lda, W, M, N, K, ep, glu, stream));
  }
  void act_conv(const DevBuf& x, int imgs, int H, int Wd, int C, const uint16_t* W, int Cout, const GemmEpilogue& ep) {
    if (precise()) KCHK(launch_conv3x3s2_gemm(x.as<float>(), imgs, H, Wd, C, W, Cout, ep, true, stream));
    else KCHK(launch_conv3x3s2_gemm16(x.as<uint16_t>(), zero_page.as<uint16_t>(), imgs, H, Wd, C, W, Cout, ep, stream));
  }
  // point a GEMM epilogue / producer at an activation buffer in the mode's storage type
  void act_out(GemmEpilogue& ep, const DevBuf& buf) const {
    if (precise()) ep.out = buf.as<float>(); else ep.out16 = buf.as<uint16_t>();
  }
  uint16_t* act16(const DevBuf& buf) const { return precise() ? nullptr : buf.as<uint16_t>(); }

  // milliseconds between two of the stage events: ev[0] mel, ev[1] encoder, ev[2] prefill, ev[3] decode / head, ev[4] end
  float stage_ms(int i, int j) { float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, ev[i], ev[j])); return ms; }

  // =====================================================================================
  void init_common(const std::string& model_dir, int dev, const q3a_opts* o) {
    if (o) opts = *o; else q3a_opts_default(&opts);
    if (opts.max_new_tokens <= 0) opts.max_new_tokens = 4096;
    d = parse_config_file(model_dir + "/config.json");
    validate_dims(d);
    L = plan_arena(d);
    device = dev;
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev == 0)
      fail("no HIP device available: libq3asr_hip has no CPU fallback (hipGetDeviceCount: " + std::string(hipGetErrorString(e)) + ")");
    if (dev < 0 || dev >= n_dev) fail("device index out of range");
    HIPCHK(hipSetDevice(dev));
    KCHK(skinny_init());
    (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (auto& x : ev) HIPCHK(hipEventCreate(&x));
    HIPCHK(hipHostMalloc((void**)&host_prog, 64, hipHostMallocMapped));
    memset(host_prog, 0, 64);
    HIPCHK(hipHostGetDevicePointer((void**)&host_prog_dev, host_prog, 0));
    step.n_done.ensure(64);
    step.prune_stats.ensure(8);
    HIPCHK(hipMemsetAsync(step.prune_stats.p, 0, 8, stream));
    if (!d.aligner()) {  // the logit bias vector: allocated once, zeros while no bias is set
      step.logit_bias.ensure((size_t)d.vocab * 4);
      HIPCHK(hipMemsetAsync(step.logit_bias.p, 0, (size_t)d.vocab * 4, stream));
      logit_bias_finite_ = d.vocab;
      step.samp_params.ensure(16);  // (written by q3a_set_sampling, read only while sampling is on: engine set-up launches nothing for it)
      step.rep_params.ensure(16);   // (likewise: q3a_set_repetition)
    }
  }

  void init_tables() {
    auto dftm = make_dft_matrix(400, 416);
    auto filt = make_mel_filterbank_T(d.n_mels, 400, 16000, 202);
    auto pe = make_sinusoid_rows(d.tokens_per_chunk(), d.enc_d);
    upload(dft, dftm, stream);
    upload(filt_t, filt, stream);
    upload(pos_emb, pe, stream);
    zero_page.ensure(256);
    HIPCHK(hipMemsetAsync(zero_page.p, 0, 256, stream));
    ensure_rope(8192);
    HIPCHK(hipStreamSynchronize(stream));
  }

  void ensure_rope(int n_pos) {
    if (n_pos <= rope_positions) return;
    int n = std::max(n_pos, 8192);
    std::vector<float> c, s;
    make_rope_tables(n, d.head_dim, d.rope_theta, c, s);
    HIPCHK(hipStreamSynchronize(stream));
    upload(step.rope_cos, c, stream);
    upload(step.rope_sin, s, stream);
    HIPCHK(hipStreamSynchronize(stream));
    rope_positions = n;
  }

  // int8 copy of the lm_head for the pruned one-sequence argmax (kernels.h LmHeadPruneArgs), built once from the arena's bf16
  // matrix; not in the precise mode, which never uses it (vocab * 1024 (2048) + vocab * 16 bytes of device memory)
  void init_lm_head_q() {
    const int cols = lm_head_q_cols(d.hidden);
    if (precise() || d.aligner() || cols == 0 || d.hidden % 8 != 0) return;  // (an aligner has no vocabulary lm_head)
    lm_q_buf.ensure((size_t)d.vocab * cols);
    lm_qs_buf.ensure((size_t)d.vocab * 16);
    KCHK(launch_lm_head_quantize(wh(L.lm_head), d.vocab, d.hidden, lm_q_buf.as<int8_t>(), lm_qs_buf.as<float>(), stream));
    HIPCHK(hipStreamSynchronize(stream));
    lm_q = lm_q_buf.as<int8_t>(); lm_qs = lm_qs_buf.as<float>(); lm_q_cols = cols;
  }

  void check_arena_header() {
    ArenaHeader h;
    HIPCHK(hipMemcpy(&h, arena, sizeof(h), hipMemcpyDeviceToHost));
    if (h.magic != kArenaMagic || h.version != kArenaVersion) fail("weight arena: bad magic/version");
    if (h.total_bytes != L.total) fail("weight arena: size does not match config.json");
    arena_flags = h.flags;
  }

  // =====================================================================================
  // batch geometry (host integers; audio_encoder.rs:79-121, 263-279)
  void set_batch(const int64_t* ns, int b) {
    // a failure below must not leave the previous batch's device tables paired with new host geometry
    rewind(Stage::None);
    if (b <= 0) { B = 0; fail("batch must be >= 1"); }
    // the same lengths as the batch before (fixed-length serving windows; every repetition of a benchmark): all tables
    // below are functions of the lengths alone and are already on the device
    if (geom_valid && b == B && (int)n_samples.size() == b && std::equal(ns, ns + b, n_samples.begin())) return advance(Stage::Batch);
    geom_valid = false;
    B = 0;
    for (int u = 0; u < b; ++u)
      if (ns[u] < 161) fail("utterance too short: reflection padding needs more than 160 samples (src/mel.rs:63-65)");
    n_samples.assign(ns, ns + b);
    pcm_off.resize(b); mel_off.resize(b); n_frames.resize(b); n_chunks.resize(b); T.resize(b); tok_off.resize(b);
    std::vector<int> chunk_utt, chunk_frame0, convout_map, conv3_map;
    enc_segs_h.clear();
    int64_t po = 0, mo = 0;
    int tok = 0;
    total_chunks = 0; max_frames = 0; enc_max_seg = 0;
    const int cf = d.chunk_frames(), tpc = d.tokens_per_chunk(), cpw = d.chunks_per_window();
    for (int u = 0; u < b; ++u) {
      pcm_off[u] = po;
      po += (ns[u] + 3) & ~int64_t(3);
      int F = (int)((ns[u] + 159) / 160);  // mel.rs:51,83-84
      n_frames[u] = F;
      max_frames = std::max(max_frames, F);
      mel_off[u] = mo;
      mo += (int64_t)F * d.n_mels;
      int nc = (F + cf - 1) / cf;
      n_chunks[u] = nc;
      tok_off[u] = tok;
      std::vector<int> valid(nc);
      for (int c = 0; c < nc; ++c) {
        int frames = std::min(cf, F - c * cf);
        valid[c] = Dims::feat_len(frames);
        chunk_utt.push_back(u);
        chunk_frame0.push_back(c * cf);
        for (int t = 0; t < tpc; ++t) convout_map.push_back(t < valid[c] ? tok + t : -1);
        tok += valid[c];
      }
      T[u] = tok - tok_off[u];
      // attention windows (audio_encoder.rs:172-260): None (= one segment) when nc <= cpw
      int t0 = tok_off[u];
      if (nc <= cpw) {
        enc_segs_h.push_back(AttnSeg{t0, T[u], (int64_t)t0 * 3 * d.enc_d});
        enc_max_seg = std::max(enc_max_seg, T[u]);
      } else {
        for (int c0 = 0; c0 < nc; c0 += cpw) {
          int len = 0;
          for (int c = c0; c < std::min(nc, c0 + cpw); ++c) len += valid[c];
          enc_segs_h.push_back(AttnSeg{t0, len, (int64_t)t0 * 3 * d.enc_d});
          enc_max_seg = std::max(enc_max_seg, len);
          t0 += len;
        }
      }
      total_chunks += nc;
    }
    total_T = tok;
    const int f3 = d.freq3();
    conv3_map.resize((size_t)total_chunks * f3 * tpc);
    for (int c = 0; c < total_chunks; ++c)
      for (int f = 0; f < f3; ++f)
        for (int t = 0; t < tpc; ++t) conv3_map[((size_t)c * f3 + f) * tpc + t] = (c * tpc + t) * f3 + f;
    pcm.ensure((size_t)po * 4);
    upload(d_pcm_off, pcm_off, stream);
    upload(d_n_samples, n_samples, stream);
    upload(d_mel_off, mel_off, stream);
    upload(d_n_frames, n_frames, stream);
    upload(d_chunk_utt, chunk_utt, stream);
    upload(d_chunk_frame0, chunk_frame0, stream);
    upload(convout_rowmap, convout_map, stream);
    upload(conv3_rowmap, conv3_map, stream);
    upload(enc_segs, enc_segs_h, stream);
    mel.ensure((size_t)mo * 4);
    gmax.ensure((size_t)b * 4);
    HIPCHK(hipStreamSynchronize(stream));  // host vectors above go out of scope
    B = b;  // committed only after every table is on the device
    geom_valid = true;
    advance(Stage::Batch);
  }

  void upload_pcm(const float* host, const int64_t* ns, int b) {
    set_batch(ns, b);
    int64_t src = 0;
    for (int u = 0; u < b; ++u) {
      HIPCHK(hipMemcpyAsync(pcm.as<float>() + pcm_off[u], host + src, (size_t)ns[u] * 4, hipMemcpyHostToDevice, stream));
      src += ns[u];
    }
    HIPCHK(hipStreamSynchronize(stream));
  }

  // Host PCM of B utterances (one pointer each, pageable) -> HBM -> log-mel, overlapped (see the members above).  On return the
  // log-mel of the whole batch is ENQUEUED on `stream` (ev[0] / ev[1] recorded around it); nothing has been waited for.
  void upload_ptrs_and_mel(const float* const* ptrs, const int64_t* ns, int b) {
    const auto w0 = std::chrono::steady_clock::now();
    set_batch(ns, b);
    static const int mode = [] { const char* e = getenv("Q3A_UPLOAD_MODE"); return e ? atoi(e) : 1; }();
    static const int thr_env = [] { const char* e = getenv("Q3A_UPLOAD_THREADS"); return e ? atoi(e) : -1; }();
    static const int pieces_env = [] { const char* e = getenv("Q3A_UPLOAD_PIECES"); return e ? atoi(e) : 8; }();
    io = q3a_io_timings{};
    io.mode = mode;
    HIPCHK(hipEventRecord(ev[0], stream));
    const size_t total = (size_t)(pcm_off[b - 1] + ((ns[b - 1] + 3) & ~int64_t(3))) * 4;  // bytes of the device layout
    bool staged = mode != 0;
    if (staged && total > pin_cap) {  // (re)allocate the pinned mirror; a host that refuses to pin it gets the direct copies below
      if (up_stream) HIPCHK(hipStreamSynchronize(up_stream));  // (a call that threw may have left copies in flight that read the old buffer)
      if (pin_p) (void)hipHostFree(pin_p);
      pin_p = nullptr; pin_cap = 0;
      const size_t want = (total + (size_t(1) << 20) - 1) & ~((size_t(1) << 20) - 1);
      if (hipHostMalloc(&pin_p, want, hipHostMallocDefault) == hipSuccess && pin_p) pin_cap = want;
      else { (void)hipGetLastError(); pin_p = nullptr; staged = false; io.mode = 0; }
    }
    if (!staged) {  // round 4's form (A/B knob Q3A_UPLOAD_MODE=0, or no pinned memory to be had)
      for (int u = 0; u < b; ++u)
        HIPCHK(hipMemcpyAsync(pcm.as<float>() + pcm_off[u], ptrs[u], (size_t)ns[u] * 4, hipMemcpyHostToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));
      io.pieces = b;
      run_mel();
      HIPCHK(hipEventRecord(ev[1], stream));
      io.stage_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
      return;
    }
    if (!up_stream) {
      HIPCHK(hipStreamCreateWithFlags(&up_stream, hipStreamNonBlocking));
      HIPCHK(hipEventCreate(&up_t0));
      HIPCHK(hipEventCreate(&up_t1));
    }
    HIPCHK(hipStreamSynchronize(up_stream));  // (a call that threw may have left copies in flight that read the staging buffer)
    // pieces = runs of consecutive utterances of roughly equal bytes
    const int want_pieces = std::max(1, std::min(b, pieces_env));
    std::vector<int> first;  // first utterance of every piece (+ sentinel b)
    {
      const size_t per = (total + want_pieces - 1) / want_pieces;
      size_t acc = 0;
      first.push_back(0);
      for (int u = 0; u < b; ++u) {
        acc += (size_t)ns[u] * 4;
        if (acc >= per && u + 1 < b && (int)first.size() < want_pieces) { first.push_back(u + 1); acc = 0; }
      }
      first.push_back(b);
    }
    const int np = (int)first.size() - 1;
    while ((int)up_ev.size() < np) {
      hipEvent_t e2;
      HIPCHK(hipEventCreateWithFlags(&e2, hipEventDisableTiming));
      up_ev.push_back(e2);
    }
    const int nthr = thr_env >= 0 ? std::min(thr_env, np) : (total >= (size_t(8) << 20) ? std::min(8, np) : 0);
    io.pieces = np;
    io.threads = nthr;
    std::vector<std::atomic<int>> ready(np);
    for (auto& r : ready) r.store(0, std::memory_order_relaxed);
    std::atomic<int> next{0};
    uint8_t* const pin = (uint8_t*)pin_p;
    auto copy_piece = [&](int p) {
      for (int u = first[p]; u < first[p + 1]; ++u) memcpy(pin + (size_t)pcm_off[u] * 4, ptrs[u], (size_t)ns[u] * 4);
      ready[p].store(1, std::memory_order_release);
    };
    struct Joiner {  // an exception on the issuing thread must not unwind past running workers (they reference this frame)
      std::vector<std::thread> th;
      ~Joiner() { for (auto& t : th) if (t.joinable()) t.join(); }
    } workers;
    for (int t = 0; t < nthr; ++t)
      workers.th.emplace_back([&] { for (int p; (p = next.fetch_add(1, std::memory_order_relaxed)) < np;) copy_piece(p); });
    MelBatch mb{pcm.as<float>(), d_pcm_off.as<int64_t>(), d_n_samples.as<int64_t>(), d_mel_off.as<int64_t>(),
                d_n_frames.as<int>(), mel.as<float>(), gmax.as<unsigned>()};
    HIPCHK(hipEventRecord(up_t0, up_stream));
    for (int p = 0; p < np; ++p) {
      if (nthr == 0) copy_piece(p);
      for (unsigned spins = 0; !ready[p].load(std::memory_order_acquire);)
        if (++spins > 256) sched_yield();
      const int u0 = first[p], u1 = first[p + 1];
      const size_t o0 = (size_t)pcm_off[u0] * 4, o1 = (size_t)(pcm_off[u1 - 1] + ns[u1 - 1]) * 4;
      HIPCHK(hipMemcpyAsync((uint8_t*)pcm.p + o0, pin + o0, o1 - o0, hipMemcpyHostToDevice, up_stream));
      HIPCHK(hipEventRecord(up_ev[p], up_stream));
      HIPCHK(hipStreamWaitEvent(stream, up_ev[p], 0));
      MelBatch piece = mb;  // the tables are indexed by utterance: a piece is the same launch on offset tables
      piece.pcm_off += u0; piece.n_samples += u0; piece.mel_off += u0; piece.n_frames += u0; piece.gmax_key += u0;
      int mf = 0;
      for (int u = u0; u < u1; ++u) mf = std::max(mf, n_frames[u]);
      KCHK(launch_mel(piece, u1 - u0, mf, dft.as<float>(), filt_t.as<float>(), stream));
    }
    HIPCHK(hipEventRecord(up_t1, up_stream));
    io.stage_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
    mel_done();
    HIPCHK(hipEventRecord(ev[1], stream));
  }

  // =====================================================================================
  void run_mel() {
    MelBatch mb{pcm.as<float>(), d_pcm_off.as<int64_t>(), d_n_samples.as<int64_t>(), d_mel_off.as<int64_t>(),
                d_n_frames.as<int>(), mel.as<float>(), gmax.as<unsigned>()};
    KCHK(launch_mel(mb, B, max_frames, dft.as<float>(), filt_t.as<float>(), stream));
    mel_done();
  }
  void mel_done() {
    advance(Stage::Mel);
    size_t bytes = 0;
    for (int u = 0; u < B; ++u) bytes += (size_t)n_frames[u] * d.n_mels * 4;
    tap("mel", mel.p, bytes);
  }

  // =====================================================================================
  void run_encoder() {
    require(Stage::Mel, "q3a_encode: no mel (call q3a_mel first)");
    const int C = d.conv_ch, D = d.enc_d, Fn = d.enc_ffn;
    const int H1 = Dims::conv_len(d.n_mels), W1 = Dims::conv_len(d.chunk_frames());
    const int H2 = Dims::conv_len(H1), W2 = Dims::conv_len(W1);
    const int H3 = Dims::conv_len(H2), W3 = Dims::conv_len(W2);
    const bool sp = precise();
    const size_t nch = (size_t)total_chunks;
    const size_t ae = act_elem();
    conv1.ensure(nch * H1 * W1 * C * ae);
    conv2.ensure(nch * H2 * W2 * C * ae);
    conv3.ensure(nch * H3 * W3 * C * ae);
    const size_t Tt = (size_t)total_T;
    // the MFMA attention consumes q/k/v as bf16: the qkv GEMM then stores exactly those values (half the bytes)
    const bool qkv16 = !valu_attn();
    enc_x.ensure(Tt * D * 4); enc_ln.ensure(Tt * D * ae); enc_qkv.ensure(Tt * 3 * D * (qkv16 ? 2 : 4));
    enc_ctx.ensure(Tt * D * (valu_attn() ? 4 : ae));
    if (valu_attn() && !sp) enc_ctx16.ensure(Tt * D * 2);
    enc_ffn.ensure(Tt * Fn * ae); audio_embeds.ensure(Tt * d.enc_out * 4);

    ChunkTable ct{d_chunk_utt.as<int>(), d_chunk_frame0.as<int>()};
    KCHK(launch_conv1(mel.as<float>(), d_mel_off.as<int64_t>(), d_n_frames.as<int>(), ct, total_chunks, d.n_mels,
                      d.chunk_frames(), wf(L.conv1_w), wf(L.conv1_b), C, conv1.as<float>(), stream, act16(conv1)));
    tap_act("conv1", conv1.p, nch * H1 * W1 * C);
    {
      GemmEpilogue ep;
      act_out(ep, conv2); ep.ldo = C; ep.bias = wf(L.conv2_b); ep.act = 1;
      act_conv(conv1, total_chunks, H1, W1, C, wh(L.conv2_w), C, ep);
      tap_act("conv2", conv2.p, nch * H2 * W2 * C);
    }
    {
      GemmEpilogue ep;  // rows land as [chunk][t][f][c]  (audio_encoder.rs:132-133 permute fused away)
      act_out(ep, conv3); ep.ldo = C; ep.bias = wf(L.conv3_b); ep.act = 1; ep.rowmap = conv3_rowmap.as<int>();
      act_conv(conv2, total_chunks, H2, W2, C, wh(L.conv3_w), C, ep);
      tap_act("conv3", conv3.p, nch * H3 * W3 * C);
    }
    {
      GemmEpilogue ep;  // conv_out + positional embedding (restarting per chunk) + valid-token gather
      ep.out = enc_x.as<float>(); ep.ldo = D;
      ep.bias = (arena_flags & kFlagConvOutBias) ? wf(L.conv_out_b) : nullptr;
      ep.rowmap = convout_rowmap.as<int>();
      ep.addend = pos_emb.as<float>(); ep.addend_period = W3;
      act_gemm(conv3, H3 * C, wh(L.conv_out_w), total_chunks * W3, D, H3 * C, ep, false);
      tap("enc_in", enc_x.p, Tt * D * 4);
    }
    AttnArgs at{};
    at.q = enc_qkv.as<float>(); at.q_rs = 3 * D;
    at.k = enc_qkv.as<float>() + D; at.v = enc_qkv.as<float>() + 2 * D; at.kv_hs = 64; at.kv_rs = 3 * D;
    if (qkv16) {
      at.q16 = enc_qkv.as<uint16_t>();
      at.k = enc_qkv.as<uint16_t>() + D; at.v = enc_qkv.as<uint16_t>() + 2 * D;
    }
    at.o = enc_ctx.as<float>(); at.o_rs = D;
    at.o16 = valu_attn() ? nullptr : enc_ctx.as<uint16_t>();
    at.segs = enc_segs.as<AttnSeg>(); at.n_segs = (int)enc_segs_h.size(); at.max_len = enc_max_seg;
    at.n_kv_heads = d.enc_heads; at.scale_div = 8.0f;  // sqrt(64), layers.rs:161
    const DevBuf& ctx_in = (valu_attn() && !sp) ? enc_ctx16 : enc_ctx;  // what the out projection reads
    for (int li = 0; li < d.enc_layers; ++li) {
      const EncLayerOff& e = L.enc[li];
      KCHK(launch_layernorm(enc_x.as<float>(), wf(e.ln1_w), wf(e.ln1_b), enc_ln.as<float>(), total_T, D, 1e-5f, stream, act16(enc_ln)));
      {
        GemmEpilogue ep; ep.ldo = 3 * D; ep.bias = wf(e.qkv_b);
        if (qkv16) ep.out16 = enc_qkv.as<uint16_t>(); else ep.out = enc_qkv.as<float>();
        act_gemm(enc_ln, D, wh(e.qkv_w), total_T, 3 * D, D, ep, false);
      }
      if (valu_attn()) {
        KCHK(launch_attn_enc(at, stream));
        if (!sp) KCHK(launch_to_bf16(enc_ctx.as<float>(), enc_ctx16.as<uint16_t>(), Tt * D, stream));
      } else {
        KCHK(launch_fattn_enc(at, stream));
      }
      {
        GemmEpilogue ep; ep.out = enc_x.as<float>(); ep.ldo = D; ep.bias = wf(e.out_b); ep.resid = enc_x.as<float>();
        act_gemm(ctx_in, D, wh(e.out_w), total_T, D, D, ep, false);
      }
      KCHK(launch_layernorm(enc_x.as<float>(), wf(e.ln2_w), wf(e.ln2_b), enc_ln.as<float>(), total_T, D, 1e-5f, stream, act16(enc_ln)));
      {
        GemmEpilogue ep; act_out(ep, enc_ffn); ep.ldo = Fn; ep.bias = wf(e.fc1_b); ep.act = 1;
        act_gemm(enc_ln, D, wh(e.fc1_w), total_T, Fn, D, ep, false);
      }
      {
        GemmEpilogue ep; ep.out = enc_x.as<float>(); ep.ldo = D; ep.bias = wf(e.fc2_b); ep.resid = enc_x.as<float>();
        act_gemm(enc_ffn, Fn, wh(e.fc2_w), total_T, D, Fn, ep, false);
      }
      if (li == 0) tap("enc_layer0", enc_x.p, Tt * D * 4);
      if (opts.debug_taps == 1 && knobs().layer_taps.load() != 0) {  // (tools/bisect_layers.py)
        char name[32];
        snprintf(name, sizeof(name), "E%02d_x", li);
        tap(name, enc_x.p, Tt * D * 4);
      }
    }
    tap("enc_last", enc_x.p, Tt * D * 4);
    KCHK(launch_layernorm(enc_x.as<float>(), wf(L.ln_post_w), wf(L.ln_post_b), enc_ln.as<float>(), total_T, D, 1e-5f, stream, act16(enc_ln)));
    {
      GemmEpilogue ep; act_out(ep, enc_ffn); ep.ldo = D; ep.bias = wf(L.proj1_b); ep.act = 1;  // enc_ffn doubles as the proj1 output
      act_gemm(enc_ln, D, wh(L.proj1_w), total_T, D, D, ep, false);
    }
    {
      GemmEpilogue ep; ep.out = audio_embeds.as<float>(); ep.ldo = d.enc_out; ep.bias = wf(L.proj2_b);
      act_gemm(enc_ffn, D, wh(L.proj2_w), total_T, d.enc_out, D, ep, false);
    }
    tap("audio_embeds", audio_embeds.p, Tt * d.enc_out * 4);
    HIPCHK(hipGetLastError());
    advance(Stage::Encoded);
  }

  // =====================================================================================
  // prompts: ids concatenated, lens[B]  (inference.rs:104-137)
  // before_encoder: the whole-path entry points build the prompts BEFORE they enqueue anything of the batch -- the tables only
  // depend on T[] (host integers of set_batch), and the stream synchronisation below then meets an idle stream instead of
  // draining the encoder between its last kernel and the prefill's first
  void setup_prompts(const int32_t* ids_h, const int32_t* lens, int b, int max_new_req, bool before_encoder = false) {
    if (!before_encoder) require_encoded("q3a_prefill", b);  // (else b is the batch whose geometry the caller has just set)
    P.assign(lens, lens + b);
    end_search();  // (a beam search begins after the prefill: q3a_beam_begin)
    seq_off.resize(b);
    std::vector<int> rowseq, rowpos, amap((size_t)total_T, -1), last(b);
    int off = 0, maxP = 0;
    for (int s = 0; s < b; ++s) {
      seq_off[s] = off;
      int na = 0;
      for (int i = 0; i < P[s]; ++i) {
        rowseq.push_back(s);
        rowpos.push_back(i);
        int id = ids_h[off + i];
        if (id < 0 || id >= d.vocab) fail("q3a_prefill: token id out of range");
        if (id == kAudioPad) {
          if (na >= T[s]) fail("q3a_prefill: more <|audio_pad|> tokens than encoder tokens");
          amap[(size_t)tok_off[s] + na] = off + i;
          ++na;
        }
      }
      if (na != T[s]) fail("q3a_prefill: number of <|audio_pad|> tokens does not match the encoder output length");
      if (P[s] <= 0) fail("q3a_prefill: empty prompt");
      last[s] = off + P[s] - 1;
      off += P[s];
      maxP = std::max(maxP, P[s]);
    }
    total_P = off;
    max_new = std::min(std::max(max_new_req, 1), opts.max_new_tokens);
    max_ctx = ((maxP + max_new + 1 + 127) / 128) * 128;  // whole 128-key tiles (the batched decode attention reads cache rows tile by tile)
    pos_hi_ = maxP;
    min_P_ = *std::min_element(P.begin(), P.end());
    {  // A/B knob: extra keys per (sequence, kv head) cache row block, so that the streams of the batched decode attention
       // do not all start a power of two apart (512 keys x 256 B = 128 KiB)
      static const int pad = [] { const char* e = getenv("Q3A_CTX_PAD"); return e ? atoi(e) : 0; }();
      if (pad > 0) max_ctx += (pad + 127) / 128 * 128;
    }
    ensure_rope(max_ctx + 1);  // argmax_finalize reads the row of the position AFTER the last one the cache can hold
    std::vector<int> ids_v(ids_h, ids_h + total_P);
    std::vector<AttnSeg> segs(b);
    for (int s = 0; s < b; ++s)
      segs[s] = AttnSeg{seq_off[s], P[s], (int64_t)s * d.n_kv * max_ctx * 128};
    upload(ids, ids_v, stream);
    upload(row_seq, rowseq, stream);
    upload(row_pos, rowpos, stream);
    upload(audio_rowmap, amap, stream);
    upload(last_rows, last, stream);
    upload(dec_segs, segs, stream);
    upload(step.d_pos, P, stream);
    const size_t Pt = (size_t)total_P, H = d.hidden;
    dec_x.ensure(Pt * H * 4); dec_ln.ensure(Pt * H * act_elem()); dec_qkv.ensure(Pt * d.qkv_dim() * 4);
    dec_ctx.ensure(Pt * d.q_dim() * (valu_attn() ? 4 : act_elem())); dec_act.ensure(Pt * d.inter * act_elem());
    if (!valu_attn()) dec_q16.ensure(Pt * d.q_dim() * 2);  // q after QK-norm + RoPE as bf16 for the MFMA prefill attention
    if (valu_attn() && !precise()) dec_ctx16.ensure(Pt * d.q_dim() * 2);
    kv_layer_elems = (size_t)b * d.n_kv * max_ctx * 128;
    step.kcache.ensure(kv_layer_elems * d.dec_layers * kv_elem());
    step.vcache.ensure(kv_layer_elems * d.dec_layers * kv_elem());
    step.rope_cur.ensure((size_t)b * 128 * 4);
    {
      Knobs& kn = knobs();
      const int gs = kn.decode_group_size.load();
      gsize = (gs >= 1 && gs <= 32) ? gs : 32;
      k_parallel_groups = kn.decode_parallel_groups.load(); k_skinny_q = kn.skinny_q.load();
      k_dattn_batched_min_wgs = kn.dattn_batched_min_wgs.load();
      k_skinny_glu_hp3 = kn.skinny_glu_hp3.load();
      k_lm_head_prune = kn.lm_head_prune.load();
      k_oproj_by_head = kn.oproj_by_head.load();
    }
    const size_t ng = (size_t)step.n_groups(b);  // groups of <= gsize sequences of the batched decode step
    step.nn_x.ensure(ng * 32 * H * 2); step.nn_ss.ensure((size_t)ng * (H / 8) * 32 * 4);  // room for the finer (8-column) partial rows whichever shape the knob selects later
    step.x_dec.ensure((size_t)b * H * 4); step.next_tok.ensure((size_t)b * 4); step.forced_tok.ensure((size_t)b * 4); step.draft_accepted.ensure((size_t)b * 8);
    step.out_ids.ensure((size_t)b * max_new * 4); step.step_count.ensure((size_t)b * 4); step.done.ensure((size_t)b);
    // s_ctx / s_act also hold the bf16 fragment-order copies of the skinny GEMM path: always 32 sequences there
    step.s_ln.ensure((size_t)b * H * 4); step.s_qkv.ensure((size_t)b * d.qkv_dim() * 4); step.s_ctx.ensure(ng * 32 * d.q_dim() * 4);
    step.s_act.ensure(ng * 32 * d.inter * 4); step.logits.ensure((size_t)b * d.vocab * 4);
    part_stride = std::max(128, (d.vocab + 3) / 4);  // >= blocks of the lm_head GEMV at 1 row per wave
    step.part_val.ensure((size_t)b * part_stride * 4); step.part_idx.ensure((size_t)b * part_stride * 4);
    if (token_lp()) { step.part_sum.ensure((size_t)b * part_stride * 4); step.out_lp.ensure((size_t)b * max_new * 4); }
    if (sampling_on_) { step.samp_max.ensure((size_t)b * sample_chunks(d.vocab) * 4); step.samp_sum.ensure((size_t)b * sample_chunks(d.vocab) * 4); }
    if (sampling_on_ && sampling_filter_on_) {
      // the threshold stage finds its table zero and leaves it zero.  The b rows are zeroed at every prefill all the same: a buffer
      // that grew holds whatever the allocator gave it (at the old address too), and a step that ended between the histogram and the
      // select would otherwise leave its counts there for the life of the buffer
      step.samp_hist.ensure((size_t)b * SAMPLE_BUCKETS * 12); step.samp_sel.ensure((size_t)b * 8);
      HIPCHK(hipMemsetAsync(step.samp_hist.p, 0, (size_t)b * SAMPLE_BUCKETS * 12, stream));
    }
    if (top_lp_on_) {
      // the scratch is written before it is read, step by step; the history is cleared, so a slot no step wrote reads (0, 0.0)
      const size_t nc = (size_t)sample_chunks(d.vocab), hist = (size_t)b * max_new * TOP_LP_MAX * 4;
      step.top_n.ensure(16);
      step.top_cand.ensure((size_t)b * nc * TOP_LP_MAX * 8); step.top_max.ensure((size_t)b * nc * 4); step.top_sum.ensure((size_t)b * nc * 4);
      step.top_ids.ensure(hist); step.top_lp.ensure(hist);
      const int w[4] = {top_lp_n_, 0, 0, 0};
      HIPCHK(hipMemcpyAsync(step.top_n.p, w, 16, hipMemcpyHostToDevice, stream));  // (drained below, before w goes)
      HIPCHK(hipMemsetAsync(step.top_ids.p, 0, hist, stream));
      HIPCHK(hipMemsetAsync(step.top_lp.p, 0, hist, stream));
    }
    top_lp_run_n_ = top_lp_on_ ? top_lp_n_ : 0;
    {
      const size_t nblk4 = ((size_t)(d.vocab + 15) / 16 + 3) & ~size_t(3);  // lm_head_prune_blocks, rounded up for float4 reads
      step.blk_lo.ensure(nblk4 * 4); step.blk_hi.ensure(nblk4 * 4);
    }
    attn_nsplit = (max_ctx + dattn_keys_per_split(kv_f32()) - 1) / dattn_keys_per_split(kv_f32());
    if (step.oproj_by_head()) {  // the finer splits: up to OPROJ_HEAD_MAX_SPLITS of them, whatever max_ctx
      attn_nsplit = std::max(attn_nsplit, OPROJ_HEAD_MAX_SPLITS);
      step.o_part.ensure((size_t)(d.n_kv / 2) * H * 4); step.x_mid.ensure(H * 4);
    }
    {  // (+8 floats: the merge-first o_proj GEMV reads a head's statistics 16 bytes at a time, up to 7 entries past the last head's)
      const size_t n_stat = (size_t)b * d.n_q * attn_nsplit;
      step.attn_pm.ensure((n_stat + 8) * 4); step.attn_pl.ensure((n_stat + 8) * 4);
      step.attn_po.ensure(n_stat * 128 * 4);
      if (knobs().poison_attn_partials.load() != 0) {  // (tests) NaN wherever no decode attention launch has written yet
        HIPCHK(hipMemsetAsync(step.attn_pm.p, 0xFF, step.attn_pm.cap, stream));
        HIPCHK(hipMemsetAsync(step.attn_pl.p, 0xFF, step.attn_pl.cap, stream));
        HIPCHK(hipMemsetAsync(step.attn_po.p, 0xFF, step.attn_po.cap, stream));
      }
    }
    HIPCHK(hipMemsetAsync(step.step_count.p, 0, (size_t)b * 4, stream));
    HIPCHK(hipMemsetAsync(step.done.p, 0, (size_t)b, stream));
    HIPCHK(hipMemsetAsync(step.n_done.p, 0, 64, stream));
    HIPCHK(hipMemsetAsync(step.out_ids.p, 0, (size_t)b * max_new * 4, stream));
    if (token_lp()) HIPCHK(hipMemsetAsync(step.out_lp.p, 0, (size_t)b * max_new * 4, stream));
    // drain the stream -- and the group streams: a run that threw mid-loop may have left run-ahead steps enqueued whose
    // argmax_finalize would still write the progress words -- BEFORE the words are reset
    HIPCHK(hipStreamSynchronize(stream));
    for (auto cs : chain_streams) HIPCHK(hipStreamSynchronize(cs));
    __atomic_store_n(&host_prog[0], 0, __ATOMIC_RELAXED);
    __atomic_store_n(&host_prog[1], 0, __ATOMIC_RELAXED);
    drain_retired_graphs();
    {  // a step-visible buffer was reallocated: cached graphs may replay launches that point at the freed allocation
      bool any = false;
      DecodeStep::each_buf(step, [&](DevBuf& sb) { any = any || sb.grew; sb.grew = false; });
      if (any) drop_graphs();
    }
  }

  void run_prefill() {
    run_prefill_layers();
    const int H = d.hidden;
    // only the last row of every sequence feeds the lm_head (the reference computes all rows and keeps
    // the last, text_decoder.rs:111-112 + inference.rs:156)
    KCHK(launch_gather_rows(dec_x.as<float>(), last_rows.as<int>(), B, H, step.x_dec.as<float>(), stream));
    tap("dec_last_hidden", step.x_dec.p, (size_t)B * H * 4);
    step.run_head(0);
    tap("logits", step.logits.p, (size_t)B * d.vocab * 4);
    HIPCHK(hipGetLastError());
    advance(Stage::Decoding);
  }

  // embedding, audio rows and every decoder layer of the prompts: dec_x holds the last layer's residual stream afterwards.  The
  // layers overwrite the KV cache, so whatever decode state there was ends HERE, for every caller; run_prefill and the draft
  // prefill advance again once theirs is complete.
  void run_prefill_layers() {
    drop_decode_state();
    const int H = d.hidden, I = d.inter, QD = d.q_dim(), QKV = d.qkv_dim();
    const bool sp = precise();
    KCHK(launch_embed(ids.as<int>(), total_P, wh(L.embed), H, kAudioPad, dec_x.as<float>(), stream));
    // audio injection (inference.rs:114-124): one row scatter instead of T full-tensor slice_scatter copies
    KCHK(launch_scatter_rows(audio_embeds.as<float>(), audio_rowmap.as<int>(), total_T, d.hidden, dec_x.as<float>(), stream));  // dec_x[audio_rowmap[t]] = audio_embeds[t]
    tap("dec_embed", dec_x.p, (size_t)total_P * H * 4);
    AttnArgs at{};
    at.q = dec_qkv.as<float>(); at.q_rs = QKV; at.kv_hs = (int64_t)max_ctx * 128; at.kv_rs = 128;
    at.o = dec_ctx.as<float>(); at.o_rs = QD; at.segs = dec_segs.as<AttnSeg>(); at.n_segs = B;
    at.max_len = *std::max_element(P.begin(), P.end()); at.n_kv_heads = d.n_kv;
    at.scale_div = sqrtf((float)d.head_dim);  // layers.rs:327-328
    at.o16 = valu_attn() ? nullptr : dec_ctx.as<uint16_t>();
    if (!valu_attn()) { at.q16 = dec_q16.as<uint16_t>(); at.q_rs = QD; }  // the rope kernel leaves q as bf16 [rows][QD]
    const DevBuf& ctx_in = (valu_attn() && !sp) ? dec_ctx16 : dec_ctx;  // what the o projection reads
    // a projection over all prompt rows: W, N, K, bias and the GLU form from DecodeStep::layer_projs, the rest of ep from the caller
    auto proj_gemm = [&](const DevBuf& x, const DecodeStep::Proj& p, GemmEpilogue ep) {
      ep.bias = p.bias;
      act_gemm(x, p.K, p.W, total_P, p.N, p.K, ep, p.mode == 2);
    };
    const bool fuse_rope = knobs().fuse_qkrope.load() != 0 && !valu_attn() && !precise() && d.head_dim == 128 && gemm256_eligible(total_P, QKV, H) && H % 64 == 0;
    // (debug_taps + layer_taps: raw copies of every prefill layer's intermediate buffers, for bisecting a run-to-run difference
    // to one launch -- tools/bisect_layers.py -- and for checking one launch against a reference on its own input)
    const bool layer_taps = opts.debug_taps && knobs().layer_taps.load() != 0;
    for (int li = 0; li < d.dec_layers; ++li) {
      const DecLayerOff& l = L.dec[li];
      const DecodeStep::LayerProjs pj = step.layer_projs(li);
      auto ltap = [&](const char* what, const void* ptr, size_t bytes) {
        if (!layer_taps) return;
        char name[32];
        snprintf(name, sizeof(name), "L%02d_%s", li, what);
        tap(name, ptr, bytes);
      };
      KCHK(launch_rmsnorm(dec_x.as<float>(), wf(l.in_ln), dec_ln.as<float>(), total_P, H, d.rms_eps, stream, act16(dec_ln)));
      ltap("ln1", dec_ln.p, (size_t)total_P * H * act_elem());
      RopeKvArgs rk{};
      rk.qkv = dec_qkv.as<float>(); rk.row_seq = row_seq.as<int>(); rk.row_pos = row_pos.as<int>();
      rk.q_norm = wf(l.q_norm); rk.k_norm = wf(l.k_norm); rk.eps = d.rms_eps;
      rk.cos_t = step.rope_cos.as<float>(); rk.sin_t = step.rope_sin.as<float>();
      rk.kcache = step.kc_layer(li); rk.vcache = step.vc_layer(li); rk.n_q = d.n_q; rk.n_kv = d.n_kv; rk.max_ctx = max_ctx;
      rk.q16 = valu_attn() ? nullptr : dec_q16.as<uint16_t>();
      if (fuse_rope) {
        // batch-sized prefill: QK-norm, RoPE and the cache append are the epilogue of the qkv GEMM (k_gemm256.hip)
        KCHK(launch_gemm256_qkrope(dec_ln.as<uint16_t>(), pj.qkv.K, pj.qkv.W, total_P, pj.qkv.K, pj.qkv.bias, rk, stream));
      } else {
        GemmEpilogue ep; ep.out = dec_qkv.as<float>(); ep.ldo = QKV;
        proj_gemm(dec_ln, pj.qkv, ep);
        KCHK(launch_qknorm_rope_kv(rk, total_P, kv_f32(), stream));
      }
      at.k = step.kc_layer(li); at.v = step.vc_layer(li);
      if (fuse_rope) {
        ltap("qkvs", dec_qkv.p, std::min((size_t)1024, (size_t)total_P) * QKV * 4);  // fp32 scratch of the trailing rows (small GEMM -> separate rope kernel)
      }
      if (!valu_attn()) ltap("q", dec_q16.p, (size_t)total_P * QD * 2);  // q after QK-norm + RoPE, bf16 [rows][QD]
      ltap("k", step.kc_layer(li), (size_t)B * d.n_kv * max_ctx * 128 * kv_elem());
      ltap("v", step.vc_layer(li), (size_t)B * d.n_kv * max_ctx * 128 * kv_elem());
      if (valu_attn()) {
        KCHK(launch_attn_prefill(at, d.n_q / d.n_kv, kv_f32(), stream));
        if (!sp) KCHK(launch_to_bf16(dec_ctx.as<float>(), dec_ctx16.as<uint16_t>(), (size_t)total_P * QD, stream));
      } else {
        KCHK(launch_fattn_prefill(at, d.n_q / d.n_kv, stream));
      }
      ltap("attn", ctx_in.p, (size_t)total_P * QD * act_elem());
      {
        GemmEpilogue ep; ep.out = dec_x.as<float>(); ep.ldo = H; ep.resid = dec_x.as<float>();
        proj_gemm(ctx_in, pj.o, ep);
      }
      ltap("o", dec_x.p, (size_t)total_P * H * 4);
      KCHK(launch_rmsnorm(dec_x.as<float>(), wf(l.post_ln), dec_ln.as<float>(), total_P, H, d.rms_eps, stream, act16(dec_ln)));
      ltap("ln2", dec_ln.p, (size_t)total_P * H * act_elem());
      {
        GemmEpilogue ep; act_out(ep, dec_act); ep.ldo = I;
        proj_gemm(dec_ln, pj.gu, ep);
      }
      ltap("act", dec_act.p, (size_t)total_P * I * act_elem());
      {
        GemmEpilogue ep; ep.out = dec_x.as<float>(); ep.ldo = H; ep.resid = dec_x.as<float>();
        proj_gemm(dec_act, pj.down, ep);
      }
      ltap("x", dec_x.p, (size_t)total_P * H * 4);
      if (li == 0) tap("dec_layer0", dec_x.p, (size_t)total_P * H * 4);
    }
  }

  // =====================================================================================
  // forced aligner (Qwen3-ForcedAligner): one prefill of the aligner prompts, then the classifier head at every marker row
  // (k_align.hip); no vocabulary lm_head, no argmax_finalize, no decode state
  void require_asr(const char* what) const {
    if (d.aligner()) fail(std::string(what) + ": this engine holds a forced aligner (classify_num in config.json); use q3a_align*");
  }
  // the pair every call of the step API that prefills begins with (`what`: its name in the texts)
  void require_encoded(const char* what, int b) const {
    require(Stage::Encoded, std::string(what) + ": no encoder output (call q3a_encode first)");
    if (b != B) fail(std::string(what) + ": batch size differs from the encoded batch");
  }
  void require_aligner(const char* what) const {
    if (!d.aligner()) fail(std::string(what) + ": not a forced-aligner checkpoint (config.json has no thinker_config.classify_num)");
  }
  // marker rows of the prompts (ids_h as setup_prompts takes them) and their count per utterance; refuses a short stride
  std::vector<int> align_marker_rows(const int32_t* ids_h, const int32_t* lens, int b, int stride, int32_t* counts) const {
    std::vector<int> rows;
    int off = 0;
    for (int s = 0; s < b; ++s) {
      int n = 0;
      for (int i = 0; i < lens[s]; ++i)
        if (ids_h[off + i] == d.timestamp_token_id) { rows.push_back(off + i); ++n; }
      if (n > stride)
        fail("q3a_align: utterance " + std::to_string(s) + " has " + std::to_string(n) + " timestamp markers, more than stride " + std::to_string(stride));
      counts[s] = n;
      off += lens[s];
    }
    return rows;
  }
  // The skeleton the aligner and the scoring call share: prefill layers, then a head at a list of rows of the last layer's residual
  // stream (uploaded to align_rows), no decode state.  Prompts already set up (setup_prompts).  Events: ev[2] before the prefill
  // (recorded here), ev[3] after the layers, ev[4] after the head; the stream is idle on return.  head_ms null (the draft prefill,
  // whose whole-path call records ev[2] / ev[3] around its rounds): no event is recorded and no timing written.
  template <class Head>
  void run_prefill_then_head(const std::vector<int>& rows, float* head_ms, Head&& enqueue_head) {
    auto mark = [&](int i) { if (head_ms) HIPCHK(hipEventRecord(ev[i], stream)); };
    mark(2);
    run_prefill_layers();
    mark(3);
    if (!rows.empty()) {
      upload(align_rows, rows, stream);
      enqueue_head();
    }
    mark(4);
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipGetLastError());
    if (!head_ms) return;
    timings.prefill_ms = stage_ms(2, 4);
    *head_ms = stage_ms(3, 4);
    timings.decode_ms = 0.f; timings.decode_steps = 0; timings.batch = B; timings.total_audio_tokens = total_T;
    timings.total_prompt_tokens = total_P;
  }
  // every whole-path call (transcription, alignment, scoring): mel and encoder times of the events upload_ptrs_and_mel / the caller
  // recorded, total = ev[0] through ev[4]; the caller adds what its own stages between ev[2] and ev[4] are
  // a call that decodes (greedy, beam): prefill = ev[2] .. ev[3], decode = ev[3] .. ev[4] over `steps` steps
  void decode_timings(int steps) {
    front_and_total_timings();
    timings.prefill_ms = stage_ms(2, 3);
    timings.decode_ms = stage_ms(3, 4);
    timings.decode_steps = steps; timings.batch = B; timings.total_audio_tokens = total_T; timings.total_prompt_tokens = total_P;
  }
  void front_and_total_timings() {
    timings.mel_ms = stage_ms(0, 1);
    timings.encoder_ms = stage_ms(1, 2);
    timings.total_ms = stage_ms(0, 4);
  }
  // What both row heads share (kernels.h RowHeadArgs), workspace sized: the M rows align_rows names of the last prefill's residual
  // stream, the final norm, W = lm_head [N][hidden] (the aligner's classifier sits there); log_sum: partials with that channel;
  // want_logits: the only M x N buffer, and only on request.
  void fill_row_head(RowHeadArgs& a, int M, int N, bool log_sum, bool want_logits) {
    const int H = d.hidden, planes = precise() ? 2 : 1, n_part = align_head_parts(N);
    align_xn.ensure((size_t)planes * align_rows_padded(M) * H * 2);
    align_pval.ensure((size_t)M * n_part * 4); align_pidx.ensure((size_t)M * n_part * 4);
    if (log_sum) score_psum.ensure((size_t)M * n_part * 4);
    if (want_logits) align_logits.ensure((size_t)M * N * 4);
    a.x = dec_x.as<float>(); a.ldx = H; a.rows = align_rows.as<int>(); a.M = M;
    a.norm_w = wf(L.final_norm); a.eps = d.rms_eps; a.W = wh(L.lm_head); a.N = N; a.K = H;
    a.planes = planes; a.xn = align_xn.as<uint16_t>();
    a.part = ArgmaxPartials{align_pval.as<float>(), align_pidx.as<int>(), log_sum ? score_psum.as<float>() : nullptr, n_part};
    a.logits = want_logits ? align_logits.as<float>() : nullptr; a.ldl = (size_t)N;
  }
  // The scoring head over the vocabulary at those rows against `targets` [M] (q3a_score*, draft verification): results in score_out
  // as tgt_logit | lp | top_id | top_lp, M words each.
  ScoreHeadArgs score_head_args(int M, const std::vector<int>& targets, bool want_logits) {
    ScoreHeadArgs a{};
    fill_row_head(a, M, d.vocab, true, want_logits);
    upload(score_tgt, targets, stream);
    score_out.ensure((size_t)M * 4 * 4);
    a.targets = score_tgt.as<int>();
    a.tgt_logit = score_out.as<float>(); a.lp = score_out.as<float>() + M;
    a.top_id = score_out.as<int>() + 2 * (size_t)M; a.top_lp = score_out.as<float>() + 3 * (size_t)M;
    return a;
  }
  // Packed per-position results of a row head (utterance after utterance, n[s] positions each) to the caller's [utterance][stride];
  // out null: not asked for.
  template <class T> void scatter_rows(const T* packed, const int32_t* n, int stride, T* out) const {
    if (!out) return;
    for (int s = 0, k = 0; s < B; ++s)
      for (int i = 0; i < n[s]; ++i) out[(size_t)s * stride + i] = packed[k++];
  }
  // Classes (and logits) to the host, [utterance][stride].
  void run_align(const std::vector<int>& rows, const int32_t* counts, int stride, int32_t* out_classes, float* logits_out) {
    const int M = (int)rows.size(), N = d.classify_num;
    run_prefill_then_head(rows, &align_head_ms, [&] {
      AlignHeadArgs a{};
      fill_row_head(a, M, N, false, logits_out != nullptr);
      align_cls.ensure((size_t)M * 4);
      a.classes = align_cls.as<int>();
      KCHK(launch_align_head(a, stream));
    });
    std::vector<int> cls((size_t)M);
    if (M > 0) HIPCHK(hipMemcpy(cls.data(), align_cls.p, (size_t)M * 4, hipMemcpyDeviceToHost));
    if (M > 0 && logits_out) HIPCHK(hipMemcpy(logits_out, align_logits.p, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    scatter_rows(cls.data(), counts, stride, out_classes);
  }
  DevBuf align_rows, align_xn, align_pval, align_pidx, align_cls, align_logits;
  float align_head_ms = 0.f;  // the head's launches of the last align call (q3a_debug_read "align_head_ms")

  // =====================================================================================
  // scoring a given transcript (q3a_score*): ONE causal prefill over prompt + targets[:-1], then the lm_head at the rows that
  // predict the targets with a reducing epilogue (k_align.hip launch_score_head); no argmax_finalize, no decode state.
  // Ids a caller hands in to be fed behind the prompt -- targets to score, a draft to verify -- as ONE plan of the prefill and its head rows.
  struct GivenPlan {
    std::vector<int32_t> ids, lens;  // what is prefilled: per utterance prompt ++ given ids (all of them, or all but the last)
    std::vector<int> rows, targets;  // per head row: row of the residual stream, and the given id it predicts (a trailing row has none: id 0)
    std::vector<int32_t> n;          // given ids per utterance
  };
  // The two uses differ in this much.  Scoring never feeds the last target (nothing is predicted from it); a draft feeds every id, adds
  // the row that predicts the token after the draft, and may hold no EOS.  The rest is what their refusals name.
  struct GivenPolicy {
    const char* noun;          // "target id 7 out of range" / "draft id 7 out of range"
    const char* cannot_be;     // "cannot be a target" / "cannot be a draft id"
    bool feed_last, trailing_row, refuse_eos;
    const char *count_pre, *count_post, *limit_noun;  // "has 9 targets, more than stride 8" / "has a draft of 9 ids, more than max_new 8"
  };
  static constexpr GivenPolicy kScored{"target", "target", false, false, false, "", " targets", "stride"};
  static constexpr GivenPolicy kDrafted{"draft", "draft id", true, true, true, "a draft of ", " ids", "max_new"};
  // prompt_ids / given_ids concatenated over the batch; refuses what the header lists for the call `what`
  GivenPlan given_plan(const char* what, const GivenPolicy& pol, const int32_t* prompt_ids, const int32_t* prompt_lens, const int32_t* given_ids,
                       const int32_t* given_lens, int b, int limit) const {
    const std::string w(what);
    GivenPlan gp;
    gp.lens.resize(b);
    gp.n.assign(given_lens, given_lens + b);
    size_t po = 0, to = 0;
    for (int s = 0; s < b; ++s) {
      const int p = prompt_lens[s], n = given_lens[s];
      if (p <= 0) fail(w + ": empty prompt");
      if (n < 0 || (n > 0 && !given_ids)) fail(w + ": bad " + pol.noun + " length");
      if (n > limit)
        fail(w + ": utterance " + std::to_string(s) + " has " + pol.count_pre + std::to_string(n) + pol.count_post + ", more than " + pol.limit_noun + " " + std::to_string(limit));
      const int row0 = (int)gp.ids.size() + p - 1, fed = pol.feed_last ? n : std::max(n - 1, 0);
      gp.ids.insert(gp.ids.end(), prompt_ids + po, prompt_ids + po + p);
      for (int i = 0; i < n; ++i) {
        const int32_t y = given_ids[to + i];
        if (y < 0 || y >= d.vocab) fail(w + ": " + pol.noun + " id " + std::to_string(y) + " out of range (vocabulary " + std::to_string(d.vocab) + ")");
        if (y == kAudioPad) fail(w + ": <|audio_pad|> (" + std::to_string(kAudioPad) + ") cannot be a " + pol.cannot_be + ": the engine finds audio rows by this id");
        if (pol.refuse_eos && (y == kEos0 || y == kEos1)) fail(w + ": an EOS id (" + std::to_string(y) + ") cannot be a draft id: a draft ends where its ids end");
        if (i < fed) gp.ids.push_back(y);
        gp.rows.push_back(row0 + i);
        gp.targets.push_back(y);
      }
      if (pol.trailing_row) { gp.rows.push_back(row0 + n); gp.targets.push_back(0); }
      gp.lens[s] = p + fed;
      po += p; to += n;
    }
    return gp;
  }
  // prompts of sp already set up.  Results to the host [utterance][stride]; logits_out (nullable): [rows][vocab].
  void run_score(const GivenPlan& sp, int stride, float* out_lp, int32_t* out_top_ids, float* out_top_lp, float* logits_out) {
    const int M = (int)sp.rows.size(), V = d.vocab;
    run_prefill_then_head(sp.rows, &score_head_ms, [&] { KCHK(launch_score_head(score_head_args(M, sp.targets, logits_out != nullptr), stream)); });
    if (M == 0) return;
    std::vector<float> res((size_t)M * 4);  // tgt_logit | lp | top_id | top_lp
    HIPCHK(hipMemcpy(res.data(), score_out.p, res.size() * 4, hipMemcpyDeviceToHost));
    if (logits_out) HIPCHK(hipMemcpy(logits_out, align_logits.p, (size_t)M * V * 4, hipMemcpyDeviceToHost));
    scatter_rows(res.data() + M, sp.n.data(), stride, out_lp);
    scatter_rows(reinterpret_cast<const int32_t*>(res.data()) + 2 * (size_t)M, sp.n.data(), stride, out_top_ids);
    scatter_rows(res.data() + 3 * (size_t)M, sp.n.data(), stride, out_top_lp);
  }
  DevBuf score_tgt, score_psum, score_out;
  float score_head_ms = 0.f;  // the head's launches of the last score call (q3a_debug_read "score_head_ms")

  // =====================================================================================
  // draft-verified decoding (q3a_prefill_draft / q3a_transcribe_draft_batch_ptrs): ONE causal prefill over
  // prompt ++ draft, the scoring head at the n + 1 rows p - 1 .. p - 1 + n (under the logit bias, if one is set), then
  // DecodeStep::enqueue_draft_accept -- and the engine stands where the greedy loop stands after its first k + 1 tokens.
  // what no draft call runs under (the header's list; the per-id refusals are given_plan's)
  void draft_check(const char* what) const {
    require_asr(what);
    if (sampling_on_) fail(std::string(what) + ": sampling is on (q3a_set_sampling with temperature > 0): a sampled id is not the argmax of its row -- turn it off first");
    if (repetition_on_) fail(std::string(what) + ": repetition control is on (q3a_set_repetition): its choice depends on the history, not on the row alone -- turn it off first");
    if (sequence_bias_on_) fail(std::string(what) + ": a sequence bias is on (q3a_set_sequence_bias): its choice depends on the history, not on the row alone -- turn it off first");
    if (top_lp_on_) fail(std::string(what) + ": top log-probabilities are on (q3a_set_top_logprobs): accepted draft tokens never pass the step's head -- turn them off first");
    if (beam_w() > 0) fail(std::string(what) + ": a beam search owns the decode state (a new q3a_prefill returns to the greedy step)");
  }
  // prompts of dp (a kDrafted plan) already set up (setup_prompts over dp.ids / dp.lens).  acc [2 B]: k per utterance, then its token.
  // logits_out (nullable): the head's rows [sum (n + 1)][vocab].  The stream is idle on return and the engine holds decode state.
  void run_prefill_draft(const GivenPlan& dp, std::vector<int>& acc, float* logits_out) {
    const int M = (int)dp.rows.size(), V = d.vocab;
    // the accept kernel's inputs: draft_off [B + 1] | prompt_len [B] | draft ids (what each utterance feeds behind its prompt)
    std::vector<int> words((size_t)2 * B + 1, 0);
    for (int s = 0, off = 0; s < B; off += dp.lens[s++]) {
      words[s + 1] = words[s] + dp.n[s];
      words[(size_t)B + 1 + s] = dp.lens[s] - dp.n[s];
      words.insert(words.end(), dp.ids.begin() + off + dp.lens[s] - dp.n[s], dp.ids.begin() + off + dp.lens[s]);
    }
    const int* const plen = words.data() + B + 1;  // (the insertions are over)
    run_prefill_then_head(dp.rows, nullptr, [&] {
      upload(draft_in, words, stream);
      ScoreHeadArgs a = score_head_args(M, dp.targets, logits_out != nullptr);
      a.bias = step.head_bias();  // a logit bias composes: the verify head is a head of the generation paths
      KCHK(launch_score_head(a, stream));
      DraftAcceptArgs da{};
      da.draft_off = draft_in.as<int>(); da.prompt_len = da.draft_off + B + 1; da.draft = da.prompt_len + B;
      da.top_id = a.top_id; da.top_lp = a.top_lp;
      step.enqueue_draft_accept(da);
    });
    acc.resize((size_t)2 * B);
    HIPCHK(hipMemcpy(acc.data(), step.draft_accepted.p, acc.size() * 4, hipMemcpyDeviceToHost));
    if (logits_out) HIPCHK(hipMemcpy(logits_out, align_logits.p, (size_t)M * V * 4, hipMemcpyDeviceToHost));
    // the host-side bounds of the decode loop, from what was accepted: pos_hi_ an upper bound of every position (decode_steps derives
    // live_nsplit_ from it), min_P_ a lower bound of the live lengths (trim_prologue; both are in the graph signature)
    pos_hi_ = 0; min_P_ = 0x7fffffff;
    for (int s = 0; s < B; ++s) {
      if (acc[s] < 0 || acc[s] > dp.n[s]) fail("draft accept: the device returned a first mismatch outside the draft");
      pos_hi_ = std::max(pos_hi_, plen[s] + acc[s]);
      min_P_ = std::min(min_P_, plen[s] + acc[s]);
    }
    draft_stats_[0] += 1;
    draft_stats_.push_back(total_P);
    advance(Stage::Decoding);
  }
  DevBuf draft_in;
  std::vector<int32_t> draft_stats_{0};  // of the last draft call: rounds run, then the rows prefilled in each (q3a_debug_read "draft_stats")

  // the captured step, through the unit (which cannot create the streams its groups fork onto)
  void enqueue_step() {
    if (step.forks()) ensure_chain_streams(step.n_groups(B) - 1);
    step.enqueue_step();
  }
  void ensure_chain_streams(int n) {
    while ((int)chain_streams.size() < n) {
      hipStream_t s2;
      hipEvent_t e2;
      HIPCHK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&e2, hipEventDisableTiming));
      chain_streams.push_back(s2);
      join_ev.push_back(e2);
    }
    if (!fork_ev) HIPCHK(hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming));
  }

  std::string make_graph_sig() const {
    // everything the captured step's launches depend on: geometry, latched knobs and the address of EVERY step-visible buffer
    // (FNV-1a over DecodeStep::each_buf: the same walk as the reallocation sweep of setup_prompts)
    uint64_t h = 1469598103934665603ull;
    DecodeStep::each_buf(step, [&](const DevBuf& sb) {
      uint64_t v = (uint64_t)(uintptr_t)sb.p;
      for (int i = 0; i < 8; ++i) { h ^= (v >> (8 * i)) & 0xff; h *= 1099511628211ull; }
    });
    char buf[320];
    // (one field per latched knob, as latched: packing several into one integer let distinct settings collide -- ADVICE r5)
    snprintf(buf, sizeof(buf), "%d.%d.%d.%d.%d.%d.%d.%d.%d.%d.%d.b%d.lb%d.sm%d.sf%d.rp%d.sb%d.rt%d.tl%d/%d.%d/%d/%d/%p/%016llx", B, gsize, k_parallel_groups, k_skinny_q,
             k_dattn_batched_min_wgs, k_skinny_glu_hp3, k_lm_head_prune, k_oproj_by_head, (int)(min_P_ < 256), (int)head_logits(), (int)token_lp(), beam_w(), (int)logit_bias_on_, (int)sampling_on_, (int)(sampling_on_ && sampling_filter_on_), (int)repetition_on_, (int)sequence_bias_on_, (int)row_table_on_, (int)top_lp_on_, live_nsplit_, live_kps_,
             max_ctx, max_new, (const void*)arena, (unsigned long long)h);
    return buf;
  }

  // what fn() enqueues on `stream`, captured and instantiated; a throw inside fn ends the capture and drops the partial graph
  template <class F> hipGraphExec_t capture_graph(F&& fn) {
    hipGraph_t g = nullptr;
    hipGraphExec_t exec = nullptr;
    HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    try {
      fn();
    } catch (...) {
      hipGraph_t tmp = nullptr;
      (void)hipStreamEndCapture(stream, &tmp);
      if (tmp) (void)hipGraphDestroy(tmp);
      throw;
    }
    HIPCHK(hipStreamEndCapture(stream, &g));
    const hipError_t ie = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    HIPCHK(ie);
    return exec;
  }
  hipGraphExec_t graph_for_step() {
    const std::string sig = make_graph_sig();
    for (size_t i = 0; i < graph_cache.size(); ++i)
      if (graph_cache[i].first == sig) {  // LRU: a hit moves the entry to the back, eviction takes the front
        if (i + 1 != graph_cache.size()) std::rotate(graph_cache.begin() + i, graph_cache.begin() + i + 1, graph_cache.end());
        return graph_cache.back().second;
      }
    const hipGraphExec_t exec = capture_graph([&] { enqueue_step(); });
    ++graph_captures_;
    if (graph_cache.size() >= kGraphCacheMax) {
      // the natural-EOS loop does not synchronise between steps, so the evicted exec may still be executing: it is only
      // destroyed after the next stream synchronisation (drain_retired_graphs)
      retired_graphs.push_back(graph_cache.front().second);
      graph_cache.erase(graph_cache.begin());
    }
    graph_cache.emplace_back(sig, exec);
    return exec;
  }
  std::vector<hipGraphExec_t> retired_graphs;
  int32_t graph_captures_ = 0;  // decode-step graphs captured over the engine's life (q3a_debug_read "graph_captures")
  // call only when the stream is known to be idle
  void drain_retired_graphs() {
    for (auto ge : retired_graphs) (void)hipGraphExecDestroy(ge);
    retired_graphs.clear();
  }
  // every cached graph holds raw device addresses: none may outlive a reallocation of ANY step-visible buffer (the signature
  // names only some of them).  Call with the stream idle.
  void drop_graphs() {
    drain_retired_graphs();
    for (auto& ge : graph_cache) (void)hipGraphExecDestroy(ge.second);
    graph_cache.clear();
  }

  void decode_steps(int n) {
    require(Stage::Decoding, "decode: no prefill state");
    if (n <= 0) return;
    const bool eager = !opts.use_graph || prof;
    const int kps = dattn_keys_per_split(kv_f32());
    // (Round 6 measured several steps per graph for the fixed-length mode -- a kernel trace shows 8.4 us between a step's finalize and
    // the next step's first GEMV against ~1.4 us inside a graph -- and un-traced it does not pay: one clip 592 -> 590 / 592 / 599 /
    // 607 / 610 us per step at 2 / 4 / 8 / 16 / 32 steps per graph, 32 clips 1131 -> 1126: the seam is the tracer's.  Code at commit
    // 03b3a8b, profiles/r6_ab_decode_steps_per_graph.txt.)
    for (int i = 0; i < n; ++i) {
      // this step feeds the token at position <= pos_hi_ and attends keys 0 .. pos_hi_
      live_kps_ = step.fine_keys_per_split(pos_hi_ + 1);
      live_nsplit_ = live_kps_ > 0 ? pos_hi_ / live_kps_ + 1
                     : step.uses_key_splits() ? std::min(attn_nsplit, pos_hi_ / kps + 1) : attn_nsplit;
      if (eager) enqueue_step();
      else HIPCHK(hipGraphLaunch(graph_for_step(), stream));
      ++pos_hi_;
    }
    if (eager) HIPCHK(hipGetLastError());
  }

  // what a transcription asks setup_prompts for: the fixed length, else the caller's limit, else the engine's
  int max_new_request(int max_new_req, int fixed_new) const { return fixed_new > 0 ? fixed_new : max_new_req > 0 ? max_new_req : opts.max_new_tokens; }
  // the transcription prompt of every utterance of the batch (q3a_build_prompt over T[] of set_batch)
  std::pair<std::vector<int32_t>, std::vector<int32_t>> asr_prompts(const int32_t* lang_ids, int n_prefix) const {
    return concat_prompts(B, [&](int s, int32_t* dst) {
      int32_t len = 0;
      q3a_build_prompt(T[s], lang_ids, n_prefix, dst, &len);
      return len;
    });
  }

  // The front of every whole-path entry point (`what`: its name in error texts), stated once because its ORDER matters: checks,
  // geometry, then the prompts -- prompts() returns (ids, lens) built from T[] alone -- and with them every table and buffer of the
  // prefill and the decode, so that the drain inside setup_prompts meets an idle stream; only then the batch's first launches
  // (upload + log-mel, encoder).  width > 1 (beam search): a clip is uploaded once per slot, `width` sequences of the batch.
  template <class Prompts>
  void whole_path_front(const char* what, const float* const* pcm16k, const int64_t* ns_in, int n, int width, int max_new_req, Prompts&& prompts) {
    if (!pcm16k || !ns_in || n < 1) fail(std::string(what) + ": bad argument");
    require_utterance_ptrs(what, pcm16k, n);
    HIPCHK(hipSetDevice(device));
    const int b = n * width;
    std::vector<const float*> ptrs((size_t)b);
    std::vector<int64_t> ns((size_t)b);
    for (int s = 0; s < b; ++s) { ptrs[s] = pcm16k[s / width]; ns[s] = ns_in[s / width]; }
    set_batch(ns.data(), b);
    auto&& [ids_v, lens_v] = prompts();
    setup_prompts(ids_v.data(), lens_v.data(), b, max_new_req, true);
    timings = q3a_timings{};
    upload_ptrs_and_mel(ptrs.data(), ns.data(), b);
    run_encoder();
  }

  // front_done: whole_path_front() has enqueued the log-mel and the encoder (ev[0] / ev[1] recorded); else the prompts are set up
  void run_resident(int fixed_new, bool front_done = false) {
    if (!front_done) {
      HIPCHK(hipEventRecord(ev[0], stream));
      run_mel();
      HIPCHK(hipEventRecord(ev[1], stream));
      run_encoder();
    }
    HIPCHK(hipEventRecord(ev[2], stream));
    run_prefill();
    HIPCHK(hipEventRecord(ev[3], stream));
    // the prefill already produced token 0; every decode step feeds one token and yields the next
    int steps = 0;
    static const bool host_timing = [] { const char* e = getenv("Q3A_DEBUG_HOST_TIMING"); return e && atoi(e) != 0; }();
    const auto h0 = std::chrono::steady_clock::now();
    if (fixed_new > 0) {
      steps = fixed_new - 1;
      decode_steps(steps);
      if (host_timing) fprintf(stderr, "[q3a host timing] %d graph launches enqueued in %.1f us\n", steps,
                               std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - h0).count());
    } else {
      // Natural EOS (inference.rs:160-167).  The stop condition of the whole batch is evaluated on the device
      // (argmax_finalize: n_done == B) and published to pinned host memory together with a progress counter; the host keeps
      // `ahead` graph replays enqueued in front of the device and reads those two words -- no stream synchronisation and no
      // D2H copy inside the loop, so the device never idles between steps.  Steps enqueued past a sequence's EOS only
      // append ids that fetch_ids cuts off (each utterance ends at ITS first EOS); at most `ahead` whole-batch steps are
      // wasted after the last sequence finishes.
      steps = run_ahead(host_prog, max_new - 1, "greedy");
    }
    HIPCHK(hipEventRecord(ev[4], stream));
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipGetLastError());
    decode_timings(steps);
  }

  void fetch_ids(int32_t* out, int stride, int32_t* out_lens) {
    if (!at(Stage::Decoding) || beam_w() > 0) fail("q3a_fetch_ids: nothing generated");
    fetch_generated<int32_t>(nullptr, out, stride, out_lens);
  }
  // opts.token_logprobs: the log-probability of every id fetch_ids returns, same order and lengths
  void fetch_logprobs(float* out, int stride, int32_t* out_lens) {
    if (!token_lp()) fail("q3a_fetch_logprobs: the engine was created without opts.token_logprobs = 1");
    require(Stage::Decoding, "q3a_fetch_logprobs: nothing generated");
    fetch_generated<float>(&step.out_lp, out, stride, out_lens);
  }
  // What the two share: out_ids to the host, the length rule, and every sequence's first min(length, stride) words -- of `vals`
  // ([B][max_new] on the device, T words), or with vals null of the ids themselves.
  template <class T> void fetch_generated(const DevBuf* vals, T* out, int stride, int32_t* out_lens) {
    std::vector<int> ids((size_t)B * max_new);
    std::vector<T> v(vals ? ids.size() : 0);
    HIPCHK(hipMemcpy(ids.data(), step.out_ids.p, ids.size() * 4, hipMemcpyDeviceToHost));
    if (vals) HIPCHK(hipMemcpy(v.data(), vals->p, v.size() * sizeof(T), hipMemcpyDeviceToHost));
    generated_lens(ids, out_lens);
    for (int s = 0; s < B; ++s)
      for (int i = 0; i < std::min(out_lens[s], stride); ++i) out[(size_t)s * stride + i] = vals ? v[(size_t)s * max_new + i] : (T)ids[(size_t)s * max_new + i];
  }
  // lengths of the generated ids per sequence (all = out_ids on the host)
  void generated_lens(const std::vector<int>& all, int32_t* out_lens) {
    std::vector<int> sc(B);
    HIPCHK(hipMemcpy(sc.data(), step.step_count.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    for (int s = 0; s < B; ++s) {
      int n = std::min(sc[s], max_new), len = 0;
      for (; len < n; ++len) {
        int t = all[(size_t)s * max_new + len];
        if (!fixed_mode() && (t == kEos0 || t == kEos1)) break;  // generated_ids excludes EOS (inference.rs:163-167)
      }
      out_lens[s] = len;
    }
  }

  // =====================================================================================
  // beam search (include/q3asr.h "beam search"; k_beam.hip).  The B sequences of the batch are U = B / W
  // utterances of W slots.  A round selects on the stored logits: top-W per sequence -> advance (candidates, rank, slots, state,
  // history, stop word) -> KV reorder -> the survivors' tokens through the set_tokens path.  Round 0 runs on the prefill's
  // logits; every later round is the tail of a decode step and is captured / replayed with it.  Nothing comes back to the host
  // inside the loop: the history is back-pointers [round][sequence] that beam_fetch follows afterwards.
  int beam_dbg_S_ = 0, beam_dbg_W_ = 0;  // shape of the last search's tables (q3a_debug_read "beam_*")
  int* beam_prog() const { return host_prog + 2; }  // pinned: [0] advance launches completed, [1] every slot finished

  // refusals of q3a_beam_begin / q3a_beam_search_batch_ptrs that need the batch (prompt lengths P of B sequences)
  void beam_check(const char* what, int W) const {
    if (W < 1 || W > BEAM_MAX_W) fail(std::string(what) + ": width must be 1..8");
    if (B % W != 0) fail(std::string(what) + ": the batch of " + std::to_string(B) + " sequences is not divisible by width " + std::to_string(W));
    if (B > 32) fail(std::string(what) + ": utterances x width = " + std::to_string(B) + " exceeds 32 sequences");
    for (int s = 0; s < B; ++s)
      if (P[s] != P[s / W * W]) fail(std::string(what) + ": the prompts of utterance " + std::to_string(s / W) + " differ in length (its " + std::to_string(W) + " slots must hold the same prompt)");
    if (d.vocab < W) fail(std::string(what) + ": vocabulary smaller than the width");
  }
  // Logit bias (q3asr.h q3a_set_logit_bias).  The dense vector is composed on the host and copied on the engine's stream; the call
  // waits for the copy (the host vector is the call's own), nothing in a decode loop ever does.  The engine holds no decode state
  // afterwards, so the vector never changes under a live sequence, and "on / off" is part of the graph signature.
  void set_logit_bias(const int32_t* ids, const float* bias, int n, float default_bias) {
    const char* what = "q3a_set_logit_bias";
    require_asr(what);
    const int V = d.vocab;
    if (n < 0 || (n > 0 && (!ids || !bias))) fail(std::string(what) + ": bad argument");
    if (!(default_bias == 0.f || default_bias == -INFINITY)) fail(std::string(what) + ": default_bias must be 0 or -inf");
    std::vector<float> b((size_t)V, default_bias);
    std::vector<uint8_t> seen((size_t)V, 0);
    for (int i = 0; i < n; ++i) {
      const int id = ids[i];
      if (id < 0 || id >= V) fail(std::string(what) + ": id " + std::to_string(id) + " is outside the vocabulary (" + std::to_string(V) + ")");
      if (seen[id]) fail(std::string(what) + ": duplicate id " + std::to_string(id));
      seen[id] = 1;
      const float v = bias[i];
      if (std::isnan(v) || v == INFINITY) fail(std::string(what) + ": the bias of id " + std::to_string(id) + " is NaN or +inf (finite or -inf only)");
      b[id] = v;
    }
    int finite = 0;
    for (int r = 0; r < V; ++r) finite += b[r] != -INFINITY;
    if (finite == 0) fail(std::string(what) + ": the bias has no finite entry (every token would be suppressed)");
    const bool on = !(n == 0 && default_bias == 0.f);
    const bool eos_open = (kEos0 < V && b[kEos0] != -INFINITY) || (kEos1 < V && b[kEos1] != -INFINITY);
    repetition_bias_check(what, rep_ngram_, eos_open, finite);
    if (!row_table_on_) sequence_bias_check(what, seq_bias_inf_targets_, default_bias == -INFINITY, finite, rep_ngram_);  // (list 0 for every row)
    rows_finite_check(what, rows_, seq_list_inf_, default_bias == -INFINITY, finite, eos_open);
    drop_decode_state();
    HIPCHK(hipMemcpyAsync(step.logit_bias.p, b.data(), (size_t)V * 4, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    logit_bias_on_ = on;
    logit_bias_finite_ = finite;
    logit_bias_eos_open_ = eos_open;
    logit_bias_allow_list_ = default_bias == -INFINITY;
  }
  // Repetition penalty and no-repeat n-grams (q3asr.h q3a_set_repetition).  Penalty and n-gram size live in a device buffer the kernel
  // reads, so a new setting replays the same graph; on / off is part of the graph signature.  No decode state afterwards.
  void set_repetition(float penalty, int ngram) {
    const char* what = "q3a_set_repetition";
    require_asr(what);
    if (!std::isfinite(penalty) || !(penalty > 0.f)) fail(std::string(what) + ": repetition_penalty must be finite and > 0 (1 turns the penalty off)");
    if (ngram < 0 || ngram > 32) fail(std::string(what) + ": no_repeat_ngram_size must lie in [0, 32] (0 turns the ban off)");
    const bool on = !(penalty == 1.f && ngram == 0);
    if (on && d.vocab > REPEAT_MAX_VOCAB)
      fail(std::string(what) + ": the vocabulary (" + std::to_string(d.vocab) + ") exceeds the " + std::to_string(REPEAT_MAX_VOCAB) + " ids the kernel's bitmap holds");
    repetition_bias_check(what, ngram, logit_bias_eos_open_, logit_bias_finite_);
    sequence_bias_check(what, seq_bias_inf_targets_, logit_bias_allow_list_, logit_bias_finite_, ngram);
    uint32_t w[4] = {0, (uint32_t)ngram, 0, 0};
    memcpy(&w[0], &penalty, 4);
    drop_decode_state();
    HIPCHK(hipMemcpyAsync(step.rep_params.p, w, 16, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    rep_penalty_ = penalty; rep_ngram_ = ngram;
    uni_on_[2] = on;
    refresh_switches();
  }
  // the one way a row could run out of finite logits: an n-gram ban over a bias that forbids every EOS and leaves no more tokens
  // finite than a sequence may generate (asked by whichever of the two setters comes second)
  void repetition_bias_check(const char* what, int ngram, bool eos_open, int finite) const {
    if (ngram > 0 && !eos_open && finite <= opts.max_new_tokens)
      fail(std::string(what) + ": no_repeat_ngram_size " + std::to_string(ngram) + " over a logit bias that forbids both EOS ids and leaves " + std::to_string(finite) +
           " tokens finite, no more than max_new_tokens (" + std::to_string(opts.max_new_tokens) + "): a row could run out of finite logits");
  }
  // Sequence bias (q3asr.h q3a_set_sequence_bias).  The list is laid out on the host (seqbias_layout) and lives in ONE device buffer of
  // fixed size the kernel reads, counts included, so another list replays the same graph; on / off is part of the graph signature.
  // The buffer is allocated by the first non-empty list and kept until the engine goes.  No decode state afterwards.
  void set_sequence_bias(const int32_t* ids, const int32_t* lens, const float* bias, int n) {
    if (n < 0) fail("q3a_set_sequence_bias: bad argument");
    set_sequence_bias_lists("q3a_set_sequence_bias", ids, lens, bias, &n, n > 0 ? 1 : 0);
  }
  // q3a_set_sequence_bias_lists: the same for several lists in the one buffer, its directory included (q3a_set_sequence_bias is the
  // case of one list).  Without a row table every row reads list 0; with one, row s reads the list its record names.
  void set_sequence_bias_lists(const char* what, const int32_t* ids, const int32_t* lens, const float* bias, const int32_t* list_lens, int n_lists) {
    require_asr(what);
    const SeqBiasTable tb = seqbias_layout_lists(what, ids, lens, bias, list_lens, n_lists, d.vocab);
    // without a row table every row reads list 0: the uniform rule; with one the rule is asked row by row, and again for list 0 when
    // the table is cleared
    if (!row_table_on_) sequence_bias_check(what, tb.inf_targets, logit_bias_allow_list_, logit_bias_finite_, rep_ngram_);
    for (size_t r = 0; r < rows_.size(); ++r)  // (the second of the two setters to come asks)
      if (rows_[r].sequence_list >= n_lists)
        fail(std::string(what) + ": row " + std::to_string(r) + " of the row table names sequence_list " + std::to_string(rows_[r].sequence_list) + ", outside [-1, " + std::to_string(n_lists) + ")");
    rows_finite_check(what, rows_, tb.list_inf_targets, logit_bias_allow_list_, logit_bias_finite_, logit_bias_eos_open_);
    drop_decode_state();
    if (tb.entries > 0 || step.seq_bias.p) {  // (an engine that never had a list has no buffer, and clearing allocates none)
      step.seq_bias.ensure(SEQBIAS_TABLE_WORDS * 4);
      HIPCHK(hipMemcpyAsync(step.seq_bias.p, tb.words.data(), SEQBIAS_TABLE_WORDS * 4, hipMemcpyHostToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));
    }
    uni_on_[3] = n_lists > 0 && tb.list_entries[0] > 0;
    seq_bias_stats_[0] = uni_on_[3]; seq_bias_stats_[1] = tb.entries; seq_bias_stats_[2] = tb.ids; seq_bias_stats_[3] = tb.groups;
    seq_bias_inf_targets_ = tb.inf_targets;
    seq_list_entries_ = tb.list_entries; seq_list_inf_ = tb.list_inf_targets;
    refresh_switches();
  }
  // Row options (q3asr.h q3a_set_row_options).  The records go to step.row_opts in the words the uniform buffers hold, one per row
  // and region, so the kernels read row s's record where they read the one record (row stride 4 instead of 0) and another table of
  // the same switches replays the same graph.  n_rows = 0 clears: the uniform settings, remembered all along, are in force again.
  void set_row_options(const q3a_row_options* rows, int n_rows) {
    const char* what = "q3a_set_row_options";
    require_asr(what);
    row_options_check(what, rows, n_rows, (int)seq_list_entries_.size(), d.vocab);
    const std::vector<q3a_row_options> table(rows, rows + n_rows);
    rows_finite_check(what, table, seq_list_inf_, logit_bias_allow_list_, logit_bias_finite_, logit_bias_eos_open_);
    // clearing puts every row back on list 0 under the uniform n-gram size: the rule no setter asked for it while the table was on
    if (n_rows == 0 && row_table_on_) sequence_bias_check(what, seq_bias_inf_targets_, logit_bias_allow_list_, logit_bias_finite_, rep_ngram_);
    drop_decode_state();
    if (n_rows > 0) {
      const std::vector<uint32_t> w = row_options_words(rows, n_rows);
      step.row_opts.ensure(w.size() * 4);
      HIPCHK(hipMemcpyAsync(step.row_opts.p, w.data(), w.size() * 4, hipMemcpyHostToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));
    }
    rows_ = table;
    row_table_on_ = n_rows > 0;
    refresh_switches();
  }
  // the switches the step runs under (graph signature): the uniform setters' own, or "for any row" of the table
  void refresh_switches() {
    bool on[4] = {uni_on_[0], uni_on_[1], uni_on_[2], uni_on_[3]};
    if (row_table_on_) {
      on[0] = on[1] = on[2] = on[3] = false;
      for (const q3a_row_options& r : rows_) {
        on[0] |= r.temperature > 0.f;
        on[1] |= r.temperature > 0.f && (r.top_k != 0 || r.top_p != 1.f);  // (a greedy row is not filtered)
        on[2] |= !(r.repetition_penalty == 1.f && r.no_repeat_ngram_size == 0);
        on[3] |= r.sequence_list >= 0 && seq_list_entries_[(size_t)r.sequence_list] > 0;
      }
    }
    sampling_on_ = on[0]; sampling_filter_on_ = on[1]; repetition_on_ = on[2]; sequence_bias_on_ = on[3];
  }
  // the two run-out-of-finite-logits rules, row by row: each row's n-gram size and the -inf targets of its own list
  void rows_finite_check(const char* what, const std::vector<q3a_row_options>& rows, const std::vector<int>& list_inf, bool allow_list, int finite, bool eos_open) const {
    for (size_t r = 0; r < rows.size(); ++r) {
      const std::string w = std::string(what) + ": row " + std::to_string(r);
      const int k = rows[r].sequence_list, inf = k >= 0 && (size_t)k < list_inf.size() ? list_inf[(size_t)k] : 0;
      repetition_bias_check(w.c_str(), rows[r].no_repeat_ngram_size, eos_open, finite);
      sequence_bias_check(w.c_str(), inf, allow_list, finite, rows[r].no_repeat_ngram_size);
    }
  }
  // a prefill under a row table serves exactly the table's rows
  void row_table_batch_check(const char* what, int b) const {
    if (row_table_on_ && b != (int)rows_.size())
      fail(std::string(what) + ": a batch of " + std::to_string(b) + " sequences under a row table of " + std::to_string(rows_.size()) + " rows (q3a_set_row_options; n_rows = 0 clears it)");
  }
  // the one way a row could run out of finite logits under a sequence bias: -inf entries over an allow-list that leaves no more
  // tokens finite than those entries can take away, plus -- with an n-gram ban -- the tokens a sequence may generate (asked by
  // whichever of the three setters comes second)
  void sequence_bias_check(const char* what, int inf_targets, bool allow_list, int finite, int ngram) const {
    const long taken = (long)inf_targets + (ngram > 0 ? opts.max_new_tokens : 0);
    if (inf_targets > 0 && allow_list && finite <= taken)
      fail(std::string(what) + ": -inf sequence-bias entries on " + std::to_string(inf_targets) + " target(s)" + (ngram > 0 ? ", no_repeat_ngram_size " + std::to_string(ngram) + " (max_new_tokens " + std::to_string(opts.max_new_tokens) + ")" : "") +
           " over an allow-list logit bias that leaves " + std::to_string(finite) + " tokens finite: a row could run out of finite logits");
  }
  void beam_sequence_bias_check(const char* what) const {
    if (sequence_bias_on_) fail(std::string(what) + ": a sequence bias is on (q3a_set_sequence_bias); beam slots reorder their histories -- turn it off first");
  }
  // Top log-probabilities (q3asr.h q3a_set_top_logprobs).  n lives in a device word the kernel reads, so another n > 0 replays the
  // same graph; on / off is part of the graph signature.  No decode state afterwards.  The buffers come with the next prefill.
  void set_top_logprobs(int n) {
    const char* what = "q3a_set_top_logprobs";
    require_asr(what);
    if (n < 0 || n > TOP_LP_MAX) fail(std::string(what) + ": n must lie in [0, " + std::to_string(TOP_LP_MAX) + "] (0 turns it off)");
    if (n > d.vocab) fail(std::string(what) + ": n " + std::to_string(n) + " exceeds the vocabulary (" + std::to_string(d.vocab) + ")");
    if (n > 0 && d.vocab > TOP_LP_MAX_VOCAB) fail(std::string(what) + ": the vocabulary (" + std::to_string(d.vocab) + ") exceeds the " + std::to_string(TOP_LP_MAX_VOCAB) + " ids the kernel's candidate table holds");
    drop_decode_state();
    top_lp_n_ = n;
    top_lp_on_ = n > 0;
  }
  // the history of the last run: [B][stride][n_stride] on the host, row b's first min(out_lens[b], stride) steps, of each the first
  // min(n, n_stride) entries
  void fetch_top_logprobs(int32_t* out_i, float* out_l, int stride, int n_stride, int32_t* out_lens) {
    const char* what = "q3a_fetch_top_logprobs";
    require_asr(what);
    if (!at(Stage::Decoding) || beam_w() > 0) fail(std::string(what) + ": nothing generated");
    if (top_lp_run_n_ <= 0 || !step.top_ids.p || !step.top_lp.p) fail(std::string(what) + ": the last run had top log-probabilities off (q3a_set_top_logprobs)");
    const size_t words = (size_t)B * max_new * TOP_LP_MAX;
    std::vector<int> ids((size_t)B * max_new), ti(words);
    std::vector<float> tl(words);
    HIPCHK(hipMemcpy(ids.data(), step.out_ids.p, ids.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ti.data(), step.top_ids.p, words * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(tl.data(), step.top_lp.p, words * 4, hipMemcpyDeviceToHost));
    generated_lens(ids, out_lens);
    const int n = std::min(top_lp_run_n_, n_stride);
    for (int s = 0; s < B; ++s)
      for (int i = 0; i < std::min(out_lens[s], stride); ++i)
        for (int k = 0; k < n; ++k) {
          const size_t src = ((size_t)s * max_new + i) * TOP_LP_MAX + k, dst = ((size_t)s * stride + i) * n_stride + k;
          out_i[dst] = ti[src]; out_l[dst] = tl[src];
        }
  }
  void beam_top_logprobs_check(const char* what) const {
    if (top_lp_on_) fail(std::string(what) + ": top log-probabilities are on (q3a_set_top_logprobs); beam search re-orders rows -- turn them off first");
  }
  void beam_repetition_check(const char* what) const {
    if (repetition_on_) fail(std::string(what) + ": repetition control is on (q3a_set_repetition); beam slots reorder their histories -- turn it off first");
  }
  // Sampling (q3asr.h q3a_set_sampling).  The setting lives in a device buffer the kernels read, so a new temperature, min_p or seed
  // replays the same graph; on / off is part of the graph signature.  No decode state afterwards, as after q3a_set_logit_bias.
  void set_sampling(float temperature, float min_p, uint64_t seed) {
    const char* what = "q3a_set_sampling";
    require_asr(what);
    if (!(temperature >= 0.f) || !std::isfinite(temperature)) fail(std::string(what) + ": temperature must be finite and >= 0 (0 turns sampling off)");
    if (!(min_p >= 0.f && min_p <= 1.f)) fail(std::string(what) + ": min_p must lie in [0, 1]");
    uint32_t w[4];
    memcpy(&w[0], &temperature, 4); memcpy(&w[1], &min_p, 4);
    w[2] = (uint32_t)seed; w[3] = (uint32_t)(seed >> 32);
    drop_decode_state();
    HIPCHK(hipMemcpyAsync(step.samp_params.p, w, 16, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    memcpy(samp_words_, w, 16);
    uni_on_[0] = temperature > 0.f;
    refresh_switches();
  }
  // Top-k / top-p (q3asr.h q3a_set_sampling_filter).  As q3a_set_sampling: the values live in a device buffer, on / off is part of
  // the graph signature, no decode state afterwards.  The first setting that is not (0, 1) allocates the buffer.
  void set_sampling_filter(int32_t top_k, float top_p) {
    const char* what = "q3a_set_sampling_filter";
    require_asr(what);
    if (top_k < 0) fail(std::string(what) + ": top_k must be >= 0 (0 turns top-k off)");
    if (!(top_p > 0.f && top_p <= 1.f)) fail(std::string(what) + ": top_p must lie in (0, 1] (1 turns top-p off)");
    const bool on = top_k != 0 || top_p != 1.f;
    uint32_t w[4] = {(uint32_t)top_k, 0u, 0u, 0u};
    memcpy(&w[1], &top_p, 4);
    drop_decode_state();
    if (on) step.samp_filter.ensure(16);
    if (step.samp_filter.p) {
      HIPCHK(hipMemcpyAsync(step.samp_filter.p, w, 16, hipMemcpyHostToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));
    }
    memcpy(samp_filter_words_, w, 8);
    uni_on_[1] = on;
    refresh_switches();
  }
  void beam_sampling_check(const char* what) const {
    if (sampling_on_) fail(std::string(what) + ": sampling is on (q3a_set_sampling with temperature > 0); beam search selects deterministically -- turn it off first");
  }
  void beam_bias_check(const char* what, int W) const {
    if (logit_bias_on_ && W > logit_bias_finite_)
      fail(std::string(what) + ": width " + std::to_string(W) + " exceeds the " + std::to_string(logit_bias_finite_) + " tokens the logit bias leaves finite");
  }

  // state for a search over the prefilled batch, then round 0 on the prefill's logits (enqueued; nothing waited for)
  void beam_begin(const char* what, int W) {
    require(Stage::Decoding, std::string(what) + ": no prefill state (call q3a_prefill first)");
    beam_check(what, W);
    beam_sampling_check(what);
    beam_repetition_check(what);
    beam_top_logprobs_check(what);
    beam_sequence_bias_check(what);
    beam_bias_check(what, W);
    if (!head_logits() || pos_hi_ != *std::max_element(P.begin(), P.end()))
      fail(std::string(what) + ": needs the logits of q3a_prefill (call it directly after the prefill)");
    const int S = B, nc = beam_topk_chunks(d.vocab);
    step.beam_cand_val.ensure((size_t)S * nc * W * 4); step.beam_cand_idx.ensure((size_t)S * nc * W * 4);
    step.beam_part_max.ensure((size_t)S * nc * 4); step.beam_part_sum.ensure((size_t)S * nc * 4);
    step.beam_topk_ids.ensure((size_t)S * W * 4); step.beam_topk_lp.ensure((size_t)S * W * 4);
    step.beam_parent.ensure((size_t)S * 4); step.beam_token.ensure((size_t)S * 4); step.beam_feed.ensure((size_t)S * 4);
    step.beam_hist_parent.ensure((size_t)max_new * S * 4); step.beam_hist_token.ensure((size_t)max_new * S * 4); step.beam_hist_lp.ensure((size_t)max_new * S * 4);
    std::vector<float> sc((size_t)S, -INFINITY);
    for (int s = 0; s < S; s += W) sc[s] = 0.f;  // only slot 0 of every utterance is live
    std::vector<uint8_t> fin((size_t)S, 0);
    std::vector<int> st(BEAM_ST_COUNT, 0);
    upload(step.beam_score, sc, stream); upload(step.beam_finished, fin, stream); upload(step.beam_state, st, stream); upload(step.beam_lo, P, stream);
    HIPCHK(hipStreamSynchronize(stream));  // (host vectors above; and no earlier launch still writes the progress words)
    __atomic_store_n(&beam_prog()[0], 0, __ATOMIC_RELAXED);
    __atomic_store_n(&beam_prog()[1], 0, __ATOMIC_RELAXED);
    begin_search(W);
    beam_dbg_S_ = S; beam_dbg_W_ = W;
    step.enqueue_beam_round();
    HIPCHK(hipGetLastError());
  }
  // The natural-EOS loop of the greedy search and of the beam rounds after round 0: `ahead` decode steps stay enqueued in front of
  // the device, and the two pinned words prog[0] (launches of the step's last kernel completed; the prefill / round 0 counts 1) and
  // prog[1] (stop) are read without synchronising.  Returns the decode steps enqueued, at most `limit`.
  // `base`: what prog[0] stood at before the first step of this loop, less one (a draft-verified prefill leaves it at k + 1).
  int run_ahead(const int* prog, int limit, const char* label, int base = 0) {
    const int ahead = std::max(1, knobs().eos_run_ahead.load());
    int steps = 0;
    unsigned spins = 0;
    while (steps < limit) {
      if (__atomic_load_n(&prog[1], __ATOMIC_RELAXED)) break;
      const int fin = __atomic_load_n(&prog[0], __ATOMIC_RELAXED);
      if (steps - std::max(fin - 1 - base, 0) < ahead) {
        decode_steps(1);
        ++steps;
        spins = 0;
      } else if (++spins > 64) {
        sched_yield();
        if ((spins & 0xffff) == 0) {  // a device fault must end the wait: the progress words would never move again
          const hipError_t q = hipStreamQuery(stream);
          if (q != hipSuccess && q != hipErrorNotReady) HIPCHK(q);
          if (q == hipSuccess && steps - std::max(__atomic_load_n(&prog[0], __ATOMIC_RELAXED) - 1 - base, 0) >= ahead)
            fail(std::string(label) + " loop: the stream drained but the device-side progress counter did not advance");
        }
      }
    }
    return steps;
  }
  std::vector<int> beam_state_host() {
    std::vector<int> st(BEAM_ST_COUNT);
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipMemcpy(st.data(), step.beam_state.p, st.size() * 4, hipMemcpyDeviceToHost));
    return st;
  }
  // hypotheses of every utterance, best first: out_ids [U][W][stride], out_lens / out_scores / out_finished [U][W], out_lp nullable
  // [U][W][stride + 1] (per token, then the EOS's when finished)
  void beam_fetch(int32_t* out, int stride, int32_t* out_lens, float* out_scores, uint8_t* out_fin, float* out_lp) {
    const int W = beam_w(), S = B, U = B / W;  // (a live search: the callers' check)
    const int R = std::min(beam_state_host()[BEAM_ST_ROUNDS], max_new);
    std::vector<int> hp((size_t)R * S), ht((size_t)R * S);
    std::vector<float> hl((size_t)R * S), sc(S);
    std::vector<uint8_t> fin(S);
    if (R > 0) {
      HIPCHK(hipMemcpy(hp.data(), step.beam_hist_parent.p, hp.size() * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(ht.data(), step.beam_hist_token.p, ht.size() * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(hl.data(), step.beam_hist_lp.p, hl.size() * 4, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipMemcpy(sc.data(), step.beam_score.p, (size_t)S * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(fin.data(), step.beam_finished.p, (size_t)S, hipMemcpyDeviceToHost));
    std::vector<int> toks;
    std::vector<float> lps;
    for (int u = 0; u < U; ++u) {
      std::vector<int> order(W);
      for (int j = 0; j < W; ++j) order[j] = j;
      std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return sc[u * W + x] > sc[u * W + y]; });  // larger score, then smaller slot
      for (int k = 0; k < W; ++k) {
        const int q = u * W + order[k];
        toks.clear(); lps.clear();
        for (int r = R - 1, cur = q; r >= 0; --r) {  // back-pointers: round r put (token, lp) into slot `cur`, continuing slot parent
          const size_t h = (size_t)r * S + cur;
          if (ht[h] >= 0) { toks.push_back(ht[h]); lps.push_back(hl[h]); }
          cur = hp[h];
        }
        std::reverse(toks.begin(), toks.end());
        std::reverse(lps.begin(), lps.end());
        const int n_lp = (int)toks.size();
        if (fin[q] && !toks.empty()) toks.pop_back();  // the ids exclude the EOS; its log-probability stays
        const int n = (int)toks.size();
        if (n > stride) fail("q3a_beam_fetch: a hypothesis has " + std::to_string(n) + " ids, more than stride " + std::to_string(stride));
        const size_t o = (size_t)u * W + k;
        for (int i = 0; i < n; ++i) out[o * stride + i] = toks[i];
        out_lens[o] = n;
        if (out_scores) out_scores[o] = sc[q];
        if (out_fin) out_fin[o] = fin[q];
        if (out_lp)
          for (int i = 0; i < n_lp && i < stride + 1; ++i) out_lp[o * (stride + 1) + i] = lps[i];
      }
    }
  }

  // Graphs, streams and events go here, before the members: every DevBuf (taps included) frees itself after this body has run.
  // So the streams, the events and an owned arena now go BEFORE the workspace buffers (they used to go after).  The device-wide wait
  // that the first hipFree implies therefore comes from the arena's, or with a borrowed arena from the first DevBuf's, after the
  // streams are destroyed: legal, since HIP keeps a destroyed stream's resources until its work has finished.
  ~q3a_engine() {
    drop_graphs();
    for (auto cs : chain_streams) (void)hipStreamDestroy(cs);
    for (auto ce : join_ev) (void)hipEventDestroy(ce);
    if (fork_ev) (void)hipEventDestroy(fork_ev);
    if (own_arena && arena) (void)hipFree(arena);
    if (host_prog) (void)hipHostFree(host_prog);
    if (up_stream) { (void)hipStreamSynchronize(up_stream); (void)hipStreamDestroy(up_stream); }
    if (pin_p) (void)hipHostFree(pin_p);
    for (auto ue : up_ev) (void)hipEventDestroy(ue);
    if (up_t0) (void)hipEventDestroy(up_t0);
    if (up_t1) (void)hipEventDestroy(up_t1);
    for (auto& x : ev)
      if (x) (void)hipEventDestroy(x);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// =========================================================================================
// C ABI
// =========================================================================================

namespace q3a {
void set_thread_error(const std::string& msg) { g_last_error = msg; }  // used by host_abi.cpp
void set_error(q3a_engine* e, const char* msg) {
  if (e) e->err = msg;
  g_last_error = msg;
}
}  // namespace q3a

extern "C" {

void q3a_opts_default(q3a_opts* o) {
  memset(o, 0, sizeof(*o));
  o->precise = 0;
  o->max_new_tokens = 4096;
  o->use_graph = 1;
  o->debug_taps = 0;
}

static int32_t create_impl(const char* model_dir, int32_t device, void* dev_arena, uint64_t bytes, const q3a_opts* opts,
                           q3a_engine** out) {
  q3a_engine* e = nullptr;
  try {
    if (!model_dir || !out) fail("null argument");
    e = new q3a_engine();
    e->init_common(model_dir, device, opts);
    if (dev_arena) {
      if (bytes != e->L.total) fail("q3a_engine_create_from_arena: arena size does not match config.json");
      e->arena = (uint8_t*)dev_arena;
      e->own_arena = false;
    } else {
      Checkpoint ck(model_dir);
      std::vector<uint8_t> host(e->L.total);
      pack_arena(e->d, e->L, ck, host.data());
      HIPCHK(hipMalloc((void**)&e->arena, e->L.total));
      e->own_arena = true;
      HIPCHK(hipMemcpy(e->arena, host.data(), e->L.total, hipMemcpyHostToDevice));
    }
    e->check_arena_header();
    e->init_tables();
    e->init_lm_head_q();
    *out = e;
    return 0;
  } catch (const std::exception& ex) {
    g_last_error = ex.what();
    delete e;
    if (out) *out = nullptr;
    return 1;
  }
}

int32_t q3a_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int32_t q3a_engine_create(const char* model_dir, int32_t device, const q3a_opts* opts, q3a_engine** out) {
  return create_impl(model_dir, device, nullptr, 0, opts, out);
}
int32_t q3a_engine_create_from_arena(const char* model_dir, int32_t device, void* device_arena, uint64_t bytes,
                                     const q3a_opts* opts, q3a_engine** out) {
  if (!device_arena) { g_last_error = "null arena"; return 1; }
  return create_impl(model_dir, device, device_arena, bytes, opts, out);
}

int32_t q3a_arena_bytes(const char* model_dir, uint64_t* bytes) {
  q3a_engine* e = nullptr;
  Q3A_TRY(e)
  Dims d = parse_config_file(std::string(model_dir) + "/config.json");
  validate_dims(d);
  *bytes = plan_arena(d).total;
  Q3A_CATCH(e)
}
int32_t q3a_arena_pack(const char* model_dir, void* host_dst, uint64_t bytes) {
  q3a_engine* e = nullptr;
  Q3A_TRY(e)
  Dims d = parse_config_file(std::string(model_dir) + "/config.json");
  validate_dims(d);
  ArenaLayout L = plan_arena(d);
  if (bytes != L.total) fail("q3a_arena_pack: buffer size does not match q3a_arena_bytes");
  Checkpoint ck(model_dir);
  pack_arena(d, L, ck, (uint8_t*)host_dst);
  Q3A_CATCH(e)
}

void q3a_engine_destroy(q3a_engine* e) { delete e; }
const char* q3a_last_error(const q3a_engine* e) { return e ? e->err.c_str() : g_last_error.c_str(); }

int32_t q3a_get_dims(const q3a_engine* e, q3a_dims* o) {
  if (!e || !o) return 1;
  const Dims& d = e->d;
  memset(o, 0, sizeof(*o));
  o->enc_d_model = d.enc_d; o->enc_layers = d.enc_layers; o->enc_heads = d.enc_heads; o->enc_ffn = d.enc_ffn;
  o->num_mel_bins = d.n_mels; o->n_window = d.n_window; o->n_window_infer = d.n_window_infer; o->conv_channels = d.conv_ch;
  o->enc_output_dim = d.enc_out; o->max_source_positions = d.max_source_positions;
  o->vocab_size = d.vocab; o->hidden_size = d.hidden; o->intermediate_size = d.inter; o->dec_layers = d.dec_layers;
  o->num_q_heads = d.n_q; o->num_kv_heads = d.n_kv; o->head_dim = d.head_dim; o->tie_word_embeddings = d.tie_embeddings;
  o->mrope_interleaved = d.mrope_interleaved;
  for (size_t i = 0; i < 4 && i < d.mrope_section.size(); ++i) o->mrope_section[i] = d.mrope_section[i];
  o->rms_norm_eps = d.rms_eps; o->rope_theta = d.rope_theta;
  return 0;
}

int32_t q3a_weights_rounded(const q3a_engine* e) { return e && (e->arena_flags & kFlagWeightsRounded) ? 1 : 0; }

int64_t q3a_num_frames(int64_t n_samples) { return (n_samples + 159) / 160; }
int32_t q3a_num_audio_tokens(const q3a_engine* e, int64_t n_frames) { return e ? e->d.audio_tokens(n_frames) : -1; }

int32_t q3a_build_prompt(int32_t num_audio_tokens, const int32_t* lang_prefix_ids, int32_t n_prefix, int32_t* ids,
                         int32_t* len) {
  // inference.rs:215-257
  static const int32_t head[9] = {151644, 8948, 198, 151645, 198, 151644, 872, 198, 151669};
  static const int32_t tail[6] = {151670, 151645, 198, 151644, 77091, 198};
  if (!lang_prefix_ids) n_prefix = 0;
  int32_t n = 9 + num_audio_tokens + 6 + n_prefix;
  if (len) *len = n;
  if (!ids) return 0;
  int32_t* p = ids;
  for (int i = 0; i < 9; ++i) *p++ = head[i];
  for (int i = 0; i < num_audio_tokens; ++i) *p++ = kAudioPad;
  for (int i = 0; i < 6; ++i) *p++ = tail[i];
  for (int i = 0; i < n_prefix; ++i) *p++ = lang_prefix_ids[i];
  return 0;
}

int32_t q3a_aligner_info(const q3a_engine* e, int32_t* classify_num, int32_t* timestamp_token_id, float* segment_ms) {
  if (!e) return 1;
  if (classify_num) *classify_num = e->d.classify_num;
  if (timestamp_token_id) *timestamp_token_id = e->d.aligner() ? e->d.timestamp_token_id : 0;
  if (segment_ms) *segment_ms = e->d.aligner() ? e->d.timestamp_segment_ms : 0.f;
  return 0;
}

int32_t q3a_align(q3a_engine* e, const int32_t* ids, const int32_t* lens, int32_t B, int32_t* out_classes, int32_t stride,
                  int32_t* out_counts, float* logits_out) {
  if (!e) return 1;
  Q3A_TRY(e)
  e->require_aligner("q3a_align");
  if (!ids || !lens || B < 1 || !out_counts || stride < 0 || (stride > 0 && !out_classes)) fail("q3a_align: bad argument");
  HIPCHK(hipSetDevice(e->device));
  e->require_encoded("q3a_align", B);
  const std::vector<int> rows = e->align_marker_rows(ids, lens, B, stride, out_counts);
  e->setup_prompts(ids, lens, B, 1);
  e->timings = q3a_timings{};
  e->run_align(rows, out_counts, stride, out_classes, logits_out);
  Q3A_CATCH(e)
}

int32_t q3a_align_batch_ptrs(q3a_engine* e, const float* const* pcm16k, const int64_t* n_samples, int32_t B, const int32_t* text_ids,
                             const int32_t* text_lens, int32_t* out_classes, int32_t stride, int32_t* out_counts) {
  if (!e) return 1;
  Q3A_TRY(e)
  e->require_aligner("q3a_align_batch");
  if (!text_lens || !out_counts || stride < 0 || (stride > 0 && !out_classes)) fail("q3a_align_batch: bad argument");
  std::vector<int> rows;
  e->whole_path_front("q3a_align_batch", pcm16k, n_samples, B, 1, 1, [&] {
    std::vector<int64_t> toff(B, 0);  // first text id of every utterance
    for (int s = 0; s < B; ++s) {
      if (text_lens[s] < 0 || (text_lens[s] > 0 && !text_ids)) fail("q3a_align_batch: bad text");
      if (s + 1 < B) toff[s + 1] = toff[s] + text_lens[s];
    }
    auto pr = concat_prompts(B, [&](int s, int32_t* dst) {
      int32_t len = 0;
      q3a_build_align_prompt(e->T[s], text_ids ? text_ids + toff[s] : nullptr, text_lens[s], dst, &len);
      return len;
    });
    rows = e->align_marker_rows(pr.first.data(), pr.second.data(), B, stride, out_counts);
    return pr;
  });
  e->run_align(rows, out_counts, stride, out_classes, nullptr);
  e->front_and_total_timings();
  Q3A_CATCH(e)
}

int32_t q3a_score(q3a_engine* e, const int32_t* prompt_ids, const int32_t* prompt_lens, const int32_t* target_ids,
                  const int32_t* target_lens, int32_t B, float* out_lp, int32_t* out_top_ids, float* out_top_lp, int32_t stride,
                  float* logits_out) {
  if (!e) return 1;
  Q3A_TRY(e)
  e->require_asr("q3a_score");
  if (!prompt_ids || !prompt_lens || !target_lens || B < 1 || stride < 0 || (stride > 0 && !out_lp)) fail("q3a_score: bad argument");
  HIPCHK(hipSetDevice(e->device));
  e->require_encoded("q3a_score", B);
  const auto sp = e->given_plan("q3a_score", q3a_engine::kScored, prompt_ids, prompt_lens, target_ids, target_lens, B, stride);
  e->setup_prompts(sp.ids.data(), sp.lens.data(), B, 1);
  e->timings = q3a_timings{};
  e->run_score(sp, stride, out_lp, out_top_ids, out_top_lp, logits_out);
  Q3A_CATCH(e)
}

int32_t q3a_score_batch_ptrs(q3a_engine* e, const float* const* pcm16k, const int64_t* n_samples, int32_t B,
                             const int32_t* lang_prefix_ids, int32_t n_prefix, const int32_t* target_ids, const int32_t* target_lens,
                             float* out_lp, int32_t* out_top_ids, float* out_top_lp, int32_t stride) {
  if (!e) return 1;
  Q3A_TRY(e)
  e->require_asr("q3a_score_batch");
  if (!target_lens || stride < 0 || (stride > 0 && !out_lp) || n_prefix < 0) fail("q3a_score_batch: bad argument");
  q3a_engine::GivenPlan sp;
  e->whole_path_front("q3a_score_batch", pcm16k, n_samples, B, 1, 1, [&] {
    const auto pr = e->asr_prompts(lang_prefix_ids, n_prefix);
    sp = e->given_plan("q3a_score_batch", q3a_engine::kScored, pr.first.data(), pr.second.data(), target_ids, target_lens, B, stride);
    return std::tie(sp.ids, sp.lens);
  });
  e->run_score(sp, stride, out_lp, out_top_ids, out_top_lp, nullptr);
  e->front_and_total_timings();
  Q3A_CATCH(e)
}

// ---- beam search ----------------------------------------------------------------------------------------------------------
int32_t q3a_beam_begin(q3a_engine* e, int32_t width) {
  if (!e) return 1;
  Q3A_TRY(e)
  e->require_asr("q3a_beam_begin");
  HIPCHK(hipSetDevice(e->device));
  e->beam_begin("q3a_beam_begin", width);
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipGetLastError());
  Q3A_CATCH(e)
}

int32_t q3a_beam_step(q3a_engine* e, uint8_t* all_finished, float* logits_out) {
  if (!e) return 1;
  Q3A_TRY(e)
  e->require_asr("q3a_beam_step");
  HIPCHK(hipSetDevice(e->device));
  if (e->beam_w() <= 0) fail("q3a_beam_step: no beam search (call q3a_beam_begin first)");
  if (e->beam_state_host()[BEAM_ST_ROUNDS] >= e->max_new) fail("q3a_beam_step: the round limit (max_new_tokens) is reached");
  e->begin_step_call();
  e->decode_steps(1);
  const std::vector<int> st = e->beam_state_host();
  HIPCHK(hipGetLastError());
  if (all_finished) *all_finished = st[BEAM_ST_ALL_DONE] ? 1 : 0;
  if (logits_out) HIPCHK(hipMemcpy(logits_out, e->step.logits.p, (size_t)e->B * e->d.vocab * 4, hipMemcpyDeviceToHost));
  Q3A_CATCH(e)
}

int32_t q3a_beam_fetch(q3a_engine* e, int32_t* out_ids, int32_t stride, int32_t* out_lens, float* out_scores, uint8_t* out_finished,
                       float* out_lp) {
  if (!e) return 1;
  Q3A_TRY(e)
  e->require_asr("q3a_beam_fetch");
  if (e->beam_w() <= 0) fail("q3a_beam_fetch: no beam search (call q3a_beam_begin first)");
  if (!out_lens || stride < 0 || (stride > 0 && !out_ids)) fail("q3a_beam_fetch: bad argument");
  HIPCHK(hipSetDevice(e->device));
  e->beam_fetch(out_ids, stride, out_lens, out_scores, out_finished, out_lp);
  Q3A_CATCH(e)
}

int32_t q3a_beam_search_batch_ptrs(q3a_engine* e, const float* const* pcm16k, const int64_t* n_samples, int32_t U,
                                   const int32_t* lang_prefix_ids, int32_t n_prefix, int32_t width, int32_t max_new, int32_t* out_ids,
                                   int32_t stride, int32_t* out_lens, float* out_scores, uint8_t* out_finished, float* out_lp) {
  if (!e) return 1;
  Q3A_TRY(e)
  e->require_asr("q3a_beam_search_batch");
  if (U < 1 || !out_lens || stride < 0 || (stride > 0 && !out_ids) || n_prefix < 0) fail("q3a_beam_search_batch: bad argument");
  if (width < 1 || width > BEAM_MAX_W) fail("q3a_beam_search_batch: width must be 1..8");
  if ((int64_t)U * width > 32) fail("q3a_beam_search_batch: utterances x width = " + std::to_string((int64_t)U * width) + " exceeds 32 sequences");
  const int cap = e->opts.max_new_tokens, want = max_new <= 0 ? cap : std::min(max_new, cap);
  if (stride < want) fail("q3a_beam_search_batch: stride " + std::to_string(stride) + " is below max_new " + std::to_string(want));
  e->beam_sampling_check("q3a_beam_search_batch");
  e->beam_repetition_check("q3a_beam_search_batch");
  e->beam_top_logprobs_check("q3a_beam_search_batch");
  e->beam_sequence_bias_check("q3a_beam_search_batch");
  e->beam_bias_check("q3a_beam_search_batch", width);
  e->row_table_batch_check("q3a_beam_search_batch", U * width);
  e->begin_call(false, true);  // every round selects on the stored logits
  // the W slots of an utterance are W ordinary sequences of the batch
  e->whole_path_front("q3a_beam_search_batch", pcm16k, n_samples, U, width, want, [&] { return e->asr_prompts(lang_prefix_ids, n_prefix); });
  HIPCHK(hipEventRecord(e->ev[2], e->stream));
  e->run_prefill();
  HIPCHK(hipEventRecord(e->ev[3], e->stream));
  e->beam_begin("q3a_beam_search_batch", width);
  e->run_ahead(e->beam_prog(), e->max_new - 1, "beam");
  HIPCHK(hipEventRecord(e->ev[4], e->stream));
  const std::vector<int> st = e->beam_state_host();
  HIPCHK(hipGetLastError());
  e->decode_timings(std::max(st[BEAM_ST_ROUNDS] - 1, 0));
  e->beam_fetch(out_ids, stride, out_lens, out_scores, out_finished, out_lp);
  e->drop_decode_state();  // as after q3a_score
  Q3A_CATCH(e)
}

int32_t q3a_set_logit_bias(q3a_engine* e, const int32_t* ids, const float* bias, int32_t n, float default_bias) {
  if (!e) return 1;
  Q3A_TRY(e)
  HIPCHK(hipSetDevice(e->device));
  e->set_logit_bias(ids, bias, n, default_bias);
  Q3A_CATCH(e)
}

int32_t q3a_set_sampling(q3a_engine* e, float temperature, float min_p, uint64_t seed) {
  if (!e) return 1;
  Q3A_TRY(e)
  HIPCHK(hipSetDevice(e->device));
  e->set_sampling(temperature, min_p, seed);
  Q3A_CATCH(e)
}

int32_t q3a_set_sampling_filter(q3a_engine* e, int32_t top_k, float top_p) {
  if (!e) return 1;
  Q3A_TRY(e)
  HIPCHK(hipSetDevice(e->device));
  e->set_sampling_filter(top_k, top_p);
  Q3A_CATCH(e)
}

int32_t q3a_set_repetition(q3a_engine* e, float repetition_penalty, int32_t no_repeat_ngram_size) {
  if (!e) return 1;
  Q3A_TRY(e)
  HIPCHK(hipSetDevice(e->device));
  e->set_repetition(repetition_penalty, no_repeat_ngram_size);
  Q3A_CATCH(e)
}

int32_t q3a_set_top_logprobs(q3a_engine* e, int32_t n) {
  if (!e) return 1;
  Q3A_TRY(e)
  HIPCHK(hipSetDevice(e->device));
  e->set_top_logprobs(n);
  Q3A_CATCH(e)
}

int32_t q3a_fetch_top_logprobs(q3a_engine* e, int32_t* out_ids, float* out_lp, int32_t stride, int32_t n_stride, int32_t* out_lens) {
  if (!e) return 1;
  Q3A_TRY(e)
  if (!out_lens || stride < 0 || n_stride < 0 || (stride > 0 && n_stride > 0 && (!out_ids || !out_lp))) fail("q3a_fetch_top_logprobs: bad argument");
  HIPCHK(hipSetDevice(e->device));
  e->fetch_top_logprobs(out_ids, out_lp, stride, n_stride, out_lens);
  Q3A_CATCH(e)
}

int32_t q3a_set_sequence_bias(q3a_engine* e, const int32_t* ids, const int32_t* lens, const float* bias, int32_t n) {
  if (!e) return 1;
  Q3A_TRY(e)
  HIPCHK(hipSetDevice(e->device));
  e->set_sequence_bias(ids, lens, bias, n);
  Q3A_CATCH(e)
}

int32_t q3a_set_sequence_bias_lists(q3a_engine* e, const int32_t* ids, const int32_t* lens, const float* bias, const int32_t* list_lens, int32_t n_lists) {
  if (!e) return 1;
  Q3A_TRY(e)
  HIPCHK(hipSetDevice(e->device));
  e->set_sequence_bias_lists("q3a_set_sequence_bias_lists", ids, lens, bias, list_lens, n_lists);
  Q3A_CATCH(e)
}

int32_t q3a_set_row_options(q3a_engine* e, const q3a_row_options* rows, int32_t n_rows) {
  if (!e) return 1;
  Q3A_TRY(e)
  HIPCHK(hipSetDevice(e->device));
  e->set_row_options(rows, n_rows);
  Q3A_CATCH(e)
}

int32_t q3a_upload_pcm(q3a_engine* e, const float* pcm16k, const int64_t* n_samples, int32_t B) {
  if (!e) return 1;
  Q3A_TRY(e)
  HIPCHK(hipSetDevice(e->device));
  e->upload_pcm(pcm16k, n_samples, B);
  Q3A_CATCH(e)
}

int32_t q3a_mel(q3a_engine* e, const float* pcm16k, const int64_t* n_samples, int32_t B, float* mel_out,
                int32_t* n_frames_out) {
  if (!e) return 1;
  Q3A_TRY(e)
  HIPCHK(hipSetDevice(e->device));
  e->upload_pcm(pcm16k, n_samples, B);
  e->run_mel();
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipGetLastError());
  if (n_frames_out)
    for (int u = 0; u < B; ++u) n_frames_out[u] = e->n_frames[u];
  if (mel_out) {
    size_t total = 0;
    for (int u = 0; u < B; ++u) total += (size_t)e->n_frames[u] * e->d.n_mels;
    HIPCHK(hipMemcpy(mel_out, e->mel.p, total * 4, hipMemcpyDeviceToHost));
  }
  Q3A_CATCH(e)
}

int32_t q3a_encode(q3a_engine* e, float* audio_embeds_out, int32_t* T_out) {
  if (!e) return 1;
  Q3A_TRY(e)
  HIPCHK(hipSetDevice(e->device));
  e->run_encoder();
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipGetLastError());
  if (T_out)
    for (int u = 0; u < e->B; ++u) T_out[u] = e->T[u];
  if (audio_embeds_out)
    HIPCHK(hipMemcpy(audio_embeds_out, e->audio_embeds.p, (size_t)e->total_T * e->d.enc_out * 4, hipMemcpyDeviceToHost));
  Q3A_CATCH(e)
}

int32_t q3a_prefill(q3a_engine* e, const int32_t* ids, const int32_t* lens, int32_t B, float* last_logits_out,
                    int32_t* next_ids) {
  if (!e) return 1;
  Q3A_TRY(e)
  e->require_asr("q3a_prefill");
  HIPCHK(hipSetDevice(e->device));
  e->row_table_batch_check("q3a_prefill", B);
  e->begin_call(false, true);
  e->setup_prompts(ids, lens, B, e->opts.max_new_tokens);
  e->run_prefill();
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipGetLastError());
  if (last_logits_out) HIPCHK(hipMemcpy(last_logits_out, e->step.logits.p, (size_t)B * e->d.vocab * 4, hipMemcpyDeviceToHost));
  if (next_ids) HIPCHK(hipMemcpy(next_ids, e->step.next_tok.p, (size_t)B * 4, hipMemcpyDeviceToHost));
  Q3A_CATCH(e)
}

int32_t q3a_decode_step(q3a_engine* e, int32_t* next_ids, uint8_t* done, float* logits_out) {
  if (!e) return 1;
  Q3A_TRY(e)
  e->require_asr("q3a_decode_step");
  if (e->beam_w() > 0) fail("q3a_decode_step: a beam search owns the decode state (q3a_beam_step; a new q3a_prefill returns to the greedy step)");
  HIPCHK(hipSetDevice(e->device));
  {
    // capacity guard: position of the token being fed must stay inside the cache
    std::vector<int> pos(e->B);
    HIPCHK(hipMemcpy(pos.data(), e->step.d_pos.p, (size_t)e->B * 4, hipMemcpyDeviceToHost));
    for (int s = 0; s < e->B; ++s)
      if (pos[s] + 1 > e->max_ctx) fail("q3a_decode_step: KV cache capacity exhausted (max_new_tokens reached)");
  }
  e->begin_step_call();
  e->decode_steps(1);
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipGetLastError());
  if (next_ids) HIPCHK(hipMemcpy(next_ids, e->step.next_tok.p, (size_t)e->B * 4, hipMemcpyDeviceToHost));
  if (done) HIPCHK(hipMemcpy(done, e->step.done.p, (size_t)e->B, hipMemcpyDeviceToHost));
  if (logits_out) HIPCHK(hipMemcpy(logits_out, e->step.logits.p, (size_t)e->B * e->d.vocab * 4, hipMemcpyDeviceToHost));
  Q3A_CATCH(e)
}

int32_t q3a_set_next_tokens(q3a_engine* e, const int32_t* ids, int32_t B) {
  if (!e) return 1;
  Q3A_TRY(e)
  HIPCHK(hipSetDevice(e->device));
  if (!e->at(Stage::Decoding) || B != e->B || e->beam_w() > 0) fail("q3a_set_next_tokens: no decode state / batch mismatch");
  for (int s = 0; s < B; ++s)
    if (ids[s] < 0 || ids[s] >= e->d.vocab) fail("q3a_set_next_tokens: token id out of range");
  e->step.enqueue_forced_tokens(ids);
  HIPCHK(hipStreamSynchronize(e->stream));
  Q3A_CATCH(e)
}

int32_t q3a_run_resident(q3a_engine* e, const int32_t* lang_prefix_ids, int32_t n_prefix, int32_t max_new,
                         int32_t fixed_new_tokens) {
  if (!e) return 1;
  Q3A_TRY(e)
  e->require_asr("q3a_run_resident");
  HIPCHK(hipSetDevice(e->device));
  e->begin_call(fixed_new_tokens > 0, e->opts.debug_taps != 0);
  e->rewind(Stage::Batch);  // mel and encoder run again, on the PCM that is resident
  e->require(Stage::Batch, "q3a_run_resident: no batch uploaded");
  e->row_table_batch_check("q3a_run_resident", e->B);
  // prompts and every table / buffer of the prefill + decode: host integers only (T[] of set_batch), before the batch's first kernel
  const auto pr = e->asr_prompts(lang_prefix_ids, n_prefix);
  e->setup_prompts(pr.first.data(), pr.second.data(), e->B, e->max_new_request(max_new, fixed_new_tokens), true);
  e->run_resident(fixed_new_tokens);
  Q3A_CATCH(e)
}

int32_t q3a_fetch_ids(q3a_engine* e, int32_t* out_ids, int32_t stride, int32_t* out_lens) {
  if (!e) return 1;
  Q3A_TRY(e)
  HIPCHK(hipSetDevice(e->device));
  e->fetch_ids(out_ids, stride, out_lens);
  Q3A_CATCH(e)
}

int32_t q3a_fetch_logprobs(q3a_engine* e, float* out_lp, int32_t stride, int32_t* out_lens) {
  if (!e) return 1;
  Q3A_TRY(e)
  if (!out_lens || (stride > 0 && !out_lp)) fail("q3a_fetch_logprobs: bad argument");
  HIPCHK(hipSetDevice(e->device));
  e->fetch_logprobs(out_lp, stride, out_lens);
  Q3A_CATCH(e)
}

int32_t q3a_transcribe_batch_ptrs(q3a_engine* e, const float* const* pcm16k, const int64_t* n_samples, int32_t B,
                                  const int32_t* lang_prefix_ids, int32_t n_prefix, int32_t max_new, int32_t fixed_new_tokens,
                                  int32_t* out_ids, int32_t stride, int32_t* out_lens) {
  if (!e) return 1;
  Q3A_TRY(e)
  e->require_asr("q3a_transcribe_batch");
  e->row_table_batch_check("q3a_transcribe_batch", B);
  const auto w0 = std::chrono::steady_clock::now();
  e->begin_call(fixed_new_tokens > 0, e->opts.debug_taps != 0);
  e->whole_path_front("q3a_transcribe_batch", pcm16k, n_samples, B, 1, e->max_new_request(max_new, fixed_new_tokens),
                      [&] { return e->asr_prompts(lang_prefix_ids, n_prefix); });
  e->run_resident(fixed_new_tokens, true);
  e->fetch_ids(out_ids, stride, out_lens);
  if (e->io.mode != 0) {
    // (a timing probe must not be able to fail the call: the marker sits on the copy stream, which fetch_ids did not synchronise)
    float ms = 0.f;
    if (hipEventSynchronize(e->up_t1) != hipSuccess || hipEventElapsedTime(&ms, e->up_t0, e->up_t1) != hipSuccess) { (void)hipGetLastError(); ms = 0.f; }
    e->io.h2d_ms = ms;
  }
  e->io.wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
  Q3A_CATCH(e)
}

int32_t q3a_transcribe_batch(q3a_engine* e, const float* pcm16k, const int64_t* n_samples, int32_t B,
                             const int32_t* lang_prefix_ids, int32_t n_prefix, int32_t max_new, int32_t fixed_new_tokens,
                             int32_t* out_ids, int32_t stride, int32_t* out_lens) {
  if (!e) return 1;
  if (!pcm16k || !n_samples || B < 1) { e->err = "q3a_transcribe_batch: bad argument"; return 1; }  // (the rest: the _ptrs form's checks)
  std::vector<const float*> ptrs((size_t)B);
  int64_t off = 0;
  for (int u = 0; u < B; ++u) { ptrs[u] = pcm16k + off; off += n_samples[u]; }
  return q3a_transcribe_batch_ptrs(e, ptrs.data(), n_samples, B, lang_prefix_ids, n_prefix, max_new, fixed_new_tokens, out_ids, stride, out_lens);
}

// ---- draft-verified decoding ----------------------------------------------------------------------------------------------
int32_t q3a_prefill_draft(q3a_engine* e, const int32_t* prompt_ids, const int32_t* prompt_lens, const int32_t* draft_ids, const int32_t* draft_lens,
                          int32_t B, int32_t* accepted_out, int32_t* next_ids_out, float* logits_out) {
  if (!e) return 1;
  Q3A_TRY(e)
  const char* what = "q3a_prefill_draft";
  e->draft_check(what);
  e->row_table_batch_check(what, B);
  if (!prompt_ids || !prompt_lens || !draft_lens || B < 1) fail(std::string(what) + ": bad argument");
  HIPCHK(hipSetDevice(e->device));
  e->require_encoded(what, B);
  const auto dp = e->given_plan(what, q3a_engine::kDrafted, prompt_ids, prompt_lens, draft_ids, draft_lens, B, e->opts.max_new_tokens);
  e->begin_call(false, true);
  e->setup_prompts(dp.ids.data(), dp.lens.data(), B, e->opts.max_new_tokens);
  e->timings = q3a_timings{};
  e->draft_stats_.assign(1, 0);
  std::vector<int> acc;
  e->run_prefill_draft(dp, acc, logits_out);
  for (int s = 0; s < B; ++s) {
    if (accepted_out) accepted_out[s] = acc[s];
    if (next_ids_out) next_ids_out[s] = acc[(size_t)B + s];
  }
  Q3A_CATCH(e)
}

int32_t q3a_transcribe_draft_batch_ptrs(q3a_engine* e, const float* const* pcm16k, const int64_t* n_samples, int32_t B,
                                        const int32_t* lang_prefix_ids, int32_t n_prefix, const int32_t* draft_ids, const int32_t* draft_lens,
                                        int32_t max_new, int32_t max_rounds, int32_t min_tail, int32_t* out_ids, int32_t stride,
                                        int32_t* out_lens, int32_t* accepted_out) {
  if (!e) return 1;
  Q3A_TRY(e)
  const char* what = "q3a_transcribe_draft_batch";
  e->draft_check(what);
  e->row_table_batch_check(what, B);
  if (!draft_lens || !out_lens || stride < 0 || (stride > 0 && !out_ids) || n_prefix < 0 || B < 1) fail(std::string(what) + ": bad argument");
  const auto w0 = std::chrono::steady_clock::now();
  e->begin_call(false, e->opts.debug_taps != 0);
  const int mn = e->max_new_request(max_new, 0), mn_eff = std::min(std::max(mn, 1), e->opts.max_new_tokens);
  std::pair<std::vector<int32_t>, std::vector<int32_t>> pr;  // the prompts without a draft: the same in every round
  q3a_engine::GivenPlan dp;
  e->whole_path_front(what, pcm16k, n_samples, B, 1, mn, [&] {
    pr = e->asr_prompts(lang_prefix_ids, n_prefix);
    dp = e->given_plan(what, q3a_engine::kDrafted, pr.first.data(), pr.second.data(), draft_ids, draft_lens, B, mn_eff);
    return std::tie(dp.ids, dp.lens);
  });
  e->draft_stats_.assign(1, 0);
  HIPCHK(hipEventRecord(e->ev[2], e->stream));
  std::vector<int> acc;
  std::vector<int32_t> cur, cur_lens(B), nxt;
  {
    size_t total = 0;
    for (int s = 0; s < B; ++s) { cur_lens[s] = draft_lens[s]; total += draft_lens[s]; }
    if (total) cur.assign(draft_ids, draft_ids + total);
  }
  for (int round = 0;; ++round) {
    e->run_prefill_draft(dp, acc, nullptr);
    // another round pays while the longest rejected tail is worth a prefill (mel and encoder are not run again)
    int tail = 0;
    for (int s = 0; s < B; ++s) tail = std::max(tail, cur_lens[s] - acc[s] - 1);
    if (round + 1 >= max_rounds || tail < std::max(min_tail, 1)) break;
    nxt.clear();
    size_t off = 0;
    for (int s = 0; s < B; ++s) {
      int32_t need = 0;
      const size_t o = nxt.size();
      nxt.resize(o + (size_t)cur_lens[s] + 1);
      if (q3a_draft_next_round(cur.data() + off, cur_lens[s], acc[s], acc[(size_t)B + s], nxt.data() + o, cur_lens[s] + 1, &need) != 0)
        fail(std::string(what) + ": " + q3a_last_error(nullptr));
      off += cur_lens[s];
      cur_lens[s] = std::min(need, mn_eff);  // (an accepted draft of max_new ids plus the head's next id: the id has no slot)
      nxt.resize(o + cur_lens[s]);
    }
    cur.swap(nxt);
    dp = e->given_plan(what, q3a_engine::kDrafted, pr.first.data(), pr.second.data(), cur.data(), cur_lens.data(), B, mn_eff);
    e->setup_prompts(dp.ids.data(), dp.lens.data(), B, mn);
  }
  HIPCHK(hipEventRecord(e->ev[3], e->stream));
  int min_k = e->max_new;
  for (int s = 0; s < B; ++s) min_k = std::min(min_k, acc[s]);
  // every sequence has k + 1 tokens: the one that has the fewest bounds the steps the loop may still run
  const int steps = e->run_ahead(e->host_prog, e->max_new - 1 - min_k, "draft", acc[0]);
  HIPCHK(hipEventRecord(e->ev[4], e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipGetLastError());
  e->decode_timings(steps);
  e->fetch_ids(out_ids, stride, out_lens);
  if (accepted_out)
    for (int s = 0; s < B; ++s) accepted_out[s] = acc[s];
  e->io.wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
  Q3A_CATCH(e)
}

int32_t q3a_io_timings_last(const q3a_engine* e, q3a_io_timings* out) {
  if (!e || !out) return 1;
  *out = e->io;
  return 0;
}

int32_t q3a_stage_timings(const q3a_engine* e, q3a_timings* out) {
  if (!e || !out) return 1;
  *out = e->timings;
  return 0;
}

int32_t q3a_profile_decode_step(q3a_engine* e, q3a_kernel_profile* out) {
  if (!e || !out) return 1;
  Q3A_TRY(e)
  HIPCHK(hipSetDevice(e->device));
  e->require(Stage::Decoding, "q3a_profile_decode_step: no decode state");
  std::vector<ProfEvent> evs;
  e->prof = &evs;
  try {
    e->decode_steps(1);  // eager while `prof` is set: every launch between a pair of events
    HIPCHK(hipStreamSynchronize(e->stream));
  } catch (...) {
    e->prof = nullptr;
    throw;
  }
  e->prof = nullptr;
  memset(out, 0, sizeof(*out));
  for (auto& pe : evs) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, pe.a, pe.b));
    out->total_us[pe.kclass] += ms * 1000.f;
    out->launches[pe.kclass] += 1;
    out->weight_bytes[pe.kclass] += pe.bytes;
    (void)hipEventDestroy(pe.a);
    (void)hipEventDestroy(pe.b);
  }
  Q3A_CATCH(e)
}

int32_t q3a_profile_weight_stream(q3a_engine* e, int32_t reps, float* avg_us, double* bytes_per_launch, int32_t* launches) {
  if (!e) return 1;
  Q3A_TRY(e)
  HIPCHK(hipSetDevice(e->device));
  e->require(Stage::Decoding, "q3a_profile_weight_stream: no decode state");
  if (e->B > kGemvMaxSeq) fail("q3a_profile_weight_stream: the GEMV path serves at most 2 sequences");
  if (reps < 1) reps = 1;
  const Dims& d = e->d;
  const int S = e->B;
  auto sweep = [&]() {
    for (int li = 0; li < d.dec_layers; ++li) {
      const DecLayerOff& l = e->L.dec[li];
      const auto pj = e->step.layer_projs(li);
      GemvArgs g = e->step.gemv_args(pj.qkv);
      g.x = e->step.x_dec.as<float>(); g.rms_w = e->wf(l.in_ln); g.out = e->step.s_qkv.as<float>();
      KCHK(launch_gemv(g, S, e->stream));
      GemvArgs u = e->step.gemv_args(pj.gu);
      u.x = e->step.x_dec.as<float>(); u.rms_w = e->wf(l.post_ln); u.out = e->step.s_act.as<float>();
      KCHK(launch_gemv(u, S, e->stream));
    }
  };
  // replayed from a hipGraph like the decode step itself: an eager host loop issues ~6 us per launch, slower than
  // these kernels run, and would time the host
  const hipGraphExec_t ge = e->capture_graph([&] { for (int r = 0; r < reps; ++r) sweep(); });
  HIPCHK(hipGraphLaunch(ge, e->stream));  // warm-up (code objects, clocks)
  HIPCHK(hipStreamSynchronize(e->stream));
  hipEvent_t a, b;
  HIPCHK(hipEventCreate(&a));
  HIPCHK(hipEventCreate(&b));
  float ms = 0.f;
  constexpr int kReplays = 3;
  for (int rep = 0; rep < kReplays; ++rep) {  // average over the replays
    HIPCHK(hipEventRecord(a, e->stream));
    HIPCHK(hipGraphLaunch(ge, e->stream));
    HIPCHK(hipEventRecord(b, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, a, b));
    ms += t / kReplays;
  }
  HIPCHK(hipGetLastError());
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  (void)hipGraphExecDestroy(ge);
  const int n = reps * d.dec_layers * 2;
  if (avg_us) *avg_us = ms * 1000.f / (float)n;
  const auto pj0 = e->step.layer_projs(0);
  if (bytes_per_launch) *bytes_per_launch = (pj0.qkv.bytes + pj0.gu.bytes) / 2.0;
  if (launches) *launches = n;
  Q3A_CATCH(e)
}

int32_t q3a_debug_read(q3a_engine* e, const char* name, void* dst, uint64_t bytes, uint64_t* actual) {
  if (!e) return 1;
  Q3A_TRY(e)
  HIPCHK(hipSetDevice(e->device));
  // n bytes at src (device memory: after the stream has drained) to the caller
  auto give = [&](const void* src, size_t n, bool on_device) {
    if (actual) *actual = n;
    if (!dst) return;
    if (bytes < n) fail("q3a_debug_read: destination too small");
    if (!on_device) { memcpy(dst, src, n); return; }
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
  };
  // counters and times, not taps: readable without opts.debug_taps
  const uint64_t device_bytes = g_device_bytes.load();
  const struct { const char* name; const void* src; size_t n; bool on_device; } scalars[] = {
      {"lm_head_prune_stats", e->step.prune_stats.p, 8, true},
      {"align_head_ms", &e->align_head_ms, 4, false},  // the aligner head's launches (norm, classifier, merge) of the last align call
      {"score_head_ms", &e->score_head_ms, 4, false},  // the scoring head's launches (norm, lm_head with the reducing epilogue, merge) of the last score call
      {"device_bytes", &device_bytes, 8, false},       // device memory the DevBufs of the whole process hold
      {"graph_captures", &e->graph_captures_, 4, false},  // decode-step graphs captured so far: a setting that lives in a device buffer adds none
  };
  for (const auto& sc : scalars)
    if (strcmp(name, sc.name) == 0) { give(sc.src, sc.n, sc.on_device); return 0; }
  // the logit bias as the device holds it (zeros while off) and {active, finite entries}
  if (strcmp(name, "logit_bias") == 0) {
    e->require_asr("q3a_debug_read: logit_bias");
    give(e->step.logit_bias.p, (size_t)e->d.vocab * 4, true);
    return 0;
  }
  if (strcmp(name, "draft_stats") == 0) {  // the last draft call: rounds run, then the rows prefilled in each round
    give(e->draft_stats_.data(), e->draft_stats_.size() * 4, false);
    return 0;
  }
  if (strcmp(name, "sampling") == 0) {  // {on, temperature bits, min_p bits, seed low, seed high} as last set
    e->require_asr("q3a_debug_read: sampling");
    const uint32_t st[5] = {e->uni_on_[0] ? 1u : 0u, e->samp_words_[0], e->samp_words_[1], e->samp_words_[2], e->samp_words_[3]};
    give(st, 20, false);
    return 0;
  }
  if (strcmp(name, "sampling_filter") == 0) {  // {on, top_k, top_p bits} as last set
    e->require_asr("q3a_debug_read: sampling_filter");
    const uint32_t st[3] = {e->uni_on_[1] ? 1u : 0u, e->samp_filter_words_[0], e->samp_filter_words_[1]};
    give(st, 12, false);
    return 0;
  }
  if (strcmp(name, "sample_threshold") == 0 || strcmp(name, "sample_kept") == 0) {  // the threshold stage of the last sampled step
    e->require_asr("q3a_debug_read: sample_threshold");
    const size_t S = (size_t)e->B;
    // (the decode state: a prefill under the setting has run and nothing has dropped it since -- a setter does -- so the values are this run's)
    if (!(e->sampling_on_ && e->sampling_filter_on_) || !e->at(Stage::Decoding) || !e->step.samp_sel.p || S == 0 || e->step.samp_sel.cap < S * 8)
      fail(std::string("q3a_debug_read: '") + name + "' needs a step sampled with q3a_set_sampling_filter on (no decode state under that setting)");
    const bool kept = strcmp(name, "sample_kept") == 0;  // [S] thresholds, then [S] counts
    give((const uint8_t*)e->step.samp_sel.p + (kept ? S * 4 : 0), S * 4, true);
    return 0;
  }
  if (strcmp(name, "top_logprobs") == 0) {  // n as last set
    e->require_asr("q3a_debug_read: top_logprobs");
    const int32_t w[1] = {e->top_lp_n_};
    give(w, 4, false);
    return 0;
  }
  if (strcmp(name, "repetition") == 0) {  // {on, penalty bits, n-gram size} as last set
    e->require_asr("q3a_debug_read: repetition");
    uint32_t st[3] = {e->uni_on_[2] ? 1u : 0u, 0u, (uint32_t)e->rep_ngram_};
    memcpy(&st[1], &e->rep_penalty_, 4);
    give(st, 12, false);
    return 0;
  }
  if (strcmp(name, "sequence_bias") == 0) {  // {on, entries, ids over all entries, distinct targets} of the list as last set
    e->require_asr("q3a_debug_read: sequence_bias");
    give(e->seq_bias_stats_, 16, false);
    return 0;
  }
  if (strcmp(name, "row_options") == 0) {  // the table as uploaded: n_rows records of q3a_row_options (nothing while no table is set)
    e->require_asr("q3a_debug_read: row_options");
    give(e->rows_.data(), e->rows_.size() * sizeof(q3a_row_options), false);
    return 0;
  }
  if (strcmp(name, "logit_bias_stats") == 0) {
    e->require_asr("q3a_debug_read: logit_bias");
    const int32_t st[2] = {e->logit_bias_on_ ? 1 : 0, e->logit_bias_finite_};
    give(st, 8, false);
    return 0;
  }
  // the last round of the last beam search (tables of beam_dbg_S_ sequences x beam_dbg_W_)
  const size_t bS = (size_t)e->beam_dbg_S_, bW = (size_t)e->beam_dbg_W_;
  const struct { const char* name; const DevBuf* buf; size_t n; } beams[] = {
      {"beam_topk_ids", &e->step.beam_topk_ids, bS * bW * 4}, {"beam_topk_lp", &e->step.beam_topk_lp, bS * bW * 4},
      {"beam_parent", &e->step.beam_parent, bS * 4}, {"beam_token", &e->step.beam_token, bS * 4}, {"beam_score", &e->step.beam_score, bS * 4},
      {"beam_finished", &e->step.beam_finished, bS}, {"beam_stats", &e->step.beam_state, 16},
  };
  for (const auto& bm : beams)
    if (strcmp(name, bm.name) == 0) {
      if (bS == 0) fail(std::string("q3a_debug_read: '") + name + "' before any beam search");
      give(bm.buf->p, bm.n, true);
      return 0;
    }
  auto it = e->taps.bufs.find(name);
  if (it == e->taps.bufs.end()) fail(std::string("q3a_debug_read: no tap named '") + name + "' (opts.debug_taps set?)");
  give(it->second.p, e->taps.bytes[name], true);
  Q3A_CATCH(e)
}

int32_t q3a_debug_set(const char* key, int32_t value) {
  if (!key) return 1;
  for (const KnobEntry& t : kKnobTable)
    if (strcmp(key, t.key) == 0) { (knobs().*t.field).store(value); return 0; }
  g_last_error = std::string("q3a_debug_set: unknown key '") + key + "'";
  return 1;
}

}  // extern "C"
