// `asr <model_path> <audio_file> [language]` -- the reference's CLI (src/main.rs:7-81) on top of libq3asr_hip.so.
// Same argv contract, same usage text on stderr + exit status 1, same stdout ("Language: ...\nText: ...").
// Logging: RUST_LOG=info|debug (default info) prints the reference's progress lines to stderr
// (src/inference.rs:31-103,203-205).  Input: WAV files (the FFmpeg path of src/audio.rs is out of scope).
// Q3A_TOKEN_LOGPROBS=1 adds one stdout line after "Text:": "Confidence: avg_logprob <mean token log-probability>
// min_token_prob <smallest token probability>" (q3a_fetch_logprobs); without it stdout and stderr are unchanged.
// Q3A_ALIGNER=<forced-aligner model dir> aligns the transcript just produced to the audio (q3a_align_batch_ptrs) and adds one stdout
// line per word after those: "Word: <start s> <end s> <word>"; without it nothing is printed and no aligner is loaded.
// Q3A_SCORE_TEXT=<path of a UTF-8 file> with a `language` argument scores that transcript of the audio (q3a_score_batch_ptrs on the
// ids of "<asr_text>" + text + <|im_end|>, the language prefix in the prompt) after the lines above and adds "Score: avg_logprob <mean
// token log-probability> min_token_prob <smallest token probability> tokens <n> disagree <rows whose argmax is another id>"; without it
// nothing changes.
// Q3A_BEAM=<W> runs a beam search of width W (q3a_beam_search_batch_ptrs; 1..8) over the same audio and prompt after "Text:" (and
// "Confidence:") and adds one stdout line per hypothesis, best first: "Hyp <k>: <score> <text>"; without it nothing changes.
// Q3A_SUPPRESS_TOKENS=<id,lo-hi,...> and Q3A_LOGIT_BIAS=<path of a file of "id bias" / "lo-hi bias" lines> constrain the decoding
// (q3a_parse_logit_bias + q3a_set_logit_bias, default bias 0): the transcription and a Q3A_BEAM search run under the bias, a
// Q3A_SCORE_TEXT score does not; without them nothing changes.
// Q3A_TEMPERATURE=<T> [Q3A_MIN_P=<p>] [Q3A_SEED=<n>] samples the transcription at ONE temperature (q3a_set_sampling; min_p 0 and seed
// 0 when absent); a Q3A_BEAM search is then refused by the engine.  There is no temperature fallback here (no zlib).
// Q3A_TOP_K=<k> and / or Q3A_TOP_P=<p> with Q3A_TEMPERATURE filter the sampled step (q3a_set_sampling_filter; 0 and 1 when absent);
// without a Q3A_TEMPERATURE > 0 they are an error: nothing is sampled.
// Q3A_REPETITION_PENALTY=<p> and / or Q3A_NO_REPEAT_NGRAM=<n> run the transcription under q3a_set_repetition (1 and 0 when absent); a
// Q3A_BEAM search is then refused by the engine, a Q3A_SCORE_TEXT score never sees it.
// Q3A_DRAFT_TEXT=<path of a UTF-8 file> with a `language` argument transcribes with that text as a draft (q3a_transcribe_draft_batch_ptrs:
// the ids of "<asr_text>" + text, as Q3A_SCORE_TEXT reads a transcript): the same "Language:" / "Text:" lines as without it, then
// "Accepted: <k> / <n>" -- the leading draft ids the greedy loop would have written itself, of the n the draft has.  Q3A_DRAFT_ROUNDS=<r>
// (default 1) allows further verification rounds.  The engine refuses it together with Q3A_TEMPERATURE / Q3A_REPETITION_PENALTY /
// Q3A_NO_REPEAT_NGRAM.
// Q3A_HOTWORDS=<path of a file, one phrase per line> with Q3A_HOTWORD_BOOST=<b> (required: no value has been tuned on real weights) and
// optionally Q3A_HOTWORD_START_BOOST=<b> boosts those phrases (q3a_hotword_sequences); Q3A_BANNED_PHRASES=<path, one phrase per line>
// never writes them (q3a_banned_sequences); Q3A_SEQUENCE_BIAS=<path of a file of "bias id id ..." lines> gives entries as ids
// (q3a_parse_sequence_bias).  The three are concatenated in that order (a sequence named twice keeps the larger bias) and set with
// q3a_set_sequence_bias before anything is generated; the engine then refuses a Q3A_BEAM search and Q3A_DRAFT_TEXT, a
// Q3A_SCORE_TEXT score never sees it.  '#' starts a comment in the phrase files too; without the variables nothing changes.
// Q3A_TOP_LOGPROBS=<n> (1..20) records the n best candidates of every generated token (q3a_set_top_logprobs / q3a_fetch_top_logprobs)
// and adds, after all the lines above, one stdout line per generated token: "Top <t>: <token text> | <candidate text> <probability> |
// ..." with the n candidates best first (control characters, backslash and '|' escaped in the texts).  The setting is taken back before a Q3A_BEAM search, which
// the engine refuses under it, as it refuses Q3A_DRAFT_TEXT.  Without the variable stdout and stderr are unchanged.
#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/q3asr.h"

static int g_level = 1;  // 0 warn, 1 info, 2 debug
static void logf(int level, const char* fmt, const std::string& a = "") {
  if (level > g_level) return;
  fprintf(stderr, "%s ", level == 2 ? "DEBUG" : " INFO");
  fprintf(stderr, fmt, a.c_str());
  fputc('\n', stderr);
}
static bool exists(const char* p) { struct stat st; return stat(p, &st) == 0; }
static int die(const std::string& msg) { fprintf(stderr, "Error: %s\n", msg.c_str()); return 1; }

// Q3A_SUPPRESS_TOKENS / Q3A_LOGIT_BIAS: the engine's logit bias, set before anything is generated
static int set_logit_bias_from_env(q3a_engine* eng) {
  const char* list = getenv("Q3A_SUPPRESS_TOKENS");
  const char* path = getenv("Q3A_LOGIT_BIAS");
  if ((!list || !*list) && (!path || !*path)) return 0;
  std::string text;
  if (path && *path) {
    FILE* f = fopen(path, "rb");
    if (!f) return die(std::string("Logit bias failed: cannot read ") + path);
    char buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) text.append(buf, k);
    fclose(f);
  }
  int32_t n = 0;
  if (q3a_parse_logit_bias(text.c_str(), list, nullptr, nullptr, 0, &n) != 0) return die(std::string("Logit bias failed: ") + q3a_last_error(nullptr));
  std::vector<int32_t> ids((size_t)n + 1);
  std::vector<float> bias((size_t)n + 1);
  if (q3a_parse_logit_bias(text.c_str(), list, ids.data(), bias.data(), n, &n) != 0) return die(std::string("Logit bias failed: ") + q3a_last_error(nullptr));
  if (q3a_set_logit_bias(eng, ids.data(), bias.data(), n, 0.f) != 0) return die(std::string("Logit bias failed: ") + q3a_last_error(eng));
  logf(1, "Logit bias: %s entries", std::to_string(n));
  return 0;
}

// Q3A_TEMPERATURE / Q3A_MIN_P / Q3A_SEED: the engine's sampling setting, set before anything is generated
static int set_sampling_from_env(q3a_engine* eng) {
  const char* t = getenv("Q3A_TEMPERATURE");
  if (!t || !*t) return 0;
  const char *p = getenv("Q3A_MIN_P"), *sd = getenv("Q3A_SEED");
  char* end = nullptr;
  const float temperature = strtof(t, &end);
  if (end == t || *end) return die(std::string("Sampling failed: Q3A_TEMPERATURE is not a number: ") + t);
  float min_p = 0.f;
  if (p && *p) {
    min_p = strtof(p, &end);
    if (end == p || *end) return die(std::string("Sampling failed: Q3A_MIN_P is not a number: ") + p);
  }
  unsigned long long seed = 0;
  if (sd && *sd) {
    seed = strtoull(sd, &end, 10);
    if (end == sd || *end || *sd == '-') return die(std::string("Sampling failed: Q3A_SEED is not an unsigned integer: ") + sd);
  }
  if (q3a_set_sampling(eng, temperature, min_p, (uint64_t)seed) != 0) return die(std::string("Sampling failed: ") + q3a_last_error(eng));
  logf(1, "Sampling: temperature %s", t);
  return 0;
}

// Q3A_TOP_K / Q3A_TOP_P: the sampled step's top-k / top-p filter, set before anything is generated
static int set_sampling_filter_from_env(q3a_engine* eng) {
  const char *k = getenv("Q3A_TOP_K"), *p = getenv("Q3A_TOP_P"), *t = getenv("Q3A_TEMPERATURE");
  const bool have_k = k && *k, have_p = p && *p;
  if (!have_k && !have_p) return 0;
  char* end = nullptr;
  if (!t || !*t || !(strtof(t, &end) > 0.f)) return die("Sampling filter failed: Q3A_TOP_K / Q3A_TOP_P need a Q3A_TEMPERATURE > 0 (nothing is sampled without it)");
  long top_k = 0;
  if (have_k) {
    top_k = strtol(k, &end, 10);
    if (end == k || *end || top_k < 0 || top_k > 0x7fffffffL) return die(std::string("Sampling filter failed: Q3A_TOP_K is not an integer >= 0: ") + k);
  }
  float top_p = 1.f;
  if (have_p) {
    top_p = strtof(p, &end);
    if (end == p || *end) return die(std::string("Sampling filter failed: Q3A_TOP_P is not a number: ") + p);
  }
  if (q3a_set_sampling_filter(eng, (int32_t)top_k, top_p) != 0) return die(std::string("Sampling filter failed: ") + q3a_last_error(eng));
  logf(1, "Sampling filter: top_k %s", std::to_string(top_k) + " top_p " + std::to_string(top_p));
  return 0;
}

// Q3A_REPETITION_PENALTY / Q3A_NO_REPEAT_NGRAM: the engine's repetition setting, set before anything is generated
static int set_repetition_from_env(q3a_engine* eng) {
  const char *p = getenv("Q3A_REPETITION_PENALTY"), *n = getenv("Q3A_NO_REPEAT_NGRAM");
  const bool have_p = p && *p, have_n = n && *n;
  if (!have_p && !have_n) return 0;
  char* end = nullptr;
  float penalty = 1.f;
  if (have_p) {
    penalty = strtof(p, &end);
    if (end == p || *end) return die(std::string("Repetition control failed: Q3A_REPETITION_PENALTY is not a number: ") + p);
  }
  long ngram = 0;
  if (have_n) {
    ngram = strtol(n, &end, 10);
    if (end == n || *end || ngram < -1000 || ngram > 1000) return die(std::string("Repetition control failed: Q3A_NO_REPEAT_NGRAM is not an integer: ") + n);
  }
  if (q3a_set_repetition(eng, penalty, (int32_t)ngram) != 0) return die(std::string("Repetition control failed: ") + q3a_last_error(eng));
  logf(1, "Repetition control: penalty %s", have_p ? p : "1");
  logf(1, "Repetition control: no-repeat n-gram %s", have_n ? n : "0");
  return 0;
}

// Q3A_TOP_LOGPROBS: n, or 0 without the variable; -1 after an error was reported
static int top_logprobs_from_env(q3a_engine* eng) {
  const char* v = getenv("Q3A_TOP_LOGPROBS");
  if (!v || !*v) return 0;
  char* end = nullptr;
  const long n = strtol(v, &end, 10);
  if (end == v || *end || n < -1000 || n > 1000) { die(std::string("Top log-probabilities failed: Q3A_TOP_LOGPROBS is not an integer: ") + v); return -1; }
  if (q3a_set_top_logprobs(eng, (int32_t)n) != 0) { die(std::string("Top log-probabilities failed: ") + q3a_last_error(eng)); return -1; }
  return (int)n;
}
// one token's text for a line of its own: printable as it is, the rest escaped
static std::string token_text(q3a_tokenizer* tok, int32_t id) {
  int32_t need = 0;
  q3a_tokenizer_decode(tok, &id, 1, 0, nullptr, 0, &need);
  std::string s((size_t)need + 1, '\0');
  q3a_tokenizer_decode(tok, &id, 1, 0, &s[0], need + 1, &need);
  s.resize((size_t)need);
  std::string out;
  for (unsigned char c : s) {
    if (c == '\n') out += "\\n";
    else if (c == '\r') out += "\\r";
    else if (c == '\t') out += "\\t";
    else if (c == '\\') out += "\\\\";
    else if (c == '|') out += "\\|";
    else if (c < 0x20) { char b[8]; snprintf(b, sizeof(b), "\\x%02x", c); out += b; }
    else out += (char)c;
  }
  return out;
}

static bool read_file(const char* path, std::string& text) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  char buf[4096];
  for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) text.append(buf, k);
  fclose(f);
  return true;
}

// Q3A_HOTWORDS (+ Q3A_HOTWORD_BOOST, Q3A_HOTWORD_START_BOOST) / Q3A_BANNED_PHRASES / Q3A_SEQUENCE_BIAS: the engine's sequence bias,
// set before anything is generated
static int set_sequence_bias_from_env(q3a_engine* eng, q3a_tokenizer* tok) {
  const char *hot = getenv("Q3A_HOTWORDS"), *ban = getenv("Q3A_BANNED_PHRASES"), *file = getenv("Q3A_SEQUENCE_BIAS");
  const char *boost_s = getenv("Q3A_HOTWORD_BOOST"), *start_s = getenv("Q3A_HOTWORD_START_BOOST");
  const bool have_hot = hot && *hot, have_ban = ban && *ban, have_file = file && *file;
  if (!have_hot && !have_ban && !have_file) return 0;
  const std::string what = "Sequence bias failed: ";
  std::vector<std::vector<int32_t>> seqs;
  std::vector<float> biases;
  // one of the three list helpers, sized by a first call without room, appended (an equal sequence keeps the larger bias)
  auto take = [&](auto&& call) -> int {
    int32_t n_ids = 0, n = 0;
    if (call(nullptr, 0, nullptr, nullptr, 0, &n_ids, &n) != 0) return die(what + q3a_last_error(nullptr));
    std::vector<int32_t> ids((size_t)n_ids + 1), lens((size_t)n + 1);
    std::vector<float> bias((size_t)n + 1);
    if (call(ids.data(), n_ids, lens.data(), bias.data(), n, &n_ids, &n) != 0) return die(what + q3a_last_error(nullptr));
    for (int32_t k = 0, o = 0; k < n; o += lens[k++]) {
      const std::vector<int32_t> q(ids.begin() + o, ids.begin() + o + lens[k]);
      const auto it = std::find(seqs.begin(), seqs.end(), q);
      if (it != seqs.end()) { float& b = biases[(size_t)(it - seqs.begin())]; b = std::max(b, bias[k]); }
      else { seqs.push_back(q); biases.push_back(bias[k]); }
    }
    return 0;
  };
  // the phrases of a file: one per line, '#' comments and blank lines dropped
  auto phrases_of = [&](const char* path, std::vector<std::string>& out) -> int {
    std::string text;
    if (!read_file(path, text)) return die(what + "cannot read " + path);
    for (size_t pos = 0; pos <= text.size();) {
      size_t nl = text.find('\n', pos);
      if (nl == std::string::npos) nl = text.size();
      std::string line = text.substr(pos, nl - pos);
      pos = nl + 1;
      const size_t hash = line.find('#');
      if (hash != std::string::npos) line.resize(hash);
      while (!line.empty() && isspace((unsigned char)line.back())) line.pop_back();
      size_t a = 0;
      while (a < line.size() && isspace((unsigned char)line[a])) ++a;
      if (a < line.size()) out.push_back(line.substr(a));
    }
    return 0;
  };
  auto number = [&](const char* name, const char* v, float& out) -> int {
    char* end = nullptr;
    out = strtof(v, &end);
    if (end == v || *end) return die(what + name + " is not a number: " + v);
    return 0;
  };
  if (have_hot) {
    if (!boost_s || !*boost_s) return die(what + "Q3A_HOTWORDS needs Q3A_HOTWORD_BOOST (no default: no value has been tuned on real weights)");
    float boost = 0.f, start = 0.f;
    if (number("Q3A_HOTWORD_BOOST", boost_s, boost) != 0) return 1;
    if (start_s && *start_s && number("Q3A_HOTWORD_START_BOOST", start_s, start) != 0) return 1;
    std::vector<std::string> ph;
    if (phrases_of(hot, ph) != 0) return 1;
    std::vector<const char*> pp;
    for (auto& x : ph) pp.push_back(x.c_str());
    pp.push_back(nullptr);
    const int32_t np = (int32_t)ph.size();
    if (take([&](int32_t* ids, int32_t ic, int32_t* lens, float* bias, int32_t cap, int32_t* n_ids, int32_t* n) {
          return q3a_hotword_sequences(tok, pp.data(), np, boost, start, ids, ic, lens, bias, cap, n_ids, n); }) != 0) return 1;
  }
  if (have_ban) {
    std::vector<std::string> ph;
    if (phrases_of(ban, ph) != 0) return 1;
    std::vector<const char*> pp;
    for (auto& x : ph) pp.push_back(x.c_str());
    pp.push_back(nullptr);
    const int32_t np = (int32_t)ph.size();
    if (take([&](int32_t* ids, int32_t ic, int32_t* lens, float* bias, int32_t cap, int32_t* n_ids, int32_t* n) {
          return q3a_banned_sequences(tok, pp.data(), np, ids, ic, lens, bias, cap, n_ids, n); }) != 0) return 1;
  }
  if (have_file) {
    std::string text;
    if (!read_file(file, text)) return die(what + "cannot read " + file);
    if (take([&](int32_t* ids, int32_t ic, int32_t* lens, float* bias, int32_t cap, int32_t* n_ids, int32_t* n) {
          return q3a_parse_sequence_bias(text.c_str(), ids, ic, lens, bias, cap, n_ids, n); }) != 0) return 1;
  }
  std::vector<int32_t> ids, lens;
  for (const auto& q : seqs) { ids.insert(ids.end(), q.begin(), q.end()); lens.push_back((int32_t)q.size()); }
  ids.push_back(0); lens.push_back(0); biases.push_back(0.f);  // (never read: valid pointers for an empty list)
  if (q3a_set_sequence_bias(eng, ids.data(), lens.data(), biases.data(), (int32_t)seqs.size()) != 0) return die(what + q3a_last_error(eng));
  logf(1, "Sequence bias: %s entries", std::to_string(seqs.size()));
  return 0;
}

// Q3A_ALIGNER: word times of `text` in the audio (the forced aligner's word split, prompt, head and monotonicity fix-up)
static int print_word_times(const char* aligner_dir, const float* pcm, int64_t n, const char* text, const char* language) {
  int32_t nw = 0, need = 0;
  if (q3a_split_words_for_alignment(text, language, nullptr, 0, &nw, &need) != 0)
    return die(std::string("Alignment failed: ") + q3a_last_error(nullptr));
  std::string joined((size_t)need + 1, '\0');
  q3a_split_words_for_alignment(text, language, &joined[0], need + 1, &nw, &need);
  joined.resize((size_t)need);
  std::vector<std::string> words;
  for (size_t b = 0; nw > 0 && b <= joined.size();) {
    size_t e = joined.find('\n', b);
    if (e == std::string::npos) e = joined.size();
    words.push_back(joined.substr(b, e - b));
    b = e + 1;
  }
  logf(1, "Loading forced aligner from \"%s\"", aligner_dir);
  q3a_opts opts;
  q3a_opts_default(&opts);
  q3a_engine* al = nullptr;
  if (q3a_engine_create(aligner_dir, 0, &opts, &al) != 0) return die(std::string("Failed to load aligner: ") + q3a_last_error(nullptr));
  q3a_tokenizer* atok = nullptr;
  const std::string tj = std::string(aligner_dir) + "/tokenizer.json";
  if (q3a_tokenizer_create(tj.c_str(), &atok) != 0) {
    std::string m = q3a_last_error(nullptr);
    q3a_engine_destroy(al);
    return die("Failed to load aligner tokenizer: " + m);
  }
  int32_t classify_num = 0, ts_id = 0;
  float seg_ms = 0.f;
  q3a_aligner_info(al, &classify_num, &ts_id, &seg_ms);
  std::vector<const char*> wp;
  for (auto& w : words) wp.push_back(w.c_str());
  int32_t nt = 0;
  int rc = 0;
  std::vector<int32_t> tids;
  std::vector<int32_t> classes((size_t)2 * words.size() + 1);
  int32_t count = 0;
  if (q3a_align_text_ids(atok, wp.data(), (int32_t)wp.size(), ts_id, nullptr, 0, &nt) != 0) {
    rc = die(std::string("Alignment failed: ") + q3a_last_error(nullptr));
  } else {
    tids.resize((size_t)nt + 1);
    q3a_align_text_ids(atok, wp.data(), (int32_t)wp.size(), ts_id, tids.data(), nt, &nt);
    const float* ptrs[1] = {pcm};
    if (q3a_align_batch_ptrs(al, ptrs, &n, 1, tids.data(), &nt, classes.data(), (int32_t)classes.size(), &count) != 0)
      rc = die(std::string("Alignment failed: ") + q3a_last_error(al));
  }
  if (rc == 0) {
    std::vector<float> ms((size_t)count + 1);
    for (int32_t i = 0; i < count; ++i) ms[i] = (float)classes[i] * seg_ms;
    q3a_fix_timestamps(ms.data(), count, ms.data());
    for (size_t w = 0; w < words.size() && 2 * w + 1 < (size_t)count; ++w)
      printf("Word: %.3f %.3f %s\n", ms[2 * w] / 1000.0, ms[2 * w + 1] / 1000.0, words[w].c_str());
  }
  q3a_tokenizer_destroy(atok);
  q3a_engine_destroy(al);
  return rc;
}

// the ids of "<asr_text>" + the text in `path` (trailing line ends dropped): how Q3A_SCORE_TEXT and Q3A_DRAFT_TEXT read a transcript
static int transcript_ids(q3a_tokenizer* tok, const char* path, const char* what, std::vector<int32_t>& ids) {
  FILE* f = fopen(path, "rb");
  if (!f) return die(std::string(what) + " failed: cannot read " + path);
  std::string text;
  char buf[4096];
  for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) text.append(buf, got);
  fclose(f);
  while (!text.empty() && (text.back() == '\n' || text.back() == '\r')) text.pop_back();
  const std::string full = "<asr_text>" + text;
  int32_t nt = 0;
  ids.assign(full.size() + 8, 0);
  if (q3a_tokenizer_encode(tok, full.c_str(), ids.data(), (int32_t)ids.size(), &nt) != 0)
    return die(std::string(what) + " failed: " + q3a_last_error(nullptr));
  ids.resize((size_t)nt);
  return 0;
}

// Q3A_SCORE_TEXT: the log-probability the model gives the transcript in `path`, token by token, in one prefill
static int print_score(q3a_engine* eng, q3a_tokenizer* tok, const float* pcm, int64_t n, const std::vector<int32_t>& prefix, const char* path) {
  std::vector<int32_t> ids;
  if (transcript_ids(tok, path, "Scoring", ids) != 0) return 1;
  ids.push_back(151645);  // <|im_end|>: "the transcript stops here" is scored too
  int32_t nt = (int32_t)ids.size();
  std::vector<float> lp((size_t)nt), top_lp((size_t)nt);
  std::vector<int32_t> top((size_t)nt);
  const float* ptrs[1] = {pcm};
  if (q3a_score_batch_ptrs(eng, ptrs, &n, 1, prefix.data(), (int32_t)prefix.size(), ids.data(), &nt, lp.data(), top.data(), top_lp.data(), nt) != 0)
    return die(std::string("Scoring failed: ") + q3a_last_error(eng));
  double sum = 0.0;
  float mn = INFINITY;
  int disagree = 0;
  for (int32_t i = 0; i < nt; ++i) { sum += lp[i]; mn = std::min(mn, lp[i]); disagree += top[i] != ids[i]; }
  printf("Score: avg_logprob %.6f min_token_prob %.6f tokens %d disagree %d\n", sum / (double)nt, std::exp((double)mn), nt, disagree);
  return 0;
}

// Q3A_BEAM=<W>: a beam search of width W over the same audio and prompt; one `Hyp k: <score> <text>` line per hypothesis, best first
// (score = the sum of the tokens' natural-log probabilities, the EOS's included when the hypothesis finished).
static int print_beam(q3a_engine* eng, q3a_tokenizer* tok, const float* pcm, int64_t n, const std::vector<int32_t>& prefix, int width,
                      int32_t max_new, bool language_forced) {
  if (width < 1) return die("Beam search failed: Q3A_BEAM must be a width of 1..8");  // (the engine refuses more than 8 itself)
  std::vector<int32_t> ids((size_t)width * max_new), lens((size_t)width);
  std::vector<float> scores((size_t)width);
  std::vector<uint8_t> fin((size_t)width);
  const float* ptrs[1] = {pcm};
  if (q3a_beam_search_batch_ptrs(eng, ptrs, &n, 1, prefix.empty() ? nullptr : prefix.data(), (int32_t)prefix.size(), width, max_new, ids.data(),
                                 max_new, lens.data(), scores.data(), fin.data(), nullptr) != 0)
    return die(std::string("Beam search failed: ") + q3a_last_error(eng));
  for (int k = 0; k < width; ++k) {
    if (std::isinf(scores[k]) && lens[k] == 0) continue;  // an empty slot
    const int32_t* hyp = ids.data() + (size_t)k * max_new;
    int32_t need = 0;
    q3a_tokenizer_decode(tok, hyp, lens[k], 1, nullptr, 0, &need);
    std::string raw((size_t)need + 1, '\0');
    q3a_tokenizer_decode(tok, hyp, lens[k], 1, &raw[0], need + 1, &need);
    raw.resize((size_t)need);
    std::vector<char> lang(256), text(raw.size() + 16);
    q3a_parse_asr_output(raw.c_str(), language_forced, lang.data(), (int32_t)lang.size(), text.data(), (int32_t)text.size());
    printf("Hyp %d: %.6f %s\n", k, scores[k], text.data());
  }
  return 0;
}

int main(int argc, char** argv) {
  if (const char* rl = getenv("RUST_LOG")) {
    if (strstr(rl, "debug") || strstr(rl, "trace")) g_level = 2;
    else if (strstr(rl, "warn") || strstr(rl, "error") || strstr(rl, "off")) g_level = 0;
  }
  if (argc < 3) {  // main.rs:18-35
    fprintf(stderr, "Qwen3 ASR - Automatic Speech Recognition\n\n");
    fprintf(stderr, "Usage: asr <model_path> <audio_file> [language]\n\n");
    fprintf(stderr, "Arguments:\n");
    fprintf(stderr, "  model_path   Path to the Qwen3-ASR model directory\n");
    fprintf(stderr, "  audio_file   Path to the input audio file (WAV; PCM 8/16/24/32-bit or float32)\n");
    fprintf(stderr, "  language     Optional: force language (e.g., chinese, english, japanese)\n\n");
    fprintf(stderr, "The audio file will be automatically converted to mono 16kHz f32 for the model.\n\n");
    fprintf(stderr, "Environment variables:\n");
    fprintf(stderr, "  RUST_LOG     Set logging level (e.g., info, debug, trace)\n");
    return 1;
  }
  const char* model_path = argv[1];
  const char* audio_file = argv[2];
  const char* language = argc > 3 ? argv[3] : nullptr;
  if (!exists(model_path)) return die(std::string("Model directory not found: ") + model_path);  // main.rs:43-45
  if (!exists(audio_file)) return die(std::string("Audio file not found: ") + audio_file);       // main.rs:46-48

  const int n_dev = q3a_device_count();  // main.rs:51-65
  if (n_dev <= 0) return die("No HIP device available (libq3asr_hip has no CPU path)");
  logf(1, "Using HIP device 0 of %s (MI355X / gfx950)", std::to_string(n_dev));
  logf(1, "Loading model from \"%s\"", model_path);
  q3a_opts opts;
  q3a_opts_default(&opts);
  const char* lp_env = getenv("Q3A_TOKEN_LOGPROBS");
  const bool want_lp = lp_env && atoi(lp_env) != 0;
  opts.token_logprobs = want_lp ? 1 : 0;
  q3a_engine* eng = nullptr;
  if (q3a_engine_create(model_path, 0, &opts, &eng) != 0) return die(std::string("Failed to load model: ") + q3a_last_error(nullptr));
  if (q3a_weights_rounded(eng))
    logf(0, "warning: the checkpoint stores F16/F32 matrices; the HIP backend keeps matrices as bf16 (rounded to nearest-even)");
  if (set_logit_bias_from_env(eng) != 0) return 1;
  if (set_sampling_from_env(eng) != 0) return 1;
  if (set_sampling_filter_from_env(eng) != 0) return 1;
  if (set_repetition_from_env(eng) != 0) return 1;
  const int top_n = top_logprobs_from_env(eng);
  if (top_n < 0) return 1;
  logf(1, "Loading tokenizer...");
  q3a_tokenizer* tok = nullptr;
  const std::string tj = std::string(model_path) + "/tokenizer.json";
  if (q3a_tokenizer_create(tj.c_str(), &tok) != 0) {  // tokenizer.rs:19-29
    std::string m = q3a_last_error(nullptr);
    q3a_engine_destroy(eng);
    return die("Failed to load tokenizer: " + m);
  }
  if (set_sequence_bias_from_env(eng, tok) != 0) return 1;
  logf(1, "Model loaded successfully");

  logf(1, "Transcribing: %s", audio_file);
  logf(1, "Loading audio from %s", audio_file);
  float* pcm = nullptr;
  int64_t n = 0;
  if (q3a_load_audio(audio_file, 16000, &pcm, &n) != 0) return die(std::string("Transcription failed: ") + q3a_last_error(nullptr));

  std::vector<int32_t> prefix;
  if (language) {  // inference.rs:246-251
    char cap[256];
    q3a_capitalize_first(language, cap, sizeof(cap));
    const std::string text = std::string("language ") + cap;
    int32_t np = 0;
    prefix.resize(64);
    if (q3a_tokenizer_encode(tok, text.c_str(), prefix.data(), (int32_t)prefix.size(), &np) != 0)
      return die(std::string("Transcription failed: ") + q3a_last_error(nullptr));
    prefix.resize((size_t)np);
  }
  const int32_t max_new = 4096;  // inference.rs:153
  std::vector<int32_t> ids((size_t)max_new);
  int32_t len = 0;
  const char* draft_path = getenv("Q3A_DRAFT_TEXT");
  const bool with_draft = draft_path && *draft_path;
  int32_t accepted = 0, n_draft = 0;
  if (with_draft) {
    if (!language) return die("Draft failed: Q3A_DRAFT_TEXT needs the language argument (the ids after a free-running prompt start with the language the model detects)");
    std::vector<int32_t> draft;
    if (transcript_ids(tok, draft_path, "Draft", draft) != 0) return 1;
    n_draft = (int32_t)draft.size();
    const char* rounds_env = getenv("Q3A_DRAFT_ROUNDS");
    const int rounds = rounds_env && atoi(rounds_env) > 0 ? atoi(rounds_env) : 1;
    const float* ptrs[1] = {pcm};
    draft.push_back(0);  // (never read: a valid pointer for an empty draft)
    if (q3a_transcribe_draft_batch_ptrs(eng, ptrs, &n, 1, prefix.data(), (int32_t)prefix.size(), draft.data(), &n_draft, max_new, rounds, 5 /* the one-clip break-even, DESIGN.md section 3.13 */,
                                        ids.data(), max_new, &len, &accepted) != 0)
      return die(std::string("Draft failed: ") + q3a_last_error(eng));
  } else if (q3a_transcribe_batch(eng, pcm, &n, 1, prefix.empty() ? nullptr : prefix.data(), (int32_t)prefix.size(), max_new, 0,
                                  ids.data(), max_new, &len) != 0)
    return die(std::string("Transcription failed: ") + q3a_last_error(eng));
  std::vector<float> lps;
  if (want_lp) {
    lps.resize((size_t)max_new);
    int32_t lp_len = 0;
    if (q3a_fetch_logprobs(eng, lps.data(), max_new, &lp_len) != 0)
      return die(std::string("Transcription failed: ") + q3a_last_error(eng));
    lps.resize((size_t)lp_len);
  }
  std::vector<int32_t> top_ids;
  std::vector<float> top_lp;
  if (top_n > 0) {  // read now, printed last: what follows may run the engine again
    top_ids.resize((size_t)max_new * top_n);
    top_lp.resize((size_t)max_new * top_n);
    int32_t top_len = 0;
    if (q3a_fetch_top_logprobs(eng, top_ids.data(), top_lp.data(), max_new, top_n, &top_len) != 0)
      return die(std::string("Top log-probabilities failed: ") + q3a_last_error(eng));
    if (q3a_set_top_logprobs(eng, 0) != 0) return die(std::string("Top log-probabilities failed: ") + q3a_last_error(eng));
  }
  q3a_timings tm;
  q3a_stage_timings(eng, &tm);
  if (g_level >= 1) {
    fprintf(stderr, " INFO Mel spectrogram: %lld frames\n", (long long)q3a_num_frames(n));
    fprintf(stderr, " INFO Audio encoder: %d tokens\n", tm.total_audio_tokens);
    fprintf(stderr, " INFO Generated %d tokens\n", len);
    fprintf(stderr, " INFO timings: mel %.2f ms, encoder %.2f ms, prefill %.2f ms, decode %.2f ms\n", tm.mel_ms, tm.encoder_ms,
            tm.prefill_ms, tm.decode_ms);
  }
  int32_t need = 0;
  q3a_tokenizer_decode(tok, ids.data(), len, 1, nullptr, 0, &need);
  std::string raw((size_t)need + 1, '\0');
  q3a_tokenizer_decode(tok, ids.data(), len, 1, &raw[0], need + 1, &need);
  raw.resize((size_t)need);
  if (g_level >= 2) fprintf(stderr, "DEBUG Raw output: \"%s\"\n", raw.c_str());
  std::vector<char> lang(256), text(raw.size() + 16);
  q3a_parse_asr_output(raw.c_str(), language != nullptr, lang.data(), (int32_t)lang.size(), text.data(), (int32_t)text.size());
  printf("Language: %s\n", lang.data());  // main.rs:77-78
  printf("Text: %s\n", text.data());
  if (want_lp) {  // mean over the generated tokens (Whisper's avg_logprob) and the least likely token
    double sum = 0.0;
    float mn = INFINITY;
    for (float v : lps) { sum += v; mn = std::min(mn, v); }
    const double avg = lps.empty() ? NAN : sum / (double)lps.size();
    printf("Confidence: avg_logprob %.6f min_token_prob %.6f\n", avg, lps.empty() ? NAN : std::exp((double)mn));
  }
  if (with_draft) printf("Accepted: %d / %d\n", accepted, n_draft);
  int rc = 0;
  const char* beam_env = getenv("Q3A_BEAM");
  if (beam_env && *beam_env) rc = print_beam(eng, tok, pcm, n, prefix, atoi(beam_env), max_new, language != nullptr);
  const char* score_path = getenv("Q3A_SCORE_TEXT");
  if (rc == 0 && score_path && *score_path && language) rc = print_score(eng, tok, pcm, n, prefix, score_path);
  const char* aligner_dir = getenv("Q3A_ALIGNER");
  if (rc == 0 && aligner_dir && *aligner_dir) rc = print_word_times(aligner_dir, pcm, n, text.data(), language);
  if (rc == 0 && top_n > 0) {
    for (int32_t t = 0; t < len; ++t) {
      std::string line = "Top " + std::to_string(t) + ": " + token_text(tok, ids[(size_t)t]);
      for (int k = 0; k < top_n; ++k) {
        char pr[32];
        snprintf(pr, sizeof(pr), " %.6f", std::exp((double)top_lp[(size_t)t * top_n + k]));
        line += " | " + token_text(tok, top_ids[(size_t)t * top_n + k]) + pr;
      }
      printf("%s\n", line.c_str());
    }
  }
  q3a_free(pcm);
  q3a_tokenizer_destroy(tok);
  q3a_engine_destroy(eng);
  return rc;
}
