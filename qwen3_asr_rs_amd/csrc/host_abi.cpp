// C ABI of the host-only pipeline-shell helpers (include/q3asr.h, "pipeline shell" section).
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../include/q3asr.h"
#include "host.h"
#include "model.h"

namespace q3a {
void set_thread_error(const std::string& msg);  // engine.cpp
}
using namespace q3a;

struct q3a_tokenizer {
  BpeTokenizer tok;
  explicit q3a_tokenizer(const std::string& p) : tok(p) {}
};

#define HOST_TRY try {
#define HOST_CATCH                                   \
  }                                                  \
  catch (const std::exception& ex) {                 \
    set_thread_error(ex.what());                     \
    return 1;                                        \
  }                                                  \
  catch (...) {                                      \
    set_thread_error("unknown error");               \
    return 1;                                        \
  }                                                  \
  return 0;

static int32_t give(const std::vector<float>& v, float** out, int64_t* n) {
  float* p = (float*)malloc(std::max<size_t>(v.size(), 1) * sizeof(float));
  if (!p) fail("out of memory");
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(float));
  *out = p;
  *n = (int64_t)v.size();
  return 0;
}
static int32_t put_str(const std::string& s, char* out, int32_t cap) {
  if (!out || cap <= 0) return 0;
  size_t n = std::min<size_t>(s.size(), (size_t)cap - 1);
  memcpy(out, s.data(), n);
  out[n] = 0;
  return (int32_t)n;
}

// ---- logit bias lists (q3a_parse_logit_bias) ----
namespace {
constexpr long kBiasRangeMax = 1L << 24;  // ids one "lo-hi" item may name (far beyond any vocabulary: a typo, not a list)

std::string trimmed(const std::string& s) {
  size_t a = 0, b = s.size();
  while (a < b && isspace((unsigned char)s[a])) ++a;
  while (b > a && isspace((unsigned char)s[b - 1])) --b;
  return s.substr(a, b - a);
}
// "id" or "lo-hi" (decimal, lo <= hi, both ends included)
void parse_id_range(const std::string& item, const std::string& where, long& lo, long& hi) {
  auto number = [&](const std::string& t) {
    if (t.empty() || t.size() > 10 || t.find_first_not_of("0123456789") != std::string::npos) fail(where + ": '" + item + "' is not an id or a lo-hi range");
    return strtol(t.c_str(), nullptr, 10);
  };
  const size_t dash = item.find('-');
  if (dash == std::string::npos) { lo = hi = number(item); }
  else { lo = number(trimmed(item.substr(0, dash))); hi = number(trimmed(item.substr(dash + 1))); }
  if (lo > hi) fail(where + ": range '" + item + "' runs backwards");
  if (hi > 0x7fffffffL || hi - lo >= kBiasRangeMax) fail(where + ": range '" + item + "' is too large");
}
float parse_bias_value(const std::string& t, const std::string& where) {
  std::string l;
  for (char c : t) l += (char)tolower((unsigned char)c);
  if (l == "-inf" || l == "-infinity") return -INFINITY;
  char* end = nullptr;
  const float v = strtof(t.c_str(), &end);  // (an overflow comes back as +-inf and is refused; an underflow is a tiny bias or 0)
  if (t.empty() || *end || std::isnan(v) || std::isinf(v)) fail(where + ": '" + t + "' is not a finite bias or -inf");
  return v;
}
}  // namespace

extern "C" {

int32_t q3a_parse_logit_bias(const char* text, const char* suppress_list, int32_t* ids, float* bias, int32_t cap, int32_t* n) {
  HOST_TRY
  if (!n || cap < 0 || (cap > 0 && (!ids || !bias))) fail("q3a_parse_logit_bias: bad argument");
  std::set<int32_t> seen;
  int64_t count = 0;
  auto add = [&](long lo, long hi, float v, const std::string& where) {
    for (long id = lo; id <= hi; ++id) {
      if (!seen.insert((int32_t)id).second) fail(where + ": duplicate id " + std::to_string(id));
      if (count < cap) { ids[count] = (int32_t)id; bias[count] = v; }
      ++count;
    }
  };
  const std::string t = text ? text : "";
  int line_no = 0;
  for (size_t pos = 0; pos <= t.size();) {
    size_t nl = t.find('\n', pos);
    if (nl == std::string::npos) nl = t.size();
    std::string line = t.substr(pos, nl - pos);
    pos = nl + 1;
    ++line_no;
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.resize(hash);
    line = trimmed(line);
    if (line.empty()) continue;
    const std::string where = "q3a_parse_logit_bias: line " + std::to_string(line_no);
    const size_t sp = line.find_last_of(" \t");  // "<id or lo-hi> <bias>": the bias is the last field
    if (sp == std::string::npos) fail(where + ": expected '<id> <bias>' or '<lo>-<hi> <bias>'");
    long lo = 0, hi = 0;
    parse_id_range(trimmed(line.substr(0, sp)), where, lo, hi);
    add(lo, hi, parse_bias_value(line.substr(sp + 1), where), where);
  }
  const std::string sl = suppress_list ? suppress_list : "";
  for (size_t pos = 0; !trimmed(sl).empty() && pos <= sl.size();) {
    size_t c = sl.find(',', pos);
    if (c == std::string::npos) c = sl.size();
    const std::string item = trimmed(sl.substr(pos, c - pos));
    pos = c + 1;
    const std::string where = "q3a_parse_logit_bias: suppress list";
    if (item.empty()) fail(where + ": empty item");
    long lo = 0, hi = 0;
    parse_id_range(item, where, lo, hi);
    add(lo, hi, -INFINITY, where);
  }
  if (count > 0x7fffffff) fail("q3a_parse_logit_bias: too many entries");
  *n = (int32_t)count;
  HOST_CATCH
}

// ---- sequence bias lists (q3a_parse_sequence_bias, q3a_hotword_sequences, q3a_banned_sequences) ----
}  // extern "C"
namespace {
constexpr int kSeqMaxLen = 32;  // ids of one entry (q3asr.h "sequence bias")

// entries in the order they first appeared; an equal sequence keeps the larger bias
struct SeqList {
  std::vector<std::vector<int32_t>> seqs;
  std::vector<float> bias;
  void add(const std::vector<int32_t>& q, float b) {
    for (size_t i = 0; i < seqs.size(); ++i)
      if (seqs[i] == q) { bias[i] = std::max(bias[i], b); return; }
    seqs.push_back(q);
    bias.push_back(b);
  }
  // *n_ids / *n = ids and entries needed; written only when both capacities hold everything
  void give(const char* what, int32_t* ids, int32_t ids_cap, int32_t* lens, float* out_bias, int32_t cap, int32_t* n_ids, int32_t* n) const {
    if (!n_ids || !n || ids_cap < 0 || cap < 0 || (ids_cap > 0 && !ids) || (cap > 0 && (!lens || !out_bias))) fail(std::string(what) + ": bad argument");
    size_t total = 0;
    for (const auto& q : seqs) total += q.size();
    if (total > 0x7fffffff || seqs.size() > 0x7fffffff) fail(std::string(what) + ": too many entries");
    *n_ids = (int32_t)total;
    *n = (int32_t)seqs.size();
    if (total > (size_t)ids_cap || seqs.size() > (size_t)cap) return;
    size_t o = 0;
    for (size_t i = 0; i < seqs.size(); ++i) {
      lens[i] = (int32_t)seqs[i].size();
      out_bias[i] = bias[i];
      for (int32_t id : seqs[i]) ids[o++] = id;
    }
  }
};

// both tokenisations of a phrase, encode(phrase) and encode(" " + phrase): a word at the start of the text and one behind a space
std::vector<std::vector<int32_t>> phrase_tokenisations(const char* what, const q3a_tokenizer* t, const char* phrase) {
  const std::string p = trimmed(phrase ? phrase : "");
  if (p.empty()) fail(std::string(what) + ": an empty phrase");
  std::vector<std::vector<int32_t>> out;
  for (const std::string& text : {p, " " + p}) {
    const std::vector<int64_t> v = t->tok.encode(text);
    if (v.empty()) fail(std::string(what) + ": phrase '" + p + "' encodes to no id");
    if ((int)v.size() > kSeqMaxLen) fail(std::string(what) + ": phrase '" + p + "' encodes to " + std::to_string(v.size()) + " ids, more than " + std::to_string(kSeqMaxLen));
    out.emplace_back(v.begin(), v.end());
  }
  return out;
}
}  // namespace
extern "C" {

int32_t q3a_parse_sequence_bias(const char* text, int32_t* ids, int32_t ids_cap, int32_t* lens, float* bias, int32_t cap, int32_t* n_ids, int32_t* n) {
  HOST_TRY
  const char* what = "q3a_parse_sequence_bias";
  SeqList list;
  const std::string t = text ? text : "";
  int line_no = 0;
  for (size_t pos = 0; pos <= t.size();) {
    size_t nl = t.find('\n', pos);
    if (nl == std::string::npos) nl = t.size();
    std::string line = t.substr(pos, nl - pos);
    pos = nl + 1;
    ++line_no;
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.resize(hash);
    line = trimmed(line);
    if (line.empty()) continue;
    const std::string where = std::string(what) + ": line " + std::to_string(line_no);
    std::vector<std::string> fields;  // "<bias> <id> <id> ...": the bias is the first field
    for (size_t a = 0; a < line.size();) {
      while (a < line.size() && isspace((unsigned char)line[a])) ++a;
      size_t b = a;
      while (b < line.size() && !isspace((unsigned char)line[b])) ++b;
      if (b > a) fields.push_back(line.substr(a, b - a));
      a = b;
    }
    if (fields.size() < 2) fail(where + ": expected '<bias> <id> <id> ...'");
    if ((int)fields.size() - 1 > kSeqMaxLen) fail(where + ": " + std::to_string(fields.size() - 1) + " ids, more than " + std::to_string(kSeqMaxLen));
    const float v = parse_bias_value(fields[0], where);
    std::vector<int32_t> q;
    for (size_t i = 1; i < fields.size(); ++i) {
      const std::string& f = fields[i];
      if (f.size() > 10 || f.find_first_not_of("0123456789") != std::string::npos || strtol(f.c_str(), nullptr, 10) > 0x7fffffffL) fail(where + ": '" + f + "' is not an id");
      q.push_back((int32_t)strtol(f.c_str(), nullptr, 10));
    }
    for (const auto& have : list.seqs)
      if (have == q) fail(where + ": the sequence was given on an earlier line");
    list.add(q, v);
  }
  list.give(what, ids, ids_cap, lens, bias, cap, n_ids, n);
  HOST_CATCH
}

int32_t q3a_hotword_sequences(const q3a_tokenizer* t, const char* const* phrases, int32_t n_phrases, float boost, float start_boost, int32_t* ids,
                              int32_t ids_cap, int32_t* lens, float* bias, int32_t cap, int32_t* n_ids, int32_t* n) {
  HOST_TRY
  const char* what = "q3a_hotword_sequences";
  if (!t || n_phrases < 0 || (n_phrases > 0 && !phrases)) fail(std::string(what) + ": bad argument");
  if (!std::isfinite(boost) || !std::isfinite(start_boost)) fail(std::string(what) + ": boost and start_boost must be finite");
  SeqList list;
  for (int i = 0; i < n_phrases; ++i)
    for (const auto& p : phrase_tokenisations(what, t, phrases[i])) {
      if (start_boost != 0.f) list.add({p[0]}, start_boost);
      for (size_t j = 1; j < p.size(); ++j) list.add(std::vector<int32_t>(p.begin(), p.begin() + j + 1), boost);
    }
  list.give(what, ids, ids_cap, lens, bias, cap, n_ids, n);
  HOST_CATCH
}

int32_t q3a_banned_sequences(const q3a_tokenizer* t, const char* const* phrases, int32_t n_phrases, int32_t* ids, int32_t ids_cap, int32_t* lens,
                             float* bias, int32_t cap, int32_t* n_ids, int32_t* n) {
  HOST_TRY
  const char* what = "q3a_banned_sequences";
  if (!t || n_phrases < 0 || (n_phrases > 0 && !phrases)) fail(std::string(what) + ": bad argument");
  SeqList list;
  for (int i = 0; i < n_phrases; ++i)
    for (const auto& p : phrase_tokenisations(what, t, phrases[i])) list.add(p, -INFINITY);
  list.give(what, ids, ids_cap, lens, bias, cap, n_ids, n);
  HOST_CATCH
}

// ---- draft-verified decoding: the draft of the next round (q3asr.h) ----
int32_t q3a_draft_next_round(const int32_t* draft, int32_t n, int32_t k, int32_t tok, int32_t* out, int32_t cap, int32_t* n_out) {
  HOST_TRY
  if (!n_out || n < 0 || k < 0 || k > n || cap < 0 || (n > 0 && !draft) || (cap > 0 && !out)) fail("q3a_draft_next_round: bad argument");
  const bool eos = tok == 151643 || tok == 151645;  // the model stops at k: what stood behind it in the draft is dropped
  int64_t count = 0;
  auto put = [&](int32_t id) { if (count < cap) out[count] = id; ++count; };
  for (int i = 0; i < k; ++i) put(draft[i]);
  if (!eos) {
    put(tok);
    for (int i = k + 1; i < n; ++i) put(draft[i]);
  }
  *n_out = (int32_t)count;
  HOST_CATCH
}

int32_t q3a_load_audio(const char* path, int32_t target_sr, float** samples_out, int64_t* n_out) {
  HOST_TRY
  if (!path || !samples_out || !n_out) fail("null argument");
  give(load_audio(path, target_sr), samples_out, n_out);
  HOST_CATCH
}
int32_t q3a_resample(const float* in, int64_t n, int32_t sr_in, int32_t sr_out, float** samples_out, int64_t* n_out) {
  HOST_TRY
  if (!in || n < 0 || sr_in <= 0 || sr_out <= 0) fail("bad argument");
  std::vector<float> v(in, in + n), o;
  resample_rational(v, sr_in, sr_out, o);
  give(o, samples_out, n_out);
  HOST_CATCH
}
int32_t q3a_resample_rubato(const float* in, int64_t n, int32_t sr_in, int32_t sr_out, float** samples_out, int64_t* n_out) {
  HOST_TRY
  if (!in || n < 0 || sr_in <= 0 || sr_out <= 0) fail("bad argument");
  std::vector<float> v(in, in + n), o;
  resample_rubato_sincfixedin(v, sr_in, sr_out, o);
  give(o, samples_out, n_out);
  HOST_CATCH
}
void q3a_free(void* p) { free(p); }

int32_t q3a_tokenizer_create(const char* path, q3a_tokenizer** out) {
  HOST_TRY
  if (!path || !out) fail("null argument");
  *out = new q3a_tokenizer(path);
  HOST_CATCH
}
void q3a_tokenizer_destroy(q3a_tokenizer* t) { delete t; }

int32_t q3a_tokenizer_decode(const q3a_tokenizer* t, const int32_t* ids, int32_t n, int32_t skip_special, char* out,
                             int32_t cap, int32_t* len) {
  HOST_TRY
  if (!t) fail("null tokenizer");
  std::vector<int64_t> v(ids, ids + n);
  std::string s = t->tok.decode(v, skip_special != 0);
  if (len) *len = (int32_t)s.size();
  put_str(s, out, cap);
  HOST_CATCH
}
int32_t q3a_tokenizer_encode(const q3a_tokenizer* t, const char* text, int32_t* ids, int32_t cap, int32_t* n) {
  HOST_TRY
  if (!t || !text) fail("null argument");
  std::vector<int64_t> v = t->tok.encode(text);
  if (n) *n = (int32_t)v.size();
  for (size_t i = 0; i < v.size() && (int32_t)i < cap; ++i) ids[i] = (int32_t)v[i];
  HOST_CATCH
}

int32_t q3a_parse_asr_output(const char* raw, int32_t language_forced, char* language, int32_t language_cap, char* text,
                             int32_t text_cap) {
  HOST_TRY
  std::string l, t;
  parse_asr_output(raw ? raw : "", language_forced != 0, l, t);
  put_str(l, language, language_cap);
  put_str(t, text, text_cap);
  HOST_CATCH
}
int32_t q3a_normalize_nfc(const char* utf8, char* out, int32_t cap, int32_t* len) {
  HOST_TRY
  const std::string r = normalize_nfc(utf8 ? utf8 : "");
  if (len) *len = (int32_t)r.size();
  put_str(r, out, cap);
  HOST_CATCH
}
int32_t q3a_capitalize_first(const char* s, char* out, int32_t cap) {
  HOST_TRY
  put_str(capitalize_first(s ? s : ""), out, cap);
  HOST_CATCH
}

}  // extern "C"
