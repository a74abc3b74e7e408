// Host side of the forced aligner (include/q3asr.h "forced aligner"): the prompt layout, the word split and the monotonicity
// fix-up of the original Qwen3-ForcedAligner (HF transformers: Qwen3ASRProcessor.split_words_for_alignment, _fix_timestamps).
// Pure C++, no HIP.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/q3asr.h"
#include "host.h"
#include "model.h"
#include "unicode_tables.h"

namespace q3a {
void set_thread_error(const std::string& msg);  // engine.cpp
}
using namespace q3a;

namespace {

constexpr int32_t kAudioStart = 151669, kAudioPadId = 151676, kAudioEnd = 151670;

// one code point of UTF-8 at s[i] (advances i); malformed bytes come through as U+FFFD, one byte each
uint32_t next_cp(const std::string& s, size_t& i) {
  const unsigned char c = (unsigned char)s[i];
  int n = c < 0x80 ? 0 : (c >> 5) == 6 ? 1 : (c >> 4) == 14 ? 2 : (c >> 3) == 30 ? 3 : -1;
  if (n < 0 || i + n >= s.size()) { ++i; return 0xFFFD; }
  uint32_t cp = n == 0 ? c : n == 1 ? (c & 0x1F) : n == 2 ? (c & 0x0F) : (c & 0x07);
  for (int k = 1; k <= n; ++k) {
    const unsigned char d = (unsigned char)s[i + k];
    if ((d >> 6) != 2) { ++i; return 0xFFFD; }
    cp = (cp << 6) | (d & 0x3F);
  }
  i += n + 1;
  return cp;
}

bool is_cjk(uint32_t cp) {  // _is_cjk_char
  return (cp >= 0x4E00 && cp <= 0x9FFF) || (cp >= 0x3400 && cp <= 0x4DBF) || (cp >= 0x20000 && cp <= 0x2A6DF) ||
         (cp >= 0x2A700 && cp <= 0x2B73F) || (cp >= 0x2B740 && cp <= 0x2B81F) || (cp >= 0x2B820 && cp <= 0x2CEAF) ||
         (cp >= 0xF900 && cp <= 0xFAFF) || (cp >= 0x2F800 && cp <= 0x2FA1F);
}
bool is_space(uint32_t cp) { return cp_in(kUnicodeSpace, kUnicodeSpace_n, cp) || (cp >= 0x1C && cp <= 0x1F); }  // str.isspace
bool is_kept(uint32_t cp) {  // _is_kept_char: ', letters (L*), numbers (N*), CJK
  return cp == '\'' || cp_in(kUnicodeLetter, kUnicodeLetter_n, cp) || cp_in(kUnicodeNumber, kUnicodeNumber_n, cp) || is_cjk(cp);
}

std::vector<std::string> split_words(const std::string& text) {
  std::vector<std::string> words;
  std::string buf;
  auto flush = [&] {
    if (!buf.empty()) words.push_back(buf);
    buf.clear();
  };
  for (size_t i = 0; i < text.size();) {
    const size_t b = i;
    const uint32_t cp = next_cp(text, i);
    if (is_cjk(cp)) {
      flush();
      words.push_back(text.substr(b, i - b));
    } else if (is_space(cp)) {
      flush();
    } else if (is_kept(cp)) {
      buf += text.substr(b, i - b);
    }
  }
  flush();
  return words;
}

}  // namespace

extern "C" {

int32_t q3a_build_align_prompt(int32_t num_audio_tokens, const int32_t* text_ids, int32_t n_text, int32_t* ids, int32_t* len) {
  if (num_audio_tokens < 0 || n_text < 0 || (n_text > 0 && !text_ids && ids)) {
    set_thread_error("q3a_build_align_prompt: bad argument");
    return 1;
  }
  const int32_t n = num_audio_tokens + 2 + n_text;
  if (len) *len = n;
  if (!ids) return 0;
  int32_t* p = ids;
  *p++ = kAudioStart;
  for (int32_t i = 0; i < num_audio_tokens; ++i) *p++ = kAudioPadId;
  *p++ = kAudioEnd;
  for (int32_t i = 0; i < n_text; ++i) *p++ = text_ids[i];
  return 0;
}

int32_t q3a_split_words_for_alignment(const char* utf8, const char* language, char* out, int32_t cap, int32_t* n_words,
                                      int32_t* len) {
  try {
    if (!utf8) fail("q3a_split_words_for_alignment: null text");
    if (language) {
      std::string l(language);
      for (auto& c : l) c = (char)tolower((unsigned char)c);
      if (l == "japanese" || l == "ja" || l == "korean" || l == "ko")
        fail("q3a_split_words_for_alignment: " + std::string(language) +
             " word splitting needs a morphological analyser (nagisa / soynlp) and is not supported; pass the words yourself");
    }
    const std::vector<std::string> words = split_words(utf8);
    std::string joined;
    for (size_t i = 0; i < words.size(); ++i) joined += (i ? "\n" : "") + words[i];
    if (n_words) *n_words = (int32_t)words.size();
    if (len) *len = (int32_t)joined.size();
    if (out && cap > 0) {
      const size_t n = std::min(joined.size(), (size_t)cap - 1);
      memcpy(out, joined.data(), n);
      out[n] = 0;
    }
    return 0;
  } catch (const std::exception& ex) {
    set_thread_error(ex.what());
    return 1;
  }
}

int32_t q3a_align_text_ids(const q3a_tokenizer* t, const char* const* words, int32_t n_words, int32_t timestamp_token_id,
                           int32_t* ids, int32_t cap, int32_t* n) {
  try {
    if (!t || !n || n_words < 0 || (n_words > 0 && !words)) fail("q3a_align_text_ids: bad argument");
    std::vector<int32_t> all;
    std::vector<int32_t> piece(256);
    for (int32_t w = 0; w < n_words; ++w) {
      if (!words[w]) fail("q3a_align_text_ids: null word");
      int32_t k = 0;
      if (q3a_tokenizer_encode(t, words[w], piece.data(), (int32_t)piece.size(), &k) != 0) return 1;
      if (k > (int32_t)piece.size()) {
        piece.resize((size_t)k);
        if (q3a_tokenizer_encode(t, words[w], piece.data(), (int32_t)piece.size(), &k) != 0) return 1;
      }
      all.insert(all.end(), piece.begin(), piece.begin() + k);
      all.push_back(timestamp_token_id);
      all.push_back(timestamp_token_id);
    }
    *n = (int32_t)all.size();
    if (ids)
      for (int32_t i = 0; i < std::min<int32_t>(cap, *n); ++i) ids[i] = all[i];
    return 0;
  } catch (const std::exception& ex) {
    set_thread_error(ex.what());
    return 1;
  }
}

int32_t q3a_fix_timestamps(const float* ms, int32_t n, float* out) {
  if (n < 0 || (n > 0 && (!ms || !out))) {
    set_thread_error("q3a_fix_timestamps: bad argument");
    return 1;
  }
  if (n == 0) return 0;
  const std::vector<double> data(ms, ms + n);
  // longest non-decreasing subsequence, O(n^2), the first of equally long ones by its end index (HF's dp.index(max))
  std::vector<int> dp((size_t)n, 1), parent((size_t)n, -1);
  for (int cur = 1; cur < n; ++cur)
    for (int prev = 0; prev < cur; ++prev)
      if (data[prev] <= data[cur] && dp[prev] + 1 > dp[cur]) { dp[cur] = dp[prev] + 1; parent[cur] = prev; }
  const int max_idx = (int)(std::max_element(dp.begin(), dp.end()) - dp.begin());
  std::vector<bool> normal((size_t)n, false);
  for (int i = max_idx; i != -1; i = parent[i]) normal[i] = true;
  std::vector<double> res = data;
  int bs = 0;
  while (bs < n) {
    if (normal[bs]) { ++bs; continue; }
    int be = bs;
    while (be < n && !normal[be]) ++be;
    const int cnt = be - bs;
    bool has_l = false, has_r = false;
    double lv = 0, rv = 0;
    for (int k = bs - 1; k >= 0; --k)
      if (normal[k]) { has_l = true; lv = res[k]; break; }
    for (int k = be; k < n; ++k)
      if (normal[k]) { has_r = true; rv = res[k]; break; }
    if (cnt <= 2) {
      for (int p = bs; p < be; ++p) res[p] = !has_l ? rv : !has_r ? lv : ((p - (bs - 1)) <= (be - p) ? lv : rv);
    } else if (has_l && has_r) {
      const double step = (rv - lv) / (double)(cnt + 1);
      for (int p = bs; p < be; ++p) res[p] = lv + step * (double)(p - bs + 1);
    } else if (has_l || has_r) {
      for (int p = bs; p < be; ++p) res[p] = has_l ? lv : rv;
    }
    bs = be;
  }
  for (int i = 0; i < n; ++i) out[i] = (float)(long long)res[i];  // int(val): toward zero
  return 0;
}

}  // extern "C"
