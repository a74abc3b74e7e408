// What engine.cpp and selftest.cpp share and nobody outside the library sees: the error macros, the owner of a device allocation
// and the try / catch frame of a C-ABI entry point.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/q3asr.h"
#include "kernels.h"
#include "model.h"

#define HIPCHK(expr) q3a::hip_check((expr), __FILE__, __LINE__, #expr)
#define KCHK(expr) q3a::kernel_check(expr)  // (a launch_* wrapper returns its refusal, or null)

namespace q3a {

inline void hip_check(hipError_t e, const char* file, int line, const char* expr) {
  if (e != hipSuccess) fail(std::string("HIP error: ") + hipGetErrorString(e) + " at " + file + ":" + std::to_string(line) + " (" + expr + ")");
}
inline void kernel_check(const char* msg) { if (msg) fail(std::string("kernel launch: ") + msg); }

constexpr int kAudioPad = 151676, kEos0 = 151643, kEos1 = 151645;  // src/tokenizer.rs:52-59

// bytes of device memory all DevBufs of the process hold right now (q3a_debug_read "device_bytes")
inline std::atomic<uint64_t> g_device_bytes{0};

// One device allocation and its owner, move-only: freed when it goes out of scope (engine members, taps, locals of the selftests)
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  bool grew = false;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(grew, o.grew); return *this; }  // (o frees what this held)
  ~DevBuf() { release(); }
  void ensure(size_t bytes) {
    if (bytes <= cap) return;
    release();
    size_t want = (bytes + 255) & ~size_t(255);
    HIPCHK(hipMalloc(&p, want));
    cap = want;
    g_device_bytes += want;
    grew = true;
  }
  void release() {
    if (p) { (void)hipFree(p); g_device_bytes -= cap; }
    p = nullptr;
    cap = 0;
  }
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// A sequence-bias list as the kernel reads it (kernels.h SeqBiasArgs): the block of words for the device, and what the refusals and
// q3a_debug_read "sequence_bias" need to know of it.
struct SeqBiasTable {
  std::vector<uint32_t> words;  // [SEQBIAS_TABLE_WORDS]
  int groups = 0, entries = 0, ids = 0, inf_targets = 0;  // groups: distinct targets; inf_targets: distinct targets of -inf entries (of list 0)
  int lists = 0;                                          // totals above are over all lists
  std::vector<int> list_entries, list_inf_targets;        // [lists] entries and distinct -inf targets of every list
};
// ids: the entries' ids one after the other, lens [n], bias [n] (n >= 0).  Entries are sorted stably by target id, the one-token
// entry of a target first.  Throws with `what` in front on every refusal of the header's list that needs no engine: an id outside
// [0, V), an empty or too long entry, too many entries or ids, a sequence given twice, a NaN or +inf bias.  engine.cpp
SeqBiasTable seqbias_layout(const char* what, const int32_t* ids, const int32_t* lens, const float* bias, int n, int V);
// The same for n_lists lists given one after the other, list_lens[k] entries each (q3a_set_sequence_bias_lists): the entries of a list
// stay together, so its target groups are contiguous and the block's directory (SEQBIAS_OFF_LISTS) names their range; a sequence may
// recur in another list, never inside one; the limits are totals over all lists.  One list lays out the words seqbias_layout does.
SeqBiasTable seqbias_layout_lists(const char* what, const int32_t* ids, const int32_t* lens, const float* bias, const int32_t* list_lens, int n_lists, int V);

// A row table of q3a_set_row_options (q3asr.h "row options").  row_options_check throws, `what` and the row's index in front, on every
// value a uniform setter refuses and on a sequence_list outside [-1, n_lists); row_options_words
// lays the records out as the kernels read them: regions sampling | filter | repetition | list, [n_rows][4] words each.  engine.cpp
void row_options_check(const char* what, const q3a_row_options* rows, int n_rows, int n_lists, int V);
std::vector<uint32_t> row_options_words(const q3a_row_options* rows, int n_rows);

// e->err (e null: an entry point without an engine) and the calling thread's q3a_last_error(NULL); engine.cpp
void set_error(q3a_engine* e, const char* msg);

}  // namespace q3a

// frame of a C-ABI entry point: 0, or 1 with the message recorded
#define Q3A_TRY(e) try {
#define Q3A_CATCH(e)                                                                  \
  }                                                                                   \
  catch (const std::exception& ex) { q3a::set_error(e, ex.what()); return 1; }        \
  catch (...) { q3a::set_error(e, "unknown error"); return 1; }                       \
  return 0;
