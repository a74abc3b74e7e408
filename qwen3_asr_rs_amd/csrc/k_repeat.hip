// The history-dependent logits processors on the device: sequence bias (include/q3asr.h "sequence bias") and the
// repetition penalty with the no-repeat n-gram ban (include/q3asr.h "repetition") -- what a step with
// q3a_set_sequence_bias / q3a_set_repetition on puts between the lm_head and the argmax partials (or the sampler).  Each kernel reads
// only the stored logits l' [S][V] (fp32, bias included) and the sequence's own out_ids, so it does not care which head form wrote the
// row, and it keeps nothing from step to step: no trie, no match state, nothing to undo.  The history IS out_ids[s][0 .. t),
// t = min(step_count[s], out_stride).  One kernel per processor, one workgroup of 256 threads per sequence each.
//
//   seqbias_apply_kernel (launch_seqbias_apply):
//                          0a. the last min(t, 31) ids of the history go to LDS (an entry has at most 32 ids, so 31 lead its target);
//                          0b. thread g, stride 256 over the target groups of the ROW'S list (the list index per row and the directory
//                             list_begin from device memory, as G is: another list or row table replays the same graph), walks
//                             its group's entries in the setter's order -- the one-token entry first, then the longer
//                             ones as the caller gave them --, compares each entry's leading ids with the LDS tail and adds the bias
//                             of every entry that fires to acc (0.0f at the start, one fp32 add each); if one fired, the ONE
//                             read-modify-write row[target] += acc.  A target belongs to exactly one group and a group to exactly
//                             one thread: no atomic, no order dependence.  One-token entries fire at t = 0 too (the id the prefill
//                             produces): nothing returns early here.  Every index formed from the tables is checked against the
//                             table's capacity and the row's length before it is used.
//   repeat_apply_kernel (launch_repeat_apply), four steps with a barrier between them:
//                          1. zero a ceil(V / 32)-word bitmap in LDS;
//                          2. every thread reads its share of the history, keeps it in LDS and sets the id's bit (LDS atomic OR);
//                          3. every thread walks its bitmap words and rewrites the set entries of the row in place, l / p where
//                             l > 0 and l * p elsewhere -- one correctly rounded fp32 operation each (plain / and *, the build has no
//                             fast-math flag), and the bitmap is what makes "once per distinct id" true;
//                          4. thread i compares h[i .. i + n - 1) with the last n - 1 ids and stores -inf at h[i + n - 1] on a match.
//                             Idempotent stores: colliding ones are harmless.  After step 3's barrier, or the read-modify-write
//                             of the penalty could overwrite a ban.
// The rewritten row is l''; launch_argmax_partials (or launch_sample) and argmax_finalize then run on it unchanged.
#include "dev.h"
#include "kernels.h"

namespace q3a {

namespace {

__global__ __launch_bounds__(256) void seqbias_apply_kernel(SeqBiasArgs sb) {
  __shared__ int tail[SEQBIAS_MAX_LEN - 1];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int V = sb.V, t = max(min(sb.step_count[s], sb.out_stride), 0);
  const int m = min(t, SEQBIAS_MAX_LEN - 1);  // ids of the history an entry can ask about
  const int* const h = sb.out_ids + (size_t)s * sb.out_stride;
  float* const row = sb.logits + (size_t)s * V;
  if (tid < m) tail[tid] = h[t - m + tid];
  __syncthreads();
  const int G = min(sb.params[0], SEQBIAS_MAX_ENTRIES), E = min(sb.params[1], SEQBIAS_MAX_ENTRIES);
  // the row's own list k (workgroup-uniform): its groups are list_begin[k] .. list_begin[k + 1); no list (-1): nothing to walk
  const int k = sb.row_list[(size_t)s * sb.row_stride];
  const bool listed = (unsigned)k < (unsigned)SEQBIAS_MAX_LISTS;
  const int g0 = listed ? max(sb.list_begin[k], 0) : 0, g1 = listed ? min(sb.list_begin[k + 1], G) : 0;
  for (int g = g0 + tid; g < g1; g += 256) {
    const int target = sb.grp_target[g];
    const int e0 = max(sb.grp_begin[g], 0), e1 = min(sb.grp_begin[g + 1], E);
    float acc = 0.f;
    bool fired = false;
    for (int e = e0; e < e1; ++e) {
      const int off = sb.ent_pre_off[e], n = sb.ent_pre_off[e + 1] - off;  // the entry's L - 1 leading ids: pre_ids[off .. off + n)
      if (n < 0 || n > m || off < 0 || off + n > SEQBIAS_MAX_IDS) continue;  // (n > m: t < L - 1, the entry cannot fire yet)
      bool eq = true;
      for (int k = 0; k < n; ++k) eq = eq && sb.pre_ids[off + k] == tail[m - n + k];
      if (eq) {
        acc += sb.ent_bias[e];
        fired = true;
      }
    }
    if (fired && (unsigned)target < (unsigned)V) row[target] = row[target] + acc;
  }
}

__global__ __launch_bounds__(256) void repeat_apply_kernel(RepeatArgs a, int words, int hist_cap) {
  extern __shared__ __attribute__((aligned(16))) uint32_t repeat_lds[];
  const int s = blockIdx.x, tid = threadIdx.x;
  uint32_t* const bits = repeat_lds;                                         // [words]
  int* const hist = reinterpret_cast<int*>(repeat_lds + ((words + 3) & ~3));  // [hist_cap] the first hist_cap ids of the history
  const int V = a.V;
  const float p = __uint_as_float(a.params[(size_t)s * a.row_stride]);  // the row's own record (stride 0: the one record of all rows)
  const int n = (int)a.params[(size_t)s * a.row_stride + 1];
  const int t = min(a.step_count[s], a.out_stride);
  if (t <= 0) return;  // (the whole workgroup: nothing generated yet, both repetition processors are the identity)
  const int* const h = a.out_ids + (size_t)s * a.out_stride;
  float* const row = a.logits + (size_t)s * V;
  // a history longer than the LDS copy is read where it lies for the rest (out_ids is L2 resident)
  auto at = [&](int i) { return i < hist_cap ? hist[i] : h[i]; };

  for (int w = tid; w < words; w += 256) bits[w] = 0u;
  __syncthreads();
  for (int i = tid; i < t; i += 256) {
    const int id = h[i];
    if (i < hist_cap) hist[i] = id;
    if ((unsigned)id < (unsigned)V) atomicOr(&bits[id >> 5], 1u << (id & 31));
  }
  __syncthreads();
  if (p != 1.f) {  // (x / 1 and x * 1 are x: skipping them changes no bit)
    for (int w = tid; w < words; w += 256) {
      uint32_t m = bits[w];
      while (m) {
        const int j = w * 32 + __ffs((int)m) - 1;  // (bits past V are never set)
        m &= m - 1u;
        const float l = row[j];
        row[j] = l > 0.f ? l / p : l * p;
      }
    }
  }
  __syncthreads();
  if (n >= 1 && t >= n - 1) {
    const int tail0 = t - n + 1;  // h[tail0 .. t): the n - 1 ids a banned id would complete to a seen n-gram
    for (int i = tid; i < tail0; i += 256) {
      bool eq = true;
      for (int k = 0; k < n - 1; ++k) eq = eq && at(i + k) == at(tail0 + k);
      if (eq) {
        const int id = at(i + n - 1);
        if ((unsigned)id < (unsigned)V) row[id] = -INFINITY;
      }
    }
  }
}

}  // namespace

const char* launch_repeat_apply(const RepeatArgs& a, hipStream_t s) {
  if (a.S <= 0) return nullptr;
  if (a.V < 1) return "repetition: empty vocabulary";
  if (a.V > REPEAT_MAX_VOCAB) return "repetition: the vocabulary exceeds the kernel's bitmap (262144 ids)";
  if (!a.logits || !a.params || !a.out_ids || !a.step_count || a.out_stride < 1) return "repetition: null argument";
  const int words = (a.V + 31) / 32, hist_cap = a.out_stride < REPEAT_HIST_LDS ? a.out_stride : REPEAT_HIST_LDS;
  const size_t lds = ((size_t)((words + 3) & ~3) + (size_t)hist_cap) * 4;  // <= 32 KB + 16 KB
  hipLaunchKernelGGL(repeat_apply_kernel, dim3(a.S), dim3(256), lds, s, a, words, hist_cap);
  return nullptr;
}

const char* launch_seqbias_apply(const SeqBiasArgs& a, hipStream_t s) {
  if (a.S <= 0) return nullptr;
  if (a.V < 1) return "sequence bias: empty vocabulary";
  if (!a.logits || !a.params || !a.grp_target || !a.grp_begin || !a.ent_bias || !a.ent_pre_off || !a.pre_ids || !a.list_begin || !a.row_list || !a.out_ids || !a.step_count || a.out_stride < 1)
    return "sequence bias: null argument";
  hipLaunchKernelGGL(seqbias_apply_kernel, dim3(a.S), dim3(256), 0, s, a);
  return nullptr;
}

}  // namespace q3a
