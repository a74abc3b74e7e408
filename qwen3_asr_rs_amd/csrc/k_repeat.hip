// Repetition penalty and no-repeat n-grams on the device (include/q3asr.h "repetition"): what a step with
// q3a_set_repetition on puts between the lm_head and the argmax partials (or the sampler).  The kernel reads only the stored logits
// l' [S][V] (fp32, bias included) and the sequence's own out_ids, so it does not care which head form wrote the row, and it keeps
// nothing from step to step: the history IS out_ids[s][0 .. t), t = min(step_count[s], out_stride).
//
//   repeat_apply_kernel    one workgroup of 256 threads per sequence, four phases with a barrier between them:
//                          1. zero a ceil(V / 32)-word bitmap in LDS;
//                          2. every thread reads its share of the history, keeps it in LDS and sets the id's bit (LDS atomic OR);
//                          3. every thread walks its bitmap words and rewrites the set entries of the row in place, l / p where
//                             l > 0 and l * p elsewhere -- one correctly rounded fp32 operation each (plain / and *, the build has no
//                             fast-math flag), and the bitmap is what makes "once per distinct id" true;
//                          4. thread i compares h[i .. i + n - 1) with the last n - 1 ids and stores -inf at h[i + n - 1] on a match.
//                             Idempotent stores: colliding ones are harmless.  After phase 3's barrier, or the read-modify-write
//                             of the penalty could overwrite a ban.
// The rewritten row is l''; launch_argmax_partials (or launch_sample) and argmax_finalize then run on it unchanged.
#include "dev.h"
#include "kernels.h"

namespace q3a {

namespace {

__global__ __launch_bounds__(256) void repeat_apply_kernel(RepeatArgs a, int words, int hist_cap) {
  extern __shared__ __attribute__((aligned(16))) uint32_t repeat_lds[];
  uint32_t* const bits = repeat_lds;                                         // [words]
  int* const hist = reinterpret_cast<int*>(repeat_lds + ((words + 3) & ~3));  // [hist_cap] the first hist_cap ids of the history
  const int s = blockIdx.x, tid = threadIdx.x, V = a.V;
  const float p = __uint_as_float(a.params[0]);
  const int n = (int)a.params[1];
  const int t = min(a.step_count[s], a.out_stride);
  if (t <= 0) return;  // (the whole workgroup: nothing generated yet, both processors are the identity)
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
    const int tail = t - n + 1;  // h[tail .. t): the n - 1 ids a banned id would complete to a seen n-gram
    for (int i = tid; i < tail; i += 256) {
      bool eq = true;
      for (int k = 0; k < n - 1; ++k) eq = eq && at(i + k) == at(tail + k);
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

}  // namespace q3a
