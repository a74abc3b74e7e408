// Top log-probabilities (include/q3asr.h "top log-probabilities"): the n best entries of every row of the
// step's final logits l'' with their log-probabilities.  Two kernels of 256 threads, launched by launch_top_logprobs.
//   top_lp_chunk_kernel  the chunk grid (ceil(V / 2048), S): the min(n, chunk) best of one 2048-logit chunk, and the chunk's
//                        (max, sum exp(l - max)).
//   top_lp_row_kernel    one workgroup per row: folds the chunks' pairs into the row's (m, sum) in index order, picks the n best of
//                        the chunks' candidates and writes (id, lp) to slot step_count[s] of the history.
// An entry is ONE 64-bit word (sel_key(l) << 32) | ~index: its unsigned order is "larger logit first, then smaller id", -0.0 and +0.0
// share a key, -inf has the smallest key of all values.  Words of one row are distinct (the indices are), so the r-th best is the
// largest word under the (r - 1)-th: a round is one maximum, nothing is removed and nothing depends on arrival order.  A real entry's
// word is never 0 (no value's key is 0), so 0 stands for "no entry".  The row's n best are among the union of the chunks' n best.
#include "sample_filter.h"

namespace q3a {

namespace {

__device__ __forceinline__ u64 top_lp_word(float l, int index) { return ((u64)sel_key(l) << 32) | (u64)(~(uint32_t)index); }
__device__ __forceinline__ u64 top_lp_umax(u64 a, u64 b) { return a > b ? a : b; }

// the workgroup's maximum of `mine`, for every thread.  red: [4] words of LDS that nobody else touches until the NEXT call with the
// other `red` (the callers alternate between two)
__device__ __forceinline__ u64 top_lp_wg_max(u64 mine, u64* red, int lane, int wave) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine = top_lp_umax(mine, __shfl_xor(mine, o, 64));
  if (lane == 0) red[wave] = mine;
  __syncthreads();
  return top_lp_umax(top_lp_umax(red[0], red[1]), top_lp_umax(red[2], red[3]));
}
// the workgroup's sum of `mine` in a fixed order (the xor tree inside a wave, then the four waves in index order), for every thread
__device__ __forceinline__ float top_lp_wg_sum(float mine, float* red, int lane, int wave) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if (lane == 0) red[wave] = mine;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// n as the kernels use it: the device word, clamped to what the buffers hold and the row has
__device__ __forceinline__ int top_lp_n(const TopLpArgs& a) { return max(min(min(a.n_dev[0], TOP_LP_MAX), a.V), 0); }
// does row s record this step?  not when it is done, and not without a slot (workgroup-uniform)
__device__ __forceinline__ bool top_lp_live(const TopLpArgs& a, int s, int& slot) {
  slot = a.step_count[s];
  return !a.done[s] && slot >= 0 && slot < a.out_stride;
}

template <bool VEC>
__global__ __launch_bounds__(256) void top_lp_chunk_kernel(TopLpArgs a, int n_chunk) {
  __shared__ u64 red[2][4];
  __shared__ float fred[4];
  const int s = blockIdx.y, c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.V, n = top_lp_n(a);
  int slot;
  if (n == 0 || !top_lp_live(a, s, slot)) return;
  const float* row = a.logits + (size_t)s * V;
  const int base = c * SAMPLE_CHUNK;
  float f[8];
  u64 w[8];
  if constexpr (VEC) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = base + q * 1024 + tid * 4;
      const bool in = e < V;  // (V % 4 == 0: all four or none)
      const float4 v = in ? *reinterpret_cast<const float4*>(row + e) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      f[q * 4] = v.x; f[q * 4 + 1] = v.y; f[q * 4 + 2] = v.z; f[q * 4 + 3] = v.w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[q * 4 + j] = in ? top_lp_word(f[q * 4 + j], e + j) : 0ull;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = base + q * 256 + tid;
      f[q] = e < V ? row[e] : -INFINITY;
      w[q] = e < V ? top_lp_word(f[q], e) : 0ull;
    }
  }
  u64* const cand = a.cand + ((size_t)s * n_chunk + c) * TOP_LP_MAX;
  u64 prev = ~0ull;
  float m = -INFINITY;
#pragma nounroll
  for (int r = 0; r < n; ++r) {
    u64 mine = 0ull;
#pragma unroll
    for (int q = 0; q < 8; ++q) mine = top_lp_umax(mine, w[q] < prev ? w[q] : 0ull);
    prev = top_lp_wg_max(mine, red[r & 1], lane, wave);  // (0: the chunk has fewer than n entries; every later round gives 0 again)
    if (tid == 0) cand[r] = prev;
    if (r == 0) m = sel_value((uint32_t)(prev >> 32));  // the chunk's maximum (the chunk is not empty: its workgroup exists)
  }
  // the chunk's sum of exp(l - m): per thread in the order of its eight entries, then the fixed tree.  -inf weighs 0 (and a chunk of
  // nothing but -inf sums to 0, not to exp(-inf + inf))
  float sum = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) sum += f[q] == -INFINITY ? 0.f : expf(f[q] - m);
  sum = top_lp_wg_sum(sum, fred, lane, wave);
  if (tid == 0) {
    a.chunk_max[(size_t)s * n_chunk + c] = m;
    a.chunk_sum[(size_t)s * n_chunk + c] = sum;
  }
}

__global__ __launch_bounds__(256) void top_lp_row_kernel(TopLpArgs a, int n_chunk) {
  extern __shared__ __attribute__((aligned(16))) u64 cand_lds[];  // n_chunk * TOP_LP_MAX words
  __shared__ u64 red[2][4];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.V, n = top_lp_n(a);
  int slot;
  if (n == 0 || !top_lp_live(a, s, slot)) return;
  // (m, sum) of the row from the chunks' pairs: the maximum first (any order gives the same bits), then the rescaled sums in index
  // order, by every thread for itself -- n_chunk <= a few hundred L2 hits, and no second reduction to order
  const float* const cm = a.chunk_max + (size_t)s * n_chunk;
  const float* const cs = a.chunk_sum + (size_t)s * n_chunk;
  const float m = sel_row_max(a.chunk_max, s, n_chunk, lane);
  float sum = 0.f;
  for (int x = 0; x < n_chunk; ++x) sum += cm[x] == -INFINITY ? 0.f : cs[x] * expf(cm[x] - m);
  const float log_sum = logf(sum);
  const int total = n_chunk * n;  // the chunks' first n words each
  for (int i = tid; i < total; i += 256) cand_lds[i] = a.cand[((size_t)s * n_chunk + i / n) * TOP_LP_MAX + i % n];
  __syncthreads();
  u64 prev = ~0ull, keep = 0ull;
#pragma nounroll
  for (int r = 0; r < n; ++r) {
    u64 mine = 0ull;
    for (int i = tid; i < total; i += 256) {
      const u64 x = cand_lds[i];
      mine = top_lp_umax(mine, x < prev ? x : 0ull);
    }
    prev = top_lp_wg_max(mine, red[r & 1], lane, wave);
    if (tid == r) keep = prev;
  }
  if (tid < n && keep != 0ull) {
    const uint32_t id = ~(uint32_t)keep;
    if (id < (uint32_t)V) {  // (always: the word was made from an index of the row)
      const float l = a.logits[(size_t)s * V + id];
      const size_t o = ((size_t)s * a.out_stride + slot) * TOP_LP_MAX + tid;
      a.out_ids[o] = (int)id;
      a.out_lp[o] = l == -INFINITY ? -INFINITY : (l - m) - log_sum;
    }
  }
}

}  // namespace

// The chunk grid, then one workgroup per row with the chunks' candidates in LDS.
const char* launch_top_logprobs(const TopLpArgs& a, hipStream_t s) {
  if (a.S <= 0) return nullptr;
  if (a.V < 1) return "top log-probabilities: empty vocabulary";
  if (a.V > TOP_LP_MAX_VOCAB) return "top log-probabilities: the vocabulary exceeds the row kernel's candidate table (819200 ids)";
  if (!a.logits || !a.n_dev || !a.step_count || !a.done || !a.cand || !a.chunk_max || !a.chunk_sum || !a.out_ids || !a.out_lp || a.out_stride < 1)
    return "top log-probabilities: null argument";
  const int nc = sample_chunks(a.V);
  if (a.V % 4 == 0 && ((uintptr_t)a.logits & 15) == 0) hipLaunchKernelGGL(top_lp_chunk_kernel<true>, dim3(nc, a.S), dim3(256), 0, s, a, nc);
  else hipLaunchKernelGGL(top_lp_chunk_kernel<false>, dim3(nc, a.S), dim3(256), 0, s, a, nc);
  hipLaunchKernelGGL(top_lp_row_kernel, dim3(a.S), dim3(256), (size_t)nc * TOP_LP_MAX * 8, s, a, nc);
  return nullptr;
}

}  // namespace q3a
