// Temperature sampling on the device (include/q3asr.h "sampling"): what a sampled step puts between the
// lm_head and argmax_finalize.  All three kernels read only the stored logits l' [S][V] (fp32, bias included), so they do not care
// which head form wrote them.
//
//   sample_rowstat_kernel  the clean (max, sum exp) pair of one 2048-logit chunk of one row: every logit read once, a row spread
//                          over ceil(V / 2048) workgroups (the first half of beam_topk_chunk_kernel; lse_visit is argmax.h's).
//   sample_chunk_kernel    every wave folds the row's chunk maxima into m (a maximum: any order gives the same bits), then the
//                          workgroup scans its chunk once: kept entries (l' >= m + T ln(min_p), never -inf) get the Gumbel noise of
//                          their own Philox word, z = l' + T g, and the chunk's best (z, id) becomes ONE argmax partial.
//                          argmax_finalize (k_decode.hip) then merges n_part = ceil(V / 2048) partials per row as it merges any
//                          producer's: the id, EOS, done, progress words, embedding and RoPE row are the greedy step's.
//   sample_logprob_kernel  one wave per row, after finalize: (m, sum) of the row in a fixed order and lp = (l'_id - m) - log(sum) of the
//                          id finalize chose, written where finalize would have put the greedy log-probability.
// The tie rule is ArgmaxAcc's everywhere: the larger value, on equal values the smaller id.
// With q3a_set_sampling_filter on (top-k / top-p) launch_sample_filtered runs sample_rowstat_kernel and then three
// kernels around the device functions of sample_filter.h.  Off, none of them is enqueued.
//   sample_hist_kernel          the chunk grid: the first-digit histogram of the row's keys (SAMPLE_HIST_LDS of dynamic LDS).
//   sample_select_kernel        one workgroup per row: the radix select, tau_sel[s] and kept[s] (SAMPLE_SELECT_LDS).
//   sample_chunk_filter_kernel  the chunk grid: sample_chunk_kernel with tau_sel[s] as one more threshold.
#include "sample_filter.h"

namespace q3a {

namespace {

template <bool VEC>
__global__ __launch_bounds__(256) void sample_rowstat_kernel(const float* __restrict__ logits, int V, int n_chunk,
                                                             float* __restrict__ chunk_max, float* __restrict__ chunk_sum) {
  __shared__ float wv[4], ws[4];
  __shared__ int wi[4];
  const int s = blockIdx.y, c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = logits + (size_t)s * V;
  const int base = c * SAMPLE_CHUNK;
  ArgmaxAcc<true> m;
  if constexpr (VEC) {  // V % 4 == 0: two 16-byte loads per thread, both requested before the first is used
    float4 f[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = base + q * 1024 + tid * 4;
      f[q] = e < V ? *reinterpret_cast<const float4*>(row + e) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = base + q * 1024 + tid * 4;
      if (e < V) { lse_visit(m, f[q].x, e); lse_visit(m, f[q].y, e + 1); lse_visit(m, f[q].z, e + 2); lse_visit(m, f[q].w, e + 3); }
    }
  } else {
    float f[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = base + q * 256 + tid;
      f[q] = e < V ? row[e] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = base + q * 256 + tid;
      if (e < V) lse_visit(m, f[q], e);
    }
  }
  // lanes, then waves 0..3 -- a fixed order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m.merge_lane(o);
  if (lane == 0) { wv[wave] = m.v; ws[wave] = m.s; wi[wave] = m.i; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) m.merge(wv[w], wi[w], ws[w]);
    chunk_max[(size_t)s * n_chunk + c] = m.v;
    chunk_sum[(size_t)s * n_chunk + c] = m.s;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void sample_chunk_kernel(SampleArgs a, int n_chunk) {
  __shared__ float wv[4];
  __shared__ int wi[4];
  const int s = blockIdx.y, c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.V;
  const float* row = a.logits + (size_t)s * V;
  const int base = c * SAMPLE_CHUNK;
  // everything is requested before anything is used: the chunk's logits, the setting, the step and the row's chunk maxima
  float4 fv[2];
  float fs[8];
  if constexpr (VEC) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = base + q * 1024 + tid * 4;
      fv[q] = e < V ? *reinterpret_cast<const float4*>(row + e) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = base + q * 256 + tid;
      fs[q] = e < V ? row[e] : 0.f;
    }
  }
  const uint32_t* const par = a.params + (size_t)s * a.row_stride;  // the row's own record (stride 0: the one record of all rows)
  const float T = __uint_as_float(par[0]), min_p = __uint_as_float(par[1]);
  const uint32_t seed_lo = par[2], seed_hi = par[3];
  const uint32_t t = (uint32_t)a.step_count[s];
  float m = -INFINITY;
  for (int x = lane; x < n_chunk; x += 64) m = fmaxf(m, a.chunk_max[(size_t)s * n_chunk + x]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  // a greedy row of a row table (T = 0; workgroup-uniform): every finite entry, z = l itself -- 0 * ln(0) below would be NaN
  const bool greedy = !(T > 0.f);
  const float thr = greedy ? -INFINITY : m + T * logf(min_p);  // (min_p = 0: -inf, every finite logit is kept; min_p = 1: m itself)
  ArgmaxAcc<false> acc;
  auto visit = [&](float l, int e) {
    if (l >= thr && l != -INFINITY) {
      const float z = greedy ? l : fmaf(T, gumbel_of(sample_word(seed_lo, seed_hi, (uint32_t)s, t, (uint32_t)e)), l);
      acc.merge(z, e, 0.f);
    }
  };
  if constexpr (VEC) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = base + q * 1024 + tid * 4;
      if (e < V) { visit(fv[q].x, e); visit(fv[q].y, e + 1); visit(fv[q].z, e + 2); visit(fv[q].w, e + 3); }
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = base + q * 256 + tid;
      if (e < V) visit(fs[q], e);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc.merge_lane(o);
  if (lane == 0) { wv[wave] = acc.v; wi[wave] = acc.i; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) acc.merge(wv[w], wi[w], 0.f);
    acc.store(a.part, s, c);  // (a chunk with nothing kept: (-inf, INT_MAX), beaten by every real entry)
  }
}

__global__ __launch_bounds__(64) void sample_logprob_kernel(SampleLogprobArgs a, int n_chunk) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int id = a.next_tok[s], sc = a.step_count[s] - 1;  // (finalize has counted the step it wrote)
  const float l = a.logits[(size_t)s * a.V + id];          // finalize leaves 0 <= id < V
  ArgmaxAcc<true> m;  // lane l takes chunks l, l + 64, ... in ascending order, then the xor butterfly 32 .. 1
  ArgmaxAcc<false> z;
  for (int c = lane; c < n_chunk; c += 64) {
    m.merge(a.chunk_max[(size_t)s * n_chunk + c], c, a.chunk_sum[(size_t)s * n_chunk + c]);
    if (a.out_z) z.merge(ArgmaxAcc<false>::load(a.part, s, c));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { m.merge_lane(o); z.merge_lane(o); }
  if (lane == 0) {
    float lp = (l - m.v) - logf(m.s);
    if (lp > 0.f) lp = 0.f;  // (rounding; NaN passes through)
    if (a.out_lp && sc >= 0 && sc < a.out_stride) a.out_lp[(size_t)s * a.out_stride + sc] = lp;
    if (a.out_z) a.out_z[s] = z.v;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void sample_hist_kernel(SampleArgs a, SampleFilterArgs f, int n_chunk) {
  extern __shared__ __attribute__((aligned(16))) u64 filter_lds[];
  u64* const mass = filter_lds;
  uint32_t* const cnt = reinterpret_cast<uint32_t*>(mass + SAMPLE_BUCKETS);
  sample_hist_phase<VEC>(cnt, mass, a.logits, a.V, n_chunk, a.params, f.filter, a.row_stride, a.chunk_max, f.hist_cnt, f.hist_mass);
}

__global__ __launch_bounds__(256) void sample_select_kernel(SampleArgs a, SampleFilterArgs f, int n_chunk, int vec) {
  extern __shared__ __attribute__((aligned(16))) u64 filter_lds[];
  u64* const mass0 = filter_lds;
  u64* const mass1 = mass0 + SEL_TABLE;
  uint32_t* const cnt0 = reinterpret_cast<uint32_t*>(mass1 + SEL_TABLE);
  sample_select_phase(cnt0, mass0, cnt0 + SEL_TABLE, mass1, a.logits, a.V, n_chunk, vec, a.params, f.filter, a.row_stride, a.chunk_max, f.hist_cnt, f.hist_mass,
                      f.tau_sel, f.kept);
}

template <bool VEC>
__global__ __launch_bounds__(256) void sample_chunk_filter_kernel(SampleArgs a, int n_chunk, const float* __restrict__ tau_sel) {
  sample_chunk_filter_phase<VEC>(a, n_chunk, tau_sel);
}

}  // namespace

const char* launch_sample(const SampleArgs& a, hipStream_t s) {
  if (a.S <= 0) return nullptr;
  if (a.V < 1) return "sample: empty vocabulary";
  if (!a.logits || !a.params || !a.step_count || !a.chunk_max || !a.chunk_sum || !a.part.val) return "sample: null argument";
  const int nc = sample_chunks(a.V);
  if (const char* e = argmax_partials_check(a.part, nc)) return e;
  if (a.part.sum) return "sample: the partials carry no log-sum channel";
  const bool vec = a.V % 4 == 0 && ((uintptr_t)a.logits & 15) == 0;
  const dim3 grid(nc, a.S);
  if (vec) {
    hipLaunchKernelGGL(sample_rowstat_kernel<true>, grid, dim3(256), 0, s, a.logits, a.V, nc, a.chunk_max, a.chunk_sum);
    hipLaunchKernelGGL(sample_chunk_kernel<true>, grid, dim3(256), 0, s, a, nc);
  } else {
    hipLaunchKernelGGL(sample_rowstat_kernel<false>, grid, dim3(256), 0, s, a.logits, a.V, nc, a.chunk_max, a.chunk_sum);
    hipLaunchKernelGGL(sample_chunk_kernel<false>, grid, dim3(256), 0, s, a, nc);
  }
  return nullptr;
}

const char* launch_sample_filtered(const SampleArgs& a, const SampleFilterArgs& f, hipStream_t s) {
  if (a.S <= 0) return nullptr;
  if (a.V < 1) return "sample: empty vocabulary";
  if (!a.logits || !a.params || !a.step_count || !a.chunk_max || !a.chunk_sum || !a.part.val) return "sample: null argument";
  if (!f.filter || !f.hist_cnt || !f.hist_mass || !f.tau_sel || !f.kept) return "sample filter: null argument";
  const int nc = sample_chunks(a.V);
  if (const char* e = argmax_partials_check(a.part, nc)) return e;
  if (a.part.sum) return "sample: the partials carry no log-sum channel";
  const bool vec = a.V % 4 == 0 && ((uintptr_t)a.logits & 15) == 0;
  const dim3 grid(nc, a.S);
  // the rows' statistics, the histogram on the chunk grid, the select with one workgroup per row, the filtered draw on the chunk grid
  if (vec) {
    hipLaunchKernelGGL(sample_rowstat_kernel<true>, grid, dim3(256), 0, s, a.logits, a.V, nc, a.chunk_max, a.chunk_sum);
    hipLaunchKernelGGL(sample_hist_kernel<true>, grid, dim3(256), SAMPLE_HIST_LDS, s, a, f, nc);
  } else {
    hipLaunchKernelGGL(sample_rowstat_kernel<false>, grid, dim3(256), 0, s, a.logits, a.V, nc, a.chunk_max, a.chunk_sum);
    hipLaunchKernelGGL(sample_hist_kernel<false>, grid, dim3(256), SAMPLE_HIST_LDS, s, a, f, nc);
  }
  hipLaunchKernelGGL(sample_select_kernel, dim3(a.S), dim3(256), SAMPLE_SELECT_LDS, s, a, f, nc, vec ? 1 : 0);
  if (vec) hipLaunchKernelGGL(sample_chunk_filter_kernel<true>, grid, dim3(256), 0, s, a, nc, f.tau_sel);
  else hipLaunchKernelGGL(sample_chunk_filter_kernel<false>, grid, dim3(256), 0, s, a, nc, f.tau_sel);
  return nullptr;
}

const char* launch_sample_logprob(const SampleLogprobArgs& a, hipStream_t s) {
  if (a.S <= 0) return nullptr;
  if (!a.logits || !a.next_tok || !a.step_count || !a.chunk_max || !a.chunk_sum) return "sample log-probability: null argument";
  if (!a.out_lp && !a.out_z) return nullptr;
  if (a.out_z && !a.part.val) return "sample log-probability: the noisy score needs the partials";
  hipLaunchKernelGGL(sample_logprob_kernel, dim3(a.S), dim3(64), 0, s, a, sample_chunks(a.V));
  return nullptr;
}

}  // namespace q3a
