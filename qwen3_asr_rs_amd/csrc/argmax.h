// Argmax partials on the device (kernels.h ArgmaxPartials): the one definition of the tie rule and of the (max, sum) merge that
// every producer -- the GEMV heads, the gemm16 epilogue, argmax_partial_kernel, the pruned rescore -- and argmax_finalize use.
#pragma once
#include "dev.h"
#include "kernels.h"

namespace q3a {

// Token log-probabilities (opts.token_logprobs): an argmax partial also carries s = sum exp(l - m) over the logits it covers, m being
// its own maximum.  Two pairs merge into the pair of their union as s = s_a e^(m_a - m) + s_b e^(m_b - m), m = the merged maximum;
// this is one such term.  A pair that covers no logit (m_s = -inf, s = 0) contributes 0, never NaN.
__device__ __forceinline__ float lse_term(float s, float m_s, float m) { return m_s == -INFINITY ? 0.f : s * __expf(m_s - m); }

// (maximum v, its first index i[, log-sum s]) of the logits seen so far.  merge() is the only place the tie rule -- the larger value,
// on equal values the smaller index -- and the (max, sum) merge are written.  A site's local stage (one lane's scan of its logits in
// ascending index order, where a strict > keeps the first index, and its log-sum) stays at the site; so does the order in which it
// merges lanes, waves and halves, because the sums are rounded in that order.  LP = false: s is never read, so it costs no register,
// no LDS and no instruction.
template <bool LP>
struct ArgmaxAcc {
  float v = -INFINITY;
  int i = 0x7fffffff;
  float s = 0.f;

  // (by reference: an LDS entry passed as an lvalue is read where the rule needs it; a sum array sized 1 without LP goes as s[LP ? k : 0])
  __device__ __forceinline__ void merge(const float& ov, const int& oi, const float& os) {
    const float pv = v;
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    if constexpr (LP) s = lse_term(s, pv, v) + lse_term(os, ov, v);
  }
  __device__ __forceinline__ void merge(const ArgmaxAcc& o) { merge(o.v, o.i, o.s); }
  // with the accumulator of lane ^ o (every lane of the wave active)
  __device__ __forceinline__ void merge_lane(int o) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    merge(ov, oi, LP ? __shfl_xor(s, o, 64) : 0.f);
  }
  __device__ __forceinline__ void store(const ArgmaxPartials& p, size_t row, int col) const {
    const size_t e = row * p.stride + col;
    p.val[e] = v;
    p.idx[e] = i;
    if constexpr (LP) p.sum[e] = s;
  }
  __device__ __forceinline__ static ArgmaxAcc load(const ArgmaxPartials& p, size_t row, int col) {
    const size_t e = row * p.stride + col;
    return {p.val[e], p.idx[e], LP ? p.sum[e] : 0.f};
  }
};

// one lane's scan of stored logits in ascending id order, online: the (max, first id, sum exp) of what it has seen (the beam
// top-W selection and the sampler's row statistics, k_beam.hip / k_sample.hip)
__device__ __forceinline__ void lse_visit(ArgmaxAcc<true>& m, float v, int id) {
  if (v > m.v) { m.s = lse_term(m.s, m.v, v) + 1.f; m.v = v; m.i = id; }
  else m.s += lse_term(1.f, v, m.v);
}

}  // namespace q3a
