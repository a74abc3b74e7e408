// The device side of kernels.h StepCommit: what a committed token leaves behind, each piece written once for the kernels that end
// a step or begin one (k_decode.hip argmax_finalize / set_tokens, k_draft.hip draft_accept).
#pragma once
#include "dev.h"
#include "kernels.h"

namespace q3a {

// x_next[s] = embedding row `id` (fp32).  With nn.next_w set (skinny decode path) the row is also handed to the next
// GEMM pre-normalised: bf16(x * w_norm) in fragment order plus its sum of squares (kernels.h NextNormOut), so that GEMM
// neither re-reads the fp32 row with 16-line fragment loads nor needs a norm launch.  `red`: shared, one float per wave.
__device__ __forceinline__ void embed_row(const uint16_t* __restrict__ embed, int id, int H, float* __restrict__ x_next, int s,
                                          const NextNormOut& nn, float* red) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  const uint2* src = reinterpret_cast<const uint2*>(embed + (size_t)id * H);
  float4* dst = reinterpret_cast<float4*>(x_next + (size_t)s * H);
  const int gs = nn.group_size > 0 ? nn.group_size : 32;
  const int sl = s % gs;  // position inside its group of sequences (fragment-order buffers hold one group each)
  uint16_t* const xw = nn.next_xw16f + (size_t)(s / gs) * nn.group_stride_x;
  float* const nss = nn.next_ss + (size_t)(s / gs) * nn.group_stride_ss;
  float ss = 0.f;
  for (int i = tid; i < H / 4; i += nthr) {
    const uint2 v = src[i];
    const float4 f = make_float4(bf16lo(v.x), bf16hi(v.x), bf16lo(v.y), bf16hi(v.y));
    dst[i] = f;
    if (nn.next_w) {
      const float4 w = reinterpret_cast<const float4*>(nn.next_w)[i];
      ss += f.x * f.x + f.y * f.y + f.z * f.z + f.w * f.w;
      uint2 pk;  // k = 4i .. 4i+3 are consecutive in fragment order
      pk.x = pack_bf16x2(f.x * w.x, f.y * w.y);
      pk.y = pack_bf16x2(f.z * w.z, f.w * w.w);
      *reinterpret_cast<uint2*>(xw + skinny_frag_index(sl, 4 * i)) = pk;
    }
  }
  if (nn.next_w) {  // kernel-argument condition: uniform
    ss = wave_sum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    if (tid == 0) {
      float t = 0.f;
      for (int w = 0; w < (nthr + 63) / 64; ++w) t += red[w];
      nss[sl] = t;
    }
    for (int p = 1 + tid; p < nn.nparts; p += nthr) nss[(size_t)p * 32 + sl] = 0.f;
  }
}

// One thread of sequence s's workgroup: the bookkeeping of the token `tok` chosen for slot `slot` (with_lp: and its log-probability
// lp), after which the sequence has `count` ids and feeds position `np`.  The sequence's first EOS (inference.rs:163-165; was_done:
// it had one before) sets the sticky flag and counts; ids and positions are plain stores, the pinned progress words system-scope
// atomic stores.
__device__ __forceinline__ void commit_token(const StepCommit& c, int s, int slot, int tok, bool with_lp, float lp, int count, int np,
                                             int was_done) {
  c.next_tok[s] = tok;
  if (slot < c.out_stride) c.out_ids[(size_t)s * c.out_stride + slot] = tok;
  if (with_lp && slot < c.out_stride) c.out_lp[(size_t)s * c.out_stride + slot] = lp;
  c.step_count[s] = count;
  c.pos[s] = np;
  if ((tok == c.eos0 || tok == c.eos1) && !was_done) {
    c.done[s] = 1;
    if (c.n_done) {
      const int n = atomicAdd(c.n_done, 1) + 1;
      if (n == c.n_seq && c.host_progress) __hip_atomic_store(c.host_progress + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  if (s == 0 && c.host_progress) __hip_atomic_store(c.host_progress, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The RoPE row of the position the next decode step works at, kept at a fixed address: the attention kernels of that step request
// it together with q/k/v instead of after a dependent load of pos.  Every thread of the workgroup: rope_row_elem is thread
// tid < 128's element of the cos | sin row of position np (0 where nothing is kept) -- finalize requests it long before the token
// is known -- and store_rope_row stores it, behind the barrier that follows commit_token and in front of embed_row of the token.
// (The two stay two calls in the kernels: wrapped into one function with embed_row, hipcc moves the token's LDS read in front of
// the store and argmax_finalize_kernel is no longer the code object it was.)
__device__ __forceinline__ float rope_row_elem(const StepCommit& c, int np) {
  const int tid = threadIdx.x;
  float v = 0.f;
  if (c.rope_cur && tid < 128) v = tid < 64 ? c.cos_t[(size_t)np * 64 + tid] : c.sin_t[(size_t)np * 64 + tid - 64];
  return v;
}
__device__ __forceinline__ void store_rope_row(const StepCommit& c, int s, float rope_v) {
  const int tid = threadIdx.x;
  if (c.rope_cur && tid < 128) c.rope_cur[(size_t)s * 128 + tid] = rope_v;
}

}  // namespace q3a
