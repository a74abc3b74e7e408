// Draft verification (kernels.h DraftAcceptArgs; include/q3asr.h "draft-verified decoding"): the step between ONE prefill of
// prompt ++ draft and the captured decode step.  The verify head (k_align.hip, the scoring head's tile) has left, for every sequence,
// the argmax t_i of the rows p - 1 + i, i = 0 .. n.  One workgroup per sequence:
//   1. k = min{ i < n : t_i != d_i } (n if none): every thread scans a strided share of the draft in ascending order and keeps the
//      first mismatch it meets, then a min over the wave (xor butterfly) and over the waves (LDS).  The FIRST mismatch: ids behind it
//      that happen to agree again do not count.
//   2. out_ids[0 .. k) = d, out_ids[k] = tok = t_k (and their log-probabilities: the head's top_lp at those rows, which is the
//      target's lp bit for bit where the target is the argmax), with the out_stride guard of argmax_finalize.
//   3. thread 0: next_tok, step_count = k + 1, pos = p + k, the done flag / n_done / pinned progress words as argmax_finalize sets
//      them (an EOS as tok finishes the sequence with k ids); ids and positions are plain stores, the progress words system-scope
//      atomic stores.
//   4. the RoPE row of pos and the embedding of tok (+ the pre-normalised copy of the skinny path), as argmax_finalize.
#include "embed_row.h"

namespace q3a {

namespace {

constexpr int DRAFT_THREADS = 256;

__global__ __launch_bounds__(DRAFT_THREADS) void draft_accept_kernel(DraftAcceptArgs a) {
  __shared__ int wk[DRAFT_THREADS / 64];
  __shared__ float red[16];
  __shared__ int k_s, tok_s;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d0 = a.draft_off[s], n = a.draft_off[s + 1] - d0;
  const int r0 = d0 + s;  // first head row of the sequence (every sequence in front has one row more than draft ids)
  const int p = a.prompt_len[s];
  int k = n;
  for (int i = tid; i < n; i += DRAFT_THREADS)
    if (a.top_id[r0 + i] != a.draft[d0 + i]) { k = i; break; }  // (ascending: the thread's first)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) k = min(k, __shfl_xor(k, o, 64));
  if (lane == 0) wk[wave] = k;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < DRAFT_THREADS / 64; ++w) k = min(k, wk[w]);
    int tok = a.top_id[r0 + k];
    if (tok < 0) tok = 0;  // (a row without a finite logit: the head writes id 0 there)
    k_s = k; tok_s = tok;
    a.accepted[s] = k;
    a.accepted[a.n_seq + s] = tok;
    a.next_tok[s] = tok;
    if (k < a.out_stride) {
      a.out_ids[(size_t)s * a.out_stride + k] = tok;
      if (a.out_lp) a.out_lp[(size_t)s * a.out_stride + k] = a.top_lp[r0 + k];
    }
    a.step_count[s] = k + 1;
    a.pos[s] = p + k;
    if (tok == a.eos0 || tok == a.eos1) {  // the sequence's first EOS: no draft id is one (refused on the host)
      a.done[s] = 1;
      if (a.n_done) {
        const int nd = atomicAdd(a.n_done, 1) + 1;
        if (nd == a.n_seq && a.host_progress) __hip_atomic_store(a.host_progress + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
    if (s == 0 && a.host_progress) __hip_atomic_store(a.host_progress, k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __syncthreads();
  k = k_s;
  const int kw = min(k, a.out_stride);  // accepted draft ids that have a slot
  for (int i = tid; i < kw; i += DRAFT_THREADS) {
    a.out_ids[(size_t)s * a.out_stride + i] = a.draft[d0 + i];
    if (a.out_lp) a.out_lp[(size_t)s * a.out_stride + i] = a.top_lp[r0 + i];
  }
  const int np = p + k;
  if (a.rope_cur && tid < 128) a.rope_cur[(size_t)s * 128 + tid] = tid < 64 ? a.cos_t[(size_t)np * 64 + tid] : a.sin_t[(size_t)np * 64 + tid - 64];
  embed_row(a.embed, tok_s, a.H, a.x_next, s, a.nn, red);
}

}  // namespace

const char* launch_draft_accept(const DraftAcceptArgs& a, hipStream_t s) {
  if (a.n_seq <= 0) return nullptr;
  if (!a.draft_off || !a.prompt_len || !a.top_id || !a.accepted || !a.next_tok || !a.out_ids || !a.step_count || !a.pos || !a.done || !a.embed || !a.x_next)
    return "draft accept: null argument";
  if (a.out_lp && !a.top_lp) return "draft accept: out_lp needs top_lp";
  if (a.out_stride < 1 || a.H < 4 || a.H % 4 != 0) return "draft accept: bad shape";
  if (a.rope_cur && (!a.cos_t || !a.sin_t)) return "draft accept: rope_cur needs the tables";
  if (a.nn.next_w && a.n_seq > 32 && (a.nn.group_stride_x <= 0 || a.nn.group_stride_ss <= 0)) return "draft accept: more than 32 sequences need group strides";
  hipLaunchKernelGGL(draft_accept_kernel, dim3(a.n_seq), dim3(DRAFT_THREADS), 0, s, a);
  return nullptr;
}

}  // namespace q3a
