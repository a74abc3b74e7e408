// Draft verification (kernels.h DraftAcceptArgs; include/q3asr.h "draft-verified decoding"): the step between ONE prefill of
// prompt ++ draft and the captured decode step.  The verify head (k_align.hip, the scoring head's tile) has left, for every sequence,
// the argmax t_i of the rows p - 1 + i, i = 0 .. n.  One workgroup per sequence:
//   1. k = min{ i < n : t_i != d_i } (n if none): every thread scans a strided share of the draft in ascending order and keeps the
//      first mismatch it meets, then a min over the wave (xor butterfly) and over the waves (LDS).  The FIRST mismatch: ids behind it
//      that happen to agree again do not count.
//   2. thread 0 commits tok = t_k at slot k (step_commit.h commit_token: step_count = k + 1, pos = p + k; an EOS as tok finishes the
//      sequence with k ids), with the head's top_lp at that row as its log-probability -- the target's lp bit for bit where the
//      target is the argmax.
//   3. out_ids[0 .. k) = d and their log-probabilities, under the same out_stride guard.
//   4. the RoPE row of pos (store_rope_row) and the embedding of tok (embed_row).
#include "step_commit.h"

namespace q3a {

namespace {

constexpr int DRAFT_THREADS = 256;

__global__ __launch_bounds__(DRAFT_THREADS) void draft_accept_kernel(DraftAcceptArgs a) {
  __shared__ int wk[DRAFT_THREADS / 64];
  __shared__ float red[16];
  __shared__ int k_s, tok_s;
  const StepCommit& c = a.c;
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
    const bool with_lp = c.out_lp != nullptr;
    // (was_done = 0: a prefill begins with the flags clear, and no draft id is an EOS -- refused on the host)
    commit_token(c, s, k, tok, with_lp, with_lp && k < c.out_stride ? a.top_lp[r0 + k] : 0.f, k + 1, p + k, 0);
  }
  __syncthreads();
  k = k_s;
  const int kw = min(k, c.out_stride);  // accepted draft ids that have a slot
  for (int i = tid; i < kw; i += DRAFT_THREADS) {
    c.out_ids[(size_t)s * c.out_stride + i] = a.draft[d0 + i];
    if (c.out_lp) c.out_lp[(size_t)s * c.out_stride + i] = a.top_lp[r0 + i];
  }
  store_rope_row(c, s, rope_row_elem(c, p + k));
  embed_row(c.embed, tok_s, c.H, c.x_next, s, c.nn, red);
}

}  // namespace

const char* launch_draft_accept(const DraftAcceptArgs& a, hipStream_t s) {
  if (a.n_seq <= 0) return nullptr;
  if (!a.draft_off || !a.prompt_len || !a.top_id || !a.accepted) return "draft accept: null argument";
  if (a.c.out_lp && !a.top_lp) return "draft accept: out_lp needs top_lp";
  if (const char* e = step_commit_check(a.c, a.n_seq, Q3A_STEP_COMMIT_MSGS("draft accept"))) return e;
  hipLaunchKernelGGL(draft_accept_kernel, dim3(a.n_seq), dim3(DRAFT_THREADS), 0, s, a);
  return nullptr;
}

}  // namespace q3a
