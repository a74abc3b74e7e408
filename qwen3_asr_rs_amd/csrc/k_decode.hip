// Decoder glue + the single-token (decode) kernels for gfx950.
//
//   embed_kernel            Tensor::embedding (src/tensor.rs:209-213, src/text_decoder.rs:90-92)
//   qknorm_rope_kv_kernel   per-head RMSNorm on q/k (src/layers.rs:303-304), RoPE x*cos+rotate_half(x)*sin
//                           (src/layers.rs:361-375) and the KV-cache append (src/layers.rs:311-319) -- into a
//                           pre-allocated contiguous cache instead of the reference's per-step `cat`
//   (the GEMV family lives in k_gemv.hip, the single-token attention in k_dattn.hip)
//   argmax_finalize_kernel  argmax (first-index tie-break, src/tensor.rs:370-372), EOS flag, id store and the
//                           embedding of the chosen token for the next step -- no per-token D2H sync
//                           (the reference does int64_value per token, src/inference.rs:161)
#include "argmax.h"
#include "step_commit.h"

namespace q3a {

namespace {

// --------------------------------------------------------------------------------------------------
__global__ void embed_kernel(const int* __restrict__ ids, const uint16_t* __restrict__ embed, int H, int skip_id,
                             float* __restrict__ out) {
  const int r = blockIdx.x;
  const int id = ids[r];
  if (id == skip_id) return;
  const uint2* src = reinterpret_cast<const uint2*>(embed + (size_t)id * H);
  float4* dst = reinterpret_cast<float4*>(out + (size_t)r * H);
  for (int i = threadIdx.x; i < H / 4; i += blockDim.x) {
    const uint2 v = src[i];
    dst[i] = make_float4(bf16lo(v.x), bf16hi(v.x), bf16lo(v.y), bf16hi(v.y));
  }
}

__global__ void set_tokens_kernel(const int* __restrict__ tok, const uint16_t* __restrict__ embed, int H,
                                  float* __restrict__ x_next, int* __restrict__ next_tok, NextNormOut nn) {
  __shared__ float red[16];
  const int s = blockIdx.x;
  const int id = tok[s];
  if (threadIdx.x == 0) next_tok[s] = id;
  embed_row(embed, id, H, x_next, s, nn, red);
}

template <typename KVT>
__global__ __launch_bounds__(256) void qknorm_rope_kv_kernel(RopeKvArgs a, int rows) {
  const int lane = threadIdx.x & 63;
  const int nvec = a.n_q + 2 * a.n_kv;
  const long vi = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (vi >= (long)rows * nvec) return;
  const int row = (int)(vi / nvec), hv = (int)(vi % nvec);
  float* base = a.qkv + (size_t)row * nvec * 128 + (size_t)hv * 128;
  float x1 = base[lane], x2 = base[lane + 64];
  const int pos = a.row_pos[row], seq = a.row_seq[row];
  if (hv < a.n_q) {
    head_norm_rope(x1, x2, a.q_norm, a.eps, a.cos_t, a.sin_t, pos, lane);
    if (a.q16) {
      uint16_t* q = a.q16 + (size_t)row * a.n_q * 128 + (size_t)hv * 128;
      q[lane] = (uint16_t)f32_to_bf16_bits(x1);
      q[lane + 64] = (uint16_t)f32_to_bf16_bits(x2);
    } else {
      base[lane] = x1;
      base[lane + 64] = x2;
    }
  } else {
    const bool is_k = hv < a.n_q + a.n_kv;
    const int kvh = is_k ? hv - a.n_q : hv - a.n_q - a.n_kv;
    if (is_k) head_norm_rope(x1, x2, a.k_norm, a.eps, a.cos_t, a.sin_t, pos, lane);
    KVT* c = reinterpret_cast<KVT*>(is_k ? a.kcache : a.vcache) + (((size_t)seq * a.n_kv + kvh) * a.max_ctx + pos) * 128;
    KvIo<KVT>::store(c + lane, x1);
    KvIo<KVT>::store(c + lane + 64, x2);
  }
}

// --------------------------------------------------------------------------------------------------
// argmax, stage 1 (GEMM path only; the GEMV lm_head writes its partials itself): block partial maxima.  LP: also the log-sum
// channel over the block (argmax.h), kept online per thread.
template <bool LP>
__global__ __launch_bounds__(256) void argmax_partial_kernel(const float* __restrict__ logits, int V, ArgmaxPartials p) {
  __shared__ float bv[4], bs[LP ? 4 : 1];
  __shared__ int bi[4];
  const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (V + gridDim.x - 1) / gridDim.x;
  const int lo = blockIdx.x * per, hi = min(V, lo + per);
  const float* lg = logits + (size_t)s * V;
  ArgmaxAcc<LP> m;
  for (int i = lo + tid; i < hi; i += 256) {
    const float v = lg[i];
    if constexpr (LP) {
      if (v > m.v) m.s = lse_term(m.s, m.v, v) + 1.f;
      else m.s += lse_term(1.f, v, m.v);
    }
    if (v > m.v) { m.v = v; m.i = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m.merge_lane(o);
  if (lane == 0) {
    bv[wave] = m.v; bi[wave] = m.i;
    if constexpr (LP) bs[wave] = m.s;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) m.merge(bv[w], bi[w], bs[LP ? w : 0]);
    m.store(p, s, blockIdx.x);
  }
}

// argmax, stage 2 + bookkeeping of the greedy loop.  LP (token log-probabilities): the chosen id's logit IS the global maximum M, so
// lp = -log sum_p part.sum[p] e^(part.val[p] - M), the merged sum (<= 0: the partial that holds M contributes at least e^0 = 1).
// Kernel arguments: a flat head of 14 dwords preloaded into SGPRs at wave launch (build.py KERNARG_PRELOAD_FLAGS; k_gemv.hip has the
// scheme) -- what the first batch of requests is addressed with -- then the tail, which holds no head field.  The kernel puts its
// FinalizeArgs together again from both, field by field in the order the code object was measured with (an aggregate initialiser of the
// StepCommit gives another register allocation); the token's bookkeeping and rows are step_commit.h's.
struct FinalizeTail {
  float* part_sum;
  int V; int out_stride; int advance;
  uint8_t* done; int* n_done; int n_seq; int* host_progress;
  const uint16_t* embed; int H; float* x_next; int eos0, eos1;
  const float* cos_t; const float* sin_t; float* rope_cur;
  NextNormOut nn;
  float* out_lp;
};
template <bool LP>
__global__ __launch_bounds__(1024) void argmax_finalize_kernel(float* part_val, int* part_idx, int* next_tok, int* out_ids, int* step_count,
                                                               int* pos, int n_part, int part_stride, FinalizeTail t) {
  FinalizeArgs a{};
  a.part.val = part_val; a.part.idx = part_idx; a.c.next_tok = next_tok; a.c.out_ids = out_ids; a.c.step_count = step_count; a.c.pos = pos;
  a.n_part = n_part; a.part.stride = part_stride;
  a.part.sum = t.part_sum; a.V = t.V; a.c.out_stride = t.out_stride; a.advance = t.advance; a.c.done = t.done;
  a.c.n_done = t.n_done; a.c.n_seq = t.n_seq; a.c.host_progress = t.host_progress; a.c.embed = t.embed; a.c.H = t.H; a.c.x_next = t.x_next;
  a.c.eos0 = t.eos0; a.c.eos1 = t.eos1; a.c.cos_t = t.cos_t; a.c.sin_t = t.sin_t; a.c.rope_cur = t.rope_cur; a.c.nn = t.nn; a.c.out_lp = t.out_lp;
  const ArgmaxPartials& part = a.part;
  const StepCommit& c = a.c;
  __shared__ float bv[16], bs[LP ? 16 : 1];
  __shared__ int bi[16];
  __shared__ int tok_s;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // Everything that does not depend on the chosen token is requested up front, in ONE batch: the sequence's counters, the partial
  // maxima (up to FIN_PRE per lane, clamped addresses -- round 6: the plain loop `for (i = tid; i < n_part; i += 1024)` compiled to
  // two loads and a vmcnt(0) per iteration, ten dependent L2 round trips for the 9496 partials of the one-sequence lm_head) and,
  // behind `pos`, the RoPE row of the next position.
  constexpr int FIN_PRE = 10;  // 10 240 partials (vocabulary 151 936 in 16-row blocks: 9496); more are folded by the loop below
  const int pos0 = c.pos[s];
  const int sc = c.step_count[s];
  ArgmaxAcc<LP> pre[FIN_PRE];
#pragma unroll
  for (int j = 0; j < FIN_PRE; ++j) {
    const int i = tid + j * 1024;
    pre[j] = ArgmaxAcc<LP>::load(part, s, i < n_part ? i : n_part - 1);  // all three channels in the same batch
  }
  // what is addressed through the tail comes behind the partials, which need the preloaded head only: the tail in one scalar-load
  // clause (dev.h Q3A_ARG) while they are in flight, instead of one round trip in front of each first use
  Q3A_ARG(t.advance); Q3A_ARG(c.done); Q3A_ARG(t.V); Q3A_ARG(c.out_stride); Q3A_ARG(c.n_done); Q3A_ARG(c.n_seq); Q3A_ARG(c.host_progress);
  Q3A_ARG(c.embed); Q3A_ARG(c.H); Q3A_ARG(c.x_next); Q3A_ARG(c.eos0); Q3A_ARG(c.eos1); Q3A_ARG(c.cos_t); Q3A_ARG(c.sin_t); Q3A_ARG(c.rope_cur);
  const int np = pos0 + t.advance;
  const int was_done = c.done[s];
  const float rope_v = rope_row_elem(c, np);  // (requested here, long before store_rope_row)
  ArgmaxAcc<LP> m;
#pragma unroll
  for (int j = 0; j < FIN_PRE; ++j) {
    const bool in = tid + j * 1024 < n_part;
    m.merge(in ? pre[j].v : -INFINITY, pre[j].i, LP && in ? pre[j].s : 0.f);
  }
  for (int i = tid + FIN_PRE * 1024; i < n_part; i += 1024) m.merge(ArgmaxAcc<LP>::load(part, s, i));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m.merge_lane(o);
  if (lane == 0) {
    bv[wave] = m.v; bi[wave] = m.i;
    if constexpr (LP) bs[wave] = m.s;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 16; ++w) m.merge(bv[w], bi[w], bs[LP ? w : 0]);
    int idx = m.i;
    float lp = 0.f;
    if constexpr (LP) {
      lp = -logf(m.s);
      if (lp > 0.f) lp = 0.f;  // (rounding; NaN passes through)
    }
    if (idx < 0 || idx >= t.V) { idx = 0; lp = __int_as_float(0x7fc00000); }  // all-NaN guard
    tok_s = idx;
    commit_token(c, s, sc, idx, LP, lp, sc + 1, np, was_done);
  }
  __syncthreads();
  store_rope_row(c, s, rope_v);
  embed_row(c.embed, tok_s, c.H, c.x_next, s, c.nn, bv);  // bv: its 16 floats are free again after the barrier above
}

}  // namespace

const char* launch_embed(const int* ids, int rows, const uint16_t* embed, int H, int skip_id, float* out,
                         hipStream_t s) {
  if (rows <= 0) return nullptr;
  hipLaunchKernelGGL(embed_kernel, dim3(rows), dim3(256), 0, s, ids, embed, H, skip_id, out);
  return nullptr;
}
const char* launch_set_tokens(const int* tok, int S, const StepCommit& c, hipStream_t s) {
  if (S <= 0) return nullptr;
  if (!tok) return "set_tokens: null argument";
  if (const char* e = step_commit_check(c, S, Q3A_STEP_COMMIT_MSGS("set_tokens"), true)) return e;
  hipLaunchKernelGGL(set_tokens_kernel, dim3(S), dim3(256), 0, s, tok, c.embed, c.H, c.x_next, c.next_tok, c.nn);
  return nullptr;
}
const char* launch_qknorm_rope_kv(const RopeKvArgs& a, int rows, bool kv_f32, hipStream_t s) {
  if (rows <= 0) return nullptr;
  const long nvec = (long)rows * (a.n_q + 2 * a.n_kv);
  const int blocks = (int)((nvec + 3) / 4);
  if (kv_f32) hipLaunchKernelGGL((qknorm_rope_kv_kernel<float>), dim3(blocks), dim3(256), 0, s, a, rows);
  else hipLaunchKernelGGL((qknorm_rope_kv_kernel<uint16_t>), dim3(blocks), dim3(256), 0, s, a, rows);
  return nullptr;
}
const char* launch_argmax_partials(const float* logits, int V, int S, const ArgmaxPartials& p, int nblk, hipStream_t s) {
  if (S <= 0) return nullptr;
  if (!p.val) return "argmax: partial buffer missing";
  if (const char* e = argmax_partials_check(p, nblk)) return e;
  if (p.sum) hipLaunchKernelGGL(argmax_partial_kernel<true>, dim3(nblk, S), dim3(256), 0, s, logits, V, p);
  else hipLaunchKernelGGL(argmax_partial_kernel<false>, dim3(nblk, S), dim3(256), 0, s, logits, V, p);
  return nullptr;
}
const char* launch_argmax_finalize(const FinalizeArgs& a, int S, hipStream_t s) {
  if (S <= 0) return nullptr;
  if (!a.part.val) return "argmax_finalize: partial buffer missing";
  if (const char* e = argmax_partials_check(a.part, a.n_part)) return e;
  if (!a.part.sum != !a.c.out_lp) return "argmax_finalize: part.sum and out_lp go together";
  const StepCommit& c = a.c;
  if (const char* e = step_commit_check(c, S, Q3A_STEP_COMMIT_MSGS("argmax_finalize"))) return e;
  const FinalizeTail t{a.part.sum, a.V, c.out_stride, a.advance, c.done, c.n_done, c.n_seq, c.host_progress, c.embed, c.H, c.x_next,
                       c.eos0, c.eos1, c.cos_t, c.sin_t, c.rope_cur, c.nn, c.out_lp};
#define Q3A_FIN_ARGS a.part.val, a.part.idx, c.next_tok, c.out_ids, c.step_count, c.pos, a.n_part, a.part.stride, t
  if (a.part.sum) hipLaunchKernelGGL(argmax_finalize_kernel<true>, dim3(S), dim3(1024), 0, s, Q3A_FIN_ARGS);
  else hipLaunchKernelGGL(argmax_finalize_kernel<false>, dim3(S), dim3(1024), 0, s, Q3A_FIN_ARGS);
#undef Q3A_FIN_ARGS
  return nullptr;
}

}  // namespace q3a
