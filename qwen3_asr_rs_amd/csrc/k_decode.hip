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
#include "embed_row.h"

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
// scheme) -- what the first batch of requests is addressed with -- then the tail, which holds no head field.
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
  a.part.val = part_val; a.part.idx = part_idx; a.next_tok = next_tok; a.out_ids = out_ids; a.step_count = step_count; a.pos = pos;
  a.n_part = n_part; a.part.stride = part_stride;
  a.part.sum = t.part_sum; a.V = t.V; a.out_stride = t.out_stride; a.advance = t.advance; a.done = t.done;
  a.n_done = t.n_done; a.n_seq = t.n_seq; a.host_progress = t.host_progress; a.embed = t.embed; a.H = t.H; a.x_next = t.x_next;
  a.eos0 = t.eos0; a.eos1 = t.eos1; a.cos_t = t.cos_t; a.sin_t = t.sin_t; a.rope_cur = t.rope_cur; a.nn = t.nn; a.out_lp = t.out_lp;
  __shared__ float bv[16], bs[LP ? 16 : 1];
  __shared__ int bi[16];
  __shared__ int tok_s;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // Everything that does not depend on the chosen token is requested up front, in ONE batch: the sequence's counters, the partial
  // maxima (up to FIN_PRE per lane, clamped addresses -- round 6: the plain loop `for (i = tid; i < n_part; i += 1024)` compiled to
  // two loads and a vmcnt(0) per iteration, ten dependent L2 round trips for the 9496 partials of the one-sequence lm_head) and,
  // behind `pos`, the RoPE row of the next position.
  constexpr int FIN_PRE = 10;  // 10 240 partials (vocabulary 151 936 in 16-row blocks: 9496); more are folded by the loop below
  const int pos0 = a.pos[s];
  const int sc = a.step_count[s];
  ArgmaxAcc<LP> pre[FIN_PRE];
#pragma unroll
  for (int j = 0; j < FIN_PRE; ++j) {
    const int i = tid + j * 1024;
    pre[j] = ArgmaxAcc<LP>::load(a.part, s, i < a.n_part ? i : a.n_part - 1);  // all three channels in the same batch
  }
  // what is addressed through the tail comes behind the partials, which need the preloaded head only: the tail in one scalar-load
  // clause (dev.h Q3A_ARG) while they are in flight, instead of one round trip in front of each first use
  Q3A_ARG(a.advance); Q3A_ARG(a.done); Q3A_ARG(a.V); Q3A_ARG(a.out_stride); Q3A_ARG(a.n_done); Q3A_ARG(a.n_seq); Q3A_ARG(a.host_progress);
  Q3A_ARG(a.embed); Q3A_ARG(a.H); Q3A_ARG(a.x_next); Q3A_ARG(a.eos0); Q3A_ARG(a.eos1); Q3A_ARG(a.cos_t); Q3A_ARG(a.sin_t); Q3A_ARG(a.rope_cur);
  const int np = pos0 + a.advance;
  const int was_done = a.done[s];
  float rope_v = 0.f;
  if (a.rope_cur && tid < 128) rope_v = tid < 64 ? a.cos_t[(size_t)np * 64 + tid] : a.sin_t[(size_t)np * 64 + tid - 64];
  ArgmaxAcc<LP> m;
#pragma unroll
  for (int j = 0; j < FIN_PRE; ++j) {
    const bool in = tid + j * 1024 < a.n_part;
    m.merge(in ? pre[j].v : -INFINITY, pre[j].i, LP && in ? pre[j].s : 0.f);
  }
  for (int i = tid + FIN_PRE * 1024; i < a.n_part; i += 1024) m.merge(ArgmaxAcc<LP>::load(a.part, s, i));
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
    if (idx < 0 || idx >= a.V) { idx = 0; lp = __int_as_float(0x7fc00000); }  // all-NaN guard
    tok_s = idx;
    a.next_tok[s] = idx;
    if (sc < a.out_stride) a.out_ids[(size_t)s * a.out_stride + sc] = idx;
    if constexpr (LP) {
      if (sc < a.out_stride) a.out_lp[(size_t)s * a.out_stride + sc] = lp;
    }
    a.step_count[s] = sc + 1;
    a.pos[s] = np;
    if ((idx == a.eos0 || idx == a.eos1) && !was_done) {  // this sequence's first EOS (inference.rs:163-165)
      a.done[s] = 1;
      if (a.n_done) {
        const int n = atomicAdd(a.n_done, 1) + 1;
        if (n == a.n_seq && a.host_progress) __hip_atomic_store(a.host_progress + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
    if (s == 0 && a.host_progress) __hip_atomic_store(a.host_progress, sc + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __syncthreads();
  // RoPE row of the position the next decode step works at, at a fixed address: the attention kernels of that step
  // request it together with q/k/v instead of after a dependent load of pos
  if (a.rope_cur && tid < 128) a.rope_cur[(size_t)s * 128 + tid] = rope_v;
  embed_row(a.embed, tok_s, a.H, a.x_next, s, a.nn, bv);  // bv: its 16 floats are free again after the barrier above
}

}  // namespace

const char* launch_embed(const int* ids, int rows, const uint16_t* embed, int H, int skip_id, float* out,
                         hipStream_t s) {
  if (rows <= 0) return nullptr;
  hipLaunchKernelGGL(embed_kernel, dim3(rows), dim3(256), 0, s, ids, embed, H, skip_id, out);
  return nullptr;
}
const char* launch_set_tokens(const int* tok, int S, const uint16_t* embed, int H, float* x_next, int* next_tok,
                              hipStream_t s, const NextNormOut& nn) {
  if (nn.next_w && S > 32 && (nn.group_stride_x <= 0 || nn.group_stride_ss <= 0)) return "set_tokens: more than 32 sequences need group strides";
  hipLaunchKernelGGL(set_tokens_kernel, dim3(S), dim3(256), 0, s, tok, embed, H, x_next, next_tok, nn);
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
  if (!a.part.sum != !a.out_lp) return "argmax_finalize: part.sum and out_lp go together";
  FinalizeTail t{};
  t.part_sum = a.part.sum; t.V = a.V; t.out_stride = a.out_stride; t.advance = a.advance; t.done = a.done;
  t.n_done = a.n_done; t.n_seq = a.n_seq; t.host_progress = a.host_progress; t.embed = a.embed; t.H = a.H; t.x_next = a.x_next;
  t.eos0 = a.eos0; t.eos1 = a.eos1; t.cos_t = a.cos_t; t.sin_t = a.sin_t; t.rope_cur = a.rope_cur; t.nn = a.nn; t.out_lp = a.out_lp;
#define Q3A_FIN_ARGS a.part.val, a.part.idx, a.next_tok, a.out_ids, a.step_count, a.pos, a.n_part, a.part.stride, t
  if (a.part.sum) hipLaunchKernelGGL(argmax_finalize_kernel<true>, dim3(S), dim3(1024), 0, s, Q3A_FIN_ARGS);
  else hipLaunchKernelGGL(argmax_finalize_kernel<false>, dim3(S), dim3(1024), 0, s, Q3A_FIN_ARGS);
#undef Q3A_FIN_ARGS
  return nullptr;
}

}  // namespace q3a
