// GEMV family for the single-token decode step on gfx950: y[b][n] = sum_k x[b][k] * W[n][k].
//
// Replaces Linear::forward at one token per sequence (src/layers.rs:74-80) with the surrounding
// RMSNorm (layers.rs:48-54), bias, residual add (layers.rs:442-463) and SiLU(gate)*up (layers.rs:396-400)
// fused, plus the lm_head matmul + argmax of the greedy loop (src/text_decoder.rs:111-112,
// src/inference.rs:161).  HBM-bound: every weight byte is streamed exactly once per token, 16 B per lane
// per load (a wave reads 1 KiB of one weight row per instruction); weights are bf16, x stays fp32, so
// the products are fp32-exact and only the summation order differs from the reference.
//
// Everything in these kernels is latency (a 4-12 MB matrix is 16-48 KB per CU), so the order of work is
//   1. issue the first PF weight loads of every row the wave owns -- they do not depend on x;
//   2. fetch x (L2-resident) while those are in flight.  With one sequence (NB == 1) each lane loads
//      exactly the x slice its weight columns need straight into registers: no LDS, no barrier, and
//      sum(x^2) for the RMSNorm is a plain wavefront reduction because a wave covers all of K.  For
//      NB in {2,4} x is staged through LDS once per workgroup;
//   3. FMA.  The RMSNorm scale is a scalar per row of x, so it multiplies the finished dot product
//      instead of every element (the reference's (x*rstd)*w differs by fp32 rounding only);
//   4. wavefront reduction on DPP (no LDS crossbar), fused epilogue.
// x can also be assembled on the fly from the flash-decoding partials of k_dattn.hip (o_proj input).
#include <algorithm>
#include <type_traits>

#include "argmax.h"


namespace q3a {

int gemv_rows_per_wave(const GemvArgs& a) {  // physical weight rows per wave
  const int logical = (a.mode == 2) ? a.N / 2 : a.N;
  // (2 for mid-size and 1 for small matrices are the measured best: profiles/r6_gemv_rows_per_wave.txt)
  if (logical >= 32768 && a.K <= 2048) return 4;
  if (logical >= 4096 || a.mode == 2) return 2;
  return 1;
}
int gemv_blocks(const GemvArgs& a) {
  const int pr = gemv_rows_per_wave(a);
  const int rows_per_wave = (a.mode == 2) ? pr / 2 : pr;
  const int logical = (a.mode == 2) ? a.N / 2 : a.N;
  return (logical + 4 * rows_per_wave - 1) / (4 * rows_per_wave);
}

namespace {

// Flash-decoding merge (o_proj input).  attn_scales: every workgroup first turns the per-split softmax
// statistics (m, l) of k_dattn.hip into one scale factor per (sequence, head, split),
// f = exp(m - M) / L, in LDS; attn_combined8 then builds 8 consecutive elements (k .. k+7, inside one head)
// of the attention output as sum_split f * o_split -- loads that depend on nothing but the partial buffers.
constexpr int ATTN_F_MAX = 1024;  // NB * heads * nsplit entries (three LDS tables of this size)
struct AttnTables {
  float m[ATTN_F_MAX], l[ATTN_F_MAX], f[ATTN_F_MAX];
};
__device__ __forceinline__ void attn_scales(const GemvArgs& a, int nb, AttnTables& t) {
  const int ns = a.attn_nsplit, n = nb * a.attn_heads * ns;
  // one thread per (sequence, head, split): all statistics are fetched in ONE round of parallel loads
  for (int i = threadIdx.x; i < n; i += 256) {
    t.m[i] = a.attn_pm[i];
    t.l[i] = a.attn_pl[i];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += 256) {
    const int base = (i / ns) * ns;
    float M = -INFINITY;
    for (int sp = 0; sp < ns; ++sp) M = fmaxf(M, t.m[base + sp]);
    float L = 0.f;
    for (int sp = 0; sp < ns; ++sp) {
      const float m = t.m[base + sp];
      if (m != -INFINITY) L += t.l[base + sp] * expf(m - M);
    }
    const float mi = t.m[i];
    t.f[i] = (mi == -INFINITY) ? 0.f : expf(mi - M) / L;
  }
  __syncthreads();
}
__device__ __forceinline__ void attn_combined8(const GemvArgs& a, int b, int k, const AttnTables& t, float (&x)[8]) {
  const int h = k >> 7, d = k & 127;
  const int ns = a.attn_nsplit;
  const int base = (b * a.attn_heads + h) * ns;
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = 0.f;
  for (int sp0 = 0; sp0 < ns; sp0 += 4) {  // 4 splits (8 independent 16-B loads) in flight at a time
    float4 o0[4], o1[4];
    float f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int sp = sp0 + j, spc = sp < ns ? sp : ns - 1;  // clamp the address, zero the weight
      f[j] = sp < ns ? t.f[base + spc] : 0.f;
      o0[j] = *reinterpret_cast<const float4*>(a.attn_po + (size_t)(base + spc) * 128 + d);
      o1[j] = *reinterpret_cast<const float4*>(a.attn_po + (size_t)(base + spc) * 128 + d + 4);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // empty splits carry f = 0 and zeroed partials
      x[0] += o0[j].x * f[j]; x[1] += o0[j].y * f[j]; x[2] += o0[j].z * f[j]; x[3] += o0[j].w * f[j];
      x[4] += o1[j].x * f[j]; x[5] += o1[j].y * f[j]; x[6] += o1[j].z * f[j]; x[7] += o1[j].w * f[j];
    }
  }
}

// Single-sequence form of the merge: no table, no barrier.  The 16 lanes that share a head read that head's (m, l)
// statistics themselves (same-address loads, one request) together with the partial outputs -- every load is
// independent, one L2 round trip -- and rescale online over chunks of 4 splits.
// attn_partial_row8: the request of one split's partial row (8 elements at d of head row base + sp; a split past ns is clamped to the
// last one and voided through its statistics), for this merge and for the MF forms of gemv1_body.
__device__ __forceinline__ void attn_partial_row8(const GemvArgs& a, int base, int sp, int d, float4& o0, float4& o1) {
  const int spc = sp < a.attn_nsplit ? sp : a.attn_nsplit - 1;
  o0 = *reinterpret_cast<const float4*>(a.attn_po + (size_t)(base + spc) * 128 + d);
  o1 = *reinterpret_cast<const float4*>(a.attn_po + (size_t)(base + spc) * 128 + d + 4);
}
// FAST: hardware exponential (default mode); the precise mode keeps expf.
template <bool FAST, int CH>
__device__ __forceinline__ void attn_merge8_ch(const GemvArgs& a, int b, int k, float (&x)[8]) {
  auto ex = [](float v) { return FAST ? __expf(v) : expf(v); };
  const int h = k >> 7, d = k & 127;
  const int ns = a.attn_nsplit;
  const int base = (b * a.attn_heads + h) * ns;
  float M = -INFINITY, L = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = 0.f;
  // Chunks of CH splits: every load of a chunk is requested before anything is combined.  CH = 4 up to 512 keys, 8 beyond:
  // contexts up to 1024 keys cost ONE L2 round trip (with chunks of 4 the fifth split of a 513..640-key context was a
  // second one: 2.4 us of merge in this kernel, profiles/r3_phase_probe_decode_layers.txt).
  for (int sp0 = 0; sp0 < ns; sp0 += CH) {
    float m[CH], l[CH];
    float4 o0[CH], o1[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int sp = sp0 + j, spc = sp < ns ? sp : ns - 1;  // clamp the address, void the statistics
      m[j] = a.attn_pm[base + spc];
      l[j] = a.attn_pl[base + spc];
      if (sp >= ns) m[j] = -INFINITY;
      attn_partial_row8(a, base, sp, d, o0[j], o1[j]);
    }
    // every request above stays above: without the fence hipcc sinks the l / o loads below the `continue` that only needs m --
    // m first, a wait, then the rest: two dependent round trips where the source has one (ISA: global_load x5, s_waitcnt
    // vmcnt(0), branch, global_load x21)
    asm volatile("" ::: "memory");
    float Mn = M;
#pragma unroll
    for (int j = 0; j < CH; ++j) Mn = fmaxf(Mn, m[j]);
    if (Mn == -INFINITY) continue;  // only empty splits so far
    if (sp0 > 0) {  // rescale what the earlier chunks accumulated (nothing in the common <= 8-split case)
      const float sc = (M == -INFINITY) ? 0.f : ex(M - Mn);
      L *= sc;
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] *= sc;
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const float f = ex(m[j] - Mn);  // empty split: exp(-inf) = 0 (Mn is finite here)
      L += l[j] * f;
      x[0] += o0[j].x * f; x[1] += o0[j].y * f; x[2] += o0[j].z * f; x[3] += o0[j].w * f;
      x[4] += o1[j].x * f; x[5] += o1[j].y * f; x[6] += o1[j].z * f; x[7] += o1[j].w * f;
    }
    M = Mn;
  }
  const float inv = 1.0f / L;  // split 0 always holds at least the current token
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] *= inv;
}

template <int PR>
__device__ __forceinline__ void gemv_rows(const GemvArgs& a, int g, int (&prow)[PR]) {
#pragma unroll
  for (int i = 0; i < PR; ++i) {
    if (a.mode == 2) {
      const int j = g * (PR / 2) + (i >> 1);  // logical row; W rows come in [16 gate | 16 up] blocks
      prow[i] = (j / 16) * 32 + (j % 16) + ((i & 1) ? 16 : 0);
    } else {
      prow[i] = g * PR + i;
    }
    if (prow[i] >= a.N) prow[i] = -1;
  }
}

// 8 weights x 8 activations; the multiply-adds run two wide (v_pk_fma_f32): 8 unpack + 4 packed FMA + 2 adds
__device__ __forceinline__ float dot8(const uint4& w, const float (&x)[8], float s) {
  f32x2_t a = f32x2_t{bf16lo(w.x), bf16hi(w.x)} * f32x2_t{x[0], x[1]};
  a += f32x2_t{bf16lo(w.y), bf16hi(w.y)} * f32x2_t{x[2], x[3]};
  a += f32x2_t{bf16lo(w.z), bf16hi(w.z)} * f32x2_t{x[4], x[5]};
  a += f32x2_t{bf16lo(w.w), bf16hi(w.w)} * f32x2_t{x[6], x[7]};
  return s + (a.x + a.y);
}

// ---- pieces shared by the lm_head kernels (gemv1_head_block, both passes of the pruned argmax) and gemvn_kernel ----------------
// gemv1_body keeps the same steps written out: behind these functions hipcc allocated more registers in its shipped forms (the
// qkv / gate-up form lost a wave per SIMD behind unpack_cols, the down projection behind a shared dot loop) and rescheduled the loads
// of the chunked merge (profiles/gemv_family_code_objects.txt).
// One piece of the weight stream: 16 bytes (8 columns at k) of physical row prow; a row past N (prow < 0) is clamped to the last
// one and voided by the epilogue.  Unconditional: no exec-masked blocks, no waits between requests.
__device__ __forceinline__ uint4 ld_w16(const GemvArgs& a, int prow, int k) {
  const int row = prow >= 0 ? prow : a.N - 1;
  return ld_stream16(a.W + (size_t)row * a.K + k);
}
// The HBM stream of a wave: all KI * PR pieces of its rows in flight at once
template <int KI, int PR>
__device__ __forceinline__ void request_rows(const GemvArgs& a, const int (&prow)[PR], const int (&kk)[KI], uint4 (&wq)[KI][PR]) {
#pragma unroll
  for (int it = 0; it < KI; ++it)
#pragma unroll
    for (int i = 0; i < PR; ++i) wq[it][i] = ld_w16(a, prow[i], kk[it]);
}
// The lane's column plan (one sequence): k-iteration `it` covers columns lane * 8 + it * 512 .. + 7.  kin: the piece lies inside K;
// kk: its address, clamped to 0 where it does not (the unpack voids what was loaded there).
template <int KI>
__device__ __forceinline__ void lane_cols(int lane, int K, bool (&kin)[KI], int (&kk)[KI]) {
#pragma unroll
  for (int it = 0; it < KI; ++it) {
    const int k = lane * 8 + it * 512;
    kin[it] = k < K;
    kk[it] = kin[it] ? k : 0;
  }
}
// x and the norm weight of the lane's columns, two float4 each per k-iteration, requested in the order x, x, w, w
template <int KI>
__device__ __forceinline__ void fetch_cols(const GemvArgs& a, const int (&kk)[KI], float4 (&xr)[KI][2], float4 (&nr)[KI][2]) {
#pragma unroll
  for (int it = 0; it < KI; ++it) {
    xr[it][0] = *reinterpret_cast<const float4*>(a.x + kk[it]);
    xr[it][1] = *reinterpret_cast<const float4*>(a.x + kk[it] + 4);
    nr[it][0] = *reinterpret_cast<const float4*>(a.rms_w + kk[it]);
    nr[it][1] = *reinterpret_cast<const float4*>(a.rms_w + kk[it] + 4);
  }
}
// What was fetched, as the operand of the dot products: columns beyond K contribute nothing, ss += x^2 (the RMSNorm's sum, of the
// raw x), x becomes ŷ = x * w_norm; YY (pass 1 of the pruned argmax): *yy += ŷ^2.  The bound of the pruned argmax needs both passes
// to form the same ŷ: they form it here.
template <int KI, bool YY = false>
__device__ __forceinline__ void unpack_cols(int K, const bool (&kin)[KI], const float4 (&xr)[KI][2], const float4 (&nr)[KI][2],
                                            float (&x)[KI][8], float& ss, float* yy = nullptr) {
#pragma unroll
  for (int it = 0; it < KI; ++it) {
    const float4 v0 = xr[it][0], v1 = xr[it][1];
    const float xv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) x[it][e] = (K == KI * 512 || kin[it]) ? xv[e] : 0.f;
    const float4 w0 = nr[it][0], w1 = nr[it][1];
    const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) { ss += x[it][e] * x[it][e]; x[it][e] *= wv[e]; }
    if constexpr (YY) {
#pragma unroll
      for (int e = 0; e < 8; ++e) *yy += x[it][e] * x[it][e];
    }
  }
}
// The four waves' argmax partials of sequence b (lane 0 of each wave wrote them; the caller's barrier lies in between), merged in
// wave order.  LP: with the log-sum channel am_s.
template <bool LP, int NB>
__device__ __forceinline__ ArgmaxAcc<LP> merge_wave_partials(float (*am_v)[NB], int (*am_i)[NB], float (*am_s)[NB], int b) {
  ArgmaxAcc<LP> r{am_v[0][b], am_i[0][b], LP ? am_s[0][b] : 0.f};
  for (int w = 1; w < 4; ++w) r.merge(am_v[w][b], am_i[w][b], LP ? am_s[w][b] : 0.f);
  return r;
}

// epilogue of gemvn_kernel (the one-sequence kernels finish in gemv1_body / gemv1_head_block); acc holds the finished (rstd-scaled)
// dot products, valid on every lane.  LP (mode 3, token log-probabilities): also the log-sum channel (argmax.h); am_s as am_v.
template <int NB, int PR, bool LP>
__device__ __forceinline__ void gemv_epilogue(const GemvArgs& a, int g, const int (&prow)[PR], float (&acc)[PR][NB],
                                              float (*am_v)[NB], int (*am_i)[NB], float (*am_s)[NB]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (a.mode == 3) {  // logits + argmax partial (rows ascend with i, wave, block)
    ArgmaxAcc<LP> m[NB];
    float lv[LP ? PR : 1][NB];  // LP: the wave's logits (-inf for rows past N)
#pragma unroll
    for (int i = 0; i < PR; ++i) {
      if constexpr (LP) {
#pragma unroll
        for (int b = 0; b < NB; ++b) lv[i][b] = -INFINITY;
      }
      if (prow[i] < 0) continue;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float v = acc[i][b];
        if (a.bias) v += a.bias[prow[i]];
        if (lane == 0 && a.out) a.out[(size_t)b * a.ldo + prow[i]] = v;
        if (v > m[b].v) { m[b].v = v; m[b].i = prow[i]; }
        if constexpr (LP) lv[i][b] = v;
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        am_v[wave][b] = m[b].v; am_i[wave][b] = m[b].i;
        if constexpr (LP) {
          float ws = 0.f;
#pragma unroll
          for (int i = 0; i < PR; ++i) ws += lse_term(1.f, lv[i][b], m[b].v);
          am_s[wave][b] = ws;
        }
      }
    }
    __syncthreads();
    if (tid < NB) merge_wave_partials<LP, NB>(am_v, am_i, am_s, tid).store(a.part, tid, g >> 2);
    return;
  }
  if (lane != 0) return;
  if (a.mode != 2) {
#pragma unroll
    for (int i = 0; i < PR; ++i) {
      if (prow[i] < 0) continue;
      const int n = prow[i];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float v = acc[i][b];
        if (a.bias) v += a.bias[n];
        if (a.mode == 1) v += a.resid[(size_t)b * a.ldo + n];
        a.out[(size_t)b * a.ldo + n] = v;
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i + 1 < PR; i += 2) {
      if (prow[i] < 0) continue;
      const int j = g * (PR / 2) + (i >> 1);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float gv = acc[i][b], uv = acc[i + 1][b];
        if (a.bias) { gv += a.bias[prow[i]]; uv += a.bias[prow[i + 1]]; }
        a.out[(size_t)b * a.ldo + j] = silu_sel(gv, a.fast_math != 0) * uv;
      }
    }
  }
}

// ---- NB == 1: x lives in registers (KI k-iterations of 512 columns, K <= 512*KI) ---------------------
// Straight-line by construction: RMS (norm fused) and ATTN (x = merged attention partials) are template flags and no
// load sits under a lane-divergent branch -- out-of-range rows / columns are clamped to valid addresses and voided
// arithmetically.  (With `row < N ? load : 0` guards hipcc put every weight load into its own exec-masked block with
// an s_waitcnt vmcnt(0) between them: half of the stream was only requested after the other half had landed.)
// MF (ATTN only, at most MF key splits, MF in {4, 8}): the merge's loads -- per-split statistics and partial rows -- are requested
// IN FRONT of the weight stream.  Loads return in order: behind the weights (MF = 0) the merge starts when the last weight chunk
// has landed and its exp / scale / LDS round trip / barrier sit exposed between the stream and the FMAs; in front, the partials are
// back after one L2 round trip and the merged vector is in LDS while the weights are still in flight.
// XL (round 6; !ATTN; used for the norm-fused projections at K <= 1024): x (and the norm weight) are fetched ONCE per workgroup -- KI / 2 16-byte loads per lane instead of
// 2 KI (4 KI with the norm weight) -- and handed to the four waves through LDS: every wave needs the whole vector, and in the
// register form each of them pulls it through the CU's texture-address path again (two thirds of a qkv workgroup's load
// instructions were x and norm-weight re-reads).  Same values, same arithmetic.
// XH (the plain forms at K > 2048, KI = 6 / 12: the down projection): the same hand-over of x, chosen from the other flags.  One
// row per wave at K = 3072 is 6 weight loads next to 12 loads of x per wave; with the hand-over 3.  The three x requests go IN FRONT
// of the weights: x is back after one L2 round trip and the store / barrier / read-back run while the weights are in flight (stamped
// timeline, profiles/gemv_down_handover_phase_probe.txt: issue 0.85 -> 0.19 us, span 2.02 -> 1.93 us).  Behind the weights the
// hand-over starts when the last weight chunk has landed and stands exposed in front of the FMAs (span 2.21 us: it lost).
// (Gate / up behind oproj_head_kernel, which also adds o_proj's partial vectors in its hand-over, is gemv1_xp_body below.)
template <int PR, int KI, bool RMS, bool ATTN, int MF, bool XL>
__device__ __forceinline__ void gemv1_body(const GemvArgs& a) {
  static_assert(!XL || !ATTN, "the merged attention vector already goes through LDS");
  constexpr bool XH = !RMS && !ATTN && KI > 4;
  constexpr bool XLDS = XL || XH;  // x is handed over through LDS (the norm weight, xl_w, only in the XL forms)
  static_assert(!XH || KI % 2 == 0, "the hand-over stores unguarded: its rounds of 1024 columns must end at KI * 512");
  // x through LDS: the merged attention vector (ATTN) or the hand-over (XL / XH), never both
  __shared__ __attribute__((aligned(16))) float x_lds[(ATTN || XLDS) ? KI * 512 : 4], xl_w[(XL && RMS) ? KI * 512 : 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  Q3A_STAMP_ENTRY(t_entry);
  const int K = a.K;
  // (an XCD-contiguous block -> row remap, so that each output line is dirtied in one L2 only, measured 0.6 % slower)
  const int g = blockIdx.x * 4 + wave;
  int prow[PR];
  gemv_rows<PR>(a, g, prow);
  bool kin[KI];
  int kk[KI];
#pragma unroll
  for (int it = 0; it < KI; ++it) {
    const int k = lane * 8 + it * 512;
    kin[it] = k < K;
    kk[it] = kin[it] ? k : 0;
  }
  float4 xr[KI][2], nr[RMS ? KI : 1][2];
  uint4 wq[KI][PR];
  constexpr int XLN = (KI + 1) / 2;  // 16-byte pieces of x per lane in the XL / XH forms (256 lanes x 4 floats = 1024 columns per round)
  float4 xl_rx[XLDS ? XLN : 1], xl_rw[(XL && RMS) ? XLN : 1];
  auto request_x = [&]() {  // L2 hits
    if (ATTN) return;
    if constexpr (XLDS) {
#pragma unroll
      for (int j = 0; j < XLN; ++j) {
        const int k = (tid + j * 256) * 4, kc = k < K ? k : 0;
        xl_rx[j] = *reinterpret_cast<const float4*>(a.x + kc);
        if (RMS) xl_rw[j] = *reinterpret_cast<const float4*>(a.rms_w + kc);
      }
      return;
    }
#pragma unroll
    for (int it = 0; it < KI; ++it) {
      xr[it][0] = *reinterpret_cast<const float4*>(a.x + kk[it]);
      xr[it][1] = *reinterpret_cast<const float4*>(a.x + kk[it] + 4);
      if (RMS) {
        nr[it][0] = *reinterpret_cast<const float4*>(a.rms_w + kk[it]);
        nr[it][1] = *reinterpret_cast<const float4*>(a.rms_w + kk[it] + 4);
      }
    }
  };
  auto request_w = [&]() {  // the HBM stream: all KI * PR chunks of the wave's rows in flight at once
#pragma unroll
    for (int it = 0; it < KI; ++it)
#pragma unroll
      for (int i = 0; i < PR; ++i) {
        const int row = prow[i] >= 0 ? prow[i] : a.N - 1;
        wq[it][i] = ld_stream16(a.W + (size_t)row * K + kk[it]);
      }
  };
  // Loads return in order.  With a fused norm, x and the norm weight go first: they are back, squared and scaled long
  // before the first weight chunk lands (-0.2 us).  So does an x that is handed over through LDS (XL, XH: few requests, and the
  // hand-over must not wait for the stream).  A plain x in registers goes behind the weights (2 KI requests in front of them measured
  // +0.2..0.4 us).
  constexpr int MCH = MF > 0 ? MF : 1;
  float mg_m[MCH], mg_l[MCH];
  float4 mg_o0[MCH], mg_o1[MCH];
  const int mg_k = lane * 8 + wave * 512;            // this wave merges elements mg_k .. mg_k + 7 (it == wave)
  const bool mg_on = wave < KI && mg_k < K;          // wave-uniform up to the last partial wave of a short K (clamped below)
  if constexpr (ATTN && MF > 0) {
    const int kc = mg_k < K ? mg_k : 0;
    const int h = kc >> 7, d = kc & 127, ns = a.attn_nsplit, base = h * ns;
    // A head's statistics are ns consecutive floats: 16-byte loads (4-byte aligned; entries past the head's own belong to the next
    // head or to the allocation's padding, hold anything -- NaN included -- and are voided, m AND l: 0 * NaN is NaN) instead of
    // one 4-byte load per split -- and NO branch around
    // loads: a uniform `if` whose arms load made hipcc wait at the join before requesting anything else (tests/test_isa_hazards.py).
    typedef float __attribute__((ext_vector_type(4), aligned(4))) f4u_t;
#pragma unroll
    for (int j = 0; j < MCH; j += 4) {
      const f4u_t m4 = *reinterpret_cast<const f4u_t*>(a.attn_pm + base + j), l4 = *reinterpret_cast<const f4u_t*>(a.attn_pl + base + j);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        mg_m[j + e] = j + e < ns ? m4[e] : -INFINITY;
        mg_l[j + e] = j + e < ns ? l4[e] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < MCH; ++j) attn_partial_row8(a, base, j, d, mg_o0[j], mg_o1[j]);
    __builtin_amdgcn_sched_barrier(0);  // the partials' requests stay in front of the weight stream
  }
  if (RMS || XLDS) { request_x(); request_w(); } else { request_w(); request_x(); }
  // MF forms: the bias below is addressed through the tail, whose scalar loads hipcc issues behind the fence above; without this
  // one it also puts their wait in front of the weight requests
  if constexpr (ATTN && MF > 0) __builtin_amdgcn_sched_barrier(0);
  // epilogue operands (bias, residual) ride behind the stream instead of costing an L2 round trip at the very end
  float bv[PR], rv[PR];
#pragma unroll
  for (int i = 0; i < PR; ++i) {
    const int n = prow[i] >= 0 ? prow[i] : 0;
    bv[i] = a.bias ? a.bias[n] : 0.f;
    rv[i] = a.mode == 1 ? a.resid[n] : 0.f;
  }
  __builtin_amdgcn_sched_barrier(0);  // every request is issued before anything is waited for
  Q3A_STAMP_AT(a.stamp, blockIdx.x, 1);  // every load requested
  Q3A_STAMP_PUT(a.stamp, blockIdx.x, 0, t_entry);  // entry
  // what is left of the tail, in one scalar clause under the loads in flight (dev.h Q3A_ARG)
  Q3A_ARG(a.out); Q3A_ARG(a.fast_math);
  if (ATTN) Q3A_ARG(a.attn_fast_exp);
  if constexpr (ATTN && MF > 0) {  // merge from the registers requested up front (same arithmetic as attn_merge8_ch<FAST, MF>, one chunk)
    if (mg_on) {
      const bool fast = a.attn_fast_exp != 0;
      float Mn = -INFINITY;
#pragma unroll
      for (int j = 0; j < MCH; ++j) Mn = fmaxf(Mn, mg_m[j]);
      float L = 0.f, v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
#pragma unroll
      for (int j = 0; j < MCH; ++j) {
        const float f = fast ? __expf(mg_m[j] - Mn) : expf(mg_m[j] - Mn);  // empty split: exp(-inf) = 0 (split 0 is never empty)
        L += mg_l[j] * f;
        v[0] += mg_o0[j].x * f; v[1] += mg_o0[j].y * f; v[2] += mg_o0[j].z * f; v[3] += mg_o0[j].w * f;
        v[4] += mg_o1[j].x * f; v[5] += mg_o1[j].y * f; v[6] += mg_o1[j].z * f; v[7] += mg_o1[j].w * f;
      }
      const float inv = 1.0f / L;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] *= inv;
      *reinterpret_cast<float4*>(x_lds + mg_k) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4*>(x_lds + mg_k + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
    __syncthreads();
  } else if constexpr (ATTN) {  // each wave merges a quarter of the vector, once per block
    // The two kernel-argument choices (exponential, chunk size) are made OUTSIDE the loop over the wave's pieces: with both inside,
    // every iteration carried four copies of the merge and the K = 6144 form no longer unrolled (kin / kk went to scratch).
    auto merge_pieces = [&](auto fast_c, auto ch_c) {
#pragma unroll
      for (int it = 0; it < KI; ++it) {
        if ((it & 3) == wave && kin[it]) {
          float v[8];
          attn_merge8_ch<decltype(fast_c)::value, decltype(ch_c)::value>(a, 0, kk[it], v);
          *reinterpret_cast<float4*>(x_lds + kk[it]) = make_float4(v[0], v[1], v[2], v[3]);
          *reinterpret_cast<float4*>(x_lds + kk[it] + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
      }
    };
    typedef std::integral_constant<int, 4> Ch4;
    typedef std::integral_constant<int, 8> Ch8;
    if (a.attn_fast_exp) {
      if (a.attn_nsplit <= 4) merge_pieces(std::true_type{}, Ch4{}); else merge_pieces(std::true_type{}, Ch8{});
    } else {
      if (a.attn_nsplit <= 4) merge_pieces(std::false_type{}, Ch4{}); else merge_pieces(std::false_type{}, Ch8{});
    }
    __syncthreads();
  }
  if constexpr (XLDS) {  // hand the vector to the four waves (the weights are still in flight)
#pragma unroll
    for (int j = 0; j < XLN; ++j) {
      const int k = (tid + j * 256) * 4;
      if (XH || k < KI * 512) {  // (XH: KI is even, the XLN rounds cover exactly KI * 512 columns)
        // element by element: as one aggregate copy (a memcpy from the private array to LDS) hipcc kept xl_rx[XLN > 1] in scratch
        float4 v = xl_rx[j];
        *reinterpret_cast<float4*>(x_lds + k) = make_float4(v.x, v.y, v.z, v.w);
        if (RMS) *reinterpret_cast<float4*>(xl_w + k) = xl_rw[j];
      }
    }
    __syncthreads();
  }
  // every wave reads the whole vector back (the norm weight with it in the XL forms), behind the barrier of whichever path filled x_lds
  if constexpr (ATTN || XLDS) {
#pragma unroll
    for (int it = 0; it < KI; ++it) {
      xr[it][0] = *reinterpret_cast<const float4*>(x_lds + kk[it]);
      xr[it][1] = *reinterpret_cast<const float4*>(x_lds + kk[it] + 4);
      if (XL && RMS) {
        nr[it][0] = *reinterpret_cast<const float4*>(xl_w + kk[it]);
        nr[it][1] = *reinterpret_cast<const float4*>(xl_w + kk[it] + 4);
      }
    }
  }
  Q3A_STAMP_AT(a.stamp, blockIdx.x, 2);  // (ATTN: merged vector in LDS)
  float x[KI][8], acc[PR];
  float ss = 0.f;
#pragma unroll
  for (int it = 0; it < KI; ++it) {
    const float4 v0 = xr[it][0], v1 = xr[it][1];
    const float xv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) x[it][e] = (K == KI * 512 || kin[it]) ? xv[e] : 0.f;  // columns beyond K contribute nothing
    if (RMS) {
      const float4 w0 = nr[it][0], w1 = nr[it][1];
      const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) { ss += x[it][e] * x[it][e]; x[it][e] *= wv[e]; }
    }
  }
#pragma unroll
  for (int i = 0; i < PR; ++i) acc[i] = 0.f;
#pragma unroll
  for (int it = 0; it < KI; ++it)
#pragma unroll
    for (int i = 0; i < PR; ++i) acc[i] = dot8(wq[it][i], x[it], acc[i]);
  if (wave == 0) asm volatile("" ::"v"(acc[0]));  // (the stamp below sits behind the FMAs of wave 0, i.e. behind its weights)
  Q3A_STAMP_AT(a.stamp, blockIdx.x, 3);  // weights landed, dot products done
  float rstd = 1.0f;
  if (RMS) rstd = rstd_of(wave_sum_fast(ss) / (float)K + a.eps, a.fast_math != 0);  // a wave covers all of K
#pragma unroll
  for (int i = 0; i < PR; ++i) acc[i] = wave_sum_fast(acc[i]) * rstd + bv[i];
  // epilogue (bias already added; acc is valid on every lane; mode 3 runs gemv1_head_kernel)
  if (lane != 0) return;
  if (a.mode != 2) {
#pragma unroll
    for (int i = 0; i < PR; ++i)
      if (prow[i] >= 0) a.out[prow[i]] = acc[i] + rv[i];
  } else {
#pragma unroll
    for (int i = 0; i + 1 < PR; i += 2)
      if (prow[i] >= 0) a.out[g * (PR / 2) + (i >> 1)] = silu_sel(acc[i], a.fast_math != 0) * acc[i + 1];
  }
  Q3A_STAMP_AT(a.stamp, blockIdx.x, 4);  // reduced and stored
}

// Kernel arguments of the one-sequence chain: a flat head, then a tail struct.  The head -- pointers first, at most 14 dwords -- is what
// stands in front of the kernel's first memory request; the command processor preloads it into SGPRs at wave launch (build.py
// KERNARG_PRELOAD_FLAGS), so the weight stream is requested without waiting for a scalar load of the kernarg segment.  A struct by
// value is never preloaded: the tail (what the kernel needs only behind its requests) is fetched by ordinary scalar loads that
// overlap them.  The tails hold NO head field, so no stale copy of one can be read; the kernels rebuild the launcher's GemvArgs
// from head and tail in registers and run the one body.
struct GemvTail {  // plain and norm-fused forms
  float* out; int fast_math;
  Q3A_STAMP_FIELD
};
struct GemvAttnTail {  // ATTN forms (o_proj: x = merged attention partials)
  float* out; const float* bias; int attn_heads; int attn_fast_exp; int fast_math;
  Q3A_STAMP_FIELD
};
#ifdef Q3A_STAMP
#define Q3A_STAMP_COPY(dst, src) (dst).stamp = (src).stamp
#else
#define Q3A_STAMP_COPY(dst, src) do { } while (0)
#endif
template <int PR, int KI, bool RMS, bool ATTN, int MF = 0, bool XL = false>
__global__ __launch_bounds__(256) void gemv1_kernel(const uint16_t* W, const float* x, const float* rms_w, const float* bias,
                                                    const float* resid, int N, int K, int mode, float eps, GemvTail t) {
  static_assert(!ATTN, "the ATTN forms take the partials in their head");
  GemvArgs a{};
  a.W = W; a.x = x; a.rms_w = rms_w; a.bias = bias; a.resid = resid; a.N = N; a.K = K; a.mode = mode; a.eps = eps;
  a.out = t.out; a.fast_math = t.fast_math;
  Q3A_STAMP_COPY(a, t);
  gemv1_body<PR, KI, RMS, ATTN, MF, XL>(a);
}
// (The split count and the mode stand in front of the first partial / weight address.  out is first needed by the final store, and
// the bias -- no o_proj of the models has one -- is requested behind the weight stream: both ride in the tail.)
template <int PR, int KI, bool RMS, bool ATTN, int MF = 0, bool XL = false>
__global__ __launch_bounds__(256) void gemv1_kernel(const float* attn_pm, const float* attn_pl, const float* attn_po, const uint16_t* W,
                                                    const float* resid, int N, int K, int attn_nsplit, int mode, GemvAttnTail t) {
  static_assert(ATTN && !RMS, "the plain forms take x and the norm weight in their head");
  GemvArgs a{};
  a.attn_pm = attn_pm; a.attn_pl = attn_pl; a.attn_po = attn_po; a.W = W; a.resid = resid; a.N = N; a.K = K; a.attn_nsplit = attn_nsplit;
  a.mode = mode;
  a.out = t.out; a.bias = t.bias; a.attn_heads = t.attn_heads; a.attn_fast_exp = t.attn_fast_exp; a.fast_math = t.fast_math;
  Q3A_STAMP_COPY(a, t);
  gemv1_body<PR, KI, RMS, ATTN, MF, XL>(a);
}

// ---- gate / up behind oproj_head_kernel (the XP form: mode 2, norm fused, K <= 1024) ----------------------------------------
// The vector the waves multiply is x + x_parts[0] + ... + x_parts[n - 1], n <= GEMV_X_PARTS_MAX = 4: the residual and o_proj's partial
// vectors, added in ascending order; workgroup 0 also stores the sum to x_out, the residual the down projection and the next layer read
// (a buffer no workgroup of this launch reads, so the store races with nothing).  A wave is the wave of gemv1_body<2, 2, true, false, 0,
// true>: same rows per wave (g = blockIdx.x * NW + wave), lane / column plan, dot8 order, wave_sum_fast and rstd -- bit-identical
// results whatever NW.  What NW changes is how many waves share one hand-over.  With four waves per workgroup (three workgroups per CU at
// 0.6B) every CU pulled the six vectors of the hand-over -- x, four partial vectors, the norm weight, 4 KB each -- three times through its
// load path, 72 KB in front of its 48 KB of weights, and loads return in order.  With NW = 12, one workgroup per CU, it pulls them once,
// and two thirds of the waves request nothing but their weights.  The waves take roles:
//   waves 0 .. 3   the 256 threads that own four columns each request x and the four partial vectors (5 requests), then their weights;
//                  they add in registers as the four-wave form did and store the sum to LDS (and to x_out);
//   waves 4 .. 7   request the norm weight of their four columns (1 request), then their weights, and store it to LDS;
//   waves 8 ..     request their weights only.
// One barrier, then every wave reads the sum and the norm weight back.  Each role is a straight-line program of its own behind ONE
// scalar branch on the wave index at entry: no load sits under a branch that joins again in front of another request, so every role's
// requests form one run in front of its first wait (9, 5 and 4: tests/test_gate_up_wide_isa.py).
// Measured and not kept (profiles/gate_up_wide_*.txt, docs/HISTORY.md "Gate / up: twelve waves per workgroup"): the 6 x 256 pieces spread
// evenly over all threads and added from LDS behind a second barrier, at 12 and at 6 waves -- a faster issue (0.72 -> 0.27 us) but the
// summed vector 0.66 us later, a loss of 8 - 14 us per step.
template <int PR, int KI, int NW, int ROLE>
__device__ __forceinline__ void gemv1_xp_role(const GemvArgs& a, float* x_lds, float* xl_w) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  Q3A_STAMP_ENTRY(t_entry);
  const int K = a.K;
  const int g = blockIdx.x * NW + wave;
  int prow[PR];
  gemv_rows<PR>(a, g, prow);
  bool kin[KI];
  int kk[KI];
#pragma unroll
  for (int it = 0; it < KI; ++it) {
    const int k = lane * 8 + it * 512;
    kin[it] = k < K;
    kk[it] = kin[it] ? k : 0;
  }
  float4 xr[KI][2], nr[KI][2];
  uint4 wq[KI][PR];
  const int hk = (tid & (KI * 128 - 1)) * 4, hkc = hk < K ? hk : 0;
  float4 hx, hp[GEMV_X_PARTS_MAX], hw;
  if constexpr (ROLE == 0) {  // L2 hits; a partial vector past n is clamped to the last one and not added, a column past K to column 0
    hx = *reinterpret_cast<const float4*>(a.x + hkc);
#pragma unroll
    for (int h = 0; h < GEMV_X_PARTS_MAX; ++h)
      hp[h] = *reinterpret_cast<const float4*>(a.x_parts + (size_t)(h < a.x_nparts ? h : a.x_nparts - 1) * K + hkc);
  }
  if constexpr (ROLE == 1) hw = *reinterpret_cast<const float4*>(a.rms_w + hkc);
#pragma unroll
  for (int it = 0; it < KI; ++it)  // the HBM stream: all KI * PR chunks of the wave's rows in flight at once
#pragma unroll
    for (int i = 0; i < PR; ++i) {
      const int row = prow[i] >= 0 ? prow[i] : a.N - 1;
      wq[it][i] = ld_stream16(a.W + (size_t)row * K + kk[it]);
    }
  float bv[PR];  // the bias rides behind the stream
#pragma unroll
  for (int i = 0; i < PR; ++i) bv[i] = a.bias ? a.bias[prow[i] >= 0 ? prow[i] : 0] : 0.f;
  __builtin_amdgcn_sched_barrier(0);  // every request is issued before anything is waited for
  Q3A_STAMP_AT(a.stamp, blockIdx.x, 1);  // every load requested
  Q3A_STAMP_PUT(a.stamp, blockIdx.x, 0, t_entry);  // entry
  Q3A_ARG(a.out); Q3A_ARG(a.x_out); Q3A_ARG(a.fast_math);
  if constexpr (ROLE == 0) {
    float4 v = hx;
#pragma unroll
    for (int h = 0; h < GEMV_X_PARTS_MAX; ++h)
      if (h < a.x_nparts) { v.x += hp[h].x; v.y += hp[h].y; v.z += hp[h].z; v.w += hp[h].w; }
    if (blockIdx.x == 0 && hk < K) *reinterpret_cast<float4*>(a.x_out + hk) = v;
    *reinterpret_cast<float4*>(x_lds + hk) = make_float4(v.x, v.y, v.z, v.w);
  }
  if constexpr (ROLE == 1) *reinterpret_cast<float4*>(xl_w + hk) = make_float4(hw.x, hw.y, hw.z, hw.w);
  __syncthreads();
#pragma unroll
  for (int it = 0; it < KI; ++it) {
    xr[it][0] = *reinterpret_cast<const float4*>(x_lds + kk[it]);
    xr[it][1] = *reinterpret_cast<const float4*>(x_lds + kk[it] + 4);
    nr[it][0] = *reinterpret_cast<const float4*>(xl_w + kk[it]);
    nr[it][1] = *reinterpret_cast<const float4*>(xl_w + kk[it] + 4);
  }
  Q3A_STAMP_AT(a.stamp, blockIdx.x, 2);  // the summed vector read back
  float x[KI][8], acc[PR];
  float ss = 0.f;
#pragma unroll
  for (int it = 0; it < KI; ++it) {
    const float4 v0 = xr[it][0], v1 = xr[it][1];
    const float xv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) x[it][e] = (K == KI * 512 || kin[it]) ? xv[e] : 0.f;  // columns beyond K contribute nothing
    const float4 w0 = nr[it][0], w1 = nr[it][1];
    const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) { ss += x[it][e] * x[it][e]; x[it][e] *= wv[e]; }
  }
#pragma unroll
  for (int i = 0; i < PR; ++i) acc[i] = 0.f;
#pragma unroll
  for (int it = 0; it < KI; ++it)
#pragma unroll
    for (int i = 0; i < PR; ++i) acc[i] = dot8(wq[it][i], x[it], acc[i]);
  if (wave == 0) asm volatile("" ::"v"(acc[0]));  // (the stamp below sits behind the FMAs of wave 0, i.e. behind its weights)
  Q3A_STAMP_AT(a.stamp, blockIdx.x, 3);  // weights landed, dot products done
  const float rstd = rstd_of(wave_sum_fast(ss) / (float)K + a.eps, a.fast_math != 0);  // a wave covers all of K
#pragma unroll
  for (int i = 0; i < PR; ++i) acc[i] = wave_sum_fast(acc[i]) * rstd + bv[i];
  if (lane != 0) return;
#pragma unroll
  for (int i = 0; i + 1 < PR; i += 2)
    if (prow[i] >= 0) a.out[g * (PR / 2) + (i >> 1)] = silu_sel(acc[i], a.fast_math != 0) * acc[i + 1];
  Q3A_STAMP_AT(a.stamp, blockIdx.x, 4);  // reduced and stored
}
template <int PR, int KI, int NW>
__device__ __forceinline__ void gemv1_xp_body(const GemvArgs& a) {
  static_assert(KI == 2 && NW >= 8, "four waves own the KI * 128 sixteen-byte pieces of a vector; four more fetch the norm weight");
  __shared__ __attribute__((aligned(16))) float x_lds[KI * 512], xl_w[KI * 512];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wave < 4) gemv1_xp_role<PR, KI, NW, 0>(a, x_lds, xl_w);
  else if (wave < 8) gemv1_xp_role<PR, KI, NW, 1>(a, x_lds, xl_w);
  else gemv1_xp_role<PR, KI, NW, 2>(a, x_lds, xl_w);
}
// Every vector the hand-over's requests are addressed with stands in the head; the store of the sum (x_out) rides in the tail.
struct GemvXpTail {
  float* out; float* x_out; int fast_math;
  Q3A_STAMP_FIELD
};
constexpr int GEMV_XP_WAVES = 12;  // 3072 outputs at 0.6B: 256 workgroups, one per CU
template <int PR, int KI, int NW>
__global__ __launch_bounds__(NW * 64) void gemv1_xp_kernel(const uint16_t* W, const float* x, const float* rms_w, const float* x_parts,
                                                           const float* bias, int N, int K, int x_nparts, float eps, GemvXpTail t) {
  GemvArgs a{};
  a.W = W; a.x = x; a.rms_w = rms_w; a.x_parts = x_parts; a.bias = bias; a.N = N; a.K = K; a.x_nparts = x_nparts; a.eps = eps; a.mode = 2;
  a.out = t.out; a.x_out = t.x_out; a.fast_math = t.fast_math;
  Q3A_STAMP_COPY(a, t);
  gemv1_xp_body<PR, KI, NW>(a);
}

// ---- o_proj per column slice (one sequence, default mode) ---------------------------------------------------
// Workgroup (slice p, row block): the CW columns of slice p -- whole kv heads, CW / 128 q heads -- of RB rows of W.  Today's
// o_proj merges the whole context in each of its 256 workgroups (nsplit x 8 KB of partials next to 16 KB of weights); here a
// workgroup requests only its slice's partials (nsplit x CW x 4 bytes), in one batch in front of its weights, and merges them once:
//   * thread (tg, e4) of the TG = 256 / (CW / 4) thread groups requests 4 elements (e4) of splits tg, tg + TG, ...: OPROJ_HEAD_MAX_SPLITS /
//     TG requests per thread, a split past nsplit clamped to the last one and voided through its statistics;
//   * the statistics (m, l) of the slice's heads go through LDS: one request per thread, then every thread reads its head's 16
//     entries back and forms M, L and f_j = exp(m_j - M) as attn_merge8_ch does (hardware exponential; an empty split has m = -inf,
//     f = 0, and zeroed partials);
//   * each thread group's sum over its splits goes to LDS, and every lane adds the TG sums of the 8 columns its weights need, in
//     ascending group order, and scales by 1 / L.
// The weight slice of a row is CW / 8 lanes x 16 B: a wave instruction covers 64 / (CW / 8) rows.  The result is y_part[p][n], fp32:
// no residual -- the consumer (gemv1_xp_kernel) adds the slices to it.  Slice p = blockIdx.x % n_parts.  Built and measured with CW =
// 256 (one kv head per slice: 8 partial vectors at the models' shapes, each workgroup on the XCD whose L2 holds what decode attention
// wrote for its kv head under round-robin placement) and CW = 512 (a pair of kv heads, 4 vectors): 512 won by 3 us per step -- gate / up
// requests half as many vectors -- and is the only form instantiated (profiles/oproj_by_head_headline_ab.txt).
struct OprojHeadTail {
  const float* bias;
  Q3A_STAMP_FIELD
};
template <int CW, int RB>
__global__ __launch_bounds__(256) void oproj_head_kernel(const float* pm, const float* pl, const float* po, const uint16_t* W, float* y_part,
                                                         int N, int K, int nsplit, int n_parts, OprojHeadTail t) {
  constexpr int NS = OPROJ_HEAD_MAX_SPLITS;
  constexpr int HEADS = CW / 128;  // q heads of a slice
  constexpr int LPR = CW / 8;      // lanes per row slice
  constexpr int RPI = 64 / LPR;    // rows per wave instruction
  constexpr int NI = RB / 4 / RPI; // weight requests per lane
  constexpr int E4 = CW / 4;       // 16-byte pieces of one split's slice
  constexpr int TG = 256 / E4;     // thread groups
  constexpr int SPT = NS / TG;     // splits per thread
  static_assert(CW == 128 || CW == 256 || CW == 512, "a slice is 1, 2 or 4 q heads");
  static_assert(NI >= 1 && NI * RPI * 4 == RB && SPT * TG == NS && HEADS * NS <= 256, "row block / split plan");
  __shared__ float m_s[HEADS * NS], l_s[HEADS * NS], inv_s[HEADS];
  __shared__ __attribute__((aligned(16))) float red[TG][CW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  Q3A_STAMP_ENTRY(t_entry);
  const int part = blockIdx.x % n_parts, rb = blockIdx.x / n_parts;
  const int q0 = part * HEADS;  // first q head of the slice
  const int e4 = tid % E4, tg = tid / E4, hh = e4 >> 5, d = (e4 & 31) * 4;
  // 1. statistics: entry (head, split) = tid of the first HEADS * NS threads; the others repeat the last entry (no branch around a load)
  const int st = tid < HEADS * NS ? tid : HEADS * NS - 1, st_j = st % NS, st_jc = st_j < nsplit ? st_j : nsplit - 1;
  float st_m = pm[(size_t)(q0 + st / NS) * nsplit + st_jc], st_l = pl[(size_t)(q0 + st / NS) * nsplit + st_jc];
  // 2. this thread's pieces of the partial rows
  float4 o[SPT];
#pragma unroll
  for (int i = 0; i < SPT; ++i) {
    const int j = tg + i * TG, jc = j < nsplit ? j : nsplit - 1;
    o[i] = *reinterpret_cast<const float4*>(po + ((size_t)(q0 + hh) * nsplit + jc) * 128 + d);
  }
  __builtin_amdgcn_sched_barrier(0);  // the partials' requests stay in front of the weight stream
  // 3. the weight stream: rows past N are clamped to the last one and not stored
  const int row0 = rb * RB + wave * (RB / 4) + lane / LPR;
  uint4 wq[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int row = row0 + i * RPI, rc = row < N ? row : N - 1;
    wq[i] = ld_stream16(W + (size_t)rc * K + part * CW + (lane % LPR) * 8);
  }
  __builtin_amdgcn_sched_barrier(0);
  float bv[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int row = row0 + i * RPI;
    bv[i] = (t.bias && part == 0) ? t.bias[row < N ? row : N - 1] : 0.f;
  }
  __builtin_amdgcn_sched_barrier(0);  // every request is issued before anything is waited for
  Q3A_STAMP_AT(t.stamp, blockIdx.x, 1);  // every load requested
  Q3A_STAMP_PUT(t.stamp, blockIdx.x, 0, t_entry);  // entry
  if (st_j >= nsplit) { st_m = -INFINITY; st_l = 0.f; }  // (a stale entry past nsplit may hold anything)
  if (tid < HEADS * NS) { m_s[tid] = st_m; l_s[tid] = st_l; }
  __syncthreads();
  float M = -INFINITY, L = 0.f;
#pragma unroll
  for (int j = 0; j < NS; ++j) M = fmaxf(M, m_s[hh * NS + j]);  // finite: split 0 always holds the current token
#pragma unroll
  for (int j = 0; j < NS; ++j) L += l_s[hh * NS + j] * __expf(m_s[hh * NS + j] - M);  // empty split: exp(-inf) = 0
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < SPT; ++i) {
    const float f = __expf(m_s[hh * NS + tg + i * TG] - M);
    acc.x += o[i].x * f; acc.y += o[i].y * f; acc.z += o[i].z * f; acc.w += o[i].w * f;
  }
  *reinterpret_cast<float4*>(&red[tg][e4 * 4]) = acc;
  if (tg == 0 && (e4 & 31) == 0) inv_s[hh] = 1.0f / L;
  __syncthreads();
  // 4. the merged context of the 8 columns this lane's weights multiply
  const int c0 = (lane % LPR) * 8;
  float x[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = 0.f;
#pragma unroll
  for (int g = 0; g < TG; ++g) {
    const float4 a0 = *reinterpret_cast<const float4*>(&red[g][c0]), a1 = *reinterpret_cast<const float4*>(&red[g][c0 + 4]);
    x[0] += a0.x; x[1] += a0.y; x[2] += a0.z; x[3] += a0.w; x[4] += a1.x; x[5] += a1.y; x[6] += a1.z; x[7] += a1.w;
  }
  const float inv = inv_s[c0 >> 7];
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] *= inv;
  Q3A_STAMP_AT(t.stamp, blockIdx.x, 2);  // merged slice in registers
  float y[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    float v = row16_sum(dot8(wq[i], x, 0.f));
    if (LPR >= 32) v = xor16_sum(v);
    if (LPR >= 64) v = xor32_sum(v);
    y[i] = v + bv[i];
  }
  if (wave == 0) asm volatile("" ::"v"(y[0]));
  Q3A_STAMP_AT(t.stamp, blockIdx.x, 3);  // weights landed, dot products done
  if (lane % LPR == 0) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int row = row0 + i * RPI;
      if (row < N) y_part[(size_t)part * N + row] = y[i];
    }
  }
  Q3A_STAMP_AT(t.stamp, blockIdx.x, 4);  // stored
}

// ---- lm_head (mode 3, one sequence, fused final RMSNorm) -------------------------------------------------
// One 16-row argmax block (4 waves x PR rows) of the one-sequence lm_head: the arithmetic of gemv1_kernel<PR, KI, true, false>
// (same lane / column assignment, same order of the products and sums, same rstd, first-index tie rule).  Used by the
// unpruned launch (gemv1_head_kernel: block = blockIdx.x) AND by the rescore of the pruned argmax (lm_head_rescore_kernel): the
// two cannot drift apart.  Ends with a barrier; the block's partial is valid in thread 0's `out`.  LP (token log-probabilities):
// with the log-sum channel (am_s: 4 floats of LDS); the value / row arithmetic is the same either way.
template <int PR, int KI, bool LP = false>
__device__ __forceinline__ void gemv1_head_block(const GemvArgs& a, int blk, float (&am_v)[4][1], int (&am_i)[4][1], float (*am_s)[1],
                                                 ArgmaxAcc<LP>& out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blk * 4 + wave;
  int prow[PR];
  gemv_rows<PR>(a, g, prow);
  bool kin[KI];
  int kk[KI];
  lane_cols<KI>(lane, a.K, kin, kk);
  float4 xr[KI][2], nr[KI][2];
  uint4 wq[KI][PR];
  fetch_cols<KI>(a, kk, xr, nr);  // x and the norm weight first (L2 hits), then the weight stream
  request_rows<KI, PR>(a, prow, kk, wq);
  float bv[PR];
#pragma unroll
  for (int i = 0; i < PR; ++i) bv[i] = a.bias ? a.bias[prow[i] >= 0 ? prow[i] : 0] : 0.f;
  __builtin_amdgcn_sched_barrier(0);  // every request is issued before anything is waited for
  float x[KI][8], acc[PR];
  float ss = 0.f;
  unpack_cols<KI>(a.K, kin, xr, nr, x, ss);
#pragma unroll
  for (int i = 0; i < PR; ++i) acc[i] = 0.f;
#pragma unroll
  for (int it = 0; it < KI; ++it)
#pragma unroll
    for (int i = 0; i < PR; ++i) acc[i] = dot8(wq[it][i], x[it], acc[i]);
  const float rstd = rstd_of(wave_sum_fast(ss) / (float)a.K + a.eps, a.fast_math != 0);  // a wave covers all of K
#pragma unroll
  for (int i = 0; i < PR; ++i) acc[i] = wave_sum_fast(acc[i]) * rstd + bv[i];
  ArgmaxAcc<LP> m;
#pragma unroll
  for (int i = 0; i < PR; ++i) {
    if (prow[i] < 0) continue;
    if (lane == 0 && a.out) a.out[prow[i]] = acc[i];
    if (acc[i] > m.v) { m.v = acc[i]; m.i = prow[i]; }
  }
  if (lane == 0) { am_v[wave][0] = m.v; am_i[wave][0] = m.i; }
  if constexpr (LP) {
    float ws = 0.f;
#pragma unroll
    for (int i = 0; i < PR; ++i) ws += prow[i] < 0 ? 0.f : lse_term(1.f, acc[i], m.v);
    if (lane == 0) am_s[wave][0] = ws;
  }
  __syncthreads();
  if (tid == 0) out = merge_wave_partials<LP, 1>(am_v, am_i, am_s, 0);
}

// (head / tail as gemv1_kernel: the tail is the partial descriptor, first needed by the block's final store)
template <int PR, int KI, bool LP = false>
__global__ __launch_bounds__(256) void gemv1_head_kernel(const uint16_t* W, const float* x, const float* rms_w, const float* bias, float* out,
                                                         int N, int K, float eps, int fast_math, ArgmaxPartials part) {
  __shared__ float am_v[4][1];
  __shared__ int am_i[4][1];
  __shared__ float am_s[LP ? 4 : 1][1];
  GemvArgs a{};
  a.W = W; a.x = x; a.rms_w = rms_w; a.bias = bias; a.out = out; a.N = N; a.K = K; a.eps = eps; a.fast_math = fast_math; a.mode = 3;
  ArgmaxAcc<LP> r;
  gemv1_head_block<PR, KI, LP>(a, blockIdx.x, am_v, am_i, am_s, r);
  if (threadIdx.x == 0) r.store(part, 0, blockIdx.x);
}

// ---- pruned argmax of the one-sequence lm_head ------------------------------------------------------------
// The decode step only needs argmax_r l_r, l_r = rstd * sum_k y_k W_rk (y = x o w_norm, fp32; W bf16).  Pass 1 streams the int8 copy
// Q (model.h lm_head_q: half the bytes) and gives every row an approximate logit a_r and a bound e_r with |a_r - l_r| <= e_r, where
// l_r is the fp32 value gemv1_head_block computes.  T = max_r (a_r - e_r) is then <= the logit of some row, so a row with
// a_r + e_r < T cannot be the maximum, nor tie with it.  Pass 2 recomputes, with gemv1_head_block, every 16-row block whose
// hi_b = max (a_r + e_r) is not below T and reduces them to one (value, row) partial per workgroup.  The ids are those of the
// unpruned launch; the worst case (every block a candidate) is one extra full pass.
//
// The bound.  Let ŷ_k be the fp32 products x_k * w_k both passes form (unpack_cols: one function, the same lanes), G = sum ŷ_k W_rk and
// P = sum ŷ_k Q_rk exactly, Ĝ and P̂ their fp32 evaluations, s = s_r.  Each term of either dot product passes through at most
// K/64 + 1 roundings in its lane (the product -- none if fused -- and the chain of packed adds and FMAs over the lane's K/64
// columns) and 6 in the 64-lane wave_sum_fast tree; whatever the order and the fusing, the classic bound (Higham, Accuracy and
// Stability of Numerical Algorithms, 3.1) gives |Ĝ - G| <= γ sum|ŷ_k W_rk| with γ = n u / (1 - n u), u = 2^-24, n any upper bound
// on the roundings per term.  n = cols >= K/64 + 7 (cols = 1024 or 2048 padded columns) is used.  With Cauchy-Schwarz:
//   |Ĝ - G| <= γ ||ŷ|| ||W_r||,   |s P̂ - s P| <= γ ||ŷ|| ||s Q_r||,   |G - s P| = |ŷ . (W_r - s Q_r)| <= ||ŷ|| ||W_r - s Q_r||
//   => |Ĝ - s P̂| <= ||ŷ|| (dn_r + γ (wn_r + qn_r)),  and  l_r = fl(Ĝ rstd), a_r = fl(fl(P̂ s) rstd).
// The three roundings of the final products add at most 3.1 u (|a_r| + |l_r - a_r|); the fp32 evaluation of ||ŷ|| (relative
// error <= γ/2 + u) and of e_r itself (< 8 u) are covered by the relative margin 2^-10; 2^-20 |a_r| covers the final roundings,
// and 1e-30 the absolute error of products that underflow.  dn, wn, qn are rounded up by the packer.
// NaN or infinite bounds make the block a candidate (hi = +inf): such rows are rescored, never skipped.
//
// With a logit bias (q3asr.h q3a_set_logit_bias: b_r finite or -inf, g.bias) the argmax is taken over l'_r = l_r + b_r, and both passes
// add b_r: pass 2 is gemv1_head_block, whose `acc * rstd + bv` is l'_r = fl(λ + b_r) with λ = fl(Ĝ rstd) or, where the compiler fuses
// the multiply and the add, λ = Ĝ rstd exactly; pass 1 forms a'_r = fl(α + b_r) with α = a_r or its unrounded product in the same way.
// e_r bounds |α - λ| in all four combinations: the derivation above bounds the distance of the exact products and then ADDS one
// term per rounding, so leaving a rounding out only loosens it.  Each of the two sums is rounded once:
//   |a'_r - (α + b_r)| <= u |α + b_r| <= u (|a_r| (1 + u) + |b_r|),   |l'_r - (λ + b_r)| <= u |λ + b_r| <= u (|a_r| (1 + u) + e_r + |b_r|)
//   => |a'_r - l'_r| <= e_r + u e_r + 2 u (1 + u) |a_r| + 2 u |b_r| <= e'_r = (e_r + 2^-22 (|a_r| + |b_r|)) (1 + 2^-20):
// 2 u = 2^-23 is half of the coefficient used (the other half covers the u^2 term), and the factor 1 + 2^-20 covers u e_r and the
// four roundings of e'_r's own evaluation (<= 4 u e'_r).  b_r = 0 gives a'_r = a_r and e'_r >= e_r: still a bound, a little wider.
// A suppressed row (b_r = -inf) has a'_r = l'_r = -inf exactly: lo = hi = -inf, never a candidate and NOT the "no bound" case above,
// so a block with every row suppressed is skipped by pass 2 (hi_b = -inf < T: the engine refuses a bias without a finite entry, so
// T is finite or the NaN / overflow case) and an allow-list makes pass 2 cheaper.  This holds for finite activations, the only ones
// the bound is stated for: with a NaN or inf in x the exact l'_r of a suppressed row is NaN, not -inf, and the row is still dropped
// here while the full GEMV would carry the NaN; x is shared by every row, so every unsuppressed row then takes the "no bound" case
// and is rescored to NaN as well: the two paths differ only inside a step that is poisoned in both.  The bias entry is requested with the row's qs
// entry, in the same batch as the weights: 4 bytes per row next to cols bytes.
// Without a bias the kernel that runs is the one without the code (template parameter BIAS of lm_head_approx_body: false in
// lm_head_approx_kernel, the launch of an engine that never set a bias, true in lm_head_approx_bias_kernel); pass 2 keeps
// gemv1_head_block's uniform null check on a.bias.
struct LmHeadArgsDev {  // what pass 1 reads, device side only: its kernels assemble it from their flat head and their tail
  GemvArgs g;
  const int8_t* Wq; const float* qs; int qcols;
  float gamma;
  float* blk_lo; float* blk_hi; int n_blk;
  float* dbg;  // [N][2] (a_r, e_r), debug taps only
};

__device__ __forceinline__ float dotq8(uint32_t lo, uint32_t hi, const float (&x)[8], float s) {
  f32x2_t a = f32x2_t{(float)(int8_t)lo, (float)(int8_t)(lo >> 8)} * f32x2_t{x[0], x[1]};
  a += f32x2_t{(float)(int8_t)(lo >> 16), (float)((int32_t)lo >> 24)} * f32x2_t{x[2], x[3]};
  a += f32x2_t{(float)(int8_t)hi, (float)(int8_t)(hi >> 8)} * f32x2_t{x[4], x[5]};
  a += f32x2_t{(float)(int8_t)(hi >> 16), (float)((int32_t)hi >> 24)} * f32x2_t{x[6], x[7]};
  return s + (a.x + a.y);
}

// The int8 copy: one wave per row.  Every value is formed in fp64 from the bf16 weights; the three norms are rounded up to fp32
// after a relative margin of 2^-40 that covers the fp64 summation.
__global__ __launch_bounds__(256) void lm_head_quantize_kernel(const uint16_t* W, int N, int K, int cols, int8_t* Q, float* qs) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= N) return;  // wave-uniform
  const uint16_t* w = W + (size_t)r * K;
  float m = 0.f;
  for (int k = lane; k < K; k += 64) m = fmaxf(m, fabsf(__uint_as_float((uint32_t)w[k] << 16)));
  m = wave_max(m);
  const bool fin = isfinite(m);  // (fmaxf drops NaN: a NaN row is caught by the norms below)
  const float s = fin ? (float)((double)m / 127.0) : 0.f;
  double dn = 0.0, wn = 0.0, qn = 0.0;
  for (int k = lane; k < K; k += 64) {
    const double v = __uint_as_float((uint32_t)w[k] << 16);
    const double q = s > 0.f ? fmin(127.0, fmax(-127.0, rint(v / (double)s))) : 0.0;
    Q[(size_t)r * cols + ((k % 512) / 8) * (cols / 64) + (k / 512) * 8 + k % 8] = (int8_t)q;
    const double e = v - (double)s * q;
    dn += e * e; wn += v * v; qn += q * q;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    dn += __shfl_xor(dn, o); wn += __shfl_xor(wn, o); qn += __shfl_xor(qn, o);
  }
  if (lane == 0) {
    auto up = [](double v) {  // smallest float >= v (1 + 2^-40: the fp64 sums' own rounding)
      v *= 1.0 + 0x1p-40;
      const float f = (float)v;
      return (double)f < v ? nextafterf(f, INFINITY) : f;
    };
    float4 o = make_float4(s, up(sqrt(dn)), up(sqrt(wn)), up((double)s * sqrt(qn)));
    if (!fin || !isfinite(o.y) || !isfinite(o.z)) o = make_float4(0.f, INFINITY, INFINITY, 0.f);  // no bound: always rescored
    reinterpret_cast<float4*>(qs)[r] = o;
  }
}

// Pass 1: one wave per 16-row block, 16 rows x cols/64 bytes per lane in flight (the bf16 launch: 4 rows x 2 x cols/64); no barrier
template <int KI, bool BIAS>
__device__ __forceinline__ void lm_head_approx_body(const LmHeadArgsDev& p) {
  constexpr int R = 16, NQ = KI / 2;  // rows per wave; 16-byte pieces of an int8 row per lane
  const GemvArgs& a = p.g;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = a.K, blk = blockIdx.x * 4 + wave;
  if (blk >= p.n_blk) return;  // wave-uniform
  bool kin[KI];
  int kk[KI];
  lane_cols<KI>(lane, K, kin, kk);
  float4 xr[KI][2], nr[KI][2];
  fetch_cols<KI>(a, kk, xr, nr);
  uint4 wq[R][NQ];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int r = blk * R + i, row = r < a.N ? r : a.N - 1;
#pragma unroll
    for (int j = 0; j < NQ; ++j) wq[i][j] = ld_stream16(p.Wq + (size_t)row * p.qcols + lane * (KI * 8) + j * 16);
  }
  const int my_r = blk * R + lane;  // lanes 0..15 finish one row each
  const bool my_valid = lane < R && my_r < a.N;
  const float4 q = reinterpret_cast<const float4*>(p.qs)[my_valid ? my_r : 0];  // {s, dn, wn, qn}
  float bq = 0.f;  // BIAS: the row's logit bias, same request batch
  if constexpr (BIAS) bq = a.bias[my_valid ? my_r : 0];
  __builtin_amdgcn_sched_barrier(0);  // every request is issued before anything is waited for
  float x[KI][8];
  float ss = 0.f, yy = 0.f;
  unpack_cols<KI, true>(K, kin, xr, nr, x, ss, &yy);  // gemv1_head_block's x, sum(x^2) and ŷ: the same function
  float acc[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    acc[i] = 0.f;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {  // piece j: columns of it = 2j (bytes 0..7) and it = 2j + 1 (bytes 8..15)
      acc[i] = dotq8(wq[i][j].x, wq[i][j].y, x[2 * j], acc[i]);
      acc[i] = dotq8(wq[i][j].z, wq[i][j].w, x[2 * j + 1], acc[i]);
    }
  }
  const float rstd = rstd_of(wave_sum_fast(ss) / (float)K + a.eps, a.fast_math != 0);
  const float ny = sqrtf(wave_sum_fast(yy));
  float mine = 0.f;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const float t = wave_sum_fast(acc[i]);
    if (lane == i) mine = t;
  }
  const float av = (mine * q.x) * rstd;
  const float ev = (rstd * ny) * (q.y + p.gamma * (q.z + q.w)) * (1.0f + 0x1p-10f) + fabsf(av) * 0x1p-20f + 1e-30f;
  float lo = -INFINITY, hi = -INFINITY;
  if constexpr (BIAS) {
    if (my_valid) {
      const float ab = av + bq;                                                     // a'_r
      const float eb = (ev + 0x1p-22f * (fabsf(av) + fabsf(bq))) * (1.0f + 0x1p-20f);  // e'_r (the comment above LmHeadArgsDev)
      if (bq == -INFINITY) {  // suppressed: l'_r = -inf exactly, never a candidate (lo = hi = -inf stay)
        if (p.dbg) { p.dbg[(size_t)my_r * 2] = -INFINITY; p.dbg[(size_t)my_r * 2 + 1] = 0.f; }
      } else {
        lo = ab - eb;
        hi = ab + eb;
        if (!(lo <= hi) || hi == INFINITY) { lo = -INFINITY; hi = INFINITY; }  // NaN / overflow: always rescored
        if (p.dbg) { p.dbg[(size_t)my_r * 2] = ab; p.dbg[(size_t)my_r * 2 + 1] = eb; }
      }
    }
  } else if (my_valid) {
    lo = av - ev;
    hi = av + ev;
    if (!(lo <= hi) || hi == INFINITY) { lo = -INFINITY; hi = INFINITY; }  // NaN / overflow: always rescored
    if (p.dbg) { p.dbg[(size_t)my_r * 2] = av; p.dbg[(size_t)my_r * 2 + 1] = ev; }
  }
  lo = wave_max(lo);
  hi = wave_max(hi);
  if (lane == 0) { p.blk_lo[blk] = lo; p.blk_hi[blk] = hi; }
}

// kernel arguments as gemv1_kernel: what stands in front of the int8 stream is the head, the rest the tail
struct LmHeadApproxTail {
  float eps; int fast_math; float gamma;
  float* blk_lo; float* blk_hi; float* dbg;
};
__device__ __forceinline__ LmHeadArgsDev lm_head_approx_args(const int8_t* Wq, const float* x, const float* rms_w, const float* qs, const float* bias,
                                                             int N, int K, int qcols, int n_blk, const LmHeadApproxTail& t) {
  LmHeadArgsDev p{};
  p.Wq = Wq; p.g.x = x; p.g.rms_w = rms_w; p.qs = qs; p.g.bias = bias; p.g.N = N; p.g.K = K; p.qcols = qcols; p.n_blk = n_blk;
  p.g.eps = t.eps; p.g.fast_math = t.fast_math; p.gamma = t.gamma; p.blk_lo = t.blk_lo; p.blk_hi = t.blk_hi; p.dbg = t.dbg;
  return p;
}
template <int KI>
__global__ __launch_bounds__(256) void lm_head_approx_kernel(const int8_t* Wq, const float* x, const float* rms_w, const float* qs, const float* bias,
                                                             int N, int K, int qcols, int n_blk, LmHeadApproxTail t) {
  lm_head_approx_body<KI, false>(lm_head_approx_args(Wq, x, rms_w, qs, bias, N, K, qcols, n_blk, t));
}
template <int KI>
__global__ __launch_bounds__(256) void lm_head_approx_bias_kernel(const int8_t* Wq, const float* x, const float* rms_w, const float* qs,
                                                                  const float* bias, int N, int K, int qcols, int n_blk, LmHeadApproxTail t) {
  lm_head_approx_body<KI, true>(lm_head_approx_args(Wq, x, rms_w, qs, bias, N, K, qcols, n_blk, t));  // with the logit bias
}

// Pass 2: T over every block, then this workgroup's blocks blockIdx.x + j * gridDim.x (at most 256) that pass hi_b >= T,
// rescored in ascending order; one (value, row) partial per workgroup.  No workgroup waits for another.
struct LmHeadRescoreTail {
  const float* bias; float* out; int fast_math;
  ArgmaxPartials part;
  int* stats;  // [2] += candidate blocks, += 1 per step (never read by the step)
};
template <int PR, int KI>
__global__ __launch_bounds__(256) void lm_head_rescore_kernel(const float* blk_lo, const float* blk_hi, const uint16_t* W, const float* x,
                                                              const float* rms_w, int n_blk, int N, int K, float eps, LmHeadRescoreTail tl) {
  GemvArgs g{};
  g.W = W; g.x = x; g.rms_w = rms_w; g.N = N; g.K = K; g.eps = eps;
  g.bias = tl.bias; g.out = tl.out; g.fast_math = tl.fast_math; g.part = tl.part; g.mode = 3;
  __shared__ float am_v[4][1];
  __shared__ int am_i[4][1];
  __shared__ float red[4];
  __shared__ int cand[256];
  constexpr int PRE = 10;  // float4 of block minima per thread in the first batch (40 960 blocks); more are folded by the loop below
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = n_blk, n4 = (nb + 3) / 4, G = gridDim.x;
  const float4* lo4 = reinterpret_cast<const float4*>(blk_lo);
  float4 lv[PRE];
#pragma unroll
  for (int j = 0; j < PRE; ++j) {
    const int i4 = tid + j * 256;
    lv[j] = lo4[i4 < n4 ? i4 : n4 - 1];
  }
  const int mb = blockIdx.x + tid * G;  // this thread's block
  const float hv = blk_hi[mb < nb ? mb : nb - 1];
  float t = -INFINITY;
  auto fold = [&](const float4& v, int i4) {
    const int i = i4 * 4;
    if (i < nb) t = fmaxf(t, v.x);
    if (i + 1 < nb) t = fmaxf(t, v.y);
    if (i + 2 < nb) t = fmaxf(t, v.z);
    if (i + 3 < nb) t = fmaxf(t, v.w);
  };
#pragma unroll
  for (int j = 0; j < PRE; ++j) fold(lv[j], tid + j * 256);
  for (int i4 = tid + PRE * 256; i4 < n4; i4 += 256) fold(lo4[i4], i4);
  t = wave_max(t);
  if (lane == 0) red[wave] = t;
  cand[tid] = 0;
  __syncthreads();
  const float T = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  if (mb < nb) cand[tid] = !(hv < T);
  __syncthreads();
  const int nj = (nb - blockIdx.x + G - 1) / G;
  ArgmaxAcc<false> best;
  int nc = 0;
  for (int j = 0; j < nj; ++j) {
    if (!cand[j]) continue;  // uniform
    ArgmaxAcc<false> r;
    gemv1_head_block<PR, KI>(g, blockIdx.x + j * G, am_v, am_i, nullptr, r);
    if (tid == 0) best.merge(r);
    ++nc;
    __syncthreads();  // am_v / am_i are reused by the next candidate
  }
  if (tid == 0) {
    best.store(g.part, 0, blockIdx.x);
    if (tl.stats) {
      if (nc) atomicAdd(&tl.stats[0], nc);
      if (blockIdx.x == 0) atomicAdd(&tl.stats[1], 1);
    }
  }
}

// ---- NB in {2, 4}: x staged through LDS once per workgroup ---------------------------------------------
template <int NB, int PR, int PF, bool LP = false>
__global__ __launch_bounds__(256) void gemvn_kernel(GemvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [NB][K]
  __shared__ float red[NB][4];
  __shared__ float am_v[4][NB];
  __shared__ int am_i[4][NB];
  __shared__ float am_s[LP ? 4 : 1][NB];  // (LP only)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K;
  const int g = blockIdx.x * 4 + wave;
  int prow[PR];
  gemv_rows<PR>(a, g, prow);
  bool kin[PF];  // the first PF k-iterations are requested up front, on the one-sequence column plan
  int kk[PF];
  lane_cols<PF>(lane, K, kin, kk);
  uint4 wq[PF][PR];
  request_rows<PF, PR>(a, prow, kk, wq);
  __shared__ AttnTables f_s;
  if (a.attn_po) attn_scales(a, NB, f_s);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    float ss = 0.f;
    for (int k = tid * 8; k < K; k += 2048) {
      float x[8];
      if (a.attn_po) {
        attn_combined8(a, b, k, f_s, x);
      } else {
        const float4 v0 = *reinterpret_cast<const float4*>(a.x + (size_t)b * a.ldx + k);
        const float4 v1 = *reinterpret_cast<const float4*>(a.x + (size_t)b * a.ldx + k + 4);
        x[0] = v0.x; x[1] = v0.y; x[2] = v0.z; x[3] = v0.w; x[4] = v1.x; x[5] = v1.y; x[6] = v1.z; x[7] = v1.w;
      }
      if (a.rms_w) {
        const float4 w0 = *reinterpret_cast<const float4*>(a.rms_w + k);
        const float4 w1 = *reinterpret_cast<const float4*>(a.rms_w + k + 4);
        const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) { ss += x[e] * x[e]; x[e] *= wv[e]; }
      }
      *reinterpret_cast<float4*>(xs + (size_t)b * K + k) = make_float4(x[0], x[1], x[2], x[3]);
      *reinterpret_cast<float4*>(xs + (size_t)b * K + k + 4) = make_float4(x[4], x[5], x[6], x[7]);
    }
    if (a.rms_w) {
      ss = wave_sum_fast(ss);
      if (lane == 0) red[b][wave] = ss;
    }
  }
  __syncthreads();
  float acc[PR][NB];
#pragma unroll
  for (int i = 0; i < PR; ++i)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[i][b] = 0.f;
  auto fma_all = [&](const uint4 (&w)[PR], int k) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float4 xa = *reinterpret_cast<const float4*>(xs + (size_t)b * K + k);
      const float4 xb = *reinterpret_cast<const float4*>(xs + (size_t)b * K + k + 4);
      const float x[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
#pragma unroll
      for (int i = 0; i < PR; ++i) acc[i][b] = dot8(w[i], x, acc[i][b]);
    }
  };
#pragma unroll
  for (int it = 0; it < PF; ++it)
    if (kin[it]) fma_all(wq[it], kk[it]);
  for (int k = lane * 8 + PF * 512; k < K; k += 512) {
    uint4 w[PR];
#pragma unroll
    for (int i = 0; i < PR; ++i) w[i] = ld_w16(a, prow[i], k);
    fma_all(w, k);
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    float rstd = 1.0f;
    if (a.rms_w) rstd = rstd_of((red[b][0] + red[b][1] + red[b][2] + red[b][3]) / (float)K + a.eps, a.fast_math != 0);
#pragma unroll
    for (int i = 0; i < PR; ++i) acc[i][b] = wave_sum_fast(acc[i][b]) * rstd;
  }
  gemv_epilogue<NB, PR, LP>(a, g, prow, acc, am_v, am_i, am_s);
}

// the kernels' flat heads and tails, in the order of their signatures
#define GEMV_PLAIN_ARGS(a) (a).W, (a).x, (a).rms_w, (a).bias, (a).resid, (a).N, (a).K, (a).mode, (a).eps, gemv_tail(a)
#define GEMV_ATTN_ARGS(a) (a).attn_pm, (a).attn_pl, (a).attn_po, (a).W, (a).resid, (a).N, (a).K, (a).attn_nsplit, (a).mode, gemv_attn_tail(a)
#define GEMV_HEAD_ARGS(a) (a).W, (a).x, (a).rms_w, (a).bias, (a).out, (a).N, (a).K, (a).eps, (a).fast_math, (a).part
GemvTail gemv_tail(const GemvArgs& a) {
  GemvTail t{};
  t.out = a.out; t.fast_math = a.fast_math;
  Q3A_STAMP_COPY(t, a);
  return t;
}
GemvAttnTail gemv_attn_tail(const GemvArgs& a) {
  GemvAttnTail t{};
  t.out = a.out; t.bias = a.bias; t.attn_heads = a.attn_heads; t.attn_fast_exp = a.attn_fast_exp; t.fast_math = a.fast_math;
  Q3A_STAMP_COPY(t, a);
  return t;
}

template <int PR, int KI>
void launch1k(const GemvArgs& a, hipStream_t s) {
  const dim3 grid(gemv_blocks(a)), block(256);
  // up to 8 key splits (contexts up to 1024 keys): the merge's partials go in FRONT of the weight stream (round 6: -1.2 % per step at
  // 0.6B x 1 and x 2, neutral at 1.7B; profiles/r6_ab_merge_first.txt); beyond, the chunked merge behind it
  if (a.attn_po) {
    if constexpr (KI <= 4) {  // (not instantiated beyond: never launched)
      if (a.attn_nsplit <= 4) { hipLaunchKernelGGL((gemv1_kernel<PR, KI, false, true, 4>), grid, block, 0, s, GEMV_ATTN_ARGS(a)); return; }
      if (a.attn_nsplit <= 8) { hipLaunchKernelGGL((gemv1_kernel<PR, KI, false, true, 8>), grid, block, 0, s, GEMV_ATTN_ARGS(a)); return; }
    }
    hipLaunchKernelGGL((gemv1_kernel<PR, KI, false, true>), grid, block, 0, s, GEMV_ATTN_ARGS(a));
  } else if (a.rms_w) {
    // Norm-fused projections at K <= 1024 (qkv, gate / up at hidden 1024): x and the norm weight once per workgroup through LDS
    // (round 6: 609.7 -> 595.1 us per step at 0.6B, ids identical; profiles/r6_ab_gemv_x_lds.txt).  Not where it was measured to
    // lose: K = 2048 (+18 %: 32 KiB of LDS per workgroup halves the residency of the 1536-workgroup gate / up launch), the lm_head
    // (+1.3 %: a barrier in each of 9496 workgroups).
    // The down projection (the plain form below, K > 2048) lost 4 % in that round's trial, which was put down to x standing in front
    // of the weights without a look at its assembly.  The hand-over as it then stood, instantiated with more than one 16-byte piece
    // per lane, compiles with the pieces in scratch (the aggregate copy into LDS; it now copies element by element), which that trial
    // may have measured.  Rebuilt without scratch, both request orders were stamped: x in front of the weights wins, x behind them
    // loses (gemv1_body XH; profiles/gemv_down_handover_phase_probe.txt, gemv_down_handover_headline_ab.txt).
    if (a.mode == 3) {
      if (a.part.sum) hipLaunchKernelGGL((gemv1_head_kernel<PR, KI, true>), grid, block, 0, s, GEMV_HEAD_ARGS(a));
      else hipLaunchKernelGGL((gemv1_head_kernel<PR, KI>), grid, block, 0, s, GEMV_HEAD_ARGS(a));
      return;
    }
    if constexpr (KI == 2) {
      if constexpr (PR == 2) {  // (launch_gemv has checked: mode 2, which runs two rows per wave)
        if (a.x_parts) {
          GemvXpTail t{};
          t.out = a.out; t.x_out = a.x_out; t.fast_math = a.fast_math;
          Q3A_STAMP_COPY(t, a);
          // one logical row (gate and up) per wave, GEMV_XP_WAVES waves per workgroup: rows past N / 2 are clamped and not stored
          const dim3 xp_grid((a.N / 2 + GEMV_XP_WAVES - 1) / GEMV_XP_WAVES), xp_block(GEMV_XP_WAVES * 64);
                    hipLaunchKernelGGL((gemv1_xp_kernel<PR, KI, GEMV_XP_WAVES>), xp_grid, xp_block, 0, s, a.W, a.x, a.rms_w, a.x_parts, a.bias, a.N, a.K, a.x_nparts,
                             a.eps, t);
          return;
        }
      }
      hipLaunchKernelGGL((gemv1_kernel<PR, KI, true, false, 0, true>), grid, block, 0, s, GEMV_PLAIN_ARGS(a));
    } else {  // (an `else`, not a statement behind a return: there the register form was instantiated at KI = 2 as well, three kernels nothing launches)
      hipLaunchKernelGGL((gemv1_kernel<PR, KI, true, false>), grid, block, 0, s, GEMV_PLAIN_ARGS(a));
    }
  } else {
    hipLaunchKernelGGL((gemv1_kernel<PR, KI, false, false>), grid, block, 0, s, GEMV_PLAIN_ARGS(a));
  }
}
template <int PR>
void launch1(const GemvArgs& a, hipStream_t s) {
  if (a.K <= 1024) launch1k<PR, 2>(a, s);
  else if (a.K <= 2048) launch1k<PR, 4>(a, s);
  else if constexpr (PR < 4) {  // gemv_rows_per_wave keeps 4 rows per wave to K <= 2048 (registers)
    if (a.K <= 3072) launch1k<PR, 6>(a, s); else launch1k<PR, 12>(a, s);
  }
}
template <int NB, int PR, int PF>
void launchn(const GemvArgs& a, hipStream_t s) {
  if (a.part.sum) hipLaunchKernelGGL((gemvn_kernel<NB, PR, PF, true>), dim3(gemv_blocks(a)), dim3(256), (size_t)NB * a.K * sizeof(float), s, a);
  else hipLaunchKernelGGL((gemvn_kernel<NB, PR, PF>), dim3(gemv_blocks(a)), dim3(256), (size_t)NB * a.K * sizeof(float), s, a);
}

}  // namespace

int lm_head_prune_blocks(const GemvArgs& g) { return (g.N + 15) / 16; }
const char* launch_lm_head_quantize(const uint16_t* W, int N, int K, int8_t* Q, float* qs, hipStream_t s) {
  const int cols = lm_head_q_cols(K);
  if (cols == 0 || K % 8 != 0) return "lm_head_quantize: hidden size beyond the one-sequence GEMV";
  if (hipMemsetAsync(Q, 0, (size_t)N * cols, s) != hipSuccess) return "lm_head_quantize: memset failed";
  hipLaunchKernelGGL(lm_head_quantize_kernel, dim3((N + 3) / 4), dim3(256), 0, s, W, N, K, cols, Q, qs);
  return nullptr;
}
const char* lm_head_prune_check(const LmHeadPruneArgs& a) {
  const GemvArgs& g = a.g;
  if (g.mode != 3 || !g.rms_w || !g.x || g.attn_po) return "lm_head_prune: needs the plain mode-3 GEMV with a fused norm";
  if (g.bias && !a.logit_bias) return "lm_head_prune: the only bias the bound covers is the logit bias (finite or -inf entries)";
  if (g.part.sum) return "lm_head_prune: token log-probabilities need every logit (the full GEMV)";
  if (gemv_rows_per_wave(g) != 4 || gemv_blocks(g) != lm_head_prune_blocks(g)) return "lm_head_prune: the GEMV does not run 16-row blocks here";
  if (g.K % 8 != 0 || a.qcols != lm_head_q_cols(g.K)) return "lm_head_prune: int8 row width does not match the hidden size";
  if (!a.Wq || !a.qs || !a.blk_lo || !a.blk_hi || !g.part.val) return "lm_head_prune: missing buffer";
  if (const char* e = argmax_partials_check(g.part, 1)) return e;  // (the rescore grid against the stride: launch_lm_head_rescore)
  return nullptr;
}
const char* launch_lm_head_approx(const LmHeadPruneArgs& a, hipStream_t s) {
  if (const char* e = lm_head_prune_check(a)) return e;
  const GemvArgs& g = a.g;
  const int n_blk = lm_head_prune_blocks(g);
  const dim3 grid((n_blk + 3) / 4), block(256);
  const double nu = (double)a.qcols * 0x1p-24;  // γ of the bound above, n = cols
  const LmHeadApproxTail t{g.eps, g.fast_math, (float)(nu / (1.0 - nu)) * (1.0f + 0x1p-20f), a.blk_lo, a.blk_hi, a.dbg};
#define LM_HEAD_APPROX_ARGS a.Wq, g.x, g.rms_w, a.qs, g.bias, g.N, g.K, a.qcols, n_blk, t
  if (a.g.bias) {
    if (a.qcols == 1024) hipLaunchKernelGGL(lm_head_approx_bias_kernel<2>, grid, block, 0, s, LM_HEAD_APPROX_ARGS);
    else hipLaunchKernelGGL(lm_head_approx_bias_kernel<4>, grid, block, 0, s, LM_HEAD_APPROX_ARGS);
  } else {
    if (a.qcols == 1024) hipLaunchKernelGGL(lm_head_approx_kernel<2>, grid, block, 0, s, LM_HEAD_APPROX_ARGS);
    else hipLaunchKernelGGL(lm_head_approx_kernel<4>, grid, block, 0, s, LM_HEAD_APPROX_ARGS);
  }
#undef LM_HEAD_APPROX_ARGS
  return nullptr;
}
int lm_head_rescore_groups(const GemvArgs& g, int n_cu) {
  const int nb = lm_head_prune_blocks(g);
  return std::min(nb, std::max(n_cu > 0 ? n_cu : 256, (nb + 255) / 256));
}
const char* launch_lm_head_rescore(const LmHeadPruneArgs& a, int groups, hipStream_t s) {
  if (const char* e = lm_head_prune_check(a)) return e;
  const GemvArgs& g = a.g;
  const int n_blk = lm_head_prune_blocks(g);
  if (groups < 1 || groups > g.part.stride || (n_blk + groups - 1) / groups > 256) return "lm_head_prune: bad rescore grid";
  const LmHeadRescoreTail t{g.bias, g.out, g.fast_math, g.part, a.stats};
#define LM_HEAD_RESCORE_ARGS a.blk_lo, a.blk_hi, g.W, g.x, g.rms_w, n_blk, g.N, g.K, g.eps, t
  if (a.qcols == 1024) hipLaunchKernelGGL((lm_head_rescore_kernel<4, 2>), dim3(groups), dim3(256), 0, s, LM_HEAD_RESCORE_ARGS);
  else hipLaunchKernelGGL((lm_head_rescore_kernel<4, 4>), dim3(groups), dim3(256), 0, s, LM_HEAD_RESCORE_ARGS);
#undef LM_HEAD_RESCORE_ARGS
  return nullptr;
}

const char* oproj_head_check(const OprojHeadArgs& a) {
  if (!a.pm || !a.pl || !a.po || !a.W || !a.y_part || a.N < 1) return "oproj_head: missing buffer";
  if (a.N > 1024) return "oproj_head: N <= 1024 (the gate / up form that adds the partial vectors exists at K <= 1024)";
  if (a.nsplit < 1 || a.nsplit > OPROJ_HEAD_MAX_SPLITS) return "oproj_head: 1 .. 16 key splits (more: the merging o_proj of launch_gemv)";
  if (a.n_parts < 1 || a.K != a.n_parts * 512) return "oproj_head: a slice is 512 columns (two kv heads of two q heads)";
  return nullptr;
}
const char* launch_oproj_head(const OprojHeadArgs& a, hipStream_t s) {
  if (const char* e = oproj_head_check(a)) return e;
  OprojHeadTail t{};
  t.bias = a.bias;
  Q3A_STAMP_COPY(t, a);
  // 4 slices x 16-row blocks: 256 workgroups at N = 1024, the only hidden size the chain runs at (the gate / up form behind it
  // exists at K <= 1024)
  constexpr int rb = 16;
  const dim3 grid(a.n_parts * ((a.N + rb - 1) / rb)), block(256);
#define OPROJ_HEAD_ARGS a.pm, a.pl, a.po, a.W, a.y_part, a.N, a.K, a.nsplit, a.n_parts, t
  hipLaunchKernelGGL((oproj_head_kernel<512, rb>), grid, block, 0, s, OPROJ_HEAD_ARGS);
#undef OPROJ_HEAD_ARGS
  return nullptr;
}

const char* launch_gemv(const GemvArgs& a0, int NB, hipStream_t s) {
  if (a0.K % 8 != 0) return "gemv: K must be a multiple of 8";
  if (a0.K > 6144) return "gemv: K > 6144 unsupported";
  if (a0.mode == 2 && a0.N % 32 != 0) return "gemv: GLU needs N % 32 == 0";
  if (a0.mode == 3 && !a0.rms_w) return "gemv: mode 3 (the lm_head) needs the fused final norm";
  if (a0.mode == 3 && !a0.part.val) return "gemv: argmax partial buffer missing";
  if (const char* e = argmax_partials_check(a0.part, a0.mode == 3 ? gemv_blocks(a0) : 0)) return e;
  if (a0.part.sum && a0.mode != 3) return "gemv: log-sum partials need mode 3";
  if (a0.attn_po && (a0.K % 128 != 0 || a0.K != a0.attn_heads * 128)) return "gemv: attention-partial input needs K = heads*128";
  if (a0.attn_po && a0.rms_w) return "gemv: attention-partial input cannot be combined with a fused RMSNorm";
  if (a0.attn_po && (NB < 4 ? NB : 4) * a0.attn_heads * a0.attn_nsplit > ATTN_F_MAX) return "gemv: too many attention splits for the LDS scale table";
  if (a0.x_parts && (NB != 1 || !a0.x || !a0.rms_w || a0.mode != 2 || a0.K > 1024 || a0.x_nparts < 1 || a0.x_nparts > GEMV_X_PARTS_MAX || !a0.x_out))
    return "gemv: partial vectors are added in the one-sequence norm-fused GLU form at K <= 1024 only (1 .. 4 vectors, x_out set)";
  const int pr = gemv_rows_per_wave(a0);
  const int nb_cap = (int)((64 * 1024) / ((size_t)a0.K * 4));  // rows of x that fit in 64 KiB of LDS
  int done = 0;
  while (done < NB) {
    GemvArgs a = a0;
    if (a0.x) a.x = a0.x + (size_t)done * a0.ldx;
    if (a0.out) a.out = a0.out + (size_t)done * a0.ldo;
    if (a0.resid) a.resid = a0.resid + (size_t)done * a0.ldo;
    a.part = a0.part.at(done);
    if (a0.attn_po) {
      const size_t adv = (size_t)done * a0.attn_heads * a0.attn_nsplit;
      a.attn_pm = a0.attn_pm + adv; a.attn_pl = a0.attn_pl + adv; a.attn_po = a0.attn_po + adv * 128;
    }
    int nb = NB - done;
    if (nb >= 4 && nb_cap >= 4) nb = 4;
    else if (nb >= 2 && nb_cap >= 2) nb = 2;
    else nb = 1;
    if (nb == 1) {
      if (pr == 4) launch1<4>(a, s); else if (pr == 2) launch1<2>(a, s); else launch1<1>(a, s);
    } else if (nb == 2) {
      if (pr == 4) launchn<2, 4, 2>(a, s); else if (pr == 2) launchn<2, 2, 4>(a, s); else launchn<2, 1, 6>(a, s);
    } else {
      if (pr == 4) launchn<4, 4, 2>(a, s); else if (pr == 2) launchn<4, 2, 4>(a, s); else launchn<4, 1, 6>(a, s);
    }
    done += nb;
  }
  return nullptr;
}

}  // namespace q3a
