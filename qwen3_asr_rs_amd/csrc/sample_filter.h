// Top-k / top-p of the sampled step (include/q3asr.h "sampling filter"): the threshold stage and the filtered
// draw as device functions, 256 threads each.  k_sample.hip wraps each in a kernel of its own (sample_hist_kernel,
// sample_select_kernel, sample_chunk_filter_kernel); the key, the row maximum and u64 are shared with the top log-probabilities
// (k_toplp.hip), which is why this is a header.
#pragma once
#include "argmax.h"
#include "sample_rng.h"

namespace q3a {

namespace {

// ---- top-k / top-p: the threshold stage (include/q3asr.h "sampling filter") ------------------------------
// An exact radix select over key(l), the uint32 whose unsigned order is the order of the fp32 values: 11 + 11 + 10 bits.
//   sample_hist_phase      the chunk grid: count and summed weight of every first digit (top 11 key bits) of one 2048-logit chunk in
//                          LDS, then one integer atomic per non-empty bucket into the row's table.
//   sample_select_phase    one workgroup per row: walks the table downwards to the bucket that holds the k-th largest entry, resolves
//                          the other 21 bits in two passes over the row that histogram only the entries under the prefix found so
//                          far; the same again for top-p on the weights, over the entries >= tau_k.  Leaves the table zero.
// Counts are uint32, weights uint64 fixed point (w 2^40 truncated; w <= 1, so a row sums to less than 2^58): integer adds commute,
// so neither the atomics' arrival order nor the launch form changes a bit of tau.
using u64 = unsigned long long;

__device__ __forceinline__ uint32_t sel_key(float l) {
  uint32_t u = __float_as_uint(l);
  if (u == 0x80000000u) u = 0u;  // -0.0 and +0.0 are one value: one key
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // negative floats order backwards
}
__device__ __forceinline__ float sel_value(uint32_t key) { return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key); }
// w = exp((l - m) / T) in fixed point; l <= m, so w <= 2^40; -inf weighs 0.  ONE definition: both kernels must agree to the bit.
__device__ __forceinline__ u64 sel_weight(float l, float m, float T) { return (u64)(expf((l - m) / T) * 0x1p40f); }
// the row maximum from the chunk maxima (a maximum: any order gives the same bits); every lane of the wave gets it
__device__ __forceinline__ float sel_row_max(const float* __restrict__ chunk_max, int s, int n_chunk, int lane) {
  float m = -INFINITY;
  for (int x = lane; x < n_chunk; x += 64) m = fmaxf(m, chunk_max[(size_t)s * n_chunk + x]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  return m;
}

template <bool VEC>
__device__ __forceinline__ void sample_hist_phase(uint32_t* cnt, u64* mass, const float* __restrict__ logits, int V, int n_chunk, const uint32_t* __restrict__ params,
                                                          const uint32_t* __restrict__ filter, int row_stride, const float* __restrict__ chunk_max,
                                                          uint32_t* __restrict__ hist_cnt, u64* __restrict__ hist_mass) {
  const int s = blockIdx.y, c = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const float* row = logits + (size_t)s * V;
  const int base = c * SAMPLE_CHUNK;
  float f[8];
  if constexpr (VEC) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = base + q * 1024 + tid * 4;
      const float4 v = e < V ? *reinterpret_cast<const float4*>(row + e) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      f[q * 4] = v.x; f[q * 4 + 1] = v.y; f[q * 4 + 2] = v.z; f[q * 4 + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = base + q * 256 + tid;
      f[q] = e < V ? row[e] : -INFINITY;  // (-inf: counted nowhere)
    }
  }
  for (int b = tid; b < SAMPLE_BUCKETS; b += 256) { cnt[b] = 0u; mass[b] = 0ull; }
  const float T = __uint_as_float(params[(size_t)s * row_stride]);  // the row's own records (stride 0: the one record of all rows)
  // top-p off: nobody reads the weights; a greedy row of a row table (T = 0) has no filter, and sel_weight divides by T
  const bool weigh = __uint_as_float(filter[(size_t)s * row_stride + 1]) < 1.f && T > 0.f;
  const float m = sel_row_max(chunk_max, s, n_chunk, lane);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    if (f[q] != -INFINITY) {
      const uint32_t b = sel_key(f[q]) >> 21;
      atomicAdd(&cnt[b], 1u);
      if (weigh) atomicAdd(&mass[b], sel_weight(f[q], m, T));
    }
  }
  __syncthreads();
  for (int b = tid; b < SAMPLE_BUCKETS; b += 256) {
    if (cnt[b]) {
      atomicAdd(&hist_cnt[(size_t)s * SAMPLE_BUCKETS + b], cnt[b]);
      if (mass[b]) atomicAdd(&hist_mass[(size_t)s * SAMPLE_BUCKETS + b], mass[b]);
    }
  }
}

// LDS tables of the select: bucket i at i + i / 32, so the 64 lanes that each walk 32 consecutive buckets start on different banks
constexpr int SEL_TABLE = SAMPLE_BUCKETS + SAMPLE_BUCKETS / 32;
__device__ __forceinline__ int sel_pad(int i) { return i + (i >> 5); }

struct SelWalk { int found; int bucket; uint32_t cnt_above; u64 mass_above; };  // sums over the buckets ABOVE `bucket`

// One wave, all 64 lanes: lane i owns buckets 2047 - 32 i downwards.  Sums of its 32 buckets and of all lanes before it.
__device__ __forceinline__ void sel_prefix(const uint32_t* cnt, const u64* mass, int lane, uint32_t& ce, u64& me, uint32_t& ci, u64& mi) {
  const int top = SAMPLE_BUCKETS - 1 - 32 * lane;
  uint32_t c = 0u;
  u64 w = 0ull;
#pragma nounroll
  for (int j = 0; j < 32; ++j) { c += cnt[sel_pad(top - j)]; w += mass[sel_pad(top - j)]; }
  ci = c; mi = w;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t tc = __shfl_up(ci, o, 64);
    const u64 tw = __shfl_up(mi, o, 64);
    if (lane >= o) { ci += tc; mi += tw; }
  }
  ce = ci - c; me = mi - w;
}
// The boundary bucket of a table, walked from the top.
//   by count (top-k): the bucket in which the running count reaches `need` (>= 1); not found: the table holds fewer entries.
//   by mass (top-p):  the LOWEST non-empty bucket >= min_bucket whose mass above it (base + the table's) is still under P.  The mass
//                     above grows downwards, so every non-empty bucket over that one qualifies too and none under it does.
__device__ __forceinline__ SelWalk sel_walk(const uint32_t* cnt, const u64* mass, bool by_mass, uint32_t need, u64 base, u64 P, int min_bucket, int lane) {
  uint32_t ce, ci;
  u64 me, mi;
  sel_prefix(cnt, mass, lane, ce, me, ci, mi);
  const int top = SAMPLE_BUCKETS - 1 - 32 * lane;
  int b = -1;
  uint32_t bc = 0u;
  u64 bm = 0ull;
#pragma nounroll
  for (int j = 0; j < 32; ++j) {
    const uint32_t x = cnt[sel_pad(top - j)];
    const bool hit = by_mass ? (x && top - j >= min_bucket && base + me < P) : (b < 0 && ce + x >= need);
    if (hit) { b = top - j; bc = ce; bm = me; }
    ce += x; me += mass[sel_pad(top - j)];
  }
  const u64 who = __ballot(b >= 0);
  SelWalk r{0, 0, 0u, 0ull};
  if (!who) return r;
  const int src = by_mass ? 63 - __clzll((long long)who) : __ffsll((long long)who) - 1;  // the lowest bucket / the first to reach the count
  r.found = 1; r.bucket = __shfl(b, src, 64); r.cnt_above = __shfl(bc, src, 64); r.mass_above = __shfl(bm, src, 64);
  return r;
}

__device__ __forceinline__ void sample_select_phase(uint32_t* cnt0, u64* mass0, uint32_t* cnt1, u64* mass1, const float* __restrict__ logits, int V, int n_chunk, int vec, const uint32_t* __restrict__ params,
                                                             const uint32_t* __restrict__ filter, int row_stride, const float* __restrict__ chunk_max,
                                                             uint32_t* __restrict__ hist_cnt, u64* __restrict__ hist_mass,
                                                             float* __restrict__ tau_sel, int* __restrict__ kept) {
  __shared__ SelWalk walk;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = logits + (size_t)s * V;
  const float T = __uint_as_float(params[(size_t)s * row_stride]);  // the row's own records (stride 0: the one record of all rows)
  const uint32_t top_k = filter[(size_t)s * row_stride];
  const float top_p = __uint_as_float(filter[(size_t)s * row_stride + 1]);
  // a greedy row of a row table (T = 0) is not filtered: its table is still read and zeroed, tau = -inf, kept = the finite count
  const bool sampled = T > 0.f, k_on = sampled && top_k >= 1u && top_k < (uint32_t)V, p_on = sampled && top_p < 1.f;
  const float m = sel_row_max(chunk_max, s, n_chunk, lane);
  for (int b = tid; b < SEL_TABLE; b += 256) { cnt0[b] = 0u; mass0[b] = 0ull; }  // (the padding words too: nothing here is left unset)
  __syncthreads();
  for (int b = tid; b < SAMPLE_BUCKETS; b += 256) {
    const size_t g = (size_t)s * SAMPLE_BUCKETS + b;
    cnt0[sel_pad(b)] = hist_cnt[g]; mass0[sel_pad(b)] = hist_mass[g];
    hist_cnt[g] = 0u; hist_mass[g] = 0ull;  // the next step's histogram adds into zeros
  }
  __syncthreads();
  // wave 0 walks, everybody reads the result
  auto share = [&](const SelWalk& r) {
    if (tid == 0) walk = r;
    __syncthreads();
    const SelWalk got = walk;
    __syncthreads();
    return got;
  };
  // nothing cut: every finite entry, and the weight of all of them
  uint32_t key_tau = 0u, n_kept;  // key_tau = 0: no threshold yet (no value's key is 0: that is a NaN's)
  u64 Z;
  {
    SelWalk t{};
    if (wave == 0) {
      uint32_t ce, ci;
      u64 me, mi;
      sel_prefix(cnt0, mass0, lane, ce, me, ci, mi);
      t.cnt_above = __shfl(ci, 63, 64); t.mass_above = __shfl(mi, 63, 64);
    }
    t = share(t);
    n_kept = t.cnt_above; Z = t.mass_above;
  }
  int bucket_k = 0;
  bool cut = false;
  // stage 0, top-k: the key of the top_k-th largest entry, by counts.  stage 1, top-p: over the entries >= that key, the smallest key
  // whose mass above is under top_p Z, by weights.  Either way 11 + 11 + 10 bits: the first digit from the row's table, the others from
  // a pass over the row each, which histograms the entries under the prefix found so far.
#pragma nounroll
  for (int stage = 0; stage < 2; ++stage) {
    const bool by_mass = stage == 1;
    if (by_mass ? !(p_on && Z > 0ull) : !k_on) continue;
    u64 P = 0ull;
    if (by_mass) {
      // G(v) < top_p  <=>  mass above v < top_p Z  <=>  (integers) mass above v < ceil(top_p Z); fp64 holds Z to 2^-53
      const double pz = (double)top_p * (double)Z;
      P = (u64)pz;
      if ((double)P < pz) ++P;
    }
    const uint32_t floor = key_tau;  // top-p sees the top-k set only
    uint32_t above = 0u, prefix = 0u;
    u64 mabove = 0ull;
#pragma nounroll
    for (int level = 0; level < 3; ++level) {
      const uint32_t* cnt = level ? cnt1 : cnt0;
      const u64* mass = level ? mass1 : mass0;
      if (level) {
        const int shift = level == 1 ? 21 : 10, dshift = level == 1 ? 10 : 0;
        const uint32_t dmask = level == 1 ? 2047u : 1023u;
        for (int b = tid; b < SEL_TABLE; b += 256) { cnt1[b] = 0u; mass1[b] = 0ull; }
        __syncthreads();
        auto visit = [&](float l) {
          const uint32_t key = sel_key(l);
          if (l != -INFINITY && (key >> shift) == prefix && key >= floor) {
            const int d = sel_pad((int)((key >> dshift) & dmask));
            atomicAdd(&cnt1[d], 1u);
            if (p_on) atomicAdd(&mass1[d], sel_weight(l, m, T));
          }
        };
        if (vec) {  // V % 4 == 0: 16-byte loads, four of them in flight per thread -- one workgroup has the whole row to read
          const float4* row4 = reinterpret_cast<const float4*>(row);
#pragma unroll 8
          for (int e = tid; e < (V >> 2); e += 256) {
            const float4 f = row4[e];
            visit(f.x); visit(f.y); visit(f.z); visit(f.w);
          }
        } else {
#pragma unroll 4
          for (int e = tid; e < V; e += 256) visit(row[e]);
        }
        __syncthreads();
      }
      SelWalk r{};
      if (wave == 0) r = sel_walk(cnt, mass, by_mass, top_k - above, mabove, P, level == 0 && cut ? bucket_k : 0, lane);
      r = share(r);
      if (!r.found) break;  // (the first digit of top-k only: fewer than top_k finite entries, every one of them stays)
      above += r.cnt_above; mabove += r.mass_above;
      prefix = (prefix << (level == 2 ? 10 : 11)) | (uint32_t)r.bucket;
      if (level == 0 && !by_mass) bucket_k = r.bucket;
      if (level == 2) {  // every entry that ties the boundary value stays: equal values share their fate
        key_tau = prefix; cut = true;
        n_kept = above + cnt[sel_pad(r.bucket)];
        Z = mabove + mass[sel_pad(r.bucket)];
      }
    }
  }
  if (tid == 0) {
    tau_sel[s] = cut ? sel_value(key_tau) : -INFINITY;
    kept[s] = (int)n_kept;
  }
}

// sample_chunk_kernel (k_sample.hip) with one more input: kept iff l >= max(thr_minp, tau_sel[s]).  Its own text, not a parameter of that
// kernel: the filter-off kernels stay the code objects they were.
template <bool VEC>
__device__ __forceinline__ void sample_chunk_filter_phase(const SampleArgs& a, int n_chunk, const float* __restrict__ tau_sel) {
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
  const float thr = greedy ? -INFINITY : fmaxf(m + T * logf(min_p), tau_sel[s]);  // tau = max(tau_minp, tau_k, tau_p): a value, never a rank
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

// Dynamic LDS of the two: the histogram's mass[SAMPLE_BUCKETS] then cnt[SAMPLE_BUCKETS] (24 KB); the select's mass0, mass1, cnt0, cnt1
// of SEL_TABLE words each (2 x 24.75 KB).  The 64-bit tables come first: the launch's LDS is 16-byte aligned.
constexpr size_t SAMPLE_HIST_LDS = (size_t)SAMPLE_BUCKETS * 12, SAMPLE_SELECT_LDS = (size_t)SEL_TABLE * 24;

}  // namespace

}  // namespace q3a
