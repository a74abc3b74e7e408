// Forced-aligner head (kernels.h AlignHeadArgs): at the marker rows of the aligner prompt, the final RMSNorm, the classifier
// [classify_num][hidden] and the argmax over the time classes.  Three launches:
//   1. align_norm_kernel: one wave per marker row gathers the row from the residual stream, applies the final RMSNorm in fp32
//      (k_norm.hip's arithmetic) and writes bf16 operand planes: plane 0 = bf16(y); in the precise mode plane 1 = bf16(y - plane 0),
//      the hi + lo split of k_gemm.hip.  Rows M .. padded(M) are written as zeros, so the GEMM reads whole 64-row tiles.
//   2. align_head_kernel: 64 x 128 output tiles, 4 waves as 2 (rows) x 2 (columns) of 32 x 64, mfma_f32_16x16x32_bf16 over
//      64-deep K tiles staged in LDS (registers prefetch tile k + 1 while tile k is multiplied).  Every plane accumulates into the
//      same fp32 accumulators.  Epilogue: one argmax partial per row and 64-column strip (col = 2 * tile + wave column), the logits
//      only when asked for.
//   3. align_merge_kernel: one thread per row merges its partials in column order -> class.
// The tie rule (larger value, then smaller index) is argmax.h ArgmaxAcc's.
//
// Scoring head (kernels.h ScoreHeadArgs): the same norm launch and the same 64 x 128 tile (head_tile<.., LP = true>) against the
// vocabulary lm_head at the rows that predict a given transcript.  The M x vocab logits are never stored (unless asked for): per row
// and 64-column strip the epilogue leaves one (max, first index, sum exp(l - max)) partial, and the one lane that holds column
// target[row] stores that accumulator to tgt_logit[row] (single writer).  score_head_kernel walks the tiles M fastest inside the
// contiguous chunk of tile ids its XCD receives, so the row tiles that share a 128-row slab of the lm_head run together on one L2.
// score_merge_kernel: one wave per row merges the row's partials (lane l takes partials l, l + 64, ... in ascending order, then the
// xor butterfly 32 .. 1: a fixed order) and writes lp = l[target] - logsumexp, top_id, top_lp = -log(sum).
#include <limits.h>

#include <type_traits>

#include "argmax.h"
#include "dev.h"
#include "kernels.h"

namespace q3a {
namespace {

constexpr int BM = 64, BN = 128, BK = 64, LDSK = BK + 8;  // LDS rows padded by 16 B against bank conflicts of the fragment reads

__global__ __launch_bounds__(256) void align_norm_kernel(const float* __restrict__ x, int ldx, const int* __restrict__ rows, int M,
                                                         int Mp, const float* __restrict__ w, float eps, int K, int planes,
                                                         uint16_t* __restrict__ xn) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= Mp) return;
  const int nv = K / 4;  // float4 per row (K <= 2048: at most 8 per lane)
  uint16_t* o0 = xn + (size_t)r * K;
  uint16_t* o1 = xn + ((size_t)Mp + r) * K;
  if (r >= M) {
    for (int c = lane; c < nv; c += 64) {
      *reinterpret_cast<uint2*>(o0 + 4 * c) = make_uint2(0u, 0u);
      if (planes == 2) *reinterpret_cast<uint2*>(o1 + 4 * c) = make_uint2(0u, 0u);
    }
    return;
  }
  const float* xr = x + (size_t)rows[r] * ldx;
  float4 v[8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + i * 64;
    v[i] = c < nv ? reinterpret_cast<const float4*>(xr)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    sum += v[i].x * v[i].x + v[i].y * v[i].y + v[i].z * v[i].z + v[i].w * v[i].w;
  }
  sum = wave_sum(sum);
  const float rstd = 1.0f / sqrtf(sum / (float)K + eps);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + i * 64;
    if (c >= nv) break;
    const float4 wv = reinterpret_cast<const float4*>(w)[c];
    const float y0 = (v[i].x * rstd) * wv.x, y1 = (v[i].y * rstd) * wv.y, y2 = (v[i].z * rstd) * wv.z, y3 = (v[i].w * rstd) * wv.w;
    const uint2 hi = make_uint2(pack_bf16x2(y0, y1), pack_bf16x2(y2, y3));
    *reinterpret_cast<uint2*>(o0 + 4 * c) = hi;
    if (planes == 2) {
      const uint2 lo = make_uint2(pack_bf16x2(y0 - bf16lo(hi.x), y1 - bf16hi(hi.x)), pack_bf16x2(y2 - bf16lo(hi.y), y3 - bf16hi(hi.y)));
      *reinterpret_cast<uint2*>(o1 + 4 * c) = lo;
    }
  }
}

// One 64 x 128 output tile at (m0, n0 = 128 tile_n).  LP (scoring head): the partials carry the log-sum channel and the lane that
// holds column targets[m] stores its accumulator to tgt_logit[m].  BIAS (draft verification under a logit bias, LP only): bias[n], finite
// or -inf, is added to the fp32 accumulator in front of every channel and of the stored logits; a -inf logit stays exactly -inf,
// contributes 0 to the log-sum and never yields NaN (a lane whose columns are all suppressed keeps (max -inf, sum 0), which
// ArgmaxAcc::merge drops).
template <int NP, bool LOGITS, bool LP, bool BIAS = false>
__device__ __forceinline__ void head_tile(const uint16_t* __restrict__ xn, int Mp, int M, const uint16_t* __restrict__ W, int N, int K,
                                          const ArgmaxPartials& part, float* __restrict__ logits, size_t ldl, int m0, int tile_n,
                                          const int* __restrict__ targets, float* __restrict__ tgt_logit,
                                          const float* __restrict__ bias = nullptr) {
  __shared__ __attribute__((aligned(16))) uint16_t As[NP][BM * LDSK];
  __shared__ __attribute__((aligned(16))) uint16_t Bs[BN * LDSK];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
  const int n0 = tile_n * BN;
  // staging: 16-B chunks, 8 per 64-deep row; A: 2 per thread and plane, B: 4 per thread (rows beyond N read row N - 1).  Chunk
  // c = t + 256 j sits at row (t >> 3) + 32 j, column 8 (t & 7) of its tile.
  const int srow = t >> 3, skc = (t & 7) * 8;
  const uint16_t* ga = xn + (size_t)(m0 + srow) * K + skc;
  const uint16_t* gb = W + (size_t)min(n0 + srow, N - 1) * K + skc;
  const size_t ga_plane = (size_t)Mp * K;
  int gb_row[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) gb_row[j] = min(n0 + srow + 32 * j, N - 1) - min(n0 + srow, N - 1);
  // (named registers, not arrays: the compiler kept arrays filled inside the k loop in scratch)
  uint4 ra0, ra1, rl0, rl1, rb0, rb1, rb2, rb3;
  const size_t a1 = (size_t)32 * K;
  const size_t b1 = (size_t)gb_row[1] * K, b2 = (size_t)gb_row[2] * K, b3 = (size_t)gb_row[3] * K;
#define ALIGN_LOAD(k0)                                                                           \
  do {                                                                                           \
    ra0 = *reinterpret_cast<const uint4*>(ga + (k0));                                            \
    ra1 = *reinterpret_cast<const uint4*>(ga + a1 + (k0));                                       \
    if constexpr (NP == 2) {                                                                     \
      rl0 = *reinterpret_cast<const uint4*>(ga + ga_plane + (k0));                               \
      rl1 = *reinterpret_cast<const uint4*>(ga + ga_plane + a1 + (k0));                          \
    }                                                                                            \
    rb0 = *reinterpret_cast<const uint4*>(gb + (k0));                                            \
    rb1 = *reinterpret_cast<const uint4*>(gb + b1 + (k0));                                       \
    rb2 = *reinterpret_cast<const uint4*>(gb + b2 + (k0));                                       \
    rb3 = *reinterpret_cast<const uint4*>(gb + b3 + (k0));                                       \
  } while (0)
  f32x4_t acc[2][4];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int nk = K / BK;
  ALIGN_LOAD(0);
  for (int kt = 0; kt < nk; ++kt) {
    if (kt > 0) __syncthreads();  // every wave is done with the previous tile
    *reinterpret_cast<uint4*>(&As[0][srow * LDSK + skc]) = ra0;
    *reinterpret_cast<uint4*>(&As[0][(srow + 32) * LDSK + skc]) = ra1;
    if constexpr (NP == 2) {
      *reinterpret_cast<uint4*>(&As[NP - 1][srow * LDSK + skc]) = rl0;
      *reinterpret_cast<uint4*>(&As[NP - 1][(srow + 32) * LDSK + skc]) = rl1;
    }
    *reinterpret_cast<uint4*>(&Bs[srow * LDSK + skc]) = rb0;
    *reinterpret_cast<uint4*>(&Bs[(srow + 32) * LDSK + skc]) = rb1;
    *reinterpret_cast<uint4*>(&Bs[(srow + 64) * LDSK + skc]) = rb2;
    *reinterpret_cast<uint4*>(&Bs[(srow + 96) * LDSK + skc]) = rb3;
    __syncthreads();
    if (kt + 1 < nk) ALIGN_LOAD((kt + 1) * BK);
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      const int kof = kk * 32 + 8 * (lane >> 4);
      bf16x8_t b[4];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        b[ni] = *reinterpret_cast<const bf16x8_t*>(&Bs[(64 * wn + 16 * ni + (lane & 15)) * LDSK + kof]);
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
          const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(&As[p][(32 * wm + 16 * mi + (lane & 15)) * LDSK + kof]);
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[ni], acc[mi][ni], 0, 0, 0);
        }
    }
  }
  // epilogue: lane holds rows 4 (lane >> 4) + r of each 16 x 16 tile, column lane & 15; a lane's columns ascend with ni
  const int strip = tile_n * 2 + wn;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + 32 * wm + 16 * mi + 4 * (lane >> 4) + r;
      int tgt = -1;
      if constexpr (LP) tgt = m < M ? targets[m] : -1;
      ArgmaxAcc<LP> best;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int n = n0 + 64 * wn + 16 * ni + (lane & 15);
        if constexpr (BIAS) {
          if (n < N) acc[mi][ni][r] += bias[n];
        }
        const float v = acc[mi][ni][r];
        if (n < N && v > best.v) { best.v = v; best.i = n; }
        if (LOGITS && n < N && m < M) logits[(size_t)m * ldl + n] = v;
        if constexpr (LP) {
          if (n == tgt && n < N) tgt_logit[m] = v;  // (m < M: tgt is -1 otherwise) the accumulator the max channel sees
        }
      }
      if constexpr (LP) {  // this lane's log-sum around its own maximum (a lane whose columns are all beyond N keeps s = 0)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          const int n = n0 + 64 * wn + 16 * ni + (lane & 15);
          if constexpr (BIAS) {
            if (n < N && acc[mi][ni][r] != -INFINITY) best.s += __expf(acc[mi][ni][r] - best.v);
          } else {
            if (n < N) best.s += __expf(acc[mi][ni][r] - best.v);
          }
        }
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) best.merge_lane(o);
      if ((lane & 15) == 0 && m < M) best.store(part, m, strip);
    }
#undef ALIGN_LOAD
}

template <int NP, bool LOGITS>
__global__ __launch_bounds__(256) void align_head_kernel(const uint16_t* __restrict__ xn, int Mp, int M, const uint16_t* __restrict__ W,
                                                         int N, int K, ArgmaxPartials part, float* __restrict__ logits, int ldl) {
  head_tile<NP, LOGITS, false>(xn, Mp, M, W, N, K, part, logits, (size_t)ldl, blockIdx.y * BM, blockIdx.x, nullptr, nullptr);
}

// 1-D grid of 8 * ceil(tiles / 8) workgroups: the hardware deals workgroup ids round-robin to the 8 XCDs, so workgroup w walks tile
// (w % 8) * chunk + w / 8 -- every XCD a contiguous chunk of the tile order, in which the row tiles (m_tiles of them) are fastest
// BIAS: the same walk on l' = l + b (draft verification while a logit bias is set).  The bias pointer is a trailing argument that
// only the BIAS instantiations have (Bias = const float*, else empty): the others keep the kernarg segment they had without it.
template <int NP, bool LOGITS, bool BIAS, class... Bias>
__global__ __launch_bounds__(256) void score_head_kernel(const uint16_t* __restrict__ xn, int Mp, int M, const uint16_t* __restrict__ W,
                                                         int N, int K, ArgmaxPartials part, float* __restrict__ logits, size_t ldl,
                                                         const int* __restrict__ targets, float* __restrict__ tgt_logit, int m_tiles,
                                                         int tiles, Bias __restrict__... bias) {
  static_assert(sizeof...(Bias) == (BIAS ? 1 : 0), "the bias argument goes with BIAS");
  const int chunk = gridDim.x >> 3;
  const int id = (blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
  if (id >= tiles) return;  // (the whole workgroup)
  head_tile<NP, LOGITS, true, BIAS>(xn, Mp, M, W, N, K, part, logits, ldl, (id % m_tiles) * BM, id / m_tiles, targets, tgt_logit, bias...);
}

__global__ __launch_bounds__(256) void score_merge_kernel(ArgmaxPartials part, int n_part, int M, int N, const float* __restrict__ tgt_logit,
                                                          float* __restrict__ lp, int* __restrict__ top_id, float* __restrict__ top_lp) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;  // (the whole wave)
  ArgmaxAcc<true> best;
  for (int c = lane; c < n_part; c += 64) best.merge(ArgmaxAcc<true>::load(part, m, c));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best.merge_lane(o);
  if (lane != 0) return;
  // logsumexp = max + log(sum): the top logit IS the max, so top_lp = -log(sum) and lp = (l[target] - max) - log(sum) equals it
  // bit for bit when the target is the argmax
  const float ls = logf(best.s);
  float tl = -ls, yl = (tgt_logit[m] - best.v) - ls;
  if (tl > 0.f) tl = 0.f;  // (rounding; NaN passes through)
  if (yl > 0.f) yl = 0.f;
  int idx = best.i;
  if (idx < 0 || idx >= N) { idx = 0; tl = yl = __int_as_float(0x7fc00000); }  // no finite logit in the row
  lp[m] = yl;
  if (top_id) top_id[m] = idx;
  if (top_lp) top_lp[m] = tl;
}

__global__ __launch_bounds__(256) void align_merge_kernel(ArgmaxPartials part, int n_part, int M, int N, int* __restrict__ classes) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  ArgmaxAcc<false> best;
  for (int c = 0; c < n_part; ++c) best.merge(ArgmaxAcc<false>::load(part, m, c));
  classes[m] = best.i < N ? best.i : 0;  // (no finite logit in the row: class 0)
}

}  // namespace

int align_rows_padded(int M) { return (M + BM - 1) / BM * BM; }
int align_head_parts(int N) { return 2 * ((N + BN - 1) / BN); }

const char* launch_head_rows_norm(const RowHeadArgs& a, hipStream_t s) {
  if (a.M <= 0) return nullptr;
  if (!a.x || !a.rows || !a.norm_w || !a.xn) return "head rows norm: null argument";
  if (a.planes != 1 && a.planes != 2) return "head rows norm: planes must be 1 or 2";
  if (a.K % BK != 0 || a.K > 2048) return "head rows norm: hidden must be a multiple of 64 and at most 2048";
  const int Mp = align_rows_padded(a.M);
  hipLaunchKernelGGL(align_norm_kernel, dim3(Mp / 4), dim3(256), 0, s, a.x, a.ldx, a.rows, a.M, Mp, a.norm_w, a.eps, a.K, a.planes, a.xn);
  return nullptr;
}

// What launch_head_rows_norm does not check itself: the weights, the partials (n_part per row) and the logits' row stride.
static const char* row_head_check(const RowHeadArgs& a, int n_part) {
  if (!a.W || !a.part.val) return "row head: null argument";
  if (a.N <= 0) return "row head: no output columns";
  if (const char* e = argmax_partials_check(a.part, n_part)) return e;
  if (a.logits && a.ldl < (size_t)a.N) return "row head: logits row stride below the output columns";
  return nullptr;
}
// f(planes, logits, bias) with the three as compile-time constants: the one dispatch of both heads' tile kernels
template <class F>
static void row_head_dispatch(int planes, bool logits, bool bias, F&& f) {
  auto flag = [](bool v, auto&& g) { if (v) g(std::true_type{}); else g(std::false_type{}); };
  flag(planes == 2, [&](auto p2) {
    flag(logits, [&](auto lg) {
      flag(bias, [&](auto bs) { f(std::integral_constant<int, decltype(p2)::value ? 2 : 1>{}, lg, bs); });
    });
  });
}

const char* launch_score_head(const ScoreHeadArgs& a, hipStream_t s) {
  if (a.M <= 0) return nullptr;
  if (!a.targets || !a.tgt_logit || !a.lp || !a.part.sum) return "score head: null argument";
  const int n_part = align_head_parts(a.N);
  if (const char* e = row_head_check(a, n_part)) return e;
  const int Mp = align_rows_padded(a.M), m_tiles = Mp / BM;
  const long long tiles = (long long)m_tiles * ((a.N + BN - 1) / BN);
  if (tiles > (1ll << 30)) return "score head: too many tiles";
  if (const char* e = launch_head_rows_norm(a, s)) return e;
  const dim3 grid((unsigned)((tiles + 7) / 8 * 8));
  row_head_dispatch(a.planes, a.logits != nullptr, a.bias != nullptr, [&](auto np, auto lg, auto bs) {
    auto launch = [&](auto... bias) {
      hipLaunchKernelGGL((score_head_kernel<decltype(np)::value, decltype(lg)::value, decltype(bs)::value>), grid, dim3(256), 0, s, a.xn, Mp, a.M,
                         a.W, a.N, a.K, a.part, a.logits, a.ldl, a.targets, a.tgt_logit, m_tiles, (int)tiles, bias...);
    };
    if constexpr (decltype(bs)::value) launch(a.bias); else launch();
  });
  hipLaunchKernelGGL(score_merge_kernel, dim3((a.M + 3) / 4), dim3(256), 0, s, a.part, n_part, a.M, a.N, a.tgt_logit, a.lp, a.top_id, a.top_lp);
  return nullptr;
}

const char* launch_align_head(const AlignHeadArgs& a, hipStream_t s) {
  if (a.M <= 0) return nullptr;
  if (!a.classes) return "align head: null argument";
  if (a.part.sum) return "align head: no log-sum channel";
  if (a.ldl > (size_t)INT_MAX) return "align head: logits row stride too large";
  const int n_part = align_head_parts(a.N);
  if (const char* e = row_head_check(a, n_part)) return e;
  if (const char* e = launch_head_rows_norm(a, s)) return e;
  const int Mp = align_rows_padded(a.M);
  const dim3 grid((a.N + BN - 1) / BN, Mp / BM);
  row_head_dispatch(a.planes, a.logits != nullptr, false, [&](auto np, auto lg, auto) {
    hipLaunchKernelGGL((align_head_kernel<decltype(np)::value, decltype(lg)::value>), grid, dim3(256), 0, s, a.xn, Mp, a.M, a.W, a.N, a.K, a.part,
                       a.logits, (int)a.ldl);
  });
  hipLaunchKernelGGL(align_merge_kernel, dim3((a.M + 255) / 256), dim3(256), 0, s, a.part, n_part, a.M, a.N, a.classes);
  return nullptr;
}

}  // namespace q3a
