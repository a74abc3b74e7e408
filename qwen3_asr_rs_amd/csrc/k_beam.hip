// Beam search on the device (include/q3asr.h "beam search"): what one round adds to the greedy step.
//
//   beam_topk_chunk_kernel  the W best (logit, id) and the (max, sum exp) pair of one 2048-logit chunk of one row of logits [S][V]:
//                           every logit is read exactly once, a row is spread over ceil(V / 2048) workgroups.  Per thread the W best
//                           of its 8 logits sit in registers (sorted, unrolled insertion); the workgroup then extracts its W best
//                           in W rounds of "best list head wins, its owner pops".
//   beam_topk_merge_kernel  one wave per row: the row's W best of the chunk tables (the same two stages, 64 lanes), the row's
//                           (m, sum) in a fixed order, and lp = (l - m) - log(sum) of each -- the formula of score_merge_kernel.
//   beam_advance_kernel     one wave per utterance: candidates of the W slots (live: W each; finished: itself), their rank under
//                           (larger score, smaller parent slot, smaller token), slot assignment, new state, history, statistics and the
//                           stop word in pinned host memory.
//   kv_reorder_kernel       survivors that continue another slot's history get that slot's generated KV rows: one workgroup per
//                           (layer, K / V, kv head, row slice) moves one row of ALL sequences at a time -- every load of the row
//                           lands in registers before the barrier, every store comes after it, so cycles and fan-out are safe and
//                           there is no scratch copy of the suffix.
// The tie rule is ArgmaxAcc's everywhere: the larger value, on equal values the smaller id.
#include "argmax.h"

namespace q3a {

namespace {

__device__ __forceinline__ bool beats(float v, int i, float ov, int oi) { return v > ov || (v == ov && i < oi); }

// the W best (value, id) seen so far, best first; registers only (every index below is a compile-time constant after unrolling).
// Empty entries are (-inf, INT_MAX): a real -inf logit beats them, nothing is beaten by them.
template <int W>
struct TopList {
  float v[W];
  int i[W];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int j = 0; j < W; ++j) { v[j] = -INFINITY; i[j] = 0x7fffffff; }
  }
  __device__ __forceinline__ void insert(float x, int id) {
    if (!beats(x, id, v[W - 1], i[W - 1])) return;
#pragma unroll
    for (int j = W - 1; j >= 1; --j) {
      if (beats(x, id, v[j - 1], i[j - 1])) { v[j] = v[j - 1]; i[j] = i[j - 1]; }
      else if (beats(x, id, v[j], i[j])) { v[j] = x; i[j] = id; }
    }
    if (beats(x, id, v[0], i[0])) { v[0] = x; i[0] = id; }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int j = 0; j + 1 < W; ++j) { v[j] = v[j + 1]; i[j] = i[j + 1]; }
    v[W - 1] = -INFINITY; i[W - 1] = 0x7fffffff;
  }
};

// best (value, id) of the wave's list heads, in every lane
__device__ __forceinline__ void wave_best(float& bv, int& bi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (beats(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
}

template <int W, bool VEC>
__global__ __launch_bounds__(256) void beam_topk_chunk_kernel(const float* __restrict__ logits, int V, int n_chunk,
                                                              float* __restrict__ cand_val, int* __restrict__ cand_idx,
                                                              float* __restrict__ part_max, float* __restrict__ part_sum) {
  __shared__ float wv[2][4], ws[4];
  __shared__ int wi[2][4];
  const int s = blockIdx.y, c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* row = logits + (size_t)s * V;
  const int base = c * BEAM_CHUNK;
  TopList<W> L;
  L.init();
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
      if (e < V) {
        lse_visit(m, f[q].x, e); L.insert(f[q].x, e);
        lse_visit(m, f[q].y, e + 1); L.insert(f[q].y, e + 1);
        lse_visit(m, f[q].z, e + 2); L.insert(f[q].z, e + 2);
        lse_visit(m, f[q].w, e + 3); L.insert(f[q].w, e + 3);
      }
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
      if (e < V) { lse_visit(m, f[q], e); L.insert(f[q], e); }
    }
  }
  // (max, sum) of the chunk: lanes, then waves 0..3 -- a fixed order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m.merge_lane(o);
  if (lane == 0) { wv[0][wave] = m.v; ws[wave] = m.s; wi[0][wave] = m.i; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) m.merge(wv[0][w], wi[0][w], ws[w]);
    part_max[(size_t)s * n_chunk + c] = m.v;
    part_sum[(size_t)s * n_chunk + c] = m.s;
  }
  __syncthreads();
  // the chunk's W best: W rounds, the best list head of the workgroup wins and its owner pops
  const size_t out = ((size_t)s * n_chunk + c) * W;
#pragma unroll
  for (int r = 0; r < W; ++r) {
    float bv = L.v[0];
    int bi = L.i[0];
    wave_best(bv, bi);
    if (lane == 0) { wv[r & 1][wave] = bv; wi[r & 1][wave] = bi; }
    __syncthreads();
    bv = wv[r & 1][0]; bi = wi[r & 1][0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (beats(wv[r & 1][w], wi[r & 1][w], bv, bi)) { bv = wv[r & 1][w]; bi = wi[r & 1][w]; }
    if (bi != 0x7fffffff && L.i[0] == bi) L.pop();  // (ids are unique: exactly one owner)
    if (tid == 0) { cand_val[out + r] = bv; cand_idx[out + r] = bi; }
  }
}

template <int W>
__global__ __launch_bounds__(64) void beam_topk_merge_kernel(const float* __restrict__ cand_val, const int* __restrict__ cand_idx,
                                                             const float* __restrict__ part_max, const float* __restrict__ part_sum,
                                                             int n_chunk, int* __restrict__ out_ids, float* __restrict__ out_lp) {
  const int s = blockIdx.x, lane = threadIdx.x;
  TopList<W> L;
  L.init();
  const size_t cb = (size_t)s * n_chunk * W;
  for (int x = lane; x < n_chunk * W; x += 64) L.insert(cand_val[cb + x], cand_idx[cb + x]);
  ArgmaxAcc<true> m;  // lane l takes chunks l, l + 64, ... in ascending order, then the xor butterfly 32 .. 1
  for (int c = lane; c < n_chunk; c += 64) m.merge(part_max[(size_t)s * n_chunk + c], c, part_sum[(size_t)s * n_chunk + c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m.merge_lane(o);
  const float ls = logf(m.s);
#pragma unroll
  for (int r = 0; r < W; ++r) {
    float bv = L.v[0];
    int bi = L.i[0];
    wave_best(bv, bi);
    if (bi != 0x7fffffff && L.i[0] == bi) L.pop();
    if (lane == 0) {
      float lp = (bv - m.v) - ls;
      if (lp > 0.f) lp = 0.f;  // (rounding; NaN passes through)
      out_ids[(size_t)s * W + r] = bi;
      out_lp[(size_t)s * W + r] = lp;
    }
  }
}

// --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void beam_advance_kernel(BeamAdvanceArgs a) {
  __shared__ float sv_sc[16][BEAM_MAX_W], sv_lp[16][BEAM_MAX_W];
  __shared__ int sv_par[16][BEAM_MAX_W], sv_tok[16][BEAM_MAX_W];
  __shared__ int w_copies[16], w_rows[16], w_fin[16], w_live[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int W = a.W;
  const int round = a.state[BEAM_ST_ROUNDS];
  if (a.state[BEAM_ST_ALL_DONE]) {  // the search has ended: a run-ahead launch only reports that it came by
    if (tid == 0) {
      const int n = a.state[BEAM_ST_LAUNCHES] + 1;
      a.state[BEAM_ST_LAUNCHES] = n;
      if (a.host_progress) __hip_atomic_store(a.host_progress, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return;
  }
  if (lane == 0) { w_copies[wave] = 0; w_rows[wave] = 0; w_fin[wave] = 0; w_live[wave] = 0; }
  for (int u0 = 0; u0 < a.U; u0 += nw) {  // (uniform trip count: the barriers below are met by every wave)
    const int u = u0 + wave;
    const bool on = u < a.U;
    const int ps = lane / W, k = lane - ps * W;  // candidate k of parent slot ps
    bool valid = false;
    float sc = -INFINITY, lp = 0.f;
    int tok = -1;
    if (on && lane < W * W) {
      const int q = u * W + ps;
      const float pscore = a.score[q];
      if (a.finished[q]) {
        if (k == 0) { valid = true; sc = pscore; }
      } else if (pscore != -INFINITY) {  // live; an empty slot (score -inf) has no candidates
        valid = true;
        lp = a.topk_lp[(size_t)q * W + k];
        tok = a.topk_ids[(size_t)q * W + k];
        sc = pscore + lp;
      }
    }
    // rank = candidates that come before this one: larger score, then smaller parent slot, then smaller token ("none" = -1 first)
    int rank = 0;
    for (int o = 0; o < 64; ++o) {
      const bool ov = __shfl((int)valid, o, 64) != 0;
      const float os = __shfl(sc, o, 64);
      const int op = __shfl(ps, o, 64), ot = __shfl(tok, o, 64);
      const bool first = ov && (!valid || os > sc || (os == sc && (op < ps || (op == ps && ot < tok))));
      rank += first ? 1 : 0;
    }
    const int n_valid = __popcll(__ballot(valid));
    const int n_surv = n_valid < W ? n_valid : W;
    if (valid && rank < W) { sv_sc[wave][rank] = sc; sv_lp[wave][rank] = lp; sv_par[wave][rank] = ps; sv_tok[wave][rank] = tok; }
    __syncthreads();
    // slot assignment (every lane the same few steps): a survivor keeps its parent's slot if that is still free, the others take
    // the free slots in ascending order
    int mine = -1;  // rank of the survivor that lands in slot `lane`
    if (on && lane < W) {
      unsigned taken = 0;
      int slot_of[BEAM_MAX_W];
#pragma unroll
      for (int r = 0; r < BEAM_MAX_W; ++r) {
        slot_of[r] = -1;
        if (r < n_surv) {
          const int p = sv_par[wave][r];
          if (!((taken >> p) & 1u)) { slot_of[r] = p; taken |= 1u << p; }
        }
      }
#pragma unroll
      for (int r = 0; r < BEAM_MAX_W; ++r) {
        if (r < n_surv && slot_of[r] < 0) {
          const int j = __ffs(~taken) - 1;
          slot_of[r] = j; taken |= 1u << j;
        }
        if (r < n_surv && slot_of[r] == lane) mine = r;
      }
    }
    bool copy = false, newly = false, fin_now = false;
    if (on && lane < W) {
      const int q = u * W + lane;
      int par = q, tk = -1;
      float ns = -INFINITY, nlp = 0.f;
      if (mine >= 0) {
        par = u * W + sv_par[wave][mine]; tk = sv_tok[wave][mine]; ns = sv_sc[wave][mine]; nlp = sv_lp[wave][mine];
        newly = tk == a.eos0 || tk == a.eos1;
        fin_now = tk < 0 || newly;
        copy = par != q;
      }
      a.parent[q] = par; a.token[q] = tk; a.score[q] = ns; a.finished[q] = fin_now ? 1 : 0;
      if (a.feed) a.feed[q] = (fin_now || tk < 0) ? 0 : tk;
      if (a.hist_parent && round < a.hist_cap) {
        const size_t h = (size_t)round * a.U * W + q;
        a.hist_parent[h] = par; a.hist_token[h] = tk; a.hist_lp[h] = nlp;
      }
    }
    const int n_copy = __popcll(__ballot(copy)), n_new = __popcll(__ballot(newly)), n_fin = __popcll(__ballot(fin_now));
    if (on && lane == 0) {
      int rows = 0;
      if (a.pos && a.lo) rows = a.pos[u * W] + a.hi_bias - a.lo[u * W] + 1;
      w_copies[wave] += n_copy; w_rows[wave] += n_copy * (rows > 0 ? rows : 0); w_fin[wave] += n_new;
      w_live[wave] += n_fin == W ? 0 : 1;
    }
    __syncthreads();
  }
  if (tid == 0) {
    int copies = 0, rows = 0, fin = 0, live = 0;
    for (int w = 0; w < nw; ++w) { copies += w_copies[w]; rows += w_rows[w]; fin += w_fin[w]; live += w_live[w]; }
    const int n = a.state[BEAM_ST_LAUNCHES] + 1;
    a.state[BEAM_ST_ROUNDS] = round + 1;
    a.state[BEAM_ST_COPIES] += copies;
    a.state[BEAM_ST_KV_ROWS] += rows;
    a.state[BEAM_ST_FINISHED] += fin;
    a.state[BEAM_ST_ALL_DONE] = live == 0;
    a.state[BEAM_ST_LAUNCHES] = n;
    if (a.host_progress) {
      if (live == 0) __hip_atomic_store(a.host_progress + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(a.host_progress, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// --------------------------------------------------------------------------------------------------
// UPR: 16-byte units per cache row (128 elements): 16 (bf16) or 32 (fp32)
template <int UPR>
__global__ __launch_bounds__(256) void kv_reorder_kernel(KvReorderArgs a) {
  __shared__ int s_n[32], s_par[32], s_lo[32];
  __shared__ int s_max;
  const int tid = threadIdx.x;
  if (a.all_done && *a.all_done) return;  // a run-ahead step after the search ended
  if (tid < a.S) {
    const int p = a.parent[tid], lo = a.lo[tid], hi = a.hi[tid] + a.hi_bias;
    s_par[tid] = p; s_lo[tid] = lo;
    s_n[tid] = (p != tid && hi >= lo) ? hi - lo + 1 : 0;
  }
  __syncthreads();
  if (tid == 0) {
    int mx = 0;
    for (int s = 0; s < a.S; ++s) mx = s_n[s] > mx ? s_n[s] : mx;
    s_max = mx;
  }
  __syncthreads();
  const int n_rows = s_max;
  if (n_rows == 0) return;  // every slot keeps its history
  // blockIdx.x = (layer, K | V, kv head); blockIdx.y = row slice
  const int kvh = blockIdx.x % a.n_kv, which = (blockIdx.x / a.n_kv) & 1, layer = blockIdx.x / (2 * a.n_kv);
  uint4* const base = reinterpret_cast<uint4*>(which ? a.vcache : a.kcache);
  const size_t seq_units = (size_t)a.n_kv * a.max_ctx * UPR, layer_units = (size_t)a.S * seq_units;
  constexpr int NQ = 32 * UPR / 256;  // units per thread and row of all sequences (S <= 32)
  for (int i = blockIdx.y; i < n_rows; i += gridDim.y) {
    // unit x of the row of all sequences: sequence x / UPR, 16-byte unit x % UPR; offset of (sequence, row, unit) inside a layer
    auto unit = [&](int q, bool parent, size_t& off) {
      const int x = tid + q * 256, s = x / UPR, c = x % UPR;
      if (s >= a.S || i >= s_n[s]) return false;
      off = (size_t)layer * layer_units + (size_t)(parent ? s_par[s] : s) * seq_units + ((size_t)kvh * a.max_ctx + s_lo[s] + i) * UPR + c;
      return true;
    };
    uint4 b0 = {}, b1 = {}, b2 = {}, b3 = {};
    size_t off;
    if (unit(0, true, off)) b0 = base[off];
    if (unit(1, true, off)) b1 = base[off];
    if constexpr (NQ == 4) {
      if (unit(2, true, off)) b2 = base[off];
      if (unit(3, true, off)) b3 = base[off];
    }
    // every load of this row has returned before any store to it is issued
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (unit(0, false, off)) base[off] = b0;
    if (unit(1, false, off)) base[off] = b1;
    if constexpr (NQ == 4) {
      if (unit(2, false, off)) base[off] = b2;
      if (unit(3, false, off)) base[off] = b3;
    }
  }
}

}  // namespace

const char* launch_beam_topk(const BeamTopkArgs& a, hipStream_t s) {
  if (a.S <= 0) return nullptr;
  if (a.W < 1 || a.W > BEAM_MAX_W) return "beam top-W: width must be 1..8";
  if (a.V < a.W) return "beam top-W: fewer logits than the width";
  if (!a.logits || !a.cand_val || !a.cand_idx || !a.part_max || !a.part_sum || !a.out_ids || !a.out_lp) return "beam top-W: null argument";
  const int nc = beam_topk_chunks(a.V);
  const bool vec = a.V % 4 == 0 && ((uintptr_t)a.logits & 15) == 0;
  const dim3 grid(nc, a.S);
#define Q3A_BEAM_W(Wc)                                                                                                              \
  case Wc:                                                                                                                          \
    if (vec) hipLaunchKernelGGL((beam_topk_chunk_kernel<Wc, true>), grid, dim3(256), 0, s, a.logits, a.V, nc, a.cand_val, a.cand_idx, a.part_max, a.part_sum); \
    else hipLaunchKernelGGL((beam_topk_chunk_kernel<Wc, false>), grid, dim3(256), 0, s, a.logits, a.V, nc, a.cand_val, a.cand_idx, a.part_max, a.part_sum); \
    hipLaunchKernelGGL((beam_topk_merge_kernel<Wc>), dim3(a.S), dim3(64), 0, s, a.cand_val, a.cand_idx, a.part_max, a.part_sum, nc, a.out_ids, a.out_lp); \
    break;
  switch (a.W) {
    Q3A_BEAM_W(1) Q3A_BEAM_W(2) Q3A_BEAM_W(3) Q3A_BEAM_W(4) Q3A_BEAM_W(5) Q3A_BEAM_W(6) Q3A_BEAM_W(7) Q3A_BEAM_W(8)
  }
#undef Q3A_BEAM_W
  return nullptr;
}

const char* launch_beam_advance(const BeamAdvanceArgs& a, hipStream_t s) {
  if (a.U <= 0) return nullptr;
  if (a.W < 1 || a.W > BEAM_MAX_W) return "beam advance: width must be 1..8";
  if (a.U * a.W > 32) return "beam advance: more than 32 sequences";
  if (!a.topk_ids || !a.topk_lp || !a.score || !a.finished || !a.parent || !a.token || !a.state) return "beam advance: null argument";
  if (a.hist_parent && (!a.hist_token || !a.hist_lp)) return "beam advance: the history arrays go together";
  const int waves = a.U < 16 ? a.U : 16;
  hipLaunchKernelGGL(beam_advance_kernel, dim3(1), dim3(64 * waves), 0, s, a);
  return nullptr;
}

const char* launch_kv_reorder(const KvReorderArgs& a, hipStream_t s) {
  if (a.S <= 0 || a.layers <= 0) return nullptr;
  if (a.S > 32) return "kv reorder: more than 32 sequences";
  if (a.elem_bytes != 2 && a.elem_bytes != 4) return "kv reorder: element size must be 2 or 4";
  if (!a.kcache || !a.vcache || !a.parent || !a.lo || !a.hi) return "kv reorder: null argument";
  const dim3 grid(a.layers * 2 * a.n_kv, KV_REORDER_SLICES);
  if (a.elem_bytes == 2) hipLaunchKernelGGL(kv_reorder_kernel<16>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(kv_reorder_kernel<32>, grid, dim3(256), 0, s, a);
  return nullptr;
}

}  // namespace q3a
