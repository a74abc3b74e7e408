// Launch wrappers of the gfx950 kernels.  Every launch goes to the caller's HIP stream; nothing here
// allocates or synchronises (graph-capture safe).  A non-null return value is a static error string.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#ifndef Q3A_STAMP_FIELD  // (dev.h defines it for device code; host-only translation units get the same layout)
#ifdef Q3A_STAMP
#define Q3A_STAMP_FIELD unsigned long long* stamp = nullptr;
#else
#define Q3A_STAMP_FIELD
#endif
#endif

namespace q3a {

// ---- argmax partials ----------------------------------------------------------------------------------
// What every producer of the decode step's argmax writes and argmax_finalize merges: per row (sequence) and partial (a block of
// the vocabulary) the block maximum val, its first index idx and, for token log-probabilities, sum = sum exp(logit - val) over
// the block; entry [row * stride + col].  sum is null when that channel is off.  The tie rule and the (max, sum) merge live in
// ONE place, argmax.h ArgmaxAcc.
struct ArgmaxPartials {
  float* val = nullptr;
  int* idx = nullptr;
  float* sum = nullptr;
  int stride = 0;
  ArgmaxPartials at(size_t rows) const {  // the same partials from row `rows` on
    const size_t o = rows * stride;
    return {val ? val + o : nullptr, idx ? idx + o : nullptr, sum ? sum + o : nullptr, stride};
  }
};
// the rules every producer and argmax_finalize share: val and idx go together, sum needs them, a row holds n_part entries
inline const char* argmax_partials_check(const ArgmaxPartials& p, int n_part) {
  if (!p.val != !p.idx) return "argmax partials: val and idx go together";
  if (p.sum && !p.val) return "argmax partials: the log-sum channel needs val and idx";
  if (p.val && p.stride < n_part) return "argmax partials: buffer too small";
  return nullptr;
}

// ---- heads at a list of rows of a prefill's residual stream (k_align.hip) -----------------------------------------
// What both heads share: at the M rows `rows` of x the final RMSNorm, then W [N][K] (bf16) on 64 x 128 tiles with one argmax
// partial per row and 64-column strip.  The logits are written only when `logits` is set.
struct RowHeadArgs {
  const float* x; int ldx;        // residual stream after the last decoder layer, fp32 [rows][ldx]
  const int* rows; int M;         // [M] rows of x (device)
  const float* norm_w; float eps; // final RMSNorm
  const uint16_t* W; int N; int K;
  int planes;                     // 1: bf16 operand (default mode); 2: hi + lo bf16 split of the fp32 normed rows (precise mode)
  uint16_t* xn;                   // workspace [planes][align_rows_padded(M)][K]
  ArgmaxPartials part;            // [M] rows x align_head_parts(N) partials
  float* logits; size_t ldl;      // nullable: [M][ldl] fp32
};
// the first launch of both heads: rows[M] of x gathered, final RMSNorm, bf16 operand planes xn [planes][align_rows_padded(M)][K]
// (rows M .. padded are zeros); it reads x .. xn of the arguments
int align_rows_padded(int M);
const char* launch_head_rows_norm(const RowHeadArgs& a, hipStream_t s);
// Forced-aligner head: the rows are the marker rows of an aligner prefill, W the classifier [N = classify_num][K = hidden], and the
// result the argmax over the N time classes.  part has no log-sum channel.
struct AlignHeadArgs : RowHeadArgs {
  int* classes;                   // [M] argmax (first index on ties)
};
int align_head_parts(int N);
const char* launch_align_head(const AlignHeadArgs& a, hipStream_t s);
// Scoring head: log-probabilities of given tokens.  The rows are those that predict a given transcript, W the lm_head
// [N = vocab][K = hidden]; per row the log-probability of targets[m], the argmax and its log-probability.  part carries the log-sum
// channel.
struct ScoreHeadArgs : RowHeadArgs {
  const int* targets;             // [M] in [0, N) (device)
  float* tgt_logit;               // [M] workspace: the fp32 accumulator of column targets[m]
  float* lp;                      // [M] l[target] - logsumexp(l)
  int* top_id; float* top_lp;     // [M] argmax (first index on ties) and its log-probability; nullable
  // draft verification only (nullable; q3a_score* never sets it): a logit bias [N], every entry finite or -inf, added to the fp32
  // accumulator in front of the max, log-sum and target channels and of the stored logits -- the BIAS instantiation of the same tile
  const float* bias;
};
const char* launch_score_head(const ScoreHeadArgs& a, hipStream_t s);

// ---- GEMM (k_gemm.hip) -----------------------------------------------------------------------------
struct GemmEpilogue {
  float* out = nullptr;          // [rows][ldo] fp32
  uint16_t* out16 = nullptr;     // alternative bf16 output (k_gemm16.hip only): feeds the next GEMM's LDS-DMA directly
  int ldo = 0;
  const float* bias = nullptr;   // [N] or null
  int act = 0;                   // 0 none, 1 erf-GELU
  const float* resid = nullptr;  // [rows][ldo] added after the activation (may alias out)
  const int* rowmap = nullptr;   // GEMM row m -> output row (negative: drop the row); null = identity
  const float* addend = nullptr; // [addend_period][ldo] added before the activation (positional embedding)
  int addend_period = 1;
  // k_gemm16.hip, M <= 32 (lm_head of a batched decode step): one argmax partial per output row and 64-column tile (col = tile);
  // `out` may then be null (no logits stored)
  ArgmaxPartials part;
  Q3A_STAMP_FIELD
};
// Y = X[M][K](fp32, row stride lda) . W[N][K]^T(bf16).  glu: W rows are [16 gate|16 up] blocks, out has N/2 columns.
const char* launch_gemm(const float* X, int lda, const uint16_t* W, int M, int N, int K, const GemmEpilogue& ep,
                        bool glu, bool split, hipStream_t s);
// 3x3 / stride 2 / pad 1 convolution as implicit GEMM over an NHWC fp32 map [imgs][H][W][C]; W bf16 [Cout][3][3][C].
const char* launch_conv3x3s2_gemm(const float* X, int imgs, int H, int Wd, int C, const uint16_t* Wt, int Cout,
                                  const GemmEpilogue& ep, bool split, hipStream_t s);
void launch_gemm_ref(const float* X, const uint16_t* W, float* Y, int M, int N, int K, hipStream_t s);
// bf16-activation versions (k_gemm16.hip, default mode): both operands go HBM -> LDS with global_load_lds.
const char* launch_gemm16(const uint16_t* X, int lda, const uint16_t* W, int M, int N, int K, const GemmEpilogue& ep,
                          bool glu, hipStream_t s);
// zero_page: >= 128 B of zeros (padded filter taps read it)
const char* launch_conv3x3s2_gemm16(const uint16_t* X, const uint16_t* zero_page, int imgs, int H, int Wd, int C,
                                    const uint16_t* Wt, int Cout, const GemmEpilogue& ep, hipStream_t s);
// 256 x 256 x 64, 8-wave, counted-vmcnt version of the two above for batch-sized problems (k_gemm256.hip); launch_gemm16 /
// launch_conv3x3s2_gemm16 dispatch to it when gemm256_eligible (enough 256 x 256 tiles, K % 64 == 0, K >= 128)
bool gemm256_eligible(int M, int N, int K);
// launch_gemm16 without the dispatch to gemm256 (the 4-wave tiles of k_gemm16.hip): small problems and gemm256's split remainder
const char* launch_gemm16_small(const uint16_t* X, int lda, const uint16_t* W, int M, int N, int K, const GemmEpilogue& ep,
                                bool glu, hipStream_t s);
// Process-wide A/B knobs (engine.cpp).  Initialised from the environment exactly once (std::call_once) and atomics
// afterwards: q3a_group_transcribe drives one host thread per GPU through the code that reads them, q3a_debug_set writes them.
struct Knobs {
  std::atomic<int> gemm256_min_tiles{128};      // Q3A_GEMM256_MIN_TILES: 256 x 256 tiles from which gemm256 is used (k_gemm256.hip)
  std::atomic<int> gemm256_persist{1};          // Q3A_GEMM256_PERSIST: gemm256 launches min(tiles, CUs) workgroups that walk the tiles, the next tile's first K tile arriving under the epilogue (0 = one workgroup per tile, n > 1 = exactly n workgroups; bit-identical)
  std::atomic<int> gemm256_group_m{0};          // Q3A_GEMM256_GROUP_M: gemm256's tile order -- groups of this many tile rows, M fastest inside a group (1 = N fastest over the whole matrix; 0 = 8 where the matrix is at least 8 tiles wide, else 1); the same tiles, another assignment to workgroups: bit-identical
  std::atomic<int> dattn_batched_min_wgs{128};  // Q3A_DATTN_BATCHED_MIN_WGS: S * n_kv from which launch_decode_attn_batched is used
  std::atomic<int> decode_group_size{0};        // Q3A_DECODE_GROUP: sequences per group of the batched decode step (0 = 32)
  std::atomic<int> decode_parallel_groups{1};   // Q3A_DECODE_PARALLEL: groups as parallel stream / graph branches
  std::atomic<int> fuse_qkrope{1};              // Q3A_FUSE_QKROPE: QK-norm + RoPE + cache append as the qkv GEMM's epilogue
  std::atomic<int> skinny_q{1};                 // Q3A_SKINNY_Q: quarter workgroups for the o / down projections
  std::atomic<int> eos_run_ahead{1};            // Q3A_EOS_RUN_AHEAD: decode steps kept enqueued ahead of the device in natural-EOS mode.  1: exactly the steps needed are executed; paired with a fixed-N run of the same engine (profiles/r5_eos_run_ahead_ab.txt, two processes): 1 costs +0.03 / +1.24 ms per 100 tokens, 2 costs +2.07 / +1.86 ms (one wasted step + the same launch latency), 3 +1.3 / +1.2, 4 +3.3 / +3.1
  std::atomic<int> skinny_glu_hp3{1};           // Q3A_SKINNY_GLU_HP3: gate/up skinny GEMM as 3 half-pair tiles per workgroup when the pair form has more workgroups than CUs (k_skinny.hip HP; 0 = off, 2 = whenever the shape allows)
  std::atomic<int> lm_head_prune{1};            // Q3A_LM_HEAD_PRUNE: one-sequence decode argmax from an int8 pre-pass + bf16 rescore of the candidate blocks (k_gemv.hip; bit-identical ids)
  std::atomic<int> oproj_by_head{1};            // Q3A_OPROJ_BY_HEAD: one-sequence decode chain of the default mode (hidden <= 1024) with o_proj per pair of kv heads, its partial vectors added by gate / up, and 32- / 64-key attention splits up to 512 / 1024 keys; 0 = the merging o_proj and 128-key splits, which contexts beyond 2048 keys run anyway (tests compare the two; ids equal, logits differ by fp32 summation order)
  // debug aids (tests): no effect on what a run computes
  std::atomic<int> layer_taps{0};               // Q3A_DEBUG_LAYER_TAPS: with debug taps, raw copies of every encoder / decoder prefill layer's intermediate buffers
  std::atomic<int> poison_attn_partials{0};     // every batch set-up fills the decode attention's split partials (m, l, o) with NaN bytes
  // Round 6 removed nine knobs together with the code only they selected (docs/HISTORY.md "Pruned in round 6"; last present at commit
  // caf7a05): fuse_qkv_attn, dattn_pair_split, fattn_pipe, rope_variant, rope_twice (measured alternatives that lost / finished debug
  // aids), gemm16_ring, gemm256_resid_prefetch, live_key_splits, skinny_glu_2pass (the winning form is now the only form).
};
Knobs& knobs();
const char* launch_gemm256(const uint16_t* X, int lda, const uint16_t* W, int M, int N, int K, const GemmEpilogue& ep,
                           bool glu, hipStream_t s);
const char* launch_conv3x3s2_gemm256(const uint16_t* X, const uint16_t* zero_page, int imgs, int H, int Wd, int C,
                                     const uint16_t* Wt, int Cout, const GemmEpilogue& ep, hipStream_t s);
// fp32 -> bf16 (round to nearest even), n elements
const char* launch_to_bf16(const float* x, uint16_t* y, size_t n, hipStream_t s);
// bf16 -> fp32 (debug taps of bf16 intermediates)
const char* launch_from_bf16(const uint16_t* x, float* y, size_t n, hipStream_t s);

// ---- log-mel front end (k_mel.hip) -------------------------------------------------------------------
struct MelBatch {
  const float* pcm;            // concatenated utterances
  const int64_t* pcm_off;      // [B] sample offset of each utterance (device)
  const int64_t* n_samples;    // [B] (device)
  const int64_t* mel_off;      // [B] float offset of each (128, F_b) block (device)
  const int* n_frames;         // [B] (device)
  float* mel;                  // output, concatenated (128, F_b) blocks
  unsigned* gmax_key;          // [B] order-preserving key of the per-utterance max (zeroed by the launcher)
};
const char* launch_mel(const MelBatch& mb, int B, int max_frames, const float* dft /*[400][416]*/,
                       const float* filt_t /*[202][128]*/, hipStream_t s);

// ---- conv stem first layer (k_conv1.hip) ---------------------------------------------------------------
struct ChunkTable {
  const int* chunk_utt;    // [C] utterance of each chunk (device)
  const int* chunk_frame0; // [C] first mel frame of the chunk inside its utterance (device)
};
// mel (128, F_b) blocks -> NHWC fp32 [chunk][64][W/2][Cout] = gelu(conv3x3 s2 p1 + bias), chunk zero-padded to `chunk_frames`
const char* launch_conv1(const float* mel, const int64_t* mel_off, const int* n_frames, const ChunkTable& ct,
                         int n_chunks, int n_mels, int chunk_frames, const float* w /*[Cout][9]*/,
                         const float* b, int Cout, float* out, hipStream_t s, uint16_t* out16 = nullptr);

// ---- norms (k_norm.hip) ----------------------------------------------------------------------------------
const char* launch_layernorm(const float* x, const float* w, const float* b, float* y, int rows, int D, float eps,
                             hipStream_t s, uint16_t* y16 = nullptr);  // y16 != null: write bf16 there instead of y
const char* launch_rmsnorm(const float* x, const float* w, float* y, int rows, int D, float eps, hipStream_t s,
                           uint16_t* y16 = nullptr);

// ---- attention over independent segments (k_attn.hip) ------------------------------------------------------
// One segment = a set of `len` queries/keys that attend to each other (encoder windows, non-causal) or a
// whole decoder sequence (causal).  Element (row j, head h, dim d):
//   Q: q + (q_row0 + j) * q_rs + h * HD + d                          (fp32)
//   K: k + kv_off + kvh * kv_hs + j * kv_rs + d   (V likewise)       (KVT = float or bf16)
//   O: o + (q_row0 + j) * o_rs + h * HD + d                          (fp32)
struct AttnSeg {
  int q_row0;
  int len;
  int64_t kv_off;
};
struct AttnArgs {
  const float* q; int q_rs;
  const uint16_t* q16;  // MFMA flash attention only: when non-null, Q is read from here as bf16 (same strides) instead of q
  const void* k; const void* v; int64_t kv_hs; int kv_rs;
  float* o; int o_rs;
  uint16_t* o16;    // MFMA flash attention only: when non-null the output is written here as bf16 (same strides)
  const AttnSeg* segs; int n_segs; int max_len;
  int n_kv_heads;
  float scale_div;  // scores are divided by this (sqrt(head_dim)), as the reference does
};
const char* launch_attn_enc(const AttnArgs& a, hipStream_t s);                            // HD=64, 1 q-head per kv head, non-causal, fp32 K/V
const char* launch_attn_prefill(const AttnArgs& a, int group, bool kv_f32, hipStream_t s);  // HD=128, causal, GQA group 1/2/4
// MFMA flash-attention versions of the two above (k_fattn.hip): bf16 operands, default mode only
const char* launch_fattn_enc(const AttnArgs& a, hipStream_t s);                 // fp32 K/V rounded to bf16 while staging
const char* launch_fattn_prefill(const AttnArgs& a, int group, hipStream_t s);  // bf16 KV cache
// The instantiation the last launch_attn_* / launch_fattn_* call of this thread launched (all zero: none -- an empty batch or a refusal).
// Tests compare it with the form they mean to run: the launchers pick by pointer alignment, strides, shape and knobs read once per process.
struct AttnForm { int hd, group, causal, kv_f32, qpw, grid_x, grid_y, grid_z; };
AttnForm attn_last_form();
struct FattnForm { int dma, hd, group, causal, kv_f32, ksplit, ns, grid_x, grid_y, grid_z; };  // dma 1: fattn_dma_kernel with NS stages; 0: fattn_kernel (ns 0)
FattnForm fattn_last_form();

// ---- decoder glue (k_decode.hip) ----------------------------------------------------------------------------
// hidden[r] = embed[ids[r]] for rows whose id is not `skip_id` (audio rows are written by the encoder tail)
const char* launch_embed(const int* ids, int rows, const uint16_t* embed, int H, int skip_id, float* out, hipStream_t s);
struct RopeKvArgs {
  float* qkv;               // [rows][qkv_dim] fp32; q part is normalised + rotated in place
  const int* row_seq;       // [rows] sequence of the row
  const int* row_pos;       // [rows] position inside the sequence
  const float* q_norm; const float* k_norm; float eps;
  const float* cos_t; const float* sin_t;  // [max_pos][64]
  void* kcache; void* vcache;              // this layer: [S][n_kv][max_ctx][128]
  int n_q, n_kv, max_ctx;
  uint16_t* q16;            // non-null (default mode, MFMA attention): q is written HERE as bf16 [rows][n_q*128] -- the value the
                            // attention kernel rounds it to on load anyway -- instead of in place as fp32 (half the bytes twice)
};
const char* launch_qknorm_rope_kv(const RopeKvArgs& a, int rows, bool kv_f32, hipStream_t s);
// rows [0, M1) of an M x N problem that launch_gemm256 / launch_gemm256_qkrope give to the 256 x 256 kernel when they split off
// the trailing rows (0: no split)
int gemm256_split_rows(int M, int N);
// qkv projection (bf16 X [M][K] . W[(n_q + 2 n_kv) * 128][K]^T + bias) with the kernel above as its epilogue: q -> a.q16, k / v
// -> bf16 KV cache; a.qkv is not touched.  256 x 256 tiles (k_gemm256.hip): call when gemm256_eligible(M, N, K).
const char* launch_gemm256_qkrope(const uint16_t* X, int lda, const uint16_t* W, int M, int K, const float* bias,
                                  const RopeKvArgs& a, hipStream_t s);
// dst[i] = src[row_idx[i]]
const char* launch_gather_rows(const float* src, const int* row_idx, int n, int D, float* dst, hipStream_t s);
// dst[dst_row[i]] = src[i]  (negative dst_row: skip)
const char* launch_scatter_rows(const float* src, const int* dst_row, int n, int D, float* dst, hipStream_t s);

// GEMV family: y[b][n] = sum_k xn[b][k] * W[n][k], b < NB <= 4, x fp32 staged in LDS, W bf16 streamed once.
struct GemvArgs {
  const float* x; int ldx;      // [NB][K]
  const float* rms_w;           // non-null: x is RMS-normalised with this weight first (eps below)
  float eps;
  const uint16_t* W; int N; int K;
  const float* bias;            // [N] or null
  int mode;                     // 0: store, 1: out = resid + y, 2: GLU (W rows in [16 gate|16 up] blocks; N = 2*inter),
                                // 3 (needs rms_w: the lm_head): logits (out nullable) + per-block argmax partials
  float* out; int ldo;
  const float* resid;
  ArgmaxPartials part;          // mode 3: one partial per sequence and workgroup (col = blockIdx.x)
  // optional: x = attention output merged on the fly from the flash-decoding partials of launch_decode_attn
  // (x/ldx ignored; K must equal attn_heads*128)
  const float* attn_pm; const float* attn_pl; const float* attn_po; int attn_nsplit; int attn_heads;
  int attn_fast_exp;            // merge weights with the hardware exponential (default mode) instead of expf
  int fast_math;                // default mode: hardware rsq / exp / rcp in the RMSNorm scale and SiLU of the epilogue (dev.h rstd_of)
  // optional (one sequence, norm-fused, K <= 1024: the gate / up projection behind launch_oproj_head): the kernel's input is
  // x + x_parts[0] + ... + x_parts[x_nparts - 1] (rows of K floats, added in ascending order), and workgroup 0 stores that sum to
  // x_out [K], which must not overlap x or x_parts: every workgroup of the launch reads those
  const float* x_parts; int x_nparts; float* x_out;
  Q3A_STAMP_FIELD
};
constexpr int GEMV_X_PARTS_MAX = 4;
const char* launch_gemv(const GemvArgs& a, int NB, hipStream_t s);

// o_proj of the one-sequence chain by column slice (k_gemv.hip oproj_head_kernel): the K = n_q * 128 columns are cut into n_parts
// slices of 512 -- two kv heads of two q heads each (one kv head per slice, 8 partial vectors at the models' shapes, measured 3 us per
// step slower: profiles/oproj_by_head_headline_ab.txt); workgroup (slice p, row block) merges the flash-decoding partials of the slice's q heads ONCE, through
// LDS, streams its rows of the slice and stores their dot products to y_part[p][n] -- fp32, no residual (the bias, if any, rides in
// slice 0).  The consumer adds the n_parts vectors to the residual (GemvArgs::x_parts).  Default arithmetic (hardware exponential).
struct OprojHeadArgs {
  const float* pm; const float* pl; const float* po; int nsplit;  // partials of launch_decode_attn: [n_q][nsplit]( [128]), one sequence
  const uint16_t* W; int N; int K;                                // bf16 [N][K], K = n_q * 128
  const float* bias;                                              // [N] or null
  int n_parts;                                                    // K / n_parts = 512 columns (two kv heads of two q heads)
  float* y_part;                                                  // [n_parts][N]
  Q3A_STAMP_FIELD
};
constexpr int OPROJ_HEAD_MAX_SPLITS = 16;
const char* oproj_head_check(const OprojHeadArgs& a);  // null when the launch can run on these arguments
const char* launch_oproj_head(const OprojHeadArgs& a, hipStream_t s);
constexpr int GEMV_ATTN_MAX_TABLE = 1024;  // min(NB,4) * heads * nsplit must fit (else merge with launch_attn_combine first)
int gemv_blocks(const GemvArgs& a);        // grid size launch_gemv uses (= number of argmax partials in mode 3)
int gemv_rows_per_wave(const GemvArgs& a);

// Exact argmax of the one-sequence lm_head (mode 3, fused final norm) from an int8 pre-pass (k_gemv.hip): pass 1 streams the int8
// copy and writes per 16-row block lo_b / hi_b of the approximate logits +- a rigorous bound; pass 2 (`groups` workgroups) rescores
// with the bf16 arithmetic of the unpruned launch only the blocks with hi_b >= max lo_b and leaves ONE argmax partial per workgroup in
// g.part (argmax_finalize with n_part = groups; no log-sum channel).  The ids are those of launch_gemv.
struct LmHeadPruneArgs {
  GemvArgs g;                   // the mode-3 launch it replaces (g.out is not written by pass 1; pass 2 stores rescored rows if set)
  const int8_t* Wq; int qcols;  // launch_lm_head_quantize: [N][qcols], columns in the GEMV's lane order
  const float* qs;              // [N][4] {s, ||W - sQ||, ||W||, ||sQ||}
  float* blk_lo; float* blk_hi; // [lm_head_prune_blocks(g)] (pass 1 -> pass 2; blk_lo readable as float4: round up to 4)
  float* dbg;                   // nullable: [N][2] (approximate logit, bound) per row (pass 1)
  int* stats;                   // nullable: [2] += candidate blocks, += 1 per pass 2 (debug; the step never reads it)
  int logit_bias;               // 1: g.bias is the logit bias (every entry finite or -inf): both passes add it and the bound is the
                                // extended one (k_gemv.hip, above LmHeadArgsDev); 0 with g.bias set: refused
};
// columns of one int8 lm_head row (a multiple of 1024: 16 (32) bytes per lane of a wave), 0 = hidden size beyond the GEMV
inline int lm_head_q_cols(int hidden) { return hidden <= 1024 ? 1024 : hidden <= 2048 ? 2048 : 0; }
// int8 copy of a bf16 [N][K] lm_head for LmHeadPruneArgs (one launch at engine set-up): Q [N][cols] zero-padded, row r scaled by
// s_r = max|W_r| / 127 (rounded to nearest), columns in the GEMV's lane order (lane l owns columns l*8 + it*512 + e, it < cols/512,
// e < 8, as ONE piece of cols/64 bytes); qs [N][4] = {s, ||W - sQ||, ||W||, ||sQ||}, the norms in fp64, rounded up to fp32
const char* launch_lm_head_quantize(const uint16_t* W, int N, int K, int8_t* Q, float* qs, hipStream_t s);
int lm_head_prune_blocks(const GemvArgs& g);
int lm_head_rescore_groups(const GemvArgs& g, int n_cu);
const char* lm_head_prune_check(const LmHeadPruneArgs& a);  // null when both passes can run on these arguments
const char* launch_lm_head_approx(const LmHeadPruneArgs& a, hipStream_t s);
const char* launch_lm_head_rescore(const LmHeadPruneArgs& a, int groups, hipStream_t s);

// Skinny MFMA GEMM (k_skinny.hip): 4 < S <= 32 sequences, weights streamed once.
struct SkinnyArgs {
  const float* x; int ldx; int S;   // [S][K] fp32 ...
  const uint16_t* x16;              // ... or, when non-null, the same as bf16 (default mode: written by the producer)
  int x16_frag;                     // x16 is in MFMA-fragment order (skinny_frag_index) instead of row-major [S][K]
  int out16_frag;                   // out16 is written in that order (for the next skinny GEMM)
  const float* rms_w; float eps;    // non-null (fp32 x only): RMSNorm fused -- x*w enters the MFMA, rstd scales the result
  const uint16_t* W; int N; int K;  // bf16 [N][K]
  const float* bias;                // [N] or null
  int mode;                         // 0: store, 1: out = resid + y, 2: GLU ([16 gate|16 up] row blocks, out has N/2 columns)
  float* out; int ldo;
  uint16_t* out16;                  // mode 2 only: when non-null the result is written here as bf16 instead of out
  const float* resid;
  // Pre-normalised input (default mode, replaces x + rms_w): xw16f = bf16(x * w_norm) in fragment order and
  // ss_parts[p][32] = partial sums of x^2 (p < ss_nparts) -- both written by the kernel that produced x (below), so
  // this GEMM's activation loads are lane-linear and the RMSNorm still costs no launch.  eps as above.
  const uint16_t* xw16f; const float* ss_parts; int ss_nparts;
  // mode 1 only, producer side of the above for the NEXT GEMM (null: off): after out = resid + y is stored,
  // next_xw16f[frag(s, n)] = bf16(out * next_w[n]) and next_ss[blockIdx.x][s] = sum over the block's 16 columns of out^2
  const float* next_w; uint16_t* next_xw16f; float* next_ss;
  // mode 1, bf16 fragment-order x, N % 64 == 0: "quarter" workgroups of 8 rows x 16 sequences (k_skinny.hip); next_ss then has
  // N / 8 partial rows instead of N / 16 -- the caller sizes its buffers and the consumer's ss_nparts accordingly
  int qsplit;
  int qs_halves;  // (set by the launcher: 16-sequence halves per row tile)
  int glu_hp3;    // gate/up as 256 workgroups x 3 half-pair tiles (k_skinny.hip HP): 1 = when that balances the CUs (set by the engine from knob skinny_glu_hp3), 0 = never, 2 = whenever the shape allows
  int n_cu;       // compute units of the device the launch goes to (0: 256) -- chooses between the gate/up forms; set by the engine
  int fast_math;  // default mode: hardware rsq / exp / rcp in the RMSNorm scale and SiLU of the epilogue (dev.h rstd_of)
  Q3A_STAMP_FIELD
};
// the same producer duty for kernels that write a whole row of the residual stream (token embedding)
struct NextNormOut {
  const float* next_w;      // [H] norm weight of the GEMM that consumes the row next (null: off)
  uint16_t* next_xw16f;     // [32 * H] fragment order
  float* next_ss;           // [nparts][32]: row 0 receives the row's sum of squares, rows 1..nparts-1 zero
  int nparts;
  // more than 32 sequences: sequence s belongs to group s / 32, whose buffers start group_stride_* elements further on
  long group_stride_x, group_stride_ss;
  int group_size;  // sequences per group (0 means 32)
};
const char* launch_skinny(const SkinnyArgs& a, bool split, hipStream_t s);
const char* skinny_init();  // once per device before the first launch_skinny (sets the large-LDS kernel attributes)
// The skinny_kernel instantiation the calling thread's last launch_skinny ran (k_skinny.hip's template axes), its grid and its dynamic
// LDS bytes; all zero when that call launched nothing (S <= 0, a refusal).  For tests: which form serves a shape is part of what they check.
struct SkinnyForm { int split, tiles, sh, xmode, unr, wlds, qs, palias, hp, grid, dyn_lds; };
SkinnyForm skinny_last_form();
// Fragment order of a bf16 activation matrix for up to 32 sequences: the 16 B that lane (sequence s & 15, k-chunk
// (k >> 3) & 3) of a v_mfma_f32_16x16x32_bf16 B operand needs for k-step k >> 5 and sequence half s >> 4 sit at
// lane-linear offsets, so one wave load is 1 KiB contiguous (8 cache lines) instead of 16 rows x 64 B (16 lines).
// Buffers in this order always hold 32 sequences: 32 * K elements.
__host__ __device__ inline size_t skinny_frag_index(int s, int k) {
  return ((((size_t)(k >> 5) * 2 + (s >> 4)) * 4 + ((k >> 3) & 3)) * 16 + (s & 15)) * 8 + (k & 7);
}

struct DecodeAttnArgs {
  const float* qkv;            // [S][qkv_dim] fp32 (raw projections of the current token)
  const int* pos;              // [S] number of tokens already in the cache = position of the current token
  const float* q_norm; const float* k_norm; float eps;
  const float* rope_cur;       // [S][128]: cos (64) | sin (64) of position pos[s], maintained by launch_argmax_finalize
  void* kcache; void* vcache;  // this layer
  float* pm; float* pl;       // [S][n_q][nsplit] partial softmax max / sum per key split
  float* po;                   // [S][n_q][nsplit][128] unnormalised partial outputs
  int nsplit;                  // splits launched: every pos < nsplit * keys per split
  int keys_per_split;          // launch_decode_attn, bf16 cache, GQA group <= 2: 32 or 64 (4 waves per workgroup) or 128; 0 = dattn_keys_per_split
  int n_q, n_kv, max_ctx;
  float scale_div;
  // launch_decode_attn_batched only: when the batch alone fills the chip (S * n_kv workgroups), one workgroup walks ALL
  // keys of its (sequence, kv head) and writes the normalised context itself -- no partials, no merge launch:
  float* out;                  // [S][n_q*128] fp32 (precise mode) ...
  uint16_t* out16;             // ... or bf16 (default mode), row-major or, with out_frag, in skinny_frag_index order
  int out_frag;
  int trim_prologue;           // batched kernel: 1 = some sequence of the batch is shorter than the two prologue key tiles, trim them to the live rows too
  Q3A_STAMP_FIELD
};
constexpr int DATTN_KEYS_PER_SPLIT_BF16 = 128, DATTN_KEYS_PER_SPLIT_F32 = 128;  // (DecodeAttnArgs::keys_per_split = 0)
inline int dattn_keys_per_split(bool kv_f32) { return kv_f32 ? DATTN_KEYS_PER_SPLIT_F32 : DATTN_KEYS_PER_SPLIT_BF16; }
// Keys per split of the one-sequence chain whose o_proj runs per pair of kv heads (launch_oproj_head merges at most OPROJ_HEAD_MAX_SPLITS
// partials per head): the smallest size that keeps the live splits of a context of `keys` keys (the new token's included) at 16 or
// fewer; 0: beyond the table, the chain with launch_gemv's merging o_proj runs.
inline int dattn_fine_keys_per_split(int keys) { return keys <= 512 ? 32 : keys <= 1024 ? 64 : keys <= 2048 ? 128 : 0; }
const char* launch_decode_attn(const DecodeAttnArgs& a, int S, bool kv_f32, hipStream_t s);
// one workgroup per (sequence, kv head), online softmax over 128-key tiles, final output written directly (a.out / a.out16)
const char* launch_decode_attn_batched(const DecodeAttnArgs& a, int S, bool kv_f32, hipStream_t s);
// out[S][n_q*128] = merged partials (needed as its own launch only on the GEMM decode path)
const char* launch_attn_combine(const float* pm, const float* pl, const float* po, int nsplit, int S, int n_q, float* out,
                                hipStream_t s, uint16_t* out16 = nullptr, bool frag = false);
// out16 != null: bf16 there instead of out; frag: in skinny_frag_index order (S <= 32)

// The state a committed token leaves behind, whichever kernel commits it (argmax_finalize, draft_accept; set_tokens writes the
// part a fed token has: next_tok, x_next, nn).  The device side is step_commit.h.
struct StepCommit {
  int* next_tok;           // [S] token to feed next (written)
  int* out_ids;            // [S][out_stride] generated ids (written at the token's slot: the step_count[s] it was chosen at)
  int out_stride;
  // token log-probabilities (nullable): [S][out_stride] logit[id] - logsumexp(logits) of the chosen id next to out_ids (NaN where
  // the all-NaN guard fires)
  float* out_lp;
  int* step_count;         // [S] ids generated so far
  int* pos;                // [S] position of the token to feed next
  uint8_t* done;           // [S] sticky: set when the token is EOS
  int* n_done;             // device counter of sequences whose done flag is set (nullable); n_seq = sequences in the batch
  int n_seq;
  int* host_progress;      // pinned host words the greedy loop's host side polls WITHOUT synchronising the stream (nullable):
                           // [0] = step_count of sequence 0 (prefill counts as 1), [1] = 1 once every
                           // sequence has produced its EOS (src/inference.rs:163-165 evaluated for the whole batch on the device)
  const uint16_t* embed; int H;
  float* x_next;           // [S][H] embedding of the chosen token
  int eos0, eos1;
  const float* cos_t; const float* sin_t;  // RoPE tables [max_pos][64]
  float* rope_cur;         // [S][128] (written): cos | sin row of the updated pos[s] (DecodeAttnArgs::rope_cur); nullable
  NextNormOut nn;          // pre-normalised copy of x_next for the first layer's qkv GEMM (skinny path)
};
// The one host check of a StepCommit for S sequences, in the words of the launcher that calls it: required pointers, H >= 4 and
// H % 4 == 0, out_stride >= 1, rope_cur needs the tables, more than 32 sequences with nn.next_w need group strides.  fed_only:
// only what launch_set_tokens reads (next_tok, embed, H, x_next, nn).
struct StepCommitMsgs { const char *null_arg, *shape, *rope, *groups; };
#define Q3A_STEP_COMMIT_MSGS(who) \
  q3a::StepCommitMsgs { who ": null argument", who ": bad shape", who ": rope_cur needs the tables", who ": more than 32 sequences need group strides" }
inline const char* step_commit_check(const StepCommit& c, int S, const StepCommitMsgs& m, bool fed_only = false) {
  if (!c.next_tok || !c.embed || !c.x_next) return m.null_arg;
  if (c.H < 4 || c.H % 4 != 0) return m.shape;
  if (c.nn.next_w && S > 32 && (c.nn.group_stride_x <= 0 || c.nn.group_stride_ss <= 0)) return m.groups;
  if (fed_only) return nullptr;
  if (!c.out_ids || !c.step_count || !c.pos || !c.done) return m.null_arg;
  if (c.out_stride < 1) return m.shape;
  if (c.rope_cur && (!c.cos_t || !c.sin_t)) return m.rope;
  return nullptr;
}
struct FinalizeArgs {
  ArgmaxPartials part;     // [S] rows of n_part partials; with part.sum (and c.out_lp) the token log-probabilities
  int n_part;
  int V;
  int advance;             // c.pos[s] += advance
  StepCommit c;
};
// nblk block partials per row of logits [S][V] (GEMM decode path; the GEMV lm_head produces its own)
const char* launch_argmax_partials(const float* logits, int V, int S, const ArgmaxPartials& p, int nblk, hipStream_t s);
const char* launch_argmax_finalize(const FinalizeArgs& a, int S, hipStream_t s);
// c.x_next[s] = embed[tok[s]] (+ c.nn); c.next_tok[s] = tok[s]  (teacher forcing)
const char* launch_set_tokens(const int* tok, int S, const StepCommit& c, hipStream_t s);

// ---- draft verification (k_draft.hip) ------------------------------------------------------------------------
// After ONE prefill of prompt ++ draft and the scoring head at the n + 1 rows p - 1 .. p - 1 + n of every sequence (top_id / top_lp of
// ScoreHeadArgs): the first position k at which the head's argmax differs from the draft (n if none), and the state the greedy loop
// has after producing the k + 1 tokens d_0 .. d_{k-1}, top_id[k] -- everything launch_argmax_finalize would have left behind.
// One workgroup per sequence.  Sequence s owns draft[draft_off[s] .. draft_off[s + 1]) and head rows draft_off[s] + s + i.
struct DraftAcceptArgs {
  int n_seq;
  const int* draft; const int* draft_off;  // [draft_off[n_seq]] ids, [n_seq + 1] offsets
  const int* prompt_len;                   // [n_seq] p: the prompt without the draft
  const int* top_id; const float* top_lp;  // [draft_off[n_seq] + n_seq] of the verify head; top_lp read only with c.out_lp
  int* accepted;                           // [2 n_seq] (written): k per sequence, then the token top_id[k] per sequence
  StepCommit c;                            // all written: step_count = k + 1, pos = p + k, out_ids / out_lp at slots 0 .. k
};
const char* launch_draft_accept(const DraftAcceptArgs& a, hipStream_t s);

// ---- beam search (k_beam.hip) --------------------------------------------------------------------------------
constexpr int BEAM_MAX_W = 8;       // slots per utterance
constexpr int BEAM_CHUNK = 2048;    // logits one workgroup of the top-W selection reads (8 per thread)
constexpr int KV_REORDER_SLICES = 8;  // workgroups that share the rows of one (layer, K / V, kv head): a fixed grid, capturable
inline int beam_topk_chunks(int V) { return (V + BEAM_CHUNK - 1) / BEAM_CHUNK; }
// Per row of logits [S][V] (fp32, row stride V): the W best ids (larger logit, then smaller id; -inf is a legal logit and ranks
// last) and lp = (l - m) - log sum exp(l - m) of each, m the row maximum, the sum in fp32 in a fixed order.  Any V >= W.
struct BeamTopkArgs {
  const float* logits; int S; int V; int W;
  float* cand_val; int* cand_idx;    // workspace [S][beam_topk_chunks(V)][W]
  float* part_max; float* part_sum;  // workspace [S][beam_topk_chunks(V)]
  int* out_ids; float* out_lp;       // [S][W], best first
};
const char* launch_beam_topk(const BeamTopkArgs& a, hipStream_t s);
// state words of a search (device ints, BeamAdvanceArgs::state); the first four are q3a_debug_read "beam_stats"
enum { BEAM_ST_ROUNDS = 0, BEAM_ST_COPIES = 1, BEAM_ST_KV_ROWS = 2, BEAM_ST_FINISHED = 3, BEAM_ST_ALL_DONE = 4, BEAM_ST_LAUNCHES = 5, BEAM_ST_COUNT = 8 };
// One round of U utterances x W slots (sequence u * W + j = slot j of utterance u), include/q3asr.h "beam search".  score / finished
// are the state before the round and are overwritten with the state after it.  A launch that finds BEAM_ST_ALL_DONE set changes
// nothing but BEAM_ST_LAUNCHES and host_progress[0].
struct BeamAdvanceArgs {
  int U, W;
  const int* topk_ids; const float* topk_lp;  // [U * W][W] of launch_beam_topk
  float* score; uint8_t* finished;            // [U * W]
  int* parent;                                // [U * W] sequence the slot's new hypothesis continues (itself: no copy)
  int* token;                                 // [U * W] the survivor's token: an EOS id when it finishes now, -1 for a hypothesis that was finished (or an empty slot)
  int* feed;                                  // nullable [U * W]: the id the next step feeds (0 for a finished slot)
  int* hist_parent; int* hist_token; float* hist_lp; int hist_cap;  // nullable [hist_cap][U * W]: row BEAM_ST_ROUNDS receives parent / token / lp
  int* state;                                 // [BEAM_ST_COUNT]
  const int* pos; const int* lo; int hi_bias; // nullable: rows lo[s] .. pos[s] + hi_bias are what a copy moves (BEAM_ST_KV_ROWS)
  int* host_progress;                         // nullable pinned host words: [0] = BEAM_ST_LAUNCHES, [1] = 1 once every slot is finished
  int eos0, eos1;
};
const char* launch_beam_advance(const BeamAdvanceArgs& a, hipStream_t s);
// For every sequence j with parent[j] != j: rows lo[j] .. hi[j] + hi_bias of K and V, every layer and kv head, become a copy of the
// same rows of sequence parent[j] as they were before the launch (parent[j] must share j's lo and hi: a slot of the same utterance).
// Any permutation with cycles and fan-out; nothing outside those rows is read or written.
struct KvReorderArgs {
  void* kcache; void* vcache;  // [layers][S][n_kv][max_ctx][128] elements each
  int elem_bytes;              // 2 (bf16) or 4 (fp32)
  int layers, S, n_kv, max_ctx;
  const int* parent; const int* lo; const int* hi; int hi_bias;
  const int* all_done;         // nullable device word: non-zero = do nothing
};
const char* launch_kv_reorder(const KvReorderArgs& a, hipStream_t s);

// ---- temperature sampling (k_sample.hip) -----------------------------------------------------------------------
constexpr int SAMPLE_CHUNK = 2048;  // logits one workgroup of the sampler reads (8 per thread)
inline int sample_chunks(int V) { return (V + SAMPLE_CHUNK - 1) / SAMPLE_CHUNK; }
// Per row s of logits [S][V] (fp32, row stride V): with m the row maximum, the kept set { j : l_j >= m + T ln(min_p), l_j != -inf }
// and z_j = l_j + T g_j, g_j the Gumbel noise of sample_word(seed, s, step_count[s], j) (sample_rng.h), ONE argmax partial per
// 2048-logit chunk: the chunk's largest z and its id.  launch_argmax_finalize with n_part = sample_chunks(V) picks the row's id.
// Two launches: the clean (max, sum exp) pair of every chunk, then the noisy partials.
struct SampleArgs {
  const float* logits; int S; int V;
  const uint32_t* params;              // device [4]: temperature and min_p (fp32 bits), seed low and high word
  int row_stride;                      // words between the records of two rows: 0 one record for all rows, 4 a record per row
                                       // (q3asr.h "row options"); a row with temperature 0 takes the argmax of its finite entries
  const int* step_count;               // [S] the step t of each sequence (tokens it has generated so far)
  float* chunk_max; float* chunk_sum;  // [S][sample_chunks(V)] (written)
  ArgmaxPartials part;                 // (written) [S] rows x sample_chunks(V) partials, no log-sum channel
};
const char* launch_sample(const SampleArgs& a, hipStream_t s);
// Top-k / top-p (q3asr.h "sampling filter").  launch_sample with two launches between its two: the threshold stage writes
// tau_sel[s] = max(tau_k, tau_p) (a row value or -inf) and kept[s] = #{ j : l_j >= tau_sel[s], l_j != -inf }, and the kept set of the
// noisy partials becomes { l >= max(m + T ln(min_p), tau_sel[s]), l != -inf }.  An exact radix select over the order-preserving
// uint32 key of the logit: integer counts for top-k, fixed-point weights (uint64)(exp((l - m) / T) 2^40) for top-p.
constexpr int SAMPLE_BUCKETS = 2048;  // the select's first digit: the top 11 bits of the key
struct SampleFilterArgs {
  const uint32_t* filter;              // device [4]: top_k, top_p (fp32 bits), 0, 0 -- as validated by the setter
  int row_stride;                      // as SampleArgs::row_stride (the two agree); a row with (0, 1.0f) gets tau_sel = -inf
  uint32_t* hist_cnt;                  // [S][SAMPLE_BUCKETS] entries per first digit: ZERO on entry, zero again when the stage returns
  unsigned long long* hist_mass;       // [S][SAMPLE_BUCKETS] their summed weights; likewise
  float* tau_sel; int* kept;           // [S] (written)
};
const char* launch_sample_filtered(const SampleArgs& a, const SampleFilterArgs& f, hipStream_t s);
// After launch_argmax_finalize: lp = (l_id - m) - log sum exp(l - m) of the id it chose (next_tok[s]), the sum merged in a fixed
// order, written to out_lp[s][step_count[s] - 1] -- the entry finalize filled for this step; out_z[s] = the winning noisy score.
struct SampleLogprobArgs {
  const float* logits; int S; int V;
  const float* chunk_max; const float* chunk_sum;  // of launch_sample
  const int* next_tok; const int* step_count;      // [S] as finalize left them
  float* out_lp; int out_stride;                   // nullable [S][out_stride]
  ArgmaxPartials part; float* out_z;               // nullable [S] (selftest), with the partials of launch_sample
};
const char* launch_sample_logprob(const SampleLogprobArgs& a, hipStream_t s);

// ---- top log-probabilities (k_toplp.hip) --------------------------------------------------------------------------
constexpr int TOP_LP_MAX = 20;  // entries per step: the largest n, and the fixed inner stride of the history and of the candidates
// Per row s of logits [S][V] (fp32, row stride V) that is not done and has a slot t = step_count[s] < out_stride: the n = min(*n_dev,
// TOP_LP_MAX, V) best entries -- larger logit first, then smaller id; -0.0 and +0.0 one value; -inf last -- as out_ids / out_lp
// [s][t][0 .. n), lp = (l - m) - log sum exp(l - m) in fp32 with a fixed summation order (-inf exactly where l is -inf).  Any other row
// writes nothing.  Two launches: the chunk grid (candidates and (max, sum) per 2048-logit chunk), then one workgroup per row.  It only
// reads the logits; it runs behind the step's last rewriting kernel and in front of launch_argmax_finalize, which advances step_count.
struct TopLpArgs {
  const float* logits; int S; int V;
  const int* n_dev;                    // device [1]: n as last set (read by the kernel: another n > 0, the same launch)
  const int* step_count;               // [S]
  const uint8_t* done;                 // [S]
  unsigned long long* cand;            // [S][sample_chunks(V)][TOP_LP_MAX] (written) the chunks' best entries as ordered words
  float* chunk_max; float* chunk_sum;  // [S][sample_chunks(V)] (written)
  int* out_ids; float* out_lp;         // [S][out_stride][TOP_LP_MAX] the history
  int out_stride;
};
constexpr int TOP_LP_MAX_VOCAB = 400 * 2048;  // the row kernel keeps every chunk's candidates in LDS (400 chunks x 20 x 8 bytes)
const char* launch_top_logprobs(const TopLpArgs& a, hipStream_t s);

// ---- repetition penalty and no-repeat n-grams (k_repeat.hip: repeat_apply_kernel) --------------------------------
constexpr int REPEAT_MAX_VOCAB = 1 << 18;  // ids the kernel's LDS bitmap holds (8192 words, 32 KB)
constexpr int REPEAT_HIST_LDS = 4096;      // ids of a history kept in LDS (16 KB); a longer history is read in place beyond them
// Per row s of logits [S][V] (fp32, row stride V), rewritten IN PLACE: with h = out_ids[s][0 .. t), t = min(step_count[s], out_stride),
// every distinct id j of h gets l_j / p where l_j > 0 and l_j * p elsewhere (once, however often it occurred), then every id that
// would complete an n-gram already in h gets -inf (n >= 1, t >= n - 1).  t = 0 leaves the row as it is.  One launch, one workgroup
// per row; it runs before launch_argmax_partials / launch_sample, which then see l''.
struct RepeatArgs {
  float* logits; int S; int V;
  const uint32_t* params;              // device [4]: p (fp32 bits), n, 0, 0 -- as validated by the setter: p finite and > 0, 0 <= n <= 32
  int row_stride;                      // words between the records of two rows: 0 one record for all rows, 4 a record per row
  const int* out_ids; int out_stride;  // [S][out_stride] the ids generated so far
  const int* step_count;               // [S]
};
const char* launch_repeat_apply(const RepeatArgs& a, hipStream_t s);

// ---- sequence bias (k_repeat.hip: seqbias_apply_kernel) ----------------------------------------------------------
constexpr int SEQBIAS_MAX_ENTRIES = 4096;  // entries over all lists (and so target groups)
constexpr int SEQBIAS_MAX_LISTS = 256;     // lists of q3a_set_sequence_bias_lists
constexpr int SEQBIAS_MAX_LEN = 32;        // ids of one entry
constexpr int SEQBIAS_MAX_IDS = 65536;     // ids over all entries
// Per row s of logits [S][V] (fp32, row stride V), rewritten IN PLACE: with h = out_ids[s][0 .. t), t = min(step_count[s], out_stride),
// an entry q_0 .. q_{L-1} fires iff t >= L - 1 and h[t - L + 1 .. t) == q_0 .. q_{L-2}; for every target id with a firing entry,
// l_target += acc, acc = 0.0f + the biases of its firing entries in table order (one fp32 add each).  Entries are grouped by target:
// group g owns entries grp_begin[g] .. grp_begin[g + 1), entry e the leading ids pre_ids[ent_pre_off[e] .. ent_pre_off[e + 1]).
// Row s uses the groups of ITS list k = row_list[s * row_stride], list_begin[k] .. list_begin[k + 1) (k outside [0, SEQBIAS_MAX_LISTS):
// none, the row is left as it is); q3a_set_sequence_bias is the case of one list, and without a row table every row reads list 0.
// One launch, one workgroup per row; it runs before launch_repeat_apply / launch_argmax_partials / launch_sample.
struct SeqBiasArgs {
  float* logits; int S; int V;
  const int* params;                       // device [4]: groups G, entries E, 0, 0 (read by the kernel: another list, the same launch)
  const int* grp_target; const int* grp_begin;   // [SEQBIAS_MAX_ENTRIES], [SEQBIAS_MAX_ENTRIES + 1]
  const float* ent_bias; const int* ent_pre_off; // [SEQBIAS_MAX_ENTRIES], [SEQBIAS_MAX_ENTRIES + 1]
  const int* pre_ids;                      // [SEQBIAS_MAX_IDS]
  const int* list_begin;                   // [SEQBIAS_MAX_LISTS + 1] first group of every list (groups of one list are contiguous)
  const int* row_list; int row_stride;     // the list of row s at row_list[s * row_stride]; stride 0: one word for all rows
  const int* out_ids; int out_stride;      // [S][out_stride] the ids generated so far
  const int* step_count;                   // [S]
};
const char* launch_seqbias_apply(const SeqBiasArgs& a, hipStream_t s);
// The tables as ONE block of 32-bit words at fixed offsets (so one device buffer of fixed size holds any list), laid out on the host:
// entries sorted stably by target id, the one-token entry of a target first.
constexpr size_t SEQBIAS_OFF_TARGET = 4, SEQBIAS_OFF_BEGIN = SEQBIAS_OFF_TARGET + SEQBIAS_MAX_ENTRIES,
                 SEQBIAS_OFF_BIAS = SEQBIAS_OFF_BEGIN + SEQBIAS_MAX_ENTRIES + 1, SEQBIAS_OFF_PRE_OFF = SEQBIAS_OFF_BIAS + SEQBIAS_MAX_ENTRIES,
                 SEQBIAS_OFF_PRE_IDS = SEQBIAS_OFF_PRE_OFF + SEQBIAS_MAX_ENTRIES + 1, SEQBIAS_OFF_LISTS = SEQBIAS_OFF_PRE_IDS + SEQBIAS_MAX_IDS,
                 SEQBIAS_TABLE_WORDS = SEQBIAS_OFF_LISTS + SEQBIAS_MAX_LISTS + 1;  // (the list directory behind pre_ids: no older offset moves)
// the kernel's table pointers into a device copy of that block (engine_internal.h seqbias_layout writes it).  Every row reads list 0
// (word 2 of the block's head is always 0) until the caller points row_list at a row table.
inline void seqbias_point(SeqBiasArgs& a, const void* table_dev) {
  const int* const w = static_cast<const int*>(table_dev);
  a.params = w; a.grp_target = w + SEQBIAS_OFF_TARGET; a.grp_begin = w + SEQBIAS_OFF_BEGIN;
  a.ent_bias = reinterpret_cast<const float*>(w + SEQBIAS_OFF_BIAS); a.ent_pre_off = w + SEQBIAS_OFF_PRE_OFF; a.pre_ids = w + SEQBIAS_OFF_PRE_IDS;
  a.list_begin = w + SEQBIAS_OFF_LISTS; a.row_list = w + 2; a.row_stride = 0;
}

}  // namespace q3a
