// q3a_selftest_*: product kernels on their own (no model) -- host arrays in, the product launches, host arrays or error figures out.
#include <cmath>
#include <cstring>

#include "engine_internal.h"
#include "sample_rng.h"

using namespace q3a;

namespace {

// ---- staging: every selftest runs on the null stream with blocking copies ----
void use_device(int device) {
  if (int n_dev = 0; hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) fail("no HIP device available");
  HIPCHK(hipSetDevice(device));
}
DevBuf room(size_t bytes) { DevBuf b; b.ensure(bytes); return b; }
template <class T> DevBuf to_device(const T* src, size_t n) {
  DevBuf b = room(n * sizeof(T));
  HIPCHK(hipMemcpy(b.p, src, n * sizeof(T), hipMemcpyHostToDevice));
  return b;
}
template <class T> DevBuf to_device(const std::vector<T>& v) { return to_device(v.data(), v.size()); }
template <class T> void to_host(T* dst, const DevBuf& b, size_t n) { HIPCHK(hipMemcpy(dst, b.p, n * sizeof(T), hipMemcpyDeviceToHost)); }
template <class T> std::vector<T> to_host(const DevBuf& b, size_t n) { std::vector<T> v(n); to_host(v.data(), b, n); return v; }
void finish() { HIPCHK(hipDeviceSynchronize()); HIPCHK(hipGetLastError()); }

// ---- test data ----
struct Lcg {  // uniform in [-0.5, 0.5)
  uint32_t st;
  float operator()() { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xffff) / 65536.0f - 0.5f; }
};
uint16_t bf16_trunc(float f) { uint32_t u; memcpy(&u, &f, 4); return (uint16_t)(u >> 16); }  // truncation is fine for a test
float bf16_value(uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; }

// x [M][K] fp32 (bf16-representable when exact16) and w [N][K] bf16 from one generator, with room for a product Y and the reference R
struct GemmCase {
  std::vector<float> X, R;
  std::vector<uint16_t> W;
  const size_t MN;  DevBuf dX, dW, dY, dR;
  GemmCase(Lcg& rnd, int M, int N, int K, bool exact16) : X((size_t)M * K), W((size_t)N * K), MN((size_t)M * N) {
    for (auto& v : X) { v = rnd(); if (exact16) v = bf16_value(bf16_trunc(v)); }
    for (auto& v : W) v = bf16_trunc(rnd());
    dX = to_device(X); dW = to_device(W); dY = room(MN * 4); dR = room(MN * 4);
  }
  // after the launch under test wrote dY: the reference product, then max |Y - R| and max |R|
  void check(int M, int N, int K, float& me, float& rm) {
    launch_gemm_ref(dX.as<float>(), dW.as<uint16_t>(), dR.as<float>(), M, N, K, nullptr);
    finish();
    R = to_host<float>(dR, MN);
    const std::vector<float> Y = to_host<float>(dY, MN);
    for (size_t i = 0; i < MN; ++i) { me = std::max(me, std::fabs(Y[i] - R[i])); rm = std::max(rm, std::fabs(R[i])); }
  }
};

// An output buffer between two guard zones.  The caller's bytes (pre-filled with its sentinel) go up, the launch under test writes what
// it writes, and the bytes come back whole; a guard byte that changed is a write outside the buffer and fails the call.
struct Guarded {
  static constexpr size_t ZONE = 4096;
  static constexpr uint8_t FILL = 0xA5;
  DevBuf b;
  size_t bytes = 0;
  Guarded() = default;
  Guarded(const void* host, size_t n) : bytes(n) {
    std::vector<uint8_t> img(n + 2 * ZONE, FILL);
    memcpy(img.data() + ZONE, host, n);
    b = to_device(img);
  }
  template <class T> T* as() const { return b.p ? reinterpret_cast<T*>(static_cast<uint8_t*>(b.p) + ZONE) : nullptr; }
  void fetch(void* host, const char* what) const {
    const std::vector<uint8_t> img = to_host<uint8_t>(b, bytes + 2 * ZONE);
    for (size_t i = 0; i < ZONE; ++i)
      if (img[i] != FILL || img[ZONE + bytes + i] != FILL) fail(std::string("selftest: a byte outside the ") + what + " buffer was written");
    memcpy(host, img.data() + ZONE, bytes);
  }
};

// A StepCommit over a test's own buffers: the counters and rows every commit writes.  The caller adds what its launch also keeps
// (n_done and the progress words, the RoPE row, the pre-normalised copy); left out, they are off.
StepCommit bare_commit(int S, const DevBuf& tok, int* out_ids, int out_stride, float* out_lp, const DevBuf& step_count, const DevBuf& pos,
                       const DevBuf& done, const uint16_t* embed, int H, float* x_next, int eos0, int eos1) {
  StepCommit c{};
  c.next_tok = tok.as<int>(); c.out_ids = out_ids; c.out_stride = out_stride; c.out_lp = out_lp;
  c.step_count = step_count.as<int>(); c.pos = pos.as<int>(); c.done = done.as<uint8_t>(); c.n_seq = S;
  c.embed = embed; c.H = H; c.x_next = x_next; c.eos0 = eos0; c.eos1 = eos1;
  return c;
}

}  // namespace

extern "C" {

int32_t q3a_gemm256_split_rows(int32_t M, int32_t N) { return gemm256_split_rows(M, N); }

int32_t q3a_selftest_gemm_launch(int32_t device, int32_t launcher, int32_t flags, const void* x, const uint16_t* w, int32_t M, int32_t N, int32_t K,
                                 int32_t lda, int32_t ldo, int32_t imgs, int32_t H, int32_t Wd, int32_t C, const float* bias, const float* addend,
                                 int32_t addend_period, const float* resid, const int32_t* rowmap, int32_t act, void* out, int32_t out_rows) {
  Q3A_TRY(nullptr)
  use_device(device);
  const bool split = flags & 1, glu = flags & 2, o16 = flags & 4, alias = flags & 8;
  const bool conv = launcher == 3 || launcher == 4, x16 = launcher == 1 || launcher == 2 || launcher == 4;
  // every index the launch will form is checked here: a refusal, never an access outside a buffer
  if (launcher < 0 || launcher > 4 || (flags & ~15) || !x || !w || !out || M < 1 || N < 1 || K < 1 || out_rows < 1 || (act != 0 && act != 1))
    fail("q3a_selftest_gemm_launch: bad argument");
  if (conv) {
    if (imgs < 1 || H < 1 || Wd < 1 || C < 1 || C % 32 != 0 || K != 9 * C || glu) fail("q3a_selftest_gemm_launch: bad convolution geometry");
    if ((long)M != (long)imgs * ((H - 1) / 2 + 1) * ((Wd - 1) / 2 + 1)) fail("q3a_selftest_gemm_launch: M is not imgs * OH * OW");
  } else if (lda < K) fail("q3a_selftest_gemm_launch: lda < K");
  if (glu && N % 32 != 0) fail("q3a_selftest_gemm_launch: GLU needs N % 32 == 0");
  if (ldo < (glu ? N / 2 : N)) fail("q3a_selftest_gemm_launch: ldo smaller than the output row");
  if (o16 && !x16) fail("q3a_selftest_gemm_launch: the fp32-activation kernels have no bf16 output");
  if (split && x16) fail("q3a_selftest_gemm_launch: split belongs to the fp32-activation kernels");
  if (alias && (resid || o16)) fail("q3a_selftest_gemm_launch: an aliased residual is the fp32 output buffer itself");
  if (addend && addend_period < 1) fail("q3a_selftest_gemm_launch: addend period");
  if (rowmap) {
    for (int m = 0; m < M; ++m)
      if (rowmap[m] >= out_rows) fail("q3a_selftest_gemm_launch: row map points past the output");
  } else if (out_rows < M) fail("q3a_selftest_gemm_launch: output has fewer rows than the product");
  const size_t n_out = (size_t)out_rows * ldo, n_x = conv ? (size_t)imgs * H * Wd * C : (size_t)M * lda;
  const DevBuf dX = to_device((const uint8_t*)x, n_x * (x16 ? 2 : 4)), dW = to_device(w, (size_t)N * K);
  const DevBuf dZero = to_device(std::vector<uint16_t>(128, 0));
  DevBuf dB, dA, dS, dM;
  if (bias) dB = to_device(bias, (size_t)N);
  if (addend) dA = to_device(addend, (size_t)addend_period * ldo);
  if (resid) dS = to_device(resid, n_out);
  if (rowmap) dM = to_device(rowmap, (size_t)M);
  const Guarded dO(out, n_out * (o16 ? 2 : 4));
  GemmEpilogue ep;
  if (o16) ep.out16 = dO.as<uint16_t>(); else ep.out = dO.as<float>();
  ep.ldo = ldo; ep.bias = dB.as<float>(); ep.act = act; ep.rowmap = dM.as<int>();
  ep.resid = alias ? dO.as<float>() : dS.as<float>();
  ep.addend = dA.as<float>(); ep.addend_period = addend ? addend_period : 1;
  switch (launcher) {
    case 0: KCHK(launch_gemm(dX.as<float>(), lda, dW.as<uint16_t>(), M, N, K, ep, glu, split, nullptr)); break;
    case 1: KCHK(launch_gemm16(dX.as<uint16_t>(), lda, dW.as<uint16_t>(), M, N, K, ep, glu, nullptr)); break;
    case 2: KCHK(launch_gemm16_small(dX.as<uint16_t>(), lda, dW.as<uint16_t>(), M, N, K, ep, glu, nullptr)); break;
    case 3: KCHK(launch_conv3x3s2_gemm(dX.as<float>(), imgs, H, Wd, C, dW.as<uint16_t>(), N, ep, split, nullptr)); break;
    default: KCHK(launch_conv3x3s2_gemm16(dX.as<uint16_t>(), dZero.as<uint16_t>(), imgs, H, Wd, C, dW.as<uint16_t>(), N, ep, nullptr)); break;
  }
  finish();
  dO.fetch(out, "output");
  Q3A_CATCH(nullptr)
}

int32_t q3a_selftest_qkrope_launch(int32_t device, int32_t fused, int32_t kv_f32, const uint16_t* x, int32_t lda, const uint16_t* w, int32_t M, int32_t K,
                                   const float* bias, float* qkv, const int32_t* row_seq, const int32_t* row_pos, const float* q_norm,
                                   const float* k_norm, float eps, const float* cos_t, const float* sin_t, int32_t max_pos, int32_t n_q, int32_t n_kv,
                                   int32_t n_seq, int32_t max_ctx, uint16_t* q16, void* kcache, void* vcache) {
  Q3A_TRY(nullptr)
  use_device(device);
  if (!row_seq || !row_pos || !q_norm || !k_norm || !cos_t || !sin_t || !kcache || !vcache || M < 1 || n_q < 1 || n_kv < 1 || n_seq < 1 || max_ctx < 1 ||
      max_pos < 1)
    fail("q3a_selftest_qkrope_launch: bad argument");
  const int N = (n_q + 2 * n_kv) * 128;
  if (fused) {
    if (!x || !w || !q16 || kv_f32 || K < 128 || K % 64 != 0 || lda < K || lda % 8 != 0)
      fail("q3a_selftest_qkrope_launch: the fused form needs bf16 x / W, K % 64 == 0, K >= 128, a bf16 q and a bf16 cache");
  } else if (x || w || bias || !qkv) fail("q3a_selftest_qkrope_launch: the separate kernel takes the fp32 qkv matrix alone");
  {  // every cache row a token names exists and is named once (two rows on one cache row would race)
    std::vector<char> seen((size_t)n_seq * max_ctx, 0);
    for (int m = 0; m < M; ++m) {
      if (row_seq[m] < 0 || row_seq[m] >= n_seq || row_pos[m] < 0 || row_pos[m] >= max_ctx || row_pos[m] >= max_pos)
        fail("q3a_selftest_qkrope_launch: a row's sequence or position is outside the cache or the RoPE table");
      char& s = seen[(size_t)row_seq[m] * max_ctx + row_pos[m]];
      if (s) fail("q3a_selftest_qkrope_launch: two rows name one cache row");
      s = 1;
    }
  }
  const size_t n_cache = (size_t)n_seq * n_kv * max_ctx * 128, kv_bytes = n_cache * (kv_f32 ? 4 : 2), n_q16 = (size_t)M * n_q * 128;
  DevBuf dX, dW, dB;
  if (fused) { dX = to_device(x, (size_t)M * lda); dW = to_device(w, (size_t)N * K); }
  if (bias) dB = to_device(bias, (size_t)N);
  const DevBuf dSeq = to_device(row_seq, (size_t)M), dPos = to_device(row_pos, (size_t)M), dQn = to_device(q_norm, 128), dKn = to_device(k_norm, 128);
  const DevBuf dCos = to_device(cos_t, (size_t)max_pos * 64), dSin = to_device(sin_t, (size_t)max_pos * 64);
  Guarded gQkv, gQ16;
  if (qkv) gQkv = Guarded(qkv, (size_t)M * N * 4);
  if (q16) gQ16 = Guarded(q16, n_q16 * 2);
  const Guarded gK(kcache, kv_bytes), gV(vcache, kv_bytes);
  RopeKvArgs rk{};
  rk.qkv = gQkv.as<float>(); rk.row_seq = dSeq.as<int>(); rk.row_pos = dPos.as<int>(); rk.q_norm = dQn.as<float>(); rk.k_norm = dKn.as<float>();
  rk.eps = eps; rk.cos_t = dCos.as<float>(); rk.sin_t = dSin.as<float>(); rk.kcache = gK.as<void>(); rk.vcache = gV.as<void>();
  rk.n_q = n_q; rk.n_kv = n_kv; rk.max_ctx = max_ctx; rk.q16 = gQ16.as<uint16_t>();
  if (fused) KCHK(launch_gemm256_qkrope(dX.as<uint16_t>(), lda, dW.as<uint16_t>(), M, K, dB.as<float>(), rk, nullptr));
  else KCHK(launch_qknorm_rope_kv(rk, M, kv_f32 != 0, nullptr));
  finish();
  if (qkv) gQkv.fetch(qkv, "qkv");
  if (q16) gQ16.fetch(q16, "q");
  gK.fetch(kcache, "K cache"); gV.fetch(vcache, "V cache");
  Q3A_CATCH(nullptr)
}

int32_t q3a_selftest_beam_topk(int32_t device, const float* logits, int32_t S, int32_t V, int32_t W, int32_t* out_ids, float* out_lp) {
  Q3A_TRY(nullptr)
  use_device(device);
  if (!logits || !out_ids || !out_lp || S < 1 || V < 1) fail("q3a_selftest_beam_topk: bad argument");
  const size_t nc = beam_topk_chunks(V), Sz = S;
  const DevBuf dLg = to_device(logits, Sz * V), dCv = room(Sz * nc * BEAM_MAX_W * 4), dCi = room(Sz * nc * BEAM_MAX_W * 4);
  const DevBuf dPm = room(Sz * nc * 4), dPs = room(Sz * nc * 4), dOi = room(Sz * BEAM_MAX_W * 4), dOl = room(Sz * BEAM_MAX_W * 4);
  BeamTopkArgs t{dLg.as<float>(), S, V, W, dCv.as<float>(), dCi.as<int>(), dPm.as<float>(), dPs.as<float>(), dOi.as<int>(), dOl.as<float>()};
  KCHK(launch_beam_topk(t, nullptr));
  finish();
  to_host(out_ids, dOi, Sz * W); to_host(out_lp, dOl, Sz * W);
  Q3A_CATCH(nullptr)
}

int32_t q3a_selftest_beam_advance(int32_t device, int32_t U, int32_t W, const int32_t* topk_ids, const float* topk_lp, const float* score_in,
                                  const uint8_t* finished_in, int32_t* parent_out, int32_t* token_out, float* score_out, uint8_t* finished_out) {
  Q3A_TRY(nullptr)
  use_device(device);
  if (!topk_ids || !topk_lp || !score_in || !finished_in || !parent_out || !token_out || !score_out || !finished_out || U < 1 || W < 1 || W > BEAM_MAX_W || U * W > 32)
    fail("q3a_selftest_beam_advance: bad argument");
  const size_t S = (size_t)U * W;
  const DevBuf dTi = to_device(topk_ids, S * W), dTl = to_device(topk_lp, S * W), dSc = to_device(score_in, S), dFi = to_device(finished_in, S);
  const DevBuf dPa = room(S * 4), dTo = room(S * 4), dSt = to_device(std::vector<int>(BEAM_ST_COUNT, 0));
  BeamAdvanceArgs a{};
  a.U = U; a.W = W; a.topk_ids = dTi.as<int>(); a.topk_lp = dTl.as<float>(); a.score = dSc.as<float>(); a.finished = dFi.as<uint8_t>();
  a.parent = dPa.as<int>(); a.token = dTo.as<int>(); a.state = dSt.as<int>(); a.eos0 = kEos0; a.eos1 = kEos1;
  KCHK(launch_beam_advance(a, nullptr));
  finish();
  to_host(parent_out, dPa, S); to_host(token_out, dTo, S); to_host(score_out, dSc, S); to_host(finished_out, dFi, S);
  Q3A_CATCH(nullptr)
}

int32_t q3a_selftest_kv_reorder(int32_t device, void* cache, int32_t elem_bytes, int32_t layers, int32_t S, int32_t n_kv, int32_t max_ctx,
                                const int32_t* lo, const int32_t* hi, const int32_t* parent) {
  Q3A_TRY(nullptr)
  use_device(device);
  if (!cache || !lo || !hi || !parent || layers < 1 || S < 1 || S > 32 || n_kv < 1 || max_ctx < 1 || (elem_bytes != 2 && elem_bytes != 4))
    fail("q3a_selftest_kv_reorder: bad argument");
  for (int s = 0; s < S; ++s) {  // bounds before anything runs: a copy stays inside the cache and inside one utterance's rows
    const int p = parent[s];
    if (p < 0 || p >= S) fail("q3a_selftest_kv_reorder: parent out of range");
    if (lo[s] < 0 || hi[s] >= max_ctx) fail("q3a_selftest_kv_reorder: rows outside the cache");
    if (p != s && (lo[p] != lo[s] || hi[p] != hi[s])) fail("q3a_selftest_kv_reorder: a parent must share its child's row range (a slot of the same utterance)");
  }
  const size_t half = (size_t)layers * S * n_kv * max_ctx * 128 * elem_bytes;  // K, then V
  const DevBuf dC = to_device((const uint8_t*)cache, 2 * half), dLo = to_device(lo, S), dHi = to_device(hi, S), dPar = to_device(parent, S);
  KvReorderArgs r{};
  r.kcache = dC.p; r.vcache = (uint8_t*)dC.p + half; r.elem_bytes = elem_bytes; r.layers = layers; r.S = S; r.n_kv = n_kv; r.max_ctx = max_ctx;
  r.parent = dPar.as<int>(); r.lo = dLo.as<int>(); r.hi = dHi.as<int>();
  KCHK(launch_kv_reorder(r, nullptr));
  finish();
  to_host((uint8_t*)cache, dC, 2 * half);
  Q3A_CATCH(nullptr)
}

uint32_t q3a_sample_word(uint64_t seed, uint32_t s, uint32_t t, uint32_t j) { return sample_word((uint32_t)seed, (uint32_t)(seed >> 32), s, t, j); }

// the sampled step's tail as the engine enqueues it: launch_sample, argmax_finalize on its partials, launch_sample_logprob
int32_t q3a_selftest_sample(int32_t device, const float* logits, int32_t S, int32_t V, float temperature, float min_p, uint64_t seed,
                            int32_t step, int32_t* out_ids, float* out_lp, float* out_z) {
  Q3A_TRY(nullptr)
  if (!logits || S < 1 || V < 1 || step < 0 || step > (1 << 20)) fail("q3a_selftest_sample: bad argument");
  if (!(temperature > 0.f) || !std::isfinite(temperature)) fail("q3a_selftest_sample: temperature must be finite and > 0");
  if (!(min_p >= 0.f && min_p <= 1.f)) fail("q3a_selftest_sample: min_p must lie in [0, 1]");
  use_device(device);
  const size_t Sz = S, nc = sample_chunks(V), stride = (size_t)step + 1;
  constexpr int H = 4;  // finalize embeds the chosen id: a token table of zeros, four columns wide
  uint32_t w[4];
  memcpy(&w[0], &temperature, 4); memcpy(&w[1], &min_p, 4);
  w[2] = (uint32_t)seed; w[3] = (uint32_t)(seed >> 32);
  const DevBuf dLg = to_device(logits, Sz * V), dPar = to_device(w, 4), dSc = to_device(std::vector<int>(Sz, step));
  const DevBuf dCm = room(Sz * nc * 4), dCs = room(Sz * nc * 4), dPv = room(Sz * nc * 4), dPi = room(Sz * nc * 4);
  const DevBuf dEmb = to_device(std::vector<uint16_t>((size_t)V * H, 0)), dX = room(Sz * H * 4), dTok = room(Sz * 4);
  const DevBuf dIds = to_device(std::vector<int>(Sz * stride, -1)), dLp = to_device(std::vector<float>(Sz * stride, 0.f));
  const DevBuf dPos = to_device(std::vector<int>(Sz, 0)), dDone = to_device(std::vector<uint8_t>(Sz, 0)), dZ = room(Sz * 4);
  SampleArgs sa{};
  sa.logits = dLg.as<float>(); sa.S = S; sa.V = V; sa.params = dPar.as<uint32_t>(); sa.step_count = dSc.as<int>();
  sa.chunk_max = dCm.as<float>(); sa.chunk_sum = dCs.as<float>();
  sa.part = ArgmaxPartials{dPv.as<float>(), dPi.as<int>(), nullptr, (int)nc};
  KCHK(launch_sample(sa, nullptr));
  FinalizeArgs f{};
  f.part = sa.part; f.n_part = (int)nc; f.V = V; f.advance = 1;
  f.c = bare_commit(S, dTok, dIds.as<int>(), (int)stride, nullptr, dSc, dPos, dDone, dEmb.as<uint16_t>(), H, dX.as<float>(), kEos0, kEos1);
  KCHK(launch_argmax_finalize(f, S, nullptr));
  SampleLogprobArgs sl{};
  sl.logits = sa.logits; sl.S = S; sl.V = V; sl.chunk_max = sa.chunk_max; sl.chunk_sum = sa.chunk_sum; sl.next_tok = f.c.next_tok;
  sl.step_count = f.c.step_count; sl.out_lp = dLp.as<float>(); sl.out_stride = (int)stride; sl.part = sa.part; sl.out_z = dZ.as<float>();
  KCHK(launch_sample_logprob(sl, nullptr));
  finish();
  const std::vector<int> ids = to_host<int>(dIds, Sz * stride);
  const std::vector<float> lp = to_host<float>(dLp, Sz * stride);
  for (size_t s = 0; s < Sz; ++s) {
    if (out_ids) out_ids[s] = ids[s * stride + step];
    if (out_lp) out_lp[s] = lp[s * stride + step];
  }
  if (out_z) to_host(out_z, dZ, Sz);
  Q3A_CATCH(nullptr)
}

// the same tail with q3a_set_sampling_filter on: launch_sample_filtered in the place of launch_sample.  It runs the stage TWICE on one
// table, as two steps of a decode do, and hands out the second run: the stage must leave its table as it found it.
int32_t q3a_selftest_sample_filter(int32_t device, const float* logits, int32_t S, int32_t V, float temperature, float min_p, int32_t top_k,
                                   float top_p, uint64_t seed, int32_t step, int32_t* out_ids, float* out_lp, float* out_z, float* out_thr,
                                   int32_t* out_kept) {
  Q3A_TRY(nullptr)
  if (!logits || S < 1 || V < 1 || step < 0 || step > (1 << 20)) fail("q3a_selftest_sample_filter: bad argument");
  if (!(temperature > 0.f) || !std::isfinite(temperature)) fail("q3a_selftest_sample_filter: temperature must be finite and > 0");
  if (!(min_p >= 0.f && min_p <= 1.f)) fail("q3a_selftest_sample_filter: min_p must lie in [0, 1]");
  if (top_k < 0) fail("q3a_selftest_sample_filter: top_k must be >= 0");
  if (!(top_p > 0.f && top_p <= 1.f)) fail("q3a_selftest_sample_filter: top_p must lie in (0, 1]");
  use_device(device);
  const size_t Sz = S, nc = sample_chunks(V), stride = (size_t)step + 1;
  constexpr int H = 4;
  uint32_t w[4], fw[4] = {(uint32_t)top_k, 0u, 0u, 0u};
  memcpy(&w[0], &temperature, 4); memcpy(&w[1], &min_p, 4); memcpy(&fw[1], &top_p, 4);
  w[2] = (uint32_t)seed; w[3] = (uint32_t)(seed >> 32);
  const DevBuf dLg = to_device(logits, Sz * V), dPar = to_device(w, 4), dFil = to_device(fw, 4);
  const DevBuf dCm = room(Sz * nc * 4), dCs = room(Sz * nc * 4), dPv = room(Sz * nc * 4), dPi = room(Sz * nc * 4);
  const DevBuf dHist = to_device(std::vector<uint32_t>(Sz * SAMPLE_BUCKETS * 3, 0u)), dSel = room(Sz * 8);
  const DevBuf dEmb = to_device(std::vector<uint16_t>((size_t)V * H, 0)), dX = room(Sz * H * 4), dTok = room(Sz * 4);
  const DevBuf dZ = room(Sz * 4);
  std::vector<int> ids;
  std::vector<float> lp;
  for (int run = 0; run < 2; ++run) {
    const DevBuf dSc = to_device(std::vector<int>(Sz, step)), dIds = to_device(std::vector<int>(Sz * stride, -1));
    const DevBuf dLp = to_device(std::vector<float>(Sz * stride, 0.f));
    const DevBuf dPos = to_device(std::vector<int>(Sz, 0)), dDone = to_device(std::vector<uint8_t>(Sz, 0));
    SampleArgs sa{};
    sa.logits = dLg.as<float>(); sa.S = S; sa.V = V; sa.params = dPar.as<uint32_t>(); sa.step_count = dSc.as<int>();
    sa.chunk_max = dCm.as<float>(); sa.chunk_sum = dCs.as<float>();
    sa.part = ArgmaxPartials{dPv.as<float>(), dPi.as<int>(), nullptr, (int)nc};
    SampleFilterArgs sf{};
    sf.filter = dFil.as<uint32_t>(); sf.hist_mass = dHist.as<unsigned long long>();
    sf.hist_cnt = reinterpret_cast<uint32_t*>(sf.hist_mass + Sz * SAMPLE_BUCKETS);
    sf.tau_sel = dSel.as<float>(); sf.kept = dSel.as<int>() + S;
    KCHK(launch_sample_filtered(sa, sf, nullptr));
    FinalizeArgs f{};
    f.part = sa.part; f.n_part = (int)nc; f.V = V; f.advance = 1;
    f.c = bare_commit(S, dTok, dIds.as<int>(), (int)stride, nullptr, dSc, dPos, dDone, dEmb.as<uint16_t>(), H, dX.as<float>(), kEos0, kEos1);
    KCHK(launch_argmax_finalize(f, S, nullptr));
    SampleLogprobArgs sl{};
    sl.logits = sa.logits; sl.S = S; sl.V = V; sl.chunk_max = sa.chunk_max; sl.chunk_sum = sa.chunk_sum; sl.next_tok = f.c.next_tok;
    sl.step_count = f.c.step_count; sl.out_lp = dLp.as<float>(); sl.out_stride = (int)stride; sl.part = sa.part; sl.out_z = dZ.as<float>();
    KCHK(launch_sample_logprob(sl, nullptr));
    finish();
    ids = to_host<int>(dIds, Sz * stride);
    lp = to_host<float>(dLp, Sz * stride);
  }
  for (size_t s = 0; s < Sz; ++s) {
    if (out_ids) out_ids[s] = ids[s * stride + step];
    if (out_lp) out_lp[s] = lp[s * stride + step];
  }
  if (out_z) to_host(out_z, dZ, Sz);
  const std::vector<float> sel = to_host<float>(dSel, Sz * 2);
  if (out_thr) memcpy(out_thr, sel.data(), Sz * 4);
  if (out_kept) memcpy(out_kept, sel.data() + Sz, Sz * 4);
  Q3A_CATCH(nullptr)
}

// a step's tail with q3a_set_repetition on, as the engine enqueues it without sampling: launch_repeat_apply on the stored rows, fresh
// argmax partials (with the log-sum channel) over the rewritten rows, argmax_finalize on those
int32_t q3a_selftest_repeat(int32_t device, const float* logits, int32_t S, int32_t V, const int32_t* hist, int32_t stride,
                            const int32_t* lens, float p, int32_t n, float* out_logits, int32_t* out_ids, float* out_lp) {
  Q3A_TRY(nullptr)
  if (!logits || !lens || S < 1 || V < 1 || stride < 0 || stride > (1 << 20) || (stride > 0 && !hist)) fail("q3a_selftest_repeat: bad argument");
  if (!std::isfinite(p) || !(p > 0.f)) fail("q3a_selftest_repeat: repetition_penalty must be finite and > 0");
  if (n < 0 || n > 32) fail("q3a_selftest_repeat: no_repeat_ngram_size must lie in [0, 32]");
  if (V > REPEAT_MAX_VOCAB) fail("q3a_selftest_repeat: the vocabulary exceeds the kernel's bitmap");
  const size_t Sz = S, pitch = (size_t)stride + 1;  // (one more column than any history: finalize writes the chosen id behind it)
  std::vector<int> ids(Sz * pitch, -1);
  for (size_t s = 0; s < Sz; ++s) {
    if (lens[s] < 0 || lens[s] > stride) fail("q3a_selftest_repeat: a history length outside [0, stride]");
    for (int i = 0; i < lens[s]; ++i) {
      const int id = hist[s * stride + i];
      if (id < 0 || id >= V) fail("q3a_selftest_repeat: a history id outside the vocabulary");
      ids[s * pitch + i] = id;
    }
  }
  use_device(device);
  constexpr int H = 4, NP = 128;  // finalize embeds the chosen id: a token table of zeros, four columns wide
  uint32_t w[4] = {0, (uint32_t)n, 0, 0};
  memcpy(&w[0], &p, 4);
  const DevBuf dLg = to_device(logits, Sz * V), dPar = to_device(w, 4), dSc = to_device(lens, Sz), dIds = to_device(ids);
  const DevBuf dPv = room(Sz * NP * 4), dPi = room(Sz * NP * 4), dPs = room(Sz * NP * 4);
  const DevBuf dEmb = to_device(std::vector<uint16_t>((size_t)V * H, 0)), dX = room(Sz * H * 4), dTok = room(Sz * 4);
  const DevBuf dLp = to_device(std::vector<float>(Sz * pitch, 0.f));
  const DevBuf dPos = to_device(std::vector<int>(Sz, 0)), dDone = to_device(std::vector<uint8_t>(Sz, 0));
  RepeatArgs ra{};
  ra.logits = dLg.as<float>(); ra.S = S; ra.V = V; ra.params = dPar.as<uint32_t>();
  ra.out_ids = dIds.as<int>(); ra.out_stride = (int)pitch; ra.step_count = dSc.as<int>();
  KCHK(launch_repeat_apply(ra, nullptr));
  const ArgmaxPartials part{dPv.as<float>(), dPi.as<int>(), dPs.as<float>(), NP};
  KCHK(launch_argmax_partials(ra.logits, V, S, part, NP, nullptr));
  FinalizeArgs f{};
  f.part = part; f.n_part = NP; f.V = V; f.advance = 1;
  f.c = bare_commit(S, dTok, dIds.as<int>(), (int)pitch, dLp.as<float>(), dSc, dPos, dDone, dEmb.as<uint16_t>(), H, dX.as<float>(), kEos0, kEos1);
  KCHK(launch_argmax_finalize(f, S, nullptr));
  finish();
  if (out_logits) to_host(out_logits, dLg, Sz * V);
  if (out_ids) to_host(out_ids, dTok, Sz);
  if (out_lp) {
    const std::vector<float> lp = to_host<float>(dLp, Sz * pitch);
    for (size_t s = 0; s < Sz; ++s) out_lp[s] = lp[s * pitch + lens[s]];
  }
  Q3A_CATCH(nullptr)
}

// the top log-probabilities of a step as the engine enqueues them (launch_top_logprobs on the stored rows), TWICE on the same scratch
// and into two histories: the second run sees whatever the first left in the candidates and the chunk pairs.  out_ids / out_lp: the
// whole [S][stride][TOP_LP_MAX] history of the second run (ids -1 and lp 0 where nothing was written); nonzero if the two differ.
int32_t q3a_selftest_top_logprobs(int32_t device, const float* logits, int32_t S, int32_t V, int32_t n, const int32_t* step_count,
                                  const uint8_t* done, int32_t stride, int32_t* out_ids, float* out_lp) {
  Q3A_TRY(nullptr)
  if (!logits || !step_count || !done || !out_ids || !out_lp || S < 1 || V < 1 || stride < 1 || stride > (1 << 16)) fail("q3a_selftest_top_logprobs: bad argument");
  if (n < 1 || n > TOP_LP_MAX || n > V) fail("q3a_selftest_top_logprobs: n must lie in [1, min(20, V)]");
  use_device(device);
  const size_t Sz = S, nc = (size_t)sample_chunks(V), hist = Sz * stride * TOP_LP_MAX;
  const DevBuf dLg = to_device(logits, Sz * V), dN = to_device(&n, 1), dSc = to_device(step_count, Sz), dDone = to_device(done, Sz);
  const DevBuf dCand = room(Sz * nc * TOP_LP_MAX * 8), dMax = room(Sz * nc * 4), dSum = room(Sz * nc * 4);
  // the scratch starts as all-ones words (NaN pairs, candidates above every real entry): what a run does not write itself shows
  HIPCHK(hipMemset(dCand.p, 0xFF, Sz * nc * TOP_LP_MAX * 8));
  HIPCHK(hipMemset(dMax.p, 0xFF, Sz * nc * 4));
  HIPCHK(hipMemset(dSum.p, 0xFF, Sz * nc * 4));
  std::vector<int> ids[2];
  std::vector<float> lp[2];
  for (int run = 0; run < 2; ++run) {
    const DevBuf dIds = to_device(std::vector<int>(hist, -1)), dLp = to_device(std::vector<float>(hist, 0.f));
    TopLpArgs a{};
    a.logits = dLg.as<float>(); a.S = S; a.V = V; a.n_dev = dN.as<int>(); a.step_count = dSc.as<int>(); a.done = dDone.as<uint8_t>();
    a.cand = dCand.as<unsigned long long>(); a.chunk_max = dMax.as<float>(); a.chunk_sum = dSum.as<float>();
    a.out_ids = dIds.as<int>(); a.out_lp = dLp.as<float>(); a.out_stride = stride;
    KCHK(launch_top_logprobs(a, nullptr));
    finish();
    ids[run] = to_host<int>(dIds, hist); lp[run] = to_host<float>(dLp, hist);
  }
  memcpy(out_ids, ids[1].data(), hist * 4);
  memcpy(out_lp, lp[1].data(), hist * 4);
  if (ids[0] != ids[1] || memcmp(lp[0].data(), lp[1].data(), hist * 4) != 0) fail("q3a_selftest_top_logprobs: the second run on the same scratch differs from the first");
  Q3A_CATCH(nullptr)
}

// a step's tail with q3a_set_sequence_bias on, as the engine enqueues it without repetition control and without sampling: the list laid
// out by the setter's own function, launch_seqbias_apply on the stored rows, fresh argmax partials (with the log-sum channel) over the
// rewritten rows, argmax_finalize on those
int32_t q3a_selftest_seqbias(int32_t device, const float* logits, int32_t S, int32_t V, const int32_t* hist, int32_t stride, const int32_t* lens,
                             const int32_t* seq_ids, const int32_t* seq_lens, const float* seq_bias, int32_t n, float* out_logits,
                             int32_t* out_ids, float* out_lp) {
  Q3A_TRY(nullptr)
  const char* what = "q3a_selftest_seqbias";
  if (!logits || !lens || S < 1 || V < 1 || stride < 0 || stride > (1 << 20) || (stride > 0 && !hist)) fail(std::string(what) + ": bad argument");
  const SeqBiasTable tb = seqbias_layout(what, seq_ids, seq_lens, seq_bias, n, V);
  const size_t Sz = S, pitch = (size_t)stride + 1;  // (one more column than any history: finalize writes the chosen id behind it)
  std::vector<int> ids(Sz * pitch, -1);
  for (size_t s = 0; s < Sz; ++s) {
    if (lens[s] < 0 || lens[s] > stride) fail(std::string(what) + ": a history length outside [0, stride]");
    for (int i = 0; i < lens[s]; ++i) {
      const int id = hist[s * stride + i];
      if (id < 0 || id >= V) fail(std::string(what) + ": a history id outside the vocabulary");
      ids[s * pitch + i] = id;
    }
  }
  use_device(device);
  constexpr int H = 4, NP = 128;  // finalize embeds the chosen id: a token table of zeros, four columns wide
  const DevBuf dLg = to_device(logits, Sz * V), dTab = to_device(tb.words), dSc = to_device(lens, Sz), dIds = to_device(ids);
  const DevBuf dPv = room(Sz * NP * 4), dPi = room(Sz * NP * 4), dPs = room(Sz * NP * 4);
  const DevBuf dEmb = to_device(std::vector<uint16_t>((size_t)V * H, 0)), dX = room(Sz * H * 4), dTok = room(Sz * 4);
  const DevBuf dLp = to_device(std::vector<float>(Sz * pitch, 0.f));
  const DevBuf dPos = to_device(std::vector<int>(Sz, 0)), dDone = to_device(std::vector<uint8_t>(Sz, 0));
  SeqBiasArgs sa{};
  sa.logits = dLg.as<float>(); sa.S = S; sa.V = V; seqbias_point(sa, dTab.p);
  sa.out_ids = dIds.as<int>(); sa.out_stride = (int)pitch; sa.step_count = dSc.as<int>();
  KCHK(launch_seqbias_apply(sa, nullptr));
  const ArgmaxPartials part{dPv.as<float>(), dPi.as<int>(), dPs.as<float>(), NP};
  KCHK(launch_argmax_partials(sa.logits, V, S, part, NP, nullptr));
  FinalizeArgs f{};
  f.part = part; f.n_part = NP; f.V = V; f.advance = 1;
  f.c = bare_commit(S, dTok, dIds.as<int>(), (int)pitch, dLp.as<float>(), dSc, dPos, dDone, dEmb.as<uint16_t>(), H, dX.as<float>(), kEos0, kEos1);
  KCHK(launch_argmax_finalize(f, S, nullptr));
  finish();
  if (out_logits) to_host(out_logits, dLg, Sz * V);
  if (out_ids) to_host(out_ids, dTok, Sz);
  if (out_lp) {
    const std::vector<float> lp = to_host<float>(dLp, Sz * pitch);
    for (size_t s = 0; s < Sz; ++s) out_lp[s] = lp[s * pitch + lens[s]];
  }
  Q3A_CATCH(nullptr)
}

// a step's tail under a row table (q3asr.h "row options"), in the order the engine enqueues it: the lists laid out by the setter's own
// function and the records by row_options_words, launch_seqbias_apply and launch_repeat_apply with a row stride of 4 where a row has
// them on, then the sampler (with the threshold stage if a row filters) or fresh argmax partials, argmax_finalize, the log-probability.
// With a filter the sampler's part runs TWICE on one table, as two steps of a decode do: the stage must leave its table as it found it.
int32_t q3a_selftest_row_options(int32_t device, const float* logits, int32_t S, int32_t V, const int32_t* hist, int32_t stride, const int32_t* lens,
                                 const q3a_row_options* rows, const int32_t* seq_ids, const int32_t* seq_lens, const float* seq_bias,
                                 const int32_t* list_lens, int32_t n_lists, float* out_logits, int32_t* out_ids, float* out_lp, float* out_z,
                                 float* out_thr, int32_t* out_kept) {
  Q3A_TRY(nullptr)
  const char* what = "q3a_selftest_row_options";
  if (!logits || !lens || !rows || S < 1 || V < 1 || stride < 0 || stride > (1 << 20) || (stride > 0 && !hist)) fail(std::string(what) + ": bad argument");
  const SeqBiasTable tb = seqbias_layout_lists(what, seq_ids, seq_lens, seq_bias, list_lens, n_lists, V);
  row_options_check(what, rows, S, n_lists, V);
  const size_t Sz = S, pitch = (size_t)stride + 1;  // (one more column than any history: finalize writes the chosen id behind it)
  std::vector<int> ids(Sz * pitch, -1);
  bool sample = false, filter = false, repeat = false, seqb = false;
  for (size_t s = 0; s < Sz; ++s) {
    if (lens[s] < 0 || lens[s] > stride) fail(std::string(what) + ": a history length outside [0, stride]");
    for (int i = 0; i < lens[s]; ++i) {
      const int id = hist[s * stride + i];
      if (id < 0 || id >= V) fail(std::string(what) + ": a history id outside the vocabulary");
      ids[s * pitch + i] = id;
    }
    const q3a_row_options& o = rows[s];
    sample |= o.temperature > 0.f;
    filter |= o.temperature > 0.f && (o.top_k != 0 || o.top_p != 1.f);
    repeat |= !(o.repetition_penalty == 1.f && o.no_repeat_ngram_size == 0);
    seqb |= o.sequence_list >= 0 && tb.list_entries[(size_t)o.sequence_list] > 0;
  }
  use_device(device);
  constexpr int H = 4, NP = 128;  // finalize embeds the chosen id: a token table of zeros, four columns wide
  const size_t nc = sample_chunks(V), np = sample ? nc : (size_t)NP;
  const DevBuf dLg = to_device(logits, Sz * V), dTab = to_device(tb.words), dRow = to_device(row_options_words(rows, S));
  const uint32_t* const rw = dRow.as<uint32_t>();  // regions sampling | filter | repetition | list, [S][4] words each
  const DevBuf dCm = room(Sz * nc * 4), dCs = room(Sz * nc * 4), dPv = room(Sz * np * 4), dPi = room(Sz * np * 4), dPs = room(Sz * np * 4);
  const DevBuf dHist = to_device(std::vector<uint32_t>(Sz * SAMPLE_BUCKETS * 3, 0u)), dSel = room(Sz * 8);
  const DevBuf dEmb = to_device(std::vector<uint16_t>((size_t)V * H, 0)), dX = room(Sz * H * 4), dTok = room(Sz * 4), dZ = room(Sz * 4);
  {  // the rewriting kernels run once: they work in place, and both read only the history in front of lens[s]
    const DevBuf dSc = to_device(lens, Sz), dIds = to_device(ids);
    if (seqb) {
      SeqBiasArgs sa{};
      sa.logits = dLg.as<float>(); sa.S = S; sa.V = V; seqbias_point(sa, dTab.p);
      sa.row_list = reinterpret_cast<const int*>(rw + 3 * Sz * 4); sa.row_stride = 4;
      sa.out_ids = dIds.as<int>(); sa.out_stride = (int)pitch; sa.step_count = dSc.as<int>();
      KCHK(launch_seqbias_apply(sa, nullptr));
    }
    if (repeat) {
      RepeatArgs ra{};
      ra.logits = dLg.as<float>(); ra.S = S; ra.V = V; ra.params = rw + 2 * Sz * 4; ra.row_stride = 4;
      ra.out_ids = dIds.as<int>(); ra.out_stride = (int)pitch; ra.step_count = dSc.as<int>();
      KCHK(launch_repeat_apply(ra, nullptr));
    }
    finish();
  }
  std::vector<int> tok;
  std::vector<float> lp;
  for (int run = 0; run < (filter ? 2 : 1); ++run) {
    const DevBuf dSc = to_device(lens, Sz), dIds = to_device(ids), dLp = to_device(std::vector<float>(Sz * pitch, 0.f));
    const DevBuf dPos = to_device(std::vector<int>(Sz, 0)), dDone = to_device(std::vector<uint8_t>(Sz, 0));
    FinalizeArgs f{};
    f.V = V; f.advance = 1;
    SampleArgs sa{};
    if (sample) {
      sa.logits = dLg.as<float>(); sa.S = S; sa.V = V; sa.params = rw; sa.row_stride = 4; sa.step_count = dSc.as<int>();
      sa.chunk_max = dCm.as<float>(); sa.chunk_sum = dCs.as<float>();
      sa.part = ArgmaxPartials{dPv.as<float>(), dPi.as<int>(), nullptr, (int)nc};
      if (filter) {
        SampleFilterArgs sf{};
        sf.filter = rw + Sz * 4; sf.row_stride = 4; sf.hist_mass = dHist.as<unsigned long long>();
        sf.hist_cnt = reinterpret_cast<uint32_t*>(sf.hist_mass + Sz * SAMPLE_BUCKETS);
        sf.tau_sel = dSel.as<float>(); sf.kept = dSel.as<int>() + S;
        KCHK(launch_sample_filtered(sa, sf, nullptr));
      } else {
        KCHK(launch_sample(sa, nullptr));
      }
      f.part = sa.part; f.n_part = (int)nc;
    } else {
      f.part = ArgmaxPartials{dPv.as<float>(), dPi.as<int>(), dPs.as<float>(), NP}; f.n_part = NP;
      KCHK(launch_argmax_partials(dLg.as<float>(), V, S, f.part, NP, nullptr));
    }
    f.c = bare_commit(S, dTok, dIds.as<int>(), (int)pitch, sample ? nullptr : dLp.as<float>(), dSc, dPos, dDone, dEmb.as<uint16_t>(), H, dX.as<float>(), kEos0, kEos1);
    KCHK(launch_argmax_finalize(f, S, nullptr));
    if (sample) {
      SampleLogprobArgs sl{};
      sl.logits = sa.logits; sl.S = S; sl.V = V; sl.chunk_max = sa.chunk_max; sl.chunk_sum = sa.chunk_sum; sl.next_tok = f.c.next_tok;
      sl.step_count = f.c.step_count; sl.out_lp = dLp.as<float>(); sl.out_stride = (int)pitch; sl.part = sa.part; sl.out_z = dZ.as<float>();
      KCHK(launch_sample_logprob(sl, nullptr));
    }
    finish();
    tok = to_host<int>(dTok, Sz);
    lp = to_host<float>(dLp, Sz * pitch);
  }
  if (out_logits) to_host(out_logits, dLg, Sz * V);
  for (size_t s = 0; s < Sz; ++s) {
    if (out_ids) out_ids[s] = tok[s];
    if (out_lp) out_lp[s] = lp[s * pitch + lens[s]];
  }
  if (out_z && sample) to_host(out_z, dZ, Sz);
  if (filter) {
    const std::vector<float> sel = to_host<float>(dSel, Sz * 2);
    if (out_thr) memcpy(out_thr, sel.data(), Sz * 4);
    if (out_kept) memcpy(out_kept, sel.data() + Sz, Sz * 4);
  }
  Q3A_CATCH(nullptr)
}

int32_t q3a_selftest_gemv_launch(int32_t device, int32_t pruned, const uint16_t* w, int32_t N, int32_t K, const float* x, const float* rms_w, float eps,
                                 const float* bias, int32_t mode, const float* resid, const float* attn_pm, const float* attn_pl, const float* attn_po,
                                 int32_t attn_nsplit, int32_t attn_heads, float* out, int32_t* out_state) {
  Q3A_TRY(nullptr)
  const char* what = "q3a_selftest_gemv_launch";
  // every index the launches will form is checked here: a refusal, never an access outside a buffer
  if (!w || N < 1 || K < 8 || K % 8 != 0 || K > 6144 || mode < 0 || mode > 3 || (pruned != 0 && pruned != 1)) fail(std::string(what) + ": bad argument");
  const bool attn = attn_po != nullptr;
  if (attn ? (x || rms_w || !attn_pm || !attn_pl || attn_nsplit < 1 || attn_heads < 1 || K != attn_heads * 128 ||
              (long)attn_heads * attn_nsplit > GEMV_ATTN_MAX_TABLE) : (!x || attn_pm || attn_pl))
    fail(std::string(what) + ": x alone, or the three partial arrays with K = heads * 128 alone");
  if (mode == 2 && N % 32 != 0) fail(std::string(what) + ": GLU needs N % 32 == 0");
  if ((mode == 1) != (resid != nullptr)) fail(std::string(what) + ": the residual goes with mode 1");
  if (mode == 3 ? (!rms_w || !out_state) : (!out || pruned)) fail(std::string(what) + ": mode 3 needs the norm weight and out_state, the other modes out");
  if (pruned && out) fail(std::string(what) + ": the pruned argmax stores no logits");
  use_device(device);
  const size_t n_out = mode == 2 ? (size_t)N / 2 : (size_t)N;
  const DevBuf dW = to_device(w, (size_t)N * K);
  DevBuf dX, dG, dB, dR, dPm, dPl, dPo;
  // x and the norm weight go on past K with NaN, to beyond the longest K of any form (checked above): a read past K that the
  // kernel does not void shows in the output
  auto padded = [&](const float* src) {
    std::vector<float> v(6144 + 8, NAN);
    memcpy(v.data(), src, (size_t)K * 4);
    return to_device(v);
  };
  if (x) dX = padded(x);
  if (rms_w) dG = padded(rms_w);
  if (bias) dB = to_device(bias, (size_t)N);
  if (resid) dR = to_device(resid, (size_t)N);
  if (attn) {
    // the kernels read a head's statistics 16 bytes at a time, past the last head's own into the allocation's padding: NaN there
    const size_t ns = (size_t)attn_heads * attn_nsplit;
    std::vector<float> pm(ns + 8, NAN), pl(ns + 8, NAN);
    memcpy(pm.data(), attn_pm, ns * 4); memcpy(pl.data(), attn_pl, ns * 4);
    dPm = to_device(pm); dPl = to_device(pl); dPo = to_device(attn_po, ns * 128);
  }
  Guarded dO;
  if (out) dO = Guarded(out, n_out * 4);
  GemvArgs g{};
  g.x = dX.as<float>(); g.ldx = K; g.rms_w = dG.as<float>(); g.eps = eps; g.W = dW.as<uint16_t>(); g.N = N; g.K = K; g.bias = dB.as<float>();
  g.mode = mode; g.out = dO.as<float>(); g.ldo = (int)n_out; g.resid = dR.as<float>();
  g.attn_pm = dPm.as<float>(); g.attn_pl = dPl.as<float>(); g.attn_po = dPo.as<float>(); g.attn_nsplit = attn_nsplit; g.attn_heads = attn_heads;
  g.attn_fast_exp = 0; g.fast_math = 0;  // the precise arithmetic: only fp32 rounding enters
  if (mode != 3) {
    KCHK(launch_gemv(g, 1, nullptr));
    finish();
    dO.fetch(out, "output");
  } else {
    int n_part = gemv_blocks(g);
    const DevBuf dPv = room((size_t)n_part * 4), dPi = room((size_t)n_part * 4);
    g.part = ArgmaxPartials{dPv.as<float>(), dPi.as<int>(), nullptr, n_part};
    DevBuf dQ, dQs, dLo, dHi;
    if (pruned) {
      LmHeadPruneArgs pa{};
      pa.g = g; pa.qcols = lm_head_q_cols(K); pa.logit_bias = bias ? 1 : 0;
      if (pa.qcols == 0) fail(std::string(what) + ": hidden size beyond the pruned argmax");
      const size_t nb4 = ((size_t)lm_head_prune_blocks(g) + 3) / 4 * 4;
      dQ = room((size_t)N * pa.qcols); dQs = room((size_t)N * 16); dLo = room(nb4 * 4); dHi = room(nb4 * 4);
      pa.Wq = dQ.as<int8_t>(); pa.qs = dQs.as<float>(); pa.blk_lo = dLo.as<float>(); pa.blk_hi = dHi.as<float>();
      KCHK(lm_head_prune_check(pa));
      KCHK(launch_lm_head_quantize(g.W, N, K, dQ.as<int8_t>(), dQs.as<float>(), nullptr));
      n_part = lm_head_rescore_groups(g, 0);
      KCHK(launch_lm_head_approx(pa, nullptr));
      KCHK(launch_lm_head_rescore(pa, n_part, nullptr));
    } else {
      KCHK(launch_gemv(g, 1, nullptr));
    }
    // finalize as the greedy loop runs it, from a state in which every counter it touches is visible: step 2 of 4, position 5
    constexpr int STRIDE = 4, STEP = 2, POS = 5;
    const DevBuf dTok = to_device(std::vector<int>(1, -1)), dIds = to_device(std::vector<int>(STRIDE, -1)), dSc = to_device(std::vector<int>(1, STEP));
    const DevBuf dPos = to_device(std::vector<int>(1, POS)), dDone = to_device(std::vector<uint8_t>(1, 0)), dXn = room((size_t)K * 4);
    FinalizeArgs f{};
    f.part = g.part; f.n_part = n_part; f.V = N; f.advance = 1;
    f.c = bare_commit(1, dTok, dIds.as<int>(), STRIDE, nullptr, dSc, dPos, dDone, g.W, K, dXn.as<float>(), -1, -1);  // (the embedding row of the chosen id: a row of w)
    KCHK(launch_argmax_finalize(f, 1, nullptr));
    finish();
    if (out) dO.fetch(out, "output");
    const std::vector<int> ids = to_host<int>(dIds, STRIDE);
    out_state[0] = to_host<int>(dTok, 1)[0]; out_state[1] = ids[STEP]; out_state[2] = to_host<int>(dSc, 1)[0]; out_state[3] = to_host<int>(dPos, 1)[0];
  }
  Q3A_CATCH(nullptr)
}

int32_t q3a_selftest_oproj_head_launch(int32_t device, const uint16_t* w, int32_t N, int32_t K, const float* bias, const float* attn_pm, const float* attn_pl,
                                       const float* attn_po, int32_t attn_nsplit, int32_t attn_heads, int32_t n_parts, float* y_part) {
  Q3A_TRY(nullptr)
  const char* what = "q3a_selftest_oproj_head_launch";
  // every index the launch will form is checked here or by the launcher's own check, in front of any copy to the device
  if (!w || !attn_pm || !attn_pl || !attn_po || !y_part || N < 1 || attn_heads < 1 || attn_nsplit < 1 || n_parts < 1 || K != attn_heads * 128)
    fail(std::string(what) + ": bad argument");
  OprojHeadArgs a{};
  a.pm = attn_pm; a.pl = attn_pl; a.po = attn_po;  // (host pointers: only looked at for null by the check)
  a.nsplit = attn_nsplit; a.W = w; a.N = N; a.K = K; a.n_parts = n_parts; a.y_part = y_part;
  KCHK(oproj_head_check(a));
  use_device(device);
  const size_t ns = (size_t)attn_heads * attn_nsplit;
  const DevBuf dW = to_device(w, (size_t)N * K), dPm = to_device(attn_pm, ns), dPl = to_device(attn_pl, ns), dPo = to_device(attn_po, ns * 128);
  DevBuf dB;
  if (bias) dB = to_device(bias, (size_t)N);
  const Guarded dY(y_part, (size_t)n_parts * N * 4);
  a.pm = dPm.as<float>(); a.pl = dPl.as<float>(); a.po = dPo.as<float>(); a.W = dW.as<uint16_t>(); a.bias = dB.as<float>(); a.y_part = dY.as<float>();
  KCHK(launch_oproj_head(a, nullptr));
  finish();
  dY.fetch(y_part, "partial vectors");
  Q3A_CATCH(nullptr)
}

int32_t q3a_selftest_gemv_parts_launch(int32_t device, const uint16_t* w, int32_t N, int32_t K, const float* x, const float* rms_w, float eps,
                                       const float* bias, const float* x_parts, int32_t n_parts, float* out, float* x_out) {
  Q3A_TRY(nullptr)
  const char* what = "q3a_selftest_gemv_parts_launch";
  if (!w || !x || !rms_w || !x_parts || !out || !x_out || N < 32 || N % 32 != 0 || K < 8 || K % 8 != 0 || K > 1024 || n_parts < 1 || n_parts > GEMV_X_PARTS_MAX)
    fail(std::string(what) + ": bad argument");
  use_device(device);
  const DevBuf dW = to_device(w, (size_t)N * K), dP = to_device(x_parts, (size_t)n_parts * K);
  // x and the norm weight go on past K with NaN, as in q3a_selftest_gemv_launch (the partial vectors are rows of exactly K floats: a
  // read past the last one's end would leave the allocation, so the kernel's column clamp is what the K = 1016 case checks there)
  auto padded = [&](const float* src) {
    std::vector<float> v(1024 + 8, NAN);
    memcpy(v.data(), src, (size_t)K * 4);
    return to_device(v);
  };
  const DevBuf dX = padded(x), dG = padded(rms_w);
  DevBuf dB;
  if (bias) dB = to_device(bias, (size_t)N);
  const Guarded dO(out, (size_t)N / 2 * 4), dXo(x_out, (size_t)K * 4);
  GemvArgs g{};
  g.x = dX.as<float>(); g.ldx = K; g.rms_w = dG.as<float>(); g.eps = eps; g.W = dW.as<uint16_t>(); g.N = N; g.K = K; g.bias = dB.as<float>();
  g.mode = 2; g.out = dO.as<float>(); g.ldo = N / 2; g.fast_math = 0;
  g.x_parts = dP.as<float>(); g.x_nparts = n_parts; g.x_out = dXo.as<float>();
  KCHK(launch_gemv(g, 1, nullptr));
  finish();
  dO.fetch(out, "output"); dXo.fetch(x_out, "summed x");
  Q3A_CATCH(nullptr)
}

int32_t q3a_selftest_decode_attn_launch(int32_t device, int32_t kv_f32, const float* qkv, int32_t pos, const float* q_norm, const float* k_norm, float eps,
                                        const float* rope_cur, void* kcache, void* vcache, int32_t n_q, int32_t n_kv, int32_t max_ctx, int32_t nsplit,
                                        float scale_div, float* pm, float* pl, float* po) {
  return q3a_selftest_decode_attn_split_launch(device, kv_f32, 0, qkv, pos, q_norm, k_norm, eps, rope_cur, kcache, vcache, n_q, n_kv, max_ctx, nsplit,
                                               scale_div, pm, pl, po);
}

int32_t q3a_selftest_decode_attn_split_launch(int32_t device, int32_t kv_f32, int32_t keys_per_split, const float* qkv, int32_t pos, const float* q_norm,
                                              const float* k_norm, float eps, const float* rope_cur, void* kcache, void* vcache, int32_t n_q, int32_t n_kv,
                                              int32_t max_ctx, int32_t nsplit, float scale_div, float* pm, float* pl, float* po) {
  Q3A_TRY(nullptr)
  const char* what = "q3a_selftest_decode_attn_launch";
  if (!qkv || !q_norm || !k_norm || !rope_cur || !kcache || !vcache || !pm || !pl || !po || n_q < 1 || n_kv < 1 || n_q % n_kv != 0 || max_ctx < 1 ||
      nsplit < 1 || !(scale_div > 0.f))
    fail(std::string(what) + ": bad argument");
  if (keys_per_split != 0 && keys_per_split != 32 && keys_per_split != 64 && keys_per_split != 128) fail(std::string(what) + ": 32, 64 or 128 keys per split (0: the default)");
  const int keys = keys_per_split ? keys_per_split : dattn_keys_per_split(kv_f32 != 0);
  if (pos < 0 || pos >= max_ctx || pos >= nsplit * keys) fail(std::string(what) + ": pos outside the cache or beyond the last split");
  use_device(device);
  const size_t eb = kv_f32 ? 4 : 2, n_cache = (size_t)n_kv * max_ctx * 128, ns = (size_t)n_q * nsplit;
  const DevBuf dQkv = to_device(qkv, (size_t)(n_q + 2 * n_kv) * 128), dQn = to_device(q_norm, 128), dKn = to_device(k_norm, 128);
  const DevBuf dRope = to_device(rope_cur, 128), dPos = to_device(std::vector<int>(1, pos));
  const Guarded dK(kcache, n_cache * eb), dV(vcache, n_cache * eb), dPm(pm, ns * 4), dPl(pl, ns * 4), dPo(po, ns * 128 * 4);
  DecodeAttnArgs a{};
  a.qkv = dQkv.as<float>(); a.pos = dPos.as<int>(); a.q_norm = dQn.as<float>(); a.k_norm = dKn.as<float>(); a.eps = eps; a.rope_cur = dRope.as<float>();
  a.kcache = dK.as<void>(); a.vcache = dV.as<void>(); a.pm = dPm.as<float>(); a.pl = dPl.as<float>(); a.po = dPo.as<float>();
  a.nsplit = nsplit; a.keys_per_split = keys_per_split; a.n_q = n_q; a.n_kv = n_kv; a.max_ctx = max_ctx; a.scale_div = scale_div;
  KCHK(launch_decode_attn(a, 1, kv_f32 != 0, nullptr));
  finish();
  dK.fetch(kcache, "key cache"); dV.fetch(vcache, "value cache"); dPm.fetch(pm, "split maxima"); dPl.fetch(pl, "split sums"); dPo.fetch(po, "split outputs");
  Q3A_CATCH(nullptr)
}

int32_t q3a_selftest_skinny_launch(int32_t device, const uint16_t* w, int32_t N, int32_t K, int32_t S, const float* x, int32_t ldx, const float* rms_w,
                                   const uint16_t* x16, int32_t x16_frag, const uint16_t* xw16f, const float* ss_parts, int32_t ss_nparts, float eps,
                                   const float* bias, int32_t mode, const float* resid, float* out, uint16_t* out16, int32_t out16_frag, int32_t ldo,
                                   const float* next_w, uint16_t* next_xw16f, float* next_ss, int32_t flags, int32_t glu_hp3, int32_t n_cu,
                                   int32_t* form) {
  Q3A_TRY(nullptr)
  const char* what = "q3a_selftest_skinny_launch";
  const bool split = flags & 1, fast = flags & 2, qsplit = flags & 4, inplace = flags & 8;
  // every index the launch will form is checked here or by launch_skinny's own check, in front of any copy to the device
  if (!w || !form || (flags & ~15) || N < 1 || K < 32 || K % 32 != 0 || K > 6144 || S < 1 || S > 32 || mode < 0 || mode > 2 || glu_hp3 < 0 || glu_hp3 > 2 || n_cu < 0)
    fail(std::string(what) + ": bad argument");
  if ((x != nullptr) + (x16 != nullptr) + (xw16f != nullptr) != 1) fail(std::string(what) + ": exactly one of x, x16 and xw16f");
  if (rms_w && !x) fail(std::string(what) + ": the fused norm takes fp32 x");
  if (xw16f && (!ss_parts || ss_nparts < 1 || ss_nparts > 4096)) fail(std::string(what) + ": xw16f needs ss_parts [ss_nparts][32]");
  if ((x || (x16 && !x16_frag)) && (ldx < K || ldx % 8 != 0)) fail(std::string(what) + ": ldx below K or no multiple of 8");
  if (mode == 2 && N % 32 != 0) fail(std::string(what) + ": GLU needs N % 32 == 0");
  const int cols = mode == 2 ? N / 2 : N;
  if ((out != nullptr) == (out16 != nullptr) || (out16 && mode != 2) || ldo < cols) fail(std::string(what) + ": one of out / out16 (GLU only) with ldo >= its columns");
  if (inplace ? (mode != 1 || resid || !out) : ((mode == 1) != (resid != nullptr))) fail(std::string(what) + ": the residual goes with mode 1 (in place: it is `out`)");
  if (next_w && (mode != 1 || !next_xw16f || !next_ss)) fail(std::string(what) + ": next_w needs mode 1, next_xw16f and next_ss");
  if (qsplit && (split || mode != 1 || !x16 || !x16_frag || N % 64 != 0 || (K / 32) % 8 != 0)) fail(std::string(what) + ": quarter workgroups need mode 1, fragment-order x16, N % 64 == 0, K % 256 == 0");
  use_device(device);
  KCHK(skinny_init());
  const size_t Sz = S, frag_x = (size_t)32 * K, frag_cols = (size_t)32 * ((cols + 31) / 32 * 32);
  const DevBuf dW = to_device(w, (size_t)N * K);
  // fp32 x and the norm weight go on past their end with NaN, as in q3a_selftest_gemv_launch
  auto padded = [&](const float* src, size_t n) {
    std::vector<float> v(n + 6144 + 8, NAN);
    memcpy(v.data(), src, n * 4);
    return to_device(v);
  };
  DevBuf dX, dG, dX16, dXw, dSs, dB, dR, dNw;
  if (x) dX = padded(x, Sz * ldx);
  if (rms_w) dG = padded(rms_w, (size_t)K);
  if (x16) dX16 = to_device(x16, x16_frag ? frag_x : Sz * ldx);
  if (xw16f) { dXw = to_device(xw16f, frag_x); dSs = to_device(ss_parts, (size_t)ss_nparts * 32); }
  if (bias) dB = to_device(bias, (size_t)N);
  if (resid) dR = to_device(resid, Sz * ldo);
  if (next_w) dNw = to_device(next_w, (size_t)N);
  Guarded gO, gO16, gNx, gNs;
  // (row-major outputs have 32 rows whatever S is: a store to a row >= S lands in the caller's sentinel, where it is seen)
  if (out) gO = Guarded(out, (size_t)32 * ldo * 4);
  if (out16) gO16 = Guarded(out16, (out16_frag ? frag_cols : (size_t)32 * ldo) * 2);
  const size_t ss_rows = qsplit ? (size_t)N / 8 : ((size_t)N + 15) / 16;
  if (next_w) { gNx = Guarded(next_xw16f, frag_cols * 2); gNs = Guarded(next_ss, ss_rows * 32 * 4); }
  SkinnyArgs a{};
  a.x = dX.as<float>(); a.ldx = (x || (x16 && !x16_frag)) ? ldx : K; a.S = S; a.x16 = dX16.as<uint16_t>(); a.x16_frag = x16_frag ? 1 : 0; a.out16_frag = out16_frag ? 1 : 0;
  a.rms_w = dG.as<float>(); a.eps = eps; a.W = dW.as<uint16_t>(); a.N = N; a.K = K; a.bias = dB.as<float>(); a.mode = mode;
  a.out = gO.as<float>(); a.ldo = ldo; a.out16 = gO16.as<uint16_t>(); a.resid = inplace ? gO.as<float>() : dR.as<float>();
  a.xw16f = dXw.as<uint16_t>(); a.ss_parts = dSs.as<float>(); a.ss_nparts = xw16f ? ss_nparts : 0;
  a.next_w = dNw.as<float>(); a.next_xw16f = gNx.as<uint16_t>(); a.next_ss = gNs.as<float>();
  a.qsplit = qsplit ? 1 : 0; a.glu_hp3 = glu_hp3; a.n_cu = n_cu; a.fast_math = fast ? 1 : 0;
  KCHK(launch_skinny(a, split, nullptr));
  const SkinnyForm f = skinny_last_form();
  finish();
  const int rep[11] = {f.split, f.tiles, f.sh, f.xmode, f.unr, f.wlds, f.qs, f.palias, f.hp, f.grid, f.dyn_lds};
  memcpy(form, rep, sizeof rep);
  if (out) gO.fetch(out, "output");
  if (out16) gO16.fetch(out16, "bf16 output");
  if (next_w) { gNx.fetch(next_xw16f, "next_xw16f"); gNs.fetch(next_ss, "next_ss"); }
  Q3A_CATCH(nullptr)
}

int32_t q3a_selftest_batched_attn_launch(int32_t device, int32_t kv_f32, int32_t split_path, int32_t S, const float* qkv, const int32_t* pos,
                                         const float* q_norm, const float* k_norm, float eps, const float* rope_cur, void* kcache, void* vcache,
                                         int32_t n_q, int32_t n_kv, int32_t max_ctx, float scale_div, int32_t trim_prologue, int32_t nsplit,
                                         int32_t keys_per_split, int32_t out_form, void* out, float* pm, float* pl, float* po) {
  Q3A_TRY(nullptr)
  const char* what = "q3a_selftest_batched_attn_launch";
  if (!qkv || !pos || !q_norm || !k_norm || !rope_cur || !kcache || !vcache || !out || S < 1 || S > 64 || n_q < 1 || n_kv < 1 || n_q % n_kv != 0 ||
      max_ctx < 1 || !(scale_div > 0.f) || out_form < 0 || out_form > 2 || (trim_prologue != 0 && trim_prologue != 1))
    fail(std::string(what) + ": bad argument");
  int keys = 0;
  if (split_path) {
    if (!pm || !pl || !po || nsplit < 1) fail(std::string(what) + ": the split path needs nsplit and the three partial arrays");
    if (keys_per_split != 0 && keys_per_split != 32 && keys_per_split != 64 && keys_per_split != 128) fail(std::string(what) + ": 32, 64 or 128 keys per split (0: the default)");
    keys = keys_per_split ? keys_per_split : dattn_keys_per_split(kv_f32 != 0);
  } else if (pm || pl || po) fail(std::string(what) + ": the batched kernel writes no partials");
  for (int s = 0; s < S; ++s)
    if (pos[s] < 0 || pos[s] >= max_ctx || (split_path && pos[s] >= nsplit * keys)) fail(std::string(what) + ": a pos outside the cache or beyond the last split");
  use_device(device);
  const size_t Sz = S, eb = kv_f32 ? 4 : 2, n_cache = Sz * n_kv * max_ctx * 128, ns = Sz * n_q * (split_path ? nsplit : 0), hd = (size_t)n_q * 128;
  // (fragment order holds 32 sequences; with more the launcher refuses before anything runs, and the buffer is sized for the row-major form)
  const size_t n_out = out_form == 2 && S <= 32 ? 32 * hd : Sz * hd;
  const DevBuf dQkv = to_device(qkv, Sz * (n_q + 2 * n_kv) * 128), dQn = to_device(q_norm, 128), dKn = to_device(k_norm, 128);
  const DevBuf dRope = to_device(rope_cur, Sz * 128), dPos = to_device(pos, Sz);
  const Guarded dK(kcache, n_cache * eb), dV(vcache, n_cache * eb), dO(out, n_out * (out_form ? 2 : 4));
  Guarded dPm, dPl, dPo;
  if (split_path) { dPm = Guarded(pm, ns * 4); dPl = Guarded(pl, ns * 4); dPo = Guarded(po, ns * 128 * 4); }
  DecodeAttnArgs a{};
  a.qkv = dQkv.as<float>(); a.pos = dPos.as<int>(); a.q_norm = dQn.as<float>(); a.k_norm = dKn.as<float>(); a.eps = eps; a.rope_cur = dRope.as<float>();
  a.kcache = dK.as<void>(); a.vcache = dV.as<void>(); a.n_q = n_q; a.n_kv = n_kv; a.max_ctx = max_ctx; a.scale_div = scale_div;
  if (split_path) {
    a.pm = dPm.as<float>(); a.pl = dPl.as<float>(); a.po = dPo.as<float>(); a.nsplit = nsplit; a.keys_per_split = keys_per_split;
    if (out_form == 2 && S > 32) fail("attn_combine: fragment order holds at most 32 sequences");  // (its launcher's own refusal, in front of the first launch)
    KCHK(launch_decode_attn(a, S, kv_f32 != 0, nullptr));
    KCHK(launch_attn_combine(a.pm, a.pl, a.po, nsplit, S, n_q, out_form ? nullptr : dO.as<float>(), nullptr, out_form ? dO.as<uint16_t>() : nullptr, out_form == 2));
  } else {
    if (out_form) { a.out16 = dO.as<uint16_t>(); a.out_frag = out_form == 2; } else a.out = dO.as<float>();
    a.trim_prologue = trim_prologue;
    KCHK(launch_decode_attn_batched(a, S, kv_f32 != 0, nullptr));
  }
  finish();
  dK.fetch(kcache, "key cache"); dV.fetch(vcache, "value cache"); dO.fetch(out, "context");
  if (split_path) { dPm.fetch(pm, "split maxima"); dPl.fetch(pl, "split sums"); dPo.fetch(po, "split outputs"); }
  Q3A_CATCH(nullptr)
}

int32_t q3a_selftest_seg_attn_launch(int32_t device, int32_t launcher, int32_t kv_f32, int32_t group, const int32_t* seg_q_row0, const int32_t* seg_len,
                                     const int64_t* seg_kv_off, int32_t n_segs, int32_t max_len, const float* q, const uint16_t* q16, int32_t q_rows,
                                     int32_t q_rs, const void* k, const void* v, int64_t kv_elems, int64_t k_base, int64_t v_base, int64_t kv_hs,
                                     int32_t kv_rs, int32_t n_kv_heads, float scale_div, float* o, uint16_t* o16, int32_t o_rows, int32_t o_rs,
                                     int32_t* form) {
  Q3A_TRY(nullptr)
  const char* what = "q3a_selftest_seg_attn_launch";
  const bool mfma = launcher >= 2, enc = launcher == 0 || launcher == 2;
  if (launcher < 0 || launcher > 3 || !seg_q_row0 || !seg_len || !seg_kv_off || !k || !v || !form || n_segs < 1 || n_segs > 4096 || max_len < 1 ||
      q_rows < 1 || q_rs < 1 || o_rows < 1 || o_rs < 1 || kv_elems < 1 || k_base < 0 || v_base < 0 || kv_hs < 0 || kv_rs < 1 || n_kv_heads < 1 ||
      n_kv_heads > 64 || group < 1 || group > 8 || !(scale_div > 0.f))
    fail(std::string(what) + ": bad argument");
  if (enc && group != 1) fail(std::string(what) + ": the encoder form has one query head per K/V head");
  if ((o != nullptr) == (o16 != nullptr) || (!mfma && (o16 || q16 || !q)) || (!q && !q16)) fail(std::string(what) + ": one of o / o16 and q and / or q16 (bf16: the MFMA launchers only)");
  // the K/V element type each launcher reads: fp32 windows (bf16 with q16) in the encoder, the cache's type in the prefill
  if ((kv_f32 != 0) != (launcher == 0 || (launcher == 1 && kv_f32) || (launcher == 2 && !q16))) fail(std::string(what) + ": kv_f32 does not name what this launcher reads");
  // every index the launch will form is checked here or by the launcher's own check: a refusal, never an access outside a buffer
  const int HD = enc ? 64 : 128, al = kv_f32 ? 4 : 8;
  const long cols = (long)n_kv_heads * group * HD;
  if (cols > q_rs || cols > o_rs || HD > kv_rs) fail(std::string(what) + ": a row stride below the row");
  if (k_base % al || v_base % al || kv_hs % al || (launcher != 2 && kv_rs % al)) fail(std::string(what) + ": K/V offsets and strides in whole 16-byte groups");
  std::vector<AttnSeg> segs(n_segs);
  int longest = 0;
  for (int i = 0; i < n_segs; ++i) {
    const int r0 = seg_q_row0[i], len = seg_len[i];
    const int64_t off = seg_kv_off[i];
    if (r0 < 0 || len < 1 || (long)r0 + len > q_rows || (long)r0 + len > o_rows) fail(std::string(what) + ": a segment's rows lie outside q or the output");
    if (off < 0 || off % al || std::max(k_base, v_base) + off + (int64_t)(n_kv_heads - 1) * kv_hs + (int64_t)(len - 1) * kv_rs + HD > kv_elems)
      fail(std::string(what) + ": a segment's keys lie outside K / V");
    segs[i] = AttnSeg{r0, len, off};
    longest = std::max(longest, len);
  }
  if (max_len < longest || max_len > (1 << 20)) fail(std::string(what) + ": max_len below the longest segment");
  use_device(device);
  const size_t eb = kv_f32 ? 4 : 2, n_q = (size_t)q_rows * q_rs, n_o = (size_t)o_rows * o_rs;
  const DevBuf dK = to_device((const uint8_t*)k, (size_t)kv_elems * eb), dV = to_device((const uint8_t*)v, (size_t)kv_elems * eb), dSeg = to_device(segs);
  DevBuf dQ, dQ16;
  if (q) dQ = to_device(q, n_q);
  if (q16) dQ16 = to_device(q16, n_q);
  const Guarded dO(o ? (const void*)o : (const void*)o16, n_o * (o ? 4 : 2));
  AttnArgs a{};
  a.q = dQ.as<float>(); a.q_rs = q_rs; a.q16 = dQ16.as<uint16_t>();
  a.k = static_cast<const uint8_t*>(dK.p) + k_base * eb; a.v = static_cast<const uint8_t*>(dV.p) + v_base * eb; a.kv_hs = kv_hs; a.kv_rs = kv_rs;
  if (o) a.o = dO.as<float>(); else a.o16 = dO.as<uint16_t>();
  a.o_rs = o_rs; a.segs = dSeg.as<AttnSeg>(); a.n_segs = n_segs; a.max_len = max_len; a.n_kv_heads = n_kv_heads; a.scale_div = scale_div;
  switch (launcher) {
    case 0: KCHK(launch_attn_enc(a, nullptr)); break;
    case 1: KCHK(launch_attn_prefill(a, group, kv_f32 != 0, nullptr)); break;
    case 2: KCHK(launch_fattn_enc(a, nullptr)); break;
    default: KCHK(launch_fattn_prefill(a, group, nullptr)); break;
  }
  int rep[12] = {0};
  if (mfma) {
    const FattnForm f = fattn_last_form();
    const int r[12] = {1, f.dma, f.hd, f.group, f.causal, f.kv_f32, f.ksplit, f.ns, 0, f.grid_x, f.grid_y, f.grid_z};
    memcpy(rep, r, sizeof rep);
  } else {
    const AttnForm f = attn_last_form();
    const int r[12] = {0, 0, f.hd, f.group, f.causal, f.kv_f32, 1, 0, f.qpw, f.grid_x, f.grid_y, f.grid_z};
    memcpy(rep, r, sizeof rep);
  }
  finish();
  memcpy(form, rep, sizeof rep);
  if (o) dO.fetch(o, "output"); else dO.fetch(o16, "bf16 output");
  // K and V are inputs: the launch leaves every byte of them as it was
  if (memcmp(to_host<uint8_t>(dK, (size_t)kv_elems * eb).data(), k, (size_t)kv_elems * eb) != 0) fail(std::string(what) + ": the launch changed K");
  if (memcmp(to_host<uint8_t>(dV, (size_t)kv_elems * eb).data(), v, (size_t)kv_elems * eb) != 0) fail(std::string(what) + ": the launch changed V");
  Q3A_CATCH(nullptr)
}

int32_t q3a_selftest_draft_accept(int32_t device, int32_t S, const int32_t* draft_ids, const int32_t* draft_off, const int32_t* prompt_lens,
                                  const int32_t* top_ids, const float* top_lp, int32_t out_stride, const uint16_t* embed, int32_t V, int32_t H,
                                  const float* norm_w, int32_t group_size, const float* cos_t, const float* sin_t, int32_t max_pos,
                                  int32_t* accepted, int32_t* out_ids, float* out_lp, int32_t* state, float* x_next, float* rope_cur,
                                  uint16_t* nn_x, float* nn_ss) {
  Q3A_TRY(nullptr)
  const char* what = "q3a_selftest_draft_accept";
  if (S < 1 || !draft_off || !prompt_lens || !top_ids || !embed || !cos_t || !sin_t || !accepted || !out_ids || !state || !x_next || !rope_cur)
    fail(std::string(what) + ": bad argument");
  if (out_stride < 1 || V < 1 || H < 64 || H % 64 != 0 || max_pos < 1) fail(std::string(what) + ": bad shape");
  if (group_size < 1 || group_size > 32) fail(std::string(what) + ": group_size must lie in [1, 32]");
  if (norm_w && (!nn_x || !nn_ss)) fail(std::string(what) + ": norm_w needs nn_x and nn_ss");
  if (draft_off[0] != 0) fail(std::string(what) + ": draft_off[0] must be 0");
  const size_t Sz = S;
  for (size_t s = 0; s < Sz; ++s) {
    const int n = draft_off[s + 1] - draft_off[s];
    if (n < 0 || (n > 0 && !draft_ids)) fail(std::string(what) + ": bad draft offsets");
    if (prompt_lens[s] < 1 || prompt_lens[s] + n >= max_pos) fail(std::string(what) + ": a position outside the RoPE tables");
  }
  const size_t nd = draft_off[S], M = nd + Sz;
  for (size_t r = 0; r < M; ++r)
    if (top_ids[r] < 0 || top_ids[r] >= V) fail(std::string(what) + ": a head id outside the embedding table");
  use_device(device);
  const int groups = (S + group_size - 1) / group_size, nparts = H / 16;
  const size_t nnx = (size_t)groups * 32 * H, nns = (size_t)groups * nparts * 32;
  std::vector<int> dr(draft_ids, draft_ids + nd);
  dr.resize(nd + 4, 0);
  const DevBuf dDr = to_device(dr), dOff = to_device(draft_off, Sz + 1), dPl = to_device(prompt_lens, Sz), dTop = to_device(top_ids, M);
  DevBuf dTlp;
  if (top_lp) dTlp = to_device(top_lp, M);
  const DevBuf dAcc = room(Sz * 8), dTok = room(Sz * 4), dSc = to_device(std::vector<int>(Sz, -7)), dPos = to_device(std::vector<int>(Sz, -7));
  const Guarded gIds(out_ids, Sz * out_stride * 4);
  Guarded gLp;
  if (top_lp && out_lp) gLp = Guarded(out_lp, Sz * out_stride * 4);
  const DevBuf dDone = to_device(std::vector<uint8_t>(Sz, 0)), dNd = to_device(std::vector<int>(16, 0)), dProg = to_device(std::vector<int>(16, 0));
  const DevBuf dEmb = to_device(embed, (size_t)V * H), dCos = to_device(cos_t, (size_t)max_pos * 64), dSin = to_device(sin_t, (size_t)max_pos * 64);
  const Guarded gX(x_next, Sz * H * 4), gRope(rope_cur, Sz * 128 * 4);
  DevBuf dW;
  Guarded gNx, gNs;
  if (norm_w) { dW = to_device(norm_w, (size_t)H); gNx = Guarded(nn_x, nnx * 2); gNs = Guarded(nn_ss, nns * 4); }
  DraftAcceptArgs a{};
  a.n_seq = S; a.draft = dDr.as<int>(); a.draft_off = dOff.as<int>(); a.prompt_len = dPl.as<int>();
  a.top_id = dTop.as<int>(); a.top_lp = top_lp ? dTlp.as<float>() : nullptr; a.accepted = dAcc.as<int>();
  StepCommit& c = a.c;
  c = bare_commit(S, dTok, gIds.as<int>(), out_stride, gLp.b.p ? gLp.as<float>() : nullptr, dSc, dPos, dDone, dEmb.as<uint16_t>(), H, gX.as<float>(), kEos0, kEos1);
  c.n_done = dNd.as<int>(); c.host_progress = dProg.as<int>();
  c.cos_t = dCos.as<float>(); c.sin_t = dSin.as<float>(); c.rope_cur = gRope.as<float>();
  if (norm_w) {
    c.nn.next_w = dW.as<float>(); c.nn.next_xw16f = gNx.as<uint16_t>(); c.nn.next_ss = gNs.as<float>(); c.nn.nparts = nparts;
    c.nn.group_stride_x = (long)32 * H; c.nn.group_stride_ss = (long)nparts * 32; c.nn.group_size = group_size;
  }
  KCHK(launch_draft_accept(a, nullptr));
  finish();
  to_host(accepted, dAcc, Sz * 2);
  gIds.fetch(out_ids, "out_ids");
  if (gLp.b.p) gLp.fetch(out_lp, "out_lp");
  gX.fetch(x_next, "x_next");
  gRope.fetch(rope_cur, "rope_cur");
  if (norm_w) { gNx.fetch(nn_x, "nn_x"); gNs.fetch(nn_ss, "nn_ss"); }
  // state: next_tok [S] | step_count [S] | pos [S] | done [S] | n_done | progress[0] | progress[1]
  to_host(state, dTok, Sz);
  to_host(state + Sz, dSc, Sz);
  to_host(state + 2 * Sz, dPos, Sz);
  const std::vector<uint8_t> dn = to_host<uint8_t>(dDone, Sz);
  for (size_t s = 0; s < Sz; ++s) state[3 * Sz + s] = dn[s];
  to_host(state + 4 * Sz, dNd, 1);
  to_host(state + 4 * Sz + 1, dProg, 2);
  Q3A_CATCH(nullptr)
}

int32_t q3a_selftest_gemm(int32_t device, int32_t M, int32_t N, int32_t K, int32_t split, float* max_abs_err,
                          float* ref_abs_max) {
  Q3A_TRY(nullptr)
  use_device(device);
  Lcg rnd{12345u};
  GemmCase c(rnd, M, N, K, false);
  GemmEpilogue ep; ep.out = c.dY.as<float>(); ep.ldo = N;
  KCHK(launch_gemm(c.dX.as<float>(), K, c.dW.as<uint16_t>(), M, N, K, ep, false, split != 0, nullptr));
  float me = 0.f, rm = 0.f;
  c.check(M, N, K, me, rm);
  if (max_abs_err) *max_abs_err = me;  if (ref_abs_max) *ref_abs_max = rm;
  Q3A_CATCH(nullptr)
}

int32_t q3a_selftest_gemm16(int32_t device, int32_t M, int32_t N, int32_t K, int32_t reps, float* max_abs_err,
                            float* ref_abs_max, float* avg_us_bf16, float* avg_us_f32) {
  Q3A_TRY(nullptr)
  use_device(device);
  Lcg rnd{777u};
  GemmCase c(rnd, M, N, K, true);  // bf16-representable activations: the bf16 copy is exact
  const size_t MN = c.MN;
  const DevBuf &dX = c.dX, &dW = c.dW, dX16 = room(c.X.size() * 2);
  KCHK(launch_to_bf16(dX.as<float>(), dX16.as<uint16_t>(), c.X.size(), nullptr));
  GemmEpilogue ep; ep.out = c.dY.as<float>(); ep.ldo = N;
  KCHK(launch_gemm16(dX16.as<uint16_t>(), K, dW.as<uint16_t>(), M, N, K, ep, false, nullptr));
  float me = 0.f, rm = 0.f;
  c.check(M, N, K, me, rm);
  const std::vector<float>& R = c.R;
  // ---- the epilogue variants, against the reference product R ----
  {
    const int P = 7;  // addend period
    std::vector<float> bias(N), addend((size_t)P * N), resid(MN);
    std::vector<int> rowmap(M);
    for (auto& v : bias) v = rnd();
    for (auto& v : addend) v = rnd();
    for (auto& v : resid) v = rnd();
    for (int m = 0; m < M; ++m) rowmap[m] = (m % 11 == 5) ? -1 : M - 1 - m;  // reversed rows, some dropped
    const DevBuf dB = to_device(bias), dA = to_device(addend), dS = to_device(resid), dM = to_device(rowmap);
    const DevBuf dY2 = to_device(std::vector<float>(MN, 0.f)), dY16 = room(MN * 2);
    // (a) fp32 out: bias + periodic addend + row map + residual
    GemmEpilogue e2; e2.out = dY2.as<float>(); e2.ldo = N; e2.bias = dB.as<float>(); e2.addend = dA.as<float>(); e2.addend_period = P;
    e2.rowmap = dM.as<int>(); e2.resid = dS.as<float>();
    KCHK(launch_gemm16(dX16.as<uint16_t>(), K, dW.as<uint16_t>(), M, N, K, e2, false, nullptr));
    finish();
    const std::vector<float> Y2 = to_host<float>(dY2, MN);
    std::vector<char> hit(M, 0);
    for (int m = 0; m < M; ++m) {
      const int o = rowmap[m];
      if (o < 0) continue;
      hit[o] = 1;
      for (int n = 0; n < N; ++n) {
        const float want = R[(size_t)m * N + n] + bias[n] + addend[(size_t)(m % P) * N + n] + resid[(size_t)o * N + n];
        me = std::max(me, std::fabs(Y2[(size_t)o * N + n] - want));
      }
    }
    for (int o = 0; o < M; ++o)
      if (!hit[o])
        for (int n = 0; n < N; ++n)
          if (Y2[(size_t)o * N + n] != 0.f) fail("selftest_gemm16: a row dropped by the row map was written");
    // (b) bf16 out: bias only; one bf16 ulp
    GemmEpilogue e3; e3.out16 = dY16.as<uint16_t>(); e3.ldo = N; e3.bias = dB.as<float>();
    KCHK(launch_gemm16(dX16.as<uint16_t>(), K, dW.as<uint16_t>(), M, N, K, e3, false, nullptr));
    finish();
    std::vector<uint16_t> Y16 = to_host<uint16_t>(dY16, MN);
    for (size_t i = 0; i < Y16.size(); ++i) {
      const float want = R[i] + bias[i % N];
      if (std::fabs(bf16_value(Y16[i]) - want) > std::fabs(want) / 128.f + 1e-4f * std::max(rm, 1.f)) fail("selftest_gemm16: bf16 output with bias is off by more than an ulp");
    }
    // (c) SwiGLU pairs ([16 gate | 16 up] row blocks of W), bf16 out
    if (N % 32 == 0) {
      GemmEpilogue e4; e4.out16 = dY16.as<uint16_t>(); e4.ldo = N / 2;
      KCHK(launch_gemm16(dX16.as<uint16_t>(), K, dW.as<uint16_t>(), M, N, K, e4, true, nullptr));
      finish();
      to_host(Y16.data(), dY16, MN / 2);
      for (int m = 0; m < M; ++m)
        for (int c2 = 0; c2 < N / 2; ++c2) {
          const float g = R[(size_t)m * N + (c2 / 16) * 32 + c2 % 16], u = R[(size_t)m * N + (c2 / 16) * 32 + 16 + c2 % 16];
          const float want = g / (1.f + std::exp(-g)) * u;
          if (std::fabs(bf16_value(Y16[(size_t)m * (N / 2) + c2]) - want) > std::fabs(want) / 64.f + 1e-3f * std::max(rm * rm, 1.f))
            fail("selftest_gemm16: SwiGLU epilogue is off");
        }
    }
  }
  if (max_abs_err) *max_abs_err = me;  if (ref_abs_max) *ref_abs_max = rm;
  if (reps > 0) {
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    auto avg_us = [&](auto&& launch) {  // `reps` back-to-back launches between two events
      float ms = 0.f;
      HIPCHK(hipEventRecord(a, nullptr));
      for (int r = 0; r < reps; ++r) KCHK(launch());
      HIPCHK(hipEventRecord(b, nullptr));
      HIPCHK(hipEventSynchronize(b));
      HIPCHK(hipEventElapsedTime(&ms, a, b));
      return ms * 1000.f / reps;
    };
    const float us16 = avg_us([&] { return launch_gemm16(dX16.as<uint16_t>(), K, dW.as<uint16_t>(), M, N, K, ep, false, nullptr); });
    const float us32 = avg_us([&] { return launch_gemm(dX.as<float>(), K, dW.as<uint16_t>(), M, N, K, ep, false, false, nullptr); });
    if (avg_us_bf16) *avg_us_bf16 = us16;
    if (avg_us_f32) *avg_us_f32 = us32;
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
  }
  Q3A_CATCH(nullptr)
}

}  // extern "C"
