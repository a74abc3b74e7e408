// The embedding row of a chosen token as the next decode step reads it, shared by the kernels that end a step or begin one
// (k_decode.hip argmax_finalize / set_tokens, k_draft.hip draft_accept).
#pragma once
#include "dev.h"
#include "kernels.h"

namespace q3a {

// x_next[s] = embedding row `id` (fp32).  With nn.next_w set (skinny decode path) the row is also handed to the next
// GEMM pre-normalised: bf16(x * w_norm) in fragment order plus its sum of squares (kernels.h NextNormOut), so that GEMM
// neither re-reads the fp32 row with 16-line fragment loads nor needs a norm launch.  `red`: shared, one float per wave.
__device__ __forceinline__ void embed_row(const uint16_t* __restrict__ embed, int id, int H, float* __restrict__ x_next, int s,
                                          const NextNormOut& nn, float* red) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  const uint2* src = reinterpret_cast<const uint2*>(embed + (size_t)id * H);
  float4* dst = reinterpret_cast<float4*>(x_next + (size_t)s * H);
  const int gs = nn.group_size > 0 ? nn.group_size : 32;
  const int sl = s % gs;  // position inside its group of sequences (fragment-order buffers hold one group each)
  uint16_t* const xw = nn.next_xw16f + (size_t)(s / gs) * nn.group_stride_x;
  float* const nss = nn.next_ss + (size_t)(s / gs) * nn.group_stride_ss;
  float ss = 0.f;
  for (int i = tid; i < H / 4; i += nthr) {
    const uint2 v = src[i];
    const float4 f = make_float4(bf16lo(v.x), bf16hi(v.x), bf16lo(v.y), bf16hi(v.y));
    dst[i] = f;
    if (nn.next_w) {
      const float4 w = reinterpret_cast<const float4*>(nn.next_w)[i];
      ss += f.x * f.x + f.y * f.y + f.z * f.z + f.w * f.w;
      uint2 pk;  // k = 4i .. 4i+3 are consecutive in fragment order
      pk.x = pack_bf16x2(f.x * w.x, f.y * w.y);
      pk.y = pack_bf16x2(f.z * w.z, f.w * w.w);
      *reinterpret_cast<uint2*>(xw + skinny_frag_index(sl, 4 * i)) = pk;
    }
  }
  if (nn.next_w) {  // kernel-argument condition: uniform
    ss = wave_sum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    if (tid == 0) {
      float t = 0.f;
      for (int w = 0; w < (nthr + 63) / 64; ++w) t += red[w];
      nss[sl] = t;
    }
    for (int p = 1 + tid; p < nn.nparts; p += nthr) nss[(size_t)p * 32 + sl] = 0.f;
  }
}

}  // namespace q3a
