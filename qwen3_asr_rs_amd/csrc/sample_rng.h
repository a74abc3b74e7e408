// The sampler's random words (include/q3asr.h "sampling"): ONE function that the device kernel
// (k_sample.hip) and the host (q3a_sample_word) both compile, so a reference can reproduce the noise of any logit on its own.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#if defined(__HIPCC__)
#define Q3A_HOST_DEVICE __host__ __device__
#else
#define Q3A_HOST_DEVICE
#endif

namespace q3a {

// Word 0 of Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) with counter (j, t, s, 0) and key
// (seed_lo, seed_hi): j the token id, t the sequence's step, s the sequence's index in the call.
Q3A_HOST_DEVICE inline uint32_t sample_word(uint32_t seed_lo, uint32_t seed_hi, uint32_t s, uint32_t t, uint32_t j) {
  uint32_t c0 = j, c1 = t, c2 = s, c3 = 0u, k0 = seed_lo, k1 = seed_hi;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

#if defined(__HIPCC__)
// g = -log(-log u) of u = ((x >> 8) + 0.5) 2^-24.  With k = x >> 8 < 2^23 that u is an fp32 number; above, k + 0.5 needs 25 bits (and
// the largest k would round to u = 1), but 1 - u = ((2^24 - k) - 0.5) 2^-24 is an fp32 number, and -log u = -log1p(-(1 - u)).
__device__ __forceinline__ float gumbel_of(uint32_t x) {
  const uint32_t k = x >> 8;
  float nl;
  if (k < (1u << 23)) nl = -logf(((float)k + 0.5f) * 0x1p-24f);
  else nl = -log1pf(-(((float)(0x1000000u - k) - 0.5f) * 0x1p-24f));
  return -logf(nl);
}
#endif

}  // namespace q3a
