// fastdiv.h — unsigned division by a launch constant as a multiply-high and a shift (host and
// device).  The host makes the magic pair for a divisor d and the largest dividend nmax the
// kernel can form, and refuses a pair that is not exact on 0..nmax; the kernel then divides
// with two scalar (or vector) instructions where the compiler's expansion of n / d is ~35.
//
// For k = 32 + shift and mul = ceil(2^k / d), e = mul * d - 2^k (0 <= e < d):
//   n * mul / 2^k = n / d + n * e / (d * 2^k),
// and the floor of that equals floor(n / d) for every n <= nmax exactly when the excess stays
// below the distance to the next integer at the worst residue (n = d - 1 mod d: 1 / d), i.e.
// when nmax * e < 2^k.  The smallest shift whose pair satisfies that (and fits 32 bits) is
// taken.  d = 1 has no 32-bit multiplier (it would be 2^32): mul = 0 stands for it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TTS_FASTDIV_HD __host__ __device__ inline
#else
#define TTS_FASTDIV_HD inline
#endif

namespace tts {

struct FastDiv {
  uint32_t mul = 0;    // ceil(2^(32 + shift) / d); 0: d == 1
  uint32_t shift = 0;  // 0..31
};

// floor(n / d) for 0 <= n <= the nmax the pair was made for
TTS_FASTDIV_HD uint32_t fastdiv(uint32_t n, FastDiv f) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t hi = __umulhi(n, f.mul);
#else
  const uint32_t hi = (uint32_t)(((uint64_t)n * f.mul) >> 32);
#endif
  return f.mul ? hi >> f.shift : n;
}
// the same where the host has made sure that d > 1 (no test for the d == 1 form)
TTS_FASTDIV_HD uint32_t fastdiv_gt1(uint32_t n, FastDiv f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(n, f.mul) >> f.shift;
#else
  return (uint32_t)(((uint64_t)n * f.mul) >> 32) >> f.shift;
#endif
}

// The pair for divisor d, exact for every dividend 0..nmax.  False (and *out untouched) when
// d == 0 or no 32-bit pair is exact on that range: the caller must then refuse the launch.
inline bool fastdiv_make(uint32_t d, uint32_t nmax, FastDiv* out) {
  if (d == 0) return false;
  if (d == 1) {
    *out = FastDiv{0u, 0u};
    return true;
  }
  for (uint32_t s = 0; s < 32; ++s) {
    const unsigned __int128 p = (unsigned __int128)1 << (32 + s);
    const unsigned __int128 m = (p + d - 1) / d;
    if (m >> 32) break;  // (mul grows with the shift: no later one fits either)
    const unsigned __int128 e = m * d - p;
    if ((unsigned __int128)nmax * e < p) {
      *out = FastDiv{(uint32_t)m, s};
      return true;
    }
  }
  return false;
}

// Is this pair exact for d on 0..nmax?  (the condition above, for a pair made elsewhere)
inline bool fastdiv_exact(FastDiv f, uint32_t d, uint32_t nmax) {
  if (d == 0) return false;
  if (f.mul == 0) return d == 1;
  if (f.shift > 31) return false;
  const unsigned __int128 p = (unsigned __int128)1 << (32 + f.shift);
  const unsigned __int128 md = (unsigned __int128)f.mul * d;
  if (md < p || md - p >= d) return false;  // mul is not ceil(2^k / d)
  return (unsigned __int128)nmax * (md - p) < p;
}

}  // namespace tts
