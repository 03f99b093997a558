// tdr_mt_dev.h — mt19937 words as the reference's distributions read them: the tempering of a raw state word,
// generate_canonical<float, 24> and one attempt of libstdc++'s normal_distribution (Marsaglia polar).  The generator
// kernels (tdr_rng.hip) and the device particle initialisation (tdr_init.hip) both call these, so both sit on the same
// stream, bit for bit.
#ifndef TDR_MT_DEV_H_
#define TDR_MT_DEV_H_
#include "tdr_common.h"
#include "tdr_logf.h"

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
  y ^= (y >> 11);                    // (d = 0xffffffff)
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= (y >> 18);
  return y;
}
// generate_canonical<float, 24>(mt19937) (bits/random.tcc): one word, float(u) / 2^32, clamped below 1
__device__ __forceinline__ float mt_canonical(uint32_t u) {
  float c = (float)u * 0x1p-32f;     // u32 -> float rounds to nearest; the scaling is exact
  return c >= 1.f ? 0x1.fffffep-1f : c;
}

// the attempt on the raw words g, g + 1 of the stream
struct MtAttempt {
  float c0, c1;      // the two canonical floats
  float x, y, r2;
  bool ok;           // accepted
};
__device__ __forceinline__ MtAttempt mt_attempt(const uint32_t* __restrict__ raw, int64_t g) {
  MtAttempt a;
  a.c0 = mt_canonical(mt_temper(raw[g]));
  a.c1 = mt_canonical(mt_temper(raw[g + 1]));
  a.x = (float)((double)(2.0f * a.c0) - 1.0);   // result_type(2.0) * aurng() - 1.0: float product, double difference
  a.y = (float)((double)(2.0f * a.c1) - 1.0);
  a.r2 = a.x * a.x + a.y * a.y;                 // (compiled with -ffp-contract=off: two roundings, like the host's)
  a.ok = !((double)a.r2 > 1.0 || (double)a.r2 == 0.0);
  return a;
}
// std::sqrt(-2 * std::log(r2) / r2) of an accepted attempt: the float overloads (glibc logf, IEEE division and square
// root); the attempt's two values are y * mult and x * mult, in that order
__device__ __forceinline__ float mt_attempt_mult(float r2) { return sqrtf(-2.f * tdr_libm::logf_t<true>(r2) / r2); }

#endif  // TDR_MT_DEV_H_
