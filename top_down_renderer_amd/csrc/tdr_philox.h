// tdr_philox.h — Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the
// counter-based random source of the recovery injection (include/tdr.h, "recovery injection").  Four words out of a
// 128-bit counter and a 64-bit key, no state: a word depends on (counter, key) alone, never on who asked first, and the
// reference's std::mt19937 stream is not touched.  Device and host; integer operations only.
#ifndef TDR_PHILOX_H_
#define TDR_PHILOX_H_
#include <cstdint>

#if defined(__HIPCC__)
#define TDR_PHILOX_FN __host__ __device__ __forceinline__
#else
#define TDR_PHILOX_FN inline
#endif

struct TdrPhilox4 {
  uint32_t w[4];
};

TDR_PHILOX_FN TdrPhilox4 tdr_philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; round++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return TdrPhilox4{{c0, c1, c2, c3}};
}
#endif  // TDR_PHILOX_H_
