// tdr_score_int_dev.h — what the kernels of the INTEGER form share: score_polar_su_kernel (tdr_score_su.hip),
// score_polar_ray_kernel (tdr_score_ray.hip), score_cart_su_kernel and score_cart_ray_kernel (tdr_score_cart.hip).  The
// polar and the Cartesian kernels differ in how a sample's point is formed and in how a list word names its bin; the rest
// — the cell of a point, the addresses with a per-bin constant, the dictionary lookup, the per-class accumulate, the
// ray-mapped kernels' prologue, list pass and epilogue, the words a kernel writes — is here once.  (Not here: the two halves
// of a ray-mapped sample and the wave's box of the known mask stand in both geometries' files; the shared forms compiled
// the polar kernels worse, see tdr_score_ray.hip and tdr_score_su.hip.)  Every function is forced inline and takes what it needs as arguments; where the geometries differ it takes a
// callable.
#ifndef TDR_SCORE_INT_DEV_H_
#define TDR_SCORE_INT_DEV_H_
#include "tdr_score_dev.h"

typedef float tdr_v2f __attribute__((ext_vector_type(2)));

// Cell of a sample from its point {row, column} in map cells: clamped into the guard ring [-1, rows] x [-1, cols], then
// rounded half away from zero (round_half_away_clamped, on both coordinates at once).  The caller forms the point its own
// way: table entry, direction x radius, row term + column term.
__device__ __forceinline__ void int_cell(tdr_v2f pv, float rmaxf, float cmaxf, int& ri, int& ci) {
  tdr_v2f qv = {__builtin_amdgcn_fmed3f(pv.x, -1.f, rmaxf), __builtin_amdgcn_fmed3f(pv.y, -1.f, cmaxf)};
  qv = qv + 0.49999997f;
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(ri) : "v"(qv.x));
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(ci) : "v"(qv.y));
}

// ---- addresses with the PER-BIN constant in a scalar register ----------------------------------------------------------------
// A VALU instruction takes at most one SGPR operand.  cmap_offset, plane_offset and kmask_offset (tdr_score_dev.h) are for
// a lane whose constant is its own (a class table entry, a particle's plane): the column stride is the scalar, the constant
// a vector register.  The dense kernels read the constant out of the bin's descriptor with a scalar load — it is
// wave-uniform — and keep the stride, which lives through the whole kernel, in a vector register: the forms below, the
// operand classes the other way round.
template <int CW>
__device__ __forceinline__ unsigned cmap_offset_sconst(int ri, int ci, int ckcol, uint32_t ckconst) {   // the record's dword
  int t1, t2, off;
  const int cq = ci >> 2;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(t1) : "v"(cq), "v"(ckcol), "s"(ckconst));
  asm("v_lshl_add_u32 %0, %1, %2, %3" : "=v"(t2) : "v"(ci), "n"(CW == 1 ? 2 : (CW == 2 ? 3 : 4)), "v"(t1));
  asm("v_lshl_add_u32 %0, %1, %2, %3" : "=v"(off) : "v"(ri), "n"(CW == 1 ? 4 : (CW == 2 ? 5 : 6)), "v"(t2));
  return (unsigned)off;
}
__device__ __forceinline__ unsigned plane_offset_sconst(int ri, int ci, int pkcol, uint32_t pkconst) {   // the class plane's cell
  int t1, t2, off;
  const int cq = ci >> 3;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(t1) : "v"(cq), "v"(pkcol), "s"(pkconst));
  asm("v_lshl_add_u32 %0, %1, 1, %2" : "=v"(t2) : "v"(ci), "v"(t1));
  asm("v_lshl_add_u32 %0, %1, 4, %2" : "=v"(off) : "v"(ri), "v"(t2));
  return (unsigned)off;
}
// the known mask STAGED IN LDS (the dense kernels' boxes): LDS byte address of the cell's word — row ri has krow4 bytes, the box's
// constant is scalar — and the cell's bit of that word as 0 / -1
__device__ __forceinline__ unsigned staged_mask_addr(int ri, int ci, int krow4, int kconst) {
  int wa;
  unsigned la;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(wa) : "v"(ri), "v"(krow4), "s"(kconst));
  const int cw5 = ci >> 5;
  asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(la) : "v"(cw5), "v"(wa));
  return la;
}
__device__ __forceinline__ int staged_mask_bit(uint32_t word, int ci) {
  int kmsk;
  asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(kmsk) : "v"(word), "v"(ci));
  return kmsk;
}

// ---- the integer dictionary (in LDS) ------------------------------------------------------------------------------------------
// x holds a dictionary index * 4 in bits 2..11: a class plane's cell, or a compact record's dword shifted down to a field
__device__ __forceinline__ uint32_t int_dict_at(const uint32_t* ldict, uint32_t x) {
  return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(ldict) + (x & 0xFFCu));
}
// distance k of a compact record whose dword k / 3 is ww (cmap_decode, one field, as an integer)
__device__ __forceinline__ uint32_t int_record_field(const uint32_t* ldict, uint32_t ww, int k) {
  const int sh = 10 * (k % 3);
  return int_dict_at(ldict, sh ? ww >> sh : ww);
}
// acc[cd - 1] += v * m for a bin that holds class cd - 1 only: a switch over a wave-uniform value (v: the bin's count,
// scalar; m: the looked-up dictionary value), so that the accumulators stay registers
template <class T, int ND>
__device__ __forceinline__ void int_add_class(T (&acc)[ND], uint32_t cd, uint32_t v, uint32_t m) {
  switch (cd) {
#define TDR_INT_CASE(K)                                                                                            \
  case K + 1:                                                                                                      \
    if constexpr (K < ND) asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc[K < ND ? K : 0]) : "s"(v), "v"(m) : "vcc"); \
    break;
    TDR_INT_CASE(0) TDR_INT_CASE(1) TDR_INT_CASE(2) TDR_INT_CASE(3) TDR_INT_CASE(4) TDR_INT_CASE(5)
    TDR_INT_CASE(6) TDR_INT_CASE(7) TDR_INT_CASE(8) TDR_INT_CASE(9) TDR_INT_CASE(10)
#undef TDR_INT_CASE
    default: break;
  }
}

// ---- a launch's sums: ONE block [2 ncls + 2][npad] of words for all its kernels, rows, waves and splits ------------------------
// Rows 2 k and 2 k + 1 together are class k's 64-bit sums, one per slot (8-byte aligned: the block is, npad is a multiple of
// 64); row 2 ncls the normalisation, row 2 ncls + 1 the known count, 32-bit words (their totals stay below 2^32:
// score_prep_kernel's bound on the scan's mass, a window of fewer than 2^32 samples).  Whoever holds a share of a slot's
// sums ADDS it — integers: the total is the same number in whatever order the shares arrive — with relaxed no-return
// atomics of agent scope, a class sum with one 64-bit add (two 32-bit adds would lose the carry between the halves).  The
// launch in front of the first scoring kernel zeroes the block (int_zero_sums); score_finalize_exact_kernel reads it.
__device__ __forceinline__ void int_add_u64(unsigned long long* at, unsigned long long v) {
  (void)__hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void int_add_u32(uint32_t* at, uint32_t v) {
  (void)__hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the zeroing, by every thread of a grid of `threads` threads of which this is thread `t` (words: a multiple of 4 — npad is
// one of 64; 16-byte stores where the block is aligned for them)
__device__ __forceinline__ void int_zero_sums(uint32_t* sums, int64_t words, int64_t t, int64_t threads) {
  if (!sums) return;
  if ((reinterpret_cast<uintptr_t>(sums) & 15) == 0) {
    uint4* const s4 = reinterpret_cast<uint4*>(sums);
    for (int64_t i = t; i < (words >> 2); i += threads) s4[i] = make_uint4(0u, 0u, 0u, 0u);
  } else {
    for (int64_t i = t; i < words; i += threads) sums[i] = 0u;
  }
}
// what a lane = particle kernel adds: the lane's sums over its row's samples, at the particle's slot.  (A zero adds nothing
// and is not sent: a row of few rings meets few classes.)
template <class T, int ND>
__device__ __forceinline__ void int_add_sums(uint32_t* sums, int64_t npad, int64_t slot, int ncls, const T (&acc)[ND], uint32_t norm,
                                             uint32_t known) {
  unsigned long long* const s64 = reinterpret_cast<unsigned long long*>(sums) + slot;
#pragma unroll
  for (int k = 0; k < ND; k++)
    if (k < ncls && (unsigned long long)acc[k] != 0ull) int_add_u64(s64 + (int64_t)k * npad, (unsigned long long)acc[k]);
  if (norm) int_add_u32(sums + (int64_t)(2 * ncls) * npad + slot, norm);
  if (known) int_add_u32(sums + (int64_t)(2 * ncls + 1) * npad + slot, known);
}

// ---- the ray-mapped kernels (one wave per particle): prologue, list pass, epilogue ---------------------------------------------
// Both launch structs (RayArgs, CartRayArgs) name the fields these read alike.
// Prologue, up to the workgroup's barrier (the caller's): the dictionary into LDS; lut, per class code: {plane constant,
// column shift, known-bit index, accumulator}; the lane's accumulators zeroed — lacc [4 waves][ncls + 1][64 lanes], a lane's
// sums per class (slot 0: no class).  Returns the lane's accumulator 0.
template <class Args>
__device__ __forceinline__ unsigned long long* ray_prologue(const Args& a, unsigned long long* lacc, uint32_t* ldict, uint4* lut,
                                                            int wave, int lane) {
  for (int t = threadIdx.x; t < a.dict_n; t += 256) ldict[t] = a.dict_int[t];
  const unsigned pconst = (unsigned)(a.pkcol + 16) + 128u;   // plane_offset's constant without the plane's own offset
  if (threadIdx.x < 16) {
    const int code = threadIdx.x;
    uint4 e;
    if (code >= 1 && code <= a.ncls) {   // class code - 1 alone: its plane, cells as they are, `known` in bit 15
      e.x = a.planes_off + (unsigned)(code - 1) * a.plane_bytes + pconst;
      e.y = 0; e.z = 15; e.w = (unsigned)code * 512u;
    } else {                             // nothing to multiply: the coarse mask plane (4 x 4 map cells per cell)
      e.x = a.cmask_off + pconst;
      e.y = 2; e.z = 0; e.w = 0;
    }
    lut[code] = e;
  }
  unsigned long long* const my = lacc + (size_t)wave * (a.ncls + 1) * 64 + lane;
  for (int c = 0; c <= a.ncls; c++) my[c * 64] = 0;
  return my;
}
// The list: bins that hold several classes (or one large count).  The loop saw them as empty bins — their cell's known bit
// is counted — ; here every class present meets its plane, and the bin's count enters the normalisation.  where(w, ri, ci)
// -> bin: the cell and the scan bin of list word w (the polar kernel un-rotates the row, the Cartesian one does not).
template <class Args, class Where>
__device__ __forceinline__ void ray_list_pass(const Args& a, int part_id, int lane, const char* crecb, const uint32_t* ldict,
                                              unsigned long long* my, uint32_t& norm, Where where) {
  const int nm = *a.n_list, mper = (nm + a.nsplit - 1) / a.nsplit;
  const int e1 = min(nm, (part_id + 1) * mper);
  for (int e = part_id * mper + lane; e < e1; e += 64) {
    int ri, ci;
    const int64_t bin = where(a.list[e], ri, ci);
    const unsigned cell_off = plane_offset(ri, ci, a.pkcol, (int)(a.planes_off + (unsigned)(a.pkcol + 16) + 128u));
    uint32_t kbit = 0;
    for (int c = 0; c < a.ncls; c++) {
      const float s = a.scan_pk[bin * a.rf + c];
      if (s != 0.f) {
        const uint32_t vv = *reinterpret_cast<const uint16_t*>(crecb + cell_off + (unsigned)c * a.plane_bytes);
        kbit = vv >> 15;
        __hip_atomic_fetch_add(&my[(c + 1) * 64], (unsigned long long)(uint32_t)s * ldict[(vv & 0xFFCu) >> 2],
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    norm += (uint32_t)a.scan_pk[bin * a.rf + a.rf - 1] & (0u - kbit);
  }
}
// Epilogue: lanes -> one sum per class, added to the launch's sums (int_add_sums has the block) at the particle's slot, by
// lane 0, as it wrote them before (kept in this shape: with the class sums collected into lanes for one atomic instruction the
// patch-order kernel took 82 registers for 79 and lost a wave per SIMD).  KNOWN_FOLDED: every lane already holds the wave's
// known count.
template <bool KNOWN_FOLDED>
__device__ __forceinline__ void ray_add_sums(uint32_t* sums, int64_t npad, int64_t slot, int ncls, int lane, unsigned long long* my,
                                             uint32_t& known, uint32_t& norm) {   // (by reference: by value the
  unsigned long long* const s64 = reinterpret_cast<unsigned long long*>(sums) + slot;   // Cartesian kernel's loop takes 7 registers more)
  for (int c = 0; c < ncls; c++) {
    unsigned long long s = __hip_atomic_load(&my[(c + 1) * 64], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
    for (int dlt = 32; dlt > 0; dlt >>= 1) s += __shfl_xor(s, dlt, 64);
    if (lane == 0 && s != 0ull) int_add_u64(s64 + (int64_t)c * npad, s);
  }
#pragma unroll
  for (int dlt = 32; dlt > 0; dlt >>= 1) {
    if constexpr (!KNOWN_FOLDED) known += __shfl_xor(known, dlt, 64);
    norm += __shfl_xor(norm, dlt, 64);
  }
  if (lane == 0) {
    if (norm) int_add_u32(sums + (int64_t)(2 * ncls) * npad + slot, norm);
    if (known) int_add_u32(sums + (int64_t)(2 * ncls + 1) * npad + slot, known);
  }
}
#endif  // TDR_SCORE_INT_DEV_H_
