// Receive-and-reduce (--reduce): the element types, the map from PRNG words to
// operands, and the sum of one 32-bit word over K operands.  Shared by the
// gfx950 reduce / fill_operand / verify_reduced kernels (reduce.hip), the host
// transport and the host-side regeneration of expected values, so all of them
// produce the same bits.
//
// Operands.  A message's operand words are the sender's PRNG words passed
// through operand_word(), which pins the exponent field of every float:
//   u32   identity; the sum wraps mod 2^32;
//   f32   (w & 0xBFFFFFFF) | 0x20000000: bit 30 cleared, bit 29 set, so the
//         exponent field lies in [64, 127] and |x| is in [2^-63, 2);
//   bf16  the same map on both halves: (w & 0xBFFFBFFF) | 0x20002000.
// Every operand is finite.  With at most a few dozen operands (kMaxReduceSeeds)
// a partial sum stays below 32 * 2 = 2^6 < 2^7, far from overflow.  A non-zero
// partial sum of such values is a multiple of the ulp of the smallest addend,
// 2^-63 * 2^-23 = 2^-86 for f32 and 2^-63 * 2^-7 = 2^-70 for bf16 (widened to
// f32, summed in f32), far above f32's subnormal range (< 2^-126): no add
// produces or consumes a subnormal, so the device's denormal mode cannot
// change a bit.  The single bf16 rounding at the end sees a normal f32 too.
//
// Order.  The sum is sequential in operand order (operand 0 is the receiver's
// own shard, then the incoming messages as posted): f32 is a chain of plain
// f32 adds; bf16 widens each element to f32 (a shift), chains f32 adds and
// rounds once at the end, to nearest even.  Only adds occur, nothing is fused
// or reassociated.
#pragma once

#include <cstdint>
#include <string>

#include "prng.hpp"

namespace p2p {

enum class ReduceType : int { Off = 0, U32 = 1, F32 = 2, Bf16 = 3 };
constexpr int kMaxReduceSeeds = 32;  // operands verify_reduced regenerates ("a few dozen" above)

inline const char* reduce_type_name(ReduceType t) {
  return t == ReduceType::U32 ? "u32" : t == ReduceType::F32 ? "f32" : t == ReduceType::Bf16 ? "bf16" : "off";
}
// "u32" | "f32" | "bf16" (and "off"); false for anything else.
inline bool parse_reduce_type(const std::string& s, ReduceType* t) {
  for (ReduceType c : {ReduceType::Off, ReduceType::U32, ReduceType::F32, ReduceType::Bf16})
    if (s == reduce_type_name(c)) {
      *t = c;
      return true;
    }
  return false;
}

P2P_HD uint32_t operand_word(uint32_t w, ReduceType t) {
  if (t == ReduceType::F32) return (w & 0xBFFFFFFFu) | 0x20000000u;
  if (t == ReduceType::Bf16) return (w & 0xBFFFBFFFu) | 0x20002000u;
  return w;
}

P2P_HD float reduce_bits_to_f32(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}
P2P_HD uint32_t reduce_f32_to_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}

// Two finite, normal f32 values rounded to nearest even into one word of two
// bf16 (lo in bits 0..15).  On gfx950 this is the packed conversion
// v_cvt_pk_bf16_f32; elsewhere the same rounding in integer arithmetic.
P2P_HD uint32_t reduce_pack_bf16(float lo, float hi) {
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  const f32x2 v = {lo, hi};
  const bf16x2 b = __builtin_convertvector(v, bf16x2);
  uint32_t u;
  __builtin_memcpy(&u, &b, 4);
  return u;
#else
  uint32_t a = reduce_f32_to_bits(lo), b = reduce_f32_to_bits(hi);
  a += 0x7FFFu + ((a >> 16) & 1u);
  b += 0x7FFFu + ((b >> 16) & 1u);
  return (a >> 16) | (b & 0xFFFF0000u);
#endif
}

// The running sum of one 32-bit word: begin with operand 0, add the others in
// order, finish once.
struct ReduceAcc {
  uint32_t u;
  float lo, hi;  // f32: lo only; bf16: the two halves widened
};
P2P_HD ReduceAcc reduce_begin(uint32_t w, ReduceType t) {
  ReduceAcc a{w, 0.0f, 0.0f};
  if (t == ReduceType::F32) a.lo = reduce_bits_to_f32(w);
  if (t == ReduceType::Bf16) {
    a.lo = reduce_bits_to_f32(w << 16);
    a.hi = reduce_bits_to_f32(w & 0xFFFF0000u);
  }
  return a;
}
P2P_HD void reduce_add(ReduceAcc& a, uint32_t w, ReduceType t) {
  if (t == ReduceType::F32) {
    a.lo = a.lo + reduce_bits_to_f32(w);
  } else if (t == ReduceType::Bf16) {
    a.lo = a.lo + reduce_bits_to_f32(w << 16);
    a.hi = a.hi + reduce_bits_to_f32(w & 0xFFFF0000u);
  } else {
    a.u += w;
  }
}
P2P_HD uint32_t reduce_finish(const ReduceAcc& a, ReduceType t) {
  if (t == ReduceType::F32) return reduce_f32_to_bits(a.lo);
  if (t == ReduceType::Bf16) return reduce_pack_bf16(a.lo, a.hi);
  return a.u;
}

// One 32-bit word of K operands (k >= 1), summed in operand order.
P2P_HD uint32_t reduce_word(const uint32_t* w, int k, ReduceType t) {
  ReduceAcc a = reduce_begin(w[0], t);
  for (int i = 1; i < k; ++i) reduce_add(a, w[i], t);
  return reduce_finish(a, t);
}

// Host side (transport_host.cpp): out = the sum of the k operand buffers of
// `bytes` (a multiple of 4) each; out may be operand 0.  Any alignment.
void host_reduce(void* out, const void* const* operands, int k, size_t bytes, ReduceType t);
// Operand stream `seed`: host_fill with operand_word applied.
void host_fill_operand(void* p, size_t bytes, uint64_t seed, ReduceType t);
// Compares p with the sum of the operand streams `seeds` (operand order).
VerifyResult host_verify_reduced(const void* p, size_t bytes, const uint64_t* seeds, int nseeds, ReduceType t);

}  // namespace p2p
