// Gated receive-and-reduce (--reduce-gate H): the combine of an expert-parallel
// MoE layer.  A message is R rows of H bf16 elements; row r of the output is
//   y[r] = sum over k of g[r][k] * x_k[r]
// where x_k is operand k (operand 0 the receiver's own shard, then the incoming
// messages as posted) and g the receiver's gate table (topk_weights, padded to
// 8).  Shared by the gfx950 gated reduce / fill_gate / verify_gated_reduced
// kernels (reduce_gate.hip), the host transport and the host-side regeneration
// of expected values, so all of them produce the same bits.
//
// Operands.  Exactly --reduce bf16's operand streams (reduce_op.hpp
// operand_word): every bf16 has its exponent field in [64, 127], |x| in
// [2^-63, 2).
//
// Gate table.  R entries of 16 B; entry r holds 8 bf16 gates, gate k (bits
// 16 * (k & 1) .. of word k / 2) belongs to operand k; entries at k >= K are
// present and ignored.  Word j of entry r is gate_word() of word 4r + j of PRNG
// stream `gate_seed`: each half-word h becomes the positive bf16
//   ((123 + ((h >> 7) & 3)) << 7) | (h & 0x7F),
// exponent field 123..126, a value in [2^-4, 1).
//
// Sum.  acc = g0 * x0, then acc = acc + gk * xk in operand order, all in f32,
// rounded once to bf16 to nearest even (reduce_pack_bf16).
//
// Range.  A bf16 has 8 significant bits, so a product g * x has at most 16 and
// is exact in f32 (24): rounding the product and then the sum (mul + add) and
// rounding only the sum (v_fma_f32, or its packed form) see the same real
// number and give the same bits; nothing depends on contraction.  |g * x| < 2
// and there are at most 8 terms, so |sum| < 8 * 2 = 2^4: no overflow.  A gate is
// a multiple of 2^-4 * 2^-7 and an operand of 2^-63 * 2^-7, so every product and
// every non-zero partial sum is a multiple of 2^-81 (rounding a multiple of
// 2^-81 to 24 bits leaves one), far above f32's subnormal range (< 2^-126): no
// operation produces or consumes a subnormal, the device's denormal mode cannot
// change a bit, and the single bf16 rounding sees a normal f32 or zero.
#pragma once

#include <cstdint>

#include "prng.hpp"
#include "reduce_op.hpp"

namespace p2p {

constexpr int kGateSlots = 8;         // gates per table entry (the fan-in limit of one launch)
constexpr size_t kGateEntryBytes = 16;
constexpr size_t kGateRowMultiple = 512;  // row_elems is a multiple of this: a row is whole KiB

// Rows of a message of `bytes` with rows of `row_elems` bf16; 0 if it is not whole rows.
inline size_t gate_rows(size_t bytes, size_t row_elems) {
  return row_elems && row_elems % kGateRowMultiple == 0 && bytes % (2 * row_elems) == 0 ? bytes / (2 * row_elems) : 0;
}

// Both half-words of a PRNG word as gates: 0x3D80 = 123 << 7, and bits 7..8 of
// a half-word add 0..3 to the exponent field without a carry out of it.
P2P_HD uint32_t gate_word(uint32_t w) { return 0x3D803D80u + (w & 0x01FF01FFu); }

// Gate k of a table entry (4 words) as f32.
P2P_HD float gate_value(const uint32_t* entry, int k) {
  const uint32_t w = entry[k >> 1];
  return reduce_bits_to_f32((k & 1) ? (w & 0xFFFF0000u) : (w << 16));
}

// One 32-bit word (two bf16) of K operands under the K gates g.
P2P_HD uint32_t gated_reduce_word(const uint32_t* w, const float* g, int k) {
  float lo = g[0] * reduce_bits_to_f32(w[0] << 16);
  float hi = g[0] * reduce_bits_to_f32(w[0] & 0xFFFF0000u);
  for (int i = 1; i < k; ++i) {
    lo = lo + g[i] * reduce_bits_to_f32(w[i] << 16);
    hi = hi + g[i] * reduce_bits_to_f32(w[i] & 0xFFFF0000u);
  }
  return reduce_pack_bf16(lo, hi);
}

// Host side (transport_host.cpp): out = the gated sum of the k (1..8) operand
// buffers of `bytes` (whole rows of row_elems bf16) under the table `gate`
// (gate_rows() entries); out may be operand 0.  Any alignment.
void host_gated_reduce(void* out, const void* const* operands, int k, size_t bytes, const void* gate, size_t row_elems);
// The table of `rows` entries from stream `seed`.
void host_fill_gate(void* p, size_t rows, uint64_t seed);
// Compares p with the gated sum of the operand streams `seeds` (operand order) under the table of `gate_seed`.
VerifyResult host_verify_gated_reduced(const void* p, size_t bytes, const uint64_t* seeds, int nseeds, uint64_t gate_seed,
                                       size_t row_elems);

}  // namespace p2p
