// Receive-and-reduce of block-scaled operands (--reduce-wire): every operand of
// a receiver's sum is an MXFP8 / MXFP6 / MXFP4 wire image (wire_op.hpp: format, tiles,
// scale rule), the sum leaves as bf16.  Shared by the gfx950 kernels
// (wire_reduce.hip), the host transport and the host-side regeneration of
// expected values, so all of them produce the same bits.  Nothing new is
// computed here: the function below composes wire_op.hpp and reduce_op.hpp.
//
// Arithmetic.  An element is dequantised to f32 (exactly a bf16 value: a 4- or
// 2-bit significand times a power of two), the K operands are added in operand
// order (operand 0 is the receiver's own image, then the incoming ones as
// posted) in a chain of plain f32 adds, and the sum is rounded once, to
// nearest even, to bf16.  That is reduce_word with ReduceType::Bf16 over the
// widened words.
//
// Range.  Operand exponent fields lie in [64, 110] (wire_operand_word), so a
// block's scale byte is >= 64 - 8 = 56 (mxfp8) or >= 64 - 2 = 62 (mxfp4) and
// <= 110 - 1.  The smallest non-zero dequantised magnitude is e4m3's smallest
// subnormal under the smallest scale, 2^-9 x 2^(56 - 127) = 2^-80 (mxfp4:
// 0.5 x 2^(62 - 127) = 2^-66); every operand and every partial sum is a
// multiple of it, so a non-zero partial sum is at least 2^-80, far above f32's
// subnormal range (< 2^-126).  The largest operand is below 2^9 x 2^(109 - 127)
// = 2^-9, and kMaxWireReduceSrcs = 8 of them stay below 2^-6: nothing
// overflows.  No add produces or consumes a subnormal, so the device's
// denormal mode cannot change a bit, and the single bf16 rounding sees a
// normal f32 or a zero.  mxfp6 (e2m3) has mxfp4's exponent range: its scale
// byte is >= 64 - 2 = 62 and <= 109, its smallest non-zero magnitude is the
// subnormal step 0.125 x 2^(62 - 127) = 2^-68, every partial sum a multiple of
// it, and its largest operand 7.5 x 2^(109 - 127) < 2^-15, so eight of them
// stay below 2^-12: the same argument holds with room to spare.
//
// A bf16 own shard (own_bf16, --reduce-own bf16).  A real receiver holds its
// local shard in bf16 and only what arrives is quantised: operand 0 is then the
// raw word of the receiver's operand stream (wire_operand_word), operands
// 1..K-1 stay round-tripped images.  Chain, order and the one rounding are the
// same.  Range: the own operand's exponent field lies in [64, 110], so its
// magnitude is at least 2^(64 - 127) = 2^-63 with a 7-bit significand, a
// multiple of 2^-70 and therefore of every granule above (2^-80, 2^-68,
// 2^-66): partial sums stay multiples of the old granule and a non-zero one is
// still at least 2^-80.  It is below 2^(111 - 127) = 2^-16, so own + 7 incoming
// is below 2^-16 + 7 x 2^-9 < 2^-6, the bound that held for eight images.  No
// subnormal, no overflow, and the sum's range [2^-80, 2^-6) is the one the
// requantised output's argument below starts from: its scale-byte clamp still
// never acts.  K = 1 is a copy of the own shard (widening a normal bf16 to f32
// and rounding it back is exact, zeros keep their sign), or its pack.
//
// Zeros are real operands here, unlike in reduce_op.hpp: the codes 0x00 / 0x80
// (mxfp8), 0x00 / 0x20 (mxfp6) and 0x0 / 0x8 (mxfp4) occur, and the sign of a zero is kept by the
// dequantisation.  Signed zeros follow IEEE addition in round-to-nearest:
// (+0) + (-0) = +0, (-0) + (-0) = -0, and an exact cancellation x + (-x) gives
// +0.  A single operand passes through with its sign.  reduce_pack_bf16 keeps
// the sign of a zero on both sides: v_cvt_pk_bf16_f32 maps +-0 to +-0, and the
// host's integer form adds 0x7FFF to 0x00000000 / 0x80000000, which carries
// nothing into the upper half, so 0x0000 / 0x8000 come out.
//
// Requantised output (--reduce-out wire).  The output image of a hop that
// forwards low precision is, by definition, wire_pack_block (same format as the
// operands) of the bf16 sum above: the f32 chain is rounded once to bf16, and
// that bf16 value is quantised under the no-clip scale of the block's bf16
// amax.  No new rounding rule, and not a quantisation of the f32 sum: going
// through bf16 makes the image bit-identical to packing the bf16 output, so a
// chain of hops stays checkable.  Range: a non-zero sum lies in [2^-80, 2^-6),
// so its bf16 rounding is zero or normal with exponent field in about
// [47, 121] (rounding up can carry into the next binade, never further).  The
// scale byte is then within [47 - 8, 121 - 1]: wire_scale_byte's clamp to
// [1, 254] never acts.  A block whose sums are all zero (either sign) has
// amax 0 and scale byte 127.  wire_quantize keeps the sign bit whatever the
// magnitude, so a -0 sum is the code 0x80 / 0x8.  A block of sums may span
// more binades than an operand block (16): cancellation leaves small sums next
// to large ones, so the format's subnormals and zeros get more frequent under
// the block's scale; wire_quantize covers those (its contract asks only for a
// zero or normal bf16 and a quotient inside the format, which the no-clip
// scale guarantees).  mxfp6 (e2m3): the sum's range is the one argued above,
// bf16 exponent fields in about [47, 121], and e2m3's scale-byte rule is E - 2
// (significand <= 1.875) or E - 1, so the byte lies within [45, 120] and the
// clamp never acts here either.  A -0 sum gives the code 0x20, which widens
// back to -0 under any scale byte.
//
// Both outputs (--reduce-out both).  The bf16 output beside that image is
// wire_unpack of it: wire_roundtrip_word of every sum word under the block's
// scale byte.  Unpacking is exact (wire_op.hpp), so nothing is rounded again.
#pragma once

#include <cstddef>
#include <cstdint>

#include "reduce_op.hpp"
#include "wire_op.hpp"

namespace p2p {

constexpr int kMaxWireReduceSrcs = 8;  // operands of one sum: the own image and up to 7 incoming

// One 32-bit word (two elements) of the sum.  w[k] is operand k's word of its
// operand stream (wire_operand_word), sb[k] the scale byte of the block that
// word lies in; k in 1..kMaxWireReduceSrcs.  own_bf16: operand 0 enters as it
// is, not as its image (sb[0] is not read).
P2P_HD uint32_t wire_reduce_word(const uint32_t* w, const uint32_t* sb, int k, WireFormat f, bool own_bf16 = false) {
  ReduceAcc a = reduce_begin(own_bf16 ? w[0] : wire_roundtrip_word(w[0], sb[0], f), ReduceType::Bf16);
  for (int i = 1; i < k; ++i) reduce_add(a, wire_roundtrip_word(w[i], sb[i], f), ReduceType::Bf16);
  return reduce_finish(a, ReduceType::Bf16);
}

// Host side (transport_host.cpp).  n is the payload size, a multiple of 64.
// out: n bytes of bf16 = the sum of the k wire images (wire_bytes(n, f) each)
// in order.  Any alignment.  own_bf16: images[0] is n bytes of bf16, the
// receiver's own shard, not an image.
void host_wire_reduce(void* out, const void* const* images, int k, size_t n, WireFormat f, bool own_bf16 = false);
// Compares p with the sum of the operand streams `seeds` (operand order), each
// packed and unpacked by the shared functions (own_bf16: all but the first); a
// wrong 32-bit word counts once.  roundtrip: p is the bf16 output of
// --reduce-out both, the sum's words under wire_roundtrip_word with the scale
// byte of the block's sums.
VerifyResult host_verify_wire_reduced(const void* p, size_t n, const uint64_t* seeds, int nseeds, WireFormat f,
                                      bool own_bf16 = false, bool roundtrip = false);
// n bytes of bf16: operand stream `seed` as a receiver holds its own shard.
void host_fill_wire_operand(void* p, size_t n, uint64_t seed);

// ---- requantised output (--reduce-out wire) ----
// The largest magnitude (bits & 0x7FFF) of the two bf16 halves of a sum word.
P2P_HD uint32_t wire_word_amax(uint32_t w) {
  const uint32_t lo = w & 0x7FFFu, hi = (w >> 16) & 0x7FFFu;
  return lo > hi ? lo : hi;
}
// The codes of two sum words (4 elements, mxfp8: one word of 4 bytes) or of
// four (8 elements, mxfp4: one word of 8 nibbles) under the block's scale byte.
P2P_HD uint32_t wire_code_word(const uint32_t* w, uint32_t sb, WireFormat f) {
  const int nw = f == WireFormat::Mxfp4 ? 4 : 2, bits = f == WireFormat::Mxfp4 ? 4 : 8;
  uint32_t out = 0;
  for (int i = 0; i < nw; ++i)
    out |= (wire_quantize(w[i] & 0xFFFFu, sb, f) | (wire_quantize(w[i] >> 16, sb, f) << bits)) << (2 * bits * i);
  return out;
}
// mxfp6: the codes of four sum words (8 elements) under the block's scale byte,
// 48 bits = the 6 bytes they occupy in the block's 24, element 0 lowest.
P2P_HD uint64_t wire_code_bits6(const uint32_t* w, uint32_t sb) {
  uint64_t out = 0;
  for (int i = 0; i < 4; ++i) {
    const uint64_t lo = wire_quantize(w[i] & 0xFFFFu, sb, WireFormat::Mxfp6), hi = wire_quantize(w[i] >> 16, sb, WireFormat::Mxfp6);
    out |= (lo | (hi << 6)) << (12 * i);
  }
  return out;
}
// out_image: wire_bytes(n, f) bytes = the wire image (padding zeroed) of the
// sum host_wire_reduce gives for the k images.  Any alignment.
void host_wire_reduce_packed(void* out_image, const void* const* images, int k, size_t n, WireFormat f, bool own_bf16 = false);
// Compares `image` with the packed sum of the operand streams `seeds`: a wrong
// 32-bit word of element codes counts once, a wrong scale byte once, first_bad
// is the lowest byte offset in the image of either, the checksum is the sum
// of the code words and the scale bytes.  The padding is not read.  mxfp6: the
// unit is the 6 bytes of 8 codes (wire_code_bits6), four a block.
VerifyResult host_verify_wire_reduced_packed(const void* image, size_t n, const uint64_t* seeds, int nseeds, WireFormat f,
                                             bool own_bf16 = false);

}  // namespace p2p
