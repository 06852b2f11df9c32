// Block-scaled wire formats (--wire): bf16 payloads that cross the link as OCP
// microscaling ("MX") elements, 8-bit e4m3, 6-bit e2m3 or 4-bit e2m1, with one shared
// power-of-two scale (an E8M0 byte) per block of 32 elements, and are widened
// back to bf16 by the receiver.  Shared by the gfx950 pack / unpack / verify
// kernels (wire.hip), the host transport and the host-side regeneration of
// expected values, so all of them produce the same bits.
//
// Payload.  bf16 elements; a block is 32 consecutive elements (64 B), so a
// payload is a multiple of 64 B.
//
// Operands.  wire_operand_word() keeps sign and mantissa of both halves of a
// PRNG word and sets each half's exponent field to
//   64 + (block index & 31) + (the low 4 bits of the half's own exponent field),
// a finite normal bf16 with exponent field in [64, 110].  Blocks walk over 32
// binades (every scale byte of that span occurs); inside a block the elements
// spread over 16 binades, which reaches e4m3's subnormals and zero, and
// e2m1's subnormal and zero often.
//
// Scale, the no-clip rule.  With the block's amax = 1.m x 2^E (the magnitude
// order of bf16 is the integer order of bits & 0x7FFF) the scale is 2^e, the
// smallest power of two under which no element exceeds the format's maximum:
//   e4m3 (max 448 = 1.75 x 2^8):  e = E - 8 if 1.m <= 1.75, else E - 7;
//   e2m3 (max 7.5 = 1.875 x 2^2): e = E - 2 if 1.m <= 1.875, else E - 1;
//   e2m1 (max   6 = 1.5  x 2^2):  e = E - 2 if 1.m <= 1.5,  else E - 1.
// Nothing saturates, so what a conversion does on overflow cannot change a
// bit.  The scale byte is e + 127 clamped to [1, 254]; amax = 0 gives 127.
//
// Elements.  q = x / 2^e rounded to nearest even onto the format's grid, its
// subnormals included (steps of 2^-9 below 2^-6 for e4m3, of 0.125 below 1
// for e2m3, of 0.5 below 1 for e2m1); the sign is kept (-0 stays -0).  No
// format here has an Inf; e2m3 and e2m1 have no NaN either.  Element j of a
// block occupies bits bj .. bj + b - 1 (b = 8, 6 or 4 code bits) of the
// block's element bytes read as one little-endian integer: mxfp8: element j
// is byte j; mxfp4: element 2j is the low nibble of byte j; mxfp6: four
// elements share three bytes.  That is the order in which
// v_cvt_scalef32_pk32_*_fp6 reads and writes its 6 VGPRs (VGPR 0 is the
// lowest 32 bits), settled on a GPU by scripts/wire_cvt_probe.hip
// (docs/DESIGN.md).
//
// Unpacking is exact: a 4- or 2-bit significand times a power of two is a
// normal bf16 for every scale byte the operand map can produce.  NaN, Inf and
// bf16 subnormal inputs and the scale bytes 0 and 255 are outside the
// contract (the functions below stay defined on them, nothing more).
//
// Wire image of n payload bytes: tiles of up to 128 blocks (8 KiB of payload).
// A tile of nb blocks is nb x EB element bytes (EB = 32 for mxfp8, 24 for
// mxfp6, 16 for mxfp4) and zeros up to a multiple of 16 B (only an odd count
// of 24 B blocks leaves any: 8 B), then nb scale bytes, then zeros up to a
// multiple of 16 B: a full tile is 4224 B (mxfp8, 0.516 of the payload),
// 3200 B (mxfp6, 0.391) or 2176 B (mxfp4, 0.266).
// Every tile and every scale section starts 16 B aligned.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "prng.hpp"

namespace p2p {

enum class WireFormat : int { Off = 0, Mxfp8 = 1, Mxfp4 = 2, Mxfp6 = 3 };

// What tells the formats apart; everything below is written over it, so a
// further element type (e3m2, say) is one more row.
struct WireTraits {
  int bits;      // code bits of an element, the sign on top
  int mbits;     // stored mantissa bits
  int emin;      // exponent of the smallest normal
  int bias;      // exponent bias
  int emax;      // exponent of the largest value
  uint32_t max_mant;  // bf16 mantissa field (7 bits) of the largest value's significand
  uint32_t top;       // the largest finite magnitude code
};
P2P_HD constexpr WireTraits wire_traits(WireFormat f) {
  return f == WireFormat::Mxfp4   ? WireTraits{4, 1, 0, 1, 2, 0x40u, 7u}
         : f == WireFormat::Mxfp6 ? WireTraits{6, 3, 0, 1, 2, 0x70u, 0x1Fu}
                                  : WireTraits{8, 3, -6, 7, 8, 0x60u, 0x7Eu};
}
P2P_HD constexpr bool wire_format_valid(WireFormat f) {
  return f == WireFormat::Mxfp8 || f == WireFormat::Mxfp4 || f == WireFormat::Mxfp6;
}
constexpr const char* kWireFormatList = "mxfp8, mxfp6 or mxfp4";

constexpr uint32_t kWireBlockElems = 32;
constexpr uint32_t kWireBlockBytes = 64;   // payload bytes of a block
constexpr uint32_t kWireTileBlocks = 128;  // blocks of a full tile
constexpr uint32_t kWireTilePayload = kWireTileBlocks * kWireBlockBytes;  // 8 KiB

inline const char* wire_format_name(WireFormat f) {
  return f == WireFormat::Mxfp8 ? "mxfp8" : f == WireFormat::Mxfp6 ? "mxfp6" : f == WireFormat::Mxfp4 ? "mxfp4" : "off";
}
// "mxfp8" | "mxfp6" | "mxfp4" (and "off"); false for anything else.
inline bool parse_wire_format(const std::string& s, WireFormat* f) {
  for (WireFormat c : {WireFormat::Off, WireFormat::Mxfp8, WireFormat::Mxfp4, WireFormat::Mxfp6})
    if (s == wire_format_name(c)) {
      *f = c;
      return true;
    }
  return false;
}

// Element bytes of one block.
P2P_HD constexpr uint32_t wire_block_elem_bytes(WireFormat f) { return 4u * static_cast<uint32_t>(wire_traits(f).bits); }
// Where the scale bytes of a tile of nb blocks begin: behind the element
// section, padded to 16 B.
P2P_HD constexpr uint32_t wire_tile_scale_offset(uint32_t nb, WireFormat f) {
  return (nb * wire_block_elem_bytes(f) + 15u) & ~15u;
}
// Bytes of a tile of nb blocks: the element section, scale bytes, padding to 16 B.
P2P_HD constexpr uint32_t wire_tile_bytes(uint32_t nb, WireFormat f) {
  return (wire_tile_scale_offset(nb, f) + nb + 15u) & ~15u;
}
// The wire image's size for n payload bytes (a multiple of 64).
P2P_HD constexpr uint64_t wire_bytes(uint64_t n, WireFormat f) {
  const uint64_t blocks = n / kWireBlockBytes;
  return blocks / kWireTileBlocks * wire_tile_bytes(kWireTileBlocks, f) +
         wire_tile_bytes(static_cast<uint32_t>(blocks % kWireTileBlocks), f);
}

// One bf16 half: sign and mantissa kept, exponent field pinned by the block.
P2P_HD uint32_t wire_operand_half(uint32_t h, uint32_t block) {
  return (h & 0x807Fu) | ((64u + (block & 31u) + ((h >> 7) & 15u)) << 7);
}
// Word `word_index` of a payload (two elements; 16 words are a block).
P2P_HD uint32_t wire_operand_word(uint32_t w, uint64_t word_index) {
  const uint32_t block = static_cast<uint32_t>(word_index >> 4);
  return wire_operand_half(w & 0xFFFFu, block) | (wire_operand_half(w >> 16, block) << 16);
}

// The E8M0 byte of a block whose largest magnitude is `amax` (bits & 0x7FFF).
P2P_HD uint32_t wire_scale_byte(uint32_t amax, WireFormat f) {
  if (amax == 0) return 127u;
  const int E = static_cast<int>(amax >> 7), m = static_cast<int>(amax & 0x7Fu);
  const WireTraits t = wire_traits(f);
  const int b = E - t.emax + (m > static_cast<int>(t.max_mant));
  return static_cast<uint32_t>(b < 1 ? 1 : b > 254 ? 254 : b);
}

// bf16 bits -> the element's code (8, 6 or 4 bits) under scale byte sb.
P2P_HD uint32_t wire_quantize(uint32_t x, uint32_t sb, WireFormat f) {
  const WireTraits t = wire_traits(f);
  const int mbits = t.mbits, emin = t.emin;
  const uint32_t top = t.top;
  const uint32_t sign = (x >> 15) & 1u;
  const int ex = static_cast<int>((x >> 7) & 0xFFu);
  uint32_t code = 0;
  if (ex != 0) {  // a bf16 subnormal or zero quantises to zero
    const uint32_t s = 128u + (x & 0x7Fu);  // 1.7 significand
    const int k = ex - static_cast<int>(sb);  // q = s / 128 x 2^k
    const int shift = 7 - mbits + (k < emin ? emin - k : 0);
    uint32_t r = 0;
    if (shift <= 9) {  // beyond: below half of the smallest step
      r = s >> shift;
      const uint32_t rest = s & ((1u << shift) - 1u), half = 1u << (shift - 1);
      r += (rest > half) || (rest == half && (r & 1u));
    }
    code = r + (k >= emin ? static_cast<uint32_t>(k - emin) << mbits : 0u);  // a carry steps the exponent
    if (code > top) code = top;  // outside the contract: the no-clip scale never gets here
  }
  return code | (sign << (t.bits - 1));
}

// The element's code under scale byte sb -> bf16 bits, exact inside the contract.
P2P_HD uint32_t wire_dequantize(uint32_t code, uint32_t sb, WireFormat f) {
  const WireTraits t = wire_traits(f);
  const int mbits = t.mbits, bias = t.bias;
  const uint32_t sign = (code >> (t.bits - 1)) & 1u;
  const uint32_t mag = code & ((1u << (t.bits - 1)) - 1u);
  uint32_t out = 0;
  if (mag) {
    int e = static_cast<int>(mag >> mbits);
    uint32_t m = mag & ((1u << mbits) - 1u);
    if (e == 0) {  // the format's subnormal: normalise
      e = 1;
      while (!(m >> mbits)) {
        m <<= 1;
        --e;
      }
      m &= (1u << mbits) - 1u;
    }
    out = ((static_cast<uint32_t>(e - bias + static_cast<int>(sb)) & 0xFFu) << 7) | (m << (7 - mbits));
  }
  return out | (sign << 15);
}

// One block: 32 bf16 (as bits) -> wire_block_elem_bytes element bytes and the scale byte.
P2P_HD void wire_pack_block(const uint16_t* x, uint8_t* elems, uint8_t* scale, WireFormat f) {
  uint32_t amax = 0;
  for (uint32_t j = 0; j < kWireBlockElems; ++j) amax = amax > (x[j] & 0x7FFFu) ? amax : (x[j] & 0x7FFFu);
  const uint32_t sb = wire_scale_byte(amax, f);
  *scale = static_cast<uint8_t>(sb);
  // Codes enter a little-endian bit stream, whole bytes leave it.
  const uint32_t bits = static_cast<uint32_t>(wire_traits(f).bits);
  uint32_t acc = 0, have = 0;
  for (uint32_t j = 0; j < kWireBlockElems; ++j) {
    acc |= wire_quantize(x[j], sb, f) << have;
    for (have += bits; have >= 8; have -= 8, acc >>= 8) *elems++ = static_cast<uint8_t>(acc);
  }
}

P2P_HD void wire_unpack_block(const uint8_t* elems, uint8_t scale, uint16_t* x, WireFormat f) {
  const uint32_t bits = static_cast<uint32_t>(wire_traits(f).bits);
  uint32_t acc = 0, have = 0;
  for (uint32_t j = 0; j < kWireBlockElems; ++j) {
    for (; have < bits; have += 8) acc |= static_cast<uint32_t>(*elems++) << have;
    x[j] = static_cast<uint16_t>(wire_dequantize(acc & ((1u << bits) - 1u), scale, f));
    acc >>= bits, have -= bits;
  }
}

// What the receiver holds for a word of the sender's operand stream: both
// halves quantised under the block's scale byte and widened again.
P2P_HD uint32_t wire_roundtrip_word(uint32_t w, uint32_t sb, WireFormat f) {
  return wire_dequantize(wire_quantize(w & 0xFFFFu, sb, f), sb, f) |
         (wire_dequantize(wire_quantize(w >> 16, sb, f), sb, f) << 16);
}

// Host side (transport_host.cpp).  n is the payload size, a multiple of 64.
// wire: wire_bytes(n, f) bytes; payload: n bytes.  Any alignment.
void host_wire_pack(void* wire, const void* payload, size_t n, WireFormat f);
void host_wire_unpack(void* payload, const void* wire, size_t n, WireFormat f);
// The wire image of operand stream `seed`.
void host_fill_packed(void* wire, size_t n, uint64_t seed, WireFormat f);
// Regenerates the operand stream, packs and unpacks it, compares 32-bit words with p.
VerifyResult host_verify_unpacked(const void* p, size_t n, uint64_t seed, WireFormat f);

}  // namespace p2p
