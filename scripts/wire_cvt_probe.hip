// Do the gfx950 scaled conversion instructions agree with csrc/wire_op.hpp?  Stand-alone:
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -Icsrc scripts/wire_cvt_probe.hip -o build/wire_cvt_probe
// Narrowing: every normal bf16 under every scale byte for which the quotient is inside the
// format, with the scale operand 2^e (divides) and 2^-e (multiplies); widening: every code under
// every scale byte with a normal result.  Prints the mismatch counts and a few examples.
// The 6-bit block instructions (pk32: 32 elements, 6 VGPRs of codes) are probed with the value
// under test at a varying element position among 31 markers, which also settles their register
// layout: element j in bits 6j .. 6j + 5 of the 6 VGPRs read as one little-endian integer.
#include <hip/hip_runtime.h>
#include <cstdio>
#include "wire_op.hpp"
using namespace p2p;
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));

typedef unsigned int u32x6 __attribute__((ext_vector_type(6)));
typedef unsigned int u32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x32 __attribute__((ext_vector_type(32)));
typedef float f32x32 __attribute__((ext_vector_type(32)));
typedef unsigned int u32x32 __attribute__((ext_vector_type(32)));

struct Out6 {
  unsigned long long nbad[2], ntotal;      // narrow: [mode]
  unsigned long long wbad[2], wtotal;      // widen: [0: to bf16, 1: to f32]
  unsigned int nex[8][4], nnex, wex[8][4], wnex;
};

__device__ void put_code(u32x6& c, unsigned pos, unsigned code) {
  const unsigned bit = 6 * pos, w = bit >> 5, sh = bit & 31;
  c[w] = (c[w] & ~(0x3Fu << sh)) | (code << sh);
  if (sh > 26) c[w + 1] = (c[w + 1] & ~(0x3Fu >> (32 - sh))) | (code >> (32 - sh));
}
__device__ unsigned get_code(const u32x6& c, unsigned pos) {
  const unsigned bit = 6 * pos, w = bit >> 5, sh = bit & 31;
  unsigned v = c[w] >> sh;
  if (sh > 26) v |= c[w + 1] << (32 - sh);
  return v & 0x3Fu;
}

__global__ void narrow6_probe(Out6* o) {
  const unsigned gid = blockIdx.x * blockDim.x + threadIdx.x;  // x (16 bits) | sb (8 bits) << 16
  const unsigned x = gid & 0xFFFF, sb = gid >> 16;
  if (sb < 1 || sb > 254) return;
  const int ex = (x >> 7) & 0xFF, m = x & 0x7F;
  if (ex == 255 || (ex == 0 && m)) return;  // zero or normal
  const int k = ex - (int)sb;
  if (ex && (!(k < 2 || (k == 2 && m <= 0x70)) || k < -40)) return;
  const unsigned want = wire_quantize(x, sb, WireFormat::Mxfp6), pos = (x ^ (x >> 5) ^ sb) & 31;
  atomicAdd(&o->ntotal, 1ull);
  for (int mode = 0; mode < 2; ++mode) {
    const float scale = __builtin_bit_cast(float, (mode ? 254u - sb : sb) << 23);
    u32x16 w;
    for (int i = 0; i < 16; ++i) w[i] = 0;  // markers: +0 everywhere else
    w[pos >> 1] = x << (16 * (pos & 1));
    const u32x6 c = __builtin_amdgcn_cvt_scalef32_pk32_fp6_bf16(__builtin_bit_cast(bf16x32, w), scale);
    bool ok = true;
    for (unsigned j = 0; j < 32; ++j) ok = ok && get_code(c, j) == (j == pos ? want : 0u);
    if (!ok) {
      atomicAdd(&o->nbad[mode], 1ull);
      if (mode == 0) {
        const unsigned n = atomicAdd(&o->nnex, 1u);
        if (n < 8) { o->nex[n][0] = x; o->nex[n][1] = sb; o->nex[n][2] = get_code(c, pos); o->nex[n][3] = want; }
      }
    }
  }
}

__global__ void widen6_probe(Out6* o) {
  const unsigned gid = blockIdx.x * blockDim.x + threadIdx.x;  // code (6 bits) | pos (5 bits) << 6 | sb << 11
  const unsigned code = gid & 63, pos = (gid >> 6) & 31, sb = gid >> 11;
  if (sb < 4 || sb > 252) return;  // every result a normal bf16: 0.125 x 2^(sb-127) .. 7.5 x 2^(sb-127)
  const float scale = __builtin_bit_cast(float, sb << 23);
  const unsigned want = wire_dequantize(code, sb, WireFormat::Mxfp6), marker = sb << 7;  // code 0x08 is 1.0
  u32x6 c;
  for (int i = 0; i < 6; ++i) c[i] = 0;
  for (unsigned j = 0; j < 32; ++j) put_code(c, j, j == pos ? code : 0x08u);
  const u32x16 b = __builtin_bit_cast(u32x16, __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(c, scale));
  const u32x32 f = __builtin_bit_cast(u32x32, __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(c, scale));
  unsigned diffb = 0, difff = 0;  // or of the differences: one compare at the end
  for (unsigned j = 0; j < 32; ++j) {
    const unsigned w = j == pos ? want : marker;
    diffb |= ((b[j >> 1] >> (16 * (j & 1))) & 0xFFFFu) ^ w;
    difff |= f[j] ^ (w << 16);
  }
  const bool okb = diffb == 0, okf = difff == 0;
  atomicAdd(&o->wtotal, 1ull);
  if (!okb) atomicAdd(&o->wbad[0], 1ull);
  if (!okf) atomicAdd(&o->wbad[1], 1ull);
  if (!okb || !okf) {
    const unsigned n = atomicAdd(&o->wnex, 1u);
    if (n < 8) { o->wex[n][0] = code | pos << 8; o->wex[n][1] = sb; o->wex[n][2] = (b[pos >> 1] >> (16 * (pos & 1))) & 0xFFFFu; o->wex[n][3] = want; }
  }
}

struct Out {
  unsigned long long bad[8];  // [fmt*4 + mode*2 + subnormal]
  unsigned long long total[2];
  unsigned int ex[8][8][4];
  unsigned int nex[8];
  unsigned long long wbad[2], wtotal[2];
  unsigned int wex[2][8][4];
  unsigned int wnex[2];
};

__global__ void narrow_probe(Out* o) {
  const unsigned gid = blockIdx.x * blockDim.x + threadIdx.x;  // x (16 bits) | sb (8 bits) << 16
  const unsigned x = gid & 0xFFFF, sb = gid >> 16;
  if (sb < 1 || sb > 254) return;
  const int ex = (x >> 7) & 0xFF, m = x & 0x7F;
  if (ex == 0 || ex == 255) return;
  const int k = ex - (int)sb;
  for (int fi = 0; fi < 2; ++fi) {
    const WireFormat f = fi ? WireFormat::Mxfp4 : WireFormat::Mxfp8;
    const bool ok = fi ? (k < 2 || (k == 2 && m <= 0x40)) : (k < 8 || (k == 8 && m <= 0x60));
    if (!ok || k < -40) continue;
    const unsigned want = wire_quantize(x, sb, f);
    atomicAdd(&o->total[fi], 1ull);
    for (int mode = 0; mode < 2; ++mode) {
      const float scale = __builtin_bit_cast(float, (mode ? 254u - sb : sb) << 23);
      const bf16x2 v = __builtin_bit_cast(bf16x2, x | (0x3F80u << 16));  // .y = 1.0
      unsigned got;
      if (fi == 0) {
        i16x2 r = {0, 0};
        r = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(r, v, scale, false);
        got = __builtin_bit_cast(unsigned, r) & 0xFF;
      } else {
        got = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(0u, v, scale, 0) & 0xF;
      }
      if (got != want) {
        const int sub = fi ? k < 0 : k < -6;
        const int c = fi * 4 + mode * 2 + sub;
        atomicAdd(&o->bad[c], 1ull);
        const unsigned n = atomicAdd(&o->nex[c], 1u);
        if (n < 8) { o->ex[c][n][0] = x; o->ex[c][n][1] = sb; o->ex[c][n][2] = got; o->ex[c][n][3] = want; }
      }
    }
  }
}

__global__ void widen_probe(Out* o) {
  const unsigned gid = blockIdx.x * blockDim.x + threadIdx.x;  // code | sb << 8
  const unsigned code = gid & 0xFF, sb = gid >> 8;
  if (sb < 1 || sb > 254) return;
  const float scale = __builtin_bit_cast(float, sb << 23);
  for (int fi = 0; fi < 2; ++fi) {
    const WireFormat f = fi ? WireFormat::Mxfp4 : WireFormat::Mxfp8;
    if (fi && code > 15) continue;
    if (!fi && (code & 0x7F) == 0x7F) continue;
    const unsigned want = wire_dequantize(code, sb, f);
    const int e = (want >> 7) & 0xFF;
    // inside the contract: a normal bf16 (or zero); recompute the exponent without the mask
    const int mb = fi ? 1 : 3, bias = fi ? 1 : 7;
    const unsigned mag = code & (fi ? 7u : 0x7Fu);
    int ee = (int)(mag >> mb);
    if (mag && ee == 0) { unsigned mm = mag; ee = 1; while (!(mm >> mb)) { mm <<= 1; --ee; } }
    const int field = ee - bias + (int)sb;
    if (mag && (field < 1 || field > 254)) continue;
    (void)e;
    // element 0 = code, element 1 = a marker (code 0x38 = 1.0 for fp8, 2 = 1.0 for fp4)
    unsigned got, got1;
    if (fi == 0) {
      const bf16x2 r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(code | (0x38u << 8), scale, false);
      got = __builtin_bit_cast(unsigned, r) & 0xFFFF;
      got1 = __builtin_bit_cast(unsigned, r) >> 16;
    } else {
      const bf16x2 r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(code | (0x2u << 4), scale, 0);
      got = __builtin_bit_cast(unsigned, r) & 0xFFFF;
      got1 = __builtin_bit_cast(unsigned, r) >> 16;
    }
    atomicAdd(&o->wtotal[fi], 1ull);
    const unsigned want1 = sb << 7;  // 1.0 x 2^(sb-127)
    if (got != want || got1 != want1) {
      atomicAdd(&o->wbad[fi], 1ull);
      const unsigned n = atomicAdd(&o->wnex[fi], 1u);
      if (n < 8) { o->wex[fi][n][0] = code; o->wex[fi][n][1] = sb; o->wex[fi][n][2] = got | got1 << 16; o->wex[fi][n][3] = want | want1 << 16; }
    }
  }
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

int main() {
  Out* d;
  CK(hipMalloc(&d, sizeof(Out)));
  CK(hipMemset(d, 0, sizeof(Out)));
  narrow_probe<<<(65536 * 256) / 256, 256>>>(d);
  widen_probe<<<(256 * 256) / 256, 256>>>(d);
  CK(hipDeviceSynchronize());
  Out h;
  CK(hipMemcpy(&h, d, sizeof(Out), hipMemcpyDeviceToHost));
  const char* fmt[2] = {"mxfp8", "mxfp4"};
  const char* mode[2] = {"scale=2^e (divides)", "scale=2^-e (multiplies)"};
  for (int fi = 0; fi < 2; ++fi) {
    printf("narrow %s: %llu in-contract inputs\n", fmt[fi], h.total[fi]);
    for (int m = 0; m < 2; ++m)
      for (int s = 0; s < 2; ++s) {
        const int c = fi * 4 + m * 2 + s;
        printf("  %-26s %-10s mismatches %llu\n", mode[m], s ? "subnormal" : "normal", h.bad[c]);
        for (unsigned n = 0; n < (h.nex[c] < 8 ? h.nex[c] : 8) && m == 0; ++n)
          printf("    x=%04x sb=%u got=%02x want=%02x\n", h.ex[c][n][0], h.ex[c][n][1], h.ex[c][n][2], h.ex[c][n][3]);
      }
    printf("widen %s: %llu inputs, mismatches %llu\n", fmt[fi], h.wtotal[fi], h.wbad[fi]);
    for (unsigned n = 0; n < (h.wnex[fi] < 8 ? h.wnex[fi] : 8); ++n)
      printf("    code=%02x sb=%u got=%08x want=%08x\n", h.wex[fi][n][0], h.wex[fi][n][1], h.wex[fi][n][2], h.wex[fi][n][3]);
  }
  Out6* d6;
  CK(hipMalloc(&d6, sizeof(Out6)));
  CK(hipMemset(d6, 0, sizeof(Out6)));
  narrow6_probe<<<(65536 * 256) / 256, 256>>>(d6);
  widen6_probe<<<(64 * 32 * 256) / 256, 256>>>(d6);
  CK(hipDeviceSynchronize());
  Out6 h6;
  CK(hipMemcpy(&h6, d6, sizeof(Out6), hipMemcpyDeviceToHost));
  printf("narrow mxfp6 (pk32_fp6_bf16, value at a varying element, zeros elsewhere): %llu in-contract inputs\n", h6.ntotal);
  for (int m = 0; m < 2; ++m) printf("  %-26s mismatches %llu\n", mode[m], h6.nbad[m]);
  for (unsigned n = 0; n < (h6.nnex < 8 ? h6.nnex : 8); ++n)
    printf("    x=%04x sb=%u got=%02x want=%02x\n", h6.nex[n][0], h6.nex[n][1], h6.nex[n][2], h6.nex[n][3]);
  printf("widen mxfp6 (every code x element position x scale byte 4..252): %llu inputs, mismatches pk32_bf16_fp6 %llu, pk32_f32_fp6 %llu\n",
         h6.wtotal, h6.wbad[0], h6.wbad[1]);
  for (unsigned n = 0; n < (h6.wnex < 8 ? h6.wnex : 8); ++n)
    printf("    code=%02x pos=%u sb=%u got=%04x want=%04x\n", h6.wex[n][0] & 0xFF, h6.wex[n][0] >> 8, h6.wex[n][1], h6.wex[n][2], h6.wex[n][3]);
  printf("mxfp6 register layout (element j in bits 6j..6j+5, VGPR 0 lowest): %s\n",
         h6.nbad[0] == 0 && h6.wbad[0] == 0 && h6.wbad[1] == 0 ? "confirmed" : "NOT confirmed");
  return 0;
}
