// gfx950 gated receive-and-reduce kernels (--reduce-gate H): the expert
// combine's y[r] = sum_k g[r][k] * x_k[r] in the pull engine's one launch, the
// gate table's fill and the check of a gated sum.  kernels.hpp has the
// contract, reduce_gate_op.hpp the arithmetic.  Design:
//   * The unit of work is a wave's 1 KiB (64 lanes x 16 B), not a block's 4 KiB:
//     a row is a multiple of 1 KiB and an op starts at a row, so a wave's chunk
//     lies in exactly one row whether rows straddle 4 KiB blocks (H = 1536) or
//     a block holds several (H = 512).  The chunk index is made wave-uniform
//     with a read-first-lane, the row is one 32-bit division on it, and the
//     row's 16 B gate entry is one load from the constant address space through
//     the scalar data cache: 4 SGPRs per wave and chunk, no VGPR, no LDS, no
//     broadcast.  The 8 gates are split with scalar shifts and masks and enter
//     the multiplies as scalar operands.
//   * The gate load and the lane's K 16 B operand loads are all issued before
//     the first wait and the first multiply (the compiler places the scalar
//     load right behind the vector loads): the wave waits once, for both
//     counters, and the entry has arrived long before the operands.
//   * K is a template parameter (1..8): K x 4 VGPRs of operands, 8 f32 chains of
//     one multiply and K - 1 fused multiply-adds per lane.  A product of two
//     bf16 is exact in f32, so fused, unfused and packed forms agree bit for
//     bit (reduce_gate_op.hpp) and this file needs no special flags.
//   * The reduce kernel's cache policy: a range-checked system-scope descriptor
//     per peer buffer and chunk, non-temporal loads for local sources, one
//     non-temporal or system-scope 16 B store.  Sizes are whole rows, so whole
//     KiB: a wave is either inside the op or outside it, and there is no tail.
//   * Workgroups are split across a launch's ops by size (split_blocks) and
//     grid-stride when capped, as the reduce kernel's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "block_split.hpp"
#include "common.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"

namespace p2p {
namespace dev {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) u32x4* GateTable;  // read-only for the kernel's life: scalar loads

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr uint32_t kChunkVecs = 64;          // a wave's chunk: 64 x 16 B = 1 KiB
constexpr uint64_t kChunkBytes = kChunkVecs * 16;
constexpr uint64_t kBlockVecs = kBlock;      // 4 KiB per block iteration
constexpr uint64_t kMaxGrid = 1ull << 20;    // 4 GiB of output per grid pass
constexpr int kVerifyPerCu = 16;
constexpr int kSystemCoherent = 1 | 16;  // sc0 sc1
constexpr int kNonTemporal = 2;           // nt
constexpr int kRsrcFlags = 0x00020000;

// By value in the kernarg segment, like the reduce kernel's ReduceArgs.
struct GateArgs {
  const uint4* src[kMaxReduceOps][kMaxReduceSrcs];
  uint4* dst[kMaxReduceOps];
  const uint4* gate[kMaxReduceOps];
  uint64_t nvec[kMaxReduceOps];         // a multiple of kChunkVecs
  uint32_t row_chunks[kMaxReduceOps];   // chunks per row: row_elems / 512
  uint32_t coherent[kMaxReduceOps];     // GatedReduceOp::coherent_mask
  uint32_t block_begin[kMaxReduceOps + 1];
  int nops;
  int32_t uniform;  // > 0: every op has this many blocks; 0: binary search
};

template <int K>
__global__ __launch_bounds__(kBlock) void gated_reduce_kernel(const GateArgs a) {
  int op = 0;
  if (a.uniform > 0) {
    op = min(static_cast<int>(blockIdx.x / static_cast<uint32_t>(a.uniform)), a.nops - 1);
  } else {
    int lo = 0, hi = a.nops - 1;  // largest op with block_begin[op] <= blockIdx.x
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (blockIdx.x >= a.block_begin[mid]) lo = mid; else hi = mid - 1;
    }
    op = lo;
  }
  const uint32_t b = blockIdx.x - a.block_begin[op];
  const uint32_t nb = a.block_begin[op + 1] - a.block_begin[op];
  const uint64_t n = a.nvec[op];
  const uint32_t coh = a.coherent[op];
  const uint32_t row_chunks = a.row_chunks[op];
  const uint4* s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = a.src[op][k];
  uint4* d = a.dst[op];
  const GateTable gate = (GateTable)a.gate[op];
  // The compiler does not know that threadIdx.x / 64 is the same in every lane.
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  const int lane_off = static_cast<int>(threadIdx.x) * 16;

  for (uint64_t base = static_cast<uint64_t>(b) * kBlockVecs; base < n; base += static_cast<uint64_t>(nb) * kBlockVecs) {
    // Block-uniform: the chunks of this block iteration that exist (1..4).
    const uint32_t left = static_cast<uint32_t>(min<uint64_t>(kWaves, (n - base) / kChunkVecs));
    const int bytes = static_cast<int>(left * kChunkBytes);
    const bool mine = wave < left;
    // A wave past the end takes the last chunk's row and vectors and stores nothing.
    const uint32_t in_block = min(wave, left - 1u);
    const uint32_t chunk = static_cast<uint32_t>(base / kChunkVecs) + in_block;
    const uint32_t row = chunk / row_chunks;
    const u32x4 ge = gate[row];  // wave-uniform address, constant address space: one scalar 16 B load
    u32x4 v[K];
    if ((coh & ((1u << K) - 1u)) == 0) {
      const uint32_t at = in_block * kChunkVecs + lane;
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(s[k] + base) + at);
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(s[k] + base), 0, bytes, kRsrcFlags);
        if ((coh >> k) & 1u)
          v[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, 0, kSystemCoherent);
        else
          v[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, 0, kNonTemporal);
      }
    }
    // Every load above is in flight; the gates first (scalar unit), then the chains.
    float g[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const uint32_t w = ge[k >> 1];
      g[k] = reduce_bits_to_f32((k & 1) ? (w & 0xFFFF0000u) : (w << 16));
    }
    u32x4 r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float lo = g[0] * reduce_bits_to_f32(v[0][c] << 16);
      float hi = g[0] * reduce_bits_to_f32(v[0][c] & 0xFFFF0000u);
#pragma unroll
      for (int k = 1; k < K; ++k) {
        lo = __builtin_fmaf(g[k], reduce_bits_to_f32(v[k][c] << 16), lo);
        hi = __builtin_fmaf(g[k], reduce_bits_to_f32(v[k][c] & 0xFFFF0000u), hi);
      }
      r[c] = reduce_pack_bf16(lo, hi);
    }
    if (coh & kReduceDstCoherent) {
      auto rd = __builtin_amdgcn_make_buffer_rsrc(d + base, 0, bytes, kRsrcFlags);
      __builtin_amdgcn_raw_buffer_store_b128(r, rd, lane_off, 0, kSystemCoherent);  // past the end: dropped
    } else if (mine) {
      __builtin_nontemporal_store(r, reinterpret_cast<u32x4*>(d + base) + threadIdx.x);
    }
  }
}

// ---------------------------------------------------------------- gate fill ----

__global__ __launch_bounds__(kBlock) void fill_gate_kernel(uint4* __restrict__ p, uint64_t rows, uint64_t seed) {
  for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; r < rows;
       r += static_cast<uint64_t>(gridDim.x) * kBlock)
    p[r] = make_uint4(gate_word(prng_word(seed, 4 * r)), gate_word(prng_word(seed, 4 * r + 1)),
                      gate_word(prng_word(seed, 4 * r + 2)), gate_word(prng_word(seed, 4 * r + 3)));
}

// ------------------------------------------------------ verify gated reduced ----

struct GateSeedArgs {
  uint64_t seed[kMaxReduceSrcs];
  uint64_t gate_seed;
  int n;
};

struct Partial {
  unsigned long long mism, sum, first;
};

// verify_reduced_kernel's shape: per lane a 16 B vector, its expected words
// regenerated from the operand streams and the row's gate entry, then the
// wave butterfly, the 4 waves through LDS and one atomic per non-zero field.
__global__ __launch_bounds__(kBlock) void verify_gated_reduced_kernel(const uint4* __restrict__ p, uint64_t nvec,
                                                                      uint32_t row_chunks, const GateSeedArgs s,
                                                                      VerifyAccum* __restrict__ out) {
  Partial acc{0, 0, ~0ull};
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kBlockVecs; base < nvec;
       base += static_cast<uint64_t>(gridDim.x) * kBlockVecs) {
    const uint64_t i = base + threadIdx.x;
    if (i >= nvec) continue;  // whole waves: nvec is a multiple of 64
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p) + i);
    const uint64_t row = static_cast<uint32_t>(i / kChunkVecs) / row_chunks;
    uint32_t entry[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) entry[j] = gate_word(prng_word(s.gate_seed, 4 * row + j));
    const uint32_t lo = static_cast<uint32_t>(i * 4);
    float a_lo[4], a_hi[4];
    for (int k = 0; k < s.n; ++k) {
      const uint32_t key = prng_key(s.seed[k], base * 4);  // block-uniform: scalar ALU
      const float g = gate_value(entry, k);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t w = operand_word(prng_word_k(key, lo + c), ReduceType::Bf16);
        const float x_lo = reduce_bits_to_f32(w << 16), x_hi = reduce_bits_to_f32(w & 0xFFFF0000u);
        a_lo[c] = k ? a_lo[c] + g * x_lo : g * x_lo;
        a_hi[c] = k ? a_hi[c] + g * x_hi : g * x_hi;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      acc.sum += v[c];
      if (v[c] != reduce_pack_bf16(a_lo[c], a_hi[c])) {
        acc.mism += 1;
        acc.first = min(acc.first, static_cast<unsigned long long>(i * 16 + 4 * c));
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc.mism += __shfl_xor(acc.mism, off, 64);
    acc.sum += __shfl_xor(acc.sum, off, 64);
    acc.first = min(acc.first, __shfl_xor(acc.first, off, 64));
  }
  __shared__ Partial red[kWaves];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x / 64] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    Partial t = red[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      t.mism += red[w].mism;
      t.sum += red[w].sum;
      t.first = min(t.first, red[w].first);
    }
    VerifyAccum* sh = out + (blockIdx.x % kVerifyShards);
    if (t.sum) atomicAdd(&sh->checksum, t.sum);
    if (t.mism) {
      atomicAdd(&sh->mismatches, t.mism);
      atomicMin(&sh->first_bad, t.first);
    }
  }
}

// ------------------------------------------------------------------ launch ----

template <int K = kMaxReduceSrcs>
void launch_gated_k(int nsrc, uint32_t grid, const GateArgs& a, hipStream_t stream) {
  if constexpr (K < 1) {
    P2P_FATAL("gated_reduce: an op needs 1..8 sources");
  } else {
    if (nsrc == K)
      gated_reduce_kernel<K><<<grid, kBlock, 0, stream>>>(a);
    else
      launch_gated_k<K - 1>(nsrc, grid, a, stream);
  }
}

// One launch: cnt <= kMaxReduceOps ops of equal nsrc.
void launch_gated_group(const GatedReduceOp* ops, int cnt, hipStream_t stream, int max_blocks) {
  GateArgs a{};
  a.nops = cnt;
  for (int i = 0; i < cnt; ++i) {
    const GatedReduceOp& o = ops[i];
    for (int k = 0; k < o.nsrc; ++k) a.src[i][k] = static_cast<const uint4*>(o.src[k]);
    a.dst[i] = static_cast<uint4*>(o.dst);
    a.gate[i] = static_cast<const uint4*>(o.gate);
    a.nvec[i] = o.bytes / 16;
    a.row_chunks[i] = static_cast<uint32_t>(o.row_elems / kGateRowMultiple);
    a.coherent[i] = o.coherent_mask;
  }
  const uint64_t cap = max_blocks > 0 ? static_cast<uint64_t>(max_blocks) : kMaxGrid;
  const uint32_t grid = split_blocks(a.nvec, cnt, kBlockVecs, cap, a.block_begin);
  a.uniform = static_cast<int32_t>(a.block_begin[1] - a.block_begin[0]);
  for (int i = 1; i < cnt; ++i)
    if (a.block_begin[i + 1] - a.block_begin[i] != static_cast<uint32_t>(a.uniform)) a.uniform = 0;
  launch_gated_k<>(ops[0].nsrc, grid, a, stream);
  HIPCHECK(hipGetLastError());
}

uint64_t gated_blocks(size_t bytes) { return std::max<uint64_t>(1, (bytes / 16 + kBlockVecs - 1) / kBlockVecs); }

}  // namespace

void launch_gated_reduce(const GatedReduceOp* ops, int nops, hipStream_t stream, int max_blocks) {
  std::vector<GatedReduceOp> pieces;
  for (int i = 0; i < nops; ++i) {
    const GatedReduceOp& o = ops[i];
    P2P_CHECK(o.nsrc >= 1 && o.nsrc <= kMaxReduceSrcs, "gated_reduce: an op needs 1..8 sources");
    P2P_CHECK(o.row_elems >= kGateRowMultiple && o.row_elems % kGateRowMultiple == 0,
              "gated_reduce: row_elems must be a multiple of 512 (a row is whole KiB)");
    const size_t row_bytes = 2 * o.row_elems;
    P2P_CHECK(o.bytes > 0 && o.bytes % row_bytes == 0, "gated_reduce: bytes must be whole rows of row_elems bf16");
    // The kernel counts 1 KiB chunks in 32 bits, and a block iteration's descriptor range is an int.
    P2P_CHECK(o.bytes / kChunkBytes <= 0xFFFFFFFFull && o.row_elems / kGateRowMultiple <= 0xFFFFFFFFull,
              "gated_reduce: at most 2^32 KiB per op");
    P2P_CHECK(o.gate && reinterpret_cast<uintptr_t>(o.gate) % 16 == 0 && reinterpret_cast<uintptr_t>(o.dst) % 16 == 0,
              "gated_reduce: 16-byte aligned buffers and gate table required");
    for (int k = 0; k < o.nsrc; ++k)
      P2P_CHECK(o.src[k] && reinterpret_cast<uintptr_t>(o.src[k]) % 16 == 0, "gated_reduce: 16-byte aligned buffers required");
    // Ops above 4 GiB go in pieces of whole rows (the gate table moves with
    // them), unless the caller caps the grid and the kernel strides anyway.
    const size_t piece = std::max<size_t>(1, static_cast<size_t>(kMaxGrid * kBlockVecs * 16) / row_bytes) * row_bytes;
    size_t off = 0;
    do {
      const size_t n = max_blocks > 0 ? o.bytes : std::min(piece, o.bytes - off);
      GatedReduceOp p = o;
      p.dst = static_cast<char*>(o.dst) + off;
      for (int k = 0; k < o.nsrc; ++k) p.src[k] = static_cast<const char*>(o.src[k]) + off;
      p.gate = static_cast<const char*>(o.gate) + off / row_bytes * kGateEntryBytes;
      p.bytes = n;
      pieces.push_back(p);
      off += n;
    } while (off < o.bytes);
  }
  // A launch: consecutive pieces of one fan-in, at most kMaxReduceOps, and
  // (uncapped) at most kMaxGrid blocks, so every piece gets a full grid.
  size_t i = 0;
  while (i < pieces.size()) {
    size_t j = i;
    uint64_t blocks = 0;
    while (j < pieces.size() && j - i < static_cast<size_t>(kMaxReduceOps) && pieces[j].nsrc == pieces[i].nsrc &&
           (j == i || max_blocks > 0 || blocks + gated_blocks(pieces[j].bytes) <= kMaxGrid))
      blocks += gated_blocks(pieces[j++].bytes);
    launch_gated_group(pieces.data() + i, static_cast<int>(j - i), stream, max_blocks);
    i = j;
  }
}

void launch_fill_gate(void* p, size_t rows, uint64_t seed, hipStream_t stream) {
  if (!rows) return;
  P2P_CHECK(reinterpret_cast<uintptr_t>(p) % 16 == 0, "fill_gate: table must be 16-byte aligned");
  const unsigned grid = static_cast<unsigned>(std::min<uint64_t>((rows + kBlock - 1) / kBlock, kMaxGrid));
  fill_gate_kernel<<<grid, kBlock, 0, stream>>>(static_cast<uint4*>(p), rows, seed);
  HIPCHECK(hipGetLastError());
}

void launch_verify_gated_reduced(const void* p, size_t bytes, const uint64_t* seeds, int nseeds, uint64_t gate_seed,
                                 size_t row_elems, VerifyAccum* acc, hipStream_t stream) {
  P2P_CHECK(nseeds >= 1 && nseeds <= kMaxReduceSrcs, "verify_gated_reduced: 1..8 operand seeds");
  P2P_CHECK(gate_rows(bytes, row_elems) > 0 || bytes == 0, "verify_gated_reduced: whole rows of row_elems bf16, row_elems a multiple of 512");
  P2P_CHECK(bytes / kChunkBytes <= 0xFFFFFFFFull, "verify_gated_reduced: at most 2^32 KiB");
  if (bytes) {
    P2P_CHECK(reinterpret_cast<uintptr_t>(p) % 16 == 0, "verify_gated_reduced: buffer must be 16-byte aligned");
    GateSeedArgs s{};
    s.n = nseeds;
    s.gate_seed = gate_seed;
    for (int k = 0; k < nseeds; ++k) s.seed[k] = seeds[k];
    const uint64_t nvec = bytes / 16;
    const uint64_t cap = static_cast<uint64_t>(cu_count()) * kVerifyPerCu;
    const unsigned grid = static_cast<unsigned>(std::max<uint64_t>(1, std::min((nvec + kBlockVecs - 1) / kBlockVecs, cap)));
    verify_gated_reduced_kernel<<<grid, kBlock, 0, stream>>>(static_cast<const uint4*>(p), nvec,
                                                            static_cast<uint32_t>(row_elems / kGateRowMultiple), s, acc);
    HIPCHECK(hipGetLastError());
  }
  // The finalize of launch_verify (zero bytes: nothing else runs): shards -> acc[0].
  launch_verify(nullptr, 0, 0, acc, VerifyImpl::Auto, false, stream);
}

}  // namespace dev
}  // namespace p2p
