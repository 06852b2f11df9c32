// gfx950 receive-and-reduce kernels: multi-source reduce, operand fill and the
// check of a reduced buffer.  kernels.hpp has the contract, reduce_op.hpp the
// arithmetic.  Design:
//   * The copy kernel's geometry: one 16 B vector per lane, one 4 KiB block
//     per 256-thread workgroup, workgroups split across a launch's ops by size
//     (split_blocks), the uniform / binary-search workgroup -> op lookup.
//   * The fan-in K is a template parameter: a lane issues its K 16 B loads
//     back to back (K x 4 VGPRs, 32 at K = 8), and only then walks the add
//     chain, so K remote loads are in flight per lane and a wave waits once.
//   * Output traffic is 1 / K of the input: one non-temporal 16 B store.
//   * No LDS and no matrix instructions: every byte is used once.
//   * This file is built without packed f32 instructions: the add chains of
//     the four words of a vector are independent, and a pairing of them into
//     packed adds is not wanted here.
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

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr uint64_t kBlockVecs = kBlock;    // 16 B vectors per block iteration (4 KiB)
constexpr uint64_t kMaxGrid = 1ull << 20;  // 4 GiB of output per grid pass
constexpr int kVerifyPerCu = 16;           // verify_reduced: workgroups per CU, grid-stride beyond
// Cache-policy bits and descriptor word of the cross-GPU accesses (kernels.hip).
constexpr int kSystemCoherent = 1 | 16;  // sc0 sc1
constexpr int kNonTemporal = 2;           // nt
constexpr int kRsrcFlags = 0x00020000;

// By value in the kernarg segment, like the copy's CopyArgs (about 700 B).
struct ReduceArgs {
  const uint4* src[kMaxReduceOps][kMaxReduceSrcs];
  uint4* dst[kMaxReduceOps];
  uint4* dst_hi[kMaxReduceOps];        // partial_out: the plane of the high halves' f32 sums
  uint64_t nvec[kMaxReduceOps];
  uint32_t tail_words[kMaxReduceOps];  // 0..3 words after the last whole vector
  uint32_t coherent[kMaxReduceOps];    // ReduceOp::coherent_mask
  uint32_t block_begin[kMaxReduceOps + 1];
  int nops;
  int32_t uniform;  // > 0: every op has this many blocks (one division); 0: binary search
};

// One word of K loaded operands.  PIN (bf16 only): operands 0 and 1 are not
// messages but the two f32 planes of a running sum (the low halves' sums, the
// high halves'); POUT: the sum leaves as those two planes, unrounded, so a
// fan-in spread over several launches still rounds once, at the end.
template <ReduceType T, int K, bool PIN, bool POUT>
__device__ __forceinline__ void reduce_one(const uint32_t (&w)[K], uint32_t& r, uint32_t& r_hi) {
  ReduceAcc a;
  if constexpr (PIN)
    a = ReduceAcc{0u, reduce_bits_to_f32(w[0]), reduce_bits_to_f32(w[1])};
  else
    a = reduce_begin(w[0], T);
#pragma unroll
  for (int k = PIN ? 2 : 1; k < K; ++k) reduce_add(a, w[k], T);
  if constexpr (POUT) {
    r = reduce_f32_to_bits(a.lo);
    r_hi = reduce_f32_to_bits(a.hi);
  } else {
    r = reduce_finish(a, T);
  }
}

template <ReduceType T, int K, bool PIN, bool POUT>
__device__ __forceinline__ void reduce_vec(const u32x4 (&v)[K], u32x4& r, u32x4& r_hi) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    uint32_t w[K], x = 0, y = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = v[k][c];
    reduce_one<T, K, PIN, POUT>(w, x, y);
    r[c] = x;
    r_hi[c] = y;
  }
}

template <ReduceType T, int K, bool PIN, bool POUT>
__global__ __launch_bounds__(kBlock) void multi_reduce_kernel(const ReduceArgs a) {
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
  // dst may be one of the sources (a later launch of a wide fan-in): no
  // __restrict__ on either.
  const uint4* s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = a.src[op][k];
  uint4* d = a.dst[op];
  const int lane_off = static_cast<int>(threadIdx.x) * 16;

  for (uint64_t base = static_cast<uint64_t>(b) * kBlockVecs; base < n; base += static_cast<uint64_t>(nb) * kBlockVecs) {
    // Block-uniform: the chunk's bytes, the range of every descriptor below.
    const int bytes = static_cast<int>(min<uint64_t>(kBlockVecs, n - base) * 16);
    const bool mine = lane_off < bytes;
    // All K loads are issued before the first add, and nothing else writes
    // v[] in between (no zero-fill of the lanes past the end, which made the
    // compiler wait for each load in turn): the wave waits once.
    u32x4 v[K];
    if ((coh & ((1u << K) - 1u)) == 0) {
      // Every source is local: straight-line non-temporal loads; a lane past
      // the end re-reads the chunk's last vector and stores nothing.
      const uint32_t at = mine ? threadIdx.x : static_cast<uint32_t>(bytes / 16 - 1);
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(s[k] + base) + at);
    } else {
      // A range-checked descriptor per source and chunk (a lane past the end
      // loads 0); the block-uniform branch only picks the cache policy:
      // system scope for a peer's buffer, non-temporal for a local one.
#pragma unroll
      for (int k = 0; k < K; ++k) {
        auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(s[k] + base), 0, bytes, kRsrcFlags);
        if ((coh >> k) & 1u)
          v[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, 0, kSystemCoherent);
        else
          v[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, lane_off, 0, kNonTemporal);
      }
    }
    u32x4 r, r_hi;
    reduce_vec<T, K, PIN, POUT>(v, r, r_hi);
    if constexpr (POUT) {  // the planes are local scratch
      if (mine) {
        __builtin_nontemporal_store(r, reinterpret_cast<u32x4*>(d + base) + threadIdx.x);
        __builtin_nontemporal_store(r_hi, reinterpret_cast<u32x4*>(a.dst_hi[op] + base) + threadIdx.x);
      }
    } else if (coh & kReduceDstCoherent) {
      auto rd = __builtin_amdgcn_make_buffer_rsrc(d + base, 0, bytes, kRsrcFlags);
      __builtin_amdgcn_raw_buffer_store_b128(r, rd, lane_off, 0, kSystemCoherent);  // past the end: dropped
    } else if (mine) {
      __builtin_nontemporal_store(r, reinterpret_cast<u32x4*>(d + base) + threadIdx.x);
    }
  }
  // The 4 / 8 / 12-byte tail, one word per lane.
  if (b == 0 && threadIdx.x < a.tail_words[op]) {
    const int tail_bytes = static_cast<int>(a.tail_words[op]) * 4;
    const int off = static_cast<int>(threadIdx.x) * 4;
    uint32_t w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if ((coh >> k) & 1u) {
        auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(s[k] + n), 0, tail_bytes, kRsrcFlags);
        w[k] = __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, kSystemCoherent);
      } else {
        w[k] = reinterpret_cast<const uint32_t*>(s[k] + n)[threadIdx.x];
      }
    }
    uint32_t r = 0, r_hi = 0;
    reduce_one<T, K, PIN, POUT>(w, r, r_hi);
    if constexpr (POUT) {
      reinterpret_cast<uint32_t*>(d + n)[threadIdx.x] = r;
      reinterpret_cast<uint32_t*>(a.dst_hi[op] + n)[threadIdx.x] = r_hi;
    } else if (coh & kReduceDstCoherent) {
      auto rd = __builtin_amdgcn_make_buffer_rsrc(d + n, 0, tail_bytes, kRsrcFlags);
      __builtin_amdgcn_raw_buffer_store_b32(r, rd, off, 0, kSystemCoherent);
    } else {
      reinterpret_cast<uint32_t*>(d + n)[threadIdx.x] = r;
    }
  }
}

// ------------------------------------------------------------ operand fill ----

template <ReduceType T>
__global__ __launch_bounds__(kBlock) void fill_operand_kernel(uint4* __restrict__ p, uint64_t begin, uint64_t nvec,
                                                              uint64_t seed, uint32_t tail_words) {
  for (uint64_t base = begin + static_cast<uint64_t>(blockIdx.x) * kBlockVecs; base < nvec;
       base += static_cast<uint64_t>(gridDim.x) * kBlockVecs) {
    const uint32_t key = prng_key(seed, base * 4);  // block-uniform: scalar ALU
    const uint64_t i = base + threadIdx.x;
    if (i < nvec) {
      const uint32_t lo = static_cast<uint32_t>(i * 4);
      p[i] = make_uint4(operand_word(prng_word_k(key, lo), T), operand_word(prng_word_k(key, lo + 1), T),
                        operand_word(prng_word_k(key, lo + 2), T), operand_word(prng_word_k(key, lo + 3), T));
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < tail_words)
    reinterpret_cast<uint32_t*>(p + nvec)[threadIdx.x] = operand_word(prng_word(seed, nvec * 4 + threadIdx.x), T);
}

// ---------------------------------------------------------- verify reduced ----

struct SeedArgs {
  uint64_t seed[kMaxReduceSeeds];
  int n;
};

struct Partial {
  unsigned long long mism, sum, first;
};

// Words [lo, lo + N) of the sum of the operand streams (all in one 2^32-word
// key span starting at word `key_word`): one scalar key per operand, N sums.
template <ReduceType T, int N>
__device__ __forceinline__ void expected_words(const SeedArgs& s, uint64_t key_word, uint32_t lo, uint32_t (&want)[N]) {
  ReduceAcc a[N];
  const uint32_t key0 = prng_key(s.seed[0], key_word);  // block-uniform: scalar ALU
#pragma unroll
  for (int c = 0; c < N; ++c) a[c] = reduce_begin(operand_word(prng_word_k(key0, lo + c), T), T);
  for (int k = 1; k < s.n; ++k) {
    const uint32_t key = prng_key(s.seed[k], key_word);
#pragma unroll
    for (int c = 0; c < N; ++c) reduce_add(a[c], operand_word(prng_word_k(key, lo + c), T), T);
  }
#pragma unroll
  for (int c = 0; c < N; ++c) want[c] = reduce_finish(a[c], T);
}

template <ReduceType T>
__global__ __launch_bounds__(kBlock) void verify_reduced_kernel(const uint4* __restrict__ p, uint64_t nvec,
                                                                uint32_t tail_words, const SeedArgs s,
                                                                VerifyAccum* __restrict__ out) {
  Partial acc{0, 0, ~0ull};
  auto check = [&](uint32_t got, uint32_t want, uint64_t byte) {
    acc.sum += got;
    if (got != want) {
      acc.mism += 1;
      acc.first = min(acc.first, static_cast<unsigned long long>(byte));
    }
  };
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kBlockVecs; base < nvec;
       base += static_cast<uint64_t>(gridDim.x) * kBlockVecs) {
    const uint64_t i = base + threadIdx.x;
    const u32x4 v = i < nvec ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p) + i) : u32x4{0, 0, 0, 0};
    uint32_t want[4];
    expected_words<T, 4>(s, base * 4, static_cast<uint32_t>(i * 4), want);
    if (i < nvec) {
#pragma unroll
      for (int c = 0; c < 4; ++c) check(v[c], want[c], i * 16 + 4 * c);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < tail_words) {
    const uint64_t word = nvec * 4 + threadIdx.x;
    uint32_t want[1];
    expected_words<T, 1>(s, nvec * 4, static_cast<uint32_t>(word), want);
    check(reinterpret_cast<const uint32_t*>(p + nvec)[threadIdx.x], want[0], word * 4);
  }
  // kernels.hip block_commit: wave butterfly, the 4 waves through LDS, one
  // atomic per non-zero field into this block's shard.
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

template <ReduceType T, bool PIN, bool POUT, int K = kMaxReduceSrcs>
void launch_reduce_k(int nsrc, uint32_t grid, const ReduceArgs& a, hipStream_t stream) {
  if constexpr (K < (PIN ? 3 : 1)) {
    P2P_FATAL("multi_reduce: an op needs 1..8 sources (3..8 with a partial sum coming in)");
  } else {
    if (nsrc == K)
      multi_reduce_kernel<T, K, PIN, POUT><<<grid, kBlock, 0, stream>>>(a);
    else
      launch_reduce_k<T, PIN, POUT, K - 1>(nsrc, grid, a, stream);
  }
}

// One launch: cnt <= kMaxReduceOps ops of equal nsrc and partial flags.
void launch_reduce_group(const ReduceOp* ops, int cnt, ReduceType dtype, hipStream_t stream, int max_blocks) {
  ReduceArgs a{};
  a.nops = cnt;
  for (int i = 0; i < cnt; ++i) {
    const ReduceOp& o = ops[i];
    P2P_CHECK(reinterpret_cast<uintptr_t>(o.dst) % 16 == 0, "multi_reduce: 16-byte aligned buffers required");
    for (int k = 0; k < o.nsrc; ++k) {
      P2P_CHECK(o.src[k] && reinterpret_cast<uintptr_t>(o.src[k]) % 16 == 0, "multi_reduce: 16-byte aligned buffers required");
      a.src[i][k] = static_cast<const uint4*>(o.src[k]);
    }
    a.dst[i] = static_cast<uint4*>(o.dst);
    P2P_CHECK(!o.partial_out || (o.dst_hi && reinterpret_cast<uintptr_t>(o.dst_hi) % 16 == 0),
              "multi_reduce: partial_out needs a 16-byte aligned dst_hi");
    a.dst_hi[i] = static_cast<uint4*>(o.dst_hi);
    a.nvec[i] = o.bytes / 16;
    a.tail_words[i] = static_cast<uint32_t>(o.bytes % 16 / 4);
    a.coherent[i] = o.coherent_mask;
  }
  const uint64_t cap = max_blocks > 0 ? static_cast<uint64_t>(max_blocks) : kMaxGrid;
  const uint32_t grid = split_blocks(a.nvec, cnt, kBlockVecs, cap, a.block_begin);
  a.uniform = static_cast<int32_t>(a.block_begin[1] - a.block_begin[0]);
  for (int i = 1; i < cnt; ++i)
    if (a.block_begin[i + 1] - a.block_begin[i] != static_cast<uint32_t>(a.uniform)) a.uniform = 0;
  const int nsrc = ops[0].nsrc;
  const bool pin = ops[0].partial_in, pout = ops[0].partial_out;
  P2P_CHECK(dtype == ReduceType::Bf16 || !(pin || pout), "multi_reduce: partial sums are bf16's (f32 and u32 need none)");
  if (dtype == ReduceType::U32)
    launch_reduce_k<ReduceType::U32, false, false>(nsrc, grid, a, stream);
  else if (dtype == ReduceType::F32)
    launch_reduce_k<ReduceType::F32, false, false>(nsrc, grid, a, stream);
  else if (pin && pout)
    launch_reduce_k<ReduceType::Bf16, true, true>(nsrc, grid, a, stream);
  else if (pin)
    launch_reduce_k<ReduceType::Bf16, true, false>(nsrc, grid, a, stream);
  else if (pout)
    launch_reduce_k<ReduceType::Bf16, false, true>(nsrc, grid, a, stream);
  else
    launch_reduce_k<ReduceType::Bf16, false, false>(nsrc, grid, a, stream);
  HIPCHECK(hipGetLastError());
}

uint64_t reduce_blocks(size_t bytes) { return std::max<uint64_t>(1, (bytes / 16 + kBlockVecs - 1) / kBlockVecs); }

void check_dtype(ReduceType t, const char* who) {
  P2P_CHECK(t == ReduceType::U32 || t == ReduceType::F32 || t == ReduceType::Bf16,
            std::string(who) + ": dtype must be u32, f32 or bf16");
}

}  // namespace

void launch_multi_reduce(const ReduceOp* ops, int nops, ReduceType dtype, hipStream_t stream, int max_blocks) {
  check_dtype(dtype, "multi_reduce");
  // Ops above 4 GiB go in 4 GiB pieces (a multiple of 16: the pieces keep
  // their alignment, and only the last one has a tail), unless the caller
  // caps the grid and the kernel strides anyway.
  const size_t piece = static_cast<size_t>(kMaxGrid * kBlockVecs * 16);
  std::vector<ReduceOp> pieces;
  for (int i = 0; i < nops; ++i) {
    const ReduceOp& o = ops[i];
    P2P_CHECK(o.bytes % 4 == 0, "multi_reduce: bytes must be a multiple of 4");
    P2P_CHECK(o.nsrc >= 1 && o.nsrc <= kMaxReduceSrcs, "multi_reduce: an op needs 1..8 sources");
    size_t off = 0;
    do {
      const size_t n = max_blocks > 0 ? o.bytes : std::min(piece, o.bytes - off);
      ReduceOp p = o;
      p.dst = static_cast<char*>(o.dst) + off;
      if (o.dst_hi) p.dst_hi = static_cast<char*>(o.dst_hi) + off;
      for (int k = 0; k < o.nsrc; ++k) p.src[k] = static_cast<const char*>(o.src[k]) + off;
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
           pieces[j].partial_in == pieces[i].partial_in && pieces[j].partial_out == pieces[i].partial_out &&
           (j == i || max_blocks > 0 || blocks + reduce_blocks(pieces[j].bytes) <= kMaxGrid))
      blocks += reduce_blocks(pieces[j++].bytes);
    launch_reduce_group(pieces.data() + i, static_cast<int>(j - i), dtype, stream, max_blocks);
    i = j;
  }
}

void launch_reduce_wide(void* dst, size_t bytes, const void* const* srcs, const unsigned char* coherent, int nsrcs,
                        bool dst_coherent, ReduceType dtype, hipStream_t stream, int max_blocks, void* partial) {
  P2P_CHECK(nsrcs >= 1, "reduce: at least one source");
  // bf16 rounds once, after the last operand: between launches the running
  // sum travels as two f32 planes in `partial` (reduce_partial_bytes), never
  // through dst.  u32 and f32 sums are exact in their own type: dst carries them.
  const bool planes = dtype == ReduceType::Bf16 && nsrcs > kMaxReduceSrcs;
  P2P_CHECK(!planes || (partial && reinterpret_cast<uintptr_t>(partial) % 16 == 0),
            "reduce: a bf16 fan-in above 8 needs reduce_partial_bytes() of 16-byte aligned scratch");
  void* lo = partial;
  void* hi = planes ? static_cast<char*>(partial) + reduce_partial_bytes(bytes) / 2 : nullptr;
  for (int first = 0; first < nsrcs;) {
    ReduceOp op;
    op.dst = dst;
    op.bytes = bytes;
    if (first > 0 && planes) {  // the running sum is operands 0 and 1
      op.partial_in = true;
      op.src[op.nsrc++] = lo;
      op.src[op.nsrc++] = hi;
    } else if (first > 0) {  // the running sum is operand 0
      if (dst_coherent) op.coherent_mask |= 1u;
      op.src[op.nsrc++] = dst;
    }
    while (first < nsrcs && op.nsrc < kMaxReduceSrcs) {
      if (coherent && coherent[first]) op.coherent_mask |= 1u << op.nsrc;
      op.src[op.nsrc++] = srcs[first++];
    }
    if (planes && first < nsrcs) {  // not the last launch: the planes go out
      op.partial_out = true;
      op.dst = lo;
      op.dst_hi = hi;
    } else if (dst_coherent) {
      op.coherent_mask |= kReduceDstCoherent;
    }
    launch_multi_reduce(&op, 1, dtype, stream, max_blocks);
  }
}

void launch_fill_operand(void* p, size_t bytes, uint64_t seed, ReduceType dtype, hipStream_t stream) {
  check_dtype(dtype, "fill_operand");
  P2P_CHECK(bytes % 4 == 0, "fill_operand: bytes must be a multiple of 4");
  if (dtype == ReduceType::U32) {
    launch_fill(p, bytes, seed, stream);
    return;
  }
  if (!bytes) return;
  P2P_CHECK(reinterpret_cast<uintptr_t>(p) % 16 == 0, "fill_operand: buffer must be 16-byte aligned");
  const uint64_t nvec = bytes / 16;
  const uint32_t tail_words = static_cast<uint32_t>(bytes % 16 / 4);
  auto* vp = static_cast<uint4*>(p);
  const uint64_t chunk = kMaxGrid * kBlockVecs;  // full grids: one launch per 4 GiB, as launch_fill
  for (uint64_t begin = 0;; begin += chunk) {
    const uint64_t end = std::min(nvec, begin + chunk);
    const bool last = end == nvec;
    const unsigned grid =
        static_cast<unsigned>(std::max<uint64_t>(1, std::min((end - begin + kBlockVecs - 1) / kBlockVecs, kMaxGrid)));
    if (dtype == ReduceType::F32)
      fill_operand_kernel<ReduceType::F32><<<grid, kBlock, 0, stream>>>(vp, begin, end, seed, last ? tail_words : 0);
    else
      fill_operand_kernel<ReduceType::Bf16><<<grid, kBlock, 0, stream>>>(vp, begin, end, seed, last ? tail_words : 0);
    HIPCHECK(hipGetLastError());
    if (last) break;
  }
}

void launch_verify_reduced(const void* p, size_t bytes, const uint64_t* seeds, int nseeds, ReduceType dtype,
                           VerifyAccum* acc, hipStream_t stream) {
  check_dtype(dtype, "verify_reduced");
  P2P_CHECK(bytes % 4 == 0, "verify_reduced: bytes must be a multiple of 4");
  P2P_CHECK(nseeds >= 1 && nseeds <= kMaxReduceSeeds, "verify_reduced: 1..32 operand seeds");
  if (bytes) {
    P2P_CHECK(reinterpret_cast<uintptr_t>(p) % 16 == 0, "verify_reduced: buffer must be 16-byte aligned");
    SeedArgs s{};
    s.n = nseeds;
    for (int k = 0; k < nseeds; ++k) s.seed[k] = seeds[k];
    const uint64_t nvec = bytes / 16;
    const uint32_t tail_words = static_cast<uint32_t>(bytes % 16 / 4);
    const uint64_t cap = static_cast<uint64_t>(cu_count()) * kVerifyPerCu;
    const unsigned grid = static_cast<unsigned>(std::max<uint64_t>(1, std::min((nvec + kBlockVecs - 1) / kBlockVecs, cap)));
    const auto* vp = static_cast<const uint4*>(p);
    if (dtype == ReduceType::U32)
      verify_reduced_kernel<ReduceType::U32><<<grid, kBlock, 0, stream>>>(vp, nvec, tail_words, s, acc);
    else if (dtype == ReduceType::F32)
      verify_reduced_kernel<ReduceType::F32><<<grid, kBlock, 0, stream>>>(vp, nvec, tail_words, s, acc);
    else
      verify_reduced_kernel<ReduceType::Bf16><<<grid, kBlock, 0, stream>>>(vp, nvec, tail_words, s, acc);
    HIPCHECK(hipGetLastError());
  }
  // The finalize of launch_verify (zero bytes: nothing else runs): shards -> acc[0].
  launch_verify(nullptr, 0, 0, acc, VerifyImpl::Auto, false, stream);
}

}  // namespace dev
}  // namespace p2p
