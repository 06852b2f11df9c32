// gfx950 (MI355X, CDNA4) mismatch diagnosis kernel.  See diagnose.hpp for the
// contract.  Design notes:
//   * The clean path is verify_stride_kernel's (kernels.hip): 16 B per lane,
//     four loads in flight per lane, one PRNG key per 16 KiB tile from
//     block-uniform values on the scalar unit, four mixes per vector.  A wave
//     whose tile holds no wrong word does nothing else.
//   * A workgroup walks units of two consecutive tiles (32 KiB).  A unit lies
//     in one granule or covers at most eight whole ones, so its counts fit a
//     small LDS table: a wave that holds wrong words classifies them,
//     reduces each 4 KiB piece with the wave64 butterfly (as block_commit)
//     and adds the piece's totals to the table with LDS atomics.
//   * At the end of a unit the workgroup votes (__syncthreads_or) whether any
//     of its waves touched the table.  Only then is it flushed: one global
//     atomic per non-zero field of each record, add for the counts, max for
//     both ends of the damage (DiagRecord's encoding turns the first word's
//     min into a max).  Workgroups that share a large granule's record meet
//     in those atomics.  A clean workgroup issues none.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "diagnose.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"

namespace p2p {
namespace dev {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;
constexpr int kUnroll = 4;                                        // loads in flight per lane
constexpr uint64_t kTileVecs = kBlock * kUnroll;                  // 16 KiB
constexpr int kUnitTiles = 2;
constexpr uint64_t kUnitVecs = kTileVecs * kUnitTiles;            // 32 KiB
constexpr uint32_t kUnitShift = 15;                               // log2 of a unit's bytes
constexpr int kPieceShift = 12;                                   // one load of the workgroup: 4 KiB
constexpr int kSlots = static_cast<int>((kUnitVecs * 16) >> kPieceShift);  // granules of a unit, at most
constexpr int kPerCu = 16;                                        // workgroups per CU (verify_stride's cap)
static_assert(kUnitVecs * 16 == 1ull << kUnitShift, "kUnitShift is the unit's size");
static_assert(kSlots * kDiagFields <= kBlock, "one thread flushes one field of one slot");

// Field order of DiagRecord; the LDS table keeps the same order in 32 bits
// (a unit holds 8192 words), with both ends as word offsets into the unit.
enum : int { kZero = 0, kOther = 1, kCand = 2, kFlipped = 8, kFirst = 9, kLast = 10 };

// Passed by value in the kernarg segment.
struct CandArgs {
  uint64_t seed[kMaxDiagCandidates];
  long long shift_words[kMaxDiagCandidates];  // multiples of 4
  int n;
};

struct LaneDiag {
  uint32_t f[kDiagFields];
};

__device__ __forceinline__ uint4 load_nt(const uint4* p, uint64_t i) {
  const u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p) + i);
  return make_uint4(t.x, t.y, t.z, t.w);
}

__device__ __forceinline__ uint4 prng_vec_k(uint32_t key, uint64_t vec_index) {
  const uint32_t lo = static_cast<uint32_t>(vec_index * 4);
  return make_uint4(prng_word_k(key, lo), prng_word_k(key, lo + 1), prng_word_k(key, lo + 2), prng_word_k(key, lo + 3));
}

// Classifies the four words of vector `vec_index` (a lane's 16 B); `word0` is
// the offset of its first word in the unit.
__device__ __forceinline__ void classify_vec(const uint4 v, const uint4 e, uint64_t vec_index, uint32_t word0,
                                             const CandArgs& c, LaneDiag& d) {
  const uint32_t got[4] = {v.x, v.y, v.z, v.w};
  const uint32_t want[4] = {e.x, e.y, e.z, e.w};
  bool open[4];  // wrong, not poison, no candidate matched yet
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool bad = got[j] != want[j];
    const bool zero = bad && got[j] == 0;
    open[j] = bad && !zero;
    d.f[kZero] += zero;
    if (bad) {
      d.f[kFirst] = min(d.f[kFirst], word0 + j);
      d.f[kLast] = max(d.f[kLast], word0 + j + 1);
    }
  }
#pragma unroll
  for (int k = 0; k < kMaxDiagCandidates; ++k) {
    if (k >= c.n || !(open[0] || open[1] || open[2] || open[3])) continue;
    // A shift is a multiple of 4 words: the four shifted words share a sign
    // and a 2^32-word region, so one key serves them.
    const long long w0 = static_cast<long long>(vec_index * 4) + c.shift_words[k];
    if (w0 < 0) continue;
    const uint32_t key = prng_key(c.seed[k], static_cast<uint64_t>(w0));
    const uint32_t lo = static_cast<uint32_t>(w0);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (open[j] && got[j] == prng_word_k(key, lo + j)) {
        open[j] = false;
        d.f[kCand + k] += 1;
      }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (open[j]) {
      d.f[kOther] += 1;
      d.f[kFlipped] += __popc(got[j] ^ want[j]);
    }
}

// The wave's totals of one 4 KiB piece into LDS slot `slot`.
__device__ __forceinline__ void wave_commit(LaneDiag d, uint32_t* slot) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int f = 0; f < kFirst; ++f) d.f[f] += __shfl_xor(d.f[f], off, 64);
    d.f[kFirst] = min(d.f[kFirst], __shfl_xor(d.f[kFirst], off, 64));
    d.f[kLast] = max(d.f[kLast], __shfl_xor(d.f[kLast], off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int f = 0; f < kFirst; ++f)
      if (d.f[f]) atomicAdd(&slot[f], d.f[f]);
    atomicMin(&slot[kFirst], d.f[kFirst]);
    atomicMax(&slot[kLast], d.f[kLast]);
  }
}

__device__ __forceinline__ void record_commit(DiagRecord* rec, int field, unsigned long long v) {
  unsigned long long* p = reinterpret_cast<unsigned long long*>(rec) + field;
  if (field < kFirst)
    atomicAdd(p, v);
  else
    atomicMax(p, v);
}

__global__ __launch_bounds__(kBlock) void diagnose_kernel(const uint4* __restrict__ p, uint64_t nvec, uint64_t seed,
                                                          const CandArgs cands, uint32_t granule_shift,
                                                          const uint8_t* __restrict__ tail, uint32_t tail_bytes,
                                                          uint64_t tail_offset, DiagRecord* __restrict__ records) {
  __shared__ uint32_t table[kSlots][kDiagFields];
  for (int t = threadIdx.x; t < kSlots * kDiagFields; t += kBlock)
    table[t / kDiagFields][t % kDiagFields] = (t % kDiagFields) == kFirst ? ~0u : 0u;
  __syncthreads();

  // Granules smaller than a unit: piece q of the unit belongs to slot
  // q >> piece_to_slot.  Otherwise the whole unit lies in one granule: slot 0.
  const bool small = granule_shift < kUnitShift;
  const uint32_t piece_to_slot = small ? granule_shift - kPieceShift : 31;

  for (uint64_t ubase = static_cast<uint64_t>(blockIdx.x) * kUnitVecs; ubase < nvec;
       ubase += static_cast<uint64_t>(gridDim.x) * kUnitVecs) {
    int dirty = 0;  // wave-uniform: this wave added to the table in this unit
#pragma unroll
    for (int t = 0; t < kUnitTiles; ++t) {
      const uint64_t base = ubase + static_cast<uint64_t>(t) * kTileVecs;
      if (base >= nvec) break;  // block-uniform
      uint4 v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {  // all loads issued before any compare
        const uint64_t i = base + static_cast<uint64_t>(u) * kBlock + threadIdx.x;
        v[u] = i < nvec ? load_nt(p, i) : make_uint4(0, 0, 0, 0);
      }
      const uint32_t key = prng_key(seed, base * 4);  // block-uniform: scalar ALU
      unsigned bad = 0;  // bit u: this lane's vector u holds a wrong word
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const uint64_t i = base + static_cast<uint64_t>(u) * kBlock + threadIdx.x;
        if (i < nvec) {
          const uint4 e = prng_vec_k(key, i);
          bad |= static_cast<unsigned>(v[u].x != e.x || v[u].y != e.y || v[u].z != e.z || v[u].w != e.w) << u;
        }
      }
      if (!__any(bad)) continue;  // the clean path ends here
      dirty = 1;
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (!__any(bad & (1u << u))) continue;
        LaneDiag d;
#pragma unroll
        for (int f = 0; f < kDiagFields; ++f) d.f[f] = f == kFirst ? ~0u : 0u;
        if (bad & (1u << u)) {
          const uint64_t i = base + static_cast<uint64_t>(u) * kBlock + threadIdx.x;
          classify_vec(v[u], prng_vec_k(key, i), i, static_cast<uint32_t>(i - ubase) * 4, cands, d);
        }
        wave_commit(d, table[(t * kUnroll + u) >> piece_to_slot]);
      }
    }
    if (__syncthreads_or(dirty)) {  // every wave's LDS atomics are done
      const int t = threadIdx.x;
      if (t < kSlots * kDiagFields) {
        const int s = t / kDiagFields, f = t % kDiagFields;
        const uint32_t val = table[s][f];
        const uint64_t ubyte = ubase * 16;
        DiagRecord* rec = records + (ubyte >> granule_shift) + (small ? s : 0);
        if (f == kFirst) {
          if (val != ~0u) record_commit(rec, f, ~(ubyte + 4ull * val));
          table[s][f] = ~0u;
        } else {
          if (val) record_commit(rec, f, f == kLast ? ubyte + 4ull * (val - 1) + 1 : val);
          table[s][f] = 0;
        }
      }
      __syncthreads();  // the table is reset before the next unit's waves add to it
    }
  }

  // Sub-16-byte tail: whole words, then a masked partial word, as check_tail.
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (uint32_t off = 0; off < tail_bytes; off += 4) {
      const uint32_t n = min(4u, tail_bytes - off);
      uint32_t got = 0;  // the bytes past the end stay zero: `got` is masked already
      for (uint32_t b = 0; b < n; ++b) got |= static_cast<uint32_t>(tail[off + b]) << (8 * b);
      const uint32_t mask = n == 4 ? 0xFFFFFFFFu : ((1u << (8 * n)) - 1u);
      const uint64_t byte = tail_offset + off;
      const uint32_t want = prng_word(seed, byte / 4) & mask;
      if (got == want) continue;
      int field = got == 0 ? kZero : kOther;
#pragma unroll
      for (int k = 0; k < kMaxDiagCandidates; ++k) {  // static indices: the candidates stay in kernarg registers
        const long long w = static_cast<long long>(byte / 4) + cands.shift_words[k];
        if (field == kOther && k < cands.n && w >= 0 &&
            got == (prng_word(cands.seed[k], static_cast<uint64_t>(w)) & mask))
          field = kCand + k;
      }
      DiagRecord* rec = records + (byte >> granule_shift);
      record_commit(rec, field, 1);
      if (field == kOther) record_commit(rec, kFlipped, __popc(got ^ want));
      record_commit(rec, kFirst, ~byte);
      record_commit(rec, kLast, byte + 1);
    }
  }
}

}  // namespace

void launch_diagnose(const void* p, size_t bytes, uint64_t seed, const DiagCandidate* cands, int ncand, size_t granule,
                     DiagRecord* records, hipStream_t stream, unsigned max_grid) {
  check_diagnose_args(cands, ncand, granule);
  if (!bytes) return;
  P2P_CHECK(reinterpret_cast<uintptr_t>(p) % 16 == 0, "diagnose: buffer must be 16-byte aligned");
  HIPCHECK(hipMemsetAsync(records, 0, diagnose_records(bytes, granule) * sizeof(DiagRecord), stream));
  CandArgs c{};
  c.n = ncand;
  for (int k = 0; k < ncand; ++k) {
    c.seed[k] = cands[k].seed;
    c.shift_words[k] = cands[k].shift / 4;
  }
  uint32_t shift = 0;
  while ((size_t{1} << shift) < granule) ++shift;
  const uint64_t nvec = bytes / 16;
  const uint32_t tail = static_cast<uint32_t>(bytes - nvec * 16);
  const uint64_t units = (nvec + kUnitVecs - 1) / kUnitVecs;
  const uint64_t cap = max_grid ? max_grid : static_cast<uint64_t>(cu_count()) * kPerCu;
  const unsigned grid = static_cast<unsigned>(std::max<uint64_t>(1, std::min(units, cap)));
  diagnose_kernel<<<grid, kBlock, 0, stream>>>(static_cast<const uint4*>(p), nvec, seed, c, shift,
                                               static_cast<const uint8_t*>(p) + nvec * 16, tail, nvec * 16, records);
  HIPCHECK(hipGetLastError());
}

}  // namespace dev
}  // namespace p2p
