// Mismatch diagnosis: where a buffer differs from its PRNG stream, and what
// the wrong words hold instead.
//
// verify answers "how many words are wrong"; this answers "which bytes, and
// are they still poison, another stream, or noise".  The payload is a
// counter-based PRNG (prng.hpp), so every sender, generation and offset has a
// stream that can be regenerated next to the received data.
//
// Classification, per 32-bit word w of the buffer (the final partial word is
// compared under the byte mask check_tail / host_verify use, in every
// comparison below), first rule that holds:
//   1. the word equals prng_word(seed, w)                       -> ok
//   2. the word is zero (the poison zero_slots writes)          -> zero
//   3. the first candidate k, in list order, with w + shift_k/4 >= 0 and the
//      word equal to prng_word(seed_k, w + shift_k/4)           -> cand k
//      (the key comes from the shifted index: a shift may cross a 2^32-word
//      region of the stream)
//   4. otherwise -> other, and flipped_bits += popcount((got ^ expected) & mask)
//
// Results are kept per granule (a power of two >= 4 KiB): one DiagRecord each.
// The HIP kernel (diagnose.hip), host_diagnose and the PyTorch reference
// (ops/buffers.py reference_diagnose) produce the same records bit for bit.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "prng.hpp"

// hipStream_t as <hip/hip_runtime.h> declares it, so this header also serves
// the host-only build.
struct ihipStream_t;
typedef struct ihipStream_t* hipStream_t;

namespace p2p {

constexpr int kMaxDiagCandidates = 6;
constexpr size_t kMinDiagGranule = 4096;
constexpr size_t kMaxDiagRecords = 65536;  // the default granule gives at most this many

// Another stream the wrong words may come from: prng_word(seed, w + shift/4).
// `shift` is a signed byte count, a multiple of 16.  kind / value only say
// what the candidate stands for in describe_extent's text.
struct DiagCandidate {
  enum Kind : int { Stream = 0, Generation = 1, Offset = 2, Sender = 3 };
  uint64_t seed = 0;
  int64_t shift = 0;
  int kind = Stream;
  int64_t value = 0;  // Generation: the generation; Sender: the rank
};

// One granule.  All-zero bytes mean "nothing damaged", so a memset resets an
// array of them: first_enc is ~(byte offset of the first damaged word), kept
// with an atomic max, last_enc is (byte offset of the last damaged word) + 1.
struct DiagRecord {
  unsigned long long zero;
  unsigned long long other;
  unsigned long long cand[kMaxDiagCandidates];
  unsigned long long flipped_bits;
  unsigned long long first_enc;
  unsigned long long last_enc;

  bool damaged() const { return last_enc != 0; }
  uint64_t first_bad() const { return ~first_enc; }
  uint64_t last_bad() const { return last_enc - 1; }
};
constexpr int kDiagFields = 11;
static_assert(sizeof(DiagRecord) == kDiagFields * sizeof(unsigned long long), "fields are addressed by index");

// A maximal run of consecutive damaged granules with the same set of non-zero
// classes: [begin, end) runs from its first damaged word to the end of its
// last one (clipped to the buffer).
struct DiagExtent {
  uint64_t begin = 0;
  uint64_t end = 0;
  uint64_t zero = 0;
  uint64_t other = 0;
  uint64_t cand[kMaxDiagCandidates] = {0, 0, 0, 0, 0, 0};
  uint64_t flipped_bits = 0;
  uint64_t words() const {
    uint64_t n = zero + other;
    for (uint64_t c : cand) n += c;
    return n;
  }
};

// Class of one word: 0 ok, 1 zero, 2 other, 3 + k candidate k.
enum : int { kDiagOk = 0, kDiagZero = 1, kDiagOther = 2, kDiagCand0 = 3 };

P2P_HD int diag_classify(uint32_t got, uint32_t mask, uint64_t seed, uint64_t word, const DiagCandidate* cands,
                         int ncand, uint32_t* flipped) {
  const uint32_t want = prng_word(seed, word);
  got &= mask;
  if (got == (want & mask)) return kDiagOk;
  if (got == 0) return kDiagZero;
  for (int k = 0; k < ncand; ++k) {
    const int64_t w = static_cast<int64_t>(word) + cands[k].shift / 4;
    if (w >= 0 && got == (prng_word(cands[k].seed, static_cast<uint64_t>(w)) & mask)) return kDiagCand0 + k;
  }
  *flipped = static_cast<uint32_t>(__builtin_popcount((got ^ want) & mask));
  return kDiagOther;
}

// Smallest power of two >= 4 KiB that covers `bytes` in at most 65536 records.
size_t diagnose_granule(size_t bytes);
// Records a buffer of `bytes` has at `granule` (0 for an empty buffer).
size_t diagnose_records(size_t bytes, size_t granule);
// Fails a P2P_CHECK unless the candidates and the granule are usable.
void check_diagnose_args(const DiagCandidate* cands, int ncand, size_t granule);

// Host implementation (the CPU transports; the kernel's reference in tests).
// granule == 0: diagnose_granule(bytes).
std::vector<DiagRecord> host_diagnose(const void* p, size_t bytes, uint64_t seed, const DiagCandidate* cands, int ncand,
                                      size_t granule = 0);
std::vector<DiagExtent> merge_extents(const DiagRecord* records, size_t nrecords, size_t bytes, size_t granule);
// "bytes [b, e) of N: ..." -- what the extent's words hold instead.
std::string describe_extent(const DiagExtent& e, size_t bytes, const DiagCandidate* cands, int ncand);

namespace dev {

// Stream-ordered: zeroes `records` (diagnose_records(bytes, granule) of them,
// device memory) and runs the gfx950 kernel over the buffer.  max_grid > 0
// caps the workgroup count (the kernel grid-strides beyond it); 0 = the
// default, 16 workgroups per CU.
void launch_diagnose(const void* p, size_t bytes, uint64_t seed, const DiagCandidate* cands, int ncand, size_t granule,
                     DiagRecord* records, hipStream_t stream, unsigned max_grid = 0);
// (device_checks.hpp Diagnoser owns the records and their host copy.)

}  // namespace dev
}  // namespace p2p
