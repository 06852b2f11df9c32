// Host side of the mismatch diagnosis (diagnose.hpp): the CPU implementation
// of the classification, the merge of granule records into extents and the
// text of an extent.
#include "diagnose.hpp"

#include <algorithm>
#include <cstring>

#include "common.hpp"
#include "transport.hpp"

namespace p2p {

size_t diagnose_granule(size_t bytes) {
  size_t g = kMinDiagGranule;
  while ((bytes + g - 1) / g > kMaxDiagRecords) g <<= 1;
  return g;
}

size_t diagnose_records(size_t bytes, size_t granule) { return (bytes + granule - 1) / granule; }

void check_diagnose_args(const DiagCandidate* cands, int ncand, size_t granule) {
  P2P_CHECK(ncand >= 0 && ncand <= kMaxDiagCandidates, strfmt("diagnose: at most %d candidates", kMaxDiagCandidates));
  for (int k = 0; k < ncand; ++k)
    P2P_CHECK(cands[k].shift % 16 == 0, "diagnose: a candidate's shift must be a multiple of 16 bytes");
  P2P_CHECK(granule >= kMinDiagGranule && (granule & (granule - 1)) == 0,
            "diagnose: the granule must be a power of two, at least 4 KiB");
}

namespace {

void count_word(DiagRecord& r, int cls, uint32_t flipped, uint64_t byte_offset) {
  if (cls == kDiagOk) return;
  if (cls == kDiagZero) {
    ++r.zero;
  } else if (cls == kDiagOther) {
    ++r.other;
    r.flipped_bits += flipped;
  } else {
    ++r.cand[cls - kDiagCand0];
  }
  r.first_enc = std::max<unsigned long long>(r.first_enc, ~byte_offset);
  r.last_enc = std::max<unsigned long long>(r.last_enc, byte_offset + 1);
}

// Bit k + 2: cand k; bit 0 zero, bit 1 other.
unsigned class_set(const DiagRecord& r) {
  unsigned s = (r.zero ? 1u : 0u) | (r.other ? 2u : 0u);
  for (int k = 0; k < kMaxDiagCandidates; ++k) s |= r.cand[k] ? 4u << k : 0u;
  return s;
}

std::string candidate_text(const DiagCandidate& c, int k) {
  switch (c.kind) {
    case DiagCandidate::Generation:
      return strfmt("the sender's generation %lld (stale)", static_cast<long long>(c.value));
    case DiagCandidate::Offset:
      return strfmt("the sender's stream %lld bytes %s (misplaced op)",
                    static_cast<long long>(c.shift < 0 ? -c.shift : c.shift), c.shift < 0 ? "earlier" : "further on");
    case DiagCandidate::Sender:
      return strfmt("rank %lld's payload (wrong sender)", static_cast<long long>(c.value));
    default:
      break;
  }
  if (c.shift)
    return strfmt("candidate %d (seed 0x%llx, %+lld bytes)", k, static_cast<unsigned long long>(c.seed),
                  static_cast<long long>(c.shift));
  return strfmt("candidate %d (seed 0x%llx)", k, static_cast<unsigned long long>(c.seed));
}

}  // namespace

std::vector<DiagRecord> host_diagnose(const void* p, size_t bytes, uint64_t seed, const DiagCandidate* cands, int ncand,
                                      size_t granule) {
  if (!granule) granule = diagnose_granule(bytes);
  check_diagnose_args(cands, ncand, granule);
  std::vector<DiagRecord> recs(diagnose_records(bytes, granule));
  if (!recs.empty()) std::memset(recs.data(), 0, recs.size() * sizeof(DiagRecord));
  const auto* b = static_cast<const uint8_t*>(p);
  for (size_t off = 0; off < bytes; off += 4) {
    const size_t n = std::min<size_t>(4, bytes - off);
    uint32_t got = 0;
    std::memcpy(&got, b + off, n);
    const uint32_t mask = n == 4 ? 0xFFFFFFFFu : ((1u << (8 * n)) - 1u);
    uint32_t flipped = 0;
    const int cls = diag_classify(got, mask, seed, off / 4, cands, ncand, &flipped);
    count_word(recs[off / granule], cls, flipped, off);
  }
  return recs;
}

// Records carry absolute offsets, so the granule's size is not needed here.
std::vector<DiagExtent> merge_extents(const DiagRecord* records, size_t nrecords, size_t bytes, size_t /*granule*/) {
  std::vector<DiagExtent> out;
  unsigned open_set = 0;  // class set of the extent being grown; 0: none open
  for (size_t i = 0; i < nrecords; ++i) {
    const DiagRecord& r = records[i];
    const unsigned set = r.damaged() ? class_set(r) : 0;
    if (!set) {
      open_set = 0;
      continue;
    }
    if (set != open_set) {
      DiagExtent e;
      e.begin = r.first_bad();
      out.push_back(e);
      open_set = set;
    }
    DiagExtent& e = out.back();
    e.end = std::min<uint64_t>(r.last_bad() + 4, bytes);
    e.zero += r.zero;
    e.other += r.other;
    for (int k = 0; k < kMaxDiagCandidates; ++k) e.cand[k] += r.cand[k];
    e.flipped_bits += r.flipped_bits;
  }
  return out;
}

std::vector<DiagExtent> host_diagnose_extents(const void* p, size_t bytes, uint64_t seed,
                                              const std::vector<DiagCandidate>& candidates) {
  const size_t granule = diagnose_granule(bytes);
  const auto recs = host_diagnose(p, bytes, seed, candidates.data(), static_cast<int>(candidates.size()), granule);
  return merge_extents(recs.data(), recs.size(), bytes, granule);
}

std::string describe_extent(const DiagExtent& e, size_t bytes, const DiagCandidate* cands, int ncand) {
  std::string o = strfmt("bytes [%llu, %llu) of %zu:", static_cast<unsigned long long>(e.begin),
                         static_cast<unsigned long long>(e.end), bytes);
  bool first = true;
  auto part = [&](uint64_t words, const std::string& what) {
    if (!words) return;
    o += strfmt("%s %llu word%s %s", first ? "" : ";", static_cast<unsigned long long>(words), words == 1 ? "" : "s",
                what.c_str());
    first = false;
  };
  part(e.zero, "still poison (never written)");
  for (int k = 0; k < kMaxDiagCandidates; ++k)
    part(e.cand[k], std::string(e.cand[k] == 1 ? "matches " : "match ") +
                        (k < ncand ? candidate_text(cands[k], k) : strfmt("candidate %d", k)));
  part(e.other, strfmt("%s from every candidate in %llu bit%s", e.other == 1 ? "differs" : "differ",
                       static_cast<unsigned long long>(e.flipped_bits), e.flipped_bits == 1 ? "" : "s"));
  return o;
}

}  // namespace p2p
