// DeviceChecks and the two checks that own arrays (device_checks.hpp).
#include "device_checks.hpp"

#include <cstdlib>
#include <cstring>

#include "common.hpp"

namespace p2p {

namespace dev {

BatchVerifier::~BatchVerifier() {
  if (scratch_) (void)hipFree(scratch_);
}

void BatchVerifier::enqueue(const VerifyJob* jobs, int njobs, hipStream_t stream, const StreamWait& drain,
                            bool readback) {
  if (njobs <= 0) return;
  if (!scratch_) HIPCHECK(hipMalloc(&scratch_, multi_verify_scratch_bytes()));
  out_.reserve(static_cast<size_t>(njobs), drain);
  launch_multi_verify(jobs, njobs, scratch_, out_.device(), stream);
  if (readback) out_.readback(static_cast<size_t>(njobs), stream);
}

size_t Diagnoser::enqueue(const void* p, size_t bytes, uint64_t seed, const DiagCandidate* cands, int ncand,
                          size_t granule, hipStream_t stream, const StreamWait& drain, unsigned max_grid,
                          bool readback) {
  if (!granule) granule = diagnose_granule(bytes);
  check_diagnose_args(cands, ncand, granule);
  count_ = diagnose_records(bytes, granule);
  recs_.reserve(count_, drain);
  if (!count_) return granule;
  launch_diagnose(p, bytes, seed, cands, ncand, granule, recs_.device(), stream, max_grid);
  if (readback) recs_.readback(count_, stream);
  return granule;
}

}  // namespace dev

VerifyResult to_result(const dev::VerifyAccum& a) { return {a.mismatches, a.checksum, a.first_bad}; }
Transport::InlineCheck to_inline_check(const dev::CopyCheck& c) { return {c.mismatches, c.first_bad}; }

namespace {
// P2P_VERIFY_BATCH=0: the one-buffer-at-a-time check (the A/B of round 3's
// post-timing verification against the batched one).
bool batch_verify_enabled() {
  static const bool on = [] {
    const char* e = std::getenv("P2P_VERIFY_BATCH");
    return !(e && std::strcmp(e, "0") == 0);
  }();
  return on;
}
}  // namespace

void DeviceChecks::verify_enqueue(const void* p, size_t bytes, uint64_t seed, hipStream_t stream, dev::VerifyImpl impl,
                                  bool check, unsigned max_grid, int lds_stages, bool readback) {
  acc_.reserve(dev::kVerifyShards, [] {});  // one size: allocated once, never regrown
  dev::launch_verify_reset(acc_.device(), stream);
  dev::launch_verify(p, bytes, seed, acc_.device(), impl, check, stream, max_grid, lds_stages);
  if (readback) acc_.readback(1, stream);
}

VerifyResult DeviceChecks::verify(const void* p, size_t bytes, uint64_t seed, hipStream_t stream,
                                  const StreamWait& wait, bool check, unsigned max_grid, int lds_stages) {
  verify_enqueue(p, bytes, seed, stream, impl_, check, max_grid, lds_stages, true);
  wait();
  return verify_result();
}

std::vector<VerifyResult> DeviceChecks::verify_many(const std::vector<VerifyJob>& jobs, hipStream_t stream,
                                                    const StreamWait& wait) {
  if (jobs.empty()) return {};
  // The batched kernel is the default LDS8 verify; another --verify-impl
  // keeps the one-buffer path.
  if ((impl_ != dev::VerifyImpl::Auto && impl_ != dev::VerifyImpl::Lds8) || !batch_verify_enabled()) {
    std::vector<VerifyResult> out;
    for (const auto& j : jobs) out.push_back(verify(j.p, j.bytes, j.seed, stream, wait));
    return out;
  }
  batch_.enqueue(jobs.data(), static_cast<int>(jobs.size()), stream, wait);
  wait();
  std::vector<VerifyResult> out(jobs.size());
  for (size_t i = 0; i < out.size(); ++i) out[i] = to_result(batch_.results()[i]);
  return out;
}

std::vector<DiagExtent> DeviceChecks::diagnose(const void* p, size_t bytes, uint64_t seed,
                                               const std::vector<DiagCandidate>& candidates, hipStream_t stream,
                                               const StreamWait& wait) {
  const size_t granule =
      diag_.enqueue(p, bytes, seed, candidates.data(), static_cast<int>(candidates.size()), 0, stream, wait);
  wait();
  return merge_extents(diag_.records(), diag_.count(), bytes, granule);
}

void DeviceChecks::records_begin(size_t n, hipStream_t stream, const StreamWait& wait, bool reset) {
  records_.reserve(n, wait);
  nrecords_ = n;
  if (reset) dev::launch_copy_check_reset(records_.device(), static_cast<int>(n), stream);
}

dev::CopyCheck* DeviceChecks::record(size_t i) const {
  P2P_CHECK(i < nrecords_, "inline check: begin first, with enough records (inline_check_begin)");
  return records_.device() + i;
}

std::vector<Transport::InlineCheck> DeviceChecks::records_read(hipStream_t stream, const StreamWait& wait) {
  std::vector<Transport::InlineCheck> out(nrecords_);
  if (!nrecords_) return out;
  records_.readback(nrecords_, stream);
  wait();
  for (size_t i = 0; i < nrecords_; ++i) out[i] = to_inline_check(records_.host()[i]);
  return out;
}

}  // namespace p2p
