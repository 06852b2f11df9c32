// The device-side checks of one stream's user (a GPU transport, or the Python
// module per device): the single verify, the batched verify, the mismatch
// diagnosis and the inline-check records, with the arrays they read back.
// Every array is a DeviceMirror, so a stream is drained before an array it
// may still use is freed.  A blocking call takes the stream and the caller's
// own wait for it: the transports' bounded, abort-aware sync(),
// hipStreamSynchronize in the Python module.  GPU translation units only.
#pragma once

#include <functional>
#include <vector>

#include "device_mirror.hpp"
#include "diagnose.hpp"
#include "kernels.hpp"
#include "transport.hpp"

namespace p2p {

using StreamWait = std::function<void()>;

namespace dev {

// launch_multi_verify with its scratch, device results and host results.
// enqueue() makes room for njobs results (draining first should they grow),
// then puts the batched verify and, unless readback is false (timing the
// kernels), ONE readback of every job's totals on `stream`; results() is
// valid once the caller has waited for the stream.
class BatchVerifier {
 public:
  BatchVerifier() = default;
  BatchVerifier(const BatchVerifier&) = delete;
  BatchVerifier& operator=(const BatchVerifier&) = delete;
  ~BatchVerifier();
  void enqueue(const VerifyJob* jobs, int njobs, hipStream_t stream, const StreamWait& drain, bool readback = true);
  const VerifyAccum* results() const { return out_.host(); }

 private:
  VerifyAccum* scratch_ = nullptr;  // fixed size, allocated once: never freed under a stream
  DeviceMirror<VerifyAccum> out_;
};

// launch_diagnose with its device records and their host copy.  enqueue()
// makes room (draining first should the records grow), then puts the kernel
// and ONE readback of the records on `stream`; records() is valid once the
// caller has waited for the stream.
class Diagnoser {
 public:
  // Returns the granule used (granule == 0: diagnose_granule(bytes)).
  // readback = false leaves the records on the device (timing the kernel).
  size_t enqueue(const void* p, size_t bytes, uint64_t seed, const DiagCandidate* cands, int ncand, size_t granule,
                 hipStream_t stream, const StreamWait& drain, unsigned max_grid = 0, bool readback = true);
  const DiagRecord* records() const { return recs_.host(); }
  size_t count() const { return count_; }

 private:
  DeviceMirror<DiagRecord> recs_;
  size_t count_ = 0;
};

}  // namespace dev

VerifyResult to_result(const dev::VerifyAccum& a);
Transport::InlineCheck to_inline_check(const dev::CopyCheck& c);

class DeviceChecks {
 public:
  explicit DeviceChecks(dev::VerifyImpl impl = dev::VerifyImpl::Auto) : impl_(impl) {}

  // ---- single verify (Transport::verify) ----
  VerifyResult verify(const void* p, size_t bytes, uint64_t seed, hipStream_t stream, const StreamWait& wait,
                      bool check = true, unsigned max_grid = 0, int lds_stages = 0);
  // Stream-ordered reset + verify + finalize with `impl`, and the readback
  // unless readback is false; verify_result() once the caller has waited.
  void verify_enqueue(const void* p, size_t bytes, uint64_t seed, hipStream_t stream, dev::VerifyImpl impl, bool check,
                      unsigned max_grid, int lds_stages, bool readback);
  VerifyResult verify_result() const { return to_result(acc_.host()[0]); }

  // ---- batched verify (Transport::verify_many) ----
  // One buffer at a time under --verify-impl stride or P2P_VERIFY_BATCH=0.
  std::vector<VerifyResult> verify_many(const std::vector<VerifyJob>& jobs, hipStream_t stream, const StreamWait& wait);
  dev::BatchVerifier& batch() { return batch_; }  // always the batched kernel; its launch-only form

  // ---- diagnosis (Transport::diagnose) ----
  std::vector<DiagExtent> diagnose(const void* p, size_t bytes, uint64_t seed,
                                   const std::vector<DiagCandidate>& candidates, hipStream_t stream,
                                   const StreamWait& wait);
  dev::Diagnoser& diagnoser() { return diag_; }  // the record-level and launch-only forms

  // ---- inline-check records (kernels.hpp CopyCheck) ----
  // n records; reset to {0, ~0} on `stream` unless reset is false.
  void records_begin(size_t n, hipStream_t stream, const StreamWait& wait, bool reset = true);
  size_t records() const { return nrecords_; }
  dev::CopyCheck* record(size_t i) const;
  // Blocking, one readback: one entry per record.
  std::vector<Transport::InlineCheck> records_read(hipStream_t stream, const StreamWait& wait);

 private:
  dev::VerifyImpl impl_;
  DeviceMirror<dev::VerifyAccum> acc_;  // kVerifyShards shards; the totals end in shard 0
  dev::BatchVerifier batch_;
  dev::Diagnoser diag_;
  DeviceMirror<dev::CopyCheck> records_;
  size_t nrecords_ = 0;
};

}  // namespace p2p
