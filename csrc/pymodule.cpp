// Python bindings (`test_nccl_p2p_amd._p2pcore`), pybind11.
//
// Exposes the native engine to bench.py / the Python package: a Session owns
// a Bootstrap (TCP star, or local) and a Transport (RCCL on the MI355X, or
// host sockets).  Everything long-running releases the GIL.  Results cross
// the boundary as JSON text produced by report.cpp, so the Python side and
// the p2p_matrix executable share one result schema.
//
// The fill / verify kernels are also exposed on raw device pointers so they
// can be driven on torch tensors and checked against a PyTorch reference; so
// are the one-wave ping-pong and signal kernels, with the two kinds of memory
// they spin on (signal_page, HostWords), for tests against a protocol model.
#include <hip/hip_runtime.h>

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "app.hpp"
#include "bootstrap.hpp"
#include "common.hpp"
#include "device_checks.hpp"
#include "kernels.hpp"
#include "load.hpp"
#include "provenance.hpp"
#include "report.hpp"
#include "runner.hpp"
#include "routing.hpp"
#include "schedule.hpp"
#include "stream_layout.hpp"
#include "transport.hpp"
#include "units.hpp"

namespace py = pybind11;
using namespace p2p;

namespace {

// Teardown of an engine object from Python's deallocation: the transports'
// waits (buffers freed, streams drained) run without the GIL, so bench.py's
// deadline watchdog keeps running meanwhile, and inside a NativeCall, so the
// watchdog does not abort these communicators from its thread (the drain
// honours its abort request instead).
template <class Fn>
void teardown_outside_gil(Fn&& fn) {
  NativeCall in_engine(std::nothrow);
  if (PyGILState_Check()) {
    py::gil_scoped_release nogil;
    fn();
  } else {
    fn();
  }
}

class Session {
 public:
  Session(int rank, int world, const std::string& host, int port, int device, const std::string& transport,
          double timeout_s, TcpListener* listener)
      : transport_kind_(transport) {
    if (world == 1)
      boot_ = make_local_bootstrap();
    else
      boot_ = make_tcp_bootstrap(rank, world, host, port, timeout_s, listener);
    TransportOptions opt;
    opt.device = device;
    opt.timeout_s = timeout_s;
    // "ipc" or "ipc:kernel" / "ipc:sdma" / "ipc:push"
    std::string kind = transport.substr(0, transport.find(':'));
    if (kind == "ipc" && transport.size() > 4) opt.ipc_engine = transport.substr(4);
    // "rccl:K": K communicators per rank (TransportOptions::rccl_comms)
    if (kind == "rccl" && transport.size() > 5) opt.rccl_comms = std::atoi(transport.substr(5).c_str());
    if (kind == "rccl")
      t_ = make_rccl_transport(*boot_, opt);
    else if (kind == "ipc")
      t_ = make_ipc_transport(*boot_, opt);
    else if (kind == "host")
      t_ = make_host_transport(*boot_, opt);
    else if (kind == "shm")
      t_ = make_shm_transport(*boot_, opt);
    else
      P2P_FATAL("transport must be 'rccl[:K]', 'ipc[:kernel|:sdma|:push|:relay]', 'host' or 'shm'");
  }

  ~Session() {
    teardown_outside_gil([this] {
      loads_.clear();  // before the transport they came from
      t_.reset();
      boot_.reset();
    });
  }

  int rank() const { return boot_->rank(); }
  int world() const { return boot_->size(); }
  std::string transport() const { return t_->name(); }
  std::string device_desc() const { return t_->device_desc(); }
  Bootstrap& boot() { return *boot_; }
  Transport& t() { return *t_; }

  void barrier() { boot_->barrier(); }
  double allreduce_max(double v) { return boot_->allreduce_max(v); }
  double allreduce_sum(double v) { return boot_->allreduce_sum(v); }

  // One (mode, dir, size) run; returns the run JSON (report.cpp schema).
  std::string run(const std::string& mode, const std::string& dir, size_t bytes, int iters, int warmup,
                  const std::string& timing, bool verify, bool warm, const std::vector<std::pair<int, int>>& cells,
                  int diagnose, bool inline_check, const std::string& load) {
    LoadSpec load_spec;
    std::string why;
    P2P_CHECK(load.empty() || parse_load_spec(load, &load_spec, &why), "load '" + load + "': " + why);
    Schedule s = make_schedule(parse_mode(mode), parse_direction(dir), world());
    restrict_cells(&s, cells, true);
    RunConfig cfg;
    cfg.bytes = bytes;
    cfg.iters = iters;
    cfg.warmup = warmup;
    cfg.timing = parse_timing(timing);
    cfg.verify = verify;
    cfg.salt = ++salt_;
    cfg.diagnose = std::max(0, diagnose);
    cfg.inline_check = inline_check;
    P2P_CHECK(!inline_check || (verify && t_->supports_inline_check()),
              "inline_check needs verify=True and transport 'ipc' or 'ipc:kernel' (the pull engine's own copy kernel)");
    const int slots = std::max(1, s.max_recv_slots());
    // Verified runs: one receive generation per iteration, as far as memory
    // allows (runner.hpp RunConfig::gens).
    cfg.gens = verify ? verify_generations(*t_, *boot_, bytes, slots, std::max(iters, warmup)) : 1;
    if (const char* rc = std::getenv("P2P_RECHUNK")) cfg.rechunk = std::atoi(rc) != 0;
    Buffers bufs(*t_, bytes, slots * cfg.gens, slot_stride_bytes(bytes) * static_cast<size_t>(cfg.gens));
    if (warm) {
      warm_connections(*t_, *boot_, s, bufs);
      t_->refine_op_limits(*boot_);
    }
    RunRecord rec;
    rec.mode = s.mode;
    rec.dir = s.dir;
    rec.bytes = bytes;
    rec.cfg = cfg;
    rec.phases = run_schedule(*t_, *boot_, s, cfg, bufs);
    if (!load_spec.on()) return run_to_json(rec, world());
    // load="mfma[:WGS]" | "hbm[:WGS]": the run once more beside a background
    // load (app.hpp run_loaded); the loaded record is what comes back.
    // One calibrated load per spec for the session's life: a run does not pay
    // (or drift with) a fresh 256 MiB scratch and calibration each time.
    auto it = loads_.find(load);
    if (it == loads_.end()) it = loads_.emplace(load, open_load(*t_, *boot_, load_spec)).first;
    return run_to_json(run_loaded(*t_, *boot_, s, rec, ++salt_, it->second, bufs), world());
  }

  std::string latency(size_t bytes, int iters, int warmup, int preposted) {
    Buffers bufs(*t_, std::max<size_t>(bytes, 16), 1);
    auto lat = run_latency(*t_, *boot_, bytes, iters, warmup, bufs, preposted);
    return latency_to_json(lat, world());
  }

  uint64_t fuzz(int rounds, uint64_t seed, size_t max_bytes) { return fuzz_transport(*t_, *boot_, rounds, seed, max_bytes); }

  // Test hook for the transports' watchdogs: a receive from this rank that
  // no send matches, then sync().  Returns the error the watchdog raised (""
  // if none did).  The buffer is kept: an aborted transfer may not have let go.
  std::string unmatched_recv(size_t bytes) {
    void* p = t_->alloc(bytes);
    try {
      t_->group_begin();
      t_->recv(p, bytes, rank());
      t_->group_end();
      t_->sync();
    } catch (const Error& e) {
      return e.what();
    }
    t_->release(p);
    return "";
  }

  // Test hook for teardown: a receive from `peer` that no send matches,
  // posted and left pending (no sync); the session's destructor must still
  // end, bounded by its timeout (RcclTransport::drain_quietly).  The buffer is
  // leaked on purpose: an aborted transfer may not have let go of it.
  void post_unmatched_recv(size_t bytes, int peer) {
    void* p = t_->alloc(bytes);
    t_->group_begin();
    t_->recv(p, bytes, peer);
    t_->group_end();
  }

  // Test hooks for the timing tests: the transport's own marks, so a test can
  // bracket work it posted itself.  elapsed_ms is valid after a sync.
  int mark() { return t_->mark(); }
  double elapsed_ms(int from, int to) { return t_->elapsed_ms(from, to); }
  void clear_marks() { t_->clear_marks(); }

  // Test hook for the stream gate: arm one, release it or not, wait for the
  // stream.  An unreleased gate must open by itself at its deadline.
  std::string gate_probe(double timeout_s, bool release) {
    const double t0 = now_seconds();
    if (!t_->gate_arm(timeout_s)) return "{\"supported\":false}";
    if (release) t_->gate_release();
    t_->sync();
    const double waited = now_seconds() - t0;
    const bool expired = t_->gate_timed_out();
    if (!release) t_->gate_release();  // keep the sequence consistent for later gates
    return strfmt("{\"supported\":true,\"timed_out\":%s,\"seconds\":%.4f}", expired ? "true" : "false", waited);
  }

  // Test hooks for the rendezvous tests: the gate on its own (a rank holds
  // its stream while its peers post), and whether the stream has finished
  // what was posted, without waiting for it.
  bool gate_arm(double timeout_s) { return t_->gate_arm(timeout_s); }
  void gate_release() { t_->gate_release(); }
  bool gate_timed_out() { return t_->gate_timed_out(); }
  bool stream_idle() { return t_->stream_idle(); }
  std::string async_error() { return t_->async_error(); }

  std::string device_latency(size_t bytes, int iters, int warmup) {
    return latency_to_json(run_device_latency(*t_, *boot_, bytes, iters, warmup), world());
  }

  // Device-initiated stream (runner.hpp run_device_stream): a JSON list, one
  // {"device_stream": ...} object per (direction form, size).
  std::string device_stream(const std::vector<size_t>& sizes, int depth, int channels, int iters, const std::string& dir) {
    std::vector<Direction> dirs;
    if (dir == "both")
      dirs = {Direction::Uni, Direction::Bi};
    else
      dirs = {parse_direction(dir)};
    std::string o = "[";
    for (const StreamResult& r : run_device_stream(*t_, *boot_, sizes, depth, channels, iters, dirs))
      o += (o.size() > 1 ? "," : "") + device_stream_to_json(r);
    return o + "]";
  }

  // Dependent ring token chain (runner.hpp run_ring_latency); device=true
  // runs it as the one-wave kernel of the IPC transport.
  std::string ring_latency(size_t bytes, int laps, int warmup, bool device) {
    if (device) return ring_latency_to_json(run_device_ring_latency(*t_, *boot_, bytes, laps, warmup));
    Buffers bufs(*t_, std::max<size_t>(bytes, 16), 1);
    return ring_latency_to_json(run_ring_latency(*t_, *boot_, bytes, laps, warmup, bufs));
  }

  // Bounds every later wait of this session (transport and bootstrap).
  void set_timeout(double seconds) {
    t_->set_timeout(seconds);
    boot_->set_timeout(seconds);
  }

  // Largest op a message is posted as (RCCL: 16 MiB per p2p channel, see
  // transport_rccl.cpp), capped on every rank alike.
  bool set_chunk_cap(size_t bytes) { return t_->set_chunk_cap(bytes); }
  size_t max_chunk(int peer) const { return t_->max_chunk(peer); }
  // Collective: re-derive the op limits from what the transport connected.
  bool refine_op_limits() { return t_->refine_op_limits(*boot_); }

  // Collective: every rank's Transport::link_report() as a JSON list (rank
  // order; null where the transport has nothing to report).
  std::string link_reports() {
    const auto all = boot_->allgather_string(t_->link_report());
    std::string o = "[";
    for (size_t r = 0; r < all.size(); ++r) o += (r ? "," : "") + (all[r].empty() ? std::string("null") : all[r]);
    return o + "]";
  }

  // Collective: provenance_json() for this session's ranks.
  std::string provenance(int device) { return provenance_json(*boot_, device); }

 private:
  std::unique_ptr<Bootstrap> boot_;
  std::unique_ptr<Transport> t_;
  std::string transport_kind_;
  std::map<std::string, LoadSession> loads_;  // run(load=): by spec text
  uint64_t salt_ = 1000;
};

class PyStepDriver {
 public:
  PyStepDriver(std::shared_ptr<Session> s, const std::string& mode, const std::string& dir, size_t bytes, int msgs,
               bool verify, bool batch, bool graph, int depth, size_t recv_budget, uint64_t salt)
      : session_(std::move(s)),
        d_(std::make_unique<StepDriver>(session_->t(), session_->boot(),
                                        make_schedule(parse_mode(mode), parse_direction(dir), session_->world()),
                                        bytes, msgs, verify, salt, StepOptions{batch, graph, depth, recv_budget})) {}
  ~PyStepDriver() {
    teardown_outside_gil([this] {
      // Drain first (bounded): the driver's buffers are freed next.
      if (!session_->t().drain_quietly()) {
        (void)d_.release();  // leaked: kernels may still use its buffers
        return;
      }
      d_.reset();
    });
  }
  StepDriver& d() { return *d_; }

 private:
  std::shared_ptr<Session> session_;  // keeps transport alive
  std::unique_ptr<StepDriver> d_;
};

hipStream_t as_stream(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

// Kernel entry points on raw device pointers (torch tensors' data_ptr()).
// Every check's arrays live in one DeviceChecks per device, never destroyed:
// a static destructor would free device memory after the HIP runtime shut
// down.  Growing one waits on the stream passed in (stream_wait).
DeviceChecks& checks_for_current_device() {
  static auto* per_device = new std::vector<DeviceChecks*>();
  int dv = 0;
  HIPCHECK(hipGetDevice(&dv));
  if (static_cast<int>(per_device->size()) <= dv) per_device->resize(static_cast<size_t>(dv) + 1, nullptr);
  DeviceChecks*& c = (*per_device)[static_cast<size_t>(dv)];
  if (!c) c = new DeviceChecks();
  return *c;
}

StreamWait stream_wait(hipStream_t st) {
  return [st] { HIPCHECK(hipStreamSynchronize(st)); };
}

dev::VerifyImpl verify_impl_arg(int impl) {
  if (impl < 0 || impl > static_cast<int>(dev::VerifyImpl::Stride))
    throw py::value_error(strfmt("verify: impl %d is not 0 (auto), 1 (lds8) or 2 (stride); round 5 removed the "
                                 "other variants (parse_verify_impl names them)", impl));
  return static_cast<dev::VerifyImpl>(impl);
}

// 0 (the kernel by size), 4 or 8 (that template at any size); checked before
// any device work.
int lds_stages_arg(int lds_stages) {
  if (lds_stages != 0 && lds_stages != 4 && lds_stages != 8)
    throw py::value_error(strfmt("verify: lds_stages %d is not 0 (by size), 4 or 8", lds_stages));
  return lds_stages;
}

py::tuple device_verify(uintptr_t ptr, size_t bytes, uint64_t seed, int impl, bool check, uintptr_t stream,
                        unsigned max_grid, int lds_stages) {
  const dev::VerifyImpl vi = verify_impl_arg(impl);
  lds_stages_arg(lds_stages);
  DeviceChecks& c = checks_for_current_device();
  hipStream_t st = as_stream(stream);
  {
    py::gil_scoped_release nogil;
    c.verify_enqueue(reinterpret_cast<const void*>(ptr), bytes, seed, st, vi, check, max_grid, lds_stages, true);
    stream_wait(st)();
  }
  const VerifyResult r = c.verify_result();
  return py::make_tuple(r.mismatches, r.checksum, r.first_bad);
}

// The batched verify on raw pointers, always the batched kernel:
// [(mismatches, checksum, first_bad)] per (ptr, bytes, seed) job, one
// readback; readback = false: stream-ordered launches only (timing with
// events), nothing returned.
py::list device_verify_many(const std::vector<std::tuple<uintptr_t, size_t, uint64_t>>& jobs, uintptr_t stream,
                            bool readback) {
  dev::BatchVerifier& bv = checks_for_current_device().batch();
  std::vector<VerifyJob> dj;
  for (const auto& j : jobs) dj.push_back({reinterpret_cast<const void*>(std::get<0>(j)), std::get<1>(j), std::get<2>(j)});
  hipStream_t st = as_stream(stream);
  py::list out;
  {
    py::gil_scoped_release nogil;
    bv.enqueue(dj.data(), static_cast<int>(dj.size()), st, stream_wait(st), readback);
    if (readback) stream_wait(st)();
  }
  for (size_t i = 0; readback && i < dj.size(); ++i)
    out.append(py::make_tuple(bv.results()[i].mismatches, bv.results()[i].checksum, bv.results()[i].first_bad));
  return out;
}

// ---- checked copy (kernels.hpp CheckedCopyOp) on raw pointers ----
// (dst, src, bytes, seed, stream_offset, record_index)
using CheckedOpTuple = std::tuple<uintptr_t, uintptr_t, size_t, uint64_t, uint64_t, int>;

// The distinct record indices of `ops`, ascending; every argument is checked
// here, before any device work.
std::vector<int> checked_record_indices(const std::vector<CheckedOpTuple>& ops) {
  std::vector<int> idx;
  for (const auto& o : ops) {
    if (std::get<4>(o) % 4096)
      throw py::value_error(strfmt("copy_checked: stream_offset %llu is not a multiple of 4096",
                                   static_cast<unsigned long long>(std::get<4>(o))));
    if (std::get<5>(o) < 0) throw py::value_error("copy_checked: a record index is >= 0");
    idx.push_back(std::get<5>(o));
  }
  std::sort(idx.begin(), idx.end());
  idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
  return idx;
}

std::vector<dev::CheckedCopyOp> checked_ops_arg(const std::vector<CheckedOpTuple>& ops, const std::vector<int>& idx,
                                                const DeviceChecks& checks, bool coherent) {
  std::vector<dev::CheckedCopyOp> v;
  for (const auto& o : ops) {
    dev::CheckedCopyOp c;
    c.src = reinterpret_cast<const void*>(std::get<1>(o));
    c.dst = reinterpret_cast<void*>(std::get<0>(o));
    c.bytes = std::get<2>(o);
    c.coherent = coherent;
    c.seed = std::get<3>(o);
    c.stream_offset = std::get<4>(o);
    c.record = checks.record(static_cast<size_t>(std::lower_bound(idx.begin(), idx.end(), std::get<5>(o)) - idx.begin()));
    v.push_back(c);
  }
  return v;
}

py::list device_copy_checked(const std::vector<CheckedOpTuple>& ops, uintptr_t stream, bool coherent, int max_blocks,
                             int accumulate_launches) {
  if (accumulate_launches < 1) throw py::value_error("copy_checked: accumulate_launches is >= 1");
  const std::vector<int> idx = checked_record_indices(ops);
  std::vector<Transport::InlineCheck> host;
  if (!idx.empty()) {
    DeviceChecks& c = checks_for_current_device();
    hipStream_t st = as_stream(stream);
    py::gil_scoped_release nogil;
    c.records_begin(idx.size(), st, stream_wait(st));
    const std::vector<dev::CheckedCopyOp> v = checked_ops_arg(ops, idx, c, coherent);
    for (int k = 0; k < accumulate_launches; ++k)
      dev::launch_multi_copy_checked(v.data(), static_cast<int>(v.size()), st, max_blocks);
    host = c.records_read(st, stream_wait(st));
  }
  py::list out;
  for (const auto& r : host) out.append(py::make_tuple(r.mismatches, r.first_bad));
  return out;
}

// ---- mismatch diagnosis (diagnose.hpp) ----
// Candidates cross as (seed, shift[, kind[, value]]) tuples; granule records
// as (index, first_bad, last_bad, zero, other, flipped_bits, cand0..cand5),
// damaged granules only; extents as (begin, end, zero, other, flipped_bits,
// cand0..cand5).
std::vector<DiagCandidate> candidates_arg(const std::vector<py::tuple>& in) {
  if (in.size() > static_cast<size_t>(kMaxDiagCandidates))
    throw py::value_error(strfmt("diagnose: at most %d candidates", kMaxDiagCandidates));
  std::vector<DiagCandidate> out;
  for (const py::tuple& t : in) {
    if (t.size() < 2 || t.size() > 4) throw py::value_error("diagnose: a candidate is (seed, shift[, kind[, value]])");
    DiagCandidate c;
    c.seed = t[0].cast<uint64_t>();
    c.shift = t[1].cast<int64_t>();
    if (t.size() > 2) c.kind = t[2].cast<int>();
    if (t.size() > 3) c.value = t[3].cast<int64_t>();
    if (c.shift % 16) throw py::value_error("diagnose: a candidate's shift must be a multiple of 16 bytes");
    out.push_back(c);
  }
  return out;
}

size_t granule_arg(size_t granule, size_t bytes) {
  if (!granule) return diagnose_granule(bytes);
  if (granule < kMinDiagGranule || (granule & (granule - 1)))
    throw py::value_error("diagnose: the granule must be a power of two, at least 4 KiB");
  return granule;
}

py::list records_py(const DiagRecord* recs, size_t n) {
  py::list out;
  for (size_t i = 0; i < n; ++i) {
    const DiagRecord& r = recs[i];
    if (!r.damaged()) continue;
    out.append(py::make_tuple(i, r.first_bad(), r.last_bad(), r.zero, r.other, r.flipped_bits, r.cand[0], r.cand[1],
                              r.cand[2], r.cand[3], r.cand[4], r.cand[5]));
  }
  return out;
}

py::tuple extent_py(const DiagExtent& e) {
  return py::make_tuple(e.begin, e.end, e.zero, e.other, e.flipped_bits, e.cand[0], e.cand[1], e.cand[2], e.cand[3],
                        e.cand[4], e.cand[5]);
}

// The kernel and, with readback, one copy of its records and the wait:
// returns the damaged granules (none without readback: launch only).
py::list device_diagnose(uintptr_t ptr, size_t bytes, uint64_t seed, const std::vector<py::tuple>& candidates,
                         size_t granule, uintptr_t stream, unsigned max_grid, bool readback) {
  const std::vector<DiagCandidate> c = candidates_arg(candidates);
  granule = granule_arg(granule, bytes);
  dev::Diagnoser& dg = checks_for_current_device().diagnoser();
  hipStream_t st = as_stream(stream);
  {
    py::gil_scoped_release nogil;
    dg.enqueue(reinterpret_cast<const void*>(ptr), bytes, seed, c.data(), static_cast<int>(c.size()), granule, st,
               stream_wait(st), max_grid, readback);
    if (readback) stream_wait(st)();
  }
  return readback ? records_py(dg.records(), dg.count()) : py::list();
}

py::list merge_extents_py(const std::vector<py::tuple>& records, size_t bytes, size_t granule) {
  granule = granule_arg(granule, bytes);
  std::vector<DiagRecord> dense(diagnose_records(bytes, granule), DiagRecord{});
  for (const py::tuple& t : records) {
    if (t.size() != 6 + kMaxDiagCandidates) throw py::value_error("merge_extents: a record has 12 fields");
    const size_t i = t[0].cast<size_t>();
    if (i >= dense.size()) throw py::value_error("merge_extents: record index past the buffer");
    DiagRecord& r = dense[i];
    r.first_enc = ~t[1].cast<uint64_t>();
    r.last_enc = t[2].cast<uint64_t>() + 1;
    r.zero = t[3].cast<uint64_t>();
    r.other = t[4].cast<uint64_t>();
    r.flipped_bits = t[5].cast<uint64_t>();
    for (int k = 0; k < kMaxDiagCandidates; ++k) r.cand[k] = t[6 + static_cast<size_t>(k)].cast<uint64_t>();
  }
  py::list out;
  for (const DiagExtent& e : merge_extents(dense.data(), dense.size(), bytes, granule)) out.append(extent_py(e));
  return out;
}

std::string describe_extent_py(const py::tuple& t, size_t bytes, const std::vector<py::tuple>& candidates) {
  if (t.size() != 5 + kMaxDiagCandidates) throw py::value_error("describe_extent: an extent has 11 fields");
  const std::vector<DiagCandidate> c = candidates_arg(candidates);
  DiagExtent e;
  e.begin = t[0].cast<uint64_t>();
  e.end = t[1].cast<uint64_t>();
  e.zero = t[2].cast<uint64_t>();
  e.other = t[3].cast<uint64_t>();
  e.flipped_bits = t[4].cast<uint64_t>();
  for (int k = 0; k < kMaxDiagCandidates; ++k) e.cand[k] = t[5 + static_cast<size_t>(k)].cast<uint64_t>();
  return describe_extent(e, bytes, c.data(), static_cast<int>(c.size()));
}

// ---- the ping-pong and signal kernels on raw pointers (pingpong.hip) ----
// Launch only, like copy and verify_launch; every argument is checked before
// anything touches the device, so a bad call raises ValueError and launches
// nothing.
uintptr_t pointer_arg(uintptr_t p, size_t align, const char* what) {
  if (!p) throw py::value_error(strfmt("%s is a null pointer", what));
  if (p % align) throw py::value_error(strfmt("%s must be %zu-byte aligned", what, align));
  return p;
}

using FlagList = std::vector<std::pair<uintptr_t, uint64_t>>;

// Entries past the lists do not stay null: they point at trap_flag, with a
// post value that shows (0xDEAD) and a wait value no flag reaches, so a
// kernel that went past nposts / nwaits leaves a wrong word or an expired
// deadline behind, not a fault.  Without a trap flag both lists must be full.
dev::SignalArgs signal_args(const FlagList& posts, const FlagList& waits, uintptr_t status, uint64_t timeout_ticks,
                            bool release_first, uintptr_t trap_flag) {
  constexpr size_t kMax = static_cast<size_t>(dev::kMaxSignals);
  if (posts.size() > kMax || waits.size() > kMax)
    throw py::value_error(strfmt("signal: at most %d posts and %d waits", dev::kMaxSignals, dev::kMaxSignals));
  if (!trap_flag && (posts.size() != kMax || waits.size() != kMax))
    throw py::value_error(strfmt("signal: without a trap_flag all %d posts and all %d waits must be given",
                                 dev::kMaxSignals, dev::kMaxSignals));
  if (trap_flag) pointer_arg(trap_flag, 8, "signal: trap_flag");
  dev::SignalArgs a{};
  for (size_t i = 0; i < kMax; ++i) {
    const bool post = i < posts.size(), wait = i < waits.size();
    a.post_flag[i] = reinterpret_cast<unsigned long long*>(post ? pointer_arg(posts[i].first, 8, "signal: a post flag")
                                                                : trap_flag);
    a.post_value[i] = post ? posts[i].second : 0xDEADull;
    a.wait_flag[i] = reinterpret_cast<const unsigned long long*>(
        wait ? pointer_arg(waits[i].first, 8, "signal: a wait flag") : trap_flag);
    a.wait_value[i] = wait ? waits[i].second : ~0ull;
  }
  a.nposts = static_cast<int>(posts.size());
  a.nwaits = static_cast<int>(waits.size());
  a.release_first = release_first ? 1 : 0;
  a.status = reinterpret_cast<unsigned int*>(pointer_arg(status, 4, "signal: status_ptr"));
  a.timeout_ticks = timeout_ticks;
  return a;
}

// A role as a dict (a dict, what dict() accepts, or a named tuple) whose keys
// are all among `fields`; `what` names the call in the error.
py::dict role_dict(const py::object& role, const char* what, std::initializer_list<const char*> fields) {
  py::dict d;
  if (py::isinstance<py::dict>(role))
    d = role.cast<py::dict>();
  else if (py::hasattr(role, "_asdict"))
    d = py::dict(role.attr("_asdict")());
  else
    d = py::dict(role);
  for (const auto& kv : d) {
    const std::string key = py::str(kv.first);
    bool known = false;
    for (const char* f : fields) known = known || key == f;
    if (!known) throw py::value_error(std::string(what) + ": a role has no field '" + key + "'");
  }
  return d;
}
// Field `key` of such a dict as an unsigned integer; 0 where an optional one is absent.
uint64_t role_field(const py::dict& d, const char* what, const char* key, bool required) {
  if (!d.contains(key)) {
    if (required) throw py::value_error(strfmt("%s: a role needs '%s'", what, key));
    return 0;
  }
  return d[key].cast<uint64_t>();
}

// A role is a dict of the PingRole fields (role_dict);
// base, in_base, leader and stamps default to 0, and only a
// leader needs stamps.
dev::PingRole ping_role_arg(const py::object& role) {
  const py::dict d = role_dict(role, "pingpong", {"out_flag", "out_payload", "in_flag", "in_payload", "bytes", "base", "in_base",
                                                  "iters", "leader", "stamps", "status", "timeout_ticks"});
  auto get = [&d](const char* key, bool required) { return role_field(d, "pingpong", key, required); };
  dev::PingRole r{};
  r.bytes = get("bytes", true);
  if (r.bytes < 16 || r.bytes % 16) throw py::value_error("pingpong: bytes must be a multiple of 16, at least 16");
  const long long iters = d.contains("iters") ? d["iters"].cast<long long>() : 0;
  if (iters < 1 || iters > INT32_MAX) throw py::value_error("pingpong: iters must be at least 1");
  r.iters = static_cast<int>(iters);
  r.leader = get("leader", false) ? 1 : 0;
  r.base = get("base", false);
  r.in_base = get("in_base", false);
  r.timeout_ticks = get("timeout_ticks", true);
  r.out_flag = reinterpret_cast<unsigned long long*>(pointer_arg(get("out_flag", true), 8, "pingpong: out_flag"));
  r.out_payload = reinterpret_cast<unsigned char*>(pointer_arg(get("out_payload", true), 16, "pingpong: out_payload"));
  r.in_flag = reinterpret_cast<const unsigned long long*>(pointer_arg(get("in_flag", true), 8, "pingpong: in_flag"));
  r.in_payload = reinterpret_cast<const unsigned char*>(pointer_arg(get("in_payload", true), 16, "pingpong: in_payload"));
  r.status = reinterpret_cast<unsigned int*>(pointer_arg(get("status", true), 4, "pingpong: status"));
  const uintptr_t stamps = get("stamps", false);
  if (r.leader || stamps) pointer_arg(stamps, 8, "pingpong: stamps");
  r.stamps = reinterpret_cast<unsigned long long*>(stamps);
  return r;
}

// A role is a dict of the StreamRole fields; base, sender and check_all
// default to 0.
dev::StreamRole stream_role_arg(const py::object& role) {
  const py::dict d = role_dict(role, "stream", {"out_flag", "in_flag", "ring", "bytes", "base", "depth", "iters", "sender",
                                                "check_all", "stamps", "status", "timeout_ticks"});
  auto get = [&d](const char* key, bool required) { return role_field(d, "stream", key, required); };
  dev::StreamRole r{};
  r.bytes = get("bytes", true);
  if (r.bytes < 16 || r.bytes % 16 || r.bytes > dev::kMaxStreamBytes)
    throw py::value_error("stream: bytes must be a multiple of 16, 16 .. 1 MiB");
  const uint64_t depth = get("depth", true), iters = get("iters", true);
  if (depth < 1 || depth > static_cast<uint64_t>(dev::kMaxStreamDepth)) throw py::value_error("stream: depth must be 1 .. 64");
  if (depth * r.bytes > dev::kMaxStreamRingBytes) throw py::value_error("stream: depth x bytes is at most 4 MiB");
  if (iters < 1 || iters > static_cast<uint64_t>(dev::kMaxStreamIters)) throw py::value_error("stream: iters must be 1 .. 100000");
  r.depth = static_cast<int>(depth);
  r.iters = static_cast<int>(iters);
  r.sender = get("sender", false) ? 1 : 0;
  r.check_all = get("check_all", false) ? 1 : 0;
  r.base = get("base", false);
  r.timeout_ticks = get("timeout_ticks", true);
  r.out_flag = reinterpret_cast<unsigned long long*>(pointer_arg(get("out_flag", true), 8, "stream: out_flag"));
  r.in_flag = reinterpret_cast<const unsigned long long*>(pointer_arg(get("in_flag", true), 8, "stream: in_flag"));
  r.ring = reinterpret_cast<unsigned char*>(pointer_arg(get("ring", true), 16, "stream: ring"));
  r.stamps = reinterpret_cast<unsigned long long*>(pointer_arg(get("stamps", true), 8, "stream: stamps"));
  r.status = reinterpret_cast<unsigned int*>(pointer_arg(get("status", true), 4, "stream: status"));
  return r;
}

// stream_layout.hpp as a dict: the sizes, and every region as (name, offset,
// bytes): "tail r.c" and "ring r.c" per source and channel, then "credit";
// "head" lists the credit lines' offsets per destination and channel.
py::dict stream_layout_py(int n, int channels, int depth, size_t bytes) {
  StreamLayout l;
  try {
    l = stream_layout(n, channels, depth, bytes);
  } catch (const Error& e) {
    throw py::value_error(e.what());
  }
  py::list regions, tails, rings, heads;
  for (int r = 0; r <= n; ++r) {
    py::list tr, rr, hr;
    for (int c = 0; c < channels; ++c) {
      regions.append(py::make_tuple(strfmt("tail %d.%d", r, c), l.tail(r, c), StreamLayout::kHeader));
      regions.append(py::make_tuple(strfmt("ring %d.%d", r, c), l.ring(r, c), l.ring_bytes));
      tr.append(l.tail(r, c));
      rr.append(l.ring(r, c));
      hr.append(l.head(r, c));
    }
    tails.append(tr);
    rings.append(rr);
    heads.append(hr);
  }
  regions.append(py::make_tuple("credit", l.credit_offset, l.credit_bytes));
  py::dict d;
  d["n"] = l.n;
  d["channels"] = l.channels;
  d["depth"] = l.depth;
  d["bytes"] = l.bytes;
  d["ring_bytes"] = l.ring_bytes;
  d["header_bytes"] = StreamLayout::kHeader;
  d["credit_line"] = StreamLayout::kCreditLine;
  d["credit_offset"] = l.credit_offset;
  d["credit_bytes"] = l.credit_bytes;
  d["total"] = l.total;
  d["cap"] = StreamLayout::kPageCap;
  d["self_slot"] = l.n;
  d["regions"] = regions;
  d["tail"] = tails;
  d["ring"] = rings;
  d["head"] = heads;
  return d;
}

void launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) P2P_FATAL(strfmt("%s: launch failed: %s", what, hipGetErrorString(e)));
}

// One allocation made as the transports make their signal pages.
class SignalPage {
 public:
  explicit SignalPage(size_t bytes) : bytes_(bytes) {
    if (!bytes) throw py::value_error("signal_page: bytes must be positive");
    const hipError_t e = dev::alloc_signal_page(&p_, bytes, &uncached_);
    if (e != hipSuccess) P2P_FATAL(strfmt("signal_page: allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e)));
  }
  SignalPage(const SignalPage&) = delete;
  SignalPage& operator=(const SignalPage&) = delete;
  ~SignalPage() {
    if (p_) (void)hipFree(p_);
  }
  uintptr_t ptr() const { return reinterpret_cast<uintptr_t>(p_); }
  size_t bytes() const { return bytes_; }
  bool uncached() const { return uncached_; }

 private:
  void* p_ = nullptr;
  size_t bytes_;
  bool uncached_ = false;
};

// n 64-byte lines of fine-grained (coherent) pinned host memory, the stream
// gate's kind: what the host writes while a kernel spins on it.
class HostWords {
 public:
  static constexpr size_t kLine = 64;
  explicit HostWords(size_t n) : n_(n) {
    if (!n) throw py::value_error("HostWords: at least one line");
    const hipError_t e = hipHostMalloc(&p_, n * kLine, hipHostMallocCoherent);
    if (e != hipSuccess) P2P_FATAL(strfmt("HostWords: hipHostMalloc failed: %s", hipGetErrorString(e)));
    for (size_t i = 0; i < n; ++i) store(i, 0);
  }
  HostWords(const HostWords&) = delete;
  HostWords& operator=(const HostWords&) = delete;
  ~HostWords() {
    if (p_) (void)hipHostFree(p_);
  }
  size_t size() const { return n_; }
  uintptr_t ptr(size_t i) const { return reinterpret_cast<uintptr_t>(line(i)); }
  uint64_t load(size_t i) const { return __atomic_load_n(line(i), __ATOMIC_ACQUIRE); }
  void store(size_t i, uint64_t v) { __atomic_store_n(line(i), v, __ATOMIC_RELEASE); }

 private:
  uint64_t* line(size_t i) const {
    if (i >= n_) throw py::index_error(strfmt("HostWords: line %zu of %zu", i, n_));
    return reinterpret_cast<uint64_t*>(static_cast<unsigned char*>(p_) + i * kLine);
  }
  void* p_ = nullptr;
  size_t n_;
};

// ---- the background-load kernels on raw pointers, and BackgroundLoad ----
dev::LoadCtl load_ctl_arg(uintptr_t cancel, uintptr_t done, uintptr_t tickets, uint64_t ordinal) {
  if (done && !tickets) throw py::value_error("load: done_ptr needs tickets_ptr (the launch's ticket counter)");
  dev::LoadCtl c;
  if (cancel) c.cancel = reinterpret_cast<const unsigned int*>(pointer_arg(cancel, 4, "load: cancel_ptr"));
  if (done) c.done = reinterpret_cast<unsigned long long*>(pointer_arg(done, 8, "load: done_ptr"));
  if (tickets) c.tickets = reinterpret_cast<unsigned long long*>(pointer_arg(tickets, 8, "load: tickets_ptr"));
  c.ordinal = ordinal;
  return c;
}

py::dict load_stats_py(const LoadStats& s) {
  py::dict d;
  d["launches"] = s.launches;
  d["launches_done"] = s.launches_done;
  d["window_launches"] = s.window_launches;
  d["window_s"] = s.window_s;
  d["during_rate"] = s.during_rate;
  d["covered"] = s.covered;
  return d;
}

// A load on the current device, as the GPU transports hand one out.
class PyBackgroundLoad {
 public:
  PyBackgroundLoad(const std::string& kind, int wgs, double timeout_s) {
    if (kind != "mfma" && kind != "hbm") throw py::value_error("BackgroundLoad: kind must be 'mfma' or 'hbm'");
    if (wgs < 0) throw py::value_error("BackgroundLoad: wgs must be >= 1 (0: one per CU)");
    load_ = make_background_load(kind, wgs, timeout_s);
  }
  ~PyBackgroundLoad() {
    teardown_outside_gil([this] { load_.reset(); });
  }
  BackgroundLoad& l() { return *load_; }

 private:
  std::unique_ptr<BackgroundLoad> load_;
};

// report.hpp load_table of a hand-built loaded record: phases are dicts of
// label, agg_gbs and the phase's "load" keys (docs/OUTPUT.md).
std::string load_table_py(const std::string& kind, int wgs, double launch_us, double alone_rate, const std::string& unit,
                          const std::vector<py::dict>& phases) {
  RunRecord rec{};
  rec.load.kind = kind;
  rec.load.wgs = wgs;
  rec.load.launch_us = launch_us;
  rec.load.alone_rate = alone_rate;
  rec.load.unit = unit;
  for (const py::dict& d : phases) {
    PhaseResult ph;
    ph.label = d["label"].cast<std::string>();
    ph.agg_gbs = d["agg_gbs"].cast<double>();
    const py::dict l = d["load"].cast<py::dict>();
    ph.load.present = true;
    ph.load.quiet_agg_gbs = l["quiet_agg_gbs"].cast<double>();
    ph.load.launches = l["launches"].cast<long>();
    ph.load.launches_done = l["launches_done"].cast<long>();
    ph.load.window_launches = l["window_launches"].cast<long>();
    ph.load.window_s = l["window_s"].cast<double>();
    ph.load.during_rate = l["during_rate"].cast<double>();
    ph.load.covered = l["covered"].cast<bool>();
    ph.load.ranks = l["ranks"].cast<std::vector<int>>();
    rec.phases.push_back(ph);
  }
  return load_table(rec);
}

py::list schedule_py(const std::string& mode, const std::string& dir, int n) {
  Schedule s = make_schedule(parse_mode(mode), parse_direction(dir), n);
  py::list phases;
  for (const auto& p : s.phases) {
    py::dict d;
    d["label"] = p.label;
    d["row"] = p.row;
    d["col"] = p.col;
    d["idle"] = p.idle;
    py::list flows;
    for (const auto& f : p.flows) flows.append(py::make_tuple(f.src, f.dst));
    d["flows"] = flows;
    py::list ranks;
    for (const auto& r : p.ranks) ranks.append(py::make_tuple(r.send_to, r.recv_from));
    d["ranks"] = ranks;
    phases.append(d);
  }
  return phases;
}

}  // namespace

PYBIND11_MODULE(_p2pcore, m) {
  m.doc() = "MI355X-native P2P benchmark engine (RCCL over xGMI, gfx950 kernels)";
  set_throw_on_fatal(true);

  py::class_<TcpListener>(m, "TcpListener")
      .def(py::init<int, const std::string&>(), py::arg("port") = 0, py::arg("bind_addr") = "0.0.0.0")
      .def_property_readonly("port", &TcpListener::port);

  py::class_<Session, std::shared_ptr<Session>>(m, "Session")
      .def(py::init<int, int, const std::string&, int, int, const std::string&, double, TcpListener*>(), py::arg("rank"),
           py::arg("world"), py::arg("host") = "127.0.0.1", py::arg("port") = 0, py::arg("device") = 0,
           py::arg("transport") = "rccl", py::arg("timeout_s") = 300.0, py::arg("listener") = nullptr,
           py::call_guard<NativeCall, py::gil_scoped_release>())
      .def_property_readonly("rank", &Session::rank)
      .def_property_readonly("world", &Session::world)
      .def_property_readonly("transport", &Session::transport)
      .def_property_readonly("device_desc", &Session::device_desc)
      .def("barrier", &Session::barrier, py::call_guard<NativeCall, py::gil_scoped_release>())
      .def("allreduce_max", &Session::allreduce_max, py::call_guard<NativeCall, py::gil_scoped_release>())
      .def("allreduce_sum", &Session::allreduce_sum, py::call_guard<NativeCall, py::gil_scoped_release>())
      .def("run", &Session::run, py::arg("mode") = "pair", py::arg("dir") = "uni", py::arg("bytes") = 32u << 20,
           py::arg("iters") = 128, py::arg("warmup") = 8, py::arg("timing") = "events", py::arg("verify") = false,
           py::arg("warm") = true, py::arg("cells") = std::vector<std::pair<int, int>>{}, py::arg("diagnose") = 0,
           py::arg("inline_check") = false, py::arg("load") = "",
           py::call_guard<NativeCall, py::gil_scoped_release>())
      .def("gate_probe", &Session::gate_probe, py::arg("timeout_s") = 0.2, py::arg("release") = true,
           py::call_guard<NativeCall, py::gil_scoped_release>())
      .def("device_latency", &Session::device_latency, py::arg("bytes") = 8, py::arg("iters") = 1000,
           py::arg("warmup") = 100, py::call_guard<NativeCall, py::gil_scoped_release>())
      .def("device_stream", &Session::device_stream, py::arg("sizes"), py::arg("depth") = 8, py::arg("channels") = 1,
           py::arg("iters") = 2000, py::arg("dir") = "uni", py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Device-initiated stream (collective; one-sided transports): per flow `channels` credit-flow rings of `depth` "
           "slots, one sender and one receiver wave each.  dir uni | bi | both.  JSON list, one device_stream object per "
           "(direction form, size).")
      .def("latency", &Session::latency, py::arg("bytes") = 8, py::arg("iters") = 1000, py::arg("warmup") = 100,
           py::arg("preposted") = 0, py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Ping-pong matrix (collective).  preposted=B: exchanges posted B at a time behind a stream gate and "
           "released together (GPU-timeline latency; host-posted where the transport has no gate).")
      .def("fuzz", &Session::fuzz, py::arg("rounds") = 20, py::arg("seed") = 1, py::arg("max_bytes") = size_t{4} << 20,
           py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Random groups of verified messages through the transport (collective); returns mismatching words.")
      .def("ring_latency", &Session::ring_latency, py::arg("bytes") = 8, py::arg("laps") = 200, py::arg("warmup") = 20,
           py::arg("device") = false, py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Dependent ring token chain 0 -> 1 -> ... -> 0 (collective); JSON with per-hop and per-lap times.")
      .def("set_timeout", &Session::set_timeout, py::arg("seconds"),
           "Bounds every later wait of the session (transport sync / rendezvous, bootstrap receives).")
      .def("set_chunk_cap", &Session::set_chunk_cap, py::arg("bytes"),
           "Caps the ops messages to every peer are posted as at `bytes` (0: lifts the cap, back to the limits the "
           "transport derived per peer); False where nothing is split. Call it on every rank with the same value.")
      .def("max_chunk", &Session::max_chunk, py::arg("peer"), "Largest op a message to `peer` is posted as (0: unsplit).")
      .def("refine_op_limits", &Session::refine_op_limits, py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Collective: op limits from the connections made so far (RCCL: its connection lines).")
      .def("link_reports", &Session::link_reports, py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Collective: what the data plane set up towards each peer, per rank (RCCL: p2p channels from its INFO log, "
           "each peer's transport, the op limit in use); JSON list.")
      .def("provenance", &Session::provenance, py::arg("device") = -1, py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Collective: runtime, RCCL library, knobs, every rank's GPU and the links between them (JSON).")
      .def("_post_unmatched_recv", &Session::post_unmatched_recv, py::arg("bytes"), py::arg("peer"),
           py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Test hook: a receive no send matches, left pending; the session's teardown must still end.")
      .def("_unmatched_recv", &Session::unmatched_recv, py::arg("bytes") = size_t{1} << 20,
           py::call_guard<NativeCall, py::gil_scoped_release>(), "Test hook: a receive no send matches; returns the watchdog's error.")
      .def("_mark", &Session::mark, py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Test hook: a timestamp of the transport behind all work posted so far; returns its id.")
      .def("_elapsed_ms", &Session::elapsed_ms, py::arg("a"), py::arg("b"),
           py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Test hook: milliseconds between two marks of the transport; valid after a sync.")
      .def("_clear_marks", &Session::clear_marks, py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Test hook: forget the transport's marks (their ids are handed out again).")
      .def("_gate_arm", &Session::gate_arm, py::arg("timeout_s"), py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Test hook: hold the transport's stream until _gate_release() or `timeout_s`; False where there is no gate.")
      .def("_gate_release", &Session::gate_release, py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Test hook: let every armed gate pass.")
      .def("_gate_timed_out", &Session::gate_timed_out, py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Test hook: did a gate expire instead of being released? Call it after a sync.")
      .def("_stream_idle", &Session::stream_idle, py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Test hook: has the transport's stream finished everything posted so far? Never waits.")
      .def("_async_error", &Session::async_error, py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Test hook: the transport's asynchronous error, '' when there is none.");

  py::class_<PyStepDriver>(m, "StepDriver")
      .def(py::init<std::shared_ptr<Session>, const std::string&, const std::string&, size_t, int, bool, bool, bool, int,
                    size_t, uint64_t>(),
           py::arg("session"), py::arg("mode") = "tournament", py::arg("dir") = "bi", py::arg("bytes") = 32u << 20,
           py::arg("msgs") = 8, py::arg("verify") = false, py::arg("batch") = false, py::arg("graph") = false,
           py::arg("depth") = 1, py::arg("recv_budget") = size_t{0}, py::arg("salt") = uint64_t{0},
           py::call_guard<NativeCall, py::gil_scoped_release>())
      .def("poison", [](PyStepDriver& s) { s.d().poison(); }, py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Collective: zero every receive slot (after the warmup, before the timed steps) and arm the skip faults.")
      .def("clear", [](PyStepDriver& s) { s.d().clear(); }, py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Collective: zero every receive slot once every rank has drained (no fault armed).")
      .def("recapture", [](PyStepDriver& s) { s.d().recapture(); }, py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Collective: record the step graphs again after the op sizes changed (no-op without graphs).")
      .def_property_readonly("recaptures", [](PyStepDriver& s) { return s.d().recaptures(); })
      .def_property_readonly("limit_changes", [](PyStepDriver& s) { return s.d().limit_changes(); })
      .def_property_readonly("graphs", [](PyStepDriver& s) { return s.d().graphs(); })
      .def("verify_steps", [](PyStepDriver& s, long first, long count) {
            StepVerifyReport r;
            {
              NativeCall in_engine;
              py::gil_scoped_release nogil;
              r = s.d().verify_steps(first, count);
            }
            py::dict d;
            d["mismatches"] = r.mismatches;
            d["verified_msgs"] = r.verified_msgs;
            d["timed_msgs"] = r.timed_msgs;
            d["slots"] = r.slots;
            return d;
          }, py::arg("first"), py::arg("count"),
           "Collective: checks every receive slot steps [first, first+count) wrote (all ranks' totals).")
      .def("flows_per_step", [](PyStepDriver& s, long k) { return s.d().flows_per_step(k); })
      .def_property_readonly("depth", [](PyStepDriver& s) { return s.d().depth(); })
      .def_property_readonly("msgs", [](PyStepDriver& s) { return s.d().msgs(); })
      .def_property_readonly("recv_bytes", [](PyStepDriver& s) { return s.d().recv_bytes(); })
      .def("connect", [](PyStepDriver& s) { s.d().connect(); }, py::call_guard<NativeCall, py::gil_scoped_release>())
      .def("step", [](PyStepDriver& s, long k) { s.d().step(k); }, py::call_guard<NativeCall, py::gil_scoped_release>())
      .def("run_steps", [](PyStepDriver& s, long first, long count) { s.d().run_steps(first, count); },
           py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Enqueue steps [first, first+count); consecutive steps share their boundary timestamp.")
      .def("sync", [](PyStepDriver& s) { s.d().sync(); }, py::call_guard<NativeCall, py::gil_scoped_release>())
      .def("step_ms", [](PyStepDriver& s) { return s.d().step_ms(); })
      .def("post_ms", [](PyStepDriver& s) { return s.d().post_ms(); },
           "Host time each recorded step took to post (ms).")
      .def("reset", [](PyStepDriver& s) { s.d().reset(); })
      .def("verify_last", [](PyStepDriver& s) { return s.d().verify_last(); }, py::call_guard<NativeCall, py::gil_scoped_release>())
      .def("deliveries", [](PyStepDriver& s, long k) {
            std::vector<std::tuple<uintptr_t, size_t, int, int>> out;
            for (const auto& x : s.d().deliveries(k))
              out.emplace_back(reinterpret_cast<uintptr_t>(x.p), s.d().msg_bytes(), x.src, x.msg);
            return out;
          }, py::arg("step"),
           "This rank's receive slots of step `step`, in message order: [(address, bytes, sender, message)] "
           "(read them after sync()).")
      .def("msg_seed", [](PyStepDriver& s, int src, int msg) { return s.d().msg_seed(src, msg); }, py::arg("src"),
           py::arg("msg"), "PRNG stream of message `msg` as rank `src` sends it (what a delivery must hold).")
      .def("bytes_sent_per_step", [](PyStepDriver& s, long k) { return s.d().bytes_sent_per_step(k); })
      .def("job_bytes_per_step", [](PyStepDriver& s, long k) { return s.d().job_bytes_per_step(k); })
      .def_property_readonly("phases", [](PyStepDriver& s) { return s.d().phases(); })
      .def("phase_flows", [](PyStepDriver& s, long k) {
        const auto& p = s.d().schedule().phases[static_cast<size_t>(k % s.d().phases())];
        std::vector<std::pair<int, int>> f;
        for (auto& x : p.flows) f.emplace_back(x.src, x.dst);
        return f;
      });

  // ---- kernels on raw pointers ----
  m.def("fill", [](uintptr_t ptr, size_t bytes, uint64_t seed, uintptr_t stream, int impl) {
        if (impl >= 2 && impl <= 6)
          throw py::value_error(strfmt("fill: impl %d (non-temporal / grid-stride / XCD-ordered / 2 or 4 stores per "
                                       "lane) was removed in round 5: it lost its A/B against the full grid "
                                       "(profiles/r3b_nt_ab/, r4_gpu_tier/); use 0 or 1", impl));
        if (impl < 0 || impl > static_cast<int>(dev::FillImpl::Grid)) throw py::value_error("fill: unknown impl");
        dev::launch_fill(reinterpret_cast<void*>(ptr), bytes, seed, as_stream(stream), static_cast<dev::FillImpl>(impl));
      }, py::arg("ptr"), py::arg("bytes"), py::arg("seed"), py::arg("stream") = 0, py::arg("impl") = 0,
      "impl: 0 auto = 1 full grid (one 16 B store per lane, one 4 KiB block per workgroup)");
  m.def("verify", &device_verify, py::arg("ptr"), py::arg("bytes"), py::arg("seed"), py::arg("impl") = 0,
        py::arg("check") = true, py::arg("stream") = 0, py::arg("max_grid") = 0, py::arg("lds_stages") = 0,
        "impl: 0 auto (= 1), 1 LDS-DMA staged (lds8), 2 register staged (stride).  max_grid > 0 caps the workgroup "
        "count; lds_stages 4 or 8 forces that LDS-staged kernel (0: by size).  Returns (mismatching words, "
        "checksum, first bad byte offset or 2**64-1).");
  m.def("verify_many", [](const std::vector<std::tuple<uintptr_t, size_t, uint64_t>>& jobs, uintptr_t stream) {
        return device_verify_many(jobs, stream, true);
      }, py::arg("jobs"), py::arg("stream") = 0,
        "Batched verify of [(ptr, bytes, seed)]: one (mismatches, checksum, first_bad) per job, one readback.");
  m.def("verify_many_launch", [](const std::vector<std::tuple<uintptr_t, size_t, uint64_t>>& jobs, uintptr_t stream) {
        device_verify_many(jobs, stream, false);
      }, py::arg("jobs"), py::arg("stream") = 0,
        "Stream-ordered batched verify launches only (timing).");
  m.def("verify_launch", [](uintptr_t ptr, size_t bytes, uint64_t seed, int impl, bool check, uintptr_t stream,
                            unsigned max_grid, int lds_stages) {
        // Stream-ordered launch only (reset + verify + finalize), no readback:
        // for timing the kernel with events.
        const dev::VerifyImpl vi = verify_impl_arg(impl);
        lds_stages_arg(lds_stages);
        checks_for_current_device().verify_enqueue(reinterpret_cast<const void*>(ptr), bytes, seed, as_stream(stream), vi,
                                                   check, max_grid, lds_stages, false);
      }, py::arg("ptr"), py::arg("bytes"), py::arg("seed"), py::arg("impl") = 0, py::arg("check") = true,
      py::arg("stream") = 0, py::arg("max_grid") = 0, py::arg("lds_stages") = 0);
  m.def("copy", [](uintptr_t dst, uintptr_t src, size_t bytes, uintptr_t stream, int max_blocks, bool coherent) {
        dev::CopyOp op{reinterpret_cast<const void*>(src), reinterpret_cast<void*>(dst), bytes, coherent};
        dev::launch_multi_copy(&op, 1, as_stream(stream), max_blocks);
      }, py::arg("dst"), py::arg("src"), py::arg("bytes"), py::arg("stream") = 0, py::arg("max_blocks") = 0,
      py::arg("coherent") = false,
      "The IPC transport's gfx950 copy kernel on one (dst, src) pair (coherent: the cross-GPU form with "
      "system-scope sc0 sc1 buffer loads and stores).");
  m.def("copy_many", [](const std::vector<std::tuple<uintptr_t, uintptr_t, size_t>>& ops, uintptr_t stream,
                        bool coherent, int max_blocks) {
        std::vector<dev::CopyOp> v;
        for (const auto& o : ops)
          v.push_back({reinterpret_cast<const void*>(std::get<1>(o)), reinterpret_cast<void*>(std::get<0>(o)),
                       std::get<2>(o), coherent});
        dev::launch_multi_copy(v.data(), static_cast<int>(v.size()), as_stream(stream), max_blocks);
      }, py::arg("ops"), py::arg("stream") = 0, py::arg("coherent") = false, py::arg("max_blocks") = 0,
      "The copy kernel over several (dst, src, bytes) ops, as the IPC transport launches a group's receives "
      "(max_blocks > 0: the ops of a launch share that many workgroups and grid-stride).");
  m.def("copy_checked", &device_copy_checked, py::arg("ops"), py::arg("stream") = 0, py::arg("coherent") = false,
        py::arg("max_blocks") = 0, py::arg("accumulate_launches") = 1,
        "The checked copy kernel over [(dst, src, bytes, seed, stream_offset, record_index)]: every word is compared "
        "with bytes [stream_offset, stream_offset + bytes) of PRNG stream `seed` as it is copied (stream_offset a "
        "multiple of 4096).  Resets the records, launches accumulate_launches times, reads back once: one "
        "(mismatching words, first bad stream byte or 2**64-1) per distinct record index, in ascending order.");
  m.def("copy_checked_launch", [](const std::vector<CheckedOpTuple>& ops, uintptr_t stream, bool coherent, int max_blocks) {
        const std::vector<int> idx = checked_record_indices(ops);
        DeviceChecks& c = checks_for_current_device();
        c.records_begin(idx.size(), as_stream(stream), stream_wait(as_stream(stream)), false);
        const std::vector<dev::CheckedCopyOp> v = checked_ops_arg(ops, idx, c, coherent);
        dev::launch_multi_copy_checked(v.data(), static_cast<int>(v.size()), as_stream(stream), max_blocks);
      }, py::arg("ops"), py::arg("stream") = 0, py::arg("coherent") = false, py::arg("max_blocks") = 0,
      "Stream-ordered launch of the checked copy only (timing with events): no reset, no readback.");
  m.attr("MAX_SIGNALS") = dev::kMaxSignals;
  m.def("signal", [](const FlagList& posts, const FlagList& waits, uintptr_t status_ptr, uint64_t timeout_ticks,
                     bool release_first, uintptr_t stream, uintptr_t trap_flag) {
        const dev::SignalArgs a = signal_args(posts, waits, status_ptr, timeout_ticks, release_first, trap_flag);
        dev::launch_signal(a, as_stream(stream));
        launched("signal");
      }, py::arg("posts"), py::arg("waits"), py::arg("status_ptr"), py::arg("timeout_ticks"),
      py::arg("release_first") = false, py::arg("stream") = 0, py::arg("trap_flag") = 0,
      "The one-wave signal kernel (launch only): posts and waits are lists of (flag_ptr, value), at most MAX_SIGNALS "
      "each; bit 0 of the 32-bit word at status_ptr is set if a wait passed timeout_ticks.  Unused entries point at "
      "trap_flag (post value 0xDEAD, wait value 2**64-1); with trap_flag 0 both lists must be full.");
  m.def("pingpong", [](const py::object& a, const py::object& b, uintptr_t stream) {
        const dev::PingRole ra = ping_role_arg(a);
        dev::PingRole rb{};
        if (!b.is_none()) rb = ping_role_arg(b);
        dev::launch_pingpong(ra, b.is_none() ? nullptr : &rb, as_stream(stream));
        launched("pingpong");
      }, py::arg("a"), py::arg("b") = py::none(), py::arg("stream") = 0,
      "The ping-pong kernel (launch only): role a as one wave, or a and b as the two waves of one workgroup.  A role "
      "is a dict of out_flag, out_payload, in_flag, in_payload, bytes, base, in_base, iters, leader, stamps, status, "
      "timeout_ticks (pointers as integers).");
  m.attr("MAX_STREAM_ROLES") = dev::kMaxStreamRoles;
  m.def("stream", [](const std::vector<py::object>& roles, uintptr_t stream) {
        if (roles.empty() || roles.size() > static_cast<size_t>(dev::kMaxStreamRoles))
          throw py::value_error(strfmt("stream: 1 .. %d roles per launch", dev::kMaxStreamRoles));
        std::vector<dev::StreamRole> v;
        for (const py::object& r : roles) v.push_back(stream_role_arg(r));
        dev::launch_stream(v.data(), static_cast<int>(v.size()), as_stream(stream));
        launched("stream");
      }, py::arg("roles"), py::arg("stream") = 0,
      "The device-initiated stream kernel (launch only): up to MAX_STREAM_ROLES roles, one workgroup of one wave each.  "
      "A role is a dict of out_flag, in_flag, ring, bytes, base, depth, iters, sender, check_all, stamps, status, "
      "timeout_ticks (pointers as integers).");
  m.def("stream_layout", &stream_layout_py, py::arg("n"), py::arg("channels"), py::arg("depth"), py::arg("bytes"),
        "Where the device stream keeps its rings and flags in a rank's page (host code, no GPU): sizes, every region as "
        "(name, offset, bytes), and the tail / ring / head offsets per rank slot (n: the self path) and channel.  "
        "ValueError names the limit an argument breaks.");
  m.def("load_mfma", [](int wgs, uint32_t reps, uint64_t seed, uintptr_t out_ptr, uintptr_t stream, uintptr_t cancel_ptr,
                        uintptr_t done_ptr, uintptr_t tickets_ptr, uint64_t ordinal) {
        if (wgs < 1) throw py::value_error("load_mfma: wgs must be at least 1");
        const dev::LoadCtl ctl = load_ctl_arg(cancel_ptr, done_ptr, tickets_ptr, ordinal);
        dev::launch_load_mfma(wgs, reps, seed, reinterpret_cast<float*>(pointer_arg(out_ptr, 16, "load_mfma: out_ptr")), ctl,
                              as_stream(stream));
      }, py::arg("wgs"), py::arg("reps"), py::arg("seed"), py::arg("out_ptr"), py::arg("stream") = 0,
      py::arg("cancel_ptr") = 0, py::arg("done_ptr") = 0, py::arg("tickets_ptr") = 0, py::arg("ordinal") = 0,
      "The matrix-core load kernel (launch only): wgs workgroups of 4 waves, each wave reps pairs of +A.B / -A.B bf16 "
      "MFMAs and a final +A.B, its 32x32 f32 tile stored at out[(wg * 4 + wave) * 1024 + lane * 16 + reg] (wgs * 4096 "
      "floats).  cancel_ptr: a 32-bit host-pinned word, non-zero makes every workgroup return without touching out; "
      "done_ptr: a 64-bit host-pinned word that becomes ordinal + 1 when the launch's last workgroup ends; tickets_ptr: "
      "the 64-bit device counter (0 between launches) that finds that workgroup.");
  m.def("load_hbm", [](uintptr_t ptr, size_t bytes, uint32_t passes, int wgs, uintptr_t out_ptr, uintptr_t stream,
                       uintptr_t cancel_ptr, uintptr_t done_ptr, uintptr_t tickets_ptr, uint64_t ordinal) {
        if (wgs < 1) throw py::value_error("load_hbm: wgs must be at least 1");
        if (!bytes || bytes % 4096) throw py::value_error("load_hbm: bytes must be a positive multiple of 4096");
        const dev::LoadCtl ctl = load_ctl_arg(cancel_ptr, done_ptr, tickets_ptr, ordinal);
        dev::launch_load_hbm(reinterpret_cast<const void*>(pointer_arg(ptr, 16, "load_hbm: ptr")), bytes, passes, wgs,
                             reinterpret_cast<unsigned long long*>(pointer_arg(out_ptr, 8, "load_hbm: out_ptr")), ctl,
                             as_stream(stream));
      }, py::arg("ptr"), py::arg("bytes"), py::arg("passes"), py::arg("wgs"), py::arg("out_ptr"), py::arg("stream") = 0,
      py::arg("cancel_ptr") = 0, py::arg("done_ptr") = 0, py::arg("tickets_ptr") = 0, py::arg("ordinal") = 0,
      "The HBM-streaming load kernel (launch only): wgs workgroups read the buffer passes times with non-temporal 16 B "
      "loads; out[wg] is the 64-bit sum of the 32-bit words that workgroup read.  cancel_ptr, done_ptr, tickets_ptr and "
      "ordinal as in load_mfma.");
  m.def("load_plan", [](double expected_s, double launch_s) {
        const LoadPlan p = load_plan(expected_s, launch_s);
        return py::make_tuple(p.launches, p.covers_s);
      }, py::arg("expected_s"), py::arg("launch_s"),
      "The train BackgroundLoad.start enqueues: (launches, seconds they cover) = ceil(2 expected_s / launch_s) launches, "
      "at least 1 and at most MAX_LOAD_LAUNCHES.");
  m.attr("MAX_LOAD_LAUNCHES") = kMaxLoadLaunches;
  m.def("load_table", &load_table_py, py::arg("kind"), py::arg("wgs"), py::arg("launch_us"), py::arg("alone_rate"),
        py::arg("unit"), py::arg("phases"),
        "The lines the extended tables add for a loaded run (--load), from a run's \"load\" object and its phases "
        "(dicts with label, agg_gbs and load).");
  py::class_<PyBackgroundLoad>(m, "BackgroundLoad")
      .def(py::init<const std::string&, int, double>(), py::arg("kind"), py::arg("wgs") = 0, py::arg("timeout_s") = 30.0,
           py::call_guard<NativeCall, py::gil_scoped_release>())
      .def("calibrate", [](PyBackgroundLoad& b) { b.l().calibrate(); }, py::call_guard<NativeCall, py::gil_scoped_release>(),
           "Sizes one launch to about 250 us and measures the load alone (blocking).")
      .def_property_readonly("kind", [](PyBackgroundLoad& b) { return b.l().kind(); })
      .def_property_readonly("wgs", [](PyBackgroundLoad& b) { return b.l().wgs(); })
      .def_property_readonly("unit", [](PyBackgroundLoad& b) { return std::string(b.l().unit()); })
      .def_property_readonly("launch_s", [](PyBackgroundLoad& b) { return b.l().launch_s(); })
      .def_property_readonly("alone_rate", [](PyBackgroundLoad& b) { return b.l().alone_rate(); })
      .def("start", [](PyBackgroundLoad& b, double expected_s) { b.l().start(expected_s); }, py::arg("expected_s"),
           py::call_guard<NativeCall, py::gil_scoped_release>())
      .def("window_begin", [](PyBackgroundLoad& b) { b.l().window_begin(); })
      .def("window_end", [](PyBackgroundLoad& b) { b.l().window_end(); })
      .def("stop", [](PyBackgroundLoad& b) {
             LoadStats s;
             {
               NativeCall in_engine;
               py::gil_scoped_release nogil;
               s = b.l().stop();
             }
             return load_stats_py(s);
           }, "Cancels the queued launches, waits for the stream and returns the counters as a dict.");
  m.def("wall_clock_hz", []() {
        int dv = 0;
        if (hipGetDevice(&dv) != hipSuccess) P2P_FATAL("no HIP device");
        return dev::wall_clock_hz(dv);
      }, "Ticks per second of the current device's wall clock, the unit of timeout_ticks and of the stamps.");
  py::class_<SignalPage>(m, "signal_page")
      .def(py::init<size_t>(), py::arg("bytes"))
      .def_property_readonly("ptr", &SignalPage::ptr)
      .def_property_readonly("bytes", &SignalPage::bytes)
      .def_property_readonly("uncached", &SignalPage::uncached);
  py::class_<HostWords>(m, "HostWords")
      .def(py::init<size_t>(), py::arg("n"))
      .def("__len__", &HostWords::size)
      .def("ptr", &HostWords::ptr, py::arg("i"))
      .def("load", &HostWords::load, py::arg("i"))
      .def("store", &HostWords::store, py::arg("i"), py::arg("v"));
  m.def("fill_geometry", [](size_t bytes) {
    auto g = dev::fill_geometry(bytes);
    return py::make_tuple(g.grid, g.block, g.lds_bytes);
  });
  m.def("verify_geometry", [](size_t bytes, int impl, unsigned max_grid, int lds_stages) {
    auto g = dev::verify_geometry(bytes, verify_impl_arg(impl), max_grid, lds_stages_arg(lds_stages));
    return py::make_tuple(g.grid, g.block, g.lds_bytes);
  }, py::arg("bytes"), py::arg("impl"), py::arg("max_grid") = 0, py::arg("lds_stages") = 0);
  m.def("rccl_available", &rccl_transport_available);
  m.def("runtime_json", &runtime_json, "HIP runtime / RCCL library versions and paths, visible devices and links.");
  m.def("env_knobs_json", &env_knobs_json, "Every NCCL_/RCCL_/HSA_/HIP_/GPU_... environment knob that is set.");
  m.def("request_abort", []() { request_abort(); },
        "Ask every transport wait of this process to abort its communicators on its own thread and fail.");
  m.def("abort_requested", []() { return abort_requested(); });
  m.def("abort_done", []() { return abort_done(); },
        "True once a transport wait has aborted its communicators after request_abort().");
  m.def("abort_if_idle", &abort_if_idle, py::call_guard<py::gil_scoped_release>(),
        "Watchdog: when no thread is inside the engine, abort every communicator from this thread, take no more "
        "engine calls and note the abort done; False (nothing done) while a call is in flight.  Releases the GIL "
        "(and holds no engine lock) while the aborts run, so a blocking abort stalls no other thread.");
  m.def("_push_blocking_abort_hook", [](double seconds) {
        push_abort_hook([seconds](int) { std::this_thread::sleep_for(std::chrono::duration<double>(seconds)); });
      }, py::arg("seconds"),
      "Test hook: an abort hook that blocks for `seconds` (an ncclCommAbort that does not return).");
  m.def("run_abort_hooks", []() { run_abort_hooks(1); }, py::call_guard<py::gil_scoped_release>(),
        "Aborts every live RCCL communicator / bootstrap (their kernels exit); for a watchdog about to end the "
        "process.");

  // ---- host reference (bit-compatible with the kernels) ----
  m.def("host_fill", [](size_t bytes, uint64_t seed) {
    std::string out(bytes, '\0');
    host_fill(&out[0], bytes, seed);
    return py::bytes(out);
  });
  m.def("host_verify", [](py::bytes data, uint64_t seed) {
    std::string s = data;
    VerifyResult r = host_verify(s.data(), s.size(), seed);
    return py::make_tuple(r.mismatches, r.checksum, r.first_bad);
  });
  // ---- mismatch diagnosis ----
  m.attr("MAX_DIAG_CANDIDATES") = kMaxDiagCandidates;
  m.def("diagnose", [](uintptr_t ptr, size_t bytes, uint64_t seed, const std::vector<py::tuple>& candidates,
                       size_t granule, uintptr_t stream, unsigned max_grid) {
        return device_diagnose(ptr, bytes, seed, candidates, granule, stream, max_grid, true);
      }, py::arg("ptr"), py::arg("bytes"), py::arg("seed"),
        py::arg("candidates") = std::vector<py::tuple>{}, py::arg("granule") = 0, py::arg("stream") = 0,
        py::arg("max_grid") = 0,
        "The gfx950 diagnosis kernel on a device buffer (blocking): the damaged granules, each (index, first_bad, "
        "last_bad, zero, other, flipped_bits, cand0..cand5) with first_bad / last_bad the byte offsets of its first "
        "and last damaged word.  candidates: up to 6 (seed, shift) with shift a multiple of 16 bytes; granule 0: "
        "by size; max_grid > 0 caps the workgroup count.");
  m.def("diagnose_launch", [](uintptr_t ptr, size_t bytes, uint64_t seed, const std::vector<py::tuple>& candidates,
                              size_t granule, uintptr_t stream, unsigned max_grid) {
        // Stream-ordered launch only (the records' memset + the kernel), no
        // readback: for timing the kernel with events.
        device_diagnose(ptr, bytes, seed, candidates, granule, stream, max_grid, false);
      }, py::arg("ptr"), py::arg("bytes"), py::arg("seed"), py::arg("candidates") = std::vector<py::tuple>{},
      py::arg("granule") = 0, py::arg("stream") = 0, py::arg("max_grid") = 0);
  m.def("host_diagnose", [](py::bytes data, uint64_t seed, const std::vector<py::tuple>& candidates, size_t granule) {
        const std::string s = data;
        const std::vector<DiagCandidate> c = candidates_arg(candidates);
        granule = granule_arg(granule, s.size());
        const auto recs = host_diagnose(s.data(), s.size(), seed, c.data(), static_cast<int>(c.size()), granule);
        return records_py(recs.data(), recs.size());
      }, py::arg("data"), py::arg("seed"), py::arg("candidates") = std::vector<py::tuple>{}, py::arg("granule") = 0,
      "CPU implementation of diagnose, the same records bit for bit.");
  m.def("merge_extents", &merge_extents_py, py::arg("records"), py::arg("bytes"), py::arg("granule") = 0,
        "Damaged granules -> extents (begin, end, zero, other, flipped_bits, cand0..cand5): maximal runs of "
        "consecutive damaged granules with the same set of non-zero classes.");
  m.def("describe_extent", &describe_extent_py, py::arg("extent"), py::arg("bytes"),
        py::arg("candidates") = std::vector<py::tuple>{}, "One line saying what an extent's words hold instead.");
  m.def("diagnose_granule", &diagnose_granule, py::arg("bytes"),
        "The default granule: the smallest power of two >= 4 KiB with at most 65536 records for the buffer.");
  m.def("prng_word", &prng_word);
  m.def("payload_seed", &payload_seed);

  // ---- pure host helpers ----
  m.def("schedule", &schedule_py, py::arg("mode"), py::arg("dir"), py::arg("n"));
  m.def("round_robin_rounds", &round_robin_rounds);
  m.def("plan_routes",
        [](int n, const std::vector<std::pair<int, int>>& flows, size_t bytes, size_t min_bytes, double relay_weight,
           int max_relays) {
          RouteOptions o;
          o.min_bytes = min_bytes;
          o.relay_weight = relay_weight;
          o.max_relays = max_relays;
          py::list out;
          for (const auto& stripes : plan_routes(n, flows, bytes, o)) {
            py::list l;
            for (const auto& st : stripes) l.append(py::make_tuple(st.via, st.offset, st.bytes));
            out.append(l);
          }
          return out;
        },
        py::arg("n"), py::arg("flows"), py::arg("bytes"), py::arg("min_bytes") = size_t{1} << 20,
        py::arg("relay_weight") = 1.0, py::arg("max_relays") = -1,
        "The relay engine's split of each flow of a group: [(via, offset, bytes), ...] per flow, direct stripe "
        "first (via = -1).");
  m.def("parse_size", &parse_size);
  m.def("parse_size_list", &parse_size_list);
  m.def("format_size", &format_size);
  m.def("host_hash", &host_hash);
  m.def("compute_placement", [](const std::vector<uint64_t>& h, int rank) {
    Placement p = compute_placement(h, rank);
    py::dict d;
    d["ok"] = p.ok;
    d["error"] = p.error;
    d["num_hosts"] = p.num_hosts;
    d["ranks_per_host"] = p.ranks_per_host;
    d["local_rank"] = p.local_rank;
    return d;
  });
  m.def("usage", &usage_text);
  m.def("parse_verify_impl", [](const std::string& name) {
        std::string note;
        const int v = parse_verify_impl(name, &note);
        if (v < 0) throw py::value_error("verify impl '" + name + "': " + note);
        return v;
      }, py::arg("name"), "Verify kernel name -> impl number (auto 0, lds8 1, stride 2), as p2p_matrix --verify-impl.");
  // The full p2p_matrix application in-process (TCP/env or local bootstrap),
  // e.g. `torchrun --nproc-per-node 8 -m test_nccl_p2p_amd --mode all`.
  m.def("run_cli", [](std::vector<std::string> args) {
    std::vector<char*> argv;
    for (auto& a : args) argv.push_back(&a[0]);
    AppConfig cfg;
    int code = 0;
    if (!parse_cli(static_cast<int>(argv.size()), argv.data(), &cfg, &code)) return code;
    // In the engine for the whole app: a watchdog's abort_if_idle
    // must not abort its communicators from another thread meanwhile.  Taken
    // with the GIL held, like every binding's NativeCall.
    NativeCall in_engine;
    py::gil_scoped_release nogil;
    std::string kind = cfg.bootstrap == "mpi" ? "env" : cfg.bootstrap;
    auto boot = make_bootstrap(kind, nullptr, nullptr);
    return run_app(cfg, *boot, stdout);
  }, py::arg("args"));
}
