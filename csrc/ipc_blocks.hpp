// IpcBlocks: the IPC transport's exporting allocator and its reuse pool, as
// pure policy (plain host code, no HIP; the host unit tests drive it with
// counting fakes).  The transport supplies "allocate", "free" and "export"; a
// handle is an opaque 64-byte blob (hipIpcMemHandle_t passes through it).
//
// Every buffer is an allocation of its own, exported once, when it is made,
// and keeps its handle.  Released buffers are kept for reuse, by exact size,
// up to a cap: a buffer set is created per run, and reusing the same exported
// blocks avoids allocation churn between runs.
#pragma once

#include <algorithm>
#include <cstddef>
#include <functional>
#include <map>
#include <utility>
#include <vector>

#include "common.hpp"

namespace p2p {

struct IpcHandle {
  unsigned char bytes[64];
};

class IpcBlocks {
 public:
  using AllocFn = std::function<const char*(void** p, size_t size)>;          // null, or the error's text
  using ExportFn = std::function<const char*(void* p, IpcHandle* handle)>;    // null, or the refusal's text
  using RefusedFn = std::function<void(size_t blocks, size_t size)>;  // exports refused before a good block

  // pool_cap: bytes the pool may hold (0 keeps nothing).  size_fix: see size_for().
  IpcBlocks(size_t pool_cap, bool size_fix, AllocFn alloc, std::function<void(void*)> free, ExportFn exp, RefusedFn refused)
      : pool_cap_(pool_cap), size_fix_(size_fix), alloc_(std::move(alloc)), free_(std::move(free)),
        export_(std::move(exp)), refused_(std::move(refused)) {}

  // At least 2 MiB, rounded to 2 MiB.  With size_fix, a size whose remainder
  // mod 4 GiB is 2 GiB or more goes up to the next multiple of 4 GiB (blocks
  // HIP 7.0's hipIpcOpenMemHandle never returns for, see IpcTransport).
  static size_t size_for(size_t bytes, bool size_fix) {
    constexpr size_t kGrain = size_t{2} << 20, k4G = size_t{4} << 30;
    const size_t size = (std::max<size_t>(bytes, 1) + kGrain - 1) / kGrain * kGrain;
    return size_fix && size % k4G >= k4G / 2 ? (size / k4G + 1) * k4G : size;
  }

  void* alloc(size_t bytes) {
    const size_t size = size_for(bytes, size_fix_);
    for (auto it = pool_.begin(); it != pool_.end(); ++it)
      if (it->second.size == size) {
        void* p = it->first;
        pool_bytes_ -= size;
        blocks_[p] = it->second;
        pool_.erase(it);
        return p;
      }
    Block b;
    b.size = size;
    void* p = exportable(size, &b.handle, [&](void** q, size_t) {
      const char* e = alloc_(q, size);
      if (e && !pool_.empty()) {  // give the pool back and retry once
        drain();
        e = alloc_(q, size);
      }
      return e;
    });
    blocks_[p] = b;
    return p;
  }

  void release(void* p) {
    if (!p) return;
    auto it = blocks_.find(p);
    P2P_CHECK(it != blocks_.end(), "release of a buffer this transport did not allocate");
    const Block b = it->second;
    blocks_.erase(it);
    if (pool_bytes_ + b.size <= pool_cap_) {
      pool_.emplace_back(p, b);
      pool_bytes_ += b.size;
    } else {
      free_(p);
    }
  }

  const IpcHandle& handle_of(void* p) const {
    auto it = blocks_.find(p);
    P2P_CHECK(it != blocks_.end(), "ipc transport exports only buffers it allocated");
    return it->second.handle;
  }
  size_t pooled_bytes() const { return pool_bytes_; }  // handed back on demand
  void drain() {
    for (auto& b : pool_) free_(b.first);
    pool_.clear();
    pool_bytes_ = 0;
  }

  // A new allocation from alloc_fn whose export works, with its handle (not
  // entered in the live map: the signal pages come from here too).  The
  // runtime now and then refuses to export a fresh block ("invalid argument",
  // seen with 8 processes allocating on one GPU); such a block is held (so the
  // allocator cannot hand it straight back) until a good one is found, then
  // freed, and the retry is reported.  The eighth refusal in a row is fatal.
  void* exportable(size_t size, IpcHandle* handle, const AllocFn& alloc_fn) {
    std::vector<void*> refused;
    const auto free_refused = [&] {
      for (void* r : refused) free_(r);
    };
    void* p = nullptr;
    for (int attempt = 0;; ++attempt) {
      const char* e = alloc_fn(&p, size);
      if (e) {
        free_refused();
        P2P_FATAL(strfmt("device allocation of %zu bytes failed: %s", size, e));
      }
      e = export_(p, handle);
      if (!e) break;
      refused.push_back(p);
      if (attempt == 7) {
        free_refused();
        P2P_FATAL(strfmt("hipIpcGetMemHandle refused 8 fresh %zu-byte blocks: %s", size, e));
      }
    }
    if (!refused.empty()) refused_(refused.size(), size);
    free_refused();
    return p;
  }

 private:
  struct Block {
    size_t size = 0;
    IpcHandle handle{};
  };
  const size_t pool_cap_;
  const bool size_fix_;
  const AllocFn alloc_;
  const std::function<void(void*)> free_;
  const ExportFn export_;
  const RefusedFn refused_;
  std::vector<std::pair<void*, Block>> pool_;  // released, kept for reuse
  size_t pool_bytes_ = 0;
  std::map<void*, Block> blocks_;  // live allocations
};

}  // namespace p2p
