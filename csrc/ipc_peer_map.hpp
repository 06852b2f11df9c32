// The IPC transport's one exchange: export mine, allgather, open every
// peer's, keep my own pointer in my slot.  GPU translation units only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "bootstrap.hpp"
#include "common.hpp"
#include "hip_check.hpp"
#include "ipc_blocks.hpp"

namespace p2p {

struct PeerMap {
  std::vector<void*> ptr;       // every rank's block as this process sees it (null: not mapped)
  std::vector<uint32_t> value;  // what every rank handed in
};

constexpr uint64_t kPeerMapUnchecked = ~0ull;

// Collective, one allgather.  `same` must be equal on every rank (`differ`
// is the error's text) unless it is kPeerMapUnchecked; a rank on another host
// is refused ("<who> is intra-node only: ...").  *out is filled as the
// mappings are opened, so after a failure close_peers() drops what was made.
inline void map_peers(Bootstrap& boot, const IpcHandle& mine, void* own, uint64_t same, const char* differ,
                      uint32_t value, const char* who, PeerMap* out) {
  struct Export {
    IpcHandle handle;
    uint64_t same;
    uint64_t host_hash;
    uint32_t value;
  };
  static_assert(sizeof(hipIpcMemHandle_t) == sizeof(IpcHandle), "IpcHandle carries a hipIpcMemHandle_t");
  Export me{};  // zeroed: the padding travels too
  me.handle = mine;
  me.same = same;
  me.host_hash = host_hash(real_hostname());
  me.value = value;
  const auto all = boot.allgather_value(me);
  const int rank = boot.rank(), n = boot.size();
  out->ptr.assign(static_cast<size_t>(n), nullptr);
  out->value.assign(static_cast<size_t>(n), 0);
  for (int r = 0; r < n; ++r) {
    out->value[static_cast<size_t>(r)] = all[static_cast<size_t>(r)].value;
    if (r == rank) {
      out->ptr[static_cast<size_t>(r)] = own;
      continue;
    }
    P2P_CHECK(all[static_cast<size_t>(r)].host_hash == me.host_hash,
              strfmt("%s is intra-node only: rank %d is on another host", who, r));
    P2P_CHECK(same == kPeerMapUnchecked || all[static_cast<size_t>(r)].same == same, differ);
    hipIpcMemHandle_t handle;
    std::memcpy(&handle, &all[static_cast<size_t>(r)].handle, sizeof(handle));
    void* mapped = nullptr;
    HIPCHECK(hipIpcOpenMemHandle(&mapped, handle, hipIpcMemLazyEnablePeerAccess));
    out->ptr[static_cast<size_t>(r)] = mapped;
  }
}

// Closes every mapping but this rank's own slot; safe on a half-built map.
inline void close_peers(PeerMap* m, int rank) {
  for (size_t r = 0; r < m->ptr.size(); ++r)
    if (m->ptr[r] && static_cast<int>(r) != rank) (void)hipIpcCloseMemHandle(m->ptr[r]);
  m->ptr.clear();
  m->value.clear();
}

}  // namespace p2p
