// How one launch's workgroups are shared by its jobs (the batched verify's
// buffers, the multi-source copy's ops).  Plain C++: the host unit tests
// cover it.
#pragma once

#include <algorithm>
#include <cstdint>

namespace p2p {

// Job i of `cnt` holds nvec[i] 16-byte vectors and needs one workgroup per
// `block_vecs` of them, at least one.  While the needs fit `cap` every job
// gets its need; beyond it, its share of `cap` in proportion (rounded down,
// at least one workgroup: the kernels stride over the rest).  Job i's
// workgroups are [block_begin[i], block_begin[i + 1]); returns their total,
// block_begin[cnt].
inline uint32_t split_blocks(const uint64_t* nvec, int cnt, uint64_t block_vecs, uint64_t cap, uint32_t* block_begin) {
  auto need = [&](int i) { return std::max<uint64_t>(1, (nvec[i] + block_vecs - 1) / block_vecs); };
  uint64_t total = 0;
  for (int i = 0; i < cnt; ++i) total += need(i);
  uint32_t acc = 0;
  for (int i = 0; i < cnt; ++i) {
    block_begin[i] = acc;
    const uint64_t share = total <= cap ? need(i) : std::max<uint64_t>(1, need(i) * cap / total);
    acc += static_cast<uint32_t>(std::min(share, need(i)));
  }
  block_begin[cnt] = acc;
  return acc;
}

}  // namespace p2p
