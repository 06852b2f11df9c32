// Device-initiated stream: the pipelined counterpart of the ping-pong
// (pingpong.hip), over the same hipIpc-mapped, uncached signal pages.
//
// The ping-pong keeps exactly one message in flight and measures latency.
// What a kernel-driven communication pattern gets out of a link (a fused
// all-to-all dispatch, a device-side pipeline hand-off, a low-latency
// collective protocol) is the pipelined case: how many messages of B bytes a
// second one wave pushes into a peer with D of them in flight, and how many
// such channels run side by side.  A channel is a credit-flow ring:
//
//   sender, message i:   i >= depth: spin on its own `head` until the slot's
//                        credit came back -> write slot i % depth of the
//                        peer's ring (16 B stores) -> release -> tail = seq
//   receiver, message i: spin on its own `tail` until >= seq -> one acquire
//                        -> stamp -> load and compare the slot -> head = seq
//
// As in the ping-pong every store crosses the link and every spin is on local
// memory; flags are 64-bit monotonic sequence numbers that are never reset;
// every spin is bounded by an s_memrealtime deadline that ends the kernel
// with status bit 0 instead of hanging the GPU.  One role is one workgroup of
// one wave, so no workgroup barrier is involved.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "kernels.hpp"

namespace p2p {
namespace dev {
namespace {

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u64 now_ticks() { return static_cast<u64>(wall_clock64()); }

// Wave-uniform: every lane loads the same flag and reads the same scalar
// clock.  Relaxed: polling with acquire loads costs an invalidate per poll;
// the receiver fences once after the poll, the sender reads no data at all.
__device__ __forceinline__ bool stream_wait(const u64* flag, u64 want, u64 deadline) {
  while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < want)
    if (now_ticks() > deadline) return false;
  return true;
}

__device__ __forceinline__ void stream_send(const StreamRole& r, int lane, u64 deadline) {
  const u64 nvec = r.bytes / 16;
  const u64 depth = static_cast<u64>(r.depth);
  if (lane == 0) r.stamps[0] = now_ticks();
  for (int i = 0; i < r.iters; ++i) {
    const u64 seq = r.base + static_cast<u64>(i) + 1;
    // The slot is free once the message that last used it was consumed.
    if (static_cast<u64>(i) >= depth && !stream_wait(r.in_flag, seq - depth, deadline)) {
      if (lane == 0) atomicOr(r.status, 1u);
      return;
    }
    unsigned char* slot = r.ring + (static_cast<u64>(i) % depth) * r.bytes;
    for (u64 j = static_cast<u64>(lane); j < nvec; j += 64) {
      const u64x2 v = {seq, j};
      *reinterpret_cast<u64x2*>(slot + j * 16) = v;
    }
    // All of this wave's payload stores are complete (vmcnt is per wave) and
    // written back before the flag becomes visible to the peer.  The explicit
    // wait stays: behind the waited credit load above the compiler may take
    // the scoreboard for empty and drop the fence's own.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
      __hip_atomic_store(r.out_flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      r.stamps[i + 1] = now_ticks();
    }
  }
  // Leave only when the ring is consumed: the next launch may reuse it.
  if (!stream_wait(r.in_flag, r.base + static_cast<u64>(r.iters), deadline)) {
    if (lane == 0) atomicOr(r.status, 1u);
    return;
  }
  if (lane == 0) r.stamps[r.iters + 1] = now_ticks();
}

__device__ __forceinline__ void stream_recv(const StreamRole& r, int lane, u64 deadline) {
  const u64 nvec = r.bytes / 16;
  const u64 depth = static_cast<u64>(r.depth);
  for (int i = 0; i < r.iters; ++i) {
    const u64 seq = r.base + static_cast<u64>(i) + 1;
    if (!stream_wait(r.in_flag, seq, deadline)) {
      if (lane == 0) atomicOr(r.status, 1u);
      return;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    if (lane == 0) r.stamps[i] = now_ticks();
    const unsigned char* slot = r.ring + (static_cast<u64>(i) % depth) * r.bytes;
    unsigned int bad = 0;  // wave-uniform
    if (r.check_all) {
      // Lane 0 holds the lowest vector of every pass, so it is in all of them.
      for (u64 j = static_cast<u64>(lane); j < nvec; j += 64) {
        const u64x2 v = *reinterpret_cast<const u64x2*>(slot + j * 16);
        bad += static_cast<unsigned int>(__popcll(__ballot(v.x != seq || v.y != j)));
      }
    } else {
      bool wrong = false;
      if (lane == 0 || (lane == 1 && nvec > 1)) {
        const u64 j = lane == 0 ? 0 : nvec - 1;
        const u64x2 v = *reinterpret_cast<const u64x2*>(slot + j * 16);
        wrong = v.x != seq || v.y != j;
      }
      bad = static_cast<unsigned int>(__popcll(__ballot(wrong)));
    }
    if (bad && lane == 0) atomicAdd(r.status + 1, bad);
    // The compares above consumed every load of the slot, so they have
    // completed; the fence keeps the credit behind them in program order.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    if (lane == 0) __hip_atomic_store(r.out_flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ __launch_bounds__(64) void stream_kernel(StreamArgs a) {
  if (static_cast<int>(blockIdx.x) >= a.nroles) return;
  const StreamRole& r = a.role[blockIdx.x];
  const int lane = static_cast<int>(threadIdx.x);
  const u64 deadline = now_ticks() + r.timeout_ticks;
  if (r.sender)
    stream_send(r, lane, deadline);
  else
    stream_recv(r, lane, deadline);
}

}  // namespace

void launch_stream(const StreamRole* roles, int nroles, hipStream_t stream) {
  P2P_CHECK(roles && nroles >= 1 && nroles <= kMaxStreamRoles, strfmt("stream: 1..%d roles per launch", kMaxStreamRoles));
  StreamArgs a{};
  for (int k = 0; k < nroles; ++k) {
    const StreamRole& r = roles[k];
    P2P_CHECK(r.bytes >= 16 && r.bytes % 16 == 0 && r.bytes <= kMaxStreamBytes,
              strfmt("stream: message bytes must be a multiple of 16, 16..%llu", kMaxStreamBytes));
    P2P_CHECK(r.depth >= 1 && r.depth <= kMaxStreamDepth, strfmt("stream: depth 1..%d", kMaxStreamDepth));
    P2P_CHECK(static_cast<unsigned long long>(r.depth) * r.bytes <= kMaxStreamRingBytes,
              strfmt("stream: depth x bytes is at most %llu", kMaxStreamRingBytes));
    P2P_CHECK(r.iters >= 1 && r.iters <= kMaxStreamIters, strfmt("stream: 1..%d messages", kMaxStreamIters));
    P2P_CHECK(r.out_flag && r.in_flag && r.ring && r.stamps && r.status, "stream: a role has a null pointer");
    P2P_CHECK(reinterpret_cast<uintptr_t>(r.ring) % 16 == 0 && reinterpret_cast<uintptr_t>(r.out_flag) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(r.in_flag) % 8 == 0 && reinterpret_cast<uintptr_t>(r.stamps) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(r.status) % 4 == 0,
              "stream: a role has a misaligned pointer");
    a.role[k] = r;
  }
  a.nroles = nroles;
  hipLaunchKernelGGL(stream_kernel, dim3(static_cast<unsigned>(nroles)), dim3(64), 0, stream, a);
}

}  // namespace dev
}  // namespace p2p
