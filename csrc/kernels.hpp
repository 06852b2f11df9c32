// Host-side launch API for the gfx950 buffer kernels (kernels.hip).
//
// The reference has no device code at all: its buffers are zeroed with
// cudaMemset (p2p_matrix.cc:129-130) and never read back.
// These kernels replace that with verifiable random payloads:
//   fill    — counter-based PRNG, one 16-byte global_store_dwordx4 per lane
//   verify  — regenerates the stream and compares; two stagings, the A/B
//             SURVEY.md §7.5 item 6 asks for:
//               * LDS (Lds8, the default): non-temporal global_load_lds_dwordx4
//                           (LDS-DMA, 1 KiB per wave instruction) into a
//                           per-wave LDS slot of 8 KiB, then ds_read_b128 —
//                           the LDS-staged form the north star asks for;
//                           6.44 / 6.64 TB/s at 1 / 4 GiB, within 1-2% of
//                           register staging
//               * stride:   register staging, 4 x global_load_dwordx4 in flight
//                           per lane, grid capped at 16 workgroups per CU so the
//                           reduction epilogue is amortised over 64 KiB+
//             (round 5 removed the variants that lost: profiles/r1_tuned/,
//             r4_verify_span/)
//   reduce  — fused epilogue of verify: wave64 __shfl_xor tree -> LDS across
//             the 4 waves -> one atomic per block into one of kVerifyShards
//             64-byte counters (no single hot address), then a one-wave
//             finalize kernel folds the shards
//   copy    — multi-source copy for the IPC transport (remote loads over xGMI),
//             and its checked form: the same copy comparing every word it
//             loads with the PRNG stream due, for the inline check
//
// Measured on MI355X (profiles/, scripts/fill_probe.hip): streaming at one
// 16 B access per lane with one block per 4 KiB (a "full grid", up to 2^20
// blocks, then grid-stride) reaches 6.9-7.0 TB/s for stores and 6.7-6.8 TB/s
// for loads, against 5.1-5.6 / 6.3 TB/s for grid-stride loops over a grid
// capped at 4-32 blocks per CU.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "prng.hpp"

namespace p2p {
namespace dev {

// One 64-byte shard of the device-side accumulator; `first_bad` starts at ~0
// (launch_verify_reset).  Allocate verify_accum_bytes() for the whole array;
// after launch_verify the totals are in shard 0.
struct alignas(64) VerifyAccum {
  unsigned long long mismatches;
  unsigned long long checksum;
  unsigned long long first_bad;
};
constexpr int kVerifyShards = 64;
constexpr size_t verify_accum_bytes() { return sizeof(VerifyAccum) * kVerifyShards; }

// Verify staging (app.hpp parse_verify_impl maps the CLI / Python names).
enum class VerifyImpl : int { Auto = 0, Lds8 = 1, Stride = 2 };
// One fill kernel, the full grid; the enum stays so callers name it.
enum class FillImpl : int { Auto = 0, Grid = 1 };

// Geometry chosen for a launch (exposed for tests / profiling scripts).
struct LaunchGeom {
  unsigned grid = 0;
  unsigned block = 256;
  size_t lds_bytes = 0;
  int lds_stages = 0;  // LDS-staged verify: KiB each wave stages per pass (4 or 8); 0 for the stride kernel
};

LaunchGeom fill_geometry(size_t bytes, FillImpl impl = FillImpl::Auto);
// max_grid > 0 caps the workgroup count (the kernels grid-stride beyond it);
// 0 = the tuned default of the variant.  lds_stages picks the LDS-staged
// kernel's template: 0 = by size (4 KiB per wave below 2 GiB, 8 KiB from
// there), 4 or 8 force that one at any size (tests reach either kernel's
// loop on small buffers); anything else fails a P2P_CHECK.  The stride
// kernel ignores the value.  The returned geometry is what launch_verify
// launches: grid, LDS bytes and template.
LaunchGeom verify_geometry(size_t bytes, VerifyImpl impl, unsigned max_grid = 0, int lds_stages = 0);

void launch_fill(void* p, size_t bytes, uint64_t seed, hipStream_t stream, FillImpl impl = FillImpl::Auto);
void launch_verify_reset(VerifyAccum* acc, hipStream_t stream);
// check_prng=false only sums the words (checksum of an arbitrary buffer).
// Leaves the totals in acc[0] (stream-ordered).  max_grid and lds_stages as
// in verify_geometry (0, 0: the production launch).
void launch_verify(const void* p, size_t bytes, uint64_t seed, VerifyAccum* acc, VerifyImpl impl, bool check_prng,
                   hipStream_t stream, unsigned max_grid = 0, int lds_stages = 0);

// ---- batched verify (the post-timing check of many receive slots) ----
// Job i's totals land in out[i] (device memory, njobs entries; nothing needs
// resetting).  Batches of kMaxVerifyJobs, three launches each (reset, the
// LDS-DMA verify over all the batch's buffers, finalize); `scratch` holds
// multi_verify_scratch_bytes() and is reused by every batch (stream order).
// VerifyJob is prng.hpp's; device_checks.hpp BatchVerifier owns the arrays.
constexpr int kMaxVerifyJobs = 32;
constexpr size_t multi_verify_scratch_bytes() { return verify_accum_bytes() * kMaxVerifyJobs; }
void launch_multi_verify(const VerifyJob* jobs, int njobs, VerifyAccum* scratch, VerifyAccum* out, hipStream_t stream);

// Device attributes cached per device (CU count drives grid sizing).
int cu_count();

// ---- multi-source copy (IPC transport data plane) ----
// One launch moves every receive of a group: op i copies ops[i].bytes from
// src (typically a peer GPU's buffer mapped through hipIpcOpenMemHandle, so
// the loads travel over xGMI) to dst.  Full grid: one 16 B load + store per
// lane, one 4 KiB block per workgroup, workgroups split across ops by size.
// coherent = the op crosses GPUs (a hipIpc-mapped peer buffer on either side):
// its loads and stores carry system-scope cache bits (sc0 sc1), so a reader
// never sees a line its L2 kept from an earlier run of the peer's buffer and
// the payload is written through to the owner's HBM before the kernel ends.
// Local ops (the self path) keep plain accesses.
struct CopyOp {
  const void* src;
  void* dst;
  size_t bytes;
  bool coherent = false;
};
constexpr int kMaxCopyOps = 32;  // ops per launch (one bit each in CopyArgs::coherent)
void launch_multi_copy(const CopyOp* ops, int nops, hipStream_t stream, int max_blocks = 0);

// ---- checked multi-source copy (inline verification of a pull) ----
// The same copy (geometry, accesses, host-side splitting) whose every lane
// also regenerates the word it expects and compares it with the one it
// loaded, before storing that loaded value -- matched or not.  Op i's data
// is bytes [stream_offset, stream_offset + bytes) of PRNG stream `seed`;
// stream_offset must be a multiple of 4096 (a P2P_CHECK), so a workgroup's
// 1024 words never straddle a 2^32-word key span.  Words and the tail follow
// the verify kernels' rules (32-bit words, the final partial word masked).
// A wave with no wrong word does nothing more (no LDS, no barrier, no
// atomic); a wave with one reduces over its lanes and commits with one
// atomicAdd and one atomicMin into the op's record, first_bad in stream
// bytes (stream_offset + position).  Several ops may name one record: it
// accumulates over ops and launches until launch_copy_check_reset.
// What it proves: the value the receiver LOADED is the one due.  Whether the
// store landed is the memory check's business (launch_verify).
struct CopyCheck {
  unsigned long long mismatches;  // wrong 32-bit words (a partial tail word counts once)
  unsigned long long first_bad;   // lowest wrong stream byte offset, ~0 if none
};
struct CheckedCopyOp : CopyOp {
  uint64_t seed = 0;
  uint64_t stream_offset = 0;
  CopyCheck* record = nullptr;  // device memory (hipMalloc)
};
// Stream-ordered: records [0, n) become {0, ~0}.
void launch_copy_check_reset(CopyCheck* records, int n, hipStream_t stream);
void launch_multi_copy_checked(const CheckedCopyOp* ops, int nops, hipStream_t stream, int max_blocks = 0);

// ---- device-initiated ping-pong (pingpong.hip) ----
// One wave per role.  The leader writes message i (payload words = base+i+1,
// then the flag) into the peer's inbox and spins on its own inbox for the
// reply; the follower mirrors it.  stamps[0..iters] (leader only) are
// s_memrealtime ticks; status[0] bit 0 = a spin hit the deadline, status[1] =
// payloads that arrived without their sequence number.
struct PingRole {
  unsigned long long* out_flag;        // peer's inbox flag
  unsigned char* out_payload;          // peer's inbox payload
  const unsigned long long* in_flag;   // own inbox flag (written by the peer)
  const unsigned char* in_payload;     // own inbox payload
  unsigned long long bytes;            // payload bytes, multiple of 16, >= 16
  unsigned long long base;             // sequence base of what this wave writes (iteration i: base + i + 1)
  unsigned long long in_base;          // sequence base of what it waits for (== base for a ping-pong pair;
                                       // a ring token chain reads its predecessor's count, writes its own)
  int iters;
  int leader;
  unsigned long long* stamps;          // leader: iters + 1 entries
  unsigned int* status;                // 2 words, zeroed by the caller
  unsigned long long timeout_ticks;    // per kernel, in s_memrealtime ticks
};
// b == nullptr: one wave (cross-process partner).  Otherwise both roles run
// as two waves of one workgroup (self ping-pong on one GPU).
void launch_pingpong(const PingRole& a, const PingRole* b, hipStream_t stream);

// ---- stream-ordered flag signalling (pingpong.hip; IPC push engine) ----
// One wave: optionally a system-scope release fence (so the writes of earlier
// kernels in the stream, e.g. a copy into a peer's memory, reach their
// memory first), then every post stores its value to its flag (system scope),
// then the wave spins until every wait flag is >= its value (system-scope
// acquire), each spin bounded by timeout_ticks; a deadline sets bit 0 of
// *status (host-visible memory) and ends the kernel.
constexpr int kMaxSignals = 16;
struct SignalArgs {
  unsigned long long* post_flag[kMaxSignals];
  unsigned long long post_value[kMaxSignals];
  const unsigned long long* wait_flag[kMaxSignals];
  unsigned long long wait_value[kMaxSignals];
  int nposts;
  int nwaits;
  int release_first;
  unsigned int* status;
  unsigned long long timeout_ticks;
};
void launch_signal(const SignalArgs& args, hipStream_t stream);

// ---- device-initiated stream (stream.hip) ----
// The pipelined counterpart of the ping-pong: a channel is a one-directional
// single-producer / single-consumer ring of `depth` slots of `bytes` in the
// receiver's memory, with a `tail` flag beside it (messages published, written
// by the sender) and a `head` flag in the sender's memory (messages consumed,
// written by the receiver: the credit).  One role is one workgroup of one
// wave; a launch carries up to kMaxStreamRoles of them by value.  Vector j of
// the message with sequence s is the two 64-bit words {s, j}.  The sender
// stamps stamps[0] before the first message, stamps[i + 1] after publishing
// message i and stamps[iters + 1] after the final credit (it leaves only when
// the ring is consumed); the receiver stamps stamps[i] when message i has
// arrived.  status[0] bit 0 = a spin hit the deadline, status[1] = wrong 16 B
// vectors among those the receiver checked (check_all: every one; otherwise
// the first and, where there is more than one, the last of each message).
struct StreamRole {
  unsigned long long* out_flag;       // sender: peer's tail;  receiver: peer's head (credit)
  const unsigned long long* in_flag;  // sender: own head;     receiver: own tail
  unsigned char* ring;                // sender: peer's ring (written); receiver: own ring (read)
  unsigned long long bytes;           // per message, multiple of 16, 16 .. 1 MiB
  unsigned long long base;            // sequence base: message i carries seq = base + i + 1
  int depth;                          // 1 .. 64, depth * bytes <= 4 MiB
  int iters;                          // 1 .. 100000
  int sender;                         // 1 = sender, 0 = receiver
  int check_all;                      // receiver: 1 = every 16 B vector, 0 = first and last vector of each message
  unsigned long long* stamps;         // sender: iters + 2 entries; receiver: iters entries
  unsigned int* status;               // [0] bit 0 = deadline, [1] = wrong 16 B vectors
  unsigned long long timeout_ticks;
};
constexpr int kMaxStreamRoles = 16;
constexpr unsigned long long kMaxStreamBytes = 1ull << 20;      // per message
constexpr unsigned long long kMaxStreamRingBytes = 4ull << 20;  // depth * bytes
constexpr int kMaxStreamDepth = 64;
constexpr int kMaxStreamIters = 100000;
struct StreamArgs {
  StreamRole role[kMaxStreamRoles];
  int nroles;
};
// Checks every role's bounds and pointers (a P2P_CHECK each) before it launches.
void launch_stream(const StreamRole* roles, int nroles, hipStream_t stream);

// ---- what these kernels spin on and count in (pingpong.hip) ----
// Memory for flags a wave spins on: uncached device memory when the runtime
// allows it, so the spinning wave reads HBM rather than a stale line; plain
// hipMalloc otherwise.  *uncached (if given) says which one it became.
hipError_t alloc_signal_page(void** p, size_t bytes, bool* uncached = nullptr);
// Ticks per second of the clock the deadlines and stamps count in
// (s_memrealtime), as the device reports it; 0 if it reports none.
double wall_clock_hz(int device);

}  // namespace dev
}  // namespace p2p
