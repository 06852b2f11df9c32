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
//   sum     — multi-source receive-and-reduce for the IPC transport (--reduce,
//             reduce.hip): K loads in flight per lane, one store; with it the
//             operand fill and the check of a reduced buffer
//   gsum    — the same launch as a gated sum over rows (--reduce-gate,
//             reduce_gate.hip): the expert combine, a row's 8 gates read once
//             per wave through the scalar cache; the gate fill and the check
//   wire    — block-scaled payloads for the IPC transport (--wire, wire.hip):
//             the receive that widens MXFP8 / MXFP4 to bf16 as it pulls, the
//             sender's pack, and the check of an unpacked buffer
//   wsum    — receive-and-reduce of wire images (--reduce-wire, wire_reduce.hip):
//             K MXFP8 / MXFP4 images summed in f32 into bf16 in one launch,
//             and the check of such a sum
//   wpack   — the same sum requantised (--reduce-out wire, wire_reduce_pack.hip):
//             K images in, one image of their bf16 sum out, in one launch,
//             and the check of such an image
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
#include "reduce_gate_op.hpp"
#include "reduce_op.hpp"
#include "wire_op.hpp"
#include "wire_reduce_op.hpp"

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

// ---- multi-source receive-and-reduce (reduce.hip; --reduce) ----
// The pull engine's other data plane: op i loads `bytes` from each of its nsrc
// sources and stores their sum (reduce_op.hpp: element type, operand order)
// to dst, which may be one of the sources (each lane reads a vector before it
// writes it).  One workgroup per 4 KiB of output, one 16 B vector per lane;
// a lane issues all nsrc 16 B loads before its first add, so nsrc links are
// in flight at once (nsrc = 8: 32 VGPRs).  Bit i of coherent_mask: source i
// is a hipIpc-mapped peer buffer and is read with the copy's system-scope
// (sc0 sc1) raw-buffer loads, one range-checked descriptor per 4 KiB chunk;
// bit kReduceDstCoherent: dst is one and is written with the coherent store.
// Local sources and dst use non-temporal accesses.  No LDS: nothing is reused.
// nsrc is a template parameter dispatched on the host (load burst and add
// chain unrolled); a launch carries consecutive ops of equal nsrc, up to
// kMaxReduceOps by value in the kernarg, so it stays graph-capturable.
// `bytes` is a multiple of 4 (a P2P_CHECK); the 4 / 8 / 12-byte tail is done
// word-wise by lanes 0..2 of the op's first workgroup.  Ops above 4 GiB and
// max_blocks as in launch_multi_copy.
constexpr int kMaxReduceSrcs = 8;
constexpr int kMaxReduceOps = 8;
constexpr uint32_t kReduceDstCoherent = 1u << kMaxReduceSrcs;
struct ReduceOp {
  void* dst = nullptr;
  size_t bytes = 0;
  int nsrc = 0;
  const void* src[kMaxReduceSrcs] = {};
  uint32_t coherent_mask = 0;
  // bf16 only, a fan-in spread over several launches (launch_reduce_wide):
  // partial_in: src[0] and src[1] are the f32 planes of a running sum (the low
  // halves' sums, the high halves'), `bytes` each; partial_out: the sum is
  // stored as those planes, unrounded, to dst and dst_hi (local memory).
  bool partial_in = false, partial_out = false;
  void* dst_hi = nullptr;
};
void launch_multi_reduce(const ReduceOp* ops, int nops, ReduceType dtype, hipStream_t stream, int max_blocks = 0);
// A fan-in above kMaxReduceSrcs: the first launch sums operands 0..7, each
// further one the running sum plus more, in operand order, so the bits are
// those of one chain.  u32 and f32 carry the running sum in dst (operand 0 of
// the next launch, up to 7 more beside it).  bf16 must not round in between:
// its running sum travels as two f32 planes in `partial`, local scratch of
// reduce_partial_bytes(bytes) that only such a call needs (up to 6 more
// operands beside them), and the last launch rounds into dst.  coherent[i]
// flags source i.
constexpr size_t reduce_partial_bytes(size_t bytes) { return 2 * ((bytes + 15) / 16 * 16); }
void launch_reduce_wide(void* dst, size_t bytes, const void* const* srcs, const unsigned char* coherent, int nsrcs,
                        bool dst_coherent, ReduceType dtype, hipStream_t stream, int max_blocks = 0,
                        void* partial = nullptr);
// Operand stream `seed` (reduce_op.hpp operand_word over the fill's stream),
// the fill kernel's grid; `bytes` a multiple of 4.  U32 is launch_fill.
void launch_fill_operand(void* p, size_t bytes, uint64_t seed, ReduceType dtype, hipStream_t stream);
// Regenerates the nseeds (<= kMaxReduceSeeds) operand streams, sums them with
// reduce_op.hpp's function and compares with p word by word (a bf16 word
// counts once if either half differs); the totals end in acc[0] like
// launch_verify's (reset acc first).  Register staging: never inside timing.
void launch_verify_reduced(const void* p, size_t bytes, const uint64_t* seeds, int nseeds, ReduceType dtype,
                           VerifyAccum* acc, hipStream_t stream);

// ---- gated receive-and-reduce (reduce_gate.hip; --reduce-gate) ----
// The expert combine of a MoE layer in the same one launch: op i's `bytes` are
// rows of row_elems bf16 (a multiple of 512, so a row is whole KiB; bytes whole
// rows: P2P_CHECKs), and row r of dst is sum_k gate[r][k] * src[k][r]
// (reduce_gate_op.hpp: f32 chains in operand order, one rounding).  `gate` is
// local memory, bytes / (2 * row_elems) entries of 16 B (8 bf16 gates, gate k
// operand k's), read-only while the kernel runs.  A wave's 1 KiB lies in one
// row: it reads that row's entry once per chunk with a scalar 16 B load issued
// ahead of the lane's nsrc vector loads, and the gates enter the multiplies as
// scalar operands.  Sources, dst, coherent_mask, max_blocks and the grouping of
// ops into launches (equal nsrc, up to kMaxReduceOps) as launch_multi_reduce;
// ops above 4 GiB go in pieces of whole rows.  No tail path.
struct GatedReduceOp {
  void* dst = nullptr;
  size_t bytes = 0;
  int nsrc = 0;
  const void* src[kMaxReduceSrcs] = {};
  uint32_t coherent_mask = 0;
  const void* gate = nullptr;
  size_t row_elems = 0;
};
void launch_gated_reduce(const GatedReduceOp* ops, int nops, hipStream_t stream, int max_blocks = 0);
// `rows` table entries from PRNG stream `seed` (reduce_gate_op.hpp gate_word): gates in [2^-4, 1).
void launch_fill_gate(void* p, size_t rows, uint64_t seed, hipStream_t stream);
// launch_verify_reduced for a gated sum: regenerates the nseeds (<= 8) bf16
// operand streams and the table of gate_seed, and compares word by word; the
// totals end in acc[0] (reset acc first).  Never inside timing.
void launch_verify_gated_reduced(const void* p, size_t bytes, const uint64_t* seeds, int nseeds, uint64_t gate_seed,
                                 size_t row_elems, VerifyAccum* acc, hipStream_t stream);

// ---- block-scaled wire formats (wire.hip; --wire) ----
// The pull engine's third data plane: op i reads the MXFP8 / MXFP4 wire image
// (wire_op.hpp: wire_bytes(payload_bytes)) at src and stores payload_bytes of
// bf16 to dst.  A 256-thread workgroup takes whole tiles (128 blocks, 8 KiB
// of payload), 16 elements per lane: 16 B / 8 B element loads and one scale
// byte load per unit, v_cvt_scalef32_pk_bf16_fp8 / _fp4, two 16 B stores.
// coherent: src is a hipIpc-mapped peer buffer and is read with system-scope
// (sc0 sc1) raw-buffer loads through one range-checked descriptor per tile;
// dst_coherent: dst is one and is written the same way.  Local memory uses
// non-temporal accesses.  Up to kMaxUnpackOps ops per launch by value in the
// kernarg (more: further launches), workgroups split over them by tiles
// (split_blocks); max_blocks > 0 caps the grid and the kernel strides.
// payload_bytes is a multiple of 64 (a P2P_CHECK).  `lanes` picks the lane
// mapping: Split (a lane's two units lie 4 KiB of payload apart, both stores
// coalesced), Contiguous (one wider load, stores with a 32 B lane stride);
// Auto is the one measured faster.  mxfp6 (24 B blocks, one block per lane and
// v_cvt_scalef32_pk32_bf16_fp6; wire6_lane.hpp) maps `lanes` onto its own two
// store paths: Contiguous is four 16 B stores straight from the lane (64 B
// lane stride), Split sends the wave's 4 KiB through a wave-private LDS slot
// and stores fully coalesced; Auto is Split.  The same holds for
// launch_wire_reduce, whose mxfp6 kernel keeps 32 f32 accumulators per lane;
// launch_wire_reduce_packed's mxfp6 kernel has store paths of its own (below).
constexpr int kMaxUnpackOps = 32;
enum class WireLanes : int { Auto = 0, Contiguous = 1, Split = 2 };
struct UnpackOp {
  void* dst = nullptr;
  const void* src = nullptr;
  size_t payload_bytes = 0;
  bool coherent = false;
  bool dst_coherent = false;
};
void launch_multi_unpack(const UnpackOp* ops, int nops, WireFormat fmt, hipStream_t stream, int max_blocks = 0,
                         WireLanes lanes = WireLanes::Auto);
// The sender's quantise step: payload_bytes of bf16 -> the wire image.  A lane
// loads the 2 (mxfp8) or 4 (mxfp4) vectors that yield one 16 B element store;
// the scale bytes of a tile leave through LDS as 16 B stores.
void launch_pack(void* wire, const void* payload, size_t payload_bytes, WireFormat fmt, hipStream_t stream);
// The same kernel fed by wire_operand_word over the fill's stream `seed`: a
// send region gets the wire image of its operand stream, no bf16 staging.
void launch_fill_packed(void* wire, size_t payload_bytes, uint64_t seed, WireFormat fmt, hipStream_t stream);
// Regenerates operand stream `seed`, applies wire_op.hpp's pack and unpack
// per block (4 lanes each) and compares with p word by word; the totals end
// in acc[0] like launch_verify's (reset acc first).  Never inside timing.
void launch_verify_unpacked(const void* p, size_t payload_bytes, uint64_t seed, WireFormat fmt, VerifyAccum* acc,
                            hipStream_t stream);

// ---- receive-and-reduce of wire images (wire_reduce.hip; --reduce-wire) ----
// The pull engine's fourth data plane: every one of the nsrc sources is the
// MXFP8 / MXFP4 wire image of payload_bytes of bf16, and dst receives
// payload_bytes of bf16, the sum of the dequantised operands in source order
// (wire_reduce_op.hpp: f32 add chain, one rounding).  One op per launch, as
// the engine posts one reduce per group.  A 256-thread workgroup takes whole
// tiles, 16 elements per lane; a lane issues the nsrc element loads and scale
// byte loads of a tile before its first conversion (nsrc is a template
// parameter dispatched on the host), keeps 16 f32 accumulators and ends in two
// 16 B non-temporal stores to dst (local memory).  Bit k of coherent_mask:
// source k is a hipIpc-mapped peer buffer, read with system-scope (sc0 sc1)
// raw-buffer loads through one range-checked descriptor per tile; other
// sources use non-temporal loads.  payload_bytes is a multiple of 64, buffers
// are 16 B aligned, nsrc is 1..8 (a P2P_CHECK each).  max_blocks > 0 caps the
// grid and the kernel strides; `lanes` as in launch_multi_unpack, Auto being
// the mapping measured faster for the format and fan-in.
struct WireReduceOp {
  void* dst = nullptr;
  size_t payload_bytes = 0;
  int nsrc = 0;
  const void* src[kMaxWireReduceSrcs] = {};
  uint32_t coherent_mask = 0;
  // --reduce-own bf16: src[0] is the receiver's own shard, payload_bytes of
  // bf16 in local memory (bit 0 of coherent_mask clear, a P2P_CHECK), not an
  // image; it begins the f32 chains unquantised (wire_reduce_op.hpp own_bf16).
  // A lane loads its 16 own elements as two 16 B non-temporal loads (split: 4
  // KiB apart, both coalesced; contiguous: its 32 B) with the tile's other
  // loads and widens them with shifts and masks; the mxfp6 kernel, a block per
  // lane, reads the wave's 4 KiB coalesced and turns it into rows through the
  // store stage's LDS slot (wire6_lane.hpp load_block).  OWN is a template
  // parameter beside the fan-in: the all-image kernels are unchanged.
  bool own_bf16 = false;
  // --reduce-out both (launch_wire_reduce_packed only; launch_wire_reduce wants
  // it null, a P2P_CHECK): payload_bytes of bf16 in local memory, 16 B aligned,
  // that receive what the image in dst widens to, wire_unpack of it: every
  // sum word under wire_roundtrip_word with the block's scale byte.
  void* dst_bf16 = nullptr;
};
void launch_wire_reduce(const WireReduceOp& op, WireFormat fmt, hipStream_t stream, int max_blocks = 0,
                        WireLanes lanes = WireLanes::Auto);
// Regenerates the nseeds (<= kMaxWireReduceSrcs) operand streams, packs and
// unpacks each per block (4 lanes each), sums them with reduce_op.hpp's
// functions and compares with p word by word; the totals end in acc[0] like
// launch_verify's (reset acc first).  Never inside timing.
// own_bf16: operand 0 (seeds[0]) enters as the raw stream.
// roundtrip: p is the bf16 output of --reduce-out both: after summing, the
// block's amax of the sums is completed over its 4 lanes and every sum word
// goes through wire_roundtrip_word (the integer functions) before comparing.
void launch_verify_wire_reduced(const void* p, size_t payload_bytes, const uint64_t* seeds, int nseeds, WireFormat fmt,
                                VerifyAccum* acc, hipStream_t stream, bool own_bf16 = false, bool roundtrip = false);
// payload_bytes of bf16: operand stream `seed` (wire_operand_word over the
// fill's stream) unquantised, the own shard of a --reduce-own bf16 sum; what
// launch_fill_packed packs.  The fill kernel's geometry.
void launch_fill_wire_operand(void* p, size_t payload_bytes, uint64_t seed, hipStream_t stream);

// ---- the same hop with a requantised output (wire_reduce_pack.hip; --reduce-out wire) ----
// launch_wire_reduce whose op.dst receives wire_bytes(payload_bytes, fmt)
// bytes: the wire image, in the operands' format, of the bf16 sum (wire_op.hpp
// wire_pack_block of wire_reduce_op.hpp's sum: the f32 chain is rounded once
// to bf16, and that value is quantised under the no-clip scale of the block's
// bf16 amax), padding zeroed, bit-identical to launch_wire_reduce into scratch
// followed by launch_pack.  Load side and lane mappings as launch_wire_reduce;
// the epilogue rounds the 16 accumulators to bf16, completes the block's amax
// over its 4 (split) or 2 (contiguous) lanes with xor shuffles, narrows with
// the scaled conversions and stores the codes with 16 B / 8 B (contiguous) or
// two 8 B / 4 B (split) non-temporal stores; the tile's 128 scale bytes and
// their padding leave as 16 B stores through a double-buffered LDS stage, one
// barrier per tile.  Same argument rules as launch_wire_reduce; dst is local.
// Auto is contiguous here, the mapping measured faster in every cell, and
// split when op.dst_bf16 is given: its 8 KiB of bf16 per tile then dominate.
// op.dst_bf16 non-null (--reduce-out both, the turn-around hop of a two-shot
// all-reduce): the same launch also stores wire_unpack of that image there, so
// the owner keeps exactly what its peers will reconstruct; a lane widens its
// own codes back with the unpack's conversion under the same scale operand and
// adds two 16 B stores.  Bit-identical to this launch without dst_bf16 followed
// by launch_multi_unpack of dst.
// mxfp6 is served by a kernel of its own (wire_reduce_pack6.hip): a lane per
// block, 256 lanes and two tiles per workgroup, amax, scale byte and the pk32
// conversions inside the lane, no workgroup barrier; contiguous stores 24 B per
// lane as three 8 B stores, split sends a wave's 1536 B of codes through its
// LDS slot and stores coalesced 16 B chunks; Auto is split for mxfp6.
void launch_wire_reduce_packed(const WireReduceOp& op, WireFormat fmt, hipStream_t stream, int max_blocks = 0,
                               WireLanes lanes = WireLanes::Auto);
// The mxfp6 kernel behind launch_wire_reduce_packed, which has checked op.
void launch_wire_reduce_packed6(const WireReduceOp& op, hipStream_t stream, int max_blocks, WireLanes lanes);
// The check of such an image, in launch_verify_wire_reduced's geometry (one
// payload vector per lane, 4 lanes per block): regenerates and sums the
// operand streams, takes the block's amax of the sums, quantises with the
// integer functions and compares the image's code words and scale byte.  A
// wrong 32-bit word of codes counts once, a wrong scale byte once; first_bad is
// the lowest byte offset in the image of either; the checksum sums the code
// words and the scale bytes; the padding is not read.  mxfp6: a lane's 8
// codes are 6 bytes at a 6-byte stride (wire_code_bits6), not whole words; one
// mismatch is one such 6-byte group with any wrong bit (four groups a block),
// first_bad its first byte, and the checksum adds the group as a 48-bit number.
void launch_verify_wire_reduced_packed(const void* image, size_t payload_bytes, const uint64_t* seeds, int nseeds,
                                       WireFormat fmt, VerifyAccum* acc, hipStream_t stream, bool own_bf16 = false);

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
