// Host-side launch API of the background-load kernels (load.hip), and the
// factory of the BackgroundLoad the GPU transports hand out (load.cpp).
//
//   load_mfma  every wave builds a 32x16 A and a 16x32 B bf16 fragment in
//              registers from prng_word(seed, ...), keyed by workgroup and
//              wave, every element ((w % 31) - 15) / 8, so every product and
//              every sum is exact in f32.  It runs `reps` pairs of
//              v_mfma_f32_32x32x16_bf16, +A.B then -A.B with the negated
//              fragment (the accumulator stays bounded), then one final +A.B,
//              and stores its 32x32 tile: whatever `reps`, exactly A.B.
//              (2 reps + 1) x 32768 FLOP per wave; no LDS and no global
//              traffic in the loop.
//   load_hbm   grid-stride non-temporal 16 B loads over a buffer, `passes`
//              times; the 64-bit sum of its 32-bit words per workgroup.
//
// Both share a prologue and an epilogue (LoadCtl).  Prologue: the workgroup
// reads `cancel` (pinned host memory) once; if it is set it does no work and
// leaves `out` alone.  Epilogue: it takes a ticket from a device counter; the
// workgroup that draws the launch's last ticket resets the counter and, when
// no workgroup of the launch was cancelled, publishes done = ordinal + 1
// (pinned host memory, system-scope release).  Nothing spins, nothing waits
// on the host: every launch does a fixed amount of work and ends.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>

#include "background_load.hpp"

namespace p2p {
namespace dev {

struct LoadCtl {
  const unsigned int* cancel = nullptr;   // pinned host word, or null: never cancelled
  unsigned long long* done = nullptr;     // pinned host word, or null: nothing published
  unsigned long long* tickets = nullptr;  // device counter, 0 between launches; needed with `done`
  unsigned long long ordinal = 0;         // this launch's number, from 0
};

constexpr int kLoadBlock = 256;                    // 4 waves, one per SIMD
constexpr int kLoadWaves = kLoadBlock / 64;
constexpr size_t kLoadTileFloats = 32 * 32;        // per wave
constexpr double kLoadMfmaFlop = 2.0 * 32 * 32 * 16;  // one 32x32x16 MFMA

// Word `i` of the stream as an operand element: ((w % 31) - 15) / 8.
// A of wave g (= workgroup * 4 + wave) is words [g * 1024, +512) as A[row][k]
// (row-major 32x16), B the next 512 as B[k][col] (row-major 16x32).
// out: wgs * 4 tiles of 1024 floats in the C/D register layout: float
// lane * 16 + reg of a tile is C[row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)][col = lane & 31].
void launch_load_mfma(int wgs, uint32_t reps, uint64_t seed, float* out, const LoadCtl& ctl, hipStream_t stream);
// bytes: a multiple of 4096.  out: wgs 64-bit sums.
void launch_load_hbm(const void* p, size_t bytes, uint32_t passes, int wgs, unsigned long long* out, const LoadCtl& ctl,
                     hipStream_t stream);

}  // namespace dev

// One per GPU: a non-blocking stream of its own, the pinned cancel and done
// words and (hbm) a 256 MiB scratch buffer, on the current device.  wgs 0: one
// workgroup per CU.  Waits are bounded by `timeout_s`.  `beside`: the stream
// the transfers run on; the load's stream is then chosen among a few
// candidates as one whose kernels overlap that stream's (streams that share a
// hardware queue run one after the other).  Null: no such choice is made.
std::unique_ptr<BackgroundLoad> make_background_load(const std::string& kind, int wgs, double timeout_s,
                                                     hipStream_t beside = nullptr);

}  // namespace p2p
