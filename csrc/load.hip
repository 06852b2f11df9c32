// gfx950 background-load kernels (load.hpp): a matrix-core load and an
// HBM-streaming load, each a short launch of fixed work that a train of
// launches repeats (BackgroundLoad, load.cpp).
#include "load.hpp"

#include "common.hpp"
#include "hip_check.hpp"
#include "prng.hpp"

namespace p2p {
namespace dev {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kHbmUnroll = 4;  // 16 B loads a lane issues back to back per full tile (the stride verify kernel's depth)

// ---- shared prologue / epilogue ----

// Workgroup-uniform: one lane reads the host's word, every wave takes the same
// branch (the hbm kernel's reduction has a barrier in it).
__device__ __forceinline__ bool load_cancelled(const LoadCtl& c) {
  __shared__ unsigned int cancel_seen;
  if (threadIdx.x == 0)
    cancel_seen = c.cancel ? __hip_atomic_load(c.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0u;
  __syncthreads();
  return cancel_seen != 0;
}

// One ticket per workgroup, cancelled or not, so the counter always returns to
// 0 at the end of a launch; a cancelled workgroup marks the upper half, and a
// launch with a mark is not counted as done.
__device__ __forceinline__ void load_epilogue(const LoadCtl& c, bool cancelled) {
  if (!c.tickets) return;
  __syncthreads();  // every wave of the workgroup has issued its stores
  if (threadIdx.x != 0) return;
  const unsigned long long inc = cancelled ? (1ull << 32) + 1ull : 1ull;
  const unsigned long long now =
      __hip_atomic_fetch_add(c.tickets, inc, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + inc;
  if (static_cast<unsigned int>(now) != gridDim.x) return;
  __hip_atomic_store(c.tickets, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (c.done && (now >> 32) == 0)
    __hip_atomic_store(c.done, c.ordinal + 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- matrix-core load ----

// ((w % 31) - 15) / 8 as bf16 bits: a multiple of 1/8 below 2 in magnitude has
// at most 5 significant bits, so the upper half of its f32 form is exact.
__device__ __forceinline__ short operand_bits(uint64_t seed, uint64_t word) {
  const float v = static_cast<float>(static_cast<int>(prng_word(seed, word) % 31u) - 15) * 0.125f;
  return static_cast<short>(__float_as_uint(v) >> 16);
}

__global__ __launch_bounds__(kLoadBlock) void load_mfma_kernel(uint32_t reps, uint64_t seed, float* __restrict__ out,
                                                               const LoadCtl ctl) {
  const bool cancelled = load_cancelled(ctl);
  if (!cancelled) {
    const unsigned lane = threadIdx.x & 63u;
    const uint64_t g = static_cast<uint64_t>(blockIdx.x) * kLoadWaves + threadIdx.x / 64u;
    const uint64_t base = g * 1024u;
    const unsigned r = lane & 31u, h = lane >> 5;
    // Lane l holds A[row r][k = 8h + j] and B[k = 8h + j][col r], j = 0..7.
    s16x8 a, na, b;
#pragma unroll
    for (unsigned j = 0; j < 8; ++j) {
      const unsigned k = 8u * h + j;
      a[j] = operand_bits(seed, base + r * 16u + k);
      na[j] = static_cast<short>(a[j] ^ static_cast<short>(0x8000));
      b[j] = operand_bits(seed, base + 512u + k * 32u + r);
    }
    const bf16x8 fa = __builtin_bit_cast(bf16x8, a), fna = __builtin_bit_cast(bf16x8, na),
                 fb = __builtin_bit_cast(bf16x8, b);
    f32x16 acc = {0};
    uint32_t i = 0;
    for (; i + 8 <= reps; i += 8) {  // 8 pairs per trip: 16 MFMAs per branch
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fna, fb, acc, 0, 0, 0);
      }
    }
    for (; i < reps; ++i) {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fna, fb, acc, 0, 0, 0);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc, 0, 0, 0);
    f32x4* tile = reinterpret_cast<f32x4*>(out + base + lane * 16u);
#pragma unroll
    for (int q = 0; q < 4; ++q) tile[q] = f32x4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
  }
  load_epilogue(ctl, cancelled);
}

// ---- HBM-streaming load ----

__device__ __forceinline__ unsigned long long word_sum(const u32x4 v) {
  return static_cast<unsigned long long>(v.x) + v.y + static_cast<unsigned long long>(v.z) + v.w;
}

__global__ __launch_bounds__(kLoadBlock) void load_hbm_kernel(const u32x4* __restrict__ p, uint64_t nvec, uint32_t passes,
                                                              unsigned long long* __restrict__ out, const LoadCtl ctl) {
  const bool cancelled = load_cancelled(ctl);
  if (!cancelled) {
    unsigned long long sum = 0;
    const uint64_t tile = static_cast<uint64_t>(kLoadBlock) * kHbmUnroll;
    for (uint32_t pass = 0; pass < passes; ++pass) {
      asm volatile("" ::: "memory");  // every pass loads again
      for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * tile; base < nvec;
           base += static_cast<uint64_t>(gridDim.x) * tile) {
        // nvec is a multiple of the block (the buffer of 4 KiB), so whether a
        // 256-vector piece lies inside is the same for every lane: a scalar
        // test, no per-lane branch between the loads.  A full tile issues its
        // four loads back to back before the first add waits for one.
        const u32x4* q = p + base + threadIdx.x;
        if (base + tile <= nvec) {
          u32x4 v[kHbmUnroll];
#pragma unroll
          for (int u = 0; u < kHbmUnroll; ++u) v[u] = __builtin_nontemporal_load(q + u * kLoadBlock);
#pragma unroll
          for (int u = 0; u < kHbmUnroll; ++u) sum += word_sum(v[u]);
        } else {  // the buffer's last, partial tile
          for (uint64_t piece = base; piece < nvec; piece += kLoadBlock, q += kLoadBlock)
            sum += word_sum(__builtin_nontemporal_load(q));
        }
      }
    }
    // Wave64 butterfly, the 4 wave partials through LDS, one store per
    // workgroup (kernels.hip block_commit's pattern).
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    __shared__ unsigned long long red[kLoadWaves];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x / 64] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long t = red[0];
#pragma unroll
      for (int w = 1; w < kLoadWaves; ++w) t += red[w];
      out[blockIdx.x] = t;
    }
  }
  load_epilogue(ctl, cancelled);
}

void check_ctl(const LoadCtl& ctl) {
  P2P_CHECK(!ctl.done || ctl.tickets, "load: a done word needs a ticket counter");
}

}  // namespace

void launch_load_mfma(int wgs, uint32_t reps, uint64_t seed, float* out, const LoadCtl& ctl, hipStream_t stream) {
  P2P_CHECK(wgs >= 1, "load_mfma: at least one workgroup");
  P2P_CHECK(out != nullptr, "load_mfma: no output buffer");
  check_ctl(ctl);
  hipLaunchKernelGGL(load_mfma_kernel, dim3(static_cast<unsigned>(wgs)), dim3(kLoadBlock), 0, stream, reps, seed, out, ctl);
  HIPCHECK(hipGetLastError());
}

void launch_load_hbm(const void* p, size_t bytes, uint32_t passes, int wgs, unsigned long long* out, const LoadCtl& ctl,
                     hipStream_t stream) {
  P2P_CHECK(wgs >= 1, "load_hbm: at least one workgroup");
  P2P_CHECK(p != nullptr && out != nullptr, "load_hbm: no buffer");
  P2P_CHECK(bytes > 0 && bytes % 4096 == 0, "load_hbm: the buffer must be a multiple of 4 KiB");
  check_ctl(ctl);
  hipLaunchKernelGGL(load_hbm_kernel, dim3(static_cast<unsigned>(wgs)), dim3(kLoadBlock), 0, stream,
                     static_cast<const u32x4*>(p), static_cast<uint64_t>(bytes / 16), passes, out, ctl);
  HIPCHECK(hipGetLastError());
}

}  // namespace dev
}  // namespace p2p
