// Co-tenancy workload: what one tenant of a shared card runs while another
// process runs next to it.
//   * cu_tenant_run — a series of back-to-back launches of one fixed piece of
//     work, either register-resident FP32 FMA chains ("fma"), a read-only
//     stream over one large allocation ("stream"), repeated reads of a
//     working set that every workgroup keeps to itself ("cache"), a walk
//     along a chain of dependent loads, one in flight per wave ("chase"), or
//     MFMAs (bf16, or the fp8, mxfp8 or mxfp4 form) issued back to back on
//     operands held in registers or re-read from LDS every step ("mfma"),
//     each launch stamped with the device's constant-rate wall clock. The
//     clock is the card's, not the
//     process's, so two separate processes can lay their launches side by
//     side afterwards and see which of them really ran at the same time
//     (agent/cotenancy.py).
//
// Same conventions as cumask.hip. Every kernel runs a fixed iteration count,
// waits on nothing another kernel or process does, and leaves its results
// through ordinary vector stores or atomics. The stream of a call is created,
// used and destroyed inside it (RAII), a masked one under the process-wide
// masked-stream lock.
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "common.h"

namespace py = pybind11;
using gpuprobe::DevBuf;
using gpuprobe::EventGuard;
using gpuprobe::MaskWords;
using gpuprobe::StreamGuard;
using gpuprobe::pattern_word;
using gpuprobe::require_device;

namespace {

constexpr int kBlock = 256;       // 4 waves
constexpr int kGroupsPerCu = 32;  // 8 resident per CU: four fills of the card
constexpr int kCacheGroupsPerCu = 8;  // "cache": one fill, every chunk live at once
constexpr int kFmaChains = 16;
constexpr int kStreamUnroll = 4;  // independent 16-byte loads in flight per lane
constexpr int kMaxLaunches = 64;
constexpr int kWavesPerGroup = kBlock / 64;
constexpr uint64_t kNodeBytes = 128;  // "chase": one node is one cache line
constexpr uint64_t kNodeWords = kNodeBytes / 8;
constexpr int kMaxChaseIters = 1 << 22;
constexpr int kMfmaGroupsPerCu = 8;  // "mfma": one wave per SIMD already fills the pipe
constexpr int kMfmaVariants = 16;    // operand sets; wave w uses w % 16
constexpr int kMaxMfmaIters = 1 << 20;
constexpr double kMfmaFlopsPerK = 2.0 * 32 * 32;  // one 32x32xK MFMA, per unit of K
constexpr uint64_t kGiB = 1ULL << 30;
constexpr uint64_t kMiB = 1ULL << 20;

// ---- stamps ----------------------------------------------------------------

// A launch's record is two words, {min start, max end} of wall_clock64(), set
// to {~0, 0} by the host. One workgroup contributes one pair: its start is read
// by thread 0 before a barrier that every wave's work comes after, its end
// after a barrier that every wave reaches with its result store complete.
// So the record spans the work of every wave of the grid.
__device__ inline unsigned long long stamp_start() {
  const unsigned long long t = wall_clock64();
  __syncthreads();
  return t;
}

__device__ inline void stamp_end(unsigned long long* __restrict__ rec,
                                 unsigned long long t0) {
  // The lane's result store has left the wave before the barrier is joined.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const unsigned long long t1 = wall_clock64();
  if (threadIdx.x == 0) {
    atomicMin(&rec[0], t0);
    atomicMax(&rec[1], t1);
  }
}

// ---- fma -------------------------------------------------------------------

// kFmaChains independent FMA chains per lane, all in registers; every lane
// stores its sum once at the end.
__global__ void __launch_bounds__(kBlock)
tenant_fma_kernel(float* __restrict__ out, int iters, float a, float b,
                  unsigned long long* __restrict__ rec) {
  const unsigned long long t0 = stamp_start();
  float x[kFmaChains];
#pragma unroll
  for (int c = 0; c < kFmaChains; ++c)
    x[c] = static_cast<float>(threadIdx.x + c) * (1.0f / (kBlock + kFmaChains));
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int c = 0; c < kFmaChains; ++c) x[c] = __builtin_fmaf(x[c], a, b);
  }
  float sum = 0.0f;
#pragma unroll
  for (int c = 0; c < kFmaChains; ++c) sum += x[c];
  out[static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x] = sum;
  stamp_end(rec, t0);
}

// ---- stream ----------------------------------------------------------------

// buf[i] = {pattern(2i), pattern(2i+1)}, one 16-byte store per element,
// grid-stride. n16 counts 16-byte elements; all indices are 64-bit.
__global__ void __launch_bounds__(kBlock)
tenant_fill_kernel(ulonglong2* __restrict__ buf, uint64_t n16, uint64_t seed) {
  uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
  for (; i < n16; i += stride) {
    ulonglong2 v;
    v.x = pattern_word(seed, 2 * i);
    v.y = pattern_word(seed, 2 * i + 1);
    buf[i] = v;
  }
}

using u64x2 = __attribute__((ext_vector_type(2))) unsigned long long;

__device__ inline uint64_t load_fold(const u64x2* p) {
  const u64x2 v = __builtin_nontemporal_load(p);
  return v.x ^ v.y;
}

// Reads the whole buffer `passes` times, grid-stride, kStreamUnroll
// independent 16-byte non-temporal loads per lane and step, and XOR-folds
// what it read; the elements past the last whole step are read one at a time.
// Every index is below n16. `passes` is odd, so each lane's fold over all
// passes equals its fold over one pass, and the XOR of every lane's word is
// the XOR of the buffer.
__global__ void __launch_bounds__(kBlock)
tenant_stream_kernel(const u64x2* __restrict__ buf, uint64_t n16, int passes,
                     unsigned long long* __restrict__ out,
                     unsigned long long* __restrict__ rec) {
  const unsigned long long t0 = stamp_start();
  const uint64_t lane = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
  uint64_t fold = 0;
  for (int p = 0; p < passes; ++p) {
    uint64_t i = lane;
    for (; i + (kStreamUnroll - 1) * stride < n16; i += kStreamUnroll * stride) {
      uint64_t f[kStreamUnroll];
#pragma unroll
      for (int u = 0; u < kStreamUnroll; ++u) f[u] = load_fold(buf + i + u * stride);
#pragma unroll
      for (int u = 0; u < kStreamUnroll; ++u) fold ^= f[u];
    }
    for (; i < n16; i += stride) fold ^= load_fold(buf + i);
    // Nothing read in one pass may stand in for a load of the next.
    asm volatile("" ::: "memory");
  }
  out[lane] = fold;
  stamp_end(rec, t0);
}

// ---- cache -----------------------------------------------------------------

__device__ inline uint64_t load_fold_cached(const u64x2* p) {
  const u64x2 v = *p;  // default cache policy: the line stays in L1, L2 and beyond
  return v.x ^ v.y;
}

// Workgroup b reads its own elements [b * n16 / grid, (b + 1) * n16 / grid)
// `passes` times with plain 16-byte loads, kStreamUnroll independent ones per
// lane and step, the elements past the last whole step one at a time, and
// XOR-folds what it read. The grid is one resident fill of the card, so every
// chunk is live for the whole launch, and a workgroup never leaves its CU, so
// its chunk is re-read through one XCD's L2. A chunk may be empty; the last
// one ends at n16, so every index is below n16. `passes` is odd, as in
// tenant_stream_kernel.
__global__ void __launch_bounds__(kBlock)
tenant_cache_kernel(const u64x2* __restrict__ buf, uint64_t n16, int passes,
                    unsigned long long* __restrict__ out,
                    unsigned long long* __restrict__ rec) {
  const unsigned long long t0 = stamp_start();
  const uint64_t b = blockIdx.x, grid = gridDim.x;
  const uint64_t begin = b * n16 / grid, end = (b + 1) * n16 / grid;
  uint64_t fold = 0;
  for (int p = 0; p < passes; ++p) {
    uint64_t i = begin + threadIdx.x;
    for (; i + (kStreamUnroll - 1) * kBlock < end; i += kStreamUnroll * kBlock) {
      uint64_t f[kStreamUnroll];
#pragma unroll
      for (int u = 0; u < kStreamUnroll; ++u)
        f[u] = load_fold_cached(buf + i + u * kBlock);
#pragma unroll
      for (int u = 0; u < kStreamUnroll; ++u) fold ^= f[u];
    }
    for (; i < end; i += kBlock) fold ^= load_fold_cached(buf + i);
    // Nothing read in one pass may stand in for a load of the next.
    asm volatile("" ::: "memory");
  }
  out[b * kBlock + threadIdx.x] = fold;
  stamp_end(rec, t0);
}

// ---- chase -----------------------------------------------------------------

// The buffer is `nodes` nodes of one 128-byte line each; every 8-byte word of
// node i holds next(i) = (i + stride) % nodes. One 16-byte store of {next,
// next} per element, grid-stride. n16 = 8 * nodes counts 16-byte elements;
// stride < nodes (0 for a single node), so one subtraction wraps; all indices
// are 64-bit.
__global__ void __launch_bounds__(kBlock)
tenant_chase_fill_kernel(ulonglong2* __restrict__ buf, uint64_t n16, uint64_t nodes,
                         uint64_t stride) {
  uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kBlock;
  for (; i < n16; i += step) {
    uint64_t next = i / (kNodeBytes / 16) + stride;
    if (next >= nodes) next -= nodes;
    ulonglong2 v;
    v.x = next;
    v.y = next;
    buf[i] = v;
  }
}

// Wave w of the W = 4 x grid starts at node (seed + w * nodes / W) % nodes
// (`seed` arrives already reduced modulo nodes) and hops `iters` times: every
// lane loads word (lane & 15) of the current node and takes what it loaded as
// the next node. The sixteen words of a node are equal, so the lanes of a wave
// stay together, but each lane's address is its own: the compiler cannot know
// the addresses to be uniform across the wave, so the hop has to be a vector
// memory load of one 128-byte line per wave and can never be served by the
// scalar cache. The load is a plain one under the default cache policy, and
// the next address depends on it, so a wave has exactly one load in flight.
// Every value stored by the fill is below `nodes`, so every word index is
// below 16 * nodes; a node's byte offset reaches 16 GiB and is 64-bit.
__global__ void __launch_bounds__(kBlock)
tenant_chase_kernel(const unsigned long long* __restrict__ buf, uint64_t nodes,
                    uint64_t seed, int iters, unsigned long long* __restrict__ out,
                    unsigned long long* __restrict__ rec) {
  const uint64_t waves = static_cast<uint64_t>(gridDim.x) * kWavesPerGroup;
  const uint64_t w = static_cast<uint64_t>(blockIdx.x) * kWavesPerGroup + threadIdx.x / 64;
  const uint64_t word = threadIdx.x & (kNodeWords - 1);
  uint64_t node = (seed + w * nodes / waves) % nodes;
  const unsigned long long t0 = stamp_start();
  for (int i = 0; i < iters; ++i) node = buf[node * kNodeWords + word];
  out[static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x] = node;
  stamp_end(rec, t0);
}

// The stride of the chain: the first of s0, s0 + 1, ... that is coprime to
// `nodes`, s0 = floor(nodes * 28657 / 46368) (two Fibonacci numbers, a ratio
// of about 0.618). Coprime, so the chain is one cycle through every node; 0
// for a single node. Integers only: agent/cotenancy.py states the same rule
// on its own.
uint64_t chase_stride(uint64_t nodes) {
  auto gcd = [](uint64_t a, uint64_t b) {
    while (b) {
      const uint64_t t = a % b;
      a = b;
      b = t;
    }
    return a;
  };
  uint64_t s = nodes * 28657 / 46368;
  while (gcd(s, nodes) != 1) ++s;
  return s;
}

// ---- mfma ------------------------------------------------------------------

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using short8 = __attribute__((ext_vector_type(8))) short;
using int4v = __attribute__((ext_vector_type(4))) int;
using int8v = __attribute__((ext_vector_type(8))) int;
using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ inline uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

// The instruction an mfma tenant issues. The id enters the operand hashes,
// so no two forms multiply the same matrices.
enum MfmaFormId : int { kBf16 = 0, kFp8 = 1, kMxfp8 = 2, kMxfp4 = 3 };
constexpr int kMfmaForms = 4;

// Per form: the K of one MFMA, the steps between two folds of the
// accumulators (the largest partial sum of a chunk stays below 2^23, see the
// kernel) and the steps of a default launch, about as long for every form.
// agent/cotenancy.py keeps the same table.
struct MfmaFormInfo {
  const char* name;
  int k, chunk, default_iters;
};
constexpr MfmaFormInfo kMfmaFormTable[kMfmaForms] = {
    {"bf16", 16, 2048, 32768},
    {"fp8", 16, 2048, 32768},
    {"mxfp8", 64, 512, 16384},
    {"mxfp4", 64, 256, 32768},
};

// Operands from LDS (tenant_mfma_lds_kernel): a workgroup's image is one slot
// per wave, and a slot is the bytes a wave reads per step, in planes of 64
// lanes x 16 bytes: bf16 and mxfp4 one plane per fragment, mxfp8 two, fp8
// one for A0|A1 and one for B0|B1, the block-scaled forms one more for the
// scales. LDS per workgroup is 4 slots: 16, 8, 36 and 20 KiB.
// agent/cotenancy.py keeps the same table.
constexpr int kMfmaLdsSlots = kWavesPerGroup;
constexpr int kMfmaLdsPlaneBytes = 64 * 16;
constexpr int kMfmaLdsStepBytes[kMfmaForms] = {4096, 2048, 9216, 5120};

// The hashes behind A[row][k] and B[k][col] of one operand variant and, for
// the block-scaled forms, behind the scale of a row's or column's block of 32
// k. Hashed, so nothing is symmetric in its two indices; for bf16 (F = 0) the
// form's bits vanish. agent/cotenancy.py states the same rules on its own.
template <int F>
__device__ inline uint32_t mfma_a_hash(uint32_t key, uint32_t row, uint32_t k) {
  return mix32(key ^ (row << 8) ^ k ^ 0x00A00000u ^ (static_cast<uint32_t>(F) << 24));
}
template <int F>
__device__ inline uint32_t mfma_b_hash(uint32_t key, uint32_t k, uint32_t col) {
  return mix32(key ^ (k << 8) ^ col ^ 0x00B00000u ^ (static_cast<uint32_t>(F) << 24));
}
template <int F>
__device__ inline uint32_t mfma_a_scale_bit(uint32_t key, uint32_t row, uint32_t blk) {
  return mix32(key ^ (row << 8) ^ blk ^ 0x00E00000u ^ (static_cast<uint32_t>(F) << 24)) & 1u;
}
template <int F>
__device__ inline uint32_t mfma_b_scale_bit(uint32_t key, uint32_t blk, uint32_t col) {
  return mix32(key ^ (blk << 8) ^ col ^ 0x00F00000u ^ (static_cast<uint32_t>(F) << 24)) & 1u;
}

// Small integers are exact in bf16: the bf16 is the float's upper half.
__device__ inline short to_bf16_bits(int v) {
  return static_cast<short>(__float_as_uint(static_cast<float>(v)) >> 16);
}

// -15..15 as OCP e4m3fn (bias 7, three mantissa bits): 1 is 0x38, 15 is 0x57.
__device__ inline uint32_t to_e4m3_bits(int v) {
  if (v == 0) return 0u;
  const uint32_t mag = static_cast<uint32_t>(v < 0 ? -v : v);
  const uint32_t e = 31u - static_cast<uint32_t>(__builtin_clz(mag));  // 0..3
  return (v < 0 ? 0x80u : 0u) | ((e + 7u) << 3) | ((mag << (3u - e)) & 7u);
}

// One wave's operand fragments of a form: two of A, two of B and, for the
// block-scaled forms, the E8M0 scale (byte 0: 2^(byte - 127)) that goes with
// each. Lane r = lane & 31, h = lane >> 5 of fragment t holds row or column
// 32t + r, element j in the j-th slot of the lane's registers from the low
// end: a bf16 per 16 bits, an e4m3 per byte, an e2m1 per nibble. For bf16
// and fp8 that is k = 8h + j, j = 0..7, and for mxfp4 k = 32h + j, j = 0..31:
// the lane's four dwords are block h of 32 k. For mxfp8 a lane's eight dwords
// are half of each block, dwords 0..3 k = 16h + j and dwords 4..7 k = 32 +
// 16h + (j - 16): the instruction scales a lane's low four dwords by the
// scale register of lane r and its high four by that of lane r + 32 (found
// on the card with exact data: with k = 32h + j every product came out as if
// scaled that way). In both block-scaled forms the scale register of lane r +
// 32h holds the scale of block h. A and B follow the same rule, so whatever
// order the instruction gives the k inside a block, it pairs equal k.
//   bf16, fp8: h % 31 - 15.
//   mxfp8: h % 15 - 7, scale byte 127 + e on both sides: |element| <= 14.
//   mxfp4: the code h & 15 as it is, +-(0, 0.5, 1, 1.5, 2, 3, 4, 6)[code & 7],
//          negative with code & 8; A's scale byte 128 + e, B's 128: every
//          effective element is an integer, |A| <= 24 and |B| <= 12.
template <int F>
struct MfmaFrags;

template <>
struct MfmaFrags<kBf16> {
  bf16x8 a[2], b[2];
  __device__ void build(uint32_t key, uint32_t r, uint32_t h) {
#pragma unroll
    for (uint32_t t = 0; t < 2; ++t) {
      short8 af, bf;
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) {
        af[j] = to_bf16_bits(
            static_cast<int>(mfma_a_hash<kBf16>(key, 32 * t + r, 8 * h + j) % 31u) - 15);
        bf[j] = to_bf16_bits(
            static_cast<int>(mfma_b_hash<kBf16>(key, 8 * h + j, 32 * t + r) % 31u) - 15);
      }
      a[t] = __builtin_bit_cast(bf16x8, af);
      b[t] = __builtin_bit_cast(bf16x8, bf);
    }
  }
  __device__ void pin() {
    asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]));
  }
  __device__ f32x16 mfma(int m, int n, f32x16 c) const {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m], b[n], c, 0, 0, 0);
  }
  static constexpr int kLdsPlanes = 4;  // A0, A1, B0, B1
  __device__ void to_lds(int4v* slot, uint32_t lane) const {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      slot[64 * t + lane] = __builtin_bit_cast(int4v, a[t]);
      slot[64 * (2 + t) + lane] = __builtin_bit_cast(int4v, b[t]);
    }
  }
  __device__ void from_lds(const int4v* slot, uint32_t lane) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      a[t] = __builtin_bit_cast(bf16x8, slot[64 * t + lane]);
      b[t] = __builtin_bit_cast(bf16x8, slot[64 * (2 + t) + lane]);
    }
  }
};

template <>
struct MfmaFrags<kFp8> {
  long a[2], b[2];
  __device__ void build(uint32_t key, uint32_t r, uint32_t h) {
#pragma unroll
    for (uint32_t t = 0; t < 2; ++t) {
      uint64_t af = 0, bf = 0;
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) {
        af |= static_cast<uint64_t>(to_e4m3_bits(
                  static_cast<int>(mfma_a_hash<kFp8>(key, 32 * t + r, 8 * h + j) % 31u) - 15))
              << (8 * j);
        bf |= static_cast<uint64_t>(to_e4m3_bits(
                  static_cast<int>(mfma_b_hash<kFp8>(key, 8 * h + j, 32 * t + r) % 31u) - 15))
              << (8 * j);
      }
      a[t] = static_cast<long>(af);
      b[t] = static_cast<long>(bf);
    }
  }
  __device__ void pin() {
    asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]));
  }
  __device__ f32x16 mfma(int m, int n, f32x16 c) const {
    return __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a[m], b[n], c, 0, 0, 0);
  }
  // A fragment is 8 bytes per lane: A0|A1 side by side in one plane, B0|B1
  // in the other, so that the reads are 16 bytes wide like every other form's.
  static constexpr int kLdsPlanes = 2;
  using long2v = __attribute__((ext_vector_type(2))) long;
  __device__ void to_lds(int4v* slot, uint32_t lane) const {
    slot[lane] = __builtin_bit_cast(int4v, long2v{a[0], a[1]});
    slot[64 + lane] = __builtin_bit_cast(int4v, long2v{b[0], b[1]});
  }
  __device__ void from_lds(const int4v* slot, uint32_t lane) {
    const long2v av = __builtin_bit_cast(long2v, slot[lane]);
    const long2v bv = __builtin_bit_cast(long2v, slot[64 + lane]);
    a[0] = av[0];
    a[1] = av[1];
    b[0] = bv[0];
    b[1] = bv[1];
  }
};

template <>
struct MfmaFrags<kMxfp8> {
  int8v a[2], b[2];
  int sa[2], sb[2];
  __device__ void build(uint32_t key, uint32_t r, uint32_t h) {
#pragma unroll
    for (uint32_t t = 0; t < 2; ++t) {
#pragma unroll
      for (uint32_t d = 0; d < 8; ++d) {
        uint32_t aw = 0, bw = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
          const uint32_t k = 32 * (d >> 2) + 16 * h + 4 * (d & 3) + q;
          aw |= to_e4m3_bits(
                    static_cast<int>(mfma_a_hash<kMxfp8>(key, 32 * t + r, k) % 15u) - 7)
                << (8 * q);
          bw |= to_e4m3_bits(
                    static_cast<int>(mfma_b_hash<kMxfp8>(key, k, 32 * t + r) % 15u) - 7)
                << (8 * q);
        }
        a[t][d] = static_cast<int>(aw);
        b[t][d] = static_cast<int>(bw);
      }
      sa[t] = static_cast<int>(127u + mfma_a_scale_bit<kMxfp8>(key, 32 * t + r, h));
      sb[t] = static_cast<int>(127u + mfma_b_scale_bit<kMxfp8>(key, h, 32 * t + r));
    }
  }
  __device__ void pin() {
    asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]));
    asm volatile("" : "+v"(sa[0]), "+v"(sa[1]), "+v"(sb[0]), "+v"(sb[1]));
  }
  __device__ f32x16 mfma(int m, int n, f32x16 c) const {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[m], b[n], c, 0, 0, 0, sa[m], 0,
                                                           sb[n]);
  }
  // Two planes per fragment, the lane's low four dwords and its high four,
  // in the order A0, A1, B0, B1, then the plane of {sa[0], sa[1], sb[0], sb[1]}.
  static constexpr int kLdsPlanes = 9;
  __device__ void to_lds(int4v* slot, uint32_t lane) const {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      slot[64 * (2 * t) + lane] = int4v{a[t][0], a[t][1], a[t][2], a[t][3]};
      slot[64 * (2 * t + 1) + lane] = int4v{a[t][4], a[t][5], a[t][6], a[t][7]};
      slot[64 * (4 + 2 * t) + lane] = int4v{b[t][0], b[t][1], b[t][2], b[t][3]};
      slot[64 * (5 + 2 * t) + lane] = int4v{b[t][4], b[t][5], b[t][6], b[t][7]};
    }
    slot[64 * 8 + lane] = int4v{sa[0], sa[1], sb[0], sb[1]};
  }
  __device__ void from_lds(const int4v* slot, uint32_t lane) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int4v al = slot[64 * (2 * t) + lane], ah = slot[64 * (2 * t + 1) + lane];
      const int4v bl = slot[64 * (4 + 2 * t) + lane], bh = slot[64 * (5 + 2 * t) + lane];
      a[t] = int8v{al[0], al[1], al[2], al[3], ah[0], ah[1], ah[2], ah[3]};
      b[t] = int8v{bl[0], bl[1], bl[2], bl[3], bh[0], bh[1], bh[2], bh[3]};
    }
    const int4v s = slot[64 * 8 + lane];
    sa[0] = s[0];
    sa[1] = s[1];
    sb[0] = s[2];
    sb[1] = s[3];
  }
};

template <>
struct MfmaFrags<kMxfp4> {
  int4v a[2], b[2];  // the low four of the instruction's eight dwords
  int sa[2], sb[2];
  __device__ void build(uint32_t key, uint32_t r, uint32_t h) {
#pragma unroll
    for (uint32_t t = 0; t < 2; ++t) {
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d) {
        uint32_t aw = 0, bw = 0;
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) {
          const uint32_t k = 32 * h + 8 * d + q;
          aw |= (mfma_a_hash<kMxfp4>(key, 32 * t + r, k) & 15u) << (4 * q);
          bw |= (mfma_b_hash<kMxfp4>(key, k, 32 * t + r) & 15u) << (4 * q);
        }
        a[t][d] = static_cast<int>(aw);
        b[t][d] = static_cast<int>(bw);
      }
      sa[t] = static_cast<int>(128u + mfma_a_scale_bit<kMxfp4>(key, 32 * t + r, h));
      sb[t] = 128;
    }
  }
  __device__ void pin() {
    asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]));
    asm volatile("" : "+v"(sa[0]), "+v"(sa[1]), "+v"(sb[0]), "+v"(sb[1]));
  }
  __device__ static int8v widen(int4v v) {
    return int8v{v[0], v[1], v[2], v[3], 0, 0, 0, 0};
  }
  __device__ f32x16 mfma(int m, int n, f32x16 c) const {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(widen(a[m]), widen(b[n]), c, 4, 4,
                                                           0, sa[m], 0, sb[n]);
  }
  static constexpr int kLdsPlanes = 5;  // A0, A1, B0, B1, {sa[0], sa[1], sb[0], sb[1]}
  __device__ void to_lds(int4v* slot, uint32_t lane) const {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      slot[64 * t + lane] = a[t];
      slot[64 * (2 + t) + lane] = b[t];
    }
    slot[64 * 4 + lane] = int4v{sa[0], sa[1], sb[0], sb[1]};
  }
  __device__ void from_lds(const int4v* slot, uint32_t lane) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      a[t] = slot[64 * t + lane];
      b[t] = slot[64 * (2 + t) + lane];
    }
    const int4v s = slot[64 * 4 + lane];
    sa[0] = s[0];
    sa[1] = s[1];
    sb[0] = s[2];
    sb[1] = s[3];
  }
};

// Every wave owns a 64x64 output tile, 2 x 2 accumulators of 32x32, and keeps
// two A fragments (rows 32m + r) and two B fragments (columns 32n + r) of the
// form's K in registers (MfmaFrags above); output register reg is row (reg &
// 3) + 8 * (reg >> 2) + 4h of column r, for every form. The fragments are
// built once, before the start stamp, from variant (global wave) % 16 of the
// hashes above. One step is the four MFMAs acc[m][n] += A_m x B_n; `iters`
// steps run in chunks of at most the form's chunk. A chunk starts from zero
// accumulators and ends with every lane folding its 64 registers into a
// 64-bit sum, each weighted by 1 + reg + 16 * (2m + n). Per step |A x B| <=
// 16 * 15 * 15 = 3600 (bf16, fp8), 64 * 14 * 14 = 12544 (mxfp8), 64 * 24 * 12
// = 18432 (mxfp4), and 2048 * 3600, 512 * 12544 and 256 * 18432 are all below
// 2^23, so every partial sum is exact in f32, its conversion to int is exact,
// and the fold is linear in the number of steps. Nothing is read from memory
// between the stamps.
//
// clk is the launch's {sum of shader cycles, sum of wall ticks}: thread 0 of
// every workgroup reads s_memtime next to each end of its wall-clock interval
// and adds both differences. cycles / ticks x tick_hz is the shader clock the
// launch ran at, averaged over its workgroups.
using MfmaTile = f32x16[2][2];

// The key of the variant that global wave w builds.
__device__ inline uint32_t mfma_key(uint32_t seed32, uint32_t w) {
  return mix32(seed32 ^ ((w % kMfmaVariants) * 0x9E3779B1u));
}

__device__ inline void mfma_zero(MfmaTile& acc) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc[t >> 1][t & 1][reg] = 0.0f;
}

// One step: acc[m][n] += A_m x B_n.
template <int F>
__device__ inline void mfma_step(const MfmaFrags<F>& frags, MfmaTile& acc) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
    acc[t >> 1][t & 1] = frags.mfma(t >> 1, t & 1, acc[t >> 1][t & 1]);
}

// Adds a chunk to the lane's fold.
__device__ inline void mfma_fold(const MfmaTile& acc, uint64_t& fold) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg)
      fold += static_cast<uint64_t>(static_cast<int64_t>(
                  static_cast<int>(acc[t >> 1][t & 1][reg]))) *
              static_cast<uint64_t>(1 + reg + 16 * t);
}

// The lane's store, the end stamp and the workgroup's share of clk.
__device__ inline void mfma_finish(unsigned long long* __restrict__ out,
                                   unsigned long long* __restrict__ rec,
                                   unsigned long long* __restrict__ clk, uint64_t fold,
                                   unsigned long long c0, unsigned long long t0) {
  out[static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x] = fold;
  stamp_end(rec, t0);
  if (threadIdx.x == 0) {
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    const unsigned long long t1 = wall_clock64();
    atomicAdd(&clk[0], c1 - c0);
    atomicAdd(&clk[1], t1 - t0);
  }
}

template <int F>
__global__ void __launch_bounds__(kBlock)
tenant_mfma_kernel(uint32_t seed32, int iters, unsigned long long* __restrict__ out,
                   unsigned long long* __restrict__ rec,
                   unsigned long long* __restrict__ clk) {
  constexpr int kChunk = kMfmaFormTable[F].chunk;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = lane & 31u, h = lane >> 5;
  const uint32_t w = blockIdx.x * kWavesPerGroup + threadIdx.x / 64;
  MfmaFrags<F> frags;
  frags.build(mfma_key(seed32, w), r, h);
  // The fragments are in their registers before either clock is read.
  frags.pin();
  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  const unsigned long long t0 = stamp_start();
  uint64_t fold = 0;
  for (int done = 0; done < iters; done += kChunk) {
    const int steps = min(iters - done, kChunk);
    f32x16 acc[2][2];
    mfma_zero(acc);
    for (int i = 0; i < steps; ++i) mfma_step(frags, acc);
    mfma_fold(acc, fold);
  }
  mfma_finish(out, rec, clk, fold, c0, t0);
}

// The order of a step of tenant_mfma_lds_kernel: the step's `reads` LDS reads
// spread over the gaps in front of its first three MFMAs, at most `per_gap`
// in each, so that no gap carries more reads than the LDS array serves
// beside the MFMA, and none is issued later than three MFMAs before the
// step that needs it.
template <int reads, int per_gap>
__device__ inline void mfma_lds_interleave() {
  constexpr int n0 = reads < per_gap ? reads : per_gap;
  constexpr int n1 = reads - n0 < per_gap ? reads - n0 : per_gap;
  constexpr int n2 = reads - n0 - n1;
  static_assert(n2 <= per_gap + 1, "the reads fit the first three gaps");
  __builtin_amdgcn_sched_group_barrier(0x100, n0, 0);  // DS reads
  __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
  __builtin_amdgcn_sched_group_barrier(0x100, n1, 0);
  __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
  __builtin_amdgcn_sched_group_barrier(0x100, n2, 0);
  __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
}

// The same tenant with its operands re-read from LDS before every step, as a
// GEMM or an attention kernel re-reads its own. Grid, tile, the four MFMAs of
// a step, chunks, fold, stamps and cycle sums are tenant_mfma_kernel's.
//
// Before either clock is read, wave j (0..3) of workgroup b builds the
// fragments of its own variant (4b + j) % 16, as above, and stores them to
// slot j of the workgroup's image (layout: MfmaFrags<F>::to_lds and the table
// at kMfmaLdsStepBytes: every fragment lane-contiguous in planes of 16 bytes
// per lane, address = plane base + 16 x lane, so every read is a 16-byte one
// in which no two lanes of a group share a bank); a workgroup barrier closes
// the fill. At step i of the launch, counted across chunks, global wave w
// multiplies the fragments of slot (w + i) & 3, which are those of variant
// (w & ~3) % 16 + ((w + i) & 3). The slot index is masked to 0..3, so every
// address is inside the image.
//
// Two register sets: the reads of step i + 1 are issued in front of the first
// three MFMAs of step i (mfma_lds_interleave) and are first needed after its
// last, so that one wave per SIMD hides the LDS latency behind its own MFMAs
// (the wait is the counted one the compiler places in front of the first
// use). The last step of a launch reads one slot
// more than it multiplies. The slot changes every step and a compiler barrier
// closes every step, so nothing a wave read for one step stands in for a
// later one. Nothing is read from global memory between the stamps.
//
// The per-step bounds on |A x B| hold for every variant, so the chunks and the
// exactness argument above (every partial sum below 2^23) carry over
// unchanged; the fold is linear in the number of steps of each of the four
// slots (agent/cotenancy.py, mfma_checksum(operands="lds")).
template <int F>
__global__ void __launch_bounds__(kBlock)
tenant_mfma_lds_kernel(uint32_t seed32, int iters, unsigned long long* __restrict__ out,
                       unsigned long long* __restrict__ rec,
                       unsigned long long* __restrict__ clk) {
  constexpr int kChunk = kMfmaFormTable[F].chunk;
  constexpr int kSlotVecs = MfmaFrags<F>::kLdsPlanes * 64;
  static_assert(kSlotVecs * 16 == kMfmaLdsStepBytes[F], "the table is the layout's");
  // Two 16-byte reads per 32 cycles of MFMA.
  constexpr int kReadsPerGap = F == kMxfp8 ? 4 : 2;
  static_assert(kChunk % 4 == 0, "a chunk starts on the first register set and on slot j");
  __shared__ int4v image[kMfmaLdsSlots][kSlotVecs];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = lane & 31u, h = lane >> 5;
  const uint32_t j = threadIdx.x / 64;
  const uint32_t w = blockIdx.x * kWavesPerGroup + j;
  MfmaFrags<F> f0, f1;
  f0.build(mfma_key(seed32, w), r, h);
  f0.to_lds(image[j], lane);
  __syncthreads();
  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  const unsigned long long t0 = stamp_start();
  uint64_t fold = 0;
  f0.from_lds(image[j], lane);  // step 0
  for (int done = 0; done < iters; done += kChunk) {
    const int steps = min(iters - done, kChunk);
    f32x16 acc[2][2];
    mfma_zero(acc);
    // Step done + i multiplies slot (j + done + i) & 3; done is a multiple of 4.
    int i = 0;
    for (; i + 1 < steps; i += 2) {
      f1.from_lds(image[(j + i + 1) & 3u], lane);
      mfma_step(f0, acc);
      mfma_lds_interleave<MfmaFrags<F>::kLdsPlanes, kReadsPerGap>();
      asm volatile("" ::: "memory");
      f0.from_lds(image[(j + i + 2) & 3u], lane);
      mfma_step(f1, acc);
      mfma_lds_interleave<MfmaFrags<F>::kLdsPlanes, kReadsPerGap>();
      asm volatile("" ::: "memory");
    }
    if (i < steps) {  // an odd last chunk
      mfma_step(f0, acc);
      asm volatile("" ::: "memory");
    }
    mfma_fold(acc, fold);
  }
  mfma_finish(out, rec, clk, fold, c0, t0);
}

// ---- host ------------------------------------------------------------------

enum class Kind : int { kFma, kStream, kCache, kChase, kMfma };
constexpr int kKinds = 5;
// Per kind: name, workgroups per CU (chase: one, that is one wave per SIMD),
// whether it reads a buffer filled beforehand, whether it takes form and operands.
struct KindInfo {
  const char* name;
  int groups_per_cu;
  bool reads, matrix;
};
constexpr KindInfo kKindTable[kKinds] = {
    {"fma", kGroupsPerCu, false, false},   {"stream", kGroupsPerCu, true, false},
    {"cache", kCacheGroupsPerCu, true, false}, {"chase", 1, true, false},
    {"mfma", kMfmaGroupsPerCu, false, true}};

// The kernel of an mfma tenant: [operands from LDS][form].
using MfmaKernel = decltype(&tenant_mfma_kernel<kBf16>);
constexpr MfmaKernel kMfmaKernels[2][kMfmaForms] = {
    {tenant_mfma_kernel<kBf16>, tenant_mfma_kernel<kFp8>, tenant_mfma_kernel<kMxfp8>,
     tenant_mfma_kernel<kMxfp4>},
    {tenant_mfma_lds_kernel<kBf16>, tenant_mfma_lds_kernel<kFp8>,
     tenant_mfma_lds_kernel<kMxfp8>, tenant_mfma_lds_kernel<kMxfp4>}};

double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  const size_t n = v.size();
  return n % 2 ? v[n / 2] : 0.5 * (v[n / 2 - 1] + v[n / 2]);
}

// 64-bit words on the host and their copy on the device; none, nothing to copy.
struct Mirror {
  std::vector<unsigned long long>& h;
  DevBuf d;
  void copy(bool up) {  // up: allocates
    if (h.empty()) return;
    if (up) d.alloc(h.size() * sizeof(h[0]));
    HIP_CHECK(hipMemcpy(up ? d.p : h.data(), up ? h.data() : d.p, h.size() * sizeof(h[0]),
                        up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
  }
  unsigned long long* at(size_t word) const { return d.as<unsigned long long>() + word; }
};

struct Launch {
  unsigned long long t0 = 0, t1 = 0;
  double seconds = 0.0, event_seconds = 0.0, rate = 0.0;
  unsigned long long cycles = 0, ticks = 0;  // mfma only
  double clock_ghz = 0.0;                    // mfma only
};

struct TenantResult {
  bool skipped = false;
  uint64_t free_bytes = 0;
  Kind kind = Kind::kFma;
  int form = kBf16;  // mfma only
  bool lds = false;  // mfma only: operands re-read from LDS
  uint64_t lds_bytes = 0, lds_bytes_per_launch = 0;  // mfma from LDS only
  MaskWords applied;
  double tick_hz = 0.0;
  int workgroups = 0;
  uint64_t bytes = 0;
  int iters = 0, passes = 0;
  uint64_t nodes = 0, stride = 0;  // chase only
  double work_per_launch = 0.0;  // flops (fma, mfma), bytes (stream, cache) or hops (chase)
  double bytes_per_cu = 0.0;     // cache only
  std::vector<Launch> launches;
  double rate = 0.0;  // median over launches: GFLOP/s, GB/s or Ghop/s
  double ns_per_hop = 0.0;  // chase only: median over launches
  double clock_ghz = 0.0;   // mfma only: median over launches
  uint64_t checksum = 0;
  // Raw: the last launch's word per lane (fma: none), the stamps, mfma's clocks.
  std::vector<unsigned long long> out, recs, clks;
};

// Plan: what a call launches, from its arguments alone (no HIP call). The grid
// depends on the card, never on the mask: the same work either way. (To a
// process started under ROC_GLOBAL_CU_MASK the runtime reports only that mask's
// CUs, so there the grid is 32 x its own CUs; every rate is over the work launched.)
TenantResult plan_tenant(Kind kind, int cus, int iters, uint64_t bytes, int passes,
                         int form, bool lds) {
  TenantResult r;
  r.kind = kind;
  r.form = form;
  r.lds = lds;
  r.workgroups = kKindTable[static_cast<int>(kind)].groups_per_cu * cus;
  const double lanes = static_cast<double>(r.workgroups) * kBlock;
  const uint64_t waves = static_cast<uint64_t>(r.workgroups) * kWavesPerGroup;
  switch (kind) {
    case Kind::kFma:
      if (iters <= 0) iters = 65536;
      r.iters = std::min(iters, 1 << 18);
      r.work_per_launch = 2.0 * kFmaChains * lanes * r.iters;
      break;
    case Kind::kStream:
    case Kind::kCache: {
      const bool cache = kind == Kind::kCache;
      if (bytes == 0) bytes = cache ? 16 * kMiB : kGiB;
      bytes = std::min<uint64_t>(std::max<uint64_t>(bytes, 16), cache ? kGiB : 16 * kGiB);
      r.bytes = bytes & ~static_cast<uint64_t>(15);
      if (passes <= 0) passes = cache ? 1023 : 127;
      passes = std::min(passes, cache ? 65535 : 4095);
      r.passes = passes | 1;  // odd: the XOR over all passes is that of one
      r.work_per_launch = static_cast<double>(r.bytes) * r.passes;
      if (cache) r.bytes_per_cu = static_cast<double>(r.bytes) / cus;
      break;
    }
    case Kind::kChase:
      if (bytes == 0) bytes = kGiB;
      bytes = std::min<uint64_t>(std::max<uint64_t>(bytes, kNodeBytes), 16 * kGiB);
      r.bytes = bytes & ~(kNodeBytes - 1);
      r.nodes = r.bytes / kNodeBytes;
      r.stride = chase_stride(r.nodes);
      if (iters <= 0) iters = 65536;
      r.iters = std::min(iters, kMaxChaseIters);  // hops per wave and launch
      r.work_per_launch = static_cast<double>(waves) * r.iters;
      break;
    case Kind::kMfma:
      if (iters <= 0) iters = kMfmaFormTable[form].default_iters;
      r.iters = std::min(iters, kMaxMfmaIters);  // steps of four MFMAs per wave and launch
      r.work_per_launch = static_cast<double>(waves) * r.iters * 4.0 * kMfmaFlopsPerK *
                          kMfmaFormTable[form].k;
      if (lds) {
        r.lds_bytes = static_cast<uint64_t>(kMfmaLdsSlots) * kMfmaLdsStepBytes[form];
        r.lds_bytes_per_launch = waves * r.iters * kMfmaLdsStepBytes[form];
      }
      break;
  }
  return r;
}

// Run: buffers, stream, fill, one untimed launch and `launches` timed ones;
// leaves r's raw words, the launches' event_seconds and the stream's mask.
void run_planned(TenantResult& r, int cus, const MaskWords& mask, int launches,
                 uint64_t seed) {
  const dim3 grid(r.workgroups);
  const size_t lanes = static_cast<size_t>(r.workgroups) * kBlock;
  const uint64_t n16 = r.bytes / 16;
  DevBuf buf, out;
  Mirror recs{r.recs}, clks{r.clks};
  // One record {~0, 0} per timed launch, and one more for the warm-up.
  recs.h.assign(2 * static_cast<size_t>(launches + 1), 0ULL);
  for (size_t i = 0; i < recs.h.size(); i += 2) recs.h[i] = ~0ULL;
  if (kKindTable[static_cast<int>(r.kind)].reads) buf.alloc(r.bytes);
  switch (r.kind) {  // what a lane stores, and what else a launch records
    case Kind::kFma:
      out.alloc(lanes * sizeof(float));
      break;
    case Kind::kMfma:  // {sum of shader cycles, sum of wall ticks}, from zero
      clks.h.assign(recs.h.size(), 0ULL);
      [[fallthrough]];
    default:
      r.out.resize(lanes);
      out.alloc(lanes * sizeof(unsigned long long));
  }
  recs.copy(true);
  clks.copy(true);
  HIP_CHECK(hipDeviceSynchronize());
  std::vector<EventGuard> ev(2 * static_cast<size_t>(launches));
  for (auto& e : ev) e.create();
  {
    StreamGuard g;
    gpuprobe::open_stream(g, mask, r.applied);
    const auto go = [&](dim3 blocks, auto kernel, auto... args) {
      hipLaunchKernelGGL(kernel, blocks, dim3(kBlock), 0, g.s, args...);
      HIP_CHECK(hipGetLastError());
    };
    unsigned long long* const o64 = out.as<unsigned long long>();
    const auto launch = [&](int slot) {
      unsigned long long* rec = recs.at(2 * slot);
      switch (r.kind) {
        case Kind::kFma:
          go(grid, tenant_fma_kernel, out.as<float>(), r.iters, 0.999f, 0.001f, rec);
          break;
        case Kind::kStream:
        case Kind::kCache:
          go(grid, r.kind == Kind::kCache ? tenant_cache_kernel : tenant_stream_kernel,
             buf.as<const u64x2>(), n16, r.passes, o64, rec);
          break;
        case Kind::kChase:
          go(grid, tenant_chase_kernel, buf.as<const unsigned long long>(), r.nodes,
             seed % r.nodes, r.iters, o64, rec);
          break;
        case Kind::kMfma:
          go(grid, kMfmaKernels[r.lds][r.form], static_cast<uint32_t>(seed), r.iters, o64,
             rec, clks.at(2 * slot));
          break;
      }
    };
    switch (r.kind) {  // the fill
      case Kind::kStream:
      case Kind::kCache:
        go(grid, tenant_fill_kernel, buf.as<ulonglong2>(), n16, seed);
        break;
      case Kind::kChase:
        go(dim3(kGroupsPerCu * cus), tenant_chase_fill_kernel, buf.as<ulonglong2>(), n16,
           r.nodes, r.stride);
        break;
      default:
        break;
    }
    // Warm-up, not timed: the same launch once, so that the code object is
    // loaded and the clocks have settled under this load before the timed ones.
    launch(launches);
    for (int l = 0; l < launches; ++l) {
      HIP_CHECK(hipEventRecord(ev[2 * l].e, g.s));
      launch(l);
      HIP_CHECK(hipEventRecord(ev[2 * l + 1].e, g.s));
    }
    HIP_CHECK(hipStreamSynchronize(g.s));
    recs.copy(false);
    clks.copy(false);
    if (!r.out.empty())
      HIP_CHECK(hipMemcpy(r.out.data(), out.p, lanes * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost));
  }  // the stream is gone before the result is looked at
  r.launches.resize(launches);
  for (int l = 0; l < launches; ++l) {
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, ev[2 * l].e, ev[2 * l + 1].e));
    r.launches[l].event_seconds = static_cast<double>(ms) * 1e-3;
  }
}

// Summarise: launch entries, medians, the last launch's checksum. No HIP call.
void summarise(TenantResult& r) {
  std::vector<double> rates, own;
  for (size_t l = 0; l < r.launches.size(); ++l) {
    Launch& e = r.launches[l];
    e.t0 = r.recs[2 * l];
    e.t1 = r.recs[2 * l + 1];
    if (e.t0 == ~0ULL || e.t1 <= e.t0)
      throw std::runtime_error("cu_tenant_run: launch " + std::to_string(l) +
                               " left no usable clock record");
    e.seconds = static_cast<double>(e.t1 - e.t0) / r.tick_hz;
    e.rate = r.work_per_launch / e.seconds / 1e9;
    rates.push_back(e.rate);
  }
  r.rate = median(rates);
  switch (r.kind) {
    case Kind::kFma:
      break;
    case Kind::kStream:
    case Kind::kCache:
      for (unsigned long long w : r.out) r.checksum ^= w;
      break;
    case Kind::kChase:
      // Every lane's end node weighted by its global index, both from 1 so
      // that neither lane 0 nor node 0 drops out.
      for (size_t g = 0; g < r.out.size(); ++g) r.checksum += (g + 1) * (r.out[g] + 1);
      for (const auto& e : r.launches) own.push_back(e.seconds * 1e9 / r.iters);
      r.ns_per_hop = median(own);
      break;
    case Kind::kMfma:  // every lane's fold weighted likewise
      for (size_t g = 0; g < r.out.size(); ++g) r.checksum += (g + 1) * r.out[g];
      for (size_t l = 0; l < r.launches.size(); ++l) {
        Launch& e = r.launches[l];
        e.cycles = r.clks[2 * l];
        e.ticks = r.clks[2 * l + 1];
        if (e.ticks == 0)
          throw std::runtime_error("cu_tenant_run: launch " + std::to_string(l) +
                                   " left no usable cycle record");
        e.clock_ghz = static_cast<double>(e.cycles) / static_cast<double>(e.ticks) *
                      r.tick_hz / 1e9;
        own.push_back(e.clock_ghz);
      }
      r.clock_ghz = median(own);
      break;
  }
}

TenantResult run_tenant(int device, const MaskWords& raw_mask, Kind kind, int launches,
                        int iters, uint64_t bytes, int passes, uint64_t seed, int form,
                        bool lds) {
  require_device(device);
  const int cus = gpuprobe::device_cus(device);
  const MaskWords mask =
      raw_mask.empty() ? MaskWords{} : gpuprobe::fit_mask(raw_mask, cus);
  launches = std::min(std::max(launches, 1), kMaxLaunches);
  TenantResult r = plan_tenant(kind, cus, iters, bytes, passes, form, lds);
  if (kKindTable[static_cast<int>(kind)].reads) {
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    r.free_bytes = free_b;
    if (free_b < r.bytes + kGiB) {
      r.skipped = true;
      return r;
    }
  }
  int clock_khz = 0;
  HIP_CHECK(hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate, device));
  if (clock_khz <= 0)
    throw std::runtime_error("cu_tenant_run: device reports no wall-clock rate");
  r.tick_hz = static_cast<double>(clock_khz) * 1e3;
  run_planned(r, cus, mask, launches, seed);
  summarise(r);
  return r;
}

}  // namespace

void register_cotenant(py::module_& m) {
  m.def(
      "cu_tenant_run",
      [](int device, py::object mask, const std::string& kind, int launches, int iters,
         uint64_t bytes, int passes, uint64_t seed, const std::string& form,
         const std::string& operands) {
        const MaskWords words = gpuprobe::mask_from_python(mask);
        int k = 0;
        while (k < kKinds && kind != kKindTable[k].name) ++k;
        if (k == kKinds)
          throw py::value_error(
              "cu_tenant_run: kind must be \"fma\", \"stream\", \"cache\", "
              "\"chase\" or \"mfma\"");
        int f = 0;
        while (f < kMfmaForms && form != kMfmaFormTable[f].name) ++f;
        if (f == kMfmaForms)
          throw py::value_error(
              "cu_tenant_run: form must be \"bf16\", \"fp8\", \"mxfp8\" or \"mxfp4\"");
        if (f != kBf16 && !kKindTable[k].matrix)
          throw py::value_error(
              "cu_tenant_run: form \"" + form + "\" needs kind \"mfma\"; of the forms "
              "\"bf16\", \"fp8\", \"mxfp8\" and \"mxfp4\" every other kind takes only "
              "\"bf16\"");
        if (operands != "registers" && operands != "lds")
          throw py::value_error(
              "cu_tenant_run: operands must be \"registers\" or \"lds\"");
        const bool lds = operands == "lds";
        if (lds && !kKindTable[k].matrix)
          throw py::value_error(
              "cu_tenant_run: operands \"lds\" needs kind \"mfma\"; of the operands "
              "\"registers\" and \"lds\" every other kind takes only \"registers\"");
        TenantResult r;
        {
          py::gil_scoped_release release;
          r = run_tenant(device, words, static_cast<Kind>(k), launches, iters, bytes,
                         passes, seed, f, lds);
        }
        py::dict d;
        if (r.skipped) {
          d["skipped"] = "insufficient free memory";
          d["bytes"] = r.bytes;
          d["free_bytes"] = r.free_bytes;
          return d;
        }
        d["kind"] = kind;
        d["applied_mask"] = gpuprobe::mask_to_python(r.applied);
        d["tick_hz"] = r.tick_hz;
        d["workgroups"] = r.workgroups;
        // The kind's keys, whether a launch has clocks, what follows the rate.
        py::dict last;
        bool clocks = false;
        switch (r.kind) {
          case Kind::kFma:
            d["iters"] = r.iters;
            break;
          case Kind::kStream:
          case Kind::kCache:
            d["bytes"] = r.bytes;
            d["passes"] = r.passes;
            d["checksum"] = r.checksum;
            if (r.kind == Kind::kCache) d["bytes_per_cu"] = r.bytes_per_cu;
            break;
          case Kind::kChase:
            d["bytes"] = r.bytes;
            d["nodes"] = r.nodes;
            d["stride"] = r.stride;
            d["iters"] = r.iters;
            d["checksum"] = r.checksum;
            last["ns_per_hop"] = r.ns_per_hop;
            break;
          case Kind::kMfma:
            d["form"] = kMfmaFormTable[r.form].name;
            d["iters"] = r.iters;
            d["checksum"] = r.checksum;
            if (r.lds) {
              d["operands"] = operands;
              d["lds_bytes"] = r.lds_bytes;
              d["lds_bytes_per_launch"] = r.lds_bytes_per_launch;
            }
            clocks = true;
            last["clock_ghz"] = r.clock_ghz;
            break;
        }
        d["work_per_launch"] = r.work_per_launch;
        py::list launches_out;
        for (const auto& e : r.launches) {
          py::dict l;
          l["t0"] = e.t0;
          l["t1"] = e.t1;
          l["seconds"] = e.seconds;
          l["event_seconds"] = e.event_seconds;
          l["rate"] = e.rate;
          if (clocks) {
            l["cycles"] = e.cycles;
            l["ticks"] = e.ticks;
            l["clock_ghz"] = e.clock_ghz;
          }
          launches_out.append(l);
        }
        d["launches"] = launches_out;
        d["rate"] = r.rate;
        d.attr("update")(last);
        return d;
      },
      py::arg("device") = 0, py::arg("mask") = py::none(), py::arg("kind") = "fma",
      py::arg("launches") = 8, py::arg("iters") = 0, py::arg("bytes") = 0,
      py::arg("passes") = 0, py::arg("seed") = 1, py::arg("form") = "bf16",
      py::arg("operands") = "registers",
      "One tenant's workload, stamped with the card's wall clock. `mask` as in "
      "cu_occupancy (None: a plain stream, which is what a process started "
      "under ROC_GLOBAL_CU_MASK uses); `kind` is \"fma\", \"stream\", "
      "\"cache\", \"chase\" or \"mfma\", anything else raises ValueError "
      "before the device is touched. After one untimed "
      "launch, `launches` (1..64) launches of the same work run back to back "
      "on one stream, each between its own pair of events; the grid is 32 x "
      "CUs workgroups of 256 lanes (cache: 8 x CUs, all resident at once; "
      "chase: 1 x CUs, one wave per SIMD; mfma: 8 x CUs) "
      "whatever `mask` is, CUs being what the device reports to this "
      "process.\n\n"
      "fma: 16 independent FP32 FMA chains of `iters` (default 65536, at most "
      "262144) per lane, in registers. stream: every lane reads one allocation "
      "of `bytes` (default 1 GiB, rounded down to a multiple of 16, clamped to "
      "16 B .. 16 GiB) `passes` times (default 127, at most 4095, an even value "
      "is raised by one) with 16-byte non-temporal loads, four in flight, and "
      "XOR-folds them; the buffer holds pattern_word(`seed`, w), written once "
      "on the same stream before anything is timed. When less than bytes + 1 "
      "GiB is free nothing is allocated and {skipped, bytes, free_bytes} is "
      "returned. A buffer that fits the Infinity Cache (256 MiB) measures the "
      "cache, not HBM.\n\n"
      "cache: workgroup b of the 8 x CUs re-reads its own contiguous 16-byte "
      "elements [b * n / grid, (b + 1) * n / grid) of one allocation of `bytes` "
      "(default 16 MiB, half the aggregate L2; rounded down to a multiple of "
      "16, clamped to 16 B .. 1 GiB) `passes` times (default 1023, at most "
      "65535, an even value is raised by one) with plain 16-byte loads, four "
      "in flight. The whole buffer is live for the whole launch and each "
      "chunk is read through one XCD's L2. A default launch moves 16 GiB, "
      "which a whole card reading its L2 does in 0.6 ms. Filled "
      "and refused like stream; the result adds bytes_per_cu = bytes / "
      "CUs.\n\n"
      "chase: one allocation of `bytes` (default 1 GiB, rounded down to a "
      "multiple of 128, clamped to 128 B .. 16 GiB) is `nodes` = bytes / 128 "
      "nodes of one 128-byte line; all sixteen 8-byte words of node i hold (i "
      "+ `stride`) % nodes, written once on the same stream before anything "
      "is timed. `stride` is the first of s0, s0 + 1, ... coprime to nodes, "
      "s0 = nodes * 28657 // 46368, so the chain is a single cycle through "
      "every node and consecutive hops land far apart (a single node loops "
      "on itself, stride 0). Wave w of the W = 4 x CUs starts at node (`seed` "
      "+ w * nodes // W) % nodes and hops `iters` times (hops per wave and "
      "launch: default 65536, clamped to 1 .. 4194304; `passes` is ignored): "
      "every lane loads word (lane & 15) of the current node with a plain "
      "load and takes the value as the next node, so a wave has exactly one "
      "load of one line in flight; at the end every lane stores its node. "
      "Refused like stream. The result has bytes, nodes, stride, iters in "
      "place of passes, work_per_launch = W * iters hops, rates in Ghop/s, "
      "and adds ns_per_hop = the median over launches of seconds * 1e9 / "
      "iters; its checksum is the sum over all lanes g of (g + 1) * (end node "
      "of g + 1) modulo 2^64, which equals the closed form ((start + iters * "
      "stride) % nodes per wave) only when every wave ended where it should "
      "and its lanes agree. ns_per_hop is one wave's dependent-load latency "
      "only while every workgroup is resident at once: always so for a "
      "process started under ROC_GLOBAL_CU_MASK, whose grid is its own CUs, "
      "but not for an in-process `mask` smaller than 1/8 of the card, under "
      "which workgroups queue behind one another. Every XCD walks the whole "
      "buffer, so the working set fits \"the L2\" only up to 4 MiB, one XCD's "
      "L2, unlike the cache kind, whose chunks spread over the eight L2s.\n\n"
      "mfma: every wave of the 8 x CUs workgroups owns a 64 x 64 output tile "
      "as 2 x 2 accumulators of 32 x 32 and keeps two A and two B fragments "
      "of K = 16 in registers; one step is the four v_mfma_f32_32x32x16_bf16 "
      "acc[m][n] += A_m x B_n, and a wave runs `iters` steps per launch "
      "(default 32768, clamped to 1 .. 1048576; `bytes` and `passes` are "
      "ignored, nothing is allocated and nothing refused). One wave per SIMD "
      "already issues MFMAs back to back, so the rate does not depend on how "
      "many of the eight workgroups are resident. The operands are small "
      "integers, -15 .. 15, exact in bf16, hashed from the low 32 bits of "
      "`seed` and the wave's variant w % 16 before anything is timed: "
      "A[row][k] = mix32(key ^ row << 8 ^ k ^ 0xA00000) % 31 - 15, B[k][col] "
      "likewise with 0xB00000 and k << 8 ^ col, key = mix32(seed32 ^ (w % 16) "
      "* 0x9E3779B1). Steps run in chunks of at most 2048 from zero "
      "accumulators, so every partial sum stays below 2^23 and is exact in "
      "f32; after a chunk every lane adds its 64 accumulator registers, as "
      "integers weighted by 1 + reg + 16 * (2m + n), to a 64-bit sum that it "
      "stores at the end. The result has iters, work_per_launch = waves * "
      "iters * 4 * 32768 flops, rates in GFLOP/s, and checksum = the sum over "
      "all lanes g of (g + 1) * (sum of g) modulo 2^64, which equals the "
      "closed form (agent/cotenancy.py, mfma_checksum) only when every MFMA "
      "of every wave gave the exact product. Thread 0 of every workgroup "
      "also reads the shader-cycle counter (s_memtime) at both ends of its "
      "wall-clock interval; a launch entry adds cycles and ticks, both "
      "summed over the workgroups, and clock_ghz = cycles / ticks * tick_hz "
      "/ 1e9, the shader clock the launch ran at, and the result adds "
      "clock_ghz, the median over launches. The chip lowers its shader clock "
      "under matrix load, chip-wide and whatever the CU mask, and how far "
      "depends on the data: the clock it holds under these small integers "
      "may differ from the one it holds under a real GEMM's operands "
      "(all-zero operands have been seen to run 19 % faster than random "
      "ones at equal cycles), which is why the result reports the clock it "
      "saw and not only the rate.\n\n"
      "mfma, `form`: the instruction, \"bf16\" (the default, everything above), "
      "\"fp8\", \"mxfp8\" or \"mxfp4\"; anything else, or a form other than "
      "\"bf16\" with a kind other than \"mfma\", raises ValueError before the "
      "device is touched. Tile, fragments in registers, steps, fold, clocks "
      "and grid are the same for every form; the result adds form, and "
      "work_per_launch = waves * iters * 4 * the form's flop per MFMA. The "
      "form's id f (0..3 in the order above) enters the hashes: A[row][k] "
      "from mix32(key ^ row << 8 ^ k ^ 0xA00000 ^ f << 24), B[k][col] from "
      "mix32(key ^ k << 8 ^ col ^ 0xB00000 ^ f << 24). fp8: "
      "v_mfma_f32_32x32x16_fp8_fp8 on OCP e4m3fn operands, K = 16, 32768 "
      "flop, the same hash % 31 - 15, chunks of 2048, default 32768 steps. "
      "mxfp8: v_mfma_scale_f32_32x32x64_f8f6f4 on e4m3 operands, K = 64, "
      "131072 flop, hash % 15 - 7, chunks of 512, default 16384 steps (a "
      "step takes twice the cycles). mxfp4: the same instruction on e2m1 "
      "operands, K = 64, 131072 flop, the code hash & 15 stored as it is (+-"
      "(0, 0.5, 1, 1.5, 2, 3, 4, 6)[code & 7], negative with code & 8), "
      "chunks of 256, default 32768 steps. Both block-scaled forms give "
      "every row of A and column of B one E8M0 scale (byte s: 2^(s - 127)) "
      "per block of 32 k, from the bits eA = mix32(key ^ row << 8 ^ blk ^ "
      "0xE00000 ^ f << 24) & 1 and eB = mix32(key ^ blk << 8 ^ col ^ 0xF00000 "
      "^ f << 24) & 1: mxfp8 byte 127 + e on both sides (|element| <= 14), "
      "mxfp4 byte 128 + eA for A (|A| <= 24) and 128 for B (|B| <= 12), so "
      "every effective element is an integer. Lane r + 32 h of fragment t "
      "holds row or column 32 t + r, element j in the j-th slot from the low "
      "end, at k = 8 h + j (bf16, fp8), k = 32 h + j (mxfp4: the lane's four "
      "dwords are block h) or k = 32 (j // 16) + 16 h + j % 16 (mxfp8: the "
      "lane's low four dwords are half of block 0 and its high four half of "
      "block 1, which is how the instruction applies the scales); the scale "
      "register of lane r + 32 h holds the scale of block h; both sides "
      "alike. A chunk's partial "
      "sums stay below 2048 * 3600, 512 * 12544 and 256 * 18432, all below "
      "2^23, so mfma_checksum(..., form) is exact for every form.\n\n"
      "mfma, `operands`: \"registers\" (the default, everything above) or "
      "\"lds\"; anything else, or \"lds\" with a kind other than \"mfma\", "
      "raises ValueError before the device is touched. With \"lds\" every "
      "step's fragments are re-read from LDS, for every form; grid, tile, "
      "steps, chunks, fold, clocks, `iters` and its defaults are the same. "
      "Before anything is timed wave j (0..3) of workgroup b builds the "
      "fragments of its own variant (4 b + j) % 16 and stores them to slot j "
      "of the workgroup's static LDS image of 4 slots; a slot holds A0, A1, "
      "B0, B1 lane-contiguous in planes of 16 bytes per lane (address = plane "
      "base + 16 * lane, so every read is a conflict-free ds_read_b128): one "
      "plane per fragment for bf16 and mxfp4, two for mxfp8 (the lane's low "
      "four dwords, then its high four), for fp8 one plane A0|A1 and one "
      "B0|B1 (8 bytes each, side by side), and for the block-scaled forms one "
      "more plane of {sa[0], sa[1], sb[0], sb[1]}: 4096, 2048, 9216 and 5120 "
      "bytes per slot, 16, 8, 36 and 20 KiB per workgroup (bf16, fp8, mxfp8, "
      "mxfp4). At step i of the launch, counted across chunks, global wave w "
      "multiplies the fragments of slot (w + i) & 3, that is variant (w & ~3) "
      "% 16 + ((w + i) & 3); the reads of step i + 1 are issued in front of the "
      "first three MFMAs of step i, at most two per 32 cycles of MFMA, into a "
      "second register set, and nothing is read from "
      "global memory between the stamps. At full MFMA rate that is 128, 64, "
      "144 and 160 B per clock and CU, below the LDS array's 256. The bounds "
      "per step hold for every variant, so the chunks stay exact; the result "
      "adds operands, lds_bytes (per workgroup) and lds_bytes_per_launch = "
      "waves * iters * the form's bytes per slot, and its checksum equals "
      "mfma_checksum(..., form, \"lds\"). With \"registers\" the result has "
      "none of the three.\n\n"
      "Every launch records {earliest start, latest end} of wall_clock64() over "
      "all its workgroups; the clock runs at `tick_hz` "
      "(hipDeviceAttributeWallClockRate) for every process on the card. Returns "
      "{kind, [form,] applied_mask, tick_hz, workgroups, iters | bytes, passes, checksum, "
      "[operands, lds_bytes, lds_bytes_per_launch,] "
      "[bytes_per_cu,] work_per_launch: flops, bytes or hops, launches: [{t0, t1, "
      "seconds: (t1 - t0) "
      "/ tick_hz, event_seconds, rate[, cycles, ticks, clock_ghz]}], rate[, "
      "clock_ghz]}; rates are GFLOP/s, GB/s or "
      "Ghop/s over "
      "`seconds`, the top-level one the median over launches. checksum (stream "
      "and cache) is the XOR of the words the last launch's lanes stored and "
      "equals "
      "pattern_xor(seed, 0, bytes // 8) when every byte was read.");
}
