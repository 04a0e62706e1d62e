// Co-tenancy workload: what one tenant of a shared card runs while another
// process runs next to it.
//   * cu_tenant_run — a series of back-to-back launches of one fixed piece of
//     work, either register-resident FP32 FMA chains ("fma"), a read-only
//     stream over one large allocation ("stream"), repeated reads of a
//     working set that every workgroup keeps to itself ("cache"), a walk
//     along a chain of dependent loads, one in flight per wave ("chase"), or
//     MFMAs (bf16, or the fp8, mxfp8 or mxfp4 form) issued back to back on
//     operands held in registers or re-read from LDS every step ("mfma"),
//     or a whole GEMM fed from memory through LDS, bf16 ("gemm") or
//     block-scaled ("gemm-mxfp8", "gemm-mxfp4"), or the decode shape of the
//     latter, 32 rows against weights streamed from memory straight into
//     registers ("decode-mxfp8", "decode-mxfp4"), or a causal flash-attention
//     forward pass in bf16 ("attention"),
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
#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>
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

__host__ __device__ inline uint32_t mix32(uint32_t x) {
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

// The end stamp and the workgroup's share of clk, after its result store.
__device__ inline void clocked_end(unsigned long long* __restrict__ rec,
                                   unsigned long long* __restrict__ clk,
                                   unsigned long long c0, unsigned long long t0) {
  stamp_end(rec, t0);
  if (threadIdx.x == 0) {
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    const unsigned long long t1 = wall_clock64();
    atomicAdd(&clk[0], c1 - c0);
    atomicAdd(&clk[1], t1 - t0);
  }
}

// The lane's store, the end stamp and the workgroup's share of clk.
__device__ inline void mfma_finish(unsigned long long* __restrict__ out,
                                   unsigned long long* __restrict__ rec,
                                   unsigned long long* __restrict__ clk, uint64_t fold,
                                   unsigned long long c0, unsigned long long t0) {
  out[static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x] = fold;
  clocked_end(rec, clk, c0, t0);
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

// ---- gemm ------------------------------------------------------------------

constexpr int kGemmTile = 128;  // rows of A, and of B (columns of C), per workgroup
constexpr int kGemmBk = 64;     // k per step
constexpr int kGemmRowVecs = kGemmBk * 2 / 16;           // 16-byte chunks per slab row: 8
constexpr int kGemmSlabVecs = kGemmTile * kGemmRowVecs;  // one operand's slab: 16 KiB
constexpr int kGemmLoads = kGemmSlabVecs / kBlock;       // loads per lane, operand and step: 4
constexpr uint32_t kGemmRowPeriod = 192, kGemmKPeriod = 96;
constexpr uint32_t kGemmKeySalt = 0x47454D4Du;
constexpr int kGemmDefaultIters = 64, kGemmMaxIters = 512;
constexpr int kGemmMaxSide = 32768;
constexpr int kGemmDefaultPasses = 16;
constexpr int kGemmMaxGroups = 1 << 22;
constexpr uint32_t kXcds = 8;          // consecutive workgroup ids go round them
constexpr uint32_t kGemmBandRows = 8;  // tile rows an XCD's workgroups share

// The operands of a gemm tenant: `buf` is A (S x K, row-major) followed by B
// (S x K, row n holding column n of the product's right-hand side), both bf16.
// A[m][k] = mfma_a_hash(key, m % 192, k % 96) % 31 - 15 and B[n][k] =
// mfma_b_hash(key, k % 96, n % 192) % 31 - 15. One 16-byte store of eight
// elements per step, grid-stride; k8 = K / 8 counts the stores of a row and
// n16 = 2 * S * k8 those of both matrices. Eight elements never straddle the
// k period, a multiple of 8. All indices are 64-bit and below n16.
__global__ void __launch_bounds__(kBlock)
tenant_gemm_fill_kernel(int4v* __restrict__ buf, uint64_t n16, uint64_t k8, uint32_t key) {
  uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
  const uint64_t half = n16 / 2;
  for (; i < n16; i += stride) {
    const bool is_b = i >= half;
    const uint64_t at = is_b ? i - half : i;
    const uint32_t row = static_cast<uint32_t>((at / k8) % kGemmRowPeriod);
    const uint32_t k0 = static_cast<uint32_t>((at % k8) * 8 % kGemmKPeriod);
    short8 v;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      const uint32_t h = is_b ? mfma_b_hash<kBf16>(key, k0 + j, row)
                              : mfma_a_hash<kBf16>(key, row, k0 + j);
      v[j] = to_bf16_bits(static_cast<int>(h % 31u) - 15);
    }
    buf[i] = __builtin_bit_cast(int4v, v);
  }
}

// Which tile workgroup i of a pass computes, as (tile row) << 16 | (tile
// column), over side x side tiles (side <= 256). A bijection of 0 .. tiles - 1
// for every tile count, in two steps.
// 1. Consecutive workgroup ids go round-robin over the 8 XCDs, so XCD x runs
//    i = x, x + 8, ...: count(x) = tiles / 8 + (x < tiles % 8) of them. They
//    are given the consecutive positions j = start(x) + i / 8, start(x) = the
//    sum of the counts before x. i < tiles makes i / 8 < count(x), so the j of
//    different XCDs do not meet and together are 0 .. tiles - 1.
// 2. Position j walks the tiles in bands of 8 tile rows (the last band has
//    the rows that are left), down a band's column first: 64 positions in a
//    row are an 8 x 8 block of tiles, which reads 8 row slabs of A and 8 of B
//    where 64 tiles of one row read 1 and 64. j < tiles keeps the column
//    below side.
// The workgroups an XCD has in flight are so neighbours in j and share its L2.
// With GPUPROBE_GEMM_ROW_MAJOR defined the order is the plain one, tile i at
// row i / side; it is what the kept order was measured against
// (profiles/gemm_cotenancy_results.md: about 1 % faster than row-major on the
// whole card, 0.3 % slower on half of it, both near the run-to-run change;
// the kernel waits on load latency, not on bandwidth, so the order decides
// little yet).
__device__ inline uint32_t gemm_order(uint32_t i, uint32_t tiles, uint32_t side) {
#ifdef GPUPROBE_GEMM_ROW_MAJOR
  return (i / side) << 16 | (i % side);
#else
  const uint32_t x = i % kXcds, q = tiles / kXcds, rem = tiles % kXcds;
  const uint32_t j = x * q + min(x, rem) + i / kXcds;
  const uint32_t band = kGemmBandRows * side;
  const uint32_t first = j / band * kGemmBandRows;
  const uint32_t rows = min(side - first, kGemmBandRows);
  const uint32_t in = j % band;
  return (first + in % rows) << 16 | (in / rows);
#endif
}

// Where 16-byte chunk c (0..7, k = 8c .. 8c + 7) of row `row` of a slab
// lives, in 16-byte units: the row's 128 bytes are unpadded and its chunks
// are permuted by an XOR with a key of the row's bits 1, 2 and 3.
__device__ inline uint32_t gemm_key(uint32_t row) {
  return (row & 6u) | ((row >> 3) & 1u);
}
__device__ inline uint32_t gemm_slot(uint32_t row, uint32_t c) {
  return row * kGemmRowVecs + (c ^ gemm_key(row));
}

// One step's sixteen MFMAs of a wave on the slabs {A, B} of `from`. The lane
// reads rows read_a / 8 and read_b / 8 (+ 32 t) of the slabs, chunk (2 s + h)
// ^ read_key at sub-step s.
__device__ inline void gemm_multiply(MfmaTile& acc, const int4v (*from)[kGemmSlabVecs],
                                     uint32_t read_a, uint32_t read_b, uint32_t read_key,
                                     uint32_t h) {
  const auto read = [&](MfmaFrags<kBf16>& f, uint32_t s) {
    const uint32_t c = (2 * s + h) ^ read_key;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f.a[t] = __builtin_bit_cast(bf16x8, from[0][read_a + 32 * kGemmRowVecs * t + c]);
      f.b[t] = __builtin_bit_cast(bf16x8, from[1][read_b + 32 * kGemmRowVecs * t + c]);
    }
  };
  MfmaFrags<kBf16> f[2];
  read(f[0], 0);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (uint32_t s = 0; s < 4; ++s) {
    if (s < 3) read(f[(s + 1) & 1u], s + 1);
    mfma_step(f[s & 1u], acc);
    if (s < 3) mfma_lds_interleave<4, 2>();
  }
  __builtin_amdgcn_sched_barrier(0);
}

// The lane's 64 accumulators as integers, the entry at (m, n), global, weighed
// by (1 + m) (1 + n) modulo 2^64. The wave's tile starts at (row0 + 64 (wave
// >> 1), col0 + 64 (wave & 1)).
__device__ inline uint64_t gemm_tile_sum(const MfmaTile& acc, uint32_t row0, uint32_t col0,
                                         uint32_t wave, uint32_t r, uint32_t h) {
  uint64_t sum = 0;
#pragma unroll
  for (uint32_t t = 0; t < 4; ++t) {
    const uint32_t m = row0 + 64 * (wave >> 1) + 32 * (t >> 1) + 4 * h;
    const uint32_t n = col0 + 64 * (wave & 1u) + 32 * (t & 1u) + r;
    uint64_t column = 0;
#pragma unroll
    for (uint32_t reg = 0; reg < 16; ++reg)
      column += static_cast<uint64_t>(static_cast<int64_t>(
                    static_cast<int>(acc[t >> 1][t & 1][reg]))) *
                static_cast<uint64_t>(1 + m + (reg & 3u) + 8 * (reg >> 2));
    sum += column * static_cast<uint64_t>(1 + n);
  }
  return sum;
}

// The 256 sums of a workgroup added up through LDS, its one word stored by
// thread 0.
__device__ inline void gemm_store_sum(unsigned long long* sums, uint64_t sum,
                                      unsigned long long* __restrict__ out) {
  sums[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t width = kBlock / 2; width > 0; width >>= 1) {
    if (threadIdx.x < width) sums[threadIdx.x] += sums[threadIdx.x + width];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = sums[0];
}

// A bf16 GEMM whose operands travel global memory -> LDS -> MFMA: C (S x S,
// f32 accumulators, never stored) = A (S x K) . B^T, B stored S x K, K =
// 64 x steps, S = 128 x side. The grid is tiles x passes workgroups, tiles =
// side^2; workgroup g computes tile gemm_order(g % tiles) of pass g / tiles,
// every pass the same product.
//
// Work split. A workgroup owns a 128 x 128 tile of C; its four waves sit 2 x
// 2 (wave j: rows 64 (j >> 1), columns 64 (j & 1)) and each owns 64 x 64 as
// an MfmaTile, with the fragment rule of MfmaFrags<kBf16>: lane r + 32 h of
// fragment t holds row (A) or column (B) 32 t + r at k = 8 h .. 8 h + 7, one
// 16-byte chunk. One step (64 k) is four sub-steps of four MFMAs; sub-step s
// uses chunk 2 s + h.
//
// Data movement. Per step the workgroup moves a 128 x 64 slab of A and one of
// B, 16 KiB each, into LDS: lane t loads chunk t & 7 of rows (t >> 3) + 32 i,
// i = 0..3, of either slab, so eight lanes read the 128 contiguous bytes of a
// row and a lane has eight 16-byte loads in flight. LDS holds two buffers of
// {A slab, B slab}, 64 KiB, and 2 KiB for the reduction at the end: two
// workgroups fit a CU's 160 KiB.
//
// LDS layout (gemm_slot): row-major, 128 bytes a row, no padding; chunk c of
// row R is stored at chunk position c ^ q(R), q(R) = (R & 6) | ((R >> 3) & 1).
// The 64 banks are 256 bytes, that is two rows, so a 16-byte access falls
// into bank group (R & 1) * 8 + (c ^ q(R)) of 16, and 16 lanes are served at a
// time. A fragment read has lane r on row base + r (base a multiple of 32) at
// one c per h: over 16 consecutive r, (r & 1, q(r)) takes all 16 values, so
// the 16 lanes fall into 16 different bank groups; and should the hardware
// pair eight lanes of h = 0 with eight of h = 1 instead, their chunks c and c
// ^ 1 meet keys q(0..7) = {0, 2, 4, 6} and stay apart too. A slab write has
// 16 consecutive lanes on rows R, R + 1 (R even) and all eight c: whatever q,
// each row's eight lanes fill its eight positions. So neither ds_read_b128
// nor ds_write_b128 has a bank conflict. (With plain 128-byte rows every
// lane of a fragment read would fall into one of two bank groups.)
//
// Pipeline. The slab of step i + 1 is loaded from global memory into
// registers before the MFMAs of step i are issued and written to the other
// LDS buffer after them; one workgroup barrier ends the step. That barrier
// is enough: the buffer written in step i was last read in step i - 1, which
// every wave left through the barrier before. Within a step the fragment
// reads of sub-step s + 1 go in front of the first three MFMAs of sub-step s
// (gemm_multiply: mfma_lds_interleave, two reads per 32 cycles of MFMA) into
// a second register set; only sub-step 0's reads, which have to follow the barrier,
// are not covered by the wave's own MFMAs, and there the CU's other waves
// issue theirs. The last step loads and writes nothing.
//
// Bounds. S and K are multiples of the tile and of the step by construction,
// so nothing is masked. A global index is (128 tile + row) * K/8 + 8 step +
// chunk with tile < side, row < 128, step < steps and chunk < 8, below S *
// K/8, the 16-byte elements of one matrix. An LDS index is gemm_slot of a row
// below 128 and a chunk below 8, below the slab's 1024.
//
// Exactness. Operands are integers of magnitude <= 15, so a product's sum
// over K <= 32768 stays below 32768 * 225 < 2^23: every accumulator is an
// exact integer in f32 at every step.
//
// Result. Every lane converts its 64 accumulators to integers and weighs the
// entry at (m, n), global, by (1 + m) (1 + n) modulo 2^64; the 256 sums are
// added up through LDS and thread 0 stores the workgroup's one word out[g]
// (gemm_tile_sum, gemm_store_sum).
// Stamps and clocks are the mfma kind's (clocked_end). The addresses of the
// first slab are computed before the start stamp, its loads are inside it;
// between the stamps nothing but the operand loads and that one store
// touches global memory.
//
// No FP32 arithmetic but the MFMAs' is written here or in the fill, so the
// compiler has nothing to pack into two-wide FP32 instructions.
//
// hipcc -O3 for gfx950 reports (-Rpass-analysis=kernel-resource-usage) 158
// VGPRs, no AGPRs, 32 SGPRs, no scratch and no spills, 67584 bytes of LDS and
// an occupancy of 2 waves per SIMD: two workgroups per CU by registers and
// by LDS alike.
__global__ void __launch_bounds__(kBlock, 2)
tenant_gemm_kernel(const int4v* __restrict__ a, const int4v* __restrict__ b, uint32_t side,
                   uint32_t steps, unsigned long long* __restrict__ out,
                   unsigned long long* __restrict__ rec,
                   unsigned long long* __restrict__ clk) {
  __shared__ int4v slab[2][2][kGemmSlabVecs];  // [buffer][A, B]
  __shared__ unsigned long long sums[kBlock];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = lane & 31u, h = lane >> 5;
  const uint32_t wave = threadIdx.x / 64;
  const uint32_t tiles = side * side;
  const uint32_t tile = gemm_order(blockIdx.x % tiles, tiles, side);
  const uint32_t row0 = (tile >> 16) * kGemmTile, col0 = (tile & 0xFFFFu) * kGemmTile;
  // What this lane loads: chunk threadIdx & 7 of rows (threadIdx >> 3) + 32 i.
  const uint64_t k8 = static_cast<uint64_t>(steps) * kGemmRowVecs;
  const uint32_t load_row = threadIdx.x >> 3, load_c = threadIdx.x & 7u;
  const int4v* pa = a + (row0 + load_row) * k8 + load_c;
  const int4v* pb = b + (col0 + load_row) * k8 + load_c;
  const uint64_t load_stride = 32 * k8;                   // 32 rows on
  const uint32_t write_at = gemm_slot(load_row, load_c);  // + 32 rows: + 256
  // What this lane reads: rows 64 x (wave's half) + 32 t + r of either slab,
  // at sub-step s the chunk 2 s + h; 32 t and 64 leave the row's key alone.
  const uint32_t read_a = (64 * (wave >> 1) + r) * kGemmRowVecs;
  const uint32_t read_b = (64 * (wave & 1u) + r) * kGemmRowVecs;
  const uint32_t read_key = gemm_key(r);

  int4v next[2][kGemmLoads];
  const auto fetch = [&] {
#pragma unroll
    for (int i = 0; i < kGemmLoads; ++i) {
      next[0][i] = pa[i * load_stride];
      next[1][i] = pb[i * load_stride];
    }
    pa += kGemmRowVecs;
    pb += kGemmRowVecs;
  };
  const auto store = [&](int4v (*to)[kGemmSlabVecs]) {
#pragma unroll
    for (int i = 0; i < kGemmLoads; ++i) {
      to[0][write_at + 32 * kGemmRowVecs * i] = next[0][i];
      to[1][write_at + 32 * kGemmRowVecs * i] = next[1][i];
    }
  };
  f32x16 acc[2][2];

  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  const unsigned long long t0 = stamp_start();
  mfma_zero(acc);
  fetch();
  store(slab[0]);
  __syncthreads();
  for (uint32_t i = 0; i + 1 < steps; ++i) {
    fetch();  // step i + 1, in flight under the MFMAs of step i
    gemm_multiply(acc, slab[i & 1u], read_a, read_b, read_key, h);
    store(slab[(i + 1) & 1u]);
    __syncthreads();
  }
  gemm_multiply(acc, slab[(steps - 1) & 1u], read_a, read_b, read_key, h);
  gemm_store_sum(sums, gemm_tile_sum(acc, row0, col0, wave, r, h), out);
  clocked_end(rec, clk, c0, t0);
}

// ---- gemm-mxfp8, gemm-mxfp4 ------------------------------------------------

using int2v = __attribute__((ext_vector_type(2))) int;

// What the two block-scaled GEMMs differ in. A slab row is 128 bytes in
// either form, as in the bf16 kernel: 128 k of e4m3 or 256 k of e2m1, that is
// two or four sub-steps of 64 k (one MFMA deep) and four or eight blocks of
// 32 k, each with its own E8M0 scale byte. A row's scale bytes of one step
// are one word of 4 or 8 bytes, block b in byte b. K stays exact up to
// kMaxIters steps (see the kernel). agent/cotenancy.py keeps the same table.
template <int F>
struct MxGemm {
  static_assert(F == kMxfp8 || F == kMxfp4, "a block-scaled form");
  static constexpr int kSub = F == kMxfp8 ? 2 : 4;
  static constexpr int kStepK = 64 * kSub;
  static constexpr int kWordBytes = 2 * kSub;
  static constexpr int kWordDwords = kWordBytes / 4;
  static constexpr int kMaxIters = F == kMxfp8 ? 256 : 64;  // K <= 32768, 16384
  static constexpr int kDefaultIters = 4096 / kStepK;
  // 16-byte LDS reads per sub-step, and how many of them go in front of one
  // MFMA: two per 32 cycles of MFMA, and the mxfp8 MFMA takes 64.
  static constexpr int kReads = F == kMxfp8 ? 8 : 4;
  static constexpr int kReadsPerGap = F == kMxfp8 ? 4 : 2;
  using Word = typename std::conditional<F == kMxfp8, int, int2v>::type;
  __device__ static uint32_t dword(Word w, int d) {
    if constexpr (F == kMxfp8) return static_cast<uint32_t>(w);
    else return static_cast<uint32_t>(w[d]);
  }
};
constexpr int kMxGemmDefaultSide = 8192;
constexpr int kMxGemmDefaultPasses[kMfmaForms] = {0, 0, 32, 64};

// Which 16-byte chunk (0..7) of a row's 128-byte step lane half h holds in
// piece p (0..3) of its registers; see tenant_decode_kernel.
template <int F>
__device__ constexpr uint32_t decode_chunk(uint32_t p, uint32_t h) {
  return F == kMxfp8 ? 2 * p + h : 4 * h + p;
}

// The operands of a block-scaled gemm or decode tenant. `buf` is A (rows_a x
// K, row-major) followed by B (rows_b x K, row n holding column n), S and S
// rows for the gemm kinds, 32 and N for decode (whose B is W); e4m3 bytes or
// e2m1 nibbles, low nibble first: element (row, k) is that of MfmaFrags<F> at
// mfma_a_hash<F>(key, row % 192, k % 96) or mfma_b_hash<F>(key, k % 96, row %
// 192), mxfp8 hash % 15 - 7 and mxfp4 the code hash & 15. One 16-byte store of
// 16 or 32 elements per step, grid-stride; v16 = 8 x steps counts the stores
// of a row and n16 = (rows_a + rows_b) v16 those of both matrices. 96 is a
// multiple of 16 and of 32, so a store never straddles the k period.
//
// `scales` is step-major: A's words [steps][rows_a], then B's [steps][rows_b],
// one word per row and step, byte b the scale of the step's block b, that is
// of block ((k % 96) / 32) of the hashes with k = kStepK x step + 32 b: mxfp8
// 127 + e on both sides, mxfp4 128 + e for A and 128 for B, e the form's scale
// bit. So the 32 rows of a fragment are 128 or 256 contiguous bytes. nwords =
// (rows_a + rows_b) x steps. All indices are 64-bit, below n16 and below
// nwords.
//
// kTiled (decode's weights = "tiled", rows_b a multiple of 32) stores B's
// 16-byte chunks in the order tenant_decode_kernel's waves consume them and
// leaves A and the scale words as they are. The unit is a row block of 32
// rows x one step, 256 chunks, 4 KiB; units go row-block-major, then by step;
// inside a unit chunk [piece p][lane l = r + 32 h] is chunk decode_chunk<F>(p,
// h) of the step of row 32 block + r. Store index j = i - rows_a v16 of B is
// unit j / 256 = block x steps + step, p = (j % 256) / 64 and l = j % 64; it is
// mapped back to its row and its chunk 8 step + decode_chunk of the row before
// hashing, a bijection of B's rows_b v16 indices, so that the same elements
// are stored, one store per index, each below n16.
template <int F, bool kTiled = false>
__global__ void __launch_bounds__(kBlock)
tenant_mxgemm_fill_kernel(int4v* __restrict__ buf, uint64_t n16, uint64_t v16,
                          typename MxGemm<F>::Word* __restrict__ scales, uint64_t nwords,
                          uint64_t rows_a, uint64_t rows_b, uint32_t key) {
  using G = MxGemm<F>;
  constexpr uint32_t kPerDword = F == kMxfp8 ? 4 : 8;  // elements of one dword
  const uint64_t first = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
  for (uint64_t i = first; i < n16; i += stride) {
    uint64_t at = i;  // the row-major index of the chunk that store i holds
    if constexpr (kTiled) {
      if (i >= rows_a * v16) {
        const uint64_t j = i - rows_a * v16, unit = j / 256, steps = v16 / kGemmRowVecs;
        const uint32_t p = static_cast<uint32_t>(j % 256) / 64, l = static_cast<uint32_t>(j % 64);
        at = (rows_a + 32 * (unit / steps) + (l & 31u)) * v16 + kGemmRowVecs * (unit % steps) +
             decode_chunk<F>(p, l >> 5);
      }
    }
    const uint64_t line = at / v16;
    const bool is_b = line >= rows_a;
    const uint32_t row = static_cast<uint32_t>((is_b ? line - rows_a : line) % kGemmRowPeriod);
    const uint32_t k0 = static_cast<uint32_t>((at % v16) * (4 * kPerDword) % kGemmKPeriod);
    int4v v;
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) {
      uint32_t word = 0;
#pragma unroll
      for (uint32_t q = 0; q < kPerDword; ++q) {
        const uint32_t k = k0 + kPerDword * d + q;
        const uint32_t hash = is_b ? mfma_b_hash<F>(key, k, row) : mfma_a_hash<F>(key, row, k);
        if constexpr (F == kMxfp8)
          word |= to_e4m3_bits(static_cast<int>(hash % 15u) - 7) << (8 * q);
        else
          word |= (hash & 15u) << (4 * q);
      }
      v[d] = static_cast<int>(word);
    }
    buf[i] = v;
  }
  const uint64_t a_words = nwords / (rows_a + rows_b) * rows_a;  // steps x rows_a
  for (uint64_t i = first; i < nwords; i += stride) {
    const bool is_b = i >= a_words;
    const uint64_t rows = is_b ? rows_b : rows_a, at = is_b ? i - a_words : i;
    const uint32_t row = static_cast<uint32_t>((at % rows) % kGemmRowPeriod);
    const uint32_t blk0 = static_cast<uint32_t>((at / rows) * G::kWordBytes % 3);
    uint32_t word[2] = {0, 0};
#pragma unroll
    for (uint32_t b = 0; b < G::kWordBytes; ++b) {
      const uint32_t blk = (blk0 + b) % 3;
      uint32_t byte;
      if constexpr (F == kMxfp8)
        byte = 127u + (is_b ? mfma_b_scale_bit<F>(key, blk, row)
                            : mfma_a_scale_bit<F>(key, row, blk));
      else
        byte = 128u + (is_b ? 0u : mfma_a_scale_bit<F>(key, row, blk));
      word[b / 4] |= byte << (8 * (b % 4));
    }
    if constexpr (F == kMxfp8)
      scales[i] = static_cast<int>(word[0]);
    else
      scales[i] = int2v{static_cast<int>(word[0]), static_cast<int>(word[1])};
  }
}

// Buffer loads (raw, no stride): the descriptor's last word for gfx9 (32-bit
// data format), and an offset no descriptor here reaches: every window is
// below 2^31 bytes (a matrix is at most 32768 x 32768 bytes, the scale words
// of one operand 32 MiB), whether or not the hardware counts the shared
// offset into its range check.
constexpr int kBufferWord3 = 0x00020000;
constexpr uint32_t kBufferOutside = 0x80000000u;

// The descriptor of the `bytes` bytes that start at `first`.
__device__ inline __amdgpu_buffer_rsrc_t buffer_window(const void* first, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(first), 0, static_cast<int>(bytes),
                                           kBufferWord3);
}

template <int F>
__device__ inline typename MxGemm<F>::Word mx_load_word(__amdgpu_buffer_rsrc_t window,
                                                        uint32_t lane_off, uint32_t shared_off) {
  if constexpr (F == kMxfp8)
    return static_cast<int>(__builtin_amdgcn_raw_buffer_load_b32(window, lane_off, shared_off, 0));
  else
    return __builtin_bit_cast(
        int2v, __builtin_amdgcn_raw_buffer_load_b64(window, lane_off, shared_off, 0));
}

// One step's loads of a lane, as they come from global memory: its eight
// chunks of the two slabs and the scale words of its four fragments' rows.
template <int F>
struct MxPrefetch {
  int4v slab[2][kGemmLoads];
  typename MxGemm<F>::Word sa[2], sb[2];
};

// The scale words of the step being multiplied, shifted right by 8 h: byte 0
// of dword d is the scale of block 4 d + h and byte 2 that of block 4 d + 2 +
// h, the two blocks lane r + 32 h supplies the scale of (see MfmaFrags).
template <int F>
struct MxScales {
  int a[2][MxGemm<F>::kWordDwords], b[2][MxGemm<F>::kWordDwords];
  __device__ void take(const MxPrefetch<F>& p, uint32_t h) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int d = 0; d < MxGemm<F>::kWordDwords; ++d) {
        a[t][d] = static_cast<int>(MxGemm<F>::dword(p.sa[t], d) >> (8 * h));
        b[t][d] = static_cast<int>(MxGemm<F>::dword(p.sb[t], d) >> (8 * h));
      }
  }
};

// Sub-step S of a step: acc[m][n] += A_m x B_n over 64 k, the fragments under
// the scales of blocks 2 S + h. The lane's byte is byte 2 (S & 1) of dword S
// >> 1 of the shifted word, picked by the scale operands' op_sel: no VALU
// work per sub-step, and every checksum on the card came out exact with it
// (profiles/mxgemm_cotenancy_results.md). With GPUPROBE_MXGEMM_SHIFT_SCALES
// defined the byte is shifted down to byte 0 instead and op_sel stays 0; that
// build was not run.
template <int F, int S>
__device__ inline void mx_step(const MfmaFrags<F>& f, MfmaTile& acc, const MxScales<F>& sc) {
#ifdef GPUPROBE_MXGEMM_SHIFT_SCALES
  constexpr int kSel = 0, kShift = 16 * (S & 1);
#else
  constexpr int kSel = 2 * (S & 1), kShift = 0;
#endif
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int m = t >> 1, n = t & 1;
    const int sa = static_cast<int>(static_cast<uint32_t>(sc.a[m][S >> 1]) >> kShift);
    const int sb = static_cast<int>(static_cast<uint32_t>(sc.b[n][S >> 1]) >> kShift);
    if constexpr (F == kMxfp8)
      acc[m][n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(f.a[m], f.b[n], acc[m][n], 0,
                                                                  0, kSel, sa, kSel, sb);
    else
      acc[m][n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
          MfmaFrags<F>::widen(f.a[m]), MfmaFrags<F>::widen(f.b[n]), acc[m][n], 4, 4, kSel, sa,
          kSel, sb);
  }
}

// A block-scaled GEMM, MXFP8 (e4m3) or MXFP4 (e2m1) elements under E8M0
// scales per block of 32 k, whose elements travel global memory -> LDS ->
// MFMA and whose scales travel global memory -> registers: C (S x S, f32
// accumulators, never stored) = A (S x K) . B^T, B stored S x K, K = 128
// (mxfp8) or 256 (mxfp4) x steps, S = 128 x side. Grid, tile walk
// (gemm_order), work split, slab geometry and result are tenant_gemm_kernel's;
// the pipeline and the scale path are this kernel's own.
//
// Work split. A workgroup owns a 128 x 128 tile of C, its four waves 2 x 2 on
// 64 x 64 each as an MfmaTile. A step is a slab row of 128 bytes, two (mxfp8)
// or four (mxfp4) sub-steps of four v_mfma_scale_f32_32x32x64_f8f6f4: per
// wave and step 8 MFMAs of 64 cycles or 16 of 32, 512 cycles as for bf16.
// The fragment rule is MfmaFrags<F>'s: lane r + 32 h of fragment t holds row
// or column 32 t + r; for mxfp4 its four dwords are block 2 s + h of sub-step
// s, one 16-byte chunk, 2 s + h, the bf16 kernel's addressing; for mxfp8 its
// low four dwords are half h of block 2 s, chunk 4 s + h, and its high four
// half h of block 2 s + 1, chunk 4 s + 2 + h, two reads per fragment.
//
// Data movement and LDS layout are the bf16 kernel's: lane t loads chunk t & 7
// of rows (t >> 3) + 32 i of either slab, eight 16-byte loads a step; two
// buffers of {A slab, B slab}, 64 KiB, and 2 KiB for the reduction; chunk c of
// row R at chunk position c ^ q(R), q(R) = (R & 6) | ((R >> 3) & 1)
// (gemm_slot). Its proof holds for these chunk indices: every fragment read
// is a ds_read_b128 with lane r on row base + r (base a multiple of 32) at one
// chunk per h, and the chunks of h = 0 and h = 1 are c and c ^ 1 here too (2
// s, 4 s and 4 s + 2 are even); over 16 consecutive r, (r & 1, q(r)) takes all
// 16 values, so 16 lanes of one h fall into 16 different groups of four
// banks, and eight lanes of each h, should the hardware pair them so, meet
// the keys q(0..7) = {0, 2, 4, 6} with c and c ^ 1 and stay apart as well.
// The slab writes are the bf16 kernel's own. No bank conflict either way.
//
// Pipeline: two slabs in flight. A dependent load from HBM takes 375-399 ns
// on an idle card (profiles/chase_cotenancy_results.md), about 900 cycles,
// and a step is 512 cycles of MFMA, so a prefetch distance of one step, the
// bf16 kernel's, cannot cover it. Here the global loads of step i + 2 are
// issued at the top of step i into register set i & 1 (the set's loads of
// step i were written to LDS a step before) and written to LDS buffer i & 1
// at the end of step i + 1; every wave left that buffer through the barrier
// that ended step i. Still two LDS buffers and one barrier per step. The
// prologue loads steps 0 and 1 and writes step 0; the loop runs two steps an
// iteration so that each register set is a fixed one; an odd last step
// follows the loop. The last two steps load nothing: their loads are issued
// all the same, but with every lane's offset outside the buffer descriptors'
// range, which the hardware answers with zeros without reading memory, and
// what they return is written to an LDS buffer nobody reads again (steps = 1
// and 2 included). So no load has a branch around it, and every wait in
// front of a slab write leaves exactly the newer step's twelve loads
// outstanding (vmcnt counts in order).
//
// Scales. The scale words of a step go global -> registers at the same
// distance and never touch LDS: every lane loads the word of each of its own
// four rows, A at t = 0, 1 and B at t = 0, 1, lanes r and r + 32 the same
// one, first in the step's loads so that they are there when its slabs are.
// The words are step-major (see the fill), so a fragment's 32 lanes read 128
// or 256 contiguous bytes. Once per step the words are shifted right by 8 h
// (MxScales); a sub-step picks its byte with op_sel (mx_step).
//
// Within a step the fragment reads of sub-step s + 1 go in front of the MFMAs
// of sub-step s into a second register set (mfma_lds_interleave), at most two
// 16-byte reads per 32 cycles of MFMA: 4 + 4 in front of the first two mxfp8
// MFMAs, 2 + 2 for mxfp4.
//
// Bounds. S and K are multiples of the tile and of the step, so nothing is
// masked. A global element index is (128 tile + row) * 8 steps + 8 step +
// chunk with tile < side, row < 128, step < steps and chunk < 8, below S * 8
// steps, the 16-byte elements of one matrix; every descriptor ends where its
// matrix or scale array does, and a load past the last step is outside it by
// construction (offset bit 31). A scale index is step * S + row with step < steps and
// row < S, below steps * S, one operand's words. An LDS index is gemm_slot of
// a row below 128 and a chunk below 8 (4 s + 2 + h <= 7, 2 s + h <= 7), below
// the slab's 1024.
//
// Exactness. Effective elements are integers. mxfp8: |a b| <= 14 * 14 and 196
// * 32768 < 2^23, so K <= 32768, 256 steps. mxfp4: |A| <= 24 and |B| <= 12,
// 288 * 16384 < 2^23 but 288 * 32768 > 2^23, so K <= 16384, 64 steps. Every
// accumulator is an exact integer in f32 at every step.
//
// Result, stamps and clocks are the bf16 kernel's (gemm_tile_sum,
// gemm_store_sum, clocked_end). No FP32 arithmetic but the MFMAs' is written
// here or in the fill.
//
// hipcc -O3 for gfx950 reports (-Rpass-analysis=kernel-resource-usage), mxfp8
// and mxfp4: 227 and 207 VGPRs (64 of accumulators, 64 and 32 of fragments,
// 64 of prefetched slabs, 12 and 24 of scale words), no AGPRs, 54 SGPRs, no
// scratch and no spills, 67584 bytes of LDS and an occupancy of 2 waves per
// SIMD: two workgroups per CU still fit, by registers (256 a wave) and by
// LDS alike. To get there no lane carries a 64-bit address (buffer loads)
// and the loop has one exit: with a second exit in its middle the compiler
// kept the accumulators twice and spilled.
//
// On the card (profiles/mxgemm_cotenancy_results.md) a SIMD spends 147-150
// cycles per mxfp8 MFMA and 84-87 per mxfp4 one, where the instructions take
// 64 and 32: per step and wave about 1190 and 1360 cycles against the bf16
// kernel's 1120. The second slab in flight did not bring the step nearer its
// 512 cycles of MFMA.
template <int F>
__global__ void __launch_bounds__(kBlock, 2)
tenant_mxgemm_kernel(const int4v* __restrict__ a, const int4v* __restrict__ b,
                     const typename MxGemm<F>::Word* __restrict__ sa,
                     const typename MxGemm<F>::Word* __restrict__ sb, uint32_t side,
                     uint32_t steps, unsigned long long* __restrict__ out,
                     unsigned long long* __restrict__ rec,
                     unsigned long long* __restrict__ clk) {
  using G = MxGemm<F>;
  using Slabs = int4v (*)[kGemmSlabVecs];
  __shared__ int4v slab[2][2][kGemmSlabVecs];  // [buffer][A, B]
  __shared__ unsigned long long sums[kBlock];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = lane & 31u, h = lane >> 5;
  const uint32_t wave = threadIdx.x / 64;
  const uint32_t tiles = side * side;
  const uint32_t tile = gemm_order(blockIdx.x % tiles, tiles, side);
  const uint32_t row0 = (tile >> 16) * kGemmTile, col0 = (tile & 0xFFFFu) * kGemmTile;
  // What this lane loads: chunk threadIdx & 7 of rows (threadIdx >> 3) + 32 i,
  // and the scale words of rows 64 x (wave's half) + 32 t + r, all as buffer
  // loads: a descriptor the workgroup shares (from the tile's first row to
  // the matrix's end, below 2^31 bytes), one 32-bit byte offset of the lane's
  // and one the workgroup shares, so that the addresses of a step's twelve
  // loads cost three vector registers and no load has a branch around it.
  const uint32_t row_bytes = steps * (kGemmRowVecs * 16);
  const uint32_t s_rows = side * kGemmTile;
  const uint32_t load_row = threadIdx.x >> 3, load_c = threadIdx.x & 7u;
  const uint32_t load_at = load_row * row_bytes + load_c * 16;
  const uint32_t write_at = gemm_slot(load_row, load_c);  // + 32 rows: + 256
  const uint32_t scale_a_at = (64 * (wave >> 1) + r) * G::kWordBytes;
  const uint32_t scale_b_at = (64 * (wave & 1u) + r) * G::kWordBytes;
  const auto ra = buffer_window(a + static_cast<uint64_t>(row0) * (row_bytes / 16),
                                (s_rows - row0) * row_bytes);
  const auto rb = buffer_window(b + static_cast<uint64_t>(col0) * (row_bytes / 16),
                                (s_rows - col0) * row_bytes);
  const auto rsa = buffer_window(sa + row0, (steps * s_rows - row0) * G::kWordBytes);
  const auto rsb = buffer_window(sb + col0, (steps * s_rows - col0) * G::kWordBytes);
  // What this lane reads: rows 64 x (wave's half) + 32 t + r of either slab;
  // 32 t and 64 leave the row's key alone.
  const uint32_t read_a = (64 * (wave >> 1) + r) * kGemmRowVecs;
  const uint32_t read_b = (64 * (wave & 1u) + r) * kGemmRowVecs;
  const uint32_t read_key = gemm_key(r);

  MxPrefetch<F> p0, p1;
  MxScales<F> cur;
  // The loads of step `at_step`; past the last step every lane's offset is
  // moved out of the descriptors' range, where a buffer load returns zeros
  // and reads no memory.
  const auto fetch = [&](MxPrefetch<F>& p, uint32_t at_step) __attribute__((always_inline)) {
    const uint32_t outside = at_step < steps ? 0u : kBufferOutside;
    const uint32_t word_off = at_step * s_rows * G::kWordBytes;
    const uint32_t slab_off = at_step * (kGemmRowVecs * 16);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      p.sa[t] = mx_load_word<F>(rsa, (scale_a_at | outside) + 32 * t * G::kWordBytes, word_off);
      p.sb[t] = mx_load_word<F>(rsb, (scale_b_at | outside) + 32 * t * G::kWordBytes, word_off);
    }
#pragma unroll
    for (int i = 0; i < kGemmLoads; ++i) {
      p.slab[0][i] = __builtin_bit_cast(int4v, __builtin_amdgcn_raw_buffer_load_b128(
          ra, load_at | outside, slab_off + 32 * i * row_bytes, 0));
      p.slab[1][i] = __builtin_bit_cast(int4v, __builtin_amdgcn_raw_buffer_load_b128(
          rb, load_at | outside, slab_off + 32 * i * row_bytes, 0));
    }
  };
  const auto store = [&](const MxPrefetch<F>& p, Slabs to) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < kGemmLoads; ++i) {
      to[0][write_at + 32 * kGemmRowVecs * i] = p.slab[0][i];
      to[1][write_at + 32 * kGemmRowVecs * i] = p.slab[1][i];
    }
  };
  const auto read = [&](MfmaFrags<F>& f, Slabs from, uint32_t s) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int4v* ra = from[0] + read_a + 32 * kGemmRowVecs * t;
      const int4v* rb = from[1] + read_b + 32 * kGemmRowVecs * t;
      if constexpr (F == kMxfp8) {
        const uint32_t lo = (4 * s + h) ^ read_key, hi = (4 * s + 2 + h) ^ read_key;
        const int4v al = ra[lo], ah = ra[hi], bl = rb[lo], bh = rb[hi];
        f.a[t] = int8v{al[0], al[1], al[2], al[3], ah[0], ah[1], ah[2], ah[3]};
        f.b[t] = int8v{bl[0], bl[1], bl[2], bl[3], bh[0], bh[1], bh[2], bh[3]};
      } else {
        const uint32_t c = (2 * s + h) ^ read_key;
        f.a[t] = ra[c];
        f.b[t] = rb[c];
      }
    }
  };
  f32x16 acc[2][2];
  // One step's MFMAs on the slabs of `from` under the scales of `cur`.
  const auto multiply = [&](Slabs from) __attribute__((always_inline)) {
    MfmaFrags<F> f[2];
    read(f[0], from, 0);
    __builtin_amdgcn_sched_barrier(0);
    read(f[1], from, 1);
    mx_step<F, 0>(f[0], acc, cur);
    mfma_lds_interleave<G::kReads, G::kReadsPerGap>();
    if constexpr (G::kSub == 4) {
      read(f[0], from, 2);
      mx_step<F, 1>(f[1], acc, cur);
      mfma_lds_interleave<G::kReads, G::kReadsPerGap>();
      read(f[1], from, 3);
      mx_step<F, 2>(f[0], acc, cur);
      mfma_lds_interleave<G::kReads, G::kReadsPerGap>();
      mx_step<F, 3>(f[1], acc, cur);
    } else {
      mx_step<F, 1>(f[1], acc, cur);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  // Step i on buffer i & 1 with the scales of `mine`, whose loads those of
  // step i + 2 replace; `next`, step i + 1, goes to the other buffer behind
  // the MFMAs.
  const auto step = [&](MxPrefetch<F>& mine, uint32_t i, const MxPrefetch<F>& next)
      __attribute__((always_inline)) {
    cur.take(mine, h);
    fetch(mine, i + 2);
    multiply(slab[i & 1u]);
    store(next, slab[(i + 1) & 1u]);
    __syncthreads();
  };

  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  const unsigned long long t0 = stamp_start();
  mfma_zero(acc);
  fetch(p0, 0);
  fetch(p1, 1);
  store(p0, slab[0]);
  __syncthreads();
  for (uint32_t i = 0; i + 1 < steps; i += 2) {
    step(p0, i, p1);
    step(p1, i + 1, p0);
  }
  if (steps & 1u) step(p0, steps - 1, p1);
  gemm_store_sum(sums, gemm_tile_sum(acc, row0, col0, wave, r, h), out);
  clocked_end(rec, clk, c0, t0);
}

// ---- gemm, loads straight to LDS ---------------------------------------------

// How many {A slab, B slab} pairs the ring of tenant_gemm_direct_kernel holds:
// 2 (64 KiB of slabs, two workgroups per CU) unless GPUPROBE_GEMM_DIRECT_STAGES
// is defined as 3 (96 KiB, one workgroup per CU), the depth the kept one was
// measured against (profiles/gemm_direct_cotenancy_results.md: on the whole
// card two pairs run 1.29-1.30 PFLOP/s at 47.7-47.9 cycles per MFMA and SIMD,
// three 1.03-1.04 at 75.3-76.0, beside 1.05-1.07 at 69.9-70.8 for the
// kernel that stages through registers, the same command repeated moving
// each by about 1 %. A second workgroup on the CU hides a barrier and the
// reads behind it; a deeper ring that costs that workgroup does not.)
#ifndef GPUPROBE_GEMM_DIRECT_STAGES
#define GPUPROBE_GEMM_DIRECT_STAGES 2
#endif
constexpr int kGemmDirectStages = GPUPROBE_GEMM_DIRECT_STAGES;
static_assert(kGemmDirectStages == 2 || kGemmDirectStages == 3, "a ring of two or three");

using LdsPtr = __attribute__((address_space(3))) void*;

// tenant_gemm_kernel's product from the same buffers with the slabs loaded
// global memory -> LDS without passing through registers (the 16-byte LDS-DMA
// load of gfx950, buffer_load_dwordx4 ... lds), as production GEMMs on this
// chip feed their LDS. Fill, grid, tile walk (gemm_order), work split, K-step,
// LDS layout as the reading side sees it (gemm_slot), the fragment reads
// (gemm_multiply), exactness, result, stamps and clocks are
// tenant_gemm_kernel's; what follows is this kernel's own.
//
// Where the swizzle lives. An LDS-DMA load writes lane l's 16 bytes to (a
// wave-uniform base, in m0) + 16 l: one wave instruction fills 64 consecutive
// chunk positions, eight whole slab rows, and no lane chooses where its data
// lands. The readers still find chunk c of row R at position c ^ q(R)
// (gemm_slot, so its bank argument for ds_read_b128 holds unchanged); hence
// the lane that lands on position p of row R fetches chunk p ^ q(R) of that
// row from memory. Wave w's instruction i (0..3) fills rows 32 i + 8 w .. + 7
// of a slab, lane l on row R = 32 i + 8 w + (l >> 3) at position l & 7. q(R) =
// (R & 6) | ((R >> 3) & 1) = ((l >> 3) & 6) | (w & 1): 32 i and 8 w leave bits
// 1 and 2 alone, and bit 3 of R is bit 0 of w, as l >> 3 < 8 carries nothing
// into it. The key does not depend on i, so a lane's offset into the matrix
// is computed once, before the start stamp. Eight lanes still read one row's
// 128 contiguous bytes of the step, permuted. Four loads per lane, operand
// and step, eight in all; no ds_write, and no registers hold a slab.
//
// Ring and wait. LDS holds D = kGemmDirectStages pairs {A slab, B slab}. Step
// i issues the loads of step i + D - 1 into pair (i + D - 1) % D, multiplies
// from pair i % D, waits for s_waitcnt vmcnt(8 (D - 2)) and crosses one
// barrier. Nothing makes a wave wait for what the other waves loaded but
// this count: loads retire in issue order, a lane has issued eight per step,
// so with at most 8 (D - 2) outstanding everything up to the loads of step i
// + 1 has landed, and behind the barrier that holds for every wave. With D =
// 3 the loads of step i + 2 stay in flight across the barrier, which a
// kernel that stages through registers cannot express: its ds_write needs
// the data. The pair overwritten in step i, (i - 1) % D, was last read in
// step i - 1, and every wave left that step through its barrier after its
// MFMAs had consumed what it read. The prologue issues steps 0 .. D - 2 and
// waits with the same count: of its 8 (D - 1) loads the first eight, step
// 0's, have landed. Every step, the last D - 1 included, issues its eight
// loads (see Bounds), so the count means the same in every step; behind the
// loop vmcnt(0) lets nothing land after the reduction has begun.
//
// Bounds. Buffer loads on a descriptor that covers exactly the tile's 128
// rows of the operand, at most 128 x 65536 bytes: a lane's offset is (8 w +
// (l >> 3)) x row bytes + 16 x chunk, the shared one 32 i x row bytes + 128 x
// step, together row x row bytes + 128 step + 16 chunk with row < 128, step <
// steps, chunk < 8, so the 16 bytes end at or before the window's end, which
// is inside the matrix. Chosen over a branch around the loads because the
// wait count then never changes: a load of a step past the last (steps < D -
// 1 in the prologue, the last D - 1 steps of the loop) is issued with bit 31
// set in every lane's offset, outside any window, which the hardware answers
// without reading memory; what it leaves in LDS lies in a pair nobody reads
// again. No load and no barrier has a branch around it but the loop's own,
// whose count is the workgroup's. The LDS address handed to a load is
// computed from the wave's number, made a scalar with readfirstlane, and
// constants: wave-uniform by construction. An LDS address is pair x 32 KiB +
// operand x 16 KiB + (32 i + 8 w) x 128 + 16 l + 15 < D x 32 KiB.
//
// The loads are written as assembly, not as the compiler's
// raw_ptr_buffer_load_lds builtin: behind the builtin the compiler puts
// s_waitcnt vmcnt(0) in front of the first LDS read that follows and in front
// of the barrier, which takes the loads out of flight at once; the assembly
// it knows only as something that touches memory, and the counted wait above
// is the only one.
//
// No FP32 arithmetic but the MFMAs' is written here.
//
// hipcc -O3 for gfx950 reports (-Rpass-analysis=kernel-resource-usage), D = 2
// and D = 3: 170 VGPRs and no AGPRs, 168 VGPRs and 64 AGPRs (the
// accumulators), 42 SGPRs, no scratch and no spills, 67584 and 100352 bytes
// of LDS and an occupancy of 2 and 1 waves per SIMD, by LDS in either case.
// tenant_gemm_kernel and both tenant_mxgemm_kernels report what they did
// before this kernel was added.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"  // m0 is clobbered on purpose
template <int D>
__global__ void __launch_bounds__(kBlock, D == 2 ? 2 : 1)
tenant_gemm_direct_kernel(const int4v* __restrict__ a, const int4v* __restrict__ b,
                          uint32_t side, uint32_t steps, unsigned long long* __restrict__ out,
                          unsigned long long* __restrict__ rec,
                          unsigned long long* __restrict__ clk) {
  __shared__ int4v slab[D][2][kGemmSlabVecs];  // [pair][A, B]
  __shared__ unsigned long long sums[kBlock];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = lane & 31u, h = lane >> 5;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const uint32_t tiles = side * side;
  const uint32_t tile = gemm_order(blockIdx.x % tiles, tiles, side);
  const uint32_t row0 = (tile >> 16) * kGemmTile, col0 = (tile & 0xFFFFu) * kGemmTile;
  // What this lane loads: of rows 8 wave + (lane >> 3) + 32 i the chunk that
  // belongs at position lane & 7.
  const uint32_t row_bytes = steps * (kGemmRowVecs * 16);
  const uint32_t load_key = ((lane >> 3) & 6u) | (wave & 1u);
  const uint32_t load_at = (8 * wave + (lane >> 3)) * row_bytes + 16 * ((lane & 7u) ^ load_key);
  const uint32_t land_at = 8 * wave * kGemmRowVecs;  // + 32 rows: + 256
  // The descriptor's four words, written out because an asm operand takes
  // them as a vector: base, base's high 16 bits with stride 0, bytes, word 3.
  const auto window = [&](const int4v* first) {
    const uint64_t base = reinterpret_cast<uint64_t>(first);
    return int4v{static_cast<int>(static_cast<uint32_t>(base)),
                 static_cast<int>(static_cast<uint32_t>(base >> 32) & 0xFFFFu),
                 static_cast<int>(kGemmTile * row_bytes), kBufferWord3};
  };
  const auto ra = window(a + static_cast<uint64_t>(row0) * (row_bytes / 16));
  const auto rb = window(b + static_cast<uint64_t>(col0) * (row_bytes / 16));
  const uint32_t read_a = (64 * (wave >> 1) + r) * kGemmRowVecs;
  const uint32_t read_b = (64 * (wave & 1u) + r) * kGemmRowVecs;
  const uint32_t read_key = gemm_key(r);

  // One load: m0 = the LDS address of the wave's 1 KiB, a wait state that a
  // write of m0 needs before an LDS-DMA load reads it, the load.
  const auto load = [](int4v rsrc, const int4v* lds, uint32_t lane_off, uint32_t shared_off)
      __attribute__((always_inline)) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                 :
                 : "s"(static_cast<uint32_t>(reinterpret_cast<uintptr_t>((LdsPtr)lds))),
                   "v"(lane_off), "s"(rsrc), "s"(shared_off)
                 : "memory", "m0");
  };
  // The eight loads of step `at_step` into the pair `to`.
  const auto issue = [&](const int4v (*to)[kGemmSlabVecs], uint32_t at_step)
      __attribute__((always_inline)) {
    const uint32_t at = load_at | (at_step < steps ? 0u : kBufferOutside);
    const uint32_t slab_off = at_step * (kGemmRowVecs * 16);
#pragma unroll
    for (int i = 0; i < kGemmLoads; ++i) {
      load(ra, to[0] + land_at + 32 * kGemmRowVecs * i, at, slab_off + 32 * i * row_bytes);
      load(rb, to[1] + land_at + 32 * kGemmRowVecs * i, at, slab_off + 32 * i * row_bytes);
    }
  };
  // At most 8 (D - 2) of this wave's loads still outstanding, then the barrier.
  const auto landed = [] {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * kGemmLoads * (D - 2)) : "memory");
    __syncthreads();
  };
  f32x16 acc[2][2];

  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  const unsigned long long t0 = stamp_start();
  mfma_zero(acc);
  for (uint32_t i = 0; i + 1 < D; ++i) issue(slab[i], i);
  landed();
  uint32_t from = 0, to = D - 1;  // i % D and (i + D - 1) % D
  for (uint32_t i = 0; i < steps; ++i) {
    issue(slab[to], i + D - 1);
    gemm_multiply(acc, slab[from], read_a, read_b, read_key, h);
    landed();
    to = from;
    from = from + 1 == D ? 0 : from + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  gemm_store_sum(sums, gemm_tile_sum(acc, row0, col0, wave, r, h), out);
  clocked_end(rec, clk, c0, t0);
}
#pragma clang diagnostic pop

// ---- decode-mxfp8, decode-mxfp4 ----------------------------------------------

constexpr int kDecodeRows = 32;       // rows of A: the tokens of one decode step
constexpr int kDecodeDefaultK = 8192;
constexpr uint64_t kDecodeMaxN = 1 << 20;
// Tiled weights: a wave's 32 rows x one step of 128 bytes, stored together.
constexpr uint32_t kDecodeUnitBytes = 32 * kGemmRowVecs * 16;
// A default launch lasts about as long as the gemm kinds' default launches
// (profiles/decode_cotenancy_results.md).
constexpr int kDecodeDefaultPasses[kMfmaForms] = {0, 0, 48, 48};
// Steps of loads a wave keeps in flight, and the workgroups per CU (waves per
// SIMD) the kernel is built for at least: 2 and 5, measured against 3 steps
// at 4 waves, 4 at 3 and 8 at 2 (profiles/decode_cotenancy_results.md: all
// four within 1 % of each other for mxfp8, the kept one ahead; for mxfp4
// eight steps at two waves 1.5 % ahead of the other three).
#ifndef GPUPROBE_DECODE_DISTANCE
#define GPUPROBE_DECODE_DISTANCE 2
#endif
#ifndef GPUPROBE_DECODE_WAVES
#define GPUPROBE_DECODE_WAVES 5
#endif
constexpr int kDecodeDistance = GPUPROBE_DECODE_DISTANCE;
constexpr int kDecodeWaves = GPUPROBE_DECODE_WAVES;
// A distance of 1 is not built: its mxfp4 launch under a half-card mask did
// not end within two minutes on the card, cause not found
// (profiles/decode_cotenancy_results.md).
static_assert(kDecodeDistance >= 2 && kDecodeDistance <= 8, "register sets of a wave");
static_assert(kDecodeWaves >= 1 && kDecodeWaves <= 8, "waves per SIMD");

// One step's loads of a lane, as they come from global memory: the scale
// words of its weight row and of its row of A, its chunk of A's slab and the
// four pieces of its weight row.
template <int F>
struct DecodeFetch {
  typename MxGemm<F>::Word sw, sa;
  int4v a, w[4];
};

// Sub-step S of a decode step: acc += A x W^T over 64 k, one MFMA. `a` and
// `w` are the lane's four pieces of the step, `sa` and `sw` its scale
// registers for the sub-step, the byte picked by op_sel `kSel` (mx_step's 0
// and 2, the two values every checksum on the card was exact with).
template <int F, int S, int kSel>
__device__ inline f32x16 decode_mfma(const int4v (&a)[4], const int4v (&w)[4], f32x16 acc,
                                     int sa, int sw) {
  if constexpr (F == kMxfp8) {
    const int4v al = a[2 * S], ah = a[2 * S + 1], wl = w[2 * S], wh = w[2 * S + 1];
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
        int8v{al[0], al[1], al[2], al[3], ah[0], ah[1], ah[2], ah[3]},
        int8v{wl[0], wl[1], wl[2], wl[3], wh[0], wh[1], wh[2], wh[3]}, acc, 0, 0, kSel, sa, kSel,
        sw);
  } else {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
        MfmaFrags<F>::widen(a[S]), MfmaFrags<F>::widen(w[S]), acc, 4, 4, kSel, sa, kSel, sw);
  }
}

// The decode shape of a block-scaled GEMM: a few token rows against a weight
// matrix that is read once, C (32 x N, f32 accumulators, never stored) = A
// (32 x K) . W^T, W stored N x K, MXFP8 or MXFP4 under E8M0 scales per block
// of 32 k, K = 128 (mxfp8) or 256 (mxfp4) x steps, N = 128 x tiles. Every
// byte of W is used for 32 rows of C and never again, so the kernel streams
// W from memory at about 64 (mxfp8) or 128 (mxfp4) flop per byte and HBM,
// not the MFMA pipe, sets its pace. The grid is tiles x passes workgroups;
// workgroup g computes tile g % tiles of pass g / tiles, every pass the same
// product and a whole re-read of W.
//
// Work split. A workgroup owns 128 rows of W (128 columns of C) over the
// whole K; wave j owns rows 32 j .. 32 j + 31 and one 32 x 32 accumulator,
// output register reg row (reg & 3) + 8 (reg >> 2) + 4 h of column r as in
// every kernel here. A is the MFMA's first operand and W its second. A step
// is 128 bytes of every row, two (mxfp8) or four (mxfp4) sub-steps of one
// v_mfma_scale_f32_32x32x64_f8f6f4: per wave and step 4 KiB of W and 128
// cycles of MFMA.
//
// Which k a lane holds (decode_chunk). The step's 128 bytes are eight 16-byte
// chunks, and a lane keeps four of them, pieces p = 0..3, of its row. Any
// assignment is correct that A's fragments and both scale selections share.
//   mxfp4: a chunk is a block of 32 k and sub-step s multiplies piece s.
//     Lane half h holds chunks 4 h + s: the 64 contiguous bytes 64 h .. 64 h
//     + 63 of its row's step, four buffer_load_dwordx4 at consecutive
//     immediate offsets (the prefill kernels' 2 s + h gave a lane four pieces
//     32 bytes apart). One load instruction touches 16 bytes at 64 h + 16 s of
//     each of the wave's 32 rows, and the four of a step together every byte
//     of 32 lines of 128 bytes.
//   mxfp8: a block is two chunks, and the instruction scales a lane's low
//     four dwords by the scale register of lane r and its high four by that
//     of lane r + 32 (MfmaFrags), so the low dwords of lanes r and r + 32
//     have to be the two halves of one block and a lane cannot hold 32
//     contiguous bytes. Sub-step s multiplies pieces 2 s (low) and 2 s + 1
//     (high); piece p of lane half h is chunk 2 p + h, half h of block p.
//     One load instruction touches the 32 contiguous bytes of block p of
//     each of the 32 rows.
//
// Weights: global memory -> registers, in fragment layout, no LDS and no
// ds_write, because no other wave ever needs them. Buffer loads on a
// descriptor of exactly the tile's 128 rows (at most 128 x 32768 bytes); the
// lane's offset is (32 j + r) x row bytes + 16 x chunk(0, h), the piece an
// immediate, the step (128 x step) the shared offset.
//
// Weights, kTiled (weights = "tiled"): the same elements, W's 16-byte chunks
// stored once in the order the waves consume them (the fill, kTiled): a unit
// is a wave's 32 rows x one step, 4 KiB (kDecodeUnitBytes), units
// row-block-major and then by step, and inside a unit [piece p][lane r + 32
// h] is chunk decode_chunk<F>(p, h) of row 32 block + r, what that lane holds
// as piece p either way. The same loads into the same registers on the same
// descriptor (a tile's 128 rows are still one contiguous piece of 128 x row
// bytes), at other offsets: the lane's is wave x steps x 4 KiB + 16 x lane,
// the piece an immediate of 1 KiB x p, the step (4 KiB x step) the shared
// offset. One wave instruction reads 1 KiB of consecutive addresses, 8 whole
// lines, where row-major W has it touch 32 lines, and a wave's whole K is
// one run of steps x 4 KiB. A, the scale words, the pipeline, the waits and
// the result are the same code.
//
// Scales: global memory -> registers as in tenant_mxgemm_kernel, one word per
// lane, step and operand (lanes r and r + 32 the same one), step-major so
// that a wave's 32 rows are 128 or 256 contiguous bytes. The lane supplies
// the scale of its own half's block: mxfp8 block 2 s + h, byte 2 s of the word
// shifted right by 8 h, op_sel 2 s; mxfp4 block 4 h + s, byte s of dword h,
// which sub-steps 0 and 2 pick with op_sel 0 and 2 and sub-steps 1 and 3 with
// the same two from the dword shifted right by 8: one or two shifts per step
// and operand, and no op_sel value the card has not been seen exact with.
//
// Activations: global memory -> registers -> LDS, shared by the four waves.
// A step's slab of A is 32 rows x 128 bytes, 4 KiB: one 16-byte load and one
// ds_write_b128 per lane. LDS holds it in fragment order, plane p = the 64
// lanes' piece p at 16 x lane: wave p loads and writes plane p (lane r + 32 h
// fetches chunk(p, h) of row r), and every wave reads its four pieces as
// plane base + 16 x lane. Writes and reads alike are 64 lanes on 1 KiB of
// consecutive addresses, so neither has a bank conflict and nothing is
// swizzled. Two buffers of 4 KiB and 2 KiB for the reduction: 10 KiB. A is
// not kept resident: at the forms' largest K it is 1 MiB (mxfp8) or 256 KiB
// (mxfp4). It is re-read by every workgroup, 32 rows against the tile's 128,
// and is served by the L2 after its first use.
//
// Pipeline: D = kDecodeDistance steps in flight per wave. A step is only 4
// KiB per wave and 128 cycles of MFMA, and a dependent load from HBM takes
// about 900 cycles on an idle card (profiles/chase_cotenancy_results.md), so
// one step ahead covers nothing. Register set u = i % D holds the loads of
// step i: seven loads, always in the order slab chunk, W's scale word, A's
// scale word, weight pieces 0..3. Step i reads A's fragments from LDS buffer
// i & 1, takes its scales, issues the first three loads of step i + D into
// the same set, then its MFMAs, each followed by the loads that replace the
// pieces it has just read; it writes the slab of step i + 1 (set (u + 1) % D,
// loaded D - 1 steps ago) to buffer (i + 1) & 1 and crosses one barrier.
// Scheduling barriers (pin) keep the compiler from moving a load or the
// next step's scale selection, so prologue and steps issue in one order.
// That buffer
// was last read in step i - 1, which every wave left through the barrier
// before. The loop is unrolled D times so that every set is a fixed one, and
// runs ceil(steps / D) x D steps: a step past the last loads nothing (every
// lane's offset is moved outside the descriptors, kBufferOutside, which the
// hardware answers with zeros without reading memory), so its elements and
// scale bytes are zero, its products are +0 and the accumulators stay as
// they are. Hence no load and no barrier has a branch around it but the
// loop's own, every step issues the same seven loads in the same order, and
// every counted vmcnt the compiler places means the same in every step. In
// the gfx950 assembly of D = 2 every step waits vmcnt(11) for its scale
// words, vmcnt(12) (mxfp8) or vmcnt(13) (mxfp4) in front of each MFMA and
// vmcnt(13) in front of the slab write: each leaves the whole newer set
// outstanding, and the loop holds no vmcnt(0); at D = 4 the counts are 25,
// 26 or 27 and 27. With D x 4 KiB per wave and 4 x 5 waves a CU has 160 KiB
// of W in flight at D = 2; the same bytes in flight as fewer, deeper waves
// (D = 3 at four waves, 4 at three, 8 at two) measured within 1.5 %.
//
// The tile walk is the plain one, tile g % tiles: no byte of W is read by two
// workgroups of a pass, so there is nothing for gemm_order to keep in an L2,
// and A is in every L2. A tile's rows are one contiguous piece of memory.
//
// Bounds. N and K are multiples of the tile and of the step. W: (32 j + r) x
// row bytes + 16 x chunk + 128 x step + 15 with 32 j + r < 128, chunk < 8 and
// step < steps is below 128 x row bytes, the window. Tiled W: j x steps x
// 4096 + 16 x lane + 1024 x p + 4096 x step + 15 with j < 4, lane < 64, p < 4
// and step < steps is at most j x steps x 4096 + 4096 (steps - 1) + 4095,
// below (j + 1) x steps x 4096 <= 4 x steps x 4096 = 128 x row bytes, the same
// window; past the last step bit 31 puts it outside, as for rows (the offset
// stays below 2^31 + 2^22). A: the same as rows with r < 32
// in a window of 32 rows. W's scale words: window from the tile's first word
// to its last of the last step, ((steps - 1) N + 128) words, offset step x N +
// 32 j + r; A's: steps x 32 words, offset 32 step + r. Every window is below
// 2^31 bytes (W's scale words of all tiles at most 2^20 x 256 x 4). An LDS
// index is buffer x 256 + 64 p + lane < 512.
//
// Exactness. The elements and scales are the prefill kernels', so their
// bounds hold: K <= 32768 (mxfp8) and 16384 (mxfp4) keep every accumulator
// an exact integer in f32.
//
// Result. Every lane weighs its 16 entries at (m, n), n global, by (1 + m) (1
// + n) modulo 2^64; the 256 sums are added up through LDS and thread 0
// stores the workgroup's word (gemm_store_sum). Stamps and clocks are
// clocked_end's. No FP32 arithmetic but the MFMAs' is written here.
//
// hipcc -O3 for gfx950 reports (-Rpass-analysis=kernel-resource-usage), mxfp8
// and mxfp4: 89 and 94 VGPRs (16 of accumulator, 2 x 22 or 24 of loads in
// flight, 16 of A's fragments), no AGPRs, 45 and 49 SGPRs, no scratch and no
// spills, 10240 bytes of LDS and an occupancy of 5 waves per SIMD, by
// registers. Every kernel that was here before reports what it did. The
// tiled instantiations report 89 and 94 VGPRs, no AGPRs, 46 and 49 SGPRs, no
// scratch and no spills, 10240 bytes of LDS and 5 waves per SIMD, and their
// assembly has the waits of the row-major ones: vmcnt(11) for the scale
// words, vmcnt(12) (mxfp8) or vmcnt(13) (mxfp4) in front of each MFMA,
// vmcnt(13) in front of the slab write, no vmcnt(0) in the loop, the pieces
// at offset:1024, 2048 and 3072. The row-major instantiations keep their
// instructions, 427 and 444, one for one.
//
// On the card (profiles/decode_cotenancy_results.md) the default window
// streams its weights at 5.2 (mxfp8) and 4.6 TB/s (mxfp4) where the stream
// tenant reads 6.5-6.8, at an unlowered clock of 2.39 GHz, and on half the
// CUs at 0.56 of that where the streamer keeps 6.1; neither the distance nor
// the waves move it. So the limit is in the CUs, not HBM; a load instruction
// touches 32 lines of 128 bytes, one per row, for 1 KiB. That was the cause
// (profiles/decode_tiled_cotenancy_results.md): on tiled weights, alternating
// with row-major ones in fresh processes beside a streamer at 7.06 TB/s, the
// default window streams 5.69 (mxfp8) and 5.67 TB/s (mxfp4) against 5.17 and
// 4.59, and on half the CUs 4.66 and 4.27 against 2.92 and 2.54 where the
// streamer reads 6.19. Four steps at three waves and eight at two, on tiled
// weights, stayed within 1 % of two at five on the whole card and fell 1 to 7
// % behind on half of it, so one distance and one occupancy serve both
// layouts.
template <int F, bool kTiled>
__global__ void __launch_bounds__(kBlock, kDecodeWaves)
tenant_decode_kernel(const int4v* __restrict__ a, const int4v* __restrict__ w,
                     const typename MxGemm<F>::Word* __restrict__ sa,
                     const typename MxGemm<F>::Word* __restrict__ sw, uint32_t tiles,
                     uint32_t steps, unsigned long long* __restrict__ out,
                     unsigned long long* __restrict__ rec,
                     unsigned long long* __restrict__ clk) {
  using G = MxGemm<F>;
  constexpr int D = kDecodeDistance;
  // From one weight piece of a lane to its next, and from one step to the
  // next: within the row, or through the row block's units.
  constexpr uint32_t kPiece =
      kTiled ? kDecodeUnitBytes / 4 : 16 * (decode_chunk<F>(1, 0) - decode_chunk<F>(0, 0));
  constexpr uint32_t kStepBytes = kTiled ? kDecodeUnitBytes : kGemmRowVecs * 16;
  __shared__ int4v slab[2][kBlock];  // [buffer][plane x 64 + lane]
  __shared__ unsigned long long sums[kBlock];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = lane & 31u, h = lane >> 5;
  const uint32_t wave = threadIdx.x / 64;
  const uint32_t tile = blockIdx.x % tiles;
  const uint32_t n_rows = tiles * kGemmTile;
  const uint32_t row_bytes = steps * (kGemmRowVecs * 16);
  const uint32_t w_at = kTiled ? wave * steps * kDecodeUnitBytes + 16 * lane
                               : (32 * wave + r) * row_bytes + 16 * decode_chunk<F>(0, h);
  const uint32_t a_at = r * row_bytes + 16 * decode_chunk<F>(wave, h);
  const uint32_t sw_at = (32 * wave + r) * G::kWordBytes, sa_at = r * G::kWordBytes;
  const auto rw = buffer_window(w + static_cast<uint64_t>(tile) * kGemmTile * (row_bytes / 16),
                                kGemmTile * row_bytes);
  const auto ra = buffer_window(a, kDecodeRows * row_bytes);
  const auto rsw = buffer_window(sw + tile * kGemmTile,
                                 ((steps - 1) * n_rows + kGemmTile) * G::kWordBytes);
  const auto rsa = buffer_window(sa, steps * kDecodeRows * G::kWordBytes);

  DecodeFetch<F> p[D];
  // Nothing is scheduled across a pin: the loads keep the order they are
  // written in, the same in the prologue and in every step.
  const auto pin = [] { __builtin_amdgcn_sched_barrier(0); };
  // The loads of step `at_step`, past the last step outside every window:
  // first the slab chunk and the two scale words, then the weight pieces.
  const auto fetch_head = [&](DecodeFetch<F>& f, uint32_t at_step)
      __attribute__((always_inline)) {
    const uint32_t outside = at_step < steps ? 0u : kBufferOutside;
    f.a = __builtin_bit_cast(int4v, __builtin_amdgcn_raw_buffer_load_b128(
        ra, a_at | outside, at_step * (kGemmRowVecs * 16), 0));
    pin();
    f.sw = mx_load_word<F>(rsw, sw_at | outside, at_step * n_rows * G::kWordBytes);
    pin();
    f.sa = mx_load_word<F>(rsa, sa_at | outside, at_step * kDecodeRows * G::kWordBytes);
    pin();
  };
  const auto fetch_piece = [&](DecodeFetch<F>& f, uint32_t at_step, uint32_t pc)
      __attribute__((always_inline)) {
    const uint32_t outside = at_step < steps ? 0u : kBufferOutside;
    f.w[pc] = __builtin_bit_cast(int4v, __builtin_amdgcn_raw_buffer_load_b128(
        rw, (w_at | outside) + kPiece * pc, at_step * kStepBytes, 0));
    pin();
  };
  f32x16 acc;
  // Step i from the set `mine`, which the loads of step i + D replace piece
  // by piece behind the MFMA that read the piece; `next` holds the slab of
  // step i + 1.
  const auto step = [&](DecodeFetch<F>& mine, const DecodeFetch<F>& next, uint32_t i)
      __attribute__((always_inline)) {
    int4v af[4];
#pragma unroll
    for (int pc = 0; pc < 4; ++pc) af[pc] = slab[i & 1u][64 * pc + lane];
    if constexpr (F == kMxfp8) {
      const int ca = static_cast<int>(static_cast<uint32_t>(mine.sa) >> (8 * h));
      const int cw = static_cast<int>(static_cast<uint32_t>(mine.sw) >> (8 * h));
      pin();
      fetch_head(mine, i + D);
      acc = decode_mfma<F, 0, 0>(af, mine.w, acc, ca, cw);
      pin();
      fetch_piece(mine, i + D, 0);
      fetch_piece(mine, i + D, 1);
      acc = decode_mfma<F, 1, 2>(af, mine.w, acc, ca, cw);
      pin();
      fetch_piece(mine, i + D, 2);
      fetch_piece(mine, i + D, 3);
    } else {
      const uint32_t ca = static_cast<uint32_t>(h ? mine.sa[1] : mine.sa[0]);
      const uint32_t cw = static_cast<uint32_t>(h ? mine.sw[1] : mine.sw[0]);
      const int ca1 = static_cast<int>(ca >> 8), cw1 = static_cast<int>(cw >> 8);
      pin();
      fetch_head(mine, i + D);
      acc = decode_mfma<F, 0, 0>(af, mine.w, acc, static_cast<int>(ca), static_cast<int>(cw));
      pin();
      fetch_piece(mine, i + D, 0);
      acc = decode_mfma<F, 1, 0>(af, mine.w, acc, ca1, cw1);
      pin();
      fetch_piece(mine, i + D, 1);
      acc = decode_mfma<F, 2, 2>(af, mine.w, acc, static_cast<int>(ca), static_cast<int>(cw));
      pin();
      fetch_piece(mine, i + D, 2);
      acc = decode_mfma<F, 3, 2>(af, mine.w, acc, ca1, cw1);
      pin();
      fetch_piece(mine, i + D, 3);
    }
    slab[(i + 1) & 1u][threadIdx.x] = next.a;
    __syncthreads();
    pin();
  };

  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  const unsigned long long t0 = stamp_start();
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) acc[reg] = 0.0f;
  pin();
#pragma unroll
  for (int u = 0; u < D; ++u) {
    fetch_head(p[u], u);
#pragma unroll
    for (uint32_t pc = 0; pc < 4; ++pc) fetch_piece(p[u], u, pc);
  }
  slab[0][threadIdx.x] = p[0].a;
  __syncthreads();
  pin();
  for (uint32_t i = 0; i < steps; i += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) step(p[u], p[(u + 1) % D], i + u);
  }

  uint64_t column = 0;
#pragma unroll
  for (uint32_t reg = 0; reg < 16; ++reg)
    column += static_cast<uint64_t>(static_cast<int64_t>(static_cast<int>(acc[reg]))) *
              static_cast<uint64_t>(1 + 4 * h + (reg & 3u) + 8 * (reg >> 2));
  gemm_store_sum(sums, column * static_cast<uint64_t>(1 + tile * kGemmTile + 32 * wave + r), out);
  clocked_end(rec, clk, c0, t0);
}

// ---- attention ---------------------------------------------------------------

constexpr int kAttnDim = 128;    // head dimension: a row of Q, K, V or O is 256 bytes
constexpr int kAttnRows = 128;   // query rows per workgroup, 32 per wave
constexpr int kAttnKeys = 64;    // keys per K/V tile
constexpr int kAttnRowVecs = kAttnDim * 2 / 16;          // 16-byte chunks per row: 16
constexpr int kAttnTileVecs = kAttnKeys * kAttnRowVecs;  // one tile of K or V: 16 KiB
constexpr int kAttnLoads = kAttnTileVecs / kBlock;       // loads per lane, operand and tile: 4
constexpr uint32_t kAttnKeySalt = 0x4154544Eu;
constexpr int kAttnDefaultIters = 64, kAttnMaxIters = 256;  // sequence length / 128
constexpr uint64_t kAttnDefaultHeads = 64, kAttnMaxHeads = 1024;
// A default launch on a whole card lasts about as long as gemm's
// (profiles/attention_cotenancy_results.md).
constexpr int kAttnDefaultPasses = 8;
constexpr int kAttnSamples = 256;  // rows the reference kernel recomputes
constexpr uint64_t kAttnMaxOutput = 64 * kMiB;  // attention_output: the most it returns
// log2(e) / sqrt(128): exp((s - m) / sqrt(128)) = exp2((s - m) * kAttnScale).
constexpr float kAttnScale = 1.4426950408889634f * 0.08838834764831845f;

using short4v = __attribute__((ext_vector_type(4))) short;
using f32x2 = __attribute__((ext_vector_type(2))) float;

// A value that bf16 holds exactly, as its bits: the float's upper half.
__device__ inline short exact_bf16_bits(float v) {
  return static_cast<short>(__float_as_uint(v) >> 16);
}

// The operands of an attention tenant: `buf` is Q, [head][q_rows][128] bf16,
// then K, then V, each [head][seq][128] (the prefill kind: q_rows = seq; the
// decode kind: 16). key = mix32(seed_key ^ which * 0x9E3779B1 ^ head) with
// which = 0, 1, 2 and seed_key = mix32(seed32 ^ 0x4154544E); the element at
// [row][d] is (mix32(key ^ (row << 7 | d)) % 31 - 15) / 8, / 4 or / 16: at most
// four significant bits under a power of two, exact in bf16. One 16-byte store
// of eight elements per step, grid-stride; n16 = heads * (q_rows + 2 seq) * 16
// counts the stores. All indices are 64-bit and below n16; row < 2^15, so row
// << 7 | d is below 2^22.
__global__ void __launch_bounds__(kBlock)
tenant_attention_fill_kernel(int4v* __restrict__ buf, uint64_t n16, uint32_t heads,
                             uint32_t q_rows, uint32_t seq, uint32_t seed_key) {
  uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
  const uint64_t q_vecs = static_cast<uint64_t>(q_rows) * kAttnRowVecs * heads;
  const uint64_t per_operand = static_cast<uint64_t>(seq) * kAttnRowVecs * heads;
  for (; i < n16; i += stride) {
    const uint32_t which = i < q_vecs ? 0u : 1u + static_cast<uint32_t>((i - q_vecs) / per_operand);
    const uint64_t at = i < q_vecs ? i : (i - q_vecs) % per_operand;
    const uint64_t per_head = static_cast<uint64_t>(which == 0 ? q_rows : seq) * kAttnRowVecs;
    const uint32_t head = static_cast<uint32_t>(at / per_head);
    const uint32_t row = static_cast<uint32_t>(at % per_head / kAttnRowVecs);
    const uint32_t d0 = static_cast<uint32_t>(at % kAttnRowVecs) * 8;
    const uint32_t key = mix32(seed_key ^ (which * 0x9E3779B1u) ^ head);
    const float scale = which == 0 ? 0.125f : which == 1 ? 0.25f : 0.0625f;
    short8 v;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      const uint32_t hash = mix32(key ^ (row << 7 | (d0 + j)));
      v[j] = exact_bf16_bits(static_cast<float>(static_cast<int>(hash % 31u) - 15) * scale);
    }
    buf[i] = __builtin_bit_cast(int4v, v);
  }
}

// Where 16-byte chunk c (0..15, d = 8c .. 8c + 7) of row `row` of a K tile or
// of a V tile lives, as the XOR key of its chunk position: a row's 256 bytes
// are unpadded and span all 64 banks, so only the position decides the banks.
//   K is read as MFMA A fragments with ds_read_b128, lane r on row base + r at
//   one chunk per h: the key takes 16 values over 16 consecutive rows, and
//   rows 0..7 differ in its upper three bits, so that 16 lanes of one h, or
//   eight of h = 0 (chunk c) with eight of h = 1 (chunk c ^ 1), fall into 16
//   different bank groups of 16 bytes (gemm_key's argument, for 16 chunks).
//   V is read with ds_read_b64_tr_b16, 32 lanes on 4 consecutive rows (base a
//   multiple of 4) x 4 consecutive chunks 4u .. 4u + 3: the key moves row
//   (R & 3) by 4 (R & 3) chunks, so the 16 (row, chunk) pairs take all 16
//   positions and the 32 8-byte reads all 64 banks.
__device__ inline uint32_t attn_k_key(uint32_t row) {
  return ((row & 7u) << 1) | ((row >> 3) & 1u);
}
__device__ inline uint32_t attn_v_key(uint32_t row) { return (row & 3u) << 2; }

// One number across the lane pair (l, l + 32), which holds one query column:
// v_permlane32_swap exchanges the upper half of its first operand with the
// lower half of its second, so with both operands x the two results are, in
// either half, the lane's own x and the other lane's.
__device__ inline f32x2 attn_pair(float x) {
  const auto both = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x),
                                                     false, false);
  return f32x2{__uint_as_float(both[0]), __uint_as_float(both[1])};
}

// A causal flash-attention forward pass in bf16: per head O = softmax(Q K^T /
// sqrt(128), causal) V, row i attending to keys 0 .. i, head dimension 128, Q,
// K, V and O row-major [head][row][128]. The grid is passes x heads x seq / 128
// workgroups, every pass the same product into its own O.
//
// Work split. A workgroup owns 128 query rows of one head of one pass, wave j
// rows 32 j .. 32 j + 31. Workgroup g of a pass takes query tile T - 1 - g /
// heads of head g % heads, T = seq / 128: the longest tiles (most keys) start
// first, so that what is left at the end of a launch are the short ones.
// (Supposed, not measured: if consecutive workgroup ids go round the 8 XCDs,
// as gemm_order takes them to, then with heads a multiple of 8 a head's
// workgroups, heads apart in g, share one XCD and its L2 for K and V. No
// counter was read to confirm it.)
//
// Scores. Per tile of 64 keys a wave computes S^T = K Q^T, 64 keys x 32
// queries, as two 32 x 32 accumulators (keys 32 t ..) over d = 128 in eight
// v_mfma_f32_32x32x16_bf16 each: A is K from LDS (lane r + 32 h: key 32 t + r,
// chunk 2 s + h at sub-step s), B is Q, loaded once from memory into registers
// in that same fragment layout (lane r + 32 h: query r, chunk 2 s + h). Lane r
// + 32 h then holds in register i of accumulator t the score of query r and
// key 32 t + (i & 3) + 8 (i >> 2) + 4 h: 32 keys of one query column. The
// maximum of a column is an in-lane maximum and one exchange with lane r + 32
// h ^ 32 (attn_pair); no LDS round trip.
//
// Softmax, online and in base 2: m is the running maximum of the raw scores
// and l the running sum, both f32; a tile gives m' = max(m, tile), alpha =
// exp2((m - m') c), p = exp2((s - m') c), c = log2(e) / sqrt(128), l = l alpha
// + sum of p, O = O alpha + P V, all exponentials v_exp_f32. A lane sums only
// its own 32 keys into l (alpha is the pair's), and the pair is added up once
// at the end, where O is divided by l and stored as bf16. Key 0 is in every
// row's first tile and never masked, so m is finite from the first tile on:
// alpha is exp2(-inf) = 0 there, and a tile whose keys a row may not see at
// all leaves m alone and gives p = exp2(-inf) = 0.
//
// Output. O^T = V^T P^T, 128 d x 32 queries as four accumulators (d 32 u ..),
// 16 MFMAs per tile: sixteen keys a step, step (t, g) taking registers 8 g ..
// 8 g + 7 of score accumulator t, rounded to bf16 (nearest even), as they are
// as the B operand. Lane r + 32 h, slot e of that operand is key kappa = 32 t
// + 16 g + 8 (e >> 2) + 4 h + (e & 3), not the 8 h + e the instruction counts
// by; P is not moved, the A operand pairs it with V[kappa]: lane r' + 32 h,
// slot e holds V[kappa][32 u + r']. Those come from the row-major V tile with
// two ds_read_b64_tr_b16 per fragment: in a block of 16 lanes, lane i points
// at the four elements 4 (i & 3) .. + 3 of row i >> 2 of a 4 x 16 block, and
// receives column i of its four rows. Block b = lane >> 4 reads rows 32 t +
// 16 g + 8 x + 4 h .., x = 0, 1 the half of the fragment, columns 32 u + 16
// (b & 1) ...
//
// Data movement. K and V travel global memory -> LDS in tiles of 64 keys, 16
// KiB each, with tenant_gemm_direct_kernel's 16-byte LDS-DMA load and its
// discipline: LDS holds two pairs {K tile, V tile}, 64 KiB, two workgroups per
// CU; step i issues the eight loads of tile i + 1 into the other pair,
// computes from pair i & 1, waits for vmcnt(0) and crosses one barrier. The
// pair overwritten in step i was last read in step i - 1, which every wave
// left through its barrier after its MFMAs had consumed what it read. One
// wave instruction fills 64 consecutive chunk positions, four whole rows:
// wave w's instruction i fills rows 16 i + 4 w .. + 3, lane l on row R = 16 i
// + 4 w + (l >> 4) at position l & 15, and fetches chunk (l & 15) ^ key(R)
// of that row; neither key depends on i (attn_k_key: bits 0..3 of R are those
// of 4 w + (l >> 4); attn_v_key: bits 0..1 are l >> 4).
//
// Masking. Tiles above the diagonal are never loaded: a workgroup on query
// tile qt runs 2 (qt + 1) tiles, keys 0 .. 128 qt + 127. Only the last two can
// hold a key beyond one of its rows; there, and only there, a score whose key
// is beyond its query is set to -inf before the maximum.
//
// Barriers. The tile count is the workgroup's, from blockIdx alone: every wave
// runs the same number of steps and reaches every barrier, a wave whose rows
// see nothing of a tile included; the only branches inside a step are the
// mask's, which holds no barrier and no load. No load has a branch around it:
// the tile past the last is issued with bit 31 set in every lane's offset,
// outside any window, reads nothing, and lands in a pair nobody reads again.
//
// Bounds. Buffer loads on a descriptor of the head's K or V, seq x 256 bytes
// (at most 8 MiB): a lane's offset is (4 w + (l >> 4)) x 256 + 16 x chunk, the
// shared one (64 tile + 16 i) x 256, together row x 256 + 16 chunk with row <
// 64 (tile + 1) <= 128 (qt + 1) <= seq and chunk < 16. An LDS address handed
// to a load is pair x 32 KiB + operand x 16 KiB + (16 i + 4 w) x 256 + 16 l +
// 15 < 64 KiB, wave-uniform by construction. A fragment read is row < 64 and
// position < 16 of a tile. Q and O rows are 128 qt + 32 j + r < seq of the
// head, and the pass's O.
//
// Stamps and clocks are the gemm kinds' (clocked_end); Q's loads and the
// first tile's are inside them.
//
// hipcc -O3 for gfx950 reports (-Rpass-analysis=kernel-resource-usage) 176
// VGPRs, no AGPRs, 38 SGPRs, no scratch and no spills, 65536 bytes of LDS and
// an occupancy of 2 waves per SIMD, by LDS and by registers alike. On the
// card it spends 61.4-63.4 (whole card) and 61.2-61.5 (half) cycles per MFMA
// and SIMD where the instruction takes 32, about 0.52 of the matrix pipe
// (profiles/attention_cotenancy_results.md).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"  // m0 is clobbered on purpose
__global__ void __launch_bounds__(kBlock, 2)
tenant_attention_kernel(const int4v* __restrict__ q, const int4v* __restrict__ k,
                        const int4v* __restrict__ v, short4v* __restrict__ o, uint32_t heads,
                        uint32_t qtiles, unsigned long long* __restrict__ rec,
                        unsigned long long* __restrict__ clk) {
  __shared__ int4v ring[2][2][kAttnTileVecs];  // [pair][K, V]
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = lane & 31u, h = lane >> 5;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const uint32_t per_pass = heads * qtiles;
  const uint32_t pass = blockIdx.x / per_pass, in_pass = blockIdx.x % per_pass;
  const uint32_t qt = qtiles - 1 - in_pass / heads, head = in_pass % heads;
  const uint32_t seq = qtiles * kAttnRows;
  const uint32_t tiles = 2 * (qt + 1);
  const uint64_t head_vecs = static_cast<uint64_t>(seq) * kAttnRowVecs;
  // What this lane loads: of rows 4 wave + (lane >> 4) + 16 i the chunk that
  // belongs at position lane & 15.
  const uint32_t land_row = 4 * wave + (lane >> 4);
  const uint32_t load_k = land_row * 256 + 16 * ((lane & 15u) ^ attn_k_key(land_row));
  const uint32_t load_v = land_row * 256 + 16 * ((lane & 15u) ^ attn_v_key(land_row));
  const uint32_t land_at = 4 * wave * kAttnRowVecs;  // + 16 rows: + 256
  const auto window = [&](const int4v* first) {
    const uint64_t base = reinterpret_cast<uint64_t>(first);
    return int4v{static_cast<int>(static_cast<uint32_t>(base)),
                 static_cast<int>(static_cast<uint32_t>(base >> 32) & 0xFFFFu),
                 static_cast<int>(seq * 256u), kBufferWord3};
  };
  const auto rk = window(k + head * head_vecs);
  const auto rv = window(v + head * head_vecs);
  // What this lane reads of a K tile: rows r + 32 t, chunk (2 s + h) ^ key; of
  // a V tile, per d block u: row 4 h + (i >> 2) (+ 32 t + 16 g + 8 x), chunk 4 u
  // + 2 (b & 1) + ((i >> 1) & 1) under the row's key 4 (i >> 2), bytes 8 (i & 1)
  // .. + 7 of it, i = lane & 15 and b = lane >> 4.
  const uint32_t read_k = r * kAttnRowVecs, read_key = attn_k_key(r);
  const uint32_t i16 = lane & 15u;
  uint32_t read_v[4];  // in bytes
#pragma unroll
  for (uint32_t u = 0; u < 4; ++u)
    read_v[u] = (4 * h + (i16 >> 2)) * 256 +
                16 * ((4 * u + 2 * ((lane >> 4) & 1u) + ((i16 >> 1) & 1u)) ^ (i16 & 12u)) +
                8 * (i16 & 1u);
  const uint32_t my_query = 32 * wave + r;  // within the workgroup's 128
  const uint64_t q_row = static_cast<uint64_t>(head) * seq + qt * kAttnRows + my_query;
  const int4v* pq = q + q_row * kAttnRowVecs + h;

  const auto load = [](int4v rsrc, const int4v* lds, uint32_t lane_off, uint32_t shared_off)
      __attribute__((always_inline)) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                 :
                 : "s"(static_cast<uint32_t>(reinterpret_cast<uintptr_t>((LdsPtr)lds))),
                   "v"(lane_off), "s"(rsrc), "s"(shared_off)
                 : "memory", "m0");
  };
  // The eight loads of tile `at` into the pair `to`.
  const auto issue = [&](const int4v (*to)[kAttnTileVecs], uint32_t at)
      __attribute__((always_inline)) {
    const uint32_t outside = at < tiles ? 0u : kBufferOutside;
    const uint32_t tile_off = at * (kAttnKeys * 256);
#pragma unroll
    for (int i = 0; i < kAttnLoads; ++i) {
      load(rk, to[0] + land_at + 16 * kAttnRowVecs * i, load_k | outside, tile_off + 16 * 256 * i);
      load(rv, to[1] + land_at + 16 * kAttnRowVecs * i, load_v | outside, tile_off + 16 * 256 * i);
    }
  };
  const auto landed = [] {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  };

  bf16x8 qf[8];
  f32x16 out[4];
  float m = -__builtin_inff(), l = 0.0f;
  // One tile: scores, online softmax, output.
  const auto step = [&](const int4v (*from)[kAttnTileVecs], uint32_t at)
      __attribute__((always_inline)) {
    f32x16 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) s[t][reg] = 0.0f;
#pragma unroll
    for (uint32_t sub = 0; sub < 8; ++sub) {
      const uint32_t c = (2 * sub + h) ^ read_key;
#pragma unroll
      for (uint32_t t = 0; t < 2; ++t) {
        const bf16x8 kf =
            __builtin_bit_cast(bf16x8, from[0][read_k + 32 * kAttnRowVecs * t + c]);
        s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[sub], s[t], 0, 0, 0);
      }
    }
    if (at + 2 >= tiles) {  // a diagonal tile: its keys start at 0 or 64 of the 128
      const uint32_t key0 = 64 * (at + 2 - tiles) + 4 * h;
#pragma unroll
      for (uint32_t t = 0; t < 2; ++t)
#pragma unroll
        for (uint32_t reg = 0; reg < 16; ++reg)
          if (key0 + 32 * t + (reg & 3u) + 8 * (reg >> 2) > my_query)
            s[t][reg] = -__builtin_inff();
    }
    float top = s[0][0];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) top = __builtin_fmaxf(top, s[t][reg]);
    const f32x2 tops = attn_pair(top);
    const float m_new = __builtin_fmaxf(m, __builtin_fmaxf(tops[0], tops[1]));
    const float alpha = __builtin_amdgcn_exp2f((m - m_new) * kAttnScale);
    m = m_new;
    bf16x8 p[2][2];  // [t][g]: registers 8 g .. 8 g + 7 of s[t]
    float sum = 0.0f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const float e = __builtin_amdgcn_exp2f((s[t][reg] - m) * kAttnScale);
        sum += e;
        p[t][reg >> 3][reg & 7] = static_cast<__bf16>(e);
      }
    l = l * alpha + sum;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) out[u][reg] *= alpha;
    const char* tile_v = reinterpret_cast<const char*>(from[1]);
#pragma unroll
    for (uint32_t tg = 0; tg < 4; ++tg) {  // keys 16 tg ..: t = tg >> 1, g = tg & 1
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u) {
        short4v half[2];
#pragma unroll
        for (uint32_t x = 0; x < 2; ++x)
          half[x] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) short4v*)(tile_v + read_v[u] +
                                                           (16 * tg + 8 * x) * 256));
        const short8 vf = __builtin_shufflevector(half[0], half[1], 0, 1, 2, 3, 4, 5, 6, 7);
        out[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vf),
                                                         p[tg >> 1][tg & 1u], out[u], 0, 0, 0);
      }
    }
  };

  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  const unsigned long long t0 = stamp_start();
#pragma unroll
  for (int sub = 0; sub < 8; ++sub) qf[sub] = __builtin_bit_cast(bf16x8, pq[2 * sub]);
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) out[u][reg] = 0.0f;
  issue(ring[0], 0);
  landed();
  // Q is in its registers here, and the compiler knows it: it counts its own
  // loads only, so a wait for Q that it placed at the first use, inside the
  // loop, would be a wait for the tile just issued in every step.
  asm volatile("" : "+v"(qf[0]), "+v"(qf[1]), "+v"(qf[2]), "+v"(qf[3]), "+v"(qf[4]),
               "+v"(qf[5]), "+v"(qf[6]), "+v"(qf[7]));
  for (uint32_t i = 0; i < tiles; ++i) {
    issue(ring[(i + 1) & 1u], i + 1);
    step(ring[i & 1u], i);
    landed();
  }
  // O[query][32 u + 8 a + 4 h + 0..3] = registers 4 a .. 4 a + 3 of out[u] / l.
  const f32x2 sums = attn_pair(l);
  const float scale = 1.0f / (sums[0] + sums[1]);
  short4v* po = o + ((static_cast<uint64_t>(pass) * heads * seq + q_row) * kAttnDim) / 4 + h;
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      short4v four;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        four[j] = __builtin_bit_cast(short, static_cast<__bf16>(out[u][4 * a + j] * scale));
      po[8 * u + 2 * a] = four;
    }
  clocked_end(rec, clk, c0, t0);
}
#pragma clang diagnostic pop

// ---- attention, the decode shape ---------------------------------------------

// Ring depth per wave, in stages of kAdKeys keys: 2 as built (one workgroup
// per CU, 128 KiB of LDS), 1 with GPUPROBE_ATTN_DECODE_DEPTH=1 (64 KiB, two
// workgroups per CU, a wave's loads overlapped by the other seven waves only).
#ifndef GPUPROBE_ATTN_DECODE_DEPTH
#define GPUPROBE_ATTN_DECODE_DEPTH 2
#endif
constexpr int kAdDepth = GPUPROBE_ATTN_DECODE_DEPTH;
constexpr int kAdKeys = 32;  // keys per stage: the k of one output MFMA
static_assert(kAdDepth == 1 || kAdDepth == 2, "160 KiB of LDS hold 4 waves x 2 stages at most");
static_assert(kAdKeys == 32, "a stage is the 32 keys of one v_mfma_f32_16x16x32_bf16");
constexpr int kAdQueries = 16;                          // query rows per head
constexpr int kAdTileVecs = kAdKeys * kAttnRowVecs;     // a stage of K or of V: 8 KiB
constexpr int kAdLoads = kAdTileVecs / 64;              // loads per lane, operand and stage: 8
constexpr int kAdSplitFloats = kAdQueries * kAttnDim;   // a split's O, f32
constexpr uint64_t kAdDefaultHeads = 256;
constexpr int kAdTargetGroups = 2048;  // splits = this / heads, at least 1024 keys each
// A default launch on a whole card lasts 6.2 ms beside 8.4-9.2 ms of gemm's in
// the same run, on half of it 8.2 beside 14.7
// (profiles/attention_decode_cotenancy_results.md).
constexpr int kAdDefaultPasses = 32;

using f32x4 = __attribute__((ext_vector_type(4))) float;

// The live keys of head `head`: every residue of 128 occurs over 128 heads.
__host__ __device__ inline uint32_t attn_decode_len(uint32_t head, uint32_t seq) {
  return seq - (37u * head) % 128u;
}

// The maximum or the sum of x over the four lanes l, l + 16, l + 32, l + 48,
// in all four: v_permlane16_swap exchanges the odd rows (of 16 lanes) of its
// first operand with the even rows of its second, so with both operands x
// the results are rows {0, 0, 2, 2} and {1, 1, 3, 3} of x; attn_pair does the
// same for the halves. No LDS round trip, and every lane of the four adds
// the same numbers in the same order.
template <bool kMax>
__device__ inline float attn_quad(float x) {
  const auto rows = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x),
                                                     false, false);
  const float a = __uint_as_float(rows[0]), b = __uint_as_float(rows[1]);
  const f32x2 halves = attn_pair(kMax ? __builtin_fmaxf(a, b) : a + b);
  return kMax ? __builtin_fmaxf(halves[0], halves[1]) : halves[0] + halves[1];
}

// exp2((m - top) c) for a running maximum m that may still be -inf under a
// maximum `top` that may be -inf too: the difference of two -inf never
// reaches the exponential, a part without a key weighs 0.
__device__ inline float attn_weight(float m, float top) {
  return __builtin_amdgcn_exp2f(m == -__builtin_inff() ? m : (m - top) * kAttnScale);
}

// The decode step's attention in bf16: 16 query rows (a grouped-query group of
// 16, or 8 at two speculative positions) of one head attend to the head's live
// keys, O = softmax(Q K^T / sqrt(128)) V with no mask but the length, head
// dimension 128, Q [head][16][128], K and V [head][seq][128] row-major. Head h
// is live for len(h) = seq - 37 h % 128 keys; keys beyond are in memory and
// must not count. Every byte of K and V is read once per pass and meets the
// same 16 queries: memory sets the pace, not the matrix pipe.
//
// Work split. The grid is passes x heads x splits workgroups, workgroup g on
// split g % splits of head g / splits % heads; split s owns keys [128 span s,
// min(128 span (s + 1), len)), `live` of them, possibly none. Nothing is
// shared between waves, so the split's ceil(live / 32) tiles of 32 keys are
// dealt round: wave j takes tiles j, j + 4, ..., (tiles - j + 3) / 4 of them or
// none, into a ring of its own in LDS, with its own running m, l and O^T. No
// barrier is inside the key loop: a wave waits for its own loads with
// s_waitcnt vmcnt(n) alone. (That vmcnt's in-order return makes the bytes of
// an LDS-DMA load visible to a later ds_read of the same wave is read from the
// ISA description; the every-element test is what confirms it.)
//
// Data movement. K and V travel memory -> LDS with tenant_gemm_direct_kernel's
// 16-byte LDS-DMA load, one wave instruction filling 4 whole rows (8 lines).
// A stage is 32 keys, 8 KiB of K and 8 KiB of V, 8 + 8 loads per lane, K's
// first. Step i issues the stage of tile i + kAdDepth - 1 (the prologue those
// before it), waits until at most 8 + 16 (kAdDepth - 1) loads are outstanding,
// which is when tile i's K has landed, computes the scores and the softmax,
// waits for at most 16 (kAdDepth - 1), tile i's V, and adds to the output. The
// stage a step overwrites was last read one step earlier (depth 1: in this
// step's predecessor), by this wave alone; an s_waitcnt lgkmcnt(0) in front of
// the first load of a stage says that those reads have returned. Lane l of
// instruction n lands on position l & 15 of row R = 4 n + (l >> 4) of the tile
// and fetches chunk (l & 15) ^ attn_k_key(R); the key depends on n & 3 only, so
// four lane offsets serve K and V alike. Fragment reads: K as MFMA A operands,
// ds_read_b128, lane r + 16 g on row 16 t + r at chunk 4 s + g, 16 rows whose
// keys are all 16 values, or eight rows each of chunk c and c ^ 1, whose keys
// are the even ones: 16 bank groups either way (attn_k_key's argument). V with
// ds_read_b64_tr_b16, 32 lanes on 8 consecutive rows (base a multiple of 8) x
// chunks 2 u and 2 u + 1: the eight keys differ in bits 1..3, so the 16 (row,
// chunk) pairs take 16 positions and the 32 8-byte reads all 64 banks. So the
// one key function serves both tiles.
//
// Scores. S^T = K Q^T per tile, 32 keys x 16 queries, as two 16 x 16
// accumulators (keys 16 t ..) over d = 128 in four v_mfma_f32_16x16x32_bf16
// each: A is K from LDS, B is Q, loaded once (lane r + 16 g: query r, chunk 4 s
// + g). Lane r + 16 g then holds in register i of accumulator t the score of
// query r and key 16 t + 4 g + i: a query column's 32 scores sit in four lanes
// x 8 registers, its maximum is in-lane plus attn_quad.
//
// Softmax, online and in base 2 as in the prefill kernel. Only the last tile of
// a split can hold a key at or beyond len; there, and only there, such a score
// is set to -inf before the maximum, whatever K's bits were (a select, no
// arithmetic). Every tile a wave runs has a live key, so m is finite from a
// wave's first tile on: alpha = exp2(-inf) = 0 there and never exp2(-inf - -inf).
// A wave without a tile keeps m = -inf, l = 0, O = 0.
//
// Output. O^T = V^T P^T, 128 d x 16 queries as eight 16 x 16 accumulators (d 16
// u ..), one MFMA of k = 32 keys each per tile. P, rounded to bf16, stays where
// the scores left it: slot e of lane r + 16 g is key kappa = 16 (e >> 2) + 4 g +
// (e & 3), not the 8 g + e the instruction counts by, and the A operand pairs
// it: lane i + 16 g, slot e holds V[kappa][16 u + i]. Two ds_read_b64_tr_b16 per
// fragment: block g of 16 lanes reads the 4 x 16 block of rows 16 x + 4 g .. + 3,
// columns 16 u .. + 15, lane i pointing at row i >> 2, elements 4 (i & 3) .. + 3,
// and receives column i of the four rows, slots 4 x .. 4 x + 3.
//
// Tail. The descriptors are sized to the head's live rows, len x 256 bytes, and
// the whole row offset is in the lane's offset register, which is what the
// range check looks at: nothing at or past len is fetched, and the tile past a
// wave's last is sent to bit 31, outside any window (no load has a branch
// around it). An unfetched V row must not meet p = 0 as stale bits (0 x NaN):
// every wave writes zeros over the V half of its ring once, before its first
// load. From then on a V row holds zeros, or a row of V that a load left there,
// or zeros that a clipped load wrote: finite in every case, so p = 0 gives 0.
// K's half may hold anything; its masked scores are replaced, not multiplied.
//
// Merge. After its loop a wave waits for vmcnt(0) (its last, clipped stage) and
// writes O^T, m and the quad's sum of l over the start of its own ring, which
// nobody else touches; one barrier, the only one behind the start stamp's;
// then thread (w, l) merges for accumulators 2 w and 2 w + 1 the four parts
// under the workgroup's maximum (attn_weight: a part or a whole split without
// a key weighs 0 and leaves m = -inf, l = 0, O = 0) and stores the split's
// unnormalised f32 O, 8 KiB in the order [u][lane][4] of the accumulators (d =
// 16 u + 4 (lane >> 4) + i, query lane & 15), and (m, l), 16 floats each, at
// workgroup g of the workspace, which is [pass][head][split].
// tenant_attention_decode_combine_kernel, launched right behind on the same
// stream, merges the splits.
//
// Barriers. stamp_start's, the merge's and stamp_end's: all outside the loop
// and outside every branch, reached by every wave whatever its tile count.
//
// Bounds. head < heads, split < splits from blockIdx.x < passes x heads x
// splits. Loads: descriptor of len x 256 bytes at the head's K or V, len <= seq,
// inside the buffer; an offset is below (seq + 128) x 256 < 2^24 or has bit 31
// set, and the hardware clips both beyond len. LDS handed to a load: wave x
// ring + stage x 16 KiB + operand x 8 KiB + n x 1 KiB + 16 lane + 15, inside the
// wave's ring, wave-uniform. Fragment reads: row < 32, position < 16 of a
// tile. The merge's 8 KiB + 128 bytes fit the smallest ring, 16 KiB. Q: row
// head x 16 + r. Workspace: 2048 floats and 32 floats at blockIdx.x, 64-bit.
//
// Stamps and clocks are the gemm kinds' (clocked_end).
//
// hipcc -O3 for gfx950 reports (-Rpass-analysis=kernel-resource-usage) 96
// VGPRs, 32 AGPRs, 46 SGPRs, no scratch and no spills, 131072 bytes of LDS and
// an occupancy of 1 wave per SIMD at depth 2; 96 VGPRs, no AGPRs, 58 SGPRs,
// 65536 bytes and 2 waves per SIMD at depth 1. On the card the default window
// streams 5.53-5.56 TB/s on the whole card (0.78 of a streamer's 7.09 in the
// same run) and 4.17-4.26 on half of it (0.68-0.69 of 6.16) at depth 2, and
// 5.32-5.39 and 4.57-4.67 (0.75 and 0.74-0.76) at depth 1: depth 2 is the
// default for the whole card's sake, and half a card would rather have depth
// 1's eight waves per CU (profiles/attention_decode_cotenancy_results.md).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"  // m0 is clobbered on purpose
__device__ inline void attn_dma(int4v rsrc, const int4v* lds, uint32_t lane_off) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
               :
               : "s"(static_cast<uint32_t>(reinterpret_cast<uintptr_t>((LdsPtr)lds))),
                 "v"(lane_off), "s"(rsrc)
               : "memory", "m0");
}

__global__ void __launch_bounds__(kBlock, kAdDepth == 1 ? 2 : 1)
tenant_attention_decode_kernel(const int4v* __restrict__ q, const int4v* __restrict__ k,
                               const int4v* __restrict__ v, f32x4* __restrict__ ws_o,
                               float* __restrict__ ws_ml, uint32_t heads, uint32_t seq,
                               uint32_t splits, uint32_t span,
                               unsigned long long* __restrict__ rec,
                               unsigned long long* __restrict__ clk) {
  __shared__ int4v ring[kWavesPerGroup][kAdDepth][2][kAdTileVecs];  // [wave][stage][K, V]
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = lane & 15u, g = lane >> 4;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const uint32_t split = blockIdx.x % splits, head = blockIdx.x / splits % heads;
  const uint32_t len = attn_decode_len(head, seq);
  const uint32_t key0 = 128 * span * split;
  const uint32_t live = key0 < len ? min(128 * span, len - key0) : 0u;
  const uint32_t tiles = (live + kAdKeys - 1) / kAdKeys;
  const uint32_t count = tiles > wave ? (tiles - wave + 3) / 4 : 0u;  // this wave's tiles
  const uint64_t head_vecs = static_cast<uint64_t>(seq) * kAttnRowVecs;
  const auto window = [&](const int4v* first) {
    const uint64_t base = reinterpret_cast<uint64_t>(first);
    return int4v{static_cast<int>(static_cast<uint32_t>(base)),
                 static_cast<int>(static_cast<uint32_t>(base >> 32) & 0xFFFFu),
                 static_cast<int>(len * 256u), kBufferWord3};
  };
  const auto rk = window(k + head * head_vecs);
  const auto rv = window(v + head * head_vecs);
  // What this lane loads with instruction n of a stage: of row 4 n + g the
  // chunk that belongs at position r; n & 3 decides the key.
  uint32_t load_at[4];
#pragma unroll
  for (uint32_t n = 0; n < 4; ++n) load_at[n] = g * 256 + 16 * (r ^ attn_k_key(4 * n + g));
  // What it reads: of a K tile rows 16 t + r at chunk (4 s + g) ^ key; of a V
  // tile row 4 g + (r >> 2) (+ 16 x), chunk 2 u + ((r >> 1) & 1) under that
  // row's key, bytes 8 (r & 1) .. + 7 of it.
  const uint32_t read_k = r * kAttnRowVecs, read_key = attn_k_key(r);
  const uint32_t v_row = 4 * g + (r >> 2);
  const uint32_t read_v = v_row * 256 + 8 * (r & 1u);
  const uint32_t v_key = ((r >> 1) & 1u) ^ attn_k_key(v_row);

  // The 16 loads of this wave's tile `at` into stage `to`.
  const auto issue = [&](const int4v (*to)[kAdTileVecs], uint32_t at)
      __attribute__((always_inline)) {
    const uint32_t outside = at < count ? 0u : kBufferOutside;
    const uint32_t tile_off = (key0 + kAdKeys * (wave + 4 * at)) * 256;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    uint32_t off[kAdLoads];
#pragma unroll
    for (uint32_t n = 0; n < kAdLoads; ++n) off[n] = (load_at[n & 3] + tile_off + 1024 * n) | outside;
#pragma unroll
    for (int n = 0; n < kAdLoads; ++n) attn_dma(rk, to[0] + 64 * n, off[n]);
#pragma unroll
    for (int n = 0; n < kAdLoads; ++n) attn_dma(rv, to[1] + 64 * n, off[n]);
  };

  bf16x8 qf[4];
  f32x4 out[8];
  float m = -__builtin_inff(), l = 0.0f;
  // One tile: scores, online softmax, output.
  const auto step = [&](const int4v (*from)[kAdTileVecs], uint32_t at)
      __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kAdLoads + 2 * kAdLoads * (kAdDepth - 1)) : "memory");
    f32x4 s[2] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll
    for (uint32_t sub = 0; sub < 4; ++sub) {
      const uint32_t c = (4 * sub + g) ^ read_key;
#pragma unroll
      for (uint32_t t = 0; t < 2; ++t) {
        const bf16x8 kf = __builtin_bit_cast(bf16x8, from[0][read_k + 16 * kAttnRowVecs * t + c]);
        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[sub], s[t], 0, 0, 0);
      }
    }
    const uint32_t first = kAdKeys * (wave + 4 * at);  // within the split
    if (first + kAdKeys > live) {  // the split's last tile: keys at or beyond len
#pragma unroll
      for (uint32_t t = 0; t < 2; ++t)
#pragma unroll
        for (uint32_t reg = 0; reg < 4; ++reg)
          if (first + 16 * t + 4 * g + reg >= live) s[t][reg] = -__builtin_inff();
    }
    float top = s[0][0];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) top = __builtin_fmaxf(top, s[t][reg]);
    const float m_new = __builtin_fmaxf(m, attn_quad<true>(top));  // finite: a live key
    const float alpha = __builtin_amdgcn_exp2f((m - m_new) * kAttnScale);
    m = m_new;
    bf16x8 p;  // slot 4 t + reg
    float sum = 0.0f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float e = __builtin_amdgcn_exp2f((s[t][reg] - m) * kAttnScale);
        sum += e;
        p[4 * t + reg] = static_cast<__bf16>(e);
      }
    l = l * alpha + sum;
#pragma unroll
    for (int u = 0; u < 8; ++u) out[u] *= alpha;
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * kAdLoads * (kAdDepth - 1)) : "memory");
    const char* tile_v = reinterpret_cast<const char*>(from[1]);
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) {
      short4v half[2];
#pragma unroll
      for (uint32_t x = 0; x < 2; ++x)
        half[x] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) short4v*)(tile_v + read_v + 16 * ((2 * u) ^ v_key) +
                                                         16 * x * 256));
      const short8 vf = __builtin_shufflevector(half[0], half[1], 0, 1, 2, 3, 4, 5, 6, 7);
      out[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vf), p, out[u],
                                                       0, 0, 0);
    }
  };

  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  const unsigned long long t0 = stamp_start();
  const int4v* pq = q + (static_cast<uint64_t>(head) * kAdQueries + r) * kAttnRowVecs + g;
#pragma unroll
  for (int sub = 0; sub < 4; ++sub) qf[sub] = __builtin_bit_cast(bf16x8, pq[4 * sub]);
#pragma unroll
  for (int u = 0; u < 8; ++u) out[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int stage = 0; stage < kAdDepth; ++stage)  // V's half of the ring, once
#pragma unroll
    for (int n = 0; n < kAdLoads; ++n) ring[wave][stage][1][64 * n + lane] = int4v{0, 0, 0, 0};
  // Q is in its registers here, and the compiler knows it: it counts its own
  // loads only, so a wait for Q that it placed at the first use, inside the
  // loop, would be a wait for the stage just issued in every step.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("" : "+v"(qf[0]), "+v"(qf[1]), "+v"(qf[2]), "+v"(qf[3]));
  for (uint32_t i = 0; i + 1 < kAdDepth; ++i) issue(ring[wave][i], i);
  for (uint32_t i = 0; i < count; ++i) {
    issue(ring[wave][(i + kAdDepth - 1) % kAdDepth], i + kAdDepth - 1);
    step(ring[wave][i % kAdDepth], i);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clipped stage past the last

  // The wave's part over the start of its ring: O^T as [u][lane] f32x4, then m
  // and l per query.
  l = attn_quad<false>(l);
  f32x4* part = reinterpret_cast<f32x4*>(&ring[0][0][0][0]);
  constexpr int kPartVecs = sizeof(ring[0]) / 16;  // one wave's ring
#pragma unroll
  for (int u = 0; u < 8; ++u) part[wave * kPartVecs + 64 * u + lane] = out[u];
  if (g == 0) {
    float* ml = reinterpret_cast<float*>(part + wave * kPartVecs + 512);
    ml[r] = m;
    ml[kAdQueries + r] = l;
  }
  __syncthreads();
  float weight[kWavesPerGroup], top = -__builtin_inff(), sum = 0.0f;
#pragma unroll
  for (int j = 0; j < kWavesPerGroup; ++j)
    top = __builtin_fmaxf(top, reinterpret_cast<const float*>(part + j * kPartVecs + 512)[r]);
#pragma unroll
  for (int j = 0; j < kWavesPerGroup; ++j) {
    const float* ml = reinterpret_cast<const float*>(part + j * kPartVecs + 512);
    weight[j] = attn_weight(ml[r], top);
    sum += weight[j] * ml[kAdQueries + r];
  }
  const uint64_t group = blockIdx.x;
#pragma unroll
  for (uint32_t u = 2 * wave; u < 2 * wave + 2; ++u) {
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < kWavesPerGroup; ++j) acc += weight[j] * part[j * kPartVecs + 64 * u + lane];
    ws_o[group * (kAdSplitFloats / 4) + 64 * u + lane] = acc;
  }
  if (threadIdx.x < kAdQueries) {
    ws_ml[group * (2 * kAdQueries) + r] = top;
    ws_ml[group * (2 * kAdQueries) + kAdQueries + r] = sum;
  }
  clocked_end(rec, clk, c0, t0);
}
#pragma clang diagnostic pop

// Merges the splits of a head: workgroup n of passes x heads reads the `splits`
// parts of (pass, head) n from the workspace, thread (w, lane) the same
// accumulators 2 w and 2 w + 1 at the same lane as in the main kernel's merge,
// weighs them under the head's maximum (attn_weight; split 0 always has a key,
// len >= seq - 127 >= 1, so the sum is positive), divides by the sum and stores
// O as bf16, [pass][head][16][128]: query lane & 15, d = 16 u + 4 (lane >> 4) +
// 0..3, one 8-byte store. It runs for one split too: one code path. Its stamps
// go to the launch's record, which is a minimum and a maximum and so spans
// both kernels; it adds nothing to the clock words. No barrier but the
// stamps'. Every index is 64-bit and below passes x heads x splits x 2048 (or
// x 32) of the workspace, and n x 2048 + 2047 of O.
__global__ void __launch_bounds__(kBlock)
tenant_attention_decode_combine_kernel(const f32x4* __restrict__ ws_o,
                                       const float* __restrict__ ws_ml,
                                       short4v* __restrict__ o, uint32_t splits,
                                       unsigned long long* __restrict__ rec) {
  const unsigned long long t0 = stamp_start();
  const uint32_t lane = threadIdx.x & 63u, r = lane & 15u, g = lane >> 4;
  const uint32_t wave = threadIdx.x / 64;
  const uint64_t first = static_cast<uint64_t>(blockIdx.x) * splits;
  float top = -__builtin_inff(), sum = 0.0f;
  for (uint32_t s = 0; s < splits; ++s)
    top = __builtin_fmaxf(top, ws_ml[(first + s) * (2 * kAdQueries) + r]);
  f32x4 acc[2] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
  for (uint32_t s = 0; s < splits; ++s) {
    const float* ml = ws_ml + (first + s) * (2 * kAdQueries);
    const float weight = attn_weight(ml[r], top);
    sum += weight * ml[kAdQueries + r];
#pragma unroll
    for (uint32_t x = 0; x < 2; ++x)
      acc[x] += weight * ws_o[(first + s) * (kAdSplitFloats / 4) + 64 * (2 * wave + x) + lane];
  }
  const float scale = 1.0f / sum;
#pragma unroll
  for (uint32_t x = 0; x < 2; ++x) {
    short4v four;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      four[j] = __builtin_bit_cast(short, static_cast<__bf16>(acc[x][j] * scale));
    o[(static_cast<uint64_t>(blockIdx.x) * kAdSplitFloats + r * kAttnDim + 16 * (2 * wave + x) +
       4 * g) / 4] = four;
  }
  stamp_end(rec, t0);
}

// What the reference kernel adds up through LDS: the block's maximum, the
// last operand winning when it is not a number so that one is never lost, or
// its sum. Every thread gets the result.
template <bool kMax>
__device__ inline double attn_reduce(double* red, double x) {
  __syncthreads();  // red is free again
  red[threadIdx.x] = x;
  __syncthreads();
  for (uint32_t width = kBlock / 2; width > 0; width >>= 1) {
    if (threadIdx.x < width) {
      const double a = red[threadIdx.x], b = red[threadIdx.x + width];
      red[threadIdx.x] = kMax ? ((b > a || b != b) ? b : a) : a + b;
    }
    __syncthreads();
  }
  return red[0];
}

__device__ inline double bf16_to_double(unsigned short bits) {
  return static_cast<double>(__uint_as_float(static_cast<uint32_t>(bits) << 16));
}

// The plain reference: workgroup b recomputes row samples[3 b + 2] of head
// samples[3 b + 1] of pass samples[3 b] in fp64 and holds the kernel's O
// against it. Scores of keys 0 .. row (one key per thread at a time, into the
// workgroup's own seq doubles of `scratch`), their maximum, exp and the sum,
// then thread d < 128 the weighted sum over V's column d, divided by the sum.
// With `decode` the head has q_rows = 16 rows of Q and of O and every row sees
// keys 0 .. len(head) - 1 (attn_decode_len); otherwise q_rows = seq.
// worst is the maximum over all workgroups of |O - reference|, kept as the
// bits of a non-negative double, which order as the doubles do and put a
// not-a-number above everything. Every index is below its buffer's size:
// sample < passes x heads x q_rows by construction of the samples, key <= last
// < seq.
__global__ void __launch_bounds__(kBlock)
tenant_attention_reference_kernel(const unsigned short* __restrict__ q,
                                  const unsigned short* __restrict__ k,
                                  const unsigned short* __restrict__ v,
                                  const unsigned short* __restrict__ o,
                                  const uint32_t* __restrict__ samples, uint32_t heads,
                                  uint32_t q_rows, uint32_t seq, bool decode,
                                  double* __restrict__ scratch,
                                  unsigned long long* __restrict__ worst) {
  __shared__ double red[kBlock];
  const uint32_t pass = samples[3 * blockIdx.x], head = samples[3 * blockIdx.x + 1];
  const uint32_t row = samples[3 * blockIdx.x + 2];
  const uint64_t head_at = static_cast<uint64_t>(head) * seq * kAttnDim;
  const uint64_t q_at = (static_cast<uint64_t>(head) * q_rows + row) * kAttnDim;
  const uint32_t last = decode ? attn_decode_len(head, seq) - 1 : row;  // < seq
  const unsigned short* qr = q + q_at;
  double* score = scratch + static_cast<uint64_t>(blockIdx.x) * seq;
  double top = -__builtin_inf();
  for (uint32_t key = threadIdx.x; key <= last; key += kBlock) {
    const unsigned short* kr = k + head_at + static_cast<uint64_t>(key) * kAttnDim;
    double dot = 0.0;
    for (int d = 0; d < kAttnDim; ++d) dot += bf16_to_double(qr[d]) * bf16_to_double(kr[d]);
    score[key] = dot / sqrt(static_cast<double>(kAttnDim));
    top = fmax(top, score[key]);
  }
  top = attn_reduce<true>(red, top);
  double sum = 0.0;
  for (uint32_t key = threadIdx.x; key <= last; key += kBlock) {
    score[key] = exp(score[key] - top);
    sum += score[key];
  }
  sum = attn_reduce<false>(red, sum);  // its barriers publish score[] to the workgroup
  double error = 0.0;
  if (threadIdx.x < kAttnDim) {
    double acc = 0.0;
    for (uint32_t key = 0; key <= last; ++key)
      acc += score[key] * bf16_to_double(v[head_at + static_cast<uint64_t>(key) * kAttnDim +
                                           threadIdx.x]);
    const uint64_t at = (static_cast<uint64_t>(pass) * heads * q_rows * kAttnDim) + q_at +
                        threadIdx.x;
    error = fabs(bf16_to_double(o[at]) - acc / sum);
  }
  error = attn_reduce<true>(red, error);
  if (threadIdx.x == 0)
    atomicMax(worst, static_cast<unsigned long long>(__double_as_longlong(error)));
}

// ---- host ------------------------------------------------------------------

enum class Kind : int {
  kFma, kStream, kCache, kChase, kMfma, kGemm, kGemmMxfp8, kGemmMxfp4, kDecodeMxfp8,
  kDecodeMxfp4, kAttention, kAttentionDecode
};
constexpr int kKinds = 12;
// What a kind shares with others: nothing (plain), form and operands (mfma),
// the bf16 GEMM, a block-scaled GEMM, the decode shape of one, attention, or
// the decode shape of that.
enum class Family : int {
  kPlain, kMfma, kGemm, kMxGemm, kDecode, kAttention, kAttentionDecode
};
// Per kind: the kind itself (the table is indexed by it), name, family, the
// form a block-scaled kind implies (kBf16 otherwise), workgroups per CU
// (chase: one, that is one wave per SIMD; the gemms and attention: none, their
// grid is the problem's), whether it reads a buffer filled beforehand, whether its
// launches carry clocks.
struct KindInfo {
  Kind kind;
  const char* name;
  Family family;
  int form, groups_per_cu;
  bool reads, clocks;
};
constexpr KindInfo kKindTable[kKinds] = {
    {Kind::kFma, "fma", Family::kPlain, kBf16, kGroupsPerCu, false, false},
    {Kind::kStream, "stream", Family::kPlain, kBf16, kGroupsPerCu, true, false},
    {Kind::kCache, "cache", Family::kPlain, kBf16, kCacheGroupsPerCu, true, false},
    {Kind::kChase, "chase", Family::kPlain, kBf16, 1, true, false},
    {Kind::kMfma, "mfma", Family::kMfma, kBf16, kMfmaGroupsPerCu, false, true},
    {Kind::kGemm, "gemm", Family::kGemm, kBf16, 0, true, true},
    {Kind::kGemmMxfp8, "gemm-mxfp8", Family::kMxGemm, kMxfp8, 0, true, true},
    {Kind::kGemmMxfp4, "gemm-mxfp4", Family::kMxGemm, kMxfp4, 0, true, true},
    {Kind::kDecodeMxfp8, "decode-mxfp8", Family::kDecode, kMxfp8, 0, true, true},
    {Kind::kDecodeMxfp4, "decode-mxfp4", Family::kDecode, kMxfp4, 0, true, true},
    {Kind::kAttention, "attention", Family::kAttention, kBf16, 0, true, true},
    {Kind::kAttentionDecode, "attention-decode", Family::kAttentionDecode, kBf16, 0, true,
     true}};
constexpr bool kind_table_in_order() {
  for (int i = 0; i < kKinds; ++i)
    if (static_cast<int>(kKindTable[i].kind) != i) return false;
  return true;
}
static_assert(kind_table_in_order(), "row i of kKindTable describes kind i");
constexpr const KindInfo& kind_info(Kind k) { return kKindTable[static_cast<int>(k)]; }

// Whether a kind is one of the GEMMs, the decode-shaped ones included, and
// whether a block-scaled one; the form of the latter is the kind's.
constexpr bool is_mxgemm(Kind k) {
  return kind_info(k).family == Family::kMxGemm || kind_info(k).family == Family::kDecode;
}
constexpr bool is_gemm(Kind k) { return kind_info(k).family == Family::kGemm || is_mxgemm(k); }
// Whether a kind is attention, in either shape: O, the reference, max_error.
constexpr bool is_attention(Kind k) {
  return k == Kind::kAttention || k == Kind::kAttentionDecode;
}

// What plan_tenant needs of a block-scaled form, from MxGemm<F>; by form.
struct MxFormInfo {
  int step_k, max_iters;
  uint64_t word_bytes;
};
template <int F>
constexpr MxFormInfo mx_form_of() {
  return {MxGemm<F>::kStepK, MxGemm<F>::kMaxIters, MxGemm<F>::kWordBytes};
}
constexpr MxFormInfo kMxFormTable[kMfmaForms] = {
    {}, {}, mx_form_of<kMxfp8>(), mx_form_of<kMxfp4>()};

// Calls fn with a block-scaled form as a compile-time constant.
template <class Fn>
void with_mx_form(int form, Fn&& fn) {
  if (form == kMxfp8) fn(std::integral_constant<int, kMxfp8>{});
  else fn(std::integral_constant<int, kMxfp4>{});
}

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
  unsigned long long cycles = 0, ticks = 0;  // mfma and gemm only
  double clock_ghz = 0.0;                    // mfma and gemm only
};

struct TenantResult {
  bool skipped = false;
  uint64_t free_bytes = 0;
  Kind kind = Kind::kFma;
  int form = kBf16;  // mfma, and the block-scaled gemms, whose kind names it
  bool lds = false;  // mfma only: operands re-read from LDS
  uint64_t lds_bytes = 0, lds_bytes_per_launch = 0;  // mfma from LDS only
  bool direct = false;  // gemm only: slabs loaded straight to LDS; sets lds_bytes too
  bool tiled = false;   // decode only: W stored in the order the waves consume it
  MaskWords applied;
  double tick_hz = 0.0;
  int workgroups = 0;
  uint64_t bytes = 0;
  int iters = 0, passes = 0;
  uint64_t nodes = 0, stride = 0;  // chase only
  int side = 0, tiles = 0;         // gemm only: tiles per side and per pass
  uint64_t m = 0, n = 0, k = 0;    // gemm only
  uint64_t scale_bytes = 0;        // block-scaled gemm only: A's and B's scale words
  uint64_t lead_bytes = 0;         // decode only: A's elements, in the buffer before W's
  uint64_t load_bytes_per_launch = 0;  // gemm and attention only
  // attention only: rows and heads, every pass's O, the reference kernel's
  // scores, the rows it recomputed and the largest |O - reference| it found
  uint64_t seq = 0, heads = 0, out_bytes = 0, scratch_bytes = 0;
  // attention-decode only: query rows per head (0: seq of them), splits of a
  // head, 128-key units per split, the splits' f32 parts
  uint64_t queries = 0, work_bytes = 0;
  int splits = 0, span = 0;
  int checked_rows = 0;
  double max_error = 0.0;
  // flops (fma, mfma, gemm, attention), bytes (stream, cache) or hops (chase)
  double work_per_launch = 0.0;
  double bytes_per_cu = 0.0;     // cache only
  std::vector<Launch> launches;
  double rate = 0.0;  // median over launches: GFLOP/s, GB/s or Ghop/s
  double ns_per_hop = 0.0;  // chase only: median over launches
  double clock_ghz = 0.0;   // mfma and gemm only: median over launches
  uint64_t checksum = 0;
  // Raw: the last launch's word per lane (fma: none; gemm: per workgroup),
  // the stamps, mfma's and gemm's clocks.
  std::vector<unsigned long long> out, recs, clks;
};

// The end of a GEMM's plan, from m, n, k and the tiles of a pass: the passes
// (0: the kind's default) clamped to the largest grid, the grid and the flops.
void plan_gemm_grid(TenantResult& r, int tiles, int passes, int default_passes) {
  r.tiles = tiles;
  if (passes <= 0) passes = default_passes;
  r.passes = std::min(passes, kGemmMaxGroups / r.tiles);
  r.workgroups = r.tiles * r.passes;
  r.work_per_launch = 2.0 * r.m * r.n * r.k * r.passes;
}

// Plan: what a call launches, from its arguments alone (no HIP call). The grid
// depends on the card, never on the mask: the same work either way. (To a
// process started under ROC_GLOBAL_CU_MASK the runtime reports only that mask's
// CUs, so there the grid is 32 x its own CUs; every rate is over the work launched.)
TenantResult plan_tenant(Kind kind, int cus, int iters, uint64_t bytes, int passes,
                         int form, bool lds, bool direct, bool tiled) {
  TenantResult r;
  r.kind = kind;
  r.form = is_mxgemm(kind) ? kind_info(kind).form : form;
  r.lds = lds;
  r.direct = direct;
  r.tiled = tiled;
  r.workgroups = kind_info(kind).groups_per_cu * cus;
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
    case Kind::kGemm: {
      // agent/cotenancy.py states the same rule on its own (gemm_shape).
      if (iters <= 0) iters = kGemmDefaultIters;
      r.iters = std::min(iters, kGemmMaxIters);  // steps of 64 k
      r.k = static_cast<uint64_t>(kGemmBk) * r.iters;
      if (bytes == 0) bytes = 128 * kMiB;
      const uint64_t s = bytes / (4 * r.k) / kGemmTile * kGemmTile;
      r.m = r.n = std::min<uint64_t>(std::max<uint64_t>(s, kGemmTile), kGemmMaxSide);
      r.bytes = 4 * r.m * r.k;  // A and B, two bytes an element
      r.side = static_cast<int>(r.m / kGemmTile);
      plan_gemm_grid(r, r.side * r.side, passes, kGemmDefaultPasses);
      r.load_bytes_per_launch =
          static_cast<uint64_t>(r.workgroups) * 2 * kGemmTile * r.k * 2;
      if (direct)  // the ring of slab pairs and the reduction's words
        r.lds_bytes = kGemmDirectStages * 2 * kGemmSlabVecs * 16 + kBlock * 8;
      break;
    }
    case Kind::kGemmMxfp8:
    case Kind::kGemmMxfp4: {
      // agent/cotenancy.py states the same rule on its own (gemm_shape). A
      // row of A plus one of B is 256 bytes a step in either form.
      const MxFormInfo& mx = kMxFormTable[r.form];
      if (iters <= 0) iters = 4096 / mx.step_k;
      r.iters = std::min(iters, mx.max_iters);
      r.k = static_cast<uint64_t>(mx.step_k) * r.iters;
      const uint64_t s = bytes == 0 ? kMxGemmDefaultSide
                                    : bytes / (256ULL * r.iters) / kGemmTile * kGemmTile;
      r.m = r.n = std::min<uint64_t>(std::max<uint64_t>(s, kGemmTile), kGemmMaxSide);
      r.bytes = 256 * r.m * r.iters;
      r.scale_bytes = 2 * r.m * r.iters * mx.word_bytes;
      r.side = static_cast<int>(r.m / kGemmTile);
      plan_gemm_grid(r, r.side * r.side, passes, kMxGemmDefaultPasses[r.form]);
      // Per workgroup and step two slabs of 16 KiB, and per wave the words of
      // its 64 rows of A and 64 of B (lanes r and r + 32 ask for the same one).
      r.load_bytes_per_launch =
          static_cast<uint64_t>(r.workgroups) * r.iters *
          (2 * kGemmSlabVecs * 16 + kWavesPerGroup * kGemmTile * mx.word_bytes);
      break;
    }
    case Kind::kDecodeMxfp8:
    case Kind::kDecodeMxfp4: {
      // agent/cotenancy.py states the same rule on its own (decode_shape). A
      // row is 128 bytes a step in either form.
      const MxFormInfo& mx = kMxFormTable[r.form];
      if (iters <= 0) iters = kDecodeDefaultK / mx.step_k;
      r.iters = std::min(iters, mx.max_iters);
      r.k = static_cast<uint64_t>(mx.step_k) * r.iters;
      if (bytes == 0) bytes = kGiB;  // more than the Infinity Cache holds
      const uint64_t n = bytes / (128ULL * r.iters) / kGemmTile * kGemmTile;
      r.m = kDecodeRows;
      r.n = std::min<uint64_t>(std::max<uint64_t>(n, kGemmTile), kDecodeMaxN);
      r.bytes = 128 * r.n * r.iters;  // W's elements
      r.lead_bytes = 128ULL * kDecodeRows * r.iters;
      r.scale_bytes = (kDecodeRows + r.n) * r.iters * mx.word_bytes;
      plan_gemm_grid(r, static_cast<int>(r.n / kGemmTile), passes, kDecodeDefaultPasses[r.form]);
      // Per workgroup and step 16 KiB of W, the 4 KiB slab of A, and per wave
      // the words of its 32 rows of W and of the 32 of A.
      r.load_bytes_per_launch =
          static_cast<uint64_t>(r.workgroups) * r.iters *
          (kGemmTile * 128 + kDecodeRows * 128 + 2 * kWavesPerGroup * kDecodeRows * mx.word_bytes);
      break;
    }
    case Kind::kAttention: {
      // agent/cotenancy.py states the same rule on its own (attention_shape).
      // A row of Q plus one of K plus one of V is 768 bytes.
      if (iters <= 0) iters = kAttnDefaultIters;
      r.iters = std::min(iters, kAttnMaxIters);  // query tiles of 128 rows
      r.seq = static_cast<uint64_t>(kAttnRows) * r.iters;
      const uint64_t heads = bytes == 0 ? kAttnDefaultHeads : bytes / (768 * r.seq);
      r.heads = std::min<uint64_t>(std::max<uint64_t>(heads, 1), kAttnMaxHeads);
      r.bytes = 768 * r.seq * r.heads;
      // The GEMMs' clamp of passes and their grid, with heads x query tiles as
      // the "tiles" of a pass (nothing divides by r.tiles here: r.out stays
      // empty); the flops it leaves are for m = n = k = 0 and are set below.
      plan_gemm_grid(r, static_cast<int>(r.heads) * r.iters, passes, kAttnDefaultPasses);
      r.out_bytes = 256 * r.seq * r.heads * r.passes;
      const uint64_t rows = r.seq * r.heads * r.passes;
      r.checked_rows = static_cast<int>(std::min<uint64_t>(rows, kAttnSamples));
      r.scratch_bytes = r.checked_rows * r.seq * sizeof(double);
      // Two flops for Q K^T and two for P V per pair (row, key <= row); the
      // masked half of a diagonal tile is issued but not counted.
      r.work_per_launch = 4.0 * kAttnDim * (0.5 * r.seq * (r.seq + 1)) * r.heads * r.passes;
      // Per workgroup on query tile qt its 128 rows of Q and 2 (qt + 1) tiles of
      // K and of V, 32 KiB each: over qt < T, T + T (T + 1) of them.
      r.load_bytes_per_launch = static_cast<uint64_t>(r.passes) * r.heads * 32768 *
                                r.iters * (r.iters + 2);
      break;
    }
    case Kind::kAttentionDecode: {
      // agent/cotenancy.py states the same rule on its own
      // (attention_decode_shape). Per head 16 rows of Q, 4096 bytes, and a row
      // of K plus one of V, 512 bytes, per key of capacity.
      if (iters <= 0) iters = kAttnDefaultIters;
      r.iters = std::min(iters, kAttnMaxIters);  // capacity in units of 128 keys
      r.seq = static_cast<uint64_t>(128) * r.iters;
      r.queries = kAdQueries;
      const uint64_t heads = bytes == 0 ? kAdDefaultHeads : bytes / (512 * r.seq + 4096);
      r.heads = std::min<uint64_t>(std::max<uint64_t>(heads, 1), kAttnMaxHeads);
      r.bytes = (512 * r.seq + 4096) * r.heads;
      // About 2048 workgroups a pass, a split no shorter than 1024 keys.
      r.splits = std::min(std::max(kAdTargetGroups / static_cast<int>(r.heads), 1),
                          (r.iters + 7) / 8);
      r.span = (r.iters + r.splits - 1) / r.splits;
      plan_gemm_grid(r, static_cast<int>(r.heads) * r.splits, passes, kAdDefaultPasses);
      r.out_bytes = 2ULL * kAdSplitFloats * r.heads * r.passes;
      r.work_bytes = static_cast<uint64_t>(r.workgroups) * (kAdSplitFloats + 2 * kAdQueries) * 4;
      const uint64_t rows = r.queries * r.heads * r.passes;
      r.checked_rows = static_cast<int>(std::min<uint64_t>(rows, kAttnSamples));
      r.scratch_bytes = r.checked_rows * r.seq * sizeof(double);
      uint64_t live = 0;  // the sum of the heads' lengths
      for (uint32_t h = 0; h < r.heads; ++h)
        live += attn_decode_len(h, static_cast<uint32_t>(r.seq));
      // Two flops for Q K^T and two for P V per pair of a query and a live key.
      r.work_per_launch = 4.0 * kAttnDim * kAdQueries * live * r.passes;
      // The live rows of K and of V once, and Q once per split's workgroup.
      r.load_bytes_per_launch = static_cast<uint64_t>(r.passes) *
                                (512 * live + 4096 * r.heads * r.splits);
      break;
    }
  }
  return r;
}

// The rows the reference kernel recomputes, as (pass, head, row) triples: all
// of them when there are no more than kAttnSamples; otherwise the first and
// the last row of head 0 in the first and in the last pass, and the rest hashed from
// the seed and the sample's index.
std::vector<uint32_t> attention_samples(const TenantResult& r, uint64_t seed) {
  // The rows of Q a head has: the decode shape's 16, else seq.
  const uint32_t seq = static_cast<uint32_t>(r.queries ? r.queries : r.seq);
  const uint32_t heads = static_cast<uint32_t>(r.heads);
  const uint32_t passes = static_cast<uint32_t>(r.passes);
  const bool all = static_cast<uint64_t>(seq) * r.heads * r.passes <= kAttnSamples;
  const uint32_t key = mix32(static_cast<uint32_t>(seed) ^ kAttnKeySalt);
  std::vector<uint32_t> out;
  for (uint32_t i = 0; i < static_cast<uint32_t>(r.checked_rows); ++i) {
    if (all) {
      out.insert(out.end(), {i / (heads * seq), i / seq % heads, i % seq});
    } else if (i < 4) {
      out.insert(out.end(), {i & 2u ? passes - 1 : 0u, 0u, i & 1u ? seq - 1 : 0u});
    } else {
      const uint32_t hash = mix32(key ^ i);
      out.insert(out.end(), {hash % passes, mix32(hash ^ 1u) % heads, mix32(hash ^ 2u) % seq});
    }
  }
  return out;
}

// The fill and one launch of an attention tenant on `stream`: Q, K and V lie
// in `buf` one behind the other, `o` takes every pass's O.
void attention_fill(hipStream_t stream, const TenantResult& r, int cus, void* buf,
                    uint64_t seed) {
  hipLaunchKernelGGL(tenant_attention_fill_kernel, dim3(kGroupsPerCu * cus), dim3(kBlock), 0,
                     stream, static_cast<int4v*>(buf), r.bytes / 16,
                     static_cast<uint32_t>(r.heads),
                     static_cast<uint32_t>(r.queries ? r.queries : r.seq),
                     static_cast<uint32_t>(r.seq),
                     mix32(static_cast<uint32_t>(seed) ^ kAttnKeySalt));
  HIP_CHECK(hipGetLastError());
}

void attention_launch(hipStream_t stream, const TenantResult& r, const void* buf, void* o,
                      unsigned long long* rec, unsigned long long* clk) {
  const auto* q = static_cast<const int4v*>(buf);
  const uint64_t operand = r.bytes / 3 / 16;
  hipLaunchKernelGGL(tenant_attention_kernel, dim3(r.workgroups), dim3(kBlock), 0, stream, q,
                     q + operand, q + 2 * operand, static_cast<short4v*>(o),
                     static_cast<uint32_t>(r.heads), static_cast<uint32_t>(r.iters), rec, clk);
  HIP_CHECK(hipGetLastError());
}

// One launch of an attention-decode tenant on `stream`: Q, K and V lie in `buf`
// one behind the other, `work` takes the splits' f32 parts and their (m, l)
// behind them, `o` every pass's O; the combine kernel follows the main one.
void attention_decode_launch(hipStream_t stream, const TenantResult& r, const void* buf,
                             void* work, void* o, unsigned long long* rec,
                             unsigned long long* clk) {
  const auto* q = static_cast<const int4v*>(buf);
  const auto* k = q + r.heads * kAdQueries * kAttnRowVecs;
  auto* ws_o = static_cast<f32x4*>(work);
  auto* ws_ml = reinterpret_cast<float*>(ws_o + static_cast<uint64_t>(r.workgroups) *
                                                    (kAdSplitFloats / 4));
  hipLaunchKernelGGL(tenant_attention_decode_kernel, dim3(r.workgroups), dim3(kBlock), 0, stream,
                     q, k, k + r.heads * r.seq * kAttnRowVecs, ws_o, ws_ml,
                     static_cast<uint32_t>(r.heads), static_cast<uint32_t>(r.seq),
                     static_cast<uint32_t>(r.splits), static_cast<uint32_t>(r.span), rec, clk);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(tenant_attention_decode_combine_kernel,
                     dim3(static_cast<uint32_t>(r.heads) * r.passes), dim3(kBlock), 0, stream,
                     ws_o, ws_ml, static_cast<short4v*>(o), static_cast<uint32_t>(r.splits), rec);
  HIP_CHECK(hipGetLastError());
}

// Run: buffers, stream, fill, one untimed launch and `launches` timed ones;
// leaves r's raw words, the launches' event_seconds and the stream's mask.
void run_planned(TenantResult& r, int cus, const MaskWords& mask, int launches,
                 uint64_t seed) {
  const dim3 grid(r.workgroups);
  // What a launch leaves: a word per lane, for gemm one per workgroup.
  const size_t lanes =
      static_cast<size_t>(r.workgroups) * (is_gemm(r.kind) ? 1 : kBlock);
  const uint64_t n16 = (r.lead_bytes + r.bytes) / 16;
  DevBuf buf, scales, out;
  Mirror recs{r.recs}, clks{r.clks};
  // One record {~0, 0} per timed launch, and one more for the warm-up.
  recs.h.assign(2 * static_cast<size_t>(launches + 1), 0ULL);
  for (size_t i = 0; i < recs.h.size(); i += 2) recs.h[i] = ~0ULL;
  if (kind_info(r.kind).reads) buf.alloc(r.lead_bytes + r.bytes);
  if (is_mxgemm(r.kind)) scales.alloc(r.scale_bytes);
  // {sum of shader cycles, sum of wall ticks} per launch, from zero.
  if (kind_info(r.kind).clocks) clks.h.assign(recs.h.size(), 0ULL);
  // attention: the rows to recompute, the reference's scores, its one word.
  DevBuf samples, scratch, work;
  std::vector<unsigned long long> worst_word;
  Mirror worst{worst_word};
  if (r.kind == Kind::kFma) {  // what a lane stores
    out.alloc(lanes * sizeof(float));
  } else if (is_attention(r.kind)) {  // every pass's O
    out.alloc(r.out_bytes);
    if (r.work_bytes) work.alloc(r.work_bytes);
    const std::vector<uint32_t> rows = attention_samples(r, seed);
    samples.alloc(rows.size() * sizeof(uint32_t));
    HIP_CHECK(hipMemcpy(samples.p, rows.data(), rows.size() * sizeof(uint32_t),
                        hipMemcpyHostToDevice));
    scratch.alloc(r.scratch_bytes);
    worst_word.assign(1, 0ULL);
    worst.copy(true);
  } else {
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
    // A launch of a block-scaled form's `kernel`: A, then B (decode: W) behind
    // A's r.m rows of 128 bytes a step; A's scale words, then B's behind them.
    const auto mx_go = [&](auto form, auto kernel, int shape, unsigned long long* rec,
                           unsigned long long* clk) {
      const auto* a = buf.as<const int4v>();
      const auto* words = scales.as<const typename MxGemm<decltype(form)::value>::Word>();
      go(grid, kernel, a, a + r.m * r.iters * kGemmRowVecs, words, words + r.m * r.iters,
         static_cast<uint32_t>(shape), static_cast<uint32_t>(r.iters), o64, rec, clk);
    };
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
        case Kind::kGemm:  // A, then B behind it
          go(grid, r.direct ? tenant_gemm_direct_kernel<kGemmDirectStages> : tenant_gemm_kernel,
             buf.as<const int4v>(), buf.as<const int4v>() + n16 / 2,
             static_cast<uint32_t>(r.side), static_cast<uint32_t>(r.iters), o64, rec,
             clks.at(2 * slot));
          break;
        case Kind::kGemmMxfp8:
        case Kind::kGemmMxfp4:
          with_mx_form(r.form, [&](auto form) {
            mx_go(form, tenant_mxgemm_kernel<decltype(form)::value>, r.side, rec,
                  clks.at(2 * slot));
          });
          break;
        case Kind::kDecodeMxfp8:
        case Kind::kDecodeMxfp4:
          with_mx_form(r.form, [&](auto form) {
            constexpr int F = decltype(form)::value;
            mx_go(form, r.tiled ? tenant_decode_kernel<F, true> : tenant_decode_kernel<F, false>,
                  r.tiles, rec, clks.at(2 * slot));
          });
          break;
        case Kind::kAttention:
          attention_launch(g.s, r, buf.p, out.p, rec, clks.at(2 * slot));
          break;
        case Kind::kAttentionDecode:
          attention_decode_launch(g.s, r, buf.p, work.p, out.p, rec, clks.at(2 * slot));
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
      case Kind::kGemm:
        go(dim3(kGroupsPerCu * cus), tenant_gemm_fill_kernel, buf.as<int4v>(), n16, r.k / 8,
           mix32(static_cast<uint32_t>(seed) ^ kGemmKeySalt));
        break;
      case Kind::kGemmMxfp8:  // elements, then the scale words; r.m and r.n rows
      case Kind::kGemmMxfp4:
      case Kind::kDecodeMxfp8:
      case Kind::kDecodeMxfp4:
        with_mx_form(r.form, [&](auto form) {
          constexpr int F = decltype(form)::value;
          go(dim3(kGroupsPerCu * cus),
             r.tiled ? tenant_mxgemm_fill_kernel<F, true> : tenant_mxgemm_fill_kernel<F>,
             buf.as<int4v>(), n16,
             static_cast<uint64_t>(r.iters) * kGemmRowVecs,
             scales.as<typename MxGemm<F>::Word>(), (r.m + r.n) * r.iters, r.m, r.n,
             mix32(static_cast<uint32_t>(seed) ^ kGemmKeySalt));
        });
        break;
      case Kind::kAttention:
      case Kind::kAttentionDecode:
        attention_fill(g.s, r, cus, buf.p, seed);
        break;
      case Kind::kFma:
      case Kind::kMfma:
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
    if (is_attention(r.kind)) {  // the last launch's O against fp64, not timed
      const auto* q = buf.as<const unsigned short>();
      const uint64_t q_rows = r.queries ? r.queries : r.seq;
      const uint64_t operand = r.heads * r.seq * kAttnDim;
      const auto* k = q + r.heads * q_rows * kAttnDim;
      go(dim3(r.checked_rows), tenant_attention_reference_kernel, q, k, k + operand,
         out.as<const unsigned short>(), samples.as<const uint32_t>(),
         static_cast<uint32_t>(r.heads), static_cast<uint32_t>(q_rows),
         static_cast<uint32_t>(r.seq), r.kind == Kind::kAttentionDecode, scratch.as<double>(),
         worst.at(0));
    }
    HIP_CHECK(hipStreamSynchronize(g.s));
    recs.copy(false);
    clks.copy(false);
    worst.copy(false);
    if (!worst_word.empty()) std::memcpy(&r.max_error, &worst_word[0], sizeof(double));
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
  if (kind_info(r.kind).clocks) {
    // mfma: every lane's fold weighted by its global index, from 1; the GEMMs:
    // every workgroup's word weighted by its pass, from 1.
    for (size_t g = 0; g < r.out.size(); ++g)
      r.checksum += (is_gemm(r.kind) ? 1 + g / r.tiles : g + 1) * r.out[g];
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
  } else if (r.kind == Kind::kChase) {
    // Every lane's end node weighted by its global index, both from 1 so
    // that neither lane 0 nor node 0 drops out.
    for (size_t g = 0; g < r.out.size(); ++g) r.checksum += (g + 1) * (r.out[g] + 1);
    for (const auto& e : r.launches) own.push_back(e.seconds * 1e9 / r.iters);
    r.ns_per_hop = median(own);
  } else {  // stream and cache; fma leaves no words
    for (unsigned long long w : r.out) r.checksum ^= w;
  }
}

TenantResult run_tenant(int device, const MaskWords& raw_mask, Kind kind, int launches,
                        int iters, uint64_t bytes, int passes, uint64_t seed, int form,
                        bool lds, bool direct, bool tiled) {
  require_device(device);
  const int cus = gpuprobe::device_cus(device);
  const MaskWords mask =
      raw_mask.empty() ? MaskWords{} : gpuprobe::fit_mask(raw_mask, cus);
  launches = std::min(std::max(launches, 1), kMaxLaunches);
  TenantResult r = plan_tenant(kind, cus, iters, bytes, passes, form, lds, direct, tiled);
  if (kind_info(kind).reads) {
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    r.free_bytes = free_b;
    if (free_b < r.lead_bytes + r.bytes + r.scale_bytes + r.out_bytes + r.scratch_bytes + r.work_bytes +
                     kGiB) {
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
         const std::string& operands, const std::string& loads, const std::string& weights) {
        const MaskWords words = gpuprobe::mask_from_python(mask);
        int k = 0;
        while (k < kKinds && kind != kKindTable[k].name) ++k;
        if (k == kKinds) {
          std::string names;  // "a", "b", ... "y" or "z"
          for (int i = 0; i < kKinds; ++i)
            names += std::string(i == 0 ? "\"" : i + 1 < kKinds ? ", \"" : " or \"") +
                     kKindTable[i].name + "\"";
          throw py::value_error("cu_tenant_run: kind must be " + names);
        }
        const bool matrix = kKindTable[k].family == Family::kMfma;  // takes form and operands
        int f = 0;
        while (f < kMfmaForms && form != kMfmaFormTable[f].name) ++f;
        if (f == kMfmaForms)
          throw py::value_error(
              "cu_tenant_run: form must be \"bf16\", \"fp8\", \"mxfp8\" or \"mxfp4\"");
        if (f != kBf16 && !matrix)
          throw py::value_error(
              "cu_tenant_run: form \"" + form + "\" needs kind \"mfma\"; of the forms "
              "\"bf16\", \"fp8\", \"mxfp8\" and \"mxfp4\" every other kind takes only "
              "\"bf16\"");
        if (operands != "registers" && operands != "lds")
          throw py::value_error(
              "cu_tenant_run: operands must be \"registers\" or \"lds\"");
        const bool lds = operands == "lds";
        if (lds && !matrix)
          throw py::value_error(
              "cu_tenant_run: operands \"lds\" needs kind \"mfma\"; of the operands "
              "\"registers\" and \"lds\" every other kind takes only \"registers\"");
        if (loads != "registers" && loads != "direct")
          throw py::value_error("cu_tenant_run: loads must be \"registers\" or \"direct\"");
        const bool direct = loads == "direct";
        if (direct && static_cast<Kind>(k) != Kind::kGemm)
          throw py::value_error(
              "cu_tenant_run: loads \"direct\" needs kind \"gemm\"; of the loads "
              "\"registers\" and \"direct\" every other kind takes only \"registers\"");
        if (weights != "rows" && weights != "tiled")
          throw py::value_error("cu_tenant_run: weights must be \"rows\" or \"tiled\"");
        const bool tiled = weights == "tiled";
        if (tiled && kKindTable[k].family != Family::kDecode)
          throw py::value_error(
              "cu_tenant_run: weights \"tiled\" needs kind \"decode-mxfp8\" or "
              "\"decode-mxfp4\"; of the weights \"rows\" and \"tiled\" every other kind takes "
              "only \"rows\"");
        TenantResult r;
        {
          py::gil_scoped_release release;
          r = run_tenant(device, words, static_cast<Kind>(k), launches, iters, bytes,
                         passes, seed, f, lds, direct, tiled);
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
        // The kind's keys; `last`: what follows the rate.
        py::dict last;
        const bool clocks = kind_info(r.kind).clocks;
        switch (kind_info(r.kind).family) {
          case Family::kPlain:
            if (r.kind == Kind::kFma) {
              d["iters"] = r.iters;
            } else if (r.kind == Kind::kStream || r.kind == Kind::kCache) {
              d["bytes"] = r.bytes;
              d["passes"] = r.passes;
              d["checksum"] = r.checksum;
              if (r.kind == Kind::kCache) d["bytes_per_cu"] = r.bytes_per_cu;
            } else {  // chase
              d["bytes"] = r.bytes;
              d["nodes"] = r.nodes;
              d["stride"] = r.stride;
              d["iters"] = r.iters;
              d["checksum"] = r.checksum;
              last["ns_per_hop"] = r.ns_per_hop;
            }
            break;
          case Family::kMfma:
            d["form"] = kMfmaFormTable[r.form].name;
            d["iters"] = r.iters;
            d["checksum"] = r.checksum;
            if (r.lds) {
              d["operands"] = operands;
              d["lds_bytes"] = r.lds_bytes;
              d["lds_bytes_per_launch"] = r.lds_bytes_per_launch;
            }
            break;
          case Family::kGemm:
          case Family::kMxGemm:
          case Family::kDecode:
            if (is_mxgemm(r.kind)) d["form"] = kMfmaFormTable[r.form].name;
            d["m"] = r.m;
            d["n"] = r.n;
            d["k"] = r.k;
            d["bytes"] = r.bytes;
            if (is_mxgemm(r.kind)) d["scale_bytes"] = r.scale_bytes;
            d["passes"] = r.passes;
            d["checksum"] = r.checksum;
            d["load_bytes_per_launch"] = r.load_bytes_per_launch;
            if (r.direct) {
              d["loads"] = loads;
              d["stages"] = kGemmDirectStages;
              d["lds_bytes"] = r.lds_bytes;
            }
            if (r.tiled) d["weights"] = weights;
            break;
          case Family::kAttention:
            d["seq"] = r.seq;
            d["heads"] = r.heads;
            d["head_dim"] = kAttnDim;
            d["bytes"] = r.bytes;
            d["out_bytes"] = r.out_bytes;
            d["passes"] = r.passes;
            d["max_error"] = r.max_error;
            d["checked_rows"] = r.checked_rows;
            d["load_bytes_per_launch"] = r.load_bytes_per_launch;
            break;
          case Family::kAttentionDecode:
            d["seq"] = r.seq;
            d["heads"] = r.heads;
            d["head_dim"] = kAttnDim;
            d["queries"] = r.queries;
            d["splits"] = r.splits;
            d["bytes"] = r.bytes;
            d["out_bytes"] = r.out_bytes;
            d["passes"] = r.passes;
            d["max_error"] = r.max_error;
            d["checked_rows"] = r.checked_rows;
            d["load_bytes_per_launch"] = r.load_bytes_per_launch;
            break;
        }
        if (clocks) last["clock_ghz"] = r.clock_ghz;
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
      py::arg("operands") = "registers", py::arg("loads") = "registers",
      py::arg("weights") = "rows",
      "One tenant's workload, stamped with the card's wall clock. `mask` as in "
      "cu_occupancy (None: a plain stream, which is what a process started "
      "under ROC_GLOBAL_CU_MASK uses); `kind` is \"fma\", \"stream\", "
      "\"cache\", \"chase\", \"mfma\", \"gemm\", \"gemm-mxfp8\", \"gemm-mxfp4\", "
      "\"decode-mxfp8\", \"decode-mxfp4\", \"attention\" or \"attention-decode\", anything "
      "else raises "
      "ValueError before the device is touched. After one untimed "
      "launch, `launches` (1..64) launches of the same work run back to back "
      "on one stream, each between its own pair of events; the grid is 32 x "
      "CUs workgroups of 256 lanes (cache: 8 x CUs, all resident at once; "
      "chase: 1 x CUs, one wave per SIMD; mfma: 8 x CUs; gemm: the problem's "
      "tiles x passes) "
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
      "gemm: a bf16 GEMM whose operands travel global memory -> LDS -> MFMA, C "
      "(M x N, f32 accumulators, never stored) = A (M x K, row-major) . B^T "
      "with B stored N x K, M = N. `iters` is the steps of 64 k, K = 64 * "
      "iters (default 64: K = 4096; clamped to 1 .. 512); `bytes` is the size "
      "of A plus B (default 128 MiB), M = bytes // (4 K) rounded down to a "
      "multiple of 128 and clamped to 128 .. 32768, and the result reports "
      "the bytes really used, 4 M K (default: M = 8192); `passes` is the "
      "whole GEMMs of one launch (default 16, clamped to 1 .. 2^22 // tiles). "
      "Refused like stream. The grid is tiles x passes workgroups, tiles = (M "
      "/ 128)^2; workgroup g computes, in pass g // tiles, the 128 x 128 tile "
      "that a fixed bijection gives g % tiles: the workgroups of one XCD "
      "(ids 8 apart) take consecutive places in a walk over the tiles in "
      "bands of 8 tile rows, column by column. Its four waves sit 2 x 2, "
      "each on 64 x 64 as for mfma, and one step is 16 "
      "v_mfma_f32_32x32x16_bf16 per wave on a 128 x 64 slab of A and one of "
      "B, 32 KiB, that the workgroup loaded with eight 16-byte loads per "
      "lane into one of two LDS buffers (rows of 128 bytes whose eight "
      "16-byte chunks are permuted by an XOR with row bits 1, 2 and 3, so "
      "that neither the ds_write_b128 of a slab nor the ds_read_b128 of a "
      "fragment has a bank conflict; 66 KiB of LDS, two workgroups per CU); "
      "the loads of the next step are in flight under the MFMAs of this one, "
      "with one barrier per step. Both matrices are written once on the same "
      "stream before anything is timed: A[m][k] = mix32(key ^ (m % 192) << 8 "
      "^ (k % 96) ^ 0xA00000) % 31 - 15, B[n][k] = mix32(key ^ (k % 96) << 8 "
      "^ (n % 192) ^ 0xB00000) % 31 - 15, key = mix32(seed32 ^ 0x47454D4D): "
      "integers, so every accumulator stays below 32768 * 225 < 2^23 and is "
      "exact. At the end every lane weighs its entries at (m, n) by (1 + m) "
      "(1 + n) modulo 2^64, the workgroup adds its lanes up through LDS and "
      "stores one word; checksum = the sum over g of (1 + g // tiles) * "
      "word(g) modulo 2^64, equal to agent/cotenancy.py's gemm_checksum only "
      "when every tile of every pass was computed exactly and once. Clocks "
      "as for mfma. The result has m, n, k, bytes, passes, checksum, "
      "load_bytes_per_launch = tiles * passes * 2 * 128 * K * 2, what the "
      "global loads ask for, work_per_launch = 2 M N K passes flops, rates "
      "in GFLOP/s, and clock_ghz per launch and as the median. It takes no "
      "form but \"bf16\" and no operands but \"registers\".\n\n"
      "gemm, `loads`: \"registers\" (the default, everything above) or "
      "\"direct\"; anything else, or \"direct\" with a kind other than "
      "\"gemm\", raises ValueError before the device is touched. With "
      "\"direct\" the same product is computed from the same buffers, but "
      "the slabs go from memory straight to LDS (buffer_load_dwordx4 ... "
      "lds, 16 bytes per lane) and pass through no register: such a load "
      "puts lane l's bytes at a wave-uniform LDS address + 16 l, so the XOR "
      "of the LDS layout is applied to the address in memory instead (the "
      "lane that lands on position p of row R fetches chunk p ^ key(R)) and "
      "the fragment reads stay as they are. LDS holds a ring of `stages` "
      "slab pairs (2 as built; 3 with GPUPROBE_GEMM_DIRECT_STAGES=3); step i "
      "issues the loads of step i + stages - 1, multiplies, waits until at "
      "most 8 (stages - 2) of its loads are outstanding and crosses one "
      "barrier, so with three stages a step's loads stay in flight across a "
      "barrier. All loads are buffer loads on a descriptor of the tile's 128 "
      "rows; past the last step they are sent outside it and read nothing. "
      "The result adds loads, stages and lds_bytes (per workgroup: stages x "
      "32 KiB + 2 KiB) after load_bytes_per_launch; with \"registers\" it "
      "has none of the three. The checksum is gemm_checksum's either way.\n\n"
      "gemm-mxfp8, gemm-mxfp4: the same GEMM block-scaled, e4m3 bytes or e2m1 "
      "nibbles (low first) under one E8M0 scale byte per row and block of 32 "
      "k; grid, tile walk, work split, LDS layout, result, checksum rule and "
      "clocks are gemm's, and neither takes a form or operands. `iters` is "
      "the steps of 128 k (mxfp8; default 32, clamped to 1 .. 256) or 256 k "
      "(mxfp4; default 16, clamped to 1 .. 64), a slab row of 128 bytes "
      "either way; `bytes` is the elements of A plus B, 2 M K or M K, that is "
      "256 M iters (0: M = 8192), M rounded down to a multiple of 128 and "
      "clamped to 128 .. 32768; `passes` defaults to 32 and 64, a default "
      "launch lasting about as long as gemm's. Elements are those of the "
      "mfma forms at A(m % 192, k % 96) and B(k % 96, n % 192) under key = "
      "mix32(seed32 ^ 0x47454D4D): mxfp8 hash % 15 - 7 with scale byte 127 + "
      "e on both sides, mxfp4 the code hash & 15 with 128 + e for A and 128 "
      "for B, e the scale bit of block (k % 96) // 32; every effective "
      "element is an integer, |a b| <= 196 and 288, so K <= 32768 and 16384 "
      "keep every sum below 2^23 and exact. The scales lie step-major, per "
      "operand [iters][M] words of 4 or 8 bytes, byte b the step's block b, "
      "so the 32 rows of a fragment are 128 or 256 contiguous bytes. A step "
      "is 8 (mxfp8) or 16 (mxfp4) v_mfma_scale_f32_32x32x64_f8f6f4 per wave; "
      "a fragment is read from LDS as chunk 4 s + h and 4 s + 2 + h (mxfp8) "
      "or 2 s + h (mxfp4) of sub-step s, conflict-free ds_read_b128 as for "
      "gemm. Two slabs are in flight: the loads of step i + 2 are issued at "
      "the top of step i into one of two register sets and written to LDS "
      "at the end of step i + 1, one barrier per step; the step's scale words "
      "go from memory to registers at the same distance, never through LDS, "
      "are shifted by 8 h once and picked per sub-step by the scale "
      "operand's op_sel. All loads are buffer loads; past the last step they "
      "are sent outside the buffer's range and read nothing. The result adds "
      "form (\"mxfp8\" or \"mxfp4\") after workgroups and scale_bytes = 2 "
      "iters M x 4 or 8 after bytes; load_bytes_per_launch = tiles * passes * "
      "iters * (32768 + 4 * 128 * 4 or 8), slabs plus every wave's scale "
      "words; the free-memory refusal counts bytes + scale_bytes; checksum "
      "equals gemm_checksum(..., form=).\n\n"
      "decode-mxfp8, decode-mxfp4: the decode shape of that block-scaled GEMM, C "
      "(32 x N, never stored) = A (32 x K) . W^T with W stored N x K and read "
      "once per pass, so that HBM and not the matrix pipe sets the pace (64 "
      "or 128 flop per byte of W). `iters` is the steps of 128 k (mxfp8; "
      "clamped to 1 .. 256) or 256 k (mxfp4; 1 .. 64), 0: K = 8192; `bytes` is "
      "W's elements, N = bytes // (128 iters) rounded down to a multiple of "
      "128 and clamped to 128 .. 2^20 (0: 1 GiB, more than the Infinity Cache "
      "holds), and the result reports the bytes really used, 128 N iters; "
      "`passes` is the whole re-reads of W in one launch (default 48 for "
      "both, a default launch lasting about as long as gemm's; clamped to 1 "
      ".. 2^22 // tiles). Elements and scales are gemm-mxfp8's and "
      "gemm-mxfp4's for A (rows 0 .. 31) and B (= W), written once before "
      "anything is timed, and the K limits are theirs. The grid is tiles x "
      "passes workgroups, tiles = N / 128, tile g % tiles in pass g // tiles, "
      "in plain order. A workgroup owns 128 rows of W over the whole K, each "
      "of its four waves 32 of them and one 32 x 32 accumulator; a step is "
      "128 bytes of every row, 2 (mxfp8) or 4 (mxfp4) "
      "v_mfma_scale_f32_32x32x64_f8f6f4 per wave. W goes from memory "
      "straight to registers in fragment layout, buffer loads on a "
      "descriptor of the tile's 128 rows, no LDS: an mxfp4 lane holds the 64 "
      "contiguous bytes 64 h .. 64 h + 63 of its row's step (blocks 4 h + s "
      "at sub-step s), an mxfp8 lane half h of each of the step's four "
      "blocks (the instruction scales a lane's low and high dwords by the "
      "scale registers of lanes r and r + 32). The 32 rows of A are shared by "
      "the four waves through LDS, 4 KiB a step in fragment order, one load "
      "and one ds_write_b128 per lane, two buffers and one barrier per step; "
      "scale words go from memory to registers. Two steps of loads are in "
      "flight per wave at five or six workgroups per CU; the loop runs whole "
      "rounds of two steps, a step past the last loading nothing (outside "
      "the buffers' range) and adding zeros. The result has the gemm kinds' "
      "keys: form, m = 32, n, k, bytes (W's elements), scale_bytes = (32 + N) "
      "iters x 4 or 8, passes, checksum = gemm_checksum(32, n, k, passes, "
      "seed, form=), load_bytes_per_launch = tiles * passes * iters * (16384 "
      "+ 4096 + 256 x 4 or 8), work_per_launch = 2 x 32 N K passes, rates in "
      "GFLOP/s and the clocks. The free-memory refusal counts A, W and the "
      "scale words. Neither takes a form, operands or loads. `weights` "
      "(\"rows\", the default, or \"tiled\"; anything else raises ValueError, "
      "as does \"tiled\" on any other kind) says how W lies in memory. "
      "\"rows\" is row-major: every lane of a weight load sits on its own row, "
      "so one wave instruction touches 32 lines of 128 bytes for 1 KiB. "
      "\"tiled\" is the layout production decode GEMMs shuffle their weights "
      "into once, offline: the same elements under the same scales, the "
      "16-byte chunks in the order a wave consumes them. A unit is 32 rows x "
      "one step, 4 KiB, units row-block-major and then by step, inside a unit "
      "[piece p][lane r + 32 h] = the chunk that lane holds as piece p of row "
      "32 block + r. A wave instruction then reads 1 KiB of consecutive "
      "addresses, 8 whole lines, and a wave's whole K is one run of iters x 4 "
      "KiB; the lane's offset is 16 x lane, the piece an immediate of 1 KiB, "
      "the step 4 KiB. The fill writes W in that order, A and the scale words "
      "stay as they are, the product and so the checksum are the same, and "
      "so is every shape and byte key; the result adds weights = \"tiled\" "
      "after load_bytes_per_launch.\n\n"
      "attention: a causal flash-attention forward pass in bf16, per head O = "
      "softmax(Q K^T / sqrt(128), causal) V with row i attending to keys 0 .. i, "
      "head dimension 128, Q, K, V and O row-major [head][row][128]: the matrix "
      "pipe and the transcendental unit busy in one wave, and K and V re-read "
      "out of the caches by every query tile of their head. `iters` is the "
      "sequence length in units of 128 rows (default 64: seq = 8192; clamped to "
      "1 .. 256); `bytes` is Q plus K plus V, heads = bytes // (768 seq) clamped "
      "to 1 .. 1024 (0: 64 heads), and the result reports the bytes really "
      "used, 768 seq heads; `passes` is the whole forward passes of one launch, "
      "each into its own O (default 8, a default launch lasting about as long "
      "as gemm's; clamped to 1 .. 2^22 // (heads iters)). "
      "O, 256 seq heads passes bytes, is reported as out_bytes and is no part "
      "of bytes; the free-memory refusal counts bytes, out_bytes and the "
      "reference's 8 seq checked_rows. The grid is passes x heads x iters "
      "workgroups; workgroup g of a pass owns the 128 query rows of tile iters "
      "- 1 - g // heads of head g % heads, the longest first, each of its four "
      "waves 32 rows. K and V come in tiles of 64 keys, 16 KiB each, from memory "
      "straight to a ring of two {K, V} pairs in LDS (the 16-byte LDS-DMA load "
      "of gemm's `loads` \"direct\", its wait and its one barrier per tile; 64 "
      "KiB, two workgroups per CU); tiles above the diagonal are never loaded, "
      "so a workgroup runs 2 (tile + 1) of them and a launch has a tail. Per "
      "tile a wave computes S^T = K Q^T, 64 keys x 32 queries, in 16 "
      "v_mfma_f32_32x32x16_bf16 with Q held in registers; a lane then holds 32 "
      "keys of one query column, so the row maximum is an in-lane one and one "
      "v_permlane32_swap. The softmax is online and in base 2, p = exp2((s - m) "
      "c) with c = log2(e) / sqrt(128) through v_exp_f32, running maximum and "
      "sum in f32; the last two tiles of a workgroup set the scores beyond the "
      "diagonal to -inf first. P is rounded to bf16 in registers and is as it "
      "stands the B operand of O^T = V^T P^T, 16 more MFMAs into a 128 x 32 "
      "accumulator; V^T comes from the row-major V tile with the transposing "
      "LDS read ds_read_b64_tr_b16, in the key order P's registers have. O is "
      "divided by the sum once and stored as bf16. Q, K and V are written once "
      "on the same stream before anything is timed: key = mix32(mix32(seed32 ^ "
      "0x4154544E) ^ which * 0x9E3779B1 ^ head), which = 0, 1, 2, and the "
      "element at [row][d] is (mix32(key ^ (row << 7 | d)) % 31 - 15) / 8, / 4 "
      "or / 16, exact in bf16, every score exact in f32, and a row's softmax "
      "weighing a few keys so that a dropped tile or a mask off by one moves "
      "the output far. The output is no integer and there is no checksum: "
      "after the timed launches a plain fp64 kernel (one workgroup a row: the "
      "scores, their maximum, exp, the sum, the weighted sum; no MFMA, no LDS "
      "tiling, no online softmax) recomputes checked_rows = min(256, passes "
      "heads seq) rows of the last launch's O, (pass, head, row) hashed from "
      "`seed` and the sample's index with rows 0 and seq - 1 of head 0 of the "
      "first and the last pass always among them, and max_error is the "
      "largest |O - reference| over their elements (agent/cotenancy.py, "
      "ATTENTION_TOLERANCE, is what it may be). Clocks as for mfma. The result "
      "has seq, heads, head_dim, bytes, out_bytes, passes, max_error, "
      "checked_rows, load_bytes_per_launch = passes heads 32768 iters (iters + "
      "2), Q once and the K and V tiles of every workgroup, work_per_launch = "
      "passes heads 4 x 128 seq (seq + 1) / 2 flops, two for Q K^T and two for P "
      "V per pair of a row and a key it sees (the masked half of a diagonal "
      "tile is issued but not counted), rates in GFLOP/s and the clocks. It "
      "takes no form, operands, loads or weights. attention_output returns "
      "every element of one pass's O.\n\n"
      "attention-decode: a decode step's attention in bf16, the 16 query rows of "
      "one step (a grouped-query group of 16, or 8 at two speculative positions) "
      "against a head's K and V, which are read from memory once per pass: O = "
      "softmax(Q K^T / sqrt(128)) V over the head's live keys, no causal mask, head "
      "dimension 128. A head is one (sequence, KV head) pair. `iters` is the "
      "capacity in units of 128 keys (default 64: seq = 8192; clamped to 1 .. "
      "256); `bytes` is Q plus K plus V, heads = bytes // (512 seq + 4096) clamped "
      "to 1 .. 1024 (0: 256 heads, 1 GiB of K and V), and the result reports the "
      "bytes really used; the buffer is Q [head][16][128], then K [head][seq][128], "
      "then V likewise, filled by attention's data rule. Head h is live for len(h) "
      "= seq - 37 h % 128 keys; the keys beyond are in memory and must not count. "
      "splits = 2048 // heads clamped to 1 .. ceil(iters / 8), span = ceil(iters / "
      "splits) units, split s owning keys [128 span s, min(128 span (s + 1), len)); "
      "`passes` is the whole steps of one launch, each into its own O (default "
      "32; clamped to 1 .. 2^22 // (heads splits)). The grid is passes x heads x "
      "splits workgroups. A split's tiles of 32 keys are dealt round to the four "
      "waves, each with a ring of its own in LDS (2 stages of 8 KiB of K and 8 KiB "
      "of V as built, 128 KiB per workgroup, one per CU; GPUPROBE_ATTN_DECODE_DEPTH=1: "
      "1 stage, two per CU), filled by the 16-byte LDS-DMA load on descriptors of "
      "the head's live rows and waited for with s_waitcnt vmcnt alone: no barrier "
      "inside the key loop. Per tile a wave computes S^T = K Q^T in 8 "
      "v_mfma_f32_16x16x32_bf16 with Q in registers, a column's maximum over four "
      "lanes with v_permlane16_swap and v_permlane32_swap, the softmax online in "
      "base 2 (a key at or beyond len scores -inf), and O^T += V^T P^T in 8 more "
      "MFMAs with V read transposed by ds_read_b64_tr_b16. After one barrier the "
      "waves' (m, l, O) are merged through LDS and stored, unnormalised f32, to a "
      "workspace [pass][head][split]; a second kernel right behind on the same "
      "stream merges the splits, divides by l and stores O as bf16, "
      "[pass][head][16][128]. Both kernels stamp the launch's record; the clocks "
      "are the first one's. Verified as attention is: checked_rows = min(256, "
      "passes heads 16) rows of the last launch's O recomputed in fp64 over keys 0 "
      ".. len - 1, max_error the largest difference. The result has seq, heads, "
      "head_dim, queries = 16, splits, bytes, out_bytes = 4096 heads passes, "
      "passes, max_error, checked_rows, load_bytes_per_launch = passes (512 x the "
      "sum of the lengths + 4096 heads splits), the live K and V once and Q once "
      "per workgroup, work_per_launch = passes 4 x 128 x 16 x the sum of the "
      "lengths flops, rates in GFLOP/s and the clocks; the free-memory refusal "
      "counts the workspace, 8320 bytes per workgroup, too. It takes no form, "
      "operands, loads or weights. attention_output(kind=\"attention-decode\") "
      "returns every element of one pass's O.\n\n"
      "Every launch records {earliest start, latest end} of wall_clock64() over "
      "all its workgroups; the clock runs at `tick_hz` "
      "(hipDeviceAttributeWallClockRate) for every process on the card. Returns "
      "{kind, [form,] applied_mask, tick_hz, workgroups, iters | [m, n, k,] bytes, "
      "[scale_bytes,] passes, (attention: seq, heads, head_dim, bytes, out_bytes, "
      "passes, max_error, checked_rows, load_bytes_per_launch, attention-decode "
      "the same with queries, splits after head_dim, in place of these "
      "and of what follows up to work_per_launch) "
      "checksum, [load_bytes_per_launch, [loads, stages, lds_bytes,] [weights,]] "
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

  m.def(
      "attention_output",
      [](int device, py::object mask, int iters, uint64_t bytes, uint64_t seed,
         const std::string& kind) {
        const MaskWords raw = gpuprobe::mask_from_python(mask);
        if (kind != "attention" && kind != "attention-decode")
          throw py::value_error(
              "attention_output: kind must be \"attention\" or \"attention-decode\"");
        const bool decode = kind == "attention-decode";
        // The plan depends on no device; the fill's grid alone takes its CUs.
        TenantResult r = plan_tenant(decode ? Kind::kAttentionDecode : Kind::kAttention, 0, iters,
                                     bytes, 1, kBf16, false, false, false);
        if (r.out_bytes > kAttnMaxOutput)
          throw py::value_error("attention_output: the output of " + std::to_string(r.heads) +
                                " heads of " + std::to_string(r.seq) + " rows is " +
                                std::to_string(r.out_bytes) + " bytes, more than 64 MiB");
        std::string o(r.out_bytes, '\0');
        {
          py::gil_scoped_release release;
          require_device(device);
          const int cus = gpuprobe::device_cus(device);
          const MaskWords words = raw.empty() ? MaskWords{} : gpuprobe::fit_mask(raw, cus);
          DevBuf buf, out, work;
          std::vector<unsigned long long> stamps{~0ULL, 0ULL, 0ULL, 0ULL};  // rec, clk
          Mirror marks{stamps};
          buf.alloc(r.bytes);
          out.alloc(r.out_bytes);
          if (decode) work.alloc(r.work_bytes);
          marks.copy(true);
          HIP_CHECK(hipDeviceSynchronize());
          StreamGuard g;
          gpuprobe::open_stream(g, words, r.applied);
          attention_fill(g.s, r, cus, buf.p, seed);
          if (decode)
            attention_decode_launch(g.s, r, buf.p, work.p, out.p, marks.at(0), marks.at(2));
          else
            attention_launch(g.s, r, buf.p, out.p, marks.at(0), marks.at(2));
          HIP_CHECK(hipStreamSynchronize(g.s));
          HIP_CHECK(hipMemcpy(o.data(), out.p, r.out_bytes, hipMemcpyDeviceToHost));
        }
        py::dict d;
        d["seq"] = r.seq;
        d["heads"] = r.heads;
        d["output"] = py::bytes(o);
        if (decode) {
          d["queries"] = r.queries;
          d["splits"] = r.splits;
        }
        return d;
      },
      py::arg("device") = 0, py::arg("mask") = py::none(), py::arg("iters") = 0,
      py::arg("bytes") = 0, py::arg("seed") = 1, py::arg("kind") = "attention",
      "What one pass of an attention tenant computes: the fill and one launch of "
      "cu_tenant_run(kind=\"attention\")'s kernel for the same `iters`, `bytes` "
      "and `seed`, one pass. Returns {seq, heads, output}, output being O as "
      "little-endian bf16, [head][row][128], 256 * seq * heads bytes; raises "
      "ValueError before the device is touched when that is more than 64 MiB. "
      "With kind \"attention-decode\" it is that kind's two kernels and the "
      "result adds queries (16) and splits; output is [head][16][128], 4096 * "
      "heads bytes. Any other kind raises ValueError.");
}
