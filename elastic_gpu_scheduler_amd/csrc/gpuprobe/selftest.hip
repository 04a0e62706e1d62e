// Deep card self-test: three probes that look where the streaming-copy
// bandwidth number cannot.
//   * hbm_pattern_test — moving-inversions data-integrity test over one large
//     allocation (write pattern / verify / write complement / verify);
//   * xcd_bandwidth — read bandwidth of each XCD separately, all running at
//     once, each workgroup finding its XCD from HW_REG_XCC_ID at run time;
//   * mfma_selftest — chains of bf16 MFMAs on exact small-integer data,
//     checked bit-for-bit against int32 arithmetic on the vector ALU.
//
// Same conventions as probe.hip: every entry point validates the device,
// bounds its sizes and iteration counts, and releases the GIL. No kernel has
// an unbounded loop, no workgroup waits on another, and every result leaves
// a kernel through ordinary vector stores or atomics.
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "common.h"

namespace py = pybind11;
using gpuprobe::DevBuf;
using gpuprobe::pattern_word;  // the test pattern: common.h
using gpuprobe::require_device;

namespace {

constexpr uint64_t kMaxXorWords = 1ULL << 28;  // 2 GiB of pattern
constexpr uint64_t kXcdSeed = 0x5EEDC0DE0BADF00DULL;
constexpr uint32_t kMfmaSeed = 0x3C6EF372u;

uint64_t pattern_xor(uint64_t seed, uint64_t first_word, uint64_t n_words) {
  if (n_words > kMaxXorWords)
    throw std::invalid_argument("pattern_xor: n_words above 2^28");
  uint64_t x = 0;
  for (uint64_t i = 0; i < n_words; ++i) x ^= pattern_word(seed, first_word + i);
  return x;
}

constexpr int kBlock = 256;  // 4 waves

// ---- HBM pattern test ----------------------------------------------------

constexpr int kMaxRecords = 16;
// Per pass: [0] mismatching words, [1] record slots claimed,
// [2 + 2s] word index, [3 + 2s] expected ^ got of record s.
constexpr int kMetaWords = 2 + 2 * kMaxRecords;

// buf[i] = {pattern(2i), pattern(2i+1)} ^ inv, one 16-byte store per element,
// grid-stride. n16 counts 16-byte elements; all indices are 64-bit.
__global__ void __launch_bounds__(kBlock)
pattern_write_kernel(ulonglong2* __restrict__ buf, uint64_t n16, uint64_t seed,
                     uint64_t inv) {
  uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
  for (; i < n16; i += stride) {
    ulonglong2 v;
    v.x = pattern_word(seed, 2 * i) ^ inv;
    v.y = pattern_word(seed, 2 * i + 1) ^ inv;
    buf[i] = v;
  }
}

__device__ inline void record_mismatch(unsigned long long* meta, uint64_t word,
                                       uint64_t diff) {
  // Look before claiming a slot: on a card with a great many bad words this
  // keeps the slot counter from taking one atomic per bad word.
  if (__hip_atomic_load(&meta[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >=
      static_cast<unsigned long long>(kMaxRecords))
    return;
  unsigned long long slot = atomicAdd(&meta[1], 1ULL);
  if (slot < static_cast<unsigned long long>(kMaxRecords)) {
    meta[2 + 2 * slot] = word;
    meta[3 + 2 * slot] = diff;
  }
}

__global__ void __launch_bounds__(kBlock)
pattern_verify_kernel(const ulonglong2* __restrict__ buf, uint64_t n16,
                      uint64_t seed, uint64_t inv, unsigned long long* meta) {
  uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
  unsigned long long bad = 0;
  for (; i < n16; i += stride) {
    const ulonglong2 v = buf[i];
    const uint64_t e0 = pattern_word(seed, 2 * i) ^ inv;
    const uint64_t e1 = pattern_word(seed, 2 * i + 1) ^ inv;
    if (v.x != e0) {
      ++bad;
      record_mismatch(meta, 2 * i, e0 ^ v.x);
    }
    if (v.y != e1) {
      ++bad;
      record_mismatch(meta, 2 * i + 1, e1 ^ v.y);
    }
  }
  if (bad) atomicAdd(&meta[0], bad);
}

int stream_grid(uint64_t n16) {
  uint64_t blocks = (n16 + kBlock - 1) / kBlock;
  return static_cast<int>(std::min<uint64_t>(std::max<uint64_t>(blocks, 1), 8192));
}

using Corruption = std::tuple<int, uint64_t, uint64_t>;  // pass, word, mask

struct PatternResult {
  bool skipped = false;
  uint64_t bytes = 0;
  uint64_t free_bytes = 0;
  uint64_t mismatches[2] = {0, 0};
  std::vector<std::tuple<int, uint64_t, uint64_t>> records;
  double seconds = 0.0;
};

constexpr uint64_t kGiB = 1ULL << 30;

PatternResult run_pattern_test(int device, uint64_t bytes, uint64_t seed,
                               const std::vector<Corruption>& corrupt) {
  require_device(device);
  bytes = std::min<uint64_t>(std::max<uint64_t>(bytes, 16), 16 * kGiB);
  bytes &= ~static_cast<uint64_t>(15);
  const uint64_t n16 = bytes / 16;
  const uint64_t n_words = bytes / 8;
  if (corrupt.size() > 64)
    throw std::invalid_argument("hbm_pattern_test: more than 64 corruptions");
  for (const auto& c : corrupt) {
    if (std::get<0>(c) < 0 || std::get<0>(c) > 1)
      throw std::invalid_argument("hbm_pattern_test: corrupt pass must be 0 or 1");
    if (std::get<1>(c) >= n_words)
      throw std::invalid_argument("hbm_pattern_test: corrupt word index out of range");
  }

  PatternResult r;
  r.bytes = bytes;
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  r.free_bytes = free_b;
  if (free_b < bytes + kGiB) {
    r.skipped = true;
    return r;
  }

  DevBuf buf, meta;
  buf.alloc(bytes);
  meta.alloc(2 * kMetaWords * sizeof(unsigned long long));
  HIP_CHECK(hipMemset(meta.p, 0, 2 * kMetaWords * sizeof(unsigned long long)));
  const dim3 grid(stream_grid(n16)), block(kBlock);
  uint64_t* words = buf.as<uint64_t>();

  for (int pass = 0; pass < 2; ++pass) {
    const uint64_t inv = pass ? ~0ULL : 0ULL;
    auto t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(pattern_write_kernel, grid, block, 0, nullptr,
                       buf.as<ulonglong2>(), n16, seed, inv);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    auto t1 = std::chrono::steady_clock::now();
    // Test hook: flip bits of single words from the host between this pass's
    // write and its verify. Not timed.
    for (const auto& c : corrupt) {
      if (std::get<0>(c) != pass) continue;
      uint64_t w = 0;
      HIP_CHECK(hipMemcpy(&w, words + std::get<1>(c), 8, hipMemcpyDeviceToHost));
      w ^= std::get<2>(c);
      HIP_CHECK(hipMemcpy(words + std::get<1>(c), &w, 8, hipMemcpyHostToDevice));
    }
    auto t2 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(pattern_verify_kernel, grid, block, 0, nullptr,
                       buf.as<ulonglong2>(), n16, seed, inv,
                       meta.as<unsigned long long>() + pass * kMetaWords);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    auto t3 = std::chrono::steady_clock::now();
    r.seconds += std::chrono::duration<double>(t1 - t0).count() +
                 std::chrono::duration<double>(t3 - t2).count();
  }

  unsigned long long host_meta[2 * kMetaWords];
  HIP_CHECK(hipMemcpy(host_meta, meta.p, sizeof(host_meta), hipMemcpyDeviceToHost));
  for (int pass = 0; pass < 2; ++pass) {
    const unsigned long long* m = host_meta + pass * kMetaWords;
    r.mismatches[pass] = m[0];
    const int n = static_cast<int>(std::min<unsigned long long>(m[1], kMaxRecords));
    for (int s = 0; s < n; ++s)
      r.records.emplace_back(pass, m[2 + 2 * s], m[3 + 2 * s]);
  }
  std::sort(r.records.begin(), r.records.end());  // by pass, then word index
  return r;
}

// ---- per-XCD read bandwidth ----------------------------------------------

// HW_REG_XCC_ID is read as a 4-bit field, so stats has 16 rows; only ids 0..7
// own a slice and read memory.
constexpr int kXccRows = 16;
constexpr int kXcdSlices = 8;
// One row per XCC id, 256 bytes: the chunk ticket sits on a line of its own,
// away from the result words.
constexpr int kRowWords = 32;
enum : int { kTicket = 0, kChunks = 16, kGroups = 17, kChecksum = 18,
             kStart = 19, kEnd = 20 };

__device__ inline uint32_t xcc_id() {
  // s_getreg_b32 hwreg(HW_REG_XCC_ID, 0, 4): id 20, offset 0, width 4.
  return __builtin_amdgcn_s_getreg((3u << 11) | 20u) & 15u;
}

__device__ inline uint64_t wave_xor(uint64_t v) {
  for (int off = 32; off > 0; off >>= 1) v ^= __shfl_xor(v, off, 64);
  return v;
}

// Each workgroup reads chunks of ITS XCD's slice only, pulling chunk numbers
// from that XCD's ticket until the slice is exhausted. chunk16 (16-byte
// elements per chunk) is a multiple of the block size.
__global__ void __launch_bounds__(kBlock)
xcd_read_kernel(const ulonglong2* __restrict__ base, uint64_t slice16,
                uint32_t chunk16, uint32_t chunks_per_slice,
                unsigned long long* __restrict__ stats) {
  __shared__ unsigned long long s_chunk;
  const uint32_t xcc = xcc_id();
  unsigned long long* row = stats + static_cast<uint64_t>(xcc) * kRowWords;
  const uint32_t tid = threadIdx.x;
  uint64_t fold = 0;
  uint32_t done = 0;
  const uint64_t t0 = wall_clock64();
  if (xcc < static_cast<uint32_t>(kXcdSlices)) {
    const ulonglong2* slice = base + static_cast<uint64_t>(xcc) * slice16;
    // At most chunks_per_slice chunks plus the one ticket that says "empty".
    for (uint32_t turn = 0; turn <= chunks_per_slice; ++turn) {
      if (tid == 0) s_chunk = atomicAdd(&row[kTicket], 1ULL);
      __syncthreads();
      const unsigned long long c = s_chunk;
      __syncthreads();
      if (c >= chunks_per_slice) break;  // uniform across the workgroup
      const ulonglong2* p = slice + c * static_cast<uint64_t>(chunk16);
#pragma unroll 8
      for (uint32_t i = tid; i < chunk16; i += kBlock) {
        const ulonglong2 v = p[i];
        fold ^= v.x ^ v.y;
      }
      ++done;
    }
  }
  // Every load has landed before the end stamp is taken.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const uint64_t t1 = wall_clock64();
  if (done) {
    fold = wave_xor(fold);
    if ((tid & 63u) == 0) atomicXor(&row[kChecksum], fold);
  }
  if (tid == 0) {
    atomicAdd(&row[kGroups], 1ULL);
    if (done) {
      atomicAdd(&row[kChunks], static_cast<unsigned long long>(done));
      atomicMin(&row[kStart], static_cast<unsigned long long>(t0));
      atomicMax(&row[kEnd], static_cast<unsigned long long>(t1));
    }
  }
}

struct XcdEntry {
  int xcc = 0;
  uint64_t workgroups = 0, chunks = 0, bytes = 0, checksum = 0;
  double seconds = 0.0, gbps = 0.0;
  bool stable = true;
};

int selftest_grid(int device) {
  int cus = 0;
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  cus = std::min(std::max(cus, 1), 1024);
  return 4 * cus;
}

std::vector<XcdEntry> run_xcd_bandwidth(int device, int slice_mib, int iters,
                                        int chunk_kib, uint64_t seed) {
  require_device(device);
  if (slice_mib <= 0) slice_mib = 128;
  if (slice_mib > 512) slice_mib = 512;
  if (iters <= 0) iters = 3;
  if (iters > 20) iters = 20;
  if (chunk_kib <= 0) chunk_kib = 256;
  const uint64_t slice_bytes = static_cast<uint64_t>(slice_mib) << 20;
  const uint64_t chunk_bytes = static_cast<uint64_t>(chunk_kib) << 10;
  // A chunk is whole passes of 256 lanes x 16 bytes, and divides the slice.
  if (chunk_bytes % (kBlock * 16) != 0 || chunk_bytes > slice_bytes ||
      slice_bytes % chunk_bytes != 0)
    throw std::invalid_argument(
        "xcd_bandwidth: chunk_kib must be a multiple of 4 that divides the slice");
  const uint64_t slice16 = slice_bytes / 16;
  const uint32_t chunk16 = static_cast<uint32_t>(chunk_bytes / 16);
  const uint32_t chunks_per_slice = static_cast<uint32_t>(slice_bytes / chunk_bytes);
  const uint64_t total_bytes = slice_bytes * kXcdSlices;

  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  if (free_b < total_bytes + kGiB)
    throw std::runtime_error("xcd_bandwidth: insufficient free device memory");
  int clock_khz = 0;
  HIP_CHECK(hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate, device));
  if (clock_khz <= 0)
    throw std::runtime_error("xcd_bandwidth: device reports no wall-clock rate");
  const double tick_s = 1.0 / (static_cast<double>(clock_khz) * 1e3);

  DevBuf buf, stats;
  buf.alloc(total_bytes);
  constexpr size_t kStatsWords = static_cast<size_t>(kXccRows) * kRowWords;
  stats.alloc(kStatsWords * sizeof(unsigned long long));
  const uint64_t n16 = total_bytes / 16;
  hipLaunchKernelGGL(pattern_write_kernel, dim3(stream_grid(n16)), dim3(kBlock), 0,
                     nullptr, buf.as<ulonglong2>(), n16, seed, 0ULL);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());

  std::vector<unsigned long long> zero(kStatsWords, 0);
  for (int x = 0; x < kXccRows; ++x) zero[x * kRowWords + kStart] = ~0ULL;
  const dim3 grid(selftest_grid(device)), block(kBlock);
  std::vector<std::vector<unsigned long long>> runs;
  int best = -1;
  unsigned long long best_span = ~0ULL;
  for (int it = 0; it < iters; ++it) {
    HIP_CHECK(hipMemcpy(stats.p, zero.data(), kStatsWords * sizeof(unsigned long long),
                        hipMemcpyHostToDevice));
    hipLaunchKernelGGL(xcd_read_kernel, grid, block, 0, nullptr,
                       buf.as<ulonglong2>(), slice16, chunk16, chunks_per_slice,
                       stats.as<unsigned long long>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<unsigned long long> h(kStatsWords);
    HIP_CHECK(hipMemcpy(h.data(), stats.p, kStatsWords * sizeof(unsigned long long),
                        hipMemcpyDeviceToHost));
    // The launch's span: first start to last end over every XCD that read.
    unsigned long long lo = ~0ULL, hi = 0;
    for (int x = 0; x < kXcdSlices; ++x) {
      if (!h[x * kRowWords + kChunks]) continue;
      lo = std::min(lo, h[x * kRowWords + kStart]);
      hi = std::max(hi, h[x * kRowWords + kEnd]);
    }
    const unsigned long long span = hi > lo ? hi - lo : ~0ULL - 1;
    if (span < best_span) {
      best_span = span;
      best = it;
    }
    runs.push_back(std::move(h));
  }

  std::vector<XcdEntry> out;
  if (best < 0) return out;
  const auto& h = runs[best];
  for (int x = 0; x < kXcdSlices; ++x) {
    const unsigned long long* row = h.data() + x * kRowWords;
    if (!row[kChunks]) continue;
    XcdEntry e;
    e.xcc = x;
    e.workgroups = row[kGroups];
    e.chunks = row[kChunks];
    e.bytes = e.chunks * chunk_bytes;
    e.checksum = row[kChecksum];
    const unsigned long long ticks =
        row[kEnd] > row[kStart] ? row[kEnd] - row[kStart] : 1;
    e.seconds = static_cast<double>(ticks) * tick_s;
    e.gbps = static_cast<double>(e.bytes) / e.seconds / 1e9;
    for (const auto& other : runs) {
      const unsigned long long* o = other.data() + x * kRowWords;
      if (o[kChunks] != row[kChunks] || o[kChecksum] != row[kChecksum])
        e.stable = false;
    }
    out.push_back(e);
  }
  return out;
}

// ---- MFMA against the vector ALU -----------------------------------------

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using short8 = __attribute__((ext_vector_type(8))) short;
using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ inline uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

// A[row][k] in -7..7 and B[k][col] in 1..7 of one (wave, iteration) tile.
// Hashed, so neither is symmetric in its two indices.
__device__ inline int a_elem(uint32_t key, uint32_t row, uint32_t k) {
  return static_cast<int>(mix32(key ^ (row << 8) ^ k ^ 0x00A00000u) % 15u) - 7;
}
__device__ inline int b_elem(uint32_t key, uint32_t k, uint32_t col) {
  return static_cast<int>(mix32(key ^ (k << 8) ^ col ^ 0x00B00000u) % 7u) + 1;
}

// Small integers are exact in bf16: the bf16 is the float's upper half.
__device__ inline short to_bf16_bits(int v) {
  return static_cast<short>(__float_as_uint(static_cast<float>(v)) >> 16);
}

constexpr int kMfmaRows = 16;  // stats rows, one per 4-bit XCC id
enum : int { kMfmaGroups = 0, kMfmaBad = 1, kMfmaRowWords = 16 };

// One wave = one 32x32 tile accumulated over `iters` 32x32x16 bf16 MFMAs.
// |a|,|b| <= 7 (8 with the control's +1), K = 16, iters <= 1024: every partial
// sum is below 2^24, so the f32 accumulator is exact and must equal the int32
// recomputation bit for bit.
__global__ void __launch_bounds__(kBlock)
mfma_check_kernel(uint32_t seed, int iters, int perturb_wg,
                  unsigned long long* __restrict__ stats) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave_in_wg = threadIdx.x >> 6;
  const uint32_t wave = blockIdx.x * (kBlock / 64) + wave_in_wg;
  const uint32_t r = lane & 31u, h = lane >> 5;
  const bool perturb = static_cast<int>(blockIdx.x) == perturb_wg &&
                       wave_in_wg == 0 && lane == 0;

  f32x16 acc;
  int ref[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    acc[i] = 0.0f;
    ref[i] = 0;
  }

  for (int it = 0; it < iters; ++it) {
    const uint32_t key = seed ^ (wave * 0x9E3779B1u) ^
                         (static_cast<uint32_t>(it) * 0x85EBCA77u);
    // MFMA operands: lane holds A[row r][k = 8h + j] and B[k = 8h + j][col r].
    short8 af, bf;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      int a = a_elem(key, r, 8 * h + j);
      if (perturb && it == 0 && j == 0) a += 1;  // A[0][0], MFMA input only
      af[j] = to_bf16_bits(a);
      bf[j] = to_bf16_bits(b_elem(key, 8 * h + j, r));
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
        __builtin_bit_cast(bf16x8, af), __builtin_bit_cast(bf16x8, bf), acc, 0, 0, 0);
    // Reference on the vector ALU: this lane's 16 outputs are column r, rows
    // (reg & 3) + 8 * (reg >> 2) + 4 * h.
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
      const int b = b_elem(key, k, r);
#pragma unroll
      for (uint32_t reg = 0; reg < 16; ++reg) {
        const uint32_t row = (reg & 3u) + 8u * (reg >> 2) + 4u * h;
        ref[reg] += a_elem(key, row, k) * b;
      }
    }
  }

  unsigned int bad = 0;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg)
    bad += __float_as_uint(acc[reg]) != __float_as_uint(static_cast<float>(ref[reg]));
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off, 64);

  unsigned long long* row = stats + static_cast<uint64_t>(xcc_id()) * kMfmaRowWords;
  if (lane == 0 && bad) atomicAdd(&row[kMfmaBad], static_cast<unsigned long long>(bad));
  if (threadIdx.x == 0) atomicAdd(&row[kMfmaGroups], 1ULL);
}

struct MfmaEntry {
  int xcc = 0;
  uint64_t workgroups = 0, mismatched = 0;
};

std::vector<MfmaEntry> run_mfma_selftest(int device, int iters, int perturb_wg) {
  require_device(device);
  if (iters <= 0) iters = 256;
  if (iters > 1024) iters = 1024;  // keeps every partial sum below 2^24
  constexpr size_t kWords = static_cast<size_t>(kMfmaRows) * kMfmaRowWords;
  DevBuf stats;
  stats.alloc(kWords * sizeof(unsigned long long));
  HIP_CHECK(hipMemset(stats.p, 0, kWords * sizeof(unsigned long long)));
  hipLaunchKernelGGL(mfma_check_kernel, dim3(selftest_grid(device)), dim3(kBlock), 0,
                     nullptr, kMfmaSeed, iters, perturb_wg,
                     stats.as<unsigned long long>());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  unsigned long long h[kWords];
  HIP_CHECK(hipMemcpy(h, stats.p, sizeof(h), hipMemcpyDeviceToHost));
  std::vector<MfmaEntry> out;
  for (int x = 0; x < kMfmaRows; ++x) {
    if (!h[x * kMfmaRowWords + kMfmaGroups]) continue;
    MfmaEntry e;
    e.xcc = x;
    e.workgroups = h[x * kMfmaRowWords + kMfmaGroups];
    e.mismatched = h[x * kMfmaRowWords + kMfmaBad];
    out.push_back(e);
  }
  return out;
}

}  // namespace

void register_selftest(py::module_& m) {
  m.attr("XCD_PATTERN_SEED") = py::int_(kXcdSeed);

  m.def("pattern_word", [](uint64_t seed, uint64_t w) { return pattern_word(seed, w); },
        py::arg("seed"), py::arg("w"),
        "Value of 8-byte word `w` of the self-test pattern (splitmix64 "
        "finaliser of seed + (w+1)*golden). Host only.");
  m.def("pattern_xor", &pattern_xor, py::arg("seed"), py::arg("first_word"),
        py::arg("n_words"), py::call_guard<py::gil_scoped_release>(),
        "XOR of pattern words [first_word, first_word + n_words); n_words at "
        "most 2^28. Host only.");

  m.def(
      "hbm_pattern_test",
      [](int device, uint64_t bytes, uint64_t seed, std::vector<Corruption> corrupt) {
        PatternResult r;
        {
          py::gil_scoped_release release;
          r = run_pattern_test(device, bytes, seed, corrupt);
        }
        py::dict d;
        d["bytes"] = r.bytes;
        if (r.skipped) {
          d["skipped"] = "insufficient free memory";
          d["free_bytes"] = r.free_bytes;
          return d;
        }
        py::list mism;
        mism.append(r.mismatches[0]);
        mism.append(r.mismatches[1]);
        d["mismatches"] = mism;
        py::list recs;
        for (const auto& rec : r.records)
          recs.append(py::make_tuple(std::get<0>(rec), std::get<1>(rec), std::get<2>(rec)));
        d["records"] = recs;
        d["seconds"] = r.seconds;
        // Two writes and two reads of the whole buffer.
        d["gbps"] = r.seconds > 0 ? 4.0 * static_cast<double>(r.bytes) / r.seconds / 1e9
                                  : 0.0;
        return d;
      },
      py::arg("device") = 0, py::arg("bytes") = 1ULL << 30, py::arg("seed") = 1,
      py::arg("corrupt") = std::vector<Corruption>{},
      "Moving-inversions data test over one allocation of `bytes` (rounded down "
      "to a multiple of 16, clamped to 16 B .. 16 GiB): pass 0 writes "
      "pattern_word(seed, w) and verifies it, pass 1 does the same with the "
      "complement. Returns {bytes, mismatches: [n0, n1], records, seconds, gbps}; "
      "records are the first 16 mismatches of each pass as (pass, word_index, "
      "expected ^ got), sorted. When less than bytes + 1 GiB is free nothing is "
      "allocated and {skipped, bytes, free_bytes} is returned.\n\n"
      "Cache rule: a line written and then read back is served on-die as long "
      "as everything touched in between fits in about 256 MiB (the Infinity "
      "Cache). Only a buffer well above that size makes the verify pass read "
      "HBM cells; the agent default is 1 GiB. Smaller sizes exercise the kernel "
      "logic and the cache hierarchy: fine for tests, meaningless as a health "
      "result.\n\n"
      "`corrupt` is a test hook: a list of (pass, word_index, xor_mask) that the "
      "host applies to single words between that pass's write and verify.");

  m.def(
      "xcd_bandwidth",
      [](int device, int slice_mib, int iters, int chunk_kib, uint64_t seed) {
        std::vector<XcdEntry> entries;
        {
          py::gil_scoped_release release;
          entries = run_xcd_bandwidth(device, slice_mib, iters, chunk_kib, seed);
        }
        py::list out;
        for (const auto& e : entries) {
          py::dict d;
          d["xcc"] = e.xcc;
          d["workgroups"] = e.workgroups;
          d["chunks"] = e.chunks;
          d["bytes"] = e.bytes;
          d["seconds"] = e.seconds;
          d["gbps"] = e.gbps;
          d["checksum"] = e.checksum;
          d["stable"] = e.stable;
          out.append(d);
        }
        return out;
      },
      py::arg("device") = 0, py::arg("slice_mib") = 128, py::arg("iters") = 3,
      py::arg("chunk_kib") = 256, py::arg("seed") = kXcdSeed,
      "Read bandwidth of each XCD, all XCDs running at once. Eight slices of "
      "slice_mib MiB (at most 512) hold the pattern of `seed`, slice x starting "
      "at word x * slice_words; slice x is read only by workgroups that find "
      "themselves on XCD x (HW_REG_XCC_ID), in chunk_kib KiB chunks handed out "
      "by a per-XCD atomic ticket. Of `iters` (at most 20) launches the fastest "
      "is reported, one entry per XCD that read at least one chunk: {xcc, "
      "workgroups, chunks, bytes, seconds, gbps, checksum, stable}. checksum is "
      "the XOR of every word read and equals pattern_xor over the slice when "
      "the slice was read exactly once; stable is false when another launch "
      "disagreed on chunks or checksum. A CPX-partitioned device reports one "
      "XCD.");

  m.def(
      "mfma_selftest",
      [](int device, int iters, int perturb_wg) {
        std::vector<MfmaEntry> entries;
        {
          py::gil_scoped_release release;
          entries = run_mfma_selftest(device, iters, perturb_wg);
        }
        py::list out;
        for (const auto& e : entries) {
          py::dict d;
          d["xcc"] = e.xcc;
          d["workgroups"] = e.workgroups;
          d["mismatched_elements"] = e.mismatched;
          out.append(d);
        }
        return out;
      },
      py::arg("device") = 0, py::arg("iters") = 256, py::arg("perturb_wg") = -1,
      "Matrix cores against the vector ALU: 4 x CU-count workgroups of 4 waves, "
      "each wave chaining `iters` (at most 1024) 32x32x16 bf16 MFMAs on exact "
      "small-integer data and comparing its tile bit for bit with an int32 "
      "recomputation. Returns per XCD {xcc, workgroups, mismatched_elements}. "
      "perturb_wg >= 0 is the negative control: wave 0 of that workgroup adds 1 "
      "to A[0][0] of its first MFMA only, which must show as exactly 32 "
      "mismatched elements.");
}
