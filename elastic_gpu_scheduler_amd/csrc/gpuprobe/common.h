// Shared between the probe's translation units (probe.hip, selftest.hip,
// cumask.hip, cotenant.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <cstdint>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#define HIP_CHECK(expr)                                                        \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      throw std::runtime_error(std::string("HIP error at " #expr ": ") +       \
                               hipGetErrorString(_e));                         \
    }                                                                          \
  } while (0)

namespace gpuprobe {

// Throws std::runtime_error unless `device` is a visible HIP device; selects
// it on success. Defined in probe.hip.
void require_device(int device);

// The test pattern (single definition, host and device): splitmix64 finaliser
// of (seed, word index). `w` indexes the buffer viewed as 8-byte words. The
// host oracle over a range of words is selftest.hip's pattern_xor.
__host__ __device__ inline uint64_t pattern_word(uint64_t seed, uint64_t w) {
  uint64_t z = seed + (w + 1) * 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// ---- small RAII so an exception mid-probe frees what the card holds --------

struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  void alloc(size_t bytes) { HIP_CHECK(hipMalloc(&p, bytes)); }
  template <typename T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

struct StreamGuard {
  hipStream_t s = nullptr;
  // Released after the destructor body, that is after the stream is gone.
  std::unique_lock<std::mutex> masked;
  StreamGuard() = default;
  StreamGuard(const StreamGuard&) = delete;
  StreamGuard& operator=(const StreamGuard&) = delete;
  ~StreamGuard() {
    if (s) (void)hipStreamDestroy(s);
  }
};

struct EventGuard {
  hipEvent_t e = nullptr;
  EventGuard() = default;
  EventGuard(const EventGuard&) = delete;
  EventGuard& operator=(const EventGuard&) = delete;
  ~EventGuard() {
    if (e) (void)hipEventDestroy(e);
  }
  void create() { HIP_CHECK(hipEventCreate(&e)); }
};

// ---- CU masks (defined in cumask.hip) --------------------------------------

// A mask as the HIP API takes it: word w bit b is CU 32 * w + b. Empty means
// "no mask" (a plain stream).
using MaskWords = std::vector<uint32_t>;

// The device's CU count; throws when it is outside 1..256.
int device_cus(int device);

// Sizes `mask` to ceil(cus / 32) words; a bit at or above `cus` is an error.
MaskWords fit_mask(const MaskWords& mask, int cus);

// Creates the stream of one probe call: masked when `mask` is non-empty, and
// then holding the process-wide masked-stream lock for as long as the guard
// lives. `applied` receives what the runtime reads back for a masked stream.
void open_stream(StreamGuard& g, const MaskWords& mask, MaskWords& applied);

// None -> empty. Otherwise a positive int with no bit at or above 256, checked
// before any HIP call (ValueError).
MaskWords mask_from_python(const pybind11::object& mask);
pybind11::object mask_to_python(const MaskWords& words);

}  // namespace gpuprobe

// Adds the deep self-test entry points (selftest.hip) to the module.
void register_selftest(pybind11::module_& m);

// Adds the CU-mask probes (cumask.hip) to the module.
void register_cumask(pybind11::module_& m);

// Adds the co-tenancy workload (cotenant.hip) to the module.
void register_cotenant(pybind11::module_& m);
