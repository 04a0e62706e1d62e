// Shared between the probe's translation units (probe.hip, selftest.hip,
// cumask.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>

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

}  // namespace gpuprobe

// Adds the deep self-test entry points (selftest.hip) to the module.
void register_selftest(pybind11::module_& m);

// Adds the CU-mask probes (cumask.hip) to the module.
void register_cumask(pybind11::module_& m);
