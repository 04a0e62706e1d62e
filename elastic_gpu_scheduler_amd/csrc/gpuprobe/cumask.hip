// CU-mask probes: what a per-queue CU mask does on the card.
//   * cu_occupancy — which physical CUs (xcc, se, sh, cu) the workgroups of
//     one dispatch ran on, under a stream CU mask or on a plain stream;
//   * cu_mask_layout — how mask bits map to XCDs, learnt from an unmasked run
//     and one masked run that leaves every XCD populated whichever way the
//     bits are dealt;
//   * cu_mask_throughput — FP32 FMA rate of a fixed amount of register-resident
//     work under a mask: the number that says a share limits compute.
//
// Same conventions as selftest.hip. Every kernel runs a fixed iteration
// count, waits on nothing and leaves its results through ordinary vector
// stores. A masked stream is created, used and destroyed inside one call
// (RAII, so on the error path too), and never more than one exists at a time.
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "common.h"

namespace py = pybind11;
using gpuprobe::DevBuf;
using gpuprobe::EventGuard;
using gpuprobe::MaskWords;
using gpuprobe::StreamGuard;
using gpuprobe::device_cus;
using gpuprobe::fit_mask;
using gpuprobe::mask_from_python;
using gpuprobe::mask_to_python;
using gpuprobe::open_stream;
using gpuprobe::require_device;

// ---- shared with cotenant.hip (declared in common.h) -------------------------

namespace gpuprobe {

namespace {

// No gfx950 part has more than 256 CUs, so a mask with a bit at or above 256
// is refused before the device is even looked at.
constexpr int kMaxCus = 256;
constexpr int kMaxMaskWords = kMaxCus / 32;

}  // namespace

int device_cus(int device) {
  int cus = 0;
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  if (cus < 1 || cus > kMaxCus)
    throw std::runtime_error("cu mask probe: device reports " + std::to_string(cus) +
                             " CUs, outside 1.." + std::to_string(kMaxCus));
  return cus;
}

MaskWords fit_mask(const MaskWords& mask, int cus) {
  const size_t n_words = static_cast<size_t>((cus + 31) / 32);
  MaskWords out(n_words, 0u);
  bool any = false;
  for (size_t w = 0; w < mask.size(); ++w) {
    for (int b = 0; b < 32; ++b) {
      if (!((mask[w] >> b) & 1u)) continue;
      if (static_cast<int>(32 * w) + b >= cus)
        throw std::invalid_argument("cu mask: bit " + std::to_string(32 * w + b) +
                                    " set, device has " + std::to_string(cus) + " CUs");
      out[w] |= 1u << b;
      any = true;
    }
  }
  if (!any) throw std::invalid_argument("cu mask: no bit set");
  return out;
}

namespace {

// Held for as long as a masked stream exists: the entry points release the
// GIL, and two threads must not each hold one.
std::mutex g_masked_stream;

}  // namespace

void open_stream(StreamGuard& g, const MaskWords& mask, MaskWords& applied) {
  applied.clear();
  if (mask.empty()) {
    HIP_CHECK(hipStreamCreate(&g.s));
    return;
  }
  g.masked = std::unique_lock<std::mutex>(g_masked_stream);
  HIP_CHECK(hipExtStreamCreateWithCUMask(&g.s, static_cast<uint32_t>(mask.size()),
                                         mask.data()));
  applied.assign(mask.size(), 0u);
  HIP_CHECK(hipExtStreamGetCUMask(g.s, static_cast<uint32_t>(applied.size()),
                                  applied.data()));
}

// None -> empty. Otherwise a positive int with no bit at or above kMaxCus,
// checked here, before any HIP call; the device's own CU count is checked in
// fit_mask before anything is created or launched.
MaskWords mask_from_python(const py::object& mask) {
  if (mask.is_none()) return {};
  if (!py::isinstance<py::int_>(mask)) throw py::type_error("mask must be an int or None");
  if (mask.attr("__le__")(0).cast<bool>())
    throw py::value_error("cu mask must be positive");
  if (mask.attr("bit_length")().cast<int>() > kMaxCus)
    throw py::value_error("cu mask has a bit at or above CU " + std::to_string(kMaxCus));
  MaskWords words(kMaxMaskWords, 0u);
  for (int w = 0; w < kMaxMaskWords; ++w)
    words[w] = mask.attr("__rshift__")(32 * w).attr("__and__")(0xFFFFFFFFu).cast<uint32_t>();
  return words;
}

py::object mask_to_python(const MaskWords& words) {
  if (words.empty()) return py::none();
  py::object v = py::int_(0);
  for (size_t w = words.size(); w-- > 0;)
    v = v.attr("__lshift__")(32).attr("__or__")(py::int_(words[w]));
  return v;
}

}  // namespace gpuprobe

namespace {

// ---- occupancy -------------------------------------------------------------

constexpr int kOccBlock = 64;  // one wave
// Dynamic LDS per workgroup. It holds nothing of value: it keeps a CU (160 KiB
// of LDS) from taking more than three of these workgroups at once, so the
// grid spreads over every CU the queue may use instead of piling onto a few.
constexpr unsigned kOccLdsBytes = 48 * 1024;
constexpr int kOccRecWords = 4;  // hw_id, xcc_id, chain value, unused
constexpr uint32_t kOccUnwritten = 0xFFFFFFFFu;

__device__ inline uint32_t hw_id_reg() {
  // s_getreg_b32 hwreg(HW_REG_HW_ID, 0, 32): id 4, offset 0, width 32.
  return __builtin_amdgcn_s_getreg((31u << 11) | 4u);
}

__device__ inline uint32_t xcc_id_reg() {
  // s_getreg_b32 hwreg(HW_REG_XCC_ID, 0, 4): id 20, offset 0, width 4.
  return __builtin_amdgcn_s_getreg((3u << 11) | 20u) & 15u;
}

// Each workgroup runs a dependent chain of `work` FMAs (a few microseconds),
// then lane 0 records where it ran.
__global__ void __launch_bounds__(kOccBlock)
cu_occupancy_kernel(uint32_t* __restrict__ out, int work, float a, float b) {
  extern __shared__ float occ_lds[];
  float x = static_cast<float>(threadIdx.x) * (1.0f / kOccBlock);
  for (int i = 0; i < work; ++i) x = __builtin_fmaf(x, a, b);
  occ_lds[threadIdx.x] = x;
  if (threadIdx.x == 0) {
    uint32_t* rec = out + static_cast<size_t>(blockIdx.x) * kOccRecWords;
    rec[0] = hw_id_reg();
    rec[1] = xcc_id_reg();
    rec[2] = __float_as_uint(x);
  }
}

using CuKey = std::array<int, 4>;  // xcc, se, sh, cu

// HW_ID fields of the gfx9/CDNA ISA: cu_id [11:8], sh_id [12], se_id [15:13].
CuKey decode_cu(uint32_t hw_id, uint32_t xcc) {
  return {static_cast<int>(xcc & 15u), static_cast<int>((hw_id >> 13) & 7u),
          static_cast<int>((hw_id >> 12) & 1u), static_cast<int>((hw_id >> 8) & 15u)};
}

struct Occupancy {
  int device_cus = 0;
  std::map<CuKey, uint64_t> cus;  // workgroups per physical CU
  uint64_t workgroups = 0;        // records written
  MaskWords applied;
  double seconds = 0.0;
};

Occupancy run_occupancy(int device, const MaskWords& raw_mask, int workgroups, int work) {
  require_device(device);
  Occupancy r;
  r.device_cus = device_cus(device);
  const MaskWords mask = raw_mask.empty() ? MaskWords{} : fit_mask(raw_mask, r.device_cus);
  if (workgroups <= 0) workgroups = 16 * r.device_cus;
  workgroups = std::min(workgroups, 1 << 16);
  if (work <= 0) work = 2048;
  work = std::min(work, 1 << 16);

  const size_t words = static_cast<size_t>(workgroups) * kOccRecWords;
  DevBuf out;
  out.alloc(words * sizeof(uint32_t));
  HIP_CHECK(hipMemset(out.p, 0xFF, words * sizeof(uint32_t)));
  HIP_CHECK(hipDeviceSynchronize());
  EventGuard t0, t1;
  t0.create();
  t1.create();

  std::vector<uint32_t> h(words);
  {
    StreamGuard g;
    open_stream(g, mask, r.applied);
    HIP_CHECK(hipEventRecord(t0.e, g.s));
    hipLaunchKernelGGL(cu_occupancy_kernel, dim3(workgroups), dim3(kOccBlock),
                       kOccLdsBytes, g.s, out.as<uint32_t>(), work, 0.999f, 0.001f);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(t1.e, g.s));
    HIP_CHECK(hipStreamSynchronize(g.s));
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, t0.e, t1.e));
    r.seconds = static_cast<double>(ms) * 1e-3;
    HIP_CHECK(hipMemcpy(h.data(), out.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }  // the stream is gone before the result is looked at

  for (int wg = 0; wg < workgroups; ++wg) {
    const uint32_t* rec = h.data() + static_cast<size_t>(wg) * kOccRecWords;
    if (rec[0] == kOccUnwritten && rec[1] == kOccUnwritten) continue;
    ++r.cus[decode_cu(rec[0], rec[1])];
    ++r.workgroups;
  }
  return r;
}

// ---- layout ----------------------------------------------------------------

struct Layout {
  int cus = 0;
  int xccs = 0;
  int granule = 0;
  bool interleaved = false;
  std::vector<CuKey> lost;
};

std::map<int, int> cus_per_xcc(const std::map<CuKey, uint64_t>& cus) {
  std::map<int, int> n;
  for (const auto& kv : cus) ++n[kv.first[0]];
  return n;
}

Layout run_layout(int device) {
  Layout l;
  const Occupancy all = run_occupancy(device, {}, 0, 0);
  l.cus = all.device_cus;
  const std::map<int, int> per_xcc = cus_per_xcc(all.cus);
  l.xccs = static_cast<int>(per_xcc.size());
  l.granule = l.xccs;
  // The masked run is made only from a sound picture of the card: every CU
  // seen, the same number on every XCD, at least two per XCD.
  if (l.xccs < 1 || static_cast<int>(all.cus.size()) != l.cus ||
      l.cus % l.xccs != 0 || l.cus / l.xccs < 2)
    return l;
  for (const auto& kv : per_xcc)
    if (kv.second != l.cus / l.xccs) return l;

  // Every bit but the lowest `granule`: dealt round-robin that costs each XCD
  // one CU, in blocks per XCD it costs one XCD `granule` CUs. Either way no
  // XCD is left empty.
  MaskWords mask(static_cast<size_t>((l.cus + 31) / 32), 0u);
  for (int bit = l.granule; bit < l.cus; ++bit) mask[bit / 32] |= 1u << (bit % 32);
  const Occupancy rest = run_occupancy(device, mask, 0, 0);
  std::set<int> lost_xccs;
  for (const auto& kv : all.cus) {
    if (rest.cus.count(kv.first)) continue;
    l.lost.push_back(kv.first);
    lost_xccs.insert(kv.first[0]);
  }
  bool subset = true;
  for (const auto& kv : rest.cus) subset = subset && all.cus.count(kv.first);
  l.interleaved = subset && static_cast<int>(l.lost.size()) == l.granule &&
                  static_cast<int>(lost_xccs.size()) == l.xccs;
  return l;
}

// ---- throughput ------------------------------------------------------------

constexpr int kFmaBlock = 256;
constexpr int kFmaChains = 16;
constexpr int kFmaGroupsPerCu = 32;  // 8 resident per CU: four fills of the card

// kFmaChains independent FMA chains per lane, all in registers; every lane
// stores its sum once at the end.
__global__ void __launch_bounds__(kFmaBlock)
cu_fma_kernel(float* __restrict__ out, int iters, float a, float b) {
  float x[kFmaChains];
#pragma unroll
  for (int c = 0; c < kFmaChains; ++c)
    x[c] = static_cast<float>(threadIdx.x + c) * (1.0f / (kFmaBlock + kFmaChains));
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int c = 0; c < kFmaChains; ++c) x[c] = __builtin_fmaf(x[c], a, b);
  }
  float sum = 0.0f;
#pragma unroll
  for (int c = 0; c < kFmaChains; ++c) sum += x[c];
  out[static_cast<size_t>(blockIdx.x) * kFmaBlock + threadIdx.x] = sum;
}

struct Throughput {
  double gflops = 0.0, seconds = 0.0;
  MaskWords applied;
};

Throughput run_throughput(int device, const MaskWords& raw_mask, int iters) {
  require_device(device);
  const int cus = device_cus(device);
  const MaskWords mask = raw_mask.empty() ? MaskWords{} : fit_mask(raw_mask, cus);
  if (iters <= 0) iters = 65536;
  iters = std::min(iters, 1 << 18);
  // The grid depends on the card, never on the mask: the same work either way.
  const int grid = kFmaGroupsPerCu * cus;
  const size_t n = static_cast<size_t>(grid) * kFmaBlock;

  Throughput r;
  DevBuf out;
  out.alloc(n * sizeof(float));
  EventGuard t0, t1;
  t0.create();
  t1.create();
  StreamGuard g;
  open_stream(g, mask, r.applied);
  // Warm-up, not timed: the same launch once, so that the code object is
  // loaded and the clocks have settled under this load before the timed one.
  hipLaunchKernelGGL(cu_fma_kernel, dim3(grid), dim3(kFmaBlock), 0, g.s,
                     out.as<float>(), iters, 0.999f, 0.001f);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(t0.e, g.s));
  hipLaunchKernelGGL(cu_fma_kernel, dim3(grid), dim3(kFmaBlock), 0, g.s,
                     out.as<float>(), iters, 0.999f, 0.001f);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(t1.e, g.s));
  HIP_CHECK(hipStreamSynchronize(g.s));
  float ms = 0.0f;
  HIP_CHECK(hipEventElapsedTime(&ms, t0.e, t1.e));
  r.seconds = static_cast<double>(ms) * 1e-3;
  const double flops = 2.0 * kFmaChains * static_cast<double>(n) * iters;
  r.gflops = r.seconds > 0 ? flops / r.seconds / 1e9 : 0.0;
  return r;
}

py::tuple key_tuple(const CuKey& k) { return py::make_tuple(k[0], k[1], k[2], k[3]); }

}  // namespace

void register_cumask(py::module_& m) {
  m.def(
      "cu_occupancy",
      [](int device, py::object mask, int workgroups, int work) {
        const MaskWords words = mask_from_python(mask);
        Occupancy r;
        {
          py::gil_scoped_release release;
          r = run_occupancy(device, words, workgroups, work);
        }
        py::list cus;
        for (const auto& kv : r.cus) {  // std::map: sorted by (xcc, se, sh, cu)
          py::dict d;
          d["xcc"] = kv.first[0];
          d["se"] = kv.first[1];
          d["sh"] = kv.first[2];
          d["cu"] = kv.first[3];
          d["workgroups"] = kv.second;
          cus.append(d);
        }
        py::dict d;
        d["cus"] = cus;
        d["workgroups"] = r.workgroups;
        d["applied_mask"] = mask_to_python(r.applied);
        d["seconds"] = r.seconds;
        return d;
      },
      py::arg("device") = 0, py::arg("mask") = py::none(), py::arg("workgroups") = 0,
      py::arg("work") = 0,
      "Which physical CUs one dispatch ran on. `mask` is an int, bit i = CU i as "
      "in hipExtStreamCreateWithCUMask; None launches on a plain stream. 0, a "
      "negative value or a bit at or above the CU count raises ValueError before "
      "anything is launched. `workgroups` one-wave workgroups (default 16 x CUs, "
      "at most 65536), each holding 48 KiB of LDS so that at most three share a "
      "CU, run a dependent chain of `work` FMAs (default 2048, at most 65536) and "
      "record HW_REG_HW_ID and HW_REG_XCC_ID. Returns {cus: sorted [{xcc, se, sh, "
      "cu, workgroups}], workgroups: records written, applied_mask: what "
      "hipExtStreamGetCUMask reads back (None on a plain stream), seconds}.");

  m.def(
      "cu_mask_layout",
      [](int device) {
        Layout l;
        {
          py::gil_scoped_release release;
          l = run_layout(device);
        }
        py::list lost;
        for (const auto& k : l.lost) lost.append(key_tuple(k));
        py::dict d;
        d["cus"] = l.cus;
        d["xccs"] = l.xccs;
        d["granule"] = l.granule;
        d["interleaved"] = l.interleaved;
        d["lost"] = lost;
        return d;
      },
      py::arg("device") = 0,
      "How CU-mask bits map to XCDs. Run 1 is unmasked and counts the XCDs, g. "
      "Run 2 sets every bit but the lowest g, which leaves every XCD populated "
      "whether bits are dealt round-robin over the XCDs or in blocks per XCD; it "
      "is made only when run 1 saw every CU, equally many per XCD. Returns {cus, "
      "xccs, granule: g, interleaved, lost: [(xcc, se, sh, cu)]}; interleaved is "
      "true when run 2 lost exactly one CU on each XCD, so that any g aligned "
      "consecutive bits are one CU per XCD.");

  m.def(
      "cu_mask_throughput",
      [](int device, py::object mask, int iters) {
        const MaskWords words = mask_from_python(mask);
        Throughput r;
        {
          py::gil_scoped_release release;
          r = run_throughput(device, words, iters);
        }
        py::dict d;
        d["gflops"] = r.gflops;
        d["seconds"] = r.seconds;
        d["applied_mask"] = mask_to_python(r.applied);
        return d;
      },
      py::arg("device") = 0, py::arg("mask") = py::none(), py::arg("iters") = 65536,
      "FP32 FMA rate of a fixed amount of work under a CU mask: 32 x CUs "
      "workgroups of 256 lanes, each lane running 16 independent chains of "
      "`iters` FMAs (default 65536, at most 262144) in registers, timed with "
      "events on the (masked) stream after one untimed launch of the same work: a "
      "window of a few milliseconds measures the clocks settling, not the mask. "
      "The grid does not depend on the mask. Returns {gflops, seconds, "
      "applied_mask}.");
}
