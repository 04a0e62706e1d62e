// MI355X device probe: the GPU-facing half of the node agent.
//
// The reference scheduler ecosystem relies on a node agent (elastic-gpu-agent)
// to discover devices and wire them into containers; this module is the
// MI355X-native analogue's measurement core:
//   * inventory  — per-card identity, HBM3E capacity, CU count (hip runtime);
//   * hbm_bandwidth — streaming float4 copy kernel; verifies a card is
//     healthy and delivers expected HBM3E bandwidth (~6.3 TB/s achievable on
//     a good MI355X; a sick card or wrong partition mode shows up here);
//   * p2p_* — xGMI link discovery and measured peer bandwidth, feeding the
//     scheduler's topology matrix (hop counts for locality scoring);
//   * stamp — writes a pod-unique pattern into a small device allocation and
//     verifies it, proving a bound pod's container really landed on the card
//     indexes the scheduler chose (placement verification).
// The deep card self-test (HBM pattern, per-XCD bandwidth, MFMA check) lives
// in selftest.hip, the CU-mask probes in cumask.hip, the co-tenancy workload
// in cotenant.hip; all three register into this module.
//
// All entry points are bounded in memory and time; kernels are trivial
// streaming loops sized with grid-stride so any buffer size fills the chip
// (256 CUs need >> 256 workgroups).
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <chrono>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "common.h"

namespace py = pybind11;

namespace {

// Streaming copy: dst[i] = src[i] as float4, grid-stride. 256 threads/block,
// wave64-native (4 waves per block).
__global__ void copy_f4_kernel(const float4* __restrict__ src,
                               float4* __restrict__ dst, size_t n4) {
  size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < n4; i += stride) dst[i] = src[i];
}

// Fill a buffer with a per-element pattern derived from a 64-bit tag.
__global__ void stamp_kernel(uint64_t* __restrict__ buf, size_t n, uint64_t tag) {
  size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < n; i += stride) buf[i] = tag ^ (0x9e3779b97f4a7c15ULL * (i + 1));
}

// Verify the stamp; accumulate mismatch count.
__global__ void verify_kernel(const uint64_t* __restrict__ buf, size_t n,
                              uint64_t tag, unsigned long long* mismatches) {
  size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  unsigned long long local = 0;
  for (; i < n; i += stride)
    if (buf[i] != (tag ^ (0x9e3779b97f4a7c15ULL * (i + 1)))) ++local;
  if (local) atomicAdd(mismatches, local);
}

int checked_device_count() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return 0;
  return n;
}

// Diagnostic: raw device-count call result (count, error string).
std::pair<int, std::string> hip_status() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  return {e == hipSuccess ? n : -1, hipGetErrorString(e)};
}

}  // namespace

void gpuprobe::require_device(int device) {
  int n = checked_device_count();
  if (device < 0 || device >= n)
    throw std::runtime_error("device index " + std::to_string(device) +
                             " out of range (count=" + std::to_string(n) + ")");
  HIP_CHECK(hipSetDevice(device));
}

using gpuprobe::require_device;

static py::dict device_info(int device) {
  require_device(device);
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  py::dict d;
  d["index"] = device;
  d["name"] = std::string(prop.name);
  d["gcn_arch"] = std::string(prop.gcnArchName);
  d["total_mem_bytes"] = static_cast<int64_t>(prop.totalGlobalMem);
  d["multi_processor_count"] = prop.multiProcessorCount;  // CUs
  d["warp_size"] = prop.warpSize;                          // 64 on CDNA
  d["clock_khz"] = prop.clockRate;
  d["pci_bus_id"] = prop.pciBusID;
  d["pci_device_id"] = prop.pciDeviceID;
  d["pci_domain_id"] = prop.pciDomainID;
  return d;
}

static py::list inventory() {
  py::list out;
  int n = checked_device_count();
  for (int i = 0; i < n; ++i) out.append(device_info(i));
  return out;
}

// Measured HBM bandwidth in GB/s (read + write bytes counted), bounded.
static double hbm_bandwidth(int device, int mib, int iters) {
  require_device(device);
  if (mib <= 0) mib = 256;
  if (mib > 4096) mib = 4096;  // bound the sweep: never drive the box OOM
  if (iters <= 0) iters = 10;
  if (iters > 100) iters = 100;
  size_t bytes = static_cast<size_t>(mib) * 1024 * 1024;
  size_t n4 = bytes / sizeof(float4);
  float4 *src = nullptr, *dst = nullptr;
  HIP_CHECK(hipMalloc(&src, bytes));
  HIP_CHECK(hipMalloc(&dst, bytes));
  HIP_CHECK(hipMemset(src, 1, bytes));
  dim3 block(256);
  // >> 256 workgroups to fill 256 CUs across 8 XCDs.
  dim3 grid(4096);
  hipStream_t stream;
  HIP_CHECK(hipStreamCreate(&stream));
  // Warmup.
  hipLaunchKernelGGL(copy_f4_kernel, grid, block, 0, stream, src, dst, n4);
  HIP_CHECK(hipStreamSynchronize(stream));
  auto t0 = std::chrono::steady_clock::now();
  for (int it = 0; it < iters; ++it)
    hipLaunchKernelGGL(copy_f4_kernel, grid, block, 0, stream, src, dst, n4);
  HIP_CHECK(hipStreamSynchronize(stream));
  auto t1 = std::chrono::steady_clock::now();
  HIP_CHECK(hipStreamDestroy(stream));
  HIP_CHECK(hipFree(src));
  HIP_CHECK(hipFree(dst));
  double sec = std::chrono::duration<double>(t1 - t0).count();
  double moved = 2.0 * static_cast<double>(bytes) * iters;  // read + write
  return moved / sec / 1e9;
}

// Peer-access matrix: 1 = direct peer access possible (xGMI on an OAM board).
static std::vector<std::vector<int>> p2p_access_matrix() {
  int n = checked_device_count();
  std::vector<std::vector<int>> m(n, std::vector<int>(n, 0));
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) {
      if (i == j) {
        m[i][j] = 1;
        continue;
      }
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, i, j) == hipSuccess) m[i][j] = can;
    }
  }
  return m;
}

// Hop matrix for the scheduler's Topology: 0 diag, 1 for direct peers
// (refined by hipDeviceGetP2PAttribute performance rank when available),
// 3 for non-peer pairs (routed via host).
static std::vector<std::vector<int>> xgmi_hop_matrix() {
  int n = checked_device_count();
  std::vector<std::vector<int>> m(n, std::vector<int>(n, 0));
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) {
      if (i == j) continue;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, i, j) != hipSuccess || !can) {
        m[i][j] = 3;
        continue;
      }
      int rank = 0;
      if (hipDeviceGetP2PAttribute(&rank, hipDevP2PAttrPerformanceRank, i, j) ==
          hipSuccess) {
        m[i][j] = rank <= 0 ? 1 : 1 + rank;  // rank 0 = best (direct link)
      } else {
        m[i][j] = 1;
      }
    }
  }
  return m;
}

// Measured peer-to-peer bandwidth i->j in GB/s via hipMemcpyPeerAsync.
static double p2p_bandwidth(int src_dev, int dst_dev, int mib, int iters) {
  int n = checked_device_count();
  if (src_dev < 0 || src_dev >= n || dst_dev < 0 || dst_dev >= n)
    throw std::runtime_error("p2p_bandwidth: device index out of range");
  if (mib <= 0) mib = 128;
  if (mib > 1024) mib = 1024;
  if (iters <= 0) iters = 10;
  if (iters > 100) iters = 100;
  size_t bytes = static_cast<size_t>(mib) * 1024 * 1024;
  void *src = nullptr, *dst = nullptr;
  HIP_CHECK(hipSetDevice(src_dev));
  HIP_CHECK(hipMalloc(&src, bytes));
  HIP_CHECK(hipMemset(src, 1, bytes));
  if (src_dev != dst_dev) {
    int can = 0;
    HIP_CHECK(hipDeviceCanAccessPeer(&can, src_dev, dst_dev));
    if (can) (void)hipDeviceEnablePeerAccess(dst_dev, 0);  // already-enabled is fine
  }
  HIP_CHECK(hipSetDevice(dst_dev));
  HIP_CHECK(hipMalloc(&dst, bytes));
  HIP_CHECK(hipSetDevice(src_dev));
  hipStream_t stream;
  HIP_CHECK(hipStreamCreate(&stream));
  HIP_CHECK(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  auto t0 = std::chrono::steady_clock::now();
  for (int it = 0; it < iters; ++it)
    HIP_CHECK(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  auto t1 = std::chrono::steady_clock::now();
  HIP_CHECK(hipStreamDestroy(stream));
  HIP_CHECK(hipFree(src));
  HIP_CHECK(hipSetDevice(dst_dev));
  HIP_CHECK(hipFree(dst));
  HIP_CHECK(hipSetDevice(src_dev));
  double sec = std::chrono::duration<double>(t1 - t0).count();
  return static_cast<double>(bytes) * iters / sec / 1e9;
}

// Placement verification: stamp a tag pattern on `device`, verify on-device,
// return true iff every element matches. `mib` bounded small — this runs in
// the bind/verify path.
static bool stamp(int device, uint64_t tag, int mib) {
  require_device(device);
  if (mib <= 0) mib = 16;
  if (mib > 256) mib = 256;
  size_t bytes = static_cast<size_t>(mib) * 1024 * 1024;
  size_t n = bytes / sizeof(uint64_t);
  uint64_t* buf = nullptr;
  unsigned long long* mism = nullptr;
  HIP_CHECK(hipMalloc(&buf, bytes));
  HIP_CHECK(hipMalloc(&mism, sizeof(unsigned long long)));
  HIP_CHECK(hipMemset(mism, 0, sizeof(unsigned long long)));
  dim3 block(256), grid(2048);
  hipLaunchKernelGGL(stamp_kernel, grid, block, 0, nullptr, buf, n, tag);
  hipLaunchKernelGGL(verify_kernel, grid, block, 0, nullptr, buf, n, tag, mism);
  unsigned long long host_mism = 1;
  HIP_CHECK(hipMemcpy(&host_mism, mism, sizeof(host_mism), hipMemcpyDeviceToHost));
  HIP_CHECK(hipFree(buf));
  HIP_CHECK(hipFree(mism));
  return host_mism == 0;
}

PYBIND11_MODULE(_gpuprobe, m) {
  m.doc() = "MI355X (gfx950) device probe: inventory, HBM/xGMI bandwidth, placement stamp";
  m.def("device_count", &checked_device_count);
  m.def("hip_status", [] {
    auto s = hip_status();
    return py::make_tuple(s.first, s.second);
  });
  m.def("device_info", &device_info, py::arg("device"));
  m.def("inventory", &inventory);
  m.def("hbm_bandwidth", &hbm_bandwidth, py::arg("device") = 0, py::arg("mib") = 256,
        py::arg("iters") = 10, py::call_guard<py::gil_scoped_release>());
  m.def("p2p_access_matrix", &p2p_access_matrix);
  m.def("xgmi_hop_matrix", &xgmi_hop_matrix);
  m.def("p2p_bandwidth", &p2p_bandwidth, py::arg("src") = 0, py::arg("dst") = 1,
        py::arg("mib") = 128, py::arg("iters") = 10,
        py::call_guard<py::gil_scoped_release>());
  m.def("stamp", &stamp, py::arg("device") = 0, py::arg("tag") = 0,
        py::arg("mib") = 16, py::call_guard<py::gil_scoped_release>());
  register_selftest(m);
  register_cumask(m);
  register_cotenant(m);
}
