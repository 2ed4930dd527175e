// gfx950 batch collation: ragged rows of several decoded shards gathered
// into padded dense tensors, all columns of a batch in ONE launch.
//
// A training batch of 8192 flagship rows is under 2 MB: its time is launches
// and host round trips, not bytes. So one kernel produces every output
// column, writes the padding and the length words itself (no fill launch per
// column), and reports errors and the truncated-row count through two status
// words the caller reads back with one copy. The semantics live in
// csrc/collate_core.h (do_unit), shared with the host path.
//
//   collate_rows_kernel   blocks take (column, tile) pairs, found through
//                         the columns' tile0 prefix in the descriptor, and
//                         grid-stride over them; consecutive lanes produce
//                         consecutive units (an 8- or 4-byte element, or one
//                         8-byte word of a byte column), so stores coalesce
//
// Reads are a gather: a lane looks up its batch row's (slot, row), then the
// slot's offsets, then the values. Lanes of one row share those loads through
// the cache. No LDS and no per-lane arrays: there is nothing to stage.
// Reference behavior being extended: the reference hands rows to Spark
// (TFRecordDeserializer.scala:21-66); dense device batches have no analog.

#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "../collate_core.h"

namespace py = pybind11;
using namespace tfrec::collate;

namespace {

#define HIPC_CHECK(expr)                                                       \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess)                                                      \
      throw std::runtime_error(std::string("HIP error: ") +                    \
                               hipGetErrorString(_e));                         \
  } while (0)

using ull = unsigned long long;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;  // 256 CUs x 8 blocks; the rest grid-strides

struct DevOps {
  __device__ static void min64(u64* p, u64 v) {
    atomicMin(reinterpret_cast<ull*>(p), (ull)v);
  }
  // one add per truncated row; the compiler folds a wave's adds into one
  __device__ static void inc64(u64* p) {
    atomicAdd(reinterpret_cast<ull*>(p), 1ull);
  }
};

__global__ void __launch_bounds__(kThreads) collate_rows_kernel(
    Batch bt, i64 ntiles) {
  for (i64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // (column, tile) from the prefix table: wave-uniform, at most 64 steps
    int c = 0;
    while (c + 1 < (int)bt.ncols && bt.cols[c + 1].tile0 <= tile) ++c;
    const i64 units = bt.cols[c].units;
    const i64 u0 = (tile - bt.cols[c].tile0) * kTileUnits + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kTileUnits / kThreads; ++k) {
      const i64 u = u0 + k * kThreads;
      if (u < units) do_unit<DevOps>(bt, c, (u32)u);
    }
  }
}

// The launcher trusts the geometry: the caller (spark_tfrecord_amd/
// collate.py) checks every slot, row and output size on the host first.
void gpu_collate_rows(uintptr_t src, uintptr_t cols, uintptr_t sel_slot,
                      uintptr_t sel_row, i64 ncols, i64 B, i64 ntiles,
                      uintptr_t status, uintptr_t stream) {
  if (B <= 0 || ncols <= 0 || ntiles <= 0) return;
  if (ncols > kMaxCols)
    throw std::invalid_argument("gpu_collate_rows: more than 64 columns");
  Batch bt{(const Src*)src, (const Col*)cols, (const i32*)sel_slot,
           (const i64*)sel_row, ncols, B, (u64*)status};
  const i64 blocks = ntiles < kMaxBlocks ? ntiles : kMaxBlocks;
  hipLaunchKernelGGL(collate_rows_kernel, dim3((uint32_t)blocks),
                     dim3(kThreads), 0, (hipStream_t)stream, bt, ntiles);
  HIPC_CHECK(hipGetLastError());
}

}  // namespace

void register_collate(py::module_& m) {
  m.def("gpu_collate_rows", &gpu_collate_rows, py::arg("src"),
        py::arg("cols"), py::arg("sel_slot"), py::arg("sel_row"),
        py::arg("ncols"), py::arg("B"), py::arg("ntiles"), py::arg("status"),
        py::arg("stream"),
        "Collate B (slot, row) pairs into the dense outputs of the column "
        "table, one launch; status[0] (init all ones) collects the first bad "
        "cell as (b << 16) | (column << 8) | cause, status[1] (init 0) the "
        "truncated rows");
}
