// gfx950 LZ4 decompressor for Hadoop-framed `.lz4` files: one container
// block per WAVE.
//
// The container (spark_tfrecord_amd/io/paths.py lz4_walk) frames raw LZ4
// chunks with their compressed lengths only: a block states how many bytes
// it holds, a chunk does not, so the host knows every BLOCK's input and
// output extent from the headers and the wave walks the block's chunks
// itself (csrc/lz4_core.h unlz4_container_block, which also holds the
// cause codes). All blocks of all files of a group decode in one launch.
//
// LZ4's serial chain per sequence is token -> length bytes -> offset behind
// the literals -> next token, each a dependent read: from HBM the walk
// would be pure latency. So the wave stages the chunk's input in LDS, a
// 4 KiB window per wave filled by all 64 lanes with 8-byte loads, and the
// walk's header reads are LDS reads. Literals inside the window go LDS ->
// output; a literal longer than what is left of the window is copied input
// -> output by all lanes and the window restarts behind it. Matches are
// shared by the lanes in 8-byte words, self-overlapping ones by doubling
// (lz4_core.h match_copy).
//
//   unlz4_blocks_kernel   1 wave per container block, grid-stride over the
//                         block table rows (in_off, in_len, out_off,
//                         raw_len, file)
//
// A block the core refuses sets its file's error word to
// ((block + 1) << 8) | cause with atomicMin, block counted within the file;
// -1 = clean. The caller sends a refused file to the host decoder.
// Reference behavior being replaced: Hadoop CodecStreams read of an
// Lz4Codec file, DefaultSource.scala:95-102 (codec by extension).

#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "../lz4_core.h"

namespace py = pybind11;
using namespace tfrec;
using tfrec::lz4::i64;
using tfrec::lz4::u32;
using tfrec::lz4::u8;

namespace {

#define HIPL_CHECK(expr)                                                       \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess)                                                      \
      throw std::runtime_error(std::string("HIP error: ") +                    \
                               hipGetErrorString(_e));                         \
  } while (0)

using ull = unsigned long long;

constexpr int kWaves = 4;      // waves per workgroup
constexpr int kBlockCols = 5;  // in_off, in_len, out_off, raw_len, file
enum { BK_IN_OFF, BK_IN_LEN, BK_OUT_OFF, BK_RAW_LEN, BK_FILE };
constexpr int kLdsBytes = kWaves * (int)lz4::kWindowAlloc;

// LDS: one input window per wave. The walk's state is a handful of uniform
// values (no per-lane arrays, no scratch); occupancy is bounded by the
// launch: the caller caps the grid at the resident-wave count.
__global__ void __launch_bounds__(256) unlz4_blocks_kernel(
    const u8* __restrict__ comp, const i64* __restrict__ bt,
    const i64* __restrict__ file_block0, i64 nblock, u8* __restrict__ out,
    ull* __restrict__ err) {
  __shared__ __attribute__((aligned(8))) u8 lds[kWaves][lz4::kWindowAlloc];
  // the wave's index is the same in all its lanes: as a scalar it keeps the
  // table row, the window's address and the whole walk in scalar registers
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  for (i64 g = (i64)blockIdx.x * kWaves + wid; g < nblock;
       g += (i64)gridDim.x * kWaves) {
    // the five words are independent of each other: one batch of loads
    const i64* b = bt + g * kBlockCols;
    const i64 in_off = b[BK_IN_OFF], in_len = b[BK_IN_LEN];
    const i64 out_off = b[BK_OUT_OFF], raw_len = b[BK_RAW_LEN];
    const i64 fi = b[BK_FILE];
    int rc = lz4::unlz4_container_block(comp + in_off, in_len, out + out_off,
                                        raw_len, lane, lds[wid]);
    if (rc && lane == 0)
      atomicMin(err + fi, ((ull)(g - file_block0[fi] + 1) << 8) | (u32)rc);
  }
}

// The launcher trusts the table's geometry: the caller (engine/gpu.py
// _device_unlz4_group) builds it on the host from the container headers
// and checks every extent against both buffers before it uploads it.
void gpu_unlz4_blocks(uintptr_t comp, uintptr_t block_table,
                      uintptr_t file_block0, i64 nblock, uintptr_t out,
                      uintptr_t err, i64 max_waves, uintptr_t stream) {
  if (nblock <= 0) return;
  if (max_waves < kWaves)
    throw std::invalid_argument("gpu_unlz4_blocks: max_waves < 4");
  i64 blocks = (nblock + kWaves - 1) / kWaves;
  if (blocks > max_waves / kWaves) blocks = max_waves / kWaves;
  hipLaunchKernelGGL(unlz4_blocks_kernel, dim3((uint32_t)blocks), dim3(256),
                     0, (hipStream_t)stream, (const u8*)comp,
                     (const i64*)block_table, (const i64*)file_block0, nblock,
                     (u8*)out, (ull*)err);
  HIPL_CHECK(hipGetLastError());
}

}  // namespace

void register_lz4(py::module_& m) {
  m.def("gpu_unlz4_blocks", &gpu_unlz4_blocks, py::arg("comp"),
        py::arg("block_table"), py::arg("file_block0"), py::arg("nblock"),
        py::arg("out"), py::arg("err"), py::arg("max_waves"),
        py::arg("stream"),
        "Decode LZ4 container blocks, one per wave; block_table rows are "
        "(in_off, in_len, out_off, raw_len, file); err[file] (init -1) "
        "collects ((block+1)<<8)|cause of the first block refused");
  m.attr("LZ4_BLOCK_COLS") = (int)kBlockCols;
  m.attr("LZ4_WAVES_PER_BLOCK") = (int)kWaves;
  m.attr("LZ4_LDS_BYTES_PER_BLOCK") = (int)kLdsBytes;
}
