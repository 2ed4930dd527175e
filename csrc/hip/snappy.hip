// gfx950 Snappy decompressor for Hadoop-framed `.snappy` files: one raw
// chunk per WAVE.
//
// The container (spark_tfrecord_amd/io/paths.py, "Hadoop block container")
// frames independent raw-Snappy chunks with explicit lengths, so the host
// knows every chunk's input and output extent from the 8-byte headers alone
// and the device decodes all chunks of all files of a group in one launch.
// Snappy is byte-aligned and has no entropy code: the walk over the elements
// is serial, but every element is a plain copy that the 64 lanes share, and
// the lanes parse the element headers of 64 input bytes at a time
// (csrc/snappy_core.h, which also holds the cause codes).
//
//   unsnap_chunks_kernel   1 wave per chunk, grid-stride over the chunk
//                          table rows (in_off, in_len, out_off, out_len,
//                          file)
//
// A chunk the core refuses sets its file's error word to
// ((chunk + 1) << 8) | cause with atomicMin, chunk counted within the file;
// -1 = clean. The caller sends a refused file to the host decoder.
// Reference behavior being replaced: Hadoop CodecStreams read of a
// SnappyCodec file, DefaultSource.scala:95-102 (codec by extension).

#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "../snappy_core.h"

namespace py = pybind11;
using namespace tfrec;
using tfrec::snappy::i64;
using tfrec::snappy::u32;
using tfrec::snappy::u8;

namespace {

#define HIPS_CHECK(expr)                                                       \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess)                                                      \
      throw std::runtime_error(std::string("HIP error: ") +                    \
                               hipGetErrorString(_e));                         \
  } while (0)

using ull = unsigned long long;

constexpr int kWaves = 4;      // waves per block
constexpr int kChunkCols = 5;  // in_off, in_len, out_off, out_len, file
enum { CK_IN_OFF, CK_IN_LEN, CK_OUT_OFF, CK_OUT_LEN, CK_FILE };

// No LDS and no scratch arrays: the walk's state is a handful of uniform
// values, so occupancy is bounded by the launch (the caller caps the grid
// at the resident-wave count), not by registers.
__global__ void __launch_bounds__(256) unsnap_chunks_kernel(
    const u8* __restrict__ comp, const i64* __restrict__ ct,
    const i64* __restrict__ file_chunk0, i64 nchunk, u8* __restrict__ out,
    ull* __restrict__ err) {
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  for (i64 g = (i64)blockIdx.x * kWaves + wid; g < nchunk;
       g += (i64)gridDim.x * kWaves) {
    // the five words are independent of each other: one batch of loads
    const i64* c = ct + g * kChunkCols;
    const i64 in_off = c[CK_IN_OFF], in_len = c[CK_IN_LEN];
    const i64 out_off = c[CK_OUT_OFF], out_len = c[CK_OUT_LEN];
    const i64 fi = c[CK_FILE];
    int rc = snappy::unsnap_one(comp + in_off, in_len, out + out_off,
                                out_len, lane);
    if (rc && lane == 0)
      atomicMin(err + fi, ((ull)(g - file_chunk0[fi] + 1) << 8) | (u32)rc);
  }
}

// The launcher trusts the table's geometry: the caller (engine/gpu.py
// _device_unsnap_group) builds it on the host from the container headers
// and checks every extent against both buffers before it uploads it.
void gpu_unsnap_chunks(uintptr_t comp, uintptr_t chunk_table,
                       uintptr_t file_chunk0, i64 nchunk, uintptr_t out,
                       uintptr_t err, i64 max_waves, uintptr_t stream) {
  if (nchunk <= 0) return;
  if (max_waves < kWaves)
    throw std::invalid_argument("gpu_unsnap_chunks: max_waves < 4");
  i64 blocks = (nchunk + kWaves - 1) / kWaves;
  if (blocks > max_waves / kWaves) blocks = max_waves / kWaves;
  hipLaunchKernelGGL(unsnap_chunks_kernel, dim3((uint32_t)blocks), dim3(256),
                     0, (hipStream_t)stream, (const u8*)comp,
                     (const i64*)chunk_table, (const i64*)file_chunk0, nchunk,
                     (u8*)out, (ull*)err);
  HIPS_CHECK(hipGetLastError());
}

}  // namespace

void register_snappy(py::module_& m) {
  m.def("gpu_unsnap_chunks", &gpu_unsnap_chunks, py::arg("comp"),
        py::arg("chunk_table"), py::arg("file_chunk0"), py::arg("nchunk"),
        py::arg("out"), py::arg("err"), py::arg("max_waves"),
        py::arg("stream"),
        "Decode raw-Snappy chunks, one per wave; chunk_table rows are "
        "(in_off, in_len, out_off, out_len, file); err[file] (init -1) "
        "collects ((chunk+1)<<8)|cause of the first chunk refused");
  m.attr("SNAPPY_CHUNK_COLS") = (int)kChunkCols;
}
