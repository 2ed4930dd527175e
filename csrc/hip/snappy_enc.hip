// gfx950 Snappy compressor: the write half of the Hadoop-framed `.snappy`
// format (spark_tfrecord_amd/io/paths.py snappy_walk; csrc/hip/snappy.hip is
// the read half). An uncompressed file image in HBM becomes a complete
// `.snappy` file image in HBM:
//
//   snap_blocks_kernel      one block per WAVE -> raw-Snappy chunk in the
//                           block's bounded staging slot, and its length
//   rocprim exclusive scan  of the lengths (gpu_excl_sum_strided)
//   snappy_assemble_kernel  writes each block's 8 header bytes (raw length,
//                           chunk length, big-endian) and gathers the chunk
//                           behind them
//
// Every container block holds one chunk, so block k starts at
// 8 * k + (sum of the chunk lengths before it) and nothing goes back to the
// host but one read of the final image size. The algorithm itself lives in
// csrc/snappy_enc_core.h, shared with the host build that the CPU tests run.
// Reference behavior being replaced: Hadoop CodecStreams write through
// SnappyCodec, DefaultSource.scala (codec option).

#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "../snappy_enc_core.h"

namespace py = pybind11;
using namespace tfrec;
using tfrec::snappy::EncScratch;
using tfrec::snappy::i64;
using tfrec::snappy::u32;
using tfrec::snappy::u64;
using tfrec::snappy::u8;

namespace {

#define HIPSE_CHECK(expr)                                                      \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess)                                                      \
      throw std::runtime_error(std::string("HIP error: ") +                    \
                               hipGetErrorString(_e));                         \
  } while (0)

using ull = unsigned long long;

constexpr int kWavesPerBlock = 4;
enum { SE_CORE_REFUSED = 1, SE_BAD_GEOMETRY = 2 };

// One block per wave, grid-stride over blocks. Block k covers
// img[k*B, min(n, (k+1)*B)) and writes its chunk to staging[k*slot, ...),
// slot >= snap_out_bound(B). err (init ~0ull) collects ((block+1)<<8)|cause
// of the first failure, as in the other codecs.
__global__ void __launch_bounds__(256) snap_blocks_kernel(
    const u8* __restrict__ img, i64 n, i64 B, i64 nblk,
    u8* __restrict__ staging, i64 slot, i64* __restrict__ comp_len,
    ull* __restrict__ err) {
  __shared__ EncScratch S[kWavesPerBlock];
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const i64 nwaves = (i64)gridDim.x * kWavesPerBlock;
  for (i64 k = (i64)blockIdx.x * kWavesPerBlock + wid; k < nblk; k += nwaves) {
    const i64 lo = k * B;
    const i64 u = n - lo < B ? n - lo : B;
    int rc = 0;
    i64 len = 0;
    if (u <= 0 || snappy::snap_out_bound(u) > slot) {
      rc = SE_BAD_GEOMETRY;  // launcher contract broken: write nothing
    } else {
      len = snappy::snap_one(img + lo, u, staging + k * slot, slot, S[wid],
                             lane);
      if (len < 0) {
        rc = SE_CORE_REFUSED;
        len = 0;
      }
    }
    if (lane == 0) {
      comp_len[k] = len;
      if (rc) atomicMin(err, ((ull)(k + 1) << 8) | (u32)rc);
    }
  }
}

// Grid-stride over blocks, one workgroup per block at a time: thread 0
// writes the 8 header bytes, all threads copy the chunk behind them. Block
// 0's thread 0 also writes result[0] = final image size, result[1] = the
// error word. A length the compressor kernel could not have produced is
// skipped (the error word already names its block).
__global__ void __launch_bounds__(256) snappy_assemble_kernel(
    const u8* __restrict__ staging, i64 slot, const i64* __restrict__ comp_len,
    const i64* __restrict__ comp_off, i64 n, i64 B, i64 nblk,
    u8* __restrict__ out, i64 out_cap, const ull* __restrict__ err,
    i64* __restrict__ result) {
  const int tid = threadIdx.x;
  for (i64 k = blockIdx.x; k < nblk; k += gridDim.x) {
    const u8* src = staging + k * slot;
    const i64 len = comp_len[k];
    const i64 dst_off = 8 * k + comp_off[k];
    if (len <= 0 || len > slot || dst_off < 0 || dst_off + 8 + len > out_cap)
      continue;
    u8* dst = out + dst_off;
    if (tid == 0) {
      const i64 lo = k * B;
      const u32 raw = (u32)(n - lo < B ? n - lo : B);
      const u32 c = (u32)len;
      for (int i = 0; i < 4; ++i) {
        dst[i] = (u8)(raw >> (24 - 8 * i));
        dst[4 + i] = (u8)(c >> (24 - 8 * i));
      }
    }
    dst += 8;
    const i64 words = len >> 3;
    for (i64 w = tid; w < words; w += 256) {
      u64 x;
      __builtin_memcpy(&x, src + 8 * w, 8);
      __builtin_memcpy(dst + 8 * w, &x, 8);
    }
    for (i64 b = (words << 3) + tid; b < len; b += 256) dst[b] = src[b];
  }
  if (blockIdx.x == 0 && tid == 0) {
    result[0] = 8 * nblk + comp_off[nblk];
    result[1] = (i64)err[0];
  }
}

bool bad_geometry(i64 n, i64 B, i64 nblk) {
  return B <= 0 || n <= 0 || nblk <= 0 || (nblk - 1) * B >= n || nblk * B < n;
}

void gpu_snap_blocks(uintptr_t img, i64 n, i64 B, i64 nblk, uintptr_t staging,
                     i64 slot, uintptr_t comp_len, i64 nwaves, uintptr_t err,
                     uintptr_t stream) {
  if (bad_geometry(n, B, nblk) || nwaves < kWavesPerBlock ||
      nwaves % kWavesPerBlock != 0 ||
      slot < snappy::snap_out_bound(n < B ? n : B))
    throw std::invalid_argument("gpu_snap_blocks: bad geometry");
  hipLaunchKernelGGL(snap_blocks_kernel,
                     dim3((uint32_t)(nwaves / kWavesPerBlock)), dim3(256), 0,
                     (hipStream_t)stream, (const u8*)img, n, B, nblk,
                     (u8*)staging, slot, (i64*)comp_len, (ull*)err);
  HIPSE_CHECK(hipGetLastError());
}

void gpu_snappy_assemble(uintptr_t staging, i64 slot, uintptr_t comp_len,
                         uintptr_t comp_off, i64 n, i64 B, i64 nblk,
                         uintptr_t out, i64 out_cap, uintptr_t err,
                         uintptr_t result, uintptr_t stream) {
  if (bad_geometry(n, B, nblk) || slot <= 0 || out_cap < 0)
    throw std::invalid_argument("gpu_snappy_assemble: bad geometry");
  const i64 grid = nblk < 4096 ? nblk : 4096;
  hipLaunchKernelGGL(snappy_assemble_kernel, dim3((uint32_t)grid), dim3(256),
                     0, (hipStream_t)stream, (const u8*)staging, slot,
                     (const i64*)comp_len, (const i64*)comp_off, n, B, nblk,
                     (u8*)out, out_cap, (const ull*)err, (i64*)result);
  HIPSE_CHECK(hipGetLastError());
}

}  // namespace

void register_snappy_enc(py::module_& m) {
  m.def("gpu_snap_blocks", &gpu_snap_blocks, py::arg("img"), py::arg("n"),
        py::arg("block"), py::arg("nblk"), py::arg("staging"),
        py::arg("slot"), py::arg("comp_len"), py::arg("nwaves"),
        py::arg("err"), py::arg("stream"),
        "Compress img[0, n) as nblk raw-Snappy chunks of `block` raw bytes, "
        "one per wave, into staging slots; comp_len gets each chunk's "
        "length; err[0] (init ~0ull) collects ((block+1)<<8)|cause of the "
        "first failure");
  m.def("gpu_snappy_assemble", &gpu_snappy_assemble, py::arg("staging"),
        py::arg("slot"), py::arg("comp_len"), py::arg("comp_off"),
        py::arg("n"), py::arg("block"), py::arg("nblk"), py::arg("out"),
        py::arg("out_cap"), py::arg("err"), py::arg("result"),
        py::arg("stream"),
        "Write each block's 8 header bytes and gather its chunk behind "
        "them; result = [image size, error word]");
  m.attr("SNAP_LDS_BYTES_PER_BLOCK") =
      (int)(kWavesPerBlock * sizeof(EncScratch));
  m.attr("SNAP_WAVES_PER_BLOCK") = (int)kWavesPerBlock;
}
