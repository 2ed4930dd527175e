// gfx950 DEFLATE compressor: the write half of the segmented gzip format
// (spark_tfrecord_amd/io/paths.py compress_bytes; csrc/hip/inflate.hip is
// the read half). An uncompressed file image in HBM becomes a complete gzip
// file image in HBM:
//
//   deflate_segments_kernel  one segment per WAVE -> raw-deflate sub-stream
//                            in the segment's bounded staging slot, its
//                            length and its CRC-32
//   rocprim exclusive scan   of the lengths (gpu_excl_sum_strided)
//   gzip_assemble_kernel     gathers the sub-streams behind the header,
//                            writes header + FEXTRA 'TS' table from the
//                            device-side lengths, folds the segment CRCs
//                            into the trailer
//
// The layout is known before any byte is compressed (the table's size
// depends only on the segment count), so nothing goes back to the host but
// one read of the final image size. The algorithm itself lives in
// csrc/deflate_core.h, shared with the host build that the CPU tests run.
// Reference behavior being replaced: Hadoop CodecStreams gzip write,
// DefaultSource.scala (codec option).

#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <cstdint>
#include <cstdlib>
#include <string>

#include "../crc32c.h"
#include "../deflate_core.h"
#include "crc_wave.h"

namespace py = pybind11;
using namespace tfrec;

namespace {

#define HIPD_CHECK(expr)                                                       \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess)                                                      \
      throw std::runtime_error(std::string("HIP error: ") +                    \
                               hipGetErrorString(_e));                         \
  } while (0)

using tfrec::deflate::Scratch;
using tfrec::inflate::i64;
using tfrec::inflate::u32;
using tfrec::inflate::u64;
using tfrec::inflate::u8;

constexpr int kWavesPerBlock = 4;

// One segment per wave, grid-stride over segments. Segment i covers
// in[i*seg, min(n, (i+1)*seg)) and writes its sub-stream to
// staging[i*slot, ...), slot >= seg_out_bound(seg). Tokens go to a global
// workspace sized per RESIDENT wave (tok_cap entries each), not per
// segment. err (init ~0ull) collects ((seg+1)<<8)|cause of the first
// failure, as in the inflater.
__global__ void __launch_bounds__(256) deflate_segments_kernel(
    const u8* __restrict__ in, i64 n, i64 seg, i64 nseg,
    u8* __restrict__ staging, i64 slot, i64* __restrict__ comp_len,
    u32* __restrict__ seg_crc, u32* __restrict__ tok_ws, i64 tok_cap,
    double stored_threshold, unsigned long long* __restrict__ err) {
  __shared__ Scratch S[kWavesPerBlock];
  __shared__ u32 C[kWavesPerBlock][64];
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  i64 wave = (i64)blockIdx.x * kWavesPerBlock + wid;
  i64 nwaves = (i64)gridDim.x * kWavesPerBlock;
  u32* toks = tok_ws + wave * tok_cap;
  for (i64 s = wave; s < nseg; s += nwaves) {
    i64 lo = s * seg;
    i64 u = n - lo < seg ? n - lo : seg;
    if (u < 0) u = 0;
    int rc = 0;
    i64 len = 0;
    if (u > tok_cap || deflate::seg_out_bound(u) > slot) {
      rc = 2;  // launcher contract broken: write nothing
    } else {
      u32 crc = crc32_ieee_wave(in + lo, u, lane, C[wid]);
      len = deflate::deflate_one(in + lo, u, staging + s * slot, slot,
                                 s == nseg - 1, stored_threshold, toks,
                                 S[wid], lane);
      if (lane == 0) seg_crc[s] = crc;
      if (len < 0) {
        rc = 1;
        len = 0;
      }
    }
    if (lane == 0) {
      comp_len[s] = len;
      if (rc) atomicMin(err, ((unsigned long long)(s + 1) << 8) | (u32)rc);
    }
  }
}

// Blocks [0, gridDim.x - 1) gather the sub-streams to their final offsets;
// the last block writes the header, the 'TS' table and the trailer, and
// result[0] = final image size, result[1] = the error word.
__global__ void __launch_bounds__(256) gzip_assemble_kernel(
    const u8* __restrict__ staging, i64 slot, const i64* __restrict__ comp_len,
    const i64* __restrict__ comp_off, const u32* __restrict__ seg_crc, i64 n,
    i64 seg, i64 nseg, u8* __restrict__ out, i64 out_cap,
    const unsigned long long* __restrict__ err, i64* __restrict__ result) {
  const i64 body_off = 20 + 8 * nseg;
  const int tid = threadIdx.x;
  if (blockIdx.x + 1 < gridDim.x) {
    for (i64 s = blockIdx.x; s < nseg; s += gridDim.x - 1) {
      const u8* src = staging + s * slot;
      i64 len = comp_len[s];
      i64 dst_off = body_off + comp_off[s];
      if (len < 0 || len > slot || dst_off + len + 8 > out_cap) continue;
      u8* dst = out + dst_off;
      i64 words = len >> 3;
      for (i64 k = tid; k < words; k += 256) {
        u64 w;
        __builtin_memcpy(&w, src + 8 * k, 8);
        __builtin_memcpy(dst + 8 * k, &w, 8);
      }
      for (i64 b = (words << 3) + tid; b < len; b += 256) dst[b] = src[b];
    }
    return;
  }
  // header: ID1 ID2 CM=8 FLG=FEXTRA, MTIME=0, XFL=0, OS=255, XLEN, then
  // 'T' 'S' LEN, version 1, pad 0, nseg, (comp, uncomp) u32 pairs
  if (tid == 0) {
    const u32 payload = 4 + 8 * (u32)nseg, xlen = payload + 4;
    const u8 h[20] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff,
                      (u8)xlen, (u8)(xlen >> 8), 'T', 'S',
                      (u8)payload, (u8)(payload >> 8), 1, 0,
                      (u8)nseg, (u8)(nseg >> 8)};
    for (int i = 0; i < 20; ++i) out[i] = h[i];
  }
  for (i64 s = tid; s < nseg; s += 256) {
    u32 c = (u32)comp_len[s];
    i64 lo = s * seg;
    u32 u = (u32)(n - lo < seg ? (n - lo < 0 ? 0 : n - lo) : seg);
    u8* e = out + 20 + 8 * s;
    for (int i = 0; i < 4; ++i) {
      e[i] = (u8)(c >> (8 * i));
      e[4 + i] = (u8)(u >> (8 * i));
    }
  }
  // trailer CRC: segments [0, nseg-1) all have length seg, so one shift
  // element folds them; each thread folds a contiguous run, thread 0 joins
  // the runs and appends the (shorter) last segment
  __shared__ u32 part[256];
  const i64 m = nseg - 1;
  const i64 per = (m + 255) / 256;
  const u32 sh_seg = crc32_ieee_shift_elem((u64)seg);
  {
    i64 a = (i64)tid * per, b = a + per < m ? a + per : m;
    u32 acc = 0;
    for (i64 s = a; s < b; ++s) acc = crc_ieee_gfmul(acc, sh_seg) ^ seg_crc[s];
    part[tid] = acc;
  }
  __syncthreads();
  if (tid == 0) {
    u32 acc = 0;
    const u32 sh_run = crc32_ieee_shift_elem((u64)per * (u64)seg);
    for (int t = 0; t < 256; ++t) {
      i64 a = (i64)t * per;
      if (a >= m) break;
      i64 cnt = a + per < m ? per : m - a;
      u32 sh = cnt == per ? sh_run
                          : crc32_ieee_shift_elem((u64)cnt * (u64)seg);
      acc = crc_ieee_gfmul(acc, sh) ^ part[t];
    }
    i64 last_u = n - m * seg;
    if (last_u < 0) last_u = 0;
    u32 crc = crc32_ieee_combine(acc, seg_crc[m], (u64)last_u);
    i64 total = comp_off[nseg];
    i64 size = body_off + total + 8;
    if (size <= out_cap && total >= 0) {
      u8* t = out + body_off + total;
      u32 isize = (u32)((u64)n & 0xFFFFFFFFull);
      for (int i = 0; i < 4; ++i) {
        t[i] = (u8)(crc >> (8 * i));
        t[4 + i] = (u8)(isize >> (8 * i));
      }
    }
    result[0] = size;
    result[1] = (i64)err[0];
  }
}

void gpu_deflate_segments(uintptr_t in, i64 n, i64 seg, i64 nseg,
                          uintptr_t staging, i64 slot, uintptr_t comp_len,
                          uintptr_t seg_crc, uintptr_t tok_ws, i64 tok_cap,
                          i64 nwaves, double stored_threshold, uintptr_t err,
                          uintptr_t stream) {
  if (nseg <= 0) return;
  if (seg <= 0 || n < 0 || nwaves < kWavesPerBlock ||
      nwaves % kWavesPerBlock != 0 || (nseg - 1) * seg > n ||
      nseg * seg < n)
    throw std::invalid_argument("gpu_deflate_segments: bad geometry");
  i64 blocks = nwaves / kWavesPerBlock;
  hipLaunchKernelGGL(deflate_segments_kernel, dim3((uint32_t)blocks),
                     dim3(256), 0, (hipStream_t)stream, (const u8*)in, n, seg,
                     nseg, (u8*)staging, slot, (i64*)comp_len, (u32*)seg_crc,
                     (u32*)tok_ws, tok_cap, stored_threshold,
                     (unsigned long long*)err);
  HIPD_CHECK(hipGetLastError());
}

void gpu_gzip_assemble(uintptr_t staging, i64 slot, uintptr_t comp_len,
                       uintptr_t comp_off, uintptr_t seg_crc, i64 n, i64 seg,
                       i64 nseg, uintptr_t out, i64 out_cap, uintptr_t err,
                       uintptr_t result, uintptr_t stream) {
  if (nseg <= 0 || nseg > 8189)
    throw std::invalid_argument("gpu_gzip_assemble: bad segment count");
  i64 gather = nseg < 2048 ? nseg : 2048;
  hipLaunchKernelGGL(gzip_assemble_kernel, dim3((uint32_t)gather + 1),
                     dim3(256), 0, (hipStream_t)stream, (const u8*)staging,
                     slot, (const i64*)comp_len, (const i64*)comp_off,
                     (const u32*)seg_crc, n, seg, nseg, (u8*)out, out_cap,
                     (const unsigned long long*)err, (i64*)result);
  HIPD_CHECK(hipGetLastError());
}

}  // namespace

void register_deflate(py::module_& m) {
  m.def("gpu_deflate_segments", &gpu_deflate_segments, py::arg("src"),
        py::arg("n"), py::arg("seg"), py::arg("nseg"), py::arg("staging"),
        py::arg("slot"), py::arg("comp_len"), py::arg("seg_crc"),
        py::arg("tok_ws"), py::arg("tok_cap"), py::arg("nwaves"),
        py::arg("stored_threshold"), py::arg("err"), py::arg("stream"),
        "Compress src[0, n) as nseg raw-deflate segments of `seg` bytes, one "
        "per wave, into staging slots; comp_len/seg_crc get each segment's "
        "length and CRC-32; err[0] (init ~0ull) collects "
        "((seg+1)<<8)|cause of the first failure");
  m.def("gpu_gzip_assemble", &gpu_gzip_assemble, py::arg("staging"),
        py::arg("slot"), py::arg("comp_len"), py::arg("comp_off"),
        py::arg("seg_crc"), py::arg("n"), py::arg("seg"), py::arg("nseg"),
        py::arg("out"), py::arg("out_cap"), py::arg("err"),
        py::arg("result"), py::arg("stream"),
        "Gather the segments behind a gzip header with the 'TS' table and "
        "write the CRC-32/ISIZE trailer; result = [image size, error word]");
  m.def("deflate_seg_out_bound",
        [](i64 u) { return deflate::seg_out_bound(u); },
        "Worst-case sub-stream length of a u-byte segment");
}
