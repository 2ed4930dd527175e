// gfx950 inflater for gzip files that carry no segment table (any writer's
// gzip): block-parallel speculative decode, the pugz / rapidgzip technique.
// The six steps and the tables are described in csrc/inflate_spec_core.h,
// which also holds the decode itself, shared with the host build.
//
//   foreign_find_kernel     1 wave per chunk: 64 bit positions screened per
//                           step in registers, __ballot, survivors parsed
//                           in full one at a time, wave-uniformly
//   foreign_count_kernel    1 wave per start found: decode without stores
//   foreign_chain_kernel    1 thread per file: live chunks, output offsets
//   foreign_decode_kernel   1 wave per live chunk: decode to u16 symbols
//   foreign_window_kernel   1 workgroup per file: last 32 KiB of each live
//                           chunk to bytes, in order, a barrier in between
//   foreign_resolve_kernel  1 workgroup per live chunk: all other symbols
//   foreign_crc_kernel      1 wave per 64 KiB piece of the output
//   foreign_finish_kernel   1 thread per file: fold the piece CRCs, compare
//                           with the trailer
//
// All files of a group share each launch. A file whose error word (RS_ERR)
// is set is skipped by every later kernel; the caller sends it to host
// zlib. Nothing returns to the host between the launches.
// Reference behavior being replaced: Hadoop CodecStreams gzip read,
// DefaultSource.scala:95-102 (codec by extension, whoever wrote the file).

#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <cstdint>
#include <cstdlib>
#include <string>

#include "../inflate_spec_core.h"
#include "crc_wave.h"

namespace py = pybind11;
using namespace tfrec;
using namespace tfrec::inflate;

namespace {

#define HIPF_CHECK(expr)                                                       \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess)                                                      \
      throw std::runtime_error(std::string("HIP error: ") +                    \
                               hipGetErrorString(_e));                         \
  } while (0)

using ull = unsigned long long;

constexpr int kWaves = 4;  // waves per block in the per-chunk kernels

__device__ inline void set_err(i64* res, i64 chunk, int cause) {
  atomicMin(reinterpret_cast<ull*>(res + RS_ERR),
            ((ull)(chunk + 1) << 8) | (u32)cause);
}

__global__ void __launch_bounds__(256) foreign_find_kernel(
    const u8* __restrict__ comp, const i64* __restrict__ ft,
    i64* __restrict__ ct, i64 nchunk_total, i64 chunk_bytes) {
  __shared__ LaneScratch S[kWaves];
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const i64 chunk_bits = chunk_bytes * 8;
  for (i64 g = (i64)blockIdx.x * kWaves + wid; g < nchunk_total;
       g += (i64)gridDim.x * kWaves) {
    const i64* f = ft + ct[g * kChunkCols + CH_FILE] * kFileCols;
    const i64 j = g - f[FL_CHUNK0];
    i64 found = -1;
    if (j == 0) {
      found = 0;  // the stream's first block, of any type
    } else {
      const u8* body = comp + f[FL_BODY_OFF];
      const i64 body_len = f[FL_BODY_LEN];
      const i64 lo = j * chunk_bits;
      const i64 hi =
          lo + chunk_bits < body_len * 8 ? lo + chunk_bits : body_len * 8;
      for (i64 base = lo; base < hi && found < 0; base += 64) {
        i64 bit = base + lane;
        bool pass =
            bit < hi && cheap_head_check(load_bits96(body, body_len, bit));
        ull mask = __ballot(pass);
        while (mask) {
          int b = __ffsll((long long)mask) - 1;
          mask &= mask - 1;
          if (full_head_check(body, body_len, base + b, S[wid])) {
            found = base + b;
            break;
          }
        }
      }
    }
    if (lane == 0) ct[g * kChunkCols + CH_START] = found;
  }
}

__global__ void __launch_bounds__(256) foreign_count_kernel(
    const u8* __restrict__ comp, const i64* __restrict__ ft, i64* ct,
    i64 nchunk_total, i64 chunk_bytes) {
  __shared__ LaneScratch S[kWaves];
  __shared__ uint16_t T[kWaves][kLitTabSize];
  __shared__ uint16_t D[kWaves][kDistTabSize];
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  for (i64 g = (i64)blockIdx.x * kWaves + wid; g < nchunk_total;
       g += (i64)gridDim.x * kWaves) {
    i64* c = ct + g * kChunkCols;
    const i64 start = c[CH_START];
    if (start < 0) continue;
    const i64* f = ft + c[CH_FILE] * kFileCols;
    const i64 j = g - f[FL_CHUNK0];
    i64 out_len, end_bit, next;
    int rc = spec_run<false>(comp + f[FL_BODY_OFF], f[FL_BODY_LEN], start,
                             ct + f[FL_CHUNK0] * kChunkCols, f[FL_NCHUNK],
                             chunk_bytes * 8, f[FL_ISIZE], nullptr,
                             j ? f[FL_ISIZE] : 0, S[wid], T[wid], D[wid], lane,
                             out_len, end_bit, next);
    if (lane == 0) {
      c[CH_OUT_LEN] = out_len;
      c[CH_END] = end_bit;
      c[CH_NEXT] = next;
      c[CH_RC] = rc;
    }
  }
}

__global__ void foreign_chain_kernel(const i64* __restrict__ ft, i64* ct,
                                     i64* res, i64 nfile) {
  i64 fi = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (fi >= nfile) return;
  const i64* f = ft + fi * kFileCols;
  i64 n_live = 0;
  i64 err = spec_chain(ct + f[FL_CHUNK0] * kChunkCols, f[FL_NCHUNK],
                       f[FL_BODY_LEN], f[FL_ISIZE], n_live);
  res[fi * kResCols + RS_LIVE] = n_live;
  if (err) res[fi * kResCols + RS_ERR] = err;
}

__global__ void __launch_bounds__(256) foreign_decode_kernel(
    const u8* __restrict__ comp, const i64* __restrict__ ft,
    const i64* __restrict__ ct, i64* res, uint16_t* __restrict__ symbuf,
    i64 nchunk_total, i64 chunk_bytes) {
  __shared__ LaneScratch S[kWaves];
  __shared__ uint16_t T[kWaves][kLitTabSize];
  __shared__ uint16_t D[kWaves][kDistTabSize];
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  for (i64 g = (i64)blockIdx.x * kWaves + wid; g < nchunk_total;
       g += (i64)gridDim.x * kWaves) {
    const i64* c = ct + g * kChunkCols;
    const i64 fi = c[CH_FILE];
    const i64* f = ft + fi * kFileCols;
    const i64 out_off = c[CH_OUT_OFF];
    // the chain has checked that the live [out_off, out_off + out_len)
    // tile [0, ISIZE), the symbol buffer's share of this file
    if (out_off < 0 || res[fi * kResCols + RS_ERR] != -1) continue;
    i64 out_len, end_bit, next;
    int rc = spec_run<true>(comp + f[FL_BODY_OFF], f[FL_BODY_LEN], c[CH_START],
                            ct + f[FL_CHUNK0] * kChunkCols, f[FL_NCHUNK],
                            chunk_bytes * 8, c[CH_OUT_LEN],
                            symbuf + f[FL_SYM_BASE] + out_off, out_off, S[wid],
                            T[wid], D[wid], lane, out_len, end_bit, next);
    if (!rc && (out_len != c[CH_OUT_LEN] || end_bit != c[CH_END] ||
                next != c[CH_NEXT]))
      rc = SPEC_DISAGREE;
    if (rc && lane == 0) set_err(res + fi * kResCols, g - f[FL_CHUNK0], rc);
  }
}

// Symbols [lo, hi) of the chunk at `start` -> bytes; returns markers seen.
__device__ inline i64 resolve_range(const uint16_t* __restrict__ sym, u8* out,
                                    i64 start, i64 lo, i64 hi, int tid,
                                    int nthreads, bool& bad) {
  i64 markers = 0;
  for (i64 i = lo + tid; i < hi; i += nthreads) {
    int b = spec_resolve_sym(sym[start + i], out, start, markers);
    if (b < 0) {
      bad = true;
      b = 0;
    }
    out[start + i] = (u8)b;
  }
  return markers;
}

__global__ void __launch_bounds__(1024) foreign_window_kernel(
    const i64* __restrict__ ft, const i64* __restrict__ ct, i64* res,
    const uint16_t* __restrict__ symbuf, u8* out) {
  const i64 fi = blockIdx.x;
  const i64* f = ft + fi * kFileCols;
  i64* r = res + fi * kResCols;
  const bool skip = r[RS_ERR] != -1;
  const i64 n_live = r[RS_LIVE];
  __syncthreads();  // every thread has read the error word before any sets it
  if (skip) return;
  const i64* fct = ct + f[FL_CHUNK0] * kChunkCols;
  const uint16_t* sym = symbuf + f[FL_SYM_BASE];
  u8* fout = out + f[FL_OUT_BASE];
  i64 markers = 0;
  bool bad = false;
  for (i64 k = 0; k < n_live; ++k) {
    const i64* c = fct + fct[k * kChunkCols + CH_LIVE] * kChunkCols;
    const i64 len = c[CH_OUT_LEN];
    const i64 tail = len > kSpecWindow ? len - kSpecWindow : 0;
    markers += resolve_range(sym, fout, c[CH_OUT_OFF], tail, len, threadIdx.x,
                             blockDim.x, bad);
    __syncthreads();  // the next chunk's markers read these bytes
  }
  if (markers) atomicAdd(reinterpret_cast<ull*>(r + RS_MARKERS), (ull)markers);
  if (bad) set_err(r, 0, SPEC_MARKER);
}

__global__ void __launch_bounds__(256) foreign_resolve_kernel(
    const i64* __restrict__ ft, const i64* __restrict__ ct, i64* res,
    const uint16_t* __restrict__ symbuf, u8* out, i64 nchunk_total) {
  for (i64 g = blockIdx.x; g < nchunk_total; g += gridDim.x) {
    const i64* c = ct + g * kChunkCols;
    const i64 fi = c[CH_FILE];
    const i64* f = ft + fi * kFileCols;
    i64* r = res + fi * kResCols;
    const i64 len = c[CH_OUT_LEN];
    if (c[CH_OUT_OFF] < 0 || len <= kSpecWindow) continue;
    // a file that failed earlier keeps its symbols: nothing to resolve.
    // (SPEC_MARKER set by another block of this launch only skips work.)
    if (r[RS_ERR] != -1) continue;
    bool bad = false;
    i64 markers = resolve_range(symbuf + f[FL_SYM_BASE], out + f[FL_OUT_BASE],
                                c[CH_OUT_OFF], 0, len - kSpecWindow,
                                threadIdx.x, blockDim.x, bad);
    if (markers)
      atomicAdd(reinterpret_cast<ull*>(r + RS_MARKERS), (ull)markers);
    if (bad) set_err(r, g - f[FL_CHUNK0], SPEC_MARKER);
  }
}

__global__ void __launch_bounds__(256) foreign_crc_kernel(
    const i64* __restrict__ ft, const i64* __restrict__ res,
    const u8* __restrict__ out, u32* __restrict__ piece_crc) {
  __shared__ u32 C[kWaves][64];
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const i64 fi = blockIdx.y;
  const i64* f = ft + fi * kFileCols;
  if (res[fi * kResCols + RS_ERR] != -1) return;
  const i64 isize = f[FL_ISIZE];
  const i64 npiece = (isize + kSpecCrcPiece - 1) / kSpecCrcPiece;
  for (i64 p = (i64)blockIdx.x * kWaves + wid; p < npiece;
       p += (i64)gridDim.x * kWaves) {
    i64 a = p * kSpecCrcPiece;
    i64 len = isize - a < kSpecCrcPiece ? isize - a : kSpecCrcPiece;
    u32 crc = crc32_ieee_wave(out + f[FL_OUT_BASE] + a, len, lane, C[wid]);
    if (lane == 0) piece_crc[f[FL_PIECE0] + p] = crc;
  }
}

__global__ void foreign_finish_kernel(const i64* __restrict__ ft, i64* res,
                                      const u32* __restrict__ piece_crc,
                                      i64 nfile) {
  i64 fi = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (fi >= nfile) return;
  const i64* f = ft + fi * kFileCols;
  i64* r = res + fi * kResCols;
  if (r[RS_ERR] != -1) return;
  const i64 isize = f[FL_ISIZE];
  const i64 npiece = (isize + kSpecCrcPiece - 1) / kSpecCrcPiece;
  const u32* pc = piece_crc + f[FL_PIECE0];
  const u32 sh = crc32_ieee_shift_elem((u64)kSpecCrcPiece);
  u32 acc = 0;
  for (i64 p = 0; p + 1 < npiece; ++p) acc = crc_ieee_gfmul(acc, sh) ^ pc[p];
  if (npiece > 0)
    acc = crc32_ieee_combine(acc, pc[npiece - 1],
                             (u64)(isize - (npiece - 1) * kSpecCrcPiece));
  r[RS_CRC] = (i64)acc;
  if (acc != (u32)f[FL_CRC]) r[RS_ERR] = SPEC_CRC;
}

// The launcher trusts the tables' geometry: the caller (engine/gpu.py
// _device_inflate_foreign_group) builds them on the host from the files'
// sizes and checks every extent against its buffer before it uploads them.
void gpu_inflate_foreign(uintptr_t comp, uintptr_t ft, uintptr_t ct,
                         uintptr_t res, uintptr_t piece_crc, uintptr_t symbuf,
                         uintptr_t out, i64 nfile, i64 nchunk_total,
                         i64 max_pieces, i64 chunk_bytes, uintptr_t stream) {
  if (nfile <= 0 || nchunk_total <= 0) return;
  if (chunk_bytes <= 0 || max_pieces <= 0 || nfile > 65535)
    throw std::invalid_argument("gpu_inflate_foreign: bad geometry");
  hipStream_t st = (hipStream_t)stream;
  i64 wave_blocks = (nchunk_total + kWaves - 1) / kWaves;
  if (wave_blocks > 16384) wave_blocks = 16384;
  i64 file_blocks = (nfile + 63) / 64;
  hipLaunchKernelGGL(foreign_find_kernel, dim3((uint32_t)wave_blocks),
                     dim3(256), 0, st, (const u8*)comp, (const i64*)ft,
                     (i64*)ct, nchunk_total, chunk_bytes);
  hipLaunchKernelGGL(foreign_count_kernel, dim3((uint32_t)wave_blocks),
                     dim3(256), 0, st, (const u8*)comp, (const i64*)ft,
                     (i64*)ct, nchunk_total, chunk_bytes);
  hipLaunchKernelGGL(foreign_chain_kernel, dim3((uint32_t)file_blocks),
                     dim3(64), 0, st, (const i64*)ft, (i64*)ct, (i64*)res,
                     nfile);
  hipLaunchKernelGGL(foreign_decode_kernel, dim3((uint32_t)wave_blocks),
                     dim3(256), 0, st, (const u8*)comp, (const i64*)ft,
                     (const i64*)ct, (i64*)res, (uint16_t*)symbuf,
                     nchunk_total, chunk_bytes);
  hipLaunchKernelGGL(foreign_window_kernel, dim3((uint32_t)nfile), dim3(1024),
                     0, st, (const i64*)ft, (const i64*)ct, (i64*)res,
                     (const uint16_t*)symbuf, (u8*)out);
  i64 res_blocks = nchunk_total < 16384 ? nchunk_total : 16384;
  hipLaunchKernelGGL(foreign_resolve_kernel, dim3((uint32_t)res_blocks),
                     dim3(256), 0, st, (const i64*)ft, (const i64*)ct,
                     (i64*)res, (const uint16_t*)symbuf, (u8*)out,
                     nchunk_total);
  i64 crc_blocks = (max_pieces + kWaves - 1) / kWaves;
  if (crc_blocks > 4096) crc_blocks = 4096;
  hipLaunchKernelGGL(foreign_crc_kernel,
                     dim3((uint32_t)crc_blocks, (uint32_t)nfile), dim3(256), 0,
                     st, (const i64*)ft, (const i64*)res, (const u8*)out,
                     (u32*)piece_crc);
  hipLaunchKernelGGL(foreign_finish_kernel, dim3((uint32_t)file_blocks),
                     dim3(64), 0, st, (const i64*)ft, (i64*)res,
                     (const u32*)piece_crc, nfile);
  HIPF_CHECK(hipGetLastError());
}

}  // namespace

void register_inflate_foreign(py::module_& m) {
  m.def("gpu_inflate_foreign", &gpu_inflate_foreign, py::arg("comp"),
        py::arg("file_table"), py::arg("chunk_table"), py::arg("result"),
        py::arg("piece_crc"), py::arg("symbuf"), py::arg("out"),
        py::arg("nfile"), py::arg("nchunk_total"), py::arg("max_pieces"),
        py::arg("chunk_bytes"), py::arg("stream"),
        "Speculative block-parallel inflate of table-less gzip members "
        "(tables as in csrc/inflate_spec_core.h); result[f][0] stays -1 for "
        "a file inflated and CRC-checked, else ((chunk+1)<<8)|cause");
  m.attr("FOREIGN_CHUNK_COLS") = (int)kChunkCols;
  m.attr("FOREIGN_FILE_COLS") = (int)kFileCols;
  m.attr("FOREIGN_RES_COLS") = (int)kResCols;
  m.attr("FOREIGN_CRC_PIECE") = (i64)kSpecCrcPiece;
}
