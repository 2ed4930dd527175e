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
//
// Packed (values + offsets) columns add two launches per batch, however many
// of them there are, and no host wait:
//
//   ragged_offsets_kernel  one 256-lane block per ragged column scans the
//                          rows' (items, values) counts in batch order: four
//                          consecutive rows per lane, a 64-wide shuffle scan
//                          per wave, four wave totals through LDS, a running
//                          carry over passes of 1024 rows. Writes the raw
//                          64-bit offsets (scratch), the clamped int32
//                          offsets, CAPACITY and the cut-row count.
//   ragged_gather_kernel   (column, tile) grid-stride like the dense kernel,
//                          1024 units per tile over the whole capacity (so
//                          the zero tail is written here too). The unit ->
//                          batch row map is staged in LDS per tile: two
//                          wave-uniform binary searches bound the tile's
//                          rows, each row that covers a unit of the tile
//                          marks the first such unit with its RowRef, and a
//                          max-scan over the 1024 marks hands every unit the
//                          mark at or before it. A lane then does no
//                          dependent global load before its value load. A
//                          RAGGED2D tile runs the same map a second time
//                          over the item offsets for its item_offsets units.
//                          Byte columns: one aligned 8-byte word per lane,
//                          two aligned loads and a funnel shift.
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

// ---------------------------------------------------------------------------
// packed columns
// ---------------------------------------------------------------------------

constexpr int kRowsPerLane = 4;

__device__ inline i64 shfl_up64(i64 v, int d) {
  return (i64)__shfl_up((long long)v, (unsigned)d, 64);
}

__global__ void __launch_bounds__(kThreads) ragged_offsets_kernel(Batch bt) {
  // this block's column: the blockIdx.x-th ragged one
  int c = 0;
  for (int k = 0, seen = 0; k < (int)bt.ncols; ++k)
    if (is_ragged(bt.cols[k]) && seen++ == (int)blockIdx.x) c = k;
  __shared__ i64 wave_v[kThreads / 64], wave_i[kThreads / 64];
  const u32 B = (u32)bt.B;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) ragged_row0<DevOps>(bt, c);
  i64 carry_v = 0, carry_i = 0;
  for (u32 base = 0; base < B; base += kThreads * kRowsPerLane) {
    const u32 b0 = base + threadIdx.x * kRowsPerLane;
    // loads only: the four rows' lookups are independent and overlap
    Counts n[kRowsPerLane];
    i64 lv = 0, li = 0;
#pragma unroll
    for (int k = 0; k < kRowsPerLane; ++k) {
      n[k] = b0 + k < B ? row_counts(bt, c, b0 + k) : Counts{0, 0, false};
      lv += n[k].values;
      li += n[k].items;
    }
    i64 sv = lv, si = li;  // inclusive over the wave, 64-bit throughout
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const i64 tv = shfl_up64(sv, d), ti = shfl_up64(si, d);
      if (lane >= d) {
        sv += tv;
        si += ti;
      }
    }
    if (lane == 63) {
      wave_v[wave] = sv;
      wave_i[wave] = si;
    }
    __syncthreads();
    i64 ev = carry_v + sv - lv, ei = carry_i + si - li;  // before row b0
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
      if (w < wave) {
        ev += wave_v[w];
        ei += wave_i[w];
      }
      carry_v += wave_v[w];
      carry_i += wave_i[w];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kRowsPerLane; ++k)
      if (b0 + k < B) {
        ev += n[k].values;
        ei += n[k].items;
        ragged_row<DevOps>(bt, c, b0 + k, n[k], ev, ei);
      }
  }
}

// The tile's unit -> row map, and its units. ITEMS: positions are items and
// units item_offsets entries; else positions are values and a unit is g of
// them (g = 8 for byte columns, else 1).
struct TileMap {
  i32 seg[kTileUnits];   // the mark at or before each unit, -1: none
  u32 row[kTileUnits];   // per mark: the batch row
  u64 addr[kTileUnits];  // per mark: the row's RowRef
  i64 aux[kTileUnits];
  i32 wave_max[kThreads / 64];
};

template <bool ITEMS>
__device__ inline void ragged_tile(const Batch& bt, int c, i64 u0, i64 nunits,
                                   TileMap& m) {
  const Col& col = bt.cols[c];
  const u32 B = (u32)bt.B;
  const i64* off = ITEMS ? col.raw + B + 1 : col.raw;
  const i64 g = (!ITEMS && col.esize == 1) ? 8 : 1;
  const i64 total = off[B];
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < kTileUnits / kThreads; ++k) m.seg[t + k * kThreads] = -1;
  __syncthreads();
  const i64 p0 = u0 * g, p1 = (u0 + kTileUnits) * g;
  if (p0 < total) {
    // the rows at the tile's two ends: the same search in every lane
    const u32 b_lo = find_row(off, B, p0);
    const u32 b_hi = find_row(off, B, (p1 < total ? p1 : total) - 1);
    for (u32 b = b_lo + t; b <= b_hi; b += kThreads) {
      const i64 s = off[b], e = off[b + 1];
      i64 w = (s + g - 1) / g;  // the row's first unit start
      if (w < u0) w = u0;
      // exactly one row covers a unit's first position: no two rows mark
      // the same unit, and empty rows mark none
      if (w * g < e && w < u0 + kTileUnits) {
        const int i = (int)(w - u0);
        const RowRef rr = ITEMS ? item_ref(bt, c, b) : value_ref(bt, c, b);
        m.seg[i] = i;
        m.row[i] = b;
        m.addr[i] = rr.addr;
        m.aux[i] = rr.aux;
      }
    }
  }
  __syncthreads();
  // inclusive max-scan of the marks: four consecutive units per lane
  const int lane = t & 63, wave = t >> 6;
  i32 loc[kTileUnits / kThreads];
  i32 run = -1;
#pragma unroll
  for (int k = 0; k < kTileUnits / kThreads; ++k) {
    const i32 v = m.seg[t * (kTileUnits / kThreads) + k];
    run = v > run ? v : run;
    loc[k] = run;
  }
  i32 inc = run;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const i32 o = __shfl_up(inc, (unsigned)d, 64);
    if (lane >= d && o > inc) inc = o;
  }
  i32 before = __shfl_up(inc, 1u, 64);
  if (lane == 0) before = -1;
  if (lane == 63) m.wave_max[wave] = inc;
  __syncthreads();
  for (int w = 0; w < wave; ++w)
    if (m.wave_max[w] > before) before = m.wave_max[w];
#pragma unroll
  for (int k = 0; k < kTileUnits / kThreads; ++k)
    m.seg[t * (kTileUnits / kThreads) + k] = loc[k] > before ? loc[k] : before;
  __syncthreads();
  // consecutive lanes, consecutive units
#pragma unroll
  for (int k = 0; k < kTileUnits / kThreads; ++k) {
    const int i = t + k * kThreads;
    const i64 u = u0 + i;
    if (u >= nunits) continue;
    const i32 sg = m.seg[i];
    RowRef rr{0, 0};
    u32 b = 0;
    if (sg >= 0) {
      rr = RowRef{m.addr[sg], m.aux[sg]};
      b = m.row[sg];
    }
    if (ITEMS)
      ragged_item_unit(bt, c, (u32)u, rr);
    else
      ragged_value_unit<DevOps, true>(bt, c, (u32)u, b, rr);
  }
  __syncthreads();  // the map is reused
}

__global__ void __launch_bounds__(kThreads) ragged_gather_kernel(
    Batch bt, i64 ntiles) {
  __shared__ TileMap m;
  for (i64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int c = 0;
    while (c + 1 < (int)bt.ncols && bt.cols[c + 1].rtile0 <= tile) ++c;
    const Col& col = bt.cols[c];
    const i64 u0 = (tile - col.rtile0) * kTileUnits;
    const i64 vunits = value_units(col);
    if (u0 < vunits) ragged_tile<false>(bt, c, u0, vunits, m);
    if (col.mode == CM_RAGGED2D && u0 <= col.icap)
      ragged_tile<true>(bt, c, u0, col.icap + 1, m);
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

// The packed columns of the same tables: the offsets scan (one block per
// ragged column), then the gather over their rtiles tiles. Same trust.
void gpu_collate_ragged(uintptr_t src, uintptr_t cols, uintptr_t sel_slot,
                        uintptr_t sel_row, i64 ncols, i64 B, i64 nragged,
                        i64 rtiles, uintptr_t status, uintptr_t stream) {
  if (B <= 0 || ncols <= 0 || nragged <= 0 || rtiles <= 0) return;
  if (ncols > kMaxCols || nragged > ncols)
    throw std::invalid_argument("gpu_collate_ragged: more than 64 columns");
  Batch bt{(const Src*)src, (const Col*)cols, (const i32*)sel_slot,
           (const i64*)sel_row, ncols, B, (u64*)status};
  hipLaunchKernelGGL(ragged_offsets_kernel, dim3((uint32_t)nragged),
                     dim3(kThreads), 0, (hipStream_t)stream, bt);
  HIPC_CHECK(hipGetLastError());
  const i64 blocks = rtiles < kMaxBlocks ? rtiles : kMaxBlocks;
  hipLaunchKernelGGL(ragged_gather_kernel, dim3((uint32_t)blocks),
                     dim3(kThreads), 0, (hipStream_t)stream, bt, rtiles);
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
  m.def("gpu_collate_ragged", &gpu_collate_ragged, py::arg("src"),
        py::arg("cols"), py::arg("sel_slot"), py::arg("sel_row"),
        py::arg("ncols"), py::arg("B"), py::arg("nragged"), py::arg("rtiles"),
        py::arg("status"), py::arg("stream"),
        "The Ragged / Ragged2D columns of the same tables, two launches: "
        "batch-order offsets (scan), then values and item offsets (gather)");
}
