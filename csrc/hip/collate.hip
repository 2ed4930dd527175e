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
//                          over the item offsets for its item_offsets units,
//                          a RAGGED3D tile a third time over the step
//                          offsets for its step_offsets units.
//                          Byte columns: one aligned 8-byte word per lane,
//                          two aligned loads and a funnel shift.
//
// Three-level dense columns (a FeatureList of bytes as [B, S, T, L]) add one
// launch per batch, however many of them there are:
//
//   collate_cells3d_kernel (column, tile) grid-stride over 1024-word tiles.
//                          Phase one stages the tile's cell table in LDS: a
//                          lane per (b, s, t) cell walks selection ->
//                          presence -> list_off -> sub_off -> elem_off once
//                          and keeps the source address and clamped length;
//                          cell owners write len / outer / steps and the
//                          row's error or truncation. Phase two: every lane
//                          finds its word's cell by a division, reads a word
//                          inside one string as two aligned loads and a
//                          funnel shift, builds padding without a load, and
//                          assembles boundary words from the table. Tiles of
//                          more than 1024 cells (L < 8) take the core's
//                          per-unit walk.
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
  __shared__ i64 wave_v[kThreads / 64], wave_i[kThreads / 64],
      wave_s[kThreads / 64];
  const u32 B = (u32)bt.B;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) ragged_row0<DevOps>(bt, c);
  i64 carry_v = 0, carry_i = 0, carry_s = 0;
  for (u32 base = 0; base < B; base += kThreads * kRowsPerLane) {
    const u32 b0 = base + threadIdx.x * kRowsPerLane;
    // loads only: the four rows' lookups are independent and overlap
    Counts n[kRowsPerLane];
    i64 lv = 0, li = 0, ls = 0;
#pragma unroll
    for (int k = 0; k < kRowsPerLane; ++k) {
      n[k] = b0 + k < B ? row_counts(bt, c, b0 + k) : Counts{0, 0, 0, false};
      lv += n[k].values;
      li += n[k].items;
      ls += n[k].steps;
    }
    // inclusive over the wave, 64-bit throughout
    i64 sv = lv, si = li, ss = ls;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const i64 tv = shfl_up64(sv, d), ti = shfl_up64(si, d),
                ts = shfl_up64(ss, d);
      if (lane >= d) {
        sv += tv;
        si += ti;
        ss += ts;
      }
    }
    if (lane == 63) {
      wave_v[wave] = sv;
      wave_i[wave] = si;
      wave_s[wave] = ss;
    }
    __syncthreads();
    // before row b0
    i64 ev = carry_v + sv - lv, ei = carry_i + si - li,
        es = carry_s + ss - ls;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
      if (w < wave) {
        ev += wave_v[w];
        ei += wave_i[w];
        es += wave_s[w];
      }
      carry_v += wave_v[w];
      carry_i += wave_i[w];
      carry_s += wave_s[w];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kRowsPerLane; ++k)
      if (b0 + k < B) {
        ev += n[k].values;
        ei += n[k].items;
        es += n[k].steps;
        ragged_row<DevOps>(bt, c, b0 + k, n[k], ev, ei, es);
      }
  }
}

// The tile's unit -> row map, and its units. LEVEL 1: positions are items and
// units item_offsets entries; LEVEL 2: steps and step_offsets entries; LEVEL
// 0: positions are values and a unit is g of them (g = 8 for byte columns,
// else 1).
struct TileMap {
  i32 seg[kTileUnits];   // the mark at or before each unit, -1: none
  u32 row[kTileUnits];   // per mark: the batch row
  u64 addr[kTileUnits];  // per mark: the row's RowRef
  i64 aux[kTileUnits];
  i32 wave_max[kThreads / 64];
};

template <int LEVEL>
__device__ inline void ragged_tile(const Batch& bt, int c, i64 u0, i64 nunits,
                                   TileMap& m) {
  const Col& col = bt.cols[c];
  const u32 B = (u32)bt.B;
  const i64* off = col.raw + LEVEL * (B + 1);
  const i64 g = (LEVEL == 0 && col.esize == 1) ? 8 : 1;
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
        const RowRef rr = LEVEL == 2   ? step_ref(bt, c, b)
                          : LEVEL == 1 ? item_ref(bt, c, b)
                                       : value_ref(bt, c, b);
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
    if (LEVEL == 2)
      ragged_step_unit(bt, c, (u32)u, rr);
    else if (LEVEL == 1)
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
    if (u0 < vunits) ragged_tile<0>(bt, c, u0, vunits, m);
    if (col.mode != CM_RAGGED && u0 <= col.icap)
      ragged_tile<1>(bt, c, u0, col.icap + 1, m);
    if (col.mode == CM_RAGGED3D && u0 <= col.scap)
      ragged_tile<2>(bt, c, u0, col.scap + 1, m);
  }
}

// ---------------------------------------------------------------------------
// three-level dense columns (PADDED3D)
// ---------------------------------------------------------------------------

// A tile is kTileUnits aligned 8-byte words of one column's [B, S, T, L]
// bytes. Its cell table holds, for every cell (b, s, t) the tile's byte range
// touches, the cell's first source byte and its clamped length: the five
// dependent loads from the selection to the string are walked once per cell,
// by one lane, and every word of the tile then finds its cell by a division
// and two LDS reads. kCells is what a tile touches at L = 8, the smallest L
// at which a word can lie inside one cell; from L = 9 on no tile touches
// more (at most 8190 / L + 2 cells), below L = 8 a full tile does and takes
// the core's per-unit walk.
constexpr int kCells = 1024;

struct CellTable {
  u64 addr[kCells];
  u32 n[kCells];
};

__device__ inline u64 pad_word(const Col& col) {
  return (col.fill & 0xFFull) * 0x0101010101010101ull;
}

__global__ void __launch_bounds__(kThreads) collate_cells3d_kernel(
    Batch bt, i64 ntiles) {
  __shared__ CellTable m;
  const int t = threadIdx.x;
  for (i64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int c = 0;
    while (c + 1 < (int)bt.ncols && bt.cols[c + 1].ctile0 <= tile) ++c;
    const Col& col = bt.cols[c];
    const u32 L = (u32)col.L;
    const u32 total = (u32)bt.B * (u32)col.S * (u32)col.T * L;
    const u32 u0 = (u32)(tile - col.ctile0) * kTileUnits;
    const u32 p0 = u0 * 8u;  // p0 < total: the column has this tile
    const u32 p1 = total - p0 < 8u * kTileUnits ? total : p0 + 8u * kTileUnits;
    const u32 g0 = p0 / L, ncells = (p1 - 1) / L - g0 + 1;
    if (ncells > (u32)kCells) {
      // wave-uniform: the whole block takes the walk for this tile
#pragma unroll
      for (int k = 0; k < kTileUnits / kThreads; ++k) {
        const u32 u = u0 + t + k * kThreads;
        if ((i64)u < col.units) unit3d<DevOps>(bt, c, u);
      }
      continue;
    }
    // phase one: a lane per cell. The tile that holds a cell's byte 0 owns
    // the cell's words; a cell that began in the tile before is only read.
    for (u32 i = t; i < ncells; i += kThreads) {
      const u32 g = g0 + i;
      const Cell3 x = cell3_of(bt, c, g);
      m.addr[i] = x.addr;
      m.n[i] = x.n;
      if (g * L >= p0) emit_cell3_head<DevOps>(bt, c, g, x);
    }
    __syncthreads();
    // phase two: consecutive lanes, consecutive words; no global load
    // stands before a lane's value loads
    const u64 pad = pad_word(col);
#pragma unroll
    for (int k = 0; k < kTileUnits / kThreads; ++k) {
      const u32 u = u0 + t + k * kThreads;
      const u32 p = u * 8u;
      if (p >= total) continue;
      const u32 cnt = total - p < 8u ? total - p : 8u;
      u32 g = p / L, j = p - g * L, i = g - g0;
      u32 n = m.n[i];
      u64 a = m.addr[i];
      u64 word;
      if (j + 8u <= n) {
        // all eight bytes lie in the source string: two aligned loads
        a += j;
        const u32 mis = (u32)(a & 7);
        const u64* q = reinterpret_cast<const u64*>(a - mis);
        word = q[0];
        if (mis) word = (word >> (8 * mis)) | (q[1] << (64 - 8 * mis));
      } else if (j >= n && j + 8u <= L) {
        word = pad;
      } else {
        // a cell boundary or the cell's n boundary inside the word
        word = 0;
        for (u32 e = 0; e < cnt; ++e) {
          const u8 byte = j < n ? *(const u8*)(a + j) : (u8)pad;
          word |= (u64)byte << (8 * e);
          if (++j == L && e + 1 < cnt) {
            j = 0;
            ++i;
            n = m.n[i];
            a = m.addr[i];
          }
        }
      }
      if (cnt == 8) {
        reinterpret_cast<u64*>(col.out)[u] = word;
      } else {
        for (u32 e = 0; e < cnt; ++e) col.out[p + e] = (u8)(word >> (8 * e));
      }
    }
    __syncthreads();  // the table is reused
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

// The Padded3D columns of the same tables, one launch over their ctiles
// tiles. Same trust.
void gpu_collate_cells3d(uintptr_t src, uintptr_t cols, uintptr_t sel_slot,
                         uintptr_t sel_row, i64 ncols, i64 B, i64 ctiles,
                         uintptr_t status, uintptr_t stream) {
  if (B <= 0 || ncols <= 0 || ctiles <= 0) return;
  if (ncols > kMaxCols)
    throw std::invalid_argument("gpu_collate_cells3d: more than 64 columns");
  Batch bt{(const Src*)src, (const Col*)cols, (const i32*)sel_slot,
           (const i64*)sel_row, ncols, B, (u64*)status};
  const i64 blocks = ctiles < kMaxBlocks ? ctiles : kMaxBlocks;
  hipLaunchKernelGGL(collate_cells3d_kernel, dim3((uint32_t)blocks),
                     dim3(kThreads), 0, (hipStream_t)stream, bt, ctiles);
  HIPC_CHECK(hipGetLastError());
}

}  // namespace

void register_collate(py::module_& m) {
  m.def("gpu_collate_cells3d", &gpu_collate_cells3d, py::arg("src"),
        py::arg("cols"), py::arg("sel_slot"), py::arg("sel_row"),
        py::arg("ncols"), py::arg("B"), py::arg("ctiles"), py::arg("status"),
        py::arg("stream"),
        "The Padded3D columns of the same tables, one launch: a cell table "
        "staged in LDS per tile, then one aligned 8-byte word per lane");
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
