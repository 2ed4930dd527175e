// Batch collation core, shared host/device: gathers ragged rows of several
// decoded shards into padded dense tensors.
//
// A batch row is a (slot, row) pair into a window of decoded shards. Every
// output column is a flat array of B*T*L elements (FixedLen: T = 1, L = K;
// Padded: T = 1) cut into UNITS: one element for 8- and 4-byte columns, one
// aligned 8-byte word (eight elements) for byte columns. do_unit() produces
// one unit, and with it the per-row words of every row whose element 0 lies
// in the unit. The gfx950 kernel (csrc/hip/collate.hip) gives consecutive
// lanes consecutive units; the host build (ext.cpp host_collate, and
// csrc/tests/collate_selftest.cpp) loops over them. There is no second
// implementation of the semantics. Design notes: docs/KERNELS.md
// "collate_rows_kernel".
//
// Semantics per (column, row), count = values of the row (0 when absent):
//   FIXED     count == K copies; count == 0 fills `fill` when a default was
//             given, else MISSING; any other count is LENGTH
//   PADDED    copies min(count, L), pads the rest, len = min(count, L);
//             count > L counts the row as truncated or is LENGTH
//   PADDED2D  the PADDED rule at both levels: row -> outer items (lists of
//             a FeatureList, or strings of a bytes column) against T, each
//             item's elements against L; a row is truncated once
// The two PADDED2D sources differ only in which offset arrays are walked
// (list_off/sub_off or row_off/elem_off) and in the element size.
#pragma once

#include <cstdint>
#include <cstring>

#include "crc32c.h"  // TFR_HOSTDEV

namespace tfrec {
namespace collate {

using i32 = int32_t;
using i64 = int64_t;
using u32 = uint32_t;
using u64 = uint64_t;
using u8 = uint8_t;

enum Mode : int { CM_FIXED = 0, CM_PADDED = 1, CM_PADDED2D = 2 };

// Cause codes (the low byte of the status word).
enum Cause : int { CC_OK = 0, CC_MISSING = 1, CC_LENGTH = 2 };

enum Flags : int {
  CF_DEFAULT = 1,   // FIXED: `fill` is a default for absent/empty rows
  CF_TRUNCATE = 2,  // PADDED*: over-long rows are cut and counted
  CF_BYTES = 4,     // PADDED2D: walk row_off/elem_off (else list_off/sub_off)
};

// The six wire-form pointers of one column of one window slot
// (spark_tfrecord_amd/columnar.py WireColumn); table index slot*ncols + col.
struct Src {
  const u8* presence;
  const i64* row_off;
  const u8* values;
  const i64* elem_off;
  const i64* list_off;
  const i64* sub_off;
};
constexpr int kSrcWords = 6;

// One output column; twelve 8-byte words, built by collate.py.
struct Col {
  i64 mode;
  i64 esize;  // 8, 4 or 1
  i64 T;      // 1 unless PADDED2D
  i64 L;      // K for FIXED
  u64 fill;   // pad or default bits, in the low esize bytes
  i64 flags;
  u8* out;     // B*T*L elements
  i32* len;    // PADDED: [B]; PADDED2D: [B, T]; FIXED: null
  i32* outer;  // PADDED2D: [B]; else null
  i64 tile0;   // first tile of this column (the kernel's prefix table)
  i64 units;   // units in this column
  i64 rsv;
};
constexpr int kColWords = 12;
constexpr int kMaxCols = 64;
constexpr int kTileUnits = 1024;  // units per tile (256 lanes x 4)

// status[0]: min over bad cells of (b << 16) | (column << 8) | cause, all
// ones when clean; status[1]: truncated rows.
constexpr u64 kStatusClean = ~0ull;

struct Batch {
  const Src* src;
  const Col* cols;
  const i32* sel_slot;
  const i64* sel_row;
  i64 ncols;
  i64 B;
  u64* status;
};

// One (b, t) cell: n elements are copied from src, the rest is fill.
struct Cell {
  const u8* src;
  u32 n;
};

struct RowWords {
  i32 outer;  // PADDED2D: min(outer count, T)
  int cause;
  bool truncated;
};

TFR_HOSTDEV inline const Src& src_of(const Batch& bt, int c, u32 b, i64& r) {
  r = bt.sel_row[b];
  return bt.src[(i64)bt.sel_slot[b] * bt.ncols + c];
}

TFR_HOSTDEV inline Cell cell_of(const Batch& bt, int c, u32 b, u32 t) {
  const Col& col = bt.cols[c];
  i64 r;
  const Src& s = src_of(bt, c, b, r);
  Cell cell{nullptr, 0};
  if (!s.presence[r]) return cell;
  if (col.mode == CM_PADDED2D) {
    const bool by = col.flags & CF_BYTES;
    const i64* outer_off = by ? s.row_off : s.list_off;
    const i64* inner_off = by ? s.elem_off : s.sub_off;
    const i64 o0 = outer_off[r];
    if ((i64)t >= outer_off[r + 1] - o0) return cell;
    const i64 v0 = inner_off[o0 + t];
    const i64 n = inner_off[o0 + t + 1] - v0;
    cell.n = (u32)(n < col.L ? n : col.L);
    cell.src = s.values + v0 * col.esize;
    return cell;
  }
  const i64 v0 = s.row_off[r];
  const i64 n = s.row_off[r + 1] - v0;
  if (col.mode == CM_FIXED)
    cell.n = n == col.L ? (u32)n : 0u;
  else
    cell.n = (u32)(n < col.L ? n : col.L);
  cell.src = s.values + v0 * col.esize;
  return cell;
}

// Bits of output element j of a cell; a bit copy (memcpy, never a float
// move), so NaN payloads and negative zero survive.
TFR_HOSTDEV inline u64 cell_elem(const Col& col, const Cell& cell, u32 j) {
  if (j >= cell.n) return col.fill;
  if (col.esize == 8) {
    u64 v;
    __builtin_memcpy(&v, cell.src + (i64)j * 8, 8);
    return v;
  }
  if (col.esize == 4) {
    u32 v;
    __builtin_memcpy(&v, cell.src + (i64)j * 4, 4);
    return v;
  }
  return cell.src[j];
}

// Output element (column, b, t, j).
TFR_HOSTDEV inline u64 element(const Batch& bt, int c, u32 b, u32 t, u32 j) {
  return cell_elem(bt.cols[c], cell_of(bt, c, b, t), j);
}

// The per-row words of (column, b): outer count, error cause, truncation.
TFR_HOSTDEV inline RowWords row_words(const Batch& bt, int c, u32 b) {
  const Col& col = bt.cols[c];
  i64 r;
  const Src& s = src_of(bt, c, b, r);
  RowWords w{0, CC_OK, false};
  const bool present = s.presence[r] != 0;
  bool over = false;
  if (col.mode == CM_PADDED2D) {
    const bool by = col.flags & CF_BYTES;
    const i64* outer_off = by ? s.row_off : s.list_off;
    const i64* inner_off = by ? s.elem_off : s.sub_off;
    const i64 o0 = present ? outer_off[r] : 0;
    i64 oc = present ? outer_off[r + 1] - o0 : 0;
    if (oc > col.T) {
      over = true;
      oc = col.T;
    }
    w.outer = (i32)oc;
    for (i64 t = 0; t < oc; ++t)
      over |= inner_off[o0 + t + 1] - inner_off[o0 + t] > col.L;
  } else {
    const i64 n = present ? s.row_off[r + 1] - s.row_off[r] : 0;
    if (col.mode == CM_FIXED) {
      if (n == 0)
        w.cause = (col.flags & CF_DEFAULT) ? CC_OK : CC_MISSING;
      else if (n != col.L)
        w.cause = CC_LENGTH;
      return w;
    }
    over = n > col.L;
  }
  if (over) {
    if (col.flags & CF_TRUNCATE)
      w.truncated = true;
    else
      w.cause = CC_LENGTH;
  }
  return w;
}

// Side effects of the lane that owns element 0 of row b of column c. A row
// cut in several columns is counted by the first of them only, so the
// counter counts rows and takes at most B adds per batch.
template <class Ops>
TFR_HOSTDEV inline void emit_row(const Batch& bt, int c, u32 b) {
  const Col& col = bt.cols[c];
  const RowWords w = row_words(bt, c, b);
  if (col.outer) col.outer[b] = w.outer;
  if (w.cause)
    Ops::min64(bt.status, ((u64)b << 16) | ((u64)c << 8) | (u64)w.cause);
  if (w.truncated) {
    bool first = true;
    for (int p = 0; p < c && first; ++p)
      if (bt.cols[p].flags & CF_TRUNCATE)
        first = !row_words(bt, p, b).truncated;
    if (first) Ops::inc64(bt.status + 1);
  }
}

// Element 0 of cell (b, t): its length word, and for t == 0 the row's words.
template <class Ops>
TFR_HOSTDEV inline void emit_cell_head(const Batch& bt, int c, u32 b, u32 t,
                                       const Cell& cell) {
  const Col& col = bt.cols[c];
  if (col.len) col.len[(i64)b * col.T + t] = (i32)cell.n;
  if (t == 0) emit_row<Ops>(bt, c, b);
}

// Unit u of column c. The caller guarantees u < cols[c].units, and that
// B*T*L fits 31 bits (collate.py checks it), so the index split is 32-bit.
template <class Ops>
TFR_HOSTDEV inline void do_unit(const Batch& bt, int c, u32 u) {
  const Col& col = bt.cols[c];
  const u32 T = (u32)col.T, L = (u32)col.L;
  if (col.esize != 1) {
    const u32 j = u % L, bt_ = u / L;
    const u32 t = bt_ % T, b = bt_ / T;
    const Cell cell = cell_of(bt, c, b, t);
    const u64 v = cell_elem(col, cell, j);
    if (col.esize == 8) {
      reinterpret_cast<u64*>(col.out)[u] = v;
    } else {
      reinterpret_cast<u32*>(col.out)[u] = (u32)v;
    }
    if (j == 0) emit_cell_head<Ops>(bt, c, b, t, cell);
    return;
  }
  // eight consecutive bytes, which may span cells; the source bytes sit at
  // any alignment and are read one by one, the word is stored once
  const u32 total = (u32)bt.B * T * L;
  const u32 e0 = u * 8u;
  const u32 cnt = total - e0 < 8u ? total - e0 : 8u;
  u32 j = e0 % L, bt_ = e0 / L;
  u32 t = bt_ % T, b = bt_ / T;
  Cell cell = cell_of(bt, c, b, t);
  u64 word = 0;
  for (u32 k = 0; k < cnt; ++k) {
    if (j == 0) {
      if (k) cell = cell_of(bt, c, b, t);
      emit_cell_head<Ops>(bt, c, b, t, cell);
    }
    word |= cell_elem(col, cell, j) << (8 * k);
    if (++j == L) {
      j = 0;
      if (++t == T) {
        t = 0;
        ++b;
      }
    }
  }
  if (cnt == 8) {
    reinterpret_cast<u64*>(col.out)[u] = word;
  } else {
    for (u32 k = 0; k < cnt; ++k) col.out[e0 + k] = (u8)(word >> (8 * k));
  }
}

// Host atomics: the host path is one thread.
struct HostOps {
  static void min64(u64* p, u64 v) {
    if (v < *p) *p = v;
  }
  static void inc64(u64* p) { *p += 1; }
};

inline void host_run(const Batch& bt) {
  for (int c = 0; c < (int)bt.ncols; ++c)
    for (i64 u = 0; u < bt.cols[c].units; ++u) do_unit<HostOps>(bt, c, (u32)u);
}

}  // namespace collate
}  // namespace tfrec
