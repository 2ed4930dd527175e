// Batch collation core, shared host/device: gathers ragged rows of several
// decoded shards into padded dense tensors, or into packed values + offsets.
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
//   PADDED3D  a FeatureList of bytes, the PADDED rule at three levels: row ->
//             steps against S, a step's strings against T, a string's bytes
//             against L; steps[B], outer[B, S], len[B, S, T]; a row over any
//             bound is truncated once, or is LENGTH; an absent row is all
//             padding with zero lengths
// The two PADDED2D sources differ only in which offset arrays are walked
// (list_off/sub_off or row_off/elem_off) and in the element size.
//
// The packed modes keep the wire form's shape, re-based to the batch:
//   RAGGED    the rows' values back to back in `cap` elements, offsets[B+1];
//             a row is cut to its first L values (counted as truncated)
//   RAGGED2D  the rows' items (lists or strings) back to back: values in
//             `cap` elements, item_offsets[icap+1], offsets[B+1] over items
//   RAGGED3D  a FeatureList of bytes, one level more: bytes in `cap`,
//             item_offsets[icap+1] over the strings, step_offsets[scap+1]
//             into the strings, offsets[B+1] over the steps; CAPACITY at the
//             first row whose end passes any of the three capacities
// They run in two steps. Step one gives every row its raw 64-bit offsets in
// batch order (row_counts + a prefix sum: serial on the host, a block scan on
// the device) and ragged_row() writes them, the clamped int32 offsets, and
// raises CAPACITY at the first row whose end passes a capacity. Step two cuts
// the capacity into units like the dense columns; ragged_value_unit() and
// ragged_item_unit() produce one unit from the RowRef of the batch row its
// first position lies in (the caller finds that row: a cursor on the host, a
// map staged in LDS on the device). Offsets are min(raw, capacity), values
// past the batch's total are zero, item offsets past the last item repeat
// the total: every output byte is defined, on errors too.
//
// osize 4 on an 8-byte column narrows int64 to int32 in the store; a copied
// value outside int32 raises RANGE and its low 32 bits are stored.
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

enum Mode : int {
  CM_FIXED = 0,
  CM_PADDED = 1,
  CM_PADDED2D = 2,
  CM_RAGGED = 3,
  CM_RAGGED2D = 4,
  CM_RAGGED3D = 5,
  CM_PADDED3D = 6,
};

// Cause codes (the low byte of the status word).
enum Cause : int {
  CC_OK = 0,
  CC_MISSING = 1,
  CC_LENGTH = 2,
  CC_RANGE = 3,     // an int64 value does not fit the int32 output
  CC_CAPACITY = 4,  // RAGGED*: the batch's total passes a capacity
};

enum Flags : int {
  CF_DEFAULT = 1,   // FIXED: `fill` is a default for absent/empty rows
  CF_TRUNCATE = 2,  // PADDED*, RAGGED: over-long rows are cut and counted
  CF_BYTES = 4,     // *2D: walk row_off/elem_off (else list_off/sub_off)
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

// One output column; twenty 8-byte words, built by collate.py. The dense
// kernel, the ragged gather kernel and the three-level dense kernel each walk
// their own tile prefix (tile0, rtile0, ctile0); a column has tiles in one.
struct Col {
  i64 mode;
  i64 esize;  // source element: 8, 4 or 1
  i64 T;      // 1 unless PADDED2D / PADDED3D
  i64 L;      // K for FIXED; RAGGED: max_len (huge when there is none)
  u64 fill;   // pad or default bits, in the low esize bytes
  i64 flags;
  u8* out;     // dense: B*T*L elements; RAGGED*: cap elements
  i32* len;    // PADDED: [B]; PADDED2D: [B, T]; PADDED3D: [B, S, T];
               // RAGGED*: offsets [B+1]
  i32* outer;  // PADDED2D: [B]; PADDED3D: [B, S]; RAGGED2D/3D: item_offsets
               // [icap+1]; else null
  i64 tile0;   // first tile of this column in the dense kernel
  i64 units;   // units in this column
  i64 osize;   // output element: 0 or esize, or 4 when int64 narrows to int32
  i64* raw;    // RAGGED*: scratch, raw value offsets [B+1], then (RAGGED2D/3D)
               // raw item offsets [B+1], then (RAGGED3D) raw step offsets
  i64 cap;     // RAGGED*: value capacity
  i64 icap;    // RAGGED2D/3D: item capacity
  i64 rtile0;  // first tile of this column in the ragged gather kernel
  i64 S;       // PADDED3D: max steps; else 1
  i32* steps;  // PADDED3D: [B]; RAGGED3D: step_offsets [scap+1]; else null
  i64 scap;    // RAGGED3D: step capacity
  i64 ctile0;  // first tile of this column in the three-level dense kernel
};
constexpr int kColWords = 20;
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
  i32 outer;  // PADDED2D: min(outer count, T); PADDED3D: min(steps, S)
  int cause;
  bool truncated;
};

// int64 values are stored as int32. osize was a reserved zero word once: a
// descriptor that leaves it 0 stores esize bytes, as before.
TFR_HOSTDEV inline bool narrows(const Col& col) {
  return col.esize == 8 && col.osize == 4;
}

TFR_HOSTDEV inline bool is_ragged(const Col& col) {
  return col.mode >= CM_RAGGED && col.mode <= CM_RAGGED3D;
}

TFR_HOSTDEV inline i64 min64v(i64 a, i64 b) { return a < b ? a : b; }

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

// Raw counts of row b of a RAGGED* column: its steps (RAGGED3D), its items
// (RAGGED2D/3D) and its values, after the max_len cut (RAGGED). Absent and
// empty rows are 0.
struct Counts {
  i64 items;
  i64 values;
  i64 steps;
  bool cut;
};

TFR_HOSTDEV inline Counts row_counts(const Batch& bt, int c, u32 b) {
  const Col& col = bt.cols[c];
  i64 r;
  const Src& s = src_of(bt, c, b, r);
  Counts n{0, 0, 0, false};
  if (!s.presence[r]) return n;
  if (col.mode == CM_RAGGED) {
    const i64 v = s.row_off[r + 1] - s.row_off[r];
    n.cut = v > col.L;
    n.values = n.cut ? col.L : v;
    return n;
  }
  if (col.mode == CM_RAGGED3D) {
    const i64 l0 = s.list_off[r];
    n.steps = s.list_off[r + 1] - l0;
    const i64 e0 = s.sub_off[l0], e1 = s.sub_off[l0 + n.steps];
    n.items = e1 - e0;
    n.values = s.elem_off[e1] - s.elem_off[e0];
    return n;
  }
  const bool by = col.flags & CF_BYTES;
  const i64* outer_off = by ? s.row_off : s.list_off;
  const i64* inner_off = by ? s.elem_off : s.sub_off;
  const i64 o0 = outer_off[r];
  n.items = outer_off[r + 1] - o0;
  n.values = inner_off[o0 + n.items] - inner_off[o0];
  return n;
}

// The per-row words of (column, b): outer count, error cause, truncation.
TFR_HOSTDEV inline RowWords row_words(const Batch& bt, int c, u32 b) {
  const Col& col = bt.cols[c];
  RowWords w{0, CC_OK, false};
  if (is_ragged(col)) {
    w.truncated = row_counts(bt, c, b).cut;
    return w;
  }
  i64 r;
  const Src& s = src_of(bt, c, b, r);
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
  } else if (col.mode == CM_PADDED3D) {
    const i64 l0 = present ? s.list_off[r] : 0;
    i64 ns = present ? s.list_off[r + 1] - l0 : 0;
    if (ns > col.S) {
      over = true;
      ns = col.S;
    }
    w.outer = (i32)ns;  // the row's steps
    for (i64 k = 0; k < ns; ++k) {
      const i64 e0 = s.sub_off[l0 + k];
      i64 ne = s.sub_off[l0 + k + 1] - e0;
      if (ne > col.T) {
        over = true;
        ne = col.T;
      }
      for (i64 t = 0; t < ne; ++t)
        over |= s.elem_off[e0 + t + 1] - s.elem_off[e0 + t] > col.L;
    }
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

template <class Ops>
TFR_HOSTDEV inline void raise(const Batch& bt, int c, u32 b, int cause) {
  Ops::min64(bt.status, ((u64)b << 16) | ((u64)c << 8) | (u64)cause);
}

// Row b is cut in column c. A row cut in several columns is counted by the
// first of them only, so the counter counts rows and takes at most B adds
// per batch.
template <class Ops>
TFR_HOSTDEV inline void count_cut(const Batch& bt, int c, u32 b) {
  bool first = true;
  for (int p = 0; p < c && first; ++p)
    if (bt.cols[p].flags & CF_TRUNCATE)
      first = !row_words(bt, p, b).truncated;
  if (first) Ops::inc64(bt.status + 1);
}

// Side effects of the lane that owns element 0 of row b of dense column c.
template <class Ops>
TFR_HOSTDEV inline void emit_row(const Batch& bt, int c, u32 b) {
  const Col& col = bt.cols[c];
  const RowWords w = row_words(bt, c, b);
  if (col.outer) col.outer[b] = w.outer;
  if (w.cause) raise<Ops>(bt, c, b, w.cause);
  if (w.truncated) count_cut<Ops>(bt, c, b);
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
    if (col.esize == 8 && !narrows(col)) {
      reinterpret_cast<u64*>(col.out)[u] = v;
    } else {
      if (narrows(col) && j < cell.n && (i64)v != (i64)(i32)v)
        raise<Ops>(bt, c, b, CC_RANGE);
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

// ---------------------------------------------------------------------------
// PADDED3D: cells are numbered g = (b*S + s)*T + t over the whole column
// ---------------------------------------------------------------------------

// Cell g after one walk selection -> presence -> list_off -> sub_off ->
// elem_off: its first source byte (kept as an integer; 0 where there is no
// string), its clamped length, and the clamped counts of its row and step.
struct Cell3 {
  u64 addr;
  u32 n;
  i32 steps;  // min(steps of the row, S)
  i32 outer;  // min(strings of the step, T), 0 past the row's steps
};

TFR_HOSTDEV inline Cell3 cell3_of(const Batch& bt, int c, u32 g) {
  const Col& col = bt.cols[c];
  const u32 T = (u32)col.T, ST = (u32)col.S * T;
  const u32 b = g / ST, st = g % ST, s = st / T, t = st % T;
  i64 r;
  const Src& sr = src_of(bt, c, b, r);
  Cell3 x{0, 0, 0, 0};
  if (!sr.presence[r]) return x;
  const i64 l0 = sr.list_off[r];
  const i64 ns = sr.list_off[r + 1] - l0;
  x.steps = (i32)min64v(ns, col.S);
  if ((i64)s >= ns) return x;
  const i64 e0 = sr.sub_off[l0 + s];
  const i64 ne = sr.sub_off[l0 + s + 1] - e0;
  x.outer = (i32)min64v(ne, col.T);
  if ((i64)t >= ne) return x;
  const i64 v0 = sr.elem_off[e0 + t];
  x.n = (u32)min64v(sr.elem_off[e0 + t + 1] - v0, col.L);
  x.addr = (u64)sr.values + (u64)v0;
  return x;
}

// Side effects of whoever owns byte 0 of cell g: the cell's length word, the
// step's word for a step's first cell, the row's words for a row's first.
template <class Ops>
TFR_HOSTDEV inline void emit_cell3_head(const Batch& bt, int c, u32 g,
                                        const Cell3& x) {
  const Col& col = bt.cols[c];
  const u32 T = (u32)col.T, ST = (u32)col.S * T;
  col.len[g] = (i32)x.n;
  if (g % T) return;
  col.outer[g / T] = x.outer;
  if (g % ST) return;
  const u32 b = g / ST;
  col.steps[b] = x.steps;
  const RowWords w = row_words(bt, c, b);
  if (w.cause) raise<Ops>(bt, c, b, w.cause);
  if (w.truncated) count_cut<Ops>(bt, c, b);
}

// Unit u (one 8-byte word) of PADDED3D column c by a walk of its own: the
// host path, and the device's for tiles of more cells than its table holds.
// The caller guarantees u < cols[c].units and that B*S*T*L fits 31 bits.
template <class Ops>
TFR_HOSTDEV inline void unit3d(const Batch& bt, int c, u32 u) {
  const Col& col = bt.cols[c];
  const u32 L = (u32)col.L;
  const u32 total = (u32)bt.B * (u32)col.S * (u32)col.T * L;
  const u32 e0 = u * 8u;
  const u32 cnt = total - e0 < 8u ? total - e0 : 8u;
  u32 g = e0 / L, j = e0 % L;
  Cell3 x = cell3_of(bt, c, g);
  u64 word = 0;
  for (u32 k = 0; k < cnt; ++k) {
    if (j == 0) {
      if (k) x = cell3_of(bt, c, g);
      emit_cell3_head<Ops>(bt, c, g, x);
    }
    const u8 byte = j < x.n ? *(const u8*)(x.addr + j) : (u8)col.fill;
    word |= (u64)byte << (8 * k);
    if (++j == L) {
      j = 0;
      ++g;
    }
  }
  if (cnt == 8) {
    reinterpret_cast<u64*>(col.out)[u] = word;
  } else {
    for (u32 k = 0; k < cnt; ++k) col.out[e0 + k] = (u8)(word >> (8 * k));
  }
}

// ---------------------------------------------------------------------------
// RAGGED / RAGGED2D / RAGGED3D
// ---------------------------------------------------------------------------

// Value units of a ragged column: elements, or 8-byte words of a byte column.
TFR_HOSTDEV inline i64 value_units(const Col& col) {
  return col.esize == 1 ? (col.cap + 7) / 8 : col.cap;
}

// Step one, per row: n are the row's counts, v_end / i_end / s_end the
// inclusive prefix sums of values / items / steps over the batch rows up to b.
template <class Ops>
TFR_HOSTDEV inline void ragged_row(const Batch& bt, int c, u32 b,
                                   const Counts& n, i64 v_end, i64 i_end,
                                   i64 s_end) {
  const Col& col = bt.cols[c];
  const bool three = col.mode == CM_RAGGED3D;
  const bool two = three || col.mode == CM_RAGGED2D;
  col.raw[b + 1] = v_end;
  if (two) col.raw[bt.B + 1 + b + 1] = i_end;
  if (three) col.raw[2 * (bt.B + 1) + b + 1] = s_end;
  col.len[b + 1] = (i32)(three ? min64v(s_end, col.scap)
                         : two ? min64v(i_end, col.icap)
                               : min64v(v_end, col.cap));
  // the first row whose end passes a capacity; its start did not
  const bool over_v = v_end > col.cap && v_end - n.values <= col.cap;
  const bool over_i = two && i_end > col.icap && i_end - n.items <= col.icap;
  const bool over_s = three && s_end > col.scap && s_end - n.steps <= col.scap;
  if (over_v || over_i || over_s) raise<Ops>(bt, c, b, CC_CAPACITY);
  if (n.cut) count_cut<Ops>(bt, c, b);
}

template <class Ops>
TFR_HOSTDEV inline void ragged_row0(const Batch& bt, int c) {
  const Col& col = bt.cols[c];
  col.raw[0] = 0;
  if (col.mode != CM_RAGGED) col.raw[bt.B + 1] = 0;
  if (col.mode == CM_RAGGED3D) col.raw[2 * (bt.B + 1)] = 0;
  col.len[0] = 0;
}

// Largest b with off[b] <= p, for 0 <= p < off[B]: the (non-empty) row that
// position p lies in.
TFR_HOSTDEV inline u32 find_row(const i64* off, u32 B, i64 p) {
  u32 lo = 0, hi = B;
  while (hi - lo > 1) {
    const u32 mid = lo + (hi - lo) / 2;
    if (off[mid] <= p)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// What a unit needs of the batch row its first position lies in. Values:
// position p of the batch is read at addr + p*esize, aux is the row's raw
// end. Items: the raw value offset of item q is *(i64*)(addr + q*8) + aux;
// steps: the raw item offset of step q, likewise.
// The address is kept as an integer: it may lie before its array.
struct RowRef {
  u64 addr;
  i64 aux;
};

TFR_HOSTDEV inline RowRef value_ref(const Batch& bt, int c, u32 b) {
  const Col& col = bt.cols[c];
  i64 r;
  const Src& s = src_of(bt, c, b, r);
  i64 v0;
  if (col.mode == CM_RAGGED) {
    v0 = s.row_off[r];
  } else if (col.mode == CM_RAGGED3D) {
    v0 = s.elem_off[s.sub_off[s.list_off[r]]];
  } else {
    const bool by = col.flags & CF_BYTES;
    v0 = (by ? s.elem_off : s.sub_off)[(by ? s.row_off : s.list_off)[r]];
  }
  return RowRef{(u64)s.values + (u64)((v0 - col.raw[b]) * col.esize),
                col.raw[b + 1]};
}

TFR_HOSTDEV inline RowRef item_ref(const Batch& bt, int c, u32 b) {
  const Col& col = bt.cols[c];
  i64 r;
  const Src& s = src_of(bt, c, b, r);
  const bool by = col.flags & CF_BYTES;
  const i64* inner_off = by ? s.elem_off : s.sub_off;
  const i64 o0 = col.mode == CM_RAGGED3D ? s.sub_off[s.list_off[r]]
                                         : (by ? s.row_off : s.list_off)[r];
  return RowRef{(u64)inner_off + (u64)((o0 - col.raw[bt.B + 1 + b]) * 8),
                col.raw[b] - inner_off[o0]};
}

TFR_HOSTDEV inline RowRef step_ref(const Batch& bt, int c, u32 b) {
  const Col& col = bt.cols[c];
  i64 r;
  const Src& s = src_of(bt, c, b, r);
  const i64 l0 = s.list_off[r];
  return RowRef{
      (u64)s.sub_off + (u64)((l0 - col.raw[2 * (bt.B + 1) + b]) * 8),
      col.raw[bt.B + 1 + b] - s.sub_off[l0]};
}

// Value unit u of ragged column c; b is the batch row that the unit's first
// position lies in and rr its value_ref (both unused when that position is
// past the batch's total). WORDS: a word of a byte column that lies inside
// one row is read as two aligned 8-byte loads and funnel-shifted; an aligned
// word that holds a wanted byte lies in that byte's page, so the over-read
// cannot fault. Other words, and the host, go byte by byte.
template <class Ops, bool WORDS>
TFR_HOSTDEV inline void ragged_value_unit(const Batch& bt, int c, u32 u, u32 b,
                                          RowRef rr) {
  const Col& col = bt.cols[c];
  const i64 total = col.raw[bt.B];
  if (col.esize != 1) {
    const i64 p = u;
    u64 v = 0;
    if (p < total) {
      if (col.esize == 8) {
        __builtin_memcpy(&v, (const u8*)(rr.addr + (u64)p * 8), 8);
      } else {
        u32 w;
        __builtin_memcpy(&w, (const u8*)(rr.addr + (u64)p * 4), 4);
        v = w;
      }
    }
    if (col.esize == 8 && !narrows(col)) {
      reinterpret_cast<u64*>(col.out)[u] = v;
    } else {
      if (narrows(col) && (i64)v != (i64)(i32)v)
        raise<Ops>(bt, c, b, CC_RANGE);
      reinterpret_cast<u32*>(col.out)[u] = (u32)v;
    }
    return;
  }
  const i64 p = (i64)u * 8;
  const u32 cnt = (u32)min64v(8, col.cap - p);
  u64 word = 0;
  if (WORDS && p + 8 <= rr.aux) {
    const u64 a = rr.addr + (u64)p;
    const u32 mis = (u32)(a & 7);
    const u64* q = reinterpret_cast<const u64*>(a - mis);
    word = q[0];
    if (mis) word = (word >> (8 * mis)) | (q[1] << (64 - 8 * mis));
  } else {
    for (u32 k = 0; k < cnt && p + k < total; ++k) {
      if (p + k >= rr.aux) {
        while (p + k >= col.raw[b + 1]) ++b;
        rr = value_ref(bt, c, b);
      }
      const u8 byte = *(const u8*)(rr.addr + (u64)(p + k));
      word |= (u64)byte << (8 * k);
    }
  }
  if (cnt == 8) {
    reinterpret_cast<u64*>(col.out)[u] = word;
  } else {
    for (u32 k = 0; k < cnt; ++k) col.out[p + k] = (u8)(word >> (8 * k));
  }
}

// item_offsets entry q (0..icap) of RAGGED2D column c; rr is the item_ref of
// the batch row that owns item q (unused past the last item).
TFR_HOSTDEV inline void ragged_item_unit(const Batch& bt, int c, u32 q,
                                         RowRef rr) {
  const Col& col = bt.cols[c];
  i64 v = col.raw[bt.B];
  if ((i64)q < col.raw[2 * bt.B + 1]) {
    __builtin_memcpy(&v, (const u8*)(rr.addr + (u64)q * 8), 8);
    v += rr.aux;
  }
  col.outer[q] = (i32)min64v(v, col.cap);
}

// step_offsets entry q (0..scap) of RAGGED3D column c; rr is the step_ref of
// the batch row that owns step q (unused past the last step).
TFR_HOSTDEV inline void ragged_step_unit(const Batch& bt, int c, u32 q,
                                         RowRef rr) {
  const Col& col = bt.cols[c];
  i64 v = col.raw[2 * bt.B + 1];
  if ((i64)q < col.raw[3 * bt.B + 2]) {
    __builtin_memcpy(&v, (const u8*)(rr.addr + (u64)q * 8), 8);
    v += rr.aux;
  }
  col.steps[q] = (i32)min64v(v, col.icap);
}

// Host atomics: the host path is one thread.
struct HostOps {
  static void min64(u64* p, u64 v) {
    if (v < *p) *p = v;
  }
  static void inc64(u64* p) { *p += 1; }
};

// A ragged column on the host: a serial prefix sum, then the units in order
// with a cursor for the row of each.
inline void host_ragged(const Batch& bt, int c) {
  const Col& col = bt.cols[c];
  const u32 B = (u32)bt.B;
  ragged_row0<HostOps>(bt, c);
  i64 v = 0, i = 0, st = 0;
  for (u32 b = 0; b < B; ++b) {
    const Counts n = row_counts(bt, c, b);
    v += n.values;
    i += n.items;
    st += n.steps;
    ragged_row<HostOps>(bt, c, b, n, v, i, st);
  }
  const i64 g = col.esize == 1 ? 8 : 1;
  u32 b = 0;
  for (i64 u = 0, nu = value_units(col); u < nu; ++u) {
    RowRef rr{0, 0};
    if (u * g < v) {
      while (u * g >= col.raw[b + 1]) ++b;
      rr = value_ref(bt, c, b);
    }
    ragged_value_unit<HostOps, false>(bt, c, (u32)u, b, rr);
  }
  if (col.mode == CM_RAGGED) return;
  const i64* ioff = col.raw + B + 1;
  b = 0;
  for (i64 q = 0; q <= col.icap; ++q) {
    RowRef rr{0, 0};
    if (q < i) {
      while (q >= ioff[b + 1]) ++b;
      rr = item_ref(bt, c, b);
    }
    ragged_item_unit(bt, c, (u32)q, rr);
  }
  if (col.mode != CM_RAGGED3D) return;
  const i64* soff = col.raw + 2 * (B + 1);
  b = 0;
  for (i64 q = 0; q <= col.scap; ++q) {
    RowRef rr{0, 0};
    if (q < st) {
      while (q >= soff[b + 1]) ++b;
      rr = step_ref(bt, c, b);
    }
    ragged_step_unit(bt, c, (u32)q, rr);
  }
}

inline void host_run(const Batch& bt) {
  for (int c = 0; c < (int)bt.ncols; ++c) {
    if (is_ragged(bt.cols[c])) {
      host_ragged(bt, c);
      continue;
    }
    const bool three = bt.cols[c].mode == CM_PADDED3D;
    for (i64 u = 0; u < bt.cols[c].units; ++u) {
      if (three)
        unit3d<HostOps>(bt, c, (u32)u);
      else
        do_unit<HostOps>(bt, c, (u32)u);
    }
  }
}

}  // namespace collate
}  // namespace tfrec
