// Stand-alone host check of the batch collation core (collate_core.h
// host_run / do_unit) over generated columns: every mode (FIXED with and
// without default, PADDED, PADDED2D over list_off/sub_off and over
// row_off/elem_off) at every element size (8, 4, 1), with absent rows, empty
// rows, rows of exactly L and over-long rows, batches that interleave three
// slots with repeats, and B, T, L around the unit and tile sizes. Every
// input array and every output gets an exact-size heap block, so one byte
// read or written past an end trips the sanitizer; outputs are also compared
// with a direct per-element evaluation written here. Meant to be built with
// sanitizers and run as its own executable on the CPU, before the kernel
// first runs on a GPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -fno-sanitize-recover=all csrc/tests/collate_selftest.cpp \
//       -o collate_selftest && ./collate_selftest
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../collate_core.h"

using namespace tfrec::collate;

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint32_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static int g_fail = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      std::printf("FAIL %s:%d ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
      ++g_fail;                               \
    }                                         \
  } while (0)

// An exact-size heap copy of a vector: ASan's redzones sit right at both
// ends. Empty arrays still get a (1-byte) block, never a null pointer the
// core could not be caught dereferencing.
template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
  std::unique_ptr<T[]> p(new T[v.empty() ? 1 : v.size()]);
  if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

// One generated column of one slot, as nested counts, plus its wire form.
struct GenCol {
  std::vector<u8> presence;
  std::vector<std::vector<std::vector<u64>>> rows;  // row -> items -> elems
  std::unique_ptr<u8[]> h_presence, h_values;
  std::unique_ptr<i64[]> h_row_off, h_elem_off, h_list_off, h_sub_off;
  Src src{};
};

// two_level: rows hold several items; otherwise exactly one item per row
// (its elements are the row's values).
static void gen_col(GenCol& g, int R, int esize, bool two_level, bool bytes,
                    int T, int L, bool over, bool fixed, bool allow_missing) {
  g.presence.assign(R, 1);
  g.rows.assign(R, {});
  auto inner = [&](bool exact_only) {
    int n;
    uint32_t pick = rnd() % 5;
    if (exact_only)
      n = L;
    else if (pick == 0)
      n = 0;
    else if (pick == 1)
      n = L;
    else if (pick == 2 && over)
      n = L + 1 + rnd() % 3;
    else
      n = rnd() % (L + 1);
    std::vector<u64> v(n);
    for (auto& x : v) x = ((u64)rnd() << 32) | rnd();
    return v;
  };
  for (int r = 0; r < R; ++r) {
    uint32_t pick = (r + rnd() % 2) % 5;
    if (fixed) {
      if (allow_missing && pick == 0) {
        g.presence[r] = 0;
      } else if (allow_missing && pick == 1) {
        g.rows[r].push_back({});
      } else {
        g.rows[r].push_back(inner(true));
        // a wrong count, for LENGTH
        if (allow_missing && pick == 2) g.rows[r].back().push_back(1);
      }
      continue;
    }
    if (pick == 0) {
      g.presence[r] = 0;
      continue;
    }
    if (!two_level) {
      g.rows[r].push_back(inner(false));
      continue;
    }
    int oc = pick == 1 ? 0 : pick == 2 ? T
             : (pick == 3 && over) ? T + 1 + rnd() % 2 : rnd() % (T + 1);
    for (int t = 0; t < oc; ++t) g.rows[r].push_back(inner(false));
  }
  // wire form
  std::vector<i64> row_off{0}, elem_off, list_off, sub_off;
  std::vector<u8> values;
  if (bytes) {
    values.push_back(0xEE);  // strings start at odd offsets
    elem_off.push_back(1);
  }
  if (two_level && !bytes) {
    list_off.push_back(0);
    sub_off.push_back(0);
  }
  i64 nvals = 0, nitems = 0;
  for (int r = 0; r < R; ++r) {
    for (auto& item : g.rows[r]) {
      for (u64 x : item)
        for (int k = 0; k < esize; ++k) values.push_back((u8)(x >> (8 * k)));
      nvals += (i64)item.size();
      ++nitems;
      if (bytes) elem_off.push_back((i64)values.size());
      if (two_level && !bytes) sub_off.push_back(nvals);
    }
    row_off.push_back(bytes ? nitems : nvals);
    if (two_level && !bytes) list_off.push_back(nitems);
  }
  g.h_presence = exact(g.presence);
  g.h_values = exact(values);
  g.h_row_off = exact(row_off);
  g.src.presence = g.h_presence.get();
  g.src.values = g.h_values.get();
  g.src.row_off = g.h_row_off.get();
  if (bytes) {
    g.h_elem_off = exact(elem_off);
    g.src.elem_off = g.h_elem_off.get();
  }
  if (two_level && !bytes) {
    g.h_list_off = exact(list_off);
    g.h_sub_off = exact(sub_off);
    g.src.list_off = g.h_list_off.get();
    g.src.sub_off = g.h_sub_off.get();
  }
}

struct ColPlan {
  int mode, esize, T, L;
  bool bytes, truncate, has_default;
};

static u64 mask_of(int esize) {
  return esize == 8 ? ~0ull : esize == 4 ? 0xFFFFFFFFull : 0xFFull;
}

// One batch over `plans`, three slots, B rows; returns checks run.
static long run_batch(const std::vector<ColPlan>& plans, int B) {
  const int nslots = 3;
  const int slot_rows[nslots] = {5, 1 + B / 2, 17};
  const int nc = (int)plans.size();
  std::vector<GenCol> gen((size_t)nslots * nc);
  std::vector<Src> src((size_t)nslots * nc);
  for (int s = 0; s < nslots; ++s)
    for (int c = 0; c < nc; ++c) {
      const ColPlan& p = plans[c];
      GenCol& g = gen[(size_t)s * nc + c];
      // refusing columns get over-long rows too: their LENGTH errors
      gen_col(g, slot_rows[s], p.esize, p.mode == CM_PADDED2D, p.bytes, p.T,
              p.L, /*over=*/true, p.mode == CM_FIXED, p.has_default);
      src[(size_t)s * nc + c] = g.src;
    }
  std::vector<i32> sel_slot(B);
  std::vector<i64> sel_row(B);
  for (int b = 0; b < B; ++b) {
    sel_slot[b] = (i32)(rnd() % nslots);
    sel_row[b] = (i64)(rnd() % slot_rows[sel_slot[b]]);
  }
  auto h_src = exact(src);
  auto h_slot = exact(sel_slot);
  auto h_row = exact(sel_row);

  std::vector<Col> cols(nc);
  std::vector<std::unique_ptr<u8[]>> outs(nc);
  std::vector<std::unique_ptr<i32[]>> lens(nc), outers(nc);
  i64 tile0 = 0;
  for (int c = 0; c < nc; ++c) {
    const ColPlan& p = plans[c];
    const i64 elems = (i64)B * p.T * p.L;
    Col& col = cols[c];
    col = Col{};
    col.mode = p.mode;
    col.esize = p.esize;
    col.T = p.T;
    col.L = p.L;
    col.fill = 0xA5A5A5A5A5A5A5A5ull & mask_of(p.esize);
    col.flags = (p.has_default ? CF_DEFAULT : 0) |
                (p.truncate ? CF_TRUNCATE : 0) | (p.bytes ? CF_BYTES : 0);
    outs[c].reset(new u8[elems * p.esize]);
    std::memset(outs[c].get(), 0x5C, elems * p.esize);
    col.out = outs[c].get();
    if (p.mode != CM_FIXED) {
      lens[c].reset(new i32[(size_t)B * p.T]);
      col.len = lens[c].get();
    }
    if (p.mode == CM_PADDED2D) {
      outers[c].reset(new i32[B]);
      col.outer = outers[c].get();
    }
    col.tile0 = tile0;
    col.units = p.esize == 1 ? (elems + 7) / 8 : elems;
    tile0 += (col.units + kTileUnits - 1) / kTileUnits;
  }
  auto h_cols = exact(cols);
  std::unique_ptr<u64[]> status(new u64[2]);
  status[0] = kStatusClean;
  status[1] = 0;
  Batch bt{h_src.get(), h_cols.get(), h_slot.get(), h_row.get(), nc, B,
           status.get()};
  host_run(bt);

  // direct evaluation from the nested counts
  long checks = 0;
  u64 want_status = kStatusClean, want_trunc = 0;
  for (int b = 0; b < B; ++b) {
    bool row_trunc = false;
    for (int c = 0; c < nc; ++c) {
      const ColPlan& p = plans[c];
      const GenCol& g = gen[(size_t)sel_slot[b] * nc + c];
      const i64 r = sel_row[b];
      const bool present = g.presence[r];
      const auto& items = g.rows[r];
      int cause = 0;
      bool trunc = false;
      const u64 fill = cols[c].fill;
      for (int t = 0; t < p.T; ++t) {
        const std::vector<u64>* item = nullptr;
        if (present && t < (int)items.size()) item = &items[t];
        int n = item ? (int)item->size() : 0;
        if (p.mode == CM_FIXED) {
          if (n == 0)
            cause = p.has_default ? 0 : CC_MISSING;
          else if (n != p.L)
            cause = CC_LENGTH;
          if (n != p.L) n = 0;
        } else if (n > p.L) {
          n = p.L;
          if (p.truncate) trunc = true; else cause = CC_LENGTH;
        }
        for (int j = 0; j < p.L; ++j) {
          u64 want = j < n ? (*item)[j] & mask_of(p.esize) : fill;
          u64 got = 0;
          std::memcpy(&got,
                      outs[c].get() + (((i64)b * p.T + t) * p.L + j) * p.esize,
                      p.esize);
          CHECK(got == want, "col %d b %d t %d j %d: %llx != %llx", c, b, t,
                j, (unsigned long long)got, (unsigned long long)want);
          ++checks;
        }
        if (p.mode != CM_FIXED)
          CHECK(lens[c][(size_t)b * p.T + t] == n, "len col %d b %d t %d", c,
                b, t);
      }
      if (p.mode == CM_PADDED2D) {
        int oc = present ? (int)items.size() : 0;
        if (oc > p.T) {
          oc = p.T;
          if (p.truncate) trunc = true; else cause = CC_LENGTH;
        }
        CHECK(outers[c][b] == oc, "outer col %d b %d", c, b);
      }
      row_trunc |= trunc;
      if (cause) {
        u64 w = ((u64)b << 16) | ((u64)c << 8) | (u64)cause;
        if (w < want_status) want_status = w;
      }
    }
    want_trunc += row_trunc;
  }
  CHECK(status[0] == want_status, "status %llx != %llx",
        (unsigned long long)status[0], (unsigned long long)want_status);
  CHECK(status[1] == want_trunc, "truncated %llu != %llu",
        (unsigned long long)status[1], (unsigned long long)want_trunc);
  return checks;
}

int main() {
  long checks = 0;
  const int Bs[] = {1, 63, 64, 65, 257};
  const int Ls[] = {1, 3, 7, 8, 12, 17, 64, 65};
  const int Ts[] = {1, 2, 5};
  for (int B : Bs)
    for (int L : Ls) {
      // every one-level mode at both numeric sizes, in one batch
      std::vector<ColPlan> one;
      for (int esize : {8, 4}) {
        one.push_back({CM_FIXED, esize, 1, L, false, false, false});
        one.push_back({CM_FIXED, esize, 1, L, false, false, true});
        one.push_back({CM_PADDED, esize, 1, L, false, true, false});
        one.push_back({CM_PADDED, esize, 1, L, false, false, false});
      }
      checks += run_batch(one, B);
      for (int T : Ts) {
        // both two-level walks, cutting and refusing, at every size
        std::vector<ColPlan> two;
        for (bool cut : {true, false}) {
          two.push_back({CM_PADDED2D, 8, T, L, false, cut, false});
          two.push_back({CM_PADDED2D, 4, T, L, false, cut, false});
          two.push_back({CM_PADDED2D, 1, T, L, true, cut, false});
        }
        checks += run_batch(two, B);
      }
    }
  // a column that spans several tiles next to one smaller than a block
  checks += run_batch({{CM_FIXED, 8, 1, 1, false, false, true},
                       {CM_PADDED2D, 1, 5, 65, true, true, false},
                       {CM_PADDED2D, 4, 5, 65, false, true, false}},
                      257);
  if (g_fail) {
    std::printf("collate_selftest: %d FAILED of %ld checks\n", g_fail, checks);
    return 1;
  }
  std::printf("collate_selftest: ok (%ld element checks)\n", checks);
  return 0;
}
