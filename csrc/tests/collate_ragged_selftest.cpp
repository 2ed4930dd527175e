// Stand-alone host check of the packed modes of the batch collation core
// (collate_core.h host_ragged: RAGGED and RAGGED2D, the int32 narrowing)
// over generated columns: absent rows, empty rows, empty items, a row longer
// than a tile, capacities at, below and above the batch's total and not a
// multiple of 8. Every input array, every output and the raw-offset scratch
// get an exact-size heap block, so one byte read or written past an end
// trips the sanitizer; outputs are also compared with a direct evaluation
// written here. Meant to be built with sanitizers and run as its own
// executable on the CPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -fno-sanitize-recover=all csrc/tests/collate_ragged_selftest.cpp \
//       -o collate_ragged_selftest && ./collate_ragged_selftest
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../collate_core.h"

using namespace tfrec::collate;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static int g_fail = 0;
#define CHECK(cond, ...)                              \
  do {                                                \
    if (!(cond)) {                                    \
      std::printf("FAIL %s:%d ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                       \
      std::printf("\n");                              \
      ++g_fail;                                       \
    }                                                 \
  } while (0)

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
  std::unique_ptr<T[]> p(new T[v.empty() ? 1 : v.size()]);
  if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

// One generated column of one slot: row -> items -> elements (a one-level
// column has one item per present row), and its wire form.
struct GenCol {
  std::vector<u8> presence;
  std::vector<std::vector<std::vector<u64>>> rows;
  std::unique_ptr<u8[]> h_presence, h_values;
  std::unique_ptr<i64[]> h_row_off, h_elem_off, h_list_off, h_sub_off;
  Src src{};
};

static void gen_col(GenCol& g, int R, int esize, bool two, bool bytes,
                    int long_row) {
  g.presence.assign(R, 1);
  g.rows.assign(R, {});
  for (int r = 0; r < R; ++r) {
    if (rnd() % 6 == 0) {
      g.presence[r] = 0;
      continue;
    }
    const int items = two ? rnd() % 4 : 1;
    for (int t = 0; t < items; ++t) {
      std::vector<u64> v(r == long_row ? 2500 : rnd() % 6);
      for (auto& x : v) x = esize == 8 ? (u64)(i64)(int32_t)rnd() : rnd();
      g.rows[r].push_back(v);
    }
  }
  std::vector<i64> row_off{0}, elem_off, list_off{0}, sub_off{0};
  std::vector<u8> values;
  if (bytes) {
    values.assign(1 + rnd() % 7, 0xEE);  // strings start at any alignment
    elem_off.push_back((i64)values.size());
  }
  i64 nvals = 0, nitems = 0;
  for (int r = 0; r < R; ++r) {
    for (auto& item : g.rows[r]) {
      for (u64 x : item)
        for (int k = 0; k < esize; ++k) values.push_back((u8)(x >> (8 * k)));
      nvals += (i64)item.size();
      ++nitems;
      if (bytes) elem_off.push_back((i64)values.size());
      if (two && !bytes) sub_off.push_back(nvals);
    }
    row_off.push_back(bytes ? nitems : nvals);
    list_off.push_back(nitems);
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
  } else if (two) {
    g.h_list_off = exact(list_off);
    g.h_sub_off = exact(sub_off);
    g.src.list_off = g.h_list_off.get();
    g.src.sub_off = g.h_sub_off.get();
  }
}

// One column, two slots, B rows; slack: capacity minus the batch's total.
static long run(int esize, bool two, bool narrow, i64 max_len, int B,
                int slack, bool with_long_row) {
  const bool bytes = esize == 1;
  const int slot_rows[2] = {7, 1 + B / 2};
  GenCol gen[2];
  Src src[2];
  for (int s = 0; s < 2; ++s) {
    gen_col(gen[s], slot_rows[s], esize, two, bytes,
            with_long_row && s == 1 ? 0 : -1);
    src[s] = gen[s].src;
  }
  std::vector<i32> sel_slot(B);
  std::vector<i64> sel_row(B);
  // direct evaluation: the batch's items and values, in order
  std::vector<u64> flat;
  std::vector<i64> voff{0}, ioff{0}, item_start;
  i64 want_cut = 0;
  for (int b = 0; b < B; ++b) {
    sel_slot[b] = (i32)(rnd() % 2);
    sel_row[b] = (i64)(rnd() % slot_rows[sel_slot[b]]);
    i64 items = 0;
    for (auto& item : gen[sel_slot[b]].rows[sel_row[b]]) {
      size_t n = item.size();
      if (!two && max_len && (i64)n > max_len) {
        n = (size_t)max_len;
        ++want_cut;
      }
      item_start.push_back((i64)flat.size());
      flat.insert(flat.end(), item.begin(), item.begin() + n);
      ++items;
    }
    voff.push_back((i64)flat.size());
    ioff.push_back(ioff.back() + (two ? items : 0));
  }
  const i64 total = (i64)flat.size(), itotal = ioff.back();
  const i64 cap = total + slack > 0 ? total + slack : 1;
  const i64 icap = itotal + slack > 0 ? itotal + slack : 1;
  const int osize = narrow ? 4 : esize;

  auto h_src = exact(std::vector<Src>(src, src + 2));
  auto h_slot = exact(sel_slot);
  auto h_row = exact(sel_row);
  std::unique_ptr<u8[]> out(new u8[cap * osize]);
  std::unique_ptr<i32[]> offs(new i32[B + 1]), ioffs(new i32[icap + 1]);
  std::unique_ptr<i64[]> raw(new i64[(two ? 2 : 1) * (B + 1)]);
  std::memset(out.get(), 0x5C, cap * osize);
  Col col{};
  col.mode = two ? CM_RAGGED2D : CM_RAGGED;
  col.esize = esize;
  col.osize = osize;
  col.T = 1;
  col.L = max_len ? max_len : (i64)1 << 62;
  col.flags = (max_len ? CF_TRUNCATE : 0) | (bytes ? CF_BYTES : 0);
  col.out = out.get();
  col.len = offs.get();
  col.outer = two ? ioffs.get() : nullptr;
  col.raw = raw.get();
  col.cap = cap;
  col.icap = two ? icap : 0;
  auto h_col = exact(std::vector<Col>{col});
  std::unique_ptr<u64[]> status(new u64[2]);
  status[0] = kStatusClean;
  status[1] = 0;
  Batch bt{h_src.get(), h_col.get(), h_slot.get(), h_row.get(), 1, B,
           status.get()};
  host_run(bt);

  u64 want_status = kStatusClean;
  for (int b = B - 1; b >= 0; --b)
    if (voff[b + 1] > cap || (two && ioff[b + 1] > icap))
      want_status = ((u64)b << 16) | CC_CAPACITY;
  CHECK(status[0] == want_status, "status %llx != %llx",
        (unsigned long long)status[0], (unsigned long long)want_status);
  CHECK((i64)status[1] == want_cut, "cut rows");
  for (int b = 0; b <= B; ++b) {
    const i64 w = two ? (ioff[b] < icap ? ioff[b] : icap)
                      : (voff[b] < cap ? voff[b] : cap);
    CHECK(offs[b] == w, "offsets[%d]", b);
  }
  const u64 mask = osize == 8 ? ~0ull : osize == 4 ? 0xFFFFFFFFull : 0xFFull;
  for (i64 p = 0; p < cap; ++p) {
    u64 got = 0;
    std::memcpy(&got, out.get() + p * osize, osize);
    CHECK(got == (p < total ? flat[p] & mask : 0), "value %lld", (long long)p);
  }
  for (i64 q = 0; two && q <= icap; ++q) {
    const i64 w = q < itotal ? item_start[q] : total;
    CHECK(ioffs[q] == (w < cap ? w : cap), "item_offsets[%lld]", (long long)q);
  }
  return cap + B + 1 + (two ? icap + 1 : 0);
}

int main() {
  long checks = 0;
  for (int B : {1, 65, 257})
    for (int slack : {0, 3, -1, -40})
      for (bool with_long_row : {false, true}) {
        checks += run(8, false, false, 0, B, slack, with_long_row);
        checks += run(8, false, true, 3, B, slack, with_long_row);
        checks += run(4, false, false, 4, B, slack, with_long_row);
        checks += run(8, true, true, 0, B, slack, with_long_row);
        checks += run(4, true, false, 0, B, slack, with_long_row);
        checks += run(1, true, false, 0, B, slack, with_long_row);
      }
  if (g_fail) {
    std::printf("collate_ragged_selftest: %d FAILED of %ld checks\n", g_fail,
                checks);
    return 1;
  }
  std::printf("collate_ragged_selftest: ok (%ld checks)\n", checks);
  return 0;
}
