// Stand-alone host check of the raw-Snappy chunk decoder core (unsnap_one)
// over the cases of tests/snappy_cases.py, regenerated here with a small
// PRNG: chunks from a plain greedy encoder, the hand-assembled encodings,
// one malformed chunk per cause code, and every truncation of every valid
// chunk. Each run gets exact-size heap blocks, so one byte read or written
// past either end trips the sanitizer; each chunk is also walked once per
// lane (lane = 0..63, the device's share of the copies) for the bounds of
// the lane-strided paths. Meant to be built with sanitizers and run as its
// own executable on the CPU, before the kernel first runs on a GPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -fno-sanitize-recover=all csrc/tests/snappy_selftest.cpp \
//       -o snappy_selftest && ./snappy_selftest
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../snappy_core.h"

using namespace tfrec;
using Bytes = std::vector<uint8_t>;

static uint64_t g_state = 0x13198A2E03707344ull;
static uint32_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static Bytes random_bytes(size_t n, uint32_t lo = 0, uint32_t hi = 256) {
  Bytes b(n);
  for (auto& x : b) x = (uint8_t)(lo + rnd() % (hi - lo));
  return b;
}

static Bytes varint(uint64_t n) {
  Bytes b;
  while (n >= 0x80) {
    b.push_back((uint8_t)((n & 0x7F) | 0x80));
    n >>= 7;
  }
  b.push_back((uint8_t)n);
  return b;
}

static void append(Bytes& a, const Bytes& b) {
  a.insert(a.end(), b.begin(), b.end());
}

// Assembles a chunk element by element and plays it forward.
struct Chunk {
  Bytes body, out;
  std::vector<size_t> starts;  // each element's offset in body

  Chunk& lit(const Bytes& d, int form = -1) {
    starts.push_back(body.size());
    uint64_t n = d.size() - 1;
    if (form < 0) {
      form = 0;
      if (n >= 60)
        for (form = 1; form < 4 && (n >> (8 * form)); ++form) {
        }
    }
    if (form == 0) {
      body.push_back((uint8_t)(n << 2));
    } else {
      body.push_back((uint8_t)((59 + form) << 2));
      for (int i = 0; i < form; ++i) body.push_back((uint8_t)(n >> (8 * i)));
    }
    append(body, d);
    append(out, d);
    return *this;
  }
  // raw copy element, not played (for the malformed cases)
  static Bytes copy_bytes(int tag, int len, uint32_t off) {
    Bytes e;
    if (tag == 1) {
      e.push_back((uint8_t)(1 | ((len - 4) << 2) | ((off >> 8) << 5)));
      e.push_back((uint8_t)off);
    } else {
      e.push_back((uint8_t)(tag | ((len - 1) << 2)));
      for (int i = 0; i < (tag == 2 ? 2 : 4); ++i)
        e.push_back((uint8_t)(off >> (8 * i)));
    }
    return e;
  }
  Chunk& copy(int tag, int len, uint32_t off) {
    starts.push_back(body.size());
    append(body, copy_bytes(tag, len, off));
    for (int i = 0; i < len; ++i) out.push_back(out[out.size() - off]);
    return *this;
  }
  Bytes comp() const {
    Bytes c = varint(out.size());
    append(c, body);
    return c;
  }
};

// Plain greedy encoder (4-byte hash, tag-10 copies in pieces of <= 64,
// literals in between): stands in for the library's chunks.
static Bytes encode(const Bytes& d) {
  Chunk c;
  std::vector<int64_t> table(1 << 12, -1);
  size_t n = d.size(), i = 0, lit0 = 0;
  auto flush = [&](size_t hi) {
    if (hi > lit0) c.lit(Bytes(d.begin() + lit0, d.begin() + hi));
  };
  while (i + 4 <= n) {
    uint32_t v;
    std::memcpy(&v, &d[i], 4);
    uint32_t h = (v * 0x1E35A7BDu) >> 20;
    int64_t cand = table[h];
    table[h] = (int64_t)i;
    if (cand >= 0 && i - (size_t)cand <= 65535 &&
        std::memcmp(&d[cand], &d[i], 4) == 0) {
      size_t len = 4;
      while (i + len < n && d[cand + len] == d[i + len]) ++len;
      flush(i);
      size_t off = i - (size_t)cand;
      for (size_t left = len; left;) {
        int take = left > 64 ? 64 : (int)left;
        c.copy(2, take, (uint32_t)off);
        left -= take;
      }
      i += len;
      lit0 = i;
    } else {
      ++i;
    }
  }
  flush(n);
  if (c.out != d) {
    std::printf("FAIL encoder self-check\n");
    std::exit(2);
  }
  return c.comp();
}

// One run of the core over exact-size blocks; *got receives the output.
static int run(const Bytes& comp, int64_t expect, int lane, Bytes* got) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[comp.size() ? comp.size() : 1]);
  if (!comp.empty()) std::memcpy(in.get(), comp.data(), comp.size());
  // a zero-length range still needs a pointer the core must not touch
  std::unique_ptr<uint8_t[]> out(new uint8_t[expect ? expect : 1]);
  std::memset(out.get(), 0xA5, expect ? (size_t)expect : 1);
  int rc = snappy::unsnap_one(comp.empty() ? in.get() + 1 : in.get(),
                              (int64_t)comp.size(),
                              expect ? out.get() : out.get() + 1, expect, lane);
  if (got) got->assign(out.get(), out.get() + expect);
  return rc;
}

static int g_fail = 0;

static void check_valid(const std::string& name, const Bytes& comp,
                        const Bytes& want) {
  Bytes got;
  int rc = run(comp, (int64_t)want.size(), -1, &got);
  if (rc || got != want) {
    std::printf("FAIL %s: rc %d, bytes %s\n", name.c_str(), rc,
                got == want ? "equal" : "differ");
    ++g_fail;
    return;
  }
  for (int lane = 0; lane < 64; ++lane) {
    rc = run(comp, (int64_t)want.size(), lane, nullptr);
    if (rc) {
      std::printf("FAIL %s: lane %d rc %d\n", name.c_str(), lane, rc);
      ++g_fail;
      return;
    }
  }
  // every truncation ends in a cause code, within bounds
  size_t step = comp.size() > 4096 ? comp.size() / 512 : 1;
  for (size_t cut = 0; cut < comp.size(); cut += step) {
    Bytes part(comp.begin(), comp.begin() + cut);
    for (int lane : {-1, 0, 63}) {
      if (!run(part, (int64_t)want.size(), lane, nullptr)) {
        std::printf("FAIL %s: cut at %zu accepted\n", name.c_str(), cut);
        ++g_fail;
        return;
      }
    }
  }
  std::printf("ok   %s (%zu -> %zu)\n", name.c_str(), comp.size(),
              want.size());
}

static void check_bad(const std::string& name, const Bytes& comp,
                      int64_t expect, int cause) {
  for (int lane : {-1, 0, 17, 63}) {
    int rc = run(comp, expect, lane, nullptr);
    if (rc != cause) {
      std::printf("FAIL %s: lane %d rc %d, want %d\n", name.c_str(), lane, rc,
                  cause);
      ++g_fail;
      return;
    }
  }
  std::printf("ok   %s (cause %d)\n", name.c_str(), cause);
}

int main() {
  // encoder-made chunks (the library's role in tests/snappy_cases.py)
  {
    Bytes abcd;
    for (int i = 0; i < 20000; ++i) abcd.push_back((uint8_t)("abcd"[i & 3]));
    Bytes rows;  // record-like: a fixed key, a counter, noise
    for (int r = 0; r < 200; ++r) {
      const char* key = "\x0a\x04ints\x12\x10";
      rows.insert(rows.end(), key, key + 8);
      rows.push_back((uint8_t)r);
      append(rows, random_bytes(40));
    }
    struct {
      const char* name;
      Bytes data;
    } lib[] = {{"empty", {}},
               {"one_byte", {0x2a}},
               {"random_100", random_bytes(100)},
               {"abcd_x5000", abcd},
               {"zeros_70000", Bytes(70000, 0)},
               {"letters_64k", random_bytes(64 << 10, 97, 123)},
               {"record_like", rows}};
    for (auto& c : lib) check_valid(c.name, encode(c.data), c.data);
  }
  // hand-assembled encodings
  for (size_t n : {60, 61, 256, 257}) {
    Chunk c;
    c.lit(random_bytes(n));
    check_valid("literal_" + std::to_string(n), c.comp(), c.out);
  }
  for (int form : {2, 3, 4}) {
    Chunk c;
    c.lit({'h', 'e', 'l', 'l', 'o'}, form);
    check_valid("literal_5_form_" + std::to_string(form), c.comp(), c.out);
  }
  {
    Chunk c;
    c.lit(random_bytes(2047));
    for (int len : {4, 11})
      for (uint32_t off : {1u, 2047u}) c.copy(1, len, off);
    check_valid("copy01_len_4_11_off_1_2047", c.comp(), c.out);
  }
  {
    Chunk c;
    c.lit(random_bytes(65535));
    for (int len : {1, 64})
      for (uint32_t off : {1u, 3u, 63u, 64u, 65535u}) c.copy(2, len, off);
    check_valid("copy10_len_1_64_offsets", c.comp(), c.out);
  }
  {
    Chunk c;
    c.lit(random_bytes(40)).copy(3, 30, 5).copy(3, 64, 5).copy(3, 1, 5);
    check_valid("copy11_off_5", c.comp(), c.out);
  }
  {
    Chunk c;
    c.lit(random_bytes(70000)).copy(3, 64, 70000).copy(3, 7, 70000);
    c.lit(random_bytes((128 << 10) - c.out.size() - 64)).copy(3, 64, 70000);
    check_valid("copy11_off_70000_in_128k", c.comp(), c.out);
  }
  {
    Chunk c;
    c.lit(random_bytes(10)).copy(2, 10, 10);
    check_valid("copy_source_at_byte_0", c.comp(), c.out);
  }
  {
    Chunk c;
    c.lit({'x', 'y', 'z'}).copy(1, 11, 2);
    check_valid("copy_ends_at_expect_len", c.comp(), c.out);
  }
  for (int shift = 0; shift < 4; ++shift) {
    Chunk c;
    c.lit(random_bytes(shift + 1));
    for (int k = 0; k < 200; ++k) c.lit({(uint8_t)k, (uint8_t)shift, 0x5A});
    check_valid("elements_4_bytes_x200_shift_" + std::to_string(shift),
                c.comp(), c.out);
  }
  // one malformed chunk per cause, each one edit away from `base`
  {
    Chunk base;
    const char* s = "snappy-chunk-";
    base.lit(Bytes(s, s + 13)).copy(2, 20, 7).lit({'t', 'a', 'i', 'l'});
    Chunk lit_last = base;
    base.copy(2, 9, 3);
    int64_t n = (int64_t)base.out.size();
    Bytes pre = varint(n), body = base.body;
    auto elems = [&](size_t lo, size_t hi) {  // elements [lo, hi) of base
      size_t a = base.starts[lo];
      size_t b = hi < base.starts.size() ? base.starts[hi] : body.size();
      return Bytes(body.begin() + a, body.begin() + b);
    };
    auto cat = [](std::initializer_list<Bytes> parts) {
      Bytes r;
      for (auto& p : parts) append(r, p);
      return r;
    };
    check_bad("preamble_6_bytes",
              cat({Bytes(5, 0x80), Bytes(1, 0), body}), n,
              snappy::SN_PREAMBLE_LONG);
    check_bad("preamble_off_by_one", cat({varint(n + 1), body}), n,
              snappy::SN_PREAMBLE_MISMATCH);
    check_bad("offset_zero",
              cat({pre, elems(0, 1), Chunk::copy_bytes(2, 20, 0),
                   elems(2, 4)}),
              n, snappy::SN_OFFSET_ZERO);
    check_bad("offset_past_start",
              cat({pre, elems(0, 1), Chunk::copy_bytes(2, 20, 14),
                   elems(2, 4)}),
              n, snappy::SN_OFFSET_FAR);
    Bytes cut = cat({pre, body});
    cut.pop_back();
    check_bad("operand_cut", cut, n, snappy::SN_OPERAND_PAST_INPUT);
    Bytes lcut = lit_last.comp();
    lcut.pop_back();
    check_bad("literal_cut", lcut, (int64_t)lit_last.out.size(),
              snappy::SN_LITERAL_PAST_INPUT);
    check_bad("output_overrun",
              cat({pre, elems(0, 3), Chunk::copy_bytes(2, 10, 3)}), n,
              snappy::SN_OUTPUT_OVERRUN);
    check_bad("input_short", cat({pre, elems(0, 3)}), n,
              snappy::SN_INPUT_SHORT);
    check_bad("input_left_over", cat({pre, body, Bytes{0x00, '!'}}), n,
              snappy::SN_INPUT_LEFT);
    // lengths and offsets at the top of their fields must not wrap
    check_bad("literal_4g", cat({pre, Bytes{0xFC, 0xFF, 0xFF, 0xFF, 0xFF}}),
              n, snappy::SN_LITERAL_PAST_INPUT);
    check_bad("offset_4g",
              cat({pre, elems(0, 1), Chunk::copy_bytes(3, 20, 0xFFFFFFFFu)}),
              n, snappy::SN_OFFSET_FAR);
  }
  // random byte soup under every expect_len class: only bounds matter
  for (int k = 0; k < 2000; ++k) {
    Bytes soup = random_bytes(1 + rnd() % 96);
    int64_t expect = rnd() % 300;
    Bytes pre = varint((uint64_t)expect);
    if (k & 1) std::memcpy(soup.data(), pre.data(),
                           pre.size() < soup.size() ? pre.size() : soup.size());
    for (int lane : {-1, 0, 63}) run(soup, expect, lane, nullptr);
  }
  std::printf("ok   byte soup x2000\n");
  if (g_fail) {
    std::printf("%d case(s) FAILED\n", g_fail);
    return 1;
  }
  std::printf("all snappy core cases passed\n");
  return 0;
}
