// Stand-alone host check of the raw-Snappy chunk compressor core (snap_one)
// over the cases of tests/snappy_enc_cases.py, regenerated here with a small
// PRNG, and a few thousand seeded random and low-entropy inputs of 0 to
// 70000 bytes. Input and output live in exact-size heap blocks, so one byte
// read or written past either end trips the sanitizer. Each input is
// compressed into snap_out_bound(n) bytes, where the elements before the
// fallback must fit, and again into n + 10 bytes, which must give the same
// chunk; the chunk, moved to a block of its own size, must decode through
// unsnap_one to the input. Meant to be built with sanitizers and run as its
// own executable on the CPU, before the kernel first runs on a GPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -fno-sanitize-recover=all csrc/tests/snappy_enc_selftest.cpp \
//       -o snappy_enc_selftest && ./snappy_enc_selftest
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../snappy_enc_core.h"

using namespace tfrec;
using snappy::i64;
using Bytes = std::vector<uint8_t>;

static uint64_t g_state = 0x243F6A8885A308D3ull;
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

static void append(Bytes& a, const Bytes& b, size_t n = (size_t)-1) {
  a.insert(a.end(), b.begin(), b.begin() + (n < b.size() ? n : b.size()));
}

static int g_runs = 0, g_fallbacks = 0;

struct Heap {  // exact-size block: the sanitizer guards both ends
  uint8_t* p;
  explicit Heap(i64 n) : p((uint8_t*)std::malloc((size_t)(n > 0 ? n : 1))) {
    if (!p) std::abort();
  }
  ~Heap() { std::free(p); }
};

static i64 compress(const uint8_t* in, i64 n, uint8_t* out, i64 cap,
                    i64* emitted) {
  // LDS starts out with whatever the last block left there
  std::unique_ptr<snappy::EncScratch> S(new snappy::EncScratch);
  std::memset(static_cast<void*>(S.get()), 0xA5, sizeof(snappy::EncScratch));
  i64 len = snappy::snap_one(in, n, out, cap, *S);
  *emitted = S->emitted;
  return len;
}

#define REQUIRE(cond)                                                      \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "FAIL %s (n=%lld): %s, line %d\n", name,        \
                   (long long)n, #cond, __LINE__);                         \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

static void check(const char* name, const Bytes& data) {
  const i64 n = (i64)data.size();
  Heap in(n);
  if (n) std::memcpy(in.p, data.data(), (size_t)n);
  const i64 bound = snappy::snap_out_bound(n);
  const i64 lit = snappy::one_literal_len(n);
  REQUIRE(lit <= n + 10 && lit <= bound);

  Heap a(bound);
  i64 emitted = -2;
  const i64 len = compress(in.p, n, a.p, bound, &emitted);
  REQUIRE(len >= 1 && len <= lit);
  if (n) {
    // the bound holds: the elements never had to be cut short
    REQUIRE(emitted >= 1 && emitted <= bound);
    if (emitted > lit) ++g_fallbacks;  // only the rewrite gets len <= lit
  }

  Heap b(n + 10);
  i64 emitted_b = -2;
  const i64 len_b = compress(in.p, n, b.p, n + 10, &emitted_b);
  REQUIRE(len_b == len && std::memcmp(a.p, b.p, (size_t)len) == 0);

  if (lit > 1) {  // one byte short of the single literal: refused, untouched
    Heap c(lit - 1);
    i64 e = -2;
    REQUIRE(compress(in.p, n, c.p, lit - 1, &e) == -1);
  }

  Heap chunk(len);
  std::memcpy(chunk.p, a.p, (size_t)len);
  Heap back(n);
  REQUIRE(snappy::unsnap_one(chunk.p, len, back.p, n) == snappy::SN_OK);
  REQUIRE(n == 0 || std::memcmp(back.p, in.p, (size_t)n) == 0);
  ++g_runs;
}

static Bytes repeat_case(size_t length, size_t dist) {
  Bytes s = random_bytes(length), d = s;
  append(d, random_bytes(dist - length));
  append(d, s);
  append(d, random_bytes(37));
  return d;
}

static void named_cases() {
  check("empty", Bytes());
  for (size_t n : {1, 3, 4, 63, 64, 65}) check("random_short", random_bytes(n));
  Bytes abcd;
  for (int i = 0; i < 5000; ++i) append(abcd, Bytes{'a', 'b', 'c', 'd'});
  check("abcd_x5000", abcd);
  check("zeros_65536", Bytes(65536, 0));
  check("zeros_4464", Bytes(70000 - 65536, 0));
  check("random_64k", random_bytes(64 << 10));
  check("letters_64k", random_bytes(64 << 10, 97, 123));
  {
    Bytes r = random_bytes(100), d = r;
    append(d, r, 80);
    append(d, random_bytes(20));
    check("match_crosses_window", d);
  }
  {
    Bytes r = random_bytes(200), d = r;
    append(d, r, 50);
    check("match_ends_at_block_end", d);
  }
  for (size_t length : {11, 12})
    for (size_t dist : {2047, 2048}) check("tag_edge", repeat_case(length, dist));
  for (size_t length : {64, 65, 67, 68})
    check("split_rule", repeat_case(length, length + 100));
  for (size_t gap : {60, 61, 256, 257}) {
    Bytes s = random_bytes(20), d = s;
    append(d, random_bytes(70));
    append(d, s);
    append(d, random_bytes(gap));
    append(d, s);
    append(d, random_bytes(31));
    check("literal_between_matches", d);
  }
  {
    Bytes far = random_bytes(65537), d = far;
    append(d, far, 60000);
    check("repeat_beyond_65535_in_128k", d);
  }
  {
    // a record-like block: a fixed skeleton with a few varying bytes
    Bytes rec = random_bytes(215), d;
    while (d.size() < 65536) {
      Bytes r = rec;
      for (int k = 0; k < 12; ++k) r[rnd() % r.size()] = (uint8_t)rnd();
      append(d, r);
    }
    d.resize(65536);
    check("records_64k", d);
    d.resize(1000);
    check("records_1000", d);
  }
  check("one_mib_of_text", random_bytes(1 << 20, 97, 101));
  // one 4-byte repeat 2504 back in random bytes: the 3-byte copy saves a
  // byte and the second literal header costs three, so the elements lose
  // to the single literal (whenever the table still holds the first copy)
  for (int t = 0; t < 20; ++t) {
    Bytes s = random_bytes(4), d = s;
    append(d, random_bytes(2500));
    append(d, s);
    append(d, random_bytes(2496));
    check("fallback_after_copy", d);
  }
}

static size_t random_length() {
  uint32_t k = rnd() % 100;
  if (k < 55) return rnd() % 300;
  if (k < 85) return rnd() % 5000;
  return rnd() % 70001;
}

static void random_cases(int count) {
  for (int t = 0; t < count; ++t) {
    const size_t n = random_length();
    Bytes d;
    switch (rnd() % 5) {
      case 0:  // incompressible
        d = random_bytes(n);
        break;
      case 1: {  // a small alphabet: many short matches at every distance
        uint32_t lo = rnd() % 250;
        d = random_bytes(n, lo, lo + 2 + rnd() % 4);
        break;
      }
      case 2: {  // runs of one byte value of every length
        while (d.size() < n) {
          size_t run = 1 + rnd() % (rnd() % 8 ? 40 : 3000);
          d.insert(d.end(), run, (uint8_t)rnd());
        }
        d.resize(n);
        break;
      }
      case 3: {  // a short period, with the odd byte changed
        Bytes unit = random_bytes(1 + rnd() % 70);
        while (d.size() < n) append(d, unit);
        d.resize(n);
        for (size_t k = 0; k < n / 500; ++k) d[rnd() % n] = (uint8_t)rnd();
        break;
      }
      default: {  // random pieces, each copied from further back or fresh
        while (d.size() < n) {
          size_t len = 1 + rnd() % 90;
          if (d.size() > 4 && rnd() % 2) {
            size_t from = rnd() % d.size();
            for (size_t k = 0; k < len; ++k) d.push_back(d[from + k]);
          } else {
            append(d, random_bytes(len));
          }
        }
        d.resize(n);
      }
    }
    check("random", d);
  }
}

int main() {
  named_cases();
  random_cases(3000);
  if (g_fallbacks == 0) {
    std::fprintf(stderr, "FAIL no input reached the fallback rewrite\n");
    return 1;
  }
  std::printf("snappy_enc_selftest: %d inputs ok (%d through the fallback)\n",
              g_runs, g_fallbacks);
  return 0;
}
