// Stand-alone host check of the speculative foreign-gzip inflater core
// (csrc/inflate_spec_core.h): streams are generated here with zlib, the
// foreign writer, over the kinds of input of tests/foreign_gz_cases.py
// (regenerated with a small PRNG), inflated by host_spec_inflate at several
// chunk strides and compared to the input; damaged copies must be refused.
// Meant to be built with sanitizers and run as its own executable on the
// CPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -fno-sanitize-recover=all csrc/tests/inflate_foreign_selftest.cpp \
//       -lz -o inflate_foreign_selftest && ./inflate_foreign_selftest
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../inflate_spec_core.h"

using namespace tfrec;
using Bytes = std::vector<uint8_t>;

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint32_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static Bytes random_bytes(size_t n, uint32_t lo, uint32_t hi) {
  Bytes b(n);
  for (auto& x : b) x = (uint8_t)(lo + rnd() % (hi - lo));
  return b;
}

// One gzip member around zlib's raw deflate of `data`; `flush_at` > 0 puts
// a flush of mode `flush` there.
static Bytes gzip_of(const Bytes& data, int level, int mem_level,
                     size_t flush_at = 0, int flush = Z_SYNC_FLUSH) {
  z_stream z;
  std::memset(&z, 0, sizeof z);
  deflateInit2(&z, level, Z_DEFLATED, -15, mem_level, Z_DEFAULT_STRATEGY);
  Bytes body(deflateBound(&z, (uLong)data.size()) + 64);
  z.next_out = body.data();
  z.avail_out = (uInt)body.size();
  static uint8_t none = 0;
  z.next_in = data.empty() ? &none : const_cast<uint8_t*>(data.data());
  const size_t first = flush_at < data.size() ? flush_at : 0;
  if (first) {
    z.avail_in = (uInt)first;
    deflate(&z, flush);
  }
  z.avail_in = (uInt)(data.size() - first);  // zlib advanced next_in
  deflate(&z, Z_FINISH);
  body.resize(z.total_out);
  deflateEnd(&z);
  Bytes gz = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};
  gz.insert(gz.end(), body.begin(), body.end());
  uint32_t crc = (uint32_t)crc32(0, data.empty() ? &none : data.data(),
                                 (uInt)data.size());
  uint32_t isize = (uint32_t)data.size();
  for (int i = 0; i < 4; ++i) gz.push_back((uint8_t)(crc >> (8 * i)));
  for (int i = 0; i < 4; ++i) gz.push_back((uint8_t)(isize >> (8 * i)));
  return gz;
}

// Runs the core on an exact-size heap copy (one byte past either end trips
// the sanitizer). want = nullptr: the stream must be refused.
static int run(const char* name, const Bytes& gz, const Bytes* want,
               int64_t chunk, inflate::SpecStats* st_out = nullptr) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[gz.size()]);
  std::memcpy(in.get(), gz.data(), gz.size());
  Bytes out;
  inflate::SpecStats st;
  int64_t err = inflate::host_spec_inflate(in.get(), (int64_t)gz.size(), chunk,
                                           out, st);
  if (st_out) *st_out = st;
  if (!want) {
    if (err == 0) {
      std::printf("FAIL %s chunk %lld: damaged stream accepted\n", name,
                  (long long)chunk);
      return 1;
    }
    return 0;
  }
  if (err || out != *want) {
    std::printf("FAIL %s chunk %lld: err %lld\n", name, (long long)chunk,
                (long long)err);
    return 1;
  }
  return 0;
}

int main() {
  struct Case {
    std::string name;
    Bytes data;
    int level, mem_level;
    size_t flush_at;
    int flush;
  };
  std::vector<Case> cases;
  Bytes text = random_bytes(200000, 65, 75);
  cases.push_back({"dyn_small_blocks", text, 6, 1, 0, 0});
  cases.push_back({"dyn_default", text, 6, 8, 0, 0});
  cases.push_back({"stored", random_bytes(100000, 0, 256), 6, 8, 0, 0});
  Bytes mix;
  const char* words[] = {"feature", "int64_list", "bytes_list", "value",
                         "float_list", "label", "tfrecord", "key"};
  while (mix.size() < 300000) {
    uint32_t k = rnd() % 11;
    if (k < 8)
      mix.insert(mix.end(), words[k], words[k] + std::strlen(words[k]));
    else
      mix.push_back((uint8_t)rnd());
  }
  cases.push_back({"fixed_mix", mix, 6, 2, 0, 0});
  cases.push_back({"one_byte", Bytes(1, 'x'), 6, 8, 0, 0});
  Bytes block = random_bytes(32768 - 262, 97, 123);
  Bytes twice = block;
  twice.insert(twice.end(), block.begin(), block.end());
  cases.push_back({"window_edge", twice, 9, 1, 0, 0});
  Bytes far = random_bytes(40000, 0, 256);
  Bytes far2 = far;
  far2.insert(far2.end(), far.begin(), far.end());
  cases.push_back({"far_repeat", far2, 6, 1, 0, 0});
  Bytes part(text.begin(), text.begin() + 120000);
  cases.push_back({"sync_flush", part, 6, 8, 60000, Z_SYNC_FLUSH});
  cases.push_back({"full_flush", part, 6, 8, 60000, Z_FULL_FLUSH});

  int bad = 0;
  for (const auto& c : cases) {
    Bytes gz = gzip_of(c.data, c.level, c.mem_level, c.flush_at, c.flush);
    for (int64_t chunk : {int64_t(1024), int64_t(4096), int64_t(32768),
                          (int64_t)gz.size() + 1})
      bad += run(c.name.c_str(), gz, &c.data, chunk);
  }
  // the small-block stream must really run in parallel, through markers
  {
    Bytes gz = gzip_of(text, 6, 1);
    inflate::SpecStats st;
    bad += run("stats", gz, &text, 2048, &st);
    if (st.live < 20 || st.markers <= 0) {
      std::printf("FAIL stats: live %lld markers %lld\n", (long long)st.live,
                  (long long)st.markers);
      ++bad;
    }
    // damaged copies: every one must be refused, none may read or write
    // out of bounds
    Bytes t = gz;
    t.resize(gz.size() / 2);
    t.insert(t.end(), gz.end() - 8, gz.end());
    bad += run("truncated", t, nullptr, 2048);
    Bytes two = gz;
    Bytes small = gzip_of(Bytes(3000, 'q'), 6, 8);
    two.insert(two.end(), small.begin(), small.end());
    bad += run("two_members", two, nullptr, 2048);
    Bytes c1 = gz;
    c1[c1.size() - 8] ^= 1;
    bad += run("bad_crc", c1, nullptr, 2048);
    Bytes c2 = gz;
    c2[c2.size() - 4] ^= 1;
    bad += run("bad_isize", c2, nullptr, 2048);
    for (int k = 0; k < 64; ++k) {
      Bytes f = gz;
      f[10 + rnd() % (gz.size() - 18)] ^= (uint8_t)(1u << (rnd() % 8));
      bad += run("bit_flip", f, nullptr, 1024);
    }
    bad += run("empty", gzip_of(Bytes(), 6, 8), nullptr, 1024);
    bad += run("short", Bytes(gz.begin(), gz.begin() + 17), nullptr, 1024);
    // arbitrary bytes behind a gzip header: must terminate and be refused
    for (int k = 0; k < 16; ++k) {
      Bytes junk = random_bytes(20000, 0, 256);
      junk[0] = 0x1f, junk[1] = 0x8b, junk[2] = 8, junk[3] = 0;
      uint32_t isz = 50000;
      std::memcpy(&junk[junk.size() - 4], &isz, 4);
      bad += run("junk", junk, nullptr, 512);
    }
  }
  std::printf("%zu cases, %d failures\n", cases.size(), bad);
  return bad ? 1 : 0;
}
