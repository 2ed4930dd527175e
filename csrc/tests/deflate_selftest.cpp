// Stand-alone host check of the DEFLATE compressor core: deflate_one, then
// inflate_one, over the inputs of tests/deflate_cases.py (regenerated here
// with a small PRNG), comparing the result to the input. Meant to be built
// with sanitizers and run as its own executable on the CPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -fno-sanitize-recover=all csrc/tests/deflate_selftest.cpp \
//       -o deflate_selftest && ./deflate_selftest
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../deflate_core.h"
#include "../inflate_core.h"

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

static Bytes repeat(const Bytes& p, size_t n) {
  Bytes b(n);
  for (size_t i = 0; i < n; ++i) b[i] = p[i % p.size()];
  return b;
}

static int check(const char* name, const Bytes& data, int64_t seg,
                 double threshold) {
  int64_t n = (int64_t)data.size();
  int64_t nseg = n ? (n + seg - 1) / seg : 1;
  for (int64_t s = 0; s < nseg; ++s) {
    int64_t lo = s * seg, u = n - lo < seg ? n - lo : seg;
    int64_t cap = deflate::seg_out_bound(u);
    // exact-size heap blocks: one byte past either end trips the sanitizer
    std::unique_ptr<uint8_t[]> in(new uint8_t[u ? u : 1]);
    if (u) std::memcpy(in.get(), data.data() + lo, (size_t)u);
    std::unique_ptr<uint8_t[]> out(new uint8_t[cap]);
    std::unique_ptr<uint32_t[]> toks(new uint32_t[u ? u : 1]);
    std::unique_ptr<deflate::Scratch> S(new deflate::Scratch);
    std::memset(static_cast<void*>(S.get()), 0xA5, sizeof(deflate::Scratch));
    int64_t len = deflate::deflate_one(in.get(), u, out.get(), cap,
                                       s == nseg - 1, threshold, toks.get(),
                                       *S);
    if (len < 0 || len > cap) {
      std::printf("FAIL %s seg %lld: deflate_one -> %lld (cap %lld)\n", name,
                  (long long)s, (long long)len, (long long)cap);
      return 1;
    }
    std::unique_ptr<uint8_t[]> comp(new uint8_t[len ? len : 1]);
    std::memcpy(comp.get(), out.get(), (size_t)len);
    std::unique_ptr<uint8_t[]> back(new uint8_t[u ? u : 1]);
    inflate::LaneScratch L;
    uint16_t lit_tab[inflate::kLitTabSize];
    uint16_t dist_tab[inflate::kDistTabSize];
    int rc = inflate::inflate_one(comp.get(), len, back.get(), u, L, lit_tab,
                                  dist_tab);
    if (rc || (u && std::memcmp(back.get(), in.get(), (size_t)u))) {
      std::printf("FAIL %s seg %lld: inflate rc %d\n", name, (long long)s, rc);
      return 1;
    }
  }
  return 0;
}

int main() {
  const int64_t kSeg = 32 << 10;
  struct Case {
    std::string name;
    Bytes data;
    int64_t seg;
  };
  std::vector<Case> cases;
  for (size_t n = 0; n <= 4; ++n)
    cases.push_back({"len" + std::to_string(n), Bytes(n, 'a'), kSeg});
  cases.push_back({"run258", Bytes(258, 'r'), kSeg});
  cases.push_back({"run259", Bytes(259, 'r'), kSeg});
  cases.push_back({"same32k", Bytes(32768, 0), kSeg});
  cases.push_back({"pattern64", repeat(random_bytes(64, 0, 256), 32768), kSeg});
  cases.push_back({"alpha2", random_bytes(32768, 0, 2), kSeg});
  cases.push_back({"alpha4", random_bytes(32768, 0, 4), kSeg});
  cases.push_back({"alpha25", random_bytes(32768, 97, 122), kSeg});
  cases.push_back({"random128k", random_bytes(128 << 10, 0, 256), 128 << 10});
  Bytes text = random_bytes(2 * 4096 + 7, 97, 122);
  for (size_t n : {size_t(4095), size_t(4096), size_t(4097), text.size()})
    cases.push_back({"text" + std::to_string(n),
                     Bytes(text.begin(), text.begin() + n), 4096});
  Bytes block = random_bytes(40000, 0, 256);
  Bytes twice = block;
  twice.insert(twice.end(), block.begin(), block.end());
  cases.push_back({"far_repeat", twice, 96 << 10});
  Bytes distinct(256);
  for (int i = 0; i < 256; ++i) distinct[i] = (uint8_t)i;
  cases.push_back({"distinct256", distinct, kSeg});
  cases.push_back({"one_distance", repeat(random_bytes(100, 0, 256), 4000),
                   kSeg});
  cases.push_back({"one_literal", Bytes(64, 'a'), kSeg});
  int bad = 0;
  for (const auto& c : cases)
    for (double thr : {0.98, 0.0})
      bad += check(c.name.c_str(), c.data, c.seg, thr);
  std::printf("%zu cases, %d failures\n", cases.size(), bad);
  return bad ? 1 : 0;
}
