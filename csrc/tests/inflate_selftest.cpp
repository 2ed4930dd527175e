// Stand-alone host check of the segment inflater core (inflate_one) in the
// three shapes the kernels of csrc/hip/inflate.hip instantiate: <64> (whole
// wave), <32> (half-wave pairs) and <16, 9, 7> (quarter-wave, narrower root
// tables). A representative subset of tests/inflate_cases.py is regenerated
// here with a small bit writer and PRNG: the block with lit/len and distance
// codes of every length 1..15, the match geometry at the copy-path switches,
// stored blocks at every byte residue, several blocks per segment, one
// malformed segment per cause code, every truncation of the valid ones, and
// random byte soup. Each run gets exact-size heap blocks for the input, the
// output and both root tables, so one byte read or written past any end
// trips the sanitizer. A segment runs once serially (lane = -1; the bytes
// must match) and once per lane (lane = 0..NLANES-1, the device's share of
// the lane-split copies and table fill). One lane alone leaves holes in the
// output, so there only the bounds and the return code count. It leaves
// holes in the root tables too, which the other lanes fill on the device:
// here the lane starts from the tables the serial run ended with, so in a
// segment with one Huffman code (all but the several-block cases) it sees
// whole tables and must return what the serial run returned, since the
// decode never reads the output to decide anything; with several codes
// only the bounds count. The two lane-split helpers are also checked on
// their own: all lanes' shares of fill_huff_table and of bulk_copy, put
// together, must be exactly the serial result, each element written once.
// Meant to be built with sanitizers and run as its own executable on the
// CPU (ROCm's clang++: the core uses a clang builtin):
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -fno-sanitize-recover=all csrc/tests/inflate_selftest.cpp \
//       -o inflate_selftest && ./inflate_selftest
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../inflate_core.h"

using namespace tfrec::inflate;
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

// LSB-first bit packer (RFC 1951 3.1.1).
struct BitWriter {
  Bytes out;
  uint64_t acc = 0;
  int n = 0;
  void bits(uint32_t v, int k) {
    acc |= (uint64_t)(v & ((1ull << k) - 1)) << n;
    n += k;
    while (n >= 8) {
      out.push_back((uint8_t)acc);
      acc >>= 8;
      n -= 8;
    }
  }
  void code(uint32_t c, int k) {  // Huffman codes go in MSB first
    uint32_t rev = 0;
    for (int i = 0; i < k; ++i) rev |= ((c >> i) & 1u) << (k - 1 - i);
    bits(rev, k);
  }
  void align() {
    if (n) bits(0, 8 - n);
  }
  size_t bit_length() const { return 8 * out.size() + (size_t)n; }
  Bytes value() const {
    BitWriter w = *this;
    w.align();
    return w.out;
  }
};

struct Code {
  std::vector<uint32_t> code;
  std::vector<int> len;
};

// Canonical code (RFC 1951 3.2.2) from lengths indexed by symbol.
static Code canonical(const std::vector<int>& lens) {
  int count[16] = {0};
  for (int l : lens) ++count[l];
  count[0] = 0;
  uint32_t nxt[16] = {0}, c = 0;
  for (int l = 1; l < 16; ++l) {
    c = (c + (uint32_t)count[l - 1]) << 1;
    nxt[l] = c;
  }
  Code out;
  out.len = lens;
  out.code.assign(lens.size(), 0);
  for (size_t s = 0; s < lens.size(); ++s)
    if (lens[s]) out.code[s] = nxt[lens[s]]++;
  return out;
}

static std::vector<int> lens_of(const std::map<int, int>& pairs, int n) {
  std::vector<int> out((size_t)n, 0);
  for (auto& p : pairs) out[(size_t)p.first] = p.second;
  return out;
}

static std::vector<int> fixed_lit_lens() {
  std::vector<int> l(288, 8);
  for (int s = 144; s < 256; ++s) l[(size_t)s] = 9;
  for (int s = 256; s < 280; ++s) l[(size_t)s] = 7;
  return l;
}

// the code-length code of every dynamic header here: complete, all 19 used
static std::vector<int> cl_lens() {
  std::vector<int> l(19, 4);
  for (int s = 13; s < 19; ++s) l[(size_t)s] = 5;
  return l;
}

// One raw-deflate segment, assembled block by block and played forward.
struct Stream {
  BitWriter w;
  Bytes data;
  Code lit, dist;
  int ncodes = 0;  // Huffman blocks so far

  Stream& stored(const Bytes& p, bool final = false) {
    w.bits(final ? 1 : 0, 1);
    w.bits(0, 2);
    w.align();
    uint32_t n = (uint32_t)p.size();
    w.bits(n, 16);
    w.bits(n ^ 0xFFFFu, 16);
    w.out.insert(w.out.end(), p.begin(), p.end());
    data.insert(data.end(), p.begin(), p.end());
    return *this;
  }
  Stream& sync() { return stored({}); }
  Stream& fixed(bool final = false) {
    w.bits(final ? 1 : 0, 1);
    w.bits(1, 2);
    ++ncodes;
    lit = canonical(fixed_lit_lens());
    dist = canonical(std::vector<int>(32, 5));
    return *this;
  }
  static void dyn_counts(BitWriter& w, bool final, int hlit, int hdist,
                         const std::vector<int>& cl) {
    w.bits(final ? 1 : 0, 1);
    w.bits(2, 2);
    w.bits((uint32_t)(hlit - 257), 5);
    w.bits((uint32_t)(hdist - 1), 5);
    w.bits(19 - 4, 4);
    for (int i = 0; i < 19; ++i) w.bits((uint32_t)cl[kClOrder[i]], 3);
  }
  Stream& dynamic(const std::vector<int>& ll, const std::vector<int>& dl,
                  bool final = false) {
    Code cl = canonical(cl_lens());
    ++ncodes;
    dyn_counts(w, final, (int)ll.size(), (int)dl.size(), cl_lens());
    std::vector<int> seq(ll);
    seq.insert(seq.end(), dl.begin(), dl.end());
    for (size_t i = 0; i < seq.size();) {
      int v = seq[i];
      size_t run = 1;
      while (i + run < seq.size() && seq[i + run] == v) ++run;
      if (v == 0 && run >= 3) {
        size_t take = run > 138 ? 138 : run;
        if (take >= 11) {
          w.code(cl.code[18], cl.len[18]);
          w.bits((uint32_t)(take - 11), 7);
        } else {
          w.code(cl.code[17], cl.len[17]);
          w.bits((uint32_t)(take - 3), 3);
        }
        i += take;
      } else if (v && run >= 4) {
        size_t take = run - 1 > 6 ? 6 : run - 1;
        w.code(cl.code[(size_t)v], cl.len[(size_t)v]);
        w.code(cl.code[16], cl.len[16]);
        w.bits((uint32_t)(take - 3), 2);
        i += 1 + take;
      } else {
        w.code(cl.code[(size_t)v], cl.len[(size_t)v]);
        ++i;
      }
    }
    lit = canonical(ll);
    dist = canonical(dl);
    return *this;
  }
  Stream& sym(int s) {
    if (!lit.len[(size_t)s]) {
      std::printf("FAIL generator: symbol %d has no code\n", s);
      std::exit(2);
    }
    w.code(lit.code[(size_t)s], lit.len[(size_t)s]);
    return *this;
  }
  Stream& lits(const Bytes& p) {
    for (uint8_t b : p) {
      sym(b);
      data.push_back(b);
    }
    return *this;
  }
  Stream& lits(const char* s) {
    return lits(Bytes(s, s + std::strlen(s)));
  }
  Stream& match(int length, int distance, int len_sym = -1,
                bool play = true) {
    int ls = len_sym;
    if (ls < 0)
      for (ls = 28; kLenBase[ls] > length; --ls) {
      }
    sym(257 + ls);
    w.bits((uint32_t)(length - kLenBase[ls]), kLenExtra[ls]);
    int ds = 29;
    while (kDistBase[ds] > distance) --ds;
    if (!dist.len[(size_t)ds]) {
      std::printf("FAIL generator: distance code %d has no code\n", ds);
      std::exit(2);
    }
    w.code(dist.code[(size_t)ds], dist.len[(size_t)ds]);
    w.bits((uint32_t)(distance - kDistBase[ds]), kDistExtra[ds]);
    if (play) {
      if ((size_t)distance > data.size()) {
        std::printf("FAIL generator: distance %d too far\n", distance);
        std::exit(2);
      }
      for (int i = 0; i < length; ++i)
        data.push_back(data[data.size() - (size_t)distance]);
    }
    return *this;
  }
  Stream& end() { return sym(256); }
  Bytes comp() const { return w.value(); }
};

// Root tables as a run left them, to start a single lane's run from.
struct Tables {
  std::vector<uint16_t> lit, dist;
};

// One run of one instantiation over exact-size blocks.
template <int NL, int LB, int DB>
static int run(const Bytes& comp, int64_t expect, int lane, Bytes* got,
               Tables* tabs) {
  std::unique_ptr<u8[]> in(new u8[comp.size() ? comp.size() : 1]);
  if (!comp.empty()) std::memcpy(in.get(), comp.data(), comp.size());
  // a zero-length range still needs a pointer the core must not touch
  std::unique_ptr<u8[]> out(new u8[expect ? expect : 1]);
  std::memset(out.get(), 0xA5, expect ? (size_t)expect : 1);
  std::unique_ptr<uint16_t[]> lit_tab(new uint16_t[1 << LB]);
  std::unique_ptr<uint16_t[]> dist_tab(new uint16_t[1 << DB]);
  if (lane < 0) {
    std::memset(lit_tab.get(), 0, sizeof(uint16_t) << LB);
    std::memset(dist_tab.get(), 0, sizeof(uint16_t) << DB);
  } else {
    std::memcpy(lit_tab.get(), tabs->lit.data(), sizeof(uint16_t) << LB);
    std::memcpy(dist_tab.get(), tabs->dist.data(), sizeof(uint16_t) << DB);
  }
  std::unique_ptr<LaneScratch> L(new LaneScratch);
  std::memset(L.get(), 0, sizeof(LaneScratch));
  int rc = inflate_one<NL, LB, DB>(
      comp.empty() ? in.get() + 1 : in.get(), (i64)comp.size(),
      expect ? out.get() : out.get() + 1, expect, *L, lit_tab.get(),
      dist_tab.get(), lane);
  if (got) got->assign(out.get(), out.get() + expect);
  if (lane < 0) {
    tabs->lit.assign(lit_tab.get(), lit_tab.get() + (1 << LB));
    tabs->dist.assign(dist_tab.get(), dist_tab.get() + (1 << DB));
  }
  return rc;
}

static int g_fail = 0;

// Serial return code, or -1 (and a FAIL line) when `same_rc` is asked and
// some lane disagrees.
template <int NL, int LB, int DB>
static int run_all_lanes(const std::string& name, const Bytes& comp,
                         int64_t expect, Bytes* got, bool every_lane,
                         bool same_rc) {
  Tables tabs;
  int rc = run<NL, LB, DB>(comp, expect, -1, got, &tabs);
  for (int lane = 0; lane < NL; ++lane) {
    if (!every_lane && lane != 0 && lane != NL / 2 + 1 && lane != NL - 1)
      continue;
    int r = run<NL, LB, DB>(comp, expect, lane, nullptr, &tabs);
    if (same_rc && r != rc) {
      std::printf("FAIL %s <%d,%d,%d>: lane %d rc %d, serial rc %d\n",
                  name.c_str(), NL, LB, DB, lane, r, rc);
      ++g_fail;
      return -1;
    }
  }
  return rc;
}

template <int NL, int LB, int DB>
static bool valid_one(const std::string& name, const Bytes& comp,
                      const Bytes& want, bool one_code) {
  Bytes got;
  int rc = run_all_lanes<NL, LB, DB>(name, comp, (int64_t)want.size(), &got,
                                     true, one_code);
  if (rc < 0) return false;
  if (rc || got != want) {
    std::printf("FAIL %s <%d,%d,%d>: rc %d, bytes %s\n", name.c_str(), NL, LB,
                DB, rc, got == want ? "equal" : "differ");
    ++g_fail;
    return false;
  }
  return true;
}

// Every truncation: within bounds, every lane agreeing on the code. (A cut
// inside the closing sync block or the last padding may still be accepted:
// all of the output is there.)
template <int NL, int LB, int DB>
static bool cuts_one(const std::string& name, const Bytes& comp,
                     int64_t expect, bool one_code) {
  size_t step = comp.size() > 2048 ? comp.size() / 256 : 1;
  for (size_t cut = 0; cut < comp.size(); cut += step) {
    Bytes part(comp.begin(), comp.begin() + (long)cut);
    if (run_all_lanes<NL, LB, DB>(name + " cut " + std::to_string(cut), part,
                                  expect, nullptr, false, one_code) < 0)
      return false;
  }
  return true;
}

static void check_valid(const std::string& name, const Stream& s) {
  Bytes comp = s.comp();
  bool one = s.ncodes <= 1;
  int64_t n = (int64_t)s.data.size();
  bool ok = valid_one<64, 10, 8>(name, comp, s.data, one) &&
            valid_one<32, 10, 8>(name, comp, s.data, one) &&
            valid_one<16, 9, 7>(name, comp, s.data, one) &&
            cuts_one<64, 10, 8>(name, comp, n, one) &&
            cuts_one<32, 10, 8>(name, comp, n, one) &&
            cuts_one<16, 9, 7>(name, comp, n, one);
  if (ok)
    std::printf("ok   %s (%zu -> %zu)\n", name.c_str(), comp.size(),
                s.data.size());
}

static void check_bad(const std::string& name, const Bytes& comp,
                      int64_t expect, int cause) {
  int rc[3] = {
      run_all_lanes<64, 10, 8>(name, comp, expect, nullptr, true, true),
      run_all_lanes<32, 10, 8>(name, comp, expect, nullptr, true, true),
      run_all_lanes<16, 9, 7>(name, comp, expect, nullptr, true, true)};
  for (int r : rc) {
    if (r < 0) return;
    if (r != cause) {
      std::printf("FAIL %s: rc %d, want %d\n", name.c_str(), r, cause);
      ++g_fail;
      return;
    }
  }
  std::printf("ok   %s (cause %d)\n", name.c_str(), cause);
}

// lit/len lengths 1..15,15 and distance lengths 1..15,15 (the long-code
// block of tests/inflate_cases.py)
static const std::map<int, int> kLongLit = {
    {'a', 1}, {'b', 2},  {'c', 3},  {257, 4},  {'d', 5},  {264, 6},
    {'e', 7}, {285, 8},  {'f', 9},  {'g', 10}, {'h', 11}, {265, 12},
    {256, 13}, {'i', 14}, {0xFF, 15}, {284, 15}};
static const std::map<int, int> kLongDist = {
    {0, 1},   {6, 2},   {1, 3},   {16, 4},  {2, 5},   {29, 6},
    {3, 7},   {4, 8},   {5, 9},   {28, 10}, {10, 11}, {13, 12},
    {20, 13}, {22, 14}, {25, 15}, {27, 15}};

static Bytes skewed(size_t n) {
  static const uint8_t sym[10] = {'a', 'b', 'c', 'd', 'e',
                                  'f', 'g', 'h', 'i', 0xFF};
  static const uint32_t upto[10] = {50, 70, 80, 86, 90, 93, 96, 98, 99, 100};
  Bytes b(n);
  for (auto& x : b) {
    uint32_t r = rnd() % 100;
    int k = 0;
    while (r >= upto[k]) ++k;
    x = sym[k];
  }
  return b;
}

static Stream long_block(size_t nlit) {
  Stream s;
  s.dynamic(lens_of(kLongLit, 286), lens_of(kLongDist, 30));
  return s.lits(skewed(nlit));
}

static const int kGeometry[][2] = {
    {3, 1},     {258, 1},   {3, 2},       {3, 3},     {3, 4},
    {10, 5},    {10, 7},    {10, 8},      {10, 9},    {10, 10},
    {258, 257}, {258, 258}, {258, 32768}, {3, 24577}, {10, 16385},
    {11, 33},   {12, 48},   {250, 97},    {257, 128}, {3, 1025},
    {10, 1536}, {258, 2049}, {12, 3072},  {227, 6145}, {10, 8192},
    {11, 12289}, {258, 16384}};

// All lanes' shares of a root-table fill, put together: the serial table,
// every entry written by exactly one lane.
template <int BITS>
static void check_fill(const char* what, const std::vector<int>& lens,
                       int nlanes) {
  LaneScratch L;
  std::memset(&L, 0, sizeof L);
  for (size_t s = 0; s < lens.size(); ++s)
    set_len4(L.lens4, (int)s, (u32)lens[s]);
  if (!build_huff4(L.lens4, 0, (int)lens.size(), L.bc_lit, L.rank_lit,
                   L.sym)) {
    std::printf("FAIL fill %s: code refused\n", what);
    ++g_fail;
    return;
  }
  const int size = 1 << BITS;
  std::unique_ptr<uint16_t[]> serial(new uint16_t[size]);
  std::unique_ptr<uint16_t[]> lanes(new uint16_t[size]);
  fill_huff_table<BITS>(L.bc_lit, L.sym, serial.get(), -1, nlanes);
  const uint16_t unset = 0xFFFF;  // no entry: symbols stay below 4096
  for (int i = 0; i < size; ++i) lanes[i] = unset;
  int written = 0;
  for (int lane = 0; lane < nlanes; ++lane) {
    std::unique_ptr<uint16_t[]> one(new uint16_t[size]);
    for (int i = 0; i < size; ++i) one[i] = unset;
    fill_huff_table<BITS>(L.bc_lit, L.sym, one.get(), lane, nlanes);
    for (int i = 0; i < size; ++i) {
      if (one[i] == unset) continue;
      if (lanes[i] != unset) written = -size;  // two lanes, one entry
      lanes[i] = one[i];
      ++written;
    }
  }
  if (written != size || std::memcmp(serial.get(), lanes.get(),
                                     sizeof(uint16_t) * (size_t)size)) {
    std::printf("FAIL fill %s <%d> over %d lanes\n", what, BITS, nlanes);
    ++g_fail;
  }
}

// All lanes' shares of a bulk copy, put together: every byte of [0, n)
// copied by exactly one lane, none beyond (the blocks are exact-size).
static void check_bulk_copy(int nlanes) {
  for (i64 n = 0; n <= 8 * nlanes * 2 + 17; ++n) {
    Bytes src = random_bytes((size_t)n);
    std::unique_ptr<u8[]> in(new u8[n ? n : 1]);
    if (n) std::memcpy(in.get(), src.data(), (size_t)n);
    std::vector<int> hits((size_t)n, 0);
    for (int lane = 0; lane < nlanes; ++lane) {
      std::unique_ptr<u8[]> out(new u8[n ? n : 1]);
      // the complement of the source marks what this lane left alone
      for (i64 i = 0; i < n; ++i) out[i] = (u8)~src[(size_t)i];
      bulk_copy(out.get(), in.get(), n, lane, nlanes);
      for (i64 i = 0; i < n; ++i)
        if (out[i] == src[(size_t)i]) ++hits[(size_t)i];
    }
    for (i64 i = 0; i < n; ++i)
      if (hits[(size_t)i] != 1) {
        std::printf("FAIL bulk_copy n %lld over %d lanes: byte %lld copied "
                    "%d times\n", (long long)n, nlanes, (long long)i,
                    hits[(size_t)i]);
        ++g_fail;
        return;
      }
  }
  std::printf("ok   bulk_copy shares over %d lanes\n", nlanes);
}

int main() {
  for (int nlanes : {64, 32, 16}) check_bulk_copy(nlanes);
  for (int nlanes : {64, 32, 16}) {
    check_fill<10>("long lit/len", lens_of(kLongLit, 286), nlanes);
    check_fill<9>("long lit/len", lens_of(kLongLit, 286), nlanes);
    check_fill<10>("fixed lit/len", fixed_lit_lens(), nlanes);
    check_fill<9>("fixed lit/len", fixed_lit_lens(), nlanes);
    check_fill<8>("long distance", lens_of(kLongDist, 30), nlanes);
    check_fill<7>("long distance", lens_of(kLongDist, 30), nlanes);
  }
  if (!g_fail) std::printf("ok   fill_huff_table shares\n");
  const std::vector<int> simple_lit =
      lens_of({{'x', 1}, {'y', 2}, {256, 3}, {258, 4}, {285, 4}}, 286);
  // long codes + match geometry, each match after 0..9 pending literals
  {
    Stream s = long_block(33000);
    for (auto& g : kGeometry) s.match(g[0], g[1]);
    int k = 0;
    for (auto& g : kGeometry) s.lits(skewed(1 + k++ % 9)).match(g[0], g[1]);
    s.match(258, 1, 27);  // length 258 spelled 227 + 31
    for (int tail : {0, 3, 8, 9}) {
      Stream t = s;
      t.lits(skewed((size_t)tail)).end();
      if (tail & 1) t.sync(); else t.stored({}, true);
      check_valid("long_geometry_tail_" + std::to_string(tail), t);
    }
  }
  for (auto& g : kGeometry) {
    if (g[1] > 258) continue;
    Stream s = long_block(300);
    s.match(g[0], g[1]).lits(skewed(5)).match(g[0], g[1]).end().sync();
    check_valid("long_len" + std::to_string(g[0]) + "_dist" +
                    std::to_string(g[1]), s);
  }
  // several blocks; later matches reach into earlier blocks
  for (bool final : {true, false}) {
    Stream s;
    Bytes text = random_bytes(260, 97, 101);
    s.fixed().lits(Bytes(text.begin(), text.begin() + 200)).match(30, 200);
    s.match(258, 1).lits(Bytes(text.begin() + 200, text.end())).end();
    s.dynamic(lens_of(kLongLit, 286), lens_of(kLongDist, 30));
    s.lits(skewed(150)).match(258, 257).match(10, 5).lits("abc").end();
    s.stored(random_bytes(100));
    s.dynamic(simple_lit,
              lens_of({{0, 2}, {5, 2}, {12, 2}, {16, 3}, {18, 4}, {19, 4}}, 30),
              final);
    s.match(258, 1000).match(4, 90).match(258, 8).match(258, 300);
    s.match(258, 700).lits("xyx").match(4, 1).match(258, 96).end();
    if (!final) s.sync();
    check_valid(final ? "blocks_final" : "blocks_sync", s);
  }
  {
    Stream s;
    check_valid("end_of_block_only", s.fixed(true).end());
    Stream e;
    check_valid("empty_sync_only", e.sync());
    Stream n;
    n.dynamic(simple_lit, {0}, true).lits("xyyxxxyxyxxyxyyx").end();
    check_valid("no_distance_code", n);
    Stream o;
    o.dynamic(simple_lit, {1}, true).lits("xy").match(4, 1).lits("x");
    check_valid("one_distance_code",
                o.match(258, 1).match(4, 1).lits("yyx").end());
    Stream f;
    f.fixed(true).lits(random_bytes(3001, 0, 144)).end();
    check_valid("fixed_literals", f);
  }
  // stored blocks at every byte residue of the 8-byte prefetch word
  {
    const size_t first[] = {0, 1, 7, 8, 9, 63, 64, 65, 511, 513};
    const size_t second[] = {512, 257, 255, 129, 127, 256, 128, 3, 1000, 0};
    for (int r = 0; r < 9; ++r)
      for (int k = 0; k < 10; ++k) {
        Stream s;
        s.fixed().lits(Bytes((size_t)r, (uint8_t)('A' + r))).end();
        s.stored(random_bytes(first[k]));
        bool final = (r + k) % 2 == 0;
        s.stored(random_bytes(second[k]), final);
        if (!final) s.sync();
        check_valid("stored_after_" + std::to_string(r) + "_literals_" +
                        std::to_string(first[k]) + "_" +
                        std::to_string(second[k]), s);
      }
    Stream big;
    check_valid("stored_65535", big.stored(random_bytes(65535), true));
    Stream m;
    m.stored(random_bytes(300)).fixed(true).match(258, 300).match(10, 10);
    m.lits("tail").match(42, 300 + 258 + 14).end();
    check_valid("match_reads_stored_bytes", m);
  }
  // one malformed segment per cause code (tests/inflate_cases.py has the
  // reasoning for each)
  {
    Stream ok;
    ok.fixed(true).lits("abcabc").match(5, 3).lits("!").end();
    int64_t want = (int64_t)ok.data.size();
    Bytes okc = ok.comp();
    check_bad("no_block_header", {}, 5, 1);
    check_bad("stored_nlen_mismatch",
              {1, 5, 0, 0, 0, 'h', 'e', 'l', 'l', 'o'}, 5, 2);
    check_bad("stored_past_input", {1, 5, 0, 0xFA, 0xFF, 'h', 'e', 'l'}, 5, 3);
    check_bad("stored_past_output",
              {1, 5, 0, 0xFA, 0xFF, 'h', 'e', 'l', 'l', 'o'}, 4, 3);
    check_bad("block_type_3", {7, 0}, 1, 4);
    check_bad("dynamic_counts_cut", {5}, 1, 5);
    {
      BitWriter w;
      std::vector<int> cl(19, 0);
      cl[0] = cl[1] = cl[2] = 1;
      Stream::dyn_counts(w, true, 257, 1, cl);
      w.bits(0, 16);
      check_bad("code_length_code_oversubscribed", w.value(), 1, 6);
    }
    {
      BitWriter w;
      std::vector<int> cl(19, 0);
      cl[0] = 1;
      Stream::dyn_counts(w, true, 257, 1, cl);
      w.bits(0xFFFF, 16);
      check_bad("code_length_symbol_unassigned", w.value(), 1, 7);
    }
    {
      BitWriter w;
      Code cl = canonical(cl_lens());
      Stream::dyn_counts(w, true, 257, 1, cl_lens());
      w.code(cl.code[18], cl.len[18]);
      w.bits(127, 7);
      Bytes c = w.value();
      c.resize(10);  // bit 80 of 86: one of the repeat's 7 extra bits
      check_bad("repeat_extra_bits_cut", c, 1, 8);
    }
    {
      Stream s;
      s.dynamic(lens_of({{65, 1}, {66, 1}, {256, 1}}, 257), {0}, true);
      Bytes c = s.comp();
      c.insert(c.end(), 2, 0);
      check_bad("litlen_code_oversubscribed", c, 1, 9);
      Stream d;
      d.dynamic(simple_lit, {1, 1, 1}, true);
      c = d.comp();
      c.insert(c.end(), 2, 0);
      check_bad("distance_code_oversubscribed", c, 1, 10);
    }
    check_bad("symbols_cut", Bytes(okc.begin(), okc.begin() + 4), want, 11);
    check_bad("literal_past_output", okc, want - 1, 12);
    for (int sym : {286, 287}) {
      Stream s;
      s.fixed(true).lits("abc").sym(sym);
      s.w.bits(0, 24);
      check_bad("length_symbol_" + std::to_string(sym), s.comp(), 10, 13);
    }
    for (int sym : {30, 31}) {
      Stream s;
      s.fixed(true).lits("abc").sym(257);
      s.w.code(s.dist.code[(size_t)sym], 5);
      s.w.bits(0, 24);
      check_bad("distance_symbol_" + std::to_string(sym), s.comp(), 10, 14);
    }
    {
      Stream s;
      s.fixed(true).lits("a").match(3, 32768, -1, false);
      Bytes c = s.comp();
      c.resize(3);  // bit 24 of 36: one of the distance's 13 extra bits
      check_bad("distance_extra_bits_cut", c, 4, 15);
      Stream f;
      f.fixed(true).lits("a").match(3, 2, -1, false).end();
      check_bad("distance_before_start", f.comp(), 4, 16);
      Stream p;
      p.fixed(true).lits("abc").match(10, 3).end();
      check_bad("match_past_output", p.comp(), 12, 16);
    }
    check_bad("final_block_ends_short", okc, want + 1, 17);
  }
  // random byte soup behind every block type: only bounds and lane
  // agreement matter
  for (int k = 0; k < 3000; ++k) {
    Bytes soup = random_bytes(1 + rnd() % 120);
    int64_t expect = rnd() % 400;
    if (k % 3 == 1) soup[0] = (uint8_t)((soup[0] & ~7u) | 3u);  // fixed
    if (k % 3 == 2) soup[0] = (uint8_t)((soup[0] & ~7u) | 5u);  // dynamic
    std::string name = "soup " + std::to_string(k);
    run_all_lanes<64, 10, 8>(name, soup, expect, nullptr, false, false);
    run_all_lanes<32, 10, 8>(name, soup, expect, nullptr, false, false);
    run_all_lanes<16, 9, 7>(name, soup, expect, nullptr, false, false);
  }
  std::printf("ok   byte soup x3000\n");
  if (g_fail) {
    std::printf("%d case(s) FAILED\n", g_fail);
    return 1;
  }
  std::printf("all inflate core cases passed\n");
  return 0;
}
