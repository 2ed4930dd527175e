// Stand-alone host check of the raw LZ4 block decoder core (unlz4_block) and
// the container block walk (unlz4_container_block): a small table of valid
// and malformed streams assembled here (the kinds of tests/test_lz4_codec.py)
// and played forward for the expected bytes. Each run gets heap blocks of the
// exact sizes, so one byte read or written past either end trips the
// sanitizer; each stream is walked serially, in place and through the staging
// window, and once per lane (lane = 0..63, the device's share of the copies)
// for the bounds of the lane-strided paths. The long streams (the edge cases
// of tests/lz4_cases.py: a token, a literal's end or a bypassed literal at
// every position around the window's edge, three refills, chunk runs) are
// then mutated one byte at a time, 2000 mutants run for lanes -1, 0 and 63,
// so malformed input also reaches a refill, a bypassed literal and a doubling
// round; there only the bounds matter. Meant to be built with sanitizers
// and run as its own executable on the CPU, before the kernel runs on a GPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -fno-sanitize-recover=all csrc/tests/lz4_selftest.cpp \
//       -o lz4_selftest && ./lz4_selftest
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../lz4_core.h"

using namespace tfrec;
using Bytes = std::vector<uint8_t>;

static uint32_t g_state = 2463534242u;
static Bytes rnd(size_t n) {  // xorshift32
  Bytes b(n);
  for (auto& x : b) {
    g_state ^= g_state << 13, g_state ^= g_state >> 17, g_state ^= g_state << 5;
    x = (uint8_t)(g_state >> 11);
  }
  return b;
}

// Assembles a block sequence by sequence and plays it forward; `hdr` lists
// where its tokens, length bytes and offsets stand.
struct Block {
  Bytes comp, out;
  std::vector<size_t> hdr;
  static void ext(Bytes& c, size_t n) {
    if (n < 15) return;
    for (n -= 15; n >= 255; n -= 255) c.push_back(255);
    c.push_back((uint8_t)n);
  }
  // off < 0: the last sequence; `play` false leaves a bad match unplayed
  Block& seq(const Bytes& lit, int off = -1, size_t mlen = 4, bool play = true) {
    size_t m = off < 0 ? 0 : mlen - 4, at = comp.size();
    comp.push_back((uint8_t)((lit.size() < 15 ? lit.size() : 15) << 4 | (m < 15 ? m : 15)));
    ext(comp, lit.size());
    while (at < comp.size()) hdr.push_back(at++);
    comp.insert(comp.end(), lit.begin(), lit.end());
    out.insert(out.end(), lit.begin(), lit.end());
    if (off < 0) return *this;
    at = comp.size();
    comp.push_back((uint8_t)off), comp.push_back((uint8_t)(off >> 8));
    ext(comp, m);
    while (at < comp.size()) hdr.push_back(at++);
    for (size_t i = 0; play && i < mlen; ++i) out.push_back(out[out.size() - off]);
    return *this;
  }
  Block& tail() { return seq(rnd(12)); }
};

static int g_fail = 0;

// One run over exact-size blocks; chunked = `comp` is a container block.
static int64_t run(const Bytes& comp, int64_t cap, int lane, bool window,
                   bool chunked, Bytes* got) {
  // a zero-length range still needs a pointer the core must not touch
  std::unique_ptr<uint8_t[]> in(new uint8_t[comp.size() ? comp.size() : 1]);
  std::copy(comp.begin(), comp.end(), in.get());
  std::unique_ptr<uint8_t[]> out(new uint8_t[cap ? cap : 1]);
  std::unique_ptr<uint64_t[]> win(new uint64_t[lz4::kWindowAlloc / 8]);
  uint8_t* w = window ? (uint8_t*)win.get() : nullptr;
  const uint8_t* ip = comp.empty() ? in.get() + 1 : in.get();
  uint8_t* op = cap ? out.get() : out.get() + 1;
  int64_t rc = chunked ? -lz4::unlz4_container_block(ip, (int64_t)comp.size(), op, cap, lane, w)
                       : lz4::unlz4_block(ip, (int64_t)comp.size(), op, cap, lane, w);
  if (chunked && rc == 0) rc = cap;
  if (got) got->assign(op, op + (rc > 0 ? rc : 0));
  return rc;
}

// want_rc >= 0: bytes produced, and they must equal want; < 0: -cause.
static void check(const std::string& name, const Bytes& comp, int64_t cap,
                  int64_t want_rc, const Bytes& want, bool chunked = false) {
  for (int window = 0; window < 2; ++window) {
    Bytes got;
    int64_t rc = run(comp, cap, -1, window, chunked, &got);
    bool ok = rc == want_rc && (rc < 0 || got == want);
    for (int lane = 0; ok && lane < 64; ++lane)  // a lane always stages
      ok = run(comp, cap, lane, true, chunked, nullptr) == want_rc;
    if (!ok) {
      std::printf("FAIL %s (window %d): rc %lld, want %lld\n", name.c_str(),
                  window, (long long)rc, (long long)want_rc);
      ++g_fail;
      return;
    }
  }
  // no truncation of a valid stream gives as many bytes, all within bounds
  size_t step = comp.size() > 2048 ? comp.size() / 256 : 1;
  for (size_t cut = 0; want_rc >= 0 && cut < comp.size(); cut += step)
    for (int lane : {-1, 0, 63})
      if (run(Bytes(comp.begin(), comp.begin() + cut), cap, lane, lane >= 0,
              chunked, nullptr) >= want_rc) {
        std::printf("FAIL %s: cut at %zu accepted\n", name.c_str(), cut);
        ++g_fail;
        return;
      }
  std::printf("ok   %s (%zu -> %lld)\n", name.c_str(), comp.size(), (long long)want_rc);
}

// The long valid streams, kept for the mutation loop at the end.
struct Long {
  std::string name;
  Bytes comp;
  int64_t cap;
  bool chunked;
  std::vector<size_t> hdr;  // of a raw block: its header bytes
};
static std::vector<Long> g_long;

static void valid(const std::string& name, const Block& b) {
  check(name, b.comp, (int64_t)b.out.size(), (int64_t)b.out.size(), b.out);
  check(name + "+room", b.comp, (int64_t)b.out.size() + 77, (int64_t)b.out.size(), b.out);
  // long in either sense: more input than a window, or (match_5000,
  // match_70000) a match of many doubling rounds
  if (b.comp.size() > 4000 || b.out.size() > 4000) g_long.push_back({name, b.comp, (int64_t)b.out.size(), false, b.hdr});
}

static void be32(Bytes& c, size_t v) {
  for (int s = 24; s >= 0; s -= 8) c.push_back((uint8_t)(v >> s));
}

// The chunk run of a container block, and what it produces.
static Bytes chunks(std::initializer_list<const Block*> parts, Bytes* out) {
  Bytes run;
  for (const Block* c : parts) {
    be32(run, c->comp.size());
    run.insert(run.end(), c->comp.begin(), c->comp.end());
    if (out) out->insert(out->end(), c->out.begin(), c->out.end());
  }
  return run;
}

// Sequences of exactly t bytes (4038..4292): the next token is byte t.
static Block upto(size_t t) {
  Block b;
  b.seq(rnd(4000), 5, 4).seq(rnd(t - 4023), 5, 4);
  if (b.comp.size() != t) std::printf("FAIL upto(%zu) is %zu bytes\n", t, b.comp.size()), ++g_fail;
  return b;
}

// `n` short sequences: literals of 0..20 bytes, matches of 4..40 bytes.
static Block& shorts(Block& b, int n) {
  for (int k = 0; k < n; ++k) {
    Bytes lit = rnd(rnd(1)[0] % 21 + (b.out.empty() ? 1 : 0));
    size_t reach = b.out.size() + lit.size();
    b.seq(lit, 1 + rnd(1)[0] % (reach < 200 ? reach : 200), 4 + rnd(1)[0] % 37);
  }
  return b;
}

int main() {
  for (size_t n : {0, 14, 15, 270, 271})
    valid("literal_" + std::to_string(n), Block().seq(rnd(20), 7, 5).seq(rnd(n), 9, 6).tail());
  for (size_t n : {4, 18, 19, 274, 5000, 70000})
    valid("match_" + std::to_string(n), Block().seq(rnd(40), 33, n).tail());
  for (int o : {1, 2, 3, 7, 8, 9, 63, 64, 65, 99, 100, 200})
    valid("offset_" + std::to_string(o), Block().seq(rnd(200), o, 100).seq({}, o, 3000).tail());
  valid("offset_65535", Block().seq(rnd(65535), 65535, 20).tail());
  valid("literals_only", Block().seq(rnd(1000)));
  valid("empty", Block().seq({}));
  // the staging window's edge inside a token, length bytes, an offset, a literal
  for (size_t t : {4091, 4094, 4095, 4096})
    for (size_t lit : {3, 9, 273})
      valid("window_" + std::to_string(t) + "_" + std::to_string(lit),
            Block().seq(rnd(4000), 5, 4).seq(rnd(t - 4023), 5, 4).seq(rnd(lit), 30, 8).tail());
  valid("literal_over_window", Block().seq(rnd(30), 3, 9).seq(rnd(5000), 4000, 70).seq(rnd(6), 1, 300).tail());
  // the next token at stream byte t, then a literal and a match with length
  // bytes: the window's edge in every part of a sequence in turn
  for (size_t t = 4088; t <= 4100; ++t)
    for (size_t lit : {0, 1, 3, 9, 15, 273}) {
      Block b = upto(t);
      b.seq(rnd(lit), 30, 300);
      valid("token_at_" + std::to_string(t) + "_lit" + std::to_string(lit), shorts(b, 3).tail());
    }
  // a literal that ends inside the window, on its last byte (woff + n ==
  // kWindow, the read of the slack words) and one past it (the bypass)
  for (size_t end : {4095, 4096, 4097}) {
    Block b;
    b.seq(rnd(10), 3, 4).seq(rnd(end - 30), 77, 10);  // token, 16 length bytes
    if (b.comp.size() != end + 2) std::printf("FAIL literal_ends_at_%zu layout\n", end), ++g_fail;
    valid("literal_ends_at_" + std::to_string(end), shorts(b, 6).tail());
  }
  // bypassed literals: the window restarts behind them at every residue
  for (size_t k = 0; k <= 8; ++k) {
    Block b;
    b.seq(rnd(5), 2, 4).seq(rnd(4096 + k), 100, 20);
    valid("bypass_" + std::to_string(4096 + k), shorts(b, 12).tail());
  }
  {
    Block b;
    while (b.comp.size() < 3 * 4096 + 700) shorts(b, 50);
    valid("three_refills", b.tail());
    Block e = upto(4096 - 50);
    e.seq(rnd(15 + 299 * 255 + 40), 65535, 300);  // 300 length bytes over the refill
    valid("length_bytes_300", shorts(e, 5).tail());
  }
  // one malformed block per cause
  const Bytes L = rnd(13);
  const int64_t N = 13 + 20 + 12;
  check("offset_zero", Block().seq(L, 0, 20, false).tail().comp, N, -lz4::LZ_OFFSET_ZERO, {});
  check("offset_before_block", Block().seq(L, 14, 20, false).tail().comp, N, -lz4::LZ_OFFSET_FAR, {});
  check("length_bytes_cut", {0xF0, 0xFF, 0xFF}, N, -lz4::LZ_LENGTH_PAST_INPUT, {});
  Bytes cut = Block().seq(L).comp;
  cut.pop_back();
  check("literal_cut", cut, N, -lz4::LZ_LITERAL_PAST_INPUT, {});
  check("output_overrun", Block().seq(L, 7, 30).tail().comp, N, -lz4::LZ_OUTPUT_OVERRUN, {});
  check("match_overrun", Block().seq(L, 7, 70000).tail().comp, N, -lz4::LZ_OUTPUT_OVERRUN, {});
  check("no_last_sequence", Block().seq(L, 7, 20).comp, N, -lz4::LZ_INPUT_SHORT, {});
  Bytes left = Block().seq(L, 7, 20).tail().comp;
  left.insert(left.end(), 3, 0);
  check("input_left", left, N, -lz4::LZ_INPUT_LEFT, {});
  // container blocks: three chunks, and each way the chunk walk can end
  Block a = Block().seq(rnd(5000), 100, 600).tail(), b = Block().seq(rnd(9), 2, 40).tail();
  Bytes three, all = a.out;
  for (const Block* c : {&a, &b, &a}) be32(three, c->comp.size()), three.insert(three.end(), c->comp.begin(), c->comp.end());
  all.insert(all.end(), b.out.begin(), b.out.end()), all.insert(all.end(), a.out.begin(), a.out.end());
  check("three_chunks", three, (int64_t)all.size(), (int64_t)all.size(), all, true);
  check("block_short", three, (int64_t)all.size() + 1, -lz4::LZ_BLOCK_SHORT, {}, true);
  check("block_input_left", three, (int64_t)(a.out.size() + b.out.size()), -lz4::LZ_BLOCK_INPUT_LEFT, {}, true);
  Bytes past = three;
  past[0] = 0x7F;  // the first comp_len, far more than the block has
  check("chunk_past_block", past, (int64_t)all.size(), -lz4::LZ_CHUNK_PAST_BLOCK, {}, true);
  g_long.push_back({"three_chunks", three, (int64_t)all.size(), true, {}});
  // the causes again behind a window refill and doubling rounds
  {
    auto pre = [] { return Block().seq(rnd(3000), 5, 300).seq(rnd(1500), 70, 400); };
    const int64_t P = (int64_t)pre().out.size(), M = P + N;
    check("far:offset_zero", pre().seq(L, 0, 20, false).tail().comp, M, -lz4::LZ_OFFSET_ZERO, {});
    check("far:offset_before_block", pre().seq(L, (int)P + 14, 20, false).tail().comp, M, -lz4::LZ_OFFSET_FAR, {});
    Bytes c = pre().comp;
    c.insert(c.end(), {0xF0, 0xFF, 0xFF});
    check("far:length_bytes_cut", c, M, -lz4::LZ_LENGTH_PAST_INPUT, {});
    c = pre().seq(L).comp, c.pop_back();
    check("far:literal_cut", c, M, -lz4::LZ_LITERAL_PAST_INPUT, {});
    check("far:output_overrun", pre().seq(L, 7, 30).tail().comp, M, -lz4::LZ_OUTPUT_OVERRUN, {});
    check("far:match_overrun", pre().seq(L, 7, 70000).tail().comp, M, -lz4::LZ_OUTPUT_OVERRUN, {});
    check("far:no_last_sequence", pre().seq(L, 7, 20).comp, M, -lz4::LZ_INPUT_SHORT, {});
    c = pre().seq(L, 7, 8).comp, c.pop_back();
    check("far:offset_cut", c, M, -lz4::LZ_INPUT_SHORT, {});
    c = pre().seq(L, 7, 20).tail().comp, c.insert(c.end(), 3, 0);
    check("far:input_left", c, M, -lz4::LZ_INPUT_LEFT, {});
    // chunks: one that produces nothing, a small one behind a long one (the
    // window still holds the long one's end), a header cut short, and a
    // match that reaches into the previous chunk's output
    Block big = pre().tail(), small = Block().seq(rnd(6), 2, 9).seq(rnd(3), 4, 5).tail(), none;
    none.comp.push_back(0);
    Bytes want, run = chunks({&b, &none, &a}, &want);
    check("empty_chunk_in_the_middle", run, (int64_t)want.size(), (int64_t)want.size(), want, true);
    want.clear(), run = chunks({&small, &big, &small}, &want);
    check("small_big_small", run, (int64_t)want.size(), (int64_t)want.size(), want, true);
    g_long.push_back({"small_big_small", run, (int64_t)want.size(), true, {}});
    run = chunks({&a, &b}, nullptr), run.insert(run.end(), 3, 0);
    check("chunk_header_cut", run, (int64_t)all.size(), -lz4::LZ_CHUNK_PAST_BLOCK, {}, true);
    Block reach = Block().seq(rnd(5), 6, 8, false).tail();
    check("match_into_previous_chunk", chunks({&big, &reach}, nullptr),
          (int64_t)big.out.size() + 5 + 8 + 12, -lz4::LZ_OFFSET_FAR, {}, true);
  }
  // single-byte mutants of the long valid streams: only bounds matter. They
  // are dealt round-robin, some 17 to a stream; every other round lands on a
  // raw block's header bytes (a chunk run keeps no such list: its mutants
  // fall anywhere, chunk headers included). Every third mutant gets spare
  // room, so a lengthened match is copied, not refused.
  {
    size_t runs = 0;
    for (int k = 0; k < 2000; ++k) {
      const Long& s = g_long[k % g_long.size()];
      Bytes m = s.comp;
      Bytes r = rnd(5);
      size_t at = ((size_t)r[0] << 16 | (size_t)r[1] << 8 | r[2]) % m.size();
      // every other one on a token, a length byte or an offset
      if ((k / g_long.size() & 1) && !s.hdr.empty()) at = s.hdr[at % s.hdr.size()];
      m[at] ^= (uint8_t)(r[3] | 1);
      for (int lane : {-1, 0, 63}) run(m, s.cap + (k % 3 ? 0 : 300), lane, true, s.chunked, nullptr), ++runs;
    }
    std::printf("ok   %zu mutant runs over %zu long streams\n", runs, g_long.size());
  }
  // random byte soup under every cap: only bounds matter
  for (int k = 0; k < 3000; ++k) {
    Bytes soup = rnd(1 + k % 97);
    for (int lane : {-1, 0, 63}) run(soup, k % 301, lane, lane >= 0, k & 1, nullptr);
  }
  std::printf(g_fail ? "%d case(s) FAILED\n" : "all lz4 core cases passed\n", g_fail);
  return g_fail ? 1 : 0;
}
