// DEFLATE (RFC 1951) segment compressor core, shared host/device: the
// counterpart of inflate_core.h. One call turns one uncompressed segment
// into one raw-deflate sub-stream of the project's segmented gzip layout
// (spark_tfrecord_amd/io/paths.py compress_bytes): non-final segments end
// byte-aligned with the empty stored block 00 00 FF FF, only the last one
// carries BFINAL.
//
// The gfx950 kernel (csrc/hip/deflate.hip) runs this one-segment-per-WAVE:
// the 64 lanes find matches for a window of 64 consecutive positions at
// once against a per-wave LDS hash table, a wave-uniform walk picks the
// non-overlapping tokens, and the encoding (stored / fixed / dynamic) is
// chosen by bit cost from the token histogram. The host build (`lane` < 0)
// emulates the lanes with loops; every step is written so that the result
// does not depend on lane timing (hash inserts are a max, not a store), so
// host and device output are byte-identical — the CPU tests of the
// algorithm rest on that. Design notes: docs/KERNELS.md
// "deflate_segments_kernel".
#pragma once

#include <cstdint>
#include <cstring>

#include "crc32c.h"        // TFR_HOSTDEV
#include "inflate_core.h"  // RFC 1951 tables, bulk_copy, TFR_WAVE_FENCE

// Lanes of one wave exchange data through LDS between the steps below: all
// pending LDS/global accesses complete, and the compiler moves nothing
// across (no-op on host, where the "lanes" are loop iterations).
#if defined(__HIP_DEVICE_COMPILE__)
#define TFR_WAVE_SYNC()              \
  do {                               \
    TFR_WAVE_FENCE();                \
    __builtin_amdgcn_wave_barrier(); \
  } while (0)
#else
#define TFR_WAVE_SYNC() ((void)0)
#endif

// for (i over this lane's share of [0, count)): every i on host, i = lane,
// lane + 64, ... on device.
#define TFR_LANE_LOOP(i, lane, count)                      \
  for (int i = ((lane) < 0 ? 0 : (lane)); i < (count);     \
       i += ((lane) < 0 ? 1 : ::tfrec::deflate::kWin))

namespace tfrec {
namespace deflate {

using inflate::i64;
using inflate::u32;
using inflate::u64;
using inflate::u8;
using u16 = uint16_t;

constexpr int kWin = 64;  // positions matched per step == wave width
constexpr int kHashBits = 12;
constexpr int kHashSize = 1 << kHashBits;
constexpr int kMinMatch = 3;
constexpr int kMaxMatch = 258;
constexpr int kMaxDist = 32768;
constexpr int kTooFar = 4096;  // a 3-byte match further back costs more
                               // than its literals (zlib's TOO_FAR)
constexpr i64 kStoredMax = 65535;
constexpr u32 kTokMatch = 0x80000000u;  // | (len-3) << 16 | (dist-1)

// Worst case of one segment of u input bytes: all stored blocks plus the
// full-flush marker. The caller gives each segment this much room.
TFR_HOSTDEV inline i64 seg_out_bound(i64 u) {
  return u + 5 * ((u + kStoredMax - 1) / kStoredMax) + 5;
}

struct LenCodeTab {
  u8 c[256];  // match length - 3 -> length code (symbol - 257)
};

constexpr LenCodeTab make_len_code_tab() {
  LenCodeTab t{};
  for (int l = 0; l < 256; ++l) {
    int len = l + 3, c = 0;
    for (int k = 0; k < 29; ++k)
      if (inflate::kLenBase[k] <= len) c = k;
    t.c[l] = (u8)c;
  }
  return t;
}

inline constexpr LenCodeTab kLenCode = make_len_code_tab();

TFR_HOSTDEV inline u32 dist_code(u32 dist) {  // 1..32768 -> 0..29
  u32 d = dist - 1;
  if (d < 4) return d;
  u32 msb = 31u - (u32)__builtin_clz(d);
  return 2 * msb + ((d >> (msb - 1)) & 1u);
}

TFR_HOSTDEV inline u32 fixed_lit_len(int s) {
  return s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8));
}

// Huffman-build workspace; overlays the hash table, which is dead once the
// segment is parsed.
struct HuffWs {
  u32 w[576];       // node weights, then node depths
  u16 parent[576];
  u16 order[288];   // used symbols, ascending (freq, symbol)
  u32 cnt[16];      // codes per length
};

// Per-wave state: LDS on the device, stack on the host.
struct Scratch {
  union {
    u32 hash[kHashSize];  // position + 1 of the latest insert, 0 = empty
    HuffWs hw;
  };
  u32 lit_freq[288];
  u32 dist_freq[32];
  u32 cl_freq[19];
  u16 lit_code[288];  // bit-reversed: ready for the LSB-first writer
  u16 dist_code[32];
  u16 cl_code[19];
  u8 lit_len[288];
  u8 dist_len[32];
  u8 cl_len[19];
  // one window of per-lane match results
  u16 wlen[kWin];   // 0 = no match
  u16 wdist[kWin];  // dist - 1
  u16 whash[kWin];  // 0xFFFF = position has no 3 bytes to hash
  u8 wlit[kWin];
  // one batch of per-lane encoded tokens
  u64 ebits[kWin];
  u8 enb[kWin];
  // lane 0 -> wave broadcasts
  i64 r_len;
  int r_mode;
};

TFR_HOSTDEV inline void hash_insert_max(u32* slot, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  // several lanes can hit one bucket in the same step: the highest
  // position wins whatever the order the hardware serves them in
  __hip_atomic_fetch_max(slot, v, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_WORKGROUP);
#else
  if (v > *slot) *slot = v;
#endif
}

TFR_HOSTDEV inline u32 match_len(const u8* a, const u8* b, u32 maxl) {
  u32 i = 0;
  while (i + 8 <= maxl) {
    u64 x, y;
    __builtin_memcpy(&x, a + i, 8);
    __builtin_memcpy(&y, b + i, 8);
    if (x != y) return i + ((u32)__builtin_ctzll(x ^ y) >> 3);
    i += 8;
  }
  while (i < maxl && a[i] == b[i]) ++i;
  return i;
}

// Length-limited Huffman code lengths for freq[0, nsym), nsym <= 288:
// used symbols get 1..max_len, unused ones 0; the Kraft sum is exactly 1
// when two or more symbols are used (a single used symbol gets length 1).
// The (freq, symbol) rank sort is spread over the lanes; the two-queue
// merge and the Kraft fix-up run on one lane — ~300 symbols is small next
// to the matching of a whole segment.
TFR_HOSTDEV inline void build_lengths(const u32* freq, int nsym, int max_len,
                                      u8* len_out, HuffWs& W, int lane) {
  int m = 0;
  for (int s = 0; s < nsym; ++s) m += freq[s] != 0;
  TFR_LANE_LOOP(s, lane, nsym) {
    u32 f = freq[s];
    len_out[s] = 0;
    if (!f) continue;
    int r = 0;
    for (int t = 0; t < nsym; ++t) {
      u32 ft = freq[t];
      r += (ft != 0 && (ft < f || (ft == f && t < s))) ? 1 : 0;
    }
    W.order[r] = (u16)s;
  }
  TFR_WAVE_SYNC();
  if (lane <= 0 && m == 1) len_out[W.order[0]] = 1;
  if (lane <= 0 && m >= 2) {
    for (int k = 0; k < m; ++k) W.w[k] = freq[W.order[k]];
    // leaves are sorted and internal nodes come out in nondecreasing
    // weight, so the two lightest nodes are always at the two queue heads
    int li = 0, ni = m;
    for (int nn = m; nn < 2 * m - 1; ++nn) {
      int a, b;
      if (li < m && (ni >= nn || W.w[li] <= W.w[ni])) a = li++;
      else a = ni++;
      if (li < m && (ni >= nn || W.w[li] <= W.w[ni])) b = li++;
      else b = ni++;
      W.w[nn] = W.w[a] + W.w[b];
      W.parent[a] = (u16)nn;
      W.parent[b] = (u16)nn;
    }
    W.w[2 * m - 2] = 0;  // weights are spent: reuse as depths
    for (int k = 2 * m - 3; k >= 0; --k) W.w[k] = W.w[W.parent[k]] + 1;
    for (int l = 0; l < 16; ++l) W.cnt[l] = 0;
    for (int k = 0; k < m; ++k) {
      u32 d = W.w[k];
      ++W.cnt[d > (u32)max_len ? (u32)max_len : d];
    }
    // Kraft fix-up: clamping over-long codes over-subscribes the code
    // space by `total - 2^max_len` units of 2^-max_len. Each round gives
    // one unit back: drop a code from the longest length, and split the
    // deepest shorter code into two of the next length.
    u32 total = 0;
    for (int l = 1; l <= max_len; ++l) total += W.cnt[l] << (max_len - l);
    while (total > (1u << max_len)) {
      --W.cnt[max_len];
      for (int l = max_len - 1; l > 0; --l) {
        if (W.cnt[l]) {
          --W.cnt[l];
          W.cnt[l + 1] += 2;
          break;
        }
      }
      --total;
    }
    int j = m;  // the most frequent symbols take the shortest codes
    for (int l = 1; l <= max_len; ++l)
      for (u32 c = W.cnt[l]; c > 0; --c) len_out[W.order[--j]] = (u8)l;
  }
  TFR_WAVE_SYNC();
}

// Canonical codes from lengths, bit-reversed for the LSB-first writer.
TFR_HOSTDEV inline void assign_codes(const u8* len, int nsym, u16* code) {
  u32 cnt[16], next[16];
  for (int l = 0; l < 16; ++l) cnt[l] = 0;
  for (int s = 0; s < nsym; ++s) ++cnt[len[s]];
  cnt[0] = 0;
  u32 c = 0;
  next[0] = 0;
  for (int l = 1; l < 16; ++l) {
    c = (c + cnt[l - 1]) << 1;
    next[l] = c;
  }
  for (int s = 0; s < nsym; ++s) {
    u32 l = len[s];
    code[s] = l ? (u16)(__builtin_bitreverse32(next[l]++) >> (32 - l)) : 0;
  }
}

struct BitWr {
  u8* out;
  i64 o;
  i64 cap;
  u64 bb;
  int bn;     // < 8 between calls
  bool over;  // a write would have passed cap (nothing was written there)
};

TFR_HOSTDEV inline void bw_put(BitWr& b, u64 bits, int nb) {  // nb <= 48
  b.bb |= bits << b.bn;
  b.bn += nb;
  int k = b.bn >> 3;
  if (!k) return;
  if (b.o + 8 <= b.cap) {
    // bytes past k are rewritten by the next put, or lie beyond the
    // stream inside this segment's own slot
    __builtin_memcpy(b.out + b.o, &b.bb, 8);
  } else if (b.o + k <= b.cap) {
    for (int i = 0; i < k; ++i) b.out[b.o + i] = (u8)(b.bb >> (8 * i));
  } else {
    b.over = true;
  }
  b.o += k;
  b.bb = (k >= 8) ? 0 : (b.bb >> (8 * k));
  b.bn &= 7;
}

TFR_HOSTDEV inline void bw_align(BitWr& b) {
  if (b.bn) bw_put(b, 0, 8 - b.bn);
}

// Run-length coding of the hlit + hdist code lengths with the code-length
// alphabet (16 = repeat previous 3-6, 17 = zeros 3-10, 18 = zeros 11-138);
// sink(symbol, extra_bits, extra_value) sees every emitted symbol. Runs may
// cross from the literal/length lengths into the distance lengths.
template <class Sink>
TFR_HOSTDEV inline void cl_rle(const Scratch& S, int hlit, int hdist,
                               Sink sink) {
  int total = hlit + hdist;
  auto L = [&](int i) -> int {
    return i < hlit ? S.lit_len[i] : S.dist_len[i - hlit];
  };
  int i = 0;
  while (i < total) {
    int v = L(i);
    int run = 1;
    while (i + run < total && L(i + run) == v) ++run;
    i += run;
    if (v == 0) {
      while (run >= 11) {
        int t = run > 138 ? 138 : run;
        sink(18, 7, t - 11);
        run -= t;
      }
      if (run >= 3) {
        sink(17, 3, run - 3);
        run = 0;
      }
      while (run-- > 0) sink(0, 0, 0);
    } else {
      sink(v, 0, 0);
      --run;
      while (run >= 3) {
        int t = run > 6 ? 6 : run;
        sink(16, 2, t - 3);
        run -= t;
      }
      while (run-- > 0) sink(v, 0, 0);
    }
  }
}

enum Mode { kStored = 0, kFixed = 1, kDynamic = 2 };

TFR_HOSTDEV inline i64 stored_len(i64 n, bool final) {
  if (n == 0) return 5;  // one empty block: the final one, or the marker
  return n + 5 * ((n + kStoredMax - 1) / kStoredMax) + (final ? 0 : 5);
}

// Stored encoding: <= 65535 bytes per block, lanes split the copies.
TFR_HOSTDEV inline i64 emit_stored(const u8* __restrict__ in, i64 n,
                                   u8* __restrict__ out, bool final,
                                   int lane) {
  i64 o = 0, p = 0;
  if (n > 0 || final) {
    do {
      i64 blk = n - p < kStoredMax ? n - p : kStoredMax;
      bool last = p + blk == n;
      if (lane <= 0) {
        out[o] = (final && last) ? 1 : 0;
        out[o + 1] = (u8)blk;
        out[o + 2] = (u8)(blk >> 8);
        out[o + 3] = (u8)~blk;
        out[o + 4] = (u8)(~blk >> 8);
      }
      inflate::bulk_copy(out + o + 5, in + p, blk, lane, kWin);
      o += 5 + blk;
      p += blk;
    } while (p < n);
  }
  if (!final) {
    if (lane <= 0) {
      out[o] = 0;
      out[o + 1] = 0;
      out[o + 2] = 0;
      out[o + 3] = 0xFF;
      out[o + 4] = 0xFF;
    }
    o += 5;
  }
  return o;
}

// Compress in[0, n) into out[0, cap), cap >= seg_out_bound(n); returns the
// stream length, or -1 on an internal inconsistency (never expected; the
// caller reports it). `toks` holds n entries. `stored_threshold` keeps
// TFREC_GZ_STORED_THRESHOLD's meaning: a segment whose best Huffman
// encoding is >= threshold * n goes stored (<= 0 disables); apart from
// that the cheapest of stored / fixed / dynamic wins, so no segment ever
// exceeds its stored encoding, which always fits the bound.
// `lane` < 0 = host/serial; otherwise the whole wave runs this in lockstep
// on one segment.
TFR_HOSTDEV inline i64 deflate_one(const u8* __restrict__ in, i64 n,
                                   u8* __restrict__ out, i64 cap, bool final,
                                   double stored_threshold,
                                   u32* __restrict__ toks, Scratch& S,
                                   int lane = -1) {
  TFR_LANE_LOOP(i0, lane, kHashSize) S.hash[i0] = 0;
  TFR_LANE_LOOP(i1, lane, 320) {
    if (i1 < 288) {
      S.lit_freq[i1] = 0;
      S.lit_len[i1] = 0;  // symbols 286/287 and 30/31 never get a length
    } else {
      S.dist_freq[i1 - 288] = 0;
      S.dist_len[i1 - 288] = 0;
    }
  }
  TFR_WAVE_SYNC();

  // ---- LZ77: 64 positions per step --------------------------------------
  i64 ntok = 0;
  u64 xbits = 0;  // extra bits of all match tokens
  i64 base = 0;
  while (base < n) {
    TFR_LANE_LOOP(i, lane, kWin) {
      i64 p = base + i;
      u32 len = 0, dist = 0, h = 0xFFFFu;
      if (p < n) S.wlit[i] = in[p];
      if (p + kMinMatch <= n) {
        u32 v = (u32)in[p] | ((u32)in[p + 1] << 8) | ((u32)in[p + 2] << 16);
        h = (v * 0x9E3779B1u) >> (32 - kHashBits);
        // the table holds positions of EARLIER windows only (this
        // window's inserts come after every lane has looked up)
        u32 e = S.hash[h];
        if (e) {
          i64 c = (i64)e - 1;
          i64 d = p - c;
          if (d <= kMaxDist) {
            u32 maxl = (u32)(n - p < kMaxMatch ? n - p : kMaxMatch);
            u32 l = match_len(in + c, in + p, maxl);
            if (l >= (u32)kMinMatch && !(l == (u32)kMinMatch && d > kTooFar)) {
              len = l;
              dist = (u32)d;
            }
          }
        }
      }
      S.wlen[i] = (u16)len;
      S.wdist[i] = (u16)(dist - 1);
      S.whash[i] = (u16)h;
    }
    TFR_WAVE_SYNC();
    TFR_LANE_LOOP(i, lane, kWin) {
      u32 h = S.whash[i];
      if (h != 0xFFFFu) hash_insert_max(&S.hash[h], (u32)(base + i) + 1u);
    }
    // wave-uniform walk: greedy, non-overlapping; a match may run past
    // the window, the next window starts where the walk ends (>= 1 byte
    // of progress per token, >= 1 token per window)
    i64 pos = base;
    i64 wend = base + kWin < n ? base + kWin : n;
    while (pos < wend) {
      int i = (int)(pos - base);
      u32 l = S.wlen[i];
      u32 tok;
      if (l) {
        u32 d1 = S.wdist[i];
        tok = kTokMatch | ((l - 3) << 16) | d1;
        u32 lc = kLenCode.c[l - 3];
        u32 dc = dist_code(d1 + 1);
        xbits += inflate::kLenExtra[lc] + inflate::kDistExtra[dc];
        if (lane <= 0) {
          ++S.lit_freq[257 + lc];
          ++S.dist_freq[dc];
        }
        pos += l;
      } else {
        tok = S.wlit[i];
        if (lane <= 0) ++S.lit_freq[tok];
        pos += 1;
      }
      if (lane <= 0) toks[ntok] = tok;
      ++ntok;
    }
    base = pos;
    TFR_WAVE_SYNC();
  }
  if (lane <= 0) S.lit_freq[256] = 1;  // end of block
  TFR_WAVE_SYNC();

  // ---- encoding choice by bit cost ---------------------------------------
  build_lengths(S.lit_freq, 286, 15, S.lit_len, S.hw, lane);
  build_lengths(S.dist_freq, 30, 15, S.dist_len, S.hw, lane);
  int hlit = 286, hdist = 30;
  while (hlit > 257 && S.lit_len[hlit - 1] == 0) --hlit;
  while (hdist > 1 && S.dist_len[hdist - 1] == 0) --hdist;
  TFR_LANE_LOOP(i2, lane, kWin)
    if (i2 < 19) S.cl_freq[i2] = 0;
  TFR_WAVE_SYNC();
  u64 cl_xbits = 0;
  cl_rle(S, hlit, hdist, [&](int s, int eb, int) {
    if (lane <= 0) ++S.cl_freq[s];
    cl_xbits += (u64)eb;
  });
  TFR_WAVE_SYNC();
  build_lengths(S.cl_freq, 19, 7, S.cl_len, S.hw, lane);
  const i64 stored_total = stored_len(n, final);
  if (lane <= 0) {
    // zlib rejects an incomplete code-length code: a lone symbol gets a
    // never-used sibling
    int used = 0, only = 0;
    for (int s = 0; s < 19; ++s)
      if (S.cl_len[s]) {
        ++used;
        only = s;
      }
    if (used == 1) S.cl_len[only == 0 ? 1 : 0] = 1;
    int hclen = 19;
    while (hclen > 4 && S.cl_len[inflate::kClOrder[hclen - 1]] == 0) --hclen;
    u64 fixed_bits = 3 + xbits, dyn_bits = 3 + 14 + 3 * (u64)hclen + cl_xbits +
                                           xbits;
    for (int s = 0; s < 286; ++s) {
      fixed_bits += (u64)S.lit_freq[s] * fixed_lit_len(s);
      dyn_bits += (u64)S.lit_freq[s] * S.lit_len[s];
    }
    for (int s = 0; s < 30; ++s) {
      fixed_bits += (u64)S.dist_freq[s] * 5;
      dyn_bits += (u64)S.dist_freq[s] * S.dist_len[s];
    }
    for (int s = 0; s < 19; ++s) dyn_bits += (u64)S.cl_freq[s] * S.cl_len[s];
    int mode = (n > 0 && dyn_bits < fixed_bits) ? kDynamic : kFixed;
    u64 bits = mode == kDynamic ? dyn_bits : fixed_bits;
    i64 huff_total = final ? (i64)((bits + 7) >> 3)
                           : (i64)((bits + 3 + 7) >> 3) + 4;
    if (huff_total >= stored_total || huff_total > cap ||
        (stored_threshold > 0 && n > 0 &&
         (double)huff_total >= stored_threshold * (double)n))
      mode = kStored;
    if (mode == kFixed) {
      for (int s = 0; s < 288; ++s) S.lit_len[s] = (u8)fixed_lit_len(s);
      for (int s = 0; s < 32; ++s) S.dist_len[s] = 5;
    }
    if (mode != kStored) {
      assign_codes(S.lit_len, 288, S.lit_code);
      assign_codes(S.dist_len, 32, S.dist_code);
      assign_codes(S.cl_len, 19, S.cl_code);
    }
    S.r_mode = mode;
    S.r_len = mode == kStored ? stored_total : huff_total;
  }
  TFR_WAVE_SYNC();
  const int mode = S.r_mode;
  const i64 want = S.r_len;
  if (mode == kStored) {
    if (stored_total > cap) return -1;
    return emit_stored(in, n, out, final, lane);
  }

  // ---- one Huffman block: lanes encode tokens, lane 0 concatenates --------
  BitWr bw{out, 0, cap, 0, 0, false};
  if (lane <= 0) {
    bw_put(bw, (final ? 1u : 0u) | ((u32)mode << 1), 3);
    if (mode == kDynamic) {
      int hclen = 19;
      while (hclen > 4 && S.cl_len[inflate::kClOrder[hclen - 1]] == 0) --hclen;
      bw_put(bw, (u64)(hlit - 257) | ((u64)(hdist - 1) << 5) |
                     ((u64)(hclen - 4) << 10), 14);
      for (int k = 0; k < hclen; ++k)
        bw_put(bw, S.cl_len[inflate::kClOrder[k]], 3);
      cl_rle(S, hlit, hdist, [&](int s, int eb, int ev) {
        bw_put(bw, (u64)S.cl_code[s] | ((u64)ev << S.cl_len[s]),
               S.cl_len[s] + eb);
      });
    }
  }
  for (i64 t0 = 0; t0 < ntok; t0 += kWin) {
    int cnt = (int)(ntok - t0 < kWin ? ntok - t0 : kWin);
    TFR_LANE_LOOP(i, lane, cnt) {
      u32 tok = toks[t0 + i];
      u64 bits;
      int nb;
      if (tok & kTokMatch) {
        u32 l3 = (tok >> 16) & 0xFFu;
        u32 dist = (tok & 0x7FFFu) + 1;
        u32 lc = kLenCode.c[l3];
        u32 dc = dist_code(dist);
        bits = S.lit_code[257 + lc];
        nb = S.lit_len[257 + lc];
        bits |= (u64)(l3 + 3 - inflate::kLenBase[lc]) << nb;
        nb += inflate::kLenExtra[lc];
        bits |= (u64)S.dist_code[dc] << nb;
        nb += S.dist_len[dc];
        bits |= (u64)(dist - inflate::kDistBase[dc]) << nb;
        nb += inflate::kDistExtra[dc];
      } else {
        bits = S.lit_code[tok];
        nb = S.lit_len[tok];
      }
      S.ebits[i] = bits;
      S.enb[i] = (u8)nb;
    }
    TFR_WAVE_SYNC();
    if (lane <= 0)
      for (int i = 0; i < cnt; ++i) bw_put(bw, S.ebits[i], S.enb[i]);
    TFR_WAVE_SYNC();
  }
  if (lane <= 0) {
    bw_put(bw, S.lit_code[256], S.lit_len[256]);
    if (!final) {
      bw_put(bw, 0, 3);  // empty stored block: the full-flush marker
      bw_align(bw);
      bw_put(bw, 0xFFFF0000u, 32);
    } else {
      bw_align(bw);
    }
    S.r_len = (bw.over || bw.o != want) ? -1 : bw.o;
  }
  TFR_WAVE_SYNC();
  return S.r_len;
}

}  // namespace deflate
}  // namespace tfrec
