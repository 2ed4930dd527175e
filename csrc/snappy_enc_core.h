// Raw-Snappy chunk compressor core, shared host/device: the counterpart of
// snappy_core.h. One call turns one uncompressed block into one raw-Snappy
// chunk (varint of the length, then literal and copy elements; the format
// is described at the top of snappy_core.h).
//
// The gfx950 kernel (csrc/hip/snappy_enc.hip) runs this one-block-per-WAVE
// with the matcher of deflate_core.h: the 64 lanes look up 64 consecutive
// positions at once in a per-wave LDS hash table that holds earlier windows
// only, this window's positions go in after a wave sync through
// hash_insert_max, and a wave-uniform greedy walk takes the non-overlapping
// matches. Snappy has no entropy stage, so the walk emits the elements as it
// goes: lane 0 writes the few header bytes, the lanes share each literal's
// body. The host build (`lane` < 0) emulates the lanes with loops; nothing
// depends on lane timing, so host and device output are byte-identical and
// the CPU tests of the algorithm rest on that. Design notes: docs/KERNELS.md
// "snap_blocks_kernel".
#pragma once

#include <cstdint>
#include <cstring>

#include "crc32c.h"        // TFR_HOSTDEV
#include "deflate_core.h"  // hash_insert_max, match_len, TFR_WAVE_SYNC
#include "snappy_core.h"   // lane_copy

namespace tfrec {
namespace snappy {

using u16 = uint16_t;

constexpr int kEncWin = deflate::kWin;  // positions matched per step
constexpr int kEncHashBits = 12;
constexpr int kEncHashSize = 1 << kEncHashBits;
constexpr u32 kEncMinMatch = 4;
// A match further back than this would need a tag-3 copy (5 bytes for what
// is usually a short match); the encoder emits tags 1 and 2 only.
constexpr i64 kEncMaxDist = 65535;
// Longest match one lane extends: 16 full copy elements. Every lane of a
// window extends its own candidate at the same time, so a window costs as
// much as its longest extension (128 eight-byte compares at this bound),
// and the walk may then skip over it. Without a bound one lane would walk
// a run of one byte value to the block's end while 63 wait; with it such a
// run still moves 1024 bytes per window, and the next window finds its
// continuation through the table. A multiple of 64 splits into whole
// elements.
constexpr u32 kEncMaxMatch = 1024;

// Room for the elements of an n-byte block before the fallback: the
// library's bound. The walk's worst case is a 4-byte match as a 3-byte
// tag-2 copy (one byte saved) followed by a literal of 61..64 bytes (two
// header bytes): at most one byte more per 65 of input, far inside n/6.
TFR_HOSTDEV inline i64 snap_out_bound(i64 n) { return 32 + n + n / 6; }

// Per-wave state: LDS on the device, heap on the host.
struct EncScratch {
  u32 hash[kEncHashSize];  // position + 1 of the latest insert, 0 = empty
  // one window of per-lane match results
  u16 wlen[kEncWin];   // 0 = no match
  u16 woff[kEncWin];
  u16 whash[kEncWin];  // 0xFFFF = position has no 4 bytes to hash
  // length of the elements before the fallback, -1 when they passed `cap`
  // (written by lane 0 for the bound check of the self-test)
  i64 emitted;
};

TFR_HOSTDEV inline int varint_len(u64 n) {
  int k = 1;
  while (n >= 0x80) {
    n >>= 7;
    ++k;
  }
  return k;
}

// Header bytes of a literal of len >= 1 in its minimal form.
TFR_HOSTDEV inline int lit_hdr_len(i64 len) {
  u64 n1 = (u64)len - 1;
  return n1 < 60 ? 1 : (n1 < 256 ? 2 : (n1 < 65536 ? 3 : (n1 < (1u << 24) ? 4 : 5)));
}

// The whole block as one literal: what no chunk ever exceeds.
TFR_HOSTDEV inline i64 one_literal_len(i64 n) {
  return n > 0 ? varint_len((u64)n) + lit_hdr_len(n) + n : 1;
}

// Bytes of the copy elements for a match of len >= 4 (split rule below).
TFR_HOSTDEV inline i64 copy_bytes(u32 len, u32 off) {
  i64 b = 0;
  while (len >= 68) {
    b += 3;
    len -= 64;
  }
  if (len > 64) {
    b += 3;
    len -= 60;
  }
  return b + ((len <= 11 && off < 2048) ? 2 : 3);
}

// One copy element of 4..64 bytes (tag 1 takes 4..11 at offsets below
// 2048); lane 0 writes it. Returns the element's length.
TFR_HOSTDEV inline i64 put_copy(u8* out, u32 len, u32 off, int lane) {
  const bool tag1 = len <= 11 && off < 2048;
  if (lane <= 0) {
    if (tag1) {
      out[0] = (u8)(1u | ((len - 4) << 2) | ((off >> 8) << 5));
      out[1] = (u8)off;
    } else {
      out[0] = (u8)(2u | ((len - 1) << 2));
      out[1] = (u8)off;
      out[2] = (u8)(off >> 8);
    }
  }
  return tag1 ? 2 : 3;
}

// Literal element for in[0, len), len >= 1, at out: lane 0 writes the
// header, the lanes share the body. Returns the element's length.
TFR_HOSTDEV inline i64 put_literal(u8* __restrict__ out,
                                   const u8* __restrict__ in, i64 len,
                                   int lane) {
  const int hdr = lit_hdr_len(len);
  if (lane <= 0) {
    const u64 n1 = (u64)len - 1;
    if (hdr == 1) {
      out[0] = (u8)(n1 << 2);
    } else {
      out[0] = (u8)((59 + (hdr - 1)) << 2);
      for (int i = 0; i + 1 < hdr; ++i) out[1 + i] = (u8)(n1 >> (8 * i));
    }
  }
  lane_copy(out + hdr, in, len, lane, kLanes);
  return hdr + len;
}

// Compress in[0, n) into out[0, cap) as one raw-Snappy chunk; returns its
// length, or -1 when cap is below one_literal_len(n). A cap of
// snap_out_bound(n) never cuts the elements short; a smaller one only makes
// the block a single literal sooner, the chunk stays valid. No chunk is
// longer than one_literal_len(n) <= n + 10. Every access is inside
// [in, in + n) and [out, out + cap); the output is never read.
// `lane` < 0 = host/serial; otherwise the whole wave runs this in lockstep
// on one block.
TFR_HOSTDEV inline i64 snap_one(const u8* __restrict__ in, i64 n,
                                u8* __restrict__ out, i64 cap, EncScratch& S,
                                int lane = -1) {
  const i64 lit_total = one_literal_len(n);
  if (n < 0 || cap < lit_total) return -1;
  const int pre = varint_len((u64)n);
  if (lane <= 0)
    for (int k = 0; k < pre; ++k)
      out[k] = (u8)((((u64)n >> (7 * k)) & 0x7Fu) | (k + 1 < pre ? 0x80u : 0u));
  if (n == 0) return pre;

  TFR_LANE_LOOP(i0, lane, kEncHashSize) S.hash[i0] = 0;
  TFR_WAVE_SYNC();

  // everything below that steers the walk is wave-uniform
  i64 o = pre;        // bytes emitted
  i64 lit_start = 0;  // first byte not yet covered by an element
  bool over = false;  // an element would have passed cap (nothing written)
  bool copied = false;
  i64 base = 0;
  while (base < n && !over) {
    u64 m = 0;  // bit i: position base + i starts a match
    TFR_LANE_LOOP(i, lane, kEncWin) {
      const i64 p = base + i;
      u32 len = 0, off = 0, h = 0xFFFFu;
      if (p + (i64)kEncMinMatch <= n) {
        u32 v;
        __builtin_memcpy(&v, in + p, 4);
        h = (v * 0x9E3779B1u) >> (32 - kEncHashBits);
        // the table holds positions of EARLIER windows only (this
        // window's inserts come after every lane has looked up)
        const u32 e = S.hash[h];
        if (e) {
          const i64 c = (i64)e - 1;
          const i64 d = p - c;
          if (d <= kEncMaxDist) {
            const u32 maxl =
                (u32)(n - p < (i64)kEncMaxMatch ? n - p : (i64)kEncMaxMatch);
            const u32 l = deflate::match_len(in + c, in + p, maxl);
            if (l >= kEncMinMatch) {
              len = l;
              off = (u32)d;
            }
          }
        }
      }
      S.wlen[i] = (u16)len;
      S.woff[i] = (u16)off;
      S.whash[i] = (u16)h;
      if (len) m |= 1ull << i;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    m = __builtin_amdgcn_ballot_w64(m != 0);  // each lane held its own bit
#endif
    TFR_WAVE_SYNC();
    TFR_LANE_LOOP(i, lane, kEncWin) {
      const u32 h = S.whash[i];
      if (h != 0xFFFFu) deflate::hash_insert_max(&S.hash[h], (u32)(base + i) + 1u);
    }
    // wave-uniform walk: greedy, non-overlapping. Positions without a
    // match join the pending literal; a match may run past the window, the
    // next window starts where the walk ends.
    const i64 wend = base + kEncWin < n ? base + kEncWin : n;
    i64 pos = base;
    while (pos < wend) {
      const u64 left = m >> (int)(pos - base);
      if (!left) {
        pos = wend;
        break;
      }
      pos += __builtin_ctzll(left);
      const int i = (int)(pos - base);
      u32 l = S.wlen[i];
      const u32 off = S.woff[i];
      const i64 lit = pos - lit_start;
      const i64 need = (lit ? lit_hdr_len(lit) + lit : 0) + copy_bytes(l, off);
      if (need > cap - o) {
        over = true;
        break;
      }
      if (lit) o += put_literal(out + o, in + lit_start, lit, lane);
      pos += l;
      lit_start = pos;
      copied = true;
      // elements of at most 64 bytes, no remainder under 4
      while (l) {
        const u32 t = l >= 68 ? 64 : (l > 64 ? 60 : l);
        o += put_copy(out + o, t, off, lane);
        l -= t;
      }
    }
    base = pos;
    TFR_WAVE_SYNC();
  }
  if (!over && lit_start < n) {
    const i64 lit = n - lit_start;
    if (lit_hdr_len(lit) + lit > cap - o)
      over = true;
    else
      o += put_literal(out + o, in + lit_start, lit, lane);
  }
  if (lane <= 0) S.emitted = over ? -1 : o;
  // Fallback: elements that are no shorter than the block as one literal
  // give way to that literal (a block without a single copy already is it).
  if (over || (copied && o >= lit_total)) {
    TFR_WAVE_FENCE();  // the literal goes over what other lanes stored
    o = pre + put_literal(out + pre, in, n, lane);
  }
  return o;
}

}  // namespace snappy
}  // namespace tfrec
