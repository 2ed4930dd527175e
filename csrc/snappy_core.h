// Raw-Snappy chunk decoder core, shared host/device.
//
// The gfx950 kernel (csrc/hip/snappy.hip) runs this one-chunk-per-WAVE: the
// 64 lanes walk the element stream in lockstep (every value that steers the
// walk is wave-uniform) and split each literal or copy among themselves;
// the host build (lane < 0, the lanes' share done by a loop) backs the CPU
// tests and the stand-alone sanitizer program, and gives the same bytes.
// Design notes: docs/KERNELS.md "unsnap_chunks_kernel".
//
// Format (public description, github.com/google/snappy format_description):
// a varint of the uncompressed length (at most 5 bytes for 32 bits), then
// elements, each led by a tag byte whose low two bits give the kind:
//   00 literal  upper 6 bits = len-1 for len 1..60; 60..63 = len-1 follows
//               in 1..4 little-endian bytes
//   01 copy     len 4..11 = 4 + bits 2..4; offset 11 bits = bits 5..7 << 8
//               | next byte
//   10 copy     len 1..64 = 1 + upper 6 bits; offset = next 2 bytes LE
//   11 copy     len 1..64 = 1 + upper 6 bits; offset = next 4 bytes LE
// A copy reads `offset` bytes back in the output and may overlap itself:
// offset < len repeats a period, offset 1 is a byte run.
#pragma once

#include <cstdint>
#include <cstring>

#include "crc32c.h"        // TFR_HOSTDEV
#include "inflate_core.h"  // TFR_WAVE_FENCE

namespace tfrec {
namespace snappy {

using inflate::i64;
using inflate::u32;
using inflate::u64;
using inflate::u8;

// Cause codes of unsnap_one (the low byte of the kernel's error word).
enum Cause : int {
  SN_OK = 0,
  SN_PREAMBLE_LONG = 1,      // varint unterminated within 5 bytes / the input
  SN_PREAMBLE_MISMATCH = 2,  // varint != expect_len
  SN_OFFSET_ZERO = 3,
  SN_OFFSET_FAR = 4,         // copy reaches before the chunk's first byte
  SN_OPERAND_PAST_INPUT = 5, // tag's length/offset bytes run past the input
  SN_LITERAL_PAST_INPUT = 6, // literal body runs past the input
  SN_OUTPUT_OVERRUN = 7,     // element would write past expect_len
  SN_INPUT_SHORT = 8,        // input ends before expect_len bytes exist
  SN_INPUT_LEFT = 9,         // input remains after expect_len bytes exist
};

// Up to 8 input bytes at p, little-endian, never reading past p + avail
// (avail > 0). Safe at any alignment: the chunk starts wherever the 8-byte
// container headers left it.
TFR_HOSTDEV inline u64 load_window(const u8* __restrict__ p, i64 avail) {
  u64 w = 0;
  if (avail >= 8) {
    __builtin_memcpy(&w, p, 8);
  } else {
    for (int i = 0; i < (int)avail; ++i) w |= (u64)p[i] << (8 * i);
  }
  return w;
}

// One element's header, parsed from the window at its tag byte.
struct Elem {
  u32 a;     // header bytes (1..5) | tag << 3 | (header past input) << 5
  u32 len1;  // bytes produced - 1
  u32 off;   // copy offset (0 for a literal)
};

TFR_HOSTDEV inline Elem parse_elem(u64 w, i64 avail) {
  const u32 tag = (u32)w & 3u;
  const u32 up6 = ((u32)w >> 2) & 63u;
  u32 hdr, len1 = up6, off = 0;
  if (tag == 0) {
    hdr = 1;
    if (up6 >= 60) {
      const int nb = (int)up6 - 59;  // 1..4 length bytes
      hdr = 1 + (u32)nb;
      len1 = (u32)(w >> 8) & (0xFFFFFFFFu >> (32 - 8 * nb));
    }
  } else if (tag == 1) {
    hdr = 2;
    len1 = 3 + (up6 & 7u);
    off = ((up6 >> 3) << 8) | ((u32)(w >> 8) & 0xFFu);
  } else if (tag == 2) {
    hdr = 3;
    off = (u32)(w >> 8) & 0xFFFFu;
  } else {
    hdr = 5;
    off = (u32)(w >> 8);
  }
  // a window cut short by the input's end holds zeros past it: the fields
  // above are then meaningless, and the flag says so
  return Elem{hdr | (tag << 3) | ((i64)hdr > avail ? 32u : 0u), len1, off};
}

// The lanes' share of a copy, no fence: the caller fences before the next
// read of `dst`'s buffer. Serial on host (lane < 0). src and dst must not
// overlap. Every access is inside [src, src + n) and [dst, dst + n).
TFR_HOSTDEV inline void lane_copy(u8* dst, const u8* src, i64 n, int lane,
                                  int nlanes) {
  if (lane < 0) {
    for (i64 i = 0; i < n; ++i) dst[i] = src[i];
    return;
  }
  for (i64 i = (i64)lane * 8; i + 8 <= n; i += (i64)nlanes * 8) {
    u64 w;
    __builtin_memcpy(&w, src + i, 8);
    __builtin_memcpy(dst + i, &w, 8);
  }
  const i64 tail = n & ~((i64)7);
  for (i64 b = tail + lane; b < n; b += nlanes) dst[b] = src[b];
}

// dst[0, len) = the `off` bytes before dst, repeated (off < len: the copy
// overlaps itself). Each lane takes bytes lane, lane + nlanes, ... and
// reads only from the period, which was complete before this element.
TFR_HOSTDEV inline void period_copy(u8* dst, u32 off, i64 len, int lane,
                                    int nlanes) {
  const u8* src = dst - off;
  int start = lane < 0 ? 0 : lane;
  int step = lane < 0 ? 1 : nlanes;
  for (i64 i = start; i < len; i += step) dst[i] = src[(u32)i % off];
}

// Decode one raw-Snappy chunk in[0, ilen) into out[0, expect). Returns
// SN_OK or a Cause; on any return nothing outside the two ranges has been
// read or written (on failure the output's content is unspecified).
// `lane` < 0 = host/serial; otherwise the whole wave calls this in lockstep
// on one chunk and `lane` only splits the copies.
//
// On the device every lane parses the element that would start at its byte
// of a 64-byte input window, with one load for the whole wave, and the walk
// then hops from start to start by reading the parsed headers out of the
// lanes' registers: one load per window on the serial chain, not one per
// element. The host takes the same steps one element at a time.
//
// Stores are not fenced one by one: a literal reads only the input, so the
// wave fences in front of every copy (which reads what other lanes stored)
// and nowhere else.
constexpr int kLanes = 64;

TFR_HOSTDEV inline int unsnap_one(const u8* __restrict__ in, i64 ilen,
                                  u8* __restrict__ out, i64 expect,
                                  int lane = -1) {
  // preamble
  u64 want = 0;
  i64 ip = 0;
  for (;;) {
    if (ip >= 5 || ip >= ilen) return SN_PREAMBLE_LONG;
    u32 b = in[ip];
    want |= (u64)(b & 0x7Fu) << (7 * ip);
    ++ip;
    if (!(b & 0x80u)) break;
  }
  if (expect < 0 || want != (u64)expect) return SN_PREAMBLE_MISMATCH;
  const bool window = lane >= 0;
  i64 op = 0;
  while (ip < ilen) {
    Elem mine{0, 0, 0};
    if (window) {
      const i64 av = ilen - ip - lane;
      if (av > 0) mine = parse_elem(load_window(in + ip + lane, av), av);
    }
    i64 s = 0;  // position in the window, wave-uniform
    do {
      if (op >= expect) return SN_INPUT_LEFT;
      const i64 avail = ilen - ip - s;
      Elem e;
#if defined(__HIP_DEVICE_COMPILE__)
      // what lane s parsed (the device always runs with lanes)
      e.a = (u32)__builtin_amdgcn_readlane((int)mine.a, (int)s);
      e.len1 = (u32)__builtin_amdgcn_readlane((int)mine.len1, (int)s);
      e.off = (u32)__builtin_amdgcn_readlane((int)mine.off, (int)s);
#else
      // a host "lane" (the sanitizer program's bounds runs) cannot read
      // another's registers: it parses what lane s holds, and checks its
      // own window against that when it is lane s itself
      e = parse_elem(load_window(in + ip + s, avail), avail);
      if (window && lane == s &&
          (mine.a != e.a || mine.len1 != e.len1 || mine.off != e.off))
        return -1;
#endif
      if (e.a & 32u) return SN_OPERAND_PAST_INPUT;
      const i64 hdr = e.a & 7u;
      const i64 len = (i64)e.len1 + 1;
      if (((e.a >> 3) & 3u) == 0) {
        if (len > avail - hdr) return SN_LITERAL_PAST_INPUT;
        if (len > expect - op) return SN_OUTPUT_OVERRUN;
        lane_copy(out + op, in + ip + s + hdr, len, lane, kLanes);
        s += hdr + len;
      } else {
        if (e.off == 0) return SN_OFFSET_ZERO;
        if ((i64)e.off > op) return SN_OFFSET_FAR;
        if (len > expect - op) return SN_OUTPUT_OVERRUN;
        TFR_WAVE_FENCE();  // other lanes wrote what this reads
        if ((i64)e.off >= len)
          lane_copy(out + op, out + op - e.off, len, lane, kLanes);
        else
          period_copy(out + op, e.off, len, lane, kLanes);
        s += hdr;
      }
      op += len;
    } while (window && s < 64 && ip + s < ilen);
    ip += s;
  }
  return op == expect ? SN_OK : SN_INPUT_SHORT;
}

}  // namespace snappy
}  // namespace tfrec
