// Raw LZ4 block decoder core, shared host/device, and the walk over the
// chunks of one Hadoop container block.
//
// The gfx950 kernel (csrc/hip/lz4.hip) runs this one-container-block-per-
// WAVE: the 64 lanes walk the sequences in lockstep (every value that steers
// the walk is wave-uniform) and split each literal or match among
// themselves; the host build (lane < 0, the lanes' share done by loops)
// backs the CPU engine's `.lz4` reads, the CPU tests and the stand-alone
// sanitizer program, and gives the same bytes.
// Design notes: docs/KERNELS.md "unlz4_blocks_kernel".
//
// Format (public description, "LZ4 Block Format", lz4/doc in the LZ4
// sources): a block is a run of sequences. A sequence is
//   token        high nibble = literal length, low nibble = match length - 4
//   [255 255 .. b]  when the literal nibble is 15: bytes added to the length
//                   until one is below 255
//   literals
//   offset       2 bytes little-endian, 1..65535, back from the output end
//   [255 255 .. b]  when the match nibble is 15: the same for the match
// and the last sequence ends after its literals. A match may overlap
// itself: offset < length repeats a period, offset 1 is a byte run. The
// block does not state its own uncompressed length.
//
// The format's end-of-block rules for ENCODERS (the last 5 bytes are
// literals, the last match starts at least 12 bytes before the end) are NOT
// enforced here: any block that decodes within its bounds is taken.
#pragma once

#include <cstdint>
#include <cstring>

#include "snappy_core.h"  // lane_copy, period_copy, kLanes, TFR_WAVE_FENCE

namespace tfrec {
namespace lz4 {

using snappy::i64;
using snappy::kLanes;
using snappy::u32;
using snappy::u64;
using snappy::u8;

// Cause codes: unlz4_block returns -cause, unlz4_container_block the cause
// (the low byte of the kernel's error word).
enum Cause : int {
  LZ_OK = 0,
  LZ_OFFSET_ZERO = 1,
  LZ_OFFSET_FAR = 2,          // match reaches before the block's first byte
  LZ_LENGTH_PAST_INPUT = 3,   // length-extension bytes run past the input
  LZ_LITERAL_PAST_INPUT = 4,  // literal run past the input
  LZ_OUTPUT_OVERRUN = 5,      // sequence would write past `cap`
  LZ_INPUT_SHORT = 6,         // input ends inside a sequence: no final
                              // literals-only sequence
  LZ_INPUT_LEFT = 7,          // input left after the sequence that filled
                              // the output
  // the container block's chunk walk
  LZ_CHUNK_PAST_BLOCK = 8,    // chunk header or body runs past the block
  LZ_BLOCK_SHORT = 9,         // chunks end before raw_len bytes exist
  LZ_BLOCK_INPUT_LEFT = 10,   // chunks left after raw_len bytes exist
};

// The input window a wave stages in LDS. The shifted word reads of
// window_copy may touch the 8 bytes behind the window, never use them.
constexpr i64 kWindow = 4096;
constexpr i64 kWindowAlloc = kWindow + 8;

// Where the walk reads its header bytes (token, length bytes, offset).
// Without `win` it reads the input in place (the serial host decoder); with
// it, in[base, base + len) stands in win[0, len) and a read outside that
// restarts the window at the byte asked for. All fields but `lane` are
// wave-uniform.
struct Window {
  const u8* in;
  i64 ilen;
  u8* win;  // 8-byte aligned, kWindowAlloc bytes
  i64 base, len;
  int lane;
};

TFR_HOSTDEV inline void fill(Window& W, i64 pos) {
  W.base = pos;
  W.len = W.ilen - pos < kWindow ? W.ilen - pos : kWindow;
  const u8* src = W.in + pos;
  u8* win = (u8*)__builtin_assume_aligned(W.win, 8);
  if (W.lane >= 0) {
    // 8-byte loads at whatever alignment the container left the chunk,
    // aligned 8-byte LDS stores
#pragma unroll 2
    for (i64 i = (i64)W.lane * 8; i + 8 <= W.len; i += (i64)kLanes * 8) {
      u64 w;
      __builtin_memcpy(&w, src + i, 8);
      __builtin_memcpy(win + i, &w, 8);
    }
#pragma unroll 1
    for (i64 b = (W.len & ~(i64)7) + W.lane; b < W.len; b += kLanes)
      win[b] = src[b];
  }
#if !defined(__HIP_DEVICE_COMPILE__)
  // a host "lane" has no other lanes to fill the rest; the serial build
  // fills it all here
  std::memcpy(win, src, (size_t)W.len);
#endif
  TFR_WAVE_FENCE();  // the walk reads what other lanes staged
}

// Input byte `ip` (< ilen).
TFR_HOSTDEV inline u32 rd(Window& W, i64 ip) {
  if (!W.win) return W.in[ip];
  if (ip - W.base >= W.len) fill(W, ip);
#if defined(__HIP_DEVICE_COMPILE__)
  // every lane read the same byte: say so, and the walk stays scalar
  return (u32)__builtin_amdgcn_readfirstlane((int)W.win[ip - W.base]);
#else
  return W.win[ip - W.base];
#endif
}

// 255 255 .. b behind a nibble of 15. False when the bytes run past the
// input.
TFR_HOSTDEV inline bool extend(Window& W, i64& ip, i64& len) {
  u32 b;
  do {
    if (ip >= W.ilen) return false;
    b = rd(W, ip++);
    len += b;
  } while (b == 255);
  return true;
}

// dst[0, n) = win[woff, woff + n), the lanes' share, no fence. A lane takes
// 8 bytes from the two aligned LDS words that hold them; every read is
// inside win[0, kWindowAlloc) for woff + n <= kWindow.
TFR_HOSTDEV inline void window_copy(u8* dst, const u8* win, i64 woff, i64 n,
                                    int lane) {
  if (lane < 0) {
    for (i64 i = 0; i < n; ++i) dst[i] = win[woff + i];
    return;
  }
  const int sh = (int)(woff & 7) * 8;
  const u8* w = (const u8*)__builtin_assume_aligned(win + (woff & ~(i64)7), 8);
#pragma unroll 1
  for (i64 i = (i64)lane * 8; i + 8 <= n; i += (i64)kLanes * 8) {
    u64 lo, hi;
    __builtin_memcpy(&lo, w + i, 8);
    __builtin_memcpy(&hi, w + i + 8, 8);
    const u64 v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
    __builtin_memcpy(dst + i, &v, 8);
  }
#pragma unroll 1
  for (i64 b = (n & ~(i64)7) + lane; b < n; b += kLanes)
    dst[b] = win[woff + b];
}

// dst[0, len) = the bytes `off` back, the lanes' share. One fence in front
// of every copy that reads what other lanes stored. A match that overlaps
// itself (off < len) is periodic: a short period is first laid out byte by
// byte from the complete period (snappy::period_copy) to a whole number of
// periods of at least 64 bytes, so offsets 1..7 never meet the 8-byte path;
// then the complete part is copied onto what follows it, doubling with
// every round, each round a non-overlapping 8-byte lane_copy at a distance
// that is a multiple of the period.
TFR_HOSTDEV inline void match_copy(u8* dst, u32 off, i64 len, int lane) {
  TFR_WAVE_FENCE();
  if ((i64)off >= len) {
    snappy::lane_copy(dst, dst - off, len, lane, kLanes);
    return;
  }
  i64 done = 0, dist = off;
  if (off < 64) {
    dist = (i64)(63u / off + 1) * off;  // 64..126
    done = len < dist ? len : dist;
    snappy::period_copy(dst, off, done, lane, kLanes);
  }
  while (done < len) {
    if (done) TFR_WAVE_FENCE();
    const i64 n = len - done < dist ? len - done : dist;
    // [dst + done - dist, dst + done) is complete: dist <= off + done
    snappy::lane_copy(dst + done, dst + done - dist, n, lane, kLanes);
    done += n;
    dist *= 2;
  }
}

// Decode one raw LZ4 block in[0, ilen) into out[0, cap). Returns the number
// of bytes produced (0..cap) or -Cause; on any return nothing outside
// [in, in + ilen) has been read and nothing outside [out, out + cap) read
// or written (on failure the output's content is unspecified). A match may
// not reach before `out`: blocks are independent, whatever lies there.
// `lane` < 0 = host/serial; otherwise the whole wave calls this in lockstep
// on one block and `lane` only splits the copies. `win` (or null) is the
// wave's window buffer, see Window.
//
// Literals inside the window go LDS -> output; a literal that is longer
// than what is left of the window goes input -> output by all lanes, and
// the window restarts behind it with the next header read.
TFR_HOSTDEV inline i64 unlz4_block(const u8* __restrict__ in, i64 ilen,
                                   u8* __restrict__ out, i64 cap,
                                   int lane = -1, u8* win = nullptr) {
  Window W{in, ilen, win, 0, 0, lane};
  i64 ip = 0, op = 0;
  for (;;) {
    if (ip >= ilen) return -LZ_INPUT_SHORT;
    const u32 token = rd(W, ip++);
    i64 lit = token >> 4;
    if (lit == 15 && !extend(W, ip, lit)) return -LZ_LENGTH_PAST_INPUT;
    if (lit > ilen - ip) return -LZ_LITERAL_PAST_INPUT;
    if (lit > cap - op) return -LZ_OUTPUT_OVERRUN;
    if (lit) {
      if (win && ip >= W.base && ip + lit <= W.base + W.len)
        window_copy(out + op, win, ip - W.base, lit, lane);
      else
        snappy::lane_copy(out + op, in + ip, lit, lane, kLanes);
      ip += lit;
      op += lit;
    }
    if (ip == ilen) return op;  // the last sequence: literals only
    if (op == cap) return -LZ_INPUT_LEFT;
    if (ilen - ip < 2) return -LZ_INPUT_SHORT;
    const u32 off = rd(W, ip) | (rd(W, ip + 1) << 8);
    ip += 2;
    i64 len = token & 15u;
    if (len == 15 && !extend(W, ip, len)) return -LZ_LENGTH_PAST_INPUT;
    len += 4;
    if (off == 0) return -LZ_OFFSET_ZERO;
    if ((i64)off > op) return -LZ_OFFSET_FAR;
    if (len > cap - op) return -LZ_OUTPUT_OVERRUN;
    match_copy(out + op, off, len, lane);
    op += len;
  }
}

// Decode one container block: in[0, in_len) holds its chunks, each a u32
// big-endian comp_len and comp_len bytes of raw LZ4, and they must produce
// exactly raw_len bytes and use exactly in_len. A chunk does not state how
// much it produces, so each is given what the block still misses as its
// `cap`. Returns LZ_OK or a Cause, with unlz4_block's guarantees for
// [in, in + in_len) and [out, out + raw_len).
TFR_HOSTDEV inline int unlz4_container_block(const u8* __restrict__ in,
                                             i64 in_len,
                                             u8* __restrict__ out, i64 raw_len,
                                             int lane = -1,
                                             u8* win = nullptr) {
  i64 ip = 0, op = 0;
  while (op < raw_len) {
    if (ip == in_len) return LZ_BLOCK_SHORT;
    if (in_len - ip < 4) return LZ_CHUNK_PAST_BLOCK;
    const i64 clen = ((i64)in[ip] << 24) | ((i64)in[ip + 1] << 16) |
                     ((i64)in[ip + 2] << 8) | (i64)in[ip + 3];
    ip += 4;
    if (clen > in_len - ip) return LZ_CHUNK_PAST_BLOCK;
    const i64 got = unlz4_block(in + ip, clen, out + op, raw_len - op, lane,
                                win);
    if (got < 0) return (int)-got;
    ip += clen;
    op += got;
  }
  return ip == in_len ? LZ_OK : LZ_BLOCK_INPUT_LEFT;
}

}  // namespace lz4
}  // namespace tfrec
