// Block-parallel speculative inflate of a gzip member that carries no
// segment table (any writer's file), shared host/device. The technique is
// the one pugz and rapidgzip use:
//
//   1 find    cut the compressed body into chunks; in every chunk but the
//             first, find the first bit that parses as the head of a
//             non-final dynamic-Huffman block
//   2 count   decode from each start found without storing anything, up to
//             the block boundary where another chunk's start sits (or the
//             final block's end): output length, end bit, successor
//   3 chain   follow the successors from chunk 0: the chunks on that chain
//             are live and tile the stream; their lengths, summed, place
//             each one in the output
//   4 decode  decode each live chunk again into 16-bit symbols: a byte, or
//             a marker 0x8000 | w for "byte w of the 32 KiB window before
//             this chunk", which is not known yet
//   5 window  chunk by chunk in order, turn each live chunk's last 32 KiB
//             of symbols into bytes (markers read the bytes before it)
//   6 resolve turn every other symbol into a byte, in any order; then the
//             CRC-32 of the whole output must equal the trailer's
//
// csrc/hip/inflate_foreign.hip runs steps 1, 2 and 4 one chunk per wave
// (the wave in lockstep on one bitstream, as inflate_one); the host build
// below runs all six serially for the CPU tests. Every loop consumes input
// bits or is bounded by a count taken from the tables, so arbitrary bytes
// terminate; every store is checked against the capacity the caller gave.
#pragma once

#include <vector>

#include "inflate_core.h"

namespace tfrec {
namespace inflate {

// Chunk table: kChunkCols i64 per chunk, chunks of one file contiguous.
enum : int {
  CH_FILE = 0,     // file index (filled by the launcher)
  CH_START = 1,    // start bit within the body, -1 = none found
  CH_OUT_LEN = 2,  // count pass: bytes this chunk produces
  CH_END = 3,      // count pass: bit after the last block decoded
  CH_NEXT = 4,     // count pass: successor chunk, kNextEnd or kNextNone
  CH_RC = 5,       // count pass: cause code, 0 = clean
  CH_OUT_OFF = 6,  // chain: output offset within the file, -1 = not live
  CH_LIVE = 7,     // chain: row k holds the k-th live chunk's index
  kChunkCols = 8
};
// File table: kFileCols i64 per file (filled by the launcher).
enum : int {
  FL_BODY_OFF = 0,  // deflate body within the compressed buffer
  FL_BODY_LEN = 1,
  FL_ISIZE = 2,
  FL_CRC = 3,
  FL_CHUNK0 = 4,    // first row in the chunk table
  FL_NCHUNK = 5,
  FL_OUT_BASE = 6,  // first output byte within the output buffer
  FL_SYM_BASE = 7,  // first symbol within the symbol buffer
  FL_PIECE0 = 8,    // first row in the CRC piece table
  kFileCols = 10
};
// Result table: kResCols i64 per file.
enum : int {
  RS_ERR = 0,      // init -1; atomicMin of ((chunk + 1) << 8) | cause
  RS_LIVE = 1,     // live chunks
  RS_CRC = 2,      // CRC-32 computed over the output
  RS_MARKERS = 3,  // marker symbols resolved
  kResCols = 4
};

constexpr i64 kNextEnd = -1;   // the chunk ran to the final block's end
constexpr i64 kNextNone = -2;  // the chunk did not finish
constexpr i64 kSpecWindow = 32768;
constexpr i64 kSpecCrcPiece = 64 << 10;  // bytes per CRC piece

// Cause codes past inflate_one's 1..17 and parse_dyn_header's 20..23.
enum : int {
  SPEC_REACH = 18,       // a match reaches past the window or the file start
  SPEC_CYCLE = 30,       // chain: more links than chunks
  SPEC_CHUNK_RC = 31,    // chain: a live chunk reported a cause
  SPEC_TOO_LONG = 32,    // chain: lengths exceed ISIZE
  SPEC_END = 33,         // chain: final block does not end at the body end
  SPEC_LINK = 34,        // chain: successor out of order or range
  SPEC_ISIZE = 35,       // chain: lengths do not sum to ISIZE
  SPEC_DISAGREE = 36,    // decode pass and count pass differ
  SPEC_MARKER = 37,      // a marker points before the file start
  SPEC_CRC = 40          // member CRC-32 mismatch
};

// Bit position of the reader within the body it was seeked on.
TFR_HOSTDEV inline i64 br_pos(const BitRd& b, const u8* body) {
  return ((i64)(b.p - body) - b.pre_n) * 8 - b.n;
}

TFR_HOSTDEV inline void br_seek(BitRd& b, const u8* body, i64 body_len,
                                i64 bit) {
  br_init(b, body + (bit >> 3), body_len - (bit >> 3));
  if (bit & 7) br_bits(b, (int)(bit & 7));
}

// The 96 bits at `bit`, low-order first; bytes past the body end read 0.
struct Bits96 {
  u64 lo;
  u32 hi;
};

TFR_HOSTDEV inline Bits96 load_bits96(const u8* body, i64 body_len, i64 bit) {
  i64 byte = bit >> 3;
  int s = (int)(bit & 7);
  u64 a = 0, b = 0;
  if (byte + 16 <= body_len) {
    __builtin_memcpy(&a, body + byte, 8);
    __builtin_memcpy(&b, body + byte + 8, 8);
  } else {
    for (int i = 0; i < 8; ++i) {
      if (byte + i < body_len) a |= (u64)body[byte + i] << (8 * i);
      if (byte + 8 + i < body_len) b |= (u64)body[byte + 8 + i] << (8 * i);
    }
  }
  Bits96 w;
  w.lo = s ? (a >> s) | (b << (64 - s)) : a;
  w.hi = (u32)(b >> s);
  return w;
}

// Register-only screen of a block head: BFINAL = 0, BTYPE = 2, HLIT and
// HDIST within the alphabets, and the code-length code complete (Kraft sum
// exactly 1 over the 4..19 three-bit lengths). About one random position
// in two thousand passes; those get full_head_check.
TFR_HOSTDEV inline bool cheap_head_check(Bits96 w) {
  u32 h = (u32)w.lo;
  if ((h & 7u) != 4u) return false;
  if (((h >> 3) & 31u) > 29u || ((h >> 8) & 31u) > 29u) return false;
  int hclen = (int)((h >> 13) & 15u) + 4;
  u64 lo = (w.lo >> 17) | ((u64)w.hi << 47);  // lengths 0..20
  u32 kraft = 0;
  for (int i = 0; i < 19; ++i) {
    u32 l = (u32)lo & 7u;
    lo >>= 3;
    if (i < hclen && l) kraft += 128u >> l;
  }
  return kraft == 128u;
}

// The whole head at `bit`: the strict header parse, then symbol 256 coded,
// the literal/length code complete, the distance code complete or of at
// most one code (what a compressor emits for no or one distance).
TFR_HOSTDEV inline bool full_head_check(const u8* body, i64 body_len, i64 bit,
                                        LaneScratch& L) {
  BitRd br;
  br_seek(br, body, body_len, bit);
  u32 head = br_bits(br, 3);
  if (br.n < 0 || head != 4u) return false;
  int hlit, hdist;
  if (parse_dyn_header<true>(br, L, hlit, hdist)) return false;
  if (!get_len4(L.lens4, 256)) return false;
  u32 kl = 0, kd = 0, nd = 0;
  for (int s = 0; s < hlit; ++s) {
    u32 l = get_len4(L.lens4, s);
    if (l) kl += 32768u >> l;
  }
  for (int s = 0; s < hdist; ++s) {
    u32 l = get_len4(L.lens4, hlit + s);
    if (l) {
      kd += 32768u >> l;
      ++nd;
    }
  }
  return kl == 32768u && (kd == 32768u || nd <= 1);
}

// Steps 2 and 4: decode blocks from start_bit until a block ends where
// another chunk's start sits (ct = the file's rows of the chunk table) or
// the final block ends. WRITE = false only counts; WRITE = true stores one
// symbol per output byte into sym[0, out_limit). out_limit is ISIZE for
// the count pass and the count pass's length for the decode pass: nothing
// is stored, or counted, past it. `hist` is the number of output bytes
// before this chunk (how far back a match may reach at all). `lane` as in
// inflate_one.
template <bool WRITE, int NLANES = 64>
TFR_HOSTDEV inline int spec_run(const u8* __restrict__ body, i64 body_len,
                                i64 start_bit, const i64* ct,
                                i64 nchunk, i64 chunk_bits, i64 out_limit,
                                uint16_t* __restrict__ sym, i64 hist,
                                LaneScratch& L,
                                uint16_t* __restrict__ lit_tab,
                                uint16_t* __restrict__ dist_tab, int lane,
                                i64& out_len, i64& end_bit, i64& next) {
  constexpr int nlanes = NLANES;
  const int l0 = lane < 0 ? 0 : lane;
  const int lstep = lane < 0 ? 1 : nlanes;
  BitRd br;
  br_seek(br, body, body_len, start_bit);
  i64 opos = 0;
  out_len = 0;
  end_bit = start_bit;
  next = kNextNone;
  for (;;) {
    u32 final = br_bits(br, 1);
    u32 btype = br_bits(br, 2);
    if (br.n < 0) return 1;
    if (btype == 0) {  // stored
      br.buf >>= (br.n & 7);
      br.n &= ~7;
      u32 len = br_bits(br, 16);
      u32 nlen = br_bits(br, 16);
      if (br.n < 0 || ((len ^ nlen) & 0xFFFFu) != 0xFFFFu) return 2;
      const u8* src = br.p - br.pre_n - (br.n >> 3);
      if (src + len > br.end || opos + (i64)len > out_limit) return 3;
      if (WRITE) {
        for (i64 i = l0; i < (i64)len; i += lstep) sym[opos + i] = src[i];
        TFR_WAVE_FENCE();
      }
      opos += len;
      br.p = src + len;
      br.buf = 0;
      br.n = 0;
      br.pre = 0;
      br.pre_n = 0;
      br_load_pre(br);
    } else if (btype == 3) {
      return 4;
    } else {
      int hlit, hdist, dist_off;
      if (btype == 1) {  // fixed codes
        hlit = 288;
        hdist = 32;
        dist_off = 288;
        for (int s = 0; s < 144; ++s) set_len4(L.lens4, s, 8);
        for (int s = 144; s < 256; ++s) set_len4(L.lens4, s, 9);
        for (int s = 256; s < 280; ++s) set_len4(L.lens4, s, 7);
        for (int s = 280; s < 288; ++s) set_len4(L.lens4, s, 8);
        for (int s = 0; s < 32; ++s) set_len4(L.lens4, 288 + s, 5);
      } else {
        int rc = parse_dyn_header<false>(br, L, hlit, hdist);
        if (rc) return rc;
        dist_off = hlit;
      }
      if (!build_huff4(L.lens4, 0, hlit, L.bc_lit, L.rank_lit, L.sym))
        return 9;
      if (!build_huff4(L.lens4, dist_off, hdist, L.bc_dist, L.rank_dist,
                       &L.sym[288]))
        return 10;
      fill_huff_table<kLitTabBits>(L.bc_lit, L.sym, lit_tab, lane, nlanes);
      fill_huff_table<kDistTabBits>(L.bc_dist, &L.sym[288], dist_tab, lane,
                                    nlanes);
      for (;;) {
        int s = huff_decode_tab<kLitTabBits>(br, L.bc_lit, L.sym, lit_tab);
        if (s < 0) return 11;
        if (s < 256) {
          if (opos >= out_limit) return 12;
          if (WRITE) sym[opos] = (uint16_t)s;
          ++opos;
        } else if (s == 256) {
          break;
        } else {
          s -= 257;
          if (s >= 29) return 13;
          i64 mlen = kLenBase[s] + (i64)br_bits(br, kLenExtra[s]);
          int d = huff_decode_tab<kDistTabBits>(br, L.bc_dist, &L.sym[288],
                                                dist_tab);
          if (d < 0 || d >= 30) return 14;
          i64 dist = kDistBase[d] + (i64)br_bits(br, kDistExtra[d]);
          if (br.n < 0) return 15;
          if (opos + mlen > out_limit) return 16;
          if (dist > opos &&
              (dist - opos > kSpecWindow || dist - opos > hist))
            return SPEC_REACH;
          if (WRITE) {
            // src < 0 lies -src bytes before this chunk: byte
            // (32768 + src) of the window that ends at the chunk's start
            const i64 from = opos - dist;
            if (lane >= 0 && dist >= mlen) {
              for (i64 i = l0; i < mlen; i += lstep) {
                i64 src = from + i;
                sym[opos + i] = src < 0
                                    ? (uint16_t)(0x8000 | (kSpecWindow + src))
                                    : sym[src];
              }
              TFR_WAVE_FENCE();
            } else {
              for (i64 i = 0; i < mlen; ++i) {
                i64 src = from + i;
                sym[opos + i] = src < 0
                                    ? (uint16_t)(0x8000 | (kSpecWindow + src))
                                    : sym[src];
              }
            }
          }
          opos += mlen;
        }
      }
    }
    i64 e = br_pos(br, body);
    out_len = opos;
    end_bit = e;
    if (final) {
      next = kNextEnd;
      return 0;
    }
    // at most one start per chunk, inside the chunk: only the chunk that
    // holds bit e can start at e; starts below e are passed over for good
    i64 j = e / chunk_bits;
    if (j > 0 && j < nchunk && ct[j * kChunkCols + CH_START] == e) {
      next = j;
      return 0;
    }
  }
}

// Step 3, one thread per file. Fills CH_OUT_OFF of the live chunks and the
// CH_LIVE list; returns 0 or ((chunk + 1) << 8) | cause.
TFR_HOSTDEV inline i64 spec_chain(i64* ct, i64 nchunk, i64 body_len,
                                  i64 isize, i64& n_live) {
  i64 j = 0, total = 0, k = 0;
  n_live = 0;
  for (;;) {
    i64* c = ct + j * kChunkCols;
    if (k >= nchunk) return ((j + 1) << 8) | SPEC_CYCLE;
    if (c[CH_RC] != 0 || c[CH_NEXT] == kNextNone)
      return ((j + 1) << 8) | SPEC_CHUNK_RC;
    c[CH_OUT_OFF] = total;
    ct[k * kChunkCols + CH_LIVE] = j;
    ++k;
    total += c[CH_OUT_LEN];
    if (c[CH_OUT_LEN] < 0 || total > isize)
      return ((j + 1) << 8) | SPEC_TOO_LONG;
    i64 nx = c[CH_NEXT];
    if (nx == kNextEnd) {
      if (((c[CH_END] + 7) >> 3) != body_len) return ((j + 1) << 8) | SPEC_END;
      break;
    }
    if (nx <= j || nx >= nchunk) return ((j + 1) << 8) | SPEC_LINK;
    j = nx;
  }
  if (total != isize) return ((j + 1) << 8) | SPEC_ISIZE;
  n_live = k;
  return 0;
}

// Steps 5 and 6 for one symbol at output position `pos` of a chunk that
// starts at chunk_start: the byte it stands for, or -1 for a marker that
// points before the file start. `out` is the file's output.
TFR_HOSTDEV inline int spec_resolve_sym(uint16_t s, const u8* out,
                                        i64 chunk_start, i64& markers) {
  if (!(s & 0x8000u)) return (int)(s & 0xFFu);
  ++markers;
  i64 idx = chunk_start - kSpecWindow + (i64)(s & 0x7FFFu);
  if (idx < 0 || idx >= chunk_start) return -1;
  return out[idx];
}

// gzip member framing (RFC 1952): walks FEXTRA, FNAME, FCOMMENT and FHCRC.
// Returns false unless the bytes are one CM = 8 member of at least 18
// bytes; the body is everything between the header and the 8-byte trailer.
inline bool parse_gzip_member(const u8* p, i64 n, i64& body_off, i64& body_len,
                              u32& crc, u32& isize) {
  if (n < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8) return false;
  u32 flg = p[3];
  if (flg & 0xE0u) return false;  // reserved bits
  i64 pos = 10;
  if (flg & 4u) {
    if (pos + 2 > n) return false;
    pos += 2 + (i64)(p[pos] | (p[pos + 1] << 8));
  }
  for (u32 bit = 8u; bit <= 16u; bit <<= 1) {  // FNAME, FCOMMENT
    if (!(flg & bit)) continue;
    while (pos < n && p[pos]) ++pos;  // zero-terminated
    ++pos;
  }
  if (flg & 2u) pos += 2;
  if (pos + 8 > n) return false;
  body_off = pos;
  body_len = n - 8 - pos;
  auto le32 = [&](i64 o) {
    return (u32)p[o] | ((u32)p[o + 1] << 8) | ((u32)p[o + 2] << 16) |
           ((u32)p[o + 3] << 24);
  };
  crc = le32(n - 8);
  isize = le32(n - 4);
  return true;
}


// ---------------------------------------------------------------------------
// Host run of the six steps over one gzip member, serially, on the tables
// the kernels use. For the CPU tests and the sanitizer self-test; it is not
// a read path. Returns 0 and fills `out`, or the error word (a cause
// word as in RS_ERR, or -2 for bytes that are no eligible gzip member).
// ---------------------------------------------------------------------------
struct SpecStats {
  i64 candidates = 0;    // block starts the finder reported
  i64 live = 0;          // chunks on the chain
  i64 false_starts = 0;  // starts that decoded with an error
  i64 discarded = 0;     // starts off the chain (false ones included)
  i64 markers = 0;       // marker symbols resolved
};

// Whether the device path takes a member at all (the rest goes to zlib).
// DEFLATE cannot expand past 1032:1, so a larger ISIZE is not worth buffers.
inline bool spec_eligible(i64 body_len, u32 isize) {
  return isize != 0 && body_len > 0 && body_len < ((i64)1 << 32) &&
         (i64)isize <= body_len * 1032 + 64;
}

inline i64 host_spec_inflate(const u8* gz, i64 n, i64 chunk_bytes,
                             std::vector<u8>& out_bytes, SpecStats& st) {
  i64 body_off, body_len;
  u32 crc, isize;
  if (chunk_bytes <= 0 ||
      !parse_gzip_member(gz, n, body_off, body_len, crc, isize) ||
      !spec_eligible(body_len, isize))
    return -2;
  const u8* body = gz + body_off;
  const i64 chunk_bits = chunk_bytes * 8;
  const i64 nchunk = (body_len + chunk_bytes - 1) / chunk_bytes;
  i64* ct = new i64[nchunk * kChunkCols];
  uint16_t* sym = nullptr;  // sized once the chain has confirmed ISIZE
  u8* out = nullptr;
  LaneScratch* L = new LaneScratch;
  uint16_t* lit_tab = new uint16_t[kLitTabSize];
  uint16_t* dist_tab = new uint16_t[kDistTabSize];
  i64 err = 0;
  for (i64 j = 0; j < nchunk; ++j) {
    i64* c = ct + j * kChunkCols;
    for (int k = 0; k < kChunkCols; ++k) c[k] = 0;
    c[CH_START] = -1;
    c[CH_NEXT] = kNextNone;
    c[CH_OUT_OFF] = -1;
  }
  ct[CH_START] = 0;
  for (i64 j = 1; j < nchunk; ++j) {  // 1 find
    i64 lo = j * chunk_bits;
    i64 hi = lo + chunk_bits < body_len * 8 ? lo + chunk_bits : body_len * 8;
    for (i64 bit = lo; bit < hi; ++bit) {
      if (cheap_head_check(load_bits96(body, body_len, bit)) &&
          full_head_check(body, body_len, bit, *L)) {
        ct[j * kChunkCols + CH_START] = bit;
        ++st.candidates;
        break;
      }
    }
  }
  for (i64 j = 0; j < nchunk; ++j) {  // 2 count
    i64* c = ct + j * kChunkCols;
    if (c[CH_START] < 0) continue;
    c[CH_RC] = spec_run<false>(body, body_len, c[CH_START], ct, nchunk,
                               chunk_bits, (i64)isize, nullptr,
                               j ? (i64)isize : 0, *L, lit_tab, dist_tab, -1,
                               c[CH_OUT_LEN], c[CH_END], c[CH_NEXT]);
    if (j && c[CH_RC]) ++st.false_starts;
  }
  i64 n_live = 0;
  err = spec_chain(ct, nchunk, body_len, (i64)isize, n_live);  // 3 chain
  st.live = n_live;
  st.discarded = st.candidates - (n_live ? n_live - 1 : 0);
  if (!err) {
    sym = new uint16_t[isize];
    out_bytes.assign((size_t)isize, 0);
    out = out_bytes.data();
  }
  for (i64 k = 0; !err && k < n_live; ++k) {  // 4 decode
    i64 j = ct[k * kChunkCols + CH_LIVE];
    i64* c = ct + j * kChunkCols;
    i64 olen, end, next;
    int rc = spec_run<true>(body, body_len, c[CH_START], ct, nchunk,
                            chunk_bits, c[CH_OUT_LEN], sym + c[CH_OUT_OFF],
                            c[CH_OUT_OFF], *L, lit_tab, dist_tab, -1, olen,
                            end, next);
    if (!rc && (olen != c[CH_OUT_LEN] || end != c[CH_END] ||
                next != c[CH_NEXT]))
      rc = SPEC_DISAGREE;
    if (rc) err = ((j + 1) << 8) | rc;
  }
  for (int pass = 0; pass < 2 && !err; ++pass) {  // 5 window, 6 resolve
    for (i64 k = 0; !err && k < n_live; ++k) {
      i64 j = ct[k * kChunkCols + CH_LIVE];
      i64 start = ct[j * kChunkCols + CH_OUT_OFF];
      i64 len = ct[j * kChunkCols + CH_OUT_LEN];
      i64 tail = len > kSpecWindow ? len - kSpecWindow : 0;
      for (i64 i = pass ? 0 : tail; i < (pass ? tail : len); ++i) {
        int b = spec_resolve_sym(sym[start + i], out, start, st.markers);
        if (b < 0) {
          err = ((j + 1) << 8) | SPEC_MARKER;
          break;
        }
        out[start + i] = (u8)b;
      }
    }
  }
  if (!err) {  // member CRC over fixed pieces, folded as the kernels do
    u32 acc = 0;
    const u32 sh = crc32_ieee_shift_elem((u64)kSpecCrcPiece);
    for (i64 a = 0; a < (i64)isize; a += kSpecCrcPiece) {
      i64 len = (i64)isize - a < kSpecCrcPiece ? (i64)isize - a
                                               : kSpecCrcPiece;
      u32 c = crc32_ieee(out + a, (size_t)len);
      acc = len == kSpecCrcPiece ? crc_ieee_gfmul(acc, sh) ^ c
                                 : crc32_ieee_combine(acc, c, (u64)len);
    }
    if (acc != crc) err = SPEC_CRC;
  }
  delete[] ct;
  delete[] sym;
  delete L;
  delete[] lit_tab;
  delete[] dist_tab;
  return err;
}
}  // namespace inflate
}  // namespace tfrec
