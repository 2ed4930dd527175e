// Wave-cooperative CRC-32 (IEEE), shared by the device compressor
// (deflate.hip) and the foreign-gzip inflater (inflate_foreign.hip).
#pragma once

#include "../crc32c.h"
#include "../deflate_core.h"  // TFR_WAVE_SYNC

namespace tfrec {

// CRC-32 of in[0, n) by one wave: each lane checksums a contiguous chunk
// (all chunks but the last share one length, so one shift element serves
// them), lane 0 folds the 64 values in order.
__device__ inline uint32_t crc32_ieee_wave(const uint8_t* __restrict__ in,
                                           int64_t n, int lane,
                                           uint32_t* lds) {
  int64_t chunk = (((n + 63) / 64) + 7) & ~(int64_t)7;
  int64_t lo = (int64_t)lane * chunk;
  if (lo > n) lo = n;
  int64_t hi = lo + chunk < n ? lo + chunk : n;
  lds[lane] = crc32_ieee(in + lo, (size_t)(hi - lo));
  TFR_WAVE_SYNC();
  uint32_t acc = 0;
  if (lane == 0 && n > 0) {
    uint32_t full = crc32_ieee_shift_elem((uint64_t)chunk);
    for (int l = 0; l < 64; ++l) {
      int64_t a = (int64_t)l * chunk;
      if (a >= n) break;
      int64_t len = a + chunk < n ? chunk : n - a;
      uint32_t sh = len == chunk ? full : crc32_ieee_shift_elem((uint64_t)len);
      acc = crc_ieee_gfmul(acc, sh) ^ lds[l];
    }
  }
  TFR_WAVE_SYNC();
  return acc;  // valid on lane 0
}

}  // namespace tfrec
