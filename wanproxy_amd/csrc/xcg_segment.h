// The XCodec segment on the host: its length and its hash.  No HIP here: the
// kernels' headers (xcg_device.h, xcg_cache.h) and the host-only volume format
// (xcg_volume.cpp) both include this.
#pragma once
#include <stdint.h>

namespace xcg {

constexpr int SEG = 2048;                // XCODEC_SEGMENT_LENGTH, xcodec/xcodec.h:87

// XCodecHash::hash of one whole segment (xcodec/xcodec_hash.h:166-174) on the host.
inline uint64_t host_seg_hash(const uint8_t* w) {
  uint32_t s1 = 0, s2 = 0, b1 = 0, b2 = 0;
  for (uint32_t k = 0; k < 2048; ++k) {
    s1 += (uint32_t)w[k] + 1u;
    s2 += s1;
    b1 += w[k] ? (uint32_t)__builtin_ctz(w[k]) + 1u : 0u;
    b2 += b1;
  }
  return ((uint64_t)((b1 << 16) + b2) << 36) + (uint64_t)((s1 << 20) + s2);
}

}  // namespace xcg
