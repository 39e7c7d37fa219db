// Wave-level pieces of the XCodec op walk shared by the decode kernels
// (xcg_decode.hip: one stream per batch; xcg_decode_indep.hip: one fresh
// decoder per chunk): the op search, the literal-run copy, the EXTRACT payload
// hash and the 2 KiB segment copy.  Device code only, one wave64 per call.
#pragma once
#include "xcg_device.h"

namespace xcg {

// Next real op at or after i in x[0..len): an 0xF1 not followed by 0x00.
// Returns its position (or len) and the number of ESCAPE pairs before it.
// (P: a generic pointer, or an LDS-qualified one for input staged in LDS -- then
// the walk's loads wait on LDS alone, not on the global stores queued behind them)
template <typename P>
__device__ __forceinline__ uint32_t next_op(P x, uint32_t i, uint32_t len, uint32_t& nesc) {
  const int l = lane_id();
  nesc = 0;
  // Fast path: the op follows immediately (EXTRACT/REF-dense streams).
  if (i < len && x[i] == MAGIC && (i + 1 >= len || x[i + 1] != 0u)) return i;
  for (uint32_t base = i; base < len; base += 1024) {
    const uint32_t off = base + 16u * l;
    uint32_t opmask = 0, escmask = 0;
    if (off < len) {
      const uint32_t cnt = min(16u, len - off);
      uint32_t b[17];
#pragma unroll
      for (int k = 0; k < 17; ++k) b[k] = (off + k < len) ? (uint32_t)x[off + k] : 0x100u;  // 0x100: past the end
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        if ((uint32_t)k < cnt && b[k] == MAGIC) {
          if (b[k + 1] == 0u) escmask |= 1u << k;
          else opmask |= 1u << k;
        }
      }
    }
    // An ESCAPE's 0x00 is never itself scanned as a byte that matters (it is
    // not 0xF1), so the masks are exact.  First op in this window:
    const uint64_t bal = ballot(opmask != 0u);
    if (bal) {
      const int lw = __builtin_ctzll(bal);
      const uint32_t om = readlane(opmask, lw);
      const uint32_t pos = base + 16u * lw + __builtin_ctz(om);
      // escapes strictly before pos
      uint32_t e = (uint32_t)l < (uint32_t)lw ? __builtin_popcount(escmask)
                   : ((uint32_t)l == (uint32_t)lw ? __builtin_popcount(escmask & ((1u << __builtin_ctz(om)) - 1u)) : 0u);
      nesc += wave_sum(e);
      return pos;
    }
    nesc += wave_sum(__builtin_popcount(escmask));
  }
  return len;
}

// Copy the literal run x[a..b) (which contains only ESCAPE pairs) to dst with
// F1 00 -> F1.  Returns bytes written.
__device__ __noinline__ uint32_t wave_unescape(uint8_t* dst, const uint8_t* x, uint32_t a, uint32_t b) {
  const int l = lane_id();
  uint32_t written = 0;
  // An escape pair never straddles 16-byte lanes ambiguously: a 0x00 is an
  // escape zero iff the byte before it is 0xF1 (runs hold no other 0xF1).
  for (uint32_t base = a; base < b; base += 1024) {
    const uint32_t off = base + 16u * l;
    uint32_t cnt = off < b ? min(16u, b - off) : 0u;
    uint32_t v[16];
    uint32_t prev = (off > a && off - 1 < b) ? (uint32_t)x[off - 1] : 0u;
    uint32_t keep = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      v[k] = ((uint32_t)k < cnt) ? (uint32_t)x[off + k] : 0u;
      const bool drop = (uint32_t)k < cnt && v[k] == 0u && prev == MAGIC;
      if ((uint32_t)k < cnt && !drop) keep |= 1u << k;
      prev = drop ? 0u : v[k];   // F1 00 F1 00: the 00 resets
    }
    const uint32_t nk = __builtin_popcount(keep);
    const uint32_t incl = wave_incl_scan(nk);
    uint32_t o = written + incl - nk;
    if (nk == 16u && cnt == 16u) {
      u32x4 w;
#pragma unroll
      for (int q = 0; q < 4; ++q) w[q] = v[4 * q] | (v[4 * q + 1] << 8) | (v[4 * q + 2] << 16) | (v[4 * q + 3] << 24);
      *(u32x4_u*)(dst + o) = w;
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if ((keep >> k) & 1u) dst[o++] = (uint8_t)v[k];
    }
    written += readlane(incl, 63);
  }
  return written;
}

// 16 bytes at any alignment, from global memory or from LDS
typedef const __attribute__((address_space(3))) uint8_t* lds_u8p;
typedef const __attribute__((address_space(3))) u32x4_u* lds_u32x4p;
__device__ __forceinline__ u32x4 load16(const uint8_t* p) { return *(const u32x4_u*)p; }
__device__ __forceinline__ u32x4 load16(lds_u8p p) { return *(lds_u32x4p)p; }

template <typename P>
__device__ __noinline__ uint2 dec_window_hash(P w) {
  const int l = lane_id();
  uint32_t X1 = 0, X2 = 0, F1 = 0, F2 = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t k0 = 1024u * h + 16u * l;
    const u32x4 v = load16(w + k0);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t c = byte_of(v[k >> 2], k & 3);
      const uint32_t f = ffbl(c) + 1u;
      const uint32_t wt = 2048u - (k0 + k);
      X1 += c; X2 += wt * c; F1 += f; F2 += wt * f;
    }
  }
  X1 = wave_sum(X1); X2 = wave_sum(X2); F1 = wave_sum(F1); F2 = wave_sum(F2);
  return make_uint2((X1 << 20) + X2 + CLO, ((F1 << 16) + F2) << 4);
}

__device__ __forceinline__ void wave_copy2048(uint8_t* dst, const uint8_t* src) {
  const int l = lane_id();
  *(u32x4_u*)(dst + 32 * l) = *(const u32x4_u*)(src + 32 * l);
  *(u32x4_u*)(dst + 32 * l + 16) = *(const u32x4_u*)(src + 32 * l + 16);
}

template <typename P>
__device__ __forceinline__ uint64_t be64(P p) {
  uint64_t h = 0;
  for (int k = 0; k < 8; ++k) h = (h << 8) | p[k];
  return h;
}

}  // namespace xcg
