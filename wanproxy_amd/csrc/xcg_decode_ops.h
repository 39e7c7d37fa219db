// Wave-level pieces of the XCodec op walk shared by the decode kernels
// (xcg_decode.hip, xcg_decode_bounded.hip and xcg_decode_small.hip through
// xcg_decode_batch.h: one stream per batch or call; xcg_decode_indep.hip: one fresh
// decoder per chunk; xcg_decode_group.hip: one per group of chunks): the op
// search, the literal-run copy, the EXTRACT payload hash, the 2 KiB segment
// copy, and the per-wave LDS decoder (cache table and window) of the
// independent and grouped kernels.  Device code only, one wave64 per call.
#pragma once
#include "xcg_device.h"
#include "xcg_cache.h"

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

// ---- a decoder in one wave's LDS (decode_independent_kernel, decode_group_kernel)
//   X   its cache: hash -> where the EXTRACT payload lies (open addressing,
//       probed 64 slots at a time); a later EXTRACT of a hash overwrites the
//       value: cache_->replace, or the same bytes (xcodec_decoder.cc:106-136).
//   W   its XCodecWindow (xcodec/xcodec_window.h:68-111): 256 slots of (hash,
//       source) and the cursor.  A slot keeps the source its declare saw.
// SRC names a payload: a chunk-local offset (uint32_t) or an offset into the
// whole batch input (uint64_t).  ~0 is an empty slot, never an offset.
template <int XSLOTS, typename SRC>
struct DecWave {
  static constexpr SRC NONE = (SRC)~(SRC)0;
  uint64_t xk[XSLOTS];   // X keys (valid where xv != NONE)
  uint64_t wh[256];      // W hashes (valid where ws != NONE)
  SRC xv[XSLOTS];
  SRC ws[256];
};

__device__ __forceinline__ uint32_t readlane_src(uint32_t v, int l) { return readlane(v, l); }
__device__ __forceinline__ uint64_t readlane_src(uint64_t v, int l) { return readlane64(v, l); }

// One wave's LDS writes are visible to its own later reads, whichever lanes
// made them (the LDS serves a wave's instructions in order): this only keeps
// the compiler from moving or reusing LDS accesses across it.
__device__ __forceinline__ void lds_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// X lookup, wave-uniform: the payload source of h, or NONE; `slot` is where h
// is, or the empty slot it would take.  Lane l probes slot s + l.
template <int XSLOTS, typename SRC>
__device__ __forceinline__ SRC xtab_find(const DecWave<XSLOTS, SRC>& S, uint64_t h, uint32_t& slot) {
  constexpr SRC NONE = DecWave<XSLOTS, SRC>::NONE;
  const uint32_t l = (uint32_t)lane_id();
  uint32_t s = tab_slot((uint32_t)h, (uint32_t)(h >> 32), XSLOTS - 1);
  for (;;) {                                                 // ends: X is never more than half full
    const uint32_t idx = (s + l) & (XSLOTS - 1);
    const SRC v = S.xv[idx];
    const uint64_t k = S.xk[idx];
    const uint64_t hit = ballot(v != NONE && k == h), emp = ballot(v == NONE);
    const uint32_t ph = hit ? (uint32_t)__builtin_ctzll(hit) : 64u, pe = emp ? (uint32_t)__builtin_ctzll(emp) : 64u;
    if (ph < pe) {
      slot = (s + ph) & (XSLOTS - 1);
      return readlane_src(v, (int)ph);
    }
    if (pe < 64u) {
      slot = (s + pe) & (XSLOTS - 1);
      return NONE;
    }
    s += 64u;
  }
}

// XCodecWindow::declare (xcodec_window.h:68-99): the slot that holds the hash
// already is emptied, the cursor's slot takes (hash, src), the cursor wraps.
// Lane l owns slots l, l + 64, l + 128, l + 192.
template <int XSLOTS, typename SRC>
__device__ __forceinline__ void win_declare(DecWave<XSLOTS, SRC>& S, uint32_t& cursor, uint64_t h, SRC src) {
  constexpr SRC NONE = DecWave<XSLOTS, SRC>::NONE;
  const uint32_t l = (uint32_t)lane_id();
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t idx = l + 64u * j;
    if (idx == cursor) {
      S.wh[idx] = h;
      S.ws[idx] = src;
    } else if (S.ws[idx] != NONE && S.wh[idx] == h) {
      S.ws[idx] = NONE;
    }
  }
  cursor = (cursor + 1u) & 255u;
  lds_wave_sync();
}

// Does an op start right at x[i] (an 0xF1 not followed by 0x00)?  Asked for the
// next op before the current op's stores are issued: on gfx9 a load's wait
// also drains the stores queued before it.
__device__ __forceinline__ bool op_at(const uint8_t* x, uint32_t i, uint32_t len) {
  if (i >= len) return false;
  const uint32_t b0 = x[i], b1 = i + 1 < len ? (uint32_t)x[i + 1] : 0x100u;
  return readfirst(b0) == MAGIC && readfirst(b1) != 0u;
}

}  // namespace xcg
