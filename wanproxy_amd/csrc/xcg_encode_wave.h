// XCodec encoder, MI355X (gfx950) HIP kernels.
//
// Restates XCodecEncoder::encode (xcodec/xcodec_encoder.cc:74-274) for a batch
// of independent encode() calls: one wave64 per chunk, so a 64 KiB chunk (the
// unit tack and wanproxy hand to encode(), programs/tack/tack.cc:308-321,
// io/io_system_handle.cc:39) is parsed by 64 lanes with no inter-wave sync.
//
// The reference walks every byte offset sequentially: roll the 2048-byte
// XCodecHash (xcodec_hash.h:93-163), probe the cache (find_reference,
// xcodec_encoder.cc:374-416), and run a greedy candidate / declare / reference
// state machine (:183-248).  Here a chunk is parsed in PIECES of 2048 window
// positions:
//
//   1. vector phase: lane i rolls the hash over the 32 positions
//      [p + 32 i, p + 32 i + 32) -- its start sums come from wave prefix scans
//      over 32-byte segment sums -- and probes a per-wave LDS fingerprint table
//      of the declarations made so far, producing a 32-bit event mask;
//   2. resolve phase (wave-uniform): the state machine jumps from event to
//      event through those masks.  Within 2048 positions of the parse point at
//      most ONE declaration can become visible (the candidate pending at piece
//      start, visible from cand + 2048), which the vector phase covers with a
//      gated compare, so every event the masks miss is a true miss.
//
// Events are re-checked exactly (full 64-bit hash, then byte compare against
// the declared segment) before a REF or a collision skip is emitted, so the
// fingerprint table can be approximate without affecting output.  Output ops
// (ESCAPE / EXTRACT / REF, xcodec_encoder.cc:276-372) are written by the whole
// wave as they are resolved, into the chunk's output slot.
//
// This header is the device code the encoder's units share: encode_chunk and
// its parts.  Its kernels: xcg_encode_indep.hip, xcg_encode_group.hip,
// xcg_encode_stream.h (instances in xcg_encode_stream.hip and _lru.hip);
// xcg_encode_screen.hip uses the piece sums.
#pragma once
#include <stddef.h>

#include <type_traits>

#include "xcg_cache.h"
#include "xcg_args.h"
#include "../../include/xcgpu.h"

namespace xcg {

// A chunk's piece loads.  Independent chunks read theirs as streaming
// (non-temporal) loads: each byte is read once, and the headline launch runs
// ~5 % faster so (the stream kernel, whose probes read L2-resident tables,
// measured no gain: C4 654 vs 636 us, C2-S2 294 vs 297).
constexpr bool STREAM_NT = false;   // stream chunks: plain loads
template <bool STREAM>
__device__ __forceinline__ u32x4 piece_ld_safe(const uint8_t* x, int q, int len) {
  if constexpr (STREAM && !STREAM_NT) return load16_aligned_safe(x, q, len);
  else return load16_aligned_safe_stream(x, q, len);
}
template <bool STREAM>
__device__ __forceinline__ u32x4 piece_ld(const uint8_t* p) {
  if constexpr (STREAM && !STREAM_NT) return *(const u32x4*)p;
  else return load16_stream(p);
}

// Per-wave LDS state of one encode() call's XCodecMemoryCache
// (xcodec_cache.h:245-365): a 2-slot-bucket table of probe keys K = -lo over
// the chunk's declarations -- bucket = bits 3.. of K; an empty slot of bucket b
// holds kempty(b), whose bucket bits are ~b, so it never equals a K probed
// there -- plus the exact records the slots point to.  The key tables of a
// block's waves sit first in LDS, 8 << LOGNB bytes each, so a lane's probe
// address is a single and-or of K.
// Overflow keys a chunk's table holds: 8, or 32 for frames of up to 512 KiB
// (~256 declarations in 1024 buckets: a tail of 9+ three-key buckets happens).
// Independent chunks' direct-mapped tables (DMV, roll_probe_dm): 32, a key
// overflowing as soon as its slot is taken.
template <int MAXD, bool DMV = false>
constexpr int ovf_cap() { return MAXD > 72 || DMV ? 32 : 8; }

template <int LOGNB, int MAXD, bool DMV = false>
struct WaveRecs {
  static constexpr int NB = 1 << LOGNB;
  uint32_t rlo[MAXD], rhi[MAXD], rc[MAXD];  // exact hash + chunk position
  uint32_t ovf_k[ovf_cap<MAXD, DMV>()];     // keys whose bucket was full
};

template <int LOGNB>
__device__ __forceinline__ uint32_t kbucket(uint32_t k) { return (k >> 3) & ((1u << LOGNB) - 1u); }
template <int LOGNB>
__device__ __forceinline__ uint32_t kempty(uint32_t b) { return (~b & ((1u << LOGNB) - 1u)) << 3; }

typedef __attribute__((address_space(3))) uint8_t lds_u8;
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
// DM: the direct-mapped table of chunks of up to 128 KiB (roll_probe_dm).
template <int LOGNB, int MAXD, int W, bool DM = (MAXD <= 72)>
struct IndepLDS {
  uint32_t key[W][2 << LOGNB];
  WaveRecs<LOGNB, MAXD, false> rec[W];
  __device__ __forceinline__ const lds_u8* ring_of(int) const { return nullptr; }
};
// Its waves also stage their pieces' entering bytes through two 2 KiB buffers
// each (encode_chunk, "the input ring"), written by LDS-DMA loads.
template <int LOGNB, int MAXD, int W>
struct IndepLDS<LOGNB, MAXD, W, true> {
  uint32_t key[W][2 << LOGNB];
  WaveRecs<LOGNB, MAXD, true> rec[W];
  alignas(16) uint8_t ring[W][2][2048];
  __device__ __forceinline__ const lds_u8* ring_of(int wv) const { return (const lds_u8*)&ring[wv][0][0]; }
};
constexpr int GSLOTS = 8;        // pass-1 queue depth per lane (roll_probe)
template <int LOGNB, int MAXD, int W>
struct StreamLDS {
  uint32_t key[W][2 << LOGNB];               // offset 0, as in IndepLDS
  uint32_t lfilt[FILT_WORDS];                // the lane filter (64 KiB)
  uint32_t scr[W][GSLOTS + 1][64];           // pass-1 queues (+ a garbage slot)
  WaveRecs<LOGNB, MAXD> rec[W];
  uint32_t ro[W][MAXD];                      // output length after each declaration's op (restart points)
  uint32_t rsv[W][8];                        // restart state (kept out of registers)
  uint32_t cmax;                             // the workgroup's highest chunk (prefix filter slice)
};

// Re-parse restart (bounded / pair passes after the first; the driver backs up
// the previous pass's rows of each flagged chunk, xcg_restart_backup_kernel).
struct RestartArgs {
  const uint32_t* bad_t;   // [n] in-chunk time of the chunk's earliest contradicted lookup (~0: none)
  const uint32_t* bad_hi;  // [n] ... and of its latest
  const uint32_t* bslot;   // [n] backup slot of the chunk's previous pass (~0: none)
  const uint4* b_ev;       // [slots * maxe] its reference rows
  const uint32_t* b_eo;    // [slots * maxe] their REF output lengths
  const uint64_t* b_hits;  // [slots * maxh] its batch hits
  const uint32_t* b_cnt;   // [slots * 4] its nev, nhits, output length, ndecl
  uint4* splice;           // [n] {new offset, old offset, old end, 1}: the old tail to append
};

struct EncParams {
  const uint8_t* in;
  const uint64_t* chunk_off;
  const uint32_t* chunk_len;
  uint32_t n;
  uint32_t flags;
  uint8_t* out;
  const uint64_t* out_off;
  uint64_t* out_len;
  uint32_t* stats;     // optional: per chunk {n_extract, n_ref, n_collision, n_pieces}
  int32_t* status;     // optional: nonzero on internal overflow
  // ---- stream semantics (XCG_SEM_STREAM) only
  HashTab g;           // the persistent cache: hash -> segment index
  const uint8_t* pool; // its segment bytes
  HashTab b;           // this batch's declarations (earlier rounds): hash -> (chunk << 32 | pos)
  bool use_b;
  LaneFilter lf;       // lane probe filter over g + b
  uint4* decl;         // [n * maxd] (lo, hi, pos, 0) declarations of the chunk, this round
  uint32_t* ndecl;     // [n]
  uint32_t maxd;
  uint32_t* changed;   // lowest chunk whose declaration list differs from the last round (~0: none)
  uint32_t lds_filter_keys;  // LDS lane filter up to this many keys, else the global one
  uint32_t lds_prefilter_keys;  // up to this many: the LDS filter in front of the global one (fmode 3)
  const uint32_t* nseg;    // segments in the persistent cache
  const uint32_t* bcount;  // [64] partial counts of the batch table's declarations (use_b)
  uint32_t skip_below; // chunks below this keep their last parse (their batch input is unchanged)
  const uint32_t* need;  // (verification rounds) parse only chunks with need[c] != 0
  uint64_t* hits;      // [n * maxh] hashes the chunk found among the batch declarations (REF or collision)
  uint32_t* nhits;     // [n] (> maxh: overflowed, always re-parsed)
  uint32_t maxh;
  uint32_t max_len;    // the caller's bound on every chunk length (sizes LDS records and declaration rows)
  // ---- bounded (LRU) cache only (xcg_lru.hip); null otherwise
  const uint64_t* ptime;  // [pool slot] batch time from which the entry is evicted (~0: never)
  uint4* ev;           // [n * maxe] the chunk's cache references in order (lo, hi, time, kind << 30 | ref)
  uint32_t* nev;       // [n] (> maxe: overflowed)
  uint32_t maxe;
  uint32_t* eo;        // [n * maxe] output length after the REF a lookup made (~0: it made none)
  RestartArgs rs;      // re-parse from the previous pass's rows (bslot null: off)
  // ---- (stream) parse only the chunks of a work list: work[0] = count, work[1..] chunks (null: all)
  const uint32_t* work;
};

// INDEP_W chunk-waves per workgroup, INDEP_OCC workgroups per CU: four waves
// per SIMD, one resident wave per chunk of a 4096-chunk launch.
// (xcg_encode_indep.hip, and one wave per group in xcg_encode_group.hip)
constexpr int INDEP_W = 4;
constexpr int INDEP_OCC = 4;
// The 64 KiB / 128 KiB instance's direct-mapped key table: 2 << 9 = 1024 slots
// per wave.  The input ring's 4 KiB per wave came out of it (2048 slots before),
// so a workgroup stays at 36,736 B and four share a CU's LDS; the smaller table
// alone measured +0.4 %, the ring 0.942 of the register prefetch's time
// (profiles/indep_ring_ab.txt).
constexpr int INDEP_LOGNB = 9;

// ------------------------------------------------------------------ emission

// Copy n bytes src -> dst (any alignment), whole wave.
inline __device__ __noinline__ void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t n) {
  const int l = lane_id();
  for (uint32_t base = 0; base < n; base += 1024) {
    uint32_t off = base + 16u * l;
    if (off + 16 <= n) {
      *(u32x4_u*)(dst + off) = *(const u32x4_u*)(src + off);
    } else if (off < n) {
      for (uint32_t k = off; k < n; ++k) dst[k] = src[k];
    }
  }
}

// encode_escape (xcodec_encoder.cc:315-340): x[a..b) with F1 -> F1 00.
// Returns bytes written (uniform).
inline __device__ __noinline__ uint32_t wave_escape(uint8_t* dst, const uint8_t* x, uint32_t a, uint32_t b) {
  const int l = lane_id();
  const uint32_t n = b - a;
  uint32_t written = 0;
  for (uint32_t base = 0; base < n; base += 1024) {
    uint32_t off = base + 16u * l;
    uint32_t cnt = off < n ? min(16u, n - off) : 0u;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (cnt == 16) {
      v = *(const u32x4_u*)(x + a + off);
    } else {
      for (uint32_t k = 0; k < cnt; ++k) v[k >> 2] |= (uint32_t)x[a + off + k] << (8 * (k & 3));
    }
    uint32_t nm = count_magic(v[0]) + count_magic(v[1]) + count_magic(v[2]) + count_magic(v[3]);
    if (cnt < 16) {
      // padding bytes are 0 (never magic) unless the chunk byte was; recount exactly
      nm = 0;
      for (uint32_t k = 0; k < cnt; ++k) nm += byte_of(v[k >> 2], k & 3) == MAGIC;
    }
    uint32_t olen = cnt + nm;
    uint32_t incl = wave_incl_scan(olen);
    uint32_t pos = written + incl - olen;
    if (nm == 0) {
      if (cnt == 16) {
        *(u32x4_u*)(dst + pos) = v;
      } else {
        for (uint32_t k = 0; k < cnt; ++k) dst[pos + k] = (uint8_t)byte_of(v[k >> 2], k & 3);
      }
    } else {
      uint32_t o = pos;
      for (uint32_t k = 0; k < cnt; ++k) {
        uint32_t c = byte_of(v[k >> 2], k & 3);
        dst[o++] = (uint8_t)c;
        if (c == MAGIC) dst[o++] = (uint8_t)OP_ESCAPE;
      }
    }
    written += readlane(incl, 63);
  }
  return written;
}

// F1 02 BE64(hash): encode_reference, xcodec_encoder.cc:357-360.
__device__ __forceinline__ void wave_put_ref(uint8_t* dst, uint32_t lo, uint32_t hi) {
  const int l = lane_id();
  if (l < 10) {
    uint32_t v;
    if (l == 0) v = MAGIC;
    else if (l == 1) v = OP_REF;
    else if (l < 6) v = hi >> (8 * (5 - l));
    else v = lo >> (8 * (9 - l));
    dst[l] = (uint8_t)v;
  }
}

// ------------------------------------------------------------ exact checks

// XCodecHash::hash of the 2048-byte window at w (xcodec_hash.h:166-174),
// whole wave: lane l sums bytes [16l, 16l+16) and [1024+16l, +16).  z = the
// window's direct-mapped probe key -(X2 + CLO) (independent chunks, see
// roll_probe_dm).
inline __device__ __noinline__ uint3 wave_window_hash(const uint8_t* w) {
  const int l = lane_id();
  uint32_t X1 = 0, X2 = 0, F1 = 0, F2 = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t k0 = 1024u * h + 16u * l;
    u32x4 v = *(const u32x4_u*)(w + k0);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      uint32_t x = byte_of(v[k >> 2], k & 3);
      uint32_t f = ffbl(x) + 1u;
      uint32_t wt = 2048u - (k0 + k);
      X1 += x; X2 += wt * x; F1 += f; F2 += wt * f;
    }
  }
  X1 = wave_sum(X1); X2 = wave_sum(X2); F1 = wave_sum(F1); F2 = wave_sum(F2);
  return make_uint3((X1 << 20) + X2 + CLO, ((F1 << 16) + F2) << 4, 0u - (X2 + CLO));
}

// Byte-equality of two 2048-byte segments (BufferSegment::equal in
// find_reference, xcodec_encoder.cc:383-390), whole wave.
inline __device__ __noinline__ bool wave_equal2048(const uint8_t* a, const uint8_t* b) {
  const int l = lane_id();
  bool ok = true;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t k0 = 1024u * h + 16u * l;
    u32x4 va = *(const u32x4_u*)(a + k0);
    u32x4 vb = *(const u32x4_u*)(b + k0);
    ok = ok && va[0] == vb[0] && va[1] == vb[1] && va[2] == vb[2] && va[3] == vb[3];
  }
  return ballot(!ok) == 0;
}

// Call-site wrappers: a non-inlined call returns in VGPRs, which hipcc must
// treat as divergent; these values are wave-uniform, and saying so keeps the
// whole parse state machine in SGPRs / scalar branches.
__device__ __forceinline__ uint32_t escape_u(uint8_t* dst, const uint8_t* x, uint32_t a, uint32_t b) {
  return readfirst(wave_escape(dst, x, a, b));
}
__device__ __forceinline__ uint3 window_hash_u(const uint8_t* w) {
  const uint3 h = wave_window_hash(w);
  return make_uint3(readfirst(h.x), readfirst(h.y), readfirst(h.z));
}
__device__ __forceinline__ bool equal2048_u(const uint8_t* a, const uint8_t* b) {
  return readfirst((uint32_t)wave_equal2048(a, b)) != 0u;
}
// The same compare when the window is a piece start: its bytes are the A
// registers (lane l holds [32 l, 32 l + 32)), so only the other side is read.
__device__ __forceinline__ bool equal2048_regs(const uint8_t* a, const u32x4& w0, const u32x4& w1) {
  const uint32_t o = 32u * (uint32_t)lane_id();
  const u32x4 v0 = *(const u32x4_u*)(a + o), v1 = *(const u32x4_u*)(a + o + 16);
  const bool ok = v0[0] == w0[0] && v0[1] == w0[1] && v0[2] == w0[2] && v0[3] == w0[3] && v1[0] == w1[0] &&
                  v1[1] == w1[1] && v1[2] == w1[2] && v1[3] == w1[3];
  return ballot(!ok) == 0;
}

// ------------------------------------------------------------ vector phase

// Make the registers of v live here (the compiler waits for their load first).
__device__ __forceinline__ void vuse(const u32x4& v) {
  asm volatile("" ::"v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]));
}

// The input ring (independent chunks): the entering bytes of the next two
// contiguous pieces go global -> LDS without passing through registers, as a
// linear image of the 2 KiB (lane l's two 16-byte loads read src + 16 l and
// src + 1024 + 16 l: whole lines; the instruction offset applies to both
// sides), non-temporal like the register loads.  hipcc does not count these
// loads: the waits for them are written by hand (encode_chunk).
__device__ __forceinline__ void ring_load(const uint8_t* src, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off nt\n\t"
      "global_load_lds_dwordx4 %1, off offset:1024 nt\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(src), "s"(lds_dst)
      : "memory");
}

struct Piece {
  u32x4 a0, a1;   // bytes [q0, q0+32): the windows' leaving bytes
  u32x4 b0, b1;   // bytes [q0+2048, q0+2080): the entering bytes
  // byte sums of the A and B segments: plain and weighted by j (offset in it)
  uint32_t sxa, sqxa;
  uint32_t sxb, sqxb;
};

__device__ __forceinline__ void seg_sums(const u32x4 d0, const u32x4 d1, uint32_t& sx, uint32_t& sqx) {
  const uint32_t d[8] = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
  sx = 0; sqx = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t wts = (4u * k) | ((4u * k + 1) << 8) | ((4u * k + 2) << 16) | ((4u * k + 3) << 24);
    sx = __builtin_amdgcn_udot4(d[k], 0x01010101u, sx, false);
    sqx = __builtin_amdgcn_udot4(d[k], wts, sqx, false);
  }
}

// bits_hash half of the hash of the window that starts at lane L's first
// position (bytes A of lanes >= L, then B of lanes < L), from the registers:
// hi = ((F1 << 16) + F2) << 4 with F1 = sum ffs(x), F2 = sum (2048 - k) ffs(x_k)
// (XCodecHash, xcodec_hash.h:93-174).  Only candidates need it.
__device__ __forceinline__ uint32_t lane_window_hi(const Piece& P, int L) {
  const int l = lane_id();
  const bool useA = l >= L;
  const uint32_t d[8] = {useA ? P.a0[0] : P.b0[0], useA ? P.a0[1] : P.b0[1], useA ? P.a0[2] : P.b0[2],
                         useA ? P.a0[3] : P.b0[3], useA ? P.a1[0] : P.b1[0], useA ? P.a1[1] : P.b1[1],
                         useA ? P.a1[2] : P.b1[2], useA ? P.a1[3] : P.b1[3]};
  uint32_t sf = 0, sqf = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t f = ffbl(byte_of(d[k], b)) + 1u;
      sf += f;
      sqf += (4u * k + b) * f;
    }
  }
  const uint32_t o = 32u * (uint32_t)((l - L) & 63);   // lane's offset in the window
  const uint32_t F1 = wave_sum(sf), F2 = wave_sum((2048u - o) * sf - sqf);
  return ((F1 << 16) + F2) << 4;
}

// Lane mask of a == b, straight from v_cmp (a bool would be materialised
// in a VGPR and compared again before any ballot).
__device__ __forceinline__ uint64_t lanes_eq(uint32_t a, uint32_t b) { return __builtin_amdgcn_uicmp(a, b, 32); }

// ev = 2 ev + (this lane's bit of m) in one v_addc, m being the carry-in: no
// per-position bit constants, which VOP3 cannot encode as literals on gfx9.
__device__ __forceinline__ uint32_t shift_in(uint32_t ev, uint64_t m) {
  uint32_t r;
  uint64_t co;
  asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(r), "=s"(co) : "v"(ev), "s"(readfirst64(m)));
  return r;
}

// Stream-semantics probe of the persistent cache + batch declarations.
// Pass 1 (inside the roll): the key's lane-filter word -- the blocked-Bloom
// LDS filter (xcg_cache.h filt_*) or, for large caches, the global one
// (gfilt_*); a passing key is queued in the wave's LDS scratch, slot
// min(passes, GSLOTS) of the lane (slot-major, so a wave's 64 stores are
// consecutive dwords), and its position bit set in pm.  Pass 2 (glb_flush,
// after each half of the lane's 32 positions) checks the queued keys against
// the 16-bit fingerprint buckets (an L2-resident table), all of a lane's
// loads in flight together instead of one round trip per group of positions.
// Passes beyond GSLOTS in one half are reported as events unchecked.
// FM 3 (caches past the LDS filter's ~220 k keys): the global filter mode is
// bound by L2 requests, one per window position (rocprofv3 TCC_READ ~430 M per
// 512 MiB C5 sub-batch at a 97 % L2 hit rate, profiles/r06_l2_*), so the
// saturated LDS filter (FP ~0.4 at 260 k keys, ~0.7 at 470 k) goes first and
// only the lanes it passes load their global word (exec-masked: the other
// lanes send no request).
// (with the prefix slices; measured on C2-S2 / C5, profiles/r06_filter_modes.txt:
// the two-level mode beats the LDS filter alone beyond ~150 k keys)
constexpr uint32_t LDS_FILTER_KEYS_DEFAULT = 150000;
constexpr uint32_t LDS_PREFILTER_KEYS_DEFAULT = 700000;
struct GlbQ {
  char* lds;        // LDS base of the workgroup's struct (offset 0)
  uint32_t lfo;     // byte offset of the lane filter (FM 1)
  const uint32_t* gf;   // global lane filter (FM 2)
  uint32_t gmask;
  const u32x4* ftab;    // fingerprint buckets
  uint32_t fmask;
  uint32_t sa0;     // this lane's scratch slot 0 (absolute LDS byte address)
  uint32_t sa;      // its next slot
  uint32_t salim;   // its garbage slot (slot GSLOTS)
  uint32_t pm;      // filter passes of the current half, bit j = position j
  uint32_t gev;     // verified cache / batch hits, bit j = position j
};

// Pass 2 over the queued keys of the current half; resets the queue.
__device__ __forceinline__ void glb_flush(GlbQ& gq) {
  const uint32_t cnt = (gq.sa - gq.sa0) >> 8;
  uint32_t rem = gq.pm;
#pragma unroll
  for (int i0 = 0; i0 < GSLOTS; i0 += 4) {
    if (ballot(cnt > (uint32_t)i0) == 0) break;
    uint32_t kk[4];
    u32x4 q[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) kk[t] = *(const uint32_t*)(gq.lds + gq.sa0 + 256u * (i0 + t));
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      q[t] = u32x4{0u, 0u, 0u, 0u};
      if ((uint32_t)(i0 + t) < cnt) q[t] = gq.ftab[fbucket(kk[t], gq.fmask)];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if ((uint32_t)(i0 + t) < cnt) {
        const uint32_t j = (uint32_t)__builtin_ctz(rem);
        rem &= rem - 1u;
        gq.gev |= (uint32_t)ftab_match(q[t], kk[t]) << j;
      }
    }
  }
  gq.gev |= rem;
  gq.pm = 0;
  gq.sa = gq.sa0;
}

// Roll the probe key over the lane's 32 positions; bit j of the result is set
// when position q0 + j is a possible cache hit.  NX1 = -X1, NX2 = -(X2 + CLO)
// at q0 (RollingHash::roll, xcodec_hash.h:57-70, negated), so K = -lo costs one
// instruction.  C0: the pending candidate (key c0k) is not in the table yet and
// becomes visible at piece offset rvis (position p + rvis).  OVF: also compare the (rare) overflow
// keys ovk[NOVF].  FM: also run pass 1 of the persistent cache / batch probe (gq)
// through the LDS lane filter (1) or the global one (2); 0: no such probe.
template <int LOGNB, bool C0, int NOVF, int FM>
__device__ __forceinline__ uint32_t roll_probe(const Piece& P, uint32_t NX1, uint32_t NX2, const char* kblk,
                                               uint32_t kofs, uint32_t c0k, int rvis, const uint32_t* ovk,
                                               GlbQ& gq) {
  constexpr bool GLB = FM != 0;
  // bucket mask in a VGPR so that (K & KM) | kofs is one v_and_or_b32 (VOP3
  // takes no literal and one SGPR on gfx9)
  const uint32_t KM = (uint32_t)opaque((int)(((1u << LOGNB) - 1u) << 3));
  const uint32_t xa[8] = {P.a0[0], P.a0[1], P.a0[2], P.a0[3], P.a1[0], P.a1[1], P.a1[2], P.a1[3]};
  const uint32_t xb[8] = {P.b0[0], P.b0[1], P.b0[2], P.b0[3], P.b1[0], P.b1[1], P.b1[2], P.b1[3]};
  uint32_t o[NOVF > 0 ? NOVF : 1];
#pragma unroll
  for (int k = 0; k < NOVF; ++k) o[k] = ovk[k];
  // C0 visibility: lanes l with 32 l + j >= rvis.  With rvis = 32 A + B that is
  // l >= A + 1 for j < B and l >= A for j >= B -- two masks per piece.
  uint64_t vis_hi = 0, vis_lo = 0;
  int vB = 0;
  if (C0) {
    const int A = rvis >> 5;
    vB = rvis & 31;
    auto from_lane = [](int t) -> uint64_t { return t <= 0 ? ~0ull : (t >= 64 ? 0ull : (~0ull << t)); };
    vis_hi = from_lane(A + 1);
    vis_lo = from_lane(A);
  }
  uint32_t ev = 0;
  // Groups of 4 positions, software-pipelined: group g+1's keys are rolled and
  // its 4 LDS probes issued before group g's probes are compared, so each
  // group's LDS latency overlaps the next group's arithmetic.  The
  // sched_barrier keeps hipcc from hoisting more than that (VGPRs).
  auto roll4 = [&](int g, uint32_t (&kv)[4], uint2 (&e)[4], uint32_t (&fw)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = 4 * g + t;
      kv[t] = (NX1 << 20) + NX2;
      if (j < 31) {
        const uint32_t xo = byte_of(xa[j >> 2], j & 3);
        const uint32_t xn = byte_of(xb[j >> 2], j & 3);
        NX1 += xo - xn;
        NX2 += NX1 + (xo << 11);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) e[t] = *(const uint2*)(kblk + ((kv[t] & KM) | kofs));
    if (FM == 1 || FM == 3) {
#pragma unroll
      for (int t = 0; t < 4; ++t) fw[t] = *(const uint32_t*)(gq.lds + gq.lfo + filt_word_ofs(kv[t]));
    } else if (FM == 2) {
#pragma unroll
      for (int t = 0; t < 4; ++t) fw[t] = gq.gf[gfilt_word(kv[t], gq.gmask)];
    }
    if (FM == 3) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const uint32_t w = filt_test(fw[t], kv[t]) ? gq.gf[gfilt_word(kv[t], gq.gmask)] : 0u;
        fw[t] = w;
      }
    }
  };
  uint32_t kc[4], fc[4];
  uint2 ec[4];
  roll4(0, kc, ec, fc);
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    uint32_t kn[4], fn[4];
    uint2 en[4];
    if (g < 7) roll4(g + 1, kn, en, fn);
    if (GLB) {
      // Persistent cache + batch declarations, pass 1: queue filter passes.
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const uint32_t p = FM == 1 ? filt_test(fc[t], kc[t]) : gfilt_test(fc[t], kc[t]);   // (FM 3: 0 if the LDS one failed)
        *(uint32_t*)(gq.lds + gq.sa) = kc[t];
        gq.sa = min(gq.sa + (p << 8), gq.salim);
        gq.pm |= p << (4 * g + t);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = 4 * g + t;
      uint64_t hit = lanes_eq(ec[t].x, kc[t]) | lanes_eq(ec[t].y, kc[t]);
      if (C0) hit |= lanes_eq(kc[t], c0k) & (j < vB ? vis_hi : vis_lo);
#pragma unroll
      for (int k = 0; k < NOVF; ++k) hit |= lanes_eq(o[k], kc[t]);
      ev = shift_in(ev, hit);
    }
    asm volatile("" : "+v"(ev));   // materialise this group's bits before the next group
    __builtin_amdgcn_sched_barrier(0);
    if (GLB && (g == 3 || g == 7)) glb_flush(gq);
    if (g < 7) {
#pragma unroll
      for (int t = 0; t < 4; ++t) { kc[t] = kn[t]; ec[t] = en[t]; fc[t] = fn[t]; }
    }
  }
  return __builtin_bitreverse32(ev) | (GLB ? gq.gev : 0u);   // ev: position j was shifted in at bit 31 - j
}

// Independent chunks of up to 128 KiB (the headline path): the wave's table
// holds only its own chunk's declarations (at most 63), so its probe key need
// not be -lo, which the persistent cache's filters are built on.  It is NX2 =
// -(X2 + CLO), the rolled weighted sum itself (no key instruction), in a
// direct-mapped table of 2 << LOGNB slots (slot = bits 2.. of the key; one
// compare; a key whose slot is taken is an overflow key).  EVW false: return
// only the lanes with a possible hit (per lane, the minimum of slot ^ key over
// its positions is 0), no per-position event bit -- in independent chunks
// almost every piece has none, and a piece that has one is rolled again with
// EVW true for its event word.  Per position: 4 VALU to roll, 1 for the LDS
// address, 1.5 for the xor / min3 (vs 9 for roll_probe's event word).
template <int LOGNB>
__device__ __forceinline__ uint32_t dm_slot_mask() { return ((2u << LOGNB) - 1u) << 2; }
template <int LOGNB>
__device__ __forceinline__ uint32_t dm_empty(uint32_t slot) { return (~slot & ((2u << LOGNB) - 1u)) << 2; }

template <int LOGNB, bool C0, int NOVF, bool EVW>
__device__ __forceinline__ uint64_t roll_probe_dm(const Piece& P, uint32_t NX1, uint32_t NX2, const char* kblk,
                                                  uint32_t kofs, uint32_t c0k, int rvis, const uint32_t* ovp,
                                                  uint32_t novf) {
  const uint32_t KM = (uint32_t)opaque((int)dm_slot_mask<LOGNB>());
  const uint32_t xa[8] = {P.a0[0], P.a0[1], P.a0[2], P.a0[3], P.a1[0], P.a1[1], P.a1[2], P.a1[3]};
  const uint32_t xb[8] = {P.b0[0], P.b0[1], P.b0[2], P.b0[3], P.b1[0], P.b1[1], P.b1[2], P.b1[3]};
  // (unused overflow slots repeat a real overflow key)
  uint32_t o[NOVF > 0 ? NOVF : 1];
#pragma unroll
  for (int k = 0; k < NOVF; ++k) o[k] = readfirst(ovp[(uint32_t)k < novf ? k : 0]);
  uint64_t vis_hi = 0, vis_lo = 0;
  int vB = 0;
  if (C0) {
    const int A = rvis >> 5;
    vB = rvis & 31;
    auto from_lane = [](int t) -> uint64_t { return t <= 0 ? ~0ull : (t >= 64 ? 0ull : (~0ull << t)); };
    vis_hi = from_lane(A + 1);
    vis_lo = from_lane(A);
  }
  static_assert(EVW || !C0, "a piece with a pending candidate takes the event word directly");
  uint32_t ev = 0, amin = ~0u;
  auto roll4 = [&](int g, uint32_t (&kv)[4], uint32_t (&e)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = 4 * g + t;
      kv[t] = NX2;
      if (j < 31) {
        const uint32_t xo = byte_of(xa[j >> 2], j & 3);
        const uint32_t xn = byte_of(xb[j >> 2], j & 3);
        NX1 += xo - xn;
        NX2 += NX1 + (xo << 11);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) e[t] = *(const uint32_t*)(kblk + ((kv[t] & KM) | kofs));
  };
  uint32_t kc[4], ec[4];
  roll4(0, kc, ec);
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    uint32_t kn[4], en[4];
    if (g < 7) roll4(g + 1, kn, en);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = 4 * g + t;
      if (EVW) {
        uint64_t hit = lanes_eq(ec[t], kc[t]);
        if (C0) hit |= lanes_eq(kc[t], c0k) & (j < vB ? vis_hi : vis_lo);
#pragma unroll
        for (int k = 0; k < NOVF; ++k) hit |= lanes_eq(o[k], kc[t]);
        ev = shift_in(ev, hit);
      }
    }
    if (!EVW) {
      // per lane: the minimum of (slot ^ key) over the positions is 0 iff one
      // matched -- xor + half a min3 per position, no SGPR round trip
      uint32_t xx[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) xx[t] = ec[t] ^ kc[t];
      amin = min(amin, min(xx[0], xx[1]));
      amin = min(amin, min(xx[2], xx[3]));
#pragma unroll
      for (int k = 0; k < NOVF; ++k) {
#pragma unroll
        for (int t = 0; t < 4; t += 2) amin = min(amin, min(o[k] ^ kc[t], o[k] ^ kc[t + 1]));
      }
    }
    if (EVW) asm volatile("" : "+v"(ev));
    __builtin_amdgcn_sched_barrier(0);
    if (g < 7) {
#pragma unroll
      for (int t = 0; t < 4; ++t) { kc[t] = kn[t]; ec[t] = en[t]; }
    }
  }
  return EVW ? (uint64_t)__builtin_bitreverse32(ev) : ballot(amin == 0u);
}

// ------------------------------------------------------------------ kernel

// Waves sharing a SIMD issue by priority, then age: with equal priorities the
// oldest of the four chunk-waves runs ahead and the youngest finishes alone,
// leaving its SIMD under-used.  A wave's priority falls as it parses its
// chunk (bands 1/2, 3/4, 15/16: a wave that reaches a band boundary first
// yields until the others catch up), so the four finish nearly together;
// only the last 1/16 is age-ordered.
__device__ __forceinline__ void progress_priority(int s, int L) {
  const int s16 = 16 * s;                          // sixteenths of the chunk parsed: 16 s / L (no division)
  if (s16 < 8 * L) __builtin_amdgcn_s_setprio(3);
  else if (s16 < 12 * L) __builtin_amdgcn_s_setprio(2);
  else if (s16 < 15 * L) __builtin_amdgcn_s_setprio(1);
  else __builtin_amdgcn_s_setprio(0);
}

// The diagnostics builds' clock: encode_chunk marks its spans on a WaveClock.
// Shipped build: WaveClockOff (no data, every mark empty; the stats words are
// the chunk's op counts).  -DXCG_TIMING (scripts/dev/wave_timing.py): {start,
// end} of the chunk's wave (100 MHz realtime, low words), HW_ID, XCC_ID.
// -DXCG_PHASES (scripts/dev/stream_phases.py): {vector phase, slot 1, whole chunk}
// ticks, events << 16 | pieces; XCG_PHASES_SLOT1: 0 exact events, 1 piece setup, 2 prefetch wait.
struct WaveClockOff {
  static constexpr bool ON = false;   // store() replaces the op counts
  __device__ __forceinline__ void piece_begin() {}
  __device__ __forceinline__ void chain_begin() {}
  __device__ __forceinline__ void chain_end() {}
  __device__ __forceinline__ void vector_begin() {}   // (ends the piece's setup)
  __device__ __forceinline__ void wait_begin() {}
  __device__ __forceinline__ void wait_end() {}
  __device__ __forceinline__ void vector_end() {}
  struct Event {   // an exact event check, until the end of its scope
    __device__ __forceinline__ explicit Event(WaveClockOff&) {}
  };
  __device__ __forceinline__ void store(uint32_t*, uint32_t, uint32_t) {}
};
#if defined(XCG_PHASES)
#ifndef XCG_PHASES_SLOT1
#define XCG_PHASES_SLOT1 0
#endif
struct WaveClock {
  static constexpr bool ON = true;
  static __device__ __forceinline__ uint64_t now() { return __builtin_amdgcn_s_memrealtime(); }
  const uint64_t t_start = now();
  uint64_t t_piece = 0, t_chain = 0, t_vec = 0, t_wait = 0;
  uint64_t vec = 0, chain = 0, ev = 0, setup = 0, wait = 0;
  uint32_t nev = 0;
  __device__ __forceinline__ void piece_begin() { t_piece = now(); }
  __device__ __forceinline__ void chain_begin() { t_chain = now(); }
  __device__ __forceinline__ void chain_end() { chain += now() - t_chain; }
  __device__ __forceinline__ void vector_begin() { t_vec = now(); setup += t_vec - t_piece; }
  __device__ __forceinline__ void wait_begin() { t_wait = now(); }
  __device__ __forceinline__ void wait_end() { wait += now() - t_wait; }
  __device__ __forceinline__ void vector_end() { vec += now() - t_vec; }
  struct Event {
    WaveClock& c;
    const uint64_t t0;
    __device__ __forceinline__ explicit Event(WaveClock& clk) : c(clk), t0(now()) { ++c.nev; }
    __device__ __forceinline__ ~Event() { c.ev += now() - t0; }
  };
  __device__ __forceinline__ void store(uint32_t* stats, uint32_t chunk, uint32_t n_pieces) {
    stats[4 * chunk + 0] = (uint32_t)vec;
    stats[4 * chunk + 1] = (uint32_t)(XCG_PHASES_SLOT1 == 2 ? wait : XCG_PHASES_SLOT1 ? setup : ev);
    stats[4 * chunk + 2] = (uint32_t)(now() - t_start);
    stats[4 * chunk + 3] = (nev << 16) | n_pieces;
  }
};
#elif defined(XCG_TIMING)
struct WaveClock : WaveClockOff {
  static constexpr bool ON = true;
  const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
  __device__ __forceinline__ void store(uint32_t* stats, uint32_t chunk, uint32_t) {
    const uint64_t t_end = __builtin_amdgcn_s_memrealtime();
    stats[4 * chunk + 0] = (uint32_t)t_start;
    stats[4 * chunk + 1] = (uint32_t)t_end;
    stats[4 * chunk + 2] = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));    // HW_REG_HW_ID
    stats[4 * chunk + 3] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11));   // HW_REG_XCC_ID
  }
};
#else
using WaveClock = WaveClockOff;
#endif

// One wave encodes chunk `chunk` (one XCodecEncoder::encode call).  Its key
// table is kblk + kofs (LDS), its records T.  STREAM: the cache also holds the
// persistent GPU cache g and the batch declarations b of chunks < chunk,
// probed through the workgroup's LDS filter lfilt.
// What a stream wave probes besides its own table: the workgroup's LDS (base
// = offset 0), where the lane filter sits (lfo), the wave's pass-1 scratch
// (sofs), and which filter pass 1 reads (fmode; 0 = the filter holds nothing).
struct GlbView {
  char* lds;
  uint32_t lfo;
  uint32_t sofs;
  int fmode;   // 0: no probe, 1: LDS lane filter, 2: global lane filter, 3: LDS filter, then global
  uint32_t* ro;   // (stream) the wave's per-declaration output lengths, LDS
  uint32_t* rsv;  // (stream) the wave's restart state, LDS: slot, old nev, nhits, olen, ndecl, restart ndecl
};

// GROUP (xcg_encode_group.hip): the chunk is one encode() call of a short
// stream whose earlier calls this wave has made, on the same cache.  The key
// table, the records and the overflow keys are then carried, not cleared
// (the kernel clears them once per group), with their counts in `gc`; a record
// names its segment by its byte offset in the whole batch input (T.rc the low
// word, gc->rch bits 32..47: device addresses have 48 bits), since it may lie
// in an earlier chunk, placed anywhere.  Everything else of the parse is per
// call, as in the reference.
struct GroupCarry {
  uint32_t ndecl, novf;   // records and overflow keys so far
  uint16_t* rch;          // LDS, [MAXD]: bits 32..47 of the records' input offsets
  int done, total;        // bytes of the group parsed before this chunk, and in all (progress_priority)
};

template <int LOGNB, int MAXD, bool STREAM, bool LRU = false, bool GROUP = false>
__device__ __forceinline__ void encode_chunk(const EncParams& prm, char* kblk, const uint32_t kofs,
                                             WaveRecs<LOGNB, MAXD, (!STREAM && MAXD <= 72)>& T, const uint32_t chunk,
                                             const GlbView gs, const lds_u8* ring = nullptr,
                                             GroupCarry* gc = nullptr) {
  static_assert(!GROUP || (!STREAM && !LRU), "a group is a batch of fresh caches");
  constexpr int NB = 1 << LOGNB;
  // independent chunks of up to 128 KiB: direct-mapped NX2 keys (roll_probe_dm), input through `ring`
  constexpr bool DM = !STREAM && MAXD <= 72;
  const int l = lane_id();

  // (GROUP: a later chunk's loads follow the kernel's own stores, so they are
  // vector loads; their values are wave-uniform, and the parse state stays in SGPRs)
  const uint8_t* x = prm.in + (GROUP ? readfirst64(prm.chunk_off[chunk]) : prm.chunk_off[chunk]);
  const int L = (int)(GROUP ? readfirst(prm.chunk_len[chunk]) : prm.chunk_len[chunk]);
  uint8_t* const out = prm.out + (GROUP ? readfirst64(prm.out_off[chunk]) : prm.out_off[chunk]);
  const bool oob = (prm.flags & XCG_FLAG_OOB) != 0;
  const bool nullcache = (prm.flags & XCG_FLAG_NULLCACHE) != 0;
  uint32_t olen = 0;
  uint32_t n_extract = 0, n_ref = 0, n_coll = 0, n_pieces = 0;

  WaveClock clk;
  // A chunk longer than the launch's bound would overrun the records sized
  // for it: refuse it loudly (status bit 3) instead.
  // (a group is refused as a whole by its kernel, which has summed its lengths)
  if (!GROUP && ((uint32_t)L > prm.max_len || (uint32_t)L / SEG >= (uint32_t)MAXD)) {
    if (l == 0) {
      prm.out_len[chunk] = 0;
      if (prm.status) atomicOr(prm.status, 8);
      if (LRU) prm.nev[chunk] = 0;
    }
    return;
  }
  if (L < SEG) {                                   // xcodec_encoder.cc:77-83
    if (L > 0) olen = escape_u(out, x, 0, (uint32_t)L);
    if (l == 0) {
      prm.out_len[chunk] = olen;
      if (LRU) prm.nev[chunk] = 0;                 // (no cache reference; the list is scratch)
      if constexpr (GROUP) {                       // (the carried cache is untouched: ordinary traffic)
        if (prm.stats) {
          for (int k = 0; k < 4; ++k) prm.stats[4 * chunk + k] = 0u;
        }
      }
    }
    // (GROUP: lane 0's branch joins here, not at the group loop's latch, where
    // the carried counts of the different exits meet: they stay wave-uniform)
    if constexpr (GROUP) __builtin_amdgcn_wave_barrier();
    return;
  }

  uint32_t* const keyt = (uint32_t*)(kblk + kofs);
  if constexpr (!GROUP) {
    for (int k = l; k < 2 * NB; k += 64) keyt[k] = DM ? dm_empty<LOGNB>((uint32_t)k) : kempty<LOGNB>((uint32_t)k >> 1);
  }
  uint32_t ndecl = 0, novf = 0;
  if constexpr (GROUP) { ndecl = gc->ndecl; novf = gc->novf; }
  // (GROUP) a record's segment: its offset in the batch input; else in the chunk
  const uint64_t xin = GROUP ? (uint64_t)(x - prm.in) : 0u;
  auto rec_bytes = [&](uint32_t d) -> const uint8_t* {
    if constexpr (GROUP) return prm.in + (((uint64_t)readfirst((uint32_t)gc->rch[d]) << 32) | readfirst(T.rc[d]));
    else return x + readfirst(T.rc[d]);
  };
  // (stream) the own key table overflowed: this parse may have missed one of
  // its own declarations.  The chunk's hit count becomes maxh + 1, which the
  // verification treats as "always re-parse" (structured data can put a
  // transient round's many declarations into few buckets; the re-parse sees the
  // round's lists); a result no verification follows is checked by the driver.
  bool own_ovf = false;

  const int last = L - SEG;                        // last window start
  const int mis = (int)(reinterpret_cast<uintptr_t>(x) & 15u);
  int s = 0, base = 0;
  bool have_cand = false;
  int cand = 0;
  uint32_t cand_lo = 0, cand_hi = 0;
  uint32_t cand_k = 0;                             // (DM) the candidate's probe key
  // In-band independent encoding never outputs a declared hash, and its hi half
  // only matters when a later window matches the declaration's lo: then it is
  // computed from the declared bytes (lookup).  HI_LAZY (odd) marks "not yet";
  // a real hi has its low 4 bits clear (mix(), xcodec_hash.h:155-164).
  constexpr uint32_t HI_LAZY = 1u;
  const bool lazy_hi = !STREAM && !oob;
  bool c0_in_table = true;                         // pending candidate already inserted?

  Piece P;
  int p_prev = INT32_MIN;
  // Registers that already hold window bytes: the previous piece's A half
  // (bytes [p_prev, p_prev + 2048) across the wave) and the next piece's
  // prefetched B half (the bucket-table variants' only input path).
  u32x4 nb0 = {0u, 0u, 0u, 0u}, nb1 = nb0;
  int nb_start = INT32_MIN;
  // (DM) The input ring instead of nb*: buffer (p >> 11) & 1 holds the
  // entering bytes of the piece at p.  rg_n = how many of the next contiguous
  // pieces have theirs loaded or under way; rg_steady = whether each of the
  // last two pieces issued a ring load and then the quiet steady state's
  // three stores (bit 0: the latest piece).
  int rg_n = 0;
  uint32_t rg_steady = 0;
  // A candidate set at the piece start has its whole segment in the wave's A
  // registers; its EXTRACT body is written to the output right then, at the
  // offset the declaration will have if nothing cancels it (spec_olen).
  int spec_cand = -1;
  uint32_t spec_olen = 0;
  uint32_t totXA = 0, totTA = 0;                   // sums over the A half (carried)

  // Insert a declaration into the LDS table (XCodecMemoryCache::enter,
  // xcodec_cache.h:303-325) -- by lane 0, visible to later LDS reads of the
  // wave (LDS ops of one wave complete in order).
  // (DM) enter into slot sl of the direct-mapped table, whose word s0 the
  // caller has read
  auto insert_dm = [&](uint32_t lo, uint32_t hi, uint32_t c, uint32_t k2, uint32_t sl, uint32_t s0) {
    const uint32_t d = ndecl++, ke = dm_empty<LOGNB>(sl);
    if (l == 0) {
      T.rlo[d] = lo; T.rhi[d] = hi;
      if constexpr (GROUP) { T.rc[d] = (uint32_t)(xin + c); gc->rch[d] = (uint16_t)((xin + c) >> 32); }
      else T.rc[d] = c;
      if (s0 == ke) keyt[sl] = k2;
      else if (novf < (uint32_t)ovf_cap<MAXD, DM>()) T.ovf_k[novf] = k2;
    }
    if (s0 != ke) {
      if (novf < (uint32_t)ovf_cap<MAXD, DM>()) ++novf;
      else if (l == 0 && prm.status) atomicOr(prm.status, 1);
    }
    __builtin_amdgcn_wave_barrier();
  };
  auto insert = [&](uint32_t lo, uint32_t hi, uint32_t c, uint32_t k2) {
    if (DM) {
      const uint32_t sl = (k2 >> 2) & ((2u << LOGNB) - 1u);
      insert_dm(lo, hi, c, k2, sl, readfirst(keyt[sl]));
      return;
    }
    const uint32_t d = ndecl++;
    const uint32_t k = probe_key(lo);
    const uint32_t b = kbucket<LOGNB>(k), ke = kempty<LOGNB>(b);
    const uint32_t s0 = readfirst(keyt[2 * b]), s1 = readfirst(keyt[2 * b + 1]);
    if (l == 0) {
      T.rlo[d] = lo; T.rhi[d] = hi;
      if constexpr (GROUP) { T.rc[d] = (uint32_t)(xin + c); gc->rch[d] = (uint16_t)((xin + c) >> 32); }
      else T.rc[d] = c;
      if (s0 == ke) keyt[2 * b] = k;
      else if (s1 == ke) keyt[2 * b + 1] = k;
      else if (novf < (uint32_t)ovf_cap<MAXD>()) T.ovf_k[novf] = k;
    }
    if (s0 != ke && s1 != ke) {
      if (novf < (uint32_t)ovf_cap<MAXD>()) ++novf;
      else if (STREAM) own_ovf = true;
      else if (l == 0 && prm.status) atomicOr(prm.status, 1);
    }
    __builtin_amdgcn_wave_barrier();
  };

  // Exact lookup: declaration index whose hash is (lo, hi), or -1; or -2 - d
  // when record d matches lo but its hi has not been computed yet.
  auto rec_matches = [&](uint32_t d, uint32_t lo, uint32_t hi, int& found) {
    if (readfirst(T.rlo[d]) != lo) return;
    const uint32_t rh = readfirst(T.rhi[d]);
    if (rh == HI_LAZY) found = -2 - (int)d;
    else if (rh == hi) found = (int)d;
  };
  auto lookup = [&](uint32_t lo, uint32_t hi) -> int {
    // records whose lo matches, by a wave ballot (at most MAXD of them)
    int found = -1;
    for (uint32_t base = 0; base < ndecl && found == -1; base += 64) {
      const uint32_t d = base + (uint32_t)l;
      uint64_t m = ballot(d < ndecl && T.rlo[d] == lo);
      while (m && found == -1) {
        rec_matches(base + (uint32_t)__builtin_ctzll(m), lo, hi, found);
        m &= m - 1;
      }
    }
    return found;
  };

  // Segment bytes of a hash in the persistent cache or, declared by an
  // earlier chunk of the batch, in the batch input (nullptr if neither).
  // A batch hit is recorded: the verification after the round re-parses the
  // chunk if that declaration's visibility or bytes change (xcg_verify_*).
  uint32_t nh = 0;
  // Bounded cache: every reference the chunk makes to the cache, in order --
  // enter (declaration d), lookup hit (XCodecMemoryCache::lookup refreshes the
  // entry's recency whether or not the bytes then match, xcodec_cache.h:348-364),
  // and a lookup of a persistent entry the LRU has evicted by then.  The
  // LRU pass (xcg_lru.hip) derives the eviction times from these.
  uint32_t ne = 0;
  auto record = [&](uint32_t lo, uint32_t hi, uint32_t t, uint32_t kind, uint32_t ref) {
    if (ne < prm.maxe && l == 0) {
      prm.ev[(uint64_t)chunk * prm.maxe + ne] = make_uint4(lo, hi, t, (kind << 30) | ref);
      if (prm.eo) prm.eo[(uint64_t)chunk * prm.maxe + ne] = ~0u;
    }
    ++ne;
  };
  // (after a REF: the output length, at the lookup that made it)
  auto ref_made = [&]() {
    if (LRU && prm.eo && l == 0 && ne > 0 && ne - 1 < prm.maxe) prm.eo[(uint64_t)chunk * prm.maxe + ne - 1] = olen;
  };
  auto cache_src = [&](uint32_t lo, uint32_t hi, int at) -> const uint8_t* {
    uint64_t gv, bv;                               // (both tables probed in one round trip)
    tab_lookup2(prm.g, prm.use_b ? prm.b : prm.g, lo, hi, gv, bv);
    if (gv != ~0ull) {
      if (!LRU) return prm.pool + gv * (uint64_t)SEG;
      const uint32_t t = 2u * (uint32_t)at + 1u;
      if ((((uint64_t)chunk << 21) | t) < prm.ptime[gv]) {
        record(lo, hi, t, EV_GHIT, (uint32_t)gv);
        return prm.pool + gv * (uint64_t)SEG;
      }
      record(lo, hi, t, EV_GMISS, (uint32_t)gv);   // evicted earlier in the batch
    }
    if (prm.use_b) {
      if (bv != ~0ull && (uint32_t)(bv >> 32) < chunk) {
        if (nh < prm.maxh && l == 0) prm.hits[(uint64_t)chunk * prm.maxh + nh] = ((uint64_t)hi << 32) | lo;
        ++nh;
        if (LRU) record(lo, hi, 2u * (uint32_t)at + 1u, EV_HIT, 1u);   // (ref 1: a batch hit, listed in hits)
        return prm.in + prm.chunk_off[bv >> 32] + (uint32_t)bv;
      }
    }
    return nullptr;
  };
  // Could the cache or the batch hold probe key k?  (the LDS lane filter, no
  // false negatives; the global-filter mode goes to the exact tables)
  auto glb_pass = [&](uint32_t k) -> bool {
    if (gs.fmode == 0) return false;
    if (gs.fmode == 2) return true;   // (1 and 3: the LDS filter)
    return readfirst(filt_test(*(const uint32_t*)(gs.lds + gs.lfo + filt_word_ofs(k)), k)) != 0u;
  };
  bool chain = false;                              // the last op was a REF

  // encode_declaration (xcodec_encoder.cc:276-313), made while examining
  // window `at` (the enter precedes that window's lookup).
  auto declare = [&](int at) {
    if (LRU) record(cand_lo, cand_hi, 2u * (uint32_t)at, EV_ENTER, n_extract);
    if (cand > base) olen += escape_u(out + olen, x, (uint32_t)base, (uint32_t)cand);
    if (!nullcache && !c0_in_table) insert(cand_lo, cand_hi, (uint32_t)cand, cand_k);
    if (oob) {
      wave_put_ref(out + olen, cand_lo, cand_hi);           // :288-295
      olen += 10;
    } else {
      if (l < 2) out[olen + l] = (uint8_t)(l == 0 ? MAGIC : OP_EXTRACT);   // :300-302
      if (!(cand == spec_cand && olen == spec_olen)) wave_copy(out + olen + 2, x + cand, SEG);
      olen += 2 + SEG;
    }
    ++n_extract;
    if (STREAM && gs.ro && !nullcache && l == 0 && ndecl > 0) gs.ro[ndecl - 1] = olen;   // (the candidate's record)
    base = cand + SEG;
    have_cand = false;
    c0_in_table = true;
  };

  // ---- Re-parse restart (bounded / pair passes after the first, xcg_lru.hip /
  // xcg_pair.hip).  The previous pass's parse of this chunk stands up to its
  // first lookup the new eviction times contradict (in-chunk time bad_t).
  // Resume at its last clean point before that -- right after a declaration or
  // a REF: parse point = base, nothing pending, about to look that window up
  // (xcodec_encoder.cc:183-208) -- from the state its rows give, and stop as
  // soon as the new parse reaches a clean point the old one also passed
  // through, with the same own declarations as far as the old remainder looks
  // them up: the old remainder is then appended (rows here, output bytes by
  // xcg_splice_kernel after the launch).  The rows of a chunk are in time
  // order, so everything before the restart point is still in place.
  constexpr uint32_t NONE = 0xFFFFFFFFu;
  int rs_q = -1;
  uint32_t rs_hi = 0;                              // in-chunk time of the latest contradicted lookup
  bool spliced = false;
  if (LRU && STREAM && prm.rs.bslot && prm.eo && gs.ro && gs.rsv && !nullcache) {
    const uint32_t rs_slot = readfirst(prm.rs.bslot[chunk]);
    const uint32_t tb = readfirst(prm.rs.bad_t[chunk]);
    rs_hi = readfirst(prm.rs.bad_hi[chunk]);
    if (rs_slot != NONE && tb != NONE) {
      const uint4* const odl = prm.decl + (uint64_t)chunk * prm.maxd;   // old rows (in place until the end)
      const uint4* oev = prm.rs.b_ev + (uint64_t)rs_slot * prm.maxe;
      const uint32_t* oeo = prm.rs.b_eo + (uint64_t)rs_slot * prm.maxe;
      const uint32_t o_nev = min(readfirst(prm.rs.b_cnt[4 * rs_slot]), prm.maxe);
      const uint32_t o_nd = readfirst(prm.rs.b_cnt[4 * rs_slot + 3]);
      // the latest clean point q (a window, <= last) with 2q + 1 <= tb
      int best = -1;
      uint32_t best_olen = 0;
      for (uint32_t i0 = 0; i0 < o_nev; i0 += 64) {
        const uint32_t i = i0 + (uint32_t)l;
        int q = -1;
        uint32_t ol = 0;
        if (i < o_nev) {
          const uint4 e = oev[i];
          if ((e.w >> 30) == EV_ENTER) {               // declared while examining window e.z / 2
            const uint32_t d = e.w & EV_REF_MASK;
            if (d < o_nd) { q = (int)(e.z >> 1); ol = odl[d].w; }
          } else if (oeo[i] != NONE) {                  // a REF at window (e.z - 1) / 2
            q = (int)((e.z - 1u) >> 1) + SEG;
            ol = oeo[i];
          }
          if (q > last || (q >= 0 && 2u * (uint32_t)q + 1u > tb)) q = -1;
        }
        int mq = q;
        for (int off = 32; off >= 1; off >>= 1) mq = max(mq, __shfl_xor(mq, off));
        mq = readfirst(mq);
        if (mq > best) {
          const uint64_t bl = ballot(q == mq);
          best = mq;
          best_olen = readlane(ol, (int)__builtin_ctzll(bl));
        }
      }
      if (best >= 0) {
        rs_q = best;
        uint32_t ne_r = 0, nd_r = 0, nh_r = 0, nref_r = 0;
        for (uint32_t i0 = 0; i0 < o_nev; i0 += 64) {
          const uint32_t i = i0 + (uint32_t)l;
          bool in = false, ent = false, bh = false, rf = false;
          if (i < o_nev) {
            const uint4 e = oev[i];
            in = e.z < 2u * (uint32_t)best + 1u;
            ent = in && (e.w >> 30) == EV_ENTER;
            bh = in && (e.w >> 30) == EV_HIT && (e.w & EV_REF_MASK) == 1u;
            rf = in && oeo[i] != NONE;
          }
          ne_r += (uint32_t)__builtin_popcountll(ballot(in));
          nd_r += (uint32_t)__builtin_popcountll(ballot(ent));
          nh_r += (uint32_t)__builtin_popcountll(ballot(bh));
          nref_r += (uint32_t)__builtin_popcountll(ballot(rf));
        }
        for (uint32_t d = 0; d < nd_r; ++d) {           // the own records and key table so far
          const uint4 r = odl[d];
          insert(readfirst(r.x), readfirst(r.y), readfirst(r.z), 0u);   // (stream: keyed by lo)
          if (l == 0) gs.ro[d] = r.w;
        }
        if (l == 0) {
          gs.rsv[0] = rs_slot;
          gs.rsv[1] = o_nev;
          gs.rsv[2] = readfirst(prm.rs.b_cnt[4 * rs_slot + 1]);
          gs.rsv[3] = readfirst(prm.rs.b_cnt[4 * rs_slot + 2]);
          gs.rsv[4] = o_nd;
          gs.rsv[5] = nd_r;
        }
        __builtin_amdgcn_wave_barrier();
        ne = ne_r;
        nh = nh_r;
        olen = best_olen;
        n_extract = nd_r;
        n_ref = nref_r;
        s = base = best;
        chain = true;
      }
    }
  }
  // Splice at clean point s (the new parse is about to look window s up, with
  // nothing pending): true when the old parse had the same state there.
  auto try_splice = [&]() -> bool {
    const uint32_t rs_slot = readfirst(gs.rsv[0]), o_nev = readfirst(gs.rsv[1]), o_nh = readfirst(gs.rsv[2]);
    const uint32_t o_olen = readfirst(gs.rsv[3]), o_nd = readfirst(gs.rsv[4]), rs_nd = readfirst(gs.rsv[5]);
    const uint4* const odl = prm.decl + (uint64_t)chunk * prm.maxd;
    const uint4* const oev = prm.rs.b_ev + (uint64_t)rs_slot * prm.maxe;
    const uint32_t* const oeo = prm.rs.b_eo + (uint64_t)rs_slot * prm.maxe;
    // the old clean point at s: a declaration made at window s, or a REF at s - 2048
    int it = -1, dt = -1;
    uint32_t ol_old = 0;
    for (uint32_t i0 = 0; i0 < o_nev && it < 0; i0 += 64) {
      const uint32_t i = i0 + (uint32_t)l;
      bool hit = false;
      if (i < o_nev) {
        const uint4 e = oev[i];
        hit = ((e.w >> 30) == EV_ENTER && e.z == 2u * (uint32_t)s) ||
              (oeo[i] != NONE && s >= SEG && e.z == 2u * (uint32_t)(s - SEG) + 1u);
      }
      const uint64_t bl = ballot(hit);
      if (bl) it = (int)(i0 + (uint32_t)__builtin_ctzll(bl));
    }
    if (it < 0) return false;
    {
      const uint4 e = oev[it];
      if ((e.w >> 30) == EV_ENTER) {
        dt = (int)(e.w & EV_REF_MASK) + 1;
        ol_old = readfirst(odl[dt - 1].w);
      } else {
        ol_old = readfirst(oeo[it]);
        uint32_t c = 0;                                  // declarations before the REF
        for (uint32_t i0 = 0; i0 < (uint32_t)it; i0 += 64) {
          const uint32_t i = i0 + (uint32_t)l;
          c += (uint32_t)__builtin_popcountll(ballot(i < (uint32_t)it && (oev[i].w >> 30) == EV_ENTER));
        }
        dt = (int)c;
      }
    }
    ++it;                                                // the old remainder's first reference
    if ((uint32_t)dt < rs_nd || (uint32_t)dt > o_nd) return false;
    // own declarations that differ: the new ones since the restart vs the old ones
    const uint32_t nn = ndecl - rs_nd, no = (uint32_t)dt - rs_nd;
    if (nn > 32 || no > 32) return false;
    uint32_t hlo = 0, hhi = 0;
    if ((uint32_t)l < nn) { hlo = T.rlo[rs_nd + l]; hhi = T.rhi[rs_nd + l]; }
    else if ((uint32_t)l >= 32 && (uint32_t)l - 32 < no) { const uint4 r = odl[rs_nd + l - 32]; hlo = r.x; hhi = r.y; }
    const bool is_new = (uint32_t)l < nn, is_old = (uint32_t)l >= 32 && (uint32_t)l - 32 < no;
    bool inD = is_new || is_old;
    for (uint32_t j = 0; j < (nn > no ? nn : no); ++j) {   // (uniform: readlane of lanes j and 32 + j)
      const uint32_t nlo = readlane(hlo, (int)j), nhi = readlane(hhi, (int)j);
      const uint32_t olo = readlane(hlo, (int)(32 + j)), ohi = readlane(hhi, (int)(32 + j));
      if (is_old && j < nn && hlo == nlo && hhi == nhi) inD = false;
      if (is_new && j < no && hlo == olo && hhi == ohi) inD = false;
    }
    const uint64_t dm = ballot(inD);
    // The old remainder's lookups of these are in its rows only where the old
    // parse found the hash: as its own record (the old ones), in the
    // persistent table, or in the batch table visible to this chunk.  A new
    // declaration found nowhere else may have been missed there unrecorded
    // (an in-chunk repeat): no splice then.
    bool unknown = false;
    if (is_new && inD) {
      bool known = tab_lookup_t(prm.g, hlo, hhi) != ~0ull;
      if (!known && prm.use_b) {
        const uint64_t bv = tab_lookup_t(prm.b, hlo, hhi);
        known = bv != ~0ull && (uint32_t)(bv >> 32) < chunk;
      }
      unknown = !known;
    }
    if (ballot(unknown)) return false;
    // the old remainder must not look any of them up (or declare one)
    for (uint32_t i0 = (uint32_t)it; i0 < o_nev; i0 += 64) {
      const uint32_t i = i0 + (uint32_t)l;
      const uint4 e = i < o_nev ? oev[i] : make_uint4(0u, 0u, 0u, 0u);
      bool clash = false;
      uint64_t m = dm;
      while (m) {
        const int j = __builtin_ctzll(m);
        m &= m - 1;
        clash |= i < o_nev && e.x == (uint32_t)readlane(hlo, j) && e.y == (uint32_t)readlane(hhi, j);
      }
      if (ballot(clash)) return false;
    }
    // splice: the old remainder's declarations, references and batch hits follow
    const uint32_t delta = olen - ol_old;                // (mod 2^32: offsets shift by it)
    const uint32_t nd0 = ndecl;
    for (uint32_t d = (uint32_t)dt; d < o_nd && ndecl < (uint32_t)MAXD; ++d) {
      const uint4 r = odl[d];
      if (l == 0) {
        T.rlo[ndecl] = r.x; T.rhi[ndecl] = r.y; T.rc[ndecl] = r.z;
        gs.ro[ndecl] = r.w + delta;
      }
      ++ndecl;
    }
    uint32_t hb = 0;                                     // batch hits before the old remainder
    for (uint32_t i0 = 0; i0 < (uint32_t)it; i0 += 64) {
      const uint32_t i = i0 + (uint32_t)l;
      hb += (uint32_t)__builtin_popcountll(
          ballot(i < (uint32_t)it && (oev[i].w >> 30) == EV_HIT && (oev[i].w & EV_REF_MASK) == 1u));
    }
    uint32_t nref_t = 0;
    for (uint32_t i0 = (uint32_t)it; i0 < o_nev; i0 += 64) {
      const uint32_t i = i0 + (uint32_t)l;
      if (i < o_nev) {
        uint4 e = oev[i];
        if ((e.w >> 30) == EV_ENTER) e.w = (EV_ENTER << 30) | ((e.w & EV_REF_MASK) - (uint32_t)dt + nd0);
        const uint32_t o = oeo[i];
        const uint32_t k = ne + (i - (uint32_t)it);
        if (k < prm.maxe) {
          prm.ev[(uint64_t)chunk * prm.maxe + k] = e;
          prm.eo[(uint64_t)chunk * prm.maxe + k] = o == NONE ? NONE : o + delta;
        }
      }
      nref_t += (uint32_t)__builtin_popcountll(ballot(i < o_nev && oeo[i] != NONE));
    }
    ne += o_nev - (uint32_t)it;
    const uint64_t* oh = prm.rs.b_hits + (uint64_t)rs_slot * prm.maxh;
    for (uint32_t j = hb + (uint32_t)l; j < o_nh && j < prm.maxh; j += 64) {
      const uint32_t k = nh + (j - hb);
      if (k < prm.maxh) prm.hits[(uint64_t)chunk * prm.maxh + k] = oh[j];
    }
    nh += o_nh > hb ? o_nh - hb : 0u;
    n_ref += nref_t;
    n_extract += o_nd - (uint32_t)dt;
    if (l == 0) prm.rs.splice[chunk] = make_uint4(olen, ol_old, o_olen, 1u);
    olen += o_olen - ol_old;
    return true;
  };

  while (s <= last) {
    clk.piece_begin();
    // ---- piece geometry: q0 = p + 32 lane, loads 16-byte aligned in memory
    const int p = s - (int)(((uint32_t)mis + (uint32_t)s) & 15u);
    const int l = opaque(lane_id());
    const int q0 = p + 32 * l;
    const bool contig = (p == p_prev + SEG);
    ++n_pieces;
    if constexpr (GROUP) progress_priority(gc->done + s, gc->total);   // the wave's whole job: its group
    else progress_priority(s, L);
    // vmcnt counts loads and stores together, in order (gfx9): every wait on
    // a load also waits for all older stores.  So fresh loads are waited for
    // here, inside their branch, and the prefetch below is waited for after
    // the vector phase -- never right behind its own issue.
    // (contig implies nb_start == p: the previous piece prefetched this B.)
    if constexpr (DM) {
      const bool counted = rg_steady == 3u;
      rg_steady = (rg_steady << 1) & 2u;
      // (each register load is waited for in the branch that issued it: a
      // wait the compiler places later would drain the ring loads too)
      if (!contig) {
        // first piece, or after a jump: the register path
        P.a0 = piece_ld_safe<STREAM>(x, q0, L);
        P.a1 = piece_ld_safe<STREAM>(x, q0 + 16, L);
        P.b0 = piece_ld_safe<STREAM>(x, q0 + SEG, L);
        P.b1 = piece_ld_safe<STREAM>(x, q0 + SEG + 16, L);
        vuse(P.a0); vuse(P.a1); vuse(P.b0); vuse(P.b1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (nothing of the ring in flight when it is primed again)
        seg_sums(P.a0, P.a1, P.sxa, P.sqxa);
        rg_n = 0;
      } else {
        P.a0 = P.b0; P.a1 = P.b1;
        P.sxa = P.sxb; P.sqxa = P.sqxb;
        if (rg_n > 0) {
          // This piece's ring load was issued two pieces ago.  In the quiet
          // steady state exactly eight vector memory operations are younger:
          // the two pieces' three stores each (header, two body halves), and
          // the two loads the previous piece issued.  vmcnt retires in order,
          // so everything else stays in flight.  Any other history: wait for all.
          if (counted) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
          else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          const lds_u8* rb = ring + ((((uint32_t)p >> 11) & 1u) << 11) + 32 * l;
          P.b0 = *(const volatile lds_u32x4*)rb;
          P.b1 = *(const volatile lds_u32x4*)(rb + 16);
          --rg_n;
        } else {
          // a B half that reaches past the chunk (the guarded tail)
          P.b0 = piece_ld_safe<STREAM>(x, q0 + SEG, L);
          P.b1 = piece_ld_safe<STREAM>(x, q0 + SEG + 16, L);
          vuse(P.b0); vuse(P.b1);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
      }
      // Fill the ring up to two pieces ahead, with loads that lie wholly
      // inside the chunk (x + p is 16-byte aligned).  The buffer refilled in
      // the steady state is the one just read: its reads return first.
      const uint32_t ring_a = (uint32_t)(uintptr_t)ring;
      const uint8_t* src = x + p + 16 * l;
      if (rg_n == 0 && p + 3 * SEG <= L) {
        ring_load(src + 2 * SEG, ring_a + (((((uint32_t)p >> 11) & 1u) ^ 1u) << 11));
        rg_n = 1;
      }
      if (rg_n == 1 && p + 4 * SEG <= L) {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(P.b0), "+v"(P.b1)::"memory");
        ring_load(src + 3 * SEG, ring_a + ((((uint32_t)p >> 11) & 1u) << 11));
        rg_n = 2;
      }
    } else if (contig) {
      P.a0 = P.b0; P.a1 = P.b1;
      P.sxa = P.sxb; P.sqxa = P.sqxb;
      P.b0 = nb0; P.b1 = nb1;
    } else {
      P.a0 = piece_ld_safe<STREAM>(x, q0, L);
      P.a1 = piece_ld_safe<STREAM>(x, q0 + 16, L);
      P.b0 = piece_ld_safe<STREAM>(x, q0 + SEG, L);
      P.b1 = piece_ld_safe<STREAM>(x, q0 + SEG + 16, L);
      vuse(P.a0); vuse(P.a1); vuse(P.b0); vuse(P.b1);
      seg_sums(P.a0, P.a1, P.sxa, P.sqxa);
    }
    seg_sums(P.b0, P.b1, P.sxb, P.sqxb);
    p_prev = p;

    // ---- start sums of lane l's first window (positions relative to p)
    const uint32_t qa = 32u * (uint32_t)l, qb = 2048u + 32u * (uint32_t)l;
    const uint32_t ta = qa * P.sxa + P.sqxa, tb = qb * P.sxb + P.sqxb;
    if (!contig) {
      totXA = wave_sum(P.sxa); totTA = wave_sum(ta);
    }
    const uint32_t dx = P.sxb - P.sxa, dt = tb - ta;
    const uint32_t ix = wave_incl_scan(dx), it = wave_incl_scan(dt);
    const uint32_t X1 = totXA + ix - dx;
    const uint32_t TT = totTA + it - dt;
    const uint32_t X2c = (2048u + qa) * X1 - TT + CLO;
    // Next piece's A half (if contiguous) is this B half, shifted by 2048.
    const uint32_t totXB = totXA + readlane(ix, 63);
    const uint32_t totTB = totTA + readlane(it, 63) - 2048u * totXB;
    // probe key of the lane's first window
    const uint32_t NX1 = 0u - X1, NX2 = 0u - X2c;
    const uint32_t k0 = (NX1 << 20) + NX2;

    // Prefetch the next contiguous piece's entering bytes; they land while
    // this piece rolls (issued after every use of this piece's loads).
    nb_start = p + SEG;
    if (!DM && nb_start < last) {                           // (nb_start == last: decided as this piece's tail1 window)
      if (p + 3 * SEG <= L) {                      // (uniform) every lane's 32 bytes inside the chunk: no guards
        nb0 = piece_ld<STREAM>(x + q0 + 2 * SEG);
        nb1 = piece_ld<STREAM>(x + q0 + 2 * SEG + 16);
      } else {
        nb0 = piece_ld_safe<STREAM>(x, q0 + 2 * SEG, L);
        nb1 = piece_ld_safe<STREAM>(x, q0 + 2 * SEG + 16, L);
      }
    }

    // ---- REF chaining (stream semantics).  The previous piece ended with a
    // REF, so this piece starts at the parse point with no candidate pending;
    // in REF-dense streams (warm caches, duplicated runs) the window there is
    // usually the next REF.  Probe it exactly (lookup, find_reference
    // xcodec_encoder.cc:374-416) before rolling 2048 positions; a miss goes
    // through the filters only, and a miss or a collision falls through to
    // the ordinary vector phase, which decides position s itself.
    // The same holds right after a declaration: a candidate that survived its
    // 2048 windows is declared here, at window s = cand + 2048, before that
    // window's lookup (:183-196) -- and when the data repeats in 2 KiB blocks
    // the window at the end of a new block is often the next REF.
    int chain_miss = -1;
    if (STREAM && !nullcache && !chain && have_cand && cand + SEG == s) {
      declare(s);
      chain = true;
    }
    // a clean point past every contradicted lookup: rejoin the old parse?
    if (LRU && rs_q >= 0 && chain && s > rs_q && 2u * (uint32_t)s + 1u > rs_hi && try_splice()) {
      spliced = true;
      break;
    }
    if (STREAM && chain && !nullcache) {
      clk.chain_begin();
      chain = false;
      uint32_t lo, hi;
      if (s == p) {
        lo = 0u - readfirst(k0);
        hi = readfirst(lane_window_hi(P, 0));
      } else {
        const uint3 h = window_hash_u(x + s);
        lo = h.x; hi = h.y;
      }
      const int d = lookup(lo, hi);                 // stream records carry their hi
      const uint8_t* src = d >= 0 ? x + readfirst(T.rc[d]) : nullptr;
      if (LRU && d >= 0) record(lo, hi, 2u * (uint32_t)s + 1u, EV_HIT, 0u);
      // (straight to the exact tables after the LDS lane filter: a chain probe
      // hits often, and both tables cost one round trip together)
      if (src == nullptr && glb_pass(probe_key(lo))) src = cache_src(lo, hi, s);
      if (src != nullptr && (s == p ? equal2048_regs(src, P.a0, P.a1) : equal2048_u(src, x + s))) {
        wave_put_ref(out + olen, lo, hi);           // encode_reference :342-372
        olen += 10;
        ref_made();
        ++n_ref;
        base = s + SEG;
        s = base;
        chain = true;
        totXA = totXB; totTA = totTB;               // (as at the end of a piece)
        clk.chain_end();
        continue;
      }
      if (src == nullptr) chain_miss = s;          // an exact miss: the vector phase's event at s is moot
      clk.chain_end();
    }

    // ---- vector phase
    clk.vector_begin();
    uint32_t ev = 0;
    bool quiet = false;                            // (DM) no lane has a possible hit in this piece
    const int pe = min(p + SEG, last + 1);         // piece end (exclusive)
    if (!nullcache) {
      // c0 = the pending candidate; once it is visible from the piece start on,
      // it goes straight into the table (a REF can no longer cancel it).
      if (have_cand && !c0_in_table && cand + SEG <= p) {
        insert(cand_lo, cand_hi, (uint32_t)cand, cand_k);
        c0_in_table = true;
      }
      if (pe - s <= 2) {
        // One or two positions left (every chunk of 2048 k bytes ends with a
        // one-position piece): decide them exactly, as events, instead of
        // rolling 2048 positions for them.
        ev = lane_id() == 0 ? ((1u << (uint32_t)(pe - s)) - 1u) << (uint32_t)(s - p) : 0u;
      } else {
        const bool c0 = have_cand && !c0_in_table;
        const int vis = cand + SEG;
        const int rvis = vis - p;
        const uint32_t c0k = DM ? cand_k : probe_key(cand_lo);
        // Bucket overflows are rare (three of a chunk's keys in one 2-slot
        // bucket); one overflow key costs one compare, more cost eight (32
        // beyond eight, in frames of up to 512 KiB).
        constexpr int OC = ovf_cap<MAXD, DM>();
        uint32_t ovk[OC];
  #pragma unroll
        for (int k = 0; k < (DM ? 1 : OC); ++k) ovk[k] = novf ? readfirst(T.ovf_k[(uint32_t)k < novf ? k : 0]) : 0u;
        const uint32_t sa0 = gs.sofs + 4u * (uint32_t)lane_id();
        GlbQ gq{gs.lds, gs.lfo, prm.lf.gfilt, prm.lf.gmask, prm.lf.ftab, prm.lf.fmask, sa0, sa0, sa0 + 256u * GSLOTS,
                0u, 0u};
        // G = probe the persistent cache / batch declarations too
        auto roll = [&](auto c0t, auto novft, auto glbt) {
          return roll_probe<LOGNB, decltype(c0t)::value, decltype(novft)::value, decltype(glbt)::value>(
              P, NX1, NX2, kblk, kofs, c0k, rvis, ovk, gq);
        };
        using T0 = std::integral_constant<bool, false>;
        using T1 = std::integral_constant<bool, true>;
        using N0 = std::integral_constant<int, 0>;
        using N1 = std::integral_constant<int, 1>;
        using N8 = std::integral_constant<int, 8>;
        using NC = std::integral_constant<int, OC>;
        auto by_novf = [&](auto glbt) {
          if (novf == 0) return c0 ? roll(T1{}, N0{}, glbt) : roll(T0{}, N0{}, glbt);
          if (novf == 1) return c0 ? roll(T1{}, N1{}, glbt) : roll(T0{}, N1{}, glbt);
          // duplicates of a real overflow key pad the unused slots
          if (OC == 8 || novf <= 8) return c0 ? roll(T1{}, N8{}, glbt) : roll(T0{}, N8{}, glbt);
          return c0 ? roll(T1{}, NC{}, glbt) : roll(T0{}, NC{}, glbt);
        };
        if constexpr (DM) {
          // the lane mask of possible hits first; the event word only if any
          auto rolld = [&](auto c0t, auto novft, auto evwt) -> uint64_t {
            return roll_probe_dm<LOGNB, decltype(c0t)::value, decltype(novft)::value, decltype(evwt)::value>(
                P, NX1, NX2, kblk, kofs, c0k, rvis, T.ovf_k, novf);
          };
          auto by_novf_dm = [&](auto evwt) -> uint64_t {
            if (novf == 0) return rolld(T0{}, N0{}, evwt);
            if (novf == 1) return rolld(T0{}, N1{}, evwt);
            return rolld(T0{}, N8{}, evwt);
          };
          if (c0 || novf > 8) {   // (rare: the event word straight away)
            if (novf == 0) ev = (uint32_t)rolld(T1{}, N0{}, T1{});
            else if (novf == 1) ev = (uint32_t)rolld(T1{}, N1{}, T1{});
            else if (novf <= 8) ev = (uint32_t)rolld(T1{}, N8{}, T1{});
            else ev = (uint32_t)(c0 ? rolld(T1{}, NC{}, T1{}) : rolld(T0{}, NC{}, T1{}));
          } else {
            quiet = by_novf_dm(T0{}) == 0;
            ev = quiet ? 0u : (uint32_t)by_novf_dm(T1{});
          }
        } else if (STREAM && gs.fmode == 1) {
          ev = by_novf(std::integral_constant<int, STREAM ? 1 : 0>{});
        } else if (STREAM && gs.fmode == 2) {
          ev = by_novf(std::integral_constant<int, STREAM ? 2 : 0>{});
        } else if (STREAM && gs.fmode == 3) {
          ev = by_novf(std::integral_constant<int, STREAM ? 3 : 0>{});
        } else {
          ev = by_novf(std::integral_constant<int, 0>{});
        }
        // positions past the last window are not positions (branch-free mask)
        const int nvalid = pe - q0;
        const uint32_t vm = nvalid >= 32 ? 0xFFFFFFFFu : ((1u << (uint32_t)max(nvalid, 0)) - 1u);
        ev &= vm;
        if (STREAM && chain_miss >= 0) {         // (chain_miss == s: decided by the chain probe)
          const int rel = chain_miss - p;
          if (lane_id() == (rel >> 5)) ev &= ~(1u << (rel & 31));
        }
      }
    }
    // The prefetch has had the vector phase to land; take it before the
    // resolve phase issues this piece's stores.
    clk.wait_begin();
    if constexpr (!DM) {
      vuse(nb0); vuse(nb1);                        // (unconditional: so the compiler sees them waited)
    }
    clk.wait_end();
    clk.vector_end();

    // ---- resolve phase (wave-uniform)
    // A chunk whose last window is one past a full piece (every chunk of
    // 2048 k + 2048 bytes: C2's 64 KiB, C4's 4 KiB) decides that window here,
    // as an event (hashed by the one window-hash call site), instead of in a
    // piece of its own.
    const bool tail1 = pe == p + SEG && last == pe;
    const int pe_x = tail1 ? pe + 1 : pe;
    auto next_event = [&](int from) -> int {
      if (tail1 && from == pe) return from;
      const int rel = from - p;
      const int ls = rel >> 5, bs = rel & 31;
      uint32_t m = l < ls ? 0u : (l == ls ? (ev & (0xFFFFFFFFu << bs)) : ev);
      const uint64_t bal = ballot(m != 0u);
      if (bal == 0) return INT32_MAX;
      const int lw = __builtin_ctzll(bal);
      const uint32_t mm = readlane(m, lw);
      return p + 32 * lw + __builtin_ctz(mm);
    };
    auto hash_at = [&](int pos, uint32_t& lo, uint32_t& hi, uint32_t& k2) {
      const int rel = pos - p;
      if ((rel & 31) == 0 && rel < SEG) {
        lo = 0u - readlane(k0, rel >> 5);
        hi = lazy_hi ? HI_LAZY : readfirst(lane_window_hi(P, rel >> 5));
        k2 = DM ? readlane(NX2, rel >> 5) : 0u;
      } else {
        const uint3 h = window_hash_u(x + pos);
        lo = h.x; hi = h.y; k2 = h.z;
      }
    };

    // Independent chunks' steady state: the candidate set at the previous
    // piece's start is declared here (its key went into the table before the
    // vector phase, its body was stored from registers), nothing matched, and
    // the next candidate is this piece's first window -- the resolve loop
    // below would do exactly this, through two event searches.
    // The new candidate can no longer be cancelled: positions before its
    // declaration point (the next piece's start) are all in this quiet piece.
    // So it enters the table now (XCodecMemoryCache::enter at its declaration,
    // visible from the next piece on), its slot read overlapping the stores.
    if (DM && quiet && !oob && !nullcache && have_cand && c0_in_table && cand + SEG == s && s == p && base == cand &&
        spec_cand == cand && spec_olen == olen && pe == p + SEG) {
      const uint32_t k2 = readlane(NX2, 0);
      const uint32_t sl = (k2 >> 2) & ((2u << LOGNB) - 1u);
      const uint32_t s0v = keyt[sl];
      if (l < 2) out[olen + l] = (uint8_t)(l == 0 ? MAGIC : OP_EXTRACT);   // encode_declaration :300-302
      olen += 2 + SEG;
      ++n_extract;
      base = s;
      cand = s;                                     // :246-248, the hash from registers
      cand_lo = 0u - readlane(k0, 0);
      cand_hi = lazy_hi ? HI_LAZY : readfirst(lane_window_hi(P, 0));
      cand_k = k2;
      uint8_t* dst = out + olen + 2 + 32 * lane_id();
      *(u32x4_u*)dst = P.a0;
      *(u32x4_u*)(dst + 16) = P.a1;
      spec_cand = s;
      spec_olen = olen;
      s = pe;
      insert_dm(cand_lo, cand_hi, (uint32_t)cand, k2, sl, readfirst(s0v));   // (its slot already read)
      c0_in_table = true;
      if (rg_n == 2) rg_steady |= 1u;               // (rg_n == 2: this piece issued the load two pieces ahead)
    }
    while (s < pe_x) {
      if (have_cand && cand + SEG <= s) declare(s);           // :183-190
      const int e = nullcache ? INT32_MAX : next_event(s);
      if (e == s) {
        const WaveClock::Event clk_event(clk);
        // Exact re-check of the probe (find_reference, :374-416).  A record
        // still missing its hi gets it from the same (single) hash call site,
        // then the window is hashed again.
        uint32_t lo = 0, hi = 0;
        int d = -1, fill = -1;
        uint3 hh;
        for (;;) {
          if (fill < 0 && ((s - p) & 31) == 0 && s - p < SEG) {   // a lane's first window: the hash from registers
            hh.x = 0u - readlane(k0, (s - p) >> 5);
            hh.y = readfirst(lane_window_hi(P, (s - p) >> 5));
            hh.z = DM ? readlane(NX2, (s - p) >> 5) : 0u;
          } else {
            hh = window_hash_u(fill >= 0 ? rec_bytes((uint32_t)fill) : x + s);
          }
          if (fill >= 0) {
            if (l == 0) T.rhi[fill] = hh.y;
            __builtin_amdgcn_wave_barrier();
            fill = -1;
            continue;
          }
          lo = hh.x; hi = hh.y;
          d = lookup(lo, hi);
          if (d >= -1) break;
          fill = -2 - d;
        }
        // Where the hash is declared: this chunk (d), the persistent cache, or
        // an earlier chunk of the batch.  src = that segment's bytes.
        const uint8_t* src = d >= 0 ? rec_bytes((uint32_t)d) : nullptr;
        if (LRU && d >= 0) record(lo, hi, 2u * (uint32_t)s + 1u, EV_HIT, 0u);
        // (through the lane filter first: the forced events of a chunk's last
        // one or two windows and own-table false positives have not passed it)
        if (STREAM && src == nullptr && glb_pass(probe_key(lo))) src = cache_src(lo, hi, s);
        if (src != nullptr) {
          if (s == p ? equal2048_regs(src, P.a0, P.a1) : equal2048_u(src, x + s)) {
            if (spec_cand >= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // speculative body lands first
            if (s > base) olen += escape_u(out + olen, x, (uint32_t)base, (uint32_t)s);
            wave_put_ref(out + olen, lo, hi);                 // encode_reference :342-372
            olen += 10;
            ref_made();
            ++n_ref;
            base = s + SEG;
            s = base;
            have_cand = false;                                // :208
            c0_in_table = true;
            chain = true;
            continue;
          }
          ++n_coll;                                           // collision, :390-406 / :215-216
          ++s;
          continue;
        }
        // fingerprint false positive: an ordinary miss
        if (!have_cand) {
          have_cand = true; cand = s; cand_lo = lo; cand_hi = hi; cand_k = hh.z; c0_in_table = false;
        }
        ++s;
        continue;
      }
      if (!have_cand) {                                       // :246-248
        hash_at(s, cand_lo, cand_hi, cand_k);
        have_cand = true;
        cand = s;
        c0_in_table = false;
        if (s == p && base == s && !oob) {
          // Declaration body = bytes [p, p + 2048) = the A registers.
          uint8_t* dst = out + olen + 2 + 32 * lane_id();
          *(u32x4_u*)dst = P.a0;
          *(u32x4_u*)(dst + 16) = P.a1;
          spec_cand = s;
          spec_olen = olen;
        }
        ++s;
        continue;
      }
      // Non-event positions before the next milestone change nothing.
      s = min(min(e, cand + SEG), pe);
    }
    // The table holds every declaration once the piece is done; a still
    // pending candidate stays out of it until declared.
    totXA = totXB; totTA = totTB;
  }
  // (an input ring load still in flight lands in this wave's LDS before the wave ends)
  if constexpr (DM) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  if (!spliced) {
    if (have_cand) declare(last + 1);                         // :257-261 (after every lookup)
    if (base < L) olen += escape_u(out + olen, x, (uint32_t)base, (uint32_t)L);   // :267-269
  }
  if constexpr (GROUP) { gc->ndecl = ndecl; gc->novf = novf; }   // (every candidate is declared by now)
  if (STREAM) {
    // This round's declarations; flag a change against the previous round's.
    const uint32_t nold = prm.ndecl[chunk];
    bool diff = nold != ndecl;
    uint4* dl = prm.decl + (uint64_t)chunk * prm.maxd;
    for (uint32_t k = l; k < ndecl; k += 64) {
      const uint4 nv = make_uint4(T.rlo[k], T.rhi[k], T.rc[k], gs.ro ? gs.ro[k] : 0u);
      if (k < nold) {
        const uint4 ov = dl[k];
        diff |= ov.x != nv.x || ov.y != nv.y || ov.z != nv.z;
      }
      dl[k] = nv;
    }
    if (ballot(diff) != 0 && l == 0) atomicMin(prm.changed, chunk);
    if (l == 0) {
      prm.ndecl[chunk] = ndecl;
      prm.nhits[chunk] = own_ovf ? prm.maxh + 1u : nh;
      if (LRU) prm.nev[chunk] = ne;
    }
  }
  if (l == 0) {
    prm.out_len[chunk] = olen;
    if (prm.stats) {
      if constexpr (WaveClock::ON) {
        clk.store(prm.stats, chunk, n_pieces);
      } else {
        prm.stats[4 * chunk + 0] = n_extract;
        prm.stats[4 * chunk + 1] = n_ref;
        prm.stats[4 * chunk + 2] = n_coll;
        prm.stats[4 * chunk + 3] = n_pieces;
      }
    }
  }
  if constexpr (GROUP) __builtin_amdgcn_wave_barrier();   // (as at the early exit)
}

}  // namespace xcg
