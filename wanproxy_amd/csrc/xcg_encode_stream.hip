// XCodec encoder, stream semantics: the parse kernel's plain instances, the
// kernels of the rounds around it and the round driver xcg_launch_encode_stream.
#include <stdio.h>
#include <stdlib.h>

#include <mutex>
#include <utility>
#include <vector>

#include "xcg_encode_stream.h"

// ---- the driver's knobs: all it reads from the environment, and their xcg_debug_* setters

// LDS / global lane filter threshold (keys): XCG_LDS_FILTER_KEYS at load
// time, or xcg_debug_set_lds_filter_keys (tests force either mode with it).
// Default (LFK_AUTO): per cache -- LDS_FILTER_KEYS_DEFAULT while its fingerprint
// buckets fit 2 MiB of L2, else 0: with a larger bucket table (unbounded caches
// of 2^19+ segments, pairs) an LDS-filter pass costs fewer HBM misses as a
// probe of the L2-resident global filter than as a bucket load (C5 308 -> 316
// GiB/s; C2-S2 and the LRU cache, 2 MiB of buckets, lose with 0:
// profiles/r06_s3_lfk.txt).
constexpr uint32_t LFK_AUTO = ~0u;
static uint32_t g_lds_filter_keys = [] {
  const char* e = getenv("XCG_LDS_FILTER_KEYS");
  return e ? (uint32_t)strtoul(e, nullptr, 10) : LFK_AUTO;
}();
static uint32_t xcg_lds_filter_keys() { return __atomic_load_n(&g_lds_filter_keys, __ATOMIC_RELAXED); }
extern "C" uint32_t xcg_debug_set_lds_filter_keys(uint32_t keys) {
  return __atomic_exchange_n(&g_lds_filter_keys, keys, __ATOMIC_RELAXED);
}
// Past that, the LDS filter still screens the global one's loads up to this
// many keys (XCG_LDS_PREFILTER_KEYS, xcg_debug_set_lds_prefilter_keys).
static uint32_t g_lds_prefilter_keys = [] {
  const char* e = getenv("XCG_LDS_PREFILTER_KEYS");
  return e ? (uint32_t)strtoul(e, nullptr, 10) : xcg::LDS_PREFILTER_KEYS_DEFAULT;
}();
extern "C" uint32_t xcg_debug_set_lds_prefilter_keys(uint32_t keys) {
  return __atomic_exchange_n(&g_lds_prefilter_keys, keys, __ATOMIC_RELAXED);
}

// The quiet-chunk screen on (default) / off: XCG_SCREEN=0, or
// xcg_debug_set_screen (tests run both ways).
static int g_screen = [] {
  const char* e = getenv("XCG_SCREEN");
  return e ? atoi(e) : 1;
}();
static bool xcg_screen_on() { return __atomic_load_n(&g_screen, __ATOMIC_RELAXED) != 0; }
// (2: on, and count what the screen sees -- a host sync per screened launch)
static bool xcg_screen_counting() { return __atomic_load_n(&g_screen, __ATOMIC_RELAXED) == 2; }
extern "C" int xcg_debug_set_screen(int mode) {
  return __atomic_exchange_n(&g_screen, mode < 0 ? 0 : (mode > 2 ? 2 : mode), __ATOMIC_RELAXED);
}
static uint64_t g_screen_seen = 0, g_screen_parsed = 0;
extern "C" int xcg_debug_screen_counts(uint64_t* seen, uint64_t* parsed) {
  if (seen) *seen = __atomic_exchange_n(&g_screen_seen, 0ull, __ATOMIC_RELAXED);
  if (parsed) *parsed = __atomic_exchange_n(&g_screen_parsed, 0ull, __ATOMIC_RELAXED);
  return 0;
}

static bool stream_debug() {
  static const bool on = getenv("XCG_STREAM_DEBUG") != nullptr;
  return on;
}

static bool prefix_filters_off() {   // XCG_NO_PREFIX_FILTERS: one slice of the round's LDS filter (A/B runs)
  static const bool off = getenv("XCG_NO_PREFIX_FILTERS") != nullptr;
  return off;
}

// ------------------------------------------------------------ stream rounds

namespace xcg {

template __global__ void encode_stream_kernel<8, 72, 16, false>(EncParams);
template __global__ void encode_stream_kernel<8, 72, 8, false>(EncParams);
template __global__ void encode_stream_kernel<8, 72, 4, false>(EncParams);
template __global__ void encode_stream_kernel<10, 264, 6, false>(EncParams);
template __global__ void encode_stream_kernel<10, 264, 2, false>(EncParams);

// B <- every declaration of this round (earliest chunk wins per hash), and the
// round's lane filter = the persistent cache's filter + B.  One thread per
// (chunk, declaration).
constexpr uint32_t PREP_TABLE = 1, PREP_FILTERS = 2;   // (what a round's prep / build covers)

// The round's LDS-filter slices (xcg_cache.h PREFIX_FILTERS): a batch key of
// chunk c goes into slice c / pfdiv, then every slice is ORed into the ones
// above it, so slice j = the cache + the keys of chunks < (j + 1) pfdiv.
__device__ __forceinline__ FiltSet prefix_slice(FiltSet f, uint32_t c, uint32_t pfdiv) {
  if (pfdiv) f.filt += (uint64_t)min(c / pfdiv, PREFIX_FILTERS - 1u) * FILT_WORDS;
  return f;
}
__global__ __launch_bounds__(256) void filt_prefix_kernel(uint32_t* f) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t w = 0;
#pragma unroll
  for (uint32_t j = 0; j < PREFIX_FILTERS; ++j) {
    w |= f[(uint64_t)j * FILT_WORDS + i];
    f[(uint64_t)j * FILT_WORDS + i] = w;
  }
}

// what: PREP_TABLE (the table and the counters), PREP_FILTERS, or both.  A
// verification builds the table alone: the filters of its declarations are
// only needed if a re-parse follows (then a filters-only pass adds them).
__global__ __launch_bounds__(256) void build_batch_table_kernel(const uint4* decl, const uint32_t* ndecl, uint32_t n,
                                                                uint32_t maxd, HashTab b, FiltSet fs, uint32_t* bcount,
                                                                int32_t* status, uint32_t what, uint32_t pfdiv) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t c = (uint32_t)(i / maxd), k = (uint32_t)(i % maxd);
  const bool have = c < n && k < ndecl[c];
  const uint64_t m = ballot(have);
  if ((what & PREP_TABLE) && lane_id() == 0 && m) atomicAdd(bcount + ((i >> 6) & 63u), (uint32_t)__builtin_popcountll(m));
  if (!have) return;
  const uint4 d = decl[i];
  if (what == (PREP_TABLE | PREP_FILTERS)) {
    if (!tab_insert_min_filt(b, prefix_slice(fs, c, pfdiv), d.x, d.y, ((uint64_t)c << 32) | d.z)) atomicOr(status, 2);
  } else if (what == PREP_TABLE) {
    if (!tab_insert_min(b, d.x, d.y, ((uint64_t)c << 32) | d.z)) atomicOr(status, 2);
  } else {
    filt_insert(prefix_slice(fs, c, pfdiv), d.x, d.y);
  }
}

// Restart backup (before a re-parse round that may resume chunks from their
// rows): every flagged chunk with a contradicted-lookup time gets a backup
// slot (while slots last) holding its previous pass's reference rows, REF
// output lengths, batch hits, counts and output bytes.  One workgroup per chunk.
__global__ __launch_bounds__(256) void restart_backup_kernel(uint32_t n, const uint32_t* need, const uint32_t* bad_t,
                                                             uint32_t* bslot, uint32_t* b_count, uint32_t slots,
                                                             const uint8_t* out, const uint64_t* out_off,
                                                             const uint64_t* out_len, uint8_t* b_out, uint64_t stride,
                                                             const uint4* ev, const uint32_t* eo, const uint32_t* nev,
                                                             uint32_t maxe, const uint64_t* hits, const uint32_t* nhits,
                                                             uint32_t maxh, const uint32_t* ndecl, uint4* b_ev,
                                                             uint32_t* b_eo, uint64_t* b_hits, uint32_t* b_cnt) {
  __shared__ uint32_t sk;
  const uint32_t c = blockIdx.x, t = threadIdx.x;
  if (c >= n) return;
  if (t == 0) {
    uint32_t k = ~0u;
    // (overflowed rows are incomplete: such a chunk re-parses from the start,
    // like one flagged with bad_t 0 or ~0)
    if (need[c] && bad_t[c] != ~0u && bad_t[c] != 0u && nev[c] <= maxe && nhits[c] <= maxh) {
      const uint32_t j = atomicAdd(b_count, 1u);
      if (j < slots) {
        k = j;
        atomicAdd(b_count + 2, 1u);                  // (cumulative: chunks resumed from their rows)
      }
    }
    bslot[c] = k;
    sk = k;
  }
  __syncthreads();
  const uint32_t k = sk;
  if (k == ~0u) return;
  const uint32_t ne = nev[c], nh = nhits[c];
  const uint64_t ol = out_len[c];
  if (t == 0) {
    b_cnt[4 * k] = ne;
    b_cnt[4 * k + 1] = nh;
    b_cnt[4 * k + 2] = (uint32_t)ol;
    b_cnt[4 * k + 3] = ndecl[c];
  }
  for (uint32_t i = t; i < ne; i += 256) {
    b_ev[(uint64_t)k * maxe + i] = ev[(uint64_t)c * maxe + i];
    b_eo[(uint64_t)k * maxe + i] = eo[(uint64_t)c * maxe + i];
  }
  for (uint32_t i = t; i < nh; i += 256) b_hits[(uint64_t)k * maxh + i] = hits[(uint64_t)c * maxh + i];
  const uint8_t* src = out + out_off[c];
  uint8_t* dst = b_out + (uint64_t)k * stride;
  for (uint64_t i = 16ull * t; i < ol; i += 16ull * 256) {
    if (i + 16 <= ol) *(u32x4_u*)(dst + i) = *(const u32x4_u*)(src + i);
    else for (uint64_t j = i; j < ol; ++j) dst[j] = src[j];
  }
}

// After that round: the old output tail of every spliced chunk (its previous
// pass's bytes from the rejoin point on) to its place behind the new part.
__global__ __launch_bounds__(256) void restart_splice_kernel(uint32_t n, uint4* splice, const uint32_t* bslot,
                                                             const uint8_t* b_out, uint64_t stride, uint8_t* out,
                                                             const uint64_t* out_off, uint32_t* b_count) {
  const uint32_t c = blockIdx.x, t = threadIdx.x;
  if (c >= n) return;
  const uint4 sp = splice[c];
  if (sp.w == 0u) return;
  if (t == 0) atomicAdd(b_count + 3, 1u);          // (cumulative: chunks that rejoined their old parse)
  const uint8_t* src = b_out + (uint64_t)bslot[c] * stride + sp.y;
  uint8_t* dst = out + out_off[c] + sp.x;
  const uint64_t len = sp.z - sp.y;
  for (uint64_t i = 16ull * t; i < len; i += 16ull * 256) {
    if (i + 16 <= len) *(u32x4_u*)(dst + i) = *(const u32x4_u*)(src + i);
    else for (uint64_t j = i; j < len; ++j) dst[j] = src[j];
  }
  __syncthreads();
  if (t == 0) splice[c].w = 0u;
}

// Seed for the rounds instead of round 0: a chunk's cold parse (nothing
// cached, no repeat inside the chunk) declares exactly the 2048-byte tiling
// 0, 2048, ... ("the cold parse of unique data is an exact
// 2048-aligned tiling").  Round 1 then parses every chunk against the
// tiling of the chunks before it; the verification flags every chunk the
// guess misled, so the result is exact whatever the data.  One wave per
// (chunk, tile): a hash pass over the batch instead of a full parse.
// SEED_TILES tiles per wave (several waves per chunk): all of a wave's loads
// are in flight together, and the batch's ~32 k waves hide HBM latency (one
// wave per chunk walking its tiles four at a time left each wave waiting).
constexpr uint32_t SEED_TILES = 8;
// With b.keys set, the kernel also builds round 1's batch table and filters
// from the tiles (what build_batch_table_kernel does from the lists): lane 0
// of each wave inserts its tiles' hashes as they are made, so the table's
// atomics overlap the other waves' hashing instead of a second pass.
__global__ __launch_bounds__(256) void seed_tiling_kernel(const uint8_t* in, const uint64_t* chunk_off,
                                                          const uint32_t* chunk_len, uint32_t n, uint32_t maxd,
                                                          uint4* decl, uint32_t* ndecl, uint32_t* nhits,
                                                          uint32_t* changed, HashTab b, FiltSet fs, uint32_t* bcount,
                                                          int32_t* status, uint32_t pfdiv) {
  const uint32_t wpc = (maxd + SEED_TILES - 1) / SEED_TILES;       // waves per chunk
  const uint32_t w = blockIdx.x * 4u + readfirst(threadIdx.x >> 6);
  const uint32_t c = w / wpc, k0 = (w % wpc) * SEED_TILES;
  if (w == 0 && threadIdx.x == 0) *changed = ~0u;
  if (c >= n) return;
  const int l = lane_id();
  const uint32_t m = min(chunk_len[c] / SEG, maxd);    // (an over-long chunk is refused by the round)
  const uint8_t* x = in + chunk_off[c];
  if (l == 0 && k0 == 0) {
    ndecl[c] = m;
    nhits[c] = 0u;
  }
  if (k0 >= m) return;
  // lane l sums bytes [16 l, 16 l + 16) and [1024 + 16 l, ...) of each tile
  u32x4 v[SEED_TILES][2];
  uint32_t mlo = 0, mhi = 0;
#pragma unroll
  for (uint32_t t = 0; t < SEED_TILES; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      v[t][h] = k0 + t < m ? *(const u32x4_u*)(x + (uint64_t)(k0 + t) * SEG + 1024u * h + 16u * l)
                           : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
  for (uint32_t t = 0; t < SEED_TILES; ++t) {
    if (k0 + t >= m) break;
    // Per 16-byte group h (offset q0 = 1024 h + 16 l in the tile): plain and
    // k-weighted sums of the bytes (v_dot4) and of ffs = ffbl + 1 (ffbl of a
    // zero byte is -1, so ffs sums are the ffbl sums + 16 and + 0 + ... + 15);
    // then X2 = sum (2048 - q0) S - W per group, and the same for F.
    uint32_t X1 = 0, X2 = 0, F1 = 0, F2 = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t q0 = 1024u * h + 16u * l;
      uint32_t sx = 0, wx = 0;
      int sf = 0, wf = 0;
#pragma unroll
      for (int w4 = 0; w4 < 4; ++w4) {
        const uint32_t d = v[t][h][w4];
        const uint32_t wts = (4u * w4) | ((4u * w4 + 1) << 8) | ((4u * w4 + 2) << 16) | ((4u * w4 + 3) << 24);
        sx = __builtin_amdgcn_udot4(d, 0x01010101u, sx, false);
        wx = __builtin_amdgcn_udot4(d, wts, wx, false);
        // the four bytes' ffbl (-1 for a zero byte) packed as signed bytes, then
        // summed plain and k-weighted by v_dot4_i32_i8 (8 VALU per word, not 12)
        auto fb = [d](int b) {   // (the compiler's ffbl reads the byte in place: v_ffbl_b32_sdwa)
          return (uint32_t)(__builtin_ffs((int)__builtin_amdgcn_ubfe(d, 8u * b, 8u)) - 1);
        };
        const uint32_t p = __builtin_amdgcn_perm(fb(1), fb(0), 0x0c0c0400u) |
                           __builtin_amdgcn_perm(fb(3), fb(2), 0x04000c0cu);
        sf = __builtin_amdgcn_sdot4((int)p, 0x01010101, sf, false);
        wf = __builtin_amdgcn_sdot4((int)p, (int)wts, wf, false);
      }
      sf += 16;
      wf += 120;
      X1 += sx; X2 += (2048u - q0) * sx - wx;
      F1 += sf; F2 += (2048u - q0) * sf - wf;
    }
    X1 = wave_sum(X1); X2 = wave_sum(X2); F1 = wave_sum(F1); F2 = wave_sum(F2);
    if ((uint32_t)l == t) {                        // lane t keeps tile t's hash
      mlo = (X1 << 20) + X2 + CLO;
      mhi = ((F1 << 16) + F2) << 4;
    }
  }
  // lanes 0 .. tiles-1: the declaration records and, with a table, its inserts
  // (all of the wave's tiles in one chain of round trips)
  const uint32_t tiles = min(SEED_TILES, m - k0);
  if ((uint32_t)l < tiles) {
    const uint32_t k = k0 + (uint32_t)l;
    decl[(uint64_t)c * maxd + k] = make_uint4(mlo, mhi, k * SEG, 0u);
    if (b.keys && !tab_insert_min_filt(b, prefix_slice(fs, c, pfdiv), mlo, mhi, ((uint64_t)c << 32) | (k * SEG)))
      atomicOr(status, 2);
  }
  if (b.keys && l == 0 && k0 == 0) atomicAdd(bcount + (c & 63u), m);   // (the chunk's count, once)
}

// Everything a round clears or copies before its batch table is built, in
// one launch (six separate memset / copy calls cost ~7 us each in launch
// gaps): the table, the round's filters (copies of the cache's, or zero while
// the cache is empty), the key counters, the changed word and, for a
// verification, the changed-hash table and its flags.
struct RoundPrep {
  HashTab tab;
  uint32_t* r_filt; const uint32_t* g_filt;
  u32x4* r_ftab; const u32x4* g_ftab; uint32_t ftab_n;      // 16-byte units
  uint32_t* r_gfilt; const uint32_t* g_gfilt; uint32_t gfilt_n;
  const uint32_t* nseg;
  uint32_t* bcount;
  uint32_t* changed;
  HashTab rt;           // keys == nullptr: not a verification round
  uint32_t* vflags;
  HashTab at;           // (keys == nullptr: no (a)-probe) newly visible hashes
  uint32_t* abits;
  uint32_t n;           // verification: need[0..n) cleared, bad_t / bad_hi (nullable) reset
  uint32_t* need;
  uint32_t* bad_t;
  uint32_t* bad_hi;
  uint32_t what;        // PREP_TABLE: the table, counters and verification state; PREP_FILTERS: the filters
};
__global__ __launch_bounds__(256) void round_prep_kernel(RoundPrep a) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool g_empty = *a.nseg == 0u;
  if (a.what & PREP_FILTERS) {
    // slice 0 starts as the cache's filter, the others empty (filt_prefix_kernel
    // ORs each slice into the ones above it once the batch keys are in)
    for (uint64_t i = i0; i < (uint64_t)FILT_WORDS * PREFIX_FILTERS; i += stride)
      a.r_filt[i] = (g_empty || i >= FILT_WORDS) ? 0u : a.g_filt[i];
    for (uint64_t i = i0; i < a.ftab_n; i += stride) a.r_ftab[i] = g_empty ? u32x4{0u, 0u, 0u, 0u} : a.g_ftab[i];
    for (uint64_t i = i0; i < a.gfilt_n; i += stride) a.r_gfilt[i] = g_empty ? 0u : a.g_gfilt[i];
  }
  if (!(a.what & PREP_TABLE)) return;
  for (uint64_t i = i0; i <= a.tab.mask; i += stride) { a.tab.keys[i] = EMPTY_KEY; a.tab.vals[i] = ~0ull; }
  if (a.rt.keys)
    for (uint64_t i = i0; i <= a.rt.mask; i += stride) { a.rt.keys[i] = EMPTY_KEY; a.rt.vals[i] = ~0ull; }
  if (a.rt.keys && a.need)
    for (uint64_t i = i0; i < a.n; i += stride) {
      a.need[i] = 0u;
      if (a.bad_t) { a.bad_t[i] = ~0u; a.bad_hi[i] = 0u; }
    }
  if (a.rt.keys && a.at.keys) {
    for (uint64_t i = i0; i <= a.at.mask; i += stride) { a.at.keys[i] = EMPTY_KEY; a.at.vals[i] = ~0ull; }
    for (uint64_t i = i0; i < XCG_VERIFY_A_WORDS; i += stride) a.abits[i] = 0u;
  }
  if (i0 < 64) a.bcount[i0] = 0u;
  if (i0 == 0) {
    *a.changed = ~0u;
    if (a.rt.keys) { a.vflags[0] = ~0u; a.vflags[1] = 0u; a.vflags[3] = 0u; }
  }
}

// ------------------------------------------------ verification of a round
//
// Round r parsed chunk k against V = the batch table of round r-1's
// declarations; T = the table of round r's.  k's parse depends on the batch
// only through its lookups, so it stands under T unless, for some hash h,
// (a) h becomes visible to k (earliest declaring chunk c_T < k <= c_V: a miss
//     may turn into a hit) and one of k's windows has hash h
//     (verify_probe_kernel; with more than XCG_VERIFY_A_LIMIT such hashes,
//     conservatively every k > c_T); or
// (b) k found h in V (a recorded hit) and under T h is invisible to k, or its
//     earliest declaration has other bytes.
// The fixed point is reached when no chunk is flagged.
__device__ __forceinline__ bool v4_ne(u32x4 a, u32x4 b) { return a[0] != b[0] || a[1] != b[1] || a[2] != b[2] || a[3] != b[3]; }
__device__ __forceinline__ bool seg_equal_t(const uint8_t* a, const uint8_t* b) {   // one thread, 2048 bytes
  for (int i = 0; i < SEG; i += 16)
    if (v4_ne(*(const u32x4_u*)(a + i), *(const u32x4_u*)(b + i))) return false;
  return true;
}

// The newly visible hashes' blocked Bloom filter: one word, two bits.
__device__ __forceinline__ uint32_t abits_word(uint32_t lo, uint32_t hi) {
  return (lo ^ (hi >> 4)) & (XCG_VERIFY_A_WORDS - 1u);
}
__device__ __forceinline__ uint32_t abits_mask(uint32_t lo, uint32_t hi) {
  return (1u << ((lo >> 13) & 31u)) | (1u << ((hi >> 21) & 31u));
}

__global__ __launch_bounds__(256) void verify_diff_kernel(HashTab tv, HashTab tt, const uint8_t* in,
                                                          const uint64_t* chunk_off, HashTab rt, uint32_t* a_first,
                                                          HashTab at, uint32_t* abits, int32_t* status) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nt = (uint64_t)tt.mask + 1, nv = (uint64_t)tv.mask + 1;
  uint64_t h, vt, vv;
  if (i < nt) {
    h = tt.keys[i];
    if (h == EMPTY_KEY) return;
    vt = tt.vals[i];
    vv = tab_lookup_t(tv, (uint32_t)h, (uint32_t)(h >> 32));
  } else if (i < nt + nv) {
    h = tv.keys[i - nt];
    if (h == EMPTY_KEY) return;
    if (tab_lookup_t(tt, (uint32_t)h, (uint32_t)(h >> 32)) != ~0ull) return;   // seen from T's side
    vt = ~0ull;
    vv = tv.vals[i - nt];
  } else {
    return;
  }
  if (vt == vv) return;
  const uint32_t INF = 0xFFFFFFFFu;
  const uint32_t ct = vt == ~0ull ? INF : (uint32_t)(vt >> 32), cv = vv == ~0ull ? INF : (uint32_t)(vv >> 32);
  uint32_t rlo = INF, rhi = 0;
  if (ct < cv) {                                                             // (a)
    atomicMin(a_first, ct + 1);
    if (at.keys) {                  // chunks (ct, cv] newly see h (a_first[3]: how many such h)
      const uint32_t j = atomicAdd(a_first + 3, 1u);
      if (j < XCG_VERIFY_A_LIMIT) {
        const uint32_t lo = (uint32_t)h, hi = (uint32_t)(h >> 32);
        if (!tab_insert_min(at, lo, hi, ((uint64_t)(ct + 1) << 32) | (cv == INF ? INF - 1 : cv)))
          atomicOr(a_first + 3, 0x80000000u);                                 // (conservative then)
        atomicOr(abits + abits_word(lo, hi), abits_mask(lo, hi));
      }
    }
  }
  bool same = false;
  if (vt != ~0ull && vv != ~0ull)
    same = seg_equal_t(in + chunk_off[ct] + (uint32_t)vt, in + chunk_off[cv] + (uint32_t)vv);
  // (b): chunks in (cv, ct] lose h; with other bytes, every chunk > min(cv, ct) that found h
  if (cv < ct) { rlo = min(rlo, cv + 1); rhi = max(rhi, ct == INF ? INF - 1 : ct); }
  if (!same && ct != INF && cv != INF) { rlo = min(rlo, min(ct, cv) + 1); rhi = INF - 1; }
  if (rlo <= rhi && !tab_insert_min(rt, (uint32_t)h, (uint32_t)(h >> 32), ((uint64_t)rlo << 32) | rhi))
    atomicOr(status, 2);
}

__global__ __launch_bounds__(256) void own_ovf_check_kernel(const uint32_t* nhits, uint32_t n, uint32_t maxh,
                                                            int32_t* status) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n && nhits[c] == maxh + 1u && status) atomicOr(status, 1);
}

// need[k] for every chunk: the conservative (a) (no probe, or too many newly
// visible hashes) or overflowed hit / reference lists -- such a chunk re-parses
// from its start (bad_t 0); then (a) by the probe and (b), which also give
// the times of the first and last affected lookup (bad_t / bad_hi, for the
// re-parse restart; ~0 / 0 until then).
__device__ __forceinline__ void verify_check_body(uint32_t bid, uint32_t n, const uint32_t* nhits, uint32_t maxh,
                                                  const uint32_t* nev, uint32_t maxe, bool probe,
                                                  const uint32_t* vflags, uint32_t* need, uint32_t* any,
                                                  uint32_t* bad_t, uint32_t* bad_hi) {
  const uint32_t k = bid * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const bool conservative = !probe || vflags[3] > XCG_VERIFY_A_LIMIT;
  const bool f = (k >= vflags[0] && conservative) || nhits[k] > maxh || (nev && nev[k] > maxe);
  if (f) {                                       // (need / bad_t / bad_hi start cleared: round_prep)
    need[k] = 1u;
    if (bad_t) {
      bad_t[k] = 0u;
      bad_hi[k] = ~1u;
    }
  }
  if (ballot(f) != 0 && lane_id() == 0) atomicOr(any, 1u);
}

// Flag chunk k with the in-chunk times [lo, hi] of affected lookups.
__device__ __forceinline__ void flag_chunk(uint32_t k, uint32_t lo, uint32_t hi, uint32_t* need, uint32_t* any,
                                           uint32_t* bad_t, uint32_t* bad_hi) {
  for (int off = 32; off >= 1; off >>= 1) {
    lo = min(lo, (uint32_t)__shfl_xor((int)lo, off));
    hi = max(hi, (uint32_t)__shfl_xor((int)hi, off));
  }
  if (lane_id() == 0 && lo != ~0u) {
    need[k] = 1u;
    atomicOr(any, 1u);
    if (bad_t) {
      atomicMin(bad_t + k, lo);
      atomicMax(bad_hi + k, hi);
    }
  }
}

// (a) exactly: every window of every chunk >= a_first, hashed like
// window_hashes_kernel (one wave per 2048 positions, 32 per lane), tested
// against the newly visible hashes' Bloom filter in LDS, then exactly; a
// window of chunk k whose hash became visible to k flags k at that window's
// lookup time 2 s + 1.  Blocks loop over the (chunk, span) items.
__device__ __forceinline__ void verify_probe_body(uint32_t bid, uint32_t nblk, uint32_t* sb, const uint8_t* in,
                                                  const uint64_t* chunk_off, const uint32_t* chunk_len, uint32_t n,
                                                  uint32_t spc, const uint32_t* vflags, HashTab at,
                                                  const uint32_t* abits, uint32_t* need, uint32_t* any,
                                                  uint32_t* bad_t, uint32_t* bad_hi) {
  const uint32_t a_first = vflags[0], acount = vflags[3];
  if (acount == 0u || acount > XCG_VERIFY_A_LIMIT || a_first >= n) return;
  for (uint32_t i = threadIdx.x; i < XCG_VERIFY_A_WORDS / 4; i += blockDim.x)
    ((u32x4*)sb)[i] = ((const u32x4*)abits)[i];
  __syncthreads();
  const int l = lane_id();
  const uint64_t items = (uint64_t)(n - a_first) * spc, nw = (uint64_t)nblk * 4u;
  for (uint64_t it = (uint64_t)bid * 4u + readfirst(threadIdx.x >> 6); it < items; it += nw) {
    const uint32_t k = a_first + (uint32_t)(it / spc);
    const int64_t len = chunk_len[k], npos = len - SEG + 1, p = (int64_t)(it % spc) * SEG;
    if (p >= npos) continue;
    const uint8_t* x = in + chunk_off[k];
    const int64_t q0 = p + 32 * l;
    const u32x4 a0 = load16_guarded(x, q0, len), a1 = load16_guarded(x, q0 + 16, len);
    const u32x4 b0 = load16_guarded(x, q0 + SEG, len), b1 = load16_guarded(x, q0 + SEG + 16, len);
    const uint32_t xa[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    const uint32_t xb[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
    uint32_t sxa = 0, sqxa = 0, sfa = 0, sqfa = 0, sxb = 0, sqxb = 0, sfb = 0, sqfb = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const uint32_t va = byte_of(xa[j >> 2], j & 3), vb = byte_of(xb[j >> 2], j & 3);
      const uint32_t fa = ffbl(va) + 1u, fb = ffbl(vb) + 1u;
      sxa += va; sqxa += j * va; sfa += fa; sqfa += j * fa;
      sxb += vb; sqxb += j * vb; sfb += fb; sqfb += j * fb;
    }
    const uint32_t qa = 32u * l, qb = 2048u + 32u * l;
    const uint32_t ta = qa * sxa + sqxa, tb = qb * sxb + sqxb;
    const uint32_t tfa = qa * sfa + sqfa, tfb = qb * sfb + sqfb;
    const uint32_t dx = sxb - sxa, dt = tb - ta, df = sfb - sfa, dtf = tfb - tfa;
    uint32_t X1 = wave_sum(sxa) + wave_incl_scan(dx) - dx;
    const uint32_t TT = wave_sum(ta) + wave_incl_scan(dt) - dt;
    uint32_t F1 = wave_sum(sfa) + wave_incl_scan(df) - df;
    const uint32_t TF = wave_sum(tfa) + wave_incl_scan(dtf) - dtf;
    uint32_t X2c = (2048u + qa) * X1 - TT + CLO;
    uint32_t F2 = (2048u + qa) * F1 - TF;
    uint32_t tlo = ~0u, thi = 0u;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const int64_t s = q0 + j;
      const uint32_t lo = (X1 << 20) + X2c, hi = ((F1 << 16) + F2) << 4;
      const uint32_t w = sb[abits_word(lo, hi)], m = abits_mask(lo, hi);
      if (s < npos && (w & m) == m) {
        const uint64_t v = tab_lookup_t(at, lo, hi);
        if (v != ~0ull && k >= (uint32_t)(v >> 32) && k <= (uint32_t)v) {
          tlo = min(tlo, 2u * (uint32_t)s + 1u);
          thi = max(thi, 2u * (uint32_t)s + 1u);
        }
      }
      const uint32_t xo = byte_of(xa[j >> 2], j & 3), xn = byte_of(xb[j >> 2], j & 3);
      const uint32_t ro = ffbl(xo), rn = ffbl(xn);
      X1 = X1 + xn - xo;
      X2c = X2c + X1 - (xo << 11);
      F1 = F1 + rn - ro;
      F2 = F2 + F1 - (ro << 11) - 2048u;
    }
    flag_chunk(k, tlo, thi, need, any, bad_t, bad_hi);
  }
}

// (b) from the reference rows (bounded caches: batch hits carry their lookup
// times), one wave per chunk; the hit lists' verify_hits_kernel otherwise.
__device__ __forceinline__ void verify_hit_events_body(uint32_t bid, uint32_t n, const uint4* ev, const uint32_t* nev,
                                                       uint32_t maxe, HashTab rt, uint32_t* need, uint32_t* any,
                                                       uint32_t* bad_t, uint32_t* bad_hi) {
  const uint32_t k = bid * 4u + readfirst(threadIdx.x >> 6);
  if (k >= n) return;
  const uint32_t cnt = min(nev[k], maxe);
  uint32_t lo = ~0u, hi = 0u;
  for (uint32_t i = lane_id(); i < cnt; i += 64) {
    const uint4 e = ev[(uint64_t)k * maxe + i];
    if ((e.w >> 30) == EV_HIT && (e.w & EV_REF_MASK) == 1u) {
      const uint64_t r = tab_lookup_t(rt, e.x, e.y);
      if (r != ~0ull && k >= (uint32_t)(r >> 32) && k <= (uint32_t)r) { lo = min(lo, e.z); hi = max(hi, e.z); }
    }
  }
  flag_chunk(k, lo, hi, need, any, bad_t, bad_hi);
}
__device__ __forceinline__ void verify_hits_body(uint32_t bid, uint32_t n, const uint64_t* hits, const uint32_t* nhits,
                                                 uint32_t maxh, HashTab rt, uint32_t* need, uint32_t* any) {
  const uint64_t j = (uint64_t)bid * blockDim.x + threadIdx.x;
  const uint32_t k = (uint32_t)(j / maxh), i = (uint32_t)(j % maxh);
  bool f = false;
  if (k < n && i < nhits[k]) {
    const uint64_t h = hits[j];
    const uint64_t r = tab_lookup_t(rt, (uint32_t)h, (uint32_t)(h >> 32));
    f = r != ~0ull && k >= (uint32_t)(r >> 32) && k <= (uint32_t)r;
    if (f) need[k] = 1u;
  }
  if (ballot(f) != 0 && lane_id() == 0) atomicOr(any, 1u);
}

// The verification's flagging passes in one launch (they only set flags, so
// their order does not matter; round_prep cleared need / bad_t / bad_hi):
// blocks [0, bc) the per-chunk check (block 0 also sums the declaration
// counters into vflags[2]), [bc, bc + bp) the (a)-probe, the rest the (b)
// hit check -- four launches' gaps fewer per round.
struct VerifyFlags {
  uint32_t n, bc, bp, bh;
  const uint32_t* nhits; uint32_t maxh; const uint64_t* hits;
  const uint32_t* nev; uint32_t maxe; const uint4* ev;
  bool probe; uint32_t* vflags; uint32_t* need; uint32_t* bad_t; uint32_t* bad_hi;
  const uint8_t* in; const uint64_t* chunk_off; const uint32_t* chunk_len; uint32_t spc;
  HashTab at; const uint32_t* abits; HashTab rt; const uint32_t* bcount;
};
__global__ __launch_bounds__(256) void verify_flags_kernel(VerifyFlags v) {
  __shared__ uint32_t sb[XCG_VERIFY_A_WORDS];
  const uint32_t b = blockIdx.x;
  uint32_t* any = v.vflags + 1;
  if (b < v.bc) {
    if (b == 0 && threadIdx.x < 64) {
      const uint32_t t = wave_sum(v.bcount[lane_id()]);
      if (lane_id() == 0) v.vflags[2] = t;
    }
    verify_check_body(b, v.n, v.nhits, v.maxh, v.nev, v.maxe, v.probe, v.vflags, v.need, any, v.bad_t, v.bad_hi);
  } else if (b < v.bc + v.bp) {
    verify_probe_body(b - v.bc, v.bp, sb, v.in, v.chunk_off, v.chunk_len, v.n, v.spc, v.vflags, v.at, v.abits, v.need,
                      any, v.bad_t, v.bad_hi);
  } else if (v.ev) {
    verify_hit_events_body(b - v.bc - v.bp, v.n, v.ev, v.nev, v.maxe, v.rt, v.need, any, v.bad_t, v.bad_hi);
  } else {
    verify_hits_body(b - v.bc - v.bp, v.n, v.hits, v.nhits, v.maxh, v.rt, v.need, any);
  }
}

// Segment numbers of the committed declarations: seg_base[c] = nseg + the
// declarations of chunks < c (exclusive scan, one workgroup), and nseg
// advanced by the total -- no per-block atomic on one counter (16 k of those
// serialised to ~190 us for a batch of 4 KiB packets).
// gate (nullable): run only if *gate == 0 -- the commit is queued right
// behind a verification and does nothing if that verification flagged chunks.
__global__ __launch_bounds__(1024) void commit_scan_kernel(const uint32_t* ndecl, uint32_t n, uint32_t* seg_base,
                                                           uint32_t* nseg, const uint32_t* gate) {
  // tiles of 1024 x 8 counts: each thread loads its 8 consecutive counts as
  // two 16-byte loads (coalesced across the wave), the block scans the 1024
  // thread sums (wave scans + the 16 wave totals: two barriers a tile, where a
  // Hillis-Steele pass per 4096 counts took twenty -- 54 us at 65 k chunks)
  constexpr uint32_t PER = 8;
  __shared__ uint32_t wtot[16];
  const uint32_t t = threadIdx.x, wv = t >> 6;
  if (gate && *gate) return;
  uint32_t carry = *nseg;
  for (uint32_t base = 0; base < n; base += 1024 * PER) {
    const uint32_t i0 = base + PER * t;
    uint32_t v[PER];
    if (i0 + PER <= n) {
      const uint4 a0 = *(const uint4*)(ndecl + i0), a1 = *(const uint4*)(ndecl + i0 + 4);
      v[0] = a0.x; v[1] = a0.y; v[2] = a0.z; v[3] = a0.w; v[4] = a1.x; v[5] = a1.y; v[6] = a1.z; v[7] = a1.w;
    } else {
#pragma unroll
      for (uint32_t k = 0; k < PER; ++k) v[k] = i0 + k < n ? ndecl[i0 + k] : 0u;
    }
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) sum += v[k];
    const uint32_t incl = wave_incl_scan(sum);
    if (lane_id() == 63) wtot[wv] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t q = 0; q < 16; ++q) {
      const uint32_t x = wtot[q];
      before += q < wv ? x : 0u;
      total += x;
    }
    uint32_t o[PER];
    uint32_t run = carry + before + incl - sum;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
      o[k] = run;
      run += v[k];
    }
    if (i0 + PER <= n) {
      *(uint4*)(seg_base + i0) = make_uint4(o[0], o[1], o[2], o[3]);
      *(uint4*)(seg_base + i0 + 4) = make_uint4(o[4], o[5], o[6], o[7]);
    } else {
#pragma unroll
      for (uint32_t k = 0; k < PER; ++k)
        if (i0 + k < n) seg_base[i0 + k] = o[k];
    }
    carry += total;
    __syncthreads();                                   // (wtot is reused)
  }
  if (t == 0) *nseg = carry;
}

// Commit the converged declarations into the persistent cache
// (XCodecMemoryCache::enter, xcodec_cache.h:303-325).  Block (chunk c, part q)
// takes declarations q*256 .. q*256+255 of chunk c, whose segments are
// seg_base[c] + q*256 + j in declaration order.  Each wave first copies four
// 2048-byte segments at a time into the pool with all eight 16-byte loads per
// lane in flight together (the input offsets staged in LDS), then each thread
// inserts its declaration's hash.  The copy is issued
// before the inserts: on gfx9 an atomic's return waits on every older memory
// operation of the wave, so inserts first serialised each segment copy behind
// the insert chain (70 -> 44 us for C2-S2's ~66 k declarations).
__global__ __launch_bounds__(256) void commit_kernel(const uint4* decl, const uint32_t* ndecl, uint32_t n,
                                                     uint32_t maxd, const uint8_t* in, const uint64_t* chunk_off,
                                                     HashTab g, uint8_t* pool, const uint32_t* seg_base,
                                                     uint32_t seg_cap, FiltSet fs, int32_t* status,
                                                     const uint32_t* gate) {
  if (gate && *gate) return;
  const uint32_t parts = (maxd + 255) / 256;
  const uint32_t c = blockIdx.x / parts, k0 = (blockIdx.x % parts) * 256u;
  const uint32_t nd = c < n ? ndecl[c] : 0u;
  const uint32_t cnt = nd > k0 ? min(256u, nd - k0) : 0u;
  if (cnt == 0) return;                            // uniform over the block
  const uint32_t s_base = seg_base[c] + k0;
  const uint32_t k = k0 + threadIdx.x;
  const bool have = k < nd;
  __shared__ uint32_t zoff[256];                   // the declarations' input offsets
  uint4 d = make_uint4(0u, 0u, 0u, 0u);
  if (have) d = decl[(uint64_t)c * maxd + k];
  zoff[threadIdx.x] = d.z;
  __syncthreads();
  const int l = lane_id();
  const uint32_t wv = readfirst(threadIdx.x >> 6);
  const uint8_t* x = in + chunk_off[c];
  for (uint32_t j0 = 4u * wv; j0 < cnt; j0 += 16u) {
    u32x4 v[8];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      if (j0 + j < cnt) {
        const uint8_t* src = x + readfirst(zoff[j0 + j]);
        v[2 * j] = *(const u32x4_u*)(src + 32 * l);
        v[2 * j + 1] = *(const u32x4_u*)(src + 32 * l + 16);
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t sg = s_base + j0 + j;
      if (j0 + j < cnt && sg < seg_cap) {
        uint8_t* dst = pool + (uint64_t)sg * SEG;
        *(u32x4_u*)(dst + 32 * l) = v[2 * j];
        *(u32x4_u*)(dst + 32 * l + 16) = v[2 * j + 1];
      }
    }
  }
  if (have) {
    const uint32_t seg = s_base + threadIdx.x;
    if (seg >= seg_cap) {
      atomicOr(status, 4);
    } else {
      if (!tab_insert_min_filt(g, fs, d.x, d.y, seg)) atomicOr(status, 2);
    }
  }
}

}  // namespace xcg

// The tiling seed alone (decl / ndecl / nhits / changed), for a caller that
// looks at it before the rounds (the bounded cache's first eviction guess);
// then xcg_launch_encode_stream with keep_decls.
extern "C" int xcg_launch_seed_tiling(const XcgStreamArgs* a, hipStream_t stream) {
  if (a->n == 0) return 0;
  const uint32_t seed_waves = a->n * ((a->maxd + xcg::SEED_TILES - 1) / xcg::SEED_TILES);
  hipLaunchKernelGGL(xcg::seed_tiling_kernel, dim3((seed_waves + 3) / 4), dim3(256), 0, stream, a->in, a->chunk_off,
                     a->chunk_len, a->n, a->maxd, (uint4*)a->decl, a->ndecl, a->nhits, a->changed,
                     xcg::HashTab{nullptr, nullptr, 0u}, xcg::FiltSet{}, nullptr, nullptr, 0u);
  return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}

// Live timing of the stream-parse kernel for bench.py's roofline: while on,
// every encode_stream_kernel launch is bracketed by HIP events on its own
// launch stream; xcg_debug_stream_kernel_time sums them (process-wide).
namespace {
std::mutex g_ktime_mu;
bool g_ktime_on = false;
std::vector<std::pair<hipEvent_t, hipEvent_t>> g_ktime_ev;
}  // namespace
extern "C" int xcg_debug_stream_kernel_timing(int on) {
  std::lock_guard<std::mutex> g(g_ktime_mu);
  const int old = g_ktime_on;
  g_ktime_on = on != 0;
  return old;
}
extern "C" int xcg_debug_stream_kernel_time(double* ms, uint32_t* launches) {
  std::lock_guard<std::mutex> g(g_ktime_mu);
  double tot = 0;
  int rc = 0;
  for (auto& e : g_ktime_ev) {
    float t = 0;
    if (hipEventSynchronize(e.second) != hipSuccess || hipEventElapsedTime(&t, e.first, e.second) != hipSuccess)
      rc = XCG_RC_HIP;
    tot += t;
    (void)hipEventDestroy(e.first);
    (void)hipEventDestroy(e.second);
  }
  if (ms) *ms = tot;
  if (launches) *launches = (uint32_t)g_ktime_ev.size();
  g_ktime_ev.clear();
  return rc;
}
static hipEvent_t ktime_begin(hipStream_t s) {
  std::lock_guard<std::mutex> g(g_ktime_mu);
  hipEvent_t e = nullptr;
  if (!g_ktime_on || hipEventCreate(&e) != hipSuccess) return nullptr;
  (void)hipEventRecord(e, s);
  return e;
}
static void ktime_end(hipEvent_t e0, hipStream_t s) {
  if (!e0) return;
  std::lock_guard<std::mutex> g(g_ktime_mu);
  hipEvent_t e1 = nullptr;
  if (hipEventCreate(&e1) != hipSuccess) return;
  (void)hipEventRecord(e1, s);
  g_ktime_ev.emplace_back(e0, e1);
}

// The event behind the verification flags' copy: the context's (destroyed with
// it), or one made for this call when the caller passes none.
struct FlagsEvent {
  hipEvent_t ev = nullptr;
  bool own = false;
  explicit FlagsEvent(void* given) {
    if (given) {
      ev = (hipEvent_t)given;
    } else if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {
      own = true;
    } else {
      ev = nullptr;
    }
  }
  ~FlagsEvent() {
    if (own) (void)hipEventDestroy(ev);
  }
};

extern "C" int xcg_launch_encode_stream(const XcgStreamArgs* a, int* rounds_out, hipStream_t stream) {
  using namespace xcg;

  const uint32_t n = a->n;
  if (n == 0) return 0;
  EncParams prm{a->in, a->chunk_off, a->chunk_len, n, a->flags, a->out, a->out_off, a->out_len, a->stats, a->status};
  prm.max_len = (a->maxd - 1) * SEG + (SEG - 1);     // maxd = max_chunk_len / 2048 + 1
  prm.g = tab_of(a->g);
  prm.pool = a->g.pool;
  prm.b = HashTab{a->b_keys, a->b_vals, a->b_mask};
  prm.decl = (uint4*)a->decl;
  prm.ndecl = a->ndecl;
  prm.maxd = a->maxd;
  prm.changed = a->changed;
  prm.nseg = a->g.nseg;
  prm.bcount = a->bcount;
  prm.lds_filter_keys = xcg_lds_filter_keys();
  if (prm.lds_filter_keys == LFK_AUTO)
    prm.lds_filter_keys = 16ull * ((uint64_t)a->g.fmask + 1) > (2ull << 20) ? 0u : xcg::LDS_FILTER_KEYS_DEFAULT;
  prm.lds_prefilter_keys = __atomic_load_n(&g_lds_prefilter_keys, __ATOMIC_RELAXED);
  prm.ptime = a->ptime;
  prm.ev = (uint4*)a->ev;
  prm.nev = a->nev;
  prm.maxe = a->maxe;
  prm.eo = a->ev ? a->eo : nullptr;
  prm.rs = RestartArgs{};
  const size_t tbytes = ((size_t)a->g.fmask + 1) * 16;
  const size_t gbytes = ((size_t)a->g.gmask + 1) * 4;
  FlagsEvent flags_ev(a->flags_ev);
  int dev = 0;
  int cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return XCG_RC_HIP;
  const uint32_t wgs = (uint32_t)cus;
  const bool big = a->maxd > 72;                     // chunks > 128 KiB (<= 512 KiB frames): 264 records
  // One workgroup per CU (LDS): SW chunk-waves each.  A batch too small to
  // give every CU a full workgroup spreads over more CUs with fewer waves
  // (a wave alone on its SIMD parses faster than four sharing it).
  const uint32_t SW = big ? (n <= 2 * wgs ? 2u : 6u) : (n <= 4 * wgs ? 4u : (n <= 8 * wgs ? 8u : 16u));
  const dim3 sgrid(min(wgs, (n + SW - 1) / SW)), sblock(64 * SW);
  // The quiet-chunk screen (stream_screen_kernel) in front of the parse: small
  // chunks, in-band, not the bounded / pair variants (which record references).
  const bool screen = a->s_fold && a->s_work && a->s_info && a->s_rows && a->s_qcnt && a->s_qkeys && !a->ev && !(a->flags & (XCG_FLAG_OOB | XCG_FLAG_NULLCACHE)) &&
                      a->maxd <= (uint32_t)SCREEN_MAXD && xcg_screen_on();
  // bounded cache: the variant that records the chunks' cache references (xcg_lru.hip)
  auto launch = [&]() {
    if (screen) {
      xcg_launch_stream_screen(a, &prm, wgs, stream);
      prm.work = a->s_work;
      if (xcg_screen_counting()) {
        uint32_t w = 0;
        (void)hipMemcpyAsync(&w, a->s_work, 4, hipMemcpyDeviceToHost, stream);
        (void)hipStreamSynchronize(stream);
        uint32_t seen = n;
        if (prm.need) {
          std::vector<uint32_t> h(n);
          (void)hipMemcpy(h.data(), prm.need, 4ull * n, hipMemcpyDeviceToHost);
          seen = 0;
          for (uint32_t v : h) seen += v != 0;
        }
        __atomic_add_fetch(&g_screen_seen, (uint64_t)(seen - (prm.skip_below < seen ? prm.skip_below : 0u)),
                           __ATOMIC_RELAXED);
        __atomic_add_fetch(&g_screen_parsed, (uint64_t)w, __ATOMIC_RELAXED);
      }
    }
    if (stream_debug()) {
      uint32_t cnt = n;
      if (prm.need) {
        std::vector<uint32_t> h(n);
        (void)hipMemcpyAsync(h.data(), prm.need, 4ull * n, hipMemcpyDeviceToHost, stream);
        (void)hipStreamSynchronize(stream);
        cnt = 0;
        for (uint32_t v : h) cnt += v != 0;
      }
      fprintf(stderr, "stream: launch over %u of %u chunks (skip below %u)\n", cnt, n, prm.skip_below);
    }
    hipEvent_t e0 = ktime_begin(stream);
    if (prm.ev) xcg_launch_encode_stream_lru(big, SW, sgrid, sblock, &prm, stream);
    else launch_stream_instance<false>(big, SW, sgrid, sblock, prm, stream);
    ktime_end(e0, stream);
    prm.work = nullptr;
  };
  // lowest chunk whose declaration list changed in the round just run (~0u: none)
  auto changed_after = [&](uint32_t& fc) -> bool {
    if (hipMemcpyAsync(a->h_changed, a->changed, 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
      return false;
    fc = *a->h_changed;
    return true;
  };
  const bool keep = a->keep_decls && n > 1;
  const bool seeded = (a->seed || keep) && n > 1;
  if (!seeded && (hipMemsetAsync(a->ndecl, 0, 4ull * n, stream) != hipSuccess ||
                  hipMemsetAsync(a->nhits, 0, 4ull * n, stream) != hipSuccess ||
                  hipMemsetAsync(a->changed, 0xFF, 4, stream) != hipSuccess))
    return XCG_RC_HIP;                                       // (the seed kernel initialises these itself)
  if (a->decls_out) *a->decls_out = ~0u;
  prm.need = nullptr;
  prm.hits = a->hits;                              // every stream round writes nhits[chunk]
  prm.nhits = a->nhits;
  prm.maxh = a->maxh;
  // Round 0: every chunk against the persistent cache + its own declarations.
  prm.use_b = false;
  prm.skip_below = 0;
  prm.lf = LaneFilter{a->g.filt, (const u32x4*)a->g.ftab, a->g.fmask, a->g.gfilt, a->g.gmask};
  HashTab tabs[2] = {HashTab{a->b_keys, a->b_vals, a->b_mask}, HashTab{a->b2_keys, a->b2_vals, a->b_mask}};
  const HashTab rt{a->r_keys, a->r_vals, a->r_mask};
  // (a) by probing the windows (a_bits null: the conservative flag)
  const bool probe = a->a_bits && a->a_keys;
  const HashTab at = probe ? HashTab{a->a_keys, a->a_vals, XCG_VERIFY_A_CAP - 1} : HashTab{nullptr, nullptr, 0u};
  int cur = 0;
  int dev_cus = (int)wgs;
  // A round's batch table, filters and counters cleared / copied from the cache's.
  // later rounds resume flagged chunks too (bounded / pair: the verification
  // gives the affected lookups' times)
  const bool rs_rounds = a->ev && a->restart && a->bslot && prm.eo && a->bad_t;
  const uint32_t pfdiv = prefix_filters_off() ? 0u : (n + PREFIX_FILTERS - 1) / PREFIX_FILTERS;   // chunks per slice of the round's LDS filter
  auto prep = [&](int t, bool verify, uint32_t what) -> bool {
    RoundPrep rp{tabs[t], a->r_filt, a->g.filt, (u32x4*)a->r_ftab, (const u32x4*)a->g.ftab, (uint32_t)(tbytes / 16),
                 a->r_gfilt, a->g.gfilt, (uint32_t)(gbytes / 4), a->g.nseg, a->bcount, a->changed,
                 verify ? rt : HashTab{nullptr, nullptr, 0u}, a->vflags, at, a->a_bits, n, a->need,
                 rs_rounds ? a->bad_t : nullptr, rs_rounds ? a->bad_hi : nullptr, what};
    hipLaunchKernelGGL(round_prep_kernel, dim3(4 * dev_cus), dim3(256), 0, stream, rp);
    return hipGetLastError() == hipSuccess;
  };
  bool seed_built = false;
  int rounds = 0;
  uint32_t fc = 0;
  if (keep) {
    // the previous pass's declaration lists seed round 1 (a bounded cache's
    // eviction times changed under them)
  } else if (seeded) {
    // Round 1's table and filters are built by the seed itself (after the
    // round's prep has cleared them) when its waves hash full groups of tiles;
    // with small chunks (a wave per chunk of one or two tiles) the waves would
    // sit on their inserts at low occupancy (C4's 4 KiB packets: seed 66 ->
    // 342 us), so the separate build keeps them.
    const bool fuse = a->maxd > SEED_TILES;
    if (fuse && !prep(cur, false, PREP_TABLE | PREP_FILTERS)) return XCG_RC_HIP;
    const uint32_t seed_waves = n * ((a->maxd + SEED_TILES - 1) / SEED_TILES);
    hipLaunchKernelGGL(seed_tiling_kernel, dim3((seed_waves + 3) / 4), dim3(256), 0, stream, a->in, a->chunk_off,
                       a->chunk_len, n, a->maxd, (uint4*)a->decl, a->ndecl, a->nhits, a->changed,
                       fuse ? tabs[cur] : HashTab{nullptr, nullptr, 0u},
                       FiltSet{a->r_filt, a->r_ftab, a->g.fmask, a->r_gfilt, a->g.gmask}, a->bcount, a->status, pfdiv);
    if (fuse) hipLaunchKernelGGL(filt_prefix_kernel, dim3(FILT_WORDS / 256), dim3(256), 0, stream, a->r_filt);
    seed_built = fuse;
  } else {
    launch();
    rounds = 1;
    // (one chunk: no round follows, so no need to learn what it declared)
    if (n > 1 && !changed_after(fc)) return XCG_RC_HIP;
    if (n > 1 && fc == ~0u && a->decls_out) *a->decls_out = 0;   // round 0 declared nothing
  }
  // Jacobi rounds: chunk k re-parses against the declarations chunks < k made
  // in the previous round.  Chunk 0 is exact after round 0 and, inductively,
  // chunk k after round k.  Round 1 re-parses every chunk after the first
  // that declared anything in round 0 (those before it saw an empty batch);
  // after each later round the verification (verify_*_kernel) compares the
  // round's batch table with the one the round parsed against and flags the
  // chunks whose lookups could change; only those are re-parsed.  No flag =
  // the fixed point, which is the sequential result.

  // Commit the declaration lists into the persistent cache; with a gate, only
  // if the verification that precedes it in the stream flagged nothing.
  bool committed = false;
  auto commit = [&](const uint32_t* gate) {
    if (a->no_commit) return;
    const uint32_t parts = (a->maxd + 255) / 256;
    uint32_t* seg_base = (uint32_t*)a->hits;       // (free once the rounds are over: n words)
    hipLaunchKernelGGL(commit_scan_kernel, dim3(1), dim3(1024), 0, stream, (const uint32_t*)a->ndecl, n, seg_base,
                       a->g.nseg, gate);
    hipLaunchKernelGGL(commit_kernel, dim3(n * parts), dim3(256), 0, stream, (const uint4*)a->decl,
                       (const uint32_t*)a->ndecl, n, a->maxd, a->in, a->chunk_off, prm.g, a->g.pool,
                       (const uint32_t*)seg_base, a->g.seg_cap, filters_of(a->g), a->status, gate);
  };
  auto build = [&](int t, bool verify, uint32_t what) -> bool {
    if (!prep(t, verify, what)) return false;
    const uint64_t nthreads = (uint64_t)n * a->maxd;
    hipLaunchKernelGGL(build_batch_table_kernel, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, stream,
                       (const uint4*)a->decl, (const uint32_t*)a->ndecl, n, a->maxd, tabs[t],
                       FiltSet{a->r_filt, a->r_ftab, a->g.fmask, a->r_gfilt, a->g.gmask}, a->bcount, a->status, what,
                       pfdiv);
    if (what & PREP_FILTERS)
      hipLaunchKernelGGL(filt_prefix_kernel, dim3(FILT_WORDS / 256), dim3(256), 0, stream, a->r_filt);
    return hipGetLastError() == hipSuccess;
  };
  // A re-parse round whose flagged chunks (their first contradicted lookup in
  // bad_t) resume from their rows (encode_chunk, "Re-parse restart"): back
  // the rows up, parse, splice the rejoined tails' bytes.
  auto run_restarted = [&]() {
    (void)hipMemsetAsync(a->b_count, 0, 4, stream);
    hipLaunchKernelGGL(restart_backup_kernel, dim3(n), dim3(256), 0, stream, n, (const uint32_t*)a->need,
                       (const uint32_t*)a->bad_t, a->bslot, a->b_count, a->b_slots, (const uint8_t*)a->out,
                       a->out_off, (const uint64_t*)a->out_len, a->b_out, a->b_stride, (const uint4*)a->ev,
                       (const uint32_t*)a->eo, (const uint32_t*)a->nev, a->maxe, (const uint64_t*)a->hits,
                       (const uint32_t*)a->nhits, a->maxh, (const uint32_t*)a->ndecl, (uint4*)a->b_ev, a->b_eo,
                       a->b_hits, a->b_cnt);
    prm.rs = RestartArgs{a->bad_t, a->bad_hi, a->bslot, (const uint4*)a->b_ev, a->b_eo, a->b_hits, a->b_cnt,
                         (uint4*)a->splice};
    launch();
    hipLaunchKernelGGL(restart_splice_kernel, dim3(n), dim3(256), 0, stream, n, (uint4*)a->splice,
                       (const uint32_t*)a->bslot, (const uint8_t*)a->b_out, a->b_stride, a->out, a->out_off,
                       a->b_count);
    prm.rs = RestartArgs{};
    if (stream_debug()) {
      uint32_t bc[4] = {0, 0, 0, 0};
      (void)hipMemcpyAsync(bc, a->b_count, 16, hipMemcpyDeviceToHost, stream);
      (void)hipStreamSynchronize(stream);
      fprintf(stderr, "stream: restart slots %u, cumulative resumed %u rejoined %u\n", bc[0], bc[2], bc[3]);
    }
  };
  if (n > 1 && fc != ~0u) {
    if (!seed_built && !build(cur, false, PREP_TABLE | PREP_FILTERS)) return XCG_RC_HIP;
    prm.use_b = true;
    prm.b = tabs[cur];
    prm.skip_below = seeded ? 0 : fc + 1;            // (seeded: round 1 parses every chunk)
    prm.lf = LaneFilter{a->r_filt, (const u32x4*)a->r_ftab, a->g.fmask, a->r_gfilt, a->g.gmask, pfdiv};
    if (keep && a->need_given) prm.need = a->need;   // the rest stand under the kept lists
    const bool rs = keep && a->need_given && a->restart && a->bslot && prm.eo;
    if (rs) run_restarted();
    else launch();
    ++rounds;
    prm.skip_below = 0;
    // (no host sync here: the verification's own sync tells whether round 1
    // changed anything that matters)
    // Each round fixes at least the first flagged chunk (every chunk before
    // it already stands under the final lists), so n rounds always suffice.
    bool converged = false;
    for (uint32_t r = 2; r <= n + 1; ++r) {
      // verify round r-1 (parsed against tabs[cur]) against its own declarations
      const int nxt = cur ^ 1;
      if (!build(nxt, true, PREP_TABLE)) return XCG_RC_HIP;   // (filters only if a re-parse follows)
      const uint64_t slots = 2ull * (a->b_mask + 1);
      hipLaunchKernelGGL(verify_diff_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, stream, tabs[cur],
                         tabs[nxt], a->in, a->chunk_off, rt, a->vflags, at, a->a_bits, a->status);
      uint32_t* vbad_t = rs_rounds ? a->bad_t : nullptr;
      uint32_t* vbad_hi = rs_rounds ? a->bad_hi : nullptr;
      {
        VerifyFlags v{};
        v.n = n;
        v.bc = (n + 255) / 256;
        if (probe) {
          const uint64_t items = (uint64_t)n * a->maxd;   // (chunk, 2048-position span) pairs, maxd per chunk
          const uint64_t blocks = (items + 3) / 4, cap = 5ull * (uint64_t)dev_cus;   // (32 KiB of LDS each)
          v.bp = (uint32_t)(blocks < cap ? blocks : cap);
        }
        v.bh = a->ev ? (n + 3) / 4 : (uint32_t)(((uint64_t)n * a->maxh + 255) / 256);
        v.nhits = (const uint32_t*)a->nhits; v.maxh = a->maxh; v.hits = (const uint64_t*)a->hits;
        v.nev = (const uint32_t*)(a->ev ? a->nev : nullptr); v.maxe = a->maxe; v.ev = (const uint4*)a->ev;
        v.probe = probe; v.vflags = a->vflags; v.need = a->need; v.bad_t = vbad_t; v.bad_hi = vbad_hi;
        v.in = a->in; v.chunk_off = a->chunk_off; v.chunk_len = a->chunk_len; v.spc = a->maxd;
        v.at = at; v.abits = (const uint32_t*)a->a_bits; v.rt = rt; v.bcount = (const uint32_t*)a->bcount;
        hipLaunchKernelGGL(verify_flags_kernel, dim3(v.bc + v.bp + v.bh), dim3(256), 0, stream, v);
      }
      if (hipMemcpyAsync(a->h_vflags, a->vflags, 16, hipMemcpyDeviceToHost, stream) != hipSuccess) return XCG_RC_HIP;
      // The host waits for the flags alone: the commit (a no-op if anything was
      // flagged) runs on the device while the host returns and queues the next
      // batch behind it, so the device does not idle through the host's turn.
      const hipEvent_t vev = flags_ev.ev;
      if (!vev || hipEventRecord(vev, stream) != hipSuccess) return XCG_RC_HIP;
      commit(a->vflags + 1);
      if (a->post_verify && a->post_verify(a->post_user, a->vflags + 1, stream)) return XCG_RC_HIP;
      if (hipEventSynchronize(vev) != hipSuccess) return XCG_RC_HIP;
      if (a->decls_out) *a->decls_out = a->h_vflags[2];
      if (stream_debug())
        fprintf(stderr, "stream: n %u round %u first (a)-flag %d any %u newly visible %u\n", n, r,
                (int)a->h_vflags[0], a->h_vflags[1], a->h_vflags[3]);
      if (a->h_vflags[1] == 0) {                       // nothing flagged: fixed point (already committed)
        converged = true;
        committed = true;
        break;
      }
      if (hipMemsetAsync(a->changed, 0xFF, 4, stream) != hipSuccess) return XCG_RC_HIP;
      if (!build(nxt, false, PREP_FILTERS)) return XCG_RC_HIP;   // the re-parse's filters: cache + round r-1's lists
      cur = nxt;
      prm.b = tabs[cur];
      prm.need = a->need;
      if (rs_rounds) run_restarted();                // (resumed before the first affected lookup)
      else launch();                                 // (flagged by the verification: from the start)
      ++rounds;
    }
    if (!converged) return XCG_RC_OVERFLOW;
  }
  // A result no verification passed over (one chunk, or round 0 declared
  // nothing): an own-table overflow in it is reported (status bit 0).
  if (!committed) hipLaunchKernelGGL(own_ovf_check_kernel, dim3((n + 255) / 256), dim3(256), 0, stream,
                                     (const uint32_t*)a->nhits, n, a->maxh, a->status);
  if (!committed) commit(nullptr);
  if (rounds_out) *rounds_out = rounds;
  return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}
