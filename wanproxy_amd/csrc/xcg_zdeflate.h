// wanproxy's zlib stage on the GPU: DeflatePipe (zlib/deflate_pipe.cc:57-115)
// for many streams at once, bit-exact with zlib 1.2.11's deflate at levels 4-9
// (deflate_slow; wanproxy.conf sets level 6).  gfx950, wave64.
//
// A DeflatePipe::consume() of n bytes is deflate(Z_NO_FLUSH) over its
// segments then deflate(Z_SYNC_FLUSH); an empty consume is deflate(Z_FINISH).
// The output does not depend on the segmentation (every position zlib
// processes under Z_NO_FLUSH has >= MIN_LOOKAHEAD bytes of lookahead), so a
// call is its bytes plus a flush.  Per call, in HBM:
//
//   X      the stream's last 32 KiB (history) ++ the call's bytes.  X index j
//          is stream position total - 32768 + j.          zd_prep_kernel (match)
//   d16    hash-chain links: j - prev(j), prev(j) = the latest earlier position
//          with the same 3-byte hash (zlib's head/prev, deflate.c INSERT_STRING:
//          deflate_slow inserts every position once its 3 bytes exist, in
//          order), 0 = none / farther than 32767.   zd_hashes / zd_chain (match)
//   tf/tq  per position: longest_match's walk from the chain head with the full
//          and the quartered (prev_length >= good_match) chain budget: best
//          length and the distance of the first candidate reaching it.  The
//          threshold prev_length cannot change which candidate wins (first of
//          maximal length) nor where the nice-length break falls, so one walk
//          serves every prev_length.  Bytes past the lookahead never change
//          longest_match's result (nice is clipped to the lookahead), so lengths
//          are capped there and zlib's 64 KiB window is never materialised.
//                                                  zd_match_kernel (match)
//   sym    the lazy-matching scan (deflate_slow) over that table, one wave per
//          call, sequential but cheap per position; runs of positions where no
//          match can start are emitted 64 at a time.  Window slides are
//          tracked (coord 0 is NIL; a block whose start slid out cannot be
//          stored).  Blocks end every 16383 symbols (lit_bufsize - 1).
//                                          zd_scan_kernel, zd_fscan_kernel (parse)
//   trees  per block (one wave): symbol histogram, zlib's build_tree /
//          gen_bitlen / gen_codes, bit-length tree, the stored / static /
//          dynamic choice of _tr_flush_block.       zd_trees_kernel (huff)
//   out    layout (block bit offsets, zeroed output), then every block's bits
//          in parallel (atomicOr into the zeroed words).   zd_layout / zd_emit (huff)
// (match), (parse), (huff): the unit xcg_zdeflate_<name>.hip.  The stream state
// after the call (zd_commit_kernel), level 0, the host object and its drivers
// are in xcg_zdeflate.hip.
//
// The reference interface replaced is DeflatePipe(level) / consume(Buffer*)
// (zlib/deflate_pipe.h:33-42, deflate_pipe.cc:36-115).
// This header: the device side the four units share and the launch functions
// each kernel unit exports (a kernel is launched only from its own unit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "xcg_device.h"
#include "xcg_zdeflate_types.h"

namespace xcg {
namespace zd {

// configuration_table (deflate.c): good, lazy, nice, chain.  (One copy per
// unit that reads it: no relocatable device code.)
static __constant__ int CFG[10][4] = {{0, 0, 0, 0},        {4, 4, 8, 4},     {4, 5, 16, 8},      {4, 6, 32, 32},
                                      {4, 4, 16, 16},      {8, 16, 32, 32},  {8, 16, 128, 128},  {8, 32, 128, 256},
                                      {32, 128, 258, 1024}, {32, 258, 258, 4096}};

// length - 3 (0..255) -> length code 0..28 (trees.c _length_code; 255 -> 28)
__device__ __forceinline__ int len_code(uint32_t lc) {
  if (lc >= 255) return 28;
  if (lc < 8) return (int)lc;
  int b = 31 - __clz(lc);                       // 3..7
  return 4 * (b - 1) + (int)((lc >> (b - 2)) & 3);
}
// distance - 1 (0..32767) -> distance code 0..29 (trees.c d_code)
__device__ __forceinline__ int dist_code(uint32_t d) {
  if (d < 4) return (int)d;
  int b = 31 - __clz(d);                        // 2..14
  return 2 * b + (int)((d >> (b - 1)) & 1);
}
__device__ __forceinline__ uint32_t bitrev(uint32_t c, int n) { return __brev(c) >> (32 - n); }
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) { return *(const u32_u*)p; }

__device__ __forceinline__ uint32_t call_of(const uint32_t* starts, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;   // last call with starts[call] <= x
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (starts[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int64_t first_valid(const ZState& s) {
  return (s.total - s.base >= (uint64_t)WSIZE) ? 0 : (int64_t)WSIZE - (int64_t)(s.total - s.base);
}
// call of x in a prefix array (starts[0] = 0), searched 64 entries per step by
// the whole wave: two dependent loads for n <= 4096 instead of a 12-step chain
__device__ __forceinline__ uint32_t call_of_wave(const uint32_t* starts, uint32_t n, uint32_t x, int lane) {
  uint32_t lo = 0, span = n;   // answer in [lo, lo + span), starts[lo] <= x
  while (span > 1) {
    const uint32_t step = (span + 63) / 64;
    const uint32_t idx = lo + (uint32_t)lane * step;
    const uint64_t b = ballot(idx < lo + span && starts[idx] <= x);
    const uint32_t nlo = lo + (uint32_t)(__popcll(b) - 1) * step;
    span = std::min(step, lo + span - nlo);
    lo = nlo;
  }
  return lo;
}

#ifdef XCG_ZD_TIMING
// diagnostics build: wave cycles per phase summed over blocks (trees: histogram,
// literal tree, distance + bit-length trees, bit count, tables; emit: tables and
// header, sizing pass, packing pass; scan: loop tops, literal runs and their positions,
// cycles) and block / call counts.  One array per unit; the slots are disjoint
// by phase: trees 0-4 and 14-15, emit 8-10 (huff), scan 5-7 and 11-12 (parse).
static __device__ unsigned long long g_zd_t[16];
#define ZD_NOW() __builtin_readcyclecounter()
#define ZD_ADD(i, t0)                                                         \
  do {                                                                        \
    uint64_t t1_ = ZD_NOW();                                                  \
    if (threadIdx.x == 0) atomicAdd(&g_zd_t[i], (unsigned long long)(t1_ - (t0))); \
    t0 = t1_;                                                                 \
  } while (0)
// adds the including unit's counters to acc[16] and clears them
static inline bool zd_times_take(uint64_t* acc) {
  uint64_t t[16], z[16] = {0};
  if (hipMemcpyFromSymbol(t, HIP_SYMBOL(g_zd_t), sizeof t) != hipSuccess ||
      hipMemcpyToSymbol(HIP_SYMBOL(g_zd_t), z, sizeof z) != hipSuccess)
    return false;
  for (int i = 0; i < 16; i++) acc[i] += t[i];
  return true;
}
bool zd_parse_times(uint64_t* acc);   // xcg_zdeflate_parse.hip
bool zd_huff_times(uint64_t* acc);    // xcg_zdeflate_huff.hip
#else
#define ZD_NOW() 0ull
#define ZD_ADD(i, t0) (void)(t0)
#endif

// The launch functions, in the order a batch runs them (the driver reads
// hipGetLastError() once at the end).  xcg_zdeflate_match.hip:
void zd_launch_prep(const ZArgs& a, uint32_t maxlen, hipStream_t st);    // X = history ++ data ++ pad
void zd_launch_adler(const ZArgs& a, hipStream_t st);
void zd_launch_match(const ZArgs& a, uint32_t groups, uint32_t mtiles, hipStream_t st);   // hashes, chains, tf / tq
// xcg_zdeflate_parse.hip (mo: the mask words of the whole batch)
void zd_launch_scan(const ZArgs& a, hipStream_t st);                     // deflate_slow
void zd_launch_mfill(const ZArgs& a, uint64_t mo, hipStream_t st);       // round 0: mcur all ones, mnext clear
void zd_launch_fscan(const ZArgs& a, hipStream_t st);                    // deflate_fast, then mnext against mcur
void zd_launch_mzero(const ZArgs& a, uint64_t mo, hipStream_t st);       // mnext clear
void zd_launch_ring(const ZArgs& a, hipStream_t st);
// xcg_zdeflate_huff.hip (bo: the block records of the whole batch)
void zd_launch_huff(const ZArgs& a, uint32_t bo, hipStream_t st);        // trees, layout, emit

}  // namespace zd
}  // namespace xcg
