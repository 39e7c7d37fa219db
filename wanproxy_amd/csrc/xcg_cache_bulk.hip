// Bulk access to a memory cache: learn many segments in one call
// (XCodecPipePair's <LEARN> sequence per segment, xcodec/xcodec_pipe_pair.cc:
// 311-327: lookup; equal bytes -> nothing more, other bytes -> replace, absent
// -> enter) and export every live (hash, segment) -- what `tack -p` writes and
// reads (programs/tack/tack.cc:103-127).  DESIGN.md 3.9.
//
// The sequential definition has a closed form, and the kernels implement it
// directly:
//   - of the occurrences of one hash in the batch, the last one's bytes stand
//     (an earlier one is entered or replaced, then replaced again);
//   - an unbounded cache ends up with its earlier content plus every distinct
//     hash of the batch;
//   - a bounded cache (XCodecLRU, xcodec/xcodec_lru.h) treats every occurrence
//     as a reference at its batch position, so it ends up with the `limit`
//     most recently referenced distinct hashes of (earlier content, batch),
//     least recently referenced first.  The time of an entry the batch names is
//     its last occurrence's; the others keep theirs.
// One wave per segment hashes it (64 lanes x 32 bytes, coalesced) and enters
// (hash -> n - 1 - i) into a batch table with atomicMin: the last occurrence
// wins.  A thread per segment then classifies the winners against G, and the
// commit writes each winner's 2048 bytes once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "xcg_args.h"
#include "xcg_cache.h"

namespace xcg {

constexpr uint32_t B_SKIP = ~0u;            // slot[i]: not its hash's last occurrence, or evicted within the batch
constexpr uint32_t B_NEW = ~0u - 1u;        // a winner whose hash G does not hold
constexpr uint32_t B_PRESENT = 1u << 31;    // | pool slot: a winner whose hash G holds (slots are < 2^30)
constexpr uint64_t T_NEVER = ~0ull;
// cnt[]: device words of one call
enum : uint32_t { N_NEW = 0, N_GATE, N_FREE, N_TAKEN, N_TOTAL, N_EVICT, N_WORDS = 8 };

// A lane's 32 bytes [32 l, 32 l + 32) of the segment at p as 8 dwords.  p
// 16-byte aligned: two dwordx4 loads.  Otherwise three aligned dwordx4 loads
// from p rounded down and a byte shift (v_alignbyte_b32): every 16-byte block
// read overlaps the segment, so it lies in a page of the caller's buffer.
template <int WO>
__device__ __forceinline__ void load32_shifted(const uint8_t* base16, uint32_t sh, uint32_t* w) {
  const u32x4* q = (const u32x4*)base16;
  const u32x4 a0 = q[0], a1 = q[1], a2 = q[2];
  const uint32_t t[12] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3], a2[0], a2[1], a2[2], a2[3]};
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = __builtin_amdgcn_alignbyte(t[j + WO + 1], t[j + WO], sh);
}
__device__ __forceinline__ void seg_load32(const uint8_t* p, int l, uint32_t* w) {
  const uint32_t a = (uint32_t)(uintptr_t)p & 15u;       // (wave-uniform: every segment of a call has it)
  if (a == 0) {
    const u32x4* q = (const u32x4*)(p + 32 * l);
    const u32x4 a0 = q[0], a1 = q[1];
    w[0] = a0[0]; w[1] = a0[1]; w[2] = a0[2]; w[3] = a0[3];
    w[4] = a1[0]; w[5] = a1[1]; w[6] = a1[2]; w[7] = a1[3];
    return;
  }
  const uint8_t* b = p - a + 32 * l;
  switch (a >> 2) {
    case 0: load32_shifted<0>(b, a & 3u, w); break;
    case 1: load32_shifted<1>(b, a & 3u, w); break;
    case 2: load32_shifted<2>(b, a & 3u, w); break;
    default: load32_shifted<3>(b, a & 3u, w); break;
  }
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(256) void bulk_fill_kernel(uint64_t* keys, uint64_t* vals, uint64_t cap, uint32_t* cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (uint64_t i = i0; i < cap; i += stride) { keys[i] = EMPTY_KEY; vals[i] = ~0ull; }
  if (i0 < N_WORDS) cnt[i0] = 0u;
}

// One wave per segment: XCodecHash::hash (xcodec/xcodec_hash.h:166-174) from
// per-lane partial sums weighted as in segment_hashes_kernel (2048 - position),
// reduced over the wave; lane 0 stores it and enters it into the batch table.
__global__ __launch_bounds__(256) void bulk_hash_kernel(const uint8_t* __restrict__ segs, uint32_t n,
                                                        uint64_t* __restrict__ hash, uint64_t* __restrict__ hash_out,
                                                        HashTab b, int32_t* status) {
  const uint32_t i = blockIdx.x * 4u + readfirst(threadIdx.x >> 6);
  if (i >= n) return;
  const int l = lane_id();
  uint32_t w[8];
  seg_load32(segs + (uint64_t)i * SEG, l, w);
  uint32_t sx = 0, qx = 0, sf = 0, qf = 0;
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const uint32_t c = byte_of(w[j >> 2], j & 3);
    const uint32_t f = ffbl(c) + 1u;
    sx += c; qx += j * c; sf += f; qf += j * f;
  }
  const uint32_t wt = 2048u - 32u * l;                    // weight of the lane's first byte
  const uint32_t X1 = wave_sum(sx), X2 = wave_sum(wt * sx - qx);
  const uint32_t F1 = wave_sum(sf), F2 = wave_sum(wt * sf - qf);
  const uint32_t lo = (X1 << 20) + X2 + CLO;
  const uint32_t hi = ((F1 << 16) + F2) << 4;
  if (l == 0) {
    const uint64_t h = ((uint64_t)hi << 32) | lo;
    hash[i] = h;
    if (hash_out) hash_out[i] = h;
    if (!tab_insert_min(b, lo, hi, (uint64_t)(n - 1u - i))) atomicOr(status, 2);
  }
}

// A thread per segment: is it its hash's last occurrence, and does G hold the
// hash?  Counts the new hashes; on a bounded cache a present entry's time
// becomes this reference's.
__global__ __launch_bounds__(256) void bulk_classify_kernel(uint32_t n, const uint64_t* hash, HashTab b, HashTab g,
                                                            uint32_t* slot, uint32_t* cnt, uint64_t* lastref,
                                                            uint64_t clock) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool fresh = false;
  if (i < n) {
    const uint64_t h = hash[i];
    const uint32_t lo = (uint32_t)h, hi = (uint32_t)(h >> 32);
    uint32_t s = B_SKIP;
    if (tab_lookup_t(b, lo, hi) == (uint64_t)(n - 1u - i)) {
      const uint64_t gv = tab_lookup_t(g, lo, hi);
      fresh = gv == ~0ull;
      s = fresh ? B_NEW : ((uint32_t)gv | B_PRESENT);
      if (!fresh && lastref) lastref[gv] = clock + i;
    }
    slot[i] = s;
  }
  const uint64_t m = ballot(fresh);
  if (m && lanes_below(m) == 0 && fresh) atomicAdd(&cnt[N_NEW], (uint32_t)__builtin_popcountll(m));
}

// Unbounded: the capacity gate, before anything is written.
__global__ void bulk_gate_kernel(const uint32_t* nseg, uint32_t seg_cap, uint32_t* cnt) {
  if (threadIdx.x == 0) {
    // (the raw counter: block_alloc_segs numbers the new slots from it)
    cnt[N_GATE] = cnt[N_NEW] && (uint64_t)*nseg + cnt[N_NEW] > seg_cap ? 1u : 0u;
  }
}

// Unbounded: pool slots, table and filters of the new hashes (a thread each).
__global__ __launch_bounds__(256) void bulk_assign_kernel(uint32_t n, const uint64_t* hash, uint32_t* slot,
                                                          const uint32_t* cnt, HashTab g, FiltSet fs, uint32_t* nseg,
                                                          int32_t* status) {
  __shared__ uint32_t s_cnt, s_base;
  if (cnt[N_GATE]) return;                                // (uniform)
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool need = i < n && slot[i] == B_NEW;
  const uint32_t s = block_alloc_segs(need, nseg, &s_cnt, &s_base);
  if (!need) return;
  const uint64_t h = hash[i];
  slot[i] = s;
  if (!tab_insert_min_filt(g, fs, (uint32_t)h, (uint32_t)(h >> 32), s)) atomicOr(status, 2);
}

// One wave per winner: its 2048 bytes into its pool slot.  alive (bounded): a
// present entry is written only if it stayed (1), not if the batch evicted it
// (0) or gave its slot to a new entry (2: alive as any nonzero value is to the
// LRU passes, which set their own marks at the next commit).
__global__ __launch_bounds__(256) void bulk_copy_kernel(const uint8_t* __restrict__ segs, uint32_t n,
                                                        const uint32_t* slot, const uint32_t* cnt, uint8_t* pool,
                                                        const uint32_t* alive) {
  const uint32_t i = blockIdx.x * 4u + readfirst(threadIdx.x >> 6);
  if (i >= n || readfirst(cnt[N_GATE])) return;
  uint32_t s = readfirst(slot[i]);
  if (s == B_SKIP || s == B_NEW) return;
  if (s & B_PRESENT) {
    s &= ~B_PRESENT;
    if (alive && readfirst(alive[s]) != 1u) return;
  }
  const int l = lane_id();
  uint32_t w[8];
  seg_load32(segs + (uint64_t)i * SEG, l, w);
  u32x4* dst = (u32x4*)(pool + (uint64_t)s * SEG + 32 * l);
  dst[0] = u32x4{w[0], w[1], w[2], w[3]};
  dst[1] = u32x4{w[4], w[5], w[6], w[7]};
}

// ---- bounded: the new LRU order by one sort over (live slots, new hashes)

// Item r < C: the r-th live slot and its time (a present winner's already
// moved to its reference); item C + i: segment i if it is a new hash.
__global__ __launch_bounds__(256) void bulk_items_kernel(uint32_t n, uint32_t C, const uint32_t* nseg,
                                                         const uint32_t* queue, const uint64_t* lastref,
                                                         const uint32_t* slot, uint64_t clock, uint64_t* key,
                                                         uint32_t* val) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (uint64_t)C + n) return;
  uint64_t t = T_NEVER;
  if (k < C) {
    const uint32_t a = *nseg < C ? *nseg : C;
    uint32_t s = (uint32_t)k;
    if (k < a) { s = queue[k]; t = lastref[s]; }
    val[k] = s;
  } else {
    const uint32_t i = (uint32_t)(k - C);
    if (slot[i] == B_NEW) t = clock + i;
    val[k] = (uint32_t)k;
  }
  key[k] = t;
}

__global__ void bulk_plan_kernel(uint32_t C, uint32_t* nseg, uint32_t* cnt) {
  if (threadIdx.x == 0) {
    const uint32_t a = *nseg < C ? *nseg : C;
    const uint64_t total = (uint64_t)a + cnt[N_NEW];
    const uint32_t ev = total > C ? (uint32_t)(total - C) : 0u;
    cnt[N_TOTAL] = (uint32_t)total;                       // (n <= 2^30, C <= 2^29)
    cnt[N_EVICT] = ev;
    *nseg = (uint32_t)total - ev;
  }
}

__global__ __launch_bounds__(256) void bulk_zero32_kernel(uint32_t* p, uint32_t n) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0u;
}

// The sorted items [evict, total) stay.  Old slots among them are alive.
__global__ __launch_bounds__(256) void bulk_keep_kernel(uint32_t C, const uint32_t* cnt, const uint32_t* val,
                                                        uint32_t* alive) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < cnt[N_EVICT] || p >= cnt[N_TOTAL]) return;
  const uint32_t v = val[p];
  if (v < C) alive[v] = 1u;
}

__global__ __launch_bounds__(256) void bulk_free_kernel(uint32_t C, const uint32_t* alive, uint32_t* freel,
                                                        uint32_t* cnt) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  const bool f = s < C && !alive[s];
  const uint64_t m = ballot(f);
  uint32_t base = 0;
  if (m && lanes_below(m) == 0 && f) base = atomicAdd(&cnt[N_FREE], (uint32_t)__builtin_popcountll(m));
  base = readlane(base, m ? __builtin_ctzll(m) : 0);
  if (f) freel[base + lanes_below(m)] = s;
}

// The new order; a new hash that stays takes a free slot (any one: slot numbers
// are not observable), one the batch itself evicted is dropped.
__global__ __launch_bounds__(256) void bulk_place_kernel(uint32_t C, uint32_t* cnt, const uint64_t* key,
                                                         const uint32_t* val, const uint64_t* hash,
                                                         const uint32_t* freel, uint32_t* slot, uint64_t* skey,
                                                         uint64_t* lastref, uint32_t* alive, uint32_t* queue2) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t ev = cnt[N_EVICT];
  if (p >= cnt[N_TOTAL]) return;
  const uint32_t v = val[p];
  if (p < ev) {
    if (v >= C) slot[v - C] = B_SKIP;
    return;
  }
  uint32_t s = v;
  if (v >= C) {
    const uint32_t i = v - C;
    s = freel[atomicAdd(&cnt[N_TAKEN], 1u)];
    slot[i] = s;
    skey[s] = hash[i];
    lastref[s] = key[p];
    alive[s] = 2u;
  }
  queue2[p - ev] = s;
}

// ---- export

// Unbounded: every table entry (hash, slot), in any order; the sort orders them.
__global__ __launch_bounds__(256) void bulk_compact_kernel(HashTab g, uint32_t live, uint64_t* key, uint32_t* val,
                                                           uint32_t* cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool f = i <= g.mask && g.keys[i] != EMPTY_KEY;
  const uint64_t m = ballot(f);
  uint32_t base = 0;
  if (m && lanes_below(m) == 0 && f) base = atomicAdd(&cnt[0], (uint32_t)__builtin_popcountll(m));
  base = readlane(base, m ? __builtin_ctzll(m) : 0);
  const uint32_t o = base + lanes_below(m);
  if (f && o < live) { key[o] = g.keys[i]; val[o] = (uint32_t)g.vals[i]; }
}

// One wave per exported segment j: order[j] is its pool slot (bounded: the LRU
// queue, least recently used first; unbounded: the slots sorted by hash).
__global__ __launch_bounds__(256) void bulk_gather_kernel(uint32_t live, const uint32_t* order, const uint64_t* okey,
                                                          const uint64_t* skey, const uint8_t* __restrict__ pool,
                                                          uint8_t* __restrict__ out, uint64_t* hash_out) {
  const uint32_t j = blockIdx.x * 4u + readfirst(threadIdx.x >> 6);
  if (j >= live) return;
  const uint32_t s = readfirst(order[j]);
  const int l = lane_id();
  const u32x4* src = (const u32x4*)(pool + (uint64_t)s * SEG + 32 * l);
  const u32x4 v0 = src[0], v1 = src[1];
  uint8_t* dst = out + (uint64_t)j * SEG + 32 * l;        // (any alignment)
  *(u32x4_u*)dst = v0;
  *(u32x4_u*)(dst + 16) = v1;
  if (l == 0 && hash_out) hash_out[j] = okey ? okey[j] : skey[s];
}

}  // namespace xcg

namespace {

using xcg::grid_for;

uint64_t pow2_above(uint64_t v) {
  uint64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

// Carves one stream-ordered block into 256-byte aligned arrays.
struct Carver {
  uint8_t* base = nullptr;
  uint64_t off = 0;
  template <class T>
  T* take(uint64_t count) {
    T* p = base ? (T*)(base + off) : nullptr;
    off += (count * sizeof(T) + 255) & ~255ull;
    return p;
  }
};

size_t sort_temp_bytes(uint64_t m) {
  size_t b = 0;
  (void)rocprim::radix_sort_pairs(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                                  (uint32_t*)nullptr, (size_t)m, 0, 64);
  return b ? b : 256;
}

}  // namespace

// Learn a->n segments in order.  0; XCG_RC_OVERFLOW: an unbounded cache would have to hold
// more than its capacity (nothing written); XCG_RC_NOMEM; XCG_RC_HIP.  Asynchronous on a
// bounded cache; an unbounded one synchronises `st` once (the gate's verdict).
extern "C" int xcg_bulk_learn(const XcgBulkLearn* a, hipStream_t st) {
  using namespace xcg;
  const uint32_t n = (uint32_t)a->n;
  XcgLruState* L = a->lru;
  const uint32_t C = L ? L->C : 0u;
  const uint64_t bcap = pow2_above(2ull * n + 1024), items = (uint64_t)C + n;
  const size_t sort_bytes = L ? sort_temp_bytes(items) : 0;
  // two passes over the layout: sizes, then pointers
  StreamTemp tmp(st);
  Carver cv;
  uint64_t *hash = nullptr, *bkeys = nullptr, *bvals = nullptr, *k0 = nullptr, *k1 = nullptr;
  uint32_t *slot = nullptr, *cnt = nullptr, *v0 = nullptr, *v1 = nullptr;
  uint8_t* sort_tmp = nullptr;
  for (int pass = 0; pass < 2; ++pass) {
    cv.off = 0;
    hash = cv.take<uint64_t>(n);
    bkeys = cv.take<uint64_t>(bcap);
    bvals = cv.take<uint64_t>(bcap);
    slot = cv.take<uint32_t>(n);
    cnt = cv.take<uint32_t>(N_WORDS);
    if (L) {
      k0 = cv.take<uint64_t>(items);
      k1 = cv.take<uint64_t>(items);
      v0 = cv.take<uint32_t>(items);
      v1 = cv.take<uint32_t>(items);
      sort_tmp = cv.take<uint8_t>(sort_bytes);
    }
    if (pass == 0 && !tmp.alloc(&cv.base, cv.off)) return XCG_RC_NOMEM;
  }
  const HashTab b{bkeys, bvals, (uint32_t)(bcap - 1)}, g = tab_of(a->g);
  const FiltSet fs = filters_of(a->g);
  const dim3 waves((n + 3) / 4), threads(grid_for(n)), blk(256);
  hipLaunchKernelGGL(bulk_fill_kernel, dim3(1024), blk, 0, st, bkeys, bvals, bcap, cnt);
  hipLaunchKernelGGL(bulk_hash_kernel, waves, blk, 0, st, a->segs, n, hash, a->hash_out, b, a->status);
  hipLaunchKernelGGL(bulk_classify_kernel, threads, blk, 0, st, n, (const uint64_t*)hash, b, g, slot, cnt,
                     L ? L->lastref : (uint64_t*)nullptr, L ? L->clock : 0ull);
  if (!L) {
    hipLaunchKernelGGL(bulk_gate_kernel, dim3(1), dim3(64), 0, st, (const uint32_t*)a->g.nseg, a->g.seg_cap, cnt);
    hipLaunchKernelGGL(bulk_assign_kernel, threads, blk, 0, st, n, (const uint64_t*)hash, slot, (const uint32_t*)cnt,
                       g, fs, a->g.nseg, a->status);
    hipLaunchKernelGGL(bulk_copy_kernel, waves, blk, 0, st, a->segs, n, (const uint32_t*)slot, (const uint32_t*)cnt,
                       a->g.pool, (const uint32_t*)nullptr);
    uint32_t gate = 0;
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(&gate, cnt + N_GATE, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return XCG_RC_HIP;
    return gate ? XCG_RC_OVERFLOW : 0;
  }
  const unsigned cg = grid_for(C) < 1024 ? grid_for(C) : 1024;
  hipLaunchKernelGGL(bulk_items_kernel, dim3(grid_for(items)), blk, 0, st, n, C, (const uint32_t*)a->g.nseg,
                     (const uint32_t*)L->queue, (const uint64_t*)L->lastref, (const uint32_t*)slot, L->clock, k0, v0);
  size_t sb = sort_bytes;
  if (rocprim::radix_sort_pairs(sort_tmp, sb, k0, k1, v0, v1, (size_t)items, 0, 64, st) != hipSuccess)
    return XCG_RC_HIP;
  hipLaunchKernelGGL(bulk_plan_kernel, dim3(1), dim3(64), 0, st, C, a->g.nseg, cnt);
  hipLaunchKernelGGL(bulk_zero32_kernel, dim3(cg), blk, 0, st, L->alive, C);
  hipLaunchKernelGGL(bulk_keep_kernel, dim3(grid_for(items)), blk, 0, st, C, (const uint32_t*)cnt,
                     (const uint32_t*)v1, L->alive);
  hipLaunchKernelGGL(bulk_free_kernel, dim3(grid_for(C)), blk, 0, st, C, (const uint32_t*)L->alive, L->freel, cnt);
  hipLaunchKernelGGL(bulk_place_kernel, dim3(grid_for(items)), blk, 0, st, C, cnt, (const uint64_t*)k1,
                     (const uint32_t*)v1, (const uint64_t*)hash, (const uint32_t*)L->freel, slot, L->skey, L->lastref,
                     L->alive, L->queue2);
  hipLaunchKernelGGL(bulk_copy_kernel, waves, blk, 0, st, a->segs, n, (const uint32_t*)slot, (const uint32_t*)cnt,
                     a->g.pool, (const uint32_t*)L->alive);
  // G and its filters again from the live slots: an open-addressed table has no delete
  if (hipGetLastError() != hipSuccess || xcg_lru_rebuild_table(&a->g, L, a->status, st)) return XCG_RC_HIP;
  // the host side of the commit, as xcg_lru_commit's: the new order, and a
  // clock above every time the batch gave out (clock + i, i < n)
  uint32_t* q = L->queue;
  L->queue = L->queue2;
  L->queue2 = q;
  L->clock += (uint64_t)n + 4;
  return 0;
}

// Export `live` segments (the caller read the count and checked its room):
// asynchronous on `st`.
extern "C" int xcg_bulk_export(const XcgCacheView* gv, const XcgLruState* L, uint32_t live, uint8_t* d_segs,
                               uint64_t* d_hash, hipStream_t st) {
  using namespace xcg;
  if (live == 0) return 0;
  const dim3 waves((live + 3) / 4), blk(256);
  if (L) {
    hipLaunchKernelGGL(bulk_gather_kernel, waves, blk, 0, st, live, (const uint32_t*)L->queue,
                       (const uint64_t*)nullptr, (const uint64_t*)L->skey, (const uint8_t*)gv->pool, d_segs, d_hash);
    return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
  }
  const size_t sort_bytes = sort_temp_bytes(live);
  StreamTemp tmp(st);
  Carver cv;
  uint64_t *k0 = nullptr, *k1 = nullptr;
  uint32_t *v0 = nullptr, *v1 = nullptr, *cnt = nullptr;
  uint8_t* sort_tmp = nullptr;
  for (int pass = 0; pass < 2; ++pass) {
    cv.off = 0;
    k0 = cv.take<uint64_t>(live);
    k1 = cv.take<uint64_t>(live);
    v0 = cv.take<uint32_t>(live);
    v1 = cv.take<uint32_t>(live);
    cnt = cv.take<uint32_t>(N_WORDS);
    sort_tmp = cv.take<uint8_t>(sort_bytes);
    if (pass == 0 && !tmp.alloc(&cv.base, cv.off)) return XCG_RC_NOMEM;
  }
  const HashTab g = tab_of(*gv);
  if (hipMemsetAsync(cnt, 0, 4 * N_WORDS, st) != hipSuccess) return XCG_RC_HIP;
  hipLaunchKernelGGL(bulk_compact_kernel, dim3(grid_for((uint64_t)g.mask + 1)), blk, 0, st, g, live, k0, v0, cnt);
  size_t sb = sort_bytes;
  if (rocprim::radix_sort_pairs(sort_tmp, sb, k0, k1, v0, v1, (size_t)live, 0, 64, st) != hipSuccess) return XCG_RC_HIP;
  hipLaunchKernelGGL(bulk_gather_kernel, waves, blk, 0, st, live, (const uint32_t*)v1, (const uint64_t*)k1,
                     (const uint64_t*)nullptr, (const uint8_t*)gv->pool, d_segs, d_hash);
  return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}
