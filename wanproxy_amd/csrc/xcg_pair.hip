// XCodecCachePair (xcodec/xcodec_cache.h:140-237) of a bounded
// XCodecMemoryCache primary (:245-365, XCodecLRU xcodec/xcodec_lru.h) and an
// XCodecDisk secondary (xcodec/xcodec_cache_disk.{h,cc}): wanproxy.conf's
// cache, `memory` + `disk` under a `pair` (programs/wanproxy/wanproxy.conf:
// 8-26).  Stream-semantics encode and decode batches stay bit-exact with the
// sequential XCodecEncoder / XCodecDecoder on such a pair.  Everything --
// the pair's state and its policy -- lives on the GPU.
//
// Semantics (restated from the reference):
//   lookup(h)  primary hit: LRU use, then the disk's touch -- re-enter h if
//              the disk index lost it (:217-221, xcodec_cache_disk.cc:813-823);
//              else disk hit: enter h into the primary, evicting its LRU entry
//              at the limit (:223-227); else miss.
//   enter(h)   primary enter (may evict) and disk enter (:163-185).
//   disk       FIFO: entry number e goes to data block e mod nb*204; when an
//              index block of 204 entries fills, the write head moves to the
//              next one and the entries written there one lap earlier leave the
//              index (xcodec_cache_disk.cc:694-741, :327-382).
// A hash is visible while it is in either level.
//
// State in HBM.  Per front (one XCodecCache object): the primary's slots
// (pkey: hash, pdisk: the number of the same hash's disk entry) and its LRU
// order (lru[0 .. pcount), least recent first).  Per disk (shared by the fronts
// on it, as XCodecDisk is by its XCodecDiskCache front-ends): per data block
// the hash, the entry number written there (dent, NOENT when removed) and the
// writing front's xuid.  An entry's index block is invalidated when the write
// clock reaches 204 * (e / 204 + nb) (the write head entering that block one lap
// on), so liveness is a function of the clock and nothing is swept.  The pool
// holds C primary segments and the disk's data blocks; with HIP virtual memory
// the disk's blocks are ONE physical allocation mapped behind every front's
// primary, so `pool + id * 2048` addresses both and N fronts cost one disk.
//
// Division of work.  The parse (encode_stream_kernel, the same rounds as every
// stream batch) runs against G = one table over both levels (id s < C = primary
// slot s, id C + i = disk block i; a hash in both maps to its primary slot),
// takes per id the batch time from which the hash is gone from both levels
// (ptime) as given, and records every cache reference it makes (ENTER / HIT /
// GHIT / GMISS, xcg_cache.h).  The replay below recomputes the pair's state
// along those references with data-parallel passes instead of a sequential
// walk (tests/pair_model.py states the formulation and checks it against a
// sequential replay of the reference's policy):
//  * primary residency at a reference is an LRU stack distance: the entity of
//    reference j (previous reference p) is still in the primary iff fewer than
//    C distinct entities were referenced in (p, j), i.e. fewer than C
//    references k in (p, j) have their own previous reference before p.  The
//    primary's content at the start is a prefix of pseudo references in LRU
//    order.  Short gaps are decided by a prefix count; long ones by a block
//    table of 2-D prefix counts plus two partial block scans;
//  * evictions: the i-th miss of a full primary evicts the entity of the i-th
//    *terminal* reference (an entity's last reference before a miss of it, or
//    its last) in sequence order;
//  * the disk clock is the prefix count of appends (every enter, and every
//    primary hit on an entity whose disk entry has died: XCodecDisk::touch);
//    touches depend on the clock through the deaths, so the clock is the least
//    fixed point of "touches under this clock", reached by monotone rounds;
//  * presence at a lookup = primary residency or a live disk entry; a recorded
//    lookup that contradicts it flags its chunk, and the time each cached entity
//    leaves both levels becomes ptime for the re-parse.
// All consistent = the sequential encoder's result (by induction over stream
// time); otherwise the flagged chunks are parsed again under the new ptime.  An
// entry a sub-batch made must not leave both levels within it (the parse sees
// the batch's declarations to its end): a sub-batch writes less than a disk lap,
// which guarantees that.  The commit then places the final primary residents,
// writes the appended disk blocks and rebuilds G -- all on the device.
//
// This unit is the engine: the replay, the commit and the encode / decode
// entry points.  The two state objects it works on (XcgDiskState,
// XcgPairState: xcg_pair_state.h) are created, bound to a device, mapped (the
// pool), saved, reopened, counted and destroyed by xcg_pair_state.hip; the
// volume file (registry, index blocks and their counters, the reload, the
// clock of a reloaded ring) belongs to xcg_volume.{h,cpp}, host code only.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_radix_sort_config.hpp>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "xcg_cache.h"
#include "xcg_args.h"
#include "xcg_pair_state.h"

namespace xcg {

constexpr uint64_t NEVERT = ~0ull;       // ptime: visible to the end

// Position kinds.  A position is a pseudo reference (the primary at the start,
// LRU order) or a recorded row.
enum : uint8_t { K_PSEUDO = 0, K_ENTER = 1, K_LOOKUP = 2, K_GMISS = 3, K_SKIP = 4, K_REPL = 5 };

// The live disk entry an initial entity (id < newb) had at the pass start.
__device__ __forceinline__ uint64_t e0_of(const PairDev& d, uint32_t x) {
  uint64_t e;
  if (x < d.C) {
    e = d.pdisk[x];
  } else {
    const uint32_t i = x - d.C;
    if (d.dxuid[i] != d.xuid) return NOENT;
    e = d.dent[i];
  }
  if (e == NOENT || d.dent[e % d.D] != e || d.dclock0 >= death_of(e, d.nb)) return NOENT;
  return e;
}

__device__ __forceinline__ void mark_bad(const PairDev& d, uint64_t tm) {
  const uint32_t c = (uint32_t)(tm >> 21), t = (uint32_t)tm & 0x1FFFFFu;
  d.need[c] = 1u;
  atomicMin(d.bad_t + c, t);
  atomicMax(d.bad_hi + c, t);
  atomicAdd(&d.cnt->nbad, 1u);
}

__global__ __launch_bounds__(256) void pr_fill64_kernel(uint64_t* p, uint64_t n, uint64_t v) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    p[i] = v;
}
__global__ __launch_bounds__(256) void pr_fill32_kernel(uint32_t* p, uint64_t n, uint32_t v) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    p[i] = v;
}

__global__ __launch_bounds__(256) void pr_iota_kernel(uint32_t* p, uint32_t n, uint32_t base) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = base + i;
}

constexpr uint32_t HITMARK = 0xFFFFFFFEu;   // yent of a decode HIT row (resolved by hash)

// Encode: rows per chunk (a chunk whose list overflowed splits the sub-batch).
__global__ __launch_bounds__(256) void pr_count_kernel(PairDev d) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > d.n) return;
  if (c == d.n) { d.pcnt[c] = 0u; return; }
  const uint32_t m = d.nev[c];
  if (m > d.maxe) atomicOr(&d.cnt->split, 1u);
  d.pcnt[c] = m < d.maxe ? m : d.maxe;
}

// Pseudo references: the primary at the start, least recent first.
__global__ __launch_bounds__(256) void pr_pseudo_kernel(PairDev d) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= d.P) return;
  const uint32_t s = d.lru[r];
  d.ent[r] = s;
  d.yent[r] = NIL;
  d.kind[r] = K_PSEUDO;
  d.tim[r] = 0;
  d.hsh[r] = d.pkey[s];
  d.app[r] = 0u;
}

// Rows -> positions, one wave per chunk.  ENTER: a new entity numbered by its
// declaration row; GHIT / GMISS: the G id it found; HIT: resolved afterwards.
// Decode rows: a GHIT with the REPLACE flag (name reuse, xcodec_decoder.cc:
// 110-133) makes a new entity from the declaration row numbered with the
// ENTERs in op order; GMISS rows have no cache effect.
__global__ __launch_bounds__(256) void pr_rows_kernel(PairDev d) {
  const uint32_t c = blockIdx.x * 4u + readfirst(threadIdx.x >> 6);
  if (c >= d.n) return;
  uint32_t m;
  uint64_t rb, pb;
  if (d.dec) {
    m = (uint32_t)d.cnt64[c];
    rb = d.base64[c];
    pb = d.P + d.base64[c];
  } else {
    m = min(d.nev[c], d.maxe);
    rb = (uint64_t)c * d.maxe;
    pb = d.P + d.pbase[c];
  }
  uint32_t ndecl = 0;
  for (uint32_t k0 = 0; k0 < m; k0 += 64) {
    const uint32_t k = k0 + (uint32_t)lane_id();
    const bool valid = k < m;
    const uint4 e = valid ? d.ev[rb + k] : make_uint4(0u, 0u, 0u, 0u);
    const uint32_t kd = e.w >> 30, ref = e.w & EV_REF_MASK;
    const bool rep = d.dec && (e.z >> 31) != 0u;
    const uint32_t t = d.dec ? (e.z & 0x7FFFFFFFu) : e.z;
    const bool isdecl = valid && d.dec && (kd == EV_ENTER || (kd == EV_GHIT && rep));
    const uint64_t dm = ballot(isdecl);
    const uint32_t dnum = ndecl + __builtin_amdgcn_mbcnt_hi((uint32_t)(dm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)dm, 0u));
    ndecl += (uint32_t)__builtin_popcountll(dm);
    if (!valid) continue;
    if (k > 0 && (d.dec ? (d.ev[rb + k - 1].z & 0x7FFFFFFFu) : d.ev[rb + k - 1].z) > t) atomicOr(&d.cnt->unsorted, 1u);
    const uint64_t pos = pb + k;
    const uint64_t tm = ((uint64_t)c << 21) | t;
    d.tim[pos] = tm;
    d.hsh[pos] = ((uint64_t)e.y << 32) | e.x;
    d.yent[pos] = NIL;
    uint32_t x = NIL;
    uint8_t kk = K_SKIP;
    uint32_t a = 0u;
    if (kd == EV_ENTER) {
      if (ref < d.maxd) {
        x = d.newb + c * d.maxd + ref;
        kk = K_ENTER;
        a = 1u;
        if (!d.dec && !tab_insert_min(d.bm, e.x, e.y, pos)) atomicOr(&d.cnt->split, 2u);
      } else {
        atomicOr(&d.cnt->split, 4u);
      }
    } else if (kd == EV_HIT) {
      kk = K_LOOKUP;                                 // (entity resolved by pr_resolve_kernel)
      if (d.dec) d.yent[pos] = HITMARK;
    } else if (kd == EV_GHIT) {
      if (ref < d.newb) {
        x = ref;
        kk = K_LOOKUP;
        if (rep) {
          if (dnum < d.maxd) {
            kk = K_REPL;
            d.yent[pos] = d.newb + c * d.maxd + dnum;
            d.erep[ref] = (uint32_t)pos;
            a = 1u;
          } else {
            atomicOr(&d.cnt->split, 4u);
          }
        }
      } else if (!d.dec) {
        mark_bad(d, tm);
      }
    } else {                                         // EV_GMISS
      if (d.dec) {
        kk = K_SKIP;                                 // (decode: no cache effect)
      } else if (ref < d.newb) {
        x = ref;
        kk = K_GMISS;
      } else {
        mark_bad(d, tm);
      }
    }
    d.ent[pos] = x;
    d.kind[pos] = kk;
    d.app[pos] = a;
  }
}

// Decode definers of a hash for HIT resolution: ENTER / REPL rows (the entity
// they make) and GHIT rows (the cached entity); bm maps hash -> a chain head.
// A decode HIT resolves to the latest ENTER / REPL of its hash before it, else
// the first GHIT before it (XcgPairState's bmap: a GHIT puts only when absent,
// xcodec_decoder.cc's lookups).  Done by sorting (hash, position) pairs: see
// pr_dec_hits_kernel.
//
// Encode HIT resolution: the ENTER of the hash (the table holds the earliest;
// a second ENTER of a hash present in the sub-batch contradicts the replay).
__global__ __launch_bounds__(256) void pr_resolve_kernel(PairDev d) {
  const uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x;
  if (pos >= d.np) return;
  uint8_t kk = d.kind[pos];
  if (pos >= d.P && !d.dec) {
    const uint64_t h = d.hsh[pos];
    if (kk == K_LOOKUP && d.ent[pos] == NIL) {
      const uint64_t v = tab_lookup_t(d.bm, (uint32_t)h, (uint32_t)(h >> 32));
      if (v != ~0ull && v < pos) {
        d.ent[pos] = d.ent[v];
      } else {
        kk = K_SKIP;
        d.kind[pos] = kk;
        mark_bad(d, d.tim[pos]);
      }
    } else if (kk == K_ENTER) {
      const uint64_t v = tab_lookup_t(d.bm, (uint32_t)h, (uint32_t)(h >> 32));
      if (v != pos) {                                // a second ENTER of a hash the sub-batch holds
        kk = K_SKIP;
        d.kind[pos] = kk;
        d.app[pos] = 0u;
        mark_bad(d, d.tim[pos]);
      }
    }
  }
  if (kk != K_SKIP && d.ent[pos] >= d.etot) {        // (a decode HIT with no definer: the pass returns XCG_RC_NOTSUP)
    kk = K_SKIP;
    d.kind[pos] = kk;
  }
  const bool r = kk != K_SKIP && kk != K_GMISS;
  d.skey[pos] = kk == K_SKIP ? d.etot : d.ent[pos];
  d.sval[pos] = pos;
  d.isr[pos] = r ? 1u : 0u;
  if (pos == 0) { d.isr[d.np] = 0u; d.app[d.np] = 0u; }
}

// Segmented scans.  Runs (an entity's elements in the entity-sorted order, a
// hash's in the hash-sorted one) are numbered in ascending order, so a max-scan
// of (run << 32 | v) never carries a value across runs: an element's scan value
// belongs to its own run iff its upper half is the run's number.  v = 0 is
// "none"; indices and positions are stored + 1.
__device__ __forceinline__ uint64_t pk(uint32_t run, uint32_t v) { return ((uint64_t)run << 32) | v; }
__device__ __forceinline__ uint32_t in_run(uint64_t s, uint32_t run) { return (uint32_t)(s >> 32) == run ? (uint32_t)s : 0u; }

// Decode HIT resolution over rows sorted by (hash, position) (hk / hv, m rows):
// a HIT resolves to the latest ENTER / REPL of its hash before it, else to the
// first GHIT of the hash before it.  Step 1: run heads (-> run numbers by a
// scan); step 2: per run the first GHIT (atomicMin) and per row the packed
// latest-definer value (-> max-scan); step 3: the resolution.
__global__ __launch_bounds__(256) void pr_dh_heads_kernel(const uint64_t* hk, uint32_t m, uint32_t* head) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= m) head[i] = (i < m && (i == 0 || hk[i - 1] != hk[i])) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void pr_dh_vals_kernel(PairDev d, const uint32_t* hv, uint32_t m, const uint32_t* head,
                                                         const uint32_t* hrank, uint32_t* fg) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t r = hrank[i] + head[i] - 1u;        // this row's run
  const uint32_t q = hv[i];
  const uint8_t kq = d.kind[q];
  if (kq == K_LOOKUP && d.ent[q] != NIL && d.ent[q] < d.newb) atomicMin(fg + r, i);
  d.sa[i] = pk(r, (kq == K_ENTER || kq == K_REPL) ? i + 1u : 0u);
}
__global__ __launch_bounds__(256) void pr_dec_hits_kernel(PairDev d, const uint32_t* hv, uint32_t m, const uint32_t* head,
                                                          const uint32_t* hrank, const uint32_t* fg) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t pos = hv[i];
  if (d.kind[pos] != K_LOOKUP || d.ent[pos] != NIL) return;
  const uint32_t r = hrank[i] + head[i] - 1u;
  const uint32_t v = in_run(d.sb[i], r);
  uint32_t x = NIL;
  if (v) {
    const uint32_t q = hv[v - 1u];
    x = d.kind[q] == K_ENTER ? d.ent[q] : d.yent[q];
  } else if (fg[r] < i) {
    x = d.ent[hv[fg[r]]];
  }
  if (x == NIL) {
    atomicOr(&d.cnt->nohit, 1u);
    return;
  }
  d.ent[pos] = x;
}

// Per sorted element: the entity's previous / next reference (GMISS rows are
// not references) and the bounds of each entity's run.  prv = the latest
// non-GMISS element before it in the run (an exclusive max-scan); each
// reference's successor is written by that successor (nxt starts at -1).
__global__ __launch_bounds__(256) void pr_link_vals_kernel(PairDev d) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.np) return;
  const uint32_t e = d.sk[i];
  if (e >= d.etot) { d.sa[i] = pk(d.etot, 0u); return; }
  if (i == 0 || d.sk[i - 1] != e) d.erun[e] = i;
  if (i + 1 == d.np || d.sk[i + 1] != e) d.erend[e] = i + 1;
  d.sa[i] = pk(e, d.kind[d.sv[i]] != K_GMISS ? i + 1u : 0u);
}
__global__ __launch_bounds__(256) void pr_links_kernel(PairDev d) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.np) return;
  const uint32_t e = d.sk[i];
  if (e >= d.etot) return;
  const uint32_t pos = d.sv[i];
  const uint32_t v = in_run(d.sb[i], e);
  const int32_t p = v ? (int32_t)d.sv[v - 1u] : -1;
  d.prv[pos] = p;
  if (p >= 0 && d.kind[pos] != K_GMISS) d.nxt[p] = (int32_t)pos;
}

// Decode REPLACE rows: the new entity continues the replaced one's place in
// the primary (the slot keeps its LRU position, xcodec_cache.h:187-196), so
// for the stack distance the replaced entity's references and the new one's
// form one chain through the REPLACE row.
__global__ __launch_bounds__(256) void pr_repl_links_kernel(PairDev d) {
  const uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x;
  if (pos >= d.np || d.kind[pos] != K_REPL) return;
  const uint32_t y = d.yent[pos];
  const uint32_t i = d.erun[y];
  if (i == NIL) { d.nxt[pos] = -1; return; }
  // y's first reference (its run holds only references: HITs)
  const uint32_t q = d.sv[i];
  d.nxt[pos] = (int32_t)q;
  d.prv[q] = (int32_t)pos;
}

// Primary hits from the stack distance: short gaps by the reference count
// alone, the rest queued for the block table.
__global__ __launch_bounds__(256) void pr_hits_kernel(PairDev d) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= d.np || j < d.P) return;
  const uint8_t kk = d.kind[j];
  uint8_t h = 0;
  if (kk == K_LOOKUP || kk == K_GMISS || kk == K_REPL) {
    const int32_t p = d.prv[j];
    if (p >= 0) {
      const uint32_t between = d.rc[j] - d.rc[p + 1];
      if (between < d.C) h = 1;
      else d.slow[atomicAdd(&d.cnt->nslow, 1u)] = j;
    }
  }
  d.phit[j] = h;
}

// Block table: H[b][v] = references k in block b whose previous reference is
// in block v - 1 (v = 0: none).
__global__ __launch_bounds__(256) void pr_tab_hist_kernel(PairDev d) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= d.np || !d.isr[k]) return;
  const int32_t p = d.prv[k];
  const uint32_t v = p < 0 ? 0u : ((uint32_t)p >> d.bsh) + 1u;
  atomicAdd(d.tab + (uint64_t)(k >> d.bsh) * (d.nbk + 1) + v, 1u);
}
// Row prefix over v (inclusive), one wave per row.
__global__ __launch_bounds__(256) void pr_tab_rows_kernel(PairDev d) {
  const uint32_t b = blockIdx.x * 4u + readfirst(threadIdx.x >> 6);
  if (b >= d.nbk) return;
  uint32_t* row = d.tab + (uint64_t)b * (d.nbk + 1);
  uint32_t carry = 0;
  for (uint32_t v0 = 0; v0 <= d.nbk; v0 += 64) {
    const uint32_t v = v0 + (uint32_t)lane_id();
    const uint32_t x = v <= d.nbk ? row[v] : 0u;
    const uint32_t s = wave_incl_scan(x) + carry;
    if (v <= d.nbk) row[v] = s;
    carry = readlane(s, 63);
  }
}
// Column prefix over b (exclusive) in 32 segments: segment sums, their prefix,
// then each segment's rows.
constexpr uint32_t TSEG = 32;
__global__ __launch_bounds__(256) void pr_tab_cols_kernel(PairDev d, uint32_t* segsum, int phase) {
  const uint32_t w = d.nbk + 1;
  const uint32_t per = (d.nbk + TSEG - 1) / TSEG;
  const uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (phase == 1) {                                  // prefix over the segments, per column
    if (id >= w) return;
    uint32_t acc = 0;
    for (uint32_t s = 0; s < TSEG; ++s) {
      const uint32_t x = segsum[(uint64_t)s * w + id];
      segsum[(uint64_t)s * w + id] = acc;
      acc += x;
    }
    return;
  }
  if (id >= (uint64_t)w * TSEG) return;
  const uint32_t v = (uint32_t)(id % w), s = (uint32_t)(id / w);
  const uint32_t b0 = s * per, b1 = min(d.nbk, b0 + per);
  if (phase == 0) {
    uint32_t acc = 0;
    for (uint32_t b = b0; b < b1; ++b) acc += d.tab[(uint64_t)b * w + v];
    segsum[(uint64_t)s * w + v] = acc;
  } else {
    uint32_t acc = segsum[(uint64_t)s * w + v];
    for (uint32_t b = b0; b < b1; ++b) {
      const uint32_t x = d.tab[(uint64_t)b * w + v];
      d.tab[(uint64_t)b * w + v] = acc;
      acc += x;
    }
  }
}
// One wave per queued position j (previous reference p):
//   count = T[jb][pb] + #{m in [pb*B, p): nxt(m) < jb*B} + #{k in [jb*B, j): prv(k) < p} - rc[p + 1]
// = distinct entities referenced in (p, j); a hit iff < C.
__global__ __launch_bounds__(256) void pr_tab_query_kernel(PairDev d) {
  const uint32_t q = blockIdx.x * 4u + readfirst(threadIdx.x >> 6);
  if (q >= d.cnt->nslow) return;
  const uint32_t j = d.slow[q];
  const uint32_t p = (uint32_t)d.prv[j];
  const uint32_t jb = j >> d.bsh, pb = p >> d.bsh;
  uint32_t cnt = d.tab[(uint64_t)jb * (d.nbk + 1) + pb];
  const uint32_t lim1 = jb << d.bsh;
  for (uint32_t m = (pb << d.bsh) + (uint32_t)lane_id(); m < p + 63u; m += 64) {
    const bool ok = m < p && d.isr[m] && d.nxt[m] >= 0 && (uint32_t)d.nxt[m] < lim1;
    cnt += (uint32_t)__builtin_popcountll(ballot(ok));
  }
  for (uint32_t k = lim1 + (uint32_t)lane_id(); k < j + 63u; k += 64) {
    const bool ok = k < j && d.isr[k] && d.prv[k] < (int32_t)p;
    cnt += (uint32_t)__builtin_popcountll(ballot(ok));
  }
  cnt -= d.rc[p + 1];
  if (lane_id() == 0) d.phit[j] = cnt < d.C ? 1 : 0;
}

// The disk entry a REPLACE-made entity starts with: the REPLACE row's append
// (after the replaced entity's touch there, if any).
__device__ __forceinline__ uint64_t repl_entry(const PairDev& d, uint32_t rp) {
  return d.dclock0 + d.clk[rp] + d.tflag[rp];
}

// One fixed-point round of the disk clock.  Per entity, in stream order: the
// entity's current disk entry (the initial one, its ENTER's, or its last
// touch's) and, at every primary hit, a touch if that entry has died by the
// row's clock (XCodecDisk::touch re-enters the hash; an entry can die and be
// re-entered more than once when the sub-batch laps a small disk).  Each row
// also records the death clock of the entry current at it (presence checks).
//
// Without walking a run: the touches of an entity are a chain -- from the
// current entry (clock c), the next touch is the first element that can touch
// (nq: a primary-hit lookup / REPLACE) at or after the first element whose clock
// reaches death(c) (a binary search: clocks grow along the run).  A chain is as
// long as the entity's entries die, at most a few per sub-batch.  Then every
// row's current entry is its run's latest setter (ENTER / touch) before it: an
// exclusive max-scan (pr_touch_rows_kernel).
__global__ __launch_bounds__(256) void pr_nq_vals_kernel(PairDev d) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.np) return;
  const uint32_t e = min(d.sk[i], d.etot);
  const uint32_t pos = d.sv[i];
  const uint8_t kk = d.kind[pos];
  const bool can = e < d.etot && pos >= d.P && (kk == K_LOOKUP || kk == K_REPL) && d.phit[pos];
  d.sa[d.np - 1u - i] = pk(e, can ? i : NIL);        // (reversed: a min-scan finds the next one)
}
__global__ __launch_bounds__(256) void pr_nq_kernel(PairDev d) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.np) return;
  const uint64_t s = d.sb[d.np - 1u - i];
  d.nq[i] = (uint32_t)(s >> 32) == d.sk[i] ? (uint32_t)s : NIL;
}
__global__ __launch_bounds__(256) void pr_touch_chain_kernel(PairDev d) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= d.etot) return;
  const uint32_t i0 = d.erun[e];
  if (i0 == NIL) return;
  const uint32_t i1 = d.erend[e];
  uint64_t cur = NOENT;
  uint32_t last = NIL, start = i0;
  if (e < d.newb) {
    cur = e0_of(d, e);
  } else {
    const uint32_t p0 = d.sv[i0];
    if (d.kind[p0] == K_ENTER) {
      last = p0;
      start = i0 + 1u;
    } else {                                         // a REPLACE-made entity: its first row is a HIT
      const int32_t rp = d.prv[p0];
      if (rp >= 0 && d.kind[rp] == K_REPL) cur = repl_entry(d, (uint32_t)rp);
    }
  }
  d.einit[e] = cur;
  if (last != NIL) cur = d.dclock0 + d.clk[last];
  for (int guard = 0; guard < (1 << 20) && start < i1; ++guard) {
    const uint64_t dth = death_of(cur, d.nb);
    uint32_t lo = start, hi = i1;                    // first element whose clock reaches dth
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (d.dclock0 + d.clk[d.sv[mid]] >= dth) hi = mid; else lo = mid + 1u;
    }
    if (lo >= i1) break;
    const uint32_t j = d.nq[lo];
    if (j == NIL || j >= i1) break;
    const uint32_t pos = d.sv[j];
    d.tnew[pos] = 1u;
    cur = d.dclock0 + d.clk[pos];
    last = pos;
    start = j + 1u;
  }
  d.elast[e] = last;
}
__global__ __launch_bounds__(256) void pr_setter_vals_kernel(PairDev d) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.np) return;
  const uint32_t e = min(d.sk[i], d.etot);
  const uint32_t pos = d.sv[i];
  const bool set = e < d.etot && pos >= d.P && (d.kind[pos] == K_ENTER || d.tnew[pos]);
  d.sa[i] = pk(e, set ? d.clk[pos] + 1u : 0u);
}
__global__ __launch_bounds__(256) void pr_touch_rows_kernel(PairDev d) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t chg = 0;
  if (i < d.np) {
    const uint32_t e = d.sk[i], pos = d.sv[i];
    if (e < d.etot && pos >= d.P) {
      const uint32_t v = in_run(d.sb[i], e);
      const uint64_t cur = v ? d.dclock0 + (v - 1u) : d.einit[e];
      d.ddeath[pos] = death_of(cur, d.nb);
      const uint8_t t = d.tnew[pos];
      d.tnew[pos] = 0u;
      if (d.tflag[pos] != t) {
        d.tflag[pos] = t;
        chg = 1u;
      }
      const uint8_t kk = d.kind[pos];
      d.app[pos] = ((kk == K_ENTER || kk == K_REPL) ? 1u : 0u) + t;
    }
  }
  const uint64_t m = ballot(chg != 0u);
  if (lane_id() == 0 && m) atomicAdd(&d.cnt->changed, (uint32_t)__builtin_popcountll(m));
}

// Presence at every recorded lookup: primary residency or a live disk entry.
// Encode: a lookup the parse recorded the other way flags its chunk; a lookup
// of an entity the sub-batch made and lost again splits the sub-batch (the
// parse sees the batch's declarations to its end).  Decode: HITs only.
__global__ __launch_bounds__(256) void pr_check_kernel(PairDev d) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= d.np || j < d.P) return;
  const uint8_t kk = d.kind[j];
  if (kk != K_LOOKUP && kk != K_GMISS) return;
  if (d.dec && d.yent[j] != HITMARK) return;
  const uint32_t x = d.ent[j];
  const bool present = d.phit[j] || d.dclock0 + d.clk[j] < d.ddeath[j];
  if (d.dec || x >= d.newb) {
    if (!present) atomicOr(&d.cnt->split, 8u);
  } else if (present != (kk == K_LOOKUP)) {
    mark_bad(d, d.tim[j]);
  }
}

// Misses (references that enter the primary) and terminal references (the
// last before a miss of the same entity, or the last).
__global__ __launch_bounds__(256) void pr_missterm_kernel(PairDev d) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > d.np) return;
  uint32_t miss = 0, term = 0;
  if (k < d.np && d.isr[k]) {
    miss = k >= d.P && !d.phit[k] ? 1u : 0u;
    const int32_t nx = d.nxt[k];
    term = (nx < 0 || !d.phit[nx]) ? 1u : 0u;
  }
  d.f1[k] = miss;
  d.f2[k] = term;
}
__global__ __launch_bounds__(256) void pr_missrow_kernel(PairDev d) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < d.np && d.f1[k]) d.missrow[d.r1[k]] = k;
}

// Position at which the entity of terminal reference k is evicted (NIL: not
// in this sub-batch).  M misses, the i-th (1-based) evicts once i > C - P.
__device__ __forceinline__ uint32_t evict_pos(const PairDev& d, uint32_t k, uint32_t M) {
  const int64_t i = (int64_t)d.r2[k] + 1 + ((int64_t)d.C - (int64_t)d.P);
  return (i >= 1 && i <= (int64_t)M) ? d.missrow[i - 1] : NIL;
}

// The position whose append brings the clock to `death` (the entry is dead
// after it), or NIL when the sub-batch does not get there.
__device__ __forceinline__ uint32_t death_row(const PairDev& d, uint64_t death) {
  if (d.dclock0 + d.clk[d.np] < death) return NIL;
  uint32_t lo = d.P, hi = d.np - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (d.dclock0 + d.clk[mid + 1] >= death) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// ptime for the next parse: per id, the batch time from which the hash is in
// neither level (NEVERT: not within the sub-batch; 0: gone at its start) = the
// first position no primary span [reference, its exit) and no disk span
// [append, death) covers.  Decode: also whether anything moved (the
// classification repeats until not).
//
// Spans start at the entity's elements, which are in position order, so the
// first uncovered position is found with a max-scan instead of a walk: X(k) =
// max(P, initial coverage, ends of the spans of elements before k); the first
// element k starting past X(k) leaves a gap at X(k); without one the coverage
// ends at X after the last element.
__global__ __launch_bounds__(256) void pr_cover_kernel(PairDev d) {
  const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= d.newb) return;
  const uint64_t e0 = e0_of(d, id);
  d.ecov[id] = e0 == NOENT ? d.P : death_row(d, death_of(e0, d.nb));
  d.egap[id] = NIL;
  d.etail[id] = NIL;
}
// encoded span end: 0 none, NIL to the end, else end + 1
__device__ __forceinline__ uint32_t span_end(const PairDev& d, uint32_t pos, uint8_t kk, uint32_t M) {
  if (kk == K_GMISS) return 0u;
  if (kk == K_REPL) return NIL;                      // (gone at the REPLACE: pr_leave_kernel)
  const int32_t nx = d.nxt[pos];
  const uint32_t b = (nx >= 0 && d.phit[nx]) ? (uint32_t)nx : evict_pos(d, pos, M);
  uint32_t end = b == NIL ? NIL : b + 1u;
  if (pos >= d.P && d.tflag[pos]) {                  // a touch's disk span [touch, death)
    const uint32_t t = death_row(d, death_of(d.dclock0 + d.clk[pos], d.nb));
    end = max(end, t == NIL ? NIL : t + 1u);
  }
  return end;
}
__global__ __launch_bounds__(256) void pr_span_vals_kernel(PairDev d, uint32_t M) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.np) return;
  const uint32_t e = min(d.sk[i], d.etot);
  d.sa[i] = pk(e, e < d.newb ? span_end(d, d.sv[i], d.kind[d.sv[i]], M) : 0u);
}
__global__ __launch_bounds__(256) void pr_gaps_kernel(PairDev d, uint32_t M) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.np) return;
  const uint32_t e = d.sk[i];
  if (e >= d.newb) return;
  const uint32_t pos = d.sv[i];
  const uint32_t v = in_run(d.sb[i], e);
  uint32_t x = max(d.ecov[e], d.P);                  // (NIL: covered to the end)
  if (v) x = max(x, v == NIL ? NIL : v - 1u);
  const uint32_t own = (uint32_t)d.sa[i];            // (this element's encoded end)
  if (own && x != NIL && pos > x) atomicMin(d.egap + e, x);
  if (i + 1u == d.erend[e]) d.etail[e] = (own == 0u || x == NIL) ? x : max(x, own == NIL ? NIL : own - 1u);
}
__global__ __launch_bounds__(256) void pr_leave_kernel(PairDev d) {
  const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= d.newb) return;
  uint64_t pt = NEVERT;
  bool entity;
  if (id < d.C) {
    entity = d.pkey[id] != NOKEY;
  } else {
    const uint32_t i = id - d.C;
    const uint64_t k = d.dkey[i];
    entity = d.dxuid[i] == d.xuid && d.dent[i] != NOENT && k != NOKEY &&
             tab_lookup_t(d.g, (uint32_t)k, (uint32_t)(k >> 32)) == id;
  }
  if (entity) {
    const bool present_at_start = id < d.C || e0_of(d, id) != NOENT;
    if (!present_at_start) {
      pt = 0;
    } else {
      uint32_t lv = d.egap[id];
      if (lv == NIL) {
        const uint32_t x = d.erun[id] == NIL ? max(d.ecov[id], d.P) : d.etail[id];
        lv = x < d.np ? x : NIL;
      }
      const uint32_t rp = d.dec ? d.erep[id] : NIL;  // replaced: gone right after its own lookup
      if (rp != NIL && (lv == NIL || lv > rp)) pt = d.tim[rp] + 1;
      else if (lv != NIL) pt = d.tim[lv];
    }
  }
  if (d.ptime[id] != pt) {
    d.ptime[id] = pt;
    atomicOr(&d.cnt->changed, 1u);
  }
}

// Commit, step 1: the final primary residents -- last references that are
// terminal and not evicted -- and the slots initial residents keep.
// E = P + M - C primary evictions, M (the misses) read on the device: the
// commit needs no readback before it.
__global__ __launch_bounds__(256) void pr_final_kernel(PairDev d, const uint32_t* Mp) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > d.np) return;
  const int64_t e64 = (int64_t)d.P + (int64_t)*Mp - (int64_t)d.C;
  const uint32_t E = e64 > 0 ? (uint32_t)e64 : 0u;
  uint32_t fin = 0, nw = 0;
  if (k < d.np && d.isr[k] && d.nxt[k] < 0 && d.r2[k] >= E) {
    const uint32_t x = d.kind[k] == K_REPL ? d.yent[k] : d.ent[k];
    fin = 1u;
    if (x < d.C) d.occ[x] = 1u;
    else nw = 1u;
  }
  d.f1[k] = fin;
  d.f2[k] = nw;
}
// step 2: free slots (never used, or an initial resident's that left)
__global__ __launch_bounds__(256) void pr_free_kernel(PairDev d, const uint32_t* frank) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= d.C) return;
  if (!d.occ[s]) {
    d.freel[frank[s]] = s;
    d.pkey[s] = NOKEY;
    d.pdisk[s] = NOENT;
  }
}

__device__ __forceinline__ void add_move(const PairDev& d, uint32_t dest, uint32_t x) {
  const uint32_t j = atomicAdd(&d.cnt->nmove, 1u);
  if (x >= d.newb) {
    const uint32_t r = x - d.newb;
    d.moves[j] = make_uint4(dest, 0u, r / d.maxd, r % d.maxd);
  } else {
    d.moves[j] = make_uint4(dest, 1u, x, atomicAdd(&d.cnt->nstage, 1u));
  }
}

// The disk entry an entity holds at the end of the sub-batch (NOENT: none).
__device__ __forceinline__ uint64_t final_disk(const PairDev& d, uint32_t x, uint64_t dend) {
  uint64_t e = NOENT;
  const uint32_t la = d.elast[x];
  if (la != NIL) {
    e = d.dclock0 + d.clk[la];                       // (an ENTER's or a touch's: the row's first append)
  } else if (x >= d.newb) {                          // a REPLACE-made entity never touched
    const uint32_t i = d.erun[x];
    if (i != NIL) {
      const int32_t rp = d.prv[d.sv[i]];
      if (rp >= 0 && d.kind[rp] == K_REPL) e = repl_entry(d, (uint32_t)rp);
    }
  } else {
    e = e0_of(d, x);
  }
  return (e != NOENT && dend < death_of(e, d.nb)) ? e : NOENT;
}

// step 3: place every final resident (new LRU order; new slots from the free
// list), with its key, disk link and, for a new slot, a byte move.
__global__ __launch_bounds__(256) void pr_place_kernel(PairDev d, uint64_t dend) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= d.np || !d.f1[k]) return;
  const uint32_t x = d.kind[k] == K_REPL ? d.yent[k] : d.ent[k];
  uint32_t s;
  if (x < d.C) {
    s = x;
  } else {
    s = d.freel[d.r2[k]];
    add_move(d, s, x);
  }
  d.lru2[d.r1[k]] = s;
  d.pkey[s] = d.hsh[k];
  uint64_t fd = NOENT;
  if (x == NIL) return;
  if (d.kind[k] == K_REPL && x == d.yent[k]) {
    // new bytes under the replaced name: the append at this row after the touch (if any)
    fd = repl_entry(d, k);
    if (dend >= death_of(fd, d.nb)) fd = NOENT;
  } else {
    fd = final_disk(d, x, dend);
  }
  d.pdisk[s] = fd;
}

// step 4: the disk appends: per appending position the entry number, the data
// block, its key and owner, and a byte move -- for the last write into each
// block only (a small disk can be lapped within a sub-batch).  A REPLACE row
// appends the new entity after the replaced one's touch; the replaced entity's
// current entry leaves the index (XCodecDisk::remove).
__device__ __forceinline__ void disk_write(const PairDev& d, uint64_t e, uint64_t dend, uint64_t key, uint32_t x,
                                           bool removed) {
  if (e + d.D < dend) return;                        // (written over later in this sub-batch)
  const uint32_t i = (uint32_t)(e % d.D);
  d.dkey[i] = key;                                   // (the volume's index entry, even when removed)
  d.dent[i] = removed ? NOENT : e;
  d.dxuid[i] = d.xuid;
  if (!removed) add_move(d, d.C + i, x);
}
__global__ __launch_bounds__(256) void pr_append_kernel(PairDev d, uint64_t dend) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= d.np || j < d.P || !d.app[j]) return;
  const uint8_t kk = d.kind[j];
  uint64_t e = d.dclock0 + d.clk[j];
  const uint32_t x = d.ent[j];
  if (d.tflag[j]) {                                  // a touch of x
    const bool removed = kk == K_REPL || (d.dec && x < d.newb && d.erep[x] != NIL && d.elast[x] == j);
    disk_write(d, e, dend, d.hsh[j], x, removed);
    ++e;
  }
  if (kk == K_ENTER) disk_write(d, e, dend, d.hsh[j], x, false);
  if (kk == K_REPL) disk_write(d, e, dend, d.hsh[j], d.yent[j], false);
}

// Decode REPLACE of an entity that appended nothing in this batch: its
// initial entry leaves the index (unless this batch wrote over that block).
__global__ __launch_bounds__(256) void pr_remove_kernel(PairDev d, uint64_t dend) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= d.np || d.kind[j] != K_REPL) return;
  const uint32_t x = d.ent[j];
  if (x >= d.newb || d.elast[x] != NIL) return;
  const uint64_t e0 = e0_of(d, x);
  if (e0 == NOENT || e0 + d.D < dend) return;
  const uint32_t i = (uint32_t)(e0 % d.D);
  d.dent[i] = NOENT;                                 // (XCodecDisk::remove leaves the volume's index block as it is)
}

// Commit moves: w = (destination pool index, kind, a, b); kind 0: the bytes of
// declaration b of chunk a (input), kind 1: the pre-batch bytes of pool index a
// (staged first into staging slot b, so no move reads what another overwrote).
__global__ __launch_bounds__(256) void pair_stage_kernel(const uint4* w, const PairCnt* cnt, const uint8_t* pool,
                                                         uint8_t* staging) {
  const uint32_t j = blockIdx.x * 4u + readfirst(threadIdx.x >> 6);
  if (j >= cnt->nmove) return;
  const uint4 m = w[j];
  if (m.y != 1u) return;
  const uint8_t* src = pool + (uint64_t)m.z * SEG;
  uint8_t* dst = staging + (uint64_t)m.w * SEG;
  const int l = lane_id();
  *(u32x4_u*)(dst + 32 * l) = *(const u32x4_u*)(src + 32 * l);
  *(u32x4_u*)(dst + 32 * l + 16) = *(const u32x4_u*)(src + 32 * l + 16);
}

// Four moves per wave (MOVES_PER_WAVE): their job words, then their source
// addresses, then all eight 16-byte loads per lane are in flight before the
// first store -- one chain of round trips per four 2 KiB copies instead of one
// per copy (the commit's largest kernel: ~2 GB per GiB of C5).
constexpr uint32_t MOVES_PER_WAVE = 4;
__global__ __launch_bounds__(256) void pair_move_kernel(const uint4* w, const PairCnt* cnt, const uint8_t* in,
                                                        const uint64_t* chunk_off, const uint4* decl, uint32_t maxd,
                                                        const uint8_t* staging, uint8_t* pool) {
  const uint32_t j0 = (blockIdx.x * 4u + readfirst(threadIdx.x >> 6)) * MOVES_PER_WAVE;
  const uint32_t nm = readfirst(cnt->nmove);
  if (j0 >= nm) return;
  const int l = lane_id();
  uint4 m[MOVES_PER_WAVE];
#pragma unroll
  for (int t = 0; t < (int)MOVES_PER_WAVE; ++t) m[t] = w[min(j0 + (uint32_t)t, nm - 1u)];
  uint64_t co[MOVES_PER_WAVE];
  uint32_t dz[MOVES_PER_WAVE];
#pragma unroll
  for (int t = 0; t < (int)MOVES_PER_WAVE; ++t) {     // (kind 0: where the declaration's bytes are)
    co[t] = 0ull;
    dz[t] = 0u;
    if (m[t].y == 0u) {
      co[t] = chunk_off[m[t].z];
      dz[t] = decl[(uint64_t)m[t].z * maxd + m[t].w].z;
    }
  }
  u32x4 v[MOVES_PER_WAVE][2];
#pragma unroll
  for (int t = 0; t < (int)MOVES_PER_WAVE; ++t) {
    const uint8_t* src = m[t].y == 0u ? in + co[t] + dz[t] : staging + (uint64_t)m[t].w * SEG;
    v[t][0] = *(const u32x4_u*)(src + 32 * l);
    v[t][1] = *(const u32x4_u*)(src + 32 * l + 16);
  }
#pragma unroll
  for (int t = 0; t < (int)MOVES_PER_WAVE; ++t) {
    if (j0 + (uint32_t)t >= nm) break;
    uint8_t* dst = pool + (uint64_t)m[t].x * SEG;
    *(u32x4_u*)(dst + 32 * l) = v[t][0];
    *(u32x4_u*)(dst + 32 * l + 16) = v[t][1];
  }
}

struct PairWipe {
  HashTab g;
  uint32_t* filt;
  u32x4* ftab; uint32_t ftab_n;
  uint32_t* gfilt; uint32_t gfilt_n;
  uint32_t* nseg;
};
__global__ __launch_bounds__(256) void pair_wipe_kernel(PairWipe w) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (uint64_t i = i0; i <= w.g.mask; i += stride) { w.g.keys[i] = EMPTY_KEY; w.g.vals[i] = ~0ull; }
  for (uint64_t i = i0; i < FILT_WORDS; i += stride) w.filt[i] = 0u;
  for (uint64_t i = i0; i < w.ftab_n; i += stride) w.ftab[i] = u32x4{0u, 0u, 0u, 0u};
  for (uint64_t i = i0; i < w.gfilt_n; i += stride) w.gfilt[i] = 0u;
  if (i0 == 0) *w.nseg = 0u;
}

// G from the state: every primary slot with a hash, and every live disk entry
// of this front (a hash in both levels maps to its primary slot: the smaller id).
__global__ __launch_bounds__(256) void pair_rebuild_kernel(const uint64_t* pkey, uint32_t C, const uint64_t* dkey,
                                                           const uint64_t* dent, const uint32_t* dxuid, uint32_t D,
                                                           uint32_t nb, uint32_t xuid, uint64_t dclock, HashTab g,
                                                           FiltSet fs, uint32_t* nseg, int32_t* status) {
  const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t k = EMPTY_KEY;
  if (id < C) {
    k = pkey[id];
  } else if (id < C + D) {
    const uint32_t i = id - C;
    const uint64_t e = dent[i];
    if (dxuid[i] == xuid && e != NOENT && dclock < death_of(e, nb)) k = dkey[i];
  }
  const bool have = k != EMPTY_KEY;
  // (the table insert and the three filters with the short chain of returning
  // atomics: two round trips per key instead of about four)
  if (have && !tab_insert_min_filt(g, fs, (uint32_t)k, (uint32_t)(k >> 32), id)) atomicOr(status, 2);
  const uint64_t m = ballot(have);
  if (lane_id() == 0 && m) atomicAdd(nseg, (uint32_t)__builtin_popcountll(m));
}

// First guess of a sub-batch's references, before any parse: every chunk
// parses as its 2048-byte tiling (its cold parse), a tile found in G being a
// lookup hit, a repeat of an earlier tile of the batch a hit on that
// declaration, and every other tile a declaration, entered while the window
// 2048 bytes on (or after the last window) is examined.  One event per tile,
// in the same row format the parse records.
__global__ __launch_bounds__(256) void pair_seed_table_kernel(uint32_t n, const uint4* decl, const uint32_t* ndecl,
                                                              uint32_t maxd, HashTab b, int32_t* status) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t c = (uint32_t)(i / maxd), dd = (uint32_t)(i % maxd);
  if (c >= n || dd >= ndecl[c]) return;
  const uint4 r = decl[i];
  if (!tab_insert_min(b, r.x, r.y, ((uint64_t)c << 32) | r.z)) atomicOr(status, 2);
}
__global__ __launch_bounds__(256) void pair_seed_events_kernel(uint32_t n, const uint4* decl, const uint32_t* ndecl,
                                                               uint32_t maxd, const uint32_t* chunk_len, HashTab g,
                                                               HashTab b, uint4* ev, uint32_t* nev, uint32_t maxe,
                                                               const uint64_t* ptime) {
  const uint32_t c = blockIdx.x * 4u + readfirst(threadIdx.x >> 6);
  if (c >= n) return;
  const uint32_t nd = min(ndecl[c], maxe / 2u), last = chunk_len[c] - SEG;
  uint32_t row = 0;
  for (uint32_t k0 = 0; k0 < nd; k0 += 64) {
    const uint32_t k = k0 + (uint32_t)lane_id();
    uint4 r0 = make_uint4(0u, 0u, 0u, 0u), r1 = r0;
    uint32_t nr = 0;
    if (k < nd) {
      const uint4 dd = decl[(uint64_t)c * maxd + k];
      const uint64_t gv = tab_lookup_t(g, dd.x, dd.y);
      const uint32_t th = 2u * dd.z + 1u, te = dd.z + SEG <= last ? 2u * (dd.z + SEG) : 2u * (last + 1u);
      if (gv != ~0ull && (!ptime || ((((uint64_t)c << 21) | th) < ptime[gv]))) {
        r0 = make_uint4(dd.x, dd.y, th, (EV_GHIT << 30) | (uint32_t)gv);
        nr = 1;
      } else {
        // gone from both levels by now (with ptime: the guess before this one)
        // or never cached: a declaration if it is the batch's earliest tile of
        // the hash, or if that earliest tile found the entry before it left
        const uint64_t e = tab_lookup_t(b, dd.x, dd.y);
        bool enter = e == (((uint64_t)c << 32) | dd.z);
        if (!enter && gv != ~0ull)
          enter = ((((e >> 32) << 21) | (2u * (uint32_t)e + 1u)) < ptime[gv]);
        if (gv != ~0ull) r0 = make_uint4(dd.x, dd.y, th, (EV_GMISS << 30) | (uint32_t)gv);
        const uint4 second = enter ? make_uint4(dd.x, dd.y, te, (EV_ENTER << 30) | k)
                                   : make_uint4(dd.x, dd.y, th, EV_HIT << 30);
        if (gv != ~0ull) { r1 = second; nr = 2; }
        else { r0 = second; nr = 1; }
      }
    }
    // rows in tile order (a GMISS precedes its tile's ENTER; an ENTER at window
    // + 2048 precedes the next tile's lookup one position later)
    const uint32_t inc = wave_incl_scan(nr);
    const uint32_t o = row + inc - nr;
    if (nr > 0) ev[(uint64_t)c * maxe + o] = r0;
    if (nr > 1) ev[(uint64_t)c * maxe + o + 1] = r1;
    row += readlane(inc, 63);
  }
  if (lane_id() == 0) nev[c] = row;
}

}  // namespace xcg

// ---------------------------------------------------------------------------
// Host side: the passes' drivers (the state objects: xcg_pair_state.h).

namespace {

using namespace xcg;

// The replay's sorts (a few hundred thousand rows of 20-bit entity keys, or
// 64-bit hashes) as rocPRIM's Onesweep radix sort: a histogram, a scan and one
// pass per 8 bits.  The default config takes merge sort up to 2^20 items, ~20
// launches of block merges for a C5 sub-batch (profiles/r06_s3_*).  Both are
// stable, which the entity runs need (positions stay in order).
using PairSortCfg = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                               rocprim::default_config, 0>;

// Guesses of a sub-batch's tiling seed replayed before its first parse
// (read per sub-batch).  Default 1: on C5-PAIR-LAPS three guesses save two of
// fifteen parse passes but each costs a replay with departures (~1.2 ms per
// 2000 chunks there), 49.7 -> 46.9 GiB/s.
int pair_seed_iters() {
  const char* e = getenv("XCG_PAIR_SEED_ITERS");
  const int k = e ? atoi(e) : 1;
  return k < 1 ? 1 : (k > 8 ? 8 : k);
}

// Pass scratch for np positions, n chunks, etot entities.
int ensure_scratch(XcgPairState* P, uint64_t np, uint64_t n, uint64_t etot) {
  DevMem& m = P->mem;
  struct Arr { void** p; size_t sz; };             // a field and its bytes per element
#define ARR(f) {(void**)&P->f, sizeof(*P->f)}
  if (np + 1 > P->np_cap) {
    const uint64_t cap = std::max<uint64_t>(np + 1, P->np_cap + P->np_cap / 2);
    const Arr arrs[] = {ARR(ent), ARR(yent), ARR(kind), ARR(tim), ARR(hsh), ARR(skey), ARR(sval), ARR(sk),
                        ARR(sv), ARR(prv), ARR(nxt), ARR(isr), ARR(rc), ARR(phit), ARR(app), ARR(clk),
                        ARR(slow), ARR(f1), ARR(f2), ARR(r1), ARR(r2), ARR(missrow),
                        {(void**)&P->moves, 32},   // (two uint4 per position)
                        ARR(tflag), ARR(ddeath), ARR(sa), ARR(sb), ARR(nq), ARR(tnew)};
    for (const Arr& a : arrs) m.release(*a.p), *a.p = nullptr;
    P->np_cap = 0;
    for (const Arr& a : arrs)
      if (!m.dev(a.p, (cap + 1) * a.sz)) return XCG_RC_HIP;
    P->np_cap = cap;
  }
  if (n + 1 > P->n_cap) {
    m.release(P->pbase);
    m.release(P->pcnt);
    P->pbase = P->pcnt = nullptr;
    P->n_cap = 0;
    if (!(m.dev(&P->pbase, 4 * (n + 1)) && m.dev(&P->pcnt, 4 * (n + 1)))) return XCG_RC_HIP;
    P->n_cap = n + 1;
  }
  if (!m.grow_exact(&P->erun, &P->et_cap, etot) || !m.grow_exact(&P->elast, &P->el_cap, etot)) return XCG_RC_HIP;
  if (etot > P->ex_cap) {
    const Arr arrs[] = {ARR(erend), ARR(einit), ARR(ecov), ARR(egap), ARR(etail)};
    P->ex_cap = 0;
    for (const Arr& a : arrs) m.release(*a.p), *a.p = nullptr;
    for (const Arr& a : arrs)
      if (!m.dev(a.p, etot * a.sz + 8)) return XCG_RC_HIP;
    P->ex_cap = etot;
  }
#undef ARR
  // rocprim temporary storage for the largest sort / scan of this size
  size_t a = 0, b = 0, c = 0;
  (void)rocprim::radix_sort_pairs<PairSortCfg>(nullptr, a, P->skey, P->sk, P->sval, P->sv, (uint32_t)np, 0, 32);
  // (the commit also scans the primary's C + 1 free-slot flags, pair_commit)
  (void)rocprim::exclusive_scan(nullptr, b, P->isr, P->rc, 0u,
                                (size_t)std::max<uint64_t>(std::max<uint64_t>(np, n), P->C) + 1,
                                rocprim::plus<uint32_t>());
  (void)rocprim::radix_sort_pairs<PairSortCfg>(nullptr, c, P->hk, P->hk2, P->hv, P->hv2, (uint32_t)np, 0, 64);
  size_t e1 = 0, e2 = 0, e3 = 0;
  (void)rocprim::exclusive_scan(nullptr, e1, P->sa, P->sb, (uint64_t)0, (size_t)np + 1, rocprim::maximum<uint64_t>());
  (void)rocprim::inclusive_scan(nullptr, e2, P->sa, P->sb, (size_t)np + 1, rocprim::maximum<uint64_t>());
  (void)rocprim::inclusive_scan(nullptr, e3, P->sa, P->sb, (size_t)np + 1, rocprim::minimum<uint64_t>());
  const uint64_t want = std::max(std::max(std::max(a, b), c), std::max(std::max(e1, e2), e3)) + 256;
  return m.grow(&P->tmp, &P->tmp_cap, want, want, want, MEM_DEV) ? 0 : XCG_RC_HIP;
}

int scan_u32(XcgPairState* P, const uint32_t* in, uint32_t* out, uint64_t n, hipStream_t st) {
  size_t tb = P->tmp_cap;
  return rocprim::exclusive_scan(P->tmp, tb, in, out, 0u, (size_t)n, rocprim::plus<uint32_t>(), st) == hipSuccess
             ? 0 : XCG_RC_HIP;
}

// Segmented max / min scans of the packed (run << 32 | v) values (sa -> sb).
int scan_max_excl(XcgPairState* P, uint64_t n, hipStream_t st) {
  size_t tb = P->tmp_cap;
  return rocprim::exclusive_scan(P->tmp, tb, P->sa, P->sb, (uint64_t)0, (size_t)n, rocprim::maximum<uint64_t>(),
                                 st) == hipSuccess ? 0 : XCG_RC_HIP;
}
int scan_max_incl(XcgPairState* P, uint64_t n, hipStream_t st) {
  size_t tb = P->tmp_cap;
  return rocprim::inclusive_scan(P->tmp, tb, P->sa, P->sb, (size_t)n, rocprim::maximum<uint64_t>(), st) == hipSuccess
             ? 0 : XCG_RC_HIP;
}
int scan_min_incl(XcgPairState* P, uint64_t n, hipStream_t st) {
  size_t tb = P->tmp_cap;
  return rocprim::inclusive_scan(P->tmp, tb, P->sa, P->sb, (size_t)n, rocprim::minimum<uint64_t>(), st) == hipSuccess
             ? 0 : XCG_RC_HIP;
}

int read_small(XcgPairState* P, const void* src, size_t bytes, hipStream_t st) {
  return hipMemcpyAsync(P->h_small, src, bytes, hipMemcpyDeviceToHost, st) == hipSuccess &&
                 hipStreamSynchronize(st) == hipSuccess
             ? 0 : XCG_RC_HIP;
}
int read_cnt(XcgPairState* P, hipStream_t st) {
  return hipMemcpyAsync(P->h_cnt, P->cnt, sizeof(PairCnt), hipMemcpyDeviceToHost, st) == hipSuccess &&
                 hipStreamSynchronize(st) == hipSuccess
             ? 0 : XCG_RC_HIP;
}

// Where the rows of a pass come from.
struct RowSrc {
  int dec;
  uint32_t n, maxd;
  const uint4* ev;
  const uint32_t* nev;             // encode
  uint32_t maxe;
  const uint64_t* base64;          // decode
  const uint64_t* cnt64;
  uint64_t rows;                   // decode: rows in all
  uint32_t* need;                  // encode: per chunk flags / contradicted times
  uint32_t* bad_t;
  uint32_t* bad_hi;
};

struct PassOut {
  uint32_t nbad = 0;
  bool split = false;
  bool changed = false;            // (want_leave) ptime moved
  uint64_t appends = 0;
};

// One replay pass (see the top of this file).  want_leave: compute ptime from
// the departures even if every lookup agrees (decode, seed guesses).
int replay(XcgPairState* P, const RowSrc& rs, const HashTab& g, bool want_leave, PassOut* out, hipStream_t st) {
  XcgDiskState* K = P->disk;
  const uint32_t n = rs.n;
  const uint32_t newb = P->C + P->D;
  const uint64_t etot64 = (uint64_t)newb + (uint64_t)n * rs.maxd;
  if (etot64 >= (1ull << 31)) return XCG_RC_NOTSUP;
  const uint32_t etot = (uint32_t)etot64;
  if (!P->cnt) {
    if (!(P->mem.dev(&P->cnt, sizeof(PairCnt)) && P->mem.pinned(&P->h_cnt, sizeof(PairCnt)) &&
          P->mem.pinned(&P->h_small, 256)))
      return XCG_RC_HIP;
  }
  if (hipMemsetAsync(P->cnt, 0, sizeof(PairCnt), st) != hipSuccess) return XCG_RC_HIP;
  PairDev d{};
  d.C = P->C; d.xuid = P->xuid; d.P = P->pcount;
  d.pkey = P->pkey; d.pdisk = P->pdisk; d.lru = P->lru; d.ptime = P->ptime;
  d.D = P->D; d.nb = P->nb; d.dclock0 = K->vol.dclock;
  d.dkey = K->dkey; d.dent = K->dent; d.dxuid = K->dxuid;
  d.dec = rs.dec; d.n = n; d.maxd = rs.maxd; d.maxe = rs.maxe; d.ev = rs.ev; d.nev = rs.nev;
  d.base64 = rs.base64; d.cnt64 = rs.cnt64;
  d.newb = newb; d.etot = etot;
  d.need = rs.need; d.bad_t = rs.bad_t; d.bad_hi = rs.bad_hi;
  d.g = g;
  // rows per chunk -> positions
  uint64_t R;
  if (ensure_scratch(P, (uint64_t)P->pcount + 1, n, etot)) return XCG_RC_HIP;
  if (!rs.dec) {
    d.pbase = P->pbase;
    d.pcnt = P->pcnt;
    d.cnt = P->cnt;
    hipLaunchKernelGGL(pr_count_kernel, dim3(grid_for(n + 1)), dim3(256), 0, st, d);
    if (scan_u32(P, P->pcnt, P->pbase, (uint64_t)n + 1, st) || read_small(P, P->pbase + n, 4, st)) return XCG_RC_HIP;
    R = P->h_small[0];
  } else {
    R = rs.rows;
  }
  const uint64_t np = (uint64_t)P->pcount + R;
  if (np >= (1ull << 31)) return XCG_RC_NOTSUP;
  if (ensure_scratch(P, np, n, etot)) return XCG_RC_HIP;
  d.np = (uint32_t)np;
  d.ent = P->ent; d.yent = P->yent; d.kind = P->kind; d.tim = P->tim; d.hsh = P->hsh;
  d.skey = P->skey; d.sval = P->sval; d.sk = P->sk; d.sv = P->sv; d.prv = P->prv; d.nxt = P->nxt;
  d.isr = P->isr; d.rc = P->rc; d.phit = P->phit; d.app = P->app; d.clk = P->clk; d.slow = P->slow;
  d.f1 = P->f1; d.f2 = P->f2; d.r1 = P->r1; d.r2 = P->r2; d.missrow = P->missrow; d.moves = P->moves;
  d.pbase = P->pbase; d.pcnt = P->pcnt; d.cnt = P->cnt; d.elast = P->elast; d.tflag = P->tflag; d.ddeath = P->ddeath; d.erep = P->erep; d.erun = P->erun;
  d.lru2 = P->lru2; d.occ = P->occ; d.freel = P->freel;
  d.erend = P->erend; d.einit = P->einit; d.ecov = P->ecov; d.egap = P->egap; d.etail = P->etail;
  d.sa = P->sa; d.sb = P->sb; d.nq = P->nq; d.tnew = P->tnew;
  // encode: hash -> ENTER position
  if (!rs.dec) {
    const uint64_t want = std::max<uint64_t>(1024, 2ull << (64 - __builtin_clzll(R + 1)));
    uint64_t kc = P->bm_cap, vc = P->bm_cap;
    if (!P->mem.grow_exact(&P->bm_keys, &kc, want) || !P->mem.grow_exact(&P->bm_vals, &vc, want)) return XCG_RC_HIP;
    P->bm_cap = std::min(kc, vc);
    d.bm = HashTab{P->bm_keys, P->bm_vals, (uint32_t)(want - 1)};
    hipLaunchKernelGGL(pr_fill64_kernel, dim3(grid_for(want)), dim3(256), 0, st, P->bm_keys, want, EMPTY_KEY);
    hipLaunchKernelGGL(pr_fill64_kernel, dim3(grid_for(want)), dim3(256), 0, st, P->bm_vals, want, ~0ull);
  }
  if (hipMemsetAsync(P->tflag, 0, np + 1, st) != hipSuccess) return XCG_RC_HIP;
  if (rs.dec) hipLaunchKernelGGL(pr_fill32_kernel, dim3(grid_for(newb)), dim3(256), 0, st, P->erep, (uint64_t)newb, NIL);
  hipLaunchKernelGGL(pr_fill32_kernel, dim3(grid_for(etot)), dim3(256), 0, st, P->erun, (uint64_t)etot, NIL);
  if (P->pcount) hipLaunchKernelGGL(pr_pseudo_kernel, dim3(grid_for(P->pcount)), dim3(256), 0, st, d);
  if (n) hipLaunchKernelGGL(pr_rows_kernel, dim3((n + 3) / 4), dim3(256), 0, st, d);
  if (rs.dec && R) {                               // decode HITs: latest definer of the hash
    uint64_t c1 = P->hk_cap, c2 = P->hk_cap, c3 = P->hk_cap, c4 = P->hk_cap;
    if (!P->mem.grow_exact(&P->hk, &c1, R) || !P->mem.grow_exact(&P->hk2, &c2, R) ||
        !P->mem.grow_exact(&P->hv, &c3, R) || !P->mem.grow_exact(&P->hv2, &c4, R))
      return XCG_RC_HIP;
    P->hk_cap = std::min(std::min(c1, c2), std::min(c3, c4));
    if (hipMemcpyAsync(P->hk, P->hsh + P->pcount, 8 * R, hipMemcpyDeviceToDevice, st) != hipSuccess) return XCG_RC_HIP;
    // values: positions P .. np-1
    hipLaunchKernelGGL(pr_iota_kernel, dim3(grid_for(R)), dim3(256), 0, st, P->hv, (uint32_t)R, P->pcount);
    size_t tb = P->tmp_cap;
    if (rocprim::radix_sort_pairs<PairSortCfg>(P->tmp, tb, P->hk, P->hk2, P->hv, P->hv2, (uint32_t)R, 0, 64, st) != hipSuccess)
      return XCG_RC_HIP;
    // latest definer / first GHIT per hash run by scans (f1: run heads, f2: their prefix, r1: first GHIT)
    hipLaunchKernelGGL(pr_dh_heads_kernel, dim3(grid_for(R + 1)), dim3(256), 0, st, (const uint64_t*)P->hk2,
                       (uint32_t)R, P->f1);
    if (scan_u32(P, P->f1, P->f2, R + 1, st)) return XCG_RC_HIP;
    hipLaunchKernelGGL(pr_fill32_kernel, dim3(grid_for(R)), dim3(256), 0, st, P->r1, R, NIL);
    hipLaunchKernelGGL(pr_dh_vals_kernel, dim3(grid_for(R)), dim3(256), 0, st, d, (const uint32_t*)P->hv2,
                       (uint32_t)R, (const uint32_t*)P->f1, (const uint32_t*)P->f2, P->r1);
    if (scan_max_incl(P, R, st)) return XCG_RC_HIP;
    hipLaunchKernelGGL(pr_dec_hits_kernel, dim3(grid_for(R)), dim3(256), 0, st, d, (const uint32_t*)P->hv2,
                       (uint32_t)R, (const uint32_t*)P->f1, (const uint32_t*)P->f2, (const uint32_t*)P->r1);
  }
  hipLaunchKernelGGL(pr_resolve_kernel, dim3(grid_for(np)), dim3(256), 0, st, d);
  // entity runs: sort positions by entity (stable: positions stay in order)
  {
    const uint32_t bits = 32 - __builtin_clz(etot | 1u);
    size_t tb = P->tmp_cap;
    if (rocprim::radix_sort_pairs<PairSortCfg>(P->tmp, tb, P->skey, P->sk, P->sval, P->sv, (uint32_t)np, 0, bits, st) !=
        hipSuccess)
      return XCG_RC_HIP;
  }
  hipLaunchKernelGGL(pr_fill32_kernel, dim3(grid_for(np)), dim3(256), 0, st, (uint32_t*)P->nxt, np, NIL);
  hipLaunchKernelGGL(pr_link_vals_kernel, dim3(grid_for(np)), dim3(256), 0, st, d);
  if (scan_max_excl(P, np, st)) return XCG_RC_HIP;
  hipLaunchKernelGGL(pr_links_kernel, dim3(grid_for(np)), dim3(256), 0, st, d);
  if (rs.dec) hipLaunchKernelGGL(pr_repl_links_kernel, dim3(grid_for(np)), dim3(256), 0, st, d);
  if (scan_u32(P, P->isr, P->rc, np + 1, st)) return XCG_RC_HIP;
  hipLaunchKernelGGL(pr_hits_kernel, dim3(grid_for(np)), dim3(256), 0, st, d);
  if (read_cnt(P, st)) return XCG_RC_HIP;
  const uint32_t nslow = P->h_cnt->nslow;
  if (P->h_cnt->nohit) return XCG_RC_NOTSUP;
  if (nslow) {                                     // the block table for long gaps
    uint32_t bsh = 8;
    while ((np >> bsh) > 1024) ++bsh;
    const uint32_t nbk = (uint32_t)((np + (1ull << bsh) - 1) >> bsh);
    const uint64_t w = (uint64_t)nbk + 1;
    const uint64_t cells = (uint64_t)nbk * w + TSEG * w;
    if (!P->mem.grow_exact(&P->tab, &P->tab_cap, cells)) return XCG_RC_HIP;
    d.tab = P->tab;
    d.bsh = bsh;
    d.nbk = nbk;
    if (hipMemsetAsync(P->tab, 0, 4 * (uint64_t)nbk * w, st) != hipSuccess) return XCG_RC_HIP;
    hipLaunchKernelGGL(pr_tab_hist_kernel, dim3(grid_for(np)), dim3(256), 0, st, d);
    hipLaunchKernelGGL(pr_tab_rows_kernel, dim3((nbk + 3) / 4), dim3(256), 0, st, d);
    uint32_t* segsum = P->tab + (uint64_t)nbk * w;
    hipLaunchKernelGGL(pr_tab_cols_kernel, dim3(grid_for(w * TSEG)), dim3(256), 0, st, d, segsum, 0);
    hipLaunchKernelGGL(pr_tab_cols_kernel, dim3(grid_for(w)), dim3(256), 0, st, d, segsum, 1);
    hipLaunchKernelGGL(pr_tab_cols_kernel, dim3(grid_for(w * TSEG)), dim3(256), 0, st, d, segsum, 2);
    hipLaunchKernelGGL(pr_tab_query_kernel, dim3((nslow + 3) / 4), dim3(256), 0, st, d);
  }
  // the disk clock: monotone rounds to the least fixed point
  hipLaunchKernelGGL(pr_nq_vals_kernel, dim3(grid_for(np)), dim3(256), 0, st, d);
  if (scan_min_incl(P, np, st)) return XCG_RC_HIP;
  hipLaunchKernelGGL(pr_nq_kernel, dim3(grid_for(np)), dim3(256), 0, st, d);
  if (hipMemsetAsync(P->tnew, 0, np + 1, st) != hipSuccess) return XCG_RC_HIP;
  int rounds = 0;
  for (;; ++rounds) {
    if (scan_u32(P, P->app, P->clk, np + 1, st)) return XCG_RC_HIP;
    if (rounds >= 64) return XCG_RC_OVERFLOW;
    if (hipMemsetAsync(&P->cnt->changed, 0, 4, st) != hipSuccess) return XCG_RC_HIP;
    hipLaunchKernelGGL(pr_touch_chain_kernel, dim3(grid_for(etot)), dim3(256), 0, st, d);
    hipLaunchKernelGGL(pr_setter_vals_kernel, dim3(grid_for(np)), dim3(256), 0, st, d);
    if (scan_max_excl(P, np, st)) return XCG_RC_HIP;
    hipLaunchKernelGGL(pr_touch_rows_kernel, dim3(grid_for(np)), dim3(256), 0, st, d);
    if (read_cnt(P, st)) return XCG_RC_HIP;
    if (P->h_cnt->changed == 0) break;
  }
  hipLaunchKernelGGL(pr_check_kernel, dim3(grid_for(np)), dim3(256), 0, st, d);
  if (hipMemcpyAsync(P->h_small, P->clk + np, 4, hipMemcpyDeviceToHost, st) != hipSuccess || read_cnt(P, st))
    return XCG_RC_HIP;
  out->appends = P->h_small[0];
  out->nbad = P->h_cnt->nbad;
  out->split = P->h_cnt->split != 0 || P->h_cnt->unsorted != 0;
  P->last = d;
  P->last_ranked = false;
  P->last_appends = out->appends;
  if (pair_debug())
    fprintf(stderr, "pair-replay: dec %d n %u rows %llu P %u slow %u touch-rounds %d appends %llu bad %u split %u "
                    "unsorted %u\n", rs.dec, n, (unsigned long long)R, P->pcount, nslow, rounds,
            (unsigned long long)out->appends, out->nbad, P->h_cnt->split, P->h_cnt->unsorted);
  if (out->split) return 0;
  if (want_leave || out->nbad) {
    hipLaunchKernelGGL(pr_missterm_kernel, dim3(grid_for(np + 1)), dim3(256), 0, st, d);
    if (scan_u32(P, P->f1, P->r1, np + 1, st) || scan_u32(P, P->f2, P->r2, np + 1, st)) return XCG_RC_HIP;
    hipLaunchKernelGGL(pr_missrow_kernel, dim3(grid_for(np)), dim3(256), 0, st, d);
    if (read_small(P, P->r1 + np, 4, st)) return XCG_RC_HIP;
    P->last_M = P->h_small[0];
    P->last_ranked = true;
    if (hipMemsetAsync(&P->cnt->changed, 0, 4, st) != hipSuccess) return XCG_RC_HIP;
    hipLaunchKernelGGL(pr_cover_kernel, dim3(grid_for(newb)), dim3(256), 0, st, d);
    hipLaunchKernelGGL(pr_span_vals_kernel, dim3(grid_for(np)), dim3(256), 0, st, d, P->last_M);
    if (scan_max_excl(P, np, st)) return XCG_RC_HIP;
    hipLaunchKernelGGL(pr_gaps_kernel, dim3(grid_for(np)), dim3(256), 0, st, d, P->last_M);
    hipLaunchKernelGGL(pr_leave_kernel, dim3(grid_for(newb)), dim3(256), 0, st, d);
    if (read_cnt(P, st)) return XCG_RC_HIP;
    out->changed = P->h_cnt->changed != 0;
  }
  return 0;
}

// G from the state: wipe, then every primary slot and live own disk block.
void pair_rebuild(XcgPairState* P, const PairGpu& G, hipStream_t st) {
  const HashTab g = tab_of(G.g);
  const FiltSet fs = filters_of(G.g);
  PairWipe wp{g, fs.filt, (u32x4*)fs.ftab, fs.fmask + 1, fs.gfilt, fs.gmask + 1, G.g.nseg};
  hipLaunchKernelGGL(pair_wipe_kernel, dim3(1024), dim3(256), 0, st, wp);
  XcgDiskState* K = P->disk;
  hipLaunchKernelGGL(pair_rebuild_kernel, dim3(grid_for((uint64_t)P->C + P->D)), dim3(256), 0, st,
                     (const uint64_t*)P->pkey, P->C, (const uint64_t*)K->dkey, (const uint64_t*)K->dent,
                     (const uint32_t*)K->dxuid, P->D, P->nb, (uint32_t)P->xuid, K->vol.dclock, g, fs, G.g.nseg,
                     G.status);
  P->gclock = K->vol.dclock;
  P->gstale = false;
}

__global__ __launch_bounds__(256) void pr_notocc_kernel(const uint32_t* occ, uint32_t C, uint32_t* fl) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s <= C) fl[s] = s < C && !occ[s] ? 1u : 0u;
}

// Commit the last (consistent) pass: final primary, disk appends, bytes, G.
int pair_commit(XcgPairState* P, const PairGpu& G, hipStream_t st) {
  XcgDiskState* K = P->disk;
  PairDev d = P->last;
  const uint64_t np = d.np;
  if (ensure_front_arrays(P)) return XCG_RC_HIP;
  d.occ = P->occ; d.freel = P->freel; d.lru2 = P->lru2;
  if (!P->last_ranked) {
    hipLaunchKernelGGL(pr_missterm_kernel, dim3(grid_for(np + 1)), dim3(256), 0, st, d);
    if (scan_u32(P, P->f1, P->r1, np + 1, st) || scan_u32(P, P->f2, P->r2, np + 1, st)) return XCG_RC_HIP;
    hipLaunchKernelGGL(pr_missrow_kernel, dim3(grid_for(np)), dim3(256), 0, st, d);
    if (P->unbounded) {                            // (only this check needs M on the host)
      if (read_small(P, P->r1 + np, 4, st)) return XCG_RC_HIP;
      P->last_M = P->h_small[0];
    }
  }
  // the primary never evicts: its capacity is exceeded
  if (P->unbounded && (int64_t)d.P + (int64_t)P->last_M - (int64_t)P->C > 0) return XCG_RC_OVERFLOW;
  const uint64_t dend = K->vol.dclock + P->last_appends;
  if (hipMemsetAsync(P->occ, 0, 4ull * P->C, st) != hipSuccess ||
      hipMemsetAsync(&P->cnt->nmove, 0, 8, st) != hipSuccess)
    return XCG_RC_HIP;
  // (terminal ranks r2 are consumed by pr_final before f1 / f2 / r1 / r2 are reused)
  hipLaunchKernelGGL(pr_final_kernel, dim3(grid_for(np + 1)), dim3(256), 0, st, d, (const uint32_t*)P->r1 + np);
  if (scan_u32(P, P->f1, P->r1, np + 1, st) || scan_u32(P, P->f2, P->r2, np + 1, st)) return XCG_RC_HIP;
  hipLaunchKernelGGL(pr_notocc_kernel, dim3(grid_for(P->C + 1)), dim3(256), 0, st, (const uint32_t*)P->occ, P->C,
                     P->ofl);
  if (scan_u32(P, P->ofl, P->ofr, (uint64_t)P->C + 1, st)) return XCG_RC_HIP;
  // (before pr_free_kernel: a replaced resident's slot is freed there, and its disk link with it)
  if (d.dec) hipLaunchKernelGGL(pr_remove_kernel, dim3(grid_for(np)), dim3(256), 0, st, d, dend);
  hipLaunchKernelGGL(pr_free_kernel, dim3(grid_for(P->C)), dim3(256), 0, st, d, (const uint32_t*)P->ofr);
  hipLaunchKernelGGL(pr_place_kernel, dim3(grid_for(np)), dim3(256), 0, st, d, dend);
  hipLaunchKernelGGL(pr_append_kernel, dim3(grid_for(np)), dim3(256), 0, st, d, dend);
  if (hipMemcpyAsync(P->h_small, P->r1 + np, 4, hipMemcpyDeviceToHost, st) != hipSuccess || read_cnt(P, st))
    return XCG_RC_HIP;
  const uint32_t pc = P->h_small[0], nmove = P->h_cnt->nmove, nstage = P->h_cnt->nstage;
  if (pc > P->C) return XCG_RC_HIP;
  if (!P->mem.grow_exact(&P->staging, &P->stg_cap, (uint64_t)std::max<uint32_t>(nstage, 1) * SEG)) return XCG_RC_HIP;
  if (nmove) {
    hipLaunchKernelGGL(pair_stage_kernel, dim3((nmove + 3) / 4), dim3(256), 0, st, (const uint4*)P->moves,
                       (const PairCnt*)P->cnt, (const uint8_t*)G.g.pool, P->staging);
    hipLaunchKernelGGL(pair_move_kernel, dim3((nmove + 4 * MOVES_PER_WAVE - 1) / (4 * MOVES_PER_WAVE)), dim3(256), 0, st,
                       (const uint4*)P->moves,
                       (const PairCnt*)P->cnt, G.in, G.chunk_off, (const uint4*)G.decl, G.maxd,
                       (const uint8_t*)P->staging, G.g.pool);
  }
  std::swap(P->lru, P->lru2);
  P->pcount = pc;
  volume_advance(&K->vol, P->last_appends);          // (the clock is now dend)
  P->appends = P->last_appends;
  pair_rebuild(P, G, st);
  return hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}

int fill_ptime(XcgPairState* P, hipStream_t st) {
  hipLaunchKernelGGL(pr_fill64_kernel, dim3(1024), dim3(256), 0, st, P->ptime, (uint64_t)P->C + P->D, NEVERT);
  return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}

// Entries another front's writes retired (the clock crossed an index block
// since G was built): rebuild G before this front looks anything up.
int pair_sync_front(XcgPairState* P, const PairGpu& G, hipStream_t st) {
  XcgDiskState* K = P->disk;
  if (!P->gstale && K->vol.dclock / DISK_ENTRIES == P->gclock / DISK_ENTRIES) return 0;
  pair_rebuild(P, G, st);
  return hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}

PairGpu gpu_of(const XcgStreamArgs& a) {
  PairGpu G{};
  G.in = a.in; G.chunk_off = a.chunk_off;
  G.decl = a.decl; G.maxd = a.maxd;
  G.g = a.g;
  G.status = a.status;
  return G;
}

}  // namespace

extern "C" {

int xcg_pair_sync(XcgPairState* P, const PairGpu* G, hipStream_t st) { return pair_sync_front(P, *G, st); }

// Decode on the pair, first step: ptime NEVER everywhere.
int xcg_pair_decode_begin(XcgPairState* P, hipStream_t st) { return fill_ptime(P, st); }

// One replay of a decode batch's classified ops (rows packed per chunk at
// d_base[c], d_cnt[c] of them; `rows` total).  *same = the departure times it
// computes equal those the classification used (then it was the sequential
// decoder's).  Otherwise ptime is updated for the next classification.
// Returns 0, XCG_RC_NOTSUP (a batch the pair model declines: a hash this batch named
// gone before a later lookup, more than a disk lap of writes), XCG_RC_HIP.
int xcg_pair_decode_pass(XcgPairState* P, const PairGpu* G, const void* d_rows, const uint64_t* d_base,
                         const uint64_t* d_cnt, uint32_t n, uint64_t rows, uint32_t maxd, int* same, hipStream_t st) {
  RowSrc rs{1, n, maxd, (const uint4*)d_rows, nullptr, 0u, d_base, d_cnt, rows, nullptr, nullptr, nullptr};
  PassOut o;
  const HashTab g = tab_of(G->g);
  const int rc = replay(P, rs, g, true, &o, st);
  if (rc) return rc;
  if (o.split) return XCG_RC_NOTSUP;
  *same = !o.changed;
  return 0;
}

// Keep the last decode replay and commit it (bytes from the batch input at the
// declaration rows: G.decl[c * maxd + d].z = the EXTRACT payload's offset).
int xcg_pair_decode_commit(XcgPairState* P, const PairGpu* G, hipStream_t st) {
  const int rc = pair_commit(P, *G, st);
  if (fill_ptime(P, st)) return XCG_RC_HIP;
  return rc;
}

// Stream-semantics encode of a batch on the pair, in sub-batches (see the top
// of this file).  Returns 0, XCG_RC_OVERFLOW (no consistent pass / overflow), XCG_RC_NOTSUP (one
// chunk alone exceeds what a sub-batch may hold), XCG_RC_HIP.
int xcg_pair_encode_stream(const XcgStreamArgs* a0, XcgPairState* P, int* rounds_out, hipStream_t st) {
  const uint32_t n = a0->n;
  int rounds = 0;
  if (pair_sync_front(P, gpu_of(*a0), st)) return XCG_RC_HIP;
  // A sub-batch is bounded by the disk only: while it writes fewer than a lap
  // of disk blocks, nothing it declared can leave both levels within it (a
  // chunk writes at most maxd declarations plus its touches).
  const uint64_t lap = P->D > 2 * DISK_ENTRIES ? P->D - 2 * DISK_ENTRIES : 1;
  // (maxd writes per chunk at most; the rate a previous sub-batch measured is
  // used when it allows more -- a sub-batch that still laps the disk is split)
  uint32_t per = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, std::max<uint64_t>(lap / a0->maxd, P->fit_per)));
  constexpr int MAX_PASSES = 12;
  uint32_t i0 = 0;
  using clk = std::chrono::steady_clock;
  auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  const HashTab g = tab_of(a0->g);
  while (i0 < n) {
    const clk::time_point t0 = clk::now();
    // what is left in equal parts of at most `per` chunks (no short tail
    // sub-batch: each costs a replay and a commit whatever its size)
    const uint32_t rem = n - i0, parts = (rem + per - 1) / per;
    const uint32_t m = (rem + parts - 1) / parts;
    XcgStreamArgs a = *a0;
    a.n = m;
    a.chunk_off += i0;
    a.chunk_len += i0;
    a.out_off += i0;
    a.out_len += i0;
    if (a.stats) a.stats += 4ull * i0;
    a.ptime = P->ptime;
    a.no_commit = 1;
    RowSrc rs{0, m, a.maxd, (const uint4*)a.ev, a.nev, a.maxe, nullptr, nullptr, 0, a.need, a.bad_t, a.bad_hi};
    auto clear_flags = [&]() {
      return hipMemsetAsync(a.need, 0, 4ull * m, st) == hipSuccess &&
             (!a.bad_t || (hipMemsetAsync(a.bad_t, 0xFF, 4ull * m, st) == hipSuccess &&
                           hipMemsetAsync(a.bad_hi, 0, 4ull * m, st) == hipSuccess));
    };
    StreamTemp flags_tmp(st);                        // (freed on `st` when the sub-batch is done, or fails)
    uint32_t* scratch_flags = nullptr;
    if (!a.bad_t) {                                  // (no restart arrays: flags into scratch)
      if (!flags_tmp.alloc(&scratch_flags, 8ull * m)) return XCG_RC_HIP;
      rs.bad_t = scratch_flags;
      rs.bad_hi = scratch_flags + m;
    }
    // The rounds start from each chunk's tiling (its cold parse).  ptime is
    // NEVER (no cached entry leaves) unless the last sub-batch needed more than
    // one pass: then the first guess is the tiling seed's own references,
    // replayed (a cached tile is a lookup hit, a repeat of an earlier tile a hit
    // on its declaration, every other tile a declaration).
    if (xcg_launch_seed_tiling(&a, st)) return XCG_RC_HIP;
    const clk::time_point t1 = clk::now();
    if (P->prev_passes > 1) {
      const HashTab b{a.b_keys, a.b_vals, a.b_mask};
      hipLaunchKernelGGL(pr_fill64_kernel, dim3(1024), dim3(256), 0, st, b.keys, (uint64_t)b.mask + 1, EMPTY_KEY);
      hipLaunchKernelGGL(pr_fill64_kernel, dim3(1024), dim3(256), 0, st, b.vals, (uint64_t)b.mask + 1, ~0ull);
      hipLaunchKernelGGL(pair_seed_table_kernel, dim3(grid_for((uint64_t)m * a.maxd)), dim3(256), 0, st, m,
                         (const uint4*)a.decl, (const uint32_t*)a.ndecl, a.maxd, b, a.status);
      // guess 0 takes every cached tile for a hit; each further guess
      // classifies against the departure times the one before implies
      // (XCG_PAIR_SEED_ITERS)
      const int iters = pair_seed_iters();
      for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(pair_seed_events_kernel, dim3((m + 3) / 4), dim3(256), 0, st, m, (const uint4*)a.decl,
                           (const uint32_t*)a.ndecl, a.maxd, a.chunk_len, g, b, (uint4*)a.ev, a.nev, a.maxe,
                           it ? (const uint64_t*)P->ptime : nullptr);
        if (!clear_flags()) return XCG_RC_HIP;
        PassOut o;
        const int rc = replay(P, rs, g, true, &o, st);
        if (rc) return rc;
        if (o.split) break;                        // (a guess the replay declines: keep the last times)
      }
    }
    const clk::time_point t2 = clk::now();
    double t_parse = 0, t_replay = 0;
    bool done = false, split = false;
    int passes = 0;
    for (int pass = 0; pass < MAX_PASSES && !done && !split; ++pass) {
      ++passes;
      a.keep_decls = 1;
      a.need_given = pass > 0;
      int r = 0;
      const clk::time_point q0 = clk::now();
      const int rc = xcg_launch_encode_stream(&a, &r, st);
      rounds += r;
      if (rc) return rc;
      if (pair_debug()) (void)hipStreamSynchronize(st);
      const clk::time_point q1 = clk::now();
      if (!clear_flags()) return XCG_RC_HIP;
      PassOut o;
      const int prc = replay(P, rs, g, false, &o, st);
      if (prc == XCG_RC_OVERFLOW) { split = true; break; }
      if (prc) return prc;
      const clk::time_point q2 = clk::now();
      t_parse += ms(q0, q1);
      t_replay += ms(q1, q2);
      if (pair_debug())
        fprintf(stderr, "pair: chunks %u+%u pass %d rounds %d appends %llu bad %u split %d\n", i0, m, pass, r,
                (unsigned long long)o.appends, o.nbad, (int)o.split);
      if (o.split) split = true;
      else if (o.nbad == 0) done = true;
      // else: the replay flagged the chunks (need / bad_t / bad_hi) and set ptime
    }
    if (!done) {
      if (m == 1) return split ? XCG_RC_NOTSUP : XCG_RC_OVERFLOW;
      per = m / 2;                                 // redo this part in halves
      P->fit_per = 0;                              // (and size the next call from the worst case again)
      P->prev_passes = MAX_PASSES;
      if (fill_ptime(P, st)) return XCG_RC_HIP;
      continue;
    }
    const clk::time_point t3 = clk::now();
    const PairGpu G = gpu_of(a);
    if (const int crc = pair_commit(P, G, st)) return crc == XCG_RC_OVERFLOW ? XCG_RC_OVERFLOW : XCG_RC_HIP;
    if (pair_debug())
      fprintf(stderr, "pair: ms seed %.2f seed-replay %.2f parse %.2f replay %.2f commit %.2f (primary %u, clock %llu)\n",
              ms(t0, t1), ms(t1, t2), t_parse, t_replay, ms(t3, clk::now()), P->pcount,
              (unsigned long long)P->disk->vol.dclock);
    // the next sub-batch starts with every hash visible to its end
    if (fill_ptime(P, st)) return XCG_RC_HIP;
    P->last_base = i0;
    P->prev_passes = passes;
    i0 += m;
    // size the next sub-batch from the disk blocks this one wrote
    const uint64_t useD = P->appends;
    uint64_t want = (uint64_t)n;
    if (useD) {
      want = std::min<uint64_t>(want, lap * 9 / 10 * m / useD);
      P->fit_per = (uint32_t)std::min<uint64_t>(lap * 9 / 10 * m / useD, 1u << 30);
    }
    per = (uint32_t)(want < 1 ? 1 : (want > n ? n : want));
  }
  if (rounds_out) *rounds_out = rounds;
  return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}

}  // extern "C"
