// The pair's two state objects (one XCodecDisk, one XCodecCachePair front on
// it) and what the units that work on them share: xcg_pair_state.hip creates,
// maps, saves, reopens, counts and destroys them, xcg_pair.hip runs the replay
// and the commit on them.  The volume file's format is neither's: xcg_volume.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <vector>

#include "xcg_args.h"
#include "xcg_cache.h"
#include "xcg_volume.h"

namespace xcg {

constexpr uint32_t NIL = 0xFFFFFFFFu;

struct PairCnt {                          // device counters of one pass
  uint32_t split;                         // a row list overflowed: a smaller sub-batch
  uint32_t nbad;                          // recorded lookups the replay contradicts
  uint32_t unsorted;                      // a chunk's rows out of time order
  uint32_t changed;                       // touches moved (fixed-point round) / ptime moved (decode)
  uint32_t nslow;                         // stack-distance queries for the block table
  uint32_t nmove, nstage, nomiss;         // commit moves, staged moves
  uint32_t nohit;                         // (decode) a HIT with no earlier definer
  uint32_t pad[7];
};

struct PairDev {
  // the front
  uint32_t C, xuid, P;                    // limit, front id, primary entries at the start
  uint64_t* pkey;                         // [C]
  uint64_t* pdisk;                        // [C] number of the same hash's disk entry (NOENT)
  const uint32_t* lru;                    // [P] slots, least recent first
  uint64_t* ptime;                        // [C + D]
  // the disk
  uint32_t D, nb;
  uint64_t dclock0;
  uint64_t* dkey;                         // [D]
  uint64_t* dent;                         // [D]
  uint32_t* dxuid;                        // [D]
  // rows
  int dec;                                // decode rows (packed, REPLACE flags) vs encode rows
  uint32_t n, maxd, maxe;
  const uint4* ev;
  const uint32_t* nev;                    // encode: rows per chunk
  const uint64_t* base64;                 // decode: row base per chunk
  const uint64_t* cnt64;                  // decode: rows per chunk
  uint32_t* pbase;                        // encode: position base per chunk (exclusive scan) [n + 1]
  uint32_t* pcnt;                         // encode: rows per chunk [n + 1]
  // positions [np)
  uint32_t newb, etot, np;
  uint32_t* ent;                          // entity (decode REPL rows: the replaced entity)
  uint32_t* yent;                         // decode REPL rows: the new entity (else NIL)
  uint8_t* kind;
  uint64_t* tim;                          // stream time (chunk << 21 | t)
  uint64_t* hsh;
  uint32_t* skey;                         // sort input keys (entity, etot = none) / values (position)
  uint32_t* sval;
  uint32_t* sk;                           // sorted
  uint32_t* sv;
  int32_t* prv;                           // previous reference of the same entity (-1)
  int32_t* nxt;                           // next reference (-1)
  uint32_t* isr;                          // 1: a reference [np + 1]
  uint32_t* rc;                           // exclusive prefix of isr [np + 1]
  uint8_t* phit;                          // primary hit (a lookup / GMISS whose entity is resident)
  uint32_t* app;                          // appends at the position [np + 1]
  uint32_t* clk;                          // exclusive prefix of app [np + 1]
  uint32_t* elast;                        // [etot] position of the entity's last append (NIL)
  uint8_t* tflag;                         // [np] a touch at the position
  uint64_t* ddeath;                       // [np] death clock of the entity's disk entry current at the row
  uint32_t* erep;                         // [newb] (decode) position of the REPLACE that ends it (NIL)
  uint32_t* erun;                         // [etot] sorted index of the entity's first element (NIL)
  uint32_t* erend;                        // [etot] one past its last element
  uint64_t* einit;                        // [etot] disk entry current before the entity's first element
  uint32_t* ecov;                         // [etot] (leave) initial coverage end (NIL: to the end)
  uint32_t* egap;                         // [etot] (leave) first uncovered position found at a span start
  uint32_t* etail;                        // [etot] (leave) coverage end after the entity's last element
  uint64_t* sa;                           // [np + 1] segmented-scan input / output
  uint64_t* sb;
  uint32_t* nq;                           // [np + 1] next element of the run that can touch (NIL)
  uint8_t* tnew;                          // [np + 1] touches of the running round
  uint32_t* slow;                         // positions for the block table
  uint32_t* tab;                          // [nbk * (nbk + 1)] 2-D prefix counts
  uint32_t bsh, nbk;                      // table block = 1 << bsh positions
  uint32_t* f1;                           // misses / final residents [np + 1]
  uint32_t* f2;                           // terminals / new residents [np + 1]
  uint32_t* r1;                           // exclusive prefixes [np + 1]
  uint32_t* r2;
  uint32_t* missrow;                      // position of the i-th miss
  uint32_t* occ;                          // [C] slot kept / free list
  uint32_t* freel;                        // [C]
  uint32_t* lru2;                         // [C] the next LRU order
  uint4* moves;                           // commit moves
  PairCnt* cnt;
  HashTab bm;                             // hash -> ENTER position (encode)
  HashTab g;                              // the front's G (leave: which disk blocks are entities)
  uint32_t* need;                         // per chunk: flagged; earliest / latest contradicted time
  uint32_t* bad_t;
  uint32_t* bad_hi;
};

// The clock at which disk entry e leaves the index: the write head enters its index block one lap on.
__device__ __forceinline__ uint64_t death_of(uint64_t e, uint32_t nb) {
  return e == NOENT ? 0ull : (uint64_t)DISK_ENTRIES * (e / DISK_ENTRIES + nb);
}

}  // namespace xcg

struct XcgPairState;

// One XCodecDisk: the ring's blocks (device arrays) and the fronts on it.
struct XcgDiskState {
  xcg::DevMem mem;                 // the ring's device arrays
  xcg::Volume vol;                 // geometry, registry, index-block counters, the disk clock; a reopened file's ring
  int device = -1;                 // bound by the first front
  uint64_t* dkey = nullptr;
  uint64_t* dent = nullptr;
  uint32_t* dxuid = nullptr;
  // the data blocks' bytes: one physical allocation mapped behind every front's primary
  uint32_t flags = 0;              // XCG_DISK_* (xcgpu.h)
  int tier = -1;                   // where the blocks live: 0 HBM, 1 pinned host memory (-1: not yet)
  bool vmm = false;
  hipMemGenericAllocationHandle_t pool_h{};
  size_t pool_bytes = 0;
  void* dva = nullptr;             // the disk's own mapping of pool_h, for its whole life (xcg_disk_save)
  std::vector<XcgPairState*> fronts;   // by xuid (nullptr: free)
  // a reopened volume's ring (vol.h_*), waiting for the first front's device
  bool pending = false;
  bool ring_loaded = false;
  bool zeroed = false;             // a fresh volume's blocks read as zeros (as the reference's ftruncate'd file)
  // without HIP virtual memory every front has its own copy of the blocks: a
  // front that goes away leaves the blocks it wrote here (shadow_ok: per block)
  std::vector<uint8_t> shadow, shadow_ok;
  int refs = 1;                    // the creator's reference + one per front
};

struct XcgPairState {
  xcg::DevMem mem;                 // the front's arrays, the pass scratch, a pool without virtual memory
  uint32_t C = 0;                  // primary limit in segments
  // XCodecCachePair over an unbounded XCodecMemoryCache (limit 0: enter never
  // evicts, xcodec_cache.h:303-318): C is then only the primary's capacity,
  // and a commit that would evict fails (XCG_EOVERFLOW) instead
  bool unbounded = false;
  uint32_t D = 0, nb = 0;
  XcgDiskState* disk = nullptr;
  uint16_t xuid = 0;
  uint32_t pcount = 0;             // primary entries
  uint64_t gclock = 0;             // disk clock when G was last rebuilt
  bool gstale = false;
  // device state
  uint64_t* pkey = nullptr;        // [C]
  uint64_t* pdisk = nullptr;       // [C]
  uint32_t* lru = nullptr;         // [C]
  uint32_t* lru2 = nullptr;        // [C]
  uint64_t* ptime = nullptr;       // [C + D]
  // the pool (C primary segments, then the disk's blocks)
  uint8_t* pool = nullptr;
  bool pool_vmm = false;
  void* va = nullptr;
  size_t va_bytes = 0, prim_bytes = 0;
  hipMemGenericAllocationHandle_t prim_h{};
  // pass scratch, grown on demand
  uint64_t np_cap = 0, n_cap = 0, et_cap = 0, tab_cap = 0, stg_cap = 0, tmp_cap = 0, bm_cap = 0, hk_cap = 0;
  uint32_t* ent = nullptr; uint32_t* yent = nullptr; uint8_t* kind = nullptr; uint64_t* tim = nullptr;
  uint64_t* hsh = nullptr; uint32_t* skey = nullptr; uint32_t* sval = nullptr; uint32_t* sk = nullptr;
  uint32_t* sv = nullptr; int32_t* prv = nullptr; int32_t* nxt = nullptr; uint32_t* isr = nullptr;
  uint32_t* rc = nullptr; uint8_t* phit = nullptr; uint32_t* app = nullptr; uint32_t* clk = nullptr;
  uint32_t* slow = nullptr; uint32_t* f1 = nullptr; uint32_t* f2 = nullptr; uint32_t* r1 = nullptr;
  uint32_t* r2 = nullptr; uint32_t* missrow = nullptr; uint4* moves = nullptr;
  uint32_t* pbase = nullptr;       // [n + 1]
  uint32_t* pcnt = nullptr;        // [n + 1]
  uint32_t* elast = nullptr;       // [etot]
  uint64_t el_cap = 0;
  uint8_t* tflag = nullptr;        // [np]
  uint64_t* ddeath = nullptr;      // [np]
  uint32_t* erep = nullptr;        // [C + D]
  uint32_t* erun = nullptr;        // [etot]
  uint32_t* erend = nullptr;       // [etot]
  uint64_t* einit = nullptr;       // [etot]
  uint32_t* ecov = nullptr; uint32_t* egap = nullptr; uint32_t* etail = nullptr;   // [etot]
  uint64_t* sa = nullptr; uint64_t* sb = nullptr;   // [np + 1] segmented scans
  uint32_t* nq = nullptr;          // [np + 1]
  uint8_t* tnew = nullptr;         // [np + 1]
  uint64_t ex_cap = 0;
  uint32_t* tab = nullptr;         // block table + its segment sums
  uint32_t* occ = nullptr; uint32_t* freel = nullptr; uint32_t* ofl = nullptr; uint32_t* ofr = nullptr;
  uint64_t* hk = nullptr; uint64_t* hk2 = nullptr; uint32_t* hv = nullptr; uint32_t* hv2 = nullptr;
  uint64_t* bm_keys = nullptr; uint64_t* bm_vals = nullptr;
  uint8_t* staging = nullptr;
  void* tmp = nullptr;
  xcg::PairCnt* cnt = nullptr;
  uint32_t* h_small = nullptr;     // pinned: small readbacks
  xcg::PairCnt* h_cnt = nullptr;   // pinned
  // the last pass (kept for the commit)
  xcg::PairDev last{};
  uint32_t last_M = 0;
  bool last_ranked = false;
  uint64_t last_appends = 0;
  // sub-batch bookkeeping
  uint64_t appends = 0;            // disk blocks the last committed sub-batch wrote
  uint32_t last_base = 0;
  int prev_passes = 1;
  // chunks per sub-batch the last committed sub-batch's disk writes imply (90 %
  // of a lap at its rate; 0: none yet); the next call starts from it
  uint32_t fit_per = 0;
};

namespace xcg {

inline bool pair_debug() {
  static const bool on = getenv("XCG_PAIR_DEBUG") != nullptr;
  return on;
}

// The primary's arrays must outlive one replay; the commit's slot arrays too.
int ensure_front_arrays(XcgPairState* P);

}  // namespace xcg
