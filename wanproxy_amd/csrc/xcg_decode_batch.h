// The batch decoder's shared pieces (xcg_decode.hip: the stream-batch passes;
// xcg_decode_bounded.hip: the bounded-cache and pair classification;
// xcg_decode_small.hip: one decode() call in one workgroup): the kernels'
// parameter block, the device helpers more than one of these units needs, and
// the host entry points they reach each other through.  Device code as in
// xcg_decode_ops.h: one wave64 per call.
#pragma once
#include "xcg_args.h"
#include "xcg_cache.h"
#include "xcg_decode_ops.h"   // next_op, wave_unescape, dec_window_hash, wave_copy2048, be64
#include "xcg_decode_words.h"

namespace xcg {

struct WinView;

struct DecParams {
  const uint8_t* in;           // encoded chunks
  const uint64_t* chunk_off;
  const uint32_t* chunk_len;
  uint32_t n;
  HashTab g;                   // persistent cache
  const uint8_t* pool;
  HashTab x;                   // batch EXTRACT table: hash -> (earliest, latest) packed positions
  uint64_t* x_latest;          // parallel to x.vals: latest position (atomicMax)
  // ---- name reuse
  uint64_t* x_owner;           // parallel to x.vals: position of the EXTRACT that claimed the slot
  uint32_t* x_flag;            // parallel: 1 = the hash's EXTRACTs differ in bytes (valid when the batch has duplicates)
  uint64_t* dup_ctr;           // duplicates listed so far, minus one (starts at ~0: cleared with the stop positions)
  uint32_t* dup_slot;          // every EXTRACT after the one that claimed its hash's slot: (slot, position)
  uint64_t* dup_pos;
  uint32_t dup_cap;
  uint32_t* nconf;             // flagged hashes
  const uint64_t* occ_key;     // (REUSE) EXTRACTs of the flagged hashes sorted by (hash, position), padded
  const uint64_t* occ_pos;     //   with (~0, ~0) to nocc entries
  uint32_t nocc;
  uint64_t* out_len;           // scan: tentative decoded length; emit: final
  const uint64_t* out_off;     // emit: exclusive scan of scan's out_len
  uint8_t* out;
  int32_t* chunk_status;       // 0 ok, 1 blocked (unknown REF), 2 not reached, 3 partial op at end, <0 error
  uint64_t* consumed;          // input bytes fully parsed per chunk
  uint64_t* unknown;           // emit: unresolvable REFs (hash), with their positions
  uint64_t* unknown_pos;
  uint32_t* nunknown;
  uint32_t unknown_cap;
  uint64_t* block_pos;         // min stream position of an unresolvable REF (atomicMin)
  int32_t* status;             // bit 9: EXTRACT name reuse inside the batch
  // ---- BACKREF window
  uint64_t* berr_pos;          // min stream position of a BACKREF to an empty slot (atomicMin); on a bounded or
                               //   pair context also the classification's cap: ops behind it have no cache effect
  uint64_t* n_decl;            // scan: declares (EXTRACT + REF) per chunk
  uint64_t* n_bref;            // scan: BACKREFs per chunk
  const uint64_t* decl_base;   // exclusive scan of n_decl: batch index of the chunk's first declare
  uint64_t* n_decl_emit;       // emit: declares made before the chunk stopped
  uint64_t* t_end;             // declares of the batch before the stop point
  uint4* D;                    // declare records (lo, hi, src lo, src hi), batch indices [D_lo, ...)
  uint64_t D_lo;               // (tail mode: D_lo = max(t_end - 256, 0), read from *t_end)
  bool D_tail;
  // (emit, no stop point) the window's tail records written by the emit pass
  // itself: declares [tail_lo, tail_hi) into tail_D (null: decl_record_kernel)
  uint4* tail_D;
  uint64_t tail_lo, tail_hi;
  uint64_t* win_hash;          // the decoder's window: 256 hashes (0 = empty slot)
  uint8_t* win_seg;            //   and the bytes of each slot
  uint64_t win_count;          // declares made before this batch
  // ---- bounded cache (xcg_lru.hip): a persistent entry serves a lookup at
  // stream time (chunk << 21 | op offset) only before ptime[slot]
  const uint64_t* ptime;
  uint64_t* u_keys;            // unknown-hash set (EMPTY_KEY = free)
  uint32_t u_mask;
  // ---- one window per decoder (xcg_decode_windows.hip; null on the one-window
  // path).  decl_base is then each chunk's base among its own window's
  // declares, and D holds the records window-major (full: window w's declare t
  // at wins[w].first + t) or 256 per window (tail: at 256 w + t - lo_w).
  WinView* wins;               // [n_windows]
  const uint32_t* chunk_win;   // chunk -> window
  uint64_t* w_tend;            // [n_windows] declares of each window before the stop point
  // ---- bounded cache or pair: the chunk's first op in the batch-order op list
  // (raw[] / ev[]): an exclusive scan of n_decl in chunk order.  One window:
  // decl_base itself; several: their own scan (dec_windows_op_base), since a
  // window-relative base is not unique across windows.
  const uint64_t* op_base;
};

// One decoder's window for the kernels that take several: hash[256], seg[256 *
// SEG], the declares made before this batch; (device) the window-major index
// of its first declare of this batch and how many the batch holds.
struct WinView {
  uint64_t* hash;
  uint8_t* seg;
  uint64_t count;
  uint64_t first;
  uint64_t total;
  uint64_t reserved;
};

// Insert h into an open-addressed set; true if it was not there.  A full set
// reports every hash as new (the caller then overflows its cap).
__device__ __forceinline__ bool uset_insert(uint64_t* keys, uint32_t mask, uint64_t h) {
  uint32_t i = tab_slot((uint32_t)h, (uint32_t)(h >> 32), mask);
  for (uint32_t n = 0; n <= mask; ++n) {
    const uint64_t prev = atomicCAS((unsigned long long*)&keys[i], (unsigned long long)EMPTY_KEY,
                                    (unsigned long long)h);
    if (prev == EMPTY_KEY) return true;
    if (prev == h) return false;
    i = (i + 1) & mask;
  }
  return true;
}

// Is persistent slot gv live for a lookup at stream position `here`?
__device__ __forceinline__ bool g_live(const DecParams& prm, uint64_t gv, uint64_t here) {
  if (gv == ~0ull) return false;
  if (!prm.ptime) return true;
  return ((here >> 32 << 21) | (uint32_t)here) < prm.ptime[gv];
}

__device__ __forceinline__ uint64_t spos(uint32_t chunk, uint32_t off) { return ((uint64_t)chunk << 32) | off; }

__device__ __noinline__ bool dec_equal2048(const uint8_t* a, const uint8_t* b) {
  const int l = lane_id();
  const u32x4 a0 = *(const u32x4_u*)(a + 32 * l), a1 = *(const u32x4_u*)(a + 32 * l + 16);
  const u32x4 b0 = *(const u32x4_u*)(b + 32 * l), b1 = *(const u32x4_u*)(b + 32 * l + 16);
  const bool ok = a0[0] == b0[0] && a0[1] == b0[1] && a0[2] == b0[2] && a0[3] == b0[3] && a1[0] == b1[0] &&
                  a1[1] == b1[1] && a1[2] == b1[2] && a1[3] == b1[3];
  return ballot(!ok) == 0;
}

// Batch table insert with earliest (vals, atomicMin) and latest (atomicMax);
// the EXTRACT that claims the slot records its position as the slot's owner.
__device__ __forceinline__ bool xtab_insert(HashTab t, uint64_t* latest, uint64_t* owner, uint32_t lo, uint32_t hi,
                                            uint64_t pos, bool& existed, uint32_t& slot) {
  const uint64_t key = ((uint64_t)hi << 32) | lo;
  uint32_t i = tab_slot(lo, hi, t.mask);
  for (uint32_t n = 0; n <= t.mask; ++n) {
    const uint64_t prev = atomicCAS((unsigned long long*)&t.keys[i], (unsigned long long)EMPTY_KEY,
                                    (unsigned long long)key);
    if (prev == EMPTY_KEY || prev == key) {
      existed = prev == key;
      slot = i;
      if (!existed) owner[i] = pos;
      atomicMin((unsigned long long*)&t.vals[i], (unsigned long long)pos);
      atomicMax((unsigned long long*)&latest[i], (unsigned long long)pos);
      return true;
    }
    i = (i + 1) & t.mask;
  }
  return false;
}

// ------------------------------------------------------------------ window

__device__ __forceinline__ uint64_t d_lo_of(const DecParams& prm) {
  if (!prm.D_tail) return prm.D_lo;
  const uint64_t te = readfirst64(*prm.t_end);
  return te > 256u ? te - 256u : 0u;
}

// XCodecWindow::dereference(c) (xcodec/xcodec_window.h:102-111) after T
// declares of this batch: false if the slot is empty, else the slot's hash
// and bytes.  Wave-uniform.  `gd` receives the global declare index.
__device__ bool window_slot(const DecParams& prm, uint64_t T, uint32_t c, uint64_t& h, const uint8_t*& src,
                            uint64_t& gd) {
  const uint64_t W = prm.win_count, G = W + T, DL = d_lo_of(prm);
  if (G == 0) return false;
  const uint64_t r = (G - 1u - c) & 255u;
  if (r > G - 1u) return false;                              // slot never written
  const uint64_t g = G - 1u - r;                              // latest declare with g = c (mod 256)
  gd = g;
  if (g < W) {                                               // made before this batch: the window holds it
    h = readfirst64(prm.win_hash[c]);
    if (h == 0) return false;                                // emptied by a re-declare (:79-83)
    src = prm.win_seg + (uint64_t)c * SEG;
  } else {
    const uint4 rec = prm.D[g - W - DL];
    h = ((uint64_t)readfirst(rec.y) << 32) | readfirst(rec.x);
    src = (const uint8_t*)(((uint64_t)readfirst(rec.w) << 32) | readfirst(rec.z));
  }
  // declared again after g (batch declares only; the window state covers the rest)?
  const uint64_t a = (g + 1u > W ? g + 1u - W : 0u), b = T;
  bool dup = false;
  for (uint64_t t = a + lane_id(); t < b; t += 64) {
    const uint4 e = prm.D[t - DL];
    dup |= e.x == (uint32_t)h && e.y == (uint32_t)(h >> 32);
  }
  return ballot(dup) == 0;
}

// Window w of a batch over several (xcg_decode_batch_windows; wave-uniform w):
// its state before the batch and its own range of the declare records.
struct ManyWindow {
  uint64_t* hash;
  uint8_t* seg;
  uint64_t count;
  const uint4* D;
  uint64_t off;                // the window's declare t of this batch at D[t + off] (mod 2^64)
  __device__ __forceinline__ ManyWindow(const DecParams& p, uint32_t w) {
    const WinView* v = p.wins + w;
    hash = (uint64_t*)readfirst64((uint64_t)v->hash);
    seg = (uint8_t*)readfirst64((uint64_t)v->seg);
    count = readfirst64(v->count);
    D = p.D;
    if (p.D_tail) {
      const uint64_t te = readfirst64(p.w_tend[w]);
      off = 256ull * w - (te > 256u ? te - 256u : 0u);
    } else {
      off = readfirst64(v->first);
    }
  }
};

// window_slot for one of several windows: T and `gd` count the window's own
// declares, and the records searched are the window's own.  (The slot
// arithmetic is window_slot's, restated rather than shared: the one-window
// kernels keep the code they were compiled to before this path existed.)
__device__ bool window_slot_of(const ManyWindow& win, uint64_t T, uint32_t c, uint64_t& h, const uint8_t*& src,
                               uint64_t& gd) {
  const uint64_t W = win.count, G = W + T;
  if (G == 0) return false;
  const uint64_t r = (G - 1u - c) & 255u;
  if (r > G - 1u) return false;
  const uint64_t g = G - 1u - r;
  gd = g;
  if (g < W) {
    h = readfirst64(win.hash[c]);
    if (h == 0) return false;
    src = win.seg + (uint64_t)c * SEG;
  } else {
    const uint4 rec = win.D[g - W + win.off];
    h = ((uint64_t)readfirst(rec.y) << 32) | readfirst(rec.x);
    src = (const uint8_t*)(((uint64_t)readfirst(rec.w) << 32) | readfirst(rec.z));
  }
  const uint64_t a = (g + 1u > W ? g + 1u - W : 0u), b = T;
  bool dup = false;
  for (uint64_t t = a + lane_id(); t < b; t += 64) {
    const uint4 e = win.D[t + win.off];
    dup |= e.x == (uint32_t)h && e.y == (uint32_t)(h >> 32);
  }
  return ballot(dup) == 0;
}

// REF source: the earliest EXTRACT of h in the batch before `here`, else the
// persistent cache (the cache state at that point of the stream).
__device__ __forceinline__ const uint8_t* ref_source(const DecParams& prm, uint32_t lo, uint32_t hi, uint64_t here) {
  const uint64_t e = tab_lookup(prm.x, lo, hi);
  if (e != ~0ull && e < here) return prm.in + prm.chunk_off[e >> 32] + (uint32_t)e;
  const uint64_t gv = tab_lookup(prm.g, lo, hi);
  if (g_live(prm, gv, here)) return prm.pool + gv * (uint64_t)SEG;
  return nullptr;
}

// Name reuse: the latest EXTRACT of a flagged hash at a position before `here`
// (~0: none), by binary search in the occurrences sorted by (hash, position).
__device__ __forceinline__ uint64_t occ_before(const DecParams& prm, uint64_t key, uint64_t here) {
  uint32_t a = 0, b = prm.nocc;                              // first entry >= (key, here)
  while (a < b) {
    const uint32_t mid = a + ((b - a) >> 1);
    const uint64_t k = prm.occ_key[mid], p = prm.occ_pos[mid];
    if (k < key || (k == key && p < here)) a = mid + 1;
    else b = mid;
  }
  if (a == 0 || prm.occ_key[a - 1] != key) return ~0ull;
  return prm.occ_pos[a - 1];
}

// Per-thread slot of a hash in the batch table (~0: absent).
__device__ __forceinline__ uint32_t xtab_find_t(const HashTab& t, uint32_t lo, uint32_t hi) {
  const uint64_t key = ((uint64_t)hi << 32) | lo;
  uint32_t i = tab_slot(lo, hi, t.mask);
  for (uint32_t n = 0; n <= t.mask; ++n) {
    const uint64_t k = t.keys[i];
    if (k == key) return i;
    if (k == EMPTY_KEY) break;
    i = (i + 1) & t.mask;
  }
  return ~0u;
}

// Per-lane REF source (the same rule as ref_source, each lane its own hash).
// REUSE: a hash whose EXTRACTs differ in bytes resolves to the latest EXTRACT
// before the REF instead of the earliest (xcodec_decoder.cc:120-136 replaced
// the entry in between).
template <bool REUSE>
__device__ __forceinline__ const uint8_t* ref_source_t(const DecParams& prm, uint32_t lo, uint32_t hi, uint64_t here) {
  uint64_t e;
  if (REUSE) {
    const uint32_t s = xtab_find_t(prm.x, lo, hi);
    e = s == ~0u ? ~0ull : prm.x.vals[s];
    if (s != ~0u && prm.x_flag[s]) e = occ_before(prm, ((uint64_t)hi << 32) | lo, here);
  } else {
    e = tab_lookup_t(prm.x, lo, hi);
  }
  if (e != ~0ull && e < here) return prm.in + prm.chunk_off[e >> 32] + (uint32_t)e;
  const uint64_t gv = tab_lookup_t(prm.g, lo, hi);
  if (g_live(prm, gv, here)) return prm.pool + gv * (uint64_t)SEG;
  return nullptr;
}

// A run of consecutive REF ops from offset i (the op at i is a whole REF
// before `limit`): lane l takes the l-th REF, at i + 10 l, while every op
// before it is a REF too (a REF is 10 bytes, so that is where the next op
// starts).  REF-dense streams (warm caches: one REF per 2 KiB) then pay one
// round of lane-parallel table lookups per 64 REFs instead of one dependent
// chain per REF.  Returns the run length (1..64, uniform); lanes < run get
// their hash and stream position.
template <typename P>
__device__ __forceinline__ uint32_t ref_run(P x, uint32_t i, uint32_t len, uint32_t chunk,
                                            uint64_t limit, uint64_t& h, uint64_t& here) {
  const uint32_t l = (uint32_t)lane_id();
  const uint32_t o = i + 10u * l;
  here = spos(chunk, o);
  bool isref = o + 10u <= len && here < limit;
  if (isref) isref = x[o] == MAGIC && x[o + 1] == OP_REF;
  const uint64_t bad = ballot(!isref);
  const uint32_t r = bad ? (uint32_t)__builtin_ctzll(bad) : 64u;
  h = 0;
  if (l < r) h = be64(x + o + 2);
  return r;
}

// Copy k segments (pointers held by lanes 0..k-1) to dst, consecutively; the
// loads of four segments are in flight together.
__device__ __forceinline__ void copy_segments(uint8_t* dst, const uint8_t* src_lane, uint32_t k) {
  const int l = lane_id();
  for (uint32_t a = 0; a < k; a += 4) {
    u32x4 v[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (a + j < k) {
        const uint64_t sp = readlane64((uint64_t)src_lane, (int)(a + j));
        const uint8_t* sj = (const uint8_t*)sp;
        v[2 * j] = *(const u32x4_u*)(sj + 32 * l);
        v[2 * j + 1] = *(const u32x4_u*)(sj + 32 * l + 16);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (a + j < k) {
        uint8_t* d = dst + (uint64_t)(a + j) * SEG;
        *(u32x4_u*)(d + 32 * l) = v[2 * j];
        *(u32x4_u*)(d + 32 * l + 16) = v[2 * j + 1];
      }
    }
  }
}

// The header-only op walk of a chunk (literal runs skipped, nothing emitted):
// every whole EXTRACT, run of REFs and BACKREF in order, up to the first op
// that is cut short or unknown.  on_extract(i), on_ref_run(i, r, h, here) --
// ref_run's run length and per-lane hash and stream position -- and
// on_backref(i) take the op's offset and return true to stop the walk.
template <class FE, class FR, class FB>
__device__ __forceinline__ void walk_op_headers(const uint8_t* x, uint32_t len, uint32_t chunk, FE on_extract,
                                                FR on_ref_run, FB on_backref) {
  uint32_t i = 0;
  while (i < len) {
    uint32_t nesc = 0;
    i = next_op(x, i, len, nesc);
    if (i + 1 >= len) break;
    const uint32_t op = x[i + 1];
    if (op == OP_EXTRACT) {
      if (len - i < 2u + SEG) break;
      if (on_extract(i)) break;
      i += 2 + SEG;
    } else if (op == OP_REF) {
      if (len - i < 10u) break;
      uint64_t h, here;
      const uint32_t r = ref_run(x, i, len, chunk, ~0ull, h, here);
      if (on_ref_run(i, r, h, here)) break;
      i += 10u * r;
    } else if (op == OP_BACKREF) {
      if (len - i < 3u) break;
      if (on_backref(i)) break;
      i += 3;
    } else {
      break;
    }
  }
}

// Declare records of one chunk whose first declare is number `base`: those
// numbered [lo_t, hi_t) go to prm.D[t + off] (mod 2^64).  One wave.
template <bool REUSE>
__device__ __forceinline__ void decl_record_chunk(const DecParams& prm, uint32_t chunk, uint64_t base, uint64_t lo_t,
                                                  uint64_t hi_t, uint64_t off) {
  const uint8_t* x = prm.in + prm.chunk_off[chunk];
  const uint32_t len = prm.chunk_len[chunk];
  uint64_t t = base;                                         // (the walk stops once the records reach hi_t)
  walk_op_headers(
      x, len, chunk,
      [&](uint32_t i) {
        if (t >= lo_t) {
          const uint2 h = dec_window_hash(x + i + 2);
          const uint64_t src = (uint64_t)(x + i + 2);
          if (lane_id() == 0) prm.D[t + off] = make_uint4(readfirst(h.x), readfirst(h.y), (uint32_t)src, (uint32_t)(src >> 32));
        }
        return ++t >= hi_t;
      },
      [&](uint32_t, uint32_t r, uint64_t h, uint64_t here) {
        const uint64_t tl = t + (uint64_t)lane_id();
        if ((uint32_t)lane_id() < r && tl >= lo_t && tl < hi_t) {
          const uint64_t src = (uint64_t)ref_source_t<REUSE>(prm, (uint32_t)h, (uint32_t)(h >> 32), here);
          prm.D[tl + off] = make_uint4((uint32_t)h, (uint32_t)(h >> 32), (uint32_t)src, (uint32_t)(src >> 32));
        }
        t += r;
        return t >= hi_t;
      },
      [](uint32_t) { return false; });
}

// ---- host entry points between the units (plain host functions, the way the
// encoder's units reach each other; nobody launches another unit's kernel)

// xcg_decode_bounded.hip: a bounded or pair context's batch (a context is one
// or the other, never both), classified against the cache as it evolves.
struct DecClassified {
  uint4* raw = nullptr;        // every EXTRACT / REF op of the batch (dec_ops_kernel)
  uint4* evs = nullptr;        // what each does to the cache (dec_classify_kernel)
  uint4* rows = nullptr;       // declaration rows: the bytes of the ENTERs (pair: and of the REPLACEs)
  uint32_t* nev = nullptr;     // per chunk: classified ops, declaration rows
  uint32_t* nrows = nullptr;
  LruBatch lb{};               // (bounded) the batch as xcg_lru_times / xcg_lru_commit take it
};
// Lists the ops (ndecl of them: the scan's declare count) and classifies them
// until the eviction / departure times the classification used are the ones
// it leaves (at most 64 passes: XCG_RC_OVERFLOW).  `tmp` owns the temporary K
// points into; p.ptime is set for the passes that follow.  *p.berr_pos is the
// cap: with BACKREFs in the batch decode_brefcheck_kernel has run before this,
// and the passes move only the unknown-REF stop in front of it.
int dec_classify(const XcgDecodeArgs* a, DecParams& p, uint64_t ndecl, StreamTemp& tmp, DecClassified* K,
                 hipStream_t stream);
// Before anything is emitted: dec_precheck_kernel (status bit 9).
void dec_launch_precheck(const DecParams& p, hipStream_t stream);
// After the window update: the cache takes the batch (bounded: replaced bytes,
// then xcg_lru_commit; pair: xcg_pair_decode_commit).
int dec_classified_commit(const XcgDecodeArgs* a, const DecParams& p, const DecClassified& K, hipStream_t stream);


// xcg_decode_windows.hip: the window passes of a batch over several windows
// (p.wins set).  Numbering: p.n_decl scanned in the plan's window-major order
// into p.decl_base (each chunk's base within its own window), every window's
// first and total, the batch's total into *d_total.
void dec_windows_number(const XcgDecodeWindows* w, const DecParams& p, uint64_t* d_total, hipStream_t stream);
// Behind the numbering (bounded and pair contexts): p.n_decl scanned in chunk
// order, the op list's base of every chunk (DecParams::op_base), into the
// numbering's scan scratch, which it no longer needs.  *d_total gets the same
// total again.
const uint64_t* dec_windows_op_base(const XcgDecodeWindows* w, const DecParams& p, uint64_t* d_total,
                                    hipStream_t stream);
// Records of every declare, window-major (the batch holds BACKREFs).
void dec_windows_records(const DecParams& p, bool reuse, hipStream_t stream);
// After the emit pass: every window's t_end, (tail: p.D = the 256 records per
// window, made here) and the update of every window the batch declared into.
void dec_windows_finish(const XcgDecodeWindows* w, DecParams& p, bool full, bool reuse, hipStream_t stream);

}  // namespace xcg
