// The library's internal interface: every struct and every extern "C" function
// that crosses translation units inside libxcgpu (the host ABI layer
// xcg_ctx.hip and xcg_api_*.hip, xcg_pipe.cpp and the kernel drivers
// xcg_encode_* / xcg_decode* / xcg_cache_* / xcg_lru / xcg_pair / xcg_hash).  The file that defines one of these functions
// and every file that calls it include this header, so a prototype that drifts
// is a compile error.  Plain data only: xcg_pipe.cpp compiles it as host C++.
//
// The argument structs are filled from `T a{};` (everything zero / null) by
// named member assignment, never by a positional initialiser list.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xcg_decode_words.h"   // the decode scratch words by name
#include "xcg_devmem.h"
#include "xcg_rc.h"      // the drivers' return codes (XCG_RC_*)

struct xcg_ctx;

// Device view of a context's persistent segment cache (layout: xcg_cache.h):
// the exact table, the segment pool and the lane-probe filters over the table.
struct XcgCacheView {
  uint64_t* keys = nullptr;
  uint64_t* vals = nullptr;
  uint32_t mask = 0;
  uint8_t* pool = nullptr;
  uint32_t seg_cap = 0;
  uint32_t* nseg = nullptr;     // device counter
  uint32_t* filt = nullptr;     // FILT_WORDS
  uint32_t* ftab = nullptr;     // fbuckets * 4
  uint32_t fmask = 0;
  uint32_t* gfilt = nullptr;    // global lane filter: gmask + 1 words (~1 per segment)
  uint32_t gmask = 0;
};

// A context's batch scratch (allocated by ensure_scratch, xcg_ctx.hip): every
// array a stream batch works in, declared here once.  The stream driver's
// arguments below begin with a copy of it.
struct XcgBatchScratch {
  uint32_t n_cap = 0, maxd_cap = 0;   // chunks / declaration rows per chunk the scratch was grown for
  uint64_t* b_keys = nullptr;
  uint64_t* b_vals = nullptr;
  uint32_t b_mask = 0;
  uint32_t* r_filt = nullptr;
  uint32_t* r_ftab = nullptr;
  void* decl = nullptr;             // uint4 rows
  uint32_t* ndecl = nullptr;
  uint32_t* changed = nullptr;
  uint32_t* h_changed = nullptr;    // pinned host word
  uint32_t* r_gfilt = nullptr;      // the round's copy of the cache's global lane filter
  uint32_t* bcount = nullptr;       // [64]
  // verification: a second batch table (tables alternate between rounds, same
  // mask), the changed-hash table (hash -> chunk range), per-chunk batch hits, flags
  uint64_t* b2_keys = nullptr;
  uint64_t* b2_vals = nullptr;
  uint64_t* r_keys = nullptr;
  uint64_t* r_vals = nullptr;
  uint32_t r_mask = 0;
  uint64_t* hits = nullptr;         // n_cap * maxh batch hits
  uint32_t* nhits = nullptr;
  uint32_t maxh = 0;
  uint32_t* need = nullptr;
  uint32_t* vflags = nullptr;       // [0] a_first, [1] any, [2] declarations in the last table built
  uint32_t* h_vflags = nullptr;     // pinned
  // verification (a), exactly (verify_probe_kernel): the hashes that became
  // visible to more chunks -> that chunk range, and their Bloom words
  uint64_t* a_keys = nullptr;       // [XCG_VERIFY_A_CAP]
  uint64_t* a_vals = nullptr;
  uint32_t* a_bits = nullptr;       // [XCG_VERIFY_A_WORDS]
  // the quiet-chunk screen (small chunks): the 128 KiB LDS fold of the round's
  // global lane filter, and the work list of chunks it sends to the parse
  // ([0] count, [1..n] chunks); null: no screen
  uint32_t* s_fold = nullptr;
  uint32_t* s_work = nullptr;
  uint32_t* s_info = nullptr;       // [n] the screen's verdict per chunk
  void* s_rows = nullptr;           // [n * 4] uint4: its staged rows
  uint32_t* s_qcnt = nullptr;       // [n] and [n * 1024]: the windows it queues for the probe
  uint32_t* s_qkeys = nullptr;
  uint32_t last_maxd = 0;           // declaration stride of the last stream batch
  // bounded (LRU) cache and pair only (null / 0 on other contexts): every
  // chunk's cache references (xcg_lru.hip)
  void* ev = nullptr;               // n_cap * maxe uint4
  uint32_t* nev = nullptr;
  uint32_t maxe = 0;
  uint32_t* ev_base = nullptr;      // [n + 1], [n + 1]: the LRU pass's row and enter bases
  uint32_t* enter_base = nullptr;
  uint32_t* ev_slot = nullptr;      // [n * maxe]: each reference's pool slot / LRU time
  uint64_t* ev_time = nullptr;
  // re-parse restart (xcg_encode_wave.h RestartArgs): output length after each
  // REF-making lookup, per chunk the earliest / latest contradicted lookup
  // time, and the backup of the previous pass's rows of the flagged chunks
  uint32_t* eo = nullptr;           // [n * maxe]
  uint32_t* bad_t = nullptr;        // [n] (~0: none)
  uint32_t* bad_hi = nullptr;       // [n]
  uint32_t* bslot = nullptr;        // [n]
  uint32_t* b_count = nullptr;      // [1]
  uint32_t b_slots = 0;
  void* b_ev = nullptr;             // [b_slots * maxe] uint4
  uint32_t* b_eo = nullptr;         // [b_slots * maxe]
  uint64_t* b_hits = nullptr;       // [b_slots * maxh]
  uint32_t* b_cnt = nullptr;        // [b_slots * 4]
  uint8_t* b_out = nullptr;         // [b_slots * b_stride]
  uint64_t b_stride = 0;
  void* splice = nullptr;           // [n] uint4
};

// Arguments of the stream-semantics encode driver (xcg_launch_encode_stream),
// and of the bounded-cache and pair passes around it: the context's batch
// scratch and the call.
struct XcgStreamArgs : XcgBatchScratch {
  const uint8_t* in;
  const uint64_t* chunk_off;
  const uint32_t* chunk_len;
  uint32_t n;
  uint32_t flags;
  uint8_t* out;
  const uint64_t* out_off;
  uint64_t* out_len;
  uint32_t* stats;
  int32_t* status;
  XcgCacheView g;        // persistent cache
  uint32_t maxd;         // the call's declaration stride (<= maxd_cap)
  int seed;              // start from the tiling seed instead of round 0
  uint32_t* decls_out;   // (host) declarations the batch made, ~0 if unknown
  // bounded (LRU) cache: eviction times per pool slot, and whether the driver
  // commits (the LRU pass commits itself)
  const uint64_t* ptime;
  int no_commit;
  int keep_decls;        // start from the declaration lists already in decl/ndecl
  int need_given;        // (keep_decls) round 1 parses only the chunks flagged in need[]
  int restart;           // (need_given) round 1 resumes flagged chunks from their rows
  // the context's event behind the verification flags' copy (hipEvent_t; null:
  // the driver makes one for the call)
  void* flags_ev;
  // (bounded cache) called behind each Jacobi verification, before the host
  // reads its flags: queues work gated on vflags[1] == 0 (the round converged)
  int (*post_verify)(void* user, const uint32_t* vbusy, hipStream_t st);
  void* post_user;
};

// (a)-probe sizes: at most A_LIMIT newly visible hashes per verification (more:
// the conservative flag), a table of twice that, a 32 KiB blocked Bloom filter.
constexpr uint32_t XCG_VERIFY_A_LIMIT = 8192, XCG_VERIFY_A_CAP = 16384, XCG_VERIFY_A_WORDS = 8192;

// Bounded cache (xcg_lru.hip): device LRU state of a context.  Persistent
// arrays only: what belongs to one batch travels in its LruBatch.
struct XcgLruState {
  xcg::DevMem* mem;       // the context's owner of these arrays (host)
  uint32_t C;             // memory_cache_limit_ in segments (= pool slots)
  uint64_t* skey;         // [C] key of the entry in pool slot s
  uint64_t* lastref;      // [C] LRU time of its last enter / lookup
  uint32_t* queue;        // [C] live slots, least recently used first
  uint32_t* queue2;
  uint64_t* ptime;        // [C] batch time from which slot s is evicted (~0: never)
  uint64_t* hmin;
  uint64_t* wpop;
  uint64_t* tau;
  uint32_t* alive;
  uint32_t* freel;
  uint32_t* tot;          // [16]
  uint32_t* h_tot;        // pinned [16]
  uint64_t clock;         // LRU time base of the next batch (host)
  uint32_t* part;         // per-tile counts of the multi-workgroup scans (grown on demand)
  uint32_t part_cap;
  uint32_t last_base;     // first chunk of the last committed sub-batch (its rows stay in the scratch)
  uint32_t fit_hint;      // chunks x maxd a full-cache sub-batch held last (0: none yet)
  void* tev;              // hipEvent_t behind the eviction times' totals (lazily made)
};

// A batch's cache references for the LRU pass: enters as declaration rows
// decl[c * maxd + d] = (lo, hi, position, -), d < ndecl[c]; references as
// ev[row(c) + k], k < nev[c] (row = c * maxe, or packed when dense).
struct LruBatch {
  uint32_t n;
  const uint8_t* in;
  const uint64_t* chunk_off;
  const void* decl;
  const uint32_t* ndecl;
  uint32_t maxd;
  const void* ev;
  const uint32_t* nev;
  uint32_t maxe;
  int dense;
  uint32_t* need;         // (encoder) chunks with an inconsistent lookup; may be scratch
  XcgCacheView g;
  int32_t* status;
  uint64_t ev_bound;      // upper bound of the batch's references (sizes the scans)
  uint32_t* bad_t;        // (encoder, optional) per chunk earliest / latest contradicted lookup time
  uint32_t* bad_hi;
  // the pass's scratch, the caller's for the batch: per reference its pool slot
  // and LRU time; per chunk its first row and first enter
  uint32_t* evslot;
  uint64_t* evtime;
  uint32_t* ev_base;      // [n + 1]
  uint32_t* enter_base;   // [n + 1]
};

// XCodecCachePair of a bounded memory primary and a disk secondary (the state
// objects' life cycle: xcg_pair_state.hip; the replay engine: xcg_pair.hip).
// The disk (XcgDiskState) is shared by every pair front on it, as XCodecDisk is
// by its XCodecDiskCache front-ends.
struct XcgDiskState;
struct XcgPairState;
// What a pair commit / table rebuild touches on the GPU: the batch input and
// its declaration rows (bytes of new entries), the pool, G and its filters.
struct PairGpu {
  const uint8_t* in;
  const uint64_t* chunk_off;
  const void* decl;       // uint4 rows: decl[c * maxd + d].z = the segment's offset in chunk c
  uint32_t maxd;
  XcgCacheView g;
  int32_t* status;
};
extern "C" int xcg_disk_state_create(uint64_t disk_bytes, uint32_t flags, XcgDiskState** out);
extern "C" int xcg_disk_state_tier(const XcgDiskState* K);
extern "C" void xcg_disk_state_release(XcgDiskState* K);
extern "C" void xcg_disk_state_stats(const XcgDiskState* K, uint64_t* st);
extern "C" int xcg_pair_state_create(uint32_t C, XcgDiskState* K, const char* uuid36, int want_xuid,
                                     XcgPairState** out);
extern "C" int xcg_disk_state_save(XcgDiskState* K, const char* path);
extern "C" int xcg_disk_state_open(const char* path, uint64_t disk_bytes, uint32_t flags, XcgDiskState** out);
extern "C" int xcg_disk_state_open_fd(int fd, uint64_t disk_bytes, uint32_t flags, XcgDiskState** out);
extern "C" void xcg_disk_state_head(const XcgDiskState* K, uint64_t* index_block, uint64_t* next);
extern "C" uint32_t xcg_pair_state_xuid(const XcgPairState* P);
extern "C" void xcg_pair_state_set_unbounded(XcgPairState* P);
extern "C" int xcg_pair_state_unbounded(const XcgPairState* P);
extern "C" void xcg_pair_state_destroy(XcgPairState* P);
extern "C" int xcg_pair_state_clear(XcgPairState* P);
extern "C" void xcg_pair_state_stats(const XcgPairState* P, uint64_t* st);
extern "C" uint32_t xcg_pair_state_last_base(const XcgPairState* P);
extern "C" uint32_t xcg_pair_state_disk_blocks(const XcgPairState* P);
extern "C" XcgDiskState* xcg_pair_state_disk(const XcgPairState* P);
extern "C" const uint64_t* xcg_pair_state_ptime(const XcgPairState* P);
extern "C" int xcg_pair_sync(XcgPairState* P, const PairGpu* G, hipStream_t st);
extern "C" int xcg_pair_encode_stream(const XcgStreamArgs* a, XcgPairState* P, int* rounds_out, hipStream_t st);
extern "C" int xcg_pair_decode_begin(XcgPairState* P, hipStream_t st);
extern "C" int xcg_pair_decode_pass(XcgPairState* P, const PairGpu* G, const void* d_rows, const uint64_t* d_base,
                                    const uint64_t* d_cnt, uint32_t n, uint64_t rows, uint32_t maxd, int* same,
                                    hipStream_t st);
extern "C" uint8_t* xcg_pair_state_pool(const XcgPairState* P);
extern "C" int xcg_pair_decode_commit(XcgPairState* P, const PairGpu* G, hipStream_t st);


// A context's decode scratch (allocated by ensure_dscratch / ensure_dchunks,
// xcg_ctx.hip), declared here once; the batch decode driver's arguments begin
// with a copy of it.
struct XcgDecodeScratch {
  uint32_t x_cap = 0;
  uint64_t* x_keys = nullptr;
  uint64_t* x_vals = nullptr;
  uint64_t* x_latest = nullptr;
  // name reuse: parallel to x_vals the EXTRACT that claimed each slot and the differing-bytes flags; the
  // duplicate EXTRACT list (the later EXTRACTs of a hash; x_cap / 2 >= every EXTRACT of a batch)
  uint64_t* x_owner = nullptr;
  uint32_t* x_flag = nullptr;
  uint32_t* dup_slot = nullptr;
  uint64_t* dup_pos = nullptr;
  uint64_t* u_keys = nullptr;      // unknown-hash set, 2 * unknown_cap slots
  uint64_t* unknown = nullptr;
  uint64_t* unknown_pos = nullptr;
  // the batch's counters and single words, and where they come back on the host (pinned): xcg_decode_words.h
  xcg::DecCounts* counts = nullptr;
  xcg::DecScratch* scratch = nullptr;
  xcg::DecHostWords* h_scratch = nullptr;
  uint32_t chunk_cap = 0;
  uint64_t* chunk_tmp = nullptr;   // 4 * n u64: n_decl, n_bref, decl_base, n_decl_emit
  uint4* d_tail = nullptr;         // 256 declare records (window update)
};

// A batch over several BACKREF windows (xcg_decode_batch_windows): the plan of
// xcg_decode_windows_plan.h and the windows' scratch, all device memory.
struct XcgDecodeWindows {
  uint32_t n_windows;
  void* views;               // xcg::WinView[n_windows]: hash, seg and count filled by the host
  const uint32_t* chunk_win; // [n] chunk -> window
  const uint32_t* order;     // [n] the chunks window-major
  const uint32_t* first;     // [n_windows + 1] each window's first position in `order`
  uint64_t* scan_tmp;        // [2 n] the declare counts in that order, and their scan
  uint64_t* w_tend;          // [n_windows] out: each window's declares before the stop point
  uint4* tail;               // [256 * n_windows] tail records
};

// Arguments of the batch decode driver (xcg_launch_decode): the context's
// decode scratch and the call.
struct XcgDecodeArgs : XcgDecodeScratch {
  const uint8_t* in;
  const uint64_t* chunk_off;
  const uint32_t* chunk_len;
  uint32_t n;
  uint8_t* out;
  uint64_t out_cap;
  uint64_t* out_off;
  uint64_t* out_len;
  int32_t* chunk_status;
  uint64_t* consumed;
  int32_t* status;
  XcgCacheView g;        // persistent cache
  uint32_t x_mask;       // x_cap - 1
  uint32_t unknown_cap;
  uint64_t* win_hash;    // the decoder's BACKREF window
  uint8_t* win_seg;
  uint64_t win_count;
  XcgLruState* lru;      // bounded cache (null: unbounded)
  uint32_t maxd;         // EXTRACTs a chunk can hold (bounded: declaration rows per chunk)
  XcgPairState* pair;    // XCodecCachePair (null: not a pair)
  int no_window;         // the BACKREF window is left alone (<LEARN>, single-segment host calls)
  uint32_t dup_cap;      // x_cap / 2
  const XcgDecodeWindows* wins;   // one window per decoder (null: win_hash / win_seg / win_count)
};

// Arguments of the independent decode driver (xcg_launch_decode_independent):
// per chunk its encoded bytes and the caller's output slot; nothing of a context
// but its sticky status word.
struct XcgIndepDecodeArgs {
  const uint8_t* in;
  const uint64_t* chunk_off;
  const uint32_t* chunk_len;
  uint32_t n;
  uint32_t max_len;         // the caller's bound on every chunk length (picks the per-wave table size)
  uint8_t* out;
  const uint64_t* out_off;
  const uint64_t* out_cap;
  uint64_t* out_len;
  int32_t* chunk_status;
  uint64_t* consumed;
  uint64_t* first_unknown;  // nullable
  int32_t* status;
};

// Arguments of the grouped decode driver (xcg_launch_decode_group): the same,
// with the chunks partitioned into groups of consecutive chunks, one decoder each.
struct XcgGroupDecodeArgs {
  const uint8_t* in;
  const uint64_t* chunk_off;
  const uint32_t* chunk_len;
  uint32_t n;
  const uint32_t* group_first;  // [n_groups + 1] ascending, 0 .. n
  uint32_t n_groups;
  uint32_t max_len;         // the caller's bound on every group's summed chunk lengths (picks the table size)
  uint8_t* out;
  const uint64_t* out_off;
  const uint64_t* out_cap;
  uint64_t* out_len;
  int32_t* chunk_status;
  uint64_t* consumed;
  uint64_t* first_unknown;  // nullable
  int32_t* status;
};

// Arguments of the encoder refmap driver (xcg_launch_encode_refmap): per chunk
// its encoder output and the caller's entry rows; of a context its sticky
// status word and, out of band, the declaration rows of its last stream batch.
struct XcgRefmapArgs {
  const uint8_t* enc;
  const uint64_t* enc_off;
  const uint64_t* enc_len;
  uint32_t n;
  uint32_t max_len;         // the caller's bound on every encoded length
  int collect;              // 0: no REF is an entry (null cache); the walk alone
  const void* decl;         // (out of band) uint4 rows (lo, hi, pos, -) of chunk i at decl[i * maxd ..); null: none
  const uint32_t* ndecl;    // [n]
  uint32_t maxd;
  uint64_t* ref_hash;       // [n * ref_cap]
  uint32_t* ref_pos;        // [n * ref_cap]
  uint32_t ref_cap;
  uint32_t* ref_count;      // [n]
  uint64_t* walked;         // nullable [n]
  int32_t* status;
};
extern "C" int xcg_launch_encode_refmap(const XcgRefmapArgs* a, hipStream_t stream);

extern "C" int xcg_launch_encode_stream(const XcgStreamArgs* a, int* rounds_out, hipStream_t stream);
extern "C" int xcg_lru_encode_stream(const XcgStreamArgs* a, XcgLruState* L, int* rounds_out, hipStream_t st);
extern "C" int xcg_lru_times(const LruBatch* b, XcgLruState* L, hipStream_t st);
extern "C" int xcg_lru_commit(const LruBatch* b, XcgLruState* L, hipStream_t st);
extern "C" int xcg_lru_reset_times(XcgLruState* L, hipStream_t st);
extern "C" int xcg_lru_rebuild_table(const XcgCacheView* g, XcgLruState* L, int32_t* status, hipStream_t st);
extern "C" int xcg_launch_seed_tiling(const XcgStreamArgs* a, hipStream_t stream);
extern "C" int xcg_launch_encode_independent(const uint8_t* d_in, const uint64_t* d_chunk_off,
                                             const uint32_t* d_chunk_len, uint32_t n, uint32_t max_chunk_len,
                                             uint32_t flags, uint8_t* d_out, const uint64_t* d_out_off,
                                             uint64_t* d_out_len, uint32_t* d_stats, int32_t* d_status,
                                             hipStream_t stream);
extern "C" int xcg_launch_encode_group(const uint8_t* d_in, const uint64_t* d_chunk_off, const uint32_t* d_chunk_len,
                                       uint32_t n, const uint32_t* d_group_first, uint32_t n_groups,
                                       uint32_t max_group_len, uint32_t flags, uint8_t* d_out,
                                       const uint64_t* d_out_off, uint64_t* d_out_len, uint32_t* d_stats,
                                       int32_t* d_status, hipStream_t stream);
extern "C" int xcg_launch_decode_group(const XcgGroupDecodeArgs* a, hipStream_t stream);
// Between the encoder's units, for the stream round driver (xcg_encode_stream.hip;
// EncParams: xcg_encode_wave.h).  The parse kernel's reference-recording
// instance for (big, SW) (xcg_encode_stream_lru.hip), and the quiet-chunk
// screen in front of a parse: a->s_work cleared, the fold, the screen and its
// finish, which leaves the chunks still to parse in a->s_work (xcg_encode_screen.hip).
namespace xcg {
struct EncParams;
constexpr int SCREEN_MAXD = 4;   // the screen takes chunks shorter than 4 tiles (< 8 KiB; s_rows: 4 rows a chunk)
}
extern "C" void xcg_launch_encode_stream_lru(int big, uint32_t SW, dim3 grid, dim3 block, const xcg::EncParams* prm,
                                             hipStream_t stream);
extern "C" void xcg_launch_stream_screen(const XcgStreamArgs* a, const xcg::EncParams* prm, uint32_t wgs,
                                         hipStream_t stream);

extern "C" int xcg_launch_window_hashes(const uint8_t* d_x, uint64_t len, uint64_t* d_hash, hipStream_t stream);
extern "C" int xcg_launch_segment_hashes(const uint8_t* d_x, uint64_t len, uint64_t* d_hash, hipStream_t stream);

extern "C" int xcg_launch_cache_lookup(const XcgCacheView* g, uint64_t key, uint8_t* seg_out, int32_t* found,
                                       hipStream_t s);
extern "C" int xcg_launch_cache_enter(const XcgCacheView* g, uint64_t key, const uint8_t* seg, int replace_only,
                                      int32_t* result, hipStream_t s);
// Bulk learn / export of a memory cache (xcg_cache_bulk.hip).  segs: n segments
// back to back, any alignment; hash_out (nullable): each one's XCodecHash;
// lru: the bounded cache's state, null on an unbounded one.
struct XcgBulkLearn {
  const uint8_t* segs;
  uint64_t n;             // at most 2^30
  uint64_t* hash_out;
  XcgCacheView g;
  XcgLruState* lru;
  int32_t* status;
};
extern "C" int xcg_bulk_learn(const XcgBulkLearn* a, hipStream_t st);
extern "C" int xcg_bulk_export(const XcgCacheView* g, const XcgLruState* lru, uint32_t live, uint8_t* d_segs,
                               uint64_t* d_hash, hipStream_t st);
// (xcg_decode.hip) exclusive scan of n u64 lengths into off[], their sum into *total: one workgroup
extern "C" void xcg_launch_exclusive_scan(const uint64_t* len, uint64_t* off, uint32_t n, uint64_t* total,
                                          hipStream_t stream);
extern "C" int xcg_launch_pack(const uint8_t* src, const uint64_t* src_off, const uint64_t* len, uint32_t n,
                               uint8_t* dst, uint64_t* dst_off, uint64_t* d_total, hipStream_t stream);
// (xcg_wire.hip) xcg_gather_pieces: one wave per (piece, 8 KiB tile)
extern "C" int xcg_launch_gather_pieces(const uint8_t* d_src, const uint64_t* d_src_off, const uint64_t* d_dst_off,
                                        const uint32_t* d_len, uint32_t n, uint32_t max_len, uint8_t* d_dst,
                                        hipStream_t stream);
extern "C" int xcg_launch_decode(const XcgDecodeArgs* a, uint64_t* total_out, uint64_t* block_pos_out,
                                 uint64_t* berr_pos_out, uint32_t* nunknown_out, hipStream_t stream);
extern "C" int xcg_launch_decode_independent(const XcgIndepDecodeArgs* a, hipStream_t stream);
extern "C" int xcg_launch_decode_small(const uint8_t* in, uint32_t len, const XcgCacheView* g, int32_t* status,
                                       void* scratch, uint32_t ops_cap, uint8_t* out, uint64_t out_cap,
                                       uint64_t* win_hash, uint8_t* win_seg, uint64_t win_count, uint64_t* res,
                                       uint64_t* tim, uint32_t* flag, uint32_t seq, hipStream_t stream);
// n such calls on n distinct caches in one launch (decode_calls_kernel): the
// host fills one record per call (xcg_small_dec_size() bytes each, 8-byte
// aligned) into the block it copies up, then launches over the device copy.
extern "C" uint32_t xcg_small_dec_size(void);
extern "C" void xcg_small_dec_fill(void* rec, const uint8_t* in, uint32_t len, const XcgCacheView* g, int32_t* status,
                                   void* scratch, uint32_t ops_cap, uint8_t* out, uint64_t out_cap,
                                   uint64_t* win_hash, uint8_t* win_seg, uint64_t win_count, uint64_t* res);
extern "C" int xcg_launch_decode_calls(const void* d_recs, uint32_t n, hipStream_t stream);

// (xcg_ctx.hip for xcg_pipe.cpp) a connecting pipe takes and drops its registry context
// (connect_hold: xcg_ctx_connect with the hold taken under the registry lock)
extern "C" int xcg_ctx_connect_hold(xcg_ctx* parent, const char* uuid36, xcg_ctx** out);
extern "C" void xcg_registry_release(xcg_ctx* c);
// (xcg_ctx.hip for xcg_pipe.cpp) neither a bounded cache nor a pair: xcg_decode_batch_windows takes it
extern "C" int xcg_ctx_unbounded(const xcg_ctx* c);
// (xcg_ctx.hip for xcg_codec.cpp) the device a context lives on
extern "C" int xcg_ctx_device(const xcg_ctx* c);
