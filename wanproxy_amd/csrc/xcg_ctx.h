// A context as the ABI layer's units see it (xcg_ctx.hip, xcg_api_cache.hip,
// xcg_api_encode.hip, xcg_api_decode.hip; nobody else includes this): the
// struct, and the helpers of xcg_ctx.hip that more than one unit calls.
//
// A context pins a device and the encoder configuration the reference keeps
// in XCodecEncoder / XCodecCache (stream_ = !cache_->out_of_band(),
// xcodec/xcodec_encoder.cc:40-46).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/xcgpu.h"
#include "xcg_api_host.h"
#include "xcg_args.h"
#include "xcg_devmem.h"

// The persistent segment cache of a context: XCodecMemoryCache's
// hash_map<Tag64, BufferSegment*> (xcodec/xcodec_cache.h:270) as an
// open-addressed table in HBM plus a segment pool, and the two lane-probe
// filters over it (see xcg_cache.h): the view the drivers get.  (A pair
// front's pool is its XcgPairState's: the context's owner never holds it.)
using GpuCache = XcgCacheView;
using BatchScratch = XcgBatchScratch;     // (declared with the drivers' arguments, xcg_args.h)
using DecodeScratch = XcgDecodeScratch;

// A decoder's BACKREF window (XCodecWindow, xcodec/xcodec_window.h): 256 slots
// of (hash, owned 2048-byte copy) and the number of declares made so far
// (cursor = count mod 256).  One per XCodecDecoder; a context has a default.
struct xcg_window {
  xcg::DevMem mem;
  int device = 0;
  uint64_t* hash = nullptr;
  uint8_t* seg = nullptr;
  uint64_t count = 0;
};
constexpr uint32_t UNKNOWN_CAP = 1u << 16;

// (made by `new xcg_ctx` and named assignments, xcg_ctx_create_ex)
struct xcg_ctx {
  int device = 0;
  uint32_t flags = 0;
  int32_t* d_status = nullptr;   // sticky internal-overflow word
  uint64_t cache_segments = 0;
  GpuCache g;
  BatchScratch bs;
  int last_rounds = 0;
  uint32_t last_stream_n = 0;      // chunks of the last encode batch if it was a stream batch with rows in bs, else 0
  DecodeScratch ds;
  xcg_window* own_win = nullptr;   // default window (lazily allocated)
  xcg_window* cur_win = nullptr;   // window used by decodes (own_win unless set)
  int32_t* h_status = nullptr;     // pinned copy of d_status
  // seed the next stream batch with the chunks' tilings: a fresh cache is cold (every
  // first batch declares), and later the last batch declared something
  bool seed_next = true;
  bool bounded = false;            // XCodecMemoryCache with a limit: LRU eviction (xcg_lru.hip)
  XcgLruState lru{};
  // Completion of the context's last enqueued work (recorded on the caller's
  // stream): the cache-inspection calls wait for this event only, never for
  // the whole device, so other contexts and streams keep running.
  hipEvent_t done_ev = nullptr;
  hipEvent_t flags_ev = nullptr;   // stream batches: behind the verification flags' copy (xcg_encode_stream.hip)
  XcgPairState* pair = nullptr;   // XCodecCachePair(memory, disk) (xcg_pair.hip): a front of a disk
  uint32_t pair_C = 0;             // its primary limit in segments
  bool no_window = false;          // (single-segment host calls: decodes that leave the window alone)
  // Host-call staging (xcg_encode_call / xcg_encode_host): kept across calls,
  // so a per-call encode() allocates nothing and synchronises once.
  uint8_t* stage_h = nullptr;      // pinned
  uint8_t* stage_d = nullptr;
  size_t stage_h_cap = 0, stage_d_cap = 0;
  hipStream_t call_st = nullptr;
  hipStream_t last_mark = nullptr; // stream of the last ctx_mark (ctx_order on it needs no wait)
  bool marked = false;
  bool mark_pending = false;       // done_ev not yet recorded behind the last call (ctx_flush_mark)
  // zero-copy staging of the one-launch decode() (coherent pinned host memory
  // the kernel reads and writes directly): [flag 256][input][output][results]
  uint8_t* zc_h = nullptr;
  size_t zc_cap = 0;
  uint32_t zc_seq = 0;
  // xcg_decode_batch_windows: the plan and the windows' scratch (device), and
  // the pinned block the plan goes up from and the t_end words come back to
  uint8_t* win_d = nullptr;
  uint8_t* win_h = nullptr;
  size_t win_d_cap = 0, win_h_cap = 0;
  // Who frees what (xcg_devmem.h): the cache, the LRU arrays, the batch and decode scratch (each
  // regrown as a whole), and the call blocks -- status words, staging, zero-copy block
  xcg::DevMem mem_cache, mem_lru, mem_bs, mem_ds, mem_call;
};

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// Every fresh cache of an independent or grouped call on this context holds
// `count` entries without evicting (xcg_api_host.h).
inline bool ctx_fresh_cache_fits(const xcg_ctx* c, uint32_t count) {
  return fresh_cache_fits(c->bounded || c->pair, c->pair ? c->pair_C : c->lru.C, count);
}

// xcg_ctx.hip, for every unit.  Ordering of a context's calls:
void ctx_flush_mark(xcg_ctx* c);
int ctx_wait(xcg_ctx* c);
void ctx_mark(xcg_ctx* c, hipStream_t st);
void ctx_order(xcg_ctx* c, hipStream_t st);
// and what a call allocates before it enqueues (XCG_OK or an ABI status):
int clear_cache(GpuCache& g, bool sync = true);
int ensure_cache(xcg_ctx* c);
int ensure_scratch(xcg_ctx* c, uint32_t n, uint32_t maxd);
int ensure_dscratch(xcg_ctx* c, uint64_t max_extracts);
int ensure_dchunks(xcg_ctx* c, uint32_t n);
int ensure_stage(xcg_ctx* c, size_t dbytes, size_t hbytes);
int window_alloc(int device, xcg_window** out);
void window_free(xcg_window* w);
