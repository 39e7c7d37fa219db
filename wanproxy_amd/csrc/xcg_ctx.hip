// Contexts of the C ABI declared in include/xcgpu.h: their life cycle, the
// process-wide UUID registry, the disk and pair handles, the order of a
// context's calls and everything a context allocates.
//
// All work is enqueued on the caller's stream; nothing here allocates or
// synchronises inside xcg_encode_batch, so a caller may capture it into a
// hipGraph.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <iterator>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/xcgpu.h"
#include "xcg_args.h"
#include "xcg_cache.h"
#include "xcg_ctx.h"
#include "xcg_devmem.h"

using xcg::FILT_WORDS;
using xcg::PREFIX_FILTERS;

namespace {

// XCodecCache's process-wide UUID map (xcodec/xcodec_cache.h:101-127):
// lowercase UUID -> context, and whether the registry made (owns) it.
struct RegEntry {
  xcg_ctx* ctx;
  bool owned;
};
std::mutex g_reg_mu;
std::map<std::string, RegEntry> g_reg;
// A pipe that connected a registry context at <HELLO> holds it until the pipe
// is destroyed (xcg_pipe.cpp); clearing the registry destroys a held context
// only when its last holder lets go (g_deferred), never under a live pipe.
std::map<xcg_ctx*, int> g_holds;
std::set<xcg_ctx*> g_deferred;

void registry_forget(xcg_ctx* c) {
  std::lock_guard<std::mutex> lk(g_reg_mu);
  for (auto it = g_reg.begin(); it != g_reg.end();) it = it->second.ctx == c ? g_reg.erase(it) : std::next(it);
}

}  // namespace

// The context's last call was enqueued on last_mark; done_ev is recorded
// behind it only when another stream or a host wait needs it.  Recording it
// later on the same stream marks the same point or a later one (never an
// earlier one), and back-to-back calls on one stream -- the batched encode's
// steady state -- enqueue nothing but their kernels (a marker per call cost
// the headline launch ~5-10 us of gap).
void ctx_flush_mark(xcg_ctx* c) {
  if (c->mark_pending && c->done_ev) (void)hipEventRecord(c->done_ev, c->last_mark);
  c->mark_pending = false;
}
// The context's work so far is complete (its last call's stream reached the
// event) -- the per-context replacement for a device-wide synchronise.
int ctx_wait(xcg_ctx* c) {
  ctx_flush_mark(c);
  return c->done_ev && hipEventSynchronize(c->done_ev) != hipSuccess ? XCG_EHIP : XCG_OK;
}
void ctx_mark(xcg_ctx* c, hipStream_t st) {
  c->last_mark = st;
  c->marked = true;
  c->mark_pending = true;
}
// Work enqueued on `st` starts after the context's last enqueued work (a cache
// clear on another stream, the previous call of another stream): the
// reference's calls on one cache are serialised, and so are these.
void ctx_order(xcg_ctx* c, hipStream_t st) {
  if (c->marked && c->last_mark == st && st != nullptr) return;   // (in stream order already)
  ctx_flush_mark(c);
  if (c->done_ev) (void)hipStreamWaitEvent(st, c->done_ev, 0);
}

namespace {
void free_cache(xcg_ctx* c) {
  c->mem_cache.release_all();
  c->g = GpuCache{};
}

void free_lru(xcg_ctx* c) {
  XcgLruState& L = c->lru;
  c->mem_lru.release_all();
  if (L.tev) (void)hipEventDestroy((hipEvent_t)L.tev);
  const uint32_t C = L.C;
  L = XcgLruState{};
  L.C = C;
}

int alloc_lru(xcg_ctx* c) {
  XcgLruState& L = c->lru;
  xcg::DevMem& m = c->mem_lru;
  L.mem = &m;
  const uint64_t C = L.C;
  if (!(m.dev(&L.skey, 8 * C) && m.dev(&L.lastref, 8 * C) && m.dev(&L.queue, 4 * C) && m.dev(&L.queue2, 4 * C) &&
        m.dev(&L.ptime, 8 * C) && m.dev(&L.hmin, 8 * C) && m.dev(&L.wpop, 8 * C) && m.dev(&L.tau, 8 * C) &&
        m.dev(&L.alive, 4 * C) && m.dev(&L.freel, 4 * C) && m.dev(&L.tot, 64) && m.pinned(&L.h_tot, 64)) ||
      hipMemset(L.lastref, 0, 8 * C) != hipSuccess) {
    free_lru(c);
    return XCG_ENOMEM;
  }
  L.clock = 1;
  return XCG_OK;
}

void free_scratch(xcg_ctx* c) {
  c->mem_bs.release_all();
  c->bs = BatchScratch{};
}

}  // namespace

// The context's host-call staging: pinned host and device blocks of at least
// the given sizes, and its own stream.
int ensure_stage(xcg_ctx* c, size_t dbytes, size_t hbytes) {
  if (!c->call_st && hipStreamCreateWithFlags(&c->call_st, hipStreamNonBlocking) != hipSuccess) return XCG_EHIP;
  // (a block that is replaced may still be in use by the last call's copies)
  if (dbytes > c->stage_d_cap) {
    if (c->stage_d) (void)hipStreamSynchronize(c->call_st);
    const size_t want = dbytes < (1u << 20) ? (1u << 20) : dbytes;
    if (!c->mem_call.grow(&c->stage_d, &c->stage_d_cap, dbytes, want, want, xcg::MEM_DEV)) return XCG_ENOMEM;
  }
  if (hbytes > c->stage_h_cap) {
    if (c->stage_h) (void)hipStreamSynchronize(c->call_st);
    const size_t want = hbytes < (1u << 20) ? (1u << 20) : hbytes;
    if (!c->mem_call.grow(&c->stage_h, &c->stage_h_cap, hbytes, want, want, xcg::MEM_PINNED)) return XCG_ENOMEM;
  }
  return XCG_OK;
}

namespace {
// Every array of an empty cache in one launch: the table (all ones), the
// segment count and the three probe filters (zero).
__global__ __launch_bounds__(256) void cache_wipe_kernel(uint4* kv, uint64_t kv_n, uint32_t* nseg, uint4* filt,
                                                         uint32_t filt_n, uint4* ftab, uint64_t ftab_n, uint4* gfilt,
                                                         uint64_t gfilt_n) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint4 ones = make_uint4(~0u, ~0u, ~0u, ~0u), zero = make_uint4(0u, 0u, 0u, 0u);
  for (uint64_t i = i0; i < kv_n; i += stride) kv[i] = ones;
  for (uint64_t i = i0; i < filt_n; i += stride) filt[i] = zero;
  for (uint64_t i = i0; i < ftab_n; i += stride) ftab[i] = zero;
  for (uint64_t i = i0; i < gfilt_n; i += stride) gfilt[i] = zero;
  if (i0 == 0) *nseg = 0u;
}
}  // namespace

int clear_cache(GpuCache& g, bool sync) {
  // keys and vals are separate allocations of (mask + 1) u64 each (>= 1024)
  const uint64_t half = (uint64_t)(g.mask + 1) / 2;   // uint4 per array
  hipLaunchKernelGGL(cache_wipe_kernel, dim3(1024), dim3(256), 0, nullptr, (uint4*)g.keys, half, g.nseg,
                     (uint4*)g.filt, FILT_WORDS / 4, (uint4*)g.ftab, (uint64_t)g.fmask + 1, (uint4*)g.gfilt,
                     ((uint64_t)g.gmask + 1) / 4);
  hipLaunchKernelGGL(cache_wipe_kernel, dim3(256), dim3(256), 0, nullptr, (uint4*)g.vals, half, g.nseg,
                     (uint4*)nullptr, 0u, (uint4*)nullptr, 0ull, (uint4*)nullptr, 0ull);
  if (hipGetLastError() != hipSuccess || (sync && hipStreamSynchronize(nullptr) != hipSuccess)) return XCG_EHIP;
  return XCG_OK;
}

// Lazily allocate the persistent cache (segments * 2 KiB of pool).
int ensure_cache(xcg_ctx* c) {
  if (c->g.keys) return XCG_OK;
  GpuCache& g = c->g;
  const uint64_t segs = c->cache_segments;
  g.seg_cap = (uint32_t)segs;
  const uint32_t cap = pow2_at_least(2 * segs + 1024);
  g.mask = cap - 1;
  // ~2 keys per bucket at capacity.  A bounded cache is always full and a
  // batch's declarations (up to the limit again) share the round's copy, so
  // it gets ~1 bucket per key (a bucket past 7 fingerprints sends every probe
  // into an exact check).
  const uint64_t fkeys = c->bounded ? 4 * segs : (c->pair ? segs + 2ull * c->pair_C : segs);
  const uint32_t fb = pow2_at_least(fkeys < 65536 ? 32768 : fkeys / 2);
  g.fmask = fb - 1;
  const uint32_t gw = pow2_at_least(fkeys < 131072 ? 65536 : fkeys / 2);
  g.gmask = gw - 1;
  // A pair front's pool is its primary followed by the disk's blocks, mapped
  // by the pair state (one physical disk behind every front, xcg_pair.hip).
  xcg::DevMem& m = c->mem_cache;
  if (c->pair) g.pool = xcg_pair_state_pool(c->pair);
  if (!(m.dev(&g.keys, 8ull * cap) && m.dev(&g.vals, 8ull * cap) &&
        (c->pair || m.dev(&g.pool, segs * (uint64_t)XCG_SEGMENT_LENGTH + 16)) && m.dev(&g.nseg, 16) &&
        m.dev(&g.filt, 4ull * FILT_WORDS) && m.dev(&g.ftab, 16ull * fb) && m.dev(&g.gfilt, 4ull * gw))) {
    free_cache(c);
    return XCG_ENOMEM;
  }
  int rc = clear_cache(g);
  if (rc == XCG_OK && c->bounded) rc = alloc_lru(c);
  if (rc) free_cache(c);
  return rc;
}

namespace {
// The quiet-chunk screen's key queues (small-chunk calls, maxd <= 4): 4 KiB
// per chunk of the scratch's capacity (SCREEN_QCAP keys; ~ the input's size
// for 4 KiB packets), allocated by the first such call on the context --
// whatever size of chunks grew the scratch before it -- and kept with it.
int ensure_screen_queues(xcg_ctx* c, uint32_t maxd) {
  BatchScratch& b = c->bs;
  xcg::DevMem& m = c->mem_bs;
  if (maxd > 4 || (b.s_qcnt && b.s_qkeys)) return XCG_OK;
  if (!(m.dev(&b.s_qcnt, 4ull * b.n_cap) && m.dev(&b.s_qkeys, 4096ull * b.n_cap))) {
    m.release(b.s_qcnt);
    m.release(b.s_qkeys);
    b.s_qcnt = nullptr; b.s_qkeys = nullptr;      // (the screen stays off; the parse decides alone)
  }
  return XCG_OK;
}
}  // namespace

int ensure_scratch(xcg_ctx* c, uint32_t n, uint32_t maxd) {
  BatchScratch& b = c->bs;
  xcg::DevMem& m = c->mem_bs;
  if (b.decl && n <= b.n_cap && maxd <= b.maxd_cap) return ensure_screen_queues(c, maxd);
  free_scratch(c);
  b.n_cap = n;
  b.maxd_cap = maxd;
  const uint32_t cap = pow2_at_least(2ull * n * maxd + 1024);
  b.b_mask = cap - 1;
  b.r_mask = 2 * cap - 1;          // union of two rounds' hashes
  b.maxh = maxd + 8;
  if (!(m.dev(&b.b_keys, 8ull * cap) && m.dev(&b.b_vals, 8ull * cap) &&
        m.dev(&b.r_filt, 4ull * FILT_WORDS * PREFIX_FILTERS) && m.dev(&b.r_ftab, 16ull * (c->g.fmask + 1)) &&
        m.dev(&b.decl, 16ull * n * maxd) && m.dev(&b.ndecl, 4ull * n) && m.dev(&b.changed, 16) &&
        m.pinned(&b.h_changed, 16) && m.dev(&b.r_gfilt, 4ull * (c->g.gmask + 1)) && m.dev(&b.bcount, 4 * 64) &&
        m.dev(&b.b2_keys, 8ull * cap) && m.dev(&b.b2_vals, 8ull * cap) && m.dev(&b.r_keys, 16ull * cap) &&
        m.dev(&b.r_vals, 16ull * cap) && m.dev(&b.hits, 8ull * n * (maxd + 8)) && m.dev(&b.nhits, 4ull * n) &&
        m.dev(&b.need, 4ull * n) && m.dev(&b.vflags, 16) && m.pinned(&b.h_vflags, 16) &&
        m.dev(&b.a_keys, 8ull * XCG_VERIFY_A_CAP) && m.dev(&b.a_vals, 8ull * XCG_VERIFY_A_CAP) &&
        m.dev(&b.a_bits, 4ull * XCG_VERIFY_A_WORDS) && m.dev(&b.s_fold, 4ull * 32768) &&
        m.dev(&b.s_work, 4ull * (n + 1)) && m.dev(&b.s_info, 4ull * n) && m.dev(&b.s_rows, 64ull * n))) {
    free_scratch(c);
    return XCG_ENOMEM;
  }
  ensure_screen_queues(c, maxd);
  if (c->bounded || c->pair) {
    b.maxe = 2 * maxd + 64;        // declarations + REFs + collision lookups of one chunk
    // restart backups for up to b_slots flagged chunks per pass (more re-parse from the start)
    b.b_slots = n < 256 ? n : 256;
    b.b_stride = (2ull * maxd * XCG_SEGMENT_LENGTH + 16 + 255) & ~255ull;   // >= xcg_encode_bound(max chunk)
    if (!(m.dev(&b.ev, 16ull * n * b.maxe) && m.dev(&b.nev, 4ull * n) && m.dev(&b.ev_base, 4ull * (n + 1)) &&
          m.dev(&b.enter_base, 4ull * (n + 1)) && m.dev(&b.ev_slot, 4ull * n * b.maxe) &&
          m.dev(&b.ev_time, 8ull * n * b.maxe) && m.dev(&b.eo, 4ull * n * b.maxe) && m.dev(&b.bad_t, 4ull * n) &&
          m.dev(&b.bad_hi, 4ull * n) && m.dev(&b.bslot, 4ull * n) && m.dev(&b.b_count, 16) &&
          m.dev(&b.b_ev, 16ull * b.b_slots * b.maxe) && m.dev(&b.b_eo, 4ull * b.b_slots * b.maxe) &&
          m.dev(&b.b_hits, 8ull * b.b_slots * b.maxh) && m.dev(&b.b_cnt, 16ull * b.b_slots) &&
          m.dev(&b.b_out, b.b_stride * b.b_slots) && m.dev(&b.splice, 16ull * n)) ||
        hipMemset(b.splice, 0, 16ull * n) != hipSuccess || hipMemset(b.bad_t, 0xFF, 4ull * n) != hipSuccess ||
        hipMemset(b.bad_hi, 0, 4ull * n) != hipSuccess || hipMemset(b.b_count, 0, 16) != hipSuccess) {
      free_scratch(c);
      return XCG_ENOMEM;
    }
  }
  return XCG_OK;
}

namespace {
void free_dscratch(xcg_ctx* c) {
  c->mem_ds.release_all();
  c->ds = DecodeScratch{};
}
}  // namespace

int ensure_dchunks(xcg_ctx* c, uint32_t n) {
  DecodeScratch& d = c->ds;
  if (!d.d_tail && !c->mem_ds.dev(&d.d_tail, 16ull * 256)) return XCG_ENOMEM;
  const uint32_t cap = n < 1024 ? 1024 : n;
  return c->mem_ds.grow(&d.chunk_tmp, &d.chunk_cap, cap, cap, 32ull * cap, xcg::MEM_DEV) ? XCG_OK : XCG_ENOMEM;
}

int window_alloc(int device, xcg_window** out) {
  xcg_window* w = new xcg_window;
  w->device = device;
  if (!(w->mem.dev(&w->hash, 8ull * 256) && w->mem.dev(&w->seg, 256ull * 2048)) ||
      hipMemset(w->hash, 0, 8ull * 256) != hipSuccess) {
    w->mem.release_all();
    delete w;
    return XCG_ENOMEM;
  }
  *out = w;
  return XCG_OK;
}

void window_free(xcg_window* w) {
  if (!w) return;
  w->mem.release_all();
  delete w;
}

int ensure_dscratch(xcg_ctx* c, uint64_t max_extracts) {
  DecodeScratch& d = c->ds;
  const uint32_t cap = pow2_at_least(2 * max_extracts + 1024);
  if (d.x_keys && cap <= d.x_cap) return XCG_OK;
  free_dscratch(c);
  d.x_cap = cap;
  xcg::DevMem& m = c->mem_ds;
  if (!(m.dev(&d.x_keys, 8ull * cap) && m.dev(&d.x_vals, 8ull * cap) && m.dev(&d.x_latest, 8ull * cap) &&
        m.dev(&d.unknown, 8ull * UNKNOWN_CAP) && m.dev(&d.u_keys, 16ull * UNKNOWN_CAP) &&
        m.dev(&d.x_owner, 8ull * cap) && m.dev(&d.x_flag, 4ull * cap) &&
        m.dev(&d.dup_slot, 4ull * (cap / 2)) && m.dev(&d.dup_pos, 8ull * (cap / 2)) &&
        m.dev(&d.unknown_pos, 8ull * UNKNOWN_CAP) && m.dev(&d.counts, sizeof(*d.counts)) &&
        m.dev(&d.scratch, sizeof(*d.scratch)) && m.pinned(&d.h_scratch, sizeof(*d.h_scratch)))) {
    free_dscratch(c);
    return XCG_ENOMEM;
  }
  return XCG_OK;
}

extern "C" {

const char* xcg_version(void) { return "xcgpu 0.1 gfx950"; }

const char* xcg_strerror(int status) {
  switch (status) {
    case XCG_OK: return "ok";
    case XCG_EHIP: return "HIP runtime error";
    case XCG_ENOMEM: return "out of device memory";
    case XCG_EINVAL: return "invalid argument";
    case XCG_EOVERFLOW: return "internal table overflow";
    case XCG_ENOTSUP: return "not supported";
    case XCG_ENOENT: return "no such segment";
    case XCG_EPROTO: return "pipe protocol error";
    case XCG_EEXIST: return "already registered";
    default: return "unknown status";
  }
}

uint64_t xcg_encode_bound(uint32_t len) { return 2ull * len + 16ull; }

int xcg_ctx_create(int device, uint32_t flags, xcg_ctx** out) {
  return xcg_ctx_create_ex(device, flags, XCG_DEFAULT_CACHE_SEGMENTS, out);
}

int xcg_ctx_create_bounded(int device, uint32_t flags, uint64_t memory_cache_limit_bytes, xcg_ctx** out) {
  if (!out || memory_cache_limit_bytes == 0) return XCG_EINVAL;
  // memory_cache_limit_ = bytes / XCODEC_SEGMENT_LENGTH, at least 1 (xcodec_cache.h:277-288)
  uint64_t segs = memory_cache_limit_bytes / XCG_SEGMENT_LENGTH;
  if (segs == 0) segs = 1;
  if (segs > (1ull << 29) || (flags & XCG_FLAG_NULLCACHE)) return XCG_EINVAL;
  const int rc = xcg_ctx_create_ex(device, flags, segs, out);
  if (rc != XCG_OK) return rc;
  (*out)->bounded = true;
  (*out)->lru.C = (uint32_t)segs;
  return XCG_OK;
}

int xcg_disk_create(uint64_t disk_bytes, xcg_disk** out) { return xcg_disk_create_ex(disk_bytes, 0, out); }

int xcg_disk_create_ex(uint64_t disk_bytes, uint32_t flags, xcg_disk** out) {
  if (!out || !disk_flags_valid(flags)) return XCG_EINVAL;
  *out = nullptr;
  XcgDiskState* K = nullptr;
  const int rc = xcg_disk_state_create(disk_bytes, flags, &K);
  if (rc) return status_of(rc);
  *out = (xcg_disk*)K;
  return XCG_OK;
}

void xcg_disk_destroy(xcg_disk* d) { xcg_disk_state_release((XcgDiskState*)d); }

int xcg_disk_open(const char* path, uint64_t disk_bytes, uint32_t flags, xcg_disk** out) {
  if (!out || !path || !disk_flags_valid(flags)) return XCG_EINVAL;
  *out = nullptr;
  XcgDiskState* K = nullptr;
  const int rc = xcg_disk_state_open(path, disk_bytes, flags, &K);
  if (rc) return status_of(rc);
  *out = (xcg_disk*)K;
  return XCG_OK;
}

int xcg_disk_open_fd(int fd, uint64_t disk_bytes, uint32_t flags, xcg_disk** out) {
  if (!out || fd < 0 || !disk_flags_valid(flags)) return XCG_EINVAL;
  *out = nullptr;
  XcgDiskState* K = nullptr;
  const int rc = xcg_disk_state_open_fd(fd, disk_bytes, flags, &K);
  if (rc) return status_of(rc);
  *out = (xcg_disk*)K;
  return XCG_OK;
}

int xcg_disk_head(const xcg_disk* d, uint64_t* index_block, uint64_t* next_entry) {
  if (!d || !index_block || !next_entry) return XCG_EINVAL;
  xcg_disk_state_head((const XcgDiskState*)d, index_block, next_entry);
  return XCG_OK;
}

int xcg_pair_xuid(const xcg_ctx* c) { return c && c->pair ? (int)xcg_pair_state_xuid(c->pair) : XCG_EINVAL; }

int xcg_disk_save(xcg_disk* d, const char* path) {
  if (!d || !path) return XCG_EINVAL;
  const int rc = xcg_disk_state_save((XcgDiskState*)d, path);
  return status_of(rc);
}

int xcg_disk_tier(const xcg_disk* d) { return d ? xcg_disk_state_tier((const XcgDiskState*)d) : XCG_EINVAL; }

int xcg_disk_stats(const xcg_disk* d, uint64_t* st) {
  if (!d || !st) return XCG_EINVAL;
  xcg_disk_state_stats((const XcgDiskState*)d, st);
  return XCG_OK;
}

int xcg_ctx_create_pair_on(int device, uint32_t flags, uint64_t memory_cache_limit_bytes, xcg_disk* disk,
                           xcg_ctx** out) {
  return xcg_ctx_create_pair_uuid(device, flags, memory_cache_limit_bytes, disk, nullptr, out);
}

int xcg_ctx_create_pair_uuid(int device, uint32_t flags, uint64_t memory_cache_limit_bytes, xcg_disk* disk,
                             const char* uuid36, xcg_ctx** out) {
  return xcg_ctx_create_pair_xuid(device, flags, memory_cache_limit_bytes, disk, uuid36, -1, out);
}

int xcg_ctx_create_pair_xuid(int device, uint32_t flags, uint64_t memory_cache_limit_bytes, xcg_disk* disk,
                             const char* uuid36, int xuid, xcg_ctx** out) {
  if (!out || !disk || memory_cache_limit_bytes == 0 || (flags & (XCG_FLAG_OOB | XCG_FLAG_NULLCACHE)) || xuid < -1)
    return XCG_EINVAL;
  *out = nullptr;
  uint64_t C = memory_cache_limit_bytes / XCG_SEGMENT_LENGTH;   // xcodec_cache.h:283-287
  if (C == 0) C = 1;
  if (C > (1ull << 28)) return XCG_EINVAL;
  XcgPairState* P = nullptr;
  {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return XCG_EINVAL;
    DeviceGuard g(device);
    const int prc = xcg_pair_state_create((uint32_t)C, (XcgDiskState*)disk, uuid36, xuid, &P);
    // (today's statuses, kept: whatever else stops a front's creation -- a failed copy too -- is XCG_ENOMEM)
    if (prc == XCG_RC_INVAL) return XCG_EINVAL;
    if (prc) return XCG_ENOMEM;
  }
  const int rc = xcg_ctx_create_ex(device, flags, C + xcg_pair_state_disk_blocks(P), out);
  if (rc != XCG_OK) {
    DeviceGuard g(device);
    xcg_pair_state_destroy(P);
    return rc;
  }
  (*out)->pair = P;
  (*out)->pair_C = (uint32_t)C;
  return XCG_OK;
}

int xcg_ctx_create_pair_unbounded(int device, uint32_t flags, uint64_t capacity_segments, xcg_disk* disk,
                                  const char* uuid36, int xuid, xcg_ctx** out) {
  if (capacity_segments == 0) capacity_segments = XCG_DEFAULT_CACHE_SEGMENTS;
  if (capacity_segments > (1ull << 28)) return XCG_EINVAL;
  const int rc = xcg_ctx_create_pair_xuid(device, flags, capacity_segments * XCG_SEGMENT_LENGTH, disk, uuid36, xuid,
                                          out);
  if (rc == XCG_OK) xcg_pair_state_set_unbounded((*out)->pair);
  return rc;
}

int xcg_ctx_create_pair(int device, uint32_t flags, uint64_t memory_cache_limit_bytes, uint64_t disk_bytes,
                        xcg_ctx** out) {
  if (!out) return XCG_EINVAL;
  xcg_disk* d = nullptr;
  int rc = xcg_disk_create(disk_bytes, &d);
  if (rc != XCG_OK) return rc;
  rc = xcg_ctx_create_pair_on(device, flags, memory_cache_limit_bytes, d, out);
  xcg_disk_destroy(d);                 // (the front holds the disk from here)
  return rc;
}

// XCodecCache::connect(uuid, parent) (xcodec/xcodec_cache.h:101-111) with
// the parent's connect: XCodecMemoryCache::connect (:340-346, an empty cache
// of the same limit), XCodecCachePair::connect (:158-161: the primary's connect
// over XCodecDisk::connect(uuid), xcodec_cache_disk.cc:640-690).
// `hold`: the caller (a connecting pipe) takes its hold on the context before
// g_reg_mu is released, so no registry clear can fall between the two.
static int ctx_connect(xcg_ctx* parent, const char* uuid36, bool hold, xcg_ctx** out) {
  std::string key;
  if (!parent || !out || !uuid_key(uuid36, &key)) return XCG_EINVAL;
  *out = nullptr;
  std::lock_guard<std::mutex> lk(g_reg_mu);
  auto it = g_reg.find(key);
  if (it != g_reg.end()) {
    *out = it->second.ctx;
    if (hold) ++g_holds[*out];
    return XCG_OK;
  }
  xcg_ctx* c = nullptr;
  int rc;
  if (parent->pair && xcg_pair_state_unbounded(parent->pair))
    rc = xcg_ctx_create_pair_unbounded(parent->device, parent->flags, parent->pair_C,
                                       (xcg_disk*)xcg_pair_state_disk(parent->pair), key.c_str(), -1, &c);
  else if (parent->pair)
    rc = xcg_ctx_create_pair_uuid(parent->device, parent->flags, (uint64_t)parent->pair_C * XCG_SEGMENT_LENGTH,
                                  (xcg_disk*)xcg_pair_state_disk(parent->pair), key.c_str(), &c);
  else if (parent->bounded)
    rc = xcg_ctx_create_bounded(parent->device, parent->flags, (uint64_t)parent->lru.C * XCG_SEGMENT_LENGTH, &c);
  else
    rc = xcg_ctx_create_ex(parent->device, parent->flags, parent->cache_segments, &c);
  if (rc != XCG_OK) return rc;
  g_reg[key] = RegEntry{c, true};
  *out = c;
  if (hold) ++g_holds[c];
  return XCG_OK;
}

int xcg_ctx_connect(xcg_ctx* parent, const char* uuid36, xcg_ctx** out) {
  return ctx_connect(parent, uuid36, false, out);
}

// XCodecCache::enter(uuid, cache) (:113-117): a context the caller keeps.
int xcg_ctx_register(xcg_ctx* c, const char* uuid36) {
  std::string key;
  if (!c || !uuid_key(uuid36, &key)) return XCG_EINVAL;
  std::lock_guard<std::mutex> lk(g_reg_mu);
  if (g_reg.count(key)) return XCG_EEXIST;
  g_reg[key] = RegEntry{c, false};
  return XCG_OK;
}

xcg_ctx* xcg_ctx_lookup(const char* uuid36) {
  std::string key;
  if (!uuid_key(uuid36, &key)) return nullptr;
  std::lock_guard<std::mutex> lk(g_reg_mu);
  auto it = g_reg.find(key);
  return it == g_reg.end() ? nullptr : it->second.ctx;
}

void xcg_connect_registry_clear(void) {
  std::vector<xcg_ctx*> owned;
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    for (auto& e : g_reg) {
      if (!e.second.owned) continue;
      if (g_holds.count(e.second.ctx)) g_deferred.insert(e.second.ctx);   // (a pipe still uses it)
      else owned.push_back(e.second.ctx);
    }
    g_reg.clear();
  }
  for (xcg_ctx* c : owned) xcg_ctx_destroy(c);
}

// (xcg_pipe.cpp, not part of the ABI) a connecting pipe takes and drops its context
extern "C" int xcg_ctx_connect_hold(xcg_ctx* parent, const char* uuid36, xcg_ctx** out) {
  return ctx_connect(parent, uuid36, true, out);
}
extern "C" void xcg_registry_release(xcg_ctx* c) {
  bool destroy = false;
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    auto it = g_holds.find(c);
    if (it == g_holds.end()) return;
    if (--it->second == 0) {
      g_holds.erase(it);
      destroy = g_deferred.erase(c) != 0;
    }
  }
  if (destroy) xcg_ctx_destroy(c);
}

int xcg_pair_stats(xcg_ctx* c, uint64_t* st) {
  if (!c || !c->pair || !st) return XCG_EINVAL;
  xcg_pair_state_stats(c->pair, st);
  return XCG_OK;
}

int xcg_ctx_create_ex(int device, uint32_t flags, uint64_t cache_segments, xcg_ctx** out) {
  if (!out || cache_segments == 0 || cache_segments > (1ull << 30)) return XCG_EINVAL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return XCG_EINVAL;
  if (flags & ~(XCG_FLAG_OOB | XCG_FLAG_NULLCACHE)) return XCG_EINVAL;
  DeviceGuard g(device);
  xcg_ctx* c = new xcg_ctx;
  c->device = device;
  c->flags = flags;
  c->cache_segments = cache_segments;
  auto fail = [&](int rc) {
    c->mem_call.release_all();
    if (c->done_ev) (void)hipEventDestroy(c->done_ev);
    if (c->flags_ev) (void)hipEventDestroy(c->flags_ev);
    delete c;
    return rc;
  };
  if (!(c->mem_call.dev(&c->d_status, 16) && c->mem_call.pinned(&c->h_status, 16))) return fail(XCG_ENOMEM);
  if (hipMemset(c->d_status, 0, 16) != hipSuccess ||
      hipEventCreateWithFlags(&c->done_ev, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->flags_ev, hipEventDisableTiming) != hipSuccess)
    return fail(XCG_EHIP);
  *out = c;
  return XCG_OK;
}

void xcg_ctx_destroy(xcg_ctx* c) {
  if (!c) return;
  registry_forget(c);
  DeviceGuard g(c->device);
  c->mem_call.release(c->d_status);
  c->mem_call.release(c->h_status);
  free_cache(c);
  free_lru(c);
  free_scratch(c);
  free_dscratch(c);
  window_free(c->own_win);
  if (c->done_ev) (void)hipEventDestroy(c->done_ev);
  if (c->flags_ev) (void)hipEventDestroy(c->flags_ev);
  xcg_pair_state_destroy(c->pair);
  c->mem_call.release_all();         // (the staging and the zero-copy block)
  if (c->call_st) (void)hipStreamDestroy(c->call_st);
  delete c;
}

uint64_t xcg_cache_size(xcg_ctx* c) {
  if (!c || !c->g.keys) return 0;
  DeviceGuard g(c->device);
  uint32_t n = 0;
  if (ctx_wait(c) != XCG_OK || hipMemcpy(&n, c->g.nseg, 4, hipMemcpyDeviceToHost) != hipSuccess)
    return 0;
  return n < c->g.seg_cap ? n : c->g.seg_cap;
}

int xcg_cache_clear(xcg_ctx* c) {
  if (!c) return XCG_EINVAL;
  if (!c->g.keys) return XCG_OK;
  DeviceGuard g(c->device);
  // The wipe is ordered behind the context's last work on the device; only a
  // pair, whose metadata lives on the host, waits for that work here.
  if (c->pair && ctx_wait(c) != XCG_OK) return XCG_EHIP;
  ctx_order(c, nullptr);
  // (the LRU clock keeps running: slots keep their last-reference times, which
  // must stay below every later batch's)
  if (c->pair && xcg_pair_state_clear(c->pair) != 0) return XCG_EHIP;
  // asynchronous: the context's later work waits for the wipe on the device
  // (ctx_order), host inspection calls wait for it (ctx_wait)
  const int rc = clear_cache(c->g, c->done_ev == nullptr);
  ctx_mark(c, nullptr);
  return rc;
}

void xcg_debug_mem_live(uint64_t out[4]) {
  for (int i = 0; i < 4; ++i) out[i] = xcg::HipMem::live[i].load();
}

int xcg_ctx_unbounded(const xcg_ctx* c) { return c && !c->bounded && !c->pair; }
int xcg_ctx_device(const xcg_ctx* c) { return c ? c->device : -1; }

int xcg_ctx_flags(const xcg_ctx* c, uint32_t* flags) {
  if (!c || !flags) return XCG_EINVAL;
  *flags = c->flags;
  return XCG_OK;
}

int xcg_ctx_status(xcg_ctx* c) {
  if (!c) return XCG_EINVAL;
  DeviceGuard g(c->device);
  int32_t st = 0;
  if (ctx_wait(c) != XCG_OK ||
      hipMemcpyAsync(c->h_status, c->d_status, sizeof st, hipMemcpyDeviceToHost, nullptr) != hipSuccess ||
      hipStreamSynchronize(nullptr) != hipSuccess)
    return XCG_EHIP;
  st = *c->h_status;
  if (st && getenv("XCG_STATUS_DEBUG")) fprintf(stderr, "xcg: context status word %#x\n", (unsigned)st);
  return st ? XCG_EOVERFLOW : XCG_OK;
}

}  // extern "C"
