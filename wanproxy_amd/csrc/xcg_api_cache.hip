// Cache inspection and host calls of the C ABI declared in include/xcgpu.h:
// single-segment lookup / enter on each kind of cache, bulk learn / export,
// the last batch's declaration and reference rows, and the debug dumps.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/xcgpu.h"
#include "xcg_args.h"
#include "xcg_cache.h"
#include "xcg_ctx.h"
#include "xcg_devmem.h"

using xcg::FILT_WORDS;

// (the reference rows' packing, restated without HIP in xcg_api_host.h)
static_assert(ROW_REF_MASK == xcg::EV_REF_MASK && (xcg::EV_GMISS >> (32 - ROW_KIND_SHIFT)) == 0, "reference rows");

extern "C" {

namespace {
// A small pinned + device staging area for single-segment host calls.
int host_seg_call(xcg_ctx* c, uint64_t hash, const uint8_t* in_seg, uint8_t* out_seg, int mode, int32_t* res) {
  DeviceGuard g(c->device);
  int rc = ensure_cache(c);
  if (rc != XCG_OK) return rc;
  xcg::DevMem mem;                   // (freed when the call returns)
  uint8_t* d_seg = nullptr;
  int32_t* d_res = nullptr;
  if (!(mem.dev(&d_seg, XCG_SEGMENT_LENGTH) && mem.dev(&d_res, 4))) return XCG_ENOMEM;
  rc = XCG_OK;
  if (mode == 0) {   // lookup
    if (xcg_launch_cache_lookup(&c->g, hash, d_seg, d_res, nullptr) != 0 ||
        hipMemcpy(res, d_res, 4, hipMemcpyDeviceToHost) != hipSuccess ||
        (*res && hipMemcpy(out_seg, d_seg, XCG_SEGMENT_LENGTH, hipMemcpyDeviceToHost) != hipSuccess))
      rc = XCG_EHIP;
  } else {           // enter (1) / replace (2)
    if (hipMemcpy(d_seg, in_seg, XCG_SEGMENT_LENGTH, hipMemcpyHostToDevice) != hipSuccess ||
        xcg_launch_cache_enter(&c->g, hash, d_seg, mode == 2, d_res, nullptr) != 0 ||
        hipMemcpy(res, d_res, 4, hipMemcpyDeviceToHost) != hipSuccess)
      rc = XCG_EHIP;
  }
  return rc;
}
}  // namespace

namespace {
// Single-segment host calls on a bounded cache: lookup (a hit refreshes the
// entry, xcodec_cache.h:348-364) and enter (XCodecPipePair's <LEARN>:
// lookup, then replace if the bytes differ or enter, evicting at the limit,
// xcodec_pipe_pair.cc:311-327) -- as a one-reference batch through the LRU
// pass and commit (xcg_lru.hip).
int lru_host_call(xcg_ctx* c, uint64_t hash, const uint8_t* in_seg, uint8_t* out_seg, int enter, int32_t* found) {
  DeviceGuard g(c->device);
  int rc = ensure_cache(c);
  if (rc != XCG_OK) return rc;
  // device scratch: [0, 2048) new bytes, [2048, 4096) old bytes, then the batch
  xcg::DevMem mem;                   // (freed when the call returns)
  uint8_t* m = nullptr;
  if (!mem.dev(&m, 8192)) return XCG_ENOMEM;
  uint8_t* d_new = m;
  uint8_t* d_old = m + 2048;
  int32_t* d_res = (int32_t*)(m + 4096);
  rc = XCG_OK;
  do {
    if (xcg_launch_cache_lookup(&c->g, hash, d_old, d_res, nullptr) != 0 ||
        hipMemcpy(found, d_res, 4, hipMemcpyDeviceToHost) != hipSuccess) {
      rc = XCG_EHIP;
      break;
    }
    if (*found && out_seg && hipMemcpy(out_seg, d_old, XCG_SEGMENT_LENGTH, hipMemcpyDeviceToHost) != hipSuccess) {
      rc = XCG_EHIP;
      break;
    }
    if (!*found && !enter) break;                   // a miss changes nothing
    if (enter && hipMemcpy(d_new, in_seg, XCG_SEGMENT_LENGTH, hipMemcpyHostToDevice) != hipSuccess) {
      rc = XCG_EHIP;
      break;
    }
    int32_t res = 0;
    if (enter && *found &&                          // replace (the table entry stays)
        (xcg_launch_cache_enter(&c->g, hash, d_new, 1, d_res, nullptr) != 0 ||
         hipMemcpy(&res, d_res, 4, hipMemcpyDeviceToHost) != hipSuccess)) {
      rc = XCG_EHIP;
      break;
    }
    // the one-reference batch: chunk 0 = the new bytes; an ENTER (declaration
    // row 0) or a HIT at time 1
    struct {
      uint64_t chunk_off;
      uint32_t ev[4], decl[4];
      uint32_t nev, ndecl, need, pad;
      uint32_t ev_base[2], enter_base[2];
      uint32_t evslot[2];
      uint64_t evtime[2];
    } h{};
    const uint32_t lo = (uint32_t)hash, hi = (uint32_t)(hash >> 32);
    h.ev[0] = lo; h.ev[1] = hi;
    h.ev[2] = *found ? 1u : 0u;
    h.ev[3] = *found ? (1u << 30) : 0u;             // EV_HIT / EV_ENTER d = 0
    h.decl[0] = lo; h.decl[1] = hi;
    h.nev = 1;
    h.ndecl = *found ? 0u : 1u;
    uint8_t* d_h = m + 4608;
    if (hipMemcpy(d_h, &h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) {
      rc = XCG_EHIP;
      break;
    }
    auto at = [&](const void* field) { return d_h + ((const uint8_t*)field - (const uint8_t*)&h); };
    XcgLruState& L = c->lru;
    LruBatch b{};
    b.ev_base = (uint32_t*)at(h.ev_base);
    b.enter_base = (uint32_t*)at(h.enter_base);
    b.evslot = (uint32_t*)at(h.evslot);
    b.evtime = (uint64_t*)at(h.evtime);
    b.n = 1; b.in = d_new; b.chunk_off = (const uint64_t*)at(&h.chunk_off);
    b.decl = at(h.decl); b.ndecl = (const uint32_t*)at(&h.ndecl); b.maxd = 1;
    b.ev = at(h.ev); b.nev = (const uint32_t*)at(&h.nev); b.maxe = 1;
    b.need = (uint32_t*)at(&h.need);
    b.g = c->g;
    b.status = c->d_status;
    b.ev_bound = 1;
    if (xcg_lru_times(&b, &L, nullptr) != 0 || xcg_lru_commit(&b, &L, nullptr) != 0 ||
        hipStreamSynchronize(nullptr) != hipSuccess)
      rc = XCG_EHIP;
  } while (0);
  return rc;
}
}  // namespace

namespace {
// Single-segment host calls on a pair: a one-op decode batch that leaves the
// BACKREF window alone.  A lookup is <REF hash> (XCodecCachePair::lookup, with
// its LRU use / disk touch / promotion, xcodec_cache.h:208-230); an enter is
// <EXTRACT seg> -- lookup, then nothing (same bytes), replace (other bytes) or
// enter (absent), exactly <LEARN>'s sequence (xcodec_pipe_pair.cc:311-327).
int pair_host_call(xcg_ctx* c, uint64_t hash, const uint8_t* in_seg, uint8_t* out_seg, int32_t* found) {
  uint8_t op[2 + XCG_SEGMENT_LENGTH];
  uint32_t len;
  op[0] = 0xF1;
  if (in_seg) {
    op[1] = 0x01;
    memcpy(op + 2, in_seg, XCG_SEGMENT_LENGTH);
    len = 2 + XCG_SEGMENT_LENGTH;
  } else {
    op[1] = 0x02;
    for (int k = 0; k < 8; ++k) op[2 + k] = (uint8_t)(hash >> (56 - 8 * k));
    len = 10;
  }
  const uint64_t off = 0;
  uint64_t ooff = 0, olen = 0, cons = 0, unk = 0;
  int32_t st = 0;
  uint32_t nunk = 0;
  uint8_t out[XCG_SEGMENT_LENGTH];
  c->no_window = true;
  const int rc = xcg_decode_host(c, op, len, &off, &len, 1, out, sizeof out, &ooff, &olen, &st, &cons, &unk, 1, &nunk);
  c->no_window = false;
  if (rc != XCG_OK) return rc;
  if (st < 0) return XCG_EHIP;
  *found = st == 0 && olen == XCG_SEGMENT_LENGTH;
  if (*found && out_seg) memcpy(out_seg, out, XCG_SEGMENT_LENGTH);
  return XCG_OK;
}
}  // namespace

int xcg_cache_lookup_host(xcg_ctx* c, uint64_t hash, uint8_t* seg_out) {
  if (!c || !seg_out) return XCG_EINVAL;
  if (c->pair) {
    int32_t found = 0;
    const int rc = pair_host_call(c, hash, nullptr, seg_out, &found);
    return rc != XCG_OK ? rc : (found ? XCG_OK : XCG_ENOENT);
  }
  if (c->bounded) {
    int32_t found = 0;
    const int rc = lru_host_call(c, hash, nullptr, seg_out, 0, &found);
    return rc != XCG_OK ? rc : (found ? XCG_OK : XCG_ENOENT);
  }
  int32_t found = 0;
  const int rc = host_seg_call(c, hash, nullptr, seg_out, 0, &found);
  if (rc != XCG_OK) return rc;
  return found ? XCG_OK : XCG_ENOENT;
}

int xcg_cache_enter_host(xcg_ctx* c, uint64_t hash, const uint8_t* seg) {
  if (!c || !seg) return XCG_EINVAL;
  if (c->pair) {
    if (xcg::host_seg_hash(seg) != hash) return XCG_EINVAL;   // (a pair names a segment by its own hash)
    int32_t found = 0;
    return pair_host_call(c, hash, seg, nullptr, &found);
  }
  if (c->bounded) {
    int32_t found = 0;
    return lru_host_call(c, hash, seg, nullptr, 1, &found);
  }
  int32_t res = 0;
  const int rc = host_seg_call(c, hash, seg, nullptr, 1, &res);
  if (rc != XCG_OK) return rc;
  return res == -2 ? XCG_EOVERFLOW : XCG_OK;
}

// Bulk learn / export of a memory cache (xcg_cache_bulk.hip): n <LEARN>
// sequences in one pass, and every live (hash, segment) in a fixed order.
int xcg_cache_learn_batch(xcg_ctx* c, const uint8_t* d_segs, uint64_t n, uint64_t* d_hash, void* stream) {
  if (!c || (n && !d_segs) || n > (1ull << 30)) return XCG_EINVAL;
  if (c->pair) return XCG_ENOTSUP;
  if (n == 0) return XCG_OK;
  DeviceGuard g(c->device);
  int rc = ensure_cache(c);
  if (rc != XCG_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  ctx_order(c, st);
  XcgBulkLearn a{};
  a.segs = d_segs;
  a.n = n;
  a.hash_out = d_hash;
  a.g = c->g;
  a.lru = c->bounded ? &c->lru : nullptr;
  a.status = c->d_status;
  rc = xcg_bulk_learn(&a, st);
  ctx_mark(c, st);
  return status_of(rc);
}

int xcg_cache_learn_host(xcg_ctx* c, const uint8_t* h_segs, uint64_t n, uint64_t* h_hash) {
  if (!c || (n && !h_segs) || n > (1ull << 30)) return XCG_EINVAL;
  if (c->pair) return XCG_ENOTSUP;
  if (n == 0) return XCG_OK;
  DeviceGuard g(c->device);
  xcg::DevMem mem;                   // (freed when the call returns)
  uint8_t* d_segs = nullptr;
  uint64_t* d_hash = nullptr;
  if (!(mem.dev(&d_segs, n * XCG_SEGMENT_LENGTH) && (!h_hash || mem.dev(&d_hash, 8 * n)))) return XCG_ENOMEM;
  if (hipMemcpy(d_segs, h_segs, n * XCG_SEGMENT_LENGTH, hipMemcpyHostToDevice) != hipSuccess) return XCG_EHIP;
  const int rc = xcg_cache_learn_batch(c, d_segs, n, d_hash, nullptr);
  // (the copy back, or the wait alone, also keeps d_segs alive until the pass has read it)
  if (h_hash ? hipMemcpy(h_hash, d_hash, 8 * n, hipMemcpyDeviceToHost) != hipSuccess
             : hipStreamSynchronize(nullptr) != hipSuccess)
    return rc != XCG_OK ? rc : XCG_EHIP;
  return rc;
}

int xcg_cache_export(xcg_ctx* c, uint8_t* d_segs, uint64_t* d_hash, uint64_t cap_segments, uint64_t* h_count,
                     void* stream) {
  if (!c || !h_count) return XCG_EINVAL;
  if (c->pair) return XCG_ENOTSUP;
  *h_count = 0;
  if (!c->g.keys) return XCG_OK;
  DeviceGuard g(c->device);
  uint32_t live = 0;
  if (ctx_wait(c) != XCG_OK || hipMemcpy(&live, c->g.nseg, 4, hipMemcpyDeviceToHost) != hipSuccess) return XCG_EHIP;
  if (live > c->g.seg_cap) live = c->g.seg_cap;
  *h_count = live;
  if (live > cap_segments) return XCG_EOVERFLOW;
  if (live == 0) return XCG_OK;
  if (!d_segs) return XCG_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  ctx_order(c, st);
  const int rc = xcg_bulk_export(&c->g, c->bounded ? &c->lru : nullptr, live, d_segs, d_hash, st);
  ctx_mark(c, st);
  return status_of(rc);
}

int xcg_cache_export_host(xcg_ctx* c, uint8_t* h_segs, uint64_t* h_hash, uint64_t cap_segments, uint64_t* h_count) {
  if (!c || !h_count) return XCG_EINVAL;
  if (c->pair) return XCG_ENOTSUP;
  const uint64_t live = xcg_cache_size(c);
  *h_count = live;
  if (live > cap_segments) return XCG_EOVERFLOW;
  if (live == 0) return XCG_OK;
  if (!h_segs) return XCG_EINVAL;
  DeviceGuard g(c->device);
  xcg::DevMem mem;                   // (freed when the call returns)
  uint8_t* d_segs = nullptr;
  uint64_t* d_hash = nullptr;
  if (!(mem.dev(&d_segs, live * XCG_SEGMENT_LENGTH) && mem.dev(&d_hash, 8 * live))) return XCG_ENOMEM;
  const int rc = xcg_cache_export(c, d_segs, d_hash, live, h_count, nullptr);
  if (rc != XCG_OK) return rc;
  if (hipMemcpy(h_segs, d_segs, live * XCG_SEGMENT_LENGTH, hipMemcpyDeviceToHost) != hipSuccess ||
      (h_hash && hipMemcpy(h_hash, d_hash, 8 * live, hipMemcpyDeviceToHost) != hipSuccess))
    return XCG_EHIP;
  return XCG_OK;
}

int xcg_last_declarations(xcg_ctx* c, uint32_t chunk, uint64_t* h_hash, uint32_t* h_pos, uint32_t cap,
                          uint32_t* h_count) {
  if (!c || !h_count || !c->bs.decl) return XCG_EINVAL;
  if (c->bounded || c->pair) {                         // rows of the last sub-batch only
    const uint32_t base = c->pair ? xcg_pair_state_last_base(c->pair) : c->lru.last_base;
    if (chunk < base) return XCG_ENOTSUP;
    chunk -= base;
  }
  if (chunk >= c->bs.n_cap) return XCG_EINVAL;
  DeviceGuard g(c->device);
  uint32_t nd = 0;
  if (ctx_wait(c) != XCG_OK ||
      hipMemcpy(&nd, c->bs.ndecl + chunk, 4, hipMemcpyDeviceToHost) != hipSuccess)
    return XCG_EHIP;
  *h_count = nd;
  const uint32_t k = nd < cap ? nd : cap;
  if (k == 0) return XCG_OK;
  std::vector<uint32_t> buf(4ull * k);                 // (only the rows that fit the cap are read)
  if (hipMemcpy(buf.data(), (const uint8_t*)c->bs.decl + 16ull * chunk * c->bs.last_maxd, 16ull * k,
                hipMemcpyDeviceToHost) != hipSuccess)
    return XCG_EHIP;
  unpack_decl_rows(buf.data(), nd, cap, h_hash, h_pos);
  return XCG_OK;
}

int xcg_last_references(xcg_ctx* c, uint32_t chunk, uint64_t* h_hash, uint32_t* h_kind, uint32_t* h_ref,
                        uint32_t cap, uint32_t* h_count) {
  if (!c || !h_count) return XCG_EINVAL;
  if (!(c->bounded || c->pair) || !c->bs.ev) return XCG_ENOTSUP;
  const uint32_t base = c->pair ? xcg_pair_state_last_base(c->pair) : c->lru.last_base;
  if (chunk < base) return XCG_ENOTSUP;
  chunk -= base;
  if (chunk >= c->bs.n_cap) return XCG_EINVAL;
  DeviceGuard g(c->device);
  uint32_t ne = 0;
  if (ctx_wait(c) != XCG_OK || hipMemcpy(&ne, c->bs.nev + chunk, 4, hipMemcpyDeviceToHost) != hipSuccess)
    return XCG_EHIP;
  if (ne > c->bs.maxe) return XCG_EOVERFLOW;
  *h_count = ne;
  std::vector<uint32_t> buf(4ull * ne);
  if (ne && hipMemcpy(buf.data(), (const uint8_t*)c->bs.ev + 16ull * chunk * c->bs.maxe, 16ull * ne,
                      hipMemcpyDeviceToHost) != hipSuccess)
    return XCG_EHIP;
  unpack_ref_rows(buf.data(), ne, cap, h_hash, h_kind, h_ref);
  return XCG_OK;
}

int xcg_debug_restart_counts(xcg_ctx* c, uint64_t* resumed, uint64_t* spliced) {
  if (!c || !resumed || !spliced) return XCG_EINVAL;
  *resumed = *spliced = 0;
  if (!c->bs.b_count) return XCG_OK;
  DeviceGuard g(c->device);
  uint32_t v[4] = {0, 0, 0, 0};
  if (ctx_wait(c) != XCG_OK || hipMemcpy(v, c->bs.b_count, 16, hipMemcpyDeviceToHost) != hipSuccess) return XCG_EHIP;
  *resumed = v[2];
  *spliced = v[3];
  return XCG_OK;
}

int xcg_debug_cache_dump(xcg_ctx* c, uint32_t* h_filt, uint32_t* h_ftab, uint64_t ftab_words, uint32_t* h_fmask) {
  if (!c || !c->g.keys) return XCG_EINVAL;
  DeviceGuard g(c->device);
  *h_fmask = c->g.fmask;
  if (ctx_wait(c) != XCG_OK) return XCG_EHIP;
  if (h_filt && hipMemcpy(h_filt, c->g.filt, 4ull * FILT_WORDS, hipMemcpyDeviceToHost) != hipSuccess) return XCG_EHIP;
  const uint64_t tw = 4ull * (c->g.fmask + 1);
  if (h_ftab && hipMemcpy(h_ftab, c->g.ftab, 4ull * (ftab_words < tw ? ftab_words : tw), hipMemcpyDeviceToHost) !=
                    hipSuccess)
    return XCG_EHIP;
  return XCG_OK;
}

}  // extern "C"
