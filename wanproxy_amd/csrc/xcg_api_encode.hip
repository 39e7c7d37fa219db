// Encode entry points of the C ABI declared in include/xcgpu.h: batch, host,
// call and grouped, and the device-side helpers around them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/xcgpu.h"
#include "xcg_args.h"
#include "xcg_cache.h"
#include "xcg_ctx.h"

using xcg::align_up;

namespace {

// Stream-round seeding: -1 automatic, 0 never, 1 always (tests exercise both).
int g_stream_seed = -1;

// A stream batch's driver arguments from the context (its cache and scratch,
// ensure_cache / ensure_scratch done) and the call: the same for the plain,
// bounded and pair drivers.
XcgStreamArgs stream_args(xcg_ctx* c, const uint8_t* d_in, const uint64_t* d_chunk_off, const uint32_t* d_chunk_len,
                          uint32_t n, uint32_t maxd, uint8_t* d_out, const uint64_t* d_out_off, uint64_t* d_out_len,
                          uint32_t* d_stats) {
  XcgStreamArgs a{};
  static_cast<XcgBatchScratch&>(a) = c->bs;          // every scratch array (bounded / pair ones: null elsewhere)
  a.in = d_in; a.chunk_off = d_chunk_off; a.chunk_len = d_chunk_len; a.n = n;
  a.flags = c->flags;
  a.out = d_out; a.out_off = d_out_off; a.out_len = d_out_len;
  a.stats = d_stats;
  a.status = c->d_status;
  a.g = c->g;
  a.maxd = maxd;
  // Seed the rounds with the chunks' 2048-byte tilings instead of a parse
  // round 0 when the last batch declared segments (cold / growing caches);
  // a warm cache's all-REF batches keep round 0, which then is all they need.
  const int mode = __atomic_load_n(&g_stream_seed, __ATOMIC_RELAXED);
  a.seed = mode < 0 ? (c->seed_next ? 1 : 0) : mode;
  if (getenv("XCG_NO_APROBE")) a.a_bits = nullptr;
  a.flags_ev = c->flags_ev;
  if (c->pair || c->bounded) a.restart = getenv("XCG_NO_RESTART") ? 0 : 1;
  return a;
}

int encode_batch_impl(xcg_ctx* c, int semantics, const uint8_t* d_in, const uint64_t* d_chunk_off,
                      const uint32_t* d_chunk_len, uint32_t n, uint32_t max_chunk_len, uint8_t* d_out,
                      const uint64_t* d_out_off, uint64_t* d_out_len, uint32_t* d_stats, void* stream) {
  if (!c) return XCG_EINVAL;
  if (n == 0) return XCG_OK;
  if (!d_in || !d_chunk_off || !d_chunk_len || !d_out || !d_out_off || !d_out_len) return XCG_EINVAL;
  if (semantics != XCG_SEM_INDEPENDENT && semantics != XCG_SEM_STREAM) return XCG_EINVAL;
  if (max_chunk_len > (1u << 19)) return XCG_EINVAL;
  DeviceGuard g(c->device);
  ctx_order(c, (hipStream_t)stream);
  c->last_stream_n = 0;              // (set again below once a stream batch has left its rows)
  // A null cache has no state to carry: both semantics are the same pass.
  if (semantics == XCG_SEM_STREAM && !(c->flags & XCG_FLAG_NULLCACHE)) {
    // declaration slots per chunk: a chunk of L bytes declares at most L / 2048
    const uint32_t maxd = max_chunk_len / XCG_SEGMENT_LENGTH + 1;
    int rc = ensure_cache(c);
    if (rc == XCG_OK) rc = ensure_scratch(c, n, maxd);
    if (rc != XCG_OK) return rc;
    c->bs.last_maxd = maxd;
    XcgStreamArgs a = stream_args(c, d_in, d_chunk_off, d_chunk_len, n, maxd, d_out, d_out_off, d_out_len, d_stats);
    uint32_t decls = ~0u;
    a.decls_out = &decls;
    int rounds = 0;
    if (c->pair) {
      rc = xcg_pair_encode_stream(&a, c->pair, &rounds, (hipStream_t)stream);
    } else if (c->bounded) {
      rc = xcg_lru_encode_stream(&a, &c->lru, &rounds, (hipStream_t)stream);
    } else {
      rc = xcg_launch_encode_stream(&a, &rounds, (hipStream_t)stream);
      if (decls != ~0u) c->seed_next = decls > 0;
    }
    c->last_rounds = rounds;
    if (rc == 0) c->last_stream_n = n;
    return status_of(rc);   // (0, XCG_RC_HIP, _OVERFLOW, and from the bounded and pair drivers _NOTSUP)
  }
  // A fresh bounded cache per chunk evicts nothing while the chunk's
  // declarations fit the limit (at most max_chunk_len / 2048 of them).
  if (!ctx_fresh_cache_fits(c, chunk_declarations(max_chunk_len))) return XCG_ENOTSUP;
  int rc = xcg_launch_encode_independent(d_in, d_chunk_off, d_chunk_len, n, max_chunk_len, c->flags, d_out,
                                         d_out_off, d_out_len, d_stats, c->d_status, (hipStream_t)stream);
  return status_of(rc);   // (0, XCG_RC_INVAL or XCG_RC_HIP)
}

// xcg_encode_host, and with `rm` xcg_encode_host_refmap: the same call with the
// refmap launch behind the batch, its rows beside the lengths.  With `d_keep`
// (xcg_encode_host_refmap_device) the call ends after its first
// synchronisation: lengths, status and rows are on the host, the encodings stay
// in the staging's output slots, *d_keep.
struct HostRefmap {
  uint64_t* hash;
  uint32_t* pos;
  uint32_t cap;
  uint32_t* count;
};

int encode_host_impl(xcg_ctx* c, int semantics, const uint8_t* h_in, uint64_t in_len, const uint64_t* h_chunk_off,
                     const uint32_t* h_chunk_len, uint32_t n, uint8_t* h_out, uint64_t out_cap,
                     const uint64_t* h_out_off, uint64_t* h_out_len, const HostRefmap* rm,
                     const uint8_t** d_keep = nullptr) {
  if (!c || (n && (!h_in || !h_chunk_off || !h_chunk_len || (!h_out && !d_keep) || !h_out_off || !h_out_len)))
    return XCG_EINVAL;
  if (n == 0) return XCG_OK;
  uint32_t maxlen = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (h_chunk_off[i] + h_chunk_len[i] > in_len) return XCG_EINVAL;
    if (h_out_off[i] + xcg_encode_bound(h_chunk_len[i]) > out_cap) return XCG_EINVAL;
    if (h_chunk_len[i] > maxlen) maxlen = h_chunk_len[i];
  }
  DeviceGuard g(c->device);
  // staging (kept by the context): [off n][oo n][ol n][len n] | input | output slots
  //                                | (refmap) [count n][hash n * cap][pos n * cap]
  const size_t meta = align_up(28ull * n, 256), inb = align_up(in_len ? in_len : 1, 256),
               outb = align_up(out_cap ? out_cap : 1, 256);
  const uint64_t rows = rm ? (uint64_t)n * rm->cap : 0;
  const size_t rcnt = rm ? align_up(4ull * n, 256) : 0, rhash = rm ? align_up(8ull * rows + 1, 256) : 0,
               rpos = rm ? align_up(4ull * rows + 1, 256) : 0;
  const size_t refb = rcnt + rhash + rpos;
  int rc = ensure_stage(c, meta + inb + outb + refb, meta + inb + outb + refb);
  if (rc != XCG_OK) return rc;
  uint8_t* hm = c->stage_h;
  uint8_t* dm = c->stage_d;
  memcpy(hm, h_chunk_off, 8ull * n);
  memcpy(hm + 8ull * n, h_out_off, 8ull * n);
  memcpy(hm + 24ull * n, h_chunk_len, 4ull * n);
  memcpy(hm + meta, h_in, in_len);
  const hipStream_t st = c->call_st;
  const uint64_t* d_off = (const uint64_t*)dm;
  const uint64_t* d_oo = (const uint64_t*)(dm + 8ull * n);
  uint64_t* d_ol = (uint64_t*)(dm + 16ull * n);
  const uint32_t* d_len = (const uint32_t*)(dm + 24ull * n);
  uint8_t* d_out = dm + meta + inb;
  const size_t ref0 = meta + inb + outb;
  if (hipMemcpyAsync(dm, hm, meta + in_len, hipMemcpyHostToDevice, st) != hipSuccess) return XCG_EHIP;
  rc = xcg_encode_batch(c, semantics, dm + meta, d_off, d_len, n, maxlen, d_out, d_oo, d_ol, nullptr, st);
  if (rc != XCG_OK) return rc;
  if (rm) {
    rc = xcg_encode_refmap_batch(c, d_out, d_oo, d_ol, n, (uint32_t)xcg_encode_bound(maxlen), 0,
                                 (uint64_t*)(dm + ref0 + rcnt), (uint32_t*)(dm + ref0 + rcnt + rhash), rm->cap,
                                 (uint32_t*)(dm + ref0), nullptr, st);
    if (rc != XCG_OK) return rc;
  }
  uint64_t* ol = (uint64_t*)(hm + 16ull * n);
  if (hipMemcpyAsync(ol, d_ol, 8ull * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(c->h_status, c->d_status, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      (rm && hipMemcpyAsync(hm + ref0, dm + ref0, rcnt + rhash + 4ull * rows, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      hipStreamSynchronize(st) != hipSuccess)
    return XCG_EHIP;
  if (*c->h_status) return XCG_EOVERFLOW;
  // only the bytes each slot holds come back
  uint8_t* ho = hm + meta + inb;
  for (uint32_t i = 0; i < n; ++i) {
    h_out_len[i] = ol[i];
    if (!d_keep && ol[i] && hipMemcpyAsync(ho + h_out_off[i], d_out + h_out_off[i], ol[i], hipMemcpyDeviceToHost, st) != hipSuccess)
      return XCG_EHIP;
  }
  if (rm) {                                          // (entries past a chunk's count stay as the caller left them)
    const uint32_t* cnt = (const uint32_t*)(hm + ref0);
    const uint64_t* hh = (const uint64_t*)(hm + ref0 + rcnt);
    const uint32_t* hp = (const uint32_t*)(hm + ref0 + rcnt + rhash);
    for (uint32_t i = 0; i < n; ++i) {
      rm->count[i] = cnt[i];
      const uint32_t k = cnt[i] < rm->cap ? cnt[i] : rm->cap;
      if (k) {
        memcpy(rm->hash + (uint64_t)i * rm->cap, hh + (uint64_t)i * rm->cap, 8ull * k);
        memcpy(rm->pos + (uint64_t)i * rm->cap, hp + (uint64_t)i * rm->cap, 4ull * k);
      }
    }
  }
  if (d_keep) {
    *d_keep = d_out;
    return XCG_OK;
  }
  if (hipStreamSynchronize(st) != hipSuccess) return XCG_EHIP;
  for (uint32_t i = 0; i < n; ++i)
    if (ol[i]) memcpy(h_out + h_out_off[i], ho + h_out_off[i], ol[i]);
  return XCG_OK;
}
}  // namespace

extern "C" {

int xcg_debug_set_stream_seed(int mode) {
  return __atomic_exchange_n(&g_stream_seed, mode < 0 ? -1 : (mode ? 1 : 0), __ATOMIC_RELAXED);
}

int xcg_last_rounds(xcg_ctx* c) { return c ? c->last_rounds : -1; }

int xcg_encode_batch(xcg_ctx* c, int semantics, const uint8_t* d_in, const uint64_t* d_chunk_off,
                     const uint32_t* d_chunk_len, uint32_t n, uint32_t max_chunk_len, uint8_t* d_out,
                     const uint64_t* d_out_off, uint64_t* d_out_len, uint32_t* d_stats, void* stream) {
  const int rc = encode_batch_impl(c, semantics, d_in, d_chunk_off, d_chunk_len, n, max_chunk_len, d_out, d_out_off,
                                   d_out_len, d_stats, stream);
  if (c) {
    DeviceGuard g(c->device);
    ctx_mark(c, (hipStream_t)stream);
  }
  return rc;
}

int xcg_encode_host(xcg_ctx* c, int semantics, const uint8_t* h_in, uint64_t in_len, const uint64_t* h_chunk_off,
                    const uint32_t* h_chunk_len, uint32_t n, uint8_t* h_out, uint64_t out_cap,
                    const uint64_t* h_out_off, uint64_t* h_out_len) {
  return encode_host_impl(c, semantics, h_in, in_len, h_chunk_off, h_chunk_len, n, h_out, out_cap, h_out_off,
                          h_out_len, nullptr);
}

int xcg_encode_host_refmap(xcg_ctx* c, int semantics, const uint8_t* h_in, uint64_t in_len,
                           const uint64_t* h_chunk_off, const uint32_t* h_chunk_len, uint32_t n, uint8_t* h_out,
                           uint64_t out_cap, const uint64_t* h_out_off, uint64_t* h_out_len, uint64_t* h_ref_hash,
                           uint32_t* h_ref_pos, uint32_t ref_cap, uint32_t* h_ref_count) {
  if (!h_ref_hash || !h_ref_pos || !h_ref_count) return XCG_EINVAL;
  const HostRefmap rm{h_ref_hash, h_ref_pos, ref_cap, h_ref_count};
  return encode_host_impl(c, semantics, h_in, in_len, h_chunk_off, h_chunk_len, n, h_out, out_cap, h_out_off,
                          h_out_len, &rm);
}

int xcg_encode_host_refmap_device(xcg_ctx* c, int semantics, const uint8_t* h_in, uint64_t in_len,
                                  const uint64_t* h_chunk_off, const uint32_t* h_chunk_len, uint32_t n,
                                  uint64_t out_cap, const uint64_t* h_out_off, uint64_t* h_out_len,
                                  uint64_t* h_ref_hash, uint32_t* h_ref_pos, uint32_t ref_cap, uint32_t* h_ref_count,
                                  const uint8_t** d_out) {
  if (!h_ref_hash || !h_ref_pos || !h_ref_count || !d_out) return XCG_EINVAL;
  *d_out = nullptr;
  const HostRefmap rm{h_ref_hash, h_ref_pos, ref_cap, h_ref_count};
  return encode_host_impl(c, semantics, h_in, in_len, h_chunk_off, h_chunk_len, n, nullptr, out_cap, h_out_off,
                          h_out_len, &rm, d_out);
}

int xcg_encode_refmap_batch(xcg_ctx* c, const uint8_t* d_enc, const uint64_t* d_enc_off, const uint64_t* d_enc_len,
                            uint32_t n, uint32_t max_enc_len, uint32_t first_chunk, uint64_t* d_ref_hash,
                            uint32_t* d_ref_pos, uint32_t ref_cap, uint32_t* d_ref_count, uint64_t* d_ref_walked,
                            void* stream) {
  if (!c) return XCG_EINVAL;
  if (n == 0) return XCG_OK;
  if (!d_enc || !d_enc_off || !d_enc_len || !d_ref_hash || !d_ref_pos || !d_ref_count) return XCG_EINVAL;
  if (max_enc_len > xcg_encode_bound(1u << 19)) return XCG_EINVAL;
  XcgRefmapArgs a{};
  a.enc = d_enc; a.enc_off = d_enc_off; a.enc_len = d_enc_len; a.n = n;
  a.max_len = max_enc_len;
  a.collect = (c->flags & XCG_FLAG_NULLCACHE) ? 0 : 1;
  if (a.collect && (c->flags & XCG_FLAG_OOB)) {
    // the declaration rows of the chunks [first_chunk, first_chunk + n) of the last stream batch
    if (!c->last_stream_n || !c->bs.decl || !c->bs.ndecl) return XCG_ENOTSUP;
    uint32_t base = 0;                                 // (bounded: rows of the last sub-batch only)
    if (c->bounded || c->pair) base = c->pair ? xcg_pair_state_last_base(c->pair) : c->lru.last_base;
    if (first_chunk < base) return XCG_ENOTSUP;
    if ((uint64_t)first_chunk + n > c->last_stream_n) return XCG_EINVAL;
    const uint32_t row0 = first_chunk - base;
    a.maxd = c->bs.last_maxd;
    a.decl = (const uint8_t*)c->bs.decl + 16ull * row0 * a.maxd;
    a.ndecl = c->bs.ndecl + row0;
  }
  a.ref_hash = d_ref_hash; a.ref_pos = d_ref_pos; a.ref_cap = ref_cap;
  a.ref_count = d_ref_count;
  a.walked = d_ref_walked;
  a.status = c->d_status;
  DeviceGuard g(c->device);
  ctx_order(c, (hipStream_t)stream);
  const int rc = xcg_launch_encode_refmap(&a, (hipStream_t)stream);
  ctx_mark(c, (hipStream_t)stream);
  return status_of(rc);   // (0, XCG_RC_INVAL or XCG_RC_HIP)
}

int xcg_encode_call(xcg_ctx* c, const uint8_t* h_in, uint32_t len, uint8_t* h_out, uint64_t out_cap,
                    uint64_t* h_out_len, uint64_t* h_decl_hash, uint32_t* h_decl_pos, uint32_t decl_cap,
                    uint32_t* h_ndecl, uint64_t* h_ref_hash, uint32_t* h_ref_kind, uint32_t* h_ref_idx, uint32_t ref_cap,
                    uint32_t* h_nref) {
  if (!c || !h_out_len || !h_ndecl || !h_nref || (len && (!h_in || !h_out))) return XCG_EINVAL;
  *h_out_len = 0;
  *h_ndecl = 0;
  *h_nref = (c->bounded || c->pair) ? 0u : XCG_NO_REFERENCES;
  if (len == 0) return XCG_OK;
  if (out_cap < xcg_encode_bound(len) || len > (1u << 19)) return XCG_EINVAL;
  DeviceGuard g(c->device);
  const bool nullc = (c->flags & XCG_FLAG_NULLCACHE) != 0;
  const bool refs = (c->bounded || c->pair) && !nullc;
  const uint32_t maxd = len / XCG_SEGMENT_LENGTH + 1;
  // staging: device [off 8][oo 8][ol 8][len 4] | input | output slot;
  //          host   the same head, then [ndecl 4][nev 4] | decl rows | event rows | output
  const uint64_t bound = xcg_encode_bound(len);
  const size_t inb = align_up(len, 256), outb = align_up(bound, 256);
  const size_t rows_d = align_up(16ull * maxd, 256);
  size_t rows_e = 0;
  if (refs) {
    int rc0 = ensure_cache(c);
    if (rc0 == XCG_OK) rc0 = ensure_scratch(c, 1, maxd);
    if (rc0 != XCG_OK) return rc0;
    rows_e = align_up(16ull * c->bs.maxe, 256);
  }
  int rc = ensure_stage(c, 256 + inb + outb, 256 + inb + 256 + rows_d + rows_e + outb);
  if (rc != XCG_OK) return rc;
  uint8_t* hm = c->stage_h;
  uint8_t* dm = c->stage_d;
  uint64_t* hmeta = (uint64_t*)hm;
  hmeta[0] = 0;                                      // chunk offset
  hmeta[1] = 0;                                      // output slot offset
  hmeta[2] = 0;
  *(uint32_t*)(hm + 24) = len;
  memcpy(hm + 256, h_in, len);
  const hipStream_t st = c->call_st;
  uint8_t* d_out = dm + 256 + inb;
  if (hipMemcpyAsync(dm, hm, 256 + len, hipMemcpyHostToDevice, st) != hipSuccess) return XCG_EHIP;
  rc = xcg_encode_batch(c, XCG_SEM_STREAM, dm + 256, (const uint64_t*)dm, (const uint32_t*)(dm + 24), 1, len, d_out,
                        (const uint64_t*)(dm + 8), (uint64_t*)(dm + 16), nullptr, st);
  if (rc != XCG_OK) return rc;
  // everything the call produced, back in one synchronisation
  uint8_t* hres = hm + 256 + inb;
  uint32_t* hcnt = (uint32_t*)hres;                  // [0] ndecl, [1] nev
  uint8_t* hdecl = hres + 256;
  uint8_t* hev = hdecl + rows_d;
  uint8_t* hout = hev + rows_e;
  const bool stream_rows = !nullc;                   // (a null cache parses without declaration rows)
  if (hipMemcpyAsync(hm + 16, dm + 16, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(c->h_status, c->d_status, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(hout, d_out, bound, hipMemcpyDeviceToHost, st) != hipSuccess)
    return XCG_EHIP;
  if (stream_rows && (hipMemcpyAsync(hcnt, c->bs.ndecl, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                      hipMemcpyAsync(hdecl, c->bs.decl, 16ull * maxd, hipMemcpyDeviceToHost, st) != hipSuccess))
    return XCG_EHIP;
  if (refs && (hipMemcpyAsync(hcnt + 1, c->bs.nev, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
               hipMemcpyAsync(hev, c->bs.ev, 16ull * c->bs.maxe, hipMemcpyDeviceToHost, st) != hipSuccess))
    return XCG_EHIP;
  if (hipStreamSynchronize(st) != hipSuccess) return XCG_EHIP;
  if (*c->h_status) return XCG_EOVERFLOW;
  const uint64_t olen = hmeta[2];
  if (olen > bound) return XCG_EHIP;
  memcpy(h_out, hout, olen);
  *h_out_len = olen;
  if (stream_rows) {
    *h_ndecl = unpack_decl_rows((const uint32_t*)hdecl, hcnt[0], decl_cap, h_decl_hash, h_decl_pos);
  }
  if (refs) {
    const uint32_t ne = hcnt[1];
    if (ne > c->bs.maxe) return XCG_EOVERFLOW;
    *h_nref = unpack_ref_rows((const uint32_t*)hev, ne, ref_cap, h_ref_hash, h_ref_kind, h_ref_idx);
  }
  return XCG_OK;
}

int xcg_encode_batch_grouped(xcg_ctx* c, const uint8_t* d_in, const uint64_t* d_chunk_off,
                             const uint32_t* d_chunk_len, uint32_t n, const uint32_t* d_group_first,
                             uint32_t n_groups, uint32_t max_group_len, uint8_t* d_out, const uint64_t* d_out_off,
                             uint64_t* d_out_len, uint32_t* d_stats, void* stream) {
  if (!c) return XCG_EINVAL;
  if (n == 0 || n_groups == 0) return XCG_OK;
  if (!d_in || !d_chunk_off || !d_chunk_len || !d_group_first || !d_out || !d_out_off || !d_out_len)
    return XCG_EINVAL;
  if (max_group_len > (1u << 19)) return XCG_EINVAL;
  // A fresh bounded cache per group evicts nothing while the group's
  // declarations fit the limit (at most max_group_len / 2048 of them).
  if (!ctx_fresh_cache_fits(c, group_declarations(max_group_len))) return XCG_ENOTSUP;
  DeviceGuard g(c->device);
  ctx_order(c, (hipStream_t)stream);
  c->last_stream_n = 0;              // (the last encode batch is no stream batch now)
  const int rc = xcg_launch_encode_group(d_in, d_chunk_off, d_chunk_len, n, d_group_first, n_groups, max_group_len,
                                         c->flags, d_out, d_out_off, d_out_len, d_stats, c->d_status,
                                         (hipStream_t)stream);
  ctx_mark(c, (hipStream_t)stream);
  return status_of(rc);   // (0, XCG_RC_INVAL or XCG_RC_HIP)
}

int xcg_pack_outputs(xcg_ctx* c, const uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_len,
                     uint32_t n, uint8_t* d_packed, uint64_t* d_packed_off, uint64_t* d_total, void* stream) {
  if (!c || (n && (!d_out || !d_out_off || !d_out_len || !d_packed || !d_packed_off || !d_total))) return XCG_EINVAL;
  DeviceGuard g(c->device);
  const int rc = xcg_launch_pack(d_out, d_out_off, d_out_len, n, d_packed, d_packed_off, d_total, (hipStream_t)stream);
  ctx_mark(c, (hipStream_t)stream);
  return rc == 0 ? XCG_OK : XCG_EHIP;
}

int xcg_gather_pieces(xcg_ctx* c, const uint8_t* d_src, const uint64_t* d_piece_src_off,
                      const uint64_t* d_piece_dst_off, const uint32_t* d_piece_len, uint32_t n_pieces,
                      uint32_t max_piece_len, uint8_t* d_dst, void* stream) {
  if (!c || (n_pieces && (!d_piece_src_off || !d_piece_dst_off || !d_piece_len || !d_dst))) return XCG_EINVAL;
  DeviceGuard g(c->device);
  return status_of(xcg_launch_gather_pieces(d_src, d_piece_src_off, d_piece_dst_off, d_piece_len, n_pieces,
                                            max_piece_len, d_dst, (hipStream_t)stream));
}

int xcg_window_hashes(xcg_ctx* c, const uint8_t* d_x, uint64_t len, uint64_t* d_hash, void* stream) {
  if (!c || (len && (!d_x || !d_hash))) return XCG_EINVAL;
  DeviceGuard g(c->device);
  return xcg_launch_window_hashes(d_x, len, d_hash, (hipStream_t)stream) == 0 ? XCG_OK : XCG_EHIP;
}

int xcg_segment_hashes(xcg_ctx* c, const uint8_t* d_x, uint64_t len, uint64_t* d_hash_be, void* stream) {
  if (!c || (len && (!d_x || !d_hash_be))) return XCG_EINVAL;
  DeviceGuard g(c->device);
  return xcg_launch_segment_hashes(d_x, len, d_hash_be, (hipStream_t)stream) == 0 ? XCG_OK : XCG_EHIP;
}

}  // extern "C"
