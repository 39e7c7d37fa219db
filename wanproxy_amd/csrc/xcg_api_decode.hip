// Decode entry points of the C ABI declared in include/xcgpu.h: batch,
// independent, grouped, host and call (with its zero-copy path), many calls on
// many caches in one launch, the BACKREF windows and the phase diagnostics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <mutex>
#include <vector>

#include "../../include/xcgpu.h"
#include "xcg_args.h"
#include "xcg_cache.h"
#include "xcg_ctx.h"
#include "xcg_decode_batch.h"          // WinView
#include "xcg_decode_windows_plan.h"

using xcg::align_up;

namespace {
// A decode batch's driver arguments from the context (its cache and scratch,
// allocated), the window `w` (null: the call brings its own windows) and the call.
XcgDecodeArgs decode_args(xcg_ctx* c, const xcg_window* w, const uint8_t* d_enc, const uint64_t* d_chunk_off,
                          const uint32_t* d_chunk_len, uint32_t n, uint32_t max_chunk_len, uint8_t* d_out,
                          uint64_t out_cap, uint64_t* d_out_off, uint64_t* d_out_len, int32_t* d_chunk_status,
                          uint64_t* d_consumed) {
  XcgDecodeArgs a{};
  static_cast<XcgDecodeScratch&>(a) = c->ds;         // every scratch array
  a.in = d_enc; a.chunk_off = d_chunk_off; a.chunk_len = d_chunk_len; a.n = n;
  a.out = d_out; a.out_cap = out_cap; a.out_off = d_out_off; a.out_len = d_out_len;
  a.chunk_status = d_chunk_status; a.consumed = d_consumed;
  a.status = c->d_status;
  a.g = c->g;
  a.x_mask = a.x_cap - 1;
  a.unknown_cap = UNKNOWN_CAP;
  if (w) { a.win_hash = w->hash; a.win_seg = w->seg; a.win_count = w->count; }
  a.lru = c->bounded ? &c->lru : nullptr;
  a.maxd = max_chunk_len / 2050 + 1;
  a.pair = c->pair;
  a.no_window = c->no_window ? 1 : 0;
  a.dup_cap = a.x_cap / 2;
  return a;
}

int decode_batch_impl(xcg_ctx* c, const uint8_t* d_enc, const uint64_t* d_chunk_off, const uint32_t* d_chunk_len,
                      uint32_t n, uint32_t max_chunk_len, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
                      uint64_t* d_out_len, int32_t* d_chunk_status, uint64_t* d_consumed, uint64_t* h_unknown,
                      uint32_t unknown_cap, uint32_t* h_nunknown, uint64_t* h_total_out, void* stream) {
  if (!c || (n && (!d_enc || !d_chunk_off || !d_chunk_len || !d_out_off || !d_out_len || !d_chunk_status ||
                   !d_consumed)))
    return XCG_EINVAL;
  if (h_nunknown) *h_nunknown = 0;
  if (h_total_out) *h_total_out = 0;
  if (n == 0) return XCG_OK;
  // a bounded or pair batch numbers its ops by (chunk << 21 | offset)
  if ((c->bounded || c->pair) && max_chunk_len >= (1u << 21)) return XCG_EINVAL;
  DeviceGuard g(c->device);
  ctx_order(c, (hipStream_t)stream);
  int rc = ensure_cache(c);
  if (rc == XCG_OK) rc = ensure_dscratch(c, (uint64_t)n * (max_chunk_len / 2050 + 1));
  if (rc == XCG_OK) rc = ensure_dchunks(c, n);
  if (rc == XCG_OK && !c->cur_win) {
    rc = window_alloc(c->device, &c->own_win);
    c->cur_win = c->own_win;
  }
  if (rc != XCG_OK) return rc;
  xcg_window* w = c->cur_win;
  const XcgDecodeArgs a = decode_args(c, w, d_enc, d_chunk_off, d_chunk_len, n, max_chunk_len, d_out, out_cap,
                                      d_out_off, d_out_len, d_chunk_status, d_consumed);
  if (c->pair) {
    PairGpu G{};
    G.in = d_enc; G.chunk_off = d_chunk_off;
    G.g = c->g;
    G.status = c->d_status;
    if (xcg_pair_sync(c->pair, &G, (hipStream_t)stream)) return XCG_EHIP;
  }
  uint64_t total = 0, blockp = 0, berr = 0;
  uint32_t nunk = 0;
  const int lrc = xcg_launch_decode(&a, &total, &blockp, &berr, &nunk, (hipStream_t)stream);
  if (h_total_out) *h_total_out = total;
  if (lrc != 0) return status_of(lrc);   // (XCG_RC_HIP, _OVERFLOW or _NOTSUP)
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return XCG_EHIP;
  // status word and the declare count, by async copies into pinned memory
  // (a synchronous 4-byte hipMemcpy costs milliseconds here)
  if (hipMemcpyAsync(c->h_status, c->d_status, 4, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
      hipMemcpyAsync(&c->ds.h_scratch->t_end, &c->ds.scratch->t_end, 8, hipMemcpyDeviceToHost,
                     (hipStream_t)stream) != hipSuccess ||
      hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return XCG_EHIP;
  const int32_t st = *c->h_status;
  const uint64_t t_end = c->ds.h_scratch->t_end;
  if (!c->no_window) w->count += t_end;               // declares made: the window cursor advances
  if (st & (1 << 9)) {
    (void)hipMemsetAsync(c->d_status, 0, 4, (hipStream_t)stream);
    return XCG_ENOTSUP;
  }
  if (nunk > UNKNOWN_CAP) return XCG_EOVERFLOW;     // more distinct unknown hashes than the set holds
  if (nunk && blockp < berr) {
    // XCodecDecoder::decode_skim (xcodec/xcodec_decoder.cc:196-272): every REF
    // from the blocking point on that cannot resolve, as a sorted set.  The
    // batch's frames are one buffered stream (a pipe pair appends each FRAME
    // to the decoder's input, xcodec/xcodec_pipe_pair.cc:425-483), so the skim
    // runs to the end of the batch.  (A BACKREF error first: decode() is false,
    // no ASK.)
    const uint32_t m = nunk < UNKNOWN_CAP ? nunk : UNKNOWN_CAP;
    std::vector<uint64_t> hs(m);
    if (hipMemcpyAsync(hs.data(), c->ds.unknown, 8ull * m, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
      return XCG_EHIP;
    std::sort(hs.begin(), hs.end());
    hs.erase(std::unique(hs.begin(), hs.end()), hs.end());
    const uint32_t k = (uint32_t)hs.size() < unknown_cap ? (uint32_t)hs.size() : unknown_cap;
    if (h_unknown) memcpy(h_unknown, hs.data(), 8ull * k);
    if (h_nunknown) *h_nunknown = k;
  }
  return XCG_OK;
}

// xcg_decode_batch_windows (`classified` false: an unbounded context) or
// xcg_decode_batch_windows_bounded (true: a bounded or pair context) without
// the context's completion mark.
int decode_windows_impl(bool classified, xcg_ctx* c, const uint8_t* d_enc, const uint64_t* d_chunk_off,
                        const uint32_t* d_chunk_len, uint32_t n, uint32_t max_chunk_len,
                        xcg_window* const* windows, uint32_t n_windows,
                        const uint32_t* h_chunk_window, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
                        uint64_t* d_out_len, int32_t* d_chunk_status, uint64_t* d_consumed, uint32_t* h_stop_chunk,
                        uint64_t* h_total_out, hipStream_t stream) {
  if (!c || (n && (!d_enc || !d_chunk_off || !d_chunk_len || !d_out_off || !d_out_len || !d_chunk_status ||
                   !d_consumed || !windows || !h_chunk_window)))
    return XCG_EINVAL;
  if (h_stop_chunk) *h_stop_chunk = n;
  if (h_total_out) *h_total_out = 0;
  if (n == 0) return XCG_OK;
  if (xcg::dec_windows_distinct((const void* const*)windows, n_windows) != xcg::DEC_PLAN_OK) return XCG_EINVAL;
  for (uint32_t w = 0; w < n_windows; ++w)
    if (windows[w]->device != c->device) return XCG_EINVAL;
  for (uint32_t i = 0; i < n; ++i)
    if (h_chunk_window[i] >= n_windows) return XCG_EINVAL;
  // a bounded or pair batch numbers its ops by (chunk << 21 | offset)
  if (classified && max_chunk_len >= (1u << 21)) return XCG_EINVAL;
  // (each kind of context has its own call: the bounded one may refuse a whole batch, this one never does)
  if (classified != (c->bounded || c->pair != nullptr)) return XCG_ENOTSUP;
  // the plan, in the pinned block: views | chunk -> window | order | first
  const size_t nw = n_windows;
  const size_t o_cw = sizeof(xcg::WinView) * nw, o_ord = o_cw + 4ull * n, o_first = o_ord + 4ull * n,
               up = align_up(o_first + 4 * (nw + 1), 256);
  // device only, behind it: t_end words | scan scratch | tail records
  const size_t o_tend = up, o_scan = align_up(o_tend + 8 * nw, 256), o_tail = align_up(o_scan + 16ull * n, 256),
               dbytes = o_tail + 16ull * 256 * nw;
  DeviceGuard g(c->device);
  ctx_order(c, stream);
  int rc = ensure_cache(c);
  if (rc == XCG_OK) rc = ensure_dscratch(c, (uint64_t)n * (max_chunk_len / 2050 + 1));
  if (rc == XCG_OK) rc = ensure_dchunks(c, n);
  if (rc != XCG_OK) return rc;
  const size_t hbytes = up + 8 * nw;
  if (!c->mem_call.grow_bytes(&c->win_h, &c->win_h_cap, hbytes, xcg::MEM_PINNED) ||
      !c->mem_call.grow_bytes(&c->win_d, &c->win_d_cap, dbytes, xcg::MEM_DEV))
    return XCG_ENOMEM;
  uint8_t* hm = c->win_h;
  uint8_t* dm = c->win_d;
  xcg::WinView* hv = (xcg::WinView*)hm;
  for (uint32_t w = 0; w < n_windows; ++w) {
    hv[w] = xcg::WinView{};
    hv[w].hash = windows[w]->hash;
    hv[w].seg = windows[w]->seg;
    hv[w].count = windows[w]->count;
  }
  memcpy(hm + o_cw, h_chunk_window, 4ull * n);
  if (xcg::dec_windows_plan(h_chunk_window, n, n_windows, (uint32_t*)(hm + o_ord), (uint32_t*)(hm + o_first)) !=
      xcg::DEC_PLAN_OK)
    return XCG_EINVAL;
  XcgDecodeWindows W{};
  W.n_windows = n_windows;
  W.views = dm;
  W.chunk_win = (const uint32_t*)(dm + o_cw);
  W.order = (const uint32_t*)(dm + o_ord);
  W.first = (const uint32_t*)(dm + o_first);
  W.w_tend = (uint64_t*)(dm + o_tend);
  W.scan_tmp = (uint64_t*)(dm + o_scan);
  W.tail = (uint4*)(dm + o_tail);
  if (hipMemcpyAsync(dm, hm, up, hipMemcpyHostToDevice, stream) != hipSuccess) return XCG_EHIP;
  XcgDecodeArgs a = decode_args(c, nullptr, d_enc, d_chunk_off, d_chunk_len, n, max_chunk_len, d_out, out_cap,
                                d_out_off, d_out_len, d_chunk_status, d_consumed);
  a.no_window = 0;
  a.wins = &W;
  if (c->pair) {
    PairGpu G{};
    G.in = d_enc; G.chunk_off = d_chunk_off;
    G.g = c->g;
    G.status = c->d_status;
    if (xcg_pair_sync(c->pair, &G, stream)) return XCG_EHIP;
  }
  uint64_t total = 0, blockp = 0, berr = 0;
  uint32_t nunk = 0;                                 // (how many hashes are unknown does not matter here)
  const int lrc = xcg_launch_decode(&a, &total, &blockp, &berr, &nunk, stream);
  if (h_total_out) *h_total_out = total;
  if (lrc != 0) return status_of(lrc);               // (XCG_RC_HIP, _OVERFLOW or _NOTSUP: nothing was written)
  uint64_t* h_tend = (uint64_t*)(hm + up);
  if (classified) *c->h_status = 0;
  if (hipMemcpyAsync(h_tend, W.w_tend, 8 * nw, hipMemcpyDeviceToHost, stream) != hipSuccess ||
      (classified && hipMemcpyAsync(c->h_status, c->d_status, 4, hipMemcpyDeviceToHost, stream) != hipSuccess) ||
      hipStreamSynchronize(stream) != hipSuccess)
    return XCG_EHIP;
  for (uint32_t w = 0; w < n_windows; ++w) windows[w]->count += h_tend[w];   // each decoder's cursor advances
  // Bit 9 this late would be dec_replace_kernel's: two EXTRACTs of one hash with
  // different bytes.  dec_dup_kernel refuses those before anything is written,
  // so it cannot be set here; if it is, the batch is committed and the call must
  // not report the refusal that changes nothing.
  if (classified && (*c->h_status & (1 << 9))) {
    (void)hipMemsetAsync(c->d_status, 0, 4, stream);
    return XCG_EHIP;
  }
  const uint64_t stop = blockp < berr ? blockp : berr;
  if (h_stop_chunk) *h_stop_chunk = stop == ~0ull ? n : (uint32_t)(stop >> 32);
  return XCG_OK;
}
}  // namespace

extern "C" {

int xcg_decode_batch(xcg_ctx* c, const uint8_t* d_enc, const uint64_t* d_chunk_off, const uint32_t* d_chunk_len,
                     uint32_t n, uint32_t max_chunk_len, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
                     uint64_t* d_out_len, int32_t* d_chunk_status, uint64_t* d_consumed, uint64_t* h_unknown,
                     uint32_t unknown_cap, uint32_t* h_nunknown, uint64_t* h_total_out, void* stream) {
  const int rc = decode_batch_impl(c, d_enc, d_chunk_off, d_chunk_len, n, max_chunk_len, d_out, out_cap, d_out_off,
                                   d_out_len, d_chunk_status, d_consumed, h_unknown, unknown_cap, h_nunknown,
                                   h_total_out, stream);
  if (c) {
    DeviceGuard g(c->device);
    ctx_mark(c, (hipStream_t)stream);
  }
  return rc;
}

int xcg_decode_batch_windows(xcg_ctx* c, const uint8_t* d_enc, const uint64_t* d_chunk_off,
                             const uint32_t* d_chunk_len, uint32_t n, uint32_t max_chunk_len,
                             xcg_window* const* windows, uint32_t n_windows, const uint32_t* h_chunk_window,
                             uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off, uint64_t* d_out_len,
                             int32_t* d_chunk_status, uint64_t* d_consumed, uint32_t* h_stop_chunk,
                             uint64_t* h_total_out, void* stream) {
  const int rc = decode_windows_impl(false, c, d_enc, d_chunk_off, d_chunk_len, n, max_chunk_len, windows, n_windows,
                                     h_chunk_window, d_out, out_cap, d_out_off, d_out_len, d_chunk_status,
                                     d_consumed, h_stop_chunk, h_total_out, (hipStream_t)stream);
  if (c) {
    DeviceGuard g(c->device);
    ctx_mark(c, (hipStream_t)stream);
  }
  return rc;
}

int xcg_decode_batch_windows_bounded(xcg_ctx* c, const uint8_t* d_enc, const uint64_t* d_chunk_off,
                                     const uint32_t* d_chunk_len, uint32_t n, uint32_t max_chunk_len,
                             xcg_window* const* windows, uint32_t n_windows, const uint32_t* h_chunk_window,
                             uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off, uint64_t* d_out_len,
                             int32_t* d_chunk_status, uint64_t* d_consumed, uint32_t* h_stop_chunk,
                             uint64_t* h_total_out, void* stream) {
  const int rc = decode_windows_impl(true, c, d_enc, d_chunk_off, d_chunk_len, n, max_chunk_len, windows, n_windows,
                                     h_chunk_window, d_out, out_cap, d_out_off, d_out_len, d_chunk_status,
                                     d_consumed, h_stop_chunk, h_total_out, (hipStream_t)stream);
  if (c) {
    DeviceGuard g(c->device);
    ctx_mark(c, (hipStream_t)stream);
  }
  return rc;
}

}  // extern "C"

namespace {
// xcg_decode_host_windows / _bounded: staging around the device call.
int decode_host_windows_impl(bool classified, xcg_ctx* c, const uint8_t* h_enc, uint64_t enc_len,
                             const uint64_t* h_chunk_off, const uint32_t* h_chunk_len, uint32_t n,
                             xcg_window* const* windows, uint32_t n_windows,
                            const uint32_t* h_chunk_window, uint8_t* h_out, uint64_t out_cap, uint64_t* h_out_off,
                            uint64_t* h_out_len, int32_t* h_chunk_status, uint64_t* h_consumed,
                            uint32_t* h_stop_chunk, uint64_t* h_total_out) {
  if (!c || (n && (!h_enc || !h_chunk_off || !h_chunk_len || !h_out_off || !h_out_len || !h_chunk_status ||
                   !h_consumed || !windows || !h_chunk_window || (out_cap && !h_out))))
    return XCG_EINVAL;
  if (h_stop_chunk) *h_stop_chunk = n;
  if (h_total_out) *h_total_out = 0;
  if (n == 0) return XCG_OK;
  uint32_t maxlen = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (h_chunk_off[i] + h_chunk_len[i] > enc_len) return XCG_EINVAL;
    if (h_chunk_len[i] > maxlen) maxlen = h_chunk_len[i];
  }
  DeviceGuard g(c->device);
  // staging as xcg_decode_host's: [off n][oo n][ol n][cons n][len n][status n] | input | output
  const size_t meta = align_up(40ull * n, 256), inb = align_up(enc_len ? enc_len : 1, 256),
               outb = align_up(out_cap ? out_cap : 1, 256);
  int rc = ensure_stage(c, meta + inb + outb, meta + inb + outb);
  if (rc != XCG_OK) return rc;
  uint8_t* hm = c->stage_h;
  uint8_t* dm = c->stage_d;
  memcpy(hm, h_chunk_off, 8ull * n);
  memcpy(hm + 32ull * n, h_chunk_len, 4ull * n);
  memcpy(hm + meta, h_enc, enc_len);
  const hipStream_t st = c->call_st;
  uint64_t* d_oo = (uint64_t*)(dm + 8ull * n);
  uint64_t* d_ol = (uint64_t*)(dm + 16ull * n);
  uint64_t* d_cons = (uint64_t*)(dm + 24ull * n);
  int32_t* d_st = (int32_t*)(dm + 36ull * n);
  uint8_t* d_out = dm + meta + inb;
  if (hipMemcpyAsync(dm, hm, meta + enc_len, hipMemcpyHostToDevice, st) != hipSuccess) return XCG_EHIP;
  uint64_t total = 0;
  const auto call = classified ? xcg_decode_batch_windows_bounded : xcg_decode_batch_windows;
  rc = call(c, dm + meta, (const uint64_t*)dm, (const uint32_t*)(dm + 32ull * n), n, maxlen, windows, n_windows,
            h_chunk_window, d_out, out_cap, d_oo, d_ol, d_st, d_cons, h_stop_chunk, &total, st);
  if (h_total_out) *h_total_out = total;
  if (rc != XCG_OK) return rc;
  uint8_t* ho = hm + meta + inb;
  const uint64_t nout = total < out_cap ? total : out_cap;
  if (hipMemcpyAsync(hm + 8ull * n, dm + 8ull * n, 24ull * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(hm + 36ull * n, d_st, 4ull * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
      (nout && hipMemcpyAsync(ho, d_out, nout, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      hipStreamSynchronize(st) != hipSuccess)
    return XCG_EHIP;
  memcpy(h_out_off, hm + 8ull * n, 8ull * n);
  memcpy(h_out_len, hm + 16ull * n, 8ull * n);
  memcpy(h_consumed, hm + 24ull * n, 8ull * n);
  memcpy(h_chunk_status, hm + 36ull * n, 4ull * n);
  if (nout) memcpy(h_out, ho, nout);
  return XCG_OK;
}
}  // namespace

extern "C" {

int xcg_decode_host_windows(xcg_ctx* c, const uint8_t* h_enc, uint64_t enc_len, const uint64_t* h_chunk_off,
                            const uint32_t* h_chunk_len, uint32_t n, xcg_window* const* windows, uint32_t n_windows,
                            const uint32_t* h_chunk_window, uint8_t* h_out, uint64_t out_cap, uint64_t* h_out_off,
                            uint64_t* h_out_len, int32_t* h_chunk_status, uint64_t* h_consumed,
                            uint32_t* h_stop_chunk, uint64_t* h_total_out) {
  return decode_host_windows_impl(false, c, h_enc, enc_len, h_chunk_off, h_chunk_len, n, windows, n_windows,
                                  h_chunk_window, h_out, out_cap, h_out_off, h_out_len, h_chunk_status, h_consumed,
                                  h_stop_chunk, h_total_out);
}

int xcg_decode_host_windows_bounded(xcg_ctx* c, const uint8_t* h_enc, uint64_t enc_len,
                                    const uint64_t* h_chunk_off, const uint32_t* h_chunk_len, uint32_t n,
                                    xcg_window* const* windows, uint32_t n_windows, const uint32_t* h_chunk_window,
                                    uint8_t* h_out, uint64_t out_cap, uint64_t* h_out_off, uint64_t* h_out_len,
                                    int32_t* h_chunk_status, uint64_t* h_consumed, uint32_t* h_stop_chunk,
                                    uint64_t* h_total_out) {
  return decode_host_windows_impl(true, c, h_enc, enc_len, h_chunk_off, h_chunk_len, n, windows, n_windows,
                                  h_chunk_window, h_out, out_cap, h_out_off, h_out_len, h_chunk_status, h_consumed,
                                  h_stop_chunk, h_total_out);
}

int xcg_decode_batch_independent(xcg_ctx* c, const uint8_t* d_enc, const uint64_t* d_chunk_off,
                                 const uint32_t* d_chunk_len, uint32_t n, uint32_t max_chunk_len, uint8_t* d_out,
                                 const uint64_t* d_out_off, const uint64_t* d_out_cap, uint64_t* d_out_len,
                                 int32_t* d_chunk_status, uint64_t* d_consumed, uint64_t* d_first_unknown,
                                 void* stream) {
  if (!c) return XCG_EINVAL;
  if (n == 0) return XCG_OK;
  if (!d_enc || !d_chunk_off || !d_chunk_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_chunk_status ||
      !d_consumed)
    return XCG_EINVAL;
  if (max_chunk_len > xcg_encode_bound(1u << 19)) return XCG_EINVAL;
  // A fresh bounded cache per chunk evicts nothing while the chunk's EXTRACTs
  // fit the limit (at most max_chunk_len / 2050 of them); lookups enter nothing.
  if (!ctx_fresh_cache_fits(c, encoded_extracts(max_chunk_len))) return XCG_ENOTSUP;
  DeviceGuard g(c->device);
  ctx_order(c, (hipStream_t)stream);
  XcgIndepDecodeArgs a{};
  a.in = d_enc; a.chunk_off = d_chunk_off; a.chunk_len = d_chunk_len; a.n = n; a.max_len = max_chunk_len;
  a.out = d_out; a.out_off = d_out_off; a.out_cap = d_out_cap; a.out_len = d_out_len;
  a.chunk_status = d_chunk_status; a.consumed = d_consumed; a.first_unknown = d_first_unknown;
  a.status = c->d_status;
  const int rc = xcg_launch_decode_independent(&a, (hipStream_t)stream);
  ctx_mark(c, (hipStream_t)stream);
  return status_of(rc);   // (0, XCG_RC_INVAL or XCG_RC_HIP)
}

int xcg_decode_batch_grouped(xcg_ctx* c, const uint8_t* d_enc, const uint64_t* d_chunk_off,
                             const uint32_t* d_chunk_len, uint32_t n, const uint32_t* d_group_first,
                             uint32_t n_groups, uint32_t max_group_len, uint8_t* d_out, const uint64_t* d_out_off,
                             const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_chunk_status,
                             uint64_t* d_consumed, uint64_t* d_first_unknown, void* stream) {
  if (!c) return XCG_EINVAL;
  if (n == 0 || n_groups == 0) return XCG_OK;
  if (!d_enc || !d_chunk_off || !d_chunk_len || !d_group_first || !d_out || !d_out_off || !d_out_cap || !d_out_len ||
      !d_chunk_status || !d_consumed)
    return XCG_EINVAL;
  if (max_group_len > xcg_encode_bound(1u << 19)) return XCG_EINVAL;
  // (the independent call's rule: at most max_group_len / 2050 EXTRACTs enter a group's cache)
  if (!ctx_fresh_cache_fits(c, encoded_extracts(max_group_len))) return XCG_ENOTSUP;
  DeviceGuard g(c->device);
  ctx_order(c, (hipStream_t)stream);
  XcgGroupDecodeArgs a{};
  a.in = d_enc; a.chunk_off = d_chunk_off; a.chunk_len = d_chunk_len; a.n = n;
  a.group_first = d_group_first; a.n_groups = n_groups; a.max_len = max_group_len;
  a.out = d_out; a.out_off = d_out_off; a.out_cap = d_out_cap; a.out_len = d_out_len;
  a.chunk_status = d_chunk_status; a.consumed = d_consumed; a.first_unknown = d_first_unknown;
  a.status = c->d_status;
  const int rc = xcg_launch_decode_group(&a, (hipStream_t)stream);
  ctx_mark(c, (hipStream_t)stream);
  return status_of(rc);   // (0, XCG_RC_INVAL or XCG_RC_HIP)
}

int xcg_debug_decode_reuse(xcg_ctx* c, uint64_t out[3]) {
  if (!c || !out) return XCG_EINVAL;
  const xcg::DecHostWords* h = c->ds.h_scratch;
  for (int k = 0; k < 3; ++k) out[k] = h ? h->reuse[k] : 0;
  return XCG_OK;
}

int xcg_window_create(xcg_ctx* c, xcg_window** out) {
  if (!c || !out) return XCG_EINVAL;
  DeviceGuard g(c->device);
  return window_alloc(c->device, out);
}

void xcg_window_destroy(xcg_window* w) {
  if (!w) return;
  DeviceGuard g(w->device);
  window_free(w);
}

int xcg_decode_set_window(xcg_ctx* c, xcg_window* w) {
  if (!c) return XCG_EINVAL;
  c->cur_win = w ? w : c->own_win;
  return XCG_OK;
}

int xcg_decode_host(xcg_ctx* c, const uint8_t* h_enc, uint64_t enc_len, const uint64_t* h_chunk_off,
                    const uint32_t* h_chunk_len, uint32_t n, uint8_t* h_out, uint64_t out_cap, uint64_t* h_out_off,
                    uint64_t* h_out_len, int32_t* h_chunk_status, uint64_t* h_consumed, uint64_t* h_unknown,
                    uint32_t unknown_cap, uint32_t* h_nunknown) {
  if (!c || (n && (!h_enc || !h_chunk_off || !h_chunk_len || !h_out_off || !h_out_len || !h_chunk_status ||
                   !h_consumed)))
    return XCG_EINVAL;
  if (n == 0) return XCG_OK;
  uint32_t maxlen = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (h_chunk_off[i] + h_chunk_len[i] > enc_len) return XCG_EINVAL;
    if (h_chunk_len[i] > maxlen) maxlen = h_chunk_len[i];
  }
  DeviceGuard g(c->device);
  // staging (kept by the context): [off n][oo n][ol n][cons n][len n][status n] | input | output
  const size_t meta = align_up(40ull * n, 256), inb = align_up(enc_len ? enc_len : 1, 256),
               outb = align_up(out_cap ? out_cap : 1, 256);
  int rc = ensure_stage(c, meta + inb + outb, meta + inb + outb);
  if (rc != XCG_OK) return rc;
  uint8_t* hm = c->stage_h;
  uint8_t* dm = c->stage_d;
  memcpy(hm, h_chunk_off, 8ull * n);
  memcpy(hm + 32ull * n, h_chunk_len, 4ull * n);
  memcpy(hm + meta, h_enc, enc_len);
  const hipStream_t st = c->call_st;
  uint64_t* d_oo = (uint64_t*)(dm + 8ull * n);
  uint64_t* d_ol = (uint64_t*)(dm + 16ull * n);
  uint64_t* d_cons = (uint64_t*)(dm + 24ull * n);
  int32_t* d_st = (int32_t*)(dm + 36ull * n);
  uint8_t* d_out = dm + meta + inb;
  if (hipMemcpyAsync(dm, hm, meta + enc_len, hipMemcpyHostToDevice, st) != hipSuccess) return XCG_EHIP;
  uint64_t total = 0;
  rc = xcg_decode_batch(c, dm + meta, (const uint64_t*)dm, (const uint32_t*)(dm + 32ull * n), n, maxlen, d_out,
                        out_cap, d_oo, d_ol, d_st, d_cons, h_unknown, unknown_cap, h_nunknown, &total, st);
  if (rc != XCG_OK) return rc;
  uint8_t* ho = hm + meta + inb;
  const uint64_t nout = total < out_cap ? total : out_cap;
  if (hipMemcpyAsync(hm + 8ull * n, dm + 8ull * n, 24ull * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(hm + 36ull * n, d_st, 4ull * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
      (nout && hipMemcpyAsync(ho, d_out, nout, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      hipStreamSynchronize(st) != hipSuccess)
    return XCG_EHIP;
  memcpy(h_out_off, hm + 8ull * n, 8ull * n);
  memcpy(h_out_len, hm + 16ull * n, 8ull * n);
  memcpy(h_consumed, hm + 24ull * n, 8ull * n);
  memcpy(h_chunk_status, hm + 36ull * n, 4ull * n);
  if (nout) memcpy(h_out, ho, nout);
  return XCG_OK;
}

}  // extern "C"

// Diagnostics: with XCG_DECODE_PHASES set, every one-launch decode() records
// clock stamps at its phase boundaries (decode_small_kernel); the sums of the
// phase durations and the call count come back through
// xcg_debug_decode_phases.  (Costs a synchronous copy per call.)
namespace {
std::mutex g_dph_mu;
std::vector<double> g_dph_sum;
uint32_t g_dph_calls = 0;
bool dphase_on() {
  static const bool on = getenv("XCG_DECODE_PHASES") != nullptr;
  return on;
}
}  // namespace

namespace {
bool getenv_flag_no_zc() {
  static const bool off = getenv("XCG_NO_ZEROCOPY") != nullptr;
  return off;
}

// The calls xcg_decode_call and xcg_decode_call_many decode in one launch
// (decode_small_body): an unbounded cache that is not the null cache, and an
// input the kernel's op scratch is sized for.
bool decode_call_fast(const xcg_ctx* c, uint32_t len) {
  return !c->bounded && !c->pair && !(c->flags & XCG_FLAG_NULLCACHE) && len <= (1u << 20);
}

// Every other call, and a call the kernel declined: one chunk through the
// batch decoder on the context's current window.
int decode_call_batch(xcg_ctx* c, const uint8_t* h_in, uint32_t len, uint8_t* h_out, uint64_t out_cap,
                      uint64_t* h_out_len, uint64_t* h_consumed, int32_t* h_status, uint64_t* h_unknown,
                      uint32_t unknown_cap, uint32_t* h_nunknown) {
  const uint64_t off = 0;
  uint64_t ooff = 0;
  return xcg_decode_host(c, h_in, len, &off, &len, 1, h_out, out_cap, &ooff, h_out_len, h_status, h_consumed,
                         h_unknown, unknown_cap, h_nunknown);
}

// One decode() in one launch with no copies: the kernel reads the input from,
// and writes the output and results to, coherent pinned host memory, then
// stores the call's sequence number there; the host waits on that word (a
// launch + poll is ~11 us on this box against ~29 us for copy in, launch, copy
// out and a stream synchronisation).  Input up to the kernel's LDS staging size.
int decode_call_zc(xcg_ctx* c, const uint8_t* h_in, uint32_t len, uint8_t* h_out, uint64_t out_cap, uint32_t ops_cap,
                   uint64_t* h_out_len, uint64_t* h_consumed, int32_t* h_status, uint64_t* h_unknown,
                   uint32_t unknown_cap, uint32_t* h_nunknown, uint64_t* h_extract_hash, uint32_t extract_cap,
                   uint32_t* h_nextract) {
  const size_t inb = align_up(len, 256), outb = align_up(out_cap ? out_cap : 1, 256), resb = align_up(8ull * xcg::SD_RES_WORDS, 256);
  const size_t need = 256 + inb + outb + resb;
  if (need > c->zc_cap) {
    if (c->zc_h) (void)hipStreamSynchronize(c->call_st);
    c->mem_call.release(c->zc_h);
    c->zc_h = nullptr;
    c->zc_cap = 0;
    const size_t want = need + need / 2;
    if (!c->mem_call.pinned(&c->zc_h, want, true)) return XCG_ENOMEM;
    c->zc_cap = want;
    memset(c->zc_h, 0, 256);
  }
  const size_t scr = align_up(xcg::SD_SCRATCH_PER_OP * ops_cap, 256);
  int rc = ensure_stage(c, scr, 0);                  // (device scratch: the op lists)
  if (rc != XCG_OK) return rc;
  uint8_t* hz = c->zc_h;
  void* dz = nullptr;
  if (hipHostGetDevicePointer(&dz, hz, 0) != hipSuccess) return XCG_EHIP;
  uint8_t* dzb = (uint8_t*)dz;
  volatile uint32_t* flag = (volatile uint32_t*)hz;
  uint8_t* h_o = hz + 256 + inb;
  const uint64_t* h_res = (const uint64_t*)(hz + 256 + inb + outb);
  memcpy(hz + 256, h_in, len);
  const uint32_t seq = ++c->zc_seq ? c->zc_seq : ++c->zc_seq;   // (never 0: the word's initial value)
  const hipStream_t st = c->call_st;
  ctx_order(c, st);
  xcg_window* w = c->cur_win;
  if (xcg_launch_decode_small(dzb + 256, len, &c->g, c->d_status, c->stage_d, ops_cap, dzb + 256 + inb, out_cap,
                              w->hash, w->seg, w->count, (uint64_t*)(dzb + 256 + inb + outb), nullptr, (uint32_t*)dzb,
                              seq, st) != 0)
    return XCG_EHIP;
  ctx_mark(c, st);
  // Spin (with a pause per poll, so a sibling hyperthread keeps its share) for
  // about the kernel's expected time; past ZC_SPIN_NS block in the runtime
  // instead, which sleeps -- so a slow or stuck kernel costs the caller's
  // event-loop thread no more than that much busy time.
  constexpr int64_t ZC_SPIN_NS = 2000000;
  const auto t_spin = std::chrono::steady_clock::now();
  for (uint64_t n = 1;; ++n) {
    if (__atomic_load_n((const uint32_t*)flag, __ATOMIC_ACQUIRE) == seq) break;
    __builtin_ia32_pause();
    if ((n & 1023) == 0) {
      const hipError_t e = hipStreamQuery(st);
      if (e == hipSuccess) {
        if (__atomic_load_n((const uint32_t*)flag, __ATOMIC_ACQUIRE) == seq) break;
        return XCG_EHIP;                             // (finished without storing the word)
      }
      if (e != hipErrorNotReady) return XCG_EHIP;
      if (std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_spin).count() >
          ZC_SPIN_NS) {
        if (hipStreamSynchronize(st) != hipSuccess) return XCG_EHIP;
        if (__atomic_load_n((const uint32_t*)flag, __ATOMIC_ACQUIRE) != seq) return XCG_EHIP;
        break;
      }
    }
  }
  return decode_call_results(&w->count, h_res, h_o, h_out, h_out_len, h_consumed, h_status, h_unknown, unknown_cap,
                             h_nunknown, h_extract_hash, extract_cap, h_nextract);
}
}  // namespace

extern "C" {

int xcg_decode_call(xcg_ctx* c, const uint8_t* h_in, uint32_t len, uint8_t* h_out, uint64_t out_cap,
                    uint64_t* h_out_len, uint64_t* h_consumed, int32_t* h_status, uint64_t* h_unknown,
                    uint32_t unknown_cap, uint32_t* h_nunknown, uint64_t* h_extract_hash, uint32_t extract_cap,
                    uint32_t* h_nextract) {
  if (!c || !h_out_len || !h_consumed || !h_status || !h_nunknown || !h_nextract || (len && !h_in) ||
      (out_cap && !h_out))
    return XCG_EINVAL;
  *h_out_len = *h_consumed = 0;
  *h_status = 0;
  *h_nunknown = 0;
  *h_nextract = XCG_NO_REFERENCES;
  if (len == 0) return XCG_OK;
  DeviceGuard g(c->device);
  const bool fast = decode_call_fast(c, len);
  if (fast) {
    int rc = ensure_cache(c);
    if (rc == XCG_OK && !c->cur_win) {
      rc = window_alloc(c->device, &c->own_win);
      c->cur_win = c->own_win;
    }
    if (rc != XCG_OK) return rc;
    const uint32_t ops_cap = len / 4 + 64;
    if (len <= xcg::SD_LDS_IN && !dphase_on() && !getenv_flag_no_zc()) {
      rc = decode_call_zc(c, h_in, len, h_out, out_cap, ops_cap, h_out_len, h_consumed, h_status, h_unknown,
                          unknown_cap, h_nunknown, h_extract_hash, extract_cap, h_nextract);
      if (rc != XCG_ENOTSUP) return rc;
      // (fallback: the batch decoder takes it; nothing was written)
      return decode_call_batch(c, h_in, len, h_out, out_cap, h_out_len, h_consumed, h_status, h_unknown, unknown_cap,
                               h_nunknown);
    }
    // device: input | output | results | op lists;  host: input | output | results (one D2H brings
    // both back; the results' last word is the context's sticky word)
    const size_t inb = align_up(len, 256), outb = align_up(out_cap ? out_cap : 1, 256), resb = align_up(8ull * xcg::SD_RES_WORDS, 256);
    const size_t scr = align_up(xcg::SD_SCRATCH_PER_OP * ops_cap, 256);
    const uint32_t nph = xcg::SD_PHASES;
    const size_t timb = dphase_on() ? align_up(8ull * nph, 256) : 0;
    rc = ensure_stage(c, inb + outb + resb + scr + timb, inb + outb + resb);
    if (rc != XCG_OK) return rc;
    uint8_t* dm = c->stage_d;
    uint8_t* hm = c->stage_h;
    uint64_t* d_res = (uint64_t*)(dm + inb + outb);
    uint64_t* h_res = (uint64_t*)(hm + inb + outb);
    uint8_t* h_o = hm + inb;
    const hipStream_t st = c->call_st;
    memcpy(hm, h_in, len);
    ctx_order(c, st);
    xcg_window* w = c->cur_win;
    if (hipMemcpyAsync(dm, hm, len, hipMemcpyHostToDevice, st) != hipSuccess ||
        xcg_launch_decode_small(dm, len, &c->g, c->d_status, dm + inb + outb + resb, ops_cap, dm + inb, out_cap,
                                w->hash, w->seg, w->count, d_res,
                                timb ? (uint64_t*)(dm + inb + outb + resb + scr) : nullptr, nullptr, 0u, st) != 0 ||
        hipMemcpyAsync(h_o, dm + inb, outb + 8ull * xcg::SD_RES_WORDS, hipMemcpyDeviceToHost, st) != hipSuccess)
      return XCG_EHIP;
    ctx_mark(c, st);
    if (hipStreamSynchronize(st) != hipSuccess) return XCG_EHIP;
    if (timb) {
      std::vector<uint64_t> tm(nph, 0);
      if (hipMemcpy(tm.data(), dm + inb + outb + resb + scr, 8ull * nph, hipMemcpyDeviceToHost) == hipSuccess &&
          h_res[xcg::SDR_FALLBACK] == xcg::SD_FB_DONE) {
        std::lock_guard<std::mutex> g(g_dph_mu);
        g_dph_sum.resize(nph, 0.0);
        for (uint32_t k = 1; k < nph; ++k)
          if (tm[k] >= tm[k - 1]) g_dph_sum[k] += (double)(tm[k] - tm[k - 1]) * 0.01;   // 100 MHz clock
        g_dph_sum[0] += (double)(tm[nph - 1] - tm[0]) * 0.01;
        ++g_dph_calls;
      }
    }
    const int r2 = decode_call_results(&w->count, h_res, h_o, h_out, h_out_len, h_consumed, h_status, h_unknown,
                                       unknown_cap, h_nunknown, h_extract_hash, extract_cap, h_nextract);
    if (r2 != XCG_ENOTSUP) return r2;
    // (fallback: the batch decoder takes it; nothing was written)
  }
  return decode_call_batch(c, h_in, len, h_out, out_cap, h_out_len, h_consumed, h_status, h_unknown, unknown_cap,
                           h_nunknown);
}

}  // extern "C"

namespace {
std::atomic<uint64_t> g_dcm_launches{0}, g_dcm_done{0}, g_dcm_outside{0};

struct ManyCall {                  // one call of a group, as staged
  uint32_t i;                      // its place in the caller's arrays
  xcg_window* w;
  size_t in_off, out_off, res_off, scr_off;   // in the up block, the down block (both), the scratch block
  uint32_t ops_cap;
};
// What call i stages on the device: its record, input, output, results and op scratch.
size_t many_call_bytes(uint32_t len, uint64_t out_cap) {
  return align_up(xcg_small_dec_size(), 256) + align_up(len, 256) + align_up(out_cap ? out_cap : 1, 256) +
         align_up(8ull * xcg::SD_RES_WORDS, 256) + align_up(xcg::SD_SCRATCH_PER_OP * (len / 4 + 64), 256);
}
}  // namespace

extern "C" {

int xcg_decode_call_many(xcg_ctx* const* ctx, xcg_window* const* windows, const uint8_t* const* h_in,
                         const uint32_t* len, uint8_t* const* h_out, const uint64_t* out_cap, uint32_t n,
                         uint64_t* h_out_len, uint64_t* h_consumed, int32_t* h_status, uint64_t* const* h_unknown,
                         const uint32_t* unknown_cap, uint32_t* h_nunknown, uint64_t* const* h_extract_hash,
                         const uint32_t* extract_cap, uint32_t* h_nextract, int* rc_out) {
  if (n == 0) return XCG_OK;
  if (!ctx || !h_in || !len || !h_out || !out_cap || !h_out_len || !h_consumed || !h_status || !h_unknown ||
      !unknown_cap || !h_nunknown || !rc_out || (h_extract_hash && (!extract_cap || !h_nextract)))
    return XCG_EINVAL;
  std::vector<xcg_window*> win(n);
  {
    std::vector<const void*> cs, ws;
    for (uint32_t i = 0; i < n; ++i) {
      xcg_ctx* c = ctx[i];
      if (!c || c->device != ctx[0]->device || (len[i] && !h_in[i]) || (out_cap[i] && !h_out[i]) ||
          (unknown_cap[i] && !h_unknown[i]))
        return XCG_EINVAL;
      win[i] = windows && windows[i] ? windows[i] : c->cur_win;   // (null: the context's own, not made yet)
      if (win[i] && win[i]->device != c->device) return XCG_EINVAL;
      cs.push_back(c);
      if (win[i]) ws.push_back(win[i]);
    }
    std::sort(cs.begin(), cs.end(), std::less<const void*>());
    std::sort(ws.begin(), ws.end(), std::less<const void*>());
    if (std::adjacent_find(cs.begin(), cs.end()) != cs.end() || std::adjacent_find(ws.begin(), ws.end()) != ws.end())
      return XCG_EINVAL;
  }
  std::vector<uint32_t> outside;                        // calls the launch does not serve
  std::vector<uint32_t> elig;
  for (uint32_t i = 0; i < n; ++i) {
    h_out_len[i] = h_consumed[i] = 0;
    h_status[i] = 0;
    h_nunknown[i] = 0;
    if (h_nextract) h_nextract[i] = XCG_NO_REFERENCES;
    rc_out[i] = XCG_OK;
    if (len[i] == 0) continue;
    (decode_call_fast(ctx[i], len[i]) ? elig : outside).push_back(i);
  }
  DeviceGuard g(ctx[0]->device);
  const size_t recb = xcg_small_dec_size(), resb = align_up(8ull * xcg::SD_RES_WORDS, 256);
  size_t e0 = 0;
  while (e0 < elig.size()) {
    // the group: consecutive eligible calls whose staging stays under the bound
    size_t e1 = e0, bytes = 0;
    while (e1 < elig.size()) {
      const size_t b = many_call_bytes(len[elig[e1]], out_cap[elig[e1]]);
      if (e1 > e0 && bytes + b > XCG_DECODE_CALL_MANY_STAGE) break;
      bytes += b;
      ++e1;
    }
    const uint32_t m = (uint32_t)(e1 - e0);
    xcg_ctx* c0 = ctx[elig[e0]];
    // up: records | inputs;  down: per call output | results;  then the op scratch (device only)
    std::vector<ManyCall> mc(m);
    size_t up = align_up(recb * m, 256), down = 0, scr = 0;
    for (uint32_t k = 0; k < m; ++k) {
      ManyCall& q = mc[k];
      q.i = elig[e0 + k];
      xcg_ctx* c = ctx[q.i];
      int rc = ensure_cache(c);
      if (rc == XCG_OK && !win[q.i]) {
        if (!c->own_win) rc = window_alloc(c->device, &c->own_win);
        c->cur_win = c->own_win;
        win[q.i] = c->cur_win;
      }
      if (rc != XCG_OK) return rc;
      q.w = win[q.i];
      q.ops_cap = len[q.i] / 4 + 64;
      q.in_off = up;
      up += align_up(len[q.i], 256);
      q.out_off = down;
      down += align_up(out_cap[q.i] ? out_cap[q.i] : 1, 256);
      q.res_off = down;
      down += resb;
      q.scr_off = scr;
      scr += align_up(xcg::SD_SCRATCH_PER_OP * q.ops_cap, 256);
    }
    int rc = ensure_stage(c0, up + down + scr, up + down);
    if (rc != XCG_OK) return rc;
    uint8_t* dm = c0->stage_d;
    uint8_t* hm = c0->stage_h;
    const hipStream_t st = c0->call_st;
    for (uint32_t k = 0; k < m; ++k) {
      const ManyCall& q = mc[k];
      xcg_ctx* c = ctx[q.i];
      memcpy(hm + q.in_off, h_in[q.i], len[q.i]);
      xcg_small_dec_fill(hm + recb * k, dm + q.in_off, len[q.i], &c->g, c->d_status, dm + up + down + q.scr_off,
                         q.ops_cap, dm + up + q.out_off, out_cap[q.i], q.w->hash, q.w->seg, q.w->count,
                         (uint64_t*)(dm + up + q.res_off));
      ctx_order(c, st);                                 // behind every listed context's earlier work
    }
    const bool ok = hipMemcpyAsync(dm, hm, up, hipMemcpyHostToDevice, st) == hipSuccess &&
                    xcg_launch_decode_calls(dm, m, st) == 0 &&
                    hipMemcpyAsync(hm + up, dm + up, down, hipMemcpyDeviceToHost, st) == hipSuccess;
    for (uint32_t k = 0; k < m; ++k) ctx_mark(ctx[mc[k].i], st);
    if (!ok || hipStreamSynchronize(st) != hipSuccess) return XCG_EHIP;
    // (the stream is c0's: the other contexts record their completion now, while it certainly exists)
    for (uint32_t k = 0; k < m; ++k)
      if (ctx[mc[k].i] != c0) ctx_flush_mark(ctx[mc[k].i]);
    ++g_dcm_launches;
    for (uint32_t k = 0; k < m; ++k) {
      const ManyCall& q = mc[k];
      const uint32_t i = q.i;
      uint32_t ne = XCG_NO_REFERENCES;
      const int r2 = decode_call_results(&q.w->count, (const uint64_t*)(hm + up + q.res_off), hm + up + q.out_off,
                                         h_out[i], &h_out_len[i], &h_consumed[i], &h_status[i], h_unknown[i],
                                         unknown_cap[i], &h_nunknown[i], h_extract_hash ? h_extract_hash[i] : nullptr,
                                         h_extract_hash ? extract_cap[i] : 0u, &ne);
      if (r2 == XCG_ENOTSUP) {                          // the kernel declined; nothing was written
        outside.push_back(i);
        continue;
      }
      if (h_nextract) h_nextract[i] = ne;
      rc_out[i] = r2;
      if (r2 == XCG_OK) ++g_dcm_done;
    }
    e0 = e1;
  }
  // in list order (pair fronts of one disk keep theirs), each on its window
  std::sort(outside.begin(), outside.end());
  for (const uint32_t i : outside) {
    xcg_ctx* c = ctx[i];
    xcg_window* const prev = c->cur_win;
    if (windows && windows[i]) c->cur_win = windows[i];
    rc_out[i] = decode_call_batch(c, h_in[i], len[i], h_out[i], out_cap[i], &h_out_len[i], &h_consumed[i],
                                  &h_status[i], h_unknown[i], unknown_cap[i], &h_nunknown[i]);
    c->cur_win = prev ? prev : c->own_win;
    ++g_dcm_outside;
  }
  return XCG_OK;
}

void xcg_debug_decode_call_many(uint64_t out[3]) {
  out[0] = g_dcm_launches;
  out[1] = g_dcm_done;
  out[2] = g_dcm_outside;
}

uint32_t xcg_debug_decode_phases(double* us, uint32_t n) {
  std::lock_guard<std::mutex> g(g_dph_mu);
  for (uint32_t k = 0; k < n; ++k) us[k] = k < g_dph_sum.size() ? g_dph_sum[k] : 0.0;
  const uint32_t calls = g_dph_calls;
  g_dph_sum.assign(g_dph_sum.size(), 0.0);
  g_dph_calls = 0;
  return calls;
}

}  // extern "C"
