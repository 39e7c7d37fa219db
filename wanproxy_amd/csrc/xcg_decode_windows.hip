// XCodec decoder, MI355X (gfx950) HIP kernels: the window passes of a batch
// whose chunks are decode() calls on several decoders (one XCodecWindow each,
// xcodec/xcodec_decoder.h) over one cache (xcg_decode_batch_windows).
//
// xcg_launch_decode runs the batch; the scan, refcheck, sizing, name reuse and
// commit passes do not know about windows.  What xcg_decode.hip does for the
// one window of xcg_decode_batch happens here per window:
//
//   number  the chunks' declare counts scanned in the host plan's window-major
//           order (xcg_decode_windows_plan.h): a chunk's base counts the
//           earlier declares of its own window, and a window's declares are
//           one range [first, first + total) of the window-major numbering
//   records (hash, bytes) of the declares, by decl_record_chunk: every one,
//           window-major, when the batch holds BACKREFs; else, after the emit
//           pass, the 256 before each window's t_end, in the window's own 256
//           slots of the tail scratch.  (The emit pass does not write tail
//           records on this path: which declares are a window's last 256 is
//           known per window only, and one more header walk over the few
//           chunks that hold them costs less than a view lookup per declare.)
//   t_end   per window: the declares of its chunks before the stop chunk, plus
//           what the stop chunk emitted when it is the window's own
//   update  window_update_kernel's step over (window, slot); a window the
//           batch did not declare into is not touched
//
// On a bounded or pair context (xcg_decode_batch_windows_bounded) the
// classified passes of xcg_decode_bounded.hip index their op list in batch
// order, not by window: dec_windows_op_base scans the declare counts once more,
// in chunk order, for them.
//
// The emit and BACKREF-check kernels are xcg_decode.hip's, instantiated with
// WINS: their BACKREFs read the chunk's ManyWindow through window_slot_of
// (xcg_decode_batch.h) instead of the one window through window_slot.
#include "xcg_decode_batch.h"

namespace xcg {

namespace {

// Position j of the window-major order: chunk order[j]'s declare count.
__global__ __launch_bounds__(256) void win_gather_kernel(const uint64_t* n_decl, const uint32_t* order, uint32_t n,
                                                         uint64_t* cnt) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j < n) cnt[j] = n_decl[order[j]];
}

// From the scan of those counts (base[j], *total): each window's first declare
// and total, and each chunk's base within its window.
__global__ __launch_bounds__(256) void win_first_kernel(const uint64_t* base, const uint64_t* total,
                                                        const uint32_t* first, uint32_t n, uint32_t n_windows,
                                                        WinView* wins) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= n_windows) return;
  const uint32_t a = first[w], b = first[w + 1];
  const uint64_t fa = a < n ? base[a] : *total, fb = b < n ? base[b] : *total;
  wins[w].first = fa;
  wins[w].total = fb - fa;
}
__global__ __launch_bounds__(256) void win_base_kernel(const uint64_t* base, const uint32_t* order,
                                                       const uint32_t* chunk_win, const WinView* wins, uint32_t n,
                                                       uint64_t* decl_base) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const uint32_t chunk = order[j];
  decl_base[chunk] = base[j] - wins[chunk_win[chunk]].first;
}

// Declare records, one wave per chunk.  Full: every declare of window w at
// D[first_w + t].  Tail: the declares [max(t_end_w - 256, 0), t_end_w) at
// D[256 w + t - lo].
template <bool REUSE>
__global__ __launch_bounds__(256) void win_record_kernel(DecParams prm) {
  const int wv = (int)readfirst(threadIdx.x >> 6);
  const uint32_t chunk = blockIdx.x * 4u + (uint32_t)wv;
  if (chunk >= prm.n) return;
  const uint32_t w = readfirst(prm.chunk_win[chunk]);
  const WinView* v = prm.wins + w;
  uint64_t lo_t = 0, hi_t, off;
  if (prm.D_tail) {
    hi_t = readfirst64(prm.w_tend[w]);
    lo_t = hi_t > 256u ? hi_t - 256u : 0u;
    off = 256ull * w - lo_t;
  } else {
    hi_t = readfirst64(v->total);
    off = readfirst64(v->first);
  }
  const uint64_t base = readfirst64(prm.decl_base[chunk]), cnt = readfirst64(prm.n_decl[chunk]);
  if (base >= hi_t || base + cnt <= lo_t) return;
  decl_record_chunk<REUSE>(prm, chunk, base, lo_t, hi_t, off);
}

// Each window's declares before the stop point (the first unknown REF or
// invalid BACKREF of the batch).  A window's chunks are ascending in `order`:
// the first one at or after the stop chunk bounds what the window declared.
__global__ __launch_bounds__(256) void win_tend_kernel(DecParams prm, const uint32_t* order, const uint32_t* first,
                                                       uint32_t n_windows) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= n_windows) return;
  const uint64_t stop = min(*prm.block_pos, *prm.berr_pos);
  uint64_t te = prm.wins[w].total;
  if (stop != ~0ull) {
    const uint32_t sc = (uint32_t)(stop >> 32);
    uint32_t a = first[w], b = first[w + 1];
    const uint32_t end = b;
    while (a < b) {                                          // first position with order[] >= sc
      const uint32_t mid = a + ((b - a) >> 1);
      if (order[mid] < sc) a = mid + 1;
      else b = mid;
    }
    if (a < end) {
      const uint32_t c = order[a];
      te = prm.decl_base[c] + (c == sc ? prm.n_decl_emit[c] : 0u);
    }
  }
  prm.w_tend[w] = te;
}

// One wave per (window, slot): 64 workgroups a window.
__global__ __launch_bounds__(256) void win_update_kernel(DecParams prm, uint32_t n_windows) {
  const uint32_t w = blockIdx.x >> 6;
  const uint32_t c = (blockIdx.x & 63u) * 4u + (uint32_t)readfirst(threadIdx.x >> 6);
  if (w >= n_windows) return;
  const uint64_t T = readfirst64(prm.w_tend[w]);
  if (T == 0) return;
  const ManyWindow win(prm, w);
  uint64_t h = 0, gd = 0;
  const uint8_t* src = nullptr;
  const bool ok = window_slot_of(win, T, c, h, src, gd);
  const uint64_t G = win.count + T;
  const bool written = ((G - 1u - c) & 255u) <= G - 1u;
  if (!written) return;
  if (!ok) {
    if (lane_id() == 0) win.hash[c] = 0;
    return;
  }
  if (gd >= win.count) wave_copy2048(win.seg + (uint64_t)c * SEG, src);
  if (lane_id() == 0) win.hash[c] = h;
}

}  // namespace

void dec_windows_number(const XcgDecodeWindows* w, const DecParams& p, uint64_t* d_total, hipStream_t stream) {
  const uint32_t n = p.n, nw = w->n_windows;
  uint64_t* cnt = w->scan_tmp;
  uint64_t* base = w->scan_tmp + n;
  const dim3 gn((n + 255) / 256), gw((nw + 255) / 256), block(256);
  hipLaunchKernelGGL(win_gather_kernel, gn, block, 0, stream, (const uint64_t*)p.n_decl, w->order, n, cnt);
  xcg_launch_exclusive_scan(cnt, base, n, d_total, stream);
  hipLaunchKernelGGL(win_first_kernel, gw, block, 0, stream, (const uint64_t*)base, (const uint64_t*)d_total, w->first,
                     n, nw, p.wins);
  hipLaunchKernelGGL(win_base_kernel, gn, block, 0, stream, (const uint64_t*)base, w->order, w->chunk_win,
                     (const WinView*)p.wins, n, (uint64_t*)p.decl_base);
}

const uint64_t* dec_windows_op_base(const XcgDecodeWindows* w, const DecParams& p, uint64_t* d_total,
                                    hipStream_t stream) {
  xcg_launch_exclusive_scan((const uint64_t*)p.n_decl, w->scan_tmp, p.n, d_total, stream);
  return w->scan_tmp;
}

void dec_windows_records(const DecParams& p, bool reuse, hipStream_t stream) {
  const dim3 grid((p.n + 3) / 4), block(256);
  if (reuse) hipLaunchKernelGGL(win_record_kernel<true>, grid, block, 0, stream, p);
  else hipLaunchKernelGGL(win_record_kernel<false>, grid, block, 0, stream, p);
}

void dec_windows_finish(const XcgDecodeWindows* w, DecParams& p, bool full, bool reuse, hipStream_t stream) {
  const uint32_t nw = w->n_windows;
  hipLaunchKernelGGL(win_tend_kernel, dim3((nw + 255) / 256), dim3(256), 0, stream, p, w->order, w->first, nw);
  if (!full) {
    p.D = w->tail;
    p.D_tail = true;
    dec_windows_records(p, reuse, stream);
  }
  hipLaunchKernelGGL(win_update_kernel, dim3(nw * 64u), dim3(256), 0, stream, p, nw);
}

}  // namespace xcg
