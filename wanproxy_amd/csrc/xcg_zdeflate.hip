// The deflate stage's host side: the xcg_zdeflate object (one DeflatePipe per stream), the batch drivers for
// levels 1-9 and level 0, the host-buffer entry point, and the kernels that close a call (zd_commit_kernel, level
// 0's byte moves).  The stage's map is at the top of xcg_zdeflate.h; the scratch's layout is xcg_zdeflate_plan.h.
#include <string.h>

#include <algorithm>
#include <vector>

#include "xcg_zdeflate.h"
#include "xcg_zdeflate_plan.h"   // xcgpu.h, xcg_devmem.h, xcg_stored_plan.h

namespace xcg {
namespace zd {

// ------------------------------------------------------------------- commit
// Stream state after the call: history = the last 32 KiB of X, position,
// window base, adler, flags.  Grid: (8 tiles, calls).
__global__ __launch_bounds__(256) void zd_commit_kernel(ZArgs a) {
  const uint32_t ci = blockIdx.y;
  const ZCall c = a.calls[ci];
  const uint8_t* X = a.X + c.x_off + c.len;   // X[len .. len + WSIZE) = the last WSIZE positions
  uint8_t* h = a.hist + (uint64_t)c.stream * WSIZE;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < (uint32_t)WSIZE / 4; i += gridDim.x * 256) {
    const uint8_t* q = X + 4 * i;
    *(uint32_t*)(h + 4 * i) = q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ZState s = a.st[c.stream];
    const ZCallRes& r = a.res[ci];
    const int64_t x2s = (int64_t)s.total - WSIZE;   // X index -> stream position
    if (r.stop) {   // resume right after the block the flush call stopped at
      const ZBlock& B = a.blk[c.blk_off + r.stop - 1];
      s.base = (uint64_t)(x2s + B.bidx);
      s.dlen = (uint32_t)((int64_t)WSIZE + c.len - (int64_t)B.p_after);
      s.block_start = (uint64_t)(x2s + (int64_t)B.start + B.stored_len);
      s.mstart = (uint64_t)(x2s + (int64_t)B.ms);
      s.avail = B.avail;
      s.mlen = B.ml;
      const uint64_t e = r.end_bit;
      s.cnb = (uint32_t)(e & 7);
      s.cbits = s.cnb ? a.out[c.out_off + (e >> 3)] & ((1u << s.cnb) - 1u) : 0u;
    } else {
      s.base = r.base_end;
      s.dlen = 0;
      s.block_start = (uint64_t)((int64_t)s.total + c.len);
      s.avail = 0;
      s.mlen = MIN_MATCH - 1;
      s.cnb = 0;
      s.cbits = 0;
    }
    s.pend = s.pend + r.out_bytes - r.deliver;
    s.total += c.len;
    s.adler = c.len ? r.adler : s.adler;
    s.flags |= 1u;
    if (c.len == 0) s.flags |= 2u;
    a.st[c.stream] = s;
  }
}

// ------------------------------------------------------------------- level 0
// deflate_stored (deflate.c, zlib 1.2.11) writes no Huffman codes: a stream
// is stored blocks (5 header bytes + raw bytes) whose sizes follow zlib's
// control flow over avail_in (the Buffer's segments, <= 2048 bytes each) and
// avail_out (DeflatePipe's 64 KiB buffer, deflate_pipe.cc:57-115): it copies
// blocks straight to next_out while they are >= 32 KiB (or flush everything),
// and otherwise collects input in its 64 KiB window and emits from there.
// The host replays that control flow over lengths only (StoredPlan) and the
// GPU moves the bytes (zs_copy_kernel): every piece of a call's output is a
// header, a range of the stream (this call's input, or earlier bytes from the
// stream's 64 KiB ring) or the adler32 trailer.
__global__ __launch_bounds__(256) void zs_copy_kernel(const ZPiece* pc, const ZCall* calls, const ZState* st,
                                                      const uint8_t* in, const uint8_t* ring, uint8_t* out) {
  const ZPiece p = pc[blockIdx.x];
  const ZCall c = calls[p.call];
  uint8_t* o = out + c.out_off + p.out;
  if (p.kind == 0) {
    if (threadIdx.x < p.len) o[threadIdx.x] = (uint8_t)(p.src >> (8 * threadIdx.x));
    return;
  }
  if (p.kind == 2) {
    const uint32_t ad = st[c.stream].adler;
    if (threadIdx.x < 4) o[threadIdx.x] = (uint8_t)(ad >> (24 - 8 * threadIdx.x));
    return;
  }
  const uint64_t total = st[c.stream].total;           // stream position of this call's first byte
  const uint8_t* r = ring + (uint64_t)c.stream * (2 * WSIZE);
  for (uint32_t i = threadIdx.x; i < p.len; i += 256) {
    const uint64_t q = p.src + i;
    o[i] = q >= total ? in[c.in_off + (q - total)] : r[q & (2 * WSIZE - 1)];
  }
}

// The stream's last 64 KiB (ring by position) after the call; adler, position.
__global__ __launch_bounds__(256) void zs_commit_kernel(ZArgs a) {
  const ZCall c = a.calls[blockIdx.x];
  const ZState s0 = a.st[c.stream];
  uint8_t* r = a.hist + (uint64_t)c.stream * (2 * WSIZE);
  const uint32_t keep = c.len < 2u * WSIZE ? c.len : 2u * WSIZE;
  for (uint32_t i = threadIdx.x; i < keep; i += 256) {
    const uint64_t q = s0.total + c.len - keep + i;
    r[q & (2 * WSIZE - 1)] = a.in[c.in_off + (c.len - keep + i)];
  }
  if (threadIdx.x == 0) {
    ZState s = s0;
    s.total += c.len;
    s.adler = c.len ? a.res[blockIdx.x].adler : s.adler;
    s.flags |= 1u;
    if (c.len == 0) s.flags |= 2u;
    a.st[c.stream] = s;
  }
}

}  // namespace zd
}  // namespace xcg

using namespace xcg::zd;

struct xcg_zdeflate {
  xcg::DevMem mem;                 // every buffer below
  int device = 0, level = 6;
  uint32_t nstreams = 0;
  ZState* st = nullptr;
  uint8_t* hist = nullptr;
  std::vector<ZState> h_init;
  // scratch (grow-only)
  uint8_t* scratch = nullptr;
  size_t scratch_cap = 0;
  void* meta = nullptr;       // ZCall[] + tile maps + block maps (device)
  size_t meta_cap = 0;
  void* h_meta = nullptr;     // pinned staging for meta
  size_t h_meta_cap = 0;
  hipEvent_t done = nullptr;
  uint32_t* ring = nullptr;   // deflate_fast: per stream, the hashed positions of the last 32 KiB
  uint32_t* h_changed = nullptr;   // pinned, per call (deflate_fast rounds)
  size_t h_changed_cap = 0;
  uint32_t last_rounds = 0;
  std::vector<StoredPlan> splan;   // level 0: zlib's control state per stream (host, lengths only)
  // host-buffer calls (xcg_zdeflate_host: the drop-in DeflatePipe::consume):
  // kept staging and a private stream, one synchronisation per call
  hipStream_t hst = nullptr;
  uint8_t* hs_h = nullptr;         // pinned
  uint8_t* hs_d = nullptr;
  size_t hs_hcap = 0, hs_dcap = 0;
};

namespace {
ZState fresh_state() {   // deflateInit
  ZState s;
  memset(&s, 0, sizeof s);
  s.adler = 1u;
  s.mlen = MIN_MATCH - 1;
  return s;
}
}  // namespace

extern "C" {

uint64_t xcg_zdeflate_bound(uint32_t len) { return zdeflate_bound(len); }

int xcg_zdeflate_create(int device, int level, uint32_t nstreams, xcg_zdeflate** out) {
  if (!out || level < 0 || level > 9 || nstreams == 0) return XCG_EINVAL;
  if (hipSetDevice(device) != hipSuccess) return XCG_EHIP;
  xcg_zdeflate* z = new xcg_zdeflate();
  z->device = device;
  z->level = level;
  z->nstreams = nstreams;
  auto fail = [&](int rc) {
    xcg_zdeflate_destroy(z);
    return rc;
  };
  if (!(z->mem.dev(&z->st, sizeof(ZState) * nstreams) &&
        z->mem.dev(&z->hist, (size_t)WSIZE * (level == 0 ? 2 : 1) * nstreams)) ||
      hipEventCreateWithFlags(&z->done, hipEventDisableTiming) != hipSuccess ||
      (level < 4 && (!z->mem.dev(&z->ring, (size_t)WSIZE / 8 * nstreams) ||
                     hipMemset(z->ring, 0, (size_t)WSIZE / 8 * nstreams) != hipSuccess)))
    return fail(XCG_ENOMEM);
  z->h_init.assign(nstreams, fresh_state());
  if (level == 0) z->splan.assign(nstreams, StoredPlan());
  if (hipMemcpy(z->st, z->h_init.data(), sizeof(ZState) * nstreams, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(z->hist, 0, (size_t)WSIZE * nstreams) != hipSuccess)
    return fail(XCG_EHIP);
  *out = z;
  return XCG_OK;
}

void xcg_zdeflate_destroy(xcg_zdeflate* z) {
  if (!z) return;
  (void)hipSetDevice(z->device);
  if (z->done) (void)hipEventSynchronize(z->done);
  z->mem.release_all();
  if (z->hst) (void)hipStreamDestroy(z->hst);
  if (z->done) (void)hipEventDestroy(z->done);
  delete z;
}

int xcg_zdeflate_reset(xcg_zdeflate* z, uint32_t stream) {
  if (!z || stream >= z->nstreams) return XCG_EINVAL;
  (void)hipSetDevice(z->device);
  if (hipEventSynchronize(z->done) != hipSuccess) return XCG_EHIP;
  const ZState s0 = fresh_state();
  if (hipMemcpy(z->st + stream, &s0, sizeof s0, hipMemcpyHostToDevice) != hipSuccess) return XCG_EHIP;
  if (z->ring && hipMemset(z->ring + (size_t)stream * (WSIZE / 32), 0, WSIZE / 8) != hipSuccess) return XCG_EHIP;
  if (!z->splan.empty()) z->splan[stream] = StoredPlan();
  return XCG_OK;
}

}  // extern "C"

namespace {
// Level 0: the host replays zlib's control flow per consume (StoredPlan), the
// GPU computes adler32, moves the pieces and keeps each stream's last 64 KiB.
int stored_batch(xcg_zdeflate* z, const uint8_t* d_in, const uint64_t* h_in_off, const uint32_t* h_len,
                 const uint32_t* h_stream, uint32_t n, const uint32_t* h_seg, const uint32_t* h_nseg, uint8_t* d_out,
                 const uint64_t* h_out_off, uint32_t* d_out_len, uint64_t* d_deliver, hipStream_t st) {
  // the plan mutates the streams' host state: check everything first, then plan
  if (int rc = check_calls(z->nstreams, h_stream, h_out_off, h_len, n)) return rc;
  std::vector<ZCall> calls(n);
  std::vector<ZPiece> pieces;
  std::vector<uint32_t> made32(n);
  std::vector<uint64_t> deliver(n);
  uint64_t so = 0;
  for (uint32_t i = 0; i < n; i++) {
    ZCall& c = calls[i];   // (all zero from the vector)
    c.in_off = h_in_off[i];
    c.out_off = h_out_off[i];
    c.len = h_len[i];
    c.stream = h_stream[i];
    const size_t first = pieces.size();
    uint64_t made = 0;
    const uint32_t ns = h_nseg ? h_nseg[i] : 0;
    if (!z->splan[c.stream].consume(c.len, h_seg ? h_seg + so : nullptr, ns, pieces, &made, &deliver[i]))
      return XCG_EINVAL;
    so += ns;
    if (made > xcg_zdeflate_bound(c.len)) return XCG_EOVERFLOW;
    made32[i] = (uint32_t)made;
    for (size_t k = first; k < pieces.size(); k++) pieces[k].call = i;
  }
  const ZsMeta m(n, pieces.size());
  if (hipEventSynchronize(z->done) != hipSuccess) return XCG_EHIP;
  if (!z->mem.grow_bytes(&z->scratch, &z->scratch_cap, m.res_bytes, xcg::MEM_DEV)) return XCG_ENOMEM;
  if (!z->mem.grow_bytes(&z->meta, &z->meta_cap, m.end, xcg::MEM_DEV) ||
      !z->mem.grow_bytes(&z->h_meta, &z->h_meta_cap, m.end, xcg::MEM_PINNED))
    return XCG_ENOMEM;
  uint8_t* hm = (uint8_t*)z->h_meta;
  memcpy(hm + m.calls, calls.data(), sizeof(ZCall) * n);
  if (!pieces.empty()) memcpy(hm + m.pc, pieces.data(), sizeof(ZPiece) * pieces.size());
  memcpy(hm + m.len, made32.data(), 4ull * n);
  memcpy(hm + m.dl, deliver.data(), 8ull * n);
  if (hipMemcpyAsync(z->meta, hm, m.end, hipMemcpyHostToDevice, st) != hipSuccess) return XCG_EHIP;
  uint8_t* dm = (uint8_t*)z->meta;
  if (hipMemcpyAsync(d_out_len, dm + m.len, 4ull * n, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d_deliver, dm + m.dl, 8ull * n, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return XCG_EHIP;
  ZArgs a{};
  a.calls = (const ZCall*)(dm + m.calls);
  a.st = z->st;
  a.hist = z->hist;
  a.in = d_in;
  a.out = d_out;
  a.res = (ZCallRes*)z->scratch;
  a.n = n;
  a.level = 0;
  zd_launch_adler(a, st);
  if (!pieces.empty())
    hipLaunchKernelGGL(zs_copy_kernel, dim3((unsigned)pieces.size()), dim3(256), 0, st, (const ZPiece*)(dm + m.pc),
                       a.calls, (const ZState*)z->st, d_in, (const uint8_t*)z->hist, d_out);
  hipLaunchKernelGGL(zs_commit_kernel, dim3(n), dim3(256), 0, st, a);
  if (hipGetLastError() != hipSuccess) return XCG_EHIP;
  if (hipEventRecord(z->done, st) != hipSuccess) return XCG_EHIP;
  return XCG_OK;
}
}  // namespace

extern "C" {

int xcg_zdeflate_batch_seg(xcg_zdeflate* z, const uint8_t* d_in, const uint64_t* h_in_off, const uint32_t* h_len,
                           const uint32_t* h_stream, uint32_t n, const uint32_t* h_seg, const uint32_t* h_nseg,
                           uint8_t* d_out, const uint64_t* h_out_off, uint32_t* d_out_len, uint64_t* d_deliver,
                           void* stream) {
  if (!z || n == 0 || !h_in_off || !h_len || !h_stream || !h_out_off || !d_out || !d_out_len || !d_deliver ||
      (h_seg && !h_nseg))
    return XCG_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  (void)hipSetDevice(z->device);
  if (z->level == 0)
    return stored_batch(z, d_in, h_in_off, h_len, h_stream, n, h_seg, h_nseg, d_out, h_out_off, d_out_len, d_deliver,
                        st);
  if (int rc = check_calls(z->nstreams, h_stream, h_out_off, h_len, n)) return rc;
  const ZdPlan p(h_in_off, h_len, h_stream, h_out_off, n, z->level);
  // the previous batch may still read the scratch
  if (hipEventSynchronize(z->done) != hipSuccess) return XCG_EHIP;
  if (!z->mem.grow_bytes(&z->scratch, &z->scratch_cap, p.s.end, xcg::MEM_DEV) ||
      !z->mem.grow_bytes(&z->meta, &z->meta_cap, p.m.end, xcg::MEM_DEV) ||
      !z->mem.grow_bytes(&z->h_meta, &z->h_meta_cap, p.m.end, xcg::MEM_PINNED) ||
      (p.fast && !z->mem.grow_bytes(&z->h_changed, &z->h_changed_cap, 4ull * n, xcg::MEM_PINNED)))
    return XCG_ENOMEM;
  p.fill_meta((uint8_t*)z->h_meta);
  if (hipMemcpyAsync(z->meta, z->h_meta, p.m.end, hipMemcpyHostToDevice, st) != hipSuccess) return XCG_EHIP;
  ZArgs a{};
  p.bind(a, z->scratch, (uint8_t*)z->meta);
  a.st = z->st;
  a.hist = z->hist;
  a.in = d_in;
  a.out = d_out;
  a.out_len = d_out_len;
  a.deliver = d_deliver;
  a.ring = z->ring;
  // from here on only a HIP failure returns early (and the round limit, right after a synchronisation)
  zd_launch_prep(a, p.maxlen, st);
  zd_launch_adler(a, st);
  if (!p.fast) {
    zd_launch_match(a, p.groups, p.mtiles, st);
    zd_launch_scan(a, st);
  } else {
    // deflate_fast: which positions zlib hashes depends on its own parse.  Guess
    // (round 0: all), build the chains and the match table from the guess, parse,
    // and repeat with the parse's hashed positions until they reproduce the guess
    // (the correct prefix grows every round, so this ends).
    zd_launch_mfill(a, p.mo, st);
    uint32_t rounds = 0;
    for (;;) {
      rounds++;
      if (hipMemsetAsync(a.changed, 0, 4ull * n, st) != hipSuccess) return XCG_EHIP;
      zd_launch_match(a, p.groups, p.mtiles, st);
      zd_launch_fscan(a, st);
      if (hipMemcpyAsync(z->h_changed, a.changed, 4ull * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess)
        return XCG_EHIP;
      bool any = false;
      for (uint32_t i = 0; i < n && !any; i++) any = z->h_changed[i] != 0;
      std::swap(a.mcur, a.mnext);   // the parse's positions are the next guess (and, when equal, final)
      if (!any) break;
      if (rounds > 100000) return XCG_EOVERFLOW;
      zd_launch_mzero(a, p.mo, st);
    }
    z->last_rounds = rounds;
  }
  zd_launch_huff(a, p.bo, st);
  if (p.fast) zd_launch_ring(a, st);   // (before commit moves the state)
  hipLaunchKernelGGL(zd_commit_kernel, dim3(8, n), dim3(256), 0, st, a);
  if (hipGetLastError() != hipSuccess) return XCG_EHIP;
  if (hipEventRecord(z->done, st) != hipSuccess) return XCG_EHIP;
  return XCG_OK;
}

int xcg_zdeflate_batch(xcg_zdeflate* z, const uint8_t* d_in, const uint64_t* h_in_off, const uint32_t* h_len,
                       const uint32_t* h_stream, uint32_t n, uint8_t* d_out, const uint64_t* h_out_off,
                       uint32_t* d_out_len, uint64_t* d_deliver, void* stream) {
  return xcg_zdeflate_batch_seg(z, d_in, h_in_off, h_len, h_stream, n, nullptr, nullptr, d_out, h_out_off, d_out_len,
                                d_deliver, stream);
}

// Host buffers: one consume() per listed stream, inputs concatenated in h_in
// at h_in_off, outputs to h_out at h_out_off (room for xcg_zdeflate_bound);
// lengths to h_out_len.  Synchronous.
int xcg_zdeflate_host(xcg_zdeflate* z, const uint8_t* h_in, const uint64_t* h_in_off, const uint32_t* h_len,
                      const uint32_t* h_stream, uint32_t n, const uint32_t* h_seg, const uint32_t* h_nseg,
                      uint8_t* h_out, const uint64_t* h_out_off, uint32_t* h_out_len, uint64_t* h_deliver) {
  if (!z || n == 0 || !h_deliver || !h_out_len || !h_in_off || !h_len) return XCG_EINVAL;
  (void)hipSetDevice(z->device);
  if (!z->hst && hipStreamCreateWithFlags(&z->hst, hipStreamNonBlocking) != hipSuccess) return XCG_EHIP;
  const ZdStaging g(h_in_off, h_len, n);
  if (!z->mem.grow_bytes(&z->hs_h, &z->hs_hcap, g.end, xcg::MEM_PINNED) ||
      !z->mem.grow_bytes(&z->hs_d, &z->hs_dcap, g.end, xcg::MEM_DEV))
    return XCG_ENOMEM;
  if (g.in_end) memcpy(z->hs_h, h_in, g.in_end);
  if (g.in_end && hipMemcpyAsync(z->hs_d, z->hs_h, g.in_end, hipMemcpyHostToDevice, z->hst) != hipSuccess)
    return XCG_EHIP;
  int rc = xcg_zdeflate_batch_seg(z, z->hs_d, h_in_off, h_len, h_stream, n, h_seg, h_nseg, z->hs_d + g.out,
                                  g.doff.data(), (uint32_t*)(z->hs_d + g.len), (uint64_t*)(z->hs_d + g.dl), z->hst);
  if (rc != XCG_OK) return rc;
  // the outputs' room (<= 1.5x the input) comes back with the lengths: one synchronisation
  if (hipMemcpyAsync(z->hs_h + g.out, z->hs_d + g.out, g.end - g.out, hipMemcpyDeviceToHost, z->hst) != hipSuccess ||
      hipStreamSynchronize(z->hst) != hipSuccess)
    return XCG_EHIP;
  memcpy(h_out_len, z->hs_h + g.len, 4ull * n);
  memcpy(h_deliver, z->hs_h + g.dl, 8ull * n);
  for (uint32_t i = 0; i < n; i++) memcpy(h_out + h_out_off[i], z->hs_h + g.out + g.doff[i], h_out_len[i]);
  return XCG_OK;
}

uint32_t xcg_debug_zdeflate_rounds(const xcg_zdeflate* z) { return z ? z->last_rounds : 0; }

#ifdef XCG_ZD_TIMING
int xcg_debug_zd_times(uint64_t* out) {
  memset(out, 0, 8 * 16);
  return zd_parse_times(out) && zd_huff_times(out) ? XCG_OK : XCG_EHIP;
}
#endif

}  // extern "C"
