// The configured codec of wanproxy.conf -- `codec XCodec` plus `compressor
// zlib` / `compressor_level N` (wanproxy.conf:32-41) -- as one call per
// direction over many pipes (host C++ over the C ABI, beside xcg_pipe.cpp).
//
// WANProxyCodecPipePair (programs/wanproxy/wanproxy_codec_pipe_pair.cc:76-196)
// links XCodecPipePair and the zlib pipes: towards the peer the pair's bytes go
// through one DeflatePipe, from the peer they come through one InflatePipe.
// The event system is not modelled, so the chain is defined call by call:
//
//   link rule  everything one upstream consume() produces is ONE downstream
//              consume() of one Buffer (PipeProducer::input corks during
//              consume, io/pipe/pipe_producer.cc:58-83, 118-143); a produce_eos
//              is that buffer first, if not empty, then one empty consume.
//   send       W = the pair's encoder_consume output; to_peer = what
//              DeflatePipe::consume(W) produces (zlib/deflate_pipe.cc:57-115),
//              the 64 KiB flush stop included: the undelivered rest is kept here
//              and delivered first by the pipe's next consume.
//   receive    InflatePipe::consume(data) (zlib/inflate_pipe.cc:60-139) gives W
//              and a status; -1 (produce_error) fails the pipe for good, else a
//              non-empty W is the pair's decoder_consume.  An empty receive is
//              an empty inflate consume: status 1 (the stream had ended,
//              produce_eos) hands the pair its bytes, if any, and an empty
//              consume; status 0 hands it nothing (:113-124).
//   replies    every to_peer of the pair -- <ASK>, <ADVANCE>, <LEARN>,
//              <EOS_ACK> of a receive call too -- goes through the pipe's one
//              deflate stream in call order; when the pair reports peer_eos
//              (encoder_produce_eos) one empty DeflatePipe::consume (Z_FINISH)
//              follows and its bytes are appended.
//
// The Buffer handed to DeflatePipe is cut into 2048-byte segments (a Buffer
// filled by append); level 0's stored blocks depend on that.
//
// The send path keeps the wire on the device between the encoder and deflate:
// the encoder step (xcg_pipe_step.h) leaves the encodings in the context's
// staging, the host plans each wire as pieces (xcg_wire_plan.h), one small
// upload carries the literals and the piece arrays, xcg_gather_pieces builds
// the deflate input, xcg_zdeflate_batch runs on it, one readback brings lengths
// and deliver counts, a second gather packs the compressed bytes and one copy
// brings them.  xcg_debug_set_codec_fused switches between this path and the
// plain host composition (the pair's to_peer on the host, then
// xcg_zdeflate_host), which is the default (profiles/codec_pipe.txt, DESIGN.md
// 3.5.1); both give the same bytes.  The receive path is a host composition of
// batched calls.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <vector>

#include "../../include/xcgpu.h"
#include "xcg_args.h"
#include "xcg_devmem.h"
#include "xcg_pipe_step.h"
#include "xcg_wire_plan.h"
#include "xcg_zdeflate_types.h"   // the stages' per-consume limits

struct xcg_codec {
  xcg_ctx* enc = nullptr;
  xcg_ctx* dec = nullptr;          // decoder context, or the parent contexts connect from
  int connect = 0, level = -1, device = 0;
  uint32_t max_pipes = 0;
  xcg_zdeflate* zd = nullptr;      // one DeflatePipe / InflatePipe slot per pipe
  xcg_zinflate* zi = nullptr;
  std::vector<uint32_t> free_slots;
  uint64_t stats[4] = {0, 0, 0, 0};
  // the fused send path's buffers (grow-only) and its stream
  xcg::DevMem mem;
  hipStream_t st = nullptr;
  uint8_t* h_up = nullptr;         // pinned: the plan's upload block
  uint8_t* d_up = nullptr;
  uint8_t* d_wire = nullptr;       // deflate input: the gathered wires
  uint8_t* d_zout = nullptr;       // deflate output slots | [out_len n] | [deliver n]
  uint8_t* d_pack = nullptr;       // the compressed bytes back to back
  uint8_t* h_pack = nullptr;       // pinned
  uint8_t* h_res = nullptr;        // pinned: lengths and deliver counts
  size_t h_up_cap = 0, d_up_cap = 0, d_wire_cap = 0, d_zout_cap = 0, d_pack_cap = 0, h_pack_cap = 0, h_res_cap = 0;
};

struct xcg_codec_pipe {
  xcg_codec* c = nullptr;
  xcg_pipe* pair = nullptr;
  uint32_t slot = 0;
  bool failed = false;                   // InflatePipe's produce_error: XCG_EPROTO from then on
  std::vector<uint8_t> undelivered;      // bytes DeflatePipe made and has not produced yet
  // this call's outputs
  std::vector<uint8_t> to_peer, to_local;
  const uint8_t* local = nullptr;        // to_local: the pair's buffer, or to_local above
  uint64_t local_len = 0;
  int local_eos = 0, peer_eos = 0;

  void begin() {
    to_peer.clear();
    to_local.clear();
    local = nullptr;
    local_len = 0;
    local_eos = peer_eos = 0;
  }
  void take(const xcg_pipe_out& o) {     // a pair call's local side
    local = o.to_local;
    local_len = o.to_local_len;
    local_eos |= o.local_eos;
    peer_eos |= o.peer_eos;
  }
  void finish(xcg_pipe_out* o) const {
    o->to_peer = to_peer.data();
    o->to_peer_len = to_peer.size();
    o->to_local = local;
    o->to_local_len = local_len;
    o->local_eos = local_eos;
    o->peer_eos = peer_eos;
  }
};

namespace {

using xcg::align_up;

std::atomic<int> g_fused{0};   // (the default path: measured)
// Diagnostics (xcg_codec_debug_counts), process-wide.
std::atomic<uint64_t> g_fused_sends{0}, g_host_sends{0}, g_inflate_batches{0}, g_decode_batches{0};

struct Guard {             // the codec's device for the call
  int prev = -1;
  explicit Guard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~Guard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// One DeflatePipe::consume per item: `len` bytes of wire (0: the empty consume, Z_FINISH).
struct Item {
  xcg_codec_pipe* p;
  uint64_t in_off;
  uint32_t len;
};

// What a consume made goes behind the pipe's undelivered bytes; it produces the first `deliver` of them.
int deliver(xcg_codec_pipe* p, const uint8_t* made, uint32_t made_len, uint64_t deliver_len) {
  p->undelivered.insert(p->undelivered.end(), made, made + made_len);
  if (deliver_len > p->undelivered.size()) return XCG_EHIP;
  p->to_peer.insert(p->to_peer.end(), p->undelivered.begin(), p->undelivered.begin() + (ptrdiff_t)deliver_len);
  p->undelivered.erase(p->undelivered.begin(), p->undelivered.begin() + (ptrdiff_t)deliver_len);
  p->c->stats[1] += deliver_len;
  return XCG_OK;
}

// The items' consumes as one xcg_zdeflate_host batch over host wires at h_in.
int deflate_host(xcg_codec* c, const std::vector<Item>& items, const uint8_t* h_in) {
  const uint32_t n = (uint32_t)items.size();
  if (n == 0) return XCG_OK;
  std::vector<uint64_t> in_off(n), out_off(n), dl(n);
  std::vector<uint32_t> len(n), slot(n), made(n);
  uint64_t room = 0;
  for (uint32_t i = 0; i < n; ++i) {
    in_off[i] = items[i].in_off;
    len[i] = items[i].len;
    slot[i] = items[i].p->slot;
    out_off[i] = room;
    room += align_up(xcg_zdeflate_bound(len[i]), 4);
  }
  std::vector<uint8_t> out(room ? room : 1);
  const uint8_t none = 0;
  const int rc = xcg_zdeflate_host(c->zd, h_in ? h_in : &none, in_off.data(), len.data(), slot.data(), n, nullptr,
                                   nullptr, out.data(), out_off.data(), made.data(), dl.data());
  if (rc != XCG_OK) return rc;
  for (uint32_t i = 0; i < n; ++i)
    if (int e = deliver(items[i].p, out.data() + out_off[i], made[i], dl[i])) return e;
  return XCG_OK;
}

// The same over wires that lie on the device, at d_in + in_off: xcg_zdeflate_batch, one readback of the
// lengths and deliver counts, a gather that packs the compressed bytes, one copy of those.
int deflate_device(xcg_codec* c, const std::vector<Item>& items, const uint8_t* d_in) {
  const uint32_t n = (uint32_t)items.size();
  if (n == 0) return XCG_OK;
  std::vector<uint64_t> in_off(n), out_off(n);
  std::vector<uint32_t> len(n), slot(n);
  uint64_t room = 0;
  for (uint32_t i = 0; i < n; ++i) {
    in_off[i] = items[i].in_off;
    len[i] = items[i].len;
    slot[i] = items[i].p->slot;
    out_off[i] = room;
    room += align_up(xcg_zdeflate_bound(len[i]), 256);
  }
  const size_t o_len = room, o_dl = align_up(o_len + 4ull * n, 256), o_end = align_up(o_dl + 8ull * n, 256);
  if (!c->mem.grow_bytes(&c->d_zout, &c->d_zout_cap, o_end, xcg::MEM_DEV) ||
      !c->mem.grow_bytes(&c->h_res, &c->h_res_cap, o_end - o_len, xcg::MEM_PINNED))
    return XCG_ENOMEM;
  int rc = xcg_zdeflate_batch(c->zd, d_in, in_off.data(), len.data(), slot.data(), n, c->d_zout, out_off.data(),
                              (uint32_t*)(c->d_zout + o_len), (uint64_t*)(c->d_zout + o_dl), c->st);
  if (rc != XCG_OK) return rc;
  if (hipMemcpyAsync(c->h_res, c->d_zout + o_len, o_end - o_len, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
      hipStreamSynchronize(c->st) != hipSuccess)
    return XCG_EHIP;
  const uint32_t* made = (const uint32_t*)c->h_res;
  const uint64_t* dl = (const uint64_t*)(c->h_res + (o_dl - o_len));
  // pack: slot i's made[i] bytes to pk_off[i]
  std::vector<uint64_t> pk_off(n);
  uint64_t total = 0;
  uint32_t longest = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (made[i] > xcg_zdeflate_bound(len[i])) return XCG_EHIP;
    pk_off[i] = total;
    total += made[i];
    longest = std::max(longest, made[i]);
  }
  if (total) {
    const size_t u_dst = align_up(8ull * n, 256), u_len = align_up(u_dst + 8ull * n, 256),
                 u_end = align_up(u_len + 4ull * n, 256);
    if (!c->mem.grow_bytes(&c->h_up, &c->h_up_cap, u_end, xcg::MEM_PINNED) ||
        !c->mem.grow_bytes(&c->d_up, &c->d_up_cap, u_end, xcg::MEM_DEV) ||
        !c->mem.grow_bytes(&c->d_pack, &c->d_pack_cap, (size_t)total, xcg::MEM_DEV) ||
        !c->mem.grow_bytes(&c->h_pack, &c->h_pack_cap, (size_t)total, xcg::MEM_PINNED))
      return XCG_ENOMEM;
    memcpy(c->h_up, out_off.data(), 8ull * n);
    memcpy(c->h_up + u_dst, pk_off.data(), 8ull * n);
    memcpy(c->h_up + u_len, made, 4ull * n);
    if (hipMemcpyAsync(c->d_up, c->h_up, u_end, hipMemcpyHostToDevice, c->st) != hipSuccess) return XCG_EHIP;
    rc = xcg_gather_pieces(c->enc, c->d_zout, (const uint64_t*)c->d_up, (const uint64_t*)(c->d_up + u_dst),
                           (const uint32_t*)(c->d_up + u_len), n, longest, c->d_pack, c->st);
    if (rc != XCG_OK) return rc;
    if (hipMemcpyAsync(c->h_pack, c->d_pack, total, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
        hipStreamSynchronize(c->st) != hipSuccess)
      return XCG_EHIP;
  }
  for (uint32_t i = 0; i < n; ++i)
    if (int e = deliver(items[i].p, c->h_pack + pk_off[i], made[i], dl[i])) return e;
  return XCG_OK;
}

// The pipes whose pair reported peer_eos: one empty consume (Z_FINISH) each, in a batch of its own
// (a stream appears at most once per batch), its bytes behind the call's to_peer.
int finish_streams(xcg_codec* c, xcg_codec_pipe* const* pipes, uint32_t n) {
  std::vector<Item> eos;
  for (uint32_t k = 0; k < n; ++k)
    if (pipes[k] && pipes[k]->peer_eos) eos.push_back(Item{pipes[k], 0, 0});
  return deflate_host(c, eos, nullptr);
}

// XCG_EINVAL of both _many calls: null arguments, pipes of different codecs, a pipe listed twice.
int check_pipes(xcg_codec_pipe* const* pipes, const uint8_t* const* data, const uint64_t* len, uint32_t n,
                const xcg_pipe_out* out) {
  if (!pipes || !data || !len || !out) return XCG_EINVAL;
  for (uint32_t k = 0; k < n; ++k)
    if (!pipes[k] || pipes[k]->c != pipes[0]->c || (len[k] && !data[k])) return XCG_EINVAL;
  std::vector<const xcg_codec_pipe*> s(pipes, pipes + n);
  std::sort(s.begin(), s.end(), std::less<const xcg_codec_pipe*>());
  if (std::adjacent_find(s.begin(), s.end()) != s.end()) return XCG_EINVAL;
  return XCG_OK;
}

struct Result {            // rc[k], and the call's return value: the first nonzero one
  int* rc;
  int first = XCG_OK;
  void set(uint32_t k, int v) {
    if (rc) rc[k] = v;
    if (v != XCG_OK && first == XCG_OK) first = v;
  }
};

}  // namespace

extern "C" {

int xcg_debug_set_codec_fused(int on) { return g_fused.exchange(on ? 1 : 0); }

void xcg_codec_debug_counts(uint64_t out[4]) {
  out[0] = g_fused_sends;
  out[1] = g_host_sends;
  out[2] = g_inflate_batches;
  out[3] = g_decode_batches;
}

int xcg_codec_create(xcg_ctx* enc, xcg_ctx* dec_or_parent, int connect, int compressor_level, uint32_t max_pipes,
                     xcg_codec** out) {
  if (!enc || !dec_or_parent || !out || max_pipes == 0 || compressor_level < -1 || compressor_level > 9)
    return XCG_EINVAL;
  *out = nullptr;
  xcg_codec* c = new xcg_codec;
  c->enc = enc;
  c->dec = dec_or_parent;
  c->connect = connect ? 1 : 0;
  c->level = compressor_level;
  c->max_pipes = max_pipes;
  c->device = xcg_ctx_device(enc);
  Guard g(c->device);
  int rc = XCG_OK;
  if (c->level >= 0) {
    rc = xcg_zdeflate_create(c->device, c->level, max_pipes, &c->zd);
    if (rc == XCG_OK) rc = xcg_zinflate_create(c->device, max_pipes, &c->zi);
    if (rc == XCG_OK && hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) != hipSuccess) rc = XCG_EHIP;
  }
  if (rc != XCG_OK) {
    xcg_codec_destroy(c);
    return rc;
  }
  for (uint32_t s = max_pipes; s-- > 0;) c->free_slots.push_back(s);   // (slot 0 goes first)
  *out = c;
  return XCG_OK;
}

void xcg_codec_destroy(xcg_codec* c) {
  if (!c) return;
  Guard g(c->device);
  if (c->st) (void)hipStreamSynchronize(c->st);
  if (c->zd) xcg_zdeflate_destroy(c->zd);
  if (c->zi) xcg_zinflate_destroy(c->zi);
  c->mem.release_all();
  if (c->st) (void)hipStreamDestroy(c->st);
  delete c;
}

int xcg_codec_pipe_create(xcg_codec* c, const uint8_t* uuid, xcg_codec_pipe** out) {
  if (!c || !uuid || !out) return XCG_EINVAL;
  *out = nullptr;
  if (c->free_slots.empty()) return XCG_ENOMEM;          // max_pipes pipes are alive
  const uint32_t slot = c->free_slots.back();
  int rc = XCG_OK;
  if (c->zd) {                                           // a fresh DeflatePipe / InflatePipe on the slot
    rc = xcg_zdeflate_reset(c->zd, slot);
    if (rc == XCG_OK) rc = xcg_zinflate_reset(c->zi, slot);
    if (rc != XCG_OK) return rc;
  }
  xcg_pipe* pair = nullptr;
  rc = c->connect ? xcg_pipe_create_connect(c->enc, c->dec, uuid, &pair) : xcg_pipe_create(c->enc, c->dec, uuid, &pair);
  if (rc != XCG_OK) return rc;
  c->free_slots.pop_back();
  xcg_codec_pipe* p = new xcg_codec_pipe;
  p->c = c;
  p->pair = pair;
  p->slot = slot;
  *out = p;
  return XCG_OK;
}

void xcg_codec_pipe_destroy(xcg_codec_pipe* p) {
  if (!p) return;
  xcg_pipe_destroy(p->pair);
  p->c->free_slots.push_back(p->slot);
  delete p;
}

xcg_pipe* xcg_codec_pipe_pair(const xcg_codec_pipe* p) { return p ? p->pair : nullptr; }

int xcg_codec_stats(const xcg_codec* c, uint64_t st[4]) {
  if (!c || !st) return XCG_EINVAL;
  memcpy(st, c->stats, sizeof c->stats);
  return XCG_OK;
}

int xcg_codec_send_many(xcg_codec_pipe* const* pipes, const uint8_t* const* data, const uint64_t* len, uint32_t n,
                        xcg_pipe_out* out, int* rc_out) {
  if (n == 0) return XCG_OK;
  if (int rc = check_pipes(pipes, data, len, n, out)) return rc;
  xcg_codec* c = pipes[0]->c;
  for (uint32_t k = 0; k < n; ++k) {
    if (xcg::pipe::sent_eos(pipes[k]->pair)) return XCG_EINVAL;
    if (c->level >= 0 && xcg::wire::worst_case(len[k], xcg_encode_bound) > xcg::zd::MAX_CALL_LEN) return XCG_EINVAL;
  }
  Guard g(c->device);
  Result res{rc_out};
  // the encoder step over the pipes that have not failed
  std::vector<uint32_t> live;
  std::vector<xcg_pipe*> pairs;
  std::vector<const uint8_t*> pd;
  std::vector<uint64_t> pl;
  for (uint32_t k = 0; k < n; ++k) {
    pipes[k]->begin();
    if (pipes[k]->failed) continue;
    live.push_back(k);
    pairs.push_back(pipes[k]->pair);
    pd.push_back(data[k]);
    pl.push_back(len[k]);
  }
  const uint32_t m = (uint32_t)live.size();
  const bool fused = c->level >= 0 && g_fused.load() != 0;
  if (m) {
    int rc = xcg::pipe::encode_check(pairs.data(), pd.data(), pl.data(), m);
    if (rc != XCG_OK) return rc;
    xcg::pipe::Encoded e;
    rc = xcg::pipe::encode_step(pairs.data(), pd.data(), pl.data(), m, fused, &e);
    if (rc != XCG_OK) return rc;
    std::vector<Item> items(m);
    if (fused) {
      std::vector<xcg::wire::PipeIn> in(m);
      for (uint32_t i = 0; i < m; ++i)
        in[i] = xcg::wire::PipeIn{e.hello[i] != 0, e.eos[i] != 0, xcg::pipe::uuid_of(pairs[i]), e.first[i],
                                  e.first[i + 1] - e.first[i]};
      const xcg::wire::WirePlan plan(in.data(), m, e.enc_off.data(), e.enc_len.data());
      const xcg::wire::WireUpload up(plan);
      if (!c->mem.grow_bytes(&c->h_up, &c->h_up_cap, up.end, xcg::MEM_PINNED) ||
          !c->mem.grow_bytes(&c->d_up, &c->d_up_cap, up.end, xcg::MEM_DEV) ||
          !c->mem.grow_bytes(&c->d_wire, &c->d_wire_cap, (size_t)plan.total + 256, xcg::MEM_DEV))
        return XCG_ENOMEM;
      // piece sources relative to the upload block on the device: its own literals, and the encodings
      // in the encoder context's staging (another allocation: wrapping integer arithmetic)
      up.fill(plan, c->h_up, up.lit, (uint64_t)((uintptr_t)e.d_enc - (uintptr_t)c->d_up));
      if (hipMemcpyAsync(c->d_up, c->h_up, up.end, hipMemcpyHostToDevice, c->st) != hipSuccess) return XCG_EHIP;
      rc = xcg_gather_pieces(c->enc, c->d_up, (const uint64_t*)(c->d_up + up.src), (const uint64_t*)(c->d_up + up.dst),
                             (const uint32_t*)(c->d_up + up.len), (uint32_t)plan.pieces.size(), plan.max_piece,
                             c->d_wire, c->st);
      if (rc != XCG_OK) return rc;
      for (uint32_t i = 0; i < m; ++i) items[i] = Item{pipes[live[i]], plan.wire_off[i], plan.wire_len[i]};
      rc = deflate_device(c, items, c->d_wire);
      if (rc != XCG_OK) return rc;
      ++g_fused_sends;
    } else {
      std::vector<uint8_t> wires;
      for (uint32_t i = 0; i < m; ++i) {
        xcg::pipe::emit_wire(pairs[i], e, i);
        xcg_pipe_out o;
        xcg::pipe::outputs(pairs[i], &o);
        if (c->level < 0) {                              // no compressor: the pair's bytes
          xcg_codec_pipe* p = pipes[live[i]];
          p->to_peer.assign(o.to_peer, o.to_peer + o.to_peer_len);
          c->stats[1] += o.to_peer_len;
          continue;
        }
        items[i] = Item{pipes[live[i]], wires.size(), (uint32_t)o.to_peer_len};
        wires.insert(wires.end(), o.to_peer, o.to_peer + o.to_peer_len);
      }
      if (c->level >= 0) {
        rc = deflate_host(c, items, wires.data());
        if (rc != XCG_OK) return rc;
        ++g_host_sends;
      }
    }
  }
  for (uint32_t k = 0; k < n; ++k) {
    xcg_codec_pipe* p = pipes[k];
    if (!p->failed) c->stats[0] += len[k];
    res.set(k, p->failed ? XCG_EPROTO : XCG_OK);
    p->finish(out + k);
  }
  return res.first;
}

int xcg_codec_receive_many(xcg_codec_pipe* const* pipes, const uint8_t* const* data, const uint64_t* len, uint32_t n,
                           xcg_pipe_out* out, int* rc_out) {
  if (n == 0) return XCG_OK;
  if (int rc = check_pipes(pipes, data, len, n, out)) return rc;
  xcg_codec* c = pipes[0]->c;
  if (c->level >= 0)
    for (uint32_t k = 0; k < n; ++k)
      if (len[k] > xcg::zd::INFLATE_MAX_CALL_LEN) return XCG_EINVAL;
  Guard g(c->device);
  Result res{rc_out};
  std::vector<int> rcs(n, XCG_OK);
  for (uint32_t k = 0; k < n; ++k) {
    pipes[k]->begin();
    if (pipes[k]->failed) rcs[k] = XCG_EPROTO;
    else c->stats[2] += len[k];
  }
  // 1. one InflatePipe::consume per pipe: W[k], status[k]
  std::vector<std::vector<uint8_t>> W(n);
  std::vector<int32_t> status(n, 0);
  if (c->level >= 0) {
    std::vector<uint32_t> todo;
    for (uint32_t k = 0; k < n; ++k)
      if (!pipes[k]->failed) todo.push_back(k);
    uint32_t grow = 1;                                   // calls that report -2 are repeated with more room
    while (!todo.empty()) {
      const uint32_t m = (uint32_t)todo.size();
      std::vector<uint64_t> in_off(m), out_off(m);
      std::vector<uint32_t> il(m), slot(m), cap(m), ol(m);
      std::vector<int32_t> st(m);
      std::vector<uint8_t> in;
      uint64_t room = 0;
      for (uint32_t i = 0; i < m; ++i) {
        const uint32_t k = todo[i];
        in_off[i] = in.size();
        il[i] = (uint32_t)len[k];
        if (len[k]) in.insert(in.end(), data[k], data[k] + len[k]);
        slot[i] = pipes[k]->slot;
        const uint64_t want = (4ull * len[k] + 65536) * grow;
        if (want > 0xffffffffu - 4) return XCG_EOVERFLOW;
        cap[i] = (uint32_t)want;
        out_off[i] = room;
        room += align_up(cap[i], 4);
      }
      if (in.empty()) in.push_back(0);
      std::vector<uint8_t> o(room);
      const int rc = xcg_zinflate_host(c->zi, in.data(), in_off.data(), il.data(), slot.data(), m, o.data(),
                                       out_off.data(), cap.data(), ol.data(), st.data());
      if (rc != XCG_OK) return rc;
      ++g_inflate_batches;
      std::vector<uint32_t> again;
      for (uint32_t i = 0; i < m; ++i) {
        const uint32_t k = todo[i];
        if (st[i] == -2) {
          again.push_back(k);
          continue;
        }
        status[k] = st[i];
        W[k].assign(o.begin() + (ptrdiff_t)out_off[i], o.begin() + (ptrdiff_t)(out_off[i] + ol[i]));
      }
      todo.swap(again);
      grow *= 4;
    }
  } else {
    for (uint32_t k = 0; k < n; ++k) {
      if (len[k]) W[k].assign(data[k], data[k] + len[k]);
      status[k] = len[k] ? 0 : 1;                        // (no compressor: an empty receive is the pair's)
    }
  }
  // 2. what reaches the pairs: one xcg_pipe_decoder_consume_many, then the empty consumes behind a
  //    produce_eos that carried bytes
  std::vector<uint32_t> served, closing;
  std::vector<xcg_pipe*> pairs;
  std::vector<const uint8_t*> pd;
  std::vector<uint64_t> pl;
  for (uint32_t k = 0; k < n; ++k) {
    xcg_codec_pipe* p = pipes[k];
    if (p->failed) continue;
    if (status[k] == -1) {                               // produce_error: nothing reaches the pair
      p->failed = true;
      rcs[k] = XCG_EPROTO;
      continue;
    }
    const bool eos = len[k] == 0 && status[k] == 1;
    if (W[k].empty() && !eos) continue;
    served.push_back(k);
    pairs.push_back(p->pair);
    pd.push_back(W[k].empty() ? nullptr : W[k].data());
    pl.push_back(W[k].size());
    if (eos && !W[k].empty()) closing.push_back(k);
  }
  std::vector<Item> replies;
  std::vector<uint8_t> wires;
  if (!served.empty()) {
    const uint32_t m = (uint32_t)served.size();
    std::vector<xcg_pipe_out> po(m);
    std::vector<int> prc(m, 1);                          // (1: not reached)
    const int rc = xcg_pipe_decoder_consume_many(pairs.data(), pd.data(), pl.data(), m, po.data(), prc.data());
    ++g_decode_batches;
    for (uint32_t i = 0; i < m; ++i)
      if (prc[i] == 1) return rc != XCG_OK ? rc : XCG_EHIP;   // an engine failure: at once
    for (uint32_t i = 0; i < m; ++i) {
      const uint32_t k = served[i];
      rcs[k] = prc[i];
      if (prc[i] != XCG_OK) continue;                    // (a failing pair call produces nothing)
      xcg_codec_pipe* p = pipes[k];
      p->take(po[i]);
      if (!po[i].to_peer_len) continue;
      if (c->level < 0) {
        p->to_peer.assign(po[i].to_peer, po[i].to_peer + po[i].to_peer_len);
        c->stats[1] += po[i].to_peer_len;
        continue;
      }
      replies.push_back(Item{p, wires.size(), (uint32_t)po[i].to_peer_len});
      wires.insert(wires.end(), po[i].to_peer, po[i].to_peer + po[i].to_peer_len);
    }
  }
  // 3. the replies through each pipe's deflate stream: one batch
  if (int rc = deflate_host(c, replies, wires.data())) return rc;
  // (a produce_eos behind bytes: the pair's empty consume follows them; its outputs join the call's)
  replies.clear();
  wires.clear();
  for (uint32_t k : closing) {
    xcg_codec_pipe* p = pipes[k];
    if (rcs[k] != XCG_OK) continue;
    p->to_local.assign(p->local, p->local + p->local_len);
    xcg_pipe_out o;
    const int rc = xcg_pipe_decoder_consume(p->pair, nullptr, 0, &o);
    if (rc != XCG_OK) {
      rcs[k] = rc;
      continue;
    }
    p->to_local.insert(p->to_local.end(), o.to_local, o.to_local + o.to_local_len);
    p->take(o);
    p->local = p->to_local.data();
    p->local_len = p->to_local.size();
    if (!o.to_peer_len) continue;
    if (c->level < 0) {
      p->to_peer.insert(p->to_peer.end(), o.to_peer, o.to_peer + o.to_peer_len);
      c->stats[1] += o.to_peer_len;
      continue;
    }
    replies.push_back(Item{p, wires.size(), (uint32_t)o.to_peer_len});
    wires.insert(wires.end(), o.to_peer, o.to_peer + o.to_peer_len);
  }
  if (int rc = deflate_host(c, replies, wires.data())) return rc;
  // 4. encoder_produce_eos: Z_FINISH
  if (c->level >= 0)
    if (int rc = finish_streams(c, pipes, n)) return rc;
  for (uint32_t k = 0; k < n; ++k) {
    xcg_codec_pipe* p = pipes[k];
    if (rcs[k] != XCG_OK) p->begin();
    c->stats[3] += p->local_len;
    res.set(k, rcs[k]);
    p->finish(out + k);
  }
  return res.first;
}

}  // extern "C"
