// XCodecPipePair protocol layer on the MI355X engine (host C++ over the C ABI).
//
// Restates xcodec/xcodec_pipe_pair.cc (encoder_consume :549-642,
// decoder_consume :68-166, decoder_decode :168-433, decoder_decode_data
// :435-547) and the wire ops of xcodec/xcodec_pipe_protocol.h:
//   <HELLO> 0xFF len[u8] uuid[len]     <FRAME> 0x02 len[BE32] data[len]
//   <ASK>   0xF0 count[BE16] hash[BE64 x count]
//   <LEARN> 0xF1 count[BE16] segment[2048 x count]
//   <ADVANCE> 0x01 count[BE32]   <EOS> 0xFC   <EOS_ACK> 0xFB
// Frames carry one XCodecEncoder::encode() call over <= XCODEC_PIPE_MAX_FRAME/2
// input bytes; the encoder keeps, per unacknowledged frame, the segments its
// REFs name (its refmap) to answer <ASK> with <LEARN>; the decoder decodes the
// concatenated frame bytes, asks for unknown hashes, and acknowledges
// finished frames with <ADVANCE>.  The codec work -- every encode and decode --
// runs on the GPU through xcg_encode_host_refmap / xcg_decode_host; pipes that share
// an encoder context (one codec, one cache) can be encoded in one GPU batch
// (xcg_pipe_encoder_consume_many), and pipes that share a decoder context (one
// peer's cache) decoded in one (xcg_pipe_decoder_consume_many, over
// xcg_decode_host_windows, or xcg_decode_host_windows_bounded on a bounded or
// pair context: one BACKREF window per pipe; pipes that each stand
// alone on a peer's cache in one launch, xcg_decode_call_many), both in the order the
// reference's single event thread would have served them.  The encoder side is
// two halves the codec layer shares (xcg_pipe_step.h, xcg_codec.cpp): the
// encode of all frames with the pipes' state changes, and the wire's emission.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <deque>
#include <functional>
#include <memory>
#include <set>
#include <unordered_map>
#include <vector>

#include "../../include/xcgpu.h"
#include "xcg_args.h"
#include "xcg_pipe_step.h"

namespace {

constexpr uint8_t OP_HELLO = 0xff, OP_LEARN = 0xf1, OP_ASK = 0xf0, OP_EOS = 0xfc, OP_EOS_ACK = 0xfb,
                  OP_FRAME = 0x02, OP_ADVANCE = 0x01;            // xcodec_pipe_protocol.h:39-118
constexpr uint32_t MAX_FRAME = 1024 * 1024;                     // XCODEC_PIPE_MAX_FRAME, :61
constexpr uint32_t ASK_MAX = 512;                               // XCODEC_PIPE_ASK_MAX, :66
constexpr uint32_t SEG = XCG_SEGMENT_LENGTH;
constexpr uint32_t UUID_LEN = 36;                               // UUID_SIZE, common/uuid/uuid.h:33

void put_be16(std::vector<uint8_t>& o, uint16_t v) { o.push_back(v >> 8); o.push_back(v & 0xff); }
void put_be32(std::vector<uint8_t>& o, uint32_t v) {
  for (int s = 24; s >= 0; s -= 8) o.push_back((v >> s) & 0xff);
}
void put_be64(std::vector<uint8_t>& o, uint64_t v) {
  for (int s = 56; s >= 0; s -= 8) o.push_back((v >> s) & 0xff);
}
uint64_t get_be(const uint8_t* p, int n) {
  uint64_t v = 0;
  for (int i = 0; i < n; ++i) v = (v << 8) | p[i];
  return v;
}

// XCodecHash::hash (xcodec/xcodec_hash.h:155-174) of a 2048-byte segment: a
// <LEARN> names no hash, the decoder derives it (xcodec_pipe_pair.cc:306).
uint64_t seg_hash(const uint8_t* d) {
  uint32_t s1 = 0, s2 = 0, b1 = 0, b2 = 0;
  for (uint32_t i = 0; i < SEG; ++i) {
    const uint32_t w = d[i] + 1u, f = d[i] ? (uint32_t)__builtin_ffs(d[i]) : 0u;
    s1 += w; s2 += (SEG - i) * w;
    b1 += f; b2 += (SEG - i) * f;
  }
  const uint64_t bits = (uint32_t)((b1 << 16) + b2), bytes = (uint32_t)((s1 << 20) + s2);
  return (bits << 36) + bytes;
}

bool uuid_ok(const uint8_t* u) {   // the string form UUID::decode accepts (8-4-4-4-12 hex)
  for (uint32_t i = 0; i < UUID_LEN; ++i) {
    const bool dash = i == 8 || i == 13 || i == 18 || i == 23;
    const uint8_t c = u[i];
    if (dash ? c != '-' : !((c >= '0' && c <= '9') || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F')))
      return false;
  }
  return true;
}

// Decoded size of enc[0..n) if every op resolves (xcodec_decoder.cc:73-185):
// literal and escaped bytes one each, EXTRACT / REF / BACKREF one segment
// each; the walk stops at an incomplete or unknown op, as the decoder does.
uint64_t decoded_bound(const uint8_t* enc, uint64_t n) {
  uint64_t i = 0, out = 0;
  while (i < n) {
    const uint8_t* m = (const uint8_t*)memchr(enc + i, 0xF1, n - i);
    if (!m) return out + (n - i);
    const uint64_t at = (uint64_t)(m - enc);
    out += at - i;
    i = at;
    if (i + 1 >= n) return out;
    const uint8_t op = enc[i + 1];
    if (op == 0x00) { out += 1; i += 2; }                       // escaped 0xF1
    else if (op == 0x01) { out += SEG; i += 2 + SEG; }          // EXTRACT
    else if (op == 0x02) { out += SEG; i += 10; }               // REF
    else if (op == 0x03) { out += SEG; i += 3; }                // BACKREF
    else return out;
  }
  return out;
}

}  // namespace

struct xcg_pipe {
  xcg_ctx* enc;
  xcg_ctx* dec;                    // (connecting pipes: set at <HELLO>)
  xcg_ctx* parent = nullptr;       // codec_->cache() of a connecting pipe
  xcg_window* win;                 // the decoder's BACKREF window (one per XCodecDecoder)
  uint8_t uuid[UUID_LEN];
  // encoder side
  bool encoder = false;            // encoder_ != NULL: <HELLO> sent
  bool encoder_sent_eos = false, encoder_sent_eos_ack = false, encoder_produced_eos = false;
  std::deque<std::unordered_map<uint64_t, std::vector<uint8_t>>> ref_frames;   // encoder_reference_frames_
  // decoder side
  bool decoder = false;            // decoder_ != NULL: <HELLO> received
  bool decoder_received_eos = false, decoder_sent_eos = false, decoder_received_eos_ack = false;
  std::vector<uint8_t> dbuf;       // decoder_buffer_
  std::vector<uint8_t> fbuf;       // decoder_frame_buffer_
  std::deque<uint32_t> flens;      // decoder_frame_lengths_
  std::set<uint64_t> unknown;      // decoder_unknown_hashes_
  // this call's outputs
  std::vector<uint8_t> to_peer, to_local;
  int local_eos = 0, peer_eos = 0;

  void begin() {
    to_peer.clear();
    to_local.clear();
    local_eos = peer_eos = 0;
  }
  void finish(xcg_pipe_out* o) const {
    if (!o) return;
    o->to_peer = to_peer.data();
    o->to_peer_len = to_peer.size();
    o->to_local = to_local.data();
    o->to_local_len = to_local.size();
    o->local_eos = local_eos;
    o->peer_eos = peer_eos;
  }
  int decode_ops();
  void ack_eos();
  int decode_data();
  int apply_decoded(int32_t st, uint64_t cons, const uint8_t* out, uint64_t out_len, const uint64_t* unk,
                    uint32_t nunk);
  void settle(int rc);
};

// decoder_decode (:168-433): process pipe ops until the buffer is empty or an
// op is incomplete.  XCG_EPROTO = decoder_error().
int xcg_pipe::decode_ops() {
  size_t i = 0;
  int rc = XCG_OK;
  while (i < dbuf.size()) {
    const uint8_t* b = dbuf.data() + i;
    const size_t avail = dbuf.size() - i;
    const uint8_t op = b[0];
    if (op == OP_HELLO) {
      if (decoder) { rc = XCG_EPROTO; break; }                       // <HELLO> twice
      if (avail < 2) break;
      const uint8_t len = b[1];
      if (avail < 2u + len) break;
      if (len != UUID_LEN || !uuid_ok(b + 2)) { rc = XCG_EPROTO; break; }
      if (parent) {                                                  // XCodecCache::connect(uuid, codec cache)
        char u[UUID_LEN + 1];
        memcpy(u, b + 2, UUID_LEN);
        u[UUID_LEN] = 0;
        xcg_ctx* c = nullptr;
        rc = xcg_ctx_connect_hold(parent, u, &c);                    // (held until xcg_pipe_destroy)
        if (rc != XCG_OK) break;
        rc = xcg_window_create(c, &win);
        if (rc != XCG_OK) {
          xcg_registry_release(c);
          break;
        }
        dec = c;
      }
      decoder = true;
      i += 2 + len;
    } else if (op == OP_ASK) {
      if (!encoder) { rc = XCG_EPROTO; break; }
      if (avail < 3) break;
      const uint32_t count = (uint32_t)get_be(b + 1, 2);
      if (count == 0 || count > ASK_MAX) { rc = XCG_EPROTO; break; }
      if (avail < 3 + 8ull * count) break;
      std::vector<uint8_t> learn;
      learn.push_back(OP_LEARN);
      put_be16(learn, (uint16_t)count);
      for (uint32_t k = 0; k < count && rc == XCG_OK; ++k) {
        const uint64_t h = get_be(b + 3 + 8 * k, 8);
        if (ref_frames.empty()) { rc = XCG_EPROTO; break; }          // all frames advanced
        bool found = false;
        for (const auto& rm : ref_frames) {
          auto it = rm.find(h);
          if (it == rm.end()) continue;
          learn.insert(learn.end(), it->second.begin(), it->second.end());
          found = true;
          break;
        }
        if (!found) rc = XCG_EPROTO;                                  // in no reference frame
      }
      if (rc != XCG_OK) break;
      to_peer.insert(to_peer.end(), learn.begin(), learn.end());
      i += 3 + 8ull * count;
    } else if (op == OP_LEARN) {
      if (!decoder) { rc = XCG_EPROTO; break; }
      if (avail < 3) break;
      const uint32_t count = (uint32_t)get_be(b + 1, 2);
      if (count == 0 || count > ASK_MAX) { rc = XCG_EPROTO; break; }
      if (avail < 3 + (size_t)SEG * count) break;
      // The segments up to the first gratuitous one are learned -- lookup: equal
      // -> redundant; else replace / enter (:311-327) -- in one batched call; a
      // pair learns segment by segment (its disk level, xcg_cache_enter_host).
      const bool pair = xcg_pair_xuid(dec) >= 0;
      uint32_t accepted = 0;
      for (; accepted < count; ++accepted) {
        const uint8_t* seg = b + 3 + (size_t)SEG * accepted;
        const uint64_t h = seg_hash(seg);
        if (!unknown.erase(h)) { rc = XCG_EPROTO; break; }           // gratuitous <LEARN>
        if (pair) {
          const int e = xcg_cache_enter_host(dec, h, seg);
          if (e != XCG_OK) { rc = e; break; }
        }
      }
      if (!pair && accepted) {
        const int e = xcg_cache_learn_host(dec, b + 3, accepted, nullptr);
        if (e != XCG_OK) rc = e;
      }
      if (rc != XCG_OK) break;
      i += 3 + (size_t)SEG * count;
    } else if (op == OP_EOS) {
      if (decoder_received_eos) { rc = XCG_EPROTO; break; }
      decoder_received_eos = true;
      i += 1;
    } else if (op == OP_EOS_ACK) {
      if (!encoder_sent_eos || decoder_received_eos_ack) { rc = XCG_EPROTO; break; }
      decoder_received_eos_ack = true;
      i += 1;
    } else if (op == OP_FRAME) {
      if (!decoder) { rc = XCG_EPROTO; break; }
      if (avail < 5) break;
      const uint32_t len = (uint32_t)get_be(b + 1, 4);
      if (len == 0 || len > MAX_FRAME) { rc = XCG_EPROTO; break; }
      if (avail < 5ull + len) break;
      fbuf.insert(fbuf.end(), b + 5, b + 5 + len);
      flens.push_back(len);
      i += 5ull + len;
    } else if (op == OP_ADVANCE) {
      if (!encoder) { rc = XCG_EPROTO; break; }
      if (avail < 5) break;
      const uint32_t count = (uint32_t)get_be(b + 1, 4);
      if (count == 0 || count > ref_frames.size()) { rc = XCG_EPROTO; break; }
      for (uint32_t k = 0; k < count; ++k) ref_frames.pop_front();   // encoder_reference_frame_advance
      i += 5;
    } else {
      rc = XCG_EPROTO;                                               // unsupported operation
      break;
    }
  }
  dbuf.erase(dbuf.begin(), dbuf.begin() + (ptrdiff_t)i);
  return rc;
}

// decoder_decode_data (:435-547): decode the buffered frame bytes on the GPU.
void xcg_pipe::ack_eos() {
  if (decoder_received_eos && !encoder_sent_eos_ack) {
    to_peer.push_back(OP_EOS_ACK);
    encoder_sent_eos_ack = true;
  }
}

int xcg_pipe::decode_data() {
  if (fbuf.empty()) {
    ack_eos();
    return XCG_OK;
  }
  // One decode() call over everything buffered, into an output sized from
  // the ops themselves (not filled: the decode writes what it returns).
  const uint64_t off = 0;
  const uint32_t len = (uint32_t)fbuf.size();
  uint64_t oo = 0, ol = 0, cons = 0;
  int32_t st = 0;
  std::vector<uint64_t> unk(1u << 16);
  uint32_t nunk = 0;
  const uint64_t cap = decoded_bound(fbuf.data(), len) + 4096;
  std::unique_ptr<uint8_t[]> out(new uint8_t[cap]);
  int rc = xcg_decode_set_window(dec, win);
  if (rc == XCG_OK)
    rc = xcg_decode_host(dec, fbuf.data(), len, &off, &len, 1, out.get(), cap, &oo, &ol, &st, &cons,
                         unk.data(), (uint32_t)unk.size(), &nunk);
  xcg_decode_set_window(dec, nullptr);
  if (rc != XCG_OK) return rc;
  return apply_decoded(st, cons, out.get() + oo, ol, unk.data(), nunk);
}

// What decoder_decode_data does with a decode() call's result: <ADVANCE>, the
// decoded bytes, the unknown hashes and their <ASK>s.  (The single call above
// and xcg_pipe_decoder_consume_many's batch both end here.)
int xcg_pipe::apply_decoded(int32_t st, uint64_t cons, const uint8_t* out, uint64_t out_len, const uint64_t* unk,
                            uint32_t nunk) {
  if (st < 0) return XCG_EPROTO;                                     // decode() returned false
  // <ADVANCE> for every frame consumed in full (:460-490)
  uint64_t consumed = cons;
  if (consumed) {
    uint32_t adv = 0;
    while (consumed) {
      const uint32_t first = flens.front();
      if (consumed < first) {
        flens.front() = first - (uint32_t)consumed;
        break;
      }
      consumed -= first;
      ++adv;
      flens.pop_front();
    }
    if (adv) {
      to_peer.push_back(OP_ADVANCE);
      put_be32(to_peer, adv);
    }
    fbuf.erase(fbuf.begin(), fbuf.begin() + (ptrdiff_t)cons);
  }
  to_local.insert(to_local.end(), out, out + out_len);
  for (uint32_t k = 0; k < nunk; ++k) unknown.insert(unk[k]);
  // <ASK>s in groups of ASK_MAX (:510-545)
  std::vector<uint64_t> hs(unknown.begin(), unknown.end());
  for (size_t a = 0; a < hs.size(); a += ASK_MAX) {
    const size_t c = std::min<size_t>(ASK_MAX, hs.size() - a);
    to_peer.push_back(OP_ASK);
    put_be16(to_peer, (uint16_t)c);
    for (size_t k = 0; k < c; ++k) put_be64(to_peer, hs[a + k]);
  }
  return XCG_OK;
}

// The end of decoder_consume (:125-159): with everything buffered consumed,
// the EOS hand-overs.
void xcg_pipe::settle(int rc) {
  if (rc != XCG_OK || !dbuf.empty() || !fbuf.empty()) return;
  if (decoder_received_eos && !decoder_sent_eos && unknown.empty()) {
    local_eos = 1;                                       // decoder_produce_eos (:125-138)
    decoder_sent_eos = true;
  }
  if (encoder_sent_eos_ack && decoder_received_eos_ack && !encoder_produced_eos) {
    peer_eos = 1;                                        // encoder_produce_eos (:150-159)
    encoder_produced_eos = true;
  }
}

namespace {
// Side-effect free: would decode_ops over the pipe's pending wire bytes (its
// buffer plus `data`) reach a <LEARN>?  The walk stops only where decode_ops
// certainly stops -- an op cut short, a length it refuses, an opcode it does
// not know -- and walks on over ops it may refuse for the pipe's state, so a
// <LEARN> it does not see is one decode_ops does not reach either.
bool reaches_learn(const uint8_t* b, size_t n) {
  size_t i = 0;
  while (i < n) {
    const size_t avail = n - i;
    const uint8_t op = b[i];
    if (op == OP_LEARN) return true;
    if (op == OP_HELLO) {
      if (avail < 2 || avail < 2u + b[i + 1]) return false;
      if (b[i + 1] != UUID_LEN || !uuid_ok(b + i + 2)) return false;
      i += 2 + UUID_LEN;
    } else if (op == OP_ASK) {
      if (avail < 3) return false;
      const uint32_t count = (uint32_t)get_be(b + i + 1, 2);
      if (count == 0 || count > ASK_MAX || avail < 3 + 8ull * count) return false;
      i += 3 + 8ull * count;
    } else if (op == OP_FRAME) {
      if (avail < 5) return false;
      const uint32_t len = (uint32_t)get_be(b + i + 1, 4);
      if (len == 0 || len > MAX_FRAME || avail < 5ull + len) return false;
      i += 5ull + len;
    } else if (op == OP_ADVANCE) {
      if (avail < 5 || get_be(b + i + 1, 4) == 0) return false;
      i += 5;
    } else if (op == OP_EOS || op == OP_EOS_ACK) {
      i += 1;
    } else {
      return false;
    }
  }
  return false;
}

// Diagnostics (xcg_pipe_debug_decode_many): batched decode calls made by
// xcg_pipe_decoder_consume_many and the chunks in them, process-wide.
std::atomic<uint64_t> g_many_calls{0}, g_many_chunks{0};
// (xcg_pipe_debug_decode_peers): xcg_decode_call_many calls made there, one
// pipe per peer cache, and the pipes in them.
std::atomic<uint64_t> g_peer_calls{0}, g_peer_pipes{0};
// Held pipes go up together from this many on; fewer take the single call.
// (Measured: scripts/pipe_peers_time.py)
constexpr uint32_t PEERS_MIN = 2;
constexpr size_t PEERS_MAX_CALL = 1u << 20;              // what xcg_decode_call_many decodes in its launch

// The shortest run on a bounded or on a pair context that goes up as a batch
// (xcg_decode_host_windows_bounded); shorter runs are the serial calls.
// (Measured: scripts/pipe_decode_many_time.py --cache bounded|pair,
// profiles/pipe_decode_many_bounded.txt; the rule and the numbers are in
// DESIGN.md section 9 item 4.)  xcg_pipe_debug_set_run_min overrides both, for
// that measurement and for tests of the batch at run lengths below them.
constexpr uint32_t BOUNDED_RUN_MIN = 2, PAIR_RUN_MIN = 2;
std::atomic<uint32_t> g_run_min{0};                      // (0: the constants)
uint32_t classified_run_min(const xcg_ctx* c) {
  const uint32_t set = g_run_min.load();
  if (set >= 2) return set;
  return xcg_pair_xuid(c) >= 0 ? PAIR_RUN_MIN : BOUNDED_RUN_MIN;
}

// A pipe xcg_pipe_decoder_consume_many may take into a run (see there).
bool plain(const xcg_pipe* p, const uint8_t* data, uint64_t len) {
  if (!p->dec) return false;
  if (len == 0) return true;                             // (peer closed: no byte is looked at)
  if (p->dbuf.empty()) return !reaches_learn(data, len);
  std::vector<uint8_t> all(p->dbuf);
  all.insert(all.end(), data, data + len);
  return !reaches_learn(all.data(), all.size());
}
}  // namespace

extern "C" {

int xcg_pipe_create(xcg_ctx* enc, xcg_ctx* dec, const uint8_t* uuid, xcg_pipe** out) {
  if (!enc || !dec || !uuid || !out || !uuid_ok(uuid)) return XCG_EINVAL;
  *out = nullptr;
  xcg_window* w = nullptr;
  const int rc = xcg_window_create(dec, &w);
  if (rc != XCG_OK) return rc;
  xcg_pipe* p = new xcg_pipe;
  p->enc = enc;
  p->dec = dec;
  p->win = w;
  memcpy(p->uuid, uuid, UUID_LEN);
  *out = p;
  return XCG_OK;
}

int xcg_pipe_create_connect(xcg_ctx* enc, xcg_ctx* parent, const uint8_t* uuid, xcg_pipe** out) {
  if (!enc || !parent || !uuid || !out || !uuid_ok(uuid)) return XCG_EINVAL;
  xcg_pipe* p = new xcg_pipe;
  p->enc = enc;
  p->dec = nullptr;
  p->parent = parent;
  p->win = nullptr;
  memcpy(p->uuid, uuid, UUID_LEN);
  *out = p;
  return XCG_OK;
}

xcg_ctx* xcg_pipe_decoder_ctx(const xcg_pipe* p) { return p ? p->dec : nullptr; }

void xcg_pipe_destroy(xcg_pipe* p) {
  if (!p) return;
  if (p->win) xcg_window_destroy(p->win);
  if (p->parent && p->dec) xcg_registry_release(p->dec);   // (a cleared registry's context goes now)
  delete p;
}

}  // extern "C"

// The two halves of xcg_pipe_encoder_consume_many (xcg_pipe_step.h).
namespace xcg {
namespace pipe {

int encode_check(xcg_pipe* const* pipes, const uint8_t* const* data, const uint64_t* len, uint32_t n) {
  if (!pipes || !data || !len) return XCG_EINVAL;
  for (uint32_t k = 0; k < n; ++k) {
    const xcg_pipe* p = pipes[k];
    if (!p || p->enc != pipes[0]->enc || p->encoder_sent_eos || (len[k] && !data[k])) return XCG_EINVAL;
  }
  return XCG_OK;
}

int encode_step(xcg_pipe* const* pipes, const uint8_t* const* data, const uint64_t* len, uint32_t n, bool on_device,
                Encoded* e) {
  xcg_ctx* enc = pipes[0]->enc;
  // Frames of every pipe's input, in order: <= MAX_FRAME / 2 bytes each
  // (:585-600), so a frame's encoding never exceeds MAX_FRAME.
  struct Frame { uint32_t pipe; uint64_t in_off; uint32_t len; };
  std::vector<Frame> frames;
  std::vector<uint64_t> base(n);
  uint64_t total = 0;
  e->first.assign(n + 1, 0);
  for (uint32_t k = 0; k < n; ++k) {
    base[k] = total;
    e->first[k] = (uint32_t)frames.size();
    for (uint64_t a = 0; a < len[k]; a += MAX_FRAME / 2)
      frames.push_back({k, total + a, (uint32_t)std::min<uint64_t>(MAX_FRAME / 2, len[k] - a)});
    total += len[k];
  }
  e->first[n] = (uint32_t)frames.size();
  std::vector<uint8_t> in(total ? total : 1);
  for (uint32_t k = 0; k < n; ++k)
    if (len[k]) memcpy(in.data() + base[k], data[k], len[k]);
  const uint32_t nf = (uint32_t)frames.size();
  std::vector<uint64_t> off(nf);
  std::vector<uint32_t> fl(nf);
  e->enc_off.assign(nf, 0);
  e->enc_len.assign(nf, 0);
  uint64_t cap = 0;
  for (uint32_t f = 0; f < nf; ++f) {
    off[f] = frames[f].in_off;
    fl[f] = frames[f].len;
    e->enc_off[f] = cap;
    cap += xcg_encode_bound(frames[f].len);
  }
  e->enc.clear();
  e->d_enc = nullptr;
  if (!on_device) e->enc.resize(cap ? cap : 1);
  // one GPU batch: successive encode() calls of one XCodecEncoder cache, and
  // each call's refmap as (hash, input offset) rows in std::map order.  The
  // window at a REF's offset equals the segment the REF names (find_reference
  // only emits a REF on byte equality, xcodec_encoder.cc:382-390), so a frame's
  // segments come from its own input.  Out-of-band declarations are no rows
  // (encode_declaration passes no refmap, :288-295; a null cache has none at
  // all), so an <ASK> for such a hash is a protocol error as in the reference
  // (xcodec_pipe_pair.cc:265-267).
  std::vector<uint64_t> rh((size_t)nf * XCG_REFMAP_MAX);
  std::vector<uint32_t> rp((size_t)nf * XCG_REFMAP_MAX), nref(nf);
  if (nf) {
    const int rc =
        on_device ? xcg_encode_host_refmap_device(enc, XCG_SEM_STREAM, in.data(), total, off.data(), fl.data(), nf, cap,
                                                  e->enc_off.data(), e->enc_len.data(), rh.data(), rp.data(),
                                                  XCG_REFMAP_MAX, nref.data(), &e->d_enc)
                  : xcg_encode_host_refmap(enc, XCG_SEM_STREAM, in.data(), total, off.data(), fl.data(), nf,
                                           e->enc.data(), e->enc.size(), e->enc_off.data(), e->enc_len.data(),
                                           rh.data(), rp.data(), XCG_REFMAP_MAX, nref.data());
    if (rc != XCG_OK) return rc;
    for (uint32_t f = 0; f < nf; ++f)
      for (uint32_t r = 0; r < nref[f] && r < XCG_REFMAP_MAX; ++r)
        if ((uint64_t)rp[(size_t)f * XCG_REFMAP_MAX + r] + SEG > fl[f])
          return XCG_EHIP;                               // (never: a REF stands for 2048 input bytes)
  }
  e->hello.assign(n, 0);
  e->eos.assign(n, 0);
  uint32_t f = 0;
  for (uint32_t k = 0; k < n; ++k) {
    xcg_pipe* p = pipes[k];
    p->begin();
    if (!p->encoder) {                                   // <HELLO> (:557-573)
      e->hello[k] = 1;
      p->encoder = true;
    }
    if (len[k] == 0) {                                   // <EOS> (:632-636)
      e->eos[k] = 1;
      p->encoder_sent_eos = true;
    }
    for (; f < nf && frames[f].pipe == k; ++f) {
      std::unordered_map<uint64_t, std::vector<uint8_t>> rm;
      const uint8_t* fin = in.data() + off[f];
      for (uint32_t r = 0; r < nref[f] && r < XCG_REFMAP_MAX; ++r) {
        const uint32_t at = rp[(size_t)f * XCG_REFMAP_MAX + r];
        rm.emplace(rh[(size_t)f * XCG_REFMAP_MAX + r], std::vector<uint8_t>(fin + at, fin + at + SEG));
      }
      p->ref_frames.push_back(std::move(rm));
    }
  }
  return XCG_OK;
}

void emit_wire(xcg_pipe* p, const Encoded& e, uint32_t k) {
  if (e.hello[k]) {
    p->to_peer.push_back(OP_HELLO);
    p->to_peer.push_back((uint8_t)UUID_LEN);
    p->to_peer.insert(p->to_peer.end(), p->uuid, p->uuid + UUID_LEN);
  }
  if (e.eos[k]) p->to_peer.push_back(OP_EOS);
  for (uint32_t f = e.first[k]; f < e.first[k + 1]; ++f) {
    p->to_peer.push_back(OP_FRAME);                      // (:620-628)
    put_be32(p->to_peer, (uint32_t)e.enc_len[f]);
    p->to_peer.insert(p->to_peer.end(), e.enc.begin() + (ptrdiff_t)e.enc_off[f],
                      e.enc.begin() + (ptrdiff_t)(e.enc_off[f] + e.enc_len[f]));
  }
}

const uint8_t* uuid_of(const xcg_pipe* p) { return p->uuid; }
bool sent_eos(const xcg_pipe* p) { return p->encoder_sent_eos; }
xcg_ctx* encoder_ctx(const xcg_pipe* p) { return p->enc; }
void outputs(const xcg_pipe* p, xcg_pipe_out* o) { p->finish(o); }

}  // namespace pipe
}  // namespace xcg

extern "C" {

int xcg_pipe_encoder_consume_many(xcg_pipe* const* pipes, const uint8_t* const* data, const uint64_t* len,
                                  uint32_t n, xcg_pipe_out* out) {
  if (n == 0) return XCG_OK;
  int rc = xcg::pipe::encode_check(pipes, data, len, n);
  if (rc != XCG_OK) return rc;
  xcg::pipe::Encoded e;
  rc = xcg::pipe::encode_step(pipes, data, len, n, false, &e);
  if (rc != XCG_OK) return rc;
  for (uint32_t k = 0; k < n; ++k) {
    xcg::pipe::emit_wire(pipes[k], e, k);
    if (out) pipes[k]->finish(out + k);
  }
  return XCG_OK;
}

int xcg_pipe_encoder_consume(xcg_pipe* p, const uint8_t* data, uint64_t len, xcg_pipe_out* out) {
  if (!p) return XCG_EINVAL;
  return xcg_pipe_encoder_consume_many(&p, &data, &len, 1, out);
}

int xcg_pipe_decoder_consume(xcg_pipe* p, const uint8_t* data, uint64_t len, xcg_pipe_out* out) {
  if (!p || (len && !data)) return XCG_EINVAL;
  p->begin();
  int rc = XCG_OK;
  if (len == 0) {                                        // peer closed (:72-87)
    if (!p->decoder_sent_eos) {
      p->decoder_sent_eos = true;
      p->local_eos = 1;
    }
    p->finish(out);
    return XCG_OK;
  }
  p->dbuf.insert(p->dbuf.end(), data, data + len);
  rc = p->decode_ops();
  if (rc == XCG_OK && p->unknown.empty()) rc = p->decode_data();
  p->settle(rc);
  p->finish(out);
  return rc;
}

// xcg_pipe_decoder_consume for every pipe in order, with the decode() calls of
// consecutive pipes on one decoder context in one GPU batch.
//
// A pipe is *plain* when its pending wire bytes hold no <LEARN>, it decodes on
// a context it has already (a connecting pipe past its <HELLO>): its
// decode_ops touches no decoder cache (only a <LEARN> enters one there), so it
// can run before
// the pipes in front of it have decoded.  A run is a maximal sequence of
// consecutive plain pipes on one context; each of its pipes brings at most one
// chunk, its frame buffer, and the run is one xcg_decode_host_windows call over
// the pipes' windows.  The batch has one stop point: the pipes before it are
// done, the stopped pipe takes its consumed prefix and -- blocked on a REF --
// the single call once more for decode_skim's set (that call blocks on its
// first op: it consumes and declares nothing), and the pipes behind it are
// the next batch.  Every other pipe is the serial call.
//
// On a bounded or pair context the batch is xcg_decode_host_windows_bounded,
// for runs of classified_run_min() pipes or more (shorter ones, a run of one
// included, are the serial calls).  That call may refuse a batch as a whole
// (XCG_ENOTSUP, nothing changed): the first half of the pending pipes is then
// presented again, down to a single pipe by decode_data().  The call makes no
// lookup behind its stop point, and the stopped pipe's decode_data() -- which
// blocks on its first op -- does the skim with its cache effects.
//
// A run of ONE -- a hub's turn: many peers, a pipe each -- runs its ops at once
// and, if that leaves frame bytes to decode (no unknown hash outstanding, at
// most 1 MiB buffered), is *held*: its decode() waits.  A held pipe decodes on
// an unbounded context no other unfinished pipe of the call uses, its
// decode_ops touched no cache, and pipes on distinct unbounded contexts share
// no decoder state (cache, window and buffers are per context or per pipe), so
// the held calls may run in any order, and together.  The held set is flushed
// before a later pipe whose context is in it, before a connecting pipe that
// has no context yet (it may connect to one of them) and at the end: one pipe
// by decode_data(), PEERS_MIN or more by one xcg_decode_call_many over the
// pipes' windows and frame buffers, whose per-call results (decode_skim's set
// included: no second call) end in apply_decoded as the single call's do.
int xcg_pipe_decoder_consume_many(xcg_pipe* const* pipes, const uint8_t* const* data, const uint64_t* len,
                                  uint32_t n, xcg_pipe_out* out, int* rc_out) {
  if (n == 0) return XCG_OK;
  if (!pipes || !data || !len) return XCG_EINVAL;
  for (uint32_t k = 0; k < n; ++k)
    if (!pipes[k] || (len[k] && !data[k])) return XCG_EINVAL;
  {
    std::vector<const xcg_pipe*> s(pipes, pipes + n);
    std::sort(s.begin(), s.end(), std::less<const xcg_pipe*>());
    if (std::adjacent_find(s.begin(), s.end()) != s.end()) return XCG_EINVAL;   // a pipe listed twice
  }
  std::vector<int> rcs(n, XCG_OK);                       // (held pipes finish out of order)
  const auto done = [&](uint32_t k, int rc) {
    if (rc_out) rc_out[k] = rc;
    rcs[k] = rc;
    if (out) pipes[k]->finish(out + k);
  };
  const auto serial = [&](uint32_t k) {
    done(k, xcg_pipe_decoder_consume(pipes[k], data[k], len[k], out ? out + k : nullptr));
  };
  // The held set: pipes whose ops are done and whose decode() waits for the
  // flush, each on a context of its own.
  std::vector<uint32_t> held;
  const auto is_held = [&](const xcg_ctx* c) {
    for (const uint32_t h : held)
      if (pipes[h]->dec == c) return true;
    return false;
  };
  const auto flush = [&]() -> int {
    const uint32_t m = (uint32_t)held.size();
    if (m < PEERS_MIN) {                                 // the single call
      for (const uint32_t h : held) {
        xcg_pipe* p = pipes[h];
        const int rc = p->decode_data();
        p->settle(rc);
        done(h, rc);
      }
      held.clear();
      return XCG_OK;
    }
    constexpr uint32_t UCAP = 1u << 16;                  // (decode_data's)
    std::vector<xcg_ctx*> cs(m);
    std::vector<xcg_window*> ws(m);
    std::vector<const uint8_t*> in(m);
    std::vector<uint32_t> il(m), ucap(m, UCAP), nunk(m);
    std::vector<uint8_t*> op(m);
    std::vector<uint64_t> cap(m), ol(m), cons(m);
    std::vector<uint64_t*> up(m);
    std::vector<int32_t> st(m);
    std::vector<int> crc(m);
    uint64_t total = 0;
    for (uint32_t i = 0; i < m; ++i) {
      const xcg_pipe* p = pipes[held[i]];
      cs[i] = p->dec;
      ws[i] = p->win;
      in[i] = p->fbuf.data();
      il[i] = (uint32_t)p->fbuf.size();
      cap[i] = decoded_bound(in[i], il[i]) + 4096;
      total += cap[i];
    }
    std::unique_ptr<uint8_t[]> dout(new uint8_t[total]);
    std::unique_ptr<uint64_t[]> unk(new uint64_t[(size_t)m * UCAP]);   // (not filled: the calls write what they count)
    total = 0;
    for (uint32_t i = 0; i < m; ++i) {
      op[i] = dout.get() + total;
      total += cap[i];
      up[i] = unk.get() + (size_t)i * UCAP;
    }
    const int brc = xcg_decode_call_many(cs.data(), ws.data(), in.data(), il.data(), op.data(), cap.data(), m,
                                         ol.data(), cons.data(), st.data(), up.data(), ucap.data(), nunk.data(),
                                         nullptr, nullptr, nullptr, crc.data());
    if (brc != XCG_OK) return brc;                       // an engine failure: at once
    ++g_peer_calls;
    g_peer_pipes += m;
    for (uint32_t i = 0; i < m; ++i) {
      xcg_pipe* p = pipes[held[i]];
      int rc = crc[i];
      if (rc == XCG_OK) rc = p->apply_decoded(st[i], cons[i], op[i], ol[i], up[i], nunk[i]);
      p->settle(rc);
      done(held[i], rc);
    }
    held.clear();
    return XCG_OK;
  };
  const auto result = [&]() {
    for (uint32_t j = 0; j < n; ++j)
      if (rcs[j] != XCG_OK) return rcs[j];
    return (int)XCG_OK;
  };
  uint32_t k = 0;
  while (k < n) {
    xcg_ctx* const ctx = pipes[k]->dec;
    // a pipe of a held context, or one that may connect to one: the held calls first
    if (!held.empty() && (!ctx || is_held(ctx))) {
      const int frc = flush();
      if (frc != XCG_OK) return frc;
    }
    uint32_t e = k;
    while (e < n && pipes[e]->dec == ctx && plain(pipes[e], data[e], len[e])) ++e;
    const bool classified = ctx && !xcg_ctx_unbounded(ctx);
    if (classified && e > k && e - k < classified_run_min(ctx)) {   // (the held path is the unbounded contexts')
      for (; k < e; ++k) serial(k);
      continue;
    }
    if (e - k == 1) {
      // a run of one: its ops now; its decode() joins the held set
      xcg_pipe* p = pipes[k];
      p->begin();
      if (len[k] == 0) {                                 // peer closed (:72-87)
        if (!p->decoder_sent_eos) {
          p->decoder_sent_eos = true;
          p->local_eos = 1;
        }
        done(k++, XCG_OK);
        continue;
      }
      p->dbuf.insert(p->dbuf.end(), data[k], data[k] + len[k]);
      const int rc = p->decode_ops();
      if (rc == XCG_OK && p->unknown.empty() && !p->fbuf.empty() && p->fbuf.size() <= PEERS_MAX_CALL) {
        held.push_back(k++);
        continue;
      }
      int rc2 = rc;
      if (rc == XCG_OK && p->unknown.empty()) rc2 = p->decode_data();
      p->settle(rc2);
      done(k++, rc2);
      continue;
    }
    if (e - k < 2) {
      serial(k++);
      continue;
    }
    // the run [k, e): every pipe's ops first, then the chunks in batches
    std::vector<uint32_t> pending;                       // pipes with a chunk to decode
    for (uint32_t j = k; j < e; ++j) {
      xcg_pipe* p = pipes[j];
      p->begin();
      if (len[j] == 0) {                                 // peer closed (:72-87)
        if (!p->decoder_sent_eos) {
          p->decoder_sent_eos = true;
          p->local_eos = 1;
        }
        done(j, XCG_OK);
        continue;
      }
      p->dbuf.insert(p->dbuf.end(), data[j], data[j] + len[j]);
      const int rc = p->decode_ops();
      if (rc == XCG_OK && p->unknown.empty() && !p->fbuf.empty()) {
        pending.push_back(j);
        continue;
      }
      if (rc == XCG_OK && p->unknown.empty()) p->ack_eos();   // (decode_data with nothing buffered)
      p->settle(rc);
      done(j, rc);
    }
    uint32_t take = (uint32_t)pending.size();             // (less after a refusal: the first half again)
    while (!pending.empty()) {
      const uint32_t m = take;
      if (m == 1) {                                      // the single call
        xcg_pipe* p = pipes[pending[0]];
        const int rc = p->decode_data();
        p->settle(rc);
        done(pending[0], rc);
        pending.erase(pending.begin());
        take = (uint32_t)pending.size();
        continue;
      }
      std::vector<uint64_t> off(m), oo(m), ol(m), cons(m);
      std::vector<uint32_t> cl(m), cw(m);
      std::vector<int32_t> st(m);
      std::vector<xcg_window*> wins(m);
      uint64_t total = 0, cap = 4096;
      for (uint32_t i = 0; i < m; ++i) {
        const xcg_pipe* p = pipes[pending[i]];
        off[i] = total;
        cl[i] = (uint32_t)p->fbuf.size();
        cw[i] = i;
        wins[i] = p->win;
        total += cl[i];
        cap += decoded_bound(p->fbuf.data(), cl[i]);
      }
      std::vector<uint8_t> in(total);
      for (uint32_t i = 0; i < m; ++i) memcpy(in.data() + off[i], pipes[pending[i]]->fbuf.data(), cl[i]);
      std::unique_ptr<uint8_t[]> dout(new uint8_t[cap]);
      uint32_t stop = m;
      const auto call = classified ? xcg_decode_host_windows_bounded : xcg_decode_host_windows;
      const int brc = call(ctx, in.data(), total, off.data(), cl.data(), m, wins.data(), m, cw.data(), dout.get(), cap,
                           oo.data(), ol.data(), st.data(), cons.data(), &stop, nullptr);
      if (classified && brc == XCG_ENOTSUP) {            // refused as a whole: nothing has changed
        take = m / 2;
        continue;
      }
      if (brc != XCG_OK) return brc;                     // an engine failure: at once
      ++g_many_calls;
      g_many_chunks += m;
      const uint32_t upto = stop < m ? stop + 1 : m;
      for (uint32_t i = 0; i < upto; ++i) {
        xcg_pipe* p = pipes[pending[i]];
        int rc = p->apply_decoded(st[i], cons[i], dout.get() + oo[i], ol[i], nullptr, 0);
        if (rc == XCG_OK && st[i] == 1) rc = p->decode_data();   // blocked: decode_skim's set and the <ASK>s
        p->settle(rc);
        done(pending[i], rc);
      }
      pending.erase(pending.begin(), pending.begin() + upto);
      take = (uint32_t)pending.size();
    }
    k = e;
  }
  const int frc = flush();
  if (frc != XCG_OK) return frc;
  return result();
}

void xcg_pipe_debug_decode_many(uint64_t out[2]) {
  out[0] = g_many_calls;
  out[1] = g_many_chunks;
}

uint32_t xcg_pipe_debug_set_run_min(uint32_t n) { return g_run_min.exchange(n >= 2 ? n : 0u); }

void xcg_pipe_debug_decode_peers(uint64_t out[2]) {
  out[0] = g_peer_calls;
  out[1] = g_peer_pipes;
}

uint32_t xcg_pipe_pending_frames(const xcg_pipe* p) { return p ? (uint32_t)p->ref_frames.size() : 0u; }

}  // extern "C"
