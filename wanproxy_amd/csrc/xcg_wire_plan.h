// The codec send path's host plan (xcg_codec.cpp): from what the encoder step
// left -- per pipe whether <HELLO> and <EOS> go out and which frames, per frame
// where its encoding lies on the device and how long it is -- the piece list of
// every pipe's wire and each wire's place in one deflate-input buffer, as
// xcg_zdeflate_batch takes its inputs (d_in + h_in_off[i], h_len[i]).  A piece
// is either literal bytes the host writes (<HELLO>, <EOS>, the 5-byte <FRAME>
// headers; xcodec/xcodec_pipe_pair.cc:557-573, 620-628, 632-636) or a range of
// the encodings; neighbouring literals are one piece.  The literals and the
// three piece arrays go up in one block (WireUpload) and xcg_gather_pieces moves
// the bytes.  Offsets and counts only, no HIP:
// tests/native/wire_plan_harness.cc runs this on the CPU under sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

namespace xcg {
namespace wire {

constexpr uint8_t OP_HELLO = 0xff, OP_EOS = 0xfc, OP_FRAME = 0x02;   // xcodec_pipe_protocol.h:39-118
constexpr uint32_t UUID_LEN = 36;                                    // UUID_SIZE, common/uuid/uuid.h:33
constexpr uint32_t HELLO_LEN = 2 + UUID_LEN, FRAME_HEAD = 5;
constexpr uint32_t FRAME_IN = 512 * 1024;                            // XCODEC_PIPE_MAX_FRAME / 2 input bytes a frame

inline size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Frames of a consume of `len` input bytes.
inline uint64_t frames_of(uint64_t len) { return (len + FRAME_IN - 1) / FRAME_IN; }

// The longest wire a consume of `len` bytes can make: <HELLO> + <EOS> + for
// every frame its header and `bound(frame length)`, the encoder's output bound.
template <class Bound>
uint64_t worst_case(uint64_t len, Bound bound) {
  uint64_t w = HELLO_LEN + 1;
  for (uint64_t a = 0; a < len; a += FRAME_IN) {
    const uint64_t fl = len - a < FRAME_IN ? len - a : FRAME_IN;
    w += FRAME_HEAD + bound((uint32_t)fl);
  }
  return w;
}

struct PipeIn {            // one pipe of the call, after the encoder step
  bool hello, eos;
  const uint8_t* uuid;     // UUID_LEN bytes (read when hello)
  uint32_t first, count;   // its frames: [first, first + count) of the call's frame list
};

struct Piece {
  uint8_t dev;             // 0: src is an offset into `lit`; 1: into the encodings
  uint32_t len;
  uint64_t src, dst;       // dst: into the deflate-input buffer
};

struct WirePlan {
  std::vector<uint8_t> lit;
  std::vector<Piece> pieces;
  std::vector<uint64_t> wire_off;   // per pipe, 256-byte aligned
  std::vector<uint32_t> wire_len;
  uint64_t total = 0;               // bytes of the deflate-input buffer
  uint32_t max_piece = 0;

  WirePlan(const PipeIn* pipes, uint32_t n, const uint64_t* enc_off, const uint64_t* enc_len)
      : wire_off(n), wire_len(n) {
    for (uint32_t k = 0; k < n; ++k) {
      const PipeIn& p = pipes[k];
      wire_off[k] = total;
      uint64_t at = total;
      size_t open = lit.size();                          // literal bytes not yet in a piece start here
      const auto close = [&]() {
        if (lit.size() == open) return;
        add(0, (uint32_t)(lit.size() - open), open, at);
        at += lit.size() - open;
        open = lit.size();
      };
      if (p.hello) {
        lit.push_back(OP_HELLO);
        lit.push_back((uint8_t)UUID_LEN);
        lit.insert(lit.end(), p.uuid, p.uuid + UUID_LEN);
      }
      if (p.eos) lit.push_back(OP_EOS);
      for (uint32_t f = p.first; f < p.first + p.count; ++f) {
        const uint32_t el = (uint32_t)enc_len[f];
        lit.push_back(OP_FRAME);
        for (int s = 24; s >= 0; s -= 8) lit.push_back((uint8_t)(el >> s));
        close();
        if (el) add(1, el, enc_off[f], at);
        at += el;
      }
      close();
      wire_len[k] = (uint32_t)(at - total);
      total = up(at, 256);
    }
  }

 private:
  void add(uint8_t dev, uint32_t len, uint64_t src, uint64_t dst) {
    pieces.push_back(Piece{dev, len, src, dst});
    if (len > max_piece) max_piece = len;
  }
};

// The block that goes up in one copy: [src_off u64][dst_off u64][len u32][literals].
struct WireUpload {
  size_t src, dst, len, lit, end;
  explicit WireUpload(const WirePlan& p) {
    const size_t np = p.pieces.size();
    src = 0;
    dst = up(8 * np, 256);
    len = up(dst + 8 * np, 256);
    lit = up(len + 4 * np, 256);
    end = up(lit + p.lit.size() + 1, 256);
  }
  // Into `end` bytes at h.  A piece's source offset is relative to one base
  // address: lit_base / enc_base are where the literals (h + lit, once on the
  // device) and the encodings lie relative to it (wrapping arithmetic).
  void fill(const WirePlan& p, uint8_t* h, uint64_t lit_base, uint64_t enc_base) const {
    uint64_t* so = (uint64_t*)(h + src);
    uint64_t* dd = (uint64_t*)(h + dst);
    uint32_t* ln = (uint32_t*)(h + len);
    for (size_t i = 0; i < p.pieces.size(); ++i) {
      const Piece& q = p.pieces[i];
      so[i] = (q.dev ? enc_base : lit_base) + q.src;
      dd[i] = q.dst;
      ln[i] = q.len;
    }
    if (!p.lit.empty()) memcpy(h + lit, p.lit.data(), p.lit.size());
  }
};

}  // namespace wire
}  // namespace xcg
