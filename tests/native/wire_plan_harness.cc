// The codec send path's host plan (wanproxy_amd/csrc/xcg_wire_plan.h) on the
// CPU: the plan's pieces are executed with memcpy into a buffer of exactly the
// planned size, and every pipe's wire is compared with the wire written by
// definition -- <HELLO>, <EOS>, then per frame its 5-byte header and its
// encoding.  The pieces must tile each wire exactly (no gap, no overlap) and
// touch nothing outside it.  Stand-alone; tests/test_wire_plan.py builds it with
// AddressSanitizer and UndefinedBehaviorSanitizer and runs it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../wanproxy_amd/csrc/xcg_wire_plan.h"
#include "../../wanproxy_amd/csrc/xcg_zdeflate_types.h"   // the deflate stage's per-consume limit

using namespace xcg::wire;

static int g_fail = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);     \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

static uint64_t bound(uint32_t len) { return 2ull * len + 16; }   // (the shape of the encoder's bound: any would do)

struct Call {                       // a send call after the encoder step, with made-up encodings
  std::vector<PipeIn> pipes;
  std::vector<std::vector<uint8_t>> uuids;
  std::vector<uint64_t> enc_off, enc_len;
  std::vector<uint8_t> enc;         // exact size: the slots' room, as the encoder lays them out
  void pipe(bool hello, bool eos, const std::vector<uint32_t>& frame_lens, uint32_t seed) {
    uuids.push_back(std::vector<uint8_t>(UUID_LEN));
    for (uint32_t i = 0; i < UUID_LEN; ++i) uuids.back()[i] = (uint8_t)('a' + (seed + i) % 26);
    PipeIn p{hello, eos, nullptr, (uint32_t)enc_off.size(), (uint32_t)frame_lens.size()};
    for (uint32_t el : frame_lens) {
      enc_off.push_back(enc.size());
      enc_len.push_back(el);
      const size_t at = enc.size();
      enc.resize(at + el + 16 + seed % 7);             // (a slot is longer than what it holds)
      for (uint32_t i = 0; i < el; ++i) enc[at + i] = (uint8_t)(seed * 31 + i * 7 + (i >> 8));
    }
    pipes.push_back(p);
  }
  void bind() {
    for (size_t k = 0; k < pipes.size(); ++k) pipes[k].uuid = uuids[k].data();
  }
};

static std::vector<uint8_t> wire_by_definition(const Call& c, uint32_t k) {
  std::vector<uint8_t> w;
  const PipeIn& p = c.pipes[k];
  if (p.hello) {
    w.push_back(0xff);
    w.push_back(36);
    w.insert(w.end(), p.uuid, p.uuid + 36);
  }
  if (p.eos) w.push_back(0xfc);
  for (uint32_t f = p.first; f < p.first + p.count; ++f) {
    const uint32_t el = (uint32_t)c.enc_len[f];
    w.push_back(0x02);
    for (int s = 24; s >= 0; s -= 8) w.push_back((uint8_t)(el >> s));
    w.insert(w.end(), c.enc.begin() + (ptrdiff_t)c.enc_off[f], c.enc.begin() + (ptrdiff_t)(c.enc_off[f] + el));
  }
  return w;
}

static void check(Call& c) {
  c.bind();
  const uint32_t n = (uint32_t)c.pipes.size();
  const WirePlan plan(c.pipes.data(), n, c.enc_off.data(), c.enc_len.data());
  const WireUpload up(plan);
  CHECK(plan.wire_off.size() == n && plan.wire_len.size() == n);
  // the upload block, then the gather as memcpy: sources relative to the block's start
  std::vector<uint8_t> block(up.end, 0xEE);
  const uint64_t enc_base = 1ull << 40;                // (the encodings lie elsewhere)
  up.fill(plan, block.data(), up.lit, enc_base);
  CHECK(up.src % 8 == 0 && up.dst % 8 == 0 && up.len % 4 == 0);
  CHECK(up.lit + plan.lit.size() <= up.end);
  const uint64_t* so = (const uint64_t*)(block.data() + up.src);
  const uint64_t* dd = (const uint64_t*)(block.data() + up.dst);
  const uint32_t* ln = (const uint32_t*)(block.data() + up.len);
  std::vector<uint8_t> dst(plan.total, 0xCC);          // exact size
  std::vector<uint8_t> hits(plan.total, 0);
  uint32_t longest = 0;
  for (size_t i = 0; i < plan.pieces.size(); ++i) {
    CHECK(ln[i] > 0);
    CHECK(dd[i] + ln[i] <= plan.total);
    if (dd[i] + ln[i] > plan.total) return;
    const uint8_t* s;
    if (so[i] >= enc_base) {
      CHECK(so[i] - enc_base + ln[i] <= c.enc.size());
      if (so[i] - enc_base + ln[i] > c.enc.size()) return;
      s = c.enc.data() + (so[i] - enc_base);
    } else {
      CHECK(so[i] >= up.lit && so[i] + ln[i] <= up.lit + plan.lit.size());
      if (so[i] + ln[i] > block.size()) return;
      s = block.data() + so[i];
    }
    memcpy(dst.data() + dd[i], s, ln[i]);
    for (uint32_t b = 0; b < ln[i]; ++b) ++hits[dd[i] + b];
    longest = std::max(longest, ln[i]);
  }
  CHECK(longest == plan.max_piece);
  uint64_t end = 0;
  for (uint32_t k = 0; k < n; ++k) {
    const std::vector<uint8_t> w = wire_by_definition(c, k);
    CHECK(plan.wire_off[k] % 256 == 0 && plan.wire_off[k] >= end);
    CHECK(plan.wire_len[k] == w.size());
    CHECK(plan.wire_off[k] + w.size() <= plan.total);
    if (plan.wire_off[k] + w.size() > plan.total) return;
    CHECK(w.empty() || memcmp(dst.data() + plan.wire_off[k], w.data(), w.size()) == 0);
    for (uint64_t b = end; b < plan.wire_off[k]; ++b) CHECK(hits[b] == 0 && dst[b] == 0xCC);   // between the wires
    for (uint64_t b = 0; b < w.size(); ++b)
      if (hits[plan.wire_off[k] + b] != 1) {             // no gap, no overlap
        CHECK(hits[plan.wire_off[k] + b] == 1);
        break;
      }
    end = plan.wire_off[k] + w.size();
  }
  for (uint64_t b = end; b < plan.total; ++b) CHECK(hits[b] == 0);
}

int main() {
  {  // zero pipes
    Call c;
    check(c);
    const WirePlan plan(nullptr, 0, nullptr, nullptr);
    CHECK(plan.total == 0 && plan.pieces.empty() && plan.lit.empty() && plan.max_piece == 0);
    printf("ok zero_pipes\n");
  }
  {  // a pipe with only <EOS>; with <HELLO> in front; between pipes that carry frames
    Call c;
    c.pipe(false, true, {}, 1);
    check(c);
    const WirePlan one(c.pipes.data(), 1, c.enc_off.data(), c.enc_len.data());
    CHECK(one.pieces.size() == 1 && one.wire_len[0] == 1 && one.max_piece == 1);
    c.pipe(true, true, {}, 2);
    c.pipe(false, false, {100}, 3);
    c.pipe(false, true, {}, 4);
    check(c);
    printf("ok eos_only\n");
  }
  {  // the three-frame consume (2 x 512 KiB + 1 input bytes), beside a new pipe and a closing one
    Call c;
    c.pipe(true, false, {3000}, 5);
    c.pipe(false, false, {(uint32_t)bound(FRAME_IN), 700000, 3}, 6);
    c.pipe(false, true, {}, 7);
    c.pipe(true, false, {1, 0, 2}, 8);                   // (an empty encoding: a header alone)
    check(c);
    CHECK(frames_of(2 * FRAME_IN + 1) == 3 && frames_of(FRAME_IN) == 1 && frames_of(0) == 0);
    printf("ok three_frames\n");
  }
  {  // the largest admitted consume: the longest input whose worst-case wire stays within the
     // deflate stage's limit, every frame at its bound
    const uint64_t limit = xcg::zd::MAX_CALL_LEN;
    uint64_t lo = 0, hi = limit;                         // worst_case is monotonic in len
    while (lo < hi) {
      const uint64_t mid = (lo + hi + 1) / 2;
      if (worst_case(mid, bound) <= limit) lo = mid;
      else hi = mid - 1;
    }
    CHECK(worst_case(lo, bound) <= limit && worst_case(lo + 1, bound) > limit);
    CHECK(worst_case(0, bound) == HELLO_LEN + 1);
    std::vector<uint32_t> frames;
    for (uint64_t a = 0; a < lo; a += FRAME_IN)
      frames.push_back((uint32_t)bound((uint32_t)std::min<uint64_t>(FRAME_IN, lo - a)));
    CHECK(frames.size() == frames_of(lo));
    Call c;
    c.pipe(true, false, frames, 9);
    check(c);
    c.bind();
    const WirePlan plan(c.pipes.data(), 1, c.enc_off.data(), c.enc_len.data());
    CHECK(plan.wire_len[0] <= limit && plan.wire_len[0] + 1 == worst_case(lo, bound));   // (no <EOS> beside frames)
    printf("ok largest_admitted\n");
  }
  return g_fail ? 1 : 0;
}
