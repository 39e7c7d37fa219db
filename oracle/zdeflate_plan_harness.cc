// CPU test of the deflate stage's host plan
// (wanproxy_amd/csrc/xcg_zdeflate_plan.h): the same code xcg_zdeflate.hip's
// drivers run, here on its own under AddressSanitizer and
// UndefinedBehaviorSanitizer (oracle/Makefile).  Stand-alone: one
// "ok <case>" line per case and exit 0, or the check that failed and exit 1.
// tests/test_zdeflate_plan.py runs it.  Any sanitizer report ends the program
// with a non-zero status.
//
// What a section must hold is taken from what the kernels index (named at each
// figure below), not from the plan's own formulas.
// TEST INFRASTRUCTURE ONLY.
#define XCG_DEVMEM_NO_HIP
#include "../wanproxy_amd/csrc/xcg_zdeflate_plan.h"

#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

using namespace xcg::zd;

namespace {

#define CHECK(x)                                                                    \
  do {                                                                              \
    if (!(x)) {                                                                     \
      fprintf(stderr, "zdeflate_plan_harness: line %d: CHECK(%s)\n", __LINE__, #x); \
      exit(1);                                                                      \
    }                                                                               \
  } while (0)

struct Calls {   // a call list in heap arrays of exactly its size
  std::vector<uint64_t> in_off, out_off;
  std::vector<uint32_t> len, stream;
  explicit Calls(const std::vector<uint32_t>& lens) : len(lens) {
    uint64_t io = 0, oo = 0;
    for (size_t i = 0; i < lens.size(); i++) {
      in_off.push_back(io);
      out_off.push_back(oo);
      stream.push_back((uint32_t)i);
      io += lens[i];
      oo += (zdeflate_bound(lens[i]) + 3) & ~3ull;
    }
  }
  uint32_t n() const { return (uint32_t)len.size(); }
  int check(uint32_t nstreams) const { return check_calls(nstreams, stream.data(), out_off.data(), len.data(), n()); }
  ZdPlan plan(int level) const { return ZdPlan(in_off.data(), len.data(), stream.data(), out_off.data(), n(), level); }
};

const std::vector<uint32_t> LENS = {0, 1, 63, 64, 255, 256, 16382, 16383, 16384, 65535, 65536, 1u << 24};

std::vector<Calls> call_lists() {
  std::vector<Calls> l;
  for (uint32_t v : LENS) l.push_back(Calls({v}));             // one call
  l.push_back(Calls(LENS));                                    // mixed in one batch
  l.push_back(Calls(std::vector<uint32_t>(4096, 1u)));         // many tiny calls
  return l;
}

void case_check() {
  const Calls good({5, 6, 7});
  CHECK(good.check(3) == XCG_OK);
  CHECK(good.check(2) == XCG_EINVAL);                          // the last call's stream == nstreams
  {
    Calls c = good;
    c.stream[0] = 3;                                           // stream == nstreams, first call
    CHECK(c.check(3) == XCG_EINVAL);
    CHECK(c.check(4) == XCG_OK);
  }
  {
    Calls c = good;
    c.stream[2] = 0;                                           // listed twice: first and last
    CHECK(c.check(3) == XCG_EINVAL);
    c = good;
    c.stream[1] = 0;                                           // listed twice: adjacent
    CHECK(c.check(3) == XCG_EINVAL);
    c = good;
    c.stream[2] = 1;
    CHECK(c.check(3) == XCG_EINVAL);
  }
  for (uint64_t off = 1; off <= 3; off++)
    for (uint32_t at = 0; at < 3; at++) {                      // (at == 2: a bad last call refuses the whole list)
      Calls c = good;
      c.out_off[at] += off;
      CHECK(c.check(3) == XCG_EINVAL);
    }
  {
    Calls c = good;
    c.out_off[1] += 4;
    CHECK(c.check(3) == XCG_OK);
  }
  for (uint32_t at = 0; at < 3; at++) {
    Calls c = good;
    c.len[at] = 1u << 24;
    CHECK(c.check(3) == XCG_OK);
    c.len[at] = (1u << 24) + 1;
    CHECK(c.check(3) == XCG_EINVAL);
  }
  CHECK(Calls(std::vector<uint32_t>()).check(1) == XCG_OK);                         // (the drivers refuse n == 0 themselves)
  puts("ok check");
}

struct Sec {
  const char* name;
  size_t off, bytes;
};

// [off, off + bytes) inside [0, end), 256-byte aligned, pairwise disjoint (empty sections overlap nothing)
void check_secs(const std::vector<Sec>& secs, size_t end) {
  CHECK(end % 256 == 0);
  for (const Sec& a : secs) {
    CHECK(a.off % 256 == 0);
    CHECK(a.off <= end && a.bytes <= end - a.off);
    for (const Sec& b : secs)
      if (&a != &b && a.bytes && b.bytes) CHECK(a.off + a.bytes <= b.off || b.off + b.bytes <= a.off);
  }
}

size_t up16(size_t v) { return (v + 15) / 16 * 16; }
// per call, the elements its kernels index past the call's offset
size_t x_bytes(const ZCall& c) { return up16((size_t)WSIZE + c.len + XPAD); }        // zd_prep_kernel: whole 16-byte vectors
size_t x_elems(const ZCall& c) { return (size_t)WSIZE + c.len; }                     // d16, pk: zd_hashes / zd_chain, j < jend
size_t t_elems(const ZCall& c) { return (size_t)c.len + DMAX; }                      // tf, tq: zd_match_kernel, t < DMAX + len;
                                                                                     // sym: one symbol per parsed position at most
size_t m_words(const ZCall& c) { return ((size_t)WSIZE + c.len + 63) / 32 + 1; }     // masks: bits up to WSIZE + len + 63
uint32_t blocks(const ZCall& c) {                                                    // a block per 16383 symbols, and the flush's
  return (uint32_t)(((size_t)c.len + DMAX + SYMS_PER_BLOCK - 1) / SYMS_PER_BLOCK) + 1;
}

void case_sections() {
  for (int level : {6, 1})
    for (const Calls& cl : call_lists()) {
      const ZdPlan p = cl.plan(level);
      const uint32_t n = cl.n();
      CHECK(p.n() == n && p.fast == (level < 4));
      size_t xb = 0, xe = 0, te = 0, mw = 0;
      for (const ZCall& c : p.calls) {
        xb = std::max(xb, (size_t)c.x_off + x_bytes(c));
        xe = std::max(xe, (size_t)c.x_off + x_elems(c));
        te = std::max(te, (size_t)c.t_off + t_elems(c));
        if (p.fast) mw = std::max(mw, (size_t)c.m_off + m_words(c));
      }
      const size_t nrec = p.bstart[n];   // zd_trees_kernel / zd_emit_kernel: block records bi < bstart[n]
      const std::vector<Sec> secs = {
          {"X", p.s.X, xb},           {"d16", p.s.d16, 2 * xe},   {"pk", p.s.pk, 4 * xe},
          {"tf", p.s.tf, 4 * te},     {"tq", p.s.tq, 4 * te},     {"sym", p.s.sym, 4 * te},
          {"blk", p.s.blk, sizeof(ZBlock) * nrec},                {"tab", p.s.tab, 4ull * TAB_WORDS * nrec},
          {"res", p.s.res, sizeof(ZCallRes) * n},                 {"ma", p.s.ma, 4 * mw},
          {"mb", p.s.mb, 4 * mw},     {"chg", p.s.chg, 4ull * n},
      };
      check_secs(secs, p.s.end);
      // zd_mfill_kernel / zd_mzero_kernel run over all p.mo words of each mask
      if (p.fast) CHECK(p.s.ma + 4 * p.mo <= p.s.mb && p.s.mb + 4 * p.mo <= p.s.chg);
    }
  // bind: each pointer is its base plus the section's offset
  const Calls one({1});
  const ZdPlan p = one.plan(1);
  uint8_t* scratch = (uint8_t*)malloc(p.s.end);
  uint8_t* meta = (uint8_t*)malloc(p.m.end);
  CHECK(scratch && meta);
  ZArgs a{};
  p.bind(a, scratch, meta);
  CHECK(a.X == scratch + p.s.X && (uint8_t*)a.d16 == scratch + p.s.d16 && (uint8_t*)a.pk == scratch + p.s.pk);
  CHECK((uint8_t*)a.tf == scratch + p.s.tf && (uint8_t*)a.tq == scratch + p.s.tq && (uint8_t*)a.sym == scratch + p.s.sym);
  CHECK((uint8_t*)a.blk == scratch + p.s.blk && (uint8_t*)a.tabs == scratch + p.s.tab && (uint8_t*)a.res == scratch + p.s.res);
  CHECK((uint8_t*)a.mcur == scratch + p.s.ma && (uint8_t*)a.mnext == scratch + p.s.mb &&
        (uint8_t*)a.changed == scratch + p.s.chg);
  CHECK((const uint8_t*)a.calls == meta + p.m.calls && (const uint8_t*)a.mstart == meta + p.m.ms &&
        (const uint8_t*)a.gstart == meta + p.m.gs && (const uint8_t*)a.bstart == meta + p.m.bs);
  CHECK(a.n == 1 && a.level == 1 && a.fast == 1);
  CHECK(!a.st && !a.hist && !a.in && !a.out && !a.out_len && !a.deliver && !a.ring);   // the driver's
  free(scratch);
  free(meta);
  puts("ok sections");
}

void case_calls() {
  for (int level : {6, 1})
    for (const Calls& cl : call_lists()) {
      const ZdPlan p = cl.plan(level);
      const uint32_t n = cl.n();
      uint32_t tiles = 0, maxlen = 0;
      for (uint32_t i = 0; i < n; i++) {
        const ZCall& c = p.calls[i];
        CHECK(c.in_off == cl.in_off[i] && c.out_off == cl.out_off[i] && c.len == cl.len[i] && c.stream == cl.stream[i]);
        CHECK(c.x_off % 256 == 0);                 // zd_prep_kernel stores 16-byte vectors
        CHECK(c.blk_cap >= blocks(c));
        CHECK(c.blk_off == p.bstart[i]);
        if (i + 1 < n) {
          const ZCall& d = p.calls[i + 1];
          CHECK(c.x_off + x_bytes(c) <= d.x_off);
          CHECK(c.t_off + t_elems(c) <= d.t_off);
          CHECK(c.blk_off + c.blk_cap <= d.blk_off);
          if (p.fast) CHECK(c.m_off + m_words(c) <= d.m_off);
        } else {
          CHECK(c.x_off + x_bytes(c) <= p.xo && c.t_off + t_elems(c) <= p.to && c.blk_off + c.blk_cap <= p.bo);
          if (p.fast) CHECK(c.m_off + m_words(c) <= p.mo);
        }
        if (!p.fast) CHECK(c.m_off == 0);
        // the prefix maps: never decreasing, and a call's share covers its positions
        CHECK(p.mstart[i + 1] >= p.mstart[i] && p.gstart[i + 1] >= p.gstart[i] && p.bstart[i + 1] >= p.bstart[i]);
        CHECK((uint64_t)(p.mstart[i + 1] - p.mstart[i]) * 256 >= t_elems(c));   // zd_match_kernel: 256 entries a tile
        CHECK((uint64_t)(p.gstart[i + 1] - p.gstart[i]) * 64 >= x_elems(c));    // zd_hashes_kernel: 64 positions a group
        CHECK(p.bstart[i + 1] - p.bstart[i] == c.blk_cap);
        tiles += (uint32_t)((t_elems(c) + 255) / 256);
        maxlen = std::max(maxlen, c.len);
      }
      CHECK(p.mstart[0] == 0 && p.gstart[0] == 0 && p.bstart[0] == 0);
      CHECK(p.mstart[n] == p.mtiles && p.mtiles == tiles);
      CHECK(p.gstart[n] == p.groups);
      CHECK(p.bstart[n] == p.bo);
      CHECK(p.maxlen == maxlen);
      if (!p.fast) CHECK(p.mo == 0);
    }
  puts("ok calls");
}

void case_meta() {
  for (const Calls& cl : call_lists()) {
    const ZdPlan p = cl.plan(6);
    const size_t n = cl.n();
    check_secs({{"calls", p.m.calls, sizeof(ZCall) * n},
                {"ms", p.m.ms, 4 * (n + 1)},
                {"gs", p.m.gs, 4 * (n + 1)},
                {"bs", p.m.bs, 4 * (n + 1)}},
               p.m.end);
    uint8_t* hm = (uint8_t*)malloc(p.m.end);   // exactly the block: a write past it is a sanitizer report
    CHECK(hm);
    p.fill_meta(hm);
    CHECK(!memcmp(hm + p.m.calls, p.calls.data(), sizeof(ZCall) * n));
    CHECK(!memcmp(hm + p.m.ms, p.mstart.data(), 4 * (n + 1)));
    CHECK(!memcmp(hm + p.m.gs, p.gstart.data(), 4 * (n + 1)));
    CHECK(!memcmp(hm + p.m.bs, p.bstart.data(), 4 * (n + 1)));
    free(hm);
  }
  // level 0: no pieces, one, many
  for (uint32_t n : {1u, 3u, 4096u})
    for (size_t np : {(size_t)0, (size_t)1, (size_t)100000}) {
      const ZsMeta m(n, np);
      check_secs({{"calls", m.calls, sizeof(ZCall) * n},
                  {"pc", m.pc, sizeof(ZPiece) * np},
                  {"len", m.len, 4ull * n},
                  {"dl", m.dl, 8ull * n}},
                 m.end);
      CHECK(m.res_bytes >= sizeof(ZCallRes) * n);
    }
  puts("ok meta");
}

void case_staging() {
  std::vector<std::vector<uint32_t>> lists = {{0}, {0, 0, 0}, {1}, {1u << 24}, LENS, std::vector<uint32_t>(4096, 1u)};
  for (const std::vector<uint32_t>& lens : lists) {
    const Calls cl(lens);
    const uint32_t n = cl.n();
    const ZdStaging g(cl.in_off.data(), cl.len.data(), n);
    uint64_t in_end = 0;
    for (uint32_t i = 0; i < n; i++) {
      in_end = std::max(in_end, cl.in_off[i] + cl.len[i]);
      CHECK(g.doff[i] % 4 == 0);
      const uint64_t next = i + 1 < n ? g.doff[i + 1] : g.out_end;
      CHECK(next >= g.doff[i] && next - g.doff[i] >= zdeflate_bound(cl.len[i]));
    }
    CHECK(g.in_end == in_end);
    CHECK(g.out % 4 == 0 && g.len % 4 == 0 && g.dl % 8 == 0);   // d_out + doff[i], uint32_t[n], uint64_t[n]
    // the input, output, length and deliver regions (an empty input takes no room but overlaps nothing)
    check_secs({{"in", 0, (size_t)in_end}, {"out", g.out, (size_t)g.out_end}, {"len", g.len, 4ull * n}, {"dl", g.dl, 8ull * n}},
               g.end);
  }
  CHECK(zdeflate_bound(0) == 2 * DMAX + 128 && zdeflate_bound(1u << 24) == (1ull << 24) + (1ull << 23) + 2 * DMAX + 128);
  puts("ok staging");
}

}  // namespace

int main() {
  case_check();
  case_sections();
  case_calls();
  case_meta();
  case_staging();
  return 0;
}
