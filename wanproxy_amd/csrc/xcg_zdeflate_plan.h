// The deflate stage's host plan: what a batch's call list is checked for, where
// each call's arrays and each scratch section lie, the meta block the kernels
// read the call list from, and the staging of a host-buffer call.  Offsets and
// counts only, no HIP: the drivers in xcg_zdeflate.hip turn them into pointers
// (ZdPlan::bind), and oracle/zdeflate_plan_harness.cc runs the same code on the
// CPU under sanitizers (tests/test_zdeflate_plan.py).  Every section starts
// 256-byte aligned.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/xcgpu.h"
#include "xcg_devmem.h"   // align_up
#include "xcg_stored_plan.h"
#include "xcg_zdeflate_types.h"

namespace xcg {
namespace zd {

// Room a call's output needs (xcg_zdeflate_bound).
inline uint64_t zdeflate_bound(uint32_t len) { return (uint64_t)len + (len >> 1) + 2 * DMAX + 128; }

// The call list both drivers accept: every stream in range and listed once,
// outputs on 4-byte boundaries, at most 2^24 bytes per call.  Reads only: a
// driver runs it before anything that mutates a stream's host state.
inline int check_calls(uint32_t nstreams, const uint32_t* h_stream, const uint64_t* h_out_off, const uint32_t* h_len,
                       uint32_t n) {
  std::vector<uint8_t> seen(nstreams, 0);
  for (uint32_t i = 0; i < n; i++) {
    if (h_stream[i] >= nstreams || seen[h_stream[i]] || (h_out_off[i] & 3) || h_len[i] > MAX_CALL_LEN)
      return XCG_EINVAL;
    seen[h_stream[i]] = 1;
  }
  return XCG_OK;
}

struct ZdScratch {   // byte offsets of the scratch sections (ZArgs members of the same names)
  size_t X, d16, pk, tf, tq, sym, blk, tab, res, ma, mb, chg, end;
};
struct ZdMeta {      // byte offsets in the meta block: the call list and the three prefix maps
  size_t calls, ms, gs, bs, end;
};

// Levels 1-9: one batch.
struct ZdPlan {
  std::vector<ZCall> calls;
  std::vector<uint32_t> mstart, gstart, bstart;   // n + 1 each (ZArgs)
  size_t xo = 0, to = 0, mo = 0;   // X bytes, table entries and mask words of the whole batch
  uint32_t bo = 0;                 // block records
  uint32_t mtiles = 0, groups = 0, maxlen = 0;
  int level = 0;
  bool fast = false;               // deflate_fast (levels 1-3)
  ZdScratch s{};
  ZdMeta m{};

  ZdPlan(const uint64_t* h_in_off, const uint32_t* h_len, const uint32_t* h_stream, const uint64_t* h_out_off,
         uint32_t n, int level_)
      : calls(n), mstart(n + 1), gstart(n + 1), bstart(n + 1), level(level_), fast(level_ < 4) {
    for (uint32_t i = 0; i < n; i++) {
      ZCall& c = calls[i];
      c.in_off = h_in_off[i];
      c.out_off = h_out_off[i];
      c.len = h_len[i];
      c.stream = h_stream[i];
      c.x_off = xo;
      xo += align_up((size_t)WSIZE + c.len + XPAD, 256);
      c.m_off = mo;                                 // (deflate_fast masks: one bit per X index)
      mo += fast ? align_up(((size_t)WSIZE + c.len + 64) / 32 + 1, 64) : 0;
      c.t_off = to;                                 // (parsed positions: up to DMAX left by the last call)
      to += align_up((size_t)c.len + DMAX + 1, 64);
      c.blk_off = bo;
      c.blk_cap = (c.len + DMAX) / SYMS_PER_BLOCK + 2;
      bstart[i] = bo;
      bo += c.blk_cap;
      mstart[i + 1] = mstart[i] + (c.len + DMAX + 255) / 256;
      gstart[i + 1] = gstart[i] + ((uint32_t)WSIZE + c.len + 63) / 64 + 1;
      maxlen = std::max(maxlen, c.len);
    }
    bstart[n] = bo;
    mtiles = mstart[n];
    groups = gstart[n];
    s.X = 0;
    s.d16 = align_up(s.X + xo, 256);
    s.pk = align_up(s.d16 + 2 * xo, 256);
    s.tf = align_up(s.pk + 4 * xo, 256);
    s.tq = align_up(s.tf + 4 * to, 256);
    s.sym = align_up(s.tq + 4 * to, 256);
    s.blk = align_up(s.sym + 4 * to, 256);
    s.tab = align_up(s.blk + sizeof(ZBlock) * bo, 256);
    s.res = align_up(s.tab + 4ull * TAB_WORDS * bo, 256);
    s.ma = align_up(s.res + sizeof(ZCallRes) * n, 256);
    s.mb = align_up(s.ma + 4 * mo, 256);
    s.chg = align_up(s.mb + 4 * mo, 256);
    s.end = align_up(s.chg + 4ull * n, 256);
    m.calls = 0;
    m.ms = align_up(sizeof(ZCall) * n, 256);
    m.gs = align_up(m.ms + 4ull * (n + 1), 256);
    m.bs = align_up(m.gs + 4ull * (n + 1), 256);
    m.end = align_up(m.bs + 4ull * (n + 1), 256);
  }
  uint32_t n() const { return (uint32_t)calls.size(); }

  // the meta block's content, into m.end bytes of (pinned) host memory
  void fill_meta(uint8_t* hm) const {
    memcpy(hm + m.calls, calls.data(), sizeof(ZCall) * n());
    memcpy(hm + m.ms, mstart.data(), 4ull * (n() + 1));
    memcpy(hm + m.gs, gstart.data(), 4ull * (n() + 1));
    memcpy(hm + m.bs, bstart.data(), 4ull * (n() + 1));
  }
  // every ZArgs member the plan places: the scratch sections and the meta block's arrays
  void bind(ZArgs& a, uint8_t* scratch, uint8_t* meta) const {
    a.calls = (const ZCall*)(meta + m.calls);
    a.mstart = (const uint32_t*)(meta + m.ms);
    a.gstart = (const uint32_t*)(meta + m.gs);
    a.bstart = (const uint32_t*)(meta + m.bs);
    a.X = scratch + s.X;
    a.d16 = (uint16_t*)(scratch + s.d16);
    a.pk = (uint32_t*)(scratch + s.pk);
    a.tf = (uint32_t*)(scratch + s.tf);
    a.tq = (uint32_t*)(scratch + s.tq);
    a.sym = (uint32_t*)(scratch + s.sym);
    a.blk = (ZBlock*)(scratch + s.blk);
    a.tabs = (uint32_t*)(scratch + s.tab);
    a.res = (ZCallRes*)(scratch + s.res);
    a.mcur = (uint32_t*)(scratch + s.ma);
    a.mnext = (uint32_t*)(scratch + s.mb);
    a.changed = (uint32_t*)(scratch + s.chg);
    a.n = n();
    a.level = level;
    a.fast = fast ? 1 : 0;
  }
};

// Level 0's meta block: the call list, the pieces, and the lengths and deliver
// counts the host already knows (copied to the caller's arrays on the device).
// Its scratch is the calls' ZCallRes alone.
struct ZsMeta {
  size_t calls, pc, len, dl, end;
  size_t res_bytes;
  ZsMeta(uint32_t n, size_t npieces) {
    calls = 0;
    pc = align_up(sizeof(ZCall) * n, 256);
    len = align_up(pc + sizeof(ZPiece) * npieces, 256);
    dl = align_up(len + 4ull * n, 256);
    end = align_up(dl + 8ull * n, 256);
    res_bytes = align_up(sizeof(ZCallRes) * n, 256);
  }
};

// xcg_zdeflate_host's staging, one layout on the host and on the device:
// [in][out][out_len n][deliver n]; doff[i]: call i's output inside [out].
struct ZdStaging {
  std::vector<uint64_t> doff;
  uint64_t in_end = 0, out_end = 0;
  size_t out, len, dl, end;
  ZdStaging(const uint64_t* h_in_off, const uint32_t* h_len, uint32_t n) : doff(n) {
    for (uint32_t i = 0; i < n; i++) {
      in_end = std::max(in_end, h_in_off[i] + h_len[i]);
      doff[i] = out_end;
      out_end += align_up(zdeflate_bound(h_len[i]), 4);
    }
    out = align_up(in_end + 1, 256);
    len = align_up(out + out_end, 256);
    dl = align_up(len + 4ull * n, 256);
    end = align_up(dl + 8ull * n, 256);
  }
};

}  // namespace zd
}  // namespace xcg
