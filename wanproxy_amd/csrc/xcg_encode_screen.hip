// XCodec encoder, stream semantics: the quiet-chunk screen in front of the parse.
//
// Small stream chunks (C4's 4 KiB packets: 2049 window positions each, a wave
// per packet, sixteen packets in turn per wave) spend their parse mostly in
// per-chunk round trips, and in hash-bound traffic (few repeats) almost every
// one of them ends as the cold parse: the 2048-byte tiling, with no lookup
// finding anything ("the cold parse of unique data is an exact
// 2048-aligned tiling").  That outcome is decided without the state machine:
// when no window of the chunk can be found -- in the persistent cache, among
// the batch's declarations, or among the chunk's own tiles declared before it
// (a tile at t is declared while examining window t + 2048, xcodec_encoder.cc:
// 183-190, so it is visible to the windows of every later piece) -- every lookup
// misses, and encode() declares exactly the tiles (:222-261) and escapes the
// tail (:267-269).
//
// stream_screen_kernel rolls every window of a chunk through the round's
// filters (a 128 KiB LDS fold of the global lane filter, then the global filter
// and the fingerprint buckets for what passes) and compares it with the
// chunk's earlier tiles; it writes the chunk's tiling output and stages its
// rows, with no dependent lookups, the next chunk's loads in flight meanwhile.
// screen_finish_kernel (a thread per chunk) checks each tile's own window
// exactly -- a tile is in the batch table as this chunk's own declaration;
// anything else there or in the persistent cache is a possible hit -- and
// either commits the staged rows and counters or puts the chunk on the work
// list encode_stream_kernel parses as always (any possible hit, an unaligned
// start, more than SCREEN_MAXD tiles).  Either way the output is the
// sequential encoder's: the screen only skips parses whose every lookup misses.
#include "xcg_encode_wave.h"

namespace xcg {

// (SCREEN_MAXD, xcg_args.h: chunks shorter than 4 tiles)
constexpr uint32_t SCREEN_FOLD_WORDS = 32768;        // 128 KiB of LDS
constexpr int SCREEN_W = 12;                         // waves per workgroup (one workgroup per CU; 16: 3 % slower)
constexpr uint32_t SCR_NEEDY = 1u << 31, SCR_SKIP = 1u << 30;   // s_info flags
__device__ __forceinline__ uint32_t fold_word_of(uint32_t k, uint32_t fwm) { return (k >> 10) & fwm; }

// The LDS fold of the global lane filter: word j of the fold = OR of the global
// words j, j + F, j + 2F, ... (gfilt_word = K bits 10..; the fold keeps the
// low bits of that index), so a key's two bits are set in the fold whenever
// they are in its global word: no false negatives.
__global__ __launch_bounds__(256) void screen_fold_kernel(const uint32_t* gf, uint32_t gwords, uint32_t* fold,
                                                          uint32_t fwords) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= fwords) return;
  uint32_t w = 0;
  for (uint32_t j = i; j < gwords; j += fwords) w |= gf[j];
  fold[i] = w;
}

// What the screen stages: per chunk s_info = flags | tiles << 16 | output
// length, its tiles' rows (lo, hi, position, output length after it), and the
// keys of its windows that passed the LDS fold (qcnt of them), for the probe.
constexpr uint32_t SCREEN_QCAP = 1024;               // fold passes kept per chunk (more: the parse)
struct ScreenStage {
  uint32_t* info;      // [n]
  uint4* rows;         // [n * SCREEN_MAXD]
  uint32_t* qcnt;      // [n]
  uint32_t* qkeys;     // [n * SCREEN_QCAP]
};

// What the screen reads (a slim copy of EncParams: kernel arguments live in
// SGPRs, and the screen needs few of them).
struct ScreenParams {
  const uint8_t* in;
  const uint64_t* chunk_off;
  const uint32_t* chunk_len;
  const uint64_t* out_off;
  uint8_t* out;
  const uint4* decl;
  const uint32_t* ndecl;
  uint32_t* changed;
  const uint32_t* need;
  uint32_t n, skip_below, max_len, maxd;
};

// The lanes' chunk metadata for chunks base + k * stride (lane k).
struct ScreenMeta {
  uint64_t off, oo;
  uint32_t len, nold, go;
};

__device__ __forceinline__ ScreenMeta screen_meta(const ScreenParams& prm, uint32_t ck) {
  ScreenMeta m{0ull, 0ull, 0u, 0u, 0u};
  if (ck < prm.n && ck >= prm.skip_below && (!prm.need || prm.need[ck] != 0u)) {
    m.go = 1u;
    m.off = prm.chunk_off[ck];
    m.oo = prm.out_off[ck];
    m.len = prm.chunk_len[ck];
    m.nold = prm.ndecl[ck];
  }
  return m;
}

// Where a chunk is (wave-uniform, read from the lanes that loaded it: no
// memory wait inside the chunk loop), its first piece's A and B halves and
// its old rows (lane i: row i), all loaded while the chunk before it rolls.
struct ScreenLoad {
  uint64_t off, oo;    // input offset, output offset
  int L;
  uint32_t nold;       // its rows of the last round
  bool go;             // screened (not skipped by the round)
  u32x4 a0, a1, b0, b1;
  uint4 ov;
};

__device__ __forceinline__ bool screen_shape(int L, uint64_t off, const uint8_t* in) {
  return L >= SEG && !(L & (SEG - 1)) && L / SEG < SCREEN_MAXD && !(off & 15u) && !((uintptr_t)in & 15u);
}

__device__ __forceinline__ void screen_issue(const ScreenParams& prm, const ScreenMeta& m, int k, uint32_t chunk,
                                             ScreenLoad& s) {
  const int l = lane_id();
  s.go = readlane(m.go, k) != 0u;
  s.off = readlane64(m.off, k);
  s.oo = readlane64(m.oo, k);
  s.L = (int)readlane(m.len, k);
  s.nold = readlane(m.nold, k);
  s.a0 = s.a1 = s.b0 = s.b1 = u32x4{0u, 0u, 0u, 0u};
  s.ov = make_uint4(0u, 0u, 0u, 0u);
  if (!s.go || !screen_shape(s.L, s.off, prm.in)) return;
  const uint8_t* x = prm.in + s.off;
  const int q0 = 32 * l;
  s.a0 = load16_stream(x + q0);
  s.a1 = load16_stream(x + q0 + 16);
  if (s.L > SEG + 1) {
    s.b0 = load16_stream(x + q0 + SEG);
    s.b1 = load16_stream(x + q0 + SEG + 16);
  }
  if ((uint32_t)l < s.nold && l < SCREEN_MAXD) s.ov = prm.decl[(uint64_t)chunk * prm.maxd + l];
}

// Pass 1 of one chunk whose loads `cur` issued: every window rolled through
// the LDS fold; the passes queued for the probe, the tiling written, the rows
// staged.  No memory wait but the loads `cur` made (the next chunk's go out
// here).
__device__ __forceinline__ void screen_chunk(const ScreenParams& prm, const uint32_t* F, uint32_t fwm, uint32_t chunk,
                                             const ScreenLoad& cur, ScreenStage st, ScreenLoad& nxt,
                                             const ScreenMeta& meta, int knext, uint32_t next_chunk) {
  const int l = lane_id();
  const int L = cur.L;
  const uint8_t* x = prm.in + cur.off;
  uint8_t* const out = prm.out + cur.oo;
  const uint4 ov = cur.ov;
  Piece P;
  P.a0 = cur.a0; P.a1 = cur.a1; P.b0 = cur.b0; P.b1 = cur.b1;
  if (knext < 64) screen_issue(prm, meta, knext, next_chunk, nxt);
  else nxt.go = false;
  auto verdict = [&](uint32_t v) {
    if (l == 0) st.info[chunk] = v;
  };
  // Longer than the launch's bound, shorter than a window (only an escape,
  // xcodec_encoder.cc:77-83), a tail after the tiles (escaped by the parse),
  // or an unaligned start (pieces = tiles needs an aligned one): the parse.
  if ((uint32_t)L > prm.max_len || L / SEG >= (int)prm.maxd || !screen_shape(L, cur.off, prm.in)) {
    verdict(SCR_NEEDY);
    return;
  }
  const uint32_t nold = cur.nold;
  const int last = L - SEG;                        // last window start
  const int nt = L / SEG;                          // tiles = pieces
  uint32_t tlo[SCREEN_MAXD] = {0u, 0u, 0u, 0u}, thi[SCREEN_MAXD] = {0u, 0u, 0u, 0u};
  uint32_t tk[SCREEN_MAXD] = {0u, 0u, 0u, 0u};
  P.sxb = 0u; P.sqxb = 0u;
  uint32_t totXA = 0, totTA = 0;
  uint32_t qn = 0;                                 // passes queued so far
  uint32_t* const q = st.qkeys + (uint64_t)chunk * SCREEN_QCAP;
  bool needy = false;
  // the old rows are the tiling (the seeded round): their hi halves stand
  const bool rows_tiling = nold == (uint32_t)nt;
#pragma unroll 1
  for (int i = 0; i < nt && !needy; ++i) {
    const int p = SEG * i;
    const int q0 = p + 32 * l;
    const int pe = min(p + SEG, last + 1);         // piece end (exclusive)
    const bool one = pe - p == 1;                  // (a chunk of 2048 k bytes ends with a one-window piece)
    if (i == 0) {
      seg_sums(P.a0, P.a1, P.sxa, P.sqxa);
    } else {
      P.a0 = P.b0; P.a1 = P.b1;
      P.sxa = P.sxb; P.sqxa = P.sqxb;
      if (!one) {
        P.b0 = load16_stream(x + q0 + SEG);
        P.b1 = load16_stream(x + q0 + SEG + 16);
      }
    }
    // start sums of the lane's first window (encode_chunk's piece setup); a
    // one-window piece needs only lane 0's, which are the carried totals
    uint32_t tki;
    uint32_t NX1 = 0, NX2 = 0, totXB = 0, totTB = 0;
    const uint32_t qa = 32u * (uint32_t)l;
    if (i == 0) {
      totXA = wave_sum(P.sxa);
      totTA = wave_sum(qa * P.sxa + P.sqxa);
    }
    if (one) {
      tki = (0u - totXA) * (1u << 20) + (0u - (2048u * totXA - totTA + CLO));
    } else {
      seg_sums(P.b0, P.b1, P.sxb, P.sqxb);
      const uint32_t qb = 2048u + qa;
      const uint32_t ta = qa * P.sxa + P.sqxa, tb = qb * P.sxb + P.sqxb;
      const uint32_t dx = P.sxb - P.sxa, dt = tb - ta;
      const uint32_t ix = wave_incl_scan(dx), it = wave_incl_scan(dt);
      const uint32_t X1 = totXA + ix - dx;
      const uint32_t TT = totTA + it - dt;
      const uint32_t X2c = (2048u + qa) * X1 - TT + CLO;
      totXB = totXA + readlane(ix, 63);
      totTB = totTA + readlane(it, 63) - 2048u * totXB;
      NX1 = 0u - X1;
      NX2 = 0u - X2c;
      tki = readfirst((NX1 << 20) + NX2);
    }
    // the tile at the piece start: its hash (the old row's hi when the row is
    // this tile), and its EXTRACT (encode_declaration :300-302; the body is
    // this piece's A half)
    const uint32_t oz = readlane(ov.z, i), ox = readlane(ov.x, i), oy = readlane(ov.y, i);
    const uint32_t thii = rows_tiling && oz == (uint32_t)p && ox == 0u - tki ? oy : readfirst(lane_window_hi(P, 0));
    bool own = false;
#pragma unroll
    for (int u = 0; u < SCREEN_MAXD; ++u) {
      if (u < i) own |= tki == tk[u];
      if (u == i) { tk[u] = tki; tlo[u] = 0u - tki; thi[u] = thii; }
    }
    {
      uint8_t* dst = out + (uint32_t)(2 + SEG) * (uint32_t)i;
      if (l < 2) dst[l] = (uint8_t)(l == 0 ? MAGIC : OP_EXTRACT);
      *(u32x4_u*)(dst + 2 + 32 * l) = P.a0;
      *(u32x4_u*)(dst + 2 + 32 * l + 16) = P.a1;
    }
    if (own) {                                     // the tile's own window = an earlier tile
      needy = true;
      break;
    }
    if (one) continue;
    // every other window of the piece: the round's filters, the earlier tiles
    const uint32_t xa[8] = {P.a0[0], P.a0[1], P.a0[2], P.a0[3], P.a1[0], P.a1[1], P.a1[2], P.a1[3]};
    const uint32_t xb[8] = {P.b0[0], P.b0[1], P.b0[2], P.b0[3], P.b1[0], P.b1[1], P.b1[2], P.b1[3]};
    // positions past the last window are not positions; the piece start is the
    // tile itself (checked exactly by the probe).  (A window past the last one
    // that equals an earlier tile only costs the screen this chunk.)
    const int nvalid = pe - q0;
    uint32_t vm = nvalid >= 32 ? 0xFFFFFFFFu : ((1u << (uint32_t)max(nvalid, 0)) - 1u);
    if (l == 0) vm &= ~1u;
    // own earlier tiles: only a full piece after the first has one (chunks are
    // 2, 4 or 6 KiB; the last piece of each is one window), tile 0
    const uint32_t ko = tk[0];
    const uint32_t fbm = fwm << 2;                 // fold byte offset = K bits 10.. as a word index
    const char* const Fb = (const char*)F;
    uint32_t kk[32];
    uint32_t pass = 0u;
    uint64_t ownl = 0;   // lanes with a window equal to an earlier tile (lane masks: no VGPRs)
    // groups of 4 positions, one group's LDS reads in flight while the next
    // group rolls (as roll_probe; the sched_barrier bounds what is hoisted)
    uint32_t fwc[4], fwn[4];
    auto roll4 = [&](int g, uint32_t (&fw)[4]) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int j = 4 * g + t;
        kk[j] = (NX1 << 20) + NX2;
        if (j < 31) {
          const uint32_t xo = byte_of(xa[j >> 2], j & 3);
          const uint32_t xn = byte_of(xb[j >> 2], j & 3);
          NX1 += xo - xn;
          NX2 += NX1 + (xo << 11);
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) fw[t] = *(const uint32_t*)(Fb + ((kk[4 * g + t] >> 8) & fbm));
    };
    auto roll = [&](auto own_t) {
      constexpr bool OWN = decltype(own_t)::value;
      roll4(0, fwc);
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        if (g < 7) roll4(g + 1, fwn);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int j = 4 * g + t;
          // gfilt_test as two bit extracts (v_bfe takes the offset mod 32)
          const uint32_t b = __builtin_amdgcn_ubfe(fwc[t], kk[j], 1u) & __builtin_amdgcn_ubfe(fwc[t], kk[j] >> 5, 1u);
          pass |= b << j;
          if (OWN) ownl |= lanes_eq(kk[j], ko);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (g < 7) {
#pragma unroll
          for (int t = 0; t < 4; ++t) fwc[t] = fwn[t];
        }
      }
    };
    if (i > 0) roll(std::integral_constant<bool, true>{});
    else roll(std::integral_constant<bool, false>{});
    pass &= vm;
    if (ownl) {
      needy = true;
      break;
    }
    // the fold's passes, queued for the probe (stores only: nothing waits)
    const uint32_t cnt = (uint32_t)__builtin_popcount(pass);
    const uint32_t incl = wave_incl_scan(cnt);
    const uint32_t tot = readlane(incl, 63);
    if (qn + tot > SCREEN_QCAP) {
      needy = true;
      break;
    }
    uint32_t* const ql = q + qn + incl - cnt;
#pragma unroll
    for (int j = 0; j < 32; ++j)
      if ((pass >> j) & 1u) ql[__builtin_popcount(pass & ((1u << j) - 1u))] = kk[j];
    qn += tot;
    totXA = totXB; totTA = totTB;
  }
  if (needy) {
    verdict(SCR_NEEDY);
    return;
  }
  // the cold parse: the tiles (written above), no tail
  const uint32_t olen = (uint32_t)(2 + SEG) * (uint32_t)nt;
  // its rows, staged; against the round's old ones (a change flagged now is
  // conservative: the chunk may still go to the parse)
  bool diff = nold != (uint32_t)nt;
  uint4 nv = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int u = 0; u < SCREEN_MAXD; ++u)
    if (l == u) nv = make_uint4(tlo[u], thi[u], (uint32_t)(SEG * u), (uint32_t)(2 + SEG) * (uint32_t)(u + 1));
  if (l < nt) {
    if ((uint32_t)l < nold) diff |= ov.x != nv.x || ov.y != nv.y || ov.z != nv.z;
    st.rows[(uint64_t)chunk * SCREEN_MAXD + l] = nv;
  }
  if (ballot(diff) != 0 && l == 0) atomicMin(prm.changed, chunk);
  if (l == 0) st.qcnt[chunk] = qn;
  verdict(((uint32_t)nt << 16) | olen);
}

// Pass 1: persistent workgroups of W waves over the chunks; a wave's
// chunks chunk0, chunk0 + stride, ... in groups of 64 whose metadata lane k
// holds.
template <int W>
__global__ __launch_bounds__(64 * W) void stream_screen_kernel(ScreenParams prm, const uint32_t* fold,
                                                               uint32_t fwords, ScreenStage st) {
  __shared__ uint32_t F[SCREEN_FOLD_WORDS];
  for (uint32_t i = threadIdx.x; i < fwords / 4; i += blockDim.x) ((u32x4*)F)[i] = ((const u32x4*)fold)[i];
  const int wv = (int)readfirst(threadIdx.x >> 6);
  const uint32_t stride = gridDim.x * W;
  __syncthreads();
  for (uint32_t base = blockIdx.x * W + (uint32_t)wv; base < prm.n; base += 64u * stride) {
    const ScreenMeta meta = screen_meta(prm, base + (uint32_t)lane_id() * stride);
    ScreenLoad cur, nxt;
    screen_issue(prm, meta, 0, base, cur);
    for (int k = 0; k < 64; ++k) {
      const uint32_t chunk = base + (uint32_t)k * stride;
      if (chunk >= prm.n) break;
      if (!cur.go) {
        if (lane_id() == 0) st.info[chunk] = SCR_SKIP;
        if (k + 1 < 64) screen_issue(prm, meta, k + 1, chunk + stride, nxt);
        else nxt.go = false;
      } else {
        screen_chunk(prm, F, fwords - 1u, chunk, cur, st, nxt, meta, k + 1, chunk + stride);
      }
      cur = nxt;
    }
  }
}

// Pass 2, a wave per chunk: the queued fold passes through the global lane
// filter and the fingerprint buckets, the tiles' own windows exactly (the
// persistent cache; the batch table, where a tile is this chunk's own
// declaration and anything else a possible hit); then either the staged rows
// and counters go in, or the chunk joins the work list (work[0] counts it).
__global__ __launch_bounds__(256) void screen_finish_kernel(EncParams prm, ScreenStage st, uint32_t* work) {
  const uint32_t c = blockIdx.x * 4u + readfirst(threadIdx.x >> 6);
  const int l = lane_id();
  if (c >= prm.n) return;
  // One round trip for the verdict and what a screened chunk's check starts
  // from (the staged count and rows are read whatever the verdict; a skipped
  // or needy chunk ignores them).
  const uint32_t info0 = st.info[c];
  const uint32_t qn0 = st.qcnt[c];
  const uint4 r0 = l < SCREEN_MAXD ? st.rows[(uint64_t)c * SCREEN_MAXD + l] : make_uint4(0u, 0u, 0u, 0u);
  const uint32_t ns0 = *prm.nseg;
  const uint32_t info = readfirst(info0);
  if (info & SCR_SKIP) return;
  bool needy = (info & SCR_NEEDY) != 0u;
  const uint32_t nt = (info >> 16) & 0xFFu;
  uint4 r = make_uint4(0u, 0u, 0u, 0u);
  if (!needy) {
    const uint32_t qn = readfirst(qn0);
    const uint32_t* const q = st.qkeys + (uint64_t)c * SCREEN_QCAP;
    const bool tile = (uint32_t)l < nt;
    if (tile) r = r0;
    // the tiles' own windows: their first probe slots in the persistent cache
    // and the batch table load with the first keys (a second round trip, not
    // a chain of them after the keys')
    const uint64_t key = ((uint64_t)r.y << 32) | r.x;
    const bool gl = tile && readfirst(ns0) != 0u, bl = tile && prm.use_b;
    const uint32_t ig = tab_slot(r.x, r.y, prm.g.mask), ib = prm.use_b ? tab_slot(r.x, r.y, prm.b.mask) : 0u;
    uint64_t kg = EMPTY_KEY, vg = 0ull, kb = EMPTY_KEY, vb = 0ull;
    if (gl) { kg = prm.g.keys[ig]; vg = prm.g.vals[ig]; }
    if (bl) { kb = prm.b.keys[ib]; vb = prm.b.vals[ib]; }
    bool hit = false;
    // up to 8 keys per lane in flight: their filter words, then (rarely) buckets
    for (uint32_t j0 = 0; j0 < qn; j0 += 512) {
      uint32_t k[8], w[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const uint32_t j = j0 + 64u * t + (uint32_t)l;
        k[t] = j < qn ? q[j] : 0u;
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const uint32_t j = j0 + 64u * t + (uint32_t)l;
        w[t] = j < qn ? prm.lf.gfilt[gfilt_word(k[t], prm.lf.gmask)] : 0u;
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const uint32_t j = j0 + 64u * t + (uint32_t)l;
        if (j < qn && gfilt_test(w[t], k[t])) hit |= ftab_match(prm.lf.ftab[fbucket(k[t], prm.lf.fmask)], k[t]);
      }
    }
    // (a tile is in the batch table as this chunk's own declaration; anything
    // else there or in the persistent cache is a possible hit)
    if (gl && (kg == key ? vg : (kg == EMPTY_KEY ? ~0ull : tab_probe_rest_t(prm.g, key, ig))) != ~0ull) hit = true;
    if (bl) {
      const uint64_t bv = kb == key ? vb : (kb == EMPTY_KEY ? ~0ull : tab_probe_rest_t(prm.b, key, ib));
      if (bv != ~0ull && ((uint32_t)(bv >> 32) < c || ((uint32_t)(bv >> 32) == c && (uint32_t)bv != r.z))) hit = true;
    }
    needy = ballot(hit) != 0;
  }
  if (needy) {
    if (l == 0) work[1 + atomicAdd(work, 1u)] = c;
    return;
  }
  if ((uint32_t)l < nt) prm.decl[(uint64_t)c * prm.maxd + l] = r;
  if (l == 0) {
    prm.ndecl[c] = nt;
    prm.nhits[c] = 0u;
    prm.out_len[c] = info & 0xFFFFu;
    if (prm.stats) {
      prm.stats[4 * c + 0] = nt; prm.stats[4 * c + 1] = 0u;
      prm.stats[4 * c + 2] = 0u; prm.stats[4 * c + 3] = nt;
    }
  }
}

}  // namespace xcg

extern "C" void xcg_launch_stream_screen(const XcgStreamArgs* a, const xcg::EncParams* prm, uint32_t wgs,
                                         hipStream_t stream) {
  using namespace xcg;
  const uint32_t gwords = prm->lf.gmask + 1u;
  const uint32_t fwords = gwords < SCREEN_FOLD_WORDS ? gwords : SCREEN_FOLD_WORDS;
  hipLaunchKernelGGL(screen_fold_kernel, dim3((fwords + 255) / 256), dim3(256), 0, stream, prm->lf.gfilt, gwords,
                     a->s_fold, fwords);
  (void)hipMemsetAsync(a->s_work, 0, 4, stream);
  const ScreenStage sst{a->s_info, (uint4*)a->s_rows, a->s_qcnt, a->s_qkeys};
  const ScreenParams sp{prm->in, prm->chunk_off, prm->chunk_len, prm->out_off, prm->out, prm->decl, prm->ndecl,
                        prm->changed, prm->need, prm->n, prm->skip_below, prm->max_len, prm->maxd};
  hipLaunchKernelGGL(stream_screen_kernel<SCREEN_W>, dim3(wgs), dim3(64 * SCREEN_W), 0, stream, sp,
                     (const uint32_t*)a->s_fold, fwords, sst);
  hipLaunchKernelGGL(screen_finish_kernel, dim3((prm->n + 3) / 4), dim3(256), 0, stream, *prm, sst, a->s_work);
}
