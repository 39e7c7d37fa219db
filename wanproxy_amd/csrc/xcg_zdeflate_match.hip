// Deflate stage, first phase: a call's input laid out as X, its adler32, the hash chains over X and the match
// table tf / tq (the map of a call's arrays is at the top of xcg_zdeflate.h).
#include "xcg_zdeflate.h"

namespace xcg {
namespace zd {

// ------------------------------------------------------------------- prep
// X = history ++ data ++ zero pad, 16 bytes per thread (X and the history are
// 256-byte aligned; WSIZE and XPAD are multiples of 16, so only the vector at
// the data's end is assembled bytewise).  Grid: (tiles of 4 KiB, calls).
__global__ __launch_bounds__(256) void zd_prep_kernel(ZArgs a) {
  const ZCall c = a.calls[blockIdx.y];
  const uint64_t dend = (uint64_t)WSIZE + c.len, nv = (dend + XPAD + 15) / 16;
  uint8_t* X = a.X + c.x_off;
  const uint8_t* h = a.hist + (uint64_t)c.stream * WSIZE;
  const uint8_t* d = a.in + c.in_off;
  for (uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += (uint64_t)gridDim.x * 256) {
    const uint64_t q = 16 * v;
    u32x4 r = {0u, 0u, 0u, 0u};
    if (q < WSIZE) {
      r = *(const u32x4*)(h + q);
    } else if (q + 16 <= dend) {
      r = *(const u32x4_u*)(d + (q - WSIZE));
    } else if (q < dend) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      for (uint64_t k = 0; q + k < dend; k++) w[k >> 2] |= (uint32_t)d[q + k - WSIZE] << (8 * (k & 3));
      r = u32x4{w[0], w[1], w[2], w[3]};
    }
    *(u32x4*)(X + q) = r;
  }
}

// adler32 of the call's bytes, combined with the stream's.  Four waves per
// call read consecutive 4-byte words (coalesced); per thread sum d_i and
// sum i * d_i (i < len <= 2^24: both fit 64 bits), reduced through LDS.
__global__ __launch_bounds__(256) void zd_adler_kernel(ZArgs a) {
  __shared__ uint64_t red[2][4];
  const ZCall c = a.calls[blockIdx.x];
  const uint8_t* d = a.in + c.in_off;
  const int t = threadIdx.x;
  uint64_t A = 0, B = 0;
  const uint32_t words = c.len / 4;
#pragma unroll 4
  for (uint32_t w = t; w < words; w += 256) {
    const uint32_t v = *(const u32_u*)(d + 4ull * w);
    const uint32_t s = (v & 0xff) + ((v >> 8) & 0xff) + ((v >> 16) & 0xff) + (v >> 24);
    const uint32_t wsum = ((v >> 8) & 0xff) + 2 * ((v >> 16) & 0xff) + 3 * (v >> 24);   // in-word offsets
    A += s;
    B += (uint64_t)(4ull * w) * s + wsum;
  }
  for (uint32_t i = 4 * words + t; i < c.len; i += 256) {
    const uint32_t v = d[i];
    A += v;
    B += (uint64_t)i * v;
  }
  for (int o = 32; o >= 1; o >>= 1) {
    A += __shfl_xor(A, o);
    B += __shfl_xor(B, o);
  }
  if ((t & 63) == 0) {
    red[0][t >> 6] = A;
    red[1][t >> 6] = B;
  }
  __syncthreads();
  if (t == 0) {
    A = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) % 65521u;
    B = (red[1][0] + red[1][1] + red[1][2] + red[1][3]) % 65521u;
    uint32_t old = a.st[c.stream].adler;
    uint64_t s1 = old & 0xffff, s2 = old >> 16, n = c.len % 65521u;
    uint64_t ns1 = (s1 + A) % 65521u;
    uint64_t ns2 = (s2 + n * s1 + n * A + 65521u - B) % 65521u;
    a.res[blockIdx.x].adler = (uint32_t)((ns2 << 16) | ns1);
  }
}

// ------------------------------------------------------------------- chains
// Hash-chain links in two passes.  Groups of 64 consecutive positions start at
// the call's first valid position jlo (max(base, total - WSIZE) as an X index).
//
// zd_hashes_kernel (every group of every call in parallel): a position's 3-byte
// hash (UPDATE_HASH x3, hash_shift 5) and its nearest lower lane with the same
// hash inside the group (lanes with an equal hash found by 15 ballots, one per
// hash bit), and whether it is the group's last with that hash; packed as
// h | pred_delta << 15 | last << 21 | valid << 22.
constexpr uint32_t HGROUPS = 8;    // hash groups per wave (a call has > 512 groups: at most two calls)
__global__ __launch_bounds__(256) void zd_hashes_kernel(ZArgs a, uint32_t n, const uint32_t* gstart) {
  const uint32_t g0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * HGROUPS;   // this wave's first group
  const uint32_t total = gstart[n];
  if (g0 >= total) return;
  const int lane = threadIdx.x & 63;
  const uint32_t c0 = call_of_wave(gstart, n, g0, lane);
  const uint32_t s0 = gstart[c0], split = gstart[c0 + 1];
  const ZCall cA = a.calls[c0];
  const ZCall cB = (split < g0 + HGROUPS && c0 + 1 < n) ? a.calls[c0 + 1] : cA;
  const ZState sA = a.st[cA.stream], sB = a.st[cB.stream];
  const int64_t jloA = first_valid(sA), jloB = first_valid(sB);
  // deflate_fast: is X index j of a call hashed (zlib's INSERT_STRING)?
  auto hashed = [&](bool B, int32_t j) -> bool {
    const ZCall& c = B ? cB : cA;
    const ZState& st = B ? sB : sA;
    if (j >= WSIZE - (int32_t)st.dlen) return (a.mcur[c.m_off + (uint32_t)(j >> 5)] >> (j & 31)) & 1u;
    const uint64_t q = st.total - WSIZE + (uint64_t)j;
    return (a.ring[(uint64_t)c.stream * (WSIZE / 32) + ((q & (WSIZE - 1)) >> 5)] >> (q & 31)) & 1u;
  };
  // per group (wave-uniform): the call's X base, the group's first position, the call's end
  auto group = [&](uint32_t k, const uint8_t*& x, int32_t& g, int32_t& jend) {
    const uint32_t gid = g0 + k;
    const bool B = gid >= split;
    x = a.X + (B ? cB.x_off : cA.x_off);
    g = (int32_t)((B ? jloB : jloA) + 64ll * (gid - (B ? split : s0)));
    jend = gid < total ? WSIZE + (int32_t)(B ? cB.len : cA.len) : 0;
  };
  uint32_t w[HGROUPS];
#pragma unroll
  for (uint32_t k = 0; k < HGROUPS; k++) {   // all loads first
    const uint8_t* x;
    int32_t g, jend;
    group(k, x, g, jend);
    const int32_t j = g + lane;
    w[k] = j + 2 < jend ? *(const u32_u*)(x + j) : 0u;
  }
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
#pragma unroll
  for (uint32_t k = 0; k < HGROUPS; k++) {
    const uint8_t* x;
    int32_t g, jend;
    group(k, x, g, jend);
    const int32_t j = g + lane;
    bool valid = j + 2 < jend;
    if (a.fast && valid) valid = hashed(g0 + k >= split, j);   // a position zlib never hashes: no link, not a head
    uint32_t h = 0x8000u;    // invalid lanes form their own class
    if (valid) h = (((w[k] & 0xff) << 10) ^ (((w[k] >> 8) & 0xff) << 5) ^ ((w[k] >> 16) & 0xff)) & 0x7fffu;
    uint64_t m = ballot(valid);
#pragma unroll
    for (int b = 0; b < 15; b++) {
      const bool bit = (h >> b) & 1;
      const uint64_t bl = ballot(bit);
      m &= bit ? bl : ~bl;
    }
    const uint64_t lower = m & below;
    const uint32_t pd = lower ? (uint32_t)(lane - (63 - __clzll(lower))) : 0u;
    const uint32_t last = (m >> lane) == 1ull ? 1u : 0u;
    if (j < jend)
      a.pk[(uint64_t)(x - a.X) + j] = (h & 0x7fffu) | (pd << 15) | (last << 21) | ((valid ? 1u : 0u) << 22);
  }
}

// zd_chain_kernel (one wave per call, groups in order): a position's previous
// occurrence is its in-group predecessor, else the LDS head table; the last of
// each hash in the group becomes the head.  The head table keeps the low 16
// bits of positions (64 KiB); an entry's age is (j - v) mod 2^16, valid for
// 1..32767 (farther links are 0 anyway).  Every 32768 positions entries aged
// 0 or above 32767 are expired (set to age 32768), so between expiries every
// live entry's true age stays below 65536 and its 16-bit age is exact.  The
// packed hashes of the next 1024 positions are loaded into registers while
// the current ones are linked, and the links leave from registers: the group
// loop touches LDS only.
constexpr int CG = 16;   // groups per tile
__global__ __launch_bounds__(64) void zd_chain_kernel(ZArgs a) {
  __shared__ uint16_t head[32768];
  const ZCall c = a.calls[blockIdx.x];
  const ZState s = a.st[c.stream];
  const int lane = threadIdx.x;
  uint16_t* d16 = a.d16 + c.x_off;
  const uint32_t* pk = a.pk + c.x_off;
  const int64_t jlo = first_valid(s);
  const uint16_t empty = (uint16_t)(jlo + 32768);   // age 32768 at jlo, expired again at jlo + 32768
  for (int i = lane; i < 32768; i += 64) head[i] = empty;
  __syncthreads();
  const int64_t jend = (int64_t)WSIZE + c.len;
  int64_t next_expiry = jlo + 32768;   // tiles are 1024 positions from jlo: expiry falls on a tile start
  uint32_t cur[CG], nxt[CG];
#pragma unroll
  for (int k = 0; k < CG; k++) {
    const int64_t q = jlo + 64 * k + lane;
    cur[k] = q < jend ? pk[q] : 0u;
  }
  for (int64_t t0 = jlo; t0 < jend; t0 += 64 * CG) {
#pragma unroll
    for (int k = 0; k < CG; k++) {
      const int64_t q = t0 + 64 * (CG + k) + lane;
      nxt[k] = q < jend ? pk[q] : 0u;
    }
    if (t0 == next_expiry) {
      next_expiry += 32768;
      const uint32_t far = (uint16_t)(t0 + 32768);
      uint64_t* h64 = (uint64_t*)head;
#pragma unroll 8
      for (int i = lane; i < 8192; i += 64) {
        const uint64_t v = h64[i];
        uint64_t r = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
          const uint16_t e = (uint16_t)(v >> (16 * b));
          const uint16_t age = (uint16_t)((uint16_t)t0 - e);
          r |= (uint64_t)((age == 0 || age > 32767) ? (uint16_t)far : e) << (16 * b);
        }
        if (r != v) h64[i] = r;
      }
      __syncthreads();
    }
    uint16_t lk[CG];
#pragma unroll
    for (int k = 0; k < CG; k++) {
      const uint32_t e = cur[k];
      const int64_t j = t0 + 64 * k + lane;
      const uint32_t h = e & 0x7fffu, pd = (e >> 15) & 63u;
      int32_t age = 0;
      if (e >> 22) age = pd ? (int32_t)pd : (int32_t)(uint16_t)((uint16_t)j - head[h]);
      lk[k] = (age > 0 && age <= 32767) ? (uint16_t)age : 0;
      if ((e >> 22) && ((e >> 21) & 1)) head[h] = (uint16_t)j;
    }
#pragma unroll
    for (int k = 0; k < CG; k++) {
      const int64_t q = t0 + 64 * k + lane;
      if (q < jend) d16[q] = lk[k];
      cur[k] = nxt[k];
    }
  }
}

// ------------------------------------------------------------------- match table

// Entry: M (9 bits) | distance of the first candidate reaching M (15 bits) << 9
// | ELIG << 31 (chain head exists, within MAX_DIST, lookahead >= 3).  The scan
// also rejects a head at zlib's window coord 0 (NIL).
// Entries are indexed t = X index - WSIZE + DMAX: positions a stopped flush
// call left (the last s.dlen before the call's bytes) are parsed again now,
// with this call's bytes as their lookahead.
__global__ __launch_bounds__(256) void zd_match_kernel(ZArgs a) {
  const uint32_t ci = call_of(a.mstart, a.n, blockIdx.x);
  const ZCall c = a.calls[ci];
  const uint32_t t = (blockIdx.x - a.mstart[ci]) * 256u + threadIdx.x;
  const ZState s = a.st[c.stream];
  if (t < (uint32_t)DMAX - s.dlen || t >= (uint32_t)DMAX + c.len) return;
  const int64_t rel = (int64_t)t - DMAX;
  const uint8_t* X = a.X + c.x_off;
  const uint16_t* d16 = a.d16 + c.x_off;
  const int64_t j = (int64_t)WSIZE + rel;
  const int64_t la = (int64_t)c.len - rel;
  uint32_t ef = 0, eq = 0;
  uint32_t d = la >= MIN_MATCH ? d16[j] : 0;
  if (d != 0 && d <= (uint32_t)MAX_DIST) {
    const int budget = CFG[a.level][3], qb = budget >> 2;
    const int cap = la < MAX_MATCH ? (int)la : MAX_MATCH;
    const int nice = CFG[a.level][2] < cap ? CFG[a.level][2] : cap;
    // chain continues while cur > max(p - MAX_DIST, stream position 0)
    int64_t limit = j - MAX_DIST;
    int64_t zero = (int64_t)WSIZE - (int64_t)s.total;
    if (zero > limit) limit = zero;
    int64_t cur = j - d;
    int best = 0, bq = -1;
    int64_t bs = 0, bsq = 0;
    const uint32_t x01 = *(const u16_u*)(X + j);
    int count = 0;
    for (;;) {
      // the next link is loaded with the candidate's bytes (both depend on cur only)
      const uint32_t dd = d16[cur];
      // longest_match: reject on bytes 0, 1 (and at best_len), then compare
      if (*(const u16_u*)(X + cur) == x01 && (best < 3 || X[cur + best] == X[j + best])) {
        int len = 2;
        while (len < cap) {
          uint32_t w = ld32(X + cur + len) ^ ld32(X + j + len);
          if (w) {
            len += __builtin_ctz(w) >> 3;
            break;
          }
          len += 4;
        }
        if (len > cap) len = cap;
        if (len >= MIN_MATCH && len > best) {
          best = len;
          bs = cur;
          if (len >= nice) break;
        }
      }
      if (++count == qb) {
        bq = best;
        bsq = bs;
      }
      if (count >= budget) break;
      if (dd == 0) break;
      cur -= dd;
      if (cur <= limit) break;
    }
    if (bq < 0) {
      bq = best;
      bsq = bs;
    }
    ef = 0x80000000u | (uint32_t)best | (best ? (uint32_t)(j - bs) << 9 : 0);
    eq = 0x80000000u | (uint32_t)bq | (bq ? (uint32_t)(j - bsq) << 9 : 0);
  }
  a.tf[c.t_off + t] = ef;
  a.tq[c.t_off + t] = eq;
}

// ------------------------------------------------------------------- launches
void zd_launch_prep(const ZArgs& a, uint32_t maxlen, hipStream_t st) {
  uint32_t prep_tiles = std::min<uint32_t>(64, ((uint32_t)WSIZE + maxlen + XPAD + 4095) / 4096);
  hipLaunchKernelGGL(zd_prep_kernel, dim3(prep_tiles, a.n), dim3(256), 0, st, a);
}
void zd_launch_adler(const ZArgs& a, hipStream_t st) { hipLaunchKernelGGL(zd_adler_kernel, dim3(a.n), dim3(256), 0, st, a); }
void zd_launch_match(const ZArgs& a, uint32_t groups, uint32_t mtiles, hipStream_t st) {
  const unsigned hgrid = (groups + 4 * HGROUPS - 1) / (4 * HGROUPS);
  hipLaunchKernelGGL(zd_hashes_kernel, dim3(hgrid), dim3(256), 0, st, a, a.n, a.gstart);
  hipLaunchKernelGGL(zd_chain_kernel, dim3(a.n), dim3(64), 0, st, a);
  if (mtiles) hipLaunchKernelGGL(zd_match_kernel, dim3(mtiles), dim3(256), 0, st, a);
}

}  // namespace zd
}  // namespace xcg
