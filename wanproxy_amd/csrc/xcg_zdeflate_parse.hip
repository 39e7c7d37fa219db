// Deflate stage, second phase: the two parsers over the match table (deflate_slow for levels 4-9, deflate_fast
// for 1-3) and deflate_fast's hashed-position masks (the map of a call's arrays is at the top of xcg_zdeflate.h).
#include "xcg_zdeflate.h"

namespace xcg {
namespace zd {

// ------------------------------------------------------------------- parse frame
struct ScanWin {
  uint32_t tf, tq, x;   // lane l: entries of position w + l, X byte w - 1 + l
  uint32_t d;
};

__device__ __forceinline__ void load_win(ScanWin& W, const ZArgs& a, const ZCall& c, int64_t w, int64_t p0) {
  const int lane = threadIdx.x;
  int64_t rel = w - WSIZE + lane;
  W.tf = 0;
  W.tq = 0;
  W.d = 0;
  if (w + lane >= p0 && rel < (int64_t)c.len) {
    W.tf = a.tf[c.t_off + rel + DMAX];
    W.tq = a.tq[c.t_off + rel + DMAX];
    W.d = a.d16[c.x_off + w + lane];
  }
  W.x = (rel - 1 < (int64_t)c.len) ? a.X[c.x_off + w - 1 + lane] : 0;
}

constexpr uint32_t SBUF = 2048;   // symbols staged in LDS before they leave (a kernel's sbuf holds SBUF + 64)

// What deflate_slow and deflate_fast share, one wave per call: zlib's window
// over the call's X, the two 64-position windows of the match table, the
// symbols on their way out and the block records.  A kernel keeps its own
// loop top and its literal-run test.
struct ParseFrame {
  // positions are X indices; bidx = X index of zlib's window coord 0.  The
  // parse resumes where the last call's left it (strstart = total - dlen, with
  // its lazy-match state); data was read up to `total`.
  int64_t bidx, end, p0, p, rd, block_start;
  uint32_t nsym, symbase, nblk;
  ScanWin W, N;   // entries of [w, w + 64) and, loaded ahead, [w + 64, w + 128)
  int64_t w;
  // Symbols are staged in LDS and written out 2048 at a time (coalesced): a
  // store per symbol would make every window load wait for all earlier
  // stores (gfx9 counts both in vmcnt).
  uint32_t* sbuf;
  uint32_t sb_n, sb_base;
  uint32_t* sym;
  ZBlock* blk;
  int lane;

  __device__ __forceinline__ void init(const ZArgs& a, const ZCall& c, const ZState& s, uint32_t* lds) {
    lane = threadIdx.x;
    sym = a.sym + c.t_off;
    blk = a.blk + c.blk_off;
    bidx = (int64_t)s.base - (int64_t)s.total + WSIZE;
    end = (int64_t)WSIZE + c.len;
    p0 = (int64_t)WSIZE - s.dlen;
    p = p0, rd = WSIZE;
    nsym = symbase = nblk = 0;
    block_start = (int64_t)s.block_start - (int64_t)s.total + WSIZE;
    w = p;
    load_win(W, a, c, w, p0);
    load_win(N, a, c, w + 64, p0);
    sbuf = lds, sb_n = sb_base = 0;
  }
  // fill_window, for a loop top with less than MIN_LOOKAHEAD ahead: slide, then read what fits; nothing ahead
  // after it (rd == p) ends the parse.  (Both tests stay in the kernels: profiles/zdeflate_split_ab.txt.)
  __device__ __forceinline__ void fill_window() {
    do {
      int64_t more = WINSZ - (rd - bidx);
      if (p - bidx >= WSIZE + MAX_DIST) {
        bidx += WSIZE;
        more += WSIZE;
      }
      if (rd == end) break;
      int64_t nrd = end - rd;
      if (nrd > more) nrd = more;
      rd += nrd;
    } while (rd - p < MIN_LOOKAHEAD && rd < end);
  }
  // W covers p again
  __device__ __forceinline__ void advance(const ZArgs& a, const ZCall& c) {
    if (p >= w + 64) {
      if (p < w + 128) {
        W = N;
        w += 64;
      } else {
        w = p;
        load_win(W, a, c, w, p0);
      }
      load_win(N, a, c, w + 64, p0);
    }
  }
  // where a literal run from p must end: W's end, the last position with
  // MIN_LOOKAHEAD bytes of lookahead, the block's last symbol
  __device__ __forceinline__ int64_t run_limit() const {
    int64_t lim = w + 64;
    if (rd - (MIN_LOOKAHEAD - 1) < lim) lim = rd - (MIN_LOOKAHEAD - 1);
    const int64_t room = SYMS_PER_BLOCK - nsym;
    if (p + room < lim) lim = p + room;
    return lim;
  }
  __device__ __forceinline__ void sflush() {
    for (uint32_t i = lane; i < sb_n; i += 64) sym[sb_base + i] = sbuf[i];
    sb_base += sb_n;
    sb_n = 0;
  }
  __device__ __forceinline__ void put(uint32_t v) {
    if (lane == 0) sbuf[sb_n] = v;
    sb_n++;
    nsym++;
    if (sb_n >= SBUF) sflush();
  }
  // k literals at once: lane li + i holds the i-th in v
  __device__ __forceinline__ void put_run(int li, int64_t k, uint32_t v) {
    if (lane >= li && lane < li + k) sbuf[sb_n + (lane - li)] = v;
    sb_n += (uint32_t)k;
    nsym += (uint32_t)k;
    if (sb_n >= SBUF) sflush();
  }
  // FLUSH_BLOCK at strstart q; `tail`: inside the flush call (loop-top
  // lookahead < MIN_LOOKAHEAD, or the final flush); the parse then stands at
  // (p_after, ms, avail, ml) -- where a consume that stops at this flush resumes
  __device__ __forceinline__ void end_block(int64_t q, bool last, bool tail, int64_t p_after, int64_t ms, int avail,
                                            int ml) {
    if (lane == 0) {
      ZBlock b;
      b.sym_begin = symbase;
      b.sym_end = symbase + nsym;
      b.start = (uint32_t)block_start;
      b.stored_len = (uint32_t)(q - block_start);
      b.flags = (block_start >= bidx ? 1u : 0u) | (last ? 2u : 0u) | (tail ? 4u : 0u);
      b.type = 0;
      b.lcodes = b.dcodes = b.blcodes = b.pad = 0;
      b.bits = 0;
      b.bit_off = 0;
      b.bidx = bidx;
      b.p_after = (uint32_t)p_after;
      b.ms = (uint32_t)ms;
      b.avail = (uint32_t)avail;
      b.ml = (uint32_t)ml;
      blk[nblk] = b;
    }
    nblk++;
    symbase += nsym;
    nsym = 0;
    block_start = q;
  }
  // the call's final flush (Z_FINISH on an empty call) and what the parse leaves for the later kernels
  __device__ __forceinline__ void finish(const ZArgs& a, uint32_t ci, const ZCall& c, const ZState& s, int64_t ms) {
    if (c.len == 0) end_block(p, true, true, p, ms, 0, MIN_MATCH - 1);
    else if (nsym) end_block(p, false, true, p, ms, 0, MIN_MATCH - 1);
    if (lane == 0) {
      ZCallRes r = a.res[ci];
      r.nblocks = nblk;
      r.nsym = symbase;
      r.base_end = (uint64_t)((int64_t)s.total - WSIZE + bidx);
      r.scan_end = (uint32_t)p;
      a.res[ci] = r;
    }
  }
};

// ------------------------------------------------------------------- lazy scan
// deflate_slow (deflate.c) over the match table; one wave per call.
__global__ __launch_bounds__(64) void zd_scan_kernel(ZArgs a) {
  __shared__ uint32_t sbuf[SBUF + 64];
  const uint32_t ci = blockIdx.x;
  const ZCall c = a.calls[ci];
  const ZState s = a.st[c.stream];
  const int lane = threadIdx.x;
  const int good = CFG[a.level][0], lazy = CFG[a.level][1];
  int ml = (int)s.mlen, avail = (int)s.avail;   // (the lazy-match state first: see profiles/zdeflate_split_ab.txt)
  int64_t ms = (int64_t)s.mstart - (int64_t)s.total + WSIZE;
  ParseFrame f;
  f.init(a, c, s, sbuf);
#ifdef XCG_ZD_TIMING
  uint64_t n_fast = 0, n_slow = 0, n_fastpos = 0, t_scan = ZD_NOW();
#endif

  for (;;) {
    if (f.rd - f.p < MIN_LOOKAHEAD) {
      f.fill_window();
      if (f.rd == f.p) break;
    }
    f.advance(a, c);
    const int li = (int)(f.p - f.w);
    if (avail && ml == MIN_MATCH - 1) {
      // literal run: positions where no match can start emit the previous byte
      const int64_t lim = f.run_limit();
      if (lim > f.p) {
        uint32_t M = f.W.tf & 511u, dist = (f.W.tf >> 9) & 0x7fffu;
        int64_t pos = f.w + lane;
        bool elig = (f.W.tf >> 31) && pos - (int64_t)f.W.d != f.bidx && M >= MIN_MATCH && !(M == MIN_MATCH && dist > TOO_FAR);
        uint64_t m = ballot(elig && pos >= f.p && pos < lim);
        int64_t stop = m ? f.w + (int64_t)__builtin_ctzll(m) : lim;
        int64_t k = stop - f.p;
        if (k > 0) {
          f.put_run(li, k, f.W.x);
          f.p = stop;
#ifdef XCG_ZD_TIMING
          n_fast++;
          n_fastpos += (uint64_t)k;
#endif
          if (f.nsym == SYMS_PER_BLOCK) f.end_block(f.p - 1, false, false, f.p, ms, 1, MIN_MATCH - 1);
          continue;
        }
      }
    }
    // one loop top of deflate_slow at p
#ifdef XCG_ZD_TIMING
    n_slow++;
#endif
    const uint32_t ef = readlane(f.W.tf, li), dd = readlane(f.W.d, li);
    const int64_t la = f.rd - f.p;
    int prev_length = ml;
    int64_t prev_match = ms;
    ml = MIN_MATCH - 1;
    bool head_ok = la >= MIN_MATCH && (ef >> 31) && (f.p - (int64_t)dd != f.bidx);
    if (head_ok && prev_length < lazy) {
      uint32_t e = prev_length >= good ? readlane(f.W.tq, li) : ef;
      int M = (int)(e & 511u);
      if (M > prev_length) {
        ml = M;
        ms = f.p - (int64_t)((e >> 9) & 0x7fffu);
      } else {
        ml = (int64_t)prev_length <= la ? prev_length : (int)la;
      }
      if (ml == MIN_MATCH && f.p - ms > TOO_FAR) ml = MIN_MATCH - 1;
    }
    if (prev_length >= MIN_MATCH && ml <= prev_length) {
      f.put((uint32_t)(prev_length - MIN_MATCH) | ((uint32_t)(f.p - 1 - prev_match) << 8));
      f.p += prev_length - 1;
      avail = 0;
      ml = MIN_MATCH - 1;
      if (f.nsym == SYMS_PER_BLOCK) f.end_block(f.p, false, la < MIN_LOOKAHEAD, f.p, ms, 0, MIN_MATCH - 1);
    } else if (avail) {
      f.put(readlane(f.W.x, li));
      if (f.nsym == SYMS_PER_BLOCK) f.end_block(f.p, false, la < MIN_LOOKAHEAD, f.p + 1, ms, 1, ml);
      f.p++;
    } else {
      avail = 1;
      f.p++;
    }
  }
  if (avail) f.put(a.X[c.x_off + f.p - 1]);
  f.sflush();
#ifdef XCG_ZD_TIMING
  if (lane == 0) {
    atomicAdd(&g_zd_t[5], (unsigned long long)n_slow);
    atomicAdd(&g_zd_t[6], (unsigned long long)n_fast);
    atomicAdd(&g_zd_t[7], (unsigned long long)n_fastpos);
    atomicAdd(&g_zd_t[11], (unsigned long long)(ZD_NOW() - t_scan));
    atomicAdd(&g_zd_t[12], 1ull);
  }
#endif
  f.finish(a, ci, c, s, ms);
}

// ------------------------------------------------------------------- deflate_fast
// deflate_fast (deflate.c, levels 1-3) over the match table built from this
// round's hashed-position guess (ZArgs::mcur); one wave per call.  zlib hashes
// every loop top with >= MIN_MATCH bytes of lookahead and the inside of a match
// only when it is at most max_lazy (= max_insert_length) long and leaves >=
// MIN_MATCH bytes of lookahead; the positions this parse hashes go to mnext.
// When mnext == mcur the table was zlib's (by induction over positions: a
// loop top's chain holds exactly the positions hashed before it) and so is
// the parse.
__device__ __forceinline__ void mark_range(uint32_t* mk, int64_t lo, int64_t hi, int lane) {
  if (hi <= lo) return;
  const int64_t w0 = lo >> 5, w1 = (hi - 1) >> 5;
  for (int64_t wd = w0 + lane; wd <= w1; wd += 64) {
    const int64_t b0 = wd * 32, a0 = lo > b0 ? lo - b0 : 0, a1 = hi < b0 + 32 ? hi - b0 : 32;
    const uint32_t m = (a1 - a0 == 32) ? ~0u : (((1u << (a1 - a0)) - 1u) << a0);
    atomicOr(mk + wd, m);
  }
}

// (A block ends at strstart q after its symbol, with no lazy-match state: end_block(.., q, 0, 0, MIN_MATCH - 1).)
__global__ __launch_bounds__(64) void zd_fscan_kernel(ZArgs a) {
  __shared__ uint32_t sbuf[SBUF + 64];
  const uint32_t ci = blockIdx.x;
  const ZCall c = a.calls[ci];
  const ZState s = a.st[c.stream];
  const int lane = threadIdx.x;
  const int max_insert = CFG[a.level][1];
  uint32_t* mk = a.mnext + c.m_off;
  ParseFrame f;
  f.init(a, c, s, sbuf);
  for (;;) {
    if (f.rd - f.p < MIN_LOOKAHEAD) {
      f.fill_window();
      if (f.rd == f.p) break;
    }
    f.advance(a, c);
    const int li = (int)(f.p - f.w);
    // X[w + lane] (W.x holds X[w - 1 + lane])
    uint32_t xs = __shfl(f.W.x, (lane + 1) & 63);
    const uint32_t nx0 = readlane(f.N.x, 0);
    if (lane == 63) xs = nx0;
    {
      // literal run: loop tops where no match starts (all hashed, lookahead >= MIN_LOOKAHEAD)
      const int64_t lim = f.run_limit();
      if (lim > f.p) {
        const int64_t pos = f.w + lane;
        const bool elig = (f.W.tf >> 31) && pos - (int64_t)f.W.d != f.bidx && (f.W.tf & 511u) >= MIN_MATCH;
        const uint64_t m = ballot(elig && pos >= f.p && pos < lim);
        const int64_t stop = m ? f.w + (int64_t)__builtin_ctzll(m) : lim;
        const int64_t k = stop - f.p;
        if (k > 0) {
          f.put_run(li, k, xs);
          mark_range(mk, f.p, stop, lane);
          f.p = stop;
          if (f.nsym == SYMS_PER_BLOCK) f.end_block(f.p, false, false, f.p, 0, 0, MIN_MATCH - 1);
          continue;
        }
      }
    }
    // one loop top of deflate_fast at p
    const uint32_t ef = readlane(f.W.tf, li), dd = readlane(f.W.d, li);
    const int64_t la = f.rd - f.p;
    if (la >= MIN_MATCH && lane == 0) atomicOr(mk + (f.p >> 5), 1u << (f.p & 31));   // INSERT_STRING
    const bool head_ok = la >= MIN_MATCH && (ef >> 31) && (f.p - (int64_t)dd != f.bidx);
    const int ml = head_ok ? (int)(ef & 511u) : 0;
    if (ml >= MIN_MATCH) {
      f.put((uint32_t)(ml - MIN_MATCH) | (((ef >> 9) & 0x7fffu) << 8));
      if (ml <= max_insert && la - ml >= MIN_MATCH) mark_range(mk, f.p + 1, f.p + ml, lane);
      f.p += ml;
    } else {
      f.put(readlane(xs, li));
      f.p++;
    }
    if (f.nsym == SYMS_PER_BLOCK) f.end_block(f.p, false, la < MIN_LOOKAHEAD, f.p, 0, 0, MIN_MATCH - 1);
  }
  f.sflush();
  // s->insert = min(strstart, MIN_MATCH - 1): the last positions are hashed once their bytes exist
  const int64_t ins = f.p - f.bidx < MIN_MATCH - 1 ? f.p - f.bidx : MIN_MATCH - 1;
  mark_range(mk, f.p - ins, f.p, lane);
  f.finish(a, ci, c, s, 0);
}

// mnext == mcur over the positions the call parses? (changed[ci] = 1 if not)
__global__ __launch_bounds__(256) void zd_mcmp_kernel(ZArgs a) {
  const uint32_t ci = blockIdx.x;
  const ZCall c = a.calls[ci];
  const ZState s = a.st[c.stream];
  const int64_t lo = (int64_t)WSIZE - s.dlen, hi = (int64_t)WSIZE + c.len;
  bool diff = false;
  for (int64_t wd = (lo >> 5) + threadIdx.x; wd <= ((hi - 1) >> 5); wd += 256) {
    const int64_t b0 = wd * 32, a0 = lo > b0 ? lo - b0 : 0, a1 = hi < b0 + 32 ? hi - b0 : 32;
    const uint32_t m = (a1 - a0 == 32) ? ~0u : (((1u << (a1 - a0)) - 1u) << a0);
    if ((a.mcur[c.m_off + wd] ^ a.mnext[c.m_off + wd]) & m) diff = true;
  }
  if (__syncthreads_or(diff) && threadIdx.x == 0) a.changed[ci] = 1u;
}

// Round 0's guess: every position hashed.  Also clears mnext.
__global__ __launch_bounds__(256) void zd_mfill_kernel(uint32_t* m, uint32_t* mn, uint64_t words) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (uint64_t)gridDim.x * 256) {
    m[i] = ~0u;
    mn[i] = 0u;
  }
}
__global__ __launch_bounds__(256) void zd_mzero_kernel(uint32_t* m, uint64_t words) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (uint64_t)gridDim.x * 256) m[i] = 0u;
}

// The stream's ring of hashed positions after the call: bit (q mod 32768) for
// the last 32 KiB; positions from strstart on come from the final mask.
__global__ __launch_bounds__(256) void zd_ring_kernel(ZArgs a) {
  const uint32_t ci = blockIdx.x;
  const ZCall c = a.calls[ci];
  const ZState s = a.st[c.stream];
  const uint64_t hi = s.total + c.len, p0 = s.total - s.dlen;
  const uint64_t lo = hi > (uint64_t)WSIZE ? hi - WSIZE : 0;
  const uint64_t from = p0 > lo ? p0 : lo;
  uint32_t* ring = a.ring + (uint64_t)c.stream * (WSIZE / 32);
  const uint32_t* mk = a.mcur + c.m_off;
  for (uint32_t r = threadIdx.x; r < (uint32_t)WSIZE / 32; r += 256) {
    uint32_t v = ring[r];
    for (int b = 0; b < 32; b++) {
      const uint64_t slot = (uint64_t)r * 32 + b;
      if (hi < (uint64_t)WSIZE && slot >= hi) continue;   // (no such position yet)
      const uint64_t q = hi - WSIZE + ((slot - hi) & (WSIZE - 1));   // the position in [hi - 32768, hi) on this slot
      if (q < from) continue;
      const uint64_t j = q - (s.total - WSIZE);
      const uint32_t bit = (mk[j >> 5] >> (j & 31)) & 1u;
      v = (v & ~(1u << b)) | (bit << b);
    }
    ring[r] = v;
  }
}

// ------------------------------------------------------------------- launches
static unsigned mask_grid(uint64_t mo) { return (unsigned)std::min<uint64_t>(4096, (mo + 255) / 256 + 1); }

void zd_launch_scan(const ZArgs& a, hipStream_t st) { hipLaunchKernelGGL(zd_scan_kernel, dim3(a.n), dim3(64), 0, st, a); }
void zd_launch_mfill(const ZArgs& a, uint64_t mo, hipStream_t st) {
  hipLaunchKernelGGL(zd_mfill_kernel, dim3(mask_grid(mo)), dim3(256), 0, st, a.mcur, a.mnext, mo);
}
void zd_launch_fscan(const ZArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(zd_fscan_kernel, dim3(a.n), dim3(64), 0, st, a);
  hipLaunchKernelGGL(zd_mcmp_kernel, dim3(a.n), dim3(256), 0, st, a);
}
void zd_launch_mzero(const ZArgs& a, uint64_t mo, hipStream_t st) {
  hipLaunchKernelGGL(zd_mzero_kernel, dim3(mask_grid(mo)), dim3(256), 0, st, a.mnext, mo);
}
void zd_launch_ring(const ZArgs& a, hipStream_t st) { hipLaunchKernelGGL(zd_ring_kernel, dim3(a.n), dim3(256), 0, st, a); }

#ifdef XCG_ZD_TIMING
bool zd_parse_times(uint64_t* acc) { return zd_times_take(acc); }
#endif

}  // namespace zd
}  // namespace xcg
