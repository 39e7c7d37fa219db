// XCodec decoder, one decode() call in one workgroup (the batch decoder's
// passes and helpers: xcg_decode.hip, xcg_decode_batch.h): one call a launch
// (decode_small_kernel), or n calls on n caches a launch (decode_calls_kernel).
//
// XCodecDecoder::decode (xcodec/xcodec_decoder.cc:66-272) of ONE call's input
// on an unbounded cache, as the drop-in adapter issues it (tack -d: one call
// per 64 KiB read, programs/tack/tack.cc:329-359; XCodecPipePair: the buffered
// frames, xcodec_pipe_pair.cc:425-446) -- the passes of the batch decoder
// (scan, hash, resolve, emit, window, commit) in one launch, with __syncthreads
// between them instead of kernel boundaries and host synchronisations.
// Wave 0 walks the ops and lists them (literal runs, EXTRACT, REF) with their
// output offsets and declare numbers; all waves hash the EXTRACTs into an LDS
// table (earliest / latest position), resolve every REF (an earlier EXTRACT
// of the call, else the cache; else it is unknown -- the first one is the stop
// point and the rest form decode_skim's set), then copy every op before the
// stop to its output offset, update the BACKREF window (window_slot over the
// call's declare records) and commit the EXTRACTs before the stop.  Anything
// this pass does not cover -- a BACKREF op, name reuse inside the call (any
// EXTRACT whose bytes differ from its hash's earliest), EXTRACTs of one hash
// on both sides of the stop, more than
// SD_XSLOTS / 2 EXTRACTs or SD_UMAX unknown hashes -- sets `fallback` before
// anything is written; the host then takes the batch path.  The result words
// and SD_UMAX, SD_EMAX, SD_LDS_IN, SD_PHASES: xcg_decode_words.h.
#include "xcg_decode_batch.h"

namespace xcg {

constexpr uint32_t SD_XSLOTS = 2048, SD_USLOTS = 4096;
constexpr uint32_t SD_LIT = 0, SD_EXT = 1, SD_REF = 2;

struct SmallDec {
  const uint8_t* in;
  uint32_t len;
  HashTab g;
  uint8_t* pool;
  uint32_t* nseg;
  uint32_t seg_cap;
  FiltSet fs;
  int32_t* status;             // the context's sticky word
  uint4* ops;                  // (type, in_off, out_off, declare number | nesc)
  uint64_t* opv;               // EXTRACT / REF hash
  uint4* D;                    // declare records (lo, hi, src lo, src hi)
  uint32_t ops_cap;
  uint8_t* out;
  uint64_t out_cap;
  uint64_t* win_hash;
  uint8_t* win_seg;
  uint64_t win_count;
  uint64_t* res;               // SD_RES_WORDS result words (SDR_*, xcg_decode_words.h)
  uint64_t* tim;               // (diagnostics, nullable) SD_PHASES clock stamps at the phase boundaries
  uint32_t* flag;              // (nullable) completion word in host memory: seq is stored there last
  uint32_t seq;
};
#define SD_STAMP(k) do { if (a.tim && threadIdx.x == 0) a.tim[k] = __builtin_amdgcn_s_memrealtime(); } while (0)

__device__ __forceinline__ void decode_small_body(const SmallDec& a) {
  __shared__ uint64_t xk[SD_XSLOTS], xf[SD_XSLOTS], xl[SD_XSLOTS];
  __shared__ uint64_t uk[SD_USLOTS];
  __shared__ uint32_t s_nops, s_ndecl, s_next, s_nunk, s_fb, s_walk_st, s_walk_end;
  __shared__ uint64_t s_stop;  // (position << 32) | declare number of the first unknown REF
  __shared__ uint64_t s_olen;
  __shared__ uint4 xin[SD_LDS_IN / 16];
  __shared__ uint16_t xlist[SD_XSLOTS / 2];                  // the occupied EXTRACT slots
  __shared__ uint16_t wcopy[256];                            // window slots that take a new segment
  __shared__ uint32_t s_nx, s_nw, s_ndup;
  const uint32_t t = threadIdx.x, w = t >> 6;
  const int l = lane_id();
  const uint32_t len = a.len;
  const uint8_t* x = a.in;
  SD_STAMP(0);
  const bool staged = len <= SD_LDS_IN;
  constexpr uint32_t SV = (SD_LDS_IN / 16 + 1023) / 1024;    // 16-byte loads per thread
  if (staged) {                                              // stage the input (all loads in flight together)
    const uint32_t nv = len / 16;
    uint4 v[SV];
#pragma unroll
    for (uint32_t j = 0; j < SV; ++j)
      if (t + 1024u * j < nv) v[j] = ((const uint4*)a.in)[t + 1024u * j];
#pragma unroll
    for (uint32_t j = 0; j < SV; ++j)
      if (t + 1024u * j < nv) xin[t + 1024u * j] = v[j];
    uint8_t* xb = (uint8_t*)xin;
    for (uint32_t i = nv * 16 + t; i < len; i += 1024) xb[i] = a.in[i];
    x = xb;
  }
  const lds_u8p xs = (lds_u8p)(const uint8_t*)xin;
  for (uint32_t i = t; i < SD_XSLOTS; i += 1024) { xk[i] = EMPTY_KEY; xf[i] = ~0ull; xl[i] = 0; }
  for (uint32_t i = t; i < SD_USLOTS; i += 1024) uk[i] = EMPTY_KEY;
  if (t == 0) {
    s_nunk = 0; s_fb = 0; s_stop = ~0ull; s_next = 0; s_ndup = 0;
    a.res[SD_RES_STICKY] = (uint64_t)(uint32_t)*a.status;   // (the paths that return early)
  }
  // (wave 0's walk reads input bytes every wave staged)
  __syncthreads();
  SD_STAMP(1);
  // ---- walk (wave 0): op list, output offsets, declare numbers
  auto walk = [&](auto xp) {
    uint32_t i = 0, k = 0, dn = 0, st = 0, fb = 0;
    uint64_t olen = 0;
    while (i < len) {
      uint32_t nesc = 0;
      const uint32_t m = next_op(xp, i, len, nesc);
      if (m > i) {                                           // literal run (:71-81, ESCAPE :91-94)
        if (k >= a.ops_cap) { fb = 1; break; }
        if (l == 0) a.ops[k] = make_uint4(SD_LIT, i, (uint32_t)olen, m - i);
        ++k;
        olen += (m - i) - nesc;
      }
      i = m;
      if (i >= len) break;
      if (len - i == 1) { st = 3; break; }
      const uint32_t op = xp[i + 1];
      if (op == OP_EXTRACT) {
        if (len - i < 2u + SEG) { st = 3; break; }
        if (k >= a.ops_cap) { fb = 1; break; }
        if (l == 0) a.ops[k] = make_uint4(SD_EXT, i, (uint32_t)olen, dn);
        ++k; ++dn;
        olen += SEG;
        i += 2 + SEG;
      } else if (op == OP_REF) {
        if (len - i < 10u) { st = 3; break; }
        uint64_t h, here;
        const uint32_t r = ref_run(xp, i, len, 0, ~0ull, h, here);
        if (k + r > a.ops_cap) { fb = 1; break; }
        if ((uint32_t)l < r) {
          a.ops[k + l] = make_uint4(SD_REF, i + 10u * l, (uint32_t)(olen + (uint64_t)SEG * l), dn + l);
          a.opv[k + l] = h;
        }
        k += r; dn += r;
        olen += (uint64_t)SEG * r;
        i += 10u * r;
      } else if (op == OP_BACKREF) {
        fb = 1;                                              // (the batch path models the window's BACKREFs)
        break;
      } else {
        st = (uint32_t)-1;                                   // :183-184 unsupported opcode
        break;
      }
    }
    if (olen >= (1ull << 32)) fb = 1;
    if (l == 0) {
      s_nops = k; s_ndecl = dn; s_walk_st = st; s_walk_end = i; s_olen = olen;
      if (fb) s_fb = 1;
    }
  };
  if (w == 0) {
    if (staged) walk(xs);
    else walk(a.in);
  }
  __syncthreads();
  SD_STAMP(2);
  const uint32_t nops = s_nops;
  if (s_fb) {
    if (t == 0) a.res[SDR_FALLBACK] = SD_FB_BATCH;
    return;
  }
  // ---- EXTRACT hashes (a wave per EXTRACT) into the LDS table
  for (uint32_t k = w; k < nops; k += 16) {
    const uint4 o = a.ops[k];
    if (readfirst(o.x) != SD_EXT) continue;
    const uint32_t pos = readfirst(o.y) + 2u;
    const uint2 h = staged ? dec_window_hash(xs + pos) : dec_window_hash(x + pos);
    const uint64_t key = ((uint64_t)readfirst(h.y) << 32) | readfirst(h.x);
    if (l == 0) {
      a.opv[k] = key;
      uint32_t i = mix32((uint32_t)key, (uint32_t)(key >> 32)) & (SD_XSLOTS - 1);
      for (uint32_t n = 0; n < SD_XSLOTS; ++n) {
        const uint64_t prev = atomicCAS((unsigned long long*)&xk[i], (unsigned long long)EMPTY_KEY, (unsigned long long)key);
        if (prev == EMPTY_KEY || prev == key) {
          atomicMin((unsigned long long*)&xf[i], (unsigned long long)pos);
          atomicMax((unsigned long long*)&xl[i], (unsigned long long)pos);
          if (prev == key) atomicAdd(&s_ndup, 1u);
          break;
        }
        i = (i + 1) & (SD_XSLOTS - 1);
      }
      atomicAdd(&s_next, 1u);
    }
  }
  if (t == 0) { s_nx = 0; s_nw = 0; }
  __syncthreads();
  SD_STAMP(3);
  if (s_next > SD_XSLOTS / 2) {
    if (t == 0) a.res[SDR_FALLBACK] = SD_FB_BATCH;
    return;
  }
  // occupied slots of the EXTRACT table, once (the precheck and the commit walk
  // only these instead of all SD_XSLOTS)
  for (uint32_t i = t; i < SD_XSLOTS; i += 1024)
    if (xk[i] != EMPTY_KEY) xlist[atomicAdd(&s_nx, 1u)] = (uint16_t)i;
  // ---- resolve every REF (a thread per op): an earlier EXTRACT of the call,
  // else the cache; else unknown (:151-156; decode_skim's set, :196-272)
  for (uint32_t k = t; k < nops; k += 1024) {
    const uint4 o = a.ops[k];
    uint64_t src = 0, key = 0;
    if (o.x == SD_EXT) {
      key = a.opv[k];
      src = (uint64_t)(x + o.y + 2);
    } else if (o.x == SD_REF) {
      key = a.opv[k];
      const uint64_t here = o.y;
      uint32_t i = mix32((uint32_t)key, (uint32_t)(key >> 32)) & (SD_XSLOTS - 1);
      uint64_t e = ~0ull;
      for (uint32_t n = 0; n < SD_XSLOTS; ++n) {
        const uint64_t kk = xk[i];
        if (kk == key) { e = xf[i]; break; }
        if (kk == EMPTY_KEY) break;
        i = (i + 1) & (SD_XSLOTS - 1);
      }
      if (e != ~0ull && e < here) {
        src = (uint64_t)(x + e);
      } else {
        const uint64_t gv = tab_lookup_t(a.g, (uint32_t)key, (uint32_t)(key >> 32));
        if (gv != ~0ull) {
          src = (uint64_t)(a.pool + gv * (uint64_t)SEG);
        } else {
          atomicMin((unsigned long long*)&s_stop, (unsigned long long)((here << 32) | o.w));
          uint32_t j = mix32((uint32_t)key, (uint32_t)(key >> 32)) & (SD_USLOTS - 1);
          for (uint32_t n = 0; n < SD_USLOTS; ++n) {
            const uint64_t prev = atomicCAS((unsigned long long*)&uk[j], (unsigned long long)EMPTY_KEY,
                                            (unsigned long long)key);
            if (prev == EMPTY_KEY) {
              const uint32_t u = atomicAdd(&s_nunk, 1u);
              if (u < SD_UMAX) a.res[SD_RES_UNKNOWN + u] = key;
              break;
            }
            if (prev == key) break;
            j = (j + 1) & (SD_USLOTS - 1);
          }
        }
      }
    }
    if (o.x != SD_LIT) a.D[o.w] = make_uint4((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)src, (uint32_t)(src >> 32));
  }
  __syncthreads();
  SD_STAMP(4);
  const uint64_t stop = s_stop;
  const uint32_t stop_pos = stop == ~0ull ? ~0u : (uint32_t)(stop >> 32);
  const uint32_t T = stop == ~0ull ? s_ndecl : (uint32_t)stop;   // declares before the stop
  if (s_nunk > SD_UMAX) {
    if (t == 0) a.res[SDR_FALLBACK] = SD_FB_BATCH;
    return;
  }
  // ---- what this pass leaves to the batch decoder: an EXTRACT whose bytes
  // differ from the earliest EXTRACT of its hash (name reuse: REFs between them
  // resolve by position there; every EXTRACT op is compared, not only the
  // latest), or EXTRACTs of one hash on both sides of the stop
  const uint32_t nx = s_nx;
  if (s_ndup) {
    for (uint32_t k = w; k < nops; k += 16) {
      const uint4 o = a.ops[k];
      if (readfirst(o.x) != SD_EXT) continue;
      const uint32_t pos = readfirst(o.y) + 2u;
      const uint64_t key = readfirst64(a.opv[k]);
      uint32_t i = mix32((uint32_t)key, (uint32_t)(key >> 32)) & (SD_XSLOTS - 1);
      for (uint32_t n = 0; n < SD_XSLOTS && xk[i] != key; ++n) i = (i + 1) & (SD_XSLOTS - 1);   // (entered above)
      const uint64_t f = xf[i];
      if (f == pos) continue;
      bool bad = f < stop_pos && pos >= stop_pos;
      if (!bad) bad = !dec_equal2048(x + f, x + pos);
      if (bad && l == 0) atomicOr(&s_fb, 1u);
    }
  }
  __syncthreads();
  SD_STAMP(5);
  if (s_fb) {
    if (t == 0) a.res[SDR_FALLBACK] = SD_FB_BATCH;
    return;
  }
  // ---- output: every op before the stop at its offset (a wave per op); the
  // output ends at the stop REF's offset
  if (stop != ~0ull)
    for (uint32_t k = t; k < nops; k += 1024) {
      const uint4 o = a.ops[k];
      if (o.x == SD_REF && o.y == stop_pos) s_olen = o.z;
    }
  __syncthreads();
  SD_STAMP(6);
  const uint64_t out_len = s_olen;
  if (out_len > a.out_cap) {
    if (t == 0) { a.res[SDR_FALLBACK] = SD_FB_ROOM; a.res[SDR_NEED] = out_len; }      // (more room needed; nothing written)
    return;
  }
  for (uint32_t k = w; k < nops; k += 16) {
    const uint4 o = a.ops[k];
    const uint32_t ty = readfirst(o.x), io = readfirst(o.y), oo = readfirst(o.z);
    if (io >= stop_pos) continue;
    if (ty == SD_LIT) {
      (void)wave_unescape(a.out + oo, x, io, io + readfirst(o.w));
    } else {
      const uint4 d = a.D[readfirst(o.w)];
      const uint8_t* src = (const uint8_t*)(((uint64_t)readfirst(d.w) << 32) | readfirst(d.z));
      wave_copy2048(a.out + oo, src);
    }
  }
  if (a.tim) {
    __syncthreads();
    SD_STAMP(7);
  }
  // ---- the BACKREF window after the call's declares (before the commit
  // overwrites any pool bytes a REF's declare reads).  Up to 256 declares: a
  // thread per slot against the call's declared hashes in LDS (uk is free
  // again); only slots this call declares into take a segment; an older slot
  // whose hash the call declares again is emptied (XCodecWindow::declare,
  // xcodec_window.h:68-90).  More declares: window_slot per slot.
  if (T > 0 && T <= 256) {
    for (uint32_t i = t; i < T; i += 1024) {
      const uint4 d = a.D[i];
      uk[i] = ((uint64_t)d.y << 32) | d.x;
    }
    __syncthreads();
    if (t < 256) {
      const uint32_t c = t;
      const uint64_t W = a.win_count, G = W + T;
      const uint64_t r = (G - 1u - c) & 255u;
      if (r <= G - 1u) {                                     // (else never written)
        const uint64_t g = G - 1u - r;
        if (g >= W) {
          const uint32_t tl = (uint32_t)(g - W);
          const uint64_t h = uk[tl];
          bool dup = false;
          for (uint32_t k = tl + 1; k < T; ++k) dup |= uk[k] == h;
          if (dup) {
            a.win_hash[c] = 0;
          } else {
            a.win_hash[c] = h;
            wcopy[atomicAdd(&s_nw, 1u)] = (uint16_t)(c | (tl << 8));   // (tl < 256)
          }
        } else {
          const uint64_t h = a.win_hash[c];
          if (h != 0) {
            bool dup = false;
            for (uint32_t k = 0; k < T; ++k) dup |= uk[k] == h;
            if (dup) a.win_hash[c] = 0;
          }
        }
      }
    }
    __syncthreads();
    for (uint32_t q = w; q < s_nw; q += 16) {
      const uint32_t e = wcopy[q], c = e & 255u, tl = e >> 8;
      const uint4 d = a.D[tl];
      wave_copy2048(a.win_seg + (uint64_t)c * SEG, (const uint8_t*)(((uint64_t)d.w << 32) | d.z));
    }
  } else {
    DecParams prm{};
    prm.D = a.D;
    prm.D_lo = 0;
    prm.D_tail = false;
    prm.win_hash = a.win_hash;
    prm.win_seg = a.win_seg;
    prm.win_count = a.win_count;
    const uint64_t G = a.win_count + T;
    for (uint32_t c = w; c < 256u && T > 0; c += 16) {
      uint64_t h = 0, gd = 0;
      const uint8_t* src = nullptr;
      const bool ok = window_slot(prm, T, c, h, src, gd);
      if (((G - 1u - c) & 255u) > G - 1u) continue;          // never written
      if (!ok) {
        if (l == 0) a.win_hash[c] = 0;
        continue;
      }
      if (gd >= a.win_count) wave_copy2048(a.win_seg + (uint64_t)c * SEG, src);
      if (l == 0) a.win_hash[c] = h;
    }
  }
  __syncthreads();
  SD_STAMP(8);
  // ---- commit: EXTRACTs before the stop enter the cache, or replace a cached
  // segment's bytes (name reuse, :106-136)
  for (uint32_t q = w; q < nx; q += 16) {
    const uint32_t i = xlist[q];
    const uint64_t key = xk[i];
    const uint64_t f = xf[i];
    if (f >= stop_pos) continue;
    const uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
    const uint64_t gv = tab_lookup(a.g, lo, hi);
    const uint8_t* src = x + f;
    if (gv != ~0ull) {
      uint8_t* dst = a.pool + gv * (uint64_t)SEG;
      if (!dec_equal2048(dst, src)) wave_copy2048(dst, src);
      continue;
    }
    uint32_t sg = 0;
    if (l == 0) sg = atomicAdd(a.nseg, 1u);
    sg = readfirst(sg);
    if (sg >= a.seg_cap) {
      if (l == 0) atomicOr(a.status, 4);
      continue;
    }
    wave_copy2048(a.pool + (uint64_t)sg * SEG, src);
    if (l == 0) {
      if (!tab_insert_min(a.g, lo, hi, sg)) atomicOr(a.status, 2);
      filt_insert(a.fs, lo, hi);
    }
  }
  if (a.tim) {
    __syncthreads();
    SD_STAMP(9);
  }
  // ---- results: the EXTRACTs before the stop in op order (the host cache's
  // mirror enters them without hashing again)
  if (w == 0) {
    uint32_t ne = 0;
    for (uint32_t k0 = 0; k0 < nops; k0 += 64) {
      const uint32_t k = k0 + (uint32_t)l;
      bool is = false;
      uint64_t key = 0;
      if (k < nops) {
        const uint4 o = a.ops[k];
        is = o.x == SD_EXT && o.y < stop_pos;
        if (is) key = a.opv[k];
      }
      const uint64_t m = ballot(is);
      const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      if (is && ne + below < SD_EMAX) a.res[SD_RES_EXTRACT + ne + below] = key;
      ne += (uint32_t)__builtin_popcountll(m);
    }
    if (l == 0) {
      const int32_t wst = (int32_t)s_walk_st;
      a.res[SD_RES_STICKY] = (uint64_t)(uint32_t)*a.status;
      a.res[SDR_OUT_LEN] = out_len;
      a.res[SDR_CONSUMED] = stop != ~0ull ? stop_pos : s_walk_end;
      a.res[SDR_STATUS] = (uint64_t)(int64_t)(stop != ~0ull ? 1 : wst);
      a.res[SDR_DECLARES] = T;
      a.res[SDR_UNKNOWNS] = s_nunk;
      a.res[SDR_FALLBACK] = SD_FB_DONE;
      a.res[SDR_EXTRACTS] = ne;
      a.res[SDR_NEED] = out_len;
    }
  }
  SD_STAMP(10);
}

// The call's input, output and results may live in host memory (the
// zero-copy call path: the input is staged into LDS first, the output and
// results cross PCIe as posted writes); the host then waits on `flag`,
// stored after every other write of the block is visible system-wide.
__global__ __launch_bounds__(1024) void decode_small_kernel(SmallDec a) {
  decode_small_body(a);
  if (a.flag) {
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(a.flag, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// N decode() calls on N distinct caches and windows in one launch: workgroup b
// is the whole call calls[b].  The calls share nothing, so the blocks need no
// order among themselves; completion is the stream's (flag and tim are null).
// The record's address depends on blockIdx.x alone, so its loads are scalar and
// the pointers and lengths stay in SGPRs, as decode_small_kernel's kernel
// arguments do.
__global__ __launch_bounds__(1024) void decode_calls_kernel(const SmallDec* __restrict__ calls, uint32_t n) {
  if (blockIdx.x >= n) return;
  const SmallDec a = calls[blockIdx.x];
  decode_small_body(a);
}

}  // namespace xcg

// One SmallDec record (host side): the cache view, the op scratch's three
// arrays and the call's buffers.
static xcg::SmallDec small_dec_of(const uint8_t* in, uint32_t len, const XcgCacheView* g, int32_t* status,
                                  void* scratch, uint32_t ops_cap, uint8_t* out, uint64_t out_cap,
                                  uint64_t* win_hash, uint8_t* win_seg, uint64_t win_count, uint64_t* res) {
  using namespace xcg;
  SmallDec a;
  a.in = in;
  a.len = len;
  a.g = tab_of(*g);
  a.pool = g->pool;
  a.nseg = g->nseg;
  a.seg_cap = g->seg_cap;
  a.fs = filters_of(*g);
  a.status = status;
  a.ops = (uint4*)scratch;
  a.opv = (uint64_t*)(a.ops + ops_cap);
  a.D = (uint4*)(a.opv + ops_cap);
  a.ops_cap = ops_cap;
  a.out = out;
  a.out_cap = out_cap;
  a.win_hash = win_hash;
  a.win_seg = win_seg;
  a.win_count = win_count;
  a.res = res;
  a.tim = nullptr;
  a.flag = nullptr;
  a.seq = 0;
  return a;
}

// The records of decode_calls_kernel, written by the host into the block it
// copies up with the inputs: xcg_small_dec_size() bytes each, 8-byte aligned.
extern "C" uint32_t xcg_small_dec_size(void) { return (uint32_t)sizeof(xcg::SmallDec); }
extern "C" void xcg_small_dec_fill(void* rec, const uint8_t* in, uint32_t len, const XcgCacheView* g, int32_t* status,
                                   void* scratch, uint32_t ops_cap, uint8_t* out, uint64_t out_cap,
                                   uint64_t* win_hash, uint8_t* win_seg, uint64_t win_count, uint64_t* res) {
  *(xcg::SmallDec*)rec = small_dec_of(in, len, g, status, scratch, ops_cap, out, out_cap, win_hash, win_seg, win_count, res);
}

// n decode() calls on n distinct unbounded caches in one launch
// (decode_calls_kernel); d_recs: n records in device memory.
extern "C" int xcg_launch_decode_calls(const void* d_recs, uint32_t n, hipStream_t stream) {
  using namespace xcg;
  if (n == 0) return 0;
  hipLaunchKernelGGL(decode_calls_kernel, dim3(n), dim3(1024), 0, stream, (const SmallDec*)d_recs, n);
  return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}

// One decode() call on an unbounded cache in one launch (decode_small_kernel).
extern "C" int xcg_launch_decode_small(const uint8_t* in, uint32_t len, const XcgCacheView* g, int32_t* status,
                                       void* scratch, uint32_t ops_cap, uint8_t* out, uint64_t out_cap,
                                       uint64_t* win_hash, uint8_t* win_seg, uint64_t win_count, uint64_t* res,
                                       uint64_t* tim, uint32_t* flag, uint32_t seq, hipStream_t stream) {
  using namespace xcg;
  SmallDec a;
  a.in = in;
  a.len = len;
  a.g = tab_of(*g);
  a.pool = g->pool;
  a.nseg = g->nseg;
  a.seg_cap = g->seg_cap;
  a.fs = filters_of(*g);
  a.status = status;
  a.ops = (uint4*)scratch;
  a.opv = (uint64_t*)(a.ops + ops_cap);
  a.D = (uint4*)(a.opv + ops_cap);
  static_assert(SD_SCRATCH_PER_OP == sizeof(uint4) + sizeof(uint64_t) + sizeof(uint4), "ops, opv, D");
  a.ops_cap = ops_cap;
  a.out = out;
  a.out_cap = out_cap;
  a.win_hash = win_hash;
  a.win_seg = win_seg;
  a.win_count = win_count;
  a.res = res;
  a.tim = tim;
  a.flag = flag;
  a.seq = seq;
  hipLaunchKernelGGL(decode_small_kernel, dim3(1), dim3(1024), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}
