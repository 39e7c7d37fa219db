// XCodec batch decoder on a bounded cache (XCodecMemoryCache with a limit,
// xcg_lru.hip) or a pair (XCodecCachePair, xcg_pair.hip): which entries a REF
// or an EXTRACT finds depends on what the batch itself evicted before it.  The
// ops' effects on the cache follow from the stream alone, so the passes here
// list every EXTRACT / REF once, then alternate a classification against the
// eviction times with the cache's own replay of the classified ops, until the
// times agree.  xcg_launch_decode (xcg_decode.hip) runs them between its scan
// and its sizing pass and commits through them at the end.
#include <stdio.h>
#include <stdlib.h>

#include "xcg_decode_batch.h"

namespace xcg {

// Every EXTRACT / REF op of the batch as (lo, hi, op offset, op), packed by
// chunk at op_base[c] (the scan's declare numbering in chunk order).  One wave
// per chunk.
__global__ __launch_bounds__(256) void dec_ops_kernel(DecParams prm, uint4* raw) {
  const int wv = (int)readfirst(threadIdx.x >> 6);
  const uint32_t chunk = blockIdx.x * 4u + (uint32_t)wv;
  if (chunk >= prm.n) return;
  const uint8_t* x = prm.in + prm.chunk_off[chunk];
  const uint32_t len = prm.chunk_len[chunk];
  uint64_t t = prm.op_base[chunk];
  walk_op_headers(
      x, len, chunk,
      [&](uint32_t i) {
        const uint2 h = dec_window_hash(x + i + 2);
        if (lane_id() == 0) raw[t] = make_uint4(readfirst(h.x), readfirst(h.y), i, OP_EXTRACT);
        ++t;
        return false;
      },
      [&](uint32_t, uint32_t r, uint64_t h, uint64_t here) {
        if ((uint32_t)lane_id() < r) raw[t + lane_id()] = make_uint4((uint32_t)h, (uint32_t)(h >> 32), (uint32_t)here, OP_REF);
        t += r;
        return false;
      },
      [](uint32_t) { return false; });
}

// What each op does to the bounded cache, given the eviction times (ptime)
// and the stop point of the last pass (blockp): an EXTRACT looks its hash up
// (xcodec_decoder.cc:106-136): an earlier EXTRACT of the batch (HIT), a live
// persistent entry (GHIT: use, replace if the bytes differ) or an ENTER; a
// REF (:141-163) hits likewise or is unknown -- the stream stops at the first
// one.  After the stop point decode_skim (:196-272) still looks up every REF
// (a hit refreshes the entry) against the cache as it stands there.
// ev[op_base[c] + k]: (lo, hi, op offset, kind << 30 | ref) with GMISS =
// no cache effect; ENTERs also as declaration rows.  One wave per chunk.
//
// PAIR (XCodecCachePair, xcg_pair.hip): ptime is the time a hash leaves both
// levels.  A skim lookup can promote a disk-only hash and so evict another
// (xcodec_cache.h:223-227), so each skim lookup sees the pair at its own time,
// not at the stop.  An EXTRACT whose cached bytes differ is a REPLACE (op
// offset | 1 << 31, GHIT): it takes a declaration row like an ENTER (the new
// bytes' source), numbered with the ENTERs in op order.
//
// The cap (*prm.berr_pos: the first BACKREF to an empty slot, found before the
// passes; a BACKREF makes no lookup, so no pass moves it): decode() returns
// false there (:172-176) and looks at nothing behind it -- no skim -- so while
// no unknown REF stands in front of it, every op behind it is GMISS and an
// unknown REF there is not one.  With the unknown-REF stop in front, the skim
// runs on over the BACKREFs (:261-266) and the cap means nothing.
//
// `noskim` (several windows, xcg_decode_batch_windows_bounded): the call ends
// at its stop point whichever kind it is and leaves the skim to the caller's
// next call, so every op behind min(blockp, cap) is GMISS.
template <bool PAIR>
__global__ __launch_bounds__(256) void dec_classify_kernel(DecParams prm, const uint4* raw, uint4* ev, uint32_t* nev,
                                                           uint4* drow, uint32_t* ndecl, uint32_t maxd,
                                                           uint64_t blockp, uint64_t* block_new, uint32_t* changes,
                                                           int first, int noskim) {
  const uint32_t c = blockIdx.x * 4u + (uint32_t)readfirst(threadIdx.x >> 6);
  if (c >= prm.n) return;
  const uint32_t cnt = (uint32_t)prm.n_decl[c];
  const uint64_t base = prm.op_base[c];
  const uint64_t tb = blockp == ~0ull ? ~0ull : ((blockp >> 32 << 21) | (uint32_t)blockp);
  const uint64_t cap = readfirst64(*prm.berr_pos);
  const bool capped = cap < blockp;                   // the error stop comes first
  const uint64_t lim = noskim ? min(cap, blockp) : capped ? cap : ~0ull;   // ops behind it: no cache effect
  const uint8_t* x = prm.in + prm.chunk_off[c];
  uint32_t nd = 0;
  bool chg = false;
  for (uint32_t k0 = 0; k0 < cnt; k0 += 64) {
    const uint32_t k = k0 + (uint32_t)lane_id();
    const bool valid = k < cnt;
    uint4 r = valid ? raw[base + k] : make_uint4(0u, 0u, 0u, 0u);
    const uint64_t here = spos(c, r.z), t = ((uint64_t)c << 21) | r.z;
    uint32_t kind = EV_GMISS, ref = 0, zflag = 0;
    bool enter = false;
    if (valid && here <= lim) {
      const uint64_t e = tab_lookup_t(prm.x, r.x, r.y);
      if (here <= blockp) {                           // (the op at the stop point is looked at again)
        if (e != ~0ull && e < here) {
          kind = EV_HIT;
        } else {
          const uint64_t gv = tab_lookup_t(prm.g, r.x, r.y);
          if (gv != ~0ull && t < prm.ptime[gv]) {
            kind = EV_GHIT;
            ref = (uint32_t)gv;
            if (PAIR && r.w == OP_EXTRACT) {          // name reuse: the cached bytes differ
              const u32x4_u* a = (const u32x4_u*)(x + r.z + 2);
              const u32x4_u* b = (const u32x4_u*)(prm.pool + gv * (uint64_t)SEG);
              bool same = true;
              for (uint32_t q = 0; q < SEG / 16 && same; ++q) {
                const u32x4 va = a[q], vb = b[q];
                same = va[0] == vb[0] && va[1] == vb[1] && va[2] == vb[2] && va[3] == vb[3];
              }
              if (!same) {
                zflag = 1u << 31;
                enter = true;                         // (a declaration row; the kind stays GHIT)
              }
            }
          } else if (r.w == OP_EXTRACT) {
            enter = true;
          } else {
            atomicMin((unsigned long long*)block_new, (unsigned long long)here);   // unknown REF
          }
        }
      } else if (r.w == OP_REF) {                     // decode_skim's lookup
        if (e != ~0ull && e < blockp) {
          kind = EV_HIT;
        } else {
          const uint64_t gv = tab_lookup_t(prm.g, r.x, r.y);
          if (gv != ~0ull && (PAIR ? t : tb) < prm.ptime[gv]) {
            kind = EV_GHIT;
            ref = (uint32_t)gv;
          }
        }
      }
    }
    const uint64_t m = ballot(enter);
    if (enter) {
      const uint32_t d = nd + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      if (!zflag) {
        kind = EV_ENTER;
        ref = d;
      }
      if (d < maxd) drow[(uint64_t)c * maxd + d] = make_uint4(r.x, r.y, r.z + 2u, 0u);
    }
    nd += (uint32_t)__builtin_popcountll(m);
    if (valid) {
      const uint32_t w = (kind << 30) | ref;
      const uint4 old = ev[base + k];
      chg |= first || old.w != w || old.z != (r.z | zflag);
      ev[base + k] = make_uint4(r.x, r.y, r.z | zflag, w);
    }
  }
  if (ballot(chg) != 0 && lane_id() == 0) atomicAdd(changes, 1u);
  if (lane_id() == 0) {
    nev[c] = cnt;
    ndecl[c] = nd;
    if (nd > maxd) atomicOr(prm.status, 1 << 11);
  }
}

// EXTRACTs that looked up a live entry: replace its bytes if they differ
// (XCodecMemoryCache::replace, :130); a second EXTRACT of a hash in the batch
// with other bytes is the name reuse the batch decoder does not model (bit 9).
__global__ __launch_bounds__(256) void dec_replace_kernel(DecParams prm, const uint4* raw, const uint4* ev,
                                                          uint8_t* pool) {
  const uint32_t c = blockIdx.x * 4u + (uint32_t)readfirst(threadIdx.x >> 6);
  if (c >= prm.n) return;
  const uint32_t cnt = (uint32_t)prm.n_decl[c];
  const uint64_t base = prm.op_base[c];
  const uint8_t* x = prm.in + prm.chunk_off[c];
  for (uint32_t k = 0; k < cnt; ++k) {
    const uint4 e = ev[base + k];
    const uint32_t kind = readfirst(e.w) >> 30;
    if (readfirst(raw[base + k].w) != OP_EXTRACT || (kind != EV_GHIT && kind != EV_HIT)) continue;
    const uint8_t* src = x + readfirst(e.z) + 2;
    if (kind == EV_GHIT) {
      uint8_t* dst = pool + (uint64_t)(readfirst(e.w) & EV_REF_MASK) * SEG;
      if (!dec_equal2048(dst, src)) wave_copy2048(dst, src);
    } else {
      const uint64_t first = tab_lookup(prm.x, readfirst(e.x), readfirst(e.y));
      const uint8_t* s0 = prm.in + prm.chunk_off[first >> 32] + (uint32_t)first;
      if (!dec_equal2048(s0, src) && lane_id() == 0) atomicOr(prm.status, 1 << 9);
    }
  }
}

// Bounded and pair contexts, before anything is emitted or committed: a hash
// with EXTRACTs on both sides of the stop point is not modelled there (status
// bit 9: XCG_ENOTSUP with the cache, window and outputs untouched; EXTRACTs
// that differ in bytes were refused by dec_dup_kernel).  One thread per
// batch-table slot.
__global__ __launch_bounds__(256) void dec_precheck_kernel(DecParams prm) {
  const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (w > prm.x.mask) return;
  const uint64_t key = prm.x.keys[w];
  if (key == EMPTY_KEY) return;
  const uint64_t first = prm.x.vals[w], last = prm.x_latest[w];
  const uint64_t blockp = min(*prm.block_pos, *prm.berr_pos);
  if (first < blockp && last != first && last >= blockp) atomicOr(prm.status, 1 << 9);
}

namespace {
// What the pair's passes touch of a decode batch: its input, the
// classification's declaration rows and the cache.
PairGpu pair_gpu(const XcgDecodeArgs* a, const void* rows) {
  PairGpu G{};
  G.in = a->in; G.chunk_off = a->chunk_off;
  G.decl = rows; G.maxd = a->maxd;
  G.g = a->g;
  G.status = a->status;
  return G;
}

// Consecutive arrays out of one block.
struct Carver {
  uint8_t* at;
  template <class T>
  T* take(uint64_t count, uintptr_t align = 1) {
    at = (uint8_t*)(((uintptr_t)at + align - 1) & ~(align - 1));
    T* r = (T*)at;
    at += count * sizeof(T);
    return r;
  }
};

// Classify until the times agree.  PAIR picks the classify instantiation and
// its `first` argument (the pair compares the replay's times itself, so every
// pass is a first one); step(pass, blockp, &same) replays the classified ops
// and brings cw back into h_scratch->cls: `same` = the times it computed are
// the ones the classification used.  Agreed: same, and the stop point stands.
template <bool PAIR, class Step>
int classify_passes(const XcgDecodeArgs* a, const DecParams& p, const DecClassified& K, DecClassifyWords* cw, Step step,
                    hipStream_t stream) {
  const dim3 grid((a->n + 3) / 4), block(256);
  uint64_t blockp = ~0ull;
  bool agreed = false;
  for (int pass = 0; pass < 64 && !agreed; ++pass) {
    if (hipMemsetAsync(&cw->block, 0xFF, 8, stream) != hipSuccess ||
        hipMemsetAsync(&cw->changes, 0, 4, stream) != hipSuccess)
      return XCG_RC_HIP;
    hipLaunchKernelGGL(dec_classify_kernel<PAIR>, grid, block, 0, stream, p, (const uint4*)K.raw, K.evs, K.nev, K.rows,
                       K.nrows, a->maxd, blockp, &cw->block, &cw->changes, PAIR || pass == 0 ? 1 : 0,
                       a->wins != nullptr ? 1 : 0);
    bool same = false;
    const int rc = step(pass, blockp, &same);
    if (rc) return rc;
    const uint64_t nb = a->h_scratch->cls.block;
    agreed = same && nb == blockp;
    blockp = nb;
  }
  return agreed ? 0 : XCG_RC_OVERFLOW;
}
}  // namespace

int dec_classify(const XcgDecodeArgs* a, DecParams& p, uint64_t ndecl, StreamTemp& tmp, DecClassified* K,
                 hipStream_t stream) {
  const uint32_t n = a->n;
  XcgLruState* L = a->lru;
  const bool pair = a->pair != nullptr;
  if (pair && xcg_pair_decode_begin(a->pair, stream)) return XCG_RC_HIP;
  const uint64_t m = ndecl ? ndecl : 1;
  // raw ops, classified ops, declaration rows | (bounded) evtime | evslot |
  // per-chunk counts, (bounded) bases, flags | the pass's words
  const uint64_t bytes = pair ? 32 * m + 16ull * n * a->maxd + 8ull * (n + 1) + 64
                              : 32 * m + 16ull * n * a->maxd + 8 * m + 4 * m + 20ull * (n + 1) + 64;
  uint8_t* mem = nullptr;
  if (!tmp.alloc(&mem, bytes)) return XCG_RC_HIP;
  Carver c{mem};
  K->raw = c.take<uint4>(m);
  K->evs = c.take<uint4>(m);
  K->rows = c.take<uint4>((uint64_t)n * a->maxd);
  LruBatch& lb = K->lb;
  if (!pair) {
    lb.evtime = c.take<uint64_t>(m);
    lb.evslot = c.take<uint32_t>(m);
  }
  K->nev = c.take<uint32_t>(n + 1);
  K->nrows = c.take<uint32_t>(n + 1);
  if (!pair) {
    lb.need = c.take<uint32_t>(n + 1);
    lb.ev_base = c.take<uint32_t>(n + 1);
    lb.enter_base = c.take<uint32_t>(n + 1);
    lb.n = n; lb.in = a->in; lb.chunk_off = a->chunk_off;
    lb.decl = K->rows; lb.ndecl = K->nrows; lb.maxd = a->maxd;
    lb.ev = K->evs; lb.nev = K->nev; lb.maxe = 0xFFFFFFFFu; lb.dense = 1;
    lb.g = a->g;
    lb.status = a->status;
    lb.ev_bound = m;
  }
  DecClassifyWords* cw = c.take<DecClassifyWords>(1, 16);
  hipLaunchKernelGGL(dec_ops_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, p, K->raw);
  DecHostWords* h = a->h_scratch;
  if (pair) {
    p.ptime = xcg_pair_state_ptime(a->pair);
    // the pair replays the classified ops through its policy (xcg_pair.hip)
    return classify_passes<true>(a, p, *K, cw, [&](int pass, uint64_t blockp, bool* agree) {
      if (hipMemcpyAsync(&h->cls, cw, 8, hipMemcpyDeviceToHost, stream) != hipSuccess) return (int)XCG_RC_HIP;
      int same = 0;
      const PairGpu G = pair_gpu(a, K->rows);
      const int prc = xcg_pair_decode_pass(a->pair, &G, K->evs, p.op_base, p.n_decl, n, ndecl, a->maxd, &same, stream);
      if (prc) return prc;
      if (getenv("XCG_PAIR_DEBUG"))
        fprintf(stderr, "pair-dec: n %u pass %d same %d block %llx -> %llx\n", n, pass, same,
                (unsigned long long)blockp, (unsigned long long)h->cls.block);
      *agree = same != 0;
      return 0;
    }, stream);
  }
  if (xcg_lru_reset_times(L, stream)) return XCG_RC_HIP;
  p.ptime = L->ptime;
  return classify_passes<false>(a, p, *K, cw, [&](int pass, uint64_t blockp, bool* agree) {
    if (xcg_lru_times(&lb, L, stream)) return (int)XCG_RC_HIP;   // (synchronises)
    if (hipMemcpyAsync(&h->cls, cw, sizeof(*cw), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
      return (int)XCG_RC_HIP;
    const uint32_t nchg = h->cls.changes;
    if ((uint64_t)L->h_tot[1] + L->h_tot[8] > L->C) return (int)XCG_RC_NOTSUP;   // enters + persistent lookups > limit
    if (getenv("XCG_LRU_DEBUG"))
      fprintf(stderr, "lru-dec: n %u pass %d enters %u evict %u live %u hits %u changes %u block %llx -> %llx\n", n,
              pass, L->h_tot[1], L->h_tot[2], L->h_tot[3], L->h_tot[8], nchg, (unsigned long long)blockp,
              (unsigned long long)h->cls.block);
    *agree = nchg == 0;
    return 0;
  }, stream);
}

void dec_launch_precheck(const DecParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(dec_precheck_kernel, dim3((unsigned)(((uint64_t)p.x.mask + 256) / 256)), dim3(256), 0, stream, p);
}

int dec_classified_commit(const XcgDecodeArgs* a, const DecParams& p, const DecClassified& K, hipStream_t stream) {
  if (a->pair) {
    // the classification's declaration rows give each new entry's bytes
    const PairGpu G = pair_gpu(a, K.rows);
    const int crc = xcg_pair_decode_commit(a->pair, &G, stream);
    if (crc) return crc;
  } else {
    hipLaunchKernelGGL(dec_replace_kernel, dim3((a->n + 3) / 4), dim3(256), 0, stream, p, (const uint4*)K.raw,
                       (const uint4*)K.evs, a->g.pool);
    const int crc = xcg_lru_commit(&K.lb, a->lru, stream);
    if (crc) return crc;
  }
  return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}

}  // namespace xcg
