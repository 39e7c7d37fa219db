// XCodec decoder, MI355X (gfx950) HIP kernels.
//
// Restates XCodecDecoder::decode (xcodec/xcodec_decoder.cc:66-188) for a batch
// of encoded chunks that form ONE stream (successive decode() calls on one
// decoder and cache, e.g. tack -d, programs/tack/tack.cc:329-359, or the
// frames of one XCodecPipePair, xcodec/xcodec_pipe_pair.cc:425-483).
//
//   scan   (one wave per chunk): walk the op stream.  Literal runs are found
//          1 KiB at a time with a wave ballot over the bytes: an 0xF1 followed
//          by 0x00 is an ESCAPE inside the run, any other 0xF1 starts an op.
//          EXTRACT payloads are hashed (XCodecHash::hash, :106) and entered in
//          the batch table X: hash -> earliest / latest stream position.
//   size   exclusive scan of the decoded lengths -> output offsets.
//   emit   (one wave per chunk): walk again and write: literal runs with
//          F1 00 -> F1, EXTRACT payloads, REF segments gathered from the
//          earliest earlier EXTRACT in the batch or from the persistent cache
//          (the cache state at that point of the stream, :151-162).  A REF
//          that neither resolves blocks the stream there (:151-156).
//   commit EXTRACTs before the blocking point enter the cache
//          (XCodecMemoryCache::enter / replace, :120-136).
//
// Name reuse (:106-136, a later EXTRACT of a hash with other bytes replaces the
// entry, and every later REF reads the new bytes): the scan lists every EXTRACT
// after a hash's first (`dup`); when there are any, dec_dup_kernel compares
// each with the hash's first-inserted EXTRACT and flags the hashes whose
// EXTRACTs differ.  With none flagged every EXTRACT of a hash holds the same
// bytes and the earliest serves.  Otherwise (unbounded contexts; bounded and
// pair contexts refuse) the flagged hashes' occurrences are gathered, sorted by
// (hash, position), and the REUSE instantiations of emit, decl_record and
// commit resolve a flagged hash by binary search: the latest EXTRACT before
// the REF (before the stop point, for the commit).
//
// BACKREF (:165-181) reads the decoder's XCodecWindow (xcodec/xcodec_window.h):
// every EXTRACT and resolved REF declares its hash into slot k mod 256 (k =
// declares made by this decoder so far), emptying the slot that held the same
// hash before (:68-100).  Slot c at declare count G therefore holds the latest
// declare g < G with g = c (mod 256) unless that hash was declared again in
// (g, G).  The scan counts declares per chunk; an exclusive scan numbers them;
// `decl_record` writes (hash, bytes) records of the declares a BACKREF or the
// window update can reach; an invalid BACKREF stops the stream like an unknown
// REF (decode() returns false there, :172-176); `window_update` carries the
// 256 slots (hash + an owned copy of the bytes) into the next batch.
//
// The neighbouring units:
//   xcg_decode_batch.h      DecParams, the device helpers shared with the two
//                           units below, and the host entry points between them
//   xcg_decode_words.h      the scratch words of a batch and the result words
//                           of a call, by name (no HIP: also the ABI layer's)
//   xcg_decode_bounded.hip  bounded-cache and pair contexts: the op list, the
//                           classification against the eviction times, the
//                           precheck and the commit through xcg_lru / xcg_pair
//   xcg_decode_small.hip    one decode() call in one workgroup
//   xcg_decode_ops.h        the wave-level op walk pieces, shared with
//                           xcg_decode_indep.hip and xcg_decode_group.hip
// Here: the stream-batch kernels, the name-reuse kernels, the kernel timer and
// xcg_launch_decode, which runs the passes in order.
#include <stdio.h>
#include <stdlib.h>

#include <mutex>
#include <utility>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "xcg_decode_batch.h"

namespace xcg {

// ------------------------------------------------------------------ kernels

// WINS: one window per decoder (xcg_decode_windows.hip) -- a BACKREF reads the
// window its chunk names; everything else is the one-window kernel.
template <bool EMIT, bool REUSE = false, bool WINS = false>
__global__ __launch_bounds__(256) void decode_kernel(DecParams prm) {
  const int wv = (int)readfirst(threadIdx.x >> 6);
  const uint32_t chunk = blockIdx.x * 4u + (uint32_t)wv;
  if (chunk >= prm.n) return;
  const int l = lane_id();
  const uint8_t* x = prm.in + prm.chunk_off[chunk];
  const uint32_t len = prm.chunk_len[chunk];
  uint8_t* out = EMIT ? prm.out + prm.out_off[chunk] : nullptr;
  uint64_t olen = 0;
  int32_t st = 0;
  uint32_t i = 0;
  uint64_t ndecl = 0, nbref = 0;
  const uint64_t blockp = EMIT ? min(readfirst64(*prm.block_pos), readfirst64(*prm.berr_pos)) : ~0ull;
  if (EMIT && spos(chunk, 0) > blockp) {      // after the stop point: decode() never got here
    if (l == 0) {
      prm.out_len[chunk] = 0;
      prm.chunk_status[chunk] = 2;
      prm.consumed[chunk] = 0;
      prm.n_decl_emit[chunk] = 0;
    }
    return;
  }
  const uint64_t dbase = EMIT ? prm.decl_base[chunk] : 0;

  while (i < len) {
    uint32_t nesc = 0;
    const uint32_t m = next_op(x, i, len, nesc);
    // literal run [i, m) with nesc escape pairs (:71-81 and OP_ESCAPE :91-94)
    if (m > i) {
      if (EMIT) olen += readfirst(wave_unescape(out + olen, x, i, m));
      else olen += (m - i) - nesc;
    }
    i = m;
    if (i >= len) break;
    if (len - i == 1) { st = 3; break; }                     // :87-88 need the op byte
    const uint32_t op = x[i + 1];
    if (op == OP_EXTRACT) {                                  // :96-140
      if (len - i < 2u + SEG) { st = 3; break; }
      const uint8_t* seg = x + i + 2;
      if (EMIT) {
        wave_copy2048(out + olen, seg);
        const uint64_t t = dbase + ndecl;
        if (prm.tail_D && t >= prm.tail_lo && t < prm.tail_hi) {   // (the window's tail: its hash here)
          const uint2 h = dec_window_hash(seg);
          const uint64_t src = (uint64_t)seg;
          if (l == 0) prm.tail_D[t - prm.tail_lo] = make_uint4(readfirst(h.x), readfirst(h.y), (uint32_t)src,
                                                               (uint32_t)(src >> 32));
        }
      } else {
        const uint2 h = dec_window_hash(seg);
        if (l == 0) {
          bool existed = false;
          uint32_t slot = 0;
          const uint64_t pos = spos(chunk, i + 2);
          if (!xtab_insert(prm.x, prm.x_latest, prm.x_owner, readfirst(h.x), readfirst(h.y), pos, existed, slot)) {
            atomicOr(prm.status, 1 << 10);
          } else if (existed) {                              // a later EXTRACT of the hash: listed for dec_dup_kernel
            const uint64_t k = atomicAdd((unsigned long long*)prm.dup_ctr, 1ull) + 1ull;
            if (k < prm.dup_cap) {
              prm.dup_slot[k] = slot;
              prm.dup_pos[k] = pos;
            }
          }
        }
      }
      olen += SEG;
      i += 2 + SEG;
      ++ndecl;                                               // window_.declare, :137
    } else if (op == OP_REF) {                               // :141-163
      if (len - i < 10u) { st = 3; break; }
      if (EMIT && spos(chunk, i) >= blockp) { st = 1; break; }   // blocked at or before this op
      // Resolvability (an earlier EXTRACT of h in the batch, or the cache)
      // is checked after the scan (decode_refcheck_kernel), once the batch
      // table is complete; emit resolves a whole run of REFs at a time.
      uint64_t h, here;
      uint32_t r = ref_run(x, i, len, chunk, blockp, h, here);
      bool stop = false;
      if (EMIT) {
        const uint8_t* src = nullptr;
        if ((uint32_t)l < r) src = ref_source_t<REUSE>(prm, (uint32_t)h, (uint32_t)(h >> 32), here);
        const uint64_t miss = ballot((uint32_t)l < r && src == nullptr);
        if (miss) {                                          // cannot happen: refcheck found all
          r = (uint32_t)__builtin_ctzll(miss);
          stop = true;
        }
        copy_segments(out + olen, src, r);
        const uint64_t tl = dbase + ndecl + (uint64_t)l;
        if (prm.tail_D && (uint32_t)l < r && tl >= prm.tail_lo && tl < prm.tail_hi)
          prm.tail_D[tl - prm.tail_lo] = make_uint4((uint32_t)h, (uint32_t)(h >> 32), (uint32_t)(uint64_t)src,
                                                    (uint32_t)((uint64_t)src >> 32));
      }
      olen += (uint64_t)SEG * r;
      i += 10u * r;
      ndecl += r;                                            // window_.declare, :160
      if (stop) { st = 1; break; }
    } else if (op == OP_BACKREF) {                           // :165-181
      if (len - i < 3u) { st = 3; break; }
      if (EMIT) {
        if (spos(chunk, i) >= blockp) { st = -1; i += 3; break; }   // empty slot: moveout precedes the check
        uint64_t h = 0, gd = 0;
        const uint8_t* src = nullptr;
        if (WINS) {
          if (!window_slot_of(ManyWindow(prm, readfirst(prm.chunk_win[chunk])), dbase + ndecl, x[i + 2], h, src, gd)) {
            st = -1; i += 3; break;
          }
        } else
        if (!window_slot(prm, dbase + ndecl, x[i + 2], h, src, gd)) { st = -1; i += 3; break; }
        wave_copy2048(out + olen, src);
      }
      ++nbref;
      olen += SEG;
      i += 3;
    } else {
      st = -1;                                               // :183-184 unsupported opcode
      break;
    }
  }
  if (l == 0) {
    prm.out_len[chunk] = olen;
    if (EMIT) {
      prm.chunk_status[chunk] = st;
      prm.consumed[chunk] = i;
      prm.n_decl_emit[chunk] = ndecl;
    } else {
      prm.n_decl[chunk] = ndecl;
      prm.n_bref[chunk] = nbref;
    }
  }
}

// Declare records for batch indices [lo_t, hi_t): full (every declare, when
// the batch holds BACKREFs) or tail (the 256 before the stop point, for the
// window update).  One wave per chunk.
template <bool REUSE>
__global__ __launch_bounds__(256) void decl_record_kernel(DecParams prm, uint64_t total) {
  const int wv = (int)readfirst(threadIdx.x >> 6);
  const uint32_t chunk = blockIdx.x * 4u + (uint32_t)wv;
  if (chunk >= prm.n) return;
  const uint64_t hi_t = prm.D_tail ? readfirst64(*prm.t_end) : total, lo_t = d_lo_of(prm);
  const uint64_t base = prm.decl_base[chunk], cnt = prm.n_decl[chunk];
  if (base >= hi_t || base + cnt <= lo_t) return;
  decl_record_chunk<REUSE>(prm, chunk, base, lo_t, hi_t, 0 - lo_t);
}

// Invalid BACKREFs (empty window slot): the first one stops the stream.
template <bool WINS>
__global__ __launch_bounds__(256) void decode_brefcheck_kernel(DecParams prm) {
  const int wv = (int)readfirst(threadIdx.x >> 6);
  const uint32_t chunk = blockIdx.x * 4u + (uint32_t)wv;
  if (chunk >= prm.n || prm.n_bref[chunk] == 0) return;
  const uint8_t* x = prm.in + prm.chunk_off[chunk];
  const uint32_t len = prm.chunk_len[chunk];
  uint64_t t = prm.decl_base[chunk];
  uint32_t i = 0;
  while (i < len) {                                          // (walk_op_headers' walk, one REF at a time: its runs cost
    uint32_t nesc = 0;                                       // this kernel 32 instructions more and buy it nothing)
    i = next_op(x, i, len, nesc);
    if (i + 1 >= len) break;
    const uint32_t op = x[i + 1];
    if (op == OP_EXTRACT) {
      if (len - i < 2u + SEG) break;
      ++t;
      i += 2 + SEG;
    } else if (op == OP_REF) {
      if (len - i < 10u) break;
      ++t;
      i += 10;
    } else if (op == OP_BACKREF) {
      if (len - i < 3u) break;
      uint64_t h = 0, gd = 0;
      const uint8_t* src = nullptr;
      const bool live = WINS ? window_slot_of(ManyWindow(prm, readfirst(prm.chunk_win[chunk])), t, x[i + 2], h, src, gd)
                             : window_slot(prm, t, x[i + 2], h, src, gd);
      if (!live) {
        if (lane_id() == 0) atomicMin((unsigned long long*)prm.berr_pos, (unsigned long long)spos(chunk, i));
        break;
      }
      i += 3;
    } else {
      break;
    }
  }
}

// Declares before the stop point (the first unknown REF or invalid BACKREF).
__global__ void decode_tend_kernel(DecParams prm, uint64_t total) {
  const uint64_t stop = min(*prm.block_pos, *prm.berr_pos);
  *prm.t_end = stop == ~0ull ? total : prm.decl_base[stop >> 32] + prm.n_decl_emit[stop >> 32];
}

// The window after the batch: slot c as window_slot() sees it at t_end, with
// the bytes copied in (the window holds its own reference to them).  One wave
// per slot; every source is batch input or pool, never another slot.
__global__ __launch_bounds__(256) void window_update_kernel(DecParams prm) {
  const uint32_t c = blockIdx.x * 4u + (uint32_t)readfirst(threadIdx.x >> 6);
  if (c >= 256u) return;
  const uint64_t T = readfirst64(*prm.t_end);
  if (T == 0) return;
  uint64_t h = 0, gd = 0;
  const uint8_t* src = nullptr;
  const bool ok = window_slot(prm, T, c, h, src, gd);
  const uint64_t G = prm.win_count + T;
  const bool written = ((G - 1u - c) & 255u) <= G - 1u;
  if (!written) return;
  if (!ok) {
    if (lane_id() == 0) prm.win_hash[c] = 0;
    return;
  }
  if (gd >= prm.win_count) wave_copy2048(prm.win_seg + (uint64_t)c * SEG, src);
  if (lane_id() == 0) prm.win_hash[c] = h;
}

// Between scan and emit: find unresolvable REFs (no earlier EXTRACT of the
// hash in the batch, not in the cache) and the first such stream position.
// One wave per chunk; walks only the op headers.
__global__ __launch_bounds__(256) void decode_refcheck_kernel(DecParams prm) {
  const int wv = (int)readfirst(threadIdx.x >> 6);
  const uint32_t chunk = blockIdx.x * 4u + (uint32_t)wv;
  if (chunk >= prm.n) return;
  const uint8_t* x = prm.in + prm.chunk_off[chunk];
  const uint32_t len = prm.chunk_len[chunk];
  walk_op_headers(
      x, len, chunk, [](uint32_t) { return false; },
      [&](uint32_t, uint32_t r, uint64_t h, uint64_t here) {
        if ((uint32_t)lane_id() < r) {
          const uint32_t lo = (uint32_t)h, hi = (uint32_t)(h >> 32);
          const uint64_t e = tab_lookup_t(prm.x, lo, hi);
          bool ok = e != ~0ull && e < here;
          if (!ok) ok = g_live(prm, tab_lookup_t(prm.g, lo, hi), here);
          if (!ok) {
            atomicMin((unsigned long long*)prm.block_pos, (unsigned long long)here);
            // decode_skim's set (xcodec_decoder.cc:196-272): each unknown hash once
            // (u: open-addressed set of 2 * unknown_cap slots); past the cap the
            // count keeps growing and xcg_decode_batch reports XCG_EOVERFLOW.
            if (uset_insert(prm.u_keys, prm.u_mask, h)) {
              const uint32_t k = atomicAdd(prm.nunknown, 1u);
              if (k < prm.unknown_cap) {
                prm.unknown[k] = h;
                prm.unknown_pos[k] = here;
              }
            }
          }
        }
        return false;
      },
      [](uint32_t) { return false; });
}

// Exclusive scan of n u64 lengths (single workgroup).  Tiles of 4096: each
// thread loads four consecutive lengths (coalesced), scans them, the block
// scans the 1024 partial sums in LDS, and a running carry joins the tiles --
// a handful of load round trips instead of one per element per thread.
__global__ __launch_bounds__(1024) void exclusive_scan_kernel(const uint64_t* len, uint64_t* off, uint32_t n,
                                                             uint64_t* total) {
  __shared__ uint64_t part[1024];
  const uint32_t t = threadIdx.x;
  uint64_t carry = 0;
  for (uint32_t base = 0; base < n; base += 4096) {
    const uint32_t i0 = base + 4 * t;
    uint64_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? len[i0 + k] : 0u;
    const uint64_t s = v[0] + v[1] + v[2] + v[3];
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
      const uint64_t u = t >= d ? part[t - d] : 0u;
      __syncthreads();
      part[t] += u;
      __syncthreads();
    }
    uint64_t run = carry + part[t] - s;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (i0 + k < n) off[i0 + k] = run;
      run += v[k];
    }
    carry += part[1023];
    __syncthreads();
  }
  if (t == 0) *total = carry;
}

// The EXTRACT whose bytes the commit takes for the hash in `slot` (first <
// blockp): the latest one before the stop point.  Without REUSE every EXTRACT
// of a hash holds the same bytes, so the earliest stands in for a later one
// the stream did not reach.  Wave-uniform arguments give a uniform result.
template <bool REUSE>
__device__ __forceinline__ uint64_t commit_pos(const DecParams& prm, uint32_t slot, uint64_t first, uint64_t last,
                                               uint64_t blockp) {
  if (REUSE && prm.x_flag[slot]) {
    const uint64_t p = occ_before(prm, prm.x.keys[slot], blockp);
    return p != ~0ull ? p : first;                           // (first < blockp is listed, so p is found)
  }
  return last < blockp ? last : first;
}

// Commit: every batch EXTRACT hash with an EXTRACT before the blocking point
// enters the cache with the bytes of the latest such EXTRACT (enter, or
// replace when the cached bytes differ: name reuse, :120-136).
// A block takes 256 batch-table slots: one thread per slot decides (enter /
// replace / skip), new segments are numbered by a block count (one global
// atomic per block), then the block's waves copy the segments.
template <bool REUSE>
__global__ __launch_bounds__(256) void decode_commit_kernel(DecParams prm, uint8_t* pool, uint32_t* nseg,
                                                            uint32_t seg_cap, FiltSet fs) {
  __shared__ uint32_t s_cnt, s_base, s_njob, s_rest;
  __shared__ uint4 s_job[256];   // (slot, destination segment, kind, -)
  const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint64_t blockp = min(*prm.block_pos, *prm.berr_pos);
  int kind = 0;                  // 0 none, 1 enter, 2 replace
  uint64_t gv = ~0ull;
  uint64_t key = EMPTY_KEY;
  if (w <= prm.x.mask) {
    key = prm.x.keys[w];
    if (key != EMPTY_KEY) {
      const uint64_t first = prm.x.vals[w];
      if (first < blockp) {                      // else never reached
        gv = tab_lookup_t(prm.g, (uint32_t)key, (uint32_t)(key >> 32));
        kind = gv != ~0ull ? 2 : 1;
      }
    }
  }
  const uint32_t seg = block_alloc_segs(kind == 1, nseg, &s_cnt, &s_base);
  if (threadIdx.x == 0) { s_njob = 0; s_rest = 0; }
  __syncthreads();
  if (kind == 1 && seg >= seg_cap) {
    atomicOr(prm.status, 4);
    kind = 0;
  }
  if (kind == 1) {
    const uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
    if (!tab_insert_min(prm.g, lo, hi, seg)) atomicOr(prm.status, 2);
    filt_insert(fs, lo, hi);
  }
  if (kind) {
    const uint32_t j = atomicAdd(&s_njob, 1u);
    s_job[j] = make_uint4((uint32_t)w, kind == 1 ? seg : (uint32_t)gv, (uint32_t)kind, 0u);
  }
  __syncthreads();
  const uint32_t njob = s_njob;
  const uint32_t wv = readfirst(threadIdx.x >> 6);
  const int l = lane_id();
  // Plain enters (one EXTRACT of the hash, not cached): four of the wave's
  // segments loaded together, then stored (one round trip per four copies
  // instead of one per copy); everything else one job at a time below.
  bool rest = false;
  for (uint32_t j0 = 4u * wv; j0 < njob; j0 += 16u) {
    u32x4 v[4][2];
    uint8_t* dst[4];
    bool plain[4];
    uint64_t first[4], last[4], coff[4];
    uint4 jb[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {                  // (the four jobs' table reads in flight together)
      const uint32_t j = min(j0 + (uint32_t)t, njob - 1u);
      jb[t] = s_job[j];
      const uint32_t slot = readfirst(jb[t].x);
      first[t] = prm.x.vals[slot];
      last[t] = prm.x_latest[slot];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)                    // (last: from here on the EXTRACT the commit takes)
      last[t] = commit_pos<REUSE>(prm, readfirst(jb[t].x), readfirst64(first[t]), readfirst64(last[t]), blockp);
#pragma unroll
    for (int t = 0; t < 4; ++t) coff[t] = prm.chunk_off[readfirst64(last[t]) >> 32];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint64_t f = readfirst64(first[t]), la = readfirst64(last[t]);
      plain[t] = j0 + (uint32_t)t < njob && readfirst(jb[t].z) == 1u && la == f;
      if (j0 + (uint32_t)t < njob && !plain[t]) rest = true;
      dst[t] = pool + (uint64_t)readfirst(jb[t].y) * SEG;
      const uint8_t* src = prm.in + readfirst64(coff[t]) + (uint32_t)la;
      if (plain[t]) {
        v[t][0] = *(const u32x4_u*)(src + 32 * l);
        v[t][1] = *(const u32x4_u*)(src + 32 * l + 16);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (plain[t]) {
        *(u32x4_u*)(dst[t] + 32 * l) = v[t][0];
        *(u32x4_u*)(dst[t] + 32 * l + 16) = v[t][1];
      }
  }
  if (rest && l == 0) s_rest = 1u;
  __syncthreads();
  if (s_rest == 0u) return;
  for (uint32_t j = wv; j < njob; j += 4) {
    const uint4 jb = s_job[j];
    const uint32_t slot = readfirst(jb.x), dseg = readfirst(jb.y), jkind = readfirst(jb.z);
    const uint64_t first = readfirst64(prm.x.vals[slot]);
    const uint64_t last = commit_pos<REUSE>(prm, slot, first, readfirst64(prm.x_latest[slot]), blockp);
    if (jkind == 1u && last == first) continue;   // (copied above)
    const uint8_t* src = prm.in + prm.chunk_off[last >> 32] + (uint32_t)last;
    uint8_t* dst = pool + (uint64_t)dseg * SEG;
    if (jkind == 1 || !readfirst((uint32_t)dec_equal2048(dst, src))) wave_copy2048(dst, src);   // enter / replace (:130)
  }
}

// Name reuse, detection: one wave per listed duplicate (an EXTRACT of a hash
// after the one that claimed the hash's slot) compares its 2 KiB with the
// owner's.  A mismatch flags the slot -- every EXTRACT of an unflagged hash
// then holds the owner's bytes -- and counts the hash once.  `refuse` (bounded
// and pair contexts, whose passes do not model name reuse): status bit 9, so
// xcg_decode_batch declines (XCG_ENOTSUP) before anything is emitted or
// committed.
__global__ __launch_bounds__(256) void dec_dup_kernel(DecParams prm, uint32_t ndup, bool refuse) {
  const uint32_t e = blockIdx.x * 4u + (uint32_t)readfirst(threadIdx.x >> 6);
  if (e >= ndup) return;
  const uint32_t slot = readfirst(prm.dup_slot[e]);
  const uint64_t pos = readfirst64(prm.dup_pos[e]), own = readfirst64(prm.x_owner[slot]);
  const uint8_t* a = prm.in + prm.chunk_off[own >> 32] + (uint32_t)own;
  const uint8_t* b = prm.in + prm.chunk_off[pos >> 32] + (uint32_t)pos;
  if (dec_equal2048(a, b)) return;
  if (lane_id() == 0) {
    if (atomicExch(&prm.x_flag[slot], 1u) == 0u) atomicAdd(prm.nconf, 1u);
    if (refuse) atomicOr(prm.status, 1 << 9);
  }
}

// Name reuse, the rare path: every EXTRACT of a flagged hash as (hash,
// position) -- the slot owners (one thread per table slot), then the listed
// duplicates (one thread per entry).  `nocc` counts them; the arrays were
// filled with ~0, which sorts behind every hash.
__global__ __launch_bounds__(256) void dec_occ_owner_kernel(DecParams prm, uint64_t* okey, uint64_t* opos,
                                                            uint32_t* nocc, uint32_t cap) {
  const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (w > prm.x.mask) return;
  const uint64_t key = prm.x.keys[w];
  if (key == EMPTY_KEY || !prm.x_flag[w]) return;
  const uint32_t k = atomicAdd(nocc, 1u);
  if (k < cap) {
    okey[k] = key;
    opos[k] = prm.x_owner[w];
  }
}
__global__ __launch_bounds__(256) void dec_occ_dup_kernel(DecParams prm, uint32_t ndup, uint64_t* okey, uint64_t* opos,
                                                          uint32_t* nocc, uint32_t cap) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= ndup) return;
  const uint32_t slot = prm.dup_slot[e];
  if (!prm.x_flag[slot]) return;
  const uint32_t k = atomicAdd(nocc, 1u);
  if (k < cap) {
    okey[k] = prm.x.keys[slot];
    opos[k] = prm.dup_pos[e];
  }
}

}  // namespace xcg

// Diagnostics (bench.py's decode roofline): HIP events bracket the batch
// decode's three device segments on its stream -- scan, refcheck / sizing,
// emit + commit (the host's two readbacks between them are not device time)
// -- and the emit kernel alone; xcg_debug_decode_kernel_time sums them.
namespace {
std::mutex g_dt_mu;
bool g_dt_on = false;
std::vector<std::pair<hipEvent_t, hipEvent_t>> g_dt_step, g_dt_emit;
struct DecTimer {
  hipStream_t s;
  hipEvent_t e0 = nullptr;
  std::vector<std::pair<hipEvent_t, hipEvent_t>>* dst;
  DecTimer(hipStream_t st, std::vector<std::pair<hipEvent_t, hipEvent_t>>* d) : s(st), dst(d) {
    std::lock_guard<std::mutex> g(g_dt_mu);
    if (g_dt_on && hipEventCreate(&e0) == hipSuccess) (void)hipEventRecord(e0, s);
  }
  ~DecTimer() {
    if (e0) (void)hipEventDestroy(e0);   // (a path that did not reach its end: not counted)
  }
  void end() {
    if (!e0) return;
    std::lock_guard<std::mutex> g(g_dt_mu);
    hipEvent_t e1 = nullptr;
    if (hipEventCreate(&e1) == hipSuccess && hipEventRecord(e1, s) == hipSuccess) dst->emplace_back(e0, e1);
    e0 = nullptr;
  }
};
double dt_sum(std::vector<std::pair<hipEvent_t, hipEvent_t>>& v) {
  double tot = 0;
  for (auto& e : v) {
    float t = 0;
    if (hipEventSynchronize(e.second) == hipSuccess && hipEventElapsedTime(&t, e.first, e.second) == hipSuccess)
      tot += t;
    (void)hipEventDestroy(e.first);
    (void)hipEventDestroy(e.second);
  }
  v.clear();
  return tot;
}
}  // namespace
extern "C" int xcg_debug_decode_kernel_timing(int on) {
  std::lock_guard<std::mutex> g(g_dt_mu);
  const int old = g_dt_on;
  g_dt_on = on != 0;
  return old;
}
extern "C" int xcg_debug_decode_kernel_time(double* step_ms, double* emit_ms, uint32_t* segments) {
  std::lock_guard<std::mutex> g(g_dt_mu);
  if (segments) *segments = (uint32_t)g_dt_step.size();
  const double s = dt_sum(g_dt_step), e = dt_sum(g_dt_emit);
  if (step_ms) *step_ms = s;
  if (emit_ms) *emit_ms = e;
  return 0;
}

extern "C" void xcg_launch_exclusive_scan(const uint64_t* len, uint64_t* off, uint32_t n, uint64_t* total,
                                          hipStream_t stream) {
  hipLaunchKernelGGL(xcg::exclusive_scan_kernel, dim3(1), dim3(1024), 0, stream, len, off, n, total);
}

namespace {
// The kernels' parameter block from the driver's arguments (what a pass adds
// later -- ptime, D, the occurrences, the tail -- stays zero).
xcg::DecParams dec_params(const XcgDecodeArgs* a) {
  using namespace xcg;
  const uint32_t n = a->n;
  DecScratch* const d = a->scratch;
  DecParams p{};
  p.in = a->in;
  p.chunk_off = a->chunk_off;
  p.chunk_len = a->chunk_len;
  p.n = n;
  p.g = tab_of(a->g);
  p.pool = a->g.pool;
  p.x = HashTab{a->x_keys, a->x_vals, a->x_mask};
  p.x_latest = a->x_latest;
  p.out_len = a->out_len;
  p.out_off = a->out_off;
  p.out = a->out;
  p.chunk_status = a->chunk_status;
  p.consumed = a->consumed;
  p.unknown = a->unknown;
  p.unknown_pos = a->unknown_pos;
  p.nunknown = &a->counts->unknown;
  p.unknown_cap = a->unknown_cap;
  p.u_keys = a->u_keys;
  p.u_mask = 2 * a->unknown_cap - 1;
  p.block_pos = &d->block_pos;
  p.berr_pos = &d->berr_pos;
  p.t_end = &d->t_end;
  p.x_owner = a->x_owner;
  p.x_flag = a->x_flag;
  p.dup_ctr = &d->dup_minus1;
  p.dup_slot = a->dup_slot;
  p.dup_pos = a->dup_pos;
  p.dup_cap = a->dup_cap;
  p.nconf = &a->counts->flagged;
  p.status = a->status;
  p.n_decl = a->chunk_tmp;
  p.n_bref = a->chunk_tmp + n;
  p.decl_base = a->chunk_tmp + 2ull * n;
  p.n_decl_emit = a->chunk_tmp + 3ull * n;
  p.op_base = p.decl_base;
  p.win_hash = a->win_hash;
  p.win_seg = a->win_seg;
  p.win_count = a->win_count;
  if (a->wins) {
    p.wins = (WinView*)a->wins->views;
    p.chunk_win = a->wins->chunk_win;
    p.w_tend = a->wins->w_tend;
  }
  return p;
}

// The record pass over every declare and the BACKREF check (one window, or one
// per decoder when p.wins is set), as the
// classified path launches them ahead of its classification.  Defined behind
// xcg_launch_decode: the kernels are instantiated, and so laid out in the code
// object, in the order of their first use, and the paths that launch what they
// launched keep their kernels where they were.
void dec_launch_records(const xcg::DecParams& p, uint64_t ndecl, hipStream_t stream);
void dec_launch_brefcheck(const xcg::DecParams& p, hipStream_t stream);
}  // namespace

// The passes of the header comment in order: scan and declare numbering (one
// readback), duplicate EXTRACTs, (bounded / pair) classification -- behind the
// declare records and the BACKREF check when the batch holds BACKREFs, which
// the other contexts run after it --, refcheck and
// sizing (the second readback), (name reuse) the occurrence sort, emit, window
// update, commit.
// Returns 0, XCG_RC_OVERFLOW (output too small), XCG_RC_NOTSUP or XCG_RC_HIP.  Outputs: total decoded bytes, the
// REF block and BACKREF error positions (~0 = none), unknown-REF count.
extern "C" int xcg_launch_decode(const XcgDecodeArgs* a, uint64_t* total_out, uint64_t* block_pos_out,
                                 uint64_t* berr_pos_out, uint32_t* nunknown_out, hipStream_t stream) {
  using namespace xcg;
  const uint32_t n = a->n;
  DecScratch* const d = a->scratch;
  DecHostWords* const h = a->h_scratch;
  DecParams p = dec_params(a);
  h->reuse[0] = h->reuse[1] = h->reuse[2] = 0;
  const dim3 grid((n + 3) / 4), block(256);
  DecTimer seg1(stream, &g_dt_step);
  if (hipMemsetAsync(a->x_keys, 0xFF, 8ull * (a->x_mask + 1), stream) != hipSuccess ||
      hipMemsetAsync(a->x_vals, 0xFF, 8ull * (a->x_mask + 1), stream) != hipSuccess ||
      hipMemsetAsync(a->x_latest, 0, 8ull * (a->x_mask + 1), stream) != hipSuccess ||
      hipMemsetAsync(&d->block_pos, 0xFF, DEC_CLEAR_BYTES, stream) != hipSuccess ||   // (stop positions, duplicate count - 1)
      hipMemsetAsync(a->counts, 0, sizeof(*a->counts), stream) != hipSuccess ||
      hipMemsetAsync(a->u_keys, 0xFF, 16ull * a->unknown_cap, stream) != hipSuccess)
    return XCG_RC_HIP;
  // scan, then number the declares
  hipLaunchKernelGGL(decode_kernel<false>, grid, block, 0, stream, p);
  const bool classified = a->lru != nullptr || a->pair != nullptr;
  if (a->wins) {
    dec_windows_number(a->wins, p, &d->n_decl, stream);     // (per window)
    if (classified) p.op_base = dec_windows_op_base(a->wins, p, &d->n_decl, stream);   // (the op list stays in batch order)
  }
  else hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, stream, (const uint64_t*)p.n_decl,
                          (uint64_t*)p.decl_base, n, &d->n_decl);
  hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, stream, (const uint64_t*)p.n_bref,
                     p.n_decl_emit, n, &d->n_bref);              // (n_decl_emit: scratch output here)
  seg1.end();
  if (hipMemcpyAsync(&h->dup_minus1, &d->dup_minus1, DEC_SCAN_BYTES, hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return XCG_RC_HIP;
  const uint64_t ndup = h->dup_minus1 + 1u, ndecl = h->n_decl, nbref = h->n_bref;
  // Duplicate EXTRACTs (rare; none in an encoder's stream on a fresh cache):
  // compare each with its hash's owner and flag the hashes whose bytes differ.
  // The count of flagged hashes comes back with the sizing pass's readback.
  if (ndup > a->dup_cap) return XCG_RC_HIP;                  // (the list holds every EXTRACT the batch can have)
  h->reuse[0] = ndup;
  if (ndup) {
    if (hipMemsetAsync(a->x_flag, 0, 4ull * (a->x_mask + 1), stream) != hipSuccess) return XCG_RC_HIP;
    hipLaunchKernelGGL(dec_dup_kernel, dim3((unsigned)((ndup + 3) / 4)), dim3(256), 0, stream, p, (uint32_t)ndup,
                       classified);
  }
  // (the call's stream-ordered temporaries: each freed on `stream` at every exit)
  StreamTemp cls_tmp(stream), dfull_tmp(stream), occ_tmp(stream);
  // Bounded cache or pair: classify every op against the eviction times until
  // they agree (xcg_decode_bounded.hip); the passes below then see the cache as
  // it evolves.
  // BACKREFs there: the first one to an empty slot caps the classification (it
  // follows from the declares' hashes and the window alone, so the check runs
  // first, on records whose REF sources are made again once p.ptime stands).
  DecClassified K;
  uint4* dfull = nullptr;
  if (classified) {
    if (nbref > 0) {
      if (ndecl > 0) {
        if (!dfull_tmp.alloc(&dfull, 16ull * ndecl)) return XCG_RC_HIP;
        p.D = dfull;
        p.D_lo = 0;
        p.D_tail = false;
        dec_launch_records(p, ndecl, stream);
      }
      dec_launch_brefcheck(p, stream);
    }
    const int krc = dec_classify(a, p, ndecl, cls_tmp, &K, stream);
    if (krc) return krc;
    if (dfull) dec_launch_records(p, ndecl, stream);
  } else if (nbref > 0 && ndecl > 0) {
    // BACKREFs present: records of every declare (rare; never made by XCodecEncoder)
    if (!dfull_tmp.alloc(&dfull, 16ull * ndecl)) return XCG_RC_HIP;
    p.D = dfull;
    p.D_lo = 0;
    p.D_tail = false;
    if (a->wins) dec_windows_records(p, false, stream);
    else hipLaunchKernelGGL(decl_record_kernel<false>, grid, block, 0, stream, p, ndecl);
  }
  DecTimer seg2(stream, &g_dt_step);
  hipLaunchKernelGGL(decode_refcheck_kernel, grid, block, 0, stream, p);
  if (nbref > 0 && !classified) {
    if (a->wins) hipLaunchKernelGGL(decode_brefcheck_kernel<true>, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(decode_brefcheck_kernel<false>, grid, block, 0, stream, p);
  }
  hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, stream, (const uint64_t*)a->out_len, a->out_off,
                     n, &d->total_out);
  if (classified) dec_launch_precheck(p, stream);
  seg2.end();
  h->status = 0;
  if (hipMemcpyAsync(&h->total_out, &d->total_out, DEC_SIZING_BYTES, hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipMemcpyAsync(&h->unknown, &a->counts->unknown, DEC_COUNTS_BYTES, hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipMemcpyAsync(&h->status, a->status, 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return XCG_RC_HIP;
  const uint32_t nconf = h->flagged;
  h->reuse[1] = nconf;
  if (h->status & (1u << 9)) {
    // refused before any output, cache or window change (dec_dup_kernel, dec_precheck_kernel)
    h->status_wb = h->status & ~(uint64_t)(1u << 9);
    (void)hipMemcpyAsync(a->status, &h->status_wb, 4, hipMemcpyHostToDevice, stream);
    (void)hipStreamSynchronize(stream);
    return XCG_RC_NOTSUP;
  }
  *total_out = h->total_out;
  *block_pos_out = h->block_pos;
  *berr_pos_out = h->berr_pos;
  *nunknown_out = h->unknown;
  if (*total_out > a->out_cap) return XCG_RC_OVERFLOW;
  // Name reuse (hashes whose EXTRACTs differ; unbounded contexts only get
  // here): their occurrences sorted by (hash, position) -- a stable sort by
  // position, then by hash -- for the REUSE kernels' binary search.
  uint8_t* occ_mem = nullptr;
  if (nconf) {
    const uint32_t m = (uint32_t)ndup + nconf;       // owners of the flagged hashes + at most every duplicate
    uint64_t *k0 = nullptr, *k1 = nullptr, *v0 = nullptr, *v1 = nullptr;
    size_t tmp1 = 0, tmp2 = 0;
    if (rocprim::radix_sort_pairs(nullptr, tmp1, v0, v1, k0, k1, m, 0, 64, stream) != hipSuccess ||
        rocprim::radix_sort_pairs(nullptr, tmp2, k1, k0, v1, v0, m, 0, 64, stream) != hipSuccess ||
        !occ_tmp.alloc(&occ_mem, 32ull * m + 256 + (tmp1 > tmp2 ? tmp1 : tmp2)))
      return XCG_RC_HIP;
    k0 = (uint64_t*)occ_mem; k1 = k0 + m; v0 = k1 + m; v1 = v0 + m;
    void* tmp = (void*)(((uintptr_t)(v1 + m) + 255) & ~(uintptr_t)255);
    uint32_t* nocc = &a->counts->occurrences;
    if (hipMemsetAsync(occ_mem, 0xFF, 32ull * m, stream) != hipSuccess) return XCG_RC_HIP;
    hipLaunchKernelGGL(dec_occ_owner_kernel, dim3((unsigned)(((uint64_t)a->x_mask + 256) / 256)), dim3(256), 0, stream,
                       p, k0, v0, nocc, m);
    hipLaunchKernelGGL(dec_occ_dup_kernel, dim3((unsigned)((ndup + 255) / 256)), dim3(256), 0, stream, p, (uint32_t)ndup,
                       k0, v0, nocc, m);
    if (rocprim::radix_sort_pairs(tmp, tmp1, v0, v1, k0, k1, m, 0, 64, stream) != hipSuccess ||
        rocprim::radix_sort_pairs(tmp, tmp2, k1, k0, v1, v0, m, 0, 64, stream) != hipSuccess)
      return XCG_RC_HIP;
    p.occ_key = k0;
    p.occ_pos = v0;
    p.nocc = m;
    h->reuse[2] = 1;
    // (BACKREFs: the records made before the sizing pass carry the earliest
    // EXTRACT as a flagged REF's source; the hashes, all the checks read, stand)
    if (dfull) {
      if (a->wins) dec_windows_records(p, true, stream);
      else hipLaunchKernelGGL(decl_record_kernel<true>, grid, block, 0, stream, p, ndecl);
    }
  }
  DecTimer seg3(stream, &g_dt_step), emit(stream, &g_dt_emit);
  // No stop point: the declares end at ndecl, so the window's tail is known
  // now and the emit pass records it (no second walk over the ops).
  // (Several windows: every tail comes from dec_windows_finish's record pass.)
  const bool fuse_tail = !a->wins && !a->no_window && !dfull && *block_pos_out == ~0ull && *berr_pos_out == ~0ull;
  if (fuse_tail) {
    p.tail_D = a->d_tail;
    p.tail_hi = ndecl;
    p.tail_lo = ndecl > 256u ? ndecl - 256u : 0u;
  }
  if (a->wins) {
    if (nconf) hipLaunchKernelGGL((decode_kernel<true, true, true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((decode_kernel<true, false, true>), grid, block, 0, stream, p);
  } else {
    if (nconf) hipLaunchKernelGGL((decode_kernel<true, true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((decode_kernel<true, false>), grid, block, 0, stream, p);
  }
  emit.end();
  p.tail_D = nullptr;
  if (a->wins) {
    dec_windows_finish(a->wins, p, dfull != nullptr, nconf != 0, stream);
  } else {
    hipLaunchKernelGGL(decode_tend_kernel, dim3(1), dim3(1), 0, stream, p, ndecl);
  }
  if (!a->wins && !a->no_window) {
    if (!dfull) {
      p.D = a->d_tail;
      p.D_tail = true;
      if (!fuse_tail) {
        if (nconf) hipLaunchKernelGGL(decl_record_kernel<true>, grid, block, 0, stream, p, ndecl);
        else hipLaunchKernelGGL(decl_record_kernel<false>, grid, block, 0, stream, p, ndecl);
      }
    }
    hipLaunchKernelGGL(window_update_kernel, dim3(64), dim3(256), 0, stream, p);
  }
  if (classified) return dec_classified_commit(a, p, K, stream);
  const uint64_t slots = (uint64_t)a->x_mask + 1;
  const FiltSet fs = filters_of(a->g);
  if (nconf)
    hipLaunchKernelGGL(decode_commit_kernel<true>, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, stream, p,
                       a->g.pool, a->g.nseg, a->g.seg_cap, fs);
  else
    hipLaunchKernelGGL(decode_commit_kernel<false>, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, stream, p,
                       a->g.pool, a->g.nseg, a->g.seg_cap, fs);
  seg3.end();
  return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}

namespace {
void dec_launch_records(const xcg::DecParams& p, uint64_t ndecl, hipStream_t stream) {
  if (p.wins) xcg::dec_windows_records(p, false, stream);
  else hipLaunchKernelGGL(xcg::decl_record_kernel<false>, dim3((p.n + 3) / 4), dim3(256), 0, stream, p, ndecl);
}
void dec_launch_brefcheck(const xcg::DecParams& p, hipStream_t stream) {
  if (p.wins) hipLaunchKernelGGL(xcg::decode_brefcheck_kernel<true>, dim3((p.n + 3) / 4), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(xcg::decode_brefcheck_kernel<false>, dim3((p.n + 3) / 4), dim3(256), 0, stream, p);
}
}  // namespace
