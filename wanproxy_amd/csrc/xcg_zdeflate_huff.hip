// Deflate stage, third phase: per block the Huffman trees and the stored / static / dynamic choice, per call the
// layout of its output, then every block's bits (the map of a call's arrays is at the top of xcg_zdeflate.h).
#include "xcg_zdeflate.h"

namespace xcg {
namespace zd {

// trees.c: the codes' extra bits, the order the bit-length code lengths are sent in, the codes' base values
__constant__ uint8_t XLB[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint8_t XDB[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t XBB[19] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 3, 7};
__constant__ uint8_t BL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
__constant__ uint16_t BASE_LEN[29] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 0};
__constant__ uint16_t BASE_DIST[30] = {0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768,
                                       1024, 1536, 2048, 3072, 4096, 6144, 8192, 12288, 16384, 24576};

// ------------------------------------------------------------------- trees
// Heap entries are freq << 15 | depth << 10 | node: trees.c's smaller(n, m)
// (freq, then depth <=) is `key(n) <= key(m)` on key = entry >> 10, so a
// downheap step is one 8-byte LDS read of both children.  A block holds at
// most 16383 symbols + END_BLOCK (+2 forced), so freq < 2^17, and a Huffman
// tree over that total weight is at most ~21 deep (Fibonacci bound): depth
// fits 5 bits, nodes (< 573) 10.
struct TreeLds {
  uint32_t heap[HEAP_SIZE + 1];
  uint16_t dl[HEAP_SIZE + 1];  // Dad | Len
  uint16_t fc[L_CODES];        // leaf Freq | Code
  uint16_t dfc[D_CODES], ddl[2 * D_CODES + 1];
  uint16_t bfc[BL_CODES], bdl[2 * BL_CODES + 1];
  uint16_t lfreq[L_CODES], dfreq[D_CODES], bfreq[BL_CODES + 1];   // real counts (forced codes excluded)
  uint16_t bl_count[MAX_BITS + 1];
  uint32_t next_code[MAX_BITS + 1];
  int64_t opt_len, static_len;
};
// one TreeLds per lane-owned block, at a stride of 4 mod 64 words (16-byte aligned, no bank conflicts
// between the TB lanes)
constexpr int TB_BATCH = 2;   // blocks per wave in batches (one per wave when few blocks)
constexpr uint32_t TSTRIDE = ((sizeof(TreeLds) + 255) / 256) * 256 + 16;

__device__ __forceinline__ uint32_t hkey(uint32_t e) { return e >> 10; }
// Two levels per LDS round trip: the children pair and the four grandchildren
// are read together (stores along the path go to indices below both).
__device__ void downheap(TreeLds& s, int k, int len) {
  const uint32_t v = s.heap[k], kv = hkey(v);
  int j = k << 1;
  while (j <= len) {
    const uint2 p = *(const uint2*)&s.heap[j];   // j even
    uint4 g = make_uint4(0, 0, 0, 0);
    if (2 * j <= len) g = *(const uint4*)&s.heap[2 * j];   // 2j % 4 == 0
    uint32_t e = p.x;
    if (j < len && hkey(p.y) <= hkey(p.x)) {
      e = p.y;
      j++;
    }
    if (kv <= hkey(e)) break;
    s.heap[k] = e;
    k = j;
    const bool right = j & 1;
    j <<= 1;
    if (j > len) break;
    const uint32_t e0 = right ? g.z : g.x, e1 = right ? g.w : g.y;
    e = e0;
    if (j < len && hkey(e1) <= hkey(e0)) {
      e = e1;
      j++;
    }
    if (kv <= hkey(e)) break;
    s.heap[k] = e;
    k = j;
    j <<= 1;
  }
  s.heap[k] = v;
}
__device__ __forceinline__ int static_llen(int n) { return n < 144 ? 8 : n < 256 ? 9 : n < 280 ? 7 : 8; }

// trees.c build_tree + gen_bitlen + gen_codes.  kind: 0 literal/length, 1 distance, 2 bit length.
__device__ int build_tree(TreeLds& s, uint16_t* fc, uint16_t* dl, int elems, int kind) {
  const int maxlen = kind == 2 ? 7 : MAX_BITS;
  int n, m, max_code = -1, node;
  int len = 0, hmax = HEAP_SIZE;
  for (n = 0; n < elems; n++) {
    if (fc[n]) {
      s.heap[++len] = ((uint32_t)fc[n] << 15) | (uint32_t)n;
      max_code = n;
    } else {
      dl[n] = 0;
    }
  }
  while (len < 2) {
    node = max_code < 2 ? ++max_code : 0;
    s.heap[++len] = (1u << 15) | (uint32_t)node;
    fc[node] = 1;
    s.opt_len--;
    if (kind == 0) s.static_len -= static_llen(node);
    else if (kind == 1) s.static_len -= 5;
  }
  for (n = len / 2; n >= 1; n--) downheap(s, n, len);
  node = elems;
  do {
    const uint32_t en = s.heap[1];
    s.heap[1] = s.heap[len--];
    downheap(s, 1, len);
    const uint32_t em = s.heap[1];
    s.heap[--hmax] = en;
    s.heap[--hmax] = em;
    const uint32_t dn = (en >> 10) & 31, dm = (em >> 10) & 31;
    const uint32_t f = (en >> 15) + (em >> 15), d = (dn >= dm ? dn : dm) + 1;
    dl[en & 1023] = dl[em & 1023] = (uint16_t)node;
    s.heap[1] = (f << 15) | (d << 10) | (uint32_t)node++;
    downheap(s, 1, len);
  } while (len >= 2);
  s.heap[--hmax] = s.heap[1];

  int h, bits, overflow = 0;
  for (bits = 0; bits <= MAX_BITS; bits++) s.bl_count[bits] = 0;
  dl[s.heap[hmax] & 1023] = 0;
  for (h = hmax + 1; h < HEAP_SIZE; h++) {
    n = s.heap[h] & 1023;
    bits = dl[dl[n]] + 1;
    if (bits > maxlen) {
      bits = maxlen;
      overflow++;
    }
    dl[n] = (uint16_t)bits;
    if (n > max_code) continue;
    s.bl_count[bits]++;
    int xb = 0;
    if (kind == 0 && n >= 257) xb = XLB[n - 257];
    else if (kind == 1) xb = XDB[n];
    else if (kind == 2) xb = XBB[n];
    s.opt_len += (int64_t)fc[n] * (bits + xb);
    if (kind == 0) s.static_len += (int64_t)fc[n] * (static_llen(n) + xb);
    else if (kind == 1) s.static_len += (int64_t)fc[n] * (5 + xb);
  }
  if (overflow) {
    do {
      bits = maxlen - 1;
      while (s.bl_count[bits] == 0) bits--;
      s.bl_count[bits]--;
      s.bl_count[bits + 1] += 2;
      s.bl_count[maxlen]--;
      overflow -= 2;
    } while (overflow > 0);
    for (bits = maxlen; bits != 0; bits--) {
      n = s.bl_count[bits];
      while (n != 0) {
        m = s.heap[--h] & 1023;
        if (m > max_code) continue;
        if (dl[m] != (unsigned)bits) {
          s.opt_len += ((int64_t)bits - dl[m]) * fc[m];
          dl[m] = (uint16_t)bits;
        }
        n--;
      }
    }
  }
  uint32_t code = 0;
  for (bits = 1; bits <= MAX_BITS; bits++) {
    code = (code + s.bl_count[bits - 1]) << 1;
    s.next_code[bits] = code;
  }
  for (n = 0; n <= max_code; n++) {
    const int l = dl[n];
    if (l) fc[n] = (uint16_t)bitrev(s.next_code[l]++, l);
  }
  return max_code;
}

// scan_tree: bit-length code frequencies of one tree's lengths (guard: 0xffff)
__device__ void scan_tree(TreeLds& s, const uint16_t* dl, int max_code) {
  int prevlen = -1, curlen, nextlen = dl[0], count = 0, max_count = 7, min_count = 4;
  if (nextlen == 0) {
    max_count = 138;
    min_count = 3;
  }
  for (int n = 0; n <= max_code; n++) {
    curlen = nextlen;
    nextlen = n + 1 <= max_code ? dl[n + 1] : 0xffff;
    if (++count < max_count && curlen == nextlen) continue;
    if (count < min_count) s.bfreq[curlen] += count;
    else if (curlen != 0) {
      if (curlen != prevlen) s.bfreq[curlen]++;
      s.bfreq[16]++;
    } else if (count <= 10) s.bfreq[17]++;
    else s.bfreq[18]++;
    count = 0;
    prevlen = curlen;
    if (nextlen == 0) {
      max_count = 138;
      min_count = 3;
    } else if (curlen == nextlen) {
      max_count = 6;
      min_count = 3;
    } else {
      max_count = 7;
      min_count = 4;
    }
  }
}

// One wave per block: histogram, trees, the _tr_flush_block decision and the
// block's exact bit count; code tables to `tabs`.
// TB blocks per wave: the wave builds each block's symbol histogram in turn,
// then lane t runs block t's trees (the heap work is a serial chain per
// block; one lane per block spends the wave's VALU issue slots on TB chains
// instead of one), then the code tables leave with the whole wave.
template <int TB>
__global__ __launch_bounds__(64) void zd_trees_kernel(ZArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t raw[TB * TSTRIDE];
  __shared__ int ttype[TB];
  const int lane = threadIdx.x;
  const uint32_t nrec = a.bstart[a.n];
  uint64_t tz = ZD_NOW();
  for (int t = 0; t < TB; t++) {
    const uint32_t bi = blockIdx.x * TB + t;
    if (lane == 0) ttype[t] = -1;
    if (bi >= nrec) continue;
    const uint32_t ci = call_of(a.bstart, a.n, bi);
    const ZCall c = a.calls[ci];
    if (bi - c.blk_off >= a.res[ci].nblocks) continue;
    TreeLds& s = *(TreeLds*)(raw + t * TSTRIDE);
    uint32_t* hist = s.heap;   // the symbol counts live in the block's heap until build_tree
    for (int i = lane; i < L_CODES + D_CODES; i += 64) hist[i] = 0;
    __syncthreads();
    const ZBlock* B = a.blk + bi;
    const uint32_t* sym = a.sym + c.t_off;
    const uint32_t sb = B->sym_begin, se = B->sym_end;
    for (uint32_t i0 = sb; i0 < se; i0 += 64 * 8) {
      uint32_t v[8];
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const uint32_t i = i0 + 64 * q + lane;
        v[q] = i < se ? sym[i] : 0xffffffffu;
      }
#pragma unroll
      for (int q = 0; q < 8; q++) {
        if (v[q] == 0xffffffffu) continue;
        const uint32_t dist = v[q] >> 8;
        if (dist == 0) atomicAdd(&hist[v[q] & 255], 1u);
        else {
          atomicAdd(&hist[257 + len_code(v[q] & 255)], 1u);
          atomicAdd(&hist[L_CODES + dist_code(dist - 1)], 1u);
        }
      }
    }
    __syncthreads();
    for (int i = lane; i < L_CODES; i += 64) {
      const uint16_t f = i == 256 ? 1 : (uint16_t)hist[i];
      s.lfreq[i] = f;
      s.fc[i] = f;
    }
    if (lane < D_CODES) s.dfreq[lane] = s.dfc[lane] = (uint16_t)hist[L_CODES + lane];
    if (lane <= BL_CODES) s.bfreq[lane] = 0;
    if (lane == 0) ttype[t] = 0;
    __syncthreads();
  }
  ZD_ADD(0, tz);
  if (lane < TB && ttype[lane] >= 0) {
    TreeLds& s = *(TreeLds*)(raw + lane * TSTRIDE);
    ZBlock* B = a.blk + blockIdx.x * TB + lane;
    s.opt_len = s.static_len = 0;
    int lmax = build_tree(s, s.fc, s.dl, L_CODES, 0);
    ZD_ADD(1, tz);
    int dmax = build_tree(s, s.dfc, s.ddl, D_CODES, 1);
    scan_tree(s, s.dl, lmax);
    scan_tree(s, s.ddl, dmax);
    for (int i = 0; i < BL_CODES; i++) s.bfc[i] = s.bfreq[i];
    build_tree(s, s.bfc, s.bdl, BL_CODES, 2);
    int max_blindex;
    for (max_blindex = BL_CODES - 1; max_blindex >= 3; max_blindex--)
      if (s.bdl[BL_ORDER[max_blindex]] != 0) break;
    s.opt_len += 3 * ((int64_t)max_blindex + 1) + 5 + 5 + 4;
    ZD_ADD(2, tz);
    int64_t opt_lenb = (s.opt_len + 3 + 7) >> 3, static_lenb = (s.static_len + 3 + 7) >> 3;
    if (static_lenb <= opt_lenb) opt_lenb = static_lenb;
    uint32_t type;
    if ((int64_t)B->stored_len + 4 <= opt_lenb && (B->flags & 1)) type = 0;
    else if (static_lenb == opt_lenb) type = 1;
    else type = 2;
    // exact bits of a Huffman block (real symbol counts; forced codes emit nothing)
    uint64_t bits = 3;
    if (type == 1) {
      for (int i = 0; i < L_CODES; i++)
        bits += (uint64_t)s.lfreq[i] * (static_llen(i) + (i >= 257 ? XLB[i - 257] : 0));
      for (int i = 0; i < D_CODES; i++) bits += (uint64_t)s.dfreq[i] * (5 + XDB[i]);
    } else if (type == 2) {
      bits += 14 + 3 * (uint64_t)(max_blindex + 1);
      for (int i = 0; i < BL_CODES; i++) bits += (uint64_t)s.bfreq[i] * (s.bdl[i] + XBB[i]);
      for (int i = 0; i < L_CODES; i++) bits += (uint64_t)s.lfreq[i] * (s.dl[i] + (i >= 257 ? XLB[i - 257] : 0));
      for (int i = 0; i < D_CODES; i++) bits += (uint64_t)s.dfreq[i] * (s.ddl[i] + XDB[i]);
    }
    B->type = type;
    B->bits = bits;
    B->lcodes = lmax + 1;
    B->dcodes = dmax + 1;
    B->blcodes = max_blindex + 1;
    ttype[lane] = (int)type;
    ZD_ADD(3, tz);
  }
  __syncthreads();
  for (int t = 0; t < TB; t++) {
    if (ttype[t] != 2) continue;
    const TreeLds& s = *(const TreeLds*)(raw + t * TSTRIDE);
    uint32_t* tab = a.tabs + (uint64_t)(blockIdx.x * TB + t) * TAB_WORDS;
    for (int i = lane; i < L_CODES; i += 64) tab[i] = s.fc[i] | ((uint32_t)s.dl[i] << 16);
    if (lane < D_CODES) tab[L_CODES + lane] = s.dfc[lane] | ((uint32_t)s.ddl[lane] << 16);
    if (lane < BL_CODES) tab[L_CODES + D_CODES + lane] = s.bfc[lane] | ((uint32_t)s.bdl[lane] << 16);
  }
  ZD_ADD(4, tz);
#ifdef XCG_ZD_TIMING
  if (lane == 0) atomicAdd(&g_zd_t[14], 1ull);
#endif
}

// ------------------------------------------------------------------- layout
// One wave per call: block bit offsets, the call's length, zeroed output, and
// where DeflatePipe::consume (zlib/deflate_pipe.cc:57-115) stops.  Output
// reaches the pipe at every block flush (flush_pending: the complete bytes).
// Under Z_NO_FLUSH the pipe takes all of it, emptying its 64 KiB buffer as it
// fills, so the one deflate(Z_SYNC_FLUSH) call starts with n mod 65536 bytes
// in the buffer (n = the bytes the consume took so far, the ones zlib still
// held from the last consume included) and returns at the first block flush
// that leaves the buffer full (FLUSH_BLOCK's need_more): the consume produces
// up to L = 65536 * (n / 65536 + 1), the rest stays pending, no sync marker
// is written, and positions after that flush are parsed with the next
// consume's bytes.  Otherwise the marker follows and the consume produces
// min(all, L).  Bits of an incomplete last byte carry into the next call
// (the call's output starts with them).
__global__ __launch_bounds__(64) void zd_layout_kernel(ZArgs a) {
  const uint32_t ci = blockIdx.x;
  const ZCall c = a.calls[ci];
  const ZState s = a.st[c.stream];
  const int lane = threadIdx.x;
  __shared__ uint32_t total_bytes;
  if (lane == 0) {
    uint64_t off = (s.flags & 1) ? s.cnb : 16;   // carried bits, or the zlib header on the first call
    const uint32_t nb = a.res[ci].nblocks;
    const bool finish = c.len == 0;
    bool last = false;
    uint32_t stop = 0, nemit = nb;
    uint64_t n = s.pend;                          // bytes the consume took before its flush call
    for (uint32_t k = 0; k < nb; k++) {
      ZBlock* B = a.blk + c.blk_off + k;
      B->bit_off = off;
      if (B->type == 0) off = (((off + 3 + 7) >> 3) + 4 + B->stored_len) * 8;
      else off += B->bits;
      if (B->flags & 2) {
        off = (off + 7) & ~7ull;   // bi_windup after the last block
        last = true;
      }
      if (finish) continue;
      const uint64_t avail = s.pend + (off >> 3);
      if (!(B->flags & 4)) {
        n = avail;
      } else if (avail >= (uint64_t)PIPE_CHUNK * (n / PIPE_CHUNK + 1)) {
        stop = k + 1;
        nemit = k + 1;
        break;
      }
    }
    ZCallRes& r = a.res[ci];
    r.end_bit = off;
    r.nblocks = nemit;
    r.stop = stop;
    uint64_t bytes, room;
    if (last) bytes = room = off / 8 + 4;                           // adler32 trailer
    else if (stop) { bytes = off >> 3; room = (off + 7) >> 3; }     // no marker; the partial byte carries
    else bytes = room = ((off + 3 + 7) >> 3) + 4;                   // Z_SYNC_FLUSH: empty stored block
    const uint64_t lim = (uint64_t)PIPE_CHUNK * (n / PIPE_CHUNK + 1), all = s.pend + bytes;
    r.deliver = finish ? all : (all < lim ? all : lim);
    r.out_bytes = (uint32_t)bytes;
    total_bytes = (uint32_t)room;
    r.out_len = (uint32_t)room;
    a.out_len[ci] = (uint32_t)bytes;
    a.deliver[ci] = r.deliver;
  }
  __syncthreads();
  uint32_t* o = (uint32_t*)(a.out + c.out_off);
  uint32_t words = (total_bytes + 3) / 4;
  for (uint32_t i = lane; i < words; i += 64) o[i] = 0;
  __syncthreads();
  if (lane == 0 && (s.flags & 1) && s.cnb) o[0] |= s.cbits;   // (the header call starts byte-aligned)
}

// ------------------------------------------------------------------- emit
// Output words of one call: writes past its computed length are dropped (they
// cannot happen when the layout is right; the guard keeps a bug from touching
// another call's output).
struct OutW {
  uint32_t* o;
  uint64_t nwords;
};
__device__ __forceinline__ void or_word(OutW o, uint64_t wi, uint32_t v) {
  if (v && wi < o.nwords) atomicOr(o.o + wi, v);
}
__device__ __forceinline__ void or_bits(OutW o, uint64_t pos, uint64_t v, int nb) {
  // v < 2^nb, nb <= 48: spans at most three words
  if (nb == 0) return;
  uint64_t wi = pos >> 5;
  int sh = (int)(pos & 31);
  uint64_t lo = v << sh;                     // bits [sh, sh + nb) of a 96-bit window
  or_word(o, wi, (uint32_t)lo);
  or_word(o, wi + 1, (uint32_t)(lo >> 32));
  if (sh) or_word(o, wi + 2, (uint32_t)(v >> (64 - sh)));
}
__device__ __forceinline__ void or_byte(OutW o, uint64_t byte, uint32_t v) {
  or_word(o, byte >> 2, v << (8 * (byte & 3)));
}

// Huffman blocks are packed through an LDS ring of output words: absolute
// word w of the call's output lives in ring[w % RING] until it is complete.
constexpr int RING = 512;
struct RingW {          // lane-0 sequential writer (block header, tree description)
  uint32_t* ring;
  uint64_t pos;
  __device__ void put(uint32_t v, int n) {   // v < 2^n, n <= 16
    const uint64_t x = (uint64_t)v << (pos & 31);
    const uint64_t w = pos >> 5;
    if ((uint32_t)x) atomicOr(&ring[w % RING], (uint32_t)x);
    if (x >> 32) atomicOr(&ring[(w + 1) % RING], (uint32_t)(x >> 32));
    pos += n;
  }
};

__device__ void send_tree(RingW& bw, const uint32_t* tab, int max_code, const uint32_t* btab) {
  int prevlen = -1, curlen, nextlen = tab[0] >> 16, count = 0, max_count = 7, min_count = 4;
  if (nextlen == 0) {
    max_count = 138;
    min_count = 3;
  }
  auto code = [&](int c) { bw.put(btab[c] & 0xffff, btab[c] >> 16); };
  for (int n = 0; n <= max_code; n++) {
    curlen = nextlen;
    nextlen = n + 1 <= max_code ? (int)(tab[n + 1] >> 16) : 0xffff;
    if (++count < max_count && curlen == nextlen) continue;
    if (count < min_count) {
      do code(curlen);
      while (--count != 0);
    } else if (curlen != 0) {
      if (curlen != prevlen) {
        code(curlen);
        count--;
      }
      code(16);
      bw.put(count - 3, 2);
    } else if (count <= 10) {
      code(17);
      bw.put(count - 3, 3);
    } else {
      code(18);
      bw.put(count - 11, 7);
    }
    count = 0;
    prevlen = curlen;
    if (nextlen == 0) {
      max_count = 138;
      min_count = 3;
    } else if (curlen == nextlen) {
      max_count = 6;
      min_count = 3;
    } else {
      max_count = 7;
      min_count = 4;
    }
  }
}

__device__ __forceinline__ uint32_t static_lcode(int n) {   // fixed literal/length tree (code | len << 16)
  uint32_t len, code;
  if (n < 144) { len = 8; code = 0x30 + n; }
  else if (n < 256) { len = 9; code = 0x190 + (n - 144); }
  else if (n < 280) { len = 7; code = n - 256; }
  else { len = 8; code = 0xc0 + (n - 280); }
  return bitrev(code, len) | (len << 16);
}

// One wave per block.  Huffman blocks: per-block LDS tables give every symbol
// its bits with the extra bits merged (literal: code; length: code + extra;
// distance: code + extra), 64 symbols per step are loaded coalesced (prefetched
// a step ahead), a wave scan places them, they are OR-ed into the LDS ring, and
// completed words leave with coalesced stores -- the block's first and last
// words (shared with its neighbours) with atomicOr.
constexpr int EBATCH = 4;   // 64-symbol steps per prefetch
__global__ __launch_bounds__(64) void zd_emit_kernel(ZArgs a) {
  __shared__ uint32_t litx[256], lenx[256], dtx[D_CODES];   // bits | nbits << 24 (dist: code | nbits << 16)
  __shared__ uint32_t stab[TAB_WORDS];
  __shared__ uint32_t ring[RING];
  const uint32_t bi = blockIdx.x;
  const uint32_t ci = call_of(a.bstart, a.n, bi);
  const ZCall c = a.calls[ci];
  const uint32_t k = bi - c.blk_off;
  const ZCallRes r = a.res[ci];
  if (k >= r.nblocks) return;
  const ZBlock B = a.blk[bi];
  const ZState s = a.st[c.stream];
  const int lane = threadIdx.x;
  uint64_t tz = ZD_NOW();
  const OutW o{(uint32_t*)(a.out + c.out_off), (r.out_len + 3ull) / 4};
  const OutW ob = o;
  const bool last = B.flags & 2;
  if (k == 0 && lane == 0 && !(s.flags & 1)) {   // zlib header (deflate.c: 0x78, level flags)
    int lf = a.level < 2 ? 0 : a.level < 6 ? 1 : a.level == 6 ? 2 : 3;
    uint32_t hdr = ((8 + (7 << 4)) << 8) | (lf << 6);
    hdr += 31 - (hdr % 31);
    or_byte(ob, 0, hdr >> 8);
    or_byte(ob, 1, hdr & 0xff);
  }
  if (B.type == 0) {   // _tr_stored_block
    if (lane == 0) {
      or_bits(o, B.bit_off, last ? 1 : 0, 3);
      uint64_t db = (B.bit_off + 3 + 7) >> 3;
      uint32_t L = B.stored_len;
      or_byte(ob, db, L & 0xff);
      or_byte(ob, db + 1, (L >> 8) & 0xff);
      or_byte(ob, db + 2, ~L & 0xff);
      or_byte(ob, db + 3, (~L >> 8) & 0xff);
    }
    const uint8_t* X = a.X + c.x_off + B.start;
    uint64_t db = ((B.bit_off + 3 + 7) >> 3) + 4;
    // whole words inside [db, db + L) by plain stores, the edge words by atomicOr
    uint64_t w0 = (db + 3) >> 2, w1 = (db + B.stored_len) >> 2;
    for (uint64_t wi = w0 + lane; wi < w1 && wi < o.nwords; wi += 64) {
      uint64_t b = wi * 4 - db;
      o.o[wi] = ld32(X + b);
    }
    for (uint64_t i = lane; i < B.stored_len; i += 64) {
      uint64_t byte = db + i;
      if ((byte >> 2) < w0 || (byte >> 2) >= w1) or_byte(ob, byte, X[i]);
    }
  } else {
    const bool dyn = B.type == 2;
    const uint32_t* tab = a.tabs + (uint64_t)bi * TAB_WORDS;
    if (dyn)
      for (int i = lane; i < TAB_WORDS; i += 64) stab[i] = tab[i];
    for (int i = lane; i < RING; i += 64) ring[i] = 0;
    __syncthreads();
    auto lcode = [&](int n) { return dyn ? stab[n] : static_lcode(n); };
    for (int i = lane; i < 256; i += 64) {
      const uint32_t t = lcode(i);
      litx[i] = (t & 0xffff) | ((t >> 16) << 24);
      const int code = len_code(i), xl = XLB[code];
      const uint32_t u = lcode(257 + code), hl = u >> 16;
      lenx[i] = ((u & 0xffff) | (xl ? (uint32_t)(i - BASE_LEN[code]) << hl : 0u)) | ((hl + xl) << 24);
    }
    if (lane < D_CODES) dtx[lane] = dyn ? stab[L_CODES + lane] : (bitrev(lane, 5) | (5u << 16));
    const uint32_t eob = lcode(256);
    uint64_t pos = B.bit_off;
    __syncthreads();
    if (lane == 0) {
      RingW bw{ring, pos};
      bw.put((B.type << 1) | (last ? 1 : 0), 3);
      if (dyn) {
        const uint32_t* btab = stab + L_CODES + D_CODES;
        bw.put(B.lcodes - 257, 5);
        bw.put(B.dcodes - 1, 5);
        bw.put(B.blcodes - 4, 4);
        for (uint32_t rk = 0; rk < B.blcodes; rk++) bw.put(btab[BL_ORDER[rk]] >> 16, 3);
        send_tree(bw, stab, B.lcodes - 1, btab);
        send_tree(bw, stab + L_CODES, B.dcodes - 1, btab);
      }
      pos = bw.pos;
    }
    pos = readlane64(pos, 0);
    __syncthreads();
    ZD_ADD(8, tz);
    const uint64_t wfirst = B.bit_off >> 5;
    uint64_t flushed = wfirst;
    auto flush = [&](uint64_t upto) {   // words [flushed, upto) are complete
      for (uint64_t w = flushed + lane; w < upto; w += 64) {
        const uint32_t v = ring[w % RING];
        ring[w % RING] = 0;
        if (w == wfirst) or_word(o, w, v);
        else if (w < o.nwords) o.o[w] = v;
      }
      flushed = upto;
    };
    const uint32_t* sym = a.sym + c.t_off;
    const uint32_t sb = B.sym_begin, se = B.sym_end;
    uint32_t cur[EBATCH], nxt[EBATCH];
#pragma unroll
    for (int q = 0; q < EBATCH; q++) {
      const uint32_t i = sb + 64 * q + lane;
      cur[q] = i < se ? sym[i] : 0xffffffffu;
    }
    for (uint32_t b0 = sb; b0 < se; b0 += 64 * EBATCH) {
#pragma unroll
      for (int q = 0; q < EBATCH; q++) {
        const uint32_t i = b0 + 64 * (EBATCH + q) + lane;
        nxt[q] = i < se ? sym[i] : 0xffffffffu;
      }
#pragma unroll
      for (int q = 0; q < EBATCH; q++) {
        if (b0 + 64 * q >= se) break;
        const uint32_t e = cur[q];
        uint64_t v = 0;
        uint32_t nb = 0;
        if (e != 0xffffffffu) {
          const uint32_t dist = e >> 8;
          if (dist == 0) {
            const uint32_t t = litx[e & 255];
            v = t & 0xffffff;
            nb = t >> 24;
          } else {
            const uint32_t t = lenx[e & 255];
            const uint32_t d = dist - 1;
            const int dc = dist_code(d);
            const uint32_t td = dtx[dc], hd = td >> 16;
            const uint32_t xd = d < 4 ? 0u : (uint32_t)(31 - __clz(d)) - 1u;   // XDB[dc]
            const uint32_t v1 = (td & 0xffff) | ((d & ((1u << xd) - 1u)) << hd);
            const uint32_t n0 = t >> 24;
            v = (uint64_t)(t & 0xffffff) | ((uint64_t)v1 << n0);
            nb = n0 + hd + xd;
          }
        }
        const uint32_t incl = wave_incl_scan(nb);
        if (nb) {
          const uint64_t P = pos + incl - nb;
          const uint64_t w = P >> 5;
          const uint32_t sh = (uint32_t)(P & 31);
          const uint64_t lo = v << sh;
          if ((uint32_t)lo) atomicOr(&ring[w % RING], (uint32_t)lo);
          if (lo >> 32) atomicOr(&ring[(w + 1) % RING], (uint32_t)(lo >> 32));
          if (sh && (v >> (64 - sh))) atomicOr(&ring[(w + 2) % RING], (uint32_t)(v >> (64 - sh)));
        }
        pos += readlane(incl, 63);
        flush(pos >> 5);
      }
#pragma unroll
      for (int q = 0; q < EBATCH; q++) cur[q] = nxt[q];
    }
    ZD_ADD(9, tz);
    if (lane == 0) {
      RingW bw{ring, pos};
      bw.put(eob & 0xffff, eob >> 16);
      pos = bw.pos;
    }
    pos = readlane64(pos, 0);
    // the last (partial) word is shared with the next block
    const uint64_t wend = (pos + 31) >> 5;
    for (uint64_t w = flushed + lane; w < wend; w += 64) {
      const uint32_t v = ring[w % RING];
      if (w == wfirst || w == wend - 1) or_word(o, w, v);
      else if (w < o.nwords) o.o[w] = v;
    }
    ZD_ADD(10, tz);
  }
#ifdef XCG_ZD_TIMING
  if (lane == 0) atomicAdd(&g_zd_t[15], 1ull);
#endif
  if (k == r.nblocks - 1 && lane == 0 && !r.stop) {
    if (last) {   // Z_FINISH: adler32 trailer, big-endian (putShortMSB x2)
      uint64_t b = r.end_bit >> 3;
      uint32_t ad = s.adler;
      or_byte(ob, b, ad >> 24);
      or_byte(ob, b + 1, (ad >> 16) & 0xff);
      or_byte(ob, b + 2, (ad >> 8) & 0xff);
      or_byte(ob, b + 3, ad & 0xff);
    } else {      // Z_SYNC_FLUSH: empty stored block, 000 + align + 00 00 FF FF
      uint64_t b = (r.end_bit + 3 + 7) >> 3;
      or_byte(ob, b + 2, 0xff);
      or_byte(ob, b + 3, 0xff);
    }
  }
}

// ------------------------------------------------------------------- launches
void zd_launch_huff(const ZArgs& a, uint32_t bo, hipStream_t st) {
  // few blocks (one consume at a time): a wave per block, whose heap chains
  // then run without a second lane's diverging beside them; many: two per wave
  if (bo <= 64) hipLaunchKernelGGL(zd_trees_kernel<1>, dim3(bo), dim3(64), 0, st, a);
  else hipLaunchKernelGGL(zd_trees_kernel<TB_BATCH>, dim3((bo + TB_BATCH - 1) / TB_BATCH), dim3(64), 0, st, a);
  hipLaunchKernelGGL(zd_layout_kernel, dim3(a.n), dim3(64), 0, st, a);
  hipLaunchKernelGGL(zd_emit_kernel, dim3(bo), dim3(64), 0, st, a);
}

#ifdef XCG_ZD_TIMING
bool zd_huff_times(uint64_t* acc) { return zd_times_take(acc); }
#endif

}  // namespace zd
}  // namespace xcg
