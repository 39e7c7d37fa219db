// The deflate stage's format constants and the plain-data records its host
// plan (xcg_zdeflate_plan.h) and its kernels (xcg_zdeflate.h and the
// xcg_zdeflate*.hip units) share.  No HIP here: oracle/zdeflate_plan_harness.cc
// compiles it with g++.
#pragma once
#include <stdint.h>

namespace xcg {
namespace zd {

constexpr int WSIZE = 32768;
constexpr int WINSZ = 65536;
constexpr int MIN_MATCH = 3;
constexpr int MAX_MATCH = 258;
constexpr int MIN_LOOKAHEAD = MAX_MATCH + MIN_MATCH + 1;   // 262
constexpr int MAX_DIST = WSIZE - MIN_LOOKAHEAD;            // 32506
constexpr int TOO_FAR = 4096;
constexpr uint32_t SYMS_PER_BLOCK = 16383;                 // lit_bufsize - 1
constexpr int L_CODES = 286, D_CODES = 30, BL_CODES = 19, HEAP_SIZE = 2 * L_CODES + 1;
constexpr int MAX_BITS = 15;
constexpr int XPAD = 272;                                  // zeroed bytes after a call's data in X
constexpr int TAB_WORDS = L_CODES + D_CODES + BL_CODES;    // per block: code | len << 16
constexpr int DMAX = 264;            // >= MIN_LOOKAHEAD - 1: positions a stopped flush call can leave
constexpr uint32_t PIPE_CHUNK = 65536;   // DeflatePipe's output buffer (DEFLATE_CHUNK_SIZE, deflate_pipe.cc:34)
// The most bytes one consume() may bring: of xcg_zdeflate_batch (check_calls, xcg_zdeflate_plan.h), and of the
// receiving stage's xcg_zinflate_batch (xcg_inflate.hip).  Callers that refuse up front (xcg_codec.cpp) read these.
constexpr uint32_t MAX_CALL_LEN = 1u << 24;
constexpr uint32_t INFLATE_MAX_CALL_LEN = 1u << 26;

struct ZState {          // one DeflatePipe's z_stream, reduced to what the output depends on
  uint64_t total;        // bytes consumed
  uint64_t base;         // stream position of zlib's window coord 0 (slides by WSIZE)
  uint32_t adler;        // adler32 of everything consumed (the Z_FINISH trailer)
  uint32_t flags;        // 1: header written, 2: finished (Z_STREAM_END)
  // What a flush call that stopped at a full pipe buffer leaves (see zd_layout_kernel):
  uint64_t pend;         // bytes produced but not delivered yet (zlib's pending past the buffer)
  uint64_t block_start;  // stream position of the open block's start
  uint64_t mstart;       // match_start (stream position)
  uint32_t dlen;         // positions before `total` not parsed yet (strstart = total - dlen)
  uint32_t avail, mlen;  // deflate_slow's match_available, match_length at strstart
  uint32_t cbits, cnb;   // the last incomplete output byte: its cnb < 8 low bits
  uint32_t pad;
};

struct ZCall {           // host-built, one per consume()
  uint64_t in_off, out_off;   // into d_in / d_out (out_off % 4 == 0)
  uint64_t x_off;             // X (and d16 at 2 * x_off) in the scratch
  uint64_t t_off;             // tf / tq / sym: call-relative position 0
  uint32_t len, stream;
  uint32_t blk_off, blk_cap;  // block records
  uint64_t m_off;             // deflate_fast: the call's hashed-position masks (words; bit j = X index j)
};

struct ZBlock {
  uint32_t sym_begin, sym_end;
  uint32_t start;        // X index of block_start
  uint32_t stored_len;
  uint32_t flags;        // 1 storable (block_start not slid out), 2 last, 4 flushed in the flush call
                         // (a loop top with lookahead < MIN_LOOKAHEAD, or the call's final flush)
  uint32_t type;         // 0 stored, 1 static, 2 dynamic
  uint32_t lcodes, dcodes, blcodes, pad;
  uint64_t bits;         // Huffman blocks: 3 + trees + symbols + end-of-block
  uint64_t bit_off;      // start of the block in the call's output
  // the parse state right after this flush (where a stopped flush call resumes)
  int64_t bidx;          // X index of window coord 0
  uint32_t p_after, ms;  // X indices: strstart, match_start
  uint32_t avail, ml;
};

struct ZCallRes {
  uint32_t nblocks;      // blocks emitted (a stopped flush call drops the ones after the stop)
  uint32_t nsym;
  uint64_t base_end;     // stream position of coord 0 after the call
  uint32_t adler;        // adler32 after the call
  uint32_t out_len;      // output bytes the emit may touch (incl. a stop's incomplete last byte)
  uint64_t end_bit;      // bit offset after the last emitted block
  uint32_t stop;         // 0 none, else 1 + the block the flush call stopped at
  uint32_t out_bytes;    // complete new bytes (what the caller appends to the undelivered ones)
  uint64_t deliver;      // bytes DeflatePipe::consume produces now
  uint32_t scan_end;     // X index the parse reached (all positions, unless stopped)
  uint32_t pad;
};

struct ZArgs {
  const ZCall* calls;
  ZState* st;
  uint8_t* hist;         // nstreams x WSIZE
  const uint8_t* in;
  uint8_t* out;
  uint8_t* X;
  uint16_t* d16;
  uint32_t* pk;          // packed hashes (zd_hashes_kernel), indexed like X
  uint32_t* tf;
  uint32_t* tq;
  uint32_t* sym;
  ZBlock* blk;
  uint32_t* tabs;        // blk index * TAB_WORDS
  ZCallRes* res;
  uint32_t* out_len;     // caller's d_out_len
  uint64_t* deliver;     // caller's d_deliver
  uint32_t n;                  // calls
  const uint32_t* mstart;      // first 256-position match tile of each call (n + 1, prefix)
  const uint32_t* gstart;      // first 64-position hash group of each call (n + 1, prefix)
  const uint32_t* bstart;      // first block record of each call (n + 1, prefix)
  int level;
  // deflate_fast (levels 1-3): which positions zlib hashes depends on its parse.
  // mcur: this round's guess (X index >= strstart; earlier ones from `ring`),
  // mnext: the positions the round's parse hashes, ring: per stream, bit
  // (position mod 32768) of the last 32 KiB, changed: per call, mnext != mcur.
  int fast;
  uint32_t* mcur;
  uint32_t* mnext;
  uint32_t* ring;
  uint32_t* changed;
};

}  // namespace zd
}  // namespace xcg
