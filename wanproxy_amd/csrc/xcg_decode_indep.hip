// XCodec decoder, independent semantics, MI355X (gfx950): the inverse of
// encode_independent_kernel.  Chunk i is one XCodecDecoder::decode(output,
// input, unknown) call (xcodec/xcodec_decoder.cc:66-188) on a decoder made for
// that chunk alone -- an empty XCodecMemoryCache, an empty XCodecWindow -- so
// nothing crosses chunks and nothing of the context is read or written.
//
// One wave64 per chunk, four waves per workgroup, ONE pass that writes as it
// walks: a chunk's output offset is a running sum, so there is no size scan, no
// batch table in HBM, no commit and no host readback.  Per wave, in LDS:
//   X   the chunk's cache: hash -> offset of the EXTRACT payload in the chunk's
//       own input (open addressing, probed 64 slots at a time).  A later EXTRACT
//       of a hash overwrites the offset: cache_->replace, or the same bytes
//       (:106-136).  A chunk of L bytes holds at most L / 2050 EXTRACTs and the
//       table has more than twice as many slots, so it cannot fill.
//   W   the decoder's XCodecWindow (xcodec/xcodec_window.h:68-111): 256 slots of
//       (hash, source offset) and the cursor.  A slot keeps the offset its
//       declare saw, as the reference's slot keeps that BufferSegment.
// Output goes to the caller's slot; from the first piece that would pass its
// capacity on nothing is stored, and the walk goes on counting (status 4).
#include "xcg_cache.h"
#include "xcg_args.h"
#include "xcg_decode_ops.h"

namespace xcg {

constexpr uint32_t NO_SRC = ~0u;   // an empty table / window slot (never an offset: chunks are <= 1 MiB + 16)

// The chunk's decoder in LDS (xcg_decode_ops.h), its sources chunk-local offsets.
template <int XSLOTS>
using IndepDecWave = DecWave<XSLOTS, uint32_t>;

template <int XSLOTS>
__global__ __launch_bounds__(256) void decode_independent_kernel(XcgIndepDecodeArgs prm) {
  __shared__ IndepDecWave<XSLOTS> lds[4];
  const int wv = (int)readfirst(threadIdx.x >> 6);
  const uint32_t chunk = blockIdx.x * 4u + (uint32_t)wv;
  if (chunk >= prm.n) return;
  const uint32_t l = (uint32_t)lane_id();
  IndepDecWave<XSLOTS>& S = lds[wv];
  const uint8_t* x = prm.in + prm.chunk_off[chunk];
  const uint32_t len = prm.chunk_len[chunk];
  uint8_t* out = prm.out + prm.out_off[chunk];
  const uint64_t cap = prm.out_cap[chunk];
  // A chunk longer than the launch's bound could fill X: refused loudly
  // (status bit 3, as the independent encode does), never walked.
  if (len > prm.max_len || len / (2u + SEG) >= (uint32_t)XSLOTS / 2u) {
    if (l == 0) {
      prm.out_len[chunk] = 0;
      prm.chunk_status[chunk] = -1;
      prm.consumed[chunk] = 0;
      if (prm.first_unknown) prm.first_unknown[chunk] = 0;
      atomicOr(prm.status, 8);
    }
    return;
  }
  for (uint32_t k = l; k < (uint32_t)XSLOTS; k += 64) S.xv[k] = NO_SRC;
  for (uint32_t k = l; k < 256u; k += 64) S.ws[k] = NO_SRC;
  lds_wave_sync();

  uint64_t olen = 0, unk = 0;
  int32_t st = 0;
  uint32_t i = 0, cursor = 0;
  bool full = false;                                         // a piece did not fit: nothing more is stored
  bool at_op = false;                                        // op_at(x, i, len), asked before the last stores
  while (i < len) {
    if (!at_op) {
      uint32_t nesc = 0;
      const uint32_t m = next_op(x, i, len, nesc);
      if (m > i) {                                           // literal run with nesc ESCAPE pairs (:71-81, :91-94)
        const uint32_t nlit = (m - i) - nesc;
        if (!full && olen + nlit <= cap) (void)wave_unescape(out + olen, x, i, m);
        else full = true;
        olen += nlit;
      }
      i = m;
      if (i >= len) break;
    }
    at_op = false;
    if (len - i == 1) { st = 3; break; }                     // :85-86 need the op byte
    const uint32_t op = readfirst(x[i + 1]);
    const uint8_t* src = nullptr;
    if (op == OP_EXTRACT) {                                  // :96-141
      if (len - i < 2u + SEG) { st = 3; break; }
      const uint2 hh = dec_window_hash(x + i + 2);
      const uint64_t h = ((uint64_t)readfirst(hh.y) << 32) | readfirst(hh.x);
      uint32_t slot;
      (void)xtab_find(S, h, slot);
      if (l == 0) {                                          // enter, or replace / the same bytes again
        S.xk[slot] = h;
        S.xv[slot] = i + 2;
      }
      win_declare(S, cursor, h, i + 2);                      // (syncs the table write too)
      src = x + i + 2;
      i += 2 + SEG;
    } else if (op == OP_REF) {                               // :143-163
      if (len - i < 10u) { st = 3; break; }
      const uint64_t h = readfirst64(be64(x + i + 2));
      uint32_t slot;
      const uint32_t so = xtab_find(S, h, slot);
      if (so == NO_SRC) { st = 1; unk = h; break; }          // :151-156: decode() returns true, the REF stays
      win_declare(S, cursor, h, so);
      src = x + so;
      i += 10;
    } else if (op == OP_BACKREF) {                           // :165-181
      if (len - i < 3u) { st = 3; break; }
      const uint32_t c = readfirst(x[i + 2]);
      i += 3;                                                // moveout precedes the check
      const uint32_t so = readfirst(S.ws[c]);
      if (so == NO_SRC) { st = -1; break; }
      src = x + so;
    } else {
      st = -1;                                               // :182-184 unsupported opcode
      break;
    }
    // the segment's loads and the look at the next op first, then the stores
    const bool fits = !full && olen + SEG <= cap;
    u32x4 v0 = {0u, 0u, 0u, 0u}, v1 = v0;
    if (fits) {
      v0 = *(const u32x4_u*)(src + 32 * l);
      v1 = *(const u32x4_u*)(src + 32 * l + 16);
    } else {
      full = true;
    }
    at_op = op_at(x, i, len);
    if (fits) {
      *(u32x4_u*)(out + olen + 32 * l) = v0;
      *(u32x4_u*)(out + olen + 32 * l + 16) = v1;
    }
    olen += SEG;
  }
  if (l == 0) {
    prm.out_len[chunk] = olen;
    prm.chunk_status[chunk] = full ? 4 : st;
    prm.consumed[chunk] = i;
    if (prm.first_unknown) prm.first_unknown[chunk] = unk;
  }
}

}  // namespace xcg

// EXTRACTs a chunk of the class can hold < half the class's table slots.
constexpr uint32_t XCG_INDEP_DEC_SMALL = 2u * 65536u + 16u;      // xcg_encode_bound(64 KiB): 63 EXTRACTs, 128 slots
constexpr uint32_t XCG_INDEP_DEC_LARGE = 2u * 524288u + 16u;     // xcg_encode_bound(512 KiB): 511 EXTRACTs, 1024 slots
static_assert(XCG_INDEP_DEC_SMALL / 2050u < 128u / 2u && XCG_INDEP_DEC_LARGE / 2050u < 1024u / 2u,
              "the per-wave EXTRACT table must stay under half full");

extern "C" int xcg_launch_decode_independent(const XcgIndepDecodeArgs* a, hipStream_t stream) {
  if (a->n == 0) return 0;
  dim3 grid((a->n + 3) / 4), block(256);
  if (a->max_len <= XCG_INDEP_DEC_SMALL) {
    hipLaunchKernelGGL((xcg::decode_independent_kernel<128>), grid, block, 0, stream, *a);
  } else if (a->max_len <= XCG_INDEP_DEC_LARGE) {
    hipLaunchKernelGGL((xcg::decode_independent_kernel<1024>), grid, block, 0, stream, *a);
  } else {
    return XCG_RC_INVAL;
  }
  return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}
