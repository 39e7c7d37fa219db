// XCodec decoder, grouped semantics, MI355X (gfx950): the inverse of
// encode_group_kernel.  The chunks of a group, in order, are successive
// XCodecDecoder::decode(output, input, unknown) calls (xcodec/xcodec_decoder.cc:
// 66-188) on ONE decoder made for that group -- an empty XCodecMemoryCache, an
// empty XCodecWindow -- so the cache (name reuse, :106-136), the window's slots
// and its cursor live from one chunk of the group to the next, nothing crosses
// groups and nothing of the context is read or written.
//
// decode_independent_kernel's design (xcg_decode_indep.hip) with one wave64 per
// group: X and W are initialised once, the walk is repeated per chunk, and the
// X values and W sources are byte offsets into the whole batch input instead of
// chunk-local ones, so a BACKREF or REF of chunk 3 reads a payload that lies in
// chunk 0's bytes, wherever the caller put that chunk.
//
// The stream rule: the group stops at the first chunk whose own status (what a
// call with room would report) is not 0; the chunks after it are not reached
// (status 2, as xcg_decode_batch reports past its blocking point).  A chunk
// that is only out of room (status 4) does not stop it: the walk went on
// counting and X and W evolved, and later chunks read their segments from the
// input, never from an output slot.
#include "xcg_cache.h"
#include "xcg_args.h"
#include "xcg_decode_ops.h"

namespace xcg {

constexpr uint32_t LEN_CLAMP = 1u << 25;   // a lane's share of its group's lengths, before the 32-bit wave sum
static_assert(LEN_CLAMP > 2u * (1u << 19) + 16u && 64ull * LEN_CLAMP <= 0xFFFFFFFFull, "the clamped sum must not wrap");
constexpr uint64_t NO_SRC64 = ~0ull;   // an empty table / window slot (never an offset into the input)

// The group's decoder in LDS (xcg_decode_ops.h), its sources offsets into the batch input.
template <int XSLOTS>
using GroupDecWave = DecWave<XSLOTS, uint64_t>;

template <int XSLOTS>
__global__ __launch_bounds__(256) void decode_group_kernel(XcgGroupDecodeArgs prm) {
  __shared__ GroupDecWave<XSLOTS> lds[4];
  const int wv = (int)readfirst(threadIdx.x >> 6);
  const uint32_t g = blockIdx.x * 4u + (uint32_t)wv;
  if (g >= prm.n_groups) return;
  const uint32_t l = (uint32_t)lane_id();
  GroupDecWave<XSLOTS>& S = lds[wv];
  const uint32_t ca = readfirst(prm.group_first[g]), cb = readfirst(prm.group_first[g + 1]);
  // A group whose bounds do not ascend within [0, n] has no chunks to name: refused, nothing written.
  if (ca > cb || cb > prm.n) {
    if (l == 0) atomicOr(prm.status, 8);
    return;
  }
  // Pre-pass over the group's lengths, before anything is written: a group
  // longer than the launch's bound could fill X.  (per-lane sums clamped to
  // 2^25 and 2^20: above every bound, and 64 clamped terms sum to at most 2^31)
  uint64_t tl = 0, te = 0;
  for (uint32_t c = ca + l; c < cb; c += 64u) {
    const uint32_t len = prm.chunk_len[c];
    tl += len;
    te += len / (2u + SEG);
  }
  const uint32_t tot = wave_sum((uint32_t)min(tl, (uint64_t)LEN_CLAMP));
  const uint32_t ext = wave_sum((uint32_t)min(te, (uint64_t)1u << 20));
  if (tot > prm.max_len || ext >= (uint32_t)XSLOTS / 2u) {
    for (uint32_t c = ca + l; c < cb; c += 64u) {
      prm.out_len[c] = 0;
      prm.chunk_status[c] = -1;
      prm.consumed[c] = 0;
      if (prm.first_unknown) prm.first_unknown[c] = 0;
    }
    if (l == 0) atomicOr(prm.status, 8);
    return;
  }
  for (uint32_t k = l; k < (uint32_t)XSLOTS; k += 64) S.xv[k] = NO_SRC64;
  for (uint32_t k = l; k < 256u; k += 64) S.ws[k] = NO_SRC64;
  lds_wave_sync();

  uint32_t cursor = 0;
  uint32_t c = ca;
  for (; c < cb; ++c) {
    const uint64_t xo = prm.chunk_off[c];
    const uint8_t* x = prm.in + xo;
    const uint32_t len = prm.chunk_len[c];
    uint8_t* out = prm.out + prm.out_off[c];
    const uint64_t cap = prm.out_cap[c];
    uint64_t olen = 0, unk = 0;
    int32_t st = 0;
    uint32_t i = 0;
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
        if (l == 0) {                                          // enter, or replace / the same bytes again (:106-136)
          S.xk[slot] = h;
          S.xv[slot] = xo + i + 2;
        }
        win_declare(S, cursor, h, xo + i + 2);                // (syncs the table write too)
        src = x + i + 2;
        i += 2 + SEG;
      } else if (op == OP_REF) {                               // :143-163
        if (len - i < 10u) { st = 3; break; }
        const uint64_t h = readfirst64(be64(x + i + 2));
        uint32_t slot;
        const uint64_t so = xtab_find(S, h, slot);
        if (so == NO_SRC64) { st = 1; unk = h; break; }        // :151-156: decode() returns true, the REF stays
        win_declare(S, cursor, h, so);
        src = prm.in + so;
        i += 10;
      } else if (op == OP_BACKREF) {                           // :165-181
        if (len - i < 3u) { st = 3; break; }
        const uint32_t b = readfirst(x[i + 2]);
        i += 3;                                                // moveout precedes the check
        const uint64_t so = readfirst64(S.ws[b]);
        if (so == NO_SRC64) { st = -1; break; }
        src = prm.in + so;
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
      prm.out_len[c] = olen;
      prm.chunk_status[c] = full ? 4 : st;
      prm.consumed[c] = i;
      if (prm.first_unknown) prm.first_unknown[c] = unk;
    }
    if (st != 0) { ++c; break; }                               // the stream stops here, with or without room
  }
  for (c += l; c < cb; c += 64u) {                             // not reached
    prm.out_len[c] = 0;
    prm.chunk_status[c] = 2;
    prm.consumed[c] = 0;
    if (prm.first_unknown) prm.first_unknown[c] = 0;
  }
}

template __global__ void decode_group_kernel<128>(XcgGroupDecodeArgs);
template __global__ void decode_group_kernel<1024>(XcgGroupDecodeArgs);

}  // namespace xcg

// EXTRACTs a group of the class can hold < half the class's table slots.
constexpr uint32_t XCG_GROUP_DEC_SMALL = 2u * 65536u + 16u;      // xcg_encode_bound(64 KiB): 63 EXTRACTs, 128 slots
constexpr uint32_t XCG_GROUP_DEC_LARGE = 2u * 524288u + 16u;     // xcg_encode_bound(512 KiB): 511 EXTRACTs, 1024 slots
static_assert(XCG_GROUP_DEC_SMALL / 2050u < 128u / 2u && XCG_GROUP_DEC_LARGE / 2050u < 1024u / 2u,
              "the per-wave EXTRACT table must stay under half full");

extern "C" int xcg_launch_decode_group(const XcgGroupDecodeArgs* a, hipStream_t stream) {
  if (a->n == 0 || a->n_groups == 0) return 0;
  dim3 grid((a->n_groups + 3) / 4), block(256);
  if (a->max_len <= XCG_GROUP_DEC_SMALL) {
    hipLaunchKernelGGL((xcg::decode_group_kernel<128>), grid, block, 0, stream, *a);
  } else if (a->max_len <= XCG_GROUP_DEC_LARGE) {
    hipLaunchKernelGGL((xcg::decode_group_kernel<1024>), grid, block, 0, stream, *a);
  } else {
    return XCG_RC_INVAL;
  }
  return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}
