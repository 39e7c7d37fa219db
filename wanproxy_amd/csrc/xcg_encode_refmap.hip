// XCodec encoder refmap, MI355X (gfx950): the third parameter of
// XCodecEncoder::encode(output, input, refmap) (xcodec/xcodec_encoder.h:42) --
// the map from every hash the call REF'd to its segment -- recovered from the
// call's output bytes.  find_reference emits a REF only on byte equality
// (xcodec_encoder.cc:382-390), so a REF's segment is the chunk's own input at
// the REF's input position, and (hash, position) is all a caller needs.
//
// One wave64 per chunk, four waves per workgroup, as decode_independent_kernel.
// The wave walks the encoding op by op with next_op (xcg_decode_ops.h) and
// tracks the input position: a literal run of k encoded bytes with e ESCAPE
// pairs is k - e input bytes, EXTRACT (F1 01 + 2048) and REF (F1 02 + BE64) are
// 2048 each.  Nothing is searched for inside an op's payload: an EXTRACT
// payload, a REF's hash bytes and the byte after an op may all hold F1, 00 or 02.
// The walk ends at the first thing no encoder writes -- a lone trailing F1, an
// op cut by the chunk's end, an opcode other than 00 / 01 / 02 (the encoder
// never emits BACKREF, :343-372) -- and what was found before it stands.
// Per wave, in LDS, the entries found so far:
//   - a REF whose (position, hash) is one of the chunk's out-of-band
//     declaration rows is no entry (encode_declaration passes no refmap,
//     :288-295; the rows are the stream batch's, XcgBatchScratch::decl);
//   - a hash is entered once, at its first REF (refmap->find(hash) == end(),
//     :364-371); the REF that would be entry 257 ends the walk;
//   - the entries leave in ascending unsigned hash order, std::map's iteration
//     order: each lane ranks its entries against all (they are distinct).
#include "../../include/xcgpu.h"   // XCG_REFMAP_MAX
#include "xcg_args.h"
#include "xcg_decode_ops.h"

namespace xcg {

constexpr uint32_t REFMAP_MAX = XCG_REFMAP_MAX;

struct RefWave {
  uint64_t h[REFMAP_MAX];
  uint32_t pos[REFMAP_MAX];
};

__global__ __launch_bounds__(256) void encode_refmap_kernel(XcgRefmapArgs prm) {
  __shared__ RefWave lds[4];
  const int wv = (int)readfirst(threadIdx.x >> 6);
  const uint32_t chunk = blockIdx.x * 4u + (uint32_t)wv;
  if (chunk >= prm.n) return;
  const uint32_t l = (uint32_t)lane_id();
  RefWave& S = lds[wv];
  const uint64_t len64 = prm.enc_len[chunk];
  // A chunk longer than the launch's bound is refused loudly (status bit 3, as
  // the independent decode does), never walked.
  if (len64 > (uint64_t)prm.max_len) {
    if (l == 0) {
      prm.ref_count[chunk] = 0;
      if (prm.walked) prm.walked[chunk] = 0;
      atomicOr(prm.status, 8);
    }
    return;
  }
  const uint8_t* x = prm.enc + prm.enc_off[chunk];
  const uint32_t len = (uint32_t)len64;
  const uint4* decl = prm.decl ? (const uint4*)prm.decl + (uint64_t)chunk * prm.maxd : nullptr;
  const uint32_t nd = decl ? min(readfirst(prm.ndecl[chunk]), prm.maxd) : 0u;

  uint32_t i = 0, pos = 0, cnt = 0;
  while (i < len) {
    uint32_t nesc = 0;
    const uint32_t m = next_op(x, i, len, nesc);
    pos += (m - i) - nesc;                                   // literal run with nesc ESCAPE pairs
    i = m;
    if (len - i < 2u) break;                                 // the end, or a lone trailing F1
    const uint32_t op = readfirst(x[i + 1]);
    if (op == OP_EXTRACT) {
      if (len - i < 2u + SEG) break;
      i += 2u + SEG;
    } else if (op == OP_REF) {
      if (len - i < 10u) break;
      if (prm.collect) {
        const uint64_t h = readfirst64(be64(x + i + 2));
        bool is_decl = false;                                // out of band: this F1 02 declares
        for (uint32_t d = 0; d < nd && !is_decl; d += 64) {
          bool eq = false;
          if (d + l < nd) {
            const uint4 r = decl[d + l];
            eq = r.z == pos && r.x == (uint32_t)h && r.y == (uint32_t)(h >> 32);
          }
          is_decl = ballot(eq) != 0;
        }
        if (!is_decl) {
          bool seen = false;
          for (uint32_t k = l; k < cnt; k += 64) seen |= S.h[k] == h;
          if (!ballot(seen)) {
            if (cnt == REFMAP_MAX) break;                    // entry 257: the walk ends at this REF
            if (l == 0) {
              S.h[cnt] = h;
              S.pos[cnt] = pos;
            }
            ++cnt;
            lds_wave_sync();
          }
        }
      }
      i += 10u;
    } else {
      break;                                                 // BACKREF or no opcode at all
    }
    pos += SEG;
  }

  const uint64_t base = (uint64_t)chunk * prm.ref_cap;
  for (uint32_t k = l; k < cnt; k += 64) {
    const uint64_t h = S.h[k];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < cnt; ++j) rank += S.h[j] < h ? 1u : 0u;
    if (rank < prm.ref_cap) {
      prm.ref_hash[base + rank] = h;
      prm.ref_pos[base + rank] = S.pos[k];
    }
  }
  if (l == 0) {
    prm.ref_count[chunk] = cnt;
    if (prm.walked) prm.walked[chunk] = i;
  }
}

}  // namespace xcg

extern "C" int xcg_launch_encode_refmap(const XcgRefmapArgs* a, hipStream_t stream) {
  if (a->n == 0) return 0;
  if (a->max_len > 2u * 524288u + 16u) return XCG_RC_INVAL;     // xcg_encode_bound(512 KiB)
  dim3 grid((a->n + 3) / 4), block(256);
  hipLaunchKernelGGL(xcg::encode_refmap_kernel, grid, block, 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}
