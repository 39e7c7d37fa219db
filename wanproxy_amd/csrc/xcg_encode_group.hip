// XCodec encoder, grouped batches: the chunks of a group, in order, are
// successive XCodecEncoder::encode calls (xcodec/xcodec_encoder.cc:74-274) of one
// encoder on a fresh, empty XCodecMemoryCache made for that group
// (xcodec_cache.h:303-365) -- a short stream.  One wave per group runs
// encode_chunk (xcg_encode_wave.h, GROUP) on each of its chunks against one
// table that is cleared once and carried from call to call; nothing crosses
// groups, nothing of a context is read or written.
#include "xcg_encode_wave.h"

namespace xcg {

// The launch geometry is the independent unit's (INDEP_W, INDEP_OCC, INDEP_LOGNB,
// xcg_encode_wave.h): four group-waves per workgroup, four workgroups per CU in
// the small class, the same key table.
// A lane's share of its group's lengths is clamped to this before the wave adds
// the 64 shares up in 32 bits: above every max_group_len, and 64 of them are 2^31.
constexpr uint32_t LEN_CLAMP = 1u << 25;
static_assert(LEN_CLAMP > (1u << 19) && 64ull * LEN_CLAMP <= 0xFFFFFFFFull, "the clamped sum must not wrap");

// The independent unit's LDS (key tables first, at offset 0) and, per wave, the
// high bits of its records' input offsets (GroupCarry::rch; 16 bits each, so
// that two workgroups of the large class still share a CU's LDS).
template <int LOGNB, int MAXD, int W>
struct GroupLDS {
  IndepLDS<LOGNB, MAXD, W> S;
  uint16_t rch[W][MAXD];
};

template <int LOGNB, int MAXD>
__global__ __launch_bounds__(64 * INDEP_W, INDEP_OCC) void encode_group_kernel(EncParams prm,
                                                                               const uint32_t* group_first,
                                                                               uint32_t n_groups) {
  __shared__ GroupLDS<LOGNB, MAXD, INDEP_W> G;
  static_assert(MAXD > 72 || INDEP_OCC * sizeof(G) <= 160u * 1024u, "the workgroups of a CU share 160 KiB of LDS");
  constexpr bool DM = MAXD <= 72;
  const int wv = (int)readfirst(threadIdx.x >> 6);   // wave-uniform: keeps the parse state in SGPRs
  const uint32_t g = blockIdx.x * (uint32_t)INDEP_W + (uint32_t)wv;
  if (g >= n_groups) return;
  const uint32_t l = (uint32_t)lane_id();
  const uint32_t ca = readfirst(group_first[g]), cb = readfirst(group_first[g + 1]);
  // A group whose bounds do not ascend within [0, n] has no chunks to name: refused, nothing written.
  if (ca > cb || cb > prm.n) {
    if (l == 0 && prm.status) atomicOr(prm.status, 8);
    return;
  }
  if (ca == cb) return;
  // A group longer than the launch's bound would overrun the records sized for
  // it (a group of T bytes declares at most T / 2048 segments): refused as a
  // whole, loudly (status bit 3), never parsed.  (per-lane sums clamped to
  // 2^25: the bound is below that, and 64 clamped terms sum to at most 2^31)
  uint64_t tl = 0;
  for (uint32_t c = ca + l; c < cb; c += 64u) tl += prm.chunk_len[c];
  const uint32_t tot = readfirst(wave_sum((uint32_t)min(tl, (uint64_t)LEN_CLAMP)));
  if (tot > prm.max_len || tot / SEG >= (uint32_t)MAXD) {
    for (uint32_t c = ca + l; c < cb; c += 64u) prm.out_len[c] = 0;
    if (l == 0 && prm.status) atomicOr(prm.status, 8);
    return;
  }
  const uint32_t kofs = (uint32_t)wv << (LOGNB + 3);
  uint32_t* const keyt = (uint32_t*)((char*)G.S.key + kofs);
  for (uint32_t k = l; k < (2u << LOGNB); k += 64u) keyt[k] = DM ? dm_empty<LOGNB>(k) : kempty<LOGNB>(k >> 1);
  __builtin_amdgcn_wave_barrier();
  GroupCarry gc{0u, 0u, G.rch[wv], 0, (int)tot};
  for (uint32_t c = ca; c < cb; ++c) {
    encode_chunk<LOGNB, MAXD, false, false, true>(prm, (char*)G.S.key, kofs, G.S.rec[wv], c,
                                                  GlbView{nullptr, 0u, 0u, 0, nullptr, nullptr}, G.S.ring_of(wv), &gc);
    gc.done += (int)readfirst(prm.chunk_len[c]);
  }
}

template __global__ void encode_group_kernel<INDEP_LOGNB, 72>(EncParams, const uint32_t*, uint32_t);
template __global__ void encode_group_kernel<11, 264>(EncParams, const uint32_t*, uint32_t);

}  // namespace xcg

extern "C" int xcg_launch_encode_group(const uint8_t* d_in, const uint64_t* d_chunk_off, const uint32_t* d_chunk_len,
                                       uint32_t n, const uint32_t* d_group_first, uint32_t n_groups,
                                       uint32_t max_group_len, uint32_t flags, uint8_t* d_out,
                                       const uint64_t* d_out_off, uint64_t* d_out_len, uint32_t* d_stats,
                                       int32_t* d_status, hipStream_t stream) {
  using namespace xcg;
  if (n == 0 || n_groups == 0) return 0;
  EncParams prm{d_in, d_chunk_off, d_chunk_len, n, flags, d_out, d_out_off, d_out_len, d_stats, d_status};
  prm.max_len = max_group_len;
  dim3 grid((n_groups + INDEP_W - 1) / INDEP_W), block(64 * INDEP_W);
  if (max_group_len <= (1u << 17)) {
    hipLaunchKernelGGL((encode_group_kernel<INDEP_LOGNB, 72>), grid, block, 0, stream, prm, d_group_first, n_groups);
  } else if (max_group_len <= (1u << 19)) {
    hipLaunchKernelGGL((encode_group_kernel<11, 264>), grid, block, 0, stream, prm, d_group_first, n_groups);
  } else {
    return XCG_RC_INVAL;
  }
  return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}
