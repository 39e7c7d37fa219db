// XCodec encoder, independent chunks: one wave per chunk runs encode_chunk
// (xcg_encode_wave.h) against a table of the chunk's own declarations; and the
// pack of its per-chunk output slots into one buffer.
#include "xcg_encode_wave.h"

namespace xcg {

template <int LOGNB, int MAXD>
__global__ __launch_bounds__(64 * INDEP_W, INDEP_OCC) void encode_independent_kernel(EncParams prm) {
  __shared__ IndepLDS<LOGNB, MAXD, INDEP_W> S;
  static_assert(MAXD > 72 || INDEP_OCC * sizeof(S) <= 160u * 1024u, "the workgroups of a CU share 160 KiB of LDS");
  const int wv = (int)readfirst(threadIdx.x >> 6);   // wave-uniform: keeps the parse state in SGPRs
  const uint32_t chunk = blockIdx.x * (uint32_t)INDEP_W + (uint32_t)wv;
  if (chunk >= prm.n) return;
  encode_chunk<LOGNB, MAXD, false>(prm, (char*)S.key, (uint32_t)wv << (LOGNB + 3), S.rec[wv], chunk,
                                   GlbView{nullptr, 0u, 0u, 0, nullptr, nullptr}, S.ring_of(wv));
}

template __global__ void encode_independent_kernel<INDEP_LOGNB, 72>(EncParams);
template __global__ void encode_independent_kernel<11, 264>(EncParams);

// Pack per-chunk output slots into one contiguous buffer (one wave per chunk).
__global__ __launch_bounds__(256) void pack_kernel(const uint8_t* src, const uint64_t* src_off, const uint64_t* len,
                                                   const uint64_t* dst_off, uint8_t* dst, uint32_t n) {
  const uint32_t c = blockIdx.x * 4u + (uint32_t)readfirst(threadIdx.x >> 6);
  if (c >= n) return;
  const uint8_t* s = src + src_off[c];
  uint8_t* d = dst + dst_off[c];
  const uint64_t m = len[c];
  const int l = lane_id();
  for (uint64_t base = 0; base < m; base += 1024) {
    const uint64_t off = base + 16u * l;
    if (off + 16 <= m) *(u32x4_u*)(d + off) = *(const u32x4_u*)(s + off);
    else for (uint64_t k = off; k < m; ++k) d[k] = s[k];
  }
}

}  // namespace xcg

// (the slots' offsets: the decoder's exclusive scan, xcg_decode.hip)
extern "C" int xcg_launch_pack(const uint8_t* src, const uint64_t* src_off, const uint64_t* len, uint32_t n,
                               uint8_t* dst, uint64_t* dst_off, uint64_t* d_total, hipStream_t stream) {
  using namespace xcg;
  if (n == 0) return 0;
  xcg_launch_exclusive_scan(len, dst_off, n, d_total, stream);
  hipLaunchKernelGGL(pack_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, src, src_off, len, (const uint64_t*)dst_off,
                     dst, n);
  return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}

extern "C" int xcg_launch_encode_independent(const uint8_t* d_in, const uint64_t* d_chunk_off,
                                             const uint32_t* d_chunk_len, uint32_t n, uint32_t max_chunk_len,
                                             uint32_t flags, uint8_t* d_out, const uint64_t* d_out_off,
                                             uint64_t* d_out_len, uint32_t* d_stats, int32_t* d_status,
                                             hipStream_t stream) {
  using namespace xcg;
  if (n == 0) return 0;
  EncParams prm{d_in, d_chunk_off, d_chunk_len, n, flags, d_out, d_out_off, d_out_len, d_stats, d_status};
  prm.max_len = max_chunk_len;
  dim3 grid((n + INDEP_W - 1) / INDEP_W), block(64 * INDEP_W);
  if (max_chunk_len <= (1u << 17)) {
    hipLaunchKernelGGL((encode_independent_kernel<INDEP_LOGNB, 72>), grid, block, 0, stream, prm);
  } else if (max_chunk_len <= (1u << 19)) {
    hipLaunchKernelGGL((encode_independent_kernel<11, 264>), grid, block, 0, stream, prm);
  } else {
    return XCG_RC_INVAL;
  }
  return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}
