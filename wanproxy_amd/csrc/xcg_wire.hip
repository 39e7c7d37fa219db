// xcg_gather_pieces: copy n byte ranges ("pieces") from anywhere to anywhere,
// at any alignment.  The codec send path (xcg_codec.cpp) builds every pipe's
// wire with it -- host literals and the encoder's output slots, side by side
// -- in the deflate stage's input buffer, and packs the compressed slots for
// the copy to the host.
//
// One wave per (piece, tile).  A piece's first bytes up to the destination's
// next 16-byte boundary (the head, < 16) go out as single bytes; from there it
// is cut into tiles of TILE bytes, each moved with 16-byte stores to aligned
// addresses; the last tile's rest (< 16) goes out as single bytes again.  Every
// store lies inside the piece and nothing is read back and rewritten, so the
// waves that write the neighbouring pieces at the same time are not disturbed.
// The loads are 16-byte too: aligned when source and destination share their
// residue mod 16, else unaligned dwordx4 loads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xcg_args.h"
#include "xcg_device.h"

namespace xcg {

constexpr uint32_t GATHER_TILE = 8192;   // bytes a wave moves per step: 8 x (64 lanes x 16 bytes)

// Global-memory views of the source: its address is an integer sum, which the compiler would otherwise
// load through flat instructions.
typedef const __attribute__((address_space(1))) uint8_t gsrc8;
typedef const __attribute__((address_space(1))) u32x4 gsrc16;
typedef const __attribute__((address_space(1))) u32x4_u gsrc16_u;

__global__ __launch_bounds__(256) void gather_pieces_kernel(const uint8_t* src, const uint64_t* src_off,
                                                            const uint64_t* dst_off, const uint32_t* len,
                                                            uint8_t* dst) {
  const uint32_t piece = blockIdx.x;
  const uint32_t m = len[piece];
  if (m == 0) return;
  // (integer sums: a piece's source may lie in another allocation than `src`)
  gsrc8* s = (gsrc8*)((uintptr_t)src + (uintptr_t)src_off[piece]);
  uint8_t* d = dst + dst_off[piece];
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t wave = readfirst(threadIdx.x >> 6);
  uint32_t head = (16u - (uint32_t)((uintptr_t)d & 15u)) & 15u;
  if (head > m) head = m;
  const uint32_t body = m - head;                       // starts on a 16-byte boundary of the destination
  const bool same = (((uintptr_t)s ^ (uintptr_t)d) & 15u) == 0;
  const uint32_t first = blockIdx.y * 4u + wave;
  if (first == 0 && lane < head) d[lane] = s[lane];
  for (uint64_t t = first; t * GATHER_TILE < body; t += (uint64_t)gridDim.y * 4u) {
    const uint32_t b = head + (uint32_t)t * GATHER_TILE;
    const uint32_t e = body - (uint32_t)t * GATHER_TILE < GATHER_TILE ? m : b + GATHER_TILE;
    const uint32_t nv = (e - b) >> 4;
    if (same) {
      for (uint32_t i = lane; i < nv; i += 64) *(u32x4*)(d + b + 16u * i) = *(gsrc16*)(s + b + 16u * i);
    } else {
      for (uint32_t i = lane; i < nv; i += 64) *(u32x4*)(d + b + 16u * i) = *(gsrc16_u*)(s + b + 16u * i);
    }
    const uint32_t r = b + 16u * nv;                    // (the piece's last tile alone has a rest)
    if (r + lane < e) d[r + lane] = s[r + lane];
  }
}

}  // namespace xcg

extern "C" int xcg_launch_gather_pieces(const uint8_t* d_src, const uint64_t* d_src_off, const uint64_t* d_dst_off,
                                        const uint32_t* d_len, uint32_t n, uint32_t max_len, uint8_t* d_dst,
                                        hipStream_t stream) {
  using namespace xcg;
  if (n == 0) return 0;
  if (n > 0x7fffffffu) return XCG_RC_INVAL;
  // tiles of the longest piece, four to a workgroup (longer pieces than max_len are still copied whole: the
  // waves stride over a piece's tiles)
  uint32_t gy = (max_len / GATHER_TILE + 1 + 3) / 4;
  if (gy > 65535u) gy = 65535u;
  hipLaunchKernelGGL(gather_pieces_kernel, dim3(n, gy), dim3(256), 0, stream, d_src, d_src_off, d_dst_off, d_len,
                     d_dst);
  return hipGetLastError() == hipSuccess ? 0 : XCG_RC_HIP;
}
