// Memory ceiling of the headline kernel's access pattern (diagnostics): 4096
// waves, each streams one 64 KiB chunk in 2 KiB pieces (32 B per lane) and
// writes 2050-byte records (a 2-byte header + the 2 KiB body: an EXTRACT),
// with the next D pieces' loads in flight.  Variants: prefetch depth D,
// record stride 2050 (unaligned bodies) or 2048 (aligned), waves per SIMD.
// The occ_kernel variants run at the encoder's occupancy (4 waves per SIMD,
// its LDS per block) with the encoder's one-piece register prefetch, and
// differ in the access shape: HALF (lane l moves 32 B at 32 l: today's), COAL
// loads and / or stores (16 B at 16 l and at 1024 + 16 l), and RING (the
// entering bytes go global -> LDS two pieces ahead, lane l reads its 32 B
// back from a linear image; waits counted by hand).
// Build: hipcc --offload-arch=gfx950 -O3 -o copy_pattern copy_pattern.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 __attribute__((aligned(1))) u32x4_u;
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;

template <int D, int STRIDE, int WORK>
__global__ __launch_bounds__(256) void copy_kernel(const uint8_t* in, uint8_t* out, uint32_t n) {
  const uint32_t wv = threadIdx.x >> 6, l = threadIdx.x & 63;
  const uint32_t chunk = blockIdx.x * 4 + wv;
  if (chunk >= n) return;
  const uint8_t* x = in + (uint64_t)chunk * 65536;
  uint8_t* o = out + (uint64_t)chunk * (32 * STRIDE + 16);
  u32x4 buf[D + 1][2];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    buf[k][0] = *(const u32x4*)(x + 2048 * k + 32 * l);
    buf[k][1] = *(const u32x4*)(x + 2048 * k + 32 * l + 16);
  }
  uint32_t acc = 0;
#pragma unroll
  for (int pc = 0; pc < 32; ++pc) {
    if (pc + D < 32) {
      buf[(pc + D) % (D + 1)][0] = *(const u32x4*)(x + 2048 * (pc + D) + 32 * l);
      buf[(pc + D) % (D + 1)][1] = *(const u32x4*)(x + 2048 * (pc + D) + 32 * l + 16);
    }
    const u32x4 a = buf[pc % (D + 1)][0], b = buf[pc % (D + 1)][1];
    // stand-in compute: WORK dependent VALU ops per piece
#pragma unroll
    for (int w = 0; w < WORK; ++w) acc = acc * 3u + (a[w & 3] ^ b[(w >> 2) & 3]);
    uint8_t* dst = o + (uint64_t)pc * STRIDE;
    if (l < 2) dst[l] = (uint8_t)(0xF1 + l + (acc & 1));
    *(u32x4_u*)(dst + 2 + 32 * l) = a;
    *(u32x4_u*)(dst + 2 + 32 * l + 16) = b;
  }
}

constexpr int OCC_LDS = 36736;   // the encoder's LDS per block
enum { HALF = 0, COAL = 1, COAL_LD = 2, COAL_ST = 3, RING = 4 };

// Two 16-byte LDS-DMA loads: lane l's 16 B at src and at src + 1024 land at
// lds_dst + 16 l and lds_dst + 1024 + 16 l (the offset applies to both sides).
__device__ __forceinline__ void glds_piece(const uint8_t* src, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off nt\n\t"
      "global_load_lds_dwordx4 %1, off offset:1024 nt\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(src), "s"(lds_dst)
      : "memory");
}

template <int MODE, int WORK>
__global__ __launch_bounds__(256, 4) void occ_kernel(const uint8_t* in, uint8_t* out, uint32_t n) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[OCC_LDS];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;
  const uint32_t chunk = blockIdx.x * 4 + wv;
  if (n == ~0u) ((volatile uint8_t*)lds)[OCC_LDS - 1 - threadIdx.x] = 1;   // (keeps the whole array allocated)
  if (chunk >= n) return;
  const uint8_t* x = in + (uint64_t)chunk * 65536;
  uint8_t* o = out + (uint64_t)chunk * (32 * 2050 + 16);
  constexpr bool CL = MODE == COAL || MODE == COAL_LD, CS = MODE == COAL || MODE == COAL_ST;
  const uint32_t l0 = CL ? 16 * l : 32 * l, l1 = CL ? 1024 + 16 * l : 32 * l + 16;
  const uint32_t s0 = CS ? 16 * l : 32 * l, s1 = CS ? 1024 + 16 * l : 32 * l + 16;
  uint8_t* ring = lds + 4096 * wv;
  const auto* ring3 = (const __attribute__((address_space(3))) uint8_t*)ring;
  const uint32_t ring_a = (uint32_t)(uintptr_t)ring3;
  u32x4 na = {0u, 0u, 0u, 0u}, nb = na;
  if (MODE == RING) {
    glds_piece(x + 16 * l, ring_a);
    glds_piece(x + 2048 + 16 * l, ring_a + 2048);
  } else {
    na = *(const u32x4*)(x + l0);
    nb = *(const u32x4*)(x + l1);
  }
  uint32_t acc = 0;
#pragma unroll
  for (int pc = 0; pc < 32; ++pc) {
    u32x4 a, b;
    if (MODE == RING) {
      // younger than this piece's two loads: the previous two pieces' three
      // stores each and the next piece's two loads
      if (pc >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      a = *(const volatile lds_u32x4*)(ring3 + 2048 * (pc & 1) + 32 * l);
      b = *(const volatile lds_u32x4*)(ring3 + 2048 * (pc & 1) + 32 * l + 16);
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b)::"memory");
      if (pc + 2 < 32) glds_piece(x + 2048 * (pc + 2) + 16 * l, ring_a + 2048 * (pc & 1));
    } else {
      a = na; b = nb;
      if (pc + 1 < 32) {
        na = *(const u32x4*)(x + 2048 * (pc + 1) + l0);
        nb = *(const u32x4*)(x + 2048 * (pc + 1) + l1);
      }
    }
#pragma unroll
    for (int w = 0; w < WORK; ++w) acc = acc * 3u + (a[w & 3] ^ b[(w >> 2) & 3]);
    uint8_t* dst = o + (uint64_t)pc * 2050;
    if (l < 2) dst[l] = (uint8_t)(0xF1 + l + (acc & 1));
    *(u32x4_u*)(dst + 2 + s0) = a;
    *(u32x4_u*)(dst + 2 + s1) = b;
  }
}

template <typename K>
static void time_it(const char* name, K launch, uint32_t n) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  for (int i = 0; i < 3; ++i) launch();
  hipEventRecord(e0, 0);
  const int R = 20;
  for (int i = 0; i < R; ++i) launch();
  hipEventRecord(e1, 0);
  hipEventSynchronize(e1);
  float ms = 0;
  hipEventElapsedTime(&ms, e0, e1);
  const double us = ms * 1e3 / R;
  const double bytes = (double)n * 65536 * 2;
  printf("%-34s %7.1f us per launch  %6.2f TB/s (in + out)\n", name, us, bytes / us / 1e6);
  hipEventDestroy(e0);
  hipEventDestroy(e1);
}

template <int MODE, int WORK>
static void run_occ(const char* name, const uint8_t* in, uint8_t* out, uint32_t n) {
  char full[64];
  snprintf(full, sizeof full, "occ4 %-8s work %d", name, WORK);
  time_it(full, [&] { hipLaunchKernelGGL((occ_kernel<MODE, WORK>), dim3(n / 4), dim3(256), 0, 0, in, out, n); }, n);
}
template <int WORK>
static void run_occ_all(const uint8_t* in, uint8_t* out, uint32_t n) {
  run_occ<HALF, WORK>("half", in, out, n);
  run_occ<COAL, WORK>("coal", in, out, n);
  run_occ<COAL_LD, WORK>("coal-ld", in, out, n);
  run_occ<COAL_ST, WORK>("coal-st", in, out, n);
  run_occ<RING, WORK>("ring", in, out, n);
}

template <int D, int STRIDE, int WORK>
static void run(const char* name, const uint8_t* in, uint8_t* out, uint32_t n) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  for (int i = 0; i < 3; ++i) hipLaunchKernelGGL((copy_kernel<D, STRIDE, WORK>), dim3(n / 4), dim3(256), 0, 0, in, out, n);
  hipEventRecord(e0, 0);
  const int R = 20;
  for (int i = 0; i < R; ++i) hipLaunchKernelGGL((copy_kernel<D, STRIDE, WORK>), dim3(n / 4), dim3(256), 0, 0, in, out, n);
  hipEventRecord(e1, 0);
  hipEventSynchronize(e1);
  float ms = 0;
  hipEventElapsedTime(&ms, e0, e1);
  const double us = ms * 1e3 / R;
  const double bytes = (double)n * 65536 * 2;
  printf("%-34s %7.1f us per launch  %6.2f TB/s (in + out)\n", name, us, bytes / us / 1e6);
}

int main() {
  const uint32_t n = 4096;
  uint8_t *in = nullptr, *out = nullptr;
  if (hipMalloc(&in, (size_t)n * 65536) != hipSuccess || hipMalloc(&out, (size_t)n * (32 * 2050 + 16)) != hipSuccess) {
    printf("alloc failed\n");
    return 1;
  }
  hipMemset(in, 7, (size_t)n * 65536);
  run<1, 2050, 0>("D=1 stride 2050 work 0", in, out, n);
  run<2, 2050, 0>("D=2 stride 2050 work 0", in, out, n);
  run<4, 2050, 0>("D=4 stride 2050 work 0", in, out, n);
  run<1, 2048, 0>("D=1 stride 2048 work 0", in, out, n);
  run<4, 2048, 0>("D=4 stride 2048 work 0", in, out, n);
  run<1, 2050, 64>("D=1 stride 2050 work 64", in, out, n);
  run<2, 2050, 64>("D=2 stride 2050 work 64", in, out, n);
  run<4, 2050, 64>("D=4 stride 2050 work 64", in, out, n);
  run<1, 2050, 200>("D=1 stride 2050 work 200", in, out, n);
  run<2, 2050, 200>("D=2 stride 2050 work 200", in, out, n);
  run<4, 2050, 200>("D=4 stride 2050 work 200", in, out, n);
  run_occ_all<0>(in, out, n);
  run_occ_all<200>(in, out, n);
  run_occ_all<360>(in, out, n);
  if (hipDeviceSynchronize() != hipSuccess) {
    printf("a launch failed\n");
    return 1;
  }
  hipFree(in);
  hipFree(out);
  return 0;
}
