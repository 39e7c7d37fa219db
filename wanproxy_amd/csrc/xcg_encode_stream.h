// XCodec encoder, stream semantics: the parse kernel and the launch of its
// instances (the plain five: xcg_encode_stream.hip, with the round driver; the
// five that record cache references: xcg_encode_stream_lru.hip).
#pragma once
#include "xcg_encode_wave.h"

namespace xcg {

// Stream semantics: persistent workgroups of SW waves share one LDS copy of
// the lane filter; each wave walks chunks wave_id, wave_id + total_waves, ...
template <int LOGNB, int MAXD, int SW, bool LRU>
__global__ __launch_bounds__(64 * SW) void encode_stream_kernel(EncParams prm) {
  using L = StreamLDS<LOGNB, MAXD, SW>;
  __shared__ L S;
  // Which lane filter the cache + batch declarations fit: the 64 KiB LDS one
  // up to LDS_FILTER_KEYS keys (FP <~10 %), else the global one.
  const int wv = (int)readfirst(threadIdx.x >> 6);
  const uint32_t stride = gridDim.x * SW;
  const uint32_t items = prm.work ? readfirst(prm.work[0]) : prm.n;
  // Prefix slices of the round's LDS filter (xcg_cache.h PREFIX_FILTERS): the
  // slice that covers the workgroup's highest chunk holds every batch key its
  // chunks can see.  (The cache's and the batch's key counts pick the mode.)
  uint32_t slice = 0, bkeys = prm.use_b ? readfirst(wave_sum(prm.bcount[lane_id()])) : 0u;
  if (prm.lf.pfdiv) {
    uint32_t cmax = 0;
    for (uint32_t i = blockIdx.x * SW + (uint32_t)wv; i < items; i += stride)
      cmax = max(cmax, prm.work ? readfirst(prm.work[1 + i]) : i);
    if (threadIdx.x == 0) S.cmax = 0u;
    __syncthreads();
    if (lane_id() == 0) atomicMax(&S.cmax, cmax);
    __syncthreads();
    slice = min(readfirst(S.cmax) / prm.lf.pfdiv, PREFIX_FILTERS - 1u);
    // (batch keys below the slice's end, taken as spread evenly over the chunks)
    const uint32_t cend = min(prm.n, (slice + 1u) * prm.lf.pfdiv);
    bkeys = (uint32_t)((uint64_t)bkeys * cend / max(prm.n, 1u));
  }
  const uint32_t keys = readfirst(*prm.nseg) + bkeys;
  const int fmode = keys == 0 ? 0 : (keys <= prm.lds_filter_keys ? 1 : (keys <= prm.lds_prefilter_keys ? 3 : 2));
  if (fmode == 1 || fmode == 3) {
    const u32x4* src = (const u32x4*)(prm.lf.filt + (uint64_t)slice * FILT_WORDS);
    for (uint32_t i = threadIdx.x; i < FILT_WORDS / 4; i += blockDim.x) ((u32x4*)S.lfilt)[i] = src[i];
  }
  __syncthreads();
  const GlbView gs{(char*)&S, (uint32_t)offsetof(L, lfilt),
                   (uint32_t)(offsetof(L, scr) + (size_t)wv * sizeof(S.scr[0])), fmode, S.ro[wv], S.rsv[wv]};
  // The batch's first chunk sees no batch declaration: on an empty cache it
  // probes nothing.  (The filter holds every chunk's keys; in a seeded round
  // of REF-dense data the first chunk's windows match thousands of later
  // chunks' tiles, each an exact lookup that finds nothing visible.)
  const bool g_empty = readfirst(*prm.nseg) == 0u;
  for (uint32_t i = blockIdx.x * SW + (uint32_t)wv; i < items; i += stride) {
    const uint32_t chunk = prm.work ? readfirst(prm.work[1 + i]) : i;
    if (chunk < prm.skip_below) continue;      // input unchanged since its last parse
    if (prm.need && readfirst(prm.need[chunk]) == 0u) continue;   // verified: its parse stands
    GlbView gv = gs;
    if (chunk == 0 && g_empty) gv.fmode = 0;
    encode_chunk<LOGNB, MAXD, true, LRU>(prm, (char*)S.key, (uint32_t)wv << (LOGNB + 3), S.rec[wv], chunk, gv);
  }
}

// Launch the instance the driver picked: big = chunks over 128 KiB (<= 512 KiB
// frames, 264 records), SW chunk-waves per workgroup (2 / 6, or 4 / 8 / 16).
template <bool LRU>
inline void launch_stream_instance(bool big, uint32_t SW, dim3 grid, dim3 block, const EncParams& prm,
                                   hipStream_t stream) {
  if (big) {
    if (SW == 2) hipLaunchKernelGGL((encode_stream_kernel<10, 264, 2, LRU>), grid, block, 0, stream, prm);
    else hipLaunchKernelGGL((encode_stream_kernel<10, 264, 6, LRU>), grid, block, 0, stream, prm);
  } else if (SW == 4) {
    hipLaunchKernelGGL((encode_stream_kernel<8, 72, 4, LRU>), grid, block, 0, stream, prm);
  } else if (SW == 8) {
    hipLaunchKernelGGL((encode_stream_kernel<8, 72, 8, LRU>), grid, block, 0, stream, prm);
  } else {
    hipLaunchKernelGGL((encode_stream_kernel<8, 72, 16, LRU>), grid, block, 0, stream, prm);
  }
}

}  // namespace xcg
