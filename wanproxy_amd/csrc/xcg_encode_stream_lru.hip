// The stream parse kernel's instances that record every cache reference a chunk
// makes (EncParams::ev: bounded caches, pairs); they compile beside the plain five.
#include "xcg_encode_stream.h"

namespace xcg {

template __global__ void encode_stream_kernel<8, 72, 16, true>(EncParams);
template __global__ void encode_stream_kernel<8, 72, 8, true>(EncParams);
template __global__ void encode_stream_kernel<8, 72, 4, true>(EncParams);
template __global__ void encode_stream_kernel<10, 264, 6, true>(EncParams);
template __global__ void encode_stream_kernel<10, 264, 2, true>(EncParams);

}  // namespace xcg

extern "C" void xcg_launch_encode_stream_lru(int big, uint32_t SW, dim3 grid, dim3 block, const xcg::EncParams* prm,
                                             hipStream_t stream) {
  xcg::launch_stream_instance<true>(big != 0, SW, grid, block, *prm, stream);
}
