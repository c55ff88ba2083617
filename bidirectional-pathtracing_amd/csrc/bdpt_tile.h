// bdpt_tile.h — the two launch shapes of the frame-sized post kernels (bdpt_denoise.hip,
// bdpt_variance.hip, bdpt_adaptive.hip): a wave per 8x8 pixel tile, and a lane per pixel in frame order.
#pragma once

#include <hip/hip_runtime.h>

namespace bdpt {

// A wave owns an 8x8 pixel tile (lane = pixel), so a filter's taps fall in few cache lines at every
// step; four tiles per 256-thread block.
constexpr int kAtrousBlock = 256;

__device__ __forceinline__ bool tile_pixel(int W, int H, int& x, int& y) {
  const int ntx = (W + 7) / 8;
  const long long tile = (long long)blockIdx.x * (kAtrousBlock / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  x = (int)(tile % ntx) * 8 + (lane & 7);
  y = (int)(tile / ntx) * 8 + (lane >> 3);
  return x < W && y < H;
}

inline dim3 tile_grid(int W, int H) {
  const long long tiles = (long long)((W + 7) / 8) * ((H + 7) / 8);
  return dim3((unsigned)((tiles + kAtrousBlock / 64 - 1) / (kAtrousBlock / 64)));
}

// One lane per pixel, linear over the frame.
constexpr int kLinBlock = 256;

inline unsigned lin_grid(size_t npix) { return (unsigned)((npix + kLinBlock - 1) / kLinBlock); }

}  // namespace bdpt
