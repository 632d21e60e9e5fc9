// Shared pieces of the channels_last (NHWC) MRLA-light kernels: the strip geometry (kS, kMaxStrips), the 3x3 taps on a row
// window and the workgroup's reduction -- which the row pipeline (light_nhwc_wide.h, nhwc_rows.h) uses as well -- and, for the
// fallback kernels of the channel counts that are no multiple of 64 (light_nhwc.hip, light_nhwc_bwd.hip, base_nhwc.hip), the
// pixel-by-pixel row readers / writers, the workgroup prologue and the launch geometry.
#pragma once
#include <algorithm>

#include "mrla_device.h"
#include "mrla_kernels.h"
#include "mrla_launch.h"

namespace mrla {

constexpr int kS = 7;          // owned columns per strip
constexpr int kMaxStrips = 8;  // waves per workgroup (wider images loop strips inside a wave)

template <typename T>
__device__ __forceinline__ float ldpix(const T* __restrict__ img, int r, int col, int H, int W, int C, int c) {
  // wave-uniform predicate: all lanes look at the same pixel
  if (r < 0 || r >= H || col < 0 || col >= W) return 0.f;
  return to_f(img[((size_t)r * W + col) * C + c]);
}

__device__ __forceinline__ float conv_at(const float (&w)[9], const float* __restrict__ ra, const float* __restrict__ rb,
                                         const float* __restrict__ rc, int j) {
  float s = w[0] * ra[j];
  s = fmaf(w[1], ra[j + 1], s); s = fmaf(w[2], ra[j + 2], s);
  s = fmaf(w[3], rb[j], s); s = fmaf(w[4], rb[j + 1], s); s = fmaf(w[5], rb[j + 2], s);
  s = fmaf(w[6], rc[j], s); s = fmaf(w[7], rc[j + 1], s); s = fmaf(w[8], rc[j + 2], s);
  return s;
}

// Sum per-lane accumulators over the waves of the workgroup that hold the same channels -- waves v with equal v % wc (wc = 1:
// all of them) -- in a fixed order; result valid in waves 0 .. wc-1.
template <int K>
__device__ __forceinline__ void wg_reduce(float (&acc)[K], float* __restrict__ red, int lane, int wave, int nwaves,
                                          int wc = 1) {
  if (nwaves == wc) return;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) red[(wave * K + k) * kWave + lane] = acc[k];
  __syncthreads();
  if (wave < wc) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float s = 0.f;
      for (int v = wave; v < nwaves; v += wc) s += red[(v * K + k) * kWave + lane];
      acc[k] = s;
    }
  }
}

// Row readers / writers of the kernels: NPX pixels of row r from column col0 on, this lane's channel (zero outside the image)
template <typename T, int NPX>
__device__ __forceinline__ void read_row(const T* __restrict__ img, int r, int col0, int H, int W, int C, int cc,
                                         float (&out)[NPX]) {
#pragma unroll
  for (int j = 0; j < NPX; ++j) out[j] = ldpix(img, r, col0 + j, H, W, C, cc);
}
template <typename T, int NPX>
__device__ __forceinline__ void write_row(T* __restrict__ img, int r, int col0, int npx, int W, int C, int c, bool cv,
                                          const float (&v)[NPX]) {
#pragma unroll
  for (int j = 0; j < NPX; ++j)
    if (j < npx && cv) img[((size_t)r * W + col0 + j) * C + c] = from_f<T>(v[j]);
}

// lane = channel of the workgroup's 64-channel chunk (cc: clamped, for loads), wave = column strip; red: NRED floats per lane
// and wave for wg_reduce
#define MRLA_NHWC_PROLOGUE(NRED)                                                                          \
  extern __shared__ __align__(16) unsigned char smem_raw[];                                               \
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nwaves = blockDim.x / kWave;    \
  float* red = reinterpret_cast<float*>(smem_raw);                                                        \
  const int c = blockIdx.x * kWave + lane;                                                                \
  const bool cv = c < C;                                                                                  \
  const int cc = cv ? c : C - 1;                                                                          \
  const int nstrips = (W + kS - 1) / kS;                                                                  \
  (void)red; (void)lane;

struct NhwcLaunch { dim3 grid, block; size_t lds; int BG; };
static NhwcLaunch nhwc_launch(int B, int C, int W, int nred) {
  NhwcLaunch L;
  const int nwaves = std::min((W + kS - 1) / kS, kMaxStrips);
  L.BG = nhwc_images_per_group(B, C, 0);
  L.grid = dim3((C + kWave - 1) / kWave, (B + L.BG - 1) / L.BG);
  L.block = dim3(nwaves * kWave);
  L.lds = (size_t)nwaves * nred * kWave * sizeof(float);
  return L;
}

}  // namespace mrla
