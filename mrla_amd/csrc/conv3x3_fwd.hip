// Forward of a 3x3 convolution (padding 1, dilation 1, groups 1, stride s = 1 or 2) of channels_last bf16 or fp16
// activations as an implicit GEMM on the MFMA, with the BatchNorm moment records of its rounded outputs:
//   y[b, yo, xo, n] = round( sum_{kh, kw, c} x[b, yo*s + kh - 1, xo*s + kw - 1, c] * wt[n, kh, kw, c] )
// Reference: conv2 of the bottleneck (resnet/models/resnet_mrla_light.py, conv3x3 of Bottleneck) and both 3x3 convolutions of
// the basic block, which the reference leaves to cuDNN; with the weight flipped and transposed (wflip[c, kh, kw, n] =
// wt[n, 2-kh, 2-kw, c]) the same kernel at stride 1 is that convolution's input gradient.
//
// Ownership (conv_spatial.h): a workgroup owns 64 output channels and a FIXED range of output rows.  It walks its range in
// steps of R rows of ONE image -- or, for rows wider than a step, pieces of one row -- and for every step sums all nine
// taps and all of c, in c-chunks of 64 in ascending order, in fp32 accumulators: no split over the reduction, no atomics, no memset, every element of y written exactly once,
// one rounding to nearest even at the store.  y and the records are a function of the arguments alone.
//
// Borders: conv_spatial.h's X raster.  Output pixel (ry, j) of a step is accumulator column p = ry*PY + j,
// so tap (kh, kw) of column p reads raster row s*p + s*(s-1)*PY*ry + kh*PX + kw: a constant offset from a row the lane
// computes once per step.  Nothing is read outside x or wt.  The pad columns and the tail of the raster are computed and
// not stored (81/49 of the useful MFMA work at a 7x7 map).
//
// Operands: both are contiguous along c.  The weights of the c-chunk sit in LDS as [64 n][9 taps][64 c] (72 KB; loaded
// once per workgroup where c = 64, per step and chunk otherwise), the raster as [pixel][64 c]; rows are 128 bytes and 16-byte
// chunk ch of row r sits at chunk position ch ^ ((r >> 1) & 7), so the 16 lanes of a ds_read_b128 group, which read one
// chunk of 16 rows, cover all 64 banks where the rows are distinct mod 16: consecutive pixels at stride 1, and weight rows
// 9 apart (9 is odd); every other raster row at stride 2 is two-way.  n is the accumulator's ROW index
// (A = weights, B = raster), so a lane holds 4 consecutive channels of one pixel and stores 8 bytes.
// Four waves: 2 halves of n x 2 interleaved 32-pixel blocks, at most two 32x32 accumulators per wave; one workgroup per
// CU (up to 136 KB of LDS), a synchronous register-staged loader.
//
// Moments (mom != null): one record [range, n, 4] = (sum (y - p), sum (y - p)^2, p, count) per channel over the ROUNDED outputs
// of the range's real pixels, p = the range's first rounded output of the channel (MRLA_GEMM_MOMENTS, what
// mrla_bn_stats_fwd_rows merges).  A lane sums its pixels in step order, the 32 lanes of a half-wave are added by an xor
// butterfly and the two pixel-waves in ascending order: a fixed order.
#include <algorithm>

#include "conv_spatial.h"

namespace mrla {
namespace {

typedef c1_f32x16 f3_f32x16;

constexpr int kF3Tile = 64;             // output channels of a workgroup
constexpr int kF3Target = 256;          // workgroups: one per CU
constexpr int kF3MaxKP1 = 128;          // raster pixels (accumulator columns) of a step at stride 1: four 32-pixel blocks
constexpr int kF3MaxKP2 = 96;           // ... at stride 2, where the X raster has four times the rows (<= 62 KB)
constexpr int kF3MaxPY = 60;            // raster pitch of the outputs
constexpr int kF3WRows = kF3Tile * 9;   // weight rows of a c-chunk
constexpr int kF3Misc = 2048;           // pivots [64] and the two pixel-waves' sums [2][64][2], in front of the tiles

struct F3Plan : Raster3x3 {
  int rows_per_wg = 0, ranges = 0, tiles = 0;
};

struct F3Args {
  int b, h, w, ho, wo, c, n;
  int py, ws, nseg, rmax;
  int rows_per_wg;
  float inv_py, inv_px;
};

__device__ __forceinline__ int f3_off(int row, int chunk) { return tile_off<7, 0>(row, chunk); }

// grid: (n / 64) * ranges workgroups, 256 threads; LDS = kF3Misc + (576 + xt_cap) * 128 bytes
template <typename T, int S, bool MOM>
__global__ __launch_bounds__(kThreads, 1) void conv3x3_fwd_kernel(const T* __restrict__ X, const T* __restrict__ W,
                                                                  T* __restrict__ Y, float* __restrict__ mom, F3Args a) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef typename Elem16<T>::x8 x8;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  float* const s_piv = reinterpret_cast<float*>(smem_raw);
  float* const s_red = s_piv + kF3Tile;
  unsigned char* const w_tile = smem_raw + kF3Misc;
  unsigned char* const x_tile = w_tile + kF3WRows * kTileRowB;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int tiles_n = a.n / kF3Tile;
  const int range = blockIdx.x / tiles_n, n0 = (blockIdx.x - range * tiles_n) * kF3Tile;
  const int rows = a.b * a.ho;
  const int r_begin = range * a.rows_per_wg, r_end = min(rows, r_begin + a.rows_per_wg);
  const int PY = a.py, PX = S * a.py;
  const int chunks = a.c / kF3Tile;

  const int wn = wave & 1, wp = wave >> 1;                 // this wave's half of n, and its pixel blocks wp, wp + 2
  const int l31 = lane & 31, hh = lane >> 5;
  const int prow = tid >> 3, pch = tid & 7;                // the loader: 32 LDS rows per pass, 8 pieces a row
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  float piv[16], s1[16], s2[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) piv[e] = s1[e] = s2[e] = 0.f;
  bool first = true;

  for (int r = r_begin; r < r_end;) {
    const RowStep st = row_step(r, r_end, a.ho, a.rmax);
    const int img = st.img, yo0 = st.yo0, R = st.R;
    for (int seg = 0; seg < a.nseg; ++seg) {
      const int xo0 = seg * a.ws, ws = min(a.ws, a.wo - xo0);
      const int KP = (R * PY + 31) & ~31;
      const int XT = S * KP + S * (S - 1) * PY * (R - 1) + 2 * PX + 3;
      const int ty_need = S * (R - 1) + 3, cx_need = S * (ws - 1) + 3;      // X raster rows / columns some tap of this step reads
      const int yi0 = yo0 * S - 1, xi0 = xo0 * S - 1;

      // this lane's pixel of its two blocks: raster row under tap (0, 0) (the tail behind the step's last row stays inside
      // the raster with ry held at R - 1), and whether it is a pixel of y
      bool act[2], real[2];
      int xr[2];
      size_t yoff[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int p = (wp + 2 * i) * 32 + l31;
        const int ry = (int)(((float)p + 0.5f) * a.inv_py), j = p - ry * PY;
        act[i] = (wp + 2 * i) * 32 < KP;
        real[i] = act[i] && ry < R && j < ws;
        xr[i] = S * p + S * (S - 1) * PY * min(ry, R - 1);
        yoff[i] = real[i] ? ((size_t)(img * a.ho + yo0 + ry) * a.wo + xo0 + j) * a.n + n0 + wn * 32 + 4 * hh : 0;
      }

      f3_f32x16 acc[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

      for (int cc = 0; cc < chunks; ++cc) {
        __syncthreads();                                    // the previous chunk's reads are done
        // ---- weights of the chunk: rows [0, 576), row = nl * 9 + tap ----
        if (chunks > 1 || first) {
          const T* wsrc = W + (size_t)n0 * 9 * a.c + cc * kF3Tile + pch * 8;
#pragma unroll 1
          for (int q0 = 0; q0 < kF3WRows; q0 += 192) {
            u32x4 v[6];
#pragma unroll
            for (int u = 0; u < 6; ++u) v[u] = *reinterpret_cast<const u32x4*>(wsrc + (size_t)(q0 + 32 * u + prow) * a.c);
#pragma unroll
            for (int u = 0; u < 6; ++u) *reinterpret_cast<u32x4*>(w_tile + f3_off(q0 + 32 * u + prow, pch)) = v[u];
          }
        }
        // ---- X raster of the chunk: rows [0, XT) ----
        for (int t0 = 0; t0 < XT; t0 += 128) {
          u32x4 v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int t = t0 + 32 * u + prow;
            const int ty = (int)(((float)t + 0.5f) * a.inv_px), cx = t - ty * PX;
            const int yi = yi0 + ty, xi = xi0 + cx;
            v[u] = zero4;
            if (t < XT && ty < ty_need && cx < cx_need && yi >= 0 && yi < a.h && xi >= 0 && xi < a.w)
              v[u] = *reinterpret_cast<const u32x4*>(X + ((size_t)((img * a.h + yi) * a.w + xi) * a.c + cc * kF3Tile + pch * 8));
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int t = t0 + 32 * u + prow;
            if (t < XT) *reinterpret_cast<u32x4*>(x_tile + f3_off(t, pch)) = v[u];
          }
        }
        __syncthreads();
        // ---- nine taps x four k-steps of 16 channels ----
        if (act[0]) {
#pragma unroll
          for (int tap = 0; tap < 9; ++tap) {
            const int wrow = (wn * 32 + l31) * 9 + tap;
            const int toff = (tap / 3) * PX + tap % 3;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
              const int ch = 2 * kk + hh;
              const x8 fa = *reinterpret_cast<const x8*>(w_tile + f3_off(wrow, ch));
              const x8 fb0 = *reinterpret_cast<const x8*>(x_tile + f3_off(xr[0] + toff, ch));
              Elem16<T>::mfma(acc[0], fa, fb0);
              if (act[1]) {
                const x8 fb1 = *reinterpret_cast<const x8*>(x_tile + f3_off(xr[1] + toff, ch));
                Elem16<T>::mfma(acc[1], fa, fb1);
              }
            }
          }
        }
      }

      // ---- D[i][j]: j = lane % 32 (pixel) on the lane, i = 8*(e/4) + 4*(lane/32) + e%4 (n) in register e ----
      unsigned pk[2][8];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int g = 0; g < 8; ++g) pk[i][g] = Elem16<T>::pack(acc[i][2 * g], acc[i][2 * g + 1]);
      if (MOM && first) {                                   // (workgroup-uniform) pixel 0 of the range's first step: the pivots
        if (wp == 0 && l31 == 0)
#pragma unroll
          for (int g = 0; g < 8; ++g) {
            const int nl = wn * 32 + 8 * (g >> 1) + 4 * hh + 2 * (g & 1);
            s_piv[nl] = Elem16<T>::lo(pk[0][g]);
            s_piv[nl + 1] = Elem16<T>::hi(pk[0][g]);
          }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; ++e) piv[e] = s_piv[wn * 32 + 8 * (e >> 2) + 4 * hh + (e & 3)];
      }
      first = false;
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (real[i]) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            uint2 o;
            o.x = pk[i][2 * g];
            o.y = pk[i][2 * g + 1];
            *reinterpret_cast<uint2*>(Y + yoff[i] + 8 * g) = o;
          }
          if (MOM) {
#pragma unroll
            for (int g = 0; g < 8; ++g) {
              const float d0 = Elem16<T>::lo(pk[i][g]) - piv[2 * g], d1 = Elem16<T>::hi(pk[i][g]) - piv[2 * g + 1];
              s1[2 * g] += d0;
              s2[2 * g] += d0 * d0;
              s1[2 * g + 1] += d1;
              s2[2 * g + 1] += d1 * d1;
            }
          }
        }
    }
    r += R;
  }

  if (MOM) {
#pragma unroll
    for (int e = 0; e < 16; ++e)
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) {
        s1[e] += __shfl_xor(s1[e], off, kWave);
        s2[e] += __shfl_xor(s2[e], off, kWave);
      }
    if (l31 == 0)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int nl = wn * 32 + 8 * (e >> 2) + 4 * hh + (e & 3);
        s_red[(wp * kF3Tile + nl) * 2] = s1[e];
        s_red[(wp * kF3Tile + nl) * 2 + 1] = s2[e];
      }
    __syncthreads();
    if (tid < kF3Tile) {
      float4 rec;
      rec.x = s_red[tid * 2] + s_red[(kF3Tile + tid) * 2];
      rec.y = s_red[tid * 2 + 1] + s_red[(kF3Tile + tid) * 2 + 1];
      rec.z = s_piv[tid];
      rec.w = (float)((r_end - r_begin) * a.wo);
      *reinterpret_cast<float4*>(mom + ((size_t)range * a.n + n0 + tid) * 4) = rec;
    }
  }
#endif
}

size_t f3_lds_bytes(const F3Plan& p) { return kF3Misc + (size_t)(kF3WRows + p.xt_cap) * kTileRowB; }

// conv_spatial.h's raster of a step (accumulator columns in whole 32-pixel blocks), and ranges of output rows so that the
// grid is one workgroup per CU.
F3Plan f3_plan(int b, int c, int n, int h, int w, int s) {
  F3Plan p;
  static_cast<Raster3x3&>(p) = raster3x3(b, c, n, h, w, s, kF3MaxKP1, kF3MaxKP2, kF3MaxPY, 32);
  if (!p.ok) return p;
  p.tiles = n / kF3Tile;
  // where c = 64 the weights (72 KB, three times a step's raster) are loaded once per workgroup: at least two full steps behind them
  const RowSplit sp = split_rows((long long)b * p.ho, p.tiles, kF3Target, (c == kF3Tile ? 2 : 1) * p.rmax);
  p.rows_per_wg = sp.per;
  p.ranges = sp.count;
  // (weights + raster <= 136 KB by the caps above; the queries and the launch answer from this one place)
  p.ok = f3_lds_bytes(p) <= 160 * 1024;
  return p;
}

template <typename T, int S>
int f3_launch(const F3Plan& p, const F3Args& a, const void* x, const void* wt, void* y, float* mom, hipStream_t st) {
  const size_t lds = f3_lds_bytes(p);
  const dim3 grid(p.tiles * p.ranges), block(kThreads);
  if (mom) {
    if (lds_opt_in(reinterpret_cast<const void*>(conv3x3_fwd_kernel<T, S, true>), lds) != hipSuccess) return MRLA_EHIP;
    hipLaunchKernelGGL((conv3x3_fwd_kernel<T, S, true>), grid, block, lds, st, (const T*)x, (const T*)wt, (T*)y, mom, a);
  } else {
    if (lds_opt_in(reinterpret_cast<const void*>(conv3x3_fwd_kernel<T, S, false>), lds) != hipSuccess) return MRLA_EHIP;
    hipLaunchKernelGGL((conv3x3_fwd_kernel<T, S, false>), grid, block, lds, st, (const T*)x, (const T*)wt, (T*)y, mom, a);
  }
  return hip_status(hipGetLastError());
}

}  // namespace

int conv3x3_fwd_rows(int b, int c, int n, int h, int w, int s) {
  const F3Plan p = f3_plan(b, c, n, h, w, s);
  return p.ok ? p.ranges : MRLA_EUNSUPPORTED;
}

// {tile n, output rows per workgroup, rows per step, segments per row, record rows, workgroups}
int conv3x3_fwd_plan(int b, int c, int n, int h, int w, int s, int* out) {
  const F3Plan p = f3_plan(b, c, n, h, w, s);
  if (!p.ok) return MRLA_EUNSUPPORTED;
  out[0] = kF3Tile; out[1] = p.rows_per_wg; out[2] = p.rmax; out[3] = p.nseg; out[4] = p.ranges; out[5] = p.tiles * p.ranges;
  return MRLA_OK;
}

int launch_conv3x3_fwd(const void* x, const void* wt, void* y, float* mom, int b, int c, int n, int h, int w, int s, int dtype,
                       hipStream_t st) {
  const F3Plan p = f3_plan(b, c, n, h, w, s);
  if (!p.ok || (dtype != MRLA_BF16 && dtype != MRLA_F16)) return MRLA_EUNSUPPORTED;
  F3Args a;
  a.b = b; a.h = h; a.w = w; a.ho = p.ho; a.wo = p.wo; a.c = c; a.n = n;
  a.py = p.py; a.ws = p.ws; a.nseg = p.nseg; a.rmax = p.rmax;
  a.rows_per_wg = p.rows_per_wg;
  a.inv_py = 1.0f / (float)p.py; a.inv_px = 1.0f / (float)(s * p.py);
  if (dtype == MRLA_F16)
    return s == 1 ? f3_launch<f16_t, 1>(p, a, x, wt, y, mom, st) : f3_launch<f16_t, 2>(p, a, x, wt, y, mom, st);
  return s == 1 ? f3_launch<bf16_t, 1>(p, a, x, wt, y, mom, st) : f3_launch<bf16_t, 2>(p, a, x, wt, y, mom, st);
}

}  // namespace mrla
