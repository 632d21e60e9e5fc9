// Weight gradient of the stem convolution -- 7x7, stride 2, padding 3, dilation 1, groups 1, THREE input channels -- of
// channels_last FP32 activations on the exact fp32-input MFMA (v_mfma_f32_32x32x2_f32: bitwise a chain of fmaf), for the recipe
// that trains without autocast:
//   dW[n, kh, kw, c] = sum_{b, y, x} dY[b, y, x, n] * X[b, 2y + kh - 3, 2x + kw - 3, c]       kh, kw in 0..6, c in 0..2
// Reference: resnet/train.py trains in fp32; there the backward of conv1 of resnet/models/resnet_mrla_light.py
// (nn.Conv2d(3, 64, 7, 2, 3, bias=False)) is the stock library's, whose solver for it accumulates with atomics.
//
// The contract is conv_spatial.h's and stem_wgrad.hip's, with which this file shares nothing but conv_spatial.h:
//   * No atomics and no memset.  A workgroup owns one output tile (64 n x all 147 (kh, kw, c)) and a FIXED range of output
//     rows; it writes its fp32 partial tile to part[split][n][7][7][3] and split_sum_kernel<float> sums the splits in
//     ascending order into dw.  Every element of part and dw is written exactly once per call; the result depends on the
//     arguments and the shape only.
//   * Every global load is predicated on its own pixel's coordinates: nothing is read outside x or dy, and a step never
//     reads the neighbouring image's rows as if they were padding (rows above the first and below the last row of the image
//     are written to LDS as zeros).
//   * No scratch: 64 n x 192 columns over 256 lanes are 48 accumulator registers per lane.
//
// Geometry (stem_wgrad.hip's).  In NHWC with c = 3 the 7 x 3 = 21 values that tap row kh pairs with output pixel (y, x) are
// contiguous: elements 6x - 9 .. 6x + 11 of input row 2y + kh - 3.  A step takes R output rows of ONE image (or, for rows
// wider than kSfMaxWS output pixels, a column segment of one row) and stages
//   * the dY pixels as a pixel-major tile [p = ry * ws + xl][64 n] (256-byte rows, no swizzle), zeros from R * ws up to an
//     even count, and
//   * the 2R + 5 input rows 2*yo0 - 3 + t as rows of pd dwords, dword e being element 6*xo0 - 9 + e of the input row: zeros
//     in front of and behind the image's row, zero rows outside the image.
// The GEMM is dY^T [64 n x pixels] times columns [pixels x (7 kh x 24)], column (kh, j) of pixel (ry, xl) being element
// 6*xl + j of staged row 2*ry + kh; j = 21..23 are the first values of the next pixel's window, accumulated and never
// stored, as is the eighth block of 24 that fills 168 columns up to 6 x 32.
//
// The operand path.  The instruction takes ONE f32 per lane and operand; its reduction index k (two per instruction, lane l
// holds k = l >> 5) is the pixel: lane half h takes pixel k0 + h, A = dY tile [pixel][n = 32*wn + l % 32], B = one dword of
// the pixel's window per column, both read with ds_read_b32.  Any element offset is 4-byte aligned, so what the 16-bit kernel
// needs for its 8-byte transposing read is gone: ONE copy of every staged input row, and ONE loader of 4-byte loads of x for
// every width, even or odd.
//
// The choices, NONE of them measured against its alternative (profiles/stem_wgrad_f32.md has what was measured):
//   * the staged-row pitch pd = 24 (mod 32) dwords: column col = 24*kh + j of a 32-column block then sits on LDS bank
//     (base + col) % 32 across the kh boundary, so a lane half's 32 columns fall on 32 banks (the clamped eighth block repeats
//     addresses of its neighbours: a broadcast); the dY tile is read 128 contiguous bytes per lane half;
//   * 2 x 2 waves, three independent 32 x 32 blocks a wave: they cover the 64-cycle dependent-accumulator latency;
//   * steps of at most 128 dY pixels (32 KB) and 128 output columns: at most 54 KB of LDS, two workgroups per CU
//     (__launch_bounds__(256, 2)) everywhere; at 112 output columns a step is ONE output row and its seven input rows, so x
//     is fetched 3.5 times (mostly from the L2: the next step's rows overlap) -- two rows a step would take 80.5 KB;
//   * the loader runs NO step ahead: dY in 16-byte pieces (at most eight a lane in flight), x in 4-byte loads, eight a lane
//     in flight; what hides it is the other workgroup of the CU.  Wider loads of x were not tried;
//   * the operands of k-step i + 1 (four LDS reads) are read into registers in front of the three MFMAs of k-step i.
//
// Supported: b, h, w >= 1, n % 64 == 0, b*h*w*3*4 < 2^31 and b*ho*wo*n*4 < 2^31 (32-bit byte offsets into x and into dy).
#include <algorithm>

#include "conv_spatial.h"

namespace mrla {
namespace {

typedef c1_f32x16 sf_f32x16;

constexpr int kSfTile = 64;             // output tile: 64 n x (7 x 24 -> 192) columns
constexpr int kSfWaves = 4;             // 2 (n) x 2 (column halves); three 32 x 32 blocks per wave
constexpr int kSfBlocks = 3;
static_assert(2 * kSfBlocks * 32 >= 7 * 24, "the waves' blocks cover the 7 x 24 columns");
constexpr int kSfTarget = 2 * 256;      // workgroups: two per CU
constexpr int kSfMaxWS = 128;           // output columns of a step
constexpr int kSfMaxKP = 128;           // dY pixels of a step (32 KB): eight 16-byte pieces a lane, all in flight at once
constexpr int kSfMaxR = 16;             // output rows of a step (bounds the staged input rows of narrow maps)
constexpr int kSfRowB = kSfTile * 4;    // bytes of a dY tile row: 64 fp32 channels of one pixel
static_assert(kSfMaxKP == 8 * 16 && kSfMaxWS <= kSfMaxKP, "the dY loader takes the tile in one pass");
constexpr int kSfLdsCap = 80 * 1024;    // LDS of a workgroup, at most (ws = 128, R = 1: 32 KB + 7 * 3168 B)

struct SfPlan {
  int ok = 0;
  int ho = 0, wo = 0;
  int ws = 0, nseg = 0, rmax = 0;              // output columns per segment, segments per row, rows per step
  int kp_cap = 0, pd = 0, lds = 0;             // dY tile rows; dwords of a staged input row; LDS bytes
  int rows_per_split = 0, splits = 0, tiles = 0;
};

struct SfArgs {
  int b, h, w, ho, wo, n;
  int ws, nseg, rmax, kp_cap, pd;
  int rows_per_split, splits;
  float inv_ws, inv_pd;
};

// grid: (n / 64) * splits workgroups, 256 threads; LDS = kp_cap * 256 + (2 * rmax + 5) * pd * 4 bytes
__global__ __launch_bounds__(kSfWaves* kWave, 2) void stem_wgrad_f32_kernel(const float* __restrict__ dY,
                                                                           const float* __restrict__ X,
                                                                           float* __restrict__ part, SfArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __align__(16) unsigned char smem_raw[];
  unsigned char* const ty_tile = smem_raw;
  float* const tx_rows = reinterpret_cast<float*>(smem_raw + a.kp_cap * kSfRowB);
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int tiles = a.n / kSfTile;
  const int split = blockIdx.x / tiles, tn = blockIdx.x - split * tiles;
  const int n0 = tn * kSfTile;
  const int rows = a.b * a.ho;
  const int r_begin = split * a.rows_per_split, r_end = min(rows, r_begin + a.rows_per_split);

  const int wn = wave >> 1, wc = wave & 1;
  const int hh = lane >> 5;                                 // this lane's pixel of a two-pixel k-step
  const int colA = (wn * 32 + (lane & 31)) * 4;             // byte column of its n
  // this lane's column of each of its wave's three blocks: (kh, j), a constant dword offset from the pixel's window in
  // staged row 2*ry (the eighth block of 24 does not exist: held at kh = 6, accumulated and never stored)
  int offB[kSfBlocks];
#pragma unroll
  for (int bl = 0; bl < kSfBlocks; ++bl) {
    const int col = 32 * (kSfBlocks * wc + bl) + (lane & 31);
    const int kh = min(col / 24, 6), j = col % 24;
    offB[bl] = kh * a.pd + j;
  }

  sf_f32x16 acc[kSfBlocks];
#pragma unroll
  for (int t = 0; t < kSfBlocks; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  const int prow = tid >> 4, pch = tid & 15;                // the dY loader: 16 tile rows per pass, 16 pieces a row
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  const int row_el = 3 * a.w;                               // elements of an image row
  constexpr int kThreadsWg = kSfWaves * kWave;
  constexpr int kSfXUnroll = 8;                             // 4-byte loads of x a lane has in flight
  // (32-bit byte offsets from the uniform bases: the planner refuses an x or a dy of 2^31 bytes)
  const unsigned char* const dYb = reinterpret_cast<const unsigned char*>(dY);
  const unsigned char* const Xb = reinterpret_cast<const unsigned char*>(X);

  for (int r = r_begin; r < r_end;) {
    const RowStep st = row_step(r, r_end, a.ho, a.rmax);
    const int img = st.img, yo0 = st.yo0, R = st.R;
    for (int seg = 0; seg < a.nseg; ++seg) {
      const int xo0 = seg * a.ws, ws = min(a.ws, a.wo - xo0);
      // (ws < a.ws only in the ragged last segment of a row cut into segments, where R = 1: pixel p = xl under either pitch)
      const int NP = R * ws, KP = (NP + 1) & ~1;
      const int yi0 = 2 * yo0 - 3, ge0 = 6 * xo0 - 9;
      const int nx = (2 * R + 5) * a.pd;                    // staged dwords of the step's input rows
      __syncthreads();                                      // the previous step's reads are done
      // ---- dY tile: rows [0, KP), every load predicated on its own pixel, zeros elsewhere ----
      u32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int p = 16 * u + prow;
        const int ry = (int)(((float)p + 0.5f) * a.inv_ws), xl = p - ry * a.ws;
        v[u] = zero4;
        if (p < KP && ry < R && xl < ws)
          v[u] = *reinterpret_cast<const u32x4*>(
              dYb + 4u * (unsigned)(((img * a.ho + yo0 + ry) * a.wo + xo0 + xl) * a.n + n0 + pch * 4));
      }
      // ---- input rows: staged dword idx = (row t, dword e) = element ge0 + e of input row yi0 + t, zeros outside the image ----
      auto load_x = [&](int i0, float (&xv)[kSfXUnroll]) {
#pragma unroll
        for (int u = 0; u < kSfXUnroll; ++u) {
          const int idx = i0 + kThreadsWg * u;
          const int t = (int)(((float)idx + 0.5f) * a.inv_pd), e = idx - t * a.pd;
          const int yi = yi0 + t, ge = ge0 + e;
          xv[u] = 0.f;
          if (idx < nx && yi >= 0 && yi < a.h && ge >= 0 && ge < row_el)
            xv[u] = *reinterpret_cast<const float*>(Xb + 4u * (unsigned)((img * a.h + yi) * row_el + ge));
        }
      };
      auto store_x = [&](int i0, const float (&xv)[kSfXUnroll]) {
#pragma unroll
        for (int u = 0; u < kSfXUnroll; ++u) {
          const int idx = i0 + kThreadsWg * u;
          if (idx < nx) tx_rows[idx] = xv[u];
        }
      };
      float xv[kSfXUnroll];
      load_x(tid, xv);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int p = 16 * u + prow;
        if (p < KP) *reinterpret_cast<u32x4*>(ty_tile + p * kSfRowB + pch * 16) = v[u];
      }
      store_x(tid, xv);
      for (int i0 = tid + kSfXUnroll * kThreadsWg; i0 < nx; i0 += kSfXUnroll * kThreadsWg) {
        load_x(i0, xv);
        store_x(i0, xv);
      }
      __syncthreads();
      // ---- the product over the step's pixels, two pixels an instruction; the next k-step's operands are read first ----
      // the window of pixel p = ry * ws + xl: staged row 2*ry, dword 6*xl.  The pad pixel behind an odd count (all zeros in dY)
      // addresses the last pixel's window and takes zeros instead of its values: 0 * 0, also where x holds an Inf or a NaN.
      auto read_ops = [&](int k0, float& fa, float (&fb)[kSfBlocks]) {
        const int k = k0 + hh;
        fa = *reinterpret_cast<const float*>(ty_tile + k * kSfRowB + colA);
        const int p = min(k, NP - 1);
        const int ry = (int)(((float)p + 0.5f) * a.inv_ws), xl = p - ry * a.ws;
        const float* const win = tx_rows + 2 * ry * a.pd + 6 * xl;
#pragma unroll
        for (int bl = 0; bl < kSfBlocks; ++bl) fb[bl] = k < NP ? win[offB[bl]] : 0.f;
      };
      float fa, fb[kSfBlocks];
      read_ops(0, fa, fb);
      for (int k0 = 0; k0 < KP; k0 += 2) {
        float fan = fa, fbn[kSfBlocks];
#pragma unroll
        for (int bl = 0; bl < kSfBlocks; ++bl) fbn[bl] = fb[bl];
        if (k0 + 2 < KP) read_ops(k0 + 2, fan, fbn);
#pragma unroll
        for (int bl = 0; bl < kSfBlocks; ++bl) acc[bl] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb[bl], acc[bl], 0, 0, 0);
        fa = fan;
#pragma unroll
        for (int bl = 0; bl < kSfBlocks; ++bl) fb[bl] = fbn[bl];
      }
    }
    r += R;
  }

  // ---- partial tile: D[i][j], j = lane % 32 (column) on the lane, i = 8*(e/4) + 4*(lane/32) + e%4 (n) in register e ----
#pragma unroll
  for (int bl = 0; bl < kSfBlocks; ++bl) {
    const int col = 32 * (kSfBlocks * wc + bl) + (lane & 31);
    const int kh = col / 24, j = col - kh * 24;
    if (kh < 7 && j < 21) {
      float* po = part + ((size_t)split * a.n + n0 + wn * 32) * 147 + kh * 21 + j;
#pragma unroll
      for (int e = 0; e < 16; ++e) po[(size_t)(8 * (e >> 2) + 4 * hh + (e & 3)) * 147] = acc[bl][e];
    }
  }
#endif
}

// A step: whole output rows where one has at most kSfMaxWS pixels -- as many as kSfMaxKP pixels hold, kSfMaxR at most --
// else segments of one row.  Splits over output rows so that the grid is two workgroups per CU where the rows allow it.
SfPlan sf_plan(int b, int n, int h, int w) {
  SfPlan p;
  if (b <= 0 || n <= 0 || h <= 0 || w <= 0 || n % kSfTile) return p;
  p.ho = (h - 1) / 2 + 1;
  p.wo = (w - 1) / 2 + 1;
  if ((unsigned long long)b * h * w * 3 * 4 >= 1ull << 31) return p;             // bytes of x
  if ((unsigned long long)b * p.ho * p.wo * n * 4 >= 1ull << 31) return p;       // bytes of dy
  if (p.wo <= kSfMaxWS) {
    p.ws = p.wo; p.nseg = 1;
    p.rmax = std::max(1, std::min(std::min(p.ho, kSfMaxR), kSfMaxKP / p.ws));
  } else {
    p.ws = kSfMaxWS; p.nseg = (p.wo + p.ws - 1) / p.ws;
    p.rmax = 1;
  }
  p.kp_cap = (p.rmax * p.ws + 1) & ~1;
  p.pd = (6 * p.ws + 18 - 24 + 31) / 32 * 32 + 24;         // >= the 6*ws + 18 elements a step reads, 24 (mod 32)
  p.lds = p.kp_cap * kSfRowB + (2 * p.rmax + 5) * p.pd * 4;
  if (p.lds > kSfLdsCap) return p;
  p.tiles = n / kSfTile;
  const long long rows = (long long)b * p.ho;
  // ... but a split is at least one full step: its five halo rows of x are loaded once per step
  const RowSplit sp = split_rows(rows, p.tiles, kSfTarget, 1, std::min<long long>(rows, p.rmax));
  p.rows_per_split = sp.per;
  p.splits = sp.count;
  p.ok = 1;
  return p;
}

}  // namespace

int stem_conv_f32_wgrad_rows(int b, int n, int h, int w) {
  const SfPlan p = sf_plan(b, n, h, w);
  return p.ok ? p.splits : MRLA_EUNSUPPORTED;
}

// {tile n, output rows per split, splits, column segments per row, LDS bytes, output columns per segment, output rows per step}
int stem_conv_f32_wgrad_plan(int b, int n, int h, int w, int* out) {
  const SfPlan p = sf_plan(b, n, h, w);
  if (!p.ok) return MRLA_EUNSUPPORTED;
  out[0] = kSfTile; out[1] = p.rows_per_split; out[2] = p.splits; out[3] = p.nseg; out[4] = p.lds; out[5] = p.ws; out[6] = p.rmax;
  return MRLA_OK;
}

int launch_stem_conv_f32_wgrad(const float* dy, const float* x, float* part, float* dw, int b, int n, int h, int w,
                               hipStream_t st) {
  const SfPlan p = sf_plan(b, n, h, w);
  if (!p.ok) return MRLA_EUNSUPPORTED;
  SfArgs a;
  a.b = b; a.h = h; a.w = w; a.ho = p.ho; a.wo = p.wo; a.n = n;
  a.ws = p.ws; a.nseg = p.nseg; a.rmax = p.rmax; a.kp_cap = p.kp_cap; a.pd = p.pd;
  a.rows_per_split = p.rows_per_split; a.splits = p.splits;
  a.inv_ws = 1.0f / (float)p.ws; a.inv_pd = 1.0f / (float)p.pd;
  if (lds_opt_in(reinterpret_cast<const void*>(stem_wgrad_f32_kernel), (size_t)p.lds) != hipSuccess) return MRLA_EHIP;
  hipLaunchKernelGGL(stem_wgrad_f32_kernel, dim3(p.tiles * p.splits), dim3(kSfWaves * kWave), (size_t)p.lds, st, dy, x, part, a);
  const int rc = hip_status(hipGetLastError());
  if (rc != MRLA_OK) return rc;
  return launch_split_sum(part, dw, 1, MRLA_F32, p.splits, n * 147, st);
}

}  // namespace mrla
