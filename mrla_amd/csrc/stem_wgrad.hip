// Weight gradient of the stem convolution -- 7x7, stride 2, padding 3, dilation 1, groups 1, THREE input channels -- of
// channels_last bf16 or fp16 activations as one split-pixel MFMA product:
//   dW[n, kh, kw, c] = sum_{b, y, x} dY[b, y, x, n] * X[b, 2y + kh - 3, 2x + kw - 3, c]       kh, kw in 0..6, c in 0..2
// Reference: the backward of conv1 of resnet/models/resnet_mrla_light.py (nn.Conv2d(3, 64, 7, 2, 3, bias=False)), which the
// reference leaves to cuDNN; the stock library's solver for it accumulates with atomics.
//
// The contract is conv_spatial.h's:
//   * No atomics and no memset.  A workgroup owns one output tile (64 n x all 147 (kh, kw, c)) and a FIXED range of output
//     rows; it writes its fp32 partial tile to part[split][n][7][7][3] and split_sum_kernel sums the splits in ascending
//     order into dw (fp32, or the operands' 16-bit type rounded once).  Every element of part and dw is written exactly once
//     per call; the result depends on the arguments and the shape only.
//   * Every global load is predicated on its own pixel's coordinates: nothing is read outside x or dy, and a step never
//     reads the neighbouring image's rows as if they were padding (rows above the first and below the last row of the image
//     are written to LDS as zeros).
//   * No scratch: 64 n x 192 columns over 256 lanes are 48 accumulator registers per lane.
//
// Geometry.  In NHWC with c = 3 the 7 x 3 = 21 values that tap row kh pairs with output pixel (y, x) are contiguous:
// elements 6x - 9 .. 6x + 11 of input row 2y + kh - 3.  A step takes R output rows of ONE image (or, for rows wider than
// kSwMaxWS output pixels, a column segment of one row) and stages
//   * the dY pixels as a pixel-major tile [p = ry * ws + xl][64 n] (128-byte rows, tile_off<1, 2>), zeros from
//     R * ws up to a multiple of 16, and
//   * the 2R + 5 input rows 2*yo0 - 3 + t as rows of 16-bit elements e = 0 .. 6*ws + 17, e being element 6*xo0 - 9 + e of
//     the input row: nine zeros in front of and behind the image's row, zero rows outside the image.
// The GEMM is dY^T [64 n x pixels] times columns [pixels x (7 kh x 24)], column (kh, j) of pixel (ry, xl) being element
// 6*xl + j of staged row 2*ry + kh; j = 21..23 are the first values of the next pixel's window, accumulated and never
// stored, as is the eighth block of 24 that fills 168 columns up to 6 x 32.  Both operands are read with gfx950's transposing
// LDS read (8 bytes per lane, every lane its own address).  Its address must be a multiple of 8 bytes and 6*xl elements are
// a multiple of 4 bytes only, so every input row is staged TWICE, the second copy one dword to the right: even xl read the
// first copy, odd xl the second.  (The other way out, an explicit [pixel][7][24] column tile, costs 77 dword moves
// per pixel through LDS; the second copy costs the X raster's LDS writes once more and no extra pass.)
//
// The loader is register-staged and synchronous; two workgroups per CU (__launch_bounds__(256, 2), <= 64 KB of LDS
// each) overlap one's loads with the other's MFMAs.  dY: 16-byte pieces, all eight of a lane in flight at once, with the
// lane's first ten (sixteen) loads of x behind them.  X: a lane builds four
// staged dwords (elements 8m .. 8m + 7 of a row) from five aligned 4-byte loads when w is even -- the staged elements are at
// odd element offsets of the image row (6*xo0 - 9), so a staged dword is the high half of one global dword and the low half of
// the next -- and from eight 2-byte loads when w is odd, where image rows (6w bytes) are only 2-byte aligned.  Odd widths
// are served; that path is slower on the X side (77 MB against dY's 411 MB at b = 256, 224 x 224).
//
// Supported: b, h, w >= 1, n % 64 == 0, bf16 or fp16, b*h*w*max(3, n)*2 < 2^31 (32-bit element offsets).
#include <algorithm>

#include "conv_spatial.h"

namespace mrla {
namespace {

typedef c1_f32x16 sw_f32x16;

constexpr int kSwTile = 64;             // output tile: 64 n x (7 x 24 -> 192) columns
constexpr int kSwWaves = 4;             // 2 (n) x 2 (column halves); three 32 x 32 blocks per wave
constexpr int kSwBlocks = 3;
static_assert(2 * kSwBlocks * 32 >= 7 * 24, "the waves' blocks cover the 7 x 24 columns");
constexpr int kSwTarget = 2 * 256;      // workgroups: two per CU
constexpr int kSwMaxWS = 128;           // output columns of a step
constexpr int kSwMaxKP = 256;           // dY pixels of a step (32 KB): eight 16-byte pieces a lane, all in flight at once
constexpr int kSwMaxR = 16;             // output rows of a step (bounds the X raster of narrow maps)
static_assert(kSwMaxKP == 8 * 32 && kSwMaxWS <= kSwMaxKP, "the dY loader takes the tile in one pass");
static_assert(kTileRowB == kSwTile * 2, "a dY tile row is one pixel, 64 channels");
constexpr int kSwLdsCap = 64 * 1024;    // LDS of a workgroup, at most (ws = 128, R = 2: 32 KB + 9 * 3200 B)

struct SwPlan {
  int ok = 0;
  int ho = 0, wo = 0;
  int ws = 0, nseg = 0, rmax = 0;              // output columns per segment, segments per row, rows per step
  int kp_cap = 0, pd = 0, lds = 0;             // dY tile rows; dwords of ONE copy of a staged input row; LDS bytes
  int rows_per_split = 0, splits = 0, tiles = 0;
};

struct SwArgs {
  int b, h, w, ho, wo, n;
  int ws, nseg, rmax, kp_cap, pd;
  int rows_per_split, splits;
  float inv_ws, inv_runs;
};

__device__ __forceinline__ int sw_off(int row, int chunk) { return tile_off<1, 2>(row, chunk); }

// grid: (n / 64) * splits workgroups, 256 threads; LDS = kp_cap * 128 + (2 * rmax + 5) * 2 * pd * 4 bytes
template <typename T>
__global__ __launch_bounds__(kSwWaves* kWave, 2) void stem_wgrad_kernel(const T* __restrict__ dY, const T* __restrict__ X,
                                                                        float* __restrict__ part, SwArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __align__(16) unsigned char smem_raw[];
  unsigned char* const ty_tile = smem_raw;
  unsigned char* const tx_rows = smem_raw + a.kp_cap * kTileRowB;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int tiles = a.n / kSwTile;
  const int split = blockIdx.x / tiles, tn = blockIdx.x - split * tiles;
  const int n0 = tn * kSwTile;
  const int rows = a.b * a.ho;
  const int r_begin = split * a.rows_per_split, r_end = min(rows, r_begin + a.rows_per_split);
  const int copyB = a.pd * 4, rowB = 2 * copyB;             // bytes of one copy / of both copies of a staged input row

  const int wn = wave >> 1, wc = wave & 1;
  const int krel = tr_krel(lane);                           // this lane's pixel of a 16-pixel k-step (and +4)
  const int colA = tr_col(wn * 32, lane);
  const int chA = tr_chunk(colA), subA = tr_sub(colA);
  // this lane's four columns of each of its wave's three blocks: (kh, j .. j + 3), a constant byte offset from the pixel's
  // window in staged row 2*ry (the eighth block of 24 does not exist: held at kh = 6, accumulated and never stored)
  int offB[kSwBlocks];
#pragma unroll
  for (int bl = 0; bl < kSwBlocks; ++bl) {
    const int col = tr_col(32 * (kSwBlocks * wc + bl), lane);
    const int kh = min(col / 24, 6), j = col % 24;
    offB[bl] = kh * rowB + 2 * j;
  }

  sw_f32x16 acc[kSwBlocks];
#pragma unroll
  for (int t = 0; t < kSwBlocks; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  const int prow = tid >> 3, pch = tid & 7;                 // the dY loader: 32 tile rows per pass, 8 pieces a row
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  const int runs = a.pd / 4 - 1;                            // runs of four staged dwords in a row
  const bool even_w = (a.w & 1) == 0;
  const int row_el = 3 * a.w;                               // elements of an image row
  const uint32_t* const Xd = reinterpret_cast<const uint32_t*>(X);
  const unsigned short* const Xe = reinterpret_cast<const unsigned short*>(X);

  for (int r = r_begin; r < r_end;) {
    const RowStep st = row_step(r, r_end, a.ho, a.rmax);
    const int img = st.img, yo0 = st.yo0, R = st.R;
    for (int seg = 0; seg < a.nseg; ++seg) {
      const int xo0 = seg * a.ws, ws = min(a.ws, a.wo - xo0);
      // (ws < a.ws only in the ragged last segment of a row cut into segments, where R = 1: pixel p = xl under either pitch)
      const int NP = R * ws, KP = (NP + 15) & ~15;
      const int XR = 2 * R + 5;
      const int yi0 = 2 * yo0 - 3;
      __syncthreads();                                      // the previous step's reads are done
      // Every global load of the step's dY tile (KP <= kSwMaxKP = 8 x 32 tile rows: eight 16-byte pieces a lane) and of the
      // lane's first two runs of the input rows is issued before anything is written to LDS.
      // ---- dY tile: rows [0, KP) ----
      u32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int p = 32 * u + prow;
        const int ry = (int)(((float)p + 0.5f) * a.inv_ws), xl = p - ry * a.ws;
        v[u] = zero4;
        if (p < KP && ry < R && xl < ws)
          v[u] = *reinterpret_cast<const u32x4*>(dY + ((size_t)((img * a.ho + yo0 + ry) * a.wo + xo0 + xl) * a.n + n0 + pch * 8));
      }
      // ---- input rows: XR rows, both copies, staged dwords [0, 4 * runs) ----
      const int nrun = XR * runs;
      // run idx = (staged row t, dwords 4m .. 4m + 3): its global values, every load predicated on its own coordinates
      auto load_run = [&](int idx, uint32_t (&raw)[8]) {
        const int t = (int)(((float)idx + 0.5f) * a.inv_runs), m = idx - t * runs;
        const int yi = yi0 + t;
        const bool row_ok = idx < nrun && yi >= 0 && yi < a.h;
        const int row0 = (img * a.h + yi) * row_el;         // element offset of the image row (used only when row_ok)
        if (even_w) {
          // staged dword 4m + i = global dword g0 + i (high half) | global dword g0 + i + 1 (low half), both of this row
          const int g0 = 3 * xo0 - 5 + 4 * m, ndw = row_el >> 1;
#pragma unroll
          for (int i = 0; i < 5; ++i) {
            const int gi = g0 + i;
            raw[i] = 0u;
            if (row_ok && gi >= 0 && gi < ndw) raw[i] = Xd[(row0 >> 1) + gi];
          }
        } else {
          const int e0 = 6 * xo0 - 9 + 8 * m;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int ei = e0 + i;
            raw[i] = 0u;
            if (row_ok && ei >= 0 && ei < row_el) raw[i] = Xe[row0 + ei];
          }
        }
      };
      auto store_run = [&](int idx, const uint32_t (&raw)[8]) {
        if (idx >= nrun) return;
        const int t = (int)(((float)idx + 0.5f) * a.inv_runs), m = idx - t * runs;
        uint32_t d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = even_w ? (raw[i] >> 16) | (raw[i + 1] << 16) : raw[2 * i] | (raw[2 * i + 1] << 16);
        unsigned char* const ra = tx_rows + t * rowB + 16 * m;
        *reinterpret_cast<u32x4*>(ra) = u32x4{d[0], d[1], d[2], d[3]};
        uint32_t* const rb = reinterpret_cast<uint32_t*>(ra + copyB + 4);      // the second copy, one dword to the right
        rb[0] = d[0]; rb[1] = d[1]; rb[2] = d[2]; rb[3] = d[3];
      };
      constexpr int kThreadsWg = kSwWaves * kWave;
      uint32_t x0[8], x1[8];
      load_run(tid, x0);
      load_run(tid + kThreadsWg, x1);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int p = 32 * u + prow;
        if (p < KP) *reinterpret_cast<u32x4*>(ty_tile + sw_off(p, pch)) = v[u];
      }
      store_run(tid, x0);
      store_run(tid + kThreadsWg, x1);
      for (int idx = tid + 2 * kThreadsWg; idx < nrun; idx += 2 * kThreadsWg) {
        load_run(idx, x0);
        load_run(idx + kThreadsWg, x1);
        store_run(idx, x0);
        store_run(idx + kThreadsWg, x1);
      }
      __syncthreads();
      // ---- the product over the step's pixels ----
      for (int k0 = 0; k0 < KP; k0 += 16) {
        const int k = k0 + krel;
        const typename Elem16<T>::x8 fa = tr16_frag<T>(ty_tile + sw_off(k, chA) + subA, ty_tile + sw_off(k + 4, chA) + subA);
        // the window of pixel p = ry * ws + xl: staged row 2*ry, byte 12*xl (+ 4 in the second copy for odd xl).  The tail
        // behind the step's last pixel, all zeros in dY, reads the last pixel's window: written, finite numbers.
        const int p1 = min(k, NP - 1), p2 = min(k + 4, NP - 1);
        const int ry1 = (int)(((float)p1 + 0.5f) * a.inv_ws), xl1 = p1 - ry1 * a.ws;
        const int ry2 = (int)(((float)p2 + 0.5f) * a.inv_ws), xl2 = p2 - ry2 * a.ws;
        const unsigned char* const b1 = tx_rows + 2 * ry1 * rowB + 12 * xl1 + (xl1 & 1) * (copyB + 4);
        const unsigned char* const b2 = tx_rows + 2 * ry2 * rowB + 12 * xl2 + (xl2 & 1) * (copyB + 4);
#pragma unroll
        for (int bl = 0; bl < kSwBlocks; ++bl) {
          const typename Elem16<T>::x8 fb = tr16_frag<T>(b1 + offB[bl], b2 + offB[bl]);
          Elem16<T>::mfma(acc[bl], fa, fb);
        }
      }
    }
    r += R;
  }

  // ---- partial tile: D[i][j], j = lane % 32 (column) on the lane, i = 8*(e/4) + 4*(lane/32) + e%4 (n) in register e ----
  const int hh = lane >> 5;
#pragma unroll
  for (int bl = 0; bl < kSwBlocks; ++bl) {
    const int col = 32 * (kSwBlocks * wc + bl) + (lane & 31);
    const int kh = col / 24, j = col - kh * 24;
    if (kh < 7 && j < 21) {
      float* po = part + ((size_t)split * a.n + n0 + wn * 32) * 147 + kh * 21 + j;
#pragma unroll
      for (int e = 0; e < 16; ++e) po[(size_t)(8 * (e >> 2) + 4 * hh + (e & 3)) * 147] = acc[bl][e];
    }
  }
#endif
}

// A step: whole output rows where one has at most kSwMaxWS pixels -- as many as kSwMaxKP pixels hold, kSwMaxR at most --
// else segments of one row.  Splits over output rows so that the grid is two workgroups per CU where the rows allow it.
SwPlan sw_plan(int b, int n, int h, int w) {
  SwPlan p;
  if (b <= 0 || n <= 0 || h <= 0 || w <= 0 || n % kSwTile) return p;
  if ((unsigned long long)b * h * w * std::max(3, n) * 2 >= 1ull << 31) return p;
  p.ho = (h - 1) / 2 + 1;
  p.wo = (w - 1) / 2 + 1;
  if (p.wo <= kSwMaxWS) {
    p.ws = p.wo; p.nseg = 1;
    p.rmax = std::max(1, std::min(std::min(p.ho, kSwMaxR), kSwMaxKP / p.ws));
  } else {
    p.ws = kSwMaxWS; p.nseg = (p.wo + p.ws - 1) / p.ws;
    p.rmax = 1;
  }
  p.kp_cap = (p.rmax * p.ws + 15) & ~15;
  const int ew = (6 * p.ws + 18 + 7) & ~7;                 // staged elements of a row, whole runs of eight
  p.pd = ew / 2 + 4;                                       // + the second copy's shift, kept a multiple of 16 bytes
  p.lds = p.kp_cap * kTileRowB + (2 * p.rmax + 5) * 2 * p.pd * 4;
  if (p.lds > kSwLdsCap) return p;
  p.tiles = n / kSwTile;
  const long long rows = (long long)b * p.ho;
  // ... but a split is at least one full step: its five halo rows of x are loaded once per step
  const RowSplit sp = split_rows(rows, p.tiles, kSwTarget, 1, std::min<long long>(rows, p.rmax));
  p.rows_per_split = sp.per;
  p.splits = sp.count;
  p.ok = 1;
  return p;
}

template <typename T>
int sw_launch(const SwPlan& p, const SwArgs& a, const void* dy, const void* x, float* part, hipStream_t st) {
  if (lds_opt_in(reinterpret_cast<const void*>(stem_wgrad_kernel<T>), (size_t)p.lds) != hipSuccess) return MRLA_EHIP;
  hipLaunchKernelGGL((stem_wgrad_kernel<T>), dim3(p.tiles * p.splits), dim3(kSwWaves * kWave), (size_t)p.lds, st, (const T*)dy,
                     (const T*)x, part, a);
  return MRLA_OK;
}

}  // namespace

int stem_conv_wgrad_rows(int b, int n, int h, int w) {
  const SwPlan p = sw_plan(b, n, h, w);
  return p.ok ? p.splits : MRLA_EUNSUPPORTED;
}

// {tile n, output rows per split, splits, column segments per row, LDS bytes, output columns per segment, output rows per step}
int stem_conv_wgrad_plan(int b, int n, int h, int w, int* out) {
  const SwPlan p = sw_plan(b, n, h, w);
  if (!p.ok) return MRLA_EUNSUPPORTED;
  out[0] = kSwTile; out[1] = p.rows_per_split; out[2] = p.splits; out[3] = p.nseg; out[4] = p.lds; out[5] = p.ws; out[6] = p.rmax;
  return MRLA_OK;
}

int launch_stem_conv_wgrad(const void* dy, const void* x, float* part, void* dw, int dw_f32, int b, int n, int h, int w,
                           int dtype, hipStream_t st) {
  const SwPlan p = sw_plan(b, n, h, w);
  if (!p.ok || (dtype != MRLA_BF16 && dtype != MRLA_F16)) return MRLA_EUNSUPPORTED;
  SwArgs a;
  a.b = b; a.h = h; a.w = w; a.ho = p.ho; a.wo = p.wo; a.n = n;
  a.ws = p.ws; a.nseg = p.nseg; a.rmax = p.rmax; a.kp_cap = p.kp_cap; a.pd = p.pd;
  a.rows_per_split = p.rows_per_split; a.splits = p.splits;
  a.inv_ws = 1.0f / (float)p.ws; a.inv_runs = 1.0f / (float)(p.pd / 4 - 1);
  const int rc = dtype == MRLA_F16 ? sw_launch<f16_t>(p, a, dy, x, part, st) : sw_launch<bf16_t>(p, a, dy, x, part, st);
  if (rc != MRLA_OK) return rc;
  return launch_split_sum(part, dw, dw_f32, dtype, p.splits, n * 147, st);
}

}  // namespace mrla
