// Input gradient of a 3x3 convolution at stride 2 (padding 1, dilation 1, groups 1) of channels_last bf16 or fp16
// activations as an implicit GEMM on the MFMA that issues no zero taps:
//   dx[b, yi, xi, c] = round( sum_{kh, kw, n} dy[b, yo, xo, n] * wt[n, kh, kw, c] )   over yi = 2*yo + kh - 1, xi = 2*xo + kw - 1
// Reference: the backward of conv2 of the first bottleneck of stages 2-4 (resnet/models/resnet_mrla_light.py, conv3x3 of
// Bottleneck) and of the first convolution of the same basic blocks, which the reference leaves to cuDNN.
//
// Cells and parity classes.  Cell (i, j) of an image is its dX pixels (2i + ey, 2j + ex), ey, ex in {0, 1}: four parity
// classes.  Per axis an even coordinate meets tap 1 of dY row i, an odd one tap 2 of dY row i and tap 0 of dY row i + 1, so
// the classes take 1, 2, 2 and 4 of the nine taps -- 9 MFMAs per cell and k-step where the forward kernel on a zero-inserted
// dY would issue 36 -- and the nine taps read only FOUR dY positions: (i, j), (i, j+1), (i+1, j), (i+1, j+1).
//
// Ownership (conv_spatial.h): a workgroup owns 64 channels of c and a FIXED range of cell rows (cell row i of an image = its
// dX rows 2i and 2i + 1; cell rows are numbered image after image, b * ho in all).  It walks its range in steps of R cell
// rows of ONE image -- or, for rows wider than a step, column segments of one row -- and for every step sums all of n, in
// 64-chunks in ascending order, the taps of a class in one fixed order (kDgTaps), each class in an fp32 accumulator of its
// own: no split of the reduction, no atomics, no memset, every element of dx written exactly once, one rounding to nearest
// even at the store.  dx is a function of the arguments alone.
//
// Borders: the dY raster of a step sits in LDS as [pixel][64 n], dY pixel (ty, cx) of the step -- row yo0 + ty, column
// xo0 + cx -- at raster row ty*PY + cx, PY = the step's columns + 1, with one more row below the step's R.  Tap (dyo, dxo) of
// cell p = ry*PY + j is raster row p + dyo*PY + dxo: a constant offset.  The row below and the column right of the step are
// the image's own next dY row / column where it has one and zeros where it has none (NOT the next image's first row); they,
// and the tail of the raster up to the last row a tap reads, are written by the loader, whose every global load is
// predicated on the pixel's own coordinates: nothing is read outside dy or wt.  The pad column's cells, the tail's, and the
// odd row / column of a cell that lies outside an odd-sized image are computed and not stored.
//
// Operands.  B = the raster, contiguous along n (the reduction): ds_read_b128 of chunk ch of 32 consecutive raster rows,
// chunk position ch ^ ((row >> 1) & 7) as in conv3x3_fwd.hip -- the rows of a 16-lane group are consecutive, so distinct
// mod 16: conflict-free.  A = the weight in the FORWARD's layout wt[n, 3, 3, c] (no flipped or transposed copy): the
// n-chunk's tile sits in LDS as [9 taps][64 n][64 c] (72 KB), row tap*64 + nl, so consecutive n are consecutive rows and
// the tile is k-major; it is read with gfx950's transposing LDS read (tr16_frag, 4 n x 16 c per 16 lanes), chunk position
// ch ^ (((row >> 1) & 1) << 2) as in conv3x3_wgrad.hip: a 32-lane half reads 4 consecutive rows x 32 channels at rows
// k and k + 8, conflict-free.  c is the accumulator's ROW index, so a lane holds 4 consecutive channels of one dX pixel
// and stores 8 bytes.  Per k-step of 16 n and 32-cell block: 9 transposing weight reads (shared by the wave's two blocks)
// + 4 raster reads for 9 MFMAs.
//
// Four waves: 2 halves of c x 2 interleaved 32-cell blocks, at most two blocks of four class accumulators per wave (128
// accumulator registers); one workgroup per CU (72 KB of weights + at most 26 KB of raster), a synchronous register-staged
// loader; the weights are loaded once per workgroup where n = 64, per step and chunk otherwise.
#include <algorithm>

#include "conv_spatial.h"

namespace mrla {
namespace {

typedef c1_f32x16 dg_f32x16;

constexpr int kDgTile = 64;             // channels of c of a workgroup
constexpr int kDgTarget = 256;          // workgroups: one per CU
constexpr int kDgMaxKP = 128;           // cells (accumulator columns) of a step: four 32-cell blocks
constexpr int kDgMaxPY = 64;            // raster pitch: at most 63 cell columns per segment
constexpr int kDgWRows = 9 * kDgTile;   // weight rows of an n-chunk

// The nine taps in the order they are summed: class (ey, ex) = cls, weight tap kh*3 + kw, raster offset (dyo, dxo)
struct DgTap {
  int cls, tap, dyo, dxo;
};
[[maybe_unused]] constexpr DgTap kDgTaps[9] = {
    {0, 4, 0, 0},                                              // even row, even column: (1, 1)
    {1, 5, 0, 0}, {1, 3, 0, 1},                                // even row, odd column:  (1, 2), (1, 0)
    {2, 7, 0, 0}, {2, 1, 1, 0},                                // odd row, even column:  (2, 1), (0, 1)
    {3, 8, 0, 0}, {3, 6, 0, 1}, {3, 2, 1, 0}, {3, 0, 1, 1},    // odd row, odd column:   (2, 2), (2, 0), (0, 2), (0, 0)
};

struct DgPlan : Raster3x3 {
  int rows_per_wg = 0, ranges = 0, tiles = 0, rt_cap = 0;
};

struct DgArgs {
  int b, h, w, ho, wo, c, n;
  int py, ws, nseg, rmax;
  int rows_per_wg;
  float inv_py;
};

__device__ __forceinline__ int dg_roff(int row, int chunk) { return tile_off<7, 0>(row, chunk); }      // the raster
__device__ __forceinline__ int dg_woff(int row, int chunk) { return tile_off<1, 2>(row, chunk); }      // the weights

// grid: (c / 64) * ranges workgroups, 256 threads; LDS = (576 + rt_cap) * 128 bytes
template <typename T>
__global__ __launch_bounds__(kThreads, 1) void conv3x3_dgrad_s2_kernel(const T* __restrict__ dY, const T* __restrict__ W,
                                                                       T* __restrict__ dX, DgArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef typename Elem16<T>::x8 x8;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  unsigned char* const w_tile = smem_raw;
  unsigned char* const r_tile = w_tile + kDgWRows * kTileRowB;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int tiles_c = a.c / kDgTile;
  const int range = blockIdx.x / tiles_c, c0 = (blockIdx.x - range * tiles_c) * kDgTile;
  const int rows = a.b * a.ho;
  const int r_begin = range * a.rows_per_wg, r_end = min(rows, r_begin + a.rows_per_wg);
  const int PY = a.py;
  const int chunks = a.n / kDgTile;

  const int wc = wave & 1, wp = wave >> 1;                 // this wave's half of c, and its cell blocks wp, wp + 2
  const int l31 = lane & 31, hh = lane >> 5;
  const int prow = tid >> 3, pch = tid & 7;                // the loader: 32 LDS rows per pass, 8 pieces a row
  const u32x4 zero4 = {0u, 0u, 0u, 0u};

  // the lane's place in the transposing read of a weight k-step: n row krel (and 4 on), 4 of the wave's 32 channels
  const int krel = tr_krel(lane), colA = tr_col(wc * 32, lane);
  const int wlo = dg_woff(krel, tr_chunk(colA)) + tr_sub(colA);           // (the swizzle sees bit 1 of the row: krel's, as
  const int whi = dg_woff(krel + 4, tr_chunk(colA)) + tr_sub(colA);       // every tap and k-step begins at a multiple of 16)

  bool first = true;

  for (int r = r_begin; r < r_end;) {
    const RowStep st = row_step(r, r_end, a.ho, a.rmax);
    const int img = st.img, yo0 = st.yo0, R = st.R;
    for (int seg = 0; seg < a.nseg; ++seg) {
      const int xo0 = seg * a.ws, ws = min(a.ws, a.wo - xo0);
      const int KP = (R * PY + 31) & ~31;
      const int RT = KP + PY + 1;                           // raster rows some tap of this step reads

      // this lane's cell of its two blocks, and where its four dX pixels go
      bool act[2], real[2];
      int yi[2], xi[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int p = (wp + 2 * i) * 32 + l31;
        const int ry = (int)(((float)p + 0.5f) * a.inv_py), j = p - ry * PY;
        act[i] = (wp + 2 * i) * 32 < KP;
        real[i] = act[i] && ry < R && j < ws;
        yi[i] = 2 * (yo0 + ry);
        xi[i] = 2 * (xo0 + j);
      }

      dg_f32x16 acc[2][4];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][q][e] = 0.f;

      for (int nc = 0; nc < chunks; ++nc) {
        __syncthreads();                                    // the previous chunk's reads are done
        // ---- weights of the chunk: global row q = nl * 9 + tap -> LDS row tap * 64 + nl ----
        if (chunks > 1 || first) {
          const T* wsrc = W + (size_t)nc * kDgTile * 9 * a.c + c0 + pch * 8;
#pragma unroll 1
          for (int q0 = 0; q0 < kDgWRows; q0 += 192) {
            u32x4 v[6];
#pragma unroll
            for (int u = 0; u < 6; ++u) v[u] = *reinterpret_cast<const u32x4*>(wsrc + (size_t)(q0 + 32 * u + prow) * a.c);
#pragma unroll
            for (int u = 0; u < 6; ++u) {
              const int q = q0 + 32 * u + prow, nl = q / 9, tap = q - nl * 9;
              *reinterpret_cast<u32x4*>(w_tile + dg_woff(tap * kDgTile + nl, pch)) = v[u];
            }
          }
        }
        // ---- dY raster of the chunk: rows [0, RT) ----
        for (int t0 = 0; t0 < RT; t0 += 128) {
          u32x4 v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int t = t0 + 32 * u + prow;
            const int ty = (int)(((float)t + 0.5f) * a.inv_py), cx = t - ty * PY;
            const int yo = yo0 + ty, xo = xo0 + cx;
            v[u] = zero4;
            if (t < RT && ty <= R && cx <= ws && yo < a.ho && xo < a.wo)
              v[u] = *reinterpret_cast<const u32x4*>(dY + ((size_t)((img * a.ho + yo) * a.wo + xo) * a.n + nc * kDgTile + pch * 8));
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int t = t0 + 32 * u + prow;
            if (t < RT) *reinterpret_cast<u32x4*>(r_tile + dg_roff(t, pch)) = v[u];
          }
        }
        __syncthreads();
        // ---- four k-steps of 16 n x nine taps ----
        if (act[0]) {                                       // (wave-uniform: the transposing reads run with every lane on)
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const int ch = 2 * kk + hh;
            x8 fb[2][4];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
              const int roff = (o >> 1) * PY + (o & 1);
              fb[0][o] = *reinterpret_cast<const x8*>(r_tile + dg_roff(wp * 32 + l31 + roff, ch));
              if (act[1]) fb[1][o] = *reinterpret_cast<const x8*>(r_tile + dg_roff((wp + 2) * 32 + l31 + roff, ch));
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
              const int wbase = (kDgTaps[t].tap * kDgTile + 16 * kk) * kTileRowB;
              const x8 fa = tr16_frag<T>(w_tile + wbase + wlo, w_tile + wbase + whi);
              const int o = kDgTaps[t].dyo * 2 + kDgTaps[t].dxo;
              Elem16<T>::mfma(acc[0][kDgTaps[t].cls], fa, fb[0][o]);
              if (act[1]) Elem16<T>::mfma(acc[1][kDgTaps[t].cls], fa, fb[1][o]);
            }
          }
        }
        first = false;
      }

      // ---- D[i][j]: j = lane % 32 (cell) on the lane, i = 8*(e/4) + 4*(lane/32) + e%4 (c) in register e ----
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (real[i]) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int y = yi[i] + (q >> 1), x = xi[i] + (q & 1);
            if (y < a.h && x < a.w) {
              T* dst = dX + ((size_t)((img * a.h + y) * a.w + x) * a.c + c0 + wc * 32 + 4 * hh);
#pragma unroll
              for (int g = 0; g < 4; ++g) {
                uint2 o;
                o.x = Elem16<T>::pack(acc[i][q][4 * g], acc[i][q][4 * g + 1]);
                o.y = Elem16<T>::pack(acc[i][q][4 * g + 2], acc[i][q][4 * g + 3]);
                *reinterpret_cast<uint2*>(dst + 8 * g) = o;
              }
            }
          }
        }
    }
    r += R;
  }
#endif
}

size_t dg_lds_bytes(const DgPlan& p) { return (size_t)(kDgWRows + p.rt_cap) * kTileRowB; }

// conv_spatial.h's stride-2 raster of dY (pitch = the step's columns + the pad column; cells in whole 32-cell blocks) with
// one more row below it, and ranges of cell rows so that the grid is one workgroup per CU.
DgPlan dg_plan(int b, int c, int n, int h, int w) {
  DgPlan p;
  static_cast<Raster3x3&>(p) = raster3x3(b, c, n, h, w, 2, kDgMaxKP, kDgMaxKP, kDgMaxPY, 32);
  if (!p.ok) return p;
  p.tiles = c / kDgTile;
  p.rt_cap = (p.kp_cap + p.py + 1 + 7) & ~7;
  // where n = 64 the weights (72 KB) are loaded once per workgroup: at least two full steps behind them
  const RowSplit sp = split_rows((long long)b * p.ho, p.tiles, kDgTarget, (n == kDgTile ? 2 : 1) * p.rmax);
  p.rows_per_wg = sp.per;
  p.ranges = sp.count;
  p.ok = dg_lds_bytes(p) <= 160 * 1024;                     // (at most 72 + 25 KB by the caps above)
  return p;
}

template <typename T>
int dg_launch(const DgPlan& p, const DgArgs& a, const void* dy, const void* wt, void* dx, hipStream_t st) {
  const size_t lds = dg_lds_bytes(p);
  if (lds_opt_in(reinterpret_cast<const void*>(conv3x3_dgrad_s2_kernel<T>), lds) != hipSuccess) return MRLA_EHIP;
  hipLaunchKernelGGL((conv3x3_dgrad_s2_kernel<T>), dim3(p.tiles * p.ranges), dim3(kThreads), lds, st, (const T*)dy, (const T*)wt,
                     (T*)dx, a);
  return hip_status(hipGetLastError());
}

}  // namespace

// {tile c, cell rows per workgroup range, cell rows per step, column segments per row, ranges, workgroups}
int conv3x3_dgrad_s2_plan(int b, int c, int n, int h, int w, int* out) {
  const DgPlan p = dg_plan(b, c, n, h, w);
  if (!p.ok) return MRLA_EUNSUPPORTED;
  out[0] = kDgTile; out[1] = p.rows_per_wg; out[2] = p.rmax; out[3] = p.nseg; out[4] = p.ranges; out[5] = p.tiles * p.ranges;
  return MRLA_OK;
}

int launch_conv3x3_dgrad_s2(const void* dy, const void* wt, void* dx, int b, int c, int n, int h, int w, int dtype,
                            hipStream_t st) {
  const DgPlan p = dg_plan(b, c, n, h, w);
  if (!p.ok || (dtype != MRLA_BF16 && dtype != MRLA_F16)) return MRLA_EUNSUPPORTED;
  DgArgs a;
  a.b = b; a.h = h; a.w = w; a.ho = p.ho; a.wo = p.wo; a.c = c; a.n = n;
  a.py = p.py; a.ws = p.ws; a.nseg = p.nseg; a.rmax = p.rmax;
  a.rows_per_wg = p.rows_per_wg;
  a.inv_py = 1.0f / (float)p.py;
  return dtype == MRLA_F16 ? dg_launch<f16_t>(p, a, dy, wt, dx, st) : dg_launch<bf16_t>(p, a, dy, wt, dx, st);
}

}  // namespace mrla
