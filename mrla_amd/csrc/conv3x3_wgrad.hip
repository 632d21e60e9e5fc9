// Weight gradient of a 3x3 convolution (padding 1, dilation 1, groups 1, stride s = 1 or 2) of channels_last bf16 or fp16
// activations as nine split-pixel MFMA products that share the dY operand:
//   dW[n, kh, kw, c] = sum_{b, y, x} dY[b, y, x, n] * X[b, y*s + kh - 1, x*s + kw - 1, c]
// Reference: the backward of the bottleneck's conv2 (resnet/models/resnet_mrla_light.py, conv3x3 of Bottleneck), of both
// 3x3 convolutions of the basic block, and of the same blocks in the mmdet backbone; the reference leaves it to cuDNN.
//
// The stock library's split-K solver for this gradient accumulates with atomics into a zero-filled buffer: not
// reproducible from run to run, and wrong from the second replay of a captured graph at small batches.  Here, as in
// conv1x1_wgrad.hip, a workgroup owns one output tile (64 n x 64 c x all nine taps: 144 accumulator registers per lane) and
// a FIXED range of output rows (a row = one image row of dY; rows are numbered image after image); it writes its fp32 partial
// tile to part[split][n][9][c] and a second kernel sums the splits in ascending order.  No atomics, no memset; every element
// of part and dw is written exactly once per call, and the result is a function of the inputs and the shape alone.
//
// Borders without per-lane masks: conv_spatial.h's rasters.  A step keeps both operands in LDS as padded rasters, dY pixel
// (ry, j) at tile row ry*PY + j and X pixel (ty, cx) at tile row ty*PX + cx, so a tap is a constant offset from a row the lane
// computes once per k-step.  The pad columns of dY and its tail up to a multiple of 16 pixels are written as zeros by a loader
// predicated like the X raster's: nothing is read outside x or dy.  The pad pixels of dY multiply into nothing (9/7 of the
// MFMA work at a 7x7 map).
//
// The loader is register-staged (16-byte pieces) and runs ONE STEP AHEAD of the products: the global loads of step i + 1 -- the
// dY raster and, at stride 1, the whole X raster (12 pieces, 48 registers); at stride 2 the dY raster and the first 128 rows of
// the X raster (7 pieces), the rest of it synchronously as before, four pieces in flight -- are issued before the k-loop of
// step i and stay outstanding across it; behind the k-loop come the barrier, the LDS writes (the compiler's vmcnt wait stands
// in front of them, none in front of the first MFMA: checked in the ISA), the barrier, the next k-loop.  One LDS stage, as
// before: the overlap is in registers (252 / 240 VGPRs at stride 1 / 2, no scratch, two waves per SIMD).  Two workgroups per CU
// (__launch_bounds__(256, 2), <= 80 KB of LDS each) still overlap one's LDS writes with the other's MFMAs.  The arithmetic --
// steps, k-steps, the nine taps and their order -- is what it was with the synchronous loader: part and dw are bit-equal to it
// (scripts/conv3x3_wgrad_against_build.py).  profiles/conv3x3_wgrad.md section 7 has what it bought.  Both MFMA operands are COLUMNS
// of the pixel-major tiles, read with gfx950's transposing LDS read (4 pixels x 16 channels per 16 lanes, every lane its own
// address -- which is what lets the X operand step by s pixels); 16-byte chunk ch of tile row r sits at chunk position
// ch ^ (((r >> 1) & 1) << 2) (conv1x1_wgrad.hip's swizzle for 128-byte rows): conflict-free at stride 1, two-way on the X
// raster at stride 2, whose half-wave reads every other row.  (Swapping rows 4..7 of every eight in pairs on top of it, which
// by the bank rule spreads those four rows over the whole bank row, was measured: 12 - 18 % SLOWER at the three stride-2
// shapes of ResNet-50, the stride-1 shapes unchanged; profiles/conv3x3_wgrad.md.  Not kept, the cause not established.)
#include <algorithm>
#include <type_traits>

#include "conv_spatial.h"

namespace mrla {
namespace {

typedef c1_f32x16 c3_f32x16;

constexpr int kC3Tile = 64;             // output tile: 64 n x 64 c (x 9 taps)
constexpr int kC3Waves = 4;             // 2 x 2 waves, a 32 x 32 block of each tap per wave
constexpr int kC3Stages = 1;            // LDS stages: the next step's pieces wait in registers, not in a second stage
constexpr int kC3Target = 2 * 256;      // workgroups: two per CU (the sibling's CU count)
constexpr int kC3MaxKP1 = 128;          // dY raster rows of a step at stride 1: (128 + 128 + 2*60 + 3) * 128 B = 48 KB at most
constexpr int kC3MaxKP2 = 96;           // ... at stride 2, where the X raster has four times the pixels: (96 + 4*96 + 2*48 + 3 + 7)
                                        // * 128 B = 74 KB at most (c3_plan's xt_cap with py * rmax <= 96, py <= 48 where rmax >= 2)
constexpr int kC3MaxPY = 60;            // dY raster pitch
static_assert(kTileRowB == kC3Tile * 2, "a tile row is one pixel, 64 channels");

struct C3Plan : Raster3x3 {
  int rows_per_split = 0, splits = 0, tiles = 0;
};

struct C3Args {
  int b, h, w, ho, wo, c, n;
  int py, ws, nseg, rmax, kp_cap;
  int rows_per_split, splits, tiles_c;
  float inv_py, inv_px;
};

__device__ __forceinline__ int c3_off(int row, int chunk) { return tile_off<1, 2>(row, chunk); }

// 32x32x16 operand: this lane's 4 channels (of the 16-lane group's 16) of tile rows r and r2, its pixel of the k-step's first
// and second eight
template <typename T>
__device__ __forceinline__ typename Elem16<T>::x8 c3_frag(const unsigned char* tile, int r, int r2, int chunk, int sub) {
  return tr16_frag<T>(tile + c3_off(r, chunk) + sub, tile + c3_off(r2, chunk) + sub);
}

// grid: tiles * splits workgroups, 256 threads; LDS = (kp_cap + xt_cap) * 128 bytes
template <typename T, int S>
__device__ __forceinline__ void conv3x3_wgrad_body(const T* __restrict__ dY, const T* __restrict__ X, float* __restrict__ part,
                                                   const C3Args& a) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __align__(16) unsigned char smem_raw[];
  unsigned char* const ty_tile = smem_raw;
  unsigned char* const tx_tile = smem_raw + a.kp_cap * kTileRowB;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int tiles = (a.n / kC3Tile) * a.tiles_c;
  const int split = blockIdx.x / tiles, tile = blockIdx.x - split * tiles;
  const int tn = tile / a.tiles_c, tc = tile - tn * a.tiles_c;
  const int n0 = tn * kC3Tile, c0 = tc * kC3Tile;
  const int rows = a.b * a.ho;
  const int r_begin = split * a.rows_per_split, r_end = min(rows, r_begin + a.rows_per_split);
  const int PY = a.py, PX = S * a.py;
  // The loader's registers: the dY raster is one pass of 32 * kYPieces tile rows, and kPreX passes of 128 rows of the X raster
  // are fetched a step ahead -- all of it at stride 1 (kXAllPre), where a later pass does not exist
  constexpr int kYPieces = S == 1 ? 4 : 3, kPreX = S == 1 ? 2 : 1;
  constexpr bool kXAllPre = S == 1;
  static_assert(kC3MaxKP1 <= 128 && kC3MaxKP2 <= 96, "the dY raster of a step is one pass of the loader");
  static_assert(kC3MaxKP1 + 2 * kC3MaxPY + 3 <= 256, "the X raster of a stride-1 step is two passes of the loader");

  const int wn = wave >> 1, wc = wave & 1;
  // (tr_krel, tr_col, tr_chunk and tr_sub of conv_spatial.h written out: through the helpers this kernel's prologue comes out
  // in another order)
  const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  const int krel = 8 * (g >> 1) + q;                       // this lane's pixel of a 16-pixel k-step (and +4)
  const int colA = wn * 32 + 16 * (g & 1) + 4 * pp, colB = wc * 32 + 16 * (g & 1) + 4 * pp;
  const int chA = colA >> 3, subA = ((colA >> 2) & 1) * 8, chB = colB >> 3, subB = ((colB >> 2) & 1) * 8;

  c3_f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  const int prow = tid >> 3, pch = tid & 7;                // the loader: 32 tile rows per pass, 8 pieces a row
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  // (32-bit byte offsets from the uniform bases: the planner refuses tensors of 2^31 bytes, and a lane's address is one register)
  const unsigned char* const dYb = reinterpret_cast<const unsigned char*>(dY);
  const unsigned char* const Xb = reinterpret_cast<const unsigned char*>(X);

  // The walk over (step, column segment), one ahead of the products: the geometry of a segment of the step at row r
  struct Seg {
    int r, seg, img, yo0, R, xo0, ws;
  };
  auto seg_at = [&](int r, int seg) {
    const RowStep st = row_step(r, r_end, a.ho, a.rmax);
    Seg g;
    g.r = r; g.seg = seg; g.img = st.img; g.yo0 = st.yo0; g.R = st.R;
    g.xo0 = seg * a.ws; g.ws = min(a.ws, a.wo - g.xo0);
    return g;
  };
  // The pieces of the dY raster (one pass: KP <= 128) and of pass `pass` of the X raster, every load predicated on its own
  // pixel, zeros elsewhere.  The pixel coordinates are computed behind the test against the raster's end, where a group of 32
  // tile rows that no lane needs costs a compare and a branch (at a 7x7 map five of the twelve groups exist), and from a row
  // number that is opaque to the optimiser: as loop invariants the coordinates of the twelve pieces are hoisted out of the
  // step loop and then spilled around the products -- recomputing them is four instructions a piece
  auto load_y = [&](const Seg& g, u32x4 (&v)[kYPieces]) {
    const int KP = (g.R * PY + 15) & ~15;
#pragma unroll
    for (int u = 0; u < kYPieces; ++u) {
      int p = 32 * u + prow;
      v[u] = zero4;
      if (p < KP) {
        asm volatile("" : "+v"(p));
        const int ry = (int)(((float)p + 0.5f) * a.inv_py), j = p - ry * PY;
        if (ry < g.R && j < g.ws)
          v[u] = *reinterpret_cast<const u32x4*>(dYb + 2u * (unsigned)(((g.img * a.ho + g.yo0 + ry) * a.wo + g.xo0 + j) * a.n + n0 + pch * 8));
      }
    }
  };
  auto load_x = [&](const Seg& g, int pass, u32x4 (&v)[4]) {
    const int KP = (g.R * PY + 15) & ~15;
    const int XT = S * KP + S * (S - 1) * PY * (g.R - 1) + 2 * PX + 3;
    const int ty_need = S * (g.R - 1) + 3, cx_need = S * (g.ws - 1) + 3;    // X raster rows / columns some tap of this step reads
    const int yi0 = g.yo0 * S - 1, xi0 = g.xo0 * S - 1;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int t = 128 * pass + 32 * u + prow;
      v[u] = zero4;
      if (t < XT) {
        asm volatile("" : "+v"(t));
        const int ty = (int)(((float)t + 0.5f) * a.inv_px), cx = t - ty * PX;
        const int yi = yi0 + ty, xi = xi0 + cx;
        if (ty < ty_need && cx < cx_need && yi >= 0 && yi < a.h && xi >= 0 && xi < a.w)
          v[u] = *reinterpret_cast<const u32x4*>(Xb + 2u * (unsigned)(((g.img * a.h + yi) * a.w + xi) * a.c + c0 + pch * 8));
      }
    }
  };
  auto store_x = [&](int XT, int pass, const u32x4 (&v)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = 128 * pass + 32 * u + prow;
      if (t < XT) *reinterpret_cast<u32x4*>(tx_tile + c3_off(t, pch)) = v[u];
    }
  };

  u32x4 vy[kYPieces], vx[kPreX > 0 ? kPreX : 1][4];        // the prefetched pieces of the step to come
  Seg cur = seg_at(r_begin, 0);
  bool more = r_begin < r_end;                              // (the planner leaves no range empty)
  if (more) {
    load_y(cur, vy);
#pragma unroll
    for (int i = 0; i < kPreX; ++i) load_x(cur, i, vx[i]);
  }
  while (more) {
    const int R = cur.R;
    const int KP = (R * PY + 15) & ~15;
    const int XT = S * KP + S * (S - 1) * PY * (R - 1) + 2 * PX + 3;
    __syncthreads();                                        // the previous step's reads are done
    // ---- dY raster: rows [0, KP); X raster: rows [0, XT), the prefetched passes, then the rest synchronously ----
#pragma unroll
    for (int u = 0; u < kYPieces; ++u) {
      const int p = 32 * u + prow;
      if (p < KP) *reinterpret_cast<u32x4*>(ty_tile + c3_off(p, pch)) = vy[u];
    }
#pragma unroll
    for (int i = 0; i < kPreX; ++i) store_x(XT, i, vx[i]);
    if (!kXAllPre)
      for (int pass = kPreX; pass * 128 < XT; ++pass) {
        u32x4 v[4];
        load_x(cur, pass, v);
        store_x(XT, pass, v);
      }
    __syncthreads();
    // ---- the next step's loads go out under this step's products ----
    Seg nxt = cur;
    more = cur.seg + 1 < a.nseg || cur.r + R < r_end;
    if (more) {
      nxt = cur.seg + 1 < a.nseg ? seg_at(cur.r, cur.seg + 1) : seg_at(cur.r + R, 0);
      load_y(nxt, vy);
#pragma unroll
      for (int i = 0; i < kPreX; ++i) load_x(nxt, i, vx[i]);
    }
    // ---- nine products over the step's pixels ----
    for (int k0 = 0; k0 < KP; k0 += 16) {
      const int k = k0 + krel;
      const typename Elem16<T>::x8 fa = c3_frag<T>(ty_tile, k, k + 4, chA, subA);
      // the X raster row of dY raster row p = ry*PY + j under tap (0, 0): (S*ry)*PX + S*j = S*p + S*(S-1)*PY*ry (the tail
      // behind the step's last row, all zeros in dY, stays inside the raster with ry held at R - 1)
      int xr = S * k, xr2 = S * (k + 4);
      if (S > 1) {
        xr += S * (S - 1) * PY * min((int)(((float)k + 0.5f) * a.inv_py), R - 1);
        xr2 += S * (S - 1) * PY * min((int)(((float)k + 4.5f) * a.inv_py), R - 1);
      }
      if constexpr (S == 1) {
        // the X operand of tap t + 1 is read while tap t multiplies: 5 - 7 % of the kernel at the ResNet-50 shapes (at stride
        // 2, where those reads are two-way bank-conflicted, the same order measured 2 - 4 % SLOWER: the loop below stays)
        typename Elem16<T>::x8 fb = c3_frag<T>(tx_tile, xr, xr2, chB, subB);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          typename Elem16<T>::x8 fbn = fb;
          if (t < 8) {
            const int off = ((t + 1) / 3) * PX + (t + 1) % 3;
            fbn = c3_frag<T>(tx_tile, xr + off, xr2 + off, chB, subB);
          }
          Elem16<T>::mfma(acc[t], fa, fb);
          fb = fbn;
        }
      } else {
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const typename Elem16<T>::x8 fb = c3_frag<T>(tx_tile, xr + kh * PX + kw, xr2 + kh * PX + kw, chB, subB);
            Elem16<T>::mfma(acc[kh * 3 + kw], fa, fb);
          }
      }
    }
    cur = nxt;
  }

  // ---- partial tile: D[i][j], j = lane % 32 (c) on the lane, i = 8*(e/4) + 4*(lane/32) + e%4 (n) in register e ----
  float* po = part + (((size_t)split * a.n + n0 + wn * 32) * 9) * a.c + c0 + wc * 32 + (lane & 31);
  const int hh = lane >> 5;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) po[((size_t)(8 * (e >> 2) + 4 * hh + (e & 3)) * 9 + t) * a.c] = acc[t][e];
#endif
}

template <typename T, int S>
__global__ __launch_bounds__(kC3Waves* kWave, 2) void conv3x3_wgrad_kernel(const T* __restrict__ dY, const T* __restrict__ X,
                                                                           float* __restrict__ part, C3Args a) {
  conv3x3_wgrad_body<T, S>(dY, X, part, a);
}

// conv_spatial.h's raster of a step, and splits over output rows so that the grid is two workgroups per CU.
C3Plan c3_plan(int b, int c, int n, int h, int w, int s) {
  C3Plan p;
  static_cast<Raster3x3&>(p) = raster3x3(b, c, n, h, w, s, kC3MaxKP1, kC3MaxKP2, kC3MaxPY, 16);
  if (!p.ok) return p;
  p.tiles = (n / kC3Tile) * (c / kC3Tile);
  const RowSplit sp = split_rows((long long)b * p.ho, p.tiles, kC3Target);
  p.rows_per_split = sp.per;
  p.splits = sp.count;
  return p;
}

template <typename T, int S>
int c3_launch(const C3Plan& p, const C3Args& a, const void* dy, const void* x, float* part, hipStream_t st) {
  const size_t lds = (size_t)(p.kp_cap + p.xt_cap) * kTileRowB;
  if (lds > 80 * 1024) return MRLA_EUNSUPPORTED;
  if (lds_opt_in(reinterpret_cast<const void*>(conv3x3_wgrad_kernel<T, S>), lds) != hipSuccess) return MRLA_EHIP;
  hipLaunchKernelGGL((conv3x3_wgrad_kernel<T, S>), dim3(p.tiles * p.splits), dim3(kC3Waves * kWave), lds, st, (const T*)dy,
                     (const T*)x, part, a);
  return MRLA_OK;
}

}  // namespace

int conv3x3_wgrad_rows(int b, int c, int n, int h, int w, int s) {
  const C3Plan p = c3_plan(b, c, n, h, w, s);
  return p.ok ? p.splits : MRLA_EUNSUPPORTED;
}

// {tile n, tile c, output rows per split, LDS stages, splits, output tiles}
int conv3x3_wgrad_plan(int b, int c, int n, int h, int w, int s, int* out) {
  const C3Plan p = c3_plan(b, c, n, h, w, s);
  if (!p.ok) return MRLA_EUNSUPPORTED;
  out[0] = kC3Tile; out[1] = kC3Tile; out[2] = p.rows_per_split; out[3] = kC3Stages; out[4] = p.splits; out[5] = p.tiles;
  return MRLA_OK;
}

// 1 where the kernel and its reduction are expected to take less device time than everything the stock operator launches for
// this gradient.  profiles/conv3x3_wgrad.md section 7: both sides carry a fixed cost of about the same size (the reduction of
// splits * n * 9 * c fp32 here, a zero-fill and two casts there), so it is kernel against solver, and the kernel -- a prologue
// whose loads nothing hides, 144 KB of partial tile per workgroup to store -- needs work to spread those over.  At stride 1 it
// won at every measured shape with kC3PreferPixels output pixels per split (three full rasters) or more, which came with
// kC3PreferSteps steps per workgroup or more; with 196 - 224 pixels (2 - 4 steps) the two sides were level, below that the
// solver won.  At stride 2, where the loader fetches only the first pass of the X raster ahead, no class won measurably.
constexpr int kC3PreferSteps = 4, kC3PreferPixels = 384;
int conv3x3_wgrad_preferred(int b, int c, int n, int h, int w, int s) {
  const C3Plan p = c3_plan(b, c, n, h, w, s);
  if (!p.ok) return MRLA_EUNSUPPORTED;
  const long long steps = (long long)((p.rows_per_split + p.rmax - 1) / p.rmax) * p.nseg;
  const long long pixels = (long long)p.rows_per_split * p.wo;
  return s == 1 && steps >= kC3PreferSteps && pixels >= kC3PreferPixels;
}

// 1 where the stride-1 input gradient is expected to take less device time as the stock FORWARD convolution of dy with the
// flipped, transposed weight (mrla_conv3x3_weight_bank_refresh keeps that weight) than as the stock backward-data solver with
// the zero-fill of dX in front of it.  profiles/conv3x3_dgrad_flip.md section 1: the forward solver wins by 9 - 35 us a launch
// once the launch has work enough -- in the plan's quantities the multiply-adds b * h * w * 9 * c * n, the same number for
// every stage of a ResNet at one batch -- and the zero-fill it saves grows with the bytes of dX; what the route costs is a
// share (1.1 us) of one refresh launch.  Measured with c == n only (every stride-1 3x3 convolution of the networks), where the
// forward problem is the layer's own forward and the stock library has its solver chosen already: nothing else is routed.
// kFlipMinMacs is the class of 224 x 224 images at batch 96: from there on every width won by more than twice the run-to-run
// spread at every measured batch (96, 128, 256).  Batch 64 won as well and batch 32 at three widths of four (512 channels on
// 7 x 7 lost by 1.8 us); they stay with the stock gradient, as do the two-image detection shapes (5e9 multiply-adds, won by
// 7 - 15 us), which a rule in this one quantity cannot tell from a batch-43 step.
constexpr long long kFlipMinMacs = 96LL * 56 * 56 * 9 * 64 * 64;
int conv3x3_dgrad_flip_preferred(int b, int c, int n, int h, int w) {
  if (c != n || c % 64) return 0;
  return (double)b * h * w * 9.0 * c * n >= (double)kFlipMinMacs;       // (double: no overflow for any int arguments)
}

int launch_conv3x3_wgrad(const void* dy, const void* x, float* part, void* dw, int dw_f32, int b, int c, int n, int h, int w,
                         int s, int dtype, hipStream_t st) {
  const C3Plan p = c3_plan(b, c, n, h, w, s);
  if (!p.ok || (dtype != MRLA_BF16 && dtype != MRLA_F16)) return MRLA_EUNSUPPORTED;
  C3Args a;
  a.b = b; a.h = h; a.w = w; a.ho = p.ho; a.wo = p.wo; a.c = c; a.n = n;
  a.py = p.py; a.ws = p.ws; a.nseg = p.nseg; a.rmax = p.rmax; a.kp_cap = p.kp_cap;
  a.rows_per_split = p.rows_per_split; a.splits = p.splits; a.tiles_c = c / kC3Tile;
  a.inv_py = 1.0f / (float)p.py; a.inv_px = 1.0f / (float)(s * p.py);
  int rc;
  if (dtype == MRLA_F16)
    rc = s == 1 ? c3_launch<f16_t, 1>(p, a, dy, x, part, st) : c3_launch<f16_t, 2>(p, a, dy, x, part, st);
  else
    rc = s == 1 ? c3_launch<bf16_t, 1>(p, a, dy, x, part, st) : c3_launch<bf16_t, 2>(p, a, dy, x, part, st);
  if (rc != MRLA_OK) return rc;
  return launch_split_sum(part, dw, dw_f32, dtype, p.splits, n * 9 * c, st);
}

}  // namespace mrla
