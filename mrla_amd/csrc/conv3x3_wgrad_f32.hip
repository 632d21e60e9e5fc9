// Weight gradient of a 3x3 convolution (padding 1, dilation 1, groups 1, stride s = 1 or 2) of channels_last FP32 activations
// on the exact fp32-input MFMA (v_mfma_f32_32x32x2_f32: bitwise a chain of fmaf), for the recipe that trains without autocast:
//   dW[n, kh, kw, c] = sum_{b, y, x} dY[b, y, x, n] * X[b, y*s + kh - 1, x*s + kw - 1, c]
// Reference: resnet/train.py trains in fp32; there the backward of every 3x3 convolution of the bottleneck and of the basic block
// is the stock library's, whose split-K solver for this gradient accumulates with atomics into a zero-filled buffer.
//
// The ownership model is conv3x3_wgrad.hip's, with which this file shares nothing but conv_spatial.h: a workgroup owns one
// output tile (64 n x 64 c x all nine taps: 144 accumulator registers per lane) and a FIXED range of output rows; it writes its
// fp32 partial tile to part[split][n][9][c], and split_sum_kernel<float> sums the splits in ascending order.  No atomics, no
// memset; every element of part and dw is written exactly once per call, nothing is read outside x and dy, and the result is a
// function of the arguments alone.
//
// Borders without per-lane masks: conv_spatial.h's rasters, dY pixel (ry, j) at tile row ry*PY + j and X pixel (ty, cx) at
// tile row ty*PX + cx (PX = s*PY), the pad columns, the rows outside the image and the tails written as zeros by a loader
// whose every global load is predicated on its own pixel.
//
// The operand path.  The instruction takes ONE f32 per lane and operand; its reduction index k (two per instruction, lane l
// holds k = l >> 5) is the pixel, and both operands are channel-contiguous in a tile row, so a lane's operand is one f32 of a
// raster row read with ds_read_b32: lane half h takes raster pixel p = k0 + h of dY and the X row of that pixel under the tap,
// s*p + s*(s-1)*PY*ry + kh*PX + kw.  No transposition anywhere.  The nine tap accumulators are independent, so the 64-cycle
// dependent-accumulator latency of the instruction is covered by the eight other taps.
//
// The choices, none of them measured against its alternative (profiles/conv3x3_wgrad_f32.md has what was measured):
//   * tile 64 n x 64 c x 9 with 256-byte raster rows (64 fp32 channels of one pixel); 2 x 2 waves, 32 x 32 of each tap a wave;
//   * NO LDS swizzle: ds_read_b32 is served per 32-lane half with bank = (a / 4) % 32, and a half reads 128 contiguous bytes
//     of one row; the loader's ds_write_b128 is served per 8 lanes, which write 128 contiguous bytes: both conflict-free on
//     the plain image;
//   * rasters of at most 64 (stride 1) / 48 (stride 2) dY pixels a step and a pitch of at most 60: at most 66 KB of LDS at
//     stride 1; at stride 2 57 - 70 KB at ResNet's maps and up to 113 KB where one output row is wider than 29 pixels;
//   * the loader runs NO step ahead: a step's rasters are fetched (four 16-byte pieces a lane in flight) between two barriers.
//     What hides it is the other workgroup of the CU -- two per CU (__launch_bounds__(256, 2)) wherever the rasters take at
//     most 80 KB; above that a CU holds one workgroup and the loads are exposed;
//   * the operands of k-step i + 1 (ten LDS reads) are read into registers in front of the nine MFMAs of k-step i.
#include <algorithm>

#include "conv_spatial.h"

namespace mrla {
namespace {

typedef c1_f32x16 c3f_f32x16;

constexpr int kC3fTile = 64;            // output tile: 64 n x 64 c (x 9 taps)
constexpr int kC3fWaves = 4;            // 2 x 2 waves, a 32 x 32 block of each tap per wave
constexpr int kC3fStages = 1;           // LDS stages
constexpr int kC3fTarget = 2 * 256;     // workgroups: two per CU
constexpr int kC3fMaxKP1 = 64;          // dY raster rows of a step at stride 1
constexpr int kC3fMaxKP2 = 48;          // ... at stride 2, where the X raster has four times the pixels
constexpr int kC3fMaxPY = 60;           // dY raster pitch
constexpr int kC3fRowB = kC3fTile * 4;  // bytes of a tile row: 64 fp32 channels of one pixel
constexpr int kC3fKpRound = 8;
constexpr size_t kC3fLdsMax = 160 * 1024;
static_assert(kC3fMaxKP1 <= 64 && kC3fMaxKP2 <= 64 && ((kC3fMaxPY + kC3fKpRound - 1) & ~(kC3fKpRound - 1)) <= 64,
              "the dY raster of a step is one pass of the loader (four pieces of 16 rows)");

struct C3fPlan : Raster3x3 {
  int rows_per_split = 0, splits = 0, tiles = 0;
};

struct C3fArgs {
  int b, h, w, ho, wo, c, n;
  int py, ws, nseg, rmax, kp_cap;
  int rows_per_split, splits, tiles_c;
  float inv_py, inv_px;
};

// grid: tiles * splits workgroups, 256 threads; LDS = (kp_cap + xt_cap) * 256 bytes
template <int S>
__global__ __launch_bounds__(kC3fWaves* kWave, 2) void conv3x3_wgrad_f32_kernel(const float* __restrict__ dY,
                                                                                const float* __restrict__ X,
                                                                                float* __restrict__ part, C3fArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __align__(16) unsigned char smem_raw[];
  unsigned char* const ty_tile = smem_raw;
  unsigned char* const tx_tile = smem_raw + a.kp_cap * kC3fRowB;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int tiles = (a.n / kC3fTile) * a.tiles_c;
  const int split = blockIdx.x / tiles, tile = blockIdx.x - split * tiles;
  const int tn = tile / a.tiles_c, tc = tile - tn * a.tiles_c;
  const int n0 = tn * kC3fTile, c0 = tc * kC3fTile;
  const int rows = a.b * a.ho;
  const int r_begin = split * a.rows_per_split, r_end = min(rows, r_begin + a.rows_per_split);
  const int PY = a.py, PX = S * a.py;

  const int wn = wave >> 1, wc = wave & 1;
  const int hh = lane >> 5;                                // this lane's pixel of a two-pixel k-step
  const int colA = (wn * 32 + (lane & 31)) * 4, colB = (wc * 32 + (lane & 31)) * 4;   // byte columns of its n and its c

  c3f_f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  const int prow = tid >> 4, pch = tid & 15;               // the loader: 16 tile rows per pass, 16 pieces a row
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  // (32-bit byte offsets from the uniform bases: the planner refuses tensors of 2^31 bytes)
  const unsigned char* const dYb = reinterpret_cast<const unsigned char*>(dY);
  const unsigned char* const Xb = reinterpret_cast<const unsigned char*>(X);

  for (int r = r_begin; r < r_end;) {
    const RowStep st = row_step(r, r_end, a.ho, a.rmax);
    const int R = st.R;
    const int KP = (R * PY + kC3fKpRound - 1) & ~(kC3fKpRound - 1);
    const int XT = S * KP + S * (S - 1) * PY * (R - 1) + 2 * PX + 3;
    for (int seg = 0; seg < a.nseg; ++seg) {
      const int xo0 = seg * a.ws, ws = min(a.ws, a.wo - xo0);
      __syncthreads();                                      // the previous step's reads are done
      // ---- dY raster: rows [0, KP), every load predicated on its own pixel, zeros elsewhere ----
      {
        u32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int p = 16 * u + prow;
          v[u] = zero4;
          if (p < KP) {
            const int ry = (int)(((float)p + 0.5f) * a.inv_py), j = p - ry * PY;
            if (ry < R && j < ws)
              v[u] = *reinterpret_cast<const u32x4*>(
                  dYb + 4u * (unsigned)(((st.img * a.ho + st.yo0 + ry) * a.wo + xo0 + j) * a.n + n0 + pch * 4));
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int p = 16 * u + prow;
          if (p < KP) *reinterpret_cast<u32x4*>(ty_tile + p * kC3fRowB + pch * 16) = v[u];
        }
      }
      // ---- X raster: rows [0, XT), 64 a pass ----
      {
        const int ty_need = S * (R - 1) + 3, cx_need = S * (ws - 1) + 3;     // X raster rows / columns some tap of this step reads
        const int yi0 = st.yo0 * S - 1, xi0 = xo0 * S - 1;
        for (int t0 = 0; t0 < XT; t0 += 64) {
          u32x4 v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int t = t0 + 16 * u + prow;
            v[u] = zero4;
            if (t < XT) {
              const int ty = (int)(((float)t + 0.5f) * a.inv_px), cx = t - ty * PX;
              const int yi = yi0 + ty, xi = xi0 + cx;
              if (ty < ty_need && cx < cx_need && yi >= 0 && yi < a.h && xi >= 0 && xi < a.w)
                v[u] = *reinterpret_cast<const u32x4*>(
                    Xb + 4u * (unsigned)(((st.img * a.h + yi) * a.w + xi) * a.c + c0 + pch * 4));
            }
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int t = t0 + 16 * u + prow;
            if (t < XT) *reinterpret_cast<u32x4*>(tx_tile + t * kC3fRowB + pch * 16) = v[u];
          }
        }
      }
      __syncthreads();
      // ---- nine products over the step's pixels, two pixels an instruction; the next k-step's operands are read first ----
      // the X raster row of dY raster row p = ry*PY + j under tap (0, 0): (S*ry)*PX + S*j = S*p + S*(S-1)*PY*ry (the tail behind
      // the step's last row, all zeros in dY, stays inside the raster with ry held at R - 1)
      auto read_ops = [&](int k0, float& fa, float (&fb)[9]) {
        const int k = k0 + hh;
        fa = *reinterpret_cast<const float*>(ty_tile + k * kC3fRowB + colA);
        int xr = S * k;
        if (S > 1) xr += S * (S - 1) * PY * min((int)(((float)k + 0.5f) * a.inv_py), R - 1);
        const unsigned char* xp = tx_tile + xr * kC3fRowB + colB;
#pragma unroll
        for (int t = 0; t < 9; ++t) fb[t] = *reinterpret_cast<const float*>(xp + ((t / 3) * PX + t % 3) * kC3fRowB);
      };
      float fa, fb[9];
      read_ops(0, fa, fb);
      for (int k0 = 0; k0 < KP; k0 += 2) {
        float fan = fa, fbn[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) fbn[t] = fb[t];
        if (k0 + 2 < KP) read_ops(k0 + 2, fan, fbn);
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb[t], acc[t], 0, 0, 0);
        fa = fan;
#pragma unroll
        for (int t = 0; t < 9; ++t) fb[t] = fbn[t];
      }
    }
    r += R;
  }

  // ---- partial tile: D[i][j], j = lane % 32 (c) on the lane, i = 8*(e/4) + 4*(lane/32) + e%4 (n) in register e ----
  float* po = part + (((size_t)split * a.n + n0 + wn * 32) * 9) * a.c + c0 + wc * 32 + (lane & 31);
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) po[((size_t)(8 * (e >> 2) + 4 * hh + (e & 3)) * 9 + t) * a.c] = acc[t][e];
#endif
}

// conv_spatial.h's raster of a step, and splits over output rows so that the grid is two workgroups per CU.  Refused on top
// of what raster3x3 refuses: b*h*w*max(c, n)*4 >= 2^31 (32-bit byte offsets of fp32 elements).
C3fPlan c3f_plan(int b, int c, int n, int h, int w, int s) {
  C3fPlan p;
  if (b <= 0 || c <= 0 || n <= 0 || h <= 0 || w <= 0) return p;
  if ((unsigned long long)b * h * w * std::max(c, n) * 4 >= 1ull << 31) return p;
  static_cast<Raster3x3&>(p) = raster3x3(b, c, n, h, w, s, kC3fMaxKP1, kC3fMaxKP2, kC3fMaxPY, kC3fKpRound);
  if (!p.ok) return p;
  if ((size_t)(p.kp_cap + p.xt_cap) * kC3fRowB > kC3fLdsMax) {
    p.ok = 0;
    return p;
  }
  p.tiles = (n / kC3fTile) * (c / kC3fTile);
  const RowSplit sp = split_rows((long long)b * p.ho, p.tiles, kC3fTarget);
  p.rows_per_split = sp.per;
  p.splits = sp.count;
  return p;
}

}  // namespace

int conv3x3_f32_wgrad_rows(int b, int c, int n, int h, int w, int s) {
  const C3fPlan p = c3f_plan(b, c, n, h, w, s);
  return p.ok ? p.splits : MRLA_EUNSUPPORTED;
}

// {tile n, tile c, output rows per split, LDS stages, splits, output tiles}
int conv3x3_f32_wgrad_plan(int b, int c, int n, int h, int w, int s, int* out) {
  const C3fPlan p = c3f_plan(b, c, n, h, w, s);
  if (!p.ok) return MRLA_EUNSUPPORTED;
  out[0] = kC3fTile; out[1] = kC3fTile; out[2] = p.rows_per_split; out[3] = kC3fStages; out[4] = p.splits; out[5] = p.tiles;
  return MRLA_OK;
}

int launch_conv3x3_f32_wgrad(const float* dy, const float* x, float* part, float* dw, int b, int c, int n, int h, int w, int s,
                             hipStream_t st) {
  const C3fPlan p = c3f_plan(b, c, n, h, w, s);
  if (!p.ok) return MRLA_EUNSUPPORTED;
  C3fArgs a;
  a.b = b; a.h = h; a.w = w; a.ho = p.ho; a.wo = p.wo; a.c = c; a.n = n;
  a.py = p.py; a.ws = p.ws; a.nseg = p.nseg; a.rmax = p.rmax; a.kp_cap = p.kp_cap;
  a.rows_per_split = p.rows_per_split; a.splits = p.splits; a.tiles_c = c / kC3fTile;
  a.inv_py = 1.0f / (float)p.py; a.inv_px = 1.0f / (float)(s * p.py);
  const size_t lds = (size_t)(p.kp_cap + p.xt_cap) * kC3fRowB;
  const dim3 grid(p.tiles * p.splits), block(kC3fWaves * kWave);
  auto launch = [&](auto kernel) {
    if (lds_opt_in(reinterpret_cast<const void*>(kernel), lds) != hipSuccess) return (int)MRLA_EHIP;
    hipLaunchKernelGGL(kernel, grid, block, lds, st, dy, x, part, a);
    return hip_status(hipGetLastError());
  };
  const int rc = s == 1 ? launch(conv3x3_wgrad_f32_kernel<1>) : launch(conv3x3_wgrad_f32_kernel<2>);
  if (rc != MRLA_OK) return rc;
  return launch_split_sum(part, dw, 1, MRLA_F32, p.splits, n * 9 * c, st);
}

}  // namespace mrla
