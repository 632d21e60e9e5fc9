// 1x1 stride-1 convolution of a channels_last fp32 activation on the exact fp32-input MFMA (v_mfma_f32_32x32x2_f32: bitwise a
// chain of fmaf, no reduced-precision path), for the recipe that trains without autocast:
//   forward / input gradient   Y[M, N] = X[M, K] * W^T   W: [N, K], or reduction-major [K, N] (w_trans: the input gradient
//                                                         dX[m, k] = dY[m, n] W[n, k] on the module's own [n, k] weight)
//   part[row, n, 0..3]         [opt] moment record of the fp32 outputs as stored (MRLA_GEMM_MOMENTS): sum (y - p),
//                              sum (y - p)^2, the pivot p (the row's first output of the channel), pixel count
//   weight gradient            dW[N, K] = sum_m dY[m, N] X[m, K]: split-M partial tiles + conv1x1_wgrad_reduce_kernel<float>
// Nothing here is shared with the 16-bit tile code (conv1x1.hip, conv1x1_wide.hip, conv1x1_kstream.hip, conv1x1_wgrad.hip).
//
// Forward.  The instruction takes ONE f32 per lane and operand: lane l holds row / column l & 31 at k = l >> 5.  A sum over
// k may be taken in any order as long as both operands use the same order, so lane half h owns k = 8j + 4h .. 8j + 4h + 3
// of its pixel's row: one 16-byte global load of X feeds four MFMAs, whose two k are (8j + i, 8j + 4 + i), and the matching
// A operand is one 16-byte LDS read of the W row -- no transposition anywhere.
//   * A = W tile (rows = out-channels), B = X tile (columns = pixels); a wave owns 32 pixels x 64 channels (two accumulator
//     tiles); a workgroup of four waves is (pixel blocks) x (64-channel groups) over a slice of NS = 64, 128 or 256 channels;
//   * an output is not ONE chain of k fused multiply-adds but four (the 8-k groups of the lane map dealt round over four
//     accumulator tiles, summed pairwise at the end): the rounding error of a sequential fp32 chain grows with its length,
//     and a single chain of k = 256 .. 2048 measured about twice the error of the stock convolution against float64;
//   * the reduction runs in chunks of 64 k: 8 x 16 bytes of X per lane, double-buffered -- the next chunk (of this pixel block,
//     or the first one of the workgroup's next block) is in flight during the 64 MFMAs of this one;
//   * resident form (k <= 256): the W slice [NS][k] stays in LDS for the whole kernel, rows padded by 16 bytes (conflict-free
//     b128 reads); the workgroups are persistent over pixel blocks;
//   * streaming form (k > 256): W goes through two LDS chunk buffers [NS][64], the next chunk loaded into registers during
//     this chunk's MFMAs and written behind them; one barrier per chunk;
//   * w_trans: the staging loop reads 16 bytes along n and writes four scalars, lanes ordered so that a wave's writes fall
//     into 64 different banks;
//   * the accumulator layout has 4 consecutive channels of one pixel per register quad: eight 16-byte writes put the wave's
//     tile [32 pixels][64 channels] into its private LDS tile, and it leaves as whole 128-byte lines (16 lanes per pixel);
//   * the moments are taken on the store lanes: a lane sees the same 4 channels of 8 pixel rows of every block, so 4
//     (sum, sum of squares, pivot) triples per lane cover the wave's 64 channels.
// Weight gradient.  The reduction index is the pixel and both operands are channel-contiguous: lane (r, h) loads
// dY[p + h][n0 + r] and X[p + h][k0 + r], a half-wave's load is one 128-byte line, no LDS.  A wave owns a 64 x 64 tile of dW
// (four accumulator tiles), the four waves of a workgroup own neighbouring tiles of the same pixel range (the shared
// operand's lines hit in the vector cache), and each workgroup writes its partial tiles of part[split]; fixed split, no atomics.
#include <algorithm>

#include "conv1x1_lds.h"
#include "mrla_device.h"
#include "mrla_kernels.h"

namespace mrla {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kFWaves = 4;                           // waves per workgroup, both kernels
constexpr int kKC = 64;                              // reduction chunk of the forward
constexpr int kXS = kKC / 8;                         // 16-byte X pieces per lane and chunk
constexpr int kChains = 4;                           // independent accumulation chains per output (k-group j goes to chain j % 4)
constexpr int kFOutRowB = 64 * 4 + 16;               // padded row of the per-wave output tile (64 channels of one pixel)
constexpr int kFOutTileB = 32 * kFOutRowB;
constexpr int kChunkRowB = kKC * 4 + 16;             // padded row of a streamed W chunk

__device__ __forceinline__ void mfma_f32(f32x16& c, float a, float b) {
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

template <int WN, bool MOM, bool STREAM>
__global__ __launch_bounds__(kFWaves* kWave) void conv1x1_f32_fwd_kernel(const float* __restrict__ X,
                                                                         const float* __restrict__ W, float* __restrict__ Y,
                                                                         float* __restrict__ part, int M, int K, int N,
                                                                         int w_trans) {
  constexpr int NS = WN * 64, WM = kFWaves / WN;
  constexpr int NST = NS * (kKC / 4) / (kFWaves * kWave);      // 16-byte pieces of a W chunk per thread
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int r = lane & 31, h = lane >> 5;
  const int wn = wave % WN, wm = wave / WN;
  const int n_slice0 = blockIdx.y * NS;
  const int NKC = K / kKC;
  const int ROWB = STREAM ? kChunkRowB : K * 4 + 16;
  const int wbytes = STREAM ? 2 * NS * kChunkRowB : NS * ROWB;
  unsigned char* otile = smem_raw + wbytes + wave * kFOutTileB;

  // chunk k0 .. k0 + 63 of the W slice: global -> registers, registers -> LDS rows (byte column colb)
  f32x4 wst[NST];
  auto w_load = [&](int k0) {
#pragma unroll
    for (int s = 0; s < NST; ++s) {
      const int i = threadIdx.x + s * (kFWaves * kWave);
      const float* src;
      if (w_trans) {
        const int k = ((i >> 6) & 3) * 16 + (i & 15), n = ((i >> 8) * 4 + ((i >> 4) & 3)) * 4;
        src = W + (size_t)(k0 + k) * N + n_slice0 + n;
      } else {
        src = W + (size_t)(n_slice0 + (i >> 4)) * K + k0 + (i & 15) * 4;
      }
      wst[s] = *reinterpret_cast<const f32x4*>(src);
    }
  };
  auto w_write = [&](unsigned char* base, int colb) {
#pragma unroll
    for (int s = 0; s < NST; ++s) {
      const int i = threadIdx.x + s * (kFWaves * kWave);
      if (w_trans) {
        const int k = ((i >> 6) & 3) * 16 + (i & 15), n = ((i >> 8) * 4 + ((i >> 4) & 3)) * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c) *reinterpret_cast<float*>(base + (n + c) * ROWB + colb + k * 4) = wst[s][c];
      } else {
        *reinterpret_cast<f32x4*>(base + (i >> 4) * ROWB + colb + (i & 15) * 16) = wst[s];
      }
    }
  };

  if (!STREAM) {
    for (int kc = 0; kc < NKC; ++kc) {
      w_load(kc * kKC);
      w_write(smem_raw, kc * kKC * 4);
    }
  } else {
    w_load(0);
    w_write(smem_raw, 0);
  }
  __syncthreads();

  // moments about a pivot (this wave's first output of the channel), on the store lanes: the 4 channels of the lane's piece
  float s1[4], s2[4], pv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { s1[i] = 0.f; s2[i] = 0.f; pv[i] = 0.f; }
  bool have_pivot = false;
  int npix = 0;                                     // pixels this wave accumulated (wave-uniform)

  const int nblk = (M + 31) / 32, ngrp = (nblk + WM - 1) / WM;
  f32x4 xf[kXS], xn[kXS];
  // chunk kc of the X fragments of this wave's block of group g_ (rows past the end: clamped, never used)
  auto load_x = [&](f32x4 (&dst)[kXS], int g_, int kc) {
    const int row = min((g_ * WM + wm) * 32 + r, M - 1);
    const f32x4* xp = reinterpret_cast<const f32x4*>(X + (size_t)row * K + kc * kKC + h * 4);
#pragma unroll
    for (int j = 0; j < kXS; ++j) dst[j] = xp[j * 2];
  };
  int it = 0;                                       // chunks done by the workgroup (streaming form: the LDS buffer in turn)
  if ((int)blockIdx.x < ngrp) load_x(xn, blockIdx.x, 0);
  for (int grp = blockIdx.x; grp < ngrp; grp += gridDim.x) {       // (workgroup-uniform: the streaming form has barriers)
    const int blk = grp * WM + wm;
    const bool valid = blk < nblk;                  // wave-uniform; only the last group can have waves without a block
    f32x16 acc[2][kChains];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int c = 0; c < kChains; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][c][i] = 0.f;
#pragma unroll 1
    for (int kc = 0; kc < NKC; ++kc, ++it) {
#pragma unroll
      for (int j = 0; j < kXS; ++j) xf[j] = xn[j];
      const bool more_k = kc + 1 < NKC;
      const bool more = more_k || grp + (int)gridDim.x < ngrp;
      if (more) load_x(xn, more_k ? grp : grp + gridDim.x, more_k ? kc + 1 : 0);
      if (STREAM && more) w_load(more_k ? (kc + 1) * kKC : 0);
      const unsigned char* wbase = STREAM ? smem_raw + (it & 1) * (NS * kChunkRowB) : smem_raw + kc * kKC * 4;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const unsigned char* wrow = wbase + (wn * 64 + t * 32 + r) * ROWB + h * 16;
#pragma unroll
        for (int j = 0; j < kXS; ++j) {
          const f32x4 wf = *reinterpret_cast<const f32x4*>(wrow + j * 32);
#pragma unroll
          for (int i = 0; i < 4; ++i) mfma_f32(acc[t][j % kChains], wf[i], xf[j][i]);
        }
      }
      if (STREAM) {
        // the other buffer was last read one chunk ago, before the barrier every wave has passed since
        if (more) w_write(smem_raw + ((it + 1) & 1) * (NS * kChunkRowB), 0);
        __syncthreads();
      }
    }
    if (valid) {
      // the chains summed pairwise (a fixed order); register quad g of tile t: channels t*32 + 8g + 4h .. + 3 of pixel r
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const f32x16 sum = (acc[t][0] + acc[t][1]) + (acc[t][2] + acc[t][3]);
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<f32x4*>(otile + r * kFOutRowB + (t * 32 + 8 * g + 4 * h) * 4) =
              (f32x4){sum[4 * g], sum[4 * g + 1], sum[4 * g + 2], sum[4 * g + 3]};
      }
      // whole lines out: 16 lanes per pixel (64 channels = 256 bytes), 4 pixels per store instruction
      const int px = lane >> 4, piece = lane & 15;
      float* ybase = Y + (size_t)blk * 32 * N + n_slice0 + wn * 64 + piece * 4;
      if (MOM && !have_pivot) {
        // first block of this wave: the pivot is tile pixel 0, which always exists, for every lane of a piece
        const f32x4 p0 = *reinterpret_cast<const f32x4*>(otile + piece * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) pv[j] = p0[j];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int pr = i * 4 + px;
        const f32x4 v = *reinterpret_cast<const f32x4*>(otile + pr * kFOutRowB + piece * 16);
        const bool lv = blk * 32 + pr < M;
        if (lv) *reinterpret_cast<f32x4*>(ybase + (size_t)pr * N) = v;
        if (MOM) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float d = lv ? v[j] - pv[j] : 0.f;
            s1[j] += d;
            s2[j] = fmaf(d, d, s2[j]);
          }
        }
      }
      have_pivot = true;
      npix += min(32, M - blk * 32);
    }
  }

  if (MOM) {
    // sum over the 4 lanes that hold the same piece (they share the pivot), then merge the workgroup's pixel-waves by
    // re-basing them onto the first one's pivot (fixed order, through the LDS of the output tiles, which are done with):
    // one record per workgroup row and channel
    __syncthreads();
    float* sums = reinterpret_cast<float*>(smem_raw + wbytes);          // [WM][NS][4]
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float a = s1[i], b = s2[i];
      a += __shfl_xor(a, 32, kWave); b += __shfl_xor(b, 32, kWave);
      a += __shfl_xor(a, 16, kWave); b += __shfl_xor(b, 16, kWave);
      if (lane < 16) {
        float* rec = sums + ((size_t)wm * NS + wn * 64 + lane * 4 + i) * 4;
        rec[0] = a; rec[1] = b; rec[2] = pv[i]; rec[3] = (float)npix;
      }
    }
    __syncthreads();
    float* dst = part + ((size_t)blockIdx.x * N + n_slice0) * 4;
    for (int ch = threadIdx.x; ch < NS; ch += kFWaves * kWave) {
      float S1 = 0.f, S2 = 0.f, P = 0.f, n = 0.f;
      for (int v = 0; v < WM; ++v) {
        const float* rec = sums + ((size_t)v * NS + ch) * 4;
        const float a = rec[0], b = rec[1], nv = rec[3];
        if (nv == 0.f) continue;                     // a pixel-wave without a block
        if (n == 0.f) P = rec[2];
        const float dlt = rec[2] - P;                // sums about rec[2] -> about P
        S2 += b + 2.f * dlt * a + nv * dlt * dlt;
        S1 += a + nv * dlt;
        n += nv;
      }
      dst[ch * 4 + 0] = S1; dst[ch * 4 + 1] = S2; dst[ch * 4 + 2] = P; dst[ch * 4 + 3] = n;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// weight gradient
// ------------------------------------------------------------------------------------------------
constexpr int kWgU = 4;                              // pixel pairs per step (8 pixels: 16 operand loads, 16 MFMAs)

__global__ __launch_bounds__(kFWaves* kWave) void conv1x1_f32_wgrad_kernel(const float* __restrict__ dY,
                                                                           const float* __restrict__ X,
                                                                           float* __restrict__ part, int M, int K, int N,
                                                                           int chunks_per_wg, int groups) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int r = lane & 31, h = lane >> 5;
  const int KT = K / 64, T = (N / 64) * KT;
  const int grp = blockIdx.x % groups, split = blockIdx.x / groups;
  const int tile = grp * kFWaves + wave;             // neighbouring tiles: the same 64 channels of dY, or of X when k = 64
  if (tile >= T) return;                             // (no barrier in this kernel)
  const int n0 = (tile / KT) * 64, k0 = (tile % KT) * 64;
  const int p0 = split * chunks_per_wg * 32, p1 = min(M, p0 + chunks_per_wg * 32);

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

  const float* ap = dY + n0 + r;
  const float* bp = X + k0 + r;
  float a[kWgU][2], b[kWgU][2], an[kWgU][2], bn[kWgU][2];
  // pixel p + 2u + h is lane half h's in pair u; pixels past the range contribute zeros
  auto load = [&](float (&a_)[kWgU][2], float (&b_)[kWgU][2], int p) {
#pragma unroll
    for (int u = 0; u < kWgU; ++u) {
      const int px = p + 2 * u + h;
      const bool ok = px < p1;
      const size_t row = (size_t)min(px, p1 - 1);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float av = ap[row * N + i * 32], bv = bp[row * K + i * 32];
        a_[u][i] = ok ? av : 0.f;
        b_[u][i] = ok ? bv : 0.f;
      }
    }
  };
  load(an, bn, p0);
  for (int p = p0; p < p1; p += 2 * kWgU) {
#pragma unroll
    for (int u = 0; u < kWgU; ++u)
#pragma unroll
      for (int i = 0; i < 2; ++i) { a[u][i] = an[u][i]; b[u][i] = bn[u][i]; }
    if (p + 2 * kWgU < p1) load(an, bn, p + 2 * kWgU);
#pragma unroll
    for (int u = 0; u < kWgU; ++u)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) mfma_f32(acc[i][j], a[u][i], b[u][j]);
  }
  // acc[i][j] register q: dW row n0 + i*32 + (q & 3) + 8 (q >> 2) + 4h, column k0 + j*32 + r: a half-wave stores a line
  float* dst = part + (size_t)split * N * K + (size_t)n0 * K + k0 + r;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) dst[(size_t)(i * 32 + (q & 3) + 8 * (q >> 2) + 4 * h) * K + j * 32] = acc[i][j][q];
}

// ------------------------------------------------------------------------------------------------
// geometry
// ------------------------------------------------------------------------------------------------
constexpr size_t kLdsBudget = 160 * 1024;

bool f32_shape_ok(int M, int K, int N) {
  if (M <= 0 || K < 64 || K > 2048 || K % 64 || N <= 0 || N % 64) return false;
  return (size_t)M * std::max(N, K) * 4 < (size_t)1 << 31;        // 32-bit element offsets everywhere
}

struct F32Geo { int stream, WN, gx, gy; size_t lds; };

bool f32_geo(F32Geo* g, int M, int K, int N) {
  if (!f32_shape_ok(M, K, N)) return false;
  g->stream = K > 256;
  int ns;
  if (g->stream) {
    ns = N % 128 == 0 ? 128 : 64;
    g->lds = (size_t)2 * ns * kChunkRowB + kFWaves * kFOutTileB;
  } else {
    // the widest slice of the weight that fits beside the output tiles: X is read N / NS times
    ns = 256;
    while (ns > 64 && (N % ns || (size_t)ns * (K * 4 + 16) + kFWaves * kFOutTileB > kLdsBudget)) ns /= 2;
    g->lds = (size_t)ns * (K * 4 + 16) + kFWaves * kFOutTileB;
  }
  g->WN = ns / 64;
  g->gy = N / ns;
  if (g->gy > 65535) return false;                      // (grid.y; far from any model shape)
  const int wm = kFWaves / g->WN;
  const int nblk = (M + 31) / 32, ngrp = (nblk + wm - 1) / wm;
  // persistent workgroups: as many per CU as their LDS allows (at most 2), each with the same number of pixel groups
  const int per_cu = g->lds * 2 <= kLdsBudget ? 2 : 1;
  const int want = std::max(1, std::min(ngrp, (256 * per_cu) / g->gy));
  const int per_wg = (ngrp + want - 1) / want;
  g->gx = (ngrp + per_wg - 1) / per_wg;
  return true;
}

struct F32WgPlan { int groups = 0, splits = 0, chunks_per_wg = 0; };

F32WgPlan f32_wgrad_plan(int M, int K, int N) {
  F32WgPlan p;
  if (!f32_shape_ok(M, K, N)) return p;
  const int tiles = (N / 64) * (K / 64);
  p.groups = (tiles + kFWaves - 1) / kFWaves;
  const int chunks = (M + 31) / 32;
  const int want = std::max(1, std::min(chunks, (512 + p.groups - 1) / p.groups));     // two workgroups per CU
  p.chunks_per_wg = (chunks + want - 1) / want;
  p.splits = (chunks + p.chunks_per_wg - 1) / p.chunks_per_wg;
  return p;
}

}  // namespace

int conv1x1_f32_rows(int M, int K, int N) {
  F32Geo g;
  return f32_geo(&g, M, K, N) ? g.gx : MRLA_EUNSUPPORTED;
}

// {form (0, 1, 2: resident weights with 1, 2, 4 channel groups per workgroup; 4, 5: streamed weights with 1, 2), X chunks
//  in flight (2), workgroups, record rows}
int conv1x1_f32_plan(int M, int K, int N, int* out) {
  F32Geo g;
  if (!f32_geo(&g, M, K, N)) return MRLA_EUNSUPPORTED;
  out[0] = g.stream * 4 + (g.WN == 4 ? 2 : g.WN - 1);
  out[1] = 2;
  out[2] = g.gx * g.gy;
  out[3] = g.gx;
  return MRLA_OK;
}

int launch_conv1x1_f32_fwd(const float* x, const float* w, int w_trans, float* y, float* part, int M, int K, int N,
                           hipStream_t st) {
  F32Geo g;
  if (!f32_geo(&g, M, K, N)) return MRLA_EUNSUPPORTED;
  const dim3 grid(g.gx, g.gy), block(kFWaves * kWave);
  auto launch = [&](auto wn, auto stream) {
    constexpr int WN = decltype(wn)::value;
    constexpr bool STREAM = decltype(stream)::value;
    return part ? launch_kernel(conv1x1_f32_fwd_kernel<WN, true, STREAM>, grid, block, g.lds, st, x, w, y, part, M, K, N, w_trans)
                : launch_kernel(conv1x1_f32_fwd_kernel<WN, false, STREAM>, grid, block, g.lds, st, x, w, y, part, M, K, N, w_trans);
  };
  if (g.stream) return g.WN == 2 ? launch(Int<2>(), std::true_type()) : launch(Int<1>(), std::true_type());
  return g.WN == 4 ? launch(Int<4>(), std::false_type())
                   : g.WN == 2 ? launch(Int<2>(), std::false_type()) : launch(Int<1>(), std::false_type());
}

int conv1x1_f32_wgrad_rows(int M, int K, int N) {
  const F32WgPlan p = f32_wgrad_plan(M, K, N);
  return p.groups ? p.splits : MRLA_EUNSUPPORTED;
}

int launch_conv1x1_f32_wgrad(const float* dy, const float* x, float* part, float* dw, int M, int K, int N, hipStream_t st) {
  const F32WgPlan p = f32_wgrad_plan(M, K, N);
  if (!p.groups) return MRLA_EUNSUPPORTED;
  const int rc = launch_kernel(conv1x1_f32_wgrad_kernel, dim3(p.groups * p.splits), dim3(kFWaves * kWave), 0, st, dy, x, part, M,
                               K, N, p.chunks_per_wg, p.groups);
  if (rc != MRLA_OK) return rc;
  return launch_conv1x1_wgrad_reduce_f32(part, dw, p.splits, N * K, st);
}

}  // namespace mrla
