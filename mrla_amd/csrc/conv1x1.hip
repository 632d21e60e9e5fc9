// 1x1 stride-1 convolution of a channels_last bf16 or fp16 activation as an MFMA GEMM with a BatchNorm-statistics epilogue:
//   Y[M, N] = X[M, K] * W[N, K]^T      (M = b*h*w pixels, K = in-channels, N = out-channels; both operands K-contiguous)
//   part[row, n, 0..3] = per-workgroup moment record of the bf16-ROUNDED outputs of channel n (MRLA_GEMM_MOMENTS):
//                        sum (y - p), sum (y - p)^2, the pivot p (a first output of the channel), pixel count
// Reference: the bottleneck's conv1 / bn1 and conv3 / bn3 (resnet/models/resnet_mrla_light.py:93-102): the statistics pass
// of the BatchNorm that follows the convolution (1N read of the large conv3 output) disappears into this epilogue, and
// the output is written exactly once (MIOpen's implicit-GEMM solver memsets it first).
//
// These GEMMs are memory-bound in the early stages (K = 64 .. 128: 50-100 flop/byte) and skinny everywhere, so the
// kernel is organised around the streams, not around a big LDS tile:
//   * MFMA 32x32x16 bf16 with A = W tile (rows = out-channels), B = X tile (columns = pixels): each lane's B fragment is
//     16 contiguous bytes of ITS pixel's row of X, loaded straight from global memory into registers (no LDS, no
//     transposition), kept for all out-channels of the wave and double-buffered against the next pixel block;
//   * the W slice of the workgroup stays in LDS for the whole kernel (rows padded by 16 B: conflict-free b128 reads);
//     a workgroup is persistent over pixel blocks, its 8 waves split (pixel blocks) x (64-channel pairs);
//   * the accumulator tile has the pixel on the lane and 16 channels in registers; after rounding to bf16 a
//     v_permlane32_swap between the two half-waves leaves every lane with 16-byte pieces of its pixel's output row;
//     a wave-private LDS tile [32 pixels][64 channels] then turns them into stores of whole 128-byte lines (8 lanes
//     per pixel) -- 32-byte fragments per pixel straight from the lanes cost the L2 four requests per line;
//   * the BatchNorm moments are per-lane running sums taken where the lines are stored: a store lane reads the same 8
//     channels of 4 pixel rows of every block back from the tile, so 8 (sum, sum of squares, pivot) triples per lane
//     cover the wave's 64 channels (in the accumulator layout, one triple per accumulator register = 96 registers, the
//     K = 256 instance spilled); they are reduced across lanes and pixel-waves once at the end of the kernel and written
//     as one partial row per workgroup;
//   * the input-gradient use with the shortcut's gradient (conv1x1_fwd_addend_kernel, no moments): the store lane adds the
//     addend's 16 bytes of the same pixel and channels to the piece it read back from the tile (conv1x1_addend.h);
//   * the inference use behind an eval-mode BatchNorm (conv1x1_fwd_affine_kernel, no moments, no addend): the store lane
//     puts that piece through the BatchNorm's per-channel affine and ReLU (conv1x1_affine.h).  A lane stores the same 8
//     channels of every row; the wave's 64 + 64 fp32 coefficients sit in the 16 padding bytes behind the 32 rows of its
//     output tile (32 x 16 B = 512 B, exactly them) and are read back per block, so no register lives across the MFMAs.
#include <algorithm>

#include "conv1x1_addend.h"
#include "conv1x1_affine.h"
#include "conv1x1_lds.h"
#include "mrla_device.h"
#include "mrla_kernels.h"

namespace mrla {

typedef c1_f32x16 f32x16;

constexpr int kOutRowB = 64 * 2 + 16;               // padded row of the per-wave output tile (64 channels of one pixel)
constexpr int kOutTileB = 32 * kOutRowB;

// channel of accumulator register `reg` inside its 32-channel tile, for lane half h
__device__ __forceinline__ int acc_channel(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

template <typename T, int KS, bool MOM, int NW, bool ADD, bool AFF = false>
__device__ __forceinline__ void conv1x1_fwd_body(
    const T* __restrict__ X, const T* __restrict__ W, T* Y, float* __restrict__ part,
    int M, int N, int NS, int WN, int rows_total, const T* A, const AddendGeo& ag,
    const float* __restrict__ sc = nullptr, const float* __restrict__ sh = nullptr, int relu = 0) {
  typedef Elem16<T> E;
  typedef typename E::x8 x8;
  static_assert(!(MOM && ADD), "the moment records are those of the GEMM's own outputs");
  static_assert(!(AFF && (MOM || ADD)), "the affine form is the plain forward of inference: no records, no addend");
  constexpr int K = KS * 16;
  constexpr int ROWB = K * 2 + 16;                   // padded LDS row of W, bytes
  constexpr int KC = KS < 16 ? KS : 16;              // k-steps whose X fragments are in registers at a time
  constexpr int NCH = KS / KC;
  constexpr bool DB = KS <= 16;                      // the next pixel block's X fragments are fetched during this one's MFMAs
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int r = lane & 31, h = lane >> 5;
  const int WM = NW / WN, wn = wave % WN, wm = wave / WN;
  const int n_slice0 = blockIdx.y * NS;
  unsigned char* otile = smem_raw + (size_t)NS * ROWB + (size_t)wave * kOutTileB;      // after the W slice

  // stage the W slice [NS][K] into LDS (16-byte pieces, coalesced)
  {
    constexpr int PPR = K / 8;                       // 16-byte pieces per row
    const u32x4* wsrc = reinterpret_cast<const u32x4*>(W + (size_t)n_slice0 * K);
    for (int i = threadIdx.x; i < NS * PPR; i += NW * kWave) {
      const int row = i / PPR, pc = i - row * PPR;
      *reinterpret_cast<u32x4*>(smem_raw + (size_t)row * ROWB + pc * 16) = wsrc[i];
    }
  }
  __syncthreads();

  if (AFF) {
    // the wave's coefficients into the padding of its output tile: row 4*piece + q holds, for the 8 channels of 16-byte
    // piece `piece`, sc[0..3], sc[4..7], sh[0..3], sh[4..7] (q = 0..3).  Wave-private, like the tile: no barrier.
    if (lane < 32) {
      const float* src = ((lane & 2) ? sh : sc) + n_slice0 + wn * 64 + (lane >> 2) * 8 + (lane & 1) * 4;
      *reinterpret_cast<u32x4*>(otile + lane * kOutRowB + 128) = *reinterpret_cast<const u32x4*>(src);
    }
  }

  // moments about a pivot (this wave's first output of the channel), see conv1x1_wide.hip; taken on the store lanes:
  // a lane keeps the 8 channels of ITS 16-byte piece of the output lines, the same piece for every block of the wave
  float s1[8], s2[8], pv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { s1[i] = 0.f; s2[i] = 0.f; pv[i] = 0.f; }
  bool have_pivot = false;
  int npix = 0;                                     // pixels this wave accumulated (wave-uniform)

  const int nblk = (M + 31) / 32;
  const int stride = gridDim.x * WM;
  int blk = blockIdx.x * WM + wm;
  u32x4 xf[KC], xn[DB ? KC : 1];
  // K chunk `kc` (KC k-steps) of the X fragments of pixel block b_
  auto load_x = [&](u32x4 (&dst)[KC], int b_, int kc) {
    const int row = min(b_ * 32 + r, M - 1);        // (rows past the end are loaded clamped and never used)
    const u32x4* xp = reinterpret_cast<const u32x4*>(X + (size_t)row * K + kc * KC * 16 + h * 8);
#pragma unroll
    for (int ks = 0; ks < KC; ++ks) dst[ks] = xp[ks * 2];
  };
  if (blk < nblk) load_x(xf, blk, 0);
  for (; blk < nblk; blk += stride) {
    if constexpr (DB) {
      if (blk + stride < nblk) load_x(reinterpret_cast<u32x4(&)[KC]>(xn), blk + stride, 0);
    }
    npix += min(32, M - blk * 32);
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    // the addend pieces of the four pixel rows this lane stores (A may alias Y: a lane reads exactly the bytes it overwrites)
    u32x4 av[ADD ? 4 : 1];
    if (ADD) {
#if defined(__HIP_DEVICE_COMPILE__)
      const auto rsA = addend_rsrc(A, ag, N);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        av[i] = __builtin_amdgcn_raw_buffer_load_b128(
            rsA, addend_offset(ag, blk * 32 + i * 8 + (lane >> 3), M, N, n_slice0 + wn * 64 + (lane & 7) * 8), 0, 0);
#endif
    }
#pragma unroll 1
    for (int kc = 0; kc < NCH; ++kc) {             // (not unrolled: the chunks' fragments must not be live together)
      if (kc > 0) load_x(xf, blk, kc);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const unsigned char* wrow = smem_raw + (size_t)(wn * 64 + t * 32 + r) * ROWB + kc * KC * 32 + h * 16;
#pragma unroll
        for (int ks = 0; ks < KC; ++ks) {
          const u32x4 wf = *reinterpret_cast<const u32x4*>(wrow + ks * 32);
          E::mfma(acc[t], __builtin_bit_cast(x8, wf), __builtin_bit_cast(x8, xf[ks]));
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      // round to the element type (pairs of neighbouring channels)
      unsigned p[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) p[i] = E::pack(acc[t][2 * i], acc[t][2 * i + 1]);
      // lane half 0 holds channels {0-3, 8-11, 16-19, 24-27} of its pixel, half 1 the other four groups; after the
      // swaps half 0 holds {0-7, 16-23} and half 1 {8-15, 24-31}: two 16-byte pieces per lane
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
      for (int g = 0; g < 2; ++g) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const auto sw = __builtin_amdgcn_permlane32_swap(p[4 * g + q], p[4 * g + 2 + q], false, false);
          p[4 * g + q] = sw[0];
          p[4 * g + 2 + q] = sw[1];
        }
      }
#endif
      // this lane's pieces of its pixel's row in the wave's output tile: channels t*32 + h*8 .. and t*32 + 16 + h*8 ..
      unsigned char* orow = otile + r * kOutRowB + (t * 32 + h * 8) * 2;
      *reinterpret_cast<u32x4*>(orow) = (u32x4){p[0], p[1], p[2], p[3]};
      *reinterpret_cast<u32x4*>(orow + 32) = (u32x4){p[4], p[5], p[6], p[7]};
    }
    // whole lines out: 8 lanes per pixel (64 channels = 128 bytes), 8 pixels per store instruction; the statistics are
    // those of the rounded values the lane stores (4 pixel rows of its 8 channels per block; rows past M: neither)
    {
      const int px = lane >> 3, piece = lane & 7;
      T* ybase = Y + (size_t)blk * 32 * N + n_slice0 + wn * 64 + piece * 8;
      if (MOM && !have_pivot) {
        // (wave-uniform) first block of this wave: the pivot is tile pixel 0, which always exists, for every lane of a piece
        const u32x4 p0 = *reinterpret_cast<const u32x4*>(otile + piece * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) { pv[2 * j] = E::lo(p0[j]); pv[2 * j + 1] = E::hi(p0[j]); }
      }
      float sc8[8], sh8[8];
      if (AFF) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const u32x4 c = *reinterpret_cast<const u32x4*>(otile + (piece * 4 + q) * kOutRowB + 128);
#pragma unroll
          for (int j = 0; j < 4; ++j) (q < 2 ? sc8 : sh8)[(q & 1) * 4 + j] = __uint_as_float(c[j]);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int pr = i * 8 + px;
        u32x4 v = *reinterpret_cast<const u32x4*>(otile + pr * kOutRowB + piece * 16);
        if (ADD) v = addend_add8<T>(v, av[i]);
        if (AFF) v = affine8<T>(v, sc8, sh8, relu);
        const bool lv = blk * 32 + pr < M;
        if (lv) *reinterpret_cast<u32x4*>(ybase + (size_t)pr * N) = v;
        if (MOM) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float lo = E::lo(v[j]), hi = E::hi(v[j]);
            const float dl = lv ? lo - pv[2 * j] : 0.f, dh = lv ? hi - pv[2 * j + 1] : 0.f;
            s1[2 * j] += dl;     s2[2 * j] = fmaf(dl, dl, s2[2 * j]);
            s1[2 * j + 1] += dh; s2[2 * j + 1] = fmaf(dh, dh, s2[2 * j + 1]);
          }
        }
      }
    }
    have_pivot = true;
    if constexpr (DB) {
#pragma unroll
      for (int ks = 0; ks < KC; ++ks) xf[ks] = xn[ks];
    } else {
      if (blk + stride < nblk) load_x(xf, blk + stride, 0);
    }
  }

  if (MOM) {
    // rows beyond the active workgroups only exist to make the row count divide M: empty records
    if (blockIdx.x == 0) {
      for (int i = threadIdx.x; i < (rows_total - (int)gridDim.x) * NS * 4; i += NW * kWave) {
        const int row = gridDim.x + i / (NS * 4), j = i % (NS * 4);
        part[((size_t)row * N + n_slice0) * 4 + j] = 0.f;
      }
    }
    // sum over the 8 lanes that hold the same piece (they share the pivot), then merge the workgroup's pixel-waves by
    // re-basing them onto the first one's pivot (fixed order, through the LDS of the output tiles, which are done
    // with): one record per workgroup and channel
    __syncthreads();
    float* sums = reinterpret_cast<float*>(smem_raw + (size_t)NS * ROWB);          // [WM][NS][4]
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float a = s1[i], b = s2[i];
#pragma unroll
      for (int off = 32; off >= 8; off >>= 1) {
        a += __shfl_xor(a, off, kWave);
        b += __shfl_xor(b, off, kWave);
      }
      if (lane < 8) {
        const int ch = wn * 64 + lane * 8 + i;
        float* rec = sums + ((size_t)wm * NS + ch) * 4;
        rec[0] = a; rec[1] = b; rec[2] = pv[i]; rec[3] = (float)npix;
      }
    }
    __syncthreads();
    float* dst = part + ((size_t)blockIdx.x * N + n_slice0) * 4;
    for (int ch = threadIdx.x; ch < NS; ch += NW * kWave) {
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

template <int KS, bool MOM, int NW>
__global__ __launch_bounds__(NW * kWave) void conv1x1_fwd_kernel(
    const bf16_t* __restrict__ X, const bf16_t* __restrict__ W, bf16_t* __restrict__ Y, float* __restrict__ part,
    int M, int N, int NS, int WN, int rows_total) {
  conv1x1_fwd_body<bf16_t, KS, MOM, NW, false>(X, W, Y, part, M, N, NS, WN, rows_total, nullptr, AddendGeo());
}
// The fp16 instances: the same body, under a name of their own (the tests that read the compiler's resource report key the
// bf16 instances by the template lists of the names above).
template <int KS, bool MOM, int NW>
__global__ __launch_bounds__(NW * kWave) void conv1x1_fwd_f16_kernel(
    const f16_t* __restrict__ X, const f16_t* __restrict__ W, f16_t* __restrict__ Y, float* __restrict__ part,
    int M, int N, int NS, int WN, int rows_total) {
  conv1x1_fwd_body<f16_t, KS, MOM, NW, false>(X, W, Y, part, M, N, NS, WN, rows_total, nullptr, AddendGeo());
}

// y = bf16(bf16(x w^T) + addend).  A kernel name of its own: tests/test_kernel_resources_cpu.py keys the instances above by
// <KS, MOM, NW>, and these are held to the same bounds by tests/test_shortcut_addend_cpu.py.
template <int KS, int NW>
__global__ __launch_bounds__(NW * kWave) void conv1x1_fwd_addend_kernel(
    const bf16_t* __restrict__ X, const bf16_t* __restrict__ W, const bf16_t* A, bf16_t* Y, int M, int N, int NS, int WN,
    AddendGeo ag) {
  conv1x1_fwd_body<bf16_t, KS, false, NW, true>(X, W, Y, nullptr, M, N, NS, WN, 0, A, ag);
}
template <int KS, int NW>
__global__ __launch_bounds__(NW * kWave) void conv1x1_fwd_f16_addend_kernel(
    const f16_t* __restrict__ X, const f16_t* __restrict__ W, const f16_t* A, f16_t* Y, int M, int N, int NS, int WN,
    AddendGeo ag) {
  conv1x1_fwd_body<f16_t, KS, false, NW, true>(X, W, Y, nullptr, M, N, NS, WN, 0, A, ag);
}

// y = T(relu?(sc * T(x w^T) + sh)): the forward in front of an eval-mode BatchNorm.  Names of their own, as above.
// Held to the waves per SIMD the plain instances (MOM = false) they are launched in place of compile to: the affine must not
// cost the register allocation a wave.
template <int KS> constexpr int kAffWaves = KS == 4 ? 5 : KS == 8 ? 4 : 2;
template <int KS, int NW>
__global__ __launch_bounds__(NW * kWave, kAffWaves<KS>) void conv1x1_fwd_affine_kernel(
    const bf16_t* __restrict__ X, const bf16_t* __restrict__ W, const float* __restrict__ sc, const float* __restrict__ sh,
    int relu, bf16_t* __restrict__ Y, int M, int N, int NS, int WN) {
  conv1x1_fwd_body<bf16_t, KS, false, NW, false, true>(X, W, Y, nullptr, M, N, NS, WN, 0, nullptr, AddendGeo(), sc, sh, relu);
}
template <int KS, int NW>
__global__ __launch_bounds__(NW * kWave, kAffWaves<KS>) void conv1x1_fwd_f16_affine_kernel(
    const f16_t* __restrict__ X, const f16_t* __restrict__ W, const float* __restrict__ sc, const float* __restrict__ sh,
    int relu, f16_t* __restrict__ Y, int M, int N, int NS, int WN) {
  conv1x1_fwd_body<f16_t, KS, false, NW, false, true>(X, W, Y, nullptr, M, N, NS, WN, 0, nullptr, AddendGeo(), sc, sh, relu);
}

// ------------------------------------------------------------------------------------------------
// geometry: N slice per workgroup (LDS), waves along N, persistent grid
// ------------------------------------------------------------------------------------------------
struct GemmGeo { int NS, WN, WM, NW, gx, gy, rows; size_t lds; };

static bool conv1x1_geo(GemmGeo* g, int M, int K, int N) {
  // K = 512 (two fragment chunks per pixel block, no prefetch across them) is slower than the stock convolution: not taken
  if (K != 64 && K != 128 && K != 256) return false;
  if (N % 64 || M <= 0) return false;
  const int rowb = K * 2 + 16;
  int ns = std::min(N, 256);                         // at most 4 channel pairs (= waves along N) per workgroup
  while (ns > 64 && (N % ns || (ns / 64 != 1 && ns / 64 != 2 && ns / 64 != 4) || (size_t)ns * rowb > 72 * 1024)) ns -= 64;
  if (N % ns) return false;
  g->NS = ns;
  g->WN = ns / 64;
  // 4-wave workgroups while the X fragments are small (more workgroups per CU under the register budget), else 8
  g->NW = K <= 128 ? 4 : 8;
  if (g->NW < g->WN) g->NW = g->WN;
  g->WM = g->NW / g->WN;
  g->gy = N / ns;
  g->lds = (size_t)ns * rowb + (size_t)g->NW * kOutTileB;
  const int nblk = (M + 31) / 32;
  // persistent workgroups: a few per CU over the whole grid; rows must divide M for the statistics kernel
  const int want = std::max(1, (256 * (g->NW == 4 ? 3 : 2)) / g->gy);
  int gx = std::max(1, std::min((nblk + g->WM - 1) / g->WM, want));
  // the statistics kernel takes (rows, M / rows): prefer a grid whose workgroup count divides M, else pad
  // the partial buffer with zero rows up to the next divisor of M
  for (int t = gx; t >= std::max(1, gx - gx / 4); --t)
    if (M % t == 0) { gx = t; break; }
  const int rows = pad_rows_to_divisor(M, gx);
  if (!rows) return false;
  g->gx = gx;
  g->rows = rows;
  return true;
}

// The kernel form of a shape, asked in this order: the streaming kernel of conv1x1_wide.hip (N % 256 == 0), the narrow kernel
// of this file (*g: its geometry), the K-streaming kernel of conv1x1_kstream.hip (K >= 512)
enum class Form { none, wide, narrow, kstream };

static Form conv1x1_form(int M, int K, int N, GemmGeo* g) {
  if (conv1x1_wide_rows(M, K, N) > 0) return Form::wide;
  if (conv1x1_geo(g, M, K, N)) return Form::narrow;
  return conv1x1_kstream_supported(M, K, N) ? Form::kstream : Form::none;
}

int conv1x1_rows(int M, int K, int N) {
  GemmGeo g;
  switch (conv1x1_form(M, K, N, &g)) {
    case Form::wide: return conv1x1_wide_rows(M, K, N);
    case Form::narrow: return g.rows;
    case Form::kstream: return conv1x1_kstream_rows(M, K, N);      // one record row per pixel tile
    default: return MRLA_EUNSUPPORTED;
  }
}

// {32-pixel blocks per workgroup (wide form) / per pixel-wave (narrow form), pipeline depth in blocks, workgroups, rows}
// add: the fp32 addend of mrla_conv1x1_fwd_add, which only the wide form has
int conv1x1_plan(int M, int K, int N, int add, int* out) {
  GemmGeo g;
  const Form form = conv1x1_form(M, K, N, &g);
  if (form == Form::wide) return conv1x1_wide_plan(M, K, N, add, out);
  if (add || form == Form::none) return MRLA_EUNSUPPORTED;
  if (form == Form::kstream) {
    out[0] = K / 32; out[1] = conv1x1_kstream_stages(M, K, N); out[2] = 0; out[3] = conv1x1_kstream_rows(M, K, N);   // 32-deep chunks per tile, LDS stages, -, record rows
    return MRLA_OK;
  }
  const int nblk = (M + 31) / 32;
  out[0] = (nblk + g.gx * g.WM - 1) / (g.gx * g.WM);
  out[1] = 2;                               // the next block's X fragments are fetched during this block's MFMAs
  out[2] = g.gx * g.gy;
  out[3] = g.rows;
  return MRLA_OK;
}

// The narrow instance of a geometry: f(KS, NW) with both as integral constants.  conv1x1_geo() takes eight waves at K = 256:
// no four-wave instance there.
template <typename F>
static int narrow_instance(int K, int NW, F&& f) {
  switch (K) {
    case 64: return NW == 4 ? f(Int<4>(), Int<4>()) : f(Int<4>(), Int<8>());
    case 128: return NW == 4 ? f(Int<8>(), Int<4>()) : f(Int<8>(), Int<8>());
    case 256: return NW == 8 ? f(Int<16>(), Int<8>()) : MRLA_EUNSUPPORTED;
    default: return MRLA_EUNSUPPORTED;
  }
}

int launch_conv1x1_fwd(const void* x, const void* w, void* y, float* part, int M, int K, int N, int dtype, hipStream_t st) {
  if (dtype != MRLA_BF16 && dtype != MRLA_F16) return MRLA_EUNSUPPORTED;
  GemmGeo g;
  switch (conv1x1_form(M, K, N, &g)) {
    case Form::wide: return launch_conv1x1_wide(x, w, nullptr, y, part, M, K, N, dtype, st);
    case Form::kstream: return launch_conv1x1_kstream(x, w, y, part, M, K, N, dtype, st);
    case Form::none: return MRLA_EUNSUPPORTED;
    case Form::narrow: break;
  }
  const dim3 grid(g.gx, g.gy), block(g.NW * kWave);
  return narrow_instance(K, g.NW, [&](auto ks, auto nw) {
    constexpr int KS = decltype(ks)::value, NW = decltype(nw)::value;
    return part ? launch_by_dtype(dtype, conv1x1_fwd_kernel<KS, true, NW>, conv1x1_fwd_f16_kernel<KS, true, NW>, grid, block,
                                  g.lds, st, x, w, y, part, M, N, g.NS, g.WN, g.rows)
                : launch_by_dtype(dtype, conv1x1_fwd_kernel<KS, false, NW>, conv1x1_fwd_f16_kernel<KS, false, NW>, grid, block,
                                  g.lds, st, x, w, y, part, M, N, g.NS, g.WN, g.rows);
  });
}

int conv1x1_addend_supported(int M, int K, int N) {
  if ((size_t)M * std::max(N, K) * 2 >= (size_t)1 << 31) return 0;      // (also keeps every pixel index exact in fp32)
  GemmGeo g;
  return conv1x1_form(M, K, N, &g) != Form::none;
}

// The same dispatch as launch_conv1x1_fwd, with the addend (conv1x1_addend.h; sh = sw = 1: as large as y).  The wide form
// adds in fp32 before its one rounding (mrla_conv1x1_fwd_add); the narrow and the K-streaming form add to the rounded output.
int launch_conv1x1_addend(const void* x, const void* w, const void* addend, void* y, int M, int K, int N, int b, int h, int wd,
                          int sh, int sw, int dtype, hipStream_t st) {
  if (dtype != MRLA_BF16 && dtype != MRLA_F16) return MRLA_EUNSUPPORTED;
  if (!conv1x1_addend_supported(M, K, N)) return MRLA_EUNSUPPORTED;
  GemmGeo g;
  switch (conv1x1_form(M, K, N, &g)) {
    case Form::wide:
      return sh * sw == 1 ? launch_conv1x1_wide(x, w, addend, y, nullptr, M, K, N, dtype, st)
                          : launch_conv1x1_wide_sparse(x, w, addend, y, M, K, N, b, h, wd, sh, sw, dtype, st);
    case Form::kstream: return launch_conv1x1_kstream_addend(x, w, addend, y, M, K, N, b, h, wd, sh, sw, dtype, st);
    case Form::none: return MRLA_EUNSUPPORTED;
    case Form::narrow: break;
  }
  const dim3 grid(g.gx, g.gy), block(g.NW * kWave);
  const AddendGeo ag = make_addend_geo(b, h, wd, sh, sw);
  return narrow_instance(K, g.NW, [&](auto ks, auto nw) {
    constexpr int KS = decltype(ks)::value, NW = decltype(nw)::value;
    return launch_by_dtype(dtype, conv1x1_fwd_addend_kernel<KS, NW>, conv1x1_fwd_f16_addend_kernel<KS, NW>, grid, block, g.lds,
                           st, x, w, addend, y, M, N, g.NS, g.WN, ag);
  });
}

// The same dispatch as launch_conv1x1_fwd (same planners, grids and LDS sizes) with the eval-mode BatchNorm's affine
// (+ReLU) applied to the rounded product on its way out (conv1x1_affine.h).  No moment records.
int conv1x1_affine_supported(int M, int K, int N) {
  GemmGeo g;
  return conv1x1_form(M, K, N, &g) != Form::none;
}

int launch_conv1x1_affine(const void* x, const void* w, const float* sc, const float* sh, int relu, void* y, int M, int K,
                          int N, int dtype, hipStream_t st) {
  if (dtype != MRLA_BF16 && dtype != MRLA_F16) return MRLA_EUNSUPPORTED;
  GemmGeo g;
  switch (conv1x1_form(M, K, N, &g)) {
    case Form::wide: return launch_conv1x1_wide_affine(x, w, sc, sh, relu, y, M, K, N, dtype, st);
    case Form::kstream: return launch_conv1x1_kstream_affine(x, w, sc, sh, relu, y, M, K, N, dtype, st);
    case Form::none: return MRLA_EUNSUPPORTED;
    case Form::narrow: break;
  }
  const dim3 grid(g.gx, g.gy), block(g.NW * kWave);
  return narrow_instance(K, g.NW, [&](auto ks, auto nw) {
    constexpr int KS = decltype(ks)::value, NW = decltype(nw)::value;
    return launch_by_dtype(dtype, conv1x1_fwd_affine_kernel<KS, NW>, conv1x1_fwd_f16_affine_kernel<KS, NW>, grid, block, g.lds,
                           st, x, w, sc, sh, relu, y, M, N, g.NS, g.WN);
  });
}

}  // namespace mrla
