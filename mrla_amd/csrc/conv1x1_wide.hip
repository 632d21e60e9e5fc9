// 1x1 stride-1 convolution with a wide output (N % 256 == 0) as a streaming MFMA GEMM, BatchNorm-statistics epilogue:
//   Y[M, N] = X[M, K] * W[N, K]^T (+ A[M, N])      K in {64, 128, 256}; bf16 or fp16 in/out, fp32 accumulate
//   part[row, n, 0..3] = per-workgroup moment record of the bf16-ROUNDED outputs of channel n (MRLA_GEMM_MOMENTS):
//                        sum (y - p), sum (y - p)^2, the pivot p (the workgroup's first output of the channel), pixel count
// Reference: the bottleneck's conv3 / bn3 (resnet/models/resnet_mrla_light.py:100-101) and, with the operands swapped
// by the caller (x = dY, w = W^T), the input gradient of conv1 (:93) -- there `A` is the gradient that reaches the
// block input through the shortcut, so the autograd accumulation (a separate 3N elementwise pass) happens in this
// epilogue.
//
// conv1x1.hip fetches every lane's X fragment straight from global memory.  For wide outputs that re-fetches X once
// per 64 output channels, and with K = 256 (512-byte pixel rows, 32 bytes used per row and instruction) the L1 thrashes:
// 1.7 TB/s on 256 -> 1024.  Here:
//   * a workgroup = 8 waves = 256 output channels; wave w keeps ITS 32 rows of W in registers for the whole kernel
//     (A operand, K/4 VGPRs) and walks a contiguous range of 32-pixel blocks;
//   * the X block [32 px][K] goes global -> LDS with LDS-DMA (16 B per lane, whole rows, every byte fetched once per
//     256 output channels); a ring of blocks is in flight; the B operand is one ds_read_b128 per k-step (chunk c of
//     pixel row r sits at chunk position c ^ f(r): conflict-free for the 16-lane groups of ds_read_b128);
//   * workgroup ids are re-mapped so that the channel groups of one pixel range run side by side on one XCD (L2 hits);
//   * the 32 x 256 bf16 output tile is assembled in LDS and leaves as whole 512-byte rows; with `A` the DMA drops the
//     addend tile into that staging buffer first and the epilogue adds in fp32 before the one rounding; SP: the addend
//     is the compact gradient of a strided subsample (conv1x1_addend.h) -- a lane's DMA offset is then computed from its
//     pixel, and a pixel without an addend is fetched at the out-of-bounds offset (zeros, no traffic);
//   * the inference use behind an eval-mode BatchNorm (conv1x1_wide_affine_kernel, AFF; no moments, no addend): the rounded
//     values go through the BatchNorm's per-channel affine and ReLU (conv1x1_affine.h) in the accumulator layout, before
//     the exchange.  There a register's channel depends on the lane half only and the wave's 32 channels are wave-uniform,
//     so the 32 + 32 fp32 coefficients are scalar loads into SGPRs, selected per half -- the row-store lanes would need 16
//     VGPRs for theirs, kept across the MFMAs of every block, which the K = 64 and K = 128 instances do not have to spare;
//   * one barrier per pixel block; LDS traffic of the pipeline is inline asm with explicit waits (conv1x1_lds.h: the
//     compiler would put `s_waitcnt vmcnt(0)` in front of every LDS access it sees after an LDS-DMA load).
#include <algorithm>

#include "conv1x1_addend.h"
#include "conv1x1_affine.h"
#include "conv1x1_lds.h"
#include "mrla_device.h"
#include "mrla_kernels.h"

namespace mrla {
namespace {

typedef c1_f32x16 cw_f32x16;

constexpr int kCwWaves = 8;
constexpr int kCwTN = 256;                // output channels per workgroup
constexpr int kOutB = 32 * kCwTN * 2;     // bytes of an output / addend tile [32 px][256 ch]

template <int KS, bool ADD>
struct CwGeo {
  static constexpr int K = KS * 16;
  static constexpr int XB = 32 * K * 2;                         // X block bytes (4 / 8 / 16 KB)
  static constexpr int NIX = XB / 1024 >= kCwWaves ? XB / 1024 / kCwWaves : 1;   // X DMA instructions per wave and unit
  static constexpr int NIA = ADD ? kOutB / 1024 / kCwWaves : 0;                  // addend DMA instructions (2)
  static constexpr int NI = NIX + NIA;
  // ring depth: ~64 KB of X in flight without the addend, as much as LDS allows with it
  static constexpr int UST = ADD ? (KS == 16 ? 3 : KS == 8 ? 4 : 5) : (KS == 16 ? 5 : KS == 8 ? 8 : 16);
  static constexpr int OST = ADD ? UST : 2;                      // output tiles (with the addend: one per ring slot)
  static constexpr int kXRing = UST * XB;
  static constexpr int kDummy = kXRing + OST * kOutB;            // 1 KB target of the idle waves' dummy DMA (K = 64)
  static constexpr int kLds = kDummy + 1024;
};

// chunk swizzle of X rows (CPR 16-byte chunks per row); the output-tile rows (32 chunks) have out_swz
template <int CPR>
__device__ __forceinline__ int cw_swz(int row) { return CPR >= 16 ? (row & 15) : ((row >> 1) & 7); }

template <typename T, int KS, bool MOM, bool ADD, bool SP, bool AFF = false>
__device__ __forceinline__ void conv1x1_wide_body(const T* __restrict__ X, const T* __restrict__ W, const T* __restrict__ A,
                                                  T* __restrict__ Y, float* __restrict__ part, int M, int N,
                                                  int units_per_wg, int nsplits, int rows_total, AddendGeo ag,
                                                  const float* __restrict__ sc = nullptr,
                                                  const float* __restrict__ sh = nullptr, int relu = 0) {
  static_assert(ADD || !SP, "a compact addend is an addend");
  static_assert(!(AFF && (MOM || ADD)), "the affine form is the plain forward of inference: no records, no addend");
#if defined(__HIP_DEVICE_COMPILE__)
  typedef Elem16<T> E;
  typedef typename E::x8 cw_x8;
  typedef CwGeo<KS, ADD> G;
  constexpr int K = G::K, CPR = K / 8, UST = G::UST;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int r = lane & 31, h = lane >> 5;
  // XCD-aware order (see conv1x1_wgrad.hip): the channel groups of one pixel range are neighbours on one XCD
  const int groups = N / kCwTN;
  const int per = gridDim.x >> 3;
  const int vid = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (vid >= groups * nsplits) return;
  int split = vid / groups, cg = vid - split * groups;
  if (AFF && KS > 4) {       // (uniform, but the division leaves them, and what derives from them, in vector registers, two more
                             // than the K = 128 instance has; K = 64, held to 8 waves, is short of scalar registers instead)
    split = __builtin_amdgcn_readfirstlane(split);
    cg = __builtin_amdgcn_readfirstlane(cg);
  }
  const int nblk = (M + 31) / 32;
  const int u_begin = split * units_per_wg;
  const int nun = min(units_per_wg, nblk - u_begin);            // >= 1 by construction of the grid
  const int n0 = cg * kCwTN + wave * 32;

  // ---- this wave's 32 rows of W, for the whole kernel ----
  cw_x8 wf[KS];
  {
    const u32x4* wp = reinterpret_cast<const u32x4*>(W + (size_t)(n0 + r) * K + h * 8);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) wf[ks] = __builtin_bit_cast(cw_x8, wp[ks * 2]);
  }

  // ---- AFF: the coefficients of this wave's 32 channels (uniform addresses: scalar registers) ----
  float scw[AFF ? 32 : 1], shw[AFF ? 32 : 1];
  if (AFF) {
#pragma unroll
    for (int i = 0; i < 32; ++i) { scw[i] = sc[n0 + i]; shw[i] = sh[n0 + i]; }
  }

  // ---- DMA plan ----
  const auto rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(X), 0, (int)((size_t)M * K * 2), kBufFlags);
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(ADD ? A : X), 0,
                                                     ADD ? (int)((size_t)(SP ? ag.rows : M) * N * 2) : 0, kBufFlags);
  unsigned voffX[G::NIX], voffA[ADD ? G::NIA : 1];
  constexpr bool kIdleWaves = G::XB / 1024 < kCwWaves;          // K = 64: four real X instructions, waves 4-7 issue a dummy
  const bool idle = kIdleWaves && wave >= G::XB / 1024;
#pragma unroll
  for (int i = 0; i < G::NIX; ++i) {
    const int u = wave + kCwWaves * i, row = u * (64 / CPR) + lane / CPR, cp = lane % CPR;
    voffX[i] = idle ? 0x80000000u
                    : (unsigned)(((size_t)u_begin * 32 + row) * K * 2 + ((cp ^ cw_swz<CPR>(row)) << 4));
  }
  if (ADD) {
#pragma unroll
    for (int i = 0; i < G::NIA; ++i) {
      const int u = wave + kCwWaves * i, row = u * 2 + lane / 32, cp = lane % 32;
      // SP: the position inside the pixel's row only; the row is found per unit
      voffA[i] = (unsigned)((SP ? (size_t)0 : ((size_t)u_begin * 32 + row) * N * 2) + cg * (kCwTN * 2) + ((cp ^ out_swz(row)) << 4));
    }
  }
  const unsigned advX = 32u * K * 2, advA = 32u * (unsigned)N * 2;
  int issued = 0;
  auto issue = [&](int slot) {
    const int pix0 = (u_begin + issued) * 32;                    // first pixel of the unit being fetched
    const unsigned kill = issued++ < nun ? 0u : 0x80000000u;     // past the range: out of bounds, no memory traffic
#pragma unroll
    for (int i = 0; i < G::NIX; ++i) {
      unsigned char* dst = idle ? smem_raw + G::kDummy : smem_raw + slot * G::XB + (wave + kCwWaves * i) * 1024;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsX, (lds_void_ptr)dst, 16, voffX[i] | kill, 0, 0, 0);
      voffX[i] += advX;
    }
    if (ADD && !SP) {
#pragma unroll
      for (int i = 0; i < G::NIA; ++i) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void_ptr)(smem_raw + G::kXRing + slot * kOutB + (wave + kCwWaves * i) * 1024),
                                                 16, voffA[i] | kill, 0, 0, 0);
        voffA[i] += advA;
      }
    }
    if (ADD && SP) {
#pragma unroll
      for (int i = 0; i < G::NIA; ++i) {
        const int arow = addend_row(ag, pix0 + (wave + kCwWaves * i) * 2 + lane / 32, M);
        const unsigned vo = arow < 0 ? 0x80000000u : (unsigned)arow * ((unsigned)N * 2) + voffA[i];
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void_ptr)(smem_raw + G::kXRing + slot * kOutB + (wave + kCwWaves * i) * 1024),
                                                 16, vo | kill, 0, 0, 0);
      }
    }
  };

  // ---- addresses ----
  const unsigned lds0 = lds_addr(smem_raw);
  const int fx = cw_swz<CPR>(r);
  const unsigned xrow = lds0 + r * (K * 2);                                  // + slot*XB + (((2ks+h) ^ fx) << 4)
  // this lane's two 16-byte pieces of its pixel's output row: channels wave*32 + h*8 .. and wave*32 + 16 + h*8 ..
  const int oc0 = wave * 4 + h, oc1 = oc0 + 2;
  const unsigned orow = lds0 + G::kXRing + r * (kCwTN * 2);
  const unsigned opc0 = orow + ((oc0 ^ out_swz(r)) << 4), opc1 = orow + ((oc1 ^ out_swz(r)) << 4);
  // cooperative store: thread -> (row, chunk) of the tile, two rows 16 apart
  const int srow = threadIdx.x >> 5, schunk = threadIdx.x & 31;
  const unsigned sld0 = lds0 + G::kXRing + srow * (kCwTN * 2) + ((schunk ^ out_swz(srow)) << 4);
  const unsigned sld1 = sld0 + 16 * (kCwTN * 2);                             // (row + 16: same swizzle, (row+16)&7 == row&7)
  T* yrow = Y + ((size_t)u_begin * 32 + srow) * N + cg * kCwTN + schunk * 8;

  // BatchNorm moments of the rounded outputs, per lane (register = channel, lane = pixel), taken about a pivot: the
  // workgroup's first output of the channel (lane r = 0 of the half-wave in the first unit).  The one-pass variance
  // E[(y-p)^2] - E[y-p]^2 then stays well conditioned when |mean| >> sigma; the per-channel kernel merges the
  // workgroups' records by re-basing them (in double).
  float s1[MOM ? 16 : 1], s2[MOM ? 16 : 1], pv[MOM ? 16 : 1];
  if (MOM) {
#pragma unroll
    for (int i = 0; i < 16; ++i) { s1[i] = 0.f; s2[i] = 0.f; pv[i] = 0.f; }
  }
  const bool ragged_tail = (u_begin + nun) * 32 > M;             // the last unit of this range has pixels past the end

  // ---- pipeline: UST-1 units issued ahead; unit u+1 is waited for in front of unit u's barrier ----
  constexpr int KC = KS < 8 ? KS : 8, NCH = KS / KC;
  constexpr int C_EARLY = (UST - 3) * G::NI > 0 ? (UST - 3) * G::NI : 0;   // DMA instructions allowed in flight
  constexpr int C_STEADY = C_EARLY + (UST - 2) * 2;                        // ... plus the row stores issued since
  static_assert(UST >= 3 && C_STEADY < 64, "vmcnt immediate");
#pragma unroll
  for (int j = 0; j < UST - 1; ++j) issue(j);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"((UST - 2) * G::NI) : "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  int slot = 0, nxt = UST - 1;
  for (int u = 0; u < nun; ++u) {
    const unsigned xs = xrow + slot * G::XB;
    const unsigned os = (ADD ? slot : (u & 1)) * kOutB;
    cw_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    u32x4 xf[2][KC];
#pragma unroll
    for (int ks = 0; ks < KC; ++ks) lds_read16(xf[0][ks], xs + (((2 * ks + h) ^ fx) << 4));
#pragma unroll
    for (int kc = 0; kc < NCH; ++kc) {
      const int cur = kc & 1;
      if (kc + 1 < NCH) {
#pragma unroll
        for (int ks = 0; ks < KC; ++ks) lds_read16(xf[cur ^ 1][ks], xs + (((2 * ((kc + 1) * KC + ks) + h) ^ fx) << 4));
#pragma unroll
        for (int ks = 0; ks < KC; ++ks) lds_fence<KC>(xf[cur][ks], ks == 0);
      } else {
#pragma unroll
        for (int ks = 0; ks < KC; ++ks) lds_fence<0>(xf[cur][ks], ks == 0);
      }
#pragma unroll
      for (int ks = 0; ks < KC; ++ks)
        E::mfma(acc, wf[kc * KC + ks], __builtin_bit_cast(cw_x8, xf[cur][ks]));
    }
    // lane = pixel r; register e = channel 8*(e/4) + 4*h + e%4 of the wave's 32.  Round pairs of neighbours to the element type.
    // (in piece order after the exchange below: piece g = channels 16g + 8h .. 16g + 8h + 7, 16 bytes of the pixel's row)
    unsigned p[8];
    float av[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) av[i] = acc[i];
    if (ADD) {
      // the addend tile is in LDS in piece order: bring the fp32 values into piece order first (swap register quads
      // between the half-waves), add, and round once
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(av[8 * g + q]), __float_as_uint(av[8 * g + 4 + q]), false, false);
          av[8 * g + q] = __uint_as_float(sw[0]);
          av[8 * g + 4 + q] = __uint_as_float(sw[1]);
        }
      u32x4 a0, a1;
      lds_read16(a0, opc0 + os);
      lds_read16(a1, opc1 + os);
      lds_fence<0>(a0, true);
      lds_fence<0>(a1, false);
      const unsigned aw[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        av[2 * i] += E::lo(aw[i]);
        av[2 * i + 1] += E::hi(aw[i]);
      }
    }
    // (AFF: nothing of the affine below may move up among the MFMAs, whose operands leave no register free at K = 64 and 128)
    if (AFF) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = E::pack(av[2 * i], av[2 * i + 1]);
    if (AFF) {
      // register e of lane half h holds channel (e & 3) + 8 * (e >> 2) + 4 * h: per half one of two scalars, selected by the
      // constant lane mask of the upper half.  (The mask is made opaque per block: selects hoisted out of the loop would be
      // 64 more vector registers, and a vector register for h is one more than the K = 64 and K = 128 instances have.)
      unsigned long long upper = 0xffffffff00000000ull;
      asm volatile("" : "+s"(upper));
      auto half_of = [&](float lo, float hi) {
        float o;
        asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(o) : "v"(lo), "v"(hi), "s"(upper));
        return o;
      };
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float yv[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int c = ((2 * i + j) & 3) + 8 * ((2 * i + j) >> 2);
          yv[j] = affine1<T>(half_of(scw[c], scw[c + 4]), j ? E::hi(p[i]) : E::lo(p[i]), half_of(shw[c], shw[c + 4]), relu);
        }
        p[i] = E::pack(yv[0], yv[1]);
      }
    }
    if (MOM) {
      // (pair by pair: the sixteen decoded values need not be live together)
      if (u == 0) {              // (uniform) the pivots: this half-wave's pixel 0, which always exists
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          pv[2 * i] = __shfl(E::lo(p[i]), h * 32, kWave);
          pv[2 * i + 1] = __shfl(E::hi(p[i]), h * 32, kWave);
        }
      }
      if (!(ragged_tail && u == nun - 1)) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float dl = E::lo(p[i]) - pv[2 * i], dh = E::hi(p[i]) - pv[2 * i + 1];
          s1[2 * i] += dl;     s2[2 * i] = fmaf(dl, dl, s2[2 * i]);
          s1[2 * i + 1] += dh; s2[2 * i + 1] = fmaf(dh, dh, s2[2 * i + 1]);
        }
      } else {                   // (uniform) the one unit with pixels past the end: those do not count
        const bool live = (u_begin + u) * 32 + r < M;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float dl = live ? E::lo(p[i]) - pv[2 * i] : 0.f, dh = live ? E::hi(p[i]) - pv[2 * i + 1] : 0.f;
          s1[2 * i] += dl;     s2[2 * i] = fmaf(dl, dl, s2[2 * i]);
          s1[2 * i + 1] += dh; s2[2 * i + 1] = fmaf(dh, dh, s2[2 * i + 1]);
        }
      }
    }
    if (!ADD) {
      // half 0 holds channels {0-3, 8-11, 16-19, 24-27}, half 1 the other four groups; after the swaps half 0 holds
      // {0-7, 16-23} and half 1 {8-15, 24-31}: two 16-byte pieces per lane
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const auto sw = __builtin_amdgcn_permlane32_swap(p[4 * g + q], p[4 * g + 2 + q], false, false);
          p[4 * g + q] = sw[0];
          p[4 * g + 2 + q] = sw[1];
        }
    }
    lds_write16(opc0 + os, (u32x4){p[0], p[1], p[2], p[3]});
    lds_write16(opc1 + os, (u32x4){p[4], p[5], p[6], p[7]});
    // hand-over: my part of unit u+1 has landed, my tile pieces are written; after the barrier everybody's are, and
    // unit u's X block is free for the DMA of unit u+UST-1
    if (u < UST) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(C_EARLY) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(C_STEADY) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    issue(nxt);
    nxt = nxt + 1 == UST ? 0 : nxt + 1;
    slot = slot + 1 == UST ? 0 : slot + 1;
    // whole 512-byte rows out: 32 lanes per pixel row, rows srow and srow + 16
    {
      u32x4 v0, v1;
      lds_read16(v0, sld0 + os);
      lds_read16(v1, sld1 + os);
      lds_fence<0>(v0, true);
      lds_fence<0>(v1, false);
      const int pix = (u_begin + u) * 32 + srow;
      T* yp = yrow + (size_t)u * 32 * N;
      if (pix < M) *reinterpret_cast<u32x4*>(yp) = v0;
      if (pix + 16 < M) *reinterpret_cast<u32x4*>(yp + (size_t)16 * N) = v1;
    }
  }

  if (MOM) {
    // rows beyond the workgroups' own only exist to make the row count divide M: empty records (written by the first range)
    if (split == 0) {
      for (int i = threadIdx.x; i < (rows_total - nsplits) * kCwTN * 4; i += kCwWaves * kWave) {
        const int row = nsplits + i / (kCwTN * 4), j = i % (kCwTN * 4);
        part[((size_t)row * N + cg * kCwTN) * 4 + j] = 0.f;
      }
    }
    const float npix = (float)(min(M, (u_begin + nun) * 32) - u_begin * 32);
    // register e of half h = channel: see the piece layout the values were accumulated in
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float a = s1[i], b = s2[i];
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, kWave);
        b += __shfl_xor(b, off, kWave);
      }
      if (r == 0) {
        const int ch = ADD ? ((i < 8 ? 0 : 16) + h * 8 + (i & 7)) : ((i & 3) + 8 * (i >> 2) + 4 * h);
        float* dst = part + ((size_t)split * N + n0 + ch) * 4;
        dst[0] = a;
        dst[1] = b;
        dst[2] = pv[i];
        dst[3] = npix;
      }
    }
  }
#endif
}

template <int KS, bool MOM, bool ADD, bool SP>
__global__ __launch_bounds__(kCwWaves* kWave) void conv1x1_wide_kernel(const bf16_t* __restrict__ X,
                                                                       const bf16_t* __restrict__ W,
                                                                       const bf16_t* __restrict__ A, bf16_t* __restrict__ Y,
                                                                       float* __restrict__ part, int M, int N,
                                                                       int units_per_wg, int nsplits, int rows_total,
                                                                       AddendGeo ag) {
  conv1x1_wide_body<bf16_t, KS, MOM, ADD, SP>(X, W, A, Y, part, M, N, units_per_wg, nsplits, rows_total, ag);
}
// the fp16 instances (a name of their own: see conv1x1_fwd_f16_kernel)
template <int KS, bool MOM, bool ADD, bool SP>
__global__ __launch_bounds__(kCwWaves* kWave) void conv1x1_wide_f16_kernel(const f16_t* __restrict__ X,
                                                                           const f16_t* __restrict__ W,
                                                                           const f16_t* __restrict__ A, f16_t* __restrict__ Y,
                                                                           float* __restrict__ part, int M, int N,
                                                                           int units_per_wg, int nsplits, int rows_total,
                                                                           AddendGeo ag) {
  conv1x1_wide_body<f16_t, KS, MOM, ADD, SP>(X, W, A, Y, part, M, N, units_per_wg, nsplits, rows_total, ag);
}

// the forward in front of an eval-mode BatchNorm: y = T(relu?(sc * T(x w^T) + sh)) (names of their own, as above)
// Held to the waves per SIMD the plain instances (no moments, no addend) they are launched in place of compile to.
template <int KS> constexpr int kCwAffWaves = KS == 4 ? 8 : KS == 8 ? 5 : 2;
template <int KS>
__global__ __launch_bounds__(kCwWaves* kWave, kCwAffWaves<KS>) void conv1x1_wide_affine_kernel(const bf16_t* __restrict__ X,
                                                                              const bf16_t* __restrict__ W,
                                                                              const float* __restrict__ sc,
                                                                              const float* __restrict__ sh, int relu,
                                                                              bf16_t* __restrict__ Y, int M, int N,
                                                                              int units_per_wg, int nsplits) {
  conv1x1_wide_body<bf16_t, KS, false, false, false, true>(X, W, nullptr, Y, nullptr, M, N, units_per_wg, nsplits, 0,
                                                           AddendGeo(), sc, sh, relu);
}
template <int KS>
__global__ __launch_bounds__(kCwWaves* kWave, kCwAffWaves<KS>) void conv1x1_wide_f16_affine_kernel(const f16_t* __restrict__ X,
                                                                                  const f16_t* __restrict__ W,
                                                                                  const float* __restrict__ sc,
                                                                                  const float* __restrict__ sh, int relu,
                                                                                  f16_t* __restrict__ Y, int M, int N,
                                                                                  int units_per_wg, int nsplits) {
  conv1x1_wide_body<f16_t, KS, false, false, false, true>(X, W, nullptr, Y, nullptr, M, N, units_per_wg, nsplits, 0,
                                                          AddendGeo(), sc, sh, relu);
}

struct CwPlan {
  int groups = 0, splits = 0, units_per_wg = 0, rows = 0;
};

CwPlan cw_plan(int M, int K, int N) {
  CwPlan p;
  if (M <= 0 || (K != 64 && K != 128 && K != 256) || N % kCwTN || (size_t)M * std::max(N, K) * 2 >= (size_t)1 << 31) return p;
  const int groups = N / kCwTN, nblk = (M + 31) / 32;
  const int want = std::max(1, std::min(nblk, (256 + groups - 1) / groups));          // one workgroup per CU
  const int upw = (nblk + want - 1) / want;
  const int splits = (nblk + upw - 1) / upw;
  const int rows = pad_rows_to_divisor(M, splits);
  if (!rows) return p;
  p.groups = groups; p.splits = splits; p.units_per_wg = upw; p.rows = rows;
  return p;
}

// f(KS) with KS = K / 16 as an integral constant, for the K this file takes
template <typename F>
int cw_instance(int K, F&& f) {
  switch (K) {
    case 64: return f(Int<4>());
    case 128: return f(Int<8>());
    case 256: return f(Int<16>());
    default: return MRLA_EUNSUPPORTED;
  }
}

dim3 cw_grid(const CwPlan& p) { return dim3((p.groups * p.splits + 7) / 8 * 8); }

template <int KS, bool MOM, bool ADD, bool SP = false>
int cw_launch(const CwPlan& p, const void* x, const void* w, const void* a, void* y, float* part, int M, int N, int dtype,
              hipStream_t st, const AddendGeo& ag = AddendGeo()) {
  typedef CwGeo<KS, ADD> G;
  static_assert(G::kLds <= 160 * 1024, "LDS");
  return launch_by_dtype(dtype, conv1x1_wide_kernel<KS, MOM, ADD, SP>, conv1x1_wide_f16_kernel<KS, MOM, ADD, SP>, cw_grid(p),
                         dim3(kCwWaves * kWave), G::kLds, st, x, w, a, y, part, M, N, p.units_per_wg, p.splits, p.rows, ag);
}

}  // namespace

int conv1x1_wide_rows(int M, int K, int N) {
  const CwPlan p = cw_plan(M, K, N);
  return p.groups ? p.rows : MRLA_EUNSUPPORTED;
}

// {32-pixel blocks per workgroup, LDS ring depth in blocks, workgroups, moment rows}
int conv1x1_wide_plan(int M, int K, int N, int add, int* out) {
  const CwPlan p = cw_plan(M, K, N);
  if (!p.groups) return MRLA_EUNSUPPORTED;
  out[0] = p.units_per_wg;
  out[2] = p.groups * p.splits;
  out[3] = p.rows;
  return cw_instance(K, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    out[1] = add ? CwGeo<KS, true>::UST : CwGeo<KS, false>::UST;
    return (int)MRLA_OK;
  });
}

int launch_conv1x1_wide(const void* x, const void* w, const void* addend, void* y, float* part, int M, int K, int N,
                        int dtype, hipStream_t st) {
  const CwPlan p = cw_plan(M, K, N);
  if (!p.groups) return MRLA_EUNSUPPORTED;
  return cw_instance(K, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    if (addend) return part ? cw_launch<KS, true, true>(p, x, w, addend, y, part, M, N, dtype, st)
                            : cw_launch<KS, false, true>(p, x, w, addend, y, part, M, N, dtype, st);
    return part ? cw_launch<KS, true, false>(p, x, w, addend, y, part, M, N, dtype, st)
                : cw_launch<KS, false, false>(p, x, w, addend, y, part, M, N, dtype, st);
  });
}

// y = x w^T + the compact addend [b, ceil(h/sh), ceil(w/sw), N] of a strided subsample (see conv1x1_addend.h); M = b*h*w
int launch_conv1x1_wide_sparse(const void* x, const void* w, const void* addend, void* y, int M, int K, int N, int b, int h,
                               int wd, int sh, int sw, int dtype, hipStream_t st) {
  const CwPlan p = cw_plan(M, K, N);
  if (!p.groups) return MRLA_EUNSUPPORTED;
  const AddendGeo ag = make_addend_geo(b, h, wd, sh, sw);
  return cw_instance(K, [&](auto ks) {
    return cw_launch<decltype(ks)::value, false, true, true>(p, x, w, addend, y, nullptr, M, N, dtype, st, ag);
  });
}

// y = T(relu?(sc * T(x w^T) + sh)): the plain forward's plan, grid and LDS, the affine applied before the tile is staged
int launch_conv1x1_wide_affine(const void* x, const void* w, const float* sc, const float* sh, int relu, void* y, int M, int K,
                               int N, int dtype, hipStream_t st) {
  const CwPlan p = cw_plan(M, K, N);
  if (!p.groups) return MRLA_EUNSUPPORTED;
  return cw_instance(K, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    return launch_by_dtype(dtype, conv1x1_wide_affine_kernel<KS>, conv1x1_wide_f16_affine_kernel<KS>, cw_grid(p),
                           dim3(kCwWaves * kWave), CwGeo<KS, false>::kLds, st, x, w, sc, sh, relu, y, M, N, p.units_per_wg,
                           p.splits);
  });
}

}  // namespace mrla
