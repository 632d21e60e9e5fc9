// Weight gradient of a 1x1 stride-1 convolution of channels_last bf16 or fp16 activations as a split-M MFMA GEMM:
//   dW[n, k] = sum_m dY[m, n] * X[m, k]        (M = b*h*w pixels; dY [M, N] and X [M, K] both channel-contiguous)
// Reference: the backward of the bottleneck's conv1 / conv3 (resnet/models/resnet_mrla_light.py:93,100, nn.Conv2d 1x1).
//
// The product sums over the SLOW index of both operands, N x K is small (4 K .. 1 M outputs) and M is huge (12 K .. 800 K):
// the kernel is a stream over pixels -- every byte of dY and X is read once when one workgroup tile covers N x K
// (stages 1-2), and the arithmetic is 10-30 % of the MFMA rate.  So:
//   * a workgroup (4 waves) owns an output tile TN x TK (<= 32 K accumulators, 64 x 64 .. 128 x 256) and a contiguous
//     range of 32-pixel chunks; tiles x splits = one workgroup per CU; every workgroup writes its fp32 partial tile to
//     part[split][N][K] and a second kernel sums the splits in a fixed order (no atomics, no memset);
//   * workgroup ids are spread over the 8 XCDs round-robin, so the ids are re-mapped to make the tiles of ONE pixel
//     range neighbours in time on ONE XCD: the operand chunk they share comes out of that XCD's L2;
//   * the chunk [32 px][TN] of dY and [32 px][TK] of X goes from global memory straight into LDS with LDS-DMA buffer
//     loads (16 B per lane, 1 KB per wave-instruction, no VGPR staging); four stages rotate, one barrier per chunk;
//     pixels beyond M arrive as zeros from the buffer bounds check;
//   * both MFMA operands are COLUMNS of those row-major tiles (lane = channel, 8 consecutive pixels per lane):
//     gfx950's transposing LDS read `ds_read_b64_tr_b16` delivers exactly that (4 pixels x 16 channels per 16 lanes),
//     two reads per 32x32x16 operand.  The DMA places 16-byte chunk c of tile row r at chunk position c ^ f(r)
//     (f = (r & 3) << 2 for rows of >= 256 B, ((r >> 1) & 1) << 2 for 128-B rows), which spreads the four rows a
//     half-wave reads over the four 64-B bank groups: conflict-free;
//   * LDS reads and the barrier are inline asm / bare `s_barrier`: the compiler orders every LDS read it can see (and
//     __syncthreads()) behind ALL outstanding LDS-DMA loads with `s_waitcnt vmcnt(0)`, which would serialise the
//     stages (measured: 1 us per chunk whatever the depth).
//
// The BN form (mrla_conv1x1_wgrad_bn) takes the BatchNorm backward apply pass in front of this GEMM into it: dY is not
// read but formed, dy = e*dz + f*xb + h with dz = g*[sc*xb + sh > 0] (nhwc_affine_flat_kernel<T, true>'s arithmetic and
// rounding), from the gradient g arriving at the BatchNorm's output and the BatchNorm's input xb, the convolution's own
// forward output.  g keeps dY's DMA route, xb gets a DMA tile of its own behind the stage's two (the largest stage,
// 256 x 128, then makes 4 x 40 KB = all of the CU's LDS; one workgroup per CU is the plan anyway).  A lane's 16-byte DMA
// piece covers the same 8 channels in every instruction and stage (the swizzle term depends on the thread alone), so it
// keeps their 40 coefficients in registers, and after ITS OWN counted vmcnt says its pieces of a stage have landed --
// that wait is what orders a wave's LDS reads behind its own DMA -- and before the barrier that publishes the stage, it
// reads its pieces of g and xb back, rewrites g's in place with the rounded dy (zeros for rows >= M) and stores the same
// 16 bytes to dy_out for the input-gradient GEMM (k-tile 0 only: the others get the store offset of a killed chunk, so
// the number of stores in flight, which the counted waits include, is one constant).  The MFMAs then see exactly the
// bytes mrla_bn_act_bwd would have written: bit-identical partial tiles.
//
// The BN + dX form (mrla_conv1x1_wgrad_bn_dx) takes the input-gradient GEMM behind this one into it as well, where ONE
// 256 x 64 tile covers all of N and K (stage 1's conv3 and downsample): dX[m, k] = dy[m, n] W[n, k] for the workgroup's own
// pixel chunks, and no dy_out -- dy, four times the size of X and dX there, never leaves the CU.  The published g tile of a
// stage IS the rounded dy[32 px][256]; two of the four waves (0/1 on even chunks, 2/3 on odd ones) multiply it with their 32
// rows of W^T, which they hold in registers for the whole kernel, with the narrow GEMM's instruction, operand roles and ONE
// accumulation chain in ascending k (conv1x1.hip, conv1x1_fwd_body): bit-identical to that launch on dy_out.  The rounded
// pieces are staged in the stage's xb tile (dead once the stage has been rewritten), and behind the chunk's barrier -- the
// pipeline's own -- all four waves store the 32 whole 128-byte lines, one counted store per wave and chunk.
#include <algorithm>
#include <type_traits>

#include "conv1x1_elem.h"
#include "conv1x1_lds.h"
#include "mrla_device.h"
#include "mrla_kernels.h"

namespace mrla {
namespace {

typedef short wg_s16x4 __attribute__((ext_vector_type(4)));
typedef c1_f32x16 wg_f32x16;
typedef __attribute__((address_space(3))) wg_s16x4* lds_s16x4_ptr;

constexpr int kPC = 32;                 // pixels per stage
constexpr int kWgStages = 4;            // LDS stages: one being read, one being refilled, two in flight
constexpr int kWgWaves = 4;
constexpr int kWgTarget = 256;          // workgroups: one per CU (the stages, not a second workgroup, hide the DMA latency;
                                        // every workgroup costs a partial tile of up to 128 KB written and re-read)

template <int TN, int TK, int PC>
struct WgGeo {
  static constexpr int WN = (TN >= 256 && TK <= 64) ? 4 : (TK >= 256 && TN <= 64) ? 1 : 2;   // waves along n
  static constexpr int WK = kWgWaves / WN;
  static constexpr int WTN = TN / WN, WTK = TK / WK;       // wave tile
  static constexpr int BN = WTN / 32, BK = WTK / 32;       // 32x32 accumulator blocks
  static constexpr int NIY = TN / 64 * (PC / 32), NIX = TK / 64 * (PC / 32);       // DMA wave-instructions per wave and stage
  static constexpr int YB = PC * TN * 2, XB = PC * TK * 2;
  static constexpr int SB = YB + XB;                       // bytes of one stage
  static_assert(BN >= 1 && BK >= 1 && BN * BK <= 8, "wave tile");
};

// chunk swizzle of tile row `row` for rows of CPR 16-byte chunks
template <int CPR>
__device__ __forceinline__ int swz(int row) { return CPR >= 16 ? ((row & 3) << 2) : (((row >> 1) & 1) << 2); }

// LDS byte offset (inside a [kPC][CPR*8] bf16 tile) this lane hands to the transposing read of the 4-pixel x 16-channel
// block it takes part in: pixels row0 .. row0+3 (row0 % 4 == 0), channels ch0 + 16*(group & 1) .. +15 -- so that the
// wave's two 32-lane halves get pixels row0.. and row0+8.. of channels ch0 .. ch0+31 (the 32x32x16 operand map).
template <int CPR>
__device__ __forceinline__ int tr_offset(int lane, int row0, int ch0) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int row = row0 + 8 * (g >> 1) + q;
  const int col = ch0 + 16 * (g & 1) + 4 * p;
  return row * (CPR * 16) + ((((col >> 3) ^ swz<CPR>(row))) << 4) + ((col >> 2) & 1) * 8;
}

// 32x32x16 operand of channels ch0 .. ch0+31 over 16 pixels of a tile: two transposing reads (pixels +0..3 and +4..7 of
// this half-wave's eight) from LDS byte address `addr` = tile + tr_offset(lane, row0, ch0).
// The reads are inline asm on purpose: the compiler treats an LDS-DMA load as a write to all of LDS and puts
// `s_waitcnt vmcnt(0)` in front of every LDS read it can see -- which would drain the chunks still in flight and turn
// the multi-stage pipeline into one DMA round trip per chunk.  Ordering is explicit instead: frag_issue only starts
// the reads, frag_fence<N> waits until at most N newer LDS reads are outstanding and ties the registers to that wait.
struct Frag {
  wg_s16x4 lo, hi;
};
template <int CPR>
__device__ __forceinline__ void frag_issue(Frag& f, unsigned addr) {
  asm volatile("ds_read_b64_tr_b16 %0, %2\n\tds_read_b64_tr_b16 %1, %2 offset:%3"
               : "=&v"(f.lo), "=&v"(f.hi)
               : "v"(addr), "n"(4 * CPR * 16));
}
template <int N>
__device__ __forceinline__ void frag_fence(Frag& f, bool wait) {
  if (wait) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(f.lo), "+v"(f.hi) : "n"(N) : "memory");
  else asm volatile("" : "+v"(f.lo), "+v"(f.hi)::"memory");      // rides on the wait of the fragment fenced just before
}
template <typename T>
__device__ __forceinline__ typename Elem16<T>::x8 frag_value(const Frag& f) {
  return __builtin_bit_cast(typename Elem16<T>::x8, __builtin_shufflevector(f.lo, f.hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// what the BN form reads and writes beside (g = dY's slot, X, part)
struct WgBnArgs {
  const void* xb;                 // [M, N] the BatchNorm's input
  const float *cb, *sc, *sh;      // [N, 3] = (e, f, h); [N]; [N]
  void* dy_out;                   // [M, N]
  int relu;
};

// what the BN + dX form reads and writes beside those (it stores no dy_out)
struct WgDxArgs {
  const void* wt;                 // [K, N] the weight's transposed working copy
  void* dx;                       // [M, K]
};
constexpr int kDxRowB = 64 * 2 + 16;      // padded row of the dX staging tile (64 channels of one pixel), as conv1x1.hip's

// The 16-byte write and the fence of the rewrite and of the dX form are conv1x1_lds.h's.  The read stays written out here:
// its output is early-clobber, and with lds_read16's plain output the two dX kernels compile to another instruction stream.
__device__ __forceinline__ void wg_read16(u32x4& v, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1" : "=&v"(v) : "v"(addr));
}
template <int OFF>
__device__ __forceinline__ void wg_read16_at(u32x4& v, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(v) : "v"(addr), "n"(OFF));
}

// grid: tiles * splits workgroups (tiles = (N/TN)*(K/TK)) padded to a multiple of 8; 256 threads; LDS = ST * SB
// BN: dY is g, and a stage is SB + YB bytes (the xb tile behind the two operand tiles)
// DX (BN, one tile over all of N = 256 and K = 64): dX = dy W as well, no dy_out; grid and LDS as the BN form's
template <typename T, int TN, int TK, int ST, int PC, bool BN, bool DX = false>
__device__ __forceinline__ void conv1x1_wgrad_body(const T* __restrict__ dY, const T* __restrict__ X,
                                                   float* __restrict__ part, int M, int N, int K, int chunks_per_wg,
                                                   int nsplits, const WgBnArgs& bn, const WgDxArgs& dxa = WgDxArgs{}) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef WgGeo<TN, TK, PC> G;
  constexpr int CPRY = TN / 8, CPRX = TK / 8;            // 16-byte chunks per tile row
  constexpr int SB = G::SB + (BN ? G::YB : 0);           // bytes of one stage
  static_assert(G::SB < 65536, "ds offset field");
  static_assert(!DX || (BN && TN == 256 && TK == 64 && PC == 32), "the dX form: one 256 x 64 tile");
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  // Workgroups go to the 8 XCDs round-robin (id % 8), each XCD with its own L2.  The tiles of one pixel range re-read
  // the same dY / X chunks, so they are made neighbours in time ON ONE XCD: XCD x takes the virtual ids
  // x*per .. (x+1)*per-1 in dispatch order, virtual id = split * tiles + tile.
  const int tiles_k = K / TK, tiles = (N / TN) * tiles_k;
  const int per = gridDim.x >> 3;
  const int vid = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (vid >= tiles * nsplits) return;                     // (the grid is padded to a multiple of 8)
  const int split = vid / tiles, tile = vid - split * tiles;
  const int tn = tile / tiles_k, tk = tile - tn * tiles_k;
  const int n0 = tn * TN, k0 = tk * TK;
  const int chunks_total = (M + PC - 1) / PC;
  const int c_begin = split * chunks_per_wg;
  const int nch = min(chunks_per_wg, chunks_total - c_begin);      // >= 1 by construction of the grid

  // ---- DMA plan: wave-instruction u of a stage moves 1 KB = 64/CPR tile rows; this wave issues u = wave + 4*i ----
  const auto rsY = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(dY), 0, (int)((size_t)M * N * 2), kBufFlags);
  const auto rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(X), 0, (int)((size_t)M * K * 2), kBufFlags);
  unsigned voffY[G::NIY], voffX[G::NIX];
#pragma unroll
  for (int i = 0; i < G::NIY; ++i) {
    const int u = wave + kWgWaves * i, row = u * (64 / CPRY) + lane / CPRY, cp = lane % CPRY;
    voffY[i] = (unsigned)(((size_t)c_begin * PC + row) * N * 2 + (n0 + ((cp ^ swz<CPRY>(row)) << 3)) * 2);
  }
#pragma unroll
  for (int i = 0; i < G::NIX; ++i) {
    const int u = wave + kWgWaves * i, row = u * (64 / CPRX) + lane / CPRX, cp = lane % CPRX;
    voffX[i] = (unsigned)(((size_t)c_begin * PC + row) * K * 2 + (k0 + ((cp ^ swz<CPRX>(row)) << 3)) * 2);
  }
  const unsigned advY = (unsigned)PC * N * 2, advX = (unsigned)PC * K * 2;
  // BN: xb has dY's shape, so its pieces are fetched at dY's offsets (and are killed with them)
  const auto rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(BN ? bn.xb : nullptr), 0,
                                                     BN ? (int)((size_t)M * N * 2) : 0, kBufFlags);
  int issued = 0;
  auto issue = [&](int stage) {
    unsigned char* sb = smem_raw + stage * SB;
    const unsigned kill = issued++ < nch ? 0u : 0x80000000u;      // past the range: out of bounds, no memory traffic
#pragma unroll
    for (int i = 0; i < G::NIY; ++i) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsY, (lds_void_ptr)(sb + (wave + kWgWaves * i) * 1024), 16, voffY[i] | kill, 0, 0, 0);
      if constexpr (BN)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void_ptr)(sb + G::SB + (wave + kWgWaves * i) * 1024), 16, voffY[i] | kill, 0, 0, 0);
      voffY[i] += advY;
    }
#pragma unroll
    for (int i = 0; i < G::NIX; ++i) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsX, (lds_void_ptr)(sb + G::YB + (wave + kWgWaves * i) * 1024), 16, voffX[i] | kill, 0, 0, 0);
      voffX[i] += advX;
    }
  };

  // ---- this wave's operand addresses (stage- and k-step-relative) ----
  const int wn = wave / G::WK, wk = wave - wn * G::WK;
  const unsigned lds0 = lds_addr(smem_raw);
  unsigned offA[G::BN], offB[G::BK];
#pragma unroll
  for (int i = 0; i < G::BN; ++i) offA[i] = lds0 + tr_offset<CPRY>(lane, 0, wn * G::WTN + i * 32);
#pragma unroll
  for (int j = 0; j < G::BK; ++j) offB[j] = lds0 + G::YB + tr_offset<CPRX>(lane, 0, wk * G::WTK + j * 32);

  wg_f32x16 acc[G::BN][G::BK];
#pragma unroll
  for (int i = 0; i < G::BN; ++i)
#pragma unroll
    for (int j = 0; j < G::BK; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // ---- BN: this lane's 8 channels, their coefficients, and the rewrite of its own pieces of a stage ----
  float cbv[BN ? 24 : 1], scv[BN ? 8 : 1], shv[BN ? 8 : 1];
  unsigned tbase[BN ? G::NIY : 1], toff = 0;             // byte offsets of the pieces of chunk 0; chunks rewritten * advY
  const auto rsO = __builtin_amdgcn_make_buffer_rsrc(BN ? bn.dy_out : nullptr, 0, BN ? (int)((size_t)M * N * 2) : 0,
                                                     kBufFlags);
  const unsigned tlimit = (unsigned)((size_t)M * N * 2);
  const unsigned skill = tk == 0 ? 0u : 0x80000000u;     // every k-tile rewrites its own copy; k-tile 0 stores dy_out
  if constexpr (BN) {
    // (the row term of the swizzle: instruction i adds 4 * i * (64 / CPRY) rows, a multiple of 8; a stage adds PC)
    const int row0 = wave * (64 / CPRY) + lane / CPRY;
    const int cch = n0 + (((lane % CPRY) ^ swz<CPRY>(row0)) << 3);
#pragma unroll
    for (int i = 0; i < G::NIY; ++i) tbase[i] = voffY[i];
    const float4* c4 = reinterpret_cast<const float4*>(bn.cb + (size_t)cch * 3);
    const float4* s4 = reinterpret_cast<const float4*>(bn.sc + cch);
    const float4* h4 = reinterpret_cast<const float4*>(bn.sh + cch);
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const float4 v = c4[q];
      cbv[4 * q] = v.x; cbv[4 * q + 1] = v.y; cbv[4 * q + 2] = v.z; cbv[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const float4 u = s4[q], v = h4[q];
      scv[4 * q] = u.x; scv[4 * q + 1] = u.y; scv[4 * q + 2] = u.z; scv[4 * q + 3] = u.w;
      shv[4 * q] = v.x; shv[4 * q + 1] = v.y; shv[4 * q + 2] = v.z; shv[4 * q + 3] = v.w;
    }
    // used here, before the first DMA: the compiler's wait for these ordinary loads must not fall into the pipeline (it
    // would be vmcnt(0)), and past this point the values are registers it cannot re-load
#pragma unroll
    for (int q = 0; q < 24; ++q) asm volatile("" : "+v"(cbv[q]));
#pragma unroll
    for (int q = 0; q < 8; ++q) asm volatile("" : "+v"(scv[q]), "+v"(shv[q]));
  }
  // ---- DX: this wave's 32 rows of W^T as MFMA A fragments (all 16 k-steps: 64 registers), the store lane's first offset ----
  // Waves 0/1 take the two 32-channel output blocks of the even chunks, waves 2/3 those of the odd ones.
  u32x4 wa[DX ? 16 : 1];
  const auto rsD = __builtin_amdgcn_make_buffer_rsrc(DX ? dxa.dx : nullptr, 0, DX ? (int)((size_t)M * K * 2) : 0, kBufFlags);
  const unsigned dlimit = (unsigned)((size_t)M * K * 2);
  const int dr = lane & 31, dh = lane >> 5, dblk = wave & 1;
  unsigned doff = 0;                                     // this lane's 16 bytes of the dX lines of the chunk stored next
  if constexpr (DX) {
    const u32x4* wp = reinterpret_cast<const u32x4*>(static_cast<const T*>(dxa.wt) + (size_t)(dblk * 32 + dr) * N + dh * 8);
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) wa[ks] = wp[ks * 2];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) asm volatile("" : "+v"(wa[ks]));      // (pinned in front of the first DMA, as the coefficients)
    doff = (unsigned)(((size_t)c_begin * PC + wave * 8 + (lane >> 3)) * K * 2 + (lane & 7) * 16);
  }
  const int relu = BN ? bn.relu : 0;
  // the pieces this lane's DMA instructions dropped into the stage at byte offset sbo: g -> dy in place and to dy_out.
  // Call it behind the counted vmcnt that covers the stage and in front of the barrier that publishes it.
  auto rewrite = [&](unsigned sbo) {
    u32x4 gq[G::NIY], xq[G::NIY];
    const unsigned at = lds0 + sbo + wave * 1024 + lane * 16;
#pragma unroll
    for (int i = 0; i < G::NIY; ++i) {
      wg_read16(gq[i], at + i * (kWgWaves * 1024));
      wg_read16_at<G::SB>(xq[i], at + i * (kWgWaves * 1024));
    }
#pragma unroll
    for (int i = 0; i < G::NIY; ++i) {
      lds_fence<0>(gq[i], i == 0);
      lds_fence<0>(xq[i], false);
    }
#pragma unroll
    for (int i = 0; i < G::NIY; ++i) {
      const unsigned off = tbase[i] + toff;
      const bool live = off < tlimit;                    // a row at or past M: zeros for the MFMAs, no store
      u32x4 o;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float gv[2] = {Elem16<T>::lo(gq[i][w]), Elem16<T>::hi(gq[i][w])};
        const float xv[2] = {Elem16<T>::lo(xq[i][w]), Elem16<T>::hi(xq[i][w])};
        float y[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int j = 2 * w + e;
          const float z = fmaf(scv[j], xv[e], shv[j]);
          const float dz = (!relu || z > 0.f) ? gv[e] : 0.f;
          y[e] = fmaf(cbv[3 * j], dz, fmaf(cbv[3 * j + 1], xv[e], cbv[3 * j + 2]));
          if constexpr (!std::is_same<T, bf16_t>::value) y[e] = as_f32_result(y[e]);      // (fp16: the apply pass's two roundings)
        }
        o[w] = live ? Elem16<T>::pack(y[0], y[1]) : 0u;
      }
      lds_write16(at + i * (kWgWaves * 1024), o);
      if constexpr (!DX) __builtin_amdgcn_raw_buffer_store_b128(o, rsO, (live ? off : 0x80000000u) | skill, 0, 0);
    }
    toff += advY;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };

  // DX: dX[32 px][32 ch] of the published stage at sbo, the narrow GEMM's arithmetic (conv1x1_fwd_body with KS = 16): A = 32
  // rows of W^T, B = the lane's pixel's 16 bytes of dy per k-step -- a plain read of the rewritten g tile -- ONE chain of 16
  // MFMAs in ascending k, rounding, the half-wave exchange.  The two 16-byte pieces go to the stage's xb tile, which is dead
  // once the stage has been rewritten, as rows of kDxRowB bytes.  Waits for every LDS read of the wave outstanding.
  auto dx_chunk = [&](unsigned sbo) {
    u32x4 bq[16];
    const unsigned rowa = lds0 + sbo + dr * (CPRY * 16);
    const int sw = swz<CPRY>(dr);
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) wg_read16(bq[ks], rowa + (((2 * ks + dh) ^ sw) << 4));
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) lds_fence<0>(bq[ks], ks == 0);
    wg_f32x16 d;
#pragma unroll
    for (int e = 0; e < 16; ++e) d[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks)
      Elem16<T>::mfma(d, __builtin_bit_cast(typename Elem16<T>::x8, wa[ks]), __builtin_bit_cast(typename Elem16<T>::x8, bq[ks]));
    unsigned p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = Elem16<T>::pack(d[2 * i], d[2 * i + 1]);
    // half 0 holds channels {0-3, 8-11, 16-19, 24-27} of its pixel, half 1 the others; after the swaps half 0 holds
    // {0-7, 16-23} and half 1 {8-15, 24-31}
#pragma unroll
    for (int g = 0; g < 2; ++g) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const auto sx = __builtin_amdgcn_permlane32_swap(p[4 * g + q], p[4 * g + 2 + q], false, false);
        p[4 * g + q] = sx[0];
        p[4 * g + 2 + q] = sx[1];
      }
    }
    const unsigned to = lds0 + sbo + G::SB + dr * kDxRowB + (dblk * 32 + dh * 8) * 2;
    lds_write16(to, (u32x4){p[0], p[1], p[2], p[3]});
    lds_write16(to + 32, (u32x4){p[4], p[5], p[6], p[7]});
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  // DX: the 32 lines (128 bytes) of the chunk staged at sbo, one 16-byte piece per lane of the workgroup; behind the
  // barrier that follows the chunk's dx_chunk.  ONE store per wave and chunk whatever M is (a row at or past M: the
  // out-of-range offset), so that the counted waits stay constants.
  auto dx_store = [&](unsigned sbo) {
    u32x4 v;
    wg_read16(v, lds0 + sbo + G::SB + (wave * 8 + (lane >> 3)) * kDxRowB + (lane & 7) * 16);
    lds_fence<0>(v, true);
    __builtin_amdgcn_raw_buffer_store_b128(v, rsD, doff < dlimit ? doff : 0x80000000u, 0, 0);
    doff += advX;
  };

  // ST stages rotate.  Chunks past the range are issued all the same, with an out-of-bounds offset (zeros from the
  // bounds check, no memory traffic): the wait counts stay compile-time constants.
  // The hand-over to the next chunk sits in front of the LAST k-step of a chunk, not between chunks: the wave waits
  // for its part of chunk c+1, meets the others at the barrier (after which chunk c-1's buffer is free for the DMA of
  // chunk c+ST-1), starts the LDS reads of chunk c+1's first k-step, and only then issues the MFMAs of chunk c's
  // last k-step -- barrier skew and LDS latency are covered by MFMAs already queued.
  constexpr int KSN = PC / 16, NF = 2 * (G::BN + G::BK), NI = (BN ? 2 : 1) * G::NIY + G::NIX;
  // BN: the NIY stores of a rewrite count in vmcnt like the loads (in order).  The wave's stream is
  //   I(0) .. I(ST-2) S(0) | S(1) I(ST-1) | S(2) I(ST) | ...   (I = the DMA of a chunk, S = the stores of its rewrite),
  // so when iteration c waits for I(c+1) there are ST-3 later I behind it, and S: ST-3 of them in the steady state,
  // only S(0) in iteration 0 (none at all with three stages).  A smaller count only waits for more, so the constant
  // is the least of these.
  // DX: no S; the one store D(c) of chunk c's dX lines follows the barrier of iteration c, in front of I(c+ST-1), and a
  // killed store D(-1) follows the prologue's barrier:
  //   I(0) .. I(ST-2) D(-1) | D(0) I(ST-1) | D(1) I(ST) | ...
  // so behind I(c+1) there are, in every iteration, ST-3 later I and ST-3 D (iteration 0: I(2) and D(-1); iteration c:
  // D(c-1) and I(c+2)).  The prologue waits for I(0) in front of D(-1): its count is the BN form's.
  constexpr int W_NEXT = (ST - 3) * NI + (DX ? ST - 3 : BN && ST > 3 ? G::NIY : 0);
  static_assert(!DX || ST == 4, "the dX form's store stream is counted for four stages");
  static_assert(KSN % 2 == 0 && ST >= 3 && W_NEXT < 64 && (ST - 2) * NI < 64, "fragment double buffer / stages / vmcnt immediate");
  Frag fa[2][G::BN], fb[2][G::BK];
  auto read_step = [&](int buf, unsigned sbo, int ks) {
#pragma unroll
    for (int i = 0; i < G::BN; ++i) frag_issue<CPRY>(fa[buf][i], offA[i] + sbo + ks * 16 * CPRY * 16);
#pragma unroll
    for (int j = 0; j < G::BK; ++j) frag_issue<CPRX>(fb[buf][j], offB[j] + sbo + ks * 16 * CPRX * 16);
  };
  auto mfma_step = [&](int buf) {
#pragma unroll
    for (int i = 0; i < G::BN; ++i)
#pragma unroll
      for (int j = 0; j < G::BK; ++j)
        Elem16<T>::mfma(acc[i][j], frag_value<T>(fa[buf][i]), frag_value<T>(fb[buf][j]));
  };
#pragma unroll
  for (int j = 0; j < ST - 1; ++j) issue(j);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"((ST - 2) * NI) : "memory");
  if constexpr (BN) rewrite(0);
  __builtin_amdgcn_s_barrier();                         // (bare: __syncthreads() would drain vmcnt as well)
  asm volatile("" ::: "memory");
  if constexpr (DX) __builtin_amdgcn_raw_buffer_store_b128((u32x4){0u, 0u, 0u, 0u}, rsD, 0x80000000u, 0, 0);      // D(-1)
  read_step(0, 0, 0);
  int stage = 0, nxt = ST - 1;
  for (int c = 0; c < nch; ++c) {
    const unsigned sbo = stage * SB;
    stage = stage + 1 == ST ? 0 : stage + 1;
#pragma unroll
    for (int ks = 0; ks < KSN; ++ks) {
      const int cur = ks & 1;
      int pending = NF;                                 // LDS reads issued after this step's own
      if (ks + 1 < KSN) {
        read_step(cur ^ 1, sbo, ks + 1);
      } else if (c + 1 < nch) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(W_NEXT) : "memory");      // my part of chunk c+1 has landed
        if constexpr (BN) rewrite(stage * SB);
        __builtin_amdgcn_s_barrier();                   // everybody's has; everybody is done reading chunk c-1
        asm volatile("" ::: "memory");
        if constexpr (DX) dx_store(sbo);                // chunk c's dX lines: both of its waves staged them in front of the barrier
        issue(nxt);
        nxt = nxt + 1 == ST ? 0 : nxt + 1;
        read_step(0, stage * SB, 0);
      } else {
        pending = 0;
      }
#pragma unroll
      for (int i = 0; i < G::BN; ++i) {
        if (pending) frag_fence<NF>(fa[cur][i], i == 0); else frag_fence<0>(fa[cur][i], i == 0);
      }
#pragma unroll
      for (int j = 0; j < G::BK; ++j) frag_fence<0>(fb[cur][j], false);
      mfma_step(cur);
      if constexpr (DX) {
        if (ks == 0 && (c & 1) == (wave >> 1)) dx_chunk(sbo);      // (behind MFMAs already queued; wave-uniform)
      }
    }
  }
  if constexpr (DX) {              // the last chunk's lines: no hand-over published them
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    dx_store((stage == 0 ? ST - 1 : stage - 1) * SB);
  }

  // ---- partial tile: D[i][j], j = lane % 32 on the lane, i = 8*(e/4) + 4*(lane/32) + e%4 in register e ----
  float* po = part + ((size_t)split * N + n0 + wn * G::WTN) * K + k0 + wk * G::WTK + (lane & 31);
  const int h = lane >> 5;
#pragma unroll
  for (int i = 0; i < G::BN; ++i)
#pragma unroll
    for (int j = 0; j < G::BK; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e)
        po[(size_t)(i * 32 + 8 * (e >> 2) + 4 * h + (e & 3)) * K + j * 32] = acc[i][j][e];
#endif
}

template <int TN, int TK, int ST, int PC>
__global__ __launch_bounds__(kWgWaves* kWave) void conv1x1_wgrad_kernel(const bf16_t* __restrict__ dY,
                                                                        const bf16_t* __restrict__ X,
                                                                        float* __restrict__ part, int M, int N, int K,
                                                                        int chunks_per_wg, int nsplits) {
  conv1x1_wgrad_body<bf16_t, TN, TK, ST, PC, false>(dY, X, part, M, N, K, chunks_per_wg, nsplits, WgBnArgs{});
}
// the fp16 instances (a name of their own: see conv1x1_fwd_f16_kernel in conv1x1.hip)
template <int TN, int TK, int ST, int PC>
__global__ __launch_bounds__(kWgWaves* kWave) void conv1x1_wgrad_f16_kernel(const f16_t* __restrict__ dY,
                                                                            const f16_t* __restrict__ X,
                                                                            float* __restrict__ part, int M, int N, int K,
                                                                            int chunks_per_wg, int nsplits) {
  conv1x1_wgrad_body<f16_t, TN, TK, ST, PC, false>(dY, X, part, M, N, K, chunks_per_wg, nsplits, WgBnArgs{});
}
// the BN form, both types
template <int TN, int TK, int ST, int PC>
__global__ __launch_bounds__(kWgWaves* kWave) void conv1x1_wgrad_bn_kernel(const bf16_t* __restrict__ g,
                                                                           const bf16_t* __restrict__ X,
                                                                           float* __restrict__ part, int M, int N, int K,
                                                                           int chunks_per_wg, int nsplits, WgBnArgs bn) {
  conv1x1_wgrad_body<bf16_t, TN, TK, ST, PC, true>(g, X, part, M, N, K, chunks_per_wg, nsplits, bn);
}
template <int TN, int TK, int ST, int PC>
__global__ __launch_bounds__(kWgWaves* kWave) void conv1x1_wgrad_bn_f16_kernel(const f16_t* __restrict__ g,
                                                                               const f16_t* __restrict__ X,
                                                                               float* __restrict__ part, int M, int N,
                                                                               int K, int chunks_per_wg, int nsplits,
                                                                               WgBnArgs bn) {
  conv1x1_wgrad_body<f16_t, TN, TK, ST, PC, true>(g, X, part, M, N, K, chunks_per_wg, nsplits, bn);
}

// the BN + dX form (256 x 64 only), both types: names of their own, the BN instances above are not touched
template <int ST>
__global__ __launch_bounds__(kWgWaves* kWave) void conv1x1_wgrad_bn_dx_kernel(const bf16_t* __restrict__ g,
                                                                              const bf16_t* __restrict__ X,
                                                                              float* __restrict__ part, int M, int N, int K,
                                                                              int chunks_per_wg, int nsplits, WgBnArgs bn,
                                                                              WgDxArgs dxa) {
  conv1x1_wgrad_body<bf16_t, 256, 64, ST, kPC, true, true>(g, X, part, M, N, K, chunks_per_wg, nsplits, bn, dxa);
}
template <int ST>
__global__ __launch_bounds__(kWgWaves* kWave) void conv1x1_wgrad_bn_dx_f16_kernel(const f16_t* __restrict__ g,
                                                                                  const f16_t* __restrict__ X,
                                                                                  float* __restrict__ part, int M, int N,
                                                                                  int K, int chunks_per_wg, int nsplits,
                                                                                  WgBnArgs bn, WgDxArgs dxa) {
  conv1x1_wgrad_body<f16_t, 256, 64, ST, kPC, true, true>(g, X, part, M, N, K, chunks_per_wg, nsplits, bn, dxa);
}

// dW[e] = sum over splits of part[s][e] in a fixed order: a workgroup takes 64 outputs, its 16 groups of 16 lanes take
// every 16th split with 16-byte loads, LDS folds the groups
template <typename TO>
__device__ __forceinline__ void conv1x1_wgrad_reduce_body(const float* __restrict__ part, TO* __restrict__ dW, int splits,
                                                          int NK) {
  __shared__ float4 red[16][16];
  const int q = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int e = blockIdx.x * 64 + q * 4;                 // NK % 64 == 0
  const float4* src = reinterpret_cast<const float4*>(part + e);
  const size_t pitch = (size_t)NK / 4;
  float4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
  int s = g;
  for (; s + 16 < splits; s += 32) {
    const float4 u = src[(size_t)s * pitch], v = src[(size_t)(s + 16) * pitch];
    a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
    b.x += v.x; b.y += v.y; b.z += v.z; b.w += v.w;
  }
  if (s < splits) {
    const float4 u = src[(size_t)s * pitch];
    a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
  }
  red[g][q] = float4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
  __syncthreads();
  if (threadIdx.x < 64) {
    const int qq = threadIdx.x >> 2, cc = threadIdx.x & 3;
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += reinterpret_cast<const float*>(&red[i][qq])[cc];
    dW[blockIdx.x * 64 + threadIdx.x] = from_f<TO>(t);
  }
}
template <typename TO>
__global__ __launch_bounds__(256) void conv1x1_wgrad_reduce_kernel(const float* __restrict__ part, TO* __restrict__ dW,
                                                                   int splits, int NK) {
  conv1x1_wgrad_reduce_body<TO>(part, dW, splits, NK);
}
__global__ __launch_bounds__(256) void conv1x1_wgrad_reduce_f16_kernel(const float* __restrict__ part, f16_t* __restrict__ dW,
                                                                       int splits, int NK) {
  conv1x1_wgrad_reduce_body<f16_t>(part, dW, splits, NK);
}

struct WgPlan {
  int tn = 0, tk = 0, tiles = 0, splits = 0, chunks_per_wg = 0;
};

// tile = the largest of {256, 128, 64} dividing each extent, shrunk (the larger side first) to <= 32 K accumulators;
// splits so that the grid is one workgroup per CU
WgPlan wgrad_plan(int M, int K, int N) {
  WgPlan p;
  if (M <= 0 || N % 64 || K % 64 || (size_t)M * std::max(N, K) * 2 >= (size_t)1 << 31) return p;
  int tn = N % 256 == 0 ? 256 : N % 128 == 0 ? 128 : 64;
  int tk = K % 256 == 0 ? 256 : K % 128 == 0 ? 128 : 64;
  // (16 K / 8 K accumulators per workgroup on the deep shapes -- fewer fp32 partial tiles -- were measured: no gain, the tile loop
  // bounds them, profiles/r03_notes.md section 9)
  while (tn * tk > 32768) {
    if (tn >= tk) tn /= 2; else tk /= 2;
  }
  p.tn = tn; p.tk = tk;
  p.tiles = (N / tn) * (K / tk);
  const int chunks = (M + kPC - 1) / kPC;
  const int want = std::max(1, std::min(chunks, (kWgTarget + p.tiles - 1) / p.tiles));
  p.chunks_per_wg = (chunks + want - 1) / want;
  p.splits = (chunks + p.chunks_per_wg - 1) / p.chunks_per_wg;
  return p;
}

dim3 wg_grid(const WgPlan& p) { return dim3((p.tiles * p.splits + 7) / 8 * 8); }

// bn [opt]: the BN form -- dy is then g, and a stage carries the xb tile as well
template <int TN, int TK, int ST, int PC>
int launch_tile(const WgPlan& p, const void* dy, const void* x, float* part, int M, int K, int N, int dtype, hipStream_t st,
                const WgBnArgs* bn = nullptr) {
  typedef WgGeo<TN, TK, PC> G;
  static_assert((size_t)ST * (G::SB + G::YB) <= 160 * 1024, "LDS of a CU");
  const dim3 block(kWgWaves * kWave);
  if (bn)
    return launch_by_dtype(dtype, conv1x1_wgrad_bn_kernel<TN, TK, ST, PC>, conv1x1_wgrad_bn_f16_kernel<TN, TK, ST, PC>, wg_grid(p),
                           block, (size_t)ST * (G::SB + G::YB), st, dy, x, part, M, N, K, p.chunks_per_wg, p.splits, *bn);
  return launch_by_dtype(dtype, conv1x1_wgrad_kernel<TN, TK, ST, PC>, conv1x1_wgrad_f16_kernel<TN, TK, ST, PC>, wg_grid(p), block,
                         (size_t)ST * G::SB, st, dy, x, part, M, N, K, p.chunks_per_wg, p.splits);
}

// the BN + dX form: the BN form's grid and LDS (the dX staging lives in the xb tiles)
int launch_tile_dx(const WgPlan& p, const void* g, const void* x, float* part, int M, int K, int N, int dtype, hipStream_t st,
                   const WgBnArgs& bn, const WgDxArgs& dxa) {
  typedef WgGeo<256, 64, kPC> G;
  constexpr size_t lds = (size_t)kWgStages * (G::SB + G::YB);
  static_assert(lds <= 160 * 1024 && kPC * kDxRowB <= G::YB, "LDS of a CU / the staging tile inside the xb tile");
  return launch_by_dtype(dtype, conv1x1_wgrad_bn_dx_kernel<kWgStages>, conv1x1_wgrad_bn_dx_f16_kernel<kWgStages>, wg_grid(p),
                         dim3(kWgWaves * kWave), lds, st, g, x, part, M, N, K, p.chunks_per_wg, p.splits, bn, dxa);
}

}  // namespace

int conv1x1_wgrad_rows(int M, int K, int N) {
  const WgPlan p = wgrad_plan(M, K, N);
  return p.tiles ? p.splits : MRLA_EUNSUPPORTED;
}

// {32-pixel chunks per workgroup, LDS stages, tile n, tile k, splits, output tiles}
int conv1x1_wgrad_plan(int M, int K, int N, int* out) {
  const WgPlan p = wgrad_plan(M, K, N);
  if (!p.tiles) return MRLA_EUNSUPPORTED;
  out[0] = p.chunks_per_wg; out[1] = kWgStages; out[2] = p.tn; out[3] = p.tk; out[4] = p.splits; out[5] = p.tiles;
  return MRLA_OK;
}

// The shapes the BN form takes: the plain form's where it is the faster route.  Every k-tile forms its own copy of dy, so
// with T k-tiles the pair moves (2T + 2) N bytes through the fused form against (T + 4) N with the apply pass: less with one
// k-tile, the same with two, more beyond -- and the kernel trace of the resnet50_mrlal step agrees (profiles/wgrad_bn.md
// section 6): four and eight k-tiles (k = 1024, 2048) lose 11 to 27 us a launch, two k-tiles win where the repeated reads
// stay in the cache (n <= 512) and are level (0.4 and 3.5 us of 118 and 66) at n = 1024 and 2048.
int conv1x1_wgrad_bn_supported(int M, int K, int N) {
  const WgPlan p = wgrad_plan(M, K, N);
  if (!p.tiles) return MRLA_EUNSUPPORTED;
  const int ktiles = K / p.tk;
  return ktiles == 1 || (ktiles == 2 && N <= 512) ? 1 : MRLA_EUNSUPPORTED;
}

// The shapes the BN + dX form takes: the BN form's whose one 256 x 64 tile covers all of N and K, so that the workgroup holds
// whole rows of dy (the reduction of dX) and writes whole rows of dX.
int conv1x1_wgrad_bn_dx_supported(int M, int K, int N) {
  if (conv1x1_wgrad_bn_supported(M, K, N) != 1) return MRLA_EUNSUPPORTED;
  const WgPlan p = wgrad_plan(M, K, N);
  return p.tiles == 1 && p.tn == 256 && p.tk == 64 ? 1 : MRLA_EUNSUPPORTED;
}

// bn [opt]: the BN form -- dy is then g, the gradient at the BatchNorm's output; dxa [opt, with bn]: the BN + dX form
static int launch_wgrad(const void* dy, const void* x, float* part, void* dw, int dw_f32, int M, int K, int N, int dtype,
                        hipStream_t st, const WgBnArgs* bn, const WgDxArgs* dxa = nullptr) {
  const WgPlan p = wgrad_plan(M, K, N);
  if (!p.tiles || (dtype != MRLA_BF16 && dtype != MRLA_F16)) return MRLA_EUNSUPPORTED;
  int rc = MRLA_EUNSUPPORTED;
  if (dxa) {
    if (!bn || conv1x1_wgrad_bn_dx_supported(M, K, N) != 1) return MRLA_EUNSUPPORTED;
    rc = launch_tile_dx(p, dy, x, part, M, K, N, dtype, st, *bn, *dxa);
  } else {
#define MRLA_WG_TILE(A, B) \
  if (p.tn == A && p.tk == B) rc = launch_tile<A, B, kWgStages, kPC>(p, dy, x, part, M, K, N, dtype, st, bn);
    MRLA_WG_TILE(64, 64) MRLA_WG_TILE(64, 128) MRLA_WG_TILE(64, 256) MRLA_WG_TILE(128, 64) MRLA_WG_TILE(128, 128)
    MRLA_WG_TILE(128, 256) MRLA_WG_TILE(256, 64) MRLA_WG_TILE(256, 128)
#undef MRLA_WG_TILE
  }
  if (rc != MRLA_OK) return rc;      // (also a failed launch of the tile kernel: the sum is not enqueued behind it)
  const int NK = N * K;
  const dim3 grid(NK / 64), block(256);
  if (dw_f32)      // the fp32 master weight's gradient directly (no cast kernel behind an autocast convolution)
    return launch_kernel(conv1x1_wgrad_reduce_kernel<float>, grid, block, 0, st, part, dw, p.splits, NK);
  return launch_by_dtype(dtype, conv1x1_wgrad_reduce_kernel<bf16_t>, conv1x1_wgrad_reduce_f16_kernel, grid, block, 0, st, part,
                         dw, p.splits, NK);
}

int launch_conv1x1_wgrad_reduce_f32(const float* part, float* dw, int splits, int NK, hipStream_t st) {
  return launch_kernel(conv1x1_wgrad_reduce_kernel<float>, dim3(NK / 64), dim3(256), 0, st, part, dw, splits, NK);
}

int launch_conv1x1_wgrad(const void* dy, const void* x, float* part, void* dw, int dw_f32, int M, int K, int N, int dtype,
                         hipStream_t st) {
  return launch_wgrad(dy, x, part, dw, dw_f32, M, K, N, dtype, st, nullptr);
}

int launch_conv1x1_wgrad_bn(const void* g, const void* xb, const float* sc, const float* sh, const float* cb, int relu,
                            void* dy_out, const void* x, float* part, void* dw, int dw_f32, int M, int K, int N, int dtype,
                            hipStream_t st) {
  if (conv1x1_wgrad_bn_supported(M, K, N) != 1) return MRLA_EUNSUPPORTED;
  const WgBnArgs bn{xb, cb, sc, sh, dy_out, relu};
  return launch_wgrad(g, x, part, dw, dw_f32, M, K, N, dtype, st, &bn);
}

int launch_conv1x1_wgrad_bn_dx(const void* g, const void* xb, const float* sc, const float* sh, const float* cb, int relu,
                               const void* x, const void* wt, void* dx, float* part, void* dw, int dw_f32, int M, int K, int N,
                               int dtype, hipStream_t st) {
  if (conv1x1_wgrad_bn_dx_supported(M, K, N) != 1) return MRLA_EUNSUPPORTED;
  const WgBnArgs bn{xb, cb, sc, sh, nullptr, relu};
  const WgDxArgs dxa{wt, dx};
  return launch_wgrad(g, x, part, dw, dw_f32, M, K, N, dtype, st, &bn, &dxa);
}

}  // namespace mrla
