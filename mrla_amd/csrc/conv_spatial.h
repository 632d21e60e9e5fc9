// What the spatial-convolution kernels (conv3x3_wgrad.hip, stem_wgrad.hip, conv3x3_fwd.hip, conv3x3_dgrad.hip) share, written once: the
// transposing LDS read and its lane geometry, the swizzled offset of a 128-byte tile row, the walk of a workgroup over its
// output rows, the fixed-order sum of fp32 partial tiles, and on the host the 3x3 raster geometry and the split of the
// output rows over workgroups.  Everything has internal linkage: each of the three translation units compiles its own
// copy, as it did when the text stood in each file.
//
// Ownership.  A workgroup owns one output tile and a FIXED range of output rows (a row = one image row of the output side;
// rows are numbered image after image).  It walks the range in steps of R rows of ONE image (row_step) -- or, for rows wider
// than a step, column segments of one row, one after the other.  No atomics and no memset anywhere: a result is a function
// of the arguments and the shape alone.
//
// Borders of a 3x3 step without per-lane masks (raster3x3 sizes the rasters; the two 3x3 kernels each keep their copy of
// the loader loop, because as a shared inline function it compiled to another instruction stream in both -- a fix to the
// loop's predicate belongs in conv3x3_wgrad.hip AND conv3x3_fwd.hip).  The output-side pixel (ry, j) of a step is raster row
// p = ry*PY + j; X pixel (ty, cx) -- input row yo0*s - 1 + ty, input column xo0*s - 1 + cx -- sits at tile row ty*PX + cx
// with PX = s*PY, so the X pixel that tap (kh, kw) pairs with p is X tile row (s*ry + kh)*PX + s*j + kw
// = s*p + s*(s-1)*PY*ry + kh*PX + kw: a tap is a constant offset from a row the lane computes once (s*p itself at stride 1).
// Everything in the X raster that is no pixel of this step -- X pixels outside the image, rows above the first and below
// the last row of the image (NOT the neighbouring image's rows), the tail behind the last row a tap reads -- is written as
// zeros by the loader, whose every global load is predicated on the pixel's own coordinates: nothing is read outside x.
#pragma once
#include <algorithm>

#include "conv1x1_elem.h"
#include "mrla_device.h"
#include "mrla_kernels.h"

namespace mrla {
namespace {

typedef short tr_s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) tr_s16x4* tr_lds_s16x4_ptr;

constexpr int kTileRowB = 128;          // bytes of a tile row: 64 16-bit channels of one pixel (or of one (n, tap))

// Half of a 32x32x16 operand by gfx950's transposing LDS read: 4 pixels x 16 channels per 16 lanes, 8 bytes per lane at an
// 8-byte-aligned address of its own
__device__ __forceinline__ tr_s16x4 tr16_read(const unsigned char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_lds_s16x4_ptr)p);
}
// ... and the operand: lo = this lane's pixel of the k-step's first eight, hi = of its second eight
template <typename T>
__device__ __forceinline__ typename Elem16<T>::x8 tr16_frag(const unsigned char* lo_ptr, const unsigned char* hi_ptr) {
  return __builtin_bit_cast(typename Elem16<T>::x8, __builtin_shufflevector(tr16_read(lo_ptr), tr16_read(hi_ptr), 0, 1, 2, 3, 4, 5, 6, 7));
}

// Byte offset of 16-byte chunk `chunk` of tile row `row`: the chunk sits at position chunk ^ (((row >> 1) & MASK) << SHIFT).
// <1, 2> is conv1x1_wgrad.hip's swizzle for the transposing read (conflict-free at stride 1, two-way where a half-wave reads
// every other row), <7, 0> the one for ds_read_b128 groups that read one chunk of 16 rows.
template <int MASK, int SHIFT>
__device__ __forceinline__ int tile_off(int row, int chunk) {
  return row * kTileRowB + ((chunk ^ (((row >> 1) & MASK) << SHIFT)) << 4);
}

// The lane's place in a 32x32x16 operand read from a pixel-major tile with tr16_frag: its pixel of a 16-pixel k-step (the
// second read is 4 pixels on), and the first of its 4 columns (channels) of the 32-column block that begins at column
// `block`; a column's chunk and the byte offset inside it.
__device__ __forceinline__ int tr_krel(int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3;
  return 8 * (g >> 1) + q;
}
__device__ __forceinline__ int tr_col(int block, int lane) {
  const int g = lane >> 4, pp = lane & 3;
  return block + 16 * (g & 1) + 4 * pp;
}
__device__ __forceinline__ int tr_chunk(int col) { return col >> 3; }
__device__ __forceinline__ int tr_sub(int col) { return ((col >> 2) & 1) * 8; }

// The step that begins at output row r of a range ending at r_end: at most rmax rows, of one image
struct RowStep {
  int img, yo0, R;
};
__device__ __forceinline__ RowStep row_step(int r, int r_end, int ho, int rmax) {
  RowStep s;
  s.img = r / ho;
  s.yo0 = r - s.img * ho;
  s.R = min(rmax, min(ho - s.yo0, r_end - r));
  return s;
}

// dW[e] = part[0][e] + part[1][e] + ... in ascending order of the split; a lane takes four consecutive outputs
template <typename TO>
__global__ __launch_bounds__(256) void split_sum_kernel(const float* __restrict__ part, TO* __restrict__ dW, int splits,
                                                        int total4) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const float4* src = reinterpret_cast<const float4*>(part) + i;
  float4 s = src[0];
#pragma unroll 8
  for (int k = 1; k < splits; ++k) {
    const float4 v = src[(size_t)k * total4];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  TO* o = dW + (size_t)i * 4;
  o[0] = from_f<TO>(s.x); o[1] = from_f<TO>(s.y); o[2] = from_f<TO>(s.z); o[3] = from_f<TO>(s.w);
}

// part[splits][total] -> dw[total] (total % 4 == 0): fp32 where dw_f32 -- the fp32 master weight's gradient directly --
// else the operands' 16-bit type, rounded once
template <typename = void>
int launch_split_sum(const float* part, void* dw, int dw_f32, int dtype, int splits, int total, hipStream_t st) {
  const int total4 = total / 4;
  const dim3 grid((total4 + 255) / 256), block(256);
  if (dw_f32)
    hipLaunchKernelGGL(split_sum_kernel<float>, grid, block, 0, st, part, (float*)dw, splits, total4);
  else if (dtype == MRLA_F16)
    hipLaunchKernelGGL(split_sum_kernel<f16_t>, grid, block, 0, st, part, (f16_t*)dw, splits, total4);
  else
    hipLaunchKernelGGL(split_sum_kernel<bf16_t>, grid, block, 0, st, part, (bf16_t*)dw, splits, total4);
  return hip_status(hipGetLastError());
}

// The raster of a 3x3 step: whole output rows where one fits (pitch = the row + its pads), else pieces of one row; as many
// rows as max_kp1 (stride 1) / max_kp2 (stride 2) raster pixels hold.  kp_cap / xt_cap: tile rows of the output-side raster
// (a multiple of kp_round) and of the X raster.  Refused (ok = 0): anything but b, c, n, h, w >= 1, s in {1, 2}, c and n
// multiples of 64 and b*h*w*max(c, n)*2 < 2^31 (32-bit element offsets).
struct Raster3x3 {
  int ok = 0;
  int ho = 0, wo = 0;
  int py = 0, ws = 0, nseg = 0, rmax = 0;      // raster pitch, output columns per segment, segments per row, rows per step
  int kp_cap = 0, xt_cap = 0;
};
static inline Raster3x3 raster3x3(int b, int c, int n, int h, int w, int s, int max_kp1, int max_kp2, int max_py, int kp_round) {
  Raster3x3 p;
  if (b <= 0 || c <= 0 || n <= 0 || h <= 0 || w <= 0 || (s != 1 && s != 2) || c % 64 || n % 64) return p;
  if ((unsigned long long)b * h * w * std::max(c, n) * 2 >= 1ull << 31) return p;
  p.ho = (h - 1) / s + 1;
  p.wo = (w - 1) / s + 1;
  const int pad = s == 1 ? 2 : 1;                          // s*PY >= the X columns of a segment, s*(ws - 1) + 3
  if (p.wo + pad <= max_py) {
    p.ws = p.wo; p.py = p.wo + pad; p.nseg = 1;
    p.rmax = std::max(1, std::min(p.ho, (s == 1 ? max_kp1 : max_kp2) / p.py));
  } else {
    p.py = max_py; p.ws = max_py - pad; p.nseg = (p.wo + p.ws - 1) / p.ws;
    p.rmax = 1;
  }
  p.kp_cap = (p.rmax * p.py + kp_round - 1) & ~(kp_round - 1);
  p.xt_cap = (s * p.kp_cap + s * (s - 1) * p.py * (p.rmax - 1) + 2 * s * p.py + 3 + 7) & ~7;
  p.ok = 1;
  return p;
}

// `rows` output rows over about target / tiles workgroups per tile: equal ranges of `per` rows, the last one shorter, none
// empty.  No more ranges than rows / floor_rows, and no range shorter than min_per (<= rows).
struct RowSplit {
  int per, count;
};
static inline RowSplit split_rows(long long rows, int tiles, int target, long long floor_rows = 1, long long min_per = 1) {
  const long long want = std::max<long long>(1, std::min<long long>(rows / floor_rows, (target + tiles - 1) / tiles));
  RowSplit r;
  r.per = (int)std::max<long long>((rows + want - 1) / want, min_per);
  r.count = (int)((rows + r.per - 1) / r.per);
  return r;
}

}  // namespace
}  // namespace mrla
