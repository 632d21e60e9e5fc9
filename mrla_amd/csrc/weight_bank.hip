// bf16 or fp16 working copies of fp32 convolution weights, all of a model in one launch (see mrla_weight_bank_refresh and
// mrla_weight_bank_refresh_dt in include/mrla_hip.h): dst[n, k] = T(src[n, k]) and, where asked for, dst_t[k, n] = its transpose (the operand of the
// input-gradient GEMM dX = dY * W, mrla_conv1x1_fwd with w^T).  Replaces one autocast cast kernel per convolution and
// forward plus one transposing copy per input gradient (~70 tiny launches per resnet50_mrlal step).
// The same for the 3x3 weights whose input gradient runs as a forward convolution on the flipped, transposed weight
// (mrla_conv3x3_weight_bank_refresh): w16 [n][kh][kw][c] and wflip [c][2-kh][2-kw][n], one launch for all of them.
#include "mrla_device.h"
#include "mrla_kernels.h"

namespace mrla {
namespace {

// One 64 x 64 tile by a workgroup of 256: dst[r][k] = T(src[r][k]) and, where dst_t, dst_t[k][r] = the same 16 bits.  The three
// pointers stand at the tile's origin; ld: elements from a row to the next; src_unit: floats from a column of src to the next
// (1: a lane loads 16 bytes).  A lane stores 8 bytes.
template <typename T>
__device__ __forceinline__ void cast_transpose_tile(const float* __restrict__ src, size_t src_ld, int src_unit, T* __restrict__ dst,
                                                    size_t dst_ld, T* __restrict__ dst_t, size_t dst_t_ld,
                                                    unsigned short (*tile)[66]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = threadIdx.x + 256 * i, r = idx >> 4, c4 = (idx & 15) * 4;
    const float* s = src + (size_t)r * src_ld + (size_t)c4 * src_unit;
    float4 v;
    if (src_unit == 1) {
      v = *reinterpret_cast<const float4*>(s);
    } else {
      v.x = s[0]; v.y = s[src_unit]; v.z = s[2 * (size_t)src_unit]; v.w = s[3 * (size_t)src_unit];
    }
    typedef T tx4 __attribute__((ext_vector_type(4)));
    tx4 o;
    o[0] = from_f<T>(v.x); o[1] = from_f<T>(v.y); o[2] = from_f<T>(v.z); o[3] = from_f<T>(v.w);
    *reinterpret_cast<tx4*>(dst + (size_t)r * dst_ld + c4) = o;
    if (dst_t) {
      const unsigned short* u = reinterpret_cast<const unsigned short*>(&o);
      tile[r][c4] = u[0]; tile[r][c4 + 1] = u[1]; tile[r][c4 + 2] = u[2]; tile[r][c4 + 3] = u[3];
    }
  }
  if (!dst_t) return;               // (uniform over the workgroup)
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = threadIdx.x + 256 * i, r = idx >> 4, c4 = (idx & 15) * 4;      // row r of the transposed tile = column r
    typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
    u16x4 o;
    o[0] = tile[c4][r]; o[1] = tile[c4 + 1][r]; o[2] = tile[c4 + 2][r]; o[3] = tile[c4 + 3][r];
    *reinterpret_cast<u16x4*>(reinterpret_cast<unsigned short*>(dst_t) + (size_t)r * dst_t_ld + c4) = o;
  }
}

// grid (max_tiles, entries): a workgroup converts one 64 x 64 tile of one weight
template <typename T>
__device__ __forceinline__ void weight_bank_body(const long long* __restrict__ table) {
  __shared__ unsigned short tile[64][66];
  const long long* e = table + (size_t)blockIdx.y * 4;
  const float* src = reinterpret_cast<const float*>(e[0]);
  T* dst = reinterpret_cast<T*>(e[1]);
  T* dst_t = reinterpret_cast<T*>(e[2]);
  const int n = (int)(e[3] >> 32), k = (int)(e[3] & 0xffffffffLL);
  const int tk = k / 64;
  if ((int)blockIdx.x >= (n / 64) * tk) return;
  const int n0 = (blockIdx.x / tk) * 64, k0 = (blockIdx.x % tk) * 64;
  cast_transpose_tile<T>(src + (size_t)n0 * k + k0, k, 1, dst + (size_t)n0 * k + k0, k,
                         dst_t ? dst_t + (size_t)k0 * n + n0 : nullptr, n, tile);
}

// The 3x3 weights (mrla_conv3x3_weight_bank_refresh): grid (max_tiles, entries), a workgroup converts the 64 x 64 (n, c) tile
// of ONE tap of one weight -- per tap the weight is a matrix [n, c], its copy w16[n][kh][kw][c] that matrix cast, and
// wflip[c][2-kh][2-kw][n] its transpose at the mirrored tap (8 - tap).  The tap is the fastest index of blockIdx.x: the nine
// workgroups that read the same lines of a contiguous [n, c, 3, 3] master (one float in nine each) are neighbours.
template <typename T>
__device__ __forceinline__ void weight_bank_conv3x3_body(const long long* __restrict__ table) {
  __shared__ unsigned short tile[64][66];
  const long long* e = table + (size_t)blockIdx.y * 5;
  const float* src = reinterpret_cast<const float*>(e[0]);
  T* w16 = reinterpret_cast<T*>(e[1]);
  T* wflip = reinterpret_cast<T*>(e[2]);
  const int n = (int)(e[3] >> 32), c = (int)(e[3] & 0xffffffffLL);
  const bool src_cl = e[4] != 0;                       // the master is [n][3][3][c] in memory, else [n][c][3][3]
  const int tc = c / 64;
  if ((int)blockIdx.x >= 9 * (n / 64) * tc) return;
  const int tap = blockIdx.x % 9, t = blockIdx.x / 9;
  const int n0 = (t / tc) * 64, c0 = (t % tc) * 64;
  const float* s = src_cl ? src + ((size_t)n0 * 9 + tap) * c + c0 : src + ((size_t)n0 * c + c0) * 9 + tap;
  cast_transpose_tile<T>(s, (size_t)9 * c, src_cl ? 1 : 9, w16 + ((size_t)n0 * 9 + tap) * c + c0, (size_t)9 * c,
                         wflip + ((size_t)c0 * 9 + (8 - tap)) * n + n0, (size_t)9 * n, tile);
}

__global__ __launch_bounds__(256) void weight_bank_kernel(const long long* __restrict__ table) { weight_bank_body<bf16_t>(table); }
__global__ __launch_bounds__(256) void weight_bank_f16_kernel(const long long* __restrict__ table) { weight_bank_body<f16_t>(table); }
__global__ __launch_bounds__(256) void weight_bank_conv3x3_kernel(const long long* __restrict__ table) { weight_bank_conv3x3_body<bf16_t>(table); }
__global__ __launch_bounds__(256) void weight_bank_conv3x3_f16_kernel(const long long* __restrict__ table) { weight_bank_conv3x3_body<f16_t>(table); }

}  // namespace

int launch_weight_bank_refresh(const long long* table, int entries, int max_tiles, int dtype, hipStream_t st) {
  if (dtype == MRLA_F16) hipLaunchKernelGGL(weight_bank_f16_kernel, dim3(max_tiles, entries), dim3(256), 0, st, table);
  else if (dtype == MRLA_BF16) hipLaunchKernelGGL(weight_bank_kernel, dim3(max_tiles, entries), dim3(256), 0, st, table);
  else return MRLA_EUNSUPPORTED;
  return hip_status(hipGetLastError());
}

int launch_conv3x3_weight_bank_refresh(const long long* table, int entries, int max_tiles, int dtype, hipStream_t st) {
  if (dtype == MRLA_F16) hipLaunchKernelGGL(weight_bank_conv3x3_f16_kernel, dim3(max_tiles, entries), dim3(256), 0, st, table);
  else if (dtype == MRLA_BF16) hipLaunchKernelGGL(weight_bank_conv3x3_kernel, dim3(max_tiles, entries), dim3(256), 0, st, table);
  else return MRLA_EUNSUPPORTED;
  return hip_status(hipGetLastError());
}

}  // namespace mrla
