// The per-channel affine of the 1x1 GEMMs' inference use (mrla_conv1x1_fwd_affine): an eval-mode BatchNorm (+ReLU) behind
// the convolution is y = relu?(sc[n] * z + sh[n]) with fixed sc, sh.  The kernels apply it to the ROUNDED product on its way
// out, with the expression and the roundings of the apply pass it replaces (bnact_nhwc.hip, nhwc_affine_flat_kernel):
//   y = T( relu ? fmaxf(fmaf(sc, float(T(acc)), sh), 0) : fmaf(sc, float(T(acc)), sh) )
// so the bytes are those of mrla_conv1x1_fwd followed by mrla_bn_act_fwd(..., MRLA_NHWC).
#pragma once
#include <type_traits>

#include "conv1x1_elem.h"
#include "mrla_device.h"

namespace mrla {

// one element, in fp32.  fp16: the fma's fp32 result is what gets rounded next, as in the apply pass, whose runtime relu
// select sits between the fma and the conversion (as_f32_result: no v_fma_mixlo_f16, which would round the exact result once)
template <typename T>
__device__ __forceinline__ float affine1(float sc, float x, float sh, int relu) {
  float z = fmaf(sc, x, sh);
  if constexpr (!std::is_same<T, bf16_t>::value) z = as_f32_result(z);
  return relu ? fmaxf(z, 0.f) : z;
}

// sc / sh of eight neighbouring channels c0 .. c0 + 7 (c0 % 8 == 0, the arrays 16-byte aligned)
__device__ __forceinline__ void affine_load8(float (&sc8)[8], float (&sh8)[8], const float* __restrict__ sc,
                                             const float* __restrict__ sh, int c0) {
#pragma unroll
  for (int i = 0; i < 8; i += 4) {
    const float4 a = *reinterpret_cast<const float4*>(sc + c0 + i), b = *reinterpret_cast<const float4*>(sh + c0 + i);
    sc8[i] = a.x; sc8[i + 1] = a.y; sc8[i + 2] = a.z; sc8[i + 3] = a.w;
    sh8[i] = b.x; sh8[i + 1] = b.y; sh8[i + 2] = b.z; sh8[i + 3] = b.w;
  }
}

// eight packed 16-bit elements (a 16-byte piece of a pixel's output row) through the affine of their channels
template <typename T>
__device__ __forceinline__ u32x4 affine8(const u32x4& v, const float (&sc8)[8], const float (&sh8)[8], int relu) {
  typedef Elem16<T> E;
  u32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    o[j] = E::pack(affine1<T>(sc8[2 * j], E::lo(v[j]), sh8[2 * j], relu), affine1<T>(sc8[2 * j + 1], E::hi(v[j]), sh8[2 * j + 1], relu));
  return o;
}

}  // namespace mrla
