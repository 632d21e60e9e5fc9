// What the 1x1 GEMM kernels (conv1x1*.hip) know about their 16-bit element type, in one place per type: the MFMA
// 32x32x16 instruction, the rounding of an fp32 pair to two packed elements (round to nearest even, overflow to +-inf: what
// a torch cast does) and the decode of a packed pair.  Everything else in those kernels moves 16-byte pieces and does not
// look inside them.
#pragma once
#include "mrla_device.h"

namespace mrla {

typedef float c1_f32x16 __attribute__((ext_vector_type(16)));

template <typename T>
struct Elem16;

template <>
struct Elem16<bf16_t> {
  typedef __bf16 x8 __attribute__((ext_vector_type(8)));
  static constexpr int kDtype = 0;                                  // MRLA_BF16
  __device__ static __forceinline__ void mfma(c1_f32x16& c, x8 a, x8 b) {              // c += a b^T
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
  // the two elements of a packed pair: a bf16 is the upper half of its fp32
  __device__ static __forceinline__ float lo(unsigned v) { return __uint_as_float(v << 16); }
  __device__ static __forceinline__ float hi(unsigned v) { return __uint_as_float(v & 0xffff0000u); }
  __device__ static __forceinline__ unsigned pack(float a, float b) {
    typedef bf16_t bf16x2 __attribute__((ext_vector_type(2)));
    bf16x2 pr;
    pr[0] = from_f<bf16_t>(a);
    pr[1] = from_f<bf16_t>(b);
    return __builtin_bit_cast(unsigned, pr);
  }
};

template <>
struct Elem16<f16_t> {
  typedef _Float16 x8 __attribute__((ext_vector_type(8)));
  static constexpr int kDtype = 1;                                  // MRLA_F16
  __device__ static __forceinline__ void mfma(c1_f32x16& c, x8 a, x8 b) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
  __device__ static __forceinline__ float lo(unsigned v) {
    typedef f16_t f16x2 __attribute__((ext_vector_type(2)));
    return to_f(__builtin_bit_cast(f16x2, v)[0]);
  }
  __device__ static __forceinline__ float hi(unsigned v) {
    typedef f16_t f16x2 __attribute__((ext_vector_type(2)));
    return to_f(__builtin_bit_cast(f16x2, v)[1]);
  }
  __device__ static __forceinline__ unsigned pack(float a, float b) {
    typedef f16_t f16x2 __attribute__((ext_vector_type(2)));
    f16x2 pr;
    pr[0] = from_f<f16_t>(a);
    pr[1] = from_f<f16_t>(b);
    return __builtin_bit_cast(unsigned, pr);
  }
};

}  // namespace mrla
