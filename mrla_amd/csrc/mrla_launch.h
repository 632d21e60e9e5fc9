// What the launchers share, written once (host only): the launch of a kernel (LDS opt-in, launch, status) and the step from
// run-time values -- the element type code, booleans, small integers -- to the template arguments of the kernel that is
// launched.  A launcher is its plan, one with_dtype() around a generic lambda, and one launch_kernel() in it:
//
//   return with_dtype(dtype, [&](auto t, auto gelu, auto has_o) {
//     using T = typename decltype(t)::type;
//     return launch_kernel(kernel<T, gelu(), has_o()>, L.grid, L.block, L.lds, st, x, o, ...);
//   }, act, o != nullptr);
//
// Only what the lambda names is instantiated: a combination that is never launched is refused under `if constexpr` with the
// launcher's return code, in front of the launch_kernel() that would name it.  Everything here is a template or inline and
// has internal linkage (each translation unit compiles its own copy, like conv_spatial.h and conv1x1_lds.h); nothing is type
// erased or allocated: a launch costs one switch over the type code and one branch per flag, inlined.
#pragma once
#include <type_traits>

#include "mrla_device.h"
#include "mrla_kernels.h"

namespace mrla {
namespace {

// One launch: the opt-in to more than 48 KB of dynamic LDS (lds_opt_in returns at once for less), the launch, its status.
// The arguments are converted to the kernel's parameter types, so a launcher hands its `const void*` operands on as they
// are.
template <typename... P, typename... A>
inline int launch_kernel(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args) {
  if (lds_opt_in(reinterpret_cast<const void*>(kernel), lds) != hipSuccess) return MRLA_EHIP;
  hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<P>(args)...);
  return hip_status(hipGetLastError());
}
// ... of the kernel of the element type: the bf16 and the fp16 instances of a body are two kernels with two names
template <typename... PB, typename... PH, typename... A>
inline int launch_by_dtype(int dtype, void (*bf16_kernel)(PB...), void (*f16_kernel)(PH...), dim3 grid, dim3 block,
                           size_t lds, hipStream_t st, A... args) {
  if (dtype == MRLA_F16) return launch_kernel(f16_kernel, grid, block, lds, st, args...);
  if (dtype == MRLA_BF16) return launch_kernel(bf16_kernel, grid, block, lds, st, args...);
  return MRLA_EUNSUPPORTED;
}

// A template argument chosen at run time, handed to a generic lambda by value: f(Int<4>()), and `ks()` inside is a constant
template <int V> using Int = std::integral_constant<int, V>;
template <bool V> using Bool = std::integral_constant<bool, V>;
template <typename T> struct Type { using type = T; };

// f(Bool<flag>()...) for run-time flags
template <typename F>
inline int with_flags(F&& f) { return f(); }
template <typename F, typename... Rest>
inline int with_flags(F&& f, bool flag, Rest... rest) {
  if (flag) return with_flags([&](auto... r) { return f(Bool<true>(), r...); }, rest...);
  return with_flags([&](auto... r) { return f(Bool<false>(), r...); }, rest...);
}

// f(Type<float | bf16_t | f16_t>(), Bool<flag>()...) for an element type code, MRLA_EINVAL for any other
template <typename F, typename... Flags>
inline int with_dtype(int dtype, F&& f, Flags... flags) {
  switch (dtype) {
    case MRLA_F32:  return with_flags([&](auto... b) { return f(Type<float>(), b...); }, flags...);
    case MRLA_BF16: return with_flags([&](auto... b) { return f(Type<bf16_t>(), b...); }, flags...);
    case MRLA_F16:  return with_flags([&](auto... b) { return f(Type<f16_t>(), b...); }, flags...);
    default: return MRLA_EINVAL;
  }
}
// ... for the kernels that exist for the 16-bit types only: MRLA_EUNSUPPORTED for any other code
template <typename F, typename... Flags>
inline int with_dtype16(int dtype, F&& f, Flags... flags) {
  switch (dtype) {
    case MRLA_BF16: return with_flags([&](auto... b) { return f(Type<bf16_t>(), b...); }, flags...);
    case MRLA_F16:  return with_flags([&](auto... b) { return f(Type<f16_t>(), b...); }, flags...);
    default: return MRLA_EUNSUPPORTED;
  }
}

}  // namespace
}  // namespace mrla
