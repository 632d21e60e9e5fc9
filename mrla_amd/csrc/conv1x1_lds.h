// What the 1x1-convolution GEMMs (conv1x1.hip, conv1x1_wide.hip, conv1x1_kstream.hip, conv1x1_wgrad.hip, conv1x1_f32.hip)
// share, written once: the inline-asm LDS accesses of the LDS-DMA pipelines with their explicit fence, the swizzle of a staged
// output tile, and on the host the launch of a kernel (LDS opt-in, launch, status), the choice between the bf16 and the fp16
// kernel of a pair, and the padding of moment-record rows to a divisor of M.  Everything has internal linkage: each
// translation unit compiles its own copy, as it did when the text stood in each file (conv_spatial.h is the same for the
// spatial convolutions).  The swizzles of the OPERAND tiles (cw_swz, ks_swz, swz) stay in their files: each belongs to
// that kernel's DMA plan and read pattern.
//
// Why the LDS accesses are inline asm: the compiler treats an LDS-DMA load as a write to all of LDS and puts
// `s_waitcnt vmcnt(0)` in front of every LDS access it can see, which would drain the stages still in flight.  Ordering is
// explicit instead: lds_read16 only starts a read, lds_fence<N> waits until at most N newer LDS operations are
// outstanding and ties the registers to that wait.
#pragma once
#include <type_traits>

#include "mrla_device.h"
#include "mrla_kernels.h"

namespace mrla {
namespace {

__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(size_t)((__attribute__((address_space(3))) const char*)p);
}
__device__ __forceinline__ void lds_read16(u32x4& v, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr));
}
__device__ __forceinline__ void lds_write16(unsigned addr, const u32x4& v) {
  asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
template <int N>
__device__ __forceinline__ void lds_fence(u32x4& v, bool wait) {
  if (wait) asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(v) : "n"(N) : "memory");
  else asm volatile("" : "+v"(v)::"memory");                    // rides on the wait of the piece fenced just before
}

// chunk swizzle of a staged output-tile row (rows of >= 8 16-byte chunks): chunk c of row r sits at chunk position c ^ out_swz(r)
__device__ __forceinline__ int out_swz(int row) { return row & 7; }

// One launch: the opt-in to more than 48 KB of dynamic LDS (lds_opt_in), the launch, its status.  The arguments are
// converted to the kernel's parameter types, so a launcher hands its `const void*` operands on as they are.
template <typename... P, typename... A>
int launch_kernel(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args) {
  if (lds_opt_in(reinterpret_cast<const void*>(kernel), lds) != hipSuccess) return MRLA_EHIP;
  hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<P>(args)...);
  return hip_status(hipGetLastError());
}
// ... of the kernel of the element type: the bf16 and the fp16 instances of a body are two kernels with two names
template <typename... PB, typename... PH, typename... A>
int launch_by_dtype(int dtype, void (*bf16_kernel)(PB...), void (*f16_kernel)(PH...), dim3 grid, dim3 block, size_t lds,
                    hipStream_t st, A... args) {
  if (dtype == MRLA_F16) return launch_kernel(f16_kernel, grid, block, lds, st, args...);
  if (dtype == MRLA_BF16) return launch_kernel(bf16_kernel, grid, block, lds, st, args...);
  return MRLA_EUNSUPPORTED;
}

// A template argument chosen at run time, handed to a generic lambda: f(Int<4>()) and `decltype(ks)::value` inside
template <int V> using Int = std::integral_constant<int, V>;

// The statistics kernel takes (rows, M / rows): `count` moment-record rows padded with empty ones up to the next divisor
// of M, or 0 where there is none up to 2 * count + 64
inline int pad_rows_to_divisor(int M, int count) {
  int rows = count;
  while (rows <= 2 * count + 64 && M % rows) ++rows;
  return M % rows ? 0 : rows;
}

}  // namespace
}  // namespace mrla
