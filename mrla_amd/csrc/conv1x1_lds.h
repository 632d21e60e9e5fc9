// What the 1x1-convolution GEMMs (conv1x1.hip, conv1x1_wide.hip, conv1x1_kstream.hip, conv1x1_wgrad.hip, conv1x1_f32.hip)
// share, written once: the inline-asm LDS accesses of the LDS-DMA pipelines with their explicit fence, the swizzle of a staged
// output tile, and on the host the padding of moment-record rows to a divisor of M (the launch of a kernel and the choice between
// the bf16 and the fp16 kernel of a pair: mrla_launch.h, which every launcher shares).  Everything has internal linkage: each
// translation unit compiles its own copy, as it did when the text stood in each file (conv_spatial.h is the same for the
// spatial convolutions).  The swizzles of the OPERAND tiles (cw_swz, ks_swz, swz) stay in their files: each belongs to
// that kernel's DMA plan and read pattern.
//
// Why the LDS accesses are inline asm: the compiler treats an LDS-DMA load as a write to all of LDS and puts
// `s_waitcnt vmcnt(0)` in front of every LDS access it can see, which would drain the stages still in flight.  Ordering is
// explicit instead: lds_read16 only starts a read, lds_fence<N> waits until at most N newer LDS operations are
// outstanding and ties the registers to that wait.
#pragma once
#include "mrla_launch.h"

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

// The statistics kernel takes (rows, M / rows): `count` moment-record rows padded with empty ones up to the next divisor
// of M, or 0 where there is none up to 2 * count + 64
inline int pad_rows_to_divisor(int M, int count) {
  int rows = count;
  while (rows <= 2 * count + 64 && M % rows) ++rows;
  return M % rows ? 0 : rows;
}

}  // namespace
}  // namespace mrla
