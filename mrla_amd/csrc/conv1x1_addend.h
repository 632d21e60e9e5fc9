// The addend of the 1x1 GEMMs' input-gradient use (mrla_conv1x1_fwd_addend): the gradient that reaches a bottleneck's
// input through its shortcut.  It is either as large as the output (stride 1) or COMPACT: the gradient of a strided
// subsample x[:, :, ::sh, ::sw], a dense channels_last tensor [b, ceil(h/sh), ceil(w/sw), n] whose pixel (i, yc, xc)
// belongs to output pixel (i, yc*sh, xc*sw); the other output pixels have no addend.  The kernels read it in place of the
// zero-filled full-size tensor a scatter would build.
#pragma once
#include "conv1x1_elem.h"
#include "mrla_device.h"

namespace mrla {

struct AddendGeo {
  int h, w, sh, sw, hc, wc;        // output map, strides, compact map (hc = ceil(h/sh), wc = ceil(w/sw))
  int rows;                        // pixels of the addend tensor: b * hc * wc
  float rw, rh, rsh, rsw;          // 1/w, 1/h, 1/sh, 1/sw
};

inline AddendGeo make_addend_geo(int b, int h, int w, int sh, int sw) {
  AddendGeo g;
  g.h = h; g.w = w; g.sh = sh; g.sw = sw;
  g.hc = (h + sh - 1) / sh; g.wc = (w + sw - 1) / sw;
  g.rows = b * g.hc * g.wc;
  g.rw = 1.f / (float)w; g.rh = 1.f / (float)h; g.rsh = 1.f / (float)sh; g.rsw = 1.f / (float)sw;
  return g;
}

// q = n / d, n = remainder, for 0 <= n < 2^24 and 0 < d < 2^24 (rd = 1/d rounded to float): the float quotient is within
// one of the true one (n and d are exact in fp32, the reciprocal and the product carry 2^-23 of relative error, the
// quotient is below 2^24), the remainder says which way.  ~10 VALU instructions, no integer division.
__device__ __forceinline__ int addend_divmod(int& n, int d, float rd) {
  int q = (int)((float)n * rd);
  int r = n - q * d;
  if (r < 0) { r += d; --q; }
  if (r >= d) { r -= d; ++q; }
  n = r;
  return q;
}

// Row of the addend tensor that belongs to output pixel p of M, or -1 when the pixel has none (p >= M, or a pixel the
// subsample skipped).  dense (sh = sw = 1): the pixel itself.
__device__ __forceinline__ int addend_row(const AddendGeo& g, int p, int M) {
  if (p >= M) return -1;
  if (g.sh == 1 && g.sw == 1) return p;              // (uniform)
  int x = p;
  int y = addend_divmod(x, g.w, g.rw);               // y = img * h + y, x = column
  const int img = addend_divmod(y, g.h, g.rh);
  int ym = y, xm = x;
  const int yc = addend_divmod(ym, g.sh, g.rsh), xc = addend_divmod(xm, g.sw, g.rsw);
  return (ym | xm) ? -1 : (img * g.hc + yc) * g.wc + xc;
}

// Descriptor and byte offset for reading addend pieces with bounds-checked buffer loads: a pixel without addend is read at
// an out-of-bounds offset, which returns zeros and moves nothing -- no branch around the load, so a thread's loads issue
// back to back.  (rows * N * 2 < 2^31: conv1x1_addend_supported.)
template <typename T>
__device__ __forceinline__ auto addend_rsrc(const T* A, const AddendGeo& g, int N) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(A), 0, (int)((size_t)g.rows * N * 2), kBufFlags);
}
__device__ __forceinline__ unsigned addend_offset(const AddendGeo& g, int p, int M, int N, int col) {
  const int row = addend_row(g, p, M);
  return row < 0 ? 0x80000000u : ((unsigned)row * (unsigned)N + (unsigned)col) * 2u;
}

// T(float(a) + float(b)) per element of eight packed 16-bit elements: what a separate elementwise add of the stored GEMM
// output and the addend produces (two roundings: the GEMM's and this one)
template <typename T>
__device__ __forceinline__ u32x4 addend_add8(const u32x4& a, const u32x4& b) {
  typedef Elem16<T> E;
  u32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = E::pack(E::lo(a[j]) + E::lo(b[j]), E::hi(a[j]) + E::hi(b[j]));
  return o;
}

}  // namespace mrla
