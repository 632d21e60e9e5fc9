// Channel attention (SE / ECA) behind a BatchNorm2d, channels_last: out = g[b,c] * (sc[c]*y + sh[c]) without the
// BatchNorm's output, the pooled tensor or the expanded gate ever existing at full size ("Channel attention").
//   bn_gate_apply  forward  out = g * fmaf(sc, y, sh)                          (1 read + 1 write)
//                  backward dy  = (e*g)*do + f*y + (h + e*q)                   (2 reads + 1 write)
//   the [b, c] kernels: plane sums and pooled means from mrla_bn_plane_moments' partial rows, the ECA gate and its
//   backward (zero-padded corr1d along c, as gate.hip's Wq / Wk), and the sums BatchNorm's backward needs
//   (mrla_bn_stats_bwd is linear in dz, so the gate enters it through per-(image, channel) rows only).
// Reference statements covered: resnet/models/resnet_mrla_light.py:77-81,105-108 (bn3, then `se` / `eca`),
// modules/eca_module.py:24-34, the pooling and the multiply of modules/se_module.py:19-23.
#include <algorithm>
#include <type_traits>

#include "mrla_device.h"
#include "mrla_kernels.h"
#include "mrla_launch.h"

namespace mrla {
namespace {

template <typename T> struct Vec16 { typedef T type __attribute__((ext_vector_type(16 / sizeof(T)))); };

template <typename T>
__device__ __forceinline__ void load16(const T* __restrict__ p, float (&v)[16 / sizeof(T)]) {
  typedef typename Vec16<T>::type VT;
  const VT t = *reinterpret_cast<const VT*>(p);
#pragma unroll
  for (int i = 0; i < (int)(16 / sizeof(T)); ++i) v[i] = static_cast<float>(t[i]);
}
template <typename T>
__device__ __forceinline__ void store16(T* __restrict__ p, const float (&v)[16 / sizeof(T)]) {
  typedef typename Vec16<T>::type VT;
  VT t;
#pragma unroll
  for (int i = 0; i < (int)(16 / sizeof(T)); ++i) t[i] = static_cast<T>(v[i]);
  *reinterpret_cast<VT*>(p) = t;
}
template <int N>
__device__ __forceinline__ void loadf(const float* __restrict__ p, float (&v)[N]) {
  static_assert(N % 4 == 0, "vector loads of 4 floats");
#pragma unroll
  for (int i = 0; i < N; i += 4) {
    const float4 t = *reinterpret_cast<const float4*>(p + i);
    v[i] = t.x; v[i + 1] = t.y; v[i + 2] = t.z; v[i + 3] = t.w;
  }
}

constexpr int kGateUnr = 4;          // independent 16-byte loads per operand and lane in flight

// grid: (pieces of an image, b), both walked from the END (the statistics pass that ran just before left the end of the
// tensor in the cache).  A workgroup stays inside one image, so its g / q vectors are loaded once; with `fixed`
// ((kThreads * VEC) % C == 0) a thread keeps its channels from iteration to iteration and all coefficients are loaded once.
// nv: 16-byte vectors per image; a workgroup covers vectors [bx * iters * kThreads, (bx + 1) * iters * kThreads) & < nv.
template <typename T, bool BWD>
__global__ __launch_bounds__(kThreads) void bn_gate_apply_kernel(const T* __restrict__ y, const T* __restrict__ go,
                                                                 const float* __restrict__ cb, const float* __restrict__ sc,
                                                                 const float* __restrict__ sh, const float* __restrict__ g,
                                                                 const float* __restrict__ q, T* __restrict__ out, int C,
                                                                 unsigned nv, int iters, int fixed) {
  constexpr int VEC = 16 / sizeof(T);
  const int b = gridDim.y - 1 - blockIdx.y;
  const unsigned bx = gridDim.x - 1 - blockIdx.x;
  const size_t img = (size_t)b * nv * VEC;
  const T* yp = y + img;
  const T* gp = BWD ? go + img : nullptr;
  T* op = out + img;
  const float* gb = g + (size_t)b * C;
  const float* qb = BWD ? q + (size_t)b * C : nullptr;
  // forward: k0 = g, k1 = sc, k2 = sh.   backward: k0 = e*g, k1 = f, k2 = h + e*q
  float k0[VEC], k1[VEC], k2[VEC];
  auto load_coef = [&](int c0) {
    loadf<VEC>(gb + c0, k0);
    if constexpr (!BWD) {
      loadf<VEC>(sc + c0, k1);
      loadf<VEC>(sh + c0, k2);
    } else {
      float cbv[3 * VEC], qv[VEC];
      loadf<3 * VEC>(cb + (size_t)c0 * 3, cbv);
      loadf<VEC>(qb + c0, qv);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        k0[i] = cbv[3 * i] * k0[i];
        k1[i] = cbv[3 * i + 1];
        k2[i] = fmaf(cbv[3 * i], qv[i], cbv[3 * i + 2]);
      }
    }
  };
  auto one = [&](const float (&yv)[VEC], const float (&dv)[VEC], unsigned at) {
    float r[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      if constexpr (!BWD) {
        r[i] = k0[i] * fmaf(k1[i], yv[i], k2[i]);
      } else {
        r[i] = fmaf(k0[i], dv[i], fmaf(k1[i], yv[i], k2[i]));
        if constexpr (sizeof(T) == 2 && !std::is_same<T, bf16_t>::value) r[i] = as_f32_result(r[i]);   // as nhwc_affine_kernel
      }
    }
    store16<T>(op + (size_t)at * VEC, r);
  };
  unsigned v = bx * (unsigned)iters * kThreads + threadIdx.x;
  int it = 0;
  if (fixed) {
    load_coef((int)((threadIdx.x * VEC) % (unsigned)C));
    for (; it + kGateUnr <= iters && v + (kGateUnr - 1) * kThreads < nv; it += kGateUnr, v += kGateUnr * kThreads) {
      float yv[kGateUnr][VEC], dv[kGateUnr][VEC];
#pragma unroll
      for (int u = 0; u < kGateUnr; ++u) {
        load16<T>(yp + (size_t)(v + u * kThreads) * VEC, yv[u]);
        if (BWD) load16<T>(gp + (size_t)(v + u * kThreads) * VEC, dv[u]);
      }
#pragma unroll
      for (int u = 0; u < kGateUnr; ++u) one(yv[u], dv[u], v + u * kThreads);
    }
  }
  for (; it < iters && v < nv; ++it, v += kThreads) {
    if (!fixed) load_coef((int)(((size_t)v * VEC) % (unsigned)C));
    float yv[VEC], dv[VEC];
    load16<T>(yp + (size_t)v * VEC, yv);
    if (BWD) load16<T>(gp + (size_t)v * VEC, dv);
    one(yv, dv, v);
  }
}

// S[b,c] = sum over the image's pixels of y (the nsplit partial rows of mrla_bn_plane_moments; their sums are about
// pivot[c] when one was recorded: S = sum (y - p) + hw*p);  pooled[b,c] = sc*S/hw + sh = the plane mean of the BatchNorm's output
__global__ __launch_bounds__(kThreads) void bn_gate_pool_kernel(const float* __restrict__ amom /*[b*ns, c, 2]*/,
                                                                const float* __restrict__ pivot,
                                                                const float* __restrict__ sc, const float* __restrict__ sh,
                                                                float* __restrict__ S, float* __restrict__ pooled, int BC,
                                                                int C, int HW, int ns) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= BC) return;
  const int b = i / C, c = i - b * C;
  double s = 0.0;
  for (int k = 0; k < ns; ++k) s += amom[(((size_t)b * ns + k) * C + c) * 2];
  if (pivot) s += (double)HW * (double)pivot[c];
  S[i] = (float)s;
  pooled[i] = (float)((double)sc[c] * (s / (double)HW) + (double)sh[c]);
}

// ECA forward, one workgroup per image: g = sigmoid(corr1d(pooled, w)), zero padded along c
__global__ __launch_bounds__(kThreads) void eca_gate_fwd_kernel(const float* __restrict__ pooled,
                                                                const float* __restrict__ w, int ks,
                                                                float* __restrict__ g, int C) {
  extern __shared__ float sm[];                 // [C + 2p]
  const int p = (ks - 1) / 2;
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < C + 2 * p; i += kThreads) {
    const int c = i - p;
    sm[i] = (c >= 0 && c < C) ? pooled[(size_t)b * C + c] : 0.f;
  }
  __syncthreads();
  for (int c = tid; c < C; c += kThreads) {
    float a = 0.f;
    for (int j = 0; j < ks; ++j) a = fmaf(w[j], sm[c + j], a);
    g[(size_t)b * C + c] = 1.0f / (1.0f + expf(-a));
  }
}

// ECA backward, one workgroup per image: da = dg*g*(1-g);  q = corr1d^T(da, w) / hw;  dw_part[b, j] = sum_c da[c] * pooled[c+j-p]
__global__ __launch_bounds__(kThreads) void eca_gate_bwd_kernel(const float* __restrict__ dg, const float* __restrict__ g,
                                                                const float* __restrict__ pooled,
                                                                const float* __restrict__ w, int ks,
                                                                float* __restrict__ q, float* __restrict__ dw_part, int C,
                                                                int HW) {
  extern __shared__ float sm[];
  const int p = (ks - 1) / 2, CPD = C + 2 * p;
  float* das = sm;                              // [CPD] padded da
  float* ps = das + CPD;                        // [CPD] padded pooled
  double* red = reinterpret_cast<double*>(ps + CPD);      // [kWaves]  (2*CPD floats in front: 8-byte aligned)
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < CPD; i += kThreads) {
    const int c = i - p;
    const bool in = c >= 0 && c < C;
    const float gg = in ? g[(size_t)b * C + c] : 0.f;
    das[i] = in ? dg[(size_t)b * C + c] * gg * (1.f - gg) : 0.f;
    ps[i] = in ? pooled[(size_t)b * C + c] : 0.f;
  }
  __syncthreads();
  const float hw = (float)HW;
  for (int c = tid; c < C; c += kThreads) {
    float d = 0.f;
    for (int j = 0; j < ks; ++j) d = fmaf(w[j], das[c - j + 2 * p], d);
    q[(size_t)b * C + c] = d / hw;
  }
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  for (int j = 0; j < ks; ++j) {
    double acc = 0.0;
    for (int c = tid; c < C; c += kThreads) acc += (double)das[p + c] * (double)ps[c + j];
    acc = wave_sum(acc);
    __syncthreads();
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (int i = 0; i < kWaves; ++i) s += red[i];
      dw_part[(size_t)b * ks + j] = (float)s;
    }
  }
}

// (A1, A2)[b,c] = the image's nsplit rows of mrla_bn_plane_dmoments(center = mean) folded: sum do, sum do*(y - mean).
//   q == NULL: dg[b,c] = sum do*z = sc*A2 + (sc*mean + sh)*A1
//   q given  : tmom[b,c,:] = (g*A1 + hw*q,  g*A2 + q*(S - hw*mean)) = (sum dz, sum dz*(y - mean)),  dz = g*do + q
__global__ __launch_bounds__(kThreads) void bn_gate_sums_bwd_kernel(const float* __restrict__ arows /*[b*ns, c, 2]*/,
                                                                    const float* __restrict__ S, const float* __restrict__ g,
                                                                    const float* __restrict__ q, const float* __restrict__ sc,
                                                                    const float* __restrict__ sh,
                                                                    const float* __restrict__ mean, float* __restrict__ dg,
                                                                    float* __restrict__ tmom, int BC, int C, int HW, int ns) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= BC) return;
  const int b = i / C, c = i - b * C;
  double a1 = 0.0, a2 = 0.0;
  const float2* src = reinterpret_cast<const float2*>(arows) + (size_t)b * ns * C + c;
  for (int k = 0; k < ns; ++k) {
    const float2 t = src[(size_t)k * C];
    a1 += t.x;
    a2 += t.y;
  }
  const double m = mean[c];
  if (!q) {
    const double s = sc[c];
    dg[i] = (float)(s * a2 + (s * m + (double)sh[c]) * a1);
  } else {
    const double gg = g[i], qq = q[i], n = (double)HW;
    tmom[(size_t)i * 2] = (float)(gg * a1 + n * qq);
    tmom[(size_t)i * 2 + 1] = (float)(gg * a2 + qq * ((double)S[i] - n * m));
  }
}

}  // namespace

static size_t eca_lds(int C, int ks, bool bwd) {
  const size_t cpd = (size_t)C + 2 * ((ks - 1) / 2);
  return bwd ? 2 * cpd * sizeof(float) + kWaves * sizeof(double) : cpd * sizeof(float);
}

// 1 when the passes here serve the shape, else MRLA_EUNSUPPORTED: whole 16-byte channel vectors, 32-bit vector indices
// inside an image, at most 65535 images, the ECA workgroup's padded rows in LDS.
int bn_gate_supported(int B, int C, int HW, int dtype) {
  if (B > 65535) return MRLA_EUNSUPPORTED;            // the image index is the grid's y dimension
  const int vec = 16 / (int)dtype_size(dtype);
  if (C % vec) return MRLA_EUNSUPPORTED;
  if ((size_t)C * HW >= ((size_t)1 << 31)) return MRLA_EUNSUPPORTED;
  if (eca_lds(C, 65, true) > 48 * 1024) return MRLA_EUNSUPPORTED;
  return 1;
}

int launch_bn_gate_apply(const void* y, const void* go, const float* cb, const float* sc, const float* sh, const float* g,
                         const float* q, void* out, int B, int C, int HW, int dtype, int bwd, hipStream_t st) {
  if (bn_gate_supported(B, C, HW, dtype) != 1) return MRLA_EUNSUPPORTED;
  const int vec = 16 / (int)dtype_size(dtype);
  const unsigned nv = (unsigned)((size_t)C * HW / vec);
  const size_t want = ((size_t)nv + kThreads - 1) / kThreads;          // workgroup iterations per image
  const int iters = (int)std::max<size_t>(1, std::min<size_t>((want * B + 4095) / 4096, 64));
  const dim3 grid((unsigned)((want + iters - 1) / iters), B);
  const int fixed = (kThreads * vec) % C == 0;
  return with_dtype(dtype, [&](auto t, auto back) {
    using T = typename decltype(t)::type;
    return launch_kernel(bn_gate_apply_kernel<T, back()>, grid, dim3(kThreads), 0, st, y, go, cb, sc, sh, g, q, out, C, nv,
                         iters, fixed);
  }, bwd != 0);
}

int launch_bn_gate_pool(const float* amom, const float* pivot, const float* sc, const float* sh, float* S, float* pooled,
                        int B, int C, int HW, hipStream_t st) {
  const int ns = nhwc_bn_splits(B, C, HW);
  hipLaunchKernelGGL(bn_gate_pool_kernel, dim3((B * C + kThreads - 1) / kThreads), dim3(kThreads), 0, st, amom, pivot, sc,
                     sh, S, pooled, B * C, C, HW, ns);
  return hip_status(hipGetLastError());
}

int launch_eca_gate_fwd(const float* pooled, const float* w, int ks, float* g, int B, int C, hipStream_t st) {
  const size_t lds = eca_lds(C, ks, false);
  if (lds > 48 * 1024) return MRLA_EUNSUPPORTED;
  hipLaunchKernelGGL(eca_gate_fwd_kernel, dim3(B), dim3(kThreads), lds, st, pooled, w, ks, g, C);
  return hip_status(hipGetLastError());
}

int launch_eca_gate_bwd(const float* dg, const float* g, const float* pooled, const float* w, int ks, float* q,
                        float* dw_part, float* dw, int B, int C, int HW, hipStream_t st) {
  const size_t lds = eca_lds(C, ks, true);
  if (lds > 48 * 1024) return MRLA_EUNSUPPORTED;
  hipLaunchKernelGGL(eca_gate_bwd_kernel, dim3(B), dim3(kThreads), lds, st, dg, g, pooled, w, ks, q, dw_part, C, HW);
  const int rc = hip_status(hipGetLastError());
  if (rc != MRLA_OK) return rc;
  return launch_reduce_rows(dw_part, dw, B, ks, st);           // fixed summation order: no atomics
}

int launch_bn_gate_sums_bwd(const float* arows, const float* S, const float* g, const float* q, const float* sc,
                            const float* sh, const float* mean, float* dg, float* tmom, int B, int C, int HW,
                            hipStream_t st) {
  const int ns = nhwc_bn_splits(B, C, HW);
  hipLaunchKernelGGL(bn_gate_sums_bwd_kernel, dim3((B * C + kThreads - 1) / kThreads), dim3(kThreads), 0, st, arows, S, g,
                     q, sc, sh, mean, dg, tmom, B * C, C, HW, ns);
  return hip_status(hipGetLastError());
}

}  // namespace mrla
