// T5 encoder around the GEMMs and the attention (transformers T5EncoderModel, the text_encoder_2 of Flux and text_encoder_3
// of SD3): the row RMSNorm, the relative-position bias table and the gated tanh-GELU.  T is 16-bit, arithmetic fp32, one
// rounding at the store.  The RMSNorm and the gated GELU have a backward to their input (the norm weights are frozen); the
// bias table is not differentiated.
#include "kernels.h"

namespace smi {
namespace {

// ---------------------------------------------------------------------------------------------------------------
// y[m, :] = w * x[m, :] * rsqrt(mean(x[m, :]^2) + eps)   (T5LayerNorm: no mean subtracted, no bias)
// A row lives in registers between the two passes: NV 16-byte vectors per lane.  WPR = 1: a wave owns a row (C <= 2048, four
// rows per workgroup, as norm.hip's LayerNorm); WPR = 4: the four waves of a workgroup share one (C <= 8192; T5-XXL's 4096),
// their partial sums meeting in LDS.  The sum of squares, the scale and the weight product are fp32.
// ---------------------------------------------------------------------------------------------------------------
constexpr int RMS_MAXV = 4;
template <typename T, int NV, int WPR>
__global__ __launch_bounds__(256) void rmsnorm_rows_kernel(const T* __restrict__ x, const T* __restrict__ w, T* __restrict__ y,
                                                           int M, int C8, float inv_c, float eps) {
  __shared__ float part[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = WPR == 1 ? blockIdx.x * 4 + wave : blockIdx.x;
  const int v0 = WPR == 1 ? lane : tid;
  constexpr int VS = WPR == 1 ? 64 : 256;  // vectors a step apart
  const bool live = row < M;               // (WPR == 4: uniform over the workgroup, so the barrier below is too)
  const T* xr = x + (int64_t)row * C8 * 8;
  Pack8<T> a[NV];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = v0 + VS * i;
    a[i].u = u32x4{0u, 0u, 0u, 0u};
    if (live && v < C8) a[i].u = *reinterpret_cast<const u32x4*>(xr + (int64_t)v * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float f = to_f(a[i].e[e]);
      ss = __builtin_fmaf(f, f, ss);
    }
  }
  ss = wave_sum(ss);
  if (WPR == 4) {
    if (lane == 0) part[wave] = ss;
    __syncthreads();
    ss = (part[0] + part[1]) + (part[2] + part[3]);
  }
  if (!live) return;
  const float r = rsqrtf(ss * inv_c + eps);
  T* yr = y + (int64_t)row * C8 * 8;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = v0 + VS * i;
    if (v < C8) {
      Pack8<T> g, o;
      g.u = *reinterpret_cast<const u32x4*>(w + (int64_t)v * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) o.e[e] = from_f<T>(to_f(g.e[e]) * (to_f(a[i].e[e]) * r));
      *reinterpret_cast<u32x4*>(yr + (int64_t)v * 8) = o.u;
    }
  }
}

// out[h, o] = weight[bucket[o], h] for o in [0, n_off): T5's bias depends on key - query alone, so the [H, L, L] tensor
// transformers builds is this table read at k - q + L - 1 (attention.hip).  A bucket outside the weight reads row 0
template <typename T>
__global__ void t5_bias_table_kernel(const T* __restrict__ weight, const int* __restrict__ bucket, float* __restrict__ out,
                                     int H, int n_off, int num_buckets) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * n_off) return;
  const int h = i / n_off, o = i - h * n_off;
  int b = bucket[o];
  b = (b < 0 || b >= num_buckets) ? 0 : b;
  out[i] = to_f(weight[(int64_t)b * H + h]);
}

// out[m, c] = gelu_tanh(p[m, c]) * p[m, F + c] on the fused projection wi_0 | wi_1 (transformers T5DenseGatedActDense with
// gelu_new).  The GELU is elementwise.hip's gelu_tanh_f to the letter: with a value half of ones the bits of launch_act kind 2
template <typename T>
__global__ void gated_gelu_tanh_kernel(const T* __restrict__ p, T* __restrict__ out, int64_t M, int F8) {
  const int64_t total = M * F8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t m = i / F8;
    const int v = (int)(i - m * F8);
    Pack8<T> g, u, o;
    g.u = *reinterpret_cast<const u32x4*>(p + (m * 2 * F8 + v) * 8);
    u.u = *reinterpret_cast<const u32x4*>(p + (m * 2 * F8 + F8 + v) * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float f = to_f(g.e[e]);
      const float u2 = 1.5957691216057308f * f * __builtin_fmaf(0.044715f * f, f, 1.f);
      o.e[e] = from_f<T>(f / (1.f + __expf(-u2)) * to_f(u.e[e]));
    }
    *reinterpret_cast<u32x4*>(out + i * 8) = o.u;
  }
}

// dx[m, :] of y = w x r, r = rsqrt(mean(x^2) + eps), for a frozen w:  dx = r (w dy) - x r^3 mean(x . w dy)  (+ add: the
// gradient the residual branch brings to the same rows, summed in fp32 before the one rounding, as launch_layernorm_bwd does).
// r is recomputed from x; the same wave-per-row / workgroup-per-row split as rmsnorm_rows_kernel, x and dy of the row in
// registers between the two passes, w read again from cache in the second.  add may alias dx (each lane reads the vector
// it writes).
template <typename T, int NV, int WPR>
__global__ __launch_bounds__(256) void rmsnorm_rows_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                               const T* __restrict__ w, const T* add, T* dx, int M, int C8,
                                                               float inv_c, float eps) {
  __shared__ float part[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = WPR == 1 ? blockIdx.x * 4 + wave : blockIdx.x;
  const int v0 = WPR == 1 ? lane : tid;
  constexpr int VS = WPR == 1 ? 64 : 256;
  const bool live = row < M;
  const T* xr = x + (int64_t)row * C8 * 8;
  const T* gr = dy + (int64_t)row * C8 * 8;
  Pack8<T> a[NV], g[NV];
  float ss = 0.f, sd = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = v0 + VS * i;
    a[i].u = u32x4{0u, 0u, 0u, 0u};
    g[i].u = u32x4{0u, 0u, 0u, 0u};
    Pack8<T> ww;
    ww.u = u32x4{0u, 0u, 0u, 0u};
    if (live && v < C8) {
      a[i].u = *reinterpret_cast<const u32x4*>(xr + (int64_t)v * 8);
      g[i].u = *reinterpret_cast<const u32x4*>(gr + (int64_t)v * 8);
      ww.u = *reinterpret_cast<const u32x4*>(w + (int64_t)v * 8);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float f = to_f(a[i].e[e]);
      ss = __builtin_fmaf(f, f, ss);
      sd = __builtin_fmaf(f, to_f(ww.e[e]) * to_f(g[i].e[e]), sd);
    }
  }
  ss = wave_sum(ss);
  sd = wave_sum(sd);
  if (WPR == 4) {
    if (lane == 0) {
      part[0][wave] = ss;
      part[1][wave] = sd;
    }
    __syncthreads();
    ss = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
    sd = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
  }
  if (!live) return;
  const float r = rsqrtf(ss * inv_c + eps);
  const float c = r * r * r * (sd * inv_c);
  const int64_t off = (int64_t)row * C8 * 8;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = v0 + VS * i;
    if (v < C8) {
      Pack8<T> ww, r2, o;
      ww.u = *reinterpret_cast<const u32x4*>(w + (int64_t)v * 8);
      r2.u = u32x4{0u, 0u, 0u, 0u};
      if (add) r2.u = *reinterpret_cast<const u32x4*>(add + off + (int64_t)v * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float t = __builtin_fmaf(-to_f(a[i].e[e]), c, r * (to_f(ww.e[e]) * to_f(g[i].e[e])));
        o.e[e] = from_f<T>(add ? t + to_f(r2.e[e]) : t);
      }
      *reinterpret_cast<u32x4*>(dx + off + (int64_t)v * 8) = o.u;
    }
  }
}

// dproj [M, 2 F] of out = gelu_tanh(gate) * up on proj = gate | up, from dout [M, F]:
//   gate half  dout * up * gelu_tanh'(gate)   (dgelu_tanh_f, launch_act_bwd kind 2's expression: with up = 1 its bits)
//   up half    dout * gelu_tanh(gate)         (the forward's GELU to the letter)
template <typename T>
__global__ void gated_gelu_tanh_bwd_kernel(const T* __restrict__ p, const T* __restrict__ dout, T* __restrict__ dp, int64_t M,
                                           int F8) {
  const int64_t total = M * F8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t m = i / F8;
    const int v = (int)(i - m * F8);
    Pack8<T> g, u, d, og, ou;
    g.u = *reinterpret_cast<const u32x4*>(p + (m * 2 * F8 + v) * 8);
    u.u = *reinterpret_cast<const u32x4*>(p + (m * 2 * F8 + F8 + v) * 8);
    d.u = *reinterpret_cast<const u32x4*>(dout + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float f = to_f(g.e[e]), dv = to_f(d.e[e]);
      const float u2 = 1.5957691216057308f * f * __builtin_fmaf(0.044715f * f, f, 1.f);
      og.e[e] = from_f<T>((dv * to_f(u.e[e])) * dgelu_tanh_f(f));
      ou.e[e] = from_f<T>(dv * (f / (1.f + __expf(-u2))));
    }
    *reinterpret_cast<u32x4*>(dp + (m * 2 * F8 + v) * 8) = og.u;
    *reinterpret_cast<u32x4*>(dp + (m * 2 * F8 + F8 + v) * 8) = ou.u;
  }
}

template <typename T>
int rmsnorm_bwd_t(const void* x, const void* dy, const void* w, const void* add, void* dx, int M, int C, float eps,
                  hipStream_t st) {
  const int C8 = C / 8;
  const float inv_c = 1.f / (float)C;
#define SMI_RMSB(NV_, WPR_)                                                                                            \
  hipLaunchKernelGGL((rmsnorm_rows_bwd_kernel<T, NV_, WPR_>), dim3(WPR_ == 1 ? cdiv(M, 4) : M), dim3(256), 0, st,      \
                     (const T*)x, (const T*)dy, (const T*)w, (const T*)add, (T*)dx, M, C8, inv_c, eps)
  if (C <= 8 * 64 * RMS_MAXV) {
    switch (cdiv(C8, 64)) {
      case 1: SMI_RMSB(1, 1); break;
      case 2: SMI_RMSB(2, 1); break;
      case 3: SMI_RMSB(3, 1); break;
      default: SMI_RMSB(4, 1); break;
    }
  } else {
    switch (cdiv(C8, 256)) {
      case 2: SMI_RMSB(2, 4); break;
      case 3: SMI_RMSB(3, 4); break;
      default: SMI_RMSB(4, 4); break;
    }
  }
#undef SMI_RMSB
  SMI_HIP(hipGetLastError());
  return 0;
}

template <typename T>
int rmsnorm_t(const void* x, const void* w, void* y, int M, int C, float eps, hipStream_t st) {
  const int C8 = C / 8;
  const float inv_c = 1.f / (float)C;
#define SMI_RMS(NV_, WPR_)                                                                                             \
  hipLaunchKernelGGL((rmsnorm_rows_kernel<T, NV_, WPR_>), dim3(WPR_ == 1 ? cdiv(M, 4) : M), dim3(256), 0, st, (const T*)x, \
                     (const T*)w, (T*)y, M, C8, inv_c, eps)
  if (C <= 8 * 64 * RMS_MAXV) {
    switch (cdiv(C8, 64)) {
      case 1: SMI_RMS(1, 1); break;
      case 2: SMI_RMS(2, 1); break;
      case 3: SMI_RMS(3, 1); break;
      default: SMI_RMS(4, 1); break;
    }
  } else {
    switch (cdiv(C8, 256)) {
      case 2: SMI_RMS(2, 4); break;
      case 3: SMI_RMS(3, 4); break;
      default: SMI_RMS(4, 4); break;
    }
  }
#undef SMI_RMS
  SMI_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int launch_rmsnorm_rows(int dtype, const void* x, const void* w, void* y, int M, int C, float eps, hipStream_t stream) {
  SMI_CHECK(M > 0 && C > 0 && C % 8 == 0 && C <= 8 * 256 * RMS_MAXV, "rmsnorm: C=%d must be a multiple of 8 and at most %d",
            C, 8 * 256 * RMS_MAXV);
  return dtype == DT_F16 ? rmsnorm_t<f16>(x, w, y, M, C, eps, stream) : rmsnorm_t<bf16>(x, w, y, M, C, eps, stream);
}

int launch_rmsnorm_rows_bwd(int dtype, const void* x, const void* dy, const void* w, const void* add, void* dx, int M, int C,
                            float eps, hipStream_t stream) {
  SMI_CHECK(M > 0 && C > 0 && C % 8 == 0 && C <= 8 * 256 * RMS_MAXV,
            "rmsnorm_bwd: C=%d must be a multiple of 8 and at most %d", C, 8 * 256 * RMS_MAXV);
  return dtype == DT_F16 ? rmsnorm_bwd_t<f16>(x, dy, w, add, dx, M, C, eps, stream)
                         : rmsnorm_bwd_t<bf16>(x, dy, w, add, dx, M, C, eps, stream);
}

int launch_gated_gelu_tanh_bwd(int dtype, const void* proj, const void* dout, void* dproj, int64_t M, int F,
                               hipStream_t stream) {
  SMI_CHECK(M > 0 && F > 0 && F % 8 == 0, "gated_gelu_tanh_bwd: F=%d must be a positive multiple of 8", F);
  const int grid = (int)std::min<int64_t>((M * (F / 8) + 255) / 256, 16384);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(gated_gelu_tanh_bwd_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)proj, (const f16*)dout,
                       (f16*)dproj, M, F / 8);
  else
    hipLaunchKernelGGL(gated_gelu_tanh_bwd_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)proj,
                       (const bf16*)dout, (bf16*)dproj, M, F / 8);
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_t5_bias_table(int dtype, const void* weight, const int* bucket, float* out, int H, int L, int num_buckets,
                         hipStream_t stream) {
  SMI_CHECK(H > 0 && L > 0 && num_buckets > 0, "t5_bias_table: empty shape");
  const int n_off = 2 * L - 1;
  const dim3 grid(cdiv((int64_t)H * n_off, 256));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(t5_bias_table_kernel<f16>, grid, dim3(256), 0, stream, (const f16*)weight, bucket, out, H, n_off, num_buckets);
  else
    hipLaunchKernelGGL(t5_bias_table_kernel<bf16>, grid, dim3(256), 0, stream, (const bf16*)weight, bucket, out, H, n_off, num_buckets);
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_gated_gelu_tanh(int dtype, const void* proj, void* out, int64_t M, int F, hipStream_t stream) {
  SMI_CHECK(M > 0 && F > 0 && F % 8 == 0, "gated_gelu_tanh: F=%d must be a positive multiple of 8", F);
  const int grid = (int)std::min<int64_t>((M * (F / 8) + 255) / 256, 16384);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(gated_gelu_tanh_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)proj, (f16*)out, M, F / 8);
  else
    hipLaunchKernelGGL(gated_gelu_tanh_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)proj, (bf16*)out, M, F / 8);
  SMI_HIP(hipGetLastError());
  return 0;
}

// transformers T5Attention._relative_position_bucket(bidirectional=True) for every offset o - (L - 1) = key - query
int t5_relative_buckets(int num_buckets, int max_distance, int L, int32_t* out) {
  SMI_CHECK(out && L >= 1 && num_buckets >= 4 && num_buckets % 2 == 0 && max_distance > num_buckets / 4,
            "smi_t5_relative_buckets: need L >= 1, an even num_buckets >= 4 and max_distance > num_buckets / 4 (got %d, %d, %d)",
            L, num_buckets, max_distance);
  const int nb = num_buckets / 2, max_exact = nb / 2;
  for (int o = 0; o < 2 * L - 1; ++o) {
    const int rel = o - (L - 1);
    int b = rel > 0 ? nb : 0;
    const int a = rel < 0 ? -rel : rel;
    if (a < max_exact) {
      b += a;
    } else {  // the float32 evaluation of torch: log(a / max_exact) / log(max_distance / max_exact) * (nb - max_exact), truncated
      const float t = logf((float)a / (float)max_exact) / logf((float)max_distance / (float)max_exact) * (float)(nb - max_exact);
      const int large = max_exact + (int)t;
      b += large < nb - 1 ? large : nb - 1;
    }
    out[o] = b;
  }
  return 0;
}

}  // namespace smi
