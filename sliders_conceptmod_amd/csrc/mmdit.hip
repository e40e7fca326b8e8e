// The pieces that make an MMDiT (SD3) an MMDiT, around the GEMMs and the attention: adaLN-Zero modulation and the gated
// residual, the joint (image + text) sequence pack / split, the patch matrix, the cropped position table, the un-patchify.
// All memory-bound: 16 bytes per lane wherever the element is 16-bit, fp32 arithmetic, one rounding at the store.
#include "kernels.h"

namespace smi {
namespace {

#define GSTRIDE(i, n) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

inline int ew_grid(int64_t n_threads) {
  int64_t g = (n_threads + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// the same sum in every lane, fixed order
__device__ __forceinline__ float wave_sum_all(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

constexpr int ADALN_MAXV = 6;  // C <= 3072 (Flux's width), forward and backward; C <= 2048 runs the instantiations it always did

// y[r, :] = LN(x[r, :]) (1 + scale[s, :]) + shift[s, :], s = r / rows_per_sample; one wave per row, the row kept in
// registers between the statistics (two passes: mean, then centred squares) and the apply.  scale / shift: rows of
// mod [n, ldm] at column offsets off_scale / off_shift
template <typename T, int NV>
__global__ __launch_bounds__(256) void adaln_modulate_kernel(const T* __restrict__ x, const T* __restrict__ mod, T* __restrict__ y,
                                                             float* __restrict__ mean_rstd, int M, int C, int rows_per_sample,
                                                             int64_t ldm, int off_scale, int off_shift, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nvec = C / 8;
  const float inv_c = 1.f / (float)C;
  float xv[NV][8];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = lane + 64 * j;
    Pack8<T> t;
    if (v < nvec) t.u = *reinterpret_cast<const u32x4*>(x + (int64_t)row * C + v * 8);
    else t.u = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) xv[j][e] = to_f(t.e[e]);
  }
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) s += xv[j][e];
  const float mean = wave_sum_all(s) * inv_c;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    if (lane + 64 * j < nvec) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = xv[j][e] - mean;
        sq += d * d;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum_all(sq) * inv_c + eps);
  const T* mrow = mod + (int64_t)(row / rows_per_sample) * ldm;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = lane + 64 * j;
    if (v < nvec) {
      Pack8<T> sc, sh, o;
      sc.u = *reinterpret_cast<const u32x4*>(mrow + off_scale + v * 8);
      sh.u = *reinterpret_cast<const u32x4*>(mrow + off_shift + v * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        o.e[e] = from_f<T>((xv[j][e] - mean) * rstd * (1.f + to_f(sc.e[e])) + to_f(sh.e[e]));
      *reinterpret_cast<u32x4*>(y + (int64_t)row * C + v * 8) = o.u;
    }
  }
  if (mean_rstd && lane == 0) {
    mean_rstd[(int64_t)row * 2] = mean;
    mean_rstd[(int64_t)row * 2 + 1] = rstd;
  }
}

// the backward to x: with g = dy (1 + scale[s, :]) and xhat = (x - mean) rstd from the forward's mean_rstd,
// dx[r, :] = rstd (g - mean_c(g) - xhat mean_c(g xhat)) (+ add[r, :]).  One wave per row; g and xhat stay in registers between
// the two reductions and the apply.  add may alias dx (a lane reads its vector before it writes it); no restrict on the two
template <typename T, int NV>
__global__ __launch_bounds__(256) void adaln_modulate_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                                 const T* __restrict__ mod, const float* __restrict__ mean_rstd,
                                                                 const T* add, T* dx, int M, int C, int rows_per_sample,
                                                                 int64_t ldm, int off_scale) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nvec = C / 8;
  const float inv_c = 1.f / (float)C;
  const float mean = mean_rstd[(int64_t)row * 2], rstd = mean_rstd[(int64_t)row * 2 + 1];
  const T* mrow = mod + (int64_t)(row / rows_per_sample) * ldm + off_scale;
  float g[NV][8], xh[NV][8];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = lane + 64 * j;
    if (v < nvec) {
      Pack8<T> xv, dv, sc;
      xv.u = *reinterpret_cast<const u32x4*>(x + (int64_t)row * C + v * 8);
      dv.u = *reinterpret_cast<const u32x4*>(dy + (int64_t)row * C + v * 8);
      sc.u = *reinterpret_cast<const u32x4*>(mrow + v * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        g[j][e] = to_f(dv.e[e]) * (1.f + to_f(sc.e[e]));
        xh[j][e] = (to_f(xv.e[e]) - mean) * rstd;
        s1 += g[j][e];
        s2 = __builtin_fmaf(g[j][e], xh[j][e], s2);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) g[j][e] = xh[j][e] = 0.f;
    }
  }
  const float m1 = wave_sum_all(s1) * inv_c;
  const float m2 = wave_sum_all(s2) * inv_c;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = lane + 64 * j;
    if (v < nvec) {
      Pack8<T> av, o;
      if (add) av.u = *reinterpret_cast<const u32x4*>(add + (int64_t)row * C + v * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = rstd * (g[j][e] - m1 - xh[j][e] * m2);
        o.e[e] = from_f<T>(add ? d + to_f(av.e[e]) : d);
      }
      *reinterpret_cast<u32x4*>(dx + (int64_t)row * C + v * 8) = o.u;
    }
  }
}

// y[r, :] = h[r, :] + gate[s, :] f[r, :]; y may alias h (every vector is read before it is written, by the same lane)
template <typename T>
__global__ void gate_residual_kernel(const T* h, const T* __restrict__ f, const T* __restrict__ mod, T* y, int64_t M, int C8,
                                     int rows_per_sample, int64_t ldm, int off_gate) {
  GSTRIDE(i, M * C8) {
    const int64_t r = i / C8;
    const int v = (int)(i - r * C8);
    Pack8<T> hv, fv, gv, o;
    hv.u = *reinterpret_cast<const u32x4*>(h + i * 8);
    fv.u = *reinterpret_cast<const u32x4*>(f + i * 8);
    gv.u = *reinterpret_cast<const u32x4*>(mod + (r / rows_per_sample) * ldm + off_gate + v * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) o.e[e] = from_f<T>(__builtin_fmaf(to_f(gv.e[e]), to_f(fv.e[e]), to_f(hv.e[e])));
    *reinterpret_cast<u32x4*>(y + i * 8) = o.u;
  }
}

// its backward to f: df[r, :] = gate[s, :] dy[r, :] (the gradient of h is dy itself: no kernel)
template <typename T>
__global__ void gate_residual_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ mod, T* __restrict__ df, int64_t M,
                                         int C8, int rows_per_sample, int64_t ldm, int off_gate) {
  GSTRIDE(i, M * C8) {
    const int64_t r = i / C8;
    const int v = (int)(i - r * C8);
    Pack8<T> dv, gv, o;
    dv.u = *reinterpret_cast<const u32x4*>(dy + i * 8);
    gv.u = *reinterpret_cast<const u32x4*>(mod + (r / rows_per_sample) * ldm + off_gate + v * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) o.e[e] = from_f<T>(to_f(gv.e[e]) * to_f(dv.e[e]));
    *reinterpret_cast<u32x4*>(df + i * 8) = o.u;
  }
}

// joint [n (Nx + Nc), W] <-> a [n Nx, W], b [n Nc, W]: per sample the Nx rows of a, then the Nc rows of b.
// PACK: joint is written; else a and b are (either may be NULL: that stream is dropped).  16-bit elements as 16-byte words
template <bool PACK>
__global__ void joint_rows_kernel(u32x4* __restrict__ a, u32x4* __restrict__ b, u32x4* __restrict__ joint, int64_t n, int Nx,
                                  int Nc, int W8) {
  const int L = Nx + Nc;
  GSTRIDE(i, n * L * W8) {
    const int64_t r = i / W8;
    const int v = (int)(i - r * W8);
    const int64_t s = r / L;
    const int t = (int)(r - s * L);
    u32x4* side = t < Nx ? a + ((s * Nx + t) * W8 + v) : b + ((s * Nc + (t - Nx)) * W8 + v);
    if (PACK) joint[i] = *side;
    else if (t < Nx ? a != nullptr : b != nullptr) *side = joint[i];
  }
}

// T[(n, gy, gx), (c, py, px)] = latents[n, c, gy p + py, gx p + px]; one lane writes 8 adjacent columns
template <typename T>
__global__ void sd3_patchify_kernel(const float* __restrict__ lat, T* __restrict__ out, int64_t rows, int Cin, int H, int W, int p) {
  const int K8 = Cin * p * p / 8;
  const int gw = W / p, gh = H / p;
  GSTRIDE(i, rows * K8) {
    const int64_t r = i / K8;
    const int k0 = (int)(i - r * K8) * 8;
    const int gx = (int)(r % gw);
    const int gy = (int)((r / gw) % gh);
    const int64_t n = r / ((int64_t)gw * gh);
    Pack8<T> o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = k0 + e;
      const int px = k % p, py = (k / p) % p, c = k / (p * p);
      o.e[e] = from_f<T>(lat[((n * Cin + c) * H + gy * p + py) * W + gx * p + px]);
    }
    *reinterpret_cast<u32x4*>(out + i * 8) = o.u;
  }
}

// y[(n, gy, gx), :] = x[(n, gy, gx), :] + pos[(top + gy) S + left + gx, :]; y may alias x
template <typename T>
__global__ void sd3_add_pos_kernel(const T* x, const T* __restrict__ pos, T* y, int64_t rows, int d8, int gh, int gw, int S,
                                   int top, int left) {
  GSTRIDE(i, rows * d8) {
    const int64_t r = i / d8;
    const int v = (int)(i - r * d8);
    const int gx = (int)(r % gw);
    const int gy = (int)((r / gw) % gh);
    Pack8<T> xv, pv, o;
    xv.u = *reinterpret_cast<const u32x4*>(x + i * 8);
    pv.u = *reinterpret_cast<const u32x4*>(pos + ((int64_t)(top + gy) * S + left + gx) * d8 * 8 + v * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) o.e[e] = from_f<T>(to_f(xv.e[e]) + to_f(pv.e[e]));
    *reinterpret_cast<u32x4*>(y + i * 8) = o.u;
  }
}

// out[n, c, gy p + py, gx p + px] = rows[(n, gy, gx), (py, px, c)]; one lane per output element (adjacent lanes: adjacent x)
template <typename T>
__global__ void sd3_unpatchify_kernel(const T* __restrict__ rows, float* __restrict__ out, int64_t total, int Cout, int gh, int gw,
                                      int p) {
  const int H = gh * p, W = gw * p;
  GSTRIDE(i, total) {
    const int X = (int)(i % W);
    const int Y = (int)((i / W) % H);
    const int c = (int)((i / ((int64_t)W * H)) % Cout);
    const int64_t n = i / ((int64_t)W * H * Cout);
    const int64_t r = (n * gh + Y / p) * gw + X / p;
    out[i] = to_f(rows[r * ((int64_t)p * p * Cout) + ((Y % p) * p + X % p) * Cout + c]);
  }
}

// the inverse, for the backward: rows[(n, gy, gx), (py, px, c)] = scale[n] d_out[n, c, gy p + py, gx p + px] (scale: the
// sample's loss scale on the device); one lane writes 8 adjacent columns
template <typename T>
__global__ void sd3_unpatchify_bwd_kernel(const float* __restrict__ d_out, T* __restrict__ rows, int64_t nrows, int Cout, int gh,
                                          int gw, int p, const float* __restrict__ scale) {
  const int K8 = p * p * Cout / 8;
  const int H = gh * p, W = gw * p;
  GSTRIDE(i, nrows * K8) {
    const int64_t r = i / K8;
    const int k0 = (int)(i - r * K8) * 8;
    const int gx = (int)(r % gw);
    const int gy = (int)((r / gw) % gh);
    const int64_t n = r / ((int64_t)gw * gh);
    const float s = scale[n];
    Pack8<T> o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = k0 + e;
      const int c = k % Cout, px = (k / Cout) % p, py = k / (Cout * p);
      o.e[e] = from_f<T>(s * d_out[((n * Cout + c) * H + gy * p + py) * W + gx * p + px]);
    }
    *reinterpret_cast<u32x4*>(rows + i * 8) = o.u;
  }
}

}  // namespace

int launch_adaln_modulate_bwd(int dtype, const void* x, const void* dy, const void* mod, const float* mean_rstd, const void* add,
                              void* dx, int M, int C, int rows_per_sample, int64_t ldm, int off_scale, hipStream_t stream) {
  SMI_CHECK(M >= 1 && C >= 8 && C % 8 == 0 && C <= 512 * ADALN_MAXV, "adaln_modulate_bwd: C %% 8, C <= 3072 (got M=%d C=%d)", M, C);
  SMI_CHECK(rows_per_sample >= 1 && ldm % 8 == 0 && off_scale % 8 == 0 && off_scale >= 0 && off_scale + C <= ldm,
            "adaln_modulate_bwd: scale is C columns of a mod row at an offset that is a multiple of 8 (ldm=%lld, %d)",
            (long long)ldm, off_scale);
  SMI_CHECK(x && dy && mod && mean_rstd && dx, "adaln_modulate_bwd: NULL operand");
  SMI_CHECK((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)mod | (uintptr_t)add | (uintptr_t)dx) & 15) == 0,
            "adaln_modulate_bwd: x, dy, mod, add and dx must be 16-byte aligned");
  const int nv = (C / 8 + 63) / 64;
#define GO(T_, NV_)                                                                                                      \
  hipLaunchKernelGGL((adaln_modulate_bwd_kernel<T_, NV_>), dim3(cdiv(M, 4)), dim3(256), 0, stream, (const T_*)x, (const T_*)dy, \
                     (const T_*)mod, mean_rstd, (const T_*)add, (T_*)dx, M, C, rows_per_sample, ldm, off_scale)
#define GO_T(T_)                  \
  switch (nv) {                   \
    case 1: GO(T_, 1); break;     \
    case 2: GO(T_, 2); break;     \
    case 3: GO(T_, 3); break;     \
    case 4: GO(T_, 4); break;     \
    case 5: GO(T_, 5); break;     \
    default: GO(T_, 6); break;    \
  }
  if (dtype == DT_F16) { GO_T(f16) } else { GO_T(bf16) }
#undef GO_T
#undef GO
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_gate_residual_bwd(int dtype, const void* dy, const void* mod, void* df, int64_t M, int C, int rows_per_sample,
                             int64_t ldm, int off_gate, hipStream_t stream) {
  SMI_CHECK(M >= 1 && C >= 8 && C % 8 == 0, "gate_residual_bwd: C %% 8 (got C=%d)", C);
  SMI_CHECK(rows_per_sample >= 1 && ldm % 8 == 0 && off_gate % 8 == 0 && off_gate >= 0 && off_gate + C <= ldm,
            "gate_residual_bwd: gate is C columns of a mod row at an offset that is a multiple of 8 (ldm=%lld, %d)",
            (long long)ldm, off_gate);
  SMI_CHECK(dy && mod && df && (((uintptr_t)dy | (uintptr_t)mod | (uintptr_t)df) & 15) == 0,
            "gate_residual_bwd: dy, mod and df must be non-NULL and 16-byte aligned");
  const int grid = ew_grid(M * (C / 8));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(gate_residual_bwd_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)dy, (const f16*)mod, (f16*)df, M, C / 8, rows_per_sample, ldm, off_gate);
  else
    hipLaunchKernelGGL(gate_residual_bwd_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)dy, (const bf16*)mod, (bf16*)df, M, C / 8, rows_per_sample, ldm, off_gate);
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_sd3_unpatchify_bwd(int dtype, const float* d_out, void* rows, int n, int Cout, int gh, int gw, int p,
                              const float* scale_dev, hipStream_t stream) {
  SMI_CHECK(n >= 1 && Cout >= 1 && gh >= 1 && gw >= 1 && p >= 1 && (Cout * p * p) % 8 == 0 && scale_dev,
            "sd3_unpatchify_bwd: Cout p p %% 8 and a scale per sample (got Cout=%d p=%d)", Cout, p);
  const int64_t nrows = (int64_t)n * gh * gw;
  const int grid = ew_grid(nrows * (Cout * p * p / 8));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(sd3_unpatchify_bwd_kernel<f16>, dim3(grid), dim3(256), 0, stream, d_out, (f16*)rows, nrows, Cout, gh, gw, p, scale_dev);
  else
    hipLaunchKernelGGL(sd3_unpatchify_bwd_kernel<bf16>, dim3(grid), dim3(256), 0, stream, d_out, (bf16*)rows, nrows, Cout, gh, gw, p, scale_dev);
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_adaln_modulate(int dtype, const void* x, const void* mod, void* y, float* mean_rstd, int M, int C,
                          int rows_per_sample, int64_t ldm, int off_scale, int off_shift, float eps, hipStream_t stream) {
  SMI_CHECK(M >= 1 && C >= 8 && C % 8 == 0 && C <= 512 * ADALN_MAXV, "adaln_modulate: C %% 8, C <= 3072 (got M=%d C=%d)", M, C);
  SMI_CHECK(rows_per_sample >= 1 && ldm % 8 == 0 && off_scale % 8 == 0 && off_shift % 8 == 0 && off_scale >= 0 &&
                off_shift >= 0 && off_scale + C <= ldm && off_shift + C <= ldm,
            "adaln_modulate: scale / shift are C columns of a mod row at offsets that are multiples of 8 (ldm=%lld, %d, %d)",
            (long long)ldm, off_scale, off_shift);
  SMI_CHECK((((uintptr_t)x | (uintptr_t)mod | (uintptr_t)y) & 15) == 0, "adaln_modulate: x, mod and y must be 16-byte aligned");
  const int nv = (C / 8 + 63) / 64;
#define GO(T_, NV_)                                                                                                        \
  hipLaunchKernelGGL((adaln_modulate_kernel<T_, NV_>), dim3(cdiv(M, 4)), dim3(256), 0, stream, (const T_*)x, (const T_*)mod, \
                     (T_*)y, mean_rstd, M, C, rows_per_sample, ldm, off_scale, off_shift, eps)
#define GO_T(T_)                  \
  switch (nv) {                   \
    case 1: GO(T_, 1); break;     \
    case 2: GO(T_, 2); break;     \
    case 3: GO(T_, 3); break;     \
    case 4: GO(T_, 4); break;     \
    case 5: GO(T_, 5); break;     \
    default: GO(T_, 6); break;    \
  }
  if (dtype == DT_F16) { GO_T(f16) } else { GO_T(bf16) }
#undef GO_T
#undef GO
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_gate_residual(int dtype, const void* h, const void* f, const void* mod, void* y, int64_t M, int C,
                         int rows_per_sample, int64_t ldm, int off_gate, hipStream_t stream) {
  SMI_CHECK(M >= 1 && C >= 8 && C % 8 == 0, "gate_residual: C %% 8 (got C=%d)", C);
  SMI_CHECK(rows_per_sample >= 1 && ldm % 8 == 0 && off_gate % 8 == 0 && off_gate >= 0 && off_gate + C <= ldm,
            "gate_residual: gate is C columns of a mod row at an offset that is a multiple of 8 (ldm=%lld, %d)", (long long)ldm,
            off_gate);
  SMI_CHECK((((uintptr_t)h | (uintptr_t)f | (uintptr_t)mod | (uintptr_t)y) & 15) == 0,
            "gate_residual: h, f, mod and y must be 16-byte aligned");
  const int grid = ew_grid(M * (C / 8));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(gate_residual_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)h, (const f16*)f, (const f16*)mod, (f16*)y, M, C / 8, rows_per_sample, ldm, off_gate);
  else
    hipLaunchKernelGGL(gate_residual_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)h, (const bf16*)f, (const bf16*)mod, (bf16*)y, M, C / 8, rows_per_sample, ldm, off_gate);
  SMI_HIP(hipGetLastError());
  return 0;
}

static int joint_rows(bool pack, void* a, void* b, void* joint, int n, int Nx, int Nc, int W, hipStream_t stream) {
  SMI_CHECK(n >= 1 && Nx >= 1 && Nc >= 1 && W >= 8 && W % 8 == 0, "joint_rows: n, Nx, Nc >= 1 and W %% 8 (got %d, %d, %d, %d)", n,
            Nx, Nc, W);
  SMI_CHECK(joint && (pack ? (a && b) : (a || b)), "joint_rows: NULL operand");
  SMI_CHECK((((uintptr_t)a | (uintptr_t)b | (uintptr_t)joint) & 15) == 0, "joint_rows: operands must be 16-byte aligned");
  const int grid = ew_grid((int64_t)n * (Nx + Nc) * (W / 8));
  if (pack)
    hipLaunchKernelGGL(joint_rows_kernel<true>, dim3(grid), dim3(256), 0, stream, (u32x4*)a, (u32x4*)b, (u32x4*)joint, (int64_t)n, Nx, Nc, W / 8);
  else
    hipLaunchKernelGGL(joint_rows_kernel<false>, dim3(grid), dim3(256), 0, stream, (u32x4*)a, (u32x4*)b, (u32x4*)joint, (int64_t)n, Nx, Nc, W / 8);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_joint_rows_pack(int dtype, const void* a, const void* b, void* joint, int n, int Nx, int Nc, int W,
                           hipStream_t stream) {
  (void)dtype;  // both types are 2 bytes wide
  return joint_rows(true, const_cast<void*>(a), const_cast<void*>(b), joint, n, Nx, Nc, W, stream);
}
int launch_joint_rows_split(int dtype, const void* joint, void* a, void* b, int n, int Nx, int Nc, int W, hipStream_t stream) {
  (void)dtype;
  return joint_rows(false, a, b, const_cast<void*>(joint), n, Nx, Nc, W, stream);
}

int launch_sd3_patchify(int dtype, const float* latents, void* out, int n, int Cin, int H, int W, int p, hipStream_t stream) {
  SMI_CHECK(n >= 1 && Cin >= 1 && p >= 1 && H >= p && W >= p && H % p == 0 && W % p == 0 && (Cin * p * p) % 64 == 0,
            "sd3_patchify: H, W multiples of p and Cin p p a multiple of 64 (got Cin=%d H=%d W=%d p=%d)", Cin, H, W, p);
  const int64_t rows = (int64_t)n * (H / p) * (W / p);
  const int grid = ew_grid(rows * (Cin * p * p / 8));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(sd3_patchify_kernel<f16>, dim3(grid), dim3(256), 0, stream, latents, (f16*)out, rows, Cin, H, W, p);
  else
    hipLaunchKernelGGL(sd3_patchify_kernel<bf16>, dim3(grid), dim3(256), 0, stream, latents, (bf16*)out, rows, Cin, H, W, p);
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_sd3_add_pos(int dtype, const void* x, const void* pos, void* y, int n, int gh, int gw, int d, int S,
                       hipStream_t stream) {
  SMI_CHECK(n >= 1 && gh >= 1 && gw >= 1 && gh <= S && gw <= S && d >= 8 && d % 8 == 0,
            "sd3_add_pos: a %d x %d grid does not fit the %d x %d position table (or d %% 8: %d)", gh, gw, S, S, d);
  SMI_CHECK((((uintptr_t)x | (uintptr_t)pos | (uintptr_t)y) & 15) == 0, "sd3_add_pos: operands must be 16-byte aligned");
  const int64_t rows = (int64_t)n * gh * gw;
  const int grid = ew_grid(rows * (d / 8));
  const int top = (S - gh) / 2, left = (S - gw) / 2;
  if (dtype == DT_F16)
    hipLaunchKernelGGL(sd3_add_pos_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)x, (const f16*)pos, (f16*)y, rows, d / 8, gh, gw, S, top, left);
  else
    hipLaunchKernelGGL(sd3_add_pos_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)x, (const bf16*)pos, (bf16*)y, rows, d / 8, gh, gw, S, top, left);
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_sd3_unpatchify(int dtype, const void* rows, float* out, int n, int Cout, int gh, int gw, int p, hipStream_t stream) {
  SMI_CHECK(n >= 1 && Cout >= 1 && gh >= 1 && gw >= 1 && p >= 1, "sd3_unpatchify: bad shape");
  const int64_t total = (int64_t)n * Cout * gh * p * gw * p;
  const int grid = ew_grid(total);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(sd3_unpatchify_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)rows, out, total, Cout, gh, gw, p);
  else
    hipLaunchKernelGGL(sd3_unpatchify_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)rows, out, total, Cout, gh, gw, p);
  SMI_HIP(hipGetLastError());
  return 0;
}

}  // namespace smi
