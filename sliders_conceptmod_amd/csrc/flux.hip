// What a Flux transformer (diffusers FluxTransformer2DModel) adds to the MMDiT pieces of mmdit.hip: RMSNorm on q and k per
// head with the rotary position embedding, fused with the pack of a stream's q|k|v rows into the joint sequence; tanh-GELU on
// a column block of a wider matrix (the single block's [attention | mlp] operand, built without a concat copy); the
// un-pack of proj_out's rows in Flux's column order; and the backward of each to the activations, for the trainable engine
// (the RMSNorm weights are frozen: no gradient).  All memory-bound: 16 bytes per lane, fp32 arithmetic, one rounding at
// the store, vector stores only, every sum ordered by the shape.
#include "kernels.h"

namespace smi {
namespace {

#define GSTRIDE(i, n) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

inline int ew_grid(int64_t n_threads) {
  int64_t g = (n_threads + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// dst[s L + row_off + t, :] = f(src[s tokens + t, :]) for a stream's q|k|v rows [n tokens, 3 H D] (row stride lds) into the
// joint q|k|v buffer [n L, 3 H D] (row stride ldd): the q and k heads are RMS-normalised, x rsqrt(mean_D(x^2) + eps) w[0..D),
// and rotated by row (row_off + t) of the table, v is copied.  NP = 3; NP = 2 is the in-place form (src == dst, lds == ldd,
// tokens == L, row_off == 0), which has nothing to do for v.
//
// Lane-to-element map.  A group of G adjacent lanes (G = the power of two >= D / 8: 8 for D = 64, 16 for 128, 32 for 160)
// owns one (row, part, head): lane g of the group holds the head's elements [8 g, 8 g + 8), one 16-byte word, and idles where
// 8 g >= D.  A word holds the interleaved rotary pairs 4 g .. 4 g + 3 whole (D % 16 == 0, so neither a pair nor a head's
// half straddles a word), whose cos and sin are one float4 each at table[row][4 g] and table[row][D / 2 + 4 g].  The mean of
// squares is the lane's eight squares added in element order, then a G-lane butterfly (xor G/2 .. 1): the same order for
// every row, so a sample has the same bits alone or in a batch.  Rotation of pair j: out[2 j] = y[2 j] cos_j - y[2 j + 1] sin_j,
// out[2 j + 1] = y[2 j + 1] cos_j + y[2 j] sin_j.  Groups are numbered (row, part, head), head fastest: a wave covers 64 / G
// adjacent heads, contiguous in memory.
template <typename T, int G, int NP>
__global__ __launch_bounds__(256) void qk_norm_rope_kernel(const T* src, T* dst, const T* __restrict__ wq, const T* __restrict__ wk,
                                                           const float* __restrict__ table, int64_t n_groups, int tokens, int L,
                                                           int row_off, int H, int D, int64_t lds, int64_t ldd, float eps) {
  const int g = threadIdx.x & (G - 1);
  const bool live = 8 * g < D;
  const float inv_d = 1.f / (float)D;
  // (whole groups stride together: blockDim.x and the grid stride are multiples of G)
  for (int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G; grp < n_groups; grp += (int64_t)gridDim.x * (blockDim.x / G)) {
    const int h = (int)(grp % H);
    const int part = (int)((grp / H) % NP);
    const int64_t r = grp / ((int64_t)H * NP);
    const int64_t s = r / tokens;
    const int t = (int)(r - s * tokens);
    const int64_t col = (int64_t)part * H * D + (int64_t)h * D + 8 * g;
    const T* sp = src + r * lds + col;
    T* dp = dst + (s * L + row_off + t) * ldd + col;
    Pack8<T> x, o;
    if (live) x.u = *reinterpret_cast<const u32x4*>(sp);
    else x.u = u32x4{0u, 0u, 0u, 0u};
    if (part == 2) {  // v (NP == 3 only)
      if (live) *reinterpret_cast<u32x4*>(dp) = x.u;
      continue;
    }
    float xv[8], ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      xv[e] = to_f(x.e[e]);
      ss = __builtin_fmaf(xv[e], xv[e], ss);
    }
#pragma unroll
    for (int ofs = G >> 1; ofs > 0; ofs >>= 1) ss += __shfl_xor(ss, ofs);
    if (!live) continue;
    const float rr = rsqrtf(ss * inv_d + eps);
    Pack8<T> w;
    w.u = *reinterpret_cast<const u32x4*>((part == 0 ? wq : wk) + 8 * g);
    const float* trow = table + (int64_t)(row_off + t) * D;
    const f32x4 c = *reinterpret_cast<const f32x4*>(trow + 4 * g);
    const f32x4 sn = *reinterpret_cast<const f32x4*>(trow + D / 2 + 4 * g);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float y0 = xv[2 * j] * rr * to_f(w.e[2 * j]);
      const float y1 = xv[2 * j + 1] * rr * to_f(w.e[2 * j + 1]);
      o.e[2 * j] = from_f<T>(__builtin_fmaf(y0, c[j], -(y1 * sn[j])));
      o.e[2 * j + 1] = from_f<T>(__builtin_fmaf(y1, c[j], y0 * sn[j]));
    }
    *reinterpret_cast<u32x4*>(dp) = o.u;
  }
}

// y[m, 0..C) = gelu_tanh(x[m, 0..C)) on column blocks of wider matrices (row strides ldx, ldy); y may alias x (a lane reads
// its word before it writes it).  The arithmetic of launch_act kind 2 (elementwise.hip gelu_tanh_f): the same bits
template <typename T>
__global__ void gelu_tanh_cols_kernel(const T* x, T* y, int64_t M, int C8, int64_t ldx, int64_t ldy) {
  GSTRIDE(i, M * C8) {
    const int64_t m = i / C8;
    const int v = (int)(i - m * C8);
    Pack8<T> a, o;
    a.u = *reinterpret_cast<const u32x4*>(x + m * ldx + v * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float f = to_f(a.e[e]);
      const float u2 = 1.5957691216057308f * f * __builtin_fmaf(0.044715f * f, f, 1.f);
      o.e[e] = from_f<T>(f / (1.f + __expf(-u2)));
    }
    *reinterpret_cast<u32x4*>(y + m * ldy + v * 8) = o.u;
  }
}

// out[n, c, gy p + py, gx p + px] = rows[(n, gy, gx), (c, py, px)]: Flux's _unpack_latents (sd3_unpatchify's columns are
// (py, px, c)).  One lane reads one 16-byte word of a row -- 8 adjacent columns, which for p = 2 are two channels' 2 x 2
// patches -- and writes its 8 / p runs of p adjacent pixels as fp32 vector stores (p = 2: float2; else element by element)
template <typename T>
__global__ void flux_unpack_kernel(const T* __restrict__ rows, float* __restrict__ out, int64_t nrows, int Cout, int gh, int gw,
                                   int p) {
  const int K8 = Cout * p * p / 8;
  const int H = gh * p, W = gw * p;
  GSTRIDE(i, nrows * K8) {
    const int64_t r = i / K8;
    const int k0 = (int)(i - r * K8) * 8;
    const int gx = (int)(r % gw);
    const int gy = (int)((r / gw) % gh);
    const int64_t n = r / ((int64_t)gw * gh);
    Pack8<T> a;
    a.u = *reinterpret_cast<const u32x4*>(rows + i * 8);
    if (p == 2) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = k0 + 2 * q;
        const int py = (k >> 1) & 1, c = k >> 2;
        float2 v = make_float2(to_f(a.e[2 * q]), to_f(a.e[2 * q + 1]));
        *reinterpret_cast<float2*>(out + ((n * Cout + c) * H + gy * 2 + py) * W + gx * 2) = v;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = k0 + e;
        const int px = k % p, py = (k / p) % p, c = k / (p * p);
        out[((n * Cout + c) * H + gy * p + py) * W + gx * p + px] = to_f(a.e[e]);
      }
    }
  }
}

// The backward of qk_norm_rope to the source rows: dsrc[s tokens + t, :] from the joint gradient dj[s L + row_off + t, :] and
// the pre-norm source (row strides ldx, ldd, lds).  The forward's lane map: G lanes per (row, part, head), one 16-byte word
// per lane, idle where 8 g >= D.  Per q or k head, with r = rsqrt(mean_D(x^2) + eps) recomputed from x in the forward's order:
// the rotation's transpose dy[2 j] = do[2 j] c_j + do[2 j + 1] s_j, dy[2 j + 1] = do[2 j + 1] c_j - do[2 j] s_j; g = dy w;
// dx = r (g - x r^2 mean_D(g x)).  Two G-lane butterflies (sum x^2, sum g x), each after the lane's eight terms in element
// order.  v is copied.  wq and wk are frozen: no gradient
template <typename T, int G>
__global__ __launch_bounds__(256) void qk_norm_rope_bwd_kernel(const T* __restrict__ dj, const T* __restrict__ src, T* __restrict__ dsrc,
                                                               const T* __restrict__ wq, const T* __restrict__ wk,
                                                               const float* __restrict__ table, int64_t n_groups, int tokens, int L,
                                                               int row_off, int H, int D, int64_t ldd, int64_t lds, int64_t ldx,
                                                               float eps) {
  const int g = threadIdx.x & (G - 1);
  const bool live = 8 * g < D;
  const float inv_d = 1.f / (float)D;
  for (int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G; grp < n_groups; grp += (int64_t)gridDim.x * (blockDim.x / G)) {
    const int h = (int)(grp % H);
    const int part = (int)((grp / H) % 3);
    const int64_t r = grp / ((int64_t)H * 3);
    const int64_t s = r / tokens;
    const int t = (int)(r - s * tokens);
    const int64_t col = (int64_t)part * H * D + (int64_t)h * D + 8 * g;
    const T* gp = dj + (s * L + row_off + t) * ldd + col;
    T* op = dsrc + r * ldx + col;
    Pack8<T> x, d, o;
    if (live) d.u = *reinterpret_cast<const u32x4*>(gp);
    else d.u = u32x4{0u, 0u, 0u, 0u};
    if (part == 2) {  // v
      if (live) *reinterpret_cast<u32x4*>(op) = d.u;
      continue;
    }
    if (live) x.u = *reinterpret_cast<const u32x4*>(src + r * lds + col);
    else x.u = u32x4{0u, 0u, 0u, 0u};
    float xv[8], ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      xv[e] = to_f(x.e[e]);
      ss = __builtin_fmaf(xv[e], xv[e], ss);
    }
#pragma unroll
    for (int ofs = G >> 1; ofs > 0; ofs >>= 1) ss += __shfl_xor(ss, ofs);
    const float rr = rsqrtf(ss * inv_d + eps);
    Pack8<T> w;
    f32x4 c = {0.f, 0.f, 0.f, 0.f}, sn = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      w.u = *reinterpret_cast<const u32x4*>((part == 0 ? wq : wk) + 8 * g);
      const float* trow = table + (int64_t)(row_off + t) * D;
      c = *reinterpret_cast<const f32x4*>(trow + 4 * g);
      sn = *reinterpret_cast<const f32x4*>(trow + D / 2 + 4 * g);
    } else {
      w.u = u32x4{0u, 0u, 0u, 0u};
    }
    float gv[8], gx = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d0 = to_f(d.e[2 * j]), d1 = to_f(d.e[2 * j + 1]);
      gv[2 * j] = __builtin_fmaf(d0, c[j], d1 * sn[j]) * to_f(w.e[2 * j]);
      gv[2 * j + 1] = __builtin_fmaf(d1, c[j], -(d0 * sn[j])) * to_f(w.e[2 * j + 1]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) gx = __builtin_fmaf(gv[e], xv[e], gx);
#pragma unroll
    for (int ofs = G >> 1; ofs > 0; ofs >>= 1) gx += __shfl_xor(gx, ofs);
    if (!live) continue;
    const float k = rr * rr * (gx * inv_d);
#pragma unroll
    for (int e = 0; e < 8; ++e) o.e[e] = from_f<T>(rr * __builtin_fmaf(-xv[e], k, gv[e]));
    *reinterpret_cast<u32x4*>(op) = o.u;
  }
}

// dx[m, 0..C) = dy[m, 0..C) gelu_tanh'(x[m, 0..C)) on column blocks of wider matrices (row strides ldx, ldy, ldd).  The
// arithmetic of launch_act_bwd kind 2 (dgelu_tanh_f): the same bits
template <typename T>
__global__ void gelu_tanh_cols_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx, int64_t M, int C8,
                                          int64_t ldx, int64_t ldy, int64_t ldd) {
  GSTRIDE(i, M * C8) {
    const int64_t m = i / C8;
    const int v = (int)(i - m * C8);
    Pack8<T> a, g, o;
    a.u = *reinterpret_cast<const u32x4*>(x + m * ldx + v * 8);
    g.u = *reinterpret_cast<const u32x4*>(dy + m * ldy + v * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) o.e[e] = from_f<T>(to_f(g.e[e]) * dgelu_tanh_f(to_f(a.e[e])));
    *reinterpret_cast<u32x4*>(dx + m * ldd + v * 8) = o.u;
  }
}

// flux_unpack's inverse, for the backward: rows[(n, gy, gx), (c, py, px)] = scale[n] d_out[n, c, gy p + py, gx p + px] (scale:
// the sample's power-of-two loss scale on the device).  One lane writes one 16-byte word of a row: 8 adjacent columns, for
// p = 2 two channels' 2 x 2 patches read as four float2
template <typename T>
__global__ void flux_unpack_bwd_kernel(const float* __restrict__ d_out, T* __restrict__ rows, int64_t nrows, int Cout, int gh,
                                       int gw, int p, const float* __restrict__ scale) {
  const int K8 = Cout * p * p / 8;
  const int H = gh * p, W = gw * p;
  GSTRIDE(i, nrows * K8) {
    const int64_t r = i / K8;
    const int k0 = (int)(i - r * K8) * 8;
    const int gx = (int)(r % gw);
    const int gy = (int)((r / gw) % gh);
    const int64_t n = r / ((int64_t)gw * gh);
    const float s = scale[n];
    Pack8<T> o;
    if (p == 2) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = k0 + 2 * q;
        const int py = (k >> 1) & 1, c = k >> 2;
        const float2 v = *reinterpret_cast<const float2*>(d_out + ((n * Cout + c) * H + gy * 2 + py) * W + gx * 2);
        o.e[2 * q] = from_f<T>(s * v.x);
        o.e[2 * q + 1] = from_f<T>(s * v.y);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = k0 + e;
        const int px = k % p, py = (k / p) % p, c = k / (p * p);
        o.e[e] = from_f<T>(s * d_out[((n * Cout + c) * H + gy * p + py) * W + gx * p + px]);
      }
    }
    *reinterpret_cast<u32x4*>(rows + i * 8) = o.u;
  }
}

}  // namespace

int launch_qk_norm_rope(int dtype, const void* src, int64_t lds, void* dst, int64_t ldd, const void* wq, const void* wk,
                        const float* table, int n, int tokens, int L, int row_off, int H, int D, float eps, hipStream_t stream) {
  SMI_CHECK(n >= 1 && tokens >= 1 && H >= 1 && D >= 16 && D % 16 == 0 && D <= 160,
            "qk_norm_rope: head_dim %d must be a multiple of 16 in [16, 160] (n=%d tokens=%d heads=%d)", D, n, tokens, H);
  SMI_CHECK(row_off >= 0 && row_off + tokens <= L, "qk_norm_rope: rows [%d, %d) outside the joint sequence of %d", row_off,
            row_off + tokens, L);
  SMI_CHECK(lds % 8 == 0 && ldd % 8 == 0 && lds >= 3 * (int64_t)H * D && ldd >= 3 * (int64_t)H * D,
            "qk_norm_rope: row strides %lld / %lld must be multiples of 8 and hold q|k|v (3 x %d x %d)", (long long)lds,
            (long long)ldd, H, D);
  SMI_CHECK(src && dst && wq && wk && table, "qk_norm_rope: NULL operand");
  SMI_CHECK((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)wq | (uintptr_t)wk | (uintptr_t)table) & 15) == 0,
            "qk_norm_rope: operands must be 16-byte aligned");
  const bool inplace = src == dst;
  SMI_CHECK(!inplace || (lds == ldd && tokens == L && row_off == 0),
            "qk_norm_rope: in place takes the whole joint sequence (tokens == L, row offset 0, equal strides)");
  const int G = D <= 16 ? 2 : D <= 32 ? 4 : D <= 64 ? 8 : D <= 128 ? 16 : 32;
  const int64_t n_groups = (int64_t)n * tokens * (inplace ? 2 : 3) * H;
  const int grid = ew_grid(n_groups * G);
#define GO(T_, G_, NP_)                                                                                                       \
  hipLaunchKernelGGL((qk_norm_rope_kernel<T_, G_, NP_>), dim3(grid), dim3(256), 0, stream, (const T_*)src, (T_*)dst,          \
                     (const T_*)wq, (const T_*)wk, table, n_groups, tokens, L, row_off, H, D, lds, ldd, eps)
#define GO_NP(T_, G_) \
  if (inplace) GO(T_, G_, 2); else GO(T_, G_, 3)
#define GO_T(T_)                     \
  switch (G) {                       \
    case 2: GO_NP(T_, 2); break;     \
    case 4: GO_NP(T_, 4); break;     \
    case 8: GO_NP(T_, 8); break;     \
    case 16: GO_NP(T_, 16); break;   \
    default: GO_NP(T_, 32); break;   \
  }
  if (dtype == DT_F16) { GO_T(f16) } else { GO_T(bf16) }
#undef GO_T
#undef GO_NP
#undef GO
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_gelu_tanh_cols(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int64_t M, int C, hipStream_t stream) {
  SMI_CHECK(M >= 1 && C >= 8 && C % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0 && ldx >= C && ldy >= C,
            "gelu_tanh_cols: C %% 8 and row strides that are multiples of 8 and >= C (got C=%d, %lld, %lld)", C, (long long)ldx,
            (long long)ldy);
  SMI_CHECK(x && y && (((uintptr_t)x | (uintptr_t)y) & 15) == 0, "gelu_tanh_cols: x and y must be non-NULL and 16-byte aligned");
  const int grid = ew_grid(M * (C / 8));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(gelu_tanh_cols_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)x, (f16*)y, M, C / 8, ldx, ldy);
  else
    hipLaunchKernelGGL(gelu_tanh_cols_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)x, (bf16*)y, M, C / 8, ldx, ldy);
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_flux_unpack(int dtype, const void* rows, float* out, int n, int Cout, int gh, int gw, int p, hipStream_t stream) {
  SMI_CHECK(n >= 1 && Cout >= 1 && gh >= 1 && gw >= 1 && p >= 1 && (Cout * p * p) % 8 == 0,
            "flux_unpack: Cout p p %% 8 (got Cout=%d p=%d)", Cout, p);
  SMI_CHECK(rows && out && (((uintptr_t)rows & 15) == 0) && (((uintptr_t)out & 7) == 0),
            "flux_unpack: rows must be 16-byte aligned, out 8-byte aligned");
  const int64_t nrows = (int64_t)n * gh * gw;
  const int grid = ew_grid(nrows * (Cout * p * p / 8));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(flux_unpack_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)rows, out, nrows, Cout, gh, gw, p);
  else
    hipLaunchKernelGGL(flux_unpack_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)rows, out, nrows, Cout, gh, gw, p);
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_qk_norm_rope_bwd(int dtype, const void* dj, int64_t ldd, const void* src, int64_t lds, void* dsrc, int64_t ldx,
                            const void* wq, const void* wk, const float* table, int n, int tokens, int L, int row_off, int H,
                            int D, float eps, hipStream_t stream) {
  SMI_CHECK(n >= 1 && tokens >= 1 && H >= 1 && D >= 16 && D % 16 == 0 && D <= 160,
            "qk_norm_rope_bwd: head_dim %d must be a multiple of 16 in [16, 160] (n=%d tokens=%d heads=%d)", D, n, tokens, H);
  SMI_CHECK(row_off >= 0 && row_off + tokens <= L, "qk_norm_rope_bwd: rows [%d, %d) outside the joint sequence of %d", row_off,
            row_off + tokens, L);
  SMI_CHECK(lds % 8 == 0 && ldd % 8 == 0 && ldx % 8 == 0 && lds >= 3 * (int64_t)H * D && ldd >= 3 * (int64_t)H * D &&
                ldx >= 3 * (int64_t)H * D,
            "qk_norm_rope_bwd: row strides %lld / %lld / %lld must be multiples of 8 and hold q|k|v (3 x %d x %d)",
            (long long)ldd, (long long)lds, (long long)ldx, H, D);
  SMI_CHECK(dj && src && dsrc && wq && wk && table, "qk_norm_rope_bwd: NULL operand");
  SMI_CHECK((((uintptr_t)dj | (uintptr_t)src | (uintptr_t)dsrc | (uintptr_t)wq | (uintptr_t)wk | (uintptr_t)table) & 15) == 0,
            "qk_norm_rope_bwd: operands must be 16-byte aligned");
  SMI_CHECK(dsrc != dj && dsrc != src, "qk_norm_rope_bwd: the source gradient may alias neither the joint gradient nor the source");
  const int G = D <= 16 ? 2 : D <= 32 ? 4 : D <= 64 ? 8 : D <= 128 ? 16 : 32;
  const int64_t n_groups = (int64_t)n * tokens * 3 * H;
  const int grid = ew_grid(n_groups * G);
#define GO(T_, G_)                                                                                                          \
  hipLaunchKernelGGL((qk_norm_rope_bwd_kernel<T_, G_>), dim3(grid), dim3(256), 0, stream, (const T_*)dj, (const T_*)src,   \
                     (T_*)dsrc, (const T_*)wq, (const T_*)wk, table, n_groups, tokens, L, row_off, H, D, ldd, lds, ldx, eps)
#define GO_T(T_)                  \
  switch (G) {                    \
    case 2: GO(T_, 2); break;     \
    case 4: GO(T_, 4); break;     \
    case 8: GO(T_, 8); break;     \
    case 16: GO(T_, 16); break;   \
    default: GO(T_, 32); break;   \
  }
  if (dtype == DT_F16) { GO_T(f16) } else { GO_T(bf16) }
#undef GO_T
#undef GO
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_gelu_tanh_cols_bwd(int dtype, const void* x, int64_t ldx, const void* dy, int64_t ldy, void* dx, int64_t ldd, int64_t M,
                              int C, hipStream_t stream) {
  SMI_CHECK(M >= 1 && C >= 8 && C % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0 && ldd % 8 == 0 && ldx >= C && ldy >= C && ldd >= C,
            "gelu_tanh_cols_bwd: C %% 8 and row strides that are multiples of 8 and >= C (got C=%d, %lld, %lld, %lld)", C,
            (long long)ldx, (long long)ldy, (long long)ldd);
  SMI_CHECK(x && dy && dx && (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0,
            "gelu_tanh_cols_bwd: x, dy and dx must be non-NULL and 16-byte aligned");
  SMI_CHECK(dx != x && dx != dy, "gelu_tanh_cols_bwd: dx may alias neither x nor dy");
  const int grid = ew_grid(M * (C / 8));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(gelu_tanh_cols_bwd_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)x, (const f16*)dy, (f16*)dx, M, C / 8, ldx, ldy, ldd);
  else
    hipLaunchKernelGGL(gelu_tanh_cols_bwd_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)x, (const bf16*)dy, (bf16*)dx, M, C / 8, ldx, ldy, ldd);
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_flux_unpack_bwd(int dtype, const float* d_out, void* rows, int n, int Cout, int gh, int gw, int p,
                           const float* scale_dev, hipStream_t stream) {
  SMI_CHECK(n >= 1 && Cout >= 1 && gh >= 1 && gw >= 1 && p >= 1 && (Cout * p * p) % 8 == 0 && scale_dev,
            "flux_unpack_bwd: Cout p p %% 8 and a scale per sample (got Cout=%d p=%d)", Cout, p);
  SMI_CHECK(d_out && rows && (((uintptr_t)rows & 15) == 0) && (((uintptr_t)d_out & 7) == 0),
            "flux_unpack_bwd: rows must be 16-byte aligned, d_out 8-byte aligned");
  const int64_t nrows = (int64_t)n * gh * gw;
  const int grid = ew_grid(nrows * (Cout * p * p / 8));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(flux_unpack_bwd_kernel<f16>, dim3(grid), dim3(256), 0, stream, d_out, (f16*)rows, nrows, Cout, gh, gw, p, scale_dev);
  else
    hipLaunchKernelGGL(flux_unpack_bwd_kernel<bf16>, dim3(grid), dim3(256), 0, stream, d_out, (bf16*)rows, nrows, Cout, gh, gw, p, scale_dev);
  SMI_HIP(hipGetLastError());
  return 0;
}

}  // namespace smi
