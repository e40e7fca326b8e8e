// HBM-bound elementwise / data-movement kernels (16-byte lanes, grid-stride) and the slider-step ops
// (CFG combine, guidance loss + gradient, global-norm clip + AdamW, scheduler update).
#include "kernels.h"
#include <cstdlib>

namespace smi {
namespace {

inline int ew_grid(int64_t n_threads) {
  int64_t g = (n_threads + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}
#define GSTRIDE(i, total)                                                         \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (total); \
       i += (int64_t)gridDim.x * blockDim.x)

// GEGLU: out[m, c] = proj[m, c] * gelu(proj[m, C4 + c])                 (diffusers GEGLU, exact erf gelu)
template <typename T>
__global__ void geglu_fwd_kernel(const T* __restrict__ proj, T* __restrict__ out, int64_t M, int C4) {
  const int c8 = C4 / 8;
  GSTRIDE(i, M * c8) {
    const int64_t m = i / c8;
    const int c = (int)(i - m * c8) * 8;
    Pack8<T> h, g, o;
    h.u = *reinterpret_cast<const u32x4*>(proj + m * 2 * C4 + c);
    g.u = *reinterpret_cast<const u32x4*>(proj + m * 2 * C4 + C4 + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) o.e[e] = from_f<T>(to_f(h.e[e]) * gelu_f(to_f(g.e[e])));
    *reinterpret_cast<u32x4*>(out + m * C4 + c) = o.u;
  }
}
template <typename T>
__global__ void geglu_bwd_kernel(const T* __restrict__ proj, const T* __restrict__ dout, T* __restrict__ dproj,
                                 int64_t M, int C4) {
  const int c8 = C4 / 8;
  GSTRIDE(i, M * c8) {
    const int64_t m = i / c8;
    const int c = (int)(i - m * c8) * 8;
    Pack8<T> h, g, d, oh, og;
    h.u = *reinterpret_cast<const u32x4*>(proj + m * 2 * C4 + c);
    g.u = *reinterpret_cast<const u32x4*>(proj + m * 2 * C4 + C4 + c);
    d.u = *reinterpret_cast<const u32x4*>(dout + m * C4 + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float gv = to_f(g.e[e]), dv = to_f(d.e[e]);
      oh.e[e] = from_f<T>(dv * gelu_f(gv));
      og.e[e] = from_f<T>(dv * to_f(h.e[e]) * dgelu_f(gv));
    }
    *reinterpret_cast<u32x4*>(dproj + m * 2 * C4 + c) = oh.u;
    *reinterpret_cast<u32x4*>(dproj + m * 2 * C4 + C4 + c) = og.u;
  }
}

// tanh-GELU 0.5 x (1 + tanh(u)), u = sqrt(2 / pi) (x + 0.044715 x^3), as x sigmoid(2 u): one v_exp and one division
__device__ __forceinline__ float gelu_tanh_f(float x) {
  const float u2 = 1.5957691216057308f * x * __builtin_fmaf(0.044715f * x, x, 1.f);
  return x / (1.f + __expf(-u2));
}

// 0: silu(a)   1: a + b   2: quick_gelu(a) = a * sigmoid(1.702 a)   3: gelu(a) (erf)   4: gelu(a) (tanh form)
template <typename T, int OP>
__global__ void ew_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ y, int64_t n8) {
  GSTRIDE(i, n8) {
    Pack8<T> x, z, o;
    x.u = *reinterpret_cast<const u32x4*>(a + i * 8);
    if (OP == 1) z.u = *reinterpret_cast<const u32x4*>(b + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = to_f(x.e[e]);
      o.e[e] = from_f<T>(OP == 4   ? gelu_tanh_f(v)
                         : OP == 0 ? silu_f(v)
                         : OP == 1 ? v + to_f(z.e[e])
                         : OP == 2 ? v / (1.f + __expf(-1.702f * v))
                                   : gelu_f(v));
    }
    *reinterpret_cast<u32x4*>(y + i * 8) = o.u;
  }
}

// dx = dy * act'(x): KIND 0 quick_gelu (x sigmoid(1.702 x))' = s (1 + 1.702 x (1 - s)), KIND 1 erf-gelu (dgelu_f), KIND 2
// tanh-gelu (dgelu_tanh_f).  Whole 8-packs vectorised; the n % 8 tail elements one thread each
template <typename T, int KIND>
__device__ __forceinline__ float dact_f(float v) {
  if (KIND == 1) return dgelu_f(v);
  if (KIND == 2) return dgelu_tanh_f(v);
  const float s = 1.f / (1.f + __expf(-1.702f * v));
  return s * (1.f + 1.702f * v * (1.f - s));
}
template <typename T, int KIND>
__global__ void act_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx, int64_t n) {
  const int64_t n8 = n / 8;
  GSTRIDE(i, n8) {
    Pack8<T> a, g, o;
    a.u = *reinterpret_cast<const u32x4*>(x + i * 8);
    g.u = *reinterpret_cast<const u32x4*>(dy + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) o.e[e] = from_f<T>(to_f(g.e[e]) * dact_f<T, KIND>(to_f(a.e[e])));
    *reinterpret_cast<u32x4*>(dx + i * 8) = o.u;
  }
  const int64_t t = n8 * 8 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) dx[t] = from_f<T>(to_f(dy[t]) * dact_f<T, KIND>(to_f(x[t])));
}

template <typename T>
__global__ void copy_cols_kernel(const T* __restrict__ src, int64_t lds, T* __restrict__ dst, int64_t ldd, int col0,
                                 int64_t M, int C) {
  const int c8 = C / 8;
  GSTRIDE(i, M * c8) {
    const int64_t m = i / c8;
    const int c = (int)(i - m * c8) * 8;
    *reinterpret_cast<u32x4*>(dst + m * ldd + col0 + c) = *reinterpret_cast<const u32x4*>(src + m * lds + c);
  }
}

// the same copy out of the four phase planes of an up-sampler conv: destination row (n, oy, ox) of the 2H x 2W map reads row
// (n, oy >> 1, ox >> 1) of plane 2 (oy & 1) + (ox & 1); walked in destination order, the same bytes as copy_cols moves
template <typename T>
__global__ void copy_cols_phase_kernel(const T* __restrict__ src, T* __restrict__ dst, int64_t ldd, int col0, int Nb, int H,
                                       int W, int C) {
  const int c8 = C / 8;
  const int64_t plane = (int64_t)Nb * H * W;
  GSTRIDE(i, 4 * plane * c8) {
    const int64_t m = i / c8;
    const int c = (int)(i - m * c8) * 8;
    const int ox = (int)(m % (2 * W));
    const int64_t t = m / (2 * W);
    const int oy = (int)(t % (2 * H));
    const int64_t n = t / (2 * H);
    const int64_t s = (2 * (oy & 1) + (ox & 1)) * plane + (n * H + (oy >> 1)) * W + (ox >> 1);
    *reinterpret_cast<u32x4*>(dst + m * ldd + col0 + c) = *reinterpret_cast<const u32x4*>(src + s * C + c);
  }
}

// NCHW (T or f32) -> token-major [Nb, HW, Cpad] T (channels >= C zero filled), value * scale (or * *scale_dev)
template <typename T>
__global__ void nchw_to_nhwc_kernel(const void* __restrict__ src, int src_f32, T* __restrict__ dst, int Nb, int C,
                                    int HW, int Cpad, float scale, const float* __restrict__ scale_dev) {
  GSTRIDE(i, (int64_t)Nb * HW * Cpad) {
    const int c = (int)(i % Cpad);
    const int64_t pix = i / Cpad;
    const int64_t n = pix / HW, hw = pix - n * HW;
    const float sc = scale_dev ? scale * scale_dev[n] : scale;  // scale_dev: one factor per sample
    float v = 0.f;
    if (c < C) {
      const int64_t si = (n * C + c) * HW + hw;
      v = src_f32 ? reinterpret_cast<const float*>(src)[si] : to_f(reinterpret_cast<const T*>(src)[si]);
    }
    dst[i] = from_f<T>(v * sc);
  }
}
__global__ void nhwc_to_nchw_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, int Nb, int C,
                                        int HW) {
  GSTRIDE(i, (int64_t)Nb * C * HW) {
    const int64_t hw = i % HW;
    const int64_t nc = i / HW;
    const int64_t n = nc / C, c = nc - n * C;
    dst[i] = src[(n * HW + hw) * C + c];
  }
}

// diffusers get_timestep_embedding(flip_sin_to_cos=True, downscale_freq_shift=0): [cos(t f_i) | sin(t f_i)]
template <typename T>
__global__ void timestep_embed_kernel(const float* __restrict__ vals, T* __restrict__ out, int n, int dim) {
  const int half = dim / 2;
  GSTRIDE(i, (int64_t)n * dim) {
    const int j = (int)(i % dim);
    const int64_t r = i / dim;
    const int k = j < half ? j : j - half;
    const float freq = expf(-9.210340371976184f * (float)k / (float)half);  // ln(10000)
    const float a = vals[r] * freq;
    out[i] = from_f<T>(j < half ? cosf(a) : sinf(a));
  }
}

template <typename T>
__global__ void pool2x2_sum_kernel(const T* __restrict__ du, T* __restrict__ dx, int Nb, int H, int W, int C) {
  const int c8 = C / 8;
  GSTRIDE(i, (int64_t)Nb * H * W * c8) {
    const int c = (int)(i % c8) * 8;
    const int64_t pix = i / c8;
    const int x = (int)(pix % W);
    const int y = (int)((pix / W) % H);
    const int64_t n = pix / ((int64_t)W * H);
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        Pack8<T> v;
        v.u = *reinterpret_cast<const u32x4*>(du + ((n * 2 * H + 2 * y + a) * 2 * W + 2 * x + b) * C + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += to_f(v.e[e]);
      }
    Pack8<T> o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o.e[e] = from_f<T>(acc[e]);
    *reinterpret_cast<u32x4*>(dx + pix * C + c) = o.u;
  }
}

// out[n][c] = mul * sum_{hw} x[n][hw][c]  (gradient of a per-sample row vector added to every pixel: the time-embedding
// projection under a c3lier adaptor).  Two launches: partial sums over COLSUM_RS row slices per sample (a thread owns 8
// columns = one 16-byte load per row; 8 row lanes per workgroup meet in LDS in a fixed order), then a fixed-order sum of the
// slices -- deterministic.  (The one-launch form had C / 64 workgroups per sample walk all HW rows with 2-byte loads:
// 80 us per call at 4096 x 320, 1.75 ms per SD-1.4 c3lier step.)
constexpr int COLSUM_RS = 16;
template <typename T>
__global__ __launch_bounds__(256) void colsum_partial_kernel(const T* __restrict__ x, float* __restrict__ part, int HW,
                                                             int C) {
  __shared__ float red[8][32][8];
  const int n = blockIdx.z, rs = blockIdx.y;
  const int cv = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int c = (blockIdx.x * 32 + cv) * 8;
  const int rows = (HW + COLSUM_RS - 1) / COLSUM_RS;
  const int r0 = rs * rows, r1 = min(HW, r0 + rows);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    const T* p = x + (int64_t)n * HW * C + c;
    for (int r = r0 + rl; r < r1; r += 8) {
      Pack8<T> v;
      v.u = *reinterpret_cast<const u32x4*>(p + (int64_t)r * C);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += to_f(v.e[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[rl][cv][e] = acc[e];
  __syncthreads();
  if (rl == 0 && c < C) {
    float* o = part + ((int64_t)n * COLSUM_RS + rs) * C + c;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) t += red[j][cv][e];
      o[e] = t;
    }
  }
}
template <typename T>
__global__ void colsum_final_kernel(const float* __restrict__ part, T* __restrict__ out, int Nb, int C, int64_t ldo,
                                    float mul) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Nb * C) return;
  const int n = i / C, c = i - n * C;
  float t = 0.f;
  for (int rs = 0; rs < COLSUM_RS; ++rs) t += part[((int64_t)n * COLSUM_RS + rs) * C + c];
  out[(int64_t)n * ldo + c] = from_f<T>(t * mul);
}
// g[i] *= silu'(x[i]): an fp32 gradient against the 16-bit pre-activation (the embedding MLPs of the pooled-embedding
// gradient, which stays in fp32 from the grouped time_emb_proj product down to d(text_embeds))
template <typename T>
__global__ void silu_bwd_f32_kernel(const T* __restrict__ x, float* __restrict__ g, int64_t n) {
  GSTRIDE(i, n) g[i] *= dsilu_f(to_f(x[i]));
}
// dx[m][j] = sum_i dy[m][i] W[i][j], j < J: the input gradient of a Linear from its own [I, ldw] weight (no transposed
// copy), for a handful of fp32 rows.  A workgroup owns 64 columns; its 16 waves take every 16th i (128-byte row pieces)
// and meet in LDS in a fixed order -- deterministic
template <typename T>
__global__ __launch_bounds__(1024) void vecmat_f32_kernel(const float* __restrict__ dy, const T* __restrict__ W,
                                                          float* __restrict__ dx, int I, int64_t ldw, int J, int64_t lddx) {
  __shared__ float red[16][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + tx, m = blockIdx.y;
  float acc = 0.f;
  if (j < J)
    for (int i = ty; i < I; i += 16) acc += dy[(int64_t)m * I + i] * to_f(W[(int64_t)i * ldw + j]);
  red[ty][tx] = acc;
  __syncthreads();
  if (ty == 0 && j < J) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][tx];
    dx[(int64_t)m * lddx + j] = t;
  }
}
// CLIP text embeddings: out[n*L + l][:] = tok[ids[n*L + l]][:] + pos[l][:]
template <typename T>
__global__ void embed_kernel(const int* __restrict__ ids, const T* __restrict__ tok, const T* __restrict__ pos,
                             T* __restrict__ out, int64_t rows, int L, int d8, int vocab) {
  GSTRIDE(i, rows * d8) {
    const int c = (int)(i % d8);
    const int64_t r = i / d8;
    int id = ids[r];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    Pack8<T> a, b, o;
    a.u = *reinterpret_cast<const u32x4*>(tok + ((int64_t)id * d8 + c) * 8);
    o.u = a.u;
    if (pos) {  // NULL: a model without a position table (T5) -- the token rows as they are
      b.u = *reinterpret_cast<const u32x4*>(pos + ((int64_t)(r % L) * d8 + c) * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) o.e[e] = from_f<T>(to_f(a.e[e]) + to_f(b.e[e]));
    }
    *reinterpret_cast<u32x4*>(out + i * 8) = o.u;
  }
}
// out[n][:] = src[n * L + idx[n]][:]
template <typename T>
__global__ void gather_rows_kernel(const T* __restrict__ src, const int* __restrict__ idx, T* __restrict__ out, int n,
                                   int L, int d8) {
  GSTRIDE(i, (int64_t)n * d8) {
    const int c = (int)(i % d8);
    const int64_t r = i / d8;
    int j = idx[r];
    j = j < 0 ? 0 : (j >= L ? L - 1 : j);
    *reinterpret_cast<u32x4*>(out + i * 8) = *reinterpret_cast<const u32x4*>(src + ((r * L + j) * d8 + c) * 8);
  }
}
// one workgroup per row: max, sum of exp, normalised write (three passes over a row that sits in L2)
template <typename T>
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ S, T* __restrict__ P, int cols,
                                                           float scale) {
  __shared__ float sh[4];
  const float* s = S + (int64_t)blockIdx.x * cols;
  T* p = P + (int64_t)blockIdx.x * cols;
  float m = -3.0e38f;
  // the maximum of the SCALED scores (max(s) * scale is the minimum of them for a negative scale; the same bits for a
  // positive one, where rounding keeps the order)
  for (int i = threadIdx.x; i < cols; i += 256) m = fmaxf(m, s[i] * scale);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  __syncthreads();
  float sum = 0.f;
  for (int i = threadIdx.x; i < cols; i += 256) sum += __expf(s[i] * scale - m);
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = sum;
  __syncthreads();
  const float inv = 1.f / ((sh[0] + sh[1]) + (sh[2] + sh[3]));
  for (int i = threadIdx.x; i < cols; i += 256) p[i] = from_f<T>(__expf(s[i] * scale - m) * inv);
}
template <typename T>
__global__ void chan_mix_kernel(const float* __restrict__ x, const T* __restrict__ W, const T* __restrict__ b,
                                float* __restrict__ y, int64_t M, int C) {
  GSTRIDE(i, M * C) {
    const int j = (int)(i % C);
    const int64_t m = i / C;
    float acc = to_f(b[j]);
    for (int k = 0; k < C; ++k) acc += x[m * C + k] * to_f(W[j * C + k]);
    y[i] = acc;
  }
}
// dst[m][0..cpad) = (T)(src[m][0..cols) * mul), zero beyond cols   (fp32 rank-r rows -> a 64-channel MFMA operand)
template <typename T>
__global__ void f32_to_padded_kernel(const float* __restrict__ src, int lds, int cols, T* __restrict__ dst, int cpad,
                                     int64_t M, float mul) {
  GSTRIDE(i, M * cpad) {
    const int c = (int)(i % cpad);
    const int64_t m = i / cpad;
    dst[i] = from_f<T>(c < cols ? src[m * lds + c] * mul : 0.f);
  }
}

// ---- reductions to a scalar: block partials into scratch, last-stage by one block (deterministic order)
template <int OP>  // 0: max|x|   1: sum x^2
__global__ __launch_bounds__(256) void reduce_partial_kernel(const float* __restrict__ x, int64_t n,
                                                             float* __restrict__ partial) {
  __shared__ float sh[4];
  float acc = 0.f;
  GSTRIDE(i, n) {
    const float v = x[i];
    acc = OP == 0 ? fmaxf(acc, fabsf(v)) : acc + v * v;
  }
  acc = OP == 0 ? wave_max(acc) : wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    partial[blockIdx.x] = OP == 0 ? fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3])) : (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// one block per sample: scale[j] = 2^floor(log2(target / max|x_j|)) (power of two: exact), inv[j] = 1 / scale[j]
__global__ __launch_bounds__(256) void grad_scale_kernel(const float* __restrict__ x, int64_t per, float* __restrict__ out,
                                                         int inv_off, float target) {
  __shared__ float sh[4];
  const float* xs = x + (int64_t)blockIdx.x * per;
  float amax = 0.f;
  for (int64_t i = threadIdx.x; i < per; i += 256) amax = fmaxf(amax, fabsf(xs[i]));
  amax = wave_max(amax);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = amax;
  __syncthreads();
  if (threadIdx.x == 0) {
    amax = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
    float s = 1.f;
    if (amax > 0.f && isfinite(amax)) {
      // e = floor(log2(target / amax)) from the exponents, exactly: amax = ma 2^ea, target = mt 2^et with ma, mt in [0.5, 1),
      // so amax 2^e <= target < amax 2^(e + 1) for e = et - ea - (ma > mt).  (floorf(log2f(target / amax)) was one too large
      // when the quotient sat within an ulp below a power of two -- log2f rounds up to the integer -- and max * scale then
      // exceeded the target: DESIGN.md section 5.)
      int ea, et;
      const float ma = frexpf(amax, &ea), mt = frexpf(target, &et);
      int e = et - ea - (ma > mt ? 1 : 0);
      e = e > 40 ? 40 : (e < -40 ? -40 : e);
      s = ldexpf(1.f, e);
    }
    out[blockIdx.x] = s;
    out[inv_off + blockIdx.x] = 1.f / s;
  }
}

__global__ void cfg_combine_kernel(const float* __restrict__ e2, float* __restrict__ out, int64_t nh, float g) {
  GSTRIDE(i, nh) {
    const float u = e2[i], t = e2[nh + i];
    out[i] = u + g * (t - u);
  }
}

__global__ __launch_bounds__(256) void slider_loss_partial_kernel(const float* __restrict__ tg,
                                                                  const float* __restrict__ po,
                                                                  const float* __restrict__ ne,
                                                                  const float* __restrict__ ng, float sign_eta,
                                                                  int64_t n, float* __restrict__ dtarget,
                                                                  float* __restrict__ partial) {
  __shared__ float sh[4];
  float acc = 0.f;
  const float k = 2.f / (float)n;
  GSTRIDE(i, n) {
    const float goal = ne[i] + sign_eta * (po[i] - ng[i]);
    const float d = tg[i] - goal;
    acc += d * d;
    if (dtarget) dtarget[i] = k * d;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__global__ void sum_finalize_kernel(const float* __restrict__ partial, int np, float mul, float* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < np; ++i) s += partial[i];
    out[0] = s * mul;
  }
}

// null-text inner step after the UNet call: guided eps, DDIM prev_step, MSE against the target latent and d(loss)/d(eps_u).
// One workgroup (gridDim.x == 1) writes the loss itself; more write one partial each for sum_finalize_kernel.
__global__ __launch_bounds__(256) void nulltext_loss_kernel(const float* __restrict__ eu, const float* __restrict__ ec,
                                                            const float* __restrict__ xt, const float* __restrict__ tg,
                                                            float g, float cx, float ce, int64_t n,
                                                            float* __restrict__ d_eu, float* __restrict__ partial,
                                                            float* __restrict__ loss_out) {
  __shared__ float sh[4];
  float acc = 0.f;
  const float k = (1.f - g) * ce * (2.f / (float)n);
  GSTRIDE(i, n) {
    const float u = eu[i];
    const float eps = u + g * (ec[i] - u);
    const float d = (cx * xt[i] + ce * eps) - tg[i];
    acc += d * d;
    if (d_eu) d_eu[i] = k * d;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float s = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    if (gridDim.x == 1) loss_out[0] = s * (1.f / (float)n);
    else partial[blockIdx.x] = s;
  }
}

__global__ void axpby_kernel(float* __restrict__ y, const float* __restrict__ x, float a, float b, int64_t n) {
  GSTRIDE(i, n) y[i] = a * x[i] + b * y[i];
}

// torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW (decoupled weight decay), single fused pass.
// norm_sq_dev: device scalar holding sum g^2 (only read when max_norm > 0)
__global__ void clip_adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                  float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                                  float bc1, float bc2_sqrt, float max_norm, const float* __restrict__ norm_sq_dev) {
  float coef = 1.f;
  if (max_norm > 0.f) {
    const float total = sqrtf(norm_sq_dev[0]);
    coef = fminf(max_norm / (total + 1e-6f), 1.f);
  }
  GSTRIDE(i, n) {
    const float gi = g[i] * coef;
    float pi = p[i] * (1.f - lr * wd);
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi -= (lr / bc1) * (mi / denom);
    p[i] = pi;
  }
}

// ---- Lion and Prodigy (include/smi.h states both algorithms).  Flat fp32 vectors; whole 4-packs go through 16-byte accesses
// when every pointer is 16-byte aligned (VEC), the n % 4 tail -- or, unaligned, every element -- one thread each.
__device__ __forceinline__ float clip_coef(float max_norm, const float* __restrict__ norm_sq_dev) {
  if (!(max_norm > 0.f)) return 1.f;
  return fminf(max_norm / (sqrtf(norm_sq_dev[0]) + 1e-6f), 1.f);
}

// The roundings are spelled out (fmaf where one is meant, contraction off for the rest) as torch's CPU kernels round
// the same updates -- x.mul_(b).add_(g, alpha=a) is fma(a, g, fl(b x)) -- so that the fp32 emulation of the tests is THIS
// arithmetic and a one-element vector agrees with it to the bit.
// The sum of np <= 1024 fp32 workgroup partials in double by ONE wave (blockDim.x == 64), in a fixed order: lane l adds
// its run of consecutive partials in index order, then the 64 lane sums are added in lane order.  Every lane gets the total.
__device__ __forceinline__ double ordered_sum_f64(const float* __restrict__ part, int np, double* sh) {
  const int lane = threadIdx.x, per = (np + 63) / 64;
  const int end = (lane + 1) * per < np ? (lane + 1) * per : np;
  double acc = 0.0;
  for (int i = lane * per; i < end; ++i) acc += (double)part[i];
  sh[lane] = acc;
  __syncthreads();
  double total = 0.0;
  for (int l = 0; l < 64; ++l) total += sh[l];
  __syncthreads();  // sh is free for the next sum
  return total;
}
// sum g^2 for Lion and Prodigy: the partials of reduce_partial_kernel<1>, added in double.  (sum_finalize_kernel adds them
// one by one in fp32; at 1024 partials that sum is ~5e-7 off, the clip coefficient 2.5e-7, and every clipped gradient with
// it -- 4.4 to 4.8 times the error of an fp32 step with an accurate norm, measured: DESIGN.md section 16.  AdamW keeps it:
// its bits are pinned.)
__global__ __launch_bounds__(64) void sum_finalize_f64_kernel(const float* __restrict__ partial, int np,
                                                              float* __restrict__ out) {
  __shared__ double sh[64];
  const double s = ordered_sum_f64(partial, np, sh);
  if (threadIdx.x == 0) out[0] = (float)s;
}

struct LionArgs {  // coefficients rounded to fp32 once on the host, from the doubles of the C ABI
  float lr, b1, b2, one_minus_b1, one_minus_b2, decay, max_norm;  // decay = 1 - lr * weight_decay
};
__device__ __forceinline__ void lion_elem(float& p, float g, float& m, const LionArgs& a, float coef) {
#pragma clang fp contract(off)
  const float gi = g * coef;
  const float c = fmaf(a.one_minus_b1, gi, m * a.b1);
  const float sgn = (float)((c > 0.f) - (c < 0.f));  // three-way, as torch.sign: an exactly zero c leaves p to the decay alone
  p = fmaf(-a.lr, sgn, p * a.decay);
  m = fmaf(a.one_minus_b2, gi, m * a.b2);
}
template <bool VEC>
__global__ __launch_bounds__(256) void clip_lion_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, int64_t n, LionArgs a,
                                                        const float* __restrict__ norm_sq_dev) {
  const float coef = clip_coef(a.max_norm, norm_sq_dev);
  const int64_t n4 = VEC ? n / 4 : 0;
  GSTRIDE(i, n4) {
    float4 pv = reinterpret_cast<const float4*>(p)[i], mv = reinterpret_cast<const float4*>(m)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    lion_elem(pv.x, gv.x, mv.x, a, coef);
    lion_elem(pv.y, gv.y, mv.y, a, coef);
    lion_elem(pv.z, gv.z, mv.z, a, coef);
    lion_elem(pv.w, gv.w, mv.w, a, coef);
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float pi = p[i], mi = m[i];
    lion_elem(pi, g[i], mi, a, coef);
    p[i] = pi;
    m[i] = mi;
  }
}

// Prodigy's device state block (doubles): what the group carries from step to step, and what one step's finalize leaves
// for its apply
enum { PS_D = 0, PS_DMAX = 1, PS_NUM = 2, PS_K = 3, PS_DLR = 4, PS_DNEW = 5, PS_SKIP = 6, PS_COUNT = 8 };
struct ProdigyArgs {
  double lr, b1, b2, b3, eps, wd, d0, d_coef, growth;
  float max_norm;
  int decouple, bias_corr, safeguard;
};
// dlr = d * lr * bc of the step that begins at state (d, k): formed on the device, identically by every thread that needs it
__device__ __forceinline__ double prodigy_dlr(const double* __restrict__ st, const ProdigyArgs& a) {
  double bc = 1.0;
  if (a.bias_corr) {
    const double k1 = st[PS_K] + 1.0;
    bc = sqrt(1.0 - pow(a.b2, k1)) / (1.0 - pow(a.b1, k1));
  }
  return st[PS_D] * a.lr * bc;
}

__global__ void prodigy_init_kernel(const float* __restrict__ p, float* __restrict__ p0, float* __restrict__ m,
                                    float* __restrict__ v, float* __restrict__ s, int64_t n, double d0,
                                    double* __restrict__ st) {
  GSTRIDE(i, n) {
    p0[i] = p[i];
    m[i] = 0.f;
    v[i] = 0.f;
    s[i] = 0.f;
  }
  if (blockIdx.x == 0 && threadIdx.x < PS_COUNT)
    st[threadIdx.x] = (threadIdx.x == PS_D || threadIdx.x == PS_DMAX || threadIdx.x == PS_DNEW) ? d0 : 0.0;
}

struct ProdigyCoef {  // the step's scalars, rounded to fp32 once (the reference package hands Python floats to fp32 tensor ops)
  float coef, wd_l2, b1, b2, b3, cm, cv, cs;
};
__device__ __forceinline__ void prodigy_acc_elem(float p, float g, float p0, float& m, float& v, float& s,
                                                 const ProdigyCoef& c, float& num, float& den) {
#pragma clang fp contract(off)
  const float gi = fmaf(c.wd_l2, p, g * c.coef);  // clip, then the coupled decay (0 when decoupled or none)
  num += gi * (p0 - p);
  m = fmaf(c.cm, gi, m * c.b1);
  v = fmaf(c.cv * gi, gi, v * c.b2);
  s = fmaf(c.cs, gi, s * c.b3);
  den += fabsf(s);
}
// accumulate: the three state updates per element, one partial per workgroup of sum g (p0 - p) and of sum |s|
template <bool VEC>
__global__ __launch_bounds__(256) void prodigy_accum_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                            const float* __restrict__ p0, float* __restrict__ m,
                                                            float* __restrict__ v, float* __restrict__ s, int64_t n,
                                                            ProdigyArgs a, const double* __restrict__ st,
                                                            const float* __restrict__ norm_sq_dev,
                                                            float* __restrict__ part_num, float* __restrict__ part_den) {
  __shared__ float sh[8];
  const double d = st[PS_D], dlr = prodigy_dlr(st, a);
  ProdigyCoef c;
  c.coef = clip_coef(a.max_norm, norm_sq_dev);
  c.wd_l2 = (a.wd != 0.0 && !a.decouple) ? (float)a.wd : 0.f;
  c.b1 = (float)a.b1, c.b2 = (float)a.b2, c.b3 = (float)a.b3;
  c.cm = (float)(d * (1.0 - a.b1));
  c.cv = (float)(d * d * (1.0 - a.b2));
  c.cs = (float)((d / a.d0) * (a.safeguard ? d : dlr));
  float num = 0.f, den = 0.f;
  const int64_t n4 = VEC ? n / 4 : 0;
  GSTRIDE(i, n4) {
    const float4 pv = reinterpret_cast<const float4*>(p)[i], gv = reinterpret_cast<const float4*>(g)[i];
    const float4 qv = reinterpret_cast<const float4*>(p0)[i];
    float4 mv = reinterpret_cast<const float4*>(m)[i], vv = reinterpret_cast<const float4*>(v)[i];
    float4 sv = reinterpret_cast<const float4*>(s)[i];
    prodigy_acc_elem(pv.x, gv.x, qv.x, mv.x, vv.x, sv.x, c, num, den);
    prodigy_acc_elem(pv.y, gv.y, qv.y, mv.y, vv.y, sv.y, c, num, den);
    prodigy_acc_elem(pv.z, gv.z, qv.z, mv.z, vv.z, sv.z, c, num, den);
    prodigy_acc_elem(pv.w, gv.w, qv.w, mv.w, vv.w, sv.w, c, num, den);
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
    reinterpret_cast<float4*>(s)[i] = sv;
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float mi = m[i], vi = v[i], si = s[i];
    prodigy_acc_elem(p[i], g[i], p0[i], mi, vi, si, c, num, den);
    m[i] = mi;
    v[i] = vi;
    s[i] = si;
  }
  num = wave_sum(num);
  den = wave_sum(den);
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6] = num;
    sh[4 + (threadIdx.x >> 6)] = den;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part_num[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    part_den[blockIdx.x] = (sh[4] + sh[5]) + (sh[6] + sh[7]);
  }
}
// finalize: one wave adds the partials in double (ordered_sum_f64); lane 0 applies the rules for d_numerator, d, d_max, k
__global__ __launch_bounds__(64) void prodigy_finalize_kernel(const float* __restrict__ part_num,
                                                              const float* __restrict__ part_den, int np, ProdigyArgs a,
                                                              double* __restrict__ st) {
  __shared__ double sh[64];
  const double sum_num = ordered_sum_f64(part_num, np, sh);
  const double den = ordered_sum_f64(part_den, np, sh);
  if (threadIdx.x != 0) return;
  double d = st[PS_D], d_max = st[PS_DMAX];
  const double dlr = prodigy_dlr(st, a);
  double num = a.b3 * st[PS_NUM];
  if (a.lr > 0.0) num += (d / a.d0) * dlr * sum_num;
  st[PS_NUM] = num;
  st[PS_DLR] = dlr;
  if (den == 0.0) {  // no gradient has arrived yet: the moments above are updated, p, d and k are not
    st[PS_DNEW] = d;
    st[PS_SKIP] = 1.0;
    return;
  }
  if (a.lr > 0.0) {
    const double d_hat = a.d_coef * num / den;
    if (d == a.d0) d = fmax(d, d_hat);
    d_max = fmax(d_max, d_hat);
    d = fmin(d_max, d * a.growth);
  }
  st[PS_D] = d;
  st[PS_DMAX] = d_max;
  st[PS_K] = st[PS_K] + 1.0;
  st[PS_DNEW] = d;
  st[PS_SKIP] = 0.0;
}
// apply: p -= wd dlr p (decoupled);  p -= dlr exp_avg / (sqrt(exp_avg_sq) + d eps) with the step's OLD dlr and NEW d
template <bool VEC>
__global__ __launch_bounds__(256) void prodigy_apply_kernel(float* __restrict__ p, const float* __restrict__ m,
                                                            const float* __restrict__ v, int64_t n, ProdigyArgs a,
                                                            const double* __restrict__ st) {
#pragma clang fp contract(off)
  if (st[PS_SKIP] != 0.0) return;
  const float dlr = (float)st[PS_DLR], deps = (float)(st[PS_DNEW] * a.eps);
  const float wdl = (a.wd != 0.0 && a.decouple) ? (float)(a.wd * st[PS_DLR]) : 0.f;
  const int64_t n4 = VEC ? n / 4 : 0;
  // p.add_(p, alpha=-wd dlr) is fma(-wdl, p, p); p.addcdiv_(m, denom, value=-dlr) is p + fl(fl(-dlr m) / denom)
#define PRODIGY_APPLY(P_, M_, V_) (fmaf(-wdl, (P_), (P_)) + (-dlr * (M_)) / (sqrtf(V_) + deps))
  GSTRIDE(i, n4) {
    float4 pv = reinterpret_cast<const float4*>(p)[i];
    const float4 mv = reinterpret_cast<const float4*>(m)[i], vv = reinterpret_cast<const float4*>(v)[i];
    pv.x = PRODIGY_APPLY(pv.x, mv.x, vv.x);
    pv.y = PRODIGY_APPLY(pv.y, mv.y, vv.y);
    pv.z = PRODIGY_APPLY(pv.z, mv.z, vv.z);
    pv.w = PRODIGY_APPLY(pv.w, mv.w, vv.w);
    reinterpret_cast<float4*>(p)[i] = pv;
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float pi = p[i];
    p[i] = PRODIGY_APPLY(pi, m[i], v[i]);
  }
#undef PRODIGY_APPLY
}

__global__ void sched_affine_kernel(float* __restrict__ x, const float* __restrict__ eps,
                                    const float* __restrict__ noise, float cx, float ce, float cn, int64_t n) {
  GSTRIDE(i, n) {
    float v = cx * x[i] + ce * eps[i];
    if (noise) v += cn * noise[i];
    x[i] = v;
  }
}

}  // namespace

int launch_geglu_fwd(int dtype, const void* proj, void* out, int M, int C4, hipStream_t stream) {
  SMI_CHECK(C4 % 8 == 0, "geglu: C4 %% 8");
  const int grid = ew_grid((int64_t)M * C4 / 8);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(geglu_fwd_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)proj, (f16*)out, (int64_t)M, C4);
  else
    hipLaunchKernelGGL(geglu_fwd_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)proj, (bf16*)out, (int64_t)M, C4);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_geglu_bwd(int dtype, const void* proj, const void* dout, void* dproj, int M, int C4, hipStream_t stream) {
  SMI_CHECK(C4 % 8 == 0, "geglu: C4 %% 8");
  const int grid = ew_grid((int64_t)M * C4 / 8);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(geglu_bwd_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)proj, (const f16*)dout, (f16*)dproj, (int64_t)M, C4);
  else
    hipLaunchKernelGGL(geglu_bwd_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)proj, (const bf16*)dout, (bf16*)dproj, (int64_t)M, C4);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_silu(int dtype, const void* x, void* y, int64_t n, hipStream_t stream) {
  SMI_CHECK(n % 8 == 0, "silu: n %% 8");
  const int grid = ew_grid(n / 8);
  if (dtype == DT_F16)
    hipLaunchKernelGGL((ew_kernel<f16, 0>), dim3(grid), dim3(256), 0, stream, (const f16*)x, nullptr, (f16*)y, n / 8);
  else
    hipLaunchKernelGGL((ew_kernel<bf16, 0>), dim3(grid), dim3(256), 0, stream, (const bf16*)x, nullptr, (bf16*)y, n / 8);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_act(int dtype, const void* x, void* y, int64_t n, int kind, hipStream_t stream) {
  SMI_CHECK(n % 8 == 0 && kind >= 0 && kind <= 2, "act: n %% 8, kind 0 (quick_gelu), 1 (gelu) or 2 (tanh gelu)");
  const int grid = ew_grid(n / 8);
#define L(TT_, OP_) hipLaunchKernelGGL((ew_kernel<TT_, OP_>), dim3(grid), dim3(256), 0, stream, (const TT_*)x, nullptr, (TT_*)y, n / 8)
  if (dtype == DT_F16) {
    if (kind == 0) L(f16, 2); else if (kind == 1) L(f16, 3); else L(f16, 4);
  } else {
    if (kind == 0) L(bf16, 2); else if (kind == 1) L(bf16, 3); else L(bf16, 4);
  }
#undef L
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_act_bwd(int dtype, const void* x, const void* dy, void* dx, int64_t n, int kind, hipStream_t stream) {
  SMI_CHECK(n >= 1 && kind >= 0 && kind <= 2, "act bwd: n >= 1, kind 0 (quick_gelu), 1 (gelu) or 2 (tanh gelu)");
  SMI_CHECK((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0, "act bwd: x, dy and dx must be 16-byte aligned");
  const int grid = ew_grid(n / 8 > 0 ? n / 8 : 1);
#define L(TT_, K_) hipLaunchKernelGGL((act_bwd_kernel<TT_, K_>), dim3(grid), dim3(256), 0, stream, (const TT_*)x, (const TT_*)dy, (TT_*)dx, n)
  if (dtype == DT_F16) {
    if (kind == 0) L(f16, 0); else if (kind == 1) L(f16, 1); else L(f16, 2);
  } else {
    if (kind == 0) L(bf16, 0); else if (kind == 1) L(bf16, 1); else L(bf16, 2);
  }
#undef L
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_embed(int dtype, const int* ids, const void* tok, const void* pos, void* out, int64_t rows, int L, int d,
                 int vocab, hipStream_t stream) {
  SMI_CHECK(d % 8 == 0, "embed: d %% 8");
  const int grid = ew_grid(rows * (d / 8));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(embed_kernel<f16>, dim3(grid), dim3(256), 0, stream, ids, (const f16*)tok, (const f16*)pos, (f16*)out, rows, L, d / 8, vocab);
  else
    hipLaunchKernelGGL(embed_kernel<bf16>, dim3(grid), dim3(256), 0, stream, ids, (const bf16*)tok, (const bf16*)pos, (bf16*)out, rows, L, d / 8, vocab);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_gather_rows(int dtype, const void* src, const int* idx, void* out, int n, int L, int d, hipStream_t stream) {
  SMI_CHECK(d % 8 == 0, "gather_rows: d %% 8");
  const int grid = ew_grid((int64_t)n * (d / 8));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(gather_rows_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)src, idx, (f16*)out, n, L, d / 8);
  else
    hipLaunchKernelGGL(gather_rows_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)src, idx, (bf16*)out, n, L, d / 8);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_add(int dtype, const void* a, const void* b, void* y, int64_t n, hipStream_t stream) {
  SMI_CHECK(n % 8 == 0, "add: n %% 8");
  const int grid = ew_grid(n / 8);
  if (dtype == DT_F16)
    hipLaunchKernelGGL((ew_kernel<f16, 1>), dim3(grid), dim3(256), 0, stream, (const f16*)a, (const f16*)b, (f16*)y, n / 8);
  else
    hipLaunchKernelGGL((ew_kernel<bf16, 1>), dim3(grid), dim3(256), 0, stream, (const bf16*)a, (const bf16*)b, (bf16*)y, n / 8);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_copy_cols(int dtype, const void* src, int64_t lds, void* dst, int64_t ldd, int col0, int M, int C,
                     hipStream_t stream) {
  (void)dtype;
  SMI_CHECK(C % 8 == 0 && lds % 8 == 0 && ldd % 8 == 0 && col0 % 8 == 0, "copy_cols: 16-byte alignment");
  const int grid = ew_grid((int64_t)M * C / 8);
  hipLaunchKernelGGL(copy_cols_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)src, lds, (f16*)dst, ldd, col0, (int64_t)M, C);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_copy_cols_phase(int dtype, const void* src, void* dst, int64_t ldd, int col0, int Nb, int H, int W, int C,
                           hipStream_t stream) {
  (void)dtype;
  SMI_CHECK(C % 8 == 0 && ldd % 8 == 0 && col0 % 8 == 0, "copy_cols_phase: 16-byte alignment");
  SMI_CHECK(Nb > 0 && H > 0 && W > 0 && col0 >= 0 && col0 + C <= ldd, "copy_cols_phase: bad shape");
  const int grid = ew_grid((int64_t)4 * Nb * H * W * C / 8);
  hipLaunchKernelGGL(copy_cols_phase_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)src, (f16*)dst, ldd, col0, Nb, H,
                     W, C);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_nchw_to_nhwc(int dtype, const void* src, int src_f32, void* dst, int Nb, int C, int HW, int Cpad,
                        float scale, hipStream_t stream) {
  const int grid = ew_grid((int64_t)Nb * HW * Cpad);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<f16>, dim3(grid), dim3(256), 0, stream, src, src_f32, (f16*)dst, Nb, C, HW, Cpad, scale, (const float*)nullptr);
  else
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<bf16>, dim3(grid), dim3(256), 0, stream, src, src_f32, (bf16*)dst, Nb, C, HW, Cpad, scale, (const float*)nullptr);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_nchw_to_nhwc_scaled(int dtype, const float* src, void* dst, int Nb, int C, int HW, int Cpad,
                               const float* scale_dev, hipStream_t stream) {
  const int grid = ew_grid((int64_t)Nb * HW * Cpad);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const void*)src, 1, (f16*)dst, Nb, C, HW, Cpad, 1.f, scale_dev);
  else
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const void*)src, 1, (bf16*)dst, Nb, C, HW, Cpad, 1.f, scale_dev);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_nhwc_to_nchw_f32(const float* src, float* dst, int Nb, int C, int HW, hipStream_t stream) {
  hipLaunchKernelGGL(nhwc_to_nchw_f32_kernel, dim3(ew_grid((int64_t)Nb * C * HW)), dim3(256), 0, stream, src, dst, Nb, C, HW);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_timestep_embed(int dtype, const float* vals, void* out, int n, int dim, hipStream_t stream) {
  SMI_CHECK(dim % 2 == 0, "timestep_embed: odd dim");
  const int grid = ew_grid((int64_t)n * dim);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(timestep_embed_kernel<f16>, dim3(grid), dim3(256), 0, stream, vals, (f16*)out, n, dim);
  else
    hipLaunchKernelGGL(timestep_embed_kernel<bf16>, dim3(grid), dim3(256), 0, stream, vals, (bf16*)out, n, dim);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_pool2x2_sum(int dtype, const void* du, void* dx, int Nb, int H, int W, int C, hipStream_t stream) {
  SMI_CHECK(C % 8 == 0, "pool2x2: C %% 8");
  const int grid = ew_grid((int64_t)Nb * H * W * C / 8);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(pool2x2_sum_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)du, (f16*)dx, Nb, H, W, C);
  else
    hipLaunchKernelGGL(pool2x2_sum_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)du, (bf16*)dx, Nb, H, W, C);
  SMI_HIP(hipGetLastError());
  return 0;
}
// scale_out[j] = scale of sample j, scale_out[inv_off + j] = its inverse
int launch_grad_scale(const float* d_eps, int n_samples, int64_t per_sample, float* scale_out, int inv_off,
                      hipStream_t stream) {
  static const float target = [] {
    const char* v = getenv("SMI_GRAD_TARGET_LOG2");
    return exp2f(v ? (float)atoi(v) : 4.f);
  }();
  hipLaunchKernelGGL(grad_scale_kernel, dim3(n_samples), dim3(256), 0, stream, d_eps, per_sample, scale_out, inv_off,
                     target);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_cfg_combine(const float* eps2, float* out, int64_t n_half, float g, hipStream_t stream) {
  hipLaunchKernelGGL(cfg_combine_kernel, dim3(ew_grid(n_half)), dim3(256), 0, stream, eps2, out, n_half, g);
  SMI_HIP(hipGetLastError());
  return 0;
}
// scratch: >= 256 floats
int launch_slider_loss(const float* target, const float* positive, const float* neutral, const float* negative,
                       float sign_eta, int64_t n, float* loss_out, float* dtarget, float* scratch,
                       hipStream_t stream) {
  const int np = ew_grid(n) > 256 ? 256 : ew_grid(n);
  hipLaunchKernelGGL(slider_loss_partial_kernel, dim3(np), dim3(256), 0, stream, target, positive, neutral, negative,
                     sign_eta, n, dtarget, scratch);
  hipLaunchKernelGGL(sum_finalize_kernel, dim3(1), dim3(64), 0, stream, scratch, np, 1.f / (float)n, loss_out);
  SMI_HIP(hipGetLastError());
  return 0;
}
// scratch: >= 256 floats.  Up to 65536 elements (a 4 x 128 x 128 latent) one workgroup does everything in ONE launch -- the
// inner loop of null-text optimisation runs at 4 x 64 x 64; beyond, block partials and the ordered sum of smi_slider_loss
int launch_nulltext_loss(const float* eps_u, const float* eps_c, const float* x_t, const float* target, float g, float c_x,
                         float c_eps, int64_t n, float* loss_out, float* d_eps_u, float* scratch, hipStream_t stream) {
  SMI_CHECK(eps_u && eps_c && x_t && target && loss_out && scratch && n > 0, "nulltext_loss: bad arguments");
  const int np = n <= 65536 ? 1 : (ew_grid(n) > 256 ? 256 : ew_grid(n));
  hipLaunchKernelGGL(nulltext_loss_kernel, dim3(np), dim3(256), 0, stream, eps_u, eps_c, x_t, target, g, c_x, c_eps, n,
                     d_eps_u, scratch, loss_out);
  if (np > 1) hipLaunchKernelGGL(sum_finalize_kernel, dim3(1), dim3(64), 0, stream, scratch, np, 1.f / (float)n, loss_out);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_axpby(float* y, const float* x, float a, float b, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(axpby_kernel, dim3(ew_grid(n)), dim3(256), 0, stream, y, x, a, b, n);
  SMI_HIP(hipGetLastError());
  return 0;
}
// scratch: >= 1 + 1024 floats ([0] = sum g^2, [1..] block partials)
int launch_clip_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                      float eps, float weight_decay, int step, float max_norm, float* scratch, hipStream_t stream) {
  SMI_CHECK(step >= 1, "adamw: step must start at 1");
  if (max_norm > 0.f) {
    const int np = ew_grid(n) > 1024 ? 1024 : ew_grid(n);
    hipLaunchKernelGGL(reduce_partial_kernel<1>, dim3(np), dim3(256), 0, stream, g, n, scratch + 1);
    hipLaunchKernelGGL(sum_finalize_kernel, dim3(1), dim3(64), 0, stream, scratch + 1, np, 1.f, scratch);
  }
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2 = 1.f - powf(beta2, (float)step);
  hipLaunchKernelGGL(clip_adamw_kernel, dim3(ew_grid(n)), dim3(256), 0, stream, p, g, m, v, n, lr, beta1, beta2, eps,
                     weight_decay, bc1, sqrtf(bc2), max_norm, scratch);
  SMI_HIP(hipGetLastError());
  return 0;
}
namespace {
// sum g^2 into scratch[0] through scratch[1 .. 1024]: the partials of launch_clip_adamw, the last stage in double
void launch_grad_norm_sq(const float* g, int64_t n, float* scratch, hipStream_t stream) {
  const int np = ew_grid(n) > 1024 ? 1024 : ew_grid(n);
  hipLaunchKernelGGL(reduce_partial_kernel<1>, dim3(np), dim3(256), 0, stream, g, n, scratch + 1);
  hipLaunchKernelGGL(sum_finalize_f64_kernel, dim3(1), dim3(64), 0, stream, scratch + 1, np, scratch);
}
inline bool aligned16(std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* q : ptrs) bits |= (uintptr_t)q;
  return (bits & 15) == 0;
}
// workgroups of an optimiser kernel over n elements, 4 per thread where vectorised; the cap is also the partial count
inline int optim_grid(int64_t n, bool vec) {
  const int g = ew_grid(vec ? (n + 3) / 4 : n);
  return g > 1024 ? 1024 : g;
}
}  // namespace

// scratch: >= 1 + 1024 floats
int launch_clip_lion(float* p, const float* g, float* m, int64_t n, double lr, double beta1, double beta2,
                     double weight_decay, float max_norm, float* scratch, hipStream_t stream) {
  SMI_CHECK(p && g && m && n > 0 && (max_norm <= 0.f || scratch), "lion: bad arguments");
  if (max_norm > 0.f) launch_grad_norm_sq(g, n, scratch, stream);
  const LionArgs a{(float)lr,           (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),
                   (float)(1.0 - lr * weight_decay), max_norm};
  const bool vec = aligned16({p, g, m});
  if (vec)
    hipLaunchKernelGGL(clip_lion_kernel<true>, dim3(optim_grid(n, true)), dim3(256), 0, stream, p, g, m, n, a, scratch);
  else
    hipLaunchKernelGGL(clip_lion_kernel<false>, dim3(optim_grid(n, false)), dim3(256), 0, stream, p, g, m, n, a, scratch);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_prodigy_init(const float* p, float* p0, float* m, float* v, float* s, int64_t n, double d0, double* state,
                        hipStream_t stream) {
  SMI_CHECK(p && p0 && m && v && s && state && n > 0 && d0 > 0.0, "prodigy_init: bad arguments");
  hipLaunchKernelGGL(prodigy_init_kernel, dim3(ew_grid(n)), dim3(256), 0, stream, p, p0, m, v, s, n, d0, state);
  SMI_HIP(hipGetLastError());
  return 0;
}
// scratch: >= 1 + 3 * 1024 floats ([0] = sum g^2, then 1024 partials each of sum g^2, sum g (p0 - p), sum |s|)
int launch_clip_prodigy(float* p, const float* g, const float* p0, float* m, float* v, float* s, int64_t n,
                        const ProdigyHyper* h, float max_norm, double* state, float* scratch, hipStream_t stream) {
  SMI_CHECK(p && g && p0 && m && v && s && h && state && scratch && n > 0 && ((uintptr_t)state & 7) == 0, "prodigy: bad arguments");
  SMI_CHECK(h->d0 > 0.0 && h->beta3 > 0.0, "prodigy: d0 and beta3 must be positive (beta3: pass sqrt(beta2) for the default)");
  if (max_norm > 0.f) launch_grad_norm_sq(g, n, scratch, stream);
  const ProdigyArgs a{h->lr,     h->beta1,       h->beta2,    h->beta3,          h->eps,
                      h->weight_decay, h->d0,    h->d_coef,   h->growth_rate,    max_norm,
                      h->decouple, h->use_bias_correction, h->safeguard_warmup};
  float* part_num = scratch + 1 + 1024;
  float* part_den = scratch + 1 + 2048;
  const bool vec = aligned16({p, g, p0, m, v, s});
  const int grid = optim_grid(n, vec);
  if (vec) {
    hipLaunchKernelGGL(prodigy_accum_kernel<true>, dim3(grid), dim3(256), 0, stream, p, g, p0, m, v, s, n, a, state, scratch,
                       part_num, part_den);
    hipLaunchKernelGGL(prodigy_finalize_kernel, dim3(1), dim3(64), 0, stream, part_num, part_den, grid, a, state);
    hipLaunchKernelGGL(prodigy_apply_kernel<true>, dim3(grid), dim3(256), 0, stream, p, m, v, n, a, state);
  } else {
    hipLaunchKernelGGL(prodigy_accum_kernel<false>, dim3(grid), dim3(256), 0, stream, p, g, p0, m, v, s, n, a, state, scratch,
                       part_num, part_den);
    hipLaunchKernelGGL(prodigy_finalize_kernel, dim3(1), dim3(64), 0, stream, part_num, part_den, grid, a, state);
    hipLaunchKernelGGL(prodigy_apply_kernel<false>, dim3(grid), dim3(256), 0, stream, p, m, v, n, a, state);
  }
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_sched_affine(float* x, const float* eps, const float* noise, float c_x, float c_eps, float c_noise,
                        int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(sched_affine_kernel, dim3(ew_grid(n)), dim3(256), 0, stream, x, eps, noise, c_x, c_eps, c_noise, n);
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_softmax_rows(int dtype, const float* S, void* P, int rows, int cols, float scale, hipStream_t stream) {
  if (dtype == DT_F16)
    hipLaunchKernelGGL(softmax_rows_kernel<f16>, dim3(rows), dim3(256), 0, stream, S, (f16*)P, cols, scale);
  else
    hipLaunchKernelGGL(softmax_rows_kernel<bf16>, dim3(rows), dim3(256), 0, stream, S, (bf16*)P, cols, scale);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_chan_mix(int dtype, const float* x, const void* W, const void* b, float* y, int64_t M, int C,
                    hipStream_t stream) {
  const int grid = ew_grid(M * C);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(chan_mix_kernel<f16>, dim3(grid), dim3(256), 0, stream, x, (const f16*)W, (const f16*)b, y, M, C);
  else
    hipLaunchKernelGGL(chan_mix_kernel<bf16>, dim3(grid), dim3(256), 0, stream, x, (const bf16*)W, (const bf16*)b, y, M, C);
  SMI_HIP(hipGetLastError());
  return 0;
}
size_t colsum_scratch_floats(int Nb, int C) { return (size_t)Nb * COLSUM_RS * C; }
int launch_colsum(int dtype, const void* x, void* out, float* scratch, int Nb, int HW, int C, float mul,
                  hipStream_t stream, int64_t ldo) {
  SMI_CHECK(C % 8 == 0 && scratch, "colsum: C %% 8 != 0 or no scratch");
  SMI_CHECK(ldo == 0 || ldo >= C, "colsum: output row stride %lld below C = %d", (long long)ldo, C);
  if (ldo == 0) ldo = C;
  dim3 grid(cdiv(C, 256), COLSUM_RS, Nb);
  const int fb = cdiv((int64_t)Nb * C, 256);
  if (dtype == DT_F16) {
    hipLaunchKernelGGL(colsum_partial_kernel<f16>, grid, dim3(256), 0, stream, (const f16*)x, scratch, HW, C);
    hipLaunchKernelGGL(colsum_final_kernel<f16>, dim3(fb), dim3(256), 0, stream, scratch, (f16*)out, Nb, C, ldo, mul);
  } else {
    hipLaunchKernelGGL(colsum_partial_kernel<bf16>, grid, dim3(256), 0, stream, (const bf16*)x, scratch, HW, C);
    hipLaunchKernelGGL(colsum_final_kernel<bf16>, dim3(fb), dim3(256), 0, stream, scratch, (bf16*)out, Nb, C, ldo, mul);
  }
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_silu_bwd_f32(int dtype, const void* x, float* g, int64_t n, hipStream_t stream) {
  const int grid = ew_grid(n);
  if (dtype == DT_F16) hipLaunchKernelGGL(silu_bwd_f32_kernel<f16>, dim3(grid), dim3(256), 0, stream, (const f16*)x, g, n);
  else hipLaunchKernelGGL(silu_bwd_f32_kernel<bf16>, dim3(grid), dim3(256), 0, stream, (const bf16*)x, g, n);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_vecmat_f32(int dtype, const float* dy, const void* W, float* dx, int M, int I, int64_t ldw, int J, int64_t lddx,
                      hipStream_t stream) {
  SMI_CHECK(dy && W && dx && M > 0 && M <= 65535 && I > 0 && J > 0 && ldw >= J && lddx >= J, "vecmat: bad arguments");
  dim3 grid(cdiv(J, 64), M);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(vecmat_f32_kernel<f16>, grid, dim3(1024), 0, stream, dy, (const f16*)W, dx, I, ldw, J, lddx);
  else
    hipLaunchKernelGGL(vecmat_f32_kernel<bf16>, grid, dim3(1024), 0, stream, dy, (const bf16*)W, dx, I, ldw, J, lddx);
  SMI_HIP(hipGetLastError());
  return 0;
}
int launch_f32_to_padded(int dtype, const float* src, int lds, int cols, void* dst, int cpad, int64_t M, float mul,
                         hipStream_t stream) {
  const int grid = ew_grid(M * cpad);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(f32_to_padded_kernel<f16>, dim3(grid), dim3(256), 0, stream, src, lds, cols, (f16*)dst, cpad, M, mul);
  else
    hipLaunchKernelGGL(f32_to_padded_kernel<bf16>, dim3(grid), dim3(256), 0, stream, src, lds, cols, (bf16*)dst, cpad, M, mul);
  SMI_HIP(hipGetLastError());
  return 0;
}

}  // namespace smi
