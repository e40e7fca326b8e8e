// LPIPS (AlexNet, v0.1) around the GEMMs: every convolution of the tower is the existing GEMM (bias epilogue) on an
// explicit patch matrix, and the kernels here build those matrices, pool, and reduce the taps to distances.
//
//   lpips_pack_filter  conv filter [Cout, Cin, k, k] -> [Cout, Kp], columns (ky, kx, ci), pad columns zero (creation)
//   lpips_stem         image (uint8 HWC or f32 CHW) -> scaled input -> patch matrix of conv1 (k 11, stride 4, pad 2)
//   lpips_im2col       NHWC map -> patch matrix for runtime k / stride / pad, max(0, .) applied on read
//   lpips_maxpool      3 x 3 / stride 2 max-pool (floor mode, no padding) of an NHWC map
//   lpips_relu         post-ReLU copy of a tap (the optional `feats` output)
//   lpips_head         per (pair, tap): channel norms, lin-weighted squared difference, sum over the map
//   lpips_head_finish  spatial mean per tap, the five taps added in layer order
//
// The GEMMs store the PRE-activation; ReLU is applied by whoever reads (im2col, head, relu copy).  The pool takes the max
// of pre-activations, which is the same thing: max(0, .) is monotone, so it commutes with the max over the window.
// All arithmetic is fp32; 16-bit storage T is written once per value.  Every thread moves 16 bytes per access.
#include <algorithm>

#include "kernels.h"

namespace smi {
namespace {

template <typename T>
__global__ __launch_bounds__(256) void lpips_pack_filter_kernel(const T* __restrict__ src, T* __restrict__ dst, int Cout,
                                                                int Cin, int k, int Kp) {
  const int64_t total = (int64_t)Cout * Kp;
  const int K = k * k * Cin;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int co = (int)(i / Kp), col = (int)(i - (int64_t)co * Kp);
    T v = from_f<T>(0.f);
    if (col < K) {
      const int tap = col / Cin, ci = col - tap * Cin;
      v = src[((int64_t)co * Cin + ci) * k * k + tap];
    }
    dst[i] = v;
  }
}

// one thread per 8 columns of one patch row.  Row r = (image, oy, ox) over 2n images: a-images, then b-images.
// Column (ky, kx, c) reads pixel (oy * 4 + ky - 2, ox * 4 + kx - 2): x = u / 127.5 - 1 (uint8 form), then the scaling layer
// (x - shift[c]) / scale[c]; outside the image the SCALED input is zero (the convolution's own padding).
constexpr int STEM_K = 11, STEM_S = 4, STEM_P = 2, STEM_COLS = 3 * STEM_K * STEM_K;
template <typename T>
__global__ __launch_bounds__(256) void lpips_stem_kernel(const uint8_t* __restrict__ u8a, const uint8_t* __restrict__ u8b,
                                                         const float* __restrict__ fa, const float* __restrict__ fb,
                                                         T* __restrict__ out, int n, int H, int W, int Ho, int Wo, int Kp,
                                                         int64_t items) {
  const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (item >= items) return;
  const int nv = Kp / 8;
  const int64_t row = item / nv;
  const int col0 = (int)(item - row * nv) * 8;
  const int img = (int)(row / ((int64_t)Ho * Wo));
  const int pos = (int)(row - (int64_t)img * Ho * Wo);
  const int oy = pos / Wo, ox = pos - oy * Wo;
  const bool second = img >= n;
  const int64_t i = second ? img - n : img;
  const uint8_t* u8 = second ? u8b : u8a;
  const float* f32 = second ? fb : fa;
  Pack8<T> o;
  o.u = u32x4{0u, 0u, 0u, 0u};
  int tap = col0 / 3, c = col0 - tap * 3;
  int ky = tap / STEM_K, kx = tap - ky * STEM_K;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int iy = oy * STEM_S + ky - STEM_P, ix = ox * STEM_S + kx - STEM_P;
    if (col0 + e < STEM_COLS && iy >= 0 && iy < H && ix >= 0 && ix < W) {
      const float x = u8 ? (float)u8[((i * H + iy) * W + ix) * 3 + c] / 127.5f - 1.f : f32[((i * 3 + c) * H + iy) * W + ix];
      const float shift = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f);
      const float scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
      o.e[e] = from_f<T>((x - shift) / scale);
    }
    if (++c == 3) {
      c = 0;
      if (++kx == STEM_K) {
        kx = 0;
        ++ky;
      }
    }
  }
  *reinterpret_cast<u32x4*>(out + row * Kp + col0) = o.u;
}

// one thread per 8 columns of one patch row: C % 8 == 0, so the 8 columns are 8 consecutive channels of ONE filter tap
template <typename T>
__global__ __launch_bounds__(256) void lpips_im2col_kernel(const T* __restrict__ in, T* __restrict__ out, int H, int W,
                                                           int C, int Ho, int Wo, int k, int stride, int pad, int Kp,
                                                           int64_t items) {
  const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (item >= items) return;
  const int nv = Kp / 8;
  const int64_t row = item / nv;
  const int col0 = (int)(item - row * nv) * 8;
  const int64_t img = row / ((int64_t)Ho * Wo);
  const int pos = (int)(row - img * Ho * Wo);
  const int oy = pos / Wo, ox = pos - oy * Wo;
  const int tap = col0 / C, ci = col0 - tap * C;
  const int ky = tap / k, kx = tap - ky * k;
  const int iy = oy * stride + ky - pad, ix = ox * stride + kx - pad;
  Pack8<T> v;
  v.u = u32x4{0u, 0u, 0u, 0u};
  if (tap < k * k && iy >= 0 && iy < H && ix >= 0 && ix < W) {
    v.u = *reinterpret_cast<const u32x4*>(in + ((img * H + iy) * W + ix) * C + ci);
#pragma unroll
    for (int e = 0; e < 8; ++e) v.e[e] = from_f<T>(fmaxf(to_f(v.e[e]), 0.f));
  }
  *reinterpret_cast<u32x4*>(out + row * Kp + col0) = v.u;
}

// one thread per 8 channels of one output pixel; every window lies inside the map (floor mode, no padding)
template <typename T>
__global__ __launch_bounds__(256) void lpips_maxpool_kernel(const T* __restrict__ in, T* __restrict__ out, int H, int W,
                                                            int C, int Ho, int Wo, int64_t items) {
  const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (item >= items) return;
  const int nv = C / 8;
  const int64_t pix = item / nv;
  const int c0 = (int)(item - pix * nv) * 8;
  const int64_t img = pix / ((int64_t)Ho * Wo);
  const int pos = (int)(pix - img * Ho * Wo);
  const int oy = pos / Wo, ox = pos - oy * Wo;
  float m[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      Pack8<T> v;
      v.u = *reinterpret_cast<const u32x4*>(in + ((img * H + oy * 2 + dy) * W + ox * 2 + dx) * C + c0);
#pragma unroll
      for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], to_f(v.e[e]));
    }
  Pack8<T> o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o.e[e] = from_f<T>(m[e]);
  *reinterpret_cast<u32x4*>(out + pix * C + c0) = o.u;
}

template <typename T>
__global__ __launch_bounds__(256) void lpips_relu_kernel(const T* __restrict__ in, T* __restrict__ out, int64_t nvec) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  Pack8<T> v;
  v.u = *reinterpret_cast<const u32x4*>(in + i * 8);
#pragma unroll
  for (int e = 0; e < 8; ++e) v.e[e] = from_f<T>(fmaxf(to_f(v.e[e]), 0.f));
  *reinterpret_cast<u32x4*>(out + i * 8) = v.u;
}

// Distance head.  A workgroup owns HEAD_POS consecutive map positions of one (pair, tap): 32 groups of 8 lanes, group g
// takes positions base + g, base + g + 32, ...  Per position the 8 lanes split the channels (vectors l, l + 8, ...), the
// three xor-shuffles leave every lane with the same sum, and the group adds its positions in ascending order; thread 0
// then adds the 32 group sums in order.  Nothing in that order knows the batch: a pair's partials depend on (H, W, C)
// alone.  a and b go through the same instructions, so swapping them negates d and leaves d * d -- and the sums -- as
// they were; equal inputs give d == 0 exactly.
__device__ __forceinline__ float group8_sum(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}
template <typename T>
__global__ __launch_bounds__(256) void lpips_head_kernel(LpipsHeadTaps taps, int n, float* __restrict__ partial) {
  __shared__ float gsum[32];
  int t = 0;
  while (t < 4 && (int)blockIdx.x >= taps.blk0[t + 1]) ++t;
  const int blk = (int)blockIdx.x - taps.blk0[t];
  const int pair = blockIdx.y;
  const int HW = taps.HW[t], C = taps.C[t];
  const T* y = reinterpret_cast<const T*>(taps.y[t]);
  const T* a = y + (int64_t)pair * HW * C;
  const T* b = y + (int64_t)(n + pair) * HW * C;
  const T* w = reinterpret_cast<const T*>(taps.w[t]);
  const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
  const int nv = C / 8;
  float acc = 0.f;
  for (int p = blk * LPIPS_HEAD_POS + g; p < min(HW, (blk + 1) * LPIPS_HEAD_POS); p += 32) {
    const T* pa = a + (int64_t)p * C;
    const T* pb = b + (int64_t)p * C;
    float aa = 0.f, bb = 0.f;
    for (int v = l; v < nv; v += 8) {
      Pack8<T> va, vb;
      va.u = *reinterpret_cast<const u32x4*>(pa + v * 8);
      vb.u = *reinterpret_cast<const u32x4*>(pb + v * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float x = fmaxf(to_f(va.e[e]), 0.f), z = fmaxf(to_f(vb.e[e]), 0.f);
        aa = __builtin_fmaf(x, x, aa);
        bb = __builtin_fmaf(z, z, bb);
      }
    }
    const float na = sqrtf(group8_sum(aa)) + 1e-10f, nb = sqrtf(group8_sum(bb)) + 1e-10f;
    float s = 0.f;
    for (int v = l; v < nv; v += 8) {
      Pack8<T> va, vb, vw;
      va.u = *reinterpret_cast<const u32x4*>(pa + v * 8);
      vb.u = *reinterpret_cast<const u32x4*>(pb + v * 8);
      vw.u = *reinterpret_cast<const u32x4*>(w + v * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = fmaxf(to_f(va.e[e]), 0.f) / na - fmaxf(to_f(vb.e[e]), 0.f) / nb;
        s = __builtin_fmaf(to_f(vw.e[e]), d * d, s);
      }
    }
    acc += group8_sum(s);
  }
  if (l == 0) gsum[g] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int k = 0; k < 32; ++k) tot += gsum[k];
    partial[(int64_t)pair * taps.blk0[5] + blockIdx.x] = tot;
  }
}

// one thread per pair: each tap's block partials in ascending order, / HW, then the five taps in layer order
__global__ __launch_bounds__(64) void lpips_head_finish_kernel(LpipsHeadTaps taps, int n, const float* __restrict__ partial,
                                                               float* __restrict__ dist, float* __restrict__ per_layer) {
  const int pair = blockIdx.x * 64 + threadIdx.x;
  if (pair >= n) return;
  const float* p = partial + (int64_t)pair * taps.blk0[5];
  float total = 0.f;
  for (int t = 0; t < 5; ++t) {
    float s = 0.f;
    for (int k = taps.blk0[t]; k < taps.blk0[t + 1]; ++k) s += p[k];
    const float v = s / (float)taps.HW[t];
    if (per_layer) per_layer[(int64_t)pair * 5 + t] = v;
    total += v;
  }
  dist[pair] = total;
}

bool grid_fits(int64_t items) { return (items + 255) / 256 < (1ll << 31); }

}  // namespace

int launch_lpips_pack_filter(int dtype, const void* src, void* dst, int Cout, int Cin, int k, int Kp, hipStream_t stream) {
  SMI_CHECK(src && dst && Cout > 0 && Cin > 0 && k > 0 && Kp >= k * k * Cin, "lpips_pack_filter: bad arguments");
  const int64_t total = (int64_t)Cout * Kp;
  const dim3 grid((unsigned)std::min<int64_t>((total + 255) / 256, 8192));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(lpips_pack_filter_kernel<f16>, grid, dim3(256), 0, stream, (const f16*)src, (f16*)dst, Cout, Cin, k, Kp);
  else
    hipLaunchKernelGGL(lpips_pack_filter_kernel<bf16>, grid, dim3(256), 0, stream, (const bf16*)src, (bf16*)dst, Cout, Cin, k, Kp);
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_lpips_stem(int dtype, const uint8_t* rgb8_a, const uint8_t* rgb8_b, const float* img_a, const float* img_b,
                      void* out, int n, int H, int W, int Kp, hipStream_t stream) {
  SMI_CHECK((rgb8_a && rgb8_b && !img_a && !img_b) || (!rgb8_a && !rgb8_b && img_a && img_b),
            "lpips_stem: exactly one input form (two uint8 or two f32 batches)");
  SMI_CHECK(n > 0 && H >= 31 && W >= 31, "lpips_stem: image %d x %d is smaller than 31 x 31", H, W);
  SMI_CHECK(Kp % 8 == 0 && Kp >= STEM_COLS, "lpips_stem: Kp=%d must be a multiple of 8 and >= %d", Kp, STEM_COLS);
  const int Ho = lpips_conv_out(H, STEM_K, STEM_S, STEM_P), Wo = lpips_conv_out(W, STEM_K, STEM_S, STEM_P);
  const int64_t items = (int64_t)2 * n * Ho * Wo * (Kp / 8);
  SMI_CHECK(grid_fits(items), "lpips_stem: grid too large");
  const dim3 grid((unsigned)((items + 255) / 256));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(lpips_stem_kernel<f16>, grid, dim3(256), 0, stream, rgb8_a, rgb8_b, img_a, img_b, (f16*)out, n, H, W, Ho, Wo, Kp, items);
  else
    hipLaunchKernelGGL(lpips_stem_kernel<bf16>, grid, dim3(256), 0, stream, rgb8_a, rgb8_b, img_a, img_b, (bf16*)out, n, H, W, Ho, Wo, Kp, items);
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_lpips_im2col(int dtype, const void* in, void* out, int Nb, int H, int W, int C, int k, int stride, int pad,
                        int Kp, hipStream_t stream) {
  SMI_CHECK(in && out && Nb > 0 && C > 0 && C % 8 == 0, "lpips_im2col: channels=%d must be a positive multiple of 8", C);
  SMI_CHECK(k > 0 && stride > 0 && pad >= 0 && Kp % 8 == 0 && Kp >= k * k * C, "lpips_im2col: bad geometry");
  const int Ho = lpips_conv_out(H, k, stride, pad), Wo = lpips_conv_out(W, k, stride, pad);
  SMI_CHECK(Ho > 0 && Wo > 0, "lpips_im2col: empty output map");
  const int64_t items = (int64_t)Nb * Ho * Wo * (Kp / 8);
  SMI_CHECK(grid_fits(items), "lpips_im2col: grid too large");
  const dim3 grid((unsigned)((items + 255) / 256));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(lpips_im2col_kernel<f16>, grid, dim3(256), 0, stream, (const f16*)in, (f16*)out, H, W, C, Ho, Wo, k, stride, pad, Kp, items);
  else
    hipLaunchKernelGGL(lpips_im2col_kernel<bf16>, grid, dim3(256), 0, stream, (const bf16*)in, (bf16*)out, H, W, C, Ho, Wo, k, stride, pad, Kp, items);
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_lpips_maxpool(int dtype, const void* in, void* out, int Nb, int H, int W, int C, hipStream_t stream) {
  SMI_CHECK(in && out && Nb > 0 && C > 0 && C % 8 == 0, "lpips_maxpool: channels=%d must be a positive multiple of 8", C);
  SMI_CHECK(H >= 3 && W >= 3, "lpips_maxpool: map %d x %d is smaller than the 3 x 3 window", H, W);
  const int Ho = lpips_pool_out(H), Wo = lpips_pool_out(W);
  const int64_t items = (int64_t)Nb * Ho * Wo * (C / 8);
  SMI_CHECK(grid_fits(items), "lpips_maxpool: grid too large");
  const dim3 grid((unsigned)((items + 255) / 256));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(lpips_maxpool_kernel<f16>, grid, dim3(256), 0, stream, (const f16*)in, (f16*)out, H, W, C, Ho, Wo, items);
  else
    hipLaunchKernelGGL(lpips_maxpool_kernel<bf16>, grid, dim3(256), 0, stream, (const bf16*)in, (bf16*)out, H, W, C, Ho, Wo, items);
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_lpips_relu(int dtype, const void* in, void* out, int64_t count, hipStream_t stream) {
  SMI_CHECK(in && out && count > 0 && count % 8 == 0, "lpips_relu: count must be a positive multiple of 8");
  SMI_CHECK(grid_fits(count / 8), "lpips_relu: grid too large");
  const dim3 grid((unsigned)((count / 8 + 255) / 256));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(lpips_relu_kernel<f16>, grid, dim3(256), 0, stream, (const f16*)in, (f16*)out, count / 8);
  else
    hipLaunchKernelGGL(lpips_relu_kernel<bf16>, grid, dim3(256), 0, stream, (const bf16*)in, (bf16*)out, count / 8);
  SMI_HIP(hipGetLastError());
  return 0;
}

void lpips_head_plan(LpipsHeadTaps& taps) {
  taps.blk0[0] = 0;
  for (int t = 0; t < 5; ++t) taps.blk0[t + 1] = taps.blk0[t] + cdiv(taps.HW[t], LPIPS_HEAD_POS);
}

int launch_lpips_head(int dtype, const LpipsHeadTaps& taps, int n, float* partial, float* dist, float* per_layer,
                      hipStream_t stream) {
  SMI_CHECK(partial && dist && n > 0 && n <= 65535, "lpips_head: %d pairs outside [1, 65535]", n);
  for (int t = 0; t < 5; ++t)
    SMI_CHECK(taps.y[t] && taps.w[t] && taps.HW[t] > 0 && taps.C[t] > 0 && taps.C[t] % 8 == 0,
              "lpips_head: tap %d: channels=%d must be a positive multiple of 8", t, taps.C[t]);
  const dim3 grid((unsigned)taps.blk0[5], (unsigned)n);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(lpips_head_kernel<f16>, grid, dim3(256), 0, stream, taps, n, partial);
  else
    hipLaunchKernelGGL(lpips_head_kernel<bf16>, grid, dim3(256), 0, stream, taps, n, partial);
  hipLaunchKernelGGL(lpips_head_finish_kernel, dim3((unsigned)cdiv(n, 64)), dim3(64), 0, stream, taps, n, partial, dist,
                     per_layer);
  SMI_HIP(hipGetLastError());
  return 0;
}

}  // namespace smi
