// Front end and head of the CLIP image tower (transformers CLIPVisionModel[WithProjection] / CLIPModel); the encoder
// layers between them are the text tower's (engine.hip), run without the causal mask.
//
//   clip_patchify   image -> patch matrix [n G^2, Kp] in the patch filter's own column order (c, py, px), so that the
//                   stride-P convolution of CLIPVisionEmbeddings is the existing GEMM against the [hidden, Kp] filter
//   vit_embed_ln    (class_embedding | patch rows) + position_embedding, then pre_layrnorm, one wave per token row
//   clip_logits     exp(logit_scale) <i, t> / (|i| |t|) for every (image, text) pair, one wave per pair
//
// All arithmetic is fp32; 16-bit storage T is written once per value.
#include "kernels.h"

namespace smi {
namespace {

// One workgroup per strip of G patches: the P image rows [gy P, gy P + P) of image i.
// uint8 HWC: the strip is ONE contiguous run of P * S * 3 bytes, read with VEC-byte loads (16 where the strip's start and
// length allow it), normalised in fp32 and scattered into LDS as T [3][P][S]; f32 CHW: three contiguous runs of P * S
// floats, one per channel, stored to the same LDS image.  The write side then reads LDS in output order: a thread builds
// 8 consecutive columns of one patch row and stores them with one 16-byte store, consecutive threads consecutive
// 16-byte pieces of the output row.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void clip_patchify_kernel(const uint8_t* __restrict__ rgb8,
                                                            const float* __restrict__ chw, T* __restrict__ out, int S,
                                                            int P, int Kp, float m0, float m1, float m2, float r0,
                                                            float r1, float r2) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  T* img = reinterpret_cast<T*>(lds_raw);  // [3][P][S]
  const int G = S / P;
  const int i = blockIdx.x / G, gy = blockIdx.x % G;
  const int tid = threadIdx.x;
  const int plane = P * S;
  if (rgb8) {
    const int row_bytes = 3 * S, strip = P * row_bytes;
    const uint8_t* src = rgb8 + ((int64_t)i * S + (int64_t)gy * P) * row_bytes;
    for (int b0 = tid * VEC; b0 < strip; b0 += 256 * VEC) {  // strip % VEC == 0 (launcher)
      __attribute__((aligned(16))) uint8_t v[VEC];
      if (VEC == 16)
        *reinterpret_cast<u32x4*>(v) = *reinterpret_cast<const u32x4*>(src + b0);
      else if (VEC == 4)
        *reinterpret_cast<uint32_t*>(v) = *reinterpret_cast<const uint32_t*>(src + b0);
      else
        v[0] = src[b0];
      int py = b0 / row_bytes;
      int rem = b0 - py * row_bytes;
      int x = rem / 3, c = rem - 3 * x;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2);
        const float rstd = c == 0 ? r0 : (c == 1 ? r1 : r2);
        img[c * plane + py * S + x] = from_f<T>(((float)v[e] * (1.f / 255.f) - mean) * rstd);
        if (++c == 3) {
          c = 0;
          if (++x == S) {
            x = 0;
            ++py;
          }
        }
      }
    }
  } else {
    for (int c = 0; c < 3; ++c) {
      const float* src = chw + (((int64_t)i * 3 + c) * S + (int64_t)gy * P) * S;
      for (int k = tid; k < plane; k += 256) img[c * plane + k] = from_f<T>(src[k]);
    }
  }
  __syncthreads();
  const int K = 3 * P * P, PP = P * P, nv = Kp / 8;
  T* dst = out + ((int64_t)i * G + gy) * G * Kp;
  for (int item = tid; item < G * nv; item += 256) {
    const int gx = item / nv, col0 = (item - gx * nv) * 8;
    Pack8<T> o;
    o.u = u32x4{0u, 0u, 0u, 0u};
    int c = col0 / PP;
    int r = col0 - c * PP;
    int py = r / P, px = r - py * P;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (col0 + e < K) o.e[e] = img[c * plane + py * S + gx * P + px];
      if (++px == P) {
        px = 0;
        if (++py == P) {
          py = 0;
          ++c;
        }
      }
    }
    *reinterpret_cast<u32x4*>(dst + (int64_t)gx * Kp + col0) = o.u;
  }
}

constexpr int VE_MAXV = 4;  // hidden <= 2048: 4 vectors of 8 per lane

// one wave per token row: x = (t == 0 ? class_embedding : patch_out[i, t - 1]) + position_embedding[t] in fp32 (never
// rounded), LayerNorm statistics over it in fp32 (two passes over the registers), y = T((x - mean) rstd gamma + beta)
template <typename T>
__global__ __launch_bounds__(256) void vit_embed_ln_kernel(const T* __restrict__ patch_out, const T* __restrict__ cls,
                                                           const T* __restrict__ pos, const T* __restrict__ gamma,
                                                           const T* __restrict__ beta, T* __restrict__ out,
                                                           int64_t rows, int tokens, int d, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t i = row / tokens;
  const int t = (int)(row - i * tokens);
  const T* src = t == 0 ? cls : patch_out + (i * (tokens - 1) + (t - 1)) * d;
  const T* pr = pos + (int64_t)t * d;
  const int nvec = d / 8;
  float x[VE_MAXV][8];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < VE_MAXV; ++j) {
    const int v = lane + 64 * j;
    Pack8<T> a, b;
    a.u = b.u = u32x4{0u, 0u, 0u, 0u};
    if (v < nvec) {
      a.u = *reinterpret_cast<const u32x4*>(src + v * 8);
      b.u = *reinterpret_cast<const u32x4*>(pr + v * 8);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      x[j][e] = to_f(a.e[e]) + to_f(b.e[e]);
      s += x[j][e];
    }
  }
  const float mean = wave_sum(s) / (float)d;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < VE_MAXV; ++j)
    if (lane + 64 * j < nvec) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float dlt = x[j][e] - mean;
        sq += dlt * dlt;
      }
    }
  const float rstd = rsqrtf(wave_sum(sq) / (float)d + eps);
#pragma unroll
  for (int j = 0; j < VE_MAXV; ++j) {
    const int v = lane + 64 * j;
    if (v < nvec) {
      Pack8<T> g, b, o;
      g.u = *reinterpret_cast<const u32x4*>(gamma + v * 8);
      b.u = *reinterpret_cast<const u32x4*>(beta + v * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) o.e[e] = from_f<T>((x[j][e] - mean) * rstd * to_f(g.e[e]) + to_f(b.e[e]));
      *reinterpret_cast<u32x4*>(out + row * d + v * 8) = o.u;
    }
  }
}

// one wave per (image i, text j): three fp32 sums over dim (|i|^2, |t|^2, <i, t>), each a wave reduction
template <typename T>
__global__ __launch_bounds__(256) void clip_logits_kernel(const T* __restrict__ img, const T* __restrict__ txt,
                                                          float* __restrict__ out, int ni, int nt, int dim,
                                                          float scale) {
  const int lane = threadIdx.x & 63;
  const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= (int64_t)ni * nt) return;
  const int i = (int)(pair / nt), j = (int)(pair - (int64_t)i * nt);
  const T* a = img + (int64_t)i * dim;
  const T* b = txt + (int64_t)j * dim;
  float aa = 0.f, bb = 0.f, ab = 0.f;
  for (int v = lane; v < dim / 8; v += 64) {
    Pack8<T> pa, pb;
    pa.u = *reinterpret_cast<const u32x4*>(a + v * 8);
    pb.u = *reinterpret_cast<const u32x4*>(b + v * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float fa = to_f(pa.e[e]), fb = to_f(pb.e[e]);
      aa = __builtin_fmaf(fa, fa, aa);
      bb = __builtin_fmaf(fb, fb, bb);
      ab = __builtin_fmaf(fa, fb, ab);
    }
  }
  aa = wave_sum(aa);
  bb = wave_sum(bb);
  ab = wave_sum(ab);
  if (lane == 0) out[pair] = scale * ab / (sqrtf(aa) * sqrtf(bb));
}

}  // namespace

size_t clip_patchify_lds_bytes(int S, int P) { return (size_t)3 * P * S * 2; }

int launch_clip_patchify(int dtype, const uint8_t* rgb8, const float* pixel_values, void* out, int n, int S, int P,
                         int Kp, const float mean[3], const float stdv[3], hipStream_t stream) {
  SMI_CHECK((rgb8 != nullptr) != (pixel_values != nullptr), "clip_patchify: exactly one of rgb8 / pixel_values");
  SMI_CHECK(n > 0 && P > 0 && S > 0 && S % P == 0, "clip_patchify: image size %d is no multiple of the patch size %d", S, P);
  SMI_CHECK(Kp % 64 == 0 && Kp >= 3 * P * P, "clip_patchify: Kp=%d must be 3 P^2 rounded up to a multiple of 64", Kp);
  const size_t lds = clip_patchify_lds_bytes(S, P);
  SMI_CHECK(lds <= 65536, "clip_patchify: a strip of %d x %d pixels needs %zu bytes of LDS (limit 65536)", P, S, lds);
  const int G = S / P;
  SMI_CHECK((int64_t)n * G < (1ll << 31), "clip_patchify: grid too large");
  const int64_t strip = (int64_t)3 * P * S;
  int vec = 1;
  if (rgb8) {
    const int64_t image = (int64_t)3 * S * S;
    const uintptr_t base = (uintptr_t)rgb8;
    if (strip % 16 == 0 && image % 16 == 0 && base % 16 == 0) vec = 16;
    else if (strip % 4 == 0 && image % 4 == 0 && base % 4 == 0) vec = 4;
  }
  const float m0 = mean[0], m1 = mean[1], m2 = mean[2];
  const float r0 = 1.f / stdv[0], r1 = 1.f / stdv[1], r2 = 1.f / stdv[2];
  const dim3 grid(n * G);
#define L(TT_, V_)                                                                                               \
  hipLaunchKernelGGL((clip_patchify_kernel<TT_, V_>), grid, dim3(256), lds, stream, rgb8, pixel_values, (TT_*)out, S, P, \
                     Kp, m0, m1, m2, r0, r1, r2)
  if (dtype == DT_F16) {
    if (vec == 16) L(f16, 16); else if (vec == 4) L(f16, 4); else L(f16, 1);
  } else {
    if (vec == 16) L(bf16, 16); else if (vec == 4) L(bf16, 4); else L(bf16, 1);
  }
#undef L
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_vit_embed_ln(int dtype, const void* patch_out, const void* cls, const void* pos, const void* gamma,
                        const void* beta, void* out, int n, int tokens, int d, float eps, hipStream_t stream) {
  SMI_CHECK(d % 8 == 0 && d <= 8 * 64 * VE_MAXV, "vit_embed_ln: hidden=%d unsupported (multiple of 8, <= 2048)", d);
  SMI_CHECK(n > 0 && tokens >= 2, "vit_embed_ln: empty shape");
  const int64_t rows = (int64_t)n * tokens;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (dtype == DT_F16)
    hipLaunchKernelGGL(vit_embed_ln_kernel<f16>, grid, dim3(256), 0, stream, (const f16*)patch_out, (const f16*)cls,
                       (const f16*)pos, (const f16*)gamma, (const f16*)beta, (f16*)out, rows, tokens, d, eps);
  else
    hipLaunchKernelGGL(vit_embed_ln_kernel<bf16>, grid, dim3(256), 0, stream, (const bf16*)patch_out, (const bf16*)cls,
                       (const bf16*)pos, (const bf16*)gamma, (const bf16*)beta, (bf16*)out, rows, tokens, d, eps);
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_clip_logits(int dtype, const void* image_embeds, int ni, const void* text_embeds, int nt, int dim,
                       float logit_scale, float* logits_per_image, hipStream_t stream) {
  SMI_CHECK(image_embeds && text_embeds && logits_per_image, "clip_logits: NULL argument");
  SMI_CHECK(dtype == DT_F16 || dtype == DT_BF16, "clip_logits: dtype must be f16 (0) or bf16 (1)");
  SMI_CHECK(ni > 0 && nt > 0 && dim > 0 && dim % 8 == 0, "clip_logits: dim=%d must be a positive multiple of 8", dim);
  const int64_t pairs = (int64_t)ni * nt;
  SMI_CHECK((pairs + 3) / 4 < (1ll << 31), "clip_logits: grid too large");
  const dim3 grid((unsigned)((pairs + 3) / 4));
  const float scale = expf(logit_scale);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(clip_logits_kernel<f16>, grid, dim3(256), 0, stream, (const f16*)image_embeds,
                       (const f16*)text_embeds, logits_per_image, ni, nt, dim, scale);
  else
    hipLaunchKernelGGL(clip_logits_kernel<bf16>, grid, dim3(256), 0, stream, (const bf16*)image_embeds,
                       (const bf16*)text_embeds, logits_per_image, ni, nt, dim, scale);
  SMI_HIP(hipGetLastError());
  return 0;
}

}  // namespace smi
