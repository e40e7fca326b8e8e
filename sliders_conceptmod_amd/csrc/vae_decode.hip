// Fused tail of the AutoencoderKL decoder: conv_norm_out (GroupNorm apply) + SiLU + conv_out (3x3, Cout <= 4) +
// NHWC -> NCHW + the eval scripts' uint8 post-processing, in ONE pass over the last up block's output.
//
// The unfused form reads x [n, H, W, C] (C = block_out_channels[0], 1024^2 x 128 per SD image), writes y = silu(GN(x))
// of the same size, re-reads it in a conv whose N (= Cout 3, padded to 4) fills 1/16 of every MFMA tile, and then moves
// the 3 channels through two layout kernels.  Here every workgroup stages its output tile's input window (+1 pixel halo)
// in LDS, 64 channels at a time, applying a * x + b and SiLU on the way in (the GroupNorm statistics come from the
// partial-sum launches, launch_groupnorm_stats), and runs the 3x3 conv as 16x16x32 MFMAs on it: rows = 16 output pixels
// (a 4 x 4 block), columns = the output channels (4 of 16 used), K = the 64 staged channels of one filter tap.
// The activated value is rounded to the storage type before the MFMA, as the unfused path stores it: only the fp32
// summation order differs between the two.  Out-of-image taps read 0 -- the conv pads the ACTIVATED tensor.
//
// Tile: 8 x 32 output pixels per workgroup (4 waves x 4 pixel blocks), LDS window 10 x 34 pixels x 64 channels (42.5 KB:
// three workgroups per CU); each input element is fetched from memory 1.33x (the halo), not 9x.
// LDS image: pixel slot `pos` holds 8 x 16 B (8 channels each); 16-B slot q is stored at q ^ (((pos >> 1) & 1) << 1) ^
// ((hy & 1) << 2) so that the ds_read_b128 of every 16-lane group touches 16 distinct bank quads (4 x 4 pixel rows: the
// pixel parity, bit 1 of pos and the row parity separate the lanes of a group).
#include "kernels.h"

namespace smi {
namespace {

constexpr int DT_TH = 8, DT_TW = 32;                 // output tile
constexpr int DT_HH = DT_TH + 2, DT_HW = DT_TW + 2;  // staged window
constexpr int DT_KC = 64;                            // channels staged per round
constexpr int DT_NPOS = DT_HH * DT_HW;               // 340 pixels
constexpr int DT_ITEMS = DT_NPOS * (DT_KC / 8);      // 16-B pieces per round (2720)
constexpr int DT_LD = (DT_ITEMS + 255) / 256;        // pieces per thread (11)
constexpr int DT_MAXC = 512;

__device__ __forceinline__ int dt_swz(int hy, int pos, int q) { return q ^ (((pos >> 1) & 1) << 1) ^ ((hy & 1) << 2); }

template <typename T>
__global__ __launch_bounds__(256) void vae_dec_tail_kernel(const T* __restrict__ x, const float* __restrict__ ab,
                                                           const T* __restrict__ w, const T* __restrict__ bias,
                                                           float* __restrict__ sample, uint8_t* __restrict__ rgb8,
                                                           int Nb, int H, int W, int C, int Cout, int tiles_x) {
  __shared__ __attribute__((aligned(16))) char win[DT_NPOS * DT_KC * 2];
  __shared__ float sa[DT_MAXC], sb[DT_MAXC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.y;
  const int ty0 = (blockIdx.x / tiles_x) * DT_TH, tx0 = (blockIdx.x % tiles_x) * DT_TW;
  for (int c = tid; c < C; c += 256) {
    sa[c] = ab[(int64_t)n * C + c];
    sb[c] = ab[((int64_t)Nb + n) * C + c];
  }
  // this wave's 4 pixel blocks: block row by = wave >> 1, block columns bx = (wave & 1) * 4 + i
  const int by = wave >> 1, bx0 = (wave & 1) * 4;
  const int p = lane & 15, q4 = lane >> 4;  // MFMA row (pixel p of the 4 x 4 block) and K quarter
  const int co = lane & 15;                 // MFMA column (output channel)
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const T* xn = x + (int64_t)n * H * W * C;

  for (int c0 = 0; c0 < C; c0 += DT_KC) {
    // the filter fragments of this round: B[k = 8 q4 + j][col co] = w[co][tap][c0 + 32 s + 8 q4 + j] (rows >= 4 zero)
    typename TT<T>::v8 bw[9][2];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        Pack8<T> v;
        v.u = u32x4{0u, 0u, 0u, 0u};
        if (co < 4) v.u = *reinterpret_cast<const u32x4*>(w + ((int64_t)co * 9 + t) * C + c0 + 32 * s + 8 * q4);
        bw[t][s] = v.v;
      }
    // the window: 16-B pieces of x (8 channels), all loads in flight before the activation
    Pack8<T> ld[DT_LD];
#pragma unroll
    for (int k = 0; k < DT_LD; ++k) {
      const int item = tid + 256 * k;
      const int pos = item >> 3, q = item & 7;
      const int hy = pos / DT_HW, hx = pos - hy * DT_HW;
      const int gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
      ld[k].u = u32x4{0u, 0u, 0u, 0u};
      if (item < DT_ITEMS && gy >= 0 && gy < H && gx >= 0 && gx < W)
        ld[k].u = *reinterpret_cast<const u32x4*>(xn + ((int64_t)gy * W + gx) * C + c0 + 8 * q);
    }
    __syncthreads();  // the previous round's reads of the window are done (and, first round, sa / sb are written)
#pragma unroll
    for (int k = 0; k < DT_LD; ++k) {
      const int item = tid + 256 * k;
      if (item >= DT_ITEMS) continue;
      const int pos = item >> 3, q = item & 7;
      const int hy = pos / DT_HW, hx = pos - hy * DT_HW;
      const int gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
      Pack8<T> o;
      o.u = u32x4{0u, 0u, 0u, 0u};
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const int cb = c0 + 8 * q;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.e[e] = from_f<T>(silu_f(to_f(ld[k].e[e]) * sa[cb + e] + sb[cb + e]));
      }
      *reinterpret_cast<u32x4*>(win + (pos * 8 + dt_swz(hy, pos, q)) * 16) = o.u;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int ky = t / 3, kx = t % 3;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int hy = 4 * by + (p >> 2) + ky;
        const int hx = 4 * (bx0 + i) + (p & 3) + kx;
        const int pos = hy * DT_HW + hx;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          Pack8<T> a;
          a.u = *reinterpret_cast<const u32x4*>(win + (pos * 8 + dt_swz(hy, pos, 4 * s + q4)) * 16);
          acc[i] = TT<T>::mfma16(a.v, bw[t][s], acc[i]);
        }
      }
    }
  }
  // D[row 4 q4 + r][col co]: pixel (dy = q4, dx = r) of the block, output channel co
  if (co >= Cout) return;
  const float bo = to_f(bias[co]);
  const int y = ty0 + 4 * by + q4;
  if (y >= H) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int x0 = tx0 + 4 * (bx0 + i);
    if (x0 >= W) continue;  // W % 4 == 0: the 4 pixels are all inside or all outside
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = acc[i][r] + bo;
    *reinterpret_cast<f32x4*>(sample + (((int64_t)n * Cout + co) * H + y) * W + x0) = v;
    if (rgb8) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float u = fminf(fmaxf(v[r] * 0.5f + 0.5f, 0.f), 1.f);
        rgb8[(((int64_t)n * H + y) * W + x0 + r) * Cout + co] = (uint8_t)rintf(u * 255.f);
      }
    }
  }
}

// the same post-processing from an NCHW sample (the unfused path, SMI_VAE_DEC_TAIL=0)
__global__ void rgb8_from_nchw_kernel(const float* __restrict__ s, uint8_t* __restrict__ out, int Nb, int C, int HW) {
  const int64_t total = (int64_t)Nb * C * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t hw = i % HW, nc = i / HW;
    const int64_t n = nc / C, c = nc - n * C;
    const float u = fminf(fmaxf(s[i] * 0.5f + 0.5f, 0.f), 1.f);
    out[(n * HW + hw) * C + c] = (uint8_t)rintf(u * 255.f);
  }
}

}  // namespace

int launch_vae_dec_tail(int dtype, const void* x, const float* ab, const void* w4, const void* bias, float* sample,
                        uint8_t* rgb8, int Nb, int H, int W, int C, int Cout, hipStream_t stream) {
  SMI_CHECK(C % DT_KC == 0 && C <= DT_MAXC, "vae decoder tail: C=%d must be a multiple of %d and <= %d", C, DT_KC,
            DT_MAXC);
  SMI_CHECK(Cout >= 1 && Cout <= 4, "vae decoder tail: Cout=%d outside [1, 4]", Cout);
  SMI_CHECK(W % 4 == 0 && H > 0 && Nb > 0, "vae decoder tail: W=%d must be a multiple of 4", W);
  SMI_CHECK(Nb <= 65535, "vae decoder tail: batch %d too large", Nb);
  const int tiles_x = (W + DT_TW - 1) / DT_TW, tiles_y = (H + DT_TH - 1) / DT_TH;
  const dim3 grid(tiles_x * tiles_y, Nb);
  if (dtype == DT_F16)
    hipLaunchKernelGGL(vae_dec_tail_kernel<f16>, grid, dim3(256), 0, stream, (const f16*)x, ab, (const f16*)w4,
                       (const f16*)bias, sample, rgb8, Nb, H, W, C, Cout, tiles_x);
  else
    hipLaunchKernelGGL(vae_dec_tail_kernel<bf16>, grid, dim3(256), 0, stream, (const bf16*)x, ab, (const bf16*)w4,
                       (const bf16*)bias, sample, rgb8, Nb, H, W, C, Cout, tiles_x);
  SMI_HIP(hipGetLastError());
  return 0;
}

int launch_rgb8_from_nchw(const float* sample, uint8_t* rgb8, int Nb, int C, int HW, hipStream_t stream) {
  const int64_t total = (int64_t)Nb * C * HW;
  int64_t g = (total + 255) / 256;
  const int grid = (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
  hipLaunchKernelGGL(rgb8_from_nchw_kernel, dim3(grid), dim3(256), 0, stream, sample, rgb8, Nb, C, HW);
  SMI_HIP(hipGetLastError());
  return 0;
}

}  // namespace smi
