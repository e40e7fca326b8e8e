// Internal launcher API of the HIP kernels (host side).  All launchers enqueue on `stream`, never synchronise,
// return 0 on success or a negative code after smi::set_error().  Activations are token-major ("NHWC"):
// an image tensor is [N, H*W, C] with C contiguous.
#pragma once
#include <vector>

#include "smi_common.h"

namespace smi {

// ---------------------------------------------------------------------------------------------------------------
// C[M,N] = A[M,K] * W[N,K]^T  (+ epilogue), W rows K-contiguous (torch nn.Linear layout).
// With conv != 0, A is gathered on the fly from an NHWC image (implicit GEMM, K = 9*Cin ordered (kh,kw,ci); 4*Cin on the
// 2x2 tap grid of an up-sampler's phase conv).
// Epilogue (all fp32, one rounding at the store):  + bias[n] + rowvec[m / rows_per_vec][n]
//     + lora_scale * sum_q xa[m][q] * up[n][q] + res[m][n]
// ---------------------------------------------------------------------------------------------------------------
struct GemmParams {
  int dtype = DT_F16;
  const void* A = nullptr;
  int64_t lda = 0;
  const void* W = nullptr;
  void* C = nullptr;
  int64_t ldc = 0;
  int out_f32 = 0;
  int M = 0, N = 0, K = 0;
  const void* bias = nullptr;    // T [N]
  const void* res = nullptr;     // T [M, ldr]
  int64_t ldr = 0;
  const void* rowvec = nullptr;  // T [M / rows_per_vec, N]
  int rows_per_vec = 1;
  int64_t ld_rowvec = 0;         // row stride of rowvec in elements (0 = N): a column block of a wider matrix
  // LoRA rank-r delta: + lora_scale * sum_q xa[m*ld_xa + seg*r + q] * up[n*up_sn + q*up_sq], seg = n / lora_seg.
  // Forward: xa = x*A^T, up = lora_up.weight [N, r] (up_sn = r, up_sq = 1); with fused q|k|v projections the three
  // [C, r] up matrices are adjacent in the flat buffer and lora_seg = C selects each column block's own xa.
  // Backward (dX): xa = dY*up, "up" = lora_down.weight [r, K] read transposed (up_sn = 1, up_sq = K).
  const float* lora_xa = nullptr;
  int64_t ld_xa = 0;
  const float* lora_up = nullptr;
  int64_t up_sn = 0, up_sq = 1;
  int lora_r = 0;
  int lora_seg = 0;
  float lora_scale = 0.f;
  int lora_row0 = 0;  // rows m < lora_row0 get no delta (frozen samples of a batched pass); xa row = m - lora_row0
  // fused GEGLU (diffusers GEGLU: proj(x).chunk(2) -> hidden * gelu(gate)), dense v2 kernel only: N = 2 * N_half,
  // every 128-column tile holds 64 hidden + their 64 gate columns; geglu_out [M, N/2] receives hidden * gelu(gate)
  // computed from the 16-bit-rounded projection (bit-identical to projection + separate GEGLU kernel); the projection
  // itself is stored to C only for rows m >= geglu_row0 (the rows whose backward needs it).  bias only.
  void* geglu_out = nullptr;
  int geglu_row0 = 0;
  // implicit-GEMM 3x3 convolution (pad 1)
  int conv = 0;
  int Nb = 0, Hin = 0, Win = 0, Cin = 0, Hout = 0, Wout = 0;
  int stride = 1;      // forward: in = out*stride + k - pad
  int pad = 1;         // 1 everywhere in the UNet; 0 for the VAE encoder's (0,1,0,1)-padded stride-2 downsampler
  int upsample = 0;    // nearest-2x upsample of the input folded into the gather
  int transposed = 0;  // gradient of a strided conv: out = (in + 1 - k) / stride
  // split-K (internal to launch_gemm, gemm2 kernels only): the workgroups of slice s accumulate K-tiles
  // [s nk / ksplit, (s + 1) nk / ksplit) and store fp32 partials to C + s * M * ldc (out_f32 form, no epilogue)
  int ksplit = 0;
  // conv tap grid: tap_w x tap_w taps (3, or 2 for a phase conv of an up-sampler), K = tap_w^2 * Cin ordered (ky, kx, ci);
  // tap (0, 0) of output pixel (oy, ox) reads input pixel (oy * stride + tap_oy, ox * stride + tap_ox): -pad for the 3x3 layers
  int tap_w = 3, tap_oy = -1, tap_ox = -1;

  // epilogue setters, chained onto one of the constructors below
  GemmParams& f32_out() { out_f32 = 1; return *this; }
  GemmParams& with_bias(const void* b) { bias = b; return *this; }
  GemmParams& with_res(const void* r, int64_t ld) { res = r; ldr = ld; return *this; }
  GemmParams& with_rowvec(const void* v, int rows_per, int64_t ld) {
    rowvec = v;
    rows_per_vec = rows_per;
    ld_rowvec = ld;
    return *this;
  }
  // forward delta: xa [M - row0, ld] fp32, up [N, r]; seg > 0: fused projections, column block n / seg reads its own r of xa
  GemmParams& with_lora(const float* xa, int64_t ld, const float* up, int r, int seg, float scale, int row0) {
    lora_xa = xa;
    ld_xa = ld;
    lora_up = up;
    up_sn = r;
    up_sq = 1;
    lora_r = xa ? r : 0;
    lora_seg = seg;
    lora_scale = scale;
    lora_row0 = row0;
    return *this;
  }
  // dX-form delta: dxa [M, ld] fp32, down [r_tot, N] read transposed
  GemmParams& with_lora_dx(const float* dxa, int64_t ld, const float* down, int r_tot, float scale) {
    lora_xa = dxa;
    ld_xa = ld;
    lora_up = down;
    up_sn = 1;
    up_sq = N;
    lora_r = r_tot;
    lora_seg = 0;
    lora_scale = scale;
    return *this;
  }
  GemmParams& with_geglu(void* out, int row0) { geglu_out = out; geglu_row0 = row0; return *this; }
};
// ---- constructors: every launch site (the engine's graph code and the smi_op_* test wrappers alike) states what it is
// through one of these and the setters above; nobody fills the struct field by field
inline GemmParams gemm_nt(int dtype, const void* A, int64_t lda, const void* W, void* C, int64_t ldc, int M, int N,
                          int K) {
  GemmParams p;
  p.dtype = dtype;
  p.A = A;
  p.lda = lda;
  p.W = W;
  p.C = C;
  p.ldc = ldc;
  p.M = M;
  p.N = N;
  p.K = K;
  return p;
}
// 3x3 implicit-GEMM conv with explicit geometry: in [Nb, Hin, Win, Cin], w [Cout][9 * Cin], out [Nb, Hout, Wout, Cout]
inline GemmParams conv3x3_geom(int dtype, const void* in, const void* w, void* out, int Nb, int Hin, int Win, int Cin,
                               int Cout, int Hout, int Wout, int stride, int pad, int upsample, int transposed) {
  GemmParams p = gemm_nt(dtype, in, 0, w, out, Cout, Nb * Hout * Wout, Cout, 9 * Cin);
  p.conv = 1;
  p.Nb = Nb;
  p.Hin = Hin;
  p.Win = Win;
  p.Cin = Cin;
  p.Hout = Hout;
  p.Wout = Wout;
  p.stride = stride;
  p.pad = pad;
  p.tap_oy = p.tap_ox = -pad;
  p.upsample = upsample;
  p.transposed = transposed;
  return p;
}
// (ky, kx) of filter tap `tap` on the launch's tap grid (tap_w is 2 or 3)
__host__ __device__ inline void conv_tap_yx(const GemmParams& p, int tap, int& ky, int& kx) {
  ky = p.tap_w == 2 ? tap >> 1 : tap / 3;
  kx = tap - ky * p.tap_w;
}
// forward conv of a layer: mode 0 stride 1, 1 stride 2, 2 nearest-2x upsample then stride 1
inline int conv3x3_out(int in, int mode) { return mode == 1 ? (in + 1) / 2 : (mode == 2 ? in * 2 : in); }
inline GemmParams conv3x3_fwd(int dtype, const void* in, const void* w, void* out, int Nb, int Hin, int Win, int Cin,
                              int Cout, int mode = 0, int pad = 1) {
  return conv3x3_geom(dtype, in, w, out, Nb, Hin, Win, Cin, Cout, conv3x3_out(Hin, mode), conv3x3_out(Win, mode),
                      mode == 1 ? 2 : 1, pad, mode == 2 ? 1 : 0, 0);
}
// Phase 2 a + b (a, b in {0, 1}) of a mode-2 layer: the output pixels (2 i + a, 2 j + b) of nearest-2x + 3x3 / pad 1 are a
// same-size 2x2 conv over the low-res input with tap origin (a - 1, b - 1) and summed filters.  wph: the layer's phase pack
// [4][Cout][4 * Cin] (16-bit), out: the phase-major result [4][Nb, Hin, Win, Cout] (16-bit) -- this launch fills plane `phase`
inline GemmParams conv2x2_phase(int dtype, const void* in, const void* wph, void* out, int Nb, int Hin, int Win, int Cin,
                                int Cout, int phase) {
  const int64_t M = (int64_t)Nb * Hin * Win;
  GemmParams p = conv3x3_geom(dtype, in, (const char*)wph + (int64_t)phase * Cout * 4 * Cin * 2,
                              (char*)out + (int64_t)phase * M * Cout * 2, Nb, Hin, Win, Cin, Cout, Hin, Win, 1, 1, 0, 0);
  p.K = 4 * Cin;
  p.tap_w = 2;
  p.tap_oy = (phase >> 1) - 1;
  p.tap_ox = (phase & 1) - 1;
  return p;
}
// gradient conv of that layer (Hin, Win, Cin, Cout are the FORWARD's): dy [Nb, Hout, Wout, Cout] against the gradient
// pack wg [Cin][9 * Cout].  Mode 0: same size.  Mode 1: transposed stride 2, dx on the input grid.  Mode 2: dx on the 2x
// (output) grid -- the caller sum-pools it 2x2 onto the input grid afterwards.
inline GemmParams conv3x3_grad(int dtype, const void* dy, const void* wg, void* dx, int Nb, int Hin, int Win, int Cin,
                               int Cout, int mode = 0) {
  const int Hy = conv3x3_out(Hin, mode), Wy = conv3x3_out(Win, mode);
  const int Hx = mode == 2 ? Hy : Hin, Wx = mode == 2 ? Wy : Win;
  return conv3x3_geom(dtype, dy, wg, dx, Nb, Hy, Wy, Cout, Cin, Hx, Wx, mode == 1 ? 2 : 1, 1, 0, mode == 1);
}
int launch_gemm(const GemmParams& p, hipStream_t stream);
// The kernels launch_gemm selects among (gemm.hip).  The gemm2 tiles are gemm_glds_kernel<WM, NL, DEEP> (gemm2.hip):
// BM x BN with 4 or 8 waves.  All of them give the same bits.
enum class GemmTile {
  Auto,          // not a kernel: the heuristic's choice
  T128x128,      // gemm2 (2, 0), 4 waves
  T128x128w8,    // gemm2 (2, 2), 8 waves
  T256x128,      // gemm2 (4, 0)
  T64x128,       // gemm2 (1, 0), 2 waves, dense only
  T64x128w4,     // gemm2 (1, 2), 4 waves
  T128x160,      // gemm2 (2, 1), 4 waves
  T64x160,       // gemm2 (1, 3)
  T128x160w8,    // gemm2 (2, 3), 8 waves
  T128x160Deep,  // gemm2 (2, 3, deep): the eight-wave tile with the four-stage prefetch loop
  Gemm3,         // 256 x 256, 8-phase schedule (gemm3.hip)
  Gemm4,         // 256 x 320, persistent (gemm4.hip)
  V1,            // register-staged kernel: the fallback for operands gemm2 cannot take
};
int launch_gemm2(const GemmParams& p, GemmTile tile, hipStream_t stream);  // the gemm2 tiles only
// what each generation can take, and its launcher (launch_gemm and the tile tuner choose among them; gemm.hip)
bool gemm2_supported(const GemmParams& p);        // 16-byte alignment / multiple-of-8 layout of the LDS-DMA kernels
bool gemm2_geglu_supported(const GemmParams& p);  // ... with the fused GEGLU epilogue
bool gemm3_supported(const GemmParams& p);
bool gemm4_supported(const GemmParams& p);
int launch_gemm3(const GemmParams& p, hipStream_t stream);
int launch_gemm4(const GemmParams& p, hipStream_t stream);
int launch_v1(const GemmParams& p, hipStream_t stream);  // register-staged kernel: operands gemm2 cannot take, SMI_GEMM=v1
// Test entry (smi_op_gemm_epilogue, smi_op_conv3x3_ex): launch p on the tile with tuner code `tile_code` (0: launch_gemm's own choice) where
// that tile can take it, else on what fit_tile puts in its place; ksplit > 1: split-K in that many slices with the tile as
// the slice kernel.  *ran_code receives the code of the tile that actually ran (0 for launch_gemm's own choice).
int launch_gemm_on_tile(const GemmParams& p, int tile_code, int ksplit, int* ran_code, hipStream_t stream);
// Scratch for split-K partial sums (fp32 slabs), set by whoever owns memory (the engine, per call; tests through
// smi_op_gemm_scratch) for the calling host thread; without it launch_gemm never splits.  Launches that use it are ordered
// on their stream, so one buffer serves every launch of a pass.
void set_gemm_scratch(void* ws, size_t bytes);
bool gemm_geglu_supported(const GemmParams& p);  // can launch_gemm take p.geglu_out?

// direct 3x3 conv for tiny channel counts (conv_in: Cin=4; conv_out: Cout=4 and their gradients)
// in [Nb,H,W,Cin] T ; w f32-free: T [Cout][9*Cin] ; out [Nb,H,W,Cout] (T or f32), stride 1 pad 1
int launch_conv3x3_small(int dtype, const void* in, const void* w, const void* bias, void* out, int out_f32, int Nb,
                         int H, int W, int Cin, int Cout, hipStream_t stream);

// ---------------------------------------------------------------------------------------------------------------
// attention: Q [B, Nq, ldq] (head h at column h*D), K/V [B, Nk, ldk/ldv], O [B, Nq, ldo]; lse f32 [B, H, Nq]
// ---------------------------------------------------------------------------------------------------------------
struct AttnParams {
  int dtype = DT_F16;
  const void *Q = nullptr, *K = nullptr, *V = nullptr;
  void* O = nullptr;
  float* lse = nullptr;
  int64_t ldq = 0, ldk = 0, ldv = 0, ldo = 0;
  int B = 0, H = 0, Nq = 0, Nk = 0, D = 0;
  float scale = 1.f;
  // key j is visible to query i iff j <= i (CLIP text encoder).  The forward kernels of attention.hip know the mask; the
  // backward of a causal pass is launch_attn_causal_bwd (attention_causal.hip), to which launch_attn_bwd routes
  int causal = 0;
  // backward
  const void* dO = nullptr;
  int64_t lddo = 0;
  float* delta = nullptr;  // f32 [B, H, Nq] workspace
  void *dQ = nullptr, *dK = nullptr, *dV = nullptr;
  int64_t lddq = 0, lddk = 0, lddv = 0;
  // additive relative-position bias f32 [H, bias_ld] (T5; launch_t5_bias_table), entry k - q + Nk - 1 of row h added to
  // s[q, k] = q.k * scale before the softmax.  Self-attention, head_dim 64, Nk <= ATTN_BIAS_MAX_L; always the tiled forward.
  // The backward (lse from the biased forward) recomputes the probabilities with it in the tiled dQ and dK / dV kernels or
  // the fused launch, never the single-pass ones; the table is frozen, no gradient to it is formed
  const float* bias = nullptr;
  int64_t bias_ld = 0;
};
// 2 L - 1 floats of dynamic LDS next to the forward's 42 KB of K / V stages, or the backward's 43.5 KB of Q / dO tiles
constexpr int ATTN_BIAS_MAX_L = 2048;
int launch_attn_fwd(const AttnParams& p, hipStream_t stream);
int launch_attn_bwd(const AttnParams& p, hipStream_t stream);
// Kernel selection of the two launchers for the parity tests: xs = the single-pass kernels for Nk <= 96, fused = the
// one-launch backward; -1 = as the environment says (SMI_ATTN_XS / SMI_ATTN_BWD_FUSED, the default), 0 = off, 1 = on.
// Process-wide, host side; the shape rules of the dispatcher still apply (1 does not force a kernel a shape cannot take).
void set_attn_select(int xs, int fused);
// What the last launch_attn_fwd / launch_attn_bwd of the calling thread launched (recorded on the host, like the
// ran_code of launch_gemm_on_tile): n == 0 after a refused call or the causal backward.
enum {
  ATTN_RAN_FWD = 1,        // attn_fwd_kernel
  ATTN_RAN_XS_FWD = 2,     // attn_xs_fwd_kernel
  ATTN_RAN_BWD_FUSED = 3,  // attn_bwd_fused_kernel
  ATTN_RAN_DQ = 4,         // attn_bwd_dq_kernel
  ATTN_RAN_XS_DQ = 5,      // attn_xs_bwd_dq_kernel
  ATTN_RAN_DKV = 6,        // attn_bwd_dkv_kernel<WHICH = 3>
  ATTN_RAN_DK_DV = 7,      // attn_bwd_dkv_kernel<1> then <2>
  ATTN_RAN_DELTA = 8,      // attn_delta_kernel
};
struct AttnRan {
  int dp = 0;     // tile depth DP
  int form = 0;   // 1 = full-depth compile-time k-steps, 2 = the alternative (40 in 64, 80 in 96), 0 = run-time
  int n = 0;      // launches, in order
  int family[4] = {0, 0, 0, 0};
  int chain = 0;  // single-pass kernels: query blocks per workgroup (nqb / gridDim.x), else 0
};
AttnRan attn_last_ran();
// causal self-attention backward, one workgroup per (sample, head): Nq == Nk <= 128, head_dim 64, dQ, dK and dV all wanted;
// every other shape is refused with an error that names the limit.  p.delta is not used (delta stays in LDS)
int launch_attn_causal_bwd(const AttnParams& p, hipStream_t stream);

// ---------------------------------------------------------------------------------------------------------------
// normalisation
// ---------------------------------------------------------------------------------------------------------------
// GroupNorm over [Nb, HW, C]; writes per-(n,c) affine a,b (f32 [Nb,C] each: y = x*a + b) into `ab` ([2,Nb,C]) and
// y = (silu?)(x*a+b).  `partial` is scratch f32, gn_partial_floats(Nb, HW, G) long ([Nb, nchunk, G, 2], nchunk from gn_num_chunks(HW), + the fold).
int gn_num_chunks(int HW);
size_t gn_partial_floats(int Nb, int HW, int G);  // floats of `partial` scratch (chunk partials + their fold for maps > 128 x 128)
// ab: [2][Nb][C] -- a = ab, b = ab + Nb*C.  The backward takes the two halves as separate pointers so that it can run
// on a sample sub-range of a larger forward batch.
int launch_groupnorm_fwd(int dtype, const void* x, const void* gamma, const void* beta, void* y, float* ab,
                         float* mean_rstd, float* partial, int Nb, int HW, int C, int G, float eps, int silu,
                         hipStream_t stream);
// statistics only: the partial-sum launches (+ fold) and the affine a, b into `ab` ([2][Nb][C]) and mean_rstd; no y
int launch_groupnorm_stats(int dtype, const void* x, const void* gamma, const void* beta, float* ab, float* mean_rstd,
                           float* partial, int Nb, int HW, int C, int G, float eps, hipStream_t stream);
// dx for y = silu?(GN(x)); needs x, gamma, beta, ab and mean_rstd from the forward.
// `partial`: scratch f32, gn_partial_floats(Nb, HW, G) long
// `add` (optional, may alias dx): gradient already accumulated for x, added in the same pass
int launch_groupnorm_bwd(int dtype, const void* x, const void* dy, const void* gamma, const void* beta,
                         const float* a, const float* b, const float* mean_rstd, const void* add, void* dx,
                         float* partial, int Nb, int HW, int C, int G, int silu, hipStream_t stream);
// Selection override of the parity tests, process-wide like set_attn_select: -1 follows SMI_GN_FUSED_HW / SMI_GN_FUSED_MAX
// (the default), 0 never takes the one-launch forward, 1 takes it wherever its shape rules hold (even group width of at
// most 256 channels, slice within LDS).
void set_gn_select(int fused);
// What the last launch_groupnorm_* / launch_layernorm_* of the calling thread launched (recorded on the host): form 0
// after a refused call.
enum {
  NORM_RAN_GN_ONE = 1,   // gn_fused_fwd_kernel
  NORM_RAN_GN_TWO = 2,   // partial + apply (or + stats), chunks == slots
  NORM_RAN_GN_FOLD = 3,  // partial + fold + apply: chunks > slots == 64
  NORM_RAN_LN = 4,       // ln_kernel<NV, R>
};
struct NormRan {
  int form = 0;
  int chunks = 0, slots = 0;  // GroupNorm two-launch forms: grid chunks per sample, partial slots the head re-reduces
  int nv = 0, r = 0;          // LayerNorm: 8-element vectors per lane, rows per wave
};
NormRan gn_last_ran();
int launch_layernorm_fwd(int dtype, const void* x, const void* gamma, const void* beta, void* y, float* mean_rstd,
                         int M, int C, float eps, hipStream_t stream);
int launch_layernorm_bwd(int dtype, const void* x, const void* dy, const void* gamma, const float* mean_rstd,
                         const void* add, void* dx, int M, int C, hipStream_t stream);

// ---------------------------------------------------------------------------------------------------------------
// elementwise / data movement
// ---------------------------------------------------------------------------------------------------------------
int launch_geglu_fwd(int dtype, const void* proj, void* out, int M, int C4, hipStream_t stream);  // proj [M, 2*C4]
int launch_geglu_bwd(int dtype, const void* proj, const void* dout, void* dproj, int M, int C4, hipStream_t stream);
int launch_silu(int dtype, const void* x, void* y, int64_t n, hipStream_t stream);
int launch_add(int dtype, const void* a, const void* b, void* y, int64_t n, hipStream_t stream);  // y = a + b
// CLIP text encoder pieces: y = quick_gelu(x) (kind 0) / gelu(x) (kind 1) / tanh-form gelu(x) (kind 2: the MMDiT's
// feed-forward; forward only); token + position embedding lookup; row gather
int launch_act(int dtype, const void* x, void* y, int64_t n, int kind, hipStream_t stream);
// dx = dy * act'(x) in fp32, one 16-bit rounding at the store; any n (x, dy, dx 16-byte aligned)
int launch_act_bwd(int dtype, const void* x, const void* dy, void* dx, int64_t n, int kind, hipStream_t stream);
int launch_embed(int dtype, const int* ids, const void* tok, const void* pos, void* out, int64_t rows, int L, int d,
                 int vocab, hipStream_t stream);
int launch_gather_rows(int dtype, const void* src, const int* idx, void* out, int n, int L, int d, hipStream_t stream);
// copy [M, C] (src row stride lds) into dst columns [col0, col0+C) of a [M, ldd] tensor (concat / split)
int launch_copy_cols(int dtype, const void* src, int64_t lds, void* dst, int64_t ldd, int col0, int M, int C,
                     hipStream_t stream);
// the same copy from a phase-major up-sampler output (conv2x2_phase): src [4][Nb, H, W, C], plane 2 a + b holding the
// pixels (2 i + a, 2 j + b), into columns [col0, col0 + C) of dst [Nb, 2 H, 2 W, ldd]
int launch_copy_cols_phase(int dtype, const void* src, void* dst, int64_t ldd, int col0, int Nb, int H, int W, int C,
                           hipStream_t stream);
// Up-sampler convs as four 2x2 phase convs (SMI_UPCONV_PHASE, default 1).  Override of the parity tests, process-wide
// like set_gn_select: -1 follows the environment, 0 / 1 force it off / on.  Read when an engine packs its weights and
// again at every forward; a layer with an adaptor, and the VAE decoder, keep the 3x3 form either way.
// phase pack [4][Cout][4 * Cin] of a torch filter [Cout, Cin, 3, 3] (engine.hip, next to the conv packs): per phase and
// 2x2 tap the one, two or four 3x3 weights that land on the same low-res pixel, summed in fp32 and rounded once
int launch_pack_conv_phase(int dtype, const void* src, void* dst, int Cout, int Cin, hipStream_t stream);
void set_upconv_phase(int on);
bool upconv_phase_on();
// ... and for a layer whose input map has this many pixels per sample: by default only from SMI_UPCONV_PHASE_MIN_PIXELS
// (1024 = 32 x 32) up; the override 1 takes every size (the parity tests run tiny maps)
bool upconv_phase_takes(int lowres_pixels);
int launch_nchw_to_nhwc(int dtype, const void* src, int src_f32, void* dst, int Nb, int C, int HW, int Cpad,
                        float scale, hipStream_t stream);
// f32 NCHW -> T token-major, sample n multiplied by scale_dev[n] (backward entry: loss-scaled d_eps)
int launch_nchw_to_nhwc_scaled(int dtype, const float* src, void* dst, int Nb, int C, int HW, int Cpad,
                               const float* scale_dev, hipStream_t stream);
int launch_nhwc_to_nchw_f32(const float* src, float* dst, int Nb, int C, int HW, hipStream_t stream);
// sinusoidal embedding (cos | sin, flip_sin_to_cos, freq shift 0): vals f32 [n] -> out T [n, dim]
int launch_timestep_embed(int dtype, const float* vals, void* out, int n, int dim, hipStream_t stream);
// dx[n,h,w,c] = sum_{2x2} du[n,2h+a,2w+b,c]
int launch_pool2x2_sum(int dtype, const void* du, void* dx, int Nb, int H, int W, int C, hipStream_t stream);
// P[r][:] = softmax(scale * S[r][:]) for rows of fp32 scores (materialised attention of the VAE's single 512-wide head)
int launch_softmax_rows(int dtype, const float* S, void* P, int rows, int cols, float scale, hipStream_t stream);
// y[m][j] = b[j] + sum_i x[m][i] W[j][i] on fp32 rows of width C <= 16 (the VAE's 1x1 quant_conv), W / b of dtype T
int launch_chan_mix(int dtype, const float* x, const void* W, const void* b, float* y, int64_t M, int C,
                    hipStream_t stream);
// out[n][c] = mul * sum over the HW rows of sample n of x[n][hw][c]   (deterministic)
size_t colsum_scratch_floats(int Nb, int C);  // fp32 scratch launch_colsum needs
// ldo: row stride of out in elements (0 = C): a column block of a wider matrix
int launch_colsum(int dtype, const void* x, void* out, float* scratch, int Nb, int HW, int C, float mul,
                  hipStream_t stream, int64_t ldo = 0);
// g[i] *= silu'(x[i]) in place: g fp32, x the 16-bit pre-activation
int launch_silu_bwd_f32(int dtype, const void* x, float* g, int64_t n, hipStream_t stream);
// dx[m][j] (fp32, row stride lddx) = sum_i dy[m][i] W[i][j] for j < J: the input gradient of a Linear for a few fp32 rows
// dy [M, I], read from the layer's own weight W T [I, ldw] (its first J input columns); fixed-order sums
int launch_vecmat_f32(int dtype, const float* dy, const void* W, float* dx, int M, int I, int64_t ldw, int J, int64_t lddx,
                      hipStream_t stream);
// dst[M][cpad] (T) = src[M][0..cols) (fp32, row stride lds) * mul, zero padded
int launch_f32_to_padded(int dtype, const float* src, int lds, int cols, void* dst, int cpad, int64_t M, float mul,
                         hipStream_t stream);
// power-of-two loss scales chosen on device, ONE PER SAMPLE, from max|d_eps[sample]| (keeps 16-bit activation
// gradients in range and makes a sample's backward independent of its batch mates):
// scale_out[j] = scale, scale_out[inv_off + j] = 1 / scale
int launch_grad_scale(const float* d_eps, int n_samples, int64_t per_sample, float* scale_out, int inv_off,
                      hipStream_t stream);

// AutoencoderKL decoder tail (vae_decode.hip): sample f32 [Nb, Cout, H, W] = conv_out(silu(x * a + b)) with x T [Nb, H, W, C],
// a / b = ab / ab + Nb*C (launch_groupnorm_stats), w4 T [4][9*C] (conv pack, rows >= Cout zero), bias T [Cout], Cout <= 4;
// rgb8 (optional) uint8 [Nb, H, W, Cout] = rint(clamp(sample / 2 + 0.5, 0, 1) * 255)
int launch_vae_dec_tail(int dtype, const void* x, const float* ab, const void* w4, const void* bias, float* sample,
                        uint8_t* rgb8, int Nb, int H, int W, int C, int Cout, hipStream_t stream);
int launch_rgb8_from_nchw(const float* sample, uint8_t* rgb8, int Nb, int C, int HW, hipStream_t stream);

// CLIP image tower front end and similarity head (clip_vision.hip).
// patches T [n G^2, Kp] (G = S / P, columns (c, py, px) as the patch filter's, Kp = 3 P^2 rounded up to 64, pad columns 0)
// from exactly one of rgb8 uint8 [n, S, S, 3] (normalised on the way: (u / 255 - mean[c]) / std[c]) and
// pixel_values f32 [n, 3, S, S] (already normalised); one workgroup per strip of G patches, clip_patchify_lds_bytes of LDS
size_t clip_patchify_lds_bytes(int S, int P);
int launch_clip_patchify(int dtype, const uint8_t* rgb8, const float* pixel_values, void* out, int n, int S, int P,
                         int Kp, const float mean[3], const float stdv[3], hipStream_t stream);
// out T [n tokens, d] = LayerNorm((t == 0 ? cls : patch_out[i, t - 1]) + pos[t]), the sum kept in fp32; d <= 2048
int launch_vit_embed_ln(int dtype, const void* patch_out, const void* cls, const void* pos, const void* gamma,
                        const void* beta, void* out, int n, int tokens, int d, float eps, hipStream_t stream);
// logits_per_image f32 [ni, nt] = exp(logit_scale) <i, t> / (|i| |t|) from T [ni, dim], T [nt, dim]; dim % 8 == 0
int launch_clip_logits(int dtype, const void* image_embeds, int ni, const void* text_embeds, int nt, int dim,
                       float logit_scale, float* logits_per_image, hipStream_t stream);

// MMDiT (SD3) around the GEMMs and the attention (mmdit.hip).  T is 16-bit, arithmetic fp32, one rounding at the store.
// scale / shift / gate are C columns of a row of one modulation tensor mod T [n, ldm], at column offsets that are multiples
// of 8; row r of the activations belongs to sample r / rows_per_sample.
// y[r, :] = LN(x[r, :]) (1 + scale[s, :]) + shift[s, :]: LayerNorm without affine, C % 8 == 0, C <= 3072 (the backward below:
// C <= 2048), one pass over x; mean_rstd f32 [M, 2] (may be NULL): what a backward needs
int launch_adaln_modulate(int dtype, const void* x, const void* mod, void* y, float* mean_rstd, int M, int C,
                          int rows_per_sample, int64_t ldm, int off_scale, int off_shift, float eps, hipStream_t stream);
// y[r, :] = h[r, :] + gate[s, :] f[r, :]; y may alias h
int launch_gate_residual(int dtype, const void* h, const void* f, const void* mod, void* y, int64_t M, int C,
                         int rows_per_sample, int64_t ldm, int off_gate, hipStream_t stream);
// joint T [n (Nx + Nc), W]: per sample the Nx rows of a [n Nx, W], then the Nc rows of b [n Nc, W]; W % 8 == 0.
// The split is the inverse; a or b may be NULL there (that stream is dropped)
int launch_joint_rows_pack(int dtype, const void* a, const void* b, void* joint, int n, int Nx, int Nc, int W,
                           hipStream_t stream);
int launch_joint_rows_split(int dtype, const void* joint, void* a, void* b, int n, int Nx, int Nc, int W, hipStream_t stream);
// out T [n (H/p) (W/p), Cin p p], columns (c, py, px) as the rows of pos_embed.proj.weight.reshape(d, -1), from latents
// f32 [n, Cin, H, W]; Cin p p % 64 == 0
int launch_sd3_patchify(int dtype, const float* latents, void* out, int n, int Cin, int H, int W, int p, hipStream_t stream);
// y[(i, gy, gx), :] = x[...] + pos[(top + gy) S + left + gx, :], pos T [S S, d], top = (S - gh) / 2, left = (S - gw) / 2:
// the centre-cropped window of the position table; y may alias x
int launch_sd3_add_pos(int dtype, const void* x, const void* pos, void* y, int n, int gh, int gw, int d, int S,
                       hipStream_t stream);
// out f32 [n, Cout, gh p, gw p] from rows T [n gh gw, p p Cout] with columns (py, px, c)
int launch_sd3_unpatchify(int dtype, const void* rows, float* out, int n, int Cout, int gh, int gw, int p, hipStream_t stream);
// The backwards to the activations (scale, shift and gate take no gradient: they depend on temb alone).
// dx[r, :] = rstd (g - mean_c(g) - xhat mean_c(g xhat)) (+ add[r, :]), g = dy (1 + scale[s, :]), xhat = (x - mean) rstd with
// mean_rstd from the forward; add is optional and may alias dx
int launch_adaln_modulate_bwd(int dtype, const void* x, const void* dy, const void* mod, const float* mean_rstd, const void* add,
                              void* dx, int M, int C, int rows_per_sample, int64_t ldm, int off_scale, hipStream_t stream);
// df[r, :] = gate[s, :] dy[r, :] (dh is dy)
int launch_gate_residual_bwd(int dtype, const void* dy, const void* mod, void* df, int64_t M, int C, int rows_per_sample,
                             int64_t ldm, int off_gate, hipStream_t stream);
// rows T [n gh gw, p p Cout] = scale_dev[n] x d_out f32 [n, Cout, gh p, gw p]: un-patchify's inverse; Cout p p % 8 == 0
int launch_sd3_unpatchify_bwd(int dtype, const float* d_out, void* rows, int n, int Cout, int gh, int gw, int p,
                              const float* scale_dev, hipStream_t stream);

// Flux (flux.hip).  One stream's q|k|v rows src T [n tokens, lds] (q | k | v, H heads of D each) into the joint buffer
// dst T [n L, ldd] at rows [row_off, row_off + tokens) of every sample: q and k heads x rsqrt(mean_D(x^2) + eps) w (wq / wk
// T [D]) and rotated -- interleaved pairs -- by row (row_off + t) of table f32 [L, D] = cos[D / 2] | sin[D / 2]; v copied.
// D % 16 == 0, D <= 160.  src == dst (tokens == L, row_off 0, lds == ldd): in place, v untouched
int launch_qk_norm_rope(int dtype, const void* src, int64_t lds, void* dst, int64_t ldd, const void* wq, const void* wk,
                        const float* table, int n, int tokens, int L, int row_off, int H, int D, float eps, hipStream_t stream);
// y[m, 0..C) = gelu_tanh(x[m, 0..C)) with row strides ldx / ldy (column blocks of wider matrices); y may alias x; the bits of
// launch_act kind 2
int launch_gelu_tanh_cols(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int64_t M, int C, hipStream_t stream);
// out f32 [n, Cout, gh p, gw p] from rows T [n gh gw, Cout p p] with columns (c, py, px): Flux's _unpack_latents
int launch_flux_unpack(int dtype, const void* rows, float* out, int n, int Cout, int gh, int gw, int p, hipStream_t stream);
// The backwards (wq and wk are frozen: no gradient).  qk_norm_rope's: dsrc T [n tokens, ldx] from rows [row_off, row_off + tokens)
// of every sample of the joint gradient dj T [n L, ldd] and the pre-norm source src T [n tokens, lds]: per q or k head the
// rotation's transpose, g = dy w, dx = r (g - x r^2 mean_D(g x)) with r recomputed from x; v copied.  dsrc aliases nothing
int launch_qk_norm_rope_bwd(int dtype, const void* dj, int64_t ldd, const void* src, int64_t lds, void* dsrc, int64_t ldx,
                            const void* wq, const void* wk, const float* table, int n, int tokens, int L, int row_off, int H,
                            int D, float eps, hipStream_t stream);
// dx[m, 0..C) = dy[m, 0..C) gelu_tanh'(x[m, 0..C)) with row strides ldx / ldy / ldd; the bits of launch_act_bwd kind 2
int launch_gelu_tanh_cols_bwd(int dtype, const void* x, int64_t ldx, const void* dy, int64_t ldy, void* dx, int64_t ldd, int64_t M,
                              int C, hipStream_t stream);
// rows T [n gh gw, Cout p p], columns (c, py, px), = scale_dev[n] x d_out f32 [n, Cout, gh p, gw p]: flux_unpack's inverse
int launch_flux_unpack_bwd(int dtype, const float* d_out, void* rows, int n, int Cout, int gh, int gw, int p,
                           const float* scale_dev, hipStream_t stream);

// T5 encoder (t5.hip).  The norm and the gated GELU have a backward to their input; the norm weights and the table are frozen.
// y[m, :] = w * x[m, :] * rsqrt(mean(x[m, :]^2) + eps): no mean subtracted, no bias; C % 8 == 0, C <= 8192
int launch_rmsnorm_rows(int dtype, const void* x, const void* w, void* y, int M, int C, float eps, hipStream_t stream);
// out f32 [H, 2 L - 1]: out[h, o] = weight[bucket[o], h] from relative_attention_bias.weight T [num_buckets, H] and the
// bucket of every offset o = key - query + L - 1 (int32 [2 L - 1] on the device; t5_relative_buckets fills a host copy)
int launch_t5_bias_table(int dtype, const void* weight, const int* bucket, float* out, int H, int L, int num_buckets,
                         hipStream_t stream);
// out[m, c] = gelu_tanh(proj[m, c]) * proj[m, F + c], proj T [M, 2 F] = wi_0 | wi_1; F % 8 == 0; the GELU of launch_act kind 2
int launch_gated_gelu_tanh(int dtype, const void* proj, void* out, int64_t M, int F, hipStream_t stream);
// dx[m, :] = r (w dy[m, :]) - x[m, :] r^3 mean(x[m, :] . w dy[m, :]) (+ add[m, :]), r = rsqrt(mean(x[m, :]^2) + eps) recomputed
// from x: the input gradient of launch_rmsnorm_rows for a frozen w.  fp32, one rounding; `add` (optional, may alias dx) is the
// gradient already gathered for x, summed before the rounding as in launch_layernorm_bwd.  C % 8 == 0, C <= 8192
int launch_rmsnorm_rows_bwd(int dtype, const void* x, const void* dy, const void* w, const void* add, void* dx, int M, int C,
                            float eps, hipStream_t stream);
// dproj T [M, 2 F] from proj T [M, 2 F] = gate | up and dout T [M, F]: gate half dout * up * gelu_tanh'(gate) (the derivative
// expression of launch_act_bwd kind 2), up half dout * gelu_tanh(gate); F % 8 == 0
int launch_gated_gelu_tanh_bwd(int dtype, const void* proj, const void* dout, void* dproj, int64_t M, int F, hipStream_t stream);
// host: transformers' bidirectional _relative_position_bucket for the offsets -(L - 1) .. L - 1 into out[2 L - 1]
int t5_relative_buckets(int num_buckets, int max_distance, int L, int32_t* out);

// LPIPS (AlexNet) around the GEMMs (lpips.hip).  Maps are NHWC T with C % 8 == 0 and hold PRE-activations: every reader
// applies max(0, .).  Patch matrices are T [rows, Kp], columns (ky, kx, ci), Kp a multiple of 8 >= k k C, pad columns 0.
inline int lpips_conv_out(int in, int k, int stride, int pad) { return (in + 2 * pad - k) / stride + 1; }
inline int lpips_pool_out(int in) { return (in - 3) / 2 + 1; }  // 3 x 3, stride 2, floor mode, no padding
// dst T [Cout, Kp] from a torch conv filter T [Cout, Cin, k, k]
int launch_lpips_pack_filter(int dtype, const void* src, void* dst, int Cout, int Cin, int k, int Kp, hipStream_t stream);
// patch matrix of conv1 (k 11, stride 4, pad 2; 363 columns) over 2n images, a-images first, from exactly one form:
// uint8 [n, H, W, 3] (x = u / 127.5 - 1) or f32 [n, 3, H, W] in [-1, 1]; the scaling layer (x - shift) / scale is applied
int launch_lpips_stem(int dtype, const uint8_t* rgb8_a, const uint8_t* rgb8_b, const float* img_a, const float* img_b,
                      void* out, int n, int H, int W, int Kp, hipStream_t stream);
int launch_lpips_im2col(int dtype, const void* in, void* out, int Nb, int H, int W, int C, int k, int stride, int pad,
                        int Kp, hipStream_t stream);
int launch_lpips_maxpool(int dtype, const void* in, void* out, int Nb, int H, int W, int C, hipStream_t stream);
int launch_lpips_relu(int dtype, const void* in, void* out, int64_t count, hipStream_t stream);  // out = max(0, in)
// distance head: per pair i and tap t, mean over the map of sum_c w[c] (a / (|a| + 1e-10) - b / (|b| + 1e-10))^2 with
// a = max(0, y[i]), b = max(0, y[n + i]) of y T [2n, HW, C], w T [C]; dist f32 [n] = the five taps added in order,
// per_layer f32 [n, 5] (may be NULL).  A workgroup sums LPIPS_HEAD_POS positions; `partial`: n * blk0[5] floats.
// The order of every sum follows from (HW, C) alone.
constexpr int LPIPS_HEAD_POS = 256;
struct LpipsHeadTaps {
  const void* y[5];
  const void* w[5];
  int HW[5], C[5];
  int blk0[6];  // first workgroup of each tap, blk0[5] = all of them (lpips_head_plan)
};
void lpips_head_plan(LpipsHeadTaps& taps);
int launch_lpips_head(int dtype, const LpipsHeadTaps& taps, int n, float* partial, float* dist, float* per_layer,
                      hipStream_t stream);

// ---------------------------------------------------------------------------------------------------------------
// LoRA skinny kernels (rank r <= 32)
// ---------------------------------------------------------------------------------------------------------------
// xa[M, r] = X[M, K] (T, row stride ldx) * A[r, K]^T (f32)                       (lora_down / dXA = dY * up)
int launch_lora_down(int dtype, const void* X, int64_t ldx, const float* A, int64_t lda_r, int64_t lda_k, float* xa,
                     int64_t ld_xa, int M, int K, int r, hipStream_t stream);
// dW (+)= alpha * P[M, r]^T (f32) * X[M, K] (T) -- weight-gradient reductions over M.
// Grouped form (lora.hip): one table entry per rank-r reduction dW (+)= alpha * P^T X of a backward pass
struct WgradJob {
  const void* X;           // [M, K] 16-bit operand (dY or the layer input), row stride ldx
  const float* P;          // [M, >= nseg * r] fp32 (xa or dxa), row stride ldp
  float* dW;               // output base; element (q, k) at dW[q * so_r + k * so_k]
  float* partial;          // scratch [nsplit - split0][r][K]
  const float* row_scale;  // per-sample factors applied to the rows of P (nullptr: none)
  int64_t ldx, ldp, so_r, so_k;
  int M, K, r, seg_cols, rows_per_sample;
  float alpha;
  // tail backward: M counts the rows of ALL adapted samples and fixes the geometry below, but only rows [m_begin, M) exist
  // (and are summed): X, P and row_scale start at row m_begin.  The skipped rows would add exact zeros, so the sums and their
  // order are those of the full job; split0 = m_begin / rows_per_wg splits are not launched
  int m_begin, split0;
  // conv_tap >= 0: X is an image [n][Hin][Win][K] and row m = (n, oy, ox) of the OUTPUT grid reads the input pixel of
  // filter tap (ky, kx) = (conv_tap / 3, conv_tap % 3) of a 3x3 / pad-1 conv (zero outside): the k x k LoRA down filter
  int conv_tap, Hin, Win, Hout, Wout, conv_stride, conv_ups;
  int cw, ncolblk, rows_per_wg, nsplit;  // geometry (wgrad_job_plan)
  int wg0, fb0;                          // first workgroup in the partial / final grid (wgrad_grouped_finish)
};
void wgrad_job_plan(WgradJob& j);
size_t wgrad_job_scratch_floats(const WgradJob& j);
// 16-bit shadow copies of the LoRA matrices as GEMM operands (see lora.hip); sites_dev: device array of HostLoraPrepSite
struct HostLoraPrepSite {
  int64_t off_down, off_up, dst_down, dst_up;
  int r, nseg, K, cs, rows_pad;
  // conv site (c3lier): 0 = Linear; 1 / 2 = 3x3 conv down [r][K][3][3] (K = Cin, cs = Cout) whose gradient filter
  // [K][9*64] at dst_gw has flipped (1) or plain (2: stride-2 layer) taps
  int conv;
  int64_t dst_gw;
};
// out[M, R] (fp32, row stride ldo) = X[M, K] * S[R, K]^T for R = 16 / 32 (LoRA shadow products), K % 128 == 0
int launch_row_scale_f32(float* x, int ld, int M, int N, const float* row_mul, int rows_per_mul, hipStream_t stream);
bool lora_skinny_supported(const void* X, int64_t ldx, const void* S, const float* out, int ldo, int M, int R, int K);
int launch_lora_skinny(int dtype, const void* X, int64_t ldx, const void* S, float* out, int ldo, int M, int R, int K,
                       hipStream_t stream, const float* row_mul = nullptr, int rows_per_mul = 1);
// the same product with one multiplier per (sample, column): out[m][c] *= col_mul[(m / rows_per_mul) * ld_mul + c % period]
// after the fixed-order reduction (one fp32 multiply); for the shapes launch_lora_skinny takes
int launch_lora_skinny_cols(int dtype, const void* X, int64_t ldx, const void* S, float* out, int ldo, int M, int R, int K,
                            const float* col_mul, int ld_mul, int period, int rows_per_mul, hipStream_t stream);
// x[m][n] *= col_mul[(m / rows_per_mul) * ld_mul + n % period] for n < N: that table on the shapes the kernel above refuses
int launch_col_scale_f32(float* x, int ld, int M, int N, const float* col_mul, int ld_mul, int period, int rows_per_mul,
                         hipStream_t stream);
// slider composition: one (site, slider) block of the rank-stacked flat buffers (lora.hip lora_stack_kernel); the layout of
// smi_lora_stack_job
struct LoraStackJob {
  const float* src_down;  // [r][row_len], NULL: the slider does not adapt the site -- its block is written as zeros
  const float* src_up;    // [n_out][r], NULL with src_down
  float* dst_down;        // the site's stacked down [R][row_len]
  float* dst_up;          // the site's stacked up [n_out][R]
  int64_t row_len;        // floats per lora_down row: `in` (Linear), Cin * kh * kw (conv)
  int r, c0, R, n_out;    // the slider's rank at the site, its first rank column, the stacked rank, rows of lora_up
  float coef;             // folded into up: alpha / r, or scale * alpha / r
  int pad_;
};
int launch_lora_stack(const LoraStackJob* jobs_dev, int n_jobs, hipStream_t stream);
// ---- DoRA (T/dora.py:124-162): dW = (W + up down) * (g / ||W + up down||_col) - W per adapted Linear (fused segments share W)
struct DoraSite {
  const void* W;                       // frozen [nseg * cs, K], 16-bit
  int64_t off_down, off_up, off_dora;  // of segment 0; segment s at + s*r*K, + s*cs*r, + s*K
  void* dW;                            // out: [nseg * cs, K] 16-bit, = lscale * dW
  void* dWt;                           // out (launch_dora_transpose): [K, nseg * cs], the dX GEMM's operand
  float* cnorm;                        // out: [nseg, K] column norms (detached in the backward)
  int r, nseg, K, cs;
  float scale;                         // alpha / rank
};
// per adapted forward: column norms, then the scaled delta weights (lscale = mult * site.scale folded in)
int launch_dora_prep(int dtype, const DoraSite* sites_dev, const DoraSite* sites_host, int n_sites, const float* down,
                     const float* up, float mult, hipStream_t stream);
// dWt = dW^T of every site in ONE launch (the backward of a saved forward needs them; 280 launches of 12 us before)
int launch_dora_transpose(int dtype, const DoraSite* sites_dev, const DoraSite* sites_host, int n_sites,
                          hipStream_t stream);
// dst[c][m] = src[m][c] * (f ? f[m / rows_per_sample] : 1) for m < M, 0 for M <= m < Mp      (dst [C, Mp], 16-bit)
int launch_transpose_scaled(int dtype, const void* src, int64_t lds, void* dst, int M, int C, int Mp, const float* f,
                            int rows_per_sample, hipStream_t stream);
// gradients of one DoRA Linear from G = dY^T X (fp32 [nseg*cs, K]): d(dora_scale), d(down) (column-wise), d(up) (row-wise);
// everything x alpha x *alpha_dev; accumulates (+=) into the flat gradient buffers
// `scratch`: dora_grad_scratch_floats(site) floats (row-slice partials of the column-wise sums)
size_t dora_grad_scratch_floats(const DoraSite& site);
int launch_dora_grads(int dtype, const DoraSite& site, const float* G, const float* down, const float* up,
                      float* d_down, float* d_up, float alpha, const float* alpha_dev, float* scratch,
                      hipStream_t stream);
// scale_buf[0..n) per-sample loss scales -> out[0] = min, out[1] = 1 / min, out[2 + j] = min / scale_j
int launch_scale_min(const float* scale_buf, int n, float* out, hipStream_t stream);
int wgrad_grouped_finish(std::vector<WgradJob>& jobs);
int launch_lora_wgrad_grouped(int dtype, const std::vector<WgradJob>& jobs, const WgradJob* jobs_dev,
                              hipStream_t stream);
int launch_lora_prep(int dtype, const void* sites_dev, int n_sites, const float* down, const float* up, void* shadow,
                     hipStream_t stream);

// ---------------------------------------------------------------------------------------------------------------
// slider-step elementwise ops (K9-K11)
// ---------------------------------------------------------------------------------------------------------------
int launch_cfg_combine(const float* eps2 /*[2B,...]*/, float* out /*[B,...]*/, int64_t n_half, float g,
                       hipStream_t stream);
// loss = mean((target - (neutral + sign*eta*(positive - negative)))^2) ; dtarget = 2*(target-goal)/n
int launch_slider_loss(const float* target, const float* positive, const float* neutral, const float* negative,
                       float sign_eta, int64_t n, float* loss_out, float* dtarget, float* scratch,
                       hipStream_t stream);
// null-text inner step: loss = mean((c_x x_t + c_eps (eps_u + g (eps_c - eps_u)) - target)^2), d_eps_u (may be NULL) =
// d(loss)/d(eps_u); fixed-order sum; scratch >= 256 floats
int launch_nulltext_loss(const float* eps_u, const float* eps_c, const float* x_t, const float* target, float g, float c_x,
                         float c_eps, int64_t n, float* loss_out, float* d_eps_u, float* scratch, hipStream_t stream);
int launch_axpby(float* y, const float* x, float a, float b, int64_t n, hipStream_t stream);  // y = a*x + b*y
// global-norm clip (max_norm<=0: none) + AdamW on flat f32 buffers; state m,v; step>=1
int launch_clip_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                      float eps, float weight_decay, int step, float max_norm, float* scratch /*>= 1024+2 floats*/,
                      hipStream_t stream);
// global-norm clip + Lion (include/smi.h smi_clip_lion); state m; scratch >= 1 + 1024 floats
int launch_clip_lion(float* p, const float* g, float* m, int64_t n, double lr, double beta1, double beta2,
                     double weight_decay, float max_norm, float* scratch, hipStream_t stream);
// Prodigy (include/smi.h smi_prodigy_init / smi_clip_prodigy; the fields of smi_prodigy_hyper): state p0, m, v, s and
// the 8-double device block; scratch >= 1 + 3 * 1024 floats
struct ProdigyHyper {
  double lr, beta1, beta2, beta3, eps, weight_decay, d0, d_coef, growth_rate;
  int decouple, use_bias_correction, safeguard_warmup;
};
int launch_prodigy_init(const float* p, float* p0, float* m, float* v, float* s, int64_t n, double d0, double* state,
                        hipStream_t stream);
int launch_clip_prodigy(float* p, const float* g, const float* p0, float* m, float* v, float* s, int64_t n,
                        const ProdigyHyper* h, float max_norm, double* state, float* scratch, hipStream_t stream);
// DDIM (eta=0): x = c0*x + c1*eps ; Euler-a: x = x + eps*dt + noise*sigma_up
int launch_sched_affine(float* x, const float* eps, const float* noise, float c_x, float c_eps, float c_noise,
                        int64_t n, hipStream_t stream);

}  // namespace smi
