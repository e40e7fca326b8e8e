// The C entry points that touch no engine: the last-error text, the fp32 helpers of the training and sampling loops, and
// the single-kernel `smi_op_*` entries of the parity tests.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/smi.h"
#include "kernels.h"

namespace smi {

static thread_local char g_err[2048] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

}  // namespace smi

using namespace smi;

extern "C" {

const char* smi_last_error(void) { return g_err; }

int smi_cfg_combine(const float* eps_2n, float* out_n, int64_t n_half, float g, void* stream) {
  return launch_cfg_combine(eps_2n, out_n, n_half, g, (hipStream_t)stream);
}
int smi_slider_loss(const float* target, const float* positive, const float* neutral, const float* negative,
                    float sign_eta, int64_t n, float* loss_out, float* dtarget, float* scratch, void* stream) {
  return launch_slider_loss(target, positive, neutral, negative, sign_eta, n, loss_out, dtarget, scratch,
                            (hipStream_t)stream);
}
int smi_nulltext_loss(const float* eps_u, const float* eps_c, const float* x_t, const float* target, float guidance_scale,
                      float c_x, float c_eps, int64_t n, float* loss_out, float* d_eps_u, float* scratch, void* stream) {
  return launch_nulltext_loss(eps_u, eps_c, x_t, target, guidance_scale, c_x, c_eps, n, loss_out, d_eps_u, scratch,
                              (hipStream_t)stream);
}
int smi_clip_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, float max_norm, float* scratch,
                   void* stream) {
  return launch_clip_adamw(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, max_norm,
                           scratch, (hipStream_t)stream);
}
int smi_clip_lion(float* param, const float* grad, float* exp_avg, int64_t n, double lr, double beta1, double beta2,
                  double weight_decay, float max_norm, float* scratch, void* stream) {
  return launch_clip_lion(param, grad, exp_avg, n, lr, beta1, beta2, weight_decay, max_norm, scratch, (hipStream_t)stream);
}
int smi_prodigy_init(const float* param, float* p0, float* exp_avg, float* exp_avg_sq, float* s, int64_t n, double d0,
                     double* state, void* stream) {
  return launch_prodigy_init(param, p0, exp_avg, exp_avg_sq, s, n, d0, state, (hipStream_t)stream);
}
int smi_clip_prodigy(float* param, const float* grad, const float* p0, float* exp_avg, float* exp_avg_sq, float* s,
                     int64_t n, const smi_prodigy_hyper* hyper, float max_norm, double* state, float* scratch,
                     void* stream) {
  if (!hyper) {
    set_error("smi_clip_prodigy: hyper is NULL");
    return 1;
  }
  const ProdigyHyper h{hyper->lr,     hyper->beta1,  hyper->beta2,       hyper->beta3,    hyper->eps, hyper->weight_decay,
                       hyper->d0,     hyper->d_coef, hyper->growth_rate, hyper->decouple, hyper->use_bias_correction,
                       hyper->safeguard_warmup};
  return launch_clip_prodigy(param, grad, p0, exp_avg, exp_avg_sq, s, n, &h, max_norm, state, scratch, (hipStream_t)stream);
}
int smi_sched_step(float* x, const float* eps, const float* noise, float c_x, float c_eps, float c_noise, int64_t n,
                   void* stream) {
  return launch_sched_affine(x, eps, noise, c_x, c_eps, c_noise, n, (hipStream_t)stream);
}

// ---- single-kernel entry points for the parity tests -----------------------------------------------------------
int smi_op_gemm_scratch(void* ws, size_t bytes) {
  smi::set_gemm_scratch(ws, bytes);
  return 0;
}
int smi_op_gemm(int dtype, const void* A, const void* W, void* C, int M, int N, int K, const void* bias,
                const void* res, const float* lora_xa, const float* lora_up, int lora_r, float lora_scale,
                int out_f32, void* stream) {
  GemmParams p = gemm_nt(dtype, A, K, W, C, N, M, N, K).with_bias(bias).with_res(res, N);
  if (out_f32) p.f32_out();
  return launch_gemm(p.with_lora(lora_xa, lora_r, lora_up, lora_r, 0, lora_scale, 0), (hipStream_t)stream);
}
int smi_op_gemm_rows(int dtype, const void* A, const void* W, void* C, int M, int N, int K, const void* bias,
                     const void* res, const float* lora_xa, const float* lora_up, int lora_r, float lora_scale,
                     int lora_row0, int lora_seg, void* stream) {
  GemmParams p = gemm_nt(dtype, A, K, W, C, N, M, N, K).with_bias(bias).with_res(res, N);
  return launch_gemm(p.with_lora(lora_xa, (int64_t)lora_r * (lora_seg > 0 ? N / lora_seg : 1), lora_up, lora_r, lora_seg,
                                 lora_scale, lora_row0),
                     (hipStream_t)stream);
}
int smi_op_gemm_epilogue(int dtype, const void* A, const void* W, void* C, int M, int N, int K, int out_f32,
                         const void* bias, const void* res, const void* rowvec, int rows_per_vec, int ld_rowvec,
                         const float* lora_xa, int ld_xa, const float* lora_up, int lora_r, int lora_seg, int lora_row0,
                         float lora_scale, int lora_dx, int tile_code, int ksplit, int* ran_code, void* stream) {
  GemmParams p = gemm_nt(dtype, A, K, W, C, N, M, N, K).with_bias(bias).with_res(res, N);
  if (out_f32) p.f32_out();
  if (rowvec) p.with_rowvec(rowvec, rows_per_vec, ld_rowvec);
  if (lora_xa && lora_dx) p.with_lora_dx(lora_xa, ld_xa, lora_up, lora_r, lora_scale);
  else if (lora_xa) p.with_lora(lora_xa, ld_xa, lora_up, lora_r, lora_seg, lora_scale, lora_row0);
  return launch_gemm_on_tile(p, tile_code, ksplit, ran_code, (hipStream_t)stream);
}
int smi_op_gemm_geglu(int dtype, const void* A, const void* W, const void* bias, void* out, void* proj, int M, int N,
                      int K, int proj_row0, void* stream) {
  return launch_gemm(gemm_nt(dtype, A, K, W, proj, N, M, N, K).with_bias(bias).with_geglu(out, proj_row0), (hipStream_t)stream);
}
int smi_op_conv3x3(int dtype, const void* in, const void* w_packed, const void* bias, void* out, int nb, int hin,
                   int win, int cin, int cout, int stride, int upsample, int transposed, int hout, int wout,
                   void* stream) {
  return launch_gemm(conv3x3_geom(dtype, in, w_packed, out, nb, hin, win, cin, cout, hout, wout, stride, 1, upsample, transposed)
                         .with_bias(bias),
                     (hipStream_t)stream);
}
// a 3x3 conv of any gather mode with every epilogue term on a NAMED tile (see include/smi.h); the geometry checks of
// launch_gemm hold on the named-tile path too (launch_gemm_on_tile)
int smi_op_conv3x3_ex(int dtype, const void* in, const void* w_packed, const void* bias, void* out, int nb, int hin, int win,
                      int cin, int cout, int stride, int upsample, int transposed, int hout, int wout, int pad, int out_f32,
                      const void* res, const void* rowvec, int rows_per_vec, int ld_rowvec, const float* lora_xa, int ld_xa,
                      const float* lora_up, int lora_r, int lora_row0, float lora_scale, int tile_code, int ksplit,
                      int* ran_code, void* stream) {
  if (ran_code) *ran_code = 0;
  if (!in || !w_packed || !out || nb <= 0 || hin <= 0 || win <= 0 || cin <= 0 || cout <= 0 || hout <= 0 || wout <= 0) {
    set_error("smi_op_conv3x3_ex: bad arguments");
    return -1;
  }
  SMI_CHECK((int64_t)nb * hout * wout < (1ll << 31) && (int64_t)nb * hin * win < (1ll << 31),
            "smi_op_conv3x3_ex: more than 2^31 pixels");
  SMI_CHECK(pad == 0 || pad == 1, "smi_op_conv3x3_ex: pad=%d (0 or 1)", pad);
  SMI_CHECK(!upsample || (stride == 1 && pad == 1 && !transposed), "smi_op_conv3x3_ex: upsample takes stride 1, pad 1, forward");
  SMI_CHECK(!transposed || pad == 1, "smi_op_conv3x3_ex: the transposed gather is the gradient of a pad-1 conv");
  if (stride == 1 || stride == 2) {  // (any other stride: launch_gemm_on_tile's geometry check refuses it)
    // forward: the output grid follows from the input's (pad 0: the (0, 1, 0, 1)-padded down-sampler, even maps);
    // transposed: `in` is dy on the forward's OUTPUT grid, `out` is dx on its input grid
    const int mode = stride == 2 ? 1 : (upsample ? 2 : 0);
    const bool ok = transposed ? (hin == conv3x3_out(hout, mode) && win == conv3x3_out(wout, mode))
                               : (hout == conv3x3_out(hin, mode) && wout == conv3x3_out(win, mode));
    SMI_CHECK(ok, "smi_op_conv3x3_ex: inconsistent geometry: %d x %d -> %d x %d (stride %d, upsample %d, transposed %d)", hin,
              win, hout, wout, stride, upsample, transposed);
    SMI_CHECK(pad == 1 || (stride == 2 && hin % 2 == 0 && win % 2 == 0),
              "smi_op_conv3x3_ex: pad 0 is the stride-2 down-sampler on an even map (%d x %d, stride %d)", hin, win, stride);
  }
  SMI_CHECK(!rowvec || rows_per_vec >= 1, "smi_op_conv3x3_ex: rows_per_vec=%d", rows_per_vec);
  SMI_CHECK(!lora_xa || (lora_up && lora_r >= 1 && ld_xa >= lora_r && lora_row0 >= 0 && lora_row0 < nb * hout * wout),
            "smi_op_conv3x3_ex: delta: r=%d ld_xa=%d row0=%d", lora_r, ld_xa, lora_row0);
  GemmParams p = conv3x3_geom(dtype, in, w_packed, out, nb, hin, win, cin, cout, hout, wout, stride, pad, upsample, transposed)
                     .with_bias(bias)
                     .with_res(res, cout);
  if (out_f32) p.f32_out();
  if (rowvec) p.with_rowvec(rowvec, rows_per_vec, ld_rowvec);
  if (lora_xa) p.with_lora(lora_xa, ld_xa, lora_up, lora_r, 0, lora_scale, lora_row0);
  return launch_gemm_on_tile(p, tile_code, ksplit, ran_code, (hipStream_t)stream);
}
// nearest-2x + 3x3 / pad 1 as the engine's phase form: pack, four 2x2 phase convs, un-shuffle (see include/smi.h)
int smi_op_upconv_phase(int dtype, const void* in, const void* w, const void* bias, void* wph, void* planes, void* out, int nb,
                        int h, int w_, int cin, int cout, int tile_code, int* ran_code, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!in || !w || !wph || !planes || !out || nb <= 0 || h <= 0 || w_ <= 0 || cin <= 0 || cout <= 0) {
    set_error("smi_op_upconv_phase: bad arguments");
    return -1;
  }
  if (int rc = launch_pack_conv_phase(dtype, w, wph, cout, cin, st)) return rc;
  for (int ph = 0; ph < 4; ++ph) {
    int ran = 0;
    const GemmParams p = conv2x2_phase(dtype, in, wph, planes, nb, h, w_, cin, cout, ph).with_bias(bias);
    if (int rc = launch_gemm_on_tile(p, tile_code, 0, &ran, st)) return rc;
    if (ran_code) ran_code[ph] = ran;
  }
  return launch_copy_cols_phase(dtype, planes, out, cout, 0, nb, h, w_, cout, st);
}
int smi_set_upconv_phase(int on) {
  set_upconv_phase(on);
  return 0;
}
// dense [b, n, h, d] operands: every leading dimension is h * d
static AttnParams attn_dense(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int b, int h,
                             int nq, int nk, int d, float scale) {
  AttnParams p;
  p.dtype = dtype;
  p.Q = q;
  p.K = k;
  p.V = v;
  p.O = o;
  p.lse = lse;
  p.ldq = p.ldk = p.ldv = p.ldo = p.lddo = p.lddq = p.lddk = p.lddv = (int64_t)h * d;
  p.B = b;
  p.H = h;
  p.Nq = nq;
  p.Nk = nk;
  p.D = d;
  p.scale = scale;
  return p;
}
int smi_op_attention_fwd(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int b, int h,
                         int nq, int nk, int d, float scale, void* stream) {
  return launch_attn_fwd(attn_dense(dtype, q, k, v, o, lse, b, h, nq, nk, d, scale), (hipStream_t)stream);
}
int smi_op_attention_bwd(int dtype, const void* q, const void* k, const void* v, const void* o, const float* lse,
                         const void* d_o, void* dq, void* dk, void* dv, float* delta, int b, int h, int nq, int nk,
                         int d, float scale, void* stream) {
  AttnParams p = attn_dense(dtype, q, k, v, const_cast<void*>(o), const_cast<float*>(lse), b, h, nq, nk, d, scale);
  p.dO = d_o;
  p.dQ = dq;
  p.dK = dk;
  p.dV = dv;
  p.delta = delta;
  return launch_attn_bwd(p, (hipStream_t)stream);
}
// every operand at its own leading dimension, the kernel selection pinned for this call, what ran reported back
static AttnParams attn_ex(const smi_attn_args* a) {
  AttnParams p;
  p.dtype = a->dtype;
  p.Q = a->q;
  p.K = a->k;
  p.V = a->v;
  p.O = a->o;
  p.lse = a->lse;
  p.ldq = a->ldq;
  p.ldk = a->ldk;
  p.ldv = a->ldv;
  p.ldo = a->ldo;
  p.B = a->b;
  p.H = a->h;
  p.Nq = a->nq;
  p.Nk = a->nk;
  p.D = a->d;
  p.scale = a->scale;
  p.causal = a->causal;
  p.dO = a->d_o;
  p.lddo = a->lddo;
  p.delta = a->delta;
  p.dQ = a->dq;
  p.dK = a->dk;
  p.dV = a->dv;
  p.lddq = a->lddq;
  p.lddk = a->lddk;
  p.lddv = a->lddv;
  return p;
}
static int attn_ex_run(const smi_attn_args* a, smi_attn_ran* ran, bool bwd) {
  if (!a) {
    set_error("smi_op_attention_ex: NULL arguments");
    return -1;
  }
  set_attn_select(a->sel_xs, a->sel_fused);
  const AttnParams p = attn_ex(a);
  const int rc = bwd ? launch_attn_bwd(p, (hipStream_t)a->stream) : launch_attn_fwd(p, (hipStream_t)a->stream);
  set_attn_select(-1, -1);
  if (ran) {
    const AttnRan r = attn_last_ran();
    ran->dp = r.dp;
    ran->form = r.form;
    ran->n_launches = r.n;
    for (int i = 0; i < 4; ++i) ran->family[i] = r.family[i];
    ran->chain = r.chain;
  }
  return rc;
}
int smi_op_attention_ex_fwd(const smi_attn_args* a, smi_attn_ran* ran) { return attn_ex_run(a, ran, false); }
int smi_op_attention_ex_bwd(const smi_attn_args* a, smi_attn_ran* ran) { return attn_ex_run(a, ran, true); }
// causal self-attention (nq == nk == n) with explicit leading dimensions: the engine's fused [M, 3C] q|k|v layout
static AttnParams attn_causal(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int b, int h, int n,
                              int d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale) {
  AttnParams p = attn_dense(dtype, q, k, v, o, lse, b, h, n, n, d, scale);
  p.ldq = ldq;
  p.ldk = ldk;
  p.ldv = ldv;
  p.ldo = ldo;
  p.causal = 1;
  return p;
}
int smi_op_attention_causal_fwd(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int b, int h,
                                int n, int d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale, void* stream) {
  return launch_attn_fwd(attn_causal(dtype, q, k, v, o, lse, b, h, n, d, ldq, ldk, ldv, ldo, scale), (hipStream_t)stream);
}
int smi_op_attention_causal_bwd(int dtype, const void* q, const void* k, const void* v, const void* o, const float* lse,
                                const void* d_o, void* dq, void* dk, void* dv, float* delta, int b, int h, int nq, int nk,
                                int d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddo, int64_t lddq,
                                int64_t lddk, int64_t lddv, float scale, void* stream) {
  AttnParams p = attn_causal(dtype, q, k, v, const_cast<void*>(o), const_cast<float*>(lse), b, h, nq, d, ldq, ldk, ldv, ldo, scale);
  p.Nk = nk;
  p.dO = d_o;
  p.lddo = lddo;
  p.dQ = dq;
  p.dK = dk;
  p.dV = dv;
  p.lddq = lddq;
  p.lddk = lddk;
  p.lddv = lddv;
  p.delta = delta;
  return launch_attn_bwd(p, (hipStream_t)stream);
}
// T5's self-attention: no mask, the additive relative-position table (smi_op_t5_bias_table), always the tiled forward
int smi_op_attention_bias_fwd(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, const float* table,
                              int64_t ld_table, int b, int h, int n, int d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                              float scale, void* stream) {
  SMI_CHECK(table != nullptr, "smi_op_attention_bias_fwd: table is NULL (attention without a bias is smi_op_attention_ex_fwd)");
  AttnParams p = attn_causal(dtype, q, k, v, o, lse, b, h, n, d, ldq, ldk, ldv, ldo, scale);
  p.causal = 0;
  p.bias = table;
  p.bias_ld = ld_table;
  return launch_attn_fwd(p, (hipStream_t)stream);
}
// its backward: smi_attn_args as smi_op_attention_ex_bwd takes them (lse from smi_op_attention_bias_fwd), plus the table
int smi_op_attention_bias_bwd(const smi_attn_args* a, const float* table, int64_t ld_table, smi_attn_ran* ran) {
  if (!a) {
    set_error("smi_op_attention_bias_bwd: NULL arguments");
    return -1;
  }
  SMI_CHECK(table != nullptr, "smi_op_attention_bias_bwd: table is NULL (attention without a bias is smi_op_attention_ex_bwd)");
  set_attn_select(a->sel_xs, a->sel_fused);
  AttnParams p = attn_ex(a);
  p.bias = table;
  p.bias_ld = ld_table;
  const int rc = launch_attn_bwd(p, (hipStream_t)a->stream);
  set_attn_select(-1, -1);
  if (ran) {
    const AttnRan r = attn_last_ran();
    ran->dp = r.dp;
    ran->form = r.form;
    ran->n_launches = r.n;
    for (int i = 0; i < 4; ++i) ran->family[i] = r.family[i];
    ran->chain = r.chain;
  }
  return rc;
}
int smi_op_rmsnorm(int dtype, const void* x, const void* w, void* y, int m, int c, float eps, void* stream) {
  return launch_rmsnorm_rows(dtype, x, w, y, m, c, eps, (hipStream_t)stream);
}
int smi_op_rmsnorm_bwd(int dtype, const void* x, const void* dy, const void* w, const void* add, void* dx, int m, int c,
                       float eps, void* stream) {
  return launch_rmsnorm_rows_bwd(dtype, x, dy, w, add, dx, m, c, eps, (hipStream_t)stream);
}
int smi_op_gated_gelu_tanh_bwd(int dtype, const void* proj, const void* dout, void* dproj, int64_t m, int f, void* stream) {
  return launch_gated_gelu_tanh_bwd(dtype, proj, dout, dproj, m, f, (hipStream_t)stream);
}
int smi_op_gated_gelu_tanh(int dtype, const void* proj, void* out, int64_t m, int f, void* stream) {
  return launch_gated_gelu_tanh(dtype, proj, out, m, f, (hipStream_t)stream);
}
int smi_op_t5_bias_table(int dtype, const void* weight, const int32_t* bucket, float* out, int h, int l, int num_buckets,
                         void* stream) {
  return launch_t5_bias_table(dtype, weight, bucket, out, h, l, num_buckets, (hipStream_t)stream);
}
int smi_op_act(int dtype, const void* x, void* y, const void* dy, void* dx, int64_t n, int kind, void* stream) {
  if (y)
    if (int rc = launch_act(dtype, x, y, n, kind, (hipStream_t)stream)) return rc;
  if (!dy) return 0;
  return launch_act_bwd(dtype, x, dy, dx, n, kind, (hipStream_t)stream);
}
// scratch layout (floats): ab[2*nb*c] | mean_rstd[nb*g*2] | partial[...]
int smi_op_groupnorm(int dtype, const void* x, const void* gamma, const void* beta, void* y, const void* dy, void* dx,
                     float* scratch, int nb, int hw, int c, int g, float eps, int silu, void* stream) {
  float* ab = scratch;
  float* mr = ab + (size_t)2 * nb * c;
  float* part = mr + (size_t)nb * g * 2;
  int rc = launch_groupnorm_fwd(dtype, x, gamma, beta, y, ab, mr, part, nb, hw, c, g, eps, silu, (hipStream_t)stream);
  if (rc || !dy) return rc;
  return launch_groupnorm_bwd(dtype, x, dy, gamma, beta, ab, ab + (size_t)nb * c, mr, nullptr, dx, part, nb, hw, c, g, silu,
                              (hipStream_t)stream);
}
int smi_op_layernorm(int dtype, const void* x, const void* gamma, const void* beta, void* y, const void* dy, void* dx,
                     float* mean_rstd, int m, int c, float eps, void* stream) {
  int rc = launch_layernorm_fwd(dtype, x, gamma, beta, y, mean_rstd, m, c, eps, (hipStream_t)stream);
  if (rc || !dy) return rc;
  return launch_layernorm_bwd(dtype, x, dy, gamma, mean_rstd, nullptr, dx, m, c, (hipStream_t)stream);
}
static void norm_ran_out(smi_norm_ran* out) {
  if (!out) return;
  const NormRan r = gn_last_ran();
  out->form = r.form;
  out->chunks = r.chunks;
  out->slots = r.slots;
  out->nv = r.nv;
  out->r = r.r;
}
// forward (or statistics only) on nb samples, backward on samples [bwd_n0, nb) with the engine's offset pointers
int smi_op_groupnorm_ex(const smi_norm_args* a, smi_norm_ran* ran_fwd, smi_norm_ran* ran_bwd) {
  if (!a) {
    set_error("smi_op_groupnorm_ex: NULL arguments");
    return -1;
  }
  if (a->bwd_n0 < 0 || a->bwd_n0 >= a->nb) {
    set_error("smi_op_groupnorm_ex: bwd_n0=%d outside [0, nb=%d)", a->bwd_n0, a->nb);
    return -1;
  }
  const int nb = a->nb, hw = a->hw, c = a->c, g = a->g, n0 = a->bwd_n0;
  float* ab = a->scratch;
  float* mr = ab + (size_t)2 * nb * c;
  float* part = mr + (size_t)nb * g * 2;
  hipStream_t st = (hipStream_t)a->stream;
  set_gn_select(a->sel_fused);
  int rc = a->y ? launch_groupnorm_fwd(a->dtype, a->x, a->gamma, a->beta, a->y, ab, mr, part, nb, hw, c, g, a->eps, a->silu, st)
                : launch_groupnorm_stats(a->dtype, a->x, a->gamma, a->beta, ab, mr, part, nb, hw, c, g, a->eps, st);
  set_gn_select(-1);
  norm_ran_out(ran_fwd);
  if (rc || !a->dy) return rc;
  const char* xs = (const char*)a->x + (size_t)n0 * hw * c * 2;  // both types are 2 bytes wide
  rc = launch_groupnorm_bwd(a->dtype, xs, a->dy, a->gamma, a->beta, ab + (size_t)n0 * c, ab + (size_t)(nb + n0) * c,
                            mr + (size_t)n0 * g * 2, a->add, a->dx, part, nb - n0, hw, c, g, a->silu, st);
  norm_ran_out(ran_bwd);
  return rc;
}
// forward on m rows (nb = m; hw, g, silu, sel_fused unused; scratch = mean_rstd f32 [m, 2]), backward on rows [bwd_n0, m)
int smi_op_layernorm_ex(const smi_norm_args* a, smi_norm_ran* ran_fwd, smi_norm_ran* ran_bwd) {
  if (!a) {
    set_error("smi_op_layernorm_ex: NULL arguments");
    return -1;
  }
  if (a->bwd_n0 < 0 || a->bwd_n0 >= a->nb) {
    set_error("smi_op_layernorm_ex: bwd_row0=%d outside [0, m=%d)", a->bwd_n0, a->nb);
    return -1;
  }
  const int m = a->nb, c = a->c, r0 = a->bwd_n0;
  hipStream_t st = (hipStream_t)a->stream;
  int rc = launch_layernorm_fwd(a->dtype, a->x, a->gamma, a->beta, a->y, a->scratch, m, c, a->eps, st);
  norm_ran_out(ran_fwd);
  if (rc || !a->dy) return rc;
  rc = launch_layernorm_bwd(a->dtype, (const char*)a->x + (size_t)r0 * c * 2, a->dy, a->gamma, a->scratch + (size_t)r0 * 2, a->add,
                            a->dx, m - r0, c, st);
  norm_ran_out(ran_bwd);
  return rc;
}
// ---- the small elementwise kernels, one thin entry each
int smi_op_pool2x2_sum(int dtype, const void* du, void* dx, int nb, int h, int w, int c, void* stream) {
  return launch_pool2x2_sum(dtype, du, dx, nb, h, w, c, (hipStream_t)stream);
}
int smi_op_colsum_floats(int nb, int c, size_t* out_floats) {
  *out_floats = colsum_scratch_floats(nb, c);
  return 0;
}
int smi_op_colsum(int dtype, const void* x, void* out, float* scratch, int nb, int hw, int c, float mul, void* stream) {
  return launch_colsum(dtype, x, out, scratch, nb, hw, c, mul, (hipStream_t)stream);
}
int smi_op_timestep_embed(int dtype, const float* vals, void* out, int n, int dim, void* stream) {
  return launch_timestep_embed(dtype, vals, out, n, dim, (hipStream_t)stream);
}
// the MMDiT kernels (mmdit.hip)
int smi_op_adaln_modulate(int dtype, const void* x, const void* mod, void* y, float* mean_rstd, int m, int c,
                          int rows_per_sample, int64_t ldm, int off_scale, int off_shift, float eps, void* stream) {
  return launch_adaln_modulate(dtype, x, mod, y, mean_rstd, m, c, rows_per_sample, ldm, off_scale, off_shift, eps,
                               (hipStream_t)stream);
}
int smi_op_gate_residual(int dtype, const void* h, const void* f, const void* mod, void* y, int64_t m, int c,
                         int rows_per_sample, int64_t ldm, int off_gate, void* stream) {
  return launch_gate_residual(dtype, h, f, mod, y, m, c, rows_per_sample, ldm, off_gate, (hipStream_t)stream);
}
int smi_op_adaln_modulate_bwd(int dtype, const void* x, const void* dy, const void* mod, const float* mean_rstd, const void* add,
                              void* dx, int m, int c, int rows_per_sample, int64_t ldm, int off_scale, void* stream) {
  return launch_adaln_modulate_bwd(dtype, x, dy, mod, mean_rstd, add, dx, m, c, rows_per_sample, ldm, off_scale,
                                   (hipStream_t)stream);
}
int smi_op_gate_residual_bwd(int dtype, const void* dy, const void* mod, void* df, int64_t m, int c, int rows_per_sample,
                             int64_t ldm, int off_gate, void* stream) {
  return launch_gate_residual_bwd(dtype, dy, mod, df, m, c, rows_per_sample, ldm, off_gate, (hipStream_t)stream);
}
int smi_op_joint_rows_pack(int dtype, const void* a, const void* b, void* joint, int n, int nx, int nc, int w, void* stream) {
  return launch_joint_rows_pack(dtype, a, b, joint, n, nx, nc, w, (hipStream_t)stream);
}
int smi_op_joint_rows_split(int dtype, const void* joint, void* a, void* b, int n, int nx, int nc, int w, void* stream) {
  return launch_joint_rows_split(dtype, joint, a, b, n, nx, nc, w, (hipStream_t)stream);
}
int smi_op_sd3_patchify(int dtype, const float* latents, void* out, int n, int cin, int h, int w, int p, void* stream) {
  return launch_sd3_patchify(dtype, latents, out, n, cin, h, w, p, (hipStream_t)stream);
}
int smi_op_sd3_add_pos(int dtype, const void* x, const void* pos, void* y, int n, int gh, int gw, int d, int s, void* stream) {
  return launch_sd3_add_pos(dtype, x, pos, y, n, gh, gw, d, s, (hipStream_t)stream);
}
int smi_op_sd3_unpatchify(int dtype, const void* rows, float* out, int n, int cout, int gh, int gw, int p, void* stream) {
  return launch_sd3_unpatchify(dtype, rows, out, n, cout, gh, gw, p, (hipStream_t)stream);
}
int smi_op_qk_norm_rope(int dtype, const void* src, int64_t lds, void* dst, int64_t ldd, const void* wq, const void* wk,
                        const float* table, int n, int tokens, int l, int row_off, int heads, int d, float eps, void* stream) {
  return launch_qk_norm_rope(dtype, src, lds, dst, ldd, wq, wk, table, n, tokens, l, row_off, heads, d, eps, (hipStream_t)stream);
}
int smi_op_gelu_tanh_cols(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int64_t m, int c, void* stream) {
  return launch_gelu_tanh_cols(dtype, x, ldx, y, ldy, m, c, (hipStream_t)stream);
}
int smi_op_flux_unpack(int dtype, const void* rows, float* out, int n, int cout, int gh, int gw, int p, void* stream) {
  return launch_flux_unpack(dtype, rows, out, n, cout, gh, gw, p, (hipStream_t)stream);
}
int smi_op_qk_norm_rope_bwd(int dtype, const void* dj, int64_t ldd, const void* src, int64_t lds, void* dsrc, int64_t ldx,
                            const void* wq, const void* wk, const float* table, int n, int tokens, int l, int row_off, int heads,
                            int d, float eps, void* stream) {
  return launch_qk_norm_rope_bwd(dtype, dj, ldd, src, lds, dsrc, ldx, wq, wk, table, n, tokens, l, row_off, heads, d, eps,
                                 (hipStream_t)stream);
}
int smi_op_gelu_tanh_cols_bwd(int dtype, const void* x, int64_t ldx, const void* dy, int64_t ldy, void* dx, int64_t ldd, int64_t m,
                              int c, void* stream) {
  return launch_gelu_tanh_cols_bwd(dtype, x, ldx, dy, ldy, dx, ldd, m, c, (hipStream_t)stream);
}
int smi_op_flux_unpack_bwd(int dtype, const float* d_out, void* rows, int n, int cout, int gh, int gw, int p,
                           const float* scale_dev, void* stream) {
  return launch_flux_unpack_bwd(dtype, d_out, rows, n, cout, gh, gw, p, scale_dev, (hipStream_t)stream);
}
int smi_op_softmax_rows(int dtype, const float* s, void* p, int rows, int cols, float scale, void* stream) {
  return launch_softmax_rows(dtype, s, p, rows, cols, scale, (hipStream_t)stream);
}
int smi_op_chan_mix(int dtype, const float* x, const void* w, const void* b, float* y, int64_t m, int c, void* stream) {
  return launch_chan_mix(dtype, x, w, b, y, m, c, (hipStream_t)stream);
}
int smi_op_conv3x3_small(int dtype, const void* in, const void* w, const void* bias, void* out, int out_f32, int nb, int h,
                         int wd, int cin, int cout, void* stream) {
  return launch_conv3x3_small(dtype, in, w, bias, out, out_f32, nb, h, wd, cin, cout, (hipStream_t)stream);
}
int smi_op_nchw_to_nhwc(int dtype, const void* src, int src_f32, void* dst, int nb, int c, int hw, int cpad, float scale,
                        void* stream) {
  return launch_nchw_to_nhwc(dtype, src, src_f32, dst, nb, c, hw, cpad, scale, (hipStream_t)stream);
}
int smi_op_nchw_to_nhwc_scaled(int dtype, const float* src, void* dst, int nb, int c, int hw, int cpad, const float* scale_dev,
                               void* stream) {
  return launch_nchw_to_nhwc_scaled(dtype, src, dst, nb, c, hw, cpad, scale_dev, (hipStream_t)stream);
}
int smi_op_geglu(int dtype, const void* proj, void* out, const void* dout, void* dproj, int m, int c4, void* stream) {
  int rc = launch_geglu_fwd(dtype, proj, out, m, c4, (hipStream_t)stream);
  if (rc || !dout) return rc;
  return launch_geglu_bwd(dtype, proj, dout, dproj, m, c4, (hipStream_t)stream);
}
int smi_op_lora_down(int dtype, const void* x, const float* a, float* xa, int m, int k, int r, void* stream) {
  return launch_lora_down(dtype, x, k, a, k, 1, xa, r, m, k, r, (hipStream_t)stream);
}
int smi_op_lora_skinny(int dtype, const void* x, const void* s, float* out, int m, int r, int k, void* stream) {
  return launch_lora_skinny(dtype, x, k, s, out, r, m, r, k, (hipStream_t)stream);
}
int smi_op_lora_skinny_cols(int dtype, const void* x, const void* s, float* out, int m, int r, int k, const float* col_mul,
                            int ld_mul, int period, int rows_per_mul, void* stream) {
  return launch_lora_skinny_cols(dtype, x, k, s, out, r, m, r, k, col_mul, ld_mul, period, rows_per_mul, (hipStream_t)stream);
}
int smi_op_lora_wgrad(int dtype, const float* p, const void* x, float* dw, int m, int k, int r, float alpha,
                      float* scratch, void* stream) {
  // the engine's grouped reduction with a one-job table (scratch: the job's partials followed by the table itself)
  std::vector<WgradJob> jobs(1);
  WgradJob& j = jobs[0];
  memset(&j, 0, sizeof(j));
  j.conv_tap = -1;
  j.X = x;
  j.ldx = k;
  j.P = p;
  j.ldp = r;
  j.dW = dw;
  j.so_r = k;
  j.so_k = 1;
  j.M = m;
  j.K = k;
  j.r = r;
  j.rows_per_sample = m;
  j.alpha = alpha;
  wgrad_job_plan(j);
  j.partial = scratch;
  wgrad_grouped_finish(jobs);
  WgradJob* dev = reinterpret_cast<WgradJob*>(scratch + ((wgrad_job_scratch_floats(j) + 63) / 64) * 64);
  SMI_HIP(hipMemcpyAsync(dev, jobs.data(), sizeof(WgradJob), hipMemcpyHostToDevice, (hipStream_t)stream));
  return launch_lora_wgrad_grouped(dtype, jobs, dev, (hipStream_t)stream);
}

// a job table as a backward pass builds it: plan per job, partials laid out in scratch, sort + launch offsets
static int wgrad_jobs_from_c(const smi_wgrad_job* in, int n, float* scratch, std::vector<WgradJob>& jobs,
                             size_t* floats) {
  SMI_CHECK(in && n >= 1, "lora_wgrad_jobs: empty table");
  jobs.resize(n);
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    const smi_wgrad_job& s = in[i];
    SMI_CHECK(s.M >= 1 && s.K >= 8 && s.r >= 1 && s.r <= 32 && s.rows_per_sample >= 1 && s.m_begin >= 0 &&
                  s.m_begin < s.M && s.m_begin % s.rows_per_sample == 0 && (s.seg_cols == 0 || s.K % s.seg_cols == 0),
              "lora_wgrad_jobs: job %d: M=%d K=%d r=%d rows_per_sample=%d m_begin=%d seg_cols=%d", i, s.M, s.K, s.r,
              s.rows_per_sample, s.m_begin, s.seg_cols);
    WgradJob& j = jobs[i];
    memset(&j, 0, sizeof(j));
    j.X = s.X;
    j.P = s.P;
    j.dW = s.dW;
    j.row_scale = s.row_scale;
    j.ldx = s.ldx;
    j.ldp = s.ldp;
    j.so_r = s.so_r;
    j.so_k = s.so_k;
    j.M = s.M;
    j.K = s.K;
    j.r = s.r;
    j.seg_cols = s.seg_cols;
    j.rows_per_sample = s.rows_per_sample;
    j.alpha = s.alpha;
    j.m_begin = s.m_begin;
    j.conv_tap = s.conv_tap;
    j.Hin = s.Hin;
    j.Win = s.Win;
    j.Hout = s.Hout;
    j.Wout = s.Wout;
    j.conv_stride = s.conv_stride;
    j.conv_ups = s.conv_ups;
    wgrad_job_plan(j);
    j.partial = scratch ? scratch + off : nullptr;
    off += ((wgrad_job_scratch_floats(j) + 63) / 64) * 64;
  }
  *floats = off;
  return 0;
}
int smi_op_lora_wgrad_jobs_floats(const smi_wgrad_job* jobs_c, int n, size_t* out_floats) {
  std::vector<WgradJob> jobs;
  size_t part = 0;
  if (int rc = wgrad_jobs_from_c(jobs_c, n, nullptr, jobs, &part)) return rc;
  *out_floats = part + ((size_t)n * sizeof(WgradJob) + 3) / 4;
  return 0;
}
int smi_op_lora_wgrad_jobs(int dtype, const smi_wgrad_job* jobs_c, int n, float* scratch, size_t scratch_floats,
                           void* stream) {
  std::vector<WgradJob> jobs;
  size_t part = 0;
  if (int rc = wgrad_jobs_from_c(jobs_c, n, scratch, jobs, &part)) return rc;
  const size_t need = part + ((size_t)n * sizeof(WgradJob) + 3) / 4;
  SMI_CHECK(scratch && scratch_floats >= need, "lora_wgrad_jobs: scratch of %zu floats, %zu needed", scratch_floats, need);
  wgrad_grouped_finish(jobs);
  WgradJob* dev = reinterpret_cast<WgradJob*>(scratch + part);
  SMI_HIP(hipMemcpyAsync(dev, jobs.data(), (size_t)n * sizeof(WgradJob), hipMemcpyHostToDevice, (hipStream_t)stream));
  const int rc = launch_lora_wgrad_grouped(dtype, jobs, dev, (hipStream_t)stream);
  SMI_HIP(hipStreamSynchronize((hipStream_t)stream));  // the host table leaves scope
  return rc;
}

static void dora_site_from_c(const smi_dora_site& s, DoraSite& d) {
  memset(&d, 0, sizeof(d));
  d.W = s.W;
  d.off_down = s.off_down;
  d.off_up = s.off_up;
  d.off_dora = s.off_dora;
  d.dW = s.dW;
  d.dWt = s.dWt;
  d.cnorm = s.cnorm;
  d.r = s.r;
  d.nseg = s.nseg;
  d.K = s.K;
  d.cs = s.cs;
  d.scale = s.scale;
}
int smi_op_dora_prep(int dtype, const smi_dora_site* sites, int n_sites, const float* down, const float* up, float mult,
                     void* sites_dev, void* stream) {
  static_assert(sizeof(DoraSite) == sizeof(smi_dora_site), "smi_dora_site sizes the device table");
  SMI_CHECK(sites && n_sites >= 1 && sites_dev, "dora_prep: empty table");
  std::vector<DoraSite> host(n_sites);
  for (int i = 0; i < n_sites; ++i) {
    SMI_CHECK(sites[i].nseg >= 1 && sites[i].cs >= 1 && sites[i].K >= 8 && sites[i].off_down % 4 == 0,
              "dora_prep: site %d: nseg=%d cs=%d K=%d off_down=%lld", i, sites[i].nseg, sites[i].cs, sites[i].K,
              (long long)sites[i].off_down);
    dora_site_from_c(sites[i], host[i]);
  }
  DoraSite* dev = reinterpret_cast<DoraSite*>(sites_dev);
  SMI_HIP(hipMemcpyAsync(dev, host.data(), (size_t)n_sites * sizeof(DoraSite), hipMemcpyHostToDevice, (hipStream_t)stream));
  int rc = launch_dora_prep(dtype, dev, host.data(), n_sites, down, up, mult, (hipStream_t)stream);
  if (!rc) rc = launch_dora_transpose(dtype, dev, host.data(), n_sites, (hipStream_t)stream);
  SMI_HIP(hipStreamSynchronize((hipStream_t)stream));  // the host table leaves scope
  return rc;
}
int smi_op_dora_grads_floats(const smi_dora_site* site, size_t* out_floats) {
  SMI_CHECK(site && site->r >= 1 && site->nseg >= 1 && site->K >= 8, "dora_grads: bad site");
  DoraSite d;
  dora_site_from_c(*site, d);
  *out_floats = dora_grad_scratch_floats(d);
  return 0;
}
int smi_op_dora_grads(int dtype, const smi_dora_site* site, const float* G, const float* down, const float* up,
                      float* d_down, float* d_up, float alpha, const float* alpha_dev, float* scratch,
                      size_t scratch_floats, void* stream) {
  SMI_CHECK(site && site->nseg >= 1 && site->cs >= 1 && site->K >= 8 && site->K % 8 == 0 && site->off_down % 4 == 0,
            "dora_grads: bad site");
  DoraSite d;
  dora_site_from_c(*site, d);
  SMI_CHECK(scratch && scratch_floats >= dora_grad_scratch_floats(d), "dora_grads: scratch of %zu floats, %zu needed",
            scratch_floats, dora_grad_scratch_floats(d));
  return launch_dora_grads(dtype, d, G, down, up, d_down, d_up, alpha, alpha_dev, scratch, (hipStream_t)stream);
}
int smi_op_lora_prep(int dtype, const smi_lora_prep_site* sites, int n_sites, const float* down, const float* up,
                     void* shadow, void* sites_dev, void* stream) {
  static_assert(sizeof(HostLoraPrepSite) == sizeof(smi_lora_prep_site), "smi_lora_prep_site sizes the device table");
  SMI_CHECK(sites && n_sites >= 1 && sites_dev && shadow, "lora_prep: empty table");
  std::vector<HostLoraPrepSite> host(n_sites);
  for (int i = 0; i < n_sites; ++i) {
    const smi_lora_prep_site& s = sites[i];
    SMI_CHECK(s.r >= 1 && s.nseg >= 1 && s.K >= 1 && s.cs >= 1 && s.rows_pad >= s.r * s.nseg && s.conv >= 0 && s.conv <= 2 &&
                  (s.conv == 0 || s.r <= 64),
              "lora_prep: site %d: r=%d nseg=%d K=%d cs=%d rows_pad=%d conv=%d", i, s.r, s.nseg, s.K, s.cs, s.rows_pad, s.conv);
    HostLoraPrepSite& h = host[i];
    memset(&h, 0, sizeof(h));
    h.off_down = s.off_down;
    h.off_up = s.off_up;
    h.dst_down = s.dst_down;
    h.dst_up = s.dst_up;
    h.r = s.r;
    h.nseg = s.nseg;
    h.K = s.K;
    h.cs = s.cs;
    h.rows_pad = s.rows_pad;
    h.conv = s.conv;
    h.dst_gw = s.dst_gw;
  }
  SMI_HIP(hipMemcpyAsync(sites_dev, host.data(), (size_t)n_sites * sizeof(HostLoraPrepSite), hipMemcpyHostToDevice,
                         (hipStream_t)stream));
  const int rc = launch_lora_prep(dtype, sites_dev, n_sites, down, up, shadow, (hipStream_t)stream);
  SMI_HIP(hipStreamSynchronize((hipStream_t)stream));  // the host table leaves scope
  return rc;
}
int smi_op_transpose_scaled(int dtype, const void* src, int64_t lds, void* dst, int M, int C, int Mp, const float* f,
                            int rows_per_sample, void* stream) {
  return launch_transpose_scaled(dtype, src, lds, dst, M, C, Mp, f, rows_per_sample, (hipStream_t)stream);
}
int smi_op_grad_scale(const float* d_eps, int n_samples, int64_t per_sample, float* scale_out, int inv_off,
                      float* min_out, void* stream) {
  int rc = launch_grad_scale(d_eps, n_samples, per_sample, scale_out, inv_off, (hipStream_t)stream);
  if (rc) return rc;
  return launch_scale_min(scale_out, n_samples, min_out, (hipStream_t)stream);
}
int smi_op_cast_f32(int dtype, const float* src, void* dst, int64_t n, void* stream) {
  SMI_CHECK(src && dst && n > 0 && n % 8 == 0, "smi_op_cast_f32: bad arguments (n must be a multiple of 8)");
  return launch_f32_to_padded(dtype, src, 8, 8, dst, 8, n / 8, 1.f, (hipStream_t)stream);
}
int smi_op_row_scale_f32(float* x, int ld, int m, int n, const float* row_mul, int rows_per_mul, void* stream) {
  return launch_row_scale_f32(x, ld, m, n, row_mul, rows_per_mul, (hipStream_t)stream);
}

int smi_op_col_scale_f32(float* x, int ld, int m, int n, const float* col_mul, int ld_mul, int period, int rows_per_mul,
                         void* stream) {
  return launch_col_scale_f32(x, ld, m, n, col_mul, ld_mul, period, rows_per_mul, (hipStream_t)stream);
}
int smi_lora_stack(const smi_lora_stack_job* jobs, int n_jobs, void* jobs_dev, void* stream) {
  static_assert(sizeof(LoraStackJob) == sizeof(smi_lora_stack_job), "smi_lora_stack_job sizes the device table");
  SMI_CHECK(jobs && n_jobs >= 1 && jobs_dev, "lora_stack: empty table");
  std::vector<LoraStackJob> host(n_jobs);
  for (int i = 0; i < n_jobs; ++i) {
    const smi_lora_stack_job& s = jobs[i];
    SMI_CHECK(s.dst_down && s.dst_up && (s.src_down != nullptr) == (s.src_up != nullptr) && s.row_len >= 1 && s.r >= 1 &&
                  s.c0 >= 0 && s.c0 + s.r <= s.R && s.n_out >= 1,
              "lora_stack: job %d: row_len=%lld r=%d c0=%d R=%d n_out=%d", i, (long long)s.row_len, s.r, s.c0, s.R, s.n_out);
    LoraStackJob& h = host[i];
    memset(&h, 0, sizeof(h));
    h.src_down = s.src_down;
    h.src_up = s.src_up;
    h.dst_down = s.dst_down;
    h.dst_up = s.dst_up;
    h.row_len = s.row_len;
    h.r = s.r;
    h.c0 = s.c0;
    h.R = s.R;
    h.n_out = s.n_out;
    h.coef = s.coef;
  }
  SMI_HIP(hipMemcpyAsync(jobs_dev, host.data(), (size_t)n_jobs * sizeof(LoraStackJob), hipMemcpyHostToDevice, (hipStream_t)stream));
  const int rc = launch_lora_stack(reinterpret_cast<const LoraStackJob*>(jobs_dev), n_jobs, (hipStream_t)stream);
  SMI_HIP(hipStreamSynchronize((hipStream_t)stream));  // the host table leaves scope
  return rc;
}

}  // extern "C"
