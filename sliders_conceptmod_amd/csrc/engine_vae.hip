// The AutoencoderKL engines, forward only, on the op core (engine.h): the encoder and the decoder are models of their
// own that share the config struct and the code of the mid block's attention.
#include "engine.h"

namespace {

struct VLevel {
  std::vector<Resnet> res;
  bool has_samp = false;
  Conv samp;
};
// the mid block: resnet, single-head attention (its GroupNorm, fused q|k|v (+ fused bias), to_out.0), resnet
struct VaeMid {
  Resnet r0, r1;
  Norm attn_norm;
  Lin qkv, o;
};
Resnet vae_resnet(smi_engine& e, const smi_vae_config& c, const std::string& name, int Cin, int Cout) {
  return e.make_resnet(name, Cin, Cout, c.norm_num_groups, 0, 1e-6f, false);
}
void build_vae_attn(smi_engine& e, VaeMid& m, const std::string& pre, int ch, int groups) {
  m.attn_norm = e.make_norm(pre + ".group_norm", ch, 1e-6f, groups);
  m.qkv = e.make_fused(pre, {"to_q", "to_k", "to_v"}, ch, ch, false);
  m.qkv.b = e.fused_bias(pre, {"to_q", "to_k", "to_v"}, ch);
  m.o = e.make_lin(pre + ".to_out.0", ch, ch, true, false);
}
void build_vae_mid(smi_engine& e, VaeMid& m, const smi_vae_config& c, const std::string& pre, int ch) {
  m.r0 = vae_resnet(e, c, pre + ".resnets.0", ch, ch);
  build_vae_attn(e, m, pre + ".attentions.0", ch, c.norm_num_groups);
  m.r1 = vae_resnet(e, c, pre + ".resnets.1", ch, ch);
}
// single-head attention over the pixels, with its own GroupNorm and residual: ONE head of width 512 over all pixels, run
// as materialised GEMMs, a few GFLOP per image.  Per image: S = Q K^T (fp32), P = softmax(S / sqrt(C)), O = P V.
// `hoist`: one set of per-image buffers (S, P, K, V^T) for all images (the decoder); otherwise each image allocates its
// own (the encoder's layout, kept as it was)
Ten* vae_attn(smi_engine& e, const VaeMid& m, Ten* h, bool hoist) {
  const int n = h->n;
  const int C = h->cols, N = h->H * h->W;
  Ten* nrm = e.groupnorm(h, m.attn_norm, false);
  Ten* qkv = e.linear(nrm, m.qkv);
  Ten* o = e.new_ten(h->rows, C, h->n, h->H, h->W);
  const float sc = 1.f / sqrtf((float)C);
  float* S = nullptr;
  void *P = nullptr, *Vt = nullptr, *Kd = nullptr, *Vd = nullptr;
  if (hoist) {
    S = e.alloc_f32((size_t)N * N);
    P = e.alloc_t(N, N);
    Vt = e.alloc_t(C, N);
    Kd = e.alloc_t(N, C);
    Vd = e.alloc_t(N, C);
  }
  for (int i = 0; i < n; ++i) {
    const char* base = (const char*)qkv->p + (size_t)i * N * 3 * C * e.esz();
    if (!hoist) {
      S = e.alloc_f32((size_t)N * N);
      P = e.alloc_t(N, N);
      Vt = e.alloc_t(C, N);
    }
    // the GEMM's W operand is dense [N_out, K]: K (and V) are column blocks of the fused tensor, so stage them
    if (!hoist) Kd = e.alloc_t(N, C);
    RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_copy_cols(e.dtype, base + (size_t)C * e.esz(), 3 * C, Kd, C, 0, N, C, e.stream));
    e.run_gemm(SMI_PROF_ATTN, gemm_nt(e.dtype, base, 3 * C, Kd, S, N, N, N, C).f32_out(), 2.0 * N * N * C, 0.0, false,
               "vae_attn QK^T");
    RUNP(SMI_PROF_ATTN, 0.0, 0.0, launch_softmax_rows(e.dtype, S, P, N, N, sc, e.stream));
    if (!hoist) Vd = e.alloc_t(N, C);
    RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_copy_cols(e.dtype, base + (size_t)2 * C * e.esz(), 3 * C, Vd, C, 0, N, C, e.stream));
    e.transpose_into(Vd, Vt, N, C, N, 0, false);
    e.run_gemm(SMI_PROF_ATTN, gemm_nt(e.dtype, P, N, Vt, (char*)o->p + (size_t)i * N * C * e.esz(), C, N, C, N),
               2.0 * N * N * C, 0.0, false, "vae_attn PV");
  }
  return e.linear(o, m.o, h);
}
Ten* vae_mid(smi_engine& e, const VaeMid& m, Ten* h, bool hoist) {
  h = e.resnet(h, m.r0, nullptr, 0);
  h = vae_attn(e, m, h, hoist);
  return e.resnet(h, m.r1, nullptr, 0);
}

// ---------------------------------------------------------------------------------------------------------
// AutoencoderKL encoder (image sliders: I/train_util.py:213-222 `vae.encode(image).latent_dist`).
// Same kernels as the UNet: GroupNorm(+SiLU), implicit-GEMM 3x3 convs (the downsampler with its (0,1,0,1) padding as
// `pad = 0`), 1x1 shortcuts as GEMMs.
// ---------------------------------------------------------------------------------------------------------
struct VaeEncoder : Model {
  smi_vae_config cfg{};
  int img_h = 0, img_w = 0;
  Conv conv_in, conv_out;
  std::vector<VLevel> down;
  VaeMid mid;
  Norm norm_out;
  const void* quant_w = nullptr;
  const void* quant_b = nullptr;
  VaeEncoder(const smi_vae_config& c, int h, int w) : cfg(c), img_h(h), img_w(w) {}

  void build(smi_engine& e) override {
    const int L = cfg.n_levels;
    const int* boc = cfg.block_out_channels;
    conv_in = e.make_conv_in("encoder.conv_in", cfg.in_channels, boc[0]);
    down.resize(L);
    int ch = boc[0];
    for (int i = 0; i < L; ++i) {
      const std::string b = "encoder.down_blocks." + std::to_string(i);
      for (int j = 0; j < cfg.layers_per_block; ++j)
        down[i].res.push_back(vae_resnet(e, cfg, b + ".resnets." + std::to_string(j), j == 0 ? ch : boc[i], boc[i]));
      ch = boc[i];
      down[i].has_samp = i != L - 1;
      if (down[i].has_samp) {
        down[i].samp = e.make_conv(b + ".downsamplers.0.conv", ch, ch, 1, false);
        down[i].samp.pad = 0;
      }
    }
    build_vae_mid(e, mid, cfg, "encoder.mid_block", ch);
    norm_out = e.make_norm("encoder.conv_norm_out", ch, 1e-6f, cfg.norm_num_groups);
    conv_out = e.make_conv("encoder.conv_out", ch, 2 * cfg.latent_channels, 0, false);
    quant_w = e.Wd("quant_conv.weight");
    quant_b = e.Wd("quant_conv.bias");
    e.check_shape("quant_conv.weight", {2 * cfg.latent_channels, 2 * cfg.latent_channels, 1, 1});
  }
  void dry_forward(smi_engine& e) override { forward(e, e.max_n, nullptr, nullptr); }

  // image f32 [n, 3, h, w] in [-1, 1]  ->  moments f32 [n, 2 * latent, h/8, w/8] (mean | logvar, before the clamp)
  int forward(smi_engine& e, int n, const float* image, float* moments_out) {
    e.begin_forward_only_pass();
    Ten* x0 = e.new_ten((int64_t)n * img_h * img_w, 64, n, img_h, img_w);
    RUN(launch_nchw_to_nhwc(e.dtype, image, 1, x0->p, n, cfg.in_channels, img_h * img_w, 64, 1.f, e.stream));
    Ten* h = e.conv3x3(x0, conv_in, nullptr, nullptr);
    for (auto& lv : down) {
      for (auto& r : lv.res) h = e.resnet(h, r, nullptr, 0);
      if (lv.has_samp) h = e.conv3x3(h, lv.samp, nullptr, nullptr);
    }
    h = vae_mid(e, mid, h, false);
    Ten* hn = e.groupnorm(h, norm_out, true);
    const int C2 = 2 * cfg.latent_channels;
    const int Ho = hn->H, Wo = hn->W;
    Ten* y = e.new_ten((int64_t)n * Ho * Wo, C2, n, Ho, Wo, sizeof(float));
    {
      const GemmParams p =
          conv3x3_fwd(e.dtype, hn->p, conv_out.Wp, y->p, n, Ho, Wo, conv_out.Cin, C2).f32_out().with_bias(conv_out.b);
      e.run_gemm(SMI_PROF_CONV, p, smi_engine::gemm_flops(p), 0.0, false, "vae conv_out");
    }
    float* q = e.alloc_f32((size_t)y->rows * C2);
    RUN(launch_chan_mix(e.dtype, (const float*)y->p, quant_w, quant_b, q, y->rows, C2, e.stream));
    RUN(launch_nhwc_to_nchw_f32(q, moments_out, n, C2, Ho * Wo, e.stream));
    return e.end_pass("this call (");
  }
};

// ---------------------------------------------------------------------------------------------------------
// AutoencoderKL decoder (what the eval scripts do after the sweep: `vae.decode(latents / scaling_factor).sample`,
// eval-scripts/generate_images_sd1.py:195-200): post_quant_conv (1x1, fp32 on the latent grid) -> conv_in -> mid block
// (resnet, single-head attention, resnet) -> up blocks over the reversed block_out_channels (layers_per_block + 1
// resnets, nearest-2x + 3x3 up-sampler on all but the last) -> conv_norm_out + SiLU + conv_out.  The tail runs as one
// fused launch (vae_decode.hip) unless SMI_VAE_DEC_TAIL=0 (then: GroupNorm+SiLU, the conv with Cout padded to 4 by a
// zero filter row, layout kernels, a separate uint8 pass).  The engine's `kind` tells decoder and encoder apart:
// encode / decode refuse the other kind, the UNet entry points refuse both.
// ---------------------------------------------------------------------------------------------------------
struct VaeDecoder : Model {
  smi_vae_config cfg{};
  int img_h = 0, img_w = 0;
  bool tail_fused = true;
  Conv conv_in;
  VaeMid mid;
  std::vector<VLevel> up;
  Norm norm_out;
  Conv conv_out;                 // Wp: [4][9*C0], rows >= out channels zero
  const void* bias4 = nullptr;   // conv_out bias zero-padded to 4 (unfused path)
  const void* pq_w = nullptr;    // post_quant_conv
  const void* pq_b = nullptr;
  VaeDecoder(const smi_vae_config& c, int h, int w) : cfg(c), img_h(h), img_w(w) {
    const char* t = getenv("SMI_VAE_DEC_TAIL");
    tail_fused = !(t && t[0] == '0');
  }

  void build(smi_engine& e) override {
    const int L = cfg.n_levels;
    const int* boc = cfg.block_out_channels;
    const int lc = cfg.latent_channels, co = cfg.in_channels;
    if (!cfg.no_post_quant_conv) {
      pq_w = e.Wd("post_quant_conv.weight");
      pq_b = e.Wd("post_quant_conv.bias");
      e.check_shape("post_quant_conv.weight", {lc, lc, 1, 1});
      e.check_shape("post_quant_conv.bias", {lc});
    }
    const int top = boc[L - 1];
    conv_in = e.make_conv_in("decoder.conv_in", lc, top);
    build_vae_mid(e, mid, cfg, "decoder.mid_block", top);
    up.resize(L);
    int ch = top;
    for (int i = 0; i < L; ++i) {
      const int out = boc[L - 1 - i];
      const std::string b = "decoder.up_blocks." + std::to_string(i);
      for (int j = 0; j <= cfg.layers_per_block; ++j)
        up[i].res.push_back(vae_resnet(e, cfg, b + ".resnets." + std::to_string(j), j == 0 ? ch : out, out));
      ch = out;
      up[i].has_samp = i != L - 1;
      if (up[i].has_samp) up[i].samp = e.make_conv(b + ".upsamplers.0.conv", ch, ch, 2, false);
    }
    norm_out = e.make_norm("decoder.conv_norm_out", ch, 1e-6f, cfg.norm_num_groups);
    {  // conv_out [co][9*C0] with co padded to 4 by zero rows: the fused tail's B operand and the unfused conv's filter
      conv_out.Cin = ch;
      conv_out.Cout = 4;
      conv_out.b = e.Wd("decoder.conv_out.bias");
      e.check_shape("decoder.conv_out.weight", {co, ch, 3, 3});
      e.check_shape("decoder.conv_out.bias", {co});
      void* wp = e.pack_alloc((size_t)4 * 9 * ch * e.esz());
      void* b4 = e.pack_alloc(4 * e.esz());
      if (!e.dry && !e.err) {
        (void)hipMemsetAsync(wp, 0, (size_t)4 * 9 * ch * e.esz(), e.stream);
        (void)hipMemsetAsync(b4, 0, 4 * e.esz(), e.stream);
        if (conv_out.b)
          (void)hipMemcpyAsync(b4, conv_out.b, (size_t)co * e.esz(), hipMemcpyDeviceToDevice, e.stream);
      }
      e.pack_conv_into(e.Wd("decoder.conv_out.weight"), wp, co, ch, 0);
      conv_out.Wp = wp;
      bias4 = b4;
    }
  }
  void dry_forward(smi_engine& e) override { forward(e, e.max_n, nullptr, nullptr, nullptr); }

  // latents f32 [n, latent, h/f, w/f] (already / scaling_factor) -> image f32 [n, 3, h, w] (+ uint8 [n, h, w, 3])
  int forward(smi_engine& e, int n, const float* latents, float* image_out, uint8_t* rgb8_out) {
    e.begin_forward_only_pass();
    const int L = cfg.n_levels, f = 1 << (L - 1);
    const int H = img_h, Wd_ = img_w;
    const int h0 = H / f, w0 = Wd_ / f, lc = cfg.latent_channels, co = cfg.in_channels;
    const int64_t M0 = (int64_t)n * h0 * w0;
    float* zt = e.alloc_f32((size_t)M0 * lc);
    // NCHW -> NHWC: the NHWC -> NCHW kernel with the roles of C and HW swapped
    RUN(launch_nhwc_to_nchw_f32(latents, zt, n, h0 * w0, lc, e.stream));
    float* zq = zt;  // (a VAE without post_quant_conv: SD3's)
    if (!cfg.no_post_quant_conv) {
      zq = e.alloc_f32((size_t)M0 * lc);
      RUN(launch_chan_mix(e.dtype, zt, pq_w, pq_b, zq, M0, lc, e.stream));
    }
    Ten* x0 = e.new_ten(M0, 64, n, h0, w0);
    RUN(launch_f32_to_padded(e.dtype, zq, lc, lc, x0->p, 64, M0, 1.f, e.stream));
    Ten* h = e.conv3x3(x0, conv_in, nullptr, nullptr);
    h = vae_mid(e, mid, h, true);
    for (auto& lv : up) {
      for (auto& r : lv.res) h = e.resnet(h, r, nullptr, 0);
      if (lv.has_samp) h = e.conv3x3(h, lv.samp, nullptr, nullptr);
    }
    const int C0 = h->cols, HWi = H * Wd_, G = cfg.norm_num_groups;
    if (tail_fused) {
      float* ab = e.alloc_f32((size_t)2 * n * C0);
      float* mr = e.alloc_f32((size_t)n * G * 2);
      float* part = e.alloc_f32(gn_partial_floats(n, HWi, G));
      RUNP(SMI_PROF_NORM, 0.0, 2.0 * h->rows * C0,
           launch_groupnorm_stats(e.dtype, h->p, norm_out.gamma, norm_out.beta, ab, mr, part, n, HWi, C0, G, norm_out.eps,
                                  e.stream));
      RUNP(SMI_PROF_CONV, 2.0 * h->rows * co * 9 * C0, 2.0 * h->rows * C0 + 4.0 * h->rows * co + (rgb8_out ? 1.0 * h->rows * co : 0.0),
           launch_vae_dec_tail(e.dtype, h->p, ab, conv_out.Wp, conv_out.b, image_out, rgb8_out, n, H, Wd_, C0, co, e.stream));
    } else {
      Ten* hn = e.groupnorm(h, norm_out, true);
      Ten* y = e.new_ten((int64_t)n * HWi, 4, n, H, Wd_, sizeof(float));
      const GemmParams p = conv3x3_fwd(e.dtype, hn->p, conv_out.Wp, y->p, n, H, Wd_, C0, 4).f32_out().with_bias(bias4);
      e.run_gemm(SMI_PROF_CONV, p, smi_engine::gemm_flops(p), 0.0, false, "vae_dec conv_out");
      float* t4 = e.alloc_f32((size_t)n * 4 * HWi);
      RUN(launch_nhwc_to_nchw_f32((const float*)y->p, t4, n, 4, HWi, e.stream));
      RUN(hipMemcpy2DAsync(image_out, (size_t)co * HWi * sizeof(float), t4, (size_t)4 * HWi * sizeof(float),
                           (size_t)co * HWi * sizeof(float), n, hipMemcpyDeviceToDevice, e.stream) == hipSuccess ? 0 : -1);
      if (rgb8_out) RUN(launch_rgb8_from_nchw(image_out, rgb8_out, n, co, HWi, e.stream));
    }
    return e.end_pass("this call (");
  }
};

int check_vae_cfg(const smi_vae_config* c, int batch, int h, int w, int max_latent = 8) {
  SMI_CHECK(c != nullptr, "config is NULL");
  SMI_CHECK(c->dtype == SMI_DTYPE_F16 || c->dtype == SMI_DTYPE_BF16, "dtype must be f16 (0) or bf16 (1)");
  SMI_CHECK(c->n_levels >= 1 && c->n_levels <= SMI_MAX_LEVELS && c->in_channels >= 1 && c->in_channels <= 16 &&
                c->latent_channels >= 1 && c->latent_channels <= max_latent && c->layers_per_block >= 1,
            "VAE config out of range");
  for (int i = 0; i < c->n_levels; ++i)
    SMI_CHECK(c->block_out_channels[i] % 64 == 0 && c->block_out_channels[i] % c->norm_num_groups == 0,
              "VAE block_out_channels must be multiples of 64 and of norm_num_groups");
  const int f = 1 << (c->n_levels - 1);
  SMI_CHECK(batch > 0 && h > 0 && w > 0 && h % f == 0 && w % f == 0, "image size must be a multiple of %d", f);
  return 0;
}
template <class M>  // VaeEncoder or VaeDecoder
Setup vae_setup(smi_engine::Kind kind, const smi_vae_config* cfg, int batch, int h, int w) {
  return [=](smi_engine* e) { e->hold(kind, new M(*cfg, h, w), cfg->dtype, batch); };
}

// largest 16-bit conv / GEMM operand (input or output) of ONE image: the GEMM addresses each operand with a 32-bit byte
// offset (gemm.hip: "larger than 4 GiB"), so batch x this must stay below that
int64_t vae_dec_image_operand_bytes(const smi_vae_config* c, int h, int w) {
  const int L = c->n_levels, f = 1 << (L - 1);
  int64_t hw = (int64_t)(h / f) * (w / f), m = hw * 64;
  int ch = c->block_out_channels[L - 1];
  m = std::max(m, hw * ch);
  for (int i = 0; i < L; ++i) {
    const int out = c->block_out_channels[L - 1 - i];
    m = std::max(m, hw * std::max(ch, out));  // first resnet reads ch, the shortcut writes out
    ch = out;
    if (i != L - 1) {
      hw *= 4;
      m = std::max(m, hw * ch);  // the up-sampler's output
    }
  }
  return m * 2;
}
int check_vae_dec_cfg(const smi_vae_config* c, int batch, int h, int w) {
  if (check_vae_cfg(c, batch, h, w, 16)) return -1;  // 16: SD3's latents (the 1x1 post_quant_conv kernel takes up to 16)
  SMI_CHECK(c->in_channels <= 4, "VAE decoder: %d image channels (the fused conv_out takes at most 4)", c->in_channels);
  SMI_CHECK(c->block_out_channels[0] <= 512, "VAE decoder: block_out_channels[0] = %d > 512", c->block_out_channels[0]);
  SMI_CHECK(w % 4 == 0, "VAE decoder: image width %d must be a multiple of 4", w);
  const int f = 1 << (c->n_levels - 1);
  const int64_t na = (int64_t)(h / f) * (w / f);
  SMI_CHECK(na * na * 4 < 0xFFFFFFF0ll, "VAE decoder: %dx%d is too large for the materialised mid-block attention "
            "(%lld latent pixels)", h, w, (long long)na);
  const int64_t per = vae_dec_image_operand_bytes(c, h, w);
  const int64_t maxb = (0xFFFFFFF0ll - 1) / per;
  SMI_CHECK(batch <= maxb, "VAE decoder: batch %d at %dx%d crosses the GEMM's 4 GiB operand limit (%lld MiB per image); "
            "the largest batch that fits is %lld", batch, h, w, (long long)(per >> 20), (long long)maxb);
  return 0;
}

}  // namespace

extern "C" {

// ---- AutoencoderKL encoder engine ------------------------------------------------------------------------------------
int smi_vae_workspace_bytes(const smi_vae_config* cfg, int batch, int h, int w, size_t* bytes) {
  if (check_vae_cfg(cfg, batch, h, w)) return -1;
  return workspace_bytes_forward_only(vae_setup<VaeEncoder>(smi_engine::VAE_ENCODER, cfg, batch, h, w), bytes);
}

int smi_vae_create(const smi_vae_config* cfg, const smi_weight* weights, int n_weights, int batch, int h, int w,
                   void* workspace, size_t workspace_bytes, void* stream, smi_engine** out) {
  if (check_vae_cfg(cfg, batch, h, w)) return -1;
  return create_forward_only(vae_setup<VaeEncoder>(smi_engine::VAE_ENCODER, cfg, batch, h, w),
                             "the VAE weights", weights, n_weights, workspace, workspace_bytes, stream, out);
}

int smi_vae_encode(smi_engine* e, int n, const float* image, float* moments_out) {
  SMI_CHECK(e && image && moments_out && (e->kind == smi_engine::VAE_ENCODER || e->kind == smi_engine::VAE_DECODER),
            "smi_vae_encode: NULL argument or not a VAE engine");
  SMI_CHECK(e->kind == smi_engine::VAE_ENCODER, "smi_vae_encode: this engine is a VAE decoder (use smi_vae_decode)");
  SMI_CHECK(n >= 1 && n <= e->max_n, "batch %d outside [1, %d] the engine was created for", n, e->max_n);
  e->err = false;
  return static_cast<VaeEncoder*>(e->model.get())->forward(*e, n, image, moments_out);
}

// ---- AutoencoderKL decoder engine ------------------------------------------------------------------------------------
int smi_vae_decoder_workspace_bytes(const smi_vae_config* cfg, int batch, int h, int w, size_t* bytes) {
  if (check_vae_dec_cfg(cfg, batch, h, w)) return -1;
  return workspace_bytes_forward_only(vae_setup<VaeDecoder>(smi_engine::VAE_DECODER, cfg, batch, h, w), bytes);
}

int smi_vae_decoder_create(const smi_vae_config* cfg, const smi_weight* weights, int n_weights, int batch, int h, int w,
                           void* workspace, size_t workspace_bytes, void* stream, smi_engine** out) {
  if (check_vae_dec_cfg(cfg, batch, h, w)) return -1;
  return create_forward_only(vae_setup<VaeDecoder>(smi_engine::VAE_DECODER, cfg, batch, h, w),
                             "the VAE decoder weights", weights, n_weights, workspace, workspace_bytes, stream, out);
}

int smi_vae_decode(smi_engine* e, int n, const float* latents, float* image_out, uint8_t* rgb8_out) {
  SMI_CHECK(e && latents && image_out, "smi_vae_decode: NULL argument");
  SMI_CHECK(e->kind == smi_engine::VAE_DECODER, "smi_vae_decode: not a VAE decoder engine (create it with smi_vae_decoder_create)");
  SMI_CHECK(n >= 1 && n <= e->max_n, "batch %d outside [1, %d] the engine was created for", n, e->max_n);
  e->err = false;
  return static_cast<VaeDecoder*>(e->model.get())->forward(*e, n, latents, image_out, rgb8_out);
}

}  // extern "C"
