// The UNet2DCondition model on the op core (engine.h): the SD-1.x / SD-XL denoising forward with its tape, the
// activation / LoRA-gradient backward, the planner of its two arenas, and the C entry points of the UNet engine.
#include "engine.h"

namespace {

// the column table of a slider stack, rows [row0, row0 + rows) of dst [.][ld]: column c of sample i gets the multiplier of
// the slider that owns rank column c (sliders in order, ranks.v[k] columns each); a.v = multipliers[rows][n_sliders]
struct I16Args {
  int v[16];
};
__global__ void col_table_kernel(float* dst, int ld, int row0, int rows, int n_sliders, I16Args ranks, F64Args a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * ld) return;
  const int s = i / ld, c = i - s * ld;
  int k = 0, end = ranks.v[0];
  while (c >= end && k + 1 < n_sliders) end += ranks.v[++k];
  dst[(int64_t)(row0 + s) * ld + c] = a.v[s * n_sliders + k];
}
__global__ void fill_kernel(float* p, float v, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// columns [col0, col0 + cols) of w [rows][ld] times s, a power of two (exact): a block of a packed weight copy
template <typename T>
__global__ void scale_cols_kernel(T* w, int ld, int rows, int col0, int cols, float s) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)rows * cols) return;
  const int64_t r = i / cols, c = i - r * cols;
  T* p = w + r * ld + col0 + c;
  *p = from_f<T>(to_f(*p) * s);
}

struct TBlock {
  Norm n1, n2, n3;
  Lin qkv1, out1, q2, kv2, out2, ff1, ff2;
  int64_t kv_col = 0;  // column offset of this block's k|v inside the grouped projection
};
struct Transformer {
  Norm norm;
  Lin proj_in, proj_out;
  std::vector<TBlock> blocks;
  int heads = 0, C = 0;
};
struct Level {
  std::vector<Resnet> res;
  std::vector<Transformer> att;
  bool has_att = false;
  bool has_samp = false;
  Conv samp;
};

struct UNet : Model {
  smi_unet_config cfg{};
  int max_n_ad = 0, lat_h = 0, lat_w = 0, ctx_len = 0;  // the shape the arenas are planned for (max_n: in the engine)
  static constexpr size_t SPLITK_WS_BYTES = (size_t)512 * 128 * 128 * sizeof(float);  // 33.5 MB
  void* splitk_ws = nullptr;
  char* arena_home = nullptr;  // the arena region inside the creation workspace (smi_replan with arena == NULL)
  size_t arena_home_bytes = 0;
  // grouped cross-attention K|V projection: every block's to_k|to_v stacked into one [sum N, D_ctx] matrix
  Lin kv_all;
  bool kv_grouped = false;
  bool kv_adapted = false;  // some to_k / to_v carries an adaptor: its weight gradient reads the context itself
  Ten* kv_all_out = nullptr;
  // gradient with respect to the context (smi_unet_ctx_grad_*, smi_unet_backward_ctx).  The transposed k|v weights it needs
  // and the larger saved-pass arena live in a buffer of the caller's (`xpack` + arena 1), so that engines that never ask
  // keep today's workspace.  ctx_cap: that buffer is attached; ctx_want: saving forwards differentiate the context;
  // bw_ctx: the saved pass does.  The backward's output is the engine's fp32 sink (smi_engine::d_ctx, [adapted rows, D]).
  Arena xpack;
  bool ctx_cap = false, ctx_want = false, bw_ctx = false;
  void build_ctx_grad(smi_engine& e) {
    const int D = cfg.cross_attention_dim;
    xpack.reset();
    auto transposed = [&](Lin& L) {
      void* t = xpack.alloc((size_t)L.out * D * e.esz());
      e.transpose_into(L.W, t, L.out, D, L.out, 0);
      L.Wt = t;
    };
    if (kv_grouped) transposed(kv_all);  // [D, sum N]: the K-contiguous operand of d_ctx = dKV_all W_all
    else for_each_tblock([&](TBlock& tb) { transposed(tb.kv2); });
  }
  Lin temb_all;  // every resnet's time_emb_proj stacked (they all read silu(emb)): one GEMM per pass
  bool temb_grouped = false;
  Ten* temb_all_out = nullptr;
  // gradient with respect to the pooled embedding text_embeds (smi_unet_pooled_grad_*, smi_unet_backward_cond): on top of
  // the context gradient.  The chain has no trainable weight on it: text_embeds -> cat[:, :P] -> add_embedding.linear_1 ->
  // SiLU -> linear_2 -> (+ time embedding) -> SiLU -> every resnet's time_emb_proj -> added to every pixel of conv1's
  // output.  Backward: every resnet's column sum of d(conv1 output) lands in its column block of ONE 16-bit gradient of
  // the grouped projection, [adapted samples, sum C]; one fp32-output GEMM against the transposed grouped weight adds all
  // the terms in one fp32 accumulation, and the rest of the chain stays in fp32 (launch_silu_bwd_f32, launch_vecmat_f32).
  // Block b's sums are stored x 2^-k_b (Ten::gmul, k_b from its map size): the transposed copy of its weight rows is
  // built x 2^k_b -- exact, a power of two -- so the product is the unscaled sum whatever mix of levels K runs over.  That
  // copy and the (again larger) saved-pass arena live in one more buffer of the caller's (`tpack` + arena 1).
  Arena tpack;
  bool pool_cap = false, pool_want = false, bw_pool = false;
  float* d_pooled = nullptr;  // the output of the backward in flight, fp32 [adapted samples, P]
  bool d_pooled_written = false;
  int pooled_dim() const { return cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim; }
  // every resnet with the pixels of the map its conv1 writes, for the engine's current latent shape
  template <typename F>
  void for_each_resnet_hw(F f) {
    int h = lat_h, w = lat_w;
    for (auto& lv : down) {
      for (auto& r : lv.res) f(r, h * w);
      if (lv.has_samp) h = conv3x3_out(h, 1), w = conv3x3_out(w, 1);
    }
    for (auto& r : mid.res) f(r, h * w);
    for (auto& lv : up) {
      for (auto& r : lv.res) f(r, h * w);
      if (lv.has_samp) h = conv3x3_out(h, 2), w = conv3x3_out(w, 2);
    }
  }
  // why this engine has no pooled-embedding gradient (nullptr: it has one); an adaptor on a time_emb_proj is named
  const char* pooled_refusal(std::string& site) {
    if (!cfg.addition_embed) return "this UNet has no added conditioning (addition_embed): there is no pooled embedding to differentiate";
    if (temb_grouped) return nullptr;
    for_each_resnet([&](Resnet& r) {
      if (site.empty() && r.temb.nsite > 0) site = r.temb.name;
    });
    return site.empty() ? "it needs the grouped time_emb_proj projection, which is off (SMI_TEMB_GROUP=0)"
                        : "not implemented through an adaptor on a time_emb_proj";
  }
  int build_pooled_grad(smi_engine& e) {
    std::string site;
    if (const char* why = pooled_refusal(site)) {
      set_error("pooled-embedding gradient: %s%s%s", why, site.empty() ? "" : ": ", site.c_str());
      return -1;
    }
    tpack.reset();
    const int ted = temb_all.in, SC = temb_all.out;
    void* t = tpack.alloc((size_t)ted * SC * e.esz());
    e.transpose_into(temb_all.W, t, SC, ted, SC, 0, false);  // [ted, sum C]: the K-contiguous operand of d(temb_act) = G W_all
    for_each_resnet_hw([&](Resnet& r, int hw) {
      const int k = smi_engine::rowvec_shift(hw);
      if (k == 0 || e.dry || e.err) return;
      const int64_t total = (int64_t)ted * r.temb.out;
      const int grid = (int)((total + 255) / 256);
      if (e.dtype == DT_F16)
        hipLaunchKernelGGL(scale_cols_kernel<f16>, dim3(grid), dim3(256), 0, e.stream, (f16*)t, SC, ted, (int)r.temb_col, r.temb.out, exp2f((float)k));
      else
        hipLaunchKernelGGL(scale_cols_kernel<bf16>, dim3(grid), dim3(256), 0, e.stream, (bf16*)t, SC, ted, (int)r.temb_col, r.temb.out, exp2f((float)k));
    });
    temb_all.Wt = t;
    return 0;
  }

  // model
  Conv conv_in, conv_out;
  Norm norm_out;
  Lin time1, time2, add1, add2;
  std::vector<Level> down, up;
  Level mid;
  // every saved forward gets a generation number; the caller keeps it with the output it will differentiate and
  // smi_unet_backward_checked refuses a stale one (a later saved forward, a replan or a backward dropped the tape)
  uint64_t tape_gen = 0;
  int64_t replans = 0;
  Ten* out_ten = nullptr;  // conv_out result (f32 [rows, 4])

  Transformer make_transformer(smi_engine& e, const std::string& name, int C, int heads, int layers) {
    Transformer t;
    t.C = C;
    t.heads = heads;
    t.norm = e.make_norm(name + ".norm", C, 1e-6f, cfg.norm_num_groups);
    t.proj_in = e.make_lin(name + ".proj_in", C, C, true);
    for (int k = 0; k < layers; ++k) {
      const std::string b = name + ".transformer_blocks." + std::to_string(k);
      TBlock tb;
      tb.n1 = e.make_norm(b + ".norm1", C, 1e-5f, 0);
      tb.qkv1 = e.make_fused(b + ".attn1", {"to_q", "to_k", "to_v"}, C, C, true);
      tb.out1 = e.make_lin(b + ".attn1.to_out.0", C, C, true);
      tb.n2 = e.make_norm(b + ".norm2", C, 1e-5f, 0);
      tb.q2 = e.make_lin(b + ".attn2.to_q", C, C, false);
      tb.kv2 = e.make_fused(b + ".attn2", {"to_k", "to_v"}, cfg.cross_attention_dim, C, false);
      tb.out2 = e.make_lin(b + ".attn2.to_out.0", C, C, true);
      tb.n3 = e.make_norm(b + ".norm3", C, 1e-5f, 0);
      tb.ff1 = e.make_lin(b + ".ff.net.0.proj", C, 8 * C, true);
      tb.ff2 = e.make_lin(b + ".ff.net.2", 4 * C, C, true);
      t.blocks.push_back(tb);
    }
    t.proj_out = e.make_lin(name + ".proj_out", C, C, true);
    return t;
  }

  void build(smi_engine& e) override {
    const int L = cfg.n_levels;
    const int* boc = cfg.block_out_channels;
    const int ted = boc[0] * 4, G = cfg.norm_num_groups;
    conv_in = e.make_conv_in("conv_in", cfg.in_channels, boc[0]);
    time1 = e.make_lin("time_embedding.linear_1", boc[0], ted, true, false);
    time2 = e.make_lin("time_embedding.linear_2", ted, ted, true, false);
    if (cfg.addition_embed) {
      add1 = e.make_lin("add_embedding.linear_1", cfg.projection_class_embeddings_input_dim, ted, true, false);
      add2 = e.make_lin("add_embedding.linear_2", ted, ted, true, false);
    }
    int out_ch = boc[0];
    down.resize(L);
    for (int i = 0; i < L; ++i) {
      const int in_ch = out_ch;
      out_ch = boc[i];
      Level& lv = down[i];
      lv.has_att = cfg.down_has_attn[i] != 0;
      const std::string b = "down_blocks." + std::to_string(i);
      for (int j = 0; j < cfg.layers_per_block; ++j) {
        lv.res.push_back(e.make_resnet(b + ".resnets." + std::to_string(j), j == 0 ? in_ch : out_ch, out_ch, G, ted));
        if (lv.has_att)
          lv.att.push_back(make_transformer(e, b + ".attentions." + std::to_string(j), out_ch, cfg.num_heads[i],
                                            cfg.transformer_layers[i]));
      }
      lv.has_samp = i != L - 1;
      if (lv.has_samp) lv.samp = e.make_conv(b + ".downsamplers.0.conv", out_ch, out_ch, 1, true);
    }
    {
      const int ch = boc[L - 1];
      mid.res.push_back(e.make_resnet("mid_block.resnets.0", ch, ch, G, ted));
      mid.att.push_back(make_transformer(e, "mid_block.attentions.0", ch, cfg.num_heads[L - 1],
                                         cfg.mid_transformer_layers));
      mid.res.push_back(e.make_resnet("mid_block.resnets.1", ch, ch, G, ted));
    }
    up.resize(L);
    out_ch = boc[L - 1];
    for (int i = 0; i < L; ++i) {
      const int prev = out_ch;
      out_ch = boc[L - 1 - i];
      const int in_ch = boc[L - 1 - std::min(i + 1, L - 1)];
      Level& lv = up[i];
      lv.has_att = cfg.up_has_attn[i] != 0;
      const std::string b = "up_blocks." + std::to_string(i);
      const int nl = cfg.layers_per_block + 1;
      for (int j = 0; j < nl; ++j) {
        const int skip = j == nl - 1 ? in_ch : out_ch;
        const int rin = j == 0 ? prev : out_ch;
        lv.res.push_back(e.make_resnet(b + ".resnets." + std::to_string(j), rin + skip, out_ch, G, ted));
        if (lv.has_att)
          lv.att.push_back(make_transformer(e, b + ".attentions." + std::to_string(j), out_ch,
                                            cfg.num_heads[L - 1 - i], cfg.transformer_layers[L - 1 - i]));
      }
      lv.has_samp = i != L - 1;
      // (phase form: the up-sampler's output goes to the next level's first concat and nowhere else, see forward)
      if (lv.has_samp) lv.samp = e.make_conv(b + ".upsamplers.0.conv", out_ch, out_ch, 2, true, true);
    }
    norm_out = e.make_norm("conv_norm_out", boc[0], 1e-5f, G);
    conv_out = e.make_conv("conv_out", boc[0], cfg.out_channels, 0, false);
    {  // conv_out gradient filter [C0][9*64]: flipped taps, d_eps channels zero-padded to 64 (MFMA conv path)
      void* wg = e.pack_alloc((size_t)boc[0] * 9 * 64 * e.esz());
      e.pack_conv_into(e.Wd("conv_out.weight"), wg, cfg.out_channels, boc[0], 2, 64);
      conv_out.Wg = wg;
    }
    build_kv_group(e);
    build_temb_group(e);
    e.finish_lora();
    e.gscale = (float*)e.pack_alloc(e.GSCALE_FLOATS * sizeof(float));
    e.samp_mult_dev = (float*)e.pack_alloc(2 * e.MAXS * sizeof(float));
    splitk_ws = e.pack_alloc(SPLITK_WS_BYTES);  // fp32 slabs of the split-K launches (gemm.hip: S x tiles <= 384 tiles)
    e.alloc_job_table(11 * (e.sites.size() + 8));  // a conv site pushes 10 jobs (d_up + one d_down job per filter tap)
    for (size_t i = 0; i < e.sites.size(); ++i)
      if (!e.site_used[i] && !e.err) {
        set_error("LoRA target '%s' is not a layer this engine adapts (attention projections; with c3lier: resnet "
                  "conv1 / conv2 / time_emb_proj / conv_shortcut and the up / down sampler convs)",
                  e.site_names[i].c_str());
        e.err = true;
      }
  }

  // every cross-attention k|v projection reads the same ctx: stack them into ONE GEMM per pass (70 launches of a
  // 3x10-tile grid -> one launch of a 3x1300-tile grid on SD-XL).  Only when no LoRA adapts to_k / to_v.
  template <typename F>
  void for_each_tblock(F f) {
    for (auto& lv : down) for (auto& t : lv.att) for (auto& tb : t.blocks) f(tb);
    for (auto& t : mid.att) for (auto& tb : t.blocks) f(tb);
    for (auto& lv : up) for (auto& t : lv.att) for (auto& tb : t.blocks) f(tb);
  }
  void build_kv_group(smi_engine& e) {
    int64_t total = 0;
    bool any_lora = false;
    for_each_tblock([&](TBlock& tb) {
      tb.kv_col = total;
      total += tb.kv2.out;
      any_lora |= tb.kv2.nsite > 0;
    });
    kv_adapted = any_lora;
    kv_grouped = !any_lora && total > 0 && total * (int64_t)cfg.cross_attention_dim * 2 < 0xFFFFFFF0ll;
    if (!kv_grouped) return;
    const int D = cfg.cross_attention_dim;
    char* w = (char*)e.pack_alloc((size_t)total * D * e.esz());
    for_each_tblock([&](TBlock& tb) {
      if (!e.dry && !e.err && tb.kv2.W)
        (void)hipMemcpyAsync(w + (size_t)tb.kv_col * D * e.esz(), tb.kv2.W, (size_t)tb.kv2.out * D * e.esz(),
                             hipMemcpyDeviceToDevice, e.stream);
    });
    kv_all.name = "grouped attn2.to_k|to_v";
    kv_all.W = w;
    kv_all.in = D;
    kv_all.out = (int)total;
  }

  // every resnet's time_emb_proj reads the same silu(emb) [n, 1280]: stack them into ONE GEMM per pass (SD-1.x: 22
  // launches of n <= 32 rows, each a split-K pair, -> one pair); the conv1 epilogues read their column block as a row
  // vector with a leading dimension.  Only when no adaptor sits on a time_emb_proj (c3lier has one on each).
  template <typename F>
  void for_each_resnet(F f) {
    for (auto& lv : down) for (auto& r : lv.res) f(r);
    for (auto& r : mid.res) f(r);
    for (auto& lv : up) for (auto& r : lv.res) f(r);
  }
  void build_temb_group(smi_engine& e) {
    int64_t total = 0;
    bool any_lora = false, same_in = true;
    int in = 0;
    for_each_resnet([&](Resnet& r) {
      r.temb_col = total;
      total += r.temb.out;
      any_lora |= r.temb.nsite > 0;
      if (in == 0) in = r.temb.in;
      same_in &= r.temb.in == in;
    });
    static const bool off = getenv("SMI_TEMB_GROUP") && atoi(getenv("SMI_TEMB_GROUP")) == 0;
    temb_grouped = !off && !any_lora && same_in && total > 0 && total % 8 == 0;
    if (!temb_grouped) return;
    char* w = (char*)e.pack_alloc((size_t)total * in * e.esz());
    char* b = (char*)e.pack_alloc((size_t)total * e.esz());
    if (!e.dry && !e.err) (void)hipMemsetAsync(b, 0, (size_t)total * e.esz(), e.stream);  // (a projection without a bias adds zero)
    for_each_resnet([&](Resnet& r) {
      if (e.dry || e.err || !r.temb.W) return;
      (void)hipMemcpyAsync(w + (size_t)r.temb_col * in * e.esz(), r.temb.W, (size_t)r.temb.out * in * e.esz(),
                           hipMemcpyDeviceToDevice, e.stream);
      if (r.temb.b)
        (void)hipMemcpyAsync(b + (size_t)r.temb_col * e.esz(), r.temb.b, (size_t)r.temb.out * e.esz(),
                             hipMemcpyDeviceToDevice, e.stream);
    });
    temb_all.name = "grouped time_emb_proj";
    temb_all.W = w;
    temb_all.b = b;
    temb_all.in = in;
    temb_all.out = (int)total;
  }

  // a resnet with its projected time embedding: a column block of the grouped projection (a gradient flows into it only
  // where the pooled embedding is differentiated: then into the block's columns of the grouped gradient), or this resnet's
  // own time_emb_proj
  Ten* resnet(smi_engine& e, Ten* x, const Resnet& r, Ten* temb_act, bool keep_out = false) {
    if (!temb_all_out) return e.resnet(x, r, e.linear(temb_act, r.temb), 0, keep_out);
    Ten* t = e.borrowed((char*)temb_all_out->p + (size_t)r.temb_col * e.esz(), temb_all_out->rows, r.temb.out, temb_all_out->n);
    t->ng = temb_all_out->ng;
    return e.resnet(x, r, t, temb_all.out, keep_out, t->ng ? temb_all_out : nullptr);
  }

  Ten* transformer(smi_engine& e, Ten* x, const Transformer& t, Ten* ctx, bool keep_out = false) {
    const int C = t.C, nb = x->n, Nq = x->H * x->W;
    Ten* h = e.groupnorm(x, t.norm, false);
    h = e.linear(h, t.proj_in);
    for (const TBlock& tb : t.blocks) {
      Ten* nrm = e.layernorm(h, tb.n1);
      Ten* qkv = e.linear(nrm, tb.qkv1);
      Ten* o = e.attention(qkv, nullptr, nullptr, t.heads, C, nb, Nq, Nq, false);
      h = e.linear(o, tb.out1, h);
      nrm = e.layernorm(h, tb.n2);
      Ten* q = e.linear(nrm, tb.q2);
      if (kv_grouped) {  // with the context differentiated, dK|dV go to this block's columns of the grouped gradient
        // (a q that takes a gradient for the pooled embedding's sake alone: dK|dV keep the bits of a pass without it)
        const bool dq_apart = temb_all_out && temb_all_out->ng && !e.grad_src && !e.lora_active(tb.q2);
        o = e.attention(nullptr, q, nullptr, t.heads, C, nb, Nq, ctx_len, false,
                        (const char*)kv_all_out->p + (size_t)tb.kv_col * e.esz(), kv_all.out,
                        kv_all_out->ng ? kv_all_out : nullptr, dq_apart);
      } else {
        Ten* kv = e.linear(ctx, tb.kv2);
        o = e.attention(nullptr, q, kv, t.heads, C, nb, Nq, ctx_len, false);
      }
      h = e.linear(o, tb.out2, h);
      nrm = e.layernorm(h, tb.n3);
      Ten* gg = e.linear_geglu(nrm, tb.ff1);
      h = e.linear(gg, tb.ff2, h);
    }
    if (keep_out) e.keep_next_output();  // (linear creates its output tensor first)
    return e.linear(h, t.proj_out, x);
  }

  // ---------------------------------------------------------------------------------------------------------
  // whole passes
  // ---------------------------------------------------------------------------------------------------------
  void dry_forward(smi_engine& e) override { forward(e, e.max_n, max_n_ad, nullptr, 0.f, nullptr, nullptr, nullptr, false, nullptr); }
  int forward(smi_engine& e, int n, int n_adapted, const float* sample, float timestep, const void* ctxp, const void* text_embeds,
              const float* time_ids, bool save, float* eps_out) {
    e.begin_pass(n_adapted, save);
    if (save) ++tape_gen;
    e.grad_src = false;
    e.phase_live = nullptr;
    const int H = lat_h, Wd_ = lat_w, HW = H * Wd_;
    const int C0 = cfg.block_out_channels[0];
    const int ted = C0 * 4;

    // ---- time / added-condition embedding (not adapted under lierla; the one gradient that flows here is the pooled
    // embedding's, by the closure below the grouped projection: these ops push none of their own)
    Ten* add_pre = nullptr;  // add_embedding.linear_1's output, the pre-activation of its SiLU
    float* tvals = e.alloc_f32(n);
    if (!e.dry && !e.err) hipLaunchKernelGGL(fill_kernel, dim3(1), dim3(64), 0, e.stream, tvals, timestep, n);
    Ten* te = e.new_ten(n, C0, n, 1, 1);  // [n, C] tensors carry n, H = W = 1: the adapted samples are the last rows
    RUN(launch_timestep_embed(e.dtype, tvals, te->p, n, C0, e.stream));
    Ten* emb = e.linear(e.silu(e.linear(te, time1)), time2);
    if (cfg.addition_embed) {
      const int P = cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim;
      Ten* tid = e.new_ten(n, 6 * cfg.addition_time_embed_dim, n, 1, 1);
      RUN(launch_timestep_embed(e.dtype, time_ids, tid->p, n * 6, cfg.addition_time_embed_dim, e.stream));
      Ten* cat = e.new_ten(n, cfg.projection_class_embeddings_input_dim, n, 1, 1);
      Ten pooled;
      pooled.p = const_cast<void*>(text_embeds);
      RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_copy_cols(e.dtype, pooled.p, P, cat->p, cat->cols, 0, n, P, e.stream));
      RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_copy_cols(e.dtype, tid->p, tid->cols, cat->p, cat->cols, P, n, tid->cols, e.stream));
      add_pre = e.linear(cat, add1);
      Ten* aug = e.linear(e.silu(add_pre), add2);
      Ten* sum = e.new_ten(n, ted, n, 1, 1);
      RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_add(e.dtype, emb->p, aug->p, sum->p, (int64_t)n * ted, e.stream));
      emb = sum;
    }
    Ten* temb_act = e.silu(emb);
    if (!e.prep_sites.empty() && (e.dry || (e.lora_down && e.lora_up && e.mult != 0.f)))
      RUNP(SMI_PROF_LORA, 0.0, 0.0, launch_lora_prep(e.dtype, e.prep_sites_dev, (int)e.prep_sites.size(), e.lora_down, e.lora_up, e.lora_shadow, e.stream));
    // (a forward always rebuilds: the parameters behind the same pointers change with every optimiser step)
    if (e.lora_down && e.lora_up && e.mult != 0.f) e.dora_prepare(e.lora_down, e.lora_up, e.mult, e.saving, false);

    // ---- context as a [n*L, D] tensor (borrowed)
    Ten* ctx = e.borrowed(ctxp, (int64_t)n * ctx_len, cfg.cross_attention_dim, n);
    // The backward of adapted to_k / to_v reads the context again (d(down) = dxa^T ctx), possibly long after this call
    // returned: the saved pass keeps its own copy, so that it does not matter what the caller does with its buffer in
    // between (a temporary handed to the forward is free for reuse as soon as the call returns).
    if (save && kv_adapted && (e.dry || (e.lora_down && e.lora_up && e.mult != 0.f))) {
      void* own = e.alloc_t(ctx->rows, ctx->cols);
      RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_copy_cols(e.dtype, ctxp, ctx->cols, own, ctx->cols, 0, (int)ctx->rows, ctx->cols, e.stream));
      ctx->p = own;
    }

    if (kv_grouped) kv_all_out = e.linear(ctx, kv_all);
    const bool ctx_grad = save && ctx_want && e.n_ad > 0;
    if (ctx_grad) {
      ctx->ng = true;
      ctx->f32g = true;
      if (kv_grouped) {  // runs after every cross-attention backward: d_ctx = dKV_all [rows, sum N] x W_all as ONE GEMM
        Ten* kvo = kv_all_out;
        kvo->ng = true;
        e.tape.push_back([=, &e]() {
          if (!kvo->g || !e.d_ctx) return;
          const GemmParams p =
              gemm_nt(e.dtype, kvo->g, kv_all.out, kv_all.Wt, e.d_ctx, ctx->cols, (int)e.MA(ctx), ctx->cols, kv_all.out).f32_out();
          e.run_gemm(SMI_PROF_GEMM, p, e.gemm_flops(p), e.gemm_bytes(p), true, "d_ctx");
          e.d_ctx_written = true;
        });
      }
    }
    // (only while nothing upstream of emb is trained: the column-block views carry no gradient)
    temb_all_out = (temb_grouped && !temb_act->ng) ? e.linear(temb_act, temb_all) : nullptr;
    const bool pool_grad = ctx_grad && pool_want && temb_all_out && add_pre;
    if (pool_grad) {  // runs after every resnet's backward: the whole chain back to text_embeds (see `tpack`)
      Ten* tao = temb_all_out;
      Ten* emb_pre = emb;  // the pre-activation of temb_act; d(emb) = d(aug): the time branch takes no gradient
      tao->ng = true;
      e.tape.push_back([=, &e]() {
        if (!tao->g || !d_pooled) return;
        const int M = (int)e.MA(tao), P = pooled_dim();
        float* ga = e.alloc_f32((size_t)M * ted);
        const GemmParams p = gemm_nt(e.dtype, tao->g, temb_all.out, temb_all.Wt, ga, ted, M, ted, temb_all.out).f32_out();
        e.run_gemm(SMI_PROF_GEMM, p, e.gemm_flops(p), e.gemm_bytes(p), true, "d_temb_act");
        RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_silu_bwd_f32(e.dtype, e.PA(emb_pre), ga, (int64_t)M * ted, e.stream));
        float* gh = e.alloc_f32((size_t)M * ted);
        RUNP(SMI_PROF_GEMM, 2.0 * M * ted * ted, 2.0 * ted * ted,
             launch_vecmat_f32(e.dtype, ga, add2.W, gh, M, add2.out, add2.in, add2.in, ted, e.stream));
        RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_silu_bwd_f32(e.dtype, e.PA(add_pre), gh, (int64_t)M * ted, e.stream));
        RUNP(SMI_PROF_GEMM, 2.0 * M * ted * P, 2.0 * ted * P,
             launch_vecmat_f32(e.dtype, gh, add1.W, d_pooled, M, add1.out, add1.in, P, P, e.stream));
        d_pooled_written = true;
      });
    }

    // ---- conv_in (MFMA implicit GEMM on the 64-channel zero-padded latent)
    Ten* x0 = e.new_ten((int64_t)n * HW, 64, n, H, Wd_);
    RUN(launch_nchw_to_nhwc(e.dtype, sample, 1, x0->p, n, cfg.in_channels, HW, 64, 1.f, e.stream));
    Ten* h = e.new_ten((int64_t)n * HW, C0, n, H, Wd_);
    {
      const GemmParams p = conv3x3_fwd(e.dtype, x0->p, conv_in.Wp, h->p, n, H, Wd_, 64, C0).with_bias(conv_in.b);
      e.run_gemm(SMI_PROF_CONV, p, 2.0 * p.M * p.N * 9 * cfg.in_channels, 0.0, true, "conv_in");
    }

    // (begin_block / end_block: scratch-region liveness of the no-grad passes, see new_ten; no-ops in a saved pass)
    std::vector<Ten*> skips;
    skips.push_back(h);
    for (size_t i = 0; i < down.size(); ++i) {
      Level& lv = down[i];
      for (size_t j = 0; j < lv.res.size(); ++j) {
        e.begin_block();  // every down-path block output is a skip connection: kept
        h = resnet(e, h, lv.res[j], temb_act, !lv.has_att);
        if (lv.has_att) h = transformer(e, h, lv.att[j], ctx, true);
        e.end_block();
        skips.push_back(h);
      }
      if (lv.has_samp) {
        e.begin_block();
        e.keep_next_output();
        h = e.conv3x3(h, lv.samp, nullptr, nullptr);
        e.end_block();
        skips.push_back(h);
      }
    }
    e.begin_block();
    h = resnet(e, h, mid.res[0], temb_act);
    e.end_block();
    e.begin_block();
    h = transformer(e, h, mid.att[0], ctx);
    e.end_block();
    e.begin_block();
    h = resnet(e, h, mid.res[1], temb_act);
    e.end_block();
    for (size_t i = 0; i < up.size(); ++i) {
      Level& lv = up[i];
      for (size_t j = 0; j < lv.res.size(); ++j) {
        Ten* sk = skips.back();
        skips.pop_back();
        e.begin_block();
        h = e.concat(h, sk);
        h = resnet(e, h, lv.res[j], temb_act);
        if (lv.has_att) h = transformer(e, h, lv.att[j], ctx);
        e.end_block();
      }
      if (lv.has_samp) {
        e.begin_block();
        h = e.conv3x3(h, lv.samp, nullptr, nullptr);
        e.end_block();
      }
    }
    e.begin_block();
    Ten* hn = e.groupnorm(h, norm_out, true);

    // ---- conv_out (MFMA path, fp32 result) + NHWC->NCHW
    Ten* y = e.new_ten((int64_t)n * HW, cfg.out_channels, n, H, Wd_, sizeof(float));
    {
      const GemmParams p =
          conv3x3_fwd(e.dtype, hn->p, conv_out.Wp, y->p, n, H, Wd_, C0, cfg.out_channels).f32_out().with_bias(conv_out.b);
      e.run_gemm(SMI_PROF_CONV, p, e.gemm_flops(p), 0.0, true, "conv_out");
    }
    RUN(launch_nhwc_to_nchw_f32((const float*)y->p, eps_out, n, cfg.out_channels, HW, e.stream));
    e.end_block();
    y->ng = hn->ng;
    if (e.saving && y->ng) {
      e.tape.push_back([=, &e]() {
        if (!y->g) return;
        void* dx = e.grad_slot(hn).out;
        // y->g [adapted rows, 64]: d_eps channels zero-padded
        const GemmParams b = conv3x3_grad(e.dtype, y->g, conv_out.Wg, dx, (int)(e.MA(hn) / HW), H, Wd_, C0, 64);
        e.run_gemm(SMI_PROF_CONV, b, 2.0 * b.M * b.N * 9 * cfg.out_channels, 0.0, true, "conv_out dX");
      });
    }
    if (save) {
      out_ten = y;
      bw_ctx = ctx_grad;
      bw_pool = pool_grad;
      e.keep_saved_pass(n_adapted);
    }
    e.saving = false;
    return e.end_pass(save ? "this call (arena 1 " : "this call (arena 0 ");
  }

  void forget_saved_pass(smi_engine& e) {  // arena 1 moves (re-plan, context-gradient buffer): what pointed into it goes
    e.saved.uploaded.clear();
    e.tape.clear();
    e.saved.valid = false;
    e.tens_[1].clear();
    out_ten = nullptr;
  }
  // n_live: d_eps covers the LAST n_live adapted samples of the saved pass; the caller promises that the gradient with
  // respect to the other adapted samples' output is exactly zero (then so is every gradient row of theirs, and they add
  // exact zeros to the weight-gradient sums).  n_live == e.saved.n is the full backward.
  int backward(smi_engine& e, const float* d_eps, float* dd, float* du, int n_live, float* dctx = nullptr,
               float* dpool = nullptr) {
    e.d_ctx = dctx;
    e.d_ctx_written = false;
    d_pooled = dpool;
    d_pooled_written = false;
    if (const int rc = e.begin_backward("smi_unet_backward: no saved forward pass (call smi_unet_forward with save_for_backward=1 first)",
                                        dd, du, n_live))
      return rc;
    const int n = n_live, HW = lat_h * lat_w;  // d_eps covers the live adapted samples only
    Ten* y = out_ten;
    if (!y->ng) {  // adaptor off: nothing depends on the LoRA parameters
      e.drop_tape();
      return 0;
    }
    if (n > e.MAXS && !e.dry) {
      set_error("smi_unet_backward: %d adapted samples exceed the %d per-sample loss scales", n, e.MAXS);
      return -1;
    }
    if (e.bw_skip > 0) {  // every closure works on rows [arow0, rows): start them at the first live sample (the tape and its
      for (Ten& t : *e.tens) {  // tensors do not outlive this call)
        if (t.n <= 0) continue;
        t.bskip = (int64_t)e.bw_skip * (t.rows / t.n);
        t.arow0 += t.bskip;
      }
    }
    // one power-of-two loss scale PER SAMPLE (from max|d_eps[sample]|): a sample's backward arithmetic then does not
    // depend on which other samples share the batch -- W ranks on shards == one rank on the global batch
    RUN(launch_grad_scale(d_eps, n, (int64_t)cfg.out_channels * HW, e.gscale, e.MAXS, e.stream));
    e.rebuild_saved_operands();
    if (!e.dora_sites.empty() && e.bw_down && e.bw_up && e.bw_mult != 0.f) {  // the DoRA delta weights likewise
      e.dora_prepare(e.bw_down, e.bw_up, e.bw_mult, true, true);
      RUN(launch_scale_min(e.gscale, n, e.gscale + 2 * e.MAXS, e.stream));
    }
    y->g = e.alloc_t(e.MA(y), 64);
    RUN(launch_nchw_to_nhwc_scaled(e.dtype, d_eps, y->g, n, cfg.out_channels, HW, 64, e.gscale, e.stream));
    if (e.run_tape_and_weight_grads()) return -1;
    if (e.d_ctx && !e.dry && !e.err) {  // the loss scale of each sample's rows divides out; no term at all: the gradient is zero
      const int L = ctx_len, D = cfg.cross_attention_dim;
      if (e.d_ctx_written) RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_row_scale_f32(e.d_ctx, D, n * L, D, e.gscale + e.MAXS, L, e.stream));
      else (void)hipMemsetAsync(e.d_ctx, 0, (size_t)n * L * D * sizeof(float), e.stream);
    }
    if (d_pooled && !e.dry && !e.err) {  // one row per sample: the same unscale; no term at all: the gradient is zero
      const int P = pooled_dim();
      if (d_pooled_written) RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_row_scale_f32(d_pooled, P, n, P, e.gscale + e.MAXS, 1, e.stream));
      else (void)hipMemsetAsync(d_pooled, 0, (size_t)n * P * sizeof(float), e.stream);
    }
    e.d_ctx = nullptr;
    d_pooled = nullptr;
    return e.end_pass("the backward (");
  }
};

int check_cfg(const smi_unet_config* c) {
  SMI_CHECK(c != nullptr, "config is NULL");
  SMI_CHECK(c->dtype == SMI_DTYPE_F16 || c->dtype == SMI_DTYPE_BF16, "dtype must be f16 (0) or bf16 (1)");
  SMI_CHECK(c->n_levels >= 1 && c->n_levels <= SMI_MAX_LEVELS, "n_levels out of range");
  SMI_CHECK(c->in_channels >= 1 && c->in_channels <= 16 && c->out_channels == 4, "in/out channels unsupported");
  for (int i = 0; i < c->n_levels; ++i) {
    SMI_CHECK(c->block_out_channels[i] % 64 == 0, "block_out_channels must be multiples of 64 (MFMA K tile)");
    SMI_CHECK(c->block_out_channels[i] % c->norm_num_groups == 0, "channels must divide by norm_num_groups");
    SMI_CHECK(c->num_heads[i] > 0 && c->block_out_channels[i] % c->num_heads[i] == 0, "heads must divide channels");
    SMI_CHECK((c->block_out_channels[i] / c->num_heads[i]) % 8 == 0, "head_dim must be a multiple of 8");
  }
  SMI_CHECK(c->cross_attention_dim % 8 == 0, "cross_attention_dim %% 8");
  return 0;
}

// the engine lends its split-K scratch to launch_gemm for the duration of one call on this host thread
struct GemmScratchScope {
  GemmScratchScope(void* ws, size_t bytes) { smi::set_gemm_scratch(ws, bytes); }
  ~GemmScratchScope() { smi::set_gemm_scratch(nullptr, 0); }
};

// the UNet of a UNet engine; NULL for every other kind
UNet* unet(const smi_engine* e) { return e->kind == smi_engine::UNET ? static_cast<UNet*>(e->model.get()) : nullptr; }

UNet* setup(smi_engine* e, const smi_unet_config* cfg, const smi_weight* weights, int n_weights,
            const smi_lora_site* sites, int n_sites, int batch, int batch_adapted, int h, int w, int ctx_len) {
  UNet* u = new UNet();
  e->hold(smi_engine::UNET, u, cfg->dtype, batch);
  u->cfg = *cfg;
  u->max_n_ad = batch_adapted;
  u->lat_h = h;
  u->lat_w = w;
  u->ctx_len = ctx_len;
  for (int i = 0; i < n_weights; ++i) e->wmap[weights[i].name] = &weights[i];
  e->register_sites(sites, n_sites);
  return u;
}

// dry run: sizes of the three regions
// ctx_bytes != NULL: the plan of an engine that differentiates the context -- *ctx_bytes receives the bytes of its extra
// transposed weights and out[2] is the saved-pass arena of a forward + backward with the context gradient on
int plan(const smi_unet_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int batch_adapted, int h, int w,
         int ctx_len, size_t out[5], size_t* ctx_bytes = nullptr, size_t* pool_bytes = nullptr) {
  smi_engine e;
  e.dry = true;
  UNet& u = *setup(&e, cfg, nullptr, 0, sites, n_sites, batch, batch_adapted, h, w, ctx_len);
  u.build(e);
  if (e.err) return -1;
  if (ctx_bytes) {
    u.build_ctx_grad(e);
    *ctx_bytes = align_up(u.xpack.peak, 4096);
    u.ctx_want = true;
  }
  if (pool_bytes) {  // (with ctx_bytes) ... that also differentiates the pooled embedding: its transposed grouped weight
    if (u.build_pooled_grad(e)) return -1;
    *pool_bytes = align_up(u.tpack.peak, 4096);
    u.pool_want = true;
  }
  out[0] = align_up(e.wpack.peak, 4096);
  u.dry_forward(e);
  // arena 0 = [persistent | scratch 0 | scratch 1] (no-grad liveness, smi_engine::begin_block)
  out[3] = align_up(e.arena[0].peak, 4096);
  out[4] = align_up(std::max(e.scr[0].peak, e.scr[1].peak), 4096);
  out[1] = out[3] + 2 * out[4];
  u.forward(e, batch, batch_adapted, nullptr, 0.f, nullptr, nullptr, nullptr, true, nullptr);
  // sized for the full backward: a tail backward needs less
  u.backward(e, nullptr, nullptr, nullptr, e.saved.n, ctx_bytes ? reinterpret_cast<float*>(16) : nullptr,
             pool_bytes ? reinterpret_cast<float*>(16) : nullptr);
  out[2] = align_up(e.arena[1].peak, 4096);
  return e.err ? -1 : 0;
}

// the refusal of the UNet-only entry points that take any engine; `why` completes the sentence
int refuse_other_kind(const smi_engine* e, const char* why) {
  SMI_CHECK(e->kind == smi_engine::UNET, "this engine is a VAE encoder / decoder or a CLIP text / vision encoder%s", why);
  return 0;
}

// smi_unet_ctx_grad_bytes / smi_unet_pooled_grad_bytes (pooled): the transposed weights of that gradient + the saved-pass
// arena of a forward + backward with it on
int grad_buffer_bytes(const smi_unet_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int batch_adapted, int h,
                      int w, int ctx_len, size_t* bytes, bool pooled) {
  if (check_cfg(cfg)) return -1;
  SMI_CHECK(bytes && batch > 0 && batch_adapted >= 0 && batch_adapted <= batch && h > 0 && w > 0 && ctx_len > 0,
            "bad arguments");
  size_t r[5], x = 0, t = 0;
  if (plan(cfg, sites, n_sites, batch, batch_adapted, h, w, ctx_len, r, &x, pooled ? &t : nullptr)) return -1;
  *bytes = (pooled ? t : x) + r[2] + 2 * 4096;
  return 0;
}

// smi_unet_ctx_grad_attach / smi_unet_pooled_grad_attach (pooled) after their own refusals: the buffer becomes
// [pack arena of the transposed weights (xpack / tpack), built here | arena 1, sized for that gradient's saved pass]
int attach_grad_buffer(smi_engine* e, void* buffer, size_t buffer_bytes, bool pooled) {
  UNet* u = unet(e);
  const char* name = pooled ? "smi_unet_pooled_grad_attach" : "smi_unet_ctx_grad_attach";
  size_t r[5], x = 0, t = 0;
  if (plan(&u->cfg, e->sites.data(), (int)e->sites.size(), e->max_n, u->max_n_ad, u->lat_h, u->lat_w, u->ctx_len, r, &x,
           pooled ? &t : nullptr))
    return -1;
  const size_t pack_bytes = pooled ? t : x;
  Arena& pack = pooled ? u->tpack : u->xpack;
  char* base = (char*)align_up((size_t)buffer, 4096);
  const size_t have = (size_t)((char*)buffer + buffer_bytes - base);
  SMI_CHECK((char*)buffer + buffer_bytes >= base && pack_bytes + r[2] <= have, "%s: buffer too small: need %zu bytes, got %zu",
            name, pack_bytes + r[2] + 2 * 4096, buffer_bytes);
  e->err = false;
  pack = Arena();
  pack.base = base;
  pack.cap = pack_bytes;
  if (!pooled) u->build_ctx_grad(*e);
  else if (u->build_pooled_grad(*e)) return -1;
  SMI_HIP(hipGetLastError());
  SMI_CHECK(!e->err && !pack.overflow, "%s: packing the transposed %s weights failed", name, pooled ? "time_emb_proj" : "k|v");
  e->arena[1] = Arena();  // the saved pass of a forward + backward with this gradient on is larger than the plain one
  e->arena[1].base = base + pack_bytes;
  e->arena[1].cap = r[2];
  u->forget_saved_pass(*e);  // the saved activations lived in the old arena
  return 0;
}

// Every backward entry point begins here, after its NULL check: another kind of engine is refused, and so is, under
// `name`, an engine without a saved pass (name NULL: smi_unet_backward, which leaves that to UNet::backward's own refusal)
int backward_begin(const smi_engine* e, const char* name) {
  if (refuse_other_kind(e, ": it has no backward")) return -1;
  SMI_CHECK(!name || e->saved.valid, "%s: no saved forward pass (call smi_unet_forward with save_for_backward=1 first)", name);
  return 0;
}

// ... and, after the refusals of its own, ends here.  d_ctx / d_pooled: smi_unet_backward_ctx / _cond, which take the
// adaptor's gradient buffers only when the saved pass ran with the adaptor on
int backward_launch(smi_engine* e, const char* name, const float* d_eps, float* d_lora_down_flat, float* d_lora_up_flat,
                    int n_live, float* d_ctx = nullptr, float* d_pooled = nullptr) {
  UNet* u = unet(e);
  const bool adapted = e->bw_down && e->bw_up && e->bw_mult != 0.f && !e->sites.empty();
  SMI_CHECK(!adapted || (d_lora_down_flat && d_lora_up_flat),
            "%s: the saved pass ran with the adaptor on: its gradient buffers are required", name);
  e->err = false;
  GemmScratchScope scratch(u->splitk_ws, UNet::SPLITK_WS_BYTES);
  return u->backward(*e, d_eps, d_lora_down_flat, d_lora_up_flat, n_live, d_ctx, d_pooled);
}

}  // namespace

extern "C" {

int smi_workspace_bytes(const smi_unet_config* cfg, const smi_lora_site* sites, int n_sites, int batch,
                        int batch_adapted, int h, int w, int ctx_len, size_t* bytes) {
  if (check_cfg(cfg)) return -1;
  SMI_CHECK(bytes && batch > 0 && batch_adapted >= 0 && batch_adapted <= batch && h > 0 && w > 0 && ctx_len > 0,
            "bad arguments");
  size_t r[5];
  if (plan(cfg, sites, n_sites, batch, batch_adapted, h, w, ctx_len, r)) return -1;
  *bytes = r[0] + r[1] + r[2] + 3 * 4096;
  return 0;
}

int smi_create(const smi_unet_config* cfg, const smi_weight* weights, int n_weights, const smi_lora_site* sites,
               int n_sites, int batch, int batch_adapted, int h, int w, int ctx_len, void* workspace,
               size_t workspace_bytes, void* stream, smi_engine** out) {
  if (check_cfg(cfg)) return -1;
  SMI_CHECK(out && workspace && weights && n_weights > 0 && batch_adapted >= 0 && batch_adapted <= batch,
            "bad arguments");
  size_t r[5];
  if (plan(cfg, sites, n_sites, batch, batch_adapted, h, w, ctx_len, r)) return -1;
  SMI_CHECK(r[0] + r[1] + r[2] + 3 * 4096 <= workspace_bytes, "workspace too small: need %zu bytes, got %zu",
            r[0] + r[1] + r[2] + 3 * 4096, workspace_bytes);
  smi_engine* e = new smi_engine();
  e->stream = (hipStream_t)stream;
  UNet* u = setup(e, cfg, weights, n_weights, sites, n_sites, batch, batch_adapted, h, w, ctx_len);
  char* base = (char*)align_up((size_t)workspace, 4096);
  e->wpack.base = base;
  e->wpack.cap = r[0];
  e->arena[0].base = base + r[0];
  e->arena[1].base = base + r[0] + r[1];
  e->arena[1].cap = r[2];
  e->set_arena0_regions(r[3], r[4]);
  u->arena_home = base + r[0];
  u->arena_home_bytes = (size_t)((char*)workspace + workspace_bytes - u->arena_home);
  u->build(*e);
  return finish_create(e, "weights", out);
}

int smi_weights_bytes(const smi_unet_config* cfg, const smi_lora_site* sites, int n_sites, size_t* bytes) {
  if (check_cfg(cfg)) return -1;
  SMI_CHECK(bytes != nullptr, "bad arguments");
  size_t r[5];
  if (plan(cfg, sites, n_sites, 1, 1, 8, 8, 8, r)) return -1;  // the packed region does not depend on the shape
  *bytes = r[0] + 4096;
  return 0;
}

int smi_arena_bytes(const smi_unet_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int batch_adapted,
                    int h, int w, int ctx_len, size_t* bytes) {
  if (check_cfg(cfg)) return -1;
  SMI_CHECK(bytes && batch > 0 && batch_adapted >= 0 && batch_adapted <= batch && h > 0 && w > 0 && ctx_len > 0,
            "bad arguments");
  size_t r[5];
  if (plan(cfg, sites, n_sites, batch, batch_adapted, h, w, ctx_len, r)) return -1;
  *bytes = r[1] + r[2] + 2 * 4096;
  return 0;
}

int smi_replan(smi_engine* e, int batch, int batch_adapted, int h, int w, int ctx_len, void* arena,
               size_t arena_bytes) {
  SMI_CHECK(e && batch > 0 && batch_adapted >= 0 && batch_adapted <= batch && h > 0 && w > 0 && ctx_len > 0,
            "bad arguments");
  SMI_CHECK(e->kind == smi_engine::UNET, "smi_replan: only UNet engines re-plan");
  UNet* u = unet(e);
  size_t r[5];
  if (plan(&u->cfg, e->sites.data(), (int)e->sites.size(), batch, batch_adapted, h, w, ctx_len, r)) return -1;
  char* base = arena ? (char*)align_up((size_t)arena, 4096) : u->arena_home;
  const size_t have = arena ? (size_t)((char*)arena + arena_bytes - base) : u->arena_home_bytes;
  SMI_CHECK(r[1] + r[2] <= have, "arena too small for batch %d (%d adapted), %dx%d latents: need %zu bytes, got %zu", batch,
            batch_adapted, h, w, r[1] + r[2] + 2 * 4096, arena ? arena_bytes : u->arena_home_bytes);
  u->forget_saved_pass(*e);  // the saved activations lived in the old arena
  e->max_n = batch;
  u->max_n_ad = batch_adapted;
  u->lat_h = h;
  u->lat_w = w;
  u->ctx_len = ctx_len;
  e->arena[0] = Arena();
  e->arena[1] = Arena();
  e->arena[0].base = base;
  e->arena[1].base = base + r[1];
  e->arena[1].cap = r[2];
  e->set_arena0_regions(r[3], r[4]);
  u->ctx_cap = u->ctx_want = false;  // the context-gradient arena was sized for the old shape: attach one for the new
  u->pool_cap = u->pool_want = false;  // (and so was the pooled-gradient buffer, whose weight copy folds the map sizes)
  e->tens_[0].clear();
  ++u->replans;
  return 0;
}

int smi_engine_stats(const smi_engine* e, int64_t out[4]) {
  SMI_CHECK(e && out, "NULL argument");
  const UNet* u = unet(e);  // (the other kinds neither re-plan nor save a pass)
  out[0] = e->pack_launches;
  out[1] = u ? u->replans : 0;
  out[2] = u && e->saved.valid ? (int64_t)u->tape_gen : 0;
  out[3] = (int64_t)e->wpack.peak;
  return 0;
}

int smi_unet_forward_batched(smi_engine* e, int n, int n_adapted, const float* sample, float timestep, const void* ctx,
                             const void* text_embeds, const float* time_ids, const float* lora_down_flat,
                             const float* lora_up_flat, float multiplier, int save_for_backward, float* eps_out) {
  SMI_CHECK(e && sample && ctx && eps_out, "NULL argument");
  if (refuse_other_kind(e, " (use smi_vae_encode / smi_vae_decode / smi_clip_encode / smi_clip_vision_encode)")) return -1;
  UNet* u = unet(e);
  SMI_CHECK(n >= 1 && n <= e->max_n, "batch %d outside [1, %d] the engine was created for", n, e->max_n);
  SMI_CHECK(n_adapted >= 0 && n_adapted <= n && n_adapted <= u->max_n_ad,
            "adapted batch %d outside [0, min(%d, %d)]", n_adapted, n, u->max_n_ad);
  SMI_CHECK(!u->cfg.addition_embed || (text_embeds && time_ids), "SD-XL engine needs text_embeds and time_ids");
  SMI_CHECK(!(save_for_backward && u->ctx_want) || u->ctx_cap,
            "context gradient asked for, but no buffer is attached for this shape (smi_unet_ctx_grad_attach)");
  SMI_CHECK(!(save_for_backward && u->pool_want) || (u->pool_cap && u->ctx_want),
            "pooled-embedding gradient asked for, but the context gradient is off or no buffer is attached for this shape "
            "(smi_unet_ctx_grad, smi_unet_pooled_grad_attach)");
  e->err = false;
  e->lora_down = lora_down_flat;
  e->lora_up = lora_up_flat;
  e->mult = (lora_down_flat && lora_up_flat && n_adapted > 0) ? multiplier : 0.f;
  GemmScratchScope scratch(u->splitk_ws, UNet::SPLITK_WS_BYTES);
  return u->forward(*e, n, n_adapted, sample, timestep, ctx, text_embeds, time_ids, save_for_backward != 0, eps_out);
}

int smi_unet_forward_multi(smi_engine* e, int n, int n_adapted, const float* sample, float timestep, const void* ctx,
                           const void* text_embeds, const float* time_ids, const float* lora_down_flat,
                           const float* lora_up_flat, const float* multipliers, int save_for_backward, float* eps_out) {
  SMI_CHECK(e && multipliers, "NULL argument");
  if (refuse_other_kind(e, ": no UNet forward")) return -1;
  SMI_CHECK(n_adapted >= 1 && n_adapted <= smi_engine::MAXS, "per-sample multipliers: 1..%d adapted samples", smi_engine::MAXS);
  bool same = true;
  for (int i = 0; i < n_adapted; ++i) same = same && multipliers[i] == multipliers[0];
  if (same)
    return smi_unet_forward_batched(e, n, n_adapted, sample, timestep, ctx, text_embeds, time_ids, lora_down_flat,
                                    lora_up_flat, multipliers[0], save_for_backward, eps_out);
  SMI_CHECK(e->n_conv_sites == 0 && e->dora_sites.empty(),
            "per-sample multipliers are implemented for Linear LoRA sites (attention projections, time_emb_proj, "
            "conv_shortcut); this network has conv or DoRA sites -- run the samples in separate passes");
  // the per-sample ratios travel in kernel arguments, ordered on the engine's stream (an async copy from a stack
  // array is only correct while the runtime stages pageable sources before returning)
  float mref = 0.f;  // (not 0: the multipliers differ)
  if (const int rc = e->set_sample_multipliers(multipliers, n_adapted, save_for_backward != 0, &mref)) return rc;
  e->samp_on = true;
  const int rc = smi_unet_forward_batched(e, n, n_adapted, sample, timestep, ctx, text_embeds, time_ids, lora_down_flat,
                                          lora_up_flat, mref, save_for_backward, eps_out);
  e->samp_on = false;
  return rc;
}

int smi_unet_forward_compose(smi_engine* e, int n, int n_adapted, const float* sample, float timestep, const void* ctx,
                             const void* text_embeds, const float* time_ids, const float* lora_down_flat,
                             const float* lora_up_flat, int n_sliders, const int* ranks, const float* multipliers,
                             float* eps_out) {
  SMI_CHECK(e && ranks && multipliers && lora_down_flat && lora_up_flat, "NULL argument");
  if (refuse_other_kind(e, ": no UNet forward")) return -1;
  SMI_CHECK(n_adapted >= 1 && n_adapted <= smi_engine::MAXS, "slider composition: 1..%d adapted samples, got %d",
            smi_engine::MAXS, n_adapted);
  SMI_CHECK(n_sliders >= 1 && n_sliders <= smi_engine::MAX_SLIDERS, "slider composition: 1..%d sliders, got %d",
            smi_engine::MAX_SLIDERS, n_sliders);
  int R = 0;
  I16Args rk;
  for (int k = 0; k < 16; ++k) rk.v[k] = 0;
  for (int k = 0; k < n_sliders; ++k) {
    SMI_CHECK(ranks[k] >= 1, "slider composition: rank %d of slider %d", ranks[k], k);
    rk.v[k] = ranks[k];
    R += ranks[k];
  }
  SMI_CHECK(R <= smi_engine::MAX_STACK_RANK, "slider composition: stacked rank %d exceeds %d", R, smi_engine::MAX_STACK_RANK);
  for (int r : e->lin_site_ranks)
    SMI_CHECK(r == R, "slider composition: the ranks sum to %d but a Linear site of this engine has rank %d (its sites must be "
                      "the stacked ones, every slider's block present)", R, r);
  SMI_CHECK(e->n_conv_sites == 0 && e->dora_sites.empty(),
            "slider composition: the multiplier table is implemented for Linear LoRA sites (attention projections, "
            "time_emb_proj, conv_shortcut); this network has conv or DoRA sites -- fold the scales into lora_up and run "
            "samples of different scales in separate plain passes");
  SMI_CHECK((int64_t)n_adapted * R <= smi_engine::COL_TABLE_FLOATS,
            "slider composition: %d adapted samples x stacked rank %d exceed the %d entries of the multiplier table", n_adapted,
            R, smi_engine::COL_TABLE_FLOATS);
  UNet* u = unet(e);
  e->drop_tape();  // inference only: no earlier saved pass answers a backward after this one
  // the table travels in kernel arguments, 64 multipliers per launch, ordered on the engine's stream (as the per-sample
  // ratios of smi_unet_forward_multi do: no asynchronous copy from pageable memory)
  const int per = 64 / n_sliders;
  for (int i0 = 0; i0 < n_adapted; i0 += per) {
    const int cnt = n_adapted - i0 < per ? n_adapted - i0 : per;
    F64Args a;
    for (int i = 0; i < 64; ++i) a.v[i] = i < cnt * n_sliders ? multipliers[i0 * n_sliders + i] : 0.f;
    hipLaunchKernelGGL(col_table_kernel, dim3((cnt * R + 255) / 256), dim3(256), 0, e->stream, e->col_table(), R, i0, cnt,
                       n_sliders, rk, a);
  }
  SMI_HIP(hipGetLastError());
  e->col_on = true;
  e->col_ld = e->col_period = R;
  const int rc = smi_unet_forward_batched(e, n, n_adapted, sample, timestep, ctx, text_embeds, time_ids, lora_down_flat,
                                          lora_up_flat, 1.f, 0, eps_out);
  e->col_on = false;
  return rc;
}

int smi_unet_forward(smi_engine* e, int n, const float* sample, float timestep, const void* ctx,
                     const void* text_embeds, const float* time_ids, const float* lora_down_flat,
                     const float* lora_up_flat, float multiplier, int save_for_backward, float* eps_out) {
  SMI_CHECK(e != nullptr, "NULL argument");
  const UNet* u = unet(e);  // (another kind: smi_unet_forward_batched refuses it)
  return smi_unet_forward_batched(e, n, u && n < u->max_n_ad ? n : u ? u->max_n_ad : 0, sample, timestep, ctx, text_embeds, time_ids,
                                  lora_down_flat, lora_up_flat, multiplier, save_for_backward, eps_out);
}

int smi_unet_backward(smi_engine* e, const float* d_eps, float* d_lora_down_flat, float* d_lora_up_flat) {
  SMI_CHECK(e && d_eps && d_lora_down_flat && d_lora_up_flat, "NULL argument");
  if (backward_begin(e, nullptr)) return -1;
  return backward_launch(e, "smi_unet_backward", d_eps, d_lora_down_flat, d_lora_up_flat, e->saved.n);
}

int smi_unet_ctx_grad_bytes(const smi_unet_config* cfg, const smi_lora_site* sites, int n_sites, int batch,
                            int batch_adapted, int h, int w, int ctx_len, size_t* bytes) {
  return grad_buffer_bytes(cfg, sites, n_sites, batch, batch_adapted, h, w, ctx_len, bytes, false);
}

int smi_unet_ctx_grad_attach(smi_engine* e, void* buffer, size_t buffer_bytes) {
  SMI_CHECK(e && buffer, "NULL argument");
  SMI_CHECK(e->kind == smi_engine::UNET, "smi_unet_ctx_grad_attach: only UNet engines differentiate a context");
  UNet* u = unet(e);
  if (const int rc = attach_grad_buffer(e, buffer, buffer_bytes, false)) return rc;
  u->ctx_cap = true;
  u->pool_cap = u->pool_want = false;  // a pooled-gradient buffer held arena 1 until now: attach it again after this one
  return 0;
}

int smi_unet_ctx_grad(smi_engine* e, int on) {
  SMI_CHECK(e != nullptr, "NULL argument");
  UNet* u = unet(e);  // (another kind never has a buffer attached)
  SMI_CHECK(!on || (u && u->ctx_cap), "smi_unet_ctx_grad: no context-gradient buffer is attached for the engine's current shape "
                                      "(smi_unet_ctx_grad_attach; smi_replan detaches it)");
  if (u) u->ctx_want = on != 0;
  if (u && !on) u->pool_want = false;  // the pooled-embedding gradient rides on the context gradient's pass
  return 0;
}

int smi_unet_backward_ctx(smi_engine* e, const float* d_eps, float* d_lora_down_flat, float* d_lora_up_flat,
                          float* d_ctx_out) {
  SMI_CHECK(e && d_eps && d_ctx_out, "NULL argument");
  if (backward_begin(e, "smi_unet_backward_ctx")) return -1;
  const UNet* u = unet(e);
  SMI_CHECK(u->bw_ctx, "smi_unet_backward_ctx: the saved pass does not differentiate the context (smi_unet_ctx_grad(e, 1) "
                       "before the saving forward)");
  return backward_launch(e, "smi_unet_backward_ctx", d_eps, d_lora_down_flat, d_lora_up_flat, e->saved.n, d_ctx_out);
}

int smi_unet_pooled_grad_bytes(const smi_unet_config* cfg, const smi_lora_site* sites, int n_sites, int batch,
                               int batch_adapted, int h, int w, int ctx_len, size_t* bytes) {
  return grad_buffer_bytes(cfg, sites, n_sites, batch, batch_adapted, h, w, ctx_len, bytes, true);
}

int smi_unet_pooled_grad_attach(smi_engine* e, void* buffer, size_t buffer_bytes) {
  SMI_CHECK(e && buffer, "NULL argument");
  SMI_CHECK(e->kind == smi_engine::UNET, "smi_unet_pooled_grad_attach: only UNet engines differentiate a pooled embedding");
  UNet* u = unet(e);
  SMI_CHECK(u->ctx_cap, "smi_unet_pooled_grad_attach: attach the context-gradient buffer first (smi_unet_ctx_grad_attach): "
                        "the pooled-embedding gradient rides on the context gradient's pass");
  if (const int rc = attach_grad_buffer(e, buffer, buffer_bytes, true)) return rc;
  u->pool_cap = true;
  return 0;
}

int smi_unet_pooled_grad(smi_engine* e, int on) {
  SMI_CHECK(e != nullptr, "NULL argument");
  UNet* u = unet(e);
  if (!on) {
    if (u) u->pool_want = false;
    return 0;
  }
  SMI_CHECK(u, "smi_unet_pooled_grad: only UNet engines differentiate a pooled embedding");
  std::string site;
  const char* why = u->pooled_refusal(site);
  SMI_CHECK(!why, "smi_unet_pooled_grad: %s%s%s", why ? why : "", site.empty() ? "" : ": ", site.c_str());
  SMI_CHECK(u->pool_cap, "smi_unet_pooled_grad: no pooled-gradient buffer is attached for the engine's current shape "
                         "(smi_unet_pooled_grad_attach; smi_replan and smi_unet_ctx_grad_attach detach it)");
  SMI_CHECK(u->ctx_want, "smi_unet_pooled_grad: the context gradient is off (smi_unet_ctx_grad(e, 1) first): the "
                         "pooled-embedding gradient rides on its pass");
  u->pool_want = true;
  return 0;
}

int smi_unet_backward_cond(smi_engine* e, const float* d_eps, float* d_lora_down_flat, float* d_lora_up_flat,
                           float* d_ctx_out, float* d_text_embeds_out) {
  SMI_CHECK(e && d_eps && d_ctx_out && d_text_embeds_out, "NULL argument");
  if (backward_begin(e, "smi_unet_backward_cond")) return -1;
  const UNet* u = unet(e);
  SMI_CHECK(u->bw_ctx && u->bw_pool, "smi_unet_backward_cond: the saved pass does not differentiate the pooled embedding "
                                     "(smi_unet_ctx_grad(e, 1) and smi_unet_pooled_grad(e, 1) before the saving forward)");
  return backward_launch(e, "smi_unet_backward_cond", d_eps, d_lora_down_flat, d_lora_up_flat, e->saved.n, d_ctx_out,
                         d_text_embeds_out);
}

int smi_unet_backward_tail(smi_engine* e, int n_live, const float* d_eps_live, float* d_lora_down_flat,
                           float* d_lora_up_flat) {
  SMI_CHECK(e && d_eps_live && d_lora_down_flat && d_lora_up_flat, "NULL argument");
  if (backward_begin(e, "smi_unet_backward_tail")) return -1;
  const UNet* u = unet(e);
  SMI_CHECK(!u->bw_pool, "smi_unet_backward_tail: the saved pass differentiates the pooled embedding; a tail backward is not "
                         "offered there (use smi_unet_backward_cond)");
  SMI_CHECK(!u->bw_ctx, "smi_unet_backward_tail: the saved pass differentiates the context; a tail backward is not offered "
                        "there (use smi_unet_backward_ctx)");
  SMI_CHECK(n_live >= 1 && n_live <= e->saved.n, "smi_unet_backward_tail: %d live samples outside [1, %d], the adapted samples of the saved pass",
            n_live, e->saved.n);
  return backward_launch(e, "smi_unet_backward_tail", d_eps_live, d_lora_down_flat, d_lora_up_flat, n_live);
}

int smi_profile_enable(smi_engine* e, int enable) {
  SMI_CHECK(e != nullptr, "NULL engine");
  e->prof_collect();
  e->prof_on = enable != 0;
  for (int i = 0; i < SMI_PROF_NCAT; ++i) {
    e->prof_ms[i] = 0;
    e->prof_flops[i] = 0;
    e->prof_bytes[i] = 0;
    e->prof_launches[i] = 0;
  }
  return 0;
}
int smi_profile_read(smi_engine* e, double* ms, double* flops, double* bytes, int64_t* launches) {
  SMI_CHECK(e && ms && flops && bytes && launches, "NULL argument");
  e->prof_collect();
  if (e->prof_dump && !e->prof_tags.empty()) {
    std::vector<std::pair<std::string, smi_engine::TagAcc>> v(e->prof_tags.begin(), e->prof_tags.end());
    std::sort(v.begin(), v.end(), [](const auto& a, const auto& b) { return a.second.ms > b.second.ms; });
    double tot = 0;
    for (auto& kv : v) tot += kv.second.ms;
    fprintf(stderr, "[smi profile] GEMM / conv launches by shape (%.2f ms total)\n", tot);
    for (auto& kv : v)
      fprintf(stderr, "  %8.3f ms %5d x %8.1f us %7.0f TF/s  %s\n", kv.second.ms, kv.second.n,
              kv.second.ms * 1e3 / kv.second.n, kv.second.flops / (kv.second.ms * 1e-3) / 1e12, kv.first.c_str());
    e->prof_tags.clear();
  }
  for (int i = 0; i < SMI_PROF_NCAT; ++i) {
    ms[i] = e->prof_ms[i];
    flops[i] = e->prof_flops[i];
    bytes[i] = e->prof_bytes[i];
    launches[i] = e->prof_launches[i];
  }
  return 0;
}

}  // extern "C"
