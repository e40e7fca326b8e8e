// The Flux transformer engine (diffusers FluxTransformer2DModel: FLUX.1-schnell / dev): the packed latents
// through x_embedder, the conditioning vector temb = time MLP [+ guidance MLP] + pooled-text MLP, double blocks -- the SD3
// joint block with q and k RMS-normalised per head and rotated, context rows first -- single blocks on the joint sequence
// (attention and MLP side by side from one modulated input, into one 5 d -> d projection), and the modulated output
// projection of the image rows, un-packed.  On the op core (engine.h) with the joint-stream ops of engine_joint_ops.h;
// Linear LoRA sites on the attention projections at one multiplier per sample, as the MMDiT takes them.  An engine made by
// smi_flux_train_create also saves a pass and differentiates it to the LoRA parameters (Flux::backward).
//
// What it does not copy: qk_norm_rope (flux.hip) writes a stream's normalised, rotated q|k|v straight into the joint
// buffer, so a double block never calls joint_pack; in a single block the attention writes its output with ldo = 5 d into
// columns [0, d) of the [rows, 5 d] operand of proj_out and proj_mlp's GEMM writes with ldc = 5 d into columns [d, 5 d),
// where tanh-GELU then runs in place: no concat copy.  A SAVED pass keeps two things the backward reads and those in-place
// forms destroy: a single block's pre-norm q|k|v (qk_norm_rope runs out of place into a fresh joint tensor) and proj_mlp's
// pre-activation (a tensor of its own, which tanh-GELU reads with ldx = 4 d and writes into columns [d, 5 d)).  The same
// kernels and arithmetic: the same bits.
#include "engine_joint_ops.h"

namespace {

struct Stream {  // one stream's half of a double block
  Lin mod;       // norm1.linear / norm1_context.linear: [6 d, d]
  Lin qkv, out, ff1, ff2;
  const void *nq = nullptr, *nk = nullptr;  // RMSNorm weights [head_dim]
};
struct DoubleBlock {
  Stream x, c;
};
struct SingleBlock {
  Lin mod;  // norm.linear: [3 d, d] (shift | scale | gate)
  Lin qkv, mlp, out;
  const void *nq = nullptr, *nk = nullptr;
};

struct Flux : Model {
  smi_flux_config cfg{};
  int H = 0, W = 0;  // latent size
  std::vector<DoubleBlock> dbl;
  std::vector<SingleBlock> sgl;
  Lin x_in, ctx_in, t1, t2, g1, g2, p1, p2, norm_out, proj_out;
  std::vector<float> rope_host;  // [Nc + Nx, head_dim]: cos | sin per row
  const float* rope = nullptr;
  // an engine made by smi_flux_train_create: transposed copies of the Linears on the gradient path, and arena 1 for the
  // saved pass and its backward
  bool trainable = false;
  Ten* out_rows = nullptr;  // proj_out's output of the saved pass: where the backward starts
  Flux(const smi_flux_config& c, int h, int w, bool train = false) : cfg(c), H(h), W(w), trainable(train) {}
  int d() const { return cfg.num_heads * cfg.attention_head_dim; }
  int gh() const { return H / cfg.patch_size; }
  int gw() const { return W / cfg.patch_size; }

  const void* rms_weight(smi_engine& e, const std::string& name) {
    e.check_shape(name, {cfg.attention_head_dim});
    return e.Wd(name);
  }

  // cos | sin of the angles id_a / theta^(2 j / D_a), the three axes one after the other: image token (row, col) has ids
  // (0, row, col), a text token (0, 0, 0); joint row = context rows, then image rows.  Angles in float64
  void build_rope() {
    const int D = cfg.attention_head_dim, Nc = cfg.context_len, L = Nc + gh() * gw();
    rope_host.assign((size_t)L * D, 0.f);
    for (int r = 0; r < L; ++r) {
      const int t = r - Nc;
      const int ids[3] = {0, t >= 0 ? t / gw() : 0, t >= 0 ? t % gw() : 0};
      int col = 0;
      for (int a = 0; a < 3; ++a) {
        const int Da = cfg.axes_dims_rope[a];
        for (int j = 0; j < Da / 2; ++j, ++col) {
          const double ang = (double)ids[a] / std::pow((double)cfg.rope_theta, 2.0 * j / Da);
          rope_host[(size_t)r * D + col] = (float)std::cos(ang);
          rope_host[(size_t)r * D + D / 2 + col] = (float)std::sin(ang);
        }
      }
    }
  }

  void build(smi_engine& e) override {
    const int D = d(), K = cfg.in_channels * cfg.patch_size * cfg.patch_size;
    const bool T = trainable;
    x_in = e.make_lin("x_embedder", K, D, true, false);
    ctx_in = e.make_lin("context_embedder", cfg.joint_attention_dim, D, true, false);
    t1 = e.make_lin("time_text_embed.timestep_embedder.linear_1", 256, D, true, false);
    t2 = e.make_lin("time_text_embed.timestep_embedder.linear_2", D, D, true, false);
    if (cfg.guidance_embeds) {
      g1 = e.make_lin("time_text_embed.guidance_embedder.linear_1", 256, D, true, false);
      g2 = e.make_lin("time_text_embed.guidance_embedder.linear_2", D, D, true, false);
    }
    p1 = e.make_lin("time_text_embed.text_embedder.linear_1", cfg.pooled_projection_dim, D, true, false);
    p2 = e.make_lin("time_text_embed.text_embedder.linear_2", D, D, true, false);
    dbl.resize(cfg.num_layers);
    for (int i = 0; i < cfg.num_layers; ++i) {
      const std::string b = "transformer_blocks." + std::to_string(i);
      DoubleBlock& B = dbl[i];
      B.x.mod = e.make_lin(b + ".norm1.linear", D, 6 * D, true, false);
      B.x.qkv = e.make_fused(b + ".attn", {"to_q", "to_k", "to_v"}, D, D, T);
      B.x.qkv.b = e.fused_bias(b + ".attn", {"to_q", "to_k", "to_v"}, D);
      B.x.nq = rms_weight(e, b + ".attn.norm_q.weight");
      B.x.nk = rms_weight(e, b + ".attn.norm_k.weight");
      B.x.out = e.make_lin(b + ".attn.to_out.0", D, D, true, T, true);
      B.x.ff1 = e.make_lin(b + ".ff.net.0.proj", D, 4 * D, true, T);
      B.x.ff2 = e.make_lin(b + ".ff.net.2", 4 * D, D, true, T);
      B.c.mod = e.make_lin(b + ".norm1_context.linear", D, 6 * D, true, false);
      B.c.qkv = e.make_fused(b + ".attn", {"add_q_proj", "add_k_proj", "add_v_proj"}, D, D, T);
      B.c.qkv.b = e.fused_bias(b + ".attn", {"add_q_proj", "add_k_proj", "add_v_proj"}, D);
      B.c.nq = rms_weight(e, b + ".attn.norm_added_q.weight");
      B.c.nk = rms_weight(e, b + ".attn.norm_added_k.weight");
      B.c.out = e.make_lin(b + ".attn.to_add_out", D, D, true, T, true);
      B.c.ff1 = e.make_lin(b + ".ff_context.net.0.proj", D, 4 * D, true, T);
      B.c.ff2 = e.make_lin(b + ".ff_context.net.2", 4 * D, D, true, T);
    }
    sgl.resize(cfg.num_single_layers);
    for (int i = 0; i < cfg.num_single_layers; ++i) {
      const std::string b = "single_transformer_blocks." + std::to_string(i);
      SingleBlock& S = sgl[i];
      S.mod = e.make_lin(b + ".norm.linear", D, 3 * D, true, false);
      S.qkv = e.make_fused(b + ".attn", {"to_q", "to_k", "to_v"}, D, D, T);
      S.qkv.b = e.fused_bias(b + ".attn", {"to_q", "to_k", "to_v"}, D);
      S.nq = rms_weight(e, b + ".attn.norm_q.weight");
      S.nk = rms_weight(e, b + ".attn.norm_k.weight");
      S.mlp = e.make_lin(b + ".proj_mlp", D, 4 * D, true, T);
      S.out = e.make_lin(b + ".proj_out", 5 * D, D, true, T);
    }
    norm_out = e.make_lin("norm_out.linear", D, 2 * D, true, false);
    proj_out = e.make_lin("proj_out", D, K, true, T);
    // the rotary table: built once, on the host; no trigonometry runs on the device
    if (!e.dry) build_rope();
    const size_t rope_bytes = (size_t)(cfg.context_len + gh() * gw()) * cfg.attention_head_dim * sizeof(float);
    rope = (const float*)e.pack_alloc(rope_bytes);
    if (!e.dry && !e.err)  // (rope_host lives as long as the engine; finish_create waits for the stream)
      (void)hipMemcpyAsync((void*)rope, rope_host.data(), rope_bytes, hipMemcpyHostToDevice, e.stream);
    e.samp_mult_dev = (float*)e.pack_alloc(2 * e.MAXS * sizeof(float));
    for (size_t i = 0; i < e.sites.size(); ++i)
      if (!e.site_used[i] && !e.err) {
        set_error("LoRA target '%s' is not an attention projection of this transformer", e.site_names[i].c_str());
        e.err = true;
      }
  }
  // what the engine packs after the layers, in the order a forward-only engine always packed them (a backward keeps its
  // per-sample loss scales in the whole block)
  void build_all(smi_engine& e) {
    build(e);
    e.gscale = (float*)e.pack_alloc((trainable ? (size_t)e.GSCALE_FLOATS : 256) * sizeof(float));
    e.finish_lora();
    // a fused q|k|v pushes at most 4 jobs for its 3 sites, an output projection 2
    if (trainable) e.alloc_job_table(2 * e.sites.size() + 8);
  }
  void dry_forward(smi_engine& e) override {
    forward(e, e.max_n, nullptr, nullptr, nullptr, (void*)16, (void*)16, (float*)16);
  }

  // a 256-wide sinusoid of n host values through its two-Linear embedder (+ res in the second GEMM's epilogue)
  Ten* embed_scalar(smi_engine& e, int n, const float* host, float mul, const Lin& l1, const Lin& l2, Ten* res) {
    float* vals = e.alloc_f32(n);
    if (!e.dry && !e.err) {
      std::vector<float> v(n);
      for (int i = 0; i < n; ++i) v[i] = host[i] * mul;
      if (e.upload_floats(vals, nullptr, v.data(), n, 1.f) != 0) e.err = true;  // (by kernel argument: v may go)
    }
    Ten* s = e.new_ten(n, 256, n, 1, 1);
    RUN(launch_timestep_embed(e.dtype, vals, s->p, n, 256, e.stream));
    return e.linear(e.silu(e.linear(s, l1)), l2, res);
  }

  // src's q and k heads normalised and rotated (v copied) into rows [row_off, row_off + tokens) of joint; src == joint: in place.
  // In a saved pass (never in place) the backward turns those rows of joint's gradient into src's: the split of the joint
  // gradient, where two streams share the tensor
  void norm_rope(smi_engine& e, Ten* src, Ten* joint, const void* wq, const void* wk, int n, int tokens, int L, int row_off) {
    const int D = cfg.attention_head_dim, heads = cfg.num_heads;
    RUNP(SMI_PROF_ELEM, 0.0, (src == joint ? 8.0 : 12.0) * src->rows * d(),
         launch_qk_norm_rope(e.dtype, src->p, src->cols, joint->p, joint->cols, wq, wk, rope, n, tokens, L, row_off, heads, D,
                             1e-6f, e.stream));
    if (src == joint) return;
    joint->ng = joint->ng || src->ng;
    if (e.saving && src->ng) {
      smi_engine* ep = &e;
      const float* table = rope;
      e.tape.push_back([=]() {
        smi_engine& e = *ep;
        if (!joint->g) return;
        const int n0 = e.ad_first(joint, L);
        void* ds = e.grad_slot(src).out;  // src has this one consumer: the slot is fresh (taken outside the launch macro)
        RUNP(SMI_PROF_ELEM, 0.0, 18.0 * e.MA(src) * src->cols / 3,
             launch_qk_norm_rope_bwd(e.dtype, joint->g, joint->cols, e.PA(src), src->cols, ds, src->cols, wq, wk, table, n - n0,
                                     tokens, L, row_off, heads, D, 1e-6f, e.stream));
      });
    }
  }

  // one stream of a double block after the attention: gated attention output, then the gated feed-forward
  Ten* stream_tail(smi_engine& e, Ten* h, Ten* attn, Ten* mod, const Stream& s) {
    const int D = d();
    h = gate_residual(e, h, e.linear(attn, s.out), mod, 2 * D);
    Ten* f = e.linear(e.act(e.linear(adaln(e, h, mod, 4 * D, 3 * D), s.ff1), 2), s.ff2);
    return gate_residual(e, h, f, mod, 5 * D);
  }

  int forward(smi_engine& e, int n, const float* sample, const float* timesteps_host, const float* guidance_host, const void* ctx,
              const void* pooled, float* out, bool save = false) {
    const int D = d(), P = cfg.patch_size, Nx = gh() * gw(), Nc = cfg.context_len, L = Nc + Nx, heads = cfg.num_heads;
    e.begin_pass(n, save);
    if (!e.prep_sites.empty() && (e.dry || (e.lora_down && e.lora_up && e.mult != 0.f)))
      RUNP(SMI_PROF_LORA, 0.0, 0.0, launch_lora_prep(e.dtype, e.prep_sites_dev, (int)e.prep_sites.size(), e.lora_down, e.lora_up, e.lora_shadow, e.stream));

    // ---- temb = time (+ guidance) + text, summed in that order; every modulation reads silu(temb)
    Ten* te = embed_scalar(e, n, timesteps_host, 1.f, t1, t2, nullptr);
    if (cfg.guidance_embeds) te = embed_scalar(e, n, guidance_host, 1000.f, g1, g2, te);
    Ten* pl = e.borrowed(pooled, n, cfg.pooled_projection_dim, n, 1, 1);
    Ten* st = e.silu(e.linear(e.silu(e.linear(pl, p1)), p2, te));

    // ---- the two streams' inputs (no position table: positions enter through the rotation of q and k)
    Ten* pm = e.new_ten((int64_t)n * Nx, x_in.in, n, Nx, 1);
    RUN(launch_sd3_patchify(e.dtype, sample, pm->p, n, cfg.in_channels, H, W, P, e.stream));
    Ten* x = e.linear(pm, x_in);
    Ten* ci = e.borrowed(ctx, (int64_t)n * Nc, cfg.joint_attention_dim, n, Nc, 1);
    Ten* c = e.linear(ci, ctx_in);

    // ---- double blocks; block k allocates from scratch region k & 1 and reads block k - 1's outputs in the other one
    for (const DoubleBlock& B : dbl) {
      e.begin_block();
      Ten* mx = e.linear(st, B.x.mod);  // shift_msa | scale_msa | gate_msa | shift_mlp | scale_mlp | gate_mlp
      Ten* mc = e.linear(st, B.c.mod);
      Ten* qx = e.linear(adaln(e, x, mx, D, 0), B.x.qkv);
      Ten* qc = e.linear(adaln(e, c, mc, D, 0), B.c.qkv);
      Ten* j = e.new_ten((int64_t)n * L, 3 * D, n, L, 1);
      norm_rope(e, qc, j, B.c.nq, B.c.nk, n, Nc, L, 0);
      norm_rope(e, qx, j, B.x.nq, B.x.nk, n, Nx, L, Nc);
      Ten* o = e.attention(j, nullptr, nullptr, heads, D, n, L, L, false);
      Ten *oc, *ox;
      joint_split(e, o, Nc, Nx, &oc, &ox, true);  // (context rows first)
      x = stream_tail(e, x, ox, mx, B.x);
      c = stream_tail(e, c, oc, mc, B.c);
      e.end_block();
    }

    // ---- single blocks on the joint sequence, context rows first
    e.begin_block();
    Ten* s = joint_pack(e, c, x);
    e.end_block();
    for (const SingleBlock& S : sgl) {
      e.begin_block();
      Ten* m = e.linear(st, S.mod);  // shift | scale | gate
      Ten* z = adaln(e, s, m, D, 0);
      Ten* qkv = e.linear(z, S.qkv);
      if (save) {  // out of place: the backward reads the pre-norm q|k|v
        Ten* j = e.new_ten(s->rows, 3 * D, n, L, 1);
        norm_rope(e, qkv, j, S.nq, S.nk, n, L, L, 0);
        qkv = j;
      } else {
        norm_rope(e, qkv, qkv, S.nq, S.nk, n, L, L, 0);
      }
      // [attention | gelu_tanh(proj_mlp z)], each producer writing its own columns
      Ten* am = e.new_ten(s->rows, 5 * D, n, L, 1);
      AttnParams p;
      p.dtype = e.dtype;
      p.B = n;
      p.H = heads;
      p.Nq = p.Nk = L;
      p.D = cfg.attention_head_dim;
      p.scale = 1.f / sqrtf((float)p.D);
      p.Q = qkv->p;
      p.K = (char*)qkv->p + (size_t)D * e.esz();
      p.V = (char*)qkv->p + (size_t)2 * D * e.esz();
      p.ldq = p.ldk = p.ldv = 3 * D;
      p.O = am->p;
      p.ldo = 5 * D;
      p.lse = e.alloc_f32((size_t)n * heads * L);
      RUNP(SMI_PROF_ATTN, 4.0 * n * heads * (double)L * L * p.D, 0.0, launch_attn_fwd(p, e.stream));
      char* mcol = (char*)am->p + (size_t)D * e.esz();
      if (save) {
        // the pre-activation in a tensor of its own (the Linear pushes its own backward), tanh-GELU from it into am's columns
        Ten* pre = e.linear(z, S.mlp);
        RUNP(SMI_PROF_ELEM, 0.0, 16.0 * z->rows * D, launch_gelu_tanh_cols(e.dtype, pre->p, 4 * D, mcol, 5 * D, z->rows, 4 * D, e.stream));
        am->ng = qkv->ng || pre->ng;
        if (am->ng) single_block_tape(e, am, qkv, pre, p);
      } else {
        const GemmParams g = gemm_nt(e.dtype, z->p, D, S.mlp.W, mcol, 5 * D, (int)z->rows, 4 * D, D).with_bias(S.mlp.b);
        e.run_gemm(SMI_PROF_GEMM, g, e.gemm_flops(g), e.gemm_bytes(g), true, "proj_mlp");
        RUNP(SMI_PROF_ELEM, 0.0, 16.0 * z->rows * D, launch_gelu_tanh_cols(e.dtype, mcol, 5 * D, mcol, 5 * D, z->rows, 4 * D, e.stream));
      }
      s = gate_residual(e, s, e.linear(am, S.out), m, 2 * D);
      e.end_block();
    }

    // ---- output: the image rows (the last Nx of each sample), LN(x) (1 + scale) + shift, proj_out, un-pack
    e.begin_block();
    Ten* xo = e.new_ten((int64_t)n * Nx, D, n, Nx, 1);
    RUNP(SMI_PROF_ELEM, 0.0, 4.0 * xo->rows * D, launch_joint_rows_split(e.dtype, s->p, nullptr, xo->p, n, Nc, Nx, D, e.stream));
    xo->ng = s->ng;
    if (e.saving && xo->ng) {
      smi_engine* ep = &e;
      e.tape.push_back([=]() {  // the pack of the image rows' gradient under zero context rows
        smi_engine& e = *ep;
        if (!xo->g) return;
        const int n0 = e.ad_first(s, L);
        void* zc = e.alloc_t((int64_t)(n - n0) * Nc, D);
        if (!e.dry && !e.err) (void)hipMemsetAsync(zc, 0, (size_t)(n - n0) * Nc * D * e.esz(), e.stream);
        e.into_slot(e.grad_slot(s), e.MA(s), D, [&](void* ds) {
          RUNP(SMI_PROF_ELEM, 0.0, 4.0 * e.MA(s) * D, launch_joint_rows_pack(e.dtype, zc, xo->g, ds, n - n0, Nc, Nx, D, e.stream));
        });
      });
    }
    Ten* mo = e.linear(st, norm_out);
    Ten* y = e.linear(adaln(e, xo, mo, 0, D), proj_out);
    RUN(launch_flux_unpack(e.dtype, y->p, out, n, cfg.in_channels, gh(), gw(), P, e.stream));
    e.end_block();
    if (save) {
      e.saving = false;
      out_rows = y;
      e.keep_saved_pass(n);
    }
    if (!save && !e.dry && (e.scr[0].overflow || e.scr[1].overflow)) e.err = true;
    return e.end_pass("this call (");
  }

  // a saved single block's two producers of am [rows, 5 d], backwards (the tape runs in reverse: tanh-GELU's first, then the
  // attention's): d(am)'s columns [0, d) are the attention's dO at leading dimension 5 d, as O is; its columns [d, 5 d) times
  // gelu_tanh'(pre) are the dense gradient of proj_mlp's output
  void single_block_tape(smi_engine& e, Ten* am, Ten* j, Ten* pre, const AttnParams& p) {
    const int D = d(), heads = cfg.num_heads, L = p.Nq, nbatch = p.B;
    smi_engine* ep = &e;
    if (j->ng)
      e.tape.push_back([=]() {
        smi_engine& e = *ep;
        if (!am->g) return;
        AttnParams b = p;
        const int b0 = e.ad_first(am, L);
        b.B = nbatch - b0;
        b.Q = (const char*)p.Q + (size_t)b0 * L * p.ldq * e.esz();
        b.K = (const char*)p.K + (size_t)b0 * L * p.ldk * e.esz();
        b.V = (const char*)p.V + (size_t)b0 * L * p.ldv * e.esz();
        b.O = e.PA(am);
        b.lse = p.lse + (size_t)b0 * heads * L;
        b.dO = am->g;
        b.lddo = 5 * D;
        b.delta = e.alloc_f32((size_t)b.B * heads * L);
        char* g = (char*)e.grad_slot(j).out;  // the joint q|k|v has this one consumer: the slot is fresh
        b.dQ = g;
        b.dK = g + (size_t)D * e.esz();
        b.dV = g + (size_t)2 * D * e.esz();
        b.lddq = b.lddk = b.lddv = 3 * D;
        RUNP(SMI_PROF_ATTN, 10.0 * b.B * heads * (double)L * L * b.D, 0.0, launch_attn_bwd(b, e.stream));
      });
    if (pre->ng)
      e.tape.push_back([=]() {
        smi_engine& e = *ep;
        if (!am->g) return;
        void* dp = e.grad_slot(pre).out;  // one consumer
        RUNP(SMI_PROF_ELEM, 0.0, 24.0 * e.MA(pre) * D,
             launch_gelu_tanh_cols_bwd(e.dtype, e.PA(pre), 4 * D, (const char*)am->g + (size_t)D * e.esz(), 5 * D, dp, 4 * D,
                                       e.MA(pre), 4 * D, e.stream));
      });
  }

  // the shared backward (engine.h) with this model's part: one power-of-two loss scale per sample from d_out, and
  // flux_unpack's inverse into the gradient of proj_out's rows (+= into dd / du).  A backward consumes the saved pass
  int backward(smi_engine& e, const float* d_out, float* dd, float* du) {
    if (const int rc = e.begin_backward("smi_flux_backward: no saved forward pass (call smi_flux_forward_save first)", dd, du, e.saved.n))
      return rc;
    Ten* y = out_rows;
    if (!y->ng || (!e.dry && (!dd || !du))) {  // adaptor off in the saved pass, or no buffers to add to: nothing to do
      e.drop_tape();
      return 0;
    }
    const int n = e.saved.n;
    RUN(launch_grad_scale(d_out, n, (int64_t)cfg.in_channels * H * W, e.gscale, e.MAXS, e.stream));
    e.rebuild_saved_operands();
    y->g = e.alloc_t(e.MA(y), y->cols);
    RUN(launch_flux_unpack_bwd(e.dtype, d_out, y->g, n, cfg.in_channels, gh(), gw(), cfg.patch_size, e.gscale, e.stream));
    if (e.run_tape_and_weight_grads()) return -1;
    return e.end_pass("the backward (");
  }
};

int check_flux(const smi_flux_config* c, const smi_lora_site* sites, int n_sites, int batch, int h, int w) {
  SMI_CHECK(c != nullptr, "config is NULL");
  SMI_CHECK(c->dtype == SMI_DTYPE_F16 || c->dtype == SMI_DTYPE_BF16, "dtype must be f16 (0) or bf16 (1)");
  SMI_CHECK(c->num_heads >= 1 && c->num_layers >= 1 && c->num_single_layers >= 1 && batch >= 1,
            "Flux config: num_heads, num_layers, num_single_layers and batch must be >= 1");
  const int D = c->attention_head_dim;
  SMI_CHECK(D >= 16 && D % 16 == 0 && D <= 160,
            "Flux config: attention_head_dim %d must be a multiple of 16 and at most 160 (qk_norm_rope and the attention)", D);
  for (int a = 0; a < 3; ++a)
    SMI_CHECK(c->axes_dims_rope[a] >= 0 && c->axes_dims_rope[a] % 2 == 0,
              "Flux config: axes_dims_rope[%d] = %d is odd (an axis is rotated in pairs)", a, c->axes_dims_rope[a]);
  SMI_CHECK(c->axes_dims_rope[0] + c->axes_dims_rope[1] + c->axes_dims_rope[2] == D,
            "Flux config: sum(axes_dims_rope) = %d is not attention_head_dim %d",
            c->axes_dims_rope[0] + c->axes_dims_rope[1] + c->axes_dims_rope[2], D);
  SMI_CHECK(c->rope_theta > 1.f, "Flux config: rope_theta %g must be > 1", (double)c->rope_theta);
  const int d = c->num_heads * D;
  SMI_CHECK(d % 64 == 0 && d <= 3072, "Flux config: width %d must be a multiple of 64 and <= 3072 (d %% 64; the adaLN rows)", d);
  SMI_CHECK(c->patch_size >= 1 && c->in_channels >= 1 && (c->in_channels * c->patch_size * c->patch_size) % 64 == 0,
            "Flux config: in_channels x patch_size^2 = %d must be a multiple of 64 (the packed width, x_embedder's K)",
            c->in_channels * c->patch_size * c->patch_size);
  SMI_CHECK(c->patch_size == 2, "Flux config: patch_size %d: the pack is 2 x 2", c->patch_size);
  SMI_CHECK(h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, "Flux: latent %d x %d: h and w must be even (odd h or w cannot be packed)", h, w);
  SMI_CHECK(c->joint_attention_dim >= 8 && c->joint_attention_dim % 8 == 0 && c->pooled_projection_dim >= 8 &&
                c->pooled_projection_dim % 8 == 0 && c->context_len >= 1,
            "Flux config: joint_attention_dim %% 8, pooled_projection_dim %% 8, context_len >= 1");
  SMI_CHECK(c->guidance_embeds == 0 || c->guidance_embeds == 1, "Flux config: guidance_embeds must be 0 or 1");
  SMI_CHECK(batch <= smi_engine::MAXS, "Flux: batch %d exceeds the %d per-sample multipliers", batch, smi_engine::MAXS);
  SMI_CHECK(n_sites == 0 || sites, "Flux: n_sites %d without sites", n_sites);
  return check_linear_lora_sites("Flux", sites, n_sites,
                                 {".attn.to_q", ".attn.to_k", ".attn.to_v", ".attn.to_out.0", ".attn.add_q_proj",
                                  ".attn.add_k_proj", ".attn.add_v_proj", ".attn.to_add_out"},
                                 "the attention projections (attn.to_q/to_k/to_v of double and single blocks, attn.to_out.0, "
                                 "attn.add_q_proj/add_k_proj/add_v_proj/to_add_out) only");
}

Flux* flux_setup(smi_engine* e, const smi_flux_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int h, int w,
                 bool train) {
  Flux* m = new Flux(*cfg, h, w, train);
  e->hold(smi_engine::FLUX, m, cfg->dtype, batch);
  e->register_sites(sites, n_sites);
  return m;
}
// dry run: out = {packed weights, persistent region of arena 0, one scratch region, arena 1}; arena 0 is out[1] + 2 out[2];
// out[3] (a saved pass and its backward) is 0 unless the engine is trainable
int flux_plan(const smi_flux_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int h, int w, size_t out[4],
              bool train) {
  smi_engine e;
  e.dry = true;
  Flux& m = *flux_setup(&e, cfg, sites, n_sites, batch, h, w, train);
  m.build_all(e);
  if (e.err) return -1;
  out[0] = align_up(e.wpack.peak, 4096);
  m.dry_forward(e);
  out[1] = align_up(e.arena[0].peak, 4096);
  out[2] = align_up(std::max(e.scr[0].peak, e.scr[1].peak), 4096);
  out[3] = 0;
  if (train) {
    m.forward(e, batch, nullptr, nullptr, nullptr, (void*)16, (void*)16, (float*)16, true);
    m.backward(e, nullptr, nullptr, nullptr);
    out[3] = align_up(e.arena[1].peak, 4096);
  }
  return e.err ? -1 : 0;
}
// (without arena 1: the bytes a forward-only engine always took)
size_t plan_bytes(const size_t r[4]) { return r[0] + r[1] + 2 * r[2] + 2 * 4096 + (r[3] ? r[3] + 4096 : 0); }

int check_flux_train(const smi_flux_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int h, int w) {
  if (check_flux(cfg, sites, n_sites, batch, h, w)) return -1;
  SMI_CHECK(sites && n_sites > 0, "smi_flux_train: n_sites 0 -- no LoRA sites to train (a frozen network is smi_flux_create's)");
  return 0;
}

int flux_workspace(bool train, const smi_flux_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int h, int w,
                   size_t* bytes) {
  SMI_CHECK(bytes != nullptr, "bad arguments");
  size_t r[4];
  if (flux_plan(cfg, sites, n_sites, batch, h, w, r, train)) return -1;
  *bytes = plan_bytes(r);
  return 0;
}

// both create entries: train says which
int flux_create(bool train, const smi_flux_config* cfg, const smi_weight* weights, int n_weights, const smi_lora_site* sites,
                int n_sites, int batch, int h, int w, void* workspace, size_t workspace_bytes, void* stream, smi_engine** out) {
  SMI_CHECK(out && workspace && weights && n_weights > 0, "bad arguments");
  size_t r[4];
  if (flux_plan(cfg, sites, n_sites, batch, h, w, r, train)) return -1;
  SMI_CHECK(plan_bytes(r) <= workspace_bytes, "workspace too small: need %zu bytes, got %zu", plan_bytes(r), workspace_bytes);
  smi_engine* e = new smi_engine();
  e->stream = (hipStream_t)stream;
  Flux* m = flux_setup(e, cfg, sites, n_sites, batch, h, w, train);
  for (int i = 0; i < n_weights; ++i) e->wmap[weights[i].name] = &weights[i];
  char* base = (char*)align_up((size_t)workspace, 4096);
  e->wpack.base = base;
  e->wpack.cap = r[0];
  e->arena[0].base = base + r[0];
  e->set_arena0_regions(r[1], r[2]);
  e->arena[1].base = base + r[0] + r[1] + 2 * r[2];
  e->arena[1].cap = r[3];
  m->build_all(*e);
  return finish_create(e, "the Flux weights", out);
}

// smi_flux_forward / smi_flux_forward_save: the adaptor's state from the arguments, then the pass
int flux_run(smi_engine* e, const char* who, int n, const float* sample, const float* timesteps, const float* guidance,
             const void* ctx, const void* pooled, const float* lora_down_flat, const float* lora_up_flat, const float* multipliers,
             float* out, bool save) {
  SMI_CHECK(e && e->kind == smi_engine::FLUX, "%s: NULL or not a Flux engine (create it with smi_flux_create)", who);
  Flux* m = static_cast<Flux*>(e->model.get());
  SMI_CHECK(!save || m->trainable, "%s: this engine keeps no pass (create it with smi_flux_train_create)", who);
  SMI_CHECK(sample && timesteps && ctx && pooled && out, "%s: sample, timesteps, ctx, pooled and out are required", who);
  SMI_CHECK(!m->cfg.guidance_embeds || guidance,
            "%s: guidance is NULL but the model has guidance_embeds = 1 (a guidance value per sample is required)", who);
  SMI_CHECK(m->cfg.guidance_embeds || !guidance,
            "%s: guidance given but the model has guidance_embeds = 0 (it has no guidance embedder)", who);
  SMI_CHECK(n >= 1 && n <= e->max_n, "batch %d outside [1, %d] the engine was created for", n, e->max_n);
  e->err = false;
  // the adaptor's state, as smi_mmdit_forward sets it: on when both flat buffers and the multipliers are given and one
  // multiplier is not 0; every adapted pass takes the per-sample route, so a sample gives the same bits alone and in a batch
  float mref = 0.f;
  if (lora_down_flat && lora_up_flat && multipliers && !e->prep_sites.empty())
    if (const int rc = e->set_sample_multipliers(multipliers, n, save, &mref)) return rc;
  e->lora_down = mref != 0.f ? lora_down_flat : nullptr;
  e->lora_up = mref != 0.f ? lora_up_flat : nullptr;
  e->mult = mref;
  e->samp_on = mref != 0.f;
  // no split-K scratch is lent: the slice count follows the launch's row count, so with one a sample's bits would depend on
  // its batch
  smi::set_gemm_scratch(nullptr, 0);
  const int rc = m->forward(*e, n, sample, timesteps, guidance, ctx, pooled, out, save);
  e->samp_on = false;
  return rc;
}

}  // namespace

extern "C" {

int smi_flux_workspace_bytes(const smi_flux_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int h, int w,
                             size_t* bytes) {
  if (check_flux(cfg, sites, n_sites, batch, h, w)) return -1;
  return flux_workspace(false, cfg, sites, n_sites, batch, h, w, bytes);
}

int smi_flux_train_workspace_bytes(const smi_flux_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int h, int w,
                                   size_t* bytes) {
  if (check_flux_train(cfg, sites, n_sites, batch, h, w)) return -1;
  return flux_workspace(true, cfg, sites, n_sites, batch, h, w, bytes);
}

int smi_flux_create(const smi_flux_config* cfg, const smi_weight* weights, int n_weights, const smi_lora_site* sites,
                    int n_sites, int batch, int h, int w, void* workspace, size_t workspace_bytes, void* stream,
                    smi_engine** out) {
  if (check_flux(cfg, sites, n_sites, batch, h, w)) return -1;
  return flux_create(false, cfg, weights, n_weights, sites, n_sites, batch, h, w, workspace, workspace_bytes, stream, out);
}

int smi_flux_train_create(const smi_flux_config* cfg, const smi_weight* weights, int n_weights, const smi_lora_site* sites,
                          int n_sites, int batch, int h, int w, void* workspace, size_t workspace_bytes, void* stream,
                          smi_engine** out) {
  if (check_flux_train(cfg, sites, n_sites, batch, h, w)) return -1;
  return flux_create(true, cfg, weights, n_weights, sites, n_sites, batch, h, w, workspace, workspace_bytes, stream, out);
}

int smi_flux_forward(smi_engine* e, int n, const float* sample, const float* timesteps, const float* guidance,
                     const void* ctx, const void* pooled, const float* lora_down_flat, const float* lora_up_flat,
                     const float* multipliers, float* out) {
  return flux_run(e, "smi_flux_forward", n, sample, timesteps, guidance, ctx, pooled, lora_down_flat, lora_up_flat, multipliers,
                  out, false);
}

int smi_flux_forward_save(smi_engine* e, int n, const float* sample, const float* timesteps, const float* guidance,
                          const void* ctx, const void* pooled, const float* lora_down_flat, const float* lora_up_flat,
                          const float* multipliers, float* out) {
  return flux_run(e, "smi_flux_forward_save", n, sample, timesteps, guidance, ctx, pooled, lora_down_flat, lora_up_flat,
                  multipliers, out, true);
}

int smi_flux_backward(smi_engine* e, const float* d_out, float* d_lora_down_flat, float* d_lora_up_flat) {
  SMI_CHECK(e && e->kind == smi_engine::FLUX && d_out, "smi_flux_backward: NULL argument or not a Flux engine");
  Flux* m = static_cast<Flux*>(e->model.get());
  SMI_CHECK(m->trainable, "smi_flux_backward: this engine keeps no pass (create it with smi_flux_train_create)");
  e->err = false;
  smi::set_gemm_scratch(nullptr, 0);
  return m->backward(*e, d_out, d_lora_down_flat, d_lora_up_flat);
}

}  // extern "C"
