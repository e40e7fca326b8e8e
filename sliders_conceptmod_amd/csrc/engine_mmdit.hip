// The SD3 MMDiT engine (diffusers SD3Transformer2DModel, SD3-medium's family): patch embedding with the centre-cropped
// position table, the conditioning vector temb = time MLP + pooled-text MLP, joint blocks -- an image stream and a context
// stream, each under adaLN-Zero modulation of temb, meeting in ONE attention over the packed (image | context) sequence --
// and the modulated output projection, un-patchified.  On the op core (engine.h); Linear LoRA sites on the attention
// projections at one multiplier per sample, as the CLIP text tower takes them.  An engine made by smi_mmdit_train_create also
// saves a pass and differentiates it to the LoRA parameters (MMDiT::backward).
//
// The four ops this model adds to the core's (adaln, gate_residual, joint_pack, joint_split) are the free functions of
// engine_joint_ops.h, which the Flux engine shares.
#include "engine_joint_ops.h"

namespace {

// ---- the model --------------------------------------------------------------------------------------------------------
struct Stream {  // one stream's half of a joint block
  Lin mod;       // norm1.linear / norm1_context.linear: [6d, d], or [2d, d] (scale | shift) in a context_pre_only block
  Lin qkv, out, ff1, ff2;
};
struct JointBlock {
  Stream x, c;
  bool pre_only = false;  // the last block: its context stream ends at the attention
};

struct MMDiT : Model {
  smi_mmdit_config cfg{};
  int H = 0, W = 0;  // latent size
  std::vector<JointBlock> blocks;
  Lin patch, ctx_in, t1, t2, p1, p2, norm_out, proj_out;
  const void* pos = nullptr;
  // an engine made by smi_mmdit_train_create: transposed copies of the Linears on the gradient path, and arena 1 for the
  // saved pass and its backward
  bool trainable = false;
  Ten* out_rows = nullptr;  // proj_out's output of the saved pass: where the backward starts
  MMDiT(const smi_mmdit_config& c, int h, int w, bool train = false) : cfg(c), H(h), W(w), trainable(train) {}
  int d() const { return cfg.num_heads * cfg.attention_head_dim; }
  int gh() const { return H / cfg.patch_size; }
  int gw() const { return W / cfg.patch_size; }

  void build(smi_engine& e) override {
    const int D = d(), P = cfg.patch_size, K = cfg.in_channels * P * P, S = cfg.pos_embed_max_size;
    // pos_embed.proj.weight [d, Cin, P, P] is [d, K] with K in (c, py, px) order: the patch GEMM's B operand as it is
    patch.name = "pos_embed.proj";
    patch.in = K;
    patch.out = D;
    patch.W = e.Wd("pos_embed.proj.weight");
    patch.b = e.Wd("pos_embed.proj.bias");
    e.check_shape("pos_embed.proj.weight", {D, cfg.in_channels, P, P});
    pos = e.Wd("pos_embed.pos_embed");
    e.check_shape("pos_embed.pos_embed", {(int64_t)S * S, D});
    ctx_in = e.make_lin("context_embedder", cfg.joint_attention_dim, D, true, false);
    t1 = e.make_lin("time_text_embed.timestep_embedder.linear_1", 256, D, true, false);
    t2 = e.make_lin("time_text_embed.timestep_embedder.linear_2", D, D, true, false);
    p1 = e.make_lin("time_text_embed.text_embedder.linear_1", cfg.pooled_projection_dim, D, true, false);
    p2 = e.make_lin("time_text_embed.text_embedder.linear_2", D, D, true, false);
    blocks.resize(cfg.num_layers);
    for (int i = 0; i < cfg.num_layers; ++i) {
      const std::string b = "transformer_blocks." + std::to_string(i);
      JointBlock& B = blocks[i];
      B.pre_only = i == cfg.num_layers - 1;
      B.x.mod = e.make_lin(b + ".norm1.linear", D, 6 * D, true, false);
      B.x.qkv = e.make_fused(b + ".attn", {"to_q", "to_k", "to_v"}, D, D, trainable);
      B.x.qkv.b = e.fused_bias(b + ".attn", {"to_q", "to_k", "to_v"}, D);
      B.x.out = e.make_lin(b + ".attn.to_out.0", D, D, true, trainable, true);
      B.x.ff1 = e.make_lin(b + ".ff.net.0.proj", D, 4 * D, true, trainable);
      B.x.ff2 = e.make_lin(b + ".ff.net.2", 4 * D, D, true, trainable);
      B.c.mod = e.make_lin(b + ".norm1_context.linear", D, (B.pre_only ? 2 : 6) * D, true, false);
      B.c.qkv = e.make_fused(b + ".attn", {"add_q_proj", "add_k_proj", "add_v_proj"}, D, D, trainable);
      B.c.qkv.b = e.fused_bias(b + ".attn", {"add_q_proj", "add_k_proj", "add_v_proj"}, D);
      if (!B.pre_only) {
        B.c.out = e.make_lin(b + ".attn.to_add_out", D, D, true, trainable, true);
        B.c.ff1 = e.make_lin(b + ".ff_context.net.0.proj", D, 4 * D, true, trainable);
        B.c.ff2 = e.make_lin(b + ".ff_context.net.2", 4 * D, D, true, trainable);
      }
    }
    norm_out = e.make_lin("norm_out.linear", D, 2 * D, true, false);
    proj_out = e.make_lin("proj_out", D, P * P * cfg.out_channels, true, trainable);
  }
  // what the engine packs after the layers
  void build_all(smi_engine& e) {
    build(e);
    e.finish_lora();
    // (a backward keeps its per-sample loss scales in the whole block)
    e.gscale = (float*)e.pack_alloc((trainable ? (size_t)e.GSCALE_FLOATS : 256) * sizeof(float));
    e.samp_mult_dev = (float*)e.pack_alloc(2 * e.MAXS * sizeof(float));
    // a fused q|k|v pushes at most 4 jobs for its 3 sites, an output projection 2
    if (trainable) e.alloc_job_table(2 * e.sites.size() + 8);
    for (size_t i = 0; i < e.sites.size(); ++i)
      if (!e.site_used[i] && !e.err) {
        set_error("LoRA target '%s' is not an attention projection of this transformer", e.site_names[i].c_str());
        e.err = true;
      }
  }
  void dry_forward(smi_engine& e) override {
    forward(e, e.max_n, nullptr, nullptr, (void*)16, (void*)16, (float*)16);
  }

  // one stream of a joint block after the attention: gated attention output, then the gated feed-forward
  Ten* stream_tail(smi_engine& e, Ten* h, Ten* attn, Ten* mod, const Stream& s) {
    const int D = d();
    h = gate_residual(e, h, e.linear(attn, s.out), mod, 2 * D);
    Ten* f = e.linear(e.act(e.linear(adaln(e, h, mod, 4 * D, 3 * D), s.ff1), 2), s.ff2);
    return gate_residual(e, h, f, mod, 5 * D);
  }

  // every sample under the adaptor (e.mult, the per-sample ratios already on the device); save: smi_engine::begin_pass
  int forward(smi_engine& e, int n, const float* sample, const float* timesteps_host, const void* ctx, const void* pooled,
              float* out, bool save = false) {
    const int D = d(), P = cfg.patch_size, Nx = gh() * gw(), Nc = cfg.context_len, heads = cfg.num_heads;
    e.begin_pass(n, save);
    if (!e.prep_sites.empty() && (e.dry || (e.lora_down && e.lora_up && e.mult != 0.f)))
      RUNP(SMI_PROF_LORA, 0.0, 0.0, launch_lora_prep(e.dtype, e.prep_sites_dev, (int)e.prep_sites.size(), e.lora_down, e.lora_up, e.lora_shadow, e.stream));

    // ---- conditioning vector: temb = time MLP(sinusoid(t)) + text MLP(pooled); every modulation reads silu(temb)
    float* tvals = e.alloc_f32(n);
    if (!e.dry && !e.err && e.upload_floats(tvals, nullptr, timesteps_host, n, 1.f) != 0) e.err = true;
    Ten* ts = e.new_ten(n, 256, n, 1, 1);
    RUN(launch_timestep_embed(e.dtype, tvals, ts->p, n, 256, e.stream));
    Ten* te = e.linear(e.silu(e.linear(ts, t1)), t2);
    Ten* pl = e.borrowed(pooled, n, cfg.pooled_projection_dim, n, 1, 1);
    Ten* temb = e.linear(e.silu(e.linear(pl, p1)), p2, te);
    Ten* st = e.silu(temb);

    // ---- the two streams' inputs
    Ten* pm = e.new_ten((int64_t)n * Nx, patch.in, n, Nx, 1);
    RUN(launch_sd3_patchify(e.dtype, sample, pm->p, n, cfg.in_channels, H, W, P, e.stream));
    Ten* pe = e.linear(pm, patch);
    Ten* x = e.new_ten(pe->rows, D, n, Nx, 1);
    RUNP(SMI_PROF_ELEM, 0.0, 4.0 * x->rows * D, launch_sd3_add_pos(e.dtype, pe->p, pos, x->p, n, gh(), gw(), D, cfg.pos_embed_max_size, e.stream));
    Ten* ci = e.borrowed(ctx, (int64_t)n * Nc, cfg.joint_attention_dim, n, Nc, 1);
    Ten* c = e.linear(ci, ctx_in);

    // ---- joint blocks.  Block k allocates from scratch region k & 1 and reads block k - 1's two outputs in the other one
    // (begin_block, engine.h): the arena is the persistent tensors above + 2 x the largest block, not 24 blocks
    for (const JointBlock& B : blocks) {
      e.begin_block();
      Ten* mx = e.linear(st, B.x.mod);  // shift_msa | scale_msa | gate_msa | shift_mlp | scale_mlp | gate_mlp
      Ten* mc = e.linear(st, B.c.mod);  // the same six, or scale | shift in the last block
      Ten* qx = e.linear(adaln(e, x, mx, D, 0), B.x.qkv);
      Ten* qc = e.linear(B.pre_only ? adaln(e, c, mc, 0, D) : adaln(e, c, mc, D, 0), B.c.qkv);
      Ten* o = e.attention(joint_pack(e, qx, qc), nullptr, nullptr, heads, D, n, Nx + Nc, Nx + Nc, false);
      Ten *ox, *oc;
      joint_split(e, o, Nx, Nc, &ox, &oc, !B.pre_only);
      x = stream_tail(e, x, ox, mx, B.x);
      if (!B.pre_only) c = stream_tail(e, c, oc, mc, B.c);
      e.end_block();
    }

    // ---- output: LN(x) (1 + scale) + shift with scale | shift = norm_out.linear(silu(temb)), proj_out, un-patchify
    e.begin_block();
    Ten* mo = e.linear(st, norm_out);
    Ten* y = e.linear(adaln(e, x, mo, 0, D), proj_out);
    RUN(launch_sd3_unpatchify(e.dtype, y->p, out, n, cfg.out_channels, gh(), gw(), P, e.stream));
    e.end_block();
    if (save) {
      e.saving = false;
      out_rows = y;
      e.keep_saved_pass(n);
    }
    if (!save && !e.dry && (e.scr[0].overflow || e.scr[1].overflow)) e.err = true;
    return e.end_pass("this call (");
  }

  // the shared backward (engine.h) with this model's part: one power-of-two loss scale per sample from d_out, and
  // un-patchify's inverse into the gradient of proj_out's rows (+= into dd / du).  A backward consumes the saved pass
  int backward(smi_engine& e, const float* d_out, float* dd, float* du) {
    if (const int rc = e.begin_backward("smi_mmdit_backward: no saved forward pass (call smi_mmdit_forward_save first)", dd, du, e.saved.n))
      return rc;
    Ten* y = out_rows;
    if (!y->ng || (!e.dry && (!dd || !du))) {  // adaptor off in the saved pass, or no buffers to add to: nothing to do
      e.drop_tape();
      return 0;
    }
    const int n = e.saved.n;
    RUN(launch_grad_scale(d_out, n, (int64_t)cfg.out_channels * H * W, e.gscale, e.MAXS, e.stream));
    e.rebuild_saved_operands();
    y->g = e.alloc_t(e.MA(y), y->cols);
    RUN(launch_sd3_unpatchify_bwd(e.dtype, d_out, y->g, n, cfg.out_channels, gh(), gw(), cfg.patch_size, e.gscale, e.stream));
    if (e.run_tape_and_weight_grads()) return -1;
    return e.end_pass("the backward (");
  }
};

int check_mmdit(const smi_mmdit_config* c, const smi_lora_site* sites, int n_sites, int batch, int h, int w) {
  SMI_CHECK(c != nullptr, "config is NULL");
  SMI_CHECK(c->dtype == SMI_DTYPE_F16 || c->dtype == SMI_DTYPE_BF16, "dtype must be f16 (0) or bf16 (1)");
  SMI_CHECK(c->dual_attention_layers == 0,
            "MMDiT config: dual_attention_layers (SD3.5) is not built: %d blocks ask for a second image-only attention",
            c->dual_attention_layers);
  SMI_CHECK(c->qk_norm == 0, "MMDiT config: qk_norm (SD3.5's rms_norm on q and k) is not built");
  SMI_CHECK(c->attention_head_dim == 64, "MMDiT config: attention_head_dim %d: the joint attention takes 64", c->attention_head_dim);
  SMI_CHECK(c->num_heads >= 1 && c->num_layers >= 1 && batch >= 1, "MMDiT config: num_heads, num_layers and batch must be >= 1");
  const int d = c->num_heads * c->attention_head_dim;
  SMI_CHECK(d % 64 == 0 && d <= 2048, "MMDiT config: width %d must be a multiple of 64 and <= 2048", d);
  SMI_CHECK(c->patch_size >= 1 && c->in_channels >= 1 && c->out_channels >= 1 &&
                (c->in_channels * c->patch_size * c->patch_size) % 64 == 0,
            "MMDiT config: in_channels x patch_size^2 = %d must be a multiple of 64 (the patch GEMM's K)",
            c->in_channels * c->patch_size * c->patch_size);
  SMI_CHECK((c->out_channels * c->patch_size * c->patch_size) % 8 == 0, "MMDiT config: out_channels x patch_size^2 %% 8");
  SMI_CHECK(h >= c->patch_size && w >= c->patch_size && h % c->patch_size == 0 && w % c->patch_size == 0,
            "MMDiT: latent %d x %d is not a multiple of patch_size %d", h, w, c->patch_size);
  SMI_CHECK(h / c->patch_size <= c->pos_embed_max_size && w / c->patch_size <= c->pos_embed_max_size,
            "MMDiT: latent grid %d x %d exceeds pos_embed_max_size %d", h / c->patch_size, w / c->patch_size,
            c->pos_embed_max_size);
  SMI_CHECK(c->joint_attention_dim >= 8 && c->joint_attention_dim % 8 == 0 && c->pooled_projection_dim >= 8 &&
                c->pooled_projection_dim % 8 == 0 && c->context_len >= 1,
            "MMDiT config: joint_attention_dim %% 8, pooled_projection_dim %% 8, context_len >= 1");
  SMI_CHECK(batch <= smi_engine::MAXS, "MMDiT: batch %d exceeds the %d per-sample multipliers", batch, smi_engine::MAXS);
  SMI_CHECK(n_sites == 0 || sites, "MMDiT: n_sites %d without sites", n_sites);
  return check_linear_lora_sites("MMDiT", sites, n_sites,
                                 {".attn.to_q", ".attn.to_k", ".attn.to_v", ".attn.to_out.0", ".attn.add_q_proj",
                                  ".attn.add_k_proj", ".attn.add_v_proj", ".attn.to_add_out"},
                                 "the attention projections (attn.to_q/to_k/to_v/to_out.0, "
                                 "attn.add_q_proj/add_k_proj/add_v_proj/to_add_out) only");
}

MMDiT* mmdit_setup(smi_engine* e, const smi_mmdit_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int h, int w,
                   bool train = false) {
  MMDiT* m = new MMDiT(*cfg, h, w, train);
  e->hold(smi_engine::MMDIT, m, cfg->dtype, batch);
  e->register_sites(sites, n_sites);
  return m;
}
// dry run: out = {packed weights, persistent region of arena 0, one scratch region, arena 1}; arena 0 is out[1] + 2 out[2];
// out[3] (a saved pass and its backward) is 0 unless the engine is trainable
int mmdit_plan(const smi_mmdit_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int h, int w, size_t out[4],
               bool train = false) {
  smi_engine e;
  e.dry = true;
  MMDiT& m = *mmdit_setup(&e, cfg, sites, n_sites, batch, h, w, train);
  m.build_all(e);
  if (e.err) return -1;
  out[0] = align_up(e.wpack.peak, 4096);
  m.dry_forward(e);
  out[1] = align_up(e.arena[0].peak, 4096);
  out[2] = align_up(std::max(e.scr[0].peak, e.scr[1].peak), 4096);
  out[3] = 0;
  if (train) {
    m.forward(e, batch, nullptr, nullptr, (void*)16, (void*)16, (float*)16, true);
    m.backward(e, nullptr, nullptr, nullptr);
    out[3] = align_up(e.arena[1].peak, 4096);
  }
  return e.err ? -1 : 0;
}
size_t plan_bytes(const size_t r[4]) { return r[0] + r[1] + 2 * r[2] + 2 * 4096 + (r[3] ? r[3] + 4096 : 0); }

int check_mmdit_train(const smi_mmdit_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int h, int w) {
  if (check_mmdit(cfg, sites, n_sites, batch, h, w)) return -1;
  SMI_CHECK(sites && n_sites > 0, "smi_mmdit_train: n_sites 0 -- no LoRA sites to train (a frozen network is smi_mmdit_create's)");
  return 0;
}

// smi_mmdit_forward / smi_mmdit_forward_save: the adaptor's state from the arguments, then the pass
int mmdit_run(smi_engine* e, const char* who, int n, const float* sample, const float* timesteps, const void* ctx,
              const void* pooled, const float* lora_down_flat, const float* lora_up_flat, const float* multipliers, float* out,
              bool save) {
  SMI_CHECK(e && e->kind == smi_engine::MMDIT, "%s: NULL or not an MMDiT engine (create it with smi_mmdit_create)", who);
  MMDiT* m = static_cast<MMDiT*>(e->model.get());
  SMI_CHECK(!save || m->trainable, "%s: this engine keeps no pass (create it with smi_mmdit_train_create)", who);
  SMI_CHECK(sample && timesteps && ctx && pooled && out, "%s: sample, timesteps, ctx, pooled and out are required", who);
  SMI_CHECK(n >= 1 && n <= e->max_n, "batch %d outside [1, %d] the engine was created for", n, e->max_n);
  e->err = false;
  // the adaptor is on when both flat buffers and the multipliers are given and one multiplier is not 0; else the frozen net.
  // Every adapted pass takes the per-sample route (sigma_i = m_i / max |m|): a sample gives the same bits alone and in a batch
  float mref = 0.f;
  if (lora_down_flat && lora_up_flat && multipliers && !e->prep_sites.empty())
    if (const int rc = e->set_sample_multipliers(multipliers, n, save, &mref)) return rc;
  e->lora_down = mref != 0.f ? lora_down_flat : nullptr;
  e->lora_up = mref != 0.f ? lora_up_flat : nullptr;
  e->mult = mref;
  e->samp_on = mref != 0.f;
  // no split-K scratch is lent to this model's GEMMs: the slice count follows the launch's row count, so with one the bits
  // of a sample would depend on its batch
  smi::set_gemm_scratch(nullptr, 0);
  const int rc = m->forward(*e, n, sample, timesteps, ctx, pooled, out, save);
  e->samp_on = false;
  return rc;
}

}  // namespace

extern "C" {

int smi_mmdit_workspace_bytes(const smi_mmdit_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int h, int w,
                              size_t* bytes) {
  if (check_mmdit(cfg, sites, n_sites, batch, h, w)) return -1;
  SMI_CHECK(bytes != nullptr, "bad arguments");
  size_t r[4];
  if (mmdit_plan(cfg, sites, n_sites, batch, h, w, r)) return -1;
  *bytes = plan_bytes(r);
  return 0;
}

int smi_mmdit_train_workspace_bytes(const smi_mmdit_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int h,
                                    int w, size_t* bytes) {
  if (check_mmdit_train(cfg, sites, n_sites, batch, h, w)) return -1;
  SMI_CHECK(bytes != nullptr, "bad arguments");
  size_t r[4];
  if (mmdit_plan(cfg, sites, n_sites, batch, h, w, r, true)) return -1;
  *bytes = plan_bytes(r);
  return 0;
}

// both create entries: train says which
static int mmdit_create(bool train, const smi_mmdit_config* cfg, const smi_weight* weights, int n_weights,
                        const smi_lora_site* sites, int n_sites, int batch, int h, int w, void* workspace,
                        size_t workspace_bytes, void* stream, smi_engine** out) {
  SMI_CHECK(out && workspace && weights && n_weights > 0, "bad arguments");
  size_t r[4];
  if (mmdit_plan(cfg, sites, n_sites, batch, h, w, r, train)) return -1;
  SMI_CHECK(plan_bytes(r) <= workspace_bytes, "workspace too small: need %zu bytes, got %zu", plan_bytes(r), workspace_bytes);
  smi_engine* e = new smi_engine();
  e->stream = (hipStream_t)stream;
  MMDiT* m = mmdit_setup(e, cfg, sites, n_sites, batch, h, w, train);
  for (int i = 0; i < n_weights; ++i) e->wmap[weights[i].name] = &weights[i];
  char* base = (char*)align_up((size_t)workspace, 4096);
  e->wpack.base = base;
  e->wpack.cap = r[0];
  e->arena[0].base = base + r[0];
  e->set_arena0_regions(r[1], r[2]);
  e->arena[1].base = base + r[0] + r[1] + 2 * r[2];
  e->arena[1].cap = r[3];
  m->build_all(*e);
  return finish_create(e, "the MMDiT weights", out);
}

int smi_mmdit_create(const smi_mmdit_config* cfg, const smi_weight* weights, int n_weights, const smi_lora_site* sites,
                     int n_sites, int batch, int h, int w, void* workspace, size_t workspace_bytes, void* stream,
                     smi_engine** out) {
  if (check_mmdit(cfg, sites, n_sites, batch, h, w)) return -1;
  return mmdit_create(false, cfg, weights, n_weights, sites, n_sites, batch, h, w, workspace, workspace_bytes, stream, out);
}

int smi_mmdit_train_create(const smi_mmdit_config* cfg, const smi_weight* weights, int n_weights, const smi_lora_site* sites,
                           int n_sites, int batch, int h, int w, void* workspace, size_t workspace_bytes, void* stream,
                           smi_engine** out) {
  if (check_mmdit_train(cfg, sites, n_sites, batch, h, w)) return -1;
  return mmdit_create(true, cfg, weights, n_weights, sites, n_sites, batch, h, w, workspace, workspace_bytes, stream, out);
}

int smi_mmdit_forward(smi_engine* e, int n, const float* sample, const float* timesteps, const void* ctx, const void* pooled,
                      const float* lora_down_flat, const float* lora_up_flat, const float* multipliers, float* out) {
  return mmdit_run(e, "smi_mmdit_forward", n, sample, timesteps, ctx, pooled, lora_down_flat, lora_up_flat, multipliers, out,
                   false);
}

int smi_mmdit_forward_save(smi_engine* e, int n, const float* sample, const float* timesteps, const void* ctx,
                           const void* pooled, const float* lora_down_flat, const float* lora_up_flat,
                           const float* multipliers, float* out) {
  return mmdit_run(e, "smi_mmdit_forward_save", n, sample, timesteps, ctx, pooled, lora_down_flat, lora_up_flat, multipliers,
                   out, true);
}

int smi_mmdit_backward(smi_engine* e, const float* d_out, float* d_lora_down_flat, float* d_lora_up_flat) {
  SMI_CHECK(e && e->kind == smi_engine::MMDIT && d_out, "smi_mmdit_backward: NULL argument or not an MMDiT engine");
  MMDiT* m = static_cast<MMDiT*>(e->model.get());
  SMI_CHECK(m->trainable, "smi_mmdit_backward: this engine keeps no pass (create it with smi_mmdit_train_create)");
  e->err = false;
  smi::set_gemm_scratch(nullptr, 0);
  return m->backward(*e, d_out, d_lora_down_flat, d_lora_up_flat);
}

}  // extern "C"
