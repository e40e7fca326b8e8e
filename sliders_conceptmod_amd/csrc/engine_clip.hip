// The CLIP engines: the text tower (transformers CLIPTextModel[WithProjection]; T/train_util.py:108-155) and the image
// tower (CLIPVisionModel[WithProjection]).  Both are pre-LayerNorm blocks on the op core (engine.h); the blocks are
// written once and differ in the causal mask only.  Forward only -- except a text tower created with LoRA sites on its
// attention projections (smi_clip_lora_*: the no-trigger trainer), which also saves a pass and differentiates it.
#include "engine.h"

namespace {

struct CLayer {
  Norm n1, n2;
  Lin qkv, out, fc1, fc2;
};
// the encoder layers of either tower: `prefix` + layer number names them in the transformers state dict
// grad: the tower is differentiated -- every Linear gets its transposed copy (dX) and may carry LoRA sites
void build_clip_layers(smi_engine& e, std::vector<CLayer>& layers, const std::string& prefix, int num_layers, int d,
                       int inter, bool grad = false) {
  layers.resize(num_layers);
  for (int i = 0; i < num_layers; ++i) {
    const std::string b = prefix + std::to_string(i);
    CLayer& L = layers[i];
    L.n1 = e.make_norm(b + ".layer_norm1", d, 1e-5f, 0);
    L.qkv = e.make_fused(b + ".self_attn", {"q_proj", "k_proj", "v_proj"}, d, d, grad);
    L.qkv.b = e.fused_bias(b + ".self_attn", {"q_proj", "k_proj", "v_proj"}, d);
    L.out = e.make_lin(b + ".self_attn.out_proj", d, d, true, grad);
    L.n2 = e.make_norm(b + ".layer_norm2", d, 1e-5f, 0);
    L.fc1 = e.make_lin(b + ".mlp.fc1", d, inter, true, grad);
    L.fc2 = e.make_lin(b + ".mlp.fc2", inter, d, true, grad);
  }
}
// one pre-LayerNorm block on h [n L, d]; `causal` says whether the self-attention is masked
Ten* clip_block(smi_engine& e, Ten* h, const CLayer& ly, int n, int L, int heads, int d, int act, bool causal) {
  Ten* qkv = e.linear(e.layernorm(h, ly.n1), ly.qkv);
  Ten* o = e.attention(qkv, nullptr, nullptr, heads, d, n, L, L, causal);
  h = e.linear(o, ly.out, h);
  Ten* f = e.linear(e.layernorm(h, ly.n2), ly.fc1);
  return e.linear(e.act(f, act), ly.fc2, h);
}

// ---------------------------------------------------------------------------------------------------------
// CLIP text encoder: token + position embedding, pre-LayerNorm blocks with CAUSAL self-attention (the fused attention
// kernel with its causal mask), quick_gelu / gelu MLP, final LayerNorm, pooled EOS row (x text_projection).
// ---------------------------------------------------------------------------------------------------------
struct ClipText : Model {
  smi_clip_config cfg{};
  std::vector<CLayer> layers;
  Norm final_norm;
  Lin proj;
  const void* tok = nullptr;
  const void* pos = nullptr;
  // a tower created with LoRA sites (smi_clip_lora_create): arena 1 holds the saved pass and its backward
  bool trainable = false;
  Ten *out_last = nullptr, *out_pen = nullptr;  // hidden_states[-1] (no final norm) and [-2] of the saved pass
  explicit ClipText(const smi_clip_config& c, bool train = false) : cfg(c), trainable(train) {}

  void build(smi_engine& e) override {
    const int d = cfg.hidden_size;
    tok = e.Wd("text_model.embeddings.token_embedding.weight");
    pos = e.Wd("text_model.embeddings.position_embedding.weight");
    e.check_shape("text_model.embeddings.token_embedding.weight", {cfg.vocab_size, d});
    e.check_shape("text_model.embeddings.position_embedding.weight", {cfg.max_positions, d});
    build_clip_layers(e, layers, "text_model.encoder.layers.", cfg.num_layers, d, cfg.intermediate_size, trainable);
    final_norm = e.make_norm("text_model.final_layer_norm", d, 1e-5f, 0);
    if (cfg.projection_dim > 0) proj = e.make_lin("text_projection", d, cfg.projection_dim, false, false);
  }
  // what a trainable tower packs after its layers (the forward-only create path packs its own: engine.hip build_model)
  void build_trainable(smi_engine& e) {
    build(e);
    e.finish_lora();
    e.gscale = (float*)e.pack_alloc(e.GSCALE_FLOATS * sizeof(float));
    e.samp_mult_dev = (float*)e.pack_alloc(2 * e.MAXS * sizeof(float));
    e.alloc_job_table(2 * e.sites.size() + 8);  // a fused q|k|v pushes at most 4 jobs for its 3 sites, out_proj 2
    for (size_t i = 0; i < e.sites.size(); ++i)
      if (!e.site_used[i] && !e.err) {
        set_error("LoRA target '%s' is not a layer of this text tower", e.site_names[i].c_str());
        e.err = true;
      }
  }
  void dry_forward(smi_engine& e) override {  // all outputs
    e.begin_forward_only_pass();
    forward(e, e.max_n, nullptr, nullptr, (void*)16, (void*)16, (void*)16);
  }

  // the pass itself; whoever calls has begun it (begin_forward_only_pass, or begin_pass with every sample adapted)
  int forward(smi_engine& e, int n, const int* ids, const int* eos_pos, void* last_hidden, void* penultimate,
              void* pooled, void* last_layer_out = nullptr) {
    const int L = cfg.max_positions, d = cfg.hidden_size;
    if (!e.prep_sites.empty() && (e.dry || (e.lora_down && e.lora_up && e.mult != 0.f)))
      RUNP(SMI_PROF_LORA, 0.0, 0.0, launch_lora_prep(e.dtype, e.prep_sites_dev, (int)e.prep_sites.size(), e.lora_down, e.lora_up, e.lora_shadow, e.stream));
    Ten* h = e.new_ten((int64_t)n * L, d, n, L, 1);  // the embeddings: no gradient flows into them (ng stays false)
    RUN(launch_embed(e.dtype, ids, tok, pos, h->p, (int64_t)n * L, L, d, cfg.vocab_size, e.stream));
    Ten* pen = h;
    for (int i = 0; i < cfg.num_layers; ++i) {
      if (i == cfg.num_layers - 1) {  // hidden_states[-2]: what enters the last layer
        pen = h;
        if (penultimate) RUN(launch_copy_cols(e.dtype, h->p, d, penultimate, d, 0, (int)h->rows, d, e.stream));
      }
      h = clip_block(e, h, layers[i], n, L, cfg.num_heads, d, cfg.hidden_act, true);
    }
    if (last_layer_out) RUN(launch_copy_cols(e.dtype, h->p, d, last_layer_out, d, 0, (int)h->rows, d, e.stream));
    if (e.saving) {
      out_last = h;
      out_pen = pen;
      e.keep_saved_pass(n);
    }
    {
      e.saving = false;  // neither output below is differentiated: the final norm and the projection stay off the tape
      Ten* fin = e.layernorm(h, final_norm);
      if (last_hidden) RUN(launch_copy_cols(e.dtype, fin->p, d, last_hidden, d, 0, (int)fin->rows, d, e.stream));
      if (pooled) {
        Ten* pl = e.new_ten(n, d, n, 1, 1);
        RUN(launch_gather_rows(e.dtype, fin->p, eos_pos, pl->p, n, L, d, e.stream));
        if (cfg.projection_dim > 0) pl = e.linear(pl, proj);
        RUN(launch_copy_cols(e.dtype, pl->p, pl->cols, pooled, pl->cols, 0, n, pl->cols, e.stream));
      }
    }
    return e.end_pass("this call (");
  }

  // the shared backward (engine.h) with this model's two parts: which 0: d_hidden is the gradient of hidden_states[-1] (the
  // last layer's output, no final norm); 1: of hidden_states[-2], and the last layer's closures see no gradient -- its
  // sites get none.  One power-of-two loss scale per sample.  A backward consumes the saved pass.
  int backward(smi_engine& e, int which, const float* d_hidden, float* dd, float* du) {
    if (const int rc = e.begin_backward("smi_clip_backward: no saved forward pass (call smi_clip_forward_lora with save_for_backward=1 first)",
                                        dd, du, e.saved.n))
      return rc;
    Ten* y = which == 0 ? out_last : out_pen;
    if (!y->ng) {  // adaptor off, or nothing adapted upstream of hidden_states[-2]: the gradient is zero
      e.drop_tape();
      return 0;
    }
    const int n = e.saved.n, L = cfg.max_positions, d = cfg.hidden_size;
    RUN(launch_grad_scale(d_hidden, n, (int64_t)L * d, e.gscale, e.MAXS, e.stream));
    e.rebuild_saved_operands();
    y->g = e.alloc_t(e.MA(y), d);
    // f32 [n, L d] -> 16-bit rows, sample j x its loss scale: the cast of the UNet's d_eps with one "channel"
    RUN(launch_nchw_to_nhwc_scaled(e.dtype, d_hidden, y->g, n, 1, L * d, 1, e.gscale, e.stream));
    if (e.run_tape_and_weight_grads()) return -1;
    return e.end_pass("the backward (");
  }
};

// ---------------------------------------------------------------------------------------------------------
// CLIP image tower: patch matrix -> patch GEMM -> class token + position embedding + pre_layrnorm -> the text tower's
// blocks without the mask -> post_layernorm of the class row (x visual_projection).  No split-K scratch is lent to its
// GEMMs (smi_clip_vision_encode): an image gives the same bits alone or in a batch.
// ---------------------------------------------------------------------------------------------------------
struct ClipVision : Model {
  smi_clip_vision_config cfg{};
  std::vector<CLayer> layers;
  Lin patch, proj;
  Norm pre, post;
  const void* cls = nullptr;
  const void* pos = nullptr;
  explicit ClipVision(const smi_clip_vision_config& c) : cfg(c) {}
  int grid() const { return cfg.image_size / cfg.patch_size; }
  int kp() const { return (3 * cfg.patch_size * cfg.patch_size + 63) / 64 * 64; }

  void build(smi_engine& e) override {
    const int d = cfg.hidden_size, P = cfg.patch_size, G = grid(), K = 3 * P * P, Kp = kp();
    const std::string emb = "vision_model.embeddings.";
    cls = e.Wd(emb + "class_embedding");
    e.check_shape(emb + "class_embedding", {d});
    pos = e.Wd(emb + "position_embedding.weight");
    e.check_shape(emb + "position_embedding.weight", {G * G + 1, d});
    // the patch filter [hidden, 3, P, P] is already [hidden, K] with K in (c, py, px) order: repacked to rows of Kp
    // with the pad columns zero, so that the patch embedding is gemm_nt on the patch matrix
    const void* pw = e.Wd(emb + "patch_embedding.weight");
    e.check_shape(emb + "patch_embedding.weight", {d, 3, P, P});
    void* wp = e.pack_alloc((size_t)d * Kp * e.esz());
    if (!e.dry && !e.err && pw) {
      ++e.pack_launches;
      if (Kp != K) (void)hipMemsetAsync(wp, 0, (size_t)d * Kp * e.esz(), e.stream);
      (void)hipMemcpy2DAsync(wp, (size_t)Kp * e.esz(), pw, (size_t)K * e.esz(), (size_t)K * e.esz(), d,
                             hipMemcpyDeviceToDevice, e.stream);
    }
    patch.name = emb + "patch_embedding";
    patch.in = Kp;
    patch.out = d;
    patch.W = wp;
    pre = e.make_norm("vision_model.pre_layrnorm", d, 1e-5f, 0);  // transformers' spelling
    build_clip_layers(e, layers, "vision_model.encoder.layers.", cfg.num_layers, d, cfg.intermediate_size);
    post = e.make_norm("vision_model.post_layernorm", d, 1e-5f, 0);
    if (cfg.projection_dim > 0) proj = e.make_lin("visual_projection", d, cfg.projection_dim, false, false);
  }
  void dry_forward(smi_engine& e) override { forward(e, e.max_n, nullptr, nullptr, (void*)16, (void*)16); }

  int forward(smi_engine& e, int n, const uint8_t* rgb8, const float* pixel_values, void* last_hidden,
              void* image_embeds) {
    e.begin_forward_only_pass();
    const int d = cfg.hidden_size, G = grid(), L = G * G + 1, Kp = kp();
    Ten* pm = e.new_ten((int64_t)n * G * G, Kp, n, G * G, 1);
    RUN(launch_clip_patchify(e.dtype, rgb8, pixel_values, pm->p, n, cfg.image_size, cfg.patch_size, Kp, cfg.image_mean,
                             cfg.image_std, e.stream));
    Ten* pe = e.linear(pm, patch);
    Ten* h = e.new_ten((int64_t)n * L, d, n, L, 1);
    RUNP(SMI_PROF_NORM, 0.0, 4.0 * h->rows * d,
         launch_vit_embed_ln(e.dtype, pe->p, cls, pos, pre.gamma, pre.beta, h->p, n, L, d, pre.eps, e.stream));
    for (int i = 0; i < cfg.num_layers; ++i)
      h = clip_block(e, h, layers[i], n, L, cfg.num_heads, d, cfg.hidden_act, false);
    if (last_hidden) RUN(launch_copy_cols(e.dtype, h->p, d, last_hidden, d, 0, (int)h->rows, d, e.stream));
    if (image_embeds) {
      Ten* cr = e.new_ten(n, d, n, 1, 1);  // the class rows: row i * L of h
      RUN(launch_copy_cols(e.dtype, h->p, (int64_t)L * d, cr->p, d, 0, n, d, e.stream));
      Ten* pl = e.layernorm(cr, post);
      if (cfg.projection_dim > 0) pl = e.linear(pl, proj);
      RUN(launch_copy_cols(e.dtype, pl->p, pl->cols, image_embeds, pl->cols, 0, n, pl->cols, e.stream));
    }
    return e.end_pass("this call (");
  }
};

int check_clip_cfg(const smi_clip_config* c, int batch) {
  SMI_CHECK(c != nullptr, "config is NULL");
  SMI_CHECK(c->dtype == SMI_DTYPE_F16 || c->dtype == SMI_DTYPE_BF16, "dtype must be f16 (0) or bf16 (1)");
  SMI_CHECK(c->hidden_size % 64 == 0 && c->hidden_size <= 2048 && c->num_heads > 0 && c->hidden_size % c->num_heads == 0 &&
                (c->hidden_size / c->num_heads) % 8 == 0 && c->intermediate_size % 64 == 0 && c->num_layers >= 1 &&
                c->vocab_size > 0 && c->max_positions > 0 && (c->hidden_act == 0 || c->hidden_act == 1) &&
                c->projection_dim >= 0 && c->projection_dim % 8 == 0 && batch > 0,
            "CLIP config out of range (hidden %% 64, hidden <= 2048, head_dim %% 8, intermediate %% 64)");
  return 0;
}
Setup clip_setup(const smi_clip_config* cfg, int batch) {
  return [=](smi_engine* e) { e->hold(smi_engine::CLIP_TEXT, new ClipText(*cfg), cfg->dtype, batch); };
}

// a text tower with LoRA sites: what the causal attention backward takes, and Linear LoRA on the attention projections only
int check_clip_lora(const smi_clip_config* c, const smi_lora_site* sites, int n_sites, int batch) {
  if (check_clip_cfg(c, batch)) return -1;
  SMI_CHECK(sites && n_sites > 0, "smi_clip_lora: no LoRA sites (a tower without them is smi_clip_create's)");
  SMI_CHECK(c->hidden_size / c->num_heads == 64 && c->max_positions <= 128,
            "smi_clip_lora: head_dim %d / %d positions -- the causal attention backward takes head_dim 64 and at most 128 "
            "positions", c->hidden_size / c->num_heads, c->max_positions);
  SMI_CHECK(batch <= smi_engine::MAXS, "smi_clip_lora: batch %d exceeds the %d per-sample multipliers", batch, smi_engine::MAXS);
  return check_linear_lora_sites("smi_clip_lora", sites, n_sites,
                                 {".self_attn.q_proj", ".self_attn.k_proj", ".self_attn.v_proj", ".self_attn.out_proj"},
                                 "self_attn.{q,k,v}_proj and self_attn.out_proj");
}
ClipText* clip_lora_setup(smi_engine* e, const smi_clip_config* cfg, const smi_lora_site* sites, int n_sites, int batch) {
  ClipText* t = new ClipText(*cfg, true);
  e->hold(smi_engine::CLIP_TEXT, t, cfg->dtype, batch);
  e->register_sites(sites, n_sites);
  return t;
}
// dry run: out = {packed weights, arena 0 (the largest no-grad pass), arena 1 (a saved pass and its backward)}
int clip_lora_plan(const smi_clip_config* cfg, const smi_lora_site* sites, int n_sites, int batch, size_t out[3]) {
  smi_engine e;
  e.dry = true;
  ClipText& t = *clip_lora_setup(&e, cfg, sites, n_sites, batch);
  t.build_trainable(e);
  if (e.err) return -1;
  out[0] = align_up(e.wpack.peak, 4096);
  e.begin_pass(batch, false);  // the adapted no-grad pass allocates what the plain one does, and xa
  t.forward(e, batch, nullptr, nullptr, (void*)16, (void*)16, (void*)16, (void*)16);
  out[1] = align_up(e.arena[0].peak, 4096);
  e.begin_pass(batch, true);
  t.forward(e, batch, nullptr, nullptr, (void*)16, (void*)16, (void*)16, (void*)16);
  t.backward(e, 0, nullptr, nullptr, nullptr);
  out[2] = align_up(e.arena[1].peak, 4096);
  return e.err ? -1 : 0;
}

int check_clip_vision_cfg(const smi_clip_vision_config* c, int batch) {
  SMI_CHECK(c != nullptr, "config is NULL");
  SMI_CHECK(c->dtype == SMI_DTYPE_F16 || c->dtype == SMI_DTYPE_BF16, "dtype must be f16 (0) or bf16 (1)");
  SMI_CHECK(c->image_size > 0 && c->patch_size > 0 && c->image_size % c->patch_size == 0,
            "CLIP vision config: image_size %d is not a multiple of patch_size %d", c->image_size, c->patch_size);
  SMI_CHECK(c->hidden_size > 0 && c->hidden_size % 64 == 0 && c->hidden_size <= 2048,
            "CLIP vision config: hidden_size %d must be a multiple of 64 and <= 2048", c->hidden_size);
  SMI_CHECK(c->num_heads > 0 && c->hidden_size % c->num_heads == 0 && (c->hidden_size / c->num_heads) % 8 == 0,
            "CLIP vision config: head_dim (hidden_size %d / num_heads %d) must be a multiple of 8", c->hidden_size,
            c->num_heads);
  SMI_CHECK(c->intermediate_size > 0 && c->intermediate_size % 64 == 0,
            "CLIP vision config: intermediate_size %d must be a multiple of 64", c->intermediate_size);
  SMI_CHECK(c->projection_dim >= 0 && c->projection_dim % 8 == 0,
            "CLIP vision config: projection_dim %d must be a multiple of 8", c->projection_dim);
  SMI_CHECK(c->num_layers >= 1 && (c->hidden_act == 0 || c->hidden_act == 1) && batch > 0,
            "CLIP vision config out of range (num_layers >= 1, hidden_act 0 / 1, batch > 0)");
  SMI_CHECK(clip_patchify_lds_bytes(c->image_size, c->patch_size) <= 65536,
            "CLIP vision config: image_size %d x patch_size %d exceeds the patch kernel's LDS strip (image_size x "
            "patch_size <= 10922)", c->image_size, c->patch_size);
  for (int k = 0; k < 3; ++k) SMI_CHECK(c->image_std[k] > 0.f, "CLIP vision config: image_std[%d] must be positive", k);
  return 0;
}
Setup clip_vision_setup(const smi_clip_vision_config* cfg, int batch) {
  return [=](smi_engine* e) { e->hold(smi_engine::CLIP_VISION, new ClipVision(*cfg), cfg->dtype, batch); };
}

}  // namespace

extern "C" {

// ---- CLIP text encoder engine ------------------------------------------------------------------------------------------
int smi_clip_workspace_bytes(const smi_clip_config* cfg, int batch, size_t* bytes) {
  if (check_clip_cfg(cfg, batch)) return -1;
  return workspace_bytes_forward_only(clip_setup(cfg, batch), bytes);
}

int smi_clip_create(const smi_clip_config* cfg, const smi_weight* weights, int n_weights, int batch, void* workspace,
                    size_t workspace_bytes, void* stream, smi_engine** out) {
  if (check_clip_cfg(cfg, batch)) return -1;
  return create_forward_only(clip_setup(cfg, batch), "the CLIP weights", weights, n_weights, workspace, workspace_bytes,
                             stream, out);
}

int smi_clip_encode(smi_engine* e, int n, const int32_t* ids, const int32_t* eos_pos, void* last_hidden,
                    void* penultimate, void* pooled) {
  SMI_CHECK(e && e->kind == smi_engine::CLIP_TEXT && ids, "smi_clip_encode: NULL argument or not a CLIP text engine");
  SMI_CHECK(n >= 1 && n <= e->max_n, "batch %d outside [1, %d] the engine was created for", n, e->max_n);
  SMI_CHECK(!pooled || eos_pos, "pooled output needs eos_pos");
  e->err = false;
  e->begin_forward_only_pass();
  return static_cast<ClipText*>(e->model.get())->forward(*e, n, ids, eos_pos, last_hidden, penultimate, pooled);
}

// smi_clip_encode plus hidden_states[-1], the last layer's output without the final norm (any output may be NULL)
int smi_clip_encode_layers(smi_engine* e, int n, const int32_t* ids, const int32_t* eos_pos, void* last_hidden,
                           void* penultimate, void* pooled, void* last_layer_out) {
  SMI_CHECK(e && e->kind == smi_engine::CLIP_TEXT && ids, "smi_clip_encode_layers: NULL argument or not a CLIP text engine");
  SMI_CHECK(n >= 1 && n <= e->max_n, "batch %d outside [1, %d] the engine was created for", n, e->max_n);
  SMI_CHECK(!pooled || eos_pos, "pooled output needs eos_pos");
  e->err = false;
  e->begin_forward_only_pass();
  return static_cast<ClipText*>(e->model.get())->forward(*e, n, ids, eos_pos, last_hidden, penultimate, pooled, last_layer_out);
}

// ---- CLIP text tower with LoRA sites: saved forward with one multiplier per sample, backward to the LoRA parameters ---
int smi_clip_lora_workspace_bytes(const smi_clip_config* cfg, const smi_lora_site* sites, int n_sites, int batch,
                                  size_t* bytes) {
  if (check_clip_lora(cfg, sites, n_sites, batch)) return -1;
  SMI_CHECK(bytes != nullptr, "bad arguments");
  size_t r[3];
  if (clip_lora_plan(cfg, sites, n_sites, batch, r)) return -1;
  *bytes = r[0] + r[1] + r[2] + 3 * 4096;
  return 0;
}

int smi_clip_lora_create(const smi_clip_config* cfg, const smi_weight* weights, int n_weights, const smi_lora_site* sites,
                         int n_sites, int batch, void* workspace, size_t workspace_bytes, void* stream, smi_engine** out) {
  if (check_clip_lora(cfg, sites, n_sites, batch)) return -1;
  SMI_CHECK(out && workspace && weights && n_weights > 0, "bad arguments");
  size_t r[3];
  if (clip_lora_plan(cfg, sites, n_sites, batch, r)) return -1;
  SMI_CHECK(r[0] + r[1] + r[2] + 3 * 4096 <= workspace_bytes, "workspace too small: need %zu bytes, got %zu",
            r[0] + r[1] + r[2] + 3 * 4096, workspace_bytes);
  smi_engine* e = new smi_engine();
  e->stream = (hipStream_t)stream;
  ClipText* t = clip_lora_setup(e, cfg, sites, n_sites, batch);
  for (int i = 0; i < n_weights; ++i) e->wmap[weights[i].name] = &weights[i];
  char* base = (char*)align_up((size_t)workspace, 4096);
  e->wpack.base = base;
  e->wpack.cap = r[0];
  e->arena[0].base = base + r[0];
  e->arena[0].cap = r[1];
  e->arena[1].base = base + r[0] + r[1];
  e->arena[1].cap = r[2];
  t->build_trainable(*e);
  return finish_create(e, "the CLIP weights", out);
}

int smi_clip_forward_lora(smi_engine* e, int n, const int32_t* ids, const int32_t* eos_pos, const float* lora_down_flat,
                          const float* lora_up_flat, const float* multipliers, int save_for_backward, void* last_layer_out,
                          void* penultimate, void* last_hidden, void* pooled) {
  SMI_CHECK(e && e->kind == smi_engine::CLIP_TEXT && ids, "smi_clip_forward_lora: NULL argument or not a CLIP text engine");
  ClipText* t = static_cast<ClipText*>(e->model.get());
  SMI_CHECK(t->trainable, "smi_clip_forward_lora: this engine has no LoRA sites (create it with smi_clip_lora_create)");
  SMI_CHECK(n >= 1 && n <= e->max_n, "batch %d outside [1, %d] the engine was created for", n, e->max_n);
  SMI_CHECK(lora_down_flat && lora_up_flat && multipliers, "smi_clip_forward_lora: lora_down_flat, lora_up_flat and multipliers are required");
  SMI_CHECK(!pooled || eos_pos, "pooled output needs eos_pos");
  e->err = false;
  // every adapted pass takes the per-sample route (sigma_i = m_i / max |m|), so that a sample gives the same bits alone and
  // in a batch; all multipliers 0 is the frozen tower
  float mref = 0.f;
  if (const int rc = e->set_sample_multipliers(multipliers, n, save_for_backward != 0, &mref)) return rc;
  e->begin_pass(n, save_for_backward != 0);
  e->lora_down = lora_down_flat;
  e->lora_up = lora_up_flat;
  e->mult = mref;
  e->samp_on = mref != 0.f;
  const int rc = t->forward(*e, n, ids, eos_pos, last_hidden, penultimate, pooled, last_layer_out);
  e->samp_on = false;
  return rc;
}

int smi_clip_backward(smi_engine* e, int which, const float* d_hidden, float* d_lora_down_flat, float* d_lora_up_flat) {
  SMI_CHECK(e && e->kind == smi_engine::CLIP_TEXT && d_hidden, "smi_clip_backward: NULL argument or not a CLIP text engine");
  ClipText* t = static_cast<ClipText*>(e->model.get());
  SMI_CHECK(t->trainable, "smi_clip_backward: this engine has no LoRA sites (create it with smi_clip_lora_create)");
  SMI_CHECK(which == 0 || which == 1, "smi_clip_backward: which must be 0 (last_layer_out) or 1 (penultimate), got %d", which);
  e->err = false;
  return t->backward(*e, which, d_hidden, d_lora_down_flat, d_lora_up_flat);
}

// ---- CLIP image tower engine and the similarity head ------------------------------------------------------------------
int smi_clip_vision_workspace_bytes(const smi_clip_vision_config* cfg, int batch, size_t* bytes) {
  if (check_clip_vision_cfg(cfg, batch)) return -1;
  return workspace_bytes_forward_only(clip_vision_setup(cfg, batch), bytes);
}

int smi_clip_vision_create(const smi_clip_vision_config* cfg, const smi_weight* weights, int n_weights, int batch,
                           void* workspace, size_t workspace_bytes, void* stream, smi_engine** out) {
  if (check_clip_vision_cfg(cfg, batch)) return -1;
  return create_forward_only(clip_vision_setup(cfg, batch), "the CLIP vision weights", weights, n_weights, workspace,
                             workspace_bytes, stream, out);
}

int smi_clip_vision_encode(smi_engine* e, int n, const uint8_t* rgb8, const float* pixel_values, void* last_hidden,
                           void* image_embeds) {
  SMI_CHECK(e && e->kind == smi_engine::CLIP_VISION,
            "smi_clip_vision_encode: NULL or not a CLIP vision engine (create it with smi_clip_vision_create)");
  SMI_CHECK((rgb8 != nullptr) != (pixel_values != nullptr), "smi_clip_vision_encode: exactly one of rgb8 / pixel_values");
  SMI_CHECK(last_hidden || image_embeds, "smi_clip_vision_encode: no output requested");
  SMI_CHECK(n >= 1 && n <= e->max_n, "batch %d outside [1, %d] the engine was created for", n, e->max_n);
  e->err = false;
  return static_cast<ClipVision*>(e->model.get())->forward(*e, n, rgb8, pixel_values, last_hidden, image_embeds);
}

int smi_clip_logits(int dtype, const void* image_embeds, int ni, const void* text_embeds, int nt, int dim,
                    float logit_scale, float* logits_per_image, void* stream) {
  return launch_clip_logits(dtype, image_embeds, ni, text_embeds, nt, dim, logit_scale, logits_per_image,
                            (hipStream_t)stream);
}

}  // extern "C"
