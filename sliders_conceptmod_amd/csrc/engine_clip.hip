// The CLIP engines, forward only: the text tower (transformers CLIPTextModel[WithProjection]; T/train_util.py:108-155)
// and the image tower (CLIPVisionModel[WithProjection]).  Both are pre-LayerNorm blocks on the op core (engine.h); the
// blocks are written once and differ in the causal mask only.
#include "engine.h"

namespace {

struct CLayer {
  Norm n1, n2;
  Lin qkv, out, fc1, fc2;
};
// the encoder layers of either tower: `prefix` + layer number names them in the transformers state dict
void build_clip_layers(smi_engine& e, std::vector<CLayer>& layers, const std::string& prefix, int num_layers, int d,
                       int inter) {
  layers.resize(num_layers);
  for (int i = 0; i < num_layers; ++i) {
    const std::string b = prefix + std::to_string(i);
    CLayer& L = layers[i];
    L.n1 = e.make_norm(b + ".layer_norm1", d, 1e-5f, 0);
    L.qkv = e.make_fused(b + ".self_attn", {"q_proj", "k_proj", "v_proj"}, d, d, false);
    L.qkv.b = e.fused_bias(b + ".self_attn", {"q_proj", "k_proj", "v_proj"}, d);
    L.out = e.make_lin(b + ".self_attn.out_proj", d, d, true, false);
    L.n2 = e.make_norm(b + ".layer_norm2", d, 1e-5f, 0);
    L.fc1 = e.make_lin(b + ".mlp.fc1", d, inter, true, false);
    L.fc2 = e.make_lin(b + ".mlp.fc2", inter, d, true, false);
  }
}
// one pre-LayerNorm block on h [n L, d]; `causal` says whether the self-attention is masked
Ten* clip_block(smi_engine& e, Ten* h, const CLayer& ly, int n, int L, int heads, int d, int act, bool causal) {
  Ten* qkv = e.linear(e.layernorm(h, ly.n1), ly.qkv);
  Ten* o = e.attention(qkv, nullptr, nullptr, heads, d, n, L, L, causal);
  h = e.linear(o, ly.out, h);
  Ten* f = e.linear(e.layernorm(h, ly.n2), ly.fc1);
  Ten* a = e.new_ten(f->rows, f->cols, n, L, 1);
  RUNP(SMI_PROF_ELEM, 0.0, 0.0, launch_act(e.dtype, f->p, a->p, f->rows * f->cols, act, e.stream));
  return e.linear(a, ly.fc2, h);
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
  explicit ClipText(const smi_clip_config& c) : cfg(c) {}

  void build(smi_engine& e) override {
    const int d = cfg.hidden_size;
    tok = e.Wd("text_model.embeddings.token_embedding.weight");
    pos = e.Wd("text_model.embeddings.position_embedding.weight");
    e.check_shape("text_model.embeddings.token_embedding.weight", {cfg.vocab_size, d});
    e.check_shape("text_model.embeddings.position_embedding.weight", {cfg.max_positions, d});
    build_clip_layers(e, layers, "text_model.encoder.layers.", cfg.num_layers, d, cfg.intermediate_size);
    final_norm = e.make_norm("text_model.final_layer_norm", d, 1e-5f, 0);
    if (cfg.projection_dim > 0) proj = e.make_lin("text_projection", d, cfg.projection_dim, false, false);
  }
  void dry_forward(smi_engine& e) override {  // all outputs
    forward(e, e.max_n, nullptr, nullptr, (void*)16, (void*)16, (void*)16);
  }

  int forward(smi_engine& e, int n, const int* ids, const int* eos_pos, void* last_hidden, void* penultimate,
              void* pooled) {
    e.begin_forward_only_pass();
    const int L = cfg.max_positions, d = cfg.hidden_size;
    Ten* h = e.new_ten((int64_t)n * L, d, n, L, 1);
    RUN(launch_embed(e.dtype, ids, tok, pos, h->p, (int64_t)n * L, L, d, cfg.vocab_size, e.stream));
    for (int i = 0; i < cfg.num_layers; ++i) {
      if (i == cfg.num_layers - 1 && penultimate)  // hidden_states[-2]: what enters the last layer
        RUN(launch_copy_cols(e.dtype, h->p, d, penultimate, d, 0, (int)h->rows, d, e.stream));
      h = clip_block(e, h, layers[i], n, L, cfg.num_heads, d, cfg.hidden_act, true);
    }
    Ten* fin = e.layernorm(h, final_norm);
    if (last_hidden) RUN(launch_copy_cols(e.dtype, fin->p, d, last_hidden, d, 0, (int)fin->rows, d, e.stream));
    if (pooled) {
      Ten* pl = e.new_ten(n, d, n, 1, 1);
      RUN(launch_gather_rows(e.dtype, fin->p, eos_pos, pl->p, n, L, d, e.stream));
      if (cfg.projection_dim > 0) pl = e.linear(pl, proj);
      RUN(launch_copy_cols(e.dtype, pl->p, pl->cols, pooled, pl->cols, 0, n, pl->cols, e.stream));
    }
    return e.end_pass("this call (");
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
  return static_cast<ClipText*>(e->model.get())->forward(*e, n, ids, eos_pos, last_hidden, penultimate, pooled);
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
