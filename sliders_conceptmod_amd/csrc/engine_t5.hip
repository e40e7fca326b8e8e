// The T5 encoder engine (transformers T5EncoderModel with a gated-GELU feed-forward: t5-v1.1-xxl, the text_encoder_2 of Flux
// and text_encoder_3 of SD3).  Pre-RMSNorm blocks on the op core (engine.h); the self-attention has no 1/sqrt(d) scale, no
// mask (the Flux and SD3 pipelines pass none: padding tokens are attended) and block 0's relative-position bias in every
// block.  Forward only, no LoRA sites.  The residual stream is stored in bf16 between the GEMMs, as transformers' bf16 model
// stores it; every GEMM adds its residual in fp32 before the one rounding.
#include "engine.h"

namespace {

struct T5Layer {
  Norm n0, n1;
  Lin qkv, o, wi, wo;
};

struct T5Encoder : Model {
  smi_t5_config cfg{};
  std::vector<T5Layer> layers;
  Norm final_norm;
  const void* tok = nullptr;
  const void* rel_w = nullptr;         // block 0's relative_attention_bias.weight [rel_buckets, num_heads]
  int* buckets_dev = nullptr;          // bucket of every offset -(max_tokens - 1) .. max_tokens - 1
  std::vector<int32_t> buckets_host;   // (the upload's source: alive until finish_create has waited for the stream)
  explicit T5Encoder(const smi_t5_config& c) : cfg(c) {}
  int inner() const { return cfg.num_heads * cfg.d_kv; }

  Norm rms(smi_engine& e, const std::string& name) {  // T5LayerNorm: a weight and no bias
    Norm n;
    n.C = cfg.d_model;
    n.eps = cfg.eps;
    n.gamma = e.Wd(name + ".weight");
    e.check_shape(name + ".weight", {cfg.d_model});
    return n;
  }
  void build(smi_engine& e) override {
    const int d = cfg.d_model, in = inner();
    // the tied embedding: a transformers state dict carries it as `shared.weight`, as `encoder.embed_tokens.weight`, or both
    const std::string emb = (e.dry || e.wmap.count("shared.weight")) ? "shared.weight" : "encoder.embed_tokens.weight";
    tok = e.Wd(emb);
    e.check_shape(emb, {cfg.vocab_size, d});
    const std::string rel = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight";
    rel_w = e.Wd(rel);
    e.check_shape(rel, {cfg.rel_buckets, cfg.num_heads});
    layers.resize(cfg.num_layers);
    for (int i = 0; i < cfg.num_layers && !e.err; ++i) {
      const std::string b = "encoder.block." + std::to_string(i) + ".layer.";
      const std::string ff = b + "1.DenseReluDense";
      if (!e.dry && !e.wmap.count(ff + ".wi_0.weight") && e.wmap.count(ff + ".wi.weight")) {
        set_error("smi_t5: '%s.wi.weight' is a non-gated feed-forward (t5 v1.0); only the gated one (wi_0 / wi_1, "
                  "feed_forward_proj gated-gelu) is built", ff.c_str());
        e.err = true;
        break;
      }
      T5Layer& L = layers[i];
      L.n0 = rms(e, b + "0.layer_norm");
      L.qkv = e.make_fused(b + "0.SelfAttention", {"q", "k", "v"}, d, in, false);
      L.o = e.make_lin(b + "0.SelfAttention.o", in, d, false, false);
      L.n1 = rms(e, b + "1.layer_norm");
      L.wi = e.make_fused(ff, {"wi_0", "wi_1"}, d, cfg.d_ff, false);
      L.wo = e.make_lin(ff + ".wo", cfg.d_ff, d, false, false);
    }
    final_norm = rms(e, "encoder.final_layer_norm");
    const int n_off = 2 * cfg.max_tokens - 1;
    buckets_dev = (int*)e.pack_alloc((size_t)n_off * sizeof(int));
    if (!e.dry && !e.err) {
      buckets_host.resize(n_off);
      if (t5_relative_buckets(cfg.rel_buckets, cfg.rel_max_distance, cfg.max_tokens, buckets_host.data()) != 0 ||
          hipMemcpyAsync(buckets_dev, buckets_host.data(), (size_t)n_off * sizeof(int), hipMemcpyHostToDevice, e.stream) != hipSuccess) {
        e.err = true;
      }
    }
  }
  void dry_forward(smi_engine& e) override {
    e.begin_forward_only_pass();
    forward(e, e.max_n, cfg.max_tokens, nullptr, (void*)16);
  }

  Ten* rmsnorm(smi_engine& e, Ten* x, const Norm& nm) {
    Ten* y = e.new_ten(x->rows, x->cols, x->n, x->H, x->W);
    RUNP(SMI_PROF_NORM, 0.0, 4.0 * x->rows * x->cols,
         launch_rmsnorm_rows(e.dtype, x->p, nm.gamma, y->p, (int)x->rows, x->cols, nm.eps, e.stream));
    return y;
  }
  Ten* attention(smi_engine& e, Ten* qkv, const float* table, int n, int L) {
    const int H = cfg.num_heads, in = inner();
    Ten* o = e.new_ten(qkv->rows, in, n, L, 1);
    AttnParams p;
    p.dtype = e.dtype;
    p.B = n;
    p.H = H;
    p.Nq = p.Nk = L;
    p.D = cfg.d_kv;
    p.scale = 1.f;  // T5 folds the scale into its initialisation
    p.Q = qkv->p;
    p.K = (char*)qkv->p + (size_t)in * e.esz();
    p.V = (char*)qkv->p + (size_t)2 * in * e.esz();
    p.ldq = p.ldk = p.ldv = 3 * in;
    p.O = o->p;
    p.ldo = in;
    p.bias = table;
    p.bias_ld = 2 * L - 1;
    RUNP(SMI_PROF_ATTN, 4.0 * n * H * (double)L * L * p.D, 0.0, launch_attn_fwd(p, e.stream));
    return o;
  }
  Ten* gated_gelu(smi_engine& e, Ten* pj) {
    const int F = pj->cols / 2;
    Ten* y = e.new_ten(pj->rows, F, pj->n, pj->H, pj->W);
    RUNP(SMI_PROF_ELEM, 0.0, 6.0 * pj->rows * F, launch_gated_gelu_tanh(e.dtype, pj->p, y->p, pj->rows, F, e.stream));
    return y;
  }

  // the pass itself; whoever calls has begun it
  int forward(smi_engine& e, int n, int L, const int* ids, void* last_hidden) {
    const int d = cfg.d_model, H = cfg.num_heads;
    Ten* h = e.new_ten((int64_t)n * L, d, n, L, 1);
    RUN(launch_embed(e.dtype, ids, tok, nullptr, h->p, (int64_t)n * L, L, d, cfg.vocab_size, e.stream));
    // one table per call, from block 0's weight, read by every block: offsets -(L - 1) .. L - 1 sit in the middle of the
    // buckets packed for max_tokens
    float* table = e.alloc_f32((size_t)H * (2 * L - 1));
    RUNP(SMI_PROF_ELEM, 0.0, 0.0,
         launch_t5_bias_table(e.dtype, rel_w, buckets_dev + (cfg.max_tokens - L), table, H, L, cfg.rel_buckets, e.stream));
    for (int i = 0; i < cfg.num_layers; ++i) {
      const T5Layer& ly = layers[i];
      e.begin_block();
      Ten* qkv = e.linear(rmsnorm(e, h, ly.n0), ly.qkv);
      Ten* o = attention(e, qkv, table, n, L);
      h = e.linear(o, ly.o, h);
      Ten* f = gated_gelu(e, e.linear(rmsnorm(e, h, ly.n1), ly.wi));
      h = e.linear(f, ly.wo, h);
      e.end_block();
    }
    Ten* fin = rmsnorm(e, h, final_norm);
    if (last_hidden) RUN(launch_copy_cols(e.dtype, fin->p, d, last_hidden, d, 0, (int)fin->rows, d, e.stream));
    return e.end_pass("this call (");
  }
};

int check_t5_cfg(const smi_t5_config* c, int batch) {
  SMI_CHECK(c != nullptr, "config is NULL");
  SMI_CHECK(c->dtype != SMI_DTYPE_F16,
            "smi_t5: dtype f16 is refused -- T5's activations overflow it (the residual stream of t5-v1.1-xxl exceeds 65504); "
            "the tower runs in bf16 (1)");
  SMI_CHECK(c->dtype == SMI_DTYPE_BF16, "smi_t5: dtype must be bf16 (1), got %d", c->dtype);
  SMI_CHECK(c->d_kv == 64, "smi_t5: d_kv %d -- the attention with a relative-position bias is built for head_dim 64 only", c->d_kv);
  SMI_CHECK(c->d_model > 0 && c->d_model % 64 == 0 && c->d_model <= 8192,
            "smi_t5: d_model %d must be a multiple of 64 and at most 8192", c->d_model);
  SMI_CHECK(c->d_ff > 0 && c->d_ff % 64 == 0, "smi_t5: d_ff %d must be a multiple of 64", c->d_ff);
  SMI_CHECK(c->num_heads >= 1 && c->num_layers >= 1 && c->vocab_size >= 1 && batch >= 1,
            "smi_t5: config out of range (num_heads, num_layers, vocab_size, batch >= 1)");
  SMI_CHECK(c->rel_buckets >= 4 && c->rel_buckets % 2 == 0 && c->rel_max_distance > c->rel_buckets / 4,
            "smi_t5: rel_buckets %d must be even and >= 4, rel_max_distance %d above rel_buckets / 4", c->rel_buckets,
            c->rel_max_distance);
  SMI_CHECK(c->max_tokens >= 1 && c->max_tokens <= ATTN_BIAS_MAX_L, "smi_t5: max_tokens %d outside [1, %d]", c->max_tokens,
            ATTN_BIAS_MAX_L);
  SMI_CHECK(c->eps > 0.f, "smi_t5: eps must be positive");
  return 0;
}
Setup t5_setup(const smi_t5_config* cfg, int batch) {
  return [=](smi_engine* e) { e->hold(smi_engine::T5_ENCODER, new T5Encoder(*cfg), cfg->dtype, batch); };
}

}  // namespace

extern "C" {

int smi_t5_workspace_bytes(const smi_t5_config* cfg, int batch, size_t* bytes) {
  if (check_t5_cfg(cfg, batch)) return -1;
  return workspace_bytes_forward_only(t5_setup(cfg, batch), bytes);
}

int smi_t5_create(const smi_t5_config* cfg, const smi_weight* weights, int n_weights, int batch, void* workspace,
                  size_t workspace_bytes, void* stream, smi_engine** out) {
  if (check_t5_cfg(cfg, batch)) return -1;
  return create_forward_only(t5_setup(cfg, batch), "the T5 weights", weights, n_weights, workspace, workspace_bytes, stream,
                             out);
}

int smi_t5_encode(smi_engine* e, int n, int L, const int32_t* ids, void* last_hidden) {
  SMI_CHECK(e && e->kind == smi_engine::T5_ENCODER && ids && last_hidden,
            "smi_t5_encode: NULL argument or not a T5 engine (create it with smi_t5_create)");
  T5Encoder* t = static_cast<T5Encoder*>(e->model.get());
  SMI_CHECK(n >= 1 && n <= e->max_n, "batch %d outside [1, %d] the engine was created for", n, e->max_n);
  SMI_CHECK(L >= 1 && L <= t->cfg.max_tokens, "smi_t5_encode: L %d outside [1, %d] (max_tokens) the engine was created for", L,
            t->cfg.max_tokens);
  e->err = false;
  // no split-K scratch is lent: the slice count follows the launch's row count, so with one a prompt's bits would depend on
  // its batch
  smi::set_gemm_scratch(nullptr, 0);
  e->begin_forward_only_pass();
  return t->forward(*e, n, L, ids, last_hidden);
}

int smi_t5_relative_buckets(int num_buckets, int max_distance, int L, int32_t* out) {
  return t5_relative_buckets(num_buckets, max_distance, L, out);
}

}  // extern "C"
