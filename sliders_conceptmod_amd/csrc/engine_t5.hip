// The T5 encoder engine (transformers T5EncoderModel with a gated-GELU feed-forward: t5-v1.1-xxl, the text_encoder_2 of Flux
// and text_encoder_3 of SD3).  Pre-RMSNorm blocks on the op core (engine.h); the self-attention has no 1/sqrt(d) scale, no
// mask (the Flux and SD3 pipelines pass none: padding tokens are attended) and block 0's relative-position bias in every
// block.  The residual stream is stored in bf16 between the GEMMs, as transformers' bf16 model stores it; every GEMM adds
// its residual in fp32 before the one rounding.  Forward only -- except a tower created with LoRA sites on its
// SelfAttention.{q,k,v,o} (smi_t5_lora_*: the no-trigger trainer on Flux's and SD3's T5), which also saves a pass and
// differentiates it on the shared scaffold of engine.h: the RMSNorm, bias-table attention and gated GELU closures are here.
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
  // a tower created with LoRA sites (smi_t5_lora_create): arena 1 holds the saved pass and its backward
  bool trainable = false;
  Ten *out_last = nullptr, *out_pen = nullptr;  // hidden_states[-1] (after the final norm) and [-2] of the saved pass
  int saved_L = 0;
  explicit T5Encoder(const smi_t5_config& c, bool train = false) : cfg(c), trainable(train) {}
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
      // trainable: every Linear lies on the gradient path (a transposed copy for dX); the attention's four may carry sites
      L.qkv = e.make_fused(b + "0.SelfAttention", {"q", "k", "v"}, d, in, trainable);
      L.o = e.make_lin(b + "0.SelfAttention.o", in, d, false, trainable);
      L.n1 = rms(e, b + "1.layer_norm");
      L.wi = e.make_fused(ff, {"wi_0", "wi_1"}, d, cfg.d_ff, trainable);
      L.wo = e.make_lin(ff + ".wo", cfg.d_ff, d, false, trainable);
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
  // what a trainable tower packs after its layers (the forward-only create path packs its own: engine.hip build_model)
  void build_trainable(smi_engine& e) {
    build(e);
    e.finish_lora();
    e.gscale = (float*)e.pack_alloc(e.GSCALE_FLOATS * sizeof(float));
    e.samp_mult_dev = (float*)e.pack_alloc(2 * e.MAXS * sizeof(float));
    e.alloc_job_table(2 * e.sites.size() + 8);  // a fused q|k|v pushes at most 4 jobs for its 3 sites, o 2
    for (size_t i = 0; i < e.sites.size(); ++i)
      if (!e.site_used[i] && !e.err) {
        set_error("LoRA target '%s' is not a SelfAttention projection of this T5 encoder", e.site_names[i].c_str());
        e.err = true;
      }
  }
  void dry_forward(smi_engine& e) override {
    e.begin_forward_only_pass();
    forward(e, e.max_n, cfg.max_tokens, nullptr, (void*)16);
  }

  // the norm weight is frozen: the closure forms dx alone; the residual's gradient, when it is already in x's slot, rides in
  // the same launch (add may equal dx)
  Ten* rmsnorm(smi_engine& e, Ten* x, const Norm& nm) {
    Ten* y = e.new_ten(x->rows, x->cols, x->n, x->H, x->W);
    RUNP(SMI_PROF_NORM, 0.0, 4.0 * x->rows * x->cols,
         launch_rmsnorm_rows(e.dtype, x->p, nm.gamma, y->p, (int)x->rows, x->cols, nm.eps, e.stream));
    y->ng = x->ng;
    if (e.saving && y->ng) {
      smi_engine* ep = &e;
      const Norm* np = &nm;
      e.tape.push_back([=]() {
        smi_engine& e = *ep;
        if (!y->g) return;
        const smi_engine::Slot gs = e.grad_slot(x);
        RUNP(SMI_PROF_NORM, 0.0, 6.0 * e.MA(x) * x->cols,
             launch_rmsnorm_rows_bwd(e.dtype, e.PA(x), y->g, np->gamma, gs.add, gs.out, (int)e.MA(x), x->cols, np->eps, e.stream));
      });
    }
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
    o->ng = qkv->ng;
    const bool taped = e.saving && o->ng;
    if (taped) p.lse = e.alloc_f32((size_t)n * H * L);  // (the row statistic changes no bit of O)
    RUNP(SMI_PROF_ATTN, 4.0 * n * H * (double)L * L * p.D, 0.0, launch_attn_fwd(p, e.stream));
    if (taped) {
      smi_engine* ep = &e;
      e.tape.push_back([=]() {  // the table is frozen and shared by the blocks: the closure reads it, no gradient goes to it
        smi_engine& e = *ep;
        if (!o->g) return;
        AttnParams b = p;
        const int b0 = e.ad_first(o, L);
        b.B = n - b0;
        b.Q = (const char*)p.Q + (size_t)b0 * L * p.ldq * e.esz();
        b.K = (const char*)p.K + (size_t)b0 * L * p.ldk * e.esz();
        b.V = (const char*)p.V + (size_t)b0 * L * p.ldv * e.esz();
        b.O = e.PA(o);
        b.lse = p.lse + (size_t)b0 * H * L;
        b.dO = o->g;
        b.lddo = in;
        b.delta = e.alloc_f32((size_t)b.B * H * L);
        char* g = (char*)e.grad_slot(qkv).out;  // q|k|v has this one consumer: its slot is fresh
        b.dQ = g;
        b.dK = g + (size_t)in * e.esz();
        b.dV = g + (size_t)2 * in * e.esz();
        b.lddq = b.lddk = b.lddv = 3 * in;
        RUNP(SMI_PROF_ATTN, 10.0 * b.B * H * (double)L * L * b.D, 0.0, launch_attn_bwd(b, e.stream));
      });
    }
    return o;
  }
  Ten* gated_gelu(smi_engine& e, Ten* pj) {
    const int F = pj->cols / 2;
    Ten* y = e.new_ten(pj->rows, F, pj->n, pj->H, pj->W);
    RUNP(SMI_PROF_ELEM, 0.0, 6.0 * pj->rows * F, launch_gated_gelu_tanh(e.dtype, pj->p, y->p, pj->rows, F, e.stream));
    y->ng = pj->ng;
    if (e.saving && y->ng) {
      smi_engine* ep = &e;
      e.tape.push_back([=]() {
        smi_engine& e = *ep;
        if (!y->g) return;
        // (a slot that holds a gradient never happens in this graph: the projection has a single consumer)
        e.into_slot(e.grad_slot(pj), e.MA(pj), pj->cols, [&](void* dp) {
          RUNP(SMI_PROF_ELEM, 0.0, 10.0 * e.MA(pj) * F,
               launch_gated_gelu_tanh_bwd(e.dtype, e.PA(pj), y->g, dp, e.MA(pj), F, e.stream));
        });
      });
    }
    return y;
  }

  // the pass itself; whoever calls has begun it (begin_forward_only_pass, or begin_pass with every sample adapted)
  int forward(smi_engine& e, int n, int L, const int* ids, void* last_hidden, void* penultimate = nullptr) {
    const int d = cfg.d_model, H = cfg.num_heads;
    if (!e.prep_sites.empty() && (e.dry || (e.lora_down && e.lora_up && e.mult != 0.f)))
      RUNP(SMI_PROF_LORA, 0.0, 0.0, launch_lora_prep(e.dtype, e.prep_sites_dev, (int)e.prep_sites.size(), e.lora_down, e.lora_up, e.lora_shadow, e.stream));
    Ten* h = e.new_ten((int64_t)n * L, d, n, L, 1);  // the embeddings: no gradient flows into them (ng stays false)
    RUN(launch_embed(e.dtype, ids, tok, nullptr, h->p, (int64_t)n * L, L, d, cfg.vocab_size, e.stream));
    // one table per call, from block 0's weight, read by every block: offsets -(L - 1) .. L - 1 sit in the middle of the
    // buckets packed for max_tokens
    float* table = e.alloc_f32((size_t)H * (2 * L - 1));
    RUNP(SMI_PROF_ELEM, 0.0, 0.0,
         launch_t5_bias_table(e.dtype, rel_w, buckets_dev + (cfg.max_tokens - L), table, H, L, cfg.rel_buckets, e.stream));
    Ten* pen = h;
    for (int i = 0; i < cfg.num_layers; ++i) {
      const T5Layer& ly = layers[i];
      if (i == cfg.num_layers - 1) {  // hidden_states[-2]: what enters the last block
        pen = h;
        if (penultimate) RUN(launch_copy_cols(e.dtype, h->p, d, penultimate, d, 0, (int)h->rows, d, e.stream));
      }
      e.begin_block();
      Ten* qkv = e.linear(rmsnorm(e, h, ly.n0), ly.qkv);
      Ten* o = attention(e, qkv, table, n, L);
      h = e.linear(o, ly.o, h);
      Ten* f = gated_gelu(e, e.linear(rmsnorm(e, h, ly.n1), ly.wi));
      h = e.linear(f, ly.wo, h);
      e.end_block();
    }
    Ten* fin = rmsnorm(e, h, final_norm);  // hidden_states[-1] of T5Stack is AFTER the final norm: it is on the tape
    if (e.saving) {
      out_last = fin;
      out_pen = pen;
      saved_L = L;
      e.keep_saved_pass(n);
      e.saving = false;
    }
    if (last_hidden) RUN(launch_copy_cols(e.dtype, fin->p, d, last_hidden, d, 0, (int)fin->rows, d, e.stream));
    return e.end_pass("this call (");
  }

  // the shared backward (engine.h) with this model's two parts: which 0: d_hidden is the gradient of hidden_states[-1], so
  // the tape starts with the final norm's closure; 1: of hidden_states[-2], and the last block's closures see no gradient --
  // its sites get none.  One power-of-two loss scale per sample.  A backward consumes the saved pass.
  int backward(smi_engine& e, int which, const float* d_hidden, float* dd, float* du) {
    if (const int rc = e.begin_backward("smi_t5_backward: no saved forward pass (call smi_t5_forward_lora with save_for_backward=1 first)",
                                        dd, du, e.saved.n))
      return rc;
    Ten* y = which == 0 ? out_last : out_pen;
    if (!y->ng) {  // adaptor off, or nothing adapted upstream of hidden_states[-2]: the gradient is zero
      e.drop_tape();
      return 0;
    }
    const int n = e.saved.n, L = e.dry ? cfg.max_tokens : saved_L, d = cfg.d_model;
    RUN(launch_grad_scale(d_hidden, n, (int64_t)L * d, e.gscale, e.MAXS, e.stream));
    e.rebuild_saved_operands();
    y->g = e.alloc_t(e.MA(y), d);
    // f32 [n, L d] -> 16-bit rows, sample j x its loss scale: the cast of the UNet's d_eps with one "channel"
    RUN(launch_nchw_to_nhwc_scaled(e.dtype, d_hidden, y->g, n, 1, L * d, 1, e.gscale, e.stream));
    if (e.run_tape_and_weight_grads()) return -1;
    return e.end_pass("the backward (");
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

// a tower with LoRA sites: plain Linear LoRA on the self-attention's four projections only
int check_t5_lora(const smi_t5_config* c, const smi_lora_site* sites, int n_sites, int batch) {
  if (check_t5_cfg(c, batch)) return -1;
  SMI_CHECK(sites && n_sites > 0, "smi_t5_lora: no LoRA sites (a tower without them is smi_t5_create's)");
  SMI_CHECK(batch <= smi_engine::MAXS, "smi_t5_lora: batch %d exceeds the %d per-sample multipliers", batch, smi_engine::MAXS);
  return check_linear_lora_sites("smi_t5_lora", sites, n_sites,
                                 {".SelfAttention.q", ".SelfAttention.k", ".SelfAttention.v", ".SelfAttention.o"},
                                 "SelfAttention.{q,k,v} and SelfAttention.o");
}
T5Encoder* t5_lora_setup(smi_engine* e, const smi_t5_config* cfg, const smi_lora_site* sites, int n_sites, int batch) {
  T5Encoder* t = new T5Encoder(*cfg, true);
  e->hold(smi_engine::T5_ENCODER, t, cfg->dtype, batch);
  e->register_sites(sites, n_sites);
  return t;
}
// dry run at max_tokens: out = {packed weights, persistent region of arena 0 (the largest no-grad pass), one of its two block
// scratch regions, arena 1 (a saved pass and its backward from hidden_states[-1])}
int t5_lora_plan(const smi_t5_config* cfg, const smi_lora_site* sites, int n_sites, int batch, size_t out[4]) {
  smi_engine e;
  e.dry = true;
  T5Encoder& t = *t5_lora_setup(&e, cfg, sites, n_sites, batch);
  t.build_trainable(e);
  if (e.err) return -1;
  out[0] = align_up(e.wpack.peak, 4096);
  e.begin_pass(batch, false);  // the adapted no-grad pass allocates what the plain one does, and xa
  t.forward(e, batch, cfg->max_tokens, nullptr, (void*)16, (void*)16);
  out[1] = align_up(e.arena[0].peak, 4096);
  out[2] = align_up(std::max(e.scr[0].peak, e.scr[1].peak), 4096);
  e.begin_pass(batch, true);
  t.forward(e, batch, cfg->max_tokens, nullptr, (void*)16, (void*)16);
  t.backward(e, 0, nullptr, nullptr, nullptr);
  out[3] = align_up(e.arena[1].peak, 4096);
  return e.err ? -1 : 0;
}
size_t t5_plan_bytes(const size_t r[4]) { return r[0] + r[1] + 2 * r[2] + r[3] + 3 * 4096; }

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

// ---- T5 tower with LoRA sites: saved forward with one multiplier per sample, backward to the LoRA parameters ---------
int smi_t5_lora_workspace_bytes(const smi_t5_config* cfg, const smi_lora_site* sites, int n_sites, int batch, size_t* bytes) {
  if (check_t5_lora(cfg, sites, n_sites, batch)) return -1;
  SMI_CHECK(bytes != nullptr, "bad arguments");
  size_t r[4];
  if (t5_lora_plan(cfg, sites, n_sites, batch, r)) return -1;
  *bytes = t5_plan_bytes(r);
  return 0;
}

int smi_t5_lora_create(const smi_t5_config* cfg, const smi_weight* weights, int n_weights, const smi_lora_site* sites,
                       int n_sites, int batch, void* workspace, size_t workspace_bytes, void* stream, smi_engine** out) {
  if (check_t5_lora(cfg, sites, n_sites, batch)) return -1;
  SMI_CHECK(out && workspace && weights && n_weights > 0, "bad arguments");
  size_t r[4];
  if (t5_lora_plan(cfg, sites, n_sites, batch, r)) return -1;
  SMI_CHECK(t5_plan_bytes(r) <= workspace_bytes, "workspace too small: need %zu bytes, got %zu", t5_plan_bytes(r), workspace_bytes);
  smi_engine* e = new smi_engine();
  e->stream = (hipStream_t)stream;
  T5Encoder* t = t5_lora_setup(e, cfg, sites, n_sites, batch);
  for (int i = 0; i < n_weights; ++i) e->wmap[weights[i].name] = &weights[i];
  char* base = (char*)align_up((size_t)workspace, 4096);
  e->wpack.base = base;
  e->wpack.cap = r[0];
  e->arena[0].base = base + r[0];
  e->set_arena0_regions(r[1], r[2]);
  e->arena[1].base = base + r[0] + r[1] + 2 * r[2];
  e->arena[1].cap = r[3];
  t->build_trainable(*e);
  return finish_create(e, "the T5 weights", out);
}

int smi_t5_forward_lora(smi_engine* e, int n, int L, const int32_t* ids, const float* lora_down_flat, const float* lora_up_flat,
                        const float* multipliers, int save_for_backward, void* last_hidden, void* penultimate) {
  SMI_CHECK(e && e->kind == smi_engine::T5_ENCODER && ids, "smi_t5_forward_lora: NULL argument or not a T5 engine");
  T5Encoder* t = static_cast<T5Encoder*>(e->model.get());
  SMI_CHECK(t->trainable, "smi_t5_forward_lora: this engine has no LoRA sites (create it with smi_t5_lora_create)");
  SMI_CHECK(n >= 1 && n <= e->max_n, "batch %d outside [1, %d] the engine was created for", n, e->max_n);
  SMI_CHECK(L >= 1 && L <= t->cfg.max_tokens, "smi_t5_forward_lora: L %d outside [1, %d] (max_tokens) the engine was created for", L,
            t->cfg.max_tokens);
  SMI_CHECK(lora_down_flat && lora_up_flat && multipliers, "smi_t5_forward_lora: lora_down_flat, lora_up_flat and multipliers are required");
  e->err = false;
  // every adapted pass takes the per-sample route (sigma_i = m_i / max |m|), so that a sample gives the same bits alone and
  // in a batch; all multipliers 0 is the frozen tower
  float mref = 0.f;
  if (const int rc = e->set_sample_multipliers(multipliers, n, save_for_backward != 0, &mref)) return rc;
  smi::set_gemm_scratch(nullptr, 0);  // (as smi_t5_encode: no split-K scratch in the forward)
  e->begin_pass(n, save_for_backward != 0);
  e->lora_down = lora_down_flat;
  e->lora_up = lora_up_flat;
  e->mult = mref;
  e->samp_on = mref != 0.f;
  const int rc = t->forward(*e, n, L, ids, last_hidden, penultimate);
  e->samp_on = false;
  return rc;
}

int smi_t5_backward(smi_engine* e, int which, const float* d_hidden, float* d_lora_down_flat, float* d_lora_up_flat) {
  SMI_CHECK(e && e->kind == smi_engine::T5_ENCODER && d_hidden, "smi_t5_backward: NULL argument or not a T5 engine");
  T5Encoder* t = static_cast<T5Encoder*>(e->model.get());
  SMI_CHECK(t->trainable, "smi_t5_backward: this engine has no LoRA sites (create it with smi_t5_lora_create)");
  SMI_CHECK(which == 0 || which == 1, "smi_t5_backward: which must be 0 (last_hidden) or 1 (penultimate), got %d", which);
  e->err = false;
  smi::set_gemm_scratch(nullptr, 0);  // nor in the backward's GEMMs
  return t->backward(*e, which, d_hidden, d_lora_down_flat, d_lora_up_flat);
}

int smi_t5_relative_buckets(int num_buckets, int max_distance, int L, int32_t* out) {
  return t5_relative_buckets(num_buckets, max_distance, L, out);
}

}  // extern "C"
