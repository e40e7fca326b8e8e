/* smi.h -- C ABI of libsmi_hip.so: the MI355X-native (gfx950) hot path of the concept-slider LoRA trainer.
 *
 * The reference (ntc-ai/sliders-conceptmod) is pure Python and has no FFI of its own; the seam this library sits
 * under is the duck-typed model call the reference's step helpers make,
 *     unet(sample, timestep, encoder_hidden_states=..., added_cond_kwargs=...).sample
 * (conceptmod/textsliders/train_util.py:290-294 and :471-476), together with the autograd backward that
 * `loss.backward()` triggers through it (train_lora.py:298, train_lora_xl.py:348) and the elementwise step ops
 * around it.  Each entry point below names the reference code it replaces.  The Python binding a maintainer adds on
 * the reference side is shown in INTEGRATION.md (ctypes; the in-tree one is sliders_conceptmod_amd/_native.py).
 *
 * Conventions: plain pointers and sizes only; every pointer is a DEVICE pointer unless it says "host"; the caller
 * owns all memory (weights, LoRA parameters, gradients, latents, the workspace) and the library borrows it for the
 * duration of a call (the workspace: for the lifetime of the engine).  All work is enqueued on the `stream` given at
 * creation (a hipStream_t passed as void*, NULL = default stream); no call synchronises with the host.  Every
 * function returns 0 on success and a negative value on error; smi_last_error() then returns a message.
 * Nothing throws across the boundary.
 */
#ifndef SMI_H_
#define SMI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMI_MAX_LEVELS 8
#define SMI_DTYPE_F16 0
#define SMI_DTYPE_BF16 1

/* Architecture of the diffusers UNet2DConditionModel being replaced (the values of its public config). */
typedef struct smi_unet_config {
  int dtype;                 /* storage / MFMA input type of weights and activations; accumulation is always fp32 */
  int in_channels;           /* 4 */
  int out_channels;          /* 4 */
  int n_levels;              /* len(block_out_channels) */
  int block_out_channels[SMI_MAX_LEVELS];
  int down_has_attn[SMI_MAX_LEVELS]; /* CrossAttnDownBlock2D (1) or DownBlock2D (0) */
  int up_has_attn[SMI_MAX_LEVELS];   /* CrossAttnUpBlock2D (1) or UpBlock2D (0), in up_blocks order */
  int layers_per_block;
  int transformer_layers[SMI_MAX_LEVELS]; /* per down level */
  int num_heads[SMI_MAX_LEVELS];          /* per down level (diffusers "attention_head_dim") */
  int mid_transformer_layers;
  int cross_attention_dim;
  int norm_num_groups;
  int use_linear_projection;
  int addition_embed;        /* 1 = SD-XL "text_time" conditioning */
  int addition_time_embed_dim;
  int projection_class_embeddings_input_dim;
} smi_unet_config;

/* One frozen weight tensor, named as in the diffusers state_dict ("down_blocks.0.resnets.0.conv1.weight"),
 * already in `dtype`, contiguous, torch layout. */
typedef struct smi_weight {
  const char* name;
  const void* data;
  int ndim;
  int64_t shape[4];
} smi_weight;

/* One LoRA-adapted Linear (reference: LoRAModule, conceptmod/textsliders/lora.py:76-138).
 * `target` is the dotted module path ("down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q").
 * lora_down.weight [rank, in] lives at down_flat + off_down, lora_up.weight [out, rank] at up_flat + off_up
 * (element offsets into the two flat fp32 buffers passed per call). scale = alpha / rank (lora.py:118-119). */
typedef struct smi_lora_site {
  const char* target;
  int64_t off_down;
  int64_t off_up;
  int rank;
  float scale;
  /* DoRA (conceptmod/textsliders/dora.py:53-162): element offset of this site's dora_scale [1, in] inside the UP flat
   * buffer (gradients accumulate at the same offset of the up-gradient buffer); < 0: a plain LoRA site.
   * dW = (W + up down) * (dora_scale / ||W + up down||_col) - W, y += scale * multiplier * x dW^T. */
  int64_t off_dora;
} smi_lora_site;

/* Architecture of the diffusers AutoencoderKL ENCODER half (image sliders encode their image pairs with it every step:
 * trainscripts/imagesliders/train_util.py:213-222). */
typedef struct smi_vae_config {
  int dtype;
  int in_channels;      /* 3 */
  int latent_channels;  /* 4: the encoder emits 2 x latent_channels moments (mean | logvar) */
  int n_levels;         /* len(block_out_channels) */
  int block_out_channels[SMI_MAX_LEVELS]; /* (128, 256, 512, 512) */
  int layers_per_block; /* 2 */
  int norm_num_groups;  /* 32 */
  int no_post_quant_conv; /* decoder only: != 0 skips post_quant_conv (SD3's 16-channel VAE has none); 0 everywhere else */
} smi_vae_config;

/* Architecture of a transformers CLIPTextModel / CLIPTextModelWithProjection (the prompt front end:
 * conceptmod/textsliders/train_util.py:108-155 `text_encode`, `text_encode_xl`). */
typedef struct smi_clip_config {
  int dtype;
  int vocab_size;        /* 49408 */
  int hidden_size;       /* 768 (CLIP ViT-L/14 text) / 1280 (OpenCLIP bigG) */
  int num_layers;        /* 12 / 32 */
  int num_heads;         /* 12 / 20 */
  int intermediate_size; /* 3072 / 5120 */
  int max_positions;     /* 77 */
  int hidden_act;        /* 0 quick_gelu, 1 gelu */
  int projection_dim;    /* 0: none (CLIPTextModel); > 0: text_projection (CLIPTextModelWithProjection) */
} smi_clip_config;

/* Architecture of a transformers CLIPVisionModel / CLIPVisionModelWithProjection (the image tower of CLIPModel: what
 * eval-scripts/clip_score.py scores a slider sweep with). */
typedef struct smi_clip_vision_config {
  int dtype;
  int hidden_size;       /* 768 (ViT-B/32) / 1024 (ViT-L/14) */
  int num_layers;        /* 12 / 24 */
  int num_heads;         /* 12 / 16 */
  int intermediate_size; /* 3072 / 4096 */
  int image_size;        /* 224 */
  int patch_size;        /* 32 / 14 */
  int hidden_act;        /* 0 quick_gelu, 1 gelu */
  int projection_dim;    /* 0: pooled = post_layernorm(class row); > 0: x visual_projection (512 / 768) */
  float image_mean[3];   /* CLIPImageProcessor image_mean / image_std: applied to uint8 input only */
  float image_std[3];
} smi_clip_vision_config;

/* LPIPS v0.1 on AlexNet (`lpips.LPIPS(net='alex')`, what eval-scripts/lpip_score.py scores a sweep with).  The geometry is
 * AlexNet's and fixed: conv k 11 / stride 4 / pad 2, max-pool 3 / 2, conv k 5 / pad 2, max-pool 3 / 2, three convs k 3 / pad 1,
 * a tap after every ReLU.  The widths are configurable, for tiny test nets. */
typedef struct smi_lpips_config {
  int dtype;
  int channels[5]; /* (64, 192, 384, 256, 256) */
} smi_lpips_config;

/* Architecture of a diffusers SD3Transformer2DModel (the MMDiT of Stable Diffusion 3 medium; what
 * conceptmod/textsliders/train_lora_sd3.py and predict_noise_sd3 drive).  Width d = num_heads x attention_head_dim. */
typedef struct smi_mmdit_config {
  int dtype;
  int patch_size;             /* 2 */
  int in_channels;            /* 16: in_channels x patch_size^2 must be a multiple of 64 (the patch GEMM's K) */
  int out_channels;           /* 16 */
  int num_layers;             /* 24: the last block is context_pre_only */
  int num_heads;              /* 24 */
  int attention_head_dim;     /* 64 (the only one built) */
  int joint_attention_dim;    /* 4096: width of encoder_hidden_states */
  int pooled_projection_dim;  /* 2048 */
  int pos_embed_max_size;     /* 192: pos_embed.pos_embed is [1, 192 x 192, d] */
  int context_len;            /* tokens per sample of encoder_hidden_states (77 + the T5 block, e.g. 333): fixed at creation */
  int dual_attention_layers;  /* number of blocks with a second, image-only attention (SD3.5): must be 0 */
  int qk_norm;                /* 0 none; 1 rms_norm (SD3.5): refused */
} smi_mmdit_config;

/* Architecture of a diffusers FluxTransformer2DModel (FLUX.1-schnell / dev; what conceptmod/textsliders/train_lora_flux.py
 * and predict_noise_flux drive).  Width d = num_heads x attention_head_dim; out_channels = in_channels. */
typedef struct smi_flux_config {
  int dtype;
  int in_channels;            /* 16: in_channels x patch_size^2 (the packed width, 64) must be a multiple of 64 */
  int patch_size;             /* 2 */
  int num_layers;             /* 19 double (joint) blocks */
  int num_single_layers;      /* 38 single blocks */
  int num_heads;              /* 24 */
  int attention_head_dim;     /* 128: a multiple of 16, at most 160 */
  int joint_attention_dim;    /* 4096: width of encoder_hidden_states (T5) */
  int pooled_projection_dim;  /* 768: CLIP-L's pooled row */
  int guidance_embeds;        /* 0 schnell, 1 dev: a guidance embedder next to the timestep embedder */
  int axes_dims_rope[3];      /* (16, 56, 56): even, summing to attention_head_dim */
  int context_len;            /* tokens per sample of encoder_hidden_states: fixed at creation */
  float rope_theta;           /* 10000 */
} smi_flux_config;

/* Architecture of a transformers T5EncoderModel with a gated-GELU feed-forward (google/t5-v1_1-xxl: the text_encoder_2 of
 * Flux and text_encoder_3 of SD3).  inner = num_heads x d_kv may differ from d_model. */
typedef struct smi_t5_config {
  int dtype;            /* bf16 only: T5's activations overflow f16 */
  int vocab_size;       /* 32128 */
  int d_model;          /* 4096: a multiple of 64, at most 8192 */
  int d_kv;             /* 64 (the only one built) */
  int num_heads;        /* 64 */
  int d_ff;             /* 10240: a multiple of 64 */
  int num_layers;       /* 24 */
  int rel_buckets;      /* 32: relative_attention_num_buckets */
  int rel_max_distance; /* 128: relative_attention_max_distance */
  int max_tokens;       /* longest sequence a call may pass (512 serves Flux's 256 / 512 and SD3's 256); at most 2048 */
  float eps;            /* 1e-6: layer_norm_epsilon */
} smi_t5_config;

typedef struct smi_engine smi_engine;

const char* smi_last_error(void);

/* Bytes of device workspace an engine needs for UNet batch `batch` (= 2B of the reference's CFG-doubled batch,
 * train_util.py:285, or 4 x 2B when the four guidance passes run as one batched pass), of which at most
 * `batch_adapted` samples are LoRA-adapted and differentiated, latent h x w, context length ctx_len, and the given
 * set of adapted layers. */
int smi_workspace_bytes(const smi_unet_config* cfg, const smi_lora_site* sites, int n_sites, int batch,
                        int batch_adapted, int h, int w, int ctx_len, size_t* bytes);

/* Builds the engine: packs the frozen weights into MFMA-friendly layouts inside `workspace` (transposed copies for
 * the activation-gradient GEMMs, (ky,kx,ci)-ordered conv filters, fused q|k|v) and lays out the activation arenas.
 * Replaces: unet.to(device, dtype); unet.requires_grad_(False); unet.eval(); LoRANetwork(...).apply_to()
 * (train_lora.py:67-78). */
int smi_create(const smi_unet_config* cfg, const smi_weight* weights, int n_weights, const smi_lora_site* sites,
               int n_sites, int batch, int batch_adapted, int h, int w, int ctx_len, void* workspace,
               size_t workspace_bytes, void* stream, smi_engine** out);
void smi_destroy(smi_engine* e);

/* Engine lifetime across shapes.  The packed weights do not depend on the batch or the latent size; only the two
 * activation arenas do.  smi_workspace_bytes == smi_weights_bytes + smi_arena_bytes (+ alignment slack).
 * smi_replan switches a live engine to another (batch, batch_adapted, h, w, ctx_len) WITHOUT re-packing any weight:
 * `arena` is a caller-owned buffer of >= smi_arena_bytes(...) bytes that must outlive its use (NULL: reuse the arena
 * region of the creation workspace, if large enough).  It invalidates a saved forward (smi_unet_backward then fails
 * with -4).  This is what the reference's `dynamic_resolution` (a random bucket every step, train_util.py:1085-1097;
 * train_lora.py:172-178) needs: keep one arena per bucket and replan between them. */
int smi_weights_bytes(const smi_unet_config* cfg, const smi_lora_site* sites, int n_sites, size_t* bytes);
int smi_arena_bytes(const smi_unet_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int batch_adapted,
                    int h, int w, int ctx_len, size_t* bytes);
int smi_replan(smi_engine* e, int batch, int batch_adapted, int h, int w, int ctx_len, void* arena,
               size_t arena_bytes);
/* out[0] = weight-packing kernel launches since creation, out[1] = replans, out[2] = generation number of the saved
 * forward whose tape is live (0: none; each save_for_backward forward gets a new number -- callers keep it next to the
 * output they will differentiate and compare before smi_unet_backward), out[3] = bytes of the packed-weight region. */
int smi_engine_stats(const smi_engine* e, int64_t out[4]);

/* ---- AutoencoderKL encoder (image sliders) ------------------------------------------------------------------------
 * moments = quant_conv(encoder(image)): replaces `vae.encode(image)` up to the posterior's parameters
 * (trainscripts/imagesliders/train_util.py:218: `vae.encode(image).latent_dist`); the caller draws the sample
 * (mean + exp(0.5 clamp(logvar, -30, 20)) eps) and multiplies by scaling_factor (:219-220).
 *   weights: diffusers AutoencoderKL state_dict entries `encoder.*` and `quant_conv.*`, dtype T
 *   image   f32 [n, 3, h, w], already preprocessed to [-1, 1] (VaeImageProcessor.preprocess)
 *   moments f32 [n, 2 * latent_channels, h / 8, w / 8]   (mean | logvar, unclamped)
 * h, w are the IMAGE size (multiples of 8 x 2^(n_levels-1)/... : each level but the last halves it).  Same ownership
 * rules as the UNet engine; smi_destroy frees it. */
int smi_vae_workspace_bytes(const smi_vae_config* cfg, int batch, int h, int w, size_t* bytes);
int smi_vae_create(const smi_vae_config* cfg, const smi_weight* weights, int n_weights, int batch, int h, int w,
                   void* workspace, size_t workspace_bytes, void* stream, smi_engine** out);
int smi_vae_encode(smi_engine* e, int n, const float* image, float* moments_out);

/* ---- AutoencoderKL decoder (looking at a trained slider) ---------------------------------------------------------------
 * image = decoder(post_quant_conv(latents)): replaces `vae.decode(latents / scaling_factor).sample` and the eval scripts'
 * post-processing (eval-scripts/generate_images_sd1.py:195-200).
 *   weights  diffusers AutoencoderKL state_dict entries `decoder.*` and `post_quant_conv.*`, dtype T (same size rule as
 *            the encoder: h, w multiples of f = 2^(n_levels-1); w also a multiple of 4; in_channels <= 4; latent_channels
 *            up to 16 here (SD3), and no `post_quant_conv.*` entries when cfg.no_post_quant_conv is set)
 *   latents  f32 [n, latent_channels, h/f, w/f]: what `vae.decode(z)` receives, i.e. ALREADY divided by scaling_factor
 *   image    f32 [n, in_channels, h, w]: `vae.decode(z).sample`, unclamped
 *   rgb8     optional (NULL: skipped) uint8 [n, h, w, in_channels] = round_half_even(clamp(sample/2 + 0.5, 0, 1) * 255)
 * Creation refuses a batch whose largest conv operand would cross the GEMM's 4 GiB limit (SD config: 7 images at 1024^2,
 * 31 at 512^2); the message names the largest batch that fits.  smi_vae_encode refuses a decoder engine, smi_vae_decode
 * an encoder engine, and every UNet entry point both.  SMI_VAE_DEC_TAIL=0 (read at creation): the unfused tail. */
int smi_vae_decoder_workspace_bytes(const smi_vae_config* cfg, int batch, int h, int w, size_t* bytes);
int smi_vae_decoder_create(const smi_vae_config* cfg, const smi_weight* weights, int n_weights, int batch, int h, int w,
                           void* workspace, size_t workspace_bytes, void* stream, smi_engine** out);
int smi_vae_decode(smi_engine* e, int n, const float* latents, float* image_out, uint8_t* rgb8_out);

/* ---- CLIP text encoder (prompt front end) -----------------------------------------------------------------------------
 * Replaces `text_encoder(tokens)[0]` (train_util.py:119-120) and `text_encoder(tokens, output_hidden_states=True)`
 * -> `[0]`, `.hidden_states[-2]` (train_util.py:139-144).  Causal self-attention, pre-LayerNorm blocks.
 *   weights: the transformers state_dict (`text_model.embeddings.token_embedding.weight`, ...,
 *            `text_model.final_layer_norm.*`, `text_projection.weight` when projection_dim > 0), dtype T
 *   ids         int32 [n, max_positions]   token ids (host tokenizer output)
 *   eos_pos     int32 [n]                  position of the pooled token (transformers: the EOS token)
 *   last_hidden T [n, L, hidden]  final_layer_norm(output of the last layer)            (may be NULL)
 *   penultimate T [n, L, hidden]  output of layer num_layers-1, no final norm = hidden_states[-2]   (may be NULL)
 *   pooled      T [n, projection_dim or hidden]  last_hidden[eos_pos] (x text_projection)           (may be NULL) */
int smi_clip_workspace_bytes(const smi_clip_config* cfg, int batch, size_t* bytes);
int smi_clip_create(const smi_clip_config* cfg, const smi_weight* weights, int n_weights, int batch, void* workspace,
                    size_t workspace_bytes, void* stream, smi_engine** out);
int smi_clip_encode(smi_engine* e, int n, const int32_t* ids, const int32_t* eos_pos, void* last_hidden,
                    void* penultimate, void* pooled);

/* smi_clip_encode with one more optional output: last_layer_out T [n, L, hidden] = hidden_states[-1], the last layer's output
 * WITHOUT the final norm (what conceptmod/notrigger/train_notrigger.py:241 reads). */
int smi_clip_encode_layers(smi_engine* e, int n, const int32_t* ids, const int32_t* eos_pos, void* last_hidden,
                           void* penultimate, void* pooled, void* last_layer_out);

/* ---- T5 encoder (the sequence embedding of Flux and SD3 prompts) --------------------------------------------------------
 * Replaces `transformers.T5EncoderModel(input_ids)[0]` without an attention mask, as the Flux and SD3 pipelines call it
 * (padding tokens are attended).  Per block: h += o(attention(q|k|v(rmsnorm(h)))), h += wo(gelu_tanh(wi_0 x) * (wi_1 x)) with
 * x = rmsnorm(h); then final_layer_norm.  The attention has no 1/sqrt(d_kv) scale and adds block 0's relative-position bias
 * in every block: one f32 [num_heads, 2 L - 1] table per call, indexed by key - query, never an [H, L, L] tensor.  The
 * residual stream is stored in bf16 between the GEMMs.  Forward only; no LoRA sites (a tower with them: smi_t5_lora_*).
 *   weights: the transformers state_dict (`shared.weight` or `encoder.embed_tokens.weight`,
 *            `encoder.block.N.layer.0.SelfAttention.{q,k,v,o}.weight`, block 0's `...relative_attention_bias.weight`,
 *            `encoder.block.N.layer.{0,1}.layer_norm.weight`, `encoder.block.N.layer.1.DenseReluDense.{wi_0,wi_1,wo}.weight`,
 *            `encoder.final_layer_norm.weight`), bf16
 *   ids         int32 [n, L]   token ids, 1 <= L <= max_tokens, any L (no alignment); an id outside the vocabulary is clamped
 *                              into it, as smi_clip_encode does
 *   last_hidden T [n, L, d_model]
 * One engine serves every L up to max_tokens and every n up to batch; a prompt gives the same bits alone and in a batch.
 * Refused, each with its reason in smi_last_error: dtype f16, d_kv != 64, d_model or d_ff not a multiple of 64, L out of
 * range, a missing or misshapen weight, a non-gated feed-forward (`wi` instead of `wi_0` / `wi_1`).
 * smi_t5_relative_buckets: host only (callable without a GPU) -- transformers' bidirectional _relative_position_bucket of
 * the offsets key - query = -(L - 1) .. L - 1, out[key - query + L - 1]. */
int smi_t5_workspace_bytes(const smi_t5_config* cfg, int batch, size_t* bytes);
int smi_t5_create(const smi_t5_config* cfg, const smi_weight* weights, int n_weights, int batch, void* workspace,
                  size_t workspace_bytes, void* stream, smi_engine** out);
int smi_t5_encode(smi_engine* e, int n, int L, const int32_t* ids, void* last_hidden);
int smi_t5_relative_buckets(int num_buckets, int max_distance, int L, int32_t* out);

/* ---- CLIP text tower with LoRA sites (the no-trigger text-encoder trainer) --------------------------------------------
 * The same tower, created with Linear LoRA sites (rank <= 16) on self_attn.{q,k,v}_proj -- all three of a layer or none,
 * adjacent in the flat buffers in that order, as the UNet's fused attn1 -- and self_attn.out_proj.  DoRA sites, other
 * targets, head_dim != 64 and more than 128 positions are refused.  workspace = [packed weights | no-grad arena | arena of
 * the saved pass and its backward], sized by a dry forward + backward.
 * smi_clip_forward_lora: every sample is adapted, sample i at multipliers[i] (f32, HOST memory, [n]); the effective weight
 * of a site is W + m_i (alpha / r) up down.  All multipliers 0 gives the bits of smi_clip_encode, which also runs on such
 * an engine.  Outputs, T [n, L, hidden] (pooled: [n, projection_dim or hidden]), any may be NULL: last_layer_out =
 * hidden_states[-1], the last layer's output WITHOUT the final norm; the other three as in smi_clip_encode.
 * save_for_backward: keeps the pass for ONE smi_clip_backward; a no-grad call in between leaves it intact.
 * smi_clip_backward: d_hidden f32 [n, L, hidden] is the gradient of last_layer_out (which 0) or of penultimate (which 1:
 * the last layer's sites then get none); accumulates (+=) into the flat gradient buffers.  No gradient flows into the
 * embeddings.  -4 without a saved pass. */
int smi_clip_lora_workspace_bytes(const smi_clip_config* cfg, const smi_lora_site* sites, int n_sites, int batch,
                                  size_t* bytes);
int smi_clip_lora_create(const smi_clip_config* cfg, const smi_weight* weights, int n_weights, const smi_lora_site* sites,
                         int n_sites, int batch, void* workspace, size_t workspace_bytes, void* stream, smi_engine** out);
int smi_clip_forward_lora(smi_engine* e, int n, const int32_t* ids, const int32_t* eos_pos, const float* lora_down_flat,
                          const float* lora_up_flat, const float* multipliers, int save_for_backward, void* last_layer_out,
                          void* penultimate, void* last_hidden, void* pooled);
int smi_clip_backward(smi_engine* e, int which, const float* d_hidden, float* d_lora_down_flat, float* d_lora_up_flat);

/* ---- T5 tower with LoRA sites (the no-trigger trainer on Flux's and SD3's T5) ----------------------------------------------
 * The T5 encoder above, created with Linear LoRA sites (rank <= 16) on encoder.block.N.layer.0.SelfAttention.{q,k,v} -- all
 * three of a block or none, adjacent in the flat buffers in that order: they ride on the fused q|k|v GEMM, as the CLIP
 * tower's -- and on SelfAttention.o.  DoRA sites, other targets and ranks above 16 are refused with the site and the reason.
 * bf16 only, as the forward.  workspace = [packed weights (every Linear twice: its transposed copy serves dX) | no-grad
 * arena and its two block scratch regions | arena of the saved pass and its backward], sized by a dry forward + backward at
 * max_tokens.
 * smi_t5_forward_lora: every sample is adapted, sample i at multipliers[i] (f32, HOST memory, [n]); the effective weight of a
 * site is W + m_i (alpha / r) up down.  All multipliers 0 gives the bits of smi_t5_encode, which also runs on such an
 * engine.  Outputs, T [n, L, d_model], either may be NULL: last_hidden = hidden_states[-1] of transformers' T5Stack, AFTER
 * final_layer_norm (unlike the CLIP tower's last_layer_out); penultimate = hidden_states[-2], the last block's input.
 * save_for_backward: keeps the pass for ONE smi_t5_backward; a no-grad call in between leaves it intact.  The backward
 * reads the saved pass's lora_down_flat / lora_up_flat again: they stay alive and unchanged until it has run.
 * smi_t5_backward: d_hidden f32 [n, L, d_model] is the gradient of last_hidden (which 0: the tape starts with the final
 * RMSNorm's backward) or of penultimate (which 1: the last block's sites then get none); accumulates (+=) into the flat
 * gradient buffers.  No gradient goes to the embedding, the norm weights or the bias table, and the tape stops at the first
 * block that has a site.  No split-K scratch is lent to the GEMMs of either direction.  -4 without a saved pass. */
int smi_t5_lora_workspace_bytes(const smi_t5_config* cfg, const smi_lora_site* sites, int n_sites, int batch, size_t* bytes);
int smi_t5_lora_create(const smi_t5_config* cfg, const smi_weight* weights, int n_weights, const smi_lora_site* sites,
                       int n_sites, int batch, void* workspace, size_t workspace_bytes, void* stream, smi_engine** out);
int smi_t5_forward_lora(smi_engine* e, int n, int L, const int32_t* ids, const float* lora_down_flat, const float* lora_up_flat,
                        const float* multipliers, int save_for_backward, void* last_hidden, void* penultimate);
int smi_t5_backward(smi_engine* e, int which, const float* d_hidden, float* d_lora_down_flat, float* d_lora_up_flat);

/* ---- CLIP image tower and similarity head (scoring a slider sweep) -----------------------------------------------------
 * Replaces `model.get_image_features(pixel_values)` / the image half of `CLIPModel(**inputs).logits_per_image`
 * (eval-scripts/clip_score.py).  Patch embedding (a GEMM on the patch matrix), class token + position embedding +
 * pre_layrnorm, the text tower's pre-LayerNorm blocks WITHOUT the causal mask, post_layernorm on the class row.
 *   weights: the transformers state_dict entries `vision_model.*` (+ `visual_projection.weight` when projection_dim > 0)
 *   rgb8         uint8 [n, S, S, 3]: resized and centre-cropped, NOT yet rescaled (normalised on the device)  } exactly
 *   pixel_values f32 [n, 3, S, S]: what CLIPImageProcessor returns                                           } one
 *   last_hidden  T [n, G*G + 1, hidden]  the encoder's output (no post_layernorm), G = S / patch_size   (may be NULL)
 *   image_embeds T [n, projection_dim or hidden]  post_layernorm(class row) (x visual_projection)
 * An image encodes to the same bits alone or in a batch.  The config check refuses image_size % patch_size != 0,
 * hidden_size % 64 != 0 or > 2048, head_dim % 8 != 0, intermediate_size % 64 != 0 and projection_dim % 8 != 0.
 * smi_clip_logits needs no engine: logits_per_image f32 [ni, nt] = exp(logit_scale) <i, t> / (|i| |t|), dim % 8 == 0. */
int smi_clip_vision_workspace_bytes(const smi_clip_vision_config* cfg, int batch, size_t* bytes);
int smi_clip_vision_create(const smi_clip_vision_config* cfg, const smi_weight* weights, int n_weights, int batch,
                           void* workspace, size_t workspace_bytes, void* stream, smi_engine** out);
int smi_clip_vision_encode(smi_engine* e, int n, const uint8_t* rgb8, const float* pixel_values, void* last_hidden,
                           void* image_embeds);
int smi_clip_logits(int dtype, const void* image_embeds, int ni, const void* text_embeds, int nt, int dim,
                    float logit_scale, float* logits_per_image, void* stream);

/* ---- LPIPS (AlexNet) distance between image pairs (how much structure a slider preserves) -----------------------------
 * Replaces `lpips.LPIPS(net='alex')(original, edited)` in eval mode (eval-scripts/lpip_score.py): scaling layer, the five
 * AlexNet convolutions (GEMMs on patch matrices) with a tap after every ReLU, per tap the channel-unit-normalised squared
 * difference through the 1x1 `lin` layer, averaged over the map; the five taps added in layer order.  The tower runs on
 * 2n images at once (a-images, then b-images); the head pairs image i with image n + i.
 *   weights: `features.{0,3,6,8,10}.weight` T [C_out, C_in, k, k] and `.bias` T [C_out] (torchvision's AlexNet names),
 *            `lin{0..4}.weight` T [1, C, 1, 1]; the scaling layer's shift / scale are constants of the metric
 *   rgb8_a, rgb8_b uint8 [n, h, w, 3]: x = u / 127.5 - 1 on the device          } exactly one form, both images of a pair
 *   img_a, img_b   f32 [n, 3, h, w] in [-1, 1]                                  } in the same one
 *   dist      f32 [n]
 *   per_layer f32 [n, 5]: the five terms of dist                                                    (may be NULL)
 *   feats     5 device pointers, T [2n, Ho, Wo, C] each: the post-ReLU taps, NHWC                   (may be NULL)
 * h, w are fixed at creation; n <= max_pairs.  Bit for bit: a pair scores the same alone or anywhere in any batch (no
 * split-K scratch is lent to the GEMMs, every other sum is ordered by the shape alone), d(a, b) == d(b, a), d(a, a) == 0.
 * Creation refuses h or w below 31 (the second pool would be empty), channel widths that are not multiples of 8 (16-byte
 * vector access and the GEMM's N % 8), max_pairs above 65535 and a patch matrix of 4 GiB or more (the GEMM's operand
 * limit: 2 max_pairs x map positions x padded k k C_in x 2 bytes).  smi_destroy frees the engine. */
int smi_lpips_workspace_bytes(const smi_lpips_config* cfg, int max_pairs, int h, int w, size_t* bytes);
int smi_lpips_create(const smi_lpips_config* cfg, const smi_weight* weights, int n_weights, int max_pairs, int h, int w,
                     void* workspace, size_t workspace_bytes, void* stream, smi_engine** out);
int smi_lpips_distance(smi_engine* e, int n, const uint8_t* rgb8_a, const uint8_t* rgb8_b, const float* img_a,
                       const float* img_b, float* dist, float* per_layer, void* const* feats);

/* ---- SD3 MMDiT, forward with LoRA sites (sweeping an SD3 slider) -------------------------------------------------------
 * Replaces `transformer(hidden_states, timestep, encoder_hidden_states, pooled_projections).sample`
 * (conceptmod/textsliders/train_util.py predict_noise_sd3).  Patch embedding (a GEMM on the patch matrix, columns (c, py, px))
 * + the centre-cropped window of pos_embed.pos_embed; temb = timestep MLP(256-wide sinusoid, cos first) + pooled-text MLP;
 * num_layers joint blocks: each stream is LN(h) (1 + scale) + shift under its own norm1[_context].linear(silu(temb)) chunks
 * (shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp; the last block's context stream: scale, shift only), the two
 * streams' q|k|v packed per sample into ONE non-causal attention over image tokens followed by context tokens, then
 * h += gate_msa to_out(attn), h += gate_mlp ff(LN(h) (1 + scale_mlp) + shift_mlp) with tanh-GELU; the last block drops its
 * context output.  norm_out (scale, shift) + proj_out, un-patchified with columns (py, px, c).
 *   weights      the diffusers state_dict (`pos_embed.proj.*`, `pos_embed.pos_embed`, `context_embedder.*`,
 *                `time_text_embed.*`, `transformer_blocks.<i>.*`, `norm_out.linear.*`, `proj_out.*`), dtype T
 *   sites        Linear LoRA sites (rank <= 16) on attn.to_q/to_k/to_v (all three of a block or none, adjacent in the flat
 *                buffers in that order: one fused GEMM), attn.add_q_proj/add_k_proj/add_v_proj (likewise), attn.to_out.0 and
 *                attn.to_add_out; n_sites 0: a frozen network.  DoRA sites and other targets are refused by name.
 *   h, w         the LATENT size, multiples of patch_size, grid <= pos_embed_max_size; fixed at creation, as context_len is
 *   sample       f32 [n, in_channels, h, w]
 *   timesteps    f32 [n], HOST memory: the scheduler's 1000 sigma, one per sample
 *   ctx          T [n, context_len, joint_attention_dim]
 *   pooled       T [n, pooled_projection_dim]
 *   multipliers  f32 [n], HOST memory: sample i runs at W + m_i (alpha / r) up down.  NULL flat buffers, NULL multipliers or
 *                all multipliers 0 give the bits of an engine created without sites.
 *   out          f32 [n, out_channels, h, w]
 * workspace = [packed weights | arena], sized by a dry forward.  n may be smaller than the creation batch.  No split-K
 * scratch is lent to the GEMMs and every other sum is ordered by the shape: a sample gives the same bits alone or anywhere
 * in a batch.  The config check refuses d % 64, d > 2048, attention_head_dim != 64, in_channels x patch_size^2 % 64, h or w
 * not a multiple of patch_size, a grid above pos_embed_max_size, and dual_attention_layers / qk_norm (SD3.5) by name. */
int smi_mmdit_workspace_bytes(const smi_mmdit_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int h, int w,
                              size_t* bytes);
int smi_mmdit_create(const smi_mmdit_config* cfg, const smi_weight* weights, int n_weights, const smi_lora_site* sites,
                     int n_sites, int batch, int h, int w, void* workspace, size_t workspace_bytes, void* stream,
                     smi_engine** out);
int smi_mmdit_forward(smi_engine* e, int n, const float* sample, const float* timesteps, const void* ctx, const void* pooled,
                      const float* lora_down_flat, const float* lora_up_flat, const float* multipliers, float* out);

/* ---- SD3 MMDiT with LoRA sites, differentiated to the LoRA parameters (training an SD3 slider: train_lora_sd3) ---------
 * A trainable engine also keeps transposed copies of every Linear on the gradient path of both streams (the fused q|k|v,
 * to_out.0 / to_add_out, ff.net.0.proj, ff.net.2, proj_out; the modulation Linears, the embedders and norm_out.linear get
 * none) and a second arena for ONE saved pass and its backward: workspace = [packed weights | arena 0 (no-grad passes) |
 * arena 1], sized by a dry forward + backward; n_sites 0 is refused by name.
 *   smi_mmdit_forward       runs on a trainable engine too and leaves a saved pass intact
 *   smi_mmdit_forward_save  the arguments of smi_mmdit_forward and the same bits in out; the pass is kept for ONE backward
 *   smi_mmdit_backward      d_out f32 [n, out_channels, h, w] (device): the gradient of `out`.  The gradients of the LoRA
 *                           parameters are ADDED to d_lora_down_flat / d_lora_up_flat (f32, the layout of the flat parameter
 *                           buffers).  One power-of-two loss scale per sample keeps the 16-bit gradients in range.  Nothing
 *                           else is differentiated: not the latents, the context, the pooled embedding or temb (scale, shift
 *                           and gate depend on temb alone and no site sits upstream of them).  The backward consumes the
 *                           saved pass: without one it returns -4.  A pass saved with all multipliers 0 or NULL flat
 *                           buffers, or NULL gradient buffers here: returns 0 and adds nothing. */
int smi_mmdit_train_workspace_bytes(const smi_mmdit_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int h,
                                    int w, size_t* bytes);
int smi_mmdit_train_create(const smi_mmdit_config* cfg, const smi_weight* weights, int n_weights, const smi_lora_site* sites,
                           int n_sites, int batch, int h, int w, void* workspace, size_t workspace_bytes, void* stream,
                           smi_engine** out);
int smi_mmdit_forward_save(smi_engine* e, int n, const float* sample, const float* timesteps, const void* ctx,
                           const void* pooled, const float* lora_down_flat, const float* lora_up_flat,
                           const float* multipliers, float* out);
int smi_mmdit_backward(smi_engine* e, const float* d_out, float* d_lora_down_flat, float* d_lora_up_flat);

/* ---- Flux transformer, forward with LoRA sites (sweeping a Flux slider) ------------------------------------------------
 * Replaces `transformer(hidden_states, timestep, guidance, pooled_projections, encoder_hidden_states, txt_ids, img_ids).sample`
 * (conceptmod/textsliders/train_util.py predict_noise_flux) on UN-packed latents: the engine packs ([n, C, h, w] ->
 * [n, (h/2)(w/2), 4 C], columns (c, py, px)) and un-packs itself, and builds the rotary table from (h, w, context_len) at
 * creation, on the host in float64 (image ids (0, row, col), text ids 0; interleaved pairs).  x = x_embedder(pack),
 * c = context_embedder(ctx), temb = timestep MLP(sinusoid256(t)) [+ guidance MLP(sinusoid256(1000 g))] + pooled-text MLP.
 * num_layers double blocks: the SD3 joint block with q and k RMS-normalised per head (attn.norm_q / norm_k, and
 * norm_added_q / norm_added_k on the context stream) and rotated, over the joint sequence CONTEXT rows first.
 * num_single_layers single blocks on that joint sequence: z = LN(s) (1 + scale) + shift, attention(rope(rms(q)), rope(rms(k)), v)
 * and gelu_tanh(proj_mlp z) side by side into one [rows, 5 d] operand of proj_out, s += gate proj_out([a | m]).  The image
 * rows (the last of each sample) go through norm_out (scale, shift) + proj_out.
 *   weights      the diffusers state_dict (`x_embedder.*`, `context_embedder.*`, `time_text_embed.*`,
 *                `transformer_blocks.<i>.*`, `single_transformer_blocks.<i>.*`, `norm_out.linear.*`, `proj_out.*`), dtype T
 *   sites        Linear LoRA sites (rank <= 16) on attn.to_q/to_k/to_v of double and single blocks (all three of a block or
 *                none, adjacent in the flat buffers in that order: one fused GEMM), attn.add_q_proj/add_k_proj/add_v_proj
 *                (likewise), attn.to_out.0 and attn.to_add_out; n_sites 0: a frozen network.  DoRA sites and other targets
 *                (proj_mlp, proj_out, ff.*) are refused by name.
 *   h, w         the LATENT size, even; fixed at creation, as context_len is
 *   sample       f32 [n, in_channels, h, w]
 *   timesteps    f32 [n], HOST memory: the scheduler's 1000 sigma, one per sample
 *   guidance     f32 [n], HOST memory, for a guidance_embeds model; NULL for one without (either mismatch is refused)
 *   ctx          T [n, context_len, joint_attention_dim]
 *   pooled       T [n, pooled_projection_dim]
 *   multipliers  f32 [n], HOST memory, as smi_mmdit_forward takes them: NULL flat buffers, NULL multipliers or all
 *                multipliers 0 give the bits of an engine created without sites.
 *   out          f32 [n, in_channels, h, w]
 * workspace = [packed weights | persistent tensors | two block scratch regions], sized by a dry forward.  n may be smaller
 * than the creation batch.  No split-K scratch is lent to the GEMMs: a sample gives the same bits alone or in a batch.  The
 * config check refuses, by name: sum(axes_dims_rope) != attention_head_dim or an odd axis width, attention_head_dim not a
 * multiple of 16 or above 160, d % 64, d > 3072 (the adaLN rows), patch_size != 2 (the pack is 2 x 2),
 * in_channels x patch_size^2 % 64, h or w odd. */
int smi_flux_workspace_bytes(const smi_flux_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int h, int w,
                             size_t* bytes);
int smi_flux_create(const smi_flux_config* cfg, const smi_weight* weights, int n_weights, const smi_lora_site* sites,
                    int n_sites, int batch, int h, int w, void* workspace, size_t workspace_bytes, void* stream,
                    smi_engine** out);
int smi_flux_forward(smi_engine* e, int n, const float* sample, const float* timesteps, const float* guidance,
                     const void* ctx, const void* pooled, const float* lora_down_flat, const float* lora_up_flat,
                     const float* multipliers, float* out);

/* ---- Flux transformer differentiated to the LoRA parameters (training a Flux slider: train_lora_flux) -------------------
 * The five entries of the trainable MMDiT, for Flux.  A trainable engine also keeps transposed copies of every Linear on the
 * gradient path (the fused q|k|v of both streams and of the single blocks, to_out.0 / to_add_out, ff / ff_context, proj_mlp,
 * the single blocks' proj_out and the final proj_out; the modulation Linears, the embedders and norm_out.linear get none)
 * and a second arena for ONE saved pass and its backward, sized by a dry saved forward + backward; n_sites 0 is refused.
 *   smi_flux_forward        runs on a trainable engine too and leaves a saved pass intact
 *   smi_flux_forward_save   the arguments of smi_flux_forward and the same bits in out; the pass is kept for ONE backward.
 *                           In a saved pass a single block's q|k|v is normalised and rotated out of place and proj_mlp's
 *                           pre-activation is kept in a tensor of its own: the backward reads both
 *   smi_flux_backward       d_out f32 [n, in_channels, h, w] (device).  The gradients of the LoRA parameters are ADDED to
 *                           d_lora_down_flat / d_lora_up_flat; one power-of-two loss scale per sample.  Nothing else is
 *                           differentiated: not the latents, the context, the pooled vector, the guidance, temb or the
 *                           RMSNorm weights.  Consumes the saved pass: without one it returns -4.  A pass saved with the
 *                           adaptor off, or NULL gradient buffers here: returns 0, adds nothing and drops the pass. */
int smi_flux_train_workspace_bytes(const smi_flux_config* cfg, const smi_lora_site* sites, int n_sites, int batch, int h, int w,
                                   size_t* bytes);
int smi_flux_train_create(const smi_flux_config* cfg, const smi_weight* weights, int n_weights, const smi_lora_site* sites,
                          int n_sites, int batch, int h, int w, void* workspace, size_t workspace_bytes, void* stream,
                          smi_engine** out);
int smi_flux_forward_save(smi_engine* e, int n, const float* sample, const float* timesteps, const float* guidance,
                          const void* ctx, const void* pooled, const float* lora_down_flat, const float* lora_up_flat,
                          const float* multipliers, float* out);
int smi_flux_backward(smi_engine* e, const float* d_out, float* d_lora_down_flat, float* d_lora_up_flat);

/* eps = unet(sample, t, ctx[, text_embeds, time_ids]).sample          (train_util.py:290-294, 471-476)
 *   sample      f32 [n, 4, h, w]  (NCHW, already scale_model_input-ed)
 *   ctx         T   [n, ctx_len, cross_attention_dim]
 *   text_embeds T   [n, P] or NULL ; time_ids f32 [n, 6] or NULL        (SD-XL added_cond_kwargs)
 *   lora_down_flat / lora_up_flat: flat fp32 LoRA parameters, NULL or multiplier == 0 -> adaptor off
 *                 (LoRANetwork.__exit__, lora.py:299-301); multiplier = 1.0 * lora_scale inside `with network`.
 *   save_for_backward != 0 keeps the activations the backward needs (the pass that runs with grad enabled).
 *   eps_out     f32 [n, 4, h, w]
 * n may be smaller than the creation batch. */
int smi_unet_forward(smi_engine* e, int n, const float* sample, float timestep, const void* ctx,
                     const void* text_embeds, const float* time_ids, const float* lora_down_flat,
                     const float* lora_up_flat, float multiplier, int save_for_backward, float* eps_out);

/* The four guidance passes of one slider step as ONE UNet pass: samples are independent through the network, so the
 * positive / neutral / negative batches (adaptor off) and the target batch (adaptor on) are stacked into a batch of
 * n = 4 x 2B with the `n_adapted` = 2B target samples LAST.  Only those samples receive the LoRA delta and only their
 * activations are differentiated by smi_unet_backward (whose d_eps then has n_adapted samples).  Same arithmetic per
 * sample as four smi_unet_forward calls; 4x larger GEMM M, ~60 % fewer launches.  n_adapted == n gives
 * smi_unet_forward. */
int smi_unet_forward_batched(smi_engine* e, int n, int n_adapted, const float* sample, float timestep, const void* ctx,
                             const void* text_embeds, const float* time_ids, const float* lora_down_flat,
                             const float* lora_up_flat, float multiplier, int save_for_backward, float* eps_out);

/* smi_unet_forward_batched with ONE ADAPTOR MULTIPLIER PER ADAPTED SAMPLE (`multipliers`: host array of n_adapted
 * floats): the image-slider step runs the adaptor at +s on the `high` image and at -s on the `low` one
 * (trainscripts/imagesliders/train_lora-scale-xl.py:317-381) -- with per-sample multipliers both sides share one UNet
 * pass and one backward.  Implemented for Linear LoRA sites (attention projections, time_emb_proj, conv_shortcut); with
 * conv (c3lier) or DoRA sites and unequal multipliers it returns an error (run the samples in separate passes).  Equal
 * multipliers are exactly smi_unet_forward_batched. */
int smi_unet_forward_multi(smi_engine* e, int n, int n_adapted, const float* sample, float timestep, const void* ctx,
                           const void* text_embeds, const float* time_ids, const float* lora_down_flat,
                           const float* lora_up_flat, const float* multipliers, int save_for_backward, float* eps_out);

/* SLIDER COMPOSITION: several sliders in one pass, one scale per (adapted sample, slider).  The engine's adaptor is the
 * sliders STACKED along the rank axis (smi_lora_stack): every Linear site has rank sum(ranks) and site scale 1, alpha_k / r_k
 * is folded into lora_up, and slider k owns ranks[k] consecutive rank columns, so that
 *     y_i = W x_i + sum_k multipliers[i][k] * (alpha_k / r_k) * up_k(down_k(x_i))
 * is the rank-sum(ranks) delta with the columns of xa = x down^T multiplied per sample.  `ranks`: host int[n_sliders];
 * `multipliers`: host float[n_adapted][n_sliders].  Inference only: nothing is saved, and a smi_unet_backward after it fails
 * as after any pass that saved nothing.  Errors: sum(ranks) differs from the rank of a Linear site; n_adapted outside
 * 1..1024; n_sliders outside 1..16, sum(ranks) > 64 or n_adapted * sum(ranks) > 3072 (the table); any conv (c3lier) or DoRA
 * site (the engine does not scale a conv xa per sample, the restriction of smi_unet_forward_multi: such a caller folds the
 * scales into lora_up and runs plain passes).  It also drops a pass saved earlier. */
int smi_unet_forward_compose(smi_engine* e, int n, int n_adapted, const float* sample, float timestep, const void* ctx,
                             const void* text_embeds, const float* time_ids, const float* lora_down_flat,
                             const float* lora_up_flat, int n_sliders, const int* ranks, const float* multipliers,
                             float* eps_out);

/* One (site, slider) block of the stacked flat buffers: dst_down[c0 + q][0..row_len) = src_down[q][.] (rows of `in` floats
 * for a Linear site, Cin * kh * kw for a conv site) and dst_up[n][c0 + q] = coef * src_up[n][q] for n < n_out (one fp32
 * multiply); dst_down / dst_up are the SITE's stacked matrices [R][row_len] / [n_out][R].  src_down == src_up == NULL: the
 * slider does not adapt the site and its block is written as zeros. */
typedef struct smi_lora_stack_job {
  const float* src_down;
  const float* src_up;
  float* dst_down;
  float* dst_up;
  int64_t row_len;
  int r, c0, R, n_out;
  float coef;
  int reserved;
} smi_lora_stack_job;
/* All jobs in one launch.  jobs_dev: device memory for the table, n_jobs * sizeof(smi_lora_stack_job) bytes.
 * Synchronises. */
int smi_lora_stack(const smi_lora_stack_job* jobs, int n_jobs, void* jobs_dev, void* stream);

/* Backward of the last save_for_backward forward: accumulates (+=) d(loss)/d(lora_down), d(loss)/d(lora_up) into
 * the flat fp32 gradient buffers (same offsets as the parameters).  Activation gradients are propagated only as far
 * as the first adapted layer; no frozen-weight gradients exist (unet.requires_grad_(False), train_lora.py:69).
 * Replaces loss.backward() through the UNet (train_lora.py:298). */
int smi_unet_backward(smi_engine* e, const float* d_eps, float* d_lora_down_flat, float* d_lora_up_flat);

/* smi_unet_backward over the LAST `n_live` adapted samples of the saved pass only: `d_eps_live` is
 * [n_live, out_channels, h, w] and THE CALLER PROMISES that the gradient with respect to the output of the other adapted
 * samples is exactly zero.  A zero output gradient stays zero through every backward op and adds exact zeros to every
 * weight-gradient sum, so those samples' rows are not run at all: every backward launch works on n_live instead of
 * n_adapted samples.  The case it is for: the CFG-doubled adapted batch [unconditional x B ; target x B] at guidance
 * scale 1, where d(u + 1 (t - u)) has no u term (n_live = B).  The forward is untouched.
 * 1 <= n_live <= n_adapted of the saved pass, anything else is an error; n_live == n_adapted is smi_unet_backward (same
 * launches, same bits).  With the kernel selection pinned the result equals, bit for bit, smi_unet_backward on
 * [zeros ; d_eps_live] for LoRA / c3lier sites; at default selection the smaller row count can select other GEMM /
 * attention kernels (equal to rounding).  DoRA: the common loss scale is the minimum over the live samples only. */
int smi_unet_backward_tail(smi_engine* e, int n_live, const float* d_eps_live, float* d_lora_down_flat,
                           float* d_lora_up_flat);

/* ---- gradient with respect to the context (null-text inversion optimises the unconditional embedding) -----------------
 * Replaces `loss.backward()` reaching `uncond_embeddings` through `unet(latent, t, encoder_hidden_states=uncond_embeddings)`
 * (demo_image_editing.ipynb, NullInversion.null_optimization).
 * The backward then needs transposed copies of every cross-attention to_k|to_v weight and a larger saved-pass arena
 * (gradients exist from the first cross-attention block on, not from the first adapted layer).  Both live in ONE extra
 * caller-owned buffer, so an engine that never asks keeps the sizes smi_weights_bytes / smi_arena_bytes report today:
 *   smi_unet_ctx_grad_bytes   bytes of that buffer for a shape (same arguments as smi_arena_bytes)
 *   smi_unet_ctx_grad_attach  packs the transposed weights into `buffer` and moves the saved-pass arena there, for the
 *                             engine's CURRENT shape.  It drops a saved forward.  The buffer must outlive its use;
 *                             smi_replan detaches it (attach again, with a buffer sized for the new shape).
 *   smi_unet_ctx_grad         on != 0: every following save_for_backward forward also differentiates the context of its
 *                             adapted samples; 0 (the state of a new engine): forwards are exactly what they were.
 *                             Turning it on without an attached buffer is an error.
 *   smi_unet_backward_ctx     smi_unet_backward of such a pass that also WRITES (not +=) d(loss)/d(ctx) of the adapted
 *                             samples to d_ctx_out, fp32 [n_adapted, ctx_len, cross_attention_dim], with the per-sample
 *                             loss scale already divided out.  d_lora_down_flat / d_lora_up_flat may both be NULL when
 *                             the saved pass ran without an adaptor (n_sites == 0, NULL parameters or multiplier 0).
 * Without LoRA on to_k / to_v every block writes dK|dV into its columns of one gradient of the grouped k|v projection and
 * d_ctx is one split-K GEMM against the transposed grouped weight; with it, each block's term is a GEMM of its own and the
 * terms are summed in fp32.  DoRA on to_k / to_v is refused.  smi_unet_backward on such a pass still works (no d_ctx);
 * smi_unet_backward_tail refuses it: `n_live` does not extend to d_ctx. */
int smi_unet_ctx_grad_bytes(const smi_unet_config* cfg, const smi_lora_site* sites, int n_sites, int batch,
                            int batch_adapted, int h, int w, int ctx_len, size_t* bytes);
int smi_unet_ctx_grad_attach(smi_engine* e, void* buffer, size_t buffer_bytes);
int smi_unet_ctx_grad(smi_engine* e, int on);
int smi_unet_backward_ctx(smi_engine* e, const float* d_eps, float* d_lora_down_flat, float* d_lora_up_flat,
                          float* d_ctx_out);

/* ---- gradient with respect to the pooled embedding (SD-XL null-text inversion optimises both unconditional parts) ------
 * SD-XL's conditioning has a second part, added_cond_kwargs["text_embeds"] [n, P], P = projection_class_embeddings_input_dim
 * - 6 addition_time_embed_dim, which reaches every resnet through the time embedding:
 *   text_embeds -> cat[:, :P] -> add_embedding.linear_1 -> SiLU -> linear_2 -> (+ time embedding) -> SiLU -> every resnet's
 *   time_emb_proj -> added to every pixel of conv1's output.
 * Its gradient rides on a pass that differentiates the context (above) and needs a transposed copy of the grouped
 * time_emb_proj weight plus a saved-pass arena that is larger again (gradients now exist from the first resnet on).  Both
 * live in ONE MORE caller-owned buffer; smi_weights_bytes / smi_arena_bytes / smi_workspace_bytes / smi_unet_ctx_grad_bytes
 * report what they reported without it:
 *   smi_unet_pooled_grad_bytes   bytes of that buffer for a shape (same arguments as smi_arena_bytes); a dry run
 *   smi_unet_pooled_grad_attach  packs the transposed weight into `buffer` and moves the saved-pass arena there, for the
 *                                engine's CURRENT shape (the copy folds the per-level gradient scale, which depends on the
 *                                map sizes).  Needs the context-gradient buffer attached; drops a saved forward;
 *                                smi_replan and smi_unet_ctx_grad_attach detach it.
 *   smi_unet_pooled_grad         on != 0: every following save_for_backward forward that differentiates the context also
 *                                differentiates text_embeds of its adapted samples.  Requires smi_unet_ctx_grad(e, 1) and an
 *                                attached buffer; an error on an engine without addition_embed and with an adaptor on a
 *                                time_emb_proj (c3lier; the error names the site).  smi_unet_ctx_grad(e, 0) turns it off too.
 *                                The forward's eps has the bits it has without the switch.
 *   smi_unet_backward_cond       smi_unet_backward_ctx of such a pass that also WRITES (not +=) d(loss)/d(text_embeds) of
 *                                the adapted samples to d_text_embeds_out, fp32 [n_adapted, P], each sample's loss scale
 *                                divided out, zero when no term arrived; nothing is written for frozen samples in front.
 *                                time_ids gets no gradient.
 * smi_unet_backward / smi_unet_backward_ctx on such a pass still work (without the new output); smi_unet_backward_tail
 * refuses it. */
int smi_unet_pooled_grad_bytes(const smi_unet_config* cfg, const smi_lora_site* sites, int n_sites, int batch,
                               int batch_adapted, int h, int w, int ctx_len, size_t* bytes);
int smi_unet_pooled_grad_attach(smi_engine* e, void* buffer, size_t buffer_bytes);
int smi_unet_pooled_grad(smi_engine* e, int on);
int smi_unet_backward_cond(smi_engine* e, const float* d_eps, float* d_lora_down_flat, float* d_lora_up_flat,
                           float* d_ctx_out, float* d_text_embeds_out);

/* Per-kernel-class timing, measured with HIP events recorded on the engine's stream around every launch
 * (measurement aid for bench.py's roofline; off by default, adds two event records per launch when on).
 * smi_profile_read synchronises with the host and returns, per class, the summed device time (ms), the algorithmic
 * FLOPs (2*M*N*K per GEMM/conv; 4*B*H*Nq*Nk*D per attention forward, 10*... per attention backward), the
 * algorithmic HBM bytes (operands read once + result written once) and the launch count since the last enable. */
#define SMI_PROF_GEMM 0  /* gemm_nt_kernel, dense operand (all Linear layers, 1x1 convs)  */
#define SMI_PROF_CONV 1  /* gemm_nt_kernel, implicit-GEMM 3x3 conv (+ the small-channel direct conv) */
#define SMI_PROF_ATTN 2  /* attention forward / backward kernels */
#define SMI_PROF_NORM 3  /* GroupNorm / LayerNorm */
#define SMI_PROF_ELEM 4  /* GEGLU, SiLU, add, concat/split copies, pooling */
#define SMI_PROF_LORA 5  /* LoRA down-projection and weight-gradient reductions */
#define SMI_PROF_NCAT 6
int smi_profile_enable(smi_engine* e, int enable);
int smi_profile_read(smi_engine* e, double* ms, double* flops, double* bytes, int64_t* launches);

/* out[i] = u[i] + g * (t[i] - u[i]) over the two halves of a CFG-doubled prediction   (train_util.py:297-300) */
int smi_cfg_combine(const float* eps_2n, float* out_n, int64_t n_half, float guidance_scale, void* stream);

/* PromptEmbedsPair.loss (prompt_util.py:134-174): loss = mean((target - (neutral + sign_eta*(positive-negative)))^2)
 * sign_eta = +eta for "enhance", -eta for "erase".  Writes the scalar to loss_out[0] and, if dtarget != NULL,
 * d(loss)/d(target).  scratch: >= 256 floats. */
int smi_slider_loss(const float* target, const float* positive, const float* neutral, const float* negative,
                    float sign_eta, int64_t n, float* loss_out, float* dtarget, float* scratch, void* stream);

/* One inner step of null-text optimisation after the UNet call (demo_image_editing.ipynb, null_optimization):
 *   eps = eps_u + g (eps_c - eps_u);  x_prev = c_x x_t + c_eps eps  (DDIM prev_step, coefficients from the host as for
 *   smi_sched_step);  loss_out[0] = mean((x_prev - target)^2);  d_eps_u = (1 - g) c_eps (2 / n) (x_prev - target).
 * All tensors fp32 of n elements; d_eps_u may be NULL.  The sum runs in a fixed order (bit-reproducible run to run).
 * scratch: >= 256 floats. */
int smi_nulltext_loss(const float* eps_u, const float* eps_c, const float* x_t, const float* target, float guidance_scale,
                      float c_x, float c_eps, int64_t n, float* loss_out, float* d_eps_u, float* scratch, void* stream);

/* torch.nn.utils.clip_grad_norm_(params, max_norm) (train_lora_xl.py:349; max_norm <= 0: no clipping) followed by
 * one torch.optim.AdamW step (train_lora_xl.py:104,350; train_util.py:1040) over flat fp32 buffers.
 * step counts from 1.  scratch: >= 1025 floats. */
int smi_clip_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, float max_norm, float* scratch,
                   void* stream);

/* clip_grad_norm_(max_norm) (max_norm <= 0: no clipping) followed by one Lion step (the reference's `lion` optimiser,
 * train_util.py:1027-1032: lion_pytorch.Lion) over flat fp32 buffers; exp_avg starts at zero:
 *   p <- p (1 - lr weight_decay);  c = beta1 exp_avg + (1 - beta1) g;  p <- p - lr sign(c)   (sign(0) = 0, as torch.sign)
 *   exp_avg <- beta2 exp_avg + (1 - beta2) g
 * One grid-stride kernel after the optional norm reduction.  The hyper-parameters are doubles (the package's Python
 * floats): 1 - beta and 1 - lr weight_decay are formed in double and rounded to fp32 once, as torch rounds a Python scalar.
 * scratch: >= 1025 floats (only read when clipping). */
int smi_clip_lion(float* param, const float* grad, float* exp_avg, int64_t n, double lr, double beta1, double beta2,
                  double weight_decay, float max_norm, float* scratch, void* stream);

/* Prodigy (the reference's `prodigy` optimiser, train_util.py:1033-1038: prodigyopt.Prodigy) over flat fp32 buffers.
 * Hyper-parameters as doubles (the package's Python floats); beta3 is passed resolved (sqrt(beta2) for the default). */
typedef struct smi_prodigy_hyper {
  double lr, beta1, beta2, beta3, eps, weight_decay, d0, d_coef, growth_rate; /* growth_rate: INFINITY for none */
  int decouple, use_bias_correction, safeguard_warmup;
} smi_prodigy_hyper;
/* The state of a fresh Prodigy group: p0 = param (a copy), exp_avg = exp_avg_sq = s = 0 (n floats each), and `state`, 8
 * device doubles: [0] d = d0, [1] d_max = d0, [2] d_numerator = 0, [3] k = 0, and what a step's finalize leaves for its
 * apply: [4] dlr (old), [5] d (new), [6] skip flag, [7] reserved. */
int smi_prodigy_init(const float* param, float* p0, float* exp_avg, float* exp_avg_sq, float* s, int64_t n, double d0,
                     double* state, void* stream);
/* clip_grad_norm_(max_norm) (max_norm <= 0: none), then one Prodigy step.  d, d_max, d_numerator, k and the two sums are
 * doubles on the device; the host reads none of them:
 *   bc = use_bias_correction ? sqrt(1 - beta2^(k+1)) / (1 - beta1^(k+1)) : 1;   dlr = d lr bc
 *   d_numerator <- beta3 d_numerator;   if weight_decay != 0 and not decouple: g <- g + weight_decay p
 *   if lr > 0: d_numerator += (d / d0) dlr sum(g (p0 - p))
 *   exp_avg <- beta1 exp_avg + d (1 - beta1) g;   exp_avg_sq <- beta2 exp_avg_sq + d^2 (1 - beta2) g^2
 *   s <- beta3 s + (d / d0) (safeguard_warmup ? d : dlr) g;   d_denom = sum |s|
 *   if d_denom == 0: stop here (p, d, d_max and k keep their values)
 *   if lr > 0: d_hat = d_coef d_numerator / d_denom;  if d == d0: d <- max(d, d_hat);  d_max <- max(d_max, d_hat);
 *              d <- min(d_max, d growth_rate)
 *   if weight_decay != 0 and decouple: p <- p - weight_decay dlr p          (the OLD dlr)
 *   p <- p - dlr exp_avg / (sqrt(exp_avg_sq) + d eps)                        (the OLD dlr, the NEW d);   k <- k + 1
 * Three launches ordered by the stream (accumulate with one partial per workgroup of each sum; finalize, one wave, the
 * partials added in double, each lane its run of consecutive partials in index order and the lane sums in lane order;
 * apply): no atomics, no grid barrier, a fixed summation order, so two runs and two ranks give the same bits.
 * scratch: >= 3073 floats. */
int smi_clip_prodigy(float* param, const float* grad, const float* p0, float* exp_avg, float* exp_avg_sq, float* s,
                     int64_t n, const smi_prodigy_hyper* hyper, float max_norm, double* state, float* scratch,
                     void* stream);

/* x = c_x * x + c_eps * eps + c_noise * noise   -- the update of scheduler.step(...).prev_sample
 * (train_util.py:324,705) for DDIM (eta = 0; noise = NULL) and Euler-ancestral; coefficients computed on the host. */
int smi_sched_step(float* x, const float* eps, const float* noise, float c_x, float c_eps, float c_noise, int64_t n,
                   void* stream);

/* ---- single-kernel entry points (used by the parity tests; same launchers the engine uses) ---------------- */
/* Lends `bytes` of device memory at `ws` to the GEMM / conv launchers of THIS host thread as split-K scratch (fp32 partial
 * slabs) until called again with NULL: with it, smi_op_gemm / smi_op_conv3x3 take the same split-K rule the engine's
 * launches take (the engine lends a region of its own workspace per call); without it they never split. */
int smi_op_gemm_scratch(void* ws, size_t bytes);
int smi_op_gemm(int dtype, const void* A, const void* W, void* C, int M, int N, int K, const void* bias,
                const void* res, const float* lora_xa, const float* lora_up, int lora_r, float lora_scale,
                int out_f32, void* stream);
/* The batched-pass form of the adapted Linear (T/lora.py:134-138 under T/train_util.py:449-489's batched UNet call):
 * rows m >= lora_row0 get + lora_scale * xa[m - lora_row0] up^T, rows below none (the frozen samples of the pass).
 * lora_seg > 0: fused projections (q|k|v) -- column block n / lora_seg has its own [lora_seg, r] up matrix (adjacent in
 * lora_up) and its own r columns of xa (row stride r * N / lora_seg). */
int smi_op_gemm_rows(int dtype, const void* A, const void* W, void* C, int M, int N, int K, const void* bias,
                     const void* res, const float* lora_xa, const float* lora_up, int lora_r, float lora_scale,
                     int lora_row0, int lora_seg, void* stream);
/* Every epilogue term of a dense GEMM on a NAMED tile (tests/test_gemm_epilogue_gpu.py): C [M, N] (T, or fp32 with
 * out_f32) = A [M, K] W [N, K]^T + bias [N] + rowvec [M / rows_per_vec, ld_rowvec] + lora_scale * delta + res [M, N]; any
 * of bias / res / rowvec / lora_xa may be NULL.  Delta, forward form (lora_dx = 0): xa [M - lora_row0, ld_xa] fp32 against
 * up [N, r], fused column blocks of lora_seg (0: none); dX form (lora_dx != 0): xa [M, ld_xa] against lora_up = down
 * [lora_r, N] read transposed.  tile_code: a tile's tuner code (csrc/gemm.hip kTileNames; 0 = launch_gemm's own choice);
 * ksplit > 1 forces split-K in that many slices with the tile as the slice kernel (needs smi_op_gemm_scratch).
 * *ran_code receives the code of the tile that ran: where the named tile cannot take the launch it is the stand-in's. */
int smi_op_gemm_epilogue(int dtype, const void* A, const void* W, void* C, int M, int N, int K, int out_f32,
                         const void* bias, const void* res, const void* rowvec, int rows_per_vec, int ld_rowvec,
                         const float* lora_xa, int ld_xa, const float* lora_up, int lora_r, int lora_seg, int lora_row0,
                         float lora_scale, int lora_dx, int tile_code, int ksplit, int* ran_code, void* stream);
/* A 3x3 implicit-GEMM conv of any gather mode on a NAMED tile (tests/test_conv_gather_gpu.py): the arguments of
 * smi_op_conv3x3, plus pad (1, or 0 for the (0, 1, 0, 1)-padded stride-2 down-sampler on an even map), the fp32 output
 * form, res [nb hout wout, cout], rowvec [nb hout wout / rows_per_vec, ld_rowvec] (the engine's per-sample vector has
 * rows_per_vec = hout wout) and the forward delta: xa [nb hout wout - lora_row0, ld_xa] fp32 against up [cout, lora_r].
 * Any of bias / res / rowvec / lora_xa may be NULL.  tile_code, ksplit and *ran_code as in smi_op_gemm_epilogue.  The
 * output grid must be the one the input grid and the mode give (transposed: `in` is dy on the forward's output grid,
 * `out` is dx on its input grid); the conv geometry checks of the ordinary launch hold for a named tile too. */
int smi_op_conv3x3_ex(int dtype, const void* in, const void* w_packed, const void* bias, void* out, int nb, int hin, int win,
                      int cin, int cout, int stride, int upsample, int transposed, int hout, int wout, int pad, int out_f32,
                      const void* res, const void* rowvec, int rows_per_vec, int ld_rowvec, const float* lora_xa, int ld_xa,
                      const float* lora_up, int lora_r, int lora_row0, float lora_scale, int tile_code, int ksplit,
                      int* ran_code, void* stream);
int smi_op_conv3x3(int dtype, const void* in, const void* w_packed, const void* bias, void* out, int nb, int hin,
                   int win, int cin, int cout, int stride, int upsample, int transposed, int hout, int wout,
                   void* stream);
/* The UNets' up-sampler conv (nearest-2x, then 3x3 / pad 1) in the engine's phase form:
 * out [nb, 2h, 2w, cout] from in [nb, h, w, cin], the torch filter w [cout, cin, 3, 3] and bias [cout] (may be NULL).
 * Packs the four summed 2x2 filters into wph (16 * cout * cin elements), runs the four phase convs into planes
 * (4 * nb * h * w * cout elements) on the tile with tuner code tile_code (0: the launcher's own choice; a tile that cannot
 * take the launch is replaced as in smi_op_gemm_epilogue) and un-shuffles the planes into out with the concat's copy.
 * ran_code (may be NULL): int [4], the code of the tile each phase ran on. */
int smi_op_upconv_phase(int dtype, const void* in, const void* w, const void* bias, void* wph, void* planes, void* out, int nb,
                        int h, int w_, int cin, int cout, int tile_code, int* ran_code, void* stream);
/* Process-wide override of SMI_UPCONV_PHASE (parity tests): -1 = the environment (default on), 0 = every up-sampler conv
 * as one 3x3 conv on the 2x grid, 1 = as four 2x2 phase convs where the layer allows it (UNet up-samplers without an
 * adaptor) at EVERY map size; the default form takes only input maps of at least SMI_UPCONV_PHASE_MIN_PIXELS (1024) pixels
 * per sample.  Read when an engine is planned and created (the phase filters are packed then) and at every forward. */
int smi_set_upconv_phase(int on);
int smi_op_attention_fwd(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int b, int h,
                         int nq, int nk, int d, float scale, void* stream);
int smi_op_attention_bwd(int dtype, const void* q, const void* k, const void* v, const void* o, const float* lse,
                         const void* d_o, void* dq, void* dk, void* dv, float* delta, int b, int h, int nq, int nk,
                         int d, float scale, void* stream);
/* Attention with every operand at its own leading dimension (elements; the engine's layouts: q|k|v as column blocks of one
 * [b n, 3 h d] tensor, k|v inside a [b nk, 2 h d] tensor or inside a wider tensor of the caller's, gradients likewise),
 * the kernel selection pinned for the call, and a report of what ran.  Test entry of tests/test_attention_kernels_gpu.py.
 *   forward:  q, k, v, o, lse (lse may be NULL)
 *   backward: q, k, v, o, lse, d_o, delta (f32 [b, h, nq] workspace) and dq and / or dk + dv; dq NULL: dK / dV only (delta
 *             from its own kernel); dk and dv NULL: dQ only
 *   sel_xs / sel_fused: -1 = as SMI_ATTN_XS / SMI_ATTN_BWD_FUSED say (the default), 0 = off, 1 = on, for this call only:
 *             the single-pass kernels for nk <= 96, and the one-launch backward.  The shape rules still apply.
 * Operands 16-byte aligned, leading dimensions multiples of 8. */
typedef struct smi_attn_args {
  const void *q, *k, *v;
  void* o;
  float* lse;
  const void* d_o;
  void *dq, *dk, *dv;
  float* delta;
  void* stream;
  int64_t ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
  int dtype, b, h, nq, nk, d;
  float scale;
  int causal, sel_xs, sel_fused;
} smi_attn_args;
#define SMI_ATTN_FWD 1       /* tiled forward (online softmax over 64-key tiles) */
#define SMI_ATTN_XS_FWD 2    /* single-pass forward, nk <= 96 */
#define SMI_ATTN_BWD_FUSED 3 /* dQ and dK / dV workgroups in one launch */
#define SMI_ATTN_DQ 4        /* tiled dQ (publishes delta) */
#define SMI_ATTN_XS_DQ 5     /* single-pass dQ, nk <= 96 (publishes delta) */
#define SMI_ATTN_DKV 6       /* dK and dV in one kernel (tile depth <= 96) */
#define SMI_ATTN_DK_DV 7     /* dK and dV as two launches (tile depth 160) */
#define SMI_ATTN_DELTA 8     /* delta kernel of the dK / dV-only form */
typedef struct smi_attn_ran {
  int dp;         /* tile depth: 32, 64, 96 or 160 */
  int form;       /* k-steps over d: 1 = full depth at compile time, 2 = the alternative (40 in 64, 80 in 96), 0 = run-time */
  int n_launches; /* kernel families launched, in order, in family[0 .. n_launches) */
  int family[4];  /* SMI_ATTN_* */
  int chain;      /* single-pass kernels: 128-query blocks per workgroup; otherwise 0 */
} smi_attn_ran;
int smi_op_attention_ex_fwd(const smi_attn_args* args, smi_attn_ran* ran);
int smi_op_attention_ex_bwd(const smi_attn_args* args, smi_attn_ran* ran);
/* Causal self-attention (key j visible to query i iff j <= i; CLIP text towers) with explicit leading dimensions, so that
 * q | k | v may be column blocks of one fused [b n, 3 h d] tensor.  The backward is one workgroup per (sample, head):
 * nq == nk <= 128, head_dim 64, all of dq / dk / dv; anything else returns an error that names the limit.  `delta` is
 * unused and may be NULL.  Operands 16-byte aligned, leading dimensions multiples of 8. */
int smi_op_attention_causal_fwd(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int b, int h,
                                int n, int d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, float scale, void* stream);
int smi_op_attention_causal_bwd(int dtype, const void* q, const void* k, const void* v, const void* o, const float* lse,
                                const void* d_o, void* dq, void* dk, void* dv, float* delta, int b, int h, int nq, int nk,
                                int d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t lddo, int64_t lddq,
                                int64_t lddk, int64_t lddv, float scale, void* stream);
/* The T5 encoder's kernels (tests/test_t5_kernels_gpu.py).  T is f16 or bf16, arithmetic fp32, one rounding at the store.
 * attention_bias_fwd: self-attention (nq == nk == n, head_dim 64, no mask) with s[q, k] = q.k * scale + table[h][k - q + n - 1]
 *   and the softmax over the biased scores; table f32 [h, ld_table], ld_table >= 2 n - 1, n <= 2048; explicit leading
 *   dimensions as smi_op_attention_causal_fwd; always the tiled forward; lse (natural log of the biased row sums) may be NULL.
 * rmsnorm: y[i, :] = w * x[i, :] * rsqrt(mean(x[i, :]^2) + eps), c % 8 == 0, c <= 8192.
 * gated_gelu_tanh: out[i, j] = gelu_tanh(proj[i, j]) * proj[i, f + j] on proj T [m, 2 f], f % 8 == 0; the GELU of smi_op_act kind 2.
 * t5_bias_table: out f32 [h, 2 l - 1], out[a, o] = weight[bucket[o], a] from weight T [num_buckets, h] and the device array
 *   bucket int32 [2 l - 1] (smi_t5_relative_buckets computes it on the host). */
int smi_op_attention_bias_fwd(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, const float* table,
                              int64_t ld_table, int b, int h, int n, int d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                              float scale, void* stream);
int smi_op_rmsnorm(int dtype, const void* x, const void* w, void* y, int m, int c, float eps, void* stream);
int smi_op_gated_gelu_tanh(int dtype, const void* proj, void* out, int64_t m, int f, void* stream);
/* Their backward (tests/test_t5_bwd_kernels_gpu.py).  The table and the norm weight are frozen: no gradient to either.
 * attention_bias_bwd: smi_attn_args as smi_op_attention_ex_bwd reads them (nq == nk, d == 64, causal 0, lse the biased
 *   forward's; dq NULL: dK / dV only; dk and dv NULL: dQ only), the probabilities recomputed as
 *   exp(scale q.k + table[h][k - q + n - 1] - lse[q]).  Runs the tiled dQ and dK / dV kernels or, with every gradient wanted
 *   and sel_fused != 0 on a grid of at most 1024 query blocks, the one-launch form; never the single-pass kernels.
 * rmsnorm_bwd: dx[i, :] = r (w dy[i, :]) - x[i, :] r^3 mean(x[i, :] . w dy[i, :]) (+ add[i, :]; add may be NULL or dx itself),
 *   r = rsqrt(mean(x[i, :]^2) + eps); c % 8 == 0, c <= 8192.
 * gated_gelu_tanh_bwd: dproj T [m, 2 f] from proj T [m, 2 f] and dout T [m, f]: columns [0, f) dout * up * gelu_tanh'(gate)
 *   (the derivative of smi_op_act kind 2), columns [f, 2 f) dout * gelu_tanh(gate). */
int smi_op_attention_bias_bwd(const smi_attn_args* args, const float* table, int64_t ld_table, smi_attn_ran* ran);
int smi_op_rmsnorm_bwd(int dtype, const void* x, const void* dy, const void* w, const void* add, void* dx, int m, int c,
                       float eps, void* stream);
int smi_op_gated_gelu_tanh_bwd(int dtype, const void* proj, const void* dout, void* dproj, int64_t m, int f, void* stream);
int smi_op_t5_bias_table(int dtype, const void* weight, const int32_t* bucket, float* out, int h, int l, int num_buckets,
                         void* stream);
/* The MLP activations, kind 0 quick_gelu / 1 erf-gelu (CLIP) / 2 tanh-gelu (MMDiT): y = act(x) when y is given
 * (n % 8 == 0), dx = dy * act'(x) when dy is given (any n >= 1). */
int smi_op_act(int dtype, const void* x, void* y, const void* dy, void* dx, int64_t n, int kind, void* stream);
int smi_op_groupnorm(int dtype, const void* x, const void* gamma, const void* beta, void* y, const void* dy, void* dx,
                     float* scratch, int nb, int hw, int c, int g, float eps, int silu, void* stream);
int smi_op_layernorm(int dtype, const void* x, const void* gamma, const void* beta, void* y, const void* dy, void* dx,
                     float* mean_rstd, int m, int c, float eps, void* stream);
/* GroupNorm / LayerNorm as the engine launches them.  Test entries of tests/test_norm_kernels_gpu.py.
 *   smi_op_groupnorm_ex: forward on nb samples of x [nb, hw, c] (y NULL: the statistics-only launch of the VAE decoder's
 *     tail: a, b and mean_rstd, no y); when dy is given, the backward on samples [bwd_n0, nb) with the forward's a, b and
 *     mean_rstd at their offsets: dy, add and dx are [nb - bwd_n0, hw, c]; add is optional and may equal dx.
 *     scratch (f32) as smi_op_groupnorm: a [nb, c] | b [nb, c] | mean_rstd [nb, g, 2] | partials.
 *     sel_fused: -1 = as SMI_GN_FUSED_HW / SMI_GN_FUSED_MAX say (the default), 0 = never the one-launch forward, 1 = the
 *     one-launch forward wherever its shape rules hold (group width even and <= 256, slice within LDS), for this call.
 *   smi_op_layernorm_ex: nb = rows m, x [m, c], scratch = mean_rstd f32 [m, 2]; backward on rows [bwd_n0, m): dy, add and
 *     dx are [m - bwd_n0, c].  hw, g, silu and sel_fused are not read.
 * ran_fwd / ran_bwd (either may be NULL) receive what the forward / backward launched. */
typedef struct smi_norm_args {
  const void *x, *gamma, *beta;
  void* y;
  const void *dy, *add;
  void* dx;
  float* scratch;
  void* stream;
  int dtype, nb, hw, c, g;
  float eps;
  int silu, bwd_n0, sel_fused;
} smi_norm_args;
#define SMI_NORM_GN_ONE 1  /* GroupNorm forward in one launch (slice in LDS) */
#define SMI_NORM_GN_TWO 2  /* chunk partials + apply (or + statistics) */
#define SMI_NORM_GN_FOLD 3 /* chunk partials + fold to 64 slots + apply */
#define SMI_NORM_LN 4      /* LayerNorm kernel <nv, r> */
typedef struct smi_norm_ran {
  int form;          /* SMI_NORM_*; 0 after a refused call */
  int chunks, slots; /* GroupNorm two-launch forms: chunks per sample, partial slots the apply head merges */
  int nv, r;         /* LayerNorm: 8-element vectors per lane, rows per wave */
} smi_norm_ran;
int smi_op_groupnorm_ex(const smi_norm_args* args, smi_norm_ran* ran_fwd, smi_norm_ran* ran_bwd);
int smi_op_layernorm_ex(const smi_norm_args* args, smi_norm_ran* ran_fwd, smi_norm_ran* ran_bwd);
/* The small elementwise kernels, one launch each (tests/test_elementwise_kernels_gpu.py):
 *   pool2x2_sum  dx [nb, h, w, c] = sum of the 2 x 2 block of du [nb, 2h, 2w, c], c % 8 == 0
 *   colsum       out [nb, c] (T) = mul * sum over hw of x [nb, hw, c]; scratch f32, smi_op_colsum_floats of them
 *   timestep_embed  out [n, dim] = cos(t f_i) | sin(t f_i), f_i = 10000^(-i / (dim / 2))
 *   softmax_rows P [rows, cols] (T) = softmax(scale * S) of fp32 rows
 *   chan_mix     y [m, c] (f32) = b + x W^T on fp32 rows, c <= 16
 *   conv3x3_small  stride 1, pad 1: in [nb, h, w, cin], w [cout][9 cin] (tap-major), out [nb, h, w, cout] T or f32
 *   nchw_to_nhwc(_scaled)  NCHW (T or f32) -> [nb, hw, cpad] T, columns >= c zero, times scale (times scale_dev[n]) */
int smi_op_pool2x2_sum(int dtype, const void* du, void* dx, int nb, int h, int w, int c, void* stream);
int smi_op_colsum_floats(int nb, int c, size_t* out_floats);
int smi_op_colsum(int dtype, const void* x, void* out, float* scratch, int nb, int hw, int c, float mul, void* stream);
int smi_op_timestep_embed(int dtype, const float* vals, void* out, int n, int dim, void* stream);
int smi_op_softmax_rows(int dtype, const float* s, void* p, int rows, int cols, float scale, void* stream);
int smi_op_chan_mix(int dtype, const float* x, const void* w, const void* b, float* y, int64_t m, int c, void* stream);
int smi_op_conv3x3_small(int dtype, const void* in, const void* w, const void* bias, void* out, int out_f32, int nb, int h,
                         int wd, int cin, int cout, void* stream);
int smi_op_nchw_to_nhwc(int dtype, const void* src, int src_f32, void* dst, int nb, int c, int hw, int cpad, float scale,
                        void* stream);
int smi_op_nchw_to_nhwc_scaled(int dtype, const float* src, void* dst, int nb, int c, int hw, int cpad, const float* scale_dev,
                               void* stream);
/* The MMDiT kernels, one launch each (tests/test_mmdit_kernels_gpu.py).  T is the 16-bit type, arithmetic fp32, one rounding
 * at the store.  scale / shift / gate are c columns of row r / rows_per_sample of mod T [n, ldm], at column offsets that are
 * multiples of 8 (as ldm is).
 *   adaln_modulate  y [m, c] = LN(x) (1 + scale) + shift, LayerNorm without affine; c % 8 == 0, c <= 2048;
 *                   mean_rstd f32 [m, 2] (may be NULL)
 *   gate_residual   y [m, c] = h + gate f; y may alias h
 *   joint_rows_pack / _split  joint [n (nx + nc), w] = per sample the nx rows of a [n nx, w], then the nc rows of b [n nc, w];
 *                   the split is the inverse and a or b may be NULL there; w % 8 == 0
 *   sd3_patchify    out T [n (h/p) (w/p), cin p p], columns (c, py, px), from latents f32 [n, cin, h, w]; cin p p % 64 == 0
 *   sd3_add_pos     y [n gh gw, d] = x + the centre-cropped gh x gw window of pos T [s s, d] (top (s - gh) / 2, left (s - gw) / 2)
 *   sd3_unpatchify  out f32 [n, cout, gh p, gw p] from rows T [n gh gw, p p cout], columns (py, px, c)
 * and the backwards to the activations (tests/test_mmdit_bwd_kernels_gpu.py); scale, shift and gate take no gradient:
 *   adaln_modulate_bwd  dx [m, c] = rstd (g - mean_c(g) - xhat mean_c(g xhat)) (+ add), g = dy (1 + scale), c <= 3072,
 *                   xhat = (x - mean) rstd from the forward's mean_rstd; add [m, c] is optional and may alias dx
 *   gate_residual_bwd   df [m, c] = gate dy (the gradient of h is dy itself)
 * pack and split are each other's backward. */
int smi_op_adaln_modulate(int dtype, const void* x, const void* mod, void* y, float* mean_rstd, int m, int c,
                          int rows_per_sample, int64_t ldm, int off_scale, int off_shift, float eps, void* stream);
int smi_op_gate_residual(int dtype, const void* h, const void* f, const void* mod, void* y, int64_t m, int c,
                         int rows_per_sample, int64_t ldm, int off_gate, void* stream);
int smi_op_adaln_modulate_bwd(int dtype, const void* x, const void* dy, const void* mod, const float* mean_rstd, const void* add,
                              void* dx, int m, int c, int rows_per_sample, int64_t ldm, int off_scale, void* stream);
int smi_op_gate_residual_bwd(int dtype, const void* dy, const void* mod, void* df, int64_t m, int c, int rows_per_sample,
                             int64_t ldm, int off_gate, void* stream);
int smi_op_joint_rows_pack(int dtype, const void* a, const void* b, void* joint, int n, int nx, int nc, int w, void* stream);
int smi_op_joint_rows_split(int dtype, const void* joint, void* a, void* b, int n, int nx, int nc, int w, void* stream);
int smi_op_sd3_patchify(int dtype, const float* latents, void* out, int n, int cin, int h, int w, int p, void* stream);
int smi_op_sd3_add_pos(int dtype, const void* x, const void* pos, void* y, int n, int gh, int gw, int d, int s, void* stream);
int smi_op_sd3_unpatchify(int dtype, const void* rows, float* out, int n, int cout, int gh, int gw, int p, void* stream);
/* The Flux kernels, one launch each (tests/test_flux_kernels_gpu.py).
 * qk_norm_rope: one stream's q|k|v rows src T [n tokens, lds] into rows [row_off, row_off + tokens) of every sample of the
 * joint buffer dst T [n l, ldd]: q and k heads x rsqrt(mean(x^2) + eps) w (wq / wk T [d]) and rotated, interleaved pairs, by row
 * (row_off + t) of table f32 [l, d] = cos[d / 2] | sin[d / 2]; v copied.  d % 16 == 0, d <= 160.  src == dst: in place.
 * gelu_tanh_cols: y[m, 0..c) = gelu_tanh(x[m, 0..c)) with row strides ldx / ldy; y may alias x.
 * flux_unpack: out f32 [n, cout, gh p, gw p] from rows T [n gh gw, cout p p] with columns (c, py, px). */
int smi_op_qk_norm_rope(int dtype, const void* src, int64_t lds, void* dst, int64_t ldd, const void* wq, const void* wk,
                        const float* table, int n, int tokens, int l, int row_off, int heads, int d, float eps, void* stream);
int smi_op_gelu_tanh_cols(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int64_t m, int c, void* stream);
int smi_op_flux_unpack(int dtype, const void* rows, float* out, int n, int cout, int gh, int gw, int p, void* stream);
/* Their backwards to the activations (tests/test_flux_bwd_kernels_gpu.py); the RMSNorm weights take no gradient.
 * qk_norm_rope_bwd: dsrc T [n tokens, ldx] from rows [row_off, row_off + tokens) of every sample of the joint gradient dj T
 * [n l, ldd] and the pre-norm source src T [n tokens, lds]: per q or k head dy = Rot^T(do), g = dy w,
 * dx = r (g - x r^2 mean(g x)), r = rsqrt(mean(x^2) + eps) recomputed from x; v copied.  dsrc aliases neither input.
 * gelu_tanh_cols_bwd: dx[m, 0..c) = dy[m, 0..c) gelu_tanh'(x[m, 0..c)) with row strides ldx / ldy / ldd: the bits of
 * smi_op_act kind 2's backward.
 * flux_unpack_bwd: rows T [n gh gw, cout p p], columns (c, py, px), = scale_dev[n] d_out f32 [n, cout, gh p, gw p]. */
int smi_op_qk_norm_rope_bwd(int dtype, const void* dj, int64_t ldd, const void* src, int64_t lds, void* dsrc, int64_t ldx,
                            const void* wq, const void* wk, const float* table, int n, int tokens, int l, int row_off, int heads,
                            int d, float eps, void* stream);
int smi_op_gelu_tanh_cols_bwd(int dtype, const void* x, int64_t ldx, const void* dy, int64_t ldy, void* dx, int64_t ldd, int64_t m,
                              int c, void* stream);
int smi_op_flux_unpack_bwd(int dtype, const float* d_out, void* rows, int n, int cout, int gh, int gw, int p,
                           const float* scale_dev, void* stream);
int smi_op_geglu(int dtype, const void* proj, void* out, const void* dout, void* dproj, int m, int c4, void* stream);
/* ff.net.0 with the GEGLU gate fused into the GEMM epilogue (the engine's forward path for
 * diffusers GEGLU: proj = x W^T + b [M, N]; out[M, N/2] = proj[:, :N/2] * gelu(proj[:, N/2:])).  Rows >= proj_row0 of
 * proj are also written (row m at proj + m*N); pass proj_row0 = M to keep none.  Fails when the layout is not
 * supported by the fused kernel (N % 256 != 0, misaligned operands). */
int smi_op_gemm_geglu(int dtype, const void* A, const void* W, const void* bias, void* out, void* proj, int M, int N,
                      int K, int proj_row0, void* stream);
int smi_op_lora_down(int dtype, const void* x, const float* a, float* xa, int m, int k, int r, void* stream);
/* out[m, r] (fp32) = x[m, k] * s[r, k]^T on 16-bit operands, r = 16 or 32, k % 128 == 0: the engine's kernel for
 * xa = x * lora_down^T and dxa = dy * lora_up (T/lora.py:134-138 and its backward) on the 16-bit shadow parameters */
int smi_op_lora_skinny(int dtype, const void* x, const void* s, float* out, int m, int r, int k, void* stream);
/* smi_op_lora_skinny, then out[i][c] *= col_mul[(i / rows_per_mul) * ld_mul + c % period] (one fp32 multiply after the
 * fixed-order reduction): the column multipliers of a slider stack */
int smi_op_lora_skinny_cols(int dtype, const void* x, const void* s, float* out, int m, int r, int k, const float* col_mul,
                            int ld_mul, int period, int rows_per_mul, void* stream);
/* dw[r, k] += alpha * p[m, r]^T x[m, k]: the engine's grouped weight-gradient reduction (T/lora.py:134-138 backward)
 * run on a one-job table.  scratch: ceil(m / 64) * r * k + 256 floats (partials + the table). */
int smi_op_lora_wgrad(int dtype, const float* p, const void* x, float* dw, int m, int k, int r, float alpha,
                      float* scratch, void* stream);

/* One entry of the engine's weight-gradient job table (the caller-owned fields of its WgradJob; geometry and scratch
 * placement are filled by the entry point, as the engine does):
 *   dW[q * so_r + k * so_k] += alpha * sum_m (P[m][seg * r + q] * row_scale[m / rows_per_sample]) * X[m][k]
 * with seg = k / seg_cols (seg_cols = 0: one segment) and row_scale NULL for none.  X is 16-bit with row stride ldx, P
 * fp32 with row stride ldp.  m_begin > 0 is the tail form: M still counts the rows of all samples, but X, P and
 * row_scale start at row m_begin and only rows [m_begin, M) are summed (rows_per_sample must divide m_begin).
 * conv_tap >= 0: X is an image [n][Hin][Win][K] and row m = (n, oy, ox) of the [Hout][Wout] output grid reads the input
 * pixel under tap (conv_tap / 3, conv_tap % 3) of a 3x3 / pad-1 filter with stride conv_stride, on the nearest-2x
 * upsampled image when conv_ups (zero outside the image); conv_tap = -1: X is a plain [M, K] matrix. */
typedef struct smi_wgrad_job {
  const void* X;
  const float* P;
  float* dW;
  const float* row_scale;
  int64_t ldx, ldp, so_r, so_k;
  int M, K, r, seg_cols, rows_per_sample;
  float alpha;
  int m_begin, conv_tap, Hin, Win, Hout, Wout, conv_stride, conv_ups;
} smi_wgrad_job;
/* The engine's grouped reduction on a table of n jobs of any ranks (1..32) in any order: planned, sorted by accumulator
 * class and launched exactly as a backward pass does it.  scratch (device, fp32): every job's partials, each rounded up
 * to 64 floats, followed by the device copy of the table; smi_op_lora_wgrad_jobs_floats gives the size.  Fails with a
 * message when scratch_floats is smaller.  Synchronises the stream before it returns. */
int smi_op_lora_wgrad_jobs_floats(const smi_wgrad_job* jobs, int n, size_t* out_floats);
int smi_op_lora_wgrad_jobs(int dtype, const smi_wgrad_job* jobs, int n, float* scratch, size_t scratch_floats,
                           void* stream);

/* One DoRA Linear (T/dora.py:124-162), possibly a fused projection of nseg segments that share the frozen W
 * [nseg * cs, K] (16-bit).  down / up are the flat fp32 parameter buffers: segment s has lora_down [r, K] at
 * down + off_down + s * r * K, lora_up [cs, r] at up + off_up + s * cs * r and dora_scale [K] at up + off_dora + s * K
 * (off_down a multiple of 4 floats, K % 8 == 0).  Outputs: cnorm [nseg, K] fp32 column norms of V = W + up down,
 * dW [nseg * cs, K] 16-bit = mult * scale * (V * dora_scale / cnorm - W), dWt [K, nseg * cs] its transpose. */
typedef struct smi_dora_site {
  const void* W;
  int64_t off_down, off_up, off_dora;
  void* dW;
  void* dWt;
  float* cnorm;
  int r, nseg, K, cs;
  float scale;
} smi_dora_site;
/* cnorm, dW and dWt of n_sites sites in the engine's three launches (norms, deltas, transposes; one rank class for the
 * whole table).  sites_dev: device memory for the table, n_sites * sizeof(smi_dora_site) bytes.  Synchronises. */
int smi_op_dora_prep(int dtype, const smi_dora_site* sites, int n_sites, const float* down, const float* up, float mult,
                     void* sites_dev, void* stream);
/* Gradients of one site from G = d(loss) / d(dW) (fp32 [nseg * cs, K]) with the column norm detached, accumulated (+=)
 * into the flat buffers: d_down at off_down, d_up at off_up (lora_up) and off_dora (dora_scale), all times
 * alpha * (alpha_dev ? alpha_dev[0] : 1).  Reads site->cnorm (smi_op_dora_prep).  scratch: device fp32,
 * smi_op_dora_grads_floats of them; fails with a message when scratch_floats is smaller. */
int smi_op_dora_grads_floats(const smi_dora_site* site, size_t* out_floats);
int smi_op_dora_grads(int dtype, const smi_dora_site* site, const float* G, const float* down, const float* up,
                      float* d_down, float* d_up, float alpha, const float* alpha_dev, float* scratch,
                      size_t scratch_floats, void* stream);
/* dst[c][m] (16-bit, [C, Mp]) = src[m][c] (row stride lds) * (f ? f[m / rows_per_sample] : 1) for m < M, 0 for
 * M <= m < Mp: the operand transposes of the DoRA weight-gradient GEMM.  16-byte accesses when C % 8 == 0, lds % 8 == 0,
 * Mp % 64 == 0 and both pointers are 16-byte aligned, element-wise otherwise. */
int smi_op_transpose_scaled(int dtype, const void* src, int64_t lds, void* dst, int M, int C, int Mp, const float* f,
                            int rows_per_sample, void* stream);
/* The 16-bit shadow operands of the adapted GEMMs, rebuilt from the flat fp32 parameters once per forward.  Per site, at
 * element offsets into `shadow`: downT [rows_pad, K] at dst_down = the nseg * r lora_down rows (at down + off_down), zero
 * rows up to rows_pad; upT [rows_pad, nseg * cs] at dst_up, block diagonal: upT[s * r + q][s * cs + n] = lora_up_s[n][q]
 * (lora_up_s [cs, r] at up + off_up + s * cs * r).  conv = 1 / 2: a 3x3 conv site, lora_down is [r][K][3][3]: downT is
 * [rows_pad, 9 K] in (tap, channel) order, and dst_gw gets the gradient filter [K][9][64], gw[c][tt][q] = down[q][c][t]
 * with t = 8 - tt (conv = 1: flipped taps) or t = tt (conv = 2: the stride-2 layer), zero for q >= r.
 * sites_dev: device memory for the table, n_sites * sizeof(smi_lora_prep_site) bytes.  Synchronises. */
typedef struct smi_lora_prep_site {
  int64_t off_down, off_up, dst_down, dst_up;
  int r, nseg, K, cs, rows_pad, conv;
  int64_t dst_gw;
} smi_lora_prep_site;
int smi_op_lora_prep(int dtype, const smi_lora_prep_site* sites, int n_sites, const float* down, const float* up,
                     void* shadow, void* sites_dev, void* stream);
/* The per-sample power-of-two loss scales of a backward pass: scale_out[j] = 2^e with max|d_eps[j]| * 2^e in
 * (target / 2, target] (target 16; 1 for an all-zero sample), scale_out[inv_off + j] = 1 / scale_out[j]; then
 * min_out[0] = min_j scale, min_out[1] = 1 / min, min_out[2 + j] = min / scale_out[j]. */
int smi_op_grad_scale(const float* d_eps, int n_samples, int64_t per_sample, float* scale_out, int inv_off,
                      float* min_out, void* stream);
/* dst[i] (T) = src[i] (fp32), n % 8 == 0: the 16-bit operand of an fp32 master tensor (the embedding null-text inversion
 * optimises is kept in fp32 and handed to smi_unet_forward in T) */
int smi_op_cast_f32(int dtype, const float* src, void* dst, int64_t n, void* stream);
/* x[m][0..n) (fp32, row stride ld) *= row_mul[m / rows_per_mul] */
int smi_op_row_scale_f32(float* x, int ld, int m, int n, const float* row_mul, int rows_per_mul, void* stream);
/* x[i][j] (fp32, row stride ld) *= col_mul[(i / rows_per_mul) * ld_mul + j % period] for j < n */
int smi_op_col_scale_f32(float* x, int ld, int m, int n, const float* col_mul, int ld_mul, int period, int rows_per_mul,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SMI_H_ */
