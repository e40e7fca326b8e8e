"""Step helpers with the reference's signatures (conceptmod/textsliders/train_util.py:27-47, 91-105, 267-327,
449-489, 677-708, 976-1097).  They are model-agnostic host code: `unet` is the engine-backed
sliders_conceptmod_amd.unet.UNet2DConditionModel (or anything with the same call surface)."""
from typing import Optional

import torch

from . import _native

UNET_IN_CHANNELS = 4
VAE_SCALE_FACTOR = 8
UNET_ATTENTION_TIME_EMBED_DIM = 256
TEXT_ENCODER_2_PROJECTION_DIM = 1280
UNET_PROJECTION_CLASS_EMBEDDING_INPUT_DIM = 2816


def get_random_noise(batch_size: int, height: int, width: int, generator: torch.Generator = None) -> torch.Tensor:
    return torch.randn((batch_size, UNET_IN_CHANNELS, height // VAE_SCALE_FACTOR, width // VAE_SCALE_FACTOR),
                       generator=generator, device="cpu")


def get_initial_latents(scheduler, n_imgs: int, height: int, width: int, n_prompts: int, generator=None):
    noise = get_random_noise(n_imgs, height, width, generator=generator).repeat(n_prompts, 1, 1, 1)
    return noise * scheduler.init_noise_sigma.to(noise.device)


def concat_embeddings(unconditional, conditional, n_imgs: int):
    return torch.cat([unconditional, conditional]).repeat_interleave(n_imgs, dim=0)


def _cfg(noise_pred: torch.Tensor, guidance_scale: float) -> torch.Tensor:
    if noise_pred.is_cuda and noise_pred.dtype == torch.float32 and not noise_pred.requires_grad:
        return _native.cfg_combine(noise_pred.contiguous(), guidance_scale)
    u, t = noise_pred.chunk(2)  # differentiable path (the adapted pass under autograd)
    return u + guidance_scale * (t - u)


def predict_noise(unet, scheduler, timestep, latents, text_embeddings, guidance_scale=7.5):
    latent_model_input = torch.cat([latents] * 2)
    latent_model_input = scheduler.scale_model_input(latent_model_input, timestep)
    noise_pred = unet(latent_model_input, timestep, encoder_hidden_states=text_embeddings).sample
    return _cfg(noise_pred, guidance_scale)


@torch.no_grad()
def diffusion(unet, scheduler, latents, text_embeddings, total_timesteps: int = 1000, start_timesteps=0, **kwargs):
    for timestep in scheduler.timesteps[start_timesteps:total_timesteps]:
        noise_pred = predict_noise(unet, scheduler, timestep, latents, text_embeddings, **kwargs)
        latents = scheduler.step(noise_pred, timestep, latents).prev_sample
    return latents


# ---- SD3 (conceptmod/textsliders/train_util.py get_initial_latents_sd3, concat_embeddings_sd3, predict_noise_sd3,
# diffusion_sd3, encode_prompts_sd3): re-written from their documented behaviour on the native MMDiT -------------------------
SD3_LATENT_CHANNELS = 16


def get_initial_latents_sd3(scheduler, n_imgs: int, height: int, width: int, n_prompts: int, generator=None):
    """randn [n_imgs, 16, height / 8, width / 8] (the reference draws it on the device; here on the CPU from `generator`, as
    the other get_initial_latents do: the caller moves it).  init_noise_sigma is 1 and n_prompts is not used, as there."""
    return torch.randn((n_imgs, SD3_LATENT_CHANNELS, height // VAE_SCALE_FACTOR, width // VAE_SCALE_FACTOR),
                       generator=generator, device="cpu")


def concat_embeddings_sd3(unconditional, conditional, n_imgs: int):
    return torch.cat([unconditional, conditional]).repeat_interleave(n_imgs, dim=0)


def encode_prompts_sd3(pipeline, tokenizers, text_encoders, prompt: str, num_images_per_prompt: int = 1,
                       t5_tokens: int = 256, joint_attention_dim: int = 4096):
    """(prompt_embeds [n, 77 + t5_tokens, joint_attention_dim], pooled [n, p1 + p2]) as the SD3 pipeline encodes a prompt
    with text_encoder_3=None: hidden_states[-2] of the two CLIP towers concatenated on the feature axis and zero-padded to
    joint_attention_dim, then t5_tokens zero rows appended on the sequence axis (256: the published pipeline's
    max_sequence_length; 77 reproduces its first release); pooled: the two projected pooled embeddings concatenated.
    `pipeline` is the reference's first argument and is not used (there is no pipeline object here).  A third tower
    (model_util.NativeT5Tower: load_models_sd3(t5_backend="native")) writes its t5_tokens rows where the zero rows are, as the
    pipeline with text_encoder_3 does."""
    del pipeline
    embeds, pooled = [], []
    for tok, enc in zip(tokenizers[:2], text_encoders[:2]):
        ids = tok(prompt, padding="max_length", max_length=tok.model_max_length, truncation=True,
                  return_tensors="pt").input_ids
        out = enc(ids.to(enc.device), output_hidden_states=True)
        pooled.append(out[0])
        embeds.append(out.hidden_states[-2])
    clip = torch.cat(embeds, dim=-1)
    if clip.shape[-1] > joint_attention_dim:
        raise ValueError(f"the CLIP towers are {clip.shape[-1]} wide, the transformer's context {joint_attention_dim}")
    clip = torch.nn.functional.pad(clip, (0, joint_attention_dim - clip.shape[-1]))
    t5 = text_encoders[2] if len(text_encoders) > 2 else None
    if t5 is None:
        zeros = torch.zeros(clip.shape[0], t5_tokens, joint_attention_dim, dtype=clip.dtype, device=clip.device)
    else:
        zeros = t5.encode_cached(prompt, t5_tokens).to(clip.device, clip.dtype)
        if zeros.shape[-1] != joint_attention_dim:
            raise ValueError(f"the T5 tower is {zeros.shape[-1]} wide, the transformer's context {joint_attention_dim}")
    prompt_embeds = torch.cat([clip, zeros], dim=1).repeat_interleave(num_images_per_prompt, dim=0)
    return prompt_embeds, torch.cat(pooled, dim=-1).repeat_interleave(num_images_per_prompt, dim=0)


def predict_noise_sd3(transformer, scheduler, timestep, latents, text_embeddings, add_text_embeddings,
                      guidance_scale=7.5, multipliers=None):
    """One CFG step: returns the STEPPED latents, not the prediction (as the reference does).  The network is fed the
    scheduler's timestep (1000 sigma).  `multipliers` (not in the reference signature): one adaptor multiplier per sample
    of the doubled batch, for a transformer with an attached LoRANetwork."""
    latent_model_input = torch.cat([latents] * 2)
    v = transformer(hidden_states=latent_model_input, timestep=[float(timestep)] * latent_model_input.shape[0],
                    encoder_hidden_states=text_embeddings, pooled_projections=add_text_embeddings,
                    multipliers=multipliers, return_dict=False)[0]
    guided = _cfg(v, guidance_scale)
    return scheduler.step(guided, timestep, latents, return_dict=False)[0]


@torch.no_grad()
def diffusion_sd3(transformer, scheduler, latents, text_embeddings, add_text_embeddings, guidance_scale: float = 1.0,
                  total_timesteps: int = 1000, start_timesteps=0):
    for timestep in scheduler.timesteps[start_timesteps:total_timesteps]:
        latents = predict_noise_sd3(transformer, scheduler, timestep, latents, text_embeddings, add_text_embeddings,
                                    guidance_scale=guidance_scale)
    return latents


@torch.no_grad()
def slider_sweep_latents_sd3(transformer, network, scheduler, latents, text_embeddings, add_text_embeddings, scale: float,
                             start_noise: float, guidance_scale: float, adapted_embeddings=None):
    """diffusion_sd3 over the whole schedule with the slider off while t > start_noise (on the 1000 sigma axis) and at
    `scale` below it.  adapted_embeddings: the context under a text-tower LoRA at `scale` (generate_images' T5 sweep): it
    replaces text_embeddings on the same steps on which the slider is on, as slider_sweep_latents does for SD-XL."""
    for timestep in scheduler.timesteps:
        below = float(timestep) <= start_noise
        on = network is not None and below
        m = [float(scale) if on else 0.0] * (2 * latents.shape[0]) if network is not None else None
        emb = adapted_embeddings if (adapted_embeddings is not None and below) else text_embeddings
        latents = predict_noise_sd3(transformer, scheduler, timestep, latents, emb, add_text_embeddings,
                                    guidance_scale=guidance_scale, multipliers=m)
    return latents


# ---- Flux (conceptmod/textsliders/train_util.py get_initial_latents_flux, concat_embeddings_flux, encode_prompts_flux,
# predict_noise_flux, diffusion_flux): their signatures where they make sense without a pipeline object (`pipeline` is kept as
# the first argument and not used); latents stay UN-packed [n, 16, h, w] -- the engine packs and un-packs -------------------
FLUX_LATENT_CHANNELS = 16


def get_initial_latents_flux(scheduler, n_imgs: int, height: int, width: int, n_prompts: int, generator=None):
    """randn [n_imgs, 16, height / 8, width / 8], on the CPU from `generator` (the reference draws on the device, unseeded)."""
    return torch.randn((n_imgs, FLUX_LATENT_CHANNELS, height // VAE_SCALE_FACTOR, width // VAE_SCALE_FACTOR),
                       generator=generator, device="cpu")


def concat_embeddings_flux(unconditional, conditional, n_imgs: int):
    return torch.cat([unconditional, conditional]).repeat_interleave(n_imgs, dim=0).detach()


def encode_prompts_flux(pipeline, tokenizers, text_encoders, prompt: str, num_images_per_prompt: int = 1,
                        max_sequence_length: int = 512, joint_attention_dim: int = 4096):
    """(prompt_embeds [n, max_sequence_length, joint_attention_dim], pooled [n, pooled_projection_dim]) as the Flux pipeline's
    encode_prompt: pooled is CLIP-L's un-projected pooled row (pooler_output, from the native text engine), prompt_embeds the
    T5 tower's output (text_encoders[1]: model_util.T5Tower, frozen torch in bf16 / fp32, run once per distinct prompt:
    its `encode_cached`) -- or, where text_encoders[1] is None, max_sequence_length zero rows, as for SD3."""
    del pipeline
    tok, clip = tokenizers[0], text_encoders[0]
    ids = tok(prompt, padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt").input_ids
    pooled = clip(ids.to(clip.device), output_hidden_states=False).pooler_output
    t5 = text_encoders[1] if len(text_encoders) > 1 else None
    if t5 is None:
        embeds = torch.zeros(1, max_sequence_length, joint_attention_dim, dtype=pooled.dtype, device=pooled.device)
    else:
        embeds = t5.encode_cached(prompt, max_sequence_length).to(pooled.device, pooled.dtype)
        if embeds.shape[-1] != joint_attention_dim:
            raise ValueError(f"the T5 tower is {embeds.shape[-1]} wide, the transformer's context {joint_attention_dim}")
    return (embeds.repeat_interleave(num_images_per_prompt, dim=0), pooled.repeat_interleave(num_images_per_prompt, dim=0))


def set_timesteps_flux(scheduler, num_inference_steps: int, latents):
    """The Flux pipeline's schedule: sigmas linspace(1, 1 / n, n), with mu from the image sequence length (h / 2) (w / 2) where
    the scheduler shifts dynamically (FLUX.1-dev)."""
    sig = torch.linspace(1.0, 1.0 / num_inference_steps, num_inference_steps, dtype=torch.float64)
    seq = (latents.shape[2] // 2) * (latents.shape[3] // 2)
    scheduler.set_timesteps(sigmas=sig, mu=scheduler.calculate_shift(seq) if scheduler.use_dynamic_shifting else None)


def predict_noise_flux(pipeline, transformer, scheduler, timestep, latents, text_embeddings, add_text_embeddings,
                       guidance_scale=7.5, multipliers=None):
    """One step, ONE transformer pass (no CFG pair): returns the STEPPED latents, as the reference does.  The network is fed
    the scheduler's timestep (1000 sigma: the reference passes timestep / 1000 to a model that multiplies by 1000) and, where
    it has a guidance embedder (FLUX.1-dev), guidance_scale as the embedded guidance; FLUX.1-schnell ignores it.
    `multipliers` (not in the reference signature): one adaptor multiplier per sample."""
    del pipeline
    n = latents.shape[0]
    guidance = [float(guidance_scale)] * n if transformer.cfg.guidance_embeds else None
    v = transformer(hidden_states=latents, timestep=[float(timestep)] * n, guidance=guidance,
                    pooled_projections=add_text_embeddings, encoder_hidden_states=text_embeddings,
                    multipliers=multipliers, return_dict=False)[0]
    return scheduler.step(v, timestep, latents, return_dict=False)[0]


@torch.no_grad()
def diffusion_flux(pipeline, transformer, scheduler, latents, text_embeddings, add_text_embeddings,
                   guidance_scale: float = 1.0, total_timesteps: int = 1000, start_timesteps=0, num_inference_steps=4):
    set_timesteps_flux(scheduler, num_inference_steps, latents)
    for timestep in scheduler.timesteps[start_timesteps:total_timesteps]:
        latents = predict_noise_flux(pipeline, transformer, scheduler, timestep, latents, text_embeddings,
                                     add_text_embeddings, guidance_scale=guidance_scale)
    return latents


@torch.no_grad()
def slider_sweep_latents_flux(transformer, network, scheduler, latents, text_embeddings, add_text_embeddings, scale: float,
                              start_noise: float, guidance_scale: float, num_inference_steps: int, adapted_embeddings=None):
    """diffusion_flux over the whole schedule with the slider off while 1000 sigma > start_noise and at `scale` below it.
    adapted_embeddings: as in slider_sweep_latents_sd3."""
    set_timesteps_flux(scheduler, num_inference_steps, latents)
    for timestep in scheduler.timesteps:
        below = float(timestep) <= start_noise
        on = network is not None and below
        m = [float(scale) if on else 0.0] * latents.shape[0] if network is not None else None
        emb = adapted_embeddings if (adapted_embeddings is not None and below) else text_embeddings
        latents = predict_noise_flux(None, transformer, scheduler, timestep, latents, emb, add_text_embeddings,
                                     guidance_scale=guidance_scale, multipliers=m)
    return latents


def predict_noise_xl(unet, scheduler, timestep, latents, text_embeddings, add_text_embeddings, add_time_ids,
                     guidance_scale=7.5, guidance_rescale=0.7):
    latent_model_input = torch.cat([latents] * 2)
    latent_model_input = scheduler.scale_model_input(latent_model_input, timestep)
    added_cond_kwargs = {"text_embeds": add_text_embeddings, "time_ids": add_time_ids}
    noise_pred = unet(latent_model_input, timestep, encoder_hidden_states=text_embeddings,
                      added_cond_kwargs=added_cond_kwargs).sample
    # the reference computes rescale_noise_cfg here and discards it (train_util.py:485-489); the plain mix is returned
    return _cfg(noise_pred, guidance_scale)


@torch.no_grad()
def diffusion_xl(unet, scheduler, latents, text_embeddings, add_text_embeddings, add_time_ids,
                 guidance_scale: float = 1.0, total_timesteps: int = 1000, start_timesteps=0):
    for timestep in scheduler.timesteps[start_timesteps:total_timesteps]:
        noise_pred = predict_noise_xl(unet, scheduler, timestep, latents, text_embeddings, add_text_embeddings,
                                      add_time_ids, guidance_scale=guidance_scale, guidance_rescale=0.7)
        latents = scheduler.step(noise_pred, timestep, latents).prev_sample
    return latents


@torch.no_grad()
def slider_sweep_latents(unet, network, scheduler, latents, text_embeddings, scale: float, start_noise: int,
                         guidance_scale: float = 7.5, num_inference_steps: int = 50, added_cond=None,
                         uncond_per_step=None, adapted_embeddings=None, adapted_added_cond=None,
                         uncond_pooled_per_step=None):
    """The inference-side slider loop of the eval scripts (eval-scripts/generate_images_sd1.py:170-190,
    generate_images_xl.py:327-343): denoise from `latents` (already x init_noise_sigma) with classifier-free guidance, the
    adaptor OFF (set_lora_slider(0)) while t > start_noise and at `scale` afterwards, every UNet call inside `with network`.
    `text_embeddings` = cat([uncond, cond]) as there; `added_cond` = (add_text_embeddings, add_time_ids) for SD-XL.
    `uncond_per_step` (real-image editing, demo_image_editing.ipynb): one unconditional embedding [1, L, D] per step, as
    null-text inversion returns them -- step k runs on cat([uncond_per_step[k] expanded to the batch, cond]), `cond` being
    the second half of `text_embeddings`; None: `text_embeddings` as given at every step.
    `uncond_pooled_per_step` (SD-XL real-image editing, with `uncond_per_step` and `added_cond`): one unconditional pooled
    embedding [1, P] per step, as NullInversionXL returns them -- step k runs with text_embeds = cat([uncond_pooled_per_step[k]
    expanded to the batch, the conditional half of added_cond[0]]).
    `adapted_embeddings` / `adapted_added_cond` (a text-encoder LoRA, conceptmod/notrigger): the same two things encoded under
    the text-encoder adaptor at `scale`; they replace `text_embeddings` / `added_cond` at the steps where the UNet slider is
    on (t <= start_noise) -- the same flip.  `network` may then be None: a text-encoder-only sweep.
    Returns the final latents (decoding them is the VAE decoder's job, outside this package)."""
    import contextlib
    scheduler.set_timesteps(num_inference_steps)
    plain_embeddings, plain_added = text_embeddings, added_cond
    if uncond_per_step is not None and len(uncond_per_step) != len(scheduler.timesteps):
        raise ValueError(f"{len(uncond_per_step)} unconditional embeddings for {len(scheduler.timesteps)} steps")
    if uncond_pooled_per_step is not None:
        if uncond_per_step is None or added_cond is None:
            raise ValueError("uncond_pooled_per_step goes with uncond_per_step and added_cond (SD-XL)")
        if len(uncond_pooled_per_step) != len(scheduler.timesteps):
            raise ValueError(f"{len(uncond_pooled_per_step)} unconditional pooled embeddings for "
                             f"{len(scheduler.timesteps)} steps")
    cond = text_embeddings.chunk(2)[1]
    for k, t in enumerate(scheduler.timesteps):
        on = not (t > start_noise)
        if network is not None:
            network.set_lora_slider(scale=scale if on else 0)
        text_embeddings = adapted_embeddings if on and adapted_embeddings is not None else plain_embeddings
        added_cond = adapted_added_cond if on and adapted_added_cond is not None else plain_added
        if uncond_per_step is not None:
            cond = text_embeddings.chunk(2)[1]
            u = uncond_per_step[k].to(cond.device, cond.dtype)
            text_embeddings = torch.cat([u.expand(*cond.shape), cond])
        if uncond_pooled_per_step is not None:
            pooled_cond = added_cond[0].chunk(2)[1]
            pu = uncond_pooled_per_step[k].to(pooled_cond.device, pooled_cond.dtype)
            added_cond = (torch.cat([pu.expand(*pooled_cond.shape), pooled_cond]), added_cond[1])
        with (network if network is not None else contextlib.nullcontext()):
            if added_cond is None:
                noise_pred = predict_noise(unet, scheduler, t, latents, text_embeddings, guidance_scale=guidance_scale)
            else:
                noise_pred = predict_noise_xl(unet, scheduler, t, latents, text_embeddings, added_cond[0], added_cond[1],
                                              guidance_scale=guidance_scale)
        latents = scheduler.step(noise_pred, t, latents).prev_sample
    if network is not None:
        network.set_lora_slider(scale=1)
    return latents


@torch.no_grad()
def slider_grid_latents(unet, stack, scheduler, latents, text_embeddings, scale_rows, start_noise: int,
                        guidance_scale: float = 7.5, num_inference_steps: int = 50, added_cond=None,
                        max_batch: Optional[int] = None):
    """`slider_sweep_latents` for a list of scale rows (one row of K scales per cell of a grid) on a compose.SliderStack.

    While t > start_noise the adaptor is off and every cell is the same computation: it runs ONCE, on the `num_samples`
    CFG pairs of `latents`, and is broadcast at the switch.  From there every cell runs in one UNet pass per step: a batch of
    cells x num_samples x 2 with both CFG halves adapted (as in the reference) and one multiplier row per sample.
    `max_batch` bounds that UNet batch: the grid is processed in chunks of max(1, max_batch // (2 num_samples)) cells, each
    chunk on its own copy of the scheduler (a multistep scheduler's history is expanded to the chunk).  Schedulers that draw
    noise per step (ddpm, euler_a) draw it for the whole chunk at once, so only the deterministic ones (ddim, lms) give a
    cell the latents it would get on its own.  The scales or grid set on the stack before the call are put back.
    Returns the final latents [cells, num_samples, C, h, w]."""
    import copy
    from .compose import grid_multiplier_rows
    scheduler.set_timesteps(num_inference_steps)
    scale_rows = [list(r) for r in scale_rows]
    if not scale_rows:
        raise ValueError("slider_grid_latents: no scale rows")
    ns = latents.shape[0]
    timesteps = list(scheduler.timesteps)
    added = added_cond

    def predict(sched, t, lat, te, add):
        if add is None:
            return predict_noise(unet, sched, t, lat, te, guidance_scale=guidance_scale)
        return predict_noise_xl(unet, sched, t, lat, te, add[0], add[1], guidance_scale=guidance_scale)

    k0 = 0
    while k0 < len(timesteps) and timesteps[k0] > start_noise:  # adaptor off: shared by every cell
        noise_pred = predict(scheduler, timesteps[k0], latents, text_embeddings, added)
        latents = scheduler.step(noise_pred, timesteps[k0], latents).prev_sample
        k0 += 1
    per = len(scale_rows) if max_batch is None else max(1, int(max_batch) // (2 * ns))
    if getattr(stack, "fold", False):  # conv sites: the scales live in lora_up, one cell per pass
        per = 1
    else:  # the engine's multiplier table bounds the samples of a pass
        if 2 * ns > stack.max_samples:
            raise ValueError(f"one cell is {2 * ns} samples, but a pass of this stack takes at most {stack.max_samples} "
                             f"(the multiplier table: {stack.max_samples} x rank {sum(stack.ranks)}); lower num_samples")
        per = min(per, stack.max_samples // (2 * ns))
    saved = stack.scale_state()
    unc, cond = text_embeddings.chunk(2)
    out = []
    for c0 in range(0, len(scale_rows), per):
        rows = scale_rows[c0:c0 + per]
        c = len(rows)
        sched = copy.deepcopy(scheduler)
        if getattr(sched, "derivatives", None):
            sched.derivatives = [d.repeat(c, 1, 1, 1) for d in sched.derivatives]
        lat = latents.repeat(c, 1, 1, 1)
        te = torch.cat([unc.repeat(c, 1, 1), cond.repeat(c, 1, 1)])
        add = None
        if added is not None:
            pu, pc = added[0].chunk(2)
            tu, tc = added[1].chunk(2)
            add = (torch.cat([pu.repeat(c, 1), pc.repeat(c, 1)]), torch.cat([tu.repeat(c, 1), tc.repeat(c, 1)]))
        stack.set_scale_grid(grid_multiplier_rows(rows, ns))
        for t in timesteps[k0:]:
            with stack:
                noise_pred = predict(sched, t, lat, te, add)
            lat = sched.step(noise_pred, t, lat).prev_sample
        out.append(lat.view(c, ns, *lat.shape[1:]))
    stack.restore_scale_state(saved)
    return torch.cat(out)


@torch.no_grad()
def get_noisy_image(img, vae, generator, unet, scheduler, total_timesteps: int = 1000, start_timesteps=0, **kwargs):
    """Image-slider front end (trainscripts/imagesliders/train_util.py:200-235), same signature and order of operations:
    preprocess -> vae.encode(image).latent_dist.sample(None) -> x vae.config.scaling_factor -> noise = randn(shape,
    generator) -> scheduler.add_noise(latents, noise, scheduler.timesteps[total_timesteps : total_timesteps + 1]).
    Returns (noised latents, noise).  `unet`, `start_timesteps` are unused there too."""
    from .vae import VaeImageProcessor
    vae_scale_factor = 2 ** (len(vae.config.block_out_channels) - 1)
    image = VaeImageProcessor(vae_scale_factor=vae_scale_factor).preprocess(img).to(vae.device)
    init_latents = vae.encode(image).latent_dist.sample(None)
    init_latents = vae.config.scaling_factor * init_latents
    shape = init_latents.shape
    # randn_tensor(shape, generator=generator, device=device): a CPU generator draws on the host and the result is moved
    gdev = "cpu" if generator is None or generator.device.type == "cpu" else init_latents.device
    noise = torch.randn(shape, generator=generator, device=gdev, dtype=init_latents.dtype).to(init_latents.device)
    timestep = scheduler.timesteps[total_timesteps:total_timesteps + 1]
    init_latents = scheduler.add_noise(init_latents, noise, timestep)
    return init_latents, noise


def get_noisy_image_pair(imgs, vae, make_generator, unet, scheduler, total_timesteps: int = 1000, start_timesteps=0,
                         **kwargs):
    """`[get_noisy_image(img, vae, make_generator(), ...) for img in imgs]` for images of ONE size with a single batched
    VAE encode (the two 1024 x 1024 images of an image-slider step: 2 x 9.1 ms -> one pass of twice the rows).  The
    encoder consumes no random numbers, so calling `make_generator()` -- the reference re-seeds with
    `torch.manual_seed(seed)` per image, I/train_lora-scale-xl.py:220-247 -- right before each image's posterior sample
    keeps the reference's draw ORDER.  The moments are the per-image ones up to fp32 summation order only: a sample's
    kernels are the same whatever its batch, except that the split-K rule (csrc/gemm.hip) picks its slice count from the
    launch's tile count, i.e. from the batch -- the pair-vs-single test therefore holds to a tolerance (2e-3), not bitwise."""
    from .vae import VaeImageProcessor
    vae_scale_factor = 2 ** (len(vae.config.block_out_channels) - 1)
    proc = VaeImageProcessor(vae_scale_factor=vae_scale_factor)
    image = torch.cat([proc.preprocess(img) for img in imgs]).to(vae.device)
    dist = vae.encode(image).latent_dist
    timestep = scheduler.timesteps[total_timesteps:total_timesteps + 1]
    out = []
    for i in range(len(imgs)):
        generator = make_generator()
        init_latents = vae.config.scaling_factor * dist.rows(i, i + 1).sample(None)
        gdev = "cpu" if generator is None or generator.device.type == "cpu" else init_latents.device
        noise = torch.randn(init_latents.shape, generator=generator, device=gdev,
                            dtype=init_latents.dtype).to(init_latents.device)
        out.append((scheduler.add_noise(init_latents, noise, timestep), noise))
    return out


def get_add_time_ids(height: int, width: int, dynamic_crops: bool = False, dtype: torch.dtype = torch.float32):
    if dynamic_crops:
        random_scale = torch.rand(1).item() * 2 + 1
        original_size = (int(height * random_scale), int(width * random_scale))
        crops_coords_top_left = (torch.randint(0, original_size[0] - height, (1,)).item(),
                                 torch.randint(0, original_size[1] - width, (1,)).item())
        target_size = (height, width)
    else:
        original_size = (height, width)
        crops_coords_top_left = (0, 0)
        target_size = (height, width)
    add_time_ids = list(original_size + crops_coords_top_left + target_size)
    passed_add_embed_dim = UNET_ATTENTION_TIME_EMBED_DIM * len(add_time_ids) + TEXT_ENCODER_2_PROJECTION_DIM
    if passed_add_embed_dim != UNET_PROJECTION_CLASS_EMBEDDING_INPUT_DIM:
        raise ValueError(f"Model expects an added time embedding vector of length "
                         f"{UNET_PROJECTION_CLASS_EMBEDDING_INPUT_DIM}, but a vector of {passed_add_embed_dim} was "
                         f"created.")
    return torch.tensor([add_time_ids], dtype=dtype)


def get_optimizer(name: str):
    name = name.lower()
    if name == "adam":
        return torch.optim.Adam
    if name == "adamw":
        return torch.optim.AdamW
    if name == "lion":  # the reference imports lion_pytorch / prodigyopt here; optim.py holds classes of our own
        from .optim import Lion
        return Lion
    if name == "prodigy":
        from .optim import Prodigy
        return Prodigy
    if name.startswith("dadapt") or name.endswith("8bit"):
        # the reference imports dadaptation / bitsandbytes here; neither is in this image
        raise ValueError(f"optimizer '{name}' needs a package that is not installed; use adam or adamw")
    raise ValueError("Optimizer must be adam, adamw, lion or Prodigy")


def get_lr_scheduler(name: Optional[str], optimizer, max_iterations: Optional[int], lr_min: Optional[float], **kwargs):
    if name == "cosine":
        return torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=max_iterations, eta_min=lr_min, **kwargs)
    elif name == "cosine_with_restarts":
        return torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(optimizer, T_0=max_iterations // 10, T_mult=2,
                                                                    eta_min=lr_min, **kwargs)
    elif name == "step":
        return torch.optim.lr_scheduler.StepLR(optimizer, step_size=max_iterations // 100, gamma=0.999, **kwargs)
    elif name == "constant":
        return torch.optim.lr_scheduler.ConstantLR(optimizer, factor=1, **kwargs)
    elif name == "linear":
        # the reference passes LinearLR(factor=0.5, ...), which is not a torch keyword and raises TypeError
        # (tests/golden: error/lr_scheduler_linear); the evident intent is start_factor
        return torch.optim.lr_scheduler.LinearLR(optimizer, start_factor=0.5, total_iters=max_iterations // 100,
                                                 **kwargs)
    raise ValueError("Scheduler must be cosine, cosine_with_restarts, step, linear or constant")


def get_random_resolution_in_bucket(bucket_resolution: int = 512):
    max_resolution = bucket_resolution
    min_resolution = bucket_resolution // 2
    step = 64
    min_step = min_resolution // step
    max_step = max_resolution // step
    height = torch.randint(min_step, max_step, (1,)).item() * step
    width = torch.randint(min_step, max_step, (1,)).item() * step
    return height, width
