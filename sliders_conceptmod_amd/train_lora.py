"""Text-slider trainer for SD-1.x -- same CLI, YAML schemas, step order, RNG draw order and output naming as the
reference script (conceptmod/textsliders/train_lora.py:32-419), on the HIP engine.

    python -m sliders_conceptmod_amd.train_lora --config_file cfg.yaml --alpha 1 --rank 4 --device 0 --name ageslider \
           --attributes "male, female"

Differences, all recorded in DESIGN.md: the reference's stale 6-argument PromptEmbedsPair / `unconditional_latents`
call works (prompt_util.py here accepts both forms); `--device cpu` is rejected (no CPU path); under torch.distributed.run the batch is
sharded over ranks and the LoRA gradient is all-reduced."""
import argparse

import torch
from tqdm import tqdm

from . import config_util, model_util, parallel, prompt_util, train_common, train_util
from .config_util import RootConfig
from .lora import DEFAULT_TARGET_REPLACE, UNET_TARGET_REPLACE_MODULE_CONV, LoRANetwork
from .prompt_util import PromptEmbedsCache, PromptEmbedsPair
from .train_common import add_fused_step_flags  # noqa: F401  (its home is train_common; importable from here as before)


def encode(text_encoder, tokenizer, prompt, device, dtype):
    if isinstance(text_encoder, model_util.SyntheticTextEncoder):
        return text_encoder.encode(prompt).to(device, dtype)
    tokens = tokenizer[0](prompt, padding="max_length", max_length=tokenizer[0].model_max_length, truncation=True,
                          return_tensors="pt").input_ids
    return text_encoder[0](tokens.to(text_encoder[0].device))[0].to(device, dtype)


def train(config: RootConfig, prompts: list, device, models=None, on_step_complete=None, save_file=True,
          fused_step=None, dedup_uncond: bool = True):
    """`fused_step` (not in the reference signature): None (default) = the fused path whenever the configured optimiser is
    Adam / AdamW, Lion or Prodigy with arguments the native step takes (train_common.step_choice), else the reference-style
    autograd loop; True = fused or ValueError; False = the reference-style loop.
    `dedup_uncond`: inside the fused step, run each distinct frozen sample once (bit-identical results, step.py)."""
    metadata = {"prompts": ",".join([p.model_dump_json() for p in prompts]), "config": config.model_dump_json()}
    # train_lora.py:44-46: `modules = DEFAULT_TARGET_REPLACE; modules += UNET_TARGET_REPLACE_MODULE_CONV` mutates the list
    # that LoRANetwork's default argument is bound to, which is how c3lier reaches the network there; here it is passed
    modules = list(DEFAULT_TARGET_REPLACE)
    if config.network.type == "c3lier":
        modules += UNET_TARGET_REPLACE_MODULE_CONV
    weight_dtype = config_util.parse_precision(config.train.precision)
    save_weight_dtype = config_util.parse_precision(config.train.precision)  # sic: train.precision (train_lora.py:55)
    if weight_dtype == torch.float32:
        raise ValueError("the HIP engine computes in fp16/bf16 storage with fp32 accumulation; set train.precision")
    tokenizer, text_encoder, unet, noise_scheduler = models or model_util.load_models(
        config.pretrained_model.name_or_path, scheduler_name=config.train.noise_scheduler,
        v2=config.pretrained_model.v2, v_pred=config.pretrained_model.v_pred)
    # data parallelism: one control RNG for all ranks, seeded BEFORE the adaptor init draws from it (parallel.py)
    rank, world = parallel.world_info()
    parallel.sync_control_rng(device=device)
    noise_scheduler.dp_shard = (rank, world)
    train_common.place_frozen(text_encoder, unet, device, weight_dtype)  # train_lora.py:64-70
    unet.enable_xformers_memory_efficient_attention()
    network = LoRANetwork(unet, rank=config.network.rank, multiplier=1.0, alpha=config.network.alpha,
                          train_method=config.network.training_method, target_replace=modules).to(device,
                                                                                                   dtype=weight_dtype)
    parallel.broadcast_(network.flat.data)
    optimizer_module = train_util.get_optimizer(config.train.optimizer)
    optimizer_kwargs = train_common.parse_optimizer_args(config.train.optimizer_args)  # train_lora.py:82-87
    fused, spec = train_common.step_choice(fused_step, config.train.optimizer, optimizer_kwargs)  # may refuse: before any work
    optimizer =optimizer_module(network.prepare_optimizer_params(), lr=config.train.lr, **optimizer_kwargs)
    lr_scheduler = train_util.get_lr_scheduler(config.train.lr_scheduler, optimizer,
                                               max_iterations=config.train.iterations, lr_min=config.train.lr / 100)
    criteria = torch.nn.MSELoss()

    cache = PromptEmbedsCache()
    prompt_pairs = []
    with torch.no_grad():
        for settings in prompts:
            for prompt in [settings.target, settings.positive, settings.neutral, settings.unconditional]:
                if cache[prompt] is None:
                    cache[prompt] = encode(text_encoder, tokenizer, prompt, device, weight_dtype)
            prompt_pairs.append(PromptEmbedsPair(criteria, cache[settings.target], cache[settings.positive],
                                                 cache[settings.unconditional], cache[settings.neutral],
                                                 settings=settings))
    del tokenizer, text_encoder

    # The fused step (default): the pre-roll and the 4-pass step run through SliderStep (one batched UNet pass, native loss /
    # AdamW, Lion or Prodigy, no autograd graph) -- the path bench.py measures.  Same arithmetic and RNG draw order as the
    # reference-style arms below (tested); `--no_fused_step` keeps those.
    stepper = None
    if fused:
        from .step import SliderStep
        stepper = SliderStep(unet, network, noise_scheduler, lr=config.train.lr, optimizer=spec, max_grad_norm=0.0,
                             cfg_scale=1.0, dedup_uncond=dedup_uncond)
    prodigy = config.train.optimizer.lower() == "prodigy"
    cond_cache = {}  # fused path: conditioning tensors per (prompt pair, batch)

    pbar = tqdm(range(config.train.iterations), disable=rank != 0)
    for i in pbar:
        with torch.no_grad():
            noise_scheduler.set_timesteps(config.train.max_denoising_steps, device=device)
            optimizer.zero_grad()
            prompt_pair, timesteps_to, height, width, bs, latents = train_common.draw_text_step(
                prompt_pairs, config, noise_scheduler, rank, world, device)
            if stepper is not None:  # fused: the pre-roll without autograd bookkeeping
                c = cond_cache.get((id(prompt_pair), bs))
                if c is None:
                    emb = {k: getattr(prompt_pair, k) for k in ("target", "positive", "neutral", "unconditional")}
                    c = cond_cache[(id(prompt_pair), bs)] = stepper.make_conditioning(emb, bs)
                denoised_latents = stepper.preroll(latents, c, timesteps_to, 3)
            else:
                with network:
                    denoised_latents = train_util.diffusion(
                        unet, noise_scheduler, latents,
                        train_util.concat_embeddings(prompt_pair.unconditional, prompt_pair.target, bs),
                        start_timesteps=0, total_timesteps=timesteps_to, guidance_scale=3)
            noise_scheduler.set_timesteps(1000)
            current_timestep = noise_scheduler.timesteps[int(timesteps_to * 1000 / config.train.max_denoising_steps)]
            if stepper is not None:
                loss = stepper.train_step(denoised_latents, current_timestep, c, prompt_pair.action,
                                          prompt_pair.guidance_scale, lr=lr_scheduler.get_last_lr()[0])
            else:
                positive_latents = train_util.predict_noise(
                    unet, noise_scheduler, current_timestep, denoised_latents,
                    train_util.concat_embeddings(prompt_pair.unconditional, prompt_pair.positive, bs), guidance_scale=1)
                neutral_latents = train_util.predict_noise(
                    unet, noise_scheduler, current_timestep, denoised_latents,
                    train_util.concat_embeddings(prompt_pair.unconditional, prompt_pair.neutral, bs), guidance_scale=1)
                unconditional_latents = train_util.predict_noise(
                    unet, noise_scheduler, current_timestep, denoised_latents,
                    train_util.concat_embeddings(prompt_pair.unconditional, prompt_pair.unconditional, bs),
                    guidance_scale=1)
        if stepper is not None:
            optimizer.step()  # no gradients: a no-op that keeps torch's "optimizer before scheduler" order
        else:
            with network:
                target_latents = train_util.predict_noise(
                    unet, noise_scheduler, current_timestep, denoised_latents,
                    train_util.concat_embeddings(prompt_pair.unconditional, prompt_pair.target, bs), guidance_scale=1)
            loss = prompt_pair.loss(target_latents=target_latents, positive_latents=positive_latents,
                                    neutral_latents=neutral_latents, unconditional_latents=unconditional_latents)
            loss.backward()
            if world > 1:  # mean over ranks == the gradient of the global-batch MSE
                parallel.allreduce_mean_(network.flat.grad)
            optimizer.step()
        lr_scheduler.step()
        lv = float(loss.item())  # the one host sync per step, as the reference's loss.item() (train_lora.py:292)
        desc = f"Loss*1k: {lv * 1000:.4f}"
        if prodigy:  # the step-size estimate; fused: one more device read, right after loss.item() has synchronised
            desc += f" d: {stepper.prodigy_d() if stepper is not None else optimizer.d:.3e}"
        pbar.set_description(desc)
        if on_step_complete is not None:
            on_step_complete(i, lv)
        if save_file and rank == 0 and train_common.checkpoint_due(i, config):
            train_common.save_checkpoint(network, config, f"{i}steps", ".pt", save_weight_dtype)
    if save_file and rank == 0:
        train_common.save_checkpoint(network, config, "last", ".pt", save_weight_dtype)
    network.fused_stepper = stepper  # the run's SliderStep (None: autograd loop), e.g. for prodigy_d()
    return network


def main(args):
    config = config_util.load_config_from_yaml(args.config_file)
    attributes = train_common.apply_cli_overrides(config, args)
    prompts = prompt_util.load_prompts_from_yaml(config.prompts_file, attributes)
    device = train_common.launch_device(args)
    train(config, prompts, device, fused_step=args.fused_step, dedup_uncond=not args.no_dedup_uncond)


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--config_file", required=False, default="data/config.yaml")
    parser.add_argument("--alpha", type=float, required=True, help="LoRA weight.")
    parser.add_argument("--rank", type=int, required=False, default=4, help="Rank of LoRA.")
    parser.add_argument("--device", required=False, default=0, help="Device to train on.")
    parser.add_argument("--name", type=str, required=False, default=None, help="Name of the slider.")
    parser.add_argument("--attributes", type=str, required=False, default=None,
                        help="attritbutes to disentangle (comma seperated string)")
    add_fused_step_flags(parser)
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
