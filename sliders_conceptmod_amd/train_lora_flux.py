"""Text-slider trainer for Flux on the native transformer (conceptmod/textsliders/train_lora_flux.py, restated from its
behaviour): five prompts encoded once as PromptEmbedsSD3; per iteration a prompt pair, `timesteps_to = 0` of an 8-step
schedule, the pre-roll `diffusion_flux` under the adaptor (no step at timesteps_to 0: it sets the schedule), the positive,
neutral and negative steps from the same latents with the network off -- ONE transformer pass per prompt, no CFG pair --,
one adapted step under autograd, `PromptEmbedsPair.loss` on the STEPPED latents, gradients accumulated over
ceil(8 / batch_size) iterations, clip_grad_value_ 1.0, AdamW(lr 1e-4, wd 1e-6), CosineAnnealingLR(T_max 50, eta_min 1e-6),
`<name>_<i>steps.safetensors` / `<name>_last.safetensors`.  LoRANetwork(target_replace=["Attention"], delimiter="-").

    python -m sliders_conceptmod_amd.train_lora_flux --config_file data/config-flux.yaml --alpha 1 --rank 4 --device 0 --name x

The adapted step runs through the trainable Flux engine (`FluxTransformer2DModel.forward` with grad enabled: a saved forward
and `smi_flux_backward`; gradients reach the LoRA matrices only).  Clip + optimiser: the native fused step where
train_common.step_choice allows it -- the accumulated gradient is clamped to [-1, 1] first, which is clip_grad_value_, and the
native step runs without its norm clip --, else (`--no_fused_step`) torch's clip_grad_value_ and optimiser class.

What differs from the reference script, on purpose:
  * the three frozen steps share one no-grad pass of 3 x batch_size samples (positive, neutral, negative): a sample has the
    same bits alone or in a batch, as in train_lora_sd3;
  * the initial noise is drawn on the CPU from torch's seeded generator (the reference draws on the device);
  * the gradients of all ceil(8 / batch_size) iterations of a group reach the optimiser: the reference zeroes the gradient
    just before the group's LAST backward, so only that one does.  The loop runs iterations x ceil(8 / batch_size) times (the
    reference one more, which never reaches the optimiser unless batch_size >= 8); checkpoints are due by optimiser step;
  * `--peft_type dora` and `network.type: c3lier` are refused by name: the engine takes plain Linear LoRA sites on the
    attention projections; `--context_stream` adds the context stream's add_q_proj / add_k_proj / add_v_proj / to_add_out;
  * `train_lora` writes its prompts file to a path given by the caller or to a temporary file, never into `data/`;
  * latents stay fp32 between the steps (the engine's output type), as in train_lora_sd3."""
import argparse
import os
import tempfile

import torch
import yaml
from tqdm import tqdm

from . import config_util, model_util, prompt_util, train_common, train_util
from .config_util import RootConfig
from .lora import LoRANetwork
from .prompt_util import PromptEmbedsCache, PromptEmbedsPair, PromptEmbedsSD3

NUM_IMAGES_PER_PROMPT = 1
CLIP_VALUE = 1.0
NUM_INFERENCE_STEPS = 8
TIMESTEPS_TO = 0
ACCUMULATE_TO = 8  # samples per optimiser step


def check_supported(config: RootConfig, peft_type: str) -> None:
    """The refusals, by name, before anything is loaded."""
    if peft_type == "dora":
        raise ValueError("--peft_type dora: DoRA on the Flux transformer is not built (the engine takes plain LoRA sites)")
    if peft_type != "lora":
        raise ValueError(f"peft_type must be lora, got {peft_type}")
    if config.network.type == "c3lier":
        raise ValueError("network.type c3lier: the Flux transformer has no conv layers to adapt; use network.type lierla")


def accumulation_steps(batch_size: int) -> int:
    """ceil(8 / batch_size) below 8 samples, else 1 (the reference's rule)."""
    return -(-ACCUMULATE_TO // batch_size) if batch_size < ACCUMULATE_TO else 1


def frozen_steps(transformer, scheduler, timestep, latents, pair: PromptEmbedsPair, bs: int, guidance_scale: float):
    """(positive, neutral, negative) stepped latents of three `predict_noise_flux` calls with the network off, from ONE pass
    of 3 x bs samples: one transformer pass per prompt, no CFG pair."""
    embs = (pair.positive, pair.neutral, pair.negative)
    ctx = torch.cat([e.text_embeds.repeat_interleave(bs, dim=0) for e in embs])
    pooled = torch.cat([e.pooled_embeds.repeat_interleave(bs, dim=0) for e in embs])
    n = 3 * latents.shape[0]
    with torch.no_grad():
        stepped = train_util.predict_noise_flux(None, transformer, scheduler, timestep, torch.cat([latents] * 3), ctx, pooled,
                                                guidance_scale=guidance_scale, multipliers=[0.0] * n)
        return tuple(stepped.chunk(3))


def train(config: RootConfig, prompts: list, device, on_step_complete=None, peft_type="lora", rank=4, save_file=True,
          models=None, fused_step=None, optimizer_kwargs=None, optimizer=None, context_stream=False, t5_tokens=512,
          t5_backend="torch"):
    """The reference's `train(config, prompts, device, on_step_complete, peft_type, rank, save_file)`; the other arguments
    are this package's (train_lora_sd3.train): `models` a preloaded load_models_flux tuple, `fused_step` / `optimizer` /
    `optimizer_kwargs` the optimiser choice, `context_stream` the form with the context stream's modules, `t5_tokens` the
    sequence length of the T5 block (zero rows where the model was loaded without the tower), `t5_backend` torch | native
    (model_util.load_models_flux; not used with preloaded `models`).  Left on the network:
    `training_losses` (per iteration, unscaled), `flat_sums` (the flat parameter's sum after every iteration: it moves only
    where the optimiser stepped), `optimizer_steps`, and `first_step`, iteration 0's draws (latents, gradient of
    loss / accumulation steps) for the parity test."""
    check_supported(config, peft_type)
    weight_dtype = config_util.parse_precision(config.train.precision)
    save_weight_dtype = config_util.parse_precision(config.train.precision)
    guidance_scale = config.train.cfg
    tokenizers, text_encoders, transformer, noise_scheduler = models or model_util.load_models_flux(
        config.pretrained_model.name_or_path, weight_dtype=weight_dtype, t5_backend=t5_backend)
    for te in text_encoders:  # (the stand-in towers of a synthetic:// model are no nn.Modules: nothing to freeze)
        if te is None:
            continue
        te.to(device, weight_dtype)
        if isinstance(te, torch.nn.Module):
            te.requires_grad_(False).eval()
    transformer.to(device, dtype=weight_dtype).requires_grad_(False).eval()
    network = LoRANetwork(transformer, rank=rank, multiplier=1.0, delimiter="-", target_replace=["Attention"],
                          train_method=config.network.training_method, context_stream=context_stream).to(device, dtype=weight_dtype)
    if optimizer is None:
        optimizer_name = "adamw"
        okw = dict(lr=1e-4, weight_decay=1e-6)
        okw.update(optimizer_kwargs or {})
        optimizer = torch.optim.AdamW(network.parameters(), **okw)
    else:
        optimizer_name = optimizer
        okw = dict(optimizer_kwargs or {})
        optimizer = train_util.get_optimizer(optimizer_name)(network.parameters(), **okw)
        okw.setdefault("lr", optimizer.defaults["lr"])
    fused, spec = train_common.step_choice(fused_step, optimizer_name, okw)
    lr_scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=50, eta_min=1e-6)
    criteria = torch.nn.MSELoss()

    cache = PromptEmbedsCache()
    prompt_pairs = []
    jd = transformer.cfg.joint_attention_dim
    with torch.no_grad():
        for settings in prompts:
            for prompt in [settings.target, settings.positive, settings.neutral, settings.unconditional, settings.negative]:
                if prompt is not None and cache[prompt] is None:
                    te, pooled = train_util.encode_prompts_flux(None, tokenizers, text_encoders, prompt, NUM_IMAGES_PER_PROMPT,
                                                                t5_tokens, jd)
                    cache[prompt] = PromptEmbedsSD3(te.to(device, weight_dtype), pooled.to(device, weight_dtype))
            neg = cache[settings.negative] if settings.negative is not None else None
            prompt_pairs.append(PromptEmbedsPair(criteria, cache[settings.target], cache[settings.positive],
                                                 cache[settings.unconditional], cache[settings.neutral], neg, settings))
    del tokenizers, text_encoders

    tail = None
    if fused:  # the native optimiser step on the flat parameter (step._FusedStep owns the optimiser state); no norm clip
        from .step import _FusedStep
        tail = _FusedStep(transformer, network, noise_scheduler, 1, okw["lr"], (0.9, 0.999), 1e-8, 0.0, 0.0, None, spec)
    acc = accumulation_steps(prompts[0].batch_size) if prompts else 1
    network.training_losses, network.flat_sums, network.optimizer_steps = [], [], 0
    network.first_step = None
    optimizer.zero_grad()
    for i in tqdm(range(config.train.iterations * acc)):
        with torch.no_grad():
            prompt_pair = prompt_pairs[torch.randint(0, len(prompt_pairs), (1,)).item()]
            height, width = prompt_pair.resolution, prompt_pair.resolution
            if prompt_pair.dynamic_resolution:
                height, width = train_util.get_random_resolution_in_bucket(prompt_pair.resolution)
            bs = prompt_pair.batch_size
            latents = train_util.get_initial_latents_flux(noise_scheduler, bs, height, width, 1).to(device, torch.float32)
            with network:  # the pre-roll under the adaptor: at timesteps_to 0 it sets the schedule and takes no step
                denoised_latents = train_util.diffusion_flux(
                    None, transformer, noise_scheduler, latents,
                    prompt_pair.unconditional.text_embeds.repeat_interleave(bs, dim=0),
                    prompt_pair.unconditional.pooled_embeds.repeat_interleave(bs, dim=0), start_timesteps=0,
                    total_timesteps=TIMESTEPS_TO, guidance_scale=guidance_scale, num_inference_steps=NUM_INFERENCE_STEPS)
            current_timestep = noise_scheduler.timesteps[TIMESTEPS_TO]
            positive_latents, neutral_latents, negative_latents = frozen_steps(
                transformer, noise_scheduler, current_timestep, denoised_latents, prompt_pair, bs, guidance_scale)
        with network:
            target_latents = train_util.predict_noise_flux(
                None, transformer, noise_scheduler, current_timestep, denoised_latents,
                prompt_pair.target.text_embeds.repeat_interleave(bs, dim=0),
                prompt_pair.target.pooled_embeds.repeat_interleave(bs, dim=0), guidance_scale=guidance_scale)
        loss = prompt_pair.loss(target_latents=target_latents, positive_latents=positive_latents,
                                neutral_latents=neutral_latents, negative_latents=negative_latents)
        (loss / acc if acc > 1 else loss).backward()
        if i == 0:
            network.first_step = dict(latents=latents.cpu(), timesteps_to=TIMESTEPS_TO, timestep=float(current_timestep),
                                      grad=network.flat.grad.detach().clone().cpu(), loss=float(loss.item()),
                                      accumulation_steps=acc)
        stepped = (i + 1) % acc == 0
        if stepped:
            if tail is not None:
                torch.clamp(network.flat.grad, -CLIP_VALUE, CLIP_VALUE, out=tail.grad)
                tail._optimizer_tail(lr_scheduler.get_last_lr()[0])
                network.flat.grad = None
                optimizer.step()  # no gradients: a no-op that keeps torch's "optimizer before scheduler" order
            else:
                torch.nn.utils.clip_grad_value_(network.parameters(), clip_value=CLIP_VALUE)
                optimizer.step()
            lr_scheduler.step()
            optimizer.zero_grad()
            network.optimizer_steps += 1
        network.training_losses.append(float(loss.item()))
        network.flat_sums.append(float(network.flat.detach().double().sum().item()))
        if stepped:
            step = (i + 1) // acc
            if save_file and train_common.checkpoint_due(step, config):
                train_common.save_checkpoint(network, config, f"{step}steps", ".safetensors", save_weight_dtype)
            if on_step_complete is not None:
                on_step_complete(step)
    if save_file:
        train_common.save_checkpoint(network, config, "last", ".safetensors", save_weight_dtype)
        return network
    return network.get_state_dict(save_weight_dtype)


def train_lora(target, positive, negative, unconditional, alpha=1.0, device=0, name=None, attributes=None, batch_size=1,
               config_file="data/config-flux.yaml", resolution=512, steps=None, on_step_complete=None, peft_type="lora", rank=4,
               save_file=False, models=None, prompts_file=None, **train_kwargs):
    """Programmatic entry (the reference's train_lora): the prompt settings written as a one-entry prompts file (neutral =
    target, action enhance) to `prompts_file`, or to a temporary file that is removed again, and read back through
    prompt_util.load_prompts_from_yaml, as the reference does through data/prompts-flux.yaml."""
    config = config_util.load_config_from_yaml(config_file)
    if steps is not None:
        config.train.iterations = steps
    attr_list = train_common.apply_cli_overrides(config, argparse.Namespace(name=name, alpha=alpha, rank=rank, attributes=attributes))
    entry = {"target": target, "positive": positive, "negative": negative, "unconditional": unconditional, "neutral": target,
             "action": "enhance", "guidance_scale": 1, "resolution": resolution, "dynamic_resolution": False,
             "batch_size": batch_size}
    path, temporary = prompts_file, prompts_file is None
    if temporary:
        fd, path = tempfile.mkstemp(suffix=".yaml", prefix="prompts-flux-")
        os.close(fd)
    try:
        with open(path, "w") as fh:
            yaml.safe_dump([entry], fh)
        prompts = prompt_util.load_prompts_from_yaml(path, attr_list)
    finally:
        if temporary:
            os.remove(path)
    dev = torch.device(f"cuda:{device}") if not isinstance(device, torch.device) else device
    return train(config, prompts, dev, on_step_complete, peft_type, rank, save_file, models, **train_kwargs)


def main(args):
    config = config_util.load_config_from_yaml(args.config_file)
    attributes = train_common.apply_cli_overrides(config, args)
    check_supported(config, args.peft_type)
    prompts = prompt_util.load_prompts_from_yaml(config.prompts_file, attributes)
    device = train_common.launch_device(args)
    return train(config, prompts, device, None, args.peft_type, args.rank, True, None, args.fused_step,
                 optimizer=args.optimizer, context_stream=args.context_stream, t5_tokens=args.t5_tokens,
                 t5_backend=args.t5_backend)


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--config_file", required=False, default="data/config-flux.yaml")
    parser.add_argument("--alpha", type=float, required=True, help="LoRA weight.")
    parser.add_argument("--rank", type=int, required=False, default=4, help="Rank of LoRA.")
    parser.add_argument("--device", required=False, default=0, help="Device to train on.")
    parser.add_argument("--name", type=str, required=False, default=None, help="Name of the slider.")
    parser.add_argument("--attributes", type=str, required=False, default=None)
    parser.add_argument("--peft_type", type=str, required=False, default="lora", help="lora (dora is refused)")
    parser.add_argument("--context_stream", action="store_true",
                        help="also adapt the context stream's add_q_proj / add_k_proj / add_v_proj / to_add_out")
    parser.add_argument("--t5_tokens", type=int, default=512,
                        help="sequence length of the T5 block of the prompt embedding (zero rows without the tower)")
    parser.add_argument("--t5_backend", choices=["torch", "native"], default="torch",
                        help="the T5 tower as transformers runs it (torch) or on the HIP engine (native)")
    parser.add_argument("--optimizer", type=str, required=False, default=None,
                        help="adam, adamw, lion or prodigy at the class's own defaults instead of the script's hard-coded "
                             "AdamW(lr 1e-4, weight_decay 1e-6)")
    train_common.add_fused_step_flags(parser)
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
