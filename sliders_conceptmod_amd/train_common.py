"""The scaffold the trainer scripts share (train_lora, train_lora_xl, train_lora_scale_xl / train_lora_scale): command-line
overrides, the multi-rank launch, optimiser-argument parsing, the fused-step rule, checkpoints, model placement and the
text trainers' per-step RNG draws.  Plain functions; what differs between the scripts stays in the scripts."""
import ast
import os
from pathlib import Path

import torch

from . import parallel, train_util
from .optim import LION_DEFAULTS, PRODIGY_DEFAULTS, OptimSpec


def apply_cli_overrides(config, args) -> list:
    """--name / --alpha / --rank over the YAML, the reference's output naming (T/train_lora.py:343-359) and the
    --attributes list; returns the attributes."""
    if args.name is not None:
        config.save.name = args.name
    attributes = [a.strip() for a in args.attributes.split(",")] if args.attributes is not None else []
    config.network.alpha = args.alpha
    config.network.rank = args.rank
    config.save.name += f"_alpha{args.alpha}_rank{config.network.rank}_{config.network.training_method}"
    config.save.path += f"/{config.save.name}"
    return attributes


def launch_device(args) -> torch.device:
    """One process per GPU under torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE in the environment): RCCL process
    group, device = LOCAL_RANK; otherwise cuda:<--device>.  `SMI_DIST_BACKEND=gloo` is for rehearsals on a box with
    fewer GPUs than ranks (tests); a process group that already exists is kept."""
    if str(args.device) == "cpu":
        raise ValueError("--device cpu: the product path has no CPU fallback (the CPU oracle lives under oracle/)")
    if "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        backend = os.environ.get("SMI_DIST_BACKEND", "nccl")
        local = int(os.environ.get("LOCAL_RANK", "0")) if backend == "nccl" else int(args.device)
        torch.cuda.set_device(local)
        if not torch.distributed.is_initialized():
            torch.distributed.init_process_group(backend)
        return torch.device("cuda", local)
    return torch.device(f"cuda:{args.device}")


def parse_optimizer_args(s) -> dict:
    """`train.optimizer_args`, "k=v k=v" -> keyword arguments of the optimiser (T/train_lora.py:82-87)."""
    kwargs = {}
    if s is not None and len(s) > 0:
        for arg in s.split(" "):
            key, value = arg.split("=")
            kwargs[key] = ast.literal_eval(value)
    return kwargs


def adam_fusable(optimizer_name: str, kwargs: dict):
    """(whether the native AdamW of the fused step expresses this optimiser, its weight decay).  It does Adam / AdamW with
    decoupled weight decay: `lr`, `weight_decay`, `betas`, `eps` and `amsgrad=False`; torch.optim.Adam's weight decay is
    the coupled (L2) kind, so Adam passes only without one."""
    name = optimizer_name.lower()
    wd = kwargs.get("weight_decay", 1e-2 if name == "adamw" else 0.0)
    unsupported = set(kwargs) - {"lr", "weight_decay", "betas", "eps", "amsgrad"}
    fusable = (name in ("adam", "adamw") and not (name == "adam" and wd != 0.0) and not kwargs.get("amsgrad")
               and not unsupported)
    return fusable, wd


def fused_step_choice(fused_step, optimizer_name: str, kwargs: dict):
    """The trainers' `fused_step` argument -> (run the fused step?, weight decay): None = whenever adam_fusable, True =
    fused or ValueError, False = the reference-style autograd loop."""
    fusable, wd = adam_fusable(optimizer_name, kwargs)
    if fused_step and not fusable:
        raise ValueError("--fused_step implements Adam / AdamW (decoupled weight decay; weight_decay, betas, eps) only")
    return fusable and fused_step is not False, wd


def native_optimizer(optimizer_name: str, kwargs: dict):
    """The optim.OptimSpec of the fused step's native kernel for this optimiser, or None where it has none.  Adam / AdamW:
    the rule of adam_fusable.  Lion / Prodigy: whenever `kwargs` holds only the algorithm's own hyper-parameters
    (optim.LION_DEFAULTS / PRODIGY_DEFAULTS); `fsdp_in_use`, `slice_p` or anything unknown leaves it to the torch class."""
    name = optimizer_name.lower()
    if name in ("lion", "prodigy"):
        return None if _refused_arguments(name, kwargs) else OptimSpec.of(name, kwargs)
    fusable, wd = adam_fusable(optimizer_name, kwargs)
    if not fusable:
        return None
    return OptimSpec.adamw(kwargs.get("betas", (0.9, 0.999)), kwargs.get("eps", 1e-8), wd)


def _refused_arguments(name: str, kwargs: dict) -> list:
    return sorted(set(kwargs) - set(LION_DEFAULTS if name == "lion" else PRODIGY_DEFAULTS))


def step_choice(fused_step, optimizer_name: str, kwargs: dict):
    """The trainers' `fused_step` argument -> (run the fused step?, its optim.OptimSpec or None): None = whenever the
    optimiser has a native kernel (native_optimizer), True = fused or ValueError naming what stands in the way, False = the
    reference-style autograd loop.  Adam / AdamW and every unknown name go through fused_step_choice."""
    name = optimizer_name.lower()
    if name not in ("lion", "prodigy"):
        fused, _ = fused_step_choice(fused_step, optimizer_name, kwargs)
        return fused, (native_optimizer(optimizer_name, kwargs) if fused else None)
    refused = _refused_arguments(name, kwargs)
    if fused_step and refused:
        raise ValueError(f"--fused_step: the native {name} step does not take {', '.join(refused)} "
                         f"(it takes {', '.join(sorted(LION_DEFAULTS if name == 'lion' else PRODIGY_DEFAULTS))})")
    fused = not refused and fused_step is not False
    return fused, (OptimSpec.of(name, kwargs) if fused else None)


def add_fused_step_flags(parser):
    """Shared by the four trainers: the fused step is the default, `--no_fused_step` keeps the reference-style loop."""
    g = parser.add_mutually_exclusive_group()
    g.add_argument("--fused_step", dest="fused_step", action="store_true", default=None,
                   help="insist on the fused step (pre-roll + 4-pass step through step.SliderStep / ImageSliderStep: one "
                        "batched UNet pass, native loss / clip / optimiser, no autograd graph -- the path bench.py "
                        "measures); it is the default whenever the optimiser is Adam / AdamW, Lion or Prodigy")
    g.add_argument("--no_fused_step", dest="fused_step", action="store_false",
                   help="the reference-style loop: one UNet call per guidance pass, torch autograd and optimiser")
    parser.add_argument("--no_dedup_uncond", action="store_true",
                        help="fused step: run the unconditional half of every frozen pass again, as the reference does, "
                             "instead of once (results are bit-identical either way)")


def checkpoint_due(i: int, config) -> bool:
    """Every `save.per_steps` steps, except at step 0 and at the last one, which writes `_last` (T/train_lora.py:317-327)."""
    return i % config.save.per_steps == 0 and i != 0 and i != config.train.iterations - 1


def save_checkpoint(network, config, tag: str, suffix: str, dtype):
    """<save.path>/<save.name>_<tag><suffix>, e.g. tag "500steps" / "last", suffix ".pt" / ".safetensors"."""
    save_path = Path(config.save.path)
    save_path.mkdir(parents=True, exist_ok=True)
    network.save_weights(save_path / f"{config.save.name}_{tag}{suffix}", dtype=dtype)


def place_frozen(text_encoders, unet, device, dtype):
    """The frozen models on the device in the training precision, in eval mode, without gradients."""
    if isinstance(text_encoders, (list, tuple)):
        for te in text_encoders:
            te.to(device, dtype=dtype)
            te.requires_grad_(False)
            te.eval()
    unet.to(device, dtype=dtype)
    unet.requires_grad_(False)
    unet.eval()


def draw_text_step(prompt_pairs, config, noise_scheduler, rank: int, world: int, device):
    """The text trainers' per-step draws, in the reference's order (T/train_lora.py:163-191, T/train_lora_xl.py:173-200):
    the prompt pair, timesteps_to, the resolution bucket if dynamic, the initial latents.  All ranks draw the GLOBAL
    latent batch from the same control RNG and keep their slice.
    Returns (prompt_pair, timesteps_to, height, width, bs of this rank, fp32 latents of this rank on `device`)."""
    prompt_pair = prompt_pairs[torch.randint(0, len(prompt_pairs), (1,)).item()]
    timesteps_to = torch.randint(1, config.train.max_denoising_steps, (1,)).item()
    height, width = prompt_pair.resolution, prompt_pair.resolution
    if prompt_pair.dynamic_resolution:
        height, width = train_util.get_random_resolution_in_bucket(prompt_pair.resolution)
    bs = prompt_pair.batch_size
    latents = train_util.get_initial_latents(noise_scheduler, bs, height, width, 1)
    if world > 1:
        latents = latents[parallel.shard_slice(bs, rank, world)]
        bs = bs // world
    return prompt_pair, timesteps_to, height, width, bs, latents.to(device, dtype=torch.float32)
