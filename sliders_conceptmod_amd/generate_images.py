"""Slider image sweep: the eval scripts' generation loop (eval-scripts/generate_images_sd1.py:145-210,
generate_images_xl.py:327-377) on the HIP engine, from a LoRA file written by this package's trainers to PNG files.

    python -m sliders_conceptmod_amd.generate_images --model_name out/age_slider.pt --prompts_path prompts.csv \\
        --save_path images --pretrained_model /models/sd-1.4 --base 1.4

Per CSV row (prompt, evaluation_seed, case_number) and slider scale: torch.manual_seed(seed), the CPU randn of the
latents, x init_noise_sigma, `train_util.slider_sweep_latents` (adaptor off while t > start_noise), then
`vae.decode_to_uint8(latents / scaling_factor)`.  Writes {save_path}/{name}/{scale_str}/{case}_{num}.png (0.5 -> "half")
and a horizontal strip of all scales to {save_path}/{name}/all/{case}_{num}.png.

Differences from the eval scripts, on purpose: rank, alpha and the train method are read from the LoRA file (its
lora_down shapes, its `.alpha` entries, its key set matched against LoRANetwork for each train method) instead of being
guessed from folder names; `--image_size` is honoured (the SD-1.x script overrides it with 512); SD-XL samples with DDIM
by default (the pipeline's EulerDiscrete is not a native scheduler); the VAE decodes in `--vae_dtype` (bf16 for SD-XL:
its decoder overflows fp16 and this engine has no fp32 path); the `all/` strip is a plain PIL image, not a matplotlib
figure."""
from __future__ import annotations

import argparse
import csv
import os
from typing import Dict, List, Optional, Tuple

import torch

from . import lora as LM
from . import model_util, train_util

TRAIN_METHODS = ("noxattn", "innoxattn", "selfattn", "xattn", "full", "xattn-strict", "noxattn-hspace",
                 "noxattn-hspace-last")
DTYPES = {"fp16": torch.float16, "float16": torch.float16, "bf16": torch.bfloat16, "bfloat16": torch.bfloat16}


def scale_str(scale: float) -> str:
    """Folder name of a slider scale, as the eval scripts write it (`f'{scale}'` with 0.5 -> 'half')."""
    return f"{scale}".replace("0.5", "half")


def parse_scales(text: str) -> List[float]:
    out = []
    for part in text.split(","):
        part = part.strip()
        if part:
            v = float(part)
            out.append(int(v) if v.is_integer() else v)
    return out


def read_prompts(path: str) -> List[Dict]:
    """The eval CSV: columns prompt, evaluation_seed, case_number (any others are ignored)."""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            r = {(k or "").strip(): v for k, v in r.items()}
            rows.append({"prompt": str(r["prompt"]), "evaluation_seed": int(float(r["evaluation_seed"])),
                         "case_number": int(float(r["case_number"]))})
    return rows


def output_paths(save_path: str, name: str, scales, case_number: int, num: int) -> Tuple[List[str], str]:
    folder = os.path.join(save_path, name)
    per_scale = [os.path.join(folder, scale_str(s), f"{case_number}_{num}.png") for s in scales]
    return per_scale, os.path.join(folder, "all", f"{case_number}_{num}.png")


def load_lora_state(path: str) -> Dict[str, torch.Tensor]:
    if os.path.splitext(path)[1] == ".safetensors":
        from safetensors.torch import load_file
        return load_file(path)
    return torch.load(path, map_location="cpu", weights_only=True)


def lora_file_params(state: Dict[str, torch.Tensor], unet) -> Tuple[int, float, str, list]:
    """(rank, alpha, train_method, target_replace) of a LoRA state dict written by LoRANetwork.save_weights: rank from
    the lora_down shapes, alpha from the `.alpha` entries, the train method (and whether conv layers are adapted) from
    the key set, matched against the networks each method builds on `unet`.  Methods with equal key sets build the same
    network; the first in TRAIN_METHODS is returned."""
    downs = {k: v for k, v in state.items() if k.endswith(".lora_down.weight")}
    if not downs:
        raise ValueError("not a LoRA file: no '*.lora_down.weight' entries")
    ranks = {int(v.shape[0]) for v in downs.values()}
    if len(ranks) != 1:
        raise ValueError(f"LoRA file mixes ranks {sorted(ranks)}")
    alphas = {float(v) for k, v in state.items() if k.endswith(".alpha")}
    if len(alphas) > 1:
        raise ValueError(f"LoRA file mixes alphas {sorted(alphas)}")
    alpha = alphas.pop() if alphas else float(ranks.copy().pop())
    names = {k[:-len(".lora_down.weight")] for k in downs}
    for target_replace in (LM.DEFAULT_TARGET_REPLACE, LM.DEFAULT_TARGET_REPLACE + LM.UNET_TARGET_REPLACE_MODULE_CONV):
        for method in TRAIN_METHODS:
            got = {t[0] for t in LM.select_targets(unet, method, target_replace, LM.LORA_PREFIX_UNET, "_")}
            if got == names:
                return ranks.pop(), alpha, method, list(target_replace)
    raise ValueError("the LoRA file's layers match no train method of this UNet (wrong --base or --pretrained_model?)")


def load_lora_network(unet, path: str, device):
    state = load_lora_state(path)
    rank, alpha, method, target_replace = lora_file_params(state, unet)
    net = LM.LoRANetwork(unet, rank=rank, multiplier=1.0, alpha=alpha, train_method=method,
                         target_replace=target_replace).to(device)
    net.load_state_dict(state)
    return net


def prompt_conditioning(text_encoders, tokenizers, prompt: str, negative: Optional[str], batch: int, xl: bool,
                        height: int, width: int, device, dtype):
    """cat([uncond, cond]) embeddings of a batch (and, for SD-XL, the added conditioning pair)."""
    neg = negative if negative is not None else ""
    if xl:
        from .train_lora_xl import encode_xl
        c, u = (encode_xl(text_encoders, tokenizers, p, device, dtype) for p in (prompt, neg))
        te = train_util.concat_embeddings(u.text_embeds, c.text_embeds, batch)
        pooled = train_util.concat_embeddings(u.pooled_embeds, c.pooled_embeds, batch)
        tid = train_util.get_add_time_ids(height, width, dtype=torch.float32).to(device)
        return te, (pooled, tid.repeat(2 * batch, 1))
    from .train_lora import encode
    c, u = (encode(text_encoders, tokenizers, p, device, dtype) for p in (prompt, neg))
    return train_util.concat_embeddings(u, c, batch), None


def initial_latents(seed: int, batch: int, height: int, width: int, scheduler, latent_channels: int = 4,
                    factor: int = 8) -> torch.Tensor:
    """torch.manual_seed(seed), then the CPU randn of the latents, then x init_noise_sigma (E/generate_images_sd1.py:149,
    172-179)."""
    generator = torch.manual_seed(seed)
    lat = torch.randn((batch, latent_channels, height // factor, width // factor), generator=generator)
    return lat * scheduler.init_noise_sigma


def strip(images) -> "Image.Image":
    from PIL import Image
    w = sum(im.width for im in images)
    out = Image.new("RGB", (w, max(im.height for im in images)))
    x = 0
    for im in images:
        out.paste(im, (x, 0))
        x += im.width
    return out


def generate(args) -> List[str]:
    from PIL import Image
    xl = args.base == "xl"
    device = torch.device(args.device if not str(args.device).isdigit() else f"cuda:{args.device}")
    if device.type != "cuda":
        raise ValueError("the product path has no CPU fallback: pass a cuda device")
    unet_dtype = torch.float16
    vae_dtype = DTYPES[args.vae_dtype] if args.vae_dtype else (torch.bfloat16 if xl else torch.float16)
    scheduler_name = args.scheduler or ("ddim" if xl else "lms")
    start_noise = args.start_noise if args.start_noise is not None else (750 if xl else 850)
    tokenizers, text_encoders, unet, scheduler = model_util.load_models(args.pretrained_model, scheduler_name,
                                                                        weight_dtype=unet_dtype, xl=xl)
    unet = unet.to(device, unet_dtype).requires_grad_(False).eval()
    if isinstance(text_encoders, (list, tuple)):
        for te in text_encoders:
            te.to(device, unet_dtype)
    network = load_lora_network(unet, args.model_name, device)
    if args.rank is not None and args.rank != network.lora_dim:
        raise ValueError(f"--rank {args.rank} but the LoRA file has rank {network.lora_dim}")
    vae = model_util.load_vae_decoder(args.pretrained_model, xl=xl).to(device, vae_dtype)
    factor = 2 ** (len(vae.config.block_out_channels) - 1)
    scales = parse_scales(args.scales)
    name = os.path.splitext(os.path.basename(args.model_name))[0]
    folder = os.path.join(args.save_path, name)
    for d in [scale_str(s) for s in scales] + ["all"]:
        os.makedirs(os.path.join(folder, d), exist_ok=True)
    h = w = args.image_size
    written = []
    for row in read_prompts(args.prompts_path):
        case = row["case_number"]
        if not (args.from_case <= case <= args.till_case):
            continue
        te, added = prompt_conditioning(text_encoders, tokenizers, row["prompt"], args.negative_prompts,
                                        args.num_samples, xl, h, w, device, unet_dtype)
        images = []  # [scale][num] -> PIL
        for scale in scales:
            scheduler.set_timesteps(args.ddim_steps)
            lat = initial_latents(row["evaluation_seed"], args.num_samples, h, w, scheduler,
                                  vae.config.latent_channels, factor).to(device)
            lat = train_util.slider_sweep_latents(unet, network, scheduler, lat, te, scale, start_noise,
                                                  args.guidance_scale, args.ddim_steps, added_cond=added)
            rgb = vae.decode_to_uint8(lat.float() / vae.config.scaling_factor).cpu().numpy()
            images.append([Image.fromarray(rgb[i]) for i in range(rgb.shape[0])])
        for num in range(args.num_samples):
            per_scale, all_path = output_paths(args.save_path, name, scales, case, num)
            for i, p in enumerate(per_scale):
                images[i][num].save(p)
                written.append(p)
            strip([images[i][num] for i in range(len(scales))]).save(all_path)
            written.append(all_path)
    return written


def build_parser():
    p = argparse.ArgumentParser(prog="python -m sliders_conceptmod_amd.generate_images",
                                description="Generate slider sweeps (eval-scripts/generate_images_*.py) on the MI355X.")
    p.add_argument("--model_name", required=True, help="LoRA file (.pt / .safetensors) written by the trainers")
    p.add_argument("--prompts_path", required=True, help="CSV with prompt, evaluation_seed, case_number")
    p.add_argument("--save_path", required=True, help="output folder")
    p.add_argument("--pretrained_model", default="synthetic://sd1x",
                   help="local diffusers directory or synthetic://(tiny_)sd1x | sdxl")
    p.add_argument("--negative_prompts", default=None, help="negative prompt (default: the empty prompt)")
    p.add_argument("--base", choices=["1.4", "xl"], default="1.4")
    p.add_argument("--guidance_scale", type=float, default=7.5)
    p.add_argument("--image_size", type=int, default=None, help="default 512 (SD-1.x) / 1024 (SD-XL)")
    p.add_argument("--from_case", type=int, default=0)
    p.add_argument("--till_case", type=int, default=1000000)
    p.add_argument("--num_samples", type=int, default=5)
    p.add_argument("--ddim_steps", type=int, default=50)
    p.add_argument("--rank", type=int, default=None, help="optional check: the rank is read from the file")
    p.add_argument("--start_noise", type=int, default=None, help="default 850 (SD-1.x) / 750 (SD-XL)")
    p.add_argument("--scales", default="-2,-1,0,1,2", help="comma-separated; write --scales=-1,0,1 (a leading '-' "
                   "would otherwise read as an option)")
    p.add_argument("--scheduler", default=None, choices=["lms", "ddim", "ddpm", "euler_a"],
                   help="default lms (SD-1.x, as the eval script) / ddim (SD-XL)")
    p.add_argument("--vae_dtype", default=None, choices=sorted(DTYPES),
                   help="decoder storage type: default fp16 (SD-1.x) / bf16 (SD-XL)")
    p.add_argument("--device", default="0")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.image_size is None:
        args.image_size = 1024 if args.base == "xl" else 512
    for path in generate(args):
        print(path)


if __name__ == "__main__":
    main()
