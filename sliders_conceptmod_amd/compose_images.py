"""Composed slider grids: `generate_images` for several sliders at once, every combination of their scales in one UNet
pass per denoising step (compose.SliderStack, train_util.slider_grid_latents).

    python -m sliders_conceptmod_amd.compose_images --model_name out/age.pt --model_name out/smile.pt \\
        --scales=-2,0,2 --scales=0,1,2 --prompts_path prompts.csv --save_path images \\
        --pretrained_model /models/sd-1.4 --base 1.4

The flags are those of `generate_images`, except that `--model_name` may be repeated (or given as a comma list) and
`--scales` is given once per slider (a single `--scales` applies to all of them); `--max_batch` bounds the UNet batch of a
pass.  Writes {save_path}/{nameA}+{nameB}/{sA}_{sB}/{case}_{num}.png (`scale_str` naming) and
{save_path}/{nameA}+{nameB}/all/{case}_{num}.png: for two sliders the 2-D grid image, rows for slider A and columns for
slider B; for any other count a strip of the cells in row-major order.  SD-1.x and SD-XL, with the defaults of
`generate_images` for the scheduler, `start_noise` and the VAE dtype.

Differences from running the eval script K times, or once per cell:
  * the sliders act TOGETHER, each at its own scale, as two LoRANetworks attached to one UNet do in the reference; K runs of
    the eval script never show a combination;
  * the steps above `start_noise` run once per prompt row, not once per cell: with the adaptor off they are the same
    computation for every cell;
  * below `start_noise` all cells of a chunk share one UNet pass (batch cells x num_samples x 2); with a scheduler that
    draws noise per step (ddpm, euler_a) a cell therefore does not see the noise it would see on its own -- the defaults
    (lms, ddim) are deterministic and give every cell exactly its own result;
  * a cell whose scales are all 0 is the adaptor-off image bit for bit, as scale 0 is in `generate_images`;
  * stacks with conv (c3lier) sites run one cell per pass (their scales are folded into lora_up);
  * rank, alpha and train method are read from each file, as in `generate_images`; DoRA files are refused.
"""
from __future__ import annotations

import argparse
import itertools
import os
from typing import List, Sequence, Tuple

import torch

from . import generate_images as G
from . import model_util, train_util
from .compose import SliderStack


def split_names(values: Sequence[str]) -> List[str]:
    """--model_name given several times and / or as comma lists -> the slider files in order."""
    out = []
    for v in values:
        out.extend(p.strip() for p in str(v).split(",") if p.strip())
    return out


def scale_lists(values: Sequence[str], n_sliders: int) -> List[List[float]]:
    """--scales once per slider; a single --scales applies to every slider."""
    lists = [G.parse_scales(v) for v in values]
    if len(lists) == 1:
        lists = lists * n_sliders
    if len(lists) != n_sliders:
        raise ValueError(f"--scales given {len(lists)} times for {n_sliders} sliders (give it once, or once per slider)")
    if any(not l for l in lists):
        raise ValueError("--scales: an empty list")
    return lists


def grid_cells(lists: Sequence[Sequence[float]]) -> List[Tuple[float, ...]]:
    """Every combination of the sliders' scales, the last slider varying fastest (row-major: rows slider A, columns B)."""
    return list(itertools.product(*lists))


def stack_name(names: Sequence[str]) -> str:
    return "+".join(os.path.splitext(os.path.basename(n))[0] for n in names)


def cell_str(cell: Sequence[float]) -> str:
    return "_".join(G.scale_str(s) for s in cell)


def output_paths(save_path: str, names: Sequence[str], cells, case_number: int, num: int) -> Tuple[List[str], str]:
    folder = os.path.join(save_path, stack_name(names))
    per_cell = [os.path.join(folder, cell_str(c), f"{case_number}_{num}.png") for c in cells]
    return per_cell, os.path.join(folder, "all", f"{case_number}_{num}.png")


def grid_image(images, n_cols: int):
    """Row-major cells -> one image of n_cols columns (n_cols = len(images): a strip)."""
    from PIL import Image
    rows = [images[i:i + n_cols] for i in range(0, len(images), n_cols)]
    strips = [G.strip(r) for r in rows]
    out = Image.new("RGB", (max(s.width for s in strips), sum(s.height for s in strips)))
    y = 0
    for s in strips:
        out.paste(s, (0, y))
        y += s.height
    return out


def generate(args) -> List[str]:
    from PIL import Image
    xl = args.base == "xl"
    device = torch.device(args.device if not str(args.device).isdigit() else f"cuda:{args.device}")
    if device.type != "cuda":
        raise ValueError("the product path has no CPU fallback: pass a cuda device")
    names = split_names(args.model_name)
    lists = scale_lists(args.scales or ["-2,-1,0,1,2"], len(names))
    cells = grid_cells(lists)
    unet_dtype = torch.float16
    vae_dtype = G.DTYPES[args.vae_dtype] if args.vae_dtype else (torch.bfloat16 if xl else torch.float16)
    scheduler_name = args.scheduler or ("ddim" if xl else "lms")
    start_noise = args.start_noise if args.start_noise is not None else (750 if xl else 850)
    tokenizers, text_encoders, unet, scheduler = model_util.load_models(args.pretrained_model, scheduler_name,
                                                                        weight_dtype=unet_dtype, xl=xl)
    unet = unet.to(device, unet_dtype).requires_grad_(False).eval()
    if isinstance(text_encoders, (list, tuple)):
        for te in text_encoders:
            te.to(device, unet_dtype)
    stack = SliderStack(unet, names)
    if args.rank is not None and any(r != args.rank for r in stack.ranks):
        raise ValueError(f"--rank {args.rank} but the LoRA files have ranks {stack.ranks}")
    vae = model_util.load_vae_decoder(args.pretrained_model, xl=xl).to(device, vae_dtype)
    factor = 2 ** (len(vae.config.block_out_channels) - 1)
    folder = os.path.join(args.save_path, stack_name(names))
    for d in [cell_str(c) for c in cells] + ["all"]:
        os.makedirs(os.path.join(folder, d), exist_ok=True)
    h = w = args.image_size
    n_cols = len(lists[1]) if len(names) == 2 else len(cells)
    written = []
    for row in G.read_prompts(args.prompts_path):
        case = row["case_number"]
        if not (args.from_case <= case <= args.till_case):
            continue
        te, added = G.prompt_conditioning(text_encoders, tokenizers, row["prompt"], args.negative_prompts,
                                          args.num_samples, xl, h, w, device, unet_dtype)
        scheduler.set_timesteps(args.ddim_steps)
        lat = G.initial_latents(row["evaluation_seed"], args.num_samples, h, w, scheduler, vae.config.latent_channels,
                                factor).to(device)
        lats = train_util.slider_grid_latents(unet, stack, scheduler, lat, te, cells, start_noise, args.guidance_scale,
                                              args.ddim_steps, added_cond=added, max_batch=args.max_batch)
        images = []  # [cell][num] -> PIL
        for i in range(len(cells)):
            rgb = vae.decode_to_uint8(lats[i].float() / vae.config.scaling_factor).cpu().numpy()
            images.append([Image.fromarray(rgb[k]) for k in range(rgb.shape[0])])
        for num in range(args.num_samples):
            per_cell, all_path = output_paths(args.save_path, names, cells, case, num)
            for i, p in enumerate(per_cell):
                images[i][num].save(p)
                written.append(p)
            grid_image([images[i][num] for i in range(len(cells))], n_cols).save(all_path)
            written.append(all_path)
    return written


def build_parser():
    p = argparse.ArgumentParser(prog="python -m sliders_conceptmod_amd.compose_images",
                                description="Generate composed slider grids: several sliders, every combination of their "
                                            "scales, on the MI355X.")
    p.add_argument("--model_name", required=True, action="append",
                   help="LoRA file (.pt / .safetensors); repeat the flag, or give a comma list, for several sliders")
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
    p.add_argument("--rank", type=int, default=None, help="optional check: the ranks are read from the files")
    p.add_argument("--start_noise", type=int, default=None, help="default 850 (SD-1.x) / 750 (SD-XL)")
    p.add_argument("--scales", action="append", default=None,
                   help="comma-separated scales, once per slider in --model_name order (a single --scales applies to "
                        "all; default -2,-1,0,1,2); write --scales=-1,0,1 (a leading '-' would otherwise read as an option)")
    p.add_argument("--scheduler", default=None, choices=["lms", "ddim", "ddpm", "euler_a"],
                   help="default lms (SD-1.x, as the eval script) / ddim (SD-XL)")
    p.add_argument("--vae_dtype", default=None, choices=sorted(G.DTYPES),
                   help="decoder storage type: default fp16 (SD-1.x) / bf16 (SD-XL)")
    p.add_argument("--max_batch", type=int, default=16,
                   help="largest UNet batch of a pass (cells x num_samples x 2): the grid runs in chunks of cells; the engine's "
                        "workspace grows with it (DESIGN.md section 14: 11.8 GB per sample at SD-XL 1024^2)")
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
