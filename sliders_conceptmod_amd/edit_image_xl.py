"""Edit a real image with a trained SD-XL slider: null-text inversion of the image on the SD-XL UNet, then the slider sweep
from the inverted latent with one optimised unconditional embedding -- sequence and pooled -- per step.

    python -m sliders_conceptmod_amd.edit_image_xl --image photo.jpg --prompt "photo of a person" \\
        --model_name out/age_slider_xl.pt --pretrained_model /models/sdxl-base-1.0 --save_path edits --scales=0,2,4

Same flags and outputs as `edit_image` (reconstruction.png, {scale_str}/{image stem}.png per scale, all/{image stem}.png),
without `--base`; `--image_size` defaults to 1024, `--pretrained_model` to synthetic://sdxl, `--vae_dtype` to bf16 (as
`generate_images --base xl`); `--no_null_pooled` optimises the sequence embedding only.

Differences from the notebook (demo_image_editing.ipynb), on top of those `edit_image` lists: the notebook is SD-1.4 only --
the SD-XL route is this package's addition.  Prompts are encoded with both text towers, exactly as `generate_images --base xl`
encodes them; the added conditioning (pooled embedding, time_ids of an uncropped image_size x image_size image) goes
through every UNet call of the inversion and of the sweep; and the null-text optimisation also optimises the unconditional
POOLED embedding (one Adam over both tensors), which the notebook has no counterpart for.  Text-encoder LoRA files are not
taken."""
from __future__ import annotations

import argparse
import os
from typing import List

import torch

from . import generate_images as GI
from . import model_util, train_util
from .edit_image import output_paths, parse_offsets
from .null_inversion_xl import NullInversionXL


def edit(args) -> List[str]:
    from PIL import Image
    device = torch.device(args.device if not str(args.device).isdigit() else f"cuda:{args.device}")
    if device.type != "cuda":
        raise ValueError("the product path has no CPU fallback: pass a cuda device")
    unet_dtype = torch.float16
    vae_dtype = GI.DTYPES[args.vae_dtype] if args.vae_dtype else torch.bfloat16
    tokenizers, text_encoders, unet, scheduler = model_util.load_models(args.pretrained_model, "ddim",
                                                                        weight_dtype=unet_dtype, xl=True)
    unet = unet.to(device, unet_dtype).requires_grad_(False).eval()
    if isinstance(text_encoders, (list, tuple)):
        for te in text_encoders:
            te.to(device, unet_dtype)
    vae = model_util.load_vae(args.pretrained_model, xl=True).to(device, vae_dtype)
    vae_dec = model_util.load_vae_decoder(args.pretrained_model, xl=True).to(device, vae_dtype)
    from .train_lora_xl import encode_xl

    def encode_prompt(p):
        e = encode_xl(text_encoders, tokenizers, p, device, unet_dtype)
        return e.text_embeds, e.pooled_embeds

    inv = NullInversionXL(unet, scheduler, vae, vae_dec, encode_prompt, num_ddim_steps=args.ddim_steps,
                          guidance_scale=args.guidance_scale, fused=not args.unfused, image_size=args.image_size)
    (_image_gt, image_rec), x_t, unconds, pooleds = inv.invert(
        args.image, args.prompt, offsets=parse_offsets(args.offsets), num_inner_steps=args.num_inner_steps,
        early_stop_epsilon=args.early_stop_epsilon, verbose=args.verbose, optimize_pooled=not args.no_null_pooled)
    network = GI.load_lora_network(unet, args.model_name, device)  # after the inversion: that runs without an adaptor
    scales = GI.parse_scales(args.scales)
    name = os.path.splitext(os.path.basename(args.model_name))[0]
    rec_path, per_scale, all_path = output_paths(args.save_path, name, scales, args.image)
    for p in [rec_path, all_path] + per_scale:
        os.makedirs(os.path.dirname(p), exist_ok=True)
    Image.fromarray(image_rec).save(rec_path)
    written = [rec_path]
    te = inv.context.to(unet_dtype)  # cat([uncond, cond]) of the prompt
    added = (inv.pooled.to(unet_dtype), inv.time_ids.repeat(2, 1))
    images = []
    for scale, path in zip(scales, per_scale):
        scheduler.set_timesteps(args.ddim_steps)
        lat = (x_t * scheduler.init_noise_sigma).float()
        lat = train_util.slider_sweep_latents(unet, network, scheduler, lat, te, scale, args.start_noise,
                                              args.guidance_scale, args.ddim_steps, added_cond=added,
                                              uncond_per_step=unconds, uncond_pooled_per_step=pooleds)
        rgb = vae_dec.decode_to_uint8(lat.float() / vae_dec.config.scaling_factor).cpu().numpy()
        images.append(Image.fromarray(rgb[0]))
        images[-1].save(path)
        written.append(path)
    GI.strip(images).save(all_path)
    written.append(all_path)
    return written


def build_parser():
    p = argparse.ArgumentParser(prog="python -m sliders_conceptmod_amd.edit_image_xl",
                                description="Edit a real image with an SD-XL slider (null-text inversion) on the MI355X.")
    p.add_argument("--image", required=True, help="the photograph (any PIL-readable file)")
    p.add_argument("--prompt", required=True, help="a prompt that describes the image")
    p.add_argument("--model_name", required=True, help="LoRA file (.pt / .safetensors) written by the trainers")
    p.add_argument("--save_path", required=True, help="output folder")
    p.add_argument("--pretrained_model", default="synthetic://sdxl",
                   help="local diffusers directory or synthetic://(tiny_)sdxl")
    p.add_argument("--scales", default="0,2,4", help="comma-separated; write --scales=-1,0,1 for negative values")
    p.add_argument("--start_noise", type=int, default=500,
                   help="the adaptor is off while t > start_noise (small values keep the identity)")
    p.add_argument("--ddim_steps", type=int, default=50)
    p.add_argument("--guidance_scale", type=float, default=7.5)
    p.add_argument("--num_inner_steps", type=int, default=10)
    p.add_argument("--early_stop_epsilon", type=float, default=1e-5)
    p.add_argument("--offsets", default="0,0,0,0", help="left,right,top,bottom pixels cropped before the square crop")
    p.add_argument("--image_size", type=int, default=1024, help="side the cropped image is resized to")
    p.add_argument("--vae_dtype", default=None, choices=sorted(GI.DTYPES), help="VAE storage type: default bf16")
    p.add_argument("--no_null_pooled", action="store_true",
                   help="optimise the unconditional sequence embedding only; the pooled one stays the encoder's")
    p.add_argument("--unfused", action="store_true", help="optimise through torch autograd instead of the fused step")
    p.add_argument("--verbose", action="store_true")
    p.add_argument("--device", default="0")
    return p


def main(argv=None):
    for path in edit(build_parser().parse_args(argv)):
        print(path)


if __name__ == "__main__":
    main()
