"""Edit a real image with a trained slider (demo_image_editing.ipynb): null-text inversion of the image, then the slider
sweep from the inverted latent with one optimised unconditional embedding per step.

    python -m sliders_conceptmod_amd.edit_image --image photo.jpg --prompt "photo of a person" \\
        --model_name out/age_slider.pt --pretrained_model /models/sd-1.4 --save_path edits --scales=0,2,4

Writes, under {save_path}/{name}/ (name = the LoRA file's stem): `reconstruction.png`, the VAE round trip of the cropped
image that the inversion starts from (the notebook's `image_enc`); {scale_str}/{image stem}.png for every slider scale,
with generate_images' folder naming (0.5 -> "half"); and the strip of all scales, all/{image stem}.png.

Differences from the notebook, on purpose: the UNet computes in 16-bit storage (fp16), not the notebook's fp32 -- the
embedding being optimised and its Adam state stay fp32; rank, alpha and the train method are read from the LoRA file, as
generate_images reads them, instead of being typed into a cell; the inversion runs before the adaptor is attached (the
notebook's network is attached but switched off there); the strip is a plain PIL image, not a matplotlib figure; `--image_size`
(default 512, the notebook's) is an argument.  SD-XL (`--base xl`) is refused: that is the command `edit_image_xl`."""
from __future__ import annotations

import argparse
import os
from typing import List, Tuple

import torch

from . import generate_images as GI
from . import model_util, train_util
from .null_inversion import NullInversion


def parse_offsets(text: str) -> Tuple[int, int, int, int]:
    """--offsets left,right,top,bottom (the notebook's load_512 arguments)"""
    parts = [int(p) for p in text.split(",") if p.strip() != ""]
    if len(parts) != 4 or min(parts) < 0:
        raise ValueError(f"--offsets wants four non-negative integers left,right,top,bottom, got '{text}'")
    return tuple(parts)


def output_paths(save_path: str, name: str, scales, image_path: str) -> Tuple[str, List[str], str]:
    """(reconstruction, one path per scale, strip)"""
    folder = os.path.join(save_path, name)
    stem = os.path.splitext(os.path.basename(image_path))[0]
    per_scale = [os.path.join(folder, GI.scale_str(s), f"{stem}.png") for s in scales]
    return os.path.join(folder, "reconstruction.png"), per_scale, os.path.join(folder, "all", f"{stem}.png")


def edit_base(args, xl: bool) -> List[str]:
    """The command's body for SD-1.x (`edit` below) and SD-XL (`edit_image_xl.edit`): the SD-XL run carries the pooled
    embedding and time_ids through the inversion and the sweep."""
    from PIL import Image
    device = torch.device(args.device if not str(args.device).isdigit() else f"cuda:{args.device}")
    if device.type != "cuda":
        raise ValueError("the product path has no CPU fallback: pass a cuda device")
    unet_dtype = torch.float16
    vae_dtype = GI.DTYPES[args.vae_dtype] if args.vae_dtype else (torch.bfloat16 if xl else torch.float16)
    tokenizers, text_encoders, unet, scheduler = model_util.load_models(args.pretrained_model, "ddim",
                                                                        weight_dtype=unet_dtype, xl=xl)
    unet = unet.to(device, unet_dtype).requires_grad_(False).eval()
    if isinstance(text_encoders, (list, tuple)):
        for te in text_encoders:
            te.to(device, unet_dtype)
    vae = model_util.load_vae(args.pretrained_model, xl=xl).to(device, vae_dtype)
    vae_dec = model_util.load_vae_decoder(args.pretrained_model, xl=xl).to(device, vae_dtype)
    inversion = dict(num_ddim_steps=args.ddim_steps, guidance_scale=args.guidance_scale, fused=not args.unfused,
                     image_size=args.image_size)
    invert = dict(offsets=parse_offsets(args.offsets), num_inner_steps=args.num_inner_steps,
                  early_stop_epsilon=args.early_stop_epsilon, verbose=args.verbose)
    sweep = {}
    if xl:
        from .null_inversion_xl import NullInversionXL
        from .train_lora_xl import encode_xl

        def encode_prompt(p):
            e = encode_xl(text_encoders, tokenizers, p, device, unet_dtype)
            return e.text_embeds, e.pooled_embeds

        inv = NullInversionXL(unet, scheduler, vae, vae_dec, encode_prompt, **inversion)
        (_image_gt, image_rec), x_t, unconds, pooleds = inv.invert(args.image, args.prompt, **invert,
                                                                   optimize_pooled=not args.no_null_pooled)
        sweep = dict(added_cond=(inv.pooled.to(unet_dtype), inv.time_ids.repeat(2, 1)), uncond_pooled_per_step=pooleds)
    else:
        from .train_lora import encode
        inv = NullInversion(unet, scheduler, vae, vae_dec, lambda p: encode(text_encoders, tokenizers, p, device, unet_dtype),
                            **inversion)
        (_image_gt, image_rec), x_t, unconds = inv.invert(args.image, args.prompt, **invert)
    network = GI.load_lora_network(unet, args.model_name, device)  # after the inversion: that runs without an adaptor
    scales = GI.parse_scales(args.scales)
    name = os.path.splitext(os.path.basename(args.model_name))[0]
    rec_path, per_scale, all_path = output_paths(args.save_path, name, scales, args.image)
    for p in [rec_path, all_path] + per_scale:
        os.makedirs(os.path.dirname(p), exist_ok=True)
    Image.fromarray(image_rec).save(rec_path)
    written = [rec_path]
    te = inv.context.to(unet_dtype)  # cat([uncond, cond]) of the prompt
    images = []
    for scale, path in zip(scales, per_scale):
        scheduler.set_timesteps(args.ddim_steps)
        lat = (x_t * scheduler.init_noise_sigma).float()
        lat = train_util.slider_sweep_latents(unet, network, scheduler, lat, te, scale, args.start_noise,
                                              args.guidance_scale, args.ddim_steps, uncond_per_step=unconds, **sweep)
        rgb = vae_dec.decode_to_uint8(lat.float() / vae_dec.config.scaling_factor).cpu().numpy()
        images.append(Image.fromarray(rgb[0]))
        images[-1].save(path)
        written.append(path)
    GI.strip(images).save(all_path)
    written.append(all_path)
    return written


def edit(args) -> List[str]:
    if args.base == "xl":
        raise ValueError("edit_image supports SD-1.x (--base 1.4); for an SD-XL slider use the command "
                         "python -m sliders_conceptmod_amd.edit_image_xl")
    return edit_base(args, False)


def build_parser_base(xl: bool):
    """The parser of `edit_image` (xl False) and of `edit_image_xl`"""
    p = argparse.ArgumentParser(
        prog="python -m sliders_conceptmod_amd.edit_image" + ("_xl" if xl else ""),
        description="Edit a real image with an SD-XL slider (null-text inversion) on the MI355X." if xl else
        "Edit a real image with a slider (demo_image_editing.ipynb) on the MI355X.")
    p.add_argument("--image", required=True, help="the photograph (any PIL-readable file)")
    p.add_argument("--prompt", required=True, help="a prompt that describes the image")
    p.add_argument("--model_name", required=True, help="LoRA file (.pt / .safetensors) written by the trainers")
    p.add_argument("--save_path", required=True, help="output folder")
    model = "sdxl" if xl else "sd1x"
    p.add_argument("--pretrained_model", default=f"synthetic://{model}",
                   help=f"local diffusers directory or synthetic://(tiny_){model}")
    if not xl:
        p.add_argument("--base", choices=["1.4", "xl"], default="1.4")
    p.add_argument("--scales", default="0,2,4", help="comma-separated; write --scales=-1,0,1 for negative values")
    p.add_argument("--start_noise", type=int, default=500,
                   help="the adaptor is off while t > start_noise (small values keep the identity)")
    p.add_argument("--ddim_steps", type=int, default=50)
    p.add_argument("--guidance_scale", type=float, default=7.5)
    p.add_argument("--num_inner_steps", type=int, default=10)
    p.add_argument("--early_stop_epsilon", type=float, default=1e-5)
    p.add_argument("--offsets", default="0,0,0,0", help="left,right,top,bottom pixels cropped before the square crop")
    p.add_argument("--image_size", type=int, default=1024 if xl else 512, help="side the cropped image is resized to")
    p.add_argument("--vae_dtype", default=None, choices=sorted(GI.DTYPES),
                   help="VAE storage type: default " + ("bf16" if xl else "fp16"))
    if xl:
        p.add_argument("--no_null_pooled", action="store_true",
                       help="optimise the unconditional sequence embedding only; the pooled one stays the encoder's")
    p.add_argument("--unfused", action="store_true", help="optimise through torch autograd instead of the fused step")
    p.add_argument("--verbose", action="store_true")
    p.add_argument("--device", default="0")
    return p


def build_parser():
    return build_parser_base(False)


def main(argv=None):
    for path in edit(build_parser().parse_args(argv)):
        print(path)


if __name__ == "__main__":
    main()


