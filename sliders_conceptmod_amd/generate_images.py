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
figure.

Text-encoder LoRA files (`train_notrigger`, conceptmod/notrigger): `--te_model_name` takes them, repeated or as a comma list;
the tower a file belongs to is told by its key prefix (`lora_te1_` / `lora_te2_`).  A file written by `combine_loras` given as
`--model_name` is split by prefix into its UNet slider and its text-encoder parts.  Per scale the text-encoder adaptor runs
at multiplier = scale on every prompt the sweep encodes, conditional and unconditional; the steps with t > start_noise use
the un-adapted embeddings and the later steps the adapted ones -- the flip the UNet slider makes.  `--model_name` may be
left out: a text-encoder-only sweep.  On a `synthetic://` model the text front end is then a pair of seeded CLIP towers
(`train_notrigger.synthetic_towers`) instead of the hashed-embedding stand-in; `--synthetic_towers` asks for them without a
file (the images a text-encoder file at scale 0 must reproduce).

`--base sd3`: the sweep of an SD3 slider (conceptmod/textsliders/train_lora_sd3.py writes them) on the native MMDiT: per CSV
row and scale a CFG pair per sample through `train_util.predict_noise_sd3` steps of the flow-matching Euler schedule, the
slider off while t > start_noise and at `scale` below it; the 16-channel VAE decodes latents / scaling_factor + shift_factor.
Prompts are encoded as the pipeline does with text_encoder_3=None (`train_util.encode_prompts_sd3`, `--t5_tokens` zero rows).
Defaults: 28 steps, guidance 7.0, 1024 x 1024, bf16 decode, start_noise 750 on the 1000 sigma axis.  Further differences, on
purpose: the reference has no SD3 sweep script, so neither start_noise 750 nor guidance 7.0 comes from it (750 is the SD-XL
sweep's value carried over, 7.0 the published pipeline's default); whether the file adapts the context stream too
(add_q_proj ... to_add_out, which the reference's own LoRANetwork leaves out) is read from its keys; `--te_model_name` takes
a T5 tower's file only (next paragraph but one).

`--base flux`: the sweep of a Flux slider (conceptmod/textsliders/train_lora_flux.py writes them, keys `lora_unet-...`) on the
native Flux transformer, reusing the SD3 branch's helpers: ONE transformer pass per step and sample (no CFG pair) through
`train_util.predict_noise_flux`; a guidance_embeds model (FLUX.1-dev) takes `--guidance_scale` (default 3.5) as its embedded
guidance and FLUX.1-schnell ignores it; the 16-channel VAE decodes latents / scaling_factor + shift_factor of its config.
Prompts: CLIP-L's pooled row and the T5 sequence (`model_util.load_models_flux`; `--t5_backend native`: the T5 tower on the
HIP engine instead of transformers', and with `--base sd3` text_encoder_3 as a third tower; `--no_t5`, or a directory without
text_encoder_2: `--t5_tokens` zero rows).  Defaults, by the scheduler's config: 4 steps and 256 tokens without dynamic
shifting (schnell), 28 steps and 512 tokens with it (dev); the slider is on where 1000 sigma <= `--start_noise` (750).
These defaults are ours: the reference has no Flux sweep script (the step and token counts are the published pipelines',
750 the SD-XL sweep's value carried over).  DoRA files are refused with `--base flux`.

`--base flux|sd3 --t5_backend native --te_model_name f`: f is a T5 tower's LoRA file (`train_notrigger --model FLUX.1
--clip_index 1` / `--model SD3-Medium --clip_index 2`: keys `lora_te2_encoder_block_*` or `lora_te3_encoder_block_*`); it may
also be the T5 part of a `combine_loras --t5` file given as `--model_name`.  Per scale the adaptor runs on the native T5 tower
at multiplier = scale on the prompt (SD3: on the negative prompt too), and the adapted context replaces the frozen one on
the steps where the transformer slider is on (1000 sigma <= `--start_noise`), as the SD-XL sweep does with CLIP files; scale 0
gives the bits of a run without the file.  The tower's prompt cache holds frozen rows only and is bypassed under the adaptor.
Without `--t5_backend native`, with `--synthetic_towers`, or with a CLIP tower's keys the call is refused by a ValueError
that names `--te_model_name`: CLIP text-encoder sweeps are not built for these two bases."""
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
    delim = file_delimiter(names)
    ctx_stream = has_context_stream(names)  # an SD3 / Flux file with the context stream's sites
    for target_replace in (LM.DEFAULT_TARGET_REPLACE, LM.DEFAULT_TARGET_REPLACE + LM.UNET_TARGET_REPLACE_MODULE_CONV):
        for method in TRAIN_METHODS:
            got = {t[0] for t in LM.select_targets(unet, method, target_replace, LM.LORA_PREFIX_UNET, delim,
                                                   context_stream=ctx_stream)}
            if got == names:
                return ranks.pop(), alpha, method, list(target_replace)
    raise ValueError("the LoRA file's layers match no train method of this UNet (wrong --base or --pretrained_model?)")


def file_delimiter(keys) -> str:
    """'-' for a file of the reference's Flux trainer (keys `lora_unet-transformer_blocks-0-attn-to_q...`), else '_'."""
    return "-" if any(k.startswith(LM.LORA_PREFIX_UNET + "-") for k in keys) else "_"


def has_context_stream(keys) -> bool:
    return any(f"{d}attn{d}add_" in k or f"{d}attn{d}to_add_out" in k for k in keys for d in "_-")


def load_lora_network(unet, path: str, device):
    return lora_network_from_state(unet, load_lora_state(path), device)


TE_PREFIXES = ("lora_te1_", "lora_te2_")


def parse_te_names(values) -> List[str]:
    """--te_model_name, repeated and / or comma lists -> file names."""
    return [p.strip() for v in (values or []) for p in v.split(",") if p.strip()]


def te_tower_of(state: Dict[str, torch.Tensor], what: str) -> int:
    """The tower (0 / 1) a text-encoder LoRA state belongs to: every key carries the one prefix."""
    towers = {i for k in state for i, p in enumerate(TE_PREFIXES) if k.startswith(p)}
    if len(towers) != 1 or not all(k.startswith(TE_PREFIXES) for k in state):
        raise ValueError(f"{what}: a text-encoder LoRA file holds keys of exactly one of {TE_PREFIXES}")
    return towers.pop()


def te_network_from_state(text_encoder, state: Dict[str, torch.Tensor], tower: int, device, target_replace=None,
                          prefix: Optional[str] = None):
    """The LoRANetwork of a text-encoder file on its tower (rank and alpha read from the file), adaptor off.  target_replace /
    prefix: a T5 tower's (t5_network_from_state); by default a CLIP tower's, the prefix told by `tower`."""
    downs = [v for k, v in state.items() if k.endswith(".lora_down.weight")]
    ranks = {int(v.shape[0]) for v in downs}
    alphas = {float(v) for k, v in state.items() if k.endswith(".alpha")}
    if len(ranks) != 1 or len(alphas) > 1:
        raise ValueError(f"text-encoder LoRA file mixes ranks {sorted(ranks)} or alphas {sorted(alphas)}")
    rank = ranks.pop()
    net = LM.LoRANetwork(text_encoder, rank=rank, multiplier=1.0, alpha=alphas.pop() if alphas else float(rank),
                         target_replace=target_replace or LM.CLIP_TARGET_REPLACE,
                         prefix=prefix or TE_PREFIXES[tower][:-1], train_method="full").to(device)
    net.load_state_dict(state)  # strict: the file's layers must be this tower's
    net.__exit__(None, None, None)  # multiplier 0 outside `with net:`
    return net


T5_TE_PREFIXES = ("lora_te2_", "lora_te3_")  # train_notrigger on FLUX.1 --clip_index 1 / SD3-Medium --clip_index 2, combine_loras --t5


def t5_sweep_states(args, base: str):
    """`--base flux|sd3`: (the transformer slider's state or None, the T5 tower's LoRA state or None, its key prefix).
    The T5 state comes from --te_model_name (one file of train_notrigger's on a T5 tower: keys lora_te2_encoder_block_* or
    lora_te3_encoder_block_*) or is the T5 part of a combine_loras file given as --model_name.  It needs --t5_backend native;
    without it, with --synthetic_towers, or with a CLIP tower's keys (*_text_model_*) the call is refused before any
    model is loaded."""
    names = parse_te_names(args.te_model_name)
    if args.synthetic_towers or (names and args.t5_backend != "native"):
        raise ValueError(f"--base {base} takes no --synthetic_towers, and --te_model_name only with --t5_backend native (a T5 "
                         f"tower's LoRA file, train_notrigger --clip_index {1 if base == 'flux' else 2}): CLIP text-encoder "
                         f"LoRA sweeps are not built for {'Flux' if base == 'flux' else 'SD3'}")
    if len(names) > 1:
        raise ValueError(f"--base {base}: one --te_model_name file (the T5 tower's), got {len(names)}")
    slider = load_lora_state(args.model_name) if args.model_name else None
    t5_state = None
    if slider is not None and any(k.startswith("lora_te") for k in slider):
        from .combine_loras import PREFIXES, split_by_prefix
        parts = split_by_prefix(slider)
        slider = parts[PREFIXES[0]] or None
        t5_state = {**parts[PREFIXES[2]], **parts[PREFIXES[3]]}
        if parts[PREFIXES[1]] or args.t5_backend != "native":
            raise ValueError(f"--base {base}: {args.model_name} holds text-encoder keys; only a T5 tower's part is swept, with "
                             f"--t5_backend native (as --te_model_name)")
    if names:
        if t5_state:
            raise ValueError(f"--te_model_name {names[0]}: {args.model_name} already holds a T5 tower's LoRA")
        t5_state = load_lora_state(names[0])
    if not t5_state:
        return slider, None, None
    what = names[0] if names else args.model_name
    prefixes = {p for k in t5_state for p in T5_TE_PREFIXES if k.startswith(p + "encoder_block_")}
    if len(prefixes) != 1 or not all(k.startswith(tuple(p + "encoder_block_" for p in prefixes)) for k in t5_state):
        raise ValueError(f"--te_model_name {what}: not a T5 tower's LoRA file (keys lora_te2_encoder_block_* or "
                         f"lora_te3_encoder_block_*; a CLIP tower's *_text_model_* keys are not swept on --base {base})")
    return slider, t5_state, prefixes.pop()[:-1]


def t5_network_from_state(tower, state: Dict[str, torch.Tensor], prefix: str, device):
    """The LoRANetwork of a T5 LoRA file on model_util.NativeT5Tower's model, adaptor off."""
    if tower is None or not hasattr(tower, "model"):
        raise ValueError("--te_model_name: the model has no native T5 tower to adapt (--no_t5, or no text_encoder directory)")
    return te_network_from_state(tower.model, state, 0, device, LM.T5_TARGET_REPLACE, prefix)


def lora_network_from_state(unet, state: Dict[str, torch.Tensor], device):
    rank, alpha, method, target_replace = lora_file_params(state, unet)
    net = LM.LoRANetwork(unet, rank=rank, multiplier=1.0, alpha=alpha, train_method=method, delimiter=file_delimiter(state),
                         target_replace=target_replace, context_stream=has_context_stream(state)).to(device)
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


def generate_sd3(args) -> List[str]:
    """`--base sd3` (module docstring)."""
    from PIL import Image
    fill_defaults(args)  # (idempotent: a caller that parsed and came here directly gets --t5_tokens 256 and the rest too)
    if args.synthetic_towers or (parse_te_names(args.te_model_name) and args.t5_backend != "native"):
        t5_sweep_states(args, "sd3")  # (raises: the refusal needs no file)
    if not args.model_name and not parse_te_names(args.te_model_name):
        raise ValueError("--base sd3 needs --model_name (an SD3 slider file)")
    if args.scheduler is not None:
        raise ValueError("--base sd3 samples with the flow-matching Euler schedule only (leave --scheduler out)")
    device = torch.device(args.device if not str(args.device).isdigit() else f"cuda:{args.device}")
    if device.type != "cuda":
        raise ValueError("the product path has no CPU fallback: pass a cuda device")
    dtype = torch.float16
    vae_dtype = DTYPES[args.vae_dtype] if args.vae_dtype else torch.bfloat16
    start_noise = args.start_noise if args.start_noise is not None else 750
    if args.t5_backend == "torch":
        raise ValueError("--base sd3 --t5_backend torch is not built: leave it out (zero rows stand in for T5) or pass native")
    tokenizers, text_encoders, transformer, scheduler = model_util.load_models_sd3(args.pretrained_model, weight_dtype=dtype,
                                                                                   t5_backend=args.t5_backend)
    transformer = transformer.to(device, dtype).requires_grad_(False).eval()
    for te in text_encoders:
        te.to(device, dtype)
    slider_state, t5_state, t5_prefix = t5_sweep_states(args, "sd3")
    network = None
    if slider_state is not None:
        network = lora_network_from_state(transformer, slider_state, device)
        if args.rank is not None and args.rank != network.lora_dim:
            raise ValueError(f"--rank {args.rank} but the LoRA file has rank {network.lora_dim}")
        network.__exit__(None, None, None)  # the sweep sets the multiplier per step
    t5_net = (t5_network_from_state(text_encoders[2] if len(text_encoders) > 2 else None, t5_state, t5_prefix, device)
              if t5_state else None)
    vae = model_util.load_vae_decoder_sd3(args.pretrained_model).to(device, vae_dtype)
    scales = parse_scales(args.scales)
    name = os.path.splitext(os.path.basename(args.model_name or parse_te_names(args.te_model_name)[0]))[0]
    folder = os.path.join(args.save_path, name)
    for d in [scale_str(s) for s in scales] + ["all"]:
        os.makedirs(os.path.join(folder, d), exist_ok=True)
    h = w = args.image_size
    jd = transformer.cfg.joint_attention_dim
    written = []
    for row in read_prompts(args.prompts_path):
        case = row["case_number"]
        if not (args.from_case <= case <= args.till_case):
            continue
        c, cp = train_util.encode_prompts_sd3(None, tokenizers, text_encoders, row["prompt"], 1, args.t5_tokens, jd)
        u, up = train_util.encode_prompts_sd3(None, tokenizers, text_encoders, args.negative_prompts or "", 1, args.t5_tokens, jd)
        te = train_util.concat_embeddings_sd3(u, c, args.num_samples)
        pooled = train_util.concat_embeddings_sd3(up, cp, args.num_samples)
        images = []
        for scale in scales:
            scheduler.set_timesteps(args.ddim_steps)
            lat = train_util.get_initial_latents_sd3(scheduler, args.num_samples, h, w, 1,
                                                     generator=torch.manual_seed(row["evaluation_seed"])).to(device)
            te_on = None
            if t5_net is not None:  # the T5 tower's LoRA at multiplier = scale, on the prompt and on the negative prompt
                t5_net.set_lora_slider(scale)
                with t5_net:
                    c_on, _ = train_util.encode_prompts_sd3(None, tokenizers, text_encoders, row["prompt"], 1, args.t5_tokens, jd)
                    u_on, _ = train_util.encode_prompts_sd3(None, tokenizers, text_encoders, args.negative_prompts or "", 1,
                                                            args.t5_tokens, jd)
                te_on = train_util.concat_embeddings_sd3(u_on, c_on, args.num_samples)
            lat = train_util.slider_sweep_latents_sd3(transformer, network, scheduler, lat, te, pooled, scale, start_noise,
                                                      args.guidance_scale, adapted_embeddings=te_on)
            z = lat.float() / vae.config.scaling_factor + vae.config.shift_factor
            rgb = vae.decode_to_uint8(z).cpu().numpy()
            images.append([Image.fromarray(rgb[i]) for i in range(rgb.shape[0])])
        for num in range(args.num_samples):
            per_scale, all_path = output_paths(args.save_path, name, scales, case, num)
            for i, p in enumerate(per_scale):
                images[i][num].save(p)
                written.append(p)
            strip([images[i][num] for i in range(len(scales))]).save(all_path)
            written.append(all_path)
    return written


def generate_flux(args) -> List[str]:
    """`--base flux` (module docstring)."""
    from PIL import Image
    if args.scheduler is not None:
        raise ValueError("--base flux samples with the flow-matching Euler schedule only (leave --scheduler out)")
    # no file: the frozen network, in folder `frozen`; a T5 tower's LoRA from --te_model_name or a combine_loras file
    state, t5_state, t5_prefix = t5_sweep_states(args, "flux")
    if state is not None and any("dora_scale" in k for k in state):
        raise ValueError("--base flux: DoRA files are not built for Flux (the engine takes plain LoRA sites only)")
    device = torch.device(args.device if not str(args.device).isdigit() else f"cuda:{args.device}")
    if device.type != "cuda":
        raise ValueError("the product path has no CPU fallback: pass a cuda device")
    dtype = torch.bfloat16  # (the published Flux weights are bf16)
    vae_dtype = DTYPES[args.vae_dtype] if args.vae_dtype else torch.bfloat16
    start_noise = args.start_noise if args.start_noise is not None else 750
    tokenizers, text_encoders, transformer, scheduler = model_util.load_models_flux(args.pretrained_model, weight_dtype=dtype,
                                                                                    no_t5=args.no_t5,
                                                                                    t5_backend=args.t5_backend or "torch")
    dev_like = scheduler.use_dynamic_shifting
    steps = args.ddim_steps if args.ddim_steps is not None else (28 if dev_like else 4)
    tokens = args.t5_tokens if args.t5_tokens is not None else (512 if dev_like else 256)
    guidance = args.guidance_scale if args.guidance_scale is not None else 3.5
    transformer = transformer.to(device, dtype).requires_grad_(False).eval()
    for te in text_encoders:
        if te is not None:
            te.to(device, dtype)
    network = None
    if state is not None:
        network = lora_network_from_state(transformer, state, device)
        if args.rank is not None and args.rank != network.lora_dim:
            raise ValueError(f"--rank {args.rank} but the LoRA file has rank {network.lora_dim}")
        network.__exit__(None, None, None)  # the sweep sets the multiplier per step
    t5_net = t5_network_from_state(text_encoders[1], t5_state, t5_prefix, device) if t5_state else None
    vae = model_util.load_vae_decoder_sd3(args.pretrained_model).to(device, vae_dtype)
    scales = parse_scales(args.scales)
    named = args.model_name or (parse_te_names(args.te_model_name) or [None])[0]
    name = os.path.splitext(os.path.basename(named))[0] if named else "frozen"
    folder = os.path.join(args.save_path, name)
    for d in [scale_str(s) for s in scales] + ["all"]:
        os.makedirs(os.path.join(folder, d), exist_ok=True)
    h = w = args.image_size
    jd = transformer.cfg.joint_attention_dim
    written = []
    for row in read_prompts(args.prompts_path):
        case = row["case_number"]
        if not (args.from_case <= case <= args.till_case):
            continue
        te, pooled = train_util.encode_prompts_flux(None, tokenizers, text_encoders, row["prompt"], args.num_samples, tokens, jd)
        images = []
        for scale in scales:
            lat = train_util.get_initial_latents_flux(scheduler, args.num_samples, h, w, 1,
                                                      generator=torch.manual_seed(row["evaluation_seed"])).to(device)
            te_on = None
            if t5_net is not None:  # the T5 tower's LoRA at multiplier = scale, switched on where the slider is
                t5_net.set_lora_slider(scale)
                with t5_net:
                    te_on, _ = train_util.encode_prompts_flux(None, tokenizers, text_encoders, row["prompt"], args.num_samples,
                                                              tokens, jd)
            lat = train_util.slider_sweep_latents_flux(transformer, network, scheduler, lat, te, pooled, scale, start_noise,
                                                       guidance, steps, adapted_embeddings=te_on)
            z = lat.float() / vae.config.scaling_factor + vae.config.shift_factor
            rgb = vae.decode_to_uint8(z).cpu().numpy()
            images.append([Image.fromarray(rgb[i]) for i in range(rgb.shape[0])])
        for num in range(args.num_samples):
            per_scale, all_path = output_paths(args.save_path, name, scales, case, num)
            for i, p in enumerate(per_scale):
                images[i][num].save(p)
                written.append(p)
            strip([images[i][num] for i in range(len(scales))]).save(all_path)
            written.append(all_path)
    return written


def generate(args) -> List[str]:
    from PIL import Image
    fill_defaults(args)
    if args.base == "flux":
        return generate_flux(args)
    if args.base == "sd3":
        return generate_sd3(args)
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
    # ---- the adaptor files: a UNet slider, text-encoder files, or a combined file split by prefix
    te_states: Dict[int, Dict[str, torch.Tensor]] = {}
    unet_state = None
    if args.model_name:
        unet_state = load_lora_state(args.model_name)
        if any(k.startswith("lora_te") for k in unet_state):
            from .combine_loras import PREFIXES, split_by_prefix
            parts = split_by_prefix(unet_state)
            if parts[PREFIXES[3]]:
                raise ValueError(f"{args.model_name}: holds a T5 tower's LoRA ({PREFIXES[3]}*, combine_loras --t5): sweep it "
                                 f"with --base flux | sd3 --t5_backend native; --base {args.base} has no T5 tower")
            unet_state = parts[PREFIXES[0]] or None
            for i, p in enumerate(TE_PREFIXES):
                if parts[p]:
                    te_states[i] = parts[p]
    for path in parse_te_names(args.te_model_name):
        state = load_lora_state(path)
        tower = te_tower_of(state, path)
        if tower in te_states:
            raise ValueError(f"{path}: text encoder {tower + 1} already has a LoRA ({TE_PREFIXES[tower]}*)")
        te_states[tower] = state
    if unet_state is None and not te_states:
        raise ValueError("nothing to sweep: give --model_name, --te_model_name or both")
    if (te_states or args.synthetic_towers) and isinstance(text_encoders, model_util.SyntheticTextEncoder):
        from .train_notrigger import synthetic_towers
        tokenizers, text_encoders = synthetic_towers(args.pretrained_model[len("synthetic://"):])
        width = sum(te.config.hidden_size for te in text_encoders)
        if width != unet.cfg.cross_attention_dim:
            raise ValueError(f"{args.pretrained_model}: the synthetic text towers are {width} wide, the UNet's context "
                             f"{unet.cfg.cross_attention_dim}: no text-encoder sweep on this model")
        for te in text_encoders:
            te.to(device, unet_dtype)
    te_networks = []
    for tower, state in sorted(te_states.items()):
        if not isinstance(text_encoders, (list, tuple)) or tower >= len(text_encoders):
            raise ValueError(f"{TE_PREFIXES[tower]}* keys, but the model has no text encoder {tower + 1}")
        te_networks.append(te_network_from_state(text_encoders[tower], state, tower, device))
    network = lora_network_from_state(unet, unet_state, device) if unet_state is not None else None
    if network is not None and args.rank is not None and args.rank != network.lora_dim:
        raise ValueError(f"--rank {args.rank} but the LoRA file has rank {network.lora_dim}")
    vae = model_util.load_vae_decoder(args.pretrained_model, xl=xl).to(device, vae_dtype)
    factor = 2 ** (len(vae.config.block_out_channels) - 1)
    scales = parse_scales(args.scales)
    name = os.path.splitext(os.path.basename(args.model_name or parse_te_names(args.te_model_name)[0]))[0]

    def conditioning(prompt, scale):
        """The prompt pair's embeddings; scale None: the un-adapted towers, else every text-encoder adaptor at `scale`."""
        import contextlib
        with contextlib.ExitStack() as stack:
            for net in (te_networks if scale is not None else []):
                net.set_lora_slider(scale)
                stack.enter_context(net)
            return prompt_conditioning(text_encoders, tokenizers, prompt, args.negative_prompts, args.num_samples, xl, h, w,
                                       device, unet_dtype)

    folder = os.path.join(args.save_path, name)
    for d in [scale_str(s) for s in scales] + ["all"]:
        os.makedirs(os.path.join(folder, d), exist_ok=True)
    h = w = args.image_size
    written = []
    for row in read_prompts(args.prompts_path):
        case = row["case_number"]
        if not (args.from_case <= case <= args.till_case):
            continue
        te, added = conditioning(row["prompt"], None)
        images = []  # [scale][num] -> PIL
        for scale in scales:
            scheduler.set_timesteps(args.ddim_steps)
            lat = initial_latents(row["evaluation_seed"], args.num_samples, h, w, scheduler,
                                  vae.config.latent_channels, factor).to(device)
            te_on, added_on = conditioning(row["prompt"], scale) if te_networks else (None, None)
            lat = train_util.slider_sweep_latents(unet, network, scheduler, lat, te, scale, start_noise,
                                                  args.guidance_scale, args.ddim_steps, added_cond=added,
                                                  adapted_embeddings=te_on, adapted_added_cond=added_on)
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
    p.add_argument("--model_name", default=None, help="LoRA file (.pt / .safetensors) written by the trainers, or a file "
                   "written by combine_loras (split by key prefix); may be left out with --te_model_name")
    p.add_argument("--te_model_name", action="append", default=None,
                   help="text-encoder LoRA file(s) written by train_notrigger: repeat the flag or join with commas; the "
                        "tower is told by the key prefix (lora_te1_ / lora_te2_); --base flux|sd3 --t5_backend native: one file "
                        "of a T5 tower (lora_te2_encoder_block_* / lora_te3_encoder_block_*)")
    p.add_argument("--synthetic_towers", action="store_true",
                   help="synthetic:// models: seeded CLIP towers as the text front end (implied by a text-encoder file)")
    p.add_argument("--prompts_path", required=True, help="CSV with prompt, evaluation_seed, case_number")
    p.add_argument("--save_path", required=True, help="output folder")
    p.add_argument("--pretrained_model", default="synthetic://sd1x",
                   help="local diffusers directory or synthetic://(tiny_)sd1x | sdxl")
    p.add_argument("--negative_prompts", default=None, help="negative prompt (default: the empty prompt)")
    p.add_argument("--base", choices=["1.4", "xl", "sd3", "flux"], default="1.4")
    p.add_argument("--guidance_scale", type=float, default=None,
                   help="default 7.5 (SD-1.x, SD-XL) / 7.0 (SD3) / 3.5, embedded, for a Flux model with guidance_embeds")
    p.add_argument("--t5_tokens", type=int, default=None, help="--base sd3: zero rows that stand in for the T5 block of the "
                   "context (default 256: the published pipeline's max_sequence_length; 77: its first release); --base flux: "
                   "the T5 sequence length (default 256 schnell / 512 dev), zero rows without a T5 tower")
    p.add_argument("--no_t5", action="store_true", help="--base flux: do not load text_encoder_2 (zero rows stand in)")
    p.add_argument("--t5_backend", choices=["torch", "native"], default=None,
                   help="--base flux: the T5 tower as transformers runs it (torch, the default) or on the HIP engine (native); "
                        "--base sd3: native loads text_encoder_3 on the HIP engine (default: none, zero rows stand in)")
    p.add_argument("--image_size", type=int, default=None, help="default 512 (SD-1.x) / 1024 (SD-XL)")
    p.add_argument("--from_case", type=int, default=0)
    p.add_argument("--till_case", type=int, default=1000000)
    p.add_argument("--num_samples", type=int, default=5)
    p.add_argument("--ddim_steps", type=int, default=None, help="default 50 (SD-1.x, SD-XL) / 28 (SD3)")
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


def fill_defaults(args):
    """The defaults that depend on --base."""
    if args.image_size is None:
        args.image_size = 512 if args.base == "1.4" else 1024
    if args.base == "flux":  # steps, tokens and guidance follow the scheduler's config (generate_flux)
        return args
    if args.guidance_scale is None:
        args.guidance_scale = 7.0 if args.base == "sd3" else 7.5
    if args.ddim_steps is None:
        args.ddim_steps = 28 if args.base == "sd3" else 50
    if args.t5_tokens is None:
        args.t5_tokens = 256
    return args


def main(argv=None):
    args = fill_defaults(build_parser().parse_args(argv))
    for path in generate(args):
        print(path)


if __name__ == "__main__":
    main()
