"""Combine a UNet slider file and up to two text-encoder LoRA files into one safetensors file
(conceptmod/notrigger/combine_loras.py, cited as N).

    python -m sliders_conceptmod_amd.combine_loras unet.safetensors te1.safetensors te2.safetensors out.safetensors \
        [unet_strength] [enc_strength] [enc2_strength] [--t5]

The output is the union of the inputs' tensors.  A strength scales `lora_down` only; `alpha`, `dora_scale` and `lora_up` are
copied (N:48-60) -- the adaptor's delta is linear in lora_down, so the file acts at multiplier x strength.  Keys stay in the
`lora_unet_*` / `lora_te1_*` / `lora_te2_*` layout this project's loaders read (a '-' delimiter becomes '_', N:35).

--t5: the third file is a T5 tower's (train_notrigger --model FLUX.1 --clip_index 1 writes `lora_te2_encoder_block_*` keys);
its `lora_te2_` keys become `lora_te3_` (N:36-38), so that they sit next to a CLIP tower's `lora_te2_` keys without a clash.  A
file already written with `lora_te3_` (SD3-Medium --clip_index 2) passes as it is.  Without the flag nothing changes.

Deviations: the reference's other Flux rename (`lora_unet-` -> `transformer.`, `_down` / `_up` -> `_A` / `_B`, N:29-33) is not
built: this project's loaders read the `lora_unet_*` layout for every base.  An input may be '-' or '' to leave it out.  Only .safetensors is read: a pickled .bin is refused.  Two inputs holding the same key are an error."""
from __future__ import annotations

import argparse

PREFIXES = ("lora_unet_", "lora_te1_", "lora_te2_", "lora_te3_")


def read_tensors(path: str) -> dict:
    if not path.endswith(".safetensors"):
        raise ValueError(f"{path}: only .safetensors files are read (a pickled .bin is not loaded)")
    from safetensors.torch import load_file
    return load_file(path)


def merge(out: dict, tensors: dict, strength: float, prefix: str, what: str):
    """N:26-62 for one input.  prefix: what every key of this input must start with once '-' is '_'."""
    for k, v in tensors.items():
        k2 = k.replace("-", "_")
        if not k2.startswith(prefix):
            raise ValueError(f"{what}: key '{k}' does not start with '{prefix}'")
        if k2 in out:
            raise ValueError(f"{what}: key '{k2}' is already in the output")
        if "alpha" in k or "dora_scale" in k or "lora_up" in k:
            out[k2] = v.clone()
        elif "lora_down" in k:
            out[k2] = (strength * v.float()).to(v.dtype)
        else:
            raise ValueError(f"{what}: key '{k}' not supported (alpha, dora_scale, lora_down, lora_up)")


def as_te3(tensors: dict) -> dict:
    """N:36-38: a T5 file's `lora_te2_` keys under `lora_te3_` ('-' delimiters already count as '_'); `lora_te3_` keys stay."""
    out = {}
    for k, v in tensors.items():
        k2 = k.replace("-", "_")
        out[PREFIXES[3] + k2[len(PREFIXES[2]):] if k2.startswith(PREFIXES[2]) else k2] = v
    return out


def combine(unet_model, encoder1_model, encoder2_model, output_model, unet_strength=0.8, enc_strength=1.0, enc2_strength=1.0,
            t5: bool = False):
    from safetensors.torch import save_file
    out = {}
    for path, strength, prefix, what in ((unet_model, unet_strength, PREFIXES[0], "unet_model"),
                                         (encoder1_model, enc_strength, PREFIXES[1], "encoder1_model"),
                                         (encoder2_model, enc2_strength, PREFIXES[3 if t5 else 2], "encoder2_model")):
        if path and path != "-":
            tensors = read_tensors(path)
            merge(out, as_te3(tensors) if t5 and what == "encoder2_model" else tensors, strength, prefix, what)
    if not out:
        raise ValueError("nothing to combine: every input was left out")
    save_file(out, output_model)
    return out


def split_by_prefix(tensors: dict) -> dict:
    """{'lora_unet_': {...}, 'lora_te1_': {...}, 'lora_te2_': {...}, 'lora_te3_': {...}} of a combined file; a key under no
    prefix is an error."""
    parts = {p: {} for p in PREFIXES}
    for k, v in tensors.items():
        for p in PREFIXES:
            if k.startswith(p):
                parts[p][k] = v
                break
        else:
            raise ValueError(f"key '{k}' starts with none of {PREFIXES}")
    return parts


def build_parser():
    p = argparse.ArgumentParser(description="Merge a UNet slider and text-encoder LoRA files into one safetensors file.")
    p.add_argument("unet_model", type=str, help="the UNet slider file ('-': none)")
    p.add_argument("encoder1_model", type=str, help="the first text encoder's file, lora_te1_* ('-': none)")
    p.add_argument("encoder2_model", type=str, help="the second text encoder's file, lora_te2_* ('-': none)")
    p.add_argument("output_model", type=str, help="the merged output file")
    p.add_argument("unet_strength", type=float, nargs="?", default=0.8, help="strength of the UNet slider")
    p.add_argument("enc_strength", type=float, nargs="?", default=1.0, help="strength of the first text encoder's LoRA")
    p.add_argument("enc2_strength", type=float, nargs="?", default=1.0, help="strength of the second text encoder's LoRA")
    p.add_argument("--t5", action="store_true", help="the third file is a T5 tower's: its lora_te2_ keys become lora_te3_")
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    out = combine(a.unet_model, a.encoder1_model, a.encoder2_model, a.output_model, a.unet_strength, a.enc_strength, a.enc2_strength,
                  a.t5)
    print(f"{a.output_model}: {len(out)} tensors")


if __name__ == "__main__":
    main()
