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
taken.

The body and the parser are `edit_image`'s, called with xl=True."""
from __future__ import annotations

from typing import List

from .edit_image import build_parser_base, edit_base, output_paths, parse_offsets  # noqa: F401 (the helpers: this module's too)


def edit(args) -> List[str]:
    return edit_base(args, True)


def build_parser():
    return build_parser_base(True)


def main(argv=None):
    for path in edit(build_parser().parse_args(argv)):
        print(path)


if __name__ == "__main__":
    main()

