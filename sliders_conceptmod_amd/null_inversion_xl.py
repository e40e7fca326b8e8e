"""Null-text inversion of a real image on an SD-XL UNet: the methods of `null_inversion.NullInversion`
(demo_image_editing.ipynb, class NullInversion) by name, with SD-XL's added conditioning carried through every UNet call.

SD-XL's unconditional conditioning has two parts: the sequence embedding [1, 77, D] and the pooled embedding `text_embeds`
[1, P], which enters every resnet through the time embedding.  `null_optimization(..., optimize_pooled=True)` optimises
both (one Adam over the two tensors); with `optimize_pooled=False` only the sequence embedding, as the notebook does for
SD-1.4, and the pooled entries returned are the encoder's, unchanged.  `time_ids` are
`train_util.get_add_time_ids(image_size, image_size)` and take no gradient.  The notebook is SD-1.4 only: this route and the
pooled optimisation are this package's additions.

`fused=True` (default): one flat fp32 parameter [77 D + P] ([77 D] with the pooled optimisation off); an inner step is the
casts of its parts to the UNet's dtype (smi_op_cast_f32), one saving smi_unet_forward on the one unconditional sample,
smi_nulltext_loss, smi_unet_backward_cond (smi_unet_backward_ctx with the pooled optimisation off) writing into the flat
gradient, one smi_clip_adamw over the flat buffer with weight_decay 0 and no clipping (Adam is element-wise: this equals one
torch.optim.Adam over the two tensors) and one scalar read for the early stop; every buffer is allocated before the loop.
`fused=False` is the notebook's loop with torch autograd through the product UNet's seam."""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import torch

from . import train_util
from .null_inversion import NullInversion


class NullInversionXL(NullInversion):
    """unet: the product SD-XL UNet2DConditionModel on a cuda device; scheduler: a DDIM scheduler of this package; vae /
    vae_decoder: the AutoencoderKL encoder and decoder (only `invert`, `image2latent`, `latent2image` need them);
    encode_prompt(str) -> (embeds [1, L, D], pooled [1, P]) (only `invert` / `init_prompt` need it).

    The loops are NullInversion's: this class sets `pooled` and `time_ids`, which they carry through every UNet call, and
    gives the public methods their pooled argument."""

    ADDED_COND = True

    def __init__(self, unet, scheduler, vae=None, vae_decoder=None, encode_prompt: Optional[Callable] = None,
                 num_ddim_steps: int = 50, guidance_scale: float = 7.5, fused: bool = True, image_size: int = 1024):
        super().__init__(unet, scheduler, vae, vae_decoder, encode_prompt, num_ddim_steps, guidance_scale, fused, image_size)
        self.time_ids = train_util.get_add_time_ids(image_size, image_size, dtype=torch.float32).to(unet.device)  # [1, 6]

    def get_noise_pred_single(self, latents, t, context, pooled):
        return self._eps(latents, t, context, pooled)

    def get_noise_pred(self, latents, t, is_forward=True, context=None, pooled=None):
        return self._guided_step(latents, t, is_forward, context, pooled)

    @torch.no_grad()
    def init_prompt(self, prompt: str):
        (uncond, pooled_u), (cond, pooled_c) = self.encode_prompt(""), self.encode_prompt(prompt)
        self.context = torch.cat([uncond, cond]).to(self.unet.device)
        self.pooled = torch.cat([pooled_u, pooled_c]).to(self.unet.device)
        self.prompt = prompt

    def null_optimization(self, latents: Sequence[torch.Tensor], num_inner_steps: int = 10, epsilon: float = 1e-5,
                          optimize_pooled: bool = True):
        """(uncond_embeddings_list, uncond_pooled_list): one [1, L, D] and one [1, P] per DDIM step."""
        return self._null_optimization(latents, num_inner_steps, epsilon, bool(optimize_pooled))

    def invert(self, image_path, prompt: str, offsets=(0, 0, 0, 0), num_inner_steps: int = 10,
               early_stop_epsilon: float = 1e-5, verbose: bool = False, optimize_pooled: bool = True):
        """((image, reconstruction), x_T, [unconditional embedding per step], [unconditional pooled embedding per step])"""
        images, ddim_latents = self._ddim_invert(image_path, prompt, offsets, verbose)
        unconds, pooleds = self.null_optimization(ddim_latents, num_inner_steps, early_stop_epsilon, optimize_pooled)
        return images, ddim_latents[-1], unconds, pooleds
